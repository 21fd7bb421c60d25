"""AES-128 transciphering: the clear model against the published vectors, the scheduled program on clear bits (S-box,
rounds, key-schedule step, value and noise bounds at three bases), the gate-sum kernel word for word, S-box passes, the
counter addition, single rounds, whole calls against FIPS-197 and SP 800-38A, other keys and bases, sharding over a stream
set, the device against the host emulation, and the refusals.

The checker is the pure-Python AES-128 below (the specification's table-free S-box by inversion in GF(2^8)); nothing of it
reads the library's tables or its gate list.  tests/golden/aes_vectors.json holds the published vectors.
tests/aes_program.py parses the program a scratch dumps (hip_test_aes_program) and runs it in NumPy.
[emu] runs the kernel sources on the host, [hip] on the MI355X, both on toy keys; one test runs PARAM_MESSAGE_2_CARRY_2.
Whole calls are 14,873 bootstraps per input and 4,280 per key schedule: they run on [hip] only."""
import ctypes as C
import dataclasses
import gc
import json
import os
import signal
import textwrap

import numpy as np
import pytest

from . import aes_program as ap
from .common import Params
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_bases import BASES, Ctx

U64 = np.uint64
BASE = {b.name: b for b in BASES}
VECTORS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aes_vectors.json")))

# the emulation runs a fibre per lane: it takes the smallest polynomial that holds the plaintext space
SMALL_4_4 = Params("toy_k1_N512_l1_p16", 8, 1, 512, 23, 1, 4, 4, 45, 17, 16, ms_type=1)
SMALL_8_8 = Params("toy_k1_N1024_l1_p64", 8, 1, 1024, 23, 1, 4, 4, 45, 17, 64, ms_type=1)

KINDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]

# pinned from docs/history/aes_log.md, at message / carry moduli (4, 4): bootstraps per input and rounds of aes_encrypt at
# S-box parallelism 16 (441 + 10 * 1,200 + 9 * 256 + 128; 9 + 10 * 13 + 9 * 2 + 1), bootstraps and rounds of key_expansion
# (10 * (300 + 128); 10 * (13 + 1)), and the rounds of one S-box pass
AES_PBS_PER_INPUT, AES_ROUNDS_P16, KEY_PBS, KEY_ROUNDS, SBOX_ROUNDS, SBOX_PBS_PER_LANE = 14873, 158, 4280, 140, 13, 75


# ================================================================================== the clear model
def gf_mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11B
        b >>= 1
    return r


def _sbox():
    inv = [0] + [next(b for b in range(1, 256) if gf_mul(a, b) == 1) for a in range(1, 256)]
    out = []
    for a in range(256):
        x = inv[a]
        y = x
        for i in range(1, 5):
            y ^= ((x << i) | (x >> (8 - i))) & 0xFF
        out.append(y ^ 0x63)
    return out


SBOX = _sbox()
RCON = [0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36]


def expand_key(key):
    """16 key bytes -> 11 round keys of 16 bytes"""
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= RCON[i // 4 - 1]
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]


def sub_shift(state):
    s = [SBOX[b] for b in state]
    return [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]


def mix_columns(state):
    out = []
    for c in range(4):
        a = state[4 * c:4 * c + 4]
        out += [gf_mul(a[r], 2) ^ gf_mul(a[(r + 1) % 4], 3) ^ a[(r + 2) % 4] ^ a[(r + 3) % 4] for r in range(4)]
    return out


def middle_round(state, rk):
    return [a ^ b for a, b in zip(mix_columns(sub_shift(state)), rk)]


def last_round(state, rk):
    return [a ^ b for a, b in zip(sub_shift(state), rk)]


def encrypt_block(block, rks):
    s = [a ^ b for a, b in zip(block, rks[0])]
    for r in range(1, 10):
        s = middle_round(s, rks[r])
    return last_round(s, rks[10])


def to_bytes(x):
    return list(int(x).to_bytes(16, "big"))


def from_bytes(b):
    return int.from_bytes(bytes(b), "big")


def ctr_block(key, iv, counter):
    return from_bytes(encrypt_block(to_bytes((iv + counter) % (1 << 128)), expand_key(to_bytes(key))))


def bits_of_bytes(b):
    """16 bytes -> 128 bits, block order (most significant bit of byte 0 first)"""
    return [(x >> (7 - j)) & 1 for x in b for j in range(8)]


def bytes_of_bits(bits):
    return [sum(int(bits[8 * i + j]) << (7 - j) for j in range(8)) for i in range(len(bits) // 8)]


KEY = int(VECTORS["sp800_38a_f51"]["key"], 16)
IV = int(VECTORS["sp800_38a_f51"]["counter_block"], 16)


# ================================================================================== 1. the model against the vectors
def test_clear_model_reproduces_the_published_vectors():
    a1 = VECTORS["fips197_a1"]
    rks = expand_key(to_bytes(int(a1["key"], 16)))
    words = ["%08x" % int.from_bytes(bytes(rk[4 * i:4 * i + 4]), "big") for rk in rks for i in range(4)]
    assert len(a1["words"]) == 44 and words == a1["words"]
    for v in VECTORS["fips197_blocks"]:
        got = encrypt_block(to_bytes(int(v["plaintext"], 16)), expand_key(to_bytes(int(v["key"], 16))))
        assert "%032x" % from_bytes(got) == v["ciphertext"], v["name"]
    f51 = VECTORS["sp800_38a_f51"]
    assert ["%032x" % ctr_block(KEY, IV, n) for n in range(2)] == f51["encrypted_counter_blocks"]
    assert SBOX[0x00] == 0x63 and SBOX[0x52] == 0x00 and SBOX[0xFF] == 0x16


# ================================================================================== 2. the schedule on clear bits
def fake_scratch(lib, kind, msg, carry, inputs=1, parallelism=16, N=None):
    """a scratch on keys that are never read (scheduling needs none); returns (mem, cleanup)"""
    from tfhe_rs_amd import core_crypto_gpu as gpu, ffi, integer_gpu as igpu
    st = gpu.CudaStreams((0,))
    s, keep = igpu.CudaServerKey._streams(st)
    N = N or max(256, msg * carry)
    bk = ffi.CudaLweBootstrapKeyParamsFFI(4, 1, N, 8, 2, N, 1, 0)
    kk = ffi.CudaLweKeyswitchKeyParamsFFI(N, 4, 4, 3)
    mem = C.c_void_p()
    if kind == "key_expansion":
        lib.hip_scratch_integer_key_expansion_64_async(s, C.byref(mem), bk, kk, msg, carry, True, 0)
    else:
        lib.hip_scratch_integer_aes_ctr_encrypt_64_async(s, C.byref(mem), bk, kk, msg, carry, True, 0, inputs, parallelism)
    return mem, lambda: getattr(lib, f"hip_cleanup_integer_{kind}_64")(s, C.byref(mem)), (st, keep)


_programs = {}


def program(kind, msg, carry, inputs=1, parallelism=16):
    key = (kind, msg, carry, inputs, parallelism)
    if key not in _programs:
        lib = use_backend("emu")
        mem, cleanup, alive = fake_scratch(lib, kind, msg, carry, inputs, parallelism)
        prog = ap.dump(lib, mem)
        counts = int(lib.hip_integer_aes_pbs_count(mem)), int(lib.hip_integer_aes_rounds(mem))
        cleanup()
        _programs[key] = prog, counts
    return _programs[key]


def load_state(prog, wires, state_bytes, n=0):
    """16 bytes of input n into the state wires x[j][lane][input]"""
    for lane, b in enumerate(state_bytes):
        for j in range(8):
            wires[prog.x[j] + lane * prog.inputs + n] = (b >> (7 - j)) & 1


def read_wires(prog, wires, first_rows, lanes, n=0):
    return [sum(int(wires[first_rows[j] + lane * prog.inputs + n]) << (7 - j) for j in range(8)) for lane in range(lanes)]


MODULI = [(4, 4), (8, 8), (4, 16)]


@pytest.mark.parametrize("msg,carry", MODULI, ids=[f"{m}_{c}" for m, c in MODULI])
def test_scheduled_sbox_equals_the_table_on_all_byte_values(msg, carry):
    """16 inputs x 16 lanes: every byte value once through the S-box segment of the dumped program."""
    prog, _ = program("aes_ctr_encrypt", msg, carry, inputs=16)
    wires = np.zeros(prog.wire_rows, dtype=np.int64)
    for n in range(16):
        load_state(prog, wires, [16 * n + lane for lane in range(16)], n)
    ap.run_segment(prog, prog.segments[1], wires)
    for n in range(16):
        assert read_wires(prog, wires, prog.sb, 16, n) == [SBOX[16 * n + lane] for lane in range(16)]


@pytest.mark.parametrize("parallelism", [16, 4, 1])
@pytest.mark.parametrize("msg,carry", MODULI, ids=[f"{m}_{c}" for m, c in MODULI])
def test_scheduled_rounds_equal_the_model_on_random_states(msg, carry, parallelism):
    """One middle round and the last round of the dumped program from random states, at three S-box parallelisms (the lane
    windows of the passes), and the counts the formulas give."""
    prog, (pbs, rounds) = program("aes_ctr_encrypt", msg, carry, parallelism=parallelism)
    add, sbox, lin, last = prog.segments
    assert sbox.lanes == parallelism and sbox.passes == 16 // parallelism
    assert pbs == add.rows_per_input + 10 * sbox.rows_per_input + 9 * lin.rows_per_input + last.rows_per_input
    assert rounds == len(add.rounds) + 10 * sbox.passes * len(sbox.rounds) + 9 * len(lin.rounds) + len(last.rounds)
    if (msg, carry) == (4, 4):
        assert pbs == AES_PBS_PER_INPUT and len(sbox.rounds) == SBOX_ROUNDS and sbox.rows_per_input == 16 * SBOX_PBS_PER_LANE
        assert rounds == AES_ROUNDS_P16 + 10 * SBOX_ROUNDS * (16 // parallelism - 1)
    rng = np.random.default_rng(10 * msg + carry + parallelism)
    state = rng.integers(0, 256, size=16).tolist()
    rk = rng.integers(0, 256, size=16).tolist()
    key_rows = np.array(bits_of_bytes(rk), dtype=np.int64)
    wires = np.zeros(prog.wire_rows, dtype=np.int64)
    load_state(prog, wires, state)
    ap.run_segment(prog, sbox, wires)
    ap.run_segment(prog, lin, wires, caller_a=key_rows)
    assert read_wires(prog, wires, prog.x, 16) == middle_round(state, rk)
    out = np.zeros(128, dtype=np.int64)
    load_state(prog, wires, state)
    ap.run_segment(prog, sbox, wires)
    ap.run_segment(prog, last, wires, caller_a=key_rows, out=out)
    assert bytes_of_bits(out) == last_round(state, rk)


@pytest.mark.parametrize("msg,carry", MODULI, ids=[f"{m}_{c}" for m, c in MODULI])
def test_scheduled_counter_addition_equals_the_model(msg, carry):
    prog, _ = program("aes_ctr_encrypt", msg, carry, inputs=3)
    rng = np.random.default_rng(77)
    k0 = rng.integers(0, 256, size=16).tolist()
    for iv, start in (((1 << 128) - 1, 1), (0, 0), (int(rng.integers(0, 1 << 62)) << 66 | 5, (1 << 64) - 1)):
        wires = np.zeros(prog.wire_rows, dtype=np.int64)
        clear = [[((start + n) >> i) & 1 for i in range(128)] for n in range(3)]
        ap.run_segment(prog, prog.segments[0], wires, caller_a=np.array(bits_of_bytes(to_bytes(iv))),
                       caller_b=np.array(bits_of_bytes(k0)), clear=clear)
        for n in range(3):
            want = [a ^ b for a, b in zip(to_bytes((iv + start + n) % (1 << 128)), k0)]
            assert read_wires(prog, wires, prog.x, 16, n) == want


@pytest.mark.parametrize("msg,carry", MODULI, ids=[f"{m}_{c}" for m, c in MODULI])
def test_scheduled_key_schedule_equals_fips197_a1(msg, carry):
    """All ten steps of the dumped key-schedule program on the clear key of Appendix A.1."""
    prog, (pbs, rounds) = program("key_expansion", msg, carry)
    assert len(prog.segments) == 11 and prog.segments[0].lanes == 4
    assert pbs == sum(prog.segments[0].rows_per_input + s.rows_per_input for s in prog.segments[1:])
    assert rounds == 10 * (len(prog.segments[0].rounds) + 1)
    if (msg, carry) == (4, 4):
        assert (pbs, rounds) == (KEY_PBS, KEY_ROUNDS)
    rks = expand_key(to_bytes(int(VECTORS["fips197_a1"]["key"], 16)))
    out = np.zeros(11 * 128, dtype=np.int64)
    out[:128] = bits_of_bytes(rks[0])
    wires = np.zeros(prog.wire_rows, dtype=np.int64)
    for k in range(1, 11):
        prev = out[128 * (k - 1):128 * k].copy()
        ap.run_segment(prog, prog.segments[0], wires, caller_a=prev)
        ap.run_segment(prog, prog.segments[k], wires, caller_a=prev, out=out)
        assert bytes_of_bits(out[128 * k:128 * (k + 1)]) == rks[k], f"round key {k}"


@pytest.mark.parametrize("kind", ["aes_ctr_encrypt", "key_expansion"])
@pytest.mark.parametrize("msg,carry", MODULI, ids=[f"{m}_{c}" for m, c in MODULI])
def test_every_row_stays_inside_its_block_and_its_noise_level(kind, msg, carry):
    """Recomputed from the dump alone: the largest value of every row (from the largest values of its sources, the largest
    table entries below THEIR largest values) stays below msg * carry — so every table entry a row can reach exists — and
    its noise level, the sum of |scalar| over encrypted sources (each a fresh bootstrap output or a clean block of the caller
    at level 1), is at most (msg * carry - 1) / (msg - 1)."""
    prog, _ = program(kind, msg, carry)
    space, max_noise = msg * carry, (msg * carry - 1) // (msg - 1)
    wires = np.zeros(prog.wire_rows, dtype=np.int64)
    ones = np.ones(11 * 128, dtype=np.int64)
    if kind == "aes_ctr_encrypt":
        for j in range(8):
            wires[prog.x[j]:prog.x[j] + 16] = 1
    bounds = []
    for seg in prog.segments:
        ap.run_segment(prog, seg, wires, caller_a=ones, caller_b=ones, clear=[[1] * 128], out=np.zeros(11 * 128, dtype=np.int64),
                       bounds=bounds)
    assert bounds
    for row, value, noise in bounds:
        assert value < space, f"a row of table {row.table} reaches {value}"
        assert noise <= max_noise, f"a row of table {row.table} has noise level {noise}"
        assert len(prog.tables[row.table]) == space
    assert max(noise for _, _, noise in bounds) >= 4


# ================================================================================== 3. the kernel alone
SENTINEL = U64(0xA5A5A5A55A5A5A5A)
LANES = 8           # lanes of the test's state: two columns
DELTA = 1 << 59


def gate_program(inputs):
    """groups: (constant, [(base, row0, lane_stride, map, flags, scalar)]).  wires: 3 wires of 8 lanes; caller_a: 8 lanes x 2
    bits, rows that exist once; caller_b: one row per input."""
    N = inputs
    wire = lambda j: j * LANES * N
    big = (1 << 64) - 3
    return [
        (0, [(ap.WIRES, wire(0), N, 0, ap.STATE_LANE, 1)]),
        (5, []),                                                                       # a constant-only row
        (1, [(ap.WIRES, wire(j % 3), N, 0, ap.STATE_LANE, 1 + j) for j in range(11)]),   # more than kSumInFlight terms
        (0, [(ap.CALLER_A, 1, 2, 0, ap.STATE_LANE | ap.BROADCAST, 3),                    # a broadcast caller row per lane
             (ap.WIRES, wire(1), N, ap.PERM | 0 << 2, ap.STATE_LANE, 1),                 # a lane permutation
             (ap.WIRES, wire(2), N, ap.COLUMN | 3 << 2, ap.STATE_LANE, big)]),           # a column offset; a wrapping scalar
        (2, [(ap.CALLER_B, 0, 0, 0, 0, big), (ap.CLEAR, 2, 0, 0, 0, 4), (ap.WIRES, wire(0) + 2 * N, 0, 0, 0, 7)]),
        (0, [(ap.WIRES, wire(2), N, ap.COLUMN | 1 << 2, ap.STATE_LANE, big), (ap.WIRES, wire(2), N, ap.PERM | 1 << 2, ap.STATE_LANE, 2)]),
    ]


GATE_MAPS = [[5, 0, 7, 2, 1, 4, 3, 6] + list(range(8, 16)), [7, 6, 5, 4, 3, 2, 1, 0] + list(range(8, 16))]


def gate_model(groups, srcs, clear, words, inputs, lanes, lane0):
    out = np.zeros((len(groups), lanes, inputs, words), dtype=U64)
    for g, (constant, terms) in enumerate(groups):
        for l in range(lanes):
            for n in range(inputs):
                body = constant
                for base, row0, ls, mp, flags, scalar in terms:
                    if base == ap.CLEAR:
                        body += scalar * int(clear[n * 4 + row0])
                        continue
                    sl = l
                    if flags & ap.STATE_LANE:
                        lane = lane0 + l
                        sl = GATE_MAPS[mp >> 2][lane] if mp & 3 == ap.PERM else ((lane & ~3) | ((lane + (mp >> 2)) & 3)) if mp & 3 == ap.COLUMN else lane
                    r = row0 + sl * ls + (0 if flags & ap.BROADCAST else n)
                    out[g, l, n] += U64(scalar) * srcs[base][r]
                out[g, l, n, -1] = U64((int(out[g, l, n, -1]) + body * DELTA) % (1 << 64))
    return out


def call_gate_sum(lib, st, d_out, d_src, d_clear, groups, words, inputs, lanes, lane0, rows):
    G = len(groups)
    terms = [t for _, ts in groups for t in ts]
    T = max(1, len(terms))
    consts = (C.c_uint64 * G)(*[c for c, _ in groups])
    counts = (C.c_uint32 * G)(*[len(ts) for _, ts in groups])
    col = lambda i, ty: (ty * T)(*[t[i] for t in terms])
    maps = (C.c_uint32 * 32)(*sum(GATE_MAPS, []))
    lib.hip_test_gate_sum_async(st.ptr[0], 0, d_out, d_src[0], d_src[1], d_src[2], d_clear, words, inputs, lanes, lane0, LANES, 4,
                                DELTA, G, consts, counts, col(5, C.c_uint64), col(1, C.c_uint32), col(2, C.c_uint32),
                                col(3, C.c_uint32), col(0, C.c_uint32), col(4, C.c_uint32), 2, maps, rows[0], rows[1], rows[2])


@pytest.mark.parametrize("inputs", [1, 3], ids=["1_input", "3_inputs"])
@pytest.mark.parametrize("words", [257, 2049], ids=["257_words", "2049_words"])   # a partial slice; four slices and one word
@pytest.mark.parametrize("kind", KINDS)
def test_gate_sum_kernel_equals_numpy_word_for_word(kind, words, inputs):
    """hip_test_gate_sum_async against the formula on random u64 words: a group of 11 terms (two passes of the load loop), a
    constant-only row, a broadcast caller row, a lane permutation, column offsets, scalars that wrap modulo 2^64, a second
    caller base, a clear term, and a launch on the upper half of the lanes.  The output sits between sentinel rows."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    lib = use_backend(kind)
    st = gpu.CudaStreams((0,))
    rng = np.random.default_rng(1000 * words + inputs)
    rows = [3 * LANES * inputs, 2 * LANES, inputs]
    srcs = {b: rng.integers(0, 2 ** 64, size=(rows[b], words), dtype=U64) for b in range(3)}
    clear = rng.integers(0, 2, size=4 * inputs, dtype=U64)
    d_src = [gpu.CudaVec.from_cpu_async(srcs[b].reshape(-1), st) for b in range(3)]
    d_clear = gpu.CudaVec.from_cpu_async(clear, st)
    groups = gate_program(inputs)
    for lanes, lane0 in ((LANES, 0), (4, 4)):
        size = len(groups) * lanes * inputs * words
        guard = 2 * words
        frame = np.full(size + 2 * guard, SENTINEL, dtype=U64)
        d_out = gpu.CudaVec.from_cpu_async(frame, st)
        call_gate_sum(lib, st, d_out.ptr + 8 * guard, [d.ptr for d in d_src], d_clear.ptr, groups, words, inputs, lanes, lane0, rows)
        got = d_out.copy_to_cpu(st)
        want = gate_model(groups, srcs, clear, words, inputs, lanes, lane0)
        assert np.array_equal(got[guard:guard + size], want.reshape(-1)), f"{lanes} lanes from lane {lane0}"
        assert (got[:guard] == SENTINEL).all() and (got[guard + size:] == SENTINEL).all(), "a sentinel row was written"


# ================================================================================== contexts
_ctx = {}


def ctx(kind, base_name, emu=None):
    """keys on the backend at a base of tests/test_radix_bases.py, toy keys on both backends; `emu`: the set the emulation
    takes instead of the base's"""
    key = (kind, base_name, emu.name if emu else None)
    if key not in _ctx:
        base = BASE[base_name]
        _ctx[key] = Ctx(kind, dataclasses.replace(base, hip=base.emu, emu=emu or base.emu))
    use_backend(kind)
    return _ctx[key]


def anchor(kind):
    return ctx(kind, "classic_4_4", SMALL_4_4 if kind == "emu" else None)


class Scratch:
    """a cipher scratch on a context's keys, for the test hooks"""

    def __init__(self, c, inputs, parallelism=16):
        self.c, self.lib = c, use_backend(c.kind)
        self.s, self.keep = c.sks._streams(c.st)
        self.ksks, self.bsks = c.sks._key_ptrs(c.st)
        self.mem = C.c_void_p()
        c.sks._aes_scratch(self.lib, self.s, self.mem, "aes_ctr_encrypt", True, inputs, parallelism)

    def close(self):
        self.lib.hip_cleanup_integer_aes_ctr_encrypt_64(self.s, C.byref(self.mem))


def wire_rows(state_bytes):
    """[input][lane] bytes -> bits in the order [wire j][lane][input]"""
    a = np.asarray(state_bytes)
    return [int(a[n, lane] >> (7 - j)) & 1 for j in range(8) for lane in range(a.shape[1]) for n in range(a.shape[0])]


def bytes_of_wire_rows(bits, inputs, lanes):
    b = np.asarray(bits).reshape(8, lanes, inputs)
    return [[sum(int(b[j, lane, n]) << (7 - j) for j in range(8)) for lane in range(lanes)] for n in range(inputs)]


def sbox_pass(c, byte_values, inputs, parallelism, seed):
    """byte_values [input][lane] through hip_test_aes_sbox_async; returns (decrypted bytes [input][lane], bootstraps, words)"""
    sc = Scratch(c, inputs, parallelism)
    x = c.enc([wire_rows(byte_values)], seed, degree=1)
    y = c.igpu.CudaUnsignedRadixCiphertext.from_blocks(np.zeros_like(c.words(x)), c.st)
    before = int(sc.lib.hip_integer_aes_pbs_count(sc.mem))
    sc.lib.hip_test_aes_sbox_async(sc.s, y.d_blocks.ptr, x.d_blocks.ptr, sc.mem, sc.bsks, sc.ksks)
    out = bytes_of_wire_rows(c.dec(y)[0], inputs, parallelism)
    words = c.words(y)
    sc.close()
    return out, before, words


# ================================================================================== 4. the S-box pass
@pytest.mark.parametrize("kind", KINDS)
def test_sbox_pass_decrypts_to_the_table(kind):
    """emu: 4 lanes of one input, 0x00, 0x52 (-> 0x00), 0xff and a random byte; hip: 16 inputs x 16 lanes, every byte value
    once.  The published count of a whole call is 441 + 75 * 160 + 16 * 144 + 128 bootstraps per input."""
    c = anchor(kind)
    if kind == "emu":
        values, inputs, par = [[0x00, 0x52, 0xFF, int(np.random.default_rng(4).integers(1, 255))]], 1, 4
    else:
        values, inputs, par = [[16 * n + lane for lane in range(16)] for n in range(16)], 16, 16
    got, pbs, _ = sbox_pass(c, values, inputs, par, 400)
    assert got == [[SBOX[v] for v in row] for row in values]
    assert pbs == AES_PBS_PER_INPUT * inputs


# ================================================================================== 5. the counter addition, 6. single rounds
def encrypt_block_bits(c, value, seed):
    from tfhe_rs_amd.integer_gpu import encrypt_u128_for_aes_ctr
    return c.enc([encrypt_u128_for_aes_ctr(value)], seed, degree=1)


def encrypt_round_keys(c, rks, seed):
    return c.enc([sum((bits_of_bytes(rk) for rk in rks), [])], seed, degree=1)


def run_rounds(c, sc, inputs, r0, r1, state_bytes=None, iv=None, rks=None, start=0, seed=500):
    """hip_test_aes_rounds_async; returns the state bytes [input][lane] after round r1, or the output blocks after round 10"""
    lib = sc.lib
    rks = rks or [[0] * 16] * 11
    keys = encrypt_round_keys(c, rks, seed)
    ivc = encrypt_block_bits(c, iv or 0, seed + 1)
    st = c.enc([wire_rows(state_bytes if state_bytes is not None else [[0] * 16] * inputs)], seed + 2, degree=1)
    out = c.igpu.CudaUnsignedRadixCiphertext.from_blocks(np.zeros((1, 128 * inputs, c.p.big_n + 1), dtype=U64), c.st)
    bits = np.array([((start + n) >> i) & 1 for n in range(inputs) for i in range(128)], dtype=U64)
    lib.hip_test_aes_rounds_async(sc.s, st.d_blocks.ptr, C.byref(out._ffi()), C.byref(ivc._ffi()), C.byref(keys._ffi()),
                                  bits.ctypes.data, r0, r1, sc.mem, sc.bsks, sc.ksks)
    c.st.synchronize()
    if r1 == 10:
        assert (out.degrees == 1).all() and (out._info[1] == 1).all()
        return [bytes_of_bits(row) for row in np.asarray(c.dec(out)[0]).reshape(inputs, 128)]
    return bytes_of_wire_rows(c.dec(st)[0], inputs, 16)


ADDITIONS = {"carry_through_all_bits_and_wrap": ((1 << 128) - 1, 1), "iv_zero": (0, 0),
             "random_iv_across_a_64_bit_boundary": (int.from_bytes(np.random.default_rng(511).bytes(16), "big"), (1 << 64) - 1)}


@pytest.mark.parametrize("case", list(ADDITIONS))
@pytest.mark.parametrize("kind", KINDS)
def test_counter_addition_alone(kind, case):
    """3 inputs: a carry through all 128 bits that wraps, iv = 0, and a random iv under counters that straddle a
    64-bit boundary; the state after the addition is (iv + counter) ^ round key 0, compared bit for bit."""
    c = anchor(kind)
    iv, start = ADDITIONS[case]
    k0 = np.random.default_rng(510).integers(0, 256, size=16).tolist()
    sc = Scratch(c, 3)
    try:
        got = run_rounds(c, sc, 3, 0, 0, iv=iv, rks=[k0] + [[0] * 16] * 10, start=start, seed=520)
    finally:
        sc.close()
    assert got == [[a ^ b for a, b in zip(to_bytes((iv + start + n) % (1 << 128)), k0)] for n in range(3)]


@pytest.mark.parametrize("r", [5, 10], ids=["middle_round", "last_round"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_round_from_a_random_state(kind, r):
    c = anchor(kind)
    rng = np.random.default_rng(600)
    state = rng.integers(0, 256, size=(1, 16)).tolist()
    rks = rng.integers(0, 256, size=(11, 16)).tolist()
    sc = Scratch(c, 1)
    try:
        got = run_rounds(c, sc, 1, r, r, state_bytes=state, rks=rks, seed=610 + r)
    finally:
        sc.close()
    assert got == [(last_round if r == 10 else middle_round)(state[0], rks[r])]


# ================================================================================== 7. whole calls
def decrypt_blocks_u128(c, ct, inputs):
    from tfhe_rs_amd.integer_gpu import decrypt_u128_from_aes_ctr
    return decrypt_u128_from_aes_ctr(c.dec(ct)[0], inputs)


@pytest.mark.gpu
def test_key_expansion_gives_fips197_a1_and_aes_encrypt_gives_sp800_38a():
    c = anchor("hip")
    key, iv = encrypt_block_bits(c, KEY, 700), encrypt_block_bits(c, IV, 701)
    rks, pbs, rounds = c.sks.key_expansion(key, c.st, return_pbs_count=True, return_rounds=True)
    assert (pbs, rounds) == (KEY_PBS, KEY_ROUNDS)
    assert (rks.degrees == 1).all() and (rks._info[1] == 1).all()
    want = expand_key(to_bytes(KEY))
    assert bytes_of_bits(c.dec(rks)[0]) == sum(want, [])
    words = ["%08x" % from_bytes([0] * 12 + b[4 * i:4 * i + 4]) for b in want for i in range(4)]
    assert words == VECTORS["fips197_a1"]["words"]
    blocks = VECTORS["sp800_38a_f51"]["encrypted_counter_blocks"]
    one, pbs, rounds = c.sks.aes_encrypt(iv, rks, 0, 1, 16, c.st, return_pbs_count=True, return_rounds=True)
    assert (pbs, rounds) == (AES_PBS_PER_INPUT, AES_ROUNDS_P16)
    assert ["%032x" % v for v in decrypt_blocks_u128(c, one, 1)] == blocks[:1]
    assert (one.degrees == 1).all() and (one._info[1] == 1).all()
    three, pbs = c.sks.aes_encrypt(iv, rks, 1, 3, 16, c.st, return_pbs_count=True)
    assert pbs == 3 * AES_PBS_PER_INPUT
    got = decrypt_blocks_u128(c, three, 3)
    assert got == [ctr_block(KEY, IV, 1 + n) for n in range(3)] and "%032x" % got[0] == blocks[1]


@pytest.mark.gpu
def test_aes_ctr_equals_key_expansion_then_aes_encrypt_at_parallelism_4_and_16():
    c = anchor("hip")
    key, iv = encrypt_block_bits(c, KEY, 710), encrypt_block_bits(c, IV, 711)
    want = [ctr_block(KEY, IV, n) for n in range(2)]
    assert decrypt_blocks_u128(c, c.sks.aes_ctr(key, iv, 0, 2, c.st), 2) == want
    rks = c.sks.key_expansion(key, c.st)
    r = {}
    for par in (4, 16):
        out, pbs, r[par] = c.sks.aes_encrypt(iv, rks, 0, 2, par, c.st, return_pbs_count=True, return_rounds=True)
        assert decrypt_blocks_u128(c, out, 2) == want and pbs == 2 * AES_PBS_PER_INPUT
    assert r[16] == AES_ROUNDS_P16 and r[4] == AES_ROUNDS_P16 + 10 * SBOX_ROUNDS * 3
    assert decrypt_blocks_u128(c, c.sks.aes_ctr_with_fixed_parallelism(key, iv, 0, 2, 4, c.st), 2) == want


# ================================================================================== 8. production parameters
@pytest.mark.gpu
def test_aes_ctr_on_param_message_2_carry_2():
    """The only test that sees real noise: PARAM_MESSAGE_2_CARRY_2, two inputs, the two SP 800-38A blocks."""
    c = Ctx("hip", BASE["classic_4_4"])
    key, iv = encrypt_block_bits(c, KEY, 800), encrypt_block_bits(c, IV, 801)
    out = c.sks.aes_ctr(key, iv, 0, 2, c.st)
    assert ["%032x" % v for v in decrypt_blocks_u128(c, out, 2)] == VECTORS["sp800_38a_f51"]["encrypted_counter_blocks"]


# ================================================================================== 9. other keys and bases
OTHER = {"multibit_g4_4_4": None, "classic_8_8": SMALL_8_8, "multibit_g3_4_4": None}


@pytest.mark.parametrize("base", list(OTHER))
@pytest.mark.parametrize("kind", KINDS)
def test_one_sbox_pass_on_other_keys_and_bases(kind, base):
    c = ctx(kind, base, OTHER[base] if kind == "emu" else None)
    values = [[0x53, 0xA7]]
    got, _, _ = sbox_pass(c, values, 1, 2, 900)
    assert got == [[SBOX[v] for v in values[0]]]


# ================================================================================== 10. sharding
@pytest.mark.parametrize("kind", KINDS)
def test_rounds_sharded_over_the_streams_of_the_set(kind):
    """One stream against three streams on the same GPU at a threshold of 20 blocks per GPU (rounds of 64 rows and more then
    run as three shards): identical words out of one S-box pass."""
    from .test_radix_integer import setup
    from . import radix_model as rm
    p = SMALL_4_4 if kind == "emu" else BASE["classic_4_4"].emu
    _, keys, st1, sks1, igpu = setup(kind, p)
    _, _, st3, sks3, _ = setup(kind, p, gpu_indexes=(0, 0, 0))
    lib = use_backend(kind)
    values = [[0x00, 0x52, 0xFF, 0x3C]]
    words = rm.encrypt_rows(p, keys, [wire_rows(values)], 1000)
    outs = {}
    for name, st, sks, thr in (("one", st1, sks1, 512), ("three", st3, sks3, 20)):
        lib.hip_integer_set_multi_gpu_threshold(thr)
        try:
            s, keep = sks._streams(st)
            ksks, bsks = sks._key_ptrs(st)
            mem = C.c_void_p()
            sks._aes_scratch(lib, s, mem, "aes_ctr_encrypt", True, 1, 4)
            x = igpu.CudaUnsignedRadixCiphertext.from_blocks(words, st)
            y = igpu.CudaUnsignedRadixCiphertext.from_blocks(np.zeros_like(words), st)
            lib.hip_test_aes_sbox_async(s, y.d_blocks.ptr, x.d_blocks.ptr, mem, bsks, ksks)
            outs[name] = y.to_blocks(st)
            lib.hip_cleanup_integer_aes_ctr_encrypt_64(s, C.byref(mem))
        finally:
            lib.hip_integer_set_multi_gpu_threshold(0)
    assert np.array_equal(outs["one"], outs["three"])
    assert bytes_of_wire_rows(rm.decrypt_many(p, keys, outs["three"])[0], 1, 4) == [[SBOX[v] for v in values[0]]]


# ================================================================================== 11. device = emulation
def sbox_pass_words(c, words):
    """every device object of the pass dies in here, while its backend is still the current one"""
    sc = Scratch(c, 1, 4)
    x, y = c.from_words(words, degree=1), c.from_words(np.zeros_like(words), degree=1)
    sc.lib.hip_test_aes_sbox_async(sc.s, y.d_blocks.ptr, x.d_blocks.ptr, sc.mem, sc.bsks, sc.ksks)
    out = c.words(y)
    sc.close()
    return out


@pytest.mark.gpu
def test_device_equals_emulation_word_for_word():
    """The same keys and the same seeded inputs through both backends: one S-box pass on four lanes."""
    from . import radix_model as rm
    toy = dataclasses.replace(BASE["classic_4_4"], hip=SMALL_4_4, emu=SMALL_4_4)
    try:
        hip = Ctx("hip", toy)
        words = rm.encrypt_rows(hip.p, hip.keys, [wire_rows([[0x00, 0x52, 0xFF, 0x3C]])], 1100)
        got = sbox_pass_words(hip, words)
        gc.collect()
        want = sbox_pass_words(Ctx("emu", toy), words)
    finally:
        use_backend("hip")
    assert np.array_equal(got, want), "the device's words differ from the emulation's"


# ================================================================================== 12. refusals
PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
N, n = 256, 4
BK = ffi.CudaLweBootstrapKeyParamsFFI(n, 1, N, 8, 2, N, 1, 0)
KK = ffi.CudaLweKeyswitchKeyParamsFFI(N, n, 4, 3)
keys = (C.c_void_p * 1)(gpu.CudaVec(16, st).ptr)
alive = []
def radix(blocks, degree=1):
    ct = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec(blocks * (N + 1), st), 1, blocks, N)
    ct.set_degrees(degree)
    alive.extend([ct, ct._ffi()])
    return C.byref(alive[-1])
def scratch(kind="aes", inputs=1, parallelism=16, msg=4, carry=4):
    mem = C.c_void_p()
    if kind == "aes":
        lib.hip_scratch_integer_aes_ctr_encrypt_64_async(s, C.byref(mem), BK, KK, msg, carry, True, 0, inputs, parallelism)
    else:
        lib.hip_scratch_integer_key_expansion_64_async(s, C.byref(mem), BK, KK, msg, carry, True, 0)
    return mem
bits = (C.c_uint64 * 256)()
"""

REFUSALS = {
    "parallelism 3": ("""
        scratch(parallelism=3)
        """, "aes_ctr_encrypt: sbox_parallelism 3 is not one of 1, 2, 4, 8, 16"),
    "zero inputs": ("""
        scratch(inputs=0)
        """, "aes_ctr_encrypt: 0 inputs"),
    "a key of 127 blocks": ("""
        lib.hip_integer_key_expansion_64_async(s, radix(1408), radix(127), scratch("key"), keys, keys)
        """, "key_expansion: the key: 127 blocks, not 128"),
    "round keys of 10 x 128 blocks": ("""
        lib.hip_integer_aes_ctr_encrypt_64_async(s, radix(128), radix(128), radix(1280), bits, 1, scratch(), keys, keys)
        """, "aes_ctr_encrypt: the round keys: 1280 blocks, not 1408"),
    "an output of the wrong length": ("""
        lib.hip_integer_aes_ctr_encrypt_64_async(s, radix(128), radix(128), radix(1408), bits, 2, scratch(inputs=2), keys, keys)
        """, "aes_ctr_encrypt: the output: 128 blocks, not 256"),
    "base (2, 2)": ("""
        scratch(msg=2, carry=2)
        """, "aes_ctr_encrypt: moduli (2, 2) do not hold the value 15 and the noise level 5 a row reaches"),
    "a gate-sum program whose output overlaps a source": ("""
        v = gpu.CudaVec(8 * 16, st)
        one32, zero32 = (C.c_uint32 * 1)(1), (C.c_uint32 * 1)(0)
        lib.hip_test_gate_sum_async(S, 0, v.ptr + 8 * 16, v.ptr, None, None, None, 16, 1, 1, 0, 1, 1, 1, 1, (C.c_uint64 * 1)(0),
                                    one32, (C.c_uint64 * 1)(1), one32, zero32, zero32, zero32, zero32, 0, None, 8, 0, 0)
        """, "gate_sum: the output overlaps the rows term 0 of group 0 reads"),
    "an empty gate-sum program": ("""
        v = gpu.CudaVec(8 * 16, st)
        lib.hip_test_gate_sum_async(S, 0, v.ptr, v.ptr, None, None, None, 16, 1, 1, 0, 1, 1, 1, 0, None, None, None, None, None,
                                    None, None, None, 0, None, 8, 0, 0)
        """, "gate_sum: empty program"),
    "a lane map that leaves the state": ("""
        v = gpu.CudaVec(64 * 16, st)
        one32, zero32 = (C.c_uint32 * 1)(1), (C.c_uint32 * 1)(0)
        lib.hip_test_gate_sum_async(S, 0, v.ptr, v.ptr + 8 * 16 * 8, None, None, None, 16, 1, 4, 0, 4, 1, 1, 1, (C.c_uint64 * 1)(0),
                                    one32, (C.c_uint64 * 1)(1), zero32, one32, (C.c_uint32 * 1)(1), zero32, (C.c_uint32 * 1)(2),
                                    1, (C.c_uint32 * 16)(*([9] * 16)), 8, 0, 0)
        """, "leaves the state of 4 lanes"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_").replace(",", "").replace("(", "").replace(")", "") for n in REFUSALS])
def test_misuse_is_refused_with_a_message(name):
    """On the host emulation only, in a child process: the library aborts with a message that names the entry point."""
    snippet, message = REFUSALS[name]
    r = run_child(PRELUDE + textwrap.dedent(snippet))
    assert r.returncode == -signal.SIGABRT, f"{name}: returned {r.returncode}\n{r.stderr[-600:]}"
    assert message in r.stderr, r.stderr[-600:]
