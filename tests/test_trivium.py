"""Trivium transciphering: the tap kernel, batches of 64 steps from arbitrary states, the re-basing of the state tapes, the
warm-up against the published vectors, stateful against monolithic use, other key kinds and bases, sharding over a stream
set, the device against the host emulation, and the refusals.

The checker is the clear model of the cipher below (the specification's three registers, one step at a time); nothing of
it reads the library's tables.  tests/golden/trivium_vectors.json holds the four key / IV / keystream vectors.
[emu] runs the kernel sources on the host, [hip] on the MI355X, both on toy keys.  A full warm-up is 6,912 bootstraps per
input: it runs on [hip] only (17 s on the emulation's smallest toy set); the batches and the re-basing are the CPU tier's
coverage."""
import ctypes as C
import dataclasses
import gc
import json
import os
import signal
import textwrap

import numpy as np
import pytest

from .common import Params
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_bases import BASES, Ctx

U64 = np.uint64
BASE = {b.name: b for b in BASES}
BITS = (93, 84, 111)
VECTORS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trivium_vectors.json")))["vectors"]

# the emulation runs a fibre per lane: it takes the smallest polynomial that holds the plaintext space
SMALL_4_4 = Params("toy_k1_N512_l1_p16", 8, 1, 512, 23, 1, 4, 4, 45, 17, 16, ms_type=1)
SMALL_8_8 = Params("toy_k1_N1024_l1_p64", 8, 1, 1024, 23, 1, 4, 4, 45, 17, 64, ms_type=1)

KINDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]


# ================================================================================== the clear model
class ClearTrivium:
    """The cipher on clear bits: a (93), b (84), c (111), position 0 the newest bit."""

    def __init__(self, a, b, c):
        self.a, self.b, self.c = list(a), list(b), list(c)
        assert (len(self.a), len(self.b), len(self.c)) == BITS

    @classmethod
    def from_key_iv(cls, key, iv):
        assert len(key) == len(iv) == 80
        a, b, c = [0] * 93, [0] * 84, [0] * 111
        for i in range(80):
            a[i], b[i] = key[79 - i], iv[79 - i]
        c[108] = c[109] = c[110] = 1
        t = cls(a, b, c)
        t.run(1152)
        return t

    def step(self):
        a, b, c = self.a, self.b, self.c
        t1, t2, t3 = a[65] ^ a[92], b[68] ^ b[83], c[65] ^ c[110]
        z = t1 ^ t2 ^ t3
        a_in = t3 ^ a[68] ^ (c[108] & c[109])
        b_in = t1 ^ b[77] ^ (a[90] & a[91])
        c_in = t2 ^ c[86] ^ (b[81] & b[82])
        self.a, self.b, self.c = [a_in] + a[:-1], [b_in] + b[:-1], [c_in] + c[:-1]
        return z

    def run(self, steps):
        return [self.step() for _ in range(steps)]


def hex_bits(text):
    return [(int(text[i:i + 2], 16) >> j) & 1 for i in range(0, len(text), 2) for j in range(8)]


def bits_hex(bits):
    return "".join("%02X" % sum(bits[i + j] << j for j in range(8)) for i in range(0, len(bits), 8))


# ================================================================================== 1. the model against the vectors
@pytest.mark.parametrize("vector", VECTORS, ids=[f"vector_{i + 1}" for i in range(len(VECTORS))])
def test_clear_model_reproduces_the_published_vectors(vector):
    assert len(VECTORS) == 4 and len(vector["keystream_hex"]) == 128
    model = ClearTrivium.from_key_iv(hex_bits(vector["key_hex"]), hex_bits(vector["iv_hex"]))
    assert bits_hex(model.run(512)) == vector["keystream_hex"]


# ================================================================================== 2. the kernel alone
SENTINEL = U64(0xA5A5A5A55A5A5A5A)
TAPE = 70        # positions of each of the two source tapes: 64 bits fit from position 0 and from position 6
MSG = 4


def tap_tables(tape_positions):
    """name -> groups; a group is (bits, [(source tape, position, backwards, scalar), ...]).  Positions reach both ends of
    a tape: bit 0 at position 0, bit 63 at the last position, forwards and backwards."""
    last = tape_positions - 1
    return {
        "one_term": [(64, [(0, 0, 0, 1)])],
        "one_term_backwards_from_the_end": [(64, [(1, last, 1, 1)])],
        "two_terms_msg_and_one": [(64, [(0, last - 63, 0, MSG), (1, 0, 0, 1)])],
        "five_terms": [(64, [(0, 0, 0, 1), (0, last - 63, 0, 1), (1, 3, 0, 1), (1, 63, 1, 1), (0, 1, 0, MSG)])],
        "four_groups_of_1_2_5_4_terms_and_unequal_bits": [
            (64, [(1, last - 63, 0, 1)]),
            (40, [(0, 2, 0, MSG), (0, 1, 0, 1)]),
            (64, [(0, 0, 0, 1), (1, 0, 0, 1), (0, 6, 0, 1), (1, last, 1, MSG), (1, 5, 0, 1)]),
            (7, [(1, last - 6, 0, 1), (0, 6, 1, 1), (0, 9, 0, MSG), (1, 9, 0, 1)]),
        ],
    }


def tap_model(src, groups, inputs):
    """src: [tape][position][input][words]; the kernel's formula in NumPy (u64 arithmetic wraps modulo 2^64)"""
    out = []
    for bits, terms in groups:
        o = np.zeros((bits, inputs, src.shape[-1]), dtype=U64)
        for q in range(bits):
            for tape, pos, backwards, scalar in terms:
                o[q] += U64(scalar) * src[tape, pos - q if backwards else pos + q]
        out.append(o)
    return out


@pytest.mark.parametrize("inputs", [1, 3], ids=["1_input", "3_inputs"])
@pytest.mark.parametrize("words", [257, 2049], ids=["257_words", "2049_words"])   # a partial slice; four slices and one word
@pytest.mark.parametrize("kind", KINDS)
def test_tap_kernel_equals_numpy_word_for_word(kind, words, inputs):
    """hip_test_tap_sum_async against the formula on random u64 words: tables of 1, 2 and 5 terms, scalars 1 and msg, four
    groups at once (with fewer bits in two of them), source positions at both ends of a tape, both directions.  Every
    group's rows sit between sentinel rows that must stay as they are."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    lib = use_backend(kind)
    st = gpu.CudaStreams((0,))
    rng = np.random.default_rng(100 * words + inputs)
    src = rng.integers(0, 2 ** 64, size=(2, TAPE, inputs, words), dtype=U64)
    d_src = gpu.CudaVec.from_cpu_async(src.reshape(-1), st)
    tape_bytes = TAPE * inputs * words * 8
    guard = 2 * words
    for name, groups in tap_tables(TAPE).items():
        sizes = [bits * inputs * words for bits, _ in groups]
        starts, at = [], 0
        for s in sizes:
            starts.append(at + guard)
            at += guard + s
        frame = np.full(at + guard, SENTINEL, dtype=U64)
        d_out = gpu.CudaVec.from_cpu_async(frame, st)
        G = len(groups)
        outs = (C.c_void_p * G)(*[d_out.ptr + 8 * s for s in starts])
        bits = (C.c_uint32 * G)(*[b for b, _ in groups])
        terms = (C.c_uint32 * G)(*[len(t) for _, t in groups])
        srcs, pos, back, scal = (C.c_void_p * (5 * G))(), (C.c_uint32 * (5 * G))(), (C.c_uint32 * (5 * G))(), (C.c_uint64 * (5 * G))()
        for g, (_, ts) in enumerate(groups):
            for t, (tape, p, backwards, scalar) in enumerate(ts):
                srcs[5 * g + t], pos[5 * g + t], back[5 * g + t], scal[5 * g + t] = d_src.ptr + tape * tape_bytes, p, backwards, scalar
        lib.hip_test_tap_sum_async(st.ptr[0], 0, words, inputs, G, outs, bits, terms, srcs, pos, back, scal)
        got = d_out.copy_to_cpu(st)
        want = tap_model(src, groups, inputs)
        covered = np.zeros(got.size, dtype=bool)
        for s, size, w in zip(starts, sizes, want):
            assert np.array_equal(got[s:s + size], w.reshape(-1)), name
            covered[s:s + size] = True
        assert (got[~covered] == SENTINEL).all(), f"{name}: a sentinel row was written"


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


def random_state(c, inputs, seed):
    """(clear bits [register][position][input], CudaTriviumState of their encryptions)"""
    rng = np.random.default_rng(seed)
    clear = [rng.integers(0, 2, size=(bits, inputs)) for bits in BITS]
    regs = [c.enc([r.reshape(-1).tolist()], seed + 1 + i, degree=1) for i, r in enumerate(clear)]
    return clear, c.igpu.CudaTriviumState(*regs)


def encrypt_bits(c, rows, seed):
    """rows: [input][80] -> 80 N blocks, bit i of input n at block i N + n"""
    return c.enc([np.asarray(rows).T.reshape(-1).tolist()], seed, degree=1)


def keystream_bits(c, ks, inputs):
    """-> [input][step]"""
    return np.asarray(c.dec(ks)[0]).reshape(-1, inputs).T.tolist()


def check_against_model(c, clear, state, ks, steps, inputs):
    got = keystream_bits(c, ks, inputs)
    regs = [np.asarray(c.dec(r)[0]).reshape(-1, inputs) for r in (state.a, state.b, state.c)]
    for n in range(inputs):
        model = ClearTrivium(*(r[:, n].tolist() for r in clear))
        assert got[n] == model.run(steps), f"keystream of input {n}"
        for name, r, want in zip("abc", regs, (model.a, model.b, model.c)):
            assert r[:, n].tolist() == want, f"register {name} of input {n}"
    for ct in (state.a, state.b, state.c, ks):
        assert (ct.degrees == 1).all() and (ct._info[1] == 1).all()


# ================================================================================== 3. one and two batches
@pytest.mark.parametrize("steps", [64, 128])
@pytest.mark.parametrize("inputs", [1, 2], ids=["1_input", "2_inputs"])
@pytest.mark.parametrize("kind", KINDS)
def test_batches_from_an_arbitrary_state(kind, inputs, steps):
    """Random bits in a, b, c: every register position and every keystream bit decrypts to the model's value (a random
    state reaches every tap and the placement of every new bit), degrees and noise levels are 1, and the published count
    is 512 N bootstraps per batch."""
    c = anchor(kind)
    clear, state = random_state(c, inputs, 700 + 10 * inputs + steps)
    ks, pbs = c.sks.trivium_next(state, steps, c.st, return_pbs_count=True)
    assert pbs == 512 * inputs * (steps // 64)
    assert ks.total_blocks == steps * inputs
    check_against_model(c, clear, state, ks, steps, inputs)


# ================================================================================== 4. re-basing
@pytest.mark.parametrize("kind", KINDS)
def test_rebasing_with_a_window_of_two_batches(kind):
    """Three batches with the window lowered to 2: the third batch runs on re-based tapes."""
    c = anchor(kind)
    clear, state = random_state(c, 1, 740)
    ks = c.sks.trivium_next(state, 192, c.st, _window=2)
    check_against_model(c, clear, state, ks, 192, 1)


@pytest.mark.gpu
def test_rebasing_with_the_default_window():
    """19 batches at one input: the 19th runs after the re-basing that follows a full window of 18."""
    c = anchor("hip")
    clear, state = random_state(c, 1, 750)
    ks, pbs = c.sks.trivium_next(state, 19 * 64, c.st, return_pbs_count=True)
    assert pbs == 19 * 512
    check_against_model(c, clear, state, ks, 19 * 64, 1)


# ================================================================================== 5. the warm-up and the vectors
@pytest.mark.gpu
@pytest.mark.parametrize("vector", VECTORS, ids=[f"vector_{i + 1}" for i in range(len(VECTORS))])
def test_generate_keystream_gives_the_published_bytes(vector):
    c = anchor("hip")
    key, iv = encrypt_bits(c, [hex_bits(vector["key_hex"])], 760), encrypt_bits(c, [hex_bits(vector["iv_hex"])], 761)
    ks = c.sks.trivium_generate_keystream(key, iv, 512, c.st)
    assert bits_hex(keystream_bits(c, ks, 1)[0]) == vector["keystream_hex"]


@pytest.mark.gpu
def test_three_vectors_side_by_side_and_the_count_of_the_warm_up():
    c = anchor("hip")
    three = VECTORS[1:]
    key = encrypt_bits(c, [hex_bits(v["key_hex"]) for v in three], 770)
    iv = encrypt_bits(c, [hex_bits(v["iv_hex"]) for v in three], 771)
    state, pbs = c.sks.trivium_init(key, iv, c.st, return_pbs_count=True)
    assert pbs == 6912 * 3
    assert [r.total_blocks for r in (state.a, state.b, state.c)] == [3 * b for b in BITS]
    for r in (state.a, state.b, state.c):
        assert (r.degrees == 1).all() and (r._info[1] == 1).all()
    ks = c.sks.trivium_next(state, 512, c.st)
    got = keystream_bits(c, ks, 3)
    assert [bits_hex(g) for g in got] == [v["keystream_hex"] for v in three]
    # the registers after warm-up and 512 steps, position by position
    regs = [np.asarray(c.dec(r)[0]).reshape(-1, 3) for r in (state.a, state.b, state.c)]
    for n, v in enumerate(three):
        model = ClearTrivium.from_key_iv(hex_bits(v["key_hex"]), hex_bits(v["iv_hex"]))
        model.run(512)
        assert [r[:, n].tolist() for r in regs] == [model.a, model.b, model.c]


# ================================================================================== 6. stateful = monolithic
@pytest.mark.gpu
def test_stateful_use_equals_monolithic_use():
    """init, then next(64) twice, against generate_keystream(128): the same bits after decryption."""
    c = anchor("hip")
    v = VECTORS[3]
    key, iv = encrypt_bits(c, [hex_bits(v["key_hex"])], 780), encrypt_bits(c, [hex_bits(v["iv_hex"])], 781)
    state = c.sks.trivium_init(key, iv, c.st)
    pieces = [keystream_bits(c, c.sks.trivium_next(state, 64, c.st), 1)[0] for _ in range(2)]
    whole = keystream_bits(c, c.sks.trivium_generate_keystream(key, iv, 128, c.st), 1)[0]
    assert pieces[0] + pieces[1] == whole
    assert bits_hex(whole) == v["keystream_hex"][:32]


# ================================================================================== 7. other key kinds and bases
OTHER = {"multibit_g4_4_4": None, "classic_k2_2_4": None, "classic_8_8": SMALL_8_8}


@pytest.mark.parametrize("base", list(OTHER))
@pytest.mark.parametrize("kind", KINDS)
def test_one_batch_on_other_keys_and_bases(kind, base):
    """A multi-bit key (g = 4) and the bases (2, 4) and (8, 8): one batch from a random state at one input."""
    c = ctx(kind, base, OTHER[base] if kind == "emu" else None)
    clear, state = random_state(c, 1, 800)
    ks, pbs = c.sks.trivium_next(state, 64, c.st, return_pbs_count=True)
    assert pbs == 512
    check_against_model(c, clear, state, ks, 64, 1)


# ================================================================================== 8. sharding
@pytest.mark.parametrize("kind", KINDS)
def test_rounds_sharded_over_the_streams_of_the_set(kind):
    """One stream against three streams on the same GPU at a threshold of 100 blocks per GPU (a round of 256 rows then runs
    as shards of 86, 85 and 85): identical keystream and register words."""
    from .test_radix_integer import setup
    from . import radix_model as rm
    p = SMALL_4_4 if kind == "emu" else BASE["classic_4_4"].emu
    _, keys, st1, sks1, igpu = setup(kind, p)
    _, _, st3, sks3, _ = setup(kind, p, gpu_indexes=(0, 0, 0))
    lib = use_backend(kind)
    rng = np.random.default_rng(820)
    clear = [rng.integers(0, 2, size=(bits, 1)) for bits in BITS]
    words = [rm.encrypt_rows(p, keys, [r.reshape(-1).tolist()], 821 + i) for i, r in enumerate(clear)]
    outs = {}
    for name, st, sks, thr in (("one", st1, sks1, 512), ("three", st3, sks3, 100)):
        lib.hip_integer_set_multi_gpu_threshold(thr)
        try:
            state = igpu.CudaTriviumState(*(igpu.CudaUnsignedRadixCiphertext.from_blocks(w, st) for w in words))
            ks = sks.trivium_next(state, 64, st)
            outs[name] = [ct.to_blocks(st) for ct in (ks, state.a, state.b, state.c)]
        finally:
            lib.hip_integer_set_multi_gpu_threshold(0)
    for one, three in zip(outs["one"], outs["three"]):
        assert np.array_equal(one, three)
    model = ClearTrivium(*(r[:, 0].tolist() for r in clear))
    assert rm.decrypt_many(p, keys, outs["three"][0])[0].tolist() == model.run(64)


# ================================================================================== 9. device = emulation
def one_batch_words(c, words):
    state = c.igpu.CudaTriviumState(*(c.from_words(w, degree=1) for w in words))
    ks = c.sks.trivium_next(state, 64, c.st)
    return [c.words(ct) for ct in (ks, state.a, state.b, state.c)]


@pytest.mark.gpu
def test_device_equals_emulation_word_for_word():
    """The same keys and the same seeded inputs through both backends: one batch with keystream at two inputs."""
    from . import radix_model as rm
    toy = dataclasses.replace(BASE["classic_4_4"], hip=SMALL_4_4, emu=SMALL_4_4)
    rng = np.random.default_rng(840)
    clear = [rng.integers(0, 2, size=(bits, 2)) for bits in BITS]
    try:
        hip = Ctx("hip", toy)
        words = [rm.encrypt_rows(hip.p, hip.keys, [r.reshape(-1).tolist()], 841 + i) for i, r in enumerate(clear)]
        got = one_batch_words(hip, words)
        gc.collect()
        want = one_batch_words(Ctx("emu", toy), words)
    finally:
        use_backend("hip")
    for name, g, w in zip(("keystream", "a", "b", "c"), got, want):
        assert np.array_equal(g, w), f"{name}: the device's words differ from the emulation's"


# ================================================================================== 10. refusals
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
def scratch(kind, inputs=1, msg=4, carry=4):
    mem = C.c_void_p()
    getattr(lib, f"hip_scratch_trivium_{kind}_async")(s, C.byref(mem), BK, KK, msg, carry, True, 0, inputs)
    return mem
"""

REFUSALS = {
    "base (2, 2)": ("""
        scratch("step", msg=2, carry=2)
        """, "trivium_step: moduli (2, 2) do not hold the value and noise level 5 a row reaches"),
    "a register block of degree 2": ("""
        lib.hip_trivium_step_async(s, radix(64), radix(93), radix(84, degree=2), radix(111), 1, 64, scratch("step"), keys, keys)
        """, "trivium_step: block 0 of register b has degree 2, a bit has at most 1"),
    "num_steps = 65": ("""
        lib.hip_trivium_step_async(s, radix(65), radix(93), radix(84), radix(111), 1, 65, scratch("step"), keys, keys)
        """, "trivium_step: num_steps 65 is not a multiple of 64"),
    "a key of 79 blocks": ("""
        lib.hip_trivium_init_async(s, radix(93), radix(84), radix(111), radix(79), radix(80), 1, scratch("init"), keys, keys)
        """, "trivium_init: the key holds 79 blocks, 80 bits of 1 inputs are 80"),
    "a call with another number of inputs than the scratch": ("""
        lib.hip_trivium_step_async(s, radix(128), radix(186), radix(168), radix(222), 2, 64, scratch("step", inputs=1), keys, keys)
        """, "trivium_step: 2 inputs on a scratch created for 1"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_misuse_is_refused_with_a_message(name):
    """On the host emulation only, in a child process: the library aborts with a message that names the entry point."""
    snippet, message = REFUSALS[name]
    r = run_child(PRELUDE + textwrap.dedent(snippet))
    assert r.returncode == -signal.SIGABRT, f"{name}: returned {r.returncode}\n{r.stderr[-600:]}"
    assert message in r.stderr, r.stderr[-600:]
