"""Multiplication of radix integers by a clear scalar (hip_*_integer_scalar_mul_64) and what sits on it: the shared
column-sum planner (progress, termination, bootstrap counts), the host shortcuts, every shape of scalar the flow tells
apart, batches in both planner modes, every propagating base, the device against the emulation word for word, and the
custom-range OPRF composed from OPRF bits, this multiplication and a right shift.

The checker is clear big-integer arithmetic on the decrypted blocks; nothing reads the library's tables.
[emu] runs the kernel sources on the host, [hip] on the MI355X; toy keys except on the anchor row of [hip]."""
import ctypes as C
import dataclasses
import gc

import numpy as np
import pytest

from . import oprf_helper as oh
from . import radix_model as rm
from .common import C1, TOY_2048, make_keys
from .harness import use_backend
from .test_radix_bases import BASES, Ctx, cases

U64 = np.uint64
ANCHOR = cases(BASES[:1])
BY_NAME = {b.name: b for b in BASES}


def bits_of(scalar):
    return np.array([(scalar >> i) & 1 for i in range(max(1, scalar.bit_length()))], dtype=U64)


class Scratch:
    """one scalar-multiplication scratch, used through the raw C entry points (several calls on the same scratch)"""

    def __init__(self, c, L, batch=1, scalar_bits=64):
        self.c, self.L, self.lib = c, L, use_backend(c.kind)
        self.s, self.keep = c.sks._streams(c.st)
        self.mem = C.c_void_p()
        self.lib.hip_integer_scratch_batch(batch)
        self.lib.hip_scratch_integer_scalar_mul_64_async(
            self.s, C.byref(self.mem), c.sks._bsk_params(), c.sks._ksk_params(), L, c.msg, c.carry, scalar_bits, True,
            c.sks._noise_reduction())
        self.lib.hip_integer_scratch_batch(1)

    def pbs_count(self, scalar):
        b = bits_of(scalar)
        return int(self.lib.hip_integer_scalar_mul_pbs_count(self.mem, b.ctypes.data_as(C.c_void_p), len(b)))

    def mul(self, ct, scalar):
        b = bits_of(scalar)
        bits = self.c.msg.bit_length() - 1
        has = np.zeros(bits, dtype=U64)
        for i, v in enumerate(b):
            if v:
                has[i % bits] = 1
        ksks, bsks = self.c.sks._key_ptrs(self.c.st)
        self.lib.hip_integer_scalar_mul_64_async(
            self.s, C.byref(ct._ffi()), b.ctypes.data_as(C.c_void_p), has.ctypes.data_as(C.c_void_p), self.mem, bsks, ksks,
            self.c.sks.bootstrapping_key.polynomial_size, self.c.msg, len(b))

    def close(self):
        self.lib.hip_cleanup_integer_scalar_mul_64(self.s, C.byref(self.mem))


def check(c, ct, rows, scalar, L, what=""):
    """the clean product of every integer: digits below msg, degrees msg - 1, nominal noise"""
    m = c.msg
    got = c.dec(ct)
    want = [rm.digits((rm.value(r, m) * scalar) % m ** L, L, m) for r in rows]
    assert got == want, (what, scalar, rows, got)
    assert list(ct.degrees) == [m - 1] * (L * len(rows)), (what, scalar)
    assert list(ct._info[1]) == [1] * (L * len(rows)), (what, scalar)


# ================================================================================== planner, host only
PLANNER = [("classic_4_4", 5, 1023), ("classic_4_4", 5, 0x2D3), ("classic_8_8", 5, 1023), ("classic_8_8", 5, 0x2D3),
           ("classic_8_8", 4, 0xFFF), ("classic_4_16", 5, 1023), ("classic_4_16", 5, 0x2D3)]


@pytest.mark.parametrize("batch", [1, 8], ids=["few_integers", "many_integers"])
@pytest.mark.parametrize("name,L,scalar", PLANNER, ids=[f"{n}-{L}_blocks-{s:#x}" for n, L, s in PLANNER])
def test_planner_makes_progress_and_terminates(name, L, scalar, batch):
    """Every plan ends.  (4, 16), many integers, 1023 leaves a column as the two terms [15, 3]: the step that would emit
    nothing emits every group of two."""
    c = Ctx("emu", BY_NAME[name])
    sc = Scratch(c, L, batch, scalar_bits=L * (c.msg.bit_length() - 1))
    try:
        n = sc.pbs_count(scalar)
        print(name, L, hex(scalar), "batch", batch, "->", n, "bootstraps per integer")
        assert n > 0
        assert sc.pbs_count(scalar) == n, "the cached plan gives another count"
    finally:
        sc.close()


@pytest.mark.parametrize("batch,mult", [(1, 1804), (8, 1762)], ids=["few_integers", "many_integers"])
def test_bootstrap_counts_of_a_64_bit_multiplication(batch, mult):
    c = Ctx("emu", BASES[0])
    lib = use_backend("emu")
    s, keep = c.sks._streams(c.st)
    mem = C.c_void_p()
    lib.hip_integer_scratch_batch(batch)
    lib.scratch_cuda_integer_mult_inplace_64_async(s, C.byref(mem), False, False, 4, 4, c.sks._bsk_params(),
                                                   c.sks._ksk_params(), 32, True, c.sks._noise_reduction())
    lib.hip_integer_scratch_batch(1)
    ct_ct = int(lib.hip_integer_mult_pbs_count(mem))
    lib.cleanup_cuda_integer_mult_inplace_64(s, C.byref(mem))
    assert ct_ct == mult, "the multiplication's plan changed"
    sc = Scratch(c, 32, batch)
    try:
        ones = sc.pbs_count((1 << 64) - 1)
        three = sc.pbs_count(3)
        print("all-ones scalar:", ones, "scalar 3:", three, "ciphertext x ciphertext:", ct_ct)
        assert ones < ct_ct
        assert three == 32 + lib.hip_integer_propagate_pbs_count(32)
        assert sc.pbs_count(0) == 0
        assert sc.pbs_count(1 << 7) == 32 - 3, "a power of two inside a block: its shifted blocks and nothing else"
        assert sc.pbs_count(1 << 8) == 0, "a whole-block power of two moves index entries"
    finally:
        sc.close()


# ================================================================================== scalar multiplication, anchor base
SCALARS = [0, 1, 2, 4, 3, 0x155, 0x2AA, 0x2D3, 1023, (1 << 12) | 5]


def anchor_rows(m, L):
    rng = np.random.default_rng(511)
    return [[m - 1] * L, [0] * L, [1] + [0] * (L - 1)] + [[int(v) for v in rng.integers(0, m, size=L)] for _ in range(2)]


@pytest.mark.parametrize("scalar", SCALARS, ids=[f"{s:#x}" for s in SCALARS])
@pytest.mark.parametrize("kind,base", ANCHOR)
def test_scalar_mul_of_every_shape_of_scalar(kind, base, scalar):
    """The five operands as one batch (one call); and the first random operand alone, where 0, 1 and the powers of two take
    the host's shortcuts (memset, nothing, a left shift)."""
    c, m, L = Ctx(kind, base), base.msg, 5
    rows = anchor_rows(m, L)
    ct = c.enc(rows, 512)
    pbs = c.sks.scalar_mul_assign(ct, scalar, c.st, return_pbs_count=True)
    print(f"scalar {scalar:#x}: {pbs} bootstraps per integer")
    if scalar == 0:
        assert c.dec(ct) == [[0] * L] * len(rows) and list(ct.degrees) == [0] * (L * len(rows)) and pbs == 0
    elif scalar == 1:
        assert c.dec(ct) == rows and pbs == 0
    else:
        check(c, ct, rows, scalar, L, "batch")
    one = c.enc(rows[3:4], 513)
    before = c.words(one)
    out = c.sks.unchecked_scalar_mul(one, scalar, c.st)
    assert np.array_equal(c.words(one), before) and list(one.degrees) == [m - 1] * L, "the copying form touched its input"
    assert c.dec(out) == [rm.digits((rm.value(rows[3], m) * scalar) % m ** L, L, m)], scalar


@pytest.mark.parametrize("kind,base", ANCHOR)
def test_plan_cache_serves_the_same_scalar_again_and_replans_for_another(kind, base):
    c, m, L = Ctx(kind, base), base.msg, 5
    rows = anchor_rows(m, L)[3:]
    sc = Scratch(c, L, batch=2, scalar_bits=10)
    try:
        for n, scalar in enumerate([0x2D3, 0x2D3, 1023, 0x155, 0x2D3, 0]):
            ct = c.enc(rows, 520 + n)
            sc.mul(ct, scalar)
            if scalar:
                check(c, ct, rows, scalar, L, f"call {n}")
            else:
                assert c.dec(ct) == [[0] * L] * 2 and list(ct.degrees) == [0] * (2 * L)
        one = c.enc(rows[:1], 530)             # fewer integers than the call before: the index arrays are rebuilt
        sc.mul(one, 1023)
        check(c, one, rows[:1], 1023, L, "one integer after two")
    finally:
        sc.close()


@pytest.mark.parametrize("count,L", [(3, 5), (8, 4)], ids=["3_integers_few_mode", "8_integers_many_mode"])
@pytest.mark.parametrize("kind,base", ANCHOR)
def test_scalar_mul_of_a_batch(kind, base, count, L):
    c, m = Ctx(kind, base), base.msg
    rng = np.random.default_rng(540 + count)
    rows = [[m - 1] * L] + [[int(v) for v in rng.integers(0, m, size=L)] for _ in range(count - 1)]
    for n, scalar in enumerate([m ** L - 1, 0x2D3, 4]):
        ct = c.enc(rows, 541 + n)
        c.sks.scalar_mul_assign(ct, scalar, c.st)
        check(c, ct, rows, scalar, L, f"{count} integers")


@pytest.mark.parametrize("kind,base", cases([b for b in BASES[1:] if b.propagates]))
def test_scalar_mul_at_every_propagating_base(kind, base):
    """(8, 8): both shifted planes; (4, 16): 21 terms per group; multi-bit keys.  All digits msg - 1 and a random operand."""
    c, m, L = Ctx(kind, base), base.msg, 4
    rng = np.random.default_rng(550)
    rows = [[m - 1] * L, [int(v) for v in rng.integers(0, m, size=L)]]
    for n, scalar in enumerate([m ** L - 1, 0x2D3, 3]):
        ct = c.enc(rows, 551 + n)
        c.sks.scalar_mul_assign(ct, scalar, c.st)
        check(c, ct, rows, scalar, L, base.name)


# ================================================================================== device equals emulation
PARITY = [BY_NAME[n] for n in ("classic_4_4", "classic_8_8", "classic_4_16", "multibit_g4_4_4")]


@pytest.mark.gpu
@pytest.mark.parametrize("base", PARITY, ids=[b.name for b in PARITY])
def test_device_equals_emulation_word_for_word(base):
    p = base.hip if base.hip is not C1 else base.emu       # toy keys on both sides
    toy = dataclasses.replace(base, hip=p, emu=p)
    keys = make_keys(p)
    L, m = 4, base.msg
    rng = np.random.default_rng(561)
    rows = [[m - 1] * L] + [[int(v) for v in rng.integers(0, m, size=L)] for _ in range(5)]
    words = rm.encrypt_rows(p, keys, rows, 562)

    def sequence(c):
        out = []
        ct = c.from_words(words[:2])
        c.sks.scalar_mul_assign(ct, 0x2D3, c.st)
        out.append(("scalar_mul", c.words(ct), list(ct.degrees)))
        total = c.sks.sum_ciphertexts([c.from_words(words[i:i + 1]) for i in range(6)], c.st)
        out.append(("sum", c.words(total), list(total.degrees)))
        return out

    try:
        got = sequence(Ctx("hip", toy))
        gc.collect()
        want = sequence(Ctx("emu", toy))
    finally:
        use_backend("hip")
    for (name, w_hip, d_hip), (_, w_emu, d_emu) in zip(got, want):
        assert np.array_equal(w_hip, w_emu), f"{name}: the device's words differ from the emulation's"
        assert d_hip == d_emu, name
    assert [rm.value(r, m) for r in rm.decrypt_many(p, keys, got[0][1]).tolist()] == \
        [(rm.value(r, m) * 0x2D3) % m ** L for r in rows[:2]]
    assert rm.value(rm.decrypt_many(p, keys, got[1][1]).tolist()[0], m) == sum(rm.value(r, m) for r in rows) % m ** L


# ================================================================================== custom-range OPRF
RANGE = [(5, 2), (5, 5), (5, 7), (6, 5), (8, 2), (8, 5), (8, 7)]


@pytest.mark.parametrize("bound,blocks_out", RANGE, ids=[f"below_{b}-{n}_blocks" for b, n in RANGE])
@pytest.mark.parametrize("kind", [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
def test_custom_range_oprf_is_the_scaled_random_value(kind, bound, blocks_out):
    """6 random bits r; the result is (r * bound) >> 6, on 2, 5 (the intermediate width for these bounds) and 7 blocks."""
    from .test_radix_integer import setup
    p, keys, st, sks, igpu = setup(kind, TOY_2048)
    nbits, m = 6, 4
    assert -(-(nbits + bound.bit_length()) // 2) == 5
    lwes = oh.seeded_lwes(p.n, p.N, 3, 400)
    xs = oh.input_cleartexts(lwes, keys.lwe_sk, p.N)
    r = sum(oh.cleartext_prf(x, 2, 2 * m * m, p.N) << (2 * i) for i, x in enumerate(xs))
    rerand = None
    if (bound, blocks_out) == (6, 5):
        from .test_rerand import rerand_key_and_zeros
        key, zeros = rerand_key_and_zeros(p, keys, igpu, st, "without_ks", 3, 308)
        rerand = (zeros, key)
    out = igpu.CudaOprfServerKey(sks.bootstrapping_key).generate_oblivious_pseudo_random_unsigned_custom_range(
        lwes, nbits, bound, blocks_out, sks, st, rerand=rerand)
    assert out.num_integers == 1 and out.num_blocks == blocks_out
    got = rm.decrypt_many(p, keys, out.to_blocks(st)).tolist()[0]
    want = (r * bound) >> nbits
    print("random value", r, "bound", bound, "->", want, "blocks", got)
    assert want < bound
    assert got == rm.digits(want % m ** blocks_out, blocks_out, m)
    assert all(d <= m - 1 for d in out.degrees)
