"""Encrypted integer division: div_rem signed and unsigned, abs, and the stage kernel under the loop.

The checker is Python integer arithmetic on the decrypted blocks.  A clear model of the loop (ClearDivision below) tells
which inputs every table of the loop was asked; nothing of it reads the library's tables.  The pairs a test divides are
chosen so that, by the model alone, they reach every (table, input) that ALL pairs of the shape reach.
[emu] runs the kernel sources on the host, [hip] on the MI355X; toy keys, the anchor on the MI355X with
PARAM_MESSAGE_2_CARRY_2.  The emulation takes 32 (16) chosen pairs where the MI355X takes all 256; five blocks (345
bootstraps per division) run on the MI355X only."""
import ctypes as C
import dataclasses
import functools
import gc
import os
import signal
import textwrap

import numpy as np
import pytest

from . import radix_model as rm
from .common import C1, Params, make_keys
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_bases import BASES, Ctx

U64 = np.uint64
BASE = {b.name: b for b in BASES}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]

# the emulation runs a fibre per lane: it takes the smallest polynomial that holds the plaintext space
EMU_SMALL = {
    "classic_4_4": Params("toy_k1_N512_l1_p16", 8, 1, 512, 23, 1, 4, 4, 45, 17, 16, ms_type=1),
    "classic_8_8": Params("toy_k1_N1024_l1_p64", 8, 1, 1024, 23, 1, 4, 4, 45, 17, 64, ms_type=1),
    "classic_4_16": Params("toy_k1_N1024_l1_p64", 8, 1, 1024, 23, 1, 4, 4, 45, 17, 64, ms_type=1),
    "multibit_g4_4_4": Params("toy_multibit_g4_N512_p16", 8, 1, 512, 15, 2, 3, 6, 45, 17, 16, grouping=4),
}


# ================================================================================== 1. the kernel alone
SENTINEL = U64(0xA5A5A5A55A5A5A5A)
MSG = 4
ALL_ONES = 2 ** 64 - 1
WORDS = (1, 5, 511, 512, 513, 2049)      # the edges of a 512-word slice, the odd production row


@dataclasses.dataclass
class Term:
    src: str
    scalar: int
    offset: int = 0
    step: int = 1
    stand: str = None
    stand_row: int = 0


@dataclasses.dataclass
class Group:
    rows: int
    terms: list
    first: int = 0
    constant: int = 0
    stride: int = None        # of the output array; None: the group's rows, dense
    first_out: int = 0


SOURCE_ROWS = {"x": 6, "y": 6, "flag": 1, "up": 3, "num": 3}


def kernel_tables():
    """name -> groups.  Every source kind (offset -1 with and without a stand-in row, offset 0, offset + 1, broadcast), the
    body constant present and absent, the scalars 1, msg, msg - 1 and 2^64 - 1, 1 to 4 groups of 1, 2 and 5 rows with 0 to 4
    terms, a group that starts above row 0 and one whose output array is wider than the group."""
    return {
        "one_group_one_term": [Group(5, [Term("x", 1)])],
        "shift_pairs_with_and_without_a_stand_in_row": [
            Group(5, [Term("x", MSG), Term("x", 1, -1, stand="num", stand_row=2)]),
            Group(2, [Term("y", MSG), Term("y", 1, -1)])],
        "merged_and_subtraction_input_with_a_constant_above": [
            Group(2, [Term("x", 1), Term("y", 1)]),
            Group(1, [Term("x", 1), Term("y", 1), Term("x", ALL_ONES, 3)], stride=5, first_out=0),
            Group(2, [Term("x", 1), Term("y", 1), Term("y", ALL_ONES, 1)], first=1, stride=6, first_out=1),
            Group(2, [], first=3, constant=(MSG - 1) << 59, stride=6, first_out=3)],
        "select_inputs_with_broadcast_flags": [
            Group(5, [Term("x", 3), Term("flag", ALL_ONES, 0, 0), Term("up", 1, 2, 0)], constant=1 << 59),
            Group(5, [Term("y", 3), Term("flag", ALL_ONES, 0, 0), Term("up", 1, 2, 0)], constant=1 << 59),
            Group(1, [Term("flag", ALL_ONES, 0, 0), Term("up", 1, 2, 0)], constant=1 << 59)],
        "four_groups_of_four_terms_and_unequal_rows": [
            Group(1, [Term("x", 1, 5), Term("y", MSG - 1, 0), Term("up", 1, 1, 0), Term("num", MSG, 2)]),
            Group(2, [Term("x", MSG - 1, 2), Term("x", 1, -1, stand="flag"), Term("y", ALL_ONES, 0), Term("flag", MSG, 0, 0)],
                  constant=7),
            Group(5, [Term("y", 1, 1), Term("y", 1, 0), Term("x", MSG, -1, stand="up", stand_row=1), Term("x", MSG - 1, 0)]),
            Group(2, [Term("x", 1, 0), Term("y", 1, -1), Term("up", ALL_ONES, 0, 0), Term("num", 1, 0)], first=1,
                  constant=ALL_ONES)],
    }


def divrem_model(src, groups, batch, words):
    """src: name -> [batch][rows][words] u64; the kernel's formula in NumPy (u64 arithmetic wraps modulo 2^64)"""
    out = []
    for g in groups:
        o = np.zeros((batch, g.rows, words), dtype=U64)
        for c in range(batch):
            for r in range(g.rows):
                j = g.first + r
                for t in g.terms:
                    row = j * t.step + t.offset
                    if row >= 0:
                        o[c, r] += U64(t.scalar) * src[t.src][c, row]
                    elif t.stand is not None:
                        o[c, r] += U64(t.scalar) * src[t.stand][c, t.stand_row]
                o[c, r, -1:] += U64(g.constant)      # (arrays wrap silently)
        out.append(o)
    return out


def launch_table(lib, st, words, batch, groups, outs, d_src):
    """groups on device arrays: outs[g] the output array's first word, d_src name -> CudaVec"""
    G = len(groups)
    c_outs, consts, gu = (C.c_void_p * G)(*outs), (C.c_uint64 * G)(*[g.constant for g in groups]), (C.c_uint32 * (6 * G))()
    srcs, stands, scal, tu = (C.c_void_p * (4 * G))(), (C.c_void_p * (4 * G))(), (C.c_uint64 * (4 * G))(), (C.c_uint32 * (24 * G))()
    for i, g in enumerate(groups):
        stride = g.rows if g.stride is None else g.stride
        gu[6 * i:6 * i + 6] = [stride, stride, g.first_out, g.first, g.rows, len(g.terms)]
        for k, t in enumerate(g.terms):
            srcs[4 * i + k], scal[4 * i + k] = d_src[t.src].ptr, t.scalar
            stands[4 * i + k] = d_src[t.stand].ptr if t.stand else None
            rows = SOURCE_ROWS[t.src]
            tu[6 * (4 * i + k):6 * (4 * i + k) + 6] = [rows, rows, t.offset & 0xFFFFFFFF, t.step,
                                                      SOURCE_ROWS[t.stand] if t.stand else 0, t.stand_row]
    lib.hip_test_divrem_sum_async(st.ptr[0], 0, words, batch, G, c_outs, consts, gu, srcs, stands, scal, tu)


@pytest.mark.parametrize("batch", [1, 3], ids=["batch_1", "batch_3"])
@pytest.mark.parametrize("words", WORDS, ids=[f"{w}_words" for w in WORDS])
@pytest.mark.parametrize("kind", KINDS)
def test_stage_kernel_equals_numpy_word_for_word(kind, words, batch):
    """hip_test_divrem_sum_async against the formula on random u64 words, every table of kernel_tables().  Every group's
    output array sits between sentinel rows, and the rows of a wider output array that the group does not own are sentinels
    too: all of them must stay as they are."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    lib = use_backend(kind)
    st = gpu.CudaStreams((0,))
    rng = np.random.default_rng(100 * words + batch)
    src = {name: rng.integers(0, 2 ** 64, size=(batch, rows, words), dtype=U64) for name, rows in SOURCE_ROWS.items()}
    d_src = {name: gpu.CudaVec.from_cpu_async(a.reshape(-1), st) for name, a in src.items()}
    guard = 2 * words
    for name, groups in kernel_tables().items():
        assert 1 <= len(groups) <= 4 and all(len(g.terms) <= 4 for g in groups)
        starts, at = [], 0
        for g in groups:
            starts.append(at + guard)
            at += guard + batch * (g.rows if g.stride is None else g.stride) * words
        frame = np.full(at + guard, SENTINEL, dtype=U64)
        d_out = gpu.CudaVec.from_cpu_async(frame, st)
        launch_table(lib, st, words, batch, groups, [d_out.ptr + 8 * s for s in starts], d_src)
        got = d_out.copy_to_cpu(st)
        covered = np.zeros(got.size, dtype=bool)
        for g, s, want in zip(groups, starts, divrem_model(src, groups, batch, words)):
            stride = g.rows if g.stride is None else g.stride
            for c in range(batch):
                lo = s + (c * stride + g.first_out) * words
                assert np.array_equal(got[lo:lo + g.rows * words], want[c].reshape(-1)), (name, c)
                covered[lo:lo + g.rows * words] = True
        assert (got[~covered] == SENTINEL).all(), f"{name}: a sentinel row was written"


# ================================================================================== the clear model of the loop
def propagate_pbs(L):
    """bootstraps of the carry look-ahead on L blocks (the comment that opens the carry propagation in integer.hip)"""
    if L == 1:
        return 1
    n = [L]
    while n[-1] > 4:
        n.append((n[-1] + 2) // 3)
    top = len(n) - 1
    count = 2 * L + sum(n[l] - 1 for l in range(1, top + 1)) + (L // 3 if top >= 1 else 0) + n[top] - 1
    return count + sum(n[l] - (n[l] + 2) // 3 for l in range(1, top))


def division_pbs(signed, L, b):
    """the closed formula of docs/history/div_rem_log.md"""
    B, lg = b * L, (L - 1).bit_length()
    n = (2 * b - 1) * L + L * lg + (b - 1) * L + 5 * b * L * (L + 1) // 2 + B * (2 + propagate_pbs(L)) + 2 * L
    if signed:
        n += 2 * (1 + propagate_pbs(L) + L) + 1 + 2 * (propagate_pbs(L) + L)
    return n


class ClearDivision:
    """The rounds of one division on clear blocks: which inputs the shift tables, the divisor's masks and flags, the cleaning
    table, both zero-out tables at their factor and the quotient-bit table see, and what comes out."""

    def __init__(self, bits_per_block, blocks):
        self.b, self.L, self.B, self.msg = bits_per_block, blocks, bits_per_block * blocks, 1 << bits_per_block

    def unsigned(self, n, d, seen):
        b, L, B, msg = self.b, self.L, self.B, self.msg
        N, D = rm.digits(n, L, msg), rm.digits(d, L, msg)
        for x in D:
            for t in range(1, b):
                seen.add(("low", t, x))
            for t in range(b):
                seen.add(("high", t, x))
        z, k = [int(x != 0) for x in D], 1
        while k < L:                                   # "a block at or above j is non-zero"
            sums = [z[j] + (z[j + k] if j + k < L else 0) for j in range(L)]
            seen.update(("nonzero", x) for x in sums)
            z, k = [int(x != 0) for x in sums], 2 * k
        z = z + [0]
        upper = {}
        for t in range(1, b):
            for j in range(L):
                x = int((D[j] >> t) != 0) + (z[j + 1] if L > 1 else 0)
                seen.add(("nonzero", x))
                upper[(t, j)] = int(x != 0)
        r1, r2, q = [0] * L, [0] * L, 0
        for s in range(B):
            blocks, i = s // b + 1, B - 1 - s
            pos, blk, f = i % b, i // b, 2 if s == B - 1 else 3
            s1, s2 = [], []
            for j in range(blocks):
                below, p = (N[blk], pos) if j == 0 else (r1[j - 1], b - 1)
                seen.add(("shift", p, msg * r1[j] + below))
                s1.append(((r1[j] << 1) | ((below >> p) & 1)) % msg)
                below = 0 if j == 0 else r2[j - 1]
                seen.add(("shift", b - 1, msg * r2[j] + below))
                s2.append(((r2[j] << 1) | ((below >> (b - 1)) & 1)) % msg)
            merged = [x + y for x, y in zip(s1, s2)]
            assert all(x < msg for x in merged)
            seen.update(("clean", x) for x in merged)
            value, trimmed = rm.value(merged, msg), d & ((1 << (s + 1)) - 1)
            borrow = int(value < trimmed)
            new = rm.digits((value - trimmed) % msg ** blocks, blocks, msg)
            t, j = (s + 1) % b, (s + 1) // b
            above = 0 if s == B - 1 else (upper[(t, j)] if t else z[j])
            assert above == int((d >> (s + 1)) != 0)
            flags = borrow + above
            for x, y in zip(merged, new):
                seen.add(("keep", f, f * x + flags))
                seen.add(("zero", f, f * y + flags))
            seen.add(("bit", pos, flags))
            if flags:
                r1[:blocks], r2[:blocks] = merged, [0] * blocks
            else:
                r1[:blocks], r2[:blocks] = [0] * blocks, new
                q |= 1 << i
        return q, rm.value(r1, msg) + rm.value(r2, msg)

    def signed(self, n, d, seen):
        """n, d: two's complement patterns"""
        B, L, msg = self.B, self.L, self.msg
        full = (1 << B) - 1

        def negate_where(v, mask):           # (v + mask) ^ mask, mask one block, the same in every block
            m = full if mask else 0
            s = (v + m) & full
            seen.update(("xor", msg * x + mask) for x in rm.digits(s, L, msg))
            return s ^ m

        masks = []
        for v in (n, d):
            top = rm.digits(v, L, msg)[-1]
            seen.add(("sign", top))
            masks.append(msg - 1 if top >> (self.b - 1) else 0)
        q, r = self.unsigned(negate_where(n, masks[0]), negate_where(d, masks[1]), seen)
        seen.add(("differ", masks[0] + masks[1]))
        return negate_where(q, msg - 1 if masks[0] != masks[1] else 0), negate_where(r, masks[0])

    def run(self, n, d, signed, seen):
        return self.signed(n, d, seen) if signed else self.unsigned(n, d, seen)


def expected(n, d, B, signed):
    """Python integers: (quotient, remainder) as B-bit patterns"""
    full = (1 << B) - 1
    if not signed:
        return (full, n) if d == 0 else (n // d, n % d)
    sn, sd = (n - (1 << B) if n >> (B - 1) else n), (d - (1 << B) if d >> (B - 1) else d)
    if sd == 0:             # what the sequence |n| / 0 = all ones, negated when the numerator is negative, yields
        return (1 if sn < 0 else full), n
    q = abs(sn) // abs(sd) * (1 if (sn < 0) == (sd < 0) else -1)
    return q & full, (sn - q * sd) & full


@functools.lru_cache(maxsize=None)
def census(b, L, signed, sample=None):
    """every (table, input) the loop asks over ALL operand pairs of the shape (over `sample` seeded pairs where the shape
    has more than 2^16), and per pair what it reaches; the model itself is checked against plain arithmetic on the way"""
    model = ClearDivision(b, L)
    B = b * L
    if sample is None:
        pairs = [(n, d) for n in range(1 << B) for d in range(1 << B)]
    else:
        rng = np.random.default_rng(B)
        pairs = [(int(n), int(d) >> int(k)) for n, d, k in zip(rng.integers(0, 1 << B, sample), rng.integers(0, 1 << B, sample),
                                                             rng.integers(0, B + 1, sample))]
    reach, everything = {}, set()
    for n, d in pairs:
        seen = set()
        assert model.run(n, d, signed, seen) == expected(n, d, B, signed), (n, d, signed)
        reach[(n, d)] = frozenset(seen)
        everything |= seen
    return everything, reach


def choose_pairs(b, L, signed, count, must=(), sample=None, at_most=True):
    """`count` pairs that reach every entry of the census: the pairs of `must`, then greedily the pair that adds most (first
    in order on a tie), then seeded draws up to `count`.  at_most=False: as many pairs as reaching every entry takes"""
    everything, reach = census(b, L, signed, sample)
    chosen, covered = [], set()
    for p in must:
        chosen.append(p)
        covered |= reach[p] if p in reach else set()
    order = list(reach)
    while covered != everything:
        best = max(order, key=lambda p: len(reach[p] - covered))
        chosen.append(best)
        covered |= reach[best]
    assert not at_most or len(chosen) <= count, f"{len(chosen)} pairs are needed to reach every table entry, {count} are allowed"
    rng = np.random.default_rng(7 * b + L)
    while len(chosen) < count:
        p = order[int(rng.integers(0, len(order)))]
        if p not in chosen:
            chosen.append(p)
    return chosen


def signed_must(B):
    """MIN / -1, x / 0 for x < 0, x = 0 and x > 0, the four sign combinations with a non-zero remainder"""
    full, low = (1 << B) - 1, 1 << (B - 1)
    return [(low, full), (full - 2, 0), (0, 0), (3, 0), (7 % low, 2), (7 % low, full - 1), (full - 6, 2), (full - 6, full - 1)]


def reached(b, L, signed, pairs):
    model, seen = ClearDivision(b, L), set()
    for n, d in pairs:
        model.run(n, d, signed, seen)
    return seen


# ================================================================================== contexts and the checked call
_ctx = {}


def ctx(kind, base_name, production=False):
    key = (kind, base_name, production)
    if key not in _ctx:
        base = BASE[base_name]
        if not production:
            base = dataclasses.replace(base, hip=EMU_SMALL.get(base_name, base.emu) if base.hip is C1 else base.hip,
                                       emu=EMU_SMALL.get(base_name, base.emu))
        _ctx[key] = Ctx(kind, base)
    use_backend(kind)
    return _ctx[key]


def check_division(c, L, pairs, signed, seed):
    """one batched call over `pairs`: quotient, remainder, degrees, noise levels, the operands untouched, the count"""
    m, b = c.msg, c.base.bits
    B = b * L
    num = c.enc([rm.digits(n, L, m) for n, _ in pairs], seed)
    den = c.enc([rm.digits(d, L, m) for _, d in pairs], seed + 1)
    before = c.words(num), c.words(den)
    q, r, pbs = c.sks.div_rem(num, den, c.st, signed=signed, return_pbs_count=True)
    lib = use_backend(c.kind)
    assert pbs == len(pairs) * lib.hip_integer_div_rem_pbs_count(signed, L, m, c.carry) == len(pairs) * division_pbs(signed, L, b)
    rows_q, rows_r = c.dec(q), c.dec(r)
    assert all(0 <= x < m for row in rows_q + rows_r for x in row)
    got = [(rm.value(x, m), rm.value(y, m)) for x, y in zip(rows_q, rows_r)]
    want = [expected(n, d, B, signed) for n, d in pairs]
    wrong = [(p, g, w) for p, g, w in zip(pairs, got, want) if g != w]
    assert not wrong, f"(numerator, divisor), got, expected: {wrong[:8]}"
    for ct in (q, r):
        assert list(ct.degrees) == [m - 1] * (L * len(pairs)) and list(ct._info[1]) == [1] * (L * len(pairs))
    assert np.array_equal(c.words(num), before[0]) and np.array_equal(c.words(den), before[1]), "an operand was touched"
    return q, r


# ================================================================================== 2. unsigned division
def test_the_formula_of_the_bootstrap_count():
    """FheUint64 at PARAM_MESSAGE_2_CARRY_2: the figures the log states"""
    assert propagate_pbs(32) == 97
    assert division_pbs(False, 32, 2) == 96 + 160 + 32 + 5280 + 64 * 99 + 64
    assert division_pbs(True, 32, 2) == division_pbs(False, 32, 2) + 2 * 130 + 1 + 2 * 129


@pytest.mark.gpu
@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
def test_all_256_pairs_in_one_call_on_the_device(signed):
    """(4, 4), two blocks: every (numerator, divisor) of 0 .. 15 (-8 .. 7 when signed), zero divisors included, in ONE
    batched call"""
    check_division(ctx("hip", "classic_4_4"), 2, [(n, d) for n in range(16) for d in range(16)], signed, 600)


UNSIGNED_SHAPES = [  # (blocks, pairs, kinds)
    (2, 32, ("emu", "hip")),
    (1, 16, ("emu", "hip")),            # one block has 16 pairs: all of them
    (3, 32, ("emu", "hip")),            # 6 bits: an odd block count
    (5, 16, ("hip",)),                  # two levels of the carry tree; 345 bootstraps per division: the MI355X only
]


def unsigned_pairs(L, count):
    if L == 1:
        return [(n, d) for n in range(4) for d in range(4)]
    B = 2 * L
    must = [(0, 0), ((1 << B) - 1, 0), ((1 << B) - 1, 1), ((1 << B) - 1, (1 << B) - 1), (1, (1 << B) - 1)]
    return choose_pairs(2, L, False, count, must, sample=4096 if L >= 5 else None)


@pytest.mark.parametrize("kind,L,count", [pytest.param(k, L, n, id=f"{k}-{L}_blocks", marks=[pytest.mark.gpu] if k == "hip" else [])
                                          for L, n, kinds in UNSIGNED_SHAPES for k in kinds])
def test_unsigned_division_of_chosen_pairs(kind, L, count):
    """(4, 4): 32 chosen pairs at one, two and three blocks (one block has 16 pairs: all), 16 at five blocks; zero divisors,
    the largest numerator and divisor among them"""
    check_division(ctx(kind, "classic_4_4"), L, unsigned_pairs(L, count), False, 610 + L)


# ================================================================================== 3. signed division, abs
@pytest.mark.parametrize("kind", KINDS)
def test_signed_division_of_chosen_pairs(kind):
    """(4, 4), two blocks: 32 pairs of -8 .. 7 with MIN / -1, x / 0 for x < 0, x = 0, x > 0 and the four sign combinations
    with a non-zero remainder.  What the sequence yields on a zero divisor: quotient 1 for a negative numerator, -1 otherwise,
    remainder = numerator."""
    pairs = choose_pairs(2, 2, True, 32, signed_must(4))
    assert expected(8, 15, 4, True) == (8, 0) and expected(13, 0, 4, True) == (1, 13) and expected(3, 0, 4, True) == (15, 3)
    assert {(expected(n, d, 4, True)[1] != 0, n >> 3, d >> 3) for n, d in pairs} >= {(True, x, y) for x in (0, 1) for y in (0, 1)}
    check_division(ctx(kind, "classic_4_4"), 2, pairs, True, 620)


@pytest.mark.parametrize("kind", KINDS)
def test_abs_of_every_value(kind):
    """all 16 values at two blocks in one call; MIN, -1, 0, 1, MAX at four blocks; |MIN| = MIN"""
    c = ctx(kind, "classic_4_4")
    for L, values in ((2, list(range(16))), (4, [128, 255, 0, 1, 127])):
        B = 2 * L
        ct = c.enc([rm.digits(v, L, 4) for v in values], 630 + L)
        c.sks.abs_assign(ct, c.st)
        got = [rm.value(row, 4) for row in c.dec(ct)]
        assert got == [((1 << B) - v) & ((1 << B) - 1) if v >> (B - 1) else v for v in values]
        assert list(ct.degrees) == [3] * (L * len(values)) and list(ct._info[1]) == [1] * (L * len(values))


# ================================================================================== 4. census
CENSUS_SHAPES = [(2, 1), (2, 2), (2, 3), (3, 2)]


@pytest.mark.parametrize("b,L", CENSUS_SHAPES, ids=[f"{b}_bits-{L}_blocks" for b, L in CENSUS_SHAPES])
def test_the_chosen_pairs_reach_every_table_entry(b, L):
    """The clear model over ALL operand pairs of the shape lists every (table, input) the loop can ask: the shift table at
    every bit position, the divisor's masks and flags, the cleaning table, both zero-out tables at both factors, the
    quotient-bit table at every position in a block, the non-zero flags; signed also the sign, xor and sign-difference
    tables.  The pairs of tests 2, 3 and 5 reach all of it; a model-only condition on the choice of inputs."""
    for signed in (False, True):
        everything, _ = census(b, L, signed)
        tables = {e[0] for e in everything}
        assert tables >= {"shift", "low", "high", "clean", "keep", "zero", "bit"} | ({"sign", "xor", "differ"} if signed else set())
        assert {e[1] for e in everything if e[0] == "shift"} == set(range(b)), "a bit position of the numerator block"
        assert {e[1] for e in everything if e[0] in ("keep", "zero")} == {2, 3}, "both factors"
        assert {e[1] for e in everything if e[0] == "bit"} == set(range(b))
        if b == 2 and L == 1:
            pairs = unsigned_pairs(1, 16) if not signed else None
        elif b == 2:
            pairs = choose_pairs(2, L, True, 32, signed_must(2 * L)) if signed else unsigned_pairs(L, 32)
        else:
            pairs = other_base_pairs(b, L, signed)
        if pairs is not None:
            assert reached(b, L, signed, pairs) == everything, (b, L, signed)


def test_the_five_block_pairs_reach_every_entry_of_their_sample():
    everything, _ = census(2, 5, False, 4096)
    assert reached(2, 5, False, unsigned_pairs(5, 16)) == everything


# ================================================================================== 5. other bases and keys
def other_base_pairs(b, L, signed):
    """16 pairs at two bits per block.  At three bits 16 divisions cannot reach the census (the shift tables alone have 3 x 64
    inputs): the list is as long as reaching every entry takes, about 50 pairs; the emulation divides its first 16, which
    the greedy order makes the ones that reach most, the MI355X all of them."""
    B = b * L
    return choose_pairs(b, L, signed, 16, signed_must(B)[:4] if signed else [(0, 0), ((1 << B) - 1, 0)], at_most=b == 2)


OTHER = ["classic_8_8", "classic_4_16", "multibit_g4_4_4"]


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("base", OTHER)
@pytest.mark.parametrize("kind", KINDS)
def test_other_bases_and_keys(kind, base, signed):
    """(8, 8): three bits per block, so every position in a block; (4, 16): carry != msg; a multi-bit key with g = 4.  Two
    blocks, the census-complete pairs of other_base_pairs."""
    c = ctx(kind, base)
    pairs = other_base_pairs(c.base.bits, 2, signed)
    check_division(c, 2, pairs if kind == "hip" else pairs[:16], signed, 640)


# ================================================================================== 6. sharding
@pytest.mark.parametrize("kind", KINDS)
def test_rounds_sharded_over_the_streams_of_the_set(kind):
    """One stream against three streams on the same GPU at a threshold of 3 blocks per GPU: a signed batched division gives
    the same words."""
    from .test_radix_integer import setup
    p = EMU_SMALL["classic_4_4"]
    _, keys, st1, sks1, igpu = setup(kind, p)
    _, _, st3, sks3, _ = setup(kind, p, gpu_indexes=(0, 0, 0))
    lib = use_backend(kind)
    L, m = 2, 4
    pairs = [(13, 3), (7, 0), (8, 15), (5, 14)]
    wn = rm.encrypt_rows(p, keys, [rm.digits(n, L, m) for n, _ in pairs], 650)
    wd = rm.encrypt_rows(p, keys, [rm.digits(d, L, m) for _, d in pairs], 651)
    outs = {}
    for name, st, sks, thr in (("one", st1, sks1, 512), ("three", st3, sks3, 3)):
        lib.hip_integer_set_multi_gpu_threshold(thr)
        try:
            mk = lambda w: igpu.CudaUnsignedRadixCiphertext.from_blocks(w, st)
            num, den = mk(wn), mk(wd)
            for ct in (num, den):
                ct.set_degrees(m - 1)
            q, r = sks.div_rem(num, den, st, signed=True)
            outs[name] = [q.to_blocks(st), r.to_blocks(st)]
        finally:
            lib.hip_integer_set_multi_gpu_threshold(0)
    for one, three in zip(outs["one"], outs["three"]):
        assert np.array_equal(one, three)
    q, r = (rm.decrypt_many(p, keys, x).tolist() for x in outs["three"])
    assert [(rm.value(x, m), rm.value(y, m)) for x, y in zip(q, r)] == [expected(n, d, 4, True) for n, d in pairs]


# ================================================================================== 7. device = emulation
def both_divisions(c, wn, wd):
    out = []
    for signed in (False, True):
        num, den = c.from_words(wn), c.from_words(wd)
        q, r = c.sks.div_rem(num, den, c.st, signed=signed)
        out.append((signed, c.words(q), c.words(r)))
    return out


@pytest.mark.gpu
def test_device_equals_emulation_word_for_word():
    """The same keys and inputs through both backends: one unsigned and one signed batched call at (4, 4), two blocks."""
    toy = dataclasses.replace(BASE["classic_4_4"], hip=EMU_SMALL["classic_4_4"], emu=EMU_SMALL["classic_4_4"])
    p, keys = toy.emu, make_keys(toy.emu)
    pairs = [(13, 3), (7, 0), (8, 15), (5, 14)]
    wn = rm.encrypt_rows(p, keys, [rm.digits(n, 2, 4) for n, _ in pairs], 660)
    wd = rm.encrypt_rows(p, keys, [rm.digits(d, 2, 4) for _, d in pairs], 661)
    try:
        got = both_divisions(Ctx("hip", toy), wn, wd)
        gc.collect()
        want = both_divisions(Ctx("emu", toy), wn, wd)
    finally:
        use_backend("hip")
    for (signed, q_hip, r_hip), (_, q_emu, r_emu) in zip(got, want):
        assert np.array_equal(q_hip, q_emu) and np.array_equal(r_hip, r_emu), f"signed={signed}: the device's words differ"


# ================================================================================== 8. the anchor
@pytest.mark.gpu
@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
def test_sixteen_bits_on_the_anchor_row(signed):
    """PARAM_MESSAGE_2_CARRY_2, 8 blocks (16 bits): four pairs in one call, a zero divisor and MIN / -1 among them"""
    c = ctx("hip", "classic_4_4", production=True)
    assert c.p is C1
    pairs = [(0x8000, 0xFFFF), (0xBEEF, 0), (0xFFF1, 7), (12345, 0xFF85)] if signed else \
        [(0xFFFF, 1), (0xBEEF, 0), (54321, 123), (255, 0x8001)]
    check_division(c, 8, pairs, signed, 670)


# ================================================================================== 9. refusals
PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
N, n = 256, 4
BK = ffi.CudaLweBootstrapKeyParamsFFI(n, 1, N, 8, 2, N, 1, 0)
KK = ffi.CudaLweKeyswitchKeyParamsFFI(N, n, 4, 3)
keys = (C.c_void_p * 1)(gpu.CudaVec(16, st).ptr)
alive = []
def radix(blocks, degree=3, dim=N, vec=None):
    ct = igpu.CudaUnsignedRadixCiphertext(vec or gpu.CudaVec(blocks * (dim + 1), st), 1, blocks, dim)
    ct.set_degrees(degree)
    alive.extend([ct, ct._ffi()])
    return C.byref(alive[-1])
def scratch(blocks, signed=False, msg=4, carry=4):
    mem = C.c_void_p()
    lib.hip_scratch_integer_div_rem_64_async(s, signed, C.byref(mem), BK, KK, blocks, msg, carry, True, 0)
    return mem
def div(q, r, a, b, mem, signed=False):
    lib.hip_integer_div_rem_64_async(s, q, r, a, b, signed, mem, keys, keys)
"""

REFUSALS = {
    "a divisor with another block count": ("""
        div(radix(2), radix(2), radix(2), radix(3), scratch(2))
        """, "div_rem: quotient, remainder, numerator and divisor hold 2, 2, 2 and 3 blocks: they must be the same"),
    "a remainder with another lwe dimension": ("""
        div(radix(2), radix(2, dim=128), radix(2), radix(2), scratch(2))
        """, "div_rem: the blocks' lwe dimension should be 256"),
    "a dirty operand": ("""
        div(radix(2), radix(2), radix(2), radix(2, 5), scratch(2))
        """, "div_rem: block 0 has degree 5, numerator and divisor must be clean"),
    "a quotient that is the numerator": ("""
        v = gpu.CudaVec(2 * (N + 1), st)
        div(radix(2, vec=v), radix(2), radix(2, vec=v), radix(2), scratch(2))
        """, "div_rem: an output overlaps an input or the other output"),
    "a remainder that is the quotient": ("""
        v = gpu.CudaVec(2 * (N + 1), st)
        div(radix(2, vec=v), radix(2, vec=v), radix(2), radix(2), scratch(2))
        """, "div_rem: an output overlaps an input or the other output"),
    "more integers than the scratch holds": ("""
        div(radix(4), radix(4), radix(4), radix(4), scratch(2))
        """, "div_rem: 2 integers exceed the scratch capacity 1"),
    "moduli 2 2": ("""
        scratch(2, msg=2, carry=2)
        """, "div_rem: moduli (2, 2) do not hold the rows of the loop: values up to 5 and noise levels up to 5, at most 3 and 3 fit"),
    "moduli 2 8": ("""
        scratch(2, msg=2, carry=8)
        """, "div_rem: the message modulus 2 is not 4, 8 or 16"),
    "an unsigned scratch in a signed call": ("""
        div(radix(2), radix(2), radix(2), radix(2), scratch(2), signed=True)
        """, "div_rem: the scratch was created for unsigned operands, the call is signed"),
    "an abs scratch handed to div_rem": ("""
        mem = C.c_void_p()
        lib.hip_scratch_integer_abs_inplace_64_async(s, C.byref(mem), True, BK, KK, 2, 4, 4, True, 0)
        div(radix(2), radix(2), radix(2), radix(2), mem)
        """, "div_rem: foreign scratch pointer"),
    "a kernel table whose output overlaps a row it reads": ("""
        v = gpu.CudaVec(8 * 5, st)
        outs, consts = (C.c_void_p * 1)(v.ptr + 8 * 5), (C.c_uint64 * 1)(0)
        gu = (C.c_uint32 * 6)(2, 2, 0, 0, 2, 1)
        srcs, stands, scal = (C.c_void_p * 4)(v.ptr), (C.c_void_p * 4)(), (C.c_uint64 * 4)(1)
        tu = (C.c_uint32 * 24)(4, 4, 0, 1, 0, 0)
        lib.hip_test_divrem_sum_async(S, G, 5, 1, 1, outs, consts, gu, srcs, stands, scal, tu)
        """, "divrem_sum: the output of group 0 overlaps rows the launch reads"),
    "a kernel table that reads beyond its array": ("""
        v, o = gpu.CudaVec(8 * 5, st), gpu.CudaVec(8 * 5, st)
        outs, consts = (C.c_void_p * 1)(o.ptr), (C.c_uint64 * 1)(0)
        gu = (C.c_uint32 * 6)(2, 2, 0, 0, 2, 1)
        srcs, stands, scal = (C.c_void_p * 4)(v.ptr), (C.c_void_p * 4)(), (C.c_uint64 * 4)(1)
        tu = (C.c_uint32 * 24)(2, 2, 1, 1, 0, 0)
        lib.hip_test_divrem_sum_async(S, G, 5, 1, 1, outs, consts, gu, srcs, stands, scal, tu)
        """, "divrem_sum: term 0 of group 0 reads rows 1 .. 2 of an array of 2 rows per integer"),
    "a kernel table of five groups": ("""
        a = (C.c_void_p * 5)()
        lib.hip_test_divrem_sum_async(S, G, 5, 1, 5, a, a, a, a, a, a, a)
        """, "hip_test_divrem_sum: 5 groups (at most 4)"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_misuse_is_refused_with_a_message(name):
    """On the host emulation only, in a child process: the library aborts with a message that names the entry point."""
    snippet, message = REFUSALS[name]
    r = run_child(PRELUDE + textwrap.dedent(snippet))
    assert r.returncode == -signal.SIGABRT, f"{name}: returned {r.returncode}\n{r.stderr[-600:]}"
    assert message in r.stderr, r.stderr[-600:]


# ================================================================================== 10. prototypes
REF_INTEGER_H = "/root/reference/backends/tfhe-cuda-backend/cuda/include/integer/integer.h"
STANDS_FOR = {
    "hip_scratch_integer_div_rem_64_async": "scratch_cuda_integer_div_rem_64_async",
    "hip_integer_div_rem_64_async": "cuda_integer_div_rem_64_async",
    "hip_cleanup_integer_div_rem_64": "cleanup_cuda_integer_div_rem_64",
    "hip_scratch_integer_abs_inplace_64_async": "scratch_cuda_integer_abs_inplace_64_async",
    "hip_integer_abs_inplace_64_async": "cuda_integer_abs_inplace_64_async",
    "hip_cleanup_integer_abs_inplace_64": "cleanup_cuda_integer_abs_inplace_64",
}


@pytest.mark.skipif(not os.path.isfile(REF_INTEGER_H), reason="reference tree absent")
def test_prototypes_equal_the_reference_prototypes_they_stand_for():
    import sys
    sys.path.insert(0, ROOT)
    from tools.c_prototypes import parse_prototypes
    ours = parse_prototypes(open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read())
    ref = parse_prototypes(open(REF_INTEGER_H).read())
    for mine, theirs in STANDS_FOR.items():
        assert mine in ours and theirs in ref, (mine, theirs)
        assert ours[mine] == ref[theirs], f"{mine}: {ours[mine]} != {ref[theirs]}"
