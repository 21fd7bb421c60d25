"""Encrypted bit counts: leading / trailing zeros / ones, ilog2, checked_ilog2, count_ones, count_zeros, and the pack kernel
under them.

The checker is Python integer arithmetic on the decrypted blocks.  A clear model of the rounds (ClearCount below) tells
which inputs the count, scan and popcount tables were asked; the bootstrap and round counts are restated from the algorithm
(the scan's closed count, the planner's rule of csrc/radix_sum.h, the carry look-ahead).  Nothing reads the library's tables.
[emu] runs the kernel sources on the host, [hip] on the MI355X; toy keys, the anchor on the MI355X with
PARAM_MESSAGE_2_CARRY_2 and the GPU multi-bit g = 4 set.  The emulation takes every value of (4, 4) up to three blocks and
the first 16 values of the census-complete lists at five blocks and, at the other bases, at one and two blocks; the MI355X
takes all of it.
Every checked call is executed a second time on the first (at most 8) integers of its batch: the words must be the same.
The device against the emulation word for word is a test of its own (the emulation of every hip case would take minutes)."""
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
from .common import C1, C4G4, make_keys
from .harness import use_backend
from .test_div_rem import BASE, EMU_SMALL, ctx, propagate_pbs
from .test_error_behaviour import run as run_child
from .test_radix_bases import Base, Ctx

U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
RUNS, ILOG2, POP = 0, 1, 2                      # `kind` of hip_integer_bit_count_pbs_count

# ================================================================================== 1. the kernel alone
SENTINEL = U64(0xA5A5A5A55A5A5A5A)
MSG = 4
ALL_ONES = 2 ** 64 - 1
WORDS = (1, 5, 511, 512, 513, 2049)      # the edges of a 512-word slice, the odd production row
FORMS = [(1, 1), (1, -1), (1, 4), (1, -4), (2, 1)]          # (step, delta)
SCALARS = [(1, MSG), (MSG, 1), (ALL_ONES, 1)]
ROWS = (1, 2, 5)


def pair_pack_model(x, first, rows, step, delta, s0, s1):
    """x: [batch][x_stride][words] u64 -> [batch][ceil(rows / step)][words]; u64 arithmetic wraps modulo 2^64"""
    outs = -(-rows // step)
    out = np.zeros((x.shape[0], outs, x.shape[2]), dtype=U64)
    for g in range(outs):
        j = g * step
        out[:, g] = U64(s0) * x[:, first + j]
        if 0 <= j + delta < rows:
            out[:, g] += U64(s1) * x[:, first + j + delta]
    return out


def kernel_cases():
    """(rows, step, delta) the launcher accepts: |delta| < rows.  One row admits no distance at all: that shape is in the
    refusals.  Five rows at step 2 leave the last row alone."""
    return [(rows, step, delta) for rows in ROWS for step, delta in FORMS if abs(delta) < rows]


@pytest.mark.parametrize("batch", [1, 3], ids=["batch_1", "batch_3"])
@pytest.mark.parametrize("words", WORDS, ids=[f"{w}_words" for w in WORDS])
@pytest.mark.parametrize("kind", KINDS)
def test_pack_kernel_equals_numpy_word_for_word(kind, words, batch):
    """hip_test_pair_pack_async against its formula on random u64 words: every accepted (rows, step, delta) of kernel_cases,
    the three scalar pairs, integers x_stride = rows + 3 rows apart with the rows used starting at row 2, and dense
    (x_stride = rows, first = 0).  The output sits between sentinel rows that must stay as they are."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    lib = use_backend(kind)
    st = gpu.CudaStreams((0,))
    rng = np.random.default_rng(1000 * words + batch)
    assert {r for r, _, _ in kernel_cases()} == {2, 5} and (5, 2, 1) in kernel_cases()
    guard = 2 * words
    for rows, step, delta in kernel_cases():
        for x_stride, first in ((rows + 3, 2), (rows, 0)):
            x = rng.integers(0, 2 ** 64, size=(batch, x_stride, words), dtype=U64)
            d_x = gpu.CudaVec.from_cpu_async(x.reshape(-1), st)
            for s0, s1 in SCALARS:
                outs = -(-rows // step)
                frame = np.full(2 * guard + batch * outs * words, SENTINEL, dtype=U64)
                d_out = gpu.CudaVec.from_cpu_async(frame, st)
                lib.hip_test_pair_pack_async(st.ptr[0], 0, d_out.ptr + 8 * guard, d_x.ptr, s0, s1, words, batch, x_stride, first,
                                             rows, step, delta)
                got = d_out.copy_to_cpu(st)
                want = pair_pack_model(x, first, rows, step, delta, s0, s1)
                assert np.array_equal(got[guard:-guard], want.reshape(-1)), (rows, step, delta, x_stride, s0, s1)
                assert (got[:guard] == SENTINEL).all() and (got[-guard:] == SENTINEL).all(), "a sentinel row was written"


# ================================================================================== the counts restated
def counter_blocks(kind, L, b):
    """ceil((floor(log2 B) + 1) / b) for the runs and the popcounts, ceil((floor(log2(B - 1)) + 2) / b) for ilog2"""
    B = b * L
    need = ((B - 1).bit_length() - 1 if B > 1 else 0) + 2 if kind == ILOG2 else (B.bit_length() - 1) + 1
    return -(-need // b)


def plan_sums(cols, deg, msg, carry, final_cap):
    """The planner's rule (the comment above plan_column_sums): groups of at most (msg carry - 1) / (msg - 1) terms whose
    degrees add up to msg carry - 1 at most, first fit, largest degree first; a group becomes a message term and, when its
    degrees reach msg and a next column exists, a carry term; a column is finished at final_cap.  -> (bootstraps, rounds)"""
    cols, deg = [list(c) for c in cols], list(deg)
    L, cap = len(cols), msg * carry - 1
    most = cap // (msg - 1)
    total = lambda c: sum(deg[x] for x in c)
    finished = lambda c: total(c) <= final_cap and len(c) <= most
    pbs = rounds = 0
    while any(not finished(c) for c in cols):
        groups = [[] for _ in range(L)]
        for c in range(L):
            if finished(cols[c]):
                continue
            for x in sorted(cols[c], key=lambda x: -deg[x]):
                for g in groups[c]:
                    if len(g) < most and total(g) + deg[x] <= cap:
                        g.append(x)
                        break
                else:
                    groups[c].append([x])
        stuck = not any(len(g) >= 2 for gs in groups for g in gs)
        nxt = [[] for _ in range(L)]
        for c in range(L):
            if not groups[c]:
                nxt[c] += cols[c]
                continue
            for g in groups[c]:
                if not (len(g) >= 2 or (stuck and deg[g[0]] > 2 * msg - 2)):
                    nxt[c] += g
                    continue
                s = total(g)
                deg.append(min(msg - 1, s))
                nxt[c].append(len(deg) - 1)
                pbs += 1
                if c + 1 < L and s >= msg:
                    deg.append(s // msg)
                    nxt[c + 1].append(len(deg) - 1)
                    pbs += 1
        cols, rounds = nxt, rounds + 1
    return pbs, rounds


def propagate_rounds(L):
    if L == 1:
        return 1
    n = [L]
    while n[-1] > 4:
        n.append((n[-1] + 2) // 3)
    top = len(n) - 1
    return 3 + top + max(0, top - 1)


def first_stage(kind, L):
    """(bootstraps, rounds) before the sum: the scan bootstraps L rows, then the L - d rows that have a neighbour at
    d = 2, 4, ... < L; the popcount one row per pair of blocks"""
    if kind == POP:
        return (L + 1) // 2, 1
    ds = [d for d in (2 ** k for k in range(1, 32)) if d < L]
    return L + sum(L - d for d in ds), 1 + len(ds)


def bit_count_cost(kind, L, msg, carry):
    b = msg.bit_length() - 1
    nc = counter_blocks(kind, L, b)
    T = (L + 1) // 2 if kind == POP else L
    deg = [2 * b if kind == POP and 2 * i + 1 < L else b for i in range(T)]
    cols = [list(range(T))] + [[] for _ in range(nc - 1)]
    if kind == ILOG2:                      # the all-ones integer: a constant on term 0, a trivial term in the other columns
        deg[0] += msg - 1
        for j in range(1, nc):
            deg.append(msg - 1)
            cols[j].append(T + j - 1)
    s_pbs, s_rounds = plan_sums(cols, deg, msg, carry, 2 * msg - 2)
    f_pbs, f_rounds = first_stage(kind, L)
    return f_pbs + s_pbs + propagate_pbs(nc), f_rounds + s_rounds + propagate_rounds(nc)


def test_the_formulas_of_the_bootstrap_and_round_counts():
    """FheUint64 at PARAM_MESSAGE_2_CARRY_2, the figures docs/history/bit_count_log.md states: the scan alone is 130
    bootstraps in 5 rounds (the reference: 32 + 5 * 32 - 31 = 161 in 6); ilog2 runs in the rounds of leading_zeros."""
    assert first_stage(RUNS, 32) == (32 + 30 + 28 + 24 + 16, 5) == (130, 5)
    assert first_stage(POP, 32) == (16, 1) and first_stage(RUNS, 1) == (1, 1) and first_stage(RUNS, 3) == (3 + 1, 2)
    assert counter_blocks(RUNS, 32, 2) == counter_blocks(ILOG2, 32, 2) == counter_blocks(POP, 32, 2) == 4
    assert [counter_blocks(RUNS, L, 2) for L in (1, 2, 3, 5)] == [1, 2, 2, 2]
    assert [counter_blocks(ILOG2, L, 2) for L in (1, 2, 3, 5)] == [1, 2, 2, 3]
    runs, ilog2, pop = (bit_count_cost(k, 32, 4, 4) for k in (RUNS, ILOG2, POP))
    assert runs[1] == ilog2[1], "ilog2 takes the rounds of leading_zeros"
    assert runs == (130 + 23 + 11, 5 + 3 + 3) and ilog2 == (130 + 26 + 11, 11) and pop == (16 + 18 + 11, 1 + 3 + 3)


@pytest.mark.parametrize("kind", KINDS)
def test_the_published_counts_equal_the_formulas(kind):
    lib = use_backend(kind)
    for msg, carry in ((4, 4), (8, 8), (4, 16)):
        for L in (1, 2, 3, 5, 8, 32):
            for k in (RUNS, ILOG2, POP):
                got = int(lib.hip_integer_bit_count_pbs_count(k, L, msg, carry)), int(lib.hip_integer_bit_count_rounds(k, L, msg, carry))
                assert got == bit_count_cost(k, L, msg, carry), (msg, carry, L, k)


# ================================================================================== the clear model of the rounds
OPS = {  # name -> (kind, leading, counted bit)
    "leading_zeros": (RUNS, True, 0), "leading_ones": (RUNS, True, 1), "trailing_zeros": (RUNS, False, 0),
    "trailing_ones": (RUNS, False, 1), "ilog2": (ILOG2, True, 0), "count_ones": (POP, None, 1), "count_zeros": (POP, None, 0),
}


def expected(name, v, B):
    """Python integers on the B-bit pattern v"""
    bits = [(v >> i) & 1 for i in range(B)]

    def run(seq, bit):
        n = 0
        for x in seq:
            if x != bit:
                break
            n += 1
        return n
    if name == "ilog2":
        return v.bit_length() - 1              # -1 for zero: all ones modulo the counter's range
    kind, leading, bit = OPS[name]
    return sum(x == bit for x in bits) if kind == POP else run(bits[::-1] if leading else bits, bit)


class ClearCount:
    """The rounds of one count on clear blocks: which inputs the pair, lone, scan and popcount tables see"""

    def __init__(self, bits_per_block, blocks):
        self.b, self.L, self.msg = bits_per_block, blocks, 1 << bits_per_block

    def block_run(self, x, leading, bit):
        order = range(self.b - 1, -1, -1) if leading else range(self.b)
        n = 0
        for i in order:
            if (x >> i) & 1 != bit:
                break
            n += 1
        return n

    def scan(self, v, leading, bit, seen):
        b, L, msg = self.b, self.L, self.msg
        X = rm.digits(v, L, msg)
        nb = lambda i, d: i + d if leading else i - d
        t = []
        for i in range(L):
            j = nb(i, 1)
            if 0 <= j < L:
                seen.add(("pair", leading, bit, msg * X[j] + X[i]))
                t.append(self.block_run(X[i], leading, bit) if self.block_run(X[j], leading, bit) == b else 0)
            else:
                seen.add(("lone", leading, bit, X[i]))
                t.append(self.block_run(X[i], leading, bit))
        d = 2
        while d < L:
            new = list(t)
            for i in range(L):
                j = nb(i, d)
                if 0 <= j < L:
                    seen.add(("scan", msg * t[j] + t[i]))
                    new[i] = t[i] if t[j] == b else 0
            t, d = new, 2 * d
        return t

    def run(self, name, v, seen):
        kind, leading, bit = OPS[name]
        b, L, msg = self.b, self.L, self.msg
        if kind == POP:
            X, total = rm.digits(v, L, msg), 0
            for g in range((L + 1) // 2):
                if 2 * g + 1 < L:
                    x = msg * X[2 * g + 1] + X[2 * g]
                    seen.add(("pop_pair", bit, x))
                    total += sum(((x >> i) & 1) == bit for i in range(2 * b))
                else:
                    seen.add(("pop_lone", bit, X[2 * g]))
                    total += sum(((X[2 * g] >> i) & 1) == bit for i in range(b))
            return total
        t = self.scan(v, leading, bit, seen)
        if kind == ILOG2:
            return (sum(b - x for x in t) - 1) % msg ** counter_blocks(ILOG2, L, b)
        return sum(t)


def structured(B):
    """0 and all ones, every single set bit and every single clear bit, every 2^k - 1 and its complement"""
    full = (1 << B) - 1
    out = [0, full]
    for k in range(B):
        out += [1 << k, full ^ (1 << k)]
    for k in range(B + 1):
        out += [(1 << k) - 1, full ^ ((1 << k) - 1)]
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def census(b, L):
    """every (table, input) the rounds ask over ALL values of the shape (over the structured values and 4,096 seeded ones
    where the shape has more than 2^12), and per value what it reaches; the model is checked against plain arithmetic"""
    B, model = b * L, ClearCount(b, L)
    values = list(range(1 << B)) if B <= 12 else \
        list(dict.fromkeys(structured(B) + [int(x) for x in np.random.default_rng(B).integers(0, 1 << B, 4096)]))
    reach, everything = {}, set()
    for v in values:
        seen = set()
        for name in OPS:
            nc = counter_blocks(OPS[name][0], L, b)
            assert model.run(name, v, seen) == expected(name, v, B) % (1 << b) ** nc, (name, v)
        reach[v] = frozenset(seen)
        everything |= seen
    return everything, reach


@functools.lru_cache(maxsize=None)
def chosen_values(b, L):
    """the structured values, then greedily the value that adds most of the census (first in order on a tie), then four
    seeded draws"""
    B = b * L
    everything, reach = census(b, L)
    chosen = structured(B)
    covered = set().union(*(reach[v] for v in chosen))
    order = list(reach)
    while covered != everything:
        best = max(order, key=lambda v: len(reach[v] - covered))
        chosen.append(best)
        covered |= reach[best]
    rng = np.random.default_rng(11 * b + L)
    for v in rng.integers(0, 1 << B, 4):
        if int(v) not in chosen:
            chosen.append(int(v))
    return chosen


def reached(b, L, values):
    model, seen = ClearCount(b, L), set()
    for v in values:
        for name in OPS:
            model.run(name, v, seen)
    return seen


SHAPES = [(b, L) for b in (2, 3) for L in (1, 2, 3, 5)]


@pytest.mark.parametrize("b,L", SHAPES, ids=[f"{b}_bits-{L}_blocks" for b, L in SHAPES])
def test_the_chosen_values_reach_every_run_length_and_every_table_entry(b, L):
    """By the clear model alone: the values of chosen_values give every run length 0 .. B from both ends for zeros and ones,
    every popcount 0 .. B, and every (table, input) that all values of the shape reach — at two blocks and more every pair of
    digits in the pair tables of the four runs and of both popcounts."""
    B, msg = b * L, 1 << b
    values = chosen_values(b, L)
    for name in ("leading_zeros", "leading_ones", "trailing_zeros", "trailing_ones", "count_ones", "count_zeros"):
        assert {expected(name, v, B) for v in values} == set(range(B + 1)), name
    assert {expected("ilog2", v, B) for v in values} == set(range(-1, B))
    everything, _ = census(b, L)
    assert reached(b, L, values) == everything
    if L >= 2:
        for leading in (True, False):
            for bit in (0, 1):
                assert {e[3] for e in everything if e[:3] == ("pair", leading, bit)} == set(range(msg * msg))
                assert {e[3] for e in everything if e[:3] == ("lone", leading, bit)} == set(range(msg))
        for bit in (0, 1):
            assert {e[2] for e in everything if e[:2] == ("pop_pair", bit)} == set(range(msg * msg))
    if L >= 3:
        full, part = {msg * b + t for t in range(b + 1)}, {msg * u + t for u in range(b) for t in range(b + 1)}
        assert {e[1] for e in everything if e[0] == "scan"} >= full and {e[1] for e in everything if e[0] == "scan"} & part


# ================================================================================== the checked call
def check_counts(c, L, values, seed, checked=()):
    """one batched call per operation over `values`: the value, counter_num_blocks, degrees, noise levels, the operand
    untouched, the published count against the formula (the library aborts when it issued another number), a second
    execution on the first integers word for word; checked_ilog2 one integer at a time on the values of `checked`"""
    m, b = c.msg, c.base.bits
    B, n = b * L, len(values)
    ct = c.enc([rm.digits(v, L, m) for v in values], seed)
    before = c.words(ct)
    lib = use_backend(c.kind)
    for name, (kind, _, _) in OPS.items():
        nc = counter_blocks(kind, L, b)
        out, pbs = getattr(c.sks, name)(ct, c.st, return_pbs_count=True)
        assert out.num_blocks == nc == c.sks.counter_num_blocks(L, ilog2=kind == ILOG2) and out.num_integers == n
        assert pbs == n * int(lib.hip_integer_bit_count_pbs_count(kind, L, m, c.carry)) == n * bit_count_cost(kind, L, m, c.carry)[0]
        rows = c.dec(out)
        assert all(0 <= x < m for row in rows for x in row)
        got, want = [rm.value(r, m) for r in rows], [expected(name, v, B) % m ** nc for v in values]
        wrong = [(v, g, w) for v, g, w in zip(values, got, want) if g != w]
        assert not wrong, f"{name}: value, got, expected: {wrong[:8]}"
        assert list(out.degrees) == [m - 1] * (nc * n) and list(out._info[1]) == [1] * (nc * n)
        k = min(n, 8)
        again = getattr(c.sks, name)(c.from_words(before[:k]), c.st)
        assert np.array_equal(c.words(again), c.words(out)[:k]), f"{name}: a second execution gives other words"
    assert np.array_equal(c.words(ct), before), "the operand was touched"
    nc = counter_blocks(ILOG2, L, b)
    for v in checked:
        one = c.enc([rm.digits(v, L, m)], seed + 1)
        value, flag = c.sks.checked_ilog2(one, c.st)
        assert rm.value(c.dec(value)[0], m) == expected("ilog2", v, B) % m ** nc and c.dec(flag)[0][0] == int(v > 0), v
        if v == 0:
            assert c.dec(value)[0] == [m - 1] * nc, "ilog2(0) is all ones"


# ================================================================================== 2. every value at (4, 4)
@pytest.mark.parametrize("L", [1, 2, 3], ids=lambda L: f"{L}_blocks")
@pytest.mark.parametrize("kind", KINDS)
def test_every_value_at_4_4(kind, L):
    """(4, 4): all 2^B values at one, two and three blocks, all eight operations (checked_ilog2 on every value too).  One
    block has no scan step and one counter block; three blocks have a step whose middle row has no partner."""
    values = list(range(1 << (2 * L)))
    check_counts(ctx(kind, "classic_4_4"), L, values, 700 + L, checked=values)


def lists_for(kind):
    """(base, L): the MI355X takes every shape with its census-complete list; the emulation the first 16 values (the
    structured ones first) at five blocks of (4, 4) and at one and two blocks of the other bases"""
    out = []
    for base in ("classic_4_4", "classic_8_8", "classic_4_16", "multibit_g4_4_4"):
        for L in (1, 2, 3, 5):
            if base == "classic_4_4" and L < 5:
                continue                              # every value: test_every_value_at_4_4
            if kind == "emu" and base != "classic_4_4" and L > 2:
                continue
            out.append((base, L))
    return out


CHOSEN = [pytest.param(k, base, L, id=f"{k}-{base}-{L}_blocks", marks=[pytest.mark.gpu] if k == "hip" else [])
          for k in ("emu", "hip") for base, L in lists_for(k)]


@pytest.mark.parametrize("kind,base,L", CHOSEN)
def test_chosen_values_at_every_base(kind, base, L):
    """(8, 8): three bits per block; (4, 16): carry != msg; a multi-bit key with g = 4; five blocks: three scan steps and, for
    ilog2 at two bits per block, a third counter block.  The values of chosen_values (0 and all ones, every single set and
    clear bit, every 2^k - 1 and its complement, what the census still lacks, seeded draws)."""
    c = ctx(kind, base)
    values = chosen_values(c.base.bits, L)
    B = c.base.bits * L
    if kind == "emu":
        values = values[:16]
    check_counts(c, L, values, 720 + L, checked=[0, 1, (1 << B) - 1, values[-1]])


# ================================================================================== 3. batches, dirty operands
def raw_calls(c, name, ct, capacity, times):
    """scratch for `capacity` integers, `times` launches on it, cleanup -> the words of every launch"""
    kind, leading, bit = OPS[name]
    sks, lib = c.sks, use_backend(c.kind)
    s, keep = sks._streams(c.st)
    ksks, bsks = sks._key_ptrs(c.st)
    L, m = ct.num_blocks, c.msg
    nc = counter_blocks(kind, L, c.base.bits)
    mem = C.c_void_p()
    lib.hip_integer_scratch_batch(capacity)
    common = (s, C.byref(mem), sks._bsk_params(), sks._ksk_params())
    if kind == RUNS:
        lib.hip_scratch_integer_count_of_consecutive_bits_64_async(*common, L, nc, m, c.carry, int(leading), bit, True,
                                                                   sks._noise_reduction())
    elif kind == ILOG2:
        lib.hip_scratch_integer_ilog2_64_async(*common, m, c.carry, L, nc, L * c.base.bits, True, sks._noise_reduction())
    else:
        lib.hip_scratch_integer_count_ones_64_async(*common, L, nc, m, c.carry, bit, True, sks._noise_reduction())
    lib.hip_integer_scratch_batch(1)
    words = []
    w = ct.lwe_dimension + 1
    for _ in range(times):
        out = c.igpu.CudaUnsignedRadixCiphertext.from_blocks(np.zeros((ct.num_integers, nc, w), dtype=U64), c.st)
        if kind == ILOG2:
            triv = [c.igpu.CudaUnsignedRadixCiphertext.from_blocks(np.zeros((1, k, w), dtype=U64), c.st) for k in (nc, nc, 1)]
            lib.hip_integer_ilog2_64_async(s, C.byref(out._ffi()), C.byref(ct._ffi()), *(C.byref(t._ffi()) for t in triv), mem,
                                           bsks, ksks)
        else:
            entry = lib.hip_integer_count_of_consecutive_bits_64_async if kind == RUNS else lib.hip_integer_count_ones_64_async
            entry(s, C.byref(out._ffi()), C.byref(ct._ffi()), mem, bsks, ksks)
        words.append(c.words(out))
    name_c = ("count_of_consecutive_bits", "ilog2", "count_ones")[kind]
    getattr(lib, f"hip_cleanup_integer_{name_c}_64")(s, C.byref(mem))
    assert not mem.value
    return words


@pytest.mark.parametrize("kind", KINDS)
def test_three_integers_on_a_scratch_created_for_four(kind):
    """(4, 4), three blocks: a scratch sized for four integers serves three, twice; both launches give the words of the call
    whose scratch was sized for three, and the right values"""
    c = ctx(kind, "classic_4_4")
    L, values = 3, [0b101100, 0, 0b000111]
    ct = c.enc([rm.digits(v, L, 4) for v in values], 740)
    for name, (k, _, _) in OPS.items():
        first, second = raw_calls(c, name, ct, 4, 2)
        exact = c.words(getattr(c.sks, name)(ct, c.st))
        assert np.array_equal(first, second) and np.array_equal(first, exact), name
        nc = counter_blocks(k, L, 2)
        assert [rm.value(r, 4) for r in rm.decrypt_many(c.p, c.keys, first).tolist()] == [expected(name, v, 6) % 4 ** nc for v in values]


@pytest.mark.parametrize("kind", KINDS)
def test_an_operand_that_is_not_clean_is_propagated_by_the_default_forms(kind):
    """x + y without propagation has blocks of degree 6: the default forms count the bits of (x + y) mod 2^B and leave the
    operand as it is (the unchecked entry refuses it: test_misuse_is_refused_with_a_message)"""
    c = ctx(kind, "classic_4_4")
    L, x, y = 3, 0b011011, 0b001110
    ct, other = c.enc([rm.digits(x, L, 4)], 750), c.enc([rm.digits(y, L, 4)], 751)
    c.sks.unchecked_add_assign(ct, other, c.st)
    if int(ct.degrees.max()) <= 3:
        ct.set_degrees(6)                   # (a backend that does not track the addition's degrees)
    before = c.words(ct)
    total = (x + y) % 64
    for name, (k, _, _) in OPS.items():
        out = getattr(c.sks, name)(ct, c.st)
        assert rm.value(c.dec(out)[0], 4) == expected(name, total, 6) % 4 ** counter_blocks(k, L, 2), name
    value, flag = c.sks.checked_ilog2(ct, c.st)
    assert rm.value(c.dec(value)[0], 4) == total.bit_length() - 1 and c.dec(flag)[0][0] == 1
    assert np.array_equal(c.words(ct), before)


# ================================================================================== 4. device = emulation
def all_counts(c, words):
    return [(name, c.words(getattr(c.sks, name)(c.from_words(words), c.st))) for name in OPS]


@pytest.mark.gpu
@pytest.mark.parametrize("L", [3, 5], ids=lambda L: f"{L}_blocks")
def test_device_equals_emulation_word_for_word(L):
    """The same keys and inputs through both backends: the seven counts at (4, 4), three and five blocks"""
    toy = dataclasses.replace(BASE["classic_4_4"], hip=EMU_SMALL["classic_4_4"], emu=EMU_SMALL["classic_4_4"])
    p, keys = toy.emu, make_keys(toy.emu)
    B = 2 * L
    values = [0, (1 << B) - 1, 1, 1 << (B - 1), 0b011010 % (1 << B), (1 << B) - 4]
    words = rm.encrypt_rows(p, keys, [rm.digits(v, L, 4) for v in values], 760)
    try:
        got = all_counts(Ctx("hip", toy), words)
        gc.collect()
        want = all_counts(Ctx("emu", toy), words)
    finally:
        use_backend("hip")
    for (name, hip), (_, emu) in zip(got, want):
        assert np.array_equal(hip, emu), f"{name}: the device's words differ"


# ================================================================================== 5. the anchor
ANCHORS = {"classic": Base("anchor_classic_4_4", C1, C1, 4, 4, True), "multibit_g4": Base("anchor_multibit_g4_4_4", C4G4, C4G4, 4, 4, True)}
_anchor = {}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(ANCHORS))
def test_sixty_four_bits_on_the_anchor_rows(which):
    """PARAM_MESSAGE_2_CARRY_2 and the GPU multi-bit g = 4 set, 32 blocks: 0, 1, 2^63, 2^64 - 1 and four seeded values in one
    call per operation, all eight operations"""
    if which not in _anchor:
        _anchor[which] = Ctx("hip", ANCHORS[which])
    c = _anchor[which]
    use_backend("hip")
    rng = np.random.default_rng(64)
    values = [0, 1, 1 << 63, (1 << 64) - 1] + [int(x) >> int(s) for x, s in zip(rng.integers(0, 2 ** 64, 4, dtype=U64), (0, 5, 23, 47))]
    check_counts(c, 32, values, 770, checked=[0, values[-1]])


# ================================================================================== 6. refusals
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
def runs(blocks, counter, msg=4, carry=4):
    mem = C.c_void_p()
    lib.hip_scratch_integer_count_of_consecutive_bits_64_async(s, C.byref(mem), BK, KK, blocks, counter, msg, carry, 1, 0, True, 0)
    return mem
def ilog2(blocks, counter, msg=4, carry=4, bits=None):
    mem = C.c_void_p()
    lib.hip_scratch_integer_ilog2_64_async(s, C.byref(mem), BK, KK, msg, carry, blocks, counter, 2 * blocks if bits is None else bits, True, 0)
    return mem
def ones(blocks, counter, msg=4, carry=4):
    mem = C.c_void_p()
    lib.hip_scratch_integer_count_ones_64_async(s, C.byref(mem), BK, KK, blocks, counter, msg, carry, 1, True, 0)
    return mem
def pack(out, x, words=5, batch=1, x_stride=5, first=0, rows=5, step=1, delta=1):
    lib.hip_test_pair_pack_async(S, G, out, x, 1, 4, words, batch, x_stride, first, rows, step, delta)
"""

REFUSALS = {
    "runs at moduli 2 2": ("runs(2, 2, msg=2, carry=2)", "count_of_consecutive_bits: moduli (2, 2): the carry propagation and the column sums take"),
    "runs at moduli 2 4": ("runs(2, 2, msg=2, carry=4)", "count_of_consecutive_bits: moduli (2, 4): the carry propagation and the column sums take"),
    "runs at moduli 2 8": ("runs(2, 2, msg=2, carry=8)", "count_of_consecutive_bits: moduli (2, 8): the carry propagation and the column sums take"),
    "ilog2 at moduli 2 2": ("ilog2(2, 2, msg=2, carry=2, bits=2)", "ilog2: moduli (2, 2): the carry propagation and the column sums take"),
    "count_ones at moduli 2 8": ("ones(2, 2, msg=2, carry=8)", "count_ones: moduli (2, 8): the carry propagation and the column sums take"),
    "a message modulus that is not a power of two": ("runs(2, 2, msg=6, carry=6)", "count_of_consecutive_bits: the message modulus 6 is not a power of two"),
    "runs with a wrong counter_num_blocks": ("runs(5, 3)", "count_of_consecutive_bits: counter_num_blocks is 3, 5 blocks of 2 bits take 2"),
    "ilog2 with the counter_num_blocks of the runs": ("ilog2(5, 2)", "ilog2: counter_num_blocks is 2, 5 blocks of 2 bits take 3"),
    "count_ones with a wrong counter_num_blocks": ("ones(1, 2)", "count_ones: counter_num_blocks is 2, 1 blocks of 2 bits take 1"),
    "ilog2 with a wrong bit count": ("ilog2(5, 3, bits=11)", "ilog2: num_bits_in_ciphertext is 11, 5 blocks of modulus 4 hold 10"),
    "an output that is the input": ("""
        v = gpu.CudaVec(2 * (N + 1), st)
        lib.hip_integer_count_of_consecutive_bits_64_async(s, radix(2, vec=v), radix(2, vec=v), runs(2, 2), keys, keys)
        """, "count_of_consecutive_bits: the output and the input must be different ciphertexts"),
    "an ilog2 output that is the input": ("""
        v = gpu.CudaVec(2 * (N + 1), st)
        lib.hip_integer_ilog2_64_async(s, radix(2, vec=v), radix(2, vec=v), radix(2), radix(2), radix(1), ilog2(2, 2), keys, keys)
        """, "ilog2: the output and the input must be different ciphertexts"),
    "a dirty operand": ("""
        lib.hip_integer_count_of_consecutive_bits_64_async(s, radix(2), radix(2, 5), runs(2, 2), keys, keys)
        """, "count_of_consecutive_bits: block 0 has degree 5, the operand must be clean"),
    "a dirty operand of count_ones": ("""
        lib.hip_integer_count_ones_64_async(s, radix(2), radix(2, 6), ones(2, 2), keys, keys)
        """, "count_ones: block 0 has degree 6, the operand must be clean"),
    "an output with another block count": ("""
        lib.hip_integer_count_ones_64_async(s, radix(3), radix(2), ones(2, 2), keys, keys)
        """, "count_ones: the output holds 3 blocks, 1 integers take 2 counter blocks each"),
    "more integers than the scratch holds": ("""
        lib.hip_integer_count_ones_64_async(s, radix(4), radix(4), ones(2, 2), keys, keys)
        """, "count_ones: 2 integers exceed the scratch capacity 1"),
    "a trivial operand of ilog2 with another block count": ("""
        lib.hip_integer_ilog2_64_async(s, radix(2), radix(2), radix(3), radix(2), radix(1), ilog2(2, 2), keys, keys)
        """, "ilog2: num blocks of trivial_ct_neg_n should be equal to counter_num_blocks"),
    "an ilog2 scratch handed to count_ones": ("""
        lib.hip_integer_count_ones_64_async(s, radix(2), radix(2), ilog2(2, 2), keys, keys)
        """, "count_ones: foreign scratch pointer"),
    "a pack without an operand": ("""
        pack(gpu.CudaVec(5 * 5, st).ptr, None)
        """, "pair_pack: null pointer or empty operand"),
    "a pack of no words": ("""
        pack(gpu.CudaVec(5 * 5, st).ptr, gpu.CudaVec(5 * 5, st).ptr, words=0)
        """, "pair_pack: null pointer or empty operand"),
    "a pack at distance zero": ("""
        pack(gpu.CudaVec(5 * 5, st).ptr, gpu.CudaVec(5 * 5, st).ptr, delta=0)
        """, "pair_pack: distance 0 on 5 rows"),
    "a pack at the distance of its rows": ("""
        pack(gpu.CudaVec(5 * 5, st).ptr, gpu.CudaVec(5 * 5, st).ptr, delta=-5)
        """, "pair_pack: distance -5 on 5 rows"),
    "a pack of one row": ("""
        pack(gpu.CudaVec(5 * 5, st).ptr, gpu.CudaVec(5 * 5, st).ptr, rows=1, delta=1)
        """, "pair_pack: distance 1 on 1 rows"),
    "a pack with step three": ("""
        pack(gpu.CudaVec(5 * 5, st).ptr, gpu.CudaVec(5 * 5, st).ptr, step=3)
        """, "pair_pack: step 3 is neither 1 nor 2"),
    "a pack whose output overlaps the rows it reads": ("""
        v = gpu.CudaVec(5 * 10, st)
        pack(v.ptr + 8 * 5 * 4, v.ptr)
        """, "pair_pack: the output overlaps the rows it reads"),
    "a pack of 65,536 integers": ("""
        pack(gpu.CudaVec(5 * 5, st).ptr, gpu.CudaVec(5 * 5, st).ptr, batch=65536)
        """, "pair_pack: 65536 integers in one launch"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_").replace(",", "") for n in REFUSALS])
def test_misuse_is_refused_with_a_message(name):
    """On the host emulation only, in a child process: the library aborts with a message that names the entry point."""
    snippet, message = REFUSALS[name]
    r = run_child(PRELUDE + textwrap.dedent(snippet))
    assert r.returncode == -signal.SIGABRT, f"{name}: returned {r.returncode}\n{r.stderr[-600:]}"
    assert message in r.stderr, r.stderr[-600:]


def test_a_size_query_allocates_nothing_and_reports_the_bytes():
    """allocate_gpu_memory = false on the three scratch entry points (host emulation, a child process): a size is returned,
    a launch on such a scratch is refused, cleanup frees it"""
    r = run_child(PRELUDE + textwrap.dedent("""
        for name, make in (("count_of_consecutive_bits", lambda m, a: lib.hip_scratch_integer_count_of_consecutive_bits_64_async(
                                s, C.byref(m), BK, KK, 5, 2, 4, 4, 1, 0, a, 0)),
                           ("ilog2", lambda m, a: lib.hip_scratch_integer_ilog2_64_async(s, C.byref(m), BK, KK, 4, 4, 5, 3, 10, a, 0)),
                           ("count_ones", lambda m, a: lib.hip_scratch_integer_count_ones_64_async(
                                s, C.byref(m), BK, KK, 5, 2, 4, 4, 1, a, 0))):
            def live():
                stats = (C.c_uint64 * 7)()
                lib.hip_backend_allocator_stats(0, stats)
                return stats[5]
            start = live()
            dry, real = C.c_void_p(), C.c_void_p()
            size = make(dry, False)
            assert live() == start, "a size query allocated"
            sized = make(real, True)
            assert size >= sized > 0 and live() > start, (size, sized)
            getattr(lib, f"hip_cleanup_integer_{name}_64")(s, C.byref(real))
            getattr(lib, f"hip_cleanup_integer_{name}_64")(s, C.byref(dry))
            assert live() == start and not real.value and not dry.value, "cleanup left device memory behind"
            print(name, size, sized, flush=True)
        mem = C.c_void_p()
        lib.hip_scratch_integer_count_ones_64_async(s, C.byref(mem), BK, KK, 2, 2, 4, 4, 1, False, 0)
        lib.hip_integer_count_ones_64_async(s, radix(2), radix(2), mem, keys, keys)
        """))
    assert r.returncode == -signal.SIGABRT and "count_ones: scratch was created with allocate_gpu_memory=false" in r.stderr, \
        r.stdout[-400:] + r.stderr[-800:]
    assert [line.split()[0] for line in r.stdout.splitlines()] == ["count_of_consecutive_bits", "ilog2", "count_ones"]


# ================================================================================== 7. prototypes
REF_INTEGER_H = "/root/reference/backends/tfhe-cuda-backend/cuda/include/integer/integer.h"
STANDS_FOR = {
    "hip_scratch_integer_count_of_consecutive_bits_64_async": "scratch_cuda_integer_count_of_consecutive_bits_64_async",
    "hip_integer_count_of_consecutive_bits_64_async": "cuda_integer_count_of_consecutive_bits_64_async",
    "hip_cleanup_integer_count_of_consecutive_bits_64": "cleanup_cuda_integer_count_of_consecutive_bits_64",
    "hip_scratch_integer_ilog2_64_async": "scratch_cuda_integer_ilog2_64_async",
    "hip_integer_ilog2_64_async": "cuda_integer_ilog2_64_async",
    "hip_cleanup_integer_ilog2_64": "cleanup_cuda_integer_ilog2_64",
}
ENUMS = ("enum Direction { Trailing = 0, Leading = 1 };", "enum BitValue { Zero = 0, One = 1 };")


def test_the_header_declares_the_two_enums_and_the_rust_crate_their_types():
    header = open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read()
    types = open(os.path.join(ROOT, "backends", "tfhe-hip-backend", "src", "ffi_types.rs")).read()
    for e in ENUMS:
        assert e in header
    for t in ("pub type Direction = ffi::c_uint;", "pub const Direction_Leading: Direction = 1;", "pub type BitValue = ffi::c_uint;",
              "pub const BitValue_One: BitValue = 1;"):
        assert t in types


@pytest.mark.skipif(not os.path.isfile(REF_INTEGER_H), reason="reference tree absent")
def test_prototypes_equal_the_reference_prototypes_they_stand_for():
    import sys
    sys.path.insert(0, ROOT)
    from tools.c_prototypes import parse_prototypes
    ref_text = open(REF_INTEGER_H).read()
    ours = parse_prototypes(open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read())
    ref = parse_prototypes(ref_text)
    for mine, theirs in STANDS_FOR.items():
        assert mine in ours and theirs in ref, (mine, theirs)
        assert ours[mine] == ref[theirs], f"{mine}: {ours[mine]} != {ref[theirs]}"
    for e in ENUMS:
        assert e in ref_text
