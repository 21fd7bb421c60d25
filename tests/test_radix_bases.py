"""Radix-integer layer at every base it is wired for: each operation of tests/test_radix_integer.py and
tests/test_radix_more_ops.py again at message/carry moduli (4, 4), (8, 8), (4, 16), on classic and multi-bit keys, and the
propagation-free operations also at one bit per block, (2, 8), (2, 4) and (2, 2); with operands BUILT so that every
reachable input of every lookup table occurs (the coverage is computed from the clear digits and asserted), every carry
state sequence of a two-level look-ahead, the device against the host emulation word for word, the refusals in a child
process, and the degrees every operation writes back.

The checker is clear big-integer arithmetic in plain Python on the decrypted blocks.  tests/radix_model.py holds the
operand builders and the coverage accounting; nothing of either reads the library's tables.
[emu] runs the kernel sources on the host, [hip] on the MI355X; both on toy keys, the anchor row on the MI355X with
PARAM_MESSAGE_2_CARRY_2."""
import dataclasses
import gc
import textwrap

import numpy as np
import pytest

from . import radix_model as rm
from .common import (C1, TOY_1024_K2, TOY_2048, TOY_2048_P64, TOY_K1, TOY_MB4_2048, TOY_MB_2048, Params, encrypt_big,
                     make_keys)
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_integer import setup


@dataclasses.dataclass(frozen=True)
class Base:
    name: str
    emu: Params
    hip: Params
    msg: int
    carry: int
    propagates: bool      # the carry look-ahead accepts the base (message_modulus >= 3, 16 values per block or more)

    @property
    def bits(self):
        return self.msg.bit_length() - 1


BASES = [
    Base("classic_4_4", TOY_2048, C1, 4, 4, True),                       # today's base, the anchor
    Base("classic_8_8", TOY_2048_P64, TOY_2048_P64, 8, 8, True),         # 3 bits per block
    Base("classic_4_16", TOY_2048_P64, TOY_2048_P64, 4, 16, True),       # carry != msg
    Base("multibit_g3_4_4", TOY_MB_2048, TOY_MB_2048, 4, 4, True),
    Base("multibit_g4_4_4", TOY_MB4_2048, TOY_MB4_2048, 4, 4, True),
    Base("classic_2_8", TOY_2048, TOY_2048, 2, 8, False),                # one bit per block
    Base("classic_k2_2_4", TOY_1024_K2, TOY_1024_K2, 2, 4, False),       # k = 2, N = 1024
    Base("classic_k1_2_2", TOY_K1, TOY_K1, 2, 2, False),                 # plaintext modulus 4, N = 256
]


def cases(bases):
    return [pytest.param(kind, b, id=f"{kind}-{b.name}", marks=[pytest.mark.gpu] if kind == "hip" else [])
            for kind in ("emu", "hip") for b in bases]


def scoped_cases(bases, scopes, narrow):
    """(kind, base, scope) for every scope.  On the MI355X every scope runs.  On the emulation the scopes in `narrow` stand
    unmarked; the others cost it a minute and more and carry the `slow` marker ("-everything" in their id)."""
    out = []
    for p in cases(bases):
        kind, base = p.values
        for sc in scopes:
            name = "_".join(str(x) for x in sc) if isinstance(sc, tuple) else str(sc)
            if kind == "emu" and sc not in narrow:
                out.append(pytest.param(kind, base, sc, id=f"{p.id}-{name}-everything", marks=[pytest.mark.slow]))
            else:
                out.append(pytest.param(kind, base, sc, id=f"{p.id}-{name}", marks=p.marks))
    return out


ALL = cases(BASES)
PROPAGATING = cases([b for b in BASES if b.propagates])


class Ctx:
    """keys on the backend `kind` at a base; encrypts digit rows, decrypts to digit rows"""

    def __init__(self, kind, base):
        self.kind, self.base, self.msg, self.carry = kind, base, base.msg, base.carry
        p = base.emu if kind == "emu" else base.hip
        assert p.plaintext_modulus == base.msg * base.carry
        self.p, self.keys, self.st, self.sks, self.igpu = setup(kind, p, msg=base.msg, carry=base.carry)

    def enc(self, rows, seed, degree=None):
        ct = self.igpu.CudaUnsignedRadixCiphertext.from_blocks(rm.encrypt_rows(self.p, self.keys, rows, seed), self.st)
        ct.set_degrees(self.msg - 1 if degree is None else degree)
        return ct

    def from_words(self, words, degree=None):
        ct = self.igpu.CudaUnsignedRadixCiphertext.from_blocks(words, self.st)
        ct.set_degrees(self.msg - 1 if degree is None else degree)
        return ct

    def dec(self, ct):
        return rm.decrypt_many(self.p, self.keys, ct.to_blocks(self.st)).tolist()

    def words(self, ct):
        return ct.to_blocks(self.st)


def values(rows, msg):
    return [rm.value(r, msg) for r in rows]


# ================================================================================== 1 + 2. tables, entry by entry
@pytest.mark.parametrize("kind,base", ALL)
def test_bitwise_tables_see_every_pair_of_digits(kind, base):
    """and / or / xor of two ciphertexts (one bivariate table, packed msg * lhs + rhs), of a ciphertext and clear blocks
    (one table per clear value) and the levelled NOT, on msg^2 blocks that hold every pair once."""
    c, m = Ctx(kind, base), base.msg
    a, b = rm.all_pairs(m)
    assert set(zip(a, b)) == {(x, y) for x in range(m) for y in range(m)}
    for op in ("and", "or", "xor"):
        # degrees: the left operand's are the tightest true ones (its digits), the right one's msg - 1
        ca, cb = c.enc([a], 301), c.enc([b], 302)
        ca.degrees[:] = a
        before = c.words(cb)
        c.sks.bitop_assign(ca, cb, op, c.st)
        assert c.dec(ca) == [[rm.clear_bitop(op, x, y) for x, y in zip(a, b)]], op
        assert list(ca.degrees) == [rm.bitop_degree(op, x, m - 1) for x in a], op      # bitwise_ops.cu:133-185
        assert np.array_equal(c.words(cb), before) and list(cb.degrees) == [m - 1] * len(b), "rhs was touched"
        # scalar form: every (block, clear block) pair
        cs = c.enc([a], 303)
        c.sks.scalar_bitop_assign(cs, b, op, c.st)
        assert c.dec(cs) == [[rm.clear_bitop(op, x, y) for x, y in zip(a, b)]], op
        assert list(cs.degrees) == [rm.bitop_degree(op, y, m - 1) for y in b], op
        # fewer clear blocks than radix blocks: AND clears the rest (degree 0), OR / XOR leave it bit for bit
        row = [m - 1, 1, m - 1, 1, m - 1]
        cs = c.enc([row], 304)
        before = c.words(cs)
        c.sks.scalar_bitop_assign(cs, [1, m - 1], op, c.st)
        want = [rm.clear_bitop(op, row[0], 1), rm.clear_bitop(op, row[1], m - 1)] + ([0] * 3 if op == "and" else row[2:])
        assert c.dec(cs) == [want], op
        assert list(cs.degrees[2:]) == ([0] * 3 if op == "and" else [m - 1] * 3), op
        if op != "and":
            assert np.array_equal(c.words(cs)[0, 2:], before[0, 2:])
    row = list(range(m)) + [m - 1, 0]
    ct = c.enc([row], 305)
    before = c.words(ct)
    c.sks.bitnot_assign(ct, c.st)
    assert c.dec(ct) == [[m - 1 - x for x in row]]
    assert list(ct.degrees) == [m - 1] * len(row)
    c.sks.bitnot_assign(ct, c.st)
    assert np.array_equal(c.words(ct), before), "NOT is a negation plus a constant: twice is the identity on the words"


def eq_candidates(L, m, G, rng):
    """operand pairs (digit rows) of L blocks: the all-pairs row when it fits, equal operands, operands whose first k
    blocks are equal, whose blocks are equal except one, and seeded random equal / unequal patterns"""
    pa, pb = rm.all_pairs(m)
    base_row = [int(v) for v in rng.integers(0, m, size=L)]
    out = []

    def differ(mask):
        return base_row, [(d + 1 + int(rng.integers(0, m - 1))) % m if x else d for d, x in zip(base_row, mask)]

    if L >= m * m:
        out.append((pa + base_row[m * m:], pb + base_row[m * m:]))
    else:
        for at in range(0, m * m, L):
            a, b = (pa + pa)[at:at + L], (pb + pb)[at:at + L]
            out.append((a, b))
    for k in range(L + 1):
        out.append(differ([j >= k for j in range(L)]))
        out.append(differ([j < k for j in range(L)]))
    for j in range(L):
        out.append(differ([i == j for i in range(L)]))
    for g in range(0, L, G):            # whole groups unequal from group g on, the one before it partly
        for s in range(G + 1):
            out.append(differ([(i >= g) or (g - G <= i < g - s) for i in range(L)]))
    for _ in range(40):
        keep = float(rng.random())
        out.append(differ([bool(rng.random() > keep) for _ in range(L)]))
    return out


def eq_cases():
    """(kind, base, blocks, sums): widths 1, G, G + 1 and G^2 + 1 (one, one, two and three levels).  The emulation stops at
    26 blocks.  sums = "all": every pair and every group sum of the width.  Where that costs the emulation minutes (G of 9
    and more on N = 2048) the full case carries the `slow` marker and a case "edges" — the sums 0 and c of every group,
    the equal pairs and one unequal pair per digit — stands unmarked beside it."""
    out = []
    for kind in ("emu", "hip"):
        for b in BASES:
            G = rm.eq_group_size(b.msg, b.carry)
            for L in (1, G, G + 1, G * G + 1):
                if kind == "emu" and L > 26:
                    continue
                name = f"{kind}-{b.name}-{L}_blocks"
                if kind == "emu" and L == 26 and b.name != "multibit_g4_4_4":   # three levels: unmarked on the g = 4 set and at (2, 2)
                    out.append(pytest.param(kind, b, L, "all", id=name + "-everything", marks=[pytest.mark.slow]))
                elif kind == "emu" and G >= 9 and (L > 1 or b.msg == 8):
                    out.append(pytest.param(kind, b, L, "edges", id=name + "-edges"))
                    out.append(pytest.param(kind, b, L, "all", id=name + "-everything", marks=[pytest.mark.slow]))
                else:
                    out.append(pytest.param(kind, b, L, "all", id=name, marks=[pytest.mark.gpu] if kind == "hip" else []))
    return out


@pytest.mark.parametrize("kind,base,L,sums", eq_cases())
def test_equality_sees_every_pair_and_every_group_sum(kind, base, L, sums):
    """eq / ne of L blocks: a bivariate first round, then sums of up to G = (msg carry - 1) / (msg - 1) block results
    against their count, level by level.  The operand pairs are chosen so that every sum 0 .. c of every group size c of
    every level occurs, and at 1 and at G blocks also every pair of digits in the first round (at 1 block ne has a
    first-round table of its own: one call per pair).  Every chosen pair, and an equal one, runs under eq and under ne."""
    c, m = Ctx(kind, base), base.msg
    G = rm.eq_group_size(m, base.carry)
    assert G == {(4, 4): 5, (8, 8): 9, (4, 16): 21, (2, 8): 15, (2, 4): 7, (2, 2): 3}[m, base.carry]
    universe = rm.eq_universe(L, G, with_pairs_of=m if L in (1, G) else None)
    if sums == "edges":
        universe = {e for e in universe if (e[0] == "sum" and e[3] in (0, e[2])) or
                    (e[0] == "pair" and (e[1] == e[2] or (e[1] + 1) % m == e[2]))}
    cand = eq_candidates(L, m, G, np.random.default_rng(311 + L))
    chosen = cover(cand, lambda ab: rm.eq_visits(ab[0], ab[1], m, G), universe, L) + [(cand[0][0], cand[0][0])]
    for n, (a, b) in enumerate(chosen):
        ca, cb = c.enc([a], 320 + n), c.enc([b], 360 + n)
        wa, wb = c.words(ca), c.words(cb)
        for op in ("eq", "ne"):
            out = c.sks.compare(ca, cb, op, c.st)
            assert c.dec(out) == [[int((a == b) == (op == "eq"))]], (op, a, b)
            assert list(out.degrees) == [1]
        assert np.array_equal(c.words(ca), wa) and np.array_equal(c.words(cb), wb), "an operand was touched"
    # against a clear scalar: the first chosen pair, and the equal one
    for (a, b), op in ((chosen[0], "eq"), (chosen[0], "ne"), (chosen[-1], "eq"), (chosen[-1], "ne")):
        out = c.sks.scalar_compare(c.enc([a], 398), rm.value(b, m), op, c.st)
        assert c.dec(out) == [[int((a == b) == (op == "eq"))]], (op, a, b)


@pytest.mark.parametrize("kind,base", ALL)
def test_if_then_else_sees_every_digit_under_both_conditions(kind, base):
    """cmux: both branches packed block + msg * condition; every digit of either branch under condition 0 and 1."""
    c, m = Ctx(kind, base), base.msg
    t = list(range(m)) + [m - 1, 0, m - 1]
    f = list(range(m - 1, -1, -1)) + [m - 1, m - 1, 0]
    seen = set()
    for cond in (0, 1):
        ct, cf, cc = c.enc([t], 331), c.enc([f], 332), c.enc([[cond]], 333 + cond, degree=1)
        wt, wf = c.words(ct), c.words(cf)
        out = c.sks.if_then_else(cc, ct, cf, c.st)
        seen |= {("true", x, cond) for x in t} | {("false", x, cond) for x in f}
        assert c.dec(out) == [t if cond else f], cond
        assert list(out.degrees) == [m - 1] * len(t)
        assert np.array_equal(c.words(ct), wt) and np.array_equal(c.words(cf), wf), "a branch was touched"
    assert seen == {(br, x, cond) for br in ("true", "false") for x in range(m) for cond in (0, 1)}


def shift_pairs(row, sh, bits, left):
    """(current, neighbour) pairs the in-block table of a shift by `sh` is asked: the surviving blocks, each with its lower
    (left shift) or upper (right shift) neighbour, nothing (0) beyond the ends"""
    L, q = len(row), sh // bits
    if sh % bits == 0 or q >= L:
        return set()
    if left:
        return {(row[j], row[j - 1] if j else 0) for j in range(L - q)}
    return {(row[j], row[j + 1] if j + 1 < L else 0) for j in range(q, L)}


@pytest.mark.parametrize("kind,base", ALL)
def test_shifts_by_every_amount(kind, base):
    """Logical shifts by a clear amount: every amount 0 .. bits + 1 in both directions on a narrow integer (whole-block
    moves, in-block shifts, both, none, and the overshift).  At one bit per block there is no table: only block moves."""
    c, m, b = Ctx(kind, base), base.msg, base.bits
    L = 3
    row = [int(v) for v in np.random.default_rng(341).integers(0, m, size=L)]
    row[-1] = m - 1
    a, bits = rm.value(row, m), b * L
    fresh = rm.encrypt_rows(c.p, c.keys, [row], 342)
    for left in (True, False):
        for sh in range(bits + 2):
            ct = c.from_words(fresh)
            c.sks.scalar_shift_assign(ct, sh, c.st, left=left)
            want = (a << sh) % (1 << bits) if left else a >> sh
            assert values(c.dec(ct), m) == [want], (left, sh)
            q, r = min(sh // b, L), sh % b
            deg = list(ct.degrees)
            assert (deg[:q] if left else deg[L - q:]) == [0] * q, (left, sh)            # the blocks shifted in are trivial zeros
            assert (deg[q:] if left else deg[:L - q]) == [m - 1] * (L - q), (left, sh)  # bootstrapped, or moved as they were
            if sh == 0:
                assert np.array_equal(c.words(ct), fresh), "a shift by 0 touched the words"


# 65 blocks at msg = 8: slow on the emulation, the 17-block rows of the bases of 4 beside it
@pytest.mark.parametrize("kind,base,row", [p for p in scoped_cases([x for x in BASES if x.bits > 1], ["de_bruijn"], [])
                                           if p.values[1].msg == 8 and p.values[0] == "emu"] +
                         [p for p in scoped_cases([x for x in BASES if x.bits > 1], ["de_bruijn"], ["de_bruijn"])
                          if not (p.values[1].msg == 8 and p.values[0] == "emu")])
def test_shift_tables_see_every_neighbour_pair(kind, base, row):
    """r = 1 .. bits per block - 1, alone and behind a move by one block, on a row of msg^2 + 1 blocks in which every
    (current, neighbour) pair of digits occurs: the table of every r sees all its msg^2 inputs."""
    c, m, b = Ctx(kind, base), base.msg, base.bits
    row = rm.de_bruijn_row(m)
    a, L = rm.value(row, m), len(row)
    fresh = rm.encrypt_rows(c.p, c.keys, [row], 343)
    everything = {(x, y) for x in range(m) for y in range(m)}
    for left in (True, False):
        for r in range(1, b):
            seen = set()
            for sh in (r, b + r):
                ct = c.from_words(fresh)
                c.sks.scalar_shift_assign(ct, sh, c.st, left=left)
                seen |= shift_pairs(row, sh, b, left)
                want = (a << sh) % (m ** L) if left else a >> sh
                assert values(c.dec(ct), m) == [want], (left, sh)
            assert seen == everything, (left, r)


@pytest.mark.parametrize("kind,base", ALL)
def test_negation_scalar_addition_and_full_propagation(kind, base):
    """The levelled negation (blocks msg - b0, msg - 1 - b_i, degrees [msg, msg - 1, ...]), the levelled scalar addition
    (degree + clear block) and the sequential full propagation after each: every (value, incoming carry) the preceding
    operation can leave occurs, value up to 2 msg - 2 after the scalar addition."""
    c, m = Ctx(kind, base), base.msg
    rng = np.random.default_rng(351)
    # negation: every (value, incoming carry) the full propagation can meet after it
    # after block 0 = msg - 0 the next block meets a carry: every value there; the third block the values without one
    rows = [[0, m - 1 - v] for v in range(m - 1)] + [[0, 0, m - 1] + [m - 1 - v for v in range(1, m)] + [m - 1]]
    seen = set()
    for n, row in enumerate(rows):
        L = len(row)
        ct = c.enc([row], 352 + n)
        before = c.words(ct)
        neg = c.sks.unchecked_neg(ct, c.st)
        raw = [m - row[0]] + [m - 1 - x for x in row[1:]]
        assert c.dec(neg) == [raw], row                                   # negation.cuh:20-49
        assert list(neg.degrees) == [m] + [m - 1] * (L - 1)
        assert np.array_equal(c.words(ct), before), "the input was touched"
        carry = 0
        for v in raw:
            seen.add((v, carry))
            carry = (v + carry) // m
        c.sks.full_propagate_assign(neg, c.st)
        assert values(c.dec(neg), m) == [(-rm.value(row, m)) % m ** L], row
        assert list(neg.degrees) == [m - 1] * L
    assert seen == {(v, 0) for v in range(m + 1)} | {(v, 1) for v in range(m)}
    # scalar addition: candidates of 6 blocks, chosen so that every (digit + clear digit, incoming carry) occurs
    L = 6
    cand = [([int(v) for v in rng.integers(0, m, size=L)], [int(v) for v in rng.integers(0, m, size=L)]) for _ in range(300)]
    cand += [([m - 1] * L, [1] + [0] * (L - 1)), ([m - 1] * L, [m - 1] * L), ([0] * L, [0] * L)]

    def visits(rs):
        out, carry = set(), 0
        for x, y in zip(*rs):
            out.add((x + y, carry))
            carry = (x + y + carry) // m
        return out

    universe = {(v, k) for v in range(2 * m - 1) for k in (0, 1)}
    chosen, missing = rm.greedy_cover(cand, visits, universe)
    assert universe <= set().union(*(visits(rs) for rs in chosen))
    for n, (row, clear) in enumerate(chosen):
        ct = c.enc([row], 360 + n)
        c.sks.unchecked_scalar_add_assign(ct, clear, c.st)
        assert c.dec(ct) == [[x + y for x, y in zip(row, clear)]]
        assert list(ct.degrees) == [m - 1 + y for y in clear]             # scalar_addition.cuh:27-55
        c.sks.full_propagate_assign(ct, c.st)
        assert values(c.dec(ct), m) == [(rm.value(row, m) + rm.value(clear, m)) % m ** L]
        assert list(ct.degrees) == [m - 1] * L
    # fewer clear blocks than radix blocks: only the first ones move, the others stay bit for bit
    row = chosen[0][0]
    ct = c.enc([row], 399)
    before = c.words(ct)
    c.sks.unchecked_scalar_add_assign(ct, [m - 1, 1], c.st)
    assert c.dec(ct) == [[row[0] + m - 1, row[1] + 1] + row[2:]]
    assert list(ct.degrees) == [2 * m - 2, m] + [m - 1] * (L - 2)
    assert np.array_equal(c.words(ct)[0, 2:], before[0, 2:])


# ------------------------------------------------------------------------------------------ carry propagation
def addition_candidates(L, m, rng, count, first_extra):
    """(a row, b row, input carry): seeded random digits, and rows realising seeded carry-state sequences (random digits
    alone seldom make long runs of `propagated`)"""
    out = []
    for n in range(count):
        if n % 2:
            a, b = rm.state_digits([int(v) for v in rng.integers(0, 3, size=L)], m, rng)
        else:
            a, b = ([int(v) for v in rng.integers(0, m, size=L)] for _ in range(2))
        out.append((a, b, int(rng.integers(0, 2)) if first_extra else 0))
    return out


def cover(cand, visits, universe, what):
    chosen, missing = rm.greedy_cover(cand, visits, universe)
    visited = set().union(*(visits(x) for x in chosen))
    assert universe <= visited, (what, sorted(universe - visited, key=repr)[:6])
    return chosen


def signed(v, bits_total):
    return v - (1 << bits_total) if v >> (bits_total - 1) else v


PROPAGATING_BASES = [b for b in BASES if b.propagates]
# (blocks, flag).  5 blocks: the last block is second in its group of three; 7: first in it; 2: no group at all
ADD_SCOPES = [(5, "carry"), (7, "carry"), (5, "overflow"), (2, "overflow")]


@pytest.mark.parametrize("kind,base,scope", scoped_cases(PROPAGATING_BASES, ADD_SCOPES, [(5, "carry")]))
def test_addition_reaches_every_entry_of_the_carry_tables(kind, base, scope):
    """add with an input carry on integers chosen so that every entry the width has is visited.
    flag "carry" (output carry): every block sum 0 .. 2 msg - 2 at the first-bootstrap table of every position, 0 ..
    2 msg - 1 at block 0's, every 4 m + z of the result tables (both at 5 and 7 blocks) and every 4 state + z of the
    output-carry table the last block reads (LUT_OUT_Z at 5 blocks, LUT_OUT_BIT at 7).
    flag "overflow": every (o1, o0, z) of the flag table the last block reads (LUT_OVF_Z at 5 blocks, LUT_OVF_BIT at 2), and
    at 2 blocks every pair of last digits of the overflow preparation."""
    L, flag = scope
    c, m = Ctx(kind, base), base.msg
    top, bits = m ** L, base.bits * L
    cand = addition_candidates(L, m, np.random.default_rng(371 + L), 600, True)
    cand += [([0] * (L - 1) + [x], [0] * (L - 1) + [y], k) for x in range(m) for y in range(m) for k in (0, 1)]
    universe = rm.propagation_universe(m, (L,), flag)
    if flag == "overflow":
        universe = {e for e in universe if e[0] == "ovf"} | {e for e in universe if e[0] == "ovf_pair" and L == 2}

    def visits(x):
        a, b, k = x
        return rm.propagation_visits([p + q for p, q in zip(a, b)], m, k, flag, (a[-1], b[-1]))

    chosen = cover(cand, visits, universe, scope)
    a, b, k = ([x[i] for x in chosen] for i in range(3))
    ca, cb = c.enc(a, 372), c.enc(b, 373)
    wb = c.words(cb)
    cin = c.from_words(encrypt_big(c.p, c.keys, k, seed=374).reshape(len(k), 1, -1), degree=1)
    va, vb = values(a, m), values(b, m)
    out = c.sks.add_assign(ca, cb, c.st, carry_in=cin, want_carry_out=flag == "carry", want_overflow=flag == "overflow")
    if flag == "carry":
        full = [x + y + z for x, y, z in zip(va, vb, k)]
        want = [f // top for f in full]
    else:
        full = [signed(x, bits) + signed(y, bits) + z for x, y, z in zip(va, vb, k)]
        want = [int(not -(1 << (bits - 1)) <= f < (1 << (bits - 1))) for f in full]
    assert values(c.dec(ca), m) == [f % top for f in full]
    assert [r[0] for r in c.dec(out)] == want
    assert list(ca.degrees) == [m - 1] * ca.total_blocks and list(out.degrees) == [1] * len(a)
    assert np.array_equal(c.words(cb), wb), "rhs was touched"


def sub_operands(L, m):
    """operand pairs of L blocks whose subtraction visits every entry the width has: block 0 holds a0 + msg - b0
    (1 .. 2 msg - 1, msg - b0 on top of a clean block), the others a + msg - 1 - b (0 .. 2 msg - 2)"""
    cand = addition_candidates(L, m, np.random.default_rng(381 + L), 600, False)
    cand = [(a, [m - 1 - y for y in b]) for a, b, _ in cand]      # so that a + (msg - 1 - b) takes the drawn sums
    cand += [([0] * L, [0] * L), ([m - 1] * L, [m - 1] * L), ([0] * L, [1] + [0] * (L - 1))]

    def visits(x):
        a, b = x
        return rm.propagation_visits([m - b[0] + a[0]] + [p + m - 1 - q for p, q in zip(a[1:], b[1:])], m, 0, "carry")

    chosen = cover(cand, visits, rm.propagation_universe(m, (L,), "carry", first_sums=range(1, 2 * m)), L)
    return [x[0] for x in chosen], [x[1] for x in chosen]


SUB_SCOPES = [("sub", 5), ("sub", 7), ("overflowing_sub", 5), ("overflowing_sub", 7)]


@pytest.mark.parametrize("kind,base,scope", scoped_cases(PROPAGATING_BASES, SUB_SCOPES, [("sub", 5)]))
def test_subtraction_reaches_every_entry_of_the_carry_tables(kind, base, scope):
    """sub with the carry of lhs + (2^bits - rhs), and the overflowing sub with its borrow, on the covering set of the
    width: every block sum, every 4 m + z of the result tables, every 4 state + z of the output-carry table."""
    op, L = scope
    c, m = Ctx(kind, base), base.msg
    a, b = sub_operands(L, m)
    va, vb, top = values(a, m), values(b, m), m ** L
    ca, cb = c.enc(a, 382), c.enc(b, 383)
    wb = c.words(cb)
    if op == "sub":
        out = c.sks.sub_assign(ca, cb, c.st, want_carry_out=True)
        assert [r[0] for r in c.dec(out)] == [int(x >= y) for x, y in zip(va, vb)]
    else:
        out = c.sks.unsigned_overflowing_sub_assign(ca, cb, c.st)
        assert [r[0] for r in c.dec(out)] == [int(x < y) for x, y in zip(va, vb)]
    assert values(c.dec(ca), m) == [(x - y) % top for x, y in zip(va, vb)]
    assert list(ca.degrees) == [m - 1] * ca.total_blocks
    assert np.array_equal(c.words(cb), wb), "rhs was touched"


ORDERINGS = ("gt", "ge", "lt", "le", "max", "min")


@pytest.mark.parametrize("kind,base,form", scoped_cases(PROPAGATING_BASES, ["ciphertext", "scalar", "equal_operands"], ["ciphertext"]))
def test_orderings_and_selection(kind, base, form):
    """gt / ge / lt / le / max / min of one pair of 5 blocks per call — the first pair of the subtraction's covering set —
    against a ciphertext, against a clear scalar, and of equal operands."""
    c, m, L = Ctx(kind, base), base.msg, 5
    a, b = sub_operands(L, m)
    x, y = a[0], (a[0] if form == "equal_operands" else b[0])
    vx, vy = rm.value(x, m), rm.value(y, m)
    cx, cy = c.enc([x], 385), c.enc([y], 390)
    wx, wy = c.words(cx), c.words(cy)
    clear = {"gt": vx > vy, "ge": vx >= vy, "lt": vx < vy, "le": vx <= vy, "max": max(vx, vy), "min": min(vx, vy)}
    for op in ORDERINGS:
        out = c.sks.scalar_compare(cx, vy, op, c.st) if form == "scalar" else c.sks.compare(cx, cy, op, c.st)
        if op in ("max", "min"):
            assert values(c.dec(out), m) == [clear[op]] and list(out.degrees) == [m - 1] * L, (op, x, y)
        else:
            assert c.dec(out) == [[int(clear[op])]] and list(out.degrees)[:1] == [1], (op, x, y)
    assert np.array_equal(c.words(cx), wx) and np.array_equal(c.words(cy), wy), "an operand was touched"


@pytest.mark.parametrize("kind,base", PROPAGATING)
def test_multiplication_sees_every_product_of_digits(kind, base):
    """mul of msg-block integers: digits 0 .. msg - 1 times 0 .. msg - 1 computes the products x y with x + y < msg (the
    others fall off the top), the reversed rows the ones with x + y >= msg - 1: together every entry of the two product
    tables (low and high half)."""
    c, m = Ctx(kind, base), base.msg
    L = m
    a = [list(range(m)), list(range(m - 1, -1, -1))]
    seen = {(x[i], y[j]) for x, y in zip(a, a) for i in range(L) for j in range(L - i)}
    assert seen == {(x, y) for x in range(m) for y in range(m)}
    ca, cb = c.enc(a, 401), c.enc(a, 402)
    wb = c.words(cb)
    c.sks.mul_assign(ca, cb, c.st)
    rows = c.dec(ca)
    assert all(0 <= d < m for r in rows for d in r)
    assert values(rows, m) == [(v * v) % m ** L for v in values(a, m)]
    assert list(ca.degrees) == [m - 1] * ca.total_blocks
    assert np.array_equal(c.words(cb), wb), "rhs was touched"


# ================================================================================== 3. carry-state sequences
SEQUENCE_BASES = [b for b in BASES if b.name in ("classic_4_4", "classic_8_8", "classic_4_16", "multibit_g4_4_4")]


def sequence_cases():
    """(kind, base, blocks, sequences): 2,187 sequences on the MI355X (all of them at 7 blocks), on the emulation the
    3 + 2 L that must be there and one seeded one; its 13-block cases on N = 2048 classic keys (39 bootstraps an integer)
    carry the `slow` marker, the 7-block ones beside them do not."""
    out = []
    for p in cases(SEQUENCE_BASES):
        kind, base = p.values
        for L in (7, 13):
            slow = kind == "emu" and L == 13 and not base.emu.grouping
            out.append(pytest.param(kind, base, L, 2187 if kind == "hip" else 3 + 2 * L + 1,
                                    id=f"{p.id}-{L}" + ("-everything" if slow else ""),
                                    marks=list(p.marks) + ([pytest.mark.slow] if slow else [])))
    return out


@pytest.mark.parametrize("kind,base,L,count", sequence_cases())
def test_every_carry_state_sequence(kind, base, L, count):
    """Block sums below msg - 1, equal to it, at least msg: {none, propagated, generated}^L.  7 blocks: groups of three
    under a top of three; 13 blocks: the last group is a single block under a top of four plus one.  `count` sequences:
    2,187 are ALL 3^7 at 7 blocks and a seeded sample at 13, each with input carry 0 and 1 (4,374 integers), each integer
    under the output carry AND under the signed-overflow flag.  A count of 3 + 2 L + 1 holds the sequences that must be
    there — all propagated (with an input carry: the ripple through every block), all generated, generated at block 0
    then all propagated, every sequence one block away from all propagated — and a seeded one, each once, input carries
    and the two flags alternating.  Result and flag against clear arithmetic."""
    c, m = Ctx(kind, base), base.msg
    rng = np.random.default_rng(411 + L)
    exhaustive = count >= 2000
    seqs = rm.state_sequences(L, count, rng, neighbours=True)
    assert len(seqs) == count and (L != 7 or not exhaustive or len(set(seqs)) == 3 ** 7)
    # not exhaustive: the first three (all propagated, all generated, generated then propagated) under both carries and
    # both flags, the others once, carries and flags alternating
    jobs = [(s, k) for s in seqs for k in (0, 1)] if exhaustive else \
        [(s, k) for s in seqs[:3] for k in (0, 1)] + [(s, n % 2) for n, s in enumerate(seqs[3:])]
    P, G_ = rm.PROPAGATED, rm.GENERATED
    have = set(jobs)
    for s in [(P,) * L, (G_,) * L, (G_,) + (P,) * (L - 1)]:
        assert (s, 1) in have or (s, 0) in have
    assert ((P,) * L, 1) in have, "the ripple through every block"
    for j in range(L):
        assert any(((P,) * j + (x,) + (P,) * (L - 1 - j), k) in have for x in (rm.NONE, G_) for k in (0, 1))
    rows = [rm.state_digits(s, m, rng) for s, _ in jobs]
    a, b, k = [r[0] for r in rows], [r[1] for r in rows], [k for _, k in jobs]
    # the digits realise the states, and their sums vary
    assert all(tuple(rm.block_state(x + y, m) for x, y in zip(ra, rb)) == s for ra, rb, (s, _) in zip(a, b, jobs))
    if exhaustive:
        assert {x + y for ra, rb in zip(a, b) for x, y in zip(ra, rb)} == set(range(2 * m - 1))
    top, bits = m ** L, base.bits * L
    va, vb = values(a, m), values(b, m)
    step = 1458                      # integers per call: the operands of one call stay below 320 MB
    # exhaustive: every integer under both flags; else the flags alternate with the carries (n % 4)
    passes = [("carry", range(len(jobs))), ("overflow", range(len(jobs)))] if exhaustive else \
        [("carry", [n for n in range(len(jobs)) if n < 6 or n % 4 < 2]), ("overflow", [n for n in range(len(jobs)) if n < 6 or n % 4 >= 2])]
    for flag, which in passes:
        for at in range(0, len(which), step):
            idx = list(which[at:at + step])
            pa, pb, pk = [a[i] for i in idx], [b[i] for i in idx], [k[i] for i in idx]
            ca, cb = c.enc(pa, 412), c.enc(pb, 413)
            cin = c.from_words(rm.encrypt_rows(c.p, c.keys, [[x] for x in pk], 414), degree=1)
            out = c.sks.add_assign(ca, cb, c.st, carry_in=cin, want_carry_out=flag == "carry", want_overflow=flag == "overflow")
            got, got_flag = values(c.dec(ca), m), [r[0] for r in c.dec(out)]
            if flag == "carry":
                full = [va[i] + vb[i] + k[i] for i in idx]
                want_flag = [f // top for f in full]
            else:
                full = [signed(va[i], bits) + signed(vb[i], bits) + k[i] for i in idx]
                want_flag = [int(not -(1 << (bits - 1)) <= f < (1 << (bits - 1))) for f in full]
            bad = [i for i, f in enumerate(full) if got[i] != f % top or got_flag[i] != want_flag[i]]
            assert not bad, (flag, [(jobs[idx[i]], a[idx[i]], b[idx[i]]) for i in bad[:3]])


# ================================================================================== 4. device = emulation
WORD_BASES = [b for b in BASES if b.name in ("classic_4_4", "classic_8_8", "classic_4_16", "multibit_g3_4_4",
                                             "multibit_g4_4_4", "classic_2_8")]


def run_sequence(c, words, cond_words):
    """The operations of the issue's list on one backend, from the same input words; (step name, words, degrees) of every
    result.  At a base without carry propagation only the propagation-free steps run."""
    m, st, sks = c.msg, c.st, c.sks
    mk = lambda i: c.from_words(words[i:i + 1])
    L = words.shape[1]
    out = []
    keep = lambda name, ct: out.append((name, c.words(ct), list(ct.degrees)))
    if c.base.propagates:
        x = mk(0)
        flag = sks.add_assign(x, mk(1), st, carry_in=c.from_words(cond_words, degree=1), want_carry_out=True)
        keep("add", x), keep("add carry", flag)
        x = mk(0)
        sks.sub_assign(x, mk(1), st)
        keep("sub", x)
        x = mk(0)
        sks.mul_assign(x, mk(1), st)
        keep("mul", x)
    x = mk(0)
    sks.bitop_assign(x, mk(1), "xor", st)
    keep("bitxor", x)
    x = mk(0)
    sks.scalar_bitop_assign(x, [(3 * j + 1) % m for j in range(L - 1)], "and", st)
    keep("scalar and", x)
    if c.base.propagates:
        keep("gt", sks.compare(mk(0), mk(1), "gt", st))
    keep("eq", sks.compare(mk(0), mk(1), "eq", st))
    if c.base.propagates:
        keep("max", sks.compare(mk(0), mk(1), "max", st))
    keep("if_then_else", sks.if_then_else(c.from_words(cond_words, degree=1), mk(0), mk(1), st))
    for left in (True, False):
        x = mk(0)
        sks.scalar_shift_assign(x, c.base.bits + 1 if c.base.bits > 1 else 1, st, left=left)
        keep("shift left" if left else "shift right", x)
    x = sks.unchecked_neg(mk(0), st)
    keep("neg", x)
    sks.full_propagate_assign(x, st)
    keep("neg + full propagation", x)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("base", WORD_BASES, ids=[b.name for b in WORD_BASES])
def test_device_equals_emulation_word_for_word(base):
    """Same keys, same input ciphertexts, same sequence of operations on the MI355X and on the host emulation: the words
    of every result and its degrees are equal.  tests/test_backend_parity.py pins both backends to the oracle bit for
    bit on these toy sets, so equality is the expectation, not a tolerance."""
    p = base.hip if base.hip is not C1 else base.emu       # toy keys on both sides
    toy = dataclasses.replace(base, hip=p, emu=p)
    keys = make_keys(p)
    L, m = 5, base.msg
    rng = np.random.default_rng(421)
    rows = [[int(v) for v in rng.integers(0, m, size=L)] for _ in range(2)]
    rows[0][2], rows[1][2] = m - 1, 0                      # a propagating block between a generating and an absorbing one
    words = rm.encrypt_rows(p, keys, rows, 422)
    cond = rm.encrypt_rows(p, keys, [[1]], 423)
    try:
        got = run_sequence(Ctx("hip", toy), words, cond)
        gc.collect()                                       # device buffers are released through the library that made them
        want = run_sequence(Ctx("emu", toy), words, cond)
    finally:
        use_backend("hip")
    assert [n for n, _, _ in got] == [n for n, _, _ in want]
    for (name, w_hip, d_hip), (_, w_emu, d_emu) in zip(got, want):
        assert np.array_equal(w_hip, w_emu), f"{name}: the device's words differ from the emulation's"
        assert d_hip == d_emu, name
    # and the last step decrypts to the clear result
    assert values(rm.decrypt_many(p, keys, got[-1][1]).tolist(), m) == [(-rm.value(rows[0], m)) % m ** L]


# ================================================================================== 5. refusals
REFUSAL_PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
N, n = 256, 4
def BK(N=N): return ffi.CudaLweBootstrapKeyParamsFFI(n, 1, N, 8, 2, N, 1, 0)
def KK(N=N): return ffi.CudaLweKeyswitchKeyParamsFFI(N, n, 4, 3)
keys = (C.c_void_p * 1)(gpu.CudaVec(16, st).ptr)
def radix(blocks, degree=3):
    ct = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec(blocks * (N + 1), st), 1, blocks, N)
    ct.set_degrees(degree)
    return ct
def scratch(name, *args, msg=4, carry=4, N=N):
    mem = C.c_void_p()
    getattr(lib, "scratch_cuda_" + name)(s, C.byref(mem), BK(N), KK(N), *args[:1], msg, carry, *args[1:], True, 0)
    return mem
alive = []
def R(ct):
    alive.extend([ct, ct._ffi()])       # the library reads the degrees through pointers into these
    return C.byref(alive[-1])
clear = np.array([1, 2, 3, 0, 1], dtype=np.uint64)
d_clear = gpu.CudaVec.from_cpu_async(clear, st)
H = clear.ctypes.data_as(C.c_void_p)
"""

SUB = "sub_and_propagate_single_carry_64_inplace_async"
REFUSALS = {
    "dirty operand to sub": (f"""
        mem = scratch("{SUB}", 3, 0)
        lib.cuda_{SUB}(s, R(radix(3)), R(radix(3, 4)), R(radix(1)), R(radix(1)), mem, keys, keys, 0, 0)
        """, "sub_and_propagate_single_carry: block 0 has degree 4, the subtraction takes clean operands"),
    "dirty operand to a comparison": ("""
        mem = scratch("integer_comparison_64_async", 3, 2, False)
        lib.cuda_integer_comparison_64_async(s, R(radix(1)), R(radix(3, 5)), R(radix(3)), mem, keys, keys)
        """, "integer_comparison: block 0 has degree 5, the comparison takes clean operands"),
    "dirty branch to cmux": ("""
        mem = scratch("cmux_64_async", 3)
        lib.cuda_cmux_64_async(s, R(radix(3)), R(radix(1, 1)), R(radix(3)), R(radix(3, 4)), mem, keys, keys)
        """, "cmux: block 0 has degree 4, the branches must be clean"),
    "cmux condition of degree 2": ("""
        mem = scratch("cmux_64_async", 3)
        lib.cuda_cmux_64_async(s, R(radix(3)), R(radix(1, 2)), R(radix(3)), R(radix(3)), mem, keys, keys)
        """, "cmux: the condition must be a boolean block (degree 2)"),
    "dirty operand to a shift": ("""
        mem = scratch("logical_scalar_shift_64_inplace_async", 3, 0)
        lib.cuda_logical_scalar_shift_64_inplace_async(s, R(radix(3, 6)), 1, mem, keys, keys)
        """, "logical_scalar_shift: block 0 has degree 6, the shift takes clean blocks"),
    "dirty operand to a bitop": ("""
        mem = scratch("integer_bitop_inplace_64_async", 3, 0)
        lib.cuda_integer_bitop_inplace_64_async(s, R(radix(3)), R(radix(3, 4)), mem, keys, keys)
        """, "integer_bitop: block 0 carries a degree of 3 / 4, the packed pair needs clean blocks"),
    "an input carry on sub": (f"""
        mem = scratch("{SUB}", 3, 0)
        lib.cuda_{SUB}(s, R(radix(3)), R(radix(3)), R(radix(1)), R(radix(1)), mem, keys, keys, 0, 1)
        """, "sub_and_propagate_single_carry: an input carry is not wired"),
    "FLAG_OVERFLOW on the sub scratch": (f"""
        scratch("{SUB}", 3, 1)
        """, "sub_and_propagate_single_carry: output flag 1 is not wired"),
    "FLAG_OVERFLOW on the sub launch": (f"""
        mem = scratch("{SUB}", 3, 0)
        lib.cuda_{SUB}(s, R(radix(3)), R(radix(3)), R(radix(1)), R(radix(1)), mem, keys, keys, 1, 0)
        """, "sub_and_propagate_single_carry: output flag 1 is not wired"),
    "an input borrow on overflowing sub": ("""
        mem = scratch("integer_overflowing_sub_64_inplace_async", 3, 1)
        lib.cuda_integer_overflowing_sub_64_inplace_async(s, R(radix(3)), R(radix(3)), R(radix(1)), R(radix(1)), mem, keys, keys, 1, 1)
        """, "integer_overflowing_sub: an input borrow is not wired"),
    "a rotation passed to the shift scratch": ("""
        scratch("logical_scalar_shift_64_inplace_async", 3, 2)
        """, "logical_scalar_shift: shift type 2 is a rotation"),
    "a message modulus that is no power of two for the shift": ("""
        scratch("logical_scalar_shift_64_inplace_async", 3, 0, msg=3, carry=8, N=768)
        """, "logical_scalar_shift: the message modulus must be a power of two"),
    "signed comparison": ("""
        scratch("integer_comparison_64_async", 3, 2, True)
        """, "integer_comparison: signed operands are not wired"),
    "a bitop scratch at the scalar entry point": ("""
        mem = scratch("integer_bitop_inplace_64_async", 3, 0)
        lib.cuda_integer_scalar_bitop_inplace_64_async(s, R(radix(3)), d_clear.ptr, H, 3, mem, keys, keys)
        """, "integer_scalar_bitop: foreign scratch pointer"),
    "a scalar bitop scratch at the ciphertext entry point": ("""
        mem = scratch("integer_scalar_bitop_inplace_64_async", 3, 3)
        lib.cuda_integer_bitop_inplace_64_async(s, R(radix(3)), R(radix(3)), mem, keys, keys)
        """, "integer_bitop: foreign scratch pointer"),
    "a ciphertext operation code at the scalar bitop scratch": ("""
        scratch("integer_scalar_bitop_inplace_64_async", 3, 0)
        """, "bitop: operation 0 does not belong to this entry point"),
    "more clear blocks than radix blocks in a scalar bitop": ("""
        mem = scratch("integer_scalar_bitop_inplace_64_async", 5, 3)
        lib.cuda_integer_scalar_bitop_inplace_64_async(s, R(radix(3)), d_clear.ptr, H, 4, mem, keys, keys)
        """, "integer_scalar_bitop: 4 clear blocks for 3 radix blocks"),
    "more scalar blocks than radix blocks in a scalar comparison": ("""
        mem = scratch("integer_scalar_comparison_64_async", 3, 0, False)
        lib.cuda_integer_scalar_comparison_64_async(s, R(radix(1)), R(radix(3)), d_clear.ptr, H, mem, keys, keys, 4)
        """, "integer_scalar_comparison: 4 scalar blocks for 3 radix blocks"),
    "a clear block of the message modulus in a scalar bitop": ("""
        mem = scratch("integer_scalar_bitop_inplace_64_async", 3, 3, msg=2, carry=8)
        lib.cuda_integer_scalar_bitop_inplace_64_async(s, R(radix(3, 1)), d_clear.ptr, H, 2, mem, keys, keys)
        """, "integer_scalar_bitop: clear block 1 is 2, not below the message modulus"),
    "a clear block of the message modulus in a scalar comparison": ("""
        mem = scratch("integer_scalar_comparison_64_async", 3, 0, False, msg=2, carry=8)
        lib.cuda_integer_scalar_comparison_64_async(s, R(radix(1)), R(radix(3, 1)), d_clear.ptr, H, mem, keys, keys, 3)
        """, "integer_scalar_comparison: scalar block 1 is 2, not below the message modulus"),
    "carry modulus below the message modulus": ("""
        scratch("cmux_64_async", 3, msg=4, carry=2)
        """, "radix layer: unsupported message/carry moduli (4, 2)"),
    "a plaintext space that does not divide the polynomial": ("""
        scratch("integer_bitop_inplace_64_async", 3, 0, msg=3, carry=3)
        """, "radix layer: unsupported message/carry moduli (3, 3)"),
    "carry propagation at one bit per block": ("""
        lib.scratch_cuda_propagate_single_carry_64_inplace_async(s, C.byref(C.c_void_p()), BK(), KK(), 3, 2, 8, 0, True, 0)
        """, "carry propagation: message_modulus 2 < 3 is not supported"),
    "subtraction at one bit per block": (f"""
        scratch("{SUB}", 3, 0, msg=2, carry=8)
        """, "carry propagation: message_modulus 2 < 3 is not supported"),
    "an ordering at one bit per block": ("""
        scratch("integer_comparison_64_async", 3, 2, False, msg=2, carry=8)
        """, "carry propagation: message_modulus 2 < 3 is not supported"),
    "carry propagation below 16 values per block": ("""
        lib.scratch_cuda_propagate_single_carry_64_inplace_async(s, C.byref(C.c_void_p()), BK(), KK(), 3, 2, 4, 0, True, 0)
        """, "carry propagation needs at least 4 bits per block"),
    "carry propagation at msg 3 with 12 values per block": ("""
        lib.scratch_cuda_propagate_single_carry_64_inplace_async(s, C.byref(C.c_void_p()), BK(768), KK(768), 3, 3, 4, 0, True, 0)
        """, "carry propagation needs at least 4 bits per block"),
    "max at 8 values per block": ("""
        scratch("integer_comparison_64_async", 3, 6, False, msg=2, carry=4)
        """, "carry propagation needs at least 4 bits per block"),
    "more integers than the add scratch holds": ("""
        mem = C.c_void_p()
        lib.scratch_cuda_add_and_propagate_single_carry_64_inplace_async(s, C.byref(mem), BK(), KK(), 3, 4, 4, 0, True, 0)
        lib.cuda_add_and_propagate_single_carry_64_inplace_async(s, R(radix(6)), R(radix(6)), R(radix(2)), R(radix(2)), mem, keys, keys, 0, 0)
        """, "carry propagation: 2 integers exceed the scratch capacity 1"),
    "operands wider than the bitop scratch": ("""
        mem = scratch("integer_bitop_inplace_64_async", 3, 0)
        lib.cuda_integer_bitop_inplace_64_async(s, R(radix(4)), R(radix(4)), mem, keys, keys)
        """, "integer_bitop: 4 blocks exceed the scratch capacity 3"),
    "operands wider than the comparison scratch": ("""
        mem = scratch("integer_comparison_64_async", 3, 0, False)
        lib.cuda_integer_comparison_64_async(s, R(radix(1)), R(radix(4)), R(radix(4)), mem, keys, keys)
        """, "integer_comparison: the operands must hold the 3 blocks the scratch was made for"),
    "branches wider than the cmux scratch": ("""
        mem = scratch("cmux_64_async", 3)
        lib.cuda_cmux_64_async(s, R(radix(4)), R(radix(1, 1)), R(radix(4)), R(radix(4)), mem, keys, keys)
        """, "cmux: the branches must hold the 3 blocks the scratch was made for"),
    "an integer narrower than the shift scratch": ("""
        mem = scratch("logical_scalar_shift_64_inplace_async", 4, 0)
        lib.cuda_logical_scalar_shift_64_inplace_async(s, R(radix(3)), 1, mem, keys, keys)
        """, "input does not have enough blocks"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_radix_misuse_is_refused_with_a_message(name):
    """On the host emulation only, in a child process: the library aborts with a message that names the entry point (an
    abort is never provoked on a GPU)."""
    import signal
    snippet, message = REFUSALS[name]
    r = run_child(REFUSAL_PRELUDE + textwrap.dedent(snippet))
    assert r.returncode == -signal.SIGABRT, f"{name}: returned {r.returncode}\n{r.stderr[-600:]}"
    assert message in r.stderr, r.stderr[-600:]
