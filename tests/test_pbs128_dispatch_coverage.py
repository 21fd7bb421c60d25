"""Every (polynomial size, k + 1) pair pbs128_dispatch lists, the fixed production instantiation on and off its
decomposition, and the edges of the u128 decomposition inside a bootstrap, each at the smallest shape at which the kernel
can still go wrong (n of 3, 4 or 8; the four toy sets of tests/test_pbs128.py keep their n = 16).

One row is one launch of six LWEs under a non-trivial table: four encryptions (messages 0, 5, 10, 15) and two crafted
mask / body patterns that are no encryptions (mask words that switch to 0, to N, that round up to 2 N and wrap, that lie
on and either side of a rounding boundary; bodies that switch to 0 directly and by wrapping).  The expected values are
the exact-product bootstrap of tests/pbs128_helper.py in phase and, on the device, the host emulation word for word.

Measured figures are printed before every assertion on them (run with -s to see them)."""
import dataclasses
import math
import os
import re
import statistics
import time

import numpy as np
import pytest

from . import pbs128_helper as h
from .harness import use_backend
from .test_pbs128 import BACKENDS, nontrivial, phase_bound, run_pbs, setup, upload_key

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
HEADER = os.path.join(ROOT, "tfhe_rs_amd", "csrc", "pbs128.h")
MESSAGES = (0, 5, 10, 15)
PLAIN, CENTRED = 0, 1


@dataclasses.dataclass(frozen=True)
class Row:
    p: h.Params128
    only_cover: tuple   # the one requirement of required_cover() that no other row is listed for

    @property
    def id(self):
        return self.p.name.replace("toy128_", "")


def _row(name, k, N, decomposition, n, switch, only_cover):
    return Row(h.Params128("toy128_" + name, n, k, N, *decomposition, ms_type=switch), only_cover)


ROWS = [
    Row(h.TOYS[0], ("pair", 256, 2)),
    Row(h.TOYS[1], ("pair", 256, 3)),
    Row(h.TOYS[2], ("pair", 512, 2)),
    Row(h.TOYS[3], ("pair", 512, 3)),
    _row("k3_N256", 3, 256, (24, 3), 4, CENTRED, ("pair", 256, 4)),
    _row("k3_N256_b32l4", 3, 256, (32, 4), 8, CENTRED, ("first base_log on the double-double digit path",)),
    _row("k1_N256_b31l4", 1, 256, (31, 4), 8, PLAIN, ("last base_log on the single-double digit path",)),
    _row("k1_N512_b64l1", 1, 512, (64, 1), 8, PLAIN, ("level 1",)),
    _row("k3_N512_b33l3", 3, 512, (33, 3), 3, PLAIN, ("pair", 512, 4)),
    _row("k1_N1024_b64l2", 1, 1024, (64, 2), 4, PLAIN, ("pair", 1024, 2)),
    _row("k2_N1024_b43l2", 2, 1024, (43, 2), 3, CENTRED, ("pair", 1024, 3)),
    _row("k3_N1024", 3, 1024, (24, 3), 3, CENTRED, ("pair", 1024, 4)),
    _row("k1_N2048_b42l3", 1, 2048, (42, 3), 3, PLAIN, ("pair", 2048, 2)),
    _row("k2_N2048_b20l4", 2, 2048, (20, 4), 3, CENTRED, ("pair", 2048, 3)),
    _row("k2_N2048_fixed", 2, 2048, (24, 3), 3, CENTRED, ("fixed", 2048, 3)),
    _row("k1_N4096_b32l4", 1, 4096, (32, 4), 3, CENTRED, ("pair", 4096, 2)),
]


# ------------------------------------------------------------------------------------------------ inputs, expected values
def crafted_inputs(p):
    """Two LWEs that are no encryptions.  unit = 2^64 / 2 N is one step of the switched modulus; the pool holds a word
    that switches to 0, one to N, one that rounds up to 2 N and wraps to 0, one to 1, one exactly on a rounding boundary
    (N - 1/2 steps), and one on (1/2 step), just below and a whole step above (N + 1) such a boundary."""
    unit = 1 << (64 - p.log2N2)
    pool = [0, 1 << 63, (1 << 64) - 1, unit, (1 << 63) - unit // 2, unit // 2, unit // 2 - 1, (1 << 63) + unit]
    first = [pool[i % 8] for i in range(p.n)] + [0]
    second = [pool[(i + 3) % 8] for i in range(p.n)] + [(1 << 64) - 1 - unit // 4]
    return np.array([first, second], dtype=np.uint64)


_cases = {}


def case_of(row):
    """keys, the six inputs, the table and the exact bootstrap's six output phases: computed once per session and shared
    by both backends"""
    p = row.p
    if p.name not in _cases:
        keys = h.make_keys128(p)
        lwes = np.concatenate([h.encrypt_inputs(p, keys, MESSAGES, seed=47), crafted_inputs(p)])
        lut = h.make_lut128(p, nontrivial)
        t0 = time.time()
        want = h.exact_phases(p, lwes, [lut] * len(lwes))
        print(f"{p.name}: exact restatement of {len(lwes)} bootstraps took {time.time() - t0:.1f} s")
        for m, w in zip(MESSAGES, want):   # the expected values themselves decode
            assert h.decode128(w) == nontrivial(m), (p.name, m)
        _cases[p.name] = (keys, lwes, lut, want)
    return _cases[p.name]


def launch_and_check(kind, row):
    """checks (a) .. (d) on one backend; returns the six output LWEs"""
    lib, gpu, st = setup(kind)
    p = row.p
    keys, lwes, lut, want = case_of(row)
    bsk = upload_key(gpu, st, p, keys)
    out = run_pbs(gpu, st, p, bsk, lwes, lut)
    again = run_pbs(gpu, st, p, bsk, lwes, lut)
    alone = run_pbs(gpu, st, p, bsk, lwes[3:4], lut)
    assert out.shape == (len(lwes), p.k * p.N + 1, 2)
    phases = [h.phase128(p, keys, o) for o in out]
    dists = [h.torus_distance128(a, b) for a, b in zip(phases, want)]
    G = phase_bound(p)
    print(f"{p.name} [{kind}]: phase distance to the exact bootstrap: max 2^{math.log2(max(max(dists), 1)):.1f}, "
          f"median 2^{math.log2(max(statistics.median(dists), 1)):.1f}, bound 2^{math.log2(G):.1f}")
    assert max(dists) <= G, (p.name, kind, dists)                                                  # (a)
    assert [h.decode128(ph) for ph in phases[:len(MESSAGES)]] == [nontrivial(m) for m in MESSAGES]   # (b)
    assert np.array_equal(again, out), "two calls on the same inputs differ"                       # (c)
    assert np.array_equal(alone, out[3:4]), "a launch of one sample differs from its row of the batch"   # (d)
    return out


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
@pytest.mark.parametrize("kind", BACKENDS)
def test_bootstrap_row(kind, row):
    """(a) every output phase within G of the exact bootstrap's, crafted inputs included; (b) the encrypted inputs
    decode; (c) a second call returns identical words; (d) a one-sample launch equals its row of the batch; on the
    device, also: the six outputs equal the host emulation's word for word."""
    out = launch_and_check(kind, row)
    if kind == "hip":
        try:
            emu = launch_and_check("emu", row)
        finally:
            use_backend("hip")
        differing = int((emu != out).any(axis=(1, 2)).sum())
        print(f"{row.p.name}: hip vs emu: {differing} of {len(out)} ciphertexts differ")
        assert np.array_equal(emu, out)


def test_crafted_inputs_switch_to_the_values_they_are_crafted_for():
    """Under the plain switch the pool's words become 0, N, 0 (rounded up to 2 N and wrapped), 1, N (a tie, rounded up),
    1 (a tie), 0 and N + 1; the first body becomes 0 and the second rounds up to 2 N and wraps to 0.  (Under the centred
    switch the same words are shifted by the mean correction first; they are then just unusual inputs.)"""
    for N in (256, 4096):
        p = h.Params128("crafted", 8, 1, N, 24, 3)
        first, second = crafted_inputs(p)
        assert h.lwe_modulus_switch(first, p.log2N2, PLAIN) == [0, N, 0, 1, N, 1, 0, N + 1, 0]
        assert h.lwe_modulus_switch(second, p.log2N2, PLAIN) == [1, N, 1, 0, N + 1, 0, N, 0, 0]
        assert int(second[-1]) + (1 << (63 - p.log2N2)) >= 1 << 64   # it is the rounding that wraps it


# ------------------------------------------------------------------------------------------------ completeness
def dispatched():
    """what pbs128.h can launch: the (N, k + 1) pairs of pbs128_dispatch, {(N, k + 1): (base_log, level)} of the fixed
    instantiations of launch_pbs128_nk, and the largest base_log digit_to_f128 turns into one double"""
    text = open(HEADER).read()
    body = text[text.index("inline bool pbs128_dispatch("):]
    body = body[body.index("#define HX_PBS128_CASE"):body.index("#undef HX_PBS128_CASE")]
    pairs = [(int(N), int(K1)) for N, K1 in re.findall(r"HX_PBS128_CASE\((\d+), (\d+)\)", body)]
    nk = text[text.index("static void launch_pbs128_nk("):text.index("inline bool pbs128_dispatch(")]
    fixed = {}
    for N, K1, tail in re.findall(r"if constexpr \(N == (\d+) && K1 == (\d+)\) \{(.*?)\n  \}", nk, re.S):
        for bl, lv, tbl, tlv in re.findall(r"a\.base_log == (\d+) && a\.level == (\d+)\) return "
                                           r"launch_pbs128_inst<N, K1, (\d+), (\d+)>", tail):
            assert (bl, lv) == (tbl, tlv), "a fixed instantiation selected by another decomposition than its own"
            fixed[(int(N), int(K1))] = (int(bl), int(lv))
    assert len(re.findall(r"launch_pbs128_inst<", nk)) == len(fixed) + 1, "launch_pbs128_nk: a launch this test cannot read"
    single = re.search(r"HX_DEV f128 digit_to_f128\(.*?base_log <= (\d+)\) return f128\{\(double\)", text, re.S)
    assert single, "digit_to_f128: the width of the single-double path was not found"
    return pairs, fixed, int(single.group(1))


def required_cover():
    pairs, fixed, single = dispatched()
    need = {("pair", N, K1): (lambda p, N=N, K1=K1: (p.N, p.k + 1) == (N, K1)
                              and (p.base_log, p.level) != fixed.get((N, K1))) for N, K1 in pairs}
    for (N, K1), decomposition in fixed.items():
        need[("fixed", N, K1)] = lambda p, N=N, K1=K1, d=decomposition: (p.N, p.k + 1, p.base_log, p.level) == (N, K1, *d)
    need[("last base_log on the single-double digit path",)] = lambda p: p.base_log == single
    need[("first base_log on the double-double digit path",)] = lambda p: p.base_log == single + 1
    need[("level 1",)] = lambda p: p.level == 1
    return need


def test_every_dispatched_instantiation_and_decomposition_edge_has_a_row():
    """Reads pbs128.h.  Every (N, k + 1) pair of the dispatcher needs a row off any fixed decomposition of that pair, every
    fixed instantiation a row on its decomposition, both sides of the digit conversion's branch and level 1 a row each;
    every row is listed for exactly one of these and fulfils it, so taking any row out leaves one uncovered.  A row for a
    pair the dispatcher does not list fails too.  Besides: some row represents all 128 bits with digits of 64 bits."""
    pairs, fixed, single = dispatched()
    assert len(pairs) == len(set(pairs)) and set(fixed) <= set(pairs)
    stray = [r.id for r in ROWS if (r.p.N, r.p.k + 1) not in pairs]
    assert not stray, f"rows for pairs the dispatcher does not list: {stray}"
    need = required_cover()
    listed = {}
    for r in ROWS:
        assert r.only_cover in need, f"{r.id} is listed for {r.only_cover}, which the header does not ask for"
        assert need[r.only_cover](r.p), f"{r.id} does not cover {r.only_cover}"
        assert r.only_cover not in listed, f"{r.id} and {listed[r.only_cover]} are both listed for {r.only_cover}"
        listed[r.only_cover] = r.id
    missing = sorted(set(need) - set(listed), key=str)
    assert not missing, f"without a row: {missing}"
    assert any(r.p.base_log == 64 and r.p.base_log * r.p.level == 128 for r in ROWS)


def test_rows_are_consistent():
    ids = [r.id for r in ROWS]
    assert len(ids) == len(set(ids)) and len({r.p.name for r in ROWS}) == len(ROWS)
    for r in ROWS:
        p = r.p
        assert 1 <= p.base_log <= 64 and p.base_log * p.level <= 128, r.id
        assert p.n <= 16 and p.ms_type in (PLAIN, CENTRED), r.id
