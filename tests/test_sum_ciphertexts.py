"""Sum of a vector of radix ciphertexts (hip_*_partial_sum_ciphertexts_vec_64) and the gather-sum kernel under it: sums that
need no bootstrap against the wrapping NumPy sum of the input rows word for word (257-, 2049- and 8193-word rows, the
output apart from the vector and in its first integer), sums that reduce their columns with and without the degrees one
carry propagation accepts, blocks of degree 0, and the refusals in a child process.

The checker is clear big-integer arithmetic on the decrypted blocks; nothing reads the library's tables.
[emu] runs the kernel sources on the host, [hip] on the MI355X (anchor row: PARAM_MESSAGE_2_CARRY_2)."""
import textwrap

import numpy as np
import pytest

from . import radix_model as rm
from .common import C1, TOY_2048, TOY_8192, TOY_K1
from .test_error_behaviour import run as run_child
from .test_radix_bases import BASES, Ctx, cases
from .test_radix_integer import setup

U64 = np.uint64
ANCHOR = cases(BASES[:1])
MSG, CARRY, L = 4, 4, 3
ROWS = [pytest.param(kind, p, id=f"{kind}-{p.name}", marks=[pytest.mark.gpu] if kind == "hip" else [])
        for kind in ("emu", "hip") for p in (TOY_K1, TOY_2048 if kind == "emu" else C1, TOY_8192)]


@pytest.mark.parametrize("kind,p", ROWS)
def test_sums_that_need_no_bootstrap_are_the_wrapping_sums_of_the_rows(kind, p):
    """V = 1, 2 and 5 integers of clean blocks fit a block of (4, 4) as they are: no bootstrap, and every output word is the
    wrapping sum of the input words — whatever the words are (random ones here), so rows of any key's length serve.  Then
    the same with the output in the vector's first integer."""
    p, keys, st, sks, igpu = setup(kind, p, msg=MSG, carry=CARRY)
    w = p.big_n + 1
    rng = np.random.default_rng(601)
    for V in (1, 2, 5):
        words = rng.integers(0, 1 << 63, size=(V, L, w), dtype=U64) * U64(2) + U64(1)
        want = words.sum(axis=0, dtype=U64)
        for alias in (False, True):
            vec = igpu.CudaUnsignedRadixCiphertext.from_blocks(words, st)
            vec.set_degrees(MSG - 1)
            out = igpu.CudaUnsignedRadixCiphertext(vec.d_blocks, 1, L, p.big_n) if alias else None
            out, pbs = sks.unchecked_partial_sum_ciphertexts(vec, st, out=out, return_pbs_count=True)
            assert pbs == 0, (V, pbs)
            after = vec.to_blocks(st)
            got = after[0] if alias else out.to_blocks(st)[0]
            assert np.array_equal(got, want), (V, alias)
            assert np.array_equal(after[1:], words[1:]) and (alias or np.array_equal(after[0], words[0])), "inputs touched"
            assert list(out.degrees) == [V * (MSG - 1)] * L and list(out._info[1]) == [V] * L


def all_top(V, m):
    return [[m - 1] * L for _ in range(V)]


@pytest.mark.parametrize("V", [6, 11])
@pytest.mark.parametrize("kind,base", ANCHOR)
def test_sums_that_reduce_their_columns(kind, base, V):
    """All digits msg - 1: every group of five reaches msg * carry - 1.  Without `reduce` a column stops at what a block
    holds, with it at what one carry propagation accepts; the carries out of the last column are dropped."""
    c, m = Ctx(kind, base), base.msg
    rows = all_top(V, m)
    total = sum(rm.value(r, m) for r in rows) % m ** L
    for reduce in (False, True):
        vec = c.enc(rows, 610 + V)
        before = c.words(vec)
        out, pbs = c.sks.unchecked_partial_sum_ciphertexts(vec, c.st, reduce=reduce, return_pbs_count=True)
        digits, degrees = c.dec(out)[0], list(out.degrees)
        print(f"V={V} reduce={reduce}: {pbs} bootstraps, digits {digits}, degrees {degrees}")
        assert pbs > 0
        assert np.array_equal(c.words(vec), before), "the vector was touched"
        assert rm.value(digits, m) % m ** L == total
        limit = 2 * m - 2 if reduce else m * base.carry - 1
        assert all(d <= g <= limit for d, g in zip(digits, degrees)), (digits, degrees)
        assert all(1 <= n <= (m * base.carry - 1) // (m - 1) for n in out._info[1])
        if reduce:
            c.sks.propagate_single_carry_assign(out, c.st)
            assert c.dec(out) == [rm.digits(total, L, m)]
    # the list form: gathers the integers, sums, propagates
    clean = c.sks.sum_ciphertexts([c.enc([r], 630 + i) for i, r in enumerate(rows)], c.st)
    assert c.dec(clean) == [rm.digits(total, L, m)] and list(clean.degrees) == [m - 1] * L
    # the output in the first integer of the vector
    vec = c.enc(rows, 640 + V)
    view = c.igpu.CudaUnsignedRadixCiphertext(vec.d_blocks, 1, L, vec.lwe_dimension)
    c.sks.unchecked_partial_sum_ciphertexts(vec, c.st, out=view)
    assert rm.value(c.dec(vec)[0], m) % m ** L == total


@pytest.mark.parametrize("kind,base", ANCHOR)
def test_sum_of_sixteen_bits_is_their_count_and_blocks_of_degree_zero_cost_no_term(kind, base):
    """16 integers whose block 0 holds a bit (degree 1) or is declared empty (degree 0), blocks 1 and 2 empty.  The empty
    blocks hold the digit 3 all the same: a term made of one would show in the sum."""
    c, m, V = Ctx(kind, base), base.msg, 16
    bits = [1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1]
    empty = [3, 7, 12]
    rows = [[3 if v in empty else bits[v], 3, 3] for v in range(V)]
    count = sum(b for v, b in enumerate(bits) if v not in empty)
    vec = c.enc(rows, 650)
    vec.degrees[:] = [0 if (j or v in empty) else 1 for v in range(V) for j in range(L)]
    out, pbs = c.sks.unchecked_partial_sum_ciphertexts(vec, c.st, reduce=True, return_pbs_count=True)
    full = c.enc(rows, 650)
    full.degrees[:] = [0 if j else 1 for v in range(V) for j in range(L)]
    _, pbs_full = c.sks.unchecked_partial_sum_ciphertexts(full, c.st, reduce=True, return_pbs_count=True)
    print("bootstraps", pbs, "with the three empty blocks counted as bits", pbs_full)
    assert pbs <= pbs_full
    assert all(d <= g <= 2 * m - 2 for d, g in zip(c.dec(out)[0], out.degrees))
    c.sks.propagate_single_carry_assign(out, c.st)
    assert c.dec(out) == [rm.digits(count, L, m)]


# ================================================================================== refusals
PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
N, n = 256, 4
BK = ffi.CudaLweBootstrapKeyParamsFFI(n, 1, N, 8, 2, N, 1, 0)
KK = ffi.CudaLweKeyswitchKeyParamsFFI(N, n, 4, 3)
keys = (C.c_void_p * 1)(gpu.CudaVec(16, st).ptr)
mem = C.c_void_p()
lib.hip_scratch_partial_sum_ciphertexts_vec_64_async(s, C.byref(mem), BK, KK, 3, 6, 4, 4, False, True, 0)
def radix(V, L=3, degree=3, dim=N, noise=1):
    ct = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec(V * L * (dim + 1), st), V, L, dim)
    ct.set_degrees(degree)
    ct._info[1][:] = noise
    return ct
def call(vec, out):
    a, b = out._ffi(), vec._ffi()
    lib.hip_partial_sum_ciphertexts_vec_64_async(s, C.byref(a), C.byref(b), mem, keys, keys)
"""

REFUSALS = {
    "a degree a block cannot hold": ("call(radix(3, degree=16), radix(1))", "has degree 16"),
    "a term above nominal noise": ("call(radix(3, noise=2), radix(1))", "has noise level 2"),
    "more integers than the scratch was created for": ("call(radix(7), radix(1))", "exceed max_num_radix_in_vec 6"),
    "blocks of another lwe dimension": ("call(radix(3, dim=128), radix(1, dim=128))", "lwe dimensions should be 256"),
    "an output with too few blocks": ("call(radix(3), radix(1, L=2))", "output does not have enough blocks"),
    "a vector that is no whole number of integers": ("call(radix(1, L=4), radix(1))", "should be a multiple of"),
}


def test_the_call_the_refusals_vary_is_accepted():
    ok = run_child(PRELUDE + "call(radix(3), radix(1))\nst.synchronize()\nprint('accepted')")
    assert ok.returncode == 0 and "accepted" in ok.stdout, ok.stderr[-600:]


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_sum_misuse_aborts_with_a_message_naming_the_entry_point(name):
    snippet, message = REFUSALS[name]
    r = run_child(PRELUDE + textwrap.dedent(snippet))
    assert r.returncode != 0, f"{name}: the call was accepted"
    assert message in r.stderr and "partial_sum_ciphertexts_vec" in r.stderr, r.stderr[-600:]
