"""The programmable bootstrap over the 128-bit torus and noise squashing: tables, the f128 transform against the
reference's own two tests, the u128 decomposer, the bootstrap against an exact restatement (in phase), the full-size
bootstrap, batches / streams / graphs, noise squashing of a radix ciphertext, refusals and the ABI.

[emu] runs the kernel sources on the host, [hip] on the MI355X.  The restatement is tests/pbs128_helper.py (plain
Python integers).  Measured figures are printed before every assertion on them (run with -s to see them)."""
import ctypes as C
import decimal
import math
import os
import statistics
import time

import numpy as np
import pytest

from . import pbs128_helper as h
from .common import C1, TOY_2048, make_keys
from .harness import use_backend
from .test_error_behaviour import run as run_child

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
U64 = np.uint64
SIZES = (256, 512, 1024, 2048, 4096)
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))


def setup(kind):
    from tfhe_rs_amd import core_crypto_gpu as gpu
    lib = use_backend(kind)
    return lib, gpu, gpu.CudaStreams([0])


def upload_key(gpu, st, p, keys):
    return gpu.CudaLweBootstrapKey128.from_lwe_bootstrap_key(keys.bsk, p.n, p.k, p.N, p.base_log, p.level, st,
                                                             ms_noise_reduction=bool(p.ms_type))


def run_pbs(gpu, st, p, bsk, lwes, lut):
    """lwes [B][n + 1] u64, lut (k + 1) N integers -> [B][k N + 1][2] u64"""
    d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(lwes, st)
    d_out = gpu.CudaLweCiphertextList.new(p.k * p.N, len(lwes), st, elem_words=2)
    d_lut = gpu.CudaGlweCiphertextList.from_glwe_ciphertext_list(h.to_pairs(lut), p.k, p.N, st, elem_words=2)
    gpu.cuda_programmable_bootstrap_128_lwe_ciphertext(d_in, d_out, d_lut, bsk, st)
    return d_out.to_lwe_ciphertext_list(st)


def nontrivial(m):
    return (3 * m + 5) % 16


# ------------------------------------------------------------------------------------------------ 1. tables
PI80 = decimal.Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")


def _dec_sincos(m, M):
    """(cos, sin)(pi m / M) to well over 60 digits: exact octant reduction, then the Taylor series"""
    m %= 2 * M
    if m % (M // 2 if M >= 2 else 1) == 0 and M >= 2:   # a multiple of pi / 2: exact
        q = m // (M // 2)
        return [(1, 0), (0, 1), (-1, 0), (0, -1)][q]
    x = PI80 * m / M
    x2 = x * x
    c = s = decimal.Decimal(0)
    tc, ts = decimal.Decimal(1), x
    for k in range(1, 60):
        c += tc
        s += ts
        tc = -tc * x2 / ((2 * k - 1) * (2 * k))
        ts = -ts * x2 / ((2 * k) * (2 * k + 1))
    return c, s


def _bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def test_twiddle_tables_are_double_double_accurate():
    """Every twiddle (hi + lo) of the host-built tables is within 2^-104 relative of the true cosine / sine (decimal, 80
    digits of pi, sums carried at 90 digits); exact zeros and ones are exact."""
    lib = use_backend("emu")   # a host function: no device involved
    decimal.getcontext().prec = 90
    bound = decimal.Decimal(2) ** -104
    worst = decimal.Decimal(0)
    for N in SIZES:
        n = N // 2
        fwd, inv, untw = (np.zeros(2 * N) for _ in range(3))
        lib.hip_test_fft128_tables_host(N, *[a.ctypes.data_as(C.c_void_p) for a in (fwd, inv, untw)])
        want = {}
        D = n.bit_length() - 1
        for d in range(D):
            for g in range(1 << d):
                want[("fwd", (1 << d) + g)] = _dec_sincos(1 + 4 * _bitrev(g, d), 1 << (d + 2))
        half = 1
        while half < n:
            for j in range(half):
                want[("inv", half + j)] = _dec_sincos(-j, half) if half > 1 else (1, 0)
            half *= 2
        for j in range(n):
            c, s = _dec_sincos(-j, N)
            want[("untw", j)] = (decimal.Decimal(c) / n, decimal.Decimal(s) / n)
        tabs = {"fwd": fwd, "inv": inv, "untw": untw}
        for (name, idx), (c, s) in want.items():
            t = tabs[name][4 * idx:4 * idx + 4]
            for true, hi, lo in ((c, t[0], t[1]), (s, t[2], t[3])):
                true = decimal.Decimal(true)
                got = decimal.Decimal(float(hi)) + decimal.Decimal(float(lo))
                if true == 0:
                    assert got == 0, (N, name, idx)
                    continue
                rel = abs(got - true) / abs(true)
                worst = max(worst, rel)
                assert rel <= bound, (N, name, idx, float(rel))
    print(f"worst relative twiddle error 2^{math.log2(float(worst)):.1f}")


# ------------------------------------------------------------------------------------------------ 2. transform
def _uniform_u128(rng, count):
    return rng.integers(0, 1 << 64, size=(count, 2), dtype=U64)


@pytest.mark.parametrize("kind", BACKENDS)
def test_transform_round_trip(kind):
    """fft128/math/fft/tests.rs (roundtrip): forward as torus then backward returns every coefficient of a uniform u128
    polynomial to within 2^28."""
    lib, gpu, st = setup(kind)
    rng = np.random.default_rng(128)
    for N in SIZES:
        poly = _uniform_u128(rng, 2 * N).reshape(2, N, 2)
        planes = gpu.cuda_fourier_transform_forward_as_torus_f128(poly, N, 2, st)
        back = gpu.cuda_fourier_transform_backward_as_torus_f128(*planes, N, 2, st)
        dist = max(h.torus_distance128(a, b) for a, b in zip(h.from_pairs(poly), h.from_pairs(back)))
        print(f"N = {N}: round trip max distance 2^{math.log2(max(dist, 1)):.1f}")
        assert dist <= 1 << 28, (N, dist)


def _cmul(lib, gpu, st, a_planes, b_planes):
    count = a_planes[0].size
    da = gpu.CudaVec.from_cpu_async(np.concatenate([p.reshape(-1) for p in a_planes]), st)
    db = gpu.CudaVec.from_cpu_async(np.concatenate([p.reshape(-1) for p in b_planes]), st)
    do = gpu.CudaVec(4 * count, st, dtype=np.float64)
    lib.hip_test_f128_cmul_async(st.ptr[0], 0, do.ptr, da.ptr, db.ptr, count)
    return list(do.copy_to_cpu(st).reshape(4, 1, count))


@pytest.mark.parametrize("kind", BACKENDS)
def test_transform_product(kind):
    """fft128/math/fft/tests.rs (product): a uniform u128 polynomial (as torus) times a polynomial of 16-bit integers
    (as integer), multiplied pointwise in the Fourier domain, comes back within 2^(28 + 16 + log2 N) of the exact
    negacyclic convolution (tests/pbs128_helper.py).  The pointwise complex multiply goes through the test hook
    hip_test_f128_cmul_async, i.e. the kernels' own f128 multiply (the one the external product uses)."""
    lib, gpu, st = setup(kind)
    rng = np.random.default_rng(129)
    for N in SIZES:
        a = _uniform_u128(rng, N).reshape(1, N, 2)
        b_small = rng.integers(0, 1 << 16, size=N, dtype=U64)
        b = np.stack([b_small, np.zeros(N, dtype=U64)], axis=-1).reshape(1, N, 2)
        fa = gpu.cuda_fourier_transform_forward_as_torus_f128(a, N, 1, st)
        fb = gpu.cuda_fourier_transform_forward_as_integer_f128(b, N, 1, st)
        prod = _cmul(lib, gpu, st, fa, fb)
        got = h.from_pairs(gpu.cuda_fourier_transform_backward_as_torus_f128(*prod, N, 1, st))
        want = h.negacyclic_product_exact(h.from_pairs(a), [int(v) for v in b_small], N)
        dist = max(h.torus_distance128(x, y) for x, y in zip(got, want))
        bound = 1 << (28 + 16 + N.bit_length() - 1)
        print(f"N = {N}: product max distance 2^{math.log2(max(dist, 1)):.1f} (bound 2^{math.log2(bound):.0f})")
        assert dist <= bound, (N, dist)


# ------------------------------------------------------------------------------------------------ 3. decomposition
@pytest.mark.parametrize("kind", BACKENDS)
def test_u128_decomposer_word_for_word(kind):
    """The digits of the kernels' u128 decomposer equal the restatement's on 0, 2^127, all ones, values exactly half way
    between two representables and one either side, representables and uniform words; (24, 3) and two toy pairs, and a
    pair that represents all 128 bits.  Then the widths the bootstrap rows of test_pbs128_dispatch_coverage.py use and
    the ends of the documented range: base_log 32 and 33 (the first digits wider than an int32), 43 and 53 (around a
    double's mantissa), 64 with one and two levels (digits of magnitude 2^63), and 128 levels of one bit / 64 of two."""
    lib, gpu, st = setup(kind)
    rng = np.random.default_rng(130)
    for base_log, level in ((24, 3), (20, 4), (12, 5), (16, 8),
                            (32, 4), (64, 2), (64, 1), (43, 2), (53, 2), (33, 3), (1, 128), (2, 64)):
        bits = base_log * level
        vals = [0, 1 << 127, h.M128] + h.from_pairs(_uniform_u128(rng, 64))
        vals += [(1 << 127) + 1, (1 << 127) - 1, 1 << 63, (1 << 64) - 1, 1 << 64]
        if bits < 128:
            r = [int(v) << (128 - bits) for v in rng.integers(0, 1 << 62, size=32)]
            r = [v & h.M128 for v in r] + [((1 << bits) - 1) << (128 - bits), ((1 << (bits - 1)) - 1) << (128 - bits)]
            half = 1 << (127 - bits)
            for v in r:
                vals += [v, (v + half) & h.M128, (v + half - 1) & h.M128, (v + half + 1) & h.M128]
        d_in = gpu.CudaVec.from_cpu_async(h.to_pairs(vals), st, elem_words=2)
        d_out = gpu.CudaVec(len(vals) * level, st, elem_words=2)
        lib.hip_test_decompose_128_async(st.ptr[0], 0, d_in.ptr, d_out.ptr, len(vals), base_log, level)
        got = h.from_pairs(d_out.copy_to_cpu(st))
        got = [g - (1 << 128) if g >> 127 else g for g in got]
        want = [d for v in vals for d in h.decompose128(v, base_log, level)]
        assert got == want, (base_log, level)
        for v in vals[:8] + vals[-8:]:   # and the digits recompose to the closest representable
            if bits < 128:
                closest = ((v + (1 << (127 - bits))) >> (128 - bits) << (128 - bits)) & h.M128
                assert h.recompose128(h.decompose128(v, base_log, level), base_log, level) == closest


def test_exact_checker_packs_digits_of_magnitude_two_to_the_63():
    """base_log 64 gives digits in [-2^63, 2^63]: +2^63 is no int64 (packing through one raised OverflowError: Python
    int too large to convert to C long).  A polynomial holding +2^63, -2^63, 0, +-1, 2^63 - 1 and uniform digits of that
    range goes through ExactKey.pack_digits, one product with a key polynomial and unpack_negacyclic, and equals
    negacyclic_product_exact on the same operands; the same for a (24, 3) key, whose slot width differs."""
    rng = np.random.default_rng(131)
    for base_log, level in ((64, 1), (64, 2), (24, 3)):
        p = h.Params128(f"pack_b{base_log}l{level}", 2, 1, 256, base_log, level)
        keys = h.make_keys128(p)
        ekey = h.ExactKey(p, keys)
        top = 1 << (base_log - 1)
        digits = [top, -top, 0, 1, -1, top - 1, -(top - 1)]
        digits += [int(v) - top for v in rng.integers(0, 1 << base_log, size=p.N - len(digits) - 2, dtype=U64)]
        digits += [-top, top]   # the last coefficients wrap negacyclically
        assert len(digits) == p.N
        for i, idx, row, col in ((0, 0, 0, 0), (1, level - 1, 1, 1)):
            got = ekey.unpack_negacyclic(ekey.pack_digits(digits) * ekey.op(i, idx, row, col))
            want = h.negacyclic_product_exact(h.from_pairs(keys.bsk[i, idx, row, col]), digits, p.N)
            assert got == want, (base_log, level, i, idx, row, col)


# ------------------------------------------------------------------------------------------------ 4. phase
_exact_cache = {}


def _phase_case(p):
    """8 inputs under the identity table (messages 0 .. 7) and 8 under a non-trivial one (messages 8 .. 15): the 16
    messages between them; the exact bootstrap's output phases, computed once per session"""
    if p.name not in _exact_cache:
        keys = h.make_keys128(p)
        lwes = h.encrypt_inputs(p, keys, range(16), seed=41)
        luts = [h.make_lut128(p, lambda m: m), h.make_lut128(p, nontrivial)]
        t0 = time.time()
        phases = h.exact_phases(p, lwes, [luts[i // 8] for i in range(16)])
        print(f"{p.name}: exact restatement of 16 bootstraps took {time.time() - t0:.0f} s")
        _exact_cache[p.name] = (keys, lwes, luts, phases)
    return _exact_cache[p.name]


def phase_bound(p):
    """The reference's product threshold summed without cancellation over a bootstrap:
    n (k + 1) l (k N + 1) 2^(28 + base_log + log2 N)"""
    return p.n * (p.k + 1) * p.level * (p.k * p.N + 1) * (1 << (28 + p.base_log + p.N.bit_length() - 1))


def _check_phases(kind, p):
    lib, gpu, st = setup(kind)
    keys, lwes, luts, want = _phase_case(p)
    bsk = upload_key(gpu, st, p, keys)
    got = np.concatenate([run_pbs(gpu, st, p, bsk, lwes[:8], luts[0]), run_pbs(gpu, st, p, bsk, lwes[8:], luts[1])])
    dists = [h.torus_distance128(h.phase128(p, keys, got[i]), want[i]) for i in range(16)]
    G = phase_bound(p)
    print(f"{p.name} [{kind}]: phase distance to the exact bootstrap: max 2^{math.log2(max(max(dists), 1)):.1f}, "
          f"median 2^{math.log2(max(statistics.median(dists), 1)):.1f}, bound 2^{math.log2(G):.1f}")
    for i in range(16):   # and the phases decode to the table's values
        f = (lambda m: m) if i < 8 else nontrivial
        assert h.decode128(want[i]) == f(i), i
    assert max(dists) <= G, (p.name, dists)


@pytest.mark.parametrize("p", h.TOYS, ids=[p.name for p in h.TOYS])
@pytest.mark.parametrize("kind", BACKENDS)
def test_bootstrap_phase_against_exact_products_toy_rings(kind, p):
    """Toy rings (N = 256 and 512, k = 1 and 2, two decompositions, both modulus switches), n = 16: the phase of every
    output under the output key is within G of the phase the exact restatement reaches."""
    _check_phases(kind, p)


@pytest.mark.slow
@pytest.mark.parametrize("kind", BACKENDS)
def test_bootstrap_phase_against_exact_products_production_ring(kind):
    """The production ring (k = 2, N = 2048, 3 levels of 24 bits, centred switch) with n = 32: G is about 2^83.  The
    exact restatement of the 16 bootstraps is most of this test's time (minutes of big-integer products)."""
    _check_phases(kind, h.PRODUCTION_N32)


# ------------------------------------------------------------------------------------------------ 5. full size
def _full_size_outputs(kind, keys, lwes, lut):
    lib, gpu, st = setup(kind)
    p = h.PRODUCTION
    bsk = upload_key(gpu, st, p, keys)
    t0 = time.time()
    first = run_pbs(gpu, st, p, bsk, lwes, lut)
    took = time.time() - t0
    second = run_pbs(gpu, st, p, bsk, lwes, lut)
    print(f"[{kind}] 16 full-size bootstraps (n = 918): {took:.1f} s")
    assert np.array_equal(first, second), "two calls on the same inputs differ"
    return first


@pytest.mark.slow
@pytest.mark.parametrize("kind", BACKENDS)
def test_full_size_bootstrap_with_squashing_parameters(kind):
    """The reference's test_bootstrap_u128_with_squashing: n = 918 (the 2_2 set's small key), the production squashing
    set, messages 0 .. 15 on u64 with TUniform(46) noise, identity table; every message comes back under the 5-bit
    rounding; two calls give identical words; on hip the same inputs also run on the host emulation and the two builds
    agree word for word.  Slow: the key is 812 MB and its generation plus the emulation's 16 bootstraps take minutes."""
    p = h.PRODUCTION
    keys = h.make_keys128(p, compute=C1)
    lwes = h.encrypt_inputs(p, keys, range(16), seed=43)
    lut = h.make_lut128(p, lambda m: m)
    out = _full_size_outputs(kind, keys, lwes, lut)
    assert [h.decode128(h.phase128(p, keys, o)) for o in out] == list(range(16))
    if kind == "hip":
        emu = _full_size_outputs("emu", keys, lwes, lut)
        use_backend("hip")
        differing = int((emu != out).any(axis=(1, 2)).sum())
        print(f"hip vs emu: {differing} of 16 ciphertexts differ")
        assert np.array_equal(emu, out)


# ------------------------------------------------------------------------------------------------ 6. batches, streams
BATCH_SET = h.TOYS[3]   # k = 2, N = 512, (24, 3), centred switch


@pytest.mark.parametrize("kind", BACKENDS)
def test_batches_give_the_same_output_per_input(kind):
    lib, gpu, st = setup(kind)
    p = BATCH_SET
    keys = h.make_keys128(p)
    bsk = upload_key(gpu, st, p, keys)
    lwes = h.encrypt_inputs(p, keys, range(16), seed=44)
    lut = h.make_lut128(p, nontrivial)
    ref = run_pbs(gpu, st, p, bsk, lwes, lut)
    assert [h.decode128(h.phase128(p, keys, o)) for o in ref] == [nontrivial(m) for m in range(16)]
    for B in ((1, 2, 257, 1024) if kind == "hip" else (1, 2, 33)):
        pick = np.arange(B) % 16 if B > 2 else np.arange(B) + 5
        out = run_pbs(gpu, st, p, bsk, lwes[pick], lut)
        assert np.array_equal(out, ref[pick]), B


BIG_RING = h.Params128("toy128_k1_N4096", 8, 1, 4096, 24, 3, ms_type=1)


@pytest.mark.parametrize("kind", BACKENDS)
def test_bootstrap_with_the_accumulator_in_device_memory(kind):
    """N = 4096: accumulator and transform buffer exceed the LDS of a CU, so the accumulator is a per-sample buffer of the
    scratch that only its own workgroup touches.  Checked by decryption (both tables, all 16 messages), by two calls
    giving identical words, and with more samples than one (every workgroup on its own slice)."""
    lib, gpu, st = setup(kind)
    p = BIG_RING
    keys = h.make_keys128(p)
    bsk = upload_key(gpu, st, p, keys)
    lwes = h.encrypt_inputs(p, keys, range(16), seed=46)
    for f in (lambda m: m, nontrivial):
        lut = h.make_lut128(p, f)
        out = run_pbs(gpu, st, p, bsk, lwes, lut)
        assert [h.decode128(h.phase128(p, keys, o)) for o in out] == [f(m) for m in range(16)]
        assert np.array_equal(run_pbs(gpu, st, p, bsk, lwes, lut), out)
        assert np.array_equal(run_pbs(gpu, st, p, bsk, lwes[3:4], lut), out[3:4])


def test_bench_tool_runs_end_to_end_on_the_host_emulation():
    """tools/bench_pbs128.py with a two-bit key and one batch, against the emulation library: every call the tool makes
    (both key conversions, scratch / bootstrap / cleanup, the squashing triple) goes through with its real argument list
    and the JSON line comes out.  The figures mean nothing here."""
    import json
    import subprocess
    import sys
    from .harness import EMU_LIB, build_emu
    build_emu()
    env = dict(os.environ, TFHE_HIP_BACKEND_LIB=EMU_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_pbs128.py"), "--n", "2", "--batches", "1,3",
                        "--window", "0.01"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out["bootstrap"]) == {"1", "3"} and out["squash_fheuint64"]["output_blocks"] == 16
    assert out["key_conversion_s"] > 0 and all(v["ms"] > 0 for v in out["bootstrap"].values())


class _Job:
    """buffers and scratch of one launch on its own stream; enqueue() is exactly one _async call"""

    def __init__(self, lib, gpu, p, bsk, lwes, lut):
        self.lib, self.p, self.B, self.bsk = lib, p, len(lwes), bsk
        self.st = gpu.CudaStreams([0])
        self.d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(lwes, self.st)
        self.d_out = gpu.CudaLweCiphertextList.new(p.k * p.N, self.B, self.st, elem_words=2)
        self.d_lut = gpu.CudaGlweCiphertextList.from_glwe_ciphertext_list(h.to_pairs(lut), p.k, p.N, self.st, elem_words=2)
        self.buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(self.st.ptr[0], 0, C.byref(self.buf), p.n, p.k, p.N, p.level, self.B,
                                                         True, p.ms_type)
        self.st.synchronize()

    def enqueue(self):
        p = self.p
        self.lib.hip_programmable_bootstrap_128_async(self.st.ptr[0], 0, self.d_out.d_vec.ptr, self.d_lut.d_vec.ptr,
                                                      self.d_in.d_vec.ptr, self.bsk.d_vec.ptr, self.buf, p.n, p.k, p.N,
                                                      p.base_log, p.level, self.B)

    def clear_output(self):
        self.lib.cuda_memset_async(self.d_out.d_vec.ptr, 0, self.B * (self.p.k * self.p.N + 1) * 16, self.st.ptr[0], 0)

    def result(self):
        return self.d_out.to_lwe_ciphertext_list(self.st)

    def close(self):
        self.lib.hip_cleanup_programmable_bootstrap_128(self.st.ptr[0], 0, C.byref(self.buf))


def _stream_case(gpu, st):
    p = BATCH_SET
    keys = h.make_keys128(p)
    bsk = upload_key(gpu, st, p, keys)
    lwes = h.encrypt_inputs(p, keys, range(16), seed=45)
    return p, keys, bsk, lwes, h.make_lut128(p, nontrivial)


@pytest.mark.gpu
def test_two_streams_running_concurrently_give_the_outputs_of_one():
    lib, gpu, st = setup("hip")
    p, keys, bsk, lwes, lut = _stream_case(gpu, st)
    big = lwes[np.arange(300) % 16]
    ref = run_pbs(gpu, st, p, bsk, big, lut)
    jobs = [_Job(lib, gpu, p, bsk, big, lut) for _ in range(2)]
    try:
        for _ in range(3):
            for j in jobs:
                j.enqueue()
        for j in jobs:
            assert np.array_equal(j.result(), ref)
    finally:
        for j in jobs:
            j.close()


@pytest.mark.gpu
def test_a_launch_is_captured_into_a_hip_graph_and_replayed():
    from .test_streams_and_graphs import Hip
    lib, gpu, st = setup("hip")
    p, keys, bsk, lwes, lut = _stream_case(gpu, st)
    job = _Job(lib, gpu, p, bsk, lwes, lut)
    hip = Hip()
    try:
        job.enqueue()
        direct = job.result()
        assert [h.decode128(h.phase128(p, keys, o)) for o in direct] == [nontrivial(m) for m in range(16)]
        graph, exe = hip.capture(job.st.ptr[0], job.enqueue)
        for _ in range(2):
            job.clear_output()
            hip.launch(exe, job.st.ptr[0])
            assert np.array_equal(job.result(), direct)
        hip.destroy(graph, exe)
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ 7. noise squashing
TOY_SQUASH = h.Params128("toy128_squash_k1_N512", TOY_2048.n, 1, 512, 24, 3, ms_type=1)


@pytest.mark.parametrize("kind", [pytest.param("emu", id="emu"),
                                  pytest.param("hip", id="hip", marks=[pytest.mark.gpu, pytest.mark.slow])])
def test_noise_squashing_of_a_radix_ciphertext(kind):
    """A 64-bit radix value (32 blocks of 2_2; hip: the compute set PARAM_MESSAGE_2_CARRY_2 and the production squashing
    set, emu: toy sets) becomes 16 u128 blocks, block i decrypting to lo + 4 hi of its pair; 5 blocks become 3; the input
    is unchanged.  Slow on hip only (the 812 MB key of the full-size test, shared with it)."""
    _squash_and_check(kind, lambda cp: h.PRODUCTION if kind == "hip" else TOY_SQUASH,
                      ((32, 0xD1CEB00C5EEDF00D), (5, 0b1110010011)))


@pytest.mark.gpu
def test_noise_squashing_on_the_device_with_a_toy_squashing_ring():
    """The device's compute set (PARAM_MESSAGE_2_CARRY_2: its keyswitch and its small key, n = 918) with a toy squashing
    ring (k = 1, N = 512, 3 levels of 24 bits, centred switch; a key of about 90 MB instead of 812 MB): 5 blocks become
    3, block i decrypting to lo + 4 hi of its pair, the input unchanged.  The assertions of the test above, without the
    production squashing key and therefore not slow."""
    _squash_and_check("hip", lambda cp: h.Params128(f"toy128_squash_k1_N512_n{cp.n}", cp.n, 1, 512, 24, 3, ms_type=1),
                      ((5, 0b1110010011),))


def _squash_and_check(kind, squashing_set, cases):
    """squashing_set(compute set) -> the Params128 of the squashing key; cases: (blocks, value) pairs"""
    from tfhe_rs_amd import integer_gpu as igpu
    from .test_radix_integer import encrypt_radix
    from .test_radix_integer import setup as radix_setup
    cp, ckeys, st, sks, _ = radix_setup(kind)
    gpu = __import__("tfhe_rs_amd.core_crypto_gpu", fromlist=["x"])
    sp = squashing_set(cp)
    skeys = h.make_keys128(sp, compute=cp)
    nsk = igpu.CudaNoiseSquashingKey(upload_key(gpu, st, sp, skeys), 4, 4)
    for blocks, value in cases:
        h_in = encrypt_radix(cp, ckeys, [value], blocks, seed=70 + blocks)
        ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(h_in, st)
        ct.set_degrees(3)
        out = igpu.squash_radix_ciphertext_noise(nsk, sks, ct, st)
        assert out.num_blocks == (blocks + 1) // 2
        digits = [(value >> (2 * j)) & 3 for j in range(blocks)] + [0]
        want = [digits[2 * i] + 4 * digits[2 * i + 1] for i in range(out.num_blocks)]
        got = [h.decode128(h.phase128(sp, skeys, b)) for b in out.to_blocks(st)]
        assert got == want, blocks
        assert np.array_equal(ct.to_blocks(st), h_in), "the input ciphertext changed"


# ------------------------------------------------------------------------------------------------ 8. refusals
REFUSALS = {
    "polynomial size below the range": ("""
        buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(S, G, C.byref(buf), 10, 1, 128, 3, 4, True, 0)
        """, "polynomial_size 128 not supported by the 128-bit PBS"),
    "polynomial size above the range": ("""
        buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(S, G, C.byref(buf), 10, 1, 8192, 3, 4, True, 0)
        """, "polynomial_size 8192 not supported by the 128-bit PBS"),
    "transform of an unsupported size": ("""
        v = gpu.CudaVec(4 * 8192, st)
        lib.hip_fourier_transform_forward_as_torus_f128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, 8192, 1)
        """, "polynomial_size 8192 not supported by the 128-bit PBS"),
    "key conversion of an unsupported size": ("""
        v = gpu.CudaVec(4 * 128, st)
        src = np.zeros(4 * 128 * 2, dtype=np.uint64)
        lib.hip_convert_lwe_programmable_bootstrap_key_128_async(S, G, v.ptr, src.ctypes.data_as(C.c_void_p), 1, 1, 1, 128)
        """, "polynomial_size 128 not supported by the 128-bit PBS"),
    "decomposition wider than the torus": ("""
        buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(S, G, C.byref(buf), 10, 1, 256, 5, 4, True, 0)
        v = gpu.CudaVec(4 * 600 * 2, st)
        lib.hip_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, buf, 10, 1, 256, 26, 5, 4)
        """, "invalid decomposition (base_log=26, level=5)"),
    "null scratch": ("""
        v = gpu.CudaVec(4 * 600 * 2, st)
        lib.hip_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, None, 10, 1, 256, 24, 3, 4)
        """, "PBS buffer was not created by hip_scratch_programmable_bootstrap_128_async"),
    "scratch of the 64-bit bootstrap": ("""
        buf = C.c_void_p()
        lib.scratch_cuda_programmable_bootstrap_64_async(S, G, C.byref(buf), 10, 1, 256, 3, 4, True, 0)
        v = gpu.CudaVec(4 * 600 * 2, st)
        lib.hip_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, buf, 10, 1, 256, 24, 3, 4)
        """, "PBS buffer was not created by hip_scratch_programmable_bootstrap_128_async"),
    "launch does not match its scratch": ("""
        buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(S, G, C.byref(buf), 10, 1, 256, 3, 4, True, 0)
        v = gpu.CudaVec(4 * 600 * 2, st)
        lib.hip_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, buf, 10, 1, 512, 24, 3, 4)
        """, "PBS buffer parameters do not match"),
    "a key converted for other sizes": ("""
        src = np.zeros((4, 3, 2, 2, 256, 2), dtype=np.uint64)
        bsk = gpu.CudaLweBootstrapKey128.from_lwe_bootstrap_key(src, 4, 1, 256, 24, 3, st)
        buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(S, G, C.byref(buf), 2, 1, 512, 3, 4, True, 0)
        v = gpu.CudaVec(4 * 600 * 2, st)
        lib.hip_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, bsk.d_vec.ptr, buf, 2, 1, 512, 24, 3, 4)
        """, "the bootstrap key was converted for other sizes (n=4, k=1, level=3, N=256)"),
    "squashing into another number of blocks than half the input's": ("""
        from tfhe_rs_amd import integer_gpu as igpu
        s, keep = igpu.CudaServerKey._streams(st)
        mem = C.c_void_p()
        lib.hip_scratch_integer_apply_noise_squashing_64_async(s, C.byref(mem), 10, 1, 256, 1, 2048, 4, 4, 3, 24, 2, 5, 4, 4,
                                                               True, 0)
        """, "should be half ceil the number input radix blocks"),
    "squashing: output ciphertext of the wrong block count": ("""
        from tfhe_rs_amd import integer_gpu as igpu
        s, keep = igpu.CudaServerKey._streams(st)
        mem = C.c_void_p()
        lib.hip_scratch_integer_apply_noise_squashing_64_async(s, C.byref(mem), 10, 1, 256, 1, 2048, 4, 4, 3, 24, 3, 5, 4, 4,
                                                               True, 0)
        ct = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec(5 * 2049, st), 1, 5, 2048)
        out = igpu.CudaSquashedNoiseRadixCiphertext(gpu.CudaVec(2 * 257, st, elem_words=2), 2, 256, 5)
        keys = (C.c_void_p * 1)(ct.d_blocks.ptr)
        lib.hip_integer_apply_noise_squashing_64_async(s, C.byref(out._ffi()), C.byref(ct._ffi()), mem, keys, keys)
        """, "should be half ceil the number input radix blocks"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_misuse_is_refused_with_a_message(name):
    snippet, message = REFUSALS[name]
    r = run_child(snippet)
    assert r.returncode != 0, r.stdout + r.stderr
    assert message in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ 9. ABI
REF_INCLUDE = "/root/reference/backends/tfhe-cuda-backend/cuda/include"
STANDS_FOR = {
    "hip_convert_lwe_programmable_bootstrap_key_128_async": "cuda_convert_lwe_programmable_bootstrap_key_128_async",
    "hip_scratch_programmable_bootstrap_128_async": "scratch_cuda_programmable_bootstrap_128_async",
    "hip_programmable_bootstrap_128_async": "cuda_programmable_bootstrap_128_async",
    "hip_cleanup_programmable_bootstrap_128": "cleanup_cuda_programmable_bootstrap_128",
    "hip_fourier_transform_forward_as_torus_f128_async": "cuda_fourier_transform_forward_as_torus_f128_async",
    "hip_fourier_transform_forward_as_integer_f128_async": "cuda_fourier_transform_forward_as_integer_f128_async",
    "hip_fourier_transform_backward_as_torus_f128_async": "cuda_fourier_transform_backward_as_torus_f128_async",
}


def test_every_new_symbol_is_declared_bound_and_exported_by_the_emulation_build():
    from tfhe_rs_amd import ffi
    lib = use_backend("emu")
    for name in list(STANDS_FOR) + ["hip_scratch_integer_apply_noise_squashing_64_async",
                                    "hip_integer_apply_noise_squashing_64_async",
                                    "hip_cleanup_integer_apply_noise_squashing_64", "hip_test_fft128_tables_host",
                                    "hip_test_decompose_128_async", "hip_test_f128_cmul_async"]:
        assert name in ffi.SIGNATURES and hasattr(lib, name), name


@pytest.mark.skipif(not os.path.isdir(REF_INCLUDE), reason="reference tree absent")
def test_128_bit_prototypes_equal_the_reference_prototypes_they_stand_for():
    import sys
    sys.path.insert(0, ROOT)
    from tools.c_prototypes import parse_prototypes
    ours = parse_prototypes(open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read())
    ref = {}
    for rel in ("pbs/programmable_bootstrap.h", "fft/fft128.h"):
        ref.update(parse_prototypes(open(os.path.join(REF_INCLUDE, rel)).read()))
    for mine, theirs in STANDS_FOR.items():
        assert mine in ours and theirs in ref, (mine, theirs)
        assert ours[mine] == ref[theirs], f"{mine}: {ours[mine]} != {ref[theirs]}"
