"""The multi-bit programmable bootstrap over the 128-bit torus and noise squashing on a multi-bit key: the key bundle word
for word, the bootstrap against an exact restatement (in phase), determinism and shape, chunking, ten groups on the
production ring, streams and graphs, noise squashing, refusals, the ABI and the dispatch census.

[emu] runs the kernel sources on the host, [hip] on the MI355X.  The restatement is tests/pbs128_multibit_helper.py (plain
Python integers).  Measured figures are printed before every assertion on them (run with -s to see them)."""
import ctypes as C
import dataclasses
import math
import os
import re
import statistics
import time

import numpy as np
import pytest

from . import pbs128_helper as h
from . import pbs128_multibit_helper as m
from .common import TOY_2048
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_pbs128 import BACKENDS, REF_INCLUDE, TOY_SQUASH, nontrivial, phase_bound, setup
from .test_pbs128 import upload_key as upload_classic_key
from .test_pbs128_dispatch_coverage import MESSAGES, crafted_inputs

U64 = np.uint64
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
HEADER = os.path.join(ROOT, "tfhe_rs_amd", "csrc", "pbs128_multibit.h")
SINGLE_HEADER = os.path.join(ROOT, "tfhe_rs_amd", "csrc", "pbs128.h")


def upload_key(gpu, st, p, keys):
    return gpu.CudaLweMultiBitBootstrapKey128.from_lwe_multi_bit_bootstrap_key(keys.bsk, p.n, p.k, p.N, p.base_log, p.level,
                                                                               p.g, st)


def run_mb(gpu, st, p, bsk, lwes, lut, in_idx=None, out_idx=None):
    """lwes [B'][n + 1] u64, lut (k + 1) N integers; sample s reads lwes[in_idx[s]] and writes row out_idx[s]
    -> [B][k N + 1][2] u64, B = len(in_idx)"""
    B = len(lwes) if in_idx is None else len(in_idx)
    d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(lwes, st)
    view = gpu.CudaLweCiphertextList(d_in.d_vec, B, p.n)
    d_out = gpu.CudaLweCiphertextList.new(p.k * p.N, B, st, elem_words=2)
    d_lut = gpu.CudaGlweCiphertextList.from_glwe_ciphertext_list(h.to_pairs(lut), p.k, p.N, st, elem_words=2)
    d_ii = gpu.CudaVec.from_cpu_async(np.asarray(np.arange(B) if in_idx is None else in_idx, dtype=U64), st)
    d_oi = gpu.CudaVec.from_cpu_async(np.asarray(np.arange(B) if out_idx is None else out_idx, dtype=U64), st)
    gpu.cuda_multi_bit_programmable_bootstrap_128_lwe_ciphertext(view, d_out, d_lut, d_oi, d_ii, bsk, st)
    return d_out.to_lwe_ciphertext_list(st)


# ------------------------------------------------------------------------------------------------ 1. key bundle
BUNDLE_SETS = [m.mb("bundle_g2", 8, 1, 256, 24, 3, 2), m.mb("bundle_g3", 12, 1, 256, 24, 3, 3),
               m.mb("bundle_g4", 16, 1, 256, 24, 3, 4), m.mb("bundle_N2048_k2_l1_g4", 16, 2, 2048, 24, 1, 4)]


def crafted_mask(p, rng):
    """four groups of mask words (and a body).  unit = 2^64 / 2 N is one step of the switched modulus.
    group 0: (N - 1) units, one unit, zeros: subsets of degree N - 1, 1, N and (g > 2) 0;
    group 1: (2 N - 1) units and one unit: degree 2 N - 1, and a u64 sum that WRAPS (to 0);
    group 2: 2^64 - 1 and zeros: a sum that rounds up to 2 N and wraps to 0; degree 0 from the zero words;
    group 3: uniform words."""
    unit = 1 << (64 - p.log2N2)
    pad = [0] * (p.g - 2)
    words = [(p.N - 1) * unit, unit] + pad + [(2 * p.N - 1) * unit, unit] + pad + [(1 << 64) - 1, 0] + pad
    words += [int(v) for v in rng.integers(0, 1 << 64, size=p.g, dtype=U64)]
    return np.array(words + [12345], dtype=U64)


@pytest.mark.parametrize("p", BUNDLE_SETS, ids=[p.name for p in BUNDLE_SETS])
@pytest.mark.parametrize("kind", BACKENDS)
def test_key_bundle_word_for_word(kind, p):
    """One sample's Fourier bundle of each group (test hook hip_test_pbs128_multibit_keybundle_async) equals the helper's
    exact integer bundle passed through hip_fourier_transform_forward_as_torus_f128_async: the same transform code on the
    same words, so the comparison is equality.  The key is uniform words (a bundle is a sum of rotations of whatever the
    key holds).  The crafted mask hits the subset degrees 0, N - 1, N and 2 N - 1, a u64 sum that wraps and a sum that
    rounds up to 2 N and wraps to 0."""
    lib, gpu, st = setup(kind)
    rng = np.random.default_rng(140 + p.g + p.N)
    per, polys, n2 = 1 << p.g, p.level * (p.k + 1) ** 2, p.N // 2
    key = rng.integers(0, 1 << 64, size=(p.groups, per, p.level, p.k + 1, p.k + 1, p.N, 2), dtype=U64)
    lwe = crafted_mask(p, rng)
    assert len(lwe) == p.n + 1 and p.groups == 4
    degrees, _ = m.multi_bit_modulus_switch(lwe, p.log2N2, p.g)
    hit = {d for row in degrees for d in row[1:]}
    assert {0, p.N - 1, p.N, 2 * p.N - 1} <= hit, sorted(hit)
    sums = [sum(int(lwe[grp * p.g + i]) for i in range(p.g) if (s >> (p.g - 1 - i)) & 1)
            for grp in range(p.groups) for s in range(1, per)]
    half = 1 << (63 - p.log2N2)
    assert any(v >= 1 << 64 for v in sums), "no subset sum wraps"
    assert any(v < 1 << 64 and v + half >= 1 << 64 for v in sums), "no subset sum rounds up to 2 N"

    bsk = upload_key(gpu, st, p, m.KeysMb128(p, None, None, key))
    d_lwe = gpu.CudaVec.from_cpu_async(lwe, st)
    d_zero = gpu.CudaVec.from_cpu_async(np.zeros(1, dtype=U64), st)
    d_out = gpu.CudaVec(polys * 4 * n2, st, dtype=np.float64)
    for grp in range(p.groups):
        lib.hip_test_pbs128_multibit_keybundle_async(st.ptr[0], 0, d_out.ptr, bsk.d_vec.ptr, d_lwe.ptr, d_zero.ptr, p.n, p.k,
                                                     p.N, p.level, p.g, grp)
        got = d_out.copy_to_cpu(st).reshape(polys, 4, n2)
        exact = m.exact_bundle(p, key[grp], degrees[grp]).reshape(polys, p.N, 2)
        want = gpu.cuda_fourier_transform_forward_as_torus_f128(exact, p.N, polys, st)
        for plane in range(4):
            assert np.array_equal(got[:, plane].view(U64), np.ascontiguousarray(want[plane]).view(U64)), (grp, plane)


def test_helper_modulus_switch_equals_the_oracles():
    """multi_bit_modulus_switch is a restatement of orc_multi_bit_modulus_switch: compared on uniform words and on the
    crafted masks"""
    from . import oracle as orc
    rng = np.random.default_rng(141)
    for p in BUNDLE_SETS:
        for lwe in (crafted_mask(p, rng), rng.integers(0, 1 << 64, size=p.n + 1, dtype=U64)):
            degrees, body = m.multi_bit_modulus_switch(lwe, p.log2N2, p.g)
            o_deg, o_body = orc.multi_bit_modulus_switch(lwe, p.log2N2, p.g)
            assert [d for row in degrees for d in row] == [int(v) for v in o_deg] and body == int(o_body)


# ------------------------------------------------------------------------------------------------ 2. phase
@dataclasses.dataclass(frozen=True)
class Row:
    p: m.ParamsMb128
    only_cover: tuple   # the one requirement of required_cover() that no other row is listed for

    @property
    def id(self):
        return self.p.name.replace("mb128_", "")


def _row(name, k, N, decomposition, g, n, only_cover):
    return Row(m.mb("mb128_" + name, n, k, N, *decomposition, g), only_cover)


ROWS = [
    _row("k1_N256_g2", 1, 256, (24, 3), 2, 12, ("pair", 256, 2)),
    _row("k2_N256_g3", 2, 256, (20, 4), 3, 12, ("pair", 256, 3)),
    _row("k1_N512_g4", 1, 512, (18, 4), 4, 12, ("pair", 512, 2)),
    _row("k3_N512_b33l3_g3", 3, 512, (33, 3), 3, 12, ("pair", 512, 4)),
    _row("k1_N256_b31l4_g4", 1, 256, (31, 4), 4, 12, ("last base_log on the single-double digit path",)),
    _row("k1_N256_b32l4_g4", 1, 256, (32, 4), 4, 12, ("first base_log on the double-double digit path",)),
    _row("k1_N512_b64l1_g2", 1, 512, (64, 1), 2, 12, ("level 1",)),
    _row("k1_N1024_g4", 1, 1024, (24, 3), 4, 12, ("pair", 1024, 2)),
    _row("k2_N2048_fixed_g4", 2, 2048, (18, 4), 4, 8, ("fixed", 2048, 3)),
    _row("k2_N2048_b20l4_g4", 2, 2048, (20, 4), 4, 8, ("pair", 2048, 3)),
    _row("k1_N4096_b32l4_g2", 1, 4096, (32, 4), 2, 4, ("pair", 4096, 2)),
    # the pairs of the dispatcher that the sets above leave out, at two groups each
    _row("k3_N256_g2", 3, 256, (24, 3), 2, 4, ("pair", 256, 4)),
    _row("k2_N512_g2", 2, 512, (24, 3), 2, 4, ("pair", 512, 3)),
    _row("k2_N1024_b43l2_g3", 2, 1024, (43, 2), 3, 6, ("pair", 1024, 3)),
    _row("k3_N1024_g2", 3, 1024, (24, 3), 2, 4, ("pair", 1024, 4)),
    _row("k1_N2048_b42l3_g2", 1, 2048, (42, 3), 2, 4, ("pair", 2048, 2)),
]


def mb_phase_bound(p):
    """the project's formula (test_pbs128.phase_bound) with n / g for n: one term per external product"""
    return phase_bound(dataclasses.replace(p, n=p.groups))


_cases = {}


def case_of(p):
    """keys, six inputs (four encryptions, two crafted non-encryptions), the table and the exact bootstrap's six output
    phases: computed once per session and shared by both backends and by the tests that reuse a set"""
    if p.name not in _cases:
        keys = m.make_keys_mb128(p)
        lwes = np.concatenate([h.encrypt_inputs(p, keys, MESSAGES, seed=47), crafted_inputs(p)])
        lut = h.make_lut128(p, nontrivial)
        t0 = time.time()
        want = m.exact_phases_multi_bit(p, lwes, lut)
        print(f"{p.name}: exact restatement of {len(lwes)} bootstraps took {time.time() - t0:.1f} s")
        for msg, w in zip(MESSAGES, want):   # the exact side first: a set the reference itself would miss cannot pass
            assert h.decode128(w) == nontrivial(msg), (p.name, msg)
        _cases[p.name] = (keys, lwes, lut, want)
    return _cases[p.name]


def launch_and_check(kind, p):
    lib, gpu, st = setup(kind)
    keys, lwes, lut, want = case_of(p)
    bsk = upload_key(gpu, st, p, keys)
    out = run_mb(gpu, st, p, bsk, lwes, lut)
    again = run_mb(gpu, st, p, bsk, lwes, lut)
    alone = run_mb(gpu, st, p, bsk, lwes[3:4], lut)
    assert out.shape == (len(lwes), p.k * p.N + 1, 2)
    phases = [h.phase128(p, keys, o) for o in out]
    dists = [h.torus_distance128(a, b) for a, b in zip(phases, want)]
    G = mb_phase_bound(p)
    print(f"{p.name} [{kind}]: phase distance to the exact bootstrap: max 2^{math.log2(max(max(dists), 1)):.1f}, "
          f"median 2^{math.log2(max(statistics.median(dists), 1)):.1f}, bound 2^{math.log2(G):.1f}")
    assert max(dists) <= G, (p.name, kind, dists)
    assert [h.decode128(ph) for ph in phases[:len(MESSAGES)]] == [nontrivial(v) for v in MESSAGES]
    assert np.array_equal(again, out), "two calls on the same inputs differ"
    assert np.array_equal(alone, out[3:4]), "a launch of one sample differs from its row of the batch"
    return out


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
@pytest.mark.parametrize("kind", BACKENDS)
def test_bootstrap_row(kind, row):
    """Six LWEs in one launch under a non-trivial table: every output phase within the bound of the exact restatement's,
    crafted inputs included; the encryptions decode; a second call returns identical words; a one-sample launch of input 3
    equals row 3; on the device the six rows also equal the host emulation's word for word (the check that can see a
    device-only fault)."""
    out = launch_and_check(kind, row.p)
    if kind == "hip":
        try:
            emu = launch_and_check("emu", row.p)
        finally:
            use_backend("hip")
        differing = int((emu != out).any(axis=(1, 2)).sum())
        print(f"{row.p.name}: hip vs emu: {differing} of {len(out)} ciphertexts differ")
        assert np.array_equal(emu, out)


# ------------------------------------------------------------------------------------------------ 3. shape
SHAPE_SET = ROWS[1].p   # k = 2, N = 256, (20, 4), g = 3


@pytest.mark.parametrize("kind", BACKENDS)
def test_indexes_and_batches_by_equality_of_words(kind):
    """Permuted input and output indexes permute the rows; batches of 1, 2 and 257 of repeated inputs give the rows of the
    batch of six."""
    lib, gpu, st = setup(kind)
    p = SHAPE_SET
    keys, lwes, lut, _ = case_of(p)
    bsk = upload_key(gpu, st, p, keys)
    ref = run_mb(gpu, st, p, bsk, lwes, lut)
    in_idx, out_idx = [4, 2, 0, 5, 1, 3], [1, 5, 3, 0, 2, 4]
    out = run_mb(gpu, st, p, bsk, lwes, lut, in_idx=in_idx, out_idx=out_idx)
    for s in range(6):
        assert np.array_equal(out[out_idx[s]], ref[in_idx[s]]), s
    for B in (1, 2, 257):
        pick = np.arange(B) % 6 if B > 2 else np.arange(B) + 2
        assert np.array_equal(run_mb(gpu, st, p, bsk, lwes[pick], lut), ref[pick]), B


# ------------------------------------------------------------------------------------------------ 4. chunking
CHUNK_SETS = [m.mb("mb128_chunk_k1_N256", 20, 1, 256, 24, 3, 4), m.mb("mb128_chunk_k2_N2048", 20, 2, 2048, 18, 4, 4)]


@pytest.mark.parametrize("p", CHUNK_SETS, ids=[p.name for p in CHUNK_SETS])
@pytest.mark.parametrize("kind", BACKENDS)
def test_chunk_size_does_not_change_a_word(kind, p):
    """Five groups with 1, 2, 3 and 5 groups per pass and the automatic choice: a chunk that does not divide the group
    count, a single chunk, and ACC saved and reloaded between every pair of groups.  Same words every time; they decode."""
    lib, gpu, st = setup(kind)
    keys = m.make_keys_mb128(p)
    lwes = h.encrypt_inputs(p, keys, (3, 9, 14), seed=48)
    lut = h.make_lut128(p, nontrivial)
    bsk = upload_key(gpu, st, p, keys)
    try:
        outs = {}
        for chunk in (0, 1, 2, 3, 5):
            lib.hip_backend_set_pbs128_multibit_chunk(chunk)
            outs[chunk] = run_mb(gpu, st, p, bsk, lwes, lut)
    finally:
        lib.hip_backend_set_pbs128_multibit_chunk(0)
    assert [h.decode128(h.phase128(p, keys, o)) for o in outs[0]] == [nontrivial(v) for v in (3, 9, 14)]
    for chunk in (1, 2, 3, 5):
        assert np.array_equal(outs[chunk], outs[0]), chunk


# ------------------------------------------------------------------------------------------------ 5. ten groups
TEN_GROUPS = m.mb("mb128_ten_groups_k2_N2048", 40, 2, 2048, 18, 4, 4)


@pytest.mark.parametrize("kind", [pytest.param("emu", id="emu", marks=pytest.mark.slow),
                                  pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
def test_ten_groups_on_the_production_ring(kind):
    """n = 40, g = 4 on k = 2, N = 2048, 4 levels of 18 bits (a key of 184 MB): messages 0 .. 15 decode and two calls give
    identical words."""
    lib, gpu, st = setup(kind)
    p = TEN_GROUPS
    keys = m.make_keys_mb128(p)
    lwes = h.encrypt_inputs(p, keys, range(16), seed=49)
    lut = h.make_lut128(p, nontrivial)
    bsk = upload_key(gpu, st, p, keys)
    out = run_mb(gpu, st, p, bsk, lwes, lut)
    assert [h.decode128(h.phase128(p, keys, o)) for o in out] == [nontrivial(v) for v in range(16)]
    assert np.array_equal(run_mb(gpu, st, p, bsk, lwes, lut), out)


# ------------------------------------------------------------------------------------------------ 6. streams, graphs
class _Job:
    """buffers and scratch of one launch on its own stream; enqueue() is exactly one _async call"""

    def __init__(self, lib, gpu, p, bsk, lwes, lut):
        self.lib, self.p, self.B, self.bsk = lib, p, len(lwes), bsk
        self.st = gpu.CudaStreams([0])
        self.d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(lwes, self.st)
        self.d_out = gpu.CudaLweCiphertextList.new(p.k * p.N, self.B, self.st, elem_words=2)
        self.d_lut = gpu.CudaGlweCiphertextList.from_glwe_ciphertext_list(h.to_pairs(lut), p.k, p.N, self.st, elem_words=2)
        self.d_idx = gpu.CudaVec.from_cpu_async(np.arange(self.B, dtype=U64), self.st)
        self.buf = C.c_void_p()
        lib.hip_scratch_multi_bit_programmable_bootstrap_128_async(self.st.ptr[0], 0, C.byref(self.buf), p.k, p.N, p.level,
                                                                   self.B, True)
        self.st.synchronize()

    def enqueue(self):
        p = self.p
        self.lib.hip_multi_bit_programmable_bootstrap_128_async(
            self.st.ptr[0], 0, self.d_out.d_vec.ptr, self.d_idx.ptr, self.d_lut.d_vec.ptr, self.d_in.d_vec.ptr, self.d_idx.ptr,
            self.bsk.d_vec.ptr, self.buf, p.n, p.k, p.N, p.g, p.base_log, p.level, self.B, 1, 0)

    def clear_output(self):
        self.lib.cuda_memset_async(self.d_out.d_vec.ptr, 0, self.B * (self.p.k * self.p.N + 1) * 16, self.st.ptr[0], 0)

    def result(self):
        return self.d_out.to_lwe_ciphertext_list(self.st)

    def close(self):
        self.lib.hip_cleanup_multi_bit_programmable_bootstrap_128(self.st.ptr[0], 0, C.byref(self.buf))


@pytest.mark.gpu
def test_two_streams_running_concurrently_give_the_outputs_of_one():
    lib, gpu, st = setup("hip")
    p = SHAPE_SET
    keys, lwes, lut, _ = case_of(p)
    bsk = upload_key(gpu, st, p, keys)
    big = lwes[np.arange(300) % 6]
    ref = run_mb(gpu, st, p, bsk, big, lut)
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
def test_a_call_is_captured_into_a_hip_graph_and_replayed():
    """two chunks, so the captured call is a chain of four launches"""
    from .test_streams_and_graphs import Hip
    lib, gpu, st = setup("hip")
    p = SHAPE_SET
    keys, lwes, lut, _ = case_of(p)
    bsk = upload_key(gpu, st, p, keys)
    lib.hip_backend_set_pbs128_multibit_chunk(3)
    try:
        job = _Job(lib, gpu, p, bsk, lwes, lut)
    finally:
        lib.hip_backend_set_pbs128_multibit_chunk(0)
    hip = Hip()
    try:
        job.enqueue()
        direct = job.result()
        assert np.array_equal(direct, run_mb(gpu, st, p, bsk, lwes, lut))
        graph, exe = hip.capture(job.st.ptr[0], job.enqueue)
        for _ in range(2):
            job.clear_output()
            hip.launch(exe, job.st.ptr[0])
            assert np.array_equal(job.result(), direct)
        hip.destroy(graph, exe)
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ 7. noise squashing
SQUASH_SET = m.mb("mb128_squash_k2_N2048_g4", TOY_2048.n, 2, 2048, 18, 4, 4)


def _squash_and_check(kind, sp, skeys, bsk_of, cases):
    from tfhe_rs_amd import integer_gpu as igpu
    from .test_radix_integer import encrypt_radix
    from .test_radix_integer import setup as radix_setup
    cp, ckeys, st, sks, _ = radix_setup(kind, p=TOY_2048)
    gpu = __import__("tfhe_rs_amd.core_crypto_gpu", fromlist=["x"])
    nsk = igpu.CudaNoiseSquashingKey(bsk_of(gpu, st), 4, 4)
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


@pytest.mark.parametrize("kind", BACKENDS)
def test_noise_squashing_with_a_multi_bit_key(kind):
    """The compute set TOY_2048 (n = 12) with a g = 4 squashing key on the production squashing ring (k = 2, N = 2048, 4
    levels of 18 bits; 55 MB): 32 blocks become 16 and 5 become 3, block i decoding to lo + 4 hi of its pair; the input is
    unchanged."""
    sp = SQUASH_SET
    skeys = m.make_keys_mb128(sp, compute=TOY_2048)
    _squash_and_check(kind, sp, skeys, lambda gpu, st: upload_key(gpu, st, sp, skeys),
                      ((32, 0xD1CEB00C5EEDF00D), (5, 0b1110010011)))


@pytest.mark.parametrize("kind", BACKENDS)
def test_noise_squashing_with_a_classic_key_still_works(kind):
    """the existing path through the same CudaNoiseSquashingKey, which now picks the scratch by the key's class"""
    sp = TOY_SQUASH
    skeys = h.make_keys128(sp, compute=TOY_2048)
    _squash_and_check(kind, sp, skeys, lambda gpu, st: upload_classic_key(gpu, st, sp, skeys), ((5, 0b1110010011),))


# ------------------------------------------------------------------------------------------------ 8. refusals
_MB_KEY = """
        src = np.zeros((2, 4, 3, 2, 2, 256, 2), dtype=np.uint64)
        bsk = gpu.CudaLweMultiBitBootstrapKey128.from_lwe_multi_bit_bootstrap_key(src, 4, 1, 256, 24, 3, 2, st)
"""
_SCRATCH = """
        buf = C.c_void_p()
        lib.hip_scratch_multi_bit_programmable_bootstrap_128_async(S, G, C.byref(buf), 1, 256, 3, 4, True)
        v = gpu.CudaVec(4 * 600 * 2, st)
"""
REFUSALS = {
    "grouping factor above the range": ("""
        v = gpu.CudaVec(64, st)
        src = np.zeros(64, dtype=np.uint64)
        lib.hip_convert_lwe_multi_bit_programmable_bootstrap_key_128_async(S, G, v.ptr, src.ctypes.data_as(C.c_void_p), 10, 1, 3,
                                                                           256, 5)
        """, "unsupported grouping_factor 5 for lwe_dimension 10"),
    "grouping factor below the range": (_SCRATCH + """
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, buf, 10, 1, 256, 1, 24,
                                                           3, 4, 1, 0)
        """, "unsupported grouping_factor 1 for lwe_dimension 10"),
    "lwe dimension no multiple of the grouping factor": (_SCRATCH + """
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, buf, 10, 1, 256, 4, 24,
                                                           3, 4, 1, 0)
        """, "unsupported grouping_factor 4 for lwe_dimension 10"),
    "unsupported ring": ("""
        buf = C.c_void_p()
        lib.hip_scratch_multi_bit_programmable_bootstrap_128_async(S, G, C.byref(buf), 3, 2048, 3, 4, True)
        """, "unsupported (polynomial_size=2048, glwe_dimension=3) for the 128-bit PBS"),
    "polynomial size outside the range": ("""
        buf = C.c_void_p()
        lib.hip_scratch_multi_bit_programmable_bootstrap_128_async(S, G, C.byref(buf), 1, 8192, 3, 4, True)
        """, "polynomial_size 8192 not supported by the 128-bit PBS"),
    "decomposition wider than the torus": ("""
        buf = C.c_void_p()
        lib.hip_scratch_multi_bit_programmable_bootstrap_128_async(S, G, C.byref(buf), 1, 256, 5, 4, True)
        v = gpu.CudaVec(4 * 600 * 2, st)
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, buf, 12, 1, 256, 4, 26,
                                                           5, 4, 1, 0)
        """, "invalid decomposition (base_log=26, level=5)"),
    "scratch of the classic 128-bit bootstrap": ("""
        buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(S, G, C.byref(buf), 12, 1, 256, 3, 4, True, 0)
        v = gpu.CudaVec(4 * 600 * 2, st)
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, buf, 12, 1, 256, 4, 24,
                                                           3, 4, 1, 0)
        """, "multi-bit PBS buffer was not created by hip_scratch_multi_bit_programmable_bootstrap_128_async"),
    "multi-bit scratch given to the classic bootstrap": (_SCRATCH + """
        lib.hip_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, buf, 12, 1, 256, 24, 3, 4)
        """, "PBS buffer was not created by hip_scratch_programmable_bootstrap_128_async"),
    "scratch of other sizes": (_SCRATCH + """
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, buf, 12, 1, 512, 4, 24,
                                                           3, 4, 1, 0)
        """, "multi-bit PBS buffer parameters do not match the call"),
    "more samples than the scratch holds": (_SCRATCH + """
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, buf, 12, 1, 256, 4, 24,
                                                           3, 5, 1, 0)
        """, "num_samples 5 exceeds the scratch capacity 4"),
    "more than one table": (_SCRATCH + """
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, buf, 12, 1, 256, 4, 24,
                                                           3, 4, 2, 0)
        """, "num_many_lut = 2 is not supported"),
    "a key converted for other sizes": (_MB_KEY + _SCRATCH + """
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, bsk.d_vec.ptr, buf, 8, 1, 256,
                                                           2, 24, 3, 4, 1, 0)
        """, "the multi-bit bootstrap key was converted for other sizes (n=4, k=1, level=3, N=256, g=2)"),
    "a key converted for another grouping factor": (_MB_KEY + _SCRATCH + """
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, bsk.d_vec.ptr, buf, 4, 1, 256,
                                                           4, 24, 3, 4, 1, 0)
        """, "the multi-bit bootstrap key was converted for other sizes (n=4, k=1, level=3, N=256, g=2)"),
    "a classic key given to the multi-bit bootstrap": ("""
        src = np.zeros((4, 3, 2, 2, 256, 2), dtype=np.uint64)
        bsk = gpu.CudaLweBootstrapKey128.from_lwe_bootstrap_key(src, 4, 1, 256, 24, 3, st)
        """ + _SCRATCH + """
        lib.hip_multi_bit_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, bsk.d_vec.ptr, buf, 4, 1, 256,
                                                           2, 24, 3, 4, 1, 0)
        """, "the bootstrap key is a classic 128-bit key"),
    "a multi-bit key given to the classic bootstrap": (_MB_KEY + """
        buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(S, G, C.byref(buf), 4, 1, 256, 3, 4, True, 0)
        v = gpu.CudaVec(4 * 600 * 2, st)
        lib.hip_programmable_bootstrap_128_async(S, G, v.ptr, v.ptr, v.ptr, bsk.d_vec.ptr, buf, 4, 1, 256, 24, 3, 4)
        """, "the bootstrap key is a multi-bit 128-bit key (grouping_factor=2)"),
    "multi-bit squashing with a noise reduction type": ("""
        from tfhe_rs_amd import integer_gpu as igpu
        s, keep = igpu.CudaServerKey._streams(st)
        mem = C.c_void_p()
        lib.hip_scratch_integer_apply_noise_squashing_multi_bit_64_async(s, C.byref(mem), 12, 1, 256, 1, 2048, 4, 4, 3, 24, 3, 5,
                                                                         4, 4, True, 1, 4)
        """, "the multi-bit bootstrap has no noise_reduction_type 1"),
    "multi-bit squashing with a grouping factor that does not divide": ("""
        from tfhe_rs_amd import integer_gpu as igpu
        s, keep = igpu.CudaServerKey._streams(st)
        mem = C.c_void_p()
        lib.hip_scratch_integer_apply_noise_squashing_multi_bit_64_async(s, C.byref(mem), 10, 1, 256, 1, 2048, 4, 4, 3, 24, 3, 5,
                                                                         4, 4, True, 0, 4)
        """, "apply_noise_squashing: unsupported grouping_factor 4 for lwe_dimension 10"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_misuse_is_refused_with_a_message(name):
    snippet, message = REFUSALS[name]
    r = run_child(snippet)
    assert r.returncode != 0, r.stdout + r.stderr
    assert message in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ 9. ABI
STANDS_FOR = {
    "hip_convert_lwe_multi_bit_programmable_bootstrap_key_128_async":
        "cuda_convert_lwe_multi_bit_programmable_bootstrap_key_128_async",
    "hip_scratch_multi_bit_programmable_bootstrap_128_async": "scratch_cuda_multi_bit_programmable_bootstrap_128_async",
    "hip_multi_bit_programmable_bootstrap_128_async": "cuda_multi_bit_programmable_bootstrap_128_async",
    "hip_cleanup_multi_bit_programmable_bootstrap_128": "cleanup_cuda_multi_bit_programmable_bootstrap_128",
}


def test_every_new_symbol_is_declared_bound_and_exported_by_the_emulation_build():
    import sys
    sys.path.insert(0, ROOT)
    from tfhe_rs_amd import ffi
    from tools.c_prototypes import parse_prototypes
    lib = use_backend("emu")
    declared = parse_prototypes(open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read())
    for name in list(STANDS_FOR) + ["hip_scratch_integer_apply_noise_squashing_multi_bit_64_async",
                                    "hip_backend_set_pbs128_multibit_chunk", "hip_test_pbs128_multibit_keybundle_async"]:
        assert name in declared and name in ffi.SIGNATURES and hasattr(lib, name), name
    # the squashing scratch: the existing one's parameter list plus grouping_factor
    assert declared["hip_scratch_integer_apply_noise_squashing_multi_bit_64_async"][1] == \
        declared["hip_scratch_integer_apply_noise_squashing_64_async"][1] + ["uint32_t"]


@pytest.mark.skipif(not os.path.isdir(REF_INCLUDE), reason="reference tree absent")
def test_multi_bit_128_prototypes_equal_the_reference_prototypes_they_stand_for():
    import sys
    sys.path.insert(0, ROOT)
    from tools.c_prototypes import parse_prototypes
    ours = parse_prototypes(open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read())
    ref = parse_prototypes(open(os.path.join(REF_INCLUDE, "pbs", "programmable_bootstrap_multibit.h")).read())
    for mine, theirs in STANDS_FOR.items():
        assert mine in ours and theirs in ref, (mine, theirs)
        assert ours[mine] == ref[theirs], f"{mine}: {ours[mine]} != {ref[theirs]}"


# ------------------------------------------------------------------------------------------------ 10. census
def dispatched():
    """what pbs128_multibit.h can launch: the (N, k + 1) pairs of pbs128_mb_dispatch, {(N, k + 1): (base_log, level)} of
    the fixed instantiations of launch_pbs128_mb_nk; and from pbs128.h the largest base_log digit_to_f128 turns into one
    double"""
    text = open(HEADER).read()
    body = text[text.index("inline bool pbs128_mb_dispatch("):]
    body = body[body.index("#define HX_PBS128_MB_CASE"):body.index("#undef HX_PBS128_MB_CASE")]
    pairs = [(int(N), int(K1)) for N, K1 in re.findall(r"HX_PBS128_MB_CASE\((\d+), (\d+)\)", body)]
    nk = text[text.index("static void launch_pbs128_mb_nk("):text.index("inline bool pbs128_mb_dispatch(")]
    fixed = {}
    for N, K1, tail in re.findall(r"if constexpr \(N == (\d+) && K1 == (\d+)\) \{(.*?)\n  \}", nk, re.S):
        for bl, lv, tbl, tlv in re.findall(r"a\.base_log == (\d+) && a\.level == (\d+)\) return "
                                           r"launch_pbs128_mb_inst<N, K1, (\d+), (\d+)>", tail):
            assert (bl, lv) == (tbl, tlv), "a fixed instantiation selected by another decomposition than its own"
            fixed[(int(N), int(K1))] = (int(bl), int(lv))
    assert len(re.findall(r"launch_pbs128_mb_inst<", nk)) == len(fixed) + 1, "launch_pbs128_mb_nk: a launch this test cannot read"
    single = re.search(r"HX_DEV f128 digit_to_f128\(.*?base_log <= (\d+)\) return f128\{\(double\)", open(SINGLE_HEADER).read(),
                       re.S)
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


def test_every_dispatched_instantiation_has_a_row():
    """Reads pbs128_multibit.h.  Every (N, k + 1) pair of the multi-bit dispatcher needs a row of section 2 off the fixed
    decomposition, the fixed instantiation a row on it, both sides of the digit conversion's branch and level 1 a row each;
    every row is listed for exactly one of these and fulfils it, so taking any row out leaves one uncovered.  The fixed
    instantiation is the production multi-bit squashing decomposition, and every grouping factor has a row."""
    pairs, fixed, single = dispatched()
    assert len(pairs) == len(set(pairs)) and set(fixed) <= set(pairs)
    assert fixed == {(2048, 3): (18, 4)}
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
    assert {r.p.g for r in ROWS} == {2, 3, 4}
    for r in ROWS:
        assert r.p.n % r.p.g == 0 and r.p.n <= 12 and 1 <= r.p.base_log <= 64 and r.p.base_log * r.p.level <= 128, r.id


def test_the_multi_bit_dispatcher_lists_the_pairs_of_the_classic_one():
    """every (N, k) that pbs128_supported accepts runs multi-bit too"""
    from .test_pbs128_dispatch_coverage import dispatched as classic
    assert sorted(dispatched()[0]) == sorted(classic()[0])
