"""The 64-bit ciphertext compression on every shape the reference ships and on the edges of its pack / unpack kernels.

tests/test_compression.py is the feature's narrative; this file is its census and its edge grid:

  1. tests/golden/reference_compression_sets.json (every CompressionParameters constant of the reference, transcribed by
     tests/golden/make_compression_sets.py) and a census that fails when one of its shapes has no word-for-word row
     here, when a row names a shape it lacks, and when its pinned counts change;
  2. the packing keyswitch at the production shape (2048 -> 4 x 256: 1 280 columns, 40 full column tiles) on every
     kernel form a packing call can reach, with hip_backend_last_keyswitch_instantiation asserted in full;
  3. pks_rotate_pack_kernel on values the test chooses (a packing key written word by word), so that every rounding
     class of the modulus switch occurs at every kind of position, at storage widths 1 ... 63;
  4. unpack_glwe_kernel and unpack_extract_kernel on host-packed values at the same widths;
  5. decompression on every bootstrap shape of the fixture, and device = emulation for compress -> host -> decompress.

Everything integer is compared WORD FOR WORD with the NumPy restatement (tests/compression_helper.py), the bootstrap
with the oracle bootstrap of the restated LWEs.  [emu] runs the kernel sources on the host, [hip] on the MI355X.
docs/history/compression_coverage_log.md records what each row covers, the mutation check and the durations.
"""
import contextlib
import ctypes as C
import dataclasses
import functools
import json
import os
import types

import numpy as np
import pytest

from tfhe_rs_amd import core_crypto_gpu as gpu
from tfhe_rs_amd import integer_gpu as igpu

from . import compression_helper as ch
from . import compression_reference_sets as cs
from . import oracle as orc
from .common import Params, decode
from .harness import use_backend
from .test_compression import MSG, N_IN, setup
from .test_keyswitch_dispatch_coverage import SENTINEL, SMALL_BASE, first_difference, gemm, one, scalar
from .test_keyswitch_dispatch_coverage import Case as KsCase
from .test_keyswitch_dispatch_coverage import expected_instantiation as ks_rule
from .test_keyswitch_dispatch_coverage import last_instantiation as last_ks_instantiation
from .test_pbs_dispatch_coverage import BLOCK, GENERIC, MB_LATENCY, PAR, PLAIN, POSITION
from .test_pbs_dispatch_coverage import last_instantiation as last_pbs_instantiation

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64
M64 = ch.M64
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


# ================================================================ 1. the reference's shapes, and the census
SETS = json.load(open(os.path.join(HERE, "golden", "reference_compression_sets.json")))["sets"]
# pinned as REFERENCE_PBS_SHAPES is: a fixture regenerated from a newer tree must fail here, not pass with a shape unseen
PINNED = {"sets": 54, "packing shapes": 3, "bootstrap shapes": 4}


def packing_shape(e):
    return (e["packing_ks_base_log"], e["packing_ks_level"], e["packing_ks_glwe_dimension"], e["packing_ks_polynomial_size"],
            e["lwe_per_glwe"], e["storage_log_modulus"])


def bootstrap_shape(e):
    return (e["br_base_log"], e["br_level"], e["grouping"])


def shape_of(cp):
    return (cp.ks_base_log, cp.ks_level, cp.k, cp.N, cp.lwe_per_glwe, cp.storage_log_modulus)


# packing shape -> (toy twin: [emu], the set at full size: [hip]); test_compress_row runs each
COMPRESS_ROWS = {shape_of(real): (toy, real) for toy, real in
                 ((ch.TOY_PACK, ch.REAL), (cs.TOY_PACK_B6, cs.REAL_GAUSSIAN), (cs.TOY_PACK_L4, cs.REAL_V0_10))}

COMPRESSION_INPUT_DIMENSION = 1024       # k N of every set of the fixture: the decompression bootstrap's input dimension


@dataclasses.dataclass(frozen=True)
class DecompressRow:
    cp_real: ch.CompressionParams        # [hip]: the compression set, on the real compute ring (k = 1, N = 2048)
    cp_toy: ch.CompressionParams         # [emu]: its packing decomposition on 4 x 256, from a toy compute ring (k = 1, N = 256)
    inst_hip: tuple                      # what the automatic choice launches for input dimension 1024, a handful of LWEs
    inst_emu: tuple


def _toy_1024(real, name):
    return dataclasses.replace(real, name=name, pksk_noise=20)


# (br_base_log, br_level, grouping) -> row.  Pairing as in the reference: (15, 2) and the classic-struct GPU sets
# (23, 1, g = 4) come with the 2^6 x 2 packing, (22, 1, g = 4) with 2^4 x 3.  [hip]: N = 2048, k = 1: the block (latency)
# kernel, templated for (1, 23) only; the multi-bit latency path with the products on the block kernel, templated for
# (1, 22) and (2, 15), keybundles in position order below 17 LWEs.  [emu]: N = 256: the generic kernels, one thread
# group per polynomial.
DECOMPRESS_ROWS = {
    (23, 1, 0): DecompressRow(ch.REAL, _toy_1024(ch.REAL, "toy_comp_4x256_b4_l3"),
                              (BLOCK, 1, 23, 0, PLAIN, 1, 2048, 2), (GENERIC, 0, 0, 0, PAR, 1, 256, 2)),
    (15, 2, 0): DecompressRow(cs.REAL_GAUSSIAN, _toy_1024(cs.REAL_GAUSSIAN, "toy_comp_4x256_b6_l2"),
                              (BLOCK, 0, 0, 0, PLAIN, 1, 2048, 2), (GENERIC, 0, 0, 0, PAR, 1, 256, 2)),
    (22, 1, 4): DecompressRow(ch.REAL, _toy_1024(ch.REAL, "toy_comp_4x256_b4_l3"),
                              (MB_LATENCY, 1, 22, 0, POSITION, 1, 2048, 2), (MB_LATENCY, 0, 0, 0, PAR, 1, 256, 2)),
    (23, 1, 4): DecompressRow(cs.REAL_GAUSSIAN, _toy_1024(cs.REAL_GAUSSIAN, "toy_comp_4x256_b6_l2"),
                              (MB_LATENCY, 0, 0, 0, POSITION, 1, 2048, 2), (MB_LATENCY, 0, 0, 0, PAR, 1, 256, 2)),
}


def census(sets, compress_rows, decompress_rows, pinned):
    assert len(sets) == pinned["sets"], f"{len(sets)} sets in the fixture, {pinned['sets']} pinned"
    assert len({e["name"] for e in sets}) == len(sets)
    packing = {packing_shape(e) for e in sets}
    bootstrap = {bootstrap_shape(e) for e in sets}
    assert len(packing) == pinned["packing shapes"], sorted(packing)
    assert len(bootstrap) == pinned["bootstrap shapes"], sorted(bootstrap)
    assert not sorted(packing - set(compress_rows)), f"packing shapes without a compress row: {sorted(packing - set(compress_rows))}"
    assert not sorted(set(compress_rows) - packing), f"compress rows for shapes the fixture lacks: {sorted(set(compress_rows) - packing)}"
    assert not sorted(bootstrap - set(decompress_rows)), f"bootstrap shapes without a decompress row: {sorted(bootstrap - set(decompress_rows))}"
    assert not sorted(set(decompress_rows) - bootstrap), f"decompress rows for shapes the fixture lacks: {sorted(set(decompress_rows) - bootstrap)}"
    for shape, (toy, real) in compress_rows.items():
        # the row runs what it is filed under: the set itself at full size, its decomposition and storage width on the twin
        assert shape_of(real) == shape, (shape, real.name)
        assert (toy.ks_base_log, toy.ks_level, toy.storage_log_modulus) == (shape[0], shape[1], shape[5]), (shape, toy.name)
        assert toy.lwe_per_glwe == toy.N and real.lwe_per_glwe == real.N and toy.ncols > 32      # more than one column tile
    for e in sets:
        assert e["packing_ks_glwe_dimension"] * e["packing_ks_polynomial_size"] == COMPRESSION_INPUT_DIMENSION, e["name"]
        assert (e["kind"] == "gpu_multi_bit") == (e["grouping"] > 0) and (e["struct"] == "Classic" or e["grouping"] > 0), e["name"]
    for (base_log, level, g), row in decompress_rows.items():
        for cp in (row.cp_real, row.cp_toy):
            assert cp.lwe_dimension == COMPRESSION_INPUT_DIMENSION
            # a pairing the reference ships: some set has this bootstrap shape with this packing decomposition
            assert any(bootstrap_shape(e) == (base_log, level, g) and packing_shape(e)[:2] == (cp.ks_base_log, cp.ks_level)
                       for e in sets), (base_log, level, g, cp.name)
        assert shape_of(row.cp_real) in compress_rows


def test_every_reference_compression_shape_has_a_row():
    census(SETS, COMPRESS_ROWS, DECOMPRESS_ROWS, PINNED)
    # what the issue counted by hand: 2^6 x 2 is the decomposition of 38 sets, and the 2^-64 files carry (15, 2)
    assert sum(packing_shape(e)[:2] == (6, 2) for e in SETS) == 38
    assert {e["where"].split("/")[-2] for e in SETS if bootstrap_shape(e) == (15, 2, 0)} == {"p_fail_2_minus_64"}


def test_census_fails_on_a_missing_row_a_stale_row_and_a_changed_count():
    extra = dict(SETS[0], name="NEW", packing_ks_base_log=5)
    with pytest.raises(AssertionError, match="pinned"):
        census(SETS + [dict(SETS[0], name="NEW")], COMPRESS_ROWS, DECOMPRESS_ROWS, PINNED)
    with pytest.raises(AssertionError):      # a new shape changes the pinned count of shapes ...
        census(SETS[:-1] + [extra], COMPRESS_ROWS, DECOMPRESS_ROWS, PINNED)
    with pytest.raises(AssertionError, match="without a compress row"):      # ... and, re-pinned, has no row
        census(SETS[:-1] + [extra], COMPRESS_ROWS, DECOMPRESS_ROWS, dict(PINNED, **{"packing shapes": 4}))
    with pytest.raises(AssertionError, match="without a decompress row"):
        census(SETS[:-1] + [dict(SETS[0], name="NEW", br_base_log=14, br_level=2)], COMPRESS_ROWS, DECOMPRESS_ROWS,
               dict(PINNED, **{"bootstrap shapes": 5}))
    stale = dict(COMPRESS_ROWS)
    stale[(8, 2, 4, 256, 256, 12)] = (ch.TOY_PACK_B8, dataclasses.replace(ch.REAL, ks_base_log=8, ks_level=2))
    with pytest.raises(AssertionError, match="compress rows for shapes the fixture lacks"):
        census(SETS, stale, DECOMPRESS_ROWS, PINNED)
    with pytest.raises(AssertionError, match="decompress rows for shapes the fixture lacks"):
        census(SETS, COMPRESS_ROWS, {**DECOMPRESS_ROWS, (14, 2, 3): DECOMPRESS_ROWS[(15, 2, 0)]}, PINNED)


# ================================================================ launching
@contextlib.contextmanager
def backend(kind):
    """The library of a backend and a stream of its own, destroyed while that library is still the selected one (a
    stream kept beyond the test would be destroyed at interpreter exit by whichever backend was selected last)."""
    lib = use_backend(kind)
    st = gpu.CudaStreams.new_single_gpu(0)
    try:
        yield lib, st
    finally:
        use_backend(kind)
        st.destroy()


def run_packing(kind, cp, key, lwes, per, n_in, choice=0):
    """hip_packing_keyswitch_lwe_list_to_glwe_64_async into an output pre-filled with a sentinel and followed by a guard
    GLWE: (the GLWEs, the keyswitch form that ran)."""
    with backend(kind) as (lib, st):
        lwes = np.ascontiguousarray(lwes, dtype=U64).reshape(-1, n_in + 1)
        count, glwes = len(lwes), -(-len(lwes) // per)
        d_out = gpu.CudaVec.from_cpu_async(np.full((glwes + 1) * cp.ncols, SENTINEL, dtype=U64), st)
        d_in, d_key = gpu.CudaVec.from_cpu_async(lwes, st), gpu.CudaVec.from_cpu_async(key, st)
        s, keep = gpu._streams_ffi(st)
        mem = C.c_void_p()
        shape = (n_in, cp.k, cp.N, cp.ks_base_log, cp.ks_level)
        lib.hip_scratch_packing_keyswitch_lwe_list_to_glwe_64_async(s, C.byref(mem), *shape, count, True)
        try:
            lib.hip_backend_set_keyswitch_kernel(choice)
            lib.hip_packing_keyswitch_lwe_list_to_glwe_64_async(s, d_out.ptr, d_in.ptr, d_key.ptr, mem, *shape, count, per)
            inst = last_ks_instantiation(lib)
        finally:
            lib.hip_backend_set_keyswitch_kernel(0)
        got = d_out.copy_to_cpu(st).reshape(glwes + 1, cp.ncols)
        lib.hip_cleanup_packing_keyswitch_lwe_list_to_glwe_64(s, C.byref(mem))
        for v in (d_out, d_in, d_key):      # the key takes its cached matrix-core layout along
            v.drop()
        assert (got[glwes] == U64(SENTINEL)).all(), "written past the last GLWE"
        return got[:glwes], inst


def run_compress(kind, cp, key, blocks, n_in):
    """hip_integer_compress_radix_ciphertext_64_async into a sentinel-filled buffer of one word more than the list:
    (the packed words, the keyswitch form that ran)."""
    with backend(kind) as (lib, st):
        blocks = np.ascontiguousarray(blocks, dtype=U64).reshape(-1, n_in + 1)
        total = len(blocks)
        words = int(lib.hip_integer_compressed_size_words(cp.k, cp.N, cp.lwe_per_glwe, cp.storage_log_modulus, total))
        assert words == -(-total // cp.lwe_per_glwe) * cp.words_per_glwe
        d_out = gpu.CudaVec.from_cpu_async(np.full(words + 1, SENTINEL, dtype=U64), st)
        d_key = gpu.CudaVec.from_cpu_async(key, st)
        ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(blocks[None], st)
        s, keep = gpu._streams_ffi(st)
        mem = C.c_void_p()
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(s, C.byref(mem), n_in, cp.k, cp.N, cp.ks_base_log, cp.ks_level,
                                                                   total, MSG, MSG, cp.lwe_per_glwe, cp.storage_log_modulus, True)
        keys = (C.c_void_p * 1)(d_key.ptr)
        lib.hip_integer_compress_radix_ciphertext_64_async(s, d_out.ptr, C.byref(ct._ffi()), keys, mem)
        inst = last_ks_instantiation(lib)
        got = d_out.copy_to_cpu(st)
        lib.hip_cleanup_integer_compress_radix_ciphertext_64(s, C.byref(mem))
        for v in (d_out, d_key, ct.d_blocks):
            v.drop()
        assert got[words] == U64(SENTINEL), "written past the last packed word"
        return got[:words], inst


def run_extract_glwe(kind, cp, words, glwe_index, total):
    """hip_integer_extract_glwe_64_async from a buffer of exactly the list's size into a sentinel-guarded GLWE"""
    with backend(kind) as (lib, st):
        d_words = gpu.CudaVec.from_cpu_async(words, st)
        assert d_words.len == len(words) == -(-total // cp.lwe_per_glwe) * cp.words_per_glwe      # nothing behind the last word
        d_out = gpu.CudaVec.from_cpu_async(np.full(2 * cp.ncols, SENTINEL, dtype=U64), st)
        s, keep = gpu._streams_ffi(st)
        lib.hip_integer_extract_glwe_64_async(s, d_out.ptr, d_words.ptr, glwe_index, cp.k, cp.N, cp.lwe_per_glwe,
                                              cp.storage_log_modulus, total)
        got = d_out.copy_to_cpu(st)
        d_words.drop(), d_out.drop()
        assert (got[cp.ncols:] == U64(SENTINEL)).all(), "written past the GLWE"
        return got[:cp.ncols]


@functools.lru_cache(maxsize=4)
def uniform_packing_key(cp, n_in):
    """Uniform words in the packing key's layout [n_in][level][(k+1) N]: the sums are exact integers modulo 2^64
    whatever the key holds, so where nothing is decrypted no key is generated."""
    rng = np.random.default_rng(n_in * 131 + cp.ncols * 17 + cp.ks_level * 5 + cp.ks_base_log)
    return rng.integers(0, 1 << 64, size=n_in * cp.ks_level * cp.ncols, dtype=U64)


# ================================================================ 2. packing keyswitch: production shapes on every form
PKS_SETS = {"b4_l3": (ch.TOY_PACK, ch.REAL), "b6_l2": (cs.TOY_PACK_B6, cs.REAL_GAUSSIAN), "b4_l4": (cs.TOY_PACK_L4, cs.REAL_V0_10)}
# every batch size at which the launch of the one-launch kernel changes (the wave split of K up to 32 LWEs, one workgroup
# row up to 128, the workgroups per column tile halved per doubling of the rows); 768 / 769: the automatic switch to
# digit pass + staged GEMM — 769 blocks are 13 FheUint128 minus 63 blocks; [hip] only: 769 x 2048 x 6 144 products on
# the emulation cost more than the form is worth there, test_keyswitch_dispatch_coverage has it on the emulation at 41 columns
PKS_BATCHES = (1, 32, 33, 128, 129, 256, 257)
PKS_BATCHES_GPU = (768, 769)
POOL = 769


@dataclasses.dataclass(frozen=True)
class PksRow:
    id: str
    tag: str
    batch: int
    choice: int = 0
    gpu_only: bool = False


PKS_ROWS = [PksRow(f"{tag}_batch_{b}", tag, b, gpu_only=b in PKS_BATCHES_GPU)
            for tag in PKS_SETS for b in PKS_BATCHES + PKS_BATCHES_GPU]
# the forced choices: scalar kernels, the one-launch kernel past 768, digit pass + GEMM from 129 on
PKS_ROWS += [PksRow(f"{tag}_forced_{choice}_batch_{b}", tag, b, choice, gpu_only=b > 257)
             for tag in PKS_SETS for choice, b in ((1, 33), (2, 257), (2, 769), (3, 129), (3, 257))]


def pks_expected(cp, row):
    return ks_rule(KsCase(row.id, N_IN, cp.ncols - 1, cp.ks_base_log, cp.ks_level, 64, row.batch, row.choice, None))


def test_packing_rows_are_what_the_issue_lists():
    """The production shape in numbers: (4, 3) runs LEVEL 4 PADDED and (6, 2) LEVEL 2 unpadded, both over 40 full column
    tiles; 2^6 is the last base the matrix cores take."""
    real = {tag: pair[1] for tag, pair in PKS_SETS.items()}
    row = lambda tag, b, choice=0: pks_expected(real[tag], PksRow("", tag, b, choice))
    assert all(cp.ncols == 1280 and cp.ncols % 32 == 0 for cp in real.values())
    assert row("b4_l3", 1) == one(4, True, 64, 4, 8, 40) and row("b4_l3", 33) == one(4, True, 64, 1, 8, 40)
    assert row("b6_l2", 32) == one(2, False, 64, 4, 8, 40) and row("b6_l2", 129) == one(2, False, 64, 1, 4, 40)
    assert row("b4_l4", 257) == one(4, False, 64, 1, 4, 40) and row("b4_l4", 768) == one(4, False, 64, 1, 2, 40)
    assert row("b4_l3", 769) == gemm(4, True, 64, 2, 40) and row("b6_l2", 769) == gemm(2, False, 64, 2, 40)
    assert row("b6_l2", 769, 2) == one(2, False, 64, 1, 2, 40) and row("b6_l2", 129, 3) == gemm(2, False, 64, 2, 40)
    assert row("b6_l2", 33, 1) == scalar(SMALL_BASE)
    for toy, cp in PKS_SETS.values():
        for b in PKS_BATCHES:       # the twin launches the form of the full size, over 6 column tiles
            full, twin = pks_expected(cp, PksRow("", "", b)), pks_expected(toy, PksRow("", "", b))
            assert twin[:7] == full[:7] and twin[7] == full[7] % 256 + 256 * 6, (toy.name, b)
    assert pks_expected(cs.TOY_PACK_B7, PksRow("", "", 33)) == scalar(SMALL_BASE)
    ids = [r.id for r in PKS_ROWS]
    assert len(ids) == len(set(ids))


@functools.lru_cache(maxsize=1)
def _pool():
    return np.random.default_rng(0x706B73).integers(0, 1 << 64, size=(POOL, N_IN + 1), dtype=U64)


@functools.lru_cache(maxsize=None)
def _pool_glwes(cp, batch):
    """The restated GLWEs of the first `batch` LWEs of the pool: once per (set, batch size), shared by the choices"""
    return ch.packing_keyswitch(_pool()[:batch], uniform_packing_key(cp, N_IN), N_IN, cp)


def _pks_params():
    out = []
    for r in PKS_ROWS:
        for kind in ("emu", "hip"):
            if kind == "emu" and r.gpu_only:
                continue
            out.append(pytest.param(kind, r, id=f"{kind}-{r.id}", marks=[pytest.mark.gpu] if kind == "hip" else []))
    return out


@pytest.mark.parametrize("kind,row", _pks_params())
def test_packing_keyswitch_form_word_for_word(kind, row):
    cp = PKS_SETS[row.tag][kind == "hip"]
    want = _pool_glwes(cp, row.batch)
    got, inst = run_packing(kind, cp, uniform_packing_key(cp, N_IN), _pool()[:row.batch], cp.lwe_per_glwe, N_IN, row.choice)
    assert inst == pks_expected(cp, row), f"{row.id}: ran {inst}, the row is for {pks_expected(cp, row)}"
    assert np.array_equal(got, want), f"{row.id}: {first_difference(got, want)}"
    if row.choice == 0 and cp.ks_base_log == 6:
        assert inst[0] in (1, 2), "2^6 must stay on the matrix cores"


@pytest.mark.parametrize("kind", BACKENDS)
def test_base_7_leaves_the_matrix_cores(kind):
    """ks_base_log <= 6 from the other side: the (7, 2) toy takes the scalar kernels under the automatic choice (the
    (6, 2) rows above take a matrix-core path), with the oracle's words."""
    cp = cs.TOY_PACK_B7
    key = uniform_packing_key(cp, N_IN)
    lwes = _pool()[:33]
    got, inst = run_packing(kind, cp, key, lwes, cp.lwe_per_glwe, N_IN)
    assert inst == scalar(SMALL_BASE), inst
    want = ch.packing_keyswitch(lwes, key, N_IN, cp)
    assert np.array_equal(got, want), first_difference(got, want)


@pytest.mark.parametrize("kind", BACKENDS)
def test_packing_keyswitch_on_decomposer_edge_values_base_6(kind):
    """tests/test_compression.py::test_packing_keyswitch_on_decomposer_edge_values on 2^6 x 2: masks made of 0, 2^63, all
    ones, and values exactly half way between two representables (and one below / above), on a generated key."""
    cp = cs.TOY_PACK_B6 if kind == "emu" else cs.REAL_GAUSSIAN
    lib, st, ck, pksk, comp, gpu_, igpu_ = setup(kind, cp)
    bits = cp.ks_base_log * cp.ks_level
    rng = np.random.default_rng(102)
    r = rng.integers(0, 1 << bits, size=N_IN, dtype=U64) << U64(64 - bits)
    half = U64(1 << (63 - bits))
    masks = [np.zeros(N_IN, dtype=U64), np.full(N_IN, 1 << 63, dtype=U64), np.full(N_IN, M64, dtype=U64),
             r + half, r + half - U64(1), r + half + U64(1), r,
             np.where(np.arange(N_IN) % 2 == 0, r + half, U64(M64))]
    lwes = np.stack([np.concatenate([m, [U64(b)]]) for m, b in zip(masks, rng.integers(0, 1 << 64, size=len(masks), dtype=U64))])
    want = ch.packing_keyswitch(lwes, ck.pksk, N_IN, cp, len(masks))
    for mode in (0, 1):
        got, inst = run_packing(kind, cp, ck.pksk, lwes, len(masks), N_IN, mode)
        assert inst[0] == (1 if mode == 0 else 0), inst
        assert np.array_equal(got, want), (cp.name, mode, first_difference(got, want))


@pytest.mark.parametrize("shape", list(COMPRESS_ROWS), ids=lambda s: "b%d_l%d_k%d_N%d_%d_per_glwe_%d_bits" % s)
@pytest.mark.parametrize("kind", BACKENDS)
def test_compress_row(kind, shape):
    """The census' compress rows: multiply, pack, switch, bit-pack on the toy twin [emu] and the set itself [hip];
    lwe_per_glwe + 1 blocks: a full GLWE and a partial one of one LWE."""
    cp = COMPRESS_ROWS[shape][kind == "hip"]
    key = uniform_packing_key(cp, N_IN)
    blocks = _pool()[-(cp.lwe_per_glwe + 1):]
    want = ch.compress(blocks, key, N_IN, cp, MSG)
    got, inst = run_compress(kind, cp, key, blocks, N_IN)
    assert inst == pks_expected(cp, PksRow("", "", len(blocks))), inst
    assert np.array_equal(got, want), (cp.name, first_difference(got.reshape(2, -1), want.reshape(2, -1)))


# ================================================================ 3. pks_rotate_pack_kernel on chosen values
WIDTHS = (1, 2, 7, 12, 31, 32, 33, 63)
BELOW, ABOVE = (1, 2, 7, 12, 31), (33, 63)
CLASSES = ("half_minus_1", "half", "half_plus_1", "wraps_to_0", "zero", "two_to_63")
REGIONS = ("mask", "body_used", "body_beyond")


@dataclasses.dataclass(frozen=True)
class GridRow:
    s: int           # storage_log_modulus
    N: int
    k: int
    per: int         # lwe_per_glwe
    full: int        # full GLWEs
    partial: int     # LWEs of the last GLWE (0: none)

    @property
    def id(self):
        return f"s{self.s}_N{self.N}_k{self.k}_per{self.per}_{self.full}x_plus_{self.partial}"

    @property
    def count(self):
        return self.full * self.per + self.partial

    @property
    def n_in(self):
        return 32 * -(-self.count // 32)     # one mask position per LWE; a multiple of 32: the matrix cores take it

    @property
    def cp(self):
        return ch.CompressionParams(self.id, self.k, self.N, 4, 3, self.per, self.s, 0)


def grid():
    """The pruning rule.  The full product widths x N x k x lwe_per_glwe x partial count has 8 * 2 * 2 * 7 * 2 = 448 rows;
    what distinguishes them for the kernel is (width, N) — the word assembly and which words a workgroup's 64 values
    span, with the mask / body border inside a workgroup at N < 64 — and (lwe_per_glwe, partial count) — which waves
    contribute and which body values are stored.  So: for each N, every lwe_per_glwe of 1, 2, 3, 4, 5, N - 1, N gets one
    width below 32 and one above, the widths taken in rotation (5 below, 2 above: each occurs with each N); the row below
    32 ends in a partial GLWE of one LWE, the row above in one of lwe_per_glwe - 1; k alternates with the rows; width
    32, which is neither, gets a row per N at lwe_per_glwe = N.  As many full GLWEs as give each class a used body
    coefficient (at least two).  30 rows."""
    rows = []
    for N in (16, 64):
        for i, per in enumerate((1, 2, 3, 4, 5, N - 1, N)):
            full = max(2, len(CLASSES) + 1 - per)
            rows.append(GridRow(BELOW[(i + (N == 64)) % 5], N, 1 + i % 2, per, full, 1 if per > 1 else 0))
            rows.append(GridRow(ABOVE[(i + (N == 64)) % 2], N, 2 - i % 2, per, full, per - 1))
        rows.append(GridRow(32, N, 1 + (N == 64), N, 2, 1))
    return rows


GRID = grid()


def test_grid_covers_what_the_pruning_rule_promises():
    assert len(GRID) == 30 and len({r.id for r in GRID}) == 30
    for N in (16, 64):
        assert {r.s for r in GRID if r.N == N} == set(WIDTHS)
        for per in (1, 2, 3, 4, 5, N - 1, N):
            widths = {r.s for r in GRID if r.N == N and r.per == per}
            assert any(s < 32 for s in widths) and any(s > 32 for s in widths), (N, per)
            if per > 1:
                assert {r.partial for r in GRID if r.N == N and r.per == per} >= {1, per - 1}
        for s in WIDTHS:     # a partial GLWE with room for every class beyond its count
            assert any(r.partial and N - r.partial >= len(CLASSES) + 1 for r in GRID if r.N == N and r.s == s), (N, s)
    assert {r.k for r in GRID} == {1, 2}
    assert all(r.n_in >= r.count and r.n_in <= 192 for r in GRID)


def class_value(name, s, rng):
    """A 64-bit value of the class: the low 64 - s bits chosen, the stored bits random (not all ones, so that only the
    class that is meant to wrap does)."""
    low = 64 - s
    high = int(rng.integers(0, (1 << s) - 1)) << low if s > 1 else 0
    if name == "zero":
        return 0
    if name == "two_to_63":
        return 1 << 63
    if name == "wraps_to_0":
        return (M64 + 1 - (1 << (low - 1))) + int(rng.integers(0, 1 << (low - 1)))
    return high + ((1 << (low - 1)) + {"half_minus_1": -1, "half": 0, "half_plus_1": 1}[name]) % (1 << low)


def classify(x, s):
    low = 64 - s
    out = set()
    r = x % (1 << low)
    for name, d in (("half_minus_1", -1), ("half", 0), ("half_plus_1", 1)):
        if r == ((1 << (low - 1)) + d) % (1 << low):
            out.add(name)
    if x >= M64 + 1 - (1 << (low - 1)):
        out.add("wraps_to_0")
    if x == 0:
        out.add("zero")
    if x == 1 << 63:
        out.add("two_to_63")
    return out


def region_of(row, glwe, v):
    m = row.per if glwe < row.full else row.partial
    return "mask" if v < row.k * row.N else "body_used" if v - row.k * row.N < m else "body_beyond"


@functools.lru_cache(maxsize=None)
def chosen(row):
    """(blocks, packing key, targets): LWE i = message_modulus * block i has ONE non-zero mask element, the top-level
    digit d_i (odd) at position i, so G_i = (0, .., b_i) - d_i K[i][top level]; value v = (q, p) of a GLWE is
    sum_i +-G_i[q][(p - i) mod N].  For every value one LWE i(v) = v mod m of the GLWE carries a chosen key word, the
    others a zero there, so the value is  -+ d_i * key word (+ b_p where it is a used body coefficient)  and equals
    targets[glwe][v]; the key's other rows (positions no LWE touches, the lower levels) are uniform words."""
    cp, n_in = row.cp, row.n_in
    rng = np.random.default_rng(row.s * 1000 + row.N * 10 + row.per)
    blocks = np.zeros((row.count, n_in + 1), dtype=U64)
    digits = [int(d) for d in rng.integers(0, 1 << (cp.ks_base_log - 2), size=row.count) * 2 + 1]      # odd, < B / 2
    for i, d in enumerate(digits):
        blocks[i, i] = U64((d << (64 - cp.ks_base_log)) // MSG)
    blocks[:, n_in] = rng.integers(0, 1 << 64, size=row.count, dtype=U64)
    body = [(int(b) * MSG) & M64 for b in blocks[:, n_in]]
    key = rng.integers(0, 1 << 64, size=(n_in, cp.ks_level, cp.ncols), dtype=U64)
    top = cp.ks_level - 1                       # row idx of the key holds level (level - idx): the first level is the last row
    key[:row.count, top, :] = 0
    glwes = row.full + (1 if row.partial else 0)
    targets = np.zeros((glwes, cp.ncols), dtype=U64)
    for g in range(glwes):
        m = row.per if g < row.full else row.partial
        at = {region: 0 for region in REGIONS}
        for v in range(cp.ncols):
            region = region_of(row, g, v)
            # every class in turn, then a uniform value; beyond the count of the partial GLWE the turn starts at "half",
            # which does not switch to 0: the first coefficients there are the ones that are stored
            start = 1 if region == "body_beyond" and row.partial and g == row.full else g
            c = (at[region] + start) % (len(CLASSES) + 1)
            at[region] += 1
            t = class_value(CLASSES[c], row.s, rng) if c < len(CLASSES) else int(rng.integers(0, 1 << 64, dtype=U64))
            targets[g, v] = t
            q, p = divmod(v, cp.N)
            i = v % m
            lwe = g * row.per + i
            rest = (t - (body[g * row.per + p] if region == "body_used" else 0)) & M64
            # the value is  sign * (-d K)  with sign = +1 where p >= i: K = -sign * rest / d
            word = (rest * pow(digits[lwe], -1, 1 << 64)) & M64
            key[lwe, top, q * cp.N + (p - i) % cp.N] = U64(word if p < i else (-word) & M64)
    return blocks, key.reshape(-1), targets


def assert_chosen_values_cover_every_class(row):
    """The pre-switch values through the restatement's storage_log_modulus = 0 path: they are the targets, and every
    class occurs in every kind of position the row has."""
    blocks, key, targets = chosen(row)
    cp = row.cp
    raw = ch.packing_keyswitch(blocks * U64(MSG), key, row.n_in, cp)
    assert np.array_equal(raw, targets), first_difference(raw, targets)
    seen = {region: set() for region in REGIONS}
    for g in range(len(raw)):
        for v in range(cp.ncols):
            if region_of(row, g, v) != "body_beyond" or (row.partial and g == row.full):
                seen[region_of(row, g, v)] |= classify(int(raw[g, v]), row.s)
    assert seen["mask"] == set(CLASSES), (row.id, "mask", sorted(set(CLASSES) - seen["mask"]))
    assert seen["body_used"] == set(CLASSES), (row.id, "body_used", sorted(set(CLASSES) - seen["body_used"]))
    # a body coefficient at or beyond the count of the partial GLWE (there is one partial GLWE per call): the classes
    # in rotation over the N - count coefficients there are — all of them from 7 coefficients on; the grid has such a
    # row at every width and N (test_grid_covers_what_the_pruning_rule_promises)
    room = cp.N - row.partial if row.partial else 0
    turn = {CLASSES[(j + 1) % (len(CLASSES) + 1)] for j in range(room) if (j + 1) % (len(CLASSES) + 1) < len(CLASSES)}
    assert seen["body_beyond"] >= turn and (room < len(CLASSES) + 1 or turn == set(CLASSES)), (row.id, "body_beyond")
    assert not row.partial or "half" in classify(int(raw[-1, cp.k * cp.N + row.partial]), row.s)      # stored wherever per > partial
    return raw


def test_chosen_values_put_every_class_at_every_position():
    for row in GRID:
        assert_chosen_values_cover_every_class(row)
    for s in WIDTHS:     # the classes are what the switch does with them
        low, rng = 64 - s, np.random.default_rng(s)
        for name, up in (("half_minus_1", 0), ("half", 1), ("half_plus_1", 1 if low > 1 else 0)):      # 64 - s = 1: residues 0, 1, 0
            x = class_value(name, s, rng)
            assert int(ch.modulus_switch(U64(x), s)) == ((x >> low) + up) % (1 << s), (s, name)
        assert int(ch.modulus_switch(U64(class_value("wraps_to_0", s, rng)), s)) == 0
        assert int(ch.modulus_switch(U64(1 << 63), s)) == 1 << (s - 1)


@pytest.mark.parametrize("row", GRID, ids=lambda r: r.id)
@pytest.mark.parametrize("kind", BACKENDS)
def test_rotate_pack_on_chosen_values(kind, row):
    raw = assert_chosen_values_cover_every_class(row)      # first: the row is about what it claims to be about
    blocks, key, targets = chosen(row)
    cp, s = row.cp, row.s
    want = ch.compress(blocks, key, row.n_in, cp, MSG)
    assert np.array_equal(want, np.concatenate([ch.bit_pack(ch.modulus_switch(g[:cp.values_per_glwe], s), s) for g in raw]))
    words, inst = run_compress(kind, cp, key, blocks, row.n_in)
    assert inst[0] == 1, inst
    got, want = words.reshape(-1, cp.words_per_glwe), want.reshape(-1, cp.words_per_glwe)
    assert np.array_equal(got, want), f"{row.id}: {first_difference(got, want)}"
    used = cp.values_per_glwe * s % 64
    if used:             # the padding bits of every GLWE's last word
        assert not np.any(got[:, -1] >> U64(used)), row.id
    glwes, inst = run_packing(kind, cp, key, blocks * U64(MSG), row.per, row.n_in)
    assert np.array_equal(glwes, raw), f"{row.id}, unswitched: {first_difference(glwes, raw)}"
    for mode in (1, 3):      # the epilogue reads the rows of whichever keyswitch form wrote them
        glwes, inst = run_packing(kind, cp, key, blocks * U64(MSG), row.per, row.n_in, mode)
        assert np.array_equal(glwes, raw), f"{row.id}, keyswitch kernel {mode}: {first_difference(glwes, raw)}"


# ================================================================ 4. unpack_glwe_kernel and unpack_extract_kernel
TOY_RING = Params("toy_k1_N256", 0, 1, 256, 15, 2, 4, 4, 40, 20, 16, ms_type=0)      # the compute ring of the unpack rows


def packed_random(row):
    """Random s-bit values, packed on the host: (values [glwe][values_per_glwe], words)"""
    cp = row.cp
    rng = np.random.default_rng(row.s * 7 + row.N + row.per)
    glwes = row.full + (1 if row.partial else 0)
    vals = rng.integers(0, 1 << row.s, size=(glwes, cp.values_per_glwe), dtype=U64)
    # all ones, where a neighbour's stray bit shows; every 11th: not the last coefficient of a polynomial (15, 31, 63, 127),
    # which the extract rows read negated — the negation of all ones is lost in what a bootstrap sees of a word
    vals[:, ::11] = U64((1 << row.s) - 1)
    return vals, np.concatenate([ch.bit_pack(v, row.s) for v in vals])


def ends_on_a_word(row):
    return any((v + 1) * row.s % 64 == 0 for v in range(row.cp.values_per_glwe))


def straddles_into_the_last_word(row):
    last = row.cp.words_per_glwe - 1
    return any(v * row.s // 64 == last - 1 and ((v + 1) * row.s - 1) // 64 == last for v in range(row.cp.values_per_glwe))


def test_unpack_rows_meet_the_selection_conditions():
    for N in (16, 64):
        rows = [r for r in GRID if r.N == N]
        assert any(ends_on_a_word(r) for r in rows) and any(straddles_into_the_last_word(r) for r in rows)
        assert any(ends_on_a_word(r) and r.s not in (1, 2, 32) for r in rows)      # ... not only where every value does
    # widths that divide 64 never straddle; 12 straddles inside the GLWE in both of its rows (36 and 67 values: the last
    # word starts on a value); every other width has a row with a value that straddles into the last word
    assert {s for s in WIDTHS if any(straddles_into_the_last_word(r) for r in GRID if r.s == s)} == {7, 31, 33, 63}
    assert all(any(v * 12 // 64 != ((v + 1) * 12 - 1) // 64 for v in range(r.cp.values_per_glwe)) for r in GRID if r.s == 12)


def extraction_indexes(row):
    """nth = lwe_per_glwe - 1 (N - 1 where lwe_per_glwe = N) and then 0 — descending within GLWE 0 —, 0 again, the
    first and a middle body of GLWE 1, the last body of the list (of the partial GLWE where there is one)."""
    per = row.per
    return np.array([per - 1, 0, 0, per, per + per // 2, row.count - 1], dtype=np.uint32)


@pytest.mark.parametrize("row", GRID, ids=lambda r: r.id)
@pytest.mark.parametrize("kind", BACKENDS)
def test_unpack_glwe_on_host_packed_values(kind, row):
    cp = row.cp
    vals, words = packed_random(row)
    assert np.array_equal(np.concatenate([ch.bit_unpack(ch.bit_pack(v, row.s), row.s, v.size) for v in vals]), vals.reshape(-1))
    for g in range(len(vals)):
        got = run_extract_glwe(kind, cp, words, g, row.count)
        want = ch.extract_glwe(words, cp, g, row.count)
        assert np.array_equal(got, want), f"{row.id}, GLWE {g}: {first_difference(got[None], want[None])}"
        bodies = row.per if g < row.full else row.partial
        assert np.array_equal(got[:cp.k * cp.N + bodies] >> U64(64 - row.s), vals[g][:cp.k * cp.N + bodies])
        assert not got[cp.k * cp.N + bodies:].any()


_toy_ring_sk = functools.lru_cache(maxsize=1)(lambda: orc.Rng(0x72696E67).binary_key(TOY_RING.k * TOY_RING.N))


def run_decompress(kind, cp, p, dbsk, words, indexes, total):
    """hip_integer_decompress_radix_ciphertext_64_async on host-supplied packed words, into blocks followed by a
    sentinel-filled guard block: (the blocks, the bootstrap instantiation that ran)."""
    with backend(kind) as (lib, st):
        n = cp.lwe_dimension
        if p.grouping:
            key = gpu.CudaLweMultiBitBootstrapKey.from_lwe_multi_bit_bootstrap_key(dbsk, n, p.k, p.N, p.pbs_base_log, p.pbs_level,
                                                                                   p.grouping, st)
        else:
            key = gpu.CudaLweBootstrapKey.from_lwe_bootstrap_key(dbsk, n, p.k, p.N, p.pbs_base_log, p.pbs_level, st,
                                                                 ms_noise_reduction=bool(p.ms_type))
        dec = igpu.CudaDecompressionKey(key, MSG, MSG)
        idx = np.ascontiguousarray(indexes, dtype=np.uint32)
        big = p.k * p.N
        d_words = gpu.CudaVec.from_cpu_async(words, st)
        assert d_words.len == len(words) == -(-total // cp.lwe_per_glwe) * cp.words_per_glwe
        d_out = gpu.CudaVec.from_cpu_async(np.full((idx.size + 1) * (big + 1), SENTINEL, dtype=U64), st)
        out = igpu.CudaUnsignedRadixCiphertext(d_out, 1, idx.size, big)
        s, keep = gpu._streams_ffi(st)
        mem = C.c_void_p()
        keys = (C.c_void_p * 1)(key.d_vec.ptr)
        lib.hip_scratch_integer_decompress_radix_ciphertext_64_async(s, C.byref(mem), dec._bsk_params(), cp.k, cp.N, cp.lwe_per_glwe,
                                                                     cp.storage_log_modulus, idx.size, MSG, MSG, True, p.ms_type)
        lib.hip_integer_decompress_radix_ciphertext_64_async(s, C.byref(out._ffi()), d_words.ptr, total,
                                                             idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size, keys, mem)
        inst = last_pbs_instantiation(lib)
        lib.hip_cleanup_integer_decompress_radix_ciphertext_64(s, C.byref(mem))
        got = d_out.copy_to_cpu(st).reshape(idx.size + 1, big + 1)
        assert int(out.degrees.max()) == MSG - 1
        for v in (d_words, d_out, key.d_vec):
            v.drop()
        assert (got[idx.size] == U64(SENTINEL)).all(), "written past the last block"
        return got[:idx.size], inst


@pytest.mark.parametrize("row", GRID, ids=lambda r: r.id)
@pytest.mark.parametrize("kind", BACKENDS)
def test_unpack_extract_on_host_packed_values(kind, row):
    """The unpack-and-extract launch has no entry point of its own: the decompression of the host-packed words on a toy
    key (compute ring 1 x 256, two levels of 15 bits) equals the oracle bootstrap of the restated extracted LWEs."""
    cp, p = row.cp, dataclasses.replace(TOY_RING, n=row.cp.lwe_dimension)
    vals, words = packed_random(row)
    indexes = extraction_indexes(row)
    per = row.per
    assert all(0 <= int(t) < row.count for t in indexes) and int(indexes[-1]) == row.count - 1
    assert all(int(b) // per >= int(a) // per for a, b in zip(indexes, indexes[1:]))      # what the entry point requires
    assert int(indexes[0]) % per == per - 1 and int(indexes[1]) == 0 == int(indexes[2])   # descending, then repeated
    assert per == 1 or int(indexes[0]) > int(indexes[1])
    if row.partial:
        assert int(indexes[-1]) // per == row.full and int(indexes[-1]) % per == row.partial - 1
    lwes = ch.extract_lwes(words, cp, indexes, row.count)
    # the restated LWE of index t: body = value k N + nth, mask element 0 of polynomial q = value q N + nth
    for t, lwe in zip(indexes, lwes):
        g, nth = divmod(int(t), per)
        assert int(lwe[-1]) == int(vals[g][cp.k * cp.N + nth]) << (64 - row.s)
        assert all(int(lwe[q * cp.N]) == int(vals[g][q * cp.N + nth]) << (64 - row.s) for q in range(cp.k))
    ck = types.SimpleNamespace(glwe_sk=orc.Rng(row.N + row.k).binary_key(cp.lwe_dimension))
    dbsk = ch.gen_decompression_bsk(cp, ck, p, types.SimpleNamespace(glwe_sk=_toy_ring_sk()))
    want = ch.decompress(words, cp, indexes, row.count, dbsk, p, MSG, MSG)
    got, inst = run_decompress(kind, cp, p, dbsk, words, indexes, row.count)
    assert inst == (GENERIC, 0, 0, 0, PAR, 1, 256, 2), inst
    assert np.array_equal(got, want), f"{row.id}: {first_difference(got, want)}"


# ================================================================ 5. decompression on every reference bootstrap shape
def compute_params(kind, shape):
    """The compute set of a decompress row: the bootstrap shape on the real ring [hip] or a toy ring [emu]; delta = 2^59
    (message 2 bits, carry 2 bits, one bit of padding)."""
    base_log, level, g = shape
    k, N = (1, 2048) if kind == "hip" else (1, 256)
    return Params(f"k{k}_N{N}_b{base_log}_l{level}_g{g}", COMPRESSION_INPUT_DIMENSION, k, N, base_log, level, 4, 4, 45, 17, 16,
                  ms_type=0 if g else 1, grouping=g)


def decompress_indexes(cp, total):
    """a handful, spanning two GLWEs: first, middle and last body of the first, first and last of the partial second"""
    per = cp.lwe_per_glwe
    return np.array([0, per // 3, per - 1, per, total - 1], dtype=np.uint32)


def restatement_decrypts(kind, shape):
    """compress -> decompress in the restatement alone at the seeds the row uses: (inputs, expectation, whether every
    chosen block decrypts to its message there)."""
    row = DECOMPRESS_ROWS[shape]
    cp, p = (row.cp_real, row.cp_toy)[kind == "emu"], compute_params(kind, shape)
    n_in = p.k * p.N
    glwe_sk = orc.Rng(0x6B6579 + p.N).binary_key(n_in)
    ck = ch.make_compression_keys(cp, glwe_sk)
    dbsk = ch.gen_decompression_bsk(cp, ck, p, types.SimpleNamespace(glwe_sk=glwe_sk))
    total = cp.lwe_per_glwe + 3
    msgs = np.random.default_rng(105).integers(0, MSG, size=total)
    enc = orc.Rng(106)
    blocks = np.stack([orc.lwe_encrypt(enc, glwe_sk, (int(m) * p.delta) % (1 << 64), p.glwe_noise) for m in msgs])
    words = ch.compress(blocks, ck.pksk, n_in, cp, MSG)
    indexes = decompress_indexes(cp, total)
    want = ch.decompress(words, cp, indexes, total, dbsk, p, MSG, MSG)
    decoded = [decode(p, orc.lwe_decrypt(b, glwe_sk)) for b in want]
    return (cp, p, n_in, glwe_sk, ck, dbsk, blocks, msgs, indexes), (words, want), decoded == [int(msgs[i]) for i in indexes]


@pytest.mark.parametrize("shape", list(DECOMPRESS_ROWS), ids=lambda s: "b%d_l%d_g%d" % s)
@pytest.mark.parametrize("kind", BACKENDS)
def test_decompress_row(kind, shape):
    """One row per bootstrap shape of the fixture, input dimension 1024: compress and decompress word for word, the
    bootstrap on the instantiation the automatic choice takes.  The blocks are decrypted only where the restatement's
    own output decrypts at these seeds (it does in all eight rows: docs/history/compression_coverage_log.md); the
    device's decryption is compared with the messages, never with the device."""
    (cp, p, n_in, glwe_sk, ck, dbsk, blocks, msgs, indexes), (words, want), decrypts = restatement_decrypts(kind, shape)
    total = len(blocks)
    got_words, ks_inst = run_compress(kind, cp, ck.pksk, blocks, n_in)
    assert np.array_equal(got_words, words), first_difference(got_words.reshape(2, -1), words.reshape(2, -1))
    assert {int(i) // cp.lwe_per_glwe for i in indexes} == {0, 1}
    got, inst = run_decompress(kind, cp, p, dbsk, got_words, indexes, total)
    row = DECOMPRESS_ROWS[shape]
    assert inst == (row.inst_hip if kind == "hip" else row.inst_emu), inst
    assert np.array_equal(got, want), first_difference(got, want)
    print(f"{cp.name} -> {p.name}: the restatement {'decrypts' if decrypts else 'does NOT decrypt'} every chosen block")
    if decrypts:
        assert [decode(p, orc.lwe_decrypt(b, glwe_sk)) for b in got] == [int(msgs[i]) for i in indexes]
    if kind == "hip":
        assert decrypts, "the real ring has the noise budget: the row must decrypt"


# ================================================================ device = emulation
def round_trip(kind, cp, seed):
    """compress -> host -> decompress on a toy compute ring (1 x 256): (packed words, decompressed blocks)"""
    p = dataclasses.replace(TOY_RING, n=cp.lwe_dimension)
    n_in = p.k * p.N
    glwe_sk = _toy_ring_sk()
    ck = ch.make_compression_keys(cp, glwe_sk)
    dbsk = ch.gen_decompression_bsk(cp, ck, p, types.SimpleNamespace(glwe_sk=glwe_sk))
    total = 2 * cp.lwe_per_glwe + 1
    blocks = np.random.default_rng(seed).integers(0, 1 << 64, size=(total, n_in + 1), dtype=U64)
    words, _ = run_compress(kind, cp, ck.pksk, blocks, n_in)
    indexes = np.array([cp.lwe_per_glwe - 1, 0, cp.lwe_per_glwe, total - 1], dtype=np.uint32)
    out, _ = run_decompress(kind, cp, p, dbsk, words, indexes, total)
    return words, out


DEVICE_VS_EMULATION = [dataclasses.replace(ch.TOY_DEC, name="toy_comp_k2_N16_b4_l3", ks_base_log=4, ks_level=3),
                       dataclasses.replace(ch.TOY_DEC, name="toy_comp_k2_N16_b6_l2", ks_base_log=6, ks_level=2),
                       dataclasses.replace(ch.TOY_DEC, name="toy_comp_k2_N16_b6_l2_33_bits_5_per_glwe", ks_base_log=6,
                                           ks_level=2, storage_log_modulus=33, lwe_per_glwe=5)]


@pytest.mark.gpu
@pytest.mark.parametrize("cp", DEVICE_VS_EMULATION, ids=lambda cp: cp.name)
def test_device_equals_emulation_word_for_word(cp):
    words, out = round_trip("hip", cp, 111)
    try:
        emu_words, emu_out = round_trip("emu", cp, 111)
    finally:
        use_backend("hip")
    print(f"{cp.name}: hip vs emu: {int((emu_words != words).sum())} of {words.size} packed words and "
          f"{int((emu_out != out).any(axis=1).sum())} of {len(out)} blocks differ")
    assert np.array_equal(emu_words, words)
    assert np.array_equal(emu_out, out)


def test_round_trip_on_the_emulation_equals_the_restatement():
    """What the device is compared with above is itself the restatement's, word for word."""
    for cp in DEVICE_VS_EMULATION:
        p = dataclasses.replace(TOY_RING, n=cp.lwe_dimension)
        words, out = round_trip("emu", cp, 111)
        ck = ch.make_compression_keys(cp, _toy_ring_sk())
        dbsk = ch.gen_decompression_bsk(cp, ck, p, types.SimpleNamespace(glwe_sk=_toy_ring_sk()))
        total = 2 * cp.lwe_per_glwe + 1
        blocks = np.random.default_rng(111).integers(0, 1 << 64, size=(total, p.k * p.N + 1), dtype=U64)
        assert np.array_equal(words, ch.compress(blocks, ck.pksk, p.k * p.N, cp, MSG))
        indexes = np.array([cp.lwe_per_glwe - 1, 0, cp.lwe_per_glwe, total - 1], dtype=np.uint32)
        assert np.array_equal(out, ch.decompress(words, cp, indexes, total, dbsk, p, MSG, MSG))
