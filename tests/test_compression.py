"""Ciphertext compression: packing keyswitch, compress, unpack / extract, decompress, the Python API, streams and
refusals.  Everything integer is compared WORD FOR WORD with the NumPy restatement of the reference CPU algorithms
(tests/compression_helper.py); the decompression bootstrap with the project's oracle bootstrap (f64 engine) of the
restated extracted LWEs, and its outputs are decrypted.  [emu] runs the kernel sources on the host with toy
compression sets on a 2048-coefficient input key, [hip] on the MI355X with the reference's set on
PARAM_MESSAGE_2_CARRY_2 (and the toy sets, which cost nothing there)."""
import ctypes as C
import types

import numpy as np
import pytest

from . import compression_helper as ch
from . import oracle as orc
from .common import C1, C4G4, TOY_2048, TOY_MB4_2048, decode
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_integer import decrypt_blocks, encrypt_radix, recompose
from .test_radix_integer import setup as radix_setup

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
U64 = np.uint64
N_IN = 2048   # every compute set here has a big key of 2048 coefficients
MSG = 4
PATHS = {0: "scalar kernels", 1: "one-launch matrix-core kernel", 2: "digit pass + staged GEMM", 3: "GEMM on emitted digits"}


def compute_key(seed=0x6B6579):
    """a big compute key (2048 bits) for the tests that need no compute bootstrap or keyswitch key"""
    return orc.Rng(seed).binary_key(N_IN)


def setup(kind, cp, sk_in=None):
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import integer_gpu as igpu
    lib = use_backend(kind)
    st = gpu.CudaStreams([0])
    sk_in = compute_key() if sk_in is None else sk_in
    ck = ch.make_compression_keys(cp, sk_in)
    pksk = gpu.CudaLwePackingKeyswitchKey.from_lwe_packing_keyswitch_key(ck.pksk, N_IN, cp.k, cp.N, cp.ks_base_log,
                                                                          cp.ks_level, st)
    comp = igpu.CudaCompressionKey(pksk, cp.lwe_per_glwe, cp.storage_log_modulus, MSG, MSG)
    return lib, st, ck, pksk, comp, gpu, igpu


def sets_for(kind, *toys):
    return list(toys) + ([ch.REAL] if kind == "hip" else [])


def gpu_pack(gpu, pksk, cp, lwes, per, st):
    d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(lwes, st)
    glwes = (len(lwes) + per - 1) // per
    d_out = gpu.CudaGlweCiphertextList(gpu.CudaVec(glwes * cp.ncols, st), glwes, cp.k, cp.N)
    gpu.cuda_keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(pksk, d_in, d_out, st, lwe_per_glwe=per)
    return d_out.to_glwe_ciphertext_list(st)


# ------------------------------------------------------------------------------------------ 1. packing keyswitch
@pytest.mark.parametrize("kind", BACKENDS)
def test_packing_keyswitch_word_for_word(kind):
    """Chunk sizes 1, 2, 33, N - 1 and N, several chunks per call (the last one partial), under every kernel selection;
    the second toy decomposition (base 2^8 x 2 levels: no level padding, a base the matrix-core path declines) reaches
    the scalar kernels without being forced."""
    for cp in sets_for(kind, ch.TOY_PACK, ch.TOY_PACK_B8):
        lib, st, ck, pksk, comp, gpu, igpu = setup(kind, cp)
        rng = np.random.default_rng(101)
        cases = {1: 3, 2: 5, 33: 33 + 33 + 5, cp.N - 1: cp.N - 1 + 10, cp.N: 2 * cp.N + 1}
        for per, count in cases.items():
            lwes = rng.integers(0, 1 << 64, size=(count, N_IN + 1), dtype=U64)
            want = ch.packing_keyswitch(lwes, ck.pksk, N_IN, cp, per)
            # 0: automatic, 1: scalar kernels, 2: one-launch matrix-core kernel, 3: digit pass + GEMM from 129 LWEs on
            for mode in (0, 1, 2, 3):
                lib.hip_backend_set_keyswitch_kernel(mode)
                try:
                    got = gpu_pack(gpu, pksk, cp, lwes, per, st)
                finally:
                    lib.hip_backend_set_keyswitch_kernel(0)
                path = int(lib.hip_backend_last_keyswitch_path())
                print(f"{cp.name}: {count} LWEs, {per} per GLWE, keyswitch kernel {mode}: {PATHS[path]}")
                assert np.array_equal(got, want), (cp.name, per, mode)
                matrix_ok = cp.ks_base_log <= 6
                assert path == (0 if mode == 1 or not matrix_ok else 2 if mode == 3 and count >= 129 else 1), (mode, path)


@pytest.mark.parametrize("kind", BACKENDS)
def test_packing_keyswitch_on_decomposer_edge_values(kind):
    """Masks made of 0, 2^63, all ones, and values exactly half way between two representables (and one below / above)."""
    for cp in sets_for(kind, ch.TOY_PACK, ch.TOY_PACK_B8):
        lib, st, ck, pksk, comp, gpu, igpu = setup(kind, cp)
        bits = cp.ks_base_log * cp.ks_level
        rng = np.random.default_rng(102)
        r = rng.integers(0, 1 << bits, size=N_IN, dtype=U64) << U64(64 - bits)
        half = U64(1 << (63 - bits))
        masks = [np.zeros(N_IN, dtype=U64), np.full(N_IN, 1 << 63, dtype=U64), np.full(N_IN, ch.M64, dtype=U64),
                 r + half, r + half - U64(1), r + half + U64(1), r,
                 np.where(np.arange(N_IN) % 2 == 0, r + half, U64(ch.M64))]
        lwes = np.stack([np.concatenate([m, [U64(b)]]) for m, b in zip(masks, rng.integers(0, 1 << 64, size=len(masks), dtype=U64))])
        want = ch.packing_keyswitch(lwes, ck.pksk, N_IN, cp, len(masks))
        for mode in (0, 1):
            lib.hip_backend_set_keyswitch_kernel(mode)
            try:
                got = gpu_pack(gpu, pksk, cp, lwes, len(masks), st)
            finally:
                lib.hip_backend_set_keyswitch_kernel(0)
            print(f"{cp.name}: edge masks, keyswitch kernel {mode}: {PATHS[int(lib.hip_backend_last_keyswitch_path())]}")
            assert np.array_equal(got, want), (cp.name, mode)


# ------------------------------------------------------------------------------------------ 2. compress
def gpu_compress(igpu, comp, blocks, st):
    ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(blocks[None], st)
    return comp.compress_ciphertexts_into_list([ct], st)


@pytest.mark.parametrize("kind", BACKENDS)
def test_compress_word_for_word(kind):
    """multiply, pack, modulus switch, bit-pack: 1, lwe_per_glwe, lwe_per_glwe + 1 and 3 lwe_per_glwe - 5 blocks; fewer
    LWEs per GLWE than coefficients; 12 stored bits (does not divide 64) and 16 (does)."""
    for cp in sets_for(kind, ch.TOY_PACK, ch.TOY_PACK_STRIDED, ch.TOY_PACK_PAD):
        lib, st, ck, pksk, comp, gpu, igpu = setup(kind, cp)
        rng = np.random.default_rng(103)
        for total in (1, cp.lwe_per_glwe, cp.lwe_per_glwe + 1, 3 * cp.lwe_per_glwe - 5):
            blocks = rng.integers(0, 1 << 64, size=(total, N_IN + 1), dtype=U64)
            packed = gpu_compress(igpu, comp, blocks, st)
            words, meta = packed.to_host(st)
            want = ch.compress(blocks, ck.pksk, N_IN, cp, MSG)
            assert words.size == want.size == -(-total // cp.lwe_per_glwe) * cp.words_per_glwe
            assert np.array_equal(words, want), (cp.name, total)
            used = cp.values_per_glwe * cp.storage_log_modulus % 64
            assert (used != 0) == (cp is ch.TOY_PACK_PAD)
            if used:   # the padding bits of the last word of every GLWE
                assert not np.any(words.reshape(-1, cp.words_per_glwe)[:, -1] >> U64(used)), (cp.name, total)


# ------------------------------------------------------------------------------------------ 3. unpack / extract
def gpu_extract_glwe(lib, gpu, igpu, st, cp, words, glwe_index, total):
    s, keep = igpu.CudaServerKey._streams(st)
    d_words = gpu.CudaVec.from_cpu_async(words, st)
    d_out = gpu.CudaVec(cp.ncols, st)
    lib.hip_integer_extract_glwe_64_async(s, d_out.ptr, d_words.ptr, glwe_index, cp.k, cp.N, cp.lwe_per_glwe,
                                          cp.storage_log_modulus, total)
    return d_out.copy_to_cpu(st)


@pytest.mark.parametrize("kind", BACKENDS)
def test_extract_glwe_and_bit_pack_round_trip(kind):
    for cp in sets_for(kind, ch.TOY_PACK, ch.TOY_PACK_STRIDED, ch.TOY_PACK_PAD):
        lib, st, ck, pksk, comp, gpu, igpu = setup(kind, cp)
        rng = np.random.default_rng(104)
        total = 3 * cp.lwe_per_glwe - 5
        blocks = rng.integers(0, 1 << 64, size=(total, N_IN + 1), dtype=U64)
        words = ch.compress(blocks, ck.pksk, N_IN, cp, MSG)
        for g in range(3):
            got = gpu_extract_glwe(lib, gpu, igpu, st, cp, words, g, total)
            assert np.array_equal(got, ch.extract_glwe(words, cp, g, total)), (cp.name, g)
        tail = got[cp.k * cp.N + cp.lwe_per_glwe - 5:]
        assert tail.size == cp.N - cp.lwe_per_glwe + 5 and not tail.any()   # the partial last GLWE's body tail
        # random s-bit values, packed on the host, unpacked on the device: the identity
        s = cp.storage_log_modulus
        vals = rng.integers(0, 1 << s, size=cp.values_per_glwe, dtype=U64)
        got = gpu_extract_glwe(lib, gpu, igpu, st, cp, ch.bit_pack(vals, s), 0, cp.lwe_per_glwe)
        assert np.array_equal(got[:cp.values_per_glwe] >> U64(64 - s), vals)
        assert np.array_equal(ch.bit_unpack(ch.bit_pack(vals, s), s, vals.size), vals)


# ------------------------------------------------------------------------------------------ 4. decompress
def decompression_key(gpu, igpu, st, cp, ck, p, glwe_sk):
    dbsk = ch.gen_decompression_bsk(cp, ck, p, types.SimpleNamespace(glwe_sk=glwe_sk))
    n = cp.lwe_dimension
    if p.grouping:
        key = gpu.CudaLweMultiBitBootstrapKey.from_lwe_multi_bit_bootstrap_key(dbsk, n, p.k, p.N, p.pbs_base_log,
                                                                               p.pbs_level, p.grouping, st)
    else:
        key = gpu.CudaLweBootstrapKey.from_lwe_bootstrap_key(dbsk, n, p.k, p.N, p.pbs_base_log, p.pbs_level, st,
                                                             ms_noise_reduction=bool(p.ms_type))
    return dbsk, igpu.CudaDecompressionKey(key, MSG, MSG)


@pytest.mark.parametrize("multi_bit", [False, True], ids=["classic", "multi_bit_g4"])
@pytest.mark.parametrize("kind", BACKENDS)
def test_decompress_word_for_word_and_decrypts(kind, multi_bit):
    """A shuffled-then-sorted subset of indexes spanning three GLWEs: the output blocks equal the oracle bootstrap of the
    restated extracted LWEs, and every one decrypts under the big key to the original message, carry zero, padding bit
    clear.  Classic key and multi-bit g = 4 key (one level, base 2^22: the reference's GPU default shape)."""
    if kind == "emu":
        p, cp = (TOY_MB4_2048 if multi_bit else TOY_2048), ch.TOY_DEC
    else:
        p, cp = (C4G4 if multi_bit else C1), ch.REAL
    lib, st, ck, pksk, comp, gpu, igpu = setup(kind, cp)
    glwe_sk = compute_key()
    dbsk, dec = decompression_key(gpu, igpu, st, cp, ck, p, glwe_sk)
    total = 3 * cp.lwe_per_glwe - 5
    rng = np.random.default_rng(105)
    msgs = rng.integers(0, MSG, size=total)
    enc = orc.Rng(106)
    blocks = np.stack([orc.lwe_encrypt(enc, glwe_sk, (int(m) * p.delta) % (1 << 64), p.glwe_noise) for m in msgs])
    packed = gpu_compress(igpu, comp, blocks, st)
    words, meta = packed.to_host(st)
    assert np.array_equal(words, ch.compress(blocks, ck.pksk, N_IN, cp, MSG))
    # first and last coefficient of every GLWE, the last block of the list, and random ones; shuffled, then sorted
    lpg = cp.lwe_per_glwe
    pick = {0, lpg - 1, lpg, 2 * lpg - 1, 2 * lpg, total - 1} | set(int(i) for i in rng.choice(total, size=18, replace=False))
    indexes = np.array(sorted(rng.permutation(sorted(pick))), dtype=np.uint32)
    assert {int(i) // lpg for i in indexes} == {0, 1, 2}
    out = dec.unpack_indexes(packed, indexes, st)
    got = out.to_blocks(st)[0]
    want = ch.decompress(words, cp, indexes, total, dbsk, p, MSG, MSG)
    assert np.array_equal(got, want)
    decoded = [decode(p, orc.lwe_decrypt(b, glwe_sk)) for b in got]   # value modulo 2 * msg * carry: padding bit kept
    assert decoded == [int(msgs[i]) for i in indexes]
    assert int(out.degrees.max()) == MSG - 1


# ------------------------------------------------------------------------------------------ 5. the Python API, end to end
@pytest.mark.parametrize("kind", BACKENDS)
def test_compressed_list_end_to_end(kind):
    """integer/gpu/list_compression/server_keys.rs tests: results of add_assign / mul_assign (real post-bootstrap noise)
    are compressed, moved through the host, decompressed, decrypted and added."""
    p, keys, st, sks, igpu = radix_setup(kind)
    from tfhe_rs_amd import core_crypto_gpu as gpu
    cp = ch.TOY_DEC if kind == "emu" else ch.REAL
    ck = ch.make_compression_keys(cp, keys.glwe_sk)
    pksk = gpu.CudaLwePackingKeyswitchKey.from_lwe_packing_keyswitch_key(ck.pksk, N_IN, cp.k, cp.N, cp.ks_base_log,
                                                                          cp.ks_level, st)
    comp = igpu.CudaCompressionKey(pksk, cp.lwe_per_glwe, cp.storage_log_modulus, MSG, MSG)
    dbsk, dec = decompression_key(gpu, igpu, st, cp, ck, p, keys.glwe_sk)
    widths = (6, 3, 9) if kind == "emu" else (32, 7, 64)
    rng = np.random.default_rng(107)
    clear, cts = [], []
    for j, L in enumerate(widths):
        mask = (1 << (2 * L)) - 1
        a, b = (int.from_bytes(rng.bytes(16), "little") & mask for _ in range(2))
        ca = igpu.CudaUnsignedRadixCiphertext.from_blocks(encrypt_radix(p, keys, [a], L, 200 + j), st)
        cb = igpu.CudaUnsignedRadixCiphertext.from_blocks(encrypt_radix(p, keys, [b], L, 210 + j), st)
        if kind == "hip" and j == 1:
            sks.mul_assign(ca, cb, st)
            clear.append((a * b) & mask)
        else:
            sks.add_assign(ca, cb, st)
            clear.append((a + b) & mask)
        cts.append(ca)
    packed = igpu.CudaCompressedCiphertextList.compress(cts, comp, st)
    assert len(packed) == 3 and packed.total_blocks == sum(widths)
    words, meta = packed.to_host(st)
    predicted = -(-sum(widths) // cp.lwe_per_glwe) * cp.words_per_glwe * 8
    assert words.size * 8 == predicted == packed.size_bytes()
    plain = sum(widths) * (N_IN + 1) * 8
    print(f"{cp.name}: {sum(widths)} blocks, {plain} bytes -> {predicted} bytes, ratio {plain / predicted:.0f}")
    back = igpu.CudaCompressedCiphertextList.from_host(words, meta, st)
    outs = [back.get(i, dec, st) for i in range(len(back))]
    for o, L, v in zip(outs, widths, clear):
        assert o.num_blocks == L
        rows = decrypt_blocks(p, keys, o.to_blocks(st))
        assert all(d < MSG for d in rows[0])   # carry zero, padding bit clear
        assert recompose(rows) == [v]
    # two decompressed integers added: entry 0 and the low blocks of entry 2
    L0 = widths[0]
    start2 = widths[0] + widths[1]
    low = dec.unpack(back, start2, start2 + L0, st)
    sks.add_assign(outs[0], low, st)
    mask0 = (1 << (2 * L0)) - 1
    assert recompose(decrypt_blocks(p, keys, outs[0].to_blocks(st))) == [(clear[0] + (clear[2] & mask0)) & mask0]
    with pytest.raises(IndexError):
        back.get(3, dec, st)
    # blocks with carries are refused by their degrees
    dirty = igpu.CudaUnsignedRadixCiphertext.from_blocks(encrypt_radix(p, keys, [1], 2, 220), st)
    dirty.set_degrees(2 * MSG - 2)
    with pytest.raises(ValueError, match="empty carries"):
        comp.compress_ciphertexts_into_list([dirty], st)


# ------------------------------------------------------------------------------------------ 6. streams
@pytest.mark.parametrize("kind", BACKENDS)
def test_compress_on_two_streams_with_one_key(kind):
    """Two streams of one GPU compress at once with the same packing key (one cached matrix-core layout, built on the first
    stream): both results equal the single-stream result."""
    cp = ch.TOY_PACK if kind == "emu" else ch.REAL
    lib, st, ck, pksk, comp, gpu, igpu = setup(kind, cp)
    st2 = gpu.CudaStreams([0])
    total = 2 * cp.lwe_per_glwe + 3
    rng = np.random.default_rng(108)
    blocks = [rng.integers(0, 1 << 64, size=(total, N_IN + 1), dtype=U64) for _ in range(2)]
    want = [ch.compress(b, ck.pksk, N_IN, cp, MSG) for b in blocks]
    runs = []
    for s_obj, b in zip((st, st2), blocks):
        s, keep = igpu.CudaServerKey._streams(s_obj)
        ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(b[None], s_obj)
        out = gpu.CudaVec(want[0].size, s_obj)
        mem = C.c_void_p()
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(
            s, C.byref(mem), N_IN, cp.k, cp.N, cp.ks_base_log, cp.ks_level, total, MSG, MSG, cp.lwe_per_glwe,
            cp.storage_log_modulus, True)
        runs.append((s, keep, ct, out, mem, s_obj))
    keys = (C.c_void_p * 1)(pksk.d_vec.ptr)
    for rep in range(2):   # the second round finds the key layout warm on both streams
        for s, keep, ct, out, mem, s_obj in runs:   # both launches are queued before either stream is waited for
            lib.hip_integer_compress_radix_ciphertext_64_async(s, out.ptr, C.byref(ct._ffi()), keys, mem)
        for (s, keep, ct, out, mem, s_obj), w in zip(runs, want):
            assert np.array_equal(out.copy_to_cpu(s_obj), w), rep
    for s, keep, ct, out, mem, s_obj in runs:
        lib.hip_cleanup_integer_compress_radix_ciphertext_64(s, C.byref(mem))
    single = gpu_compress(igpu, comp, blocks[1], st).to_host(st)[0]
    assert np.array_equal(single, want[1])
    print("redzone checks so far:", int(lib.hip_backend_redzone_checks(0)))


# ------------------------------------------------------------------------------------------ 7. refusals
COMP_PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
v = gpu.CudaVec(64 * 4200, st)
mem = C.c_void_p()
bk = ffi.CudaLweBootstrapKeyParamsFFI(32, 1, 2048, 23, 1, 2048, 1, 0)
def radix(blocks, dim, degree=1):
    ct = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec(blocks * (dim + 1), st), 1, blocks, dim)
    ct.set_degrees(degree)
    return ct
def pks_scratch(num):
    lib.hip_scratch_packing_keyswitch_lwe_list_to_glwe_64_async(s, C.byref(mem), 2048, 2, 16, 4, 3, num, True)
def dec_scratch(num):
    lib.hip_scratch_integer_decompress_radix_ciphertext_64_async(s, C.byref(mem), bk, 2, 16, 16, 12, num, 4, 4, True, 0)
idx = lambda *a: (C.c_uint32 * len(a))(*a)
keys = (C.c_void_p * 1)(v.ptr)
"""

REFUSALS = {
    "more LWEs per GLWE than coefficients": ("""
        pks_scratch(20)
        lib.hip_packing_keyswitch_lwe_list_to_glwe_64_async(s, v.ptr, v.ptr, v.ptr, mem, 2048, 2, 16, 4, 3, 20, 17)
        """, "cannot pack more than polynomial_size"),
    "more LWEs than the packing scratch holds": ("""
        pks_scratch(4)
        lib.hip_packing_keyswitch_lwe_list_to_glwe_64_async(s, v.ptr, v.ptr, v.ptr, mem, 2048, 2, 16, 4, 3, 5, 16)
        """, "exceed the scratch capacity"),
    "packing parameters other than the scratch's": ("""
        pks_scratch(4)
        lib.hip_packing_keyswitch_lwe_list_to_glwe_64_async(s, v.ptr, v.ptr, v.ptr, mem, 2048, 2, 16, 4, 2, 4, 4)
        """, "parameters differ from the ones the scratch was created with"),
    "a packing launch on a compression scratch": ("""
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(s, C.byref(mem), 2048, 2, 16, 4, 3, 4, 4, 4, 16, 12, True)
        lib.hip_packing_keyswitch_lwe_list_to_glwe_64_async(s, v.ptr, v.ptr, v.ptr, mem, 2048, 2, 16, 4, 3, 4, 4)
        """, "foreign scratch pointer"),
    "more blocks than the compression scratch holds": ("""
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(s, C.byref(mem), 2048, 2, 16, 4, 3, 4, 4, 4, 16, 12, True)
        lib.hip_integer_compress_radix_ciphertext_64_async(s, v.ptr, C.byref(radix(5, 2048)._ffi()), keys, mem)
        """, "exceed the scratch capacity"),
    "a block with a carry": ("""
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(s, C.byref(mem), 2048, 2, 16, 4, 3, 4, 4, 4, 16, 12, True)
        lib.hip_integer_compress_radix_ciphertext_64_async(s, v.ptr, C.byref(radix(4, 2048, degree=4)._ffi()), keys, mem)
        """, "ciphertexts must have empty carries to be compressed"),
    "blocks of another LWE dimension than the packing key": ("""
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(s, C.byref(mem), 2048, 2, 16, 4, 3, 4, 4, 4, 16, 12, True)
        lib.hip_integer_compress_radix_ciphertext_64_async(s, v.ptr, C.byref(radix(4, 1024)._ffi()), keys, mem)
        """, "do not have the lwe dimension of the packing keyswitch key"),
    "storage modulus of 64 bits": ("""
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(s, C.byref(mem), 2048, 2, 16, 4, 3, 4, 4, 4, 16, 64, True)
        """, "storage_log_modulus 64 must be in 1..63"),
    "compression polynomial size not a power of two": ("""
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(s, C.byref(mem), 2048, 2, 48, 4, 3, 4, 4, 4, 16, 12, True)
        """, "power-of-two polynomial_size"),
    "an index at the list's body count": ("""
        dec_scratch(4)
        lib.hip_integer_decompress_radix_ciphertext_64_async(s, C.byref(radix(4, 2048)._ffi()), v.ptr, 20, idx(3, 20), 2, keys, mem)
        """, "out of bound access"),
    "indexes going back to an earlier GLWE": ("""
        dec_scratch(4)
        lib.hip_integer_decompress_radix_ciphertext_64_async(s, C.byref(radix(4, 2048)._ffi()), v.ptr, 40, idx(17, 3), 2, keys, mem)
        """, "non-decreasing in GLWE index"),
    "more indexes than the decompression scratch holds": ("""
        dec_scratch(2)
        lib.hip_integer_decompress_radix_ciphertext_64_async(s, C.byref(radix(4, 2048)._ffi()), v.ptr, 40, idx(1, 2, 3), 3, keys, mem)
        """, "exceed the scratch capacity"),
    "a decompression key of another input dimension than the compression GLWE": ("""
        lib.hip_scratch_integer_decompress_radix_ciphertext_64_async(s, C.byref(mem), bk, 2, 32, 16, 12, 4, 4, 4, True, 0)
        """, "decompression key's input dimension"),
    "extracting a GLWE past the list": ("""
        lib.hip_integer_extract_glwe_64_async(s, v.ptr, v.ptr, 2, 2, 16, 16, 12, 32)
        """, "out of bound access"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_compression_misuse_aborts_with_a_message(name):
    snippet, message = REFUSALS[name]
    import textwrap
    r = run_child(COMP_PRELUDE + textwrap.dedent(snippet))
    assert r.returncode != 0, f"{name}: the call was accepted"
    assert message in r.stderr, r.stderr[-600:]


def test_size_helper_and_index_order_within_a_glwe():
    """What the header states: the size helper is a pure host function, and the order of the indexes of one call is
    only constrained ACROSS GLWEs (within one they may come in any order)."""
    lib = use_backend("emu")
    assert int(lib.hip_integer_compressed_size_words(4, 256, 256, 12, 256)) == 240
    assert int(lib.hip_integer_compressed_size_words(4, 256, 256, 12, 257)) == 480
    assert int(lib.hip_integer_compressed_size_words(2, 64, 40, 16, 1)) == 42
    p, cp = TOY_2048, ch.TOY_DEC
    lib, st, ck, pksk, comp, gpu, igpu = setup("emu", cp)
    glwe_sk = compute_key()
    dbsk, dec = decompression_key(gpu, igpu, st, cp, ck, p, glwe_sk)
    enc = orc.Rng(110)
    msgs = [i % MSG for i in range(20)]
    blocks = np.stack([orc.lwe_encrypt(enc, glwe_sk, m * p.delta, p.glwe_noise) for m in msgs])
    packed = gpu_compress(igpu, comp, blocks, st)
    words = packed.to_host(st)[0]
    indexes = np.array([5, 3, 17], dtype=np.uint32)
    got = dec.unpack_indexes(packed, indexes, st).to_blocks(st)[0]
    assert np.array_equal(got, ch.decompress(words, cp, indexes, 20, dbsk, p, MSG, MSG))
    assert [decode(p, orc.lwe_decrypt(b, glwe_sk)) for b in got] == [msgs[i] for i in indexes]
