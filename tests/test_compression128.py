"""Compression of squashed-noise (128-bit) ciphertext lists: the u128 packing keyswitch under both kernels, compress,
unpack / extract, the Python API end to end, streams and refusals.  Every integer result is compared WORD FOR WORD with
the NumPy / big-integer restatement of the reference CPU algorithms (tests/compression128_helper.py); there is no
tolerance anywhere.  [emu] runs the kernel sources on the host with the toy sets, [hip] on the MI355X with the toy sets
(which cost nothing there) and, in tests of their own, the three reference sets."""
import ctypes as C
import dataclasses
import textwrap

import numpy as np
import pytest

from . import compression128_helper as ch
from . import pbs128_helper as h
from .common import TOY_2048
from .harness import use_backend
from .test_error_behaviour import run as run_child

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
U64 = np.uint64
M128 = h.M128
AUTO, GENERAL, MATRIX = 0, 1, 2
PATHS = {0: "general kernel", 1: "matrix-core kernel"}


def setup(kind):
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import integer_gpu as igpu
    lib = use_backend(kind)
    return lib, gpu.CudaStreams([0]), gpu, igpu


def upload_key(gpu, st, cp, key):
    return gpu.CudaLwePackingKeyswitchKey128.from_lwe_packing_keyswitch_key(key, cp.n_in, cp.k, cp.N, cp.base_log,
                                                                            cp.level, st)


_random_keys = {}


def random_key(cp, seed=0x6B313238):
    """a key of random words (no word-for-word test needs a key that decrypts), computed once per set"""
    if cp.name not in _random_keys:
        _random_keys[cp.name] = ch.random_words(np.random.default_rng(seed), cp.n_in * cp.level, cp.ncols)
    return _random_keys[cp.name]


def gpu_pack(lib, gpu, pksk, cp, lwes, per, st, mode, max_parts=0):
    d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(lwes, st)
    glwes = (len(lwes) + per - 1) // per
    d_out = gpu.CudaGlweCiphertextList(gpu.CudaVec(glwes * cp.ncols, st, elem_words=2), glwes, cp.k, cp.N)
    lib.hip_backend_set_pks128_kernel(mode)
    lib.hip_backend_set_pks128_max_parts(max_parts)
    try:
        gpu.cuda_keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext_128(pksk, d_in, d_out, st, lwe_per_glwe=per)
    finally:
        lib.hip_backend_set_pks128_kernel(AUTO)
        lib.hip_backend_set_pks128_max_parts(0)
    return d_out.to_glwe_ciphertext_list(st), int(lib.hip_backend_last_pks128_path())


def expected_path(cp, mode):
    return 1 if cp.matrix_ok and mode != GENERAL else 0


def squashed(gpu, igpu, st, blocks, original=None):
    """[blocks][n + 1][2] uint64 -> CudaSquashedNoiseRadixCiphertext"""
    blocks = np.ascontiguousarray(blocks, dtype=U64)
    return igpu.CudaSquashedNoiseRadixCiphertext(gpu.CudaVec.from_cpu_async(blocks.reshape(-1, 2), st, elem_words=2),
                                                 blocks.shape[0], blocks.shape[1] - 1,
                                                 2 * blocks.shape[0] if original is None else original)


# ------------------------------------------------------------------------------------------ 0. the restatement itself
def test_limb_restatement_equals_the_plain_big_integer_one():
    """the float64 limb sums of the helper against one big-integer product per term, on every toy decomposition"""
    rng = np.random.default_rng(99)
    for cp in ch.TOYS:
        key = random_key(cp)
        lwes = ch.random_words(rng, 3, cp.n_in + 1)
        assert np.array_equal(ch.decomposed_products(lwes, key, cp), ch.decomposed_products_plain(lwes, key, cp)), cp.name
    assert [cp.matrix_ok for cp in ch.TOYS] == [True, True, False, True, True]
    assert all(cp.matrix_ok for cp in ch.REFERENCE_SETS)
    assert [cp.digit_bytes for cp in ch.REFERENCE_SETS] == [8, 6, 5]


# ------------------------------------------------------------------------------------------ 1. packing keyswitch
@pytest.mark.parametrize("kind", BACKENDS)
def test_packing_keyswitch_word_for_word(kind):
    """Sets A-E, random-word keys and LWEs; chunk sizes 1, 2, 31, 32, 33 and N_c per GLWE wherever the set's N_c admits them
    (33 needs set E, N_c = 64), two full GLWEs and a partial one per call; automatic, forced-general and
    forced-matrix-core selection with the path that ran asserted.  Set C (K = 80) reaches the general kernel unforced."""
    lib, st, gpu, igpu = setup(kind)
    rng = np.random.default_rng(201)
    for cp in ch.TOYS:
        key = random_key(cp)
        pksk = upload_key(gpu, st, cp, key)
        assert (pksk.d_planes is not None) == cp.matrix_ok
        pers = sorted({p for p in (1, 2, 31, 32, 33, cp.N) if p <= cp.N})
        count_of = {p: 2 * p + max(1, p // 2) for p in pers}
        lwes = ch.random_words(rng, max(count_of.values()), cp.n_in + 1)
        rows = ch.decomposed_products(lwes, key, cp)
        for per in pers:
            count = count_of[per]
            want = ch.pairs_of(ch.packing_keyswitch(lwes[:count], key, cp, per, rows))
            got = {}
            for mode in (AUTO, GENERAL, MATRIX):
                got[mode], path = gpu_pack(lib, gpu, pksk, cp, lwes[:count], per, st, mode)
                print(f"{cp.name}: {count} LWEs, {per} per GLWE, selection {mode}: {PATHS[path]}")
                assert path == expected_path(cp, mode), (cp.name, per, mode, path)
                assert np.array_equal(got[mode], want), (cp.name, per, mode)
            assert np.array_equal(got[GENERAL], got[MATRIX]), (cp.name, per)


@pytest.mark.parametrize("kind", BACKENDS)
def test_packing_keyswitch_on_decomposer_edge_values(kind):
    """Masks made of 0, 2^127, all ones, values exactly half way between two representables and one below / above, and a
    digit equal to +2^(base_log - 1) whose carry goes into the next level.  Set F (base 2^1 x 127 levels) represents 127
    bits: on the all-ones mask the rounding increment would wrap a 128-bit word."""
    lib, st, gpu, igpu = setup(kind)
    rng = np.random.default_rng(202)
    for cp in (ch.SET_A, ch.SET_B, ch.SET_C, ch.SET_D, ch.SET_F):
        key = random_key(cp)
        pksk = upload_key(gpu, st, cp, key)
        rep = cp.base_log * cp.level
        n = cp.n_in
        r = [int.from_bytes(rng.bytes(16), "little") for _ in range(n)]
        masks = [[0] * n, [1 << 127] * n, [M128] * n, r]
        if rep < 128:
            top = [(x >> (128 - rep)) << (128 - rep) for x in r]
            half = 1 << (127 - rep)
            masks += [[(x + half) & M128 for x in top], [(x + half - 1) & M128 for x in top],
                      [(x + half + 1) & M128 for x in top], top,
                      [(x + half) & M128 if j % 2 == 0 else M128 for j, x in enumerate(top)]]
        # the lowest level's digit field holds exactly B / 2: the digit is +-B / 2 and a carry moves up
        carry = (1 << (cp.base_log - 1)) << max(0, 128 - rep)
        assert abs(h.decompose128(carry, cp.base_log, cp.level)[0]) == 1 << (cp.base_log - 1)
        above = max(0, 128 - rep) + cp.base_log   # random higher levels on top of it
        masks += [[carry] * n, [(((x >> above) << above) + carry) & M128 if above < 128 else carry for x in r]]
        bodies = [int.from_bytes(rng.bytes(16), "little") for _ in masks]
        lwes = np.stack([h.to_pairs(m + [b]) for m, b in zip(masks, bodies)])
        want = ch.pairs_of(ch.packing_keyswitch(lwes, key, cp, len(masks)))
        for mode in (AUTO, GENERAL, MATRIX):
            got, path = gpu_pack(lib, gpu, pksk, cp, lwes, len(masks), st, mode)
            print(f"{cp.name}: edge masks, selection {mode}: {PATHS[path]}")
            assert path == expected_path(cp, mode)
            assert np.array_equal(got, want), (cp.name, mode)


# ------------------------------------------------------------------------------------------ 3. accumulator depth
def extreme_digit(base_log, sign):
    """the digit of largest magnitude whose balanced bytes are -128 (sign < 0) or +127 (sign > 0) in every position below
    the top one, the top byte as far out as |d| <= 2^(base_log - 1) allows"""
    J = (base_log + 1 + 7) // 8
    byte = -128 if sign < 0 else 127
    low = sum(byte << (8 * j) for j in range(J - 1))
    bound = 1 << (base_log - 1)
    tops = [t for t in range(-128, 128) if abs(low + (t << (8 * (J - 1)))) < bound]
    return low + ((min(tops) if sign < 0 else max(tops)) << (8 * (J - 1)))


@pytest.mark.parametrize("cp_ref", ch.REFERENCE_SETS, ids=lambda cp: cp.name)
@pytest.mark.parametrize("kind", BACKENDS)
def test_matrix_core_accumulators_at_full_depth(kind, cp_ref):
    """n_in = 4096 on a 1 x 16 GLWE (a 2-4 MB key) with each reference decomposition: the smallest shape at which an int32
    diagonal can overflow.  Digits with byte -128 (and +127) in every position below the top one, the top byte as far out as
    the digit range allows, against key words all 0x00..00 (every re-centred byte -128), all 0xFF..FF (+127) and
    alternating (one column group of the key each): every product of a diagonal has the same sign.  The K split is pinned to ONE share (a batch this small
    would otherwise take 8, and every accumulator would see K / 8 terms), and the reporter is asserted to say so: the whole
    K = 4096 or 8192 goes through one int32 accumulator per diagonal, |acc| above (J - 1) K 2^14 (2^28.8, 2^29.3, 2^29:
    asserted below from the inputs).  The matrix-core path is asserted; the unpinned run and the general kernel must agree."""
    lib, st, gpu, igpu = setup(kind)
    cp = dataclasses.replace(cp_ref, name=cp_ref.name + "_depth", k=1, N=16, lwe_per_glwe=0)
    assert cp.matrix_ok
    rep = cp.base_log * cp.level
    rng = np.random.default_rng(203)
    masks = []
    for sign in (-1, 1):
        d = extreme_digit(cp.base_log, sign)
        state = sum(d << (cp.base_log * idx) for idx in range(cp.level)) & ((1 << rep) - 1)
        x = state << (128 - rep)
        assert h.decompose128(x, cp.base_log, cp.level) == [d] * cp.level
        masks.append([x] * cp.n_in)
    masks.append([int.from_bytes(rng.bytes(16), "little") for _ in range(cp.n_in)])
    lwes = np.stack([h.to_pairs(m + [int.from_bytes(rng.bytes(16), "little")]) for m in masks])
    K = cp.n_in * cp.level
    # one key, three column groups (a column is an accumulator set of its own): words all 0x00..00, all 0xFF..FF, and
    # alternating along K
    key = np.zeros((K, cp.ncols, 2), dtype=U64)
    key[:, 11:22] = 0xFFFFFFFFFFFFFFFF
    key[1::2, 22:] = 0xFFFFFFFFFFFFFFFF
    # the deepest diagonal of the all -128 LWE against an all-zero column: byte j of the digit meets plane s - j, all + 2^14
    J = cp.digit_bytes
    deepest = K * (J - 1) * (1 << 14)
    assert (1 << 28) < deepest < J * K * (1 << 14) < (1 << 31)
    pksk = upload_key(gpu, st, cp, key)
    want = ch.pairs_of(ch.packing_keyswitch(lwes, key, cp, len(masks)))
    got, path = gpu_pack(lib, gpu, pksk, cp, lwes, len(masks), st, AUTO, max_parts=1)
    assert path == 1, "the matrix-core kernel did not run"
    assert int(lib.hip_backend_last_pks128_parts()) == 1, "K was split: no accumulator saw all of it"
    assert np.array_equal(got, want), cp.name
    got_split, path = gpu_pack(lib, gpu, pksk, cp, lwes, len(masks), st, AUTO)
    assert path == 1 and int(lib.hip_backend_last_pks128_parts()) == 8
    assert np.array_equal(got_split, want), cp.name
    got_general, path = gpu_pack(lib, gpu, pksk, cp, lwes, len(masks), st, GENERAL)
    assert path == 0 and np.array_equal(got_general, want), cp.name


# ------------------------------------------------------------------------------------------ 4. compress
COMPRESS_SETS = [
    dataclasses.replace(ch.SET_A, name="toy_A_20_per_glwe_s128", lwe_per_glwe=20, storage_log_modulus=128),
    dataclasses.replace(ch.SET_B, name="toy_B_16_per_glwe_s127", lwe_per_glwe=16, storage_log_modulus=127),
    dataclasses.replace(ch.SET_E, name="toy_E_40_per_glwe_s100", lwe_per_glwe=40, storage_log_modulus=100),
    dataclasses.replace(ch.SET_C, name="toy_C_7_per_glwe_s100", lwe_per_glwe=7, storage_log_modulus=100),
]


def compression_key(gpu, igpu, st, cp, key):
    pksk = upload_key(gpu, st, cp, key)
    return igpu.CudaNoiseSquashingCompressionKey(pksk, cp.per, 4, 4, storage_log_modulus=cp.storage_log_modulus)


@pytest.mark.parametrize("kind", BACKENDS)
def test_compress_word_for_word(kind):
    """pack, modulus switch, bit-pack: 1, lwe_per_glwe, lwe_per_glwe + 1 and 3 lwe_per_glwe - 5 blocks; fewer LWEs per GLWE
    than coefficients; 128 stored bits (the production value: the switch is the identity), 127, and 100 (values straddle
    words); the padding bits of every GLWE's last word are zero."""
    lib, st, gpu, igpu = setup(kind)
    rng = np.random.default_rng(204)
    for cp in COMPRESS_SETS:
        key = random_key(cp)
        comp = compression_key(gpu, igpu, st, cp, key)
        most = 3 * cp.per - 5
        blocks = ch.random_words(rng, most, cp.n_in + 1)
        rows = ch.decomposed_products(blocks, key, cp)
        for total in (1, cp.per, cp.per + 1, most):
            packed = comp.compress_noise_squashed_ciphertexts_into_list([squashed(gpu, igpu, st, blocks[:total])], st)
            words, meta = packed.to_host(st)
            want = ch.compress(blocks[:total], key, cp, rows)
            glwes = -(-total // cp.per)
            assert words.shape == want.shape == (glwes * cp.words_per_glwe, 2)
            assert words.shape[0] == int(lib.hip_integer_compressed_size_words_128(cp.k, cp.N, cp.per,
                                                                                   cp.storage_log_modulus, total))
            assert np.array_equal(words, want), (cp.name, total)
            used = cp.values_per_glwe * cp.storage_log_modulus % 128
            assert (used != 0) == (cp.storage_log_modulus != 128)
            if used:   # the padding bits of the last word of every GLWE
                last = h.from_pairs(words.reshape(glwes, cp.words_per_glwe, 2)[:, -1])
                assert not any(v >> used for v in last), (cp.name, total)


# ------------------------------------------------------------------------------------------ 5. unpack / extract
def gpu_extract_glwe(lib, gpu, igpu, st, cp, words, glwe_index, total):
    s, keep = igpu.CudaServerKey._streams(st)
    d_words = gpu.CudaVec.from_cpu_async(np.ascontiguousarray(words, dtype=U64).reshape(-1, 2), st, elem_words=2)
    d_out = gpu.CudaVec(cp.ncols, st, elem_words=2)
    lib.hip_integer_extract_glwe_128_async(s, d_out.ptr, d_words.ptr, glwe_index, cp.k, cp.N, cp.per,
                                           cp.storage_log_modulus, total)
    return d_out.copy_to_cpu(st)


@pytest.mark.parametrize("kind", BACKENDS)
def test_unpack_and_extract_round_trip(kind):
    """Restated compress on the host -> from_host -> the device's unpack + sample extract against the restated extract():
    every index of the partial last GLWE, both ends of every full one and random ones; the unpacked-GLWE entry; the body
    tail zeroed; random s-bit values packed on the host come back as they were."""
    lib, st, gpu, igpu = setup(kind)
    rng = np.random.default_rng(205)
    for cp in COMPRESS_SETS:
        key = random_key(cp)
        total = 3 * cp.per - 5
        blocks = ch.random_words(rng, total, cp.n_in + 1)
        words = ch.compress(blocks, key, cp)
        meta = {"block_counts": [total], "original_block_counts": [2 * total], "glwe_dimension": cp.k,
                "polynomial_size": cp.N, "lwe_per_glwe": cp.per, "storage_log_modulus": cp.storage_log_modulus,
                "message_modulus": 4, "carry_modulus": 4}
        packed = igpu.CudaCompressedSquashedNoiseCiphertextList.from_host(words, meta, st)
        pick = {0, cp.per - 1, cp.per, 2 * cp.per - 1} | set(range(2 * cp.per, total))
        pick |= set(int(i) for i in rng.choice(total, size=min(6, total), replace=False))
        indexes = np.array(sorted(pick), dtype=np.uint32)
        out = packed.unpack_indexes(indexes, st)
        assert out.lwe_dimension == cp.k * cp.N and out.num_blocks == len(indexes)
        assert np.array_equal(out.to_blocks(st), ch.extract_lwes(words, cp, indexes, total)), cp.name
        for g in range(3):
            got = gpu_extract_glwe(lib, gpu, igpu, st, cp, words, g, total)
            assert np.array_equal(got, h.to_pairs(ch.extract_glwe(words, cp, g, total))), (cp.name, g)
        tail = got[cp.k * cp.N + cp.per - 5:]
        assert tail.shape[0] == cp.N - cp.per + 5 and not tail.any()   # the partial last GLWE's body tail
        s = cp.storage_log_modulus
        vals = [int.from_bytes(rng.bytes(16), "little") >> (128 - s) for _ in range(cp.values_per_glwe)]
        got = gpu_extract_glwe(lib, gpu, igpu, st, cp, ch.bit_pack128(vals, s), 0, cp.per)
        assert [v >> (128 - s) for v in h.from_pairs(got[:cp.values_per_glwe])] == vals
        assert ch.bit_unpack128(ch.bit_pack128(vals, s), s, len(vals)) == vals


# ------------------------------------------------------------------------------------------ 6. end to end, real keys
# The compute set TOY_2048, the toy squashing key of tests/test_pbs128.py (k = 1, N = 512: squashed blocks of dimension 512)
# and a REAL packing key from that dimension to set A's compression GLWE (1 x 32, base 2^61 x 1 level, noise TUniform 2^30),
# stored on 128 bits.  A squashed block carries its 4 message bits below the padding bit: delta = 2^123, decoding rounds at
# 2^122.  WORST-CASE bound on what the packing adds to a block's phase, binary keys:
#   decomposition rounding     512 mask elements * 2^(127 - 61)                                       = 2^75
#   packing key noise          every one of up to 32 LWEs of a GLWE leaves 512 digits (< 2^60) * 2^30 in EVERY coefficient
#                              of the body polynomial and k N = 32 key bits fold the mask noise in:  32 * 33 * 2^99 < 2^110
#   modulus switch             none at 128 bits
# far below the 2^122 - (squashing output error < 2^110, tests/test_pbs128.py) the decoding leaves.
E2E_COMP = dataclasses.replace(ch.SET_A, name="e2e_n512_k1_N32_b61_l1", n_in=512, lwe_per_glwe=4)
# and to set B's (2 x 16, base 2^33 x 2 levels): the pairing of digit idx with key row idx, which one level cannot show.
#   decomposition rounding     512 * 2^(127 - 66)                                                     = 2^70
#   packing key noise          up to 16 LWEs, 1024 digits (< 2^32) * 2^30 each, 33 key bits:          16 * 33 * 2^72 < 2^82
E2E_COMP_B = dataclasses.replace(ch.SET_B, name="e2e_n512_k2_N16_b33_l2", n_in=512, lwe_per_glwe=4)


@pytest.mark.parametrize("kind", BACKENDS)
def test_squash_compress_unpack_decrypt_end_to_end(kind):
    """squash -> builder.push -> build -> (host and back) -> get -> decrypt: every block returns the two packed messages of
    its pair; the compressed size is what hip_integer_compressed_size_words_128 says."""
    from .test_pbs128 import TOY_SQUASH, upload_key as upload_squashing_key
    from .test_radix_integer import encrypt_radix
    from .test_radix_integer import setup as radix_setup
    p, ckeys, st, sks, igpu = radix_setup(kind)
    assert p is TOY_2048 or kind == "hip"
    from tfhe_rs_amd import core_crypto_gpu as gpu
    lib = use_backend(kind)
    sp = TOY_SQUASH if kind == "emu" else h.Params128(f"toy128_squash_k1_N512_n{p.n}", p.n, 1, 512, 24, 3, ms_type=1)
    skeys = h.make_keys128(sp, compute=p)
    nsk = igpu.CudaNoiseSquashingKey(upload_squashing_key(gpu, st, sp, skeys), 4, 4)
    cases = ((5, 0b1110010011), (4, 0b10110001), (1, 0b10))
    squashed_cts = []
    for blocks, value in cases:
        ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(encrypt_radix(p, ckeys, [value], blocks, seed=300 + blocks), st)
        ct.set_degrees(3)
        squashed_cts.append(igpu.squash_radix_ciphertext_noise(nsk, sks, ct, st))
    total = sum((b + 1) // 2 for b, _ in cases)
    for cp in (E2E_COMP, E2E_COMP_B):
        assert cp.n_in == sp.k * sp.N
        comp_sk = ch.compression_secret_key(cp)
        key = ch.gen_pksk128(0x706B3132, skeys.glwe_sk, comp_sk, cp)
        comp = compression_key(gpu, igpu, st, cp, key)
        builder = igpu.CudaCompressedSquashedNoiseCiphertextList.builder()
        for ct in squashed_cts:
            builder.push(ct)
        packed = builder.build(comp, st)
        assert int(lib.hip_backend_last_pks128_path()) == 1
        assert len(packed) == 3 and packed.total_blocks == total == 6   # two GLWEs of 4, the second partial
        words, meta = packed.to_host(st)
        predicted = int(lib.hip_integer_compressed_size_words_128(cp.k, cp.N, cp.per, cp.storage_log_modulus, total))
        assert words.shape[0] == predicted and packed.size_bytes() == 16 * predicted
        plain = total * (cp.n_in + 1) * 16
        print(f"{cp.name}: {total} squashed blocks, {plain} bytes -> {16 * predicted} bytes")
        back = igpu.CudaCompressedSquashedNoiseCiphertextList.from_host(words, meta, st)
        for i, (blocks, value) in enumerate(cases):
            out = back.get(i, st)
            assert out.num_blocks == (blocks + 1) // 2 and out.original_block_count == blocks
            assert out.lwe_dimension == cp.k * cp.N
            digits = [(value >> (2 * j)) & 3 for j in range(blocks)] + [0]
            want = [digits[2 * j] + 4 * digits[2 * j + 1] for j in range(out.num_blocks)]
            assert [h.decode128(ch.phase(b, comp_sk)) for b in out.to_blocks(st)] == want, (cp.name, i)
        with pytest.raises(IndexError):
            back.get(3, st)


# ------------------------------------------------------------------------------------------ 7. streams, refusals
@pytest.mark.parametrize("kind", BACKENDS)
def test_compress_on_two_streams_with_one_key(kind):
    """Two streams of one GPU compress at once with the same key (both layouts, converted once at upload): both results
    equal the restated words, twice."""
    lib, st, gpu, igpu = setup(kind)
    cp = COMPRESS_SETS[2]
    key = random_key(cp)
    pksk = upload_key(gpu, st, cp, key)
    st2 = gpu.CudaStreams([0])
    total = 2 * cp.per + 3
    rng = np.random.default_rng(207)
    blocks = [ch.random_words(rng, total, cp.n_in + 1) for _ in range(2)]
    want = [ch.compress(b, key, cp) for b in blocks]
    runs = []
    for s_obj, b in zip((st, st2), blocks):
        s, keep = igpu.CudaServerKey._streams(s_obj)
        ct = squashed(gpu, igpu, s_obj, b)
        out = gpu.CudaVec(want[0].shape[0], s_obj, elem_words=2)
        mem = C.c_void_p()
        lib.hip_scratch_integer_compress_radix_ciphertext_128_async(
            s, C.byref(mem), cp.n_in, cp.k, cp.N, cp.base_log, cp.level, total, 4, 4, cp.per, cp.storage_log_modulus, True)
        runs.append((s, keep, ct, out, mem, s_obj))
    st.synchronize_one(0)   # the key conversion ran on the first stream
    keys, planes = (C.c_void_p * 1)(pksk.d_vec.ptr), (C.c_void_p * 1)(pksk.planes_ptr)
    for rep in range(2):
        for s, keep, ct, out, mem, s_obj in runs:   # both launches are queued before either stream is waited for
            lib.hip_integer_compress_radix_ciphertext_128_async(s, out.ptr, C.byref(ct._ffi()), keys, planes, mem)
        for (s, keep, ct, out, mem, s_obj), w in zip(runs, want):
            assert np.array_equal(out.copy_to_cpu(s_obj), w), rep
    for s, keep, ct, out, mem, s_obj in runs:
        lib.hip_cleanup_integer_compress_radix_ciphertext_128(s, C.byref(mem))


COMP_PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
v = gpu.CudaVec(64 * 4200, st)
mem = C.c_void_p()
def radix(blocks, dim):
    return igpu.CudaSquashedNoiseRadixCiphertext(gpu.CudaVec(blocks * (dim + 1), st, elem_words=2), blocks, dim, 2 * blocks)
def pks_scratch(num, base_log=33, level=2):
    lib.hip_scratch_packing_keyswitch_lwe_list_to_glwe_128_async(s, C.byref(mem), 64, 2, 16, base_log, level, num, True)
def pks(num, per, level=2, lwes=v.ptr):
    lib.hip_packing_keyswitch_lwe_list_to_glwe_128_async(s, v.ptr, lwes, v.ptr, None, mem, 64, 2, 16, 33, level, num, per)
def comp_scratch(num, bits=128):
    lib.hip_scratch_integer_compress_radix_ciphertext_128_async(s, C.byref(mem), 64, 2, 16, 33, 2, num, 4, 4, 16, bits, True)
def dec_scratch(num):
    lib.hip_scratch_integer_decompress_radix_ciphertext_128_async(s, C.byref(mem), 2, 16, 16, 128, num, 4, 4, True)
def dec(total, *indexes, out_dim=32):
    a = (C.c_uint32 * len(indexes))(*indexes)
    lib.hip_integer_decompress_radix_ciphertext_128_async(s, C.byref(radix(4, out_dim)._ffi()), v.ptr, total, a, len(indexes), mem)
keys = (C.c_void_p * 1)(v.ptr)
"""

REFUSALS = {
    "a null input pointer": ("pks_scratch(4); pks(4, 4, lwes=None)", "null pointer"),
    "a null scratch": ("pks(4, 4)", "foreign scratch pointer"),
    "packing parameters other than the scratch's": ("pks_scratch(4); pks(4, 4, level=1)",
                                                    "parameters differ from the ones the scratch was created with"),
    "more LWEs than the packing scratch holds": ("pks_scratch(4); pks(5, 16)", "exceed the scratch capacity"),
    "more LWEs per GLWE than coefficients": ("pks_scratch(20); pks(20, 17)", "cannot pack more than polynomial_size"),
    "a decomposition wider than the word": ("pks_scratch(4, 33, 4)", "exceeds the 128 bits of a word"),
    "a base above 2^62": ("pks_scratch(4, 63, 1)", "above 62"),
    "a packing launch on a compression scratch": ("comp_scratch(4); pks(4, 4)", "foreign scratch pointer"),
    "storage modulus of 129 bits": ("comp_scratch(4, 129)", "storage_log_modulus 129 must be in 1..128"),
    "storage modulus of 0 bits": ("comp_scratch(4, 0)", "storage_log_modulus 0 must be in 1..128"),
    "more blocks than the compression scratch holds": ("""
        comp_scratch(4)
        lib.hip_integer_compress_radix_ciphertext_128_async(s, v.ptr, C.byref(radix(5, 64)._ffi()), keys, None, mem)
        """, "exceed the scratch capacity"),
    "blocks of another LWE dimension than the packing key": ("""
        comp_scratch(4)
        lib.hip_integer_compress_radix_ciphertext_128_async(s, v.ptr, C.byref(radix(4, 32)._ffi()), keys, None, mem)
        """, "do not have the lwe dimension of the packing keyswitch key"),
    "an index at the list's body count": ("dec_scratch(4); dec(20, 3, 20)", "out of bound access"),
    "indexes going back to an earlier GLWE": ("dec_scratch(4); dec(40, 17, 3)", "non-decreasing in GLWE index"),
    "more indexes than the decompression scratch holds": ("dec_scratch(2); dec(40, 1, 2, 3)", "exceed the scratch capacity"),
    "output blocks of another dimension than the compression GLWE": ("dec_scratch(4); dec(40, 1, out_dim=64)",
                                                                     "the compression GLWE extracts to 32"),
    "extracting a GLWE past the list": ("lib.hip_integer_extract_glwe_128_async(s, v.ptr, v.ptr, 2, 2, 16, 16, 128, 32)",
                                        "out of bound access"),
    "converting a key the matrix-core kernel declines": (
        "lib.hip_convert_lwe_packing_keyswitch_key_128_async(s, v.ptr, v.ptr, 40, 1, 32, 41, 2)",
        "does not carry this shape"),
    "a kernel selection that does not exist": ("lib.hip_backend_set_pks128_kernel(3)", "is not 0 (automatic)"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_compression128_misuse_aborts_with_a_message(name):
    snippet, message = REFUSALS[name]
    r = run_child(COMP_PRELUDE + textwrap.dedent(snippet).replace("; ", "\n"))
    assert r.returncode != 0, f"{name}: the call was accepted"
    assert message in r.stderr, r.stderr[-600:]


def test_size_helpers():
    """pure host functions: the packed size in u128 words and the size of the key's byte planes (0: declined shape)"""
    lib = use_backend("emu")
    assert int(lib.hip_integer_compressed_size_words_128(6, 1024, 128, 128, 128)) == 6 * 1024 + 128
    assert int(lib.hip_integer_compressed_size_words_128(6, 1024, 128, 128, 129)) == 2 * (6 * 1024 + 128)
    assert int(lib.hip_integer_compressed_size_words_128(2, 16, 16, 100, 1)) == (48 * 100 + 127) // 128
    for cp in ch.TOYS + ch.REFERENCE_SETS:
        planes = int(lib.hip_lwe_packing_keyswitch_key_128_planes_size_bytes(cp.n_in, cp.k, cp.N, cp.base_log, cp.level))
        assert (planes != 0) == cp.matrix_ok, cp.name
        if planes and cp.ncols % 32 == 0:
            assert planes == 16 * cp.n_in * cp.level * cp.ncols   # as many bytes as the key itself
    # J K 2^14 >= 2^31: 8 bytes x 16384 x 2^14 = 2^31 is declined, 8192 is carried
    assert int(lib.hip_lwe_packing_keyswitch_key_128_planes_size_bytes(8192, 1, 16, 61, 2)) == 0
    assert int(lib.hip_lwe_packing_keyswitch_key_128_planes_size_bytes(8192, 1, 16, 61, 1)) != 0


def test_bench_tool_runs_end_to_end_on_the_host_emulation():
    """tools/bench_compression128.py --toy against the emulation library: every call the tool makes (key upload and
    conversion, compress under the three selections, unpack, the key copy) goes through with its real argument list and
    the JSON line comes out.  The figures mean nothing here."""
    import json
    import os
    import subprocess
    import sys
    from .harness import EMU_LIB, build_emu
    build_emu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFHE_HIP_BACKEND_LIB=EMU_LIB)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_compression128.py"), "--toy"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])["toy_b33_l2"]
    assert out["matrix_planes"] and out["key_copy_ms"] > 0
    assert [out["compress_40"][sel]["path"] for sel in ("auto", "general", "matrix")] == [1, 0, 1]
    assert out["compress_40"]["packed_bytes"] == 3 * (64 + 16) * 16 and out["unpack_3"]["ms"] > 0


# ------------------------------------------------------------------------------------------ 8. the reference sets
def fixed_values(cp):
    return [0, 1, 31, 32, 33, cp.N - 1, cp.N, cp.k * cp.N - 1, cp.k * cp.N, cp.k * cp.N + 1, cp.k * cp.N + 127,
            cp.values_per_glwe - 1]


@pytest.mark.gpu
@pytest.mark.parametrize("cp", ch.REFERENCE_SETS, ids=lambda cp: cp.name)
def test_reference_set_on_the_device(cp):
    """n_in = 4096, N_c = 1024, a random-word key (470-940 MB), 129 LWEs at 128 per GLWE: one full GLWE and one of a single
    LWE, stored on 128 bits.  Restating all 7168 values of a GLWE is too slow on the CPU: a fixed subset per GLWE, across
    all its LWEs, is compared word for word (the values named by the issue and 12 seeded random ones).  The matrix-core
    path is asserted, and the general kernel must give the same packed words everywhere."""
    lib, st, gpu, igpu = setup("hip")
    rng = np.random.default_rng(208)
    key = ch.random_words(rng, cp.n_in * cp.level, cp.ncols)
    comp = compression_key(gpu, igpu, st, cp, key)
    total = 129
    blocks = ch.random_words(rng, total, cp.n_in + 1)
    ct = squashed(gpu, igpu, st, blocks)
    packed = comp.compress_noise_squashed_ciphertexts_into_list([ct], st)
    assert int(lib.hip_backend_last_pks128_path()) == 1, "the matrix-core kernel did not run"
    words = packed.to_host(st)[0]
    assert words.shape[0] == 2 * cp.values_per_glwe
    values = fixed_values(cp) + sorted(int(v) for v in rng.choice(cp.values_per_glwe, size=12, replace=False))
    got = np.array(h.from_pairs(words), dtype=object).reshape(2, cp.values_per_glwe)   # s = 128: a word is a value
    for g, (first, count) in enumerate(((0, 128), (128, 1))):
        want = ch.glwe_values(blocks, key, cp, first, count, values)
        assert [got[g][v] for v in values] == want, (cp.name, g)
    lib.hip_backend_set_pks128_kernel(GENERAL)
    try:
        general = comp.compress_noise_squashed_ciphertexts_into_list([ct], st).to_host(st)[0]
    finally:
        lib.hip_backend_set_pks128_kernel(AUTO)
    assert int(lib.hip_backend_last_pks128_path()) == 0
    assert np.array_equal(general, words)
