"""Re-randomisation of radix blocks (hip_*_rerand_64): the fused rotate-and-add kernel word for word against the NumPy
restatement of the expansion (tests/expand_helper.py), the keyswitch mode word for word against the oracle's keyswitch of
the expanded zeros, decryption on real keys in both modes, device against host emulation, refusals, the size query and
the prototypes of the six new entry points (re-randomisation and OPRF) against the reference's headers.  [emu] runs the
kernel sources on the host with toy keys, [hip] on the MI355X, there also with PARAM_MESSAGE_2_CARRY_2."""
import ctypes as C
import functools
import os
import textwrap

import numpy as np
import pytest

from . import expand_helper as eh
from . import oracle as orc
from .common import C1, TOY_2048, TOY_MB4_2048, decrypt_big, encrypt_big, make_keys
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_integer import setup as radix_setup

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
U64 = np.uint64
M64 = (1 << 64) - 1
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
RERAND_WITH_KS, RERAND_WITHOUT_KS = 0, 1         # integer/integer.h:45
SENTINEL = 0xD1D1D1D1D1D1D1D1


def rerand_abi(kind, blocks, zeros, n_in, *, ksk=None, shape=(0, 0, 0), allocate=True):
    """hip_scratch_rerand / hip_rerand / hip_cleanup_rerand on `blocks` ([count][n + 1]) followed by a sentinel row;
    returns the blocks, the sentinel row and the zero list as they are after the call.  `ksk`: the host keyswitch key
    ([n_in][level][n_out + 1]) with shape = (n_out, base_log, level), or None for RERAND_WITHOUT_KS."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import ffi
    from tfhe_rs_amd import integer_gpu as igpu
    lib = use_backend(kind)
    st = gpu.CudaStreams([0])
    s, keep = igpu.CudaServerKey._streams(st)
    count, w = blocks.shape
    d_blocks = gpu.CudaVec.from_cpu_async(np.concatenate([blocks.reshape(-1), np.full(w, SENTINEL, dtype=U64)]), st)
    d_zeros = gpu.CudaVec.from_cpu_async(zeros, st)
    keys, d_key = None, None
    if ksk is not None:
        d_key = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(ksk, n_in, shape[0], shape[1], shape[2], st)
        keys = (C.c_void_p * 1)(d_key.d_vecs[0].ptr)
    mem = C.c_void_p()
    lib.hip_scratch_rerand_64_async(s, C.byref(mem), ffi.CudaLweKeyswitchKeyParamsFFI(n_in, *shape), count, 4, 4, allocate,
                                    RERAND_WITHOUT_KS if ksk is None else RERAND_WITH_KS)
    lib.hip_rerand_64_async(s, d_blocks.ptr, d_zeros.ptr, mem, keys)
    lib.hip_cleanup_rerand_64(s, C.byref(mem))
    assert not mem.value
    got = d_blocks.copy_to_cpu(st).reshape(count + 1, w)
    return got[:count], got[count], d_zeros.copy_to_cpu(st)


# ------------------------------------------------------------------------------------------ 1. the fused kernel
KERNEL_CASES = {
    "n2048_1_block": (2048, 1),          # rotation 0 alone
    "n2048_2_blocks": (2048, 2),
    "n2048_2047_blocks": (2048, 2047),
    "n2048_2048_blocks": (2048, 2048),   # the full list: the last row wraps on every word but one
    "n8_8_blocks": (8, 8),               # below one chunk
    "n12_12_blocks": (12, 12),           # not a power of two
    "n1025_1025_blocks": (1025, 1025),   # rows of 1026 words: one word into their second chunk
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
@pytest.mark.parametrize("kind", BACKENDS)
def test_fused_kernel_word_for_word(kind, case):
    n, count = KERNEL_CASES[case]
    rng = np.random.default_rng(301)
    blocks = rng.integers(0, 1 << 64, size=(count, n + 1), dtype=U64)
    zeros = rng.integers(0, 1 << 64, size=n + count, dtype=U64)
    got, guard, zeros_after = rerand_abi(kind, blocks, zeros, n)
    want = blocks + eh.expand(zeros, n, [count])          # modulo 2^64: NumPy's unsigned arithmetic wraps
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"rows {bad[:8]} differ"
    assert (guard == U64(SENTINEL)).all(), "written past the last block"
    assert np.array_equal(zeros_after, zeros), "the zero list was written"


@pytest.mark.parametrize("kind", BACKENDS)
def test_fused_kernel_wraps_on_edge_masks(kind):
    """Masks of 0, 2^64 - 1 and 2^63 (-0 = 0, -(2^64 - 1) = 1, 2^63 its own negation) on blocks of 2^64 - 1, so that the
    sums carry out of the word."""
    n, count = 2048, 2048
    rng = np.random.default_rng(302)
    blocks = np.full((count, n + 1), M64, dtype=U64)
    for value in (0, M64, 1 << 63):
        zeros = np.concatenate([np.full(n, value, dtype=U64), rng.integers(0, 1 << 64, size=count, dtype=U64)])
        got, guard, zeros_after = rerand_abi(kind, blocks, zeros, n)
        assert np.array_equal(got, blocks + eh.expand(zeros, n, [count])), hex(value)
        # row 0 adds the mask as it is, the last row its negation on every word but the last of the mask
        assert int(got[0][0]) == (M64 + value) & M64 and int(got[count - 1][0]) == (M64 - value) & M64
        assert (guard == U64(SENTINEL)).all() and np.array_equal(zeros_after, zeros)


# ------------------------------------------------------------------------------------------ 2. keyswitch mode
@functools.lru_cache(maxsize=2)
def uniform_ksk(n_in, n_out, level):
    """Uniform words in the keyswitch key's layout [n_in][level][n_out + 1]: the sums are exact integer sums whatever
    the key holds."""
    return np.random.default_rng(303).integers(0, 1 << 64, size=n_in * level * (n_out + 1), dtype=U64)


KS_CASES = {
    "n1024_to_2048_1x24_count_4": (1024, 2048, 24, 1, 4),
    "n2048_to_2048_4x4_count_1": (2048, 2048, 4, 4, 1),
    "n2048_to_2048_4x4_count_33": (2048, 2048, 4, 4, 33),   # crosses a 32-sample tile of the matrix-core keyswitch
}


@pytest.mark.parametrize("case", list(KS_CASES))
@pytest.mark.parametrize("kind", BACKENDS)
def test_keyswitch_mode_word_for_word(kind, case):
    n_in, n_out, base_log, level, count = KS_CASES[case]
    rng = np.random.default_rng(304)
    blocks = rng.integers(0, 1 << 64, size=(count, n_out + 1), dtype=U64)
    zeros = rng.integers(0, 1 << 64, size=n_in + count, dtype=U64)
    ksk = uniform_ksk(n_in, n_out, level)
    got, guard, zeros_after = rerand_abi(kind, blocks, zeros, n_in, ksk=ksk, shape=(n_out, base_log, level))
    want = blocks + orc.keyswitch_batch(eh.expand(zeros, n_in, [count]), ksk, n_in, n_out, base_log, level)
    assert np.array_equal(got, want)
    assert (guard == U64(SENTINEL)).all() and np.array_equal(zeros_after, zeros)


# ------------------------------------------------------------------------------------------ 3. decryption on real keys
N_PKE = 1024          # the dedicated compact public key of the keyswitch mode; one level of 24 bits to the big key
VALUES = [0, 3, 1, 2]


@functools.lru_cache(maxsize=4)
def host_rerand_ksk(p):
    return eh.casting_key(0x7265726E, eh.pke_key(N_PKE), make_keys(p).glwe_sk, 24, 1, p.glwe_noise)


def rerand_key_and_zeros(p, keys, igpu, st, mode, blocks, seed):
    """(CudaReRandomizationKey, one compact list of `blocks` encryptions of zero) of a mode, through the Python mirror"""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    if mode == "with_ks":
        ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(host_rerand_ksk(p), N_PKE, p.big_n, 24, 1, st)
        key, sk = igpu.CudaReRandomizationKey(N_PKE, ksk), eh.pke_key(N_PKE)
    else:
        key, sk = igpu.CudaReRandomizationKey(p.big_n), keys.glwe_sk
    words = eh.make_compact_list(sk, [0] * blocks, seed)
    return key, gpu.CudaLweCompactCiphertextList.from_flat_words(words, len(sk), [blocks], st)


DECRYPT_CASES = [pytest.param("emu", TOY_2048, id="emu-toy_classic"), pytest.param("emu", TOY_MB4_2048, id="emu-toy_multi_bit_g4"),
                 pytest.param("hip", TOY_2048, id="hip-toy_classic", marks=pytest.mark.gpu),
                 pytest.param("hip", TOY_MB4_2048, id="hip-toy_multi_bit_g4", marks=pytest.mark.gpu),
                 pytest.param("hip", C1, id="hip-message_2_carry_2", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("mode", ["without_ks", "with_ks"])
@pytest.mark.parametrize("kind,p", DECRYPT_CASES)
def test_re_randomized_blocks_decrypt_and_differ(kind, p, mode):
    p, keys, st, sks, igpu = radix_setup(kind, p)
    fresh = encrypt_big(p, keys, VALUES, seed=31).reshape(1, 4, -1)
    outs = []
    for seed in (305, 306):           # two different zero lists
        ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(fresh, st)
        ct.set_degrees(3)
        key, zeros = rerand_key_and_zeros(p, keys, igpu, st, mode, 4, seed)
        ct.re_randomize(zeros, key, st)
        out = ct.to_blocks(st)[0]
        assert [decrypt_big(p, keys, b) for b in out] == VALUES
        assert (out != fresh[0]).all(), "a word of a block survived the re-randomisation"
        assert list(ct.degrees) == [3] * 4 and list(ct._info[1]) == [1] * 4
        outs.append(out)
    assert (outs[0] != outs[1]).all(), "two zero lists gave the same words"
    # the re-randomised integer is an ordinary radix ciphertext: the identity table bootstraps it
    identity = orc.generate_lut(p.k, p.N, 16, p.delta, lambda x: x)
    after = sks.apply_lookup_table(ct, identity, st, degree=3).to_blocks(st)[0]
    assert [decrypt_big(p, keys, b) for b in after] == VALUES


# ------------------------------------------------------------------------------------------ 4. device = emulation
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["without_ks", "with_ks"])
def test_device_equals_emulation_word_for_word(mode):
    p, keys = TOY_2048, make_keys(TOY_2048)
    blocks = encrypt_big(p, keys, VALUES, seed=32)
    if mode == "with_ks":
        args = dict(ksk=host_rerand_ksk(p), shape=(p.big_n, 24, 1))
        zeros, n_in = eh.make_compact_list(eh.pke_key(N_PKE), [0] * 4, 307), N_PKE
    else:
        args = {}
        zeros, n_in = eh.make_compact_list(keys.glwe_sk, [0] * 4, 307), p.big_n
    out, _, _ = rerand_abi("hip", blocks, zeros, n_in, **args)
    try:
        emu, _, _ = rerand_abi("emu", blocks, zeros, n_in, **args)
    finally:
        use_backend("hip")
    assert np.array_equal(emu, out)
    assert [decrypt_big(p, keys, b) for b in out] == VALUES


# ------------------------------------------------------------------------------------------ 5. refusals
RERAND_PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
v = gpu.CudaVec(16 * 2049, st)
mem = C.c_void_p()
KK = ffi.CudaLweKeyswitchKeyParamsFFI
def scratch(count, n=2048, mode=1, allocate=True, shape=(0, 0, 0)):
    return lib.hip_scratch_rerand_64_async(s, C.byref(mem), KK(n, *shape), count, 4, 4, allocate, mode)
def radix(blocks, n=2048):
    return igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec(blocks * (n + 1), st), 1, blocks, n)
def zero_list(blocks, n=2048):
    return gpu.CudaLweCompactCiphertextList(gpu.CudaVec(n + blocks, st), n, [blocks])
"""

REFUSALS = {
    "count 0": ("scratch(0)", "rerand: no ciphertext to re-randomise"),
    "count above the dimension": ("scratch(9, n=8)", "rerand: 9 ciphertexts, one compact list of encryptions of zero holds 1 .. 8"),
    "a launch on a size-only scratch": ("""
        scratch(2, allocate=False)
        lib.hip_rerand_64_async(s, v.ptr, v.ptr, mem, None)
        """, "rerand: scratch was created with allocate_gpu_memory=false"),
    "a launch on a scratch of another kind": ("""
        lib.hip_scratch_packing_keyswitch_lwe_list_to_glwe_64_async(s, C.byref(mem), 2048, 2, 16, 4, 3, 4, True)
        lib.hip_rerand_64_async(s, v.ptr, v.ptr, mem, None)
        """, "rerand: foreign scratch pointer"),
    "a null key in keyswitch mode": ("""
        scratch(2, n=8, mode=0, shape=(12, 4, 4))
        lib.hip_rerand_64_async(s, v.ptr, v.ptr, mem, None)
        """, "rerand: RERAND_WITH_KS without a keyswitch key"),
    "a block above nominal noise": ("""
        ct = radix(2)
        ct._info[1][1] = 2
        ct.re_randomize(zero_list(2), igpu.CudaReRandomizationKey(2048), st)
        """, "Tried to re-randomize a Ciphertext with non-nominal NoiseLevel"),
    "a public key of another dimension than the blocks": ("""
        radix(2).re_randomize(zero_list(2, 1024), igpu.CudaReRandomizationKey(1024), st)
        """, "Mismatched LweSize between the ciphertext being re-randomized and the provided CompactPublicKey"),
    "a keyswitch key that does not end on the blocks' key": ("""
        ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(np.zeros(8 * 1 * 13, dtype=np.uint64), 8, 12, 24, 1, st)
        radix(2).re_randomize(zero_list(2, 8), igpu.CudaReRandomizationKey(8, ksk), st)
        """, "Mismatched LweSize between the ciphertext being re-randomized and the provided re-randomization keyswitch key"),
    "a keyswitch key that does not start on the public key": ("""
        ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(np.zeros(8 * 1 * 13, dtype=np.uint64), 8, 12, 24, 1, st)
        igpu.CudaReRandomizationKey(16, ksk)
        """, "Mismatched LweDimension between the provided CompactPublicKey and the re-randomization keyswitch key input"),
    "zeros under another key than the re-randomisation key's": ("""
        radix(2).re_randomize(zero_list(2, 1024), igpu.CudaReRandomizationKey(2048), st)
        """, "Mismatched LweDimension between the encryptions of zero and the provided re-randomization key"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_rerand_misuse_is_refused_with_a_message(name):
    snippet, message = REFUSALS[name]
    r = run_child(RERAND_PRELUDE + textwrap.dedent(snippet))
    assert r.returncode != 0, f"{name}: the call was accepted"
    assert message in r.stderr, r.stderr[-600:]


# ------------------------------------------------------------------------------------------ 6. size query
def test_size_only_scratch_counts_and_allocates_nothing():
    """With keyswitch the scratch holds the expanded and the keyswitched zeros, the identity job table and the trivial
    indexes: positive, growing with the count.  Without keyswitch the kernel works in place and the scratch holds
    NOTHING on the device, so the truthful size is 0 for every count: there the query is checked to allocate nothing and
    to stay below the keyswitch mode's."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import ffi
    from tfhe_rs_amd import integer_gpu as igpu
    lib = use_backend("emu")
    st = gpu.CudaStreams([0])
    s, keep = igpu.CudaServerKey._streams(st)
    st.synchronize()

    def stats():
        out = (C.c_uint64 * 7)()
        lib.hip_backend_allocator_stats(0, out)
        return list(out)

    before = stats()
    sizes = {}
    for count in (2, 5, 64):
        for mode, shape in ((RERAND_WITH_KS, (2048, 24, 1)), (RERAND_WITHOUT_KS, (0, 0, 0))):
            mem = C.c_void_p()
            sizes[mode, count] = int(lib.hip_scratch_rerand_64_async(
                s, C.byref(mem), ffi.CudaLweKeyswitchKeyParamsFFI(1024, *shape), count, 4, 4, False, mode))
            assert mem.value
            lib.hip_cleanup_rerand_64(s, C.byref(mem))
            assert not mem.value
    assert stats() == before, "a size query touched the arena"
    with_ks = [sizes[RERAND_WITH_KS, c] for c in (2, 5, 64)]
    without = [sizes[RERAND_WITHOUT_KS, c] for c in (2, 5, 64)]
    assert all(x > 0 for x in with_ks) and with_ks[0] < with_ks[1] < with_ks[2]
    assert all(a > b for a, b in zip(with_ks, without))
    assert without == [0, 0, 0]
    # the two temporaries alone: count * (1025 + 2049) words
    assert with_ks[1] - with_ks[0] >= 3 * (1025 + 2049) * 8


# ------------------------------------------------------------------------------------------ 9. ABI
REF_INCLUDE = "/root/reference/backends/tfhe-cuda-backend/cuda/include/integer"
STANDS_FOR = {
    "hip_scratch_rerand_64_async": ("rerand.h", "scratch_cuda_rerand_64_async"),
    "hip_rerand_64_async": ("rerand.h", "cuda_rerand_64_async"),
    "hip_cleanup_rerand_64": ("rerand.h", "cleanup_cuda_rerand_64"),
    "hip_scratch_integer_grouped_oprf_64_async": ("integer.h", "scratch_cuda_integer_grouped_oprf_64_async"),
    "hip_integer_grouped_oprf_64_async": ("integer.h", "cuda_integer_grouped_oprf_64_async"),
    "hip_cleanup_integer_grouped_oprf_64": ("integer.h", "cleanup_cuda_integer_grouped_oprf_64"),
}


def test_symbols_are_declared_bound_and_exported_by_the_emulation_build():
    import re
    from tfhe_rs_amd import ffi
    lib = use_backend("emu")
    header = open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read()
    for name in STANDS_FOR:
        assert name in ffi.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    assert "enum RERAND_MODE { RERAND_WITH_KS = 0, RERAND_WITHOUT_KS = 1 };" in header
    crate = os.path.join(ROOT, "backends", "tfhe-hip-backend", "src")
    types, bindings = open(os.path.join(crate, "ffi_types.rs")).read(), open(os.path.join(crate, "bindings.rs")).read()
    for name in STANDS_FOR:
        assert f"pub fn {name}(" in bindings, name
    for const in ("RERAND_MODE_RERAND_WITH_KS", "RERAND_MODE_RERAND_WITHOUT_KS"):
        assert f"pub const {const}: RERAND_MODE" in types, const
    used = set(re.findall(r":\s*(?:\*(?:const|mut)\s+)*([A-Z][A-Za-z0-9_]*)\b", bindings))
    assert "RERAND_MODE" in used
    for t in sorted(used):
        assert re.search(r"pub (?:type|struct) %s\b" % t, types), f"{t} is used by bindings.rs and not defined"


@pytest.mark.skipif(not os.path.isdir(REF_INCLUDE), reason="reference tree absent")
def test_prototypes_equal_the_reference_prototypes_they_stand_for():
    import sys
    sys.path.insert(0, ROOT)
    from tools.c_prototypes import parse_prototypes
    ours = parse_prototypes(open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read())
    ref = {f: parse_prototypes(open(os.path.join(REF_INCLUDE, f)).read()) for f in ("rerand.h", "integer.h")}
    for mine, (file, theirs) in STANDS_FOR.items():
        assert mine in ours and theirs in ref[file], (mine, theirs)
        assert ours[mine] == ref[file][theirs], f"{mine}: {ours[mine]} != {ref[file][theirs]}"
