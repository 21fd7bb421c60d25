"""Expansion of compact ciphertext lists (hip_*_expand_without_verification_64): the rotation kernel word for word
against the NumPy restatement of the CPU expansion (tests/expand_helper.py), the rotation algebra by exact decryption
of noiseless fixtures, casting in both directions and the sanity-check kind by decryption of every output block, device
against host emulation word for word, sharding over a stream set, refusals, the size query, the prototypes against the
reference's zk/zk.h, and the Python mirror of the Rust caller.  [emu] runs the kernel sources on the host with toy
keys, [hip] on the MI355X, there also with PARAM_MESSAGE_2_CARRY_2 and the reference's casting decomposition."""
import ctypes as C
import functools
import os
import textwrap

import numpy as np
import pytest

from . import expand_helper as eh
from . import oracle as orc
from .common import C1, TOY_2048, TOY_MB4_2048, decode, decrypt_big, make_keys
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_integer import recompose
from .test_radix_integer import setup as radix_setup

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
U64 = np.uint64
MSG = eh.MSG
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
NO_CASTING, CASTING, SANITY_CHECK = 0, 1, 2      # zk/zk_enums.h
BIG_TO_SMALL, SMALL_TO_BIG = 0, 1                # keyswitch/ks_enums.h
MULTI_BIT, CLASSICAL = 0, 1                      # pbs/pbs_enums.h
SENTINEL = 0xD1D1D1D1D1D1D1D1


def ksk_params(n_in, n_out, base_log, level):
    from tfhe_rs_amd import ffi
    return ffi.CudaLweKeyswitchKeyParamsFFI(n_in, n_out, base_log, level)


def scratch(lib, s, mem, counts, flags, *, casting, computing=(0, 0, 0, 0), k=1, N=2048, pbs=(1, 23), grouping=0,
            msg=MSG, carry=MSG, pbs_type=CLASSICAL, ks_type=BIG_TO_SMALL, kind=CASTING, ms=0, allocate=True,
            flags_len=None):
    c_counts = (C.c_uint32 * max(1, len(counts)))(*counts)
    c_flags = (C.c_bool * max(1, len(flags)))(*flags)
    return int(lib.hip_scratch_expand_without_verification_64_async(
        s, C.byref(mem), k, N, ksk_params(*computing), ksk_params(*casting), pbs[0], pbs[1], grouping, c_counts, c_flags,
        len(flags) if flags_len is None else flags_len, len(counts), msg, carry, pbs_type, ks_type, allocate, kind, ms))


# ------------------------------------------------------------------------------------------ 1. the kernel, word for word
def expand_no_casting(kind, words, n_c, counts):
    """NO_CASTING through the C ABI into a buffer pre-filled with a sentinel, with a guard row behind it; returns the
    rows and the guard.  Every device object is local: only NumPy leaves."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import integer_gpu as igpu
    lib = use_backend(kind)
    st = gpu.CudaStreams([0])
    s, keep = igpu.CudaServerKey._streams(st)
    total = sum(counts)
    d_in = gpu.CudaVec.from_cpu_async(words, st)
    d_out = gpu.CudaVec.from_cpu_async(np.full((total + 1) * (n_c + 1), SENTINEL, dtype=U64), st)
    mem = C.c_void_p()
    scratch(lib, s, mem, counts, [], casting=(n_c, n_c, 4, 4), kind=NO_CASTING)
    lib.hip_expand_without_verification_64_async(s, d_out.ptr, d_in.ptr, mem, None, None, None)
    lib.hip_cleanup_expand_without_verification_64(s, C.byref(mem))
    assert not mem.value
    got = d_out.copy_to_cpu(st).reshape(total + 1, n_c + 1)
    return got[:total], got[total]


KERNEL_CASES = {
    "n2048_1_body": (2048, [1]),
    "n2048_2_bodies": (2048, [2]),
    "n2048_2047_bodies": (2048, [2047]),
    "n2048_2048_bodies": (2048, [2048]),
    "n2048_lists_of_5_2048_1": (2048, [5, 2048, 1]),   # the middle list's mask starts at word 2053: odd
    "n8_8_bodies": (8, [8]),
    "n12_12_bodies": (12, [12]),                        # not a power of two
    "n1025_lists_of_1025_3": (1025, [1025, 3]),         # rows of 1026 words: one word into the second chunk of a row
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
@pytest.mark.parametrize("kind", BACKENDS)
def test_expansion_kernel_word_for_word(kind, case):
    n_c, counts = KERNEL_CASES[case]
    rng = np.random.default_rng(201)
    words = rng.integers(0, 1 << 64, size=sum(n_c + c for c in counts), dtype=U64)
    assert (2048 + 5) % 2 == 1
    got, guard = expand_no_casting(kind, words, n_c, counts)
    want = eh.expand(words, n_c, counts)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"rows {bad[:8]} differ"
    assert (guard == U64(SENTINEL)).all(), "written past the last row"


@pytest.mark.parametrize("kind", BACKENDS)
def test_expansion_kernel_negates_edge_masks(kind):
    """Masks of all zeros, all ones and 2^63 (its own negation; -0 = 0; -(2^64 - 1) = 1), with random bodies."""
    n_c, c = 2048, 2048
    rng = np.random.default_rng(202)
    for value in (0, (1 << 64) - 1, 1 << 63):
        words = np.concatenate([np.full(n_c, value, dtype=U64), rng.integers(0, 1 << 64, size=c, dtype=U64)])
        got, guard = expand_no_casting(kind, words, n_c, [c])
        assert np.array_equal(got, eh.expand(words, n_c, [c])), hex(value)
        assert int(got[n_c - 1][0]) == (-value) % (1 << 64) and int(got[0][0]) == value
        assert (guard == U64(SENTINEL)).all()


# ------------------------------------------------------------------------------------------ 2. rotation algebra
@pytest.mark.parametrize("kind", BACKENDS)
def test_expanded_lwes_decrypt_exactly_to_their_bodies_messages(kind):
    """A full list (2048 bodies) made from the secret key without noise: the expanded LWE d is an encryption of body d's
    message under the same key, exactly, because <mask X^d, s> is what the fixture added to the body."""
    n_c = 2048
    sk = eh.pke_key(n_c)
    picks = (0, 1, 1023, 1024, 2047)
    values = [int(v) for v in np.random.default_rng(206).integers(0, 16, size=n_c)]
    words = eh.make_compact_list(sk, values, seed=203)
    got, _ = expand_no_casting(kind, words, n_c, [n_c])
    for d in picks:
        assert int(orc.lwe_decrypt(got[d], sk)) == (eh.DELTA * values[d]) % (1 << 64), d


# ------------------------------------------------------------------------------------------ 3 - 6. casting
@functools.lru_cache(maxsize=8)
def host_casting_key(p, n_c, to_big, base_log, level):
    keys = make_keys(p)
    dest = keys.glwe_sk if to_big else keys.lwe_sk
    return eh.casting_key(0x63617374, eh.pke_key(n_c), dest, base_log, level, p.glwe_noise if to_big else p.lwe_noise)


def expand_casting(kind, p, lists, flags, *, n_c=2048, to_big=False, decomposition=(4, 4), expand_kind=CASTING,
                   gpu_indexes=(0,), threshold=0, seed=204):
    """Compact lists of the packed values `lists` under a key of n_c bits, expanded through the C ABI with a casting key
    to the small (BIG_TO_SMALL) or big (SMALL_TO_BIG) key of the compute set p, into a dirtied buffer; returns the
    2 * bodies output blocks.  Every device object is local: only NumPy leaves."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    lib = use_backend(kind)
    _, keys, st, sks, igpu = radix_setup(kind, p, gpu_indexes)
    base_log, level = decomposition
    n_out = p.big_n if to_big else p.n
    cast = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(host_casting_key(p, n_c, to_big, base_log, level), n_c, n_out,
                                                          base_log, level, st)
    words, counts = eh.make_flattened(eh.pke_key(n_c), lists, seed)
    total = sum(counts)
    s, keep = igpu.CudaServerKey._streams(st)
    d_in = gpu.CudaVec.from_cpu_async(words, st)
    d_out = gpu.CudaVec.from_cpu_async(np.full((2 * total + 1) * (p.big_n + 1), SENTINEL, dtype=U64), st)
    ksks, bsks = sks._key_ptrs(st)
    casts = (C.c_void_p * len(st))(*[v.ptr for v in cast.d_vecs])
    mem = C.c_void_p()
    lib.hip_integer_set_multi_gpu_threshold(threshold)
    try:
        scratch(lib, s, mem, counts, flags, casting=(n_c, n_out, base_log, level),
                computing=(p.big_n, p.n, p.ks_base_log, p.ks_level), k=p.k, N=p.N, pbs=(p.pbs_level, p.pbs_base_log),
                grouping=p.grouping, pbs_type=MULTI_BIT if p.grouping else CLASSICAL,
                ks_type=SMALL_TO_BIG if to_big else BIG_TO_SMALL, kind=expand_kind, ms=p.ms_type)
        lib.hip_expand_without_verification_64_async(s, d_out.ptr, d_in.ptr, mem, bsks, ksks, casts)
        lib.hip_cleanup_expand_without_verification_64(s, C.byref(mem))
    finally:
        lib.hip_integer_set_multi_gpu_threshold(0)
    got = d_out.copy_to_cpu(st).reshape(2 * total + 1, p.big_n + 1)
    assert (got[2 * total] == U64(SENTINEL)).all(), "written past the last block"
    return got[:2 * total]


def expected_blocks(lists, flags):
    return [min(1, h) if f else h for h, f in zip(halves_of(lists), flags)]


P = eh.pack
# two lists of 3 and 2 bodies; (message, second) covers (0,0), (3,3), (1,2), (2,0), (0,1) in both orders.  Outputs 4 (the
# message of body 2) and 7 (the second of body 3) are flagged boolean: they hold 1 and 0 in order A, 3 and 1 in order B
ORDER_A = [[P(0, 0), P(3, 3), P(1, 2)], [P(2, 0), P(0, 1)]]
ORDER_B = [[P(0, 0), P(1, 2), P(3, 3)], [P(0, 1), P(2, 0)]]
FLAGS_4_7 = [q in (4, 7) for q in range(10)]
CASTING_CASES = [pytest.param("emu", TOY_2048, id="emu-toy_classic"), pytest.param("emu", TOY_MB4_2048, id="emu-toy_multi_bit_g4"),
                 pytest.param("hip", TOY_2048, id="hip-toy_classic", marks=pytest.mark.gpu),
                 pytest.param("hip", TOY_MB4_2048, id="hip-toy_multi_bit_g4", marks=pytest.mark.gpu),
                 pytest.param("hip", C1, id="hip-message_2_carry_2", marks=pytest.mark.gpu)]


def halves_of(lists):
    return [h for vals in lists for m in vals for h in (m % MSG, m // MSG)]


@pytest.mark.parametrize("kind,p", CASTING_CASES)
def test_casting_big_to_small_splits_and_sanitises_every_block(kind, p):
    """4 levels of 4 bits: the reference's PKE-to-small casting decomposition (on every set here)."""
    assert [halves_of(o)[q] for o in (ORDER_A, ORDER_B) for q in (4, 7)] == [1, 0, 3, 1]
    assert [expected_blocks(o, FLAGS_4_7)[q] for o in (ORDER_A, ORDER_B) for q in (4, 7)] == [1, 0, 1, 1]
    keys = make_keys(p)
    for lists in (ORDER_A, ORDER_B):
        out = expand_casting(kind, p, lists, FLAGS_4_7)
        got = [decrypt_big(p, keys, b) for b in out]
        print(p.name, "decrypted", got)
        assert got == expected_blocks(lists, FLAGS_4_7)


@pytest.mark.parametrize("kind", BACKENDS)
def test_casting_small_to_big_keyswitches_first(kind):
    """An encryption key of 1024 bits cast to the 2048-bit big key with one level of 24 bits (the reference's PKE-to-big
    decomposition), then the ordinary round with the computing keyswitch key.  One list of 4; outputs 4 and 7 boolean."""
    p = TOY_2048
    lists = [[P(3, 3), P(1, 2), P(3, 0), P(0, 1)]]
    flags = [q in (4, 7) for q in range(8)]
    out = expand_casting(kind, p, lists, flags, n_c=1024, to_big=True, decomposition=(24, 1))
    got = [decrypt_big(p, make_keys(p), b) for b in out]
    assert got == expected_blocks(lists, flags) == [3, 3, 1, 2, 1, 0, 0, 1]


@pytest.mark.parametrize("kind", BACKENDS)
def test_sanity_check_kind_applies_the_identity(kind):
    p = TOY_2048
    lists = [[P(0, 0), P(3, 3), P(1, 2)], [P(2, 0), P(0, 1)]]
    out = expand_casting(kind, p, lists, FLAGS_4_7, expand_kind=SANITY_CHECK)
    got = [decrypt_big(p, make_keys(p), b) for b in out]
    assert got == [m for vals in lists for m in vals for _ in (0, 1)]


@pytest.mark.gpu
def test_device_equals_emulation_word_for_word():
    out = expand_casting("hip", TOY_2048, ORDER_A, FLAGS_4_7)
    try:
        emu = expand_casting("emu", TOY_2048, ORDER_A, FLAGS_4_7)
    finally:
        use_backend("hip")
    differing = int((emu != out).any(axis=1).sum())
    print(f"hip vs emu: {differing} of {len(out)} blocks differ")
    assert np.array_equal(emu, out)


# ------------------------------------------------------------------------------------------ 11. a stream set of two
@pytest.mark.parametrize("kind", BACKENDS)
def test_round_shards_over_a_two_entry_stream_set(kind):
    """Two streams (of device 0: the machines have one GPU, as in the radix layer's sharding tests) and one block per GPU
    from which a round spreads: the expansion stays on the first stream, the ten blocks of the round travel 5 + 5 with
    the casting key's replica of each stream.  Same words as one stream."""
    one = expand_casting(kind, TOY_2048, ORDER_A, FLAGS_4_7)
    two = expand_casting(kind, TOY_2048, ORDER_A, FLAGS_4_7, gpu_indexes=(0, 0), threshold=1)
    assert np.array_equal(one, two)


def test_round_shards_over_two_distinct_devices(monkeypatch):
    """The same on the CPU tier's device model with two devices (streams and events belong to their device there)."""
    monkeypatch.setenv("HIPEMU_DEVICES", "2")
    one = expand_casting("emu", TOY_2048, ORDER_A, FLAGS_4_7)
    two = expand_casting("emu", TOY_2048, ORDER_A, FLAGS_4_7, gpu_indexes=(0, 1), threshold=1)
    assert np.array_equal(one, two)


# ------------------------------------------------------------------------------------------ 7. refusals
EXPAND_PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
v = gpu.CudaVec(16 * 2049, st)
mem = C.c_void_p()
KK = ffi.CudaLweKeyswitchKeyParamsFFI
def scratch(counts, flags, casting=(2048, 12, 4, 4), msg=4, carry=4, ks_type=0, kind=1, allocate=True, lists=None):
    c = (C.c_uint32 * max(1, len(counts)))(*counts)
    f = (C.c_bool * max(1, len(flags)))(*flags)
    return lib.hip_scratch_expand_without_verification_64_async(
        s, C.byref(mem), 1, 2048, KK(2048, 12, 4, 4), KK(*casting), 1, 23, 0, c, f, len(flags),
        len(counts) if lists is None else lists, msg, carry, 1, ks_type, allocate, kind, 0)
"""

REFUSALS = {
    "more bodies than mask words": ("scratch([3, 2049], [False] * 4104)", "holds 2049 bodies"),
    "a list of no bodies": ("scratch([3, 0], [False] * 6)", "holds 0 bodies"),
    "zero lists": ("scratch([], [], lists=0)", "no compact list to expand"),
    "is_boolean_array too short": ("scratch([3, 2], [False] * 9)", "is_boolean_array holds 9 entries"),
    "carry other than message with CASTING": ("scratch([2], [False] * 4, msg=2, carry=8)",
                                              "requires carry_modulus equal to message_modulus"),
    "SMALL_TO_BIG with SANITY_CHECK": ("scratch([2], [False] * 4, casting=(1024, 2048, 24, 1), ks_type=1, kind=2)",
                                       "SANITY_CHECK not supported for SMALL_TO_BIG"),
    "a launch on a size-only scratch": ("""
        scratch([2], [False] * 4, allocate=False)
        keys = (C.c_void_p * 1)(v.ptr)
        lib.hip_expand_without_verification_64_async(s, v.ptr, v.ptr, mem, keys, keys, keys)
        """, "scratch was created with allocate_gpu_memory=false"),
    "a launch on a scratch of another kind": ("""
        lib.hip_scratch_packing_keyswitch_lwe_list_to_glwe_64_async(s, C.byref(mem), 2048, 2, 16, 4, 3, 4, True)
        keys = (C.c_void_p * 1)(v.ptr)
        lib.hip_expand_without_verification_64_async(s, v.ptr, v.ptr, mem, keys, keys, keys)
        """, "foreign scratch pointer"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_expand_misuse_aborts_with_a_message_naming_the_entry_point(name):
    snippet, message = REFUSALS[name]
    r = run_child(EXPAND_PRELUDE + textwrap.dedent(snippet))
    assert r.returncode != 0, f"{name}: the call was accepted"
    assert message in r.stderr and "expand_without_verification" in r.stderr, r.stderr[-600:]


# ------------------------------------------------------------------------------------------ 8. size-only scratch
def test_size_only_scratch_counts_and_allocates_nothing():
    from tfhe_rs_amd import core_crypto_gpu as gpu
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
    sizes = []
    for bodies in (2, 5, 64):
        for kind, ks_type, casting in ((CASTING, BIG_TO_SMALL, (2048, 12, 4, 4)), (CASTING, SMALL_TO_BIG, (1024, 2048, 24, 1)),
                                       (SANITY_CHECK, BIG_TO_SMALL, (2048, 12, 4, 4)), (NO_CASTING, BIG_TO_SMALL, (2048, 12, 4, 4))):
            mem = C.c_void_p()
            size = scratch(lib, s, mem, [bodies], [False] * (2 * bodies), casting=casting, computing=(2048, 12, 4, 4),
                           ks_type=ks_type, kind=kind, allocate=False)
            assert mem.value
            lib.hip_cleanup_expand_without_verification_64(s, C.byref(mem))
            assert not mem.value
            sizes.append(size)
    assert stats() == before, "a size query touched the arena"
    assert all(x > 0 for x in sizes)
    for a, b in zip(sizes[:4] + sizes[4:8], sizes[4:8] + sizes[8:]):   # every kind grows with the body count
        assert b > a
    # the expanded temporary alone: bodies * (n_c + 1) words
    assert sizes[4] - sizes[0] >= 3 * 2049 * 8


# ------------------------------------------------------------------------------------------ 9. prototypes
REF_ZK = "/root/reference/backends/tfhe-cuda-backend/cuda/include/zk/zk.h"
STANDS_FOR = {
    "hip_scratch_expand_without_verification_64_async": "scratch_cuda_expand_without_verification_64_async",
    "hip_expand_without_verification_64_async": "cuda_expand_without_verification_64_async",
    "hip_cleanup_expand_without_verification_64": "cleanup_cuda_expand_without_verification_64",
}


def test_expand_symbols_are_declared_bound_and_exported_by_the_emulation_build():
    from tfhe_rs_amd import ffi
    lib = use_backend("emu")
    for name in STANDS_FOR:
        assert name in ffi.SIGNATURES and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read()
    assert "enum KS_TYPE { BIG_TO_SMALL = 0, SMALL_TO_BIG = 1 };" in header
    assert "enum EXPAND_KIND { NO_CASTING = 0, CASTING = 1, SANITY_CHECK = 2 };" in header
    # every type the generated Rust bindings name is defined by the hand-written ffi_types.rs, with bindgen's constants
    import re
    crate = os.path.join(ROOT, "backends", "tfhe-hip-backend", "src")
    types = open(os.path.join(crate, "ffi_types.rs")).read()
    used = set(re.findall(r":\s*(?:\*(?:const|mut)\s+)*([A-Z][A-Za-z0-9_]*)\b", open(os.path.join(crate, "bindings.rs")).read()))
    for t in sorted(used):
        assert re.search(r"pub (?:type|struct) %s\b" % t, types), f"{t} is used by bindings.rs and not defined"
    for const in ("KS_TYPE_BIG_TO_SMALL", "KS_TYPE_SMALL_TO_BIG", "EXPAND_KIND_NO_CASTING", "EXPAND_KIND_CASTING",
                  "EXPAND_KIND_SANITY_CHECK", "BITOP_TYPE_SCALAR_BITXOR", "COMPARISON_TYPE_MIN",
                  "SHIFT_OR_ROTATE_TYPE_RIGHT_ROTATE"):
        assert f"pub const {const}:" in types, const


@pytest.mark.skipif(not os.path.isfile(REF_ZK), reason="reference tree absent")
def test_expand_prototypes_equal_the_reference_prototypes_they_stand_for():
    import sys
    sys.path.insert(0, ROOT)
    from tools.c_prototypes import parse_prototypes
    ours = parse_prototypes(open(os.path.join(ROOT, "include", "tfhe_hip_backend.h")).read())
    ref = parse_prototypes(open(REF_ZK).read())
    for mine, theirs in STANDS_FOR.items():
        assert mine in ours and theirs in ref, (mine, theirs)
        assert ours[mine] == ref[theirs], f"{mine}: {ours[mine]} != {ref[theirs]}"


# ------------------------------------------------------------------------------------------ 10. the Python API
@pytest.mark.parametrize("kind", BACKENDS)
def test_python_api_expands_an_integer_and_a_boolean(kind):
    """One list holding a 4-block unsigned integer (2 bodies) and a boolean (1 body), as the Rust caller holds them."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    p, keys, st, sks, igpu = radix_setup(kind, TOY_2048)
    n_c = 2048
    cast = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(host_casting_key(p, n_c, False, 4, 4), n_c, p.n, 4, 4, st)
    key = igpu.CudaKeySwitchingKey(cast, "small", sks)
    clear, flag = 0xB6, 1
    digits = [(clear >> (2 * j)) & 3 for j in range(4)]
    packed = [P(digits[0], digits[1]), P(digits[2], digits[3]), P(flag, 0)]
    words = eh.make_compact_list(eh.pke_key(n_c), packed, seed=205)
    data_info = [("unsigned", 4), ("boolean",)]
    flat = igpu.CudaFlattenedVecCompactCiphertextList.from_flat_words(words, n_c, [3], data_info, MSG, MSG, st)
    assert flat.d_list.n_c == n_c and flat.num_lwe_per_compact_list == [3]
    assert flat.is_boolean == [False, False, False, False, True, False]
    expander = flat.expand(key, st)
    assert isinstance(expander, igpu.CudaCompactCiphertextListExpander)
    assert len(expander) == 2 and expander.get_kind_of(0) == ("unsigned", 4) and expander.get_kind_of(1) == ("boolean",)
    assert expander.get_kind_of(2) is None and expander.get(2, st) is None
    integer, boolean = expander.get(0, st), expander.get(1, st)
    assert isinstance(integer, igpu.CudaUnsignedRadixCiphertext) and integer.num_blocks == 4
    rows = [[decrypt_big(p, keys, b) for b in row] for row in integer.to_blocks(st)]
    assert recompose(rows) == [clear]
    assert boolean.num_blocks == 1 and decrypt_big(p, keys, boolean.to_blocks(st)[0][0]) == flag
    assert list(integer.degrees) == [MSG - 1] * 4 and list(boolean.degrees) == [1]
    assert list(integer._info[1]) == [1] * 4 and list(boolean._info[1]) == [1]   # nominal noise level
    # the expanded integer is an ordinary radix ciphertext: it adds
    sks.add_assign(integer, expander.get(0, st), st)
    assert recompose([[decrypt_big(p, keys, b) for b in row] for row in integer.to_blocks(st)]) == [(2 * clear) & 0xFF]
    # no_casting: the expanded LWEs themselves, under the encryption key
    raw = flat.expand(key, st, kind="no_casting").to_lwe_ciphertext_list(st)
    assert np.array_equal(raw, eh.expand(words, n_c, [3]))
    assert [decode(p, orc.lwe_decrypt(r, eh.pke_key(n_c))) for r in raw] == packed
