"""What a scratch of the radix layer takes from the device it gives back.

1. Give-back: every scratch entry point of the radix layer, created for real (the arena's live bytes grow), cleaned up (they
   are back where they were), and created as a size query (they never move).  The number each mode returns is compared
   with tests/golden/radix_scratch_sizes.json, recorded on the host emulation of the commit before the scratches got one
   owner for their device memory: host-side sums of the requested bytes, the same on the emulation and on the device.
2. Shape change: ONE scratch sized for two integers is called with 2, 1 and 2 integers (the arithmetic shift also with the
   amounts 3, 5, 3; the scalar multiplication also with the scalars 0xB7, 3, 0xB7; the sum with vectors of 6, 5 and 6
   integers besides, since its forms for two integers and one are shortcuts that touch no index array), so that the index
   arrays of a call are rebuilt in front of launches that read the new ones.  Every result decrypts to the clear result and
   the cleanup returns every byte.

[emu] runs the kernel sources on the host with the toy set of tests/test_radix_integer.py, [hip] on the MI355X with
PARAM_MESSAGE_2_CARRY_2; 5 blocks per integer, the smallest count at which the carry look-ahead has a level of groups above
the blocks."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

from . import compression128_helper as c128
from . import compression_helper as comp
from . import pbs128_helper as h128
from . import radix_model as rm
from .common import C1, TOY_2048
from .harness import use_backend

L = 5                       # blocks per integer
MSG = CARRY = 4
SIZES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radix_scratch_sizes.json")


def live_bytes(lib):
    out = (C.c_uint64 * 7)()
    lib.hip_backend_allocator_stats(0, out)
    return int(out[5])


def parameter_sets(kind):
    """compute set, compression set, 128-bit compression set, squashing sets (classic, multi-bit with its grouping factor)"""
    if kind == "emu":
        p = TOY_2048
        return p, comp.TOY_PACK, c128.SET_A, h128.Params128("squash", p.n, 1, 512, 24, 3, ms_type=1), \
            (h128.Params128("squash_mb", p.n, 2, 2048, 18, 4), 4)
    return C1, comp.REAL, c128.REFERENCE_SETS[0], h128.PRODUCTION, (dataclasses.replace(h128.PRODUCTION, base_log=18, level=4), 3)


def scratch_cases(kind):
    """name -> (scratch entry point, its arguments behind (streams, mem_ptr) for a real creation, cleanup entry point,
    hip_integer_scratch_batch in force).  The last bool of every argument list is allocate_gpu_memory."""
    from tfhe_rs_amd import ffi
    p, cp, cq, sq, (sqmb, g) = parameter_sets(kind)
    B = ffi.CudaLweBootstrapKeyParamsFFI(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.big_n, 1, 0)
    K = ffi.CudaLweKeyswitchKeyParamsFFI(p.big_n, p.n, p.ks_base_log, p.ks_level)
    nr = p.ms_type
    lut = np.zeros((p.k + 1) * p.N, dtype=np.uint64)
    lut_ptr = lut.ctypes.data_as(C.c_void_p)
    n_c = 64                                                  # the compact lists' encryption key (expand, rerand)
    counts, flags = (C.c_uint32 * 1)(3), (C.c_bool * 6)()     # one compact list of three bodies: six blocks, no boolean
    dec_B = ffi.CudaLweBootstrapKeyParamsFFI(cp.k * cp.N, p.k, p.N, p.pbs_base_log, p.pbs_level, p.big_n, 1, 0)
    radix = (B, K, L, MSG, CARRY)

    def squash(s):
        return (s.n, s.k, s.N, p.k, p.N, p.ks_level, p.ks_base_log, s.level, s.base_log, (L + 1) // 2, L, MSG, CARRY, True)

    cases = {
        "apply_univariate_lut": ("scratch_cuda_apply_univariate_lut_64_async", (lut_ptr, *radix, MSG - 1, True, nr),
                                 "cleanup_cuda_apply_univariate_lut_64"),
        "apply_many_univariate_lut": ("scratch_cuda_apply_many_univariate_lut_64_async", (lut_ptr, *radix, 2, MSG - 1, True, nr),
                                      "cleanup_cuda_apply_many_univariate_lut_64"),
        "propagate": ("scratch_cuda_propagate_single_carry_64_inplace_async", (*radix, 0, True, nr),
                      "cleanup_cuda_propagate_single_carry_64_inplace"),
        "add_and_propagate": ("scratch_cuda_add_and_propagate_single_carry_64_inplace_async", (*radix, 0, True, nr),
                              "cleanup_cuda_add_and_propagate_single_carry_64_inplace"),
        "add_and_propagate_overflow": ("scratch_cuda_add_and_propagate_single_carry_64_inplace_async", (*radix, 1, True, nr),
                                       "cleanup_cuda_add_and_propagate_single_carry_64_inplace"),
        "mult": ("scratch_cuda_integer_mult_inplace_64_async", (False, False, MSG, CARRY, B, K, L, True, nr),
                 "cleanup_cuda_integer_mult_inplace_64"),
        "mult_by_boolean": ("scratch_cuda_integer_mult_inplace_64_async", (False, True, MSG, CARRY, B, K, L, True, nr),
                            "cleanup_cuda_integer_mult_inplace_64"),
        "bitop": ("scratch_cuda_integer_bitop_inplace_64_async", (*radix, 0, True, nr), "cleanup_cuda_integer_bitop_inplace_64"),
        "scalar_bitop": ("scratch_cuda_integer_scalar_bitop_inplace_64_async", (*radix, 3, True, nr),
                         "cleanup_cuda_integer_scalar_bitop_inplace_64"),
        "sub": ("scratch_cuda_sub_and_propagate_single_carry_64_inplace_async", (*radix, 0, True, nr),
                "cleanup_cuda_sub_and_propagate_single_carry_64_inplace"),
        "overflowing_sub": ("scratch_cuda_integer_overflowing_sub_64_inplace_async", (*radix, 1, True, nr),
                            "cleanup_cuda_integer_overflowing_sub_64_inplace"),
        "full_propagation": ("scratch_cuda_full_propagation_64_inplace_async", (B, K, MSG, CARRY, True, nr),
                             "cleanup_cuda_full_propagation_64_inplace"),
        "comparison_eq": ("scratch_cuda_integer_comparison_64_async", (*radix, 0, False, True, nr),
                          "cleanup_cuda_integer_comparison_64"),
        "comparison_gt": ("scratch_cuda_integer_comparison_64_async", (*radix, 2, False, True, nr),
                          "cleanup_cuda_integer_comparison_64"),
        "comparison_max": ("scratch_cuda_integer_comparison_64_async", (*radix, 6, False, True, nr),
                           "cleanup_cuda_integer_comparison_64"),
        "scalar_comparison_ge": ("scratch_cuda_integer_scalar_comparison_64_async", (*radix, 3, False, True, nr),
                                 "cleanup_cuda_integer_scalar_comparison_64"),
        "cmux": ("scratch_cuda_cmux_64_async", (*radix, True, nr), "cleanup_cuda_cmux_64"),
        "logical_scalar_shift": ("scratch_cuda_logical_scalar_shift_64_inplace_async", (*radix, 0, True, nr),
                                 "cleanup_cuda_logical_scalar_shift_64_inplace"),
        "arithmetic_scalar_shift": ("hip_scratch_integer_arithmetic_scalar_shift_64_inplace_async", (*radix, 1, True, nr),
                                    "hip_cleanup_integer_arithmetic_scalar_shift_64_inplace"),
        "scalar_rotate": ("hip_scratch_integer_scalar_rotate_64_inplace_async", (*radix, 2, True, nr),
                          "hip_cleanup_integer_scalar_rotate_64_inplace"),
        "partial_sum": ("hip_scratch_partial_sum_ciphertexts_vec_64_async", (B, K, L, 6, MSG, CARRY, False, True, nr),
                        "hip_cleanup_partial_sum_ciphertexts_vec_64"),
        "scalar_mul": ("hip_scratch_integer_scalar_mul_64_async", (*radix, 8, True, nr), "hip_cleanup_integer_scalar_mul_64"),
        "packing_keyswitch_64": ("hip_scratch_packing_keyswitch_lwe_list_to_glwe_64_async",
                                 (p.big_n, cp.k, cp.N, cp.ks_base_log, cp.ks_level, L, True),
                                 "hip_cleanup_packing_keyswitch_lwe_list_to_glwe_64"),
        "compress_64": ("hip_scratch_integer_compress_radix_ciphertext_64_async",
                        (p.big_n, cp.k, cp.N, cp.ks_base_log, cp.ks_level, L, MSG, CARRY, cp.lwe_per_glwe,
                         cp.storage_log_modulus, True), "hip_cleanup_integer_compress_radix_ciphertext_64"),
        "decompress_64": ("hip_scratch_integer_decompress_radix_ciphertext_64_async",
                          (dec_B, cp.k, cp.N, cp.lwe_per_glwe, cp.storage_log_modulus, L, MSG, CARRY, True, nr),
                          "hip_cleanup_integer_decompress_radix_ciphertext_64"),
        "packing_keyswitch_128": ("hip_scratch_packing_keyswitch_lwe_list_to_glwe_128_async",
                                  (cq.n_in, cq.k, cq.N, cq.base_log, cq.level, L, True),
                                  "hip_cleanup_packing_keyswitch_lwe_list_to_glwe_128"),
        "compress_128": ("hip_scratch_integer_compress_radix_ciphertext_128_async",
                         (cq.n_in, cq.k, cq.N, cq.base_log, cq.level, L, MSG, CARRY, cq.per, cq.storage_log_modulus, True),
                         "hip_cleanup_integer_compress_radix_ciphertext_128"),
        "decompress_128": ("hip_scratch_integer_decompress_radix_ciphertext_128_async",
                           (cq.k, cq.N, cq.per, cq.storage_log_modulus, L, MSG, CARRY, True),
                           "hip_cleanup_integer_decompress_radix_ciphertext_128"),
        "noise_squashing": ("hip_scratch_integer_apply_noise_squashing_64_async", (*squash(sq), sq.ms_type),
                            "hip_cleanup_integer_apply_noise_squashing_64"),
        "noise_squashing_multi_bit": ("hip_scratch_integer_apply_noise_squashing_multi_bit_64_async", (*squash(sqmb), 0, g),
                                      "hip_cleanup_integer_apply_noise_squashing_64"),
        "expand": ("hip_scratch_expand_without_verification_64_async",
                   (p.k, p.N, K, ffi.CudaLweKeyswitchKeyParamsFFI(n_c, p.n, 4, 4), p.pbs_level, p.pbs_base_log, 0, counts, flags,
                    6, 1, MSG, CARRY, 1, 0, True, 1, nr), "hip_cleanup_expand_without_verification_64"),
        "rerand": ("hip_scratch_rerand_64_async", (ffi.CudaLweKeyswitchKeyParamsFFI(n_c, p.big_n, 4, 4), L, MSG, CARRY, True, 0),
                   "hip_cleanup_rerand_64"),
        "grouped_oprf": ("hip_scratch_integer_grouped_oprf_64_async", (B, K, L, MSG, CARRY, True, 2 * L, nr),
                         "hip_cleanup_integer_grouped_oprf_64"),
    }
    for name, (kind_of, signed) in {"left_shift": (0, False), "signed_right_shift": (1, True), "left_rotate": (2, False),
                                    "signed_right_rotate": (3, True)}.items():
        cases[name] = ("hip_scratch_integer_shift_and_rotate_64_inplace_async", (*radix, kind_of, signed, True, nr),
                       "hip_cleanup_integer_shift_and_rotate_64_inplace")
    # the entry points that read hip_integer_scratch_batch at both batches; the others once
    batched = ("propagate", "add_and_propagate", "add_and_propagate_overflow", "mult", "mult_by_boolean", "bitop", "sub",
               "overflowing_sub", "scalar_mul", "arithmetic_scalar_shift", "scalar_rotate", "left_shift", "signed_right_shift",
               "left_rotate", "signed_right_rotate")
    out = {}
    for name, case in cases.items():
        for batch in ((1, 2) if name in batched else (1,)):
            out[f"{name}-batch_{batch}" if name in batched else name] = (*case, batch, (lut, counts, flags))
    return out


def create_and_clean(lib, s, case, allocate):
    """(bytes the scratch call returned, live bytes while the scratch stood); asserts that the cleanup gave everything back"""
    scratch, args, cleanup, batch, keep = case
    fn = getattr(lib, scratch)
    at = max(i for i, t in enumerate(fn.argtypes) if t is C.c_bool) - 2     # allocate_gpu_memory among `args`
    assert args[at] is True
    args = args[:at] + (allocate,) + args[at + 1:]
    start = live_bytes(lib)
    mem = C.c_void_p()
    lib.hip_integer_scratch_batch(batch)
    size = int(fn(s, C.byref(mem), *args))
    lib.hip_integer_scratch_batch(1)
    assert mem.value
    held = live_bytes(lib)
    getattr(lib, cleanup)(s, C.byref(mem))
    assert not mem.value
    assert live_bytes(lib) == start, f"{scratch}: {live_bytes(lib) - start} bytes are still live after the cleanup"
    return size, held - start


def case_ids():
    names = list(scratch_cases("emu"))
    return [pytest.param(kind, n, id=f"{kind}-{n}", marks=[pytest.mark.gpu] if kind == "hip" else [])
            for kind in ("emu", "hip") for n in names]


@pytest.mark.parametrize("kind,name", case_ids())
def test_scratch_gives_back_what_it_took(kind, name):
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import integer_gpu as igpu
    lib = use_backend(kind)
    st = gpu.CudaStreams((0,))
    s, keep = igpu.CudaServerKey._streams(st)
    st.synchronize()
    case = scratch_cases(kind)[name]
    real, held = create_and_clean(lib, s, case, True)
    assert held > 0, "a real creation took nothing from the arena: the check above would be vacuous"
    query, held_by_query = create_and_clean(lib, s, case, False)
    assert held_by_query == 0, "a size query allocated"
    with open(SIZES) as f:
        want = json.load(f)[kind][name]
    print(f"{kind} {name}: real creation returns {real}, size query {query}; recorded {want}")
    assert [real, query] == want


# ================================================================================== 2. shape change
class Calls:
    """raw calls on ONE scratch sized for a batch of two: scratch -> calls -> cleanup, the live bytes around it"""

    def __init__(self, kind):
        from .test_radix_bases import BASES, Ctx
        base = next(b for b in BASES if b.name == "classic_4_4")
        self.c = c = Ctx(kind, base)
        self.lib = use_backend(kind)
        self.s, self.keep = c.sks._streams(c.st)
        self.ksks, self.bsks = c.sks._key_ptrs(c.st)
        self.radix = (c.sks._bsk_params(), c.sks._ksk_params(), L, MSG, CARRY)
        self.nr = c.sks._noise_reduction()
        self.mask = MSG ** L - 1
        # what the first keyswitch and the first bootstrap with fresh keys derive from them and keep for the keys' lifetime
        # (keyswitch planes, a split key's twin) is no scratch memory; in the arena's red-zone mode it is arena memory all
        # the same, so one operation comes before the first reading
        c.sks.add_assign(self.enc([1], 1), self.enc([2], 2), c.st)

    def enc(self, values, seed):
        return self.c.enc([rm.digits(v, L, MSG) for v in values], seed)

    def values(self, ct):
        return [rm.value(row, MSG) for row in self.c.dec(ct)]

    def carries(self, n):
        igpu = self.c.igpu
        from tfhe_rs_amd.core_crypto_gpu import CudaVec
        return igpu.CudaUnsignedRadixCiphertext(CudaVec(n * (self.c.p.big_n + 1), self.c.st), n, 1, self.c.p.big_n)

    def run(self, scratch, scratch_args, cleanup, calls):
        """`calls`: callables taking the scratch pointer; the operands they use were built before"""
        self.c.st.synchronize()
        start = live_bytes(self.lib)
        mem = C.c_void_p()
        self.lib.hip_integer_scratch_batch(2)
        getattr(self.lib, scratch)(self.s, C.byref(mem), *scratch_args)
        self.lib.hip_integer_scratch_batch(1)
        held = live_bytes(self.lib)
        for call in calls:
            call(mem)
        self.c.st.synchronize()
        getattr(self.lib, cleanup)(self.s, C.byref(mem))
        return start, held, live_bytes(self.lib)


BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
A, B_ = [0x2B7, 0x3FF, 0x155], [0x1C9, 0x001, 0x2AB]     # 10-bit operands; the pair 0x3FF + 1 ripples through every block


def operand_sets(k, seed):
    """operands for calls with 2, 1 and 2 integers"""
    return [(k.enc(a, seed + 2 * i), k.enc(b, seed + 2 * i + 1), a, b)
            for i, (a, b) in enumerate(((A[:2], B_[:2]), (A[2:], B_[2:]), (A[1:], B_[1:])))]


def check_memory(start, held, end):
    assert held > start
    assert end == start, f"{end - start} bytes are still live after the cleanup"


@pytest.mark.parametrize("kind", BACKENDS)
def test_carry_propagation_rebuilds_its_indexes(kind):
    k = Calls(kind)
    sets = operand_sets(k, 700)
    outs = [(k.carries(len(a)), k.carries(len(a))) for _, _, a, _ in sets]
    calls = [lambda mem, x=x, y=y, o=o: k.lib.cuda_add_and_propagate_single_carry_64_inplace_async(
        k.s, C.byref(x._ffi()), C.byref(y._ffi()), C.byref(o[0]._ffi()), C.byref(o[1]._ffi()), mem, k.bsks, k.ksks, 2, 0)
        for (x, y, _, _), o in zip(sets, outs)]
    mem = k.run("scratch_cuda_add_and_propagate_single_carry_64_inplace_async", (*k.radix, 2, True, k.nr),
                "cleanup_cuda_add_and_propagate_single_carry_64_inplace", calls)
    for (x, _, a, b), o in zip(sets, outs):
        assert k.values(x) == [(u + v) & k.mask for u, v in zip(a, b)]
        assert [r[0] for r in k.c.dec(o[0])] == [(u + v) >> (2 * L) for u, v in zip(a, b)]
    check_memory(*mem)


@pytest.mark.parametrize("kind", BACKENDS)
def test_multiplication_rebuilds_its_pass(kind):
    k = Calls(kind)
    sets = operand_sets(k, 710)
    calls = [lambda mem, x=x, y=y: k.lib.cuda_integer_mult_inplace_64_async(
        k.s, C.byref(x._ffi()), False, C.byref(y._ffi()), False, k.bsks, k.ksks, mem, k.c.p.N, L) for x, y, _, _ in sets]
    mem = k.run("scratch_cuda_integer_mult_inplace_64_async", (False, False, MSG, CARRY, *k.radix[:3], True, k.nr),
                "cleanup_cuda_integer_mult_inplace_64", calls)
    for x, _, a, b in sets:
        assert k.values(x) == [(u * v) & k.mask for u, v in zip(a, b)]
    check_memory(*mem)


@pytest.mark.parametrize("kind", BACKENDS)
def test_sum_rebuilds_its_plan(kind):
    """vectors of 2, 1 and 2 integers (an addition, a copy: no index array), then of 6, 5 and 6 (two plans, the first
    one made again)"""
    k = Calls(kind)
    terms = [0x2B7, 0x3FF, 0x155, 0x1C9, 0x001, 0x2AB]
    vecs = [terms[:2], terms[2:3], terms[1:3], terms, terms[1:], terms[::-1]]
    cts = [k.enc(v, 720 + i) for i, v in enumerate(vecs)]
    outs = [k.enc([0], 730 + i) for i in range(len(vecs))]

    def call(mem, vec, out):
        view = vec._ffi()       # the vector as the entry point reads it: V * L blocks of one radix struct
        k.lib.hip_partial_sum_ciphertexts_vec_64_async(k.s, C.byref(out._ffi()), C.byref(view), mem, k.bsks, k.ksks)

    calls = [lambda mem, v=v, o=o: call(mem, v, o) for v, o in zip(cts, outs)]
    mem = k.run("hip_scratch_partial_sum_ciphertexts_vec_64_async", (*k.radix[:3], 6, MSG, CARRY, False, True, k.nr),
                "hip_cleanup_partial_sum_ciphertexts_vec_64", calls)
    for v, o in zip(vecs, outs):
        assert k.values(o)[0] & k.mask == sum(v) & k.mask, v     # blocks may hold carries: the value modulo 2^10
    check_memory(*mem)


def scalar_mul_call(k, ct, scalar):
    bits = [(scalar >> i) & 1 for i in range(scalar.bit_length())]
    decomposed = np.ascontiguousarray(bits, dtype=np.uint64)
    has = np.zeros(2, dtype=np.uint64)
    for i, b in enumerate(bits):
        has[i % 2] |= np.uint64(b)
    return lambda mem: k.lib.hip_integer_scalar_mul_64_async(
        k.s, C.byref(ct._ffi()), decomposed.ctypes.data_as(C.c_void_p), has.ctypes.data_as(C.c_void_p), mem, k.bsks, k.ksks,
        k.c.p.N, MSG, len(bits))


@pytest.mark.parametrize("kind", BACKENDS)
def test_scalar_multiplication_rebuilds_plan_and_indexes(kind):
    """2, 1 and 2 integers times 0xB7; the last of them opens two integers times 0xB7, 3 and 0xB7"""
    k = Calls(kind)
    work = [(A[:2], 0xB7), (A[2:], 0xB7), (A[1:], 0xB7), (B_[1:], 3), (B_[:2], 0xB7)]
    cts = [k.enc(v, 740 + i) for i, (v, _) in enumerate(work)]
    calls = [scalar_mul_call(k, ct, scalar) for ct, (_, scalar) in zip(cts, work)]
    mem = k.run("hip_scratch_integer_scalar_mul_64_async", (*k.radix, 8, True, k.nr), "hip_cleanup_integer_scalar_mul_64", calls)
    for ct, (v, scalar) in zip(cts, work):
        assert k.values(ct) == [(x * scalar) & k.mask for x in v], hex(scalar)
    check_memory(*mem)


@pytest.mark.parametrize("kind", BACKENDS)
def test_arithmetic_shift_rebuilds_its_rows(kind):
    """2, 1 and 2 integers by 3 bits; the last of them opens two integers by 3, 5 and 3 bits"""
    k = Calls(kind)
    work = [(A[:2], 3), (A[2:], 3), (A[1:], 3), (A[:2], 5), (B_[1:], 3)]
    cts = [k.enc(v, 760 + i) for i, (v, _) in enumerate(work)]
    calls = [lambda mem, ct=ct, n=n: k.lib.hip_integer_arithmetic_scalar_shift_64_inplace_async(
        k.s, C.byref(ct._ffi()), n, mem, k.bsks, k.ksks) for ct, (_, n) in zip(cts, work)]
    mem = k.run("hip_scratch_integer_arithmetic_scalar_shift_64_inplace_async", (*k.radix, 1, True, k.nr),
                "hip_cleanup_integer_arithmetic_scalar_shift_64_inplace", calls)
    signed = lambda x: x - (1 << 2 * L) if x >> (2 * L - 1) else x
    for ct, (v, n) in zip(cts, work):
        assert k.values(ct) == [(signed(x) >> n) & k.mask for x in v], n
    check_memory(*mem)
