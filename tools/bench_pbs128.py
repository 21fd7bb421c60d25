#!/usr/bin/env python3
"""The 128-bit programmable bootstrap on one MI355X at the production noise-squashing set (k = 2, N = 2048, 3 levels of
24 bits, centred switch, n = 918): key conversion, the bootstrap at batch 1, 16 (one packed FheUint64), 128, 256, 1024
and 4096, and the squashing of one FheUint64 (32 blocks of PARAM_MESSAGE_2_CARRY_2: pack, keyswitch, bootstrap of 16).
Device events around the launches, a warm-up, then as many repetitions as fill about a second (at least two).
Uniform-random key material and inputs: the time does not depend on the data.  Prints one JSON line.

  python tools/bench_pbs128.py [--batches 1,16,...] [--n 918] [--window 1.0]
  python tools/bench_pbs128.py --grouping 4 [--batches 1,16,...] [--n 920] [--window 1.0]

--grouping G: the multi-bit 128-bit bootstrap at the production multi-bit squashing set instead (k = 2, N = 2048, 4 levels of
18 bits, plain switch, n = 920 on PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2): key upload, the bootstrap at batch 1, 16,
128, 256 and 1024, the squashing of one FheUint64.  The key is uniformly random words, not valid GGSWs (4.3 GB of them are
not worth generating to take a time); the output says so.

TFHE_HIP_BACKEND_LIB selects another build of the library (tests/test_pbs128.py runs the tool once on the host emulation with a
short key, so that its argument lists are exercised without a device).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import tfhe_rs_amd  # noqa: E402,F401
from tfhe_rs_amd import core_crypto_gpu as gpu  # noqa: E402
from tfhe_rs_amd import ffi  # noqa: E402
from tfhe_rs_amd import integer_gpu as igpu  # noqa: E402
from tests.common import C1, C4G4  # noqa: E402

K, N, BASE_LOG, LEVEL, MS_CENTERED = 2, 2048, 24, 3, 1

lib = ffi.default_library()
streams = gpu.CudaStreams.new_single_gpu(0)
S, G = streams.ptr[0], 0
rng = np.random.default_rng(128)


def rand_u64(n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


def events_ms(fn, reps):
    e0, e1 = lib.hip_event_create(), lib.hip_event_create()
    lib.hip_event_record(e0, S)
    for _ in range(reps):
        fn()
    lib.hip_event_record(e1, S)
    ms = lib.hip_event_elapsed_ms(e0, e1) / reps
    lib.hip_event_destroy(e0)
    lib.hip_event_destroy(e1)
    return ms


WINDOW_S = 1.0


def timed(fn, window_s=None):
    window_s = WINDOW_S if window_s is None else window_s
    fn()
    lib.cuda_synchronize_device(G)
    one = max(events_ms(fn, 1), 1e-3)
    reps = int(min(max(window_s * 1e3 / one, 2), 2000))
    return events_ms(fn, reps), reps


MB_BASE_LOG, MB_LEVEL = 18, 4


def main_multi_bit(n, g, batches, cap_mib):
    """the same figures on the multi-bit squashing set; the key stays in the standard domain, so "conversion" is an upload"""
    per_group = MB_LEVEL * (K + 1) * (K + 1) * 16 * N   # bundle bytes of one group of one sample

    def set_chunk(samples):   # the library's rule (largest number of groups under the cap, at least one) for another cap
        lib.hip_backend_set_pbs128_multibit_chunk(max(1, (cap_mib << 20) // (samples * per_group)) if cap_mib else 0)
    out = {"what": "multi-bit 128-bit programmable bootstrap", "n": n, "grouping_factor": g, "glwe_dimension": K,
           "polynomial_size": N, "base_log": MB_BASE_LOG, "level": MB_LEVEL, "centered_modulus_switch": False,
           "key": "uniformly random words, not valid GGSWs: the time does not depend on the data",
           "bundle_cap_mib": cap_mib or "library default"}
    h_key = rand_u64((n // g) * (1 << g) * MB_LEVEL * (K + 1) * (K + 1) * N * 2).reshape(-1, 2)
    out["key_bytes"] = int(h_key.nbytes)
    t0 = time.perf_counter()
    bsk = gpu.CudaLweMultiBitBootstrapKey128.from_lwe_multi_bit_bootstrap_key(h_key, n, K, N, MB_BASE_LOG, MB_LEVEL, g, streams)
    out["key_upload_first_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lib.hip_convert_lwe_multi_bit_programmable_bootstrap_key_128_async(S, G, bsk.d_vec.ptr, h_key.ctypes.data_as(C.c_void_p), n,
                                                                       K, MB_LEVEL, N, g)
    streams.synchronize()
    out["key_upload_s"] = time.perf_counter() - t0
    del h_key
    d_lut = gpu.CudaVec.from_cpu_async(rand_u64((K + 1) * N * 2).reshape(-1, 2), streams, elem_words=2)
    out["bootstrap"] = {}
    for B in batches:
        d_in = gpu.CudaVec.from_cpu_async(rand_u64(B * (n + 1)), streams)
        d_idx = gpu.CudaVec.from_cpu_async(np.arange(B, dtype=np.uint64), streams)
        d_out = gpu.CudaVec(B * (K * N + 1), streams, elem_words=2)
        buf = C.c_void_p()
        set_chunk(B)
        bytes_ = lib.hip_scratch_multi_bit_programmable_bootstrap_128_async(S, G, C.byref(buf), K, N, MB_LEVEL, B, True)
        ms, reps = timed(lambda: lib.hip_multi_bit_programmable_bootstrap_128_async(
            S, G, d_out.ptr, d_idx.ptr, d_lut.ptr, d_in.ptr, d_idx.ptr, bsk.d_vec.ptr, buf, n, K, N, g, MB_BASE_LOG, MB_LEVEL, B,
            1, 0))
        lib.hip_cleanup_multi_bit_programmable_bootstrap_128(S, G, C.byref(buf))
        out["bootstrap"][str(B)] = {"ms": ms, "reps": reps, "pbs_per_s": B / ms * 1e3, "scratch_bytes": int(bytes_)}
        for d in (d_in, d_idx, d_out):
            d.drop()
    p = C4G4
    ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(rand_u64(p.big_n * p.ks_level * (n + 1)), p.big_n, n, p.ks_base_log,
                                                         p.ks_level, streams)
    ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(rand_u64(32 * (p.big_n + 1)).reshape(1, 32, -1), streams)
    sq = igpu.CudaSquashedNoiseRadixCiphertext(gpu.CudaVec(16 * (K * N + 1), streams, elem_words=2), 16, K * N, 32)
    SF, _keep = igpu.CudaServerKey._streams(streams)
    mem = C.c_void_p()
    set_chunk(16)
    lib.hip_scratch_integer_apply_noise_squashing_multi_bit_64_async(SF, C.byref(mem), n, K, N, p.k, p.N, p.ks_level,
                                                                     p.ks_base_log, MB_LEVEL, MB_BASE_LOG, 16, 32, 4, 4, True, 0, g)
    ksks, bsks = (C.c_void_p * 1)(ksk.d_vec.ptr), (C.c_void_p * 1)(bsk.d_vec.ptr)
    ct_ffi, sq_ffi = ct._ffi(), sq._ffi()
    ms, reps = timed(lambda: lib.hip_integer_apply_noise_squashing_64_async(SF, C.byref(sq_ffi), C.byref(ct_ffi), mem, ksks, bsks))
    lib.hip_cleanup_integer_apply_noise_squashing_64(SF, C.byref(mem))
    out["squash_fheuint64"] = {"ms": ms, "reps": reps, "input_blocks": 32, "output_blocks": 16}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default=None)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of repetitions per figure")
    ap.add_argument("--grouping", type=int, default=0, help="grouping factor: time the multi-bit 128-bit bootstrap instead")
    ap.add_argument("--cap-mib", type=int, default=0,
                    help="with --grouping: size the groups per pass for this many MiB of key bundles (0: the library's cap)")
    args = ap.parse_args()
    global WINDOW_S
    WINDOW_S = args.window
    if args.grouping:
        return main_multi_bit(args.n or C4G4.n, args.grouping, [int(b) for b in (args.batches or "1,16,128,256,1024").split(",")],
                              args.cap_mib)
    n = args.n or C1.n
    batches = [int(b) for b in (args.batches or "1,16,128,256,1024,4096").split(",")]
    out = {"what": "128-bit programmable bootstrap", "n": n, "glwe_dimension": K, "polynomial_size": N, "base_log": BASE_LOG,
           "level": LEVEL, "centered_modulus_switch": bool(MS_CENTERED)}
    h_key = rand_u64(n * LEVEL * (K + 1) * (K + 1) * N * 2).reshape(-1, 2)
    out["key_bytes"] = int(h_key.nbytes)
    t0 = time.perf_counter()
    bsk = gpu.CudaLweBootstrapKey128.from_lwe_bootstrap_key(h_key, n, K, N, BASE_LOG, LEVEL, streams,
                                                            ms_noise_reduction=bool(MS_CENTERED))
    out["key_conversion_first_s"] = time.perf_counter() - t0   # tables, allocation, upload, transform
    t0 = time.perf_counter()
    lib.hip_convert_lwe_programmable_bootstrap_key_128_async(S, G, bsk.d_vec.ptr, h_key.ctypes.data_as(C.c_void_p), n, K, LEVEL,
                                                             N)
    streams.synchronize()
    out["key_conversion_s"] = time.perf_counter() - t0            # upload + transform of a second conversion
    del h_key
    d_lut = gpu.CudaVec.from_cpu_async(rand_u64((K + 1) * N * 2).reshape(-1, 2), streams, elem_words=2)
    out["bootstrap"] = {}
    for B in batches:
        d_in = gpu.CudaVec.from_cpu_async(rand_u64(B * (n + 1)), streams)
        d_out = gpu.CudaVec(B * (K * N + 1), streams, elem_words=2)
        buf = C.c_void_p()
        lib.hip_scratch_programmable_bootstrap_128_async(S, G, C.byref(buf), n, K, N, LEVEL, B, True, MS_CENTERED)
        ms, reps = timed(lambda: lib.hip_programmable_bootstrap_128_async(S, G, d_out.ptr, d_lut.ptr, d_in.ptr, bsk.d_vec.ptr,
                                                                          buf, n, K, N, BASE_LOG, LEVEL, B))
        lib.hip_cleanup_programmable_bootstrap_128(S, G, C.byref(buf))
        out["bootstrap"][str(B)] = {"ms": ms, "reps": reps, "pbs_per_s": B / ms * 1e3}
        d_in.drop()
        d_out.drop()
    # squashing of one FheUint64: 32 blocks under the compute set's big key -> 16 u128 blocks
    p = C1
    ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(rand_u64(p.big_n * p.ks_level * (n + 1)), p.big_n, n, p.ks_base_log,
                                                         p.ks_level, streams)
    ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(rand_u64(32 * (p.big_n + 1)).reshape(1, 32, -1), streams)
    sq = igpu.CudaSquashedNoiseRadixCiphertext(gpu.CudaVec(16 * (K * N + 1), streams, elem_words=2), 16, K * N, 32)
    SF, _keep = igpu.CudaServerKey._streams(streams)
    mem = C.c_void_p()
    lib.hip_scratch_integer_apply_noise_squashing_64_async(SF, C.byref(mem), n, K, N, p.k, p.N, p.ks_level, p.ks_base_log, LEVEL,
                                                           BASE_LOG, 16, 32, 4, 4, True, MS_CENTERED)
    ksks, bsks = (C.c_void_p * 1)(ksk.d_vec.ptr), (C.c_void_p * 1)(bsk.d_vec.ptr)
    ct_ffi, sq_ffi = ct._ffi(), sq._ffi()
    ms, reps = timed(lambda: lib.hip_integer_apply_noise_squashing_64_async(SF, C.byref(sq_ffi), C.byref(ct_ffi), mem, ksks, bsks))
    lib.hip_cleanup_integer_apply_noise_squashing_64(SF, C.byref(mem))
    out["squash_fheuint64"] = {"ms": ms, "reps": reps, "input_blocks": 32, "output_blocks": 16}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
