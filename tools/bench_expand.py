#!/usr/bin/env python3
"""Expansion of compact ciphertext lists on one MI355X: 64, 512 and 2048 bodies (one compact list of n_c = 2048 mask
words, the PKE-to-small casting key of 4 levels of 4 bits) under PARAM_MESSAGE_2_CARRY_2 and under the GPU multi-bit
g = 4 set.  Per body count, with device events around each:

  expand         the expansion kernel alone (a NO_CASTING call), next to hipMemcpyAsync device-to-device of the same
                 number of output bytes, the floor for a kernel that only moves data
  keyswitch      the casting keyswitch of the 2 * bodies blocks of the round, as a call of its own
  bootstrap      the bootstrap of those blocks, as a call of its own
  casting_call   the whole CASTING call (expansion, keyswitch, bootstrap), next to cuda_apply_univariate_lut_64_async on the
                 same 2 * bodies blocks with the compute keys, the existing path with the same keyswitch and bootstrap
                 work: the difference is what expansion and casting cost

Warm-up, then as many repetitions as fill the window.  Uniform-random key material (timing is data independent).  Prints
one JSON line.

  python tools/bench_expand.py                  the measurement
  python tools/bench_expand.py --toy            the same calls on a toy set (any backend library, a second or two)
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import tfhe_rs_amd  # noqa: E402,F401
from tfhe_rs_amd import core_crypto_gpu as gpu  # noqa: E402
from tfhe_rs_amd import ffi  # noqa: E402
from tfhe_rs_amd import integer_gpu as igpu  # noqa: E402

# (name, n, k, N, pbs_base_log, pbs_level, ks_base_log, ks_level, grouping, centered modulus switch)
SETS = [("PARAM_MESSAGE_2_CARRY_2", 918, 1, 2048, 23, 1, 4, 4, 0, True),
        ("PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2", 920, 1, 2048, 22, 1, 3, 5, 4, False)]
TOY = [("toy_classic", 12, 1, 2048, 23, 1, 4, 4, 0, True), ("toy_multi_bit_g4", 8, 1, 2048, 22, 1, 3, 6, 4, False)]
N_C, CAST_BASE_LOG, CAST_LEVEL, MSG = 2048, 4, 4, 4
NO_CASTING, CASTING = 0, 1

lib = ffi.default_library()
streams = gpu.CudaStreams.new_single_gpu(0)
S, G = streams.ptr[0], 0
SF, _keep = igpu.CudaServerKey._streams(streams)
rng = np.random.default_rng(13)


def rand(n):
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


def timed(fn, window_s, warmup=2):
    for _ in range(warmup):
        fn()
    lib.cuda_synchronize_device(G)
    one = max(events_ms(fn, 2), 1e-3)
    reps = int(min(max(window_s * 1e3 / one, 3), 20000))
    return {"ms": events_ms(fn, reps), "reps": reps}


def measure(name, n, k, N, pbs_base_log, pbs_level, ks_base_log, ks_level, grouping, centered, body_counts, window_s):
    big = k * N
    if grouping:
        bsk = gpu.CudaLweMultiBitBootstrapKey.from_lwe_multi_bit_bootstrap_key(
            rand((n // grouping) * (1 << grouping) * (k + 1) ** 2 * pbs_level * N), n, k, N, pbs_base_log, pbs_level,
            grouping, streams)
    else:
        bsk = gpu.CudaLweBootstrapKey.from_lwe_bootstrap_key(rand(n * (k + 1) ** 2 * pbs_level * N), n, k, N, pbs_base_log,
                                                             pbs_level, streams, ms_noise_reduction=centered)
    ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(rand(big * ks_level * (n + 1)), big, n, ks_base_log, ks_level, streams)
    cast = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(rand(N_C * CAST_LEVEL * (n + 1)), N_C, n, CAST_BASE_LOG, CAST_LEVEL,
                                                          streams)
    sks = igpu.CudaServerKey(ksk, bsk, MSG, MSG)
    bk, kk = sks._bsk_params(), sks._ksk_params()
    ck = ffi.CudaLweKeyswitchKeyParamsFFI(N_C, n, CAST_BASE_LOG, CAST_LEVEL)
    ksks, bsks = sks._key_ptrs(streams)
    casts = (C.c_void_p * 1)(cast.d_vec.ptr)
    ms_type = 1 if centered else 0
    out = {"n": n, "glwe_dimension": k, "polynomial_size": N, "grouping": grouping, "n_c": N_C,
           "casting_base_log": CAST_BASE_LOG, "casting_level": CAST_LEVEL}
    lut = np.zeros((k + 1) * N, dtype=np.uint64)
    lut[k * N:] = rand(N)
    for bodies in body_counts:
        blocks = 2 * bodies
        row = {"blocks": blocks, "expanded_bytes": bodies * (N_C + 1) * 8}
        d_in = gpu.CudaVec.from_cpu_async(rand(N_C + bodies), streams)
        d_expanded = gpu.CudaVec(bodies * (N_C + 1), streams)
        d_out = gpu.CudaVec(blocks * (big + 1), streams)
        counts = (C.c_uint32 * 1)(bodies)
        flags = (C.c_bool * blocks)(*([False] * blocks))

        def scratch(kind):
            mem = C.c_void_p()
            lib.hip_scratch_expand_without_verification_64_async(
                SF, C.byref(mem), k, N, kk, ck, pbs_level, pbs_base_log, grouping, counts, flags, blocks, 1, MSG, MSG,
                bk.pbs_type, 0, True, kind, ms_type)
            return mem

        # the expansion kernel against a device-to-device copy of its output bytes
        mem = scratch(NO_CASTING)
        row["expand"] = timed(lambda: lib.hip_expand_without_verification_64_async(SF, d_expanded.ptr, d_in.ptr, mem, None, None,
                                                                                   None), window_s)
        lib.hip_cleanup_expand_without_verification_64(SF, C.byref(mem))
        d_copy = gpu.CudaVec(bodies * (N_C + 1), streams)
        row["copy"] = timed(lambda: lib.cuda_memcpy_async_gpu_to_gpu(d_copy.ptr, d_expanded.ptr, row["expanded_bytes"], S, G),
                            window_s)
        for key in ("expand", "copy"):
            row[key]["GBps_written"] = row["expanded_bytes"] / row[key]["ms"] / 1e6
        row["expand_over_copy"] = row["expand"]["ms"] / row["copy"]["ms"]
        d_copy.drop()
        # the round's two phases as calls of their own: block q reads expanded LWE q mod bodies
        trivial = gpu.CudaVec.from_cpu_async(np.arange(blocks, dtype=np.uint64), streams)
        in_idx = gpu.CudaVec.from_cpu_async(np.arange(blocks, dtype=np.uint64) % bodies, streams)
        lut_idx = gpu.CudaVec(blocks, streams)
        d_small = gpu.CudaVec(blocks * (n + 1), streams)
        d_lut = gpu.CudaVec.from_cpu_async(lut, streams)
        row["keyswitch"] = timed(lambda: lib.cuda_keyswitch_lwe_ciphertext_vector_64_64_async(
            S, G, d_small.ptr, trivial.ptr, d_expanded.ptr, in_idx.ptr, cast.d_vec.ptr, N_C, n, CAST_BASE_LOG, CAST_LEVEL,
            blocks), window_s)
        buf = C.c_void_p()
        if grouping:
            lib.scratch_cuda_multi_bit_programmable_bootstrap_64_async(S, G, C.byref(buf), k, N, pbs_level, blocks, True)
            row["bootstrap"] = timed(lambda: lib.cuda_multi_bit_programmable_bootstrap_64_async(
                S, G, d_out.ptr, trivial.ptr, d_lut.ptr, lut_idx.ptr, d_small.ptr, trivial.ptr, bsk.d_vec.ptr, buf, n, k, N,
                grouping, pbs_base_log, pbs_level, blocks, 1, 0), window_s)
            lib.cleanup_cuda_multi_bit_programmable_bootstrap_64(S, G, C.byref(buf))
        else:
            lib.scratch_cuda_programmable_bootstrap_64_async(S, G, C.byref(buf), n, k, N, pbs_level, blocks, True, ms_type)
            row["bootstrap"] = timed(lambda: lib.cuda_programmable_bootstrap_64_async(
                S, G, d_out.ptr, trivial.ptr, d_lut.ptr, lut_idx.ptr, d_small.ptr, trivial.ptr, bsk.d_vec.ptr, buf, n, k, N,
                pbs_base_log, pbs_level, blocks, 1, 0), window_s)
            lib.cleanup_cuda_programmable_bootstrap_64(S, G, C.byref(buf))
        # the whole CASTING call against apply_univariate_lut on the same number of blocks with the compute keys
        mem = scratch(CASTING)
        row["casting_call"] = timed(lambda: lib.hip_expand_without_verification_64_async(SF, d_out.ptr, d_in.ptr, mem, bsks, ksks,
                                                                                         casts), window_s)
        lib.hip_cleanup_expand_without_verification_64(SF, C.byref(mem))
        ct_in = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec.from_cpu_async(rand(blocks * (big + 1)), streams), 1, blocks, big)
        ct_out = igpu.CudaUnsignedRadixCiphertext(d_out, 1, blocks, big)
        in_ffi, out_ffi = ct_in._ffi(), ct_out._ffi()
        mem = C.c_void_p()
        lib.scratch_cuda_apply_univariate_lut_64_async(SF, C.byref(mem), lut.ctypes.data_as(C.c_void_p), bk, kk, blocks, MSG, MSG,
                                                       MSG - 1, True, ms_type)
        row["apply_lut"] = timed(lambda: lib.cuda_apply_univariate_lut_64_async(SF, C.byref(out_ffi), C.byref(in_ffi), mem, ksks,
                                                                                bsks), window_s)
        lib.cleanup_cuda_apply_univariate_lut_64(SF, C.byref(mem))
        row["casting_call_over_apply_lut"] = row["casting_call"]["ms"] / row["apply_lut"]["ms"]
        row["casting_call_minus_apply_lut_ms"] = row["casting_call"]["ms"] - row["apply_lut"]["ms"]
        out[f"bodies_{bodies}"] = row
        del ct_out
        for v in (d_in, d_expanded, d_out, trivial, in_idx, lut_idx, d_small, d_lut, ct_in.d_blocks):
            v.drop()
    for key in (bsk, ksk, cast):
        for v in key.d_vecs:
            v.drop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--toy", action="store_true")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of repetitions per figure")
    args = ap.parse_args()
    out = {"what": "compact list expansion"}
    if args.toy:
        for s in TOY:
            out[s[0]] = measure(*s, body_counts=(3, 40), window_s=0.0)
    else:
        for s in SETS:
            out[s[0]] = measure(*s, body_counts=(64, 512, 2048), window_s=args.window)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
