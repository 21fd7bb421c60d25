#!/usr/bin/env python3
"""Re-randomisation on one MI355X: 64, 512 and 2048 blocks at the PARAM_MESSAGE_2_CARRY_2 big dimension (2048), the zeros
one compact list of 2048 mask words.  Per block count, with device events around each:

  fused          the rotate-and-add kernel alone (a RERAND_WITHOUT_KS call), next to
  expand_add     launch_lwe_expand into a temporary (a NO_CASTING expansion call) followed by the library's LWE addition
                 (cuda_add_lwe_ciphertext_vector_inplace_64): the reference's structure, same tree, same process, and to
  copy           hipMemcpyAsync device-to-device of the same block bytes, the floor for a kernel that reads and writes
                 every block once
  with_ks_call   the whole RERAND_WITH_KS call (expand, keyswitch 2048 -> 2048 with one level of 24 bits, row add), next to
  keyswitch      that keyswitch alone on already expanded zeros

Warm-up, then as many repetitions as fill the window.  Uniform-random words (timing is data independent).  Nothing is
asserted.  Prints one JSON line.

  python tools/bench_rerand.py                  the measurement
  python tools/bench_rerand.py --toy            the same calls on small shapes (any backend library, a second or two)
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

KS_BASE_LOG, KS_LEVEL, MSG = 24, 1, 4
RERAND_WITH_KS, RERAND_WITHOUT_KS = 0, 1
NO_CASTING = 0

lib = ffi.default_library()
streams = gpu.CudaStreams.new_single_gpu(0)
S, G = streams.ptr[0], 0
SF, _keep = igpu.CudaServerKey._streams(streams)
rng = np.random.default_rng(17)


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


def measure(n, block_counts, window_s):
    KK = ffi.CudaLweKeyswitchKeyParamsFFI
    ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(rand(n * KS_LEVEL * (n + 1)), n, n, KS_BASE_LOG, KS_LEVEL, streams)
    keys = (C.c_void_p * 1)(ksk.d_vec.ptr)
    out = {"lwe_dimension": n, "ks_base_log": KS_BASE_LOG, "ks_level": KS_LEVEL}
    for count in block_counts:
        row = {"block_bytes": count * (n + 1) * 8}
        blocks = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec.from_cpu_async(rand(count * (n + 1)), streams), 1, count, n)
        zeros = gpu.CudaVec.from_cpu_async(rand(n + count), streams)
        expanded = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec(count * (n + 1), streams), 1, count, n)
        blocks_ffi, expanded_ffi = blocks._ffi(), expanded._ffi()

        # the fused kernel
        mem = C.c_void_p()
        lib.hip_scratch_rerand_64_async(SF, C.byref(mem), KK(n, 0, 0, 0), count, MSG, MSG, True, RERAND_WITHOUT_KS)
        row["fused"] = timed(lambda: lib.hip_rerand_64_async(SF, blocks.d_blocks.ptr, zeros.ptr, mem, None), window_s)
        lib.hip_cleanup_rerand_64(SF, C.byref(mem))

        # the reference's structure: expand into a temporary, then add
        counts = (C.c_uint32 * 1)(count)
        flags = (C.c_bool * 1)(False)
        lib.hip_scratch_expand_without_verification_64_async(SF, C.byref(mem), 1, n, KK(n, n, 4, 4), KK(n, n, 4, 4), 1, 23, 0,
                                                             counts, flags, 0, 1, MSG, MSG, 1, 0, True, NO_CASTING, 0)

        def expand_add():
            lib.hip_expand_without_verification_64_async(SF, expanded.d_blocks.ptr, zeros.ptr, mem, None, None, None)
            lib.cuda_add_lwe_ciphertext_vector_inplace_64(S, G, C.byref(blocks_ffi), C.byref(expanded_ffi))

        row["expand_add"] = timed(expand_add, window_s)
        lib.hip_cleanup_expand_without_verification_64(SF, C.byref(mem))

        # a device-to-device copy of the same block bytes
        row["copy"] = timed(lambda: lib.cuda_memcpy_async_gpu_to_gpu(expanded.d_blocks.ptr, blocks.d_blocks.ptr,
                                                                      row["block_bytes"], S, G), window_s)
        for key in ("fused", "expand_add", "copy"):
            row[key]["GBps_of_block_bytes"] = row["block_bytes"] / row[key]["ms"] / 1e6
        row["fused_over_expand_add"] = row["fused"]["ms"] / row["expand_add"]["ms"]
        row["fused_over_copy"] = row["fused"]["ms"] / row["copy"]["ms"]

        # the keyswitch mode against its keyswitch alone
        lib.hip_scratch_rerand_64_async(SF, C.byref(mem), KK(n, n, KS_BASE_LOG, KS_LEVEL), count, MSG, MSG, True,
                                        RERAND_WITH_KS)
        row["with_ks_call"] = timed(lambda: lib.hip_rerand_64_async(SF, blocks.d_blocks.ptr, zeros.ptr, mem, keys), window_s)
        lib.hip_cleanup_rerand_64(SF, C.byref(mem))
        trivial = gpu.CudaVec.from_cpu_async(np.arange(count, dtype=np.uint64), streams)
        switched = gpu.CudaVec(count * (n + 1), streams)
        row["keyswitch"] = timed(lambda: lib.cuda_keyswitch_lwe_ciphertext_vector_64_64_async(
            S, G, switched.ptr, trivial.ptr, expanded.d_blocks.ptr, trivial.ptr, ksk.d_vec.ptr, n, n, KS_BASE_LOG, KS_LEVEL,
            count), window_s)
        row["with_ks_call_over_keyswitch"] = row["with_ks_call"]["ms"] / row["keyswitch"]["ms"]
        row["with_ks_call_minus_keyswitch_ms"] = row["with_ks_call"]["ms"] - row["keyswitch"]["ms"]
        out[f"blocks_{count}"] = row
        for v in (blocks.d_blocks, zeros, expanded.d_blocks, trivial, switched):
            v.drop()
    for v in ksk.d_vecs:
        v.drop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--toy", action="store_true")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of repetitions per figure")
    args = ap.parse_args()
    out = {"what": "re-randomisation"}
    if args.toy:
        out["toy"] = measure(64, (3, 40), 0.0)
    else:
        out["PARAM_MESSAGE_2_CARRY_2"] = measure(2048, (64, 512, 2048), args.window)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
