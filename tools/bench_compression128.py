#!/usr/bin/env python3
"""Compression of squashed-noise (128-bit) ciphertext lists on one MI355X: for each of the three reference sets
(n_in = 4096, N_c = 1024, 128 blocks per GLWE, 128 stored bits) compress 16, 32, 128 and 1024 squashed blocks under each
kernel selection (automatic, general, matrix core) and unpack 16 and 128 of them; next to it, in the same process, a
device-to-device copy of the key's byte count (how close the packing keyswitch is to streaming the key once).  Device
events, warm-up, then as many repetitions as fill the window.  Uniform-random key material (timing is data independent).
Prints one JSON line.

  python tools/bench_compression128.py                  the measurement
  python tools/bench_compression128.py --toy            the same calls on a toy set (any backend library, a second or two)
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

# (name, n_in, k_c, N_c, base_log, level, lwe_per_glwe): the noise-squashing compression sets of
# shortint/parameters/*/noise_squashing
SETS = [("b61_l1_k6", 4096, 6, 1024, 61, 1, 128), ("b41_l2_k6", 4096, 6, 1024, 41, 2, 128),
        ("b33_l2_k5", 4096, 5, 1024, 33, 2, 128)]
TOY = [("toy_b33_l2", 64, 1, 64, 33, 2, 16)]
STORAGE_BITS, MSG = 128, 4
SELECTIONS = {"auto": 0, "general": 1, "matrix": 2}

lib = ffi.default_library()
streams = gpu.CudaStreams.new_single_gpu(0)
S, G = streams.ptr[0], 0
SF, _keep = igpu.CudaServerKey._streams(streams)
rng = np.random.default_rng(12)


def rand_u128(n):
    return rng.integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)


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
    return events_ms(fn, reps), reps


def measure(name, n_in, kc, nc, base_log, level, per, block_counts, unpack_counts, window_s):
    ncols = (kc + 1) * nc
    pksk = gpu.CudaLwePackingKeyswitchKey128.from_lwe_packing_keyswitch_key(
        rand_u128(n_in * level * ncols), n_in, kc, nc, base_log, level, streams)
    key_bytes = pksk.size_bytes()
    out = {"n_in": n_in, "glwe_dimension": kc, "polynomial_size": nc, "base_log": base_log, "level": level,
           "lwe_per_glwe": per, "key_bytes": key_bytes, "matrix_planes": pksk.d_planes is not None}
    copy_dst = gpu.CudaVec(key_bytes // 8, streams)
    ms, reps = timed(lambda: lib.cuda_memcpy_async_gpu_to_gpu(copy_dst.ptr, pksk.d_vec.ptr, key_bytes, S, G), window_s)
    out["key_copy_ms"], out["key_copy_GBps"] = ms, key_bytes / ms / 1e6
    copy_dst.drop()
    keys, planes = (C.c_void_p * 1)(pksk.d_vec.ptr), (C.c_void_p * 1)(pksk.planes_ptr)
    most = max(block_counts)
    blocks = gpu.CudaVec.from_cpu_async(rand_u128(most * (n_in + 1)), streams, elem_words=2)
    words = int(lib.hip_integer_compressed_size_words_128(kc, nc, per, STORAGE_BITS, most))
    packed = gpu.CudaVec(words, streams, elem_words=2)
    for count in block_counts:
        ct = igpu.CudaSquashedNoiseRadixCiphertext(blocks, count, n_in, 2 * count)
        ct_ffi = ct._ffi()
        mem = C.c_void_p()
        lib.hip_scratch_integer_compress_radix_ciphertext_128_async(SF, C.byref(mem), n_in, kc, nc, base_log, level, count, MSG,
                                                                    MSG, per, STORAGE_BITS, True)
        row = {}
        for sel, mode in SELECTIONS.items():
            lib.hip_backend_set_pks128_kernel(mode)
            ms, reps = timed(lambda: lib.hip_integer_compress_radix_ciphertext_128_async(SF, packed.ptr, C.byref(ct_ffi), keys,
                                                                                         planes, mem), window_s)
            row[sel] = {"ms": ms, "reps": reps, "path": int(lib.hip_backend_last_pks128_path()),
                        "over_key_copy": ms / out["key_copy_ms"]}
        lib.hip_backend_set_pks128_kernel(0)
        lib.hip_cleanup_integer_compress_radix_ciphertext_128(SF, C.byref(mem))
        row["packed_bytes"] = 16 * int(lib.hip_integer_compressed_size_words_128(kc, nc, per, STORAGE_BITS, count))
        row["plain_bytes"] = 16 * count * (n_in + 1)
        out[f"compress_{count}"] = row
    for count in unpack_counts:
        dim = kc * nc
        dst = igpu.CudaSquashedNoiseRadixCiphertext(gpu.CudaVec(count * (dim + 1), streams, elem_words=2), count, dim, 2 * count)
        dst_ffi = dst._ffi()
        idx = np.arange(count, dtype=np.uint32)
        mem = C.c_void_p()
        lib.hip_scratch_integer_decompress_radix_ciphertext_128_async(SF, C.byref(mem), kc, nc, per, STORAGE_BITS, count, MSG, MSG,
                                                                      True)
        ms, reps = timed(lambda: lib.hip_integer_decompress_radix_ciphertext_128_async(
            SF, C.byref(dst_ffi), packed.ptr, most, idx.ctypes.data_as(C.POINTER(C.c_uint32)), count, mem), window_s)
        lib.hip_cleanup_integer_decompress_radix_ciphertext_128(SF, C.byref(mem))
        out[f"unpack_{count}"] = {"ms": ms, "reps": reps}
    for v in (blocks, packed, pksk.d_vec, pksk.d_planes):
        if v is not None:
            v.drop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--toy", action="store_true")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of repetitions per figure")
    args = ap.parse_args()
    out = {"what": "squashed-noise list compression", "storage_log_modulus": STORAGE_BITS}
    if args.toy:
        for s in TOY:
            out[s[0]] = measure(*s, block_counts=(3, 40), unpack_counts=(3,), window_s=0.0)
    else:
        for s in SETS:
            out[s[0]] = measure(*s, block_counts=(16, 32, 128, 1024), unpack_counts=(16, 128), window_s=args.window)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
