#!/usr/bin/env python3
"""Ciphertext compression on one MI355X: compress and decompress of one FheUint64 (32 blocks) and of 4096 blocks
(16 GLWEs) at the reference's set on PARAM_MESSAGE_2_CARRY_2, next to the two launches they are made of — the LWE
keyswitch of 4096 blocks and the headline bootstrap of 4096 at n = 918 — in the same process.  Device events, warm-up,
then as many repetitions as fill about a second.  Uniform-random key material (timing is data independent, as in
tools/measure_all.py).  Prints one JSON line.

  python tools/bench_compression.py                       the measurement
  python tools/bench_compression.py --trace               three compress + decompress of 4096 blocks and nothing else:
                                                          the program to run under `rocprofv3 --kernel-trace --stats`
  python tools/bench_compression.py --kernel-stats F.csv  the measurement, with the kernel split read from the
                                                          *_kernel_stats.csv such a run wrote
"""
import argparse
import csv
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
from tests.common import C1  # noqa: E402

# shortint/parameters/v1_7/list_compression/p_fail_2_minus_128/mod.rs:11-37
KC, NC, KS_BASE_LOG, KS_LEVEL, LWE_PER_GLWE, STORAGE_BITS, MSG = 4, 256, 4, 3, 256, 12, 4

lib = ffi.default_library()
streams = gpu.CudaStreams.new_single_gpu(0)
S, G = streams.ptr[0], 0
SF, _keep = igpu.CudaServerKey._streams(streams)
rng = np.random.default_rng(11)


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


def timed(fn, window_s=1.0, warmup=3):
    for _ in range(warmup):
        fn()
    lib.cuda_synchronize_device(G)
    one = max(events_ms(fn, 2), 1e-3)
    reps = int(min(max(window_s * 1e3 / one, 5), 20000))
    return events_ms(fn, reps), reps


class Compression:
    def __init__(self, blocks):
        p = C1
        self.blocks = blocks
        self.pksk = gpu.CudaLwePackingKeyswitchKey.from_lwe_packing_keyswitch_key(
            rand_u64(p.big_n * KS_LEVEL * (KC + 1) * NC), p.big_n, KC, NC, KS_BASE_LOG, KS_LEVEL, streams)
        n = KC * NC
        self.dbsk = gpu.CudaLweBootstrapKey.from_lwe_bootstrap_key(rand_u64(n * 4 * p.N), n, p.k, p.N, p.pbs_base_log,
                                                                   p.pbs_level, streams, ms_noise_reduction=bool(p.ms_type))
        self.ct = igpu.CudaUnsignedRadixCiphertext.from_blocks(rand_u64(blocks * (p.big_n + 1)).reshape(1, blocks, -1), streams)
        self.out = igpu.CudaUnsignedRadixCiphertext.zeros_like(self.ct, streams)
        self.words = int(lib.hip_integer_compressed_size_words(KC, NC, LWE_PER_GLWE, STORAGE_BITS, blocks))
        self.packed = gpu.CudaVec(self.words, streams)
        self.cmem, self.dmem = C.c_void_p(), C.c_void_p()
        lib.hip_scratch_integer_compress_radix_ciphertext_64_async(
            SF, C.byref(self.cmem), p.big_n, KC, NC, KS_BASE_LOG, KS_LEVEL, blocks, MSG, MSG, LWE_PER_GLWE, STORAGE_BITS, True)
        bk = ffi.CudaLweBootstrapKeyParamsFFI(n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.big_n, 1, 0)
        lib.hip_scratch_integer_decompress_radix_ciphertext_64_async(
            SF, C.byref(self.dmem), bk, KC, NC, LWE_PER_GLWE, STORAGE_BITS, blocks, MSG, MSG, True, p.ms_type)
        self.pk = (C.c_void_p * 1)(self.pksk.d_vec.ptr)
        self.bk = (C.c_void_p * 1)(self.dbsk.d_vec.ptr)
        self.idx = np.arange(blocks, dtype=np.uint32)
        self.ct_ffi, self.out_ffi = self.ct._ffi(), self.out._ffi()

    def compress(self):
        lib.hip_integer_compress_radix_ciphertext_64_async(SF, self.packed.ptr, C.byref(self.ct_ffi), self.pk, self.cmem)

    def decompress(self):
        lib.hip_integer_decompress_radix_ciphertext_64_async(
            SF, C.byref(self.out_ffi), self.packed.ptr, self.blocks, self.idx.ctypes.data_as(C.POINTER(C.c_uint32)),
            self.blocks, self.bk, self.dmem)

    def close(self):
        lib.hip_cleanup_integer_compress_radix_ciphertext_64(SF, C.byref(self.cmem))
        lib.hip_cleanup_integer_decompress_radix_ciphertext_64(SF, C.byref(self.dmem))


def keyswitch_4096():
    p, B = C1, 4096
    ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(rand_u64(p.big_n * p.ks_level * (p.n + 1)), p.big_n, p.n,
                                                         p.ks_base_log, p.ks_level, streams)
    d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(rand_u64(B * (p.big_n + 1)).reshape(B, -1), streams)
    d_out = gpu.CudaLweCiphertextList.new(p.n, B, streams)
    idx = gpu.CudaVec.from_cpu_async(np.arange(B, dtype=np.uint64), streams)
    return timed(lambda: gpu.cuda_keyswitch_lwe_ciphertext(ksk, d_in, d_out, idx, idx, True, streams))


def bootstrap_4096():
    p, B = C1, 4096
    bsk = gpu.CudaLweBootstrapKey.from_lwe_bootstrap_key(rand_u64(p.n * 4 * p.N), p.n, p.k, p.N, p.pbs_base_log, p.pbs_level,
                                                         streams, ms_noise_reduction=bool(p.ms_type))
    d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(rand_u64(B * (p.n + 1)).reshape(B, -1), streams)
    d_out = gpu.CudaLweCiphertextList.new(p.big_n, B, streams)
    d_lut = gpu.CudaGlweCiphertextList.from_glwe_ciphertext_list(rand_u64(2 * p.N), p.k, p.N, streams)
    idx = gpu.CudaVec.from_cpu_async(np.arange(B, dtype=np.uint64), streams)
    lidx = gpu.CudaVec.from_cpu_async(np.zeros(B, dtype=np.uint64), streams)
    buf = C.c_void_p()
    lib.scratch_cuda_programmable_bootstrap_64_async(S, G, C.byref(buf), p.n, p.k, p.N, p.pbs_level, B, True, p.ms_type)
    res = timed(lambda: lib.cuda_programmable_bootstrap_64_async(
        S, G, d_out.d_vec.ptr, idx.ptr, d_lut.d_vec.ptr, lidx.ptr, d_in.d_vec.ptr, idx.ptr, bsk.d_vec.ptr, buf, p.n, p.k,
        p.N, p.pbs_base_log, p.pbs_level, B, 1, 0))
    lib.cleanup_cuda_programmable_bootstrap_64(S, G, C.byref(buf))
    return res


def kernel_split(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            rows.append({"kernel": name.split("(")[0][:80], "calls": int(float(r.get("Calls", 0) or 0)),
                         "total_ms": float(r.get("TotalDurationNs", 0) or 0) / 1e6,
                         "percent": float(r.get("Percentage", 0) or 0)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats")
    args = ap.parse_args()
    if args.trace:
        c = Compression(4096)
        for _ in range(3):
            c.compress()
            c.decompress()
        streams.synchronize()
        c.close()
        return
    out = {"what": "ciphertext compression", "params": C1.name,
           "compression": {"glwe_dimension": KC, "polynomial_size": NC, "ks_base_log": KS_BASE_LOG, "ks_level": KS_LEVEL,
                           "lwe_per_glwe": LWE_PER_GLWE, "storage_log_modulus": STORAGE_BITS}}
    for blocks in (32, 4096):
        c = Compression(blocks)
        cms, creps = timed(c.compress)
        path = int(lib.hip_backend_last_keyswitch_path())
        dms, dreps = timed(c.decompress)
        out[f"blocks_{blocks}"] = {"compress_ms": cms, "compress_reps": creps, "keyswitch_path": path, "decompress_ms": dms,
                                   "decompress_reps": dreps, "packed_bytes": c.words * 8,
                                   "plain_bytes": blocks * (C1.big_n + 1) * 8, "pbs_kernel_id": int(lib.hip_backend_last_pbs_kernel())}
        c.close()
    ks_ms, ks_reps = keyswitch_4096()
    pbs_ms, pbs_reps = bootstrap_4096()
    out["keyswitch_4096_ms"], out["bootstrap_4096_n918_ms"] = ks_ms, pbs_ms
    out["compress_4096_over_keyswitch"] = out["blocks_4096"]["compress_ms"] / ks_ms
    out["compress_4096_expected_at_most_ms"] = 2 * 1.39 * ks_ms
    out["decompress_4096_over_bootstrap"] = out["blocks_4096"]["decompress_ms"] / pbs_ms
    out["decompress_4096_expected_ratio"] = 1024 / 918
    if args.kernel_stats:
        out["kernel_split"] = kernel_split(args.kernel_stats)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
