#!/usr/bin/env python3
"""FheUint64 times a clear 64-bit scalar on ONE GPU, through the radix layer of the backend (tfhe_rs_amd/integer_gpu.py):
the scalars all-ones, one random and 3, one integer (latency) and a batch (ops/s), PBS per operation, with mul_assign
(ciphertext x ciphertext) of the same build beside it for scale; and the two column-sum kernels on the same single-pool
groups.  One JSON line per measurement; results are checked against clear arithmetic outside the timed region.

The reference measures scalar_mul in tfhe-benchmark/benches/integer/bench.rs; its published numbers are for other
hardware and are not compared here."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import radix_model as rm  # noqa: E402  (encryption and the checker only)
from tests.common import C1, C4G4, make_keys  # noqa: E402

U64 = np.uint64


def kernel_comparison(gpu, lib, st, repeats, launches):
    """lwe_group_sum_kernel against lwe_gather_sum2_kernel: 640 groups of 5 rows of 2,049 words (a reduction step of a
    32-block integer times the all-ones scalar) and 32 groups of 2 rows (its final sums); `repeats` timings of `launches`
    launches each, the outputs compared word for word first."""
    words = 2049
    rng = np.random.default_rng(7)
    for name, groups, size in (("640 groups of 5 rows", 640, 5), ("32 groups of 2 rows (final sums)", 32, 2)):
        rows = groups * size
        pool = rng.integers(0, 1 << 63, size=(rows, words), dtype=U64)
        members = rng.permutation(rows).astype(U64)
        offsets = (np.arange(groups + 1) * size).astype(U64)
        d_pool, d_mem, d_off = (gpu.CudaVec.from_cpu_async(x.reshape(-1), st) for x in (pool, members, offsets))
        outs = [gpu.CudaVec(groups * words, st), gpu.CudaVec(groups * words, st)]
        want = pool[members.astype(np.int64)].reshape(groups, size, words).sum(axis=1, dtype=U64)
        e0, e1 = lib.hip_event_create(), lib.hip_event_create()
        result = {"what": "column-sum kernels", "case": name, "words": words, "launches_per_timing": launches}
        for which, kernel in ((0, "lwe_group_sum_kernel"), (1, "lwe_gather_sum2_kernel")):
            def launch():
                lib.hip_test_group_sum_async(st.ptr[0], st.gpu_indexes[0], which, outs[which].ptr, d_pool.ptr, d_off.ptr,
                                             d_mem.ptr, words, groups)
            launch()
            assert np.array_equal(outs[which].copy_to_cpu(st).reshape(groups, words), want), kernel
            for _ in range(10):
                launch()
            us = []
            for _ in range(repeats):
                st.synchronize()
                lib.hip_event_record(e0, st.ptr[0])
                for _ in range(launches):
                    launch()
                lib.hip_event_record(e1, st.ptr[0])
                us.append(1e3 * lib.hip_event_elapsed_ms(e0, e1) / launches)
            result[kernel + "_us"] = [round(u, 3) for u in us]
        lib.hip_event_destroy(e0)
        lib.hip_event_destroy(e1)
        print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--params", default="classic,multibit_g4",
                    help="classic = PARAM_MESSAGE_2_CARRY_2, multibit_g4 = PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-operations", action="store_true")
    args = ap.parse_args()
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import ffi
    from tfhe_rs_amd import integer_gpu as igpu
    lib = ffi.default_library()
    st = gpu.CudaStreams([0])
    if not args.skip_kernels:
        kernel_comparison(gpu, lib, st, args.repeats, args.launches)
    if args.skip_operations:
        return
    L, m = args.blocks, 4
    mask = (1 << (2 * L)) - 1
    rng = np.random.default_rng(1)
    scalars = [("all_ones", mask), ("random", int.from_bytes(rng.bytes(8), "little") & mask | 1 << (2 * L - 1)), ("three", 3)]
    for name in args.params.split(","):
        p = {"classic": C1, "multibit_g4": C4G4}[name]
        keys = make_keys(p)
        ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(keys.ksk, p.big_n, p.n, p.ks_base_log, p.ks_level, st)
        if p.grouping:
            bsk = gpu.CudaLweMultiBitBootstrapKey.from_lwe_multi_bit_bootstrap_key(
                keys.bsk, p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.grouping, st)
        else:
            bsk = gpu.CudaLweBootstrapKey.from_lwe_bootstrap_key(keys.bsk, p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, st,
                                                                 ms_noise_reduction=True)
        sks = igpu.CudaServerKey(ksk, bsk, m, m)
        for B in (1, args.batch):
            vals = [int.from_bytes(rng.bytes(8), "little") & mask for _ in range(B)]
            words = rm.encrypt_rows(p, keys, [rm.digits(v, L, m) for v in vals], 5)
            ops = [(f"scalar_mul {n}", s) for n, s in scalars] + [("mul", None)]
            for op, scalar in ops:
                seconds, pbs = [], 0
                for _ in range(1 + args.repeats):            # the first run warms the allocator and the code objects
                    ca = igpu.CudaUnsignedRadixCiphertext.from_blocks(words, st)
                    ca.set_degrees(m - 1)
                    cb = igpu.CudaUnsignedRadixCiphertext.from_blocks(words[::-1].copy(), st)
                    st.synchronize()
                    t0 = time.perf_counter()
                    if scalar is None:
                        pbs = sks.mul_assign(ca, cb, st, return_pbs_count=True)
                    else:
                        pbs = sks.scalar_mul_assign(ca, scalar, st, return_pbs_count=True)
                    st.synchronize()
                    seconds.append(time.perf_counter() - t0)
                got = [rm.value(r, m) for r in rm.decrypt_many(p, keys, ca.to_blocks(st)).tolist()]
                want = [(v * (scalar if scalar is not None else w)) & mask for v, w in zip(vals, vals[::-1])]
                assert got == want, f"{op}: wrong results"
                seconds = seconds[1:]
                best = min(seconds)
                print(json.dumps({"op": f"FheUint{2 * L} {op}", "params": p.name, "batch": B,
                                  "seconds": [round(s, 5) for s in seconds], "ops_per_s": round(B / best, 2),
                                  "pbs_per_op": pbs, "ks_pbs_per_s": round(B * pbs / best),
                                  "includes": "scratch allocation, index uploads, all rounds"}), flush=True)


if __name__ == "__main__":
    main()
