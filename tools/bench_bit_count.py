#!/usr/bin/env python3
"""Encrypted bit counts on ONE GPU, through the radix layer of the backend (tfhe_rs_amd/integer_gpu.py).

1. The data movement of one scan step: one launch of lwe_pair_pack_kernel against the same rows composed per integer from
   a device copy and a memset, then one pairwise addition (hip_test_pair_pack_baseline_async), at L = 32 rows of 2,049
   words, the distances 1 and 16 towards the higher rows, batch 1 and 32.  Both forms are checked against each other word
   for word outside the timed region.  The timings repeat the launches on the same buffers; the line says how large the
   working set is and whether it fits the 256 MiB of last-level cache (cache-resident repetitions) or not.
2. Whole calls for FheUint64 (scratch allocation, index uploads, all rounds) of leading_zeros, trailing_ones, ilog2,
   count_ones and count_zeros, batch 1 and 32, on PARAM_MESSAGE_2_CARRY_2 and on
   PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2, with mul_assign and add_assign of the same shapes for scale.  Every result
   is decrypted against Python integers outside the timed region.

The reference's figures are counts read from its code (cuda/src/integer/ilog2.cuh), never timings.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import radix_model as rm  # noqa: E402  (encryption and the checker only)
from tests.common import C1, C4G4, make_keys  # noqa: E402

U64 = np.uint64
LLC_BYTES = 256 << 20


def kernel_comparison(gpu, lib, st, repeats, launches, batches, L=32, words=2049, msg=4):
    rng = np.random.default_rng(12)
    s, g = st.ptr[0], st.gpu_indexes[0]
    for batch in batches:
        x = gpu.CudaVec.from_cpu_async(rng.integers(0, 1 << 63, size=batch * L * words, dtype=U64), st)
        a, b, tmp = (gpu.CudaVec(batch * L * words, st) for _ in range(3))
        for delta in (1, 16):
            fused = lambda: lib.hip_test_pair_pack_async(s, g, a.ptr, x.ptr, 1, msg, words, batch, L, 0, L, 1, delta)
            composed = lambda: lib.hip_test_pair_pack_baseline_async(s, g, b.ptr, x.ptr, tmp.ptr, msg, words, batch, L, delta)
            fused()
            composed()
            assert np.array_equal(a.copy_to_cpu(st), b.copy_to_cpu(st)), "the two forms differ"
            working_set = 8 * words * 2 * batch * L
            result = {"what": "data movement of one scan step", "rows": L, "distance": delta, "batch": batch, "words": words,
                      "launches_per_timing": launches, "fused_working_set_bytes": working_set,
                      "data": "cache-resident repetitions" if working_set < LLC_BYTES else "repetitions larger than the last-level cache",
                      "fused_launches": 1, "composed_operations": 2 * batch + 1}
            e0, e1 = lib.hip_event_create(), lib.hip_event_create()
            for name, launch in (("pair_pack_launch", fused), ("composed_from_primitives", composed)):
                for _ in range(5):
                    launch()
                us = []
                for _ in range(repeats):
                    st.synchronize()
                    lib.hip_event_record(e0, s)
                    for _ in range(launches):
                        launch()
                    lib.hip_event_record(e1, s)
                    us.append(1e3 * lib.hip_event_elapsed_ms(e0, e1) / launches)
                result[name + "_us"] = [round(u, 3) for u in us]
            lib.hip_event_destroy(e0)
            lib.hip_event_destroy(e1)
            print(json.dumps(result), flush=True)


def expected(op, v, B):
    bits = [(v >> i) & 1 for i in range(B)]

    def run(seq, bit):
        n = 0
        for x in seq:
            if x != bit:
                break
            n += 1
        return n
    return {"leading_zeros": lambda: run(bits[::-1], 0), "trailing_ones": lambda: run(bits, 1), "ilog2": lambda: v.bit_length() - 1,
            "count_ones": lambda: sum(bits), "count_zeros": lambda: B - sum(bits)}[op]()


KIND = {"leading_zeros": 0, "trailing_ones": 0, "ilog2": 1, "count_ones": 2, "count_zeros": 2}


def whole_calls(gpu, igpu, lib, st, names, batches, repeats, L=32):
    rng = np.random.default_rng(2)
    m, B = 4, 2 * L
    for name in names:
        p = {"classic": C1, "multibit_g4": C4G4}[name]
        keys = make_keys(p)
        ksk = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(keys.ksk, p.big_n, p.n, p.ks_base_log, p.ks_level, st)
        if p.grouping:
            bsk = gpu.CudaLweMultiBitBootstrapKey.from_lwe_multi_bit_bootstrap_key(
                keys.bsk, p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.grouping, st)
        else:
            bsk = gpu.CudaLweBootstrapKey.from_lwe_bootstrap_key(keys.bsk, p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, st,
                                                                 ms_noise_reduction=True)
        sks = igpu.CudaServerKey(ksk, bsk, 4, 4)
        for batch in batches:
            xs = [int.from_bytes(rng.bytes(8), "little") >> int(rng.integers(0, 60)) for _ in range(batch)]
            ys = [int.from_bytes(rng.bytes(8), "little") for _ in range(batch)]
            if batch >= 4:
                xs[1], xs[2] = 0, (1 << 64) - 1
            wx = rm.encrypt_rows(p, keys, [rm.digits(x, L, m) for x in xs], 5)
            wy = rm.encrypt_rows(p, keys, [rm.digits(y, L, m) for y in ys], 6)

            def fresh():
                cts = [igpu.CudaUnsignedRadixCiphertext.from_blocks(w, st) for w in (wx, wy)]
                for ct in cts:
                    ct.set_degrees(m - 1)
                return cts

            value = lambda ct: [rm.value(r, m) for r in rm.decrypt_many(p, keys, ct.to_blocks(st)).tolist()]
            for op in list(KIND) + ["mul_assign", "add_assign"]:
                seconds = []
                for _ in range(1 + repeats):              # the first run warms the allocator and the code objects
                    a, b = fresh()
                    st.synchronize()
                    t0 = time.perf_counter()
                    if op in KIND:
                        out, pbs = getattr(sks, "unchecked_" + op)(a, st, return_pbs_count=True)
                    elif op == "mul_assign":
                        pbs = sks.mul_assign(a, b, st, return_pbs_count=True) * batch
                    else:
                        sks.add_assign(a, b, st)
                        pbs = None
                    st.synchronize()
                    seconds.append(time.perf_counter() - t0)
                line = {"op": op, "params": p.name, "blocks": L, "batch": batch, "seconds": [round(x, 5) for x in seconds[1:]],
                        "includes": "scratch allocation, index uploads, all rounds"}
                if op in KIND:
                    nc = out.num_blocks
                    assert value(out) == [expected(op, x, B) % m ** nc for x in xs], f"{op}: wrong result"
                    line.update(pbs=pbs, rounds=int(lib.hip_integer_bit_count_rounds(KIND[op], L, m, 4)),
                                ks_pbs_per_s=round(pbs / min(seconds[1:])), calls_per_s=round(batch / min(seconds[1:]), 3))
                elif op == "mul_assign":
                    assert value(a) == [(x * y) & ((1 << B) - 1) for x, y in zip(xs, ys)], "mul_assign: wrong result"
                    line.update(pbs=pbs)
                else:
                    assert value(a) == [(x + y) & ((1 << B) - 1) for x, y in zip(xs, ys)], "add_assign: wrong result"
                print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--params", default="classic,multibit_g4",
                    help="classic = PARAM_MESSAGE_2_CARRY_2, multibit_g4 = PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    args = ap.parse_args()
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import ffi
    from tfhe_rs_amd import integer_gpu as igpu
    lib = ffi.default_library()
    st = gpu.CudaStreams([0])
    batches = [int(x) for x in args.batches.split(",")]
    if not args.skip_kernels:
        kernel_comparison(gpu, lib, st, args.repeats, args.launches, batches)
    if not args.skip_calls:
        whole_calls(gpu, igpu, lib, st, args.params.split(","), batches, args.repeats)


if __name__ == "__main__":
    main()
