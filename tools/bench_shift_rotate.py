#!/usr/bin/env python3
"""FheUint64 shifts and rotations on ONE GPU, through the radix layer of the backend (tfhe_rs_amd/integer_gpu.py): the four
operations by an encrypted amount plus the arithmetic right shift, one integer (latency) and a batch (ops/s), the
arithmetic shift and the rotation by a clear amount, bootstraps per operation, with mul_assign and add_assign of the same
build beside them for scale; and the fused rotate-and-pack kernel against the same rows composed from a device copy,
block copies, single-row copies and two axpy launches (the last stage of a signed 64-bit right shift: 64 rows of 2,049
words, distance 32, the sign row pulled in).  One JSON line per measurement; results are checked against clear arithmetic
outside the timed region.

The kernel timings repeat the launch on the same buffers: 64 rows are 1 MiB per integer, so the repetitions are
cache-resident.  The reference measures these operations in tfhe-benchmark/benches/integer/bench.rs; its published
numbers are for other hardware and are not compared here."""
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


def kernel_comparison(gpu, lib, st, repeats, launches, batches):
    words, rows, r = 2049, 64, 32
    rng = np.random.default_rng(7)
    for batch in batches:
        x = rng.integers(0, 1 << 63, size=(batch, rows, words), dtype=U64)
        ctrl = rng.integers(0, 1 << 63, size=(batch, 6, words), dtype=U64)
        idx = np.repeat(np.arange(batch, dtype=U64) * U64(6) + U64(5), rows)
        d_x, d_ctrl, d_idx = (gpu.CudaVec.from_cpu_async(a.reshape(-1), st) for a in (x, ctrl, idx))
        outs = [gpu.CudaVec(x.size, st), gpu.CudaVec(x.size, st)]
        tmp = gpu.CudaVec(2 * x.size, st)
        want = x.copy()
        want[:, :rows - r] += U64(2) * x[:, r:]
        want[:, rows - r:] += U64(2) * x[:, rows - 1:rows]        # the sign row: row 63 of the integer's own rows
        want += ctrl[:, 5:6]
        s, g = st.ptr[0], st.gpu_indexes[0]
        forms = {
            "lwe_rotate_pack_kernel": lambda: lib.hip_test_rotate_pack_async(
                s, g, outs[0].ptr, d_x.ptr, d_x.ptr, d_ctrl.ptr, 1, 2, words, rows, batch, r, 1, 2, rows, rows - 1, 6, 5),
            "composed_from_primitives": lambda: lib.hip_test_rotate_pack_baseline_async(
                s, g, outs[1].ptr, d_x.ptr, d_x.ptr, d_ctrl.ptr, d_idx.ptr, tmp.ptr, 2, words, rows, batch, r, 1, 2, rows,
                rows - 1),
        }
        e0, e1 = lib.hip_event_create(), lib.hip_event_create()
        result = {"what": "barrel stage inputs, last stage of a signed 64-bit right shift", "rows": rows, "words": words,
                  "batch": batch, "launches_per_timing": launches, "data": "cache-resident repetitions"}
        for n, (name, launch) in enumerate(forms.items()):
            launch()
            assert np.array_equal(outs[n].copy_to_cpu(st).reshape(x.shape), want), name
            for _ in range(10):
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


def clear(op, v, a, B):
    mask = (1 << B) - 1
    if op == "shl":
        return (v << a) & mask if a < B else 0
    if op == "shr":
        return v >> a if a < B else 0
    if op in ("sar", "scalar sar"):
        return ((v - (1 << B) if v >> (B - 1) else v) >> min(a, B)) & mask
    r = a % B if op in ("rotl", "scalar rotl") else (B - a % B) % B
    return ((v << r) | (v >> (B - r))) & mask if r else v


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
        kernel_comparison(gpu, lib, st, args.repeats, args.launches, (1, args.batch))
    if args.skip_operations:
        return
    L, m = args.blocks, 4
    B = 2 * L
    mask = (1 << B) - 1
    rng = np.random.default_rng(1)
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
        for batch in (1, args.batch):
            vals = [int.from_bytes(rng.bytes(8), "little") & mask | 1 << (B - 1) for _ in range(batch)]
            amounts = [int(a) for a in rng.integers(0, B + 2, size=batch)]
            words = rm.encrypt_rows(p, keys, [rm.digits(v, L, m) for v in vals], 5)
            am_words = rm.encrypt_rows(p, keys, [rm.digits(a, L, m) for a in amounts], 6)
            ops = ["shl", "shr", "sar", "rotl", "rotr", "scalar sar", "scalar rotl", "mul", "add"]
            for op in ops:
                seconds, pbs = [], None
                for _ in range(1 + args.repeats):            # the first run warms the allocator and the code objects
                    ca = igpu.CudaUnsignedRadixCiphertext.from_blocks(words, st)
                    ca.set_degrees(m - 1)
                    cb = igpu.CudaUnsignedRadixCiphertext.from_blocks(am_words, st)
                    cb.set_degrees(m - 1)
                    st.synchronize()
                    t0 = time.perf_counter()
                    if op in ("shl", "shr", "sar"):
                        pbs = sks.shift_assign(ca, cb, st, left=op == "shl", arithmetic=op == "sar", return_pbs_count=True)
                    elif op in ("rotl", "rotr"):
                        pbs = sks.rotate_assign(ca, cb, st, left=op == "rotl", return_pbs_count=True)
                    elif op == "scalar sar":
                        sks.scalar_shift_assign(ca, 13, st, left=False, arithmetic=True)
                    elif op == "scalar rotl":
                        sks.scalar_rotate_assign(ca, 13, st, left=True)
                    elif op == "mul":
                        pbs = sks.mul_assign(ca, cb, st, return_pbs_count=True)
                    else:
                        sks.add_assign(ca, cb, st)
                    st.synchronize()
                    seconds.append(time.perf_counter() - t0)
                got = [rm.value(r, m) for r in rm.decrypt_many(p, keys, ca.to_blocks(st)).tolist()]
                if op == "mul":
                    want = [(v * a) & mask for v, a in zip(vals, amounts)]
                elif op == "add":
                    want = [(v + a) & mask for v, a in zip(vals, amounts)]
                else:
                    want = [clear(op, v, 13 if op.startswith("scalar") else a, B) for v, a in zip(vals, amounts)]
                assert got == want, f"{op}: wrong results"
                if op.startswith("scalar"):
                    pbs = L - 13 // 2 + 1 if op == "scalar sar" else L       # one round: the surviving blocks (+ the padding block)
                elif op == "add":
                    pbs = int(lib.hip_integer_propagate_pbs_count(L))
                seconds = seconds[1:]
                best = min(seconds)
                print(json.dumps({"op": f"FheUint{B} {op}", "params": p.name, "batch": batch,
                                  "seconds": [round(s, 5) for s in seconds], "ops_per_s": round(batch / best, 2),
                                  "pbs_per_op": pbs, "ks_pbs_per_s": round(batch * pbs / best),
                                  "includes": "scratch allocation, index uploads, all rounds"}), flush=True)


if __name__ == "__main__":
    main()
