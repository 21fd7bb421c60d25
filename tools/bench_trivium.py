#!/usr/bin/env python3
"""Trivium transciphering on ONE GPU, through the radix layer of the backend (tfhe_rs_amd/integer_gpu.py).

1. The data movement of one batch of 64 steps with keystream: the two launches of lwe_tap_sum_kernel against the same rows
   composed from device copies and pairwise additions in the reference's order (hip_test_trivium_batch_baseline_async),
   at N = 1, 8 and 64 inputs, rows of 2,049 words.  Both forms are checked against each other outside the timed region.
   The timings repeat the launches on the same buffers; the line says how large the working set is and whether it fits
   the 256 MiB of last-level cache (cache-resident repetitions) or not.
2. Whole trivium_init and trivium_next(64 k) calls (scratch allocation, index uploads, all rounds) at N = 1, 8 and 64 on
   PARAM_MESSAGE_2_CARRY_2 and on PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2, with rounds and bootstraps per call.  The
   keystream of input 0 is checked against a clear model outside the timed region.

The reference's figures are its counts as its code states them (cuda/src/trivium/trivium.cuh): three rounds per batch,
54 rounds and 8,067 N bootstraps per init, 512 N bootstraps per batch with keystream.  No timing of the reference is used.
One JSON line per measurement."""
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
BITS = (93, 84, 111)
A, B, CC = 0, 1, 2
LLC_BYTES = 256 << 20


def clear_steps(a, b, c, steps):
    z = []
    for _ in range(steps):
        t1, t2, t3 = a[65] ^ a[92], b[68] ^ b[83], c[65] ^ c[110]
        z.append(t1 ^ t2 ^ t3)
        ai, bi, ci = t3 ^ a[68] ^ (c[108] & c[109]), t1 ^ b[77] ^ (a[90] & a[91]), t2 ^ c[86] ^ (b[81] & b[82])
        a, b, c = [ai] + a[:-1], [bi] + b[:-1], [ci] + c[:-1]
    return z, a, b, c


def clear_init(key, iv):
    a, b, c = [0] * 93, [0] * 84, [0] * 111
    for i in range(80):
        a[i], b[i] = key[79 - i], iv[79 - i]
    c[108] = c[109] = c[110] = 1
    return clear_steps(a, b, c, 1152)[1:]


class Table:
    """the host arrays of one hip_test_tap_sum_async call: groups of 64 bits, terms (source pointer, position, scalar)"""

    def __init__(self, outs, groups):
        G = len(groups)
        self.G = G
        self.outs = (C.c_void_p * G)(*outs)
        self.bits = (C.c_uint32 * G)(*([64] * G))
        self.terms = (C.c_uint32 * G)(*[len(g) for g in groups])
        self.srcs, self.pos = (C.c_void_p * (5 * G))(), (C.c_uint32 * (5 * G))()
        self.back, self.scal = (C.c_uint32 * (5 * G))(), (C.c_uint64 * (5 * G))()
        for g, ts in enumerate(groups):
            for t, (src, p, scalar) in enumerate(ts):
                self.srcs[5 * g + t], self.pos[5 * g + t], self.scal[5 * g + t] = src, p, scalar

    def launch(self, lib, s, gpu_index, words, inputs):
        lib.hip_test_tap_sum_async(s, gpu_index, words, inputs, self.G, self.outs, self.bits, self.terms, self.srcs, self.pos,
                                   self.back, self.scal)


def kernel_comparison(gpu, lib, st, repeats, launches, inputs_list, words=2049, msg=4):
    rng = np.random.default_rng(7)
    s, g = st.ptr[0], st.gpu_indexes[0]
    for N in inputs_list:
        group = 64 * N * words                      # words of one group of a round
        draw = lambda rows: rng.integers(0, 1 << 63, size=rows * words, dtype=U64)
        regs = [draw(bits * N) for bits in BITS]
        r1, r2 = draw(4 * 64 * N), draw(4 * 64 * N)
        d_regs = [gpu.CudaVec.from_cpu_async(r, st) for r in regs]          # the tap launches read these
        d_regs_b = [gpu.CudaVec.from_cpu_async(r, st) for r in regs]        # the composition shifts these in place
        d_r1, d_r2 = gpu.CudaVec.from_cpu_async(r1, st), gpu.CudaVec.from_cpu_async(r2, st)
        ins = [[gpu.CudaVec(4 * group, st) for _ in range(2)] for _ in range(2)]      # [form][round]
        d_ks, d_tmp = gpu.CudaVec(group, st), gpu.CudaVec((111 + 12 * 64) * N * words, st)
        tap = lambda r, position, scalar=1: (d_regs[r].ptr, position - 63, scalar)
        out1 = lambda k: d_r1.ptr + 8 * k * group
        t1 = Table([ins[0][0].ptr + 8 * k * group for k in range(4)],
                   [[tap(CC, 109, msg), tap(CC, 108)], [tap(A, 91, msg), tap(A, 90)], [tap(B, 82, msg), tap(B, 81)],
                    [tap(CC, 65), tap(CC, 110)]])
        t2 = Table([ins[0][1].ptr + 8 * k * group for k in range(4)],
                   [[(out1(3), 0, 1), tap(A, 68), (out1(0), 0, 1)],
                    [tap(A, 65), tap(A, 92), tap(B, 77), (out1(1), 0, 1)],
                    [tap(B, 68), tap(B, 83), tap(CC, 86), (out1(2), 0, 1)],
                    [tap(A, 65), tap(A, 92), tap(B, 68), tap(B, 83), (out1(3), 0, 1)]])

        def fused():
            t1.launch(lib, s, g, words, N)
            t2.launch(lib, s, g, words, N)

        def composed():
            lib.hip_test_trivium_batch_baseline_async(s, g, d_regs_b[0].ptr, d_regs_b[1].ptr, d_regs_b[2].ptr, ins[1][0].ptr,
                                                      d_r1.ptr, ins[1][1].ptr, d_r2.ptr, d_ks.ptr, d_tmp.ptr, words, N, msg)

        fused()
        composed()
        for k in range(2):
            assert np.array_equal(ins[0][k].copy_to_cpu(st), ins[1][k].copy_to_cpu(st)), f"round {k + 1} inputs differ"
        rows = lambda v: v.reshape(-1, N * words)
        assert np.array_equal(rows(d_ks.copy_to_cpu(st)), rows(r2)[3 * 64:][::-1]), "keystream is not in step order"
        for r, bits in enumerate(BITS):
            want = np.concatenate([rows(r2)[64 * r:64 * (r + 1)], rows(regs[r])[:bits - 64]])
            assert np.array_equal(rows(d_regs_b[r].copy_to_cpu(st)), want), f"register {r} after shift-and-insert"
        working_set = 8 * (sum(r.size for r in regs) + r1.size + 2 * 4 * group)
        result = {"what": "data movement of one batch of 64 steps with keystream", "inputs": N, "words": words,
                  "launches_per_timing": launches, "fused_working_set_bytes": working_set,
                  "data": "cache-resident repetitions" if working_set < LLC_BYTES else "repetitions larger than the last-level cache",
                  "fused_launches": 2, "composed_operations": 97}
        e0, e1 = lib.hip_event_create(), lib.hip_event_create()
        for name, launch in (("two_tap_launches", fused), ("composed_from_primitives", composed)):
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


def whole_calls(gpu, igpu, st, names, inputs_list, steps, repeats):
    rng = np.random.default_rng(1)
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
        for N in inputs_list:
            key, iv = rng.integers(0, 2, size=(N, 80)), rng.integers(0, 2, size=(N, 80))
            kw = rm.encrypt_rows(p, keys, [key.T.reshape(-1).tolist()], 5)
            vw = rm.encrypt_rows(p, keys, [iv.T.reshape(-1).tolist()], 6)
            timings = {"init": [], "next": []}
            for _ in range(1 + repeats):              # the first run warms the allocator and the code objects
                ck, cv = (igpu.CudaUnsignedRadixCiphertext.from_blocks(w, st) for w in (kw, vw))
                st.synchronize()
                t0 = time.perf_counter()
                state, init_pbs = sks.trivium_init(ck, cv, st, return_pbs_count=True)
                st.synchronize()
                t1 = time.perf_counter()
                ks, next_pbs = sks.trivium_next(state, steps, st, return_pbs_count=True)
                st.synchronize()
                timings["init"].append(t1 - t0)
                timings["next"].append(time.perf_counter() - t1)
            got = rm.decrypt_many(p, keys, ks.to_blocks(st))[0].reshape(steps, N)[:, 0].tolist()
            assert got == clear_steps(*clear_init(key[0].tolist(), iv[0].tolist()), steps)[0], "wrong keystream"
            batches = steps // 64
            for op, pbs, rounds, ref_pbs, ref_rounds in (("trivium_init", init_pbs, 36, 8067 * N, 54),
                                                         (f"trivium_next({steps})", next_pbs, 2 * batches, 512 * N * batches,
                                                          3 * batches)):
                seconds = timings["init" if op == "trivium_init" else "next"][1:]
                best = min(seconds)
                print(json.dumps({"op": op, "params": p.name, "inputs": N, "seconds": [round(x, 5) for x in seconds],
                                  "rounds": rounds, "pbs": pbs, "ks_pbs_per_s": round(pbs / best),
                                  "reference_rounds_from_its_code": ref_rounds, "reference_pbs_from_its_code": ref_pbs,
                                  "includes": "scratch allocation, index uploads, all rounds"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="1,8,64")
    ap.add_argument("--steps", type=int, default=256, help="steps of the timed trivium_next call (64 k)")
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
    inputs = [int(x) for x in args.inputs.split(",")]
    if not args.skip_kernels:
        kernel_comparison(gpu, lib, st, args.repeats, args.launches, inputs)
    if not args.skip_calls:
        whole_calls(gpu, igpu, st, args.params.split(","), inputs, args.steps, args.repeats)


if __name__ == "__main__":
    main()
