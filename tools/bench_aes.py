#!/usr/bin/env python3
"""AES-128 transciphering on ONE GPU, through the radix layer of the backend (tfhe_rs_amd/integer_gpu.py).

1. The data movement of one middle cipher round: the launches of lwe_gate_sum_kernel of one round at S-box parallelism 16
   (hip_test_aes_round_launches_async: 13 for the S-box, 2 for the linear layer at moduli (4, 4)) against the same round
   composed from device copies and pairwise additions in the reference's order (hip_test_aes_round_baseline_async), at
   N = 1, 8 and 64 inputs, rows of 2,049 words.  Neither side runs the bootstraps.  The two sides alternate, repetition by
   repetition; they run on the same buffers every time, and the line says how large the working set is and whether it fits
   the 256 MiB of last-level cache.
2. Whole key_expansion and aes_encrypt calls (scratch allocation, scheduling, uploads, all rounds) at N = 1 and 64 and
   S-box parallelism 16, on PARAM_MESSAGE_2_CARRY_2 and on PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2, with published
   rounds and bootstraps, time per round, and add_assign / mul_assign of one 64-bit integer in the same session for scale.
   Input 0 is checked against a clear AES outside the timed region.

The reference's figures are its counts as its code states them (cuda/src/aes/aes.cuh; docs/history/aes_log.md): 652 rounds and
18,816 N bootstraps per aes_ctr_encrypt, 390 rounds and 5,240 bootstraps per key_expansion.  No timing of the reference is
used: it is not run.  One JSON line per measurement."""
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
from tests.test_aes import bits_of_bytes, ctr_block, expand_key, to_bytes  # noqa: E402  (the clear model)

U64 = np.uint64
LLC_BYTES = 256 << 20
KEY, IV = 0x2B7E151628AED2A6ABF7158809CF4F3C, 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF


def kernel_comparison(gpu, ffi, igpu, lib, st, repeats, launches, inputs_list, big_n=2048):
    words = big_n + 1
    s, keep = igpu.CudaServerKey._streams(st)
    g = st.gpu_indexes[0]
    bk = ffi.CudaLweBootstrapKeyParamsFFI(8, 1, big_n, 23, 1, big_n, 1, 0)
    kk = ffi.CudaLweKeyswitchKeyParamsFFI(big_n, 8, 4, 4)
    rng = np.random.default_rng(7)
    for N in inputs_list:
        mem = C.c_void_p()
        lib.hip_scratch_integer_aes_ctr_encrypt_64_async(s, C.byref(mem), bk, kk, 4, 4, True, 0, N, 16)
        key = gpu.CudaVec.from_cpu_async(rng.integers(0, 1 << 63, size=128 * words, dtype=U64), st)
        state = gpu.CudaVec.from_cpu_async(rng.integers(0, 1 << 63, size=128 * N * words, dtype=U64), st)
        tmp = gpu.CudaVec(512 * N * words, st)
        rounds = int(lib.hip_integer_aes_rounds(mem))
        fused = lambda: lib.hip_test_aes_round_launches_async(s, key.ptr, mem)
        composed = lambda: lib.hip_test_aes_round_baseline_async(st.ptr[0], g, state.ptr, key.ptr, tmp.ptr, words, N)
        working_set = 8 * words * N * (75 + 16 + 17) * 16      # wires written and read by the gate-sum launches, roughly
        result = {"what": "data movement of one middle cipher round, no bootstraps", "inputs": N, "words": words,
                  "launches_per_timing": launches, "gate_sum_launches": 15, "fused_working_set_bytes": working_set,
                  "data": "cache-resident repetitions" if working_set < LLC_BYTES else "repetitions larger than the last-level cache",
                  "rounds_of_a_call": rounds, "interleaved": True}
        e0, e1 = lib.hip_event_create(), lib.hip_event_create()
        sides = (("gate_sum_launches", fused), ("composed_from_primitives", composed))
        for _, launch in sides:
            for _ in range(3):
                launch()
        us = {name: [] for name, _ in sides}
        for _ in range(repeats):
            for name, launch in sides:                         # the two sides alternate
                st.synchronize()
                lib.hip_event_record(e0, st.ptr[0])
                for _ in range(launches):
                    launch()
                lib.hip_event_record(e1, st.ptr[0])
                us[name].append(1e3 * lib.hip_event_elapsed_ms(e0, e1) / launches)
        for name, _ in sides:
            result[name + "_us"] = [round(u, 2) for u in us[name]]
        lib.hip_event_destroy(e0)
        lib.hip_event_destroy(e1)
        lib.hip_cleanup_integer_aes_ctr_encrypt_64(s, C.byref(mem))
        print(json.dumps(result), flush=True)


def whole_calls(gpu, igpu, st, names, inputs_list, repeats):
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
        enc = lambda v, seed: igpu.CudaUnsignedRadixCiphertext.from_blocks(
            rm.encrypt_rows(p, keys, [igpu.encrypt_u128_for_aes_ctr(v)], seed), st)
        key, iv = enc(KEY, 5), enc(IV, 6)
        seconds = []
        for _ in range(1 + repeats):                  # the first run warms the allocator and the code objects
            st.synchronize()
            t0 = time.perf_counter()
            rks, pbs, rounds = sks.key_expansion(key, st, return_pbs_count=True, return_rounds=True)
            st.synchronize()
            seconds.append(time.perf_counter() - t0)
        got = rm.decrypt_many(p, keys, rks.to_blocks(st))[0].tolist()
        assert got == sum((bits_of_bytes(rk) for rk in expand_key(to_bytes(KEY))), []), "wrong round keys"
        report("key_expansion", p, 1, seconds[1:], pbs, rounds, 5240, 390)
        for N in inputs_list:
            seconds = []
            for _ in range(1 + repeats):
                st.synchronize()
                t0 = time.perf_counter()
                out, pbs, rounds = sks.aes_encrypt(iv, rks, 0, N, 16, st, return_pbs_count=True, return_rounds=True)
                st.synchronize()
                seconds.append(time.perf_counter() - t0)
            got = igpu.decrypt_u128_from_aes_ctr(rm.decrypt_many(p, keys, out.to_blocks(st))[0].tolist()[:128], 1)
            assert got == [ctr_block(KEY, IV, 0)], "wrong block"
            report("aes_encrypt", p, N, seconds[1:], pbs, rounds, 18816 * N, 652)
        # for scale, in the same session: one 64-bit integer
        for op in ("add_assign", "mul_assign"):
            seconds = []
            for _ in range(1 + repeats):
                a, b = (igpu.CudaUnsignedRadixCiphertext.from_blocks(
                    rm.encrypt_rows(p, keys, [[(v >> (2 * i)) & 3 for i in range(32)]], 9 + k), st) for k, v in enumerate((12345678901234567, 98765432109876543)))
                st.synchronize()
                t0 = time.perf_counter()
                getattr(sks, op)(a, b, st)
                st.synchronize()
                seconds.append(time.perf_counter() - t0)
            print(json.dumps({"op": op, "params": p.name, "blocks": 32, "seconds": [round(x, 5) for x in seconds[1:]]}), flush=True)


def report(op, p, N, seconds, pbs, rounds, ref_pbs, ref_rounds):
    best = min(seconds)
    print(json.dumps({"op": op, "params": p.name, "inputs": N, "sbox_parallelism": 16, "seconds": [round(x, 5) for x in seconds],
                      "rounds": rounds, "pbs": pbs, "ms_per_round": round(1e3 * best / rounds, 3), "ks_pbs_per_s": round(pbs / best),
                      "reference_rounds_from_its_code": ref_rounds, "reference_pbs_from_its_code": ref_pbs,
                      "includes": "scratch allocation, scheduling, uploads, all rounds"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="1,8,64", help="inputs of the kernel comparison")
    ap.add_argument("--call-inputs", default="1,64", help="inputs of the whole aes_encrypt calls")
    ap.add_argument("--params", default="classic,multibit_g4",
                    help="classic = PARAM_MESSAGE_2_CARRY_2, multibit_g4 = PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    args = ap.parse_args()
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import ffi
    from tfhe_rs_amd import integer_gpu as igpu
    lib = ffi.default_library()
    st = gpu.CudaStreams([0])
    if not args.skip_kernels:
        kernel_comparison(gpu, ffi, igpu, lib, st, args.repeats, args.launches, [int(x) for x in args.inputs.split(",")])
    if not args.skip_calls:
        whole_calls(gpu, igpu, st, args.params.split(","), [int(x) for x in args.call_inputs.split(",")], args.repeats)


if __name__ == "__main__":
    main()
