#!/usr/bin/env python3
"""Encrypted integer division on ONE GPU, through the radix layer of the backend (tfhe_rs_amd/integer_gpu.py).

1. The data movement of one iteration of the division loop: the three launches of lwe_divrem_sum_kernel against the same
   rows composed from device copies, memsets and pairwise additions in the reference's order
   (hip_test_divrem_iteration_baseline_async), at L = 32 blocks, iteration s = 32 of 64 (17 interesting blocks, a trimmed
   top block, an upper-bits flag), batch 1 and 8, rows of 2,049 words.  Both forms are checked against each other word for
   word outside the timed region.  The timings repeat the launches on the same buffers; the line says how large the working
   set is and whether it fits the 256 MiB of last-level cache (cache-resident repetitions) or not.
2. Whole div_rem calls for FheUint64 (scratch allocation, index uploads, all rounds), unsigned and signed, batch 1 and 8,
   on PARAM_MESSAGE_2_CARRY_2 and on PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2, with mul_assign and add_assign of the
   same shapes for scale.  Every result is decrypted against Python integers outside the timed region.

The reference's figures are counts read from its code (cuda/src/integer/div_rem.cuh), never timings.
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
LLC_BYTES = 256 << 20
NEG = 2 ** 64 - 1


class Table:
    """the host arrays of one hip_test_divrem_sum_async call.  group: (out, stride, first_out, first, rows, constant,
    terms); term: (src, scalar, stride, extent, offset, step, stand, stand_stride, stand_row)"""

    def __init__(self, groups):
        G = self.G = len(groups)
        self.outs, self.consts, self.gu = (C.c_void_p * G)(), (C.c_uint64 * G)(), (C.c_uint32 * (6 * G))()
        self.srcs, self.stands = (C.c_void_p * (4 * G))(), (C.c_void_p * (4 * G))()
        self.scal, self.tu = (C.c_uint64 * (4 * G))(), (C.c_uint32 * (24 * G))()
        for g, (out, stride, first_out, first, rows, constant, terms) in enumerate(groups):
            self.outs[g], self.consts[g] = out, constant
            self.gu[6 * g:6 * g + 6] = [stride, stride, first_out, first, rows, len(terms)]
            for t, (src, scalar, s_stride, extent, offset, step, stand, stand_stride, stand_row) in enumerate(terms):
                k = 4 * g + t
                self.srcs[k], self.stands[k], self.scal[k] = src, stand, scalar
                self.tu[6 * k:6 * k + 6] = [s_stride, extent, offset & 0xFFFFFFFF, step, stand_stride, stand_row]

    def launch(self, lib, s, gpu_index, words, batch):
        lib.hip_test_divrem_sum_async(s, gpu_index, words, batch, self.G, self.outs, self.consts, self.gu, self.srcs,
                                      self.stands, self.scal, self.tu)


def kernel_comparison(gpu, lib, st, repeats, launches, batches, L=32, bits=2, s_iter=32, words=2049):
    rng = np.random.default_rng(11)
    s, g = st.ptr[0], st.gpu_indexes[0]
    msg, B = 1 << bits, bits * L
    n, blk, t_low = s_iter // bits + 1, (B - 1 - s_iter) // bits, (s_iter + 1) % bits
    whole, f, delta = (n - 1 if t_low else n), (2 if s_iter + 1 == B else 3), 1 << 59
    for batch in batches:
        draw = lambda rows: gpu.CudaVec.from_cpu_async(rng.integers(0, 1 << 63, size=rows * words, dtype=U64), st)
        r1, r2, num, s1, s2, negd, neglow, cl = (draw(batch * L) for _ in range(8))
        fl, up = draw(batch), draw(batch)
        row = np.zeros(words, dtype=U64)
        row[-1] = delta
        one = gpu.CudaVec.from_cpu_async(row, st)
        consts = gpu.CudaVec.from_cpu_async(np.tile(row * U64(msg - 1), L), st)
        zero_idx = gpu.CudaVec.from_cpu_async(np.zeros(L, dtype=U64), st)
        tmp = gpu.CudaVec((2 * L + 1) * words, st)
        form = lambda: dict(in1=gpu.CudaVec(2 * batch * n * words, st), in2=gpu.CudaVec(batch * n * words, st),
                            in3=gpu.CudaVec((2 * n + 1) * batch * words, st), v=draw(batch * L))
        a, b = form(), form()
        arr = lambda vec, scalar=1, offset=0, step=1, rows=L: (vec.ptr, scalar, rows, rows, offset, step, None, 0, 0)
        dense = lambda vec, at, rows, terms, constant=0, first=0: (vec.ptr + 8 * at * words, rows, 0, first, rows, constant, terms)
        below = (r1.ptr, 1, L, L, -1, 1, num.ptr, L, blk)
        flags = [arr(fl, NEG, 0, 0, 1), arr(up, 1, 0, 0, 1)]
        stage2 = [dense(a["in2"], 0, n, [arr(s1), arr(s2)])]
        if whole:
            stage2.append((a["v"].ptr, L, 0, 0, whole, 0, [arr(s1), arr(s2), arr(negd)]))
        if t_low:
            stage2.append((a["v"].ptr, L, n - 1, n - 1, 1, 0, [arr(s1), arr(s2), arr(neglow)]))
        if n < L:
            stage2.append((a["v"].ptr, L, n, n, L - n, (msg - 1) * delta, []))
        tables = [Table([dense(a["in1"], 0, n, [arr(r1, msg), below]),
                         dense(a["in1"], batch * n, n, [arr(r2, msg), arr(r2, 1, -1)])]),
                  Table(stage2),
                  Table([dense(a["in3"], 0, n, [arr(cl, f)] + flags, delta), dense(a["in3"], batch * n, n, [arr(a["v"], f)] + flags, delta),
                         dense(a["in3"], 2 * batch * n, 1, flags, delta)])]

        def fused():
            for t in tables:
                t.launch(lib, s, g, words, batch)

        def composed():
            for stage in (1, 2, 3):
                lib.hip_test_divrem_iteration_baseline_async(
                    s, g, r1.ptr, r2.ptr, num.ptr, s1.ptr, s2.ptr, negd.ptr, neglow.ptr if t_low else None, cl.ptr, b["v"].ptr,
                    fl.ptr, up.ptr, consts.ptr, one.ptr, zero_idx.ptr, b["in1"].ptr, b["in2"].ptr, b["in3"].ptr, tmp.ptr, words,
                    L, batch, s_iter, bits, msg, stage)

        fused()
        composed()
        for name in ("in1", "in2", "v", "in3"):
            assert np.array_equal(a[name].copy_to_cpu(st), b[name].copy_to_cpu(st)), f"{name}: the two forms differ"
        working_set = 8 * words * (10 * batch * L + 2 * batch + 5 * batch * n + batch)
        operations = batch * (6 + 3 + bool(whole) + bool(t_low) + bool(n < L) + 5)
        result = {"what": "data movement of one iteration of the division loop", "blocks": L, "iteration": s_iter,
                  "interesting_blocks": n, "batch": batch, "words": words, "launches_per_timing": launches,
                  "fused_working_set_bytes": working_set,
                  "data": "cache-resident repetitions" if working_set < LLC_BYTES else "repetitions larger than the last-level cache",
                  "fused_launches": 3, "composed_operations": operations}
        e0, e1 = lib.hip_event_create(), lib.hip_event_create()
        for name, launch in (("three_stage_launches", fused), ("composed_from_primitives", composed)):
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


def expected(n, d, B, signed):
    full = (1 << B) - 1
    if not signed:
        return (full, n) if d == 0 else (n // d, n % d)
    sn, sd = (n - (1 << B) if n >> (B - 1) else n), (d - (1 << B) if d >> (B - 1) else d)
    if sd == 0:
        return (1 if sn < 0 else full), n
    q = abs(sn) // abs(sd) * (1 if (sn < 0) == (sd < 0) else -1)
    return q & full, (sn - q * sd) & full


def rounds_per_division(L, bits, signed):
    """rounds of one call as docs/history/div_rem_log.md counts them"""
    def propagation(with_carry):
        if L == 1:
            return 1 + with_carry
        levels = [L]
        while levels[-1] > 4:
            levels.append((levels[-1] + 2) // 3)
        top = len(levels) - 1
        return 1 + top + 1 + max(top - 1, 0) + 1 + with_carry
    r = 1 + (L - 1).bit_length() + 1 + bits * L * (3 + propagation(1)) + 1
    return r + (2 * (2 + propagation(0)) if signed else 0)


def whole_calls(gpu, igpu, st, names, batches, repeats, L=32):
    rng = np.random.default_rng(1)
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
            nums = [int.from_bytes(rng.bytes(8), "little") for _ in range(batch)]
            dens = [int.from_bytes(rng.bytes(8), "little") >> int(rng.integers(0, 60)) for _ in range(batch)]
            if batch >= 4:
                dens[1], nums[2], dens[2] = 0, 1 << 63, (1 << 64) - 1          # a zero divisor, MIN / -1
            wn = rm.encrypt_rows(p, keys, [rm.digits(x, L, m) for x in nums], 5)
            wd = rm.encrypt_rows(p, keys, [rm.digits(x, L, m) for x in dens], 6)

            def fresh():
                cts = [igpu.CudaUnsignedRadixCiphertext.from_blocks(w, st) for w in (wn, wd)]
                for ct in cts:
                    ct.set_degrees(m - 1)
                return cts

            value = lambda ct: [rm.value(r, m) for r in rm.decrypt_many(p, keys, ct.to_blocks(st)).tolist()]
            for op in ("div_rem unsigned", "div_rem signed", "mul_assign", "add_assign"):
                seconds = []
                for _ in range(1 + repeats):              # the first run warms the allocator and the code objects
                    a, b = fresh()
                    st.synchronize()
                    t0 = time.perf_counter()
                    if op.startswith("div_rem"):
                        q, r, pbs = sks.div_rem(a, b, st, signed=op.endswith(" signed"), return_pbs_count=True)
                    elif op == "mul_assign":
                        pbs = sks.mul_assign(a, b, st, return_pbs_count=True) * batch
                    else:
                        sks.add_assign(a, b, st)
                        pbs = None
                    st.synchronize()
                    seconds.append(time.perf_counter() - t0)
                line = {"op": op, "params": p.name, "blocks": L, "batch": batch, "seconds": [round(x, 5) for x in seconds[1:]],
                        "includes": "scratch allocation, index uploads, all rounds"}
                if op.startswith("div_rem"):
                    signed = op.endswith(" signed")
                    got = list(zip(value(q), value(r)))
                    assert got == [expected(x, y, B, signed) for x, y in zip(nums, dens)], f"{op}: wrong result"
                    line.update(pbs=pbs, rounds=rounds_per_division(L, 2, signed), ks_pbs_per_s=round(pbs / min(seconds[1:])),
                                divisions_per_s=round(batch / min(seconds[1:]), 3))
                elif op == "mul_assign":
                    assert value(a) == [(x * y) & ((1 << B) - 1) for x, y in zip(nums, dens)], "mul_assign: wrong result"
                    line.update(pbs=pbs)
                else:
                    assert value(a) == [(x + y) & ((1 << B) - 1) for x, y in zip(nums, dens)], "add_assign: wrong result"
                print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--params", default="classic,multibit_g4",
                    help="classic = PARAM_MESSAGE_2_CARRY_2, multibit_g4 = PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2")
    ap.add_argument("--repeats", type=int, default=2)
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
        whole_calls(gpu, igpu, st, args.params.split(","), batches, args.repeats)


if __name__ == "__main__":
    main()
