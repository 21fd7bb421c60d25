"""Every template instantiation the PBS dispatchers can pick, bit for bit against the oracle.

A bootstrap call reaches one of many kernel instantiations, chosen by the shape (N, k), the decomposition
(level, base_log), the grouping factor, the batch size and hip_backend_set_fft_kernel.  CASES has one row per reachable
instantiation and mode; each row runs one launch on both backends and checks
  - the output against the oracle word for word (the accumulator of every LUT, gathered / scattered through
    non-trivial index vectors; on the many-LUT rows the first function's outputs, and the masks of the others);
  - that hip_backend_last_pbs_instantiation reports the instantiation the row is for;
  - that the outputs decrypt to f(m) (the bit equality is the gate; decryption says the row's inputs are meaningful).
Inputs: a toy n with the row's real (k, N, level, base_log, g) — n odd for the classic rows, g times an odd number for
the multi-bit rows — encryptions of every plaintext, and random ciphertexts on the decomposer-boundary accumulator of
test_backend_parity.test_decomposer_boundary_digits_in_every_fft_kernel.

test_every_dispatched_instantiation_has_a_row reads the dispatch functions and fails when one of them can launch an
instantiation no row selects.  Rows marked gpu_only repeat an instantiation and mode that an emulated row already
covers, at the other batch sizes of a selection boundary (the emulation of a wave launch of several hundred LWEs costs
seconds each).
"""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from . import oracle as orc
from .common import Params, REFERENCE_PBS_SHAPES, decrypt_big, encrypt_small, generate_many_lut, make_keys
from .harness import Ctx, oracle_pbs, use_backend

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
CSRC = os.path.join(ROOT, "tfhe_rs_amd", "csrc")
M64 = (1 << 64) - 1

# kernel ids (hip_backend_last_pbs_kernel) and modes (hip_backend_last_pbs_instantiation), include/tfhe_hip_backend.h
GENERIC, WAVE, NTT, MB_GENERIC, EXACT, MB_WAVE, BLOCK, BLOCK2, WAVE3, MB_LATENCY, SPLIT = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13
PLAIN, SHARE, OCTET, LIMBS, L1, PAR, BIG, SLOTS, POSITION = range(9)


def toy(k, N, base_log, level, g=0, n=None, ms_type=0):
    """A toy-n parameter set with a real bootstrap shape (the keyswitch fields are unused here)."""
    if n is None:
        n = 3 * g if g else 5
    pm = 16 if N >= 2048 else 8 if N == 1024 else 4
    return Params(f"k{k}_N{N}_b{base_log}_l{level}_g{g}_n{n}", n, k, N, base_log, level, 4, 4, 45, 17, pm,
                  ms_type=ms_type, grouping=g)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    p: Params
    batch: int
    choice: int          # hip_backend_set_fft_kernel for the launch (0: the automatic choice selects the row)
    inst: tuple          # (kernel id, L, B, G, mode, LWEs per workgroup, N, k + 1)
    engine: str = "fft64"
    many_lut: int = 1    # > 1: a many-LUT call
    gpu_only: bool = False


def C_(id, p, batch, choice, inst, **kw):
    return Case(id, p, batch, choice, inst, **kw)


# ---------------------------------------------------------------- shapes
W23 = toy(1, 2048, 23, 1, ms_type=1)      # PARAM_MESSAGE_2_CARRY_2's decomposition
W22 = toy(1, 2048, 22, 1)
W15 = toy(1, 2048, 15, 2)
E63 = toy(1, 2048, 21, 3, n=7)            # base_log * level = 63, the largest the entry points accept
E62 = toy(1, 2048, 31, 2)
E_L4 = toy(1, 2048, 15, 4)
E_L3 = toy(1, 2048, 12, 3)
E31 = toy(1, 2048, 31, 1)                 # the largest base_log the wave kernel takes
E32 = toy(1, 2048, 32, 1)                 # ... one more: it must leave the wave kernel
MB_G3L2 = toy(1, 2048, 15, 2, g=3)
MB_G3B14 = toy(1, 2048, 14, 2, g=3)
MB_G4L1 = toy(1, 2048, 22, 1, g=4)
MB_G3L1 = toy(1, 2048, 22, 1, g=3)
MB_G2L1 = toy(1, 2048, 22, 1, g=2)
MB_G1 = toy(1, 2048, 15, 2, g=1, n=3)
MB_G2L2 = toy(1, 2048, 15, 2, g=2)        # the reference's GROUP_2 ... MESSAGE_1_CARRY_3 ... 2M64 shape
MB_G3_63 = toy(1, 2048, 21, 3, g=3)
MB_G4B14 = toy(1, 2048, 14, 2, g=4)       # the reference's GROUP_4 ... MESSAGE_1_CARRY_3 ... 2M64 shape
MB_G2_62 = toy(1, 2048, 31, 2, g=2)

NK = [(256, 2), (256, 3), (256, 4), (512, 2), (512, 3), (512, 4), (1024, 2), (1024, 3), (1024, 4), (2048, 2), (2048, 3),
      (4096, 2)]
# a decomposition per ring of the generic rows: the fallback edges spread over them
NK_DECOMP = {(256, 2): (21, 3), (256, 3): (12, 3), (256, 4): (15, 2), (512, 2): (31, 2), (512, 3): (18, 2),
             (512, 4): (10, 4), (1024, 2): (15, 2), (1024, 3): (22, 1), (1024, 4): (16, 3), (2048, 2): (32, 1),
             (2048, 3): (15, 2), (4096, 2): (21, 3)}


def _nk_params(N, K1, g=0):
    bl, lv = NK_DECOMP[(N, K1)]
    return toy(K1 - 1, N, bl, lv, g=g)


def _wave(L, B, per):
    return (WAVE, L, B, 0, PLAIN, per, 2048, 2)


def _mbw(L, B, G, mode, per):
    return (MB_WAVE, L, B, G, mode, per, 2048, 2)


CASES = [
    # -------- classic f64, N = 2048, k = 1: the wave (throughput) kernel
    C_("wave_1_23_w1_forced", W23, 256, 2, _wave(1, 23, 1)),
    C_("wave_1_23_w2", W23, 257, 0, _wave(1, 23, 2)),
    C_("wave_1_23_w4_ragged", W23, 771, 0, _wave(1, 23, 4), gpu_only=True),
    C_("wave_1_22", W22, 9, 2, _wave(1, 22, 1), many_lut=2),
    C_("wave_2_15", W15, 9, 2, _wave(2, 15, 1)),
    C_("wave_0_0_b21_l3_w1", E63, 256, 2, _wave(0, 0, 1), gpu_only=True),
    C_("wave_0_0_b21_l3_w2", E63, 257, 0, _wave(0, 0, 2)),
    C_("wave_0_0_b21_l3_w2_full", E63, 512, 0, _wave(0, 0, 2), gpu_only=True),
    C_("wave_0_0_b21_l3_w3", E63, 513, 0, _wave(0, 0, 3)),
    C_("wave_0_0_b21_l3_w3_full", E63, 768, 0, _wave(0, 0, 3), gpu_only=True),
    C_("wave_0_0_b21_l3_w4_ragged", E63, 769, 0, _wave(0, 0, 4)),
    C_("wave_0_0_b21_l3_w4_full", E63, 1024, 0, _wave(0, 0, 4), gpu_only=True),
    C_("wave_0_0_b31_l2", E62, 9, 2, _wave(0, 0, 1), many_lut=2),
    C_("wave_0_0_b15_l4", E_L4, 9, 2, _wave(0, 0, 1)),
    C_("wave_0_0_b12_l3", E_L3, 9, 2, _wave(0, 0, 1)),
    C_("wave_0_0_b31_l1", E31, 257, 0, _wave(0, 0, 2)),
    C_("b32_l1_leaves_wave", E32, 257, 0, (GENERIC, 0, 0, 0, PAR, 1, 2048, 2)),
    # -------- the block (latency) kernel and its dual-stream variant; 256 / 257 LWEs: latency vs throughput
    C_("block_1_23", W23, 9, 0, (BLOCK, 1, 23, 0, PLAIN, 1, 2048, 2), many_lut=2),
    C_("block_1_23_latency_limit", W23, 256, 0, (BLOCK, 1, 23, 0, PLAIN, 1, 2048, 2), gpu_only=True),
    C_("block_0_0_b21_l3", E63, 9, 0, (BLOCK, 0, 0, 0, PLAIN, 1, 2048, 2)),
    C_("block_0_0_b21_l3_latency_limit", E63, 256, 0, (BLOCK, 0, 0, 0, PLAIN, 1, 2048, 2), gpu_only=True),
    C_("block_0_0_b15_l4", E_L4, 9, 0, (BLOCK, 0, 0, 0, PLAIN, 1, 2048, 2)),
    C_("block_0_0_b32_l1", E32, 9, 0, (BLOCK, 0, 0, 0, PLAIN, 1, 2048, 2)),
    C_("block2_1_23", W23, 9, 4, (BLOCK2, 1, 23, 0, PLAIN, 1, 2048, 2)),
    C_("block2_0_0_b21_l3", E63, 9, 4, (BLOCK2, 0, 0, 0, PLAIN, 1, 2048, 2)),
    C_("block2_0_0_b12_l3", E_L3, 9, 4, (BLOCK2, 0, 0, 0, PLAIN, 1, 2048, 2)),
    # -------- N = 1024: the wave3 kernel, single-level digit path (base_log <= 30) and the general one
    C_("wave3_k1_l1", toy(1, 1024, 23, 1), 9, 0, (WAVE3, 0, 0, 0, L1, 1, 1024, 2), many_lut=2),
    C_("wave3_k1_l2", toy(1, 1024, 15, 2), 9, 0, (WAVE3, 0, 0, 0, PLAIN, 1, 1024, 2)),
    C_("wave3_k2_l1", toy(2, 1024, 23, 1), 9, 0, (WAVE3, 0, 0, 0, L1, 1, 1024, 3)),
    C_("wave3_k2_l1_w2", toy(2, 1024, 23, 1), 257, 0, (WAVE3, 0, 0, 0, L1, 2, 1024, 3)),
    C_("wave3_k2_b31_l1", toy(2, 1024, 31, 1), 9, 0, (WAVE3, 0, 0, 0, PLAIN, 1, 1024, 3)),
    C_("wave3_k2_b21_l3", toy(2, 1024, 21, 3), 9, 0, (WAVE3, 0, 0, 0, PLAIN, 1, 1024, 3)),
    # -------- generic f64 kernels over N x k, and the rings of 2^13 / 2^14 (accumulator in device memory)
    *[C_(f"generic_{N}_{K1}", _nk_params(N, K1), 5, 1, (GENERIC, 0, 0, 0, PAR if K1 == 2 else PLAIN, 1, N, K1),
         many_lut=2 if (N, K1) == (512, 3) else 1) for N, K1 in NK],
    C_("generic_big_8192", toy(1, 8192, 23, 1, n=3), 3, 0, (GENERIC, 0, 0, 0, BIG, 1, 8192, 2)),
    C_("generic_big_16384", toy(1, 16384, 15, 2, n=3), 3, 0, (GENERIC, 0, 0, 0, BIG, 1, 16384, 2)),
    # the centred modulus switch with more mask words than threads: a term in every thread and a ragged last stride
    C_("generic_256_2_centered_n131", toy(1, 256, 21, 3, n=131, ms_type=1), 3, 1, (GENERIC, 0, 0, 0, PAR, 1, 256, 2)),
    C_("ntt_256_2_centered_n131", toy(1, 256, 21, 3, n=131, ms_type=1), 3, 0, (NTT, 0, 0, 0, PAR, 1, 256, 2), engine="ntt64"),
    C_("generic_512_3_centered_n259", toy(2, 512, 18, 2, n=259, ms_type=1), 3, 1, (GENERIC, 0, 0, 0, PLAIN, 1, 512, 3)),
    # -------- multi-bit wave kernel: plain (one LWE per workgroup), SHARE (2 or 4 per workgroup), OCTET (4, L >= 1)
    *[C_(f"mb_wave_{L}_{B}_{G}_plain", p, 9, 2, _mbw(L, B, G, PLAIN, 1), many_lut=2 if G == 2 and L == 0 else 1)
      for p, L, B, G in ((MB_G3L2, 2, 15, 3), (MB_G3B14, 2, 14, 3), (MB_G4L1, 1, 22, 4), (MB_G3L1, 1, 22, 3),
                         (MB_G2L1, 1, 22, 2), (MB_G1, 0, 0, 1), (MB_G2L2, 0, 0, 2), (MB_G3_63, 0, 0, 3),
                         (MB_G4B14, 0, 0, 4))],
    *[C_(f"mb_wave_{L}_{B}_{G}_share", p, 259, 0, _mbw(L, B, G, SHARE, 2), gpu_only=L != 0)
      for p, L, B, G in ((MB_G3L2, 2, 15, 3), (MB_G3B14, 2, 14, 3), (MB_G4L1, 1, 22, 4), (MB_G3L1, 1, 22, 3),
                         (MB_G2L1, 1, 22, 2), (MB_G1, 0, 0, 1), (MB_G2L2, 0, 0, 2), (MB_G3_63, 0, 0, 3),
                         (MB_G4B14, 0, 0, 4))],
    *[C_(f"mb_wave_{L}_{B}_{G}_octet", p, 771, 0, _mbw(L, B, G, OCTET, 4), gpu_only=True)
      for p, L, B, G in ((MB_G3L2, 2, 15, 3), (MB_G3B14, 2, 14, 3), (MB_G4L1, 1, 22, 4), (MB_G3L1, 1, 22, 3),
                         (MB_G2L1, 1, 22, 2))],
    # the fallbacks have no OCTET form: four LWEs per workgroup run as two SHARE quads; 515 LWEs take 4 per workgroup
    C_("mb_wave_0_0_4_share_w4", MB_G4B14, 515, 0, _mbw(0, 0, 4, SHARE, 4)),
    C_("mb_wave_0_0_2_share_w4_ragged", MB_G2_62, 771, 0, _mbw(0, 0, 2, SHARE, 4), gpu_only=True),
    # -------- multi-bit latency path (keybundles, then the products); N = 2048, k = 1: products on the block kernel,
    # keybundles in slot order from 17 LWEs; 256 / 257: the lat_samples limit of N = 2048, k = 1
    C_("mb_lat_block_1_22_position", MB_G4L1, 5, 0, (MB_LATENCY, 1, 22, 0, POSITION, 1, 2048, 2), many_lut=2),
    C_("mb_lat_block_1_22_slots", MB_G4L1, 17, 0, (MB_LATENCY, 1, 22, 0, SLOTS, 1, 2048, 2)),
    C_("mb_lat_block_2_15_position", MB_G3L2, 5, 0, (MB_LATENCY, 2, 15, 0, POSITION, 1, 2048, 2)),
    C_("mb_lat_block_2_15_slots", MB_G3L2, 17, 0, (MB_LATENCY, 2, 15, 0, SLOTS, 1, 2048, 2)),
    C_("mb_lat_block_0_0_position", MB_G3B14, 5, 0, (MB_LATENCY, 0, 0, 0, POSITION, 1, 2048, 2)),
    C_("mb_lat_block_0_0_slots", MB_G4B14, 17, 0, (MB_LATENCY, 0, 0, 0, SLOTS, 1, 2048, 2)),
    C_("mb_lat_block_0_0_b21_l3", MB_G3_63, 5, 0, (MB_LATENCY, 0, 0, 0, POSITION, 1, 2048, 2)),
    # the small-batch side of the reference's one-level g = 2 / g = 3 and two-level g = 2 shapes
    C_("mb_lat_block_1_22_g2", MB_G2L1, 5, 0, (MB_LATENCY, 1, 22, 0, POSITION, 1, 2048, 2)),
    C_("mb_lat_block_1_22_g3", MB_G3L1, 5, 0, (MB_LATENCY, 1, 22, 0, POSITION, 1, 2048, 2)),
    C_("mb_lat_block_2_15_g2", MB_G2L2, 5, 0, (MB_LATENCY, 2, 15, 0, POSITION, 1, 2048, 2)),
    C_("mb_lat_limit_256", MB_G3B14, 256, 0, (MB_LATENCY, 0, 0, 0, SLOTS, 1, 2048, 2), gpu_only=True),
    C_("mb_lat_limit_257", MB_G3B14, 257, 0, _mbw(2, 14, 3, SHARE, 2), gpu_only=True),
    *[C_(f"mb_lat_generic_{N}_{K1}", _nk_params(N, K1, g=3 if K1 != 3 else 2), 5, 6 if (N, K1) == (2048, 2) else 0,
         (MB_LATENCY, 0, 0, 0, PAR if K1 == 2 else PLAIN, 1, N, K1), many_lut=2 if (N, K1) == (1024, 3) else 1)
      for N, K1 in NK],
    # -------- multi-bit one-launch generic kernels
    *[C_(f"mb_generic_{N}_{K1}", _nk_params(N, K1, g=2 if K1 != 4 else 3), 5, 1, (MB_GENERIC, 0, 0, 0, PLAIN, 1, N, K1),
         many_lut=2 if (N, K1) == (256, 2) else 1) for N, K1 in NK],
    # the reference's k = 2, N = 1024 multi-bit shapes with g = 3 and g = 4 (g = 2: mb_*_generic_1024_3 above)
    C_("mb_lat_generic_1024_3_g3", toy(2, 1024, 22, 1, g=3), 5, 0, (MB_LATENCY, 0, 0, 0, PLAIN, 1, 1024, 3)),
    C_("mb_lat_generic_1024_3_g4", toy(2, 1024, 22, 1, g=4), 5, 0, (MB_LATENCY, 0, 0, 0, PLAIN, 1, 1024, 3)),
    C_("mb_generic_1024_3_g3", toy(2, 1024, 22, 1, g=3), 5, 1, (MB_GENERIC, 0, 0, 0, PLAIN, 1, 1024, 3)),
    C_("mb_generic_1024_3_g4", toy(2, 1024, 22, 1, g=4), 5, 1, (MB_GENERIC, 0, 0, 0, PLAIN, 1, 1024, 3)),
    C_("mb_generic_big_8192", toy(1, 8192, 15, 2, g=2, n=2), 3, 0, (MB_GENERIC, 0, 0, 0, BIG, 1, 8192, 2)),
    C_("mb_generic_big_16384", toy(1, 16384, 22, 1, g=1, n=3), 3, 0, (MB_GENERIC, 0, 0, 0, BIG, 1, 16384, 2)),
    # -------- exact engines: the O(N^2) integer kernel, the Goldilocks NTT kernels, the split-key form of the NTT
    *[C_(f"exact_{N}_{K1}", _nk_params(N, K1), 3, 0, (EXACT, 0, 0, 0, PLAIN, 1, N, K1), engine="exact64",
         many_lut=2 if (N, K1) == (256, 3) else 1) for N, K1 in NK],
    *[C_(f"ntt_{N}_{K1}", _nk_params(N, K1), 5, 0, (NTT, 0, 0, 0, PAR if K1 == 2 else PLAIN, 1, N, K1), engine="ntt64",
         many_lut=2 if (N, K1) == (1024, 2) else 1) for N, K1 in NK],
    C_("split_23", toy(1, 2048, 23, 1), 9, 0, (SPLIT, 1, 23, 0, LIMBS, 1, 2048, 2), engine="ntt64_split", many_lut=2),
    C_("split_22", toy(1, 2048, 22, 1), 257, 0, (SPLIT, 1, 22, 0, LIMBS, 2, 2048, 2), engine="ntt64_split"),
]

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


def _case_params():
    out = []
    for c in CASES:
        for kind in ("emu", "hip"):
            if kind == "emu" and c.gpu_only:
                continue
            out.append(pytest.param(kind, c, id=f"{kind}-{c.id}", marks=[pytest.mark.gpu] if kind == "hip" else []))
    return out


# ---------------------------------------------------------------- census (CPU tier, no backend needed)
# (file, dispatch function) pairs whose template launches the census reads
DISPATCHERS = [
    ("pbs_fft_wave.hip", "launch_pbs_fft_wave"),
    ("pbs_fft_wave.hip", "launch_pbs_multi_bit_wave"),
    ("pbs_fft_wave.hip", "launch_pbs_ntt_split_wave"),
    ("pbs_fft_block.hip", "launch_pbs_fft_block"),
    ("pbs_fft_block.hip", "launch_mb_accumulate_block"),
    ("pbs_fft_wave3.hip", "launch_pbs_fft_wave3"),
    ("pbs_generic.hip", "launch_pbs_fft_generic"),
    ("pbs_generic.hip", "launch_pbs_exact_generic"),
    ("pbs_generic.hip", "launch_pbs_ntt_generic"),
    ("multibit.hip", "launch_pbs_multi_bit"),
    ("multibit.hip", "launch_pbs_multi_bit_latency"),
]
KNOWN_INSTANTIATIONS = 88   # 4 + 9 + 2 wave, 4 + 3 block, 2 wave3, 14 f64 + 12 exact + 12 NTT generic, 14 + 12 multi-bit


def _function_body(text, name):
    m = re.search(r"^void " + re.escape(name) + r"\(.*?^\}", text, re.S | re.M)
    assert m, f"dispatch function {name} not found"
    return m.group(0)


def extract_instantiations():
    """{(launcher, 'template,args')} of every launch the dispatch functions can make."""
    found = set()
    shapes = open(os.path.join(CSRC, "pbs_generic.h")).read()
    table = re.search(r"constexpr ShapeNK PBS_SHAPES_NK\[\] = \{(.*?)\};", shapes, re.S)
    assert table, "PBS_SHAPES_NK not found"
    nk = re.findall(r"\{(\d+), (\d+)\}", table.group(1))
    for fname, func in DISPATCHERS:
        body = _function_body(open(os.path.join(CSRC, fname)).read(), func)
        for launcher, args in re.findall(r"\b(launch_\w+)<([^<>()]*)>\s*\(", body):
            found.add((launcher, ",".join(a.strip() for a in args.split(","))))
        for launcher in re.findall(r"dispatch_nk\([^;]*?\b(launch_\w+)<", body):
            found.update((launcher, f"{N},{K1}") for N, K1 in nk)
    return found


def launchers_of(inst):
    """The launcher instantiations a reported instantiation stands for."""
    kid, L, B, G, mode, _, N, K1 = inst
    if kid == WAVE:
        return {("launch_wave_t", f"{L},{B}")}
    if kid == MB_WAVE:
        return {("launch_wave_mb_t", f"{L},{B},{G}")}
    if kid == SPLIT:
        return {("launch_split_t", f"{B}")}
    if kid == BLOCK:
        return {("launch_block_t", f"{L},{B}")}
    if kid == BLOCK2:
        return {("launch_block2_t", f"{L},{B}")}
    if kid == WAVE3:
        return {("launch_wave3_t", f"{K1}")}
    if kid == MB_LATENCY:
        own = {("launch_mb_latency", f"{N},{K1}")}
        return own | ({("launch_block_mb_t", f"{L},{B}")} if mode in (SLOTS, POSITION) else set())
    if kid in (GENERIC, MB_GENERIC):
        if mode == BIG:
            return {("launch_fft_big" if kid == GENERIC else "launch_mb_big", f"{N}")}
        return {("launch_fft" if kid == GENERIC else "launch_mb", f"{N},{K1}")}
    if kid == EXACT:
        return {("launch_exact", f"{N},{K1}")}
    if kid == NTT:
        return {("launch_ntt", f"{N},{K1}")}
    raise AssertionError(f"unknown kernel id {kid}")


def test_every_dispatched_instantiation_has_a_row():
    found = extract_instantiations()
    assert len(found) >= KNOWN_INSTANTIATIONS, sorted(found)
    covered = set()
    for c in CASES:
        covered |= launchers_of(c.inst)
    missing = sorted(found - covered)
    assert not missing, f"instantiations without a bit-exact row in CASES: {missing}"
    assert not sorted(covered - found), "rows for instantiations the dispatchers no longer launch"


def test_every_mode_of_the_multi_bit_kernels_has_a_row():
    """The wave kernel's multi-bit launcher picks plain / SHARE / OCTET (OCTET only for a compile-time level count) and
    the latency path's block products slot or position order: each pair of instantiation and mode needs its own row."""
    modes = {}
    for c in CASES:
        kid, L, B, G, mode = c.inst[:5]
        modes.setdefault((kid, L, B, G), set()).add(mode)
    for launcher, args in extract_instantiations():
        if launcher == "launch_wave_mb_t":
            L, B, G = map(int, args.split(","))
            want = {PLAIN, SHARE} | ({OCTET} if L >= 1 else set())
            assert want <= modes.get((MB_WAVE, L, B, G), set()), (args, modes.get((MB_WAVE, L, B, G)))
        if launcher == "launch_block_mb_t":
            L, B = map(int, args.split(","))
            assert {SLOTS, POSITION} <= modes.get((MB_LATENCY, L, B, 0), set()), args
        if launcher == "launch_wave3_t":
            assert {L1, PLAIN} <= modes.get((WAVE3, 0, 0, 0), set())


def test_case_rows_are_consistent():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    for c in CASES:
        p = c.p
        kid, _, _, G, _, per, N, K1 = c.inst
        assert (N, K1) == (p.N, p.k + 1), c.id
        assert bool(p.grouping) == (kid in (MB_WAVE, MB_LATENCY, MB_GENERIC)), c.id
        assert not G or G == p.grouping, c.id
        assert p.pbs_base_log * p.pbs_level < 64, c.id
        if p.grouping:
            assert p.n % p.grouping == 0 and (p.n // p.grouping) % 2 == 1, c.id   # g times an odd number
        else:
            assert p.n % 2 == 1, c.id
        if kid in (WAVE, MB_WAVE):
            want = min(4, (c.batch + 255) // 256)
            assert per == (4 if kid == MB_WAVE and want == 3 else want), c.id


# ---------------------------------------------------------------- reference parameter sets -> instantiation
def _row_for_shape(s):
    """The CASES rows a reference shape runs on: same (k, N, level, base_log, g)."""
    return [c for c in CASES if c.engine == "fft64" and (c.p.k, c.p.N, c.p.pbs_base_log, c.p.pbs_level, c.p.grouping) ==
            (s.k, s.N, s.pbs_base_log, s.pbs_level, s.grouping)]


def expected_default_instantiations(s):
    """What the automatic choice runs a reference shape on: (small batch, large batch) instantiation heads."""
    if s.grouping == 0:
        if s.N == 2048:
            tl = (s.pbs_level, s.pbs_base_log) if (s.pbs_level, s.pbs_base_log) == (1, 23) else (0, 0)
            tw = (s.pbs_level, s.pbs_base_log) if (s.pbs_level, s.pbs_base_log) in ((1, 23), (1, 22), (2, 15)) else (0, 0)
            return (BLOCK, *tl), (WAVE, *tw)
        return (WAVE3, 0, 0), (WAVE3, 0, 0)
    if s.N == 2048:
        compiled = {(2, 15, 3), (2, 14, 3), (1, 22, 4), (1, 22, 3), (1, 22, 2)}
        key = (s.pbs_level, s.pbs_base_log, s.grouping)
        tw = key[:2] if key in compiled else (0, 0)
        tb = (s.pbs_level, s.pbs_base_log) if (s.pbs_level, s.pbs_base_log) in ((1, 22), (2, 15)) else (0, 0)
        return (MB_LATENCY, *tb), (MB_WAVE, *tw)
    return (MB_LATENCY, 0, 0), (MB_GENERIC, 0, 0)


def test_reference_shapes_have_rows():
    """Every reference shape on N = 1024 / 2048 is exercised by at least one bit-exact row, on the instantiations the
    automatic choice takes for it (DESIGN.md lists the shapes that land on a run-time decomposition fallback)."""
    assert len(REFERENCE_PBS_SHAPES) == 12 and sum(s.count for s in REFERENCE_PBS_SHAPES) == 199
    for s in REFERENCE_PBS_SHAPES:
        rows = _row_for_shape(s)
        assert rows, s.name
        small, large = expected_default_instantiations(s)
        heads = {c.inst[:3] for c in rows}
        if s.N == 2048:
            assert small in heads and large in heads, (s.name, small, large, heads)
        else:
            assert any(h[0] in (WAVE3, MB_LATENCY, MB_GENERIC) for h in heads), s.name


# ---------------------------------------------------------------- the bit-exact launches
_ctx_cache = {}


def _ctx(kind, p, engine):
    key = (kind, p, engine)
    if key not in _ctx_cache:
        _ctx_cache[key] = Ctx(kind, p, make_keys(p, with_ksk=False), engine)
    use_backend(kind)
    return _ctx_cache[key]


def boundary_lut(p, seed=77):
    """test_decomposer_boundary_digits_in_every_fft_kernel's accumulator: neighbouring coefficients 2^63 +- (less than
    2^40) apart, so that the first rotations put the decomposer on its B/2 states with both signs."""
    rng = np.random.default_rng(seed)
    lut = rng.integers(0, 1 << 39, size=(p.k + 1) * p.N, dtype=np.uint64)
    lut[1::2] += np.uint64(1 << 63)
    lut[2::4] -= np.uint64(1 << 40)
    return lut


def boundary_cts(p, count, seed=78):
    rng = np.random.default_rng(seed)
    cts = rng.integers(0, 1 << 64, size=(count, p.n + 1), dtype=np.uint64)
    cts[:, 0] |= np.uint64(1 << 52)
    cts[:, 0] &= np.uint64(~((1 << 51) | (1 << 50)) & M64)
    return cts


def last_instantiation(lib):
    v = (C.c_uint32 * 8)()
    lib.hip_backend_last_pbs_instantiation(v)
    return tuple(v)


def _oracle_engine(engine):
    return "ntt64" if engine == "ntt64_split" else engine


def _run_case(kind, case):
    p = case.p
    c = _ctx(kind, p, case.engine)
    B, pm = case.batch, p.plaintext_modulus
    rng = np.random.default_rng(B * 7919 + p.N)
    nb = max(1, B // 6) if case.many_lut == 1 else 0      # random ciphertexts on the boundary accumulator
    if case.many_lut == 1:
        f = lambda x: (3 * x + 1) % pm
        msgs = [i % pm for i in range(B - nb)]
        luts = np.stack([orc.generate_lut(p.k, p.N, pm, p.delta, f), boundary_lut(p)])
        fs = [f]
    else:
        fs = [lambda x: (x + 1) % pm, lambda x: (3 * x) % pm]
        acc, max_degree, stride = generate_many_lut(p, fs)
        msgs = [i % (max_degree + 1) for i in range(B)]
        luts = acc[None, :]
    cts = np.concatenate([encrypt_small(p, c.keys, msgs, seed=B + 5)] + ([boundary_cts(p, nb)] if nb else []))
    lut_of_ct = np.array([0] * len(msgs) + [1] * nb)
    in_idx = rng.permutation(B)          # launch slot i reads ciphertext in_idx[i] ...
    out_idx = rng.permutation(B)         # ... writes output out_idx[i], with LUT lut_of_ct[in_idx[i]]
    lut_idx = lut_of_ct[in_idx]
    try:
        c.lib.hip_backend_set_fft_kernel(case.choice)
        out = c.pbs(cts, luts, lut_indexes=lut_idx, in_indexes=in_idx, out_indexes=out_idx,
                    out_count=B * case.many_lut, num_many_lut=case.many_lut,
                    lut_stride=stride if case.many_lut > 1 else 0)
        inst = last_instantiation(c.lib)
    finally:
        c.lib.hip_backend_set_fft_kernel(0)
    assert inst == case.inst, f"{case.id}: ran {inst}, the row is for {case.inst}"
    # oracle, per LUT, on the gathered inputs, scattered like the kernel scatters
    ref = np.zeros((B, p.k * p.N + 1), dtype=np.uint64)
    for li in range(len(luts)):
        sel = np.nonzero(lut_idx == li)[0]
        if sel.size:
            ref[out_idx[sel]] = oracle_pbs(p, c.keys, _oracle_engine(case.engine), cts[in_idx[sel]], luts[li])
    bad = np.nonzero((out[:B] != ref).any(axis=1))[0]
    assert bad.size == 0, f"{case.id}: {bad.size} of {B} outputs differ from the oracle (first at output {bad[:8]})"
    # many-LUT: function t is the sample extraction at t * stride of the same accumulator — its mask is a signed
    # permutation of the accumulator's mask, which the first function's (bit-exact) output carries in full
    for t in range(1, case.many_lut):
        for o in range(B):
            glwe = np.zeros((p.k + 1) * p.N, dtype=np.uint64)
            for q in range(p.k):
                a = ref[o, q * p.N:(q + 1) * p.N]
                glwe[q * p.N] = a[0]
                glwe[q * p.N + 1:(q + 1) * p.N] = (np.uint64(0) - a[1:][::-1])
            want = orc.sample_extract(glwe, p.k, p.N, t * stride)[:p.k * p.N]
            assert np.array_equal(out[t * B + o, :p.k * p.N], want), f"{case.id}: many-LUT mask of function {t}"
    # decryption of the plaintext part (the boundary ciphertexts are random)
    for t in range(case.many_lut):
        ft = fs[t] if case.many_lut > 1 else fs[0]
        for i in range(B):
            if lut_idx[i] == 0:
                got = decrypt_big(p, c.keys, out[t * B + out_idx[i]])
                assert got == ft(msgs[in_idx[i]]), f"{case.id}: slot {i} (function {t}) decrypts to {got}"


@pytest.mark.parametrize("kind,case", _case_params())
def test_instantiation_bit_exact(kind, case):
    _run_case(kind, case)


@pytest.mark.parametrize("kind", BACKENDS)
def test_hook_reports_every_instantiation_of_the_split_engine_not_its_redo(kind):
    """The split-key engine's launch is followed by the integer kernel's redo launch (it returns at once when nothing
    was flagged): the hook keeps reporting the split-key instantiation."""
    case = next(c for c in CASES if c.id == "split_23")
    c = _ctx(kind, case.p, case.engine)
    cts = encrypt_small(case.p, c.keys, [1, 2, 3], seed=4)
    lut = orc.generate_lut(case.p.k, case.p.N, case.p.plaintext_modulus, case.p.delta, lambda x: x)
    c.pbs(cts, lut)
    assert last_instantiation(c.lib) == case.inst
