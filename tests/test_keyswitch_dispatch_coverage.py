"""Every kernel form the keyswitch can launch, word for word against the oracle.

A keyswitch call reaches one of the compiled forms of keyswitch.hip — ks_mfma_kernel<LEVEL, PADDED, OutT, KSPLIT>,
ks_digits_kernel<LEVEL, PADDED> + ks_gemm_kernel<OutT, SPB>, or one of the four scalar kernels — chosen by n_in, the
decomposition, the key width, the batch size, hip_backend_set_keyswitch_kernel and hip_backend_set_keyswitch_kparts.
CASES has one row per reachable (form, mode); each row runs on both backends and checks
  - the output against orc.keyswitch_batch / orc.keyswitch_64_32, word for word, gathered and scattered through
    non-trivial index vectors, into an output array pre-filled with a sentinel and followed by a guard row;
  - the output of the scalar kernels (choice 1) against the same words where they take the level count (<= 8);
  - that hip_backend_last_keyswitch_instantiation reports the form the row is for.
Inputs are uniform random ciphertexts and uniform random KEY WORDS: the sums are exact integers modulo 2^64 (2^32)
whatever the key holds, so no key is generated and nothing is decrypted.

Further down: the shape rule of the matrix-core paths as a table, the int32 / split-u64 accumulators driven to the
largest sums a ciphertext can produce, the eviction order of the key-layout cache, the production shapes at batch
sizes up to the benchmark's 4096 (MI355X only), and a census that reads keyswitch.hip and fails on a launchable form
without a row.  Rows marked gpu_only cost the emulation more than their worth; what they run is stated per row.
"""
import ctypes as C
import dataclasses
import functools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tfhe_rs_amd import core_crypto_gpu as gpu

from . import oracle as orc
from .harness import use_backend
from .test_error_behaviour import run as run_child

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
KEYSWITCH_HIP = os.path.join(ROOT, "tfhe_rs_amd", "csrc", "keyswitch.hip")
U64, U32 = np.uint64, np.uint32
SENTINEL = 0xD1D1D1D1D1D1D1D1
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]

# hip_backend_last_keyswitch_instantiation (include/tfhe_hip_backend.h): (path, scalar kernel, LEVEL, PADDED, key bits,
# KSPLIT, kparts, SPB + 256 * column tiles)
SMALL_BASE, DIGITS32, DIGITS64, KS32 = 1, 2, 3, 4
KSM_CT, KS_MAXL, GEMM_AUTO, GEMM_FORCED, KPARTS_DEFAULT = 32, 8, 769, 129, 8


def one(level, padded, bits, ksplit, kparts, col_tiles):
    """ks_mfma_kernel<level, padded, u{bits}, ksplit> over `kparts` workgroups per column tile."""
    return (1, 0, level, int(padded), bits, ksplit, kparts, 256 * col_tiles)


def gemm(level, padded, bits, spb, col_tiles):
    """ks_digits_kernel<level, padded>, then ks_gemm_kernel<u{bits}, spb>."""
    return (2, 0, level, int(padded), bits, 0, 0, spb + 256 * col_tiles)


def scalar(kernel, bits=64):
    return (0, kernel, 0, 0, bits, 0, 0, 0)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    n_in: int
    n_out: int
    base_log: int
    level: int
    bits: int            # key and output width
    batch: int
    choice: int          # hip_backend_set_keyswitch_kernel for the launch
    inst: tuple          # what hip_backend_last_keyswitch_instantiation must report
    kparts: int = KPARTS_DEFAULT   # hip_backend_set_keyswitch_kparts for the launch
    dup: bool = False    # the last launch slot gathers the same input as the first
    gpu_only: bool = False


def C_(id, n_in, n_out, ks, bits, batch, choice, inst, **kw):
    return Case(id, n_in, n_out, ks[0], ks[1], bits, batch, choice, inst, **kw)


# ---------------------------------------------------------------- the rows
# (tag, (base_log, level), LEVEL, PADDED) per key width: every pair ksm_with_level can pick.  (6, 1), (5, 2), (2, 9),
# (3, 11), (2, 16): test_backend_parity._KS_EVERY_PADDING; (4, 4), (3, 5), (4, 8): the production decompositions and the
# widest the 32-bit key takes at 8 levels; (5, 3) pads 3 levels to 4; (3, 16): 48 bits, the 64-bit decomposition at 16
FORMS = {
    64: [("1", (6, 1), 1, False), ("2", (5, 2), 2, False), ("4", (4, 4), 4, False), ("4p", (5, 3), 4, True),
         ("8", (4, 8), 8, False), ("8p", (3, 5), 8, True), ("16", (3, 16), 16, False), ("16p", (3, 11), 16, True),
         ("16p_2x9", (2, 9), 16, True)],
    32: [("1", (6, 1), 1, False), ("2", (5, 2), 2, False), ("4", (4, 4), 4, False), ("4p", (5, 3), 4, True),
         ("8", (4, 8), 8, False), ("8p", (3, 5), 8, True), ("16", (2, 16), 16, False), ("16p", (2, 9), 16, True)],
}
SPB_WANT = {64: 2, 32: 4}
NOUT = 40                 # 41 columns: two column tiles, the second one ragged


def _form_rows():
    rows = []
    for bits, forms in FORMS.items():
        for tag, ks, L, P in forms:
            n_in = 2048 // L          # 64 steps of 32 k at every LEVEL: divisible by 4 * 8 parts
            rows += [
                C_(f"mfma_{tag}_u{bits}_split4", n_in, NOUT, ks, bits, 7, 0, one(L, P, bits, 4, 8, 2), dup=L == 4),
                C_(f"mfma_{tag}_u{bits}_split1", n_in, NOUT, ks, bits, 40, 0, one(L, P, bits, 1, 8, 2)),
                C_(f"digits_{tag}_u{bits}_gemm{SPB_WANT[bits]}", n_in, NOUT, ks, bits, 131, 3, gemm(L, P, bits, SPB_WANT[bits], 2)),
            ]
    return rows


def _kparts_rows():
    rows = []
    for parts in (1, 2, 4, 8, 16):     # n_in = 2048 at 4 levels: 256 steps, every power of two up to 16 divides
        rows.append(C_(f"kparts_{parts}_y", 2048, NOUT, (4, 4), 64, 7, 0, one(4, False, 64, 4, parts, 2), kparts=parts))
        rows.append(C_(f"kparts_{parts}_z", 2048, NOUT, (4, 4), 64, 40, 0, one(4, False, 64, 1, parts, 2), kparts=parts))
    # 3 parts: 96 steps divide by 4 * 3, 256 do not (one workgroup per column tile then); 16 parts at 96 steps neither
    rows += [
        C_("kparts_3_divides_y", 768, NOUT, (4, 4), 64, 9, 0, one(4, False, 64, 4, 3, 2), kparts=3),
        C_("kparts_3_divides_z", 768, NOUT, (4, 4), 32, 70, 0, one(4, False, 32, 1, 3, 2), kparts=3),
        C_("kparts_3_falls_back_y", 2048, NOUT, (4, 4), 32, 9, 0, one(4, False, 32, 4, 1, 2), kparts=3),
        C_("kparts_3_falls_back_z", 2048, NOUT, (4, 4), 64, 70, 0, one(4, False, 64, 1, 1, 2), kparts=3),
        C_("kparts_16_falls_back_y", 768, NOUT, (4, 4), 64, 32, 0, one(4, False, 64, 4, 1, 2), kparts=16),
        C_("kparts_16_falls_back_z", 768, NOUT, (4, 4), 64, 128, 0, one(4, False, 64, 1, 1, 2), kparts=16),
    ]
    return rows


def _batch_edge_rows():
    """One shape (1024 -> 40, 4 x 4: 128 steps), every batch size at which the launch changes: the wave split up to 32
    LWEs, one workgroup row up to 128, the parts halved per doubling of the workgroup rows (129: 2 rows, 4 parts; 257:
    3 rows, still 4 — the rows are halved, not divided; 385: 4 rows, 2 parts), the automatic GEMM from 769."""
    rows = []
    for batch, ksplit, parts in ((1, 4, 8), (16, 4, 8), (17, 4, 8), (31, 4, 8), (32, 4, 8), (33, 1, 8), (127, 1, 8),
                                 (128, 1, 8), (129, 1, 4), (256, 1, 4), (257, 1, 4), (385, 1, 2)):
        rows.append(C_(f"batch_{batch}", 1024, NOUT, (4, 4), 64, batch, 0, one(4, False, 64, ksplit, parts, 2)))
    rows += [
        C_("batch_768_last_one_launch", 1024, NOUT, (4, 4), 64, 768, 0, one(4, False, 64, 1, 2, 2), gpu_only=True),
        C_("batch_769_first_gemm", 1024, NOUT, (4, 4), 64, 769, 0, gemm(4, False, 64, 2, 2), gpu_only=True),
        C_("batch_1000_gemm", 1024, NOUT, (4, 4), 32, 1000, 0, gemm(4, False, 32, 4, 2), gpu_only=True),
        C_("batch_1000_one_launch_forced", 1024, NOUT, (4, 4), 64, 1000, 2, one(4, False, 64, 1, 1, 2), gpu_only=True),
    ]
    return rows


def _column_edge_rows():
    rows = []
    for ncols in (31, 32, 33, 64, 65):      # columns (n_out + 1) around one and two column tiles
        ct = (ncols + KSM_CT - 1) // KSM_CT
        rows += [
            C_(f"cols_{ncols}_mfma_u64", 256, ncols - 1, (4, 4), 64, 7, 0, one(4, False, 64, 4, 8, ct)),
            C_(f"cols_{ncols}_mfma_u32", 256, ncols - 1, (4, 4), 32, 40, 0, one(4, False, 32, 1, 8, ct)),
            C_(f"cols_{ncols}_gemm_u64", 256, ncols - 1, (4, 4), 64, 131, 3, gemm(4, False, 64, 2, ct)),
            C_(f"cols_{ncols}_gemm_u32", 256, ncols - 1, (3, 5), 32, 131, 3, gemm(8, True, 32, 4, ct)),
        ]
    for ncols in (255, 256, 257):           # the scalar kernels' 256 columns per workgroup
        rows += [
            C_(f"cols_{ncols}_small_base", 64, ncols - 1, (4, 4), 64, 17, 1, scalar(SMALL_BASE)),
            C_(f"cols_{ncols}_digits32", 64, ncols - 1, (31, 2), 64, 17, 1, scalar(DIGITS32)),
            C_(f"cols_{ncols}_digits64", 64, ncols - 1, (32, 1), 64, 17, 1, scalar(DIGITS64)),
            C_(f"cols_{ncols}_ks32", 64, ncols - 1, (4, 4), 32, 17, 1, scalar(KS32, 32)),
        ]
    return rows


def _scalar_rows():
    """Each scalar kernel at n_in = 31, 33 and 918 (a ragged last LDS stage of 32 mask elements) and 32, with 15, 16 and
    17 LWEs (16 per workgroup).  Which kernel: the small-base one while base_log + 33 + log2(n_in * level) <= 64, int32
    digits up to base_log 31, int64 digits above; the 64 -> 32 kernel for a 32-bit key."""
    rows = []
    for n_in, batch in ((31, 15), (32, 16), (33, 17), (918, 17)):
        wide = (21, 3) if n_in == 918 else (31, 2)      # 63 and 62 bits on int32 digits
        rows += [
            C_(f"scalar_small_base_n{n_in}", n_in, 20, (4, 4), 64, batch, 1, scalar(SMALL_BASE), dup=n_in == 33),
            C_(f"scalar_digits32_n{n_in}", n_in, 20, wide, 64, batch, 1, scalar(DIGITS32)),
            C_(f"scalar_digits64_b32_n{n_in}", n_in, 20, (32, 1), 64, batch, 1, scalar(DIGITS64)),
            C_(f"scalar_digits64_b63_n{n_in}", n_in, 20, (63, 1), 64, batch, 1, scalar(DIGITS64)),
            C_(f"scalar_ks32_n{n_in}", n_in, 20, (4, 8), 32, batch, 1, scalar(KS32, 32)),
        ]
    # 32 bits exactly on the 32-bit key, by the automatic choice: 2 x 16 is the matrix cores', 8 x 4 the scalar kernel's
    rows += [
        C_("ks32_32_bits_2x16_matrix_cores", 64, 20, (2, 16), 32, 17, 0, one(16, False, 32, 4, 8, 1)),
        C_("ks32_32_bits_8x4_scalar", 64, 20, (8, 4), 32, 17, 0, scalar(KS32, 32)),
    ]
    return rows


CASES = [
    *_form_rows(),
    # -------- the GEMM forms that need a step count that is odd or 2 mod 4 (<u64,2> and <u32,4>: the rows above)
    C_("gemm_u64_spb1_steps3", 96, NOUT, (6, 1), 64, 131, 3, gemm(1, False, 64, 1, 2)),
    C_("gemm_u32_spb1_steps3", 96, NOUT, (6, 1), 32, 131, 3, gemm(1, False, 32, 1, 2)),
    C_("gemm_u64_spb2_steps10", 160, NOUT, (5, 2), 64, 131, 3, gemm(2, False, 64, 2, 2)),
    C_("gemm_u32_spb2_steps10", 160, NOUT, (5, 2), 32, 131, 3, gemm(2, False, 32, 2, 2)),
    C_("gemm_u64_spb1_steps115", 920, NOUT, (4, 4), 64, 131, 3, gemm(4, False, 64, 1, 2)),
    C_("gemm_u32_spb1_steps115", 920, NOUT, (4, 4), 32, 131, 3, gemm(4, False, 32, 1, 2), dup=True),
    C_("gemm_u64_spb2_steps230_three_workgroup_rows", 920, NOUT, (3, 5), 64, 261, 3, gemm(8, True, 64, 2, 2)),
    # -------- a step count that 4 does not divide, up to 32 LWEs: the un-split kernel, one workgroup per column tile
    C_("unsplit_steps115_u64", 920, NOUT, (4, 4), 64, 7, 0, one(4, False, 64, 1, 1, 2)),
    C_("unsplit_steps115_u32", 920, NOUT, (4, 4), 32, 32, 0, one(4, False, 32, 1, 1, 2)),
    C_("unsplit_steps3_u64", 96, NOUT, (6, 1), 64, 32, 0, one(1, False, 64, 1, 1, 2)),
    C_("unsplit_steps10_u32", 160, NOUT, (5, 2), 32, 17, 0, one(2, False, 32, 1, 1, 2)),
    C_("unsplit_steps115_70_lwes", 920, NOUT, (4, 4), 64, 70, 0, one(4, False, 64, 1, 1, 2)),
    # steps 4 divides but 4 * 8 does not: the waves split K, the workgroups do not
    C_("split4_kparts1_steps12", 96, NOUT, (4, 4), 64, 7, 0, one(4, False, 64, 4, 1, 2)),
    *_kparts_rows(),
    *_batch_edge_rows(),
    *_column_edge_rows(),
    *_scalar_rows(),
]


# ---------------------------------------------------------------- the dispatch rules, restated
def shape_rule(n_in, n_out, base_log, level):
    """ksm_shape: (level_pad, steps, column tiles, the matrix-core paths take the shape)."""
    level_pad = 1
    while level_pad < level:
        level_pad *= 2
    K = n_in * level_pad
    log_k = (K - 1).bit_length()
    ok = level_pad <= 16 and K % 32 == 0 and base_log <= 6 and base_log + 7 + log_k <= 31
    return level_pad, K // 32, (n_out + 1 + KSM_CT - 1) // KSM_CT, ok


def scalar_rule(n_in, base_log, level, bits):
    if bits == 32:
        return KS32
    log_terms = (n_in * level - 1).bit_length()
    return SMALL_BASE if base_log + 33 + log_terms <= 64 else DIGITS32 if base_log <= 31 else DIGITS64


def expected_instantiation(c):
    level_pad, steps, col_tiles, ok = shape_rule(c.n_in, c.n_out, c.base_log, c.level)
    if c.choice == 1 or not ok:
        return scalar(scalar_rule(c.n_in, c.base_log, c.level, c.bits), c.bits)
    padded = c.level < level_pad
    if c.choice != 2 and c.batch >= (GEMM_FORCED if c.choice == 3 else GEMM_AUTO):
        want = SPB_WANT[c.bits]
        spb = 4 if want >= 4 and steps % 4 == 0 else 2 if want >= 2 and steps % 2 == 0 else 1
        return gemm(level_pad, padded, c.bits, spb, col_tiles)
    split = c.batch <= 32 and steps % 4 == 0
    want, rows = c.kparts, (c.batch + 127) // 128
    while rows > 1 and want > 1:
        rows, want = rows >> 1, want >> 1
    kparts = want if want > 1 and steps % (4 * want) == 0 else 1
    return one(level_pad, padded, c.bits, 4 if split else 1, kparts, col_tiles)


def test_case_rows_are_consistent():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    for c in CASES:
        assert c.base_log * c.level <= (63 if c.bits == 64 else 32), c.id
        assert c.inst == expected_instantiation(c), (c.id, c.inst, expected_instantiation(c))
        if c.inst[0] == 0:
            assert c.level <= KS_MAXL, c.id
    # the column tiles: at least two, the last one ragged, wherever the row is not about the column count itself
    for c in CASES:
        if c.inst[0] != 0 and not c.id.startswith(("cols_", "ks32_32_bits")):
            assert c.n_out + 1 > KSM_CT and (c.n_out + 1) % KSM_CT, c.id
    assert any(c.dup for c in CASES)


# ---------------------------------------------------------------- census (CPU tier, no backend needed)
# launchable forms per family, as a floor.  ks_gemm_kernel is compiled in 6 forms; <u64,4> is never launched (launch_ks_gemm
# wants at most 2 steps per barrier for a 64-bit key), so 5 can run
KNOWN_FORMS = {"ks_mfma_kernel": 32, "ks_digits_kernel": 8, "ks_gemm_kernel": 5, "scalar": 4, "ks_zero_outputs_kernel": 2,
               "ksk_planes_kernel": 2}


def _function_body(text, name):
    m = re.search(r"^(?:static |void )[^\n;]*\b" + re.escape(name) + r"\(.*?^\}", text, re.S | re.M)
    assert m, f"{name} not found in keyswitch.hip"
    return m.group(0)


def extract_forms():
    """Every kernel form the launch code of keyswitch.hip can launch, as 'kernel<arguments>' strings."""
    text = open(KEYSWITCH_HIP).read()
    body = {f: _function_body(text, f) for f in ("ksm_with_level", "ksm_launch_one", "ksm_launch_digits_gemm", "launch_ks_gemm",
                                                 "ksm_planes", "launch_keyswitch", "launch_keyswitch_64_32")}
    levels = {(int(L), P == "true") for L, P in
              re.findall(r"f\(std::integral_constant<int, (\d+)>\{\}, std::(true|false)_type\{\}\)", body["ksm_with_level"])}
    # the key widths: one KsCall<...> per entry point
    widths = set()
    for f in ("launch_keyswitch", "launch_keyswitch_64_32"):
        m = re.search(r"KsCall<uint(\d+)_t>", body[f])
        assert m and "keyswitch_front(" in body[f], f
        widths.add(int(m.group(1)))
    found = set()
    ksplits = set()
    for args in re.findall(r"HX_LAUNCH\(\(ks_mfma_kernel<([^>]*)>\)", body["ksm_launch_one"]):
        parts = [a.strip() for a in args.split(",")]
        assert parts[:3] == ["LEVEL", "PADDED", "OutT"], args
        ksplits.add(int(parts[3]) if len(parts) > 3 else 1)
    found |= {f"ks_mfma_kernel<{L},{int(P)},u{w},{s}>" for L, P in levels for w in widths for s in ksplits}
    assert re.search(r"HX_LAUNCH\(\(ks_digits_kernel<decltype\(L\)::value, decltype\(P\)::value>\)", body["ksm_launch_digits_gemm"])
    found |= {f"ks_digits_kernel<{L},{int(P)}>" for L, P in levels}
    for spb in re.findall(r"HX_LAUNCH\(\(ks_gemm_kernel<OutT, (\d+)>\)", body["launch_ks_gemm"]):
        # a 64-bit key never takes 4 steps per barrier (WANT)
        found |= {f"ks_gemm_kernel<u{w},{spb}>" for w in widths if int(spb) <= SPB_WANT[w]}
    assert re.search(r"WANT = sizeof\(OutT\) == 8 \? 2 : 4", body["launch_ks_gemm"])
    for f in ("launch_keyswitch", "launch_keyswitch_64_32"):
        for k in re.findall(r"HX_LAUNCH\(\(?(keyswitch\w*kernel(?:<\w+>)?)\)?,", body[f]):
            found.add(k)
    if "ks_zero_outputs_kernel<OutT>" in body["ksm_launch_one"]:
        found |= {f"ks_zero_outputs_kernel<u{w}>" for w in widths}
    if "ksk_planes_kernel<OutT>" in body["ksm_planes"]:
        found |= {f"ksk_planes_kernel<u{w}>" for w in widths}
    return found


SCALAR_NAMES = {SMALL_BASE: "keyswitch_small_base_kernel", DIGITS32: "keyswitch_kernel<int32_t>",
                DIGITS64: "keyswitch_kernel<int64_t>", KS32: "keyswitch_64_32_kernel"}


def forms_of(inst):
    """The kernel forms a reported instantiation stands for."""
    path, sk, L, P, bits, ksplit, kparts, word = inst
    if path == 0:
        return {SCALAR_NAMES[sk]}
    own = {f"ksk_planes_kernel<u{bits}>"}
    if path == 1:
        return own | {f"ks_mfma_kernel<{L},{P},u{bits},{ksplit}>"} | ({f"ks_zero_outputs_kernel<u{bits}>"} if kparts > 1 else set())
    return own | {f"ks_digits_kernel<{L},{P}>", f"ks_gemm_kernel<u{bits},{word % 256}>"}


def test_every_keyswitch_form_has_a_row():
    found = extract_forms()
    for family, floor in KNOWN_FORMS.items():
        have = [f for f in found if (f.startswith("keyswitch") if family == "scalar" else f.startswith(family + "<"))]
        assert len(have) >= floor, (family, sorted(have))
    covered = set()
    for c in CASES:
        covered |= forms_of(c.inst)
    assert not sorted(found - covered), f"kernel forms without a row in CASES: {sorted(found - covered)}"
    assert not sorted(covered - found), f"rows for forms keyswitch.hip no longer launches: {sorted(covered - found)}"
    # every matrix-core form on the emulation too, not on the MI355X alone
    emu = set()
    for c in CASES:
        if not c.gpu_only:
            emu |= forms_of(c.inst)
    assert emu == found


# ---------------------------------------------------------------- launching
_streams = {}


def _backend(kind):
    lib = use_backend(kind)
    if kind not in _streams:
        _streams[kind] = gpu.CudaStreams.new_single_gpu(0)
    return lib, _streams[kind]


def last_instantiation(lib):
    v = (C.c_uint32 * 8)()
    lib.hip_backend_last_keyswitch_instantiation(v)
    return tuple(v)


@functools.lru_cache(maxsize=8)
def uniform_key(n_in, n_out, level, bits):
    """Uniform words in the keyswitch key's layout [n_in][level][n_out + 1] (tests/test_rerand.py::uniform_ksk)."""
    rng = np.random.default_rng(n_in * 131 + n_out * 17 + level)
    words = rng.integers(0, 1 << 64, size=n_in * level * (n_out + 1), dtype=U64)
    return words if bits == 64 else (words >> U64(32)).astype(U32)


_pool = ThreadPoolExecutor(8)


def oracle_keyswitch(cts, key, n_in, n_out, base_log, level, bits):
    if bits == 64:
        return orc.keyswitch_batch(cts, key, n_in, n_out, base_log, level)
    # one C call per ciphertext (ctypes drops the interpreter lock around it)
    return np.stack(list(_pool.map(lambda ct: orc.keyswitch_64_32(ct, key, n_in, n_out, base_log, level), cts)))


def index_vectors(rng, pool, batch, dup=False):
    """Launch slot i reads ciphertext in_idx[i] of `pool` and writes output out_idx[i] of `batch`."""
    in_idx = rng.permutation(pool)[:batch].astype(U64)
    if dup and batch > 1:
        in_idx[-1] = in_idx[0]
    return in_idx, rng.permutation(batch).astype(U64)


class Launcher:
    """A key and a ciphertext pool on the device; launch() runs one keyswitch into a sentinel-filled output."""

    def __init__(self, kind, cts, key, n_in, n_out, base_log, level):
        self.lib, self.st = _backend(kind)
        self.n_in, self.n_out, self.dtype = n_in, n_out, key.dtype
        self.d_key = gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(key, n_in, n_out, base_log, level, self.st)
        self.d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(cts, self.st)

    def launch(self, in_idx, out_idx, choice=0, kparts=KPARTS_DEFAULT):
        lib, st, batch = self.lib, self.st, len(in_idx)
        fill = np.full((batch + 1) * (self.n_out + 1), SENTINEL & ((1 << (8 * self.dtype.itemsize)) - 1), dtype=self.dtype)
        d_out = gpu.CudaLweCiphertextList(gpu.CudaVec.from_cpu_async(fill, st), batch, self.n_out)
        d_ii, d_oi = gpu.CudaVec.from_cpu_async(in_idx, st), gpu.CudaVec.from_cpu_async(out_idx, st)
        view = gpu.CudaLweCiphertextList(self.d_in.d_vec, batch, self.n_in)
        try:
            lib.hip_backend_set_keyswitch_kernel(choice)
            lib.hip_backend_set_keyswitch_kparts(kparts)
            gpu.cuda_keyswitch_lwe_ciphertext(self.d_key, view, d_out, d_ii, d_oi, False, st)
            inst = last_instantiation(lib)
        finally:
            lib.hip_backend_set_keyswitch_kernel(0)
            lib.hip_backend_set_keyswitch_kparts(KPARTS_DEFAULT)
        got = d_out.d_vec.copy_to_cpu(st).reshape(batch + 1, self.n_out + 1)
        assert (got[batch] == fill[0]).all(), "written past the last output"
        return got[:batch], inst

    def drop(self):
        self.d_key.d_vec.drop()      # takes the key's cached layout along
        self.d_in.d_vec.drop()


def scattered(ref, out_idx):
    want = np.zeros_like(ref)
    want[out_idx.astype(np.int64)] = ref
    return want


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} words differ, first at (output, column) {tuple(bad[0])}" if len(bad) else "equal"


@functools.lru_cache(maxsize=None)
def _case_inputs(case):
    """Ciphertexts, index vectors and the oracle's outputs of a row: computed once, shared by both backends."""
    rng = np.random.default_rng(case.batch * 7919 + case.n_in)
    pool = case.batch + 3
    cts = rng.integers(0, 1 << 64, size=(pool, case.n_in + 1), dtype=U64)
    in_idx, out_idx = index_vectors(rng, pool, case.batch, case.dup)
    key = uniform_key(case.n_in, case.n_out, case.level, case.bits)
    ref = oracle_keyswitch(cts[in_idx.astype(np.int64)], key, case.n_in, case.n_out, case.base_log, case.level, case.bits)
    return cts, in_idx, out_idx, scattered(ref, out_idx)


def _run_case(kind, case):
    cts, in_idx, out_idx, want = _case_inputs(case)
    key = uniform_key(case.n_in, case.n_out, case.level, case.bits)
    run = Launcher(kind, cts, key, case.n_in, case.n_out, case.base_log, case.level)
    try:
        got, inst = run.launch(in_idx, out_idx, case.choice, case.kparts)
        assert inst == case.inst, f"{case.id}: ran {inst}, the row is for {case.inst}"
        assert got.dtype == want.dtype and np.array_equal(got, want), f"{case.id}: {first_difference(got, want)}"
        if case.level <= KS_MAXL and case.choice != 1:
            sc, inst = run.launch(in_idx, out_idx, 1)
            assert inst[0] == 0 and inst[1] == scalar_rule(case.n_in, case.base_log, case.level, case.bits), inst
            assert np.array_equal(sc, want), f"{case.id}, scalar kernels: {first_difference(sc, want)}"
    finally:
        run.drop()


def _case_params():
    out = []
    for c in CASES:
        for kind in ("emu", "hip"):
            if kind == "emu" and c.gpu_only:
                continue
            out.append(pytest.param(kind, c, id=f"{kind}-{c.id}", marks=[pytest.mark.gpu] if kind == "hip" else []))
    return out


@pytest.mark.parametrize("kind,case", _case_params())
def test_form_bit_exact(kind, case):
    _run_case(kind, case)


# ---------------------------------------------------------------- the shape rule itself
# (n_in, base_log, level, key bits) -> the matrix-core paths take it; both sides of every clause of ksm_shape
SHAPE_VERDICTS = [
    ((64, 6, 1, 64), True), ((64, 7, 1, 64), False),             # base_log <= 6
    ((64, 6, 1, 32), True), ((64, 7, 1, 32), False),
    ((64, 6, 5, 32), True), ((64, 7, 4, 32), False),
    ((32, 6, 1, 64), True), ((24, 6, 1, 64), False),             # K = n_in * level_pad in steps of 32
    ((16, 5, 2, 64), True), ((17, 5, 2, 64), False),
    ((8, 4, 4, 64), True), ((33, 4, 4, 64), False), ((40, 4, 4, 32), True),
    ((8, 5, 3, 64), True), ((12, 5, 3, 64), False),              # 3 levels count as 4
    ((4, 3, 5, 64), True), ((6, 3, 5, 32), False),               # 5 as 8
    ((2, 2, 16, 64), True), ((2, 2, 9, 32), True), ((3, 2, 8, 64), False),   # 9 .. 16 as 16, the most; 8 x 3 = 24
    ((32768, 6, 8, 64), True), ((32772, 6, 8, 64), False),       # base_log + 7 + log2 K: 31 and 32
]


def test_shape_verdicts_cover_every_clause():
    for (n_in, bl, lv, bits), ok in SHAPE_VERDICTS:
        assert shape_rule(n_in, 3, bl, lv)[3] == ok, (n_in, bl, lv)
    level_pad, K_over_32, _, ok = shape_rule(32768, 3, 6, 8)
    assert 6 + 7 + (K_over_32 * 32 - 1).bit_length() == 31 and ok
    assert 6 + 7 + (shape_rule(32772, 3, 6, 8)[1] * 32 - 1).bit_length() == 32


@pytest.mark.parametrize("shape,ok", SHAPE_VERDICTS, ids=lambda v: "n%d_%dx%d_u%d" % v if isinstance(v, tuple) else None)
def test_shape_rule_decides_the_path(shape, ok):
    """A 3-LWE launch on the emulation takes the one-launch kernel exactly where ksm_shape says so, the scalar kernels
    otherwise, and computes the oracle's words either way."""
    n_in, base_log, level, bits = shape
    n_out = 3
    rng = np.random.default_rng(n_in + level)
    cts = rng.integers(0, 1 << 64, size=(4, n_in + 1), dtype=U64)
    key = uniform_key(n_in, n_out, level, bits)
    in_idx, out_idx = index_vectors(rng, 4, 3)
    run = Launcher("emu", cts, key, n_in, n_out, base_log, level)
    try:
        got, inst = run.launch(in_idx, out_idx)
    finally:
        run.drop()
    assert inst[0] == (1 if ok else 0), inst
    want = scattered(oracle_keyswitch(cts[in_idx.astype(np.int64)], key, n_in, n_out, base_log, level, bits), out_idx)
    assert np.array_equal(got, want), first_difference(got, want)


def test_seventeen_levels_are_refused_with_their_message():
    """17 levels would count as 32 per mask word: the matrix-core paths decline and the scalar kernels stage 8 at most —
    the call aborts with its message (in a process of its own)."""
    for entry, name in (("cuda_keyswitch_lwe_ciphertext_vector_64_64_async", "keyswitch"),):
        r = run_child(f"""
            v = gpu.CudaVec(4096, st)
            lib.{entry}(S, G, v.ptr, v.ptr, v.ptr, v.ptr, v.ptr, 32, 3, 2, 17, 1)
            """)
        assert r.returncode != 0
        assert f"{name}: level_count 17 > 8 is only supported by the matrix-core kernel" in r.stderr, r.stderr[-400:]


# ---------------------------------------------------------------- accumulators at their bounds
def extreme_rows(base_log, level):
    """(largest, smallest, all ones): mask words whose digits sum to the most / the least the decomposer emits, found
    among the words built from digit groups around B/2, and judged by the oracle's own decomposer.  Two neighbouring
    levels cannot both give +B/2 (nor both -B/2: the upper one's value B/2 would have to carry AND not carry into the
    level above the lower one), so the candidates alternate B/2 with B/2 - 1."""
    B, rep = 1 << base_log, base_log * level
    half = B // 2

    def word(groups, low):                      # groups[0] is the most significant level
        v = 0
        for g in groups:
            v = (v << base_log) | (g % B)
        return ((v << (64 - rep)) | (low & ((1 << (64 - rep)) - 1))) & ((1 << 64) - 1)

    cands = set()
    for a, b in ((half, half - 1), (half - 1, half), (half - 1, half - 1), (half, half), (half + 1, half), (half, half + 1),
                 (half + 1, half + 1), (half + 1, half + 2)):
        groups = [(a, b)[i % 2] for i in range(level)]
        for low in (0, (1 << 64) - 1, 1 << max(0, 63 - rep)):
            cands.add(word(groups, low))
            cands.add(word(groups[::-1], low))
    digits = {x: [int(d) for d in orc.decompose(x, base_log, level)] for x in cands}
    hi = max(cands, key=lambda x: sum(digits[x]))
    lo = min(cands, key=lambda x: sum(digits[x]))
    return hi, lo, (1 << 64) - 1


def int32_accumulators(row_digits, level_pad, key_bytes, base_log, n_in):
    """The sums v_mfma_i32_32x32x32_i8 accumulates for one ciphertext whose mask words all carry `row_digits`, against a
    key column whose words all have the byte `key_bytes[p]` in plane p: per plane, sum over K of (digit + B/2) *
    (byte - 128); the padded levels are digit 0 against the zero key rows (byte 0), in Python integers."""
    half = 1 << (base_log - 1)
    per_word = [sum((d + half) * (b - 128) for d in row_digits) + (level_pad - len(row_digits)) * half * (0 - 128)
                for b in key_bytes]
    return [n_in * s for s in per_word]


# byte patterns of the key words, most significant byte first: byte 0x00 is the matrix cores' -128 (the largest product), 0xFF
# their +127, 0x80 their 0, 0x7F their -1; mixed words put both signs into neighbouring planes of one accumulator set
KEY_PATTERNS = {"00": [0x00] * 8, "ff": [0xFF] * 8, "80": [0x80] * 8, "7f": [0x7F] * 8, "807f": [0x80, 0x7F] * 4,
                "00ff": [0x00, 0xFF] * 4}
PATTERN_PAIRS = [("00", "ff"), ("80", "7f"), ("807f", "00ff")]     # one pattern per column of an n_out = 1 key

# (n_in, base_log, level, key bits): K = n_in * level_pad = 2^18, the largest base_log 6 takes (6 + 7 + 18 = 31): 10 levels
# padded to 16, and 8 unpadded; the 32-bit key at 16 levels of 2 bits
ACC_SHAPES = {"u64_6x10_n16384": (16384, 6, 10, 64), "u64_6x8_n32768": (32768, 6, 8, 64), "u32_2x16_n16384": (16384, 2, 16, 32)}


def _pattern_word(pattern, bits):
    by = KEY_PATTERNS[pattern][:bits // 8]
    return int.from_bytes(bytes(by), "big")


@functools.lru_cache(maxsize=None)
def _acc_inputs(shape, pair, batch):
    n_in, base_log, level, bits = ACC_SHAPES[shape]
    B = 1 << base_log
    hi, lo, ones = extreme_rows(base_log, level)
    dh, dl = orc.decompose(hi, base_log, level), orc.decompose(lo, base_log, level)
    # the condition on the inputs, from the oracle's own digits: every digit of the row is one of the two largest (smallest)
    # the decomposer emits, and no level pair could hold more
    assert all(int(d) >= B // 2 - 1 for d in dh) and all(int(d) <= -(B // 2 - 1) for d in dl), (dh, dl)
    assert sum(int(d) for d in dh) == (B - 1) * (level // 2) + (B // 2) * (level % 2), dh
    assert sum(int(d) for d in dl) == -sum(int(d) for d in dh), dl
    rng = np.random.default_rng(n_in + batch)
    rows = [hi, lo, ones]
    cts = rng.integers(0, 1 << 64, size=(batch, n_in + 1), dtype=U64)
    for i in range(batch):
        if i < 3 or i % 2:
            cts[i, :n_in] = U64(rows[i % 3])
    dtype = U64 if bits == 64 else U32
    key = np.empty((n_in * level, 2), dtype=dtype)
    for col, pattern in enumerate(pair):
        key[:, col] = dtype(_pattern_word(pattern, bits))
    key = key.reshape(-1)
    ref = oracle_keyswitch(cts, key, n_in, 1, base_log, level, bits)
    return cts, key, ref, [int(d) for d in dh], [int(d) for d in dl]


def _largest_accumulator(shape, pair, dh, dl):
    n_in, base_log, level, bits = ACC_SHAPES[shape]
    level_pad = shape_rule(n_in, 1, base_log, level)[0]
    accs = []
    for pattern in pair:
        planes = KEY_PATTERNS[pattern][:bits // 8]
        for digits in (dh, dl):
            accs += int32_accumulators(digits, level_pad, planes, base_log, n_in)
    return accs


def test_accumulator_inputs_reach_the_int32_bound():
    """The condition on the inputs, on the CPU: with the rows and key bytes above, the largest |int32 accumulator| of the
    matrix instruction, in Python integers.  ksm_shape admits K up to B * 128 * K = 2^31; that product needs every shifted
    digit at B, which no ciphertext gives (neighbouring levels cannot both be +B/2, see extreme_rows), so the reachable
    maximum is 128 * (B - 1/2) * K on an unpadded decomposition: 2^31 - 2^24 at 6 x 8 — within one 128th of the bound the
    rule is written for — and less where padded levels (digit 0, shifted B/2) take the place of real ones:
    0.8076 * 2^31 at 6 x 10.  Every accumulator must fit an int32; the largest must be exactly that reachable maximum."""
    for shape, (n_in, base_log, level, bits) in ACC_SHAPES.items():
        B = 1 << base_log
        level_pad = shape_rule(n_in, 1, base_log, level)[0]
        worst = 0
        for pair in PATTERN_PAIRS:
            _, _, _, dh, dl = _acc_inputs(shape, pair, 3)
            accs = _largest_accumulator(shape, pair, dh, dl)
            assert all(-(1 << 31) <= a < (1 << 31) for a in accs), (shape, pair)
            worst = max(worst, max(abs(a) for a in accs))
        real = 128 * n_in * ((2 * B - 1) * (level // 2) + B * (level % 2))      # levels in pairs (B, B - 1); an odd one at B
        reachable = real + 128 * n_in * (level_pad - level) * (B // 2)
        term = 128 * B
        assert reachable - term <= worst <= reachable, (shape, worst, reachable)
        if shape == "u64_6x8_n32768":
            assert worst == (1 << 31) - (1 << 24)
        if bits == 64:
            assert worst >= 0.8 * (1 << 31), (shape, worst / (1 << 31))


def _acc_params():
    out = []
    for shape in ACC_SHAPES:
        for pair in PATTERN_PAIRS:
            for kind, batch in (("emu", 3), ("hip", 3), ("hip", 131)):
                out.append(pytest.param(kind, shape, pair, batch, id=f"{kind}-{shape}-{pair[0]}_{pair[1]}-{batch}",
                                        marks=[pytest.mark.gpu] if kind == "hip" else []))
    return out


@pytest.mark.parametrize("kind,shape,pair,batch", _acc_params())
def test_keyswitch_accumulators_at_their_bounds(kind, shape, pair, batch):
    """K = 2^18 at base_log 6 (base_log + 7 + log2 K = 31, the largest ksm_shape takes), key words of one repeated byte
    pattern per column and ciphertext rows whose every digit is extreme (test_accumulator_inputs_reach_the_int32_bound
    states how close to 2^31 the int32 accumulators come): 3 LWEs on the one-launch kernel; 131 through the digit pass and
    the GEMM on the MI355X only (the emulation needs half a minute per pattern for it)."""
    n_in, base_log, level, bits = ACC_SHAPES[shape]
    cts, key, ref, _, _ = _acc_inputs(shape, pair, batch)
    rng = np.random.default_rng(batch)
    in_idx, out_idx = index_vectors(rng, batch, batch)
    want = scattered(ref[in_idx.astype(np.int64)], out_idx)
    run = Launcher(kind, cts, key, n_in, 1, base_log, level)
    try:
        got, inst = run.launch(in_idx, out_idx, 3 if batch > 128 else 0)
        assert inst[0] == (2 if batch > 128 else 1) and inst[4] == bits, inst
        assert np.array_equal(got, want), first_difference(got, want)
        if level <= KS_MAXL:
            sc, inst = run.launch(in_idx, out_idx, 1)
            assert inst[0] == 0 and np.array_equal(sc, want), first_difference(sc, want)
    finally:
        run.drop()


@pytest.mark.parametrize("kind", BACKENDS)
def test_one_step_past_the_int32_bound_takes_the_scalar_kernels(kind):
    """n_in = 32772 at 6 x 8: K = 2^18 + 32, base_log + 7 + log2 K = 32 — the matrix cores must decline, and the
    small-base kernel must give the oracle's words on the same adversarial rows and key bytes."""
    n_in, base_log, level = 32772, 6, 8
    hi, lo, ones = extreme_rows(base_log, level)
    rng = np.random.default_rng(5)
    cts = rng.integers(0, 1 << 64, size=(3, n_in + 1), dtype=U64)
    for i, x in enumerate((hi, lo, ones)):
        cts[i, :n_in] = U64(x)
    key = np.empty((n_in * level, 2), dtype=U64)
    key[:, 0], key[:, 1] = U64(_pattern_word("00", 64)), U64(_pattern_word("ff", 64))
    key = key.reshape(-1)
    in_idx, out_idx = index_vectors(rng, 3, 3)
    run = Launcher(kind, cts, key, n_in, 1, base_log, level)
    try:
        got, inst = run.launch(in_idx, out_idx)
    finally:
        run.drop()
    assert inst == scalar(SMALL_BASE), inst
    want = scattered(orc.keyswitch_batch(cts[in_idx.astype(np.int64)], key, n_in, 1, base_log, level), out_idx)
    assert np.array_equal(got, want), first_difference(got, want)


@pytest.mark.parametrize("kind", BACKENDS)
def test_small_base_halves_at_their_bound(kind):
    """keyswitch_small_base_kernel accumulates (digit + B/2) * (a 32-bit half of the key word) in 64 bits without a carry
    chain; launch_keyswitch gives it the shapes with base_log + 33 + log2(n_in * level) <= 64.  At equality (n_in = 2048,
    one level of 20 bits) with every digit +B/2 — a single level can hold it — and key halves of 2^32 - 1, the sum is
    2048 * 2^20 * (2^32 - 1): within one term of 2^63, inside the 64 bits.  One bit more (21 x 1) must take the int32-digit
    kernel.  Both against the oracle, with 0xFFFFFFFF / 0x80000000 / 0x7FFFFFFF halves."""
    n_in, n_out = 2048, 1
    words = [0xFFFFFFFFFFFFFFFF, 0x800000007FFFFFFF]
    for base_log, kernel in ((20, SMALL_BASE), (21, DIGITS32)):
        assert scalar_rule(n_in, base_log, 1, 64) == kernel
        B = 1 << base_log
        hi, lo = (B // 2) << (64 - base_log), ((B // 2 - 1) << (64 - base_log)) | (1 << (63 - base_log))
        assert int(orc.decompose(hi, base_log, 1)[0]) == B // 2 and int(orc.decompose(lo, base_log, 1)[0]) == -(B // 2)
        if kernel == SMALL_BASE:
            acc = n_in * B * 0xFFFFFFFF           # every shifted digit at B against a half of 2^32 - 1
            assert (1 << 63) - B * 0xFFFFFFFF <= acc < (1 << 64)
            assert base_log + 33 + (n_in - 1).bit_length() == 64
        rng = np.random.default_rng(base_log)
        cts = rng.integers(0, 1 << 64, size=(3, n_in + 1), dtype=U64)
        for i, x in enumerate((hi, lo, (1 << 64) - 1)):
            cts[i, :n_in] = U64(x)
        key = np.empty((n_in, 2), dtype=U64)
        key[:, 0], key[:, 1] = U64(words[0]), U64(words[1])
        key = key.reshape(-1)
        in_idx, out_idx = index_vectors(rng, 3, 3)
        run = Launcher(kind, cts, key, n_in, n_out, base_log, 1)
        try:
            got, inst = run.launch(in_idx, out_idx)
        finally:
            run.drop()
        assert inst == scalar(kernel), inst
        want = scattered(orc.keyswitch_batch(cts[in_idx.astype(np.int64)], key, n_in, n_out, base_log, 1), out_idx)
        assert np.array_equal(got, want), (base_log, first_difference(got, want))


# ---------------------------------------------------------------- key-layout cache
@pytest.mark.parametrize("kind", BACKENDS)
def test_keyswitch_layout_cache_evicts_least_recently_used(kind):
    """40 tiny keys (n_in = 32, n_out = 3, 6 x 1) in rotation, twice, against a cache of 32 layouts: every call takes the
    one-launch kernel and gives the oracle's words, the cache never holds more than 32 and nothing once the keys are
    dropped.  Then the order: 32 keys cached, the oldest used again, a 33rd key added — the second oldest must be the one
    that went (dropping it leaves the 32 entries alone; dropping the oldest takes its entry along)."""
    lib, st = _backend(kind)
    n_in, n_out, base_log, level, count = 32, 3, 6, 1, 40
    rng = np.random.default_rng(40)
    cts = rng.integers(0, 1 << 64, size=(3, n_in + 1), dtype=U64)
    keys = [rng.integers(0, 1 << 64, size=n_in * level * (n_out + 1), dtype=U64) for _ in range(count)]
    refs = [orc.keyswitch_batch(cts, k, n_in, n_out, base_log, level) for k in keys]
    d_in = gpu.CudaLweCiphertextList.from_lwe_ciphertext_list(cts, st)
    idx = gpu.CudaVec.from_cpu_async(np.arange(3, dtype=U64), st)
    d_keys = [gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(k, n_in, n_out, base_log, level, st) for k in keys]

    def call(i):
        d_out = gpu.CudaLweCiphertextList.new(n_out, 3, st)
        gpu.cuda_keyswitch_lwe_ciphertext(d_keys[i], d_in, d_out, idx, idx, True, st)
        assert last_instantiation(lib) == one(1, False, 64, 1, 1, 1), i
        assert np.array_equal(d_out.to_lwe_ciphertext_list(st), refs[i]), i
        assert lib.hip_backend_keyswitch_cache_entries() <= 32

    try:
        for _ in range(2):
            for i in range(count):
                call(i)
        assert lib.hip_backend_keyswitch_cache_entries() == 32     # the last 32 of the rotation, nobody else's
        for k in d_keys:
            k.d_vec.drop()
        assert lib.hip_backend_keyswitch_cache_entries() == 0
        # the order of eviction
        d_keys = [gpu.CudaLweKeyswitchKey.from_lwe_keyswitch_key(k, n_in, n_out, base_log, level, st) for k in keys[:33]]
        for i in range(32):
            call(i)
        call(0)                      # key 0 is the most recently used now, key 1 the least
        call(32)
        assert lib.hip_backend_keyswitch_cache_entries() == 32
        d_keys[1].d_vec.drop()       # evicted already: no entry goes with it
        assert lib.hip_backend_keyswitch_cache_entries() == 32
        d_keys[0].d_vec.drop()       # still cached
        assert lib.hip_backend_keyswitch_cache_entries() == 31
    finally:
        for k in d_keys:
            k.d_vec.drop()
    assert lib.hip_backend_keyswitch_cache_entries() == 0


# ---------------------------------------------------------------- production shapes (MI355X only)
# (n_in, n_out, (base_log, level), key bits): PARAM_MESSAGE_2_CARRY_2, the GPU multi-bit sets of group 3 and 4, the multi-bit
# set of group 3, PARAM_MESSAGE_1_CARRY_2 on N = 1024, and the first one with a 32-bit key
PRODUCTION = {
    "2048_918_4x4": (2048, 918, (4, 4), 64), "2048_879_2x8": (2048, 879, (2, 8), 64), "2048_920_3x5": (2048, 920, (3, 5), 64),
    "2048_918_3x6": (2048, 918, (3, 6), 64), "2048_885_3x5": (2048, 885, (3, 5), 64), "2048_918_4x4_ks32": (2048, 918, (4, 4), 32),
}


@functools.lru_cache(maxsize=1)
def _production_inputs(name, count):
    n_in, n_out, (base_log, level), bits = PRODUCTION[name]
    rng = np.random.default_rng(n_out + level)
    cts = rng.integers(0, 1 << 64, size=(count, n_in + 1), dtype=U64)
    return cts, uniform_key(n_in, n_out, level, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PRODUCTION))
def test_production_shapes_against_the_oracle(name):
    """33, 257, 769 and 1000 LWEs (one-launch kernel over z, over workgroup rows; the automatic GEMM) at full size, uniform
    random keys, every output row against the oracle (computed once for the 1000 ciphertexts)."""
    n_in, n_out, (base_log, level), bits = PRODUCTION[name]
    cts, key = _production_inputs(name, 1000)
    ref = oracle_keyswitch(cts, key, n_in, n_out, base_log, level, bits)
    level_pad, steps, col_tiles, ok = shape_rule(n_in, n_out, base_log, level)
    assert ok and col_tiles == 28 + (n_out >= 896)
    run = Launcher("hip", cts, key, n_in, n_out, base_log, level)
    try:
        for batch in (33, 257, 769, 1000):
            rng = np.random.default_rng(batch)
            in_idx, out_idx = index_vectors(rng, 1000, batch)
            got, inst = run.launch(in_idx, out_idx)
            row = Case(name, n_in, n_out, base_log, level, bits, batch, 0, ())
            assert inst == expected_instantiation(row), (batch, inst)
            assert inst[0] == (2 if batch >= GEMM_AUTO else 1)
            want = scattered(ref[in_idx.astype(np.int64)], out_idx)
            assert np.array_equal(got, want), f"{name}, {batch} LWEs: {first_difference(got, want)}"
    finally:
        run.drop()


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", [("2048_918_4x4", gemm(4, False, 64, 2, 29)), ("2048_918_4x4_ks32", gemm(4, False, 32, 4, 29))])
def test_benchmark_batch_of_4096(name, form):
    """The headline benchmark's keyswitch: 4096 LWEs, 2048 -> 918, 4 x 4, 29 column tiles on ks_gemm_kernel<u64,2>
    (<u32,4> with the 32-bit key).  All rows of the automatic path against the scalar kernels and against the one-launch
    kernel, word for word; a seeded 64 of them against the oracle (rows are independent: a full check of those rows)."""
    n_in, n_out, (base_log, level), bits = PRODUCTION[name]
    count = 4096
    cts, key = _production_inputs(name, count)
    rng = np.random.default_rng(4096)
    in_idx, out_idx = index_vectors(rng, count, count)
    run = Launcher("hip", cts, key, n_in, n_out, base_log, level)
    try:
        got, inst = run.launch(in_idx, out_idx)
        assert inst == form, inst
        sc, inst = run.launch(in_idx, out_idx, 1)
        assert inst == scalar(scalar_rule(n_in, base_log, level, bits), bits), inst
        ol, inst = run.launch(in_idx, out_idx, 2)
        assert inst == one(4, False, bits, 1, 1, 29), inst
    finally:
        run.drop()
    assert np.array_equal(got, sc), f"GEMM against the scalar kernels: {first_difference(got, sc)}"
    assert np.array_equal(got, ol), f"GEMM against the one-launch kernel: {first_difference(got, ol)}"
    slots = np.sort(rng.permutation(count)[:64])
    ref = oracle_keyswitch(cts[in_idx[slots].astype(np.int64)], key, n_in, n_out, base_log, level, bits)
    assert np.array_equal(got[out_idx[slots].astype(np.int64)], ref)
