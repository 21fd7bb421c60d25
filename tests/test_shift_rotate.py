"""Shifts and rotations of the radix layer: by an encrypted amount (a barrel shifter over the bits), the arithmetic right
shift and the rotation by a clear amount, and the fused rotate-and-pack kernel under them.

The checker is clear Python integer arithmetic on the decrypted blocks.  A clear model of the rounds (ClearBarrel below)
tells which inputs every mux table and every cleanup table was asked; nothing of it reads the library's tables.
[emu] runs the kernel sources on the host, [hip] on the MI355X; toy keys, the anchor row on the MI355X with
PARAM_MESSAGE_2_CARRY_2."""
import ctypes as C
import dataclasses
import gc
import signal
import textwrap

import numpy as np
import pytest

from . import radix_model as rm
from .common import C1, Params, make_keys
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_bases import BASES, Ctx

U64 = np.uint64
BASE = {b.name: b for b in BASES}
OPS = ["shl", "shr", "sar", "rotl", "rotr"]      # sar: the arithmetic right shift


# ================================================================================== 1. the kernel alone
def rotate_pack_model(x, pad, ctrl, s0, s1, r, direction, mode, pad_row, ctrl_row):
    """x: [batch][rows][words] u64; the kernel's formula in NumPy (u64 arithmetic wraps modulo 2^64)"""
    batch, rows, _ = x.shape
    out = np.empty_like(x)
    for c in range(batch):
        for i in range(rows):
            j = i - r if direction == 0 else i + r
            if 0 <= j < rows:
                pick = x[c, j]
            elif mode == 0:
                pick = x[c, j % rows]
            elif mode == 1:
                pick = np.zeros_like(x[c, 0])
            else:
                pick = pad[c, pad_row]
            out[c, i] = U64(s0) * x[c, i] + U64(s1) * pick + (ctrl[c, ctrl_row] if ctrl is not None else U64(0))
    return out


ROWS = (1, 2, 6, 8, 64)
WORDS = (1, 5, 511, 512, 513, 2049)      # the edges of a 512-word slice, the odd production row
SENTINEL = U64(0xA5A5A5A55A5A5A5A)


def kernel_cases():
    out = []
    for kind in ("emu", "hip"):
        for words in WORDS:
            for rows in ROWS:
                for batch in (1, 3):
                    marks = [pytest.mark.gpu] if kind == "hip" else []
                    out.append(pytest.param(kind, words, rows, batch, marks=marks,
                                            id=f"{kind}-{words}_words-{rows}_rows-batch_{batch}"))
    return out


@pytest.mark.parametrize("kind,words,rows,batch", kernel_cases())
def test_rotate_pack_kernel_equals_numpy_word_for_word(kind, words, rows, batch):
    """hip_test_rotate_pack_async against the formula, on random u64 words: every distance in {1, R / 2, R - 1} that is
    valid, both directions, the three padding modes (the padding row is row 2 of 3 of its buffer), with and without a
    control row (row 1 of 2), the three scale pairs.  `out` sits between sentinel rows that must stay as they are."""
    from tfhe_rs_amd import core_crypto_gpu as gpu
    lib = use_backend(kind)
    st = gpu.CudaStreams((0,))
    rng = np.random.default_rng(1000 * words + 10 * rows + batch)
    draw = lambda *shape: rng.integers(0, 2 ** 64, size=shape, dtype=U64)
    x, pad, ctrl = draw(batch, rows, words), draw(batch, 3, words), draw(batch, 2, words)
    d_x, d_pad, d_ctrl = (gpu.CudaVec.from_cpu_async(a.reshape(-1), st) for a in (x, pad, ctrl))
    guard = 2 * words
    frame = np.full(guard + x.size + guard, SENTINEL, dtype=U64)
    d_out = gpu.CudaVec.from_cpu_async(frame, st)
    out_ptr = d_out.ptr + 8 * guard
    distances = sorted({r for r in (1, rows // 2, rows - 1) if 0 <= r < rows} or {0})
    if rows == 1:
        distances = [0]
    runs = 0
    for r in distances:
        for direction in (0, 1):
            for mode in (0, 1, 2):
                for with_ctrl in (False, True):
                    for s0, s1 in ((1, 2), (4, 1), (2, 1)):
                        d_out.copy_from_cpu_async(frame, st)
                        lib.hip_test_rotate_pack_async(st.ptr[0], 0, out_ptr, d_x.ptr, d_pad.ptr,
                                                       d_ctrl.ptr if with_ctrl else None, s0, s1, words, rows, batch, r,
                                                       direction, mode, 3, 2, 2, 1)
                        got = d_out.copy_to_cpu(st)
                        want = rotate_pack_model(x, pad, ctrl if with_ctrl else None, s0, s1, r, direction, mode, 2, 1)
                        what = (r, direction, mode, with_ctrl, s0, s1)
                        assert np.array_equal(got[guard:-guard].reshape(x.shape), want), what
                        assert (got[:guard] == SENTINEL).all() and (got[-guard:] == SENTINEL).all(), what
                        runs += 1
    assert runs == len(distances) * 36


# ================================================================================== the clear model of the rounds
class ClearBarrel:
    """The rounds of a shift / rotation by an encrypted amount on clear bits: which inputs (4 c + 2 p + a) every stage's
    mux table sees, which condition the cleanup table sees, and the value that comes out."""

    def __init__(self, bits_per_block, blocks):
        self.b, self.L, self.B = bits_per_block, blocks, bits_per_block * blocks
        self.m = (self.B - 1).bit_length()

    def run(self, op, value, amount):
        B, m = self.B, self.m
        cur = [(value >> i) & 1 for i in range(B)]
        sign = cur[B - 1]
        mux, left = set(), op in ("shl", "rotl")
        for d in range(m):
            c, r, nxt = (amount >> d) & 1, 1 << d, []
            for i in range(B):
                j = i - r if left else i + r
                if 0 <= j < B:
                    p = cur[j]
                elif op in ("rotl", "rotr"):
                    p = cur[j % B]
                else:
                    p = sign if op == "sar" else 0
                mux.add((d, 4 * c + 2 * p + cur[i]))
                nxt.append(p if c else cur[i])
            cur = nxt
        out = sum(bit << i for i, bit in enumerate(cur))
        cond = None
        if op in ("shl", "shr", "sar"):
            over = int(amount >= B)
            cond = 2 * over + sign if op == "sar" else over
            if op == "sar":
                out = (1 << B) - 1 if cond == 3 else 0 if cond == 2 else out
            elif cond:
                out = 0
        return out, mux, cond


def expected(op, value, amount, B, m):
    mask = (1 << B) - 1
    if op == "shl":
        return (value << amount) & mask if amount < B else 0
    if op == "shr":
        return value >> amount if amount < B else 0
    if op == "sar":
        signed = value - (1 << B) if value >> (B - 1) else value
        return (signed >> min(amount, B)) & mask
    r = (amount % (1 << m)) % B       # what the m control bits capture
    if op == "rotr":
        r = (B - r) % B
    return ((value << r) | (value >> (B - r))) & mask if r else value


def census(model, op, values, amounts):
    mux, conds = set(), set()
    for v in values:
        for a in amounts:
            out, seen, cond = model.run(op, v, a)
            assert out == expected(op, v, a, model.B, model.m), (op, v, a)     # the model itself against plain arithmetic
            mux |= seen
            conds.add(cond)
    return mux, conds


def census_complete(model, op, values, amounts):
    mux, conds = census(model, op, values, amounts)
    want = {None} if op in ("rotl", "rotr") else {0, 1, 2, 3} if op == "sar" else {0, 1}
    return mux == {(d, x) for d in range(model.m) for x in range(8)} and conds == want


def choose_values(model, amounts, seed):
    """(value with the top bit set, value with it clear) whose calls reach every mux input of every stage and every
    condition: searched in a fixed order, narrow integers exhaustively, wide ones among seeded patterns"""
    B = model.B
    if B <= 10:
        highs = [v for v in range(1 << B) if v >> (B - 1)]
        lows = [v for v in range(1 << B) if not v >> (B - 1)]
    else:
        rng = np.random.default_rng(seed)
        draws = [int.from_bytes(rng.bytes((B + 7) // 8), "little") & ((1 << B) - 1) for _ in range(32)]
        alt = sum(1 << i for i in range(1, B, 2))
        highs = [alt] + [v | (1 << (B - 1)) for v in draws]
        lows = [alt >> 1] + [v & ((1 << (B - 1)) - 1) for v in draws]
    for hi in reversed(highs):
        for lo in lows[1:] if B <= 10 else lows:
            if all(census_complete(model, op, [hi, lo], amounts) for op in OPS):
                return hi, lo
    raise AssertionError("no pair of values reaches every table input")


@dataclasses.dataclass(frozen=True)
class Shape:
    base: str
    L: int

    @property
    def id(self):
        return f"{self.base}-{self.L}_blocks"


SHAPES = [Shape("classic_4_4", 4),        # B = 8: a power of two
          Shape("classic_4_4", 3),        # B = 6: no power of two, an odd block count (the padded comparison), m = 3
          Shape("classic_8_8", 2),        # b = 3: two reassembly rounds
          Shape("classic_2_8", 4),        # b = 1: no reassembly loop, the cleanup a round of its own
          Shape("multibit_g3_4_4", 4)]    # multi-bit keys


# the emulation runs a fibre per lane: its shape cases take the smallest polynomial that holds the plaintext space
EMU_SMALL = {
    "classic_4_4": Params("toy_k1_N512_l1_p16", 8, 1, 512, 23, 1, 4, 4, 45, 17, 16, ms_type=1),
    "classic_2_8": Params("toy_k1_N512_l1_p16", 8, 1, 512, 23, 1, 4, 4, 45, 17, 16, ms_type=1),
    "classic_8_8": Params("toy_k1_N1024_l1_p64", 8, 1, 1024, 23, 1, 4, 4, 45, 17, 64, ms_type=1),
    "multibit_g3_4_4": Params("toy_multibit_g3_N512_p16", 9, 1, 512, 15, 2, 3, 6, 45, 17, 16, grouping=3),
}


def shape_ctx(kind, shape):
    base = BASE[shape.base]
    hip = base.emu if base.hip is C1 else base.hip       # toy keys on both backends
    return Ctx(kind, dataclasses.replace(base, hip=hip, emu=EMU_SMALL[shape.base]))


def shape_cases():
    return [pytest.param(kind, sh, id=f"{kind}-{sh.id}", marks=[pytest.mark.gpu] if kind == "hip" else [])
            for kind in ("emu", "hip") for sh in SHAPES]


def small_amounts(B, msg, L):
    return list(range(B)) + [B, B + 1, msg ** L - 1]


def call(c, op, ct, amount_ct, count=False):
    if op in ("rotl", "rotr"):
        return c.sks.rotate_assign(ct, amount_ct, c.st, left=op == "rotl", return_pbs_count=count)
    return c.sks.shift_assign(ct, amount_ct, c.st, left=op == "shl", arithmetic=op == "sar", return_pbs_count=count)


def check_encrypted_amounts(c, L, values, amounts, seed):
    m, b = c.msg, c.base.bits
    model = ClearBarrel(b, L)
    for op in OPS:
        # the second value where the operation reads the sign, or where the first alone leaves a table input unvisited
        used = values[:1] if op != "sar" and census_complete(model, op, values[:1], amounts) else values
        assert census_complete(model, op, used, amounts), op
        for n, v in enumerate(used):
            ct = c.enc([rm.digits(v, L, m)] * len(amounts), seed + n)
            am = c.enc([rm.digits(a, L, m) for a in amounts], seed + 10 + n)
            before = c.words(am)
            call(c, op, ct, am)
            rows = c.dec(ct)
            assert all(0 <= d < m for row in rows for d in row), op
            got = [rm.value(row, m) for row in rows]
            assert got == [expected(op, v, a, model.B, model.m) for a in amounts], (op, v)
            assert list(ct.degrees) == [m - 1] * (L * len(amounts)) and list(ct._info[1]) == [1] * (L * len(amounts)), op
            assert np.array_equal(c.words(am), before) and list(am.degrees) == [m - 1] * (L * len(amounts)), "the amount was touched"


# ================================================================================== 2. encrypted amounts
@pytest.mark.parametrize("kind,shape", shape_cases())
def test_every_amount_in_one_call(kind, shape):
    """LEFT / RIGHT shift, arithmetic RIGHT shift, LEFT / RIGHT rotation: one batched call per value carries the value under
    the amounts 0 .. B - 1, B, B + 1 and msg^L - 1.  The two values (sign bit set / clear) are chosen so that, by the clear
    model, every stage's mux table meets its 8 inputs and the cleanup table every condition it distinguishes."""
    c, L = shape_ctx(kind, shape), shape.L
    base = c.base
    B = base.bits * L
    amounts = small_amounts(B, base.msg, L)
    assert len(amounts) == B + 3
    values = choose_values(ClearBarrel(base.bits, L), amounts, 0)
    assert values[0] >> (B - 1) == 1 and values[1] >> (B - 1) == 0
    check_encrypted_amounts(c, L, values, amounts, 500)


@pytest.mark.gpu
def test_every_operation_on_the_anchor_row():
    """PARAM_MESSAGE_2_CARRY_2, 32 blocks: the amounts 0, 1, 31, 32, 63, 64, 65 and 2^64 - 1."""
    c, L = Ctx("hip", BASE["classic_4_4"]), 32
    assert c.p is C1
    amounts = [0, 1, 31, 32, 63, 64, 65, 2 ** 64 - 1]
    values = choose_values(ClearBarrel(2, L), amounts, 7)
    check_encrypted_amounts(c, L, values, amounts, 520)


# ================================================================================== 3. scalar forms
SCALAR_SHAPES = [Shape("classic_4_4", 4), Shape("classic_8_8", 3), Shape("classic_2_8", 4)]


@pytest.mark.parametrize("kind,shape", [pytest.param(k, sh, id=f"{k}-{sh.id}", marks=[pytest.mark.gpu] if k == "hip" else [])
                                        for k in ("emu", "hip") for sh in SCALAR_SHAPES])
def test_scalar_arithmetic_shift_and_rotations_by_every_amount(kind, shape):
    """The arithmetic right shift and both rotations by a clear amount 0 .. B + 1 and 2 B + 1, on a negative and a
    non-negative value; an amount of 0 (and a rotation by B) launches nothing and leaves words, degrees and noise levels."""
    base = BASE[shape.base]
    base = dataclasses.replace(base, hip=base.emu if base.hip is C1 else base.hip)
    c, L, m = Ctx(kind, base), shape.L, base.msg
    B = base.bits * L
    mask = (1 << B) - 1
    rng = np.random.default_rng(540 + B)
    negative = int(rng.integers(0, 1 << B)) | (1 << (B - 1)) | 1
    positive = (int(rng.integers(0, 1 << B)) & (mask >> 1)) | (1 << (B - 2))
    for n, v in enumerate((negative, positive)):
        fresh = rm.encrypt_rows(c.p, c.keys, [rm.digits(v, L, m)], 541 + n)
        signed = v - (1 << B) if v >> (B - 1) else v
        for amount in list(range(B + 2)) + [2 * B + 1]:
            for op in ("sar", "rotl", "rotr"):
                ct = c.from_words(fresh)
                ct.degrees[:] = rm.digits(v, L, m)                  # the tightest true degrees: a move must carry them along
                ct._info[1][:] = np.arange(L) % 2                   # and recognisable noise levels
                info = [a.copy() for a in ct._info]
                if op == "sar":
                    c.sks.scalar_shift_assign(ct, amount, c.st, left=False, arithmetic=True)
                    want, nothing = (signed >> min(amount, B)) & mask, amount == 0
                else:
                    c.sks.scalar_rotate_assign(ct, amount, c.st, left=op == "rotl")
                    r = amount % B if op == "rotl" else (B - amount % B) % B
                    want, nothing = ((v << r) | (v >> (B - r))) & mask if r else v, amount % B == 0
                rows = c.dec(ct)
                assert all(0 <= d < m for d in rows[0]), (op, amount)
                assert rm.value(rows[0], m) == want, (op, v, amount)
                assert all(int(d) >= int(x) for d, x in zip(ct.degrees, rows[0])), (op, amount, "a degree below its block")
                if nothing:
                    assert np.array_equal(c.words(ct), fresh), (op, amount, "no bootstrap may run")
                    assert all(np.array_equal(a, b) for a, b in zip(ct._info, info)), (op, amount)
    with pytest.raises(ValueError):
        c.sks.scalar_shift_assign(c.from_words(fresh), 1, c.st, left=True, arithmetic=True)


@pytest.mark.parametrize("kind", ["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_logical_scalar_shift_keeps_its_path(kind):
    """scalar_shift_assign(..., arithmetic=False) is the call it was: the same words as the entry point it wraps."""
    base = dataclasses.replace(BASE["classic_4_4"], hip=BASE["classic_4_4"].emu)
    c, L = Ctx(kind, base), 4
    fresh = rm.encrypt_rows(c.p, c.keys, [[3, 1, 2, 3]], 560)
    lib = use_backend(kind)
    for left in (True, False):
        a, b = c.from_words(fresh), c.from_words(fresh)
        c.sks.scalar_shift_assign(a, 3, c.st, left=left, arithmetic=False)
        s, keep = c.sks._streams(c.st)
        ksks, bsks = c.sks._key_ptrs(c.st)
        mem = C.c_void_p()
        lib.scratch_cuda_logical_scalar_shift_64_inplace_async(s, C.byref(mem), c.sks._bsk_params(), c.sks._ksk_params(), L,
                                                               4, 4, 0 if left else 1, True, c.sks._noise_reduction())
        lib.cuda_logical_scalar_shift_64_inplace_async(s, C.byref(b._ffi()), 3, mem, bsks, ksks)
        lib.cleanup_cuda_logical_scalar_shift_64_inplace(s, C.byref(mem))
        assert np.array_equal(c.words(a), c.words(b)) and list(a.degrees) == list(b.degrees)
        want = (rm.value([3, 1, 2, 3], 4) << 3) & 255 if left else rm.value([3, 1, 2, 3], 4) >> 3
        assert rm.value(c.dec(a)[0], 4) == want


# ================================================================================== 4. bootstrap count
def propagate_pbs(L):
    """bootstraps of the carry look-ahead on L blocks (the comment that opens the carry propagation in integer.hip)"""
    if L == 1:
        return 1
    n = [L]
    while n[-1] > 4:
        n.append((n[-1] + 2) // 3)
    top = len(n) - 1
    count = 2 * L + sum(n[l] - 1 for l in range(1, top + 1)) + (L // 3 if top >= 1 else 0) + n[top] - 1
    return count + sum(n[l] - (n[l] + 2) // 3 for l in range(1, top))


def comparison_pbs(L, msg):
    """"amount >= B": the flag of the look-ahead without its result round, on the digits the comparison sees (bit blocks
    paired at msg = 2, an even count from two digits on)"""
    digits = (L + 1) // 2 if msg == 2 else L
    digits += digits % 2 if digits > 1 else 0
    return 1 if digits == 1 else propagate_pbs(digits) - digits + 1


@pytest.mark.parametrize("kind,shape", shape_cases())
def test_bootstrap_count(kind, shape):
    """B + m + m B + (shifts: comparison + 1) + (b > 1: (b - 1) L; b = 1: L for a shift, nothing for a rotation).  The
    library also checks the count against the rounds it issued in every call."""
    c, L = shape_ctx(kind, shape), shape.L
    b, m = c.base.bits, c.base.msg
    B = b * L
    ctrl = (B - 1).bit_length()
    counts = {}
    for op in OPS:
        ct, am = c.enc([rm.digits(5, L, m)], 570), c.enc([rm.digits(1, L, m)], 571)
        counts[op] = call(c, op, ct, am, count=True)
        shift = op in ("shl", "shr", "sar")
        want = B + ctrl + ctrl * B + (comparison_pbs(L, m) + 1 if shift else 0) + ((b - 1) * L if b > 1 else L if shift else 0)
        assert counts[op] == want, op
    assert counts["rotl"] < counts["shl"] and counts["rotr"] < counts["shr"] and counts["shr"] == counts["sar"]


# ================================================================================== 5. sharding
@pytest.mark.parametrize("kind", ["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_rounds_sharded_over_the_streams_of_the_set(kind):
    """One stream against three streams on the same GPU at a threshold of 3 blocks per GPU: an encrypted left shift and an
    arithmetic scalar shift are bit for bit the same."""
    from .test_radix_integer import setup
    base = BASE["classic_4_4"]
    p, keys, st1, sks1, igpu = setup(kind, base.emu)
    _, _, st3, sks3, _ = setup(kind, base.emu, gpu_indexes=(0, 0, 0))
    lib = use_backend(kind)
    L, m = 4, 4
    v, a = 0b10110110, 3
    wv, wa = rm.encrypt_rows(p, keys, [rm.digits(v, L, m)], 580), rm.encrypt_rows(p, keys, [rm.digits(a, L, m)], 581)
    outs = {}
    for name, st, sks, thr in (("one", st1, sks1, 512), ("three", st3, sks3, 3)):
        lib.hip_integer_set_multi_gpu_threshold(thr)
        try:
            mk = lambda w: igpu.CudaUnsignedRadixCiphertext.from_blocks(w, st)
            x, am, y = mk(wv), mk(wa), mk(wv)
            for ct in (x, am, y):
                ct.set_degrees(m - 1)
            sks.shift_assign(x, am, st, left=True)
            sks.scalar_shift_assign(y, 3, st, left=False, arithmetic=True)
            outs[name] = [x.to_blocks(st), y.to_blocks(st)]
        finally:
            lib.hip_integer_set_multi_gpu_threshold(0)
    for one, three in zip(outs["one"], outs["three"]):
        assert np.array_equal(one, three)
    x, y = outs["three"]
    assert rm.value(rm.decrypt_many(p, keys, x)[0].tolist(), m) == (v << a) & 255
    assert rm.value(rm.decrypt_many(p, keys, y)[0].tolist(), m) == ((v - 256) >> 3) & 255


# ================================================================================== 6. device = emulation
def seven_operations(c, words, amount_words):
    out = []
    for op in OPS:
        ct, am = c.from_words(words), c.from_words(amount_words)
        call(c, op, ct, am)
        out.append((op, c.words(ct), list(ct.degrees)))
    ct = c.from_words(words)
    c.sks.scalar_shift_assign(ct, 3, c.st, left=False, arithmetic=True)
    out.append(("scalar sar", c.words(ct), list(ct.degrees)))
    for left in (True, False):
        ct = c.from_words(words)
        c.sks.scalar_rotate_assign(ct, 5, c.st, left=left)
        out.append(("scalar rotl" if left else "scalar rotr", c.words(ct), list(ct.degrees)))
    return out


@pytest.mark.gpu
def test_device_equals_emulation_word_for_word():
    """The same keys and inputs through both backends, one call of each operation at (4, 4), four blocks."""
    base = BASE["classic_4_4"]
    toy = dataclasses.replace(base, hip=base.emu)
    p, keys = toy.emu, make_keys(toy.emu)
    words = rm.encrypt_rows(p, keys, [rm.digits(0b10011101, 4, 4)], 590)
    amount = rm.encrypt_rows(p, keys, [rm.digits(3, 4, 4)], 591)
    try:
        got = seven_operations(Ctx("hip", toy), words, amount)
        gc.collect()
        want = seven_operations(Ctx("emu", toy), words, amount)
    finally:
        use_backend("hip")
    assert [n for n, _, _ in got] == [n for n, _, _ in want] and len(got) == 8
    for (name, w_hip, d_hip), (_, w_emu, d_emu) in zip(got, want):
        assert np.array_equal(w_hip, w_emu), f"{name}: the device's words differ from the emulation's"
        assert d_hip == d_emu, name


# ================================================================================== 7. refusals
PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
N, n = 256, 4
BK = ffi.CudaLweBootstrapKeyParamsFFI(n, 1, N, 8, 2, N, 1, 0)
KK = ffi.CudaLweKeyswitchKeyParamsFFI(N, n, 4, 3)
keys = (C.c_void_p * 1)(gpu.CudaVec(16, st).ptr)
alive = []
def radix(blocks, degree=3):
    ct = igpu.CudaUnsignedRadixCiphertext(gpu.CudaVec(blocks * (N + 1), st), 1, blocks, N)
    ct.set_degrees(degree)
    alive.extend([ct, ct._ffi()])
    return C.byref(alive[-1])
def scratch(blocks, shift_type, signed=False, msg=4, carry=4):
    mem = C.c_void_p()
    lib.hip_scratch_integer_shift_and_rotate_64_inplace_async(s, C.byref(mem), BK, KK, blocks, msg, carry, shift_type, signed, True, 0)
    return mem
"""

REFUSALS = {
    "fewer than 8 values per block": ("""
        scratch(3, 0, msg=2, carry=2)
        """, "shift_and_rotate: message_modulus * carry_modulus >= 8 is required (got 4)"),
    "an amount with another block count": ("""
        lib.hip_integer_shift_and_rotate_64_inplace_async(s, radix(3), radix(2), scratch(3, 2), keys, keys)
        """, "shift_and_rotate: the amount holds 2 blocks, the value 3: they must be the same"),
    "a dirty operand": ("""
        lib.hip_integer_shift_and_rotate_64_inplace_async(s, radix(3), radix(3, 5), scratch(3, 2), keys, keys)
        """, "shift_and_rotate: block 0 has degree 5, the value and the amount must be clean"),
    "an arithmetic left shift by a clear amount": ("""
        lib.hip_scratch_integer_arithmetic_scalar_shift_64_inplace_async(s, C.byref(C.c_void_p()), BK, KK, 3, 4, 4, 0, True, 0)
        """, "arithmetic_scalar_shift: shift type 0 is not a right shift"),
    "more integers than the scratch holds": ("""
        lib.hip_integer_shift_and_rotate_64_inplace_async(s, radix(6), radix(6), scratch(3, 3), keys, keys)
        """, "shift_and_rotate: 2 integers exceed the scratch capacity 1"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_misuse_is_refused_with_a_message(name):
    """On the host emulation only, in a child process: the library aborts with a message that names the entry point."""
    snippet, message = REFUSALS[name]
    r = run_child(PRELUDE + textwrap.dedent(snippet))
    assert r.returncode == -signal.SIGABRT, f"{name}: returned {r.returncode}\n{r.stderr[-600:]}"
    assert message in r.stderr, r.stderr[-600:]
