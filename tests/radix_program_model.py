"""Chained programs on the radix layer for tests/test_radix_op_sequence.py: pools of samples whose ciphertexts are the
OUTPUTS of earlier operations, a seeded schedule in which every operation occurs, an executor table (call through
tfhe_rs_amd.integer_gpu, clear function on `int`, what the call needs of its operands), the wrapper that works as the
reference's default operations do (read the degrees, propagate only where an operation needs it), and the checks made
after every step.

The clear model is plain Python on `int`; nothing here reads the library's tables or plans.  The degree and noise rules
the wrapper decides with (an addition adds both, a clear block adds to the degree, a small clear factor multiplies both,
the negation's borrowed correcting term) are restated from the reference's host code, and what the library writes back is
compared with them.  A Runner without a context (`c=None`) makes the same draws and keeps the clear values and predicted
degrees only: that is how the committed seeds were searched (tests/test_radix_op_sequence.py, `search_seeds`).

The clear value of a ciphertext of L blocks at message modulus m is sum(block_i m^i) mod m^L, carries or not; signed
operations read the same blocks as two's complement."""
import dataclasses

import numpy as np

POOL = 4                      # samples per pool: after a few steps nearly every operand is a produced one
EDGE_PROBABILITY = 0.25       # of a drawn value being one of 0, 1, 2^bits - 1, 2^(bits - 1), bits


# ------------------------------------------------------------------------------------------ clear arithmetic
def signed(v, bits):
    return v - (1 << bits) if v >> (bits - 1) else v


def rotl(a, n, bits):
    n %= bits
    return ((a << n) | (a >> (bits - n))) & ((1 << bits) - 1) if n else a


def rotr(a, n, bits):
    return rotl(a, (bits - n % bits) % bits, bits)


def control_bits(bits):
    return (bits - 1).bit_length()


def encrypted_rotation(amount, bits):
    """a rotation by an encrypted amount reads m = ceil(log2 bits) control bits: (amount mod 2^m) mod bits"""
    return (amount % (1 << control_bits(bits))) % bits


def clear_div_rem(n, d, bits):
    mask = (1 << bits) - 1
    return (mask, n) if d == 0 else (n // d, n % d)


def clear_signed_div_rem(n, d, bits):
    """truncation towards zero, the remainder takes the numerator's sign, MIN / -1 wraps to MIN; x / 0 is 1 for x < 0,
    else -1, with remainder x"""
    mask = (1 << bits) - 1
    a, b = signed(n, bits), signed(d, bits)
    if b == 0:
        return (1 if a < 0 else mask), n
    q = abs(a) // abs(b)
    if (a < 0) != (b < 0):
        q = -q
    return q & mask, (a - q * b) & mask


def clear_shift(a, s, bits, left, arithmetic=False):
    mask = (1 << bits) - 1
    if arithmetic:
        return (signed(a, bits) >> min(s, bits)) & mask
    if s >= bits:
        return 0
    return (a << s) & mask if left else a >> s


# ------------------------------------------------------------------------------------------ bootstrap counts
# the closed formulas of docs/history/shift_rotate_log.md and docs/history/div_rem_log.md, restated
def propagate_pbs(L):
    if L == 1:
        return 1
    n = [L]
    while n[-1] > 4:
        n.append((n[-1] + 2) // 3)
    top = len(n) - 1
    count = 2 * L + sum(n[l] - 1 for l in range(1, top + 1)) + (L // 3 if top >= 1 else 0) + n[top] - 1
    return count + sum(n[l] - (n[l] + 2) // 3 for l in range(1, top))


def comparison_pbs(L):
    digits = L + (L % 2 if L > 1 else 0)
    return 1 if digits == 1 else propagate_pbs(digits) - digits + 1


def shift_rotate_pbs(shift, L, b):
    B = b * L
    ctrl = control_bits(B)
    return B + ctrl + ctrl * B + (comparison_pbs(L) + 1 if shift else 0) + (b - 1) * L


def division_pbs(is_signed, L, b):
    B, lg = b * L, (L - 1).bit_length()
    n = (2 * b - 1) * L + L * lg + (b - 1) * L + 5 * b * L * (L + 1) // 2 + B * (2 + propagate_pbs(L)) + 2 * L
    if is_signed:
        n += 2 * (1 + propagate_pbs(L) + L) + 1 + 2 * (propagate_pbs(L) + L)
    return n


# ------------------------------------------------------------------------------------------ samples, operands
@dataclasses.dataclass
class Sample:
    clear: int
    ct: object                # None in a dry run
    producer: str             # "<operation>@<step>" or "encrypt"
    degrees: list             # a dry run's prediction; a real run reads the ciphertext's
    noise: list


@dataclasses.dataclass
class Info:
    """degrees and noise levels of one operand as the wrapper sees them"""
    degrees: list
    noise: list

    def clean(self, msg):
        return max(self.degrees, default=0) <= msg - 1 and max(self.noise, default=0) <= 1


# operand kinds: L / R a sample of the lhs / rhs pool, U a sample of either (the side is drawn), B a boolean sample,
# S a clear scalar below 2^bits, A a clear shift amount, F a clear factor 0 .. 3, M a coin (0 / 1)
@dataclasses.dataclass(frozen=True)
class Executor:
    name: str
    refs: tuple               # the reference's names this stands for ("signed <name>": of its signed test)
    operands: str
    outs: str                 # I an integer, B a boolean, per output
    call: object              # (h, args) -> (outputs, bootstrap count or None)
    clear: object             # (h, *clear operands) -> tuple of clear outputs
    needs_clean: bool = True
    inout: int = None         # which ciphertext operand the call writes (it is duplicated first)
    predict: object = None    # unchecked operations: (h, infos, scalars) -> Info of the result
    count: object = None      # (h, scalars) -> bootstraps the call reports
    only_base: tuple = None   # (msg, carry) the operation is wired at
    events: object = None     # (h, clears) -> set of census events the operands are


def _digits(h, v):
    return [(v // h.msg ** j) % h.msg for j in range(h.L)]


def _inplace(method, *extra, **kw):
    """lhs <- method(lhs, rhs, ...): the duplicate of the left operand is the result"""
    def call(h, a):
        pbs = getattr(h.c.sks, method)(a[0], *a[1:], *extra, h.c.st, **kw)
        return [a[0]], pbs if isinstance(pbs, int) and not isinstance(pbs, bool) else None
    return call


def _flagged(method, **kw):
    def call(h, a):
        flag = getattr(h.c.sks, method)(a[0], a[1], h.c.st, **kw)
        return [a[0], flag], None
    return call


def _bitop(op):
    return lambda h, a: (h.c.sks.bitop_assign(a[0], a[1], op, h.c.st), ([a[0]], None))[1]


def _scalar_bitop(op):
    return lambda h, a: (h.c.sks.scalar_bitop_assign(a[0], _digits(h, a[1]), op, h.c.st), ([a[0]], None))[1]


def _compare(op):
    return lambda h, a: ([h.c.sks.compare(a[0], a[1], op, h.c.st)], None)


def _scalar_compare(op):
    return lambda h, a: ([h.c.sks.scalar_compare(a[0], a[1], op, h.c.st)], None)


def _scalar_add(negate):
    def call(h, a):
        s = (-a[1]) % h.top if negate else a[1]
        h.c.sks.unchecked_scalar_add_assign(a[0], _digits(h, s), h.c.st)
        h.c.sks.propagate_single_carry_assign(a[0], h.c.st)
        return [a[0]], None
    return call


def _neg(h, a):
    out = h.c.sks.unchecked_neg(a[0], h.c.st)
    h.c.sks.full_propagate_assign(out, h.c.st)
    return [out], None


def _scalar_shift(left, arithmetic=False):
    def call(h, a):
        h.c.sks.scalar_shift_assign(a[0], a[1], h.c.st, left=left, arithmetic=arithmetic)
        return [a[0]], None
    return call


def _scalar_rotate(left):
    return lambda h, a: (h.c.sks.scalar_rotate_assign(a[0], a[1], h.c.st, left=left), ([a[0]], None))[1]


def amount_mask(h):
    return (1 << control_bits(h.bits)) - 1


def _amount(h, a):
    """the encrypted amount: the rhs sample as it is, or (coin) its low control bits, so that amounts below the width
    occur as often as overshifts; the masked amount is itself a bootstrap output"""
    if not a[2]:
        return a[1]
    masked = h.dup(a[1])
    h.c.sks.scalar_bitop_assign(masked, _digits(h, amount_mask(h)), "and", h.c.st)
    return masked


def clear_amount(h, y, coin):
    return y & amount_mask(h) if coin else y


def _shift(left, arithmetic=False):
    def call(h, a):
        pbs = h.c.sks.shift_assign(a[0], _amount(h, a), h.c.st, left=left, arithmetic=arithmetic, return_pbs_count=True)
        return [a[0]], pbs
    return call


def _rotate(left):
    def call(h, a):
        pbs = h.c.sks.rotate_assign(a[0], _amount(h, a), h.c.st, left=left, return_pbs_count=True)
        return [a[0]], pbs
    return call


def _div_rem(is_signed):
    def call(h, a):
        q, r, pbs = h.c.sks.div_rem(a[0], a[1], h.c.st, signed=is_signed, return_pbs_count=True)
        direct = int(h.lib().hip_integer_div_rem_pbs_count(is_signed, h.L, h.msg, h.carry))
        assert pbs == direct, f"div_rem reports {pbs} bootstraps, hip_integer_div_rem_pbs_count {direct}"
        return [q, r], pbs
    return call


def _abs(h, a):
    h.c.sks.abs_assign(a[0], h.c.st)
    return [a[0]], None


def _sum(reduce):
    def call(h, a):
        if reduce:
            return [h.c.sks.sum_ciphertexts(list(a), h.c.st, reduce=True)], None
        L, w = h.L, a[0].lwe_dimension + 1
        igpu = h.c.igpu
        vec = igpu.CudaUnsignedRadixCiphertext(igpu.CudaVec(len(a) * L * w, h.c.st), len(a), L, a[0].lwe_dimension)
        for i, ct in enumerate(a):
            igpu._lib().cuda_memcpy_async_gpu_to_gpu(vec.d_blocks.ptr + i * L * w * 8, ct.d_blocks.ptr, L * w * 8, h.c.st.ptr[0],
                                                     h.c.st.gpu_indexes[0])
            vec._info[0][i * L:(i + 1) * L] = ct._info[0]
            vec._info[1][i * L:(i + 1) * L] = ct._info[1]
        out, pbs = h.c.sks.unchecked_partial_sum_ciphertexts(vec, h.c.st, reduce=False, return_pbs_count=True)
        return [out], pbs
    return call


def _unchecked_add(h, a):
    h.c.sks.unchecked_add_assign(a[0], a[1], h.c.st)
    return [a[0]], None


def _unchecked_scalar_add(h, a):
    h.c.sks.unchecked_scalar_add_assign(a[0], _digits(h, a[1]), h.c.st)
    return [a[0]], None


def _small_scalar_mul(h, a):
    """the levelled multiplication by a small clear factor (the reference's small_scalar_mul); the Python mirror has no
    method for it, the entry point is called as the mirror's methods call theirs"""
    s, keep = h.c.sks._streams(h.c.st)
    import ctypes
    h.c.igpu._lib().hip_small_scalar_multiplication_integer_64_inplace_async(s, ctypes.byref(a[0]._ffi()), int(a[1]), h.msg, h.carry)
    return [a[0]], None


def _unchecked_scalar_mul(h, a):
    return [h.c.sks.unchecked_scalar_mul(a[0], a[1], h.c.st)], None


def _scalar_mul(h, a):
    pbs = h.c.sks.scalar_mul_assign(a[0], a[1], h.c.st, return_pbs_count=True)
    return [a[0]], pbs


def _mul(h, a):
    pbs = h.c.sks.mul_assign(a[0], a[1], h.c.st, return_pbs_count=True)
    return [a[0]], pbs


def _if_then_else(h, a):
    return [h.c.sks.if_then_else(a[0], a[1], a[2], h.c.st)], None


def _mul_by_boolean(h, a):
    h.c.sks.mul_by_boolean_assign(a[0], a[1], h.c.st)
    return [a[0]], None


def _bitnot(h, a):
    h.c.sks.bitnot_assign(a[0], h.c.st)
    return [a[0]], None


def _re_randomize(h, a):
    key, zeros = h.rerand_material()
    a[0].re_randomize(zeros, key, h.c.st)
    return [a[0]], None


def _compress_round_trip(h, a):
    comp, dec = h.compression_material()
    packed = h.c.igpu.CudaCompressedCiphertextList.compress([a[0]], comp, h.c.st)
    return [packed.get(0, dec, h.c.st)], None


# ---- degree and noise rules of the levelled operations (the reference's host code: linear_algebra, scalar_addition.cuh,
# negation.cuh host_negation_with_correcting_term, scalar_mul.cuh host_integer_small_scalar_mul_radix)
def _after_add(h, infos, scalars):
    return Info([x + y for x, y in zip(infos[0].degrees, infos[1].degrees)], [x + y for x, y in zip(infos[0].noise, infos[1].noise)])


def _after_scalar_add(h, infos, scalars):
    return Info([x + y for x, y in zip(infos[0].degrees, _digits(h, scalars[0]))], list(infos[0].noise))


def _after_small_mul(h, infos, scalars):
    return Info([x * scalars[0] for x in infos[0].degrees], [x * scalars[0] for x in infos[0].noise])


def negation_degrees(degrees, msg):
    out, zb = [], 0
    for d in degrees:
        z = max(1, (d + zb) // msg) * msg
        out.append(z - zb)
        zb = z // msg
    return out


def _b(x):
    return int(bool(x))


def _cmp(f):
    return lambda h, x, y: (_b(f(x, y)),)


def _mod(f):
    return lambda h, *v: (f(*v) % h.top,)


def _shifted(left, arithmetic=False):
    return lambda h, x, y, coin: (clear_shift(x, clear_amount(h, y, coin), h.bits, left, arithmetic),)


def _overshift(h, clears):
    return {"overshift"} if clears[1] >= h.bits else set()


def _overshift_encrypted(h, clears):
    return {"overshift"} if clear_amount(h, clears[1], clears[2]) >= h.bits else set()


def _zero_divisor(h, clears):
    return {"divisor 0"} if clears[1] == 0 else set()


ORDER = {"gt": lambda x, y: x > y, "ge": lambda x, y: x >= y, "lt": lambda x, y: x < y, "le": lambda x, y: x <= y,
         "eq": lambda x, y: x == y, "ne": lambda x, y: x != y}
BITS = {"and": lambda x, y: x & y, "or": lambda x, y: x | y, "xor": lambda x, y: x ^ y}
E = Executor


def executors():
    t = [
        E("add", ("add", "signed add"), "LR", "I", _inplace("add_assign"), _mod(lambda x, y: x + y), inout=0),
        E("sub", ("sub", "signed sub"), "LR", "I", _inplace("sub_assign"), _mod(lambda x, y: x - y), inout=0),
        E("mul", ("mul", "signed mul"), "LR", "I", _mul, _mod(lambda x, y: x * y), inout=0),
        E("neg", ("neg", "signed neg"), "U", "I", _neg, _mod(lambda x: -x)),
        E("bitnot", ("bitnot", "signed bitnot"), "U", "I", _bitnot, lambda h, x: (h.top - 1 - x,), inout=0),
        E("scalar add", ("scalar add", "signed scalar add"), "US", "I", _scalar_add(False), _mod(lambda x, s: x + s), inout=0),
        E("scalar sub", ("scalar sub", "signed scalar sub"), "US", "I", _scalar_add(True), _mod(lambda x, s: x - s), inout=0),
        E("scalar mul", ("scalar mul", "signed scalar mul"), "US", "I", _scalar_mul, _mod(lambda x, s: x * s), inout=0),
        E("scalar left shift", ("scalar left shift", "signed scalar left shift"), "UA", "I", _scalar_shift(True),
          lambda h, x, s: (clear_shift(x, s, h.bits, True),), inout=0, events=_overshift),
        E("scalar right shift", ("scalar right shift",), "UA", "I", _scalar_shift(False),
          lambda h, x, s: (clear_shift(x, s, h.bits, False),), inout=0, events=_overshift),
        E("signed scalar right shift", ("signed scalar right shift",), "UA", "I", _scalar_shift(False, True),
          lambda h, x, s: (clear_shift(x, s, h.bits, False, True),), inout=0, events=_overshift),
        E("scalar rotate left", ("scalar rotate left", "signed scalar rotate left"), "UA", "I", _scalar_rotate(True),
          lambda h, x, s: (rotl(x, s, h.bits),), inout=0, events=_overshift),
        E("scalar rotate right", ("scalar rotate right", "signed scalar rotate right"), "UA", "I", _scalar_rotate(False),
          lambda h, x, s: (rotr(x, s, h.bits),), inout=0, events=_overshift),
        E("left shift", ("left shift", "signed left shift"), "LRM", "I", _shift(True), _shifted(True), inout=0,
          count=lambda h, s: shift_rotate_pbs(True, h.L, h.b), events=_overshift_encrypted),
        E("right shift", ("right shift",), "LRM", "I", _shift(False), _shifted(False), inout=0,
          count=lambda h, s: shift_rotate_pbs(True, h.L, h.b), events=_overshift_encrypted),
        E("signed right shift", ("signed right shift",), "LRM", "I", _shift(False, True), _shifted(False, True), inout=0,
          count=lambda h, s: shift_rotate_pbs(True, h.L, h.b), events=_overshift_encrypted),
        E("rotate left", ("rotate left", "signed rotate left"), "LRM", "I", _rotate(True),
          lambda h, x, y, coin: (rotl(x, encrypted_rotation(clear_amount(h, y, coin), h.bits), h.bits),), inout=0,
          count=lambda h, s: shift_rotate_pbs(False, h.L, h.b), events=_overshift_encrypted),
        E("rotate right", ("rotate right", "signed rotate right"), "LRM", "I", _rotate(False),
          lambda h, x, y, coin: (rotr(x, encrypted_rotation(clear_amount(h, y, coin), h.bits), h.bits),), inout=0,
          count=lambda h, s: shift_rotate_pbs(False, h.L, h.b), events=_overshift_encrypted),
        E("max", ("max",), "LR", "I", _compare("max"), lambda h, x, y: (max(x, y),)),
        E("min", ("min",), "LR", "I", _compare("min"), lambda h, x, y: (min(x, y),)),
        E("scalar max", (), "US", "I", _scalar_compare("max"), lambda h, x, y: (max(x, y),)),
        E("scalar min", (), "US", "I", _scalar_compare("min"), lambda h, x, y: (min(x, y),)),
        E("select", ("select", "signed select"), "BLR", "I", _if_then_else, lambda h, k, x, y: (x if k else y,)),
        E("mul by boolean", (), "UB", "I", _mul_by_boolean, lambda h, x, k: (x if k else 0,), inout=0),
        E("overflowing add", ("overflowing add",), "LR", "IB", _flagged("add_assign", want_carry_out=True),
          lambda h, x, y: ((x + y) % h.top, _b(x + y >= h.top)), inout=0),
        E("overflowing sub", ("overflowing sub",), "LR", "IB", _flagged("unsigned_overflowing_sub_assign"),
          lambda h, x, y: ((x - y) % h.top, _b(x < y)), inout=0),
        E("signed overflowing add", ("signed overflowing add",), "LR", "IB", _flagged("add_assign", want_overflow=True),
          lambda h, x, y: ((x + y) % h.top, _b(not -(h.top >> 1) <= signed(x, h.bits) + signed(y, h.bits) < (h.top >> 1))),
          inout=0),
        E("div rem", ("div rem",), "LR", "II", _div_rem(False), lambda h, x, y: clear_div_rem(x, y, h.bits),
          count=lambda h, s: division_pbs(False, h.L, h.b), events=_zero_divisor),
        E("signed div rem", ("signed div rem",), "LR", "II", _div_rem(True), lambda h, x, y: clear_signed_div_rem(x, y, h.bits),
          count=lambda h, s: division_pbs(True, h.L, h.b), events=_zero_divisor),
        E("signed abs", ("signed abs",), "U", "I", _abs, lambda h, x: (abs(signed(x, h.bits)) % h.top,), inout=0),
        E("sum of 3", (), "LRU", "I", _sum(True), _mod(lambda x, y, z: x + y + z), needs_clean=False),
        # the unchecked forms: they leave carries, so that unclean samples enter the pools
        E("unchecked add", (), "LR", "I", _unchecked_add, _mod(lambda x, y: x + y), needs_clean=False, inout=0,
          predict=_after_add),
        E("unchecked neg", (), "U", "I", lambda h, a: ([h.c.sks.unchecked_neg(a[0], h.c.st)], None), _mod(lambda x: -x),
          predict=lambda h, infos, scalars: Info(negation_degrees(infos[0].degrees, h.msg), list(infos[0].noise))),
        E("unchecked scalar add", (), "US", "I", _unchecked_scalar_add, _mod(lambda x, s: x + s), needs_clean=False, inout=0,
          predict=_after_scalar_add),
        E("unchecked scalar mul", (), "UF", "I", _unchecked_scalar_mul, _mod(lambda x, s: x * s)),
        E("small scalar mul", (), "UF", "I", _small_scalar_mul, _mod(lambda x, s: x * s), needs_clean=False, inout=0,
          predict=_after_small_mul),
        E("partial sum of 3", (), "LRU", "I", _sum(False), _mod(lambda x, y, z: x + y + z), needs_clean=False),
        # value-preserving
        E("re-randomize", (), "U", "I", _re_randomize, lambda h, x: (x,), inout=0, only_base=(4, 4)),
        E("compress and get", (), "U", "I", _compress_round_trip, lambda h, x: (x,), only_base=(4, 4)),
    ]
    for op, f in BITS.items():
        t.append(E("bit" + op, ("bit" + op, "signed bit" + op), "LR", "I", _bitop(op), (lambda f: lambda h, x, y: (f(x, y),))(f), inout=0))
        t.append(E("scalar bit" + op, ("scalar bit" + op, "signed scalar bit" + op), "US", "I", _scalar_bitop(op),
                   (lambda f: lambda h, x, y: (f(x, y),))(f), inout=0))
    for op, f in ORDER.items():
        equality = ("signed " + op,) if op in ("eq", "ne") else ()       # eq / ne do not read the sign
        t.append(E(op, (op,) + equality, "LR", "B", _compare(op), _cmp(f)))
        t.append(E("scalar " + op, ("scalar " + op,) + tuple("signed scalar " + e[7:] for e in equality), "US", "B",
                   _scalar_compare(op), _cmp(f)))
    return {e.name: e for e in t}


EXECUTORS = executors()

# executors that stand for no name of the reference's lists: this project's own forms of the operations
PROJECT_ONLY = ["scalar max", "scalar min", "mul by boolean", "sum of 3", "unchecked add", "unchecked neg",
                "unchecked scalar add", "unchecked scalar mul", "small scalar mul", "partial sum of 3", "re-randomize",
                "compress and get"]

# names of the reference's lists that no executor stands for (the radix layer has no such operation yet, or, for the
# signed list, only its unsigned form)
NOT_WIRED = (
    ["scalar div rem", "ilog2", "count ones", "count zeros", "reverse bits", "match_value", "match_value_or", "overflowing mul",
     "overflowing scalar add", "overflowing scalar sub"] +
    ["par_generate_oblivious_pseudo_random_unsigned_" + s + r for s in ("integer", "integer_bounded", "custom_range")
     for r in ("", "_and_re_randomize")] +
    ["signed " + n for n in ["scalar div rem", "ilog2", "count ones", "count zeros", "reverse bits", "overflowing mul",
                             "overflowing scalar add", "overflowing scalar sub", "overflowing sub",
                             "gt", "ge", "lt", "le", "max", "min", "scalar gt", "scalar ge", "scalar lt", "scalar le"]] +
    ["signed par_generate_oblivious_pseudo_random_signed_" + s + r for s in ("integer", "integer_bounded")
     for r in ("", "_and_re_randomize")])

ACCEPTS_UNCLEAN = [e.name for e in EXECUTORS.values() if not e.needs_clean]
EVENTS = ("divisor 0", "overshift", "produced boolean as the cmux condition")


def reference_names(lists):
    """the names of tests/golden/reference_long_run_ops.json as the executors' `refs` spell them"""
    return set(lists["unsigned"]) | {"signed " + n for n in lists["signed"]}


# ------------------------------------------------------------------------------------------ the runner
class StepFailure(AssertionError):
    pass


class Runner:
    """Pools, schedule, wrapper and checks of one sequence.  c: a Ctx of tests/test_radix_bases.py (keys on a backend at a
    base), or None for a dry run.  helpers: what the value-preserving operations need (set by the test module)."""

    def __init__(self, c, msg, carry, L, seed, copies, helpers=None):
        self.c, self.msg, self.carry, self.L, self.seed, self.copies = c, msg, carry, L, seed, copies
        self.b = msg.bit_length() - 1
        self.bits, self.top = self.b * L, msg ** L
        self.cap = msg * carry - 1                              # what a block holds
        self.max_noise = (msg * carry - 1) // (msg - 1)         # the bound of the levelled multiplication (integer.hip)
        self.rng = np.random.default_rng(seed)
        self.helpers = helpers
        self.names = [n for n, e in EXECUTORS.items() if e.only_base in (None, (msg, carry))]
        self.schedule = [n for _ in range(copies) for n in self.names]
        self.rng.shuffle(self.schedule)
        self.enc_seed = 1000 * (seed % 1000003)
        self.lhs = [self.fresh_int() for _ in range(POOL)]
        self.rhs = [self.fresh_int() for _ in range(POOL)]
        self.bools = [self.fresh_bool() for _ in range(POOL)]
        self.propagations = 0
        self.bootstraps = 0                                      # of the operations that report a count
        self.skipped = []
        self.census = {n: {"runs": 0, "produced": 0, "unclean": 0} for n in self.names}
        self.seen_events = {e: 0 for e in EVENTS}
        self.log = []

    # ---- draws
    def draw_value(self):
        if self.rng.random() < EDGE_PROBABILITY:
            return int(self.rng.choice([0, 1, self.top - 1, self.top >> 1, self.bits])) % self.top
        return int(self.rng.integers(0, self.top))

    def draw_amount(self):
        if self.rng.random() < EDGE_PROBABILITY:
            return int(self.rng.choice([0, 1, self.top - 1, self.top >> 1, self.bits]))
        return int(self.rng.integers(0, self.bits))

    def next_seed(self):
        self.enc_seed += 1
        return self.enc_seed

    def fresh_int(self):
        v, seed = self.draw_value(), self.next_seed()
        ct = self.c.enc([_digits(self, v)], seed) if self.c else None
        if ct is not None:
            ct._info[1][:] = 1
        return Sample(v, ct, "encrypt", [self.msg - 1] * self.L, [1] * self.L)

    def fresh_bool(self):
        v, seed = int(self.rng.integers(0, 2)), self.next_seed()
        ct = self.c.enc([[v]], seed, degree=1) if self.c else None
        return Sample(v, ct, "encrypt", [1], [1])

    def draw_operands(self, ex):
        """as the reference's generator: an index into the lhs pool and one into the rhs pool for a binary operation, a
        side and an index for a unary one; scalars biased towards the edges"""
        out = []
        for kind in ex.operands:
            if kind == "L":
                out.append(self.lhs[int(self.rng.integers(0, POOL))])
            elif kind == "R":
                out.append(self.rhs[int(self.rng.integers(0, POOL))])
            elif kind == "U":
                side = self.lhs if int(self.rng.integers(0, 2)) == 0 else self.rhs
                out.append(side[int(self.rng.integers(0, POOL))])
            elif kind == "B":
                out.append(self.bools[int(self.rng.integers(0, POOL))])
            elif kind == "S":
                out.append(self.draw_value())
            elif kind == "A":
                out.append(self.draw_amount())
            elif kind == "F":
                out.append(int(self.rng.integers(0, 4)))
            elif kind == "M":
                out.append(int(self.rng.random() < 0.75))
            else:
                raise ValueError(kind)
        return out

    def store(self, ex, step, clears, cts, infos):
        for kind, v, ct, info in zip(ex.outs, clears, cts, infos):
            sample = Sample(v, ct, f"{ex.name}@{step}", list(info.degrees), list(info.noise))
            if kind == "B":
                self.bools[int(self.rng.integers(0, POOL))] = sample
            else:
                side = self.lhs if int(self.rng.integers(0, 2)) == 0 else self.rhs
                side[int(self.rng.integers(0, POOL))] = sample

    # ---- ciphertexts
    def lib(self):
        return self.c.igpu._lib()

    def info(self, sample):
        if sample.ct is None:
            return Info(list(sample.degrees), list(sample.noise))
        return Info([int(x) for x in sample.ct._info[0]], [int(x) for x in sample.ct._info[1]])

    def dup(self, ct):
        out = ct.duplicate(self.c.st)
        out._info[0][:] = ct._info[0]
        out._info[1][:] = ct._info[1]
        return out

    def rerand_material(self):
        return self.helpers["rerand"](self)

    def compression_material(self):
        return self.helpers["compression"](self)

    # ---- the wrapper
    def fits(self, info):
        """what the reference's smart operations ask before a levelled operation: every block, with the carry the blocks
        below can hand it in a propagation, stays within what a block holds, and the noise level within its bound"""
        carry = 0
        for d in info.degrees:
            if d + carry > self.cap:
                return False
            carry = (d + carry) // self.msg
        return max(info.noise, default=0) <= self.max_noise

    def plan(self, ex, infos, scalars):
        """which ciphertext operands (indices into infos) are propagated before the call, in order"""
        clean = Info([self.msg - 1] * self.L, [1] * self.L)
        infos, out = list(infos), []
        if ex.needs_clean:
            out = [i for i, x in enumerate(infos) if not x.clean(self.msg)]
        elif ex.predict is not None:
            while not self.fits(ex.predict(self, infos, scalars)):
                i = next(i for i, x in enumerate(infos) if not x.clean(self.msg))   # a StopIteration: clean operands do not fit
                infos[i] = clean
                out.append(i)
        else:      # the sums: terms within a block (the checks above keep every sample there) at nominal noise
            out = [i for i, x in enumerate(infos) if max(x.noise, default=0) > 1]
        for i in out:
            infos[i] = clean
        return out, infos

    # ---- one step
    def describe(self, step, ex, operands):
        parts = []
        for kind, x in zip(ex.operands, operands):
            if isinstance(x, Sample):
                parts.append(f"{kind}={x.clear} degrees={self.info(x).degrees} noise={self.info(x).noise} from {x.producer}")
            else:
                parts.append(f"{kind}={x}")
        return f"seed={self.seed} step={step} op={ex.name!r}: " + "; ".join(parts)

    def run_step(self, step, name, checked=True):
        ex = EXECUTORS[name]
        operands = self.draw_operands(ex)
        samples = [x for x in operands if isinstance(x, Sample)]
        scalars = [x for x in operands if not isinstance(x, Sample)]
        clears = [x.clear if isinstance(x, Sample) else x for x in operands]
        want = ex.clear(self, *clears)
        assert len(want) == len(ex.outs)
        infos = [self.info(x) for x in samples]
        to_propagate, entering = self.plan(ex, infos, scalars)
        self.propagations += len(to_propagate)
        stat = self.census[name]
        stat["runs"] += 1
        stat["produced"] += any(x.producer != "encrypt" for x in samples)
        stat["unclean"] += any(max(x.degrees) > self.msg - 1 for x in entering)
        events = set(ex.events(self, clears)) if ex.events else set()
        if name == "select" and samples[0].producer != "encrypt":
            events.add("produced boolean as the cmux condition")
        for e in events:
            self.seen_events[e] += 1
        what = self.describe(step, ex, operands)
        if self.c is None:
            predicted = ex.predict(self, entering, scalars) if ex.predict else None
            out_infos = []
            for kind in ex.outs:
                if kind == "B":
                    out_infos.append(Info([1], [1]))
                elif predicted is not None:
                    out_infos.append(predicted)
                elif name == "partial sum of 3":      # what the plan leaves is the library's: unclean, for the search
                    out_infos.append(Info([self.msg] * self.L, [2] * self.L))
                else:
                    out_infos.append(Info([self.msg - 1] * self.L, [1] * self.L))
            self.store(ex, step, want, [None] * len(want), out_infos)
            return
        if not checked:       # a replayed step: checked by the case that owns it, here it only fills the pools
            out_cts, _ = self.execute(ex, samples, scalars, to_propagate, entering, what)
        else:
            out_cts = self.execute_and_check(step, ex, samples, scalars, to_propagate, entering, want, what)
        self.store(ex, step, want, out_cts, [Info(list(map(int, ct._info[0])), list(map(int, ct._info[1]))) for ct in out_cts])

    def execute(self, ex, samples, scalars, to_propagate, entering, what):
        """one execution on the samples: duplicates where the call writes or the wrapper propagates, the call itself"""
        cts = []
        for i, x in enumerate(samples):
            ct = x.ct
            if i == ex.inout or i in to_propagate:
                ct = self.dup(ct)
            if i in to_propagate:
                self.c.sks.full_propagate_assign(ct, self.c.st)
                got = Info([int(d) for d in ct._info[0]], [int(d) for d in ct._info[1]])
                if got != entering[i]:
                    raise StepFailure(f"{what}: full propagation of operand {i} wrote degrees {got.degrees} noise {got.noise}")
            cts.append(ct)
        # arguments in operand order: ciphertexts where the operand is a sample, the scalar otherwise
        args, ci, si = [], 0, 0
        for kind in ex.operands:
            if kind in "LRUB":
                args.append(cts[ci])
                ci += 1
            else:
                args.append(scalars[si])
                si += 1
        outs, pbs = ex.call(self, args)
        return outs, pbs

    def execute_and_check(self, step, ex, samples, scalars, to_propagate, entering, want, what):
        c = self.c
        before = [(c.words(x.ct).copy(), self.info(x)) for x in samples]
        runs = []
        for _ in range(2):
            outs, pbs = self.execute(ex, samples, scalars, to_propagate, entering, what)
            runs.append(([c.words(ct).copy() for ct in outs], [(list(map(int, ct._info[0])), list(map(int, ct._info[1]))) for ct in outs],
                         pbs, outs))
        (words1, info1, pbs1, outs), (words2, info2, pbs2, _) = runs
        # (b) determinism: words, degrees, noise levels, bootstrap count
        for k, (w1, w2) in enumerate(zip(words1, words2)):
            if not np.array_equal(w1, w2):
                bad = np.flatnonzero((w1 != w2).reshape(w1.shape[1], -1).any(axis=1)).tolist()
                raise StepFailure(f"{what}: output {k} differs word for word between two executions (blocks {bad})")
        if info1 != info2 or pbs1 != pbs2:
            raise StepFailure(f"{what}: degrees / noise / bootstrap count differ between two executions: {info1, pbs1} / {info2, pbs2}")
        # (c) the operands are as they were
        for i, (x, (w, info)) in enumerate(zip(samples, before)):
            if not np.array_equal(c.words(x.ct), w) or self.info(x) != info:
                raise StepFailure(f"{what}: operand {i} was changed")
        # (a), (d), (e)
        for k, (kind, ct, v) in enumerate(zip(ex.outs, outs, want)):
            blocks = [int(x) for x in c.dec(ct)[0]]
            degrees, noise = info1[k]
            if kind == "B":
                if len(blocks) != 1 or blocks[0] != v:
                    raise StepFailure(f"{what}: output {k} decrypts to blocks {blocks}, expected the boolean {v}")
            else:
                got = sum(x * self.msg ** j for j, x in enumerate(blocks)) % self.top
                if len(blocks) != self.L or got != v:
                    raise StepFailure(f"{what}: output {k} decrypts to {got} (blocks {blocks}), expected {v}")
            if any(x > d for x, d in zip(blocks, degrees)):
                raise StepFailure(f"{what}: output {k} holds blocks {blocks} above its degrees {degrees}")
            if any(d > self.cap for d in degrees):
                raise StepFailure(f"{what}: output {k} reports degrees {degrees}, a block holds {self.cap}")
            if any(n > self.max_noise for n in noise):
                raise StepFailure(f"{what}: output {k} reports noise levels {noise} above {self.max_noise}")
        # the levelled operations write what the reference's rules give
        if ex.predict is not None:
            p = ex.predict(self, entering, scalars)
            if info1[0] != (p.degrees, p.noise):
                raise StepFailure(f"{what}: wrote degrees / noise {info1[0]}, the rule gives {p.degrees, p.noise}")
        # (f) bootstrap count
        if ex.count is not None:
            expect = ex.count(self, scalars)
            if pbs1 != expect:
                raise StepFailure(f"{what}: {pbs1} bootstraps reported, the count formula gives {expect}")
        if pbs1 is not None:
            self.bootstraps += pbs1
        self.log.append(f"{step:3d} {ex.name}: {what.split(': ', 1)[1]} -> {list(want)}" +
                        (f" [{len(to_propagate)} propagated]" if to_propagate else "") + (f" [{pbs1} bootstraps]" if pbs1 else ""))
        return outs

    def run(self, check_from=0, stop=None):
        """steps [0, stop) of the schedule (all of it by default); the steps before `check_from` are executed once, without
        the checks: a sequence split over two cases replays its first part in the second"""
        for step, name in enumerate(self.schedule[:stop]):
            self.run_step(step, name, checked=step >= check_from)
        return self

    # ---- census
    def census_gaps(self):
        """what the sequence did not reach; empty for a committed seed"""
        gaps = [f"skipped: {s}" for s in self.skipped]
        for n, s in self.census.items():
            if s["runs"] != self.copies:
                gaps.append(f"{n} ran {s['runs']} times, not {self.copies}")
            if not s["produced"]:
                gaps.append(f"{n} never consumed a produced operand")
            if n in ACCEPTS_UNCLEAN and not s["unclean"]:
                gaps.append(f"{n} never consumed an unclean operand")
        gaps += [f"never entered: {e}" for e, k in self.seen_events.items() if not k]
        return gaps

    def census_line(self):
        unclean = {n: s["unclean"] for n, s in self.census.items() if n in ACCEPTS_UNCLEAN}
        return (f"{len(self.schedule)} steps, {len(self.names)} operations x {self.copies}; produced operands in "
                f"{sum(s['produced'] for s in self.census.values())} steps; unclean operands entered {unclean}; events "
                f"{self.seen_events}; {self.propagations} propagations inserted")
