"""The bootstrap over the 128-bit torus restated in plain Python integers, for tests/test_pbs128.py.

Restated (tfhe-rs paths): the u128 signed decomposer (core_crypto/commons/math/decomposition/{decomposer,iter}.rs), the
modulus switches (fft_impl/common.rs, algorithms/modulus_switch.rs: tests/common.py holds the centred one), accumulator
generation (shortint/engine), u128 key generation, encryption, decryption and a bootstrap whose external products are
EXACT negacyclic convolutions modulo 2^128 — one big-integer multiplication per polynomial product (Kronecker
substitution), nothing floating.  That bootstrap is what the kernels' f128 products are compared with, in phase.

A u128 array is a uint64 array with a trailing dimension of 2, (lo, hi).

Randomness: secret keys and the seeds come from tests/oracle.py's Rng; the bulk draws (masks, TUniform noise: tens of
millions of values for a full-size key) from NumPy generators seeded by it.  The mask-times-binary-key products of KEY
GENERATION go through float64 transforms on 16-bit limbs (sums below 2^29: exact, and asserted to be); this is not the
arithmetic under test.
"""
import concurrent.futures
import dataclasses
import functools
import multiprocessing
import os

import numpy as np

from . import oracle as orc
from .common import centered_ms_reference

U64 = np.uint64
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1


@dataclasses.dataclass(frozen=True)
class Params128:
    name: str
    n: int            # input (small) LWE dimension
    k: int
    N: int
    base_log: int
    level: int
    ms_type: int = 0  # 1: centred-mean modulus switch
    key_noise: int = 30     # TUniform bound (log2) of the u128 key
    input_noise: int = 46   # TUniform bound (log2) of the u64 inputs

    @property
    def log2N2(self):
        return (2 * self.N).bit_length() - 1


# NOISE_SQUASHING_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128 (tfhe/src/shortint/parameters/v1_4 .. v1_6/
# noise_squashing): k = 2, N = 2048, 3 levels of 24 bits, centred switch, on the classic 2_2 set's small key
PRODUCTION = Params128("noise_squashing_2_2", 918, 2, 2048, 24, 3, ms_type=1)
PRODUCTION_N32 = dataclasses.replace(PRODUCTION, name="noise_squashing_2_2_n32", n=32)
TOYS = [
    Params128("toy128_k1_N256", 16, 1, 256, 24, 3, ms_type=1),
    Params128("toy128_k2_N256", 16, 2, 256, 20, 4, ms_type=0),
    Params128("toy128_k1_N512", 16, 1, 512, 20, 4, ms_type=0),
    Params128("toy128_k2_N512", 16, 2, 512, 24, 3, ms_type=1),
]
PLAINTEXT_MODULUS = 16            # message_modulus * carry_modulus of 2_2
DELTA64 = (1 << 63) // PLAINTEXT_MODULUS
DELTA128 = (1 << 127) // PLAINTEXT_MODULUS


# ------------------------------------------------------------------------------------------------ u128 <-> pairs
def to_pairs(ints):
    a = np.empty((len(ints), 2), dtype=U64)
    a[:, 0] = [int(v) & M64 for v in ints]
    a[:, 1] = [(int(v) >> 64) & M64 for v in ints]
    return a


def from_pairs(pairs):
    p = np.asarray(pairs, dtype=U64).reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in zip(p[:, 0].tolist(), p[:, 1].tolist())]


def torus_distance128(a, b):
    d = (int(a) - int(b)) & M128
    return min(d, (1 << 128) - d)


# ------------------------------------------------------------------------------------------------ decomposer
def closest_representable_state(x, base_log, level, bits=128):
    """decomposer.rs:156-185 (init_decomposer_state): the closest representable on base_log * level bits, shifted down,
    balanced into [-2^(rep-1), 2^(rep-1)) by the rounding bit (two's complement on `bits` bits)."""
    rep = base_log * level
    mask = (1 << bits) - 1
    if rep >= bits:
        return x & mask
    res = x >> (bits - rep - 1)
    rounding_bit = res & 1
    res = ((res + 1) >> 1) & ((1 << rep) - 1)
    need_balance = ((((res - 1) & mask) | (rounding_bit << (rep - 1))) & res) >> (rep - 1)
    return (res - (need_balance << rep)) & mask


def decompose128(x, base_log, level, bits=128):
    """iter.rs:122-151: `level` balanced digits in [-B/2, B/2], least significant first (digit 0 belongs to level
    `level`, the smallest factor), as signed Python integers"""
    mask = (1 << bits) - 1
    state = closest_representable_state(x, base_log, level, bits)
    out = []
    for _ in range(level):
        res = state & ((1 << base_log) - 1)
        signed = state - (1 << bits) if state >> (bits - 1) else state
        state = (signed >> base_log) & mask
        carry = ((((res - 1) & mask) | state) & res) >> (base_log - 1)
        state = (state + carry) & mask
        out.append(res - (carry << base_log))
    return out


def recompose128(digits, base_log, level):
    return sum(d << (128 - base_log * (level - i)) for i, d in enumerate(digits)) & M128


# ------------------------------------------------------------------------------------------------ switches, LUT
def modulus_switch(x, log_modulus):
    return ((int(x) + (1 << (63 - log_modulus))) & M64) >> (64 - log_modulus)


def lwe_modulus_switch(lwe, log_modulus, ms_type):
    if ms_type:
        return [int(v) for v in centered_ms_reference(lwe, log_modulus)[0]]
    return [modulus_switch(v, log_modulus) for v in lwe]


def make_lut128(p, f):
    """shortint's accumulator on the 128-bit torus: box i of N / 16 coefficients holds f(i) * 2^127 / 16, rotated by half
    a box, the wrapped half negated; mask polynomials zero.  (k + 1) N Python integers."""
    box = p.N // PLAINTEXT_MODULUS
    body = [(f(j // box) * DELTA128) & M128 for j in range(p.N)]
    half = box // 2
    body = [(-v) & M128 for v in body[:half]] + body[half:]
    body = body[half:] + body[:half]
    return [0] * (p.k * p.N) + body


# ------------------------------------------------------------------------------------------------ keys
@dataclasses.dataclass
class Keys128:
    p: Params128
    lwe_sk: np.ndarray     # n bits
    glwe_sk: np.ndarray    # k * N bits (the output LWE key)
    bsk: np.ndarray        # [n][level][k + 1][k + 1][N][2] uint64


def _negacyclic_mask_times_key(mask_limbs, key_f):
    """mask_limbs [rows][k][8][N] float64 (16-bit limbs), key_f rfft of the k binary key polynomials over 2 N points ->
    sum_j mask_j * s_j per limb, [rows][8][N] int64 (exact: |sums| < 2^29)"""
    N = mask_limbs.shape[-1]
    f = np.fft.rfft(mask_limbs, n=2 * N, axis=-1) * key_f[None, :, None, :]
    lin = np.fft.irfft(f.sum(axis=1), n=2 * N, axis=-1)
    c = lin[..., :N] - lin[..., N:]
    r = np.rint(c)
    assert np.abs(c - r).max() < 0.05, "key generation: limb product not exact"
    return r.astype(np.int64)


def gen_bsk128(p, lwe_sk, glwe_sk, gen):
    """GGSW encryptions of the bits of lwe_sk under glwe_sk on the 128-bit torus, reference container order: level matrix
    idx of a GGSW carries the factor 2^(128 - base_log * (level - idx)) (index 0: the last level); row r < k encrypts
    -bit * factor * S_r, row k encrypts bit * factor, as GLWE encryptions with uniform masks and TUniform noise."""
    n, k, N, L = p.n, p.k, p.N, p.level
    rows = L * (k + 1)
    s = np.asarray(glwe_sk, dtype=np.int64).reshape(k, N)
    key_f = np.fft.rfft(s.astype(np.float64), n=2 * N, axis=-1)
    out = np.zeros((n, L, k + 1, k + 1, N, 2), dtype=U64)
    for i in range(n):
        limbs = gen.integers(0, 1 << 16, size=(rows, k, 8, N), dtype=np.int64)
        prod = _negacyclic_mask_times_key(limbs.astype(np.float64), key_f)      # [rows][8][N]
        noise = gen.integers(-(1 << p.key_noise), (1 << p.key_noise) + 1, size=(rows, N), dtype=np.int64)
        # body = sum of limbs 2^(16 l) + noise + message, carried through 32-bit words held in int64
        A = [prod[:, 2 * w, :] + (prod[:, 2 * w + 1, :] << 16) for w in range(4)]
        A[0] = A[0] + noise
        words = []
        carry = np.zeros_like(A[0])
        for w in range(4):
            t = A[w] + carry
            words.append(t & 0xFFFFFFFF)
            carry = t >> 32
        lo = words[0].astype(U64) | (words[1].astype(U64) << U64(32))
        hi = words[2].astype(U64) | (words[3].astype(U64) << U64(32))
        lm = limbs.astype(U64)
        m_lo = lm[:, :, 0] | (lm[:, :, 1] << U64(16)) | (lm[:, :, 2] << U64(32)) | (lm[:, :, 3] << U64(48))
        m_hi = lm[:, :, 4] | (lm[:, :, 5] << U64(16)) | (lm[:, :, 6] << U64(32)) | (lm[:, :, 7] << U64(48))
        g = out[i].reshape(rows, k + 1, N, 2)
        g[:, :k, :, 0] = m_lo
        g[:, :k, :, 1] = m_hi
        g[:, k, :, 0] = lo
        g[:, k, :, 1] = hi
        if int(lwe_sk[i]):
            for idx in range(L):
                shift = 128 - p.base_log * (L - idx)
                for r in range(k + 1):
                    row = g[idx * (k + 1) + r, k]          # the body polynomial of that row, [N][2]
                    if r == k:
                        add = [1 << shift] + [0] * (N - 1)
                    else:
                        add = [(-(int(b) << shift)) & M128 for b in s[r]]
                    vals = [(v + a) & M128 for v, a in zip(from_pairs(row), add)]
                    row[:] = to_pairs(vals)
    return out


@functools.lru_cache(maxsize=8)
def make_keys128(p, seed=0x31323862, compute=None):
    """compute: a 64-bit parameter set of tests/common.py whose small key the inputs are under (noise squashing takes
    the compute set's keyswitched blocks); None: a key of this helper's own"""
    rng = orc.Rng(seed)
    lwe_sk = rng.binary_key(p.n)
    if compute is not None:
        from .common import make_keys
        lwe_sk = make_keys(compute).lwe_sk
        assert len(lwe_sk) == p.n
    glwe_sk = rng.binary_key(p.k * p.N)
    gen = np.random.default_rng(int(rng.next()))
    return Keys128(p, lwe_sk, glwe_sk, gen_bsk128(p, lwe_sk, glwe_sk, gen))


def encrypt_inputs(p, keys, msgs, seed=7):
    """u64 LWEs under the small key, message * 2^63 / 16 plus TUniform(input_noise)"""
    rng = orc.Rng(seed)
    return np.stack([orc.lwe_encrypt(rng, keys.lwe_sk, (int(m) * DELTA64) & M64, p.input_noise) for m in msgs])


def phase128(p, keys, lwe_pairs):
    """b - <a, s> modulo 2^128 of one output LWE ([k N + 1][2] uint64)"""
    v = from_pairs(lwe_pairs)
    acc = v[-1]
    for a, s in zip(v[:-1], keys.glwe_sk.tolist()):
        if s:
            acc -= a
    return acc & M128


def decode128(phase):
    """the 5-bit rounding of the reference's test: padding bit and four message bits"""
    return ((phase + (1 << 122)) >> 123) & 31


# ------------------------------------------------------------------------------------------------ exact bootstrap
class ExactKey:
    """the key's polynomials as Kronecker operands, built once per key"""

    def __init__(self, p, keys):
        self.p = p
        terms = (p.k + 1) * p.level
        self.slot = (p.base_log + 128 + p.N.bit_length() + terms.bit_length() + 2 + 7) // 8   # bytes per coefficient
        flat = keys.bsk.reshape(-1, p.N, 2)
        buf = np.zeros((flat.shape[0], p.N, self.slot), dtype=np.uint8)
        buf[:, :, :16] = np.ascontiguousarray(flat).view(np.uint8).reshape(flat.shape[0], p.N, 16)
        self.ops = [int.from_bytes(buf[j].tobytes(), "little") for j in range(flat.shape[0])]
        self.bias = sum(1 << (8 * self.slot * t + 8 * self.slot - 1) for t in range(2 * p.N))

    def op(self, i, idx, row, col):
        p = self.p
        return self.ops[((i * p.level + idx) * (p.k + 1) + row) * (p.k + 1) + col]

    def pack_digits(self, digits):
        """digits: N Python integers in [-2^63, 2^63] (base_log 64 reaches both ends, so the signed values do not fit an
        int64; their magnitudes fit a uint64) -> the Kronecker operand, positive part minus negative part"""
        N = self.p.N
        digits = [int(v) for v in digits]
        assert len(digits) == N and all(-(1 << 63) <= v <= (1 << 63) for v in digits)
        buf = np.zeros((2, N, self.slot), dtype=np.uint8)
        buf[0, :, :8] = np.array([v if v > 0 else 0 for v in digits], dtype=U64).view(np.uint8).reshape(N, 8)
        buf[1, :, :8] = np.array([-v if v < 0 else 0 for v in digits], dtype=U64).view(np.uint8).reshape(N, 8)
        return int.from_bytes(buf[0].tobytes(), "little") - int.from_bytes(buf[1].tobytes(), "little")

    def unpack_negacyclic(self, total):
        """coefficients of the (signed) sum of products, folded modulo X^N + 1, modulo 2^128"""
        N = self.p.N
        raw = np.frombuffer((total + self.bias).to_bytes(2 * N * self.slot + 8, "little"), dtype=np.uint8)
        w = np.ascontiguousarray(raw[:2 * N * self.slot].reshape(2 * N, self.slot)[:, :16]).view(U64).reshape(2 * N, 2)
        lo = w[:N, 0] - w[N:, 0]
        hi = w[:N, 1] - w[N:, 1] - (w[:N, 0] < w[N:, 0]).astype(U64)
        return [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())]


def _monomial_mul(poly, deg, N):
    """poly * X^deg modulo X^N + 1, deg < 2 N"""
    r, odd = deg % N, deg >= N
    out = [(-v) & M128 for v in poly[N - r:]] + poly[:N - r] if r else list(poly)
    return [(-v) & M128 for v in out] if odd else out


def bootstrap_exact(p, ekey, lwe, lut):
    """fft128_pbs.rs with exact external products: modulus switch to 2 N, LUT * X^-b, n CMUX steps
    ACC += ((ACC X^a - ACC) decomposed) x GGSW_i, sample extraction of coefficient 0.  Returns k N + 1 integers."""
    k, N, L = p.k, p.N, p.level
    ms = lwe_modulus_switch(lwe, p.log2N2, p.ms_type)
    acc = [_monomial_mul(lut[c * N:(c + 1) * N], (2 * N - ms[-1]) % (2 * N), N) for c in range(k + 1)]
    for i in range(p.n):
        a = ms[i]
        if a == 0:
            continue
        packed = []
        for row in range(k + 1):
            rot = _monomial_mul(acc[row], a, N)
            digs = [decompose128((x - y) & M128, p.base_log, L) for x, y in zip(rot, acc[row])]
            packed.append([ekey.pack_digits([d[idx] for d in digs]) for idx in range(L)])
        for col in range(k + 1):
            total = 0
            for row in range(k + 1):
                for idx in range(L):
                    total += packed[row][idx] * ekey.op(i, idx, row, col)
            add = ekey.unpack_negacyclic(total)
            acc[col] = [(x + y) & M128 for x, y in zip(acc[col], add)]
    out = []
    for c in range(k):
        out += [acc[c][0]] + [(-acc[c][N - j]) & M128 for j in range(1, N)]
    return out + [acc[k][0]]


def negacyclic_product_exact(a, b, N):
    """a (u128 words) times b (small signed integers) modulo X^N + 1 and 2^128, by one big-integer multiplication"""
    slot = 8 * ((128 + 64 + N.bit_length() + 2 + 7) // 8)
    A = sum(int(v) << (slot * t) for t, v in enumerate(a))
    B = sum(int(v) << (slot * t) for t, v in enumerate(b))
    bias = sum(1 << (slot * t + slot - 1) for t in range(2 * N))
    T = A * B + bias
    lin = [((T >> (slot * t)) & ((1 << slot) - 1)) - (1 << (slot - 1)) for t in range(2 * N)]
    return [(lin[t] - lin[t + N]) & M128 for t in range(N)]


# ------------------------------------------------------------------------------------------------ exact phases, in parallel
_worker_state = {}


def _exact_phase_worker(job):
    """one bootstrap in a fresh interpreter (no device, no library of the backend): keys and key operands are rebuilt
    from the seed there, once per process"""
    p, seed, lwe, lut = job
    if (p, seed) not in _worker_state:
        keys = make_keys128(p, seed)
        _worker_state[(p, seed)] = (keys, ExactKey(p, keys))
    keys, ekey = _worker_state[(p, seed)]
    return phase128(p, keys, to_pairs(bootstrap_exact(p, ekey, lwe, lut)))


def exact_phases(p, lwes, luts, seed=0x31323862, workers=None):
    """phase under the output key of the exact bootstrap of lwes[i] with luts[i], the bootstraps spread over fresh child
    processes (spawned, not forked: the parent may hold a device)"""
    jobs = [(p, seed, np.asarray(lwe), lut) for lwe, lut in zip(lwes, luts)]
    workers = workers or max(1, min(8, len(jobs), os.cpu_count() or 1))
    if workers == 1:
        return [_exact_phase_worker(j) for j in jobs]
    ctx = multiprocessing.get_context("spawn")
    with concurrent.futures.ProcessPoolExecutor(max_workers=workers, mp_context=ctx) as pool:
        return list(pool.map(_exact_phase_worker, jobs))
