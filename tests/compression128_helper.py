"""Compression of squashed-noise (128-bit) ciphertext lists: parameter sets, seeded keys and the NumPy / big-integer
restatement the kernels' results are compared with, word for word.

Restated (tfhe-rs paths), sharing no code with the kernels:
  packing keyswitch   core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187 (one LWE), :296-379 (a list)
  compress / extract  core_crypto/entities/compressed_modulus_switched_glwe_ciphertext.rs:171-258 (modulus switch,
                      PackedIntegers over u128 words, extract), with the GPU-side layout of
                      integer/gpu/ciphertext/compressed_noise_squashed_ciphertext_list.rs: every GLWE stores
                      k N + lwe_per_glwe values
  sample extraction   core_crypto/algorithms/glwe_sample_extraction.rs:89-164
The u128 signed decomposer is tests/pbs128_helper.py's (closest_representable_state, decompose128).

A u128 array is a uint64 array with a trailing dimension of 2, (lo, hi).  Values inside the restatement are Python
integers (object arrays).  The sums of decomposed products have two forms here: a plain big-integer one
(decomposed_products_plain, a few thousand products per second) and one on 16-bit limbs through float64 matrix products
(decomposed_products: every limb product is below 2^31 and a sum over K < 2^22 terms stays below 2^53, so every
float64 sum is exact); tests/test_compression128.py checks the second against the first.
"""
import dataclasses

import numpy as np

from . import oracle as orc
from .pbs128_helper import M128, decompose128, from_pairs, to_pairs

U64 = np.uint64


@dataclasses.dataclass(frozen=True)
class Comp128Params:
    name: str
    n_in: int                 # input LWE dimension (the squashing key's k N)
    k: int                    # compression GLWE dimension
    N: int                    # compression polynomial size
    base_log: int             # packing keyswitch decomposition
    level: int
    lwe_per_glwe: int = 0     # 0: N
    storage_log_modulus: int = 128
    pksk_noise: int = 30      # TUniform bound_log2 of a real packing key

    @property
    def per(self):
        return self.lwe_per_glwe or self.N

    @property
    def ncols(self):
        return (self.k + 1) * self.N

    @property
    def lwe_dimension(self):
        return self.k * self.N

    @property
    def values_per_glwe(self):
        return self.k * self.N + self.per

    @property
    def words_per_glwe(self):
        return (self.values_per_glwe * self.storage_log_modulus + 127) // 128

    @property
    def digit_bytes(self):
        return (self.base_log + 1 + 7) // 8

    @property
    def matrix_ok(self):
        """the host shape rule of the matrix-core kernel, restated"""
        K = self.n_in * self.level
        return K % 32 == 0 and self.digit_bytes <= 8 and self.digit_bytes * K * (1 << 14) < (1 << 31)


# the toy sets of the CPU tier (they also run on the device): the three reference decompositions on small GLWEs
SET_A = Comp128Params("toy_A_n64_k1_N32_b61_l1", 64, 1, 32, 61, 1)
SET_B = Comp128Params("toy_B_n64_k2_N16_b33_l2", 64, 2, 16, 33, 2)    # 48 columns: the last column tile is partial
SET_C = Comp128Params("toy_C_n40_k1_N32_b41_l2", 40, 1, 32, 41, 2)    # K = 80: no whole number of matrix steps
SET_D = Comp128Params("toy_D_n64_k1_N32_b16_l8", 64, 1, 32, 16, 8)    # all 128 bits decomposed (rep >= bits)
# more than 32 LWEs in one GLWE need N > 32: the second LWE tile of the matrix-core kernel inside one GLWE
SET_E = Comp128Params("toy_E_n64_k1_N64_b33_l2", 64, 1, 64, 33, 2)
TOYS = [SET_A, SET_B, SET_C, SET_D, SET_E]
# 127 of the 128 bits represented (only base 2^1 x 127 levels gets there): the rounding increment of the closest
# representable meets a word whose 128 bits are all in use
SET_F = Comp128Params("toy_F_n64_k1_N16_b1_l127", 64, 1, 16, 1, 127)

# NOISE_SQUASHING_COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128 and its two siblings
# (shortint/parameters/*/noise_squashing/): the decompositions and GLWE shapes of the three reference sets
REFERENCE_SETS = [
    Comp128Params("ref_b61_l1_k6", 4096, 6, 1024, 61, 1, lwe_per_glwe=128),
    Comp128Params("ref_b41_l2_k6", 4096, 6, 1024, 41, 2, lwe_per_glwe=128),
    Comp128Params("ref_b33_l2_k5", 4096, 5, 1024, 33, 2, lwe_per_glwe=128),
]


# ------------------------------------------------------------------------------------------------ random words, keys
def random_words(rng, *shape):
    """uniform u128 words as uint64 pairs, [*shape][2]"""
    return rng.integers(0, 1 << 64, size=shape + (2,), dtype=U64)


def ints_of(pairs):
    """[..., 2] uint64 -> object array of Python integers"""
    p = np.asarray(pairs, dtype=U64)
    flat = np.array(from_pairs(p.reshape(-1, 2)), dtype=object)
    return flat.reshape(p.shape[:-1])


def pairs_of(ints):
    a = np.asarray(ints, dtype=object)
    return to_pairs(a.reshape(-1).tolist()).reshape(a.shape + (2,))


def negacyclic_matrix(s):
    """M with  a @ M = a * s  in Z[X]/(X^N + 1): M[i][p] = s[p - i] (p >= i), -s[N + p - i] (p < i); s: bits"""
    N = len(s)
    s = np.array([int(b) for b in s], dtype=object)
    i, p = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    pos = s[(p - i) % N]
    return np.where(p >= i, pos, -pos)


def gen_pksk128(seed, sk_in, glwe_sk, cp):
    """lwe_packing_keyswitch_key_generation.rs over u128: row (j, idx) is a GLWE encryption, under the compression key,
    of sk_in[j] * 2^(128 - base_log * (level - idx)) at coefficient 0 (row idx holds level (level - idx)), uniform masks,
    TUniform(pksk_noise) noise.  Returns [n_in * level][(k + 1) N][2] uint64."""
    rng = np.random.default_rng(seed)
    rows = cp.n_in * cp.level
    mask = ints_of(random_words(rng, rows, cp.k * cp.N))
    noise = rng.integers(-(1 << cp.pksk_noise), (1 << cp.pksk_noise) + 1, size=(rows, cp.N), dtype=np.int64)
    body = noise.astype(object)
    for q in range(cp.k):
        body = body + mask[:, q * cp.N:(q + 1) * cp.N].dot(negacyclic_matrix(glwe_sk[q * cp.N:(q + 1) * cp.N]))
    for j in range(cp.n_in):
        for idx in range(cp.level):
            body[j * cp.level + idx, 0] += int(sk_in[j]) << (128 - cp.base_log * (cp.level - idx))
    key = np.concatenate([mask, body], axis=1)
    return pairs_of(np.vectorize(lambda v: v & M128, otypes=[object])(key))


def compression_secret_key(cp, seed=0x63703132):
    return orc.Rng(seed).binary_key(cp.k * cp.N)


# ------------------------------------------------------------------------------------------------ the restatement
def digits_of(lwes, cp):
    """[count][n_in + 1][2] -> int64 [count][n_in * level]: digit idx of mask element j at K = j * level + idx, least
    significant first (the key's row order)"""
    masks = ints_of(np.asarray(lwes)[:, :cp.n_in])
    out = np.empty((masks.shape[0], cp.n_in * cp.level), dtype=np.int64)
    for i, row in enumerate(masks.tolist()):
        out[i] = [d for x in row for d in decompose128(x, cp.base_log, cp.level)]
    return out


def decomposed_products_plain(lwes, key, cp):
    """-sum_K digit * key word modulo 2^128, plain big integers: object array [count][ncols]"""
    d = digits_of(lwes, cp).astype(object)
    return np.vectorize(lambda v: (-v) & M128, otypes=[object])(d.dot(ints_of(key).reshape(-1, cp.ncols)))


def _limb_sums(digits, key_cols):
    """digits int64 [count][K], key_cols uint64 [K][cols][2] -> object array [count][cols] of sum_K digit * word mod 2^128"""
    count, K = digits.shape
    cols = key_cols.shape[1]
    assert K < (1 << 22)
    d = digits.copy()
    dl = np.empty((count, 4, K), dtype=np.float64)   # four balanced 16-bit limbs of a digit below 2^62 in magnitude
    for a in range(4):
        limb = ((d + (1 << 15)) & 0xFFFF) - (1 << 15)
        dl[:, a, :] = limb
        d = (d - limb) >> 16
    assert not d.any()
    kl = np.ascontiguousarray(key_cols).view(np.uint16).reshape(K, cols * 8).astype(np.float64)
    sums = (dl.reshape(count * 4, K) @ kl).reshape(count, 4, cols, 8)
    assert np.abs(sums).max(initial=0) < (1 << 53)
    sums = sums.astype(np.int64).astype(object)
    total = np.zeros((count, cols), dtype=object)
    for a in range(4):
        for b in range(8 - a):   # limbs with a + b >= 8 vanish modulo 2^128
            total = total + sums[:, a, :, b] * (1 << (16 * (a + b)))
    return total


def decomposed_products(lwes, key, cp):
    """the same words as decomposed_products_plain, on 16-bit limbs"""
    total = _limb_sums(digits_of(lwes, cp), np.asarray(key, dtype=U64).reshape(-1, cp.ncols, 2))
    return np.vectorize(lambda v: (-v) & M128, otypes=[object])(total)


def pack_rows(rows, bodies, cp, per):
    """rows: object [count][ncols] (decomposed products), bodies: the input bodies; chunk by chunk
    G_i = rows_i + b_i X^0 in the body polynomial, out = sum_i X^i G_i: object [glwes][ncols]"""
    out = []
    for c0 in range(0, len(rows), per):
        acc = np.zeros((cp.k + 1, cp.N), dtype=object)
        for i in range(min(per, len(rows) - c0)):
            g = rows[c0 + i].reshape(cp.k + 1, cp.N).copy()
            g[cp.k, 0] += int(bodies[c0 + i])
            r = np.roll(g, i, axis=1)   # times the monic monomial X^i, negacyclic
            r[:, :i] = -r[:, :i]
            acc = acc + r
        out.append(np.vectorize(lambda v: v & M128, otypes=[object])(acc.reshape(-1)))
    return np.stack(out)


def packing_keyswitch(lwes, key, cp, per=None, rows=None):
    """LWE list -> GLWEs as object arrays [glwes][ncols]; rows: decomposed_products(lwes, ...) when already computed"""
    lwes = np.asarray(lwes, dtype=U64)
    rows = decomposed_products(lwes, key, cp) if rows is None else rows
    bodies = from_pairs(lwes[:, cp.n_in])
    return pack_rows(rows[:len(lwes)], bodies, cp, per or cp.per)


def modulus_switch128(x, s):
    return x if s == 128 else ((x + (1 << (127 - s))) & M128) >> (128 - s)


def bit_pack128(values, s):
    """s bits per value, least significant first, into ceil(len * s / 128) u128 words: [words][2] uint64"""
    big = 0
    for t, v in enumerate(values):
        assert 0 <= v < (1 << s)
        big |= v << (t * s)
    words = (len(values) * s + 127) // 128
    return to_pairs([(big >> (128 * w)) & M128 for w in range(words)])


def bit_unpack128(words, s, count):
    big = sum(v << (128 * w) for w, v in enumerate(from_pairs(words)))
    return [(big >> (t * s)) & ((1 << s) - 1) for t in range(count)]


def compress(blocks, key, cp, rows=None):
    """[blocks][n_in + 1][2] -> packed words [glwes * words_per_glwe][2]; no multiplication by message_modulus"""
    glwes = packing_keyswitch(blocks, key, cp, cp.per, rows)
    s = cp.storage_log_modulus
    return np.concatenate([bit_pack128([modulus_switch128(int(v), s) for v in g[:cp.values_per_glwe]], s) for g in glwes])


def extract_glwe(packed, cp, glwe_index, total_blocks):
    """GLWE glwe_index of the packed list as ncols Python integers: values scaled back up, the body tail zero"""
    s = cp.storage_log_modulus
    words = np.asarray(packed, dtype=U64).reshape(-1, 2)[glwe_index * cp.words_per_glwe:(glwe_index + 1) * cp.words_per_glwe]
    bodies = min(cp.per, total_blocks - glwe_index * cp.per)
    count = cp.k * cp.N + bodies
    return [(v << (128 - s)) & M128 for v in bit_unpack128(words, s, count)] + [0] * (cp.ncols - count)


def sample_extract(glwe, cp, nth):
    out = []
    for q in range(cp.k):
        poly = glwe[q * cp.N:(q + 1) * cp.N]
        out += [poly[nth - j] if j <= nth else (-poly[cp.N + nth - j]) & M128 for j in range(cp.N)]
    return out + [glwe[cp.k * cp.N + nth]]


def extract_lwes(packed, cp, indexes, total_blocks):
    """[len(indexes)][k N + 1][2] uint64"""
    return np.stack([to_pairs(sample_extract(extract_glwe(packed, cp, int(t) // cp.per, total_blocks), cp, int(t) % cp.per))
                     for t in indexes])


def phase(lwe_pairs, sk):
    v = from_pairs(lwe_pairs)
    return (v[-1] - sum(a for a, s in zip(v[:-1], sk.tolist()) if s)) & M128


# ------------------------------------------------------------------------------------------------ selected values of big GLWEs
def glwe_values(lwes, key, cp, first, count, values):
    """Values `values` of the GLWE that packs LWEs [first, first + count): value v = (q, p) needs column
    q N + (p - i) mod N of LWE i's decomposed products, so only those columns of the key are read."""
    lwes = np.asarray(lwes, dtype=U64)[first:first + count]
    digits = digits_of(lwes, cp)
    key = np.asarray(key, dtype=U64).reshape(-1, cp.ncols, 2)
    bodies = from_pairs(lwes[:, cp.n_in])
    out = [0] * len(values)
    for i in range(count):
        cols = [(v // cp.N) * cp.N + ((v % cp.N - i) % cp.N) for v in values]
        g = _limb_sums(digits[i:i + 1], key[:, cols])[0]
        for t, v in enumerate(values):
            q, p = divmod(v, cp.N)
            x = -int(g[t]) + (bodies[i] if q == cp.k and (p - i) % cp.N == 0 else 0)
            out[t] += x if p >= i else -x
    return [v & M128 for v in out]
