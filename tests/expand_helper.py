"""Compact ciphertext lists for the expansion tests: a NumPy restatement of the CPU expansion in its index form
(tfhe/src/core_crypto/algorithms/lwe_compact_ciphertext_list_expansion.rs over polynomial_wrapping_monic_monomial_mul),
and a fixture builder that makes compact lists straight from the secret key, with no public key and no noise, so that
every expanded LWE decrypts EXACTLY to its encoded message."""
import numpy as np

from . import oracle as orc

U64 = np.uint64
MSG = 4                      # message_modulus = carry_modulus = 4
DELTA = (1 << 63) // 16      # the four bits below the padding bit


def rotate_mask(mask, d):
    """mask * X^d in Z[X]/(X^n + 1):  out[(j + d) mod n] = mask[j] if j + d < n, -mask[j] otherwise (modulo 2^64)."""
    mask = np.ascontiguousarray(mask, dtype=U64)
    n = mask.size
    j = np.arange(n)
    out = np.empty(n, dtype=U64)
    out[(j + d) % n] = np.where(j + d < n, mask, U64(0) - mask)
    return out


def expand(words, n_c, counts):
    """The flattened lists (per list n_c mask words, then its bodies) -> [sum(counts)][n_c + 1] LWEs."""
    words = np.ascontiguousarray(words, dtype=U64)
    rows, at = [], 0
    for c in counts:
        mask, bodies = words[at:at + n_c], words[at + n_c:at + n_c + c]
        for d in range(c):
            rows.append(np.concatenate([rotate_mask(mask, d), bodies[d:d + 1]]))
        at += n_c + c
    assert at == words.size
    return np.stack(rows)


def pack(message, second):
    return int(message) + MSG * int(second)


def make_compact_list(sk, packed_values, seed, delta=DELTA):
    """One compact list under the binary key `sk`: a random mask, and for body d the word <mask * X^d, sk> + delta * m."""
    n_c = len(sk)
    assert 1 <= len(packed_values) <= n_c
    mask = np.random.default_rng(seed).integers(0, 1 << 64, size=n_c, dtype=U64)
    ones = np.asarray(sk, dtype=U64) == 1
    bodies = [(int(rotate_mask(mask, d)[ones].sum(dtype=U64)) + delta * int(m)) % (1 << 64)
              for d, m in enumerate(packed_values)]
    return np.concatenate([mask, np.array(bodies, dtype=U64)])


def make_flattened(sk, lists, seed, delta=DELTA):
    """`lists`: per compact list its packed values -> (flattened words, counts)"""
    words = [make_compact_list(sk, vals, seed + 17 * i, delta) for i, vals in enumerate(lists)]
    return np.concatenate(words), [len(v) for v in lists]


def pke_key(n_c, seed=0x706B65):
    return orc.Rng(seed).binary_key(n_c)


def casting_key(seed, sk_in, sk_out, base_log, level, noise_log2):
    """[n_in][level][n_out + 1]: the oracle's keyswitch-key generator from the encryption key to a compute key"""
    return orc.gen_ksk(seed, sk_in, sk_out, base_log, level, noise_log2)
