"""Ciphertext compression: parameter sets, seeded keys and the NumPy restatement the GPU results are compared with.

The restatement follows the reference CPU algorithms step by step and shares no code with the kernels:
  packing keyswitch   core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187 (one LWE), :296-379 (a list)
  compress            shortint/list_compression/compression.rs:17-133
  bit packing         core_crypto/entities/compressed_modulus_switched_glwe_ciphertext.rs:171-250 (PackedIntegers)
  decompress          shortint/list_compression/compression.rs:137-254
It uses the C oracle for what the oracle already restates (the decomposed products of a keyswitch, sample extraction,
the bootstrap) and plain Python integers for the bit packing.
"""
import dataclasses
import functools

import numpy as np

from . import oracle as orc

U64 = np.uint64
M64 = (1 << 64) - 1


@dataclasses.dataclass(frozen=True)
class CompressionParams:
    name: str
    k: int                    # compression GLWE dimension
    N: int                    # compression polynomial size
    ks_base_log: int          # packing keyswitch decomposition
    ks_level: int
    lwe_per_glwe: int
    storage_log_modulus: int
    pksk_noise: int           # TUniform bound_log2 of the packing key

    @property
    def ncols(self):
        return (self.k + 1) * self.N

    @property
    def lwe_dimension(self):
        return self.k * self.N

    @property
    def values_per_glwe(self):
        return self.k * self.N + self.lwe_per_glwe

    @property
    def words_per_glwe(self):
        return (self.values_per_glwe * self.storage_log_modulus + 63) // 64


# shortint/parameters/v1_7/list_compression/p_fail_2_minus_128/mod.rs:11-37 (COMP_PARAM_MESSAGE_2_CARRY_2: packing
# keyswitch base 2^4 x 3 levels, GLWE 4 x 256, 256 LWEs per GLWE, 12 bits stored, key noise TUniform 2^43)
REAL = CompressionParams("COMP_PARAM_MESSAGE_2_CARRY_2", 4, 256, 4, 3, 256, 12, 43)

# word-for-word tests on the CPU tier (no noise budget needed): the real decomposition on a small GLWE, a second
# decomposition without level padding and with a base the matrix-core path declines, fewer LWEs per GLWE than
# coefficients, and a storage width that divides 64
TOY_PACK = CompressionParams("toy_comp_k2_N64", 2, 64, 4, 3, 64, 12, 30)
TOY_PACK_B8 = dataclasses.replace(TOY_PACK, name="toy_comp_k2_N64_b8_l2", ks_base_log=8, ks_level=2)
TOY_PACK_PAD = dataclasses.replace(TOY_PACK, name="toy_comp_k2_N64_37_per_glwe", lwe_per_glwe=37)   # 165 values * 12 bits: padding
TOY_PACK_STRIDED = dataclasses.replace(TOY_PACK, name="toy_comp_k2_N64_40_per_glwe_16_bits", lwe_per_glwe=40,
                                       storage_log_modulus=16)

# decrypting tests on the CPU tier (input dimension 2048, compute set TOY_2048 / TOY_MB4_2048: delta = 2^59, the half
# box of the rescaling table is 2^60).  WORST-CASE bound on the phase error in front of the decompression bootstrap's
# blind rotation, with binary keys:
#   input blocks                   post-bootstrap error of the toy compute sets <= 12 * (k+1) N 2^22 2^17 < 2^55,
#                                  times message_modulus = 4                                              < 2^57
#   decomposition rounding         2048 coefficients * 2^(63 - 8*3)                                        = 2^50
#   packing key noise              16 LWEs * 2048 * 3 levels * 2^7 (digit) * 2^20                          < 2^44
#   modulus switch to 12 bits      (k N + 1) * 2^51 = 33 * 2^51                                            < 2^56.1
#   bootstrap's switch to 2N=2^12  (k N + 1) * 2^51                                                        < 2^56.1
#   sum                                                                                                    < 2^58.3  < 2^60
# (base 2^4 x 3 levels would allow 2048 * 2^51 = 2^62 of rounding alone: the real decomposition relies on the average)
TOY_DEC = CompressionParams("toy_comp_k2_N16_b8_l3", 2, 16, 8, 3, 16, 12, 20)


@dataclasses.dataclass
class CompressionKeys:
    cp: CompressionParams
    glwe_sk: np.ndarray       # k * N bits: the compression key, flattened = the decompression bootstrap's input key
    pksk: np.ndarray          # [n_in][level][(k+1) N]


def negacyclic_matrix(s):
    """M with  a @ M = a * s  in Z[X]/(X^N + 1), wrapping u64: M[i][p] = s[p - i] (p >= i), -s[N + p - i] (p < i)."""
    N = len(s)
    s = np.asarray(s, dtype=U64)
    i, p = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    pos = s[(p - i) % N]
    return np.where(p >= i, pos, (U64(0) - pos))


def tuniform(rng, bound_log2, size):
    return rng.integers(-(1 << bound_log2), (1 << bound_log2) + 1, size=size, dtype=np.int64).astype(U64)


def gen_pksk(seed, sk_in, glwe_sk, cp):
    """lwe_packing_keyswitch_key_generation.rs: row (j, idx) is a GLWE encryption, under the compression key, of
    sk_in[j] * 2^(64 - base_log * (level - idx)) at coefficient 0 — row idx holds level (level - idx), the order of
    the LWE keyswitch key (oracle/tfhe_oracle.c:359-373)."""
    rng = np.random.default_rng(seed)
    n_in, rows = len(sk_in), len(sk_in) * cp.ks_level
    key = np.zeros((rows, cp.ncols), dtype=U64)
    key[:, :cp.k * cp.N] = rng.integers(0, 1 << 64, size=(rows, cp.k * cp.N), dtype=U64)
    body = tuniform(rng, cp.pksk_noise, (rows, cp.N))
    for q in range(cp.k):
        body = body + key[:, q * cp.N:(q + 1) * cp.N] @ negacyclic_matrix(glwe_sk[q * cp.N:(q + 1) * cp.N])
    for idx in range(cp.ks_level):
        shift = 64 - cp.ks_base_log * (cp.ks_level - idx)
        body[idx::cp.ks_level, 0] += np.asarray(sk_in, dtype=U64) << U64(shift)
    key[:, cp.k * cp.N:] = body
    assert key.shape[0] == n_in * cp.ks_level
    return key.reshape(-1)


_key_cache = {}


def make_compression_keys(cp, sk_in, seed=0x636F6D70):
    """Keys from seeds; sk_in: the big compute key (k*N bits of the compute GLWE key)."""
    ident = (cp, seed, sk_in.tobytes())
    if ident not in _key_cache:
        if len(_key_cache) >= 4:
            _key_cache.clear()
        glwe_sk = orc.Rng(seed).binary_key(cp.k * cp.N)
        _key_cache[ident] = CompressionKeys(cp, glwe_sk, gen_pksk(seed + 1, sk_in, glwe_sk, cp))
    return _key_cache[ident]


@functools.lru_cache(maxsize=2)
def _dbsk_cached(cp, p, seed, comp_sk_bytes, glwe_sk_bytes):
    comp_sk = np.frombuffer(comp_sk_bytes, dtype=U64)
    glwe_sk = np.frombuffer(glwe_sk_bytes, dtype=U64)
    if p.grouping:
        return orc.gen_multi_bit_bsk(seed, comp_sk, glwe_sk, p.k, p.N, p.pbs_base_log, p.pbs_level, p.grouping, p.glwe_noise)
    return orc.gen_bsk(seed, comp_sk, glwe_sk, p.k, p.N, p.pbs_base_log, p.pbs_level, p.glwe_noise)


def gen_decompression_bsk(cp, ckeys, p, keys, seed=0x64636D70):
    """The decompression key: a bootstrap key (classic or multi-bit, by p.grouping) from the flattened compression key
    to the compute GLWE key, standard domain."""
    return _dbsk_cached(cp, p, seed, ckeys.glwe_sk.tobytes(), np.ascontiguousarray(keys.glwe_sk, dtype=U64).tobytes())


# ----------------------------------------------------------------------------------------------- the restatement
def packing_keyswitch(lwes, pksk, n_in, cp, lwe_per_glwe=None):
    """LWE list -> GLWEs, chunk by chunk:  G_i = (0, ..., 0, b_i X^0) - sum_j sum_idx digit_idx(a_i[j]) K[j][idx],
    out = sum_i X^i G_i."""
    lwes = np.ascontiguousarray(lwes, dtype=U64).reshape(-1, n_in + 1)
    per = lwe_per_glwe or cp.lwe_per_glwe
    # the decomposed products: the LWE keyswitch with (k+1) N columns; it puts the body in the last column
    rows = orc.keyswitch_batch(lwes, pksk, n_in, cp.ncols - 1, cp.ks_base_log, cp.ks_level)
    rows[:, cp.ncols - 1] -= lwes[:, n_in]
    rows[:, cp.k * cp.N] += lwes[:, n_in]
    out = []
    for c0 in range(0, len(lwes), per):
        acc = np.zeros((cp.k + 1, cp.N), dtype=U64)
        for i, g in enumerate(rows[c0:c0 + per]):
            r = np.roll(g.reshape(cp.k + 1, cp.N), i, axis=1)   # times the monic monomial X^i, negacyclic
            r[:, :i] = U64(0) - r[:, :i]
            acc += r
        out.append(acc.reshape(-1))
    return np.stack(out)


def modulus_switch(x, s):
    x = np.asarray(x, dtype=U64)
    return (x + U64(1 << (63 - s))) >> U64(64 - s)


def bit_pack(values, s):
    """s bits per value, least significant first, into ceil(len * s / 64) words"""
    big = 0
    for t, v in enumerate(values):
        assert 0 <= int(v) < (1 << s)
        big |= int(v) << (t * s)
    words = (len(values) * s + 63) // 64
    return np.array([(big >> (64 * w)) & M64 for w in range(words)], dtype=U64)


def bit_unpack(words, s, count):
    big = 0
    for w, x in enumerate(words):
        big |= int(x) << (64 * w)
    return np.array([(big >> (t * s)) & ((1 << s) - 1) for t in range(count)], dtype=U64)


def compress(blocks, pksk, n_in, cp, message_modulus):
    """[blocks][n_in + 1] -> packed words, [glwe][words_per_glwe] flattened"""
    blocks = np.ascontiguousarray(blocks, dtype=U64).reshape(-1, n_in + 1)
    glwes = packing_keyswitch(blocks * U64(message_modulus), pksk, n_in, cp)
    return np.concatenate([bit_pack(modulus_switch(g[:cp.values_per_glwe], cp.storage_log_modulus),
                                    cp.storage_log_modulus) for g in glwes])


def extract_glwe(packed, cp, glwe_index, total_blocks):
    """GLWE glwe_index of the packed list: values shifted back up, the body tail beyond its count zero"""
    s = cp.storage_log_modulus
    words = np.asarray(packed, dtype=U64)[glwe_index * cp.words_per_glwe:(glwe_index + 1) * cp.words_per_glwe]
    bodies = min(cp.lwe_per_glwe, total_blocks - glwe_index * cp.lwe_per_glwe)
    out = np.zeros(cp.ncols, dtype=U64)
    count = cp.k * cp.N + bodies
    out[:count] = bit_unpack(words, s, count) << U64(64 - s)
    return out


def extract_lwes(packed, cp, indexes, total_blocks):
    return np.stack([orc.sample_extract(extract_glwe(packed, cp, t // cp.lwe_per_glwe, total_blocks), cp.k, cp.N,
                                        t % cp.lwe_per_glwe) for t in indexes])


def rescaling_lut(p, message_modulus, carry_modulus):
    """compression.rs:137-162: the identity from plaintext modulus msg * carry / msg (carry space 1) to (msg, carry)"""
    return orc.generate_lut(p.k, p.N, message_modulus * carry_modulus // message_modulus,
                            (1 << 63) // (message_modulus * carry_modulus), lambda x: x)


def decompress(packed, cp, indexes, total_blocks, dbsk, p, message_modulus, carry_modulus):
    """the project's oracle bootstrap (f64 engine, fixed order) of the restated extracted LWEs"""
    lwes = extract_lwes(packed, cp, indexes, total_blocks)
    lut = rescaling_lut(p, message_modulus, carry_modulus)
    n = cp.lwe_dimension
    if p.grouping:
        return orc.pbs_multi_bit(orc.ENGINE_FFT, lwes, lut, dbsk, n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.grouping)
    bsk_f = orc.convert_bsk_fft(dbsk, n, p.k, p.N, p.pbs_level)
    return orc.pbs_batch(orc.ENGINE_FFT, lwes, lut, bsk_f, n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ms_type)
