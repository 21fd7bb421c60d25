"""The multi-bit bootstrap over the 128-bit torus restated in plain Python integers, for tests/test_pbs128_multibit.py.

Restated (tfhe-rs paths): multi-bit key generation (core_crypto/algorithms/lwe_multi_bit_bootstrap_key_generation.rs:
combine_key_bits), the multi-bit modulus switch and the standard-domain blind rotation
(core_crypto/algorithms/lwe_multi_bit_programmable_bootstrapping.rs: std_multi_bit_f128_deterministic_blind_rotate_assign)
with the conventions of oracle/tfhe_oracle_multibit.c.  The key bundle of a group is the exact integer sum
GGSW_0 + sum_{s >= 1} X^{deg_s} GGSW_s modulo 2^128; the external products are the Kronecker big-integer products of
tests/pbs128_helper.py's ExactKey — nothing floating.  Groups are applied in ascending order.

Arrays of u128 words are uint64 arrays with a trailing dimension of 2, (lo, hi), as in pbs128_helper.py.
"""
import concurrent.futures
import dataclasses
import functools
import multiprocessing
import os

import numpy as np

from . import oracle as orc
from . import pbs128_helper as h

U64 = np.uint64


@dataclasses.dataclass(frozen=True)
class ParamsMb128(h.Params128):
    g: int = 2        # grouping factor; the modulus switch is the plain one (ms_type stays 0)

    @property
    def groups(self):
        return self.n // self.g


def mb(name, n, k, N, base_log, level, g):
    return ParamsMb128(name, n, k, N, base_log, level, 0, g=g)


# ------------------------------------------------------------------------------------------------ keys
def combine_key_bits(selector, key_bits, g):
    """lwe_multi_bit_bootstrap_key_generation.rs:504-530: the product over the group of (bit if selected else 1 - bit);
    element m of the group is selected by bit g - 1 - m of the selector"""
    prod = 1
    for m in range(g):
        inv = ((selector >> (g - (m + 1))) & 1) ^ 1
        prod *= int(key_bits[m]) ^ inv
    return prod


@dataclasses.dataclass
class KeysMb128:
    p: ParamsMb128
    lwe_sk: np.ndarray     # n bits
    glwe_sk: np.ndarray    # k * N bits (the output LWE key)
    bsk: np.ndarray        # [n / g][2^g][level][k + 1][k + 1][N][2] uint64


def gen_multi_bit_bsk128(p, lwe_sk, glwe_sk, gen):
    """pbs128_helper.gen_bsk128's GGSW encryption applied to combine_key_bits of each subset of each group, in the
    reference's container order [group][subset][level, index 0 = last level][row][col][N]"""
    per = 1 << p.g
    bits = [combine_key_bits(s, lwe_sk[grp * p.g:(grp + 1) * p.g], p.g) for grp in range(p.groups) for s in range(per)]
    flat = h.gen_bsk128(dataclasses.replace(p, n=len(bits)), np.asarray(bits, dtype=U64), glwe_sk, gen)
    return flat.reshape(p.groups, per, p.level, p.k + 1, p.k + 1, p.N, 2)


@functools.lru_cache(maxsize=6)
def make_keys_mb128(p, seed=0x6D623238, compute=None):
    """compute: a 64-bit parameter set of tests/common.py whose small key the inputs are under; None: a key of its own"""
    rng = orc.Rng(seed)
    lwe_sk = rng.binary_key(p.n)
    if compute is not None:
        from .common import make_keys
        lwe_sk = make_keys(compute).lwe_sk
        assert len(lwe_sk) == p.n
    glwe_sk = rng.binary_key(p.k * p.N)
    gen = np.random.default_rng(int(rng.next()))
    return KeysMb128(p, lwe_sk, glwe_sk, gen_multi_bit_bsk128(p, lwe_sk, glwe_sk, gen))


# ------------------------------------------------------------------------------------------------ modulus switch
def multi_bit_modulus_switch(lwe, log_modulus, g):
    """orc_multi_bit_modulus_switch (oracle/tfhe_oracle_multibit.c:64-81): degrees[group][subset] (subset 0: 0), the
    plain switch of the WRAPPING u64 sum of the subset's mask words; and the plain switch of the body"""
    lwe = [int(v) for v in lwe]
    n = len(lwe) - 1
    degrees = []
    for grp in range(n // g):
        row = [0]
        for s in range(1, 1 << g):
            total = sum(lwe[grp * g + m] for m in range(g) if (s >> (g - (m + 1))) & 1) & h.M64
            row.append(h.modulus_switch(total, log_modulus))
        degrees.append(row)
    return degrees, h.modulus_switch(lwe[n], log_modulus)


# ------------------------------------------------------------------------------------------------ exact bundles
def _neg_pairs(a):
    lo = (~a[..., 0]) + U64(1)
    hi = (~a[..., 1]) + (a[..., 0] == 0).astype(U64)
    return np.stack([lo, hi], axis=-1)


def _add_pairs(a, b):
    lo = a[..., 0] + b[..., 0]
    hi = a[..., 1] + b[..., 1] + (lo < a[..., 0]).astype(U64)
    return np.stack([lo, hi], axis=-1)


def _rotate_pairs(polys, deg, N):
    """[...][N][2] times X^deg modulo X^N + 1 and 2^128, deg < 2 N: an exact integer rotation"""
    r, odd = deg % N, deg >= N
    out = polys
    if r:
        out = np.concatenate([_neg_pairs(polys[..., N - r:, :]), polys[..., :N - r, :]], axis=-2)
    return _neg_pairs(out) if odd else out


def exact_bundle(p, group_key, degrees):
    """group_key [2^g][level][k + 1][k + 1][N][2], degrees of that group -> GGSW_0 + sum_s X^{deg_s} GGSW_s, same shape
    without the subset axis, exact modulo 2^128"""
    with np.errstate(over="ignore"):
        total = np.array(group_key[0], dtype=U64)
        for s in range(1, 1 << p.g):
            total = _add_pairs(total, _rotate_pairs(np.asarray(group_key[s], dtype=U64), degrees[s], p.N))
    return total


# ------------------------------------------------------------------------------------------------ exact bootstrap
@dataclasses.dataclass
class _Bundles:
    bsk: np.ndarray


def bootstrap_exact_multi_bit(p, keys, lwe, lut):
    """modulus switch, LUT * X^-b, then per group in ascending order a FULL external product ACC <- bundle x ACC (the
    digits of the closest representable of ACC itself), sample extraction of coefficient 0.  k N + 1 integers."""
    k, N, L = p.k, p.N, p.level
    degrees, b_hat = multi_bit_modulus_switch(lwe, p.log2N2, p.g)
    acc = [h._monomial_mul(lut[c * N:(c + 1) * N], (2 * N - b_hat) % (2 * N), N) for c in range(k + 1)]
    bundles = np.stack([exact_bundle(p, keys.bsk[grp], degrees[grp]) for grp in range(p.groups)])
    ekey = h.ExactKey(dataclasses.replace(p, n=p.groups), _Bundles(bundles))
    for grp in range(p.groups):
        packed = []
        for row in range(k + 1):
            digs = [h.decompose128(x, p.base_log, L) for x in acc[row]]
            packed.append([ekey.pack_digits([d[idx] for d in digs]) for idx in range(L)])
        new = []
        for col in range(k + 1):
            total = 0
            for row in range(k + 1):
                for idx in range(L):
                    total += packed[row][idx] * ekey.op(grp, idx, row, col)
            new.append(ekey.unpack_negacyclic(total))
        acc = new
    out = []
    for c in range(k):
        out += [acc[c][0]] + [(-acc[c][N - j]) & h.M128 for j in range(1, N)]
    return out + [acc[k][0]]


_worker_state = {}


def _exact_phase_worker(job):
    """one bootstrap in a fresh interpreter (no device, no library of the backend); keys rebuilt from the seed there"""
    p, seed, lwe, lut = job
    if (p, seed) not in _worker_state:
        _worker_state[(p, seed)] = make_keys_mb128(p, seed)
    keys = _worker_state[(p, seed)]
    return h.phase128(p, keys, h.to_pairs(bootstrap_exact_multi_bit(p, keys, lwe, lut)))


def exact_phases_multi_bit(p, lwes, lut, seed=0x6D623238, workers=None):
    """phase under the output key of the exact multi-bit bootstrap of every LWE, spread over spawned child processes (the
    parent may hold a device), as pbs128_helper.exact_phases does"""
    jobs = [(p, seed, np.asarray(lwe), lut) for lwe in lwes]
    workers = workers or max(1, min(8, len(jobs), os.cpu_count() or 1))
    if workers == 1:
        return [_exact_phase_worker(j) for j in jobs]
    ctx = multiprocessing.get_context("spawn")
    with concurrent.futures.ProcessPoolExecutor(max_workers=workers, mp_context=ctx) as pool:
        return list(pool.map(_exact_phase_worker, jobs))
