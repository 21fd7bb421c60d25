"""Oblivious pseudo-random bits for the OPRF tests: a restatement of the reference's clear-text model of the encrypted
function (tfhe/src/shortint/oprf.rs cleartext_prf), the seeded inputs as the reference shapes them (every word a multiple
of 2^64 / 2N, so that the modulus switch in front of the blind rotation is exact), and the clear input such an LWE holds."""
import numpy as np

from . import oracle as orc

U64 = np.uint64


def cleartext_prf(input_cleartext, random_bits_count, output_modulus, prf_polynomial_size):
    """The value the encrypted PRF gives for the clear input x in [0, 2N): output_modulus contains the padding bit (32 for
    two message and two carry bits).  The first half of the negacyclic range reads the table, the second half its negation;
    the correction (2^bits - 1) / 2 (in units of delta) lifts both into [0, 2^bits)."""
    input_modulus = 2 * prf_polynomial_size
    random_value_modulus = 1 << random_bits_count
    poly_delta = 2 * prf_polynomial_size // random_value_modulus

    def half_negacyclic_part(x):
        return 2 * (x // poly_delta) + 1

    assert 0 <= input_cleartext < input_modulus
    if input_cleartext < input_modulus // 2:
        part = half_negacyclic_part(input_cleartext)
    else:
        part = 2 * output_modulus - half_negacyclic_part(input_cleartext - input_modulus // 2)
    a = (part + random_value_modulus - 1) % (2 * output_modulus)
    assert a % 2 == 0
    return a // 2


def seeded_lwes(n, N, blocks, seed):
    """[blocks][n + 1] words as a seed would give them after the reference's shaping: uniform multiples of 2^64 / 2N."""
    log2_2n = (2 * N).bit_length() - 1
    words = np.random.default_rng(seed).integers(0, 2 * N, size=(blocks, n + 1), dtype=U64)
    return words << U64(64 - log2_2n)


def input_cleartexts(lwes, sk, N):
    """(body - <mask, s>) mod 2^64 >> (64 - log2 2N) per LWE: exact, every word being a multiple of 2^64 / 2N."""
    log2_2n = (2 * N).bit_length() - 1
    out = []
    for lwe in lwes:
        phase = int(orc.lwe_decrypt(lwe, sk))
        assert phase % (1 << (64 - log2_2n)) == 0
        out.append(phase >> (64 - log2_2n))
    return out


def bits_per_block(total_random_bits, blocks, message_bits):
    out = [min(message_bits, total_random_bits - i * message_bits) for i in range(blocks)]
    assert all(b >= 1 for b in out) and sum(out) == total_random_bits
    return out
