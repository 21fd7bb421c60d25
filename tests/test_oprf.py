"""Oblivious pseudo-random bits (hip_*_integer_grouped_oprf_64): every block against the reference's clear-text model of
the encrypted function (tests/oprf_helper.py cleartext_prf) on inputs whose clear value is known exactly, degrees, empty
carries, determinism, the refusal of a block count that does not match the bit count, sharding over a stream set, and
the re-randomisation of the fresh blocks.  [emu] runs the kernel sources on the host with toy keys, [hip] on the MI355X,
there also with PARAM_MESSAGE_2_CARRY_2."""
import textwrap

import numpy as np
import pytest

from . import oprf_helper as oh
from .common import C1, TOY_2048, TOY_MB4_2048, decrypt_big
from .harness import use_backend
from .test_error_behaviour import run as run_child
from .test_radix_integer import setup as radix_setup

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
MSG = 4
MESSAGE_BITS = 2
OUTPUT_MODULUS = 2 * MSG * MSG    # padding bit included

SETS = [pytest.param("emu", TOY_2048, id="emu-toy_classic"), pytest.param("emu", TOY_MB4_2048, id="emu-toy_multi_bit_g4"),
        pytest.param("hip", TOY_2048, id="hip-toy_classic", marks=pytest.mark.gpu),
        pytest.param("hip", TOY_MB4_2048, id="hip-toy_multi_bit_g4", marks=pytest.mark.gpu),
        pytest.param("hip", C1, id="hip-message_2_carry_2", marks=pytest.mark.gpu)]
# (total_random_bits, blocks): full blocks; a last block of one bit; a single block of one bit
SHAPES = [(8, 4), (7, 4), (1, 1)]
# Input seeds per key set, fixed so that the clear inputs reach both halves of the negacyclic range (x < N reads the
# table, x >= N its negation): one seed for the four-block shapes, a pair for the single block.  The test asserts it.
SEEDS = {
    TOY_2048.name: {4: [400], 1: [400, 402]},
    TOY_MB4_2048.name: {4: [400], 1: [400, 401]},
    C1.name: {4: [400], 1: [400, 403]},
}


def generate(p, st, sks, igpu, lwes, total_random_bits, rerand=None):
    return igpu.CudaOprfServerKey(sks.bootstrapping_key).generate_oblivious_pseudo_random_bits(
        lwes, total_random_bits, sks, st, rerand=rerand)


def expected(p, keys, lwes, total_random_bits):
    """(clear inputs, bits per block, expected block values)"""
    xs = oh.input_cleartexts(lwes, keys.lwe_sk, p.N)
    bits = oh.bits_per_block(total_random_bits, len(xs), MESSAGE_BITS)
    return xs, bits, [oh.cleartext_prf(x, b, OUTPUT_MODULUS, p.N) for x, b in zip(xs, bits)]


# ------------------------------------------------------------------------------------------ 7. exact expectation
@pytest.mark.parametrize("total_random_bits,blocks", SHAPES, ids=[f"{t}_bits_over_{b}" for t, b in SHAPES])
@pytest.mark.parametrize("kind,p", SETS)
def test_every_block_holds_the_clear_prf_of_its_input(kind, p, total_random_bits, blocks):
    p, keys, st, sks, igpu = radix_setup(kind, p)
    halves = set()
    for seed in SEEDS[p.name][blocks]:
        lwes = oh.seeded_lwes(p.n, p.N, blocks, seed)
        xs, bits, want = expected(p, keys, lwes, total_random_bits)
        halves |= {x >= p.N for x in xs}
        out = generate(p, st, sks, igpu, lwes, total_random_bits)
        assert out.num_integers == 1 and out.num_blocks == blocks and out.lwe_dimension == p.big_n
        words = out.to_blocks(st)[0]
        got = [decrypt_big(p, keys, b) for b in words]
        print(p.name, "inputs", xs, "bits", bits, "decrypted", got)
        assert got == want
        assert all(0 <= v < (1 << b) for v, b in zip(got, bits))
        assert all(v >> MESSAGE_BITS == 0 for v in got), "carry bits set"
        assert list(out.degrees) == [(1 << b) - 1 for b in bits]
        assert list(out._info[1]) == [1] * blocks        # nominal noise level
        again = generate(p, st, sks, igpu, lwes, total_random_bits).to_blocks(st)[0]
        assert np.array_equal(again, words), "the same input gave other words"
    assert halves == {False, True}, "the inputs do not reach both halves of the negacyclic range"


# ------------------------------------------------------------------------------------------ 8. refusal, sharding, rerand
OPRF_PRELUDE = """
from tfhe_rs_amd import integer_gpu as igpu
s, keep = igpu.CudaServerKey._streams(st)
mem = C.c_void_p()
BK, KK = ffi.CudaLweBootstrapKeyParamsFFI, ffi.CudaLweKeyswitchKeyParamsFFI
def scratch(blocks, bits, msg=4, carry=4, allocate=True):
    return lib.hip_scratch_integer_grouped_oprf_64_async(s, C.byref(mem), BK(12, 1, 2048, 23, 1, 2048, 1, 0),
                                                         KK(2048, 12, 4, 4), blocks, msg, carry, allocate, bits, 0)
"""

REFUSALS = {
    "fewer blocks than the bits need": ("scratch(3, 8)", "num_blocks_to_process (3) should be equal to"),
    "more blocks than the bits need": ("scratch(4, 6)", "num_blocks_to_process (4) should be equal to"),
    "no bits": ("scratch(0, 0)", "num_blocks_to_process (0) should be equal to"),
    "a launch with another block count": ("""
        scratch(4, 8)
        v = gpu.CudaVec(4 * 2049, st)
        ct = igpu.CudaUnsignedRadixCiphertext(v, 1, 4, 2048)
        keys = (C.c_void_p * 1)(v.ptr)
        lib.hip_integer_grouped_oprf_64_async(s, C.byref(ct._ffi()), v.ptr, 3, mem, keys)
        """, "3 blocks to process on a scratch created for 4"),
    "a launch on a size-only scratch": ("""
        scratch(4, 8, allocate=False)
        v = gpu.CudaVec(4 * 2049, st)
        ct = igpu.CudaUnsignedRadixCiphertext(v, 1, 4, 2048)
        keys = (C.c_void_p * 1)(v.ptr)
        lib.hip_integer_grouped_oprf_64_async(s, C.byref(ct._ffi()), v.ptr, 4, mem, keys)
        """, "scratch was created with allocate_gpu_memory=false"),
}


@pytest.mark.parametrize("name", list(REFUSALS), ids=[n.replace(" ", "_") for n in REFUSALS])
def test_oprf_misuse_aborts_with_a_message_naming_the_entry_point(name):
    snippet, message = REFUSALS[name]
    r = run_child(OPRF_PRELUDE + textwrap.dedent(snippet))
    assert r.returncode != 0, f"{name}: the call was accepted"
    assert message in r.stderr and "integer_grouped_oprf" in r.stderr, r.stderr[-600:]


@pytest.mark.parametrize("kind", BACKENDS)
def test_bootstrap_shards_over_a_two_entry_stream_set(kind):
    """Two streams of device 0 and one block per GPU from which a round spreads: the four blocks travel 2 + 2, each
    half with the key replica of its stream.  Same words as one stream."""
    lwes = oh.seeded_lwes(TOY_2048.n, TOY_2048.N, 4, 400)
    p, keys, st, sks, igpu = radix_setup(kind, TOY_2048)
    one = generate(p, st, sks, igpu, lwes, 7).to_blocks(st)
    p, keys, st2, sks2, igpu = radix_setup(kind, TOY_2048, gpu_indexes=(0, 0))
    lib = use_backend(kind)
    lib.hip_integer_set_multi_gpu_threshold(1)
    try:
        two = generate(p, st2, sks2, igpu, lwes, 7).to_blocks(st2)
    finally:
        lib.hip_integer_set_multi_gpu_threshold(0)
    assert np.array_equal(one, two)
    assert [decrypt_big(p, keys, b) for b in two[0]] == expected(p, keys, lwes, 7)[2]


@pytest.mark.parametrize("mode", ["without_ks", "with_ks"])
@pytest.mark.parametrize("kind", BACKENDS)
def test_oprf_followed_by_re_randomisation_keeps_the_values(kind, mode):
    from .test_rerand import rerand_key_and_zeros
    p, keys, st, sks, igpu = radix_setup(kind, TOY_2048)
    lwes = oh.seeded_lwes(p.n, p.N, 4, 400)
    _, bits, want = expected(p, keys, lwes, 7)
    plain = generate(p, st, sks, igpu, lwes, 7).to_blocks(st)[0]
    key, zeros = rerand_key_and_zeros(p, keys, igpu, st, mode, 4, 308)
    out = generate(p, st, sks, igpu, lwes, 7, rerand=(zeros, key))
    words = out.to_blocks(st)[0]
    assert [decrypt_big(p, keys, b) for b in words] == want
    assert (words != plain).all(), "the blocks were not re-randomised"
    assert list(out.degrees) == [(1 << b) - 1 for b in bits] and list(out._info[1]) == [1] * 4
