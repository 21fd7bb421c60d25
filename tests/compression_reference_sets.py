"""The reference's compression sets beside compression_helper.REAL, and their toy twins.

tests/golden/reference_compression_sets.json lists every CompressionParameters constant of the reference; they have
three packing shapes.  compression_helper.REAL is one (base 2^4 x 3 levels); the other two are restated here with their
citations, in compression_helper's own CompressionParams, together with toy twins on compression_helper.TOY_PACK's
small GLWE.  A module of its own, so that tests/test_compression_coverage.py can be dropped next to any version of
compression_helper.py that has REAL and TOY_PACK.
"""
import dataclasses

from .compression_helper import REAL, TOY_PACK, CompressionParams

# shortint/parameters/v1_7/list_compression/p_fail_2_minus_128/mod.rs:40-54
# (V1_7_COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_GAUSSIAN_2M128: base 2^6 x 2 levels, the decomposition of 38 of the 54 sets;
# key noise Gaussian, std 1.34e-7 = 2^41.2 on the 64-bit torus, restated as a TUniform bound of that magnitude — our
# PRNG is not the reference's anyway)
REAL_GAUSSIAN = CompressionParams("COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_GAUSSIAN_2M128", 4, 256, 6, 2, 256, 12, 41)
# shortint/parameters/v0_10/list_compression.rs:7-18 (V0_10_COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M64: 2^4 x 4)
REAL_V0_10 = CompressionParams("V0_10_COMP_PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M64", 4, 256, 4, 4, 256, 12, 42)
REAL_SETS = (REAL, REAL_GAUSSIAN, REAL_V0_10)

# toy twins (2^6 x 2: LEVEL 2 unpadded, the largest base the matrix-core paths take; 2^4 x 4: LEVEL 4 unpadded), and
# 2^7 x 2: one past that base, the scalar kernels
TOY_PACK_B6 = dataclasses.replace(TOY_PACK, name="toy_comp_k2_N64_b6_l2", ks_base_log=6, ks_level=2)
TOY_PACK_L4 = dataclasses.replace(TOY_PACK, name="toy_comp_k2_N64_b4_l4", ks_level=4)
TOY_PACK_B7 = dataclasses.replace(TOY_PACK, name="toy_comp_k2_N64_b7_l2", ks_base_log=7, ks_level=2)
