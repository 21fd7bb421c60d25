"""Host-side mirror of tfhe/src/integer/gpu for the radix operations the backend wires ("next" row N1):
CudaServerKey (keys + parameters on the device), CudaUnsignedRadixCiphertext (here: a BATCH of
integers, [integer][block] on the device) and the operations

    unchecked_add_assign / add_assign   integer/gpu/server_key/radix/add.rs
    propagate_single_carry_assign       integer/gpu/mod.rs (cuda_backend_propagate_single_carry_assign)
    mul_assign                          integer/gpu/server_key/radix/mul.rs
    apply_lookup_table                  integer/gpu/mod.rs (cuda_backend_apply_univariate_lut)

Each call is scratch -> launch -> cleanup through the C ABI, as the Rust wrappers do
(integer/gpu/mod.rs).  No CPU fallback: everything runs in libtfhe_hip_backend.so.
"""
import ctypes as C

import numpy as np

from . import ffi
from .core_crypto_gpu import (CudaLweBootstrapKey, CudaLweCompactCiphertextList, CudaLweKeyswitchKey,
                              CudaLweMultiBitBootstrapKey128, CudaVec, _lib)

U64 = np.uint64
PBS_TYPE_MULTI_BIT, PBS_TYPE_CLASSICAL = 0, 1          # pbs/pbs_enums.h:4
OUTPUT_FLAG_NONE, OUTPUT_FLAG_OVERFLOW, OUTPUT_FLAG_CARRY = 0, 1, 2   # integer/integer.h:39
KS_TYPE_BIG_TO_SMALL, KS_TYPE_SMALL_TO_BIG = 0, 1                      # keyswitch/ks_enums.h
EXPAND_KIND = {"no_casting": 0, "casting": 1, "sanity_check": 2}       # zk/zk_enums.h
RERAND_WITH_KS, RERAND_WITHOUT_KS = 0, 1                               # integer/integer.h:45
TRIVIUM_KEY_BITS, TRIVIUM_BATCH_SIZE, TRIVIUM_REGISTER_BITS = 80, 64, (93, 84, 111)   # trivium/trivium_utilities.h:5-12
AES_BLOCK_BITS, AES_ROUND_KEYS, AES_PARALLELISMS = 128, 11, (16, 8, 4, 2, 1)             # aes/aes_utilities.h, radix/aes.rs


class CudaServerKey:
    """integer/gpu/server_key/mod.rs:26-60: keyswitch key, bootstrap key and the shortint parameters."""

    def __init__(self, ksk: CudaLweKeyswitchKey, bsk: CudaLweBootstrapKey, message_modulus, carry_modulus):
        assert ksk.output_key_lwe_dimension == bsk.input_lwe_dimension
        assert ksk.input_key_lwe_dimension == bsk.output_lwe_dimension
        self.key_switching_key, self.bootstrapping_key = ksk, bsk
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)

    # ---- FFI views
    def _bsk_params(self):
        b = self.bootstrapping_key
        g = getattr(b, "grouping_factor", 0)   # a CudaLweMultiBitBootstrapKey selects the multi-bit PBS
        return ffi.CudaLweBootstrapKeyParamsFFI(b.input_lwe_dimension, b.glwe_dimension, b.polynomial_size,
                                                b.decomp_base_log, b.decomp_level_count, b.output_lwe_dimension,
                                                PBS_TYPE_MULTI_BIT if g else PBS_TYPE_CLASSICAL, g)

    def _ksk_params(self):
        k = self.key_switching_key
        return ffi.CudaLweKeyswitchKeyParamsFFI(k.input_key_lwe_dimension, k.output_key_lwe_dimension,
                                                k.decomp_base_log, k.decomp_level_count)

    def _key_ptrs(self, streams=None):
        """One key replica per stream of the set (gpu/ffi.rs passes `ksks` / `bsks` arrays of per-GPU pointers:
        integer/gpu/mod.rs); the keys must have been converted with a stream set at least as large."""
        n = len(streams) if streams is not None else 1
        kv, bv = self.key_switching_key.d_vecs, self.bootstrapping_key.d_vecs
        assert len(kv) >= n and len(bv) >= n, "server key has fewer GPU replicas than the stream set has streams"
        ksks = (C.c_void_p * n)(*[v.ptr for v in kv[:n]])
        bsks = (C.c_void_p * n)(*[v.ptr for v in bv[:n]])
        return ksks, bsks

    @staticmethod
    def _streams(streams):
        ptrs = (C.c_void_p * len(streams))(*streams.ptr)
        idx = (C.c_uint32 * len(streams))(*streams.gpu_indexes)
        return ffi.CudaStreamsFFI(ptrs, idx, len(streams)), (ptrs, idx)

    def _noise_reduction(self):
        return 1 if getattr(self.bootstrapping_key, "ms_noise_reduction", False) else 0

    # ---- operations
    def apply_lookup_table(self, ct, lut, streams, degree=None):
        """Every block of every integer goes through KS -> PBS with `lut` (a (k+1)*N accumulator)."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        lut = np.ascontiguousarray(lut, dtype=U64)
        mem = C.c_void_p()
        n = ct.total_blocks
        _lib().scratch_cuda_apply_univariate_lut_64_async(
            s, C.byref(mem), lut.ctypes.data_as(C.c_void_p), self._bsk_params(), self._ksk_params(), n,
            self.message_modulus, self.carry_modulus, degree if degree is not None else self.message_modulus - 1, True,
            self._noise_reduction())
        out = CudaUnsignedRadixCiphertext.zeros_like(ct, streams)
        _lib().cuda_apply_univariate_lut_64_async(s, C.byref(out._ffi()), C.byref(ct._ffi()), mem, ksks, bsks)
        _lib().cleanup_cuda_apply_univariate_lut_64(s, C.byref(mem))
        return out

    def apply_many_lookup_table(self, ct, many_lut, num_luts, lut_stride, streams, degree=None):
        """integer/gpu/mod.rs cuda_backend_apply_many_univariate_lut: ONE keyswitch and ONE bootstrap per block evaluate the
        `num_luts` functions packed in `many_lut` (shortint ManyLookupTable: sub-tables of `lut_stride` coefficients,
        shortint/engine/mod.rs:169-254).  Returns a ciphertext of num_luts * blocks blocks: function t of block s of
        the input at flat block t * total_blocks + s."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        many_lut = np.ascontiguousarray(many_lut, dtype=U64)
        mem = C.c_void_p()
        n = ct.total_blocks
        _lib().scratch_cuda_apply_many_univariate_lut_64_async(
            s, C.byref(mem), many_lut.ctypes.data_as(C.c_void_p), self._bsk_params(), self._ksk_params(), n,
            self.message_modulus, self.carry_modulus, num_luts, degree if degree is not None else self.message_modulus - 1,
            True, self._noise_reduction())
        out = CudaUnsignedRadixCiphertext(CudaVec(num_luts * n * (ct.lwe_dimension + 1), streams), num_luts * ct.num_integers,
                                          ct.num_blocks, ct.lwe_dimension)
        _lib().cuda_apply_many_univariate_lut_64_async(s, C.byref(out._ffi()), C.byref(ct._ffi()), mem, ksks, bsks,
                                                       num_luts, lut_stride)
        _lib().cleanup_cuda_apply_many_univariate_lut_64(s, C.byref(mem))
        return out

    def unchecked_add_assign(self, lhs, rhs, streams):
        """Block-wise LWE addition, no carry handling (radix/add.rs unchecked_add_assign)."""
        assert lhs.total_blocks == rhs.total_blocks
        _lib().cuda_add_lwe_ciphertext_vector_inplace_64(streams.ptr[0], streams.gpu_indexes[0], C.byref(lhs._ffi()),
                                                         C.byref(rhs._ffi()))

    def _carry_blocks(self, ct, carry, streams):
        """The reference's wrappers ALWAYS hand carry_in / carry_out radix structs to the backend, whether
        or not uses_carry / requested_flag select them (integer/gpu/ffi.rs:2194-2237): one block per
        integer, zero (trivial) unless the caller supplies one."""
        if carry is not None:
            assert carry.total_blocks == ct.num_integers and carry.lwe_dimension == ct.lwe_dimension
            return carry
        return CudaUnsignedRadixCiphertext(CudaVec(ct.num_integers * (ct.lwe_dimension + 1), streams),
                                           ct.num_integers, 1, ct.lwe_dimension)

    def propagate_single_carry_assign(self, ct, streams, carry_in=None, want_carry_out=False):
        """integer/gpu/mod.rs propagate_single_carry_assign: carry_in (one block per integer, 0/1) enters
        block 0 when given; with want_carry_out (OutputFlag::Carry) the carry leaving the last block is
        returned as a one-block-per-integer ciphertext."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        flag = OUTPUT_FLAG_CARRY if want_carry_out else OUTPUT_FLAG_NONE
        cin, cout = self._carry_blocks(ct, carry_in, streams), self._carry_blocks(ct, None, streams)
        _lib().hip_integer_scratch_batch(ct.num_integers)
        _lib().scratch_cuda_propagate_single_carry_64_inplace_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), ct.num_blocks, self.message_modulus,
            self.carry_modulus, flag, True, self._noise_reduction())
        _lib().cuda_propagate_single_carry_64_inplace_async(s, C.byref(ct._ffi()), C.byref(cout._ffi()),
                                                            C.byref(cin._ffi()), mem, bsks, ksks, flag,
                                                            1 if carry_in is not None else 0)
        _lib().cleanup_cuda_propagate_single_carry_64_inplace(s, C.byref(mem))
        return cout if want_carry_out else None

    def add_assign(self, lhs, rhs, streams, carry_in=None, want_carry_out=False, want_overflow=False):
        """lhs += rhs (+ carry_in) on clean (carry-free) operands: block additions, then one carry propagation.
        want_carry_out (OutputFlag::Carry): returns the carry leaving the last block; want_overflow
        (OutputFlag::Overflow, signed integers): returns the signed-overflow flag of the addition instead
        (integer/gpu/server_key/radix/add.rs signed_overflowing_add)."""
        assert not (want_carry_out and want_overflow)
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        flag = OUTPUT_FLAG_OVERFLOW if want_overflow else OUTPUT_FLAG_CARRY if want_carry_out else OUTPUT_FLAG_NONE
        cin, cout = self._carry_blocks(lhs, carry_in, streams), self._carry_blocks(lhs, None, streams)
        _lib().hip_integer_scratch_batch(lhs.num_integers)
        _lib().scratch_cuda_add_and_propagate_single_carry_64_inplace_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), lhs.num_blocks, self.message_modulus,
            self.carry_modulus, flag, True, self._noise_reduction())
        _lib().cuda_add_and_propagate_single_carry_64_inplace_async(s, C.byref(lhs._ffi()), C.byref(rhs._ffi()),
                                                                    C.byref(cout._ffi()), C.byref(cin._ffi()), mem,
                                                                    bsks, ksks, flag, 1 if carry_in is not None else 0)
        _lib().cleanup_cuda_add_and_propagate_single_carry_64_inplace(s, C.byref(mem))
        return cout if (want_carry_out or want_overflow) else None

    def sub_assign(self, lhs, rhs, streams, want_carry_out=False):
        """lhs -= rhs (mod 2^bits) on clean operands: rhs negated with its correcting term, block additions, one carry
        propagation (integer/gpu/server_key/radix/sub.rs:347-400).  want_carry_out: the carry leaving the last block of
        lhs + (2^bits - rhs), i.e. 1 when NO borrow occurred."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        flag = OUTPUT_FLAG_CARRY if want_carry_out else OUTPUT_FLAG_NONE
        cin, cout = self._carry_blocks(lhs, None, streams), self._carry_blocks(lhs, None, streams)
        _lib().hip_integer_scratch_batch(lhs.num_integers)
        _lib().scratch_cuda_sub_and_propagate_single_carry_64_inplace_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), lhs.num_blocks, self.message_modulus,
            self.carry_modulus, flag, True, self._noise_reduction())
        _lib().cuda_sub_and_propagate_single_carry_64_inplace_async(s, C.byref(lhs._ffi()), C.byref(rhs._ffi()),
                                                                    C.byref(cout._ffi()), C.byref(cin._ffi()), mem,
                                                                    bsks, ksks, flag, 0)
        _lib().cleanup_cuda_sub_and_propagate_single_carry_64_inplace(s, C.byref(mem))
        return cout if want_carry_out else None

    def unsigned_overflowing_sub_assign(self, lhs, rhs, streams):
        """lhs -= rhs; returns the borrow, one boolean block per integer (radix/sub.rs unsigned_overflowing_sub)."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        cin, cout = self._carry_blocks(lhs, None, streams), self._carry_blocks(lhs, None, streams)
        _lib().hip_integer_scratch_batch(lhs.num_integers)
        _lib().scratch_cuda_integer_overflowing_sub_64_inplace_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), lhs.num_blocks, self.message_modulus,
            self.carry_modulus, 1, True, self._noise_reduction())
        _lib().cuda_integer_overflowing_sub_64_inplace_async(s, C.byref(lhs._ffi()), C.byref(rhs._ffi()), C.byref(cout._ffi()),
                                                             C.byref(cin._ffi()), mem, bsks, ksks, 1, 0)
        _lib().cleanup_cuda_integer_overflowing_sub_64_inplace(s, C.byref(mem))
        return cout

    def unchecked_neg(self, ct, streams):
        """-ct of ONE integer, levelled (radix/neg.rs unchecked_neg): blocks z - b with the borrowed unit handed on; the
        result carries degrees above the message modulus (propagate before the next bootstrap-free operation)."""
        assert ct.num_integers == 1
        s, keep = self._streams(streams)
        out = CudaUnsignedRadixCiphertext.zeros_like(ct, streams)
        _lib().cuda_negate_ciphertext_64(s, C.byref(out._ffi()), C.byref(ct._ffi()), self.message_modulus,
                                         self.carry_modulus, ct.total_blocks)
        return out

    def unchecked_scalar_add_assign(self, ct, clear_blocks, streams):
        """ct[i] += clear_blocks[i] (plaintext addition on the bodies; radix/scalar_add.rs unchecked_scalar_add_assign)."""
        import numpy as np
        s, keep = self._streams(streams)
        h = np.ascontiguousarray(np.asarray(clear_blocks, dtype=np.uint64))
        d = CudaVec(max(1, h.size), streams)
        d.copy_from_cpu_async(h, streams)
        _lib().cuda_scalar_addition_ciphertext_64_inplace(s, C.byref(ct._ffi()), d.ptr, h.ctypes.data_as(C.c_void_p),
                                                          h.size, self.message_modulus, self.carry_modulus)
        streams.synchronize()

    def bitnot_assign(self, ct, streams):
        """Bitwise NOT of clean blocks, levelled (radix/bitwise_op.rs unchecked_bitnot_assign)."""
        s, keep = self._streams(streams)
        _lib().cuda_bitnot_ciphertext_64(s, C.byref(ct._ffi()), self.message_modulus, self.message_modulus,
                                         self.carry_modulus)

    def bitop_assign(self, lhs, rhs, op, streams):
        """lhs <- lhs (and | or | xor) rhs, one bivariate bootstrap per block pair (radix/bitwise_op.rs
        unchecked_bitop_assign); op in {"and", "or", "xor"}."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        code = {"and": 0, "or": 1, "xor": 2}[op]
        _lib().hip_integer_scratch_batch(1)
        _lib().scratch_cuda_integer_bitop_inplace_64_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), lhs.total_blocks, self.message_modulus,
            self.carry_modulus, code, True, self._noise_reduction())
        _lib().cuda_integer_bitop_inplace_64_async(s, C.byref(lhs._ffi()), C.byref(rhs._ffi()), mem, bsks, ksks)
        _lib().cleanup_cuda_integer_bitop_inplace_64(s, C.byref(mem))

    def scalar_bitop_assign(self, ct, clear_blocks, op, streams):
        """ct <- ct (and | or | xor) scalar, the scalar given as its clear blocks, least significant first
        (radix/scalar_bitwise_op.rs): a univariate table per clear value; AND clears the blocks past the scalar's."""
        import numpy as np
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        code = {"and": 3, "or": 4, "xor": 5}[op]
        h = np.ascontiguousarray(np.asarray(clear_blocks, dtype=np.uint64))
        d = CudaVec(max(1, h.size), streams)
        d.copy_from_cpu_async(h, streams)
        _lib().hip_integer_scratch_batch(1)
        _lib().scratch_cuda_integer_scalar_bitop_inplace_64_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), ct.total_blocks, self.message_modulus,
            self.carry_modulus, code, True, self._noise_reduction())
        _lib().cuda_integer_scalar_bitop_inplace_64_async(s, C.byref(ct._ffi()), d.ptr, h.ctypes.data_as(C.c_void_p),
                                                          h.size, mem, bsks, ksks)
        _lib().cleanup_cuda_integer_scalar_bitop_inplace_64(s, C.byref(mem))
        streams.synchronize()

    def full_propagate_assign(self, ct, streams):
        """Block after block: message kept, carry added to the next block (radix/mod.rs full_propagate_parallelized's
        sequential form, integer.cuh:1924-1983); ONE integer; the last block's carry is dropped."""
        assert ct.num_integers == 1
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        _lib().scratch_cuda_full_propagation_64_inplace_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), self.message_modulus, self.carry_modulus, True,
            self._noise_reduction())
        _lib().cuda_full_propagation_64_inplace_async(s, C.byref(ct._ffi()), mem, ksks, bsks, ct.total_blocks)
        _lib().cleanup_cuda_full_propagation_64_inplace(s, C.byref(mem))

    COMPARISONS = {"eq": 0, "ne": 1, "gt": 2, "ge": 3, "lt": 4, "le": 5, "max": 6, "min": 7}  # integer.h:24-33

    def compare(self, lhs, rhs, op, streams):
        """Unsigned comparison of ONE integer pair (radix/comparison.rs unchecked_{eq,ne,gt,ge,lt,le,max,min}): a boolean
        block for eq ... le, an integer for max / min."""
        assert lhs.num_integers == rhs.num_integers == 1 and lhs.num_blocks == rhs.num_blocks
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        code = self.COMPARISONS[op]
        L, w = lhs.num_blocks, lhs.lwe_dimension + 1
        out = (CudaUnsignedRadixCiphertext.zeros_like(lhs, streams) if code >= 6 else
               CudaUnsignedRadixCiphertext(CudaVec(w, streams), 1, 1, lhs.lwe_dimension))
        _lib().scratch_cuda_integer_comparison_64_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), L, self.message_modulus, self.carry_modulus, code,
            False, True, self._noise_reduction())
        _lib().cuda_integer_comparison_64_async(s, C.byref(out._ffi()), C.byref(lhs._ffi()), C.byref(rhs._ffi()), mem, bsks,
                                                ksks)
        _lib().cleanup_cuda_integer_comparison_64(s, C.byref(mem))
        return out

    def scalar_compare(self, ct, scalar, op, streams):
        """Unsigned comparison of ONE integer with a clear scalar below 2^bits (radix/scalar_comparison.rs unchecked_scalar_*):
        the scalar's blocks stop at its last non-zero one, as BlockDecomposer::with_early_stop_at_zero yields them."""
        assert ct.num_integers == 1 and 0 <= int(scalar) < self.message_modulus ** ct.num_blocks
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        code = self.COMPARISONS[op]
        blocks, v = [], int(scalar)
        while v:
            blocks.append(v % self.message_modulus)
            v //= self.message_modulus
        h = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint64))
        d = CudaVec(max(1, h.size), streams)
        if h.size:
            d.copy_from_cpu_async(h, streams)
        L, w = ct.num_blocks, ct.lwe_dimension + 1
        out = (CudaUnsignedRadixCiphertext.zeros_like(ct, streams) if code >= 6 else
               CudaUnsignedRadixCiphertext(CudaVec(w, streams), 1, 1, ct.lwe_dimension))
        _lib().scratch_cuda_integer_scalar_comparison_64_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), L, self.message_modulus, self.carry_modulus, code,
            False, True, self._noise_reduction())
        _lib().cuda_integer_scalar_comparison_64_async(s, C.byref(out._ffi()), C.byref(ct._ffi()), d.ptr,
                                                       h.ctypes.data_as(C.c_void_p), mem, bsks, ksks, h.size)
        _lib().cleanup_cuda_integer_scalar_comparison_64(s, C.byref(mem))
        streams.synchronize()
        return out

    def if_then_else(self, condition, ct_true, ct_false, streams):
        """condition ? ct_true : ct_false, ONE integer (radix/cmux.rs unchecked_if_then_else); condition: a boolean block."""
        assert ct_true.total_blocks == ct_false.total_blocks and condition.total_blocks >= 1
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        out = CudaUnsignedRadixCiphertext.zeros_like(ct_true, streams)
        _lib().scratch_cuda_cmux_64_async(s, C.byref(mem), self._bsk_params(), self._ksk_params(), ct_true.total_blocks,
                                          self.message_modulus, self.carry_modulus, True, self._noise_reduction())
        _lib().cuda_cmux_64_async(s, C.byref(out._ffi()), C.byref(condition._ffi()), C.byref(ct_true._ffi()),
                                  C.byref(ct_false._ffi()), mem, bsks, ksks)
        _lib().cleanup_cuda_cmux_64(s, C.byref(mem))
        return out

    def _shift_family(self, name, ct, scratch_args, launch_args, streams, count=False):
        """scratch -> launch -> cleanup of one of the hip_ shift / rotate entry points, sized for ct's batch"""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        lib = _lib()
        lib.hip_integer_scratch_batch(ct.num_integers)
        getattr(lib, f"hip_scratch_integer_{name}_64_inplace_async")(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), ct.num_blocks, self.message_modulus,
            self.carry_modulus, *scratch_args, True, self._noise_reduction())
        lib.hip_integer_scratch_batch(1)
        pbs = int(lib.hip_integer_shift_and_rotate_pbs_count(mem)) if count else None
        getattr(lib, f"hip_integer_{name}_64_inplace_async")(s, C.byref(ct._ffi()), *launch_args, mem, bsks, ksks)
        getattr(lib, f"hip_cleanup_integer_{name}_64_inplace")(s, C.byref(mem))
        return pbs

    def scalar_rotate_assign(self, ct, n, streams, left=True):
        """ct = ct rotated left / right by the clear amount n (mod the bit width), every integer of the batch
        (radix/scalar_rotate.rs unchecked_scalar_rotate_{left,right}_assign)."""
        self._shift_family("scalar_rotate", ct, (2 if left else 3,), (int(n),), streams)

    def shift_assign(self, ct, amount, streams, left=True, arithmetic=False, return_pbs_count=False):
        """ct <<= amount / ct >>= amount with an ENCRYPTED amount of the same shape, every integer of the batch by its own
        amount (radix/shift.rs unchecked_{left,right}_shift_assign).  arithmetic: ct is two's complement, the right shift
        fills with its sign.  An amount of the bit width or more gives 0 (all ones for a negative arithmetic operand)."""
        if arithmetic and left:
            raise ValueError("an arithmetic shift is a right shift")
        assert amount.num_integers == ct.num_integers and amount.num_blocks == ct.num_blocks
        return self._shift_family("shift_and_rotate", ct, (0 if left else 1, bool(arithmetic)), (C.byref(amount._ffi()),),
                                  streams, count=return_pbs_count)

    def rotate_assign(self, ct, amount, streams, left=True, return_pbs_count=False):
        """ct = ct rotated by an ENCRYPTED amount of the same shape (radix/rotate.rs unchecked_rotate_{left,right}_assign):
        by (amount mod 2^m) mod bits, m = ceil(log2 bits) — amount mod bits when the bit width is a power of two."""
        assert amount.num_integers == ct.num_integers and amount.num_blocks == ct.num_blocks
        return self._shift_family("shift_and_rotate", ct, (2 if left else 3, False), (C.byref(amount._ffi()),), streams,
                                  count=return_pbs_count)

    # ---- division (integer/gpu/server_key/radix/div_mod.rs, abs.rs)
    def div_rem(self, numerator, divisor, streams, signed=False, return_pbs_count=False):
        """(numerator / divisor, numerator % divisor), every pair of the batch in the same rounds (radix/div_mod.rs
        unchecked_div_rem).  signed: two's complement operands, truncation towards zero, the remainder takes the
        numerator's sign, MIN / -1 wraps to MIN.  Unsigned x / 0 = all ones, x % 0 = x; signed x / 0 = 1 for x < 0, else -1."""
        assert numerator.num_integers == divisor.num_integers and numerator.num_blocks == divisor.num_blocks
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        q = CudaUnsignedRadixCiphertext.zeros_like(numerator, streams)
        r = CudaUnsignedRadixCiphertext.zeros_like(numerator, streams)
        mem = C.c_void_p()
        lib = _lib()
        lib.hip_integer_scratch_batch(numerator.num_integers)
        lib.hip_scratch_integer_div_rem_64_async(s, bool(signed), C.byref(mem), self._bsk_params(), self._ksk_params(),
                                                 numerator.num_blocks, self.message_modulus, self.carry_modulus, True,
                                                 self._noise_reduction())
        lib.hip_integer_scratch_batch(1)
        lib.hip_integer_div_rem_64_async(s, C.byref(q._ffi()), C.byref(r._ffi()), C.byref(numerator._ffi()),
                                         C.byref(divisor._ffi()), bool(signed), mem, bsks, ksks)
        lib.hip_cleanup_integer_div_rem_64(s, C.byref(mem))
        if not return_pbs_count:
            return q, r
        pbs = int(lib.hip_integer_div_rem_pbs_count(bool(signed), numerator.num_blocks, self.message_modulus,
                                                    self.carry_modulus))
        return q, r, pbs * numerator.num_integers

    def div(self, numerator, divisor, streams, signed=False):
        return self.div_rem(numerator, divisor, streams, signed)[0]

    def rem(self, numerator, divisor, streams, signed=False):
        return self.div_rem(numerator, divisor, streams, signed)[1]

    def abs_assign(self, ct, streams):
        """ct = |ct| for two's complement integers, every integer of the batch (radix/abs.rs unchecked_abs); |MIN| = MIN."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        lib = _lib()
        lib.hip_integer_scratch_batch(ct.num_integers)
        lib.hip_scratch_integer_abs_inplace_64_async(s, C.byref(mem), True, self._bsk_params(), self._ksk_params(),
                                                     ct.num_blocks, self.message_modulus, self.carry_modulus, True,
                                                     self._noise_reduction())
        lib.hip_integer_scratch_batch(1)
        lib.hip_integer_abs_inplace_64_async(s, C.byref(ct._ffi()), mem, True, bsks, ksks)
        lib.hip_cleanup_integer_abs_inplace_64(s, C.byref(mem))

    # ---- bit counts (integer/gpu/server_key/radix/ilog2.rs; count_ones / count_zeros: radix_parallel/count_zeros_ones.rs)
    BIT_COUNT_RUNS, BIT_COUNT_ILOG2, BIT_COUNT_POP = 0, 1, 2      # `kind` of hip_integer_bit_count_pbs_count

    def counter_num_blocks(self, num_blocks, ilog2=False):
        """blocks of the result: ceil((floor(log2 B) + 1) / b) for a run or a popcount over B = b * num_blocks bits
        (ilog2.rs:32-33), ceil((floor(log2(B - 1)) + 2) / b) for ilog2 (ilog2.rs:166-167)"""
        b = self.message_modulus.bit_length() - 1
        B = b * num_blocks
        need = ((B - 1).bit_length() - 1 if B > 1 else 0) + 2 if ilog2 else B.bit_length()
        return -(-need // b)

    def _bit_count(self, kind, ct, streams, scratch, launch, return_pbs_count):
        """scratch -> launch -> cleanup of one bit-count entry point, sized for ct's batch; out of place"""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        nc = self.counter_num_blocks(ct.num_blocks, ilog2=kind == self.BIT_COUNT_ILOG2)
        out = CudaUnsignedRadixCiphertext(CudaVec(ct.num_integers * nc * (ct.lwe_dimension + 1), streams), ct.num_integers, nc,
                                          ct.lwe_dimension)
        mem = C.c_void_p()
        lib = _lib()
        name = ("count_of_consecutive_bits", "ilog2", "count_ones")[kind]
        lib.hip_integer_scratch_batch(ct.num_integers)
        scratch(lib, s, C.byref(mem), nc)
        lib.hip_integer_scratch_batch(1)
        launch(lib, s, out, mem, bsks, ksks)
        getattr(lib, f"hip_cleanup_integer_{name}_64")(s, C.byref(mem))
        if not return_pbs_count:
            return out
        pbs = int(lib.hip_integer_bit_count_pbs_count(kind, ct.num_blocks, self.message_modulus, self.carry_modulus))
        return out, pbs * ct.num_integers

    def _unchecked_run(self, ct, streams, leading, ones, return_pbs_count=False):
        return self._bit_count(
            self.BIT_COUNT_RUNS, ct, streams,
            lambda lib, s, mem, nc: lib.hip_scratch_integer_count_of_consecutive_bits_64_async(
                s, mem, self._bsk_params(), self._ksk_params(), ct.num_blocks, nc, self.message_modulus, self.carry_modulus,
                1 if leading else 0, 1 if ones else 0, True, self._noise_reduction()),
            lambda lib, s, out, mem, bsks, ksks: lib.hip_integer_count_of_consecutive_bits_64_async(
                s, C.byref(out._ffi()), C.byref(ct._ffi()), mem, bsks, ksks),
            return_pbs_count)

    def unchecked_leading_zeros(self, ct, streams, return_pbs_count=False):
        """the number of consecutive zeros from the most significant bit, every integer of the batch, as an unsigned integer
        of counter_num_blocks blocks (ilog2.rs unchecked_leading_zeros); the operand's blocks must be clean"""
        return self._unchecked_run(ct, streams, True, False, return_pbs_count)

    def unchecked_leading_ones(self, ct, streams, return_pbs_count=False):
        return self._unchecked_run(ct, streams, True, True, return_pbs_count)

    def unchecked_trailing_zeros(self, ct, streams, return_pbs_count=False):
        return self._unchecked_run(ct, streams, False, False, return_pbs_count)

    def unchecked_trailing_ones(self, ct, streams, return_pbs_count=False):
        return self._unchecked_run(ct, streams, False, True, return_pbs_count)

    def unchecked_ilog2(self, ct, streams, return_pbs_count=False):
        """floor(log2(ct)) as an unsigned integer of counter_num_blocks(ilog2=True) blocks, in the rounds of leading_zeros
        (ilog2.rs unchecked_ilog2); ilog2(0) is all ones.  The three trivial operands of the reference's parameter list are
        handed over with the reference's block counts; the backend does not read them."""
        w = ct.lwe_dimension + 1

        def launch(lib, s, out, mem, bsks, ksks):
            nc = out.num_blocks
            triv = [CudaUnsignedRadixCiphertext(CudaVec(n * w, streams), 1, n, ct.lwe_dimension) for n in (nc, nc, 1)]
            lib.hip_integer_ilog2_64_async(s, C.byref(out._ffi()), C.byref(ct._ffi()), *(C.byref(t._ffi()) for t in triv), mem,
                                           bsks, ksks)
            streams.synchronize()          # (the trivial operands go out of scope)

        return self._bit_count(
            self.BIT_COUNT_ILOG2, ct, streams,
            lambda lib, s, mem, nc: lib.hip_scratch_integer_ilog2_64_async(
                s, mem, self._bsk_params(), self._ksk_params(), self.message_modulus, self.carry_modulus, ct.num_blocks, nc,
                ct.num_blocks * (self.message_modulus.bit_length() - 1), True, self._noise_reduction()),
            launch, return_pbs_count)

    def _unchecked_popcount(self, ct, streams, ones, return_pbs_count=False):
        return self._bit_count(
            self.BIT_COUNT_POP, ct, streams,
            lambda lib, s, mem, nc: lib.hip_scratch_integer_count_ones_64_async(
                s, mem, self._bsk_params(), self._ksk_params(), ct.num_blocks, nc, self.message_modulus, self.carry_modulus,
                1 if ones else 0, True, self._noise_reduction()),
            lambda lib, s, out, mem, bsks, ksks: lib.hip_integer_count_ones_64_async(
                s, C.byref(out._ffi()), C.byref(ct._ffi()), mem, bsks, ksks),
            return_pbs_count)

    def unchecked_count_ones(self, ct, streams, return_pbs_count=False):
        """the number of set bits, one round over the pairs of blocks, a sum and a carry propagation
        (count_zeros_ones.rs unchecked_count_ones_parallelized)"""
        return self._unchecked_popcount(ct, streams, True, return_pbs_count)

    def unchecked_count_zeros(self, ct, streams, return_pbs_count=False):
        return self._unchecked_popcount(ct, streams, False, return_pbs_count)

    def _clean(self, ct, streams):
        """ct itself when every block is clean, else a propagated duplicate (ONE integer: full_propagate_assign)"""
        if int(ct.degrees.max(initial=0)) <= self.message_modulus - 1:
            return ct
        dup = ct.duplicate(streams)
        dup._info[0][:], dup._info[1][:] = ct._info[0], ct._info[1]
        self.full_propagate_assign(dup, streams)
        return dup

    def leading_zeros(self, ct, streams, return_pbs_count=False):
        """unchecked_leading_zeros on the operand, propagated first on a duplicate when a block is not clean; the bootstraps
        reported are the count's alone"""
        return self.unchecked_leading_zeros(self._clean(ct, streams), streams, return_pbs_count)

    def leading_ones(self, ct, streams, return_pbs_count=False):
        return self.unchecked_leading_ones(self._clean(ct, streams), streams, return_pbs_count)

    def trailing_zeros(self, ct, streams, return_pbs_count=False):
        return self.unchecked_trailing_zeros(self._clean(ct, streams), streams, return_pbs_count)

    def trailing_ones(self, ct, streams, return_pbs_count=False):
        return self.unchecked_trailing_ones(self._clean(ct, streams), streams, return_pbs_count)

    def ilog2(self, ct, streams, return_pbs_count=False):
        return self.unchecked_ilog2(self._clean(ct, streams), streams, return_pbs_count)

    def count_ones(self, ct, streams, return_pbs_count=False):
        return self.unchecked_count_ones(self._clean(ct, streams), streams, return_pbs_count)

    def count_zeros(self, ct, streams, return_pbs_count=False):
        return self.unchecked_count_zeros(self._clean(ct, streams), streams, return_pbs_count)

    def checked_ilog2(self, ct, streams):
        """(ilog2(ct), ct > 0) of ONE unsigned integer (ilog2.rs checked_ilog2): the flag is scalar_compare(ct, 0, "gt").
        Unsigned only: a signed operand needs `ct > 0` as a signed comparison, which is not wired."""
        clean = self._clean(ct, streams)
        return self.unchecked_ilog2(clean, streams), self.scalar_compare(clean, 0, "gt", streams)

    # ---- Trivium transciphering (integer/gpu/server_key/radix/trivium.rs)
    def _trivium_call(self, kind, num_inputs, streams, launch, num_steps=0, window=None):
        """scratch -> launch -> cleanup of hip_trivium_{init,step}; returns the published bootstrap count of the call"""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        lib = _lib()
        getattr(lib, f"hip_scratch_trivium_{kind}_async")(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), self.message_modulus, self.carry_modulus, True,
            self._noise_reduction(), num_inputs)
        if window is not None:
            lib.hip_test_trivium_set_window(mem, window)
        pbs = int(lib.hip_trivium_pbs_count(mem, num_steps))
        launch(lib, s, mem, bsks, ksks)
        getattr(lib, f"hip_cleanup_trivium_{kind}")(s, C.byref(mem))
        return pbs

    def trivium_init(self, key, iv, streams, return_pbs_count=False):
        """The state after Trivium's 1,152 warm-up steps, N ciphers side by side: `key` and `iv` hold 80 N blocks, bit i of
        input n at block i N + n, every block an encrypted bit.  6,912 N bootstraps in 36 rounds."""
        if key.total_blocks % TRIVIUM_KEY_BITS or key.total_blocks == 0 or iv.total_blocks != key.total_blocks:
            raise ValueError(f"Input key and IV must contain {TRIVIUM_KEY_BITS} encrypted bits per input.")
        n = key.total_blocks // TRIVIUM_KEY_BITS
        w = key.lwe_dimension + 1
        state = CudaTriviumState(*(CudaUnsignedRadixCiphertext(CudaVec(bits * n * w, streams), 1, bits * n, key.lwe_dimension)
                                   for bits in TRIVIUM_REGISTER_BITS))
        pbs = self._trivium_call("init", n, streams, lambda lib, s, mem, bsks, ksks: lib.hip_trivium_init_async(
            s, C.byref(state.a._ffi()), C.byref(state.b._ffi()), C.byref(state.c._ffi()), C.byref(key._ffi()),
            C.byref(iv._ffi()), n, mem, bsks, ksks))
        return (state, pbs) if return_pbs_count else state

    def trivium_next(self, state, num_steps, streams, return_pbs_count=False, _window=None):
        """The next `num_steps` keystream bits (a multiple of 64) of every input; the state advances.  Returns num_steps N
        blocks, the bit of step t of input n at block t N + n.  512 N bootstraps per 64 steps, in two rounds."""
        if num_steps % TRIVIUM_BATCH_SIZE:
            raise ValueError(f"The number of steps must be a multiple of {TRIVIUM_BATCH_SIZE}.")
        n = state.num_inputs
        w = state.a.lwe_dimension + 1
        keystream = CudaUnsignedRadixCiphertext(CudaVec(max(1, num_steps * n * w), streams), 1, num_steps * n,
                                                state.a.lwe_dimension)
        pbs = self._trivium_call("step", n, streams, lambda lib, s, mem, bsks, ksks: lib.hip_trivium_step_async(
            s, C.byref(keystream._ffi()), C.byref(state.a._ffi()), C.byref(state.b._ffi()), C.byref(state.c._ffi()), n,
            num_steps, mem, bsks, ksks), num_steps=num_steps, window=_window)
        return (keystream, pbs) if return_pbs_count else keystream

    def trivium_generate_keystream(self, key, iv, num_steps, streams):
        """trivium_init, then trivium_next on a state that is dropped afterwards."""
        if num_steps % TRIVIUM_BATCH_SIZE:
            raise ValueError(f"The number of steps must be a multiple of {TRIVIUM_BATCH_SIZE}.")
        return self.trivium_next(self.trivium_init(key, iv, streams), num_steps, streams)

    # ---- AES-128 transciphering (integer/gpu/server_key/radix/aes.rs)
    def _aes_scratch(self, lib, s, mem, kind, allocate, num_aes_inputs=1, sbox_parallelism=16):
        head = (s, C.byref(mem), self._bsk_params(), self._ksk_params(), self.message_modulus, self.carry_modulus, allocate,
                self._noise_reduction())
        if kind == "key_expansion":
            return int(lib.hip_scratch_integer_key_expansion_64_async(*head))
        return int(lib.hip_scratch_integer_aes_ctr_encrypt_64_async(*head, num_aes_inputs, sbox_parallelism))

    def _aes_call(self, kind, streams, launch, counts, **shape):
        """scratch -> launch -> cleanup of hip_integer_{aes_ctr_encrypt,key_expansion}_64; `counts` receives the published
        bootstraps and rounds of the call"""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        lib = _lib()
        self._aes_scratch(lib, s, mem, kind, True, **shape)
        counts[:] = [int(lib.hip_integer_aes_pbs_count(mem)), int(lib.hip_integer_aes_rounds(mem))]
        launch(lib, s, mem, bsks, ksks)
        getattr(lib, f"hip_cleanup_integer_{kind}_64")(s, C.byref(mem))

    def get_key_expansion_size_on_gpu(self, streams):
        s, keep = self._streams(streams)
        mem = C.c_void_p()
        size = self._aes_scratch(_lib(), s, mem, "key_expansion", False)
        _lib().hip_cleanup_integer_key_expansion_64(s, C.byref(mem))
        return size

    def get_aes_encrypt_size_on_gpu(self, num_aes_inputs, sbox_parallelism, streams):
        s, keep = self._streams(streams)
        mem = C.c_void_p()
        size = self._aes_scratch(_lib(), s, mem, "aes_ctr_encrypt", False, num_aes_inputs, sbox_parallelism)
        _lib().hip_cleanup_integer_aes_ctr_encrypt_64(s, C.byref(mem))
        return size

    @staticmethod
    def _aes_result(ct, counts, return_pbs_count, return_rounds):
        extra = ([counts[0]] if return_pbs_count else []) + ([counts[1]] if return_rounds else [])
        return (ct, *extra) if extra else ct

    def key_expansion(self, key, streams, return_pbs_count=False, return_rounds=False):
        """The 11 round keys of AES-128 from 128 encrypted key bits (block i holds bit 127 - i): 1,408 blocks, round key r at
        blocks 128 r .. 128 r + 127 in the same bit order, every block a clean bit."""
        if key.total_blocks != AES_BLOCK_BITS:
            raise ValueError(f"Input key must contain {AES_BLOCK_BITS} encrypted bits, but contains {key.total_blocks}")
        w = key.lwe_dimension + 1
        blocks = AES_ROUND_KEYS * AES_BLOCK_BITS
        out = CudaUnsignedRadixCiphertext(CudaVec(blocks * w, streams), 1, blocks, key.lwe_dimension)
        counts = []
        self._aes_call("key_expansion", streams, lambda lib, s, mem, bsks, ksks: lib.hip_integer_key_expansion_64_async(
            s, C.byref(out._ffi()), C.byref(key._ffi()), mem, bsks, ksks), counts)
        return self._aes_result(out, counts, return_pbs_count, return_rounds)

    def aes_encrypt(self, iv, round_keys, start_counter, num_aes_inputs, sbox_parallelism, streams, return_pbs_count=False,
                    return_rounds=False):
        """AES_k((iv + start_counter + n) mod 2^128) for n < num_aes_inputs under the expanded key: 128 blocks per input, input
        n at blocks 128 n .., block i of an input holds bit 127 - i.  sbox_parallelism: state bytes per S-box pass."""
        if iv.total_blocks != AES_BLOCK_BITS:
            raise ValueError(f"AES IV must contain {AES_BLOCK_BITS} encrypted bits, but contains {iv.total_blocks}")
        if round_keys.total_blocks != AES_ROUND_KEYS * AES_BLOCK_BITS:
            raise ValueError(f"Round keys must contain {AES_ROUND_KEYS * AES_BLOCK_BITS} encrypted bits, but contain "
                             f"{round_keys.total_blocks}")
        if sbox_parallelism not in AES_PARALLELISMS:
            raise ValueError(f"Invalid S-Box parallelism: must be one of [1, 2, 4, 8, 16], got {sbox_parallelism}")
        if num_aes_inputs < 1:
            raise ValueError("AES needs at least one input")
        n = int(num_aes_inputs)
        w = iv.lwe_dimension + 1
        out = CudaUnsignedRadixCiphertext(CudaVec(AES_BLOCK_BITS * n * w, streams), 1, AES_BLOCK_BITS * n, iv.lwe_dimension)
        bits = np.array([((int(start_counter) + i) >> b) & 1 for i in range(n) for b in range(AES_BLOCK_BITS)], dtype=U64)
        counts = []
        self._aes_call("aes_ctr_encrypt", streams, lambda lib, s, mem, bsks, ksks: lib.hip_integer_aes_ctr_encrypt_64_async(
            s, C.byref(out._ffi()), C.byref(iv._ffi()), C.byref(round_keys._ffi()), bits.ctypes.data, n, mem, bsks, ksks),
            counts, num_aes_inputs=n, sbox_parallelism=sbox_parallelism)
        streams.synchronize()     # `bits` is host memory of this call
        return self._aes_result(out, counts, return_pbs_count, return_rounds)

    def aes_ctr_with_fixed_parallelism(self, key, iv, start_counter, num_aes_inputs, sbox_parallelism, streams):
        """key_expansion, then aes_encrypt at the given S-box parallelism."""
        if sbox_parallelism not in AES_PARALLELISMS:
            raise ValueError(f"Invalid S-Box parallelism: must be one of [1, 2, 4, 8, 16], got {sbox_parallelism}")
        return self.aes_encrypt(iv, self.key_expansion(key, streams), start_counter, num_aes_inputs, sbox_parallelism, streams)

    def aes_ctr(self, key, iv, start_counter, num_aes_inputs, streams):
        """AES-128 in counter mode on encrypted key and IV, at the largest S-box parallelism whose scratch fits the first GPU
        of the stream set (aes.rs aes_ctr: 16, 8, .. 1, asked of cuda_check_valid_malloc)."""
        gpu = streams.gpu_indexes[0]
        if not _lib().cuda_check_valid_malloc(self.get_key_expansion_size_on_gpu(streams), gpu):
            raise MemoryError("Not enough GPU memory for the AES key expansion")
        for parallelism in AES_PARALLELISMS:
            if _lib().cuda_check_valid_malloc(self.get_aes_encrypt_size_on_gpu(num_aes_inputs, parallelism, streams), gpu):
                return self.aes_ctr_with_fixed_parallelism(key, iv, start_counter, num_aes_inputs, parallelism, streams)
        raise MemoryError("Failed to allocate GPU memory for AES, even with the lowest parallelism setting.")

    def scalar_shift_assign(self, ct, shift, streams, left=True, arithmetic=False):
        """ct <<= shift / ct >>= shift (clear amount; radix/scalar_shift.rs unchecked_scalar_{left,right}_shift_assign).
        Logical: ONE integer.  arithmetic=True: the right shift of a two's complement value, every integer of the batch."""
        if arithmetic:
            if left:
                raise ValueError("an arithmetic shift is a right shift")
            self._shift_family("arithmetic_scalar_shift", ct, (1,), (int(shift),), streams)
            return
        assert ct.num_integers == 1
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        _lib().scratch_cuda_logical_scalar_shift_64_inplace_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), ct.total_blocks, self.message_modulus,
            self.carry_modulus, 0 if left else 1, True, self._noise_reduction())
        _lib().cuda_logical_scalar_shift_64_inplace_async(s, C.byref(ct._ffi()), int(shift), mem, bsks, ksks)
        _lib().cleanup_cuda_logical_scalar_shift_64_inplace(s, C.byref(mem))

    def mul_assign(self, lhs, rhs, streams, return_pbs_count=False):
        """lhs *= rhs (mod 2^bits) on clean operands: schoolbook block products, column sums, propagation."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        _lib().hip_integer_scratch_batch(lhs.num_integers)
        _lib().scratch_cuda_integer_mult_inplace_64_async(
            s, C.byref(mem), False, False, self.message_modulus, self.carry_modulus, self._bsk_params(),
            self._ksk_params(), lhs.num_blocks, True, self._noise_reduction())
        pbs = int(_lib().hip_integer_mult_pbs_count(mem))
        _lib().cuda_integer_mult_inplace_64_async(s, C.byref(lhs._ffi()), False, C.byref(rhs._ffi()), False, bsks, ksks,
                                                  mem, self.bootstrapping_key.polynomial_size, lhs.num_blocks)
        _lib().cleanup_cuda_integer_mult_inplace_64(s, C.byref(mem))
        return pbs if return_pbs_count else None

    def scalar_mul_assign(self, ct, scalar, streams, return_pbs_count=False):
        """ct *= scalar (mod 2^bits) on clean blocks, every integer of the batch by the same clear scalar
        (radix/scalar_mul.rs:67-110 unchecked_scalar_mul_assign, with its shortcuts: 0 gives zero, 1 does nothing, a
        power of two is a left shift).  Otherwise one round of shifted blocks, column sums, one carry propagation."""
        scalar = int(scalar)
        assert scalar >= 0
        w = ct.lwe_dimension + 1
        if scalar == 0:
            _lib().cuda_memset_async(ct.d_blocks.ptr, 0, ct.total_blocks * w * 8, streams.ptr[0], streams.gpu_indexes[0])
            ct._info[0][:] = 0
            ct._info[1][:] = 0
            return 0 if return_pbs_count else None
        if scalar == 1 or ct.total_blocks == 0:
            return 0 if return_pbs_count else None
        msg_bits = self.message_modulus.bit_length() - 1
        if scalar & (scalar - 1) == 0 and ct.num_integers == 1:
            # shifting costs one bivariate PBS per block, so it is always cheaper than multiplying
            shift = scalar.bit_length() - 1
            self.scalar_shift_assign(ct, shift, streams, left=True)
            survive = max(0, ct.num_blocks - shift // msg_bits)
            return (survive if shift % msg_bits else 0) if return_pbs_count else None
        bits = [(scalar >> i) & 1 for i in range(scalar.bit_length())]      # BlockDecomposer::with_early_stop_at_zero(scalar, 1)
        has_at_least_one_set = np.zeros(msg_bits, dtype=U64)
        for i, b in enumerate(bits):
            if b:
                has_at_least_one_set[i % msg_bits] = 1
        decomposed = np.ascontiguousarray(bits, dtype=U64)
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        _lib().hip_integer_scratch_batch(ct.num_integers)
        _lib().hip_scratch_integer_scalar_mul_64_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), ct.num_blocks, self.message_modulus,
            self.carry_modulus, len(bits), True, self._noise_reduction())
        _lib().hip_integer_scratch_batch(1)
        pbs = int(_lib().hip_integer_scalar_mul_pbs_count(mem, decomposed.ctypes.data_as(C.c_void_p), len(bits)))
        _lib().hip_integer_scalar_mul_64_async(
            s, C.byref(ct._ffi()), decomposed.ctypes.data_as(C.c_void_p), has_at_least_one_set.ctypes.data_as(C.c_void_p),
            mem, bsks, ksks, self.bootstrapping_key.polynomial_size, self.message_modulus, len(bits))
        _lib().hip_cleanup_integer_scalar_mul_64(s, C.byref(mem))
        return pbs if return_pbs_count else None

    def unchecked_scalar_mul(self, ct, scalar, streams):
        """The copying form of scalar_mul_assign (scalar_mul.rs:50-65): `ct` is left as it is."""
        out = ct.duplicate(streams)
        out._info[0][:] = ct._info[0]
        out._info[1][:] = ct._info[1]
        self.scalar_mul_assign(out, scalar, streams)
        return out

    def unchecked_partial_sum_ciphertexts(self, vec, streams, reduce=False, out=None, max_num_radix_in_vec=None,
                                          return_pbs_count=False):
        """The raw call (integer/gpu/mod.rs cuda_backend_unchecked_partial_sum_ciphertexts_assign): `vec` holds V
        integers, [v][block]; their blocks are added column by column, with message / carry rounds wherever a column
        would outgrow a block.  Without `reduce` the output blocks may be as large as a block holds; with it they end at
        what one carry propagation accepts.  `out` (one integer) may be a view of the first integer of `vec`.  Degrees
        and noise levels of the result are written back."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        if out is None:
            out = CudaUnsignedRadixCiphertext(CudaVec(vec.num_blocks * (vec.lwe_dimension + 1), streams), 1, vec.num_blocks,
                                              vec.lwe_dimension)
        mem = C.c_void_p()
        cap = vec.num_integers if max_num_radix_in_vec is None else int(max_num_radix_in_vec)
        _lib().hip_scratch_partial_sum_ciphertexts_vec_64_async(
            s, C.byref(mem), self._bsk_params(), self._ksk_params(), vec.num_blocks, cap, self.message_modulus,
            self.carry_modulus, bool(reduce), True, self._noise_reduction())
        _lib().hip_partial_sum_ciphertexts_vec_64_async(s, C.byref(out._ffi()), C.byref(vec._ffi()), mem, bsks, ksks)
        pbs = int(_lib().hip_partial_sum_ciphertexts_vec_pbs_count(mem))
        _lib().hip_cleanup_partial_sum_ciphertexts_vec_64(s, C.byref(mem))
        return (out, pbs) if return_pbs_count else out

    def sum_ciphertexts(self, cts, streams, reduce=True):
        """Sum of a list of one-integer ciphertexts of equal width (radix/mod.rs unchecked_sum_ciphertexts); with
        `reduce` the carries are propagated and the result is clean.  None for an empty list."""
        if not cts:
            return None
        L, n = cts[0].num_blocks, cts[0].lwe_dimension
        assert all(c.num_integers == 1 and c.num_blocks == L and c.lwe_dimension == n for c in cts)
        w = n + 1
        vec = CudaUnsignedRadixCiphertext(CudaVec(len(cts) * L * w, streams), len(cts), L, n)
        for i, c in enumerate(cts):
            _lib().cuda_memcpy_async_gpu_to_gpu(vec.d_blocks.ptr + i * L * w * 8, c.d_blocks.ptr, L * w * 8, streams.ptr[0],
                                                streams.gpu_indexes[0])
            vec._info[0][i * L:(i + 1) * L] = c._info[0]
            vec._info[1][i * L:(i + 1) * L] = c._info[1]
        out = self.unchecked_partial_sum_ciphertexts(vec, streams, reduce=reduce)
        if reduce and len(cts) > 1:
            if len(cts) == 2:    # a plain addition: the blocks hold what the operands held
                assert int(out.degrees.max(initial=0)) <= 2 * self.message_modulus - 2, "sum_ciphertexts: operands are not clean"
            self.propagate_single_carry_assign(out, streams)
        return out


    def mul_by_boolean_assign(self, ct, boolean, streams, boolean_is_left=False):
        """ct <- boolean ? ct : 0, block by block (integer_mult with is_boolean_right; with boolean_is_left the
        roles of the FFI operands are swapped: the boolean sits in the in/out operand, whose blocks receive the
        result — cuda/src/integer/multiplication.cuh:508-520).  `boolean`: one block per integer, value 0 or 1."""
        s, keep = self._streams(streams)
        ksks, bsks = self._key_ptrs(streams)
        mem = C.c_void_p()
        assert boolean.total_blocks == ct.num_integers
        _lib().hip_integer_scratch_batch(ct.num_integers)
        _lib().scratch_cuda_integer_mult_inplace_64_async(
            s, C.byref(mem), boolean_is_left, not boolean_is_left, self.message_modulus, self.carry_modulus,
            self._bsk_params(), self._ksk_params(), ct.num_blocks, True, self._noise_reduction())
        if boolean_is_left:
            # in/out operand: full-width buffer whose first `num_integers` blocks hold the booleans
            out = CudaUnsignedRadixCiphertext.zeros_like(ct, streams)
            w = ct.lwe_dimension + 1
            _lib().cuda_memcpy_async_gpu_to_gpu(out.d_blocks.ptr, boolean.d_blocks.ptr, boolean.total_blocks * w * 8,
                                                streams.ptr[0], streams.gpu_indexes[0])
            _lib().cuda_integer_mult_inplace_64_async(s, C.byref(out._ffi()), True, C.byref(ct._ffi()), False, bsks,
                                                      ksks, mem, self.bootstrapping_key.polynomial_size, ct.num_blocks)
            _lib().cleanup_cuda_integer_mult_inplace_64(s, C.byref(mem))
            return out
        _lib().cuda_integer_mult_inplace_64_async(s, C.byref(ct._ffi()), False, C.byref(boolean._ffi()), True, bsks,
                                                  ksks, mem, self.bootstrapping_key.polynomial_size, ct.num_blocks)
        _lib().cleanup_cuda_integer_mult_inplace_64(s, C.byref(mem))
        return ct


class CudaUnsignedRadixCiphertext:
    """A batch of unsigned radix integers on the device: [integer][block][lwe_size] u64, least
    significant block first (integer/gpu/ciphertext/mod.rs; one reference ciphertext = batch of 1)."""

    def __init__(self, d_blocks: CudaVec, num_integers, num_blocks, lwe_dimension):
        self.d_blocks = d_blocks
        self.num_integers, self.num_blocks, self.lwe_dimension = int(num_integers), int(num_blocks), int(lwe_dimension)
        # degrees / noise levels as the reference's structs carry them; the backend updates them and refuses operands
        # whose degrees exceed what an operation accepts.  Default 1: "not tracked" (callers that track set_degrees)
        self._info = np.ones(self.total_blocks, dtype=U64), np.ones(self.total_blocks, dtype=U64)

    @property
    def total_blocks(self):
        return self.num_integers * self.num_blocks

    def set_degrees(self, degree):
        self._info[0][:] = int(degree)

    @property
    def degrees(self):
        return self._info[0]

    @classmethod
    def from_blocks(cls, h_blocks, streams):
        """h_blocks: [integer][block][lwe_size] ciphertext words produced by the client key."""
        h = np.ascontiguousarray(h_blocks, dtype=U64)
        assert h.ndim == 3
        return cls(CudaVec.from_cpu_async(h.reshape(-1), streams), h.shape[0], h.shape[1], h.shape[2] - 1)

    @classmethod
    def zeros_like(cls, other, streams):
        return cls(CudaVec(other.total_blocks * (other.lwe_dimension + 1), streams), other.num_integers,
                   other.num_blocks, other.lwe_dimension)

    def duplicate(self, streams):
        h = self.to_blocks(streams)
        return CudaUnsignedRadixCiphertext.from_blocks(h, streams)

    def to_blocks(self, streams):
        return self.d_blocks.copy_to_cpu(streams).reshape(self.num_integers, self.num_blocks, self.lwe_dimension + 1)

    def _ffi(self):
        deg, noise = self._info
        return ffi.CudaRadixCiphertextFFI(self.d_blocks.ptr, deg.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          noise.ctypes.data_as(C.POINTER(C.c_uint64)), self.total_blocks,
                                          self.total_blocks, self.lwe_dimension)

    def re_randomize(self, zeros, key, streams):
        """integer/gpu/ciphertext/re_randomization.rs re_randomize: every block gains, in place, a fresh encryption of
        zero.  `zeros`: ONE compact list (CudaLweCompactCiphertextList) of at least total_blocks encryptions of zero under
        the compact public key `key` (a CudaReRandomizationKey) stands for; deriving its words from a seed is the
        caller's.  Blocks must be at nominal noise and stay there; degrees do not change."""
        ksk = key.checked_rerand_ksk(self.lwe_dimension)
        if len(zeros.num_lwe_per_compact_list) != 1 or zeros.n_c != key.zeros_dimension:
            raise ValueError("Mismatched LweDimension between the encryptions of zero and the provided re-randomization "
                             "key: one compact list under its compact public key is expected.")
        if zeros.lwe_ciphertext_count < self.total_blocks:
            raise ValueError("Not enough encryptions of zero to re-randomize every block.")
        if int(self._info[1].max(initial=0)) > 1:
            raise ValueError("Tried to re-randomize a Ciphertext with non-nominal NoiseLevel.")
        s, keep = CudaServerKey._streams(streams)
        if ksk is None:
            params, mode, keys = ffi.CudaLweKeyswitchKeyParamsFFI(key.zeros_dimension, 0, 0, 0), RERAND_WITHOUT_KS, None
        else:
            params = ffi.CudaLweKeyswitchKeyParamsFFI(ksk.input_key_lwe_dimension, ksk.output_key_lwe_dimension,
                                                      ksk.decomp_base_log, ksk.decomp_level_count)
            mode, keys = RERAND_WITH_KS, (C.c_void_p * 1)(ksk.d_vecs[0].ptr)
        mem = C.c_void_p()
        _lib().hip_scratch_rerand_64_async(s, C.byref(mem), params, self.total_blocks, key.message_modulus,
                                           key.carry_modulus, True, mode)
        _lib().hip_rerand_64_async(s, self.d_blocks.ptr, zeros.d_vec.ptr, mem, keys)
        _lib().hip_cleanup_rerand_64(s, C.byref(mem))
        self._info[1][:] = 1


def encrypt_u128_for_aes_ctr(data):
    """radix/aes.rs encrypt_u128_for_aes_ctr, the clear half: the 128 one-bit blocks of a 128-bit key, IV or block, most
    significant bit first (block i holds bit 127 - i).  The caller encrypts each as one block."""
    data = int(data)
    if not 0 <= data < 1 << AES_BLOCK_BITS:
        raise ValueError("an AES block has 128 bits")
    return [(data >> (AES_BLOCK_BITS - 1 - i)) & 1 for i in range(AES_BLOCK_BITS)]


def decrypt_u128_from_aes_ctr(bits, num_aes_inputs):
    """radix/aes.rs decrypt_u128_from_aes_ctr, the clear half: the decrypted blocks of num_aes_inputs outputs back to 128-bit
    integers."""
    bits = [int(b) for b in bits]
    if len(bits) != AES_BLOCK_BITS * num_aes_inputs or any(b not in (0, 1) for b in bits):
        raise ValueError(f"expected {AES_BLOCK_BITS * num_aes_inputs} decrypted bits")
    return [sum(b << (AES_BLOCK_BITS - 1 - i) for i, b in enumerate(bits[AES_BLOCK_BITS * n:AES_BLOCK_BITS * (n + 1)]))
            for n in range(num_aes_inputs)]


class CudaTriviumState:
    """integer/gpu/server_key/radix/trivium.rs CudaTriviumState: the registers a (93 positions), b (84) and c (111) of N
    ciphers side by side, position p of a register at blocks p N .. p N + N - 1, every block an encrypted bit."""

    def __init__(self, a, b, c):
        self.a, self.b, self.c = a, b, c
        counts = [r.total_blocks // bits for r, bits in zip((a, b, c), TRIVIUM_REGISTER_BITS)]
        assert len(set(counts)) == 1 and all(r.total_blocks == bits * counts[0]
                                             for r, bits in zip((a, b, c), TRIVIUM_REGISTER_BITS)), \
            "the registers hold 93, 84 and 111 blocks per input"
        self.num_inputs = counts[0]


# ---------------------------------------------------------------------------------------------- ciphertext compression
# integer/gpu/list_compression/server_keys.rs (CudaCompressionKey, CudaDecompressionKey) and
# integer/gpu/ciphertext/compressed_ciphertext_list.rs (CudaCompressedCiphertextList), over the hip_ entry points of
# include/tfhe_hip_backend.h, "ciphertext compression".
class CudaCompressionKey:
    """server_keys.rs: the packing keyswitch key (big compute key -> compression GLWE key) and how a GLWE is stored."""

    def __init__(self, packing_key_switching_key, lwe_per_glwe, storage_log_modulus, message_modulus, carry_modulus):
        self.packing_key_switching_key = packing_key_switching_key
        self.lwe_per_glwe, self.storage_log_modulus = int(lwe_per_glwe), int(storage_log_modulus)
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)
        assert 1 <= self.lwe_per_glwe <= packing_key_switching_key.output_polynomial_size, \
            "Cannot pack more than polynomial_size elements per glwe"

    def compress_ciphertexts_into_list(self, ciphertexts, streams):
        """`ciphertexts`: radix ciphertexts (one integer each, any widths) with empty carries.  Their blocks are laid
        end to end, multiplied by message_modulus, packed lwe_per_glwe per GLWE, modulus switched and bit-packed."""
        k = self.packing_key_switching_key
        counts = []
        for ct in ciphertexts:
            assert ct.num_integers == 1, "one integer per list entry"
            assert ct.lwe_dimension == k.input_key_lwe_dimension, \
                "All ciphertexts do not have the same lwe size as the packing keyswitch key"
            if int(ct.degrees.max(initial=0)) > self.message_modulus - 1:
                raise ValueError("Ciphertexts must have empty carries to be compressed")
            counts.append(ct.total_blocks)
        total = sum(counts)
        assert total >= 1, "nothing to compress"
        w = k.input_key_lwe_dimension + 1
        s, keep = CudaServerKey._streams(streams)
        flat = CudaUnsignedRadixCiphertext(CudaVec(total * w, streams), 1, total, k.input_key_lwe_dimension)
        at = 0
        for ct, c in zip(ciphertexts, counts):
            _lib().cuda_memcpy_async_gpu_to_gpu(flat.d_blocks.ptr + at * w * 8, ct.d_blocks.ptr, c * w * 8, streams.ptr[0],
                                                streams.gpu_indexes[0])
            flat.degrees[at:at + c] = ct.degrees
            at += c
        words = int(_lib().hip_integer_compressed_size_words(k.output_glwe_dimension, k.output_polynomial_size,
                                                             self.lwe_per_glwe, self.storage_log_modulus, total))
        packed = CudaVec(words, streams)
        mem = C.c_void_p()
        keys = (C.c_void_p * 1)(k.d_vec.ptr)
        _lib().hip_scratch_integer_compress_radix_ciphertext_64_async(
            s, C.byref(mem), k.input_key_lwe_dimension, k.output_glwe_dimension, k.output_polynomial_size,
            k.decomp_base_log, k.decomp_level_count, total, self.message_modulus, self.carry_modulus, self.lwe_per_glwe,
            self.storage_log_modulus, True)
        _lib().hip_integer_compress_radix_ciphertext_64_async(s, packed.ptr, C.byref(flat._ffi()), keys, mem)
        _lib().hip_cleanup_integer_compress_radix_ciphertext_64(s, C.byref(mem))
        return CudaCompressedCiphertextList(packed, counts, k.output_glwe_dimension, k.output_polynomial_size,
                                            self.lwe_per_glwe, self.storage_log_modulus, self.message_modulus,
                                            self.carry_modulus)


class CudaDecompressionKey:
    """server_keys.rs: the bootstrap key from the (flattened) compression GLWE key to the compute GLWE key — a
    CudaLweBootstrapKey or CudaLweMultiBitBootstrapKey whose input dimension is glwe_dimension * polynomial_size of the
    compression GLWE."""

    def __init__(self, blind_rotate_key, message_modulus, carry_modulus):
        self.blind_rotate_key = blind_rotate_key
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)

    def _bsk_params(self):
        b = self.blind_rotate_key
        g = getattr(b, "grouping_factor", 0)
        return ffi.CudaLweBootstrapKeyParamsFFI(b.input_lwe_dimension, b.glwe_dimension, b.polynomial_size,
                                                b.decomp_base_log, b.decomp_level_count, b.output_lwe_dimension,
                                                PBS_TYPE_MULTI_BIT if g else PBS_TYPE_CLASSICAL, g)

    def unpack_indexes(self, packed, indexes, streams):
        """The blocks at `indexes` of the packed list (non-decreasing in GLWE index), decompressed: one integer of
        len(indexes) clean blocks under the big compute key."""
        b = self.blind_rotate_key
        assert b.input_lwe_dimension == packed.glwe_dimension * packed.polynomial_size, \
            "decompression key and compressed list do not have the same compression GLWE"
        assert (packed.message_modulus, packed.carry_modulus) == (self.message_modulus, self.carry_modulus)
        idx = np.ascontiguousarray(indexes, dtype=np.uint32)
        s, keep = CudaServerKey._streams(streams)
        out = CudaUnsignedRadixCiphertext(CudaVec(idx.size * (b.output_lwe_dimension + 1), streams), 1, idx.size,
                                          b.output_lwe_dimension)
        mem = C.c_void_p()
        keys = (C.c_void_p * 1)(b.d_vec.ptr)
        _lib().hip_scratch_integer_decompress_radix_ciphertext_64_async(
            s, C.byref(mem), self._bsk_params(), packed.glwe_dimension, packed.polynomial_size, packed.lwe_per_glwe,
            packed.storage_log_modulus, idx.size, self.message_modulus, self.carry_modulus, True,
            1 if getattr(b, "ms_noise_reduction", False) else 0)
        _lib().hip_integer_decompress_radix_ciphertext_64_async(
            s, C.byref(out._ffi()), packed.d_packed.ptr, packed.total_blocks, idx.ctypes.data_as(C.POINTER(C.c_uint32)),
            idx.size, keys, mem)
        _lib().hip_cleanup_integer_decompress_radix_ciphertext_64(s, C.byref(mem))   # synchronises: idx may go
        return out

    def unpack(self, packed, start_block, end_block, streams):
        """server_keys.rs unpack: blocks [start_block, end_block) of the list as one radix ciphertext."""
        return self.unpack_indexes(packed, np.arange(start_block, end_block), streams)


class CudaCompressedCiphertextList:
    """The packed words on the device plus what unpacking needs: how many blocks every entry has, the compression GLWE
    shape, lwe_per_glwe, storage_log_modulus and the moduli (CompressedCiphertextListMeta, compression.rs:121-127)."""

    def __init__(self, d_packed, block_counts, glwe_dimension, polynomial_size, lwe_per_glwe, storage_log_modulus,
                 message_modulus, carry_modulus):
        self.d_packed = d_packed
        self.block_counts = [int(c) for c in block_counts]
        self.glwe_dimension, self.polynomial_size = int(glwe_dimension), int(polynomial_size)
        self.lwe_per_glwe, self.storage_log_modulus = int(lwe_per_glwe), int(storage_log_modulus)
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)

    @classmethod
    def compress(cls, ciphertexts, compression_key, streams):
        return compression_key.compress_ciphertexts_into_list(ciphertexts, streams)

    @property
    def total_blocks(self):
        return sum(self.block_counts)

    def __len__(self):
        return len(self.block_counts)

    def get(self, i, decompression_key, streams):
        """Entry i as a radix ciphertext (compressed_ciphertext_list.rs get)."""
        if not 0 <= i < len(self):
            raise IndexError(f"Tried getting index {i} for CudaCompressedCiphertextList with {len(self)} elements")
        start = sum(self.block_counts[:i])
        return decompression_key.unpack(self, start, start + self.block_counts[i], streams)

    def size_bytes(self):
        return 8 * self.d_packed.len

    def metadata(self):
        return {"block_counts": list(self.block_counts), "glwe_dimension": self.glwe_dimension,
                "polynomial_size": self.polynomial_size, "lwe_per_glwe": self.lwe_per_glwe,
                "storage_log_modulus": self.storage_log_modulus, "message_modulus": self.message_modulus,
                "carry_modulus": self.carry_modulus}

    def to_host(self, streams):
        """(packed u64 words, metadata dict)"""
        return self.d_packed.copy_to_cpu(streams), self.metadata()

    @classmethod
    def from_host(cls, words, metadata, streams):
        words = np.ascontiguousarray(words, dtype=U64)
        m = metadata
        want = int(_lib().hip_integer_compressed_size_words(m["glwe_dimension"], m["polynomial_size"], m["lwe_per_glwe"],
                                                            m["storage_log_modulus"], sum(m["block_counts"])))
        assert words.size == want, "packed words do not have the size the metadata describes"
        return cls(CudaVec.from_cpu_async(words, streams), m["block_counts"], m["glwe_dimension"], m["polynomial_size"],
                   m["lwe_per_glwe"], m["storage_log_modulus"], m["message_modulus"], m["carry_modulus"])


# ---------------------------------------------------------------------------------------------- noise squashing
# integer/gpu/noise_squashing/keys.rs (CudaNoiseSquashingKey) and integer/gpu/ciphertext/squashed_noise.rs
# (CudaSquashedNoiseRadixCiphertext), over the hip_ entry points of include/tfhe_hip_backend.h, "128-bit PBS and noise
# squashing".
class CudaSquashedNoiseRadixCiphertext:
    """ceil(blocks / 2) u128 LWE blocks under the squashing key's output key, each holding lo + message_modulus * hi of a
    pair of input blocks; [block][lwe_size][2] uint64 on the host."""

    def __init__(self, d_blocks: CudaVec, num_blocks, lwe_dimension, original_block_count):
        self.d_blocks = d_blocks
        self.num_blocks, self.lwe_dimension = int(num_blocks), int(lwe_dimension)
        self.original_block_count = int(original_block_count)
        self._info = np.ones(self.num_blocks, dtype=U64), np.ones(self.num_blocks, dtype=U64)

    def to_blocks(self, streams):
        return self.d_blocks.copy_to_cpu(streams).reshape(self.num_blocks, self.lwe_dimension + 1, 2)

    def _ffi(self):
        deg, noise = self._info
        return ffi.CudaRadixCiphertextFFI(self.d_blocks.ptr, deg.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          noise.ctypes.data_as(C.POINTER(C.c_uint64)), self.num_blocks, self.num_blocks,
                                          self.lwe_dimension)


class CudaNoiseSquashingKey:
    """keys.rs: the u128 bootstrap key (a CudaLweBootstrapKey128 or a CudaLweMultiBitBootstrapKey128 from the compute set's
    small key to the squashing GLWE key) and the moduli of the blocks it squashes."""

    def __init__(self, bootstrapping_key, message_modulus, carry_modulus):
        self.bootstrapping_key = bootstrapping_key
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)

    def squash_radix_ciphertext_noise(self, src_server_key, ciphertext, streams):
        """One integer with empty carries -> its squashed form: pack block pairs, keyswitch with the server key's
        keyswitch key, bootstrap over the 128-bit torus with the identity table.  `ciphertext` is left unchanged."""
        b, k = self.bootstrapping_key, src_server_key.key_switching_key
        assert ciphertext.num_integers == 1, "one integer per call"
        assert k.output_key_lwe_dimension == b.input_lwe_dimension, "keyswitch and squashing keys do not chain"
        assert ciphertext.lwe_dimension == k.input_key_lwe_dimension, "Mismatched input LweDimension"
        if int(ciphertext.degrees.max(initial=0)) > self.message_modulus - 1:
            raise ValueError("Ciphertexts must have empty carries to be squashed")
        n_in = ciphertext.total_blocks
        n_out = (n_in + 1) // 2
        out = CudaSquashedNoiseRadixCiphertext(CudaVec(n_out * (b.output_lwe_dimension + 1), streams, elem_words=2), n_out,
                                               b.output_lwe_dimension, n_in)
        s, keep = CudaServerKey._streams(streams)
        mem = C.c_void_p()
        ksks, bsks = (C.c_void_p * 1)(k.d_vec.ptr), (C.c_void_p * 1)(b.d_vec.ptr)
        big = src_server_key.bootstrapping_key
        lib = _lib()
        shape = (s, C.byref(mem), b.input_lwe_dimension, b.glwe_dimension, b.polynomial_size, big.glwe_dimension,
                 big.polynomial_size, k.decomp_level_count, k.decomp_base_log, b.decomp_level_count, b.decomp_base_log, n_out,
                 n_in, self.message_modulus, self.carry_modulus, True)
        if isinstance(b, CudaLweMultiBitBootstrapKey128):   # the scratch remembers its kind: apply and cleanup serve both
            lib.hip_scratch_integer_apply_noise_squashing_multi_bit_64_async(*shape, 0, b.grouping_factor)
        else:
            lib.hip_scratch_integer_apply_noise_squashing_64_async(*shape, 1 if b.ms_noise_reduction else 0)
        lib.hip_integer_apply_noise_squashing_64_async(s, C.byref(out._ffi()), C.byref(ciphertext._ffi()), mem, ksks, bsks)
        lib.hip_cleanup_integer_apply_noise_squashing_64(s, C.byref(mem))
        return out


def squash_radix_ciphertext_noise(noise_squashing_key, src_server_key, ciphertext, streams):
    return noise_squashing_key.squash_radix_ciphertext_noise(src_server_key, ciphertext, streams)


# ---------------------------------------------------------------------------------------------- squashed-noise list compression
# integer/gpu/list_compression/server_keys.rs (CudaNoiseSquashingCompressionKey) and
# integer/gpu/ciphertext/compressed_noise_squashed_ciphertext_list.rs (CudaCompressedSquashedNoiseCiphertextList), over the
# hip_ entry points of include/tfhe_hip_backend.h, "compression of squashed-noise lists".  Unpacking needs no key and no
# bootstrap: a sample extract of the packed GLWE.
STORAGE_LOG_MODULUS_128 = 128   # noise_squashing_compression.rs: the ciphertext modulus itself (the switch is the identity)


class CudaNoiseSquashingCompressionKey:
    """server_keys.rs: the u128 packing keyswitch key (squashing GLWE key, flattened -> compression GLWE key) and how many
    squashed blocks go into one GLWE."""

    def __init__(self, packing_key_switching_key, lwe_per_glwe, message_modulus, carry_modulus,
                 storage_log_modulus=STORAGE_LOG_MODULUS_128):
        self.packing_key_switching_key = packing_key_switching_key
        self.lwe_per_glwe, self.storage_log_modulus = int(lwe_per_glwe), int(storage_log_modulus)
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)
        assert 1 <= self.lwe_per_glwe <= packing_key_switching_key.output_polynomial_size, \
            "Cannot pack more than polynomial_size elements per glwe"

    def compress_noise_squashed_ciphertexts_into_list(self, ciphertexts, streams):
        """`ciphertexts`: CudaSquashedNoiseRadixCiphertext (any block counts).  Their blocks are laid end to end, packed
        lwe_per_glwe per GLWE, switched to storage_log_modulus bits and bit-packed."""
        k = self.packing_key_switching_key
        for ct in ciphertexts:
            assert ct.lwe_dimension == k.input_key_lwe_dimension, \
                "All ciphertexts do not have the same lwe size as the packing keyswitch key"
        counts = [ct.num_blocks for ct in ciphertexts]
        originals = [ct.original_block_count for ct in ciphertexts]
        total = sum(counts)
        assert total >= 1, "nothing to compress"
        w = (k.input_key_lwe_dimension + 1) * 16   # bytes of one u128 block
        s, keep = CudaServerKey._streams(streams)
        flat = CudaSquashedNoiseRadixCiphertext(CudaVec(total * (k.input_key_lwe_dimension + 1), streams, elem_words=2),
                                                total, k.input_key_lwe_dimension, 2 * total)
        at = 0
        for ct, c in zip(ciphertexts, counts):
            _lib().cuda_memcpy_async_gpu_to_gpu(flat.d_blocks.ptr + at * w, ct.d_blocks.ptr, c * w, streams.ptr[0],
                                                streams.gpu_indexes[0])
            at += c
        words = int(_lib().hip_integer_compressed_size_words_128(k.output_glwe_dimension, k.output_polynomial_size,
                                                                 self.lwe_per_glwe, self.storage_log_modulus, total))
        packed = CudaVec(words, streams, elem_words=2)
        mem = C.c_void_p()
        keys = (C.c_void_p * 1)(k.d_vec.ptr)
        planes = (C.c_void_p * 1)(k.planes_ptr)
        _lib().hip_scratch_integer_compress_radix_ciphertext_128_async(
            s, C.byref(mem), k.input_key_lwe_dimension, k.output_glwe_dimension, k.output_polynomial_size,
            k.decomp_base_log, k.decomp_level_count, total, self.message_modulus, self.carry_modulus, self.lwe_per_glwe,
            self.storage_log_modulus, True)
        _lib().hip_integer_compress_radix_ciphertext_128_async(s, packed.ptr, C.byref(flat._ffi()), keys, planes, mem)
        _lib().hip_cleanup_integer_compress_radix_ciphertext_128(s, C.byref(mem))
        return CudaCompressedSquashedNoiseCiphertextList(packed, counts, originals, k.output_glwe_dimension,
                                                         k.output_polynomial_size, self.lwe_per_glwe,
                                                         self.storage_log_modulus, self.message_modulus, self.carry_modulus)


class CudaCompressedSquashedNoiseCiphertextList:
    """The packed u128 words on the device plus what unpacking needs: the squashed block count and the original block
    count of every entry, the compression GLWE shape, lwe_per_glwe, storage_log_modulus and the moduli
    (CompressedSquashedNoiseCiphertextListMeta)."""

    def __init__(self, d_packed, block_counts, original_block_counts, glwe_dimension, polynomial_size, lwe_per_glwe,
                 storage_log_modulus, message_modulus, carry_modulus):
        self.d_packed = d_packed
        self.block_counts = [int(c) for c in block_counts]
        self.original_block_counts = [int(c) for c in original_block_counts]
        self.glwe_dimension, self.polynomial_size = int(glwe_dimension), int(polynomial_size)
        self.lwe_per_glwe, self.storage_log_modulus = int(lwe_per_glwe), int(storage_log_modulus)
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)

    class Builder:
        """compressed_noise_squashed_ciphertext_list.rs builder(): push squashed ciphertexts, then build with a key"""

        def __init__(self):
            self.ciphertexts = []

        def push(self, ciphertext):
            assert isinstance(ciphertext, CudaSquashedNoiseRadixCiphertext)
            self.ciphertexts.append(ciphertext)
            return self

        def build(self, compression_key, streams):
            return compression_key.compress_noise_squashed_ciphertexts_into_list(self.ciphertexts, streams)

    @classmethod
    def builder(cls):
        return cls.Builder()

    @property
    def total_blocks(self):
        return sum(self.block_counts)

    def __len__(self):
        return len(self.block_counts)

    def unpack_indexes(self, indexes, streams, original_block_count=None):
        """The squashed blocks at `indexes` (non-decreasing in GLWE index) as one CudaSquashedNoiseRadixCiphertext of LWE
        dimension glwe_dimension * polynomial_size."""
        idx = np.ascontiguousarray(indexes, dtype=np.uint32)
        dim = self.glwe_dimension * self.polynomial_size
        s, keep = CudaServerKey._streams(streams)
        out = CudaSquashedNoiseRadixCiphertext(CudaVec(max(idx.size, 1) * (dim + 1), streams, elem_words=2), idx.size, dim,
                                               2 * idx.size if original_block_count is None else original_block_count)
        mem = C.c_void_p()
        _lib().hip_scratch_integer_decompress_radix_ciphertext_128_async(
            s, C.byref(mem), self.glwe_dimension, self.polynomial_size, self.lwe_per_glwe, self.storage_log_modulus,
            idx.size, self.message_modulus, self.carry_modulus, True)
        _lib().hip_integer_decompress_radix_ciphertext_128_async(
            s, C.byref(out._ffi()), self.d_packed.ptr, self.total_blocks, idx.ctypes.data_as(C.POINTER(C.c_uint32)),
            idx.size, mem)
        _lib().hip_cleanup_integer_decompress_radix_ciphertext_128(s, C.byref(mem))   # synchronises: idx may go
        return out

    def get(self, i, streams):
        """Entry i with its original block count (compressed_noise_squashed_ciphertext_list.rs get)."""
        if not 0 <= i < len(self):
            raise IndexError(f"Tried getting index {i} for CudaCompressedSquashedNoiseCiphertextList with {len(self)} elements")
        start = sum(self.block_counts[:i])
        return self.unpack_indexes(np.arange(start, start + self.block_counts[i]), streams, self.original_block_counts[i])

    def size_bytes(self):
        return 16 * self.d_packed.len

    def metadata(self):
        return {"block_counts": list(self.block_counts), "original_block_counts": list(self.original_block_counts),
                "glwe_dimension": self.glwe_dimension, "polynomial_size": self.polynomial_size,
                "lwe_per_glwe": self.lwe_per_glwe, "storage_log_modulus": self.storage_log_modulus,
                "message_modulus": self.message_modulus, "carry_modulus": self.carry_modulus}

    def to_host(self, streams):
        """(packed u128 words as [words][2] uint64, metadata dict)"""
        return self.d_packed.copy_to_cpu(streams), self.metadata()

    @classmethod
    def from_host(cls, words, metadata, streams):
        words = np.ascontiguousarray(words, dtype=U64).reshape(-1, 2)
        m = metadata
        want = int(_lib().hip_integer_compressed_size_words_128(m["glwe_dimension"], m["polynomial_size"], m["lwe_per_glwe"],
                                                                m["storage_log_modulus"], sum(m["block_counts"])))
        assert words.shape[0] == want, "packed words do not have the size the metadata describes"
        return cls(CudaVec.from_cpu_async(words, streams, elem_words=2), m["block_counts"], m["original_block_counts"],
                   m["glwe_dimension"], m["polynomial_size"], m["lwe_per_glwe"], m["storage_log_modulus"],
                   m["message_modulus"], m["carry_modulus"])


# ---------------------------------------------------------------------------------------------- compact list expansion
# integer/gpu/key_switching_key.rs (CudaKeySwitchingKey) and integer/gpu/ciphertext/compact_list.rs
# (CudaFlattenedVecCompactCiphertextList, CudaCompactCiphertextListExpander), over the hip_ entry points of
# include/tfhe_hip_backend.h, "expansion of compact ciphertext lists".
class CudaKeySwitchingKey:
    """key_switching_key.rs: the casting key from the public-key encryption key to a key of the destination server key
    ("small": its bootstrap key's input key, "big": its GLWE key), with its decomposition, and the destination server key."""

    def __init__(self, lwe_keyswitch_key: CudaLweKeyswitchKey, destination_key, dest_server_key: CudaServerKey):
        assert destination_key in ("small", "big"), "destination_key: 'small' or 'big'"
        want = (dest_server_key.bootstrapping_key.input_lwe_dimension if destination_key == "small"
                else dest_server_key.bootstrapping_key.output_lwe_dimension)
        assert lwe_keyswitch_key.output_key_lwe_dimension == want, "the casting key does not end on the destination key"
        self.lwe_keyswitch_key, self.destination_key, self.dest_server_key = lwe_keyswitch_key, destination_key, dest_server_key

    def _params(self):
        k = self.lwe_keyswitch_key
        return ffi.CudaLweKeyswitchKeyParamsFFI(k.input_key_lwe_dimension, k.output_key_lwe_dimension, k.decomp_base_log,
                                                k.decomp_level_count)

    def _ks_type(self):
        return KS_TYPE_BIG_TO_SMALL if self.destination_key == "small" else KS_TYPE_SMALL_TO_BIG


class CudaFlattenedVecCompactCiphertextList:
    """compact_list.rs: compact lists end to end on the device and what they hold.  `data_info`: one entry per encrypted
    value, ("unsigned", blocks) or ("boolean",); the blocks of all values, in order, are packed two per body (block 2j +
    message_modulus * block 2j + 1 in body j), so ceil(blocks / 2) bodies in all."""

    def __init__(self, d_list: CudaLweCompactCiphertextList, data_info, message_modulus, carry_modulus):
        self.d_list = d_list
        self.data_info = [tuple(e) for e in data_info]
        for e in self.data_info:
            assert e[0] in ("unsigned", "boolean"), f"data kind {e[0]!r} is not supported"
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)
        total = self.total_blocks
        assert d_list.lwe_ciphertext_count == (total + 1) // 2, \
            "the lists do not hold one body per pair of blocks of the data they are said to hold"
        # which expanded block is a boolean; padded with False to the two blocks every body expands to
        flags = [e[0] == "boolean" for e in self.data_info for _ in range(self._blocks(e))]
        self.is_boolean = flags + [False] * (2 * d_list.lwe_ciphertext_count - len(flags))

    @staticmethod
    def _blocks(entry):
        return 1 if entry[0] == "boolean" else int(entry[1])

    @property
    def total_blocks(self):
        return sum(self._blocks(e) for e in self.data_info)

    @property
    def num_lwe_per_compact_list(self):
        return self.d_list.num_lwe_per_compact_list

    @classmethod
    def from_flat_words(cls, words, n_c, num_lwe_per_compact_list, data_info, message_modulus, carry_modulus, streams):
        return cls(CudaLweCompactCiphertextList.from_flat_words(words, n_c, num_lwe_per_compact_list, streams), data_info,
                   message_modulus, carry_modulus)

    def __len__(self):
        return len(self.data_info)

    def get_kind_of(self, i):
        return self.data_info[i] if 0 <= i < len(self.data_info) else None

    def expand(self, key: CudaKeySwitchingKey, streams, kind="casting"):
        """compact_list.rs expand: every body rotated out of its list's mask, cast with `key` and split into its two
        blocks by one bootstrap round of the destination server key.  kind "sanity_check": the identity table instead
        of the split; "no_casting": the expanded LWEs under the encryption key, returned as a CudaLweCiphertextList."""
        from .core_crypto_gpu import CudaLweCiphertextList
        sks, casting, d = key.dest_server_key, key.lwe_keyswitch_key, self.d_list
        assert casting.input_key_lwe_dimension == d.n_c, "the casting key does not start on the lists' encryption key"
        assert (sks.message_modulus, sks.carry_modulus) == (self.message_modulus, self.carry_modulus)
        bsk = sks.bootstrapping_key
        bk = sks._bsk_params()
        n = d.lwe_ciphertext_count
        s, keep = CudaServerKey._streams(streams)
        counts = (C.c_uint32 * len(d.num_lwe_per_compact_list))(*d.num_lwe_per_compact_list)
        flags = (C.c_bool * len(self.is_boolean))(*self.is_boolean)
        out_dim = d.n_c if kind == "no_casting" else bsk.output_lwe_dimension
        out_count = n if kind == "no_casting" else 2 * n
        d_out = CudaLweCiphertextList.new(out_dim, out_count, streams)
        ksks, bsks = sks._key_ptrs(streams)
        nk = len(streams) if key.destination_key == "small" else 1
        assert len(casting.d_vecs) >= nk, "casting key has fewer GPU replicas than the stream set has streams"
        casts = (C.c_void_p * nk)(*[v.ptr for v in casting.d_vecs[:nk]])
        mem = C.c_void_p()
        _lib().hip_scratch_expand_without_verification_64_async(
            s, C.byref(mem), bsk.glwe_dimension, bsk.polynomial_size, sks._ksk_params(), key._params(),
            bsk.decomp_level_count, bsk.decomp_base_log, bk.grouping_factor, counts, flags, len(self.is_boolean),
            len(d.num_lwe_per_compact_list), self.message_modulus, self.carry_modulus, bk.pbs_type, key._ks_type(), True,
            EXPAND_KIND[kind], sks._noise_reduction())
        _lib().hip_expand_without_verification_64_async(s, d_out.d_vec.ptr, d.d_vec.ptr, mem, bsks, ksks, casts)
        _lib().hip_cleanup_expand_without_verification_64(s, C.byref(mem))
        if kind == "no_casting":
            return d_out
        return CudaCompactCiphertextListExpander(d_out, self.data_info, self.message_modulus, self.carry_modulus)


class CudaCompactCiphertextListExpander:
    """compact_list.rs: the expanded blocks (one LWE per block of the data, in order, under the big compute key) and
    what they hold."""

    def __init__(self, expanded_blocks, data_info, message_modulus, carry_modulus):
        self.expanded_blocks = expanded_blocks
        self.data_info = list(data_info)
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)

    def __len__(self):
        return len(self.data_info)

    def get_kind_of(self, i):
        return self.data_info[i] if 0 <= i < len(self.data_info) else None

    def get(self, i, streams):
        """Entry i: an unsigned integer as a CudaUnsignedRadixCiphertext of its blocks (degree message_modulus - 1), a
        boolean as one of a single block (degree 1); noise level nominal.  None past the end, as the reference."""
        if not 0 <= i < len(self.data_info):
            return None
        blocks = CudaFlattenedVecCompactCiphertextList._blocks
        start, count = sum(blocks(e) for e in self.data_info[:i]), blocks(self.data_info[i])
        dim = self.expanded_blocks.lwe_dimension
        w = (dim + 1) * 8
        out = CudaUnsignedRadixCiphertext(CudaVec(count * (dim + 1), streams), 1, count, dim)
        _lib().cuda_memcpy_async_gpu_to_gpu(out.d_blocks.ptr, self.expanded_blocks.d_vec.ptr + start * w, count * w,
                                            streams.ptr[0], streams.gpu_indexes[0])
        out.set_degrees(1 if self.data_info[i][0] == "boolean" else self.message_modulus - 1)
        out.is_boolean = self.data_info[i][0] == "boolean"
        return out


# ---------------------------------------------------------------------------------------------- re-randomisation, OPRF
# integer/gpu/ciphertext/re_randomization.rs (CudaReRandomizationKey) and integer/gpu/server_key/radix/oprf.rs
# (CudaOprfServerKey), over the hip_ entry points of include/tfhe_hip_backend.h, "re-randomisation" and "oblivious
# pseudo-random bits".  Deriving words from a seed (the XOF) is host work in the reference too: callers pass the words.
class CudaReRandomizationKey:
    """re_randomization.rs CudaReRandomizationKey: `zeros_dimension` is the LWE dimension of the compact public key the
    encryptions of zero are made with.  With `ksk` (a CudaLweKeyswitchKey from that key to the blocks' key):
    LegacyDedicatedCPK; without: DerivedCPKWithoutKeySwitch, the public key is derived from the compute key itself."""

    def __init__(self, zeros_dimension, ksk=None, message_modulus=4, carry_modulus=4):
        self.zeros_dimension, self.ksk = int(zeros_dimension), ksk
        self.message_modulus, self.carry_modulus = int(message_modulus), int(carry_modulus)
        if ksk is not None and ksk.input_key_lwe_dimension != self.zeros_dimension:
            raise ValueError("Mismatched LweDimension between the provided CompactPublicKey and the re-randomization "
                             "keyswitch key input.")

    def checked_rerand_ksk(self, radix_block_lwe_dimension):
        """re_randomization.rs:36-86: the keyswitch key (or None) once the dimensions are known to match; the backend
        expands the zeros at that dimension, a mismatch would read out of bounds."""
        if self.ksk is not None:
            if self.ksk.output_key_lwe_dimension != radix_block_lwe_dimension:
                raise ValueError("Mismatched LweSize between the ciphertext being re-randomized and the provided "
                                 "re-randomization keyswitch key output.")
            return self.ksk
        if self.zeros_dimension != radix_block_lwe_dimension:
            raise ValueError("Mismatched LweSize between the ciphertext being re-randomized and the provided "
                             "CompactPublicKey.")
        return None


class CudaOprfServerKey:
    """oprf.rs: the bootstrap key of the oblivious pseudo-random function, from the key the seeded LWEs are read under
    (the small compute key) to the big compute key — a CudaLweBootstrapKey or CudaLweMultiBitBootstrapKey."""

    def __init__(self, bsk):
        self.bootstrapping_key = bsk

    def generate_oblivious_pseudo_random_bits(self, seeded_lwes, total_random_bits, server_key, streams, rerand=None):
        """`seeded_lwes`: [blocks][input dimension + 1] words derived from a seed, multiples of 2^64 / 2N, blocks =
        ceil(total_random_bits / message bits).  Returns one radix integer whose blocks hold the random bits (the last
        block what remains), degrees 2^bits - 1, nominal noise.  `rerand`: (zeros, CudaReRandomizationKey) to
        re-randomise the fresh blocks, as the reference's OPRF can."""
        b = self.bootstrapping_key
        g = getattr(b, "grouping_factor", 0)
        seeded = np.ascontiguousarray(seeded_lwes, dtype=U64)
        assert seeded.ndim == 2 and seeded.shape[1] == b.input_lwe_dimension + 1, \
            "seeded LWEs do not have the OPRF key's input dimension"
        blocks = seeded.shape[0]
        bk = ffi.CudaLweBootstrapKeyParamsFFI(b.input_lwe_dimension, b.glwe_dimension, b.polynomial_size, b.decomp_base_log,
                                              b.decomp_level_count, b.output_lwe_dimension,
                                              PBS_TYPE_MULTI_BIT if g else PBS_TYPE_CLASSICAL, g)
        s, keep = CudaServerKey._streams(streams)
        n = len(streams)
        assert len(b.d_vecs) >= n, "OPRF key has fewer GPU replicas than the stream set has streams"
        bsks = (C.c_void_p * n)(*[v.ptr for v in b.d_vecs[:n]])
        d_in = CudaVec.from_cpu_async(seeded.reshape(-1), streams)
        out = CudaUnsignedRadixCiphertext(CudaVec(blocks * (b.output_lwe_dimension + 1), streams), 1, blocks,
                                          b.output_lwe_dimension)
        mem = C.c_void_p()
        _lib().hip_scratch_integer_grouped_oprf_64_async(
            s, C.byref(mem), bk, server_key._ksk_params(), blocks, server_key.message_modulus, server_key.carry_modulus,
            True, int(total_random_bits), 1 if getattr(b, "ms_noise_reduction", False) else 0)
        _lib().hip_integer_grouped_oprf_64_async(s, C.byref(out._ffi()), d_in.ptr, blocks, mem, bsks)
        _lib().hip_cleanup_integer_grouped_oprf_64(s, C.byref(mem))
        if rerand is not None:
            zeros, key = rerand
            out.re_randomize(zeros, key, streams)
        return out

    def generate_oblivious_pseudo_random_unsigned_custom_range(self, seeded_lwes, num_input_random_bits,
                                                               excluded_upper_bound, num_blocks_output, server_key, streams,
                                                               rerand=None):
        """oprf.rs par_generate_oblivious_pseudo_random_unsigned_custom_range, the flow of cuda/src/integer/oprf.cuh:127-176
        as a composition of this layer's operations: `num_input_random_bits` oblivious random bits r (re-randomised when
        `rerand` is given), extended with zero blocks to ceil((num_input_random_bits + bit length of the bound) /
        message bits) blocks, multiplied by the bound, shifted right by num_input_random_bits, then truncated or
        zero-extended to `num_blocks_output` blocks: (r * bound) >> num_input_random_bits, a value below the bound."""
        bound, nbits = int(excluded_upper_bound), int(num_input_random_bits)
        assert bound >= 1 and nbits >= 1 and num_blocks_output >= 1
        msg_bits = server_key.message_modulus.bit_length() - 1
        ct = self.generate_oblivious_pseudo_random_bits(seeded_lwes, nbits, server_key, streams, rerand=rerand)
        inter = -(-(nbits + bound.bit_length()) // msg_bits)
        w = ct.lwe_dimension + 1

        def resized(src, blocks):
            """the first `blocks` blocks of src, zero blocks (degree 0) behind them"""
            dst = CudaUnsignedRadixCiphertext(CudaVec(blocks * w, streams), 1, blocks, src.lwe_dimension)
            keep = min(blocks, src.num_blocks)
            _lib().cuda_memcpy_async_gpu_to_gpu(dst.d_blocks.ptr, src.d_blocks.ptr, keep * w * 8, streams.ptr[0],
                                                streams.gpu_indexes[0])
            dst._info[0][:], dst._info[1][:] = 0, 0
            dst._info[0][:keep], dst._info[1][:keep] = src._info[0][:keep], src._info[1][:keep]
            return dst

        work = resized(ct, inter)
        server_key.scalar_mul_assign(work, bound, streams)
        server_key.scalar_shift_assign(work, nbits, streams, left=False)
        return work if num_blocks_output == inter else resized(work, num_blocks_output)
