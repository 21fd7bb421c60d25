"""Host-side mirror of `tfhe::core_crypto::gpu` for the PBS hot path, over the C ABI.

Same names, argument meaning and error behaviour (assertions on mismatched dimensions) as
the Rust module it mirrors:
  CudaStreams                 tfhe/src/core_crypto/gpu/mod.rs:33-150
  CudaVec                     tfhe/src/core_crypto/gpu/vec.rs
  CudaLweCiphertextList       tfhe/src/core_crypto/gpu/entities/lwe_ciphertext_list.rs
  CudaGlweCiphertextList      tfhe/src/core_crypto/gpu/entities/glwe_ciphertext_list.rs
  CudaLweBootstrapKey         tfhe/src/core_crypto/gpu/entities/lwe_bootstrap_key.rs:57-104
  CudaLweMultiBitBootstrapKey tfhe/src/core_crypto/gpu/entities/lwe_multi_bit_bootstrap_key.rs
  CudaLweKeyswitchKey         tfhe/src/core_crypto/gpu/entities/lwe_keyswitch_key.rs
  cuda_programmable_bootstrap_lwe_ciphertext           gpu/algorithms/lwe_programmable_bootstrapping.rs:10-136
  cuda_multi_bit_programmable_bootstrap_lwe_ciphertext gpu/algorithms/lwe_multi_bit_programmable_bootstrapping.rs:10-145
  cuda_keyswitch_lwe_ciphertext                        gpu/algorithms/lwe_keyswitch.rs:12-143
  cuda_extract_lwe_samples_from_glwe_ciphertext_list   gpu/algorithms/glwe_sample_extraction.rs:12
  CudaLweBootstrapKey128 / cuda_programmable_bootstrap_128_lwe_ciphertext   the u128 bootstrap of noise squashing
  CudaLweMultiBitBootstrapKey128 / cuda_multi_bit_programmable_bootstrap_128_lwe_ciphertext   the same on a multi-bit key
  cuda_fourier_transform_{forward_as_torus,forward_as_integer,backward_as_torus}_f128   gpu/ffi.rs, fft/fft128.h
The Rust original is the reference's host language; no Rust toolchain exists in this image,
so the mirror is Python (INTEGRATION.md shows the Rust binding a maintainer would add).
numpy arrays are the "CPU containers".
"""
import ctypes as C

import numpy as np

from . import ffi

U64 = np.uint64


def _lib():
    return ffi.default_library()


class CudaStreams:
    """One stream per GPU (mod.rs:33-150)."""

    def __init__(self, gpu_indexes):
        self.gpu_indexes = [int(g) for g in gpu_indexes]
        self.ptr = [_lib().cuda_create_stream_ffi(g) for g in self.gpu_indexes]

    @classmethod
    def new_single_gpu(cls, gpu_index=0):
        return cls([gpu_index])

    @classmethod
    def new_multi_gpu(cls):
        return cls(range(_lib().cuda_get_number_of_gpus()))

    def synchronize(self):
        for s, g in zip(self.ptr, self.gpu_indexes):
            _lib().cuda_synchronize_stream(s, g)

    def synchronize_one(self, i):
        _lib().cuda_synchronize_stream(self.ptr[i], self.gpu_indexes[i])

    def __len__(self):
        return len(self.ptr)

    def destroy(self):
        for s, g in zip(self.ptr, self.gpu_indexes):
            _lib().cuda_destroy_stream(s, g)
        self.ptr = []

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class CudaVec:
    """Device array of one dtype on the GPU of streams[stream_index] (vec.rs).  elem_words=2: elements of 16 bytes
    (u128), which cross the Python boundary as uint64 pairs (lo, hi) in a trailing dimension of 2 — the memory image of
    unsigned __int128 on both sides."""

    def __init__(self, length, streams, stream_index=0, dtype=U64, elem_words=1):
        self.len = int(length)
        self.dtype = np.dtype(dtype)
        self.elem_words = int(elem_words)
        assert self.elem_words in (1, 2) and (self.elem_words == 1 or self.dtype == U64)
        self.gpu_index = streams.gpu_indexes[stream_index]
        nbytes = max(self.len * self.dtype.itemsize * self.elem_words, 8)
        self.ptr = _lib().cuda_malloc(nbytes, self.gpu_index)
        _lib().cuda_memset_async(self.ptr, 0, nbytes, streams.ptr[stream_index], self.gpu_index)

    @classmethod
    def from_cpu_async(cls, src, streams, stream_index=0, elem_words=1):
        src = np.ascontiguousarray(src)
        assert elem_words == 1 or src.shape[-1] == 2, "u128 arrays are uint64 arrays with a trailing dimension of 2"
        v = cls(src.size // elem_words, streams, stream_index, src.dtype, elem_words)
        v.copy_from_cpu_async(src, streams, stream_index)
        return v

    def copy_from_cpu_async(self, src, streams, stream_index=0):
        src = np.ascontiguousarray(src, dtype=self.dtype)
        assert src.size <= self.len * self.elem_words, "CudaVec: source larger than the device vector"
        _lib().cuda_memcpy_async_to_gpu(self.ptr, src.ctypes.data_as(C.c_void_p), src.nbytes,
                                        streams.ptr[stream_index], self.gpu_index)
        # the source is pageable host memory: keep it alive until the stream is drained
        streams.synchronize_one(stream_index)

    def copy_to_cpu(self, streams, stream_index=0):
        out = np.empty(self.len * self.elem_words, dtype=self.dtype)
        _lib().cuda_memcpy_async_to_cpu(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes,
                                        streams.ptr[stream_index], self.gpu_index)
        streams.synchronize_one(stream_index)
        return out.reshape(-1, 2) if self.elem_words == 2 else out

    def drop(self):
        if self.ptr:
            _lib().cuda_drop(self.ptr, self.gpu_index)
            self.ptr = None

    def __del__(self):
        try:
            self.drop()
        except Exception:
            pass


class CudaLweCiphertextList:
    def __init__(self, d_vec, lwe_ciphertext_count, lwe_dimension):
        self.d_vec = d_vec
        self.lwe_ciphertext_count = int(lwe_ciphertext_count)
        self.lwe_dimension = int(lwe_dimension)

    @classmethod
    def new(cls, lwe_dimension, lwe_ciphertext_count, streams, dtype=U64, elem_words=1):
        """dtype=np.uint32: the 32-bit ciphertexts a u32 keyswitch key produces (KS32 pattern); elem_words=2: u128."""
        return cls(CudaVec((lwe_dimension + 1) * lwe_ciphertext_count, streams, dtype=dtype, elem_words=elem_words),
                   lwe_ciphertext_count, lwe_dimension)

    @classmethod
    def from_lwe_ciphertext_list(cls, h_ct, streams):
        """[count][lwe_size] u64 words, or [count][lwe_size][2] for u128 ciphertexts"""
        h_ct = np.ascontiguousarray(h_ct, dtype=U64)
        if h_ct.ndim == 3:
            assert h_ct.shape[2] == 2, "expected [count][lwe_size][2]"
            return cls(CudaVec.from_cpu_async(h_ct.reshape(-1, 2), streams, elem_words=2), h_ct.shape[0], h_ct.shape[1] - 1)
        assert h_ct.ndim == 2, "expected [count][lwe_size]"
        return cls(CudaVec.from_cpu_async(h_ct.reshape(-1), streams), h_ct.shape[0], h_ct.shape[1] - 1)

    def to_lwe_ciphertext_list(self, streams):
        flat = self.d_vec.copy_to_cpu(streams)
        if self.d_vec.elem_words == 2:
            return flat.reshape(self.lwe_ciphertext_count, self.lwe_dimension + 1, 2)
        return flat.reshape(self.lwe_ciphertext_count, self.lwe_dimension + 1)


class CudaLweCompactCiphertextList:
    """Compact LWE lists end to end on the device, as the expansion entry points read them (the flattened array of
    integer/gpu/ciphertext/compact_list.rs): per list n_c mask words, then one body word per ciphertext of the list."""

    def __init__(self, d_vec, n_c, num_lwe_per_compact_list):
        self.d_vec = d_vec
        self.n_c = int(n_c)
        self.num_lwe_per_compact_list = [int(c) for c in num_lwe_per_compact_list]
        assert self.n_c >= 1 and self.num_lwe_per_compact_list, "no compact list"
        assert all(1 <= c <= self.n_c for c in self.num_lwe_per_compact_list), \
            "a compact list holds between 1 and n_c bodies"
        assert d_vec.len == self.size_words(self.n_c, self.num_lwe_per_compact_list), \
            "the flattened words do not have the size the list counts describe"

    @staticmethod
    def size_words(n_c, num_lwe_per_compact_list):
        return sum(int(n_c) + int(c) for c in num_lwe_per_compact_list)

    @classmethod
    def from_flat_words(cls, words, n_c, num_lwe_per_compact_list, streams):
        words = np.ascontiguousarray(words, dtype=U64).reshape(-1)
        return cls(CudaVec.from_cpu_async(words, streams), n_c, num_lwe_per_compact_list)

    @property
    def lwe_ciphertext_count(self):
        return sum(self.num_lwe_per_compact_list)

    def to_flat_words(self, streams):
        return self.d_vec.copy_to_cpu(streams)


class CudaGlweCiphertextList:
    def __init__(self, d_vec, glwe_ciphertext_count, glwe_dimension, polynomial_size):
        self.d_vec = d_vec
        self.glwe_ciphertext_count = int(glwe_ciphertext_count)
        self.glwe_dimension = int(glwe_dimension)
        self.polynomial_size = int(polynomial_size)

    @classmethod
    def from_glwe_ciphertext_list(cls, h_ct, glwe_dimension, polynomial_size, streams, elem_words=1):
        """elem_words=2: u128 GLWEs, h_ct of shape [..., 2]"""
        h_ct = np.ascontiguousarray(h_ct, dtype=U64).reshape(-1, (glwe_dimension + 1) * polynomial_size * elem_words)
        flat = h_ct.reshape(-1, 2) if elem_words == 2 else h_ct.reshape(-1)
        return cls(CudaVec.from_cpu_async(flat, streams, elem_words=elem_words), h_ct.shape[0], glwe_dimension,
                   polynomial_size)

    def to_glwe_ciphertext_list(self, streams):
        flat = self.d_vec.copy_to_cpu(streams)
        if self.d_vec.elem_words == 2:
            return flat.reshape(self.glwe_ciphertext_count, -1, 2)
        return flat.reshape(self.glwe_ciphertext_count, -1)


class CudaLweBootstrapKey:
    """Bootstrap key converted once per GPU of `streams` (lwe_bootstrap_key.rs:57-104,
    gpu/ffi.rs:744-787).  engine 'fft64' is the reference GPU path; 'ntt64' the Goldilocks
    extension (integer arithmetic modulo 2^64 - 2^32 + 1: any parameter set), 'ntt64_split' the same function — same
    bits — on the throughput kernel's f64 transforms with the key in four 16-bit limbs (N = 2048, k = 1, one level;
    a key of four times the bytes; 1.56x the integer kernel's rate on the MI355X); 'exact64' the O(N^2)
    exact-convolution verification engine, 'ref64' the reference-order f64 verification engine (tfhe-fft's dif4
    plan: reproduces the reference's f64 golden vectors)."""

    def __init__(self):
        self.d_vec = None

    @classmethod
    def from_lwe_bootstrap_key(cls, h_bsk, input_lwe_dimension, glwe_dimension, polynomial_size,
                               decomp_base_log, decomp_level_count, streams, ms_noise_reduction=False,
                               engine="fft64"):
        self = cls()
        self.input_lwe_dimension = int(input_lwe_dimension)
        self.glwe_dimension = int(glwe_dimension)
        self.polynomial_size = int(polynomial_size)
        self.decomp_base_log = int(decomp_base_log)
        self.decomp_level_count = int(decomp_level_count)
        self.ms_noise_reduction = bool(ms_noise_reduction)
        self.engine = "ntt64" if engine == "ntt64_split" else engine
        self.engine_impl = "ntt64_int" if engine == "ntt64" else engine
        if engine == "ntt64_split":
            assert _lib().hip_programmable_bootstrap_ntt64_split_supported(
                glwe_dimension, polynomial_size, decomp_level_count, decomp_base_log), \
                "parameter set outside the split-key form of the NTT engine"
        engine = self.engine_impl
        h_bsk = np.ascontiguousarray(h_bsk, dtype=U64)
        elems = (self.input_lwe_dimension * (glwe_dimension + 1) ** 2 * decomp_level_count * polynomial_size)
        assert h_bsk.size == elems, "bootstrap key container has the wrong size"
        # n*(k+1)^2*l*N f64 per GPU — the byte size of the standard key; four limb polynomials per key polynomial for
        # 'ntt64_split'
        self.d_vecs = []
        for i in range(len(streams)):
            d = CudaVec(elems * (4 if engine == "ntt64_split" else 1), streams, i, np.float64)
            conv = {"fft64": _lib().cuda_convert_lwe_programmable_bootstrap_key_64_async,
                    "ntt64_int": _lib().hip_convert_lwe_programmable_bootstrap_key_ntt64_async,
                    "ntt64_split": _lib().hip_convert_lwe_programmable_bootstrap_key_ntt64_split_async,
                    "exact64": _lib().hip_convert_lwe_programmable_bootstrap_key_exact64_async,
                    "ref64": _lib().hip_convert_lwe_programmable_bootstrap_key_ref64_async}[engine]
            conv(streams.ptr[i], streams.gpu_indexes[i], d.ptr, h_bsk.ctypes.data_as(C.c_void_p),
                 self.input_lwe_dimension, glwe_dimension, decomp_level_count, polynomial_size)
            self.d_vecs.append(d)
        streams.synchronize()
        self.d_vec = self.d_vecs[0]
        return self

    @property
    def output_lwe_dimension(self):
        return self.glwe_dimension * self.polynomial_size


class CudaLweMultiBitBootstrapKey:
    @classmethod
    def from_lwe_multi_bit_bootstrap_key(cls, h_bsk, input_lwe_dimension, glwe_dimension, polynomial_size,
                                         decomp_base_log, decomp_level_count, grouping_factor, streams):
        self = cls()
        self.input_lwe_dimension = int(input_lwe_dimension)
        self.glwe_dimension = int(glwe_dimension)
        self.polynomial_size = int(polynomial_size)
        self.decomp_base_log = int(decomp_base_log)
        self.decomp_level_count = int(decomp_level_count)
        self.grouping_factor = int(grouping_factor)
        h_bsk = np.ascontiguousarray(h_bsk, dtype=U64)
        self.d_vecs = []
        for i in range(len(streams)):
            d = CudaVec(h_bsk.size, streams, i, U64)
            _lib().cuda_convert_lwe_multi_bit_programmable_bootstrap_key_64_async(
                streams.ptr[i], streams.gpu_indexes[i], d.ptr, h_bsk.ctypes.data_as(C.c_void_p),
                self.input_lwe_dimension, glwe_dimension, decomp_level_count, polynomial_size, grouping_factor)
            self.d_vecs.append(d)
        streams.synchronize()
        self.d_vec = self.d_vecs[0]
        return self

    @property
    def output_lwe_dimension(self):
        return self.glwe_dimension * self.polynomial_size


class CudaLweKeyswitchKey:
    @classmethod
    def from_lwe_keyswitch_key(cls, h_ksk, input_key_lwe_dimension, output_key_lwe_dimension, decomp_base_log,
                               decomp_level_count, streams):
        self = cls()
        self.input_key_lwe_dimension = int(input_key_lwe_dimension)
        self.output_key_lwe_dimension = int(output_key_lwe_dimension)
        self.decomp_base_log = int(decomp_base_log)
        self.decomp_level_count = int(decomp_level_count)
        # a uint32 array is a KS32 key (gpu/ffi.rs:503-618 dispatches on the key scalar), anything else u64
        h_ksk = np.ascontiguousarray(h_ksk)
        if h_ksk.dtype != np.uint32:
            h_ksk = h_ksk.astype(U64, copy=False)
        self.scalar_bits = 8 * h_ksk.dtype.itemsize
        assert h_ksk.size == input_key_lwe_dimension * decomp_level_count * (output_key_lwe_dimension + 1)
        self.d_vecs = [CudaVec.from_cpu_async(h_ksk, streams, i) for i in range(len(streams))]
        self.d_vec = self.d_vecs[0]
        return self


class CudaLwePackingKeyswitchKey:
    """gpu/entities/lwe_packing_keyswitch_key.rs: [input_lwe_dimension][level][(glwe_dimension + 1) * polynomial_size]
    u64 words on every GPU of `streams`, uploaded as they are."""

    @classmethod
    def from_lwe_packing_keyswitch_key(cls, h_pksk, input_key_lwe_dimension, output_glwe_dimension, output_polynomial_size,
                                       decomp_base_log, decomp_level_count, streams):
        self = cls()
        self.input_key_lwe_dimension = int(input_key_lwe_dimension)
        self.output_glwe_dimension = int(output_glwe_dimension)
        self.output_polynomial_size = int(output_polynomial_size)
        self.decomp_base_log = int(decomp_base_log)
        self.decomp_level_count = int(decomp_level_count)
        h_pksk = np.ascontiguousarray(h_pksk, dtype=U64)
        assert h_pksk.size == (self.input_key_lwe_dimension * self.decomp_level_count *
                               (self.output_glwe_dimension + 1) * self.output_polynomial_size), \
            "packing keyswitch key container has the wrong size"
        self.d_vecs = [CudaVec.from_cpu_async(h_pksk.reshape(-1), streams, i) for i in range(len(streams))]
        self.d_vec = self.d_vecs[0]
        return self


def _streams_ffi(streams):
    ptrs = (C.c_void_p * len(streams))(*streams.ptr)
    idx = (C.c_uint32 * len(streams))(*streams.gpu_indexes)
    return ffi.CudaStreamsFFI(ptrs, idx, len(streams)), (ptrs, idx)


class CudaLwePackingKeyswitchKey128:
    """The u128 packing keyswitch key of squashed-noise list compression: [input_lwe_dimension][level]
    [(glwe_dimension + 1) * polynomial_size] u128 words given as uint64 pairs, on the first GPU of `streams`.  It owns both
    device layouts: the key as it is (d_vec, the general kernel's) and, where the matrix-core kernel carries the shape, its
    byte planes (d_planes, else None), converted once here."""

    @classmethod
    def from_lwe_packing_keyswitch_key(cls, h_pksk, input_key_lwe_dimension, output_glwe_dimension, output_polynomial_size,
                                       decomp_base_log, decomp_level_count, streams):
        self = cls()
        self.input_key_lwe_dimension = int(input_key_lwe_dimension)
        self.output_glwe_dimension = int(output_glwe_dimension)
        self.output_polynomial_size = int(output_polynomial_size)
        self.decomp_base_log = int(decomp_base_log)
        self.decomp_level_count = int(decomp_level_count)
        h_pksk = np.ascontiguousarray(h_pksk, dtype=U64)
        assert h_pksk.shape[-1] == 2 and h_pksk.size == 2 * (
            self.input_key_lwe_dimension * self.decomp_level_count * (self.output_glwe_dimension + 1) *
            self.output_polynomial_size), "packing keyswitch key container has the wrong size"
        self.d_vec = CudaVec.from_cpu_async(h_pksk.reshape(-1, 2), streams, elem_words=2)
        shape = (self.input_key_lwe_dimension, self.output_glwe_dimension, self.output_polynomial_size,
                 self.decomp_base_log, self.decomp_level_count)
        self.d_planes = None
        planes_bytes = int(_lib().hip_lwe_packing_keyswitch_key_128_planes_size_bytes(*shape))
        if planes_bytes:
            s, keep = _streams_ffi(streams)
            self.d_planes = CudaVec(planes_bytes // 8, streams)
            _lib().hip_convert_lwe_packing_keyswitch_key_128_async(s, self.d_planes.ptr, self.d_vec.ptr, *shape)
        return self

    @property
    def planes_ptr(self):
        return self.d_planes.ptr if self.d_planes is not None else None

    def size_bytes(self):
        return 16 * self.d_vec.len


def cuda_keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext_128(pksk, input_lwe_list, output_glwe_list, streams,
                                                                       lwe_per_glwe=None):
    """The u128 packing keyswitch: the LWEs of `input_lwe_list` (u128), in chunks of `lwe_per_glwe` (default: all of them
    in one GLWE), are keyswitched and packed, LWE i of a chunk at X^i, into the u128 GLWEs of `output_glwe_list`."""
    assert pksk.input_key_lwe_dimension == input_lwe_list.lwe_dimension, (
        f"Mismatched input LweDimension. LwePackingKeyswitchKey input LweDimension: {pksk.input_key_lwe_dimension}, "
        f"input LweCiphertext LweDimension {input_lwe_list.lwe_dimension}.")
    assert (pksk.output_glwe_dimension == output_glwe_list.glwe_dimension and
            pksk.output_polynomial_size == output_glwe_list.polynomial_size), "Mismatched output GlweSize / PolynomialSize"
    assert input_lwe_list.d_vec.elem_words == 2 and output_glwe_list.d_vec.elem_words == 2, "u128 ciphertexts expected"
    n = input_lwe_list.lwe_ciphertext_count
    per = n if lwe_per_glwe is None else int(lwe_per_glwe)
    assert output_glwe_list.glwe_ciphertext_count * per >= n, "output GLWE list too short"
    s, keep = _streams_ffi(streams)
    mem = C.c_void_p()
    shape = (pksk.input_key_lwe_dimension, pksk.output_glwe_dimension, pksk.output_polynomial_size, pksk.decomp_base_log,
             pksk.decomp_level_count)
    lib = _lib()
    lib.hip_scratch_packing_keyswitch_lwe_list_to_glwe_128_async(s, C.byref(mem), *shape, n, True)
    lib.hip_packing_keyswitch_lwe_list_to_glwe_128_async(s, output_glwe_list.d_vec.ptr, input_lwe_list.d_vec.ptr,
                                                         pksk.d_vec.ptr, pksk.planes_ptr, mem, *shape, n, per)
    lib.hip_cleanup_packing_keyswitch_lwe_list_to_glwe_128(s, C.byref(mem))


def cuda_keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext(pksk, input_lwe_list, output_glwe_list, streams,
                                                                   lwe_per_glwe=None):
    """gpu/algorithms/lwe_packing_keyswitch.rs: the LWEs of `input_lwe_list`, in chunks of `lwe_per_glwe` (default: all
    of them in one GLWE), are keyswitched and packed, LWE i of a chunk at X^i, into the GLWEs of `output_glwe_list`
    (scratch -> launch -> cleanup)."""
    assert pksk.input_key_lwe_dimension == input_lwe_list.lwe_dimension, (
        f"Mismatched input LweDimension. LwePackingKeyswitchKey input LweDimension: {pksk.input_key_lwe_dimension}, "
        f"input LweCiphertext LweDimension {input_lwe_list.lwe_dimension}.")
    assert (pksk.output_glwe_dimension == output_glwe_list.glwe_dimension and
            pksk.output_polynomial_size == output_glwe_list.polynomial_size), "Mismatched output GlweSize / PolynomialSize"
    n = input_lwe_list.lwe_ciphertext_count
    per = n if lwe_per_glwe is None else int(lwe_per_glwe)
    assert output_glwe_list.glwe_ciphertext_count * per >= n, "output GLWE list too short"
    s, keep = _streams_ffi(streams)
    mem = C.c_void_p()
    shape = (pksk.input_key_lwe_dimension, pksk.output_glwe_dimension, pksk.output_polynomial_size, pksk.decomp_base_log,
             pksk.decomp_level_count)
    lib = _lib()
    lib.hip_scratch_packing_keyswitch_lwe_list_to_glwe_64_async(s, C.byref(mem), *shape, n, True)
    lib.hip_packing_keyswitch_lwe_list_to_glwe_64_async(s, output_glwe_list.d_vec.ptr, input_lwe_list.d_vec.ptr,
                                                        pksk.d_vec.ptr, mem, *shape, n, per)
    lib.hip_cleanup_packing_keyswitch_lwe_list_to_glwe_64(s, C.byref(mem))


# ciphertexts of the last split-key bootstrap that went through the integer kernel (cuda_programmable_bootstrap_lwe_ciphertext)
last_split_recomputed = 0


def _trivial_indexes(count, streams):
    return CudaVec.from_cpu_async(np.arange(count, dtype=U64), streams)


def cuda_programmable_bootstrap_lwe_ciphertext(input, output, accumulator, lut_indexes, output_indexes,
                                               input_indexes, bsk, streams, num_many_lut=1, lut_stride=0):
    """gpu/algorithms/lwe_programmable_bootstrapping.rs:10-136 + gpu/ffi.rs:21-92
    (scratch -> launch -> cleanup on streams.ptr[0])."""
    assert input.lwe_dimension == bsk.input_lwe_dimension, (
        f"Mismatched input LweDimension. LweCiphertext input LweDimension {input.lwe_dimension}. "
        f"BootstrapKey input LweDimension {bsk.input_lwe_dimension}.")
    assert output.lwe_dimension == bsk.output_lwe_dimension, (
        f"Mismatched output LweDimension. LweCiphertext output LweDimension {output.lwe_dimension}. "
        f"BootstrapKey output LweDimension {bsk.output_lwe_dimension}.")
    assert accumulator.glwe_dimension == bsk.glwe_dimension, "Mismatched GlweSize"
    assert accumulator.polynomial_size == bsk.polynomial_size, "Mismatched PolynomialSize"
    num_samples = input.lwe_ciphertext_count
    assert output.lwe_ciphertext_count >= num_samples * num_many_lut
    lib = _lib()
    buf = C.c_void_p()
    s, g = streams.ptr[0], streams.gpu_indexes[0]
    lib.scratch_cuda_programmable_bootstrap_64_async(
        s, g, C.byref(buf), bsk.input_lwe_dimension, bsk.glwe_dimension, bsk.polynomial_size,
        bsk.decomp_level_count, num_samples, True, 1 if bsk.ms_noise_reduction else 0)
    launch = {"fft64": lib.cuda_programmable_bootstrap_64_async,
              "ntt64_int": lib.hip_programmable_bootstrap_ntt64_async,
              "ntt64_split": lib.hip_programmable_bootstrap_ntt64_split_async,
              "exact64": lib.hip_programmable_bootstrap_exact64_async,
              "ref64": lib.hip_programmable_bootstrap_ref64_async}[bsk.engine_impl]
    launch(s, g, output.d_vec.ptr, output_indexes.ptr, accumulator.d_vec.ptr, lut_indexes.ptr,
           input.d_vec.ptr, input_indexes.ptr, bsk.d_vec.ptr, buf, bsk.input_lwe_dimension, bsk.glwe_dimension,
           bsk.polynomial_size, bsk.decomp_base_log, bsk.decomp_level_count, num_samples, num_many_lut, lut_stride)
    if bsk.engine_impl == "ntt64_split":
        # the exact products of this engine come out of f64 transforms; a ciphertext whose limb products were not within 1/4
        # of integers is recomputed by the integer kernel on the same stream (never observed on a real parameter set's data):
        # the outputs are exact either way, the count is kept for whoever wants to know
        global last_split_recomputed
        last_split_recomputed = int(lib.hip_programmable_bootstrap_ntt64_split_roundoff_status(s, g, buf))
    lib.cleanup_cuda_programmable_bootstrap_64(s, g, C.byref(buf))


def cuda_keyswitch_programmable_bootstrap_lwe_ciphertext(input, output, accumulator, lut_indexes, output_indexes,
                                                         input_indexes, ksk, bsk, streams, num_many_lut=1,
                                                         lut_stride=0):
    """The shortint atomic pattern (shortint/atomic_pattern/standard.rs:162-199: keyswitch then bootstrap) as ONE
    call of the backend (extension hip_keyswitch_programmable_bootstrap_64_async): `input` holds ciphertexts under
    the big key, the keyswitched list lives in the PBS scratch."""
    assert ksk.input_key_lwe_dimension == input.lwe_dimension, "Mismatched input LweDimension"
    assert ksk.output_key_lwe_dimension == bsk.input_lwe_dimension, "keyswitch and bootstrap keys do not chain"
    assert output.lwe_dimension == bsk.output_lwe_dimension, "Mismatched output LweDimension"
    assert bsk.engine == "fft64" and ksk.scalar_bits == 64
    num_samples = input.lwe_ciphertext_count
    assert output.lwe_ciphertext_count >= num_samples * num_many_lut
    lib = _lib()
    buf = C.c_void_p()
    s, g = streams.ptr[0], streams.gpu_indexes[0]
    lib.hip_scratch_keyswitch_programmable_bootstrap_64_async(
        s, g, C.byref(buf), bsk.input_lwe_dimension, bsk.glwe_dimension, bsk.polynomial_size,
        bsk.decomp_level_count, num_samples, True, 1 if bsk.ms_noise_reduction else 0)
    lib.hip_keyswitch_programmable_bootstrap_64_async(
        s, g, output.d_vec.ptr, output_indexes.ptr, accumulator.d_vec.ptr, lut_indexes.ptr, input.d_vec.ptr,
        input_indexes.ptr, ksk.d_vec.ptr, bsk.d_vec.ptr, buf, bsk.input_lwe_dimension, bsk.glwe_dimension,
        bsk.polynomial_size, ksk.decomp_base_log, ksk.decomp_level_count, bsk.decomp_base_log,
        bsk.decomp_level_count, num_samples, num_many_lut, lut_stride)
    lib.cleanup_cuda_programmable_bootstrap_64(s, g, C.byref(buf))


def cuda_multi_bit_programmable_bootstrap_lwe_ciphertext(input, output, accumulator, lut_indexes, output_indexes,
                                                         input_indexes, multi_bit_bsk, streams, num_many_lut=1,
                                                         lut_stride=0):
    """gpu/algorithms/lwe_multi_bit_programmable_bootstrapping.rs:10-145 + gpu/ffi.rs:208-309"""
    bsk = multi_bit_bsk
    assert input.lwe_dimension == bsk.input_lwe_dimension, "Mismatched input LweDimension"
    assert output.lwe_dimension == bsk.output_lwe_dimension, "Mismatched output LweDimension"
    assert accumulator.glwe_dimension == bsk.glwe_dimension, "Mismatched GlweSize"
    assert accumulator.polynomial_size == bsk.polynomial_size, "Mismatched PolynomialSize"
    num_samples = input.lwe_ciphertext_count
    assert output.lwe_ciphertext_count >= num_samples * num_many_lut
    lib = _lib()
    buf = C.c_void_p()
    s, g = streams.ptr[0], streams.gpu_indexes[0]
    lib.scratch_cuda_multi_bit_programmable_bootstrap_64_async(
        s, g, C.byref(buf), bsk.glwe_dimension, bsk.polynomial_size, bsk.decomp_level_count, num_samples, True)
    lib.cuda_multi_bit_programmable_bootstrap_64_async(
        s, g, output.d_vec.ptr, output_indexes.ptr, accumulator.d_vec.ptr, lut_indexes.ptr, input.d_vec.ptr,
        input_indexes.ptr, bsk.d_vec.ptr, buf, bsk.input_lwe_dimension, bsk.glwe_dimension, bsk.polynomial_size,
        bsk.grouping_factor, bsk.decomp_base_log, bsk.decomp_level_count, num_samples, num_many_lut, lut_stride)
    lib.cleanup_cuda_multi_bit_programmable_bootstrap_64(s, g, C.byref(buf))


class CudaLweBootstrapKey128:
    """gpu/entities/lwe_bootstrap_key.rs (the u128 key of noise squashing): the standard-domain key, [n][level][k + 1]
    [k + 1][N] u128 words given as uint64 pairs, converted once per GPU of `streams` to the f128 Fourier domain."""

    @classmethod
    def from_lwe_bootstrap_key(cls, h_bsk, input_lwe_dimension, glwe_dimension, polynomial_size, decomp_base_log,
                               decomp_level_count, streams, ms_noise_reduction=False):
        self = cls()
        self.input_lwe_dimension = int(input_lwe_dimension)
        self.glwe_dimension = int(glwe_dimension)
        self.polynomial_size = int(polynomial_size)
        self.decomp_base_log = int(decomp_base_log)
        self.decomp_level_count = int(decomp_level_count)
        self.ms_noise_reduction = bool(ms_noise_reduction)
        h_bsk = np.ascontiguousarray(h_bsk, dtype=U64)
        elems = self.input_lwe_dimension * (glwe_dimension + 1) ** 2 * decomp_level_count * polynomial_size
        assert h_bsk.size == 2 * elems and h_bsk.shape[-1] == 2, "bootstrap key container has the wrong size"
        self.d_vecs = []
        for i in range(len(streams)):
            d = CudaVec(2 * elems, streams, i, np.float64)  # 32 * N / 2 bytes per polynomial
            _lib().hip_convert_lwe_programmable_bootstrap_key_128_async(
                streams.ptr[i], streams.gpu_indexes[i], d.ptr, h_bsk.ctypes.data_as(C.c_void_p),
                self.input_lwe_dimension, glwe_dimension, decomp_level_count, polynomial_size)
            self.d_vecs.append(d)
        streams.synchronize()
        self.d_vec = self.d_vecs[0]
        return self

    @property
    def output_lwe_dimension(self):
        return self.glwe_dimension * self.polynomial_size


def cuda_programmable_bootstrap_128_lwe_ciphertext(input, output, accumulator, bsk, streams):
    """gpu/algorithms/lwe_programmable_bootstrapping.rs (cuda_programmable_bootstrap_128_lwe_ciphertext): u64 inputs, one
    u128 accumulator, u128 outputs (scratch -> launch -> cleanup on streams.ptr[0])."""
    assert input.lwe_dimension == bsk.input_lwe_dimension, (
        f"Mismatched input LweDimension. LweCiphertext input LweDimension {input.lwe_dimension}. "
        f"BootstrapKey input LweDimension {bsk.input_lwe_dimension}.")
    assert output.lwe_dimension == bsk.output_lwe_dimension, (
        f"Mismatched output LweDimension. LweCiphertext output LweDimension {output.lwe_dimension}. "
        f"BootstrapKey output LweDimension {bsk.output_lwe_dimension}.")
    assert accumulator.glwe_dimension == bsk.glwe_dimension, "Mismatched GlweSize"
    assert accumulator.polynomial_size == bsk.polynomial_size, "Mismatched PolynomialSize"
    assert input.d_vec.elem_words == 1 and output.d_vec.elem_words == 2 and accumulator.d_vec.elem_words == 2, \
        "the 128-bit bootstrap takes u64 inputs, a u128 accumulator and u128 outputs"
    num_samples = input.lwe_ciphertext_count
    assert output.lwe_ciphertext_count >= num_samples
    lib = _lib()
    buf = C.c_void_p()
    s, g = streams.ptr[0], streams.gpu_indexes[0]
    shape = (bsk.input_lwe_dimension, bsk.glwe_dimension, bsk.polynomial_size)
    lib.hip_scratch_programmable_bootstrap_128_async(s, g, C.byref(buf), *shape, bsk.decomp_level_count, num_samples, True,
                                                     1 if bsk.ms_noise_reduction else 0)
    lib.hip_programmable_bootstrap_128_async(s, g, output.d_vec.ptr, accumulator.d_vec.ptr, input.d_vec.ptr, bsk.d_vec.ptr,
                                             buf, *shape, bsk.decomp_base_log, bsk.decomp_level_count, num_samples)
    lib.hip_cleanup_programmable_bootstrap_128(s, g, C.byref(buf))


class CudaLweMultiBitBootstrapKey128:
    """gpu/entities/lwe_multi_bit_bootstrap_key.rs (the u128 multi-bit key of noise squashing): the standard-domain key,
    [n / g][2^g][level][k + 1][k + 1][N] u128 words given as uint64 pairs.  It stays in the standard domain on the device:
    the bootstrap sums a group's key bundle exactly and transforms it afterwards."""

    @classmethod
    def from_lwe_multi_bit_bootstrap_key(cls, h_bsk, input_lwe_dimension, glwe_dimension, polynomial_size, decomp_base_log,
                                         decomp_level_count, grouping_factor, streams):
        self = cls()
        self.input_lwe_dimension = int(input_lwe_dimension)
        self.glwe_dimension = int(glwe_dimension)
        self.polynomial_size = int(polynomial_size)
        self.decomp_base_log = int(decomp_base_log)
        self.decomp_level_count = int(decomp_level_count)
        self.grouping_factor = int(grouping_factor)
        self.ms_noise_reduction = False  # multi-bit has the plain modulus switch only
        h_bsk = np.ascontiguousarray(h_bsk, dtype=U64)
        elems = ((self.input_lwe_dimension // max(self.grouping_factor, 1)) * (1 << self.grouping_factor)
                 * (glwe_dimension + 1) ** 2 * decomp_level_count * polynomial_size)
        assert h_bsk.size == 2 * elems and h_bsk.shape[-1] == 2, "multi-bit bootstrap key container has the wrong size"
        self.d_vecs = []
        for i in range(len(streams)):
            d = CudaVec(elems, streams, i, elem_words=2)
            _lib().hip_convert_lwe_multi_bit_programmable_bootstrap_key_128_async(
                streams.ptr[i], streams.gpu_indexes[i], d.ptr, h_bsk.ctypes.data_as(C.c_void_p),
                self.input_lwe_dimension, glwe_dimension, decomp_level_count, polynomial_size, self.grouping_factor)
            self.d_vecs.append(d)
        streams.synchronize()
        self.d_vec = self.d_vecs[0]
        return self

    @property
    def output_lwe_dimension(self):
        return self.glwe_dimension * self.polynomial_size


def cuda_multi_bit_programmable_bootstrap_128_lwe_ciphertext(input, output, accumulator, output_indexes, input_indexes, bsk,
                                                             streams):
    """gpu/algorithms/lwe_multi_bit_programmable_bootstrapping.rs (cuda_multi_bit_programmable_bootstrap_128_lwe_
    ciphertext): u64 inputs, one u128 accumulator, u128 outputs; sample s reads input_indexes[s] and writes
    output_indexes[s] (scratch -> launch -> cleanup on streams.ptr[0])."""
    assert input.lwe_dimension == bsk.input_lwe_dimension, (
        f"Mismatched input LweDimension. LweCiphertext input LweDimension {input.lwe_dimension}. "
        f"BootstrapKey input LweDimension {bsk.input_lwe_dimension}.")
    assert output.lwe_dimension == bsk.output_lwe_dimension, (
        f"Mismatched output LweDimension. LweCiphertext output LweDimension {output.lwe_dimension}. "
        f"BootstrapKey output LweDimension {bsk.output_lwe_dimension}.")
    assert accumulator.glwe_dimension == bsk.glwe_dimension, "Mismatched GlweSize"
    assert accumulator.polynomial_size == bsk.polynomial_size, "Mismatched PolynomialSize"
    assert input.d_vec.elem_words == 1 and output.d_vec.elem_words == 2 and accumulator.d_vec.elem_words == 2, \
        "the 128-bit bootstrap takes u64 inputs, a u128 accumulator and u128 outputs"
    num_samples = input.lwe_ciphertext_count
    assert output.lwe_ciphertext_count >= num_samples
    lib = _lib()
    buf = C.c_void_p()
    s, g = streams.ptr[0], streams.gpu_indexes[0]
    lib.hip_scratch_multi_bit_programmable_bootstrap_128_async(s, g, C.byref(buf), bsk.glwe_dimension, bsk.polynomial_size,
                                                               bsk.decomp_level_count, num_samples, True)
    lib.hip_multi_bit_programmable_bootstrap_128_async(
        s, g, output.d_vec.ptr, output_indexes.ptr, accumulator.d_vec.ptr, input.d_vec.ptr, input_indexes.ptr, bsk.d_vec.ptr,
        buf, bsk.input_lwe_dimension, bsk.glwe_dimension, bsk.polynomial_size, bsk.grouping_factor, bsk.decomp_base_log,
        bsk.decomp_level_count, num_samples, 1, 0)
    lib.hip_cleanup_multi_bit_programmable_bootstrap_128(s, g, C.byref(buf))


def _f128_planes(polynomial_size, number_of_samples, streams):
    return [CudaVec(number_of_samples * polynomial_size // 2, streams, dtype=np.float64) for _ in range(4)]


def cuda_fourier_transform_forward_as_torus_f128(standard, polynomial_size, number_of_samples, streams):
    """gpu/ffi.rs (cuda_fourier_transform_forward_as_torus_f128_async): `standard` [samples][N][2] uint64 (u128 words);
    returns the planes re0, re1, im0, im1 as four [samples][N / 2] float64 arrays."""
    return _f128_forward(_lib().hip_fourier_transform_forward_as_torus_f128_async, standard, polynomial_size,
                         number_of_samples, streams)


def cuda_fourier_transform_forward_as_integer_f128(standard, polynomial_size, number_of_samples, streams):
    return _f128_forward(_lib().hip_fourier_transform_forward_as_integer_f128_async, standard, polynomial_size,
                         number_of_samples, streams)


def _f128_forward(fn, standard, polynomial_size, number_of_samples, streams):
    standard = np.ascontiguousarray(standard, dtype=U64)
    assert standard.size == 2 * polynomial_size * number_of_samples
    d_std = CudaVec.from_cpu_async(standard.reshape(-1, 2), streams, elem_words=2)
    planes = _f128_planes(polynomial_size, number_of_samples, streams)
    fn(streams.ptr[0], streams.gpu_indexes[0], *[p.ptr for p in planes], d_std.ptr, polynomial_size, number_of_samples)
    return [p.copy_to_cpu(streams).reshape(number_of_samples, polynomial_size // 2) for p in planes]


def cuda_fourier_transform_backward_as_torus_f128(re0, re1, im0, im1, polynomial_size, number_of_samples, streams):
    """the inverse: four [samples][N / 2] float64 planes -> [samples][N][2] uint64 (u128 words)"""
    planes = [CudaVec.from_cpu_async(np.ascontiguousarray(p, dtype=np.float64).reshape(-1), streams)
              for p in (re0, re1, im0, im1)]
    d_std = CudaVec(polynomial_size * number_of_samples, streams, elem_words=2)
    _lib().hip_fourier_transform_backward_as_torus_f128_async(streams.ptr[0], streams.gpu_indexes[0], d_std.ptr,
                                                              *[p.ptr for p in planes], polynomial_size, number_of_samples)
    return d_std.copy_to_cpu(streams).reshape(number_of_samples, polynomial_size, 2)


def cuda_keyswitch_lwe_ciphertext(ksk, input, output, input_indexes, output_indexes, uses_trivial_indices,
                                  streams, use_gemm_ks=False):
    """gpu/algorithms/lwe_keyswitch.rs:12-143 + gpu/ffi.rs:503-618"""
    assert ksk.input_key_lwe_dimension == input.lwe_dimension, (
        f"Mismatched input LweDimension. LweKeyswitchKey input LweDimension: {ksk.input_key_lwe_dimension}, "
        f"input LweCiphertext LweDimension {input.lwe_dimension}.")
    assert ksk.output_key_lwe_dimension == output.lwe_dimension, (
        f"Mismatched output LweDimension. LweKeyswitchKey output LweDimension: {ksk.output_key_lwe_dimension}, "
        f"output LweCiphertext LweDimension {output.lwe_dimension}.")
    lib = _lib()
    s, g = streams.ptr[0], streams.gpu_indexes[0]
    args = (s, g, output.d_vec.ptr, output_indexes.ptr, input.d_vec.ptr, input_indexes.ptr, ksk.d_vec.ptr,
            ksk.input_key_lwe_dimension, ksk.output_key_lwe_dimension, ksk.decomp_base_log,
            ksk.decomp_level_count, input.lwe_ciphertext_count)
    if ksk.scalar_bits == 32:
        assert output.d_vec.dtype == np.uint32, "a u32 keyswitch key writes u32 ciphertexts"
        if use_gemm_ks:
            lib.cuda_keyswitch_gemm_64_32_async(*args, bool(uses_trivial_indices))
        else:
            lib.cuda_keyswitch_lwe_ciphertext_vector_64_32_async(*args)
    elif use_gemm_ks:
        lib.cuda_keyswitch_gemm_64_64_async(*args, bool(uses_trivial_indices))
    else:
        lib.cuda_keyswitch_lwe_ciphertext_vector_64_64_async(*args)


def cuda_extract_lwe_samples_from_glwe_ciphertext_list(input_glwe_list, output_lwe_list, vec_nth, lwe_per_glwe,
                                                       streams):
    """gpu/algorithms/glwe_sample_extraction.rs:12 + gpu/ffi.rs:838-883"""
    nth = np.ascontiguousarray(vec_nth, dtype=np.uint32)
    d_nth = CudaVec.from_cpu_async(nth, streams)
    _lib().cuda_glwe_sample_extract_64_async(
        streams.ptr[0], streams.gpu_indexes[0], output_lwe_list.d_vec.ptr, input_glwe_list.d_vec.ptr, d_nth.ptr,
        nth.size, lwe_per_glwe, input_glwe_list.polynomial_size, input_glwe_list.glwe_dimension,
        input_glwe_list.polynomial_size)
    streams.synchronize()


def cuda_modulus_switch_ciphertext(output_vec, input_vec, lwe_dimension, log_modulus, centered, streams):
    """gpu/ffi.rs:885-898 (plain) / cuda_centered_modulus_switch_64_async (centered, one LWE)."""
    s, g = streams.ptr[0], streams.gpu_indexes[0]
    if centered:
        _lib().cuda_centered_modulus_switch_64_async(s, g, output_vec.ptr, input_vec.ptr, lwe_dimension, log_modulus)
    else:
        _lib().cuda_modulus_switch_64_async(s, g, output_vec.ptr, input_vec.ptr, lwe_dimension + 1, log_modulus)


def cuda_centered_modulus_switch_cooperative(output_vec, input_vec, lwe_dimension, log_modulus, block_dim, streams):
    """cuda_centered_modulus_switch_cooperative_64_async as modulus_switch.rs:405-418 calls it: one LWE, the body
    correction reduced in a block of shape ``block_dim`` = (x, y) (128 or 512 threads; other sizes abort)."""
    _lib().cuda_centered_modulus_switch_cooperative_64_async(streams.ptr[0], streams.gpu_indexes[0], output_vec.ptr,
                                                             input_vec.ptr, lwe_dimension, log_modulus,
                                                             block_dim[0], block_dim[1])


def forward_fft16x4x16_async(streams, input_vec, output_vec, polynomial_size, total_polynomials):
    """gpu/ffi.rs:1054-1085: compressed real polynomials (f64 bit patterns in the CudaVecs) -> spectra in natural frequency
    order; polynomial_size 2048 only (the library aborts otherwise, as the reference)."""
    _lib().cuda_forward_fft16x4x16_async(streams.ptr[0], streams.gpu_indexes[0], input_vec.ptr, output_vec.ptr,
                                         polynomial_size, total_polynomials)


def cuda_modulus_switch_multi_bit_ciphertext(streams, lwe_array_out, lwe_array_in, log_modulus, polynomial_size,
                                             grouping_factor):
    """gpu/ffi.rs:914-936: the multi-bit modulus switch as its own launch (the reference's noise tests); `lwe_array_in`
    is a CudaVec of len() words read as len() // grouping_factor groups, 2^grouping_factor degrees written per group."""
    _lib().cuda_modulus_switch_multi_bit_64_async(streams.ptr[0], streams.gpu_indexes[0], lwe_array_out.ptr,
                                                  lwe_array_in.ptr, lwe_array_in.len, log_modulus, polynomial_size,
                                                  grouping_factor)
    streams.synchronize()


def programmable_bootstrap_multi_bit_noise_tests(streams, lwe_array_out, output_indexes, test_vector, test_vector_indexes,
                                                 lwe_array_in, input_indexes, bootstrapping_key, lwe_dimension,
                                                 glwe_dimension, polynomial_size, base_log, level, grouping_factor,
                                                 num_samples):
    """gpu/ffi.rs:322-397: multi-bit PBS on an input that already carries the output of the multi-bit modulus switch
    behind the ciphertext ([lwe | degrees]); CudaVec arguments, one ciphertext, N = 2048."""
    assert polynomial_size == 2048, (
        f"programmable_bootstrap_multi_bit_noise_tests only supports polynomial size 2048, got {polynomial_size}")
    lib = _lib()
    buf = C.c_void_p()
    s, g = streams.ptr[0], streams.gpu_indexes[0]
    lib.scratch_cuda_multi_bit_programmable_bootstrap_noise_tests_64_async(s, g, C.byref(buf), glwe_dimension,
                                                                           polynomial_size, level, num_samples, True)
    lib.cuda_multi_bit_programmable_bootstrap_noise_tests_64_async(
        s, g, lwe_array_out.ptr, output_indexes.ptr, test_vector.ptr, test_vector_indexes.ptr, lwe_array_in.ptr,
        input_indexes.ptr, bootstrapping_key.ptr, buf, lwe_dimension, glwe_dimension, polynomial_size, grouping_factor,
        base_log, level, num_samples, 1, 0)
    lib.cleanup_cuda_multi_bit_programmable_bootstrap_noise_tests_64(s, g, C.byref(buf))


def get_number_of_gpus():
    return _lib().cuda_get_number_of_gpus()


def is_cuda_available():
    return bool(_lib().cuda_is_available())
