/*
 * tfhe_hip_backend.h — C ABI of the MI355X (gfx950) TFHE programmable-bootstrapping backend.
 *
 * This is the drop-in boundary for the PBS hot path of tfhe-rs (keyswitch -> modulus switch
 * -> blind rotation -> sample extract).  Every prototype below is EXACTLY the prototype the
 * reference's Rust FFI binds for this path (bindgen over
 * backends/tfhe-cuda-backend/cuda/include/ — build.rs:78-137 — and
 * backends/tfhe-cuda-common/src/cuda_bind.rs), with the same symbol name, argument meaning,
 * asynchrony and error behaviour, so `tfhe::core_crypto::gpu` links against
 * libtfhe_hip_backend.so unchanged for this path (INTEGRATION.md shows the binding).
 *
 * Conventions inherited from the reference boundary:
 *   - `stream` is an opaque handle made by cuda_create_stream_ffi (a hipStream_t here);
 *     `*_async` functions only enqueue on it; `cleanup_*` frees then synchronises;
 *     non-`_async` `cuda_*` functions synchronise internally
 *     (scripts/check_scratch_cleanup.py:1-20).
 *   - all ciphertext / key pointers are DEVICE pointers owned by the caller, except the
 *     `src` of the key-conversion functions, which is a HOST pointer
 *     (tfhe/src/core_crypto/gpu/ffi.rs:744-787).
 *   - no error codes: misuse prints to stderr and abort()s
 *     (backends/tfhe-cuda-common/cuda/include/device.h:13-41).
 *   - `*_indexes` are u64 arrays ON THE DEVICE selecting list element i
 *     (cuda/src/pbs/programmable_bootstrap_classic.cuh:821-826).
 *   - the bootstrap-key device buffer is opaque to the caller and has the reference's byte
 *     size: n*(k+1)^2*l*N doubles (gpu/entities/lwe_bootstrap_key.rs:57-104).
 *
 * Functions prefixed `hip_` are extensions with no counterpart in the reference GPU ABI
 * (the Goldilocks-NTT engine of cc/algorithms/lwe_programmable_bootstrapping/ntt64_bnf_pbs.rs
 * exists only on the reference's CPU side) plus test hooks.
 */
#ifndef TFHE_HIP_BACKEND_H
#define TFHE_HIP_BACKEND_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* backends/tfhe-cuda-backend/cuda/include/pbs/pbs_enums.h:4-6 */
enum PBS_TYPE { MULTI_BIT = 0, CLASSICAL = 1 };
enum PBS_VARIANT { DEFAULT = 0, CG = 1, TBC = 2 };
enum PBS_MS_REDUCTION_T { NO_REDUCTION = 0, CENTERED = 1 };
/* cuda/include/integer/integer.h:9-22 */
enum SHIFT_OR_ROTATE_TYPE { LEFT_SHIFT = 0, RIGHT_SHIFT = 1, LEFT_ROTATE = 2, RIGHT_ROTATE = 3 };
enum BITOP_TYPE { BITAND = 0, BITOR = 1, BITXOR = 2, SCALAR_BITAND = 3, SCALAR_BITOR = 4, SCALAR_BITXOR = 5 };
/* cuda/include/integer/integer.h:24-33 */
enum COMPARISON_TYPE { EQ = 0, NE = 1, GT = 2, GE = 3, LT = 4, LE = 5, MAX = 6, MIN = 7 };
/* cuda/include/keyswitch/ks_enums.h, cuda/include/zk/zk_enums.h */
enum KS_TYPE { BIG_TO_SMALL = 0, SMALL_TO_BIG = 1 };
enum EXPAND_KIND { NO_CASTING = 0, CASTING = 1, SANITY_CHECK = 2 };
/* cuda/include/integer/integer.h:45-48 */
enum RERAND_MODE { RERAND_WITH_KS = 0, RERAND_WITHOUT_KS = 1 };
/* cuda/include/integer/integer.h:41-43 */
enum Direction { Trailing = 0, Leading = 1 };
enum BitValue { Zero = 0, One = 1 };

/* ------------------------------------------------------------------ device runtime
 * backends/tfhe-cuda-common/cuda/include/device.h:58-92 (cuda_bind.rs:5-150) */
void *cuda_create_stream_ffi(uint32_t gpu_index);
void cuda_destroy_stream(void *stream, uint32_t gpu_index);
void cuda_synchronize_stream(void *stream, uint32_t gpu_index);
uint32_t cuda_is_available(void);
void *cuda_malloc(uint64_t size, uint32_t gpu_index);
/* stream-ordered: an enqueue on `stream`, no device synchronisation, usable under stream capture — served by the library's own
 * arena (hip_backend_trim_allocator below; TFHE_HIP_MALLOC_ASYNC=sync|pool|pool_hipfree select a plain hipMalloc or the
 * runtime's hipMallocAsync pool, which corrupted live allocations on ROCm 7.2.0: INTEGRATION.md).  cuda_drop returns such a
 * block in stream order behind the work queued on `stream` so far (device.cu:176-226, 457-491). */
void *cuda_malloc_async(uint64_t size, void *stream, uint32_t gpu_index);
bool cuda_check_valid_malloc(uint64_t size, uint32_t gpu_index);
uint64_t cuda_device_total_memory(uint32_t gpu_index);
void cuda_memcpy_async_to_gpu(void *dest, const void *src, uint64_t size, void *stream, uint32_t gpu_index);
void cuda_memcpy_async_gpu_to_gpu(void *dest, void const *src, uint64_t size, void *stream, uint32_t gpu_index);
void cuda_memcpy_gpu_to_gpu(void *dest, void const *src, uint64_t size, uint32_t gpu_index);
void cuda_memcpy_async_to_cpu(void *dest, const void *src, uint64_t size, void *stream, uint32_t gpu_index);
void cuda_memset_async(void *dest, uint64_t val, uint64_t size, void *stream, uint32_t gpu_index);
int cuda_get_number_of_gpus(void);
int cuda_get_number_of_sms(void);
void cuda_synchronize_device(uint32_t gpu_index);
void cuda_drop(void *ptr, uint32_t gpu_index);

/* ------------------------------------------------------------------ classic PBS
 * backends/tfhe-cuda-backend/cuda/include/pbs/programmable_bootstrap.h:52-55,62-66,83-90,99-100
 * called from tfhe/src/core_crypto/gpu/ffi.rs:21-92
 * polynomial_size: a power of two in 256..16384 (the reference's range); glwe_dimension 1..3 up to 2048,
 * 1 from 4096 up.  The scratch query returns 0 device bytes up to 4096 (the accumulator stays in LDS) and
 * num_samples * (k+1) * N * 8 beyond. */
void cuda_convert_lwe_programmable_bootstrap_key_64_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src,
    uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
    uint32_t polynomial_size);

uint64_t scratch_cuda_programmable_bootstrap_64_async(
    void *stream, uint32_t gpu_index, int8_t **buffer, uint32_t lwe_dimension,
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count,
    uint32_t input_lwe_ciphertext_count, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);

void cuda_programmable_bootstrap_64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lut_vector,
    void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *bootstrapping_key,
    int8_t *buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples, uint32_t num_many_lut, uint32_t lut_stride);

void cleanup_cuda_programmable_bootstrap_64(void *stream, uint32_t gpu_index, int8_t **pbs_buffer);

/* extension: the shortint atomic pattern KS -> PBS (tfhe/src/shortint/atomic_pattern/standard.rs:162-199) in ONE
 * call on a scratch made by hip_scratch_keyswitch_programmable_bootstrap_64_async (the classic PBS scratch plus the
 * keyswitched list and its indexes; same parameters and cleanup as scratch_cuda_programmable_bootstrap_64_async, whose
 * own size the reference's callers track): lwe_array_in holds ciphertexts under the BIG key (dimension
 * glwe_dimension * polynomial_size), ksk the big -> small keyswitch key.  Two launches on `stream`, no allocation,
 * no host synchronisation. */
uint64_t hip_scratch_keyswitch_programmable_bootstrap_64_async(
    void *stream, uint32_t gpu_index, int8_t **buffer, uint32_t lwe_dimension,
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count,
    uint32_t input_lwe_ciphertext_count, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_keyswitch_programmable_bootstrap_64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out, void const *lwe_output_indexes,
    void const *lut_vector, void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *ksk, void const *bootstrapping_key, int8_t *buffer,
    uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t ks_base_log,
    uint32_t ks_level, uint32_t base_log, uint32_t level_count, uint32_t num_samples,
    uint32_t num_many_lut, uint32_t lut_stride);

/* extension: the same call for CHAINS of rounds in which a round's keyswitch reads exactly what the previous round's
 * bootstrap wrote (apply-lookup-table chains): the sample extraction of the bootstrap is fused with the digit pass of
 * the NEXT keyswitch.  flags: HIP_KSPBS_EMIT_DIGITS — the bootstrap also writes, for every output ciphertext, the
 * shifted keyswitch digits of its mask (decomposition ks_base_log / ks_level of this call) as the int8 A operands of the
 * keyswitch GEMM, into the scratch; HIP_KSPBS_INPUT_FROM_PREVIOUS — the caller states that lwe_array_in /
 * lwe_input_indexes are the lwe_array_out / lwe_output_indexes of the previous call on this scratch and that nothing
 * wrote to them since: the keyswitch starts from the emitted operands (the library checks pointers, count and
 * decomposition against what it recorded and falls back to its digit pass otherwise).  Emission is done by the
 * N = 2048, k = 1 throughput kernel (more than 256 LWEs) for keyswitch level counts padded to 4 or 8 with
 * base_log * level <= 30; elsewhere the flags change nothing.  Identical bits with and without the flags. */
#define HIP_KSPBS_EMIT_DIGITS 1u
#define HIP_KSPBS_INPUT_FROM_PREVIOUS 2u
void hip_keyswitch_programmable_bootstrap_chain_64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out, void const *lwe_output_indexes,
    void const *lut_vector, void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *ksk, void const *bootstrapping_key, int8_t *buffer,
    uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t ks_base_log,
    uint32_t ks_level, uint32_t base_log, uint32_t level_count, uint32_t num_samples,
    uint32_t num_many_lut, uint32_t lut_stride, uint32_t flags);

/* ------------------------------------------------------------------ multi-bit PBS
 * backends/tfhe-cuda-backend/cuda/include/pbs/programmable_bootstrap_multibit.h:9-40
 * called from tfhe/src/core_crypto/gpu/ffi.rs:208-309,789-835
 * polynomial_size: a power of two in 256..16384, glwe_dimension as for the classic PBS (1..3 up to 1024, 1..2 at
 * 2048, 1 beyond); grouping_factor 1..4.
 * The scratch holds everything a launch needs (nothing is allocated by the launch itself). */
bool has_support_to_cuda_programmable_bootstrap_cg_multi_bit(
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count,
    uint32_t num_samples, uint32_t max_shared_memory);

void cuda_convert_lwe_multi_bit_programmable_bootstrap_key_64_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src,
    uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
    uint32_t polynomial_size, uint32_t grouping_factor);

uint64_t scratch_cuda_multi_bit_programmable_bootstrap_64_async(
    void *stream, uint32_t gpu_index, int8_t **pbs_buffer,
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count,
    uint32_t input_lwe_ciphertext_count, bool allocate_gpu_memory);

void cuda_multi_bit_programmable_bootstrap_64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lut_vector,
    void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *bootstrapping_key,
    int8_t *buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t grouping_factor, uint32_t base_log,
    uint32_t level_count, uint32_t num_samples, uint32_t num_many_lut,
    uint32_t lut_stride);

void cleanup_cuda_multi_bit_programmable_bootstrap_64(void *stream, uint32_t gpu_index, int8_t **pbs_buffer);

/* The variant the reference's noise tests call (cuda/include/pbs/programmable_bootstrap_multibit.h:44-60; bound by
 * tfhe/src/core_crypto/gpu/ffi.rs:322-397): the input has ALREADY been through cuda_modulus_switch_multi_bit_64_async —
 * lwe_array_in = [ ciphertext, lwe_dimension + 1 words | its output, (lwe_dimension / grouping_factor) * 2^grouping_factor
 * words ] — and the keybundle reads its monomial degrees from the second part.  num_samples must be 1 and
 * polynomial_size 2048 (anything else panics, as there); scratch and cleanup are the standard ones. */
uint64_t scratch_cuda_multi_bit_programmable_bootstrap_noise_tests_64_async(
    void *stream, uint32_t gpu_index, int8_t **pbs_buffer,
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count,
    uint32_t input_lwe_ciphertext_count, bool allocate_gpu_memory);

void cleanup_cuda_multi_bit_programmable_bootstrap_noise_tests_64(
    void *stream, uint32_t gpu_index, int8_t **pbs_buffer);

void cuda_multi_bit_programmable_bootstrap_noise_tests_64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lut_vector,
    void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *bootstrapping_key,
    int8_t *buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t grouping_factor, uint32_t base_log,
    uint32_t level_count, uint32_t num_samples, uint32_t num_many_lut,
    uint32_t lut_stride);

/* ------------------------------------------------------------------ keyswitch
 * backends/tfhe-cuda-backend/cuda/include/keyswitch/keyswitch.h:16-21,35-41,69-72
 * called from tfhe/src/core_crypto/gpu/ffi.rs:503-618 (KSK upload is a plain memcpy, :620-627) */
void cuda_keyswitch_lwe_ciphertext_vector_64_64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *ksk, uint32_t lwe_dimension_in,
    uint32_t lwe_dimension_out, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples);

void cuda_keyswitch_gemm_64_64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *ksk, uint32_t lwe_dimension_in,
    uint32_t lwe_dimension_out, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples, bool uses_trivial_indexes);

/* u64 input ciphertexts, u32 key and u32 output ciphertexts (the KS32 atomic pattern):
 * backends/tfhe-cuda-backend/cuda/include/keyswitch/keyswitch.h:23-28,42-47; semantics
 * tfhe/src/core_crypto/algorithms/lwe_keyswitch.rs:331-447 (body rounded to 32 bits, base_log*level <= 32);
 * called from tfhe/src/core_crypto/gpu/ffi.rs:503-618 when the key scalar is u32. */
void cuda_keyswitch_lwe_ciphertext_vector_64_32_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *ksk, uint32_t lwe_dimension_in,
    uint32_t lwe_dimension_out, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples);

void cuda_keyswitch_gemm_64_32_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *ksk, uint32_t lwe_dimension_in,
    uint32_t lwe_dimension_out, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples, bool uses_trivial_indexes);

void cuda_closest_representable_64_async(void *stream, uint32_t gpu_index,
                                         void const *input, void *output,
                                         uint32_t base_log, uint32_t level_count);

/* ------------------------------------------------------------------ ciphertext helpers
 * backends/tfhe-cuda-backend/cuda/include/ciphertext.h:5-42
 * called from tfhe/src/core_crypto/gpu/ffi.rs:838-898 */
void cuda_convert_lwe_ciphertext_vector_to_gpu_64_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src,
    uint32_t number_of_cts, uint32_t lwe_dimension);
void cuda_convert_lwe_ciphertext_vector_to_cpu_64_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src,
    uint32_t number_of_cts, uint32_t lwe_dimension);
void cuda_glwe_sample_extract_64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *glwe_array_in, uint32_t const *nth_array, uint32_t num_nths,
    uint32_t num_lwes_to_extract_per_glwe, uint32_t num_lwes_stored_per_glwe,
    uint32_t glwe_dimension, uint32_t polynomial_size);
void cuda_modulus_switch_inplace_64_async(void *stream, uint32_t gpu_index,
                                          void *lwe_array_out, uint32_t size,
                                          uint32_t log_modulus);
void cuda_modulus_switch_64_async(void *stream, uint32_t gpu_index,
                                  void *lwe_out, const void *lwe_in,
                                  uint32_t size, uint32_t log_modulus);
void cuda_centered_modulus_switch_64_async(void *stream, uint32_t gpu_index,
                                           void *lwe_out, const void *lwe_in,
                                           uint32_t lwe_dimension,
                                           uint32_t log_modulus);
/* cuda/include/ciphertext.h:34-37 (modulus_switch.rs:386-488 tests it): the same switch with the body correction
   reduced as the bootstrap kernels reduce it, in one block of shape (block_dim_x, block_dim_y): 128 threads (the
   (64, 2) block of the throughput kernel: per wave, as pbs_fft_wave.hip's prologue) or 512 (the block kernels'
   prologue); any other size aborts as in the reference (torus.cuh:460-463) */
void cuda_centered_modulus_switch_cooperative_64_async(
    void *stream, uint32_t gpu_index, void *lwe_out, const void *lwe_in,
    uint32_t lwe_dimension, uint32_t log_modulus, uint32_t block_dim_x,
    uint32_t block_dim_y);
/* cuda/include/pbs/programmable_bootstrap.h:8-45: the transform of the path as launches of its own, what the reference's
   backend tests drive (tests_and_benchmarks/tests/test_fft.cpp, test_forward_fft16x4x16.cpp, test_fft16x4x16.cpp;
   gpu/algorithms/test/fft/mod.rs:268-294 + its golden spectrum; gpu/ffi.rs:1070-1085).  Polynomials "compressed":
   complex[i] = (p[i], p[i + N/2]).  polynomial_mul: negacyclic product, input1 is overwritten with its spectrum (as in the
   reference), sizes 256 .. 16384.  forward_fft_classic: spectrum in the native (tree) order; forward_fft16x4x16: in NATURAL
   frequency order, natural f <-> tree index bitreverse((N/2 - f) mod N/2); backward_fft16x4x16: its inverse WITHOUT the 1/(N/2)
   scaling.  The last four take polynomial_size 2048 only (abort otherwise, as the reference); is_supported: true. */
void cuda_fourier_polynomial_mul_async(void *stream, uint32_t gpu_index,
                                       void const *input1, void const *input2,
                                       void *output, uint32_t polynomial_size,
                                       uint32_t total_polynomials);
void cuda_fourier_polynomial_mul_fft16x4x16_async(
    void *stream, uint32_t gpu_index, void const *input1, void const *input2,
    void *output, uint32_t polynomial_size, uint32_t total_polynomials);
void cuda_forward_fft_classic_async(void *stream, uint32_t gpu_index,
                                    void const *input, void *output,
                                    uint32_t polynomial_size,
                                    uint32_t total_polynomials);
void cuda_forward_fft16x4x16_async(void *stream, uint32_t gpu_index,
                                   void const *input, void *output,
                                   uint32_t polynomial_size,
                                   uint32_t total_polynomials);
void cuda_backward_fft16x4x16_async(void *stream, uint32_t gpu_index,
                                    void const *input, void *output,
                                    uint32_t polynomial_size,
                                    uint32_t total_polynomials);
bool cuda_fft16x4x16_is_supported_async(uint32_t gpu_index);
/* cuda/include/ciphertext.h:45-50 (tfhe/src/core_crypto/gpu/ffi.rs:914-936): the multi-bit switch as its own launch
 * (noise tests only; production fuses it into the keybundle).  `size` words of lwe_array_in are read as
 * size / grouping_factor groups, 2^grouping_factor degrees are written per group ([group][subset], subset 0 = 0).
 * As in the reference the switch goes to 2 * degree whatever log_modulus says, and only degree 2048 is accepted. */
void cuda_modulus_switch_multi_bit_64_async(void *stream, uint32_t gpu_index,
                                            void *lwe_array_out,
                                            void *lwe_array_in, uint32_t size,
                                            uint32_t log_modulus,
                                            uint32_t degree,
                                            uint32_t grouping_factor);

/* ------------------------------------------------------------------ extensions (hip_*)
 * Goldilocks-NTT engine: same argument meaning as the classic PBS triple above, the key
 * buffer has the same byte size (n*(k+1)^2*l*N u64).  Semantics:
 * cc/algorithms/lwe_programmable_bootstrapping/ntt64_bnf_pbs.rs:469-539 and
 * cc/algorithms/lwe_bootstrap_key_conversion.rs:367-434 (bit-exact, integer only). */
void hip_convert_lwe_programmable_bootstrap_key_ntt64_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src,
    uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
    uint32_t polynomial_size);
void hip_programmable_bootstrap_ntt64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lut_vector,
    void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *bootstrapping_key,
    int8_t *buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples, uint32_t num_many_lut, uint32_t lut_stride);

/* The same engine on the f64 transform machinery of the throughput kernel (pbs_fft_wave.hip, split-key form): every
 * key word, switched to the prime and centred, is cut into 4 balanced 16-bit limbs kept in the Fourier domain; per
 * CMUX the digit transform is multiplied with each limb, the inverse transforms are rounded to the exact integer
 * products (|.| < 2^49; the distance from an integer is checked on every coefficient, the launch traps above 1/4) and
 * recombined modulo the prime.  Identical outputs to hip_programmable_bootstrap_ntt64_async.  Accepts N = 2048,
 * k = 1, one level, base_log 22 or 23 (hip_programmable_bootstrap_ntt64_split_supported).  The key buffer takes FOUR
 * times the bytes of the standard key: n*(k+1)^2*N*32.  The first launch on a scratch allocates the accumulators'
 * device buffer (not capturable; later launches are). */
bool hip_programmable_bootstrap_ntt64_split_supported(
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count,
    uint32_t base_log);
void hip_convert_lwe_programmable_bootstrap_key_ntt64_split_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src,
    uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
    uint32_t polynomial_size);
void hip_programmable_bootstrap_ntt64_split_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lut_vector,
    void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *bootstrapping_key,
    int8_t *buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples, uint32_t num_many_lut, uint32_t lut_stride);

/* Round-off check of the split-key engine.  A ciphertext whose f64 limb products were further than 1/4 from integers (the
 * bound on them is statistical: worst-case products of 2^49 leave 4 bits of headroom; never observed on a real parameter
 * set's data, reachable with adversarial constant polynomials) is RECOMPUTED by the integer Goldilocks kernel in a second
 * launch on the same stream, with the NTT-domain twin of the key that the conversion above made and the library keeps while
 * the split key's memory lives: the entry point's outputs are the exact ones whatever the data.  This call returns how many
 * ciphertexts went that way on this scratch since the last call (synchronises the stream, clears the count).  A split key
 * the library did not convert itself (copied in) has no twin: a raised flag then panics here or at cleanup_*. */
uint32_t hip_programmable_bootstrap_ntt64_split_roundoff_status(
    void *stream, uint32_t gpu_index, int8_t *buffer);

/* Exact-integer engine (negacyclic convolution mod 2^64 on the standard-domain key,
 * cc/algorithms/lwe_programmable_bootstrapping/karatsuba_pbs.rs:71-116,199-413).  O(N^2): a
 * verification engine; it reproduces the reference's golden *_karatsuba vectors bit for bit. */
void hip_convert_lwe_programmable_bootstrap_key_exact64_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src,
    uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
    uint32_t polynomial_size);
void hip_programmable_bootstrap_exact64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lut_vector,
    void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *bootstrapping_key,
    int8_t *buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples, uint32_t num_many_lut, uint32_t lut_stride);

/* Reference-order f64 engine: the blind rotation with tfhe-fft's radix-4 DIF Stockham plan and the reference's x86
 * conversion / multiply-accumulate forms, operation for operation (csrc/pbs_ref64.hip).  A verification engine:
 * it reproduces the reference's f64 golden vectors (apps/test-vectors, lwe_after_{id,spec}_pbs.cbor, made with
 * `experimental-force_fft_algo_dif4`) bit for bit on the MI355X.  glwe_dimension 1, polynomial_size <= 2048. */
void hip_convert_lwe_programmable_bootstrap_key_ref64_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src,
    uint32_t input_lwe_dim, uint32_t glwe_dim, uint32_t level_count,
    uint32_t polynomial_size);
void hip_programmable_bootstrap_ref64_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out,
    void const *lwe_output_indexes, void const *lut_vector,
    void const *lut_vector_indexes, void const *lwe_array_in,
    void const *lwe_input_indexes, void const *bootstrapping_key,
    int8_t *buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count,
    uint32_t num_samples, uint32_t num_many_lut, uint32_t lut_stride);

/* ------------------------------------------------------------------ radix integers ("next" row N1)
 * backends/tfhe-cuda-backend/cuda/include/integer/integer.h:52-65,100-113 (FFI structs),
 * :127-148 (apply_univariate_lut), :173-187 (integer_mult_inplace), :383-413 (propagate_single_carry,
 * add_and_propagate_single_carry); include/keyswitch/keyswitch.h:7-12; include/linear_algebra.h:26-28.
 * Called from tfhe/src/integer/gpu/mod.rs (cuda_backend_apply_univariate_lut,
 * cuda_backend_propagate_single_carry_assign, cuda_backend_unchecked_mul_assign, ...).
 *
 * Wired: classic and multi-bit keys (pbs_type), carry-in (uses_carry), FLAG_CARRY, FLAG_OVERFLOW (add_and_propagate),
 * boolean operands of integer_mult, many-LUT application; a round spreads over the GPUs of the CudaStreamsFFI by the
 * reference's thresholds (hip_integer_set_multi_gpu_threshold below).  Operands must be clean up to what an operation
 * accepts (degrees are checked when given: INTEGRATION.md).  Extension: a CudaRadixCiphertextFFI may hold a batch of integers
 * ([integer][block]); the scratch's num_blocks is the blocks PER integer and the launch handles
 * num_radix_blocks / num_blocks integers in the same rounds (capacity: hip_integer_scratch_batch). */
typedef struct {
  void *const *streams;
  uint32_t const *gpu_indexes;
  uint32_t gpu_count;
} CudaStreamsFFI;

typedef struct {
  void *ptr;
  uint64_t *degrees;
  uint64_t *noise_levels;
  uint32_t num_radix_blocks;
  uint32_t max_num_radix_blocks;
  uint32_t lwe_dimension;
} CudaRadixCiphertextFFI;

typedef struct {
  uint32_t input_lwe_dimension;
  uint32_t glwe_dimension;
  uint32_t polynomial_size;
  uint32_t base_log;
  uint32_t level_count;
  uint32_t big_lwe_dimension;
  uint32_t pbs_type; /* PBS_TYPE: MULTI_BIT = 0, CLASSICAL = 1 (pbs/pbs_enums.h:4) */
  uint32_t grouping_factor;
} CudaLweBootstrapKeyParamsFFI;

typedef struct {
  uint32_t input_lwe_dimension;
  uint32_t output_lwe_dimension;
  uint32_t base_log;
  uint32_t level_count;
} CudaLweKeyswitchKeyParamsFFI;

uint64_t scratch_cuda_apply_univariate_lut_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, void const *input_lut,
    CudaLweBootstrapKeyParamsFFI bsk_params, CudaLweKeyswitchKeyParamsFFI ksk_params,
    uint32_t input_lwe_ciphertext_count, uint32_t message_modulus, uint32_t carry_modulus,
    uint64_t lut_degree, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_apply_univariate_lut_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_radix_lwe,
    CudaRadixCiphertextFFI const *input_radix_lwe, int8_t *mem_ptr, void *const *ksks, void *const *bsks);
void cleanup_cuda_apply_univariate_lut_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* integer.h:135-160: `input_lut` is ONE accumulator that packs num_many_lut functions in sub-tables of lut_stride
 * coefficients (tfhe/src/shortint/engine/mod.rs:169-254); one keyswitch and one PBS per block, the PBS extracts
 * num_luts samples; function t of input block s is written to output block t * n + s. */
uint64_t scratch_cuda_apply_many_univariate_lut_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, void const *input_lut,
    CudaLweBootstrapKeyParamsFFI bsk_params, CudaLweKeyswitchKeyParamsFFI ksk_params,
    uint32_t num_radix_blocks, uint32_t message_modulus, uint32_t carry_modulus, uint32_t num_many_lut,
    uint64_t lut_degree, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_apply_many_univariate_lut_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_radix_lwe,
    CudaRadixCiphertextFFI const *input_radix_lwe, int8_t *mem_ptr, void *const *ksks, void *const *bsks,
    uint32_t num_luts, uint32_t lut_stride);
void cleanup_cuda_apply_many_univariate_lut_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);

void cuda_add_lwe_ciphertext_vector_inplace_64(
    void *stream, uint32_t gpu_index, CudaRadixCiphertextFFI *lwe_array_inout,
    CudaRadixCiphertextFFI const *input_2);

uint64_t scratch_cuda_propagate_single_carry_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus,
    uint32_t carry_modulus, uint32_t requested_flag, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
uint64_t scratch_cuda_add_and_propagate_single_carry_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus,
    uint32_t carry_modulus, uint32_t requested_flag, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_propagate_single_carry_64_inplace_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array, CudaRadixCiphertextFFI *carry_out,
    const CudaRadixCiphertextFFI *carry_in, int8_t *mem_ptr, void *const *bsks, void *const *ksks,
    uint32_t requested_flag, uint32_t uses_carry);
void cuda_add_and_propagate_single_carry_64_inplace_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lhs_array, const CudaRadixCiphertextFFI *rhs_array,
    CudaRadixCiphertextFFI *carry_out, const CudaRadixCiphertextFFI *carry_in, int8_t *mem_ptr,
    void *const *bsks, void *const *ksks, uint32_t requested_flag, uint32_t uses_carry);
void cleanup_cuda_propagate_single_carry_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void);
void cleanup_cuda_add_and_propagate_single_carry_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void);

uint64_t scratch_cuda_integer_mult_inplace_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, bool const is_boolean_left, bool const is_boolean_right,
    uint32_t message_modulus, uint32_t carry_modulus, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_integer_mult_inplace_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *radix_lwe_inout, bool const is_bool_left,
    CudaRadixCiphertextFFI const *radix_lwe_right, bool const is_bool_right, void *const *bsks,
    void *const *ksks, int8_t *mem_ptr, uint32_t polynomial_size, uint32_t num_blocks);
void cleanup_cuda_integer_mult_inplace_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);

/* Levelled block operations and the one-round / sequential operations built on the round driver (round 6).
 * integer.h:189-198 (negate with the correcting term, scalar addition), :312-347 (bitnot, bitop, scalar bitop),
 * :559-573 (sub_and_propagate_single_carry: requested_flag 0 or 2, no input carry — what the reference's callers pass,
 * integer/gpu/server_key/radix/sub.rs:222,347-400), :159-171 (full propagation, block after block).
 * negate / scalar_addition / bitnot / bitop / scalar_bitop / full_propagation take ONE integer per ciphertext as in the
 * reference (bitop: any number of blocks up to lwe_ciphertext_count x hip_integer_scratch_batch); sub takes the batch
 * extension described above. */
void cuda_negate_ciphertext_64(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                               CudaRadixCiphertextFFI const *lwe_array_in, uint32_t message_modulus,
                               uint32_t carry_modulus, uint32_t num_radix_blocks);
void cuda_scalar_addition_ciphertext_64_inplace(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
                                                void const *scalar_input, void const *h_scalar_input,
                                                uint32_t num_scalars, uint32_t message_modulus, uint32_t carry_modulus);
void cuda_bitnot_ciphertext_64(CudaStreamsFFI streams, CudaRadixCiphertextFFI *radix_ciphertext,
                               uint32_t ct_message_modulus, uint32_t param_message_modulus,
                               uint32_t param_carry_modulus);
uint64_t scratch_cuda_integer_bitop_inplace_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t lwe_ciphertext_count, uint32_t message_modulus,
    uint32_t carry_modulus, enum BITOP_TYPE op_type, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
uint64_t scratch_cuda_integer_scalar_bitop_inplace_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t lwe_ciphertext_count, uint32_t message_modulus,
    uint32_t carry_modulus, enum BITOP_TYPE op_type, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_integer_bitop_inplace_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_inout,
                                         CudaRadixCiphertextFFI const *lwe_array_2, int8_t *mem_ptr,
                                         void *const *bsks, void *const *ksks);
void cuda_integer_scalar_bitop_inplace_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_inout,
                                                void const *clear_blocks, void const *h_clear_blocks,
                                                uint32_t num_clear_blocks, int8_t *mem_ptr, void *const *bsks,
                                                void *const *ksks);
void cleanup_cuda_integer_bitop_inplace_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
void cleanup_cuda_integer_scalar_bitop_inplace_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
uint64_t scratch_cuda_sub_and_propagate_single_carry_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
    uint32_t requested_flag, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_sub_and_propagate_single_carry_64_inplace_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lhs_array, const CudaRadixCiphertextFFI *rhs_array,
    CudaRadixCiphertextFFI *carry_out, const CudaRadixCiphertextFFI *carry_in, int8_t *mem_ptr,
    void *const *bsks, void *const *ksks, uint32_t requested_flag, uint32_t uses_carry);
void cleanup_cuda_sub_and_propagate_single_carry_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* integer.h:415-431: lhs -= rhs and the borrow (1 - the carry of lhs + (2^bits - rhs)); no input borrow */
uint64_t scratch_cuda_integer_overflowing_sub_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
    uint32_t compute_overflow, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_integer_overflowing_sub_64_inplace_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lhs_array, const CudaRadixCiphertextFFI *rhs_array,
    CudaRadixCiphertextFFI *overflow_block, const CudaRadixCiphertextFFI *input_borrow, int8_t *mem_ptr,
    void *const *bsks, void *const *ksks, uint32_t compute_overflow, uint32_t uses_input_borrow);
void cleanup_cuda_integer_overflowing_sub_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void);
uint64_t scratch_cuda_full_propagation_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus, uint32_t carry_modulus,
    bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_full_propagation_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *input_blocks,
                                            int8_t *mem_ptr, void *const *ksks, void *const *bsks,
                                            uint32_t num_blocks);
void cleanup_cuda_full_propagation_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* integer.h:246-276 (comparison: unsigned operands, EQ ... LE into block 0 of the output, MAX / MIN over all blocks) and
 * :349-365 (cmux).  Orderings ride on the subtraction's carry tree without its result round, equality on sums of block results. */
uint64_t scratch_cuda_integer_comparison_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t lwe_ciphertext_count, uint32_t message_modulus,
    uint32_t carry_modulus, enum COMPARISON_TYPE op_type, bool is_signed, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_integer_comparison_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                                      CudaRadixCiphertextFFI const *lwe_array_1,
                                      CudaRadixCiphertextFFI const *lwe_array_2, int8_t *mem_ptr, void *const *bsks,
                                      void *const *ksks);
void cleanup_cuda_integer_comparison_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
uint64_t scratch_cuda_integer_scalar_comparison_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t lwe_ciphertext_count, uint32_t message_modulus,
    uint32_t carry_modulus, enum COMPARISON_TYPE op_type, bool is_signed, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_integer_scalar_comparison_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                                             CudaRadixCiphertextFFI const *lwe_array_in, void const *scalar_blocks,
                                             void const *h_scalar_blocks, int8_t *mem_ptr, void *const *bsks,
                                             void *const *ksks, uint32_t num_scalar_blocks);
void cleanup_cuda_integer_scalar_comparison_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
uint64_t scratch_cuda_cmux_64_async(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                                    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t lwe_ciphertext_count,
                                    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
                                    enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_cmux_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                        CudaRadixCiphertextFFI const *lwe_condition, CudaRadixCiphertextFFI const *lwe_array_true,
                        CudaRadixCiphertextFFI const *lwe_array_false, int8_t *mem_ptr, void *const *bsks,
                        void *const *ksks);
void cleanup_cuda_cmux_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* integer.h:200-228: logical shift by a clear amount (LEFT_SHIFT / RIGHT_SHIFT; the rotations are refused): a move by whole
 * blocks plus one bivariate round when bits remain */
uint64_t scratch_cuda_logical_scalar_shift_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
    enum SHIFT_OR_ROTATE_TYPE shift_type, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void cuda_logical_scalar_shift_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array, uint32_t shift,
                                                int8_t *mem_ptr, void *const *bsks, void *const *ksks);
void cleanup_cuda_logical_scalar_shift_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void);

/* extensions: integers per launch the NEXT scratch_* call is sized for (default 1), and the number
 * of PBS one multiplication issues per integer (for throughput accounting) */
void hip_integer_scratch_batch(uint32_t num_integers);
/* blocks per GPU from which a KS -> PBS round of the radix layer spreads over one more GPU of its CudaStreamsFFI.
 * 0 (default): the reference's rule, cuda/src/utils/helper_multi_gpu.cu:16-48 (get_active_gpu_count) — 12 for
 * multi-bit keys, (compute units of the first GPU) + 1 for classic ones.  The stream set may also name the same GPU
 * several times (one stream each).  hip_integer_active_gpu_count: how many GPUs of a set of gpu_count a round of
 * num_blocks blocks uses under the current setting (pbs_type as PBS_TYPE: MULTI_BIT = 0, CLASSICAL = 1). */
void hip_integer_set_multi_gpu_threshold(uint32_t blocks_per_gpu);
uint32_t hip_integer_active_gpu_count(uint32_t num_blocks, uint32_t gpu_count, uint32_t pbs_type, uint32_t first_gpu);
uint64_t hip_integer_mult_pbs_count(int8_t *mem_ptr);
uint64_t hip_integer_propagate_pbs_count(uint32_t num_blocks);

/* ------------------------------------------------------------------ ciphertext compression (extensions)
 * What tfhe/src/shortint/list_compression/compression.rs:17-254 computes and the reference's GPU backend serves with
 * the packing keyswitch of cuda/include/keyswitch/keyswitch.h and the compress / decompress entry points of
 * cuda/include/integer/compression/compression.h — here under hip_ names and with argument lists of this library's
 * own: scalars, device pointers and the FFI structs above.  The reference-named compression symbols remain link stubs
 * (INTEGRATION.md).  Single GPU: everything runs on entry 0 of
 * `streams`; the multi-GPU round of the decompression bootstrap is not implemented.
 *
 * Packing keyswitch key: [input_lwe_dimension][level_count][(glwe_dimension + 1) * polynomial_size] u64 on the device,
 * row idx of an input element holding level level_count - idx (lwe_packing_keyswitch_key.rs; a plain memcpy uploads it).
 * glwe_dimension >= 1, polynomial_size a power of two >= 16, base_log * level_count < 64.
 *
 * hip_packing_keyswitch_lwe_list_to_glwe_64_async (core level; core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187,
 * 296-379): lwe_array_in holds num_lwes contiguous LWEs; every chunk of lwe_per_glwe of them (the last may be partial)
 * becomes one GLWE  sum_i X^i * G_i  of glwe_array_out ((glwe_dimension + 1) * polynomial_size words each, not modulus
 * switched).  Panics: lwe_per_glwe > polynomial_size, num_lwes above the scratch's, parameters other than the scratch's. */
uint64_t hip_scratch_packing_keyswitch_lwe_list_to_glwe_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t input_lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t num_lwes, bool allocate_gpu_memory);
void hip_packing_keyswitch_lwe_list_to_glwe_64_async(
    CudaStreamsFFI streams, void *glwe_array_out, void const *lwe_array_in, void const *fp_ksk, int8_t *mem_ptr,
    uint32_t input_lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t base_log,
    uint32_t level_count, uint32_t num_lwes, uint32_t lwe_per_glwe);
void hip_cleanup_packing_keyswitch_lwe_list_to_glwe_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* Compress (compression.rs:17-133): every block of lwe_array_in (clean: degrees, when given, must be below
 * message_modulus) is multiplied by message_modulus, chunks of lwe_per_glwe blocks are packed into GLWEs, the first
 * glwe_dimension * polynomial_size + lwe_per_glwe values of each are switched to storage_log_modulus (1..63) bits and
 * bit-packed, least significant first (compressed_modulus_switched_glwe_ciphertext.rs:171-250), at a uniform stride of
 * ceil(values * bits / 64) words per GLWE; the padding bits are zero.  packed_out: device array of
 * hip_integer_compressed_size_words(...) words.  fp_ksks: one packing key per stream of the set (entry 0 is used).
 * Panics: more blocks than the scratch's num_radix_blocks, a block with a carry, another input LWE dimension. */
uint64_t hip_scratch_integer_compress_radix_ciphertext_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t input_lwe_dimension, uint32_t compression_glwe_dimension,
    uint32_t compression_polynomial_size, uint32_t ks_base_log, uint32_t ks_level, uint32_t num_radix_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, uint32_t lwe_per_glwe, uint32_t storage_log_modulus,
    bool allocate_gpu_memory);
void hip_integer_compress_radix_ciphertext_64_async(
    CudaStreamsFFI streams, void *packed_out, CudaRadixCiphertextFFI const *lwe_array_in, void *const *fp_ksks,
    int8_t *mem_ptr);
void hip_cleanup_integer_compress_radix_ciphertext_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* Decompress (compression.rs:164-254): for every h_indexes[i] (a HOST array, as in the reference) the LWE of dimension
 * compression_glwe_dimension * compression_polynomial_size at that position of the packed list is extracted straight
 * from the packed words and bootstrapped — no keyswitch — with the decompression key bsks[0] (classic or multi-bit by
 * bsk_params.pbs_type, Fourier domain as the conversion functions above leave it; its input_lwe_dimension is the
 * compression GLWE's) and the rescaling identity table (compression.rs:137-162) into block i of lwe_array_out, a clean
 * block under the big compute key.  total_lwe_bodies_count: the blocks the list was compressed from.
 * Panics: an index at or above total_lwe_bodies_count, more indexes than the scratch's num_blocks_to_decompress or the
 * output's blocks, indexes that are not non-decreasing in GLWE index (index / lwe_per_glwe; the order within a GLWE is
 * free), message_modulus != carry_modulus. */
uint64_t hip_scratch_integer_decompress_radix_ciphertext_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    uint32_t compression_glwe_dimension, uint32_t compression_polynomial_size, uint32_t lwe_per_glwe,
    uint32_t storage_log_modulus, uint32_t num_blocks_to_decompress, uint32_t message_modulus, uint32_t carry_modulus,
    bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_decompress_radix_ciphertext_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out, void const *packed_in,
    uint32_t total_lwe_bodies_count, uint32_t const *h_indexes, uint32_t num_indexes, void *const *bsks,
    int8_t *mem_ptr);
void hip_cleanup_integer_decompress_radix_ciphertext_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* GLWE glwe_index of a packed list, unpacked (values shifted back to the top of the word) into
 * (glwe_dimension + 1) * polynomial_size words; the body coefficients beyond that GLWE's count are zero. */
void hip_integer_extract_glwe_64_async(
    CudaStreamsFFI streams, void *glwe_out, void const *packed_in, uint32_t glwe_index, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t lwe_per_glwe, uint32_t storage_log_modulus, uint32_t total_lwe_bodies_count);
/* pure host helper: u64 words of the packed list of total_blocks blocks */
uint64_t hip_integer_compressed_size_words(
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t lwe_per_glwe, uint32_t storage_log_modulus,
    uint32_t total_blocks);

/* ------------------------------------------------------------------ compression of squashed-noise lists (extensions)
 * What tfhe/src/shortint/list_compression/noise_squashing_compression.rs computes over Scalar = u128 and the reference's
 * GPU backend serves with cuda_packing_keyswitch_lwe_list_to_glwe_128_async, cuda_integer_{compress,decompress}_radix_
 * ciphertext_128_async and cuda_integer_extract_glwe_128_async — here under hip_ names with the argument lists of the
 * _64 entry points above (the reference-named *_128 symbols remain link stubs).  A u128 word is two u64
 * words, (lo, hi).  Single GPU: entry 0 of `streams`.
 *
 * Packing keyswitch key: [input_lwe_dimension][level_count][(glwe_dimension + 1) * polynomial_size] u128 on the device,
 * row idx of an input element holding level level_count - idx (a plain memcpy uploads it).  1 <= base_log <= 62,
 * base_log * level_count <= 128.  Two kernels compute the decomposed products with identical words: a general one on the
 * vector ALU (any shape) and one on the int8 matrix cores, which needs the key a second time in a byte-plane layout:
 * hip_lwe_packing_keyswitch_key_128_planes_size_bytes gives that layout's size, or 0 where the matrix-core kernel
 * declines the shape (input_lwe_dimension * level_count not a multiple of 32, or ceil((base_log + 1) / 8) *
 * input_lwe_dimension * level_count * 2^14 >= 2^31: an int32 accumulator could overflow);
 * hip_convert_lwe_packing_keyswitch_key_128_async builds it from the key ON THE DEVICE, once, when the key is uploaded.
 * Every launch takes both pointers; fp_ksk_planes may be null (then the general kernel runs).
 * hip_backend_set_pks128_kernel: 0 = automatic, 1 = general kernel, 2 = matrix-core kernel wherever it carries the shape
 * and the planes are given; hip_backend_last_pks128_path: 0 general, 1 matrix core (tests).
 * Small batches split K = input_lwe_dimension * level_count over up to 8 partial sums that the epilogue adds (same words):
 * hip_backend_set_pks128_max_parts caps that count (0 = no cap, 1 = the whole K in one pass: every accumulator of the
 * matrix-core kernel then runs over all K terms), hip_backend_last_pks128_parts reports what the last call took (tests). */
void hip_backend_set_pks128_kernel(uint32_t which);
uint32_t hip_backend_last_pks128_path(void);
void hip_backend_set_pks128_max_parts(uint32_t parts);
uint32_t hip_backend_last_pks128_parts(void);
uint64_t hip_lwe_packing_keyswitch_key_128_planes_size_bytes(
    uint32_t input_lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t base_log,
    uint32_t level_count);
void hip_convert_lwe_packing_keyswitch_key_128_async(
    CudaStreamsFFI streams, void *dest_planes, void const *src_key, uint32_t input_lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count);
/* Core level (core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187, 296-379): every chunk of lwe_per_glwe of the
 * num_lwes contiguous u128 LWEs of lwe_array_in (the last may be partial) becomes one GLWE  sum_i X^i * G_i  of
 * glwe_array_out, (glwe_dimension + 1) * polynomial_size u128 words each, not modulus switched.
 * Panics: lwe_per_glwe > polynomial_size, num_lwes above the scratch's, parameters other than the scratch's, base_log
 * above 62, base_log * level_count above 128. */
uint64_t hip_scratch_packing_keyswitch_lwe_list_to_glwe_128_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t input_lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t num_lwes, bool allocate_gpu_memory);
void hip_packing_keyswitch_lwe_list_to_glwe_128_async(
    CudaStreamsFFI streams, void *glwe_array_out, void const *lwe_array_in, void const *fp_ksk,
    void const *fp_ksk_planes, int8_t *mem_ptr, uint32_t input_lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t num_lwes, uint32_t lwe_per_glwe);
void hip_cleanup_packing_keyswitch_lwe_list_to_glwe_128(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* Compress: the u128 blocks of lwe_array_in (a squashed radix ciphertext; no multiplication by message_modulus) are
 * packed lwe_per_glwe per GLWE; the first glwe_dimension * polynomial_size + lwe_per_glwe values of every GLWE are
 * switched to storage_log_modulus = s bits, (x + 2^(127-s)) >> (128-s), the identity at s = 128 (1..128), and bit-packed
 * least significant first into ceil(values * s / 128) u128 words per GLWE (PackedIntegers,
 * compressed_modulus_switched_glwe_ciphertext.rs:171-250); the padding bits are zero.  packed_out: device array of
 * hip_integer_compressed_size_words_128(...) u128 words.  fp_ksks / fp_ksk_planes: one key (and one plane layout, or
 * null) per stream of the set (entry 0 is used).
 * Panics: more blocks than the scratch's num_radix_blocks, another input LWE dimension than the key's. */
uint64_t hip_scratch_integer_compress_radix_ciphertext_128_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t input_lwe_dimension, uint32_t compression_glwe_dimension,
    uint32_t compression_polynomial_size, uint32_t ks_base_log, uint32_t ks_level, uint32_t num_radix_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, uint32_t lwe_per_glwe, uint32_t storage_log_modulus,
    bool allocate_gpu_memory);
void hip_integer_compress_radix_ciphertext_128_async(
    CudaStreamsFFI streams, void *packed_out, CudaRadixCiphertextFFI const *lwe_array_in, void *const *fp_ksks,
    void *const *fp_ksk_planes, int8_t *mem_ptr);
void hip_cleanup_integer_compress_radix_ciphertext_128(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* Decompress: no bootstrap.  For every h_indexes[i] (a HOST array) the u128 LWE of dimension compression_glwe_dimension
 * * compression_polynomial_size at that position of the packed list is unpacked, scaled back by << (128 - s) and sample
 * extracted into block i of lwe_array_out.  Panics as the _64 entry point: an index at or above total_lwe_bodies_count,
 * more indexes than the scratch's or the output's blocks, indexes not non-decreasing in GLWE index. */
uint64_t hip_scratch_integer_decompress_radix_ciphertext_128_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t compression_glwe_dimension, uint32_t compression_polynomial_size,
    uint32_t lwe_per_glwe, uint32_t storage_log_modulus, uint32_t num_blocks_to_decompress, uint32_t message_modulus,
    uint32_t carry_modulus, bool allocate_gpu_memory);
void hip_integer_decompress_radix_ciphertext_128_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out, void const *packed_in,
    uint32_t total_lwe_bodies_count, uint32_t const *h_indexes, uint32_t num_indexes, int8_t *mem_ptr);
void hip_cleanup_integer_decompress_radix_ciphertext_128(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* GLWE glwe_index of a packed list as (glwe_dimension + 1) * polynomial_size u128 words; the body coefficients beyond
 * that GLWE's count are zero. */
void hip_integer_extract_glwe_128_async(
    CudaStreamsFFI streams, void *glwe_out, void const *packed_in, uint32_t glwe_index, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t lwe_per_glwe, uint32_t storage_log_modulus, uint32_t total_lwe_bodies_count);
/* pure host helper: u128 words of the packed list of total_blocks blocks */
uint64_t hip_integer_compressed_size_words_128(
    uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t lwe_per_glwe, uint32_t storage_log_modulus,
    uint32_t total_blocks);

/* ------------------------------------------------------------------ expansion of compact ciphertext lists (extensions)
 * cuda/include/zk/zk.h:10-27 (scratch_cuda_expand_without_verification_64_async, cuda_expand_without_verification_64_async,
 * cleanup_cuda_expand_without_verification_64; caller: tfhe/src/integer/gpu/ciphertext/compact_list.rs expand), under hip_
 * names with the reference's parameter lists.  The reference-named symbols remain link stubs.
 *
 * lwe_flattened_compact_array_in: for every compact list l, n_c mask words then num_lwes_per_compact_list[l] body words, the
 * lists end to end, on the device; n_c = casting_ksk_params.input_lwe_dimension, any n_c >= 1, 1 <= bodies per list <= n_c.
 * Body d of a list expands to the LWE (mask * X^d in Z[X]/(X^n_c + 1), body d); num_lwes = the bodies of all lists.
 *   NO_CASTING:   lwe_array_out receives the num_lwes expanded LWEs of dimension n_c.  The key arguments are not read.
 *   CASTING:      lwe_array_out receives 2 * num_lwes LWEs of dimension glwe_dimension * polynomial_size: block 2i is
 *                 x % message_modulus of the value x packed in body i, block 2i + 1 is (x / carry_modulus) % message_modulus;
 *                 a block q with is_boolean_array[q] set is clamped to {0, 1}.  BIG_TO_SMALL: casting_keys[g] (n_c -> the
 *                 bootstrap key's input dimension) is the keyswitch key of the one keyswitch + bootstrap round, which shards
 *                 over the stream set like every round.  SMALL_TO_BIG: casting_keys[0] (n_c -> glwe_dimension *
 *                 polynomial_size) first, on the first GPU, then the round with computing_ksks.
 *   SANITY_CHECK: BIG_TO_SMALL only; blocks 2i and 2i + 1 both receive the packed value of body i (identity table).
 * The scratch call builds and uploads everything a launch needs (a per-output table of mask offset and rotation, the
 * round's indexes and tables) and reads the host arrays only then; a launch enqueues one expansion kernel, for
 * SMALL_TO_BIG one keyswitch, and the round: no host-to-device copy, no allocation, no synchronisation.
 * Panics: zero lists, a list of zero bodies or of more than n_c, is_boolean_array_len < 2 * num_lwes (pad with false),
 * CASTING with carry_modulus != message_modulus, SANITY_CHECK with SMALL_TO_BIG, key dimensions that do not chain, a launch on
 * a scratch created with allocate_gpu_memory = false. */
uint64_t hip_scratch_expand_without_verification_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t glwe_dimension, uint32_t polynomial_size,
    CudaLweKeyswitchKeyParamsFFI computing_ksk_params, CudaLweKeyswitchKeyParamsFFI casting_ksk_params, uint32_t pbs_level,
    uint32_t pbs_base_log, uint32_t grouping_factor, const uint32_t *num_lwes_per_compact_list, const bool *is_boolean_array,
    const uint32_t is_boolean_array_len, uint32_t num_compact_lists, uint32_t message_modulus, uint32_t carry_modulus,
    enum PBS_TYPE pbs_type, enum KS_TYPE casting_key_type, bool allocate_gpu_memory, enum EXPAND_KIND expand_kind,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_expand_without_verification_64_async(
    CudaStreamsFFI streams, void *lwe_array_out, const void *lwe_flattened_compact_array_in, int8_t *mem_ptr,
    void *const *bsks, void *const *computing_ksks, void *const *casting_keys);
void hip_cleanup_expand_without_verification_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);

/* ------------------------------------------------------------------ re-randomisation (extensions)
 * cuda/include/integer/rerand.h:6-19 (scratch_cuda_rerand_64_async, cuda_rerand_64_async, cleanup_cuda_rerand_64; caller:
 * tfhe/src/integer/gpu/ciphertext/re_randomization.rs), under hip_ names with the reference's parameter lists.  The
 * reference-named symbols remain link stubs.
 *
 * Block o < lwe_ciphertext_count of lwe_array gains, in place, a fresh encryption of zero: body o of ONE compact list
 * (n mask words, then at least lwe_ciphertext_count body words, on the device; n = ksk_params.input_lwe_dimension, any
 * n >= 1), expanded to (mask * X^o in Z[X]/(X^n + 1), body o).
 *   RERAND_WITHOUT_KS: the blocks are under the list's key (rows of n + 1 words).  One kernel rotates the mask and adds
 *                      in place: no temporary, every row read once and written once.  The other three fields of
 *                      ksk_params are not read; ksk may be null; the scratch holds nothing on the device.
 *   RERAND_WITH_KS:    the blocks are under ksk_params.output_lwe_dimension (the reference files this dimension as the
 *                      "small" one of its radix parameters, cuda/src/integer/rerand.cu:12-16, although it is the compute
 *                      key's).  The zeros are expanded into the scratch, keyswitched with ksk[0] and added.
 * Everything runs on the first stream of the set; a launch copies nothing to the device, allocates nothing and does not
 * synchronise.  message_modulus and carry_modulus are part of the reference's list and only validated.
 * Panics: lwe_ciphertext_count 0 or above n (one list has one mask), an unknown mode, a launch on a scratch created with
 * allocate_gpu_memory = false or on a scratch of another kind, RERAND_WITH_KS with a null ksk. */
uint64_t hip_scratch_rerand_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                     CudaLweKeyswitchKeyParamsFFI ksk_params,
                                     uint32_t lwe_ciphertext_count,
                                     uint32_t message_modulus,
                                     uint32_t carry_modulus,
                                     bool allocate_gpu_memory,
                                     enum RERAND_MODE rerand_type);
void hip_rerand_64_async(
    CudaStreamsFFI streams, void *lwe_array,
    const void *lwe_flattened_encryptions_of_zero_compact_array_in,
    int8_t *mem_ptr, void *const *ksk);
void hip_cleanup_rerand_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);

/* ------------------------------------------------------------------ oblivious pseudo-random bits (extensions)
 * cuda/include/integer/integer.h:664-678 (scratch_cuda_integer_grouped_oprf_64_async, cuda_integer_grouped_oprf_64_async,
 * cleanup_cuda_integer_grouped_oprf_64; tfhe/src/shortint/oprf.rs), under hip_ names with the reference's parameter lists.
 * The reference-named symbols remain link stubs, and so do the custom-range OPRF and the bitonic shuffle.
 *
 * seeded_lwe_input: num_blocks_to_process LWEs of dimension bsk_params.input_lwe_dimension on the device, their words
 * derived from a seed by the caller and already multiples of 2^64 / (2 * polynomial_size).  They are bootstrapped as they
 * are — no keyswitch; ksk_params takes no part, as in the reference — with the table of their bit count b (coefficient x
 * holds (2 * (x / (2N / 2^b)) + 1) * delta / 2, delta = 2^(63 - log2 carry - log2 message), no input encoding), and
 * (2^b - 1) * delta / 2 is added to the body: block i of radix_lwe_out then holds b uniform bits, b = log2 message_modulus
 * for every block but the last, which takes what remains of total_random_bits.  Degrees are set to 2^b - 1, noise levels
 * to nominal.  Classic and multi-bit keys; the bootstrap is a round of the radix layer and shards over the stream set.
 * Panics: num_blocks_to_process != ceil(total_random_bits / log2 message_modulus), moduli that are no powers of two, a
 * launch with another block count than the scratch's, on a size-only scratch or on a scratch of another kind. */
uint64_t hip_scratch_integer_grouped_oprf_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks_to_process,
    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    uint32_t total_random_bits, enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_grouped_oprf_64_async(CudaStreamsFFI streams,
                                       CudaRadixCiphertextFFI *radix_lwe_out,
                                       const void *seeded_lwe_input,
                                       uint32_t num_blocks_to_process,
                                       int8_t *mem, void *const *bsks);
void hip_cleanup_integer_grouped_oprf_64(CudaStreamsFFI streams,
                                         int8_t **mem_ptr_void);

/* ------------------------------------------------------------------ sum of ciphertexts, scalar multiplication (extensions)
 * cuda/include/integer/integer.h:433-463 and :862-864 under hip_ names with the reference's parameter lists; the
 * reference-named symbols remain link stubs.
 * partial_sum_ciphertexts_vec: radix_lwe_vec holds V integers of num_blocks_in_radix blocks, [v][block]; degrees are
 * read from radix_lwe_vec->degrees when given (otherwise every block counts as message_modulus - 1), blocks of degree 0
 * are left out.  radix_lwe_out may be the first integer of the vector.  V = 1 copies, V = 2 adds.  With
 * reduce_degrees_for_single_carry_propagation every output block ends at a degree of 2 message_modulus - 2 at most
 * (what propagate_single_carry accepts), without it at message_modulus * carry_modulus - 1 at most.  Degrees and noise
 * levels of the output are written back.  The plan of a sum depends on the degrees: it is made by the call and kept until
 * a call brings other degrees.  hip_partial_sum_ciphertexts_vec_pbs_count: bootstraps the last call issued.
 * integer_scalar_mul: in place on clean blocks; lwe_array may hold a batch of integers (hip_integer_scratch_batch before
 * the scratch call), all multiplied by the same scalar.  decomposed_scalar (num_scalars bits, least significant first)
 * and has_at_least_one_set (message bits entries) are host arrays; bits at or above the integer's width are ignored.
 * hip_integer_scalar_mul_pbs_count: bootstraps per integer for that scalar (shifted blocks, column sums, propagation). */
uint64_t hip_scratch_partial_sum_ciphertexts_vec_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks_in_radix,
    uint32_t max_num_radix_in_vec, uint32_t message_modulus,
    uint32_t carry_modulus, bool reduce_degrees_for_single_carry_propagation,
    bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_partial_sum_ciphertexts_vec_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *radix_lwe_out,
    CudaRadixCiphertextFFI *radix_lwe_vec, int8_t *mem_ptr, void *const *bsks,
    void *const *ksks);
void hip_cleanup_partial_sum_ciphertexts_vec_64(CudaStreamsFFI streams,
                                                int8_t **mem_ptr_void);
uint64_t hip_partial_sum_ciphertexts_vec_pbs_count(int8_t *mem_ptr);
uint64_t hip_scratch_integer_scalar_mul_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, uint32_t num_scalar_bits,
    bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_scalar_mul_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
    uint64_t const *decomposed_scalar, uint64_t const *has_at_least_one_set,
    int8_t *mem_ptr, void *const *bsks, void *const *ksks,
    uint32_t polynomial_size, uint32_t message_modulus, uint32_t num_scalars);
void hip_cleanup_integer_scalar_mul_64(CudaStreamsFFI streams,
                                       int8_t **mem_ptr_void);
uint64_t hip_integer_scalar_mul_pbs_count(int8_t *mem_ptr,
                                          uint64_t const *decomposed_scalar,
                                          uint32_t num_scalars);
void hip_small_scalar_multiplication_integer_64_inplace_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array, uint64_t scalar,
    const uint32_t message_modulus, const uint32_t carry_modulus);
/* benches: out[g] = sum of the pool rows members[offsets[g] .. offsets[g + 1]) by the column-sum kernel of the
 * multiplication (which = 0) or by the two-base gather-sum kernel of the sum and the scalar multiplication (which = 1) */
void hip_test_group_sum_async(void *stream, uint32_t gpu_index, uint32_t which, void *out, void const *pool,
                              void const *offsets, void const *members, uint32_t words, uint32_t groups);

/* ------------------------------------------------------------------ shifts and rotations (extensions)
 * cuda/include/integer/integer.h:212-228 (arithmetic shift by a clear amount), :367-381 (rotation by a clear amount) and
 * :230-244 (shift / rotation by an encrypted amount) under hip_ names with the reference's parameter lists; the
 * reference-named symbols remain link stubs.  All three work in place on clean blocks; lwe_array may hold a batch of
 * integers of num_blocks blocks (hip_integer_scratch_batch before the scratch call), lwe_shift then holds as many.
 * Signed values are two's complement in the same blocks.
 * arithmetic_scalar_shift: RIGHT_SHIFT only (LEFT_SHIFT is refused: it is the logical shift).  A move by whole blocks and
 *   one round; shift = 0 does nothing, shift >= bits turns every block into the sign's padding block, one bit per block
 *   needs no bootstrap.
 * scalar_rotate: LEFT_ROTATE / RIGHT_ROTATE by n mod bits; a rotation by whole blocks and, when bits remain, one round.
 * shift_and_rotate: shift_type LEFT_SHIFT / RIGHT_SHIFT / LEFT_ROTATE / RIGHT_ROTATE, is_signed makes RIGHT_SHIFT
 *   arithmetic.  Needs message_modulus * carry_modulus >= 8 and a power of two as message modulus; the shifts also what
 *   the unsigned comparison needs (16 values per block).  A shift by bits or more gives 0 (all ones for a negative
 *   arithmetic operand).  A rotation rotates by (amount mod 2^m) mod bits, m = ceil(log2 bits): when bits is no power of
 *   two the m control bits capture amounts up to 2^m - 1, as in the reference's GPU code.  Outputs are clean (degree
 *   message_modulus - 1, noise level 1); lwe_shift is not written.
 * hip_integer_shift_and_rotate_pbs_count: bootstraps per integer of one call on that scratch. */
uint64_t hip_scratch_integer_arithmetic_scalar_shift_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
    uint32_t message_modulus, uint32_t carry_modulus,
    enum SHIFT_OR_ROTATE_TYPE shift_type, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_arithmetic_scalar_shift_64_inplace_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array, uint32_t shift,
    int8_t *mem_ptr, void *const *bsks, void *const *ksks);
void hip_cleanup_integer_arithmetic_scalar_shift_64_inplace(CudaStreamsFFI streams,
                                                            int8_t **mem_ptr_void);
uint64_t hip_scratch_integer_scalar_rotate_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
    uint32_t message_modulus, uint32_t carry_modulus,
    enum SHIFT_OR_ROTATE_TYPE shift_type, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_scalar_rotate_64_inplace_async(CudaStreamsFFI streams,
                                                CudaRadixCiphertextFFI *lwe_array,
                                                uint32_t n, int8_t *mem_ptr,
                                                void *const *bsks, void *const *ksks);
void hip_cleanup_integer_scalar_rotate_64_inplace(CudaStreamsFFI streams,
                                                  int8_t **mem_ptr_void);
uint64_t hip_scratch_integer_shift_and_rotate_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
    uint32_t message_modulus, uint32_t carry_modulus,
    enum SHIFT_OR_ROTATE_TYPE shift_type, bool is_signed, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_shift_and_rotate_64_inplace_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
    CudaRadixCiphertextFFI const *lwe_shift, int8_t *mem_ptr, void *const *bsks,
    void *const *ksks);
void hip_cleanup_integer_shift_and_rotate_64_inplace(CudaStreamsFFI streams,
                                                     int8_t **mem_ptr_void);
uint64_t hip_integer_shift_and_rotate_pbs_count(int8_t *mem_ptr);
/* tests, benches: the fused rotate-and-pack kernel alone.  out[c rows + i] = s0 x[c rows + i] + s1 pick(i) + (ctrl ?
 * ctrl[c ctrl_stride + ctrl_row] : 0) on u64 words; pick(i) is row i - r (dir = 0) or i + r (dir = 1) of integer c, a row
 * outside the integer taken modulo rows (mode = 0), nothing (mode = 1) or pad[c pad_stride + pad_row] (mode = 2).
 * 0 <= r < rows; out must not overlap x. */
void hip_test_rotate_pack_async(void *stream, uint32_t gpu_index, void *out, void const *x, void const *pad,
                                void const *ctrl, uint64_t s0, uint64_t s1, uint32_t words, uint32_t rows, uint32_t batch,
                                uint32_t r, uint32_t dir, uint32_t mode, uint32_t pad_stride, uint32_t pad_row,
                                uint32_t ctrl_stride, uint32_t ctrl_row);
/* benches: the same rows for s0 = 1, composed from a device copy, block copies, a memset or single-row copies and two
 * axpy launches (what a barrel stage took before the kernel).  tmp: 2 * batch * rows rows of scratch; ctrl_idx: batch * rows
 * entries c * ctrl_stride + ctrl_row on the device (read when ctrl is given). */
void hip_test_rotate_pack_baseline_async(void *stream, uint32_t gpu_index, void *out, void const *x, void const *pad,
                                         void const *ctrl, void const *ctrl_idx, void *tmp, uint64_t s1, uint32_t words,
                                         uint32_t rows, uint32_t batch, uint32_t r, uint32_t dir, uint32_t mode,
                                         uint32_t pad_stride, uint32_t pad_row);

/* ------------------------------------------------------------------ Trivium transciphering (extensions)
 * cuda/include/trivium/trivium.h under hip_ names with the reference's parameter lists, on the shared scratch protocol;
 * the reference-named symbols remain link stubs.  num_inputs = N ciphers run side by side.  Position p of a register
 * occupies blocks p N .. p N + N - 1 (a: 93 positions, b: 84, c: 111); bit i of input n of the key / the IV is block
 * i N + n (80 N blocks each); the keystream bit of step t of input n is block t N + n.  Bits are 0 / 1 in the message
 * space.  init: a[i] = key[79 - i], b[i] = iv[79 - i] (i < 80), c[108 .. 110] = 1 (trivial encryptions), everything else 0,
 * then 1,152 steps without output; it writes all 288 N register blocks.  step: num_steps steps from the registers, which hold
 * the same layout before and after.  64 steps run in two bootstrap rounds: 384 N bootstraps without keystream, 512 N with
 * it; init is 6,912 N bootstraps in 36 rounds.  Registers and keystream leave a call with degree 1 and noise level 1.
 * Limits: a row reaches the value and noise level max(message_modulus + 1, 5), which must be at most
 * message_modulus * carry_modulus - 1 and at most (message_modulus * carry_modulus - 1) / (message_modulus - 1) — (2, 4),
 * (2, 8), (4, 4), (4, 16), (8, 8) pass, (2, 2) is refused; input blocks (key, IV, the registers of step) have degree and
 * noise level at most 1; num_steps is a multiple of 64; a, b, c hold 93 N, 84 N, 111 N blocks, key and iv 80 N, the
 * keystream num_steps N; num_inputs equals the scratch's; a scratch serves the call it was created for.
 * hip_trivium_pbs_count: bootstraps of one call on that scratch (init: the warm-up, num_steps is not read); every call
 * checks it against the rounds it issued. */
uint64_t hip_scratch_trivium_init_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
    uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t num_inputs);
void hip_trivium_init_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *a_reg,
    CudaRadixCiphertextFFI *b_reg, CudaRadixCiphertextFFI *c_reg,
    const CudaRadixCiphertextFFI *key, const CudaRadixCiphertextFFI *iv,
    uint32_t num_inputs, int8_t *mem_ptr, void *const *bsks, void *const *ksks);
void hip_cleanup_trivium_init(CudaStreamsFFI streams, int8_t **mem_ptr_void);
uint64_t hip_scratch_trivium_step_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
    uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t num_inputs);
void hip_trivium_step_async(CudaStreamsFFI streams,
                            CudaRadixCiphertextFFI *keystream_output,
                            CudaRadixCiphertextFFI *a_reg,
                            CudaRadixCiphertextFFI *b_reg,
                            CudaRadixCiphertextFFI *c_reg, uint32_t num_inputs,
                            uint32_t num_steps, int8_t *mem_ptr,
                            void *const *bsks, void *const *ksks);
void hip_cleanup_trivium_step(CudaStreamsFFI streams, int8_t **mem_ptr_void);
uint64_t hip_trivium_pbs_count(int8_t *mem_ptr, uint32_t num_steps);
/* tests: batches between two re-basings of the state tapes of that scratch, 2 .. 18 (18 when the scratch is created) */
void hip_test_trivium_set_window(int8_t *mem_ptr, uint32_t window);
/* tests, benches: the tap kernel alone.  out_g[q inputs + n] = sum over the terms t of group g of
 * scalar_t * src_t[(pos_t +- q) inputs + n] on u64 words, rows of `words` words, q < bits[g]; up to 4 groups of up to 5
 * terms.  HOST arrays: outs / bits / terms one entry per group; srcs / pos / backwards / scalars five per group (term t of
 * group g at 5 g + t); backwards[i] != 0: bit q reads position pos - q (pos >= bits - 1).  No output may overlap a row read. */
void hip_test_tap_sum_async(void *stream, uint32_t gpu_index, uint32_t words, uint32_t inputs, uint32_t groups,
                            void *const *outs, uint32_t const *bits, uint32_t const *terms, void const *const *srcs,
                            uint32_t const *pos, uint32_t const *backwards, uint64_t const *scalars);
/* benches: the data movement of one batch of 64 steps with keystream, composed from device copies and pairwise additions in
 * the reference's order (cuda/src/trivium/trivium.cuh:110-275).  a, b, c: the registers, updated in place; r1 / r2 stand for
 * the outputs of the two rounds, [and_a | and_b | and_c | t3] and [a | b | c | z] of 64 * inputs rows each; in1 / in2
 * receive the rows the two tap launches form; keystream receives r2's z rows in step order.
 * tmp: (111 + 12 * 64) * inputs rows. */
void hip_test_trivium_batch_baseline_async(void *stream, uint32_t gpu_index, void *a, void *b, void *c, void *in1,
                                           void const *r1, void *in2, void const *r2, void *keystream, void *tmp,
                                           uint32_t words, uint32_t inputs, uint64_t message_modulus);

/* ------------------------------------------------------------------ AES-128 transciphering (extensions)
 * cuda/include/aes/aes.h under hip_ names with the reference's parameter lists, on the shared scratch protocol; the
 * reference-named symbols remain link stubs (AES-256 too).  key / iv: 128 one-bit blocks, block i holds bit 127 - i (most
 * significant first); round_keys / expanded_keys: 11 x 128 blocks in the same order, round key r at blocks 128 r ..;
 * output: 128 * num_aes_inputs blocks, input n at blocks 128 n .. is AES_k((iv + start_counter + n) mod 2^128);
 * counter_bits_le_all_blocks: HOST array, entry 128 n + i is bit i (little endian) of start_counter + n.  Outputs have degree 1
 * and noise level 1.  sbox_parallelism (1, 2, 4, 8 or 16): state bytes per S-box pass; it bounds the scratch and changes the
 * number of rounds, never the result.  Classic and multi-bit keys; moduli with msg * carry >= 16 and
 * (msg * carry - 1) / (msg - 1) >= 5, the others are refused.  DESIGN.md 6m has the schedule.
 * hip_integer_aes_pbs_count / hip_integer_aes_rounds: bootstraps and round-driver rounds of one call on that scratch; every
 * call checks both against what it issued. */
uint64_t hip_scratch_integer_aes_ctr_encrypt_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
    uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t num_aes_inputs,
    uint32_t sbox_parallelism);
void hip_integer_aes_ctr_encrypt_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *output,
    CudaRadixCiphertextFFI const *iv, CudaRadixCiphertextFFI const *round_keys,
    const uint64_t *counter_bits_le_all_blocks, uint32_t num_aes_inputs,
    int8_t *mem_ptr, void *const *bsks, void *const *ksks);
void hip_cleanup_integer_aes_ctr_encrypt_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
uint64_t hip_scratch_integer_key_expansion_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
    uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_key_expansion_64_async(CudaStreamsFFI streams,
                                        CudaRadixCiphertextFFI *expanded_keys,
                                        CudaRadixCiphertextFFI const *key,
                                        int8_t *mem_ptr, void *const *bsks,
                                        void *const *ksks);
void hip_cleanup_integer_key_expansion_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
uint64_t hip_integer_aes_pbs_count(int8_t *mem_ptr);
uint64_t hip_integer_aes_rounds(int8_t *mem_ptr);
/* tests, benches: the gate-sum kernel alone on a caller-given program.
 * out[(g lanes + l) inputs + n] = sum over the terms t of group g of scalar_t * src_t[row0_t + lane_t(l) * lane_stride_t + (n,
 * or 0 for a broadcast term)] on u64 words, rows of `words` words, plus (constant_g + the group's clear terms) * delta on the
 * last word.  base: 0 wires, 1 caller_a, 2 caller_b, 3 clear (entry n * clear_stride + row0 of `clear`, times the scalar).
 * flags: 1 broadcast over inputs, 2 lane of the state: lane_t(l) = map(lane0 + l) with map = kind | parameter << 2, kind
 * 0 identity, 1 permutation `parameter` of `maps` (16 entries each), 2 offset `parameter` within the column of four lanes;
 * without flag 2 lane_t(l) = l.  Device pointers: out, wires, caller_a, caller_b, clear.  HOST arrays: group_* one entry per
 * group (the groups' terms follow each other in the term_* arrays), maps.  rows_*: the rows the three bases hold.  Refused: an
 * empty program, a lane map that leaves the state_lanes lanes or the base, an output that overlaps a row read. */
void hip_test_gate_sum_async(void *stream, uint32_t gpu_index, void *out, void const *wires, void const *caller_a,
                             void const *caller_b, void const *clear, uint32_t words, uint32_t inputs, uint32_t lanes,
                             uint32_t lane0, uint32_t state_lanes, uint32_t clear_stride, uint64_t delta, uint32_t groups,
                             uint64_t const *group_constant, uint32_t const *group_terms, uint64_t const *term_scalar,
                             uint32_t const *term_row0, uint32_t const *term_lane_stride, uint32_t const *term_map,
                             uint32_t const *term_base, uint32_t const *term_flags, uint32_t num_maps, uint32_t const *maps,
                             uint64_t rows_wires, uint64_t rows_a, uint64_t rows_b);
/* tests: one S-box pass on a cipher scratch's first sbox_parallelism lanes.  in / out: device rows [wire j][lane][input], j = 0
 * the most significant bit of a byte, sbox_parallelism * num_aes_inputs rows per wire. */
void hip_test_aes_sbox_async(CudaStreamsFFI streams, void *out, void const *in, int8_t *mem_ptr, void *const *bsks,
                             void *const *ksks);
/* tests: parts of a call on a cipher scratch.  r0 = 0: the counter addition (it folds round key 0 in) from iv, round_keys and
 * the counter bits; r0 >= 1: the state is loaded from `state`.  Then the cipher rounds max(r0, 1) .. r1 (r0 <= r1 <= 10).
 * state: device rows [wire j][byte lane][input], 16 * num_aes_inputs rows per wire; it receives the state after the last
 * round run, unless that is round 10, which writes `output` in the caller's layout. */
void hip_test_aes_rounds_async(CudaStreamsFFI streams, void *state, CudaRadixCiphertextFFI *output,
                               CudaRadixCiphertextFFI const *iv, CudaRadixCiphertextFFI const *round_keys,
                               const uint64_t *counter_bits_le_all_blocks, uint32_t r0, uint32_t r1, int8_t *mem_ptr,
                               void *const *bsks, void *const *ksks);
/* tests: the scheduled program of an AES scratch as u64 words in HOST memory; returns the words it takes and writes them when
 * `capacity` holds them.  Every item is one word:
 *   header   0x41455350, message modulus, carry modulus, inputs, sbox_parallelism, key schedule (0 / 1), cipher rounds,
 *            tables T, entries per table E = msg * carry, permutations M, segments G, rows of the wires,
 *            first rows of the state wires x[0 .. 7] (0 for a key schedule), first rows of the S-box outputs sb[0 .. 7]
 *   tables   T * E entries, then M * 16 permutation entries
 *   segment  lanes, passes, rounds; per round: rows, to_caller (0: the round writes wires, 1: the caller's output);
 *            per row: table, constant (units of delta), terms, destination row0, lane_stride, in_stride, state_lane
 *            (row = row0 + (state_lane ? pass * lanes + l : l) * lane_stride + n * in_stride);
 *            per term: base, row0, lane_stride, map, flags, scalar (as for hip_test_gate_sum_async)
 * Segments of a cipher scratch: counter addition, S-box (run `passes` times per cipher round), linear layer of a middle
 * round (caller_a: that round's key), of the last round; of a key schedule: S-box, then the linear layer of steps 1 .. 10
 * (caller_a: the previous round key). */
uint64_t hip_test_aes_program(int8_t *mem_ptr, uint64_t *words, uint64_t capacity);
/* benches: the gate-sum launches of one middle cipher round of a cipher scratch (every S-box pass, then the linear layer with
 * the round key read from the 128 device rows of `round_key`), without the bootstraps between them. */
void hip_test_aes_round_launches_async(CudaStreamsFFI streams, void const *round_key, int8_t *mem_ptr);
/* benches: the data movement of one middle cipher round composed from device copies and pairwise additions in the reference's
 * order (cuda/src/aes/aes.cuh:882-974), without the bootstraps.  state: 128 * inputs rows [block][input], key: 128 rows,
 * tmp: 512 * inputs rows. */
void hip_test_aes_round_baseline_async(void *stream, uint32_t gpu_index, void *state, void const *key, void *tmp,
                                       uint32_t words, uint32_t inputs);

/* ------------------------------------------------------------------ division with remainder, absolute value (extensions)
 * cuda/include/integer/integer.h:465-499 under hip_ names with the reference's parameter lists, on the shared scratch
 * protocol; the reference-named symbols remain link stubs.  A call takes a batch of integers ([integer][block], num_blocks
 * blocks each, capacity from hip_integer_scratch_batch); every round covers the whole batch.  Two's complement operands when
 * is_signed.  Bit-by-bit restoring division (tfhe-rs unsigned_unchecked_div_rem_parallelized): the divisor's masks and
 * "a bit above position s is set" flags once per call, then per bit one shift round, the cleaning of the merged remainder,
 * the overflowing subtraction on the carry tree and one select round; three launches of one kernel form their inputs, no
 * host synchronisation, upload or row copy inside the loop.
 * Unsigned division by zero: quotient all ones, remainder = numerator.  Signed: truncation towards zero, the remainder has
 * the numerator's sign, MIN / -1 wraps to MIN with remainder 0; x / 0 = 1 for x < 0 and -1 for x >= 0, remainder x.
 * Outputs leave with degree message_modulus - 1 and noise level 1.
 * Limits (refused at scratch time): message_modulus 4, 8 or 16; 3 (message_modulus - 1) + 2 <= message_modulus *
 * carry_modulus - 1; noise levels 5 and message_modulus + 1 at most (message_modulus * carry_modulus - 1) /
 * (message_modulus - 1); what carry propagation accepts — (4, 4), (4, 16), (8, 8) pass, (2, 2) is refused.  Operand blocks
 * have degree at most message_modulus - 1; the four operands hold the same number of blocks with the key's lwe dimension; no
 * output overlaps an input or the other output; is_signed equals the scratch's.
 * hip_integer_div_rem_pbs_count: bootstraps of one division (per pair of a batch); every call checks it against the rounds
 * it issued.  abs: (x + mask) ^ mask with the sign mask as one row per integer, 1 + propagation + num_blocks bootstraps;
 * nothing is launched when !is_signed. */
uint64_t hip_scratch_integer_div_rem_64_async(
    CudaStreamsFFI streams, bool is_signed, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_div_rem_64_async(CudaStreamsFFI streams,
                                  CudaRadixCiphertextFFI *quotient,
                                  CudaRadixCiphertextFFI *remainder,
                                  CudaRadixCiphertextFFI const *numerator,
                                  CudaRadixCiphertextFFI const *divisor,
                                  bool is_signed, int8_t *mem_ptr,
                                  void *const *bsks, void *const *ksks);
void hip_cleanup_integer_div_rem_64(CudaStreamsFFI streams,
                                    int8_t **mem_ptr_void);
uint64_t hip_scratch_integer_abs_inplace_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, bool is_signed,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_abs_inplace_64_async(CudaStreamsFFI streams,
                                      CudaRadixCiphertextFFI *ct,
                                      int8_t *mem_ptr, bool is_signed,
                                      void *const *bsks, void *const *ksks);
void hip_cleanup_integer_abs_inplace_64(CudaStreamsFFI streams,
                                        int8_t **mem_ptr_void);
uint64_t hip_integer_div_rem_pbs_count(bool is_signed, uint32_t num_blocks, uint32_t message_modulus,
                                       uint32_t carry_modulus);
/* tests, benches: the stage kernel alone.  out_g[c][first_out + r] = constant_g on the body word + sum over the terms t of
 * group g of scalar_t * row_t(c, j), j = first_g + r, on u64 words, rows of `words` words; a term reads row j * step + offset
 * of its array (step 1, or 0: one row for every j), below row 0 its stand-in row (or nothing: null); arrays hold their
 * integers `stride` rows apart and `extent` rows each.  Up to 4 groups of up to 4 terms.  HOST arrays: outs / constants one
 * entry per group, group_u32 six (stride, extent, first_out, first, rows, terms); srcs / stands / scalars four per group
 * (term t of group g at 4 g + t), term_u32 six per term (stride, extent, offset as int32, step, stand_stride, stand_row).
 * Refused: an output that overlaps a row read or another output, a row outside its array, more groups or terms. */
void hip_test_divrem_sum_async(void *stream, uint32_t gpu_index, uint32_t words, uint32_t integers, uint32_t groups,
                               void *const *outs, uint64_t const *constants, uint32_t const *group_u32,
                               void const *const *srcs, void const *const *stands, uint64_t const *scalars,
                               uint32_t const *term_u32);
/* benches: stage 1, 2 or 3 of iteration s of the division loop composed from device copies, memsets and pairwise additions
 * in the reference's order (cuda/src/integer/div_rem.cuh:589-870).  Arrays hold their integers num_blocks rows apart (fl,
 * up: one row per integer).  Stage 1 reads r1, r2, num and writes in1; stage 2 reads s1, s2, negd, neglow (this iteration's
 * low part, null when the top block is whole), consts (num_blocks trivial rows of message_modulus - 1) and writes in2 and v;
 * stage 3 reads cl, v, fl, up (null in the last iteration), one (a trivial 1), zero_idx (num_blocks zeros on the device) and
 * writes in3.  tmp: 2 num_blocks + 1 rows. */
void hip_test_divrem_iteration_baseline_async(void *stream, uint32_t gpu_index, void const *r1, void const *r2,
                                              void const *num, void const *s1, void const *s2, void const *negd,
                                              void const *neglow, void const *cl, void *v, void const *fl, void const *up,
                                              void const *consts, void const *one, void const *zero_idx, void *in1, void *in2,
                                              void *in3, void *tmp, uint32_t words, uint32_t num_blocks, uint32_t batch,
                                              uint32_t s, uint32_t bits, uint64_t message_modulus, uint32_t stage);

/* ------------------------------------------------------------------ bit counts: runs, ilog2, popcounts (extensions)
 * cuda/include/integer/integer.h:648-662 and :701-718 under hip_ names with the reference's parameter lists, on the shared
 * scratch protocol; the reference-named symbols remain link stubs.  hip_*_count_ones_64 is our own (the reference's GPU
 * backend has no popcount entry point): bit_value One counts the ones, Zero the zeros.  Out of place.  A call takes a batch
 * of integers ([integer][block], num_blocks blocks each, capacity from hip_integer_scratch_batch) and writes
 * counter_num_blocks blocks per integer; a signed operand is counted on its two's complement bits as they stand.
 * With b = log2(message_modulus), B = b * num_blocks: counter_num_blocks = ceil((floor(log2 B) + 1) / b) for the runs and
 * the popcounts, ceil((floor(log2(B - 1)) + 2) / b) for ilog2; another value is refused at scratch time.
 * Runs: ceil(log2 num_blocks) scan rounds (the first reads the operand's blocks in place, bivariate: "my run if my neighbour
 * is a full run"), then the sum of num_blocks single-block terms and one carry propagation.  ilog2 = sum (b - t_i) - 1 on the
 * scan of the leading zeros: no round more; ilog2(0) is all ones.  Popcounts: one round over the pairs of blocks.
 * hip_integer_ilog2_64_async keeps the three trivial operands of the reference's parameter list: they must not be null and
 * trivial_ct_neg_n must hold counter_num_blocks blocks, as the reference checks; they are otherwise NOT read.
 * Outputs leave with degree message_modulus - 1 and noise level 1.
 * Refused at scratch time: message_modulus below 3 or fewer than 16 values per block (the carry propagation), a
 * message_modulus that is not a power of two.  Refused by a call: an operand block of degree above message_modulus - 1, an
 * output that overlaps the input, more integers than the scratch holds, a scratch of another kind.
 * hip_integer_bit_count_pbs_count / _rounds: bootstraps per integer and rounds of one call, kind 0 a run, 1 ilog2, 2 a
 * popcount; functions of their four arguments; every call checks the bootstraps it issued against the first. */
uint64_t hip_scratch_integer_count_of_consecutive_bits_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
    uint32_t counter_num_blocks, uint32_t message_modulus,
    uint32_t carry_modulus, enum Direction direction, enum BitValue bit_value,
    bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_count_of_consecutive_bits_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_ct,
    CudaRadixCiphertextFFI const *input_ct, int8_t *mem_ptr, void *const *bsks,
    void *const *ksks);
void hip_cleanup_integer_count_of_consecutive_bits_64(CudaStreamsFFI streams,
                                                      int8_t **mem_ptr_void);
uint64_t hip_scratch_integer_ilog2_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
    uint32_t carry_modulus, uint32_t input_num_blocks,
    uint32_t counter_num_blocks, uint32_t num_bits_in_ciphertext,
    bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_ilog2_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_ct,
    CudaRadixCiphertextFFI const *input_ct,
    CudaRadixCiphertextFFI const *trivial_ct_neg_n,
    CudaRadixCiphertextFFI const *trivial_ct_2,
    CudaRadixCiphertextFFI const *trivial_ct_m_minus_1_block, int8_t *mem_ptr,
    void *const *bsks, void *const *ksks);
void hip_cleanup_integer_ilog2_64(CudaStreamsFFI streams,
                                  int8_t **mem_ptr_void);
uint64_t hip_scratch_integer_count_ones_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr,
    CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
    uint32_t counter_num_blocks, uint32_t message_modulus,
    uint32_t carry_modulus, enum BitValue bit_value, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_count_ones_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_ct,
    CudaRadixCiphertextFFI const *input_ct, int8_t *mem_ptr, void *const *bsks,
    void *const *ksks);
void hip_cleanup_integer_count_ones_64(CudaStreamsFFI streams,
                                       int8_t **mem_ptr_void);
uint64_t hip_integer_bit_count_pbs_count(uint32_t kind, uint32_t num_blocks, uint32_t message_modulus,
                                         uint32_t carry_modulus);
uint32_t hip_integer_bit_count_rounds(uint32_t kind, uint32_t num_blocks, uint32_t message_modulus,
                                      uint32_t carry_modulus);
/* tests, benches: the pack kernel alone.  out[c][g] = s0 * x[c * x_stride + first + g * step] + s1 * x[c * x_stride + first +
 * g * step + delta] on u64 words, rows of `words` words, g < ceil(rows / step); a partner g * step + delta outside
 * 0 .. rows - 1 contributes nothing.  out is dense.  Refused: a null or empty operand, delta == 0 or |delta| >= rows, a step
 * other than 1 or 2, an output that overlaps the rows read, more than 65,535 integers. */
void hip_test_pair_pack_async(void *stream, uint32_t gpu_index, void *out, void const *x, uint64_t s0, uint64_t s1,
                              uint32_t words, uint32_t batch, uint32_t x_stride, uint32_t first, uint32_t rows,
                              uint32_t step, int delta);
/* benches: the same rows for s0 = 1, step = 1, first = 0, x_stride = rows composed per integer from a device copy and a
 * memset into tmp (batch * rows rows), then one pairwise addition that packs. */
void hip_test_pair_pack_baseline_async(void *stream, uint32_t gpu_index, void *out, void const *x, void *tmp, uint64_t s1,
                                       uint32_t words, uint32_t batch, uint32_t rows, int delta);

/* ------------------------------------------------------------------ 128-bit PBS and noise squashing (extensions)
 * The programmable bootstrap over the 128-bit torus that noise squashing runs on (fft128_pbs.rs; the reference's
 * cuda/include/pbs/programmable_bootstrap.h:57-60,68-72,92-97,102-103 and cuda/include/fft/fft128.h), under hip_ names
 * with the reference's parameter lists.  The reference-named *_128 / *_f128 symbols remain link stubs.
 *
 * Key: src is the standard-domain u128 key on the HOST in the reference's container order
 * [input_lwe_dim][level][glwe_dim + 1][glwe_dim + 1][polynomial_size]; dest takes 32 * polynomial_size / 2 bytes per
 * polynomial (four planes of doubles: re_hi, re_lo, im_hi, im_lo), i.e. as many bytes as the source.
 * Bootstrap: lwe_array_in holds num_samples contiguous u64 LWEs of dimension lwe_dimension, lut_vector ONE u128 GLWE,
 * lwe_array_out receives num_samples contiguous u128 LWEs of dimension glwe_dimension * polynomial_size.  One launch,
 * one workgroup per input, no synchronisation between workgroups.  polynomial_size 256 .. 4096 (glwe_dimension up to 3
 * below 2048, 2 at 2048, 1 at 4096), base_log <= 64, base_log * level_count <= 128.
 * Panics: an unsupported size, an invalid decomposition, a scratch of another kind or other sizes, more samples than
 * the scratch holds, a key that hip_convert_lwe_programmable_bootstrap_key_128_async converted for other sizes. */
void hip_convert_lwe_programmable_bootstrap_key_128_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src, uint32_t input_lwe_dim, uint32_t glwe_dim,
    uint32_t level_count, uint32_t polynomial_size);
uint64_t hip_scratch_programmable_bootstrap_128_async(
    void *stream, uint32_t gpu_index, int8_t **buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t level_count, uint32_t input_lwe_ciphertext_count, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_programmable_bootstrap_128_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out, void const *lut_vector, void const *lwe_array_in,
    void const *bootstrapping_key, int8_t *buffer, uint32_t lwe_dimension, uint32_t glwe_dimension,
    uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t num_samples);
void hip_cleanup_programmable_bootstrap_128(void *stream, uint32_t gpu_index, int8_t **pbs_buffer);
/* The negacyclic f128 transform of number_of_samples polynomials of N u128 coefficients: planes re0 (high doubles of the
 * real parts), re1 (low), im0, im1 of N / 2 doubles per polynomial, in this library's transform order.
 * "as torus": words read as signed, scaled by 2^-128; "as integer": unscaled; backward: normalised, reduced modulo 1. */
void hip_fourier_transform_forward_as_torus_f128_async(
    void *stream, uint32_t gpu_index, void *re0, void *re1, void *im0, void *im1, void const *standard, uint32_t const N,
    const uint32_t number_of_samples);
void hip_fourier_transform_forward_as_integer_f128_async(
    void *stream, uint32_t gpu_index, void *re0, void *re1, void *im0, void *im1, void const *standard, uint32_t const N,
    const uint32_t number_of_samples);
void hip_fourier_transform_backward_as_torus_f128_async(
    void *stream, uint32_t gpu_index, void *standard, void const *re0, void const *re1, void const *im0, void const *im1,
    uint32_t const N, const uint32_t number_of_samples);
/* Noise squashing of a radix ciphertext (integer.cuh:2776-2840): the ceil(blocks / 2) output blocks are u128 LWEs under
 * the squashing key's output key; block i is  in[2i] + message_modulus * in[2i + 1]  (clean inputs), keyswitched with
 * ksks[0] and bootstrapped with the 128-bit key bsks[0] and the identity table (delta = 2^127 / (message_modulus *
 * carry_modulus)).  lwe_dimension: the small key's; glwe_dimension x polynomial_size: the squashing ring; input_*: the
 * compute ring; num_radix_blocks: OUTPUT blocks; num_original_blocks: input blocks.  One GPU (entry 0 of `streams`).
 * Panics: an output block count other than ceil(input / 2), a block with a carry, other lwe dimensions. */
uint64_t hip_scratch_integer_apply_noise_squashing_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
    uint32_t input_glwe_dimension, uint32_t input_polynomial_size, uint32_t ks_level, uint32_t ks_base_log,
    uint32_t pbs_level, uint32_t pbs_base_log, uint32_t num_radix_blocks, uint32_t num_original_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type);
void hip_integer_apply_noise_squashing_64_async(
    CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out, CudaRadixCiphertextFFI const *lwe_array_in,
    int8_t *mem_ptr, void *const *ksks, void *const *bsks);
void hip_cleanup_integer_apply_noise_squashing_64(CudaStreamsFFI streams, int8_t **mem_ptr_void);
/* The multi-bit programmable bootstrap over the 128-bit torus (std_multi_bit_f128_deterministic_blind_rotate_assign; the
 * reference's cuda/include/pbs/programmable_bootstrap_multibit.h:18-21,64-80), under hip_ names with the reference's
 * parameter lists.  The reference-named *_multi_bit_*_128 symbols remain link stubs.
 *
 * Key: src is the standard-domain u128 key on the HOST in the reference's container order [input_lwe_dim /
 * grouping_factor][2^grouping_factor][level, index 0 = last level][glwe_dim + 1][glwe_dim + 1][polynomial_size]; dest takes
 * as many bytes and keeps that form: the key bundles are summed exactly modulo 2^128 and transformed afterwards.
 * Bootstrap: sample s reads the u64 LWE lwe_input_indexes[s] of lwe_array_in and writes the u128 LWE lwe_output_indexes[s]
 * of lwe_array_out; lut_vector is ONE u128 GLWE.  Plain modulus switch, groups in ascending order.  Per chunk of groups one
 * key-bundle launch and one accumulate launch on `stream`; the scratch fixes the chunk (the largest number of groups whose
 * bundles fit 512 MiB for its sample count).  Sizes as for hip_programmable_bootstrap_128_async; grouping_factor 2..4
 * dividing lwe_dimension; num_many_lut must be 1.
 * Panics: a grouping factor outside 2..4 or not dividing lwe_dimension, an unsupported size, an invalid decomposition, a
 * scratch of another kind or other sizes, more samples than the scratch holds, a key converted for other sizes or another
 * grouping factor, a classic 128-bit key (and a multi-bit key given to hip_programmable_bootstrap_128_async). */
void hip_convert_lwe_multi_bit_programmable_bootstrap_key_128_async(
    void *stream, uint32_t gpu_index, void *dest, void const *src, uint32_t input_lwe_dim, uint32_t glwe_dim,
    uint32_t level_count, uint32_t polynomial_size, uint32_t grouping_factor);
uint64_t hip_scratch_multi_bit_programmable_bootstrap_128_async(
    void *stream, uint32_t gpu_index, int8_t **buffer, uint32_t glwe_dimension, uint32_t polynomial_size,
    uint32_t level_count, uint32_t input_lwe_ciphertext_count, bool allocate_gpu_memory);
void hip_multi_bit_programmable_bootstrap_128_async(
    void *stream, uint32_t gpu_index, void *lwe_array_out, void const *lwe_output_indexes, void const *lut_vector,
    void const *lwe_array_in, void const *lwe_input_indexes, void const *bootstrapping_key, int8_t *mem_ptr,
    uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t grouping_factor, uint32_t base_log,
    uint32_t level_count, uint32_t num_samples, uint32_t num_many_lut, uint32_t lut_stride);
void hip_cleanup_multi_bit_programmable_bootstrap_128(void *stream, const uint32_t gpu_index, int8_t **buffer);
/* Noise squashing with a multi-bit 128-bit key: hip_scratch_integer_apply_noise_squashing_64_async's parameter list plus
 * grouping_factor.  The scratch remembers its kind: hip_integer_apply_noise_squashing_64_async and
 * hip_cleanup_integer_apply_noise_squashing_64 serve both.  Multi-bit takes the plain modulus switch: a non-zero
 * noise_reduction_type panics. */
uint64_t hip_scratch_integer_apply_noise_squashing_multi_bit_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
    uint32_t input_glwe_dimension, uint32_t input_polynomial_size, uint32_t ks_level, uint32_t ks_base_log,
    uint32_t pbs_level, uint32_t pbs_base_log, uint32_t num_radix_blocks, uint32_t num_original_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t grouping_factor);
/* test hooks of the multi-bit 128-bit path: groups per pass for scratches created afterwards (0: automatic); the
 * Fourier-domain key bundle of one group for the LWE lwe_input_indexes[0] of lwe_array_in, (glwe_dimension + 1)^2 *
 * level_count polynomials of four planes of polynomial_size / 2 doubles */
void hip_backend_set_pbs128_multibit_chunk(uint32_t groups);
void hip_test_pbs128_multibit_keybundle_async(
    void *stream, uint32_t gpu_index, void *bundle_out, void const *bootstrapping_key, void const *lwe_array_in,
    void const *lwe_input_indexes, uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
    uint32_t level_count, uint32_t grouping_factor, uint32_t group);
/* test hooks of the 128-bit path: the host-built double-double tables (four doubles per entry: re_hi, re_lo, im_hi,
 * im_lo; polynomial_size / 2 entries per table, indexed like hip_test_fft_tables_host's); the u128 signed decomposer
 * (level_count digits per word, least significant first, as i128); the kernels' own complex f128 product of `count`
 * points (each operand: four planes of count doubles) */
void hip_test_fft128_tables_host(uint32_t polynomial_size, double *fwd, double *inv, double *untwist);
void hip_test_decompose_128_async(void *stream, uint32_t gpu_index, void const *in, void *out, uint32_t count,
                                  uint32_t base_log, uint32_t level_count);
void hip_test_f128_cmul_async(void *stream, uint32_t gpu_index, void *out, void const *a, void const *b, uint32_t count);

/* Select which f64 kernel serves cuda_programmable_bootstrap_64_async (all give identical bits):
 * 0 = automatic (N=2048,k=1: latency kernel up to 256 LWEs, throughput kernel beyond; N=1024,k<=2: its
 *     throughput kernel; generic otherwise),
 * 1 = generic LDS kernel, 2 = throughput (wave) kernel of the parameter set, 3 = latency (block) kernel, 4 = its dual-stream
 * variant; 2..4 abort on unsupported parameter sets.  For the multi-bit entry point 2 selects the
 * multi-bit mode of the throughput kernel, 1 the generic multi-bit kernel, 5 the two-launch latency path (all
 * keybundles first, one workgroup per polynomial; then the products, for N=2048,k=1 on the latency kernel) that 0
 * takes up to 128 LWEs (256 for N = 2048, k = 1), 6 the same path with the products on the generic kernels (comparison), 7 the throughput
 * kernel without the sharing of key loads between the two LWEs of a quad of waves, 8 the throughput kernel with
 * sharing among quads only, not among all eight waves of a full workgroup of a one-level set (both: comparison). */
void hip_backend_set_fft_kernel(uint32_t which);
/* The stream-ordered arena behind cuda_malloc_async / cuda_drop (tfhe_rs_amd/csrc/arena.hip; the reference's device pool,
 * tfhe-cuda-common/cuda/src/device.cu:70-120,176-226).  trim: every idle cached block goes back to the runtime, returns the
 * bytes released (the reference's pool keeps a release threshold instead).  stats: out7 = allocations, re-uses, blocks taken
 * from the runtime, drops, re-uses that made the new stream wait for the old one's event, live bytes, cached bytes. */
uint64_t hip_backend_trim_allocator(uint32_t gpu_index);
void hip_backend_allocator_stats(uint32_t gpu_index, uint64_t *out7);
/* Debug mode TFHE_HIP_ARENA_REDZONE=1 (environment, read once): every device block of the library and of cuda_malloc[_async]
 * sits in a shared slab between two 4 KiB canaries that are checked when it is dropped, a dropped payload is poisoned and
 * checked when it is handed out again; a finding aborts with the block, its owner and the offset (the memcheck the
 * reference runs over its GPU tests, scripts/check_memory_errors.sh:1-60).  Returns the canary checks made so far
 * (0: the mode is off). */
uint64_t hip_backend_redzone_checks(uint32_t gpu_index);
/* TFHE_HIP_PROFILE=1 (environment, read once): the radix layer brackets its rounds with roctx ranges — "apply lut round",
 * "keyswitch", "bootstrap", "scatter ... to gpu", "gather ... from gpu", "carry propagation", "integer mul", "block products",
 * "column sums" — for rocprofv3 --marker-trace (the reference's NVTX ranges, tfhe-cuda-common/cuda/include/helper_profile.cuh,
 * cuda/src/integer/integer.cuh:874,958,981).  Returns the ranges pushed so far (0: off). */
uint64_t hip_backend_profile_ranges(void);
/* test hook: cap of the groups the multi-bit latency path processes per pass (0 = what the scratch holds) */
void hip_backend_set_multibit_latency_groups(uint32_t groups);
/* keyswitch kernel: 0 = automatic (int8 matrix-core GEMM, any batch size, when level <= 16 (padded to a power of
 * two), base_log <= 6 and n_in*padded level is a multiple of 32 — one launch up to 768 LWEs (K shared by the waves of
 * a workgroup and by up to 8 workgroups per column tile), from 769 on a digit pass followed by an LDS-staged GEMM;
 * scalar kernels otherwise), 1 = scalar kernels only, 2 = the one-launch matrix-core kernel at every batch size, 3 = the
 * digit pass + GEMM from 129 LWEs on (tests).  Identical bits in all four. */
void hip_backend_set_keyswitch_kernel(uint32_t which);
/* generic kernels (f64 and NTT engines): 0 = one thread group per GLWE polynomial (default), 1 = single-group
 * kernels. Same bits. */
void hip_backend_set_ntt_kernel(uint32_t which);
/* last launched PBS kernel, for tests: 1 generic f64, 2 wave f64, 3 generic ntt, 4 generic multi-bit,
 * 5 exact, 6 wave multi-bit, 7 block (latency), 8 block dual-stream, 9 wave f64 for N = 1024,
 * 10 multi-bit latency path, 11 reference-order f64 engine, 12 NTT engine in its two-prime FP64 form */
uint32_t hip_backend_last_pbs_kernel(void);
/* the template instantiation the last PBS launch took, for tests: out[0] the kernel id above, out[1] template level
 * count L, out[2] template base_log B (0, 0: the run-time decomposition form), out[3] template grouping factor G (0:
 * classic or run-time), out[4] mode (0 plain, 1 SHARE, 2 OCTET, 3 LIMBS, 4 single-level digit path, 5 one group per
 * polynomial, 6 accumulator in device memory, 7 / 8 multi-bit products on the block kernel with the keybundles in slot /
 * position order), out[5] LWEs per workgroup, out[6] the kernel's N, out[7] its k + 1.  A call with two launches reports
 * the one that runs the external products. */
void hip_backend_last_pbs_instantiation(uint32_t *out8);
/* last 64-bit keyswitch, for tests: 0 scalar kernels, 1 one-launch matrix-core kernel, 2 digit pass + staged GEMM,
 * 3 staged GEMM on the digits the previous bootstrap emitted */
uint32_t hip_backend_last_keyswitch_path(void);
/* small-batch keyswitch (<= 32 LWEs): workgroups per column tile that share the K dimension (default 8; 1 = one
 * workgroup per column tile, no atomics).  Identical bits. */
void hip_backend_set_keyswitch_kparts(uint32_t parts);
/* the kernel form the last keyswitch (64- or 32-bit key) launched, for tests: out[0] the path above (the 64->32 entry point
 * records it too), out[1] the scalar kernel (1 small-base, 2 int32 digits, 3 int64 digits, 4 the 64->32 kernel; 0 on the
 * matrix-core paths), out[2] the compile-time level count of the one-launch or the digit kernel (1, 2, 4, 8, 16; 0: neither
 * ran), out[3] 1 when that form pads the level count, out[4] the key width in bits, out[5] the one-launch kernel's split of
 * K over the waves of a workgroup (4 or 1; 0: it did not run), out[6] the workgroups per column tile it ran with,
 * out[7] the GEMM's steps per barrier (1, 2, 4; 0: no GEMM ran) + 256 * the column tiles of the matrix-core launch */
void hip_backend_last_keyswitch_instantiation(uint32_t *out8);
/* keys whose matrix-core layout is cached at the moment (at most 32: the least recently used one goes), for tests */
uint32_t hip_backend_keyswitch_cache_entries(void);
const char *hip_backend_version(void);

/* HIP events recorded on a backend stream (used by bench.py to time launches) */
void *hip_event_create(void);
void hip_event_record(void *event, void *stream);
float hip_event_elapsed_ms(void *start, void *stop); /* synchronises `stop` */
void hip_event_destroy(void *event);

/* test hooks: run single device functions / transforms so that tests can compare them with
 * the oracle (ops documented in tfhe_rs_amd/csrc/testhooks.hip) */
void hip_test_arith_async(void *stream, uint32_t gpu_index, uint32_t op, void const *in,
                          void *out, uint32_t count, uint32_t p0, uint32_t p1);
void hip_test_transform_async(void *stream, uint32_t gpu_index, uint32_t op,
                              uint32_t polynomial_size, void const *in, void *out);
void hip_test_fft_tables_host(uint32_t polynomial_size, double *fwd, double *inv, double *untwist);
void hip_test_monomial_table_host(uint32_t polynomial_size, double *mono /* 4 * polynomial_size doubles */);

#ifdef __cplusplus
}
#endif
#endif /* TFHE_HIP_BACKEND_H */
