// pks128.h — launchers of pks128_kernels.h: the packing keyswitch over the 128-bit torus (squashed-noise ciphertext lists), its
// rotate / sum / modulus switch / bit-pack epilogue, and the unpack (+ sample extract) of the packed lists.
// A u128 word is two u64 words (lo, hi); buffers cross this boundary as uint64_t pointers.
#pragma once
#include "hx.h"

namespace tfhe_hip {

// ---- which kernel computes the decomposed products (hip_backend_set_pks128_kernel / hip_backend_last_pks128_path)
enum Pks128Kernel : uint32_t { kPks128Auto = 0, kPks128General = 1, kPks128Matrix = 2 };
void pks128_set_kernel(uint32_t which);
uint32_t pks128_last_path();  // 0: general (vector ALU) kernel, 1: matrix-core kernel
// K is split over up to 8 partial row sets for small batches; a cap (0: none) and the count the last call took
void pks128_set_max_parts(uint32_t parts);
uint32_t pks128_last_parts();

// The matrix-core kernel carries a shape exactly when every digit fits J <= 8 balanced bytes, K = n_in * level is a whole
// number of 32-deep steps and an int32 diagonal cannot overflow (J * K * 2^14 < 2^31).  Returns J, or 0: declined.
uint32_t pks128_matrix_digit_bytes(uint32_t n_in, uint32_t base_log, uint32_t level);
// bytes of the byte-plane layout of a key (0 where the matrix-core kernel declines the shape)
uint64_t pks128_planes_bytes(uint32_t n_in, uint32_t ncols, uint32_t base_log, uint32_t level);
// key [n_in][level][ncols] u128 -> planes [K / 32][ceil(ncols / 32)][16][64 lanes][16 bytes], bytes re-centred by -128
void launch_pks128_convert_key(hipStream_t st, void *planes, const uint64_t *key, uint32_t n_in, uint32_t ncols,
                               uint32_t level);

// what one call needs besides its operands; sized by pks128_workspace_* for the largest batch the scratch admits
struct Pks128Workspace {
  uint64_t *rows = nullptr;    // [parts][num_lwes][ncols] u128: the decomposed products, K split over `parts`
  void *digits = nullptr;      // matrix-core kernel: the A operands (digit bytes in the instruction's layout)
  uint64_t *digit_sums = nullptr;  // matrix-core kernel: sum over K of the digits of every LWE, u128
};
uint64_t pks128_rows_bytes(uint32_t cap, uint32_t n_in, uint32_t ncols, uint32_t base_log, uint32_t level);
uint64_t pks128_digits_bytes(uint32_t cap, uint32_t n_in, uint32_t base_log, uint32_t level);

// num_lwes u128 LWEs of dimension n_in in chunks of lwe_per_glwe -> ceil(num_lwes / lwe_per_glwe) GLWEs.
// planes: the key's byte-plane layout or nullptr (then the general kernel runs whatever is selected).
// storage_log_modulus 0: `out` receives the GLWEs as they are ((k+1)*N u128 words each); 1..128: their first
// k*N + lwe_per_glwe values switched to that many bits and bit-packed, ceil(that * bits / 128) u128 words each.
void launch_packing_keyswitch128(hipStream_t st, uint64_t *out, const Pks128Workspace &ws, const uint64_t *lwe_in,
                                 const uint64_t *key, const void *planes, uint32_t n_in, uint32_t glwe_dim, uint32_t N,
                                 uint32_t base_log, uint32_t level, uint32_t num_lwes, uint32_t lwe_per_glwe,
                                 uint32_t storage_log_modulus);

// u128 words of one packed GLWE
uint32_t pks128_words_per_glwe(uint32_t glwe_dim, uint32_t N, uint32_t lwe_per_glwe, uint32_t bits);
// the LWEs (dimension k*N, u128) at `indexes` (device array) of a packed list
void launch_unpack_extract128(hipStream_t st, uint64_t *lwe_out, const uint64_t *packed, const uint32_t *indexes,
                              uint32_t count, uint32_t glwe_dim, uint32_t N, uint32_t lwe_per_glwe, uint32_t bits);
// one packed GLWE as (k+1)*N u128 words: k*N mask values and `bodies` body values, the tail zero
void launch_unpack_glwe128(hipStream_t st, uint64_t *glwe_out, const uint64_t *words, uint32_t glwe_dim, uint32_t N,
                           uint32_t bodies, uint32_t bits);

}  // namespace tfhe_hip
