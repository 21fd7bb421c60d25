// ciphertext.hip — stand-alone modulus switch / sample extraction helpers of the boundary
// (backends/tfhe-cuda-backend/cuda/include/ciphertext.h; used by tests and by callers that
// run the PBS stages separately).
#include "kernels.h"

namespace tfhe_hip {

// cc/fft_impl/common.rs:10-23 applied element-wise (cuda/src/crypto/torus.cuh:133-147)
__global__ void modulus_switch_kernel(uint64_t *out, const uint64_t *in, uint32_t size, uint32_t log_modulus) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < size) out[i] = modulus_switch(in[i], log_modulus);
}

// one LWE: mask with the plain switch, body with the centered-mean correction
// (cc/algorithms/modulus_switch.rs:35-103; cuda/src/crypto/torus.cuh:364-433)
__global__ void __launch_bounds__(256) centered_modulus_switch_kernel(uint64_t *out, const uint64_t *in,
                                                                     uint32_t lwe_dim, uint32_t log_modulus) {
  HX_DYN_SMEM(smem);
  const int tid = threadIdx.x;
  const uint32_t b = block_body_modulus_switch<256>(in, lwe_dim, log_modulus, 1, (uint64_t *)smem, tid);
  if (tid == 0) out[lwe_dim] = b;
  for (uint32_t i = tid; i < lwe_dim; i += 256) out[i] = modulus_switch(in[i], log_modulus);
}

// The same switch with the body correction reduced the way the bootstrap kernels reduce it in their prologue, in a block
// of the shape of the kernel to mimic (cuda/src/crypto/torus.cuh:404-465: 128 threads = the (64, 2) block of the
// throughput kernel, 512 = the generic one; the thread index is linearised).  Here: a block whose x extent is one
// wavefront reduces per wave and redundantly, through 128 words of LDS of its own, as pbs_fft_wave.hip's prologue does;
// any other shape goes through block_body_modulus_switch, the prologue of the block kernels.  Both are exact integer sums,
// so every shape gives the words of centered_modulus_switch_kernel.
template <int TPB, bool WAVES>
__global__ void __launch_bounds__(TPB) centered_modulus_switch_cooperative_kernel(uint64_t *out, const uint64_t *in,
                                                                                uint32_t lwe_dim, uint32_t log_modulus) {
  __shared__ uint64_t scratch[2 * TPB];
  const int tid = threadIdx.x + threadIdx.y * blockDim.x;
  uint32_t b;
  if (WAVES) {
    const int lane = tid & 63;
    uint64_t *buf64 = scratch + (tid >> 6) * 128;
    uint64_t sh = 0;
    int64_t sd = 0;
    for (uint32_t i = lane; i < lwe_dim; i += 64) {
      uint64_t h;
      int64_t dd;
      centered_ms_terms(in[i], log_modulus, h, dd);
      sh += h;
      sd += dd;
    }
    buf64[lane] = sh;
    buf64[64 + lane] = (uint64_t)sd;
    HX_WAVE_SYNC();
    uint64_t th = 0, td = 0;
    for (int l = 0; l < 64; ++l) {
      th += buf64[l];
      td += buf64[64 + l];
    }
    b = (uint32_t)modulus_switch(in[lwe_dim] + centered_ms_finish(th, (int64_t)td, log_modulus), log_modulus);
  } else {
    b = block_body_modulus_switch<TPB>(in, lwe_dim, log_modulus, 1, scratch, tid);
  }
  if (tid == 0) out[lwe_dim] = b;
  for (uint32_t i = tid; i < lwe_dim; i += TPB) out[i] = modulus_switch(in[i], log_modulus);
}

// cc/algorithms/glwe_sample_extraction.rs:89-164 ; indexing of cuda/src/crypto/ciphertext.cuh:32-54
__global__ void sample_extract_kernel(uint64_t *lwe_out, const uint64_t *glwe_in, const uint32_t *nth_array,
                                      uint32_t lwe_per_glwe, uint32_t stored_per_glwe, uint32_t glwe_dim, uint32_t N) {
  const uint32_t id = blockIdx.x;
  const size_t glwe_sz = (size_t)(glwe_dim + 1) * N, lwe_sz = (size_t)glwe_dim * N + 1;
  uint64_t *out = lwe_out + id * lwe_sz;
  const uint64_t *g = glwe_in + (size_t)(id / lwe_per_glwe) * glwe_sz;
  const uint32_t nth = nth_array[id] % stored_per_glwe;
  for (uint32_t p = 0; p < glwe_dim; ++p)
    for (uint32_t j = threadIdx.x; j < N; j += blockDim.x)
      out[(size_t)p * N + j] = (j <= nth) ? g[(size_t)p * N + nth - j] : (uint64_t)0 - g[(size_t)p * N + N + nth - j];
  if (threadIdx.x == 0) out[(size_t)glwe_dim * N] = g[(size_t)glwe_dim * N + nth];
}

// cc/commons/math/decomposition/decomposer.rs:25-50 on one value
__global__ void closest_representable_kernel(const uint64_t *in, uint64_t *out, uint32_t base_log, uint32_t level) {
  const uint32_t shift = 64 - base_log * level - 1;
  uint64_t res = in[0] >> shift;
  res += 1;
  res &= ~1ull;
  out[0] = res << shift;
}

// The multi-bit switch as a launch of its own (only the reference's noise tests call it; in production it is fused into the
// keybundle): per group of g mask words the 2^g subset degrees, subset s summing word m when bit (g - 1 - m) of s is set,
// the sum wrapping BEFORE the switch (cuda/src/crypto/torus.cuh:148-159,612-630; slot 0 = switch(0) = 0, as there)
__global__ void modulus_switch_multi_bit_kernel(uint64_t *out, const uint64_t *in, uint32_t groups, uint32_t log_modulus,
                                                uint32_t g) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= groups) return;
  const uint32_t per = 1u << g;
  const uint64_t *grp = in + (size_t)t * g;
  for (uint32_t s = 0; s < per; ++s) {
    uint64_t sum = 0;
    for (uint32_t m = 0; m < g; ++m)
      if ((s >> (g - 1 - m)) & 1) sum += grp[m];
    out[(size_t)t * per + s] = modulus_switch(sum, log_modulus);
  }
}
void launch_modulus_switch_multi_bit(hipStream_t st, uint64_t *out, const uint64_t *in, uint32_t groups, uint32_t log_modulus,
                                     uint32_t g) {
  if (!groups) return;
  HX_LAUNCH(modulus_switch_multi_bit_kernel, dim3((groups + 255) / 256), dim3(256), 0, st, out, in, groups, log_modulus, g);
}

void launch_modulus_switch(hipStream_t st, uint64_t *out, const uint64_t *in, uint32_t size, uint32_t log_modulus) {
  if (!size) return;
  HX_LAUNCH(modulus_switch_kernel, dim3((size + 255) / 256), dim3(256), 0, st, out, in, size, log_modulus);
}
void launch_centered_modulus_switch(hipStream_t st, uint64_t *out, const uint64_t *in, uint32_t lwe_dim,
                                    uint32_t log_modulus) {
  HX_LAUNCH(centered_modulus_switch_kernel, dim3(1), dim3(256), 2 * 256 * sizeof(uint64_t), st, out, in, lwe_dim,
            log_modulus);
}
bool launch_centered_modulus_switch_cooperative(hipStream_t st, uint64_t *out, const uint64_t *in, uint32_t lwe_dim,
                                                uint32_t log_modulus, uint32_t block_dim_x, uint32_t block_dim_y) {
  const dim3 block(block_dim_x, block_dim_y, 1);
  const bool waves = block_dim_x == 64;
  switch (block_dim_x * block_dim_y) {
  case 128:
    if (waves)
      HX_LAUNCH((centered_modulus_switch_cooperative_kernel<128, true>), dim3(1), block, 0, st, out, in, lwe_dim, log_modulus);
    else
      HX_LAUNCH((centered_modulus_switch_cooperative_kernel<128, false>), dim3(1), block, 0, st, out, in, lwe_dim, log_modulus);
    return true;
  case 512:
    if (waves)
      HX_LAUNCH((centered_modulus_switch_cooperative_kernel<512, true>), dim3(1), block, 0, st, out, in, lwe_dim, log_modulus);
    else
      HX_LAUNCH((centered_modulus_switch_cooperative_kernel<512, false>), dim3(1), block, 0, st, out, in, lwe_dim, log_modulus);
    return true;
  }
  return false;
}
void launch_sample_extract(hipStream_t st, uint64_t *lwe_out, const uint64_t *glwe_in, const uint32_t *nth,
                           uint32_t num_nths, uint32_t lwe_per_glwe, uint32_t stored_per_glwe, uint32_t glwe_dim,
                           uint32_t N) {
  if (!num_nths) return;
  HX_LAUNCH(sample_extract_kernel, dim3(num_nths), dim3(256), 0, st, lwe_out, glwe_in, nth, lwe_per_glwe,
            stored_per_glwe, glwe_dim, N);
}
void launch_closest_representable(hipStream_t st, const uint64_t *in, uint64_t *out, uint32_t base_log, uint32_t level) {
  HX_LAUNCH(closest_representable_kernel, dim3(1), dim3(1), 0, st, in, out, base_log, level);
}

// ------------------------------------------------------------------ compressed GLWE lists: unpack (+ sample extract)
// Value v of a packed GLWE: `bits` bits at bit offset v * bits of its words, least significant first (PackedIntegers,
// cc/entities/compressed_modulus_switched_glwe_ciphertext.rs:171-250), shifted back up to the top of the word
// (compression.cuh:293-340 does the same in a launch of its own).
HX_DEV uint64_t unpack_value(const uint64_t *words, uint32_t v, uint32_t bits) {
  const uint64_t bit = (uint64_t)v * bits;
  const uint32_t w = (uint32_t)(bit >> 6), off = (uint32_t)(bit & 63);
  uint64_t x = words[w] >> off;
  if (off + bits > 64) x |= words[w + 1] << (64 - off);  // (the value's last bit is in range, so is word w + 1)
  return (x & (((uint64_t)1 << bits) - 1)) << (64 - bits);
}

// One workgroup per requested index t: GLWE t / lwe_per_glwe of the packed list, coefficient nth = t % lwe_per_glwe, is
// extracted into an LWE of dimension k*N straight from the packed words — the mask reversal of the sample extraction
// (cc/algorithms/glwe_sample_extraction.rs:89-164) reads value nth - j or, negated, N + nth - j of every mask
// polynomial, the body is value k*N + nth.  The body values beyond the GLWE's count, which decompression treats as
// zero (compression.rs:164-227), are never read: nth is below the count (checked by the caller).
__global__ void __launch_bounds__(256) unpack_extract_kernel(uint64_t *lwe_out, const uint64_t *packed,
                                                             const uint32_t *indexes, uint32_t k, uint32_t N,
                                                             uint32_t lwe_per_glwe, uint32_t bits, uint32_t words_per_glwe) {
  const uint32_t t = indexes[blockIdx.x], nth = t % lwe_per_glwe;
  const uint64_t *words = packed + (size_t)(t / lwe_per_glwe) * words_per_glwe;
  uint64_t *out = lwe_out + (size_t)blockIdx.x * ((size_t)k * N + 1);
  for (uint32_t e = threadIdx.x; e < k * N; e += blockDim.x) {
    const uint32_t q = e / N, j = e - q * N;
    out[e] = j <= nth ? unpack_value(words, q * N + nth - j, bits)
                      : (uint64_t)0 - unpack_value(words, q * N + N + nth - j, bits);
  }
  if (threadIdx.x == 0) out[(size_t)k * N] = unpack_value(words, k * N + nth, bits);
}

// One GLWE of a packed list as (k+1)*N words: the k*N mask values and `bodies` body values, the tail zero
__global__ void __launch_bounds__(256) unpack_glwe_kernel(uint64_t *glwe_out, const uint64_t *words, uint32_t k, uint32_t N,
                                                          uint32_t bodies, uint32_t bits) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < (k + 1) * N) glwe_out[v] = v < k * N + bodies ? unpack_value(words, v, bits) : 0;
}

void launch_unpack_extract(hipStream_t st, uint64_t *lwe_out, const uint64_t *packed, const uint32_t *indexes,
                           uint32_t count, uint32_t k, uint32_t N, uint32_t lwe_per_glwe, uint32_t bits,
                           uint32_t words_per_glwe) {
  if (!count) return;
  HX_LAUNCH(unpack_extract_kernel, dim3(count), dim3(256), 0, st, lwe_out, packed, indexes, k, N, lwe_per_glwe, bits,
            words_per_glwe);
}
void launch_unpack_glwe(hipStream_t st, uint64_t *glwe_out, const uint64_t *words, uint32_t k, uint32_t N, uint32_t bodies,
                        uint32_t bits) {
  HX_LAUNCH(unpack_glwe_kernel, dim3(((k + 1) * N + 255) / 256), dim3(256), 0, st, glwe_out, words, k, N, bodies, bits);
}

// ------------------------------------------------------------------ compact LWE lists: expansion
// Output row o is the list's shared mask times X^d in Z[X]/(X^n_c + 1) followed by body d
// (cc/algorithms/polynomial_algorithms.rs polynomial_wrapping_monic_monomial_mul; cuda/src/zk/expand.cuh lwe_expand):
//   row[e] = mask[e - d]            for d <= e < n_c
//   row[e] = -mask[e - d + n_c]     for e < d
//   row[n_c] = body d, the word at mask + n_c + d
// Only data moves: (n_c + 1) * 8 bytes written per row, the mask read from cache by every workgroup of its list.  Lane
// t of a workgroup stores words t, t + 256, ... of a chunk of kExpandChunk consecutive words of ONE row, so every wave
// store is 64 consecutive 8-byte words (rows are n_c + 1 words long: every other row starts off a 16-byte boundary, so
// 8 bytes is the widest store all rows can take) and the loads are consecutive too, with one break at e = d.
// Grid: x = row, y = chunk of the row.  No LDS.
constexpr uint32_t kExpandThreads = 256, kExpandWordsPerThread = 4, kExpandChunk = kExpandThreads * kExpandWordsPerThread;
__global__ void __launch_bounds__(kExpandThreads) lwe_expand_kernel(uint64_t *__restrict__ out,
                                                                    const uint64_t *__restrict__ in,
                                                                    const ExpandJob *__restrict__ jobs, uint32_t n_c) {
  const ExpandJob job = jobs[blockIdx.x];
  const uint64_t *mask = in + job.mask_offset;
  uint64_t *row = out + (size_t)blockIdx.x * ((size_t)n_c + 1);
  const uint32_t d = job.rotation, first = blockIdx.y * kExpandChunk + threadIdx.x;
  uint64_t v[kExpandWordsPerThread];
  HX_UNROLL
  for (uint32_t u = 0; u < kExpandWordsPerThread; ++u) {
    const uint32_t e = first + u * kExpandThreads;
    v[u] = 0;
    if (e < n_c) {
      const uint64_t m = mask[e < d ? e + n_c - d : e - d];
      v[u] = e < d ? (uint64_t)0 - m : m;
    } else if (e == n_c) {
      v[u] = mask[(size_t)n_c + d];
    }
  }
  HX_UNROLL
  for (uint32_t u = 0; u < kExpandWordsPerThread; ++u) {
    const uint32_t e = first + u * kExpandThreads;
    if (e <= n_c) row[e] = v[u];
  }
}
void launch_lwe_expand(hipStream_t st, uint64_t *lwe_out, const uint64_t *flattened_in, const ExpandJob *jobs,
                       uint32_t n_c, uint32_t num_lwes) {
  if (!num_lwes) return;
  HX_LAUNCH(lwe_expand_kernel, dim3(num_lwes, (n_c + kExpandChunk) / kExpandChunk), dim3(kExpandThreads), 0, st, lwe_out,
            flattened_in, jobs, n_c);
}

// ------------------------------------------------------------------ re-randomisation: rotate and add in place
// Block o of lwe_array gains body o of ONE compact list of encryptions of zero, expanded on the fly (rerand.cuh expands
// into a temporary, then adds: the row moves four times; here it is read once and written once):
//   row[e] += zeros[e - o]          for o <= e < n
//   row[e] -= zeros[e - o + n]      for e < o
//   row[n] += zeros[n + o]
// A re-randomisation reads one list and block o takes rotation o, so there is no job table.  Grid and lane layout of
// lwe_expand_kernel: x = row, y = chunk of kExpandChunk words, 8-byte accesses (rows start off a 16-byte boundary every
// other row), the loads of a lane's four words, row and mask, issued before its stores.  No LDS.
__global__ void __launch_bounds__(kExpandThreads) lwe_rerand_add_kernel(uint64_t *__restrict__ lwe_array,
                                                                        const uint64_t *__restrict__ zeros, uint32_t n) {
  const uint32_t d = blockIdx.x, first = blockIdx.y * kExpandChunk + threadIdx.x;
  uint64_t *row = lwe_array + (size_t)blockIdx.x * ((size_t)n + 1);
  // Every lane loads: a lane past the row's end reads the body word again (index clamped to n) and stores nothing, so the
  // eight loads carry no branch and are all in flight before the first add.
  uint64_t r[kExpandWordsPerThread], z[kExpandWordsPerThread];
  HX_UNROLL
  for (uint32_t u = 0; u < kExpandWordsPerThread; ++u) {
    const uint32_t e = first + u * kExpandThreads, ec = e < n ? e : n;
    r[u] = row[ec];
    z[u] = zeros[ec == n ? (size_t)n + d : (size_t)(ec < d ? ec + n - d : ec - d)];
  }
  HX_UNROLL
  for (uint32_t u = 0; u < kExpandWordsPerThread; ++u) {
    const uint32_t e = first + u * kExpandThreads;
    if (e <= n) row[e] = r[u] + (e < d ? (uint64_t)0 - z[u] : z[u]);
  }
}
void launch_lwe_rerand_add(hipStream_t st, uint64_t *lwe_array, const uint64_t *zeros, uint32_t n, uint32_t count) {
  if (!count) return;
  HX_LAUNCH(lwe_rerand_add_kernel, dim3(count, (n + kExpandChunk) / kExpandChunk), dim3(kExpandThreads), 0, st, lwe_array,
            zeros, n);
}

// out[i] += in[i] over `words` words (the row add behind the keyswitch of a re-randomisation: rows of both sides are
// dense and equally long, so the rows need not be told apart)
__global__ void __launch_bounds__(256) lwe_add_rows_kernel(uint64_t *__restrict__ out, const uint64_t *__restrict__ in,
                                                           size_t words) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < words) out[i] += in[i];
}
void launch_lwe_add_rows(hipStream_t st, uint64_t *out, const uint64_t *in, uint32_t words_per_row, uint32_t count) {
  const size_t words = (size_t)words_per_row * count;
  if (words) HX_LAUNCH(lwe_add_rows_kernel, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, st, out, in, words);
}

__global__ void iota_u64_kernel(uint64_t *out, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = i;
}
void launch_iota_u64(hipStream_t st, uint64_t *out, uint32_t count) {
  if (count) HX_LAUNCH(iota_u64_kernel, dim3((count + 255) / 256), dim3(256), 0, st, out, count);
}

}  // namespace tfhe_hip
