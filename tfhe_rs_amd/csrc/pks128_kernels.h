// pks128_kernels.h — compression of squashed-noise (128-bit) ciphertext lists: the packing keyswitch over Scalar = u128, its
// rotate / sum / modulus switch / bit-pack epilogue, and the unpack (+ sample extract) of the packed lists.
//
// Restated (tfhe-rs): core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187 (one LWE into a GLWE), :296-379 (a list:
// out = sum_i X^i * G_i), commons/math/decomposition/{decomposer,iter}.rs on 128-bit words,
// core_crypto/entities/compressed_modulus_switched_glwe_ciphertext.rs:171-258 (modulus switch, PackedIntegers, extract),
// shortint/list_compression/noise_squashing_compression.rs.  The reference's GPU flow is
// cuda/src/crypto/packing_keyswitch.cuh and cuda/src/integer/compression/compression.cuh:199-291,293-470.
//
// G_i = (0, ..., 0, b_i X^0) - sum_j sum_idx digit_idx(a_i[j]) * K[j][idx]  with the key [n_in][level][(k+1)*N] u128,
// row idx of an input element holding level (level - idx), the digits least significant first.  The decomposed products
// -sum digit * K ("rows", one per LWE) come from one of two kernels, the body b_i is added by the epilogue:
//
//   general kernel (vector ALU)   any 1 <= base_log <= 62, level >= 1, base_log * level <= 128, any n_in: every digit is
//       a signed 64-bit value, the products are taken modulo 2^128 limb by limb; a workgroup shares each key row among
//       the 8 LWEs of its tile.
//   matrix-core kernel            every digit d in J = ceil((base_log + 1) / 8) balanced signed bytes a_j in [-128, 127],
//       every key word in its 16 bytes re-centred to b'_p = byte_p - 128:
//         sum_K d w = sum_{s<16} 2^(8s) ( sum_{j+p=s} sum_K a_j b'_p ) + 0x8080...80 * sum_K d      (mod 2^128)
//       (pairs with j + p >= 16 vanish).  The inner sums are int8 matrix products (hx_mfma_i32_32x32x32_i8); all pairs
//       of one diagonal s share one int32 accumulator: |acc| <= min(J, 16) * K * 2^14, which the shape rule keeps below
//       2^31.  One wave owns a 32 LWE x 32 column tile and all 16 diagonals (256 accumulator registers).
//
// Both kernels may split K over `parts` partial row sets (small batches would otherwise leave most of the device idle);
// the epilogue adds the parts while it reads the rows.  All sums wrap modulo 2^128: any order gives the same words.
//
// A header and not a .hip file: the host emulation build lists its translation units by name and tracks every *.h of this
// directory; this file is included by integer.hip alone, at its end (pks128.h declares what integer.hip calls).
#pragma once
#include "pks128.h"

#include <algorithm>
#include <atomic>

namespace tfhe_hip {

typedef unsigned __int128 u128;
typedef __int128 i128;

static std::atomic<uint32_t> g_pks128_kernel{kPks128Auto};
static std::atomic<uint32_t> g_pks128_last{0};
static std::atomic<uint32_t> g_pks128_max_parts{0};   // 0: the automatic K split (up to 8 shares)
static std::atomic<uint32_t> g_pks128_last_parts{0};
void pks128_set_max_parts(uint32_t parts) { g_pks128_max_parts.store(parts); }
uint32_t pks128_last_parts() { return g_pks128_last_parts.load(); }
void pks128_set_kernel(uint32_t which) {
  HX_PANIC_IF_FALSE(which <= kPks128Matrix, "hip_backend_set_pks128_kernel: %u is not 0 (automatic), 1 (general) or 2 (matrix core)",
                    which);
  g_pks128_kernel.store(which);
}
uint32_t pks128_last_path() { return g_pks128_last.load(); }

// ------------------------------------------------------------------------------------------------ u128 decomposer
// decomposer.rs:156-185 (the closest representable, shifted down and balanced) and iter.rs:122-151 (one digit off the
// state, least significant first) on 128-bit words; with all 128 bits represented the state is the word itself
HX_DEV u128 pks128_init_state(u128 x, uint32_t base_log, uint32_t level) {
  const uint32_t rep = base_log * level;
  if (rep >= 128) return x;
  u128 res = x >> (128 - rep - 1);
  const u128 rounding_bit = res & 1;
  res = (res >> 1) + (res & 1);  // (res + 1) >> 1 without the wrap at rep = 127, where res fills the word
  res &= ~(u128)0 >> (128 - rep);
  const u128 need_balance = (((res - 1) | (rounding_bit << (rep - 1))) & res) >> (rep - 1);
  return res - (need_balance << rep);
}
// base_log <= 62: a digit lies in [-2^61, 2^61]
HX_DEV int64_t pks128_next_digit(uint32_t base_log, u128 &state) {
  const u128 res = state & (((u128)1 << base_log) - 1);
  state = (u128)((i128)state >> base_log);
  const u128 carry = (((res - 1) | state) & res) >> (base_log - 1);
  state += carry;
  return (int64_t)(uint64_t)(res - (carry << base_log));
}

// |d| * w modulo 2^128 from 64 x 64 -> 128 and 64 x 64 -> 64 products (32-bit limbs under the compiler)
HX_DEV u128 pks128_mul(uint64_t mag, u128 w) {
  const u128 lo = (u128)mag * (uint64_t)w;
  const uint64_t hi = mag * (uint64_t)(w >> 64);
  return lo + ((u128)hi << 64);
}

// ------------------------------------------------------------------------------------------------ general kernel
// grid (column tiles of 256, LWE tiles of 8, parts); thread = one column, 8 running sums.  A chunk of 32 mask elements x
// 8 LWEs is one decomposer state per thread; level by level the 256 digits go through LDS and every thread multiplies
// the 32 key words of its column by the 8 digits of each.
constexpr uint32_t kGenLwes = 8, kGenChunk = 32, kGenCols = 256;
__global__ void __launch_bounds__(256) pks128_general_kernel(u128 *rows, const u128 *lwe_in, const u128 *key, uint32_t n_in,
                                                             uint32_t ncols, uint32_t base_log, uint32_t level,
                                                             uint32_t num_lwes, uint32_t per_part) {
  __shared__ int64_t dig[kGenChunk][kGenLwes];
  const uint32_t tid = threadIdx.x, col = blockIdx.x * kGenCols + tid, lwe0 = blockIdx.y * kGenLwes, part = blockIdx.z;
  const uint32_t m_begin = part * per_part, m_end = m_begin + per_part < n_in ? m_begin + per_part : n_in;
  const uint32_t cm = tid / kGenLwes, cl = tid % kGenLwes;
  u128 acc[kGenLwes];
  HX_UNROLL
  for (uint32_t l = 0; l < kGenLwes; ++l) acc[l] = 0;
  for (uint32_t m0 = m_begin; m0 < m_end; m0 += kGenChunk) {
    const bool live = m0 + cm < m_end && lwe0 + cl < num_lwes;
    u128 state = live ? pks128_init_state(lwe_in[(size_t)(lwe0 + cl) * (n_in + 1) + m0 + cm], base_log, level) : 0;
    const uint32_t count = m_end - m0 < kGenChunk ? m_end - m0 : kGenChunk;
    for (uint32_t idx = 0; idx < level; ++idx) {
      dig[cm][cl] = pks128_next_digit(base_log, state);
      __syncthreads();
      if (col < ncols) {
        const u128 *kp = key + ((size_t)m0 * level + idx) * ncols + col;
        for (uint32_t mm = 0; mm < count; ++mm) {
          const u128 w = kp[(size_t)mm * level * ncols];
          HX_UNROLL
          for (uint32_t l = 0; l < kGenLwes; ++l) {
            const int64_t d = dig[mm][l];
            const u128 prod = pks128_mul(d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d, w);
            acc[l] += d < 0 ? prod : (u128)0 - prod;
          }
        }
      }
      __syncthreads();
    }
  }
  if (col < ncols) {
    HX_UNROLL
    for (uint32_t l = 0; l < kGenLwes; ++l)
      if (lwe0 + l < num_lwes) rows[((size_t)part * num_lwes + lwe0 + l) * ncols + col] = acc[l];
  }
}

// ------------------------------------------------------------------------------------------------ matrix-core kernel
// 16 bytes as one load
struct __attribute__((aligned(16))) Pks128Frag {
  int32_t w[4];
};
HX_DEV hx_i8x16 pks128_frag(const Pks128Frag *p) {
  const Pks128Frag f = *p;
  return hx_i8x16{{f.w[0], f.w[1], f.w[2], f.w[3]}};
}

uint32_t pks128_matrix_digit_bytes(uint32_t n_in, uint32_t base_log, uint32_t level) {
  const uint32_t J = (base_log + 1 + 7) / 8;
  const uint64_t K = (uint64_t)n_in * level;
  if (base_log < 1 || base_log > 62 || level < 1 || base_log * level > 128 || J > 8) return 0;
  if (K == 0 || K % 32 != 0) return 0;                     // a whole number of 32-deep steps
  if ((uint64_t)J * K * 16384 >= ((uint64_t)1 << 31)) return 0;  // an int32 diagonal could overflow
  return J;
}
static uint32_t col_tiles(uint32_t ncols) { return (ncols + 31) / 32; }
uint64_t pks128_planes_bytes(uint32_t n_in, uint32_t ncols, uint32_t base_log, uint32_t level) {
  if (!pks128_matrix_digit_bytes(n_in, base_log, level)) return 0;
  return (uint64_t)(n_in * level / 32) * col_tiles(ncols) * 16 * 64 * 16;
}

// Key -> byte planes.  B operand of plane p, step t, column tile c: lane l supplies the 16 bytes b'_p of column
// 32 c + (l & 31) for K = 32 t + 16 (l >> 5) + 0..15.  planes[((t * col_tiles + c) * 16 + p) * 64 + l]; columns past
// ncols (a partial last tile) hold zeros, their products are never stored.  Thread = (t, c, lane): 16 key words in, 16
// planes x 16 bytes out.
__global__ void __launch_bounds__(256) pks128_convert_key_kernel(Pks128Frag *planes, const u128 *key, uint32_t ksteps,
                                                                 uint32_t ncols, uint32_t ctiles) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)ksteps * ctiles * 64) return;
  const uint32_t lane = (uint32_t)(g & 63), c = (uint32_t)((g >> 6) % ctiles), t = (uint32_t)((g >> 6) / ctiles);
  const uint32_t col = c * 32 + (lane & 31), k0 = t * 32 + (lane >> 5) * 16;
  uint8_t bytes[16][16];  // [plane][k]
  for (uint32_t b = 0; b < 16; ++b) {
    const u128 w = col < ncols ? key[(size_t)(k0 + b) * ncols + col] : 0;
    for (uint32_t p = 0; p < 16; ++p)
      bytes[p][b] = col < ncols ? (uint8_t)((uint32_t)(uint8_t)(w >> (8 * p)) - 128u) : 0;
  }
  for (uint32_t p = 0; p < 16; ++p) {
    Pks128Frag f;
    __builtin_memcpy(&f, bytes[p], 16);
    planes[(((size_t)t * ctiles + c) * 16 + p) * 64 + lane] = f;
  }
}
void launch_pks128_convert_key(hipStream_t st, void *planes, const uint64_t *key, uint32_t n_in, uint32_t ncols,
                               uint32_t level) {
  const uint32_t ksteps = n_in * level / 32, ctiles = col_tiles(ncols);
  const size_t threads = (size_t)ksteps * ctiles * 64;
  HX_LAUNCH(pks128_convert_key_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, (Pks128Frag *)planes,
            (const u128 *)key, ksteps, ncols, ctiles);
}

// Digit pass: one workgroup per row of the padded LWE tiles.  A operand of byte j, step t, LWE tile y: lane l supplies
// the 16 bytes a_j of LWE 32 y + (l & 31) for K = 32 t + 16 (l >> 5) + 0..15 (K = mask element * level + idx).
// digits[((y * ksteps + t) * J + j) * 64 + l]; rows past num_lwes are written as zeros.  digit_sums[lwe] = sum_K d.
__global__ void __launch_bounds__(256) pks128_digits_kernel(int8_t *digits, u128 *digit_sums, const u128 *lwe_in,
                                                            uint32_t n_in, uint32_t base_log, uint32_t level, uint32_t J,
                                                            uint32_t num_lwes) {
  __shared__ u128 part[256];
  const uint32_t lwe = blockIdx.x, y = lwe >> 5, row = lwe & 31, ksteps = n_in * level / 32;
  i128 sum = 0;
  for (uint32_t m = threadIdx.x; m < n_in; m += blockDim.x) {
    u128 state = lwe < num_lwes ? pks128_init_state(lwe_in[(size_t)lwe * (n_in + 1) + m], base_log, level) : 0;
    for (uint32_t idx = 0; idx < level; ++idx) {
      int64_t d = pks128_next_digit(base_log, state);
      sum += d;
      const uint32_t kk = m * level + idx, t = kk >> 5, lane = ((kk >> 4) & 1) * 32 + row, byte = kk & 15;
      for (uint32_t j = 0; j < J; ++j) {
        const int8_t a = (int8_t)(uint8_t)((uint64_t)d & 0xff);  // balanced byte: d = a + 256 * d'
        d = (d - a) >> 8;
        digits[((((size_t)y * ksteps + t) * J + j) * 64 + lane) * 16 + byte] = a;
      }
    }
  }
  part[threadIdx.x] = (u128)sum;
  __syncthreads();
  if (threadIdx.x == 0 && lwe < num_lwes) {
    u128 s = 0;
    for (uint32_t i = 0; i < blockDim.x; ++i) s += part[i];
    digit_sums[lwe] = s;
  }
}

// One wave per (LWE tile, column tile, part); a workgroup holds up to 4 waves on consecutive LWE tiles of the same column
// tile, so they read the same key planes at about the same time.  No LDS, no barrier: a wave without work leaves at once.
template <int J>
__global__ void __launch_bounds__(256) pks128_matrix_kernel(u128 *rows, const Pks128Frag *digits, const Pks128Frag *planes,
                                                            const u128 *digit_sums, uint32_t num_lwes, uint32_t ncols,
                                                            uint32_t ksteps, uint32_t steps_per_part) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t c = blockIdx.x, ctiles = gridDim.x, y = blockIdx.y * (blockDim.x >> 6) + wave, part = blockIdx.z;
  if (y * 32 >= num_lwes) return;
  hx_i32x16 acc[16];
  HX_UNROLL
  for (int s = 0; s < 16; ++s) {
    HX_UNROLL
    for (int r = 0; r < 16; ++r) acc[s].v[r] = 0;
  }
  const uint32_t t0 = part * steps_per_part;
  const Pks128Frag *ap = digits + ((size_t)y * ksteps + t0) * J * 64 + lane;
  const Pks128Frag *bp = planes + ((size_t)t0 * ctiles + c) * 16 * 64 + lane;
  HX_NO_UNROLL
  for (uint32_t t = 0; t < steps_per_part; ++t) {
    hx_i8x16 a[J];
    HX_UNROLL
    for (int j = 0; j < J; ++j) a[j] = pks128_frag(ap + j * 64);
    HX_UNROLL
    for (int p = 0; p < 16; ++p) {
      const hx_i8x16 b = pks128_frag(bp + p * 64);
      HX_UNROLL
      for (int j = 0; j < J; ++j)
        if (j + p < 16) acc[j + p] = hx_mfma_i32_32x32x32_i8(a[j], b, acc[j + p]);
    }
    ap += J * 64;
    bp += (size_t)ctiles * 16 * 64;
  }
  // D[row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][col = lane & 31] in v[r]
  const uint32_t col = c * 32 + (lane & 31);
  HX_UNROLL
  for (int r = 0; r < 16; ++r) {
    const uint32_t lwe = y * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    u128 v = 0;
    HX_UNROLL
    for (int s = 0; s < 16; ++s) v += (u128)(i128)acc[s].v[r] << (8 * s);
    if (lwe < num_lwes && col < ncols) {
      // the re-centring term, once: 128 * sum_p 2^(8p) times the digit sum
      if (part == 0) v += digit_sums[lwe] * (((u128)0x8080808080808080ull << 64) | 0x8080808080808080ull);
      rows[((size_t)part * num_lwes + lwe) * ncols + col] = (u128)0 - v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ K split
constexpr uint32_t kTargetWaves = 1024;  // one 512-register wave per SIMD on 256 compute units
// `limit`: the most shares a call may take (8 unless hip_backend_set_pks128_max_parts lowered it)
static uint32_t matrix_parts(uint32_t num_lwes, uint32_t ncols, uint32_t ksteps, uint32_t limit = 8) {
  const uint64_t waves = (uint64_t)col_tiles(ncols) * ((num_lwes + 31) / 32);
  uint32_t parts = 1;
  while (parts * 2 <= limit && waves * parts * 2 <= kTargetWaves && ksteps % (parts * 2) == 0) parts *= 2;
  return parts;
}
static uint32_t general_parts(uint32_t num_lwes, uint32_t ncols, uint32_t n_in, uint32_t limit = 8) {
  const uint64_t groups = (uint64_t)((ncols + kGenCols - 1) / kGenCols) * ((num_lwes + kGenLwes - 1) / kGenLwes);
  const uint32_t chunks = (n_in + kGenChunk - 1) / kGenChunk;
  uint32_t parts = 1;
  while (parts * 2 <= limit && groups * parts * 2 <= kTargetWaves && chunks >= parts * 2) parts *= 2;
  return parts;
}
// The share count of a batch never grows with the batch, so shares * LWEs peaks at the largest batch of some share count:
// four binary searches instead of a walk over every batch size.
uint64_t pks128_rows_bytes(uint32_t cap, uint32_t n_in, uint32_t ncols, uint32_t base_log, uint32_t level) {
  const bool matrix = pks128_matrix_digit_bytes(n_in, base_log, level) != 0;
  auto parts_of = [&](uint32_t n) {
    const uint32_t parts = general_parts(n, ncols, n_in);
    return matrix ? std::max(parts, matrix_parts(n, ncols, n_in * level / 32)) : parts;
  };
  uint64_t most = cap;  // one share at the full batch
  for (uint32_t p = 2; p <= 8; p *= 2) {
    if (parts_of(1) < p) break;
    uint32_t lo = 1, hi = cap;  // the largest n in 1..cap with parts_of(n) >= p
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      if (parts_of(mid) >= p) lo = mid;
      else hi = mid - 1;
    }
    most = std::max(most, (uint64_t)parts_of(lo) * lo);
  }
  return most * ncols * sizeof(u128);
}
uint64_t pks128_digits_bytes(uint32_t cap, uint32_t n_in, uint32_t base_log, uint32_t level) {
  const uint32_t J = pks128_matrix_digit_bytes(n_in, base_log, level);
  return (uint64_t)((cap + 31) / 32) * (n_in * level / 32) * J * 64 * 16;
}

// ------------------------------------------------------------------------------------------------ epilogue
// The u128 counterpart of pks_rotate_pack_kernel (keyswitch.hip): one workgroup per 64 consecutive output values of one
// GLWE.  Value v (polynomial q = v / N, coefficient p = v % N) is  sum_i +-G_i[q][(p - i) mod N]  (minus where p < i: the
// monic monomial X^i, negacyclic), G_i = the parts of row i added up, plus the input body at coefficient 0 of the body
// polynomial; the four waves take every fourth LWE.  No multiplication by message_modulus (a squashed block is shipped as
// it is).  s = storage_log_modulus in 1..127: (x + 2^(127-s)) >> (128-s); s = 128: the identity (no shift by 128 or -1 is
// evaluated); the 64 values are bit-packed least significant first into exactly s u64 words = s / 2 u128 words (lo word
// first: the PackedIntegers layout over u128), workgroups never share a u64 word.  Values past `nvals` count as zero; the
// padding up to whole u128 words is written as zeros.  s = 0: the 64 raw words are stored (the unswitched GLWE).
__global__ void __launch_bounds__(256) pks128_rotate_pack_kernel(uint64_t *out, const u128 *rows, const u128 *lwe_in,
                                                                 uint32_t n_in, uint32_t k, uint32_t N, uint32_t num_lwes,
                                                                 uint32_t lwe_per_glwe, uint32_t nvals, uint32_t s,
                                                                 uint32_t words64_per_glwe, uint32_t parts) {
  __shared__ u128 share[4][64];
  const uint32_t c = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const uint32_t glwe = blockIdx.y, v = blockIdx.x * 64 + c;
  const uint32_t ncols = (k + 1) * N, first = glwe * lwe_per_glwe;
  const uint32_t m = num_lwes - first < lwe_per_glwe ? num_lwes - first : lwe_per_glwe;  // LWEs of this GLWE
  u128 acc = 0;
  if (v < nvals) {
    const uint32_t q = v / N, p = v - q * N;
    for (uint32_t i = sl; i < m; i += 4) {
      const uint32_t idx = (p - i) & (N - 1), col = q * N + idx;
      u128 g = 0;
      for (uint32_t pt = 0; pt < parts; ++pt) g += rows[((size_t)pt * num_lwes + first + i) * ncols + col];
      if (q == k && idx == 0) g += lwe_in[(size_t)(first + i) * (n_in + 1) + n_in];
      acc += p >= i ? g : (u128)0 - g;
    }
  }
  share[sl][c] = acc;
  __syncthreads();
  if (sl == 0) {
    const u128 x = share[0][c] + share[1][c] + share[2][c] + share[3][c];
    if (s == 0) {
      if (v < nvals) ((u128 *)out)[(size_t)glwe * ncols + v] = x;
    } else {
      share[0][c] = v >= nvals ? (u128)0 : s == 128 ? x : (x + ((u128)1 << (127 - s))) >> (128 - s);
    }
  }
  if (s == 0) return;
  __syncthreads();
  const uint32_t j = threadIdx.x, w = blockIdx.x * s + j;  // u64 word j of this workgroup's s words
  if (j < s && w < words64_per_glwe) {
    const uint32_t t_lo = (64 * j) / s, t_hi = (64 * j + 63) / s < 63 ? (64 * j + 63) / s : 63;
    uint64_t word = 0;
    for (uint32_t t = t_lo; t <= t_hi; ++t) {
      const int sh = (int)(t * s) - (int)(64 * j);  // -128 < sh < 64
      word |= sh >= 0 ? (uint64_t)(share[0][t] << sh) : (uint64_t)(share[0][t] >> (-sh));
    }
    out[(size_t)glwe * words64_per_glwe + w] = word;
  }
  // 64 values x s bits of the last workgroup may end on an odd u64 word: the upper half of that u128 word is padding
  if (blockIdx.x == gridDim.x - 1 && j == s && w < words64_per_glwe) out[(size_t)glwe * words64_per_glwe + w] = 0;
}

uint32_t pks128_words_per_glwe(uint32_t glwe_dim, uint32_t N, uint32_t lwe_per_glwe, uint32_t bits) {
  return (uint32_t)((((uint64_t)glwe_dim * N + lwe_per_glwe) * bits + 127) / 128);
}

template <int J>
static void launch_matrix(hipStream_t st, const Pks128Workspace &ws, const void *planes, uint32_t num_lwes, uint32_t ncols,
                          uint32_t ksteps, uint32_t parts) {
  const uint32_t ytiles = (num_lwes + 31) / 32, waves = ytiles < 4 ? ytiles : 4;
  HX_LAUNCH(pks128_matrix_kernel<J>, dim3(col_tiles(ncols), (ytiles + waves - 1) / waves, parts), dim3(64 * waves), 0, st,
            (u128 *)ws.rows, (const Pks128Frag *)ws.digits, (const Pks128Frag *)planes, (const u128 *)ws.digit_sums,
            num_lwes, ncols, ksteps, ksteps / parts);
}

void launch_packing_keyswitch128(hipStream_t st, uint64_t *out, const Pks128Workspace &ws, const uint64_t *lwe_in,
                                 const uint64_t *key, const void *planes, uint32_t n_in, uint32_t glwe_dim, uint32_t N,
                                 uint32_t base_log, uint32_t level, uint32_t num_lwes, uint32_t lwe_per_glwe,
                                 uint32_t storage_log_modulus) {
  if (num_lwes == 0) return;
  const uint32_t ncols = (glwe_dim + 1) * N, glwes = (num_lwes + lwe_per_glwe - 1) / lwe_per_glwe;
  const uint32_t J = planes ? pks128_matrix_digit_bytes(n_in, base_log, level) : 0;
  const uint32_t want = g_pks128_kernel.load();
  const uint32_t cap = g_pks128_max_parts.load(), limit = cap ? std::min(cap, 8u) : 8u;
  // automatic: the matrix-core kernel wherever it carries the shape (docs/history/compression128_log.md)
  const bool matrix = J != 0 && want != kPks128General;
  uint32_t parts;
  if (matrix) {
    const uint32_t ksteps = n_in * level / 32;
    parts = matrix_parts(num_lwes, ncols, ksteps, limit);
    HX_LAUNCH(pks128_digits_kernel, dim3((num_lwes + 31) / 32 * 32), dim3(256), 0, st, (int8_t *)ws.digits,
              (u128 *)ws.digit_sums, (const u128 *)lwe_in, n_in, base_log, level, J, num_lwes);
    switch (J) {
      case 1: launch_matrix<1>(st, ws, planes, num_lwes, ncols, ksteps, parts); break;
      case 2: launch_matrix<2>(st, ws, planes, num_lwes, ncols, ksteps, parts); break;
      case 3: launch_matrix<3>(st, ws, planes, num_lwes, ncols, ksteps, parts); break;
      case 4: launch_matrix<4>(st, ws, planes, num_lwes, ncols, ksteps, parts); break;
      case 5: launch_matrix<5>(st, ws, planes, num_lwes, ncols, ksteps, parts); break;
      case 6: launch_matrix<6>(st, ws, planes, num_lwes, ncols, ksteps, parts); break;
      case 7: launch_matrix<7>(st, ws, planes, num_lwes, ncols, ksteps, parts); break;
      default: launch_matrix<8>(st, ws, planes, num_lwes, ncols, ksteps, parts); break;
    }
  } else {
    parts = general_parts(num_lwes, ncols, n_in, limit);
    const uint32_t chunks = (n_in + kGenChunk - 1) / kGenChunk, per_part = (chunks + parts - 1) / parts * kGenChunk;
    HX_LAUNCH(pks128_general_kernel, dim3((ncols + kGenCols - 1) / kGenCols, (num_lwes + kGenLwes - 1) / kGenLwes, parts),
              dim3(256), 0, st, (u128 *)ws.rows, (const u128 *)lwe_in, (const u128 *)key, n_in, ncols, base_log, level,
              num_lwes, per_part);
  }
  g_pks128_last.store(matrix ? 1 : 0);
  g_pks128_last_parts.store(parts);
  const uint32_t s = storage_log_modulus, nvals = s ? glwe_dim * N + lwe_per_glwe : ncols;
  const uint32_t words64 = s ? 2 * pks128_words_per_glwe(glwe_dim, N, lwe_per_glwe, s) : 2 * ncols;
  HX_LAUNCH(pks128_rotate_pack_kernel, dim3((nvals + 63) / 64, glwes), dim3(256), 0, st, out, (const u128 *)ws.rows,
            (const u128 *)lwe_in, n_in, glwe_dim, N, num_lwes, lwe_per_glwe, nvals, s, words64, parts);
}

// ------------------------------------------------------------------------------------------------ unpack (+ extract)
// Value v of a packed GLWE: `bits` bits at bit offset v * bits of its words read as u64 words, lo word of a u128 first
// (PackedIntegers), scaled back up by << (128 - bits).  The value's last bit is inside the GLWE's words, so is every
// word read here.
HX_DEV u128 pks128_unpack_value(const uint64_t *words, uint32_t v, uint32_t bits) {
  const uint64_t bit = (uint64_t)v * bits;
  const size_t w = (size_t)(bit >> 6);
  const uint32_t off = (uint32_t)(bit & 63);
  u128 x = (u128)(words[w] >> off);
  if (off + bits > 64) x |= (u128)words[w + 1] << (64 - off);
  if (off + bits > 128) x |= (u128)words[w + 2] << (128 - off);  // off >= 1 here
  if (bits < 128) x = (x & (((u128)1 << bits) - 1)) << (128 - bits);
  return x;
}

// One workgroup per requested index t: GLWE t / lwe_per_glwe, coefficient nth = t % lwe_per_glwe, sample-extracted
// (cc/algorithms/glwe_sample_extraction.rs:89-164) straight from the packed words.  The body values beyond a GLWE's count
// are never read: nth is below the count (checked by the caller).
__global__ void __launch_bounds__(256) pks128_unpack_extract_kernel(u128 *lwe_out, const uint64_t *packed,
                                                                    const uint32_t *indexes, uint32_t k, uint32_t N,
                                                                    uint32_t lwe_per_glwe, uint32_t bits,
                                                                    uint32_t words64_per_glwe) {
  const uint32_t t = indexes[blockIdx.x], nth = t % lwe_per_glwe;
  const uint64_t *words = packed + (size_t)(t / lwe_per_glwe) * words64_per_glwe;
  u128 *out = lwe_out + (size_t)blockIdx.x * ((size_t)k * N + 1);
  for (uint32_t e = threadIdx.x; e < k * N; e += blockDim.x) {
    const uint32_t q = e / N, j = e - q * N;
    out[e] = j <= nth ? pks128_unpack_value(words, q * N + nth - j, bits)
                      : (u128)0 - pks128_unpack_value(words, q * N + N + nth - j, bits);
  }
  if (threadIdx.x == 0) out[(size_t)k * N] = pks128_unpack_value(words, k * N + nth, bits);
}
__global__ void __launch_bounds__(256) pks128_unpack_glwe_kernel(u128 *glwe_out, const uint64_t *words, uint32_t k,
                                                                 uint32_t N, uint32_t bodies, uint32_t bits) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < (k + 1) * N) glwe_out[v] = v < k * N + bodies ? pks128_unpack_value(words, v, bits) : (u128)0;
}

void launch_unpack_extract128(hipStream_t st, uint64_t *lwe_out, const uint64_t *packed, const uint32_t *indexes,
                              uint32_t count, uint32_t glwe_dim, uint32_t N, uint32_t lwe_per_glwe, uint32_t bits) {
  if (!count) return;
  HX_LAUNCH(pks128_unpack_extract_kernel, dim3(count), dim3(256), 0, st, (u128 *)lwe_out, packed, indexes, glwe_dim, N,
            lwe_per_glwe, bits, 2 * pks128_words_per_glwe(glwe_dim, N, lwe_per_glwe, bits));
}
void launch_unpack_glwe128(hipStream_t st, uint64_t *glwe_out, const uint64_t *words, uint32_t glwe_dim, uint32_t N,
                           uint32_t bodies, uint32_t bits) {
  HX_LAUNCH(pks128_unpack_glwe_kernel, dim3(((glwe_dim + 1) * N + 255) / 256), dim3(256), 0, st, (u128 *)glwe_out, words,
            glwe_dim, N, bodies, bits);
}

}  // namespace tfhe_hip
