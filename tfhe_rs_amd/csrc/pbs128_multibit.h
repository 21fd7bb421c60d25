// pbs128_multibit.h — the multi-bit programmable bootstrap over the 128-bit torus (noise squashing on a multi-bit key):
// the key-bundle kernel, the accumulate kernel and their launchers.  Arithmetic, tables, the LDS transform and the u128
// decomposer are pbs128.h's.
//
// Restated: the standard-domain form std_multi_bit_f128_deterministic_blind_rotate_assign
// (tfhe/src/core_crypto/algorithms/lwe_multi_bit_programmable_bootstrapping.rs) and the reference GPU backend's
// pbs/programmable_bootstrap_multibit_128.cuh (algorithm).  The key stays in the STANDARD domain on the device (u128, the
// reference's container order); the bundle of a group, GGSW_0 + sum_{s >= 1} X^{deg_s} GGSW_s, is summed exactly modulo
// 2^128 and only then transformed "as torus" — no monomial is multiplied in the Fourier domain.  Subset numbering and
// deg_s: multi_bit_degrees' (pbs_common.h), i.e. subset s selects mask element m when bit g - 1 - m of s is set, the sum
// wraps on u64 before the plain modulus switch to 2 N.  Groups are applied in ascending order.
//
// Launch shape: per chunk of groups one key-bundle launch (a workgroup per sample, group and polynomial: the work that
// spreads over the chip) and one accumulate launch (a workgroup per sample: the sequential chain of n / g full external
// products), on the caller's stream, no synchronisation between workgroups.
//
// A header included by abi.hip alone, as pbs128.h is; explicit fma() and -ffp-contract=off apply as there.
#pragma once
#include "pbs128.h"

namespace tfhe_hip {

// The key bundles of one chunk take  samples x groups x (k + 1)^2 level x 16 N  bytes; a chunk is the largest number of
// groups that stays under this cap for the scratch's sample count (at least one group, at most kPbs128MbMaxChunk: the
// scratch is sized without knowing n or the grouping factor).  Not measured against other caps on the device yet
// (docs/history/pbs128_log.md).
constexpr uint64_t kPbs128MbBundleBytes = 512ull << 20;
constexpr uint32_t kPbs128MbMaxChunk = 1024;

struct Pbs128MbArgs {
  u128 *lwe_out;            // LWEs of k N + 1 words, sample s written at out_idx[s]
  const uint64_t *out_idx;
  const u128 *lut;          // one GLWE, (k + 1) N words
  const uint64_t *lwe_in;   // LWEs of n + 1 u64 words, sample s read at in_idx[s]
  const uint64_t *in_idx;
  const u128 *bsk;          // [n / g][2^g][level, index 0 = last level][k + 1][k + 1][N]
  double *bundle;           // [sample][group of the chunk][level][row][col] polynomials of four planes of N / 2 doubles
  u128 *acc_buf;            // (k + 1) N words per sample: ACC between chunks (and all along where ACC_GLOBAL)
  uint32_t n, g, base_log, level, num_samples;
  uint32_t group0, groups;  // this chunk: its first group and how many
  uint32_t first, last;     // this chunk initialises ACC / extracts the sample
};

// One workgroup per (sample, group of the chunk, polynomial of the GGSW); the sample varies fastest, so workgroups
// resident together read the same 2^g key polynomials.  Each thread holds its 2 PER coefficients (j and j + N / 2, the
// pairing of pbs128_kernel's state[]) of the sum as u128 in registers.
template <int N>
__global__ void __launch_bounds__(Cfg128<N>::TPB) pbs128_mb_keybundle_kernel(Pbs128MbArgs a, Fft128Tables tb) {
  constexpr int n = N / 2, TPB = Cfg128<N>::TPB, PER = n / TPB, LOG2N2 = ilog2_c(2 * N);
  HX_DYN_SMEM(smem);
  const F128Buf buf{(double *)smem, f128buf_stride(N)};
  const int tid = threadIdx.x;
  const uint32_t sample = blockIdx.x % a.num_samples, job = blockIdx.x / a.num_samples;
  const uint32_t grp = job % a.groups, poly = job / a.groups;
  const uint32_t polys = gridDim.x / (a.num_samples * a.groups), per = 1u << a.g;
  const uint64_t *mask = a.lwe_in + (size_t)a.in_idx[sample] * (a.n + 1) + (size_t)(a.group0 + grp) * a.g;
  const u128 *ggsw = a.bsk + ((size_t)(a.group0 + grp) * per * polys + poly) * N;

  u128 sum[2 * PER];
  HX_UNROLL
  for (int q = 0; q < PER; ++q) {
    sum[2 * q] = ggsw[tid + q * TPB];
    sum[2 * q + 1] = ggsw[tid + q * TPB + n];
  }
  HX_NO_UNROLL
  for (uint32_t s = 1; s < per; ++s) {
    uint64_t word = 0;  // uniform across the workgroup
    for (uint32_t m = 0; m < a.g; ++m)
      if ((s >> (a.g - 1 - m)) & 1) word += mask[m];
    const uint32_t deg = (uint32_t)modulus_switch(word, LOG2N2);
    const u128 *p = ggsw + (size_t)s * polys * N;
    HX_UNROLL
    for (int h = 0; h < 2 * PER; ++h) {
      bool neg;
      const uint32_t src = monomial_mul_src((uint32_t)(tid + (h >> 1) * TPB + (h & 1) * n), deg, N, neg);
      const u128 v = p[src];
      sum[h] += neg ? (u128)0 - v : v;
    }
  }
  const double scale = 2.938735877055718769921841343055614194546826e-39;  // 2^-128: "as torus"
  HX_UNROLL
  for (int q = 0; q < PER; ++q) {
    const f128 x = u128_to_signed_f128(sum[2 * q]), y = u128_to_signed_f128(sum[2 * q + 1]);
    buf.put(tid + q * TPB, c128{f128{x.hi * scale, x.lo * scale}, f128{y.hi * scale, y.lo * scale}});
  }
  __syncthreads();
  lds_fft128_forward<N, TPB>(buf, tb.fwd, tid);
  double *o = a.bundle + (((size_t)sample * a.groups + grp) * polys + poly) * (4 * n);
  HX_UNROLL
  for (int q = 0; q < PER; ++q) {
    const int j = tid + q * TPB;
    const c128 v = buf.get(j);
    o[j] = v.re.hi;
    o[n + j] = v.re.lo;
    o[2 * n + j] = v.im.hi;
    o[3 * n + j] = v.im.lo;
  }
}

// One workgroup per sample: for every group of the chunk a FULL external product ACC <- bundle [.] ACC.  The digits come
// off the closest representable of ACC itself, least significant first; the k + 1 backward transforms REPLACE ACC, which
// is safe in place because every read of ACC for the decomposition precedes the first of them (pbs128_kernel's loop
// structure).  BL, LV, ACC_GLOBAL as in pbs128_kernel.
template <int N, int K1, int BL, int LV, bool ACC_GLOBAL>
__global__ void __launch_bounds__(Cfg128<N>::TPB) pbs128_mb_accumulate_kernel(Pbs128MbArgs a, Fft128Tables tb) {
  constexpr int n = N / 2, TPB = Cfg128<N>::TPB, PER = n / TPB, LOG2N2 = ilog2_c(2 * N);
  HX_DYN_SMEM(smem);
  const int tid = threadIdx.x;
  const uint32_t sample = blockIdx.x;
  u128 *saved = a.acc_buf + (size_t)sample * K1 * N;
  u128 *acc = ACC_GLOBAL ? saved : (u128 *)smem;
  const F128Buf buf{(double *)(smem + (ACC_GLOBAL ? 0 : (size_t)K1 * N * 16)), f128buf_stride(N)};
  const uint32_t base_log = BL ? (uint32_t)BL : a.base_log, level = LV ? (uint32_t)LV : a.level;

  if (a.first) {  // acc <- LUT * X^{-b_hat}; multi-bit takes the plain switch of the body
    const uint32_t b_hat = (uint32_t)modulus_switch(a.lwe_in[(size_t)a.in_idx[sample] * (a.n + 1) + a.n], LOG2N2);
    for (int p = 0; p < K1; ++p)
      for (uint32_t j = tid; j < (uint32_t)N; j += TPB) {
        bool neg;
        const uint32_t src = monomial_div_src(j, b_hat, N, neg);
        const u128 v = a.lut[p * N + src];
        acc[p * N + j] = neg ? (u128)0 - v : v;
      }
  } else if (!ACC_GLOBAL) {
    for (uint32_t j = tid; j < (uint32_t)(K1 * N); j += TPB) acc[j] = saved[j];
  }
  __syncthreads();

  const double *kb = a.bundle + (size_t)sample * a.groups * level * K1 * K1 * (4 * n);
  for (uint32_t grp = 0; grp < a.groups; ++grp) {
    c128 facc[K1][PER];
    bool first = true;
    HX_NO_UNROLL
    for (int row = 0; row < K1; ++row) {
      u128 state[2 * PER];
      HX_UNROLL
      for (int q = 0; q < PER; ++q) {
        const uint32_t j = tid + q * TPB;
        state[2 * q] = decomp_init_state128(acc[row * N + j], base_log, level);
        state[2 * q + 1] = decomp_init_state128(acc[row * N + j + n], base_log, level);
      }
      HX_NO_UNROLL
      for (uint32_t idx = 0; idx < level; ++idx) {
        HX_UNROLL
        for (int q = 0; q < PER; ++q)
          buf.put(tid + q * TPB, c128{digit_to_f128<BL>(decompose_one_level128(base_log, state[2 * q]), base_log),
                                      digit_to_f128<BL>(decompose_one_level128(base_log, state[2 * q + 1]), base_log)});
        __syncthreads();
        lds_fft128_forward<N, TPB>(buf, tb.fwd, tid);
        const double *brow = kb + ((((size_t)grp * level + idx) * K1 + row) * K1) * (4 * n);
        HX_UNROLL
        for (int c = 0; c < K1; ++c) {
          HX_UNROLL
          for (int q = 0; q < PER; ++q) {
            const int pos = tid + q * TPB;
            const double *kp = brow + (size_t)c * (4 * n) + pos;
            const c128 y{f128{kp[0], kp[n]}, f128{kp[2 * n], kp[3 * n]}};
            facc[c][q] = first ? c128_mul(buf.get(pos), y) : c128_mul_add(buf.get(pos), y, facc[c][q]);
          }
        }
        first = false;
        __syncthreads();
      }
    }
    HX_UNROLL
    for (int c = 0; c < K1; ++c) {
      HX_UNROLL
      for (int q = 0; q < PER; ++q) buf.put(tid + q * TPB, facc[c][q]);
      __syncthreads();
      lds_fft128_inverse<N, TPB>(buf, tb.inv, tid);
      HX_UNROLL
      for (int q = 0; q < PER; ++q) {
        const int j = tid + q * TPB;
        const c128 t = untwist128(buf.get(j), tb.untw, j);
        acc[c * N + j] = f128_to_torus_u128(t.re);
        acc[c * N + j + n] = f128_to_torus_u128(t.im);
      }
      __syncthreads();
    }
  }

  if (!a.last) {
    if (!ACC_GLOBAL)
      for (uint32_t j = tid; j < (uint32_t)(K1 * N); j += TPB) saved[j] = acc[j];
    return;
  }
  // sample extraction of coefficient 0 (cc/algorithms/glwe_sample_extraction.rs:119-146)
  constexpr int k = K1 - 1;
  u128 *out = a.lwe_out + (size_t)a.out_idx[sample] * ((size_t)k * N + 1);
  for (int p = 0; p < k; ++p)
    for (uint32_t j = tid; j < (uint32_t)N; j += TPB) out[(size_t)p * N + j] = j == 0 ? acc[p * N] : (u128)0 - acc[p * N + N - j];
  if (tid == 0) out[(size_t)k * N] = acc[k * N];
}

// ------------------------------------------------------------------------------------------------ launchers
inline size_t pbs128_mb_polys(uint32_t glwe_dim, uint32_t level) { return (size_t)level * (glwe_dim + 1) * (glwe_dim + 1); }

template <int N>
static void launch_pbs128_mb_keybundle_n(hipStream_t st, const Pbs128MbArgs &a, uint32_t glwe_dim, const Fft128Tables &tb) {
  const uint64_t blocks = (uint64_t)a.num_samples * a.groups * pbs128_mb_polys(glwe_dim, a.level);
  HX_PANIC_IF_FALSE(blocks * Cfg128<N>::TPB < (1ull << 32), "multi-bit 128-bit PBS: a key-bundle grid of %llu workgroups",
                    (unsigned long long)blocks);
  if (f128buf_bytes(N) > 48 * 1024) hx_set_dynamic_smem_once<pbs128_mb_keybundle_kernel<N>>(f128buf_bytes(N));
  HX_LAUNCH((pbs128_mb_keybundle_kernel<N>), dim3((unsigned)blocks), dim3(Cfg128<N>::TPB), f128buf_bytes(N), st, a, tb);
}
inline void launch_pbs128_mb_keybundle(hipStream_t st, uint32_t N, uint32_t glwe_dim, const Pbs128MbArgs &a,
                                       const Fft128Tables &tb) {
  HX_DISPATCH_N128(launch_pbs128_mb_keybundle_n, st, a, glwe_dim, tb);
}

template <int N, int K1, int BL, int LV>
static void launch_pbs128_mb_inst(hipStream_t st, const Pbs128MbArgs &a, const Fft128Tables &tb) {
  constexpr bool G = pbs128_acc_global(N, K1);
  const size_t smem = (G ? 0 : (size_t)K1 * N * 16) + f128buf_bytes(N);
  hx_set_dynamic_smem_once<pbs128_mb_accumulate_kernel<N, K1, BL, LV, G>>(smem);
  HX_LAUNCH((pbs128_mb_accumulate_kernel<N, K1, BL, LV, G>), dim3(a.num_samples), dim3(Cfg128<N>::TPB), smem, st, a, tb);
}
template <int N, int K1>
static void launch_pbs128_mb_nk(hipStream_t st, const Pbs128MbArgs &a, const Fft128Tables &tb) {
  // the noise-squashing set of PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2 (k = 2, N = 2048, 4 levels of 18 bits) is a
  // fixed instantiation
  if constexpr (N == 2048 && K1 == 3) {
    if (a.base_log == 18 && a.level == 4) return launch_pbs128_mb_inst<N, K1, 18, 4>(st, a, tb);
  }
  launch_pbs128_mb_inst<N, K1, 0, 0>(st, a, tb);
}
// The multi-bit list of (polynomial_size, glwe_dimension) pairs: those of pbs128_dispatch.  a == nullptr: only answers
// whether the pair is listed.
inline bool pbs128_mb_dispatch(hipStream_t st, uint32_t N, uint32_t glwe_dim, const Pbs128MbArgs *a, const Fft128Tables *tb) {
#define HX_PBS128_MB_CASE(N_, K1_)                                 \
  if (N == N_ && glwe_dim + 1 == K1_) {                            \
    if (a != nullptr) launch_pbs128_mb_nk<N_, K1_>(st, *a, *tb);   \
    return true;                                                   \
  }
  HX_PBS128_MB_CASE(256, 2) HX_PBS128_MB_CASE(256, 3) HX_PBS128_MB_CASE(256, 4)
  HX_PBS128_MB_CASE(512, 2) HX_PBS128_MB_CASE(512, 3) HX_PBS128_MB_CASE(512, 4)
  HX_PBS128_MB_CASE(1024, 2) HX_PBS128_MB_CASE(1024, 3) HX_PBS128_MB_CASE(1024, 4)
  HX_PBS128_MB_CASE(2048, 2) HX_PBS128_MB_CASE(2048, 3)
  HX_PBS128_MB_CASE(4096, 2)
#undef HX_PBS128_MB_CASE
  if (a != nullptr) HX_PANIC("unsupported (polynomial_size=%u, glwe_dimension=%u) for the 128-bit PBS", N, glwe_dim);
  return false;
}

// The whole bootstrap: keybundle(chunk 0), accumulate(chunk 0), keybundle(chunk 1), ... on one stream.  `chunk` groups
// per pass is what the scratch was sized for, so a call is a fixed linear chain of launches (capture-safe).
inline void launch_pbs128_multibit(hipStream_t st, uint32_t N, uint32_t glwe_dim, Pbs128MbArgs a, uint32_t chunk,
                                   const Fft128Tables &tb) {
  const uint32_t groups = a.n / a.g;
  for (uint32_t g0 = 0; g0 < groups; g0 += chunk) {
    a.group0 = g0;
    a.groups = groups - g0 < chunk ? groups - g0 : chunk;
    a.first = g0 == 0;
    a.last = g0 + a.groups == groups;
    launch_pbs128_mb_keybundle(st, N, glwe_dim, a, tb);
    pbs128_mb_dispatch(st, N, glwe_dim, &a, &tb);
  }
}

}  // namespace tfhe_hip
