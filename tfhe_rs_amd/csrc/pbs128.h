// pbs128.h — the programmable bootstrap over the 128-bit torus (noise squashing): double-double ("f128") arithmetic,
// the negacyclic f128 transform, its host-built tables, key conversion, the one-launch bootstrap and their launchers.
//
// Restated: tfhe-fft/src/fft128/f128_ops.rs (arithmetic), tfhe/src/core_crypto/fft_impl/fft128/math/fft/mod.rs
// (torus <-> f128 conversions), fft128/crypto/{ggsw,bootstrap}.rs and the reference GPU backend's
// pbs/programmable_bootstrap_classic_128.cuh (algorithm).  The transform itself is this library's merged-twist tree of
// DESIGN.md §4 with two doubles per component; the key's order inside its buffer is this library's own.
//
// A header and not a .hip file: the host emulation build lists its translation units by name; this file is included by
// abi.hip alone.  Every error-free product is an explicit fma(); both builds compile with -ffp-contract=off, so the
// device and the emulation compute the same words.
#pragma once
#include "pbs_common.h"
#include "arena.h"

#include <map>
#include <mutex>
#include <vector>

namespace tfhe_hip {

typedef unsigned __int128 u128;
typedef __int128 i128;

// ------------------------------------------------------------------------------------------------ f128 arithmetic
struct f128 {
  double hi, lo;
};
struct c128 {
  f128 re, im;
};
HX_DEV void two_sum(double a, double b, double &s, double &e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
HX_DEV void two_diff(double a, double b, double &s, double &e) {
  s = a - b;
  const double bb = s - a;
  e = (a - (s - bb)) - (b + bb);
}
HX_DEV void quick_two_sum(double a, double b, double &s, double &e) {
  s = a + b;
  e = b - (s - a);
}
HX_DEV void two_prod(double a, double b, double &p, double &e) {
  p = a * b;
  e = fma(a, b, -p);
}
// f128_ops.rs: add_f128_f128 / sub_f128_f128 (the operators of the multiply-accumulate)
HX_DEV f128 f128_add(f128 a, f128 b) {
  double s1, s2, t1, t2;
  two_sum(a.hi, b.hi, s1, s2);
  two_sum(a.lo, b.lo, t1, t2);
  s2 = s2 + t1;
  quick_two_sum(s1, s2, s1, s2);
  s2 = s2 + t2;
  quick_two_sum(s1, s2, s1, s2);
  return f128{s1, s2};
}
HX_DEV f128 f128_sub(f128 a, f128 b) {
  double s1, s2, t1, t2;
  two_diff(a.hi, b.hi, s1, s2);
  two_diff(a.lo, b.lo, t1, t2);
  s2 = s2 + t1;
  quick_two_sum(s1, s2, s1, s2);
  s2 = s2 + t2;
  quick_two_sum(s1, s2, s1, s2);
  return f128{s1, s2};
}
// add_estimate_f128_f128 / sub_estimate_f128_f128 (the butterflies of the transform, fft128/mod.rs)
HX_DEV f128 f128_add_est(f128 a, f128 b) {
  double s, e;
  two_sum(a.hi, b.hi, s, e);
  e = e + (a.lo + b.lo);
  quick_two_sum(s, e, s, e);
  return f128{s, e};
}
HX_DEV f128 f128_sub_est(f128 a, f128 b) {
  double s, e;
  two_diff(a.hi, b.hi, s, e);
  e = e + a.lo;
  e = e - b.lo;
  quick_two_sum(s, e, s, e);
  return f128{s, e};
}
HX_DEV f128 f128_add_f64(f128 a, double b) {  // add_f128_f64
  double s1, s2;
  two_sum(a.hi, b, s1, s2);
  s2 = s2 + a.lo;
  quick_two_sum(s1, s2, s1, s2);
  return f128{s1, s2};
}
HX_DEV f128 f128_mul(f128 a, f128 b) {  // mul_f128_f128
  double p1, p2;
  two_prod(a.hi, b.hi, p1, p2);
  p2 = p2 + (a.hi * b.lo + a.lo * b.hi);
  quick_two_sum(p1, p2, p1, p2);
  return f128{p1, p2};
}
// x * y and acc + x * y of the external product (ggsw.rs:623-676: accurate additions)
HX_DEV c128 c128_mul(c128 x, c128 y) {
  return c128{f128_sub(f128_mul(x.re, y.re), f128_mul(x.im, y.im)), f128_add(f128_mul(x.im, y.re), f128_mul(x.re, y.im))};
}
HX_DEV c128 c128_mul_add(c128 x, c128 y, c128 acc) {
  const c128 p = c128_mul(x, y);
  return c128{f128_add(acc.re, p.re), f128_add(acc.im, p.im)};
}
// transform butterfly: (a, b) -> (a + s b, a - s b), estimate additions
HX_DEV void bfly128(c128 &a, c128 &b, const c128 s) {
  const f128 tr = f128_sub_est(f128_mul(b.re, s.re), f128_mul(b.im, s.im));
  const f128 ti = f128_add_est(f128_mul(b.re, s.im), f128_mul(b.im, s.re));
  const c128 o1{f128_add_est(a.re, tr), f128_add_est(a.im, ti)};
  b = c128{f128_sub_est(a.re, tr), f128_sub_est(a.im, ti)};
  a = o1;
}

// ------------------------------------------------------------------------------------------------ conversions
HX_DEV double f64_from_bits(uint64_t u) {
  double d;
  __builtin_memcpy(&d, &u, 8);
  return d;
}
// math/fft/mod.rs:104-125: u128 / i128 -> nearest f64 (ties to even), without a 128-bit conversion instruction
HX_DEV double u128_to_f64(u128 x) {
  const uint64_t A = 0x4330000000000000ull, B = 0x4670000000000000ull, C = 0x44B0000000000000ull, D = 0x47F0000000000000ull;
  if (x < ((u128)1 << 104)) {
    const double l = f64_from_bits(A | (((uint64_t)(x << 12)) >> 12)) - f64_from_bits(A);
    const double h = f64_from_bits(B | (uint64_t)(x >> 52)) - f64_from_bits(B);
    return l + h;
  }
  const double l = f64_from_bits(C | (((uint64_t)(x >> 12)) >> 12) | ((uint64_t)x & 0xFFFFFFull)) - f64_from_bits(C);
  const double h = f64_from_bits(D | (uint64_t)(x >> 76)) - f64_from_bits(D);
  return l + h;
}
HX_DEV double i128_to_f64(i128 x) {
  const uint64_t sign = ((uint64_t)((u128)x >> 64)) & (1ull << 63);
  const u128 a = x < 0 ? (u128)0 - (u128)x : (u128)x;
  return f64_from_bits(f64_bits(u128_to_f64(a)) | sign);
}
// :128-164: truncating f64 -> u128 / i128
HX_DEV u128 f64_to_u128(double f) {
  const uint64_t b = f64_bits(f);
  if (b < (1023ull << 52)) return 0;
  const u128 m = ((u128)1 << 127) | ((u128)b << 75);
  const uint64_t s = 1150ull - (b >> 52);
  return s >= 128 ? (u128)0 : m >> s;
}
HX_DEV i128 f64_to_i128(double f) {
  const uint64_t b = f64_bits(f), a = b & ~(1ull << 63);
  if (a < (1023ull << 52)) return 0;
  const u128 m = ((u128)1 << 127) | ((u128)a << 75);
  const uint64_t s = 1150ull - (a >> 52);
  const i128 u = (i128)(s >= 128 ? (u128)0 : m >> s);
  return (int64_t)b < 0 ? -u : u;
}
// :167-189: the word read as a signed integer, as an f128 (hi = nearest f64, lo = nearest f64 of what is left)
HX_DEV f128 u128_to_signed_f128(u128 x) {
  const double first = i128_to_f64((i128)x);
  const u128 back = f64_to_u128(fabs(first));
  const u128 back_signed = (f64_bits(first) >> 63) ? (u128)0 - back : back;
  return f128{first, i128_to_f64((i128)(x - back_signed))};
}
HX_DEV f128 f128_floor(f128 x) {  // :88-96
  const double f = floor(x.hi);
  if (f == x.hi) {
    double s, e;
    two_sum(f, floor(x.lo), s, e);
    return f128{s, e};
  }
  return f128{f, 0.0};
}
// :192-205: torus value (a real, taken modulo 1) -> u128
HX_DEV u128 f128_to_torus_u128(f128 x) {
  x = f128_sub_est(x, f128_floor(x));
  x.hi *= 340282366920938463463374607431768211456.0;  // 2^128
  x.lo *= 340282366920938463463374607431768211456.0;
  x = f128_floor(f128_add_f64(x, 0.5));
  return f64_to_u128(x.hi) + (u128)f64_to_i128(x.lo);
}

// ------------------------------------------------------------------------------------------------ u128 decomposer
// cc/commons/math/decomposition/decomposer.rs:156-185 and iter.rs:122-151 on 128-bit words; base_log <= 64,
// base_log * level <= 128 (with all 128 bits represented the closest representable is the word itself)
HX_DEV u128 decomp_init_state128(u128 x, uint32_t base_log, uint32_t level) {
  const uint32_t rep = base_log * level;
  if (rep >= 128) return x;
  u128 res = x >> (128 - rep - 1);
  const u128 rounding_bit = res & 1;
  res += 1;
  res >>= 1;
  res &= ~(u128)0 >> (128 - rep);
  const u128 need_balance = (((res - 1) | (rounding_bit << (rep - 1))) & res) >> (rep - 1);
  return res - (need_balance << rep);
}
HX_DEV i128 decompose_one_level128(uint32_t base_log, u128 &state) {
  const u128 res = state & (((u128)1 << base_log) - 1);
  state = (u128)((i128)state >> base_log);
  const u128 carry = (((res - 1) | state) & res) >> (base_log - 1);
  state += carry;
  return (i128)(res - (carry << base_log));
}
// a digit "as integer" (convert_forward_integer): below 2^31 in magnitude it is one exact double
template <int BL>
HX_DEV f128 digit_to_f128(i128 d, uint32_t base_log) {
  if (BL != 0 ? BL <= 31 : base_log <= 31) return f128{(double)(int32_t)d, 0.0};
  return u128_to_signed_f128((u128)d);
}

// ------------------------------------------------------------------------------------------------ tables
// Same shape as FftTables (tables.h) with four doubles per entry: re_hi, re_lo, im_hi, im_lo.
struct Fft128Tables {
  const double *fwd;
  const double *inv;
  const double *untw;
};

namespace f128_tables {
// Q2.126 fixed point on unsigned 128-bit words: sine and cosine of pi m / M by their Taylor series after an exact
// reduction to the first octant.  Every step errs by at most 2^-126, some 30 steps: far inside the 2^-106 of the
// double-double the value is rounded to, also relative to the smallest sine of the tables (pi / 4096).
inline u128 mulq(u128 a, u128 b) {  // (a b) >> 126, a b < 2^254
  const uint64_t a0 = (uint64_t)a, a1 = (uint64_t)(a >> 64), b0 = (uint64_t)b, b1 = (uint64_t)(b >> 64);
  const u128 p00 = (u128)a0 * b0, p01 = (u128)a0 * b1, p10 = (u128)a1 * b0, p11 = (u128)a1 * b1;
  const u128 mid = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;
  const u128 hi = p11 + (p01 >> 64) + (p10 >> 64) + (mid >> 64);
  const u128 lo = (mid << 64) | (uint64_t)p00;
  return (hi << 2) | (lo >> 126);
}
inline void q_to_dd(u128 v, double scale, double *hi, double *lo) {
  const double h = (double)v;  // nearest
  const i128 rest = (i128)v - (i128)(u128)h;
  *hi = h * scale;
  *lo = (double)rest * scale;
}
// (cos, sin)(pi m / M) as double-doubles; M a power of two, any integer m
inline void cis(int64_t m, int64_t M, double *out4) {
  while (M < 4) m *= 2, M *= 2;
  m &= 2 * M - 1;
  bool neg_c = false, neg_s = false, swap = false;
  if (m >= M) m -= M, neg_c = !neg_c, neg_s = !neg_s;   // half turn
  if (m > M / 2) m = M - m, neg_c = !neg_c;             // reflection about pi / 2
  if (m > M / 4) m = M / 2 - m, swap = true;            // reflection about pi / 4
  const u128 PI = ((u128)0xC90FDAA22168C234ull << 64) | 0xC4C6628B80DC1CD1ull;  // pi 2^126
  int log_m = 0;
  while (((int64_t)1 << log_m) < M) ++log_m;
  const u128 x = (PI >> log_m) * (u128)m, x2 = mulq(x, x);
  u128 sp = 0, sn = 0, cp = (u128)1 << 126, cn = 0, ts = x, tc = (u128)1 << 126;
  sp = x;
  for (int k = 1; k < 24; ++k) {
    tc = mulq(tc, x2) / (u128)((2 * k - 1) * (2 * k));
    ts = mulq(ts, x2) / (u128)((2 * k) * (2 * k + 1));
    if (k & 1) cn += tc, sn += ts; else cp += tc, sp += ts;
  }
  u128 c = cp - cn, s = sp - sn;
  if (swap) { const u128 t = c; c = s; s = t; }
  const double scale = 1.1754943508222875e-38;  // 2^-126
  q_to_dd(c, neg_c ? -scale : scale, out4 + 0, out4 + 1);
  q_to_dd(s, neg_s ? -scale : scale, out4 + 2, out4 + 3);
}
inline uint32_t bitrev(uint32_t x, uint32_t bits) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < bits; ++i) r = (r << 1) | (x & 1), x >>= 1;
  return r;
}
}  // namespace f128_tables

// fwd, inv, untw: 4 * (N / 2) doubles each, indexed as tables.h says for the f64 transform
inline void fill_fft128_tables_host(uint32_t N, double *fwd, double *inv, double *untw) {
  using namespace f128_tables;
  const uint32_t n = N / 2;
  uint32_t D = 0;
  while ((1u << D) < n) ++D;
  for (int c = 0; c < 4; ++c) fwd[c] = inv[c] = 0.0;
  for (uint32_t d = 0; d < D; ++d)
    for (uint32_t g = 0; g < (1u << d); ++g)
      cis(1 + 4 * (int64_t)bitrev(g, d), (int64_t)1 << (d + 2), fwd + 4 * (size_t)((1u << d) + g));
  for (uint32_t half = 1; half < n; half *= 2)
    for (uint32_t j = 0; j < half; ++j) cis(-(int64_t)j, half, inv + 4 * (size_t)(half + j));
  for (uint32_t j = 0; j < n; ++j) {
    double *u = untw + 4 * (size_t)j;
    cis(-(int64_t)j, N, u);
    for (int c = 0; c < 4; ++c) u[c] /= (double)n;  // a power of two: exact
  }
}

struct Fft128Entry {
  double *fwd, *inv, *untw;
};
inline std::mutex g_fft128_mu;
inline std::map<std::pair<uint32_t, uint32_t>, Fft128Entry> g_fft128;
inline Fft128Tables get_fft128_tables(uint32_t gpu_index, uint32_t N) {
  std::lock_guard<std::mutex> lk(g_fft128_mu);
  const auto key = std::make_pair(gpu_index, N);
  auto it = g_fft128.find(key);
  if (it == g_fft128.end()) {
    const size_t bytes = sizeof(double) * 2 * N;
    std::vector<double> fwd(2 * N), inv(2 * N), untw(2 * N);
    fill_fft128_tables_host(N, fwd.data(), inv.data(), untw.data());
    Fft128Entry e;
    HX_CHECK(hipSetDevice((int)gpu_index));
    HX_CHECK(hipMalloc((void **)&e.fwd, bytes));
    HX_CHECK(hipMalloc((void **)&e.inv, bytes));
    HX_CHECK(hipMalloc((void **)&e.untw, bytes));
    HX_CHECK(hipMemcpy(e.fwd, fwd.data(), bytes, hipMemcpyHostToDevice));
    HX_CHECK(hipMemcpy(e.inv, inv.data(), bytes, hipMemcpyHostToDevice));
    HX_CHECK(hipMemcpy(e.untw, untw.data(), bytes, hipMemcpyHostToDevice));
    it = g_fft128.emplace(key, e).first;
  }
  return Fft128Tables{it->second.fwd, it->second.inv, it->second.untw};
}

// ------------------------------------------------------------------------------------------------ LDS transform
// n = N / 2 complex f128 points as four planes of doubles (re_hi, re_lo, im_hi, im_lo), one spare slot after every 16
struct F128Buf {
  double *p;
  int stride;  // doubles per plane
  HX_DEV static int at(int q) { return q + (q >> 4); }
  HX_DEV c128 get(int q) const {
    const int s = at(q);
    return c128{f128{p[s], p[stride + s]}, f128{p[2 * stride + s], p[3 * stride + s]}};
  }
  HX_DEV void put(int q, const c128 v) const {
    const int s = at(q);
    p[s] = v.re.hi;
    p[stride + s] = v.re.lo;
    p[2 * stride + s] = v.im.hi;
    p[3 * stride + s] = v.im.lo;
  }
};
constexpr int f128buf_stride(int N) { return N / 2 + N / 32; }
constexpr size_t f128buf_bytes(int N) { return (size_t)4 * f128buf_stride(N) * sizeof(double); }
template <int N> struct Cfg128 {
  static constexpr int TPB = N / 8 < 256 ? N / 8 : 256;  // one radix-4 unit of a pass per thread up to N = 2048
};
HX_DEV c128 tw128(const double *__restrict__ t, int idx) {
  return c128{f128{t[4 * idx], t[4 * idx + 1]}, f128{t[4 * idx + 2], t[4 * idx + 3]}};
}
// forward: the merged-twist tree of lds_fft_forward (pbs_common.h), two radix-2 stages per barrier
template <int N, int TPB>
HX_DEV void lds_fft128_forward(const F128Buf buf, const double *__restrict__ fwd, int tid) {
  constexpr int n = N / 2;
  int m = n, cnt = 1;
  for (; m >= 4; m >>= 2, cnt <<= 2) {
    const int quarter = m >> 2;
    for (int u = tid; u < n / 4; u += TPB) {
      const int g = u / quarter, j = u - g * quarter;
      const int p0 = g * m + j, p1 = p0 + quarter, p2 = p1 + quarter, p3 = p2 + quarter;
      const c128 wa = tw128(fwd, cnt + g), wb0 = tw128(fwd, 2 * cnt + 2 * g), wb1 = tw128(fwd, 2 * cnt + 2 * g + 1);
      c128 x0 = buf.get(p0), x1 = buf.get(p1), x2 = buf.get(p2), x3 = buf.get(p3);
      bfly128(x0, x2, wa);
      bfly128(x1, x3, wa);
      bfly128(x0, x1, wb0);
      bfly128(x2, x3, wb1);
      buf.put(p0, x0);
      buf.put(p1, x1);
      buf.put(p2, x2);
      buf.put(p3, x3);
    }
    __syncthreads();
  }
  if (m == 2) {
    for (int b = tid; b < n / 2; b += TPB) {
      c128 x = buf.get(2 * b), y = buf.get(2 * b + 1);
      bfly128(x, y, tw128(fwd, cnt + b));
      buf.put(2 * b, x);
      buf.put(2 * b + 1, y);
    }
    __syncthreads();
  }
}
// one radix-2 stage of the backward transform; half = 1 (and j = 0 of half = 2) multiply by 1, j = 1 of half = 2 by -i
HX_DEV void inv_bfly128(c128 &x, c128 &y, int half, int j, const double *__restrict__ inv) {
  if (half == 1 || (half == 2 && j == 0)) {
    const c128 o1{f128_add_est(x.re, y.re), f128_add_est(x.im, y.im)}, o2{f128_sub_est(x.re, y.re), f128_sub_est(x.im, y.im)};
    x = o1;
    y = o2;
  } else if (half == 2) {
    const c128 o1{f128_add_est(x.re, y.im), f128_sub_est(x.im, y.re)}, o2{f128_sub_est(x.re, y.im), f128_add_est(x.im, y.re)};
    x = o1;
    y = o2;
  } else {
    bfly128(x, y, tw128(inv, half + j));
  }
}
template <int N, int TPB>
HX_DEV void lds_fft128_inverse(const F128Buf buf, const double *__restrict__ inv, int tid) {
  constexpr int n = N / 2;
  int half = 1;
  for (; 4 * half <= n; half <<= 2) {
    for (int u = tid; u < n / 4; u += TPB) {
      const int q = u / half, j = u - q * half;
      const int p0 = q * 4 * half + j, p1 = p0 + half, p2 = p1 + half, p3 = p2 + half;
      c128 x0 = buf.get(p0), x1 = buf.get(p1), x2 = buf.get(p2), x3 = buf.get(p3);
      inv_bfly128(x0, x1, half, j, inv);
      inv_bfly128(x2, x3, half, j, inv);
      inv_bfly128(x0, x2, 2 * half, j, inv);
      inv_bfly128(x1, x3, 2 * half, j + half, inv);
      buf.put(p0, x0);
      buf.put(p1, x1);
      buf.put(p2, x2);
      buf.put(p3, x3);
    }
    __syncthreads();
  }
  if (2 * half <= n) {
    for (int b = tid; b < n / 2; b += TPB) {
      c128 x = buf.get(b), y = buf.get(b + half);
      inv_bfly128(x, y, half, b, inv);
      buf.put(b, x);
      buf.put(b + half, y);
    }
    __syncthreads();
  }
}
// point j after the backward transform, untwisted and scaled by 1 / n: (coefficient j, coefficient j + n) as reals
HX_DEV c128 untwist128(const c128 y, const double *__restrict__ untw, int j) {
  const c128 u = tw128(untw, j);
  return c128{f128_sub_est(f128_mul(y.re, u.re), f128_mul(y.im, u.im)), f128_add_est(f128_mul(y.im, u.re), f128_mul(y.re, u.im))};
}

// ------------------------------------------------------------------------------------------------ transform kernels
// mode 0: forward "as torus" (words scaled by 2^-128), 1: forward "as integer"; one workgroup per polynomial.
// Output: planes re0, re1, im0, im1 of n doubles per polynomial — or, planar != 0, the four planes of a polynomial
// next to each other at re0 + polynomial * 4 n (the bootstrap key's layout).
template <int N>
__global__ void __launch_bounds__(Cfg128<N>::TPB) fft128_forward_kernel(double *re0, double *re1, double *im0, double *im1,
                                                                      const u128 *standard, Fft128Tables tb, int mode,
                                                                      int planar) {
  constexpr int n = N / 2, TPB = Cfg128<N>::TPB;
  HX_DYN_SMEM(smem);
  const F128Buf buf{(double *)smem, f128buf_stride(N)};
  const int tid = threadIdx.x;
  const u128 *p = standard + (size_t)blockIdx.x * N;
  const double scale = mode == 0 ? 2.938735877055718769921841343055614194546826e-39 : 1.0;  // 2^-128
  for (int j = tid; j < n; j += TPB) {
    const f128 a = u128_to_signed_f128(p[j]), b = u128_to_signed_f128(p[j + n]);
    buf.put(j, c128{f128{a.hi * scale, a.lo * scale}, f128{b.hi * scale, b.lo * scale}});
  }
  __syncthreads();
  lds_fft128_forward<N, TPB>(buf, tb.fwd, tid);
  const size_t base = (size_t)blockIdx.x * n;
  double *o0 = planar ? re0 + 4 * base : re0 + base, *o1 = planar ? o0 + n : re1 + base;
  double *o2 = planar ? o0 + 2 * n : im0 + base, *o3 = planar ? o0 + 3 * n : im1 + base;
  for (int j = tid; j < n; j += TPB) {
    const c128 v = buf.get(j);
    o0[j] = v.re.hi;
    o1[j] = v.re.lo;
    o2[j] = v.im.hi;
    o3[j] = v.im.lo;
  }
}
template <int N>
__global__ void __launch_bounds__(Cfg128<N>::TPB) fft128_backward_kernel(u128 *standard, const double *re0, const double *re1,
                                                                       const double *im0, const double *im1,
                                                                       Fft128Tables tb) {
  constexpr int n = N / 2, TPB = Cfg128<N>::TPB;
  HX_DYN_SMEM(smem);
  const F128Buf buf{(double *)smem, f128buf_stride(N)};
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * n;
  for (int j = tid; j < n; j += TPB)
    buf.put(j, c128{f128{re0[base + j], re1[base + j]}, f128{im0[base + j], im1[base + j]}});
  __syncthreads();
  lds_fft128_inverse<N, TPB>(buf, tb.inv, tid);
  u128 *o = standard + (size_t)blockIdx.x * N;
  for (int j = tid; j < n; j += TPB) {
    const c128 t = untwist128(buf.get(j), tb.untw, j);
    o[j] = f128_to_torus_u128(t.re);
    o[j + n] = f128_to_torus_u128(t.im);
  }
}

// ------------------------------------------------------------------------------------------------ the bootstrap
struct Pbs128Args {
  u128 *lwe_out;           // num_samples LWEs of k N + 1 words
  const u128 *lut;         // one GLWE, (k + 1) N words
  const uint64_t *lwe_in;  // num_samples LWEs of n + 1 u64 words
  const double *bsk;       // [n][level][k + 1][k + 1] polynomials of four planes of N / 2 doubles
  u128 *acc_scratch;       // ACC_GLOBAL instantiations: (k + 1) N words per sample in device memory
  uint32_t n, base_log, level, num_samples, ms_type;
};
HX_DEV u128 rot_sub128(const u128 *poly, uint32_t j, uint32_t a_hat, uint32_t N) {
  bool neg;
  const uint32_t src = monomial_mul_src(j, a_hat, N, neg);
  const u128 s = poly[src];
  return (neg ? (u128)0 - s : s) - poly[j];
}
// One launch for the whole blind rotation, one workgroup per input LWE, no synchronisation between workgroups
// (the shape of pbs_fft_generic_kernel).  BL, LV: the decomposition as template constants (0, 0: read from the
// arguments).  ACC_GLOBAL: the accumulator does not fit in LDS next to the transform buffer and lives in a per-sample
// device buffer that only this workgroup touches.
template <int N, int K1, int BL, int LV, bool ACC_GLOBAL>
__global__ void __launch_bounds__(Cfg128<N>::TPB) pbs128_kernel(Pbs128Args a, Fft128Tables tb) {
  constexpr int n = N / 2, TPB = Cfg128<N>::TPB, PER = n / TPB, LOG2N2 = ilog2_c(2 * N);
  HX_DYN_SMEM(smem);
  const int tid = threadIdx.x;
  const uint32_t sample = blockIdx.x;
  u128 *acc = ACC_GLOBAL ? a.acc_scratch + (size_t)sample * K1 * N : (u128 *)smem;
  const F128Buf buf{(double *)(smem + (ACC_GLOBAL ? 0 : (size_t)K1 * N * 16)), f128buf_stride(N)};
  const uint64_t *lwe = a.lwe_in + (size_t)sample * (a.n + 1);
  const uint32_t base_log = BL ? (uint32_t)BL : a.base_log, level = LV ? (uint32_t)LV : a.level;

  const uint32_t b_hat = block_body_modulus_switch<TPB>(lwe, a.n, LOG2N2, a.ms_type, (uint64_t *)buf.p, tid);
  for (int p = 0; p < K1; ++p)
    for (uint32_t j = tid; j < (uint32_t)N; j += TPB) {  // acc <- LUT * X^{-b_hat}
      bool neg;
      const uint32_t src = monomial_div_src(j, b_hat, N, neg);
      const u128 v = a.lut[p * N + src];
      acc[p * N + j] = neg ? (u128)0 - v : v;
    }
  __syncthreads();

  for (uint32_t i = 0; i < a.n; ++i) {
    const uint32_t a_hat = (uint32_t)modulus_switch(lwe[i], LOG2N2);
    if (a_hat == 0) continue;  // uniform across the workgroup: X^0 ACC - ACC = 0 adds nothing
    c128 facc[K1][PER];
    bool first = true;
    HX_NO_UNROLL
    for (int row = 0; row < K1; ++row) {
      // closest representable of ACC X^a_hat - ACC for my 2 PER coefficients of this row; the digits come off it level
      // by level, least significant first (key index 0 holds the last level)
      u128 state[2 * PER];
      HX_UNROLL
      for (int q = 0; q < PER; ++q) {
        const uint32_t j = tid + q * TPB;
        state[2 * q] = decomp_init_state128(rot_sub128(acc + row * N, j, a_hat, N), base_log, level);
        state[2 * q + 1] = decomp_init_state128(rot_sub128(acc + row * N, j + n, a_hat, N), base_log, level);
      }
      HX_NO_UNROLL
      for (uint32_t idx = 0; idx < level; ++idx) {
        HX_UNROLL
        for (int q = 0; q < PER; ++q)
          buf.put(tid + q * TPB, c128{digit_to_f128<BL>(decompose_one_level128(base_log, state[2 * q]), base_log),
                                      digit_to_f128<BL>(decompose_one_level128(base_log, state[2 * q + 1]), base_log)});
        __syncthreads();
        lds_fft128_forward<N, TPB>(buf, tb.fwd, tid);
        const double *brow = a.bsk + ((((size_t)i * level + idx) * K1 + row) * K1) * (4 * n);
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
        acc[c * N + j] += f128_to_torus_u128(t.re);
        acc[c * N + j + n] += f128_to_torus_u128(t.im);
      }
      __syncthreads();
    }
  }
  // sample extraction of coefficient 0 (cc/algorithms/glwe_sample_extraction.rs:119-146)
  constexpr int k = K1 - 1;
  u128 *out = a.lwe_out + (size_t)sample * ((size_t)k * N + 1);
  for (int p = 0; p < k; ++p)
    for (uint32_t j = tid; j < (uint32_t)N; j += TPB) out[(size_t)p * N + j] = j == 0 ? acc[p * N] : (u128)0 - acc[p * N + N - j];
  if (tid == 0) out[(size_t)k * N] = acc[k * N];
}

// ------------------------------------------------------------------------------------------------ launchers
constexpr size_t kPbs128LdsLimit = 160 * 1024;
constexpr bool pbs128_acc_global(int N, int K1) { return (size_t)K1 * N * 16 + f128buf_bytes(N) > kPbs128LdsLimit; }
inline bool pbs128_needs_acc_scratch(uint32_t N, uint32_t glwe_dim) { return pbs128_acc_global((int)N, (int)glwe_dim + 1); }

template <int N, int K1, int BL, int LV>
static void launch_pbs128_inst(hipStream_t st, const Pbs128Args &a, const Fft128Tables &tb) {
  constexpr bool G = pbs128_acc_global(N, K1);
  const size_t smem = (G ? 0 : (size_t)K1 * N * 16) + f128buf_bytes(N);
  if (G) HX_PANIC_IF_FALSE(a.acc_scratch != nullptr, "128-bit PBS: this scratch has no accumulator buffer");
  hx_set_dynamic_smem_once<pbs128_kernel<N, K1, BL, LV, G>>(smem);
  HX_LAUNCH((pbs128_kernel<N, K1, BL, LV, G>), dim3(a.num_samples), dim3(Cfg128<N>::TPB), smem, st, a, tb);
}
template <int N, int K1>
static void launch_pbs128_nk(hipStream_t st, const Pbs128Args &a, const Fft128Tables &tb) {
  // the noise-squashing set of PARAM_MESSAGE_2_CARRY_2 (k = 2, N = 2048, 3 levels of 24 bits) is a fixed instantiation
  if constexpr (N == 2048 && K1 == 3) {
    if (a.base_log == 24 && a.level == 3) return launch_pbs128_inst<N, K1, 24, 3>(st, a, tb);
  }
  launch_pbs128_inst<N, K1, 0, 0>(st, a, tb);
}
// The one list of supported (polynomial_size, glwe_dimension) pairs.  a == nullptr: only answers whether the pair is
// supported; otherwise launches on it (and panics on an unsupported pair).
inline bool pbs128_dispatch(hipStream_t st, uint32_t N, uint32_t glwe_dim, const Pbs128Args *a, const Fft128Tables *tb) {
#define HX_PBS128_CASE(N_, K1_)                                 \
  if (N == N_ && glwe_dim + 1 == K1_) {                         \
    if (a != nullptr) launch_pbs128_nk<N_, K1_>(st, *a, *tb);   \
    return true;                                                \
  }
  HX_PBS128_CASE(256, 2) HX_PBS128_CASE(256, 3) HX_PBS128_CASE(256, 4)
  HX_PBS128_CASE(512, 2) HX_PBS128_CASE(512, 3) HX_PBS128_CASE(512, 4)
  HX_PBS128_CASE(1024, 2) HX_PBS128_CASE(1024, 3) HX_PBS128_CASE(1024, 4)
  HX_PBS128_CASE(2048, 2) HX_PBS128_CASE(2048, 3)
  HX_PBS128_CASE(4096, 2)
#undef HX_PBS128_CASE
  if (a != nullptr) HX_PANIC("unsupported (polynomial_size=%u, glwe_dimension=%u) for the 128-bit PBS", N, glwe_dim);
  return false;
}
inline bool pbs128_supported(uint32_t N, uint32_t glwe_dim) { return pbs128_dispatch(nullptr, N, glwe_dim, nullptr, nullptr); }
inline void launch_pbs128(hipStream_t st, uint32_t N, uint32_t glwe_dim, const Pbs128Args &a, const Fft128Tables &tb) {
  pbs128_dispatch(st, N, glwe_dim, &a, &tb);
}
// the sizes the f128 transform exists for: one refusal, one message, for every entry point
inline void pbs128_check_poly(uint32_t N) {
  HX_PANIC_IF_FALSE(N >= 256 && N <= 4096 && (N & (N - 1)) == 0,
                    "polynomial_size %u not supported by the 128-bit PBS (256..4096, power of two)", N);
}

template <int N>
static void launch_fft128_forward_n(hipStream_t st, double *re0, double *re1, double *im0, double *im1, const u128 *standard,
                                    size_t polys, const Fft128Tables &tb, int mode, int planar) {
  if (f128buf_bytes(N) > 48 * 1024) hx_set_dynamic_smem_once<fft128_forward_kernel<N>>(f128buf_bytes(N));
  HX_LAUNCH((fft128_forward_kernel<N>), dim3((unsigned)polys), dim3(Cfg128<N>::TPB), f128buf_bytes(N), st, re0, re1, im0, im1,
            standard, tb, mode, planar);
}
template <int N>
static void launch_fft128_backward_n(hipStream_t st, u128 *standard, const double *re0, const double *re1, const double *im0,
                                     const double *im1, size_t polys, const Fft128Tables &tb) {
  if (f128buf_bytes(N) > 48 * 1024) hx_set_dynamic_smem_once<fft128_backward_kernel<N>>(f128buf_bytes(N));
  HX_LAUNCH((fft128_backward_kernel<N>), dim3((unsigned)polys), dim3(Cfg128<N>::TPB), f128buf_bytes(N), st, standard, re0, re1,
            im0, im1, tb);
}
#define HX_DISPATCH_N128(FN, ...)                                                              \
  switch (N) {                                                                                 \
    case 256: FN<256>(__VA_ARGS__); break;                                                     \
    case 512: FN<512>(__VA_ARGS__); break;                                                     \
    case 1024: FN<1024>(__VA_ARGS__); break;                                                   \
    case 2048: FN<2048>(__VA_ARGS__); break;                                                   \
    case 4096: FN<4096>(__VA_ARGS__); break;                                                   \
    default: pbs128_check_poly(N);                                                             \
  }
inline void launch_fft128_forward(hipStream_t st, uint32_t N, double *re0, double *re1, double *im0, double *im1,
                                  const u128 *standard, size_t polys, const Fft128Tables &tb, int mode, int planar) {
  if (polys == 0) return;
  HX_DISPATCH_N128(launch_fft128_forward_n, st, re0, re1, im0, im1, standard, polys, tb, mode, planar);
}
inline void launch_fft128_backward(hipStream_t st, uint32_t N, u128 *standard, const double *re0, const double *re1,
                                   const double *im0, const double *im1, size_t polys, const Fft128Tables &tb) {
  if (polys == 0) return;
  HX_DISPATCH_N128(launch_fft128_backward_n, st, standard, re0, re1, im0, im1, polys, tb);
}

// ------------------------------------------------------------------------------------------------ test hooks
// digits of count words, level per word, least significant first, as i128
__global__ void test_decompose128_kernel(const u128 *in, i128 *out, uint32_t count, uint32_t base_log, uint32_t level) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  u128 st = decomp_init_state128(in[i], base_log, level);
  for (uint32_t idx = 0; idx < level; ++idx) out[(size_t)i * level + idx] = decompose_one_level128(base_log, st);
}
// out = a * b pointwise; each operand four planes of count doubles (re_hi, re_lo, im_hi, im_lo)
__global__ void test_f128_cmul_kernel(double *out, const double *x, const double *y, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const c128 r = c128_mul(c128{f128{x[i], x[count + i]}, f128{x[2 * count + i], x[3 * count + i]}},
                          c128{f128{y[i], y[count + i]}, f128{y[2 * count + i], y[3 * count + i]}});
  out[i] = r.re.hi;
  out[count + i] = r.re.lo;
  out[2 * count + i] = r.im.hi;
  out[3 * count + i] = r.im.lo;
}

}  // namespace tfhe_hip
