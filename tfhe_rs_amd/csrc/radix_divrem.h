// radix_divrem.h — encrypted integer division (cuda/src/integer/div_rem.cuh host_unsigned_integer_div_rem, abs.cuh): the
// table-driven kernel that forms the inputs of the loop's rounds, one launch per stage, and the scratch that runs the
// bit-by-bit restoring division on the round driver.
// Included by integer.hip only, after the round driver (LutDriver), the carry propagation and the scratch protocol.
//
// Replaces, per bit of the dividend (div_rem.cuh:540-891): three phases on four sub-streams with four host synchronisations
// each, about twenty copies / block pushes / pops between "interesting" slices, and the divisor-only work the reference
// repeats in every iteration (two trimming bootstraps, the reduction "an upper block is non-zero").
#pragma once
#include "hx.h"
#include "radix_sum.h"

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace tfhe_hip {
namespace radix {

// out_g[c][first_out + r] = constant_g (body word only) + sum over the group's terms t of scalar_t * row_t(c, j), j =
// first_g + r, on u64 words modulo 2^64, rows of `words` words.  g: output group (blockIdx.z), c: integer of the batch
// (blockIdx.y), r: row of the group and the slice of kSumChunk words, both from blockIdx.x.  Every array holds its integers
// `stride` rows apart.  A term reads row j * step + offset of its array: step 1 is "row j + offset", step 0 is ONE row per
// integer for every j (broadcast).  Where j * step + offset falls below 0 the term reads its stand-in row (one row per
// integer of another array), or nothing when it has none.
// The table arrives by value in the kernel arguments, so group, source rows and scalars are workgroup-uniform and live on
// the scalar unit — no index array exists.  Rows are big_n + 1 words, an odd count, so a row is only 8-byte aligned: 8-byte
// accesses, consecutive lanes on consecutive words; the (up to) eight loads of a lane are issued before its adds and its two
// stores.  No LDS, no scratch.  No output row may overlap a row that any group reads: the launcher refuses it.
// The table is indexed by blockIdx.z, so the compiler cannot tell that the pointers it holds are kernel arguments: they are
// marked as global memory by hand (flat accesses otherwise).
constexpr uint32_t kDivGroups = 4, kDivTerms = 4;
#if defined(__HIP_DEVICE_COMPILE__)
#define DIV_GLOBAL __attribute__((address_space(1)))
#else
#define DIV_GLOBAL
#endif

struct DivTerm {
  const uint64_t *src;    // integer c starts at row c * stride
  const uint64_t *stand;  // row c * stand_stride + stand_row stands in below row 0; null: nothing does
  uint64_t scalar;
  uint32_t stride, extent;  // rows between integers; rows of an integer that exist (offsets beyond are refused)
  int32_t offset;
  uint32_t step;  // 1: row j + offset; 0: row `offset` whatever j
  uint32_t stand_stride, stand_row;
};
struct DivGroup {
  uint64_t *out;
  uint64_t constant;  // added to the body (last word) of every output row
  uint32_t stride, extent, first_out;  // of the output array
  uint32_t first, rows, terms;         // j of the group's row 0; rows per integer
  DivTerm t[kDivTerms];
};
struct DivTable {
  uint32_t words, integers, groups, slices;
  DivGroup g[kDivGroups];
};

__global__ void __launch_bounds__(kSumThreads) lwe_divrem_sum_kernel(DivTable a) {
  // all of this is uniform over the workgroup
  const DivGroup &g = a.g[blockIdx.z];
  const uint32_t r = blockIdx.x / a.slices, slice = blockIdx.x - r * a.slices, c = blockIdx.y;
  if (r >= g.rows) return;  // a group with fewer rows than the widest one of the launch
  const uint32_t first = slice * kSumChunk + threadIdx.x;
  const int64_t j = (int64_t)g.first + r;
  const DIV_GLOBAL uint64_t *ps[kDivTerms];
  uint64_t sc[kDivTerms];
  HX_UNROLL
  for (uint32_t t = 0; t < kDivTerms; ++t) {
    const DivTerm &T = g.t[t];
    const bool have = t < g.terms;
    const int64_t row = j * T.step + T.offset;
    const uint64_t *p = row >= 0 ? T.src + ((size_t)c * T.stride + (size_t)row) * a.words
                                 : (T.stand ? T.stand + ((size_t)c * T.stand_stride + T.stand_row) * a.words : nullptr);
    ps[t] = have ? (const DIV_GLOBAL uint64_t *)p : nullptr;
    sc[t] = have ? T.scalar : 0;
  }
  uint64_t v[kDivTerms][kSumWordsPerThread];
  HX_UNROLL
  for (uint32_t t = 0; t < kDivTerms; ++t) {
    HX_UNROLL
    for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
      const uint32_t e = first + u * kSumThreads;
      v[t][u] = (ps[t] && e < a.words) ? ps[t][e] : 0;
    }
  }
  DIV_GLOBAL uint64_t *po = (DIV_GLOBAL uint64_t *)(g.out + ((size_t)c * g.stride + g.first_out + r) * a.words);
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
    const uint32_t e = first + u * kSumThreads;
    uint64_t acc = e + 1 == a.words ? g.constant : 0;
    HX_UNROLL
    for (uint32_t t = 0; t < kDivTerms; ++t) acc += sc[t] * v[t][u];
    if (e < a.words) po[e] = acc;
  }
}

static DivTable div_table(uint32_t words, uint32_t integers) {
  DivTable t{};
  t.words = words, t.integers = integers, t.slices = (words + kSumChunk - 1) / kSumChunk;
  return t;
}

static void launch_divrem_sum(hipStream_t st, const DivTable &a) {
  HX_PANIC_IF_FALSE(a.words >= 1 && a.integers >= 1 && a.integers <= 65535 && a.groups >= 1 && a.groups <= kDivGroups &&
                        a.slices == (a.words + kSumChunk - 1) / kSumChunk,
                    "divrem_sum: %u words, %u integers, %u groups (at most %u)", a.words, a.integers, a.groups, kDivGroups);
  const size_t w = a.words, C = a.integers;
  uint32_t widest = 0;
  // the words a group writes and the words a term reads: `len` words from `base` for every integer, `stride` words apart
  struct Span {
    const uint64_t *base;
    size_t stride, len;
  };
  std::vector<Span> writes, reads;
  for (uint32_t g = 0; g < a.groups; ++g) {
    const DivGroup &G = a.g[g];
    HX_PANIC_IF_FALSE(G.out && G.rows >= 1 && G.terms <= kDivTerms, "divrem_sum: group %u has %u rows, %u terms (at most %u)", g,
                      G.rows, G.terms, kDivTerms);
    HX_PANIC_IF_FALSE((uint64_t)G.first_out + G.rows <= G.extent && (C == 1 || G.extent <= G.stride),
                      "divrem_sum: group %u writes rows %u .. %u of an array of %u rows per integer, %u apart", g, G.first_out,
                      G.first_out + G.rows - 1, G.extent, G.stride);
    widest = std::max(widest, G.rows);
    writes.push_back({G.out + G.first_out * w, G.stride * w, G.rows * w});
    for (uint32_t t = 0; t < G.terms; ++t) {
      const DivTerm &T = G.t[t];
      HX_PANIC_IF_FALSE(T.src && T.step <= 1, "divrem_sum: term %u of group %u: null source or step %u", t, g, T.step);
      const int64_t lo = (int64_t)G.first * T.step + T.offset, hi = (int64_t)(G.first + G.rows - 1) * T.step + T.offset;
      HX_PANIC_IF_FALSE(hi < (int64_t)T.extent && (C == 1 || T.extent <= T.stride) && (lo >= 0 || T.step == 1),
                        "divrem_sum: term %u of group %u reads rows %lld .. %lld of an array of %u rows per integer, %u apart", t,
                        g, (long long)lo, (long long)hi, T.extent, T.stride);
      const size_t l0 = (size_t)std::max<int64_t>(lo, 0);
      if (hi >= 0) reads.push_back({T.src + l0 * w, T.stride * w, ((size_t)hi + 1 - l0) * w});
      if (lo < 0 && T.stand) {
        HX_PANIC_IF_FALSE(C == 1 || T.stand_row < T.stand_stride, "divrem_sum: term %u of group %u: stand-in row %u, integers %u apart",
                          t, g, T.stand_row, T.stand_stride);
        reads.push_back({T.stand + (size_t)T.stand_row * w, T.stand_stride * w, w});
      }
    }
  }
  // two strided sets meet?  Their hulls first; inside, integer by integer of x against the integers of y next to it
  const auto meet = [C](const Span &x, const Span &y) {
    const uint64_t *xe = x.base + (C - 1) * x.stride + x.len, *ye = y.base + (C - 1) * y.stride + y.len;
    if (xe <= y.base || ye <= x.base) return false;
    for (size_t c = 0; c < C; ++c) {
      const uint64_t *lo = x.base + c * x.stride, *hi = lo + x.len;
      if (y.stride == 0 || C == 1) {
        if (lo < y.base + y.len && y.base < hi) return true;
        continue;
      }
      const int64_t k0 = lo >= y.base ? (int64_t)((size_t)(lo - y.base) / y.stride) : 0;
      for (int64_t k = std::max<int64_t>(k0 - 1, 0); k <= k0 + (int64_t)(x.len / y.stride) + 1 && k < (int64_t)C; ++k) {
        const uint64_t *ylo = y.base + (size_t)k * y.stride;
        if (lo < ylo + y.len && ylo < hi) return true;
      }
    }
    return false;
  };
  for (size_t i = 0; i < writes.size(); ++i) {
    for (const Span &s : reads)
      HX_PANIC_IF_FALSE(!meet(writes[i], s), "divrem_sum: the output of group %zu overlaps rows the launch reads", i);
    for (size_t k = i + 1; k < writes.size(); ++k)
      HX_PANIC_IF_FALSE(!meet(writes[i], writes[k]), "divrem_sum: the outputs of groups %zu and %zu overlap", i, k);
  }
  HX_PANIC_IF_FALSE((uint64_t)widest * a.slices <= 0x7fffffffu, "divrem_sum: %u rows of %u slices in one launch", widest, a.slices);
  HX_LAUNCH(lwe_divrem_sum_kernel, dim3(widest * a.slices, a.integers, a.groups), dim3(kSumThreads), 0, st, a);
}

// ------------------------------------------------------------------ the division on the round driver
// b = log2(msg) bits per block, L blocks, B = b L bits, C integers of the batch in the same rounds.  Bit-by-bit restoring
// division (tfhe/src/integer/server_key/radix_parallel/div_mod.rs unsigned_unchecked_div_rem_parallelized): iteration s =
// 0 .. B - 1 brings numerator bit i = B - 1 - s into a remainder of s + 1 significant bits, n = s / b + 1 "interesting" blocks.
// The remainder is kept as two rows sets R1 + R2 of which one is zero (the kept and the replaced remainder of the select).
//
// Once per call (the reference repeats this per iteration):
//   H1  (2 b - 1) L rows read from the divisor through the round's input index: D[j] & (2^t - 1) for t = 1 .. b - 1 (the low
//       part of a trimmed top block), (D[j] >> t) != 0 for t = 0 .. b - 1 (its high part as a flag)
//   Z   ceil(log2 L) rounds of L rows: Z[j] = a block at or above j is non-zero (suffix scan of the t = 0 flags)
//   U   (b - 1) L rows: U_t[j] = (D[j] >> t) != 0 or Z[j + 1]: "the divisor has a set bit above position j b + t - 1"; for
//       t = 0 that flag is Z[j] itself
//   one or two launches: the negated divisor with the subtraction's correcting term, - D[j] + msg - 1 (+ 1 on block 0), whole
//       blocks and every low part
// Per iteration, three launches and the rounds between them:
//   launch 1: msg R[j] + R[j - 1] for both remainders, j < n; below row 0 of R1 stands the numerator's block i / b, read
//             where the caller has it: the table of row 0 picks bit i % b of it, so no work copy of the numerator is shifted
//   round:    2 n rows, ((cur << 1) | bit) % msg  ->  S1, S2
//   launch 2: S1[j] + S2[j] (the merged remainder, j < n) and V[j] = S1[j] + S2[j] - divisor + correction over ALL L blocks:
//             whole divisor blocks below the top interesting one, its low t bits there, the propagating constant msg - 1 above
//   round:    n rows, x % msg: the clean merged remainder (the propagation's rounds are another scratch's: it cannot ride there)
//   propagation over L blocks in place on V with the output carry = 1 - borrow (one full-length scratch: the carry crosses
//             the constant blocks unchanged)
//   launch 3: f clean[j] + F, f new[j] + F and F alone, F = 1 - carry + U: the flags are ONE row per integer, broadcast
//   round:    2 n + 1 rows: F != 0 ? clean : 0  ->  R1[j];  F != 0 ? 0 : new  ->  R2[j];  (F == 0) << (i % b)  ->  bit row i
// After the loop one launch sums the b bit rows of every quotient block and R1 + R2, one round returns both to noise level 1.
// No host synchronisation, no upload and no row copy inside the loop: every index table is built with the scratch.
//
// Bootstraps per integer: (2 b - 1) L + L ceil(log2 L) + (b - 1) L + 5 b L (L + 1) / 2 + B (2 + P(L)) + 2 L, P(L) = the
// propagation's count; rounds: 1 + ceil(log2 L) + 1 + B (3 + rounds of the propagation) + 1.
//
// Signed (div_rem.cuh host_integer_div_rem, abs.cuh): the sign mask is ONE row per integer ((msg - 1) sign, what an
// arithmetic shift by B - 1 leaves in every block), broadcast: |x| = (x + mask) ^ mask on both operands in the same rounds,
// the unsigned division, then the same with the masks mask_n ^ mask_d on the quotient and mask_n on the remainder.
//
// Bounds (refused by init): the shift pair reaches msg^2 - 1 at noise level msg + 1, the select rows 3 (msg - 1) + 2 at
// noise level 5, V noise level 3, a quotient block noise level b; all at most msg carry - 1 in value and
// (msg carry - 1) / (msg - 1) in noise level.  (4, 4), (4, 16), (8, 8) pass; (2, 2) fails on the select rows.
struct DivRemCore {
  LutDriver drv;
  PropagateMem prop, prop2;  // the loop's subtraction (C integers, with the output carry); |x| and the signs (2 C integers)
  uint32_t blocks = 0, bits = 0, max_cts = 0, cached_cts = 0;
  bool is_signed = false, abs_only = false;
  struct Arr {
    size_t row0 = 0;
    uint32_t stride = 0, extent = 0;
  };
  Arr R1, R2, S1, S2, CL, V, NEGD, NEGLOW, DL, H, ZA, ZB, U, QB, FL, MN, AB, ABS2, OUT2;  // MN: the sign masks
  size_t state_rows = 0;
  uint64_t *d_state = nullptr, *d_in = nullptr;
  uint32_t in_rows = 0;
  struct Round {
    uint64_t *in = nullptr, *lut = nullptr, *out = nullptr;
    uint32_t count = 0;
  };
  Round h1, zscan, uflags;
  std::vector<Round> shift, clean, select;
  uint64_t *i_const[4] = {nullptr, nullptr, nullptr, nullptr};  // constant table indexes: MSG, SIGN, XOR, MQ
  DeviceBlocks own, shape;

  uint32_t lut_shift(uint32_t p) const { return p; }
  uint32_t lut_msg() const { return bits; }
  uint32_t lut_low(uint32_t t) const { return bits + t; }  // t = 1 .. b - 1
  uint32_t lut_high(uint32_t t) const { return 2 * bits + t; }  // t = 0 .. b - 1
  uint32_t lut_nz() const { return 3 * bits; }
  uint32_t lut_keep(uint32_t f) const { return 3 * bits + 1 + (f - 2); }
  uint32_t lut_zero(uint32_t f) const { return 3 * bits + 3 + (f - 2); }
  uint32_t lut_qbit(uint32_t pos) const { return 3 * bits + 5 + pos; }
  uint32_t lut_sign() const { return 4 * bits + 5; }
  uint32_t lut_xor() const { return 4 * bits + 6; }
  uint32_t lut_mq() const { return 4 * bits + 7; }

  static uint32_t log2_ceil(uint32_t v) {
    uint32_t k = 0;
    while ((1u << k) < v) ++k;
    return k;
  }
  // with the output carry the propagation issues one row per integer more than the count it publishes
  static uint64_t propagate_with_carry(uint32_t L) { return PropagateMem::pbs_count(L) + 1; }
  static uint64_t abs_pbs(uint32_t L) { return 1 + PropagateMem::pbs_count(L) + L; }
  static uint64_t division_pbs(bool is_signed, uint32_t L, uint32_t msg) {
    const uint64_t b = log2_ceil(msg), B = b * L;
    uint64_t n = (2 * b - 1) * L + (uint64_t)L * log2_ceil(L) + (b - 1) * L + 5 * b * L * (L + 1) / 2 +
                 B * (1 + propagate_with_carry(L)) + 2 * L;
    if (is_signed) n += 2 * abs_pbs(L) + 1 + 2 * (PropagateMem::pbs_count(L) + L);
    return n;
  }
  uint64_t issued() const { return drv.issued + prop.drv.issued + prop2.drv.issued; }

  // the bound of the loop's rows, then what the carry propagation and the four-term kernel take: msg = 4, 8 or 16
  static void check_base(const Params &p, const char *who) {
    const uint32_t space = p.msg * p.carry, cap = (space - 1) / (p.msg - 1), b = log2_ceil(p.msg);
    HX_PANIC_IF_FALSE(3 * (p.msg - 1) + 2 <= space - 1 && p.msg * p.msg - 1 <= space - 1 && 5 <= cap && p.msg + 1 <= cap && b <= cap,
                      "%s: moduli (%u, %u) do not hold the rows of the loop: values up to %u and noise levels up to %u, at most "
                      "%u and %u fit", who, p.msg, p.carry, std::max(p.msg * p.msg - 1, 3 * (p.msg - 1) + 2),
                      std::max(p.msg + 1, 5u), space - 1, cap);
    HX_PANIC_IF_FALSE((p.msg & (p.msg - 1)) == 0 && b >= 2 && b <= kDivTerms && space >= 16,
                      "%s: the message modulus %u is not 4, 8 or 16 (carry propagation takes 3 and more, a quotient block is the "
                      "sum of at most %u bit rows)", who, p.msg, kDivTerms);
  }

  // where the suffix scan ends: its rounds alternate ZA, ZB, ...  (read only when L >= 2, so at least one round ran)
  const Arr &scan_result() const { return log2_ceil(blocks) % 2 ? ZA : ZB; }
  uint64_t *ptr(const Arr &a) const { return d_state + a.row0 * ((size_t)drv.p.big_n + 1); }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t L, uint32_t cts, bool sign, bool only_abs, const char *who) {
    HX_PANIC_IF_FALSE(L >= 1 && cts >= 1 && cts <= 32767, "%s: %u blocks, %u integers", who, L, cts);
    check_base(p, who);
    blocks = L, max_cts = cts, is_signed = sign, abs_only = only_abs;
    bits = log2_ceil(p.msg);
    const uint32_t b = bits, B = b * L, K = cts;
    const uint64_t m = p.msg;
    using F = std::function<uint64_t(uint64_t)>;
    std::vector<std::vector<uint64_t>> luts(4 * b + 8, std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    const auto one = [&](uint32_t id, const F &f) { generate_lut(p, luts[id].data(), f); };
    for (uint32_t q = 0; q < b; ++q) {
      one(lut_shift(q), [m, q](uint64_t x) -> uint64_t { return (((x / m) << 1) | (((x % m) >> q) & 1)) % m; });
      one(lut_high(q), [m, q](uint64_t x) -> uint64_t { return ((x % m) >> q) != 0; });
      one(lut_qbit(q), [q](uint64_t x) -> uint64_t { return (uint64_t)(x == 0) << q; });
      if (q) one(lut_low(q), [m, q](uint64_t x) -> uint64_t { return (x % m) & ((1ull << q) - 1); });
    }
    one(lut_msg(), [m](uint64_t x) -> uint64_t { return x % m; });
    one(lut_nz(), [](uint64_t x) -> uint64_t { return x != 0; });
    for (uint64_t f = 2; f <= 3; ++f) {
      one(lut_keep((uint32_t)f), [m, f](uint64_t x) -> uint64_t { return (x % f) ? (x / f) % m : 0; });
      one(lut_zero((uint32_t)f), [m, f](uint64_t x) -> uint64_t { return (x % f) ? 0 : (x / f) % m; });
    }
    one(lut_sign(), [m, b](uint64_t x) -> uint64_t { return ((x % m) >> (b - 1)) ? m - 1 : 0; });
    one(lut_xor(), [m](uint64_t x) -> uint64_t { return ((x / m) ^ (x % m)) % m; });
    one(lut_mq(), [m](uint64_t x) -> uint64_t { return x == m - 1 ? m - 1 : 0; });
    in_rows = std::max({(2 * L + 1) * K, (2 * b - 1) * L * K, 2 * K * L, 2 * K});
    HX_PANIC_IF_FALSE((uint64_t)(2 * b + 1) * L * K <= (1u << 24), "%s: %u integers of %u blocks", who, K, L);
    drv.init(ss, p, std::min<uint32_t>(in_rows, 1u << 16), luts);
    if (!abs_only) prop.init(ss, p, L, K);
    if (is_signed) prop2.init(ss, p, L, abs_only ? K : 2 * K);
    size_t rows = 0;
    const auto arr = [&](Arr &a, uint32_t stride, uint32_t integers) {
      a.row0 = rows, a.stride = a.extent = stride, rows += (size_t)stride * integers;
    };
    arr(R1, L, K), arr(R2, L, K), arr(S1, L, K), arr(S2, L, K);  // (zeroed together at the start of a call)
    arr(CL, L, K), arr(V, L, K), arr(NEGD, L, K), arr(NEGLOW, (b - 1) * L, K), arr(DL, (b - 1) * L, K), arr(H, b * L, K);
    arr(ZA, L + 1, K), arr(ZB, L + 1, K), arr(U, (b - 1) * L, K), arr(QB, B, K), arr(FL, 1, K);
    arr(MN, 1, 3 * K), arr(AB, L, 2 * K), arr(ABS2, L, 2 * K), arr(OUT2, L, 2 * K);
    state_rows = rows;
    const size_t w = (size_t)p.big_n + 1;
    own.alloc(d_state, rows * w * sizeof(uint64_t));
    own.alloc(d_in, (size_t)in_rows * w * sizeof(uint64_t));
    const hipStream_t st = S0(ss);
    if (!t_dry) HX_CHECK(hipMemsetAsync(d_state, 0, rows * w * sizeof(uint64_t), st));  // row L of ZA / ZB stays zero
    const uint32_t ids[4] = {lut_msg(), lut_sign(), lut_xor(), lut_mq()};
    for (uint32_t i = 0; i < 4; ++i) i_const[i] = own.upload(st, std::vector<uint64_t>(2 * (size_t)K * L + 2 * K, ids[i]));
    if (!t_dry && !abs_only) build_indexes(st, K);
  }

  Round make(hipStream_t st, const std::vector<uint64_t> &in, const std::vector<uint64_t> &lut, const std::vector<uint64_t> &out) {
    Round r;
    r.in = shape.upload(st, in), r.lut = shape.upload(st, lut), r.out = shape.upload(st, out);
    r.count = (uint32_t)lut.size();
    HX_PANIC_IF_FALSE(r.count <= in_rows, "div_rem: a round of %u rows, the buffer holds %u", r.count, in_rows);
    return r;
  }

  // the rounds' index tables for C integers: they depend on (iteration, L, b, C) only.  A round's dense input rows are
  // [group][integer][row]; its output index counts rows of d_state
  void build_indexes(hipStream_t st, uint32_t C) {
    shape.release(st);  // (waits: launches of the previous shape may still read them)
    shift.clear(), clean.clear(), select.clear();
    const uint32_t L = blocks, b = bits, B = b * L;
    const auto at = [](const Arr &a, uint32_t c, uint32_t j) { return (uint64_t)(a.row0 + (size_t)c * a.stride + j); };
    std::vector<uint64_t> in, lut, out;
    for (uint32_t c = 0; c < C; ++c)
      for (uint32_t j = 0; j < L; ++j) {
        for (uint32_t t = 1; t < b; ++t) in.push_back((uint64_t)c * L + j), lut.push_back(lut_low(t)), out.push_back(at(DL, c, (t - 1) * L + j));
        for (uint32_t t = 0; t < b; ++t) in.push_back((uint64_t)c * L + j), lut.push_back(lut_high(t)), out.push_back(at(H, c, t * L + j));
      }
    h1 = make(st, in, lut, out);
    in.clear(), lut.clear(), out.clear();
    // the scan's rounds alternate between ZA and ZB: both index tables, ZA first
    for (const Arr *z : {&ZA, &ZB})
      for (uint32_t c = 0; c < C; ++c)
        for (uint32_t j = 0; j < L; ++j) lut.push_back(lut_nz()), out.push_back(at(*z, c, j));
    zscan = make(st, {}, lut, out);
    lut.clear(), out.clear();
    for (uint32_t t = 1; t < b; ++t)
      for (uint32_t c = 0; c < C; ++c)
        for (uint32_t j = 0; j < L; ++j) lut.push_back(lut_nz()), out.push_back(at(U, c, (t - 1) * L + j));
    uflags = make(st, {}, lut, out);
    for (uint32_t s = 0; s < B; ++s) {
      const uint32_t n = s / b + 1, i = B - 1 - s, pos = i % b, blk = i / b, f = s + 1 == B ? 2 : 3;
      lut.clear(), out.clear();
      for (const Arr *S : {&S1, &S2})
        for (uint32_t c = 0; c < C; ++c)
          for (uint32_t j = 0; j < n; ++j) lut.push_back(lut_shift(S == &S1 && j == 0 ? pos : b - 1)), out.push_back(at(*S, c, j));
      shift.push_back(make(st, {}, lut, out));
      lut.clear(), out.clear();
      for (uint32_t c = 0; c < C; ++c)
        for (uint32_t j = 0; j < n; ++j) lut.push_back(lut_msg()), out.push_back(at(CL, c, j));
      clean.push_back(make(st, {}, lut, out));
      lut.clear(), out.clear();
      for (uint32_t c = 0; c < C; ++c)
        for (uint32_t j = 0; j < n; ++j) lut.push_back(lut_keep(f)), out.push_back(at(R1, c, j));
      for (uint32_t c = 0; c < C; ++c)
        for (uint32_t j = 0; j < n; ++j) lut.push_back(lut_zero(f)), out.push_back(at(R2, c, j));
      for (uint32_t c = 0; c < C; ++c) lut.push_back(lut_qbit(pos)), out.push_back(at(QB, c, pos * L + blk));
      select.push_back(make(st, {}, lut, out));
    }
    cached_cts = C;
  }

  // ---- table building
  DivTerm term(const uint64_t *src, uint32_t stride, uint32_t extent, uint64_t scalar, int32_t offset = 0, uint32_t step = 1) const {
    DivTerm t{};
    t.src = src, t.stride = stride, t.extent = extent, t.scalar = scalar, t.offset = offset, t.step = step;
    return t;
  }
  // rows `base` .. of a state array; extent: the rows from there
  DivTerm term(const Arr &a, uint64_t scalar, int32_t offset = 0, uint32_t step = 1, uint32_t base = 0) const {
    return term(ptr(a) + (size_t)base * (drv.p.big_n + 1), a.stride, a.extent - base, scalar, offset, step);
  }
  static DivGroup group(uint64_t *out, uint32_t stride, uint32_t extent, uint32_t first_out, uint32_t first, uint32_t rows,
                        std::initializer_list<DivTerm> terms, uint64_t constant = 0) {
    DivGroup g{};
    g.out = out, g.stride = stride, g.extent = extent, g.first_out = first_out, g.first = first, g.rows = rows, g.constant = constant;
    for (const DivTerm &t : terms)
      if (t.src) g.t[g.terms++] = t;  // (a term without a source is left out)
    return g;
  }
  DivGroup group(const Arr &a, uint32_t first, uint32_t rows, std::initializer_list<DivTerm> terms, uint64_t constant = 0,
                 uint32_t base = 0) const {
    return group(ptr(a) + (size_t)base * (drv.p.big_n + 1), a.stride, a.extent - base, first, first, rows, terms, constant);
  }
  // dense rows of d_in from row `at` on: [integer][row]
  DivGroup dense(uint32_t at, uint32_t first, uint32_t rows, std::initializer_list<DivTerm> terms, uint64_t constant = 0) const {
    return group(d_in + (size_t)at * (drv.p.big_n + 1), rows, rows, 0, first, rows, terms, constant);
  }
  void launch(hipStream_t st, uint32_t C, const std::vector<DivGroup> &groups) const {
    for (size_t g0 = 0; g0 < groups.size(); g0 += kDivGroups) {
      DivTable t = div_table(drv.p.big_n + 1, C);
      t.groups = (uint32_t)std::min<size_t>(kDivGroups, groups.size() - g0);
      std::copy(groups.begin() + g0, groups.begin() + g0 + t.groups, t.g);
      launch_divrem_sum(st, t);
    }
  }

  // ---- the three launches of iteration s, on explicit operands (run and the bench hook share them)
  struct Stage {
    const uint64_t *num;  // the numerator's blocks, integers L rows apart
    uint32_t s, C;
  };
  DivTable stage1(const Stage &a) const {
    const uint32_t L = blocks, b = bits, n = a.s / b + 1, blk = (b * L - 1 - a.s) / b;
    DivTerm below = term(R1, 1, -1);
    below.stand = a.num, below.stand_stride = L, below.stand_row = blk;
    DivTable t = div_table(drv.p.big_n + 1, a.C);
    t.groups = 2;
    t.g[0] = dense(0, 0, n, {term(R1, drv.p.msg), below});
    t.g[1] = dense(a.C * n, 0, n, {term(R2, drv.p.msg), term(R2, 1, -1)});
    return t;
  }
  DivTable stage2(const Stage &a) const {
    const uint32_t L = blocks, b = bits, n = a.s / b + 1, t_low = (a.s + 1) % b, whole = t_low ? n - 1 : n;
    DivTable t = div_table(drv.p.big_n + 1, a.C);
    t.g[t.groups++] = dense(0, 0, n, {term(S1, 1), term(S2, 1)});
    if (whole) t.g[t.groups++] = group(V, 0, whole, {term(S1, 1), term(S2, 1), term(NEGD, 1)});
    if (t_low) t.g[t.groups++] = group(V, n - 1, 1, {term(S1, 1), term(S2, 1), term(NEGLOW, 1, 0, 1, (t_low - 1) * L)});
    if (n < L) t.g[t.groups++] = group(V, n, L - n, {}, (uint64_t)(drv.p.msg - 1) * drv.p.delta());
    return t;
  }
  DivTable stage3(const Stage &a) const {
    const uint32_t L = blocks, b = bits, B = b * L, n = a.s / b + 1, t_up = (a.s + 1) % b, j_up = (a.s + 1) / b;
    const uint64_t f = a.s + 1 == B ? 2 : 3, one = drv.p.delta();
    const DivTerm carry = term(FL, ~(uint64_t)0, 0, 0);
    DivTerm upper{};  // none in the last iteration: no bit lies above position B - 1
    if (a.s + 1 < B) upper = t_up ? term(U, 1, (int32_t)((t_up - 1) * L + j_up), 0) : term(scan_result(), 1, (int32_t)j_up, 0);
    DivTable t = div_table(drv.p.big_n + 1, a.C);
    t.groups = 3;
    t.g[0] = dense(0, 0, n, {term(CL, f), carry, upper}, one);
    t.g[1] = dense(a.C * n, 0, n, {term(V, f), carry, upper}, one);
    t.g[2] = dense(2 * a.C * n, 0, 1, {carry, upper}, one);
    return t;
  }

  // quotient and remainder of C pairs into OUT2 (quotients, then remainders, C L rows each), noise level 1
  void divide(const CudaStreamsFFI &ss, const uint64_t *num, const uint64_t *den, uint32_t C, void *const *ksks, void *const *bsks) {
    const Params &p = drv.p;
    const hipStream_t st = S0(ss);
    const uint32_t L = blocks, b = bits, B = b * L;
    const size_t w = (size_t)p.big_n + 1;
    const uint64_t delta = p.delta(), neg = ~(uint64_t)0;
    if (cached_cts != C) build_indexes(st, C);
    if (prop.cached_cts != C) prop.build_indexes(st, C);
    HX_CHECK(hipMemsetAsync(ptr(R1), 0, (size_t)4 * max_cts * L * w * sizeof(uint64_t), st));
    // once per call: the divisor's masks and flags
    drv.round(ss, d_state, h1.out, den, h1.in, h1.lut, h1.count, ksks, bsks);
    const uint32_t scans = log2_ceil(L);
    for (uint32_t k = 0; k < scans; ++k) {
      const uint32_t d = 1u << k;
      const auto from = [&](int32_t offset) { return k == 0 ? term(H, 1, offset) : term(k % 2 ? ZA : ZB, 1, offset); };
      DivGroup lo = group(d_in, L, L, 0, 0, L - d, {from(0), from((int32_t)d)}), hi = group(d_in, L, L, L - d, L - d, d, {from(0)});
      if (k == 0) lo.t[0].extent = lo.t[1].extent = hi.t[0].extent = L;  // the t = 0 flags are the first L rows of H
      launch(st, C, {lo, hi});
      drv.round(ss, d_state, zscan.out + (k % 2 ? (size_t)C * L : 0), d_in, nullptr, zscan.lut, C * L, ksks, bsks);
    }
    const Arr &Z = scan_result();
    {
      std::vector<DivGroup> g;
      for (uint32_t t = 1; t < b; ++t)
        g.push_back(group(d_in + (size_t)(t - 1) * C * L * w, L, L, 0, 0, L,
                          {term(H, 1, 0, 1, t * L), scans ? term(Z, 1, 1) : DivTerm{}}));
      for (DivGroup &x : g) x.t[0].extent = L;
      launch(st, C, g);
      drv.round(ss, d_state, uflags.out, d_in, nullptr, uflags.lut, uflags.count, ksks, bsks);
      g.clear();
      const uint64_t c1 = (uint64_t)(p.msg - 1) * delta, c0 = c1 + delta;
      const DivTerm d0 = term(den, L, L, neg);
      g.push_back(group(NEGD, 0, 1, {d0}, c0));
      if (L > 1) g.push_back(group(NEGD, 1, L - 1, {d0}, c1));
      for (uint32_t t = 1; t < b; ++t) {
        const DivTerm low = term(DL, neg, 0, 1, (t - 1) * L);
        g.push_back(group(NEGLOW, 0, 1, {low}, c0, (t - 1) * L));
        if (L > 1) g.push_back(group(NEGLOW, 1, L - 1, {low}, c1, (t - 1) * L));
      }
      launch(st, C, g);
    }
    for (uint32_t s = 0; s < B; ++s) {
      const uint32_t n = s / b + 1;
      HX_RANGE("div_rem iteration %u of %u: %u integers, %u blocks", s + 1, B, C, n);
      const Stage a{num, s, C};
      launch_divrem_sum(st, stage1(a));
      drv.round(ss, d_state, shift[s].out, d_in, nullptr, shift[s].lut, shift[s].count, ksks, bsks);
      launch_divrem_sum(st, stage2(a));
      drv.round(ss, d_state, clean[s].out, d_in, nullptr, clean[s].lut, clean[s].count, ksks, bsks);
      prop.run(ss, ptr(V), C, ksks, bsks, nullptr, ptr(FL), nullptr, true);
      launch_divrem_sum(st, stage3(a));
      drv.round(ss, d_state, select[s].out, d_in, nullptr, select[s].lut, select[s].count, ksks, bsks);
    }
    std::vector<DivGroup> g(2);
    g[0] = dense(0, 0, L, {});
    for (uint32_t q = 0; q < b; ++q) g[0].t[g[0].terms++] = term(QB, 1, (int32_t)(q * L));
    g[1] = dense(C * L, 0, L, {term(R1, 1), term(R2, 1)});
    launch(st, C, g);
    drv.round(ss, ptr(OUT2), nullptr, d_in, nullptr, i_const[0], 2 * C * L, ksks, bsks);
  }

  // ---- signs.  The masks of a call are rows of MN: mask i of integer c at row i C + c
  Arr mask(uint32_t i, uint32_t C) const { return Arr{MN.row0 + (size_t)i * C, 1, 1}; }
  using Operand = std::pair<const uint64_t *, Arr>;  // blocks (integers L rows apart) and the mask that goes with them
  // mask[c] <- (msg - 1) * sign of integer c, for every operand in ONE round; the masks are consecutive from xs[0]'s on
  void sign_masks(const CudaStreamsFFI &ss, const std::vector<Operand> &xs, uint32_t C, void *const *ksks, void *const *bsks) {
    const uint32_t L = blocks;
    std::vector<DivGroup> g;
    for (size_t i = 0; i < xs.size(); ++i) g.push_back(dense((uint32_t)i * C, 0, 1, {term(xs[i].first, L, L, 1, (int32_t)(L - 1), 0)}));
    launch(S0(ss), C, g);
    drv.round(ss, ptr(xs[0].second), nullptr, d_in, nullptr, i_const[1], (uint32_t)xs.size() * C, ksks, bsks);
  }
  // out <- (x + mask) ^ mask for the integers of every operand, all in the same rounds; out: xs.size() * C * L dense rows
  void negate_where(const CudaStreamsFFI &ss, const std::vector<Operand> &xs, uint64_t *out, uint32_t C, void *const *ksks,
                    void *const *bsks) {
    const uint32_t L = blocks, count = (uint32_t)xs.size();
    const size_t w = (size_t)drv.p.big_n + 1;
    const hipStream_t st = S0(ss);
    std::vector<DivGroup> g;
    for (uint32_t i = 0; i < count; ++i)
      g.push_back(group(ptr(AB) + (size_t)i * C * L * w, L, L, 0, 0, L, {term(xs[i].first, L, L, 1), term(xs[i].second, 1, 0, 0)}));
    launch(st, C, g);
    if (prop2.cached_cts != count * C) prop2.build_indexes(st, count * C);
    prop2.run(ss, ptr(AB), count * C, ksks, bsks);
    g.clear();
    for (uint32_t i = 0; i < count; ++i)
      g.push_back(dense(i * C * L, 0, L, {term(ptr(AB) + (size_t)i * C * L * w, L, L, drv.p.msg), term(xs[i].second, 1, 0, 0)}));
    launch(st, C, g);
    drv.round(ss, out, nullptr, d_in, nullptr, i_const[2], count * C * L, ksks, bsks);
  }

  void abs_inplace(const CudaStreamsFFI &ss, uint64_t *v, uint32_t C, void *const *ksks, void *const *bsks) {
    sign_masks(ss, {{v, mask(0, C)}}, C, ksks, bsks);
    negate_where(ss, {{v, mask(0, C)}}, v, C, ksks, bsks);
  }

  // the whole call; the results are in OUT2
  void div_rem(const CudaStreamsFFI &ss, const uint64_t *num, const uint64_t *den, uint32_t C, void *const *ksks, void *const *bsks) {
    const uint32_t L = blocks;
    const size_t w = (size_t)drv.p.big_n + 1;
    if (!is_signed) return divide(ss, num, den, C, ksks, bsks);
    const Arr mn = mask(0, C), md = mask(1, C), mq = mask(2, C);
    sign_masks(ss, {{num, mn}, {den, md}}, C, ksks, bsks);
    negate_where(ss, {{num, mn}, {den, md}}, ptr(ABS2), C, ksks, bsks);
    divide(ss, ptr(ABS2), ptr(ABS2) + (size_t)C * L * w, C, ksks, bsks);
    // the quotient's mask: the signs differ
    launch(S0(ss), C, {dense(0, 0, 1, {term(mn, 1, 0, 0), term(md, 1, 0, 0)})});
    drv.round(ss, ptr(mq), nullptr, d_in, nullptr, i_const[3], C, ksks, bsks);
    // ABS2 is free again: the negation reads OUT2 and cannot write it in the same launch
    const uint64_t *q = ptr(OUT2), *r = q + (size_t)C * L * w;
    negate_where(ss, {{q, mq}, {r, mn}}, ptr(ABS2), C, ksks, bsks);
    HX_CHECK(hipMemcpyAsync(ptr(OUT2), ptr(ABS2), (size_t)2 * C * L * w * sizeof(uint64_t), hipMemcpyDeviceToDevice, S0(ss)));
  }

  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    prop.release(ss);
    prop2.release(ss);
    shape.release(S0(ss));
    own.release(S0(ss));
  }
};

struct DivRemMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x44495631;  // "DIV1"
  DivRemCore core;
  void release(const CudaStreamsFFI &ss) { core.release(ss); }
};
struct AbsMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x41425331;  // "ABS1"
  DivRemCore core;
  void release(const CudaStreamsFFI &ss) { core.release(ss); }
};

}  // namespace radix
}  // namespace tfhe_hip
