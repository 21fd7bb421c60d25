// radix_bitcount.h — encrypted bit counts (cuda/src/integer/ilog2.cuh, cuda/include/integer/ilog2.h; tfhe-rs
// integer/server_key/radix_parallel/ilog2.rs and count_zeros_ones.rs): the kernel that packs two rows of an integer into
// one bootstrap input, and the scratch that runs leading / trailing runs, ilog2 and the popcounts on the round driver.
// Included by integer.hip only, after the round driver (LutDriver), the carry propagation and the column sums.
//
// Replaces, per call of ilog2.cuh: a copy of the operand into a work buffer, a round "run inside every block", a block
// reversal for Leading, ceil(log2 L) Hillis-Steele rounds that each copy and pack, L slice copies into a mostly-zero
// counter_num_blocks x L vector — and for ilog2 two more table rounds, a second partial sum and a block-by-block full
// propagation (ilog2.cuh:149-199).
#pragma once
#include "hx.h"
#include "radix_sum.h"

#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

namespace tfhe_hip {
namespace radix {

// out[c outs + g] = s0 x[c x_stride + first + g step] + s1 x[c x_stride + first + g step + delta], on u64 words modulo
// 2^64.  c: integer of the batch (blockIdx.z), g: output row (blockIdx.x), outs = ceil(rows / step) of them per integer,
// blockIdx.y: slice of kSumChunk words.  The integer's rows are first .. first + rows - 1 of its x_stride rows; a partner
// g step + delta outside 0 .. rows - 1 contributes nothing.  step 1: every row with its neighbour at distance delta (a scan
// step); step 2, delta 1: the pairs (0, 1), (2, 3), ... and the last row of an odd count alone (the popcount round).
// Both source rows depend on blockIdx only: they are workgroup-uniform, computed on the scalar unit, and no index table
// exists.  Rows are big_n + 1 words, an odd count, so a row is only 8-byte aligned: 8-byte accesses, consecutive lanes on
// consecutive words; the four loads of a lane are issued before its adds and its two stores.  No LDS, no scratch.
// `x` may be the caller's memory, read in place; `out` is dense and must not overlap the rows read (a row is read by another
// workgroup than the one that writes it): the launcher refuses it.
struct PairPack {
  uint64_t *out;
  const uint64_t *x;
  uint64_t s0, s1;
  uint32_t words, x_stride, first, rows, step;
  int32_t delta;
  uint32_t outs;  // ceil(rows / step): set by the launcher
};

__global__ void __launch_bounds__(kSumThreads) lwe_pair_pack_kernel(PairPack a) {
  const uint32_t g = blockIdx.x, c = blockIdx.z, first = blockIdx.y * kSumChunk + threadIdx.x;
  // all of this is uniform over the workgroup
  const uint32_t j = g * a.step;
  const int64_t k = (int64_t)j + a.delta;
  const bool have = k >= 0 && k < (int64_t)a.rows;
  const uint64_t *base = a.x + ((size_t)c * a.x_stride + a.first) * a.words;
  const uint64_t *px = base + (size_t)j * a.words;
  const uint64_t *pp = base + (size_t)(have ? k : j) * a.words;
  uint64_t vx[kSumWordsPerThread], vp[kSumWordsPerThread];
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
    const uint32_t e = first + u * kSumThreads;
    const bool in = e < a.words;
    vx[u] = in ? px[e] : 0;
    vp[u] = (in && have) ? pp[e] : 0;
  }
  uint64_t *po = a.out + ((size_t)c * a.outs + g) * a.words;
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
    const uint32_t e = first + u * kSumThreads;
    if (e < a.words) po[e] = a.s0 * vx[u] + a.s1 * vp[u];
  }
}

static uint32_t pair_pack_outs(uint32_t rows, uint32_t step) { return (rows + step - 1) / step; }

static void launch_pair_pack(hipStream_t st, PairPack a, uint32_t batch) {
  HX_PANIC_IF_FALSE(a.out && a.x && a.words >= 1 && a.rows >= 1 && batch >= 1, "pair_pack: null pointer or empty operand");
  HX_PANIC_IF_FALSE(a.step == 1 || a.step == 2, "pair_pack: step %u is neither 1 nor 2", a.step);
  HX_PANIC_IF_FALSE(a.delta != 0 && (a.delta < 0 ? (int64_t)0 - a.delta : (int64_t)a.delta) < (int64_t)a.rows,
                    "pair_pack: distance %d on %u rows", a.delta, a.rows);
  HX_PANIC_IF_FALSE(batch <= 65535, "pair_pack: %u integers in one launch", batch);
  HX_PANIC_IF_FALSE(batch == 1 || (uint64_t)a.first + a.rows <= a.x_stride,
                    "pair_pack: rows %u .. %u of integers %u rows apart", a.first, a.first + a.rows - 1, a.x_stride);
  const uint32_t outs = a.outs = pair_pack_outs(a.rows, a.step);
  const uint64_t *lo = a.x + (size_t)a.first * a.words;
  const uint64_t *hi = lo + ((size_t)(batch - 1) * a.x_stride + a.rows) * a.words;
  const uint64_t *oe = a.out + (size_t)batch * outs * a.words;
  HX_PANIC_IF_FALSE(oe <= lo || hi <= a.out, "pair_pack: the output overlaps the rows it reads");
  HX_LAUNCH(lwe_pair_pack_kernel, dim3(outs, (a.words + kSumChunk - 1) / kSumChunk, batch), dim3(kSumThreads), 0, st, a);
}

// ------------------------------------------------------------------ the counts on the round driver
// b = log2(msg) bits per block, L blocks, B = b L bits, C integers of the batch in the same rounds.  The result is an unsigned
// integer of `counter` blocks: ceil((floor(log2 B) + 1) / b) for the runs and the popcounts (ilog2.rs:32-33),
// ceil((floor(log2(B - 1)) + 2) / b) for ilog2 (ilog2.rs:166-167).
//
// Runs (leading / trailing zeros / ones).  run(x): the run inside a block, counted from the integer's end (0 .. b).  With
// the neighbour i + d (Leading) or i - d (Trailing) the scan keeps  t[i] = run(x[i]) if every block between i and the end
// within the window is a full run, else 0:
//   round 1:  t[i] = run(x[nb]) == b ? run(x[i]) : 0 on msg x[nb] + x[i], read from the operand where the caller has it; the
//             block without a neighbour takes run(x[i]) in the same round
//   round k:  t[i] = t[nb] == b ? t[i] : 0 on msg t[nb] + t[i], d = 2^(k - 1), only for the rows that have a neighbour, in place
// ceil(log2 L) rounds (one for L = 1), L + sum over d = 2, 4, .. < L of (L - d) bootstraps; the count is the sum of the
// t[i], L single-block terms of degree b in column 0, which the column sums read where the scan left them.
// ilog2 = B - 1 - leading_zeros = sum (b - t[i]) - 1 modulo 2^(b counter): b - t[i] is linear (degree b), the - 1 is the
// all-ones integer (a body constant on the first term, a trivial term in every other column); zero yields all ones, as in
// the reference.
// Popcounts: one round over ceil(L / 2) rows msg x[2 g + 1] + x[2 g] returns the count over 2 b bits (degree 2 b); the last
// block of an odd L goes alone.
// Then one plan of column sums (final degree 2 msg - 2 at most) and one carry propagation over `counter` blocks.
//
// Bounds: a packed row reaches msg^2 - 1 at noise level msg + 1, both at most msg carry - 1 and (msg carry - 1) / (msg - 1)
// exactly when carry >= msg (make_params).  Refused by init: what the carry propagation and the column sums refuse
// (message modulus below 3, fewer than 16 values per block), a message modulus that is not a power of two.
enum : uint32_t { kBitCountRuns = 0, kBitCountIlog2 = 1, kBitCountPop = 2 };

struct BitCountCore {
  LutDriver drv;  // LUTs: 0 message, 1 carry, 2 a row with its neighbour, 3 a row alone, 4 a scan step
  PropagateMem prop;
  ColumnSum cs;
  uint32_t kind = 0, blocks = 0, counter = 0, max_cts = 0, bits = 0, terms = 0, cached_cts = 0;
  bool leading = false, ones = false;
  uint64_t *d_state = nullptr, *d_in = nullptr;  // C x terms results of the scan / the pair round; a round's packed rows
  struct Round {
    uint64_t *in = nullptr, *lut = nullptr, *out = nullptr;
    uint32_t count = 0;
  };
  Round first;
  std::vector<Round> scan;  // the steps d = 2, 4, ...
  DeviceBlocks own, shape;
  enum : uint64_t { TAB_MSG = 0, TAB_CARRY = 1, TAB_PAIR = 2, TAB_LONE = 3, TAB_SCAN = 4, TAB_COUNT = 5 };

  static uint32_t log2_floor(uint32_t v) {
    uint32_t k = 0;
    while ((2u << k) <= v) ++k;
    return k;
  }
  static uint32_t log2_ceil(uint32_t v) {
    uint32_t k = 0;
    while ((1u << k) < v) ++k;
    return k;
  }
  static uint32_t counter_blocks(uint32_t which, uint32_t L, uint32_t b) {
    const uint32_t B = b * L;
    const uint32_t need = which == kBitCountIlog2 ? (B > 1 ? log2_floor(B - 1) : 0) + 2 : log2_floor(B) + 1;
    return (need + b - 1) / b;
  }
  static uint32_t term_count(uint32_t which, uint32_t L) { return which == kBitCountPop ? (L + 1) / 2 : L; }
  // bootstraps and rounds before the column sums
  static uint64_t first_stage_pbs(uint32_t which, uint32_t L) {
    if (which == kBitCountPop) return (L + 1) / 2;
    uint64_t n = L;
    for (uint32_t d = 2; d < L; d *= 2) n += L - d;
    return n;
  }
  static uint32_t first_stage_rounds(uint32_t which, uint32_t L) {
    return which == kBitCountPop ? 1 : std::max(1u, log2_ceil(L));
  }
  // the plan of the sum: term ids 0 .. terms - 1 are the rows of d_state (the column sums' caller rows).  ilog2 adds the
  // all-ones integer: block 0 of it as a body constant on term 0 (whose degree it raises by msg - 1: one term fewer in the
  // column every term lies in, which saves a round of the sum at 32 blocks of two bits), the blocks 1 .. counter - 1 as the
  // trivial terms terms .. terms + counter - 2 (the first rows of the pool)
  static SumPlan make_plan(uint32_t which, uint32_t L, uint32_t msg, uint32_t carry, std::vector<uint32_t> &deg) {
    const uint32_t b = log2_ceil(msg), T = term_count(which, L), nc = counter_blocks(which, L, b);
    std::vector<std::vector<uint64_t>> cols(nc);
    deg.clear();
    for (uint32_t i = 0; i < T; ++i) {
      deg.push_back(which == kBitCountPop && 2 * i + 1 < L ? 2 * b : b);
      cols[0].push_back(i);
    }
    if (which == kBitCountIlog2) {
      deg[0] += msg - 1;
      for (uint32_t j = 1; j < nc; ++j) deg.push_back(msg - 1), cols[j].push_back(T + j - 1);
    }
    return plan_column_sums(std::move(cols), deg, msg, carry, false, 2 * msg - 2);
  }
  static uint32_t propagate_rounds(uint32_t L) {
    if (L == 1) return 1;
    const uint32_t top = (uint32_t)PropagateMem::level_sizes(L).size() - 1;
    return 3 + top + (top ? top - 1 : 0);
  }
  static uint64_t pbs_count(uint32_t which, uint32_t L, uint32_t msg, uint32_t carry) {
    std::vector<uint32_t> deg;
    const SumPlan pl = make_plan(which, L, msg, carry, deg);
    return first_stage_pbs(which, L) + pl.bootstraps() + PropagateMem::pbs_count(counter_blocks(which, L, log2_ceil(msg)));
  }
  static uint32_t round_count(uint32_t which, uint32_t L, uint32_t msg, uint32_t carry) {
    std::vector<uint32_t> deg;
    const SumPlan pl = make_plan(which, L, msg, carry, deg);
    return first_stage_rounds(which, L) + (uint32_t)pl.steps.size() + propagate_rounds(counter_blocks(which, L, log2_ceil(msg)));
  }
  static void check_base(uint32_t msg, uint32_t carry, const char *who) {
    HX_PANIC_IF_FALSE(msg >= 3 && msg * carry >= 16,
                      "%s: moduli (%u, %u): the carry propagation and the column sums take a message modulus of 3 and more and "
                      "16 values per block", who, msg, carry);
    HX_PANIC_IF_FALSE((msg & (msg - 1)) == 0, "%s: the message modulus %u is not a power of two", who, msg);
  }
  uint64_t issued() const { return drv.issued + prop.drv.issued; }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t which, uint32_t L, uint32_t counter_num_blocks, uint32_t cts,
            bool is_leading, bool count_ones, const char *who) {
    HX_PANIC_IF_FALSE(L >= 1 && cts >= 1 && cts <= 65535 && (uint64_t)L * cts <= (1u << 24), "%s: %u blocks, %u integers", who, L, cts);
    check_base(p.msg, p.carry, who);
    kind = which, blocks = L, max_cts = cts, leading = is_leading, ones = count_ones;
    bits = log2_ceil(p.msg);
    counter = counter_blocks(which, L, bits);
    HX_PANIC_IF_FALSE(counter_num_blocks == counter, "%s: counter_num_blocks is %u, %u blocks of %u bits take %u", who,
                      counter_num_blocks, L, bits, counter);
    terms = term_count(which, L);
    const uint64_t m = p.msg, b = bits;
    const bool lead = leading, one = ones;
    // the run inside a block from the integer's end; the count over the bits of x below 2^n
    const auto run = [b, lead, one](uint64_t x) -> uint64_t {
      uint64_t n = 0;
      for (uint64_t i = 0; i < b; ++i) {
        if (((x >> (lead ? b - 1 - i : i)) & 1) != (uint64_t)one) break;
        ++n;
      }
      return n;
    };
    const auto pop = [one](uint64_t x, uint64_t n) -> uint64_t {
      uint64_t k = 0;
      for (uint64_t i = 0; i < n; ++i) k += ((x >> i) & 1) == (uint64_t)one;
      return k;
    };
    std::vector<std::vector<uint64_t>> luts(TAB_COUNT, std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    generate_lut(p, luts[TAB_MSG].data(), [m](uint64_t x) -> uint64_t { return x % m; });
    generate_lut(p, luts[TAB_CARRY].data(), [m](uint64_t x) -> uint64_t { return x / m; });
    if (kind == kBitCountPop) {
      generate_lut(p, luts[TAB_PAIR].data(), [pop, b, m](uint64_t x) -> uint64_t { return pop(x % (m * m), 2 * b); });
      generate_lut(p, luts[TAB_LONE].data(), [pop, b, m](uint64_t x) -> uint64_t { return pop(x % m, b); });
    } else {
      generate_lut(p, luts[TAB_PAIR].data(), [run, b, m](uint64_t x) -> uint64_t { return run((x / m) % m) == b ? run(x % m) : 0; });
      generate_lut(p, luts[TAB_LONE].data(), [run, m](uint64_t x) -> uint64_t { return run(x % m); });
    }
    generate_lut(p, luts[TAB_SCAN].data(), [b, m](uint64_t x) -> uint64_t { return x / m == b ? x % m : 0; });
    drv.init(ss, p, (uint32_t)std::min<uint64_t>((uint64_t)cts * std::max(L, 2 * counter), 1u << 16), luts);
    prop.init(ss, p, counter, cts);
    std::vector<uint32_t> deg;
    SumPlan pl = make_plan(kind, L, p.msg, p.carry, deg);
    const uint32_t extra = kind == kBitCountIlog2 ? counter - 1 : 0;
    cs.set_plan(std::move(pl), counter, terms, terms, deg.size());
    const size_t w = (size_t)p.big_n + 1;
    const hipStream_t st = S0(ss);
    cs.reserve(st, cts, w);  // for the whole capacity: the pool never moves, its first rows hold the all-ones blocks
    own.alloc(d_state, (size_t)cts * terms * w * sizeof(uint64_t));
    own.alloc(d_in, (size_t)cts * L * w * sizeof(uint64_t));
    if (t_dry) return;
    if (extra) {
      HX_CHECK(hipMemsetAsync(cs.d_pool, 0, cs.pool_rows * w * sizeof(uint64_t), st));
      const uint64_t all = (m - 1) * p.delta();
      for (uint32_t c = 0; c < cts; ++c) {
        uint64_t *rows = cs.d_pool + (size_t)c * cs.slots * w;
        HX_LAUNCH(lwe_negate_const_kernel, dim3(extra), dim3(256), 0, st, rows, rows, (uint32_t)w, extra, 1u, all, all);
      }
    }
    build_indexes(st, cts);
  }

  Round make(hipStream_t st, const std::vector<uint64_t> &in, const std::vector<uint64_t> &lut, const std::vector<uint64_t> &out) {
    Round r;
    r.in = shape.upload(st, in), r.lut = shape.upload(st, lut), r.out = shape.upload(st, out);
    r.count = (uint32_t)lut.size();
    return r;
  }
  int32_t towards(uint32_t d) const { return leading ? (int32_t)d : -(int32_t)d; }
  bool has_neighbour(uint32_t i, uint32_t d) const { return leading ? i + d < blocks : i >= d; }

  // the rounds' index tables for C integers.  A round's dense input rows are [integer][row]; the outputs are rows of d_state
  void build_indexes(hipStream_t st, uint32_t C) {
    shape.release(st);  // (waits: launches of the previous shape may still read them)
    scan.clear();
    const uint32_t L = blocks, T = terms;
    std::vector<uint64_t> in, lut, out;
    for (uint32_t c = 0; c < C; ++c)
      for (uint32_t g = 0; g < T; ++g) {
        const bool paired = kind == kBitCountPop ? 2 * g + 1 < L : has_neighbour(g, 1);
        lut.push_back(paired ? TAB_PAIR : TAB_LONE), out.push_back((uint64_t)c * T + g);
      }
    first = make(st, {}, lut, out);
    if (kind != kBitCountPop)
      for (uint32_t d = 2; d < L; d *= 2) {
        in.clear(), lut.clear(), out.clear();
        for (uint32_t c = 0; c < C; ++c)
          for (uint32_t i = 0; i < L; ++i)
            if (has_neighbour(i, d)) in.push_back((uint64_t)c * L + i), lut.push_back(TAB_SCAN), out.push_back((uint64_t)c * T + i);
        scan.push_back(make(st, in, lut, out));
      }
    cs.upload(st, C, TAB_MSG, TAB_CARRY);
    cached_cts = C;
  }

  // the launch that packs a scan step or the pair round into d_in: x[i] + msg x[partner], integers L rows apart in x (the
  // operand, or d_state, which holds L rows per integer whenever a scan runs)
  PairPack pack(const uint64_t *x, uint32_t step, int32_t delta) const {
    return PairPack{d_in, x, 1, drv.p.msg, drv.p.big_n + 1, blocks, 0, blocks, step, delta, 0};
  }

  // out <- the count of every one of the C integers of x (L blocks each): `counter` blocks each, degree msg - 1, noise level 1
  void run(const CudaStreamsFFI &ss, uint64_t *out, const uint64_t *x, uint32_t C, void *const *ksks, void *const *bsks) {
    const Params &p = drv.p;
    const hipStream_t st = S0(ss);
    const uint32_t L = blocks, T = terms, w = p.big_n + 1;
    if (cached_cts != C) build_indexes(st, C);
    HX_RANGE("bit count (kind %u): %u integers of %u blocks", kind, C, L);
    if (L == 1) {
      drv.round(ss, d_state, first.out, x, nullptr, first.lut, C, ksks, bsks);
    } else {
      launch_pair_pack(st, kind == kBitCountPop ? pack(x, 2, 1) : pack(x, 1, towards(1)), C);
      drv.round(ss, d_state, first.out, d_in, nullptr, first.lut, C * T, ksks, bsks);
    }
    uint32_t d = 2;
    for (const Round &r : scan) {
      launch_pair_pack(st, pack(d_state, 1, towards(d)), C);
      drv.round(ss, d_state, r.out, d_in, r.in, r.lut, r.count, ksks, bsks);
      d *= 2;
    }
    if (kind == kBitCountIlog2) {
      const uint64_t c1 = (uint64_t)bits * p.delta(), c0 = c1 + (uint64_t)(p.msg - 1) * p.delta();  // b - t[i]; + msg - 1 on term 0
      HX_LAUNCH(lwe_negate_const_kernel, dim3(C * T), dim3(256), 0, st, d_state, d_state, w, C * T, T, c0, c1);
    }
    cs.reduce(ss, drv, d_state, w, ksks, bsks);
    cs.finish(st, out, d_state, w, true);  // (`out` is not d_state: no group's output is a row another group reads)
    prop.run(ss, out, C, ksks, bsks);
  }

  void release(const CudaStreamsFFI &ss) {
    cs.release(S0(ss));
    drv.release(ss);
    prop.release(ss);
    shape.release(S0(ss));
    own.release(S0(ss));
  }
};

struct ConsecutiveBitsMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x42435231;  // "BCR1"
  BitCountCore core;
  void release(const CudaStreamsFFI &ss) { core.release(ss); }
};
struct Ilog2Mem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x494C4732;  // "ILG2"
  BitCountCore core;
  void release(const CudaStreamsFFI &ss) { core.release(ss); }
};
struct CountOnesMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x504F5031;  // "POP1"
  BitCountCore core;
  void release(const CudaStreamsFFI &ss) { core.release(ss); }
};

}  // namespace radix
}  // namespace tfhe_hip
