// radix_aes.h — AES-128 transciphering (cuda/src/aes/aes.cuh, include/aes/aes.h): the gate-sum kernel, the host-side
// scheduler that turns the cipher into levelled rounds, and the scratch that runs counter addition, cipher rounds and key
// schedule on the round driver.  Included by integer.hip only, after the round driver (LutDriver) and the scratch protocol.
//
// Replaces, in the reference: the flush after (almost) every XOR of the S-box circuit (aes.cuh:371-571, 34 sequential
// launches per S-box pass), the gather / scatter copies around every S-box pass and every batched flush or AND, the tiled
// copy and the transpose of a round key per AddRoundKey (aes.cuh:865-878, 958-972), the per-column copies of MixColumns and
// the 128-step ripple of the counter addition (aes.cuh:994-1076).  Here a wire stays a lazy sum of fresh bits until a gate
// needs a clean bit or the sum would leave the block; one launch of one kernel forms every input row of a round from a
// program built once by the scratch call; ShiftRows / RotWord are lane maps inside the terms, MixColumns / AddRoundKey /
// Rcon / NOT fold into the sums; the counter addition is a prefix scan of 9 rounds.
#pragma once
#include "hx.h"
#include "radix_sum.h"
#include "radix_trivium.h"  // TAP_GLOBAL

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

namespace tfhe_hip {
namespace radix {

// ------------------------------------------------------------------ the gate-sum kernel
// out[(g L + l) N + n] = sum over the terms t of group g of scalar_t * src_t[row_t(l, n)] on u64 words modulo 2^64, rows of
// `words` words, plus (constant_g + sum of the group's clear terms) * delta on the body word (the last one).
// g: group of the launch, l: lane of the launch (0 .. L - 1, the state's byte lane lane0 + l), n: input; all three from
// blockIdx.x; blockIdx.y: slice of kSumChunk words.
//   row_t(l, n) = row0 + lane_t(l) * lane_stride + (broadcast ? 0 : n)
//   lane_t(l)   = l                                  for a term on the lanes of the launch (wires that exist per pass)
//               = map(lane0 + l)                     for a term on the lanes of the state:
//                   identity; a permutation out of `maps` (ShiftRows, RotWord, composed with MixColumns' offsets);
//                   an offset within the column of four lanes, (lane & ~3) | ((lane + k) & 3)
// A source is a row of one of three bases — the scratch's wires, and two of the caller's ciphertexts read in place (round
// keys and IV) — or, for a clear term, entry n * clear_stride + row0 of the call's clear input (the counter bits), which
// only moves the body.  Groups and terms are a CSR the scratch call uploaded once; a launch copies nothing.
// Group, term list, source rows and scalars depend on blockIdx only: they are read once per workgroup through the scalar
// unit.  The lists are indexed by values the compiler cannot trace to kernel arguments, so the pointers are marked as global
// memory by hand (flat accesses otherwise; see radix_trivium.h).  Rows are big_n + 1 words, an odd count, so a row is only
// 8-byte aligned: 8-byte accesses, consecutive lanes on consecutive words; a lane issues the loads of up to kSumInFlight
// terms for its two words before it adds, a longer list loops.  No LDS, no scratch memory, no spills; 40 VGPRs on gfx950.
// No output row may overlap a row that any group of the launch reads: the launcher refuses it.
constexpr uint32_t kGateLanes = 16;  // byte lanes of an AES state; a permutation table holds this many entries
enum : uint32_t { kGateWires = 0, kGateCallerA = 1, kGateCallerB = 2, kGateClear = 3 };  // base of a term
enum : uint32_t { kMapIdentity = 0, kMapPerm = 1, kMapColumn = 2 };                      // map = kind | parameter << 2
enum : uint32_t { kGateBroadcast = 1, kGateStateLane = 2 };                              // flags of a term

struct GateTerm {
  uint64_t scalar;
  uint32_t row0, lane_stride, map;
  uint32_t base_flags;  // base | flags << 2
};
struct GateGroup {
  uint64_t constant;  // on the body word, in units of delta
  uint32_t first, terms;
};
struct GateLaunch {
  uint64_t *out;
  const uint64_t *wires, *caller_a, *caller_b, *clear;
  const GateGroup *groups;  // the groups of this launch
  const GateTerm *terms;    // the terms of the whole program (GateGroup::first counts from here)
  const uint32_t *maps;
  uint64_t delta;
  uint32_t words, inputs, lanes, lane0, clear_stride, ngroups;
};

__global__ void __launch_bounds__(kSumThreads) lwe_gate_sum_kernel(GateLaunch a) {
  const uint32_t row = blockIdx.x, first = blockIdx.y * kSumChunk + threadIdx.x;
  // all of this is uniform over the workgroup
  const uint32_t gl = row / a.inputs, n = row - gl * a.inputs, g = gl / a.lanes, l = gl - g * a.lanes;
  const TAP_GLOBAL GateGroup *G = (const TAP_GLOBAL GateGroup *)a.groups + g;
  const TAP_GLOBAL GateTerm *T = (const TAP_GLOBAL GateTerm *)a.terms;
  const TAP_GLOBAL uint32_t *maps = (const TAP_GLOBAL uint32_t *)a.maps;
  const TAP_GLOBAL uint64_t *clear = (const TAP_GLOBAL uint64_t *)a.clear;
  const uint32_t lo = G->first, hi = lo + G->terms;
  uint64_t body = G->constant;
  uint64_t acc[kSumWordsPerThread];
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) acc[u] = 0;
  for (uint32_t m = lo; m < hi; m += kSumInFlight) {
    uint64_t v[kSumInFlight][kSumWordsPerThread], sc[kSumInFlight];
    HX_UNROLL
    for (uint32_t t = 0; t < kSumInFlight; ++t) {
      const bool have = m + t < hi;
      const TAP_GLOBAL GateTerm *x = T + (have ? m + t : lo);
      const uint32_t base = x->base_flags & 3, flags = x->base_flags >> 2;
      const bool load = have && base != kGateClear;
      uint32_t sl = l;
      if (flags & kGateStateLane) {
        const uint32_t lane = a.lane0 + l, kind = x->map & 3, par = x->map >> 2;
        sl = kind == kMapPerm ? maps[par * kGateLanes + lane] : kind == kMapColumn ? ((lane & ~3u) | ((lane + par) & 3u)) : lane;
      }
      const size_t r = (size_t)x->row0 + (size_t)sl * x->lane_stride + ((flags & kGateBroadcast) ? 0 : n);
      const uint64_t *b = base == kGateCallerA ? a.caller_a : base == kGateCallerB ? a.caller_b : a.wires;
      const TAP_GLOBAL uint64_t *p = (const TAP_GLOBAL uint64_t *)b + r * a.words;
      if (have && base == kGateClear) body += x->scalar * clear[(size_t)n * a.clear_stride + x->row0];
      sc[t] = load ? x->scalar : 0;
      HX_UNROLL
      for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
        const uint32_t e = first + u * kSumThreads;
        v[t][u] = (load && e < a.words) ? p[e] : 0;
      }
    }
    HX_UNROLL
    for (uint32_t t = 0; t < kSumInFlight; ++t) {
      HX_UNROLL
      for (uint32_t u = 0; u < kSumWordsPerThread; ++u) acc[u] += sc[t] * v[t][u];
    }
  }
  TAP_GLOBAL uint64_t *po = (TAP_GLOBAL uint64_t *)a.out + (size_t)row * a.words;
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
    const uint32_t e = first + u * kSumThreads;
    if (e < a.words) po[e] = acc[u] + (e + 1 == a.words ? body * a.delta : 0);
  }
}

// what the launcher checks a launch against: the HOST copy of the groups / terms / maps the device pointers of `a` name, the
// lanes of the state (the domain of the lane maps) and the rows of the three bases
struct GateHost {
  const GateGroup *groups;
  const GateTerm *terms;
  const uint32_t *maps;
  uint32_t num_maps, state_lanes;
  size_t rows[3];  // wires, caller a, caller b
};

static void launch_gate_sum(hipStream_t st, const GateLaunch &a, const GateHost &h) {
  HX_PANIC_IF_FALSE(a.ngroups >= 1 && a.words >= 1 && a.inputs >= 1 && a.lanes >= 1 && a.out && h.groups,
                    "gate_sum: empty program (%u groups, %u words, %u inputs, %u lanes)", a.ngroups, a.words, a.inputs, a.lanes);
  HX_PANIC_IF_FALSE((uint64_t)a.ngroups * a.lanes * a.inputs <= 0x7fffffffu, "gate_sum: %u groups of %u lanes of %u inputs in one launch",
                    a.ngroups, a.lanes, a.inputs);
  const uint64_t *bases[3] = {a.wires, a.caller_a, a.caller_b};
  const uint64_t *o0 = a.out, *o1 = o0 + (size_t)a.ngroups * a.lanes * a.inputs * a.words;
  for (uint32_t g = 0; g < a.ngroups; ++g)
    for (uint32_t t = h.groups[g].first; t < h.groups[g].first + h.groups[g].terms; ++t) {
      const GateTerm &x = h.terms[t];
      const uint32_t base = x.base_flags & 3, flags = x.base_flags >> 2, kind = x.map & 3, par = x.map >> 2;
      if (base == kGateClear) {
        HX_PANIC_IF_FALSE(a.clear && x.row0 < a.clear_stride, "gate_sum: term %u of group %u reads clear entry %u of %u", t, g,
                          x.row0, a.clear_stride);
        continue;
      }
      HX_PANIC_IF_FALSE(bases[base] != nullptr, "gate_sum: term %u of group %u reads base %u, which is null", t, g, base);
      uint32_t lmin = 0, lmax = a.lanes - 1;
      if (flags & kGateStateLane) {
        HX_PANIC_IF_FALSE(kind <= kMapColumn && a.lane0 + a.lanes <= h.state_lanes && h.state_lanes <= kGateLanes &&
                              (kind != kMapPerm || (h.maps && par < h.num_maps)) &&
                              (kind != kMapColumn || (h.state_lanes % 4 == 0 && par < 4)),
                          "gate_sum: the lane map %u of term %u of group %u leaves the state of %u lanes", x.map, t, g,
                          h.state_lanes);
        lmin = ~0u, lmax = 0;
        for (uint32_t l = 0; l < a.lanes; ++l) {
          const uint32_t lane = a.lane0 + l;
          const uint32_t sl = kind == kMapPerm ? h.maps[par * kGateLanes + lane] : kind == kMapColumn ? ((lane & ~3u) | ((lane + par) & 3u)) : lane;
          HX_PANIC_IF_FALSE(sl < h.state_lanes, "gate_sum: the lane map %u of term %u of group %u leaves the state of %u lanes",
                            x.map, t, g, h.state_lanes);
          lmin = std::min(lmin, sl), lmax = std::max(lmax, sl);
        }
      }
      const size_t r0 = (size_t)x.row0 + (size_t)lmin * x.lane_stride;
      const size_t r1 = (size_t)x.row0 + (size_t)lmax * x.lane_stride + ((flags & kGateBroadcast) ? 0 : a.inputs - 1) + 1;
      HX_PANIC_IF_FALSE(r1 <= h.rows[base], "gate_sum: term %u of group %u reads row %zu of base %u, which holds %zu", t, g, r1 - 1,
                        base, h.rows[base]);
      const uint64_t *s0 = bases[base] + r0 * a.words, *s1 = bases[base] + r1 * a.words;
      HX_PANIC_IF_FALSE(o1 <= s0 || s1 <= o0, "gate_sum: the output overlaps the rows term %u of group %u reads", t, g);
    }
  HX_LAUNCH(lwe_gate_sum_kernel, dim3(a.ngroups * a.lanes * a.inputs, (a.words + kSumChunk - 1) / kSumChunk), dim3(kSumThreads), 0,
            st, a);
}

// ------------------------------------------------------------------ the program: segments of rounds of rows
// A row group is one bootstrap per (lane, input): its terms, its constant, its table and where the result goes.  A segment
// is a list of rounds over `lanes` lanes, run `passes` times on the lanes pass * lanes .. (the S-box at a parallelism below
// 16); wires a segment keeps to itself exist for the lanes of one pass.
struct GateDst {
  uint32_t caller;  // 0: a row of the wires, 1: a row of the caller's output
  uint32_t row0, lane_stride, in_stride, state_lane;
};
struct GateRow {
  std::vector<GateTerm> terms;
  uint64_t constant;
  uint32_t table;
  GateDst dst;
};
struct GateSegment {
  uint32_t lanes = 1, passes = 1;
  std::vector<std::vector<GateRow>> rounds;
  struct Placed {
    uint32_t g0, ng;
    size_t lut_off, out_off;  // out_off + pass * rows
    bool to_caller;
  };
  std::vector<Placed> placed;
  uint64_t rows_per_input() const {  // bootstraps of one run of the segment, per input
    uint64_t n = 0;
    for (auto &r : rounds) n += r.size();
    return n * lanes * passes;
  }
  void put(uint32_t round, GateRow row) {
    if (rounds.size() <= round) rounds.resize(round + 1);
    rounds[round].push_back(std::move(row));
  }
};

// A wire of the circuit before it is bootstrapped: the XOR of its terms (fresh bits) and of a constant bit
struct LazyTerm {
  GateTerm t;      // scalar 1
  uint32_t ready;  // the first round of the segment that can read it
};
struct Lazy {
  std::vector<LazyTerm> terms;
  uint32_t c = 0;
  uint32_t ready() const {
    uint32_t r = 0;
    for (auto &x : terms) r = std::max(r, x.ready);
    return r;
  }
};
static bool same_source(const GateTerm &a, const GateTerm &b) {
  return a.row0 == b.row0 && a.lane_stride == b.lane_stride && a.map == b.map && a.base_flags == b.base_flags;
}
static Lazy lazy_xor(const Lazy &a, const Lazy &b) {
  Lazy r = a;
  r.c ^= b.c;
  for (auto &x : b.terms) {
    auto it = std::find_if(r.terms.begin(), r.terms.end(), [&](const LazyTerm &y) { return same_source(x.t, y.t); });
    if (it != r.terms.end())
      r.terms.erase(it);  // x ^ x = 0
    else
      r.terms.push_back(x);
  }
  return r;
}
static Lazy lazy_of(uint32_t base, uint32_t row0, uint32_t lane_stride, uint32_t map, uint32_t flags, uint32_t ready = 0) {
  Lazy r;
  r.terms.push_back(LazyTerm{GateTerm{1, row0, lane_stride, map, base | flags << 2}, ready});
  return r;
}

// The Boyar-Peralta S-box (eprint 2011/332, also J. Cryptology 26(2)): 23 XORs on top, 32 ANDs and 30 XORs in the middle,
// 30 XOR / XNOR at the bottom.  U0 is the most significant input bit, S0 the most significant output bit.
// "d=a+b": XOR, "d=a*b": AND, "d=a#b": XNOR.
static const char *const kSboxGates =
    "y14=U3+U5 y13=U0+U6 y9=U0+U3 y8=U0+U5 t0=U1+U2 y1=t0+U7 y4=y1+U3 y12=y13+y14 y2=y1+U0 y5=y1+U6 y3=y5+y8 t1=U4+y12 "
    "y15=t1+U5 y20=t1+U1 y6=y15+U7 y10=y15+t0 y11=y20+y9 y7=U7+y11 y17=y10+y11 y19=y10+y8 y16=t0+y11 y21=y13+y16 y18=U0+y16 "
    "t2=y12*y15 t3=y3*y6 t4=t3+t2 t5=y4*U7 t6=t5+t2 t7=y13*y16 t8=y5*y1 t9=t8+t7 t10=y2*y7 t11=t10+t7 t12=y9*y11 t13=y14*y17 "
    "t14=t13+t12 t15=y8*y10 t16=t15+t12 t17=t4+t14 t18=t6+t16 t19=t9+t14 t20=t11+t16 t21=t17+y20 t22=t18+y19 t23=t19+y21 "
    "t24=t20+y18 t25=t21+t22 t26=t21*t23 t27=t24+t26 t28=t25*t27 t29=t28+t22 t30=t23+t24 t31=t22+t26 t32=t31*t30 t33=t32+t24 "
    "t34=t23+t33 t35=t27+t33 t36=t24*t35 t37=t36+t34 t38=t27+t36 t39=t29*t38 t40=t25+t39 t41=t40+t37 t42=t29+t33 t43=t29+t40 "
    "t44=t33+t37 t45=t42+t41 z0=t44*y15 z1=t37*y6 z2=t33*U7 z3=t43*y16 z4=t40*y1 z5=t29*y7 z6=t42*y11 z7=t45*y17 z8=t41*y10 "
    "z9=t44*y12 z10=t37*y3 z11=t33*y4 z12=t43*y13 z13=t40*y5 z14=t29*y2 z15=t42*y9 z16=t45*y14 z17=t41*y8 t46=z15+z16 "
    "t47=z10+z11 t48=z5+z13 t49=z9+z10 t50=z2+z12 t51=z2+z5 t52=z7+z8 t53=z0+z3 t54=z6+z7 t55=z16+z17 t56=z12+t48 t57=t50+t53 "
    "t58=z4+t46 t59=z3+t54 t60=t46+t57 t61=z14+t57 t62=t52+t58 t63=t49+t58 t64=z4+t59 t65=t61+t62 t66=z1+t63 S0=t59+t63 "
    "S6=t56#t62 S7=t48#t60 t67=t64+t65 S3=t53+t66 S4=t51+t66 S5=t47+t65 S1=t64#S3 S2=t55#t67";

// Host-side scheduler.  A sum of T fresh bits and a constant bit c is a row of value at most T + c and noise level T; a row
// must stay below msg carry in value and at (msg carry - 1) / (msg - 1) in noise level.  Tables:
//   parity      x & 1                                  (a refresh; XOR / XNOR / NOT / Rcon are sums and constants)
//   and_S       ((x / S) & 1) & ((x % S) & 1)          on the row S * (sum of hi) + (sum of lo), S = |lo| + c_lo + 1: the AND
//               of two lazy sums without cleaning them first (2 a + b at noise level 3 for two clean bits, where the
//               bivariate pack msg a + b costs msg + 1; 3 a + b1 + b2 or 2 (a1 + a2) + b at noise level 5)
// and the five tables of the counter addition (AesMem below).  A row goes into the first round after its terms exist.
struct GateScheduler {
  uint32_t space = 0, max_noise = 0, inputs = 1;
  std::vector<std::pair<std::string, std::function<uint64_t(uint64_t)>>> tables;
  size_t wire_rows = 0;  // rows of the wires handed out so far

  uint32_t table(const std::string &name, const std::function<uint64_t(uint64_t)> &f) {
    for (uint32_t i = 0; i < tables.size(); ++i)
      if (tables[i].first == name) return i;
    tables.emplace_back(name, f);
    return (uint32_t)tables.size() - 1;
  }
  uint32_t parity() {
    return table("parity", [](uint64_t x) -> uint64_t { return x & 1; });
  }
  uint32_t and_table(uint32_t S) {
    return table("and_" + std::to_string(S), [S](uint64_t x) -> uint64_t { return ((x / S) & 1) & ((x % S) & 1); });
  }
  size_t rows(size_t count) {
    const size_t r = wire_rows;
    wire_rows += count;
    HX_PANIC_IF_FALSE(wire_rows <= 0xffffffffu, "aes: %zu rows of wires", wire_rows);
    return r;
  }
  // a wire of `lanes` lanes of the segment (state_lane = false) or of the state (true): [lane][input]
  GateDst wire(uint32_t lanes, bool state_lane) {
    return GateDst{0, (uint32_t)rows((size_t)lanes * inputs), inputs, 1, state_lane ? 1u : 0u};
  }
  static Lazy read(const GateDst &d, uint32_t ready, uint32_t map = kMapIdentity) {
    return lazy_of(kGateWires, d.row0, d.lane_stride, map, d.state_lane ? kGateStateLane : 0, ready);
  }
  bool fits(const Lazy &x) const { return x.terms.size() <= max_noise && x.terms.size() + x.c <= space - 1; }
  static bool clean(const Lazy &x) { return x.terms.size() == 1 && x.c == 0; }

  // x & 1 of the sum into `dst`
  Lazy refresh(GateSegment &sg, const Lazy &x, const GateDst &dst) {
    HX_PANIC_IF_FALSE(fits(x) && !x.terms.empty(), "aes: a sum of %zu terms does not fit a block", x.terms.size());
    GateRow row{{}, x.c, parity(), dst};
    for (auto &t : x.terms) row.terms.push_back(t.t);
    const uint32_t r = x.ready();
    sg.put(r, std::move(row));
    return read(dst, r + 1);
  }
  // a sum of any length into `dst`: partial sums of the earliest terms are refreshed into wires of their own first
  Lazy reduce(GateSegment &sg, Lazy x, const GateDst &dst, uint32_t lanes, bool state_lane) {
    while (!fits(x)) {
      std::stable_sort(x.terms.begin(), x.terms.end(), [](const LazyTerm &a, const LazyTerm &b) { return a.ready < b.ready; });
      const uint32_t limit = std::min(max_noise, space - 2);
      const size_t take = std::min<size_t>(limit, x.terms.size() - limit + 1);
      Lazy part;
      part.terms.assign(x.terms.begin(), x.terms.begin() + take);
      x.terms.erase(x.terms.begin(), x.terms.begin() + take);
      const Lazy f = refresh(sg, part, wire(lanes, state_lane));
      x.terms.push_back(f.terms[0]);
    }
    return refresh(sg, x, dst);
  }
  // cost of the AND row with `hi` scaled: 0 when it does not fit
  uint32_t and_cost(const Lazy &hi, const Lazy &lo) const {
    const uint32_t S = (uint32_t)lo.terms.size() + lo.c + 1;
    const uint32_t value = S * ((uint32_t)hi.terms.size() + hi.c) + (uint32_t)lo.terms.size() + lo.c;
    const uint32_t noise = S * (uint32_t)hi.terms.size() + (uint32_t)lo.terms.size();
    return (value <= space - 1 && noise <= max_noise) ? noise : 0;
  }
  bool and_fits(const Lazy &a, const Lazy &b) const { return and_cost(a, b) || and_cost(b, a); }
  Lazy gate_and(GateSegment &sg, const Lazy &a, const Lazy &b, const GateDst &dst) {
    const uint32_t ab = and_cost(a, b), ba = and_cost(b, a);
    HX_PANIC_IF_FALSE(ab || ba, "aes: an AND of sums of %zu and %zu terms does not fit a block", a.terms.size(), b.terms.size());
    const bool a_hi = ab && (!ba || ab <= ba);
    const Lazy &hi = a_hi ? a : b, &lo = a_hi ? b : a;
    const uint32_t S = (uint32_t)lo.terms.size() + lo.c + 1;
    GateRow row{{}, (uint64_t)S * hi.c + lo.c, and_table(S), dst};
    for (auto &t : hi.terms) row.terms.push_back(t.t), row.terms.back().scalar = S;
    for (auto &t : lo.terms) row.terms.push_back(t.t);
    const uint32_t r = std::max(a.ready(), b.ready());
    sg.put(r, std::move(row));
    return read(dst, r + 1);
  }

  // The S-box on 8 input wires; the 8 outputs are refreshed into `out`.  Internal wires are wires of the segment's lanes.
  // A gate takes its operands as they are when the result fits; otherwise it takes the refreshed twin of an operand (made
  // once per wire), preferring in this order: the fewest new bootstraps, the earliest round, the shortest sum.
  void sbox(GateSegment &sg, const Lazy in[8], const GateDst out[8]) {
    std::map<std::string, Lazy> w, twin;
    for (uint32_t i = 0; i < 8; ++i) w["U" + std::to_string(i)] = in[i];
    const auto twin_of = [&](const std::string &n) -> Lazy {
      if (clean(w[n])) return w[n];
      if (!twin.count(n)) twin[n] = refresh(sg, w[n], wire(sg.lanes, false));
      return twin[n];
    };
    const auto twin_cost = [&](const std::string &n) -> uint32_t { return (clean(w[n]) || twin.count(n)) ? 0 : 1; };
    const auto twin_peek = [&](const std::string &n, uint32_t tag) -> Lazy {  // what twin_of would return, without making it
      if (clean(w[n])) return w[n];
      if (twin.count(n)) return twin[n];
      return lazy_of(kGateWires, 0xffffffffu - tag, 0, 0, 0, w[n].ready() + 1);  // a wire that does not exist yet
    };
    std::string gates(kSboxGates);
    size_t pos = 0;
    while (pos < gates.size()) {
      size_t end = gates.find(' ', pos);
      if (end == std::string::npos) end = gates.size();
      const std::string gte = gates.substr(pos, end - pos);
      pos = end + 1;
      if (gte.empty()) continue;
      const size_t eq = gte.find('='), op = gte.find_first_of("+*#", eq);
      const std::string d = gte.substr(0, eq), an = gte.substr(eq + 1, op - eq - 1), bn = gte.substr(op + 1);
      const char kind = gte[op];
      HX_PANIC_IF_FALSE(w.count(an) && w.count(bn), "aes: gate %s reads a wire that does not exist", gte.c_str());
      // the four ways to take the operands
      int best = -1;
      uint64_t best_score = ~(uint64_t)0;
      for (int choice = 0; choice < 4; ++choice) {
        const bool ra = choice & 1, rb = choice & 2;
        if ((ra && clean(w[an])) || (rb && clean(w[bn]))) continue;  // the same as the choice without
        const Lazy la = ra ? twin_peek(an, 0) : w[an], lb = rb ? twin_peek(bn, 1) : w[bn];
        uint32_t terms, ready = std::max(la.ready(), lb.ready());
        if (kind == '*') {
          if (!and_fits(la, lb)) continue;
          terms = 1;
        } else {
          const Lazy x = lazy_xor(la, lb);
          if (!fits(x)) continue;
          terms = (uint32_t)x.terms.size();
        }
        const uint32_t cost = (ra ? twin_cost(an) : 0) + (rb ? twin_cost(bn) : 0);
        // on equal cost, refresh the longer operand
        const uint32_t longer = (choice == 1 && w[an].terms.size() < w[bn].terms.size()) || (choice == 2 && w[bn].terms.size() < w[an].terms.size());
        const uint64_t score = ((uint64_t)cost << 48) | ((uint64_t)ready << 32) | ((uint64_t)terms << 8) | longer;
        if (score < best_score) best_score = score, best = choice;
      }
      HX_PANIC_IF_FALSE(best >= 0, "aes: gate %s fits no block at this base", gte.c_str());
      const Lazy la = (best & 1) ? twin_of(an) : w[an], lb = (best & 2) ? twin_of(bn) : w[bn];
      if (kind == '*') {
        w[d] = gate_and(sg, la, lb, wire(sg.lanes, false));
      } else {
        w[d] = lazy_xor(la, lb);
        if (kind == '#') w[d].c ^= 1;
      }
    }
    for (uint32_t i = 0; i < 8; ++i) refresh(sg, w["S" + std::to_string(i)], out[i]);
  }
};

// ------------------------------------------------------------------ the cipher on the round driver
// The state is bit-sliced and wire-major for the whole call: wire j (bit 7 - j of a byte; j = 0 the most significant, the
// caller's block order) occupies rows [byte lane][input].  Segments of a cipher scratch:
//   ADD   counter addition and AddRoundKey 0, 9 rounds: pairs of IV bits packed with their clear counter bits into one
//         generate / propagate state (2 iv_hi + iv_lo + 4 c_lo + 8 c_hi: the counter bits are clear terms, value <= 15,
//         noise level 3), a Sklansky prefix scan over the 63 pairs that matter in 6 rounds (3 hi + lo, noise level 4; a
//         prefix that starts at bit 0 is a carry bit), the carries into odd bits (iv + carry + c >= 2) and the sum bits
//         (iv + carry + c + key, parity), written into the state wires.  441 bootstraps per input.
//   SBOX  the S-box on the lanes of one pass, 16 / parallelism passes per cipher round
//   LIN   ShiftRows, MixColumns and AddRoundKey as sums of the S-box outputs (permuted lanes) and a broadcast key row
//   LAST  ShiftRows and AddRoundKey of the last round; the output index writes the caller's layout
// and of a key-schedule scratch: SBOX on the four lanes of RotWord(w[4k - 1]) read from the caller's rows in place, and one
// KLIN per step k (the Rcon constants differ): 128 rows w[4k + j] = w[4k - 4] ^ .. ^ w[4k - 4 + j] ^ SubWord ^ Rcon.
struct AesMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x41455331;  // "AES1"
  LutDriver drv;
  GateScheduler sch;
  bool key_schedule = false;
  uint32_t inputs = 0, parallelism = 0;
  uint32_t cipher_rounds = 10, key_words = 4;  // AES-128; AES-256 is (14, 8) and a second SubWord in the schedule
  std::vector<GateSegment> segs;               // cipher: ADD, SBOX, LIN, LAST; key schedule: SBOX, KLIN 1 .. rounds
  enum : uint32_t { kAdd = 0, kSbox = 1, kLin = 2, kLast = 3 };
  std::vector<GateGroup> h_groups;
  std::vector<GateTerm> h_terms;
  std::vector<uint32_t> h_maps;
  std::vector<uint64_t> h_tables;  // [table][msg carry]: the entries, for the dump
  GateDst x_wire[8], sb_wire[8];
  uint64_t *d_wires = nullptr, *d_in = nullptr, *d_clear = nullptr, *i_lut = nullptr, *i_out = nullptr;
  GateGroup *d_groups = nullptr;
  GateTerm *d_terms = nullptr;
  uint32_t *d_maps = nullptr;
  uint64_t rounds_issued = 0;
  DeviceBlocks own;

  uint32_t state_lanes() const { return key_schedule ? 4 : kGateLanes; }
  uint64_t pbs_count() const {
    if (key_schedule) {
      uint64_t n = 0;
      for (uint32_t k = 1; k <= cipher_rounds; ++k) n += segs[0].rows_per_input() + segs[k].rows_per_input();
      return n;
    }
    return inputs * (segs[kAdd].rows_per_input() + cipher_rounds * segs[kSbox].rows_per_input() +
                     (cipher_rounds - 1) * segs[kLin].rows_per_input() + segs[kLast].rows_per_input());
  }
  uint64_t round_count() const {
    if (key_schedule) return (uint64_t)cipher_rounds * (segs[0].placed.size() + segs[1].placed.size());
    return segs[kAdd].placed.size() + (uint64_t)cipher_rounds * segs[kSbox].passes * segs[kSbox].placed.size() +
           (uint64_t)(cipher_rounds - 1) * segs[kLin].placed.size() + segs[kLast].placed.size();
  }

  // lane 4 c + r of the state after ShiftRows and a step of k rows down the column: the S-box output of lane
  // 4 ((c + r') % 4) + r', r' = (r + k) % 4
  static uint32_t shift_rows_lane(uint32_t lane, uint32_t k) {
    const uint32_t c = lane / 4, r = (lane + k) % 4;
    return 4 * ((c + r) % 4) + r;
  }

  void build_add(GateSegment &sg) {
    sg.lanes = 1, sg.passes = 1;
    const uint32_t N = inputs;
    const auto local = [&]() { return sch.wire(1, false); };
    const auto term = [](uint32_t base, uint32_t row0, uint64_t scalar, uint32_t flags) {
      return GateTerm{scalar, row0, 0, kMapIdentity, base | flags << 2};
    };
    const auto iv = [&](uint32_t bit, uint64_t s) { return term(kGateCallerA, 127 - bit, s, kGateBroadcast); };
    const auto key = [&](uint32_t bit) { return term(kGateCallerB, 127 - bit, 1, kGateBroadcast); };
    const auto ctr = [&](uint32_t bit, uint64_t s) { return term(kGateClear, bit, s, 0); };
    const auto from = [&](const GateDst &d, uint64_t s) { return GateTerm{s, d.row0, 0, kMapIdentity, kGateWires}; };
    // (generate, propagate) of a span as one value: 0 neither, 1 generates, 2 propagates
    const auto pair_state = [](uint64_t x) -> uint64_t {
      const uint64_t il = x & 1, ih = (x >> 1) & 1, cl = (x >> 2) & 1, ch = (x >> 3) & 1;
      const uint64_t g = (ih & ch) | ((ih ^ ch) & il & cl), p = (ih ^ ch) & (il ^ cl);
      return g ? 1 : p ? 2 : 0;
    };
    const auto combine = [](uint64_t x) -> uint64_t {
      const uint64_t hi = x / 3, lo = x % 3;
      return x >= 9 ? 0 : hi == 2 ? lo : hi;
    };
    const uint32_t t_pair = sch.table("pair_state", pair_state);
    const uint32_t t_pair_bit = sch.table("pair_carry", [pair_state](uint64_t x) -> uint64_t { return pair_state(x) == 1; });
    const uint32_t t_comb = sch.table("combine_state", combine);
    const uint32_t t_comb_bit = sch.table("combine_carry", [combine](uint64_t x) -> uint64_t { return combine(x) == 1; });
    const uint32_t t_maj = sch.table("majority", [](uint64_t x) -> uint64_t { return x >= 2; });
    const uint32_t t_par = sch.parity();
    (void)N;
    // round 0: the pairs (bits 2 j, 2 j + 1), j < 63 (nothing reads the carry out of bit 127)
    std::vector<GateDst> e(63);
    for (uint32_t j = 0; j < 63; ++j) {
      e[j] = local();
      sg.put(0, GateRow{{iv(2 * j, 1), iv(2 * j + 1, 2), ctr(2 * j, 4), ctr(2 * j + 1, 8)}, 0, j == 0 ? t_pair_bit : t_pair, e[j]});
    }
    // rounds 1 .. 6: Sklansky — the upper half of every block of 2^l pairs takes the last prefix of the lower half
    for (uint32_t l = 1; l <= 6; ++l)
      for (uint32_t j = 0; j < 63; ++j) {
        if (!(j >> (l - 1) & 1)) continue;
        const uint32_t partner = ((j >> (l - 1)) << (l - 1)) - 1;
        const GateDst d = local();
        sg.put(l, GateRow{{from(e[j], 3), from(e[partner], 1)}, 0, (j >> l) == 0 ? t_comb_bit : t_comb, d});
        e[j] = d;
      }
    // round 7: the carry into bit 2 j + 1 from the carry into bit 2 j (e[j - 1]; none into bit 0)
    std::vector<GateDst> odd(64);
    for (uint32_t j = 0; j < 64; ++j) {
      odd[j] = local();
      GateRow row{{iv(2 * j, 1), ctr(2 * j, 1)}, 0, t_maj, odd[j]};
      if (j) row.terms.push_back(from(e[j - 1], 1));
      sg.put(7, std::move(row));
    }
    // round 8: sum bits with round key 0, into the state wires (block 127 - i is bit j = (127 - i) % 8 of byte (127 - i) / 8)
    for (uint32_t i = 0; i < 128; ++i) {
      const uint32_t blk = 127 - i;
      const GateDst &x = x_wire[blk % 8];
      GateRow row{{iv(i, 1), key(i), ctr(i, 1)}, 0, t_par, GateDst{0, x.row0 + (blk / 8) * x.lane_stride, 0, 1, 0}};
      if (i & 1)
        row.terms.push_back(from(odd[i / 2], 1));
      else if (i)
        row.terms.push_back(from(e[i / 2 - 1], 1));
      sg.put(8, std::move(row));
    }
  }

  void build_cipher() {
    const uint32_t N = inputs;
    for (uint32_t j = 0; j < 8; ++j) x_wire[j] = sch.wire(kGateLanes, true);
    for (uint32_t j = 0; j < 8; ++j) sb_wire[j] = sch.wire(kGateLanes, true);
    for (uint32_t k = 0; k < 4; ++k)
      for (uint32_t l = 0; l < kGateLanes; ++l) h_maps.push_back(shift_rows_lane(l, k));
    segs.resize(4);
    build_add(segs[kAdd]);
    GateSegment &sb = segs[kSbox];
    sb.lanes = parallelism, sb.passes = kGateLanes / parallelism;
    Lazy in[8];
    for (uint32_t j = 0; j < 8; ++j) in[j] = GateScheduler::read(x_wire[j], 0);
    sch.sbox(sb, in, sb_wire);
    // bit p of MixColumns' output byte: a, b, c, d the bytes 0 .. 3 rows down the column after ShiftRows,
    // (2 a ^ 3 b ^ c ^ d)_p = a_(p-1) ^ b_(p-1) ^ [p in {0, 1, 3, 4}] (a_7 ^ b_7) ^ b_p ^ c_p ^ d_p, without the p - 1 terms at p = 0
    GateSegment &lin = segs[kLin], &last = segs[kLast];
    lin.lanes = last.lanes = kGateLanes;
    const auto s_bit = [&](uint32_t p, uint32_t k) { return GateScheduler::read(sb_wire[7 - p], 0, kMapPerm | k << 2); };
    const auto key_bit = [&](uint32_t j) { return lazy_of(kGateCallerA, j, 8, kMapIdentity, kGateStateLane | kGateBroadcast); };
    for (uint32_t p = 0; p < 8; ++p) {
      Lazy x = lazy_xor(lazy_xor(s_bit(p, 1), s_bit(p, 2)), s_bit(p, 3));
      if (p) x = lazy_xor(x, lazy_xor(s_bit(p - 1, 0), s_bit(p - 1, 1)));
      if (p == 0 || p == 1 || p == 3 || p == 4) x = lazy_xor(x, lazy_xor(s_bit(7, 0), s_bit(7, 1)));
      sch.reduce(lin, lazy_xor(x, key_bit(7 - p)), x_wire[7 - p], kGateLanes, true);
      sch.refresh(last, lazy_xor(s_bit(p, 0), key_bit(7 - p)), GateDst{1, 7 - p, 8, 128, 1});
    }
    (void)N;
  }

  void build_key_schedule() {
    static const uint32_t rcon[] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1b, 0x36, 0x6c, 0xd8, 0xab, 0x4d};
    const uint32_t W = key_words;
    for (uint32_t j = 0; j < 8; ++j) sb_wire[j] = sch.wire(4, true);
    for (uint32_t l = 0; l < kGateLanes; ++l) h_maps.push_back(l < 4 ? (l + 1) % 4 : l);  // RotWord
    segs.resize(1 + cipher_rounds);
    GateSegment &sb = segs[0];
    sb.lanes = 4, sb.passes = 1;
    Lazy in[8];  // byte lane b of the last word of the previous round key: block 32 (W - 1) + 8 b + j
    for (uint32_t j = 0; j < 8; ++j) in[j] = lazy_of(kGateCallerA, 32 * (W - 1) + j, 8, kMapPerm, kGateStateLane | kGateBroadcast);
    sch.sbox(sb, in, sb_wire);
    for (uint32_t k = 1; k <= cipher_rounds; ++k) {
      GateSegment &lin = segs[k];
      for (uint32_t word = 0; word < W; ++word)
        for (uint32_t b = 0; b < 4; ++b)
          for (uint32_t j = 0; j < 8; ++j) {
            Lazy x = lazy_of(kGateWires, sb_wire[j].row0 + b * sb_wire[j].lane_stride, 0, kMapIdentity, 0);
            for (uint32_t m = 0; m <= word; ++m) x = lazy_xor(x, lazy_of(kGateCallerA, 32 * m + 8 * b + j, 0, kMapIdentity, kGateBroadcast));
            if (b == 0) x.c ^= (rcon[k - 1] >> (7 - j)) & 1;
            sch.reduce(lin, x, GateDst{1, 32 * W * k + 32 * word + 8 * b + j, 0, 1, 0}, 1, false);
          }
    }
  }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t num_inputs, uint32_t sbox_parallelism, bool is_key_schedule,
            const char *who) {
    const uint32_t space = p.msg * p.carry, noise = (space - 1) / (p.msg - 1);
    key_schedule = is_key_schedule;
    HX_PANIC_IF_FALSE(num_inputs >= 1 && num_inputs <= (1u << 16), "%s: %u inputs", who, num_inputs);
    HX_PANIC_IF_FALSE(sbox_parallelism == 1 || sbox_parallelism == 2 || sbox_parallelism == 4 || sbox_parallelism == 8 ||
                          sbox_parallelism == 16,
                      "%s: sbox_parallelism %u is not one of 1, 2, 4, 8, 16", who, sbox_parallelism);
    HX_PANIC_IF_FALSE(space >= 16 && noise >= 5, "%s: moduli (%u, %u) do not hold the value 15 and the noise level 5 a row reaches",
                      who, p.msg, p.carry);
    inputs = num_inputs, parallelism = sbox_parallelism;
    sch.space = space, sch.max_noise = noise, sch.inputs = inputs;
    if (key_schedule)
      build_key_schedule();
    else
      build_cipher();
    // flatten: groups and terms of all segments, table and output indexes of every round (and pass)
    std::vector<uint64_t> lut, out;
    uint32_t widest = 0;
    for (GateSegment &sg : segs)
      for (auto &round : sg.rounds) {
        if (round.empty()) continue;
        GateSegment::Placed pl{(uint32_t)h_groups.size(), (uint32_t)round.size(), lut.size(), out.size(), round[0].dst.caller != 0};
        const uint32_t rows = pl.ng * sg.lanes * inputs;
        widest = std::max(widest, rows);
        for (const GateRow &row : round) {
          HX_PANIC_IF_FALSE((row.dst.caller != 0) == pl.to_caller, "%s: a round writes both the wires and the caller's rows", who);
          h_groups.push_back(GateGroup{row.constant, (uint32_t)h_terms.size(), (uint32_t)row.terms.size()});
          h_terms.insert(h_terms.end(), row.terms.begin(), row.terms.end());
          for (uint32_t i = 0; i < sg.lanes * inputs; ++i) lut.push_back(row.table);
        }
        for (uint32_t pass = 0; pass < sg.passes; ++pass)
          for (const GateRow &row : round)
            for (uint32_t l = 0; l < sg.lanes; ++l)
              for (uint32_t n = 0; n < inputs; ++n)
                out.push_back((uint64_t)row.dst.row0 + (uint64_t)(row.dst.state_lane ? pass * sg.lanes + l : l) * row.dst.lane_stride +
                              (uint64_t)n * row.dst.in_stride);
        sg.placed.push_back(pl);
      }
    const size_t lw = (size_t)(p.k + 1) * p.N, w = (size_t)p.big_n + 1;
    std::vector<std::vector<uint64_t>> luts(sch.tables.size(), std::vector<uint64_t>(lw));
    for (size_t t = 0; t < sch.tables.size(); ++t) {
      generate_lut(p, luts[t].data(), sch.tables[t].second);
      for (uint32_t x = 0; x < space; ++x) h_tables.push_back(sch.tables[t].second(x));
    }
    drv.init(ss, p, std::min<uint32_t>(widest, 1u << 16), luts);
    own.alloc(d_wires, sch.wire_rows * w * sizeof(uint64_t));
    own.alloc(d_in, (size_t)widest * w * sizeof(uint64_t));
    if (!key_schedule) own.alloc(d_clear, (size_t)128 * inputs * sizeof(uint64_t));
    const hipStream_t st = S0(ss);
    i_lut = own.upload(st, lut), i_out = own.upload(st, out);
    d_groups = own.upload(st, h_groups), d_terms = own.upload(st, h_terms), d_maps = own.upload(st, h_maps);
  }

  // one run of a segment.  caller_a / caller_b: what its caller terms read (rows_a / rows_b rows); out_caller: where the
  // rounds marked to_caller write
  void run(const CudaStreamsFFI &ss, const GateSegment &sg, const uint64_t *caller_a, size_t rows_a, const uint64_t *caller_b,
           size_t rows_b, uint64_t *out_caller, void *const *ksks, void *const *bsks, uint32_t first_pass = 0,
           uint32_t passes = ~0u, bool launches_only = false) {
    const Params &p = drv.p;
    const hipStream_t st = S0(ss);
    const GateHost host{nullptr, h_terms.data(), h_maps.data(), (uint32_t)(h_maps.size() / kGateLanes), state_lanes(),
                        {sch.wire_rows, rows_a, rows_b}};
    for (uint32_t pass = first_pass; pass < std::min(sg.passes, passes); ++pass)
      for (const GateSegment::Placed &pl : sg.placed) {
        GateLaunch a{d_in,   d_wires,   caller_a,  caller_b,  d_clear,          d_groups + pl.g0, d_terms, d_maps,
                     p.delta(), p.big_n + 1, inputs, sg.lanes, pass * sg.lanes, 128,           pl.ng};
        GateHost h = host;
        h.groups = h_groups.data() + pl.g0;
        launch_gate_sum(st, a, h);
        if (launches_only) continue;  // (benches: the data movement without the bootstraps)
        const uint32_t rows = pl.ng * sg.lanes * inputs;
        HX_PANIC_IF_FALSE(!pl.to_caller || out_caller, "aes: a round writes the caller's rows and there are none");
        drv.round(ss, pl.to_caller ? out_caller : d_wires, i_out + pl.out_off + (size_t)pass * rows, d_in, nullptr,
                  i_lut + pl.lut_off, rows, ksks, bsks);
        ++rounds_issued;
      }
  }

  void check_count(uint64_t pbs_before, uint64_t rounds_before, const char *who) const {
    HX_PANIC_IF_FALSE(drv.issued - pbs_before == pbs_count() && rounds_issued - rounds_before == round_count(),
                      "%s: %llu bootstraps in %llu rounds issued, %llu in %llu counted", who,
                      (unsigned long long)(drv.issued - pbs_before), (unsigned long long)(rounds_issued - rounds_before),
                      (unsigned long long)pbs_count(), (unsigned long long)round_count());
  }

  void counter_addition(const CudaStreamsFFI &ss, const uint64_t *iv, const uint64_t *round_keys, const uint64_t *counter_bits,
                        void *const *ksks, void *const *bsks) {
    HX_RANGE("aes: counter addition, %u inputs", inputs);
    // the call's input, in one upload (the caller's array may be pageable: the copy is staged before the call returns)
    HX_CHECK(hipMemcpyAsync(d_clear, counter_bits, (size_t)128 * inputs * sizeof(uint64_t), hipMemcpyHostToDevice, S0(ss)));
    run(ss, segs[kAdd], iv, 128, round_keys, 128, nullptr, ksks, bsks);
  }
  // cipher rounds r0 .. r1 (1 .. cipher_rounds) on the state wires
  void cipher(const CudaStreamsFFI &ss, uint32_t r0, uint32_t r1, const uint64_t *round_keys, uint64_t *output, void *const *ksks,
              void *const *bsks) {
    const size_t w = (size_t)drv.p.big_n + 1;
    for (uint32_t r = r0; r <= r1; ++r) {
      HX_RANGE("aes: round %u of %u, %u inputs, %u S-box passes", r, cipher_rounds, inputs, segs[kSbox].passes);
      run(ss, segs[kSbox], nullptr, 0, nullptr, 0, nullptr, ksks, bsks);
      run(ss, segs[r == cipher_rounds ? kLast : kLin], round_keys + (size_t)128 * r * w, 128, nullptr, 0, output, ksks, bsks);
    }
  }
  void encrypt(const CudaStreamsFFI &ss, uint64_t *output, const uint64_t *iv, const uint64_t *round_keys,
               const uint64_t *counter_bits, void *const *ksks, void *const *bsks) {
    const uint64_t pbs = drv.issued, rounds = rounds_issued;
    counter_addition(ss, iv, round_keys, counter_bits, ksks, bsks);
    cipher(ss, 1, cipher_rounds, round_keys, output, ksks, bsks);
    check_count(pbs, rounds, "aes_ctr_encrypt");
  }
  void expand_key(const CudaStreamsFFI &ss, uint64_t *expanded, const uint64_t *key, void *const *ksks, void *const *bsks) {
    const uint64_t pbs = drv.issued, rounds = rounds_issued;
    const size_t w = (size_t)drv.p.big_n + 1, kw = (size_t)32 * key_words;
    HX_CHECK(hipMemcpyAsync(expanded, key, kw * w * sizeof(uint64_t), hipMemcpyDeviceToDevice, S0(ss)));
    for (uint32_t k = 1; k <= cipher_rounds; ++k) {
      HX_RANGE("aes: key schedule step %u of %u", k, cipher_rounds);
      const uint64_t *prev = expanded + kw * (k - 1) * w;
      run(ss, segs[0], prev, kw, nullptr, 0, nullptr, ksks, bsks);
      run(ss, segs[k], prev, kw, nullptr, 0, expanded, ksks, bsks);
    }
    check_count(pbs, rounds, "key_expansion");
  }

  // rows [wire j][lane][input] <-> 8 wires of `lanes` lanes
  void move_wires(hipStream_t st, const GateDst wires[8], uint64_t *rows, uint32_t lanes, bool load) {
    const size_t w = (size_t)drv.p.big_n + 1, n = (size_t)lanes * inputs * w;
    for (uint32_t j = 0; j < 8; ++j) {
      uint64_t *wire = d_wires + (size_t)wires[j].row0 * w, *r = rows + j * n;
      HX_CHECK(hipMemcpyAsync(load ? wire : r, load ? r : wire, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    }
  }

  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    own.release(S0(ss));
  }
};

// The data movement of one middle cipher round composed from what the layer had before the kernel, in the reference's order
// (aes.cuh:882-974; tools/bench_aes.py times it against the gate-sum launches of one round): per S-box wire a gather copy in
// and a scatter copy out per byte (aes.cuh:320-335, 576-589), the circuit's XORs as pairwise additions and its batched flushes
// and ANDs as copies into and out of the batch buffer (aes.cuh:163-183, 211-236), ShiftRows as row copies, MixColumns as
// column copies, doublings and additions (aes.cuh:721-821), the round key tiled per input, transposed and added
// (aes.cuh:958-972).  The bootstraps are not run.  state: [128][N] rows, key: 128 rows, tmp: 512 N rows.
static void aes_round_baseline(hipStream_t st, uint64_t *state, const uint64_t *key, uint64_t *tmp, uint32_t words, uint32_t N) {
  const size_t rw = (size_t)N * words, rb = rw * sizeof(uint64_t);
  uint64_t *bits = tmp, *wires = tmp + 128 * rw, *batch = wires + 128 * rw, *tiled = batch + 128 * rw;
  const auto copy = [&](uint64_t *out, const uint64_t *x, size_t bytes) {
    HX_CHECK(hipMemcpyAsync(out, x, bytes, hipMemcpyDeviceToDevice, st));
  };
  const auto add = [&](uint64_t *out, const uint64_t *x, const uint64_t *y, uint32_t rows) {
    axpy(st, out, nullptr, x, nullptr, 1, y, nullptr, words, rows);
  };
  // S-box: gather, 83 XORs on 16 N rows each, 24 flush and 7 AND batches gathered and scattered wire by wire, scatter
  for (uint32_t bit = 0; bit < 8; ++bit)
    for (uint32_t byte = 0; byte < 16; ++byte) copy(bits + (bit * 16 + byte) * rw, state + (byte * 8 + bit) * rw, rb);
  for (uint32_t x = 0; x < 83; ++x) add(wires + (x % 8) * 16 * rw, bits + (x % 8) * 16 * rw, bits + ((x + 1) % 8) * 16 * rw, 16 * N);
  for (uint32_t f = 0; f < 56 + 2 * 32; ++f) copy(batch + (f % 8) * 16 * rw, wires + (f % 8) * 16 * rw, 16 * rb);  // in
  for (uint32_t f = 0; f < 56 + 32; ++f) copy(wires + (f % 8) * 16 * rw, batch + (f % 8) * 16 * rw, 16 * rb);      // out
  for (uint32_t bit = 0; bit < 8; ++bit)
    for (uint32_t byte = 0; byte < 16; ++byte) copy(state + (byte * 8 + bit) * rw, wires + (bit * 16 + byte) * rw, rb);
  // ShiftRows: 12 bytes move through a copy of the state
  copy(bits, state, 128 * rb);
  for (uint32_t lane = 0; lane < 16; ++lane)
    if (lane % 4) copy(state + lane * 8 * rw, bits + AesMem::shift_rows_lane(lane, 0) * 8 * rw, 8 * rb);
  // MixColumns, column by column: 32 row copies, four doublings (7 copies and 3 additions each), a copy of 2 b0, and per bit
  // four rows of one copy and four additions
  for (uint32_t col = 0; col < 4; ++col) {
    uint64_t *s = state + col * 32 * rw;
    for (uint32_t i = 0; i < 32; ++i) copy(bits + i * rw, s + i * rw, rb);
    for (uint32_t b = 0; b < 4; ++b) {
      for (uint32_t i = 0; i < 7; ++i) copy(wires + (b * 8 + i) * rw, bits + (b * 8 + i + 1) * rw, rb);
      copy(wires + (b * 8 + 7) * rw, bits + b * 8 * rw, rb);
      for (uint32_t i : {3u, 4u, 6u}) add(wires + (b * 8 + i) * rw, wires + (b * 8 + i) * rw, bits + b * 8 * rw, N);
    }
    copy(wires + 32 * rw, wires, 8 * rb);
    for (uint32_t bit = 0; bit < 8; ++bit)
      for (uint32_t b = 0; b < 4; ++b) {
        uint64_t *d = s + (b * 8 + bit) * rw;
        copy(d, wires + (b * 8 + bit) * rw, rb);
        for (uint32_t k = 1; k < 4; ++k) add(d, d, bits + (((b + k) % 4) * 8 + bit) * rw, N);
        add(d, d, wires + (((b + 1) % 4) * 8 + bit) * rw, N);
      }
  }
  // AddRoundKey: the key tiled per input, transposed to [bit][input] (the reference has a kernel for the transpose: it is
  // counted as one contiguous copy here), added
  for (uint32_t n = 0; n < N; ++n) copy(tiled + (size_t)n * 128 * words, key, (size_t)128 * words * sizeof(uint64_t));
  copy(batch, tiled, 128 * rb);
  add(state, state, batch, 128 * N);
}

}  // namespace radix
}  // namespace tfhe_hip
