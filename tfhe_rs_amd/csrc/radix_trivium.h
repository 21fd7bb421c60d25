// radix_trivium.h — Trivium transciphering (cuda/src/trivium/trivium.cuh, include/trivium/trivium_utilities.h): the
// table-driven tap kernel and the scratch that runs 64 cipher steps in two bootstrap rounds.
// Included by integer.hip only, after the round driver (LutDriver) and the scratch protocol it builds on.
//
// Replaces, per batch of 64 steps of trivium_compute_64_steps (trivium.cuh:73-276): the pairwise host_addition calls, the
// copies of taps into pack buffers, two full copies of every register (shift_and_insert_batch) and the reversal of the
// keystream through a workspace — here two launches of one kernel form the inputs of the batch's two rounds from the
// taps where they are, and the second round's output index places new bits and keystream.
#pragma once
#include "hx.h"
#include "radix_sum.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace tfhe_hip {
namespace radix {

// out_g[q N + n] = sum over the group's terms t of scalar_t * src_t[(pos_t + step_t q) N + n], on u64 words modulo 2^64,
// rows of `words` words.  g: output group (blockIdx.z), q: bit of the batch (0 .. bits_g - 1) and n: input (0 .. N - 1),
// both from blockIdx.x = q N + n; blockIdx.y: slice of kSumChunk words.  A term is (source base, starting position,
// direction, scalar); the table arrives by value in the kernel arguments, so group, source rows and scalars are
// workgroup-uniform and live on the scalar unit — no index array exists.  Nothing here knows the cipher: registers, tap
// positions and the number of groups are the table's.
// Rows are big_n + 1 words, an odd count, so a row is only 8-byte aligned: 8-byte accesses, consecutive lanes on
// consecutive words; the (up to) ten loads of a lane are issued before its adds and its two stores.  No LDS, no scratch.
// No output row may overlap a row that any group reads: the launcher refuses it.
// The table is indexed by blockIdx.z, so the compiler cannot tell that the pointers it holds are kernel arguments: they are
// marked as global memory by hand (flat accesses otherwise).
constexpr uint32_t kTapGroups = 4, kTapTerms = 5;
#if defined(__HIP_DEVICE_COMPILE__)
#define TAP_GLOBAL __attribute__((address_space(1)))
#else
#define TAP_GLOBAL
#endif

struct TapTerm {
  const uint64_t *src;
  uint64_t scalar;
  uint32_t pos;  // position that bit 0 of the batch reads
  int32_t step;  // + 1: bit q reads position pos + q; - 1: pos - q
};
struct TapGroup {
  uint64_t *out;
  uint32_t bits, terms;
  TapTerm t[kTapTerms];
};
struct TapTable {
  uint32_t words, inputs, groups, reserved;
  TapGroup g[kTapGroups];
};

__global__ void __launch_bounds__(kSumThreads) lwe_tap_sum_kernel(TapTable a) {
  const uint32_t row = blockIdx.x, first = blockIdx.y * kSumChunk + threadIdx.x;
  // all of this is uniform over the workgroup
  const TapGroup &g = a.g[blockIdx.z];
  const uint32_t q = row / a.inputs, n = row - q * a.inputs;
  if (q >= g.bits) return;  // a group with fewer bits than the widest one of the launch
  const TAP_GLOBAL uint64_t *ps[kTapTerms];
  uint64_t sc[kTapTerms];
  HX_UNROLL
  for (uint32_t t = 0; t < kTapTerms; ++t) {
    const bool have = t < g.terms;
    const uint32_t p = g.t[t].step < 0 ? g.t[t].pos - q : g.t[t].pos + q;
    ps[t] = have ? (const TAP_GLOBAL uint64_t *)(g.t[t].src + ((size_t)p * a.inputs + n) * a.words) : nullptr;
    sc[t] = have ? g.t[t].scalar : 0;
  }
  uint64_t v[kTapTerms][kSumWordsPerThread];
  HX_UNROLL
  for (uint32_t t = 0; t < kTapTerms; ++t) {
    HX_UNROLL
    for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
      const uint32_t e = first + u * kSumThreads;
      v[t][u] = (ps[t] && e < a.words) ? ps[t][e] : 0;
    }
  }
  TAP_GLOBAL uint64_t *po = (TAP_GLOBAL uint64_t *)(g.out + (size_t)row * a.words);
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
    const uint32_t e = first + u * kSumThreads;
    uint64_t acc = 0;
    HX_UNROLL
    for (uint32_t t = 0; t < kTapTerms; ++t) acc += sc[t] * v[t][u];
    if (e < a.words) po[e] = acc;
  }
}

static void launch_tap_sum(hipStream_t st, const TapTable &a) {
  HX_PANIC_IF_FALSE(a.words >= 1 && a.inputs >= 1 && a.groups >= 1 && a.groups <= kTapGroups,
                    "tap_sum: %u words, %u inputs, %u groups", a.words, a.inputs, a.groups);
  uint32_t widest = 0;
  for (uint32_t g = 0; g < a.groups; ++g) {
    const TapGroup &G = a.g[g];
    HX_PANIC_IF_FALSE(G.out && G.bits >= 1 && G.terms >= 1 && G.terms <= kTapTerms, "tap_sum: group %u has %u bits, %u terms",
                      g, G.bits, G.terms);
    widest = std::max(widest, G.bits);
    for (uint32_t t = 0; t < G.terms; ++t)
      HX_PANIC_IF_FALSE(G.t[t].src && (G.t[t].step == 1 || (G.t[t].step == -1 && G.t[t].pos + 1 >= G.bits)),
                        "tap_sum: term %u of group %u: null source, or direction %d from position %u over %u bits", t, g,
                        G.t[t].step, G.t[t].pos, G.bits);
  }
  HX_PANIC_IF_FALSE((uint64_t)widest * a.inputs <= 0x7fffffffu, "tap_sum: %u bits of %u inputs in one launch", widest, a.inputs);
  // the rows group g writes against the rows any group reads
  const size_t rw = (size_t)a.inputs * a.words;
  for (uint32_t g = 0; g < a.groups; ++g) {
    const uint64_t *o0 = a.g[g].out, *o1 = o0 + a.g[g].bits * rw;
    for (uint32_t h = 0; h < a.groups; ++h)
      for (uint32_t t = 0; t < a.g[h].terms; ++t) {
        const TapTerm &T = a.g[h].t[t];
        const uint32_t lo = T.step < 0 ? T.pos + 1 - a.g[h].bits : T.pos;
        const uint64_t *s0 = T.src + lo * rw, *s1 = s0 + a.g[h].bits * rw;
        HX_PANIC_IF_FALSE(o1 <= s0 || s1 <= o0, "tap_sum: the output of group %u overlaps the rows term %u of group %u reads",
                          g, t, h);
      }
  }
  HX_LAUNCH(lwe_tap_sum_kernel, dim3(widest * a.inputs, (a.words + kSumChunk - 1) / kSumChunk, a.groups), dim3(kSumThreads),
            0, st, a);
}

// ------------------------------------------------------------------ the cipher on the round driver
// num_inputs = N ciphers side by side; position p of a register occupies rows p N .. p N + N - 1; bits are 0 / 1 in the
// message space.  One batch = 64 steps: every tap sits at position 65 or above, so step s reads position tap - s of the
// batch's starting state, and the bit it produces ends at position 63 - s.  With q = 63 - s, bit q of a batch reads
// position tap - 63 + q and becomes position q: the batch's own row order is the position order.
//
// Two rounds per batch (the reference runs three: it flushes t3 = c65 + c110 before the AND gates, which do not read it):
//   launch 1: the AND packs msg lhs + rhs of (c109, c108), (a91, a90), (b82, b81) and, when a keystream is wanted, c65 + c110
//   round 1:  192 N rows with the AND table, 64 N rows with x & 1 — one round whose rows carry their table index
//   launch 2: new_a = t3 + a68 + and_a, new_b = a65 + a92 + b77 + and_b, new_c = b68 + b83 + c86 + and_c,
//             z = a65 + a92 + b68 + b83 + t3 (five terms); without a keystream new_a = c65 + c110 + a68 + and_a, four
//             terms of noise level 1: t3 needs no flush when no z is formed
//   round 2:  x & 1 on all of them; its output index writes the register bits straight below the heads of the tapes and z
//             in step order
// A row is at most max(msg + 1, 5) in value and in noise level.
//
// State tapes: one per register, (bits + 64 window) N rows.  A call loads the caller's registers at the top; every batch
// moves the head 64 positions down and nothing is shifted; after `window` batches one launch re-bases the tapes; the
// last launch of a call writes the registers back in the caller's layout.  The output index tables of all head positions
// are built by the scratch call: a batch uploads nothing.
// Bootstraps per batch: 384 N without keystream, 512 N with it; a warm-up of 18 batches is 6,912 N in 36 rounds (the
// reference: 8,067 N in 54 rounds, 3 of them on the constant ones of c, which are trivial encryptions here).
constexpr uint32_t kTriviumBatch = 64, kTriviumWarmupBatches = 18, kTriviumKeyBits = 80;
constexpr uint32_t kTriviumBits[3] = {93, 84, 111};  // registers a, b, c
enum : uint32_t { kRegA = 0, kRegB = 1, kRegC = 2 };

// the largest value and noise level a row reaches at message modulus msg
static uint32_t trivium_peak(uint32_t msg) { return std::max(msg + 1, 5u); }

struct TriviumMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x54525631;  // "TRV1"
  LutDriver drv;  // LUT 0: AND of a packed pair, LUT 1: x & 1
  uint32_t inputs = 0;
  uint32_t window = kTriviumWarmupBatches;  // batches between two re-basings (a test hook lowers it)
  uint32_t window_max = kTriviumWarmupBatches;  // what the tapes and the index tables were built for
  bool warmup = false;  // the scratch of trivium_init
  // d_state: tape a | tape b | tape c | 64 N rows in which a batch's keystream lands in step order; the output index of
  // round 2 counts rows of d_state
  uint64_t *d_state = nullptr, *d_in = nullptr, *d_r1 = nullptr, *d_ones = nullptr;
  uint64_t *i_lut1 = nullptr, *i_lut2 = nullptr, *i_out = nullptr;  // i_out: [head / 64 - 1][group][q][n]
  size_t tape_row[3] = {0, 0, 0}, stage_row = 0;  // first rows inside d_state
  DeviceBlocks own;

  uint64_t batch_pbs(bool keystream) const { return (uint64_t)(keystream ? 512 : 384) * inputs; }
  uint64_t pbs_count(uint32_t num_steps) const {
    return warmup ? kTriviumWarmupBatches * batch_pbs(false) : (uint64_t)(num_steps / kTriviumBatch) * batch_pbs(true);
  }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t num_inputs, bool is_warmup, const char *who) {
    const uint32_t peak = trivium_peak(p.msg), space = p.msg * p.carry;
    HX_PANIC_IF_FALSE(num_inputs >= 1 && num_inputs <= (1u << 16), "%s: %u inputs", who, num_inputs);
    HX_PANIC_IF_FALSE(peak <= space - 1 && peak <= (space - 1) / (p.msg - 1),
                      "%s: moduli (%u, %u) do not hold the value and noise level %u a row reaches", who, p.msg, p.carry, peak);
    inputs = num_inputs, warmup = is_warmup;
    const uint32_t N = inputs, B = kTriviumBatch, W = window_max;
    const uint64_t msg = p.msg;
    const size_t lw = (size_t)(p.k + 1) * p.N, w = (size_t)p.big_n + 1;
    std::vector<std::vector<uint64_t>> luts(2, std::vector<uint64_t>(lw));
    generate_lut(p, luts[0].data(), [msg](uint64_t x) -> uint64_t { return (x / msg) & (x % msg) & 1; });
    generate_lut(p, luts[1].data(), [](uint64_t x) -> uint64_t { return x & 1; });
    drv.init(ss, p, std::min<uint32_t>(4 * B * N, 1u << 16), luts);
    size_t rows = 0;
    for (uint32_t r = 0; r < 3; ++r) tape_row[r] = rows, rows += (size_t)(kTriviumBits[r] + B * W) * N;
    stage_row = rows, rows += (size_t)B * N;
    own.alloc(d_state, rows * w * sizeof(uint64_t));
    own.alloc(d_in, (size_t)4 * B * N * w * sizeof(uint64_t));
    own.alloc(d_r1, (size_t)4 * B * N * w * sizeof(uint64_t));
    const hipStream_t st = S0(ss);
    const size_t G = (size_t)B * N;
    std::vector<uint64_t> l1(4 * G), l2(4 * G, 1), oi((size_t)W * 4 * G);
    for (size_t i = 0; i < l1.size(); ++i) l1[i] = i < 3 * G ? 0 : 1;
    for (uint32_t k = 1; k <= W; ++k)  // head at position 64 k: the new bits become positions 64 (k - 1) .. 64 k - 1
      for (uint32_t g = 0; g < 4; ++g)
        for (uint32_t q = 0; q < B; ++q)
          for (uint32_t n = 0; n < N; ++n)
            oi[((size_t)(k - 1) * 4 + g) * G + (size_t)q * N + n] =
                g < 3 ? tape_row[g] + (size_t)(B * (k - 1) + q) * N + n : stage_row + (size_t)(B - 1 - q) * N + n;
    i_lut1 = own.upload(st, l1), i_lut2 = own.upload(st, l2), i_out = own.upload(st, oi);
    if (warmup) {  // the three ones of c: trivial encryptions
      std::vector<uint64_t> ones((size_t)3 * N * w, 0);
      for (uint32_t i = 0; i < 3 * N; ++i) ones[(size_t)i * w + w - 1] = p.delta();
      d_ones = own.upload(st, ones);
    }
  }

  uint64_t *tape(uint32_t r) const { return d_state + tape_row[r] * ((size_t)drv.p.big_n + 1); }
  uint32_t tape_positions(uint32_t r) const { return kTriviumBits[r] + kTriviumBatch * window_max; }
  // bit q of the batch whose state starts at position `head` of the tapes reads register position tap - 63 + q
  TapTerm tap(uint32_t r, uint32_t position, uint32_t head, uint64_t scalar = 1) const {
    HX_PANIC_IF_FALSE(position >= kTriviumBatch - 1 && position < kTriviumBits[r] && head + position < tape_positions(r),
                      "trivium: tap %u of register %u at head %u leaves the tape", position, r, head);
    return TapTerm{tape(r), scalar, head + position - (kTriviumBatch - 1), 1};
  }
  // group g of the rows a round wrote or will read (d_in, d_r1)
  TapTerm round_rows(const uint64_t *base, uint32_t g) const {
    return TapTerm{base + (size_t)g * kTriviumBatch * inputs * ((size_t)drv.p.big_n + 1), 1, 0, 1};
  }
  static TapGroup group(uint64_t *out, uint32_t bits, std::initializer_list<TapTerm> terms) {
    TapGroup g{};
    g.out = out, g.bits = bits, g.terms = (uint32_t)terms.size();
    std::copy(terms.begin(), terms.end(), g.t);
    return g;
  }
  TapTable table(std::initializer_list<TapGroup> groups) const {
    TapTable t{};
    t.words = drv.p.big_n + 1, t.inputs = inputs, t.groups = (uint32_t)groups.size();
    std::copy(groups.begin(), groups.end(), t.g);
    return t;
  }
  // register r as it stands at `head` <-> rows in the caller's layout (or the same register at another head)
  TapTable move_registers(uint64_t *const to[3], const uint64_t *const from[3], uint32_t to_pos, uint32_t from_pos) const {
    const size_t rw = (size_t)inputs * (drv.p.big_n + 1);
    TapTable t = table({});
    t.groups = 3;
    for (uint32_t r = 0; r < 3; ++r) t.g[r] = group(to[r] + to_pos * rw, kTriviumBits[r], {TapTerm{from[r], 1, from_pos, 1}});
    return t;
  }

  // `batches` batches on the registers loaded at the top of the tapes; keystream: the caller's rows, or null (warm-up)
  void run_batches(const CudaStreamsFFI &ss, uint32_t batches, uint64_t *keystream, void *const *ksks, void *const *bsks) {
    const Params &p = drv.p;
    const hipStream_t st = S0(ss);
    const uint32_t N = inputs, B = kTriviumBatch;
    const size_t w = (size_t)p.big_n + 1, G = (size_t)B * N;
    const uint64_t msg = p.msg;
    const bool z = keystream != nullptr;
    const uint32_t rows = (uint32_t)((z ? 4 : 3) * G);
    uint64_t *in[4] = {d_in, d_in + G * w, d_in + 2 * G * w, d_in + 3 * G * w};
    uint64_t *const tapes[3] = {tape(kRegA), tape(kRegB), tape(kRegC)};
    uint32_t head = B * window;
    for (uint32_t b = 0; b < batches; ++b) {
      if (head == 0) {  // re-base: the registers return to the top of the tapes
        launch_tap_sum(st, move_registers(tapes, tapes, B * window, 0));
        head = B * window;
      }
      HX_RANGE("trivium batch %u of %u: %u inputs", b + 1, batches, N);
      TapTable t1 = table({group(in[0], B, {tap(kRegC, 109, head, msg), tap(kRegC, 108, head)}),
                           group(in[1], B, {tap(kRegA, 91, head, msg), tap(kRegA, 90, head)}),
                           group(in[2], B, {tap(kRegB, 82, head, msg), tap(kRegB, 81, head)}),
                           group(in[3], B, {tap(kRegC, 65, head), tap(kRegC, 110, head)})});
      if (!z) t1.groups = 3;
      launch_tap_sum(st, t1);
      drv.round(ss, d_r1, nullptr, d_in, nullptr, i_lut1, rows, ksks, bsks);
      const TapGroup new_a = z ? group(in[0], B, {round_rows(d_r1, 3), tap(kRegA, 68, head), round_rows(d_r1, 0)})
                               : group(in[0], B, {tap(kRegC, 65, head), tap(kRegC, 110, head), tap(kRegA, 68, head),
                                                  round_rows(d_r1, 0)});
      TapTable t2 = table({new_a,
                           group(in[1], B, {tap(kRegA, 65, head), tap(kRegA, 92, head), tap(kRegB, 77, head), round_rows(d_r1, 1)}),
                           group(in[2], B, {tap(kRegB, 68, head), tap(kRegB, 83, head), tap(kRegC, 86, head), round_rows(d_r1, 2)}),
                           group(in[3], B, {tap(kRegA, 65, head), tap(kRegA, 92, head), tap(kRegB, 68, head), tap(kRegB, 83, head),
                                            round_rows(d_r1, 3)})});
      if (!z) t2.groups = 3;
      launch_tap_sum(st, t2);
      drv.round(ss, d_state, i_out + (size_t)(head / B - 1) * 4 * G, d_in, nullptr, i_lut2, rows, ksks, bsks);
      // the round driver scatters relative to ONE base, and the caller's keystream is another allocation than the tapes:
      // the batch's z rows, already in step order, move with one contiguous copy
      if (z)
        HX_CHECK(hipMemcpyAsync(keystream + (size_t)b * G * w, d_state + stage_row * w, G * w * sizeof(uint64_t),
                                hipMemcpyDeviceToDevice, st));
      head -= B;
    }
    last_head = head;
  }
  uint32_t last_head = 0;

  void check_count(uint64_t before, uint64_t want, const char *who) const {
    HX_PANIC_IF_FALSE(drv.issued - before == want, "%s: %llu bootstraps issued, %llu counted", who,
                      (unsigned long long)(drv.issued - before), (unsigned long long)want);
  }

  // trivium_step: num_steps / 64 batches with keystream on the caller's registers
  void step(const CudaStreamsFFI &ss, uint64_t *const regs[3], uint64_t *keystream, uint32_t num_steps, void *const *ksks,
            void *const *bsks) {
    const uint64_t before = drv.issued;
    const uint64_t *const from[3] = {regs[0], regs[1], regs[2]};
    uint64_t *const tapes[3] = {tape(kRegA), tape(kRegB), tape(kRegC)};
    const uint64_t *const tapes_c[3] = {tapes[0], tapes[1], tapes[2]};
    launch_tap_sum(S0(ss), move_registers(tapes, from, kTriviumBatch * window, 0));
    run_batches(ss, num_steps / kTriviumBatch, keystream, ksks, bsks);
    launch_tap_sum(S0(ss), move_registers(regs, tapes_c, 0, last_head));
    check_count(before, pbs_count(num_steps), "trivium_step");
  }

  // trivium_init: a[i] = key[79 - i], b[i] = iv[79 - i], c[108 .. 110] = 1, the rest 0, then 18 batches without keystream
  void warm_up(const CudaStreamsFFI &ss, uint64_t *const regs[3], const uint64_t *key, const uint64_t *iv, void *const *ksks,
               void *const *bsks) {
    const uint64_t before = drv.issued;
    const hipStream_t st = S0(ss);
    const uint32_t head = kTriviumBatch * window, K = kTriviumKeyBits;
    const size_t rw = (size_t)inputs * (drv.p.big_n + 1), rb = rw * sizeof(uint64_t);
    uint64_t *const tapes[3] = {tape(kRegA), tape(kRegB), tape(kRegC)};
    const uint64_t *const tapes_c[3] = {tapes[0], tapes[1], tapes[2]};
    HX_CHECK(hipMemsetAsync(tapes[kRegA] + (head + K) * rw, 0, (kTriviumBits[kRegA] - K) * rb, st));
    HX_CHECK(hipMemsetAsync(tapes[kRegB] + (head + K) * rw, 0, (kTriviumBits[kRegB] - K) * rb, st));
    HX_CHECK(hipMemsetAsync(tapes[kRegC] + head * rw, 0, (kTriviumBits[kRegC] - 3) * rb, st));
    HX_CHECK(hipMemcpyAsync(tapes[kRegC] + (head + kTriviumBits[kRegC] - 3) * rw, d_ones, 3 * rb, hipMemcpyDeviceToDevice, st));
    launch_tap_sum(st, table({group(tapes[kRegA] + head * rw, K, {TapTerm{key, 1, K - 1, -1}}),
                              group(tapes[kRegB] + head * rw, K, {TapTerm{iv, 1, K - 1, -1}})}));
    run_batches(ss, kTriviumWarmupBatches, nullptr, ksks, bsks);
    launch_tap_sum(st, move_registers(regs, tapes_c, 0, last_head));
    check_count(before, pbs_count(0), "trivium_init");
  }

  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    own.release(S0(ss));
  }
};

// One batch's data movement composed from the primitives the layer had before the kernel, in the reference's order
// (trivium.cuh:110-275; tools/bench_trivium.py times it against the two tap launches): pairwise additions for t1, t2, t3,
// six copies into the AND packs and the pack itself, two additions each for new_a, new_b, new_c and z, four copies into
// the flush pack, three copies per register for shift-and-insert, and the keystream reversed row group by row group
// through a workspace.  The rounds themselves are not run: r1 / r2 stand for their outputs ([and_a | and_b | and_c | t3]
// and [a | b | c | z], 64 N rows each).  in1 / in2 receive what the two tap launches form.
// tmp: (111 + 12 * 64) N rows.
static void trivium_batch_baseline(hipStream_t st, uint64_t *const regs[3], uint64_t *in1, const uint64_t *r1, uint64_t *in2,
                                   const uint64_t *r2, uint64_t *keystream, uint64_t *tmp, uint32_t words, uint32_t N,
                                   uint64_t msg) {
  const uint32_t B = kTriviumBatch;
  const size_t rw = (size_t)N * words, G = (size_t)B * rw, gb = G * sizeof(uint64_t);
  const uint32_t rows = B * N;
  uint64_t *ws = tmp, *t1 = ws + 111 * rw, *t2 = t1 + G, *lhs = t2 + G, *rhs = lhs + 3 * G, *na = rhs + 3 * G, *nb = na + G,
           *nc = nb + G, *zz = nc + G;
  uint64_t *t3 = in1 + 3 * G;  // flushed where it is formed
  const uint64_t *a = regs[0], *b = regs[1], *c = regs[2];
  const auto slice = [&](const uint64_t *reg, uint32_t tap) { return reg + (size_t)(tap - (B - 1)) * rw; };
  const auto add = [&](uint64_t *out, const uint64_t *x, const uint64_t *y) {
    axpy(st, out, nullptr, x, nullptr, 1, y, nullptr, words, rows);
  };
  const auto copy = [&](uint64_t *out, const uint64_t *x, size_t bytes) {
    HX_CHECK(hipMemcpyAsync(out, x, bytes, hipMemcpyDeviceToDevice, st));
  };
  add(t1, slice(a, 65), slice(a, 92));
  add(t2, slice(b, 68), slice(b, 83));
  add(t3, slice(c, 65), slice(c, 110));
  copy(lhs, slice(c, 109), gb), copy(lhs + G, slice(a, 91), gb), copy(lhs + 2 * G, slice(b, 82), gb);
  copy(rhs, slice(c, 108), gb), copy(rhs + G, slice(a, 90), gb), copy(rhs + 2 * G, slice(b, 81), gb);
  axpy(st, in1, nullptr, lhs, nullptr, msg, rhs, nullptr, words, 3 * rows);
  const uint64_t *t3f = r1 + 3 * G;
  add(na, t3f, slice(a, 68)), add(na, na, r1);
  add(nb, t1, slice(b, 77)), add(nb, nb, r1 + G);
  add(nc, t2, slice(c, 86)), add(nc, nc, r1 + 2 * G);
  add(zz, t1, t2), add(zz, zz, t3f);
  copy(in2, na, gb), copy(in2 + G, nb, gb), copy(in2 + 2 * G, nc, gb), copy(in2 + 3 * G, zz, gb);
  for (uint32_t r = 0; r < 3; ++r) {  // shift_and_insert_batch
    const size_t keep = (size_t)(kTriviumBits[r] - B) * rw;
    copy(ws, r2 + r * G, gb);
    copy(ws + G, regs[r], keep * sizeof(uint64_t));
    copy(regs[r], ws, gb + keep * sizeof(uint64_t));
  }
  copy(keystream, r2 + 3 * G, gb);
  for (uint32_t i = 0; i < B; ++i) copy(ws + (size_t)(B - 1 - i) * rw, keystream + (size_t)i * rw, rw * sizeof(uint64_t));
  copy(keystream, ws, gb);
}

}  // namespace radix
}  // namespace tfhe_hip
