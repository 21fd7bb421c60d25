// radix_sum.h — column sums of the radix layer: the planner that the multiplication, the sum of a vector of ciphertexts
// and the scalar multiplication share, and the gather-sum kernel of the two that read their first terms in place.
// Included by integer.hip only (one translation unit owns the kernel).
//
// Replaces: cuda/src/integer/multiplication.cuh:286-485 (host_integer_partial_sum_ciphertexts_vec: chunks of a fixed
// size, a copy of the vector into the work buffer, smart copies between rounds).  Here a round is a CSR of groups over
// term indices; a term stays where it is until a group takes it.
#pragma once
#include "hx.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace tfhe_hip {
namespace radix {

// ------------------------------------------------------------------ gather-sum over two bases
// out[g] = sum of the rows members[offsets[g] .. offsets[g + 1]) name.  A member index with kCallerRow set is a row of
// `caller` (the operand, read in place), without it a row of `pool` (bootstrap outputs of earlier rounds).
// Grid: x = group, y = slice of kSumChunk words (lwe_expand_kernel's layout).  offsets / members depend on blockIdx only:
// they are read once per workgroup, through the scalar unit.  Rows are big_n + 1 words, an odd count, so a row is only
// 8-byte aligned: 8-byte accesses, consecutive lanes on consecutive words.  A lane issues the loads of up to kSumInFlight
// members for its two words before it adds; groups hold (msg carry - 1) / (msg - 1) members at most (5 at (4, 4), 9 at
// (8, 8), 21 at (4, 16)), so one or two passes serve the bases wired and a longer group only loops.  No LDS.
// `out` may be rows of `caller` that the SAME group reads (the sum of a vector into its first integer): a lane reads and
// writes the same words.  Rows another group reads must not be written (the callers go through a dense buffer then).
constexpr uint32_t kSumThreads = 256, kSumWordsPerThread = 2, kSumChunk = kSumThreads * kSumWordsPerThread;
constexpr uint32_t kSumInFlight = 8;
constexpr uint64_t kCallerRow = (uint64_t)1 << 63;

__global__ void __launch_bounds__(kSumThreads) lwe_gather_sum2_kernel(uint64_t *out, const uint64_t *pool,
                                                                      const uint64_t *caller,
                                                                      const uint64_t *__restrict__ offsets,
                                                                      const uint64_t *__restrict__ members,
                                                                      uint32_t words) {
  const uint32_t g = blockIdx.x, first = blockIdx.y * kSumChunk + threadIdx.x;
  const uint64_t lo = offsets[g], hi = offsets[g + 1];
  uint64_t acc[kSumWordsPerThread];
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) acc[u] = 0;
  for (uint64_t m = lo; m < hi; m += kSumInFlight) {
    uint64_t v[kSumInFlight][kSumWordsPerThread];
    HX_UNROLL
    for (uint32_t t = 0; t < kSumInFlight; ++t) {
      const bool live = m + t < hi;  // uniform over the workgroup
      const uint64_t x = members[live ? m + t : m];
      const uint64_t *row = ((x & kCallerRow) ? caller : pool) + (size_t)(x & ~kCallerRow) * words;
      HX_UNROLL
      for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
        const uint32_t e = first + u * kSumThreads;
        v[t][u] = (live && e < words) ? row[e] : 0;
      }
    }
    HX_UNROLL
    for (uint32_t t = 0; t < kSumInFlight; ++t) {
      HX_UNROLL
      for (uint32_t u = 0; u < kSumWordsPerThread; ++u) acc[u] += v[t][u];
    }
  }
  uint64_t *po = out + (size_t)g * words;
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
    const uint32_t e = first + u * kSumThreads;
    if (e < words) po[e] = acc[u];
  }
}
static void launch_gather_sum2(hipStream_t st, uint64_t *out, const uint64_t *pool, const uint64_t *caller,
                               const uint64_t *offsets, const uint64_t *members, uint32_t words, uint32_t groups) {
  if (groups == 0) return;
  HX_LAUNCH(lwe_gather_sum2_kernel, dim3(groups, (words + kSumChunk - 1) / kSumChunk), dim3(kSumThreads), 0, st, out,
            pool, caller, offsets, members, words);
}

// ------------------------------------------------------------------ the planner
// Column sums are planned on the largest value every term can take (its degree).  A group holds at most
// max_terms = (msg carry - 1) / (msg - 1) terms — every term is a fresh bootstrap output or an operand at nominal noise,
// and that count is the noise level the parameter sets are made for (shortint MaxNoiseLevel; it is also the reference's
// fixed chunk in sum_ciphertexts) — whose degrees add up to msg * carry - 1 at most; a group of degree sum S becomes a
// message term (degree min(msg - 1, S)) in its column and, when S >= msg, a carry term (S / msg) in the next one; the
// carry out of the last column is dropped.  A column is finished once it holds at most max_terms terms whose degrees add
// up to final_cap: 2 msg - 2 is what one carry propagation accepts, msg carry - 1 what a block can hold.
struct SumStep {  // one reduction step over term ids
  std::vector<uint64_t> offsets, members;      // CSR of groups
  std::vector<uint64_t> msg_slot, carry_slot;  // the terms a group becomes (carry_slot = ~0 when there is none)
};
struct SumPlan {
  std::vector<SumStep> steps;
  std::vector<std::vector<uint64_t>> final_cols;  // what is left of every column
  uint64_t bootstraps() const {
    uint64_t n = 0;
    for (auto &s : steps)
      for (size_t g = 0; g < s.msg_slot.size(); ++g) n += 1 + (s.carry_slot[g] != ~(uint64_t)0);
    return n;
  }
  size_t max_groups() const {
    size_t g = 0;
    for (auto &s : steps) g = std::max(g, s.msg_slot.size());
    return g;
  }
};

// cols: the first terms of every column, as ids into deg (degree by term id).  New terms take the ids deg.size(), ... in
// the order they are made.
// wide (many integers per call, throughput): a group costs two PBS whatever it holds, so only well-filled groups
// (max_terms terms, or four with degrees adding up to cap - 2 at least) are summed while any column can form one — what is
// left of a column waits for the next step.  Otherwise (latency): every term is grouped at once, the fewest rounds.
// A step that would emit nothing by these rules (a column left as two terms too large to finish, or one term above
// 2 msg - 2) emits every group of two or more terms, and every lone term above 2 msg - 2.
static SumPlan plan_column_sums(std::vector<std::vector<uint64_t>> cols, std::vector<uint32_t> &deg, uint32_t msg,
                                uint32_t carry, bool wide, uint32_t final_cap) {
  const uint32_t L = (uint32_t)cols.size(), m = msg;
  const uint32_t cap = msg * carry - 1, max_terms = cap / (m - 1);
  SumPlan plan;
  auto new_slot = [&](uint32_t d) {
    deg.push_back(d);
    return (uint64_t)deg.size() - 1;
  };
  auto total = [&](const std::vector<uint64_t> &c) {
    uint32_t t = 0;
    for (uint64_t x : c) t += deg[x];
    return t;
  };
  auto finished = [&](const std::vector<uint64_t> &c) { return total(c) <= final_cap && c.size() <= max_terms; };
  auto unfinished = [&]() {
    for (auto &c : cols)
      if (!finished(c)) return true;
    return false;
  };
  while (unfinished()) {
    // first-fit decreasing: the terms of an unfinished column, largest degree first, into groups of capacity cap
    std::vector<std::vector<std::vector<uint64_t>>> groups(L);
    bool any_good = false;
    auto good = [&](const std::vector<uint64_t> &g) {
      return g.size() >= max_terms || (g.size() >= 4 && total(g) + 2 >= cap);
    };
    for (uint32_t c = 0; c < L; ++c) {
      if (finished(cols[c])) continue;
      std::vector<uint64_t> sorted = cols[c];
      std::stable_sort(sorted.begin(), sorted.end(), [&](uint64_t x, uint64_t y) { return deg[x] > deg[y]; });
      for (uint64_t x : sorted) {
        bool placed = false;
        for (auto &g : groups[c])
          if (g.size() < max_terms && total(g) + deg[x] <= cap) {
            g.push_back(x);
            placed = true;
            break;
          }
        if (!placed) groups[c].push_back({x});
      }
      for (auto &g : groups[c]) any_good = any_good || good(g);
    }
    auto by_rule = [&](const std::vector<uint64_t> &g) {
      return g.size() >= 2 && (!wide || (any_good ? good(g) : g.size() >= 3));
    };
    bool stuck = true;
    for (uint32_t c = 0; c < L && stuck; ++c)
      for (auto &g : groups[c])
        if (by_rule(g)) stuck = false;
    SumStep s;
    s.offsets.push_back(0);
    std::vector<std::vector<uint64_t>> nc(L);
    for (uint32_t c = 0; c < L; ++c) {
      if (groups[c].empty()) {  // finished column: stays as it is
        nc[c].insert(nc[c].end(), cols[c].begin(), cols[c].end());
        continue;
      }
      for (auto &g : groups[c]) {
        const bool emit = stuck ? (g.size() >= 2 || deg[g[0]] > 2 * m - 2) : by_rule(g);
        if (!emit) {
          nc[c].insert(nc[c].end(), g.begin(), g.end());
          continue;
        }
        const uint32_t sum = total(g);
        s.members.insert(s.members.end(), g.begin(), g.end());
        s.offsets.push_back(s.members.size());
        const uint64_t ms = new_slot(std::min(m - 1, sum));
        s.msg_slot.push_back(ms);
        nc[c].push_back(ms);
        if (c + 1 < L && sum >= m) {
          const uint64_t cs = new_slot(sum / m);
          s.carry_slot.push_back(cs);
          nc[c + 1].push_back(cs);
        } else {
          s.carry_slot.push_back(~(uint64_t)0);
        }
      }
    }
    HX_PANIC_IF_FALSE(!s.msg_slot.empty(), "column sums: no progress");
    cols.swap(nc);
    plan.steps.push_back(std::move(s));
  }
  plan.final_cols = cols;
  return plan;
}

}  // namespace radix
}  // namespace tfhe_hip
