// pbs_generic.h — what the generic PBS kernels of pbs_generic.hip and multibit.hip share: the sample prologue, the LUT
// load, the untwist of the f64 external product, the dispatch over the supported (N, k + 1) shapes and the rule for
// one thread group per GLWE polynomial.  A new ring size is a row of PBS_SHAPES_NK.  Internal to those two files.
#pragma once
#include <type_traits>
#include <utility>

#include "kernels.h"

namespace tfhe_hip {

// ------------------------------------------------------------------------- sample prologue
HX_DEV const uint64_t *sample_lwe(const PbsArgs &a, uint32_t sample) {
  return a.lwe_in + (size_t)a.in_idx[sample] * (a.n + 1);
}
// input ciphertext and accumulator polynomials of launch slot `sample`, through the index vectors
template <int N, int K1>
struct PbsSample {
  const uint64_t *lwe, *lut;
  HX_DEV PbsSample(const PbsArgs &a, uint32_t sample)
      : lwe(sample_lwe(a, sample)), lut(a.lut + (size_t)a.lut_idx[sample] * K1 * N) {}
};
// The recomputation behind a split-key launch runs its flagged ciphertexts only: true = this workgroup has nothing to do
// (uniform across the workgroup); a workgroup that stays counts its ciphertext in `recomputed`.  Call once per kernel.
HX_DEV bool skip_unflagged_and_count(const PbsArgs &a, uint32_t sample, int tid) {
  if (a.only_flagged == nullptr) return false;
  if (a.only_flagged[sample] == 0u) return true;
  if (tid == 0 && a.recomputed != nullptr) atomicAdd(a.recomputed, 1u);
  return false;
}

// acc <- LUT * X^{-b_hat} for the polynomials p0 .. p1 - 1 that a group of TPB threads owns; lt = thread inside the group
template <int N, int TPB>
HX_DEV void block_load_lut(uint64_t *acc, const uint64_t *lut, uint32_t b_hat, int p0, int p1, int lt) {
  for (int p = p0; p < p1; ++p)
    for (uint32_t j = lt; j < (uint32_t)N; j += TPB) {
      bool neg;
      const uint32_t src = monomial_div_src(j, b_hat, N, neg);
      const uint64_t v = lut[p * N + src];
      acc[p * N + j] = neg ? (uint64_t)0 - v : v;
    }
}
// ... and the LUT as it is: the NTT engines rotate last
template <int N, int TPB>
HX_DEV void block_copy_lut(uint64_t *acc, const uint64_t *lut, int p0, int p1, int lt) {
  for (int p = p0; p < p1; ++p)
    for (uint32_t j = lt; j < (uint32_t)N; j += TPB) acc[p * N + j] = lut[p * N + j];
}

// ------------------------------------------------------------------------- f64 external product
// One point y of backward-transformed polynomial p, at transform position j: untwist, then coefficients j and j + N/2
// of that accumulator polynomial += (ADD: the classic CMUX) or = (multi-bit: dst = 0 + product) the torus values.
// Loop-free on purpose: the loop over a thread's points stays in the kernel (docs/history/generic_pbs_refactor_log.md).
template <int N, bool ADD>
HX_DEV void untwist_to_torus(const cplx y, const double *untw, uint64_t *acc, int p, int j) {
  constexpr int n = N / 2;
  const double ur = untw[2 * j], ui = untw[2 * j + 1];
  const double tr = fma(-y.im, ui, y.re * ur);
  const double ti = fma(y.im, ur, y.re * ui);
  if constexpr (ADD) {
    acc[p * N + j] += from_torus(tr);
    acc[p * N + j + n] += from_torus(ti);
  } else {
    acc[p * N + j] = from_torus(tr);
    acc[p * N + j + n] = from_torus(ti);
  }
}

// ------------------------------------------------------------------------- dispatch
// the (N, k + 1) shapes of the generic kernels (N = 8192 / 16384, k = 1: the launchers' own special case)
struct ShapeNK {
  int N, K1;
};
constexpr ShapeNK PBS_SHAPES_NK[] = {{256, 2},  {256, 3},  {256, 4},  {512, 2},  {512, 3},  {512, 4},
                                     {1024, 2}, {1024, 3}, {1024, 4}, {2048, 2}, {2048, 3}, {4096, 2}};

template <class F, size_t... I>
bool dispatch_nk_table(uint32_t N, uint32_t k1, F &f, std::index_sequence<I...>) {
  return ((N == (uint32_t)PBS_SHAPES_NK[I].N && k1 == (uint32_t)PBS_SHAPES_NK[I].K1 &&
           (f(std::integral_constant<int, PBS_SHAPES_NK[I].N>{}, std::integral_constant<int, PBS_SHAPES_NK[I].K1>{}), true)) ||
          ...);
}
// f(N, K1) with the shape as compile-time constants (std::integral_constant); `what` names the PBS in the panic
template <class F>
void dispatch_nk(uint32_t N, uint32_t glwe_dim, const char *what, F &&f) {
  constexpr size_t count = sizeof(PBS_SHAPES_NK) / sizeof(PBS_SHAPES_NK[0]);
  if (!dispatch_nk_table(N, glwe_dim + 1, f, std::make_index_sequence<count>{}))
    HX_PANIC("unsupported (polynomial_size=%u, glwe_dimension=%u) for the %s", N, glwe_dim, what);
}

// A generic product runs with one thread group per GLWE polynomial for k = 1 (43.5k PBS/s at 2_2); with three groups
// (k = 2, N = 1024) the larger workgroup costs more occupancy than the shorter barrier chain returns (45.9k vs 59.0k).
// hip_backend_set_ntt_kernel(1) keeps every shape on the single group.  Only K1 == 2 instantiates a *_par kernel.
inline bool generic_runs_par(int K1) { return K1 == 2 && !g_ntt_kernel_serial; }

}  // namespace tfhe_hip
