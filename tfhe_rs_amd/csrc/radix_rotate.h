// radix_rotate.h — the fused rotate-and-pack kernel of the shift / rotate family: one launch builds the packed inputs of a
// barrel-shifter stage (or of a scalar rotation's bivariate round) from rows that stay where they are.
// Included by integer.hip only (one translation unit owns the kernel).
//
// Replaces, per barrel stage of cuda/src/integer/shift_and_rotate.cuh:180-250: a device copy of the bit rows, a block
// rotation into a second buffer, a memset or up to 2^d single-row copies of the sign row, a bivariate pack and an
// add-one-row-to-all — here every output row is written exactly once.
#pragma once
#include "hx.h"
#include "radix_sum.h"

#include <cstdint>

namespace tfhe_hip {
namespace radix {

// out[c R + i] = s0 x[c R + i] + s1 pick(i) + (ctrl ? ctrl[c ctrl_stride + ctrl_row] : 0), on u64 words modulo 2^64.
// c: integer of the batch (blockIdx.z), R rows per integer, i: row (blockIdx.x), blockIdx.y: slice of kSumChunk words.
// pick(i) is row j = i - r (dir = kTowardsHigher: values move to higher rows, a left shift) or j = i + r (kTowardsLower)
// of the same integer; a j outside 0 .. R - 1 is taken modulo R (kPickWrap), contributes nothing (kPickZero) or is the row
// pad[c pad_stride + pad_row] (kPickRow).  0 <= r < R.
// The source row, the padding decision and the control row depend on blockIdx only: they are workgroup-uniform, computed
// on the scalar unit, and no index table exists.  Rows are big_n + 1 words, an odd count, so a row is only 8-byte aligned:
// 8-byte accesses, consecutive lanes on consecutive words; the (up to) six loads of a lane are issued before its adds and
// its two stores.  No LDS, no scratch.  `out` must not overlap `x` (a row is read by another workgroup than the one that
// writes it): the launcher refuses it.
enum : uint32_t { kTowardsHigher = 0, kTowardsLower = 1 };
enum : uint32_t { kPickWrap = 0, kPickZero = 1, kPickRow = 2 };

struct RotatePack {
  uint64_t *out;
  const uint64_t *x, *pad, *ctrl;  // pad: kPickRow only; ctrl: may be null
  uint64_t s0, s1;
  uint32_t words, rows, r, dir, mode;
  uint32_t pad_stride, pad_row, ctrl_stride, ctrl_row;
};

__global__ void __launch_bounds__(kSumThreads) lwe_rotate_pack_kernel(RotatePack a) {
  const uint32_t i = blockIdx.x, c = blockIdx.z, first = blockIdx.y * kSumChunk + threadIdx.x;
  // all of this is uniform over the workgroup
  const uint32_t R = a.rows;
  uint32_t j = a.dir == kTowardsHigher ? i + R - a.r : i + a.r;  // the source row + R (dir 0) or as it is (dir 1)
  const bool outside = a.dir == kTowardsHigher ? j < R : j >= R;
  if (j >= R) j -= R;
  const uint64_t *px = a.x + ((size_t)c * R + i) * a.words;
  const uint64_t *pp = a.x + ((size_t)c * R + j) * a.words;
  bool have = true;
  if (outside && a.mode == kPickZero) have = false;
  if (outside && a.mode == kPickRow) pp = a.pad + ((size_t)c * a.pad_stride + a.pad_row) * a.words;
  const uint64_t *pc = a.ctrl ? a.ctrl + ((size_t)c * a.ctrl_stride + a.ctrl_row) * a.words : nullptr;
  uint64_t vx[kSumWordsPerThread], vp[kSumWordsPerThread], vc[kSumWordsPerThread];
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
    const uint32_t e = first + u * kSumThreads;
    const bool in = e < a.words;
    vx[u] = in ? px[e] : 0;
    vp[u] = (in && have) ? pp[e] : 0;
    vc[u] = (in && pc) ? pc[e] : 0;
  }
  uint64_t *po = a.out + ((size_t)c * R + i) * a.words;
  HX_UNROLL
  for (uint32_t u = 0; u < kSumWordsPerThread; ++u) {
    const uint32_t e = first + u * kSumThreads;
    if (e < a.words) po[e] = a.s0 * vx[u] + a.s1 * vp[u] + vc[u];
  }
}

static void launch_rotate_pack(hipStream_t st, const RotatePack &a, uint32_t batch) {
  if (batch == 0 || a.rows == 0) return;
  const size_t span = (size_t)batch * a.rows * a.words;
  HX_PANIC_IF_FALSE(a.out && a.x && a.words >= 1, "rotate_pack: null pointer or empty rows");
  HX_PANIC_IF_FALSE(a.out + span <= a.x || a.x + span <= a.out, "rotate_pack: the output overlaps the rows it reads");
  HX_PANIC_IF_FALSE(a.r < a.rows && a.dir <= kTowardsLower && a.mode <= kPickRow,
                    "rotate_pack: distance %u on %u rows, direction %u, mode %u", a.r, a.rows, a.dir, a.mode);
  HX_PANIC_IF_FALSE(a.mode != kPickRow || (a.pad && a.pad_row < a.pad_stride), "rotate_pack: padding row %u of %u",
                    a.pad_row, a.pad_stride);
  HX_PANIC_IF_FALSE(!a.ctrl || a.ctrl_row < a.ctrl_stride, "rotate_pack: control row %u of %u", a.ctrl_row, a.ctrl_stride);
  HX_PANIC_IF_FALSE(batch <= 65535, "rotate_pack: %u integers in one launch", batch);
  HX_LAUNCH(lwe_rotate_pack_kernel, dim3(a.rows, (a.words + kSumChunk - 1) / kSumChunk, batch), dim3(kSumThreads), 0, st,
            a);
}

}  // namespace radix
}  // namespace tfhe_hip
