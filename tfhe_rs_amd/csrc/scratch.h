// scratch.h — the scratch protocol of the C boundary, shared by the core PBS entry points (abi.hip) and the
// radix layer (integer.hip).
// Every object handed out through `int8_t **` starts with ScratchHeader; a struct M derives from it, names its kMagic
// and frees what it declares in release(...).  Only the header of the object that was handed out is stamped and checked: a
// scratch that is a member of another one keeps its release() and nothing else of the protocol.
#pragma once
#include "hx.h"

namespace tfhe_hip {

struct ScratchHeader {
  uint32_t magic = 0;      // M::kMagic while the object is alive (offset 0: scratch_magic tells one kind from another)
  bool size_only = false;  // created with allocate_gpu_memory = false: sized, nothing allocated
};
inline uint32_t scratch_magic(const int8_t *mem_ptr) {
  return mem_ptr ? reinterpret_cast<const ScratchHeader *>(mem_ptr)->magic : 0;
}
constexpr const char *kForeignScratch = ": foreign scratch pointer";

// a refusal reads `who` followed by `foreign`
template <class M>
M *scratch_cast(int8_t *mem_ptr, const char *who, const char *foreign = kForeignScratch) {
  auto *h = reinterpret_cast<ScratchHeader *>(mem_ptr);
  HX_PANIC_IF_FALSE(h && h->magic == M::kMagic, "%s%s", who, foreign);
  return static_cast<M *>(h);
}
// use: the scratch a launch was handed, refused if it is of another kind or was only sized
template <class M>
M *scratch_use(int8_t *mem_ptr, const char *who, const char *foreign = kForeignScratch) {
  M *m = scratch_cast<M>(mem_ptr, who, foreign);
  HX_PANIC_IF_FALSE(!m->size_only, "%s: scratch was created with allocate_gpu_memory=false", who);
  return m;
}
// the stamped object behind *mem_ptr
template <class M>
void scratch_hand_out(M *m, bool allocate_gpu_memory, int8_t **mem_ptr) {
  m->magic = M::kMagic;
  m->size_only = !allocate_gpu_memory;
  *mem_ptr = reinterpret_cast<int8_t *>(static_cast<ScratchHeader *>(m));
}
// destroy: the stream is idle before anything is freed (cleanup_* synchronises, pbs_utilities.h:261-271); `args` go to release
template <class M, class... Args>
void scratch_destroy(uint32_t gpu_index, hipStream_t stream, int8_t **mem_ptr, const char *who, const char *foreign,
                     const Args &...args) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  M *m = scratch_cast<M>(*mem_ptr, who, foreign);
  HX_CHECK(hipStreamSynchronize(stream));
  m->release(args...);
  m->magic = 0;
  delete m;
  *mem_ptr = nullptr;
}

}  // namespace tfhe_hip
