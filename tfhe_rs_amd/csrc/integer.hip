// integer.hip — radix-integer layer on top of the KS -> PBS path ("next" row N1 of SURVEY §8):
// a batched apply-LUT round driver and, built from it, carry propagation, addition and
// schoolbook multiplication of radix ciphertexts.
//
// Replaces (host orchestration + three small kernels; all heavy work is the keyswitch and PBS
// kernels of this library):
//   backends/tfhe-cuda-backend/cuda/src/integer/integer.cuh:869-990   apply_univariate_lookup_table
//   .../integer/integer.cuh:1266-1305                                 LUT generation
//   .../integer/integer.cuh (propagate_single_carry), addition.cuh, multiplication.cuh
//   semantics: tfhe/src/integer/server_key/radix_parallel/{add.rs,mul.rs}, shortint bivariate_pbs.rs
//
// MI355X-first differences from the reference's shape:
//   * a CudaRadixCiphertextFFI may hold a BATCH of independent integers ([ciphertext][block], the
//     scratch's num_blocks = blocks per integer); every round is then ONE keyswitch launch and ONE
//     PBS launch over all blocks of all integers (thousands of PBS per launch is where the PBS
//     kernel is efficient), instead of one stream per integer.
//   * rounds are described by device index arrays (gather / scatter / LUT index per block), so no
//     ciphertext is ever moved to be "aligned" for a round.
#include "kernels.h"
#include "pks128.h"
#include "arena.h"
#include "profile.h"
#include "scratch.h"
#include "radix_sum.h"
#include "radix_rotate.h"
#include "../../include/tfhe_hip_backend.h"

#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <vector>

namespace tfhe_hip {
namespace radix {

// ------------------------------------------------------------------ device kernels
// out[oi] = a[ai] * scalar + b[bi]   (b optional), `words` u64 per LWE; null index = identity
__global__ void __launch_bounds__(256) lwe_axpy_kernel(uint64_t *out, const uint64_t *out_idx, const uint64_t *a,
                                                       const uint64_t *a_idx, uint64_t scalar, const uint64_t *b,
                                                       const uint64_t *b_idx, uint32_t words, uint32_t count) {
  const uint32_t s = blockIdx.x;
  if (s >= count) return;
  const size_t oi = out_idx ? out_idx[s] : s, ai = a_idx ? a_idx[s] : s;
  const uint64_t *pa = a + ai * words;
  uint64_t *po = out + oi * words;
  if (b) {
    const uint64_t *pb = b + (b_idx ? b_idx[s] : s) * words;
    for (uint32_t j = threadIdx.x; j < words; j += blockDim.x) po[j] = pa[j] * scalar + pb[j];
  } else {
    for (uint32_t j = threadIdx.x; j < words; j += blockDim.x) po[j] = pa[j] * scalar;
  }
}
// out[g] = sum of pool[members[m]] for m in [offsets[g], offsets[g+1])  (CSR groups)
__global__ void __launch_bounds__(256) lwe_group_sum_kernel(uint64_t *out, const uint64_t *pool,
                                                            const uint64_t *offsets, const uint64_t *members,
                                                            uint32_t words, uint32_t groups) {
  const uint32_t g = blockIdx.x;
  if (g >= groups) return;
  const uint64_t lo = offsets[g], hi = offsets[g + 1];
  for (uint32_t j = threadIdx.x; j < words; j += blockDim.x) {
    uint64_t acc = 0;
    for (uint64_t m = lo; m < hi; ++m) acc += pool[members[m] * words + j];
    out[(size_t)g * words + j] = acc;
  }
}

// Levelled block operations (no bootstrap).  out[s] = -in[s] on every word, the body takes c0 (block 0 of an integer of
// `per` blocks) or c1 (the other blocks) on top: the negation with its correcting term (negation.cuh:20-49), the
// bitwise NOT (bitwise_ops.cuh:164-191) and the plain negation are instances.  In place allowed.
__global__ void __launch_bounds__(256) lwe_negate_const_kernel(uint64_t *out, const uint64_t *in, uint32_t words,
                                                               uint32_t count, uint32_t per, uint64_t c0, uint64_t c1) {
  const uint32_t s = blockIdx.x;
  if (s >= count) return;
  const uint64_t *pi = in + (size_t)s * words;
  uint64_t *po = out + (size_t)s * words;
  const uint64_t c = (s % per) == 0 ? c0 : c1;
  for (uint32_t j = threadIdx.x; j < words; j += blockDim.x) po[j] = ((uint64_t)0 - pi[j]) + (j + 1 == words ? c : 0);
}
// body[s] += scalars[s] * delta (scalar_addition.cuh:14-25): one thread per block
__global__ void __launch_bounds__(256) lwe_body_add_scalars_kernel(uint64_t *v, const uint64_t *scalars, uint32_t words,
                                                                   uint32_t count, uint64_t delta) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < count) v[(size_t)s * words + words - 1] += scalars[s] * delta;
}

static void axpy(hipStream_t st, uint64_t *out, const uint64_t *out_idx, const uint64_t *a, const uint64_t *a_idx,
                 uint64_t scalar, const uint64_t *b, const uint64_t *b_idx, uint32_t words, uint32_t count) {
  if (count == 0) return;
  HX_LAUNCH(lwe_axpy_kernel, dim3(count), dim3(256), 0, st, out, out_idx, a, a_idx, scalar, b, b_idx, words, count);
}

// ------------------------------------------------------------------ host helpers
struct Params {
  uint32_t big_n, small_n, k, N, pbs_base_log, pbs_level, ks_base_log, ks_level, msg, carry, ms_type;
  uint32_t grouping;  // 0: classic PBS; g >= 1: multi-bit PBS with that grouping factor (pbs_type = MULTI_BIT)
  uint64_t delta() const { return ((uint64_t)1 << 63) / ((uint64_t)msg * carry); }  // scaling factor of a block's value
};

static Params make_params(CudaLweBootstrapKeyParamsFFI b, CudaLweKeyswitchKeyParamsFFI k, uint32_t msg, uint32_t carry,
                          uint32_t ms_type) {
  HX_PANIC_IF_FALSE(b.pbs_type == CLASSICAL || b.pbs_type == MULTI_BIT, "radix layer: unknown pbs_type %u", b.pbs_type);
  HX_PANIC_IF_FALSE(b.pbs_type == CLASSICAL || (b.grouping_factor >= 1 && b.grouping_factor <= 4 &&
                                                b.input_lwe_dimension % b.grouping_factor == 0),
                    "radix layer: multi-bit PBS needs a grouping factor in 1..4 dividing the LWE dimension (got %u)",
                    b.grouping_factor);
  HX_PANIC_IF_FALSE(b.glwe_dimension * b.polynomial_size == k.input_lwe_dimension &&
                        k.output_lwe_dimension == b.input_lwe_dimension,
                    "radix layer: keyswitch and bootstrap key dimensions do not chain");
  HX_PANIC_IF_FALSE(msg >= 2 && carry >= msg && (b.polynomial_size % (msg * carry)) == 0,
                    "radix layer: unsupported message/carry moduli (%u, %u)", msg, carry);
  return Params{k.input_lwe_dimension, b.input_lwe_dimension, b.glwe_dimension, b.polynomial_size, b.base_log,
                b.level_count,         k.base_log,            k.level_count,    msg,               carry,
                ms_type,               b.pbs_type == MULTI_BIT ? b.grouping_factor : 0u};
}

// cuda/src/integer/integer.cuh:1266-1305 (generate_lookup_table_with_encoding, same in/out encoding)
static void generate_lut(const Params &p, uint64_t *acc, const std::function<uint64_t(uint64_t)> &f) {
  const uint32_t sup = p.msg * p.carry, box = p.N / sup;
  const uint64_t delta = p.delta();
  std::fill(acc, acc + (size_t)p.k * p.N, 0);
  uint64_t *body = acc + (size_t)p.k * p.N;
  for (uint32_t i = 0; i < sup; ++i)
    for (uint32_t j = i * box; j < (i + 1) * box; ++j) body[j] = f(i) * delta;
  const uint32_t half = box / 2;
  for (uint32_t i = 0; i < half; ++i) body[i] = (uint64_t)0 - body[i];
  std::rotate(body, body + half, body + p.N);
}

// shortint's many-LUT accumulator (tfhe/src/shortint/engine/mod.rs:169-254 fill_many_lut_accumulator): the plaintext
// space is shared by fs.size() functions of inputs below sup / fs.size(); function t sits in sub-table t, which the
// sample extraction reaches at coefficient t * many_lut_stride(p, fs.size())
static uint32_t many_lut_stride(const Params &p, uint32_t fn) { return p.N / fn; }
static void generate_many_lut(const Params &p, uint64_t *acc, const std::vector<std::function<uint64_t(uint64_t)>> &fs) {
  const uint32_t sup = p.msg * p.carry, box = p.N / sup, fn = (uint32_t)fs.size(), inputs = sup / fn;
  const uint64_t delta = p.delta();
  std::fill(acc, acc + (size_t)(p.k + 1) * p.N, 0);
  uint64_t *body = acc + (size_t)p.k * p.N;
  for (uint32_t t = 0; t < fn; ++t)
    for (uint32_t i = 0; i < inputs; ++i)
      for (uint32_t j = 0; j < box; ++j) body[(size_t)t * inputs * box + (size_t)i * box + j] = fs[t](i) * delta;
  const uint32_t half = box / 2;
  for (uint32_t i = 0; i < half; ++i) body[i] = (uint64_t)0 - body[i];
  std::rotate(body, body + half, body + p.N);
}

// scratch_* with allocate_gpu_memory = false only reports the device bytes the scratch would take
// (gpu/ffi.rs:95-132 "size on gpu" queries): allocations are counted, not made, and nothing is uploaded
static thread_local bool t_dry = false;
static thread_local uint64_t t_bytes = 0;
// The owner of a set of device blocks.  Every struct of the layer holds one for the memory it keeps while it lives (`own`)
// and, where it rebuilds index arrays for the shape of a call, a second one that it empties at the rebuild (`shape`); the
// named pointers of the structs are views into these.  release() of a struct releases its members, then its owners.
struct DeviceBlocks {
  std::vector<void *> held;
  void *take(size_t bytes) {
    held.push_back(scratch_alloc(bytes));
    return held.back();
  }
  template <class T>
  void alloc(T *&p, size_t bytes) {
    t_bytes += bytes;
    p = t_dry ? nullptr : (T *)take(bytes);
  }
  template <class T>
  T *upload(hipStream_t st, const std::vector<T> &h) {
    const size_t bytes = h.size() * sizeof(T);
    if (t_dry) t_bytes += bytes;  // (counted by a size query only: a real creation returns less, see scratch_create)
    if (t_dry || h.empty()) return nullptr;
    T *d = (T *)take(bytes);
    HX_CHECK(hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, st));
    HX_CHECK(hipStreamSynchronize(st));  // h may be a temporary
    return d;
  }
  // one block back, for a buffer that grows by being replaced (the caller has waited for its readers)
  void give_back(void *p) {
    const auto it = std::find(held.begin(), held.end(), p);
    HX_PANIC_IF_FALSE(it != held.end(), "radix layer: a device block is given back to an owner that does not hold it");
    held.erase(it);
    scratch_free(p);
  }
  // everything back; nothing happens on an owner that holds nothing (a size query, a member never set up, a second call)
  void release(hipStream_t st) {
    if (held.empty()) return;
    HX_CHECK(hipStreamSynchronize(st));  // launches may still read the blocks
    for (void *p : held) scratch_free(p);
    held.clear();
  }
};

// The KS -> PBS round driver (integer.cuh:869-990): `count` blocks gathered from `in` through in_idx are
// keyswitched, bootstrapped with LUT lut_idx[s] and scattered to out[out_idx[s]].
//
// Multi-GPU (helper_multi_gpu.cuh:170-294, helper_multi_gpu.cu:39-101): the ciphertexts live on the first GPU of
// the stream set; a round over enough blocks is split into contiguous shards by the reference's rule
// (get_num_inputs_on_gpu), GPU 0 works on its shard in place, every other active GPU i receives its shard
// (gathered on GPU 0, one peer copy on stream i), runs the same two launches with ITS key replicas
// (ksks[i], bsks[i]) and scratch, and sends the results back for a scatter on GPU 0.  Events order the streams;
// no host synchronisation, no collective.  The same code runs with several streams on ONE device (the
// reference's debug-fake-multi-gpu idea), which is how the 1-GPU test box exercises it.
// Blocks per GPU from which a round spreads over one more GPU of the stream set.  0 (default): the reference's rule
// (get_active_gpu_count, helper_multi_gpu.cu:16-48) — 12 for multi-bit keys, (compute units of the first GPU) + 1 for
// classic ones; hip_integer_set_multi_gpu_threshold overrides it (tests, tuning).  The crossover on 8 MI355X is not
// measured (one GPU per box): the rule is the reference's, the setter is there to move it.
static std::atomic<uint32_t> g_multi_gpu_min_blocks{0};
static uint32_t multi_gpu_threshold(const Params &p, uint32_t first_gpu) {
  const uint32_t forced = g_multi_gpu_min_blocks.load();
  if (forced != 0) return forced;
  if (p.grouping) return 12;  // THRESHOLD_MULTI_GPU_WITH_MULTI_BIT_PARAMS
  static std::atomic<uint32_t> cus{0};  // get_threshold_multi_gpu_classical: computed once, first GPU's count
  uint32_t c = cus.load();
  if (c == 0) {
    hipDeviceProp_t prop;
    HX_CHECK(hipGetDeviceProperties(&prop, (int)first_gpu));
    c = (uint32_t)prop.multiProcessorCount;
    cus.store(c);
  }
  return c + 1;
}

// Copies between the GPUs of a stream set: direct (peer access enabled once per ordered pair of devices) where the
// devices can reach each other, through a pinned host buffer where they cannot (helper_multi_gpu.cuh:170-294 relies on
// cudaMemcpyPeerAsync's own fallback; here the two paths are explicit so that both are testable).
static std::mutex g_peer_mutex;
static std::map<std::pair<int, int>, bool> g_peer_direct;  // (device that issues the copy, other device) -> direct?
static bool peer_direct(int dev, int other) {
  if (dev == other) return true;
  std::lock_guard<std::mutex> lock(g_peer_mutex);
  auto it = g_peer_direct.find({dev, other});
  if (it != g_peer_direct.end()) return it->second;
  int can = 0, cur = 0;
  HX_CHECK(hipGetDevice(&cur));
  HX_CHECK(hipDeviceCanAccessPeer(&can, dev, other));
  if (can) {
    HX_CHECK(hipSetDevice(dev));
    const hipError_t e = hipDeviceEnablePeerAccess(other, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
    (void)hipGetLastError();
    HX_CHECK(hipSetDevice(cur));
  }
  g_peer_direct[{dev, other}] = can != 0;
  return can != 0;
}

static uint32_t num_inputs_on_gpu(uint32_t total, uint32_t gpu, uint32_t gpus) {  // helper_multi_gpu.cu:71-101
  if (gpus > total) return gpu < total ? 1u : 0u;
  const uint32_t large = (total + gpus - 1) / gpus, small = total / gpus, cutoff = total % gpus;
  return (cutoff != 0 && gpu < cutoff) ? large : small;
}

struct LutDriver {
  Params p{};
  uint32_t cap = 0, num_luts = 0, many_max = 1;
  uint32_t in_n = 0;  // LWE dimension of a round's inputs, the keyswitch key's input dimension: p.big_n, unless the key
                      // casts from another key (compact-list expansion)
  bool no_ks = false;  // the round bootstraps its inputs as they are (dimension in_n = p.small_n): no keyswitch, no
                       // keyswitch key (oblivious random bits)
  mutable uint64_t issued = 0;  // bootstraps of all rounds so far (the operations that publish a count check it against this)
  struct PerGpu {
    uint32_t gpu = 0;
    uint64_t *d_ks = nullptr, *d_luts = nullptr, *d_trivial = nullptr;  // d_trivial = 0, 1, ..., cap - 1
    int8_t *pbs_buf = nullptr;
    // GPUs other than the first: shard buffers on this GPU and their twins on the first GPU
    uint64_t *d_in = nullptr, *d_out = nullptr, *d_lut_idx = nullptr;   // on this GPU
    uint64_t *d0_in = nullptr, *d0_out = nullptr;                       // on the first GPU
    uint64_t *d_many = nullptr;  // first GPU only, drivers created for many-LUT rounds: dense outputs before the scatter
    bool direct = true;          // this GPU and the first one reach each other's memory (peer access enabled)
    uint64_t *h_stage = nullptr; // pinned host buffer for the copies when they do not
    hipEvent_t staged = nullptr, done = nullptr, copied = nullptr;
    DeviceBlocks own, own0;  // the blocks on this GPU; the twins on the first GPU
  };
  std::vector<PerGpu> gpus;

  void scratch_pbs(hipStream_t st, PerGpu &g) {  // (the byte counts the PBS scratch functions return are dropped)
    if (p.grouping)
      scratch_cuda_multi_bit_programmable_bootstrap_64_async(st, g.gpu, &g.pbs_buf, p.k, p.N, p.pbs_level, cap, !t_dry);
    else
      scratch_cuda_programmable_bootstrap_64_async(st, g.gpu, &g.pbs_buf, p.small_n, p.k, p.N, p.pbs_level, cap,
                                                   !t_dry, (enum PBS_MS_REDUCTION_T)p.ms_type);
  }

  // max_many: the most functions one round extracts per bootstrap (sizes the dense output buffers)
  void init(const CudaStreamsFFI &s, const Params &params, uint32_t capacity,
            const std::vector<std::vector<uint64_t>> &luts, uint32_t max_many = 1, uint32_t input_n = 0,
            bool skip_keyswitch = false) {
    HX_PANIC_IF_FALSE(s.gpu_count >= 1 && s.streams != nullptr, "radix layer: empty stream set");
    p = params;
    cap = capacity;
    many_max = std::max(1u, max_many);
    num_luts = (uint32_t)luts.size();
    no_ks = skip_keyswitch;
    in_n = no_ks ? p.small_n : input_n ? input_n : p.big_n;
    const size_t lw = (size_t)(p.k + 1) * p.N, w = (size_t)p.big_n + 1, wi = (size_t)in_n + 1;
    std::vector<uint64_t> triv(cap);
    for (uint32_t i = 0; i < cap; ++i) triv[i] = i;
    gpus.resize(s.gpu_count);
    for (uint32_t i = 0; i < s.gpu_count; ++i) {
      PerGpu &g = gpus[i];
      g.gpu = s.gpu_indexes ? s.gpu_indexes[i] : 0;
      const hipStream_t st = (hipStream_t)s.streams[i];
      HX_CHECK(hipSetDevice((int)g.gpu));
      if (!no_ks) g.own.alloc(g.d_ks, (size_t)cap * (p.small_n + 1) * sizeof(uint64_t));
      g.own.alloc(g.d_luts, std::max<size_t>(1, num_luts) * lw * sizeof(uint64_t));
      for (uint32_t t = 0; t < num_luts && !t_dry; ++t)
        HX_CHECK(hipMemcpyAsync(g.d_luts + t * lw, luts[t].data(), lw * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      g.d_trivial = g.own.upload(st, triv);
      if (i == 0 && many_max > 1) g.own.alloc(g.d_many, (size_t)many_max * cap * w * sizeof(uint64_t));
      if (i > 0) {
        g.own.alloc(g.d_in, (size_t)cap * wi * sizeof(uint64_t));
        g.own.alloc(g.d_out, (size_t)many_max * cap * w * sizeof(uint64_t));
        g.own.alloc(g.d_lut_idx, (size_t)cap * sizeof(uint64_t));
        // An event is recorded on a stream of ITS device only (hipEventRecord rejects a foreign stream): `staged` and
        // `copied` are recorded on the first GPU's stream, `done` on this GPU's; waiting across devices is allowed.
        HX_CHECK(hipSetDevice((int)gpus[0].gpu));
        g.own0.alloc(g.d0_in, (size_t)cap * wi * sizeof(uint64_t));
        g.own0.alloc(g.d0_out, (size_t)many_max * cap * w * sizeof(uint64_t));
        if (!t_dry) {
          HX_CHECK(hipEventCreateWithFlags(&g.staged, hipEventDisableTiming));
          HX_CHECK(hipEventCreateWithFlags(&g.copied, hipEventDisableTiming));
        }
        HX_CHECK(hipSetDevice((int)g.gpu));
        if (!t_dry) {
          HX_CHECK(hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
          // the copies of a round are issued on this GPU's stream in both directions
          g.direct = peer_direct((int)g.gpu, (int)gpus[0].gpu) && peer_direct((int)gpus[0].gpu, (int)g.gpu);
          // host-staged copies: three pinned regions — shard in, its LUT indexes, results out — so that each leg of a copy
          // runs on the stream of the device whose memory it touches and no region is rewritten before its reader is done
          if (!g.direct) HX_CHECK(hipHostMalloc((void **)&g.h_stage, ((size_t)cap * wi + cap + (size_t)many_max * cap * w) * sizeof(uint64_t), 0));
        }
      }
      HX_CHECK(hipStreamSynchronize(st));  // the LUT sources may be temporaries
      scratch_pbs(st, g);
    }
    HX_CHECK(hipSetDevice((int)gpus[0].gpu));
  }

  void ks_pbs(hipStream_t st, const PerGpu &g, uint64_t *out, const uint64_t *out_idx, const uint64_t *in,
              const uint64_t *in_idx, const uint64_t *lut_idx, uint32_t c, const void *ksk, const void *bsk,
              uint32_t many = 1, uint32_t stride = 0) const {
    const uint64_t *small = g.d_ks, *small_idx = g.d_trivial;
    if (no_ks) {
      small = in, small_idx = in_idx;
    } else {
      HX_RANGE("keyswitch (%u blocks, gpu %u)", c, g.gpu);
      cuda_keyswitch_lwe_ciphertext_vector_64_64_async(st, g.gpu, g.d_ks, g.d_trivial, in, in_idx, ksk, in_n, p.small_n,
                                                       p.ks_base_log, p.ks_level, c);
    }
    HX_RANGE("bootstrap (%u blocks, %u functions, gpu %u)", c, many, g.gpu);
    if (p.grouping)
      cuda_multi_bit_programmable_bootstrap_64_async(st, g.gpu, out, out_idx, g.d_luts, lut_idx, small, small_idx, bsk,
                                                     g.pbs_buf, p.small_n, p.k, p.N, p.grouping, p.pbs_base_log,
                                                     p.pbs_level, c, many, stride);
    else
      cuda_programmable_bootstrap_64_async(st, g.gpu, out, out_idx, g.d_luts, lut_idx, small, small_idx, bsk, g.pbs_buf,
                                           p.small_n, p.k, p.N, p.pbs_base_log, p.pbs_level, c, many, stride);
  }

  // One keyswitch, one PBS that extracts `many` functions out of the same accumulator (sample extraction at
  // coefficients t * stride, integer.cuh:1002-1110): function t of block s lands in out block t * count + s.  The
  // PBS kernels place function t at t * (samples of the launch), so the round is ONE launch on the first GPU of the
  // set (count <= cap by construction of the scratch); a stream set with several GPUs is accepted, the others idle.
  void round_many(const CudaStreamsFFI &s, uint64_t *out, const uint64_t *in, const uint64_t *lut_idx, uint32_t count,
                  void *const *ksks, void *const *bsks, uint32_t many, uint32_t stride) const {
    HX_PANIC_IF_FALSE(count <= cap, "apply_many_univariate_lut: more blocks than the scratch was created for");
    issued += count;
    HX_CHECK(hipSetDevice((int)gpus[0].gpu));
    ks_pbs((hipStream_t)s.streams[0], gpus[0], out, gpus[0].d_trivial, in, gpus[0].d_trivial, lut_idx, count, ksks[0],
           bsks[0], many, stride);
  }

  // Copies between this GPU and the first one.  direct: hipMemcpyPeerAsync on this GPU's stream.  Host-staged (no peer
  // access): the device-to-host leg on the stream of the device that owns the source, the host-to-device leg on the stream
  // of the device that owns the destination, ordered by the round's events (staged / done) — a stream never touches another
  // device's memory.  Not reachable on an MI355X node (every pair of GPUs is an xGMI peer): exercised on the
  // CPU tier's device model only.
  uint64_t *h_in(const PerGpu &g) const { return g.h_stage; }
  uint64_t *h_idx(const PerGpu &g) const { return g.h_stage + (size_t)cap * ((size_t)in_n + 1); }
  uint64_t *h_out(const PerGpu &g) const { return h_idx(g) + cap; }

  // one round, split into launches of at most `cap` blocks; a null in_idx / out_idx means "block s".
  // many > 1: every bootstrap extracts `many` functions of its accumulator (coefficients t * stride); out_idx then
  // holds many * count entries, function t of block s goes to out[out_idx[t * count + s]] (the PBS kernels place
  // function t behind the launch's own samples, so these rounds go through a dense buffer and a scatter).
  void round(const CudaStreamsFFI &s, uint64_t *out, const uint64_t *out_idx, const uint64_t *in, const uint64_t *in_idx,
             const uint64_t *lut_idx, uint32_t count, void *const *ksks, void *const *bsks, uint32_t many = 1,
             uint32_t stride = 0) const {
    const size_t w = (size_t)p.big_n + 1, wi = (size_t)in_n + 1;
    HX_PANIC_IF_FALSE(many >= 1 && many <= many_max && (many == 1 || out_idx != nullptr),
                      "radix layer: a round of %u functions per bootstrap on a driver created for %u", many, many_max);
    const uint32_t avail = std::min<uint32_t>(s.gpu_count, (uint32_t)gpus.size());
    const hipStream_t st0 = (hipStream_t)s.streams[0];
    HX_PANIC_IF_FALSE(no_ks || ksks != nullptr, "radix layer: null keyswitch key array");
    const auto ksk_of = [&](uint32_t i) -> const void * { return no_ks ? nullptr : ksks[i]; };
    HX_RANGE("apply lut round (%u blocks)", count);  // integer.cuh:874
    issued += count;
    for (uint32_t off = 0; off < count; off += cap) {
      const uint32_t c = std::min(cap, count - off);
      // helper_multi_gpu.cu:39-48 (get_active_gpu_count): as many GPUs as the round can keep busy
      const uint32_t min_blocks = multi_gpu_threshold(p, gpus[0].gpu);
      const uint32_t active = std::max(1u, std::min(avail, (c + min_blocks - 1) / min_blocks));
      const uint64_t *ii = in_idx ? in_idx + off : nullptr, *oi = out_idx ? out_idx + off : nullptr;
      const uint64_t *in0 = in_idx ? in : in + off * wi;
      uint64_t *out0 = out_idx ? out : out + off * w;
      uint32_t first = num_inputs_on_gpu(c, 0, active);
      // shards of the other GPUs: gather on the first GPU, ship, compute, ship back (all asynchronous)
      uint32_t begin = first;
      for (uint32_t i = 1; i < active; ++i) {
        const PerGpu &g = gpus[i];
        const hipStream_t sti = (hipStream_t)s.streams[i];
        const uint32_t ci = num_inputs_on_gpu(c, i, active);
        if (ci == 0) continue;
        HX_RANGE("scatter %u blocks to gpu %u", ci, g.gpu);  // integer.cuh:958 (the range covers the shard's launches too)
        HX_CHECK(hipSetDevice((int)gpus[0].gpu));
        if (ii)
          axpy(st0, g.d0_in, nullptr, in0, ii + begin, 1, nullptr, nullptr, (uint32_t)wi, ci);
        else  // trivial input indexing: the shard starts at block `begin`
          HX_CHECK(hipMemcpyAsync(g.d0_in, in0 + (size_t)begin * wi, (size_t)ci * wi * sizeof(uint64_t),
                                  hipMemcpyDeviceToDevice, st0));
        const size_t in_bytes = (size_t)ci * wi * sizeof(uint64_t), idx_bytes = (size_t)ci * sizeof(uint64_t),
                     out_bytes = (size_t)many * ci * w * sizeof(uint64_t);
        if (!g.direct) {  // first legs on the first GPU's stream, which owns the sources
          HX_CHECK(hipMemcpyAsync(h_in(g), g.d0_in, in_bytes, hipMemcpyDeviceToHost, st0));
          HX_CHECK(hipMemcpyAsync(h_idx(g), lut_idx + off + begin, idx_bytes, hipMemcpyDeviceToHost, st0));
        }
        HX_CHECK(hipEventRecord(g.staged, st0));
        HX_CHECK(hipSetDevice((int)g.gpu));
        HX_CHECK(hipStreamWaitEvent(sti, g.staged, 0));
        if (g.direct) {
          HX_CHECK(hipMemcpyPeerAsync(g.d_in, (int)g.gpu, g.d0_in, (int)gpus[0].gpu, in_bytes, sti));
          HX_CHECK(hipMemcpyPeerAsync(g.d_lut_idx, (int)g.gpu, lut_idx + off + begin, (int)gpus[0].gpu, idx_bytes, sti));
        } else {
          HX_CHECK(hipMemcpyAsync(g.d_in, h_in(g), in_bytes, hipMemcpyHostToDevice, sti));
          HX_CHECK(hipMemcpyAsync(g.d_lut_idx, h_idx(g), idx_bytes, hipMemcpyHostToDevice, sti));
        }
        ks_pbs(sti, g, g.d_out, g.d_trivial, g.d_in, g.d_trivial, g.d_lut_idx, ci, ksk_of(i), bsks[i], many, stride);
        if (g.direct) HX_CHECK(hipMemcpyPeerAsync(g.d0_out, (int)gpus[0].gpu, g.d_out, (int)g.gpu, out_bytes, sti));
        else HX_CHECK(hipMemcpyAsync(h_out(g), g.d_out, out_bytes, hipMemcpyDeviceToHost, sti));  // second leg below, on st0
        HX_CHECK(hipEventRecord(g.done, sti));
        begin += ci;
      }
      // the first GPU's own shard, in place
      HX_CHECK(hipSetDevice((int)gpus[0].gpu));
      if (many == 1) {
        ks_pbs(st0, gpus[0], out0, oi ? oi : gpus[0].d_trivial, in0, ii ? ii : gpus[0].d_trivial, lut_idx + off, first,
               ksk_of(0), bsks[0]);
      } else {
        ks_pbs(st0, gpus[0], gpus[0].d_many, gpus[0].d_trivial, in0, ii ? ii : gpus[0].d_trivial, lut_idx + off, first,
               ksk_of(0), bsks[0], many, stride);
        for (uint32_t t = 0; t < many; ++t)
          axpy(st0, out, out_idx + (size_t)t * count + off, gpus[0].d_many + (size_t)t * first * w, nullptr, 1, nullptr,
               nullptr, (uint32_t)w, first);
      }
      // results of the other GPUs: scatter on the first GPU
      begin = first;
      for (uint32_t i = 1; i < active; ++i) {
        const PerGpu &g = gpus[i];
        const uint32_t ci = num_inputs_on_gpu(c, i, active);
        if (ci == 0) continue;
        HX_RANGE("gather %u blocks from gpu %u", ci, g.gpu);  // integer.cuh:981
        HX_CHECK(hipStreamWaitEvent(st0, g.done, 0));
        if (!g.direct)
          HX_CHECK(hipMemcpyAsync(g.d0_out, h_out(g), (size_t)many * ci * w * sizeof(uint64_t), hipMemcpyHostToDevice, st0));
        if (many > 1)
          for (uint32_t t = 0; t < many; ++t)
            axpy(st0, out, out_idx + (size_t)t * count + off + begin, g.d0_out + (size_t)t * ci * w, nullptr, 1, nullptr,
                 nullptr, (uint32_t)w, ci);
        else if (oi)
          axpy(st0, out0, oi + begin, g.d0_out, nullptr, 1, nullptr, nullptr, (uint32_t)w, ci);
        else
          HX_CHECK(hipMemcpyAsync(out0 + (size_t)begin * w, g.d0_out, (size_t)ci * w * sizeof(uint64_t),
                                  hipMemcpyDeviceToDevice, st0));
        // the next use of this GPU's staging buffers must wait for the scatter
        HX_CHECK(hipEventRecord(g.copied, st0));
        HX_CHECK(hipSetDevice((int)g.gpu));
        HX_CHECK(hipStreamWaitEvent((hipStream_t)s.streams[i], g.copied, 0));
        HX_CHECK(hipSetDevice((int)gpus[0].gpu));
        begin += ci;
      }
    }
  }

  void release(const CudaStreamsFFI &s) {
    for (uint32_t i = 0; i < (uint32_t)gpus.size(); ++i) {
      PerGpu &g = gpus[i];
      const hipStream_t st = (hipStream_t)s.streams[i < s.gpu_count ? i : 0];
      HX_CHECK(hipSetDevice((int)g.gpu));
      HX_CHECK(hipStreamSynchronize(st));
      if (g.pbs_buf) {
        if (p.grouping)
          cleanup_cuda_multi_bit_programmable_bootstrap_64(st, g.gpu, &g.pbs_buf);
        else
          cleanup_cuda_programmable_bootstrap_64(st, g.gpu, &g.pbs_buf);
      }
      g.own.release(st);
      for (hipEvent_t e : {g.staged, g.done, g.copied})
        if (e) HX_CHECK(hipEventDestroy(e));
      if (g.h_stage) HX_CHECK(hipHostFree(g.h_stage));
      HX_CHECK(hipSetDevice((int)gpus[0].gpu));
      g.own0.release((hipStream_t)s.streams[0]);
    }
    gpus.clear();
  }
};

static hipStream_t S0(const CudaStreamsFFI &s) {
  HX_PANIC_IF_FALSE(s.gpu_count >= 1 && s.streams != nullptr, "radix layer: empty stream set");
  return (hipStream_t)s.streams[0];
}
static uint32_t G0(const CudaStreamsFFI &s) { return s.gpu_indexes ? s.gpu_indexes[0] : 0; }
// every entry point of the radix layer starts on the first GPU of its stream set: scratch_alloc / scratch_free and the index
// uploads act on the thread's CURRENT device, which a host alternating between GPUs may have left elsewhere
static void first_gpu(const CudaStreamsFFI &s) { HX_CHECK(hipSetDevice((int)G0(s))); }

// ------------------------------------------------------------------ scratch protocol (scratch.h) on a stream set
// A struct M of the layer fills itself in a callable given to scratch_create and frees what it declares in
// release(const CudaStreamsFFI &).
// create: the only place that sets the thread's dry-run state; `fill` allocates through the owners (DeviceBlocks).  (The core
// scratch functions a fill calls neither read nor reset that state.)
// Known and kept, a fix changes returned values: a size query counts the index uploads, a real creation does not
// (DeviceBlocks::upload), so the two modes return different numbers; the reference returns one size_tracker in both.
template <class M, class Fill>
static uint64_t scratch_create(const CudaStreamsFFI &s, int8_t **mem_ptr, bool allocate_gpu_memory, const char *who,
                               Fill &&fill) {
  first_gpu(s);
  HX_PANIC_IF_FALSE(mem_ptr != nullptr, "%s: null pointer", who);
  t_dry = !allocate_gpu_memory;
  t_bytes = 0;
  M *m = new M();
  fill(*m);
  t_dry = false;
  scratch_hand_out(m, allocate_gpu_memory, mem_ptr);
  return t_bytes;
}
// destroy (`who` = "cleanup <operation>"): the first stream is idle before anything is freed
template <class M>
static void scratch_destroy(const CudaStreamsFFI &s, int8_t **mem_ptr, const char *who) {
  tfhe_hip::scratch_destroy<M>(G0(s), S0(s), mem_ptr, who, kForeignScratch, s);
}

// ------------------------------------------------------------------ apply a univariate LUT
struct ApplyLutMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x4C555431;  // "LUT1"
  LutDriver drv;
  uint64_t *d_lut_idx = nullptr;  // all zero
  uint64_t degree = 0;
  uint32_t num_many_lut = 1;      // apply_many_univariate_lut: functions packed in the accumulator
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    drv.release(s);
    own.release(S0(s));
  }
};

// ------------------------------------------------------------------ carry propagation
// In place on blocks whose value is <= 2*msg - 2 (the sum of two clean blocks): at most one carry leaves a
// block.  Block states as in radix_parallel/add.rs (OutputCarry): none, generated, propagated.
//
// Carry look-ahead as a TREE OF BINARY ADDITIONS (needs msg*carry >= 16; the same family as the reference's
// advanced_add_assign_with_carry_at_least_4_bits, add.rs:828-1044, which also takes its block states from
// many-LUT bootstraps).  Among up to three neighbours the carries are resolved by an ordinary binary addition of
// their states, which is LINEAR in the ciphertexts:
//   w_q = (generated ? 2 : propagated ? 1 : 0) << q          for the neighbour at position q = 0..2
//   S_q = carry_in + w_0 + ... + w_(q-1)                       LWE additions, no PBS
//   carry into neighbour q = bit q of S_q                      (one PBS, q >= 1)
// because a propagating neighbour (bit q set) forwards an incoming carry to bit q+1, a generating one has bit
// q+1 set whatever arrives, and an absorbing one stops it.  The state of the three TOGETHER is read off
// U = w_0 + w_1 + w_2 (bit 3 of U: a carry leaves without an incoming one; bit 3 of U + 1: with one) by one PBS,
// which emits it already shifted for its own position one level up.  So: blocks -> groups of 3 -> groups of 9
// -> ... until at most 4 elements are left, whose carries are bits 1..3 of the partial sums; then the carries go
// back down, one level per round (the first element of a group takes the carry of its group as it is).
// The blocks themselves take no round of their own on the way down: the first bootstrap of a block (its value is
// below msg*carry / 2, so the accumulator holds two functions) also returns 4 * (value % msg), and the last one
// reads the result off  4 * (value % msg) + z  with z = (state of the blocks before it in its group of three:
// 0 none, 1 propagated, 2 generated) + (carry into the group): the block receives a carry iff z >= 2.
// PBS for 32 blocks: 32 first bootstraps + 10 + 3 group states + 10 states of the first two blocks of a group
// + 3 top carries + 7 carries into the groups + 32 results = 97 in 6 rounds (round 3, before: 107 in 7 with a
// round for the carries into the blocks; a Hillis-Steele scan over groups of four 116 in 8; one per block 224).
enum : uint64_t {
  LUT_FIRST2 = 0,    // many-LUT accumulators [f, 4 (x % msg)]: + q: f = state << q (q = 0..2);
                     // + 3: block 0 of an integer, f = state with "propagated" dropped (nothing can arrive);
                     // + 4: last block of an integer, f = 4 * state (only the output carry reads it)
  LUT_GROUP = 5,     // + 3 (len - 1) + q: U of a group of len = 1..3 -> state of the group << q
  LUT_BIT = 13,      // + q (q = 1..3): S -> bit q of S
  LUT_RES_BIT = 17,  // 4 m + z -> (m + z) % msg, z = the carry itself (first block of a group, or the top level)
  LUT_RES_Z = 18,    // 4 m + z -> (m + (z >= 2)) % msg
  LUT_OUT_BIT = 19,  // 4 state + z -> output carry of the integer, z = the carry into its last block
  LUT_OUT_Z = 20,    // 4 state + z -> the same, the carry into the last block is z >= 2
  LUT_MSG = 21,      // x -> x % msg                  (single-block integers)
  LUT_CARRY = 22,    // x -> x / msg
  // signed overflow of an addition (FLAG_OVERFLOW, integer_utilities.h:2311-2357, :2383-2412): the last blocks of the
  // two operands, packed msg * lhs + rhs BEFORE the addition, give 8 (overflow if a carry arrives) + 4 (if none);
  // the flag is read off that + z, z as in LUT_OUT_*
  LUT_OVF_PREP = 23,
  LUT_OVF_BIT = 24,  // 8 o1 + 4 o0 + z -> z ? o1 : o0      (z = the carry into the last block itself)
  LUT_OVF_Z = 25,    // 8 o1 + 4 o0 + z -> (z >= 2) ? o1 : o0
  LUT_PROP_COUNT = 26
};

struct PropagateMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x50524F50;  // "PROP"
  static constexpr uint32_t G = 3, TOP = 4;       // children per group; elements the top level resolves directly
  LutDriver drv;
  uint32_t blocks = 0;   // blocks per integer
  uint32_t max_cts = 0;  // integers the scratch was sized for
  // scratch ciphertexts: pool = [W of level 0 (the blocks), W of level 1, ... | C of level 0 (top level only), C of
  // level 1, ... | M: 4 (value % msg) of every block | P: state of the first two blocks of every full group | O: the
  // overflow preparation of every integer (FLAG_OVERFLOW)]
  // (shifted states; carries into the elements); P2: dense sums of one round
  uint64_t *d_pool = nullptr, *d_p = nullptr;
  uint32_t cached_cts = 0;
  DeviceBlocks own, shape;  // shape: the index arrays for cached_cts integers
  struct Idx {
    uint64_t *a = nullptr, *b = nullptr, *o = nullptr, *lut = nullptr;
    uint32_t count = 0;
  };
  Idx rA, rTop, rRes, rOut, rOvf, rOvfPrep, rIO, rOne, rLast, rOne1;
  uint64_t *d_pack = nullptr;  // msg * (last block of lhs) + (last block of rhs), one per integer (FLAG_OVERFLOW)
  std::vector<Idx> up, down;  // up[l]: states of level l + 1 from level l; down[l] (l >= 1): carries into level l

  // elements per level: n[0] = blocks, n[l + 1] = ceil(n[l] / 3) until at most TOP are left
  static std::vector<uint32_t> level_sizes(uint32_t L) {
    std::vector<uint32_t> n{L};
    while (n.back() > TOP) n.push_back((n.back() + G - 1) / G);
    return n;
  }
  static uint64_t pool_slots(uint32_t L) {  // per integer
    const auto n = level_sizes(L);
    uint64_t s = L + (n.size() > 1 ? n[1] : 0) + 1;  // M, P, O (overflow preparation of the integer)
    for (uint32_t v : n) s += 2 * (uint64_t)v;   // W, C
    return s;
  }
  // PBS one propagation issues per integer
  static uint64_t pbs_count(uint32_t L) {
    if (L == 1) return 1;
    const auto n = level_sizes(L);
    const size_t top = n.size() - 1;
    uint64_t c = 2 * (uint64_t)L;                     // first bootstraps, results
    for (size_t l = 1; l <= top; ++l) c += n[l] - 1;  // group states (every group but the last of its level)
    if (top >= 1) c += L / G;                         // state of the first two blocks of every full group
    c += n[top] - 1;                                  // carries into the top elements
    for (size_t l = 1; l < top; ++l) c += n[l] - (n[l] + G - 1) / G;  // carries into the groups that are not first in theirs
    return c;
  }

  Idx make(hipStream_t st, const std::vector<uint64_t> &a, const std::vector<uint64_t> &b,
           const std::vector<uint64_t> &o, const std::vector<uint64_t> &l) {
    Idx r;
    r.a = shape.upload(st, a);
    r.b = shape.upload(st, b);
    r.o = shape.upload(st, o);
    r.lut = shape.upload(st, l);
    r.count = (uint32_t)l.size();
    return r;
  }

  void build_indexes(hipStream_t st, uint32_t cts) {
    shape.release(st);  // (waits: launches of the previous shape may still read them)
    up.clear();
    down.clear();
    const uint32_t L = blocks;
    const auto n = level_sizes(L);
    const size_t top = n.size() - 1;
    // pool slots: W[l] at wbase[l] + c n[l] + e, C[l] likewise; M at mbase + c L + j; P at pbase + c n[1] + group
    std::vector<uint64_t> wbase(n.size()), cbase(n.size());
    uint64_t next = 0;
    for (size_t l = 0; l <= top; ++l) wbase[l] = next, next += (uint64_t)cts * n[l];
    for (size_t l = 0; l <= top; ++l) cbase[l] = next, next += (uint64_t)cts * n[l];
    const uint64_t mbase = next;
    next += (uint64_t)cts * L;
    const uint64_t pbase = next;
    next += (uint64_t)cts * (n.size() > 1 ? n[1] : 0);
    const uint64_t obase = next;
    auto O = [&](uint32_t c) { return obase + c; };
    auto W = [&](size_t l, uint32_t c, uint32_t e) { return wbase[l] + (uint64_t)c * n[l] + e; };
    auto M = [&](uint32_t c, uint32_t j) { return mbase + (uint64_t)c * L + j; };
    auto P = [&](uint32_t c, uint32_t g) { return pbase + (uint64_t)c * n[1] + g; };
    auto T = [&](uint32_t c, uint32_t j) { return (uint64_t)c * L + j; };
    auto shift = [&](size_t l, uint32_t e) { return l == top ? e : e % G; };
    // pool slot of the carry into element e of level l (the slot of its group's carry for the first element of
    // a group); e = 0 of an integer receives none
    std::function<int64_t(size_t, uint32_t, uint32_t)> carry_of = [&](size_t l, uint32_t c, uint32_t e) -> int64_t {
      if (e == 0) return -1;
      if (l < top && e % G == 0) return carry_of(l + 1, c, e / G);
      return (int64_t)(cbase[l] + (uint64_t)c * n[l] + e);
    };
    std::vector<uint64_t> a, b, o, lut;
    auto reset = [&]() { a.clear(), b.clear(), o.clear(), lut.clear(); };
    // A (two functions per bootstrap): v[t] -> W[0][t], M[t]; out_idx = [function 0 of every block | function 1]
    for (uint32_t c = 0; c < cts; ++c)
      for (uint32_t j = 0; j < L; ++j) {
        o.push_back(W(0, c, j));
        lut.push_back(LUT_FIRST2 + (j + 1 == L ? 4 : j == 0 ? 3 : shift(0, j)));
      }
    for (uint32_t c = 0; c < cts; ++c)
      for (uint32_t j = 0; j < L; ++j) o.push_back(M(c, j));
    rA = make(st, {}, {}, o, lut);
    // up: U of the children -> shifted state of the parent (CSR over the pool; a = offsets, b = members); with the
    // blocks' round also the state of the first two blocks of every full group of three
    for (size_t l = 0; l < top; ++l) {
      reset();
      a.push_back(0);
      for (uint32_t c = 0; c < cts; ++c) {
        for (uint32_t pp = 0; pp + 1 < n[l + 1]; ++pp) {
          const uint32_t len = std::min(G, n[l] - pp * G);
          for (uint32_t q = 0; q < len; ++q) b.push_back(W(l, c, pp * G + q));
          a.push_back(b.size());
          o.push_back(W(l + 1, c, pp));
          lut.push_back(LUT_GROUP + 3 * (len - 1) + shift(l + 1, pp));
        }
        for (uint32_t pp = 0; l == 0 && pp * G + 2 < L; ++pp) {
          b.push_back(W(0, c, pp * G));
          b.push_back(W(0, c, pp * G + 1));
          a.push_back(b.size());
          o.push_back(P(c, pp));
          lut.push_back(LUT_GROUP + 3 * (2 - 1) + 0);
        }
      }
      up.push_back(make(st, a, b, o, lut));
    }
    // top: carry into element j = bit j of w_0 + .. + w_(j-1)
    reset();
    a.push_back(0);
    for (uint32_t c = 0; c < cts; ++c)
      for (uint32_t j = 1; j < n[top]; ++j) {
        for (uint32_t i = 0; i < j; ++i) b.push_back(W(top, c, i));
        a.push_back(b.size());
        o.push_back((uint64_t)carry_of(top, c, j));
        lut.push_back(LUT_BIT + j);
      }
    rTop = make(st, a, b, o, lut);
    // down (levels >= 1): carry into element e = 3 p + q (q >= 1) = bit q of (carry into p) + w_(3p) + .. + w_(e-1)
    down.resize(top);
    for (size_t l = top; l-- > 1;) {
      reset();
      a.push_back(0);
      for (uint32_t c = 0; c < cts; ++c)
        for (uint32_t e = 0; e < n[l]; ++e) {
          const uint32_t pp = e / G, q = e % G;
          if (q == 0) continue;
          const int64_t cin = carry_of(l + 1, c, pp);
          if (cin >= 0) b.push_back((uint64_t)cin);
          for (uint32_t i = 0; i < q; ++i) b.push_back(W(l, c, pp * G + i));
          a.push_back(b.size());
          o.push_back((uint64_t)carry_of(l, c, e));
          lut.push_back(LUT_BIT + q);
        }
      down[l] = make(st, a, b, o, lut);
    }
    // results: 4 m + z; and the output carry of every integer from 4 (state of the last block) + z
    std::vector<uint64_t> a2{0}, b2, lut2, a3{0}, b3, lut3, o3, l3;
    reset();
    a.push_back(0);
    for (uint32_t c = 0; c < cts; ++c)
      for (uint32_t j = 0; j < L; ++j) {
        const size_t before = b.size();
        bool z_is_bit = true;
        if (top == 0) {
          if (j > 0) b.push_back((uint64_t)carry_of(0, c, j));
        } else {
          const uint32_t pp = j / G, q = j % G;
          const int64_t cin = carry_of(1, c, pp);
          if (cin >= 0) b.push_back((uint64_t)cin);
          if (q == 1) b.push_back(W(0, c, pp * G));
          if (q == 2) b.push_back(P(c, pp));
          z_is_bit = q == 0;
        }
        if (j + 1 == L) {  // the same z next to the last block's state
          b2.insert(b2.end(), b.begin() + (std::ptrdiff_t)before, b.end());
          b2.push_back(W(0, c, j));
          a2.push_back(b2.size());
          lut2.push_back(z_is_bit ? LUT_OUT_BIT : LUT_OUT_Z);
          // ... and next to the overflow preparation
          b3.insert(b3.end(), b.begin() + (std::ptrdiff_t)before, b.end());
          b3.push_back(O(c));
          a3.push_back(b3.size());
          lut3.push_back(z_is_bit ? LUT_OVF_BIT : LUT_OVF_Z);
          o3.push_back(O(c));
          l3.push_back(LUT_OVF_PREP);
        }
        b.push_back(M(c, j));
        a.push_back(b.size());
        lut.push_back(z_is_bit ? LUT_RES_BIT : LUT_RES_Z);
      }
    rRes = make(st, a, b, {}, lut);
    rOut = make(st, a2, b2, {}, lut2);
    rOvf = make(st, a3, b3, {}, lut3);
    rOvfPrep = make(st, {}, {}, o3, l3);
    // optional input carry (added to block 0 of every integer); single-block integers: message and carry of v
    reset();
    std::vector<uint64_t> l1;
    for (uint32_t c = 0; c < cts; ++c) {
      a.push_back(T(c, 0));
      lut.push_back(LUT_CARRY);
      l1.push_back(LUT_MSG);
    }
    rIO = make(st, a, {}, {}, lut);
    rOne = make(st, {}, {}, {}, l1);
    {  // last block of every integer (operand views); single-block integers: the preparation alone as a "group"
      std::vector<uint64_t> last, a1{0}, b1, lo;
      for (uint32_t c = 0; c < cts; ++c) {
        last.push_back(T(c, L - 1));
        b1.push_back(O(c));
        a1.push_back(b1.size());
        lo.push_back(LUT_OVF_BIT);
      }
      rLast = make(st, last, {}, {}, {});
      rOne1 = make(st, a1, b1, {}, lo);
    }
    cached_cts = cts;
  }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t num_blocks, uint32_t cts) {
    blocks = num_blocks;
    max_cts = cts;
    // 4 bits per block: the binary additions of three shifted states; an accumulator of two functions for values up
    // to 2 msg - 1; results packed as 4 (msg - 1) + 3
    HX_PANIC_IF_FALSE(p.msg * p.carry >= 16 && p.carry >= p.msg && 4 * p.msg <= p.msg * p.carry,
                      "carry propagation needs at least 4 bits per block (message_modulus * carry_modulus >= 16)");
    // MESSAGE_1_CARRY_3-class sets (msg = 2) are not covered by any test of this layer: refused, not guessed
    HX_PANIC_IF_FALSE(p.msg >= 3, "carry propagation: message_modulus %u < 3 is not supported", p.msg);
    const uint64_t m = p.msg;
    using F = std::function<uint64_t(uint64_t)>;
    const size_t lw = (size_t)(p.k + 1) * p.N;
    std::vector<std::vector<uint64_t>> luts(LUT_PROP_COUNT, std::vector<uint64_t>(lw, 0));
    auto one = [&](uint64_t id, const F &f) { generate_lut(p, luts[id].data(), f); };
    const F low4 = [m](uint64_t x) -> uint64_t { return 4 * (x % m); };
    for (uint64_t q = 0; q < G; ++q)
      generate_many_lut(p, luts[LUT_FIRST2 + q].data(),
                        {[m, q](uint64_t x) -> uint64_t { return (x >= m ? 2 : (x == m - 1 ? 1 : 0)) << q; }, low4});
    generate_many_lut(p, luts[LUT_FIRST2 + 3].data(), {[m](uint64_t x) -> uint64_t { return x >= m ? 2 : 0; }, low4});
    generate_many_lut(p, luts[LUT_FIRST2 + 4].data(),
                      {[m](uint64_t x) -> uint64_t { return 4 * (x >= m ? 2 : (x == m - 1 ? 1 : 0)); }, low4});
    for (uint64_t len = 1; len <= G; ++len)
      for (uint64_t q = 0; q < G; ++q)
        one(LUT_GROUP + 3 * (len - 1) + q, [len, q](uint64_t u) -> uint64_t {
          const uint64_t h0 = (u >> len) & 1, h1 = ((u + 1) >> len) & 1;  // a carry leaves without / with one coming in
          return (h0 ? 2 : (h1 ? 1 : 0)) << q;
        });
    for (uint64_t q = 1; q <= G; ++q) one(LUT_BIT + q, [q](uint64_t x) -> uint64_t { return (x >> q) & 1; });
    one(LUT_RES_BIT, [m](uint64_t x) -> uint64_t { return ((x >> 2) + (x & 3)) % m; });
    one(LUT_RES_Z, [m](uint64_t x) -> uint64_t { return ((x >> 2) + ((x & 3) >= 2)) % m; });
    // state 2 generated, 1 propagated: a carry leaves if it is generated, or propagated and one arrives
    one(LUT_OUT_BIT, [](uint64_t x) -> uint64_t { return ((x >> 2) + (x & 3)) >= 2; });
    one(LUT_OUT_Z, [](uint64_t x) -> uint64_t { return ((x >> 2) + ((x & 3) >= 2)) >= 2; });
    one(LUT_MSG, [m](uint64_t x) -> uint64_t { return x % m; });
    one(LUT_CARRY, [m](uint64_t x) -> uint64_t { return x / m; });
    {
      uint32_t bits = 0;
      while ((1ull << bits) < m) ++bits;
      // integer_utilities.h:2326-2352 (f_overflow_fp): the carry into the sign bit against the carry out of the block
      one(LUT_OVF_PREP, [m, bits](uint64_t x) -> uint64_t {
        const uint64_t lhs = x / m, rhs = x % m, mask = (1ull << (bits - 1)) - 1;
        uint64_t r = 0;
        for (uint64_t cin = 0; cin < 2; ++cin) {
          const uint64_t out_c = ((lhs + rhs + cin) >> bits) & 1;
          const uint64_t in_c = (((lhs & mask) + (rhs & mask) + cin) >> (bits - 1)) & 1;
          r |= (uint64_t)(in_c != out_c) << (2 + cin);
        }
        return r;
      });
      one(LUT_OVF_BIT, [](uint64_t x) -> uint64_t { return (x & 3) ? (x >> 3) & 1 : (x >> 2) & 1; });
      one(LUT_OVF_Z, [](uint64_t x) -> uint64_t { return (x & 3) >= 2 ? (x >> 3) & 1 : (x >> 2) & 1; });
    }
    const uint32_t T = cts * num_blocks;
    drv.init(ss, p, std::min<uint32_t>(T, 1u << 16), luts, 2);
    const size_t w = p.big_n + 1;
    own.alloc(d_pool, (size_t)cts * pool_slots(num_blocks) * w * sizeof(uint64_t));
    own.alloc(d_p, (size_t)T * w * sizeof(uint64_t));
    own.alloc(d_pack, (size_t)cts * w * sizeof(uint64_t));
    if (!t_dry) build_indexes(S0(ss), cts);  // a call with fewer integers rebuilds them
  }

  // dense sums of a round's CSR groups, then one KS -> PBS round on them
  void summed_round(const CudaStreamsFFI &ss, uint64_t *out, const Idx &r, uint32_t w, void *const *ksks,
                    void *const *bsks) {
    if (r.count == 0) return;
    HX_LAUNCH(lwe_group_sum_kernel, dim3(r.count), dim3(256), 0, S0(ss), d_p, d_pool, r.a, r.b, w, r.count);
    drv.round(ss, out, r.o, d_p, nullptr, r.lut, r.count, ksks, bsks);
  }

  // in place on v (cts integers of `blocks` blocks).  carry_in (one block per integer, value 0/1) is added to
  // block 0 first — a first block of value <= 2 msg - 1 still emits at most one carry and receives none;
  // carry_out (one block per integer) receives the carry leaving the last block.  Either may be null.
  // overflow_out (one block per integer, add_and_propagate only): the signed-overflow flag of the addition whose last
  // operand blocks the caller packed into d_pack before adding (pack_last_blocks).
  void pack_last_blocks(const CudaStreamsFFI &ss, const uint64_t *lhs, const uint64_t *rhs, uint32_t cts) {
    const Params &p = drv.p;
    const uint32_t w = p.big_n + 1;
    // block (c + 1) * blocks - 1 of both operands: strided views, one launch per integer batch through index arrays
    if (cached_cts != cts) build_indexes(S0(ss), cts);
    axpy(S0(ss), d_pack, nullptr, lhs, rLast.a, p.msg, rhs, rLast.a, w, cts);
  }
  void run(const CudaStreamsFFI &ss, uint64_t *v, uint32_t cts, void *const *ksks, void *const *bsks,
           const uint64_t *carry_in = nullptr, uint64_t *carry_out = nullptr, uint64_t *overflow_out = nullptr,
           bool results = true) {  // results = false: only the flags are wanted (comparisons), v is left with its sums
    const hipStream_t st = S0(ss);  // linear operations and index uploads: first GPU only, like the reference
    HX_PANIC_IF_FALSE(cts >= 1 && cts <= max_cts, "carry propagation: %u integers exceed the scratch capacity %u", cts,
                      max_cts);
    if (cached_cts != cts) build_indexes(st, cts);
    const Params &p = drv.p;
    const uint32_t w = p.big_n + 1, T = cts * blocks;
    const size_t top = up.size();
    HX_RANGE("carry propagation: %u integers of %u blocks", cts, blocks);
    if (carry_in) axpy(st, v, rIO.a, v, rIO.a, 1, carry_in, nullptr, w, cts);
    if (overflow_out)  // 8 o1 + 4 o0 of every integer, from the operands' last blocks
      drv.round(ss, d_pool, rOvfPrep.o, d_pack, nullptr, rOvfPrep.lut, cts, ksks, bsks);
    if (blocks == 1) {  // nothing to propagate: the carry leaves the integer
      if (overflow_out) {  // the carry into the only block is the input carry itself
        HX_LAUNCH(lwe_group_sum_kernel, dim3(cts), dim3(256), 0, st, d_p, d_pool, rOne1.a, rOne1.b, w, cts);
        if (carry_in) axpy(st, d_p, nullptr, d_p, nullptr, 1, carry_in, nullptr, w, cts);
        drv.round(ss, overflow_out, nullptr, d_p, nullptr, rOne1.lut, cts, ksks, bsks);
      }
      if (carry_out) drv.round(ss, carry_out, nullptr, v, nullptr, rIO.lut, cts, ksks, bsks);
      if (results) drv.round(ss, v, nullptr, v, nullptr, rOne.lut, cts, ksks, bsks);
      return;
    }
    // A: shifted state and 4 (value % msg) of every block; up: shifted states of the groups, level by level
    drv.round(ss, d_pool, rA.o, v, nullptr, rA.lut, T, ksks, bsks, 2, many_lut_stride(p, 2));
    for (const Idx &r : up) summed_round(ss, d_pool, r, w, ksks, bsks);
    // carries: top level, then down to the groups of three blocks
    summed_round(ss, d_pool, rTop, w, ksks, bsks);
    for (size_t l = top; l-- > 1;) summed_round(ss, d_pool, down[l], w, ksks, bsks);
    // results (and the output carry) from 4 m + z
    if (carry_out) summed_round(ss, carry_out, rOut, w, ksks, bsks);
    if (overflow_out) summed_round(ss, overflow_out, rOvf, w, ksks, bsks);
    if (results) summed_round(ss, v, rRes, w, ksks, bsks);
  }

  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    shape.release(S0(ss));
    own.release(S0(ss));
  }
};

// ------------------------------------------------------------------ multiplication
// radix_parallel/mul.rs: block products (low / high halves through bivariate LUTs), column sums in
// groups that fit the carry space, final carry propagation.
struct MulMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x4D554C31;  // "MUL1"
  LutDriver drv;       // LUTs: 0 product low, 1 product high, 2 message, 3 carry
  PropagateMem prop;
  uint32_t blocks = 0, max_cts = 0, sub = 0;  // sub = integers per pass
  uint32_t slots = 0;                          // pool slots per integer
  uint64_t *d_pool = nullptr, *d_pack = nullptr, *d_sum = nullptr;

  using Step = SumStep;  // one reduction step, ciphertext-relative: groups of pool slots, the slots they become
  std::vector<uint64_t> prod_lhs, prod_rhs, prod_slot, prod_lut;  // products
  std::vector<Step> steps;
  std::vector<std::vector<uint64_t>> final_cols;  // what is left of every column: degrees adding up to 2 msg - 2 at most

  // The first terms of the column sums (radix_sum.h plans the rest): a low half of a block product is at most msg - 1, a
  // high half at most (msg - 1)^2 / msg (2 for msg = 4).  Every column ends at degrees adding up to 2 msg - 2 at most,
  // what one carry propagation accepts.  Many integers per call: 1,762 PBS per 32-block multiplication; few: 1,804 in
  // three rounds less.
  void plan() {
    const uint32_t L = blocks, m = drv.p.msg;
    std::vector<std::vector<uint64_t>> cols(L);
    std::vector<uint32_t> deg;  // by pool slot
    auto new_slot = [&](uint32_t d) {
      deg.push_back(d);
      return (uint64_t)deg.size() - 1;
    };
    for (uint32_t i = 0; i < L; ++i)
      for (uint32_t j = 0; i + j < L; ++j) {
        prod_lhs.push_back(j);
        prod_rhs.push_back(i);
        prod_lut.push_back(0);
        prod_slot.push_back(deg.size());
        cols[i + j].push_back(new_slot(m - 1));
        if (i + j + 1 < L) {
          prod_lhs.push_back(j);
          prod_rhs.push_back(i);
          prod_lut.push_back(1);
          prod_slot.push_back(deg.size());
          cols[i + j + 1].push_back(new_slot((m - 1) * (m - 1) / m));
        }
      }
    SumPlan plan = plan_column_sums(std::move(cols), deg, m, drv.p.carry, max_cts >= 8, 2 * m - 2);
    steps = std::move(plan.steps);
    final_cols = std::move(plan.final_cols);
    slots = (uint32_t)deg.size();
  }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t num_blocks, uint32_t cts) {
    blocks = num_blocks;
    max_cts = cts;
    const uint64_t m = p.msg;
    std::vector<std::function<uint64_t(uint64_t)>> fs = {
        [m](uint64_t x) -> uint64_t { return ((x / m) * (x % m)) % m; },
        [m](uint64_t x) -> uint64_t { return ((x / m) * (x % m)) / m; },
        [m](uint64_t x) -> uint64_t { return x % m; },
        [m](uint64_t x) -> uint64_t { return x / m; },
    };
    std::vector<std::vector<uint64_t>> luts;
    for (auto &f : fs) {
      luts.emplace_back((size_t)(p.k + 1) * p.N);
      generate_lut(p, luts.back().data(), f);
    }
    drv.p = p;
    plan();
    // integers per pass: the term pool of one pass may take 12 GiB of the 288 GB (32-block integers: 37 MB
    // each, ~340 per pass) — the later reduction rounds shrink fast, so passes should be as wide as possible
    const size_t w = p.big_n + 1;
    const size_t per_ct = (size_t)slots * w * sizeof(uint64_t);
    sub = (uint32_t)std::max<size_t>(1, std::min<size_t>(cts, ((size_t)12 << 30) / per_ct));
    drv.init(ss, p, 1u << 16, luts);
    own.alloc(d_pool, (size_t)sub * per_ct);
    const size_t n_prod = prod_slot.size();
    size_t max_groups = 0;
    for (auto &s : steps) max_groups = std::max(max_groups, s.msg_slot.size());
    own.alloc(d_pack, (size_t)sub * n_prod * w * sizeof(uint64_t));
    own.alloc(d_sum, std::max<size_t>(1, (size_t)sub * max_groups) * w * sizeof(uint64_t));
    prop.init(ss, p, num_blocks, sub);
    if (!t_dry) {
      build_pass(S0(ss), std::min(sub, cts));
      if (std::min(sub, cts) != sub) prop.build_indexes(S0(ss), std::min(sub, cts));
    }
  }

  // device index arrays of one pass over nb integers (built when the scratch is created, rebuilt if a call
  // brings another count): block products, every column-sum step, the final additions
  struct PassIdx {
    uint32_t nb = 0;
    uint64_t *pa = nullptr, *pb = nullptr, *po = nullptr, *pl = nullptr;
    struct StepIdx {
      uint64_t *off = nullptr, *mem = nullptr, *in = nullptr, *out = nullptr, *lut = nullptr;
      uint32_t groups = 0, count = 0;
    };
    std::vector<StepIdx> steps;
    uint64_t *foff = nullptr, *fmem = nullptr;
  } pass;
  DeviceBlocks own, shape;  // shape: the arrays of `pass`

  void build_pass(hipStream_t st, uint32_t nb) {
    shape.release(st);  // (waits: launches of the previous shape may still read them)
    pass = PassIdx();
    pass.nb = nb;
    const uint32_t L = blocks;
    const size_t n_prod = prod_slot.size();
    {  // block products
      std::vector<uint64_t> a(nb * n_prod), b(nb * n_prod), o(nb * n_prod), l(nb * n_prod);
      for (uint32_t c = 0; c < nb; ++c)
        for (size_t q = 0; q < n_prod; ++q) {
          a[c * n_prod + q] = (uint64_t)c * L + prod_lhs[q];
          b[c * n_prod + q] = (uint64_t)c * L + prod_rhs[q];
          o[c * n_prod + q] = (uint64_t)c * slots + prod_slot[q];
          l[c * n_prod + q] = prod_lut[q];
        }
      pass.pa = shape.upload(st, a), pass.pb = shape.upload(st, b);
      pass.po = shape.upload(st, o), pass.pl = shape.upload(st, l);
    }
    for (const Step &s : steps) {  // column sums
      PassIdx::StepIdx si;
      const size_t G = s.msg_slot.size();
      if (G != 0) {
        std::vector<uint64_t> off(nb * G + 1), mem(nb * s.members.size());
        std::vector<uint64_t> in, out, lut;
        for (uint32_t c = 0; c < nb; ++c) {
          for (size_t g = 0; g < G; ++g) {
            off[c * G + g] = c * s.members.size() + s.offsets[g];
            in.push_back(c * G + g);
            out.push_back((uint64_t)c * slots + s.msg_slot[g]);
            lut.push_back(2);
            if (s.carry_slot[g] != ~(uint64_t)0) {
              in.push_back(c * G + g);
              out.push_back((uint64_t)c * slots + s.carry_slot[g]);
              lut.push_back(3);
            }
          }
          for (size_t m = 0; m < s.members.size(); ++m) mem[c * s.members.size() + m] = (uint64_t)c * slots + s.members[m];
        }
        off[nb * G] = nb * s.members.size();
        si.off = shape.upload(st, off), si.mem = shape.upload(st, mem);
        si.in = shape.upload(st, in), si.out = shape.upload(st, out), si.lut = shape.upload(st, lut);
        si.groups = (uint32_t)(nb * G);
        si.count = (uint32_t)in.size();
      }
      pass.steps.push_back(si);
    }
    {  // what is left of every column (degrees adding up to 2 msg - 2 at most): CSR over the pool, in lhs order
      std::vector<uint64_t> off{0}, mem;
      for (uint32_t c = 0; c < nb; ++c)
        for (uint32_t col = 0; col < L; ++col) {
          for (uint64_t x : final_cols[col]) mem.push_back((uint64_t)c * slots + x);
          off.push_back(mem.size());
        }
      pass.foff = shape.upload(st, off), pass.fmem = shape.upload(st, mem);
    }
  }

  // lhs <- lhs * rhs for `cts` integers
  void run(const CudaStreamsFFI &ss, uint64_t *lhs, const uint64_t *rhs, uint32_t cts, void *const *ksks,
           void *const *bsks) {
    const hipStream_t st = S0(ss);
    HX_PANIC_IF_FALSE(cts >= 1 && cts <= max_cts, "multiplication: %u integers exceed the scratch capacity %u", cts,
                      max_cts);
    const Params &p = drv.p;
    const uint32_t L = blocks, w = p.big_n + 1;
    const size_t n_prod = prod_slot.size();
    for (uint32_t c0 = 0; c0 < cts; c0 += sub) {
      const uint32_t nb = std::min(sub, cts - c0);
      uint64_t *l0 = lhs + (size_t)c0 * L * w;
      const uint64_t *r0 = rhs + (size_t)c0 * L * w;
      if (pass.nb != nb) {
        HX_CHECK(hipStreamSynchronize(st));  // the previous pass may still read its arrays
        build_pass(st, nb);
      }
      // block products
      HX_RANGE("integer mul: %u integers of %u blocks", nb, L);
      {
        HX_RANGE("block products");
        axpy(st, d_pack, nullptr, l0, pass.pa, p.msg, r0, pass.pb, w, (uint32_t)(nb * n_prod));
        drv.round(ss, d_pool, pass.po, d_pack, nullptr, pass.pl, (uint32_t)(nb * n_prod), ksks, bsks);
      }
      for (const auto &si : pass.steps) {  // column sums
        if (si.groups == 0) continue;
        HX_RANGE("column sums (%u groups)", si.groups);
        HX_LAUNCH(lwe_group_sum_kernel, dim3(si.groups), dim3(256), 0, st, d_sum, d_pool, si.off, si.mem, w, si.groups);
        drv.round(ss, d_pool, si.out, d_sum, si.in, si.lut, si.count, ksks, bsks);
      }
      // the remaining terms of every column added into lhs, then one carry propagation
      HX_LAUNCH(lwe_group_sum_kernel, dim3(nb * L), dim3(256), 0, st, l0, d_pool, pass.foff, pass.fmem, w, nb * L);
      prop.run(ss, l0, nb, ksks, bsks);
    }
  }

  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    prop.release(ss);
    shape.release(S0(ss));
    own.release(S0(ss));
  }
};

// Multiplication by an encrypted boolean (integer.h:173-177 is_boolean_left / is_boolean_right; multiplication.h:28-49,
// cmux.cuh:13-46 zero_out_if): every block of the integer packed with the boolean's single block, one bivariate
// table (condition == 0 ? 0 : block): one KS -> PBS round of `blocks` bootstraps per integer.
struct BoolMulMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x424D554C;  // "BMUL"
  LutDriver drv;
  uint32_t blocks = 0, max_cts = 0;
  uint64_t *d_pack = nullptr, *d_cond_idx = nullptr, *d_lut_idx = nullptr;
  DeviceBlocks own;

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t num_blocks, uint32_t cts) {
    blocks = num_blocks;
    max_cts = cts;
    const uint64_t m = p.msg;
    std::vector<std::vector<uint64_t>> luts(1, std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    generate_lut(p, luts[0].data(), [m](uint64_t x) -> uint64_t { return (x % m) == 0 ? 0 : x / m; });
    const uint32_t T = cts * num_blocks;
    drv.init(ss, p, std::min<uint32_t>(T, 1u << 16), luts);
    own.alloc(d_pack, (size_t)T * (p.big_n + 1) * sizeof(uint64_t));
    if (!t_dry) {  // (so a size query leaves these two uploads out, unlike every other scratch)
      std::vector<uint64_t> ci(T), li(T, 0);
      for (uint32_t i = 0; i < T; ++i) ci[i] = i / num_blocks;  // the boolean of integer c is block c of its operand
      d_cond_idx = own.upload(S0(ss), ci);
      d_lut_idx = own.upload(S0(ss), li);
    }
  }
  // out <- condition ? value : 0; `cond` holds one block per integer
  void run(const CudaStreamsFFI &ss, uint64_t *out, const uint64_t *value, const uint64_t *cond, uint32_t cts,
           void *const *ksks, void *const *bsks) {
    HX_PANIC_IF_FALSE(cts >= 1 && cts <= max_cts, "boolean multiplication: %u integers exceed the scratch capacity %u",
                      cts, max_cts);
    const Params &p = drv.p;
    const uint32_t T = cts * blocks;
    axpy(S0(ss), d_pack, nullptr, value, nullptr, p.msg, cond, d_cond_idx, p.big_n + 1, T);
    drv.round(ss, out, nullptr, d_pack, nullptr, d_lut_idx, T, ksks, bsks);
  }
  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    own.release(S0(ss));
  }
};

// ------------------------------------------------------------------ bitwise operations, subtraction, full propagation
// bitwise_ops.h:101-178 (int_bitop_buffer): one bivariate table of (lhs, rhs) packed msg * lhs + rhs for the ciphertext
// forms, one univariate table per clear block value for the scalar forms (the clear blocks are the LUT indexes)
struct BitopMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x42495431;  // "BIT1"
  LutDriver drv;
  uint32_t op = 0;
  uint64_t *d_pack = nullptr, *d_lut_idx = nullptr;  // packed operands; all-zero LUT indexes (ciphertext forms)
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    drv.release(s);
    own.release(S0(s));
  }
};
static uint64_t bitop_apply(uint32_t op, uint64_t a, uint64_t b) {
  switch (op % 3) {
    case 0: return a & b;
    case 1: return a | b;
    default: return a ^ b;
  }
}
// bitwise_ops.cu:133-185 (update_degrees_after_*): the largest value the operation can return on operands up to (a, b)
static uint64_t bitop_degree(uint32_t op, uint64_t a, uint64_t b) {
  const uint64_t hi = std::max(a, b), lo = std::min(a, b);
  if (op % 3 == 0) return lo;
  uint64_t r = hi;
  for (uint64_t j = 0; j <= lo; ++j) r = std::max(r, op % 3 == 1 ? (hi | j) : (hi ^ j));
  return r;
}

// subtraction.cuh:31-47: the negation of rhs with its correcting term, then the addition's carry propagation
struct SubMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x53554231;  // "SUB1"
  PropagateMem prop;
  uint64_t *d_neg = nullptr;
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    prop.release(s);
    own.release(S0(s));
  }
};

// integer.cuh:1924-1983 (host_full_propagate_inplace): block after block, message and carry of the block by one
// two-input bootstrap round, the carry added to the next block
struct FullPropMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x46505031;  // "FPP1"
  LutDriver drv;  // LUTs: 0 message, 1 carry
  uint64_t *d_two = nullptr, *d_lut_idx = nullptr;  // the block twice -> (message, carry); indexes {0, 1}
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    drv.release(s);
    own.release(S0(s));
  }
};

// comparison.cuh / integer.h:246-276, unsigned operands.  Orderings ride on the subtraction's carry tree:
//   a >= b  <=>  a + (2^bits - b) carries out of the last block
// so GE is the output carry of the subtraction WITHOUT its result round (65 of the 97 bootstraps of a 32-block
// subtraction, 5 rounds), LE swaps the operands, LT / GT are 1 - that (levelled).  The reference reduces block orderings
// pairwise (63 bootstraps in 6 rounds for 32 blocks: comparison.cuh).  Equality: one bivariate round, then sums of up to
// (msg * carry - 1) / (msg - 1) = 5 block results against their count, level by level (32 + 7 + 2 + 1 bootstraps in 4 rounds).
struct CompareMem {  // only ever a member of CompareScratch: no header
  uint32_t op = 0, blocks = 0;
  PropagateMem prop;  // orderings
  LutDriver eq;       // equality: LUT 0 a == b, 1 a != b (packed pairs); 2 + (c - 1): sum == c; 2 + G + (c - 1): sum != c
  uint32_t G = 0;     // largest group: (msg * carry - 1) / (msg - 1)
  uint64_t *d_tmp = nullptr, *d_neg = nullptr, *d_bool = nullptr;  // orderings: lhs copy, negated rhs, the flag
  uint64_t *d_pack = nullptr, *d_pool = nullptr, *d_sum = nullptr, *d_lut0 = nullptr;
  struct Level {
    uint32_t groups = 0, in_off = 0, out_off = 0;
    uint64_t *off = nullptr, *mem = nullptr, *lut = nullptr;
  };
  std::vector<Level> levels;
  DeviceBlocks own;
  uint32_t last_slot = 0;

  bool ordering() const { return op >= GT && op <= LE; }
  const Params &params() const { return ordering() ? prop.drv.p : eq.p; }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t L, uint32_t operation) {
    op = operation;
    blocks = L;
    const size_t w = (size_t)p.big_n + 1, lw = (size_t)(p.k + 1) * p.N;
    if (ordering()) {
      prop.init(ss, p, L, 1);
      own.alloc(d_tmp, L * w * sizeof(uint64_t));
      own.alloc(d_neg, L * w * sizeof(uint64_t));
      own.alloc(d_bool, w * sizeof(uint64_t));
      return;
    }
    // comparison.cuh are_all_comparisons_block_true: chunks of (msg * carry - 1) / (msg - 1) block results — 5 at 2_2, which is also
    // what tfhe-rs's noise-level bookkeeping allows for a sum of fresh bootstrap outputs (levels add, MaxNoiseLevel 5).  A sum of
    // 15 fits the plaintext space, but no caller of the reference ever bootstraps one
    G = (p.msg * p.carry - 1) / (p.msg - 1);
    const uint32_t msg = p.msg;
    std::vector<std::vector<uint64_t>> luts(2 + 2 * G, std::vector<uint64_t>(lw));
    generate_lut(p, luts[0].data(), [msg](uint64_t x) -> uint64_t { return x / msg == x % msg; });
    generate_lut(p, luts[1].data(), [msg](uint64_t x) -> uint64_t { return x / msg != x % msg; });
    for (uint32_t c = 1; c <= G; ++c) {
      generate_lut(p, luts[2 + c - 1].data(), [c](uint64_t x) -> uint64_t { return x == c; });
      generate_lut(p, luts[2 + G + c - 1].data(), [c](uint64_t x) -> uint64_t { return x != c; });
    }
    eq.init(ss, p, L, luts);
    own.alloc(d_pack, L * w * sizeof(uint64_t));
    // pool: the block results, then every level's results
    uint32_t slots = L, n = L;
    std::vector<uint32_t> sizes;
    while (n > 1) {
      n = (n + G - 1) / G;
      sizes.push_back(n);
      slots += n;
    }
    own.alloc(d_pool, (size_t)slots * w * sizeof(uint64_t));
    own.alloc(d_sum, (size_t)std::max<uint32_t>(1, sizes.empty() ? 1 : sizes[0]) * w * sizeof(uint64_t));
    const bool ne = op == NE;
    d_lut0 = own.upload(S0(ss), std::vector<uint64_t>(L, (L == 1 && ne) ? 1 : 0));
    uint32_t in_off = 0, in_n = L, out_off = L;
    for (size_t l = 0; l < sizes.size(); ++l) {
      Level lv;
      lv.groups = sizes[l];
      lv.in_off = in_off;
      lv.out_off = out_off;
      std::vector<uint64_t> off(lv.groups + 1), mem(in_n), lut(lv.groups);
      for (uint32_t g = 0; g <= lv.groups; ++g) off[g] = std::min<uint64_t>((uint64_t)g * G, in_n);
      for (uint32_t i = 0; i < in_n; ++i) mem[i] = in_off + i;
      const bool last = l + 1 == sizes.size();
      for (uint32_t g = 0; g < lv.groups; ++g) {
        const uint32_t c = (uint32_t)(off[g + 1] - off[g]);
        lut[g] = (last && ne) ? 2 + G + c - 1 : 2 + c - 1;
      }
      lv.off = own.upload(S0(ss), off);
      lv.mem = own.upload(S0(ss), mem);
      lv.lut = own.upload(S0(ss), lut);
      levels.push_back(lv);
      in_off = out_off;
      in_n = lv.groups;
      out_off += lv.groups;
    }
    last_slot = in_off;  // slot of the single result (0 when L == 1)
  }

  // flag (one block) <- op(a, b); a and b: `blocks` clean blocks each
  void run(const CudaStreamsFFI &ss, uint64_t *flag, const uint64_t *a, const uint64_t *b, void *const *ksks,
           void *const *bsks) {
    const hipStream_t st = S0(ss);
    const uint32_t L = blocks;
    if (ordering()) {
      const Params &p = prop.drv.p;
      const uint32_t w = p.big_n + 1;
      const uint64_t delta = p.delta();
      const bool swap = op == LE || op == GT;       // LE(a, b) = GE(b, a); GT(a, b) = LT(b, a)
      const bool invert = op == LT || op == GT;     // LT = 1 - GE
      const uint64_t *x = swap ? b : a, *y = swap ? a : b;
      HX_CHECK(hipMemcpyAsync(d_tmp, x, (size_t)L * w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      HX_LAUNCH(lwe_negate_const_kernel, dim3(L), dim3(256), 0, st, d_neg, y, w, L, L, (uint64_t)p.msg * delta,
                (uint64_t)(p.msg - 1) * delta);
      axpy(st, d_tmp, nullptr, d_tmp, nullptr, 1, d_neg, nullptr, w, L);
      prop.run(ss, d_tmp, 1, ksks, bsks, nullptr, invert ? d_bool : flag, nullptr, false);
      if (invert) HX_LAUNCH(lwe_negate_const_kernel, dim3(1), dim3(256), 0, st, flag, d_bool, w, 1, 1, delta, delta);
      return;
    }
    const Params &p = eq.p;
    const uint32_t w = p.big_n + 1;
    axpy(st, d_pack, nullptr, a, nullptr, p.msg, b, nullptr, w, L);
    eq.round(ss, d_pool, nullptr, d_pack, nullptr, d_lut0, L, ksks, bsks);
    for (const Level &lv : levels) {
      HX_LAUNCH(lwe_group_sum_kernel, dim3(lv.groups), dim3(256), 0, st, d_sum, d_pool, lv.off, lv.mem, w, lv.groups);
      eq.round(ss, d_pool + (size_t)lv.out_off * w, nullptr, d_sum, nullptr, lv.lut, lv.groups, ksks, bsks);
    }
    HX_CHECK(hipMemcpyAsync(flag, d_pool + (size_t)last_slot * w, (size_t)w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  }

  void release(const CudaStreamsFFI &ss) {
    prop.release(ss);  // (orderings; the other of the two was never set up and holds nothing)
    eq.release(ss);
    own.release(S0(ss));
  }
};

// cmux.cuh / integer.h:349-365: out <- condition ? true : false.  Both branches packed with the condition's single block
// (block + msg * condition), one round over the 2 L packed blocks keeps a branch's block or zeroes it, the halves are added
// and a message-extraction round returns the sum to nominal noise (the reference's int_cmux_buffer does the same three steps)
struct CmuxMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x434D5831;  // "CMX1"
  LutDriver drv;  // LUTs: 0 keep if the condition is 1, 1 keep if it is 0, 2 message
  uint32_t blocks = 0;
  uint64_t *d_pack = nullptr, *d_zero_idx = nullptr, *d_lut_idx = nullptr, *d_lut2 = nullptr;
  DeviceBlocks own;

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t L) {
    blocks = L;
    const uint64_t m = p.msg;
    std::vector<std::vector<uint64_t>> luts(3, std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    generate_lut(p, luts[0].data(), [m](uint64_t x) -> uint64_t { return x >= m && x < 2 * m ? x - m : 0; });
    generate_lut(p, luts[1].data(), [m](uint64_t x) -> uint64_t { return x < m ? x : 0; });
    generate_lut(p, luts[2].data(), [m](uint64_t x) -> uint64_t { return x % m; });
    drv.init(ss, p, 2 * L, luts);
    own.alloc(d_pack, (size_t)2 * L * (p.big_n + 1) * sizeof(uint64_t));
    std::vector<uint64_t> li(2 * L, 0);
    for (uint32_t i = L; i < 2 * L; ++i) li[i] = 1;
    d_zero_idx = own.upload(S0(ss), std::vector<uint64_t>(L, 0));
    d_lut_idx = own.upload(S0(ss), li);
    d_lut2 = own.upload(S0(ss), std::vector<uint64_t>(L, 2));
  }
  void run(const CudaStreamsFFI &ss, uint64_t *out, const uint64_t *cond, const uint64_t *t, const uint64_t *f,
           void *const *ksks, void *const *bsks) {
    const Params &p = drv.p;
    const hipStream_t st = S0(ss);
    const uint32_t L = blocks, w = p.big_n + 1;
    axpy(st, d_pack, nullptr, cond, d_zero_idx, p.msg, t, nullptr, w, L);
    axpy(st, d_pack + (size_t)L * w, nullptr, cond, d_zero_idx, p.msg, f, nullptr, w, L);
    drv.round(ss, d_pack, nullptr, d_pack, nullptr, d_lut_idx, 2 * L, ksks, bsks);
    axpy(st, out, nullptr, d_pack, nullptr, 1, d_pack + (size_t)L * w, nullptr, w, L);
    drv.round(ss, out, nullptr, out, nullptr, d_lut2, L, ksks, bsks);
  }
  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    own.release(S0(ss));
  }
};

// the shift by r bits inside a block, on the packing msg * current + neighbour (lower neighbour for a left shift, upper
// for a right one): the table of the logical scalar shift and of the scalar multiplication's shifted copies
static std::function<uint64_t(uint64_t)> shift_in_block(uint32_t msg, uint32_t bits, uint32_t r, bool left) {
  return [msg, bits, r, left](uint64_t x) -> uint64_t {
    const uint64_t cur = x / msg, nb = x % msg;
    return (left ? ((cur << r) | (nb >> (bits - r))) : ((cur >> r) | (nb << (bits - r)))) % msg;
  };
}

// scalar_shifts.cuh / integer.h:200-228: logical shift of an unsigned integer by a clear amount = a move by whole blocks
// and, when bits remain, ONE bivariate round over (block, its lower / upper neighbour)
struct ScalarShiftMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x53484631;  // "SHF1"
  LutDriver drv;  // LUT r - 1: the shift by r bits inside a block (r = 1 .. bits per block - 1), this scratch's direction
  uint32_t blocks = 0, bits = 0, left = 0;
  uint64_t *d_pack = nullptr, *d_lut_idx = nullptr;  // packed pairs / block copy; one constant index array per r
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    drv.release(s);
    own.release(S0(s));
  }
};

static uint32_t batch_of(const CudaRadixCiphertextFFI *ct, uint32_t blocks, const char *what) {
  HX_PANIC_IF_FALSE(ct != nullptr && ct->ptr != nullptr, "%s: null radix ciphertext", what);
  HX_PANIC_IF_FALSE(blocks != 0 && ct->num_radix_blocks % blocks == 0,
                    "%s: %u blocks is not a whole number of %u-block integers", what, ct->num_radix_blocks, blocks);
  return ct->num_radix_blocks / blocks;
}

// ------------------------------------------------------------------ bookkeeping the entry points share
// degree and noise level of blocks [first, first + count) after a launch; a caller that tracks neither passes no arrays
static void set_block_info(CudaRadixCiphertextFFI *ct, uint32_t first, uint32_t count, uint64_t degree, uint64_t noise) {
  for (uint32_t i = first; i < first + count; ++i) {
    if (ct->degrees) ct->degrees[i] = degree;
    if (ct->noise_levels) ct->noise_levels[i] = noise;
  }
}
// an optional carry operand that a flag of the call makes mandatory: one block per integer, same LWE dimension
static uint64_t *carry_blocks(const CudaRadixCiphertextFFI *carry, uint32_t cts, const CudaRadixCiphertextFFI *like,
                              const char *complaint) {
  HX_PANIC_IF_FALSE(carry && carry->ptr && carry->num_radix_blocks >= cts && carry->lwe_dimension == like->lwe_dimension,
                    "%s", complaint);
  return (uint64_t *)carry->ptr;
}
// the operations that pack two blocks into one take clean operands: the first n blocks have degree <= msg - 1
static void check_clean(std::initializer_list<const CudaRadixCiphertextFFI *> operands, uint32_t n, uint32_t msg,
                        const char *who, const char *tail) {
  for (const CudaRadixCiphertextFFI *op : operands)
    if (op->degrees)
      for (uint32_t i = 0; i < n; ++i)
        HX_PANIC_IF_FALSE(op->degrees[i] <= msg - 1, "%s: block %u has degree %llu, %s", who, i,
                          (unsigned long long)op->degrees[i], tail);
}

// ------------------------------------------------------------------ shifts and rotations
// shift_and_rotate.cuh / integer.h:230-244: shift or rotation by an ENCRYPTED amount, a barrel shifter over the bits.
// b = log2(msg) bits per block, L blocks, B = b L bits, m = ceil(log2 B) control bits.  Rounds of one call, every
// integer of the batch in the same rounds:
//   1. value bits: B rows per integer, bit i of block j -> {0, 1} (the driver's input index reads block j b times)
//   2. control bits: the m low bits of the amount, each already at plaintext position 2 (value 4 bit)
//   3. m stages: ONE lwe_rotate_pack_kernel launch forms ctrl_d + 2 src(i, 2^d) + cur(i) for every bit row — src wraps
//      (rotations), is nothing (shifts) or the sign row as step 1 extracted it (arithmetic right shift) — and one round
//      of B rows applies the mux table (x & 7 = 4 c + 2 p + a -> c ? p : a)
//   4. shifts only: "amount >= B" from the unsigned comparison against the clear digits of B (one pass per integer), for
//      the arithmetic shift 2 overshift + sign; one round of one row per integer moves it into the carry
//   5. reassembly: from each block's top bit, b - 1 times block = 2 block + next lower bit and a cleaning round; the last
//      one takes the packed condition on top and the overshift table instead.  b = 1: no loop, the cleanup (shifts only)
//      is a round of its own.
// A rotation rotates by (amount mod 2^m) mod B: when B is no power of two the m control bits capture amounts up to
// 2^m - 1 >= B and the barrel stages compose to a rotation by that many positions, which is what the reference's GPU code
// computes.
// Bootstraps per integer: B + m + m B + (shifts: comparison + 1) + (b > 1 ? (b - 1) L : shifts ? L : 0).
// Differences from the reference: at msg = 2 the amount's bit blocks are paired into base-4 digits before the comparison
// (the carry look-ahead behind GE takes digits of two bits and more; the reference pairs blocks inside its comparison), and
// the table that moves the condition into the carry keeps two bits, (x & 3) msg — at msg = 2 the reference's (x % msg) msg
// drops the overshift bit of an arithmetic shift; from msg = 4 on the two tables are the same.
struct ShiftRotateMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x53525431;  // "SRT1"
  LutDriver drv;  // LUTs: i: bit i; b + i: bit i at position 2; 2 b: mux; + 1: x % msg; + 2: condition into the carry; + 3: cleanup
  CompareMem cmp;
  uint32_t blocks = 0, bits = 0, total = 0, ctrl = 0, max_cts = 0, type = 0;
  bool arithmetic = false, overshift = false, pairs = false;
  uint32_t cmp_blocks = 0;  // digits the comparison sees (paired at msg = 2, padded to an even count)
  uint64_t *d_bits = nullptr, *d_cur = nullptr, *d_pack = nullptr, *d_ctrl = nullptr, *d_cond = nullptr,
           *d_padded = nullptr, *d_triv = nullptr;
  // index arrays, [integer][row] so that a call with fewer integers reads a prefix
  uint64_t *i_bits_in = nullptr, *i_bits_lut = nullptr, *i_ctrl_in = nullptr, *i_ctrl_lut = nullptr, *i_const = nullptr,
           *i_sign = nullptr, *i_top = nullptr, *i_bit = nullptr, *i_cond = nullptr, *i_hi = nullptr, *i_lo = nullptr;
  DeviceBlocks own;

  bool shift() const { return type == LEFT_SHIFT || type == RIGHT_SHIFT; }
  uint64_t compare_pbs() const {
    if (!overshift) return 0;
    return cmp_blocks == 1 ? 1 : PropagateMem::pbs_count(cmp_blocks) - cmp_blocks + 1;  // no result round, the flag
  }
  uint64_t pbs_count() const {
    return (uint64_t)total + ctrl + (uint64_t)ctrl * total + (overshift ? compare_pbs() + 1 : 0) +
           (bits > 1 ? (uint64_t)(bits - 1) * blocks : overshift ? blocks : 0);
  }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t L, uint32_t cts, uint32_t shift_type, bool is_signed) {
    HX_PANIC_IF_FALSE(L >= 1 && cts >= 1, "shift_and_rotate: no blocks");
    HX_PANIC_IF_FALSE(shift_type <= RIGHT_ROTATE, "shift_and_rotate: unknown shift type %u", shift_type);
    HX_PANIC_IF_FALSE((p.msg & (p.msg - 1)) == 0, "shift_and_rotate: the message modulus must be a power of two");
    // the mux packs control | previous | current into one block: three bits
    HX_PANIC_IF_FALSE(p.msg * p.carry >= 8, "shift_and_rotate: message_modulus * carry_modulus >= 8 is required (got %u)",
                      p.msg * p.carry);
    blocks = L, max_cts = cts, type = shift_type;
    bits = (uint32_t)__builtin_ctz(p.msg);
    total = bits * L;
    ctrl = 0;
    while ((1u << ctrl) < total) ++ctrl;
    overshift = shift();
    arithmetic = is_signed && shift_type == RIGHT_SHIFT;
    const uint32_t b = bits, B = total, m = ctrl;
    const uint64_t msg = p.msg;
    const size_t lw = (size_t)(p.k + 1) * p.N, w = (size_t)p.big_n + 1;
    std::vector<std::vector<uint64_t>> luts(2 * b + 4, std::vector<uint64_t>(lw));
    for (uint32_t i = 0; i < b; ++i) {
      generate_lut(p, luts[i].data(), [i](uint64_t x) -> uint64_t { return (x >> i) & 1; });
      generate_lut(p, luts[b + i].data(), [i](uint64_t x) -> uint64_t { return ((x >> i) & 1) << 2; });
    }
    generate_lut(p, luts[2 * b].data(), [](uint64_t x) -> uint64_t { return (x & 4) ? (x >> 1) & 1 : x & 1; });
    generate_lut(p, luts[2 * b + 1].data(), [msg](uint64_t x) -> uint64_t { return x % msg; });
    generate_lut(p, luts[2 * b + 2].data(), [msg](uint64_t x) -> uint64_t { return (x & 3) * msg; });
    const bool arith = arithmetic;
    generate_lut(p, luts[2 * b + 3].data(), [msg, arith](uint64_t x) -> uint64_t {
      const uint64_t c = x / msg, v = x % msg;
      if (arith) return c == 3 ? msg - 1 : c == 2 ? 0 : v;
      return c >= 1 ? 0 : v;
    });
    const uint32_t rows = cts * std::max(B, L);
    drv.init(ss, p, std::min<uint32_t>(rows, 1u << 16), luts);
    own.alloc(d_bits, (size_t)cts * B * w * sizeof(uint64_t));
    own.alloc(d_cur, (size_t)cts * B * w * sizeof(uint64_t));
    own.alloc(d_pack, (size_t)cts * B * w * sizeof(uint64_t));
    own.alloc(d_ctrl, (size_t)cts * std::max(1u, m) * w * sizeof(uint64_t));
    const hipStream_t st = S0(ss);
    std::vector<uint64_t> bi((size_t)cts * B), bl((size_t)cts * B), ci((size_t)cts * m), cl((size_t)cts * m),
        top((size_t)cts * L), bit((size_t)std::max(1u, b - 1) * cts * L), cond((size_t)cts * L), sign(cts);
    for (uint32_t c = 0; c < cts; ++c) {
      for (uint32_t j = 0; j < L; ++j) {
        for (uint32_t i = 0; i < b; ++i) bi[(size_t)c * B + j * b + i] = (uint64_t)c * L + j, bl[(size_t)c * B + j * b + i] = i;
        top[(size_t)c * L + j] = (uint64_t)c * B + j * b + b - 1;
        for (uint32_t i = 0; i + 1 < b; ++i) bit[((size_t)i * cts + c) * L + j] = (uint64_t)c * B + j * b + i;
        cond[(size_t)c * L + j] = c;
      }
      for (uint32_t d = 0; d < m; ++d) ci[(size_t)c * m + d] = (uint64_t)c * L + d / b, cl[(size_t)c * m + d] = b + d % b;
      sign[c] = (uint64_t)c * B + B - 1;
    }
    i_bits_in = own.upload(st, bi), i_bits_lut = own.upload(st, bl);
    i_ctrl_in = own.upload(st, ci), i_ctrl_lut = own.upload(st, cl);
    i_top = own.upload(st, top), i_bit = own.upload(st, bit), i_cond = own.upload(st, cond), i_sign = own.upload(st, sign);
    // constant LUT indexes: [2 b] * rows (mux), then + 1, + 2, + 3 on cts L rows each
    std::vector<uint64_t> k((size_t)cts * B + 3 * (size_t)cts * L);
    for (size_t i = 0; i < k.size(); ++i) k[i] = i < (size_t)cts * B ? 2 * b : 2 * b + 1 + (i - (size_t)cts * B) / ((size_t)cts * L);
    i_const = own.upload(st, k);
    if (!overshift) return;
    // "amount >= B" on the clear digits of B
    pairs = p.msg == 2;
    const uint32_t digits = pairs ? (L + 1) / 2 : L;
    cmp_blocks = (digits > 1 && digits % 2) ? digits + 1 : digits;
    Params pc = p;
    if (pairs) pc.msg = 4, pc.carry = p.msg * p.carry / 4;  // the same plaintext space, read as digits of two bits
    cmp.init(ss, pc, cmp_blocks, GE);
    own.alloc(d_cond, (size_t)cts * w * sizeof(uint64_t));
    if (pairs || cmp_blocks != L) own.alloc(d_padded, (size_t)cmp_blocks * w * sizeof(uint64_t));
    std::vector<uint64_t> triv((size_t)cmp_blocks * w, 0);
    uint64_t v = B;
    for (uint32_t i = 0; i < cmp_blocks; ++i, v /= pc.msg) triv[(size_t)i * w + w - 1] = (v % pc.msg) * p.delta();
    HX_PANIC_IF_FALSE(v == 0, "shift_and_rotate: the bit count %u does not fit %u digits", B, cmp_blocks);
    d_triv = own.upload(st, triv);
    if (pairs) {
      std::vector<uint64_t> hi(L / 2), lo(L / 2);
      for (uint32_t i = 0; i < L / 2; ++i) hi[i] = 2 * i + 1, lo[i] = 2 * i;
      i_hi = own.upload(st, hi), i_lo = own.upload(st, lo);
    }
  }

  void run(const CudaStreamsFFI &ss, uint64_t *v, const uint64_t *amount, uint32_t cts, void *const *ksks,
           void *const *bsks) {
    const Params &p = drv.p;
    const hipStream_t st = S0(ss);
    const uint32_t L = blocks, b = bits, B = total, m = ctrl, w = p.big_n + 1;
    const uint64_t before = drv.issued + (overshift ? cmp.prop.drv.issued : 0);
    HX_RANGE("shift / rotate by an encrypted amount: %u integers of %u bits", cts, B);
    drv.round(ss, d_bits, nullptr, v, i_bits_in, i_bits_lut, cts * B, ksks, bsks);
    if (m) drv.round(ss, d_ctrl, nullptr, amount, i_ctrl_in, i_ctrl_lut, cts * m, ksks, bsks);
    const uint64_t *cur = d_bits;
    for (uint32_t d = 0; d < m; ++d) {
      RotatePack a{};
      a.out = d_pack, a.x = cur, a.pad = d_bits, a.ctrl = d_ctrl;
      a.s0 = 1, a.s1 = 2, a.words = w, a.rows = B, a.r = 1u << d;
      a.dir = (type == LEFT_SHIFT || type == LEFT_ROTATE) ? kTowardsHigher : kTowardsLower;
      a.mode = !shift() ? kPickWrap : arithmetic ? kPickRow : kPickZero;
      a.pad_stride = B, a.pad_row = B - 1, a.ctrl_stride = m, a.ctrl_row = d;
      launch_rotate_pack(st, a, cts);
      drv.round(ss, d_cur, nullptr, d_pack, nullptr, i_const, cts * B, ksks, bsks);
      cur = d_cur;
    }
    if (overshift) {
      for (uint32_t c = 0; c < cts; ++c) {
        const uint64_t *am = amount + (size_t)c * L * w;
        if (d_padded) {
          HX_CHECK(hipMemsetAsync(d_padded, 0, (size_t)cmp_blocks * w * sizeof(uint64_t), st));
          if (pairs) {
            axpy(st, d_padded, nullptr, am, i_hi, 2, am, i_lo, w, L / 2);
            if (L % 2)
              HX_CHECK(hipMemcpyAsync(d_padded + (size_t)(L / 2) * w, am + (size_t)(L - 1) * w, w * sizeof(uint64_t),
                                      hipMemcpyDeviceToDevice, st));
          } else {
            HX_CHECK(hipMemcpyAsync(d_padded, am, (size_t)L * w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
          }
          am = d_padded;
        }
        cmp.run(ss, d_cond + (size_t)c * w, am, d_triv, ksks, bsks);
      }
      if (arithmetic) axpy(st, d_cond, nullptr, d_cond, nullptr, 2, d_bits, i_sign, w, cts);
      drv.round(ss, d_cond, nullptr, d_cond, nullptr, i_const + (size_t)max_cts * B + 1 * (size_t)max_cts * L, cts, ksks, bsks);
    }
    const uint64_t *clean = i_const + (size_t)max_cts * B, *cleanup = clean + 2 * (size_t)max_cts * L;
    if (b == 1) {
      HX_CHECK(hipMemcpyAsync(v, cur, (size_t)cts * L * w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      if (overshift) {
        axpy(st, v, nullptr, v, nullptr, 1, d_cond, i_cond, w, cts * L);
        drv.round(ss, v, nullptr, v, nullptr, cleanup, cts * L, ksks, bsks);
      }
    }
    for (uint32_t i = b - 1; i-- > 0;) {
      const uint64_t *low = i_bit + (size_t)i * max_cts * L;
      if (i == b - 2) axpy(st, v, nullptr, cur, i_top, 2, cur, low, w, cts * L);
      else axpy(st, v, nullptr, v, nullptr, 2, cur, low, w, cts * L);
      const bool last = i == 0 && overshift;
      if (last) axpy(st, v, nullptr, v, nullptr, 1, d_cond, i_cond, w, cts * L);
      drv.round(ss, v, nullptr, v, nullptr, last ? cleanup : clean, cts * L, ksks, bsks);
    }
    const uint64_t after = drv.issued + (overshift ? cmp.prop.drv.issued : 0);
    HX_PANIC_IF_FALSE(after - before == cts * pbs_count(), "shift_and_rotate: %llu bootstraps issued, %llu counted",
                      (unsigned long long)(after - before), (unsigned long long)(cts * pbs_count()));
  }

  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    cmp.release(ss);
    own.release(S0(ss));
  }
};

// scalar_shifts.cuh / integer.h:212-228: arithmetic right shift of a two's complement integer by a clear amount.  A move
// by q = shift / b whole blocks, then ONE round whose rows carry their own table (the reference runs them on three
// streams): the n - 1 surviving (block, upper neighbour) pairs the in-block shift, the last surviving block the shift
// with sign fill, one more row the padding block (msg - 1) sign, which is then written to the q vacated top blocks.
// shift >= B: every block is the padding block.  b = 1: no bootstrap, the sign block is copied.
struct ArithShiftMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x41534831;  // "ASH1"
  LutDriver drv;  // LUTs: r - 1: in-block shift by r; (b - 1) + r - 1: the same with sign fill (univariate); 2 (b - 1): padding
  uint32_t blocks = 0, bits = 0, max_cts = 0;
  uint64_t *d_pack = nullptr;  // [integer][L + 1]: the rows of the round, row L the padding row's input
  uint64_t *i_in = nullptr, *i_out = nullptr, *i_lut = nullptr, *i_from = nullptr, *i_to = nullptr;  // of the cached call
  uint32_t key_shift = ~0u, key_cts = 0, round_rows = 0, fill_rows = 0;
  DeviceBlocks own, shape;  // shape: the index arrays of the cached call

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t L, uint32_t cts) {
    HX_PANIC_IF_FALSE(L >= 1 && cts >= 1, "arithmetic_scalar_shift: no blocks");
    HX_PANIC_IF_FALSE((p.msg & (p.msg - 1)) == 0, "arithmetic_scalar_shift: the message modulus must be a power of two");
    blocks = L, max_cts = cts;
    bits = (uint32_t)__builtin_ctz(p.msg);
    const uint32_t msg = p.msg, b = bits;
    std::vector<std::vector<uint64_t>> luts(2 * (b - 1) + 1, std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    for (uint32_t r = 1; r < b; ++r) {
      generate_lut(p, luts[r - 1].data(), shift_in_block(msg, b, r, false));
      generate_lut(p, luts[b - 1 + r - 1].data(), [msg, b, r](uint64_t x) -> uint64_t {
        const uint64_t v = x % msg, sign = v >> (b - 1);
        return ((v >> r) | (sign ? (uint64_t)(msg - 1) << (b - r) : 0)) % msg;
      });
    }
    generate_lut(p, luts[2 * (b - 1)].data(), [msg, b](uint64_t x) -> uint64_t { return (msg - 1) * ((x % msg) >> (b - 1)); });
    drv.init(ss, p, cts * (L + 1), luts);
    own.alloc(d_pack, (size_t)cts * (L + 1) * (p.big_n + 1) * sizeof(uint64_t));
  }

  // the rows of the call's round and of the fill that follows it; n blocks survive, r bits remain
  void plan(hipStream_t st, uint32_t shift, uint32_t cts, uint32_t n, uint32_t r) {
    if (key_shift == shift && key_cts == cts) return;
    const uint32_t L = blocks, b = bits;
    std::vector<uint64_t> in, out, lut, from, to;
    for (uint32_t c = 0; c < cts; ++c) {
      if (b > 1) {
        for (uint32_t j = 0; j < n && r; ++j) {
          in.push_back((uint64_t)c * (L + 1) + j), out.push_back((uint64_t)c * L + j);
          lut.push_back(j + 1 < n ? r - 1 : b - 1 + r - 1);
        }
        if (n < L) in.push_back((uint64_t)c * (L + 1) + L), out.push_back((uint64_t)c * L + n), lut.push_back(2 * (b - 1));
        for (uint32_t t = n + 1; t < L; ++t) from.push_back((uint64_t)c * L + n), to.push_back((uint64_t)c * L + t);
      } else {  // one bit per block: block t takes block t + q, the sign block beyond the end (rows of d_pack)
        for (uint32_t t = 0; t < L; ++t)
          from.push_back((uint64_t)c * (L + 1) + std::min(t + (L - n), L - 1)), to.push_back((uint64_t)c * L + t);
      }
    }
    shape.release(st);  // (waits: an earlier call may still read them)
    i_in = shape.upload(st, in), i_out = shape.upload(st, out), i_lut = shape.upload(st, lut);
    i_from = shape.upload(st, from), i_to = shape.upload(st, to);
    round_rows = (uint32_t)in.size(), fill_rows = (uint32_t)from.size();
    key_shift = shift, key_cts = cts;
  }

  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    shape.release(S0(ss));
    own.release(S0(ss));
  }
};

// scalar_rotate.cuh / integer.h:367-381: rotation by a clear amount.  n mod B first; a rotation by q = n / b whole blocks,
// which wraps, and when r = n mod b bits remain ONE bivariate round over all L blocks with the wrapping neighbour (the
// tables of the logical shift).  lwe_rotate_pack_kernel builds msg block + neighbour in wrap mode from the blocks where
// they are, and the round's output index performs the block rotation: no temporary rotation, no second copy.
struct ScalarRotateMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x53524F31;  // "SRO1"
  LutDriver drv;  // LUT r - 1: the shift by r bits inside a block, this scratch's direction
  uint32_t blocks = 0, bits = 0, left = 0, max_cts = 0;
  uint64_t *d_pack = nullptr, *i_lut = nullptr, *i_out = nullptr;  // i_lut: [r - 1][integer][block]; i_out: [q][integer][block]
  DeviceBlocks own;

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t L, uint32_t cts, bool is_left) {
    HX_PANIC_IF_FALSE(L >= 1 && cts >= 1, "scalar_rotate: no blocks");
    HX_PANIC_IF_FALSE((p.msg & (p.msg - 1)) == 0, "scalar_rotate: the message modulus must be a power of two");
    blocks = L, max_cts = cts, left = is_left;
    bits = (uint32_t)__builtin_ctz(p.msg);
    const uint32_t b = bits;
    std::vector<std::vector<uint64_t>> luts(std::max(1u, b - 1), std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    for (uint32_t r = 1; r < b; ++r) generate_lut(p, luts[r - 1].data(), shift_in_block(p.msg, b, r, is_left));
    drv.init(ss, p, cts * L, luts);
    own.alloc(d_pack, (size_t)cts * L * (p.big_n + 1) * sizeof(uint64_t));
    if (b == 1) return;
    const size_t T = (size_t)cts * L;
    std::vector<uint64_t> li((size_t)(b - 1) * T), oi((size_t)L * T);
    for (size_t i = 0; i < li.size(); ++i) li[i] = i / T;
    for (uint32_t q = 0; q < L; ++q)
      for (uint32_t c = 0; c < cts; ++c)
        for (uint32_t i = 0; i < L; ++i)  // the packed pair of block i lands q blocks further in the rotation's direction
          oi[(size_t)q * T + (size_t)c * L + i] = (uint64_t)c * L + (is_left ? (i + q) % L : (i + L - q) % L);
    i_lut = own.upload(S0(ss), li), i_out = own.upload(S0(ss), oi);
  }
  void release(const CudaStreamsFFI &ss) {
    drv.release(ss);
    own.release(S0(ss));
  }
};

// ------------------------------------------------------------------ column sums read in place
// The device side of a SumPlan (radix_sum.h) whose first terms are not in a pool: term ids below n_caller are rows of the
// caller's memory (integer c of a batch owns rows c * caller_rows ...), the ids from n_caller on are rows of d_pool
// (integer c owns rows c * slots ...).  Every step is one gather-sum launch into d_sum and one KS -> PBS round (message
// and carry of every group) into the pool; what is left of every column is summed into the output.
struct ColumnSum {
  SumPlan plan;
  uint32_t L = 0, n_caller = 0, caller_rows = 0, slots = 0;
  bool final_reads_caller = false;
  uint32_t nb = 0;  // integers the device arrays were built for (0: none)
  struct StepIdx {
    uint64_t *off = nullptr, *mem = nullptr, *in = nullptr, *out = nullptr, *lut = nullptr;
    uint32_t groups = 0, count = 0;
  };
  std::vector<StepIdx> steps;
  uint64_t *foff = nullptr, *fmem = nullptr;
  uint64_t *d_pool = nullptr, *d_sum = nullptr;
  size_t pool_rows = 0, sum_rows = 0;
  DeviceBlocks own, shape;  // shape: the index arrays of the plan for nb integers

  // takes the plan of columns `cols` over the degrees `deg` (deg.size() first terms, the first n_caller_ in caller rows)
  void set_plan(SumPlan &&pl, uint32_t L_, uint32_t n_caller_, uint32_t caller_rows_, size_t terms) {
    plan = std::move(pl);
    L = L_, n_caller = n_caller_, caller_rows = caller_rows_;
    slots = (uint32_t)(terms - n_caller_);
    final_reads_caller = false;
    for (auto &c : plan.final_cols)
      for (uint64_t x : c) final_reads_caller = final_reads_caller || x < n_caller;
    nb = 0;
  }
  uint64_t row(uint64_t id, uint32_t c) const {
    return id < n_caller ? kCallerRow | ((uint64_t)c * caller_rows + id) : (uint64_t)c * slots + (id - n_caller);
  }
  // rows of the pool and of the dense sums for `cts` integers of the present plan (both only ever grow)
  void reserve(hipStream_t st, uint32_t cts, size_t w) {
    const size_t pr = (size_t)cts * slots, sr = (size_t)cts * std::max<size_t>(plan.max_groups(), L);
    auto grow = [&](uint64_t *&d, size_t &have, size_t want) {
      if (want <= have) return;
      if (d) {
        HX_CHECK(hipStreamSynchronize(st));  // launches may still use the smaller buffer
        own.give_back(d);
      }
      own.alloc(d, want * w * sizeof(uint64_t));
      have = want;
    };
    grow(d_pool, pool_rows, pr);
    grow(d_sum, sum_rows, sr);
  }
  // index arrays of the plan for cts integers (build_pass of the multiplication is the model)
  void upload(hipStream_t st, uint32_t cts, uint64_t lut_msg, uint64_t lut_carry) {
    shape.release(st);  // (waits: launches of the previous plan may still read them)
    steps.clear();
    for (const SumStep &s : plan.steps) {
      StepIdx si;
      const size_t G = s.msg_slot.size(), M = s.members.size();
      std::vector<uint64_t> off(cts * G + 1), mem(cts * M), in, out, lut;
      for (uint32_t c = 0; c < cts; ++c) {
        for (size_t g = 0; g < G; ++g) {
          off[c * G + g] = c * M + s.offsets[g];
          in.push_back(c * G + g);
          out.push_back(row(s.msg_slot[g], c));
          lut.push_back(lut_msg);
          if (s.carry_slot[g] != ~(uint64_t)0) {
            in.push_back(c * G + g);
            out.push_back(row(s.carry_slot[g], c));
            lut.push_back(lut_carry);
          }
        }
        for (size_t m = 0; m < M; ++m) mem[c * M + m] = row(s.members[m], c);
      }
      off[cts * G] = cts * M;
      si.off = shape.upload(st, off), si.mem = shape.upload(st, mem);
      si.in = shape.upload(st, in), si.out = shape.upload(st, out), si.lut = shape.upload(st, lut);
      si.groups = (uint32_t)(cts * G);
      si.count = (uint32_t)in.size();
      steps.push_back(si);
    }
    std::vector<uint64_t> off{0}, mem;
    for (uint32_t c = 0; c < cts; ++c)
      for (uint32_t col = 0; col < L; ++col) {
        for (uint64_t x : plan.final_cols[col]) mem.push_back(row(x, c));
        off.push_back(mem.size());
      }
    foff = shape.upload(st, off), fmem = shape.upload(st, mem);
    nb = cts;
  }
  void reduce(const CudaStreamsFFI &ss, const LutDriver &drv, const uint64_t *caller, uint32_t w, void *const *ksks,
              void *const *bsks) const {
    for (const StepIdx &si : steps) {
      if (si.groups == 0) continue;
      HX_RANGE("column sums (%u groups)", si.groups);
      launch_gather_sum2(S0(ss), d_sum, d_pool, caller, si.off, si.mem, w, si.groups);
      drv.round(ss, d_pool, si.out, d_sum, si.in, si.lut, si.count, ksks, bsks);
    }
  }
  // out[c * L + col] = what is left of column col of integer c.  in_place: `out` holds caller rows and every output row is
  // read by its own group only; otherwise output rows that other groups read go through the dense buffer.
  void finish(hipStream_t st, uint64_t *out, const uint64_t *caller, uint32_t w, bool in_place) const {
    if (!final_reads_caller || in_place) {
      launch_gather_sum2(st, out, d_pool, caller, foff, fmem, w, nb * L);
      return;
    }
    launch_gather_sum2(st, d_sum, d_pool, caller, foff, fmem, w, nb * L);
    HX_CHECK(hipMemcpyAsync(out, d_sum, (size_t)nb * L * w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  }
  void release(hipStream_t st) {
    shape.release(st);
    own.release(st);
  }
};

// ------------------------------------------------------------------ sum of a vector of ciphertexts
// multiplication.cuh:286-485 (host_integer_partial_sum_ciphertexts_vec): V integers of `blocks` blocks, [v][block]; column
// c holds block c of every integer whose degree there is not 0.  The plan depends on the degrees: it is made by the call
// and kept, with its device arrays, until a call brings other degrees.
struct SumMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x53554D31;  // "SUM1"
  LutDriver drv;  // LUTs: 0 message, 1 carry
  uint32_t blocks = 0, max_vec = 0;
  bool reduce = false;
  ColumnSum cs;
  std::vector<uint64_t> key;  // the degrees the present plan was made for
  std::vector<uint32_t> deg;  // degree by term id of the present plan
  uint64_t last_pbs = 0;      // bootstraps of the last call

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t num_blocks, uint32_t max_num_radix_in_vec,
            bool reduce_degrees) {
    HX_PANIC_IF_FALSE(num_blocks >= 1, "partial_sum_ciphertexts_vec: no blocks");
    HX_PANIC_IF_FALSE(p.msg >= 3, "partial_sum_ciphertexts_vec: message_modulus %u < 3 is not supported", p.msg);
    blocks = num_blocks, max_vec = max_num_radix_in_vec, reduce = reduce_degrees;
    const uint64_t m = p.msg;
    std::vector<std::vector<uint64_t>> luts(2, std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    generate_lut(p, luts[0].data(), [m](uint64_t x) -> uint64_t { return x % m; });
    generate_lut(p, luts[1].data(), [m](uint64_t x) -> uint64_t { return x / m; });
    drv.init(ss, p, std::max<uint32_t>(1, std::min<uint64_t>((uint64_t)max_vec * blocks, 1u << 16)), luts);
    // sized for a full vector of clean integers; a call whose degrees need more grows it
    make_plan(std::vector<uint64_t>((size_t)max_vec * blocks, m - 1), max_vec);
    cs.reserve(S0(ss), 1, (size_t)p.big_n + 1);
  }
  void make_plan(const std::vector<uint64_t> &d, uint32_t V) {
    const Params &p = drv.p;
    std::vector<std::vector<uint64_t>> cols(blocks);
    deg.assign(d.begin(), d.end());
    for (uint32_t v = 0; v < V; ++v)
      for (uint32_t c = 0; c < blocks; ++c)
        if (d[(size_t)v * blocks + c] != 0) cols[c].push_back((uint64_t)v * blocks + c);
    SumPlan pl = plan_column_sums(std::move(cols), deg, p.msg, p.carry, false,
                                  reduce ? 2 * p.msg - 2 : p.msg * p.carry - 1);
    cs.set_plan(std::move(pl), blocks, V * blocks, V * blocks, deg.size());
    key = d;
  }
  void release(const CudaStreamsFFI &ss) {
    cs.release(S0(ss));
    drv.release(ss);
  }
};

// ------------------------------------------------------------------ multiplication by a clear scalar
// scalar_mul.cuh:47-136 takes one logical shift per set residue of the bit position (msg_bits rounds of one copy each),
// one rotated copy of the whole integer per set bit, a copy of that vector into the sum's work buffer, the sum and a carry
// propagation.  Here: ONE round bootstraps every in-block shift some set bit uses (plane r, r = 1 .. msg_bits - 1: block j
// becomes the shift-left table on msg * b[j] + b[j - 1]; plane 0 is the operand itself), bit i then contributes block j
// of plane i % msg_bits to column j + i / msg_bits as an index entry of the gather-sum kernel, the shared planner reduces
// the columns and one carry propagation finishes.  Term ids: j (plane 0, caller rows), blocks + (r - 1) blocks + j (pool).
struct ScalarMulMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x534D554C;  // "SMUL"
  LutDriver drv;  // LUTs: 0 message, 1 carry, 2 + (r - 1): shift left by r bits inside a block
  PropagateMem prop;
  uint32_t blocks = 0, max_cts = 0, bits = 0, scalar_bits = 0;
  ColumnSum cs;
  uint64_t *d_pack = nullptr;   // msg * b[j] + b[j - 1] of every block of every integer
  std::vector<uint8_t> key;     // the bits (below bits * blocks) the present plan was made for
  bool planned = false, propagate = false, any_bit = false;
  std::vector<uint64_t> pre_j, pre_r;  // the shifted blocks some set bit uses, per integer
  // device arrays of the preshift round for cs.nb integers
  uint64_t *pk0 = nullptr, *pkj = nullptr, *pkm = nullptr, *pre_in = nullptr, *pre_out = nullptr, *pre_lut = nullptr;
  DeviceBlocks own, shape;  // shape: the arrays of the preshift round

  static std::vector<uint8_t> scalar_key(const uint64_t *decomposed, uint32_t n, uint32_t limit) {
    std::vector<uint8_t> k(std::min(n, limit));
    for (size_t i = 0; i < k.size(); ++i) k[i] = decomposed[i] == 1;
    while (!k.empty() && !k.back()) k.pop_back();
    return k;
  }
  void make_plan(const std::vector<uint8_t> &k) {
    const Params &p = drv.p;
    const uint32_t L = blocks, m = p.msg;
    std::vector<std::vector<uint64_t>> cols(L);
    std::vector<uint32_t> deg((size_t)L * bits, m - 1);
    std::vector<uint32_t> used(bits, 0);  // blocks of plane r some set bit uses: j < used[r]
    any_bit = false;
    for (size_t i = 0; i < k.size(); ++i) {
      if (!k[i]) continue;
      any_bit = true;
      const uint32_t r = (uint32_t)(i % bits), q = (uint32_t)(i / bits);
      used[r] = std::max(used[r], L - q);
      for (uint32_t j = 0; j + q < L; ++j) cols[j + q].push_back(r == 0 ? j : (uint64_t)L + (uint64_t)(r - 1) * L + j);
    }
    pre_j.clear(), pre_r.clear();
    for (uint32_t r = 1; r < bits; ++r)
      for (uint32_t j = 0; j < used[r]; ++j) pre_j.push_back(j), pre_r.push_back(r);
    SumPlan pl = plan_column_sums(std::move(cols), deg, m, p.carry, max_cts >= 8, 2 * m - 2);
    propagate = false;  // every column a single clean term or nothing (a power of two): nothing to propagate
    for (auto &c : pl.final_cols) propagate = propagate || c.size() > 1;
    cs.set_plan(std::move(pl), L, L, L, deg.size());
    key = k;
    planned = true;
  }
  uint64_t pbs_count() const {
    return pre_j.size() + cs.plan.bootstraps() + (propagate ? PropagateMem::pbs_count(blocks) : 0);
  }

  void init(const CudaStreamsFFI &ss, const Params &p, uint32_t num_blocks, uint32_t cts, uint32_t num_scalar_bits) {
    HX_PANIC_IF_FALSE(num_blocks >= 1, "integer_scalar_mul: no blocks");
    HX_PANIC_IF_FALSE((p.msg & (p.msg - 1)) == 0, "integer_scalar_mul: the message modulus must be a power of two");
    blocks = num_blocks, max_cts = cts;
    bits = (uint32_t)__builtin_ctz(p.msg);
    scalar_bits = std::min(num_scalar_bits, bits * blocks);
    const uint64_t m = p.msg;
    std::vector<std::vector<uint64_t>> luts(1 + bits, std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    generate_lut(p, luts[0].data(), [m](uint64_t x) -> uint64_t { return x % m; });
    generate_lut(p, luts[1].data(), [m](uint64_t x) -> uint64_t { return x / m; });
    for (uint32_t r = 1; r < bits; ++r) generate_lut(p, luts[1 + r].data(), shift_in_block(p.msg, bits, r, true));
    const uint64_t widest = (uint64_t)cts * blocks * std::max(bits, scalar_bits);  // no round holds more blocks
    drv.init(ss, p, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(widest, 1u << 16)), luts);
    const size_t w = (size_t)p.big_n + 1;
    own.alloc(d_pack, (size_t)cts * blocks * w * sizeof(uint64_t));
    prop.init(ss, p, num_blocks, cts);
    // sized for the scalar with every bit set; a wider plan (there is none among the scalars tried) grows it
    make_plan(std::vector<uint8_t>(scalar_bits, 1));
    cs.reserve(S0(ss), cts, w);
    planned = false;
  }

  void upload(hipStream_t st, uint32_t cts) {
    cs.upload(st, cts, 0, 1);
    shape.release(st);
    const uint32_t L = blocks;
    std::vector<uint64_t> r0, rj, rm, in, out, lut;
    for (uint32_t c = 0; c < cts; ++c) {
      r0.push_back((uint64_t)c * L);
      for (uint32_t j = 1; j < L; ++j) rj.push_back((uint64_t)c * L + j), rm.push_back((uint64_t)c * L + j - 1);
      for (size_t s = 0; s < pre_j.size(); ++s) {
        in.push_back((uint64_t)c * L + pre_j[s]);
        out.push_back((uint64_t)c * cs.slots + (pre_r[s] - 1) * L + pre_j[s]);
        lut.push_back(1 + pre_r[s]);
      }
    }
    pk0 = shape.upload(st, r0), pkj = shape.upload(st, rj), pkm = shape.upload(st, rm);
    pre_in = shape.upload(st, in), pre_out = shape.upload(st, out), pre_lut = shape.upload(st, lut);
  }

  // v <- v * scalar for `cts` integers (the plan of the scalar is in place)
  void run(const CudaStreamsFFI &ss, uint64_t *v, uint32_t cts, void *const *ksks, void *const *bsks) {
    const hipStream_t st = S0(ss);
    const Params &p = drv.p;
    const uint32_t L = blocks, w = p.big_n + 1;
    cs.reserve(st, cts, w);
    if (cs.nb != cts) upload(st, cts);
    HX_RANGE("integer scalar mul: %u integers of %u blocks", cts, L);
    if (!pre_j.empty()) {
      HX_RANGE("shifted blocks");
      axpy(st, d_pack, pk0, v, pk0, p.msg, nullptr, nullptr, w, cts);
      axpy(st, d_pack, pkj, v, pkj, p.msg, v, pkm, w, cts * (L - 1));
      drv.round(ss, cs.d_pool, pre_out, d_pack, pre_in, pre_lut, (uint32_t)(cts * pre_j.size()), ksks, bsks);
    }
    cs.reduce(ss, drv, v, w, ksks, bsks);
    cs.finish(st, v, v, w, false);
    if (propagate) prop.run(ss, v, cts, ksks, bsks);
  }

  void release(const CudaStreamsFFI &ss) {
    cs.release(S0(ss));
    drv.release(ss);
    prop.release(ss);
    shape.release(S0(ss));
    own.release(S0(ss));
  }
};

// ------------------------------------------------------------------ ciphertext compression
// tfhe/src/shortint/list_compression/compression.rs:17-133 (compress), :137-254 (decompress); the reference's GPU flow is
// cuda/src/integer/compression/compression.cuh:199-291 and :293-554.  The kernels are keyswitch.hip (packing keyswitch
// and its fused rotate / sum / modulus switch / bit-pack epilogue) and ciphertext.hip (unpack + sample extract).
struct CompressionShape {
  uint32_t n_in = 0, k = 0, N = 0, base_log = 0, level = 0;  // packing key: [n_in][level][(k+1)*N]
  uint32_t ncols() const { return (k + 1) * N; }
};
static void check_compression_glwe(uint32_t k, uint32_t N, const char *who) {
  HX_PANIC_IF_FALSE(k >= 1 && N >= 16 && (N & (N - 1)) == 0,
                    "%s: compression GLWE needs glwe_dimension >= 1 and a power-of-two polynomial_size >= 16 (got %u, %u)", who,
                    k, N);
}
static void check_storage(uint32_t N, uint32_t lwe_per_glwe, uint32_t bits, const char *who) {
  HX_PANIC_IF_FALSE(lwe_per_glwe >= 1 && lwe_per_glwe <= N, "%s: lwe_per_glwe %u must be in 1..polynomial_size (%u)", who,
                    lwe_per_glwe, N);
  HX_PANIC_IF_FALSE(bits >= 1 && bits <= 63, "%s: storage_log_modulus %u must be in 1..63", who, bits);
}
static uint32_t packed_words_per_glwe(uint32_t k, uint32_t N, uint32_t lwe_per_glwe, uint32_t bits) {
  return (uint32_t)((((uint64_t)k * N + lwe_per_glwe) * bits + 63) / 64);
}

// core level: LWE list -> unswitched GLWEs
struct PackingKsMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x504B5331;  // "PKS1"
  CompressionShape sh;
  uint32_t cap = 0;  // LWEs per call
  uint64_t *d_rows = nullptr, *d_trivial = nullptr;
  DeviceBlocks own;
  void init(const CudaStreamsFFI &s, const CompressionShape &shape, uint32_t capacity) {
    sh = shape;
    cap = std::max(1u, capacity);
    own.alloc(d_rows, (size_t)cap * sh.ncols() * sizeof(uint64_t));
    std::vector<uint64_t> triv(cap);
    for (uint32_t i = 0; i < cap; ++i) triv[i] = i;
    d_trivial = own.upload(S0(s), triv);
  }
  void release(const CudaStreamsFFI &s) { own.release(S0(s)); }
};

struct CompressMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x434D5052;  // "CMPR"
  PackingKsMem pks;  // member: no header of its own in use
  uint32_t msg = 0, carry = 0, lwe_per_glwe = 0, bits = 0;
  uint64_t *d_scaled = nullptr;  // the input blocks times message_modulus
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    pks.release(s);
    own.release(S0(s));
  }
};

struct DecompressMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x44434D50;  // "DCMP"
  Params p{};          // the compute set; small_n = k_c * N_c, the decompression key's input dimension
  uint32_t kc = 0, Nc = 0, lwe_per_glwe = 0, bits = 0, cap = 0, gpu = 0;
  uint64_t *d_extracted = nullptr, *d_lut = nullptr, *d_trivial = nullptr, *d_lut_idx = nullptr;
  uint32_t *d_indexes = nullptr, *h_indexes = nullptr;  // h_indexes: pinned staging of the caller's host array
  hipEvent_t uploaded = nullptr;                         // behind the last copy out of h_indexes
  int8_t *pbs_buf = nullptr;
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    const hipStream_t st = S0(s);
    if (pbs_buf) {
      if (p.grouping) cleanup_cuda_multi_bit_programmable_bootstrap_64(st, gpu, &pbs_buf);
      else cleanup_cuda_programmable_bootstrap_64(st, gpu, &pbs_buf);
    }
    own.release(st);
    if (h_indexes) HX_CHECK(hipHostFree(h_indexes));
    if (uploaded) HX_CHECK(hipEventDestroy(uploaded));
  }
};

// compression.rs:137-162 (rescaling_lut): the identity from the encoding the blocks have after the multiplication by
// message_modulus (plaintext modulus `carry`, no carry space) to the compute encoding (delta = 2^63 / (msg * carry))
static void generate_rescaling_lut(const Params &p, uint64_t *acc) {
  const uint32_t sup = p.carry, box = p.N / sup;
  std::fill(acc, acc + (size_t)p.k * p.N, 0);
  uint64_t *body = acc + (size_t)p.k * p.N;
  for (uint32_t i = 0; i < sup; ++i)
    for (uint32_t j = i * box; j < (i + 1) * box; ++j) body[j] = (uint64_t)i * p.delta();
  const uint32_t half = box / 2;
  for (uint32_t i = 0; i < half; ++i) body[i] = (uint64_t)0 - body[i];
  std::rotate(body, body + half, body + p.N);
}

// Noise squashing of a radix ciphertext (integer.cuh:2776-2840): pairs of clean blocks packed, keyswitched and
// bootstrapped over the 128-bit torus with the identity table
struct NoiseSquashMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x4E535131;  // "NSQ1"
  uint32_t big_n = 0, small_n = 0, k = 0, N = 0, ks_base_log = 0, ks_level = 0, pbs_base_log = 0, pbs_level = 0;
  uint32_t msg = 0, carry = 0, cap_in = 0, cap_out = 0, gpu = 0;
  uint64_t *d_packed = nullptr, *d_after_ks = nullptr, *d_trivial = nullptr, *d_lo = nullptr, *d_hi = nullptr;
  unsigned __int128 *d_lut = nullptr;
  int8_t *pbs_buf = nullptr;
  uint32_t grouping = 0;  // the kind: 0 a classic 128-bit key, otherwise the grouping factor of a multi-bit one
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    if (pbs_buf && grouping) hip_cleanup_multi_bit_programmable_bootstrap_128(S0(s), gpu, &pbs_buf);
    else if (pbs_buf) hip_cleanup_programmable_bootstrap_128(S0(s), gpu, &pbs_buf);
    own.release(S0(s));
  }
};

// Expansion of compact ciphertext lists (cuda/include/zk/zk_utilities.h zk_expand_mem, cuda/src/zk/zk.cuh): the shared
// mask of a list rotated once per body (launch_lwe_expand, ciphertext.hip), cast to the compute key, every packed body
// split into its message and carry block by ONE round of the driver over 2 * num_lwes blocks.
struct ExpandMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x58504E44;  // "XPND"
  uint32_t kind = 0, ks_type = 0;  // EXPAND_KIND, KS_TYPE
  uint32_t n_c = 0;                // the casting key's input dimension: the compact lists' mask length
  uint32_t cast_out_n = 0, cast_base_log = 0, cast_level = 0;  // SMALL_TO_BIG: the casting keyswitch of its own
  uint32_t num_lwes = 0, gpu = 0;
  LutDriver drv;  // (not set up where nothing is bootstrapped)
  ExpandJob *d_jobs = nullptr;  // per output row: where its list's mask starts, which body it takes (built once, here)
  uint64_t *d_expanded = nullptr, *d_cast = nullptr, *d_in_idx = nullptr, *d_out_idx = nullptr, *d_lut_idx = nullptr;
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    drv.release(s);
    own.release(S0(s));
  }
};

// Re-randomisation (cuda/include/integer/rerand_utilities.h int_rerand_mem, cuda/src/integer/rerand.cuh): every block
// gains a fresh encryption of zero out of ONE compact list.  Without keyswitch the list is under the blocks' own key and
// the scratch holds nothing on the device: launch_lwe_rerand_add rotates and adds in place.  With keyswitch the zeros are
// expanded (launch_lwe_expand with the identity job table built here), keyswitched to the blocks' key and added.
struct RerandMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x52524E44;  // "RRND"
  uint32_t mode = 0;                               // RERAND_MODE
  uint32_t n_in = 0, n_out = 0, base_log = 0, level = 0;  // zeros' dimension; with keyswitch: the blocks' and the key's shape
  uint32_t count = 0, gpu = 0;
  ExpandJob *d_jobs = nullptr;  // row o: the list's mask (offset 0) times X^o
  uint64_t *d_expanded = nullptr, *d_switched = nullptr, *d_trivial = nullptr;
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) { own.release(S0(s)); }
};

// Oblivious pseudo-random bits (cuda/include/integer/oprf.h int_grouped_oprf_memory, cuda/src/integer/oprf.cuh;
// tfhe/src/shortint/oprf.rs generate_oprf_lut): seeded LWEs under the small key are bootstrapped as they are — no
// keyswitch — with the table of their bit count, and a plaintext correction lands on the bodies.
struct OprfMem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x4F505246;  // "OPRF"
  uint32_t num_blocks = 0, gpu = 0;
  LutDriver drv;                      // no_ks: one table per bit count b = 1 .. message bits, table b - 1
  std::vector<uint32_t> bits;         // per block: the random bits it takes
  uint64_t *d_lut_idx = nullptr;      // per block: bits - 1
  uint64_t *d_corrections = nullptr;  // per block: (2^bits - 1) * delta / 2, added to the body
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    drv.release(s);
    own.release(S0(s));
  }
};

}  // namespace radix
}  // namespace tfhe_hip

#include "radix_trivium.h"  // TriviumMem and the tap kernel, on the round driver and the owners above
#include "radix_divrem.h"   // DivRemMem, AbsMem and the stage kernel, on the round driver and the carry propagation
#include "radix_bitcount.h" // the bit-count scratches and the pair-pack kernel, on the round driver, the sums and the propagation
#include "radix_aes.h"      // AesMem, the gate scheduler and the gate-sum kernel, on the round driver

using namespace tfhe_hip;
using namespace tfhe_hip::radix;

extern "C" {

// ---- cuda/include/integer/integer.h:127-160 ------------------------------------------------
static uint64_t scratch_apply_lut(CudaStreamsFFI streams, int8_t **mem_ptr, void const *input_lut,
                                  CudaLweBootstrapKeyParamsFFI bsk_params, CudaLweKeyswitchKeyParamsFFI ksk_params,
                                  uint32_t count, uint32_t message_modulus, uint32_t carry_modulus, uint32_t num_many_lut,
                                  uint64_t lut_degree, bool allocate_gpu_memory, uint32_t noise_reduction_type) {
  HX_PANIC_IF_FALSE(input_lut != nullptr && mem_ptr != nullptr, "apply_univariate_lut: null pointer");
  HX_PANIC_IF_FALSE(num_many_lut >= 1, "apply_many_univariate_lut: num_many_lut must be at least 1");
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, noise_reduction_type);
  return scratch_create<ApplyLutMem>(streams, mem_ptr, allocate_gpu_memory, "apply_univariate_lut", [&](ApplyLutMem &m) {
    const size_t lw = (size_t)(p.k + 1) * p.N, idx_bytes = std::max<uint32_t>(1, count) * sizeof(uint64_t);
    std::vector<std::vector<uint64_t>> luts(1);
    luts[0].assign((const uint64_t *)input_lut, (const uint64_t *)input_lut + lw);
    m.drv.init(streams, p, std::max<uint32_t>(1, count), luts);
    m.degree = lut_degree;
    m.num_many_lut = num_many_lut;
    m.own.alloc(m.d_lut_idx, idx_bytes);
    if (!t_dry) HX_CHECK(hipMemsetAsync(m.d_lut_idx, 0, idx_bytes, S0(streams)));
  });
}

uint64_t scratch_cuda_apply_univariate_lut_64_async(CudaStreamsFFI streams, int8_t **mem_ptr, void const *input_lut,
                                                    CudaLweBootstrapKeyParamsFFI bsk_params,
                                                    CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                    uint32_t input_lwe_ciphertext_count, uint32_t message_modulus,
                                                    uint32_t carry_modulus, uint64_t lut_degree,
                                                    bool allocate_gpu_memory,
                                                    enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_apply_lut(streams, mem_ptr, input_lut, bsk_params, ksk_params, input_lwe_ciphertext_count,
                           message_modulus, carry_modulus, 1, lut_degree, allocate_gpu_memory,
                           (uint32_t)noise_reduction_type);
}

// input_lut: ONE accumulator holding num_many_lut functions in sub-tables of lut_stride coefficients
// (tfhe/src/shortint/engine/mod.rs:169-254 fill_many_lut_accumulator)
uint64_t scratch_cuda_apply_many_univariate_lut_64_async(CudaStreamsFFI streams, int8_t **mem_ptr, void const *input_lut,
                                                         CudaLweBootstrapKeyParamsFFI bsk_params,
                                                         CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                         uint32_t num_radix_blocks, uint32_t message_modulus,
                                                         uint32_t carry_modulus, uint32_t num_many_lut,
                                                         uint64_t lut_degree, bool allocate_gpu_memory,
                                                         enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_apply_lut(streams, mem_ptr, input_lut, bsk_params, ksk_params, num_radix_blocks, message_modulus,
                           carry_modulus, num_many_lut, lut_degree, allocate_gpu_memory, (uint32_t)noise_reduction_type);
}

void cuda_apply_univariate_lut_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_radix_lwe,
                                        CudaRadixCiphertextFFI const *input_radix_lwe, int8_t *mem_ptr,
                                        void *const *ksks, void *const *bsks) {
  first_gpu(streams);
  auto *m = scratch_use<ApplyLutMem>(mem_ptr, "apply_univariate_lut");
  HX_PANIC_IF_FALSE(output_radix_lwe && input_radix_lwe && ksks && bsks, "apply_univariate_lut: null pointer");
  HX_PANIC_IF_FALSE(output_radix_lwe->lwe_dimension == input_radix_lwe->lwe_dimension,
                    "input and output radix ciphertexts should have the same lwe dimension");
  const uint32_t n = input_radix_lwe->num_radix_blocks;
  HX_PANIC_IF_FALSE(n <= m->drv.cap && n <= output_radix_lwe->num_radix_blocks,
                    "num radix blocks on which lut is applied should be smaller or equal to the number of lut radix "
                    "blocks");
  m->drv.round(streams, (uint64_t *)output_radix_lwe->ptr, nullptr, (const uint64_t *)input_radix_lwe->ptr, nullptr,
               m->d_lut_idx, n, ksks, bsks);
  set_block_info(output_radix_lwe, 0, n, m->degree, 1);
}

void cleanup_cuda_apply_univariate_lut_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ApplyLutMem>(streams, mem_ptr_void, "cleanup apply_univariate_lut");
}

// integer.cuh:1002-1110: the output holds num_many_lut * n blocks, function t of input block s in block t * n + s
void cuda_apply_many_univariate_lut_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_radix_lwe,
                                             CudaRadixCiphertextFFI const *input_radix_lwe, int8_t *mem_ptr,
                                             void *const *ksks, void *const *bsks, uint32_t num_luts,
                                             uint32_t lut_stride) {
  first_gpu(streams);
  auto *m = scratch_use<ApplyLutMem>(mem_ptr, "apply_many_univariate_lut");
  HX_PANIC_IF_FALSE(output_radix_lwe && input_radix_lwe && ksks && bsks, "apply_many_univariate_lut: null pointer");
  HX_PANIC_IF_FALSE(num_luts >= 1 && num_luts <= m->num_many_lut,
                    "apply_many_univariate_lut: more functions than the scratch was created for");
  const uint32_t n = input_radix_lwe->num_radix_blocks;
  HX_PANIC_IF_FALSE((uint64_t)output_radix_lwe->num_radix_blocks >= (uint64_t)n * num_luts,
                    "output radix ciphertext should have at least num_many_lut times the number of blocks of the input");
  HX_PANIC_IF_FALSE(output_radix_lwe->lwe_dimension == input_radix_lwe->lwe_dimension,
                    "input and output radix ciphertexts should have the same lwe dimension");
  HX_PANIC_IF_FALSE((uint64_t)(num_luts - 1) * lut_stride < m->drv.p.N,
                    "apply_many_univariate_lut: lut_stride * (num_luts - 1) reaches past the polynomial");
  m->drv.round_many(streams, (uint64_t *)output_radix_lwe->ptr, (const uint64_t *)input_radix_lwe->ptr, m->d_lut_idx, n,
                    ksks, bsks, num_luts, lut_stride);
  set_block_info(output_radix_lwe, 0, n * num_luts, m->degree, 1);
}

void cleanup_cuda_apply_many_univariate_lut_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  cleanup_cuda_apply_univariate_lut_64(streams, mem_ptr_void);
}

// ---- cuda/include/linear_algebra.h:26-28 -----------------------------------------------------
void cuda_add_lwe_ciphertext_vector_inplace_64(void *stream, uint32_t gpu_index,
                                               CudaRadixCiphertextFFI *lwe_array_inout,
                                               CudaRadixCiphertextFFI const *input_2) {
  (void)gpu_index;
  HX_PANIC_IF_FALSE(lwe_array_inout && input_2 && lwe_array_inout->num_radix_blocks == input_2->num_radix_blocks &&
                        lwe_array_inout->lwe_dimension == input_2->lwe_dimension,
                    "add: operands must have the same shape");
  axpy((hipStream_t)stream, (uint64_t *)lwe_array_inout->ptr, nullptr, (const uint64_t *)lwe_array_inout->ptr, nullptr,
       1, (const uint64_t *)input_2->ptr, nullptr, lwe_array_inout->lwe_dimension + 1,
       lwe_array_inout->num_radix_blocks);
  for (uint32_t i = 0; i < lwe_array_inout->num_radix_blocks; ++i) {
    if (lwe_array_inout->degrees && input_2->degrees) lwe_array_inout->degrees[i] += input_2->degrees[i];
    if (lwe_array_inout->noise_levels && input_2->noise_levels)
      lwe_array_inout->noise_levels[i] += input_2->noise_levels[i];
  }
}

// The carry tree's first bootstrap holds two functions in its accumulator, so a block's value must stay below
// msg * carry / 2: at most 2 msg - 2 (two clean blocks added), one more for block 0 of an integer when an input carry
// is added to it.  A caller that tracks degrees gets the call refused instead of an incorrect result.
static void check_propagation_degrees(const CudaRadixCiphertextFFI *ct, uint32_t msg, const char *who) {
  if (ct == nullptr || ct->degrees == nullptr) return;
  for (uint32_t i = 0; i < ct->num_radix_blocks; ++i) {
    const uint64_t limit = 2ull * msg - 2;  // (the input carry itself comes on top of block 0: 2 msg - 1 there is fine)
    HX_PANIC_IF_FALSE(ct->degrees[i] <= limit,
                      "%s: block %u has degree %llu, the carry propagation accepts at most %llu (propagate the operands first)",
                      who, i, (unsigned long long)ct->degrees[i], (unsigned long long)limit);
  }
}

// ---- cuda/include/integer/integer.h:383-413 --------------------------------------------------
// num_blocks = blocks per integer; the ciphertexts handed to the launch may hold any whole number
// of integers up to the capacity given through hip_integer_scratch_batch (default 1).
// read by the NEXT scratch_* call of the same host thread (the radix scratch entry points have no batch parameter in
// the reference's prototypes): thread-local, so that concurrent host threads size their own scratches
// (comparison and cmux ignore it: one integer per call)
static thread_local uint32_t g_scratch_batch = 1;
void hip_integer_scratch_batch(uint32_t num_integers) { g_scratch_batch = num_integers ? num_integers : 1; }
// blocks per GPU from which a KS -> PBS round spreads over one more GPU of the stream set; 0 restores the default, the
// reference's THRESHOLD_MULTI_GPU_* rule (helper_multi_gpu.cu:12-48); tests lower it
void hip_integer_set_multi_gpu_threshold(uint32_t blocks_per_gpu) {
  radix::g_multi_gpu_min_blocks.store(blocks_per_gpu);  // 0: the reference's rule (12 multi-bit, compute units + 1 classic)
}
// how many GPUs of a set of `gpu_count` a round of `num_blocks` blocks uses (get_active_gpu_count): for callers and tests
uint32_t hip_integer_active_gpu_count(uint32_t num_blocks, uint32_t gpu_count, uint32_t pbs_type, uint32_t first_gpu) {
  radix::Params p{};
  p.grouping = pbs_type == MULTI_BIT ? 1u : 0u;
  const uint32_t th = radix::multi_gpu_threshold(p, first_gpu);
  return std::max(1u, std::min(gpu_count, (num_blocks + th - 1) / th));
}

uint64_t scratch_cuda_propagate_single_carry_64_inplace_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                              CudaLweBootstrapKeyParamsFFI bsk_params,
                                                              CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                              uint32_t num_blocks, uint32_t message_modulus,
                                                              uint32_t carry_modulus, uint32_t requested_flag,
                                                              bool allocate_gpu_memory,
                                                              enum PBS_MS_REDUCTION_T noise_reduction_type) {
  HX_PANIC_IF_FALSE(requested_flag <= 2, "propagate_single_carry: unknown output flag %u", requested_flag);
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<PropagateMem>(streams, mem_ptr, allocate_gpu_memory, "propagate_single_carry",
                                      [&](PropagateMem &m) { m.init(streams, p, num_blocks, g_scratch_batch); });
}
uint64_t scratch_cuda_add_and_propagate_single_carry_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
    uint32_t requested_flag, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_cuda_propagate_single_carry_64_inplace_async(streams, mem_ptr, bsk_params, ksk_params, num_blocks,
                                                              message_modulus, carry_modulus, requested_flag,
                                                              allocate_gpu_memory, noise_reduction_type);
}

void cuda_propagate_single_carry_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
                                                  CudaRadixCiphertextFFI *carry_out,
                                                  const CudaRadixCiphertextFFI *carry_in, int8_t *mem_ptr,
                                                  void *const *bsks, void *const *ksks, uint32_t requested_flag,
                                                  uint32_t uses_carry) {
  first_gpu(streams);
  auto *m = scratch_use<PropagateMem>(mem_ptr, "propagate_single_carry");
  // integer.cuh:2368-2370: the overflow flag needs the operands of the addition
  HX_PANIC_IF_FALSE(requested_flag != 1, "single carry propagation is not supported for overflow, try using "
                                         "add_and_propagate_single_carry");
  HX_PANIC_IF_FALSE(requested_flag == 0 || requested_flag == 2, "propagate_single_carry: unknown output flag %u",
                    requested_flag);
  const uint32_t cts = batch_of(lwe_array, m->blocks, "propagate_single_carry");
  check_propagation_degrees(lwe_array, m->drv.p.msg, "propagate_single_carry");
  // the reference's Rust caller always hands over carry_in / carry_out structs (integer/gpu/ffi.rs:2213-2237);
  // they are read / written only when uses_carry / requested_flag say so
  const uint64_t *cin = nullptr;
  uint64_t *cout = nullptr;
  if (uses_carry != 0)
    cin = carry_blocks(carry_in, cts, lwe_array, "propagate_single_carry: uses_carry needs one input carry block per integer");
  if (requested_flag == 2)
    cout = carry_blocks(carry_out, cts, lwe_array, "propagate_single_carry: FLAG_CARRY needs one output carry block per integer");
  m->run(streams, (uint64_t *)lwe_array->ptr, cts, ksks, bsks, cin, cout);
  if (cout) set_block_info(carry_out, 0, cts, 1, 1);
  set_block_info(lwe_array, 0, lwe_array->num_radix_blocks, m->drv.p.msg - 1, 1);
}

void cuda_add_and_propagate_single_carry_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lhs_array,
                                                          const CudaRadixCiphertextFFI *rhs_array,
                                                          CudaRadixCiphertextFFI *carry_out,
                                                          const CudaRadixCiphertextFFI *carry_in, int8_t *mem_ptr,
                                                          void *const *bsks, void *const *ksks,
                                                          uint32_t requested_flag, uint32_t uses_carry) {
  first_gpu(streams);
  if (requested_flag != 1) {
    cuda_add_lwe_ciphertext_vector_inplace_64(streams.streams[0], G0(streams), lhs_array, rhs_array);
    cuda_propagate_single_carry_64_inplace_async(streams, lhs_array, carry_out, carry_in, mem_ptr, bsks, ksks,
                                                 requested_flag, uses_carry);
    return;
  }
  // FLAG_OVERFLOW (integer.cuh:2493-2520, integer_utilities.h:2311-2357): carry_out receives the signed-overflow flag of
  // lhs + rhs (+ carry_in) — the carry into the sign bit against the carry out of the last block.  The operands' last
  // blocks are read before the addition; both operands are clean (degrees <= msg - 1: the preparation is a bivariate
  // table of the two last blocks).
  auto *m = scratch_use<PropagateMem>(mem_ptr, "add_and_propagate_single_carry");
  HX_PANIC_IF_FALSE(lhs_array && rhs_array && lhs_array->num_radix_blocks == rhs_array->num_radix_blocks &&
                        lhs_array->lwe_dimension == rhs_array->lwe_dimension,
                    "add_and_propagate_single_carry: operands must have the same shape");
  const uint32_t cts = batch_of(lhs_array, m->blocks, "add_and_propagate_single_carry");
  uint64_t *ovf = carry_blocks(carry_out, cts, lhs_array,
                               "when requesting FLAG_CARRY or FLAG_OVERFLOW, carry_out must be a valid pointer (one block per integer)");
  const uint32_t msg = m->drv.p.msg;
  for (const CudaRadixCiphertextFFI *op : {(const CudaRadixCiphertextFFI *)lhs_array, rhs_array})
    if (op->degrees)
      for (uint32_t c = 0; c < cts; ++c)
        HX_PANIC_IF_FALSE(op->degrees[(size_t)(c + 1) * m->blocks - 1] <= msg - 1,
                          "add_and_propagate_single_carry: FLAG_OVERFLOW needs clean last blocks (degree %llu > %u)",
                          (unsigned long long)op->degrees[(size_t)(c + 1) * m->blocks - 1], msg - 1);
  const uint64_t *cin = nullptr;
  if (uses_carry != 0)
    cin = carry_blocks(carry_in, cts, lhs_array, "add_and_propagate_single_carry: uses_carry needs one input carry block per integer");
  m->pack_last_blocks(streams, (const uint64_t *)lhs_array->ptr, (const uint64_t *)rhs_array->ptr, cts);
  cuda_add_lwe_ciphertext_vector_inplace_64(streams.streams[0], G0(streams), lhs_array, rhs_array);
  check_propagation_degrees(lhs_array, msg, "add_and_propagate_single_carry");
  m->run(streams, (uint64_t *)lhs_array->ptr, cts, ksks, bsks, cin, nullptr, ovf);
  set_block_info(carry_out, 0, cts, 1, 1);
  set_block_info(lhs_array, 0, lhs_array->num_radix_blocks, msg - 1, 1);
}

void cleanup_cuda_propagate_single_carry_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<PropagateMem>(streams, mem_ptr_void, "cleanup propagate_single_carry");
}
void cleanup_cuda_add_and_propagate_single_carry_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  cleanup_cuda_propagate_single_carry_64_inplace(streams, mem_ptr_void);
}

// ---- cuda/include/integer/integer.h:173-187 --------------------------------------------------
uint64_t scratch_cuda_integer_mult_inplace_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                    bool const is_boolean_left, bool const is_boolean_right,
                                                    uint32_t message_modulus, uint32_t carry_modulus,
                                                    CudaLweBootstrapKeyParamsFFI bsk_params,
                                                    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
                                                    bool allocate_gpu_memory,
                                                    enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  if (is_boolean_left || is_boolean_right)  // one operand is an encrypted boolean: a select, not a product
    return scratch_create<BoolMulMem>(streams, mem_ptr, allocate_gpu_memory, "integer_mult",
                                      [&](BoolMulMem &m) { m.init(streams, p, num_blocks, g_scratch_batch); });
  return scratch_create<MulMem>(streams, mem_ptr, allocate_gpu_memory, "integer_mult",
                                [&](MulMem &m) { m.init(streams, p, num_blocks, g_scratch_batch); });
}

void cuda_integer_mult_inplace_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *radix_lwe_inout,
                                        bool const is_bool_left, CudaRadixCiphertextFFI const *radix_lwe_right,
                                        bool const is_bool_right, void *const *bsks, void *const *ksks,
                                        int8_t *mem_ptr, uint32_t polynomial_size, uint32_t num_blocks) {
  first_gpu(streams);
  if (is_bool_left || is_bool_right) {
    // multiplication.cuh:508-520: the boolean operand is ONE block (here: one per integer of the batch, packed at the
    // start of its ciphertext); the other operand's blocks are kept or zeroed.  In place on radix_lwe_inout, which
    // holds the full-width integers either way (as the left operand, or as the destination when it is the boolean).
    HX_PANIC_IF_FALSE(scratch_magic(mem_ptr) == BoolMulMem::kMagic,
                      "integer_mult: boolean operands need a scratch created with is_boolean_left / is_boolean_right");
    auto *bm = scratch_use<BoolMulMem>(mem_ptr, "integer_mult");
    HX_PANIC_IF_FALSE(polynomial_size == bm->drv.p.N && num_blocks == bm->blocks, "integer_mult: call does not match the scratch");
    HX_PANIC_IF_FALSE(radix_lwe_inout && radix_lwe_right && radix_lwe_inout->lwe_dimension == radix_lwe_right->lwe_dimension,
                      "integer_mult: input and output lwe dimensions should be the same");
    const uint32_t cts = batch_of(radix_lwe_inout, bm->blocks, "integer_mult");
    const CudaRadixCiphertextFFI *cond = is_bool_right ? radix_lwe_right : radix_lwe_inout;
    const CudaRadixCiphertextFFI *value = is_bool_right ? (const CudaRadixCiphertextFFI *)radix_lwe_inout : radix_lwe_right;
    HX_PANIC_IF_FALSE(cond->num_radix_blocks >= cts && value->num_radix_blocks >= cts * bm->blocks,
                      "integer_mult: input or output does not have enough radix blocks");
    // the packing msg * value + condition must stay below the padding bit: clean value blocks, a boolean that IS one
    if (value->degrees)
      for (uint32_t i = 0; i < cts * bm->blocks; ++i)
        HX_PANIC_IF_FALSE(value->degrees[i] <= bm->drv.p.msg - 1,
                          "integer_mult: block %u of the non-boolean operand has degree %llu, at most %u is accepted (propagate it first)",
                          i, (unsigned long long)value->degrees[i], bm->drv.p.msg - 1);
    if (cond->degrees)
      for (uint32_t c = 0; c < cts; ++c)
        HX_PANIC_IF_FALSE(cond->degrees[c] <= 1, "integer_mult: the boolean operand's block %u has degree %llu", c,
                          (unsigned long long)cond->degrees[c]);
    // (a boolean that sits in the destination is read by the packing launch before the bootstrap overwrites it)
    bm->run(streams, (uint64_t *)radix_lwe_inout->ptr, (const uint64_t *)value->ptr, (const uint64_t *)cond->ptr, cts,
            ksks, bsks);
    set_block_info(radix_lwe_inout, 0, cts * bm->blocks, bm->drv.p.msg - 1, 1);
    return;
  }
  auto *m = scratch_use<MulMem>(mem_ptr, "integer_mult");
  HX_PANIC_IF_FALSE(polynomial_size == m->drv.p.N && num_blocks == m->blocks, "integer_mult: call does not match the scratch");
  const uint32_t cts = batch_of(radix_lwe_inout, m->blocks, "integer_mult");
  HX_PANIC_IF_FALSE(radix_lwe_right && radix_lwe_right->num_radix_blocks == radix_lwe_inout->num_radix_blocks,
                    "integer_mult: operands must have the same shape");
  m->run(streams, (uint64_t *)radix_lwe_inout->ptr, (const uint64_t *)radix_lwe_right->ptr, cts, ksks, bsks);
  set_block_info(radix_lwe_inout, 0, radix_lwe_inout->num_radix_blocks, m->drv.p.msg - 1, 1);
}

void cleanup_cuda_integer_mult_inplace_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  if (scratch_magic(*mem_ptr_void) == BoolMulMem::kMagic)
    scratch_destroy<BoolMulMem>(streams, mem_ptr_void, "cleanup integer_mult");
  else
    scratch_destroy<MulMem>(streams, mem_ptr_void, "cleanup integer_mult");
}

// ---- cuda/include/integer/integer.h:189-198, :312-316 ------------------------------------------
// negation.cuh:85-155 (host_negation_with_correcting_term): block 0 becomes z - b, every later block z - (b + z / msg)
// with z = msg, so that the blocks stay non-negative and the borrowed unit is handed to the next block; the degrees
// follow the reference's loop (including its integer division inside the ceil)
void cuda_negate_ciphertext_64(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                               CudaRadixCiphertextFFI const *lwe_array_in, uint32_t message_modulus,
                               uint32_t carry_modulus, uint32_t num_radix_blocks) {
  first_gpu(streams);
  HX_PANIC_IF_FALSE(lwe_array_out != lwe_array_in, "Output and input pointers must be different for out-of-place operations");
  HX_PANIC_IF_FALSE(lwe_array_out && lwe_array_in && lwe_array_out->ptr && lwe_array_in->ptr, "negate: null pointer");
  HX_PANIC_IF_FALSE(lwe_array_out->num_radix_blocks >= num_radix_blocks && lwe_array_in->num_radix_blocks >= num_radix_blocks,
                    "lwe_array_in and lwe_array_out num radix blocks must be greater or equal to the number of blocks to negate");
  HX_PANIC_IF_FALSE(lwe_array_out->lwe_dimension == lwe_array_in->lwe_dimension,
                    "lwe_array_in and lwe_array_out lwe_dimension must be the same");
  HX_PANIC_IF_FALSE(message_modulus >= 2 && carry_modulus >= 1, "negate: bad moduli");
  if (num_radix_blocks == 0) return;
  const uint64_t delta = ((uint64_t)1 << 63) / ((uint64_t)message_modulus * carry_modulus);
  const uint64_t z = ((2ull * message_modulus - 1) / message_modulus) * message_modulus;
  HX_LAUNCH(lwe_negate_const_kernel, dim3(num_radix_blocks), dim3(256), 0, S0(streams), (uint64_t *)lwe_array_out->ptr,
            (const uint64_t *)lwe_array_in->ptr, lwe_array_in->lwe_dimension + 1, num_radix_blocks, num_radix_blocks,
            z * delta, (z - z / message_modulus) * delta);
  uint64_t zb = 0;
  for (uint32_t i = 0; i < lwe_array_out->num_radix_blocks; ++i) {
    const uint64_t d = (lwe_array_in->degrees ? lwe_array_in->degrees[i] : message_modulus - 1) + zb;
    const uint64_t zz = std::max<uint64_t>(1, d / message_modulus) * message_modulus;
    if (lwe_array_out->degrees) lwe_array_out->degrees[i] = zz - zb;
    if (lwe_array_out->noise_levels && lwe_array_in->noise_levels) lwe_array_out->noise_levels[i] = lwe_array_in->noise_levels[i];
    zb = zz / message_modulus;
  }
}

// scalar_addition.cuh:27-55: scalar_input (device) and h_scalar_input (host) hold the same num_scalars clear blocks
void cuda_scalar_addition_ciphertext_64_inplace(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
                                                void const *scalar_input, void const *h_scalar_input,
                                                uint32_t num_scalars, uint32_t message_modulus, uint32_t carry_modulus) {
  first_gpu(streams);
  HX_PANIC_IF_FALSE(lwe_array && lwe_array->ptr && (num_scalars == 0 || (scalar_input && h_scalar_input)),
                    "scalar_addition: null pointer");
  HX_PANIC_IF_FALSE(lwe_array->num_radix_blocks >= num_scalars,
                    "num scalars should be smaller or equal to input num radix blocks");
  if (num_scalars == 0) return;
  const uint64_t delta = ((uint64_t)1 << 63) / ((uint64_t)message_modulus * carry_modulus);
  HX_LAUNCH(lwe_body_add_scalars_kernel, dim3((num_scalars + 255) / 256), dim3(256), 0, S0(streams),
            (uint64_t *)lwe_array->ptr, (const uint64_t *)scalar_input, lwe_array->lwe_dimension + 1, num_scalars, delta);
  if (lwe_array->degrees)
    for (uint32_t i = 0; i < num_scalars; ++i) lwe_array->degrees[i] += ((const uint64_t *)h_scalar_input)[i];
}

// bitwise_ops.cuh:164-191 (host_bitnot): (ct_message_modulus - 1) - block, as a plain negation plus a constant
void cuda_bitnot_ciphertext_64(CudaStreamsFFI streams, CudaRadixCiphertextFFI *radix_ciphertext,
                               uint32_t ct_message_modulus, uint32_t param_message_modulus,
                               uint32_t param_carry_modulus) {
  first_gpu(streams);
  HX_PANIC_IF_FALSE(radix_ciphertext && radix_ciphertext->ptr, "bitnot: null pointer");
  HX_PANIC_IF_FALSE(ct_message_modulus >= 1 && param_message_modulus >= 2 && param_carry_modulus >= 1, "bitnot: bad moduli");
  const uint32_t nb = radix_ciphertext->num_radix_blocks;
  if (nb == 0) return;
  const uint64_t delta = (uint64_t)1 << (63 - __builtin_ctzll((uint64_t)param_message_modulus * param_carry_modulus));
  const uint64_t enc = delta * (ct_message_modulus - 1);
  HX_LAUNCH(lwe_negate_const_kernel, dim3(nb), dim3(256), 0, S0(streams), (uint64_t *)radix_ciphertext->ptr,
            (const uint64_t *)radix_ciphertext->ptr, radix_ciphertext->lwe_dimension + 1, nb, nb, enc, enc);
  if (radix_ciphertext->degrees)
    for (uint32_t i = 0; i < nb; ++i) radix_ciphertext->degrees[i] = ct_message_modulus - 1;
}

// ---- cuda/include/integer/integer.h:318-347 -----------------------------------------------------
static uint64_t scratch_bitop(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                              CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t count, uint32_t message_modulus,
                              uint32_t carry_modulus, uint32_t op, bool scalar, bool allocate_gpu_memory,
                              uint32_t noise_reduction_type) {
  return scratch_create<BitopMem>(streams, mem_ptr, allocate_gpu_memory, "bitop", [&](BitopMem &m) {
    HX_PANIC_IF_FALSE(scalar ? (op >= SCALAR_BITAND && op <= SCALAR_BITXOR) : op <= BITXOR,
                      "bitop: operation %u does not belong to this entry point", op);
    const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, noise_reduction_type);
    m.op = op;
    const size_t lw = (size_t)(p.k + 1) * p.N;
    const uint32_t cap = std::max<uint32_t>(1, count) * g_scratch_batch;
    std::vector<std::vector<uint64_t>> luts(scalar ? p.msg : 1, std::vector<uint64_t>(lw));
    if (scalar) {
      for (uint32_t c = 0; c < p.msg; ++c)
        generate_lut(p, luts[c].data(), [op, c](uint64_t x) { return bitop_apply(op, x, c); });
    } else {
      const uint32_t msg = p.msg;
      generate_lut(p, luts[0].data(), [op, msg](uint64_t x) { return bitop_apply(op, x / msg, x % msg); });
    }
    m.drv.init(streams, p, cap, luts);
    if (!scalar) {
      m.own.alloc(m.d_pack, (size_t)cap * (p.big_n + 1) * sizeof(uint64_t));
      m.own.alloc(m.d_lut_idx, (size_t)cap * sizeof(uint64_t));
      if (!t_dry) HX_CHECK(hipMemsetAsync(m.d_lut_idx, 0, (size_t)cap * sizeof(uint64_t), S0(streams)));
    }
  });
}
uint64_t scratch_cuda_integer_bitop_inplace_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                     CudaLweBootstrapKeyParamsFFI bsk_params,
                                                     CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                     uint32_t lwe_ciphertext_count, uint32_t message_modulus,
                                                     uint32_t carry_modulus, enum BITOP_TYPE op_type,
                                                     bool allocate_gpu_memory,
                                                     enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_bitop(streams, mem_ptr, bsk_params, ksk_params, lwe_ciphertext_count, message_modulus, carry_modulus,
                       (uint32_t)op_type, false, allocate_gpu_memory, (uint32_t)noise_reduction_type);
}
uint64_t scratch_cuda_integer_scalar_bitop_inplace_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                            CudaLweBootstrapKeyParamsFFI bsk_params,
                                                            CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                            uint32_t lwe_ciphertext_count, uint32_t message_modulus,
                                                            uint32_t carry_modulus, enum BITOP_TYPE op_type,
                                                            bool allocate_gpu_memory,
                                                            enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_bitop(streams, mem_ptr, bsk_params, ksk_params, lwe_ciphertext_count, message_modulus, carry_modulus,
                       (uint32_t)op_type, true, allocate_gpu_memory, (uint32_t)noise_reduction_type);
}

// bitwise_ops.cuh:230-271 (host_bitop): one bivariate round over all blocks
void cuda_integer_bitop_inplace_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_inout,
                                         CudaRadixCiphertextFFI const *lwe_array_2, int8_t *mem_ptr,
                                         void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<BitopMem>(mem_ptr, "integer_bitop");
  HX_PANIC_IF_FALSE(m->op <= BITXOR, "integer_bitop: foreign scratch pointer");  // a scratch of the scalar form
  HX_PANIC_IF_FALSE(lwe_array_inout && lwe_array_2 && lwe_array_inout->ptr && lwe_array_2->ptr && bsks && ksks,
                    "integer_bitop: null pointer");
  HX_PANIC_IF_FALSE(lwe_array_inout->num_radix_blocks == lwe_array_2->num_radix_blocks,
                    "input and output num radix blocks must be equal");
  HX_PANIC_IF_FALSE(lwe_array_inout->lwe_dimension == lwe_array_2->lwe_dimension,
                    "input and output lwe dimension must be equal");
  const uint32_t nb = lwe_array_inout->num_radix_blocks;
  HX_PANIC_IF_FALSE(nb <= m->drv.cap, "integer_bitop: %u blocks exceed the scratch capacity %u", nb, m->drv.cap);
  const Params &p = m->drv.p;
  if (lwe_array_inout->degrees && lwe_array_2->degrees)
    for (uint32_t i = 0; i < nb; ++i)
      HX_PANIC_IF_FALSE(lwe_array_inout->degrees[i] < p.msg && lwe_array_2->degrees[i] < p.msg,
                        "integer_bitop: block %u carries a degree of %llu / %llu, the packed pair needs clean blocks", i,
                        (unsigned long long)lwe_array_inout->degrees[i], (unsigned long long)lwe_array_2->degrees[i]);
  uint64_t *v = (uint64_t *)lwe_array_inout->ptr;
  axpy(S0(streams), m->d_pack, nullptr, v, nullptr, p.msg, (const uint64_t *)lwe_array_2->ptr, nullptr, p.big_n + 1, nb);
  m->drv.round(streams, v, nullptr, m->d_pack, nullptr, m->d_lut_idx, nb, ksks, bsks);
  for (uint32_t i = 0; i < nb; ++i) {
    if (lwe_array_inout->degrees)
      lwe_array_inout->degrees[i] = bitop_degree(m->op, lwe_array_inout->degrees[i],
                                                 lwe_array_2->degrees ? lwe_array_2->degrees[i] : p.msg - 1);
    if (lwe_array_inout->noise_levels) lwe_array_inout->noise_levels[i] = 1;
  }
}

// scalar_bitops.cuh:6-66 (host_scalar_bitop): clear_blocks (device) index the per-value tables; the blocks past the
// clear ones are ANDed with zero / left as they are
void cuda_integer_scalar_bitop_inplace_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_inout,
                                                void const *clear_blocks, void const *h_clear_blocks,
                                                uint32_t num_clear_blocks, int8_t *mem_ptr, void *const *bsks,
                                                void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<BitopMem>(mem_ptr, "integer_scalar_bitop");
  HX_PANIC_IF_FALSE(m->op >= SCALAR_BITAND, "integer_scalar_bitop: foreign scratch pointer");  // of the ciphertext form
  HX_PANIC_IF_FALSE(lwe_array_inout && lwe_array_inout->ptr && bsks && ksks, "integer_scalar_bitop: null pointer");
  const uint32_t nb = lwe_array_inout->num_radix_blocks;
  HX_PANIC_IF_FALSE(num_clear_blocks <= nb && num_clear_blocks <= m->drv.cap,
                    "integer_scalar_bitop: %u clear blocks for %u radix blocks (scratch capacity %u)", num_clear_blocks, nb,
                    m->drv.cap);
  HX_PANIC_IF_FALSE(num_clear_blocks == 0 || (clear_blocks && h_clear_blocks), "integer_scalar_bitop: null clear blocks");
  const Params &p = m->drv.p;
  const size_t w = (size_t)p.big_n + 1;
  uint64_t *v = (uint64_t *)lwe_array_inout->ptr;
  const uint64_t *hc = (const uint64_t *)h_clear_blocks;
  if (num_clear_blocks) {
    for (uint32_t i = 0; i < num_clear_blocks; ++i)
      HX_PANIC_IF_FALSE(hc[i] < p.msg, "integer_scalar_bitop: clear block %u is %llu, not below the message modulus", i,
                        (unsigned long long)hc[i]);
    m->drv.round(streams, v, nullptr, v, nullptr, (const uint64_t *)clear_blocks, num_clear_blocks, ksks, bsks);
    for (uint32_t i = 0; i < num_clear_blocks; ++i) {
      if (lwe_array_inout->degrees) lwe_array_inout->degrees[i] = bitop_degree(m->op, hc[i], lwe_array_inout->degrees[i]);
      if (lwe_array_inout->noise_levels) lwe_array_inout->noise_levels[i] = 1;
    }
  }
  if (m->op == SCALAR_BITAND && num_clear_blocks < nb) {
    HX_CHECK(hipMemsetAsync(v + (size_t)num_clear_blocks * w, 0, (size_t)(nb - num_clear_blocks) * w * sizeof(uint64_t),
                            S0(streams)));
    set_block_info(lwe_array_inout, num_clear_blocks, nb - num_clear_blocks, 0, 0);
  }
}

void cleanup_cuda_integer_bitop_inplace_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<BitopMem>(streams, mem_ptr_void, "cleanup integer_bitop");
}
void cleanup_cuda_integer_scalar_bitop_inplace_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<BitopMem>(streams, mem_ptr_void, "cleanup integer_scalar_bitop");
}

// ---- cuda/include/integer/integer.h:559-573 -----------------------------------------------------
// lhs - rhs = lhs + (negation of rhs with its correcting term), then the addition's carry propagation.  Block 0 of the
// sum reaches 2 msg - 1 (msg - b0 on top of a clean block): exactly what block 0 takes with an input carry, so an input
// carry on top of it is refused, and so is FLAG_OVERFLOW (the reference's callers — integer/gpu/server_key/radix/sub.rs:
// 222, :347-400 — pass neither).
uint64_t scratch_cuda_sub_and_propagate_single_carry_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
    uint32_t requested_flag, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_create<SubMem>(streams, mem_ptr, allocate_gpu_memory, "sub_and_propagate_single_carry", [&](SubMem &m) {
    HX_PANIC_IF_FALSE(requested_flag == 0 || requested_flag == 2,
                      "sub_and_propagate_single_carry: output flag %u is not wired (0 = none, 2 = carry)", requested_flag);
    const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
    m.prop.init(streams, p, num_blocks, g_scratch_batch);
    m.own.alloc(m.d_neg, (size_t)num_blocks * g_scratch_batch * (p.big_n + 1) * sizeof(uint64_t));
  });
}

void cuda_sub_and_propagate_single_carry_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lhs_array,
                                                          const CudaRadixCiphertextFFI *rhs_array,
                                                          CudaRadixCiphertextFFI *carry_out,
                                                          const CudaRadixCiphertextFFI *carry_in, int8_t *mem_ptr,
                                                          void *const *bsks, void *const *ksks,
                                                          uint32_t requested_flag, uint32_t uses_carry) {
  first_gpu(streams);
  (void)carry_in;
  auto *m = scratch_use<SubMem>(mem_ptr, "sub_and_propagate_single_carry");
  HX_PANIC_IF_FALSE(requested_flag == 0 || requested_flag == 2,
                    "sub_and_propagate_single_carry: output flag %u is not wired (0 = none, 2 = carry)", requested_flag);
  HX_PANIC_IF_FALSE(uses_carry == 0, "sub_and_propagate_single_carry: an input carry is not wired (block 0 already holds the "
                                     "borrowed unit of the negation)");
  HX_PANIC_IF_FALSE(lhs_array && rhs_array && lhs_array->ptr && rhs_array->ptr && bsks && ksks &&
                        lhs_array->num_radix_blocks == rhs_array->num_radix_blocks &&
                        lhs_array->lwe_dimension == rhs_array->lwe_dimension,
                    "sub_and_propagate_single_carry: operands must have the same shape");
  const uint32_t L = m->prop.blocks, cts = batch_of(lhs_array, L, "sub_and_propagate_single_carry");
  const Params &p = m->prop.drv.p;
  check_clean({lhs_array, rhs_array}, lhs_array->num_radix_blocks, p.msg, "sub_and_propagate_single_carry",
              "the subtraction takes clean operands (propagate them first)");
  uint64_t *cout = nullptr;
  if (requested_flag == 2)
    cout = carry_blocks(carry_out, cts, lhs_array, "sub_and_propagate_single_carry: FLAG_CARRY needs one output carry block per integer");
  const hipStream_t st = S0(streams);
  const uint32_t w = p.big_n + 1, T = cts * L;
  HX_LAUNCH(lwe_negate_const_kernel, dim3(T), dim3(256), 0, st, m->d_neg, (const uint64_t *)rhs_array->ptr, w, T, L,
            (uint64_t)p.msg * p.delta(), (uint64_t)(p.msg - 1) * p.delta());
  uint64_t *v = (uint64_t *)lhs_array->ptr;
  axpy(st, v, nullptr, v, nullptr, 1, m->d_neg, nullptr, w, T);
  m->prop.run(streams, v, cts, ksks, bsks, nullptr, cout);
  if (cout) set_block_info(carry_out, 0, cts, 1, 1);
  set_block_info(lhs_array, 0, lhs_array->num_radix_blocks, p.msg - 1, 1);
}

void cleanup_cuda_sub_and_propagate_single_carry_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<SubMem>(streams, mem_ptr_void, "cleanup sub_and_propagate_single_carry");
}

// ---- cuda/include/integer/integer.h:415-431 -----------------------------------------------------
// lhs -= rhs with the borrow: the subtraction above with FLAG_CARRY; the carry of lhs + (2^bits - rhs) is 1 exactly when
// nothing was borrowed, so the overflow block is 1 - carry (levelled).  An input borrow is not wired (the reference's unsigned
// overflowing_sub passes none: integer/gpu/server_key/radix/sub.rs unsigned_overflowing_sub).
uint64_t scratch_cuda_integer_overflowing_sub_64_inplace_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                               CudaLweBootstrapKeyParamsFFI bsk_params,
                                                               CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
                                                               uint32_t message_modulus, uint32_t carry_modulus,
                                                               uint32_t compute_overflow, bool allocate_gpu_memory,
                                                               enum PBS_MS_REDUCTION_T noise_reduction_type) {
  (void)compute_overflow;
  return scratch_cuda_sub_and_propagate_single_carry_64_inplace_async(streams, mem_ptr, bsk_params, ksk_params, num_blocks,
                                                                      message_modulus, carry_modulus, 2, allocate_gpu_memory,
                                                                      noise_reduction_type);
}
void cuda_integer_overflowing_sub_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lhs_array,
                                                   const CudaRadixCiphertextFFI *rhs_array,
                                                   CudaRadixCiphertextFFI *overflow_block,
                                                   const CudaRadixCiphertextFFI *input_borrow, int8_t *mem_ptr,
                                                   void *const *bsks, void *const *ksks, uint32_t compute_overflow,
                                                   uint32_t uses_input_borrow) {
  first_gpu(streams);
  HX_PANIC_IF_FALSE(uses_input_borrow == 0, "integer_overflowing_sub: an input borrow is not wired");
  if (compute_overflow == 0) {
    cuda_sub_and_propagate_single_carry_64_inplace_async(streams, lhs_array, rhs_array, overflow_block, input_borrow, mem_ptr, bsks,
                                                         ksks, 0, 0);
    return;
  }
  HX_PANIC_IF_FALSE(overflow_block && overflow_block->ptr && lhs_array, "integer_overflowing_sub: the overflow block is missing");
  cuda_sub_and_propagate_single_carry_64_inplace_async(streams, lhs_array, rhs_array, overflow_block, input_borrow, mem_ptr, bsks,
                                                       ksks, 2, 0);
  auto *m = scratch_use<SubMem>(mem_ptr, "integer_overflowing_sub");
  const Params &p = m->prop.drv.p;
  const uint32_t cts = lhs_array->num_radix_blocks / m->prop.blocks;
  HX_LAUNCH(lwe_negate_const_kernel, dim3(cts), dim3(256), 0, S0(streams), (uint64_t *)overflow_block->ptr,
            (const uint64_t *)overflow_block->ptr, p.big_n + 1, cts, 1, p.delta(), p.delta());  // 1 - carry
}
void cleanup_cuda_integer_overflowing_sub_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  cleanup_cuda_sub_and_propagate_single_carry_64_inplace(streams, mem_ptr_void);
}

// ---- cuda/include/integer/integer.h:159-171 -----------------------------------------------------
uint64_t scratch_cuda_full_propagation_64_inplace_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                        CudaLweBootstrapKeyParamsFFI bsk_params,
                                                        CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                        uint32_t message_modulus, uint32_t carry_modulus,
                                                        bool allocate_gpu_memory,
                                                        enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_create<FullPropMem>(streams, mem_ptr, allocate_gpu_memory, "full_propagation", [&](FullPropMem &m) {
    const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
    std::vector<std::vector<uint64_t>> luts(2, std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    const uint32_t msg = p.msg;
    generate_lut(p, luts[0].data(), [msg](uint64_t x) { return x % msg; });
    generate_lut(p, luts[1].data(), [msg](uint64_t x) { return x / msg; });
    m.drv.init(streams, p, 2, luts);
    m.own.alloc(m.d_two, 2 * (size_t)(p.big_n + 1) * sizeof(uint64_t));
    m.d_lut_idx = m.own.upload(S0(streams), std::vector<uint64_t>{0, 1});
  });
}

void cuda_full_propagation_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *input_blocks,
                                            int8_t *mem_ptr, void *const *ksks, void *const *bsks,
                                            uint32_t num_blocks) {
  first_gpu(streams);
  auto *m = scratch_use<FullPropMem>(mem_ptr, "full_propagation");
  HX_PANIC_IF_FALSE(input_blocks && input_blocks->ptr && ksks && bsks && num_blocks <= input_blocks->num_radix_blocks,
                    "full_propagation: null pointer or more blocks than the ciphertext holds");
  const Params &p = m->drv.p;
  const hipStream_t st = S0(streams);
  const size_t w = (size_t)p.big_n + 1;
  uint64_t *v = (uint64_t *)input_blocks->ptr;
  for (uint32_t i = 0; i < num_blocks; ++i) {
    uint64_t *blk = v + (size_t)i * w;
    HX_CHECK(hipMemcpyAsync(m->d_two, blk, w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    HX_CHECK(hipMemcpyAsync(m->d_two + w, blk, w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    m->drv.round(streams, m->d_two, nullptr, m->d_two, nullptr, m->d_lut_idx, 2, ksks, bsks);
    HX_CHECK(hipMemcpyAsync(blk, m->d_two, w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    set_block_info(input_blocks, i, 1, p.msg - 1, 1);
    if (i + 1 < num_blocks) {
      axpy(st, blk + w, nullptr, blk + w, nullptr, 1, m->d_two + w, nullptr, (uint32_t)w, 1);
      if (input_blocks->degrees) input_blocks->degrees[i + 1] += p.carry - 1;
      if (input_blocks->noise_levels) input_blocks->noise_levels[i + 1] += 1;
    }
  }
}

void cleanup_cuda_full_propagation_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<FullPropMem>(streams, mem_ptr_void, "cleanup full_propagation");
}

// ---- cuda/include/integer/integer.h:246-276 (comparison), :349-365 (cmux) ----------------------------
// Unsigned operands; the boolean lands in block 0 of lwe_array_out (its other blocks are cleared), as the single-block
// result of the reference's EQ ... LE.  MAX / MIN: the ordering's flag drives a cmux of the operands.
namespace {
struct CompareScratch : ScratchHeader {
  static constexpr uint32_t kMagic = 0x43535231;  // "CSR1"
  uint32_t op = 0;
  CompareMem cmp;
  CmuxMem mux;  // MAX / MIN only
  uint64_t *d_flag = nullptr;
  DeviceBlocks own;

  bool select() const { return op == MAX || op == MIN; }
  // shared by the ciphertext and the scalar form (one integer per call: hip_integer_scratch_batch is not read)
  void init(const CudaStreamsFFI &streams, CudaLweBootstrapKeyParamsFFI bsk_params, CudaLweKeyswitchKeyParamsFFI ksk_params,
            uint32_t count, uint32_t message_modulus, uint32_t carry_modulus, uint32_t op_type, bool is_signed,
            uint32_t noise_reduction_type) {
    HX_PANIC_IF_FALSE(count >= 1, "integer_comparison: null pointer or no blocks");
    HX_PANIC_IF_FALSE(!is_signed, "integer_comparison: signed operands are not wired");
    HX_PANIC_IF_FALSE(op_type <= MIN, "integer_comparison: unknown operation %u", op_type);
    const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, noise_reduction_type);
    op = op_type;
    cmp.init(streams, p, count, select() ? (uint32_t)GE : op_type);
    if (select()) {
      mux.init(streams, p, count);
      own.alloc(d_flag, (size_t)(p.big_n + 1) * sizeof(uint64_t));
    }
  }
  void run(const CudaStreamsFFI &streams, CudaRadixCiphertextFFI *lwe_array_out, CudaRadixCiphertextFFI const *lwe_array_1,
           CudaRadixCiphertextFFI const *lwe_array_2, void *const *bsks, void *const *ksks) {
    HX_PANIC_IF_FALSE(lwe_array_out && lwe_array_1 && lwe_array_2 && lwe_array_out->ptr && lwe_array_1->ptr &&
                          lwe_array_2->ptr && bsks && ksks,
                      "integer_comparison: null pointer");
    const uint32_t L = cmp.blocks;
    HX_PANIC_IF_FALSE(lwe_array_1->num_radix_blocks == L && lwe_array_2->num_radix_blocks == L,
                      "integer_comparison: the operands must hold the %u blocks the scratch was made for", L);
    HX_PANIC_IF_FALSE(lwe_array_1->lwe_dimension == lwe_array_2->lwe_dimension &&
                          lwe_array_out->lwe_dimension == lwe_array_1->lwe_dimension,
                      "input and output lwe dimension must be equal");
    const Params &p = cmp.params();
    check_clean({lwe_array_1, lwe_array_2}, L, p.msg, "integer_comparison",
                "the comparison takes clean operands (propagate them first)");
    const size_t w = (size_t)p.big_n + 1;
    uint64_t *out = (uint64_t *)lwe_array_out->ptr;
    const uint64_t *a = (const uint64_t *)lwe_array_1->ptr, *b = (const uint64_t *)lwe_array_2->ptr;
    if (select()) {
      HX_PANIC_IF_FALSE(lwe_array_out->num_radix_blocks >= L, "integer_comparison: MAX / MIN need %u output blocks", L);
      cmp.run(streams, d_flag, a, b, ksks, bsks);  // a >= b
      mux.run(streams, out, d_flag, op == MAX ? a : b, op == MAX ? b : a, ksks, bsks);
      set_block_info(lwe_array_out, 0, L, p.msg - 1, 1);
      return;
    }
    HX_PANIC_IF_FALSE(lwe_array_out->num_radix_blocks >= 1, "integer_comparison: the output needs a block");
    cmp.run(streams, out, a, b, ksks, bsks);
    if (lwe_array_out->num_radix_blocks > 1)
      HX_CHECK(hipMemsetAsync(out + w, 0, (size_t)(lwe_array_out->num_radix_blocks - 1) * w * sizeof(uint64_t), S0(streams)));
    set_block_info(lwe_array_out, 0, 1, 1, 1);
    set_block_info(lwe_array_out, 1, lwe_array_out->num_radix_blocks - 1, 0, 0);
  }
  void release(const CudaStreamsFFI &s) {
    cmp.release(s);
    mux.release(s);
    own.release(S0(s));
  }
};
}  // namespace
uint64_t scratch_cuda_integer_comparison_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                  CudaLweBootstrapKeyParamsFFI bsk_params,
                                                  CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                  uint32_t lwe_ciphertext_count, uint32_t message_modulus,
                                                  uint32_t carry_modulus, enum COMPARISON_TYPE op_type, bool is_signed,
                                                  bool allocate_gpu_memory,
                                                  enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_create<CompareScratch>(streams, mem_ptr, allocate_gpu_memory, "integer_comparison", [&](CompareScratch &m) {
    m.init(streams, bsk_params, ksk_params, lwe_ciphertext_count, message_modulus, carry_modulus, (uint32_t)op_type,
           is_signed, (uint32_t)noise_reduction_type);
  });
}

void cuda_integer_comparison_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                                      CudaRadixCiphertextFFI const *lwe_array_1,
                                      CudaRadixCiphertextFFI const *lwe_array_2, int8_t *mem_ptr, void *const *bsks,
                                      void *const *ksks) {
  first_gpu(streams);
  scratch_use<CompareScratch>(mem_ptr, "integer_comparison")->run(streams, lwe_array_out, lwe_array_1, lwe_array_2, bsks, ksks);
}

void cleanup_cuda_integer_comparison_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<CompareScratch>(streams, mem_ptr_void, "cleanup integer_comparison");
}

// integer.h:254-274: the scalar comes as its clear blocks (one per radix block, least significant first, the caller stops at
// the last non-zero one: integer/gpu/server_key/radix/scalar_comparison.rs:129-157).  They become trivial ciphertexts (zero
// masks) in the scratch and take the ciphertext path: the same rounds, the same tables.
namespace {
struct ScalarCompareScratch : ScratchHeader {
  static constexpr uint32_t kMagic = 0x53435231;  // "SCR1"
  CompareScratch cmp;
  uint64_t *d_triv = nullptr;
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    cmp.release(s);
    own.release(S0(s));
  }
};
}  // namespace
uint64_t scratch_cuda_integer_scalar_comparison_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                         CudaLweBootstrapKeyParamsFFI bsk_params,
                                                         CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                         uint32_t lwe_ciphertext_count, uint32_t message_modulus,
                                                         uint32_t carry_modulus, enum COMPARISON_TYPE op_type, bool is_signed,
                                                         bool allocate_gpu_memory,
                                                         enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_create<ScalarCompareScratch>(
      streams, mem_ptr, allocate_gpu_memory, "integer_scalar_comparison", [&](ScalarCompareScratch &m) {
        m.cmp.init(streams, bsk_params, ksk_params, lwe_ciphertext_count, message_modulus, carry_modulus, (uint32_t)op_type,
                   is_signed, (uint32_t)noise_reduction_type);
        m.own.alloc(m.d_triv, (size_t)lwe_ciphertext_count * (m.cmp.cmp.params().big_n + 1) * sizeof(uint64_t));
      });
}

void cuda_integer_scalar_comparison_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                                             CudaRadixCiphertextFFI const *lwe_array_in, void const *scalar_blocks,
                                             void const *h_scalar_blocks, int8_t *mem_ptr, void *const *bsks,
                                             void *const *ksks, uint32_t num_scalar_blocks) {
  first_gpu(streams);
  auto *m = scratch_use<ScalarCompareScratch>(mem_ptr, "integer_scalar_comparison");
  const Params &p = m->cmp.cmp.params();
  const uint32_t L = m->cmp.cmp.blocks;
  HX_PANIC_IF_FALSE(lwe_array_in && lwe_array_in->ptr && (num_scalar_blocks == 0 || (scalar_blocks && h_scalar_blocks)),
                    "integer_scalar_comparison: null pointer");
  HX_PANIC_IF_FALSE(num_scalar_blocks <= L, "integer_scalar_comparison: %u scalar blocks for %u radix blocks (the caller "
                    "truncates the scalar to the ciphertext's length)", num_scalar_blocks, L);
  for (uint32_t i = 0; i < num_scalar_blocks; ++i)
    HX_PANIC_IF_FALSE(((const uint64_t *)h_scalar_blocks)[i] < p.msg, "integer_scalar_comparison: scalar block %u is %llu, not below "
                      "the message modulus", i, (unsigned long long)((const uint64_t *)h_scalar_blocks)[i]);
  const hipStream_t st = S0(streams);
  const uint32_t w = p.big_n + 1;
  HX_CHECK(hipMemsetAsync(m->d_triv, 0, (size_t)L * w * sizeof(uint64_t), st));
  if (num_scalar_blocks)
    HX_LAUNCH(lwe_body_add_scalars_kernel, dim3((num_scalar_blocks + 255) / 256), dim3(256), 0, st, m->d_triv,
              (const uint64_t *)scalar_blocks, w, num_scalar_blocks, p.delta());
  std::vector<uint64_t> deg(L, 0), noise(L, 0);
  for (uint32_t i = 0; i < num_scalar_blocks; ++i) deg[i] = ((const uint64_t *)h_scalar_blocks)[i];
  CudaRadixCiphertextFFI triv{m->d_triv, deg.data(), noise.data(), L, L, p.big_n};
  m->cmp.run(streams, lwe_array_out, lwe_array_in, &triv, bsks, ksks);
}

void cleanup_cuda_integer_scalar_comparison_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ScalarCompareScratch>(streams, mem_ptr_void, "cleanup integer_scalar_comparison");
}

uint64_t scratch_cuda_cmux_64_async(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                                    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t lwe_ciphertext_count,
                                    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
                                    enum PBS_MS_REDUCTION_T noise_reduction_type) {
  HX_PANIC_IF_FALSE(mem_ptr != nullptr && lwe_ciphertext_count >= 1, "cmux: null pointer or no blocks");
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  // (one integer per call: hip_integer_scratch_batch is not read)
  return scratch_create<CmuxMem>(streams, mem_ptr, allocate_gpu_memory, "cmux",
                                 [&](CmuxMem &m) { m.init(streams, p, lwe_ciphertext_count); });
}

void cuda_cmux_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                        CudaRadixCiphertextFFI const *lwe_condition, CudaRadixCiphertextFFI const *lwe_array_true,
                        CudaRadixCiphertextFFI const *lwe_array_false, int8_t *mem_ptr, void *const *bsks,
                        void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<CmuxMem>(mem_ptr, "cmux");
  HX_PANIC_IF_FALSE(lwe_array_out && lwe_condition && lwe_array_true && lwe_array_false && lwe_array_out->ptr &&
                        lwe_condition->ptr && lwe_array_true->ptr && lwe_array_false->ptr && bsks && ksks,
                    "cmux: null pointer");
  const uint32_t L = m->blocks;
  HX_PANIC_IF_FALSE(lwe_array_true->num_radix_blocks == L && lwe_array_false->num_radix_blocks == L &&
                        lwe_array_out->num_radix_blocks >= L && lwe_condition->num_radix_blocks >= 1,
                    "cmux: the branches must hold the %u blocks the scratch was made for, the condition one block", L);
  HX_PANIC_IF_FALSE(lwe_array_true->lwe_dimension == lwe_array_false->lwe_dimension &&
                        lwe_array_out->lwe_dimension == lwe_array_true->lwe_dimension &&
                        lwe_condition->lwe_dimension == lwe_array_true->lwe_dimension,
                    "input and output lwe dimension must be equal");
  const Params &p = m->drv.p;
  check_clean({lwe_array_true, lwe_array_false}, L, p.msg, "cmux", "the branches must be clean");
  if (lwe_condition->degrees)
    HX_PANIC_IF_FALSE(lwe_condition->degrees[0] <= 1, "cmux: the condition must be a boolean block (degree %llu)",
                      (unsigned long long)lwe_condition->degrees[0]);
  m->run(streams, (uint64_t *)lwe_array_out->ptr, (const uint64_t *)lwe_condition->ptr,
         (const uint64_t *)lwe_array_true->ptr, (const uint64_t *)lwe_array_false->ptr, ksks, bsks);
  set_block_info(lwe_array_out, 0, L, p.msg - 1, 1);
}

void cleanup_cuda_cmux_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<CmuxMem>(streams, mem_ptr_void, "cleanup cmux");
}

// ---- cuda/include/integer/integer.h:200-228 -------------------------------------------------------
uint64_t scratch_cuda_logical_scalar_shift_64_inplace_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                            CudaLweBootstrapKeyParamsFFI bsk_params,
                                                            CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
                                                            uint32_t message_modulus, uint32_t carry_modulus,
                                                            enum SHIFT_OR_ROTATE_TYPE shift_type, bool allocate_gpu_memory,
                                                            enum PBS_MS_REDUCTION_T noise_reduction_type) {
  HX_PANIC_IF_FALSE(mem_ptr != nullptr && num_blocks >= 1, "logical_scalar_shift: null pointer or no blocks");
  HX_PANIC_IF_FALSE(shift_type == LEFT_SHIFT || shift_type == RIGHT_SHIFT,
                    "logical_scalar_shift: shift type %u is a rotation (scalar_rotate is not wired)", (uint32_t)shift_type);
  HX_PANIC_IF_FALSE((message_modulus & (message_modulus - 1)) == 0, "logical_scalar_shift: the message modulus must be a power of two");
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<ScalarShiftMem>(streams, mem_ptr, allocate_gpu_memory, "logical_scalar_shift", [&](ScalarShiftMem &m) {
    m.blocks = num_blocks;
    m.bits = (uint32_t)__builtin_ctz(p.msg);
    m.left = shift_type == LEFT_SHIFT;
    const uint32_t msg = p.msg, bits = m.bits;
    const bool left = m.left != 0;
    std::vector<std::vector<uint64_t>> luts(std::max(1u, bits - 1), std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    for (uint32_t r = 1; r < bits; ++r) generate_lut(p, luts[r - 1].data(), shift_in_block(msg, bits, r, left));
    m.drv.init(streams, p, num_blocks, luts);
    m.own.alloc(m.d_pack, (size_t)num_blocks * (p.big_n + 1) * sizeof(uint64_t));
    std::vector<uint64_t> li((size_t)std::max(1u, bits - 1) * num_blocks);
    for (size_t i = 0; i < li.size(); ++i) li[i] = i / num_blocks;
    m.d_lut_idx = m.own.upload(S0(streams), li);
  });
}

void cuda_logical_scalar_shift_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array, uint32_t shift,
                                                int8_t *mem_ptr, void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<ScalarShiftMem>(mem_ptr, "logical_scalar_shift");
  HX_PANIC_IF_FALSE(lwe_array && lwe_array->ptr && bsks && ksks, "logical_scalar_shift: null pointer");
  const uint32_t L = m->blocks;
  HX_PANIC_IF_FALSE(lwe_array->num_radix_blocks >= L, "input does not have enough blocks");
  const Params &p = m->drv.p;
  check_clean({lwe_array}, L, p.msg, "logical_scalar_shift", "the shift takes clean blocks");
  if (shift == 0) return;
  const hipStream_t st = S0(streams);
  const uint32_t w = p.big_n + 1;
  uint64_t *v = (uint64_t *)lwe_array->ptr;
  auto clear = [&](uint32_t first, uint32_t count) {
    if (count == 0) return;
    HX_CHECK(hipMemsetAsync(v + (size_t)first * w, 0, (size_t)count * w * sizeof(uint64_t), st));
    set_block_info(lwe_array, first, count, 0, 0);
  };
  if ((uint64_t)shift >= (uint64_t)m->bits * L) {  // every bit leaves
    clear(0, L);
    return;
  }
  const uint32_t q = shift / m->bits, r = shift % m->bits, n = L - q;  // n blocks survive
  const size_t bw = (size_t)w * sizeof(uint64_t);
  if (r == 0) {
    HX_CHECK(hipMemcpyAsync(m->d_pack, v + (m->left ? 0 : (size_t)q * w), n * bw, hipMemcpyDeviceToDevice, st));
    HX_CHECK(hipMemcpyAsync(v + (m->left ? (size_t)q * w : 0), m->d_pack, n * bw, hipMemcpyDeviceToDevice, st));
    if (lwe_array->degrees) {
      std::vector<uint64_t> d(lwe_array->degrees + (m->left ? 0 : q), lwe_array->degrees + (m->left ? 0 : q) + n);
      std::copy(d.begin(), d.end(), lwe_array->degrees + (m->left ? q : 0));
    }
    if (lwe_array->noise_levels) {
      std::vector<uint64_t> d(lwe_array->noise_levels + (m->left ? 0 : q), lwe_array->noise_levels + (m->left ? 0 : q) + n);
      std::copy(d.begin(), d.end(), lwe_array->noise_levels + (m->left ? q : 0));
    }
    clear(m->left ? 0 : n, q);
    return;
  }
  const uint64_t *lut = m->d_lut_idx + (size_t)(r - 1) * L;
  if (m->left) {
    // surviving block j (j = 0 .. n - 1) lands at position j + q: msg * b[j] + b[j - 1]
    axpy(st, m->d_pack, nullptr, v, nullptr, p.msg, nullptr, nullptr, w, 1);
    if (n > 1) axpy(st, m->d_pack + w, nullptr, v + w, nullptr, p.msg, v, nullptr, w, n - 1);
    m->drv.round(streams, v + (size_t)q * w, nullptr, m->d_pack, nullptr, lut, n, ksks, bsks);
  } else {
    // position j (j = 0 .. n - 1) takes msg * b[j + q] + b[j + q + 1]
    if (n > 1) axpy(st, m->d_pack, nullptr, v + (size_t)q * w, nullptr, p.msg, v + (size_t)(q + 1) * w, nullptr, w, n - 1);
    axpy(st, m->d_pack + (size_t)(n - 1) * w, nullptr, v + (size_t)(L - 1) * w, nullptr, p.msg, nullptr, nullptr, w, 1);
    m->drv.round(streams, v, nullptr, m->d_pack, nullptr, lut, n, ksks, bsks);
  }
  set_block_info(lwe_array, m->left ? q : 0, n, p.msg - 1, 1);
  clear(m->left ? 0 : n, q);
}

void cleanup_cuda_logical_scalar_shift_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ScalarShiftMem>(streams, mem_ptr_void, "cleanup logical_scalar_shift");
}

// ---- integer.h:212-244, :367-381: arithmetic shift and rotation by a clear amount, shift / rotation by an encrypted one
// (hip_ names with the reference's parameter lists: the reference-named symbols stay link stubs).  A batch of integers
// per call, capacity from hip_integer_scratch_batch.
uint64_t hip_scratch_integer_arithmetic_scalar_shift_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
    enum SHIFT_OR_ROTATE_TYPE shift_type, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type) {
  HX_PANIC_IF_FALSE(shift_type == RIGHT_SHIFT, "arithmetic_scalar_shift: shift type %u is not a right shift (a left shift "
                    "is the logical one)", (uint32_t)shift_type);
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<ArithShiftMem>(streams, mem_ptr, allocate_gpu_memory, "arithmetic_scalar_shift",
                                       [&](ArithShiftMem &m) { m.init(streams, p, num_blocks, g_scratch_batch); });
}

// the checks the three launches share; returns the number of integers
static uint32_t shift_family_batch(uint32_t blocks, uint32_t max_cts, const Params &p, const CudaRadixCiphertextFFI *ct,
                                   void *const *bsks, void *const *ksks, const char *who) {
  HX_PANIC_IF_FALSE(ct && ct->ptr && bsks && ksks, "%s: null pointer", who);
  HX_PANIC_IF_FALSE(ct->lwe_dimension == p.big_n, "%s: the blocks' lwe dimension should be %u", who, p.big_n);
  const uint32_t cts = batch_of(ct, blocks, who);
  HX_PANIC_IF_FALSE(cts >= 1 && cts <= max_cts, "%s: %u integers exceed the scratch capacity %u", who, cts, max_cts);
  return cts;
}
// degrees and noise levels follow the blocks of a levelled move: block to[i] takes what block from[i] had
static void move_block_info(CudaRadixCiphertextFFI *ct, const std::vector<uint32_t> &from, const std::vector<uint32_t> &to) {
  for (uint64_t *arr : {ct->degrees, ct->noise_levels}) {
    if (!arr) continue;
    std::vector<uint64_t> old(arr, arr + ct->num_radix_blocks);
    for (size_t i = 0; i < from.size(); ++i) arr[to[i]] = old[from[i]];
  }
}

void hip_integer_arithmetic_scalar_shift_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
                                                          uint32_t shift, int8_t *mem_ptr, void *const *bsks,
                                                          void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<ArithShiftMem>(mem_ptr, "arithmetic_scalar_shift");
  const Params &p = m->drv.p;
  const uint32_t cts = shift_family_batch(m->blocks, m->max_cts, p, lwe_array, bsks, ksks, "arithmetic_scalar_shift");
  const uint32_t L = m->blocks, b = m->bits, w = p.big_n + 1;
  check_clean({lwe_array}, cts * L, p.msg, "arithmetic_scalar_shift", "the shift takes clean blocks");
  if (shift == 0) return;
  const hipStream_t st = S0(streams);
  uint64_t *v = (uint64_t *)lwe_array->ptr;
  const uint32_t q = (uint32_t)std::min<uint64_t>(shift / b, L), n = L - q, r = n ? shift % b : 0;  // n blocks survive
  const size_t bw = (size_t)w * sizeof(uint64_t);
  m->plan(st, shift, cts, n, r);
  std::vector<uint32_t> from, to;
  for (uint32_t c = 0; c < cts; ++c) {
    const uint64_t *vc = v + (size_t)c * L * w;
    uint64_t *pk = m->d_pack + (size_t)c * (L + 1) * w;
    if (b == 1) {
      HX_CHECK(hipMemcpyAsync(pk, vc, L * bw, hipMemcpyDeviceToDevice, st));
      for (uint32_t t = 0; t < L; ++t) from.push_back(c * L + std::min(t + q, L - 1)), to.push_back(c * L + t);
      continue;
    }
    if (r) {
      if (n > 1) axpy(st, pk, nullptr, vc + (size_t)q * w, nullptr, p.msg, vc + (size_t)(q + 1) * w, nullptr, w, n - 1);
      HX_CHECK(hipMemcpyAsync(pk + (size_t)(n - 1) * w, vc + (size_t)(L - 1) * w, bw, hipMemcpyDeviceToDevice, st));
    } else if (n) {
      HX_CHECK(hipMemcpyAsync(pk, vc + (size_t)q * w, n * bw, hipMemcpyDeviceToDevice, st));
      for (uint32_t t = 0; t < n; ++t) from.push_back(c * L + t + q), to.push_back(c * L + t);
    }
    if (q) HX_CHECK(hipMemcpyAsync(pk + (size_t)L * w, vc + (size_t)(L - 1) * w, bw, hipMemcpyDeviceToDevice, st));
  }
  if (b > 1 && !r)  // the surviving blocks move as they are
    for (uint32_t c = 0; c < cts && n; ++c)
      HX_CHECK(hipMemcpyAsync(v + (size_t)c * L * w, m->d_pack + (size_t)c * (L + 1) * w, n * bw, hipMemcpyDeviceToDevice, st));
  if (b > 1) m->drv.round(streams, v, m->i_out, m->d_pack, m->i_in, m->i_lut, m->round_rows, ksks, bsks);
  axpy(st, v, m->i_to, b > 1 ? v : m->d_pack, m->i_from, 1, nullptr, nullptr, w, m->fill_rows);
  move_block_info(lwe_array, from, to);
  if (b > 1)
    for (uint32_t c = 0; c < cts; ++c) {
      if (r) set_block_info(lwe_array, c * L, n, p.msg - 1, 1);
      set_block_info(lwe_array, c * L + n, q, p.msg - 1, 1);
    }
}

void hip_cleanup_integer_arithmetic_scalar_shift_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ArithShiftMem>(streams, mem_ptr_void, "cleanup arithmetic_scalar_shift");
}

uint64_t hip_scratch_integer_scalar_rotate_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
    enum SHIFT_OR_ROTATE_TYPE shift_type, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type) {
  HX_PANIC_IF_FALSE(shift_type == LEFT_ROTATE || shift_type == RIGHT_ROTATE,
                    "scalar_rotate: shift type %u is not a rotation", (uint32_t)shift_type);
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<ScalarRotateMem>(streams, mem_ptr, allocate_gpu_memory, "scalar_rotate", [&](ScalarRotateMem &m) {
    m.init(streams, p, num_blocks, g_scratch_batch, shift_type == LEFT_ROTATE);
  });
}

void hip_integer_scalar_rotate_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array, uint32_t n,
                                                int8_t *mem_ptr, void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<ScalarRotateMem>(mem_ptr, "scalar_rotate");
  const Params &p = m->drv.p;
  const uint32_t cts = shift_family_batch(m->blocks, m->max_cts, p, lwe_array, bsks, ksks, "scalar_rotate");
  const uint32_t L = m->blocks, b = m->bits, w = p.big_n + 1;
  check_clean({lwe_array}, cts * L, p.msg, "scalar_rotate", "the rotation takes clean blocks");
  const uint32_t amount = n % (b * L), q = amount / b, r = amount % b;
  if (amount == 0) return;
  const hipStream_t st = S0(streams);
  uint64_t *v = (uint64_t *)lwe_array->ptr;
  RotatePack a{};
  a.out = m->d_pack, a.x = v, a.words = w, a.rows = L, a.mode = kPickWrap;
  a.dir = m->left ? kTowardsHigher : kTowardsLower;
  if (r == 0) {  // whole blocks: block i + q (left) takes block i
    a.s0 = 0, a.s1 = 1, a.r = q;
    launch_rotate_pack(st, a, cts);
    HX_CHECK(hipMemcpyAsync(v, m->d_pack, (size_t)cts * L * w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    std::vector<uint32_t> from, to;
    for (uint32_t c = 0; c < cts; ++c)
      for (uint32_t i = 0; i < L; ++i) from.push_back(c * L + i), to.push_back(c * L + (m->left ? (i + q) % L : (i + L - q) % L));
    move_block_info(lwe_array, from, to);
    return;
  }
  // msg block + its lower (left) / upper (right) neighbour, wrapping; a one-block integer is its own neighbour
  a.s0 = p.msg, a.s1 = 1, a.r = 1 % L;
  launch_rotate_pack(st, a, cts);
  m->drv.round(streams, v, m->i_out + (size_t)q * m->max_cts * L, m->d_pack, nullptr, m->i_lut + (size_t)(r - 1) * m->max_cts * L,
               cts * L, ksks, bsks);
  set_block_info(lwe_array, 0, cts * L, p.msg - 1, 1);
}

void hip_cleanup_integer_scalar_rotate_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ScalarRotateMem>(streams, mem_ptr_void, "cleanup scalar_rotate");
}

uint64_t hip_scratch_integer_shift_and_rotate_64_inplace_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
    enum SHIFT_OR_ROTATE_TYPE shift_type, bool is_signed, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<ShiftRotateMem>(streams, mem_ptr, allocate_gpu_memory, "shift_and_rotate", [&](ShiftRotateMem &m) {
    m.init(streams, p, num_blocks, g_scratch_batch, (uint32_t)shift_type, is_signed);
  });
}

void hip_integer_shift_and_rotate_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
                                                   CudaRadixCiphertextFFI const *lwe_shift, int8_t *mem_ptr,
                                                   void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<ShiftRotateMem>(mem_ptr, "shift_and_rotate");
  const Params &p = m->drv.p;
  HX_PANIC_IF_FALSE(lwe_shift && lwe_shift->ptr, "shift_and_rotate: null pointer");
  const uint32_t cts = shift_family_batch(m->blocks, m->max_cts, p, lwe_array, bsks, ksks, "shift_and_rotate");
  HX_PANIC_IF_FALSE(lwe_array->num_radix_blocks == lwe_shift->num_radix_blocks,
                    "shift_and_rotate: the amount holds %u blocks, the value %u: they must be the same",
                    lwe_shift->num_radix_blocks, lwe_array->num_radix_blocks);
  HX_PANIC_IF_FALSE(lwe_array->lwe_dimension == lwe_shift->lwe_dimension,
                    "shift_and_rotate: the amount and the value must have the same lwe dimension");
  check_clean({lwe_array, lwe_shift}, cts * m->blocks, p.msg, "shift_and_rotate",
              "the value and the amount must be clean (propagate them first)");
  m->run(streams, (uint64_t *)lwe_array->ptr, (const uint64_t *)lwe_shift->ptr, cts, ksks, bsks);
  set_block_info(lwe_array, 0, cts * m->blocks, p.msg - 1, 1);
}

void hip_cleanup_integer_shift_and_rotate_64_inplace(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ShiftRotateMem>(streams, mem_ptr_void, "cleanup shift_and_rotate");
}

// bootstraps per integer of one call on this scratch
uint64_t hip_integer_shift_and_rotate_pbs_count(int8_t *mem_ptr) {
  return scratch_cast<ShiftRotateMem>(mem_ptr, "hip_integer_shift_and_rotate_pbs_count")->pbs_count();
}

// lwe_rotate_pack_kernel alone on caller-supplied rows (tests, tools/bench_shift_rotate.py): batch integers of `rows` rows of
// `words` words in x and out; pad / ctrl may be null (mode != 2 / no control row)
void hip_test_rotate_pack_async(void *stream, uint32_t gpu_index, void *out, void const *x, void const *pad,
                                void const *ctrl, uint64_t s0, uint64_t s1, uint32_t words, uint32_t rows, uint32_t batch,
                                uint32_t r, uint32_t dir, uint32_t mode, uint32_t pad_stride, uint32_t pad_row,
                                uint32_t ctrl_stride, uint32_t ctrl_row) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  HX_PANIC_IF_FALSE(batch >= 1 && rows >= 1, "hip_test_rotate_pack: empty launch");
  RotatePack a{(uint64_t *)out, (const uint64_t *)x, (const uint64_t *)pad, (const uint64_t *)ctrl, s0, s1, words, rows, r,
               dir, mode, pad_stride, pad_row, ctrl_stride, ctrl_row};
  launch_rotate_pack((hipStream_t)stream, a, batch);
}

// the same result for s0 = 1 composed from the primitives the layer had before the kernel, as the reference composes a barrel
// stage (tools/bench_shift_rotate.py times one against the other): a device copy of the rows, per integer the rotation as
// block copies and a memset or single-row copies for the rows pulled in, one axpy that packs, one axpy that adds the
// control row to all.  tmp: 2 batch rows rows of scratch; ctrl_idx: batch rows entries c ctrl_stride + ctrl_row.
void hip_test_rotate_pack_baseline_async(void *stream, uint32_t gpu_index, void *out, void const *x, void const *pad,
                                         void const *ctrl, void const *ctrl_idx, void *tmp, uint64_t s1, uint32_t words,
                                         uint32_t rows, uint32_t batch, uint32_t r, uint32_t dir, uint32_t mode,
                                         uint32_t pad_stride, uint32_t pad_row) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  HX_PANIC_IF_FALSE(batch >= 1 && rows >= 1 && r < rows && dir <= kTowardsLower && mode <= kPickRow,
                    "hip_test_rotate_pack_baseline: empty launch or unknown form");
  const hipStream_t st = (hipStream_t)stream;
  const size_t bw = (size_t)words * sizeof(uint64_t), R = rows;
  uint64_t *copy = (uint64_t *)tmp, *rot = copy + (size_t)batch * R * words;
  HX_CHECK(hipMemcpyAsync(copy, x, batch * R * bw, hipMemcpyDeviceToDevice, st));
  for (uint32_t c = 0; c < batch; ++c) {
    const uint64_t *src = copy + (size_t)c * R * words;
    uint64_t *dst = rot + (size_t)c * R * words;
    // rows that stay inside the integer, then the r rows that wrap or are pulled in
    const uint32_t in = rows - r, first_in = dir == kTowardsHigher ? r : 0, first_out = dir == kTowardsHigher ? 0 : in;
    HX_CHECK(hipMemcpyAsync(dst + (size_t)first_in * words, src + (size_t)(dir == kTowardsHigher ? 0 : r) * words, in * bw,
                            hipMemcpyDeviceToDevice, st));
    if (r == 0) continue;
    if (mode == kPickWrap)
      HX_CHECK(hipMemcpyAsync(dst + (size_t)first_out * words, src + (size_t)(dir == kTowardsHigher ? in : 0) * words, r * bw,
                              hipMemcpyDeviceToDevice, st));
    else if (mode == kPickZero)
      HX_CHECK(hipMemsetAsync(dst + (size_t)first_out * words, 0, r * bw, st));
    else
      for (uint32_t t = 0; t < r; ++t)
        HX_CHECK(hipMemcpyAsync(dst + (size_t)(first_out + t) * words,
                                (const uint64_t *)pad + ((size_t)c * pad_stride + pad_row) * words, bw,
                                hipMemcpyDeviceToDevice, st));
  }
  axpy(st, (uint64_t *)out, nullptr, rot, nullptr, s1, (const uint64_t *)x, nullptr, words, batch * rows);
  if (ctrl)
    axpy(st, (uint64_t *)out, nullptr, (const uint64_t *)out, nullptr, 1, (const uint64_t *)ctrl, (const uint64_t *)ctrl_idx,
         words, batch * rows);
}

// ---- Trivium transciphering (radix_trivium.h; hip_ names with the parameter lists of cuda/include/trivium/trivium.h: the
// reference-named symbols stay link stubs) ------------------------------------------------------------------------------
namespace {
uint64_t trivium_scratch(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                         CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus, uint32_t carry_modulus,
                         bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t num_inputs,
                         bool warmup) {
  const char *who = warmup ? "trivium_init" : "trivium_step";
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<TriviumMem>(streams, mem_ptr, allocate_gpu_memory, who,
                                    [&](TriviumMem &m) { m.init(streams, p, num_inputs, warmup, who); });
}
// a register, the key, the IV or the keystream: `bits` positions of N rows, every block a clean bit
uint64_t *trivium_rows(const CudaRadixCiphertextFFI *ct, uint32_t bits, const TriviumMem &m, bool is_input, const char *who,
                       const char *what) {
  HX_PANIC_IF_FALSE(ct && ct->ptr, "%s: null pointer (%s)", who, what);
  HX_PANIC_IF_FALSE(ct->lwe_dimension == m.drv.p.big_n, "%s: the blocks' lwe dimension should be %u", who, m.drv.p.big_n);
  HX_PANIC_IF_FALSE(ct->num_radix_blocks == bits * m.inputs, "%s: %s holds %u blocks, %u bits of %u inputs are %u", who, what,
                    ct->num_radix_blocks, bits, m.inputs, bits * m.inputs);
  for (uint32_t i = 0; is_input && i < ct->num_radix_blocks; ++i) {
    HX_PANIC_IF_FALSE(!ct->degrees || ct->degrees[i] <= 1, "%s: block %u of %s has degree %llu, a bit has at most 1", who, i,
                      what, (unsigned long long)ct->degrees[i]);
    HX_PANIC_IF_FALSE(!ct->noise_levels || ct->noise_levels[i] <= 1, "%s: block %u of %s has noise level %llu, at most 1",
                      who, i, what, (unsigned long long)ct->noise_levels[i]);
  }
  return (uint64_t *)ct->ptr;
}
TriviumMem *trivium_use(int8_t *mem_ptr, bool warmup, uint32_t num_inputs, void *const *bsks, void *const *ksks,
                        const char *who) {
  auto *m = scratch_use<TriviumMem>(mem_ptr, who);
  HX_PANIC_IF_FALSE(m->warmup == warmup, "%s: the scratch was created by the other trivium scratch call", who);
  HX_PANIC_IF_FALSE(bsks && ksks, "%s: null pointer", who);
  HX_PANIC_IF_FALSE(num_inputs == m->inputs, "%s: %u inputs on a scratch created for %u", who, num_inputs, m->inputs);
  return m;
}
}  // namespace

uint64_t hip_scratch_trivium_init_async(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                                        CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
                                        uint32_t carry_modulus, bool allocate_gpu_memory,
                                        enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t num_inputs) {
  return trivium_scratch(streams, mem_ptr, bsk_params, ksk_params, message_modulus, carry_modulus, allocate_gpu_memory,
                         noise_reduction_type, num_inputs, true);
}

void hip_trivium_init_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *a_reg, CudaRadixCiphertextFFI *b_reg,
                            CudaRadixCiphertextFFI *c_reg, const CudaRadixCiphertextFFI *key,
                            const CudaRadixCiphertextFFI *iv, uint32_t num_inputs, int8_t *mem_ptr, void *const *bsks,
                            void *const *ksks) {
  first_gpu(streams);
  const char *who = "trivium_init";
  TriviumMem *m = trivium_use(mem_ptr, true, num_inputs, bsks, ksks, who);
  CudaRadixCiphertextFFI *const regs[3] = {a_reg, b_reg, c_reg};
  const char *const names[3] = {"register a", "register b", "register c"};
  uint64_t *rows[3];
  for (uint32_t r = 0; r < 3; ++r) rows[r] = trivium_rows(regs[r], kTriviumBits[r], *m, false, who, names[r]);
  const uint64_t *k = trivium_rows(key, kTriviumKeyBits, *m, true, who, "the key");
  const uint64_t *v = trivium_rows(iv, kTriviumKeyBits, *m, true, who, "the iv");
  m->warm_up(streams, rows, k, v, ksks, bsks);
  for (uint32_t r = 0; r < 3; ++r) set_block_info(regs[r], 0, regs[r]->num_radix_blocks, 1, 1);
}

void hip_cleanup_trivium_init(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<TriviumMem>(streams, mem_ptr_void, "cleanup trivium_init");
}

uint64_t hip_scratch_trivium_step_async(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                                        CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
                                        uint32_t carry_modulus, bool allocate_gpu_memory,
                                        enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t num_inputs) {
  return trivium_scratch(streams, mem_ptr, bsk_params, ksk_params, message_modulus, carry_modulus, allocate_gpu_memory,
                         noise_reduction_type, num_inputs, false);
}

void hip_trivium_step_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *keystream_output, CudaRadixCiphertextFFI *a_reg,
                            CudaRadixCiphertextFFI *b_reg, CudaRadixCiphertextFFI *c_reg, uint32_t num_inputs,
                            uint32_t num_steps, int8_t *mem_ptr, void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  const char *who = "trivium_step";
  TriviumMem *m = trivium_use(mem_ptr, false, num_inputs, bsks, ksks, who);
  HX_PANIC_IF_FALSE(num_steps % kTriviumBatch == 0, "%s: num_steps %u is not a multiple of %u", who, num_steps, kTriviumBatch);
  CudaRadixCiphertextFFI *const regs[3] = {a_reg, b_reg, c_reg};
  const char *const names[3] = {"register a", "register b", "register c"};
  uint64_t *rows[3];
  for (uint32_t r = 0; r < 3; ++r) rows[r] = trivium_rows(regs[r], kTriviumBits[r], *m, true, who, names[r]);
  if (num_steps == 0) return;
  uint64_t *z = trivium_rows(keystream_output, num_steps, *m, false, who, "the keystream");
  m->step(streams, rows, z, num_steps, ksks, bsks);
  for (uint32_t r = 0; r < 3; ++r) set_block_info(regs[r], 0, regs[r]->num_radix_blocks, 1, 1);
  set_block_info(keystream_output, 0, keystream_output->num_radix_blocks, 1, 1);
}

void hip_cleanup_trivium_step(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<TriviumMem>(streams, mem_ptr_void, "cleanup trivium_step");
}

// bootstraps of one call on this scratch: the warm-up for a scratch of trivium_init (num_steps is not read), num_steps
// steps with keystream for a scratch of trivium_step
uint64_t hip_trivium_pbs_count(int8_t *mem_ptr, uint32_t num_steps) {
  return scratch_cast<TriviumMem>(mem_ptr, "hip_trivium_pbs_count")->pbs_count(num_steps);
}

// tests: batches between two re-basings of the tapes, 2 .. 18
void hip_test_trivium_set_window(int8_t *mem_ptr, uint32_t window) {
  auto *m = scratch_cast<TriviumMem>(mem_ptr, "hip_test_trivium_set_window");
  HX_PANIC_IF_FALSE(window >= 2 && window <= m->window_max, "hip_test_trivium_set_window: %u is outside 2 .. %u", window,
                    m->window_max);
  m->window = window;
}

// lwe_tap_sum_kernel alone on a caller-given table (tests, tools/bench_trivium.py).  Host arrays: outs / bits / terms hold
// one entry per group, srcs / pos / backwards / scalars 5 per group (term t of group g at 5 g + t); backwards: bit q reads
// position pos - q instead of pos + q
void hip_test_tap_sum_async(void *stream, uint32_t gpu_index, uint32_t words, uint32_t inputs, uint32_t groups,
                            void *const *outs, uint32_t const *bits, uint32_t const *terms, void const *const *srcs,
                            uint32_t const *pos, uint32_t const *backwards, uint64_t const *scalars) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  HX_PANIC_IF_FALSE(groups >= 1 && groups <= kTapGroups && outs && bits && terms && srcs && pos && backwards && scalars,
                    "hip_test_tap_sum: %u groups or a null array", groups);
  TapTable t{};
  t.words = words, t.inputs = inputs, t.groups = groups;
  for (uint32_t g = 0; g < groups; ++g) {
    HX_PANIC_IF_FALSE(terms[g] <= kTapTerms, "hip_test_tap_sum: group %u has %u terms", g, terms[g]);
    t.g[g].out = (uint64_t *)outs[g], t.g[g].bits = bits[g], t.g[g].terms = terms[g];
    for (uint32_t i = 0; i < terms[g]; ++i)
      t.g[g].t[i] = TapTerm{(const uint64_t *)srcs[kTapTerms * g + i], scalars[kTapTerms * g + i], pos[kTapTerms * g + i],
                            backwards[kTapTerms * g + i] ? -1 : 1};
  }
  launch_tap_sum((hipStream_t)stream, t);
}

// one batch's data movement composed from the older primitives in the reference's order (radix_trivium.h,
// trivium_batch_baseline): a, b, c are updated in place from r2, keystream receives r2's z rows in step order
void hip_test_trivium_batch_baseline_async(void *stream, uint32_t gpu_index, void *a, void *b, void *c, void *in1,
                                           void const *r1, void *in2, void const *r2, void *keystream, void *tmp,
                                           uint32_t words, uint32_t inputs, uint64_t message_modulus) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  HX_PANIC_IF_FALSE(a && b && c && in1 && r1 && in2 && r2 && keystream && tmp && words >= 1 && inputs >= 1,
                    "hip_test_trivium_batch_baseline: null pointer or empty rows");
  uint64_t *const regs[3] = {(uint64_t *)a, (uint64_t *)b, (uint64_t *)c};
  trivium_batch_baseline((hipStream_t)stream, regs, (uint64_t *)in1, (const uint64_t *)r1, (uint64_t *)in2,
                         (const uint64_t *)r2, (uint64_t *)keystream, (uint64_t *)tmp, words, inputs, message_modulus);
}

// ---- AES-128 transciphering (radix_aes.h; hip_ names with the parameter lists of cuda/include/aes/aes.h: the reference-named
// symbols stay link stubs).  key / iv: 128 one-bit blocks, block i holds bit 127 - i; round keys: 11 x 128 blocks in the same
// order; output: 128 blocks per input, input n is AES_k((iv + start_counter + n) mod 2^128);
// counter_bits_le_all_blocks[128 n + i]: bit i (little endian) of start_counter + n, a HOST array.
namespace {
uint64_t aes_scratch(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                     CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus, uint32_t carry_modulus,
                     bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t num_aes_inputs,
                     uint32_t sbox_parallelism, bool key_schedule) {
  const char *who = key_schedule ? "key_expansion" : "aes_ctr_encrypt";
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<AesMem>(streams, mem_ptr, allocate_gpu_memory, who,
                                [&](AesMem &m) { m.init(streams, p, num_aes_inputs, sbox_parallelism, key_schedule, who); });
}
// `blocks` one-bit blocks of the caller
uint64_t *aes_rows(const CudaRadixCiphertextFFI *ct, uint32_t blocks, const AesMem &m, bool is_input, const char *who,
                   const char *what) {
  HX_PANIC_IF_FALSE(ct && ct->ptr, "%s: null pointer (%s)", who, what);
  HX_PANIC_IF_FALSE(ct->lwe_dimension == m.drv.p.big_n, "%s: the blocks' lwe dimension should be %u", who, m.drv.p.big_n);
  HX_PANIC_IF_FALSE(ct->num_radix_blocks == blocks, "%s: %s: %u blocks, not %u", who, what, ct->num_radix_blocks, blocks);
  for (uint32_t i = 0; is_input && i < ct->num_radix_blocks; ++i) {
    HX_PANIC_IF_FALSE(!ct->degrees || ct->degrees[i] <= 1, "%s: block %u of %s has degree %llu, a bit has at most 1", who, i,
                      what, (unsigned long long)ct->degrees[i]);
    HX_PANIC_IF_FALSE(!ct->noise_levels || ct->noise_levels[i] <= 1, "%s: block %u of %s has noise level %llu, at most 1",
                      who, i, what, (unsigned long long)ct->noise_levels[i]);
  }
  return (uint64_t *)ct->ptr;
}
AesMem *aes_use(int8_t *mem_ptr, bool key_schedule, void *const *bsks, void *const *ksks, const char *who) {
  auto *m = scratch_use<AesMem>(mem_ptr, who);
  HX_PANIC_IF_FALSE(m->key_schedule == key_schedule, "%s: the scratch was created by the other aes scratch call", who);
  HX_PANIC_IF_FALSE(bsks && ksks, "%s: null pointer", who);
  return m;
}
}  // namespace

uint64_t hip_scratch_integer_aes_ctr_encrypt_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                      CudaLweBootstrapKeyParamsFFI bsk_params,
                                                      CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
                                                      uint32_t carry_modulus, bool allocate_gpu_memory,
                                                      enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t num_aes_inputs,
                                                      uint32_t sbox_parallelism) {
  return aes_scratch(streams, mem_ptr, bsk_params, ksk_params, message_modulus, carry_modulus, allocate_gpu_memory,
                     noise_reduction_type, num_aes_inputs, sbox_parallelism, false);
}

void hip_integer_aes_ctr_encrypt_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *output,
                                          CudaRadixCiphertextFFI const *iv, CudaRadixCiphertextFFI const *round_keys,
                                          const uint64_t *counter_bits_le_all_blocks, uint32_t num_aes_inputs, int8_t *mem_ptr,
                                          void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  const char *who = "aes_ctr_encrypt";
  AesMem *m = aes_use(mem_ptr, false, bsks, ksks, who);
  HX_PANIC_IF_FALSE(num_aes_inputs == m->inputs, "%s: %u inputs on a scratch created for %u", who, num_aes_inputs, m->inputs);
  HX_PANIC_IF_FALSE(counter_bits_le_all_blocks != nullptr, "%s: null pointer (the counter bits)", who);
  const uint64_t *v = aes_rows(iv, 128, *m, true, who, "the iv");
  const uint64_t *k = aes_rows(round_keys, 128 * (m->cipher_rounds + 1), *m, true, who, "the round keys");
  uint64_t *out = aes_rows(output, 128 * m->inputs, *m, false, who, "the output");
  for (size_t i = 0; i < (size_t)128 * m->inputs; ++i)
    HX_PANIC_IF_FALSE(counter_bits_le_all_blocks[i] <= 1, "%s: counter bit %zu is %llu", who, i,
                      (unsigned long long)counter_bits_le_all_blocks[i]);
  m->encrypt(streams, out, v, k, counter_bits_le_all_blocks, ksks, bsks);
  set_block_info(output, 0, output->num_radix_blocks, 1, 1);
}

void hip_cleanup_integer_aes_ctr_encrypt_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<AesMem>(streams, mem_ptr_void, "cleanup aes_ctr_encrypt");
}

uint64_t hip_scratch_integer_key_expansion_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                    CudaLweBootstrapKeyParamsFFI bsk_params,
                                                    CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
                                                    uint32_t carry_modulus, bool allocate_gpu_memory,
                                                    enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return aes_scratch(streams, mem_ptr, bsk_params, ksk_params, message_modulus, carry_modulus, allocate_gpu_memory,
                     noise_reduction_type, 1, 4, true);
}

void hip_integer_key_expansion_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *expanded_keys,
                                        CudaRadixCiphertextFFI const *key, int8_t *mem_ptr, void *const *bsks,
                                        void *const *ksks) {
  first_gpu(streams);
  const char *who = "key_expansion";
  AesMem *m = aes_use(mem_ptr, true, bsks, ksks, who);
  const uint64_t *k = aes_rows(key, 32 * m->key_words, *m, true, who, "the key");
  uint64_t *out = aes_rows(expanded_keys, 128 * (m->cipher_rounds + 1), *m, false, who, "the expanded keys");
  m->expand_key(streams, out, k, ksks, bsks);
  set_block_info(expanded_keys, 0, expanded_keys->num_radix_blocks, 1, 1);
}

void hip_cleanup_integer_key_expansion_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<AesMem>(streams, mem_ptr_void, "cleanup key_expansion");
}

// bootstraps and round-driver rounds of one call on this scratch (closed formulas over the scheduled program: DESIGN.md 6m);
// every call checks both against what it issued
uint64_t hip_integer_aes_pbs_count(int8_t *mem_ptr) { return scratch_cast<AesMem>(mem_ptr, "hip_integer_aes_pbs_count")->pbs_count(); }
uint64_t hip_integer_aes_rounds(int8_t *mem_ptr) { return scratch_cast<AesMem>(mem_ptr, "hip_integer_aes_rounds")->round_count(); }

// lwe_gate_sum_kernel alone on a caller-given program (tests, tools/bench_aes.py).  Device pointers: out, wires, caller_a,
// caller_b, clear (the last three may be null).  HOST arrays: group_constant / group_terms one entry per group (the terms of
// the groups follow each other), term_* one entry per term, maps 16 entries per permutation.
void hip_test_gate_sum_async(void *stream, uint32_t gpu_index, void *out, void const *wires, void const *caller_a,
                             void const *caller_b, void const *clear, uint32_t words, uint32_t inputs, uint32_t lanes,
                             uint32_t lane0, uint32_t state_lanes, uint32_t clear_stride, uint64_t delta, uint32_t groups,
                             uint64_t const *group_constant, uint32_t const *group_terms, uint64_t const *term_scalar,
                             uint32_t const *term_row0, uint32_t const *term_lane_stride, uint32_t const *term_map,
                             uint32_t const *term_base, uint32_t const *term_flags, uint32_t num_maps, uint32_t const *maps,
                             uint64_t rows_wires, uint64_t rows_a, uint64_t rows_b) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  const hipStream_t st = (hipStream_t)stream;
  HX_PANIC_IF_FALSE(groups == 0 || (group_constant && group_terms), "hip_test_gate_sum: null array");
  std::vector<GateGroup> hg;
  std::vector<GateTerm> ht;
  for (uint32_t g = 0; g < groups; ++g) {
    hg.push_back(GateGroup{group_constant[g], (uint32_t)ht.size(), group_terms[g]});
    for (uint32_t t = 0; t < group_terms[g]; ++t) {
      const size_t i = ht.size();
      HX_PANIC_IF_FALSE(term_scalar && term_row0 && term_lane_stride && term_map && term_base && term_flags && term_base[i] <= 3 &&
                            term_flags[i] <= 3,
                        "hip_test_gate_sum: null array, or base / flags of term %zu out of range", i);
      ht.push_back(GateTerm{term_scalar[i], term_row0[i], term_lane_stride[i], term_map[i], term_base[i] | term_flags[i] << 2});
    }
  }
  std::vector<uint32_t> hm(maps ? maps : nullptr, maps ? maps + (size_t)num_maps * kGateLanes : nullptr);
  GateGroup *dg = nullptr;
  GateTerm *dt = nullptr;
  uint32_t *dm = nullptr;
  DeviceBlocks own;
  if (!hg.empty()) dg = own.upload(st, hg);
  if (!ht.empty()) dt = own.upload(st, ht);
  if (!hm.empty()) dm = own.upload(st, hm);
  GateLaunch a{(uint64_t *)out, (const uint64_t *)wires, (const uint64_t *)caller_a, (const uint64_t *)caller_b,
               (const uint64_t *)clear, dg, dt, dm, delta, words, inputs, lanes, lane0, clear_stride, groups};
  GateHost h{hg.data(), ht.data(), hm.data(), num_maps, state_lanes,
             {(size_t)rows_wires, (size_t)rows_a, (size_t)rows_b}};
  launch_gate_sum(st, a, h);
  own.release(st);
}

// one S-box pass on the lanes of the scratch's first pass: rows [wire j][lane][input] (j = 0 the most significant bit),
// sbox_parallelism * num_aes_inputs rows per wire, in and out
void hip_test_aes_sbox_async(CudaStreamsFFI streams, void *out, void const *in, int8_t *mem_ptr, void *const *bsks,
                             void *const *ksks) {
  first_gpu(streams);
  const char *who = "hip_test_aes_sbox";
  AesMem *m = aes_use(mem_ptr, false, bsks, ksks, who);
  HX_PANIC_IF_FALSE(out && in, "%s: null pointer", who);
  m->move_wires(S0(streams), m->x_wire, (uint64_t *)in, m->parallelism, true);
  m->run(streams, m->segs[AesMem::kSbox], nullptr, 0, nullptr, 0, nullptr, ksks, bsks, 0, 1);
  m->move_wires(S0(streams), m->sb_wire, (uint64_t *)out, m->parallelism, false);
}

// parts of a call.  r0 = 0: the counter addition with round key 0 (iv, round_keys and the HOST counter bits as for the call)
// into the state; otherwise the state is loaded from `state`.  Then the cipher rounds max(r0, 1) .. r1 (none when r1 = 0).
// state: rows [wire j][byte lane][input], 16 * num_aes_inputs rows per wire; it receives the state after the last round run,
// unless that is the cipher's last round, which writes `output` (the caller's layout).
void hip_test_aes_rounds_async(CudaStreamsFFI streams, void *state, CudaRadixCiphertextFFI *output,
                               CudaRadixCiphertextFFI const *iv, CudaRadixCiphertextFFI const *round_keys,
                               const uint64_t *counter_bits_le_all_blocks, uint32_t r0, uint32_t r1, int8_t *mem_ptr,
                               void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  const char *who = "hip_test_aes_rounds";
  AesMem *m = aes_use(mem_ptr, false, bsks, ksks, who);
  HX_PANIC_IF_FALSE(state && r0 <= r1 && r1 <= m->cipher_rounds, "%s: null pointer, or rounds %u .. %u", who, r0, r1);
  const uint64_t *k = aes_rows(round_keys, 128 * (m->cipher_rounds + 1), *m, true, who, "the round keys");
  uint64_t *out = r1 == m->cipher_rounds ? aes_rows(output, 128 * m->inputs, *m, false, who, "the output") : nullptr;
  if (r0 == 0) {
    HX_PANIC_IF_FALSE(counter_bits_le_all_blocks != nullptr, "%s: null pointer (the counter bits)", who);
    m->counter_addition(streams, aes_rows(iv, 128, *m, true, who, "the iv"), k, counter_bits_le_all_blocks, ksks, bsks);
  } else {
    m->move_wires(S0(streams), m->x_wire, (uint64_t *)state, kGateLanes, true);
  }
  if (r1 >= 1) m->cipher(streams, std::max(r0, 1u), r1, k, out, ksks, bsks);
  if (out)
    set_block_info(output, 0, output->num_radix_blocks, 1, 1);
  else
    m->move_wires(S0(streams), m->x_wire, (uint64_t *)state, kGateLanes, false);
}

// The scheduled program of a scratch as u64 words in HOST memory; returns the words it takes and writes them when
// `capacity` holds them.  Format (every item one word):
//   header   magic "AESP", message modulus, carry modulus, inputs, sbox_parallelism, key_schedule (0 / 1), cipher rounds,
//            tables T, entries per table E = msg * carry, permutations M, segments G, rows of the wires,
//            first row of the state wires x[0 .. 7] (0 for a key schedule), first row of the S-box outputs sb[0 .. 7]
//   tables   T * E entries, then M * 16 permutation entries
//   segment  lanes, passes, rounds R; then per round: rows, to_caller (0 / 1); then per row: table, constant, terms,
//            destination (row0, lane_stride, in_stride, state_lane); then per term: base (0 wires, 1 caller a, 2 caller b,
//            3 clear), row0, lane_stride, map (kind | parameter << 2; kinds 0 identity, 1 permutation, 2 column offset),
//            flags (1 broadcast over inputs, 2 lane of the state), scalar
// Segments of a cipher scratch: counter addition, S-box, middle round's linear layer, last round's; of a key schedule: S-box,
// then the linear layer of steps 1 .. rounds.
uint64_t hip_test_aes_program(int8_t *mem_ptr, uint64_t *words, uint64_t capacity) {
  const AesMem *m = scratch_cast<AesMem>(mem_ptr, "hip_test_aes_program");
  std::vector<uint64_t> o;
  const Params &p = m->drv.p;
  const uint64_t E = (uint64_t)p.msg * p.carry;
  for (uint64_t x : {(uint64_t)0x41455350, (uint64_t)p.msg, (uint64_t)p.carry, (uint64_t)m->inputs, (uint64_t)m->parallelism,
                     (uint64_t)m->key_schedule, (uint64_t)m->cipher_rounds, (uint64_t)(m->h_tables.size() / E), E,
                     (uint64_t)(m->h_maps.size() / kGateLanes), (uint64_t)m->segs.size(), (uint64_t)m->sch.wire_rows})
    o.push_back(x);
  for (uint32_t j = 0; j < 8; ++j) o.push_back(m->key_schedule ? 0 : m->x_wire[j].row0);
  for (uint32_t j = 0; j < 8; ++j) o.push_back(m->sb_wire[j].row0);
  o.insert(o.end(), m->h_tables.begin(), m->h_tables.end());
  o.insert(o.end(), m->h_maps.begin(), m->h_maps.end());
  for (const GateSegment &sg : m->segs) {
    uint64_t rounds = 0;
    for (auto &r : sg.rounds) rounds += !r.empty();
    o.insert(o.end(), {(uint64_t)sg.lanes, (uint64_t)sg.passes, rounds});
    for (auto &r : sg.rounds) {
      if (r.empty()) continue;
      o.insert(o.end(), {(uint64_t)r.size(), (uint64_t)r[0].dst.caller});
      for (const GateRow &row : r) {
        o.insert(o.end(), {(uint64_t)row.table, row.constant, (uint64_t)row.terms.size(), (uint64_t)row.dst.row0,
                           (uint64_t)row.dst.lane_stride, (uint64_t)row.dst.in_stride, (uint64_t)row.dst.state_lane});
        for (const GateTerm &t : row.terms)
          o.insert(o.end(), {(uint64_t)(t.base_flags & 3), (uint64_t)t.row0, (uint64_t)t.lane_stride, (uint64_t)t.map,
                             (uint64_t)(t.base_flags >> 2), t.scalar});
      }
    }
  }
  if (words && capacity >= o.size()) std::copy(o.begin(), o.end(), words);
  return o.size();
}

// benches: the gate-sum launches of one middle cipher round of a cipher scratch (every S-box pass, then the linear layer with
// the round key read from `round_key`, 128 rows), without the bootstraps between them
void hip_test_aes_round_launches_async(CudaStreamsFFI streams, void const *round_key, int8_t *mem_ptr) {
  first_gpu(streams);
  auto *m = scratch_use<AesMem>(mem_ptr, "hip_test_aes_round_launches");
  HX_PANIC_IF_FALSE(!m->key_schedule && round_key, "hip_test_aes_round_launches: null pointer, or a key-schedule scratch");
  m->run(streams, m->segs[AesMem::kSbox], nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, ~0u, true);
  m->run(streams, m->segs[AesMem::kLin], (const uint64_t *)round_key, 128, nullptr, 0, nullptr, nullptr, nullptr, 0, ~0u, true);
}

// the data movement of one middle cipher round composed from the older primitives in the reference's order (radix_aes.h,
// aes_round_baseline).  state: 128 * inputs rows [block][input], key: 128 rows, tmp: 512 * inputs rows
void hip_test_aes_round_baseline_async(void *stream, uint32_t gpu_index, void *state, void const *key, void *tmp,
                                       uint32_t words, uint32_t inputs) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  HX_PANIC_IF_FALSE(state && key && tmp && words >= 1 && inputs >= 1, "hip_test_aes_round_baseline: null pointer or empty rows");
  aes_round_baseline((hipStream_t)stream, (uint64_t *)state, (const uint64_t *)key, (uint64_t *)tmp, words, inputs);
}

// ---- integer.h:465-499: division with remainder and absolute value (radix_divrem.h; hip_ names with the reference's
// parameter lists: the reference-named symbols stay link stubs).  A batch of integer pairs per call, capacity from
// hip_integer_scratch_batch; two's complement operands when is_signed.
uint64_t hip_scratch_integer_div_rem_64_async(CudaStreamsFFI streams, bool is_signed, int8_t **mem_ptr,
                                              CudaLweBootstrapKeyParamsFFI bsk_params,
                                              CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
                                              uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
                                              enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<DivRemMem>(streams, mem_ptr, allocate_gpu_memory, "div_rem", [&](DivRemMem &m) {
    m.core.init(streams, p, num_blocks, g_scratch_batch, is_signed, false, "div_rem");
  });
}

void hip_integer_div_rem_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *quotient, CudaRadixCiphertextFFI *remainder,
                                  CudaRadixCiphertextFFI const *numerator, CudaRadixCiphertextFFI const *divisor,
                                  bool is_signed, int8_t *mem_ptr, void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  const char *who = "div_rem";
  auto *m = scratch_use<DivRemMem>(mem_ptr, who);
  DivRemCore &d = m->core;
  const Params &p = d.drv.p;
  HX_PANIC_IF_FALSE(quotient && remainder && numerator && divisor && quotient->ptr && remainder->ptr && numerator->ptr &&
                        divisor->ptr && bsks && ksks, "%s: null pointer", who);
  HX_PANIC_IF_FALSE(is_signed == d.is_signed, "%s: the scratch was created for %s operands, the call is %s", who,
                    d.is_signed ? "signed" : "unsigned", is_signed ? "signed" : "unsigned");
  const CudaRadixCiphertextFFI *const ops[4] = {quotient, remainder, numerator, divisor};
  for (const CudaRadixCiphertextFFI *o : ops) {
    HX_PANIC_IF_FALSE(o->num_radix_blocks == numerator->num_radix_blocks,
                      "%s: quotient, remainder, numerator and divisor hold %u, %u, %u and %u blocks: they must be the same", who,
                      quotient->num_radix_blocks, remainder->num_radix_blocks, numerator->num_radix_blocks,
                      divisor->num_radix_blocks);
    HX_PANIC_IF_FALSE(o->lwe_dimension == p.big_n, "%s: the blocks' lwe dimension should be %u", who, p.big_n);
  }
  const uint32_t L = d.blocks, cts = batch_of(numerator, L, who);
  HX_PANIC_IF_FALSE(cts >= 1 && cts <= d.max_cts, "%s: %u integers exceed the scratch capacity %u", who, cts, d.max_cts);
  check_clean({numerator, divisor}, cts * L, p.msg, who, "numerator and divisor must be clean (propagate them first)");
  const size_t w = (size_t)p.big_n + 1, bytes = (size_t)cts * L * w * sizeof(uint64_t);
  const auto meet = [bytes](const void *x, const void *y) {
    const char *a = (const char *)x, *b = (const char *)y;
    return a < b + bytes && b < a + bytes;
  };
  HX_PANIC_IF_FALSE(!meet(quotient->ptr, remainder->ptr) && !meet(quotient->ptr, numerator->ptr) &&
                        !meet(quotient->ptr, divisor->ptr) && !meet(remainder->ptr, numerator->ptr) &&
                        !meet(remainder->ptr, divisor->ptr),
                    "%s: an output overlaps an input or the other output", who);
  const uint64_t before = d.issued(), want = (uint64_t)cts * DivRemCore::division_pbs(is_signed, L, p.msg);
  d.div_rem(streams, (const uint64_t *)numerator->ptr, (const uint64_t *)divisor->ptr, cts, ksks, bsks);
  const hipStream_t st = S0(streams);
  HX_CHECK(hipMemcpyAsync(quotient->ptr, d.ptr(d.OUT2), bytes, hipMemcpyDeviceToDevice, st));
  HX_CHECK(hipMemcpyAsync(remainder->ptr, d.ptr(d.OUT2) + (size_t)cts * L * w, bytes, hipMemcpyDeviceToDevice, st));
  HX_PANIC_IF_FALSE(d.issued() - before == want, "%s: %llu bootstraps issued, %llu counted", who,
                    (unsigned long long)(d.issued() - before), (unsigned long long)want);
  set_block_info(quotient, 0, cts * L, p.msg - 1, 1);
  set_block_info(remainder, 0, cts * L, p.msg - 1, 1);
}

void hip_cleanup_integer_div_rem_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<DivRemMem>(streams, mem_ptr_void, "cleanup div_rem");
}

// bootstraps of one division of two integers of num_blocks blocks (a batch issues that many per pair); every call checks it
// against the rounds it issued
uint64_t hip_integer_div_rem_pbs_count(bool is_signed, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus) {
  (void)carry_modulus;
  return DivRemCore::division_pbs(is_signed, num_blocks, message_modulus);
}

uint64_t hip_scratch_integer_abs_inplace_64_async(CudaStreamsFFI streams, int8_t **mem_ptr, bool is_signed,
                                                  CudaLweBootstrapKeyParamsFFI bsk_params,
                                                  CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
                                                  uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
                                                  enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<AbsMem>(streams, mem_ptr, allocate_gpu_memory, "abs", [&](AbsMem &m) {
    m.core.init(streams, p, num_blocks, g_scratch_batch, is_signed, true, "abs");
  });
}

// an unsigned value is its own absolute value: nothing is launched (abs.cuh:38)
void hip_integer_abs_inplace_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *ct, int8_t *mem_ptr, bool is_signed,
                                      void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<AbsMem>(mem_ptr, "abs");
  DivRemCore &d = m->core;
  const Params &p = d.drv.p;
  HX_PANIC_IF_FALSE(is_signed == d.is_signed, "abs: the scratch was created for %s operands, the call is %s",
                    d.is_signed ? "signed" : "unsigned", is_signed ? "signed" : "unsigned");
  const uint32_t cts = shift_family_batch(d.blocks, d.max_cts, p, ct, bsks, ksks, "abs");
  check_clean({ct}, cts * d.blocks, p.msg, "abs", "the value must be clean (propagate it first)");
  if (!is_signed) return;
  const uint64_t before = d.issued(), want = (uint64_t)cts * DivRemCore::abs_pbs(d.blocks);
  d.abs_inplace(streams, (uint64_t *)ct->ptr, cts, ksks, bsks);
  HX_PANIC_IF_FALSE(d.issued() - before == want, "abs: %llu bootstraps issued, %llu counted",
                    (unsigned long long)(d.issued() - before), (unsigned long long)want);
  set_block_info(ct, 0, cts * d.blocks, p.msg - 1, 1);
}

void hip_cleanup_integer_abs_inplace_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<AbsMem>(streams, mem_ptr_void, "cleanup abs");
}

// lwe_divrem_sum_kernel alone on a caller-given table (tests, tools/bench_div_rem.py).  HOST arrays: group g's entries at
// g in outs / constants and at 6 g .. 6 g + 5 in group_u32 (stride, extent, first_out, first, rows, terms); term t of group
// g at 4 g + t in srcs / stands / scalars and at 6 (4 g + t) .. + 5 in term_u32 (stride, extent, offset as int32, step,
// stand_stride, stand_row)
void hip_test_divrem_sum_async(void *stream, uint32_t gpu_index, uint32_t words, uint32_t integers, uint32_t groups,
                               void *const *outs, uint64_t const *constants, uint32_t const *group_u32,
                               void const *const *srcs, void const *const *stands, uint64_t const *scalars,
                               uint32_t const *term_u32) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  HX_PANIC_IF_FALSE(groups <= kDivGroups && outs && constants && group_u32 && srcs && stands && scalars && term_u32,
                    "hip_test_divrem_sum: %u groups (at most %u) or a null array", groups, kDivGroups);
  DivTable t = div_table(words, integers);
  t.groups = groups;
  for (uint32_t g = 0; g < groups; ++g) {
    const uint32_t *gu = group_u32 + 6 * g;
    HX_PANIC_IF_FALSE(gu[5] <= kDivTerms, "hip_test_divrem_sum: group %u has %u terms (at most %u)", g, gu[5], kDivTerms);
    DivGroup &G = t.g[g];
    G.out = (uint64_t *)outs[g], G.constant = constants[g];
    G.stride = gu[0], G.extent = gu[1], G.first_out = gu[2], G.first = gu[3], G.rows = gu[4], G.terms = gu[5];
    for (uint32_t i = 0; i < G.terms; ++i) {
      const uint32_t k = kDivTerms * g + i, *tu = term_u32 + 6 * k;
      G.t[i] = DivTerm{(const uint64_t *)srcs[k], (const uint64_t *)stands[k], scalars[k], tu[0], tu[1], (int32_t)tu[2], tu[3],
                       tu[4], tu[5]};
    }
  }
  launch_divrem_sum((hipStream_t)stream, t);
}

// benches: the data movement of iteration s of the loop composed from the primitives the layer had before the kernel, in
// the reference's order (div_rem.cuh:589-870): per integer the numerator block and the remainder pushed one block up into
// a workspace and packed against the remainder, the merged remainder added, copied into the subtraction's operand, the
// negated divisor added to its whole blocks and to its trimmed top block, the blocks above filled from constant rows; the
// flags summed into one row and added through a broadcast index to the clean and to the new remainder.
// Arrays as radix_divrem.h names them, integers L rows apart (fl, up: one row per integer): in1 receives launch 1's rows,
// in2 launch 2's merged remainder, v the subtraction's operand, in3 launch 3's rows.  negd / neglow: the negated divisor and
// the negated low part for this iteration (null when the top block is whole); consts: L rows of the trivial msg - 1; one: a
// trivial 1; zero_idx: L zeros on the device; tmp: 2 L + 1 rows.
void hip_test_divrem_iteration_baseline_async(void *stream, uint32_t gpu_index, void const *r1, void const *r2,
                                              void const *num, void const *s1, void const *s2, void const *negd,
                                              void const *neglow, void const *cl, void *v, void const *fl, void const *up,
                                              void const *consts, void const *one, void const *zero_idx, void *in1, void *in2,
                                              void *in3, void *tmp, uint32_t words, uint32_t num_blocks, uint32_t batch,
                                              uint32_t s, uint32_t bits, uint64_t message_modulus, uint32_t stage) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  HX_PANIC_IF_FALSE(r1 && r2 && num && s1 && s2 && negd && cl && v && fl && consts && one && zero_idx && in1 && in2 && in3 &&
                        tmp && words && num_blocks && batch && bits && s < bits * num_blocks && stage >= 1 && stage <= 3,
                    "hip_test_divrem_iteration_baseline: null pointer, empty rows or an iteration beyond the last");
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t L = num_blocks, B = bits * L, n = s / bits + 1, blk = (B - 1 - s) / bits, t_low = (s + 1) % bits,
                 whole = t_low ? n - 1 : n;
  HX_PANIC_IF_FALSE(!t_low || neglow, "hip_test_divrem_iteration_baseline: the top block is trimmed and neglow is null");
  const size_t w = words, bw = w * sizeof(uint64_t);
  const uint64_t f = s + 1 == B ? 2 : 3;
  const auto U = [](const void *p) { return (const uint64_t *)p; };
  const auto copy = [&](uint64_t *out, const uint64_t *x, size_t rows) {
    HX_CHECK(hipMemcpyAsync(out, x, rows * bw, hipMemcpyDeviceToDevice, st));
  };
  uint64_t *ws = (uint64_t *)tmp, *ws2 = ws + L * w, *flag = ws2 + L * w;
  for (uint32_t c = 0; c < batch; ++c) {
    const size_t at = (size_t)c * L * w;
    if (stage == 1) {
      copy(ws, U(num) + at + blk * w, 1);
      if (n > 1) copy(ws + w, U(r1) + at, n - 1);
      axpy(st, (uint64_t *)in1 + (size_t)c * n * w, nullptr, U(r1) + at, nullptr, message_modulus, ws, nullptr, words, n);
      HX_CHECK(hipMemsetAsync(ws2, 0, bw, st));
      if (n > 1) copy(ws2 + w, U(r2) + at, n - 1);
      axpy(st, (uint64_t *)in1 + (size_t)(batch + c) * n * w, nullptr, U(r2) + at, nullptr, message_modulus, ws2, nullptr, words, n);
    } else if (stage == 2) {
      uint64_t *merged = (uint64_t *)in2 + (size_t)c * n * w, *vc = (uint64_t *)v + at;
      axpy(st, merged, nullptr, U(s1) + at, nullptr, 1, U(s2) + at, nullptr, words, n);
      copy(vc, merged, n);
      if (whole) axpy(st, vc, nullptr, vc, nullptr, 1, U(negd) + at, nullptr, words, whole);
      if (t_low) axpy(st, vc + (n - 1) * w, nullptr, vc + (n - 1) * w, nullptr, 1, U(neglow) + at + (n - 1) * w, nullptr, words, 1);
      if (n < L) copy(vc + n * w, U(consts) + n * w, L - n);
    } else {
      axpy(st, flag, nullptr, U(fl) + c * w, nullptr, ~(uint64_t)0, U(one), nullptr, words, 1);
      if (up) axpy(st, flag, nullptr, flag, nullptr, 1, U(up) + c * w, nullptr, words, 1);
      axpy(st, (uint64_t *)in3 + (size_t)c * n * w, nullptr, U(cl) + at, nullptr, f, flag, U(zero_idx), words, n);
      axpy(st, (uint64_t *)in3 + (size_t)(batch + c) * n * w, nullptr, U(v) + at, nullptr, f, flag, U(zero_idx), words, n);
      copy((uint64_t *)in3 + ((size_t)2 * batch * n + c) * w, flag, 1);
    }
  }
}

// ---- integer.h:41-43, :648-662, :701-718: runs of leading / trailing bits, ilog2, and the popcounts (radix_bitcount.h; hip_
// names with the reference's parameter lists: the reference-named symbols stay link stubs; count_ones is our own, the
// reference's GPU backend has no entry point for it).  Out of place; a batch of integers per call, capacity from
// hip_integer_scratch_batch; a signed operand is counted on its two's complement bits as they stand.
namespace {
void bit_count_scratch_params(CudaLweBootstrapKeyParamsFFI bsk_params, CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t msg,
                                  uint32_t carry, uint32_t noise, const char *who, Params &p) {
  BitCountCore::check_base(msg, carry, who);  // (before make_params: its refusal of these moduli names no entry point)
  p = make_params(bsk_params, ksk_params, msg, carry, noise);
}
void bit_count_call(const CudaStreamsFFI &streams, BitCountCore &d, CudaRadixCiphertextFFI *output_ct,
                    CudaRadixCiphertextFFI const *input_ct, void *const *bsks, void *const *ksks, const char *who) {
  const Params &p = d.drv.p;
  HX_PANIC_IF_FALSE(output_ct && input_ct && output_ct->ptr && input_ct->ptr && bsks && ksks, "%s: null pointer", who);
  HX_PANIC_IF_FALSE(output_ct->lwe_dimension == p.big_n && input_ct->lwe_dimension == p.big_n,
                    "%s: the blocks' lwe dimension should be %u", who, p.big_n);
  const uint32_t L = d.blocks, nc = d.counter, cts = batch_of(input_ct, L, who);
  HX_PANIC_IF_FALSE(cts >= 1 && cts <= d.max_cts, "%s: %u integers exceed the scratch capacity %u", who, cts, d.max_cts);
  HX_PANIC_IF_FALSE(output_ct->num_radix_blocks == cts * nc, "%s: the output holds %u blocks, %u integers take %u counter blocks each",
                    who, output_ct->num_radix_blocks, cts, nc);
  check_clean({input_ct}, cts * L, p.msg, who, "the operand must be clean (propagate it first)");
  const size_t w = (size_t)p.big_n + 1;
  const char *o = (const char *)output_ct->ptr, *i = (const char *)input_ct->ptr;
  HX_PANIC_IF_FALSE(o + (size_t)cts * nc * w * sizeof(uint64_t) <= i || i + (size_t)cts * L * w * sizeof(uint64_t) <= o,
                    "%s: the output and the input must be different ciphertexts", who);
  const uint64_t before = d.issued(), want = (uint64_t)cts * BitCountCore::pbs_count(d.kind, L, p.msg, p.carry);
  d.run(streams, (uint64_t *)output_ct->ptr, (const uint64_t *)input_ct->ptr, cts, ksks, bsks);
  HX_PANIC_IF_FALSE(d.issued() - before == want, "%s: %llu bootstraps issued, %llu counted", who,
                    (unsigned long long)(d.issued() - before), (unsigned long long)want);
  set_block_info(output_ct, 0, cts * nc, p.msg - 1, 1);
}
}  // namespace

uint64_t hip_scratch_integer_count_of_consecutive_bits_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params, CudaLweKeyswitchKeyParamsFFI ksk_params,
    uint32_t num_blocks, uint32_t counter_num_blocks, uint32_t message_modulus, uint32_t carry_modulus, enum Direction direction,
    enum BitValue bit_value, bool allocate_gpu_memory, enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const char *who = "count_of_consecutive_bits";
  Params p;
  bit_count_scratch_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type, who, p);
  HX_PANIC_IF_FALSE((direction == Trailing || direction == Leading) && (bit_value == Zero || bit_value == One),
                    "%s: direction %u, bit value %u", who, (uint32_t)direction, (uint32_t)bit_value);
  return scratch_create<ConsecutiveBitsMem>(streams, mem_ptr, allocate_gpu_memory, who, [&](ConsecutiveBitsMem &m) {
    m.core.init(streams, p, kBitCountRuns, num_blocks, counter_num_blocks, g_scratch_batch, direction == Leading, bit_value == One, who);
  });
}
void hip_integer_count_of_consecutive_bits_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_ct,
                                                    CudaRadixCiphertextFFI const *input_ct, int8_t *mem_ptr, void *const *bsks,
                                                    void *const *ksks) {
  first_gpu(streams);
  const char *who = "count_of_consecutive_bits";
  bit_count_call(streams, scratch_use<ConsecutiveBitsMem>(mem_ptr, who)->core, output_ct, input_ct, bsks, ksks, who);
}
void hip_cleanup_integer_count_of_consecutive_bits_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ConsecutiveBitsMem>(streams, mem_ptr_void, "cleanup count_of_consecutive_bits");
}

uint64_t hip_scratch_integer_ilog2_64_async(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                                            CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t message_modulus,
                                            uint32_t carry_modulus, uint32_t input_num_blocks, uint32_t counter_num_blocks,
                                            uint32_t num_bits_in_ciphertext, bool allocate_gpu_memory,
                                            enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const char *who = "ilog2";
  Params p;
  bit_count_scratch_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type, who, p);
  HX_PANIC_IF_FALSE(num_bits_in_ciphertext == input_num_blocks * BitCountCore::log2_ceil(message_modulus),
                    "%s: num_bits_in_ciphertext is %u, %u blocks of modulus %u hold %u", who, num_bits_in_ciphertext, input_num_blocks,
                    message_modulus, input_num_blocks * BitCountCore::log2_ceil(message_modulus));
  return scratch_create<Ilog2Mem>(streams, mem_ptr, allocate_gpu_memory, who, [&](Ilog2Mem &m) {
    m.core.init(streams, p, kBitCountIlog2, input_num_blocks, counter_num_blocks, g_scratch_batch, true, false, who);
  });
}
// the three trivial operands are those of the reference's parameter list: their block counts are checked as the reference
// checks them (trivial_ct_neg_n against counter_num_blocks), they are otherwise NOT read — the - 1 of
// sum (b - t[i]) - 1 is a row set the scratch holds
void hip_integer_ilog2_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_ct, CudaRadixCiphertextFFI const *input_ct,
                                CudaRadixCiphertextFFI const *trivial_ct_neg_n, CudaRadixCiphertextFFI const *trivial_ct_2,
                                CudaRadixCiphertextFFI const *trivial_ct_m_minus_1_block, int8_t *mem_ptr, void *const *bsks,
                                void *const *ksks) {
  first_gpu(streams);
  const char *who = "ilog2";
  BitCountCore &d = scratch_use<Ilog2Mem>(mem_ptr, who)->core;
  HX_PANIC_IF_FALSE(trivial_ct_neg_n && trivial_ct_2 && trivial_ct_m_minus_1_block, "%s: null pointer", who);
  HX_PANIC_IF_FALSE(trivial_ct_neg_n->num_radix_blocks == d.counter,
                    "%s: num blocks of trivial_ct_neg_n should be equal to counter_num_blocks", who);
  bit_count_call(streams, d, output_ct, input_ct, bsks, ksks, who);
}
void hip_cleanup_integer_ilog2_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<Ilog2Mem>(streams, mem_ptr_void, "cleanup ilog2");
}

uint64_t hip_scratch_integer_count_ones_64_async(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params,
                                                 CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
                                                 uint32_t counter_num_blocks, uint32_t message_modulus, uint32_t carry_modulus,
                                                 enum BitValue bit_value, bool allocate_gpu_memory,
                                                 enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const char *who = "count_ones";
  Params p;
  bit_count_scratch_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type, who, p);
  HX_PANIC_IF_FALSE(bit_value == Zero || bit_value == One, "%s: bit value %u", who, (uint32_t)bit_value);
  return scratch_create<CountOnesMem>(streams, mem_ptr, allocate_gpu_memory, who, [&](CountOnesMem &m) {
    m.core.init(streams, p, kBitCountPop, num_blocks, counter_num_blocks, g_scratch_batch, false, bit_value == One, who);
  });
}
void hip_integer_count_ones_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *output_ct,
                                     CudaRadixCiphertextFFI const *input_ct, int8_t *mem_ptr, void *const *bsks, void *const *ksks) {
  first_gpu(streams);
  const char *who = "count_ones";
  bit_count_call(streams, scratch_use<CountOnesMem>(mem_ptr, who)->core, output_ct, input_ct, bsks, ksks, who);
}
void hip_cleanup_integer_count_ones_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<CountOnesMem>(streams, mem_ptr_void, "cleanup count_ones");
}

// bootstraps / rounds of one call on one integer of num_blocks blocks (a batch issues the bootstraps per integer, in the same
// rounds).  kind: 0 a run of leading / trailing bits, 1 ilog2, 2 count_ones / count_zeros.  A function of the four arguments
// alone: the scan's closed count, the plan of the column sums for these degrees, the carry propagation over the counter
// blocks.  Every call checks the bootstraps against the rounds it issued.
uint64_t hip_integer_bit_count_pbs_count(uint32_t kind, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus) {
  HX_PANIC_IF_FALSE(kind <= kBitCountPop && num_blocks >= 1, "hip_integer_bit_count_pbs_count: kind %u, %u blocks", kind, num_blocks);
  BitCountCore::check_base(message_modulus, carry_modulus, "hip_integer_bit_count_pbs_count");
  return BitCountCore::pbs_count(kind, num_blocks, message_modulus, carry_modulus);
}
uint32_t hip_integer_bit_count_rounds(uint32_t kind, uint32_t num_blocks, uint32_t message_modulus, uint32_t carry_modulus) {
  HX_PANIC_IF_FALSE(kind <= kBitCountPop && num_blocks >= 1, "hip_integer_bit_count_rounds: kind %u, %u blocks", kind, num_blocks);
  BitCountCore::check_base(message_modulus, carry_modulus, "hip_integer_bit_count_rounds");
  return BitCountCore::round_count(kind, num_blocks, message_modulus, carry_modulus);
}

// lwe_pair_pack_kernel alone on caller-supplied rows (tests, tools/bench_bit_count.py): batch integers x_stride rows apart
// in x, rows first .. first + rows - 1 of each; out receives ceil(rows / step) dense rows per integer
void hip_test_pair_pack_async(void *stream, uint32_t gpu_index, void *out, void const *x, uint64_t s0, uint64_t s1,
                              uint32_t words, uint32_t batch, uint32_t x_stride, uint32_t first, uint32_t rows, uint32_t step,
                              int delta) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  launch_pair_pack((hipStream_t)stream, PairPack{(uint64_t *)out, (const uint64_t *)x, s0, s1, words, x_stride, first, rows, step, delta, 0},
                   batch);
}

// the same rows for s0 = 1, step = 1, first = 0, x_stride = rows composed from the primitives the layer had before the kernel,
// as the reference composes a Hillis-Steele step (tools/bench_bit_count.py times one against the other): per integer a copy of
// the rows that have a partner and a memset of those that have none, then one axpy that packs.  tmp: batch rows rows.
void hip_test_pair_pack_baseline_async(void *stream, uint32_t gpu_index, void *out, void const *x, void *tmp, uint64_t s1,
                                       uint32_t words, uint32_t batch, uint32_t rows, int delta) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  const uint32_t d = (uint32_t)(delta < 0 ? -delta : delta);
  HX_PANIC_IF_FALSE(out && x && tmp && words && batch && delta != 0 && d < rows, "hip_test_pair_pack_baseline: null pointer or distance");
  const hipStream_t st = (hipStream_t)stream;
  const size_t bw = (size_t)words * sizeof(uint64_t);
  for (uint32_t c = 0; c < batch; ++c) {
    const uint64_t *src = (const uint64_t *)x + (size_t)c * rows * words;
    uint64_t *dst = (uint64_t *)tmp + (size_t)c * rows * words;
    // partner of row i is row i + delta
    if (delta > 0) {
      HX_CHECK(hipMemcpyAsync(dst, src + (size_t)d * words, (rows - d) * bw, hipMemcpyDeviceToDevice, st));
      HX_CHECK(hipMemsetAsync(dst + (size_t)(rows - d) * words, 0, d * bw, st));
    } else {
      HX_CHECK(hipMemsetAsync(dst, 0, d * bw, st));
      HX_CHECK(hipMemcpyAsync(dst + (size_t)d * words, src, (rows - d) * bw, hipMemcpyDeviceToDevice, st));
    }
  }
  axpy(st, (uint64_t *)out, nullptr, (const uint64_t *)tmp, nullptr, s1, (const uint64_t *)x, nullptr, words, batch * rows);
}

// number of PBS one carry propagation / one multiplication of `num_blocks` blocks issues (for benches)
uint64_t hip_integer_propagate_pbs_count(uint32_t num_blocks) { return PropagateMem::pbs_count(num_blocks); }
uint64_t hip_integer_mult_pbs_count(int8_t *mem_ptr) {
  if (scratch_magic(mem_ptr) == BoolMulMem::kMagic) return scratch_cast<BoolMulMem>(mem_ptr, "hip_integer_mult_pbs_count")->blocks;
  auto *m = scratch_cast<MulMem>(mem_ptr, "hip_integer_mult_pbs_count");
  uint64_t n = m->prod_slot.size();
  for (auto &s : m->steps)
    for (size_t g = 0; g < s.msg_slot.size(); ++g) n += 1 + (s.carry_slot[g] != ~(uint64_t)0);
  return n + PropagateMem::pbs_count(m->blocks);
}

// ---- sum of a vector of ciphertexts, multiplication by a clear scalar (hip_ names with the parameter lists of
// cuda/include/integer/integer.h:433-463, :862-864: the reference-named symbols stay link stubs) ----------------------
uint64_t hip_scratch_partial_sum_ciphertexts_vec_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                          CudaLweBootstrapKeyParamsFFI bsk_params,
                                                          CudaLweKeyswitchKeyParamsFFI ksk_params,
                                                          uint32_t num_blocks_in_radix, uint32_t max_num_radix_in_vec,
                                                          uint32_t message_modulus, uint32_t carry_modulus,
                                                          bool reduce_degrees_for_single_carry_propagation,
                                                          bool allocate_gpu_memory,
                                                          enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<SumMem>(streams, mem_ptr, allocate_gpu_memory, "partial_sum_ciphertexts_vec", [&](SumMem &m) {
    m.init(streams, p, num_blocks_in_radix, max_num_radix_in_vec, reduce_degrees_for_single_carry_propagation);
  });
}

void hip_partial_sum_ciphertexts_vec_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *radix_lwe_out,
                                              CudaRadixCiphertextFFI *radix_lwe_vec, int8_t *mem_ptr, void *const *bsks,
                                              void *const *ksks) {
  first_gpu(streams);
  auto *m = scratch_use<SumMem>(mem_ptr, "partial_sum_ciphertexts_vec");
  HX_PANIC_IF_FALSE(radix_lwe_out && radix_lwe_vec && bsks && ksks, "partial_sum_ciphertexts_vec: null pointer");
  const Params &p = m->drv.p;
  const uint32_t L = m->blocks, w = p.big_n + 1;
  HX_PANIC_IF_FALSE(radix_lwe_out->lwe_dimension == p.big_n && radix_lwe_vec->lwe_dimension == p.big_n,
                    "partial_sum_ciphertexts_vec: input and output lwe dimensions should be %u", p.big_n);
  HX_PANIC_IF_FALSE(radix_lwe_vec->num_radix_blocks % L == 0,
                    "partial_sum_ciphertexts_vec: input vector length should be a multiple of the scratch's number of "
                    "radix blocks (%u)", L);
  const uint32_t V = radix_lwe_vec->num_radix_blocks / L;
  HX_PANIC_IF_FALSE(V <= m->max_vec, "partial_sum_ciphertexts_vec: %u integers exceed max_num_radix_in_vec %u", V,
                    m->max_vec);
  m->last_pbs = 0;
  if (V == 0) return;
  HX_PANIC_IF_FALSE(radix_lwe_out->ptr && radix_lwe_vec->ptr && radix_lwe_out->num_radix_blocks >= L,
                    "partial_sum_ciphertexts_vec: output does not have enough blocks (%u needed)", L);
  const uint32_t cap = p.msg * p.carry - 1;
  std::vector<uint64_t> d((size_t)V * L, p.msg - 1), noise((size_t)V * L, 1);
  for (size_t i = 0; i < d.size(); ++i) {
    if (radix_lwe_vec->degrees) d[i] = radix_lwe_vec->degrees[i];
    if (radix_lwe_vec->noise_levels) noise[i] = radix_lwe_vec->noise_levels[i];
    HX_PANIC_IF_FALSE(d[i] <= cap, "partial_sum_ciphertexts_vec: block %zu has degree %llu, at most %u fits a block", i,
                      (unsigned long long)d[i], cap);
    HX_PANIC_IF_FALSE(noise[i] <= 1,
                      "partial_sum_ciphertexts_vec: block %zu has noise level %llu, the terms of a sum are at nominal noise",
                      i, (unsigned long long)noise[i]);
  }
  const hipStream_t st = S0(streams);
  uint64_t *out = (uint64_t *)radix_lwe_out->ptr;
  const uint64_t *vec = (const uint64_t *)radix_lwe_vec->ptr;
  if (V == 1) {
    if (out != vec) HX_CHECK(hipMemcpyAsync(out, vec, (size_t)L * w * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    for (uint32_t c = 0; c < L; ++c) {
      if (radix_lwe_out->degrees) radix_lwe_out->degrees[c] = d[c];
      if (radix_lwe_out->noise_levels) radix_lwe_out->noise_levels[c] = noise[c];
    }
    return;
  }
  if (V == 2) {  // a plain addition (multiplication.cuh: host_addition)
    axpy(st, out, nullptr, vec, nullptr, 1, vec + (size_t)L * w, nullptr, w, L);
    for (uint32_t c = 0; c < L; ++c) {
      if (radix_lwe_out->degrees) radix_lwe_out->degrees[c] = d[c] + d[L + c];
      if (radix_lwe_out->noise_levels) radix_lwe_out->noise_levels[c] = noise[c] + noise[L + c];
    }
    return;
  }
  if (m->key != d) m->make_plan(d, V);
  m->cs.reserve(st, 1, w);
  if (m->cs.nb != 1) m->cs.upload(st, 1, 0, 1);
  HX_RANGE("sum of %u integers of %u blocks", V, L);
  m->cs.reduce(streams, m->drv, vec, w, ksks, bsks);
  m->last_pbs = m->cs.plan.bootstraps();
  // an output that is an integer of the vector is read by the groups of its own columns only: summed in place
  const bool apart = out + (size_t)L * w <= vec || out >= vec + (size_t)V * L * w;
  m->cs.finish(st, out, vec, w, apart || (out >= vec && (size_t)(out - vec) % ((size_t)L * w) == 0));
  for (uint32_t c = 0; c < L; ++c) {
    uint64_t dc = 0, nc = 0;
    for (uint64_t x : m->cs.plan.final_cols[c]) dc += m->deg[x], nc += x < (uint64_t)V * L ? noise[x] : 1;
    if (radix_lwe_out->degrees) radix_lwe_out->degrees[c] = dc;
    if (radix_lwe_out->noise_levels) radix_lwe_out->noise_levels[c] = nc;
  }
}

void hip_cleanup_partial_sum_ciphertexts_vec_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<SumMem>(streams, mem_ptr_void, "cleanup partial_sum_ciphertexts_vec");
}
// bootstraps the last sum of this scratch issued (0 before the first, and for up to two integers)
uint64_t hip_partial_sum_ciphertexts_vec_pbs_count(int8_t *mem_ptr) {
  return scratch_cast<SumMem>(mem_ptr, "hip_partial_sum_ciphertexts_vec_pbs_count")->last_pbs;
}

// A batch of integers per call takes the same scalar; capacity from hip_integer_scratch_batch, as for the multiplication.
uint64_t hip_scratch_integer_scalar_mul_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                 CudaLweBootstrapKeyParamsFFI bsk_params,
                                                 CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks,
                                                 uint32_t message_modulus, uint32_t carry_modulus,
                                                 uint32_t num_scalar_bits, bool allocate_gpu_memory,
                                                 enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const Params p = make_params(bsk_params, ksk_params, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<ScalarMulMem>(streams, mem_ptr, allocate_gpu_memory, "integer_scalar_mul", [&](ScalarMulMem &m) {
    m.init(streams, p, num_blocks, g_scratch_batch, num_scalar_bits);
  });
}

// decomposed_scalar: num_scalars bits, least significant first; has_at_least_one_set[r]: some set bit sits at a position
// i with i % msg_bits == r.  Both on the host.  Bits at or above msg_bits * num_blocks are ignored.
void hip_integer_scalar_mul_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
                                     uint64_t const *decomposed_scalar, uint64_t const *has_at_least_one_set,
                                     int8_t *mem_ptr, void *const *bsks, void *const *ksks, uint32_t polynomial_size,
                                     uint32_t message_modulus, uint32_t num_scalars) {
  first_gpu(streams);
  auto *m = scratch_use<ScalarMulMem>(mem_ptr, "integer_scalar_mul");
  HX_PANIC_IF_FALSE(lwe_array && lwe_array->ptr && bsks && ksks && (num_scalars == 0 || decomposed_scalar) &&
                        has_at_least_one_set,
                    "integer_scalar_mul: null pointer");
  const Params &p = m->drv.p;
  HX_PANIC_IF_FALSE(polynomial_size == p.N && message_modulus == p.msg, "integer_scalar_mul: call does not match the scratch");
  HX_PANIC_IF_FALSE(lwe_array->lwe_dimension == p.big_n, "integer_scalar_mul: the blocks' lwe dimension should be %u", p.big_n);
  const uint32_t L = m->blocks, w = p.big_n + 1;
  const uint32_t cts = batch_of(lwe_array, L, "integer_scalar_mul");
  HX_PANIC_IF_FALSE(cts >= 1 && cts <= m->max_cts, "integer_scalar_mul: %u integers exceed the scratch capacity %u", cts,
                    m->max_cts);
  check_clean({lwe_array}, cts * L, p.msg, "integer_scalar_mul", "the scalar multiplication takes clean blocks");
  const std::vector<uint8_t> k = ScalarMulMem::scalar_key(decomposed_scalar, num_scalars, m->bits * L);
  HX_PANIC_IF_FALSE(k.size() <= m->scalar_bits, "integer_scalar_mul: %zu scalar bits on a scratch created for %u", k.size(),
                    m->scalar_bits);
  for (size_t i = 0; i < k.size(); ++i)
    HX_PANIC_IF_FALSE(!k[i] || has_at_least_one_set[i % m->bits] == 1,
                      "integer_scalar_mul: bit %zu is set, has_at_least_one_set[%zu] is not", i, i % m->bits);
  if (!m->planned || m->key != k) m->make_plan(k);
  if (!m->any_bit) {
    HX_CHECK(hipMemsetAsync(lwe_array->ptr, 0, (size_t)cts * L * w * sizeof(uint64_t), S0(streams)));
    set_block_info(lwe_array, 0, cts * L, 0, 0);
    return;
  }
  m->run(streams, (uint64_t *)lwe_array->ptr, cts, ksks, bsks);
  set_block_info(lwe_array, 0, cts * L, p.msg - 1, 1);
}

void hip_cleanup_integer_scalar_mul_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ScalarMulMem>(streams, mem_ptr_void, "cleanup integer_scalar_mul");
}

// bootstraps per integer of a multiplication by this scalar: shifted blocks + column sums + carry propagation
uint64_t hip_integer_scalar_mul_pbs_count(int8_t *mem_ptr, uint64_t const *decomposed_scalar, uint32_t num_scalars) {
  auto *m = scratch_cast<ScalarMulMem>(mem_ptr, "hip_integer_scalar_mul_pbs_count");
  const std::vector<uint8_t> k = ScalarMulMem::scalar_key(decomposed_scalar, num_scalars, m->bits * m->blocks);
  if (!m->planned || m->key != k) m->make_plan(k);
  return m->any_bit ? m->pbs_count() : 0;
}

// the two column-sum kernels on the same CSR over one pool, for timing one against the other (tools/bench_scalar_mul.py):
// which = 0 lwe_group_sum_kernel, 1 lwe_gather_sum2_kernel (every member a pool row)
void hip_test_group_sum_async(void *stream, uint32_t gpu_index, uint32_t which, void *out, void const *pool,
                              void const *offsets, void const *members, uint32_t words, uint32_t groups) {
  HX_CHECK(hipSetDevice((int)gpu_index));
  HX_PANIC_IF_FALSE(which <= 1 && groups >= 1 && words >= 1, "hip_test_group_sum: unknown kernel or empty launch");
  if (which == 0)
    HX_LAUNCH(lwe_group_sum_kernel, dim3(groups), dim3(256), 0, (hipStream_t)stream, (uint64_t *)out,
              (const uint64_t *)pool, (const uint64_t *)offsets, (const uint64_t *)members, words, groups);
  else
    launch_gather_sum2((hipStream_t)stream, (uint64_t *)out, (const uint64_t *)pool, (const uint64_t *)pool,
                       (const uint64_t *)offsets, (const uint64_t *)members, words, groups);
}

// scalar_mul.cuh:139-177 (host_integer_small_scalar_mul_radix): every word times a small scalar; degrees and noise levels
// scale, and a noise level above what the parameter set is made for, (msg carry - 1) / (msg - 1), is refused
void hip_small_scalar_multiplication_integer_64_inplace_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array,
                                                              uint64_t scalar, const uint32_t message_modulus,
                                                              const uint32_t carry_modulus) {
  first_gpu(streams);
  HX_PANIC_IF_FALSE(lwe_array && lwe_array->ptr, "small_scalar_multiplication_integer: null radix ciphertext");
  HX_PANIC_IF_FALSE(message_modulus >= 2 && carry_modulus >= 1, "small_scalar_multiplication_integer: invalid message modulus or carry modulus");
  const uint64_t max_noise = ((uint64_t)message_modulus * carry_modulus - 1) / (message_modulus - 1);
  for (uint32_t i = 0; i < lwe_array->num_radix_blocks; ++i)
    if (lwe_array->noise_levels)
      HX_PANIC_IF_FALSE(lwe_array->noise_levels[i] * scalar <= max_noise,
                        "small_scalar_multiplication_integer: noise %llu exceeds maximum authorized value %llu",
                        (unsigned long long)(lwe_array->noise_levels[i] * scalar), (unsigned long long)max_noise);
  axpy(S0(streams), (uint64_t *)lwe_array->ptr, nullptr, (const uint64_t *)lwe_array->ptr, nullptr, scalar, nullptr, nullptr,
       lwe_array->lwe_dimension + 1, lwe_array->num_radix_blocks);
  for (uint32_t i = 0; i < lwe_array->num_radix_blocks; ++i) {
    if (lwe_array->degrees) lwe_array->degrees[i] *= scalar;
    if (lwe_array->noise_levels) lwe_array->noise_levels[i] *= scalar;
  }
}

// ---- ciphertext compression (hip_ names: the reference-named compression symbols stay link stubs) ---------------------
uint64_t hip_integer_compressed_size_words(uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t lwe_per_glwe,
                                           uint32_t storage_log_modulus, uint32_t total_blocks) {
  check_compression_glwe(glwe_dimension, polynomial_size, "compressed_size_words");
  check_storage(polynomial_size, lwe_per_glwe, storage_log_modulus, "compressed_size_words");
  const uint64_t glwes = ((uint64_t)total_blocks + lwe_per_glwe - 1) / lwe_per_glwe;
  return glwes * packed_words_per_glwe(glwe_dimension, polynomial_size, lwe_per_glwe, storage_log_modulus);
}

static CompressionShape compression_shape(uint32_t n_in, uint32_t k, uint32_t N, uint32_t base_log, uint32_t level,
                                          const char *who) {
  check_compression_glwe(k, N, who);
  HX_PANIC_IF_FALSE(n_in >= 1 && base_log >= 1 && level >= 1 && base_log * level < 64,
                    "%s: unsupported packing key (input dimension %u, base_log %u, level %u)", who, n_in, base_log, level);
  CompressionShape sh;
  sh.n_in = n_in, sh.k = k, sh.N = N, sh.base_log = base_log, sh.level = level;
  return sh;
}

uint64_t hip_scratch_packing_keyswitch_lwe_list_to_glwe_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                                 uint32_t input_lwe_dimension, uint32_t glwe_dimension,
                                                                 uint32_t polynomial_size, uint32_t base_log,
                                                                 uint32_t level_count, uint32_t num_lwes,
                                                                 bool allocate_gpu_memory) {
  const CompressionShape sh = compression_shape(input_lwe_dimension, glwe_dimension, polynomial_size, base_log, level_count,
                                                "packing_keyswitch");
  return scratch_create<PackingKsMem>(streams, mem_ptr, allocate_gpu_memory, "packing_keyswitch",
                                      [&](PackingKsMem &m) { m.init(streams, sh, num_lwes); });
}

void hip_packing_keyswitch_lwe_list_to_glwe_64_async(CudaStreamsFFI streams, void *glwe_array_out, void const *lwe_array_in,
                                                     void const *fp_ksk, int8_t *mem_ptr, uint32_t input_lwe_dimension,
                                                     uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t base_log,
                                                     uint32_t level_count, uint32_t num_lwes, uint32_t lwe_per_glwe) {
  first_gpu(streams);
  auto *m = scratch_use<PackingKsMem>(mem_ptr, "packing_keyswitch");
  HX_PANIC_IF_FALSE(glwe_array_out && lwe_array_in && fp_ksk, "packing_keyswitch: null pointer");
  HX_PANIC_IF_FALSE(m->sh.n_in == input_lwe_dimension && m->sh.k == glwe_dimension && m->sh.N == polynomial_size &&
                        m->sh.base_log == base_log && m->sh.level == level_count,
                    "packing_keyswitch: parameters differ from the ones the scratch was created with");
  HX_PANIC_IF_FALSE(lwe_per_glwe >= 1 && lwe_per_glwe <= polynomial_size,
                    "packing_keyswitch: cannot pack more than polynomial_size (%u) LWEs per GLWE, %u requested", polynomial_size,
                    lwe_per_glwe);
  HX_PANIC_IF_FALSE(num_lwes <= m->cap, "packing_keyswitch: %u LWEs exceed the scratch capacity %u", num_lwes, m->cap);
  launch_packing_keyswitch(S0(streams), (uint64_t *)glwe_array_out, m->d_rows, m->d_trivial, (const uint64_t *)lwe_array_in,
                           (const uint64_t *)fp_ksk, m->sh.n_in, m->sh.k, m->sh.N, m->sh.base_log, m->sh.level, num_lwes,
                           lwe_per_glwe, 0);
}

void hip_cleanup_packing_keyswitch_lwe_list_to_glwe_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<PackingKsMem>(streams, mem_ptr_void, "cleanup packing_keyswitch");
}

uint64_t hip_scratch_integer_compress_radix_ciphertext_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t input_lwe_dimension, uint32_t compression_glwe_dimension,
    uint32_t compression_polynomial_size, uint32_t ks_base_log, uint32_t ks_level, uint32_t num_radix_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, uint32_t lwe_per_glwe, uint32_t storage_log_modulus,
    bool allocate_gpu_memory) {
  const CompressionShape sh = compression_shape(input_lwe_dimension, compression_glwe_dimension, compression_polynomial_size,
                                                ks_base_log, ks_level, "integer_compress");
  check_storage(compression_polynomial_size, lwe_per_glwe, storage_log_modulus, "integer_compress");
  // compression.rs:51-56: the message moves into the carry space
  HX_PANIC_IF_FALSE(message_modulus >= 2 && message_modulus <= carry_modulus,
                    "integer_compress: GLWE packing is implemented with messages in carries, so carry_modulus (=%u) must be "
                    "greater than or equal to message_modulus (=%u)", carry_modulus, message_modulus);
  return scratch_create<CompressMem>(streams, mem_ptr, allocate_gpu_memory, "integer_compress", [&](CompressMem &m) {
    m.pks.init(streams, sh, num_radix_blocks);
    m.msg = message_modulus, m.carry = carry_modulus, m.lwe_per_glwe = lwe_per_glwe, m.bits = storage_log_modulus;
    m.own.alloc(m.d_scaled, (size_t)m.pks.cap * (sh.n_in + 1) * sizeof(uint64_t));
  });
}

void hip_integer_compress_radix_ciphertext_64_async(CudaStreamsFFI streams, void *packed_out,
                                                    CudaRadixCiphertextFFI const *lwe_array_in, void *const *fp_ksks,
                                                    int8_t *mem_ptr) {
  first_gpu(streams);
  auto *m = scratch_use<CompressMem>(mem_ptr, "integer_compress");
  HX_PANIC_IF_FALSE(packed_out && lwe_array_in && lwe_array_in->ptr && fp_ksks && fp_ksks[0], "integer_compress: null pointer");
  const CompressionShape &sh = m->pks.sh;
  HX_PANIC_IF_FALSE(lwe_array_in->lwe_dimension == sh.n_in,
                    "integer_compress: ciphertexts do not have the lwe dimension of the packing keyswitch key (%u, key %u)",
                    lwe_array_in->lwe_dimension, sh.n_in);
  const uint32_t n = lwe_array_in->num_radix_blocks;
  HX_PANIC_IF_FALSE(n <= m->pks.cap, "integer_compress: %u blocks exceed the scratch capacity %u", n, m->pks.cap);
  check_clean({lwe_array_in}, n, m->msg, "integer_compress", "ciphertexts must have empty carries to be compressed");
  const hipStream_t st = S0(streams);
  axpy(st, m->d_scaled, nullptr, (const uint64_t *)lwe_array_in->ptr, nullptr, m->msg, nullptr, nullptr, sh.n_in + 1, n);
  launch_packing_keyswitch(st, (uint64_t *)packed_out, m->pks.d_rows, m->pks.d_trivial, m->d_scaled,
                           (const uint64_t *)fp_ksks[0], sh.n_in, sh.k, sh.N, sh.base_log, sh.level, n, m->lwe_per_glwe,
                           m->bits);
}

void hip_cleanup_integer_compress_radix_ciphertext_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<CompressMem>(streams, mem_ptr_void, "cleanup integer_compress");
}

uint64_t hip_scratch_integer_decompress_radix_ciphertext_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweBootstrapKeyParamsFFI bsk_params, uint32_t compression_glwe_dimension,
    uint32_t compression_polynomial_size, uint32_t lwe_per_glwe, uint32_t storage_log_modulus,
    uint32_t num_blocks_to_decompress, uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type) {
  check_compression_glwe(compression_glwe_dimension, compression_polynomial_size, "integer_decompress");
  check_storage(compression_polynomial_size, lwe_per_glwe, storage_log_modulus, "integer_decompress");
  HX_PANIC_IF_FALSE(bsk_params.input_lwe_dimension == compression_glwe_dimension * compression_polynomial_size,
                    "integer_decompress: the decompression key's input dimension %u is not the compression GLWE's %u x %u",
                    bsk_params.input_lwe_dimension, compression_glwe_dimension, compression_polynomial_size);
  // compression.rs:182-188
  HX_PANIC_IF_FALSE(message_modulus == carry_modulus,
                    "integer_decompress: message modulus (%u) != carry modulus (%u) is not supported", message_modulus,
                    carry_modulus);
  // no keyswitch in front of this bootstrap: the key parameters below only restate the bootstrap's own dimensions
  const CudaLweKeyswitchKeyParamsFFI no_ks{bsk_params.glwe_dimension * bsk_params.polynomial_size,
                                           bsk_params.input_lwe_dimension, 1, 1};
  const Params p = make_params(bsk_params, no_ks, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  return scratch_create<DecompressMem>(streams, mem_ptr, allocate_gpu_memory, "integer_decompress", [&](DecompressMem &m) {
    const hipStream_t st = S0(streams);
    m.p = p;
    m.kc = compression_glwe_dimension, m.Nc = compression_polynomial_size;
    m.lwe_per_glwe = lwe_per_glwe, m.bits = storage_log_modulus;
    m.cap = std::max(1u, num_blocks_to_decompress);
    m.gpu = G0(streams);
    m.own.alloc(m.d_extracted, (size_t)m.cap * (p.small_n + 1) * sizeof(uint64_t));
    m.own.alloc(m.d_indexes, (size_t)m.cap * sizeof(uint32_t));
    m.own.alloc(m.d_lut_idx, (size_t)m.cap * sizeof(uint64_t));
    std::vector<uint64_t> lut((size_t)(p.k + 1) * p.N), triv(m.cap);
    generate_rescaling_lut(p, lut.data());
    for (uint32_t i = 0; i < m.cap; ++i) triv[i] = i;
    m.d_lut = m.own.upload(st, lut);
    m.d_trivial = m.own.upload(st, triv);
    if (!t_dry) {
      HX_CHECK(hipMemsetAsync(m.d_lut_idx, 0, (size_t)m.cap * sizeof(uint64_t), st));
      HX_CHECK(hipHostMalloc((void **)&m.h_indexes, (size_t)m.cap * sizeof(uint32_t), 0));
      HX_CHECK(hipEventCreateWithFlags(&m.uploaded, hipEventDisableTiming));
    }
    if (p.grouping)
      scratch_cuda_multi_bit_programmable_bootstrap_64_async(st, m.gpu, &m.pbs_buf, p.k, p.N, p.pbs_level, m.cap, !t_dry);
    else
      scratch_cuda_programmable_bootstrap_64_async(st, m.gpu, &m.pbs_buf, p.small_n, p.k, p.N, p.pbs_level, m.cap, !t_dry,
                                                   (enum PBS_MS_REDUCTION_T)p.ms_type);
  });
}

void hip_integer_decompress_radix_ciphertext_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                                                      void const *packed_in, uint32_t total_lwe_bodies_count,
                                                      uint32_t const *h_indexes, uint32_t num_indexes, void *const *bsks,
                                                      int8_t *mem_ptr) {
  first_gpu(streams);
  auto *m = scratch_use<DecompressMem>(mem_ptr, "integer_decompress");
  HX_PANIC_IF_FALSE(lwe_array_out && lwe_array_out->ptr && packed_in && (h_indexes || num_indexes == 0) && bsks && bsks[0],
                    "integer_decompress: null pointer");
  const Params &p = m->p;
  HX_PANIC_IF_FALSE(lwe_array_out->lwe_dimension == p.big_n,
                    "integer_decompress: output blocks of lwe dimension %u, the decompression key writes %u",
                    lwe_array_out->lwe_dimension, p.big_n);
  HX_PANIC_IF_FALSE(num_indexes <= m->cap && num_indexes <= lwe_array_out->num_radix_blocks,
                    "integer_decompress: %u indexes exceed the scratch capacity %u or the output's %u blocks", num_indexes,
                    m->cap, lwe_array_out->num_radix_blocks);
  for (uint32_t i = 0; i < num_indexes; ++i) {
    // compression.rs:169-175
    HX_PANIC_IF_FALSE(h_indexes[i] < total_lwe_bodies_count,
                      "integer_decompress: tried getting index %u for a compressed list with %u elements, out of bound access",
                      h_indexes[i], total_lwe_bodies_count);
    // compression.cuh:381-400 walks the GLWEs in order; here any order would do (a workgroup per index reads its own
    // GLWE), the check keeps the reference's contract
    HX_PANIC_IF_FALSE(i == 0 || h_indexes[i] / m->lwe_per_glwe >= h_indexes[i - 1] / m->lwe_per_glwe,
                      "integer_decompress: indexes must be non-decreasing in GLWE index (index %u after %u)", h_indexes[i],
                      h_indexes[i - 1]);
  }
  if (num_indexes == 0) return;
  const hipStream_t st = S0(streams);
  HX_CHECK(hipEventSynchronize(m->uploaded));  // the previous call's copy out of the staging buffer (no-op before the first)
  std::copy(h_indexes, h_indexes + num_indexes, m->h_indexes);
  HX_CHECK(hipMemcpyAsync(m->d_indexes, m->h_indexes, (size_t)num_indexes * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HX_CHECK(hipEventRecord(m->uploaded, st));
  launch_unpack_extract(st, m->d_extracted, (const uint64_t *)packed_in, m->d_indexes, num_indexes, m->kc, m->Nc,
                        m->lwe_per_glwe, m->bits, packed_words_per_glwe(m->kc, m->Nc, m->lwe_per_glwe, m->bits));
  uint64_t *out = (uint64_t *)lwe_array_out->ptr;
  if (p.grouping)
    cuda_multi_bit_programmable_bootstrap_64_async(st, m->gpu, out, m->d_trivial, m->d_lut, m->d_lut_idx, m->d_extracted,
                                                   m->d_trivial, bsks[0], m->pbs_buf, p.small_n, p.k, p.N, p.grouping,
                                                   p.pbs_base_log, p.pbs_level, num_indexes, 1, 0);
  else
    cuda_programmable_bootstrap_64_async(st, m->gpu, out, m->d_trivial, m->d_lut, m->d_lut_idx, m->d_extracted, m->d_trivial,
                                         bsks[0], m->pbs_buf, p.small_n, p.k, p.N, p.pbs_base_log, p.pbs_level, num_indexes,
                                         1, 0);
  set_block_info(lwe_array_out, 0, num_indexes, p.msg - 1, 1);
}

void hip_cleanup_integer_decompress_radix_ciphertext_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<DecompressMem>(streams, mem_ptr_void, "cleanup integer_decompress");
}

void hip_integer_extract_glwe_64_async(CudaStreamsFFI streams, void *glwe_out, void const *packed_in, uint32_t glwe_index,
                                       uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t lwe_per_glwe,
                                       uint32_t storage_log_modulus, uint32_t total_lwe_bodies_count) {
  first_gpu(streams);
  HX_PANIC_IF_FALSE(glwe_out && packed_in, "integer_extract_glwe: null pointer");
  check_compression_glwe(glwe_dimension, polynomial_size, "integer_extract_glwe");
  check_storage(polynomial_size, lwe_per_glwe, storage_log_modulus, "integer_extract_glwe");
  HX_PANIC_IF_FALSE((uint64_t)glwe_index * lwe_per_glwe < total_lwe_bodies_count,
                    "integer_extract_glwe: GLWE %u of a compressed list with %u elements, out of bound access", glwe_index,
                    total_lwe_bodies_count);
  const uint32_t bodies = std::min(lwe_per_glwe, total_lwe_bodies_count - glwe_index * lwe_per_glwe);
  const uint32_t words = packed_words_per_glwe(glwe_dimension, polynomial_size, lwe_per_glwe, storage_log_modulus);
  launch_unpack_glwe(S0(streams), (uint64_t *)glwe_out, (const uint64_t *)packed_in + (size_t)glwe_index * words,
                     glwe_dimension, polynomial_size, bodies, storage_log_modulus);
}

// ---- compression of squashed-noise (128-bit) ciphertext lists (hip_ names: the reference-named *_128 compression symbols
// stay link stubs).  shortint/list_compression/noise_squashing_compression.rs; the kernels are pks128_kernels.h.
namespace {
struct Pks128Shape {
  uint32_t n_in = 0, k = 0, N = 0, base_log = 0, level = 0;  // packing key: [n_in][level][(k+1)*N] u128
  uint32_t ncols() const { return (k + 1) * N; }
  bool operator==(const Pks128Shape &o) const {
    return n_in == o.n_in && k == o.k && N == o.N && base_log == o.base_log && level == o.level;
  }
  // the shapes the kernels of pks128_kernels.h are written for; anything else is refused here
  static Pks128Shape checked(uint32_t n_in, uint32_t k, uint32_t N, uint32_t base_log, uint32_t level, const char *who) {
    check_compression_glwe(k, N, who);
    HX_PANIC_IF_FALSE(n_in >= 1 && base_log >= 1 && level >= 1,
                      "%s: unsupported packing key (input dimension %u, base_log %u, level %u)", who, n_in, base_log, level);
    HX_PANIC_IF_FALSE(base_log <= 62, "%s: base_log %u above 62: a digit must fit a signed 64-bit value", who, base_log);
    HX_PANIC_IF_FALSE((uint64_t)base_log * level <= 128, "%s: base_log %u * level %u exceeds the 128 bits of a word", who,
                      base_log, level);
    Pks128Shape sh;
    sh.n_in = n_in, sh.k = k, sh.N = N, sh.base_log = base_log, sh.level = level;
    return sh;
  }
};
void check_storage128(uint32_t N, uint32_t lwe_per_glwe, uint32_t bits, const char *who) {
  HX_PANIC_IF_FALSE(lwe_per_glwe >= 1 && lwe_per_glwe <= N,
                    "%s: cannot pack more than polynomial_size (%u) LWEs per GLWE, %u requested", who, N, lwe_per_glwe);
  HX_PANIC_IF_FALSE(bits >= 1 && bits <= 128, "%s: storage_log_modulus %u must be in 1..128", who, bits);
}

// core level: u128 LWE list -> unswitched u128 GLWEs
struct PackingKs128Mem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x504B3132;  // "PK12"
  Pks128Shape sh;
  uint32_t cap = 0;  // LWEs per call
  Pks128Workspace ws;
  DeviceBlocks own;
  void init(const Pks128Shape &shape, uint32_t capacity) {
    sh = shape;
    cap = std::max(1u, capacity);
    own.alloc(ws.rows, pks128_rows_bytes(cap, sh.n_in, sh.ncols(), sh.base_log, sh.level));
    if (const uint64_t bytes = pks128_digits_bytes(cap, sh.n_in, sh.base_log, sh.level)) {
      own.alloc(ws.digits, bytes);
      own.alloc(ws.digit_sums, (size_t)cap * 16);
    }
  }
  void release(const CudaStreamsFFI &s) { own.release(S0(s)); }
};
struct Compress128Mem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x434D3132;  // "CM12"
  PackingKs128Mem pks;  // member: no header of its own in use
  uint32_t msg = 0, carry = 0, lwe_per_glwe = 0, bits = 0;
  void release(const CudaStreamsFFI &s) { pks.release(s); }
};
struct Decompress128Mem : ScratchHeader {
  static constexpr uint32_t kMagic = 0x44433132;  // "DC12"
  uint32_t kc = 0, Nc = 0, lwe_per_glwe = 0, bits = 0, cap = 0, msg = 0, carry = 0;
  uint32_t *d_indexes = nullptr, *h_indexes = nullptr;  // h_indexes: pinned staging of the caller's host array
  hipEvent_t uploaded = nullptr;                         // behind the last copy out of h_indexes
  DeviceBlocks own;
  void release(const CudaStreamsFFI &s) {
    own.release(S0(s));
    if (h_indexes) HX_CHECK(hipHostFree(h_indexes));
    if (uploaded) HX_CHECK(hipEventDestroy(uploaded));
  }
};
}  // namespace

void hip_backend_set_pks128_kernel(uint32_t which) { pks128_set_kernel(which); }
uint32_t hip_backend_last_pks128_path(void) { return pks128_last_path(); }
void hip_backend_set_pks128_max_parts(uint32_t parts) { pks128_set_max_parts(parts); }
uint32_t hip_backend_last_pks128_parts(void) { return pks128_last_parts(); }

uint64_t hip_integer_compressed_size_words_128(uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t lwe_per_glwe,
                                               uint32_t storage_log_modulus, uint32_t total_blocks) {
  check_compression_glwe(glwe_dimension, polynomial_size, "compressed_size_words_128");
  check_storage128(polynomial_size, lwe_per_glwe, storage_log_modulus, "compressed_size_words_128");
  const uint64_t glwes = ((uint64_t)total_blocks + lwe_per_glwe - 1) / lwe_per_glwe;
  return glwes * pks128_words_per_glwe(glwe_dimension, polynomial_size, lwe_per_glwe, storage_log_modulus);
}

uint64_t hip_lwe_packing_keyswitch_key_128_planes_size_bytes(uint32_t input_lwe_dimension, uint32_t glwe_dimension,
                                                             uint32_t polynomial_size, uint32_t base_log,
                                                             uint32_t level_count) {
  const Pks128Shape sh = Pks128Shape::checked(input_lwe_dimension, glwe_dimension, polynomial_size, base_log, level_count,
                                      "packing_keyswitch_key_128_planes_size");
  return pks128_planes_bytes(sh.n_in, sh.ncols(), sh.base_log, sh.level);
}

void hip_convert_lwe_packing_keyswitch_key_128_async(CudaStreamsFFI streams, void *dest_planes, void const *src_key,
                                                     uint32_t input_lwe_dimension, uint32_t glwe_dimension,
                                                     uint32_t polynomial_size, uint32_t base_log, uint32_t level_count) {
  first_gpu(streams);
  const Pks128Shape sh = Pks128Shape::checked(input_lwe_dimension, glwe_dimension, polynomial_size, base_log, level_count,
                                      "convert_packing_keyswitch_key_128");
  HX_PANIC_IF_FALSE(dest_planes && src_key, "convert_packing_keyswitch_key_128: null pointer");
  HX_PANIC_IF_FALSE(pks128_planes_bytes(sh.n_in, sh.ncols(), sh.base_log, sh.level) != 0,
                    "convert_packing_keyswitch_key_128: the matrix-core kernel does not carry this shape (the planes size is 0)");
  launch_pks128_convert_key(S0(streams), dest_planes, (const uint64_t *)src_key, sh.n_in, sh.ncols(), sh.level);
}

uint64_t hip_scratch_packing_keyswitch_lwe_list_to_glwe_128_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                                  uint32_t input_lwe_dimension, uint32_t glwe_dimension,
                                                                  uint32_t polynomial_size, uint32_t base_log,
                                                                  uint32_t level_count, uint32_t num_lwes,
                                                                  bool allocate_gpu_memory) {
  const Pks128Shape sh = Pks128Shape::checked(input_lwe_dimension, glwe_dimension, polynomial_size, base_log, level_count,
                                      "packing_keyswitch_128");
  return scratch_create<PackingKs128Mem>(streams, mem_ptr, allocate_gpu_memory, "packing_keyswitch_128",
                                         [&](PackingKs128Mem &m) { m.init(sh, num_lwes); });
}

void hip_packing_keyswitch_lwe_list_to_glwe_128_async(CudaStreamsFFI streams, void *glwe_array_out, void const *lwe_array_in,
                                                      void const *fp_ksk, void const *fp_ksk_planes, int8_t *mem_ptr,
                                                      uint32_t input_lwe_dimension, uint32_t glwe_dimension,
                                                      uint32_t polynomial_size, uint32_t base_log, uint32_t level_count,
                                                      uint32_t num_lwes, uint32_t lwe_per_glwe) {
  first_gpu(streams);
  auto *m = scratch_use<PackingKs128Mem>(mem_ptr, "packing_keyswitch_128");
  HX_PANIC_IF_FALSE(glwe_array_out && lwe_array_in && fp_ksk, "packing_keyswitch_128: null pointer");
  Pks128Shape given;
  given.n_in = input_lwe_dimension, given.k = glwe_dimension, given.N = polynomial_size, given.base_log = base_log,
  given.level = level_count;
  HX_PANIC_IF_FALSE(m->sh == given, "packing_keyswitch_128: parameters differ from the ones the scratch was created with");
  HX_PANIC_IF_FALSE(lwe_per_glwe >= 1 && lwe_per_glwe <= polynomial_size,
                    "packing_keyswitch_128: cannot pack more than polynomial_size (%u) LWEs per GLWE, %u requested",
                    polynomial_size, lwe_per_glwe);
  HX_PANIC_IF_FALSE(num_lwes <= m->cap, "packing_keyswitch_128: %u LWEs exceed the scratch capacity %u", num_lwes, m->cap);
  launch_packing_keyswitch128(S0(streams), (uint64_t *)glwe_array_out, m->ws, (const uint64_t *)lwe_array_in,
                              (const uint64_t *)fp_ksk, fp_ksk_planes, m->sh.n_in, m->sh.k, m->sh.N, m->sh.base_log,
                              m->sh.level, num_lwes, lwe_per_glwe, 0);
}

void hip_cleanup_packing_keyswitch_lwe_list_to_glwe_128(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<PackingKs128Mem>(streams, mem_ptr_void, "cleanup packing_keyswitch_128");
}

uint64_t hip_scratch_integer_compress_radix_ciphertext_128_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t input_lwe_dimension, uint32_t compression_glwe_dimension,
    uint32_t compression_polynomial_size, uint32_t ks_base_log, uint32_t ks_level, uint32_t num_radix_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, uint32_t lwe_per_glwe, uint32_t storage_log_modulus,
    bool allocate_gpu_memory) {
  const Pks128Shape sh = Pks128Shape::checked(input_lwe_dimension, compression_glwe_dimension, compression_polynomial_size,
                                      ks_base_log, ks_level, "integer_compress_128");
  check_storage128(compression_polynomial_size, lwe_per_glwe, storage_log_modulus, "integer_compress_128");
  return scratch_create<Compress128Mem>(streams, mem_ptr, allocate_gpu_memory, "integer_compress_128", [&](Compress128Mem &m) {
    m.pks.init(sh, num_radix_blocks);
    m.msg = message_modulus, m.carry = carry_modulus, m.lwe_per_glwe = lwe_per_glwe, m.bits = storage_log_modulus;
  });
}

void hip_integer_compress_radix_ciphertext_128_async(CudaStreamsFFI streams, void *packed_out,
                                                     CudaRadixCiphertextFFI const *lwe_array_in, void *const *fp_ksks,
                                                     void *const *fp_ksk_planes, int8_t *mem_ptr) {
  first_gpu(streams);
  auto *m = scratch_use<Compress128Mem>(mem_ptr, "integer_compress_128");
  HX_PANIC_IF_FALSE(packed_out && lwe_array_in && lwe_array_in->ptr && fp_ksks && fp_ksks[0], "integer_compress_128: null pointer");
  const Pks128Shape &sh = m->pks.sh;
  HX_PANIC_IF_FALSE(lwe_array_in->lwe_dimension == sh.n_in,
                    "integer_compress_128: ciphertexts do not have the lwe dimension of the packing keyswitch key (%u, key %u)",
                    lwe_array_in->lwe_dimension, sh.n_in);
  const uint32_t n = lwe_array_in->num_radix_blocks;
  HX_PANIC_IF_FALSE(n <= m->pks.cap, "integer_compress_128: %u blocks exceed the scratch capacity %u", n, m->pks.cap);
  launch_packing_keyswitch128(S0(streams), (uint64_t *)packed_out, m->pks.ws, (const uint64_t *)lwe_array_in->ptr,
                              (const uint64_t *)fp_ksks[0], fp_ksk_planes ? fp_ksk_planes[0] : nullptr, sh.n_in, sh.k, sh.N,
                              sh.base_log, sh.level, n, m->lwe_per_glwe, m->bits);
}

void hip_cleanup_integer_compress_radix_ciphertext_128(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<Compress128Mem>(streams, mem_ptr_void, "cleanup integer_compress_128");
}

uint64_t hip_scratch_integer_decompress_radix_ciphertext_128_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t compression_glwe_dimension, uint32_t compression_polynomial_size,
    uint32_t lwe_per_glwe, uint32_t storage_log_modulus, uint32_t num_blocks_to_decompress, uint32_t message_modulus,
    uint32_t carry_modulus, bool allocate_gpu_memory) {
  check_compression_glwe(compression_glwe_dimension, compression_polynomial_size, "integer_decompress_128");
  check_storage128(compression_polynomial_size, lwe_per_glwe, storage_log_modulus, "integer_decompress_128");
  return scratch_create<Decompress128Mem>(streams, mem_ptr, allocate_gpu_memory, "integer_decompress_128", [&](Decompress128Mem &m) {
    m.kc = compression_glwe_dimension, m.Nc = compression_polynomial_size;
    m.lwe_per_glwe = lwe_per_glwe, m.bits = storage_log_modulus;
    m.msg = message_modulus, m.carry = carry_modulus;
    m.cap = std::max(1u, num_blocks_to_decompress);
    m.own.alloc(m.d_indexes, (size_t)m.cap * sizeof(uint32_t));
    if (!t_dry) {
      HX_CHECK(hipHostMalloc((void **)&m.h_indexes, (size_t)m.cap * sizeof(uint32_t), 0));
      HX_CHECK(hipEventCreateWithFlags(&m.uploaded, hipEventDisableTiming));
    }
  });
}

void hip_integer_decompress_radix_ciphertext_128_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                                                       void const *packed_in, uint32_t total_lwe_bodies_count,
                                                       uint32_t const *h_indexes, uint32_t num_indexes, int8_t *mem_ptr) {
  first_gpu(streams);
  auto *m = scratch_use<Decompress128Mem>(mem_ptr, "integer_decompress_128");
  HX_PANIC_IF_FALSE(lwe_array_out && lwe_array_out->ptr && packed_in && (h_indexes || num_indexes == 0),
                    "integer_decompress_128: null pointer");
  HX_PANIC_IF_FALSE(lwe_array_out->lwe_dimension == m->kc * m->Nc,
                    "integer_decompress_128: output blocks of lwe dimension %u, the compression GLWE extracts to %u",
                    lwe_array_out->lwe_dimension, m->kc * m->Nc);
  HX_PANIC_IF_FALSE(num_indexes <= m->cap && num_indexes <= lwe_array_out->num_radix_blocks,
                    "integer_decompress_128: %u indexes exceed the scratch capacity %u or the output's %u blocks", num_indexes,
                    m->cap, lwe_array_out->num_radix_blocks);
  for (uint32_t i = 0; i < num_indexes; ++i) {
    HX_PANIC_IF_FALSE(h_indexes[i] < total_lwe_bodies_count,
                      "integer_decompress_128: tried getting index %u for a compressed list with %u elements, out of bound access",
                      h_indexes[i], total_lwe_bodies_count);
    HX_PANIC_IF_FALSE(i == 0 || h_indexes[i] / m->lwe_per_glwe >= h_indexes[i - 1] / m->lwe_per_glwe,
                      "integer_decompress_128: indexes must be non-decreasing in GLWE index (index %u after %u)", h_indexes[i],
                      h_indexes[i - 1]);
  }
  if (num_indexes == 0) return;
  const hipStream_t st = S0(streams);
  HX_CHECK(hipEventSynchronize(m->uploaded));  // the previous call's copy out of the staging buffer (no-op before the first)
  std::copy(h_indexes, h_indexes + num_indexes, m->h_indexes);
  HX_CHECK(hipMemcpyAsync(m->d_indexes, m->h_indexes, (size_t)num_indexes * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HX_CHECK(hipEventRecord(m->uploaded, st));
  launch_unpack_extract128(st, (uint64_t *)lwe_array_out->ptr, (const uint64_t *)packed_in, m->d_indexes, num_indexes, m->kc,
                           m->Nc, m->lwe_per_glwe, m->bits);
  // a squashed block holds two packed messages: shortint/ciphertext/squashed_noise.rs, degree msg * carry - 1
  set_block_info(lwe_array_out, 0, num_indexes, (uint64_t)m->msg * m->carry - 1, 1);
}

void hip_cleanup_integer_decompress_radix_ciphertext_128(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<Decompress128Mem>(streams, mem_ptr_void, "cleanup integer_decompress_128");
}

void hip_integer_extract_glwe_128_async(CudaStreamsFFI streams, void *glwe_out, void const *packed_in, uint32_t glwe_index,
                                        uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t lwe_per_glwe,
                                        uint32_t storage_log_modulus, uint32_t total_lwe_bodies_count) {
  first_gpu(streams);
  HX_PANIC_IF_FALSE(glwe_out && packed_in, "integer_extract_glwe_128: null pointer");
  check_compression_glwe(glwe_dimension, polynomial_size, "integer_extract_glwe_128");
  check_storage128(polynomial_size, lwe_per_glwe, storage_log_modulus, "integer_extract_glwe_128");
  HX_PANIC_IF_FALSE((uint64_t)glwe_index * lwe_per_glwe < total_lwe_bodies_count,
                    "integer_extract_glwe_128: GLWE %u of a compressed list with %u elements, out of bound access", glwe_index,
                    total_lwe_bodies_count);
  const uint32_t bodies = std::min(lwe_per_glwe, total_lwe_bodies_count - glwe_index * lwe_per_glwe);
  const size_t words64 = 2 * (size_t)pks128_words_per_glwe(glwe_dimension, polynomial_size, lwe_per_glwe, storage_log_modulus);
  launch_unpack_glwe128(S0(streams), (uint64_t *)glwe_out, (const uint64_t *)packed_in + (size_t)glwe_index * words64,
                        glwe_dimension, polynomial_size, bodies, storage_log_modulus);
}

// ---- noise squashing (integer.cuh:2776-2840; tfhe/src/integer/gpu/noise_squashing).  lwe_dimension: the small key's;
// glwe_dimension x polynomial_size: the squashing key's output ring; input_*: the compute set's ring (the big key the
// blocks are under).  num_radix_blocks: blocks of the OUTPUT (ceil(num_original_blocks / 2)).  One GPU.
// grouping_factor 0: the classic 128-bit bootstrap; otherwise the multi-bit one
static uint64_t scratch_noise_squashing(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
    uint32_t input_glwe_dimension, uint32_t input_polynomial_size, uint32_t ks_level, uint32_t ks_base_log,
    uint32_t pbs_level, uint32_t pbs_base_log, uint32_t num_radix_blocks, uint32_t num_original_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t grouping_factor) {
  HX_PANIC_IF_FALSE(num_radix_blocks == (num_original_blocks + 1) / 2,
                    "apply_noise_squashing: num output radix blocks (%u) should be half ceil the number input radix blocks (%u)",
                    num_radix_blocks, num_original_blocks);
  HX_PANIC_IF_FALSE(message_modulus >= 2 && carry_modulus >= message_modulus,
                    "apply_noise_squashing: two blocks are packed in one, so carry_modulus (=%u) must be at least "
                    "message_modulus (=%u)", carry_modulus, message_modulus);
  HX_PANIC_IF_FALSE(polynomial_size >= 2 * message_modulus * carry_modulus, "apply_noise_squashing: polynomial_size %u too small",
                    polynomial_size);
  return scratch_create<NoiseSquashMem>(streams, mem_ptr, allocate_gpu_memory, "apply_noise_squashing", [&](NoiseSquashMem &m) {
    const hipStream_t st = S0(streams);
    m.big_n = input_glwe_dimension * input_polynomial_size, m.small_n = lwe_dimension;
    m.k = glwe_dimension, m.N = polynomial_size;
    m.ks_base_log = ks_base_log, m.ks_level = ks_level, m.pbs_base_log = pbs_base_log, m.pbs_level = pbs_level;
    m.msg = message_modulus, m.carry = carry_modulus;
    m.cap_in = std::max(1u, num_original_blocks), m.cap_out = std::max(1u, num_radix_blocks);
    m.gpu = G0(streams);
    m.grouping = grouping_factor;
    m.own.alloc(m.d_packed, (size_t)m.cap_out * (m.big_n + 1) * sizeof(uint64_t));
    m.own.alloc(m.d_after_ks, (size_t)m.cap_out * (m.small_n + 1) * sizeof(uint64_t));
    std::vector<uint64_t> triv(m.cap_out), lo(m.cap_out), hi(m.cap_out);
    for (uint32_t i = 0; i < m.cap_out; ++i) triv[i] = i, lo[i] = 2 * i, hi[i] = 2 * i + 1;
    m.d_trivial = m.own.upload(st, triv);
    m.d_lo = m.own.upload(st, lo);
    m.d_hi = m.own.upload(st, hi);
    // the identity on message_modulus * carry_modulus values, encoded on 128 bits: delta = 2^127 / (msg * carry)
    const uint32_t sup = m.msg * m.carry, box = m.N / sup, half = box / 2;
    const unsigned __int128 delta = ((unsigned __int128)1 << 127) / sup;
    std::vector<unsigned __int128> lut((size_t)(m.k + 1) * m.N, 0);
    unsigned __int128 *body = lut.data() + (size_t)m.k * m.N;
    for (uint32_t i = 0; i < sup; ++i)
      for (uint32_t j = i * box; j < (i + 1) * box; ++j) body[j] = (unsigned __int128)i * delta;
    for (uint32_t i = 0; i < half; ++i) body[i] = (unsigned __int128)0 - body[i];
    std::rotate(body, body + half, body + m.N);
    m.d_lut = m.own.upload(st, lut);
    if (m.grouping)
      t_bytes += hip_scratch_multi_bit_programmable_bootstrap_128_async(st, m.gpu, &m.pbs_buf, m.k, m.N, m.pbs_level, m.cap_out,
                                                                        !t_dry);
    else
      t_bytes += hip_scratch_programmable_bootstrap_128_async(st, m.gpu, &m.pbs_buf, m.small_n, m.k, m.N, m.pbs_level, m.cap_out,
                                                              !t_dry, noise_reduction_type);
  });
}
uint64_t hip_scratch_integer_apply_noise_squashing_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
    uint32_t input_glwe_dimension, uint32_t input_polynomial_size, uint32_t ks_level, uint32_t ks_base_log,
    uint32_t pbs_level, uint32_t pbs_base_log, uint32_t num_radix_blocks, uint32_t num_original_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type) {
  return scratch_noise_squashing(streams, mem_ptr, lwe_dimension, glwe_dimension, polynomial_size, input_glwe_dimension,
                                 input_polynomial_size, ks_level, ks_base_log, pbs_level, pbs_base_log, num_radix_blocks,
                                 num_original_blocks, message_modulus, carry_modulus, allocate_gpu_memory, noise_reduction_type, 0);
}
// the squashing key is a multi-bit 128-bit key; the plain modulus switch is the only one multi-bit has
uint64_t hip_scratch_integer_apply_noise_squashing_multi_bit_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
    uint32_t input_glwe_dimension, uint32_t input_polynomial_size, uint32_t ks_level, uint32_t ks_base_log,
    uint32_t pbs_level, uint32_t pbs_base_log, uint32_t num_radix_blocks, uint32_t num_original_blocks,
    uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
    enum PBS_MS_REDUCTION_T noise_reduction_type, uint32_t grouping_factor) {
  HX_PANIC_IF_FALSE((uint32_t)noise_reduction_type == 0,
                    "apply_noise_squashing: the multi-bit bootstrap has no noise_reduction_type %u (plain modulus switch only)",
                    (uint32_t)noise_reduction_type);
  HX_PANIC_IF_FALSE(grouping_factor >= 2 && grouping_factor <= 4 && lwe_dimension >= grouping_factor &&
                        lwe_dimension % grouping_factor == 0,
                    "apply_noise_squashing: unsupported grouping_factor %u for lwe_dimension %u", grouping_factor, lwe_dimension);
  return scratch_noise_squashing(streams, mem_ptr, lwe_dimension, glwe_dimension, polynomial_size, input_glwe_dimension,
                                 input_polynomial_size, ks_level, ks_base_log, pbs_level, pbs_base_log, num_radix_blocks,
                                 num_original_blocks, message_modulus, carry_modulus, allocate_gpu_memory, noise_reduction_type,
                                 grouping_factor);
}

void hip_integer_apply_noise_squashing_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *lwe_array_out,
                                                CudaRadixCiphertextFFI const *lwe_array_in, int8_t *mem_ptr,
                                                void *const *ksks, void *const *bsks) {
  first_gpu(streams);
  auto *m = scratch_use<NoiseSquashMem>(mem_ptr, "apply_noise_squashing");
  HX_PANIC_IF_FALSE(lwe_array_out && lwe_array_out->ptr && lwe_array_in && lwe_array_in->ptr && ksks && ksks[0] && bsks && bsks[0],
                    "apply_noise_squashing: null pointer");
  const uint32_t n_in = lwe_array_in->num_radix_blocks, n_out = lwe_array_out->num_radix_blocks;
  HX_PANIC_IF_FALSE(n_out == (n_in + 1) / 2,
                    "apply_noise_squashing: num output radix blocks (%u) should be half ceil the number input radix blocks (%u)",
                    n_out, n_in);
  HX_PANIC_IF_FALSE(n_in <= m->cap_in && n_out <= m->cap_out, "apply_noise_squashing: %u blocks exceed the scratch capacity %u",
                    n_in, m->cap_in);
  HX_PANIC_IF_FALSE(lwe_array_in->lwe_dimension == m->big_n && lwe_array_out->lwe_dimension == m->k * m->N,
                    "apply_noise_squashing: lwe dimensions (%u in, %u out) differ from the scratch's (%u, %u)",
                    lwe_array_in->lwe_dimension, lwe_array_out->lwe_dimension, m->big_n, m->k * m->N);
  check_clean({lwe_array_in}, n_in, m->msg, "apply_noise_squashing", "ciphertexts must have empty carries to be squashed");
  if (n_out == 0) return;
  const hipStream_t st = S0(streams);
  const uint64_t *in = (const uint64_t *)lwe_array_in->ptr;
  const uint32_t words = m->big_n + 1, pairs = n_in / 2;
  // block 2i + message_modulus * block 2i + 1; an odd last block goes through alone
  axpy(st, m->d_packed, nullptr, in, m->d_hi, m->msg, in, m->d_lo, words, pairs);
  if (n_in & 1) axpy(st, m->d_packed + (size_t)pairs * words, nullptr, in + (size_t)(n_in - 1) * words, nullptr, 1, nullptr, nullptr, words, 1);
  launch_keyswitch(st, m->d_after_ks, m->d_trivial, m->d_packed, m->d_trivial, (const uint64_t *)ksks[0], m->big_n, m->small_n,
                   m->ks_base_log, m->ks_level, n_out);
  if (m->grouping)
    hip_multi_bit_programmable_bootstrap_128_async(st, m->gpu, lwe_array_out->ptr, m->d_trivial, m->d_lut, m->d_after_ks,
                                                   m->d_trivial, bsks[0], m->pbs_buf, m->small_n, m->k, m->N, m->grouping,
                                                   m->pbs_base_log, m->pbs_level, n_out, 1, 0);
  else
    hip_programmable_bootstrap_128_async(st, m->gpu, lwe_array_out->ptr, m->d_lut, m->d_after_ks, bsks[0], m->pbs_buf, m->small_n,
                                         m->k, m->N, m->pbs_base_log, m->pbs_level, n_out);
  set_block_info(lwe_array_out, 0, n_out, (uint64_t)m->msg * m->msg - 1, 1);
}

void hip_cleanup_integer_apply_noise_squashing_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<NoiseSquashMem>(streams, mem_ptr_void, "cleanup apply_noise_squashing");
}

// ---- cuda/include/zk/zk.h:10-27, under hip_ names (the reference-named symbols stay link stubs) -----------------------
// n_c = casting_ksk_params.input_lwe_dimension.  Outputs of every kind but NO_CASTING have dimension glwe_dimension *
// polynomial_size (the reference sizes them by the casting key's larger dimension, the same number in its sets).
uint64_t hip_scratch_expand_without_verification_64_async(
    CudaStreamsFFI streams, int8_t **mem_ptr, uint32_t glwe_dimension, uint32_t polynomial_size,
    CudaLweKeyswitchKeyParamsFFI computing_ksk_params, CudaLweKeyswitchKeyParamsFFI casting_ksk_params, uint32_t pbs_level,
    uint32_t pbs_base_log, uint32_t grouping_factor, const uint32_t *num_lwes_per_compact_list, const bool *is_boolean_array,
    const uint32_t is_boolean_array_len, uint32_t num_compact_lists, uint32_t message_modulus, uint32_t carry_modulus,
    enum PBS_TYPE pbs_type, enum KS_TYPE casting_key_type, bool allocate_gpu_memory, enum EXPAND_KIND expand_kind,
    enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const char *who = "expand_without_verification";
  const uint32_t kind = (uint32_t)expand_kind, ks_type = (uint32_t)casting_key_type;
  const uint32_t n_c = casting_ksk_params.input_lwe_dimension;
  HX_PANIC_IF_FALSE(kind == NO_CASTING || kind == CASTING || kind == SANITY_CHECK, "%s: unknown expand kind %u", who, kind);
  HX_PANIC_IF_FALSE(ks_type == BIG_TO_SMALL || ks_type == SMALL_TO_BIG, "%s: unknown casting key type %u", who, ks_type);
  HX_PANIC_IF_FALSE(num_compact_lists >= 1 && num_lwes_per_compact_list != nullptr, "%s: no compact list to expand", who);
  HX_PANIC_IF_FALSE(n_c >= 1 && n_c <= kExpandMaxDimension, "%s: unsupported compact list dimension %u", who, n_c);
  uint64_t total = 0;
  for (uint32_t l = 0; l < num_compact_lists; ++l) {
    const uint32_t c = num_lwes_per_compact_list[l];
    HX_PANIC_IF_FALSE(c >= 1 && c <= n_c,
                      "%s: compact list %u holds %u bodies, a list holds 1 .. %u (the casting key's input dimension)", who, l,
                      c, n_c);
    total += c;
  }
  HX_PANIC_IF_FALSE(total >= 1 && 2 * total <= 0xFFFFFFFFull, "%s: %llu bodies in all", who, (unsigned long long)total);
  const uint32_t num_lwes = (uint32_t)total;
  Params p{};
  if (kind != NO_CASTING) {
    HX_PANIC_IF_FALSE(kind != SANITY_CHECK || ks_type == BIG_TO_SMALL, "%s: SANITY_CHECK not supported for SMALL_TO_BIG casting",
                      who);
    HX_PANIC_IF_FALSE(kind != CASTING || carry_modulus == message_modulus,
                      "%s: GPU backend requires carry_modulus equal to message_modulus (got %u, %u)", who, carry_modulus,
                      message_modulus);
    HX_PANIC_IF_FALSE(is_boolean_array != nullptr && is_boolean_array_len >= 2 * num_lwes,
                      "%s: is_boolean_array holds %u entries, 2 * %u bodies need %u (pad it with false)", who,
                      is_boolean_array_len, num_lwes, 2 * num_lwes);
    const uint32_t big_n = glwe_dimension * polynomial_size;
    // BIG_TO_SMALL: the casting key IS the round's keyswitch key; SMALL_TO_BIG: a keyswitch of its own, then the computing key
    const CudaLweKeyswitchKeyParamsFFI round_ksk = ks_type == BIG_TO_SMALL ? casting_ksk_params : computing_ksk_params;
    HX_PANIC_IF_FALSE(ks_type == BIG_TO_SMALL || (casting_ksk_params.output_lwe_dimension == big_n &&
                                                  computing_ksk_params.input_lwe_dimension == big_n),
                      "%s: a SMALL_TO_BIG casting key ends on the big compute key (%u), where the computing keyswitch key starts",
                      who, big_n);
    CudaLweBootstrapKeyParamsFFI b{round_ksk.output_lwe_dimension, glwe_dimension, polynomial_size, pbs_base_log, pbs_level,
                                   big_n, (uint32_t)pbs_type, grouping_factor};
    // (make_params ties the keyswitch key's INPUT to the big key; here the round's input dimension is the driver's in_n)
    CudaLweKeyswitchKeyParamsFFI k{big_n, round_ksk.output_lwe_dimension, round_ksk.base_log, round_ksk.level_count};
    p = make_params(b, k, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  }
  return scratch_create<ExpandMem>(streams, mem_ptr, allocate_gpu_memory, who, [&](ExpandMem &m) {
    const hipStream_t st = S0(streams);
    m.kind = kind, m.ks_type = ks_type, m.n_c = n_c, m.num_lwes = num_lwes, m.gpu = G0(streams);
    std::vector<ExpandJob> jobs;
    jobs.reserve(num_lwes);
    uint64_t at = 0;
    for (uint32_t l = 0; l < num_compact_lists; ++l) {
      for (uint32_t d = 0; d < num_lwes_per_compact_list[l]; ++d) jobs.push_back(ExpandJob{at, d, 0});
      at += (uint64_t)n_c + num_lwes_per_compact_list[l];
    }
    m.d_jobs = m.own.upload(st, jobs);
    if (kind == NO_CASTING) return;
    // zk_utilities.h:190-230,283-300: per list of c bodies first the c message extractions, then the c carry extractions;
    // output 2i is the message block of body i, 2i + 1 its carry block; a boolean output takes the sanitising table
    const uint32_t blocks = 2 * num_lwes;
    std::vector<uint64_t> in_idx(blocks), out_idx(blocks), lut_idx(blocks);
    uint32_t offset = 0;
    for (uint32_t l = 0; l < num_compact_lists; ++l) {
      const uint32_t c = num_lwes_per_compact_list[l];
      for (uint32_t i = 0; i < 2 * c; ++i) {
        const uint32_t q = i + 2 * offset, half = i / c;
        in_idx[q] = i % c + offset;
        out_idx[q] = 2 * in_idx[q] + half;
        lut_idx[q] = kind == SANITY_CHECK ? 0 : half + (is_boolean_array[out_idx[q]] ? 2 : 0);
      }
      offset += c;
    }
    m.d_in_idx = m.own.upload(st, in_idx);
    m.d_out_idx = m.own.upload(st, out_idx);
    m.d_lut_idx = m.own.upload(st, lut_idx);
    const uint64_t msg = p.msg, carry = p.carry;
    std::vector<std::function<uint64_t(uint64_t)>> fs;
    if (kind == SANITY_CHECK) {
      fs = {[](uint64_t x) { return x; }};
    } else {  // (x / carry_modulus only splits the packed value because carry == message, as the reference has it)
      fs = {[=](uint64_t x) { return x % msg; }, [=](uint64_t x) { return (x / carry) % msg; },
            [=](uint64_t x) { return (uint64_t)(x % msg != 0); }, [=](uint64_t x) { return (uint64_t)((x / carry) % msg != 0); }};
    }
    std::vector<std::vector<uint64_t>> luts(fs.size(), std::vector<uint64_t>((size_t)(p.k + 1) * p.N));
    for (size_t t = 0; t < fs.size(); ++t) generate_lut(p, luts[t].data(), fs[t]);
    m.own.alloc(m.d_expanded, (size_t)num_lwes * ((size_t)n_c + 1) * sizeof(uint64_t));
    if (ks_type == SMALL_TO_BIG) {
      m.cast_out_n = casting_ksk_params.output_lwe_dimension;
      m.cast_base_log = casting_ksk_params.base_log, m.cast_level = casting_ksk_params.level_count;
      m.own.alloc(m.d_cast, (size_t)num_lwes * ((size_t)m.cast_out_n + 1) * sizeof(uint64_t));
    }
    m.drv.init(streams, p, blocks, luts, 1, ks_type == BIG_TO_SMALL ? n_c : 0);
  });
}

void hip_expand_without_verification_64_async(CudaStreamsFFI streams, void *lwe_array_out,
                                              const void *lwe_flattened_compact_array_in, int8_t *mem_ptr, void *const *bsks,
                                              void *const *computing_ksks, void *const *casting_keys) {
  first_gpu(streams);
  auto *m = scratch_use<ExpandMem>(mem_ptr, "expand_without_verification");
  HX_PANIC_IF_FALSE(lwe_array_out != nullptr && lwe_flattened_compact_array_in != nullptr,
                    "expand_without_verification: null pointer");
  const hipStream_t st = S0(streams);
  const uint64_t *in = (const uint64_t *)lwe_flattened_compact_array_in;
  if (m->kind == NO_CASTING) {
    HX_RANGE("expand (%u lwes)", m->num_lwes);
    launch_lwe_expand(st, (uint64_t *)lwe_array_out, in, m->d_jobs, m->n_c, m->num_lwes);
    return;
  }
  const bool to_big = m->ks_type == SMALL_TO_BIG;
  HX_PANIC_IF_FALSE(bsks && casting_keys && casting_keys[0] && (!to_big || computing_ksks),
                    "expand_without_verification: null key pointer");
  {
    HX_RANGE("expand (%u lwes)", m->num_lwes);
    launch_lwe_expand(st, m->d_expanded, in, m->d_jobs, m->n_c, m->num_lwes);
  }
  if (to_big) {
    HX_RANGE("casting keyswitch (%u lwes)", m->num_lwes);
    const uint64_t *triv = m->drv.gpus[0].d_trivial;  // 0 .. 2 * num_lwes - 1
    cuda_keyswitch_lwe_ciphertext_vector_64_64_async(st, m->gpu, m->d_cast, triv, m->d_expanded, triv, casting_keys[0], m->n_c,
                                                     m->cast_out_n, m->cast_base_log, m->cast_level, m->num_lwes);
  }
  HX_RANGE("message and carry extraction (%u blocks)", 2 * m->num_lwes);
  m->drv.round(streams, (uint64_t *)lwe_array_out, m->d_out_idx, to_big ? m->d_cast : m->d_expanded, m->d_in_idx, m->d_lut_idx,
               2 * m->num_lwes, to_big ? computing_ksks : casting_keys, bsks);
}

void hip_cleanup_expand_without_verification_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<ExpandMem>(streams, mem_ptr_void, "cleanup expand_without_verification");
}

// ---- cuda/include/integer/rerand.h:6-19, under hip_ names (the reference-named symbols stay link stubs) --------------
// The zeros are ONE compact list under a key of dimension ksk_params.input_lwe_dimension.  RERAND_WITHOUT_KS: the blocks
// are under that key too; the other three fields of ksk_params are not read (the reference's caller passes zeros).
// RERAND_WITH_KS: the blocks are under ksk_params.output_lwe_dimension — the reference files the two dimensions as
// "big" and "small" of its radix parameters (rerand.cu:12-16), whatever their order: "small" here is the compute key's
// dimension, usually the larger one.
uint64_t hip_scratch_rerand_64_async(CudaStreamsFFI streams, int8_t **mem_ptr, CudaLweKeyswitchKeyParamsFFI ksk_params,
                                     uint32_t lwe_ciphertext_count, uint32_t message_modulus, uint32_t carry_modulus,
                                     bool allocate_gpu_memory, enum RERAND_MODE rerand_type) {
  const char *who = "rerand";
  const uint32_t mode = (uint32_t)rerand_type, n_in = ksk_params.input_lwe_dimension, count = lwe_ciphertext_count;
  HX_PANIC_IF_FALSE(mode == RERAND_WITH_KS || mode == RERAND_WITHOUT_KS, "%s: unknown re-randomisation mode %u", who, mode);
  HX_PANIC_IF_FALSE(message_modulus >= 2 && carry_modulus >= 1, "%s: unsupported message/carry moduli (%u, %u)", who,
                    message_modulus, carry_modulus);
  HX_PANIC_IF_FALSE(n_in >= 1 && n_in <= kExpandMaxDimension, "%s: unsupported dimension %u of the encryptions of zero", who,
                    n_in);
  HX_PANIC_IF_FALSE(count >= 1, "%s: no ciphertext to re-randomise (lwe_ciphertext_count is 0)", who);
  HX_PANIC_IF_FALSE(count <= n_in,
                    "%s: %u ciphertexts, one compact list of encryptions of zero holds 1 .. %u bodies (its dimension)", who,
                    count, n_in);
  if (mode == RERAND_WITH_KS)
    HX_PANIC_IF_FALSE(ksk_params.output_lwe_dimension >= 1 && ksk_params.level_count >= 1 && ksk_params.base_log >= 1,
                      "%s: RERAND_WITH_KS needs the keyswitch key's output dimension and decomposition", who);
  return scratch_create<RerandMem>(streams, mem_ptr, allocate_gpu_memory, who, [&](RerandMem &m) {
    m.mode = mode, m.n_in = n_in, m.count = count, m.gpu = G0(streams);
    if (mode == RERAND_WITHOUT_KS) return;  // rotate and add in place: nothing on the device
    const hipStream_t st = S0(streams);
    m.n_out = ksk_params.output_lwe_dimension, m.base_log = ksk_params.base_log, m.level = ksk_params.level_count;
    std::vector<ExpandJob> jobs(count);
    std::vector<uint64_t> triv(count);
    for (uint32_t o = 0; o < count; ++o) jobs[o] = ExpandJob{0, o, 0}, triv[o] = o;
    m.d_jobs = m.own.upload(st, jobs);
    m.d_trivial = m.own.upload(st, triv);
    m.own.alloc(m.d_expanded, (size_t)count * ((size_t)n_in + 1) * sizeof(uint64_t));
    m.own.alloc(m.d_switched, (size_t)count * ((size_t)m.n_out + 1) * sizeof(uint64_t));
  });
}

void hip_rerand_64_async(CudaStreamsFFI streams, void *lwe_array,
                         const void *lwe_flattened_encryptions_of_zero_compact_array_in, int8_t *mem_ptr,
                         void *const *ksk) {
  first_gpu(streams);
  auto *m = scratch_use<RerandMem>(mem_ptr, "rerand");
  HX_PANIC_IF_FALSE(lwe_array != nullptr && lwe_flattened_encryptions_of_zero_compact_array_in != nullptr,
                    "rerand: null pointer");
  const hipStream_t st = S0(streams);
  const uint64_t *zeros = (const uint64_t *)lwe_flattened_encryptions_of_zero_compact_array_in;
  if (m->mode == RERAND_WITHOUT_KS) {
    HX_RANGE("rerand: rotate and add (%u blocks)", m->count);
    launch_lwe_rerand_add(st, (uint64_t *)lwe_array, zeros, m->n_in, m->count);
    return;
  }
  HX_PANIC_IF_FALSE(ksk != nullptr && ksk[0] != nullptr, "rerand: RERAND_WITH_KS without a keyswitch key (null pointer)");
  {
    HX_RANGE("rerand: expand (%u zeros)", m->count);
    launch_lwe_expand(st, m->d_expanded, zeros, m->d_jobs, m->n_in, m->count);
  }
  {
    HX_RANGE("rerand: keyswitch (%u zeros)", m->count);
    cuda_keyswitch_lwe_ciphertext_vector_64_64_async(st, m->gpu, m->d_switched, m->d_trivial, m->d_expanded, m->d_trivial,
                                                     ksk[0], m->n_in, m->n_out, m->base_log, m->level, m->count);
  }
  HX_RANGE("rerand: add (%u blocks)", m->count);
  launch_lwe_add_rows(st, (uint64_t *)lwe_array, m->d_switched, m->n_out + 1, m->count);
}

void hip_cleanup_rerand_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<RerandMem>(streams, mem_ptr_void, "cleanup rerand");
}

// ---- cuda/include/integer/integer.h:664-678, under hip_ names (the reference-named symbols stay link stubs) ----------
// ksk_params is part of the reference's parameter list and, as there, takes no part: no keyswitch runs.
uint64_t hip_scratch_integer_grouped_oprf_64_async(CudaStreamsFFI streams, int8_t **mem_ptr,
                                                   CudaLweBootstrapKeyParamsFFI bsk_params,
                                                   CudaLweKeyswitchKeyParamsFFI ksk_params, uint32_t num_blocks_to_process,
                                                   uint32_t message_modulus, uint32_t carry_modulus, bool allocate_gpu_memory,
                                                   uint32_t total_random_bits, enum PBS_MS_REDUCTION_T noise_reduction_type) {
  const char *who = "integer_grouped_oprf";
  (void)ksk_params;
  HX_PANIC_IF_FALSE(message_modulus >= 2 && (message_modulus & (message_modulus - 1)) == 0 && carry_modulus >= 1 &&
                        (carry_modulus & (carry_modulus - 1)) == 0,
                    "%s: message and carry moduli must be powers of two (got %u, %u)", who, message_modulus, carry_modulus);
  uint32_t message_bits = 0, carry_bits = 0;
  while ((1u << (message_bits + 1)) <= message_modulus) ++message_bits;
  while ((1u << (carry_bits + 1)) <= carry_modulus) ++carry_bits;
  // oprf.h:27-34
  const uint32_t wanted = (total_random_bits + message_bits - 1) / message_bits;
  HX_PANIC_IF_FALSE(num_blocks_to_process >= 1 && num_blocks_to_process == wanted,
                    "%s: num_blocks_to_process (%u) should be equal to ceil(total_random_bits / message bits) = ceil(%u / %u) "
                    "= %u",
                    who, num_blocks_to_process, total_random_bits, message_bits, wanted);
  // no keyswitch in front of this bootstrap: the key parameters below only restate the bootstrap's own dimensions
  const CudaLweKeyswitchKeyParamsFFI no_ks{bsk_params.glwe_dimension * bsk_params.polynomial_size,
                                           bsk_params.input_lwe_dimension, 1, 1};
  const Params p = make_params(bsk_params, no_ks, message_modulus, carry_modulus, (uint32_t)noise_reduction_type);
  HX_PANIC_IF_FALSE(2ull * p.N >= message_modulus, "%s: 2 * polynomial_size should not be smaller than the message modulus", who);
  const uint64_t delta = (uint64_t)1 << (64 - 1 - carry_bits - message_bits);
  return scratch_create<OprfMem>(streams, mem_ptr, allocate_gpu_memory, who, [&](OprfMem &m) {
    const hipStream_t st = S0(streams);
    m.num_blocks = num_blocks_to_process, m.gpu = G0(streams);
    // oprf.rs generate_oprf_lut, integer.cuh generate_lookup_table_no_encoding: coefficient x of the body holds f(x)
    std::vector<std::vector<uint64_t>> luts(message_bits, std::vector<uint64_t>((size_t)(p.k + 1) * p.N, 0));
    for (uint32_t b = 1; b <= message_bits; ++b) {
      const uint64_t poly_delta = 2ull * p.N >> b;
      uint64_t *body = luts[b - 1].data() + (size_t)p.k * p.N;
      for (uint32_t x = 0; x < p.N; ++x) body[x] = (2 * (x / poly_delta) + 1) * delta / 2;
    }
    std::vector<uint64_t> lut_idx(m.num_blocks), corrections(m.num_blocks);
    m.bits.resize(m.num_blocks);
    uint32_t processed = 0;
    for (uint32_t i = 0; i < m.num_blocks; ++i) {
      m.bits[i] = std::min(message_bits, total_random_bits - processed);
      lut_idx[i] = m.bits[i] - 1;
      corrections[i] = (((uint64_t)1 << m.bits[i]) - 1) * delta / 2;
      processed += m.bits[i];
    }
    m.d_lut_idx = m.own.upload(st, lut_idx);
    m.d_corrections = m.own.upload(st, corrections);
    m.drv.init(streams, p, m.num_blocks, luts, 1, 0, true);
  });
}

void hip_integer_grouped_oprf_64_async(CudaStreamsFFI streams, CudaRadixCiphertextFFI *radix_lwe_out,
                                       const void *seeded_lwe_input, uint32_t num_blocks_to_process, int8_t *mem,
                                       void *const *bsks) {
  first_gpu(streams);
  auto *m = scratch_use<OprfMem>(mem, "integer_grouped_oprf");
  HX_PANIC_IF_FALSE(radix_lwe_out && radix_lwe_out->ptr && seeded_lwe_input && bsks && bsks[0],
                    "integer_grouped_oprf: null pointer");
  const Params &p = m->drv.p;
  HX_PANIC_IF_FALSE(num_blocks_to_process == m->num_blocks,
                    "integer_grouped_oprf: %u blocks to process on a scratch created for %u", num_blocks_to_process,
                    m->num_blocks);
  HX_PANIC_IF_FALSE(radix_lwe_out->lwe_dimension == p.big_n && radix_lwe_out->num_radix_blocks >= m->num_blocks,
                    "integer_grouped_oprf: output of %u blocks of lwe dimension %u, the bootstrap writes %u blocks of %u",
                    radix_lwe_out->num_radix_blocks, radix_lwe_out->lwe_dimension, m->num_blocks, p.big_n);
  uint64_t *out = (uint64_t *)radix_lwe_out->ptr;
  m->drv.round(streams, out, nullptr, (const uint64_t *)seeded_lwe_input, nullptr, m->d_lut_idx, m->num_blocks, nullptr,
               bsks);
  HX_LAUNCH(lwe_body_add_scalars_kernel, dim3((m->num_blocks + 255) / 256), dim3(256), 0, S0(streams), out, m->d_corrections,
            p.big_n + 1, m->num_blocks, (uint64_t)1);
  // oprf.cuh:82-86: the degree is p - 1, not the table's
  for (uint32_t i = 0; i < m->num_blocks; ++i) set_block_info(radix_lwe_out, i, 1, ((uint64_t)1 << m->bits[i]) - 1, 1);
}

void hip_cleanup_integer_grouped_oprf_64(CudaStreamsFFI streams, int8_t **mem_ptr_void) {
  scratch_destroy<OprfMem>(streams, mem_ptr_void, "cleanup integer_grouped_oprf");
}

}  // extern "C"

// The kernels and launchers of the 128-bit packing keyswitch (declared in pks128.h): a header, as pbs128.h is for abi.hip,
// because the host emulation build lists its translation units by name.
#include "pks128_kernels.h"
