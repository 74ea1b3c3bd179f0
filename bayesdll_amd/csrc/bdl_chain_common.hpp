// bdl_chain_common.hpp — what the stacked-chain units (bdl_diag, bdl_clip,
// bdl_chain_step, bdl_stats, bdl_ess, bdl_lowp) and bdl_api.hip share beyond
// bdl_kernels.hpp: guarded float4 access, the fp64 wave sum, the extreme-value
// summary reduction, and the host entry points' validation and launch
// helpers.  The step kernel families do not include it.
//
// Every reduction here has ONE order, and a unit's values depend on it: the
// butterflies go off = 32, 16, .., 1; block_combine starts from wave 0's value
// and adds waves 1..3 (the fp64 block sums of bdl_clip.hip and bdl_api.hip
// start from 0.0 and add waves 0..3); a finalize thread takes partials t,
// t + 256, ...
#pragma once
#include "bdl_kernels.hpp"

namespace bdl {

// ------------------------------------------------------------------- device
// Float4 group at element e.  GUARD: it may be the partial last group
// (element-wise past the last full group; never past n).
template <bool GUARD>
__device__ __forceinline__ f4v gload(const float* __restrict__ p, int64_t e, int64_t n) {
  if constexpr (GUARD)
    return ld4(p, e, n);
  else
    return vload(p + e);
}

template <bool GUARD>
__device__ __forceinline__ void gstore(float* __restrict__ p, int64_t e, int64_t n, f4v v) {
  if constexpr (GUARD)
    st4(p, e, n, v);
  else
    vstore(p + e, v);
}

// The workgroup of a (blocks_per_chain, K) grid's chain that starts segment i
// (and owns its head / tail): rotated, so that a table of many small tensors
// does not pile up on workgroup 0.
__device__ __forceinline__ uint32_t rotated_block(int i) {
  return (blockIdx.x + gridDim.x - (uint32_t)i % gridDim.x) % gridDim.x;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// A lane's / wave's / block's summary of the evaluated values of a sweep: three
// counters, the hits of three thresholds, an fp64 sum and the extreme (MAX: the
// maximum, else the minimum) with its element index.  Empty: ext is -1 for the
// maximum (every evaluated value is >= 0) and +Inf for the minimum (every
// evaluated value is finite), arg is INT64_MAX, so `combine` needs no special
// case.
template <bool MAX>
struct Extreme {
  int64_t n_eval, n_deg, n_nonf, hit0, hit1, hit2, arg;
  double sum;
  float ext;

  static __device__ __forceinline__ Extreme empty() {
    Extreme s;
    s.n_eval = s.n_deg = s.n_nonf = s.hit0 = s.hit1 = s.hit2 = 0;
    s.arg = INT64_MAX;
    s.sum = 0.0;
    s.ext = MAX ? -1.0f : __builtin_inff();
    return s;
  }

  // x is beyond y: it hits y as a threshold, it replaces y as the extreme
  static __device__ __forceinline__ bool beyond(float x, float y) { return MAX ? x > y : x < y; }
};

// the better extreme wins, the lower index among equals
template <bool MAX>
__device__ __forceinline__ Extreme<MAX> combine(Extreme<MAX> a, const Extreme<MAX>& b) {
  a.n_eval += b.n_eval;
  a.n_deg += b.n_deg;
  a.n_nonf += b.n_nonf;
  a.hit0 += b.hit0;
  a.hit1 += b.hit1;
  a.hit2 += b.hit2;
  a.sum += b.sum;
  if ((MAX ? b.ext > a.ext : b.ext < a.ext) || (b.ext == a.ext && b.arg < a.arg)) {
    a.ext = b.ext;
    a.arg = b.arg;
  }
  return a;
}

template <bool MAX>
__device__ __forceinline__ Extreme<MAX> wave_combine(Extreme<MAX> s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Extreme<MAX> o;
    o.n_eval = __shfl_xor(s.n_eval, off, 64);
    o.n_deg = __shfl_xor(s.n_deg, off, 64);
    o.n_nonf = __shfl_xor(s.n_nonf, off, 64);
    o.hit0 = __shfl_xor(s.hit0, off, 64);
    o.hit1 = __shfl_xor(s.hit1, off, 64);
    o.hit2 = __shfl_xor(s.hit2, off, 64);
    o.arg = __shfl_xor(s.arg, off, 64);
    o.sum = __shfl_xor(s.sum, off, 64);
    o.ext = __shfl_xor(s.ext, off, 64);
    // both partners must form the same value: the lower lane's first
    s = (threadIdx.x & off) ? combine(o, s) : combine(s, o);
  }
  return s;
}

// The block's summary in thread 0 (4 waves through LDS, in wave order).
template <bool MAX>
__device__ __forceinline__ Extreme<MAX> block_combine(Extreme<MAX> s) {
  __shared__ Extreme<MAX> s_wave[kBlock / 64];
  s = wave_combine(s);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) s = combine(s, s_wave[w]);
  }
  return s;
}

// One value that was evaluated (finite) at element idx.  A lane's elements
// ascend: the strict comparison keeps the lowest index.
template <bool MAX>
__device__ __forceinline__ void count_value(Extreme<MAX>& s, float x, int64_t idx, float thr0,
                                            float thr1, float thr2) {
  ++s.n_eval;
  s.sum += (double)x;
  s.hit0 += Extreme<MAX>::beyond(x, thr0);
  s.hit1 += Extreme<MAX>::beyond(x, thr1);
  s.hit2 += Extreme<MAX>::beyond(x, thr2);
  if (Extreme<MAX>::beyond(x, s.ext)) {
    s.ext = x;
    s.arg = idx;
  }
}

// A workspace of these units: the summary, padded to kPartialsOffset bytes,
// then one partial per workgroup of the sweep.
constexpr int64_t kPartialsOffset = 128;

template <class Summary>
Summary* partials_of(void* workspace) {
  return reinterpret_cast<Summary*>(reinterpret_cast<char*>(workspace) + kPartialsOffset);
}

// The sweep's last step: the block's summary into its partial.  A: the unit's
// adapter between its public summary struct and Extreme, with
//   static constexpr bool kMax;
//   static Extreme<kMax> load(const Summary&);  static void store(Summary*, const Extreme<kMax>&);
template <class A, class Summary>
__device__ __forceinline__ void store_partial(Summary* __restrict__ partials,
                                              Extreme<A::kMax> s) {
  s = block_combine(s);
  if (threadIdx.x == 0) A::store(partials + blockIdx.x, s);
}

// One workgroup: the partials in a fixed order (thread t takes t, t + 256,
// ...; then the wave butterfly and the waves in order), the empty case's
// reported conventions (0.0 at index -1), the summary.
template <class A, class Summary>
__device__ __forceinline__ void finalize_summary(const Summary* __restrict__ partials, int nparts,
                                                 Summary* __restrict__ out) {
  Extreme<A::kMax> s = Extreme<A::kMax>::empty();
  for (int i = threadIdx.x; i < nparts; i += kBlock) s = combine(s, A::load(partials[i]));
  s = block_combine(s);
  if (threadIdx.x == 0) {
    if (s.n_eval == 0) {
      s.ext = 0.0f;
      s.arg = -1;
    }
    A::store(out, s);
  }
}

// --------------------------------------------------------------------- host
// bdl_api.hip
void set_last_error(const std::string& msg);
bool graph_redirect_active();
int cu_count();

inline int fail(int code, const std::string& msg) {
  set_last_error(msg);
  return code;
}

// null: no vector, never misaligned
inline bool misaligned(const void* p, uintptr_t mask) {
  return (reinterpret_cast<uintptr_t>(p) & mask) != 0;
}

// [a, a + abytes) and [b, b + bbytes) share a byte (null: no vector)
inline bool overlap(const void* a, const void* b, uint64_t abytes, uint64_t bbytes) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y ? y - x < abytes : x - y < bbytes;
}

// While a graph redirect is set, every launching entry point but
// bdl_sgmcmc_step refuses: its launches would go to the stream, mixed with node
// rewrites.
inline int no_redirect(const char* what) {
  if (!graph_redirect_active()) return BDL_OK;
  return fail(BDL_ERR_ARG, std::string(what) + ": a graph redirect is active (bdl_graph_redirect); "
              "only bdl_sgmcmc_step rewrites a node");
}

// After an entry point's launches.
inline int launched(const char* what) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return BDL_OK;
  return fail(BDL_ERR_LAUNCH, std::string(what) + ": launch failed: " + hipGetErrorString(err));
}

// What is wrong with the slots of a stacked layout (`chains` >= 1 of them,
// 4 * chain_groups elements each, n >= 1 used); nullptr: fine.  A unit checks
// its own range of chains and n first, in its own words.
inline const char* stacked_slot_error(int32_t chains, int64_t n, uint64_t chain_groups) {
  // every element index 4*chain_groups*k + j must fit the signed 64-bit index
  if (chain_groups > (uint64_t)(INT64_MAX / 4) / (uint64_t)chains)
    return "chains * chain_groups overflows the element index";
  if ((uint64_t)n > 4 * chain_groups) return "n exceeds the chain slot (4 * chain_groups)";
  return nullptr;
}

// Block iterations of per_iter float4 groups that cover n elements.
inline int64_t block_iters(int64_t n, int64_t per_iter) {
  return ((n + 3) / 4 + per_iter - 1) / per_iter;
}

// A grid for `want` workgroups of work under a cap; never empty.
inline int64_t capped_grid(int64_t want, int64_t cap) {
  return std::max<int64_t>(1, std::min(want, cap));
}

// The (blocks_per_chain, K) grids' default: per_cu workgroups per CU over all
// chains, at most `limit` per chain.
inline int64_t blocks_per_chain(int per_cu, int32_t chains, int64_t limit) {
  return capped_grid(((int64_t)cu_count() * per_cu + chains - 1) / chains, limit);
}

}  // namespace bdl
