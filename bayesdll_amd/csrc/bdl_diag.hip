// bdl_diag.hip — cross-chain R-hat and pooled posterior of stacked chains
// (include/bdl_diag.h: the arithmetic, the conventions, the summary).
//
// One sweep over the K chains' stacked (mom1, mom2): a lane owns one float4
// group of elements and walks the chains, K read streams a chain slot apart
// (non-temporal 16-B loads, the chain loop unrolled by 4 so eight loads are in
// flight per lane), then finishes its four elements (six IEEE divisions and a
// square root per element, none per chain) and stores the requested outputs.
// The summary is reduced like the clip norm (bdl_api.hip): per-lane
// accumulators, a 64-lane butterfly, the block's 4 waves through LDS, one
// partial per workgroup written with ordinary stores, and a one-workgroup
// launch that combines the partials in a fixed order.  No atomics, no host
// synchronisation, no allocation.
#include "bdl_kernels.hpp"
#include "bdl_diag.h"

namespace bdl {

// bdl_api.hip
void set_last_error(const std::string& msg);
bool graph_redirect_active();
int cu_count();

namespace {

constexpr int kMaxDiagPartials = 2048;   // 256 CUs x 8 workgroups
constexpr int64_t kPartialsOffset = 128; // the summary, padded; then the partials
constexpr int kDiagBpc = 2;              // default workgroups per CU, as the posterior draw

int fail(int code, const std::string& msg) {
  set_last_error(msg);
  return code;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

struct DArgs {
  const float* __restrict__ mom1;
  const float* __restrict__ mom2;
  float* __restrict__ pooled_mean;
  float* __restrict__ pooled_var;
  float* __restrict__ rhat;
  bdl_diag_summary* __restrict__ partials;
  int64_t n;
  int64_t slot;  // elements per chain slot, 4 * chain_groups
  int32_t chains;
  float ratio, inv_ratio, var_floor, c1;
  float fk, fkm1;  // K and K - 1 as fp32
  float thr0, thr1, thr2;
};

// A lane's / wave's / block's statistics.  Empty: mx = -1 (every evaluated
// rhat is >= 0) and argmax = INT64_MAX, so `combine` needs no special case.
struct Stat {
  int64_t n_eval, n_deg, n_nonf, above0, above1, above2, argmax;
  double sum;
  float mx;
};

__device__ __forceinline__ Stat stat_empty() {
  Stat s;
  s.n_eval = s.n_deg = s.n_nonf = s.above0 = s.above1 = s.above2 = 0;
  s.argmax = INT64_MAX;
  s.sum = 0.0;
  s.mx = -1.0f;
  return s;
}

// the larger maximum wins, the lower index among equals
__device__ __forceinline__ Stat combine(Stat a, const Stat& b) {
  a.n_eval += b.n_eval;
  a.n_deg += b.n_deg;
  a.n_nonf += b.n_nonf;
  a.above0 += b.above0;
  a.above1 += b.above1;
  a.above2 += b.above2;
  a.sum += b.sum;
  if (b.mx > a.mx || (b.mx == a.mx && b.argmax < a.argmax)) {
    a.mx = b.mx;
    a.argmax = b.argmax;
  }
  return a;
}

__device__ __forceinline__ Stat wave_combine(Stat s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Stat o;
    o.n_eval = __shfl_xor(s.n_eval, off, 64);
    o.n_deg = __shfl_xor(s.n_deg, off, 64);
    o.n_nonf = __shfl_xor(s.n_nonf, off, 64);
    o.above0 = __shfl_xor(s.above0, off, 64);
    o.above1 = __shfl_xor(s.above1, off, 64);
    o.above2 = __shfl_xor(s.above2, off, 64);
    o.argmax = __shfl_xor(s.argmax, off, 64);
    o.sum = __shfl_xor(s.sum, off, 64);
    o.mx = __shfl_xor(s.mx, off, 64);
    // both partners must form the same value: the lower lane's first
    s = (threadIdx.x & off) ? combine(o, s) : combine(s, o);
  }
  return s;
}

// The block's statistics in thread 0 (4 waves through LDS, in wave order).
__device__ __forceinline__ Stat block_combine(Stat s) {
  __shared__ Stat s_wave[kBlock / 64];
  s = wave_combine(s);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) s = combine(s, s_wave[w]);
  }
  return s;
}

__device__ __forceinline__ void store_stat(bdl_diag_summary* __restrict__ out, const Stat& s) {
  out->n_eval = s.n_eval;
  out->n_degenerate = s.n_deg;
  out->n_nonfinite = s.n_nonf;
  out->argmax = s.argmax;
  out->n_above[0] = s.above0;
  out->n_above[1] = s.above1;
  out->n_above[2] = s.above2;
  out->rhat_sum = s.sum;
  out->rhat_max = s.mx;
  out->pad = 0.0f;
}

// One chain's contribution to a group's running sums (include/bdl_diag.h).
template <int VAR, bool RECIP>
__device__ __forceinline__ void accum4(const DArgs& a, const f4v m0, const f4v m, const f4v q,
                                       f4v& S1, f4v& S2, f4v& SW) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float d = m[j] - m0[j];
    S1[j] = S1[j] + d;
    const float t = d * d;
    S2[j] = S2[j] + t;
    SW[j] = SW[j] + posterior_var<VAR, RECIP>(m[j], q[j], a.ratio, a.inv_ratio, a.var_floor);
  }
}

// One element from its sums: outputs and the lane's statistics.
__device__ __forceinline__ void finish_elem(const DArgs& a, float m0, float S1, float S2, float SW,
                                            int64_t idx, float& pm, float& pv, float& rh, Stat& s) {
  const float q = S1 / a.fk;
  pm = m0 + q;
  const float p = S1 * S1;
  const float r = p / a.fk;
  const float u = S2 - r;
  const float ss = u < 0.0f ? 0.0f : u;
  const float Bn = ss / a.fkm1;
  const float W = SW / a.fk;
  const float wa = W * a.c1;
  const float b = wa + Bn;
  const float c = b / W;
  const float rhat = sqrtf(c);
  const float e = ss / a.fk;
  pv = W + e;
  if (S2 == 0.0f) {
    rh = __builtin_nanf("");
    ++s.n_deg;
  } else {
    rh = rhat;
    if (!__builtin_isfinite(rhat)) {
      ++s.n_nonf;
    } else {
      ++s.n_eval;
      s.sum += (double)rhat;
      s.above0 += rhat > a.thr0;
      s.above1 += rhat > a.thr1;
      s.above2 += rhat > a.thr2;
      if (rhat > s.mx) {  // a lane's elements ascend: strict keeps the lowest index
        s.mx = rhat;
        s.argmax = idx;
      }
    }
  }
}

template <bool GUARD>
__device__ __forceinline__ f4v dload(const float* __restrict__ p, int64_t e, int64_t n) {
  if constexpr (GUARD)
    return ld4(p, e, n);  // element-wise past the last full group; never past n
  else
    return vload(p + e);
}

// Float4 group gi of every chain.  GUARD: the group may be the partial last
// one (elements >= n neither read, written nor counted).
template <int VAR, bool RECIP, bool GUARD>
__device__ __forceinline__ void diag_group(const DArgs& a, int64_t gi, Stat& s) {
  const int64_t e = gi * 4;
  const f4v z = {0.f, 0.f, 0.f, 0.f};
  const f4v m0 = dload<GUARD>(a.mom1, e, a.n);
  const f4v q0 = dload<GUARD>(a.mom2, e, a.n);
  f4v S1 = z, S2 = z, SW = z;
  accum4<VAR, RECIP>(a, m0, m0, q0, S1, S2, SW);
  int k = 1;
  for (; k + 4 <= a.chains; k += 4) {
    f4v m[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t o = (int64_t)(k + u) * a.slot;
      m[u] = dload<GUARD>(a.mom1 + o, e, a.n);
      q[u] = dload<GUARD>(a.mom2 + o, e, a.n);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) accum4<VAR, RECIP>(a, m0, m[u], q[u], S1, S2, SW);
  }
  for (; k < a.chains; ++k) {
    const int64_t o = (int64_t)k * a.slot;
    const f4v m = dload<GUARD>(a.mom1 + o, e, a.n);
    const f4v q = dload<GUARD>(a.mom2 + o, e, a.n);
    accum4<VAR, RECIP>(a, m0, m, q, S1, S2, SW);
  }
  f4v pm = z, pv = z, rh = z;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (GUARD && e + j >= a.n) break;
    float xm, xv, xr;
    finish_elem(a, m0[j], S1[j], S2[j], SW[j], e + j, xm, xv, xr, s);
    pm[j] = xm;
    pv[j] = xv;
    rh[j] = xr;
  }
  if constexpr (GUARD) {
    if (a.pooled_mean) st4(a.pooled_mean, e, a.n, pm);
    if (a.pooled_var) st4(a.pooled_var, e, a.n, pv);
    if (a.rhat) st4(a.rhat, e, a.n, rh);
  } else {
    if (a.pooled_mean) vstore(a.pooled_mean + e, pm);
    if (a.pooled_var) vstore(a.pooled_var + e, pv);
    if (a.rhat) vstore(a.rhat + e, rh);
  }
}

// Grid-stride sweep in bdl_sample_kernel's shape: an unguarded loop over the
// block iterations wholly inside [0, n), then at most one guarded iteration
// per block for the tail.  gridDim.x <= kMaxDiagPartials (the host's cap).
template <int VAR, bool RECIP>
__global__ __launch_bounds__(kBlock) void bdl_chain_diag_kernel(const DArgs a) {
  const int64_t ngroups = (a.n + 3) >> 2, nfull = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  Stat s = stat_empty();
  int64_t gb = (int64_t)blockIdx.x * kBlock;
  for (; gb + kBlock <= nfull; gb += stride) diag_group<VAR, RECIP, false>(a, gb + threadIdx.x, s);
  if (gb < ngroups) {
    const int64_t gi = gb + threadIdx.x;
    if (gi < ngroups) diag_group<VAR, RECIP, true>(a, gi, s);
  }
  s = block_combine(s);
  if (threadIdx.x == 0) store_stat(a.partials + blockIdx.x, s);
}

// One workgroup: the partials in a fixed order (thread t takes t, t + 256,
// ...; then the wave butterfly and the waves in order), the empty case's
// conventions, the summary.
__global__ __launch_bounds__(kBlock) void bdl_chain_diag_finalize_kernel(
    const bdl_diag_summary* __restrict__ partials, int nparts, bdl_diag_summary* __restrict__ out) {
  Stat s = stat_empty();
  for (int i = threadIdx.x; i < nparts; i += kBlock) {
    const bdl_diag_summary& p = partials[i];
    Stat o;
    o.n_eval = p.n_eval;
    o.n_deg = p.n_degenerate;
    o.n_nonf = p.n_nonfinite;
    o.above0 = p.n_above[0];
    o.above1 = p.n_above[1];
    o.above2 = p.n_above[2];
    o.argmax = p.argmax;
    o.sum = p.rhat_sum;
    o.mx = p.rhat_max;
    s = combine(s, o);
  }
  s = block_combine(s);
  if (threadIdx.x == 0) {
    if (s.n_eval == 0) {
      s.mx = 0.0f;
      s.argmax = -1;
    }
    store_stat(out, s);
  }
}

typedef void (*DiagKernel)(const DArgs);

DiagKernel pick_diag(int var_mode, bool recip) {
  switch (var_mode) {
    case BDL_VAR_RAW_MOMENTS: return bdl_chain_diag_kernel<BDL_VAR_RAW_MOMENTS, false>;
    case BDL_VAR_WELFORD:
      return recip ? bdl_chain_diag_kernel<BDL_VAR_WELFORD, true>
                   : bdl_chain_diag_kernel<BDL_VAR_WELFORD, false>;
    default: return bdl_chain_diag_kernel<BDL_VAR_GIVEN, false>;
  }
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_chain_diag_workspace_bytes(int64_t n) {
  (void)n;
  return kPartialsOffset + (int64_t)kMaxDiagPartials * (int64_t)sizeof(bdl_diag_summary);
}

int bdl_chain_diag(const bdl_chain_diag_args* d, void* stream) {
  if (graph_redirect_active())
    return fail(BDL_ERR_ARG, "bdl_chain_diag: a graph redirect is active (bdl_graph_redirect); "
                "only bdl_sgmcmc_step rewrites a node");
  if (!d) return fail(BDL_ERR_NULL, "bdl_chain_diag: null args");
  if (!d->mom1 || !d->mom2) return fail(BDL_ERR_NULL, "bdl_chain_diag: mom1 and mom2 are required");
  if (!d->workspace) return fail(BDL_ERR_NULL, "bdl_chain_diag: null workspace");
  if (d->chains < 2) return fail(BDL_ERR_ARG, "bdl_chain_diag: chains must be >= 2");
  if (d->n < 1) return fail(BDL_ERR_ARG, "bdl_chain_diag: n must be >= 1");
  if (d->var_mode < BDL_VAR_GIVEN || d->var_mode > BDL_VAR_WELFORD)
    return fail(BDL_ERR_ARG, "bdl_chain_diag: unknown var_mode");
  if (!(d->var_floor >= 0.0f)) return fail(BDL_ERR_ARG, "bdl_chain_diag: var_floor must be >= 0");
  if (d->blocks_per_cu < 0 || d->blocks_per_cu > 8)
    return fail(BDL_ERR_ARG, "bdl_chain_diag: blocks_per_cu in [0, 8]");
  // every element index 4*chain_groups*k + j must fit the signed 64-bit index
  if (d->chain_groups > (uint64_t)(INT64_MAX / 4) / (uint64_t)d->chains)
    return fail(BDL_ERR_ARG, "bdl_chain_diag: chains * chain_groups overflows the element index");
  if ((uint64_t)d->n > 4 * d->chain_groups)
    return fail(BDL_ERR_ARG, "bdl_chain_diag: n exceeds the chain slot (4 * chain_groups)");
  const void* ptrs[] = {d->mom1, d->mom2, d->pooled_mean, d->pooled_var, d->rhat};
  for (const void* p : ptrs)
    if (p && !aligned16(p)) return fail(BDL_ERR_ALIGN, "bdl_chain_diag: vector not 16-B aligned");
  if (!aligned16(d->workspace))
    return fail(BDL_ERR_ALIGN, "bdl_chain_diag: workspace not 16-B aligned");

  bdl_diag_summary* summary = reinterpret_cast<bdl_diag_summary*>(d->workspace);
  bdl_diag_summary* partials = reinterpret_cast<bdl_diag_summary*>(
      reinterpret_cast<char*>(d->workspace) + kPartialsOffset);
  DArgs a;
  a.mom1 = d->mom1;
  a.mom2 = d->mom2;
  a.pooled_mean = d->pooled_mean;
  a.pooled_var = d->pooled_var;
  a.rhat = d->rhat;
  a.partials = partials;
  a.n = d->n;
  a.slot = (int64_t)(4 * d->chain_groups);
  a.chains = d->chains;
  a.ratio = d->ratio;
  a.inv_ratio = d->inv_ratio;
  a.var_floor = d->var_floor;
  a.c1 = d->c1;
  a.fk = (float)d->chains;
  a.fkm1 = (float)(d->chains - 1);
  a.thr0 = d->thresholds[0];
  a.thr1 = d->thresholds[1];
  a.thr2 = d->thresholds[2];

  const int64_t ngroups = (d->n + 3) / 4;
  const int64_t want = (ngroups + kBlock - 1) / kBlock;
  const int64_t cap = std::min<int64_t>(
      (int64_t)cu_count() * (d->blocks_per_cu > 0 ? d->blocks_per_cu : kDiagBpc), kMaxDiagPartials);
  const int grid = (int)std::max<int64_t>(1, std::min(want, cap));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pick_diag(d->var_mode, d->inv_ratio != 0.0f), dim3(grid), dim3(kBlock), 0, st,
                     a);
  hipLaunchKernelGGL(bdl_chain_diag_finalize_kernel, dim3(1), dim3(kBlock), 0, st, partials, grid,
                     summary);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_last_error(std::string("bdl_chain_diag: launch failed: ") + hipGetErrorString(err));
    return BDL_ERR_LAUNCH;
  }
  return BDL_OK;
}

}  // extern "C"
