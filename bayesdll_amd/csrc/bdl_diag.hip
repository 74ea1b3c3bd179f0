// bdl_diag.hip — cross-chain R-hat and pooled posterior of stacked chains
// (include/bdl_diag.h: the arithmetic, the conventions, the summary).
//
// One sweep over the K chains' stacked (mom1, mom2): a lane owns one float4
// group of elements and walks the chains, K read streams a chain slot apart
// (non-temporal 16-B loads, the chain loop unrolled by 4 so eight loads are in
// flight per lane), then finishes its four elements (six IEEE divisions and a
// square root per element, none per chain) and stores the requested outputs.
// The per-element arithmetic is bdl_chain_elem.hpp's (shared with bdl_layers.hip), the
// summary's reduction bdl_chain_common.hpp's (shared with bdl_ess.hip):
// per-lane accumulators, a 64-lane butterfly, the block's 4 waves through LDS,
// one partial per workgroup written with ordinary stores, and a one-workgroup
// launch that combines the partials in a fixed order.  No atomics, no host
// synchronisation, no allocation.
#include "bdl_chain_elem.hpp"

namespace bdl {
namespace {

constexpr int kMaxDiagPartials = 2048;   // 256 CUs x 8 workgroups
constexpr int kDiagBpc = 2;              // default workgroups per CU, as the posterior draw

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

using Stat = DiagStat;  // bdl_chain_elem.hpp: the adapter DiagSummary, diag_accum4, diag_finish_elem

// Float4 group gi of every chain.  GUARD: the group may be the partial last
// one (elements >= n neither read, written nor counted).
template <int VAR, bool RECIP, bool GUARD>
__device__ __forceinline__ void diag_group(const DArgs& a, int64_t gi, Stat& s) {
  const int64_t e = gi * 4;
  const f4v z = {0.f, 0.f, 0.f, 0.f};
  const f4v m0 = gload<GUARD>(a.mom1, e, a.n);
  const f4v q0 = gload<GUARD>(a.mom2, e, a.n);
  f4v S1 = z, S2 = z, SW = z;
  diag_accum4<VAR, RECIP>(a, m0, m0, q0, S1, S2, SW);
  int k = 1;
  for (; k + 4 <= a.chains; k += 4) {
    f4v m[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t o = (int64_t)(k + u) * a.slot;
      m[u] = gload<GUARD>(a.mom1 + o, e, a.n);
      q[u] = gload<GUARD>(a.mom2 + o, e, a.n);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) diag_accum4<VAR, RECIP>(a, m0, m[u], q[u], S1, S2, SW);
  }
  for (; k < a.chains; ++k) {
    const int64_t o = (int64_t)k * a.slot;
    const f4v m = gload<GUARD>(a.mom1 + o, e, a.n);
    const f4v q = gload<GUARD>(a.mom2 + o, e, a.n);
    diag_accum4<VAR, RECIP>(a, m0, m, q, S1, S2, SW);
  }
  f4v pm = z, pv = z, rh = z;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (GUARD && e + j >= a.n) break;
    float xm, xv, xr;
    diag_finish_elem(a, m0[j], S1[j], S2[j], SW[j], e + j, xm, xv, xr, s);
    pm[j] = xm;
    pv[j] = xv;
    rh[j] = xr;
  }
  if (a.pooled_mean) gstore<GUARD>(a.pooled_mean, e, a.n, pm);
  if (a.pooled_var) gstore<GUARD>(a.pooled_var, e, a.n, pv);
  if (a.rhat) gstore<GUARD>(a.rhat, e, a.n, rh);
}

// Grid-stride sweep in bdl_sample_kernel's shape: an unguarded loop over the
// block iterations wholly inside [0, n), then at most one guarded iteration
// per block for the tail.  gridDim.x <= kMaxDiagPartials (the host's cap): one
// partial per workgroup.
template <int VAR, bool RECIP>
__global__ __launch_bounds__(kBlock) void bdl_chain_diag_kernel(const DArgs a) {
  const int64_t ngroups = (a.n + 3) >> 2, nfull = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  Stat s = Stat::empty();
  int64_t gb = (int64_t)blockIdx.x * kBlock;
  for (; gb + kBlock <= nfull; gb += stride) diag_group<VAR, RECIP, false>(a, gb + threadIdx.x, s);
  if (gb < ngroups) {
    const int64_t gi = gb + threadIdx.x;
    if (gi < ngroups) diag_group<VAR, RECIP, true>(a, gi, s);
  }
  store_partial<DiagSummary>(a.partials, s);
}

__global__ __launch_bounds__(kBlock) void bdl_chain_diag_finalize_kernel(
    const bdl_diag_summary* __restrict__ partials, int nparts, bdl_diag_summary* __restrict__ out) {
  finalize_summary<DiagSummary>(partials, nparts, out);
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
  const std::string me = "bdl_chain_diag: ";
  if (const int rc = no_redirect("bdl_chain_diag")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->mom1 || !d->mom2) return fail(BDL_ERR_NULL, me + "mom1 and mom2 are required");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->chains < 2) return fail(BDL_ERR_ARG, me + "chains must be >= 2");
  if (d->n < 1) return fail(BDL_ERR_ARG, me + "n must be >= 1");
  if (d->var_mode < BDL_VAR_GIVEN || d->var_mode > BDL_VAR_WELFORD)
    return fail(BDL_ERR_ARG, me + "unknown var_mode");
  if (!(d->var_floor >= 0.0f)) return fail(BDL_ERR_ARG, me + "var_floor must be >= 0");
  if (d->blocks_per_cu < 0 || d->blocks_per_cu > 8)
    return fail(BDL_ERR_ARG, me + "blocks_per_cu in [0, 8]");
  if (const char* why = stacked_slot_error(d->chains, d->n, d->chain_groups))
    return fail(BDL_ERR_ARG, me + why);
  const void* ptrs[] = {d->mom1, d->mom2, d->pooled_mean, d->pooled_var, d->rhat};
  for (const void* p : ptrs)
    if (misaligned(p, 15)) return fail(BDL_ERR_ALIGN, me + "vector not 16-B aligned");
  if (misaligned(d->workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");

  bdl_diag_summary* summary = reinterpret_cast<bdl_diag_summary*>(d->workspace);
  bdl_diag_summary* partials = partials_of<bdl_diag_summary>(d->workspace);
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

  const int64_t cap = std::min<int64_t>(
      (int64_t)cu_count() * (d->blocks_per_cu > 0 ? d->blocks_per_cu : kDiagBpc), kMaxDiagPartials);
  const int grid = (int)capped_grid(block_iters(d->n, kBlock), cap);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pick_diag(d->var_mode, d->inv_ratio != 0.0f), dim3(grid), dim3(kBlock), 0, st,
                     a);
  hipLaunchKernelGGL(bdl_chain_diag_finalize_kernel, dim3(1), dim3(kBlock), 0, st, partials, grid,
                     summary);
  return launched("bdl_chain_diag");
}

}  // extern "C"
