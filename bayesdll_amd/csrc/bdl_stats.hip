// bdl_stats.hip — per-chain, per-tensor sufficient statistics of stacked chains
// (include/bdl_stats.h: the arithmetic, the segment form, the alignment rule).
//
// The sweep runs on bdl_clip.hip's (blocks_per_chain, K) grid: blockIdx.y is
// the chain, so a workgroup never leaves its chain.  A workgroup walks the
// segment table (wave-uniform loads of 40-B entries) and, in every segment,
// takes its share of the chain's slice of all bound streams (the gradient,
// theta, optionally the momentum and the prior mean) in block iterations of
// kBlock x 4 units, grid-strided over the chain's workgroups, the first of
// which is rotated by the segment index.  A unit is a float4 group where the
// gradient slice and the stacked vectors' slice share one misalignment mod
// 16 B (16-B loads, four per stream in flight per lane; the up to 3 elements
// before and after the common body go to three lanes each of the rotated first
// workgroup), and one element where they differ.  Five fp64 fma accumulators
// per lane, a 64-lane butterfly, the 4 waves through LDS, five partials per
// (workgroup, segment) written with ordinary stores; a second launch combines
// them in workgroup order, scales V2 by 1 / lr and updates acc.  No atomics,
// no host synchronisation, no allocation.
//
// The 16-B loads are ordinary (temporal) loads, unlike the step sweeps': the
// step launch that follows re-reads the same vectors, and the stats + step
// pair measured 2.6-3.5 % faster this way at the stacked mlp_mnist sizes and
// the same at 1 GiB (tools/chain_stats_timing.py).
// BDL_STATS_NT_LOADS builds the non-temporal form for that comparison.
#include "bdl_chain_common.hpp"
#include "bdl_stats.h"

namespace bdl {
namespace {

constexpr int kStatsUnroll = 4;                                  // units in flight per lane and stream
constexpr int64_t kStatsIter = (int64_t)kBlock * kStatsUnroll;   // units per block iteration
constexpr int kStatsWgPerCu = 4;                                 // default grid: this many per CU
constexpr int kSums = 5;                                         // G2, V2, D2, DG, VG

struct StatsK {
  const float* theta;
  const float* mom;
  const float* prior;
  const bdl_stats_segment* segs;
  int64_t slot;  // elements per chain slot of the stacked vectors
  int32_t nseg;
};

__device__ __forceinline__ f4v ldv(const float* p) {
#ifdef BDL_STATS_NT_LOADS
  return vload(p);
#else
  return *reinterpret_cast<const f4v*>(p);
#endif
}

// One element's five products, exact in double, accumulated with fp64 fma.
template <bool MOM, bool PRIOR>
__device__ __forceinline__ void acc1(float g, float t, float v, float p, double (&a)[kSums]) {
  const float d = PRIOR ? t - p : t;  // one fp32 rounding (-ffp-contract=off)
  const double gd = (double)g, dd = (double)d;
  a[0] = fma(gd, gd, a[0]);
  a[2] = fma(dd, dd, a[2]);
  a[3] = fma(dd, gd, a[3]);
  if (MOM) {
    const double vd = (double)v;
    a[1] = fma(vd, vd, a[1]);
    a[4] = fma(vd, gd, a[4]);
  }
}

// W floats at unit i of p (W = 4: one 16-B load of an aligned group).
template <int W>
struct Unit {
  float x[W];
};

template <int W>
__device__ __forceinline__ Unit<W> ldu(const float* p, int64_t i) {
  Unit<W> u;
  if (W == 4) {
    const f4v v = ldv(p + 4 * i);
#pragma unroll
    for (int j = 0; j < W; ++j) u.x[j] = v[j];
  } else {
    u.x[0] = sload(p + i);
  }
  return u;
}

// This workgroup's share of `nunits` units of W floats of one chain's slice
// (workgroup b of the rotation): full block iterations with all loads of all
// streams issued before the first fma, then at most one partial iteration.
template <bool MOM, bool PRIOR, int W>
__device__ __forceinline__ void sweep_units(const float* g, const float* th, const float* mv,
                                            const float* pm, int64_t nunits, uint32_t b,
                                            double (&a)[kSums]) {
  const int64_t stride = (int64_t)gridDim.x * kStatsIter;
  int64_t gb = (int64_t)b * kStatsIter;
  for (; gb + kStatsIter <= nunits; gb += stride) {
    Unit<W> ug[kStatsUnroll], ut[kStatsUnroll], uv[kStatsUnroll], up[kStatsUnroll];
#pragma unroll
    for (int u = 0; u < kStatsUnroll; ++u) {
      const int64_t i = gb + (int64_t)u * kBlock + threadIdx.x;
      ug[u] = ldu<W>(g, i);
      ut[u] = ldu<W>(th, i);
      if (MOM) uv[u] = ldu<W>(mv, i);
      if (PRIOR) up[u] = ldu<W>(pm, i);
    }
#pragma unroll
    for (int u = 0; u < kStatsUnroll; ++u)
#pragma unroll
      for (int j = 0; j < W; ++j)
        acc1<MOM, PRIOR>(ug[u].x[j], ut[u].x[j], MOM ? uv[u].x[j] : 0.f, PRIOR ? up[u].x[j] : 0.f,
                         a);
  }
  if (gb < nunits) {
#pragma unroll
    for (int u = 0; u < kStatsUnroll; ++u) {
      const int64_t i = gb + (int64_t)u * kBlock + threadIdx.x;
      if (i < nunits) {
        const Unit<W> ug = ldu<W>(g, i), ut = ldu<W>(th, i);
        Unit<W> uv = {}, up = {};
        if (MOM) uv = ldu<W>(mv, i);
        if (PRIOR) up = ldu<W>(pm, i);
#pragma unroll
        for (int j = 0; j < W; ++j) acc1<MOM, PRIOR>(ug.x[j], ut.x[j], uv.x[j], up.x[j], a);
      }
    }
  }
}

// partials[((k * gridDim.x + b) * nseg + i) * 5 + q]: workgroup b's share of
// sum q of (chain k, segment i).
template <bool MOM, bool PRIOR>
__global__ __launch_bounds__(kBlock) void bdl_chain_stats_kernel(StatsK a,
                                                                 double* __restrict__ partials) {
  __shared__ double s_wave[kBlock / 64][kSums];
  const int k = blockIdx.y;
  const int t = threadIdx.x;
  double* out = partials + ((int64_t)k * gridDim.x + blockIdx.x) * a.nseg * kSums;
  for (int i = 0; i < a.nseg; ++i) {
    const bdl_stats_segment s = a.segs[i];
    const float* g = s.grad + (int64_t)k * s.grad_stride;
    const int64_t vo = (int64_t)k * a.slot + s.offset;
    const float* th = a.theta + vo;
    const float* mv = MOM ? a.mom + vo : nullptr;
    const float* pm = PRIOR ? a.prior + vo : nullptr;
    // theta, mom and prior_mean are 16-B aligned and share vo: one misalignment
    const uint32_t mg = (uint32_t)(reinterpret_cast<uintptr_t>(g) >> 2) & 3u;
    const uint32_t ms = (uint32_t)(reinterpret_cast<uintptr_t>(th) >> 2) & 3u;
    const uint32_t b = rotated_block(i);
    double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool work;
    if (mg == ms) {
      const int64_t h0 = (4 - (int64_t)mg) & 3;
      const int64_t h = h0 < s.numel ? h0 : s.numel;
      const int64_t nbody = (s.numel - h) >> 2;
      const int tail = (int)(s.numel - h - 4 * nbody);
      work = b == 0 || (int64_t)b * kStatsIter < nbody;
      if (work) {
        sweep_units<MOM, PRIOR, 4>(g + h, th + h, MOM ? mv + h : nullptr, PRIOR ? pm + h : nullptr,
                                   nbody, b, acc);
        if (b == 0) {
          int64_t e = -1;
          if (t < (int)h) e = t;
          else if (t >= 4 && t - 4 < tail) e = h + 4 * nbody + (t - 4);
          if (e >= 0)
            acc1<MOM, PRIOR>(sload(g + e), sload(th + e), MOM ? sload(mv + e) : 0.f,
                             PRIOR ? sload(pm + e) : 0.f, acc);
        }
      }
    } else {
      work = (int64_t)b * kStatsIter < s.numel;
      if (work) sweep_units<MOM, PRIOR, 1>(g, th, mv, pm, s.numel, b, acc);
    }
    if (!work) {  // wave-uniform: a small tensor leaves most workgroups idle
      if (t < kSums) out[(int64_t)i * kSums + t] = 0.0;
      continue;
    }
#pragma unroll
    for (int q = 0; q < kSums; ++q) acc[q] = wave_sum(acc[q]);
    if ((t & 63) == 0) {
#pragma unroll
      for (int q = 0; q < kSums; ++q) s_wave[t >> 6][q] = acc[q];
    }
    __syncthreads();
    if (t < kSums) {
      double r = 0.0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) r += s_wave[w][t];
      out[(int64_t)i * kSums + t] = r;
    }
    __syncthreads();  // s_wave is reused by the next segment
  }
}

// One thread per (chain, segment, sum): the chain's partials in workgroup
// order, then acc (and, from V2, V2L = V2 * (1 / lr)).
__global__ __launch_bounds__(kBlock) void bdl_chain_stats_combine_kernel(
    const double* __restrict__ partials, int bpc, int nseg, int chains,
    const bdl_stats_segment* __restrict__ segs, const float* __restrict__ lr_table, int lr_stride,
    float lr0, float lr1, int accumulate, double* __restrict__ acc) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (int64_t)chains * nseg * kSums) return;
  const int q = (int)(idx % kSums);
  const int64_t kt = idx / kSums;
  const int t = (int)(kt % nseg);
  const int64_t k = kt / nseg;
  double s = 0.0;
  for (int b = 0; b < bpc; ++b) s += partials[((k * bpc + b) * nseg + t) * kSums + q];
  double* o = acc + kt * BDL_STATS_SUMS;
  o[q] = accumulate ? o[q] + s : s;
  if (q == 1) {
    const int grp = segs[t].lr_group != 0;
    const float lr = lr_table ? lr_table[k * lr_stride + grp] : (grp ? lr1 : lr0);
    const double v = s * (1.0 / (double)lr);
    o[5] = accumulate ? o[5] + v : v;
  }
}

template <bool MOM, bool PRIOR>
void launch_sweep(dim3 grid, hipStream_t st, const StatsK& k, double* partials) {
  hipLaunchKernelGGL((bdl_chain_stats_kernel<MOM, PRIOR>), grid, dim3(kBlock), 0, st, k, partials);
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_chain_stats_workspace_bytes(int32_t chains, int32_t nsegments) {
  if (chains < 1 || chains > BDL_STATS_MAX_CHAINS) return 0;
  if (nsegments < 1 || nsegments > BDL_STATS_MAX_SEGMENTS) return 0;
  return (int64_t)chains * BDL_STATS_MAX_BLOCKS_PER_CHAIN * nsegments * kSums *
         (int64_t)sizeof(double);
}

int bdl_chain_stats(const bdl_chain_stats_args* d, void* stream) {
  if (const int rc = no_redirect("bdl_chain_stats")) return rc;
  if (!d) return fail(BDL_ERR_NULL, "bdl_chain_stats: null args");
  if (!d->theta) return fail(BDL_ERR_NULL, "bdl_chain_stats: null theta");
  if (!d->segments) return fail(BDL_ERR_NULL, "bdl_chain_stats: null segments");
  if (!d->acc) return fail(BDL_ERR_NULL, "bdl_chain_stats: null acc");
  if (!d->workspace) return fail(BDL_ERR_NULL, "bdl_chain_stats: null workspace");
  if (misaligned(d->theta, 15)) return fail(BDL_ERR_ALIGN, "bdl_chain_stats: theta not 16-B aligned");
  if (misaligned(d->mom, 15)) return fail(BDL_ERR_ALIGN, "bdl_chain_stats: mom not 16-B aligned");
  if (misaligned(d->prior_mean, 15))
    return fail(BDL_ERR_ALIGN, "bdl_chain_stats: prior_mean not 16-B aligned");
  if (misaligned(d->workspace, 15))
    return fail(BDL_ERR_ALIGN, "bdl_chain_stats: workspace not 16-B aligned");
  if (misaligned(d->segments, 7))
    return fail(BDL_ERR_ALIGN, "bdl_chain_stats: segments not 8-B aligned");
  if (misaligned(d->acc, 7)) return fail(BDL_ERR_ALIGN, "bdl_chain_stats: acc not 8-B aligned");
  if (misaligned(d->lr_table, 3))
    return fail(BDL_ERR_ALIGN, "bdl_chain_stats: lr_table not 4-B aligned");
  if (d->chains < 1 || d->chains > BDL_STATS_MAX_CHAINS)
    return fail(BDL_ERR_ARG, "bdl_chain_stats: chains in [1, " +
                std::to_string(BDL_STATS_MAX_CHAINS) + "]");
  if (d->nsegments < 1 || d->nsegments > BDL_STATS_MAX_SEGMENTS)
    return fail(BDL_ERR_ARG, "bdl_chain_stats: nsegments in [1, " +
                std::to_string(BDL_STATS_MAX_SEGMENTS) + "]");
  if (d->chain_groups < 1 || d->chain_groups > (uint64_t)BDL_STATS_MAX_CHAIN_GROUPS)
    return fail(BDL_ERR_ARG, "bdl_chain_stats: chain_groups in [1, 2^40]");
  if (d->blocks_per_chain < 0 || d->blocks_per_chain > BDL_STATS_MAX_BLOCKS_PER_CHAIN)
    return fail(BDL_ERR_ARG, "bdl_chain_stats: blocks_per_chain in [0, " +
                std::to_string(BDL_STATS_MAX_BLOCKS_PER_CHAIN) + "]");
  const bool host_lr = d->lr[0] != 0.0f || d->lr[1] != 0.0f;  // a NaN counts as given
  if (host_lr && d->lr_table)
    return fail(BDL_ERR_ARG, "bdl_chain_stats: both lr sources given (host lr and lr_table)");
  if (!host_lr && !d->lr_table)
    return fail(BDL_ERR_ARG, "bdl_chain_stats: neither lr source given (host lr or lr_table)");
  if (host_lr && !(d->lr[0] > 0.0f && d->lr[1] > 0.0f))
    return fail(BDL_ERR_ARG, "bdl_chain_stats: host lr must be > 0 for both groups");
  if (d->lr_table && d->lr_row_stride < 2)
    return fail(BDL_ERR_ARG, "bdl_chain_stats: lr_row_stride must be >= 2");
  if (d->accumulate != 0 && d->accumulate != 1)
    return fail(BDL_ERR_ARG, "bdl_chain_stats: accumulate must be 0 or 1");

  int bpc = d->blocks_per_chain;
  if (bpc == 0)  // the table's sizes are on the device: fill the CUs, whatever it holds
    bpc = (int)blocks_per_chain(kStatsWgPerCu, d->chains, BDL_STATS_MAX_BLOCKS_PER_CHAIN);
  StatsK k;
  k.theta = d->theta;
  k.mom = d->mom;
  k.prior = d->prior_mean;
  k.segs = d->segments;
  k.slot = (int64_t)(4 * d->chain_groups);
  k.nseg = d->nsegments;
  double* partials = reinterpret_cast<double*>(d->workspace);
  const dim3 grid((unsigned)bpc, (unsigned)d->chains);
  hipStream_t st = (hipStream_t)stream;
  if (d->mom && d->prior_mean) launch_sweep<true, true>(grid, st, k, partials);
  else if (d->mom) launch_sweep<true, false>(grid, st, k, partials);
  else if (d->prior_mean) launch_sweep<false, true>(grid, st, k, partials);
  else launch_sweep<false, false>(grid, st, k, partials);
  const int64_t total = (int64_t)d->chains * d->nsegments * kSums;
  hipLaunchKernelGGL(bdl_chain_stats_combine_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, st, partials, bpc, d->nsegments, d->chains, d->segments,
                     d->lr_table, d->lr_row_stride, d->lr[0], d->lr[1], d->accumulate, d->acc);
  return launched("bdl_chain_stats");
}

}  // extern "C"
