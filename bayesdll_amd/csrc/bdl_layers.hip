// bdl_layers.hip — per-tensor R-hat and effective sample size of stacked chains
// (include/bdl_layers.h: the segment table, the contract, the traversal).
//
// The traversal is bdl_stats.hip's: every workgroup walks the segment table
// (wave-uniform loads of 16-B rows) and takes block iterations of a segment,
// grid-strided from a first workgroup rotated by the segment index.  The chain
// walk is bdl_diag.hip's / bdl_ess.hip's: a lane owns one float4 group and
// loops over the K chains (chain 0 peeled, the loop unrolled by 4, non-temporal
// 16-B loads), then finishes its elements with bdl_chain_elem.hpp's functions —
// the definitions the whole-vector kernels instantiate.  The up to 3 elements
// before the first and after the last 16-B boundary of a tensor are one
// partial group each (scalar loads): the head on thread 0, the tail on thread
// 64 of the segment's rotated first workgroup, so that they run in two waves
// side by side and every lane's indices still ascend.  One partial per
// (workgroup, segment) through block_combine, laid out [segment][workgroup];
// a second launch with one workgroup per segment combines a row's partials in
// workgroup order (finalize_summary).  No atomics, no host synchronisation, no
// allocation.
#include "bdl_chain_elem.hpp"
#include "bdl_layers.h"

namespace bdl {
namespace {

constexpr int kLayersBpc = 2;  // default workgroups per CU, as bdl_chain_diag / bdl_chain_ess

struct LDArgs {
  const float* __restrict__ mom1;
  const float* __restrict__ mom2;
  int64_t slot;  // elements per chain slot, 4 * chain_groups
  int32_t chains;
  float ratio, inv_ratio, var_floor, c1;
  float fk, fkm1;  // K and K - 1 as fp32
  float thr0, thr1, thr2;
};

struct LEArgs {
  const float* __restrict__ sM2;
  const float* __restrict__ bM2;
  int64_t slot;
  int32_t chains;
  float fS1, fnb1, fKnb;  // S - 1, nb - 1 and K * nb as fp32
  float thr0, thr1, thr2;
};

// The two reports as the traversal sees them: Args, the public Summary and its
// adapter, and group<PART>(a, e, cnt, s) — the `cnt` elements at chain-local
// index e of every chain (PART: cnt < 4, scalar loads of exactly those; else a
// whole 16-B aligned group).
template <int VAR, bool RECIP>
struct DiagLayers {
  using Args = LDArgs;
  using Summary = bdl_diag_summary;
  using Adapter = DiagSummary;
  using Stat = DiagStat;

  template <bool PART>
  static __device__ __forceinline__ void group(const Args& a, int64_t e, int cnt, Stat& s) {
    const int64_t lim = e + cnt;  // gload<true>: elements >= lim are not read
    const f4v z = {0.f, 0.f, 0.f, 0.f};
    const f4v m0 = gload<PART>(a.mom1, e, lim);
    const f4v q0 = gload<PART>(a.mom2, e, lim);
    f4v S1 = z, S2 = z, SW = z;
    diag_accum4<VAR, RECIP>(a, m0, m0, q0, S1, S2, SW);
    int k = 1;
    for (; k + 4 <= a.chains; k += 4) {
      f4v m[4], q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t o = (int64_t)(k + u) * a.slot;
        m[u] = gload<PART>(a.mom1 + o, e, lim);
        q[u] = gload<PART>(a.mom2 + o, e, lim);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) diag_accum4<VAR, RECIP>(a, m0, m[u], q[u], S1, S2, SW);
    }
    for (; k < a.chains; ++k) {
      const int64_t o = (int64_t)k * a.slot;
      const f4v m = gload<PART>(a.mom1 + o, e, lim);
      const f4v q = gload<PART>(a.mom2 + o, e, lim);
      diag_accum4<VAR, RECIP>(a, m0, m, q, S1, S2, SW);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (PART && j >= cnt) break;
      float xm, xv, xr;
      diag_finish_elem(a, m0[j], S1[j], S2[j], SW[j], e + j, xm, xv, xr, s);
    }
  }
};

struct EssLayers {
  using Args = LEArgs;
  using Summary = bdl_ess_summary;
  using Adapter = EssSummary;
  using Stat = EssStat;

  template <bool PART>
  static __device__ __forceinline__ void group(const Args& a, int64_t e, int cnt, Stat& s) {
    const int64_t lim = e + cnt;
    const f4v z = {0.f, 0.f, 0.f, 0.f};
    const f4v m0 = gload<PART>(a.sM2, e, lim);
    const f4v q0 = gload<PART>(a.bM2, e, lim);
    f4v SW = z, SV = z;
    ess_accum4(m0, q0, SW, SV);
    int k = 1;
    for (; k + 4 <= a.chains; k += 4) {
      f4v m[4], q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t o = (int64_t)(k + u) * a.slot;
        m[u] = gload<PART>(a.sM2 + o, e, lim);
        q[u] = gload<PART>(a.bM2 + o, e, lim);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) ess_accum4(m[u], q[u], SW, SV);
    }
    for (; k < a.chains; ++k) {
      const int64_t o = (int64_t)k * a.slot;
      const f4v m = gload<PART>(a.sM2 + o, e, lim);
      const f4v q = gload<PART>(a.bM2 + o, e, lim);
      ess_accum4(m, q, SW, SV);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (PART && j >= cnt) break;
      float xe, xm;
      ess_finish_elem(a, SW[j], SV[j], e + j, xe, xm, s);
    }
  }
};

// partials[i * gridDim.x + b]: workgroup b's share of segment i.
template <class P>
__global__ __launch_bounds__(kBlock) void bdl_layers_kernel(
    const typename P::Args a, const bdl_layer_segment* __restrict__ segs, int nseg,
    typename P::Summary* __restrict__ partials) {
  using Stat = typename P::Stat;
  const int t = threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int i = 0; i < nseg; ++i) {
    const bdl_layer_segment sg = segs[i];
    // every chain's slice starts 4 * chain_groups * k elements on: one misalignment
    const int64_t h0 = (4 - (sg.offset & 3)) & 3;
    const int64_t h = h0 < sg.numel ? h0 : sg.numel;
    const int64_t nbody = (sg.numel - h) >> 2;
    const int tail = (int)(sg.numel - h - 4 * nbody);
    const uint32_t b = rotated_block(i);
    typename P::Summary* out = partials + (int64_t)i * gridDim.x + blockIdx.x;
    if (!(b == 0 || (int64_t)b * kBlock < nbody)) {  // wave-uniform: no iteration of this segment
      if (t == 0) P::Adapter::store(out, Stat::empty());
      continue;
    }
    Stat s = Stat::empty();
    const int64_t body = sg.offset + h;
    if (b == 0 && t == 0 && h > 0) P::template group<true>(a, sg.offset, (int)h, s);
    for (int64_t g = (int64_t)b * kBlock + t; g < nbody; g += stride)
      P::template group<false>(a, body + 4 * g, 4, s);
    if (b == 0 && t == 64 && tail > 0) P::template group<true>(a, body + 4 * nbody, tail, s);
    s = block_combine(s);
    if (t == 0) P::Adapter::store(out, s);
    __syncthreads();  // block_combine's LDS is reused by the next segment
  }
}

// One workgroup per segment: its partials in workgroup order.
template <class A, class Summary>
__global__ __launch_bounds__(kBlock) void bdl_layers_finalize_kernel(
    const Summary* __restrict__ partials, int nparts, Summary* __restrict__ table) {
  finalize_summary<A>(partials + (int64_t)blockIdx.x * nparts, nparts, table + blockIdx.x);
}

template <class P>
void launch_layers(const typename P::Args& a, const bdl_layer_segment* segs, int nseg, int grid,
                   void* workspace, typename P::Summary* table, hipStream_t st) {
  using Summary = typename P::Summary;
  Summary* partials = reinterpret_cast<Summary*>(workspace);
  hipLaunchKernelGGL((bdl_layers_kernel<P>), dim3(grid), dim3(kBlock), 0, st, a, segs, nseg,
                     partials);
  hipLaunchKernelGGL((bdl_layers_finalize_kernel<typename P::Adapter, Summary>), dim3(nseg),
                     dim3(kBlock), 0, st, partials, grid, table);
}

static_assert(sizeof(bdl_diag_summary) == sizeof(bdl_ess_summary), "one workspace size for both");

int64_t workspace_bytes(int64_t nsegments, int64_t grid_blocks) {
  const int64_t g = grid_blocks > 0 ? grid_blocks : BDL_LAYERS_MAX_GRID;
  return nsegments * g * (int64_t)sizeof(bdl_diag_summary);
}

// What both entry points check beyond their own report's fields; BDL_OK: fine.
// v0 / v1: the input vectors, `in` bytes each.
int common_error(const std::string& me, const void* v0, const void* v1, const void* segments,
                 const void* table, const void* workspace, int32_t nsegments, int32_t grid_blocks,
                 uint64_t in) {
  if (nsegments < 1 || nsegments > BDL_LAYERS_MAX_SEGMENTS)
    return fail(BDL_ERR_ARG, me + "nsegments in [1, " + std::to_string(BDL_LAYERS_MAX_SEGMENTS) +
                "]");
  if (grid_blocks < 0 || grid_blocks > BDL_LAYERS_MAX_GRID)
    return fail(BDL_ERR_ARG, me + "grid_blocks in [0, " + std::to_string(BDL_LAYERS_MAX_GRID) + "]");
  if (misaligned(v0, 15) || misaligned(v1, 15))
    return fail(BDL_ERR_ALIGN, me + "vector not 16-B aligned");
  if (misaligned(workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");
  if (misaligned(segments, 7)) return fail(BDL_ERR_ALIGN, me + "segments not 8-B aligned");
  if (misaligned(table, 7)) return fail(BDL_ERR_ALIGN, me + "table not 8-B aligned");
  const uint64_t tb = (uint64_t)nsegments * sizeof(bdl_diag_summary);
  const uint64_t sb = (uint64_t)nsegments * sizeof(bdl_layer_segment);
  const uint64_t wsb = (uint64_t)workspace_bytes(nsegments, grid_blocks);
  if (overlap(table, v0, tb, in) || overlap(table, v1, tb, in) || overlap(table, segments, tb, sb))
    return fail(BDL_ERR_ARG, me + "the table overlaps an input or the segment table");
  if (overlap(workspace, v0, wsb, in) || overlap(workspace, v1, wsb, in) ||
      overlap(workspace, segments, wsb, sb))
    return fail(BDL_ERR_ARG, me + "the workspace overlaps an input or the segment table");
  if (overlap(workspace, table, wsb, tb))
    return fail(BDL_ERR_ARG, me + "the workspace overlaps the table");
  return BDL_OK;
}

int layers_grid(int32_t grid_blocks) {
  return grid_blocks > 0
             ? grid_blocks
             : (int)capped_grid((int64_t)cu_count() * kLayersBpc, BDL_LAYERS_MAX_GRID);
}

template <int VAR, bool RECIP>
void launch_diag(const LDArgs& a, const bdl_diag_layers_args* d, int grid, hipStream_t st) {
  launch_layers<DiagLayers<VAR, RECIP>>(a, d->segments, d->nsegments, grid, d->workspace, d->table,
                                        st);
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int64_t bdl_layers_workspace_bytes(int32_t nsegments, int32_t grid_blocks) {
  if (nsegments < 1 || nsegments > BDL_LAYERS_MAX_SEGMENTS) return 0;
  if (grid_blocks < 0 || grid_blocks > BDL_LAYERS_MAX_GRID) return 0;
  return workspace_bytes(nsegments, grid_blocks);
}

int bdl_chain_diag_layers(const bdl_diag_layers_args* d, void* stream) {
  const std::string me = "bdl_chain_diag_layers: ";
  if (const int rc = no_redirect("bdl_chain_diag_layers")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->mom1 || !d->mom2) return fail(BDL_ERR_NULL, me + "mom1 and mom2 are required");
  if (!d->segments) return fail(BDL_ERR_NULL, me + "null segments");
  if (!d->table) return fail(BDL_ERR_NULL, me + "null table");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->chains < 2) return fail(BDL_ERR_ARG, me + "chains must be >= 2");
  if (d->n < 1) return fail(BDL_ERR_ARG, me + "n must be >= 1");
  if (d->var_mode < BDL_VAR_GIVEN || d->var_mode > BDL_VAR_WELFORD)
    return fail(BDL_ERR_ARG, me + "unknown var_mode");
  if (!(d->var_floor >= 0.0f)) return fail(BDL_ERR_ARG, me + "var_floor must be >= 0");
  if (const char* why = stacked_slot_error(d->chains, d->n, d->chain_groups))
    return fail(BDL_ERR_ARG, me + why);
  const uint64_t in = 4 * (4 * d->chain_groups * (uint64_t)(d->chains - 1) + (uint64_t)d->n);
  if (const int rc = common_error(me, d->mom1, d->mom2, d->segments, d->table, d->workspace,
                                  d->nsegments, d->grid_blocks, in))
    return rc;

  LDArgs a;
  a.mom1 = d->mom1;
  a.mom2 = d->mom2;
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
  const int grid = layers_grid(d->grid_blocks);
  hipStream_t st = (hipStream_t)stream;
  switch (d->var_mode) {  // the instances of bdl_chain_diag
    case BDL_VAR_RAW_MOMENTS: launch_diag<BDL_VAR_RAW_MOMENTS, false>(a, d, grid, st); break;
    case BDL_VAR_WELFORD:
      if (d->inv_ratio != 0.0f)
        launch_diag<BDL_VAR_WELFORD, true>(a, d, grid, st);
      else
        launch_diag<BDL_VAR_WELFORD, false>(a, d, grid, st);
      break;
    default: launch_diag<BDL_VAR_GIVEN, false>(a, d, grid, st);
  }
  return launched("bdl_chain_diag_layers");
}

int bdl_chain_ess_layers(const bdl_ess_layers_args* d, void* stream) {
  const std::string me = "bdl_chain_ess_layers: ";
  if (const int rc = no_redirect("bdl_chain_ess_layers")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->sM2 || !d->bM2) return fail(BDL_ERR_NULL, me + "sM2 and bM2 are required");
  if (!d->segments) return fail(BDL_ERR_NULL, me + "null segments");
  if (!d->table) return fail(BDL_ERR_NULL, me + "null table");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (d->chains < 1 || d->chains > BDL_ESS_MAX_CHAINS)
    return fail(BDL_ERR_ARG, me + "chains must be in [1, 65535]");
  if (d->n < 1) return fail(BDL_ERR_ARG, me + "n must be >= 1");
  if (const char* why = stacked_slot_error(d->chains, d->n, d->chain_groups))
    return fail(BDL_ERR_ARG, me + why);
  if (d->samples >= BDL_ESS_MAX_COUNT || d->batches >= BDL_ESS_MAX_COUNT)
    return fail(BDL_ERR_ARG, me + "samples and batches must be below 2^24 (exact in fp32)");
  if (d->samples < 2)
    return fail(BDL_ERR_ARG, me + "samples must be >= 2 (got " + std::to_string(d->samples) + ")");
  if (d->batches < 2)
    return fail(BDL_ERR_ARG, me + "batches must be >= 2 (got " + std::to_string(d->batches) + ")");
  if (d->batches > d->samples) return fail(BDL_ERR_ARG, me + "batches exceeds samples");
  const uint64_t in = 4 * (4 * d->chain_groups * (uint64_t)(d->chains - 1) + (uint64_t)d->n);
  if (const int rc = common_error(me, d->sM2, d->bM2, d->segments, d->table, d->workspace,
                                  d->nsegments, d->grid_blocks, in))
    return rc;

  LEArgs a;
  a.sM2 = d->sM2;
  a.bM2 = d->bM2;
  a.slot = (int64_t)(4 * d->chain_groups);
  a.chains = d->chains;
  a.fS1 = (float)(d->samples - 1);
  a.fnb1 = (float)(d->batches - 1);
  a.fKnb = (float)((int64_t)d->chains * d->batches);
  a.thr0 = d->thresholds[0];
  a.thr1 = d->thresholds[1];
  a.thr2 = d->thresholds[2];
  launch_layers<EssLayers>(a, d->segments, d->nsegments, layers_grid(d->grid_blocks), d->workspace,
                           d->table, (hipStream_t)stream);
  return launched("bdl_chain_ess_layers");
}

}  // extern "C"
