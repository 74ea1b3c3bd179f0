// bdl_ess.hip — batch-means effective sample size of stacked chains
// (include/bdl_ess.h: the arithmetic, the conventions, the summary).
//
// Two sweeps over vectors laid out like theta.  The fold: a lane owns one
// float4 group of one chain (the grid's y extent is the chain), reads theta and
// the accumulators the flags name with non-temporal 16-B loads and stores them
// back; the flags are template parameters, so a vector a fold does not need
// appears in no instruction.  The report: a lane owns one float4 group of
// elements and walks the chains, K read streams a chain slot apart (chain 0
// peeled, the loop unrolled by 4 so eight loads are in flight per lane), then
// finishes its four elements (four IEEE divisions and a square root per
// element, none per chain; bdl_chain_elem.hpp, shared with bdl_layers.hip).
// Its summary is reduced by bdl_chain_common.hpp
// (shared with bdl_diag.hip): per-lane accumulators, a 64-lane butterfly, the
// block's 4 waves through LDS, one partial per workgroup written with ordinary
// stores, and a one-workgroup launch that combines the partials in a fixed
// order.  No atomics, no host synchronisation, no allocation.
#include "bdl_chain_elem.hpp"

namespace bdl {
namespace {

constexpr int kEssBpc = 2;  // default workgroups per CU

// ------------------------------------------------------------------ the fold
struct FArgs {
  const float* __restrict__ theta;
  float* __restrict__ bsum;
  float* __restrict__ smean;
  float* __restrict__ sM2;
  float* __restrict__ bM2;
  int64_t n;
  int64_t slot;  // elements per chain slot, 4 * chain_groups
  float fs, fb, c;
};

// Float4 group gi of the chain whose slot starts at `o`.  GUARD: the group may
// be the partial last one (elements >= n neither read nor written).
template <int FLAGS, bool GUARD>
__device__ __forceinline__ void fold_group(const FArgs& a, int64_t o, int64_t gi) {
  constexpr bool kFirstSample = FLAGS & BDL_ESS_FIRST_SAMPLE;
  constexpr bool kFirstInBatch = FLAGS & BDL_ESS_FIRST_IN_BATCH;
  constexpr bool kClose = FLAGS & BDL_ESS_CLOSE;
  constexpr bool kFirstBatch = FLAGS & BDL_ESS_FIRST_BATCH;
  const int64_t e = gi * 4;
  const f4v z = {0.f, 0.f, 0.f, 0.f};
  const f4v x = gload<GUARD>(a.theta + o, e, a.n);
  f4v sm = z, M = z, bs = z, B = z;
  if constexpr (!kFirstSample) {
    sm = gload<GUARD>(a.smean + o, e, a.n);
    M = gload<GUARD>(a.sM2 + o, e, a.n);
  }
  if constexpr (!kFirstInBatch) bs = gload<GUARD>(a.bsum + o, e, a.n);
  if constexpr (kClose && !kFirstBatch) B = gload<GUARD>(a.bM2 + o, e, a.n);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float s1 = sm[j], m2 = M[j], b1 = bs[j], b2 = B[j];
    ess_fold_elem<FLAGS>(x[j], s1, m2, b1, b2, a.fs, a.fb, a.c);
    sm[j] = s1;
    M[j] = m2;
    bs[j] = b1;
    B[j] = b2;
  }
  gstore<GUARD>(a.smean + o, e, a.n, sm);
  gstore<GUARD>(a.sM2 + o, e, a.n, M);
  if constexpr (kClose)
    gstore<GUARD>(a.bM2 + o, e, a.n, B);
  else
    gstore<GUARD>(a.bsum + o, e, a.n, bs);
}

// Grid (blocks per chain, chains): a workgroup stays inside one chain.  An
// unguarded loop over the block iterations wholly inside the chain's [0, n),
// then at most one guarded iteration per block for the tail.
template <int FLAGS>
__global__ __launch_bounds__(kBlock) void bdl_ess_fold_kernel(const FArgs a) {
  const int64_t ngroups = (a.n + 3) >> 2, nfull = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t o = (int64_t)blockIdx.y * a.slot;
  int64_t gb = (int64_t)blockIdx.x * kBlock;
  for (; gb + kBlock <= nfull; gb += stride) fold_group<FLAGS, false>(a, o, gb + threadIdx.x);
  if (gb < ngroups) {
    const int64_t gi = gb + threadIdx.x;
    if (gi < ngroups) fold_group<FLAGS, true>(a, o, gi);
  }
}

typedef void (*FoldKernel)(const FArgs);

// the flag sets a (sample, batch) pair can imply
FoldKernel pick_fold(int flags) {
  switch (flags) {
    case 0: return bdl_ess_fold_kernel<0>;
    case BDL_ESS_FIRST_IN_BATCH: return bdl_ess_fold_kernel<BDL_ESS_FIRST_IN_BATCH>;
    case BDL_ESS_CLOSE: return bdl_ess_fold_kernel<BDL_ESS_CLOSE>;
    case BDL_ESS_CLOSE | BDL_ESS_FIRST_BATCH:
      return bdl_ess_fold_kernel<BDL_ESS_CLOSE | BDL_ESS_FIRST_BATCH>;
    case BDL_ESS_FIRST_IN_BATCH | BDL_ESS_CLOSE:
      return bdl_ess_fold_kernel<BDL_ESS_FIRST_IN_BATCH | BDL_ESS_CLOSE>;
    case BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH:
      return bdl_ess_fold_kernel<BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH>;
    case BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH | BDL_ESS_CLOSE | BDL_ESS_FIRST_BATCH:
      return bdl_ess_fold_kernel<BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH | BDL_ESS_CLOSE |
                                 BDL_ESS_FIRST_BATCH>;
    default: return nullptr;
  }
}

// ---------------------------------------------------------------- the report
struct EArgs {
  const float* __restrict__ sM2;
  const float* __restrict__ bM2;
  float* __restrict__ ess;
  float* __restrict__ mcse;
  bdl_ess_summary* __restrict__ partials;
  int64_t n;
  int64_t slot;
  int32_t chains;
  float fS1, fnb1, fKnb;  // S - 1, nb - 1 and K * nb as fp32
  float thr0, thr1, thr2;
};

using Stat = EssStat;  // bdl_chain_elem.hpp: the adapter EssSummary, ess_accum4, ess_finish_elem

// Float4 group gi of every chain.  GUARD: the group may be the partial last
// one (elements >= n neither read, written nor counted).
template <bool GUARD>
__device__ __forceinline__ void ess_group(const EArgs& a, int64_t gi, Stat& s) {
  const int64_t e = gi * 4;
  const f4v z = {0.f, 0.f, 0.f, 0.f};
  const f4v m0 = gload<GUARD>(a.sM2, e, a.n);
  const f4v q0 = gload<GUARD>(a.bM2, e, a.n);
  f4v SW = z, SV = z;
  ess_accum4(m0, q0, SW, SV);
  int k = 1;
  for (; k + 4 <= a.chains; k += 4) {
    f4v m[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t o = (int64_t)(k + u) * a.slot;
      m[u] = gload<GUARD>(a.sM2 + o, e, a.n);
      q[u] = gload<GUARD>(a.bM2 + o, e, a.n);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) ess_accum4(m[u], q[u], SW, SV);
  }
  for (; k < a.chains; ++k) {
    const int64_t o = (int64_t)k * a.slot;
    const f4v m = gload<GUARD>(a.sM2 + o, e, a.n);
    const f4v q = gload<GUARD>(a.bM2 + o, e, a.n);
    ess_accum4(m, q, SW, SV);
  }
  f4v es = z, mc = z;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (GUARD && e + j >= a.n) break;
    float xe, xm;
    ess_finish_elem(a, SW[j], SV[j], e + j, xe, xm, s);
    es[j] = xe;
    mc[j] = xm;
  }
  if (a.ess) gstore<GUARD>(a.ess, e, a.n, es);
  if (a.mcse) gstore<GUARD>(a.mcse, e, a.n, mc);
}

// The fold's sweep (unguarded full iterations, one guarded tail iteration; the
// loop is kept per kernel: as a shared function it re-allocates registers).
// gridDim.x <= BDL_ESS_MAX_GRID (the host's cap): one partial per workgroup.
__global__ __launch_bounds__(kBlock) void bdl_chain_ess_kernel(const EArgs a) {
  const int64_t ngroups = (a.n + 3) >> 2, nfull = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  Stat s = Stat::empty();
  int64_t gb = (int64_t)blockIdx.x * kBlock;
  for (; gb + kBlock <= nfull; gb += stride) ess_group<false>(a, gb + threadIdx.x, s);
  if (gb < ngroups) {
    const int64_t gi = gb + threadIdx.x;
    if (gi < ngroups) ess_group<true>(a, gi, s);
  }
  store_partial<EssSummary>(a.partials, s);
}

__global__ __launch_bounds__(kBlock) void bdl_chain_ess_finalize_kernel(
    const bdl_ess_summary* __restrict__ partials, int nparts, bdl_ess_summary* __restrict__ out) {
  finalize_summary<EssSummary>(partials, nparts, out);
}

// what both entry points check of the stacked layout; nullptr: fine
const char* layout_error(int32_t chains, int64_t n, uint64_t chain_groups, int32_t grid_blocks) {
  if (chains < 1 || chains > BDL_ESS_MAX_CHAINS) return "chains must be in [1, 65535]";
  if (n < 1) return "n must be >= 1";
  if (grid_blocks < 0 || grid_blocks > BDL_ESS_MAX_GRID) return "grid_blocks in [0, 2048]";
  return stacked_slot_error(chains, n, chain_groups);
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int bdl_chain_ess_fold(const bdl_ess_fold_args* d, void* stream) {
  const std::string me = "bdl_chain_ess_fold: ";
  if (const int rc = no_redirect("bdl_chain_ess_fold")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->theta) return fail(BDL_ERR_NULL, me + "null theta");
  if (!d->smean || !d->sM2 || !d->bM2)
    return fail(BDL_ERR_NULL, me + "smean, sM2 and bM2 are required");
  if (const char* why = layout_error(d->chains, d->n, d->chain_groups, d->grid_blocks))
    return fail(BDL_ERR_ARG, me + why);
  if (d->batch < 1 || d->batch >= BDL_ESS_MAX_COUNT)
    return fail(BDL_ERR_ARG, me + "batch must be in [1, 2^24)");
  if (d->sample < 1 || d->sample >= BDL_ESS_MAX_COUNT)
    return fail(BDL_ERR_ARG, me + "sample must be in [1, 2^24)");
  if (d->batch > 1 && !d->bsum) return fail(BDL_ERR_NULL, me + "bsum is required with batch > 1");
  const int64_t s = d->sample, b = d->batch, p = (s - 1) % b + 1;
  const int want = (s == 1 ? BDL_ESS_FIRST_SAMPLE : 0) | (p == 1 ? BDL_ESS_FIRST_IN_BATCH : 0) |
                   (p == b ? BDL_ESS_CLOSE : 0) | (s == b ? BDL_ESS_FIRST_BATCH : 0);
  if (d->flags != want)
    return fail(BDL_ERR_ARG, me + "flags " + std::to_string(d->flags) + " are not what sample " +
                std::to_string(s) + " of batch " + std::to_string(b) + " implies (" +
                std::to_string(want) + ")");
  if (d->fs != (float)s || d->fb != (float)b)
    return fail(BDL_ERR_ARG, me + "fs / fb are not fl32(sample) / fl32(batch)");
  if ((want & BDL_ESS_CLOSE) && !(want & BDL_ESS_FIRST_BATCH)) {
    const int64_t i = s / b;
    if (d->c != (float)((double)i / (double)(i - 1)))
      return fail(BDL_ERR_ARG, me + "c is not fl32(i/(i-1)) of the batch being closed");
  }
  float* const bsum = b > 1 ? d->bsum : nullptr;  // never touched at batch == 1
  const void* ptrs[] = {d->theta, bsum, d->smean, d->sM2, d->bM2};
  for (const void* q : ptrs)
    if (misaligned(q, 15)) return fail(BDL_ERR_ALIGN, me + "vector not 16-B aligned");
  const uint64_t bytes = 4 * (4 * d->chain_groups * (uint64_t)(d->chains - 1) + (uint64_t)d->n);
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j)
      if (overlap(ptrs[i], ptrs[j], bytes, bytes))
        return fail(BDL_ERR_ARG, me + "two vectors overlap");
  FoldKernel k = pick_fold(want);
  if (!k) return fail(BDL_ERR_ARG, me + "no kernel for these flags");

  FArgs a;
  a.theta = d->theta;
  a.bsum = bsum;
  a.smean = d->smean;
  a.sM2 = d->sM2;
  a.bM2 = d->bM2;
  a.n = d->n;
  a.slot = (int64_t)(4 * d->chain_groups);
  a.fs = d->fs;
  a.fb = d->fb;
  a.c = d->c;
  const int64_t cap = d->grid_blocks > 0
                          ? d->grid_blocks
                          : std::max<int64_t>(1, (int64_t)cu_count() * kEssBpc / d->chains);
  const int gx = (int)capped_grid(block_iters(d->n, kBlock), std::min<int64_t>(cap, BDL_ESS_MAX_GRID));
  hipLaunchKernelGGL(k, dim3(gx, d->chains), dim3(kBlock), 0, (hipStream_t)stream, a);
  return launched("bdl_chain_ess_fold");
}

int64_t bdl_chain_ess_workspace_bytes(int64_t n) {
  (void)n;
  return kPartialsOffset + (int64_t)BDL_ESS_MAX_GRID * (int64_t)sizeof(bdl_ess_summary);
}

int bdl_chain_ess(const bdl_chain_ess_args* d, void* stream) {
  const std::string me = "bdl_chain_ess: ";
  if (const int rc = no_redirect("bdl_chain_ess")) return rc;
  if (!d) return fail(BDL_ERR_NULL, me + "null args");
  if (!d->sM2 || !d->bM2) return fail(BDL_ERR_NULL, me + "sM2 and bM2 are required");
  if (!d->workspace) return fail(BDL_ERR_NULL, me + "null workspace");
  if (const char* why = layout_error(d->chains, d->n, d->chain_groups, d->grid_blocks))
    return fail(BDL_ERR_ARG, me + why);
  if (d->samples >= BDL_ESS_MAX_COUNT || d->batches >= BDL_ESS_MAX_COUNT)
    return fail(BDL_ERR_ARG, me + "samples and batches must be below 2^24 (exact in fp32)");
  if (d->samples < 2)
    return fail(BDL_ERR_ARG, me + "samples must be >= 2 (got " + std::to_string(d->samples) + ")");
  if (d->batches < 2)
    return fail(BDL_ERR_ARG, me + "batches must be >= 2 (got " + std::to_string(d->batches) + ")");
  if (d->batches > d->samples) return fail(BDL_ERR_ARG, me + "batches exceeds samples");
  const void* ptrs[] = {d->sM2, d->bM2, d->ess, d->mcse};
  for (const void* q : ptrs)
    if (misaligned(q, 15)) return fail(BDL_ERR_ALIGN, me + "vector not 16-B aligned");
  if (misaligned(d->workspace, 15)) return fail(BDL_ERR_ALIGN, me + "workspace not 16-B aligned");
  const uint64_t in = 4 * (4 * d->chain_groups * (uint64_t)(d->chains - 1) + (uint64_t)d->n);
  const uint64_t out = 4 * (uint64_t)d->n;
  const uint64_t wsb = (uint64_t)bdl_chain_ess_workspace_bytes(d->n);
  float* const outs[] = {d->ess, d->mcse};
  for (float* o : outs)
    if (overlap(d->sM2, o, in, out) || overlap(d->bM2, o, in, out) ||
        overlap(d->workspace, o, wsb, out))
      return fail(BDL_ERR_ARG, me + "an output overlaps an input or the workspace");
  if (overlap(d->ess, d->mcse, out, out)) return fail(BDL_ERR_ARG, me + "ess and mcse overlap");
  if (overlap(d->workspace, d->sM2, wsb, in) || overlap(d->workspace, d->bM2, wsb, in))
    return fail(BDL_ERR_ARG, me + "the workspace overlaps an input");

  bdl_ess_summary* summary = reinterpret_cast<bdl_ess_summary*>(d->workspace);
  bdl_ess_summary* partials = partials_of<bdl_ess_summary>(d->workspace);
  EArgs a;
  a.sM2 = d->sM2;
  a.bM2 = d->bM2;
  a.ess = d->ess;
  a.mcse = d->mcse;
  a.partials = partials;
  a.n = d->n;
  a.slot = (int64_t)(4 * d->chain_groups);
  a.chains = d->chains;
  a.fS1 = (float)(d->samples - 1);
  a.fnb1 = (float)(d->batches - 1);
  a.fKnb = (float)((int64_t)d->chains * d->batches);
  a.thr0 = d->thresholds[0];
  a.thr1 = d->thresholds[1];
  a.thr2 = d->thresholds[2];

  const int64_t cap = d->grid_blocks > 0
                          ? d->grid_blocks
                          : std::min<int64_t>((int64_t)cu_count() * kEssBpc, BDL_ESS_MAX_GRID);
  const int grid = (int)capped_grid(block_iters(d->n, kBlock), cap);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bdl_chain_ess_kernel, dim3(grid), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(bdl_chain_ess_finalize_kernel, dim3(1), dim3(kBlock), 0, st, partials, grid,
                     summary);
  return launched("bdl_chain_ess");
}

}  // extern "C"
