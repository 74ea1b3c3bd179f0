// bdl_chain_step.hip — one fused step of K stacked chains with per-chain
// hyperparameters (include/bdl_chain_step.h: the layout, the gradient forms,
// what is in scope).
//
// The launch runs on a (blocks_per_chain, K) grid: blockIdx.y is the chain, so
// a workgroup never leaves its chain.  It builds its own KArgs in registers —
// the launch's pointers shifted to the chain's slot, n = n1, no chain split
// (cgroups = 0), chain id chain + k, row k of the scalar table (block-uniform:
// read once, held in SGPRs), row k of the gradient-base table — and hands it to
// step_body of bdl_kernels.hpp: the production sweep itself (run table staged
// in LDS, fast / multi-run / guarded paths, 16-B non-temporal accesses, every
// load of an iteration issued before its arithmetic) with update_core and
// collect_core, so the arithmetic is shared with bdl_sgmcmc_step by
// construction.  The Philox counter is the group index inside the chain, with
// no division.  The sweep covers [0, n1) of the slot only: padding is never
// read or written.
//
// Some production instances re-read their arguments from the launch's kernarg
// segment (fresh_kargs() in the SGLD collect / buffer instances at depth >= 2;
// step_noise4 under BDL_PHILOX_KEYS_PER_CALL).  Here that segment does not
// hold the chain's values, so this unit is built WITHOUT that define and
// instantiates only depths for which fresh_step_args is false (unroll_ok).
#include "bdl_chain_common.hpp"
#include "bdl_chain_step.h"

#ifdef BDL_PHILOX_KEYS_PER_CALL
#error "bdl_chain_step.hip: step_noise4 must draw from the workgroup's own KArgs"
#endif

namespace bdl {
namespace {

constexpr int kChainWgPerCu = 2;  // default grid: this many workgroups per CU over all chains

// What the workgroups share: chain 0's pointers and the launch-uniform fields
// in `base`; where chain k's differ.
struct CArgs {
  KArgs base;
  int64_t slot;         // elements per slot (4 * chain_groups)
  int32_t nf_stride;    // nonfinite[k * nf_stride]
  int32_t pad;
};

__device__ __forceinline__ float uniform(float x) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

template <class T>
__device__ __forceinline__ T* shifted(T* p, int64_t off) {
  return p ? p + off : p;
}

template <int METHOD, int NOISE, int COLLECT, bool RECIP, int UNROLL>
__device__ __forceinline__ void chain_body(const CArgs& ca,
                                           const bdl_chain_scalars* __restrict__ scalars) {
  const uint32_t k = blockIdx.y;
  const int64_t off = (int64_t)k * ca.slot;
  KArgs a = ca.base;
  a.theta = shifted(a.theta, off);
  a.grad = shifted(a.grad, off);
  a.mom = shifted(a.mom, off);
  a.prior_mean = shifted(a.prior_mean, off);
  a.noise = shifted(a.noise, off);
  a.mom1 = shifted(a.mom1, off);
  a.mom2 = shifted(a.mom2, off);
  a.gbase = shifted(a.gbase, (int64_t)k * a.nruns);
  a.nonfinite = shifted(a.nonfinite, (int64_t)k * ca.nf_stride);
  a.chain += k;
  const bdl_chain_scalars& s = scalars[k];
  a.lr0 = uniform(s.lr[0]);
  a.lr1 = uniform(s.lr[1]);
  a.ns0 = uniform(s.noise_scale[0]);
  a.ns1 = uniform(s.noise_scale[1]);
  a.one_minus_alpha = uniform(s.one_minus_alpha);
  a.prior_sig = uniform(s.prior_sig);
  a.sigma2 = uniform(s.sigma2);
  a.n_data = uniform(s.n_data);
  a.mu = uniform(s.mu);
  if constexpr (RECIP && METHOD == BDL_SGLD) {
    const float i2 = uniform(s.inv_sigma2), in = uniform(s.inv_n_data);
    a.inv_s2 = i2 != 0.0f ? i2 : 1.0f / a.sigma2;  // recip_or, per chain
    a.inv_nd = in != 0.0f ? in : 1.0f / a.n_data;
  }
  // variant 0: no GRAD_READY, no clip (both refused by the entry point)
  step_body<METHOD, NOISE, COLLECT, RECIP, UNROLL, 0>(a);
}

template <int METHOD, int NOISE, int COLLECT, int UNROLL>
__global__ __launch_bounds__(kBlock) void bdl_chain_step_kernel(
    const CArgs ca, const bdl_chain_scalars* __restrict__ scalars) {
  static_assert(!fresh_step_args<METHOD, NOISE, COLLECT, UNROLL>(),
                "this instance would re-read the launch's kernarg segment");
  if (ca.base.flags & BDL_FLAG_RECIP_DIV)
    chain_body<METHOD, NOISE, COLLECT, true, UNROLL>(ca, scalars);
  else
    chain_body<METHOD, NOISE, COLLECT, false, UNROLL>(ca, scalars);
}

using ChainKernel = void (*)(const CArgs, const bdl_chain_scalars*);

template <int METHOD, int NOISE, int COLLECT>
ChainKernel pick_depth(int unroll) {
  if (unroll == 1) return bdl_chain_step_kernel<METHOD, NOISE, COLLECT, 1>;
  if constexpr (!fresh_step_args<METHOD, NOISE, COLLECT, 2>()) {
    if (unroll == 2) return bdl_chain_step_kernel<METHOD, NOISE, COLLECT, 2>;
    if (unroll == 4) return bdl_chain_step_kernel<METHOD, NOISE, COLLECT, 4>;
  }
  return nullptr;
}

template <int NOISE>
ChainKernel pick_csghmc(int collect, int unroll) {
  switch (collect) {
    case BDL_COLLECT_NONE: return pick_depth<BDL_CSGHMC, NOISE, BDL_COLLECT_NONE>(unroll);
    case BDL_COLLECT_WELFORD_INIT:
      return pick_depth<BDL_CSGHMC, NOISE, BDL_COLLECT_WELFORD_INIT>(unroll);
    case BDL_COLLECT_WELFORD: return pick_depth<BDL_CSGHMC, NOISE, BDL_COLLECT_WELFORD>(unroll);
  }
  return nullptr;
}

template <int NOISE>
ChainKernel pick_sgld(int collect, int unroll) {
  switch (collect) {
    case BDL_COLLECT_NONE: return pick_depth<BDL_SGLD, NOISE, BDL_COLLECT_NONE>(unroll);
    case BDL_COLLECT_MEAN_INIT: return pick_depth<BDL_SGLD, NOISE, BDL_COLLECT_MEAN_INIT>(unroll);
    case BDL_COLLECT_MEAN: return pick_depth<BDL_SGLD, NOISE, BDL_COLLECT_MEAN>(unroll);
  }
  return nullptr;
}

ChainKernel pick_chain(int method, int noise, int collect, int unroll) {
  if (method == BDL_CSGHMC) {
    switch (noise) {
      case BDL_NOISE_NONE: return pick_csghmc<BDL_NOISE_NONE>(collect, unroll);
      case BDL_NOISE_BUFFER: return pick_csghmc<BDL_NOISE_BUFFER>(collect, unroll);
      case BDL_NOISE_PHILOX: return pick_csghmc<BDL_NOISE_PHILOX>(collect, unroll);
    }
  } else if (method == BDL_SGLD) {
    switch (noise) {
      case BDL_NOISE_BUFFER: return pick_sgld<BDL_NOISE_BUFFER>(collect, unroll);
      case BDL_NOISE_PHILOX: return pick_sgld<BDL_NOISE_PHILOX>(collect, unroll);
    }
  }
  return nullptr;
}

// the method / noise / collect table of the header
const char* scope_error(int method, int noise, int collect) {
  if (method != BDL_CSGHMC && method != BDL_SGLD)
    return "method must be BDL_CSGHMC or BDL_SGLD (SGHMC, the *_GRAD methods and Adam have no "
           "per-chain launch)";
  if (noise < BDL_NOISE_NONE || noise > BDL_NOISE_PHILOX) return "unknown noise mode";
  if (method == BDL_SGLD && noise == BDL_NOISE_NONE)
    return "BDL_SGLD needs BDL_NOISE_BUFFER or BDL_NOISE_PHILOX";
  const bool ok = collect == BDL_COLLECT_NONE ||
                  (method == BDL_CSGHMC
                       ? (collect == BDL_COLLECT_WELFORD_INIT || collect == BDL_COLLECT_WELFORD)
                       : (collect == BDL_COLLECT_MEAN_INIT || collect == BDL_COLLECT_MEAN));
  if (!ok)
    return "collect must be NONE, or WELFORD_INIT / WELFORD for BDL_CSGHMC, MEAN_INIT / MEAN for "
           "BDL_SGLD";
  return nullptr;
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int bdl_chain_step_unroll_ok(int32_t method, int32_t noise_mode, int32_t collect, int32_t unroll) {
  if (scope_error(method, noise_mode, collect)) return 0;
  return pick_chain(method, noise_mode, collect, unroll) != nullptr ? 1 : 0;
}

int bdl_chain_step(const bdl_chain_step_args* d, void* stream) {
  const std::string W = "bdl_chain_step: ";
  if (const int rc = no_redirect("bdl_chain_step")) return rc;
  if (!d) return fail(BDL_ERR_NULL, W + "null args");
  if (d->chains < 1 || d->chains > BDL_CHAIN_STEP_MAX_CHAINS)
    return fail(BDL_ERR_ARG, W + "chains in [1, " + std::to_string(BDL_CHAIN_STEP_MAX_CHAINS) + "]");
  if (d->n1 < 1 || d->chain_groups > (uint64_t)INT64_MAX / 4 ||
      (uint64_t)d->n1 > 4 * d->chain_groups)
    return fail(BDL_ERR_ARG, W + "n1 in [1, 4 * chain_groups]");
  if ((uint64_t)d->chains * d->chain_groups > (uint64_t)INT64_MAX / 4)
    return fail(BDL_ERR_ARG, W + "chains * chain_groups too large");
  if (const char* e = scope_error(d->method, d->noise_mode, d->collect))
    return fail(BDL_ERR_ARG, W + e);
  constexpr int32_t kFlags = BDL_FLAG_FIRST_STEP | BDL_FLAG_RECIP_DIV | BDL_FLAG_MOMENTUM;
  if (d->flags & BDL_FLAG_GRAD_READY)
    return fail(BDL_ERR_ARG, W + "BDL_FLAG_GRAD_READY is not supported (the clipped step has no "
                "per-chain launch)");
  if (d->flags & ~kFlags) return fail(BDL_ERR_ARG, W + "unknown flag");
  if (!d->theta) return fail(BDL_ERR_NULL, W + "theta is required");
  if (!d->runs) return fail(BDL_ERR_NULL, W + "runs are required");
  if (!d->scalars) return fail(BDL_ERR_NULL, W + "scalars are required");
  if (d->nruns < 1 || d->nruns > BDL_CHAIN_STEP_MAX_RUNS ||
      (d->grad_base && d->nruns > BDL_CHAIN_STEP_MAX_RUNS_BASES))
    return fail(BDL_ERR_RUNS, W + "nruns in [1, 4096] (2730 with grad_base): the run table is "
                "staged in 64 KiB of LDS");
  if (!d->grad && !d->grad_base) return fail(BDL_ERR_NULL, W + "grad or grad_base is required");
  const bool sgd_mom = d->method == BDL_SGLD && (d->flags & BDL_FLAG_MOMENTUM);
  if ((d->method == BDL_CSGHMC || sgd_mom) && !d->mom)
    return fail(BDL_ERR_NULL, W + "mom is required");
  if (d->method == BDL_SGLD && !d->prior_mean)
    return fail(BDL_ERR_NULL, W + "prior_mean is required for BDL_SGLD");
  if (d->noise_mode == BDL_NOISE_BUFFER && !d->noise)
    return fail(BDL_ERR_NULL, W + "noise buffer is required");
  if (d->collect != BDL_COLLECT_NONE && !d->mom1)
    return fail(BDL_ERR_NULL, W + "mom1 is required to collect");
  const void* vecs[] = {d->theta, d->grad, d->mom, d->prior_mean, d->noise, d->mom1, d->mom2};
  for (const void* p : vecs)
    if (misaligned(p, 15)) return fail(BDL_ERR_ALIGN, W + "vector not 16-B aligned");
  if (misaligned(d->scalars, 15)) return fail(BDL_ERR_ALIGN, W + "scalars not 16-B aligned");
  if (misaligned(d->runs, 7)) return fail(BDL_ERR_ALIGN, W + "runs not 8-B aligned");
  if (misaligned(d->grad_base, 7))
    return fail(BDL_ERR_ALIGN, W + "grad_base not 8-B aligned");
  if (misaligned(d->nonfinite, 3))
    return fail(BDL_ERR_ALIGN, W + "nonfinite not 4-B aligned");
  if (d->nonfinite_per_chain != 0 && d->nonfinite_per_chain != 1)
    return fail(BDL_ERR_ARG, W + "nonfinite_per_chain is 0 or 1");
  if (d->noise_mode == BDL_NOISE_PHILOX) {
    constexpr uint64_t k2p32 = 1ull << 32;
    if (((uint64_t)d->n1 + 3) / 4 > k2p32)
      return fail(BDL_ERR_ARG, W + "Philox noise needs every float4 group index of a chain "
                  "below 2^32 (n1 / 4)");
    if (d->chain >= k2p32 || d->chain + (uint64_t)d->chains >= k2p32)
      return fail(BDL_ERR_ARG, W + "Philox noise needs every chain id below 2^32 (chain + chains)");
  }
  if (d->blocks_per_chain < 0 || d->blocks_per_chain > BDL_CHAIN_STEP_MAX_BLOCKS_PER_CHAIN)
    return fail(BDL_ERR_ARG, W + "blocks_per_chain in [0, " +
                std::to_string(BDL_CHAIN_STEP_MAX_BLOCKS_PER_CHAIN) + "]");
  if (d->unroll != 0 && d->unroll != 1 && d->unroll != 2 && d->unroll != 4)
    return fail(BDL_ERR_ARG, W + "unroll is 0, 1, 2 or 4");
  const int unroll = d->unroll ? d->unroll : 1;
  ChainKernel kern = pick_chain(d->method, d->noise_mode, d->collect, unroll);
  if (!kern)
    return fail(BDL_ERR_ARG, W + "no kernel instance at this unroll depth for this method / noise "
                "/ collect (bdl_chain_step_unroll_ok)");

  int64_t bpc = d->blocks_per_chain;
  if (bpc == 0)
    bpc = blocks_per_chain(kChainWgPerCu, d->chains,
                           std::min<int64_t>(block_iters(d->n1, (int64_t)kBlock * unroll),
                                             BDL_CHAIN_STEP_MAX_BLOCKS_PER_CHAIN));

  CArgs ca;
  memset(&ca, 0, sizeof(ca));
  KArgs& a = ca.base;
  a.theta = d->theta;
  a.grad = d->grad;
  a.mom = d->mom;
  a.prior_mean = d->prior_mean;
  a.noise = d->noise;
  a.mom1 = d->mom1;
  a.mom2 = d->mom2;
  a.runs = d->runs;
  a.gbase = d->grad_base;
  a.nruns = d->nruns;
  a.flags = d->flags;
  a.n = d->n1;
  a.groups_per_block = 0;  // the chain's workgroups advance through its slot together
  a.ca = d->collect_a;
  a.cb = d->collect_b;
  a.inv_ca = recip_or(d->inv_collect_a, d->collect_a);
  a.inv_cb = recip_or(d->inv_collect_b, d->collect_b);
  a.inv_s2 = 1.0f;  // per chain, set by the workgroup (BDL_FLAG_RECIP_DIV, BDL_SGLD)
  a.inv_nd = 1.0f;
  a.seed = d->seed;
  a.chain = d->chain;
  a.step = d->step;
  a.clip = nullptr;
  a.nonfinite = d->nonfinite;
  a.goff = 0;
  a.cgroups = 0;
  ca.slot = (int64_t)(4 * d->chain_groups);
  ca.nf_stride = d->nonfinite_per_chain;

  const size_t lds = (size_t)d->nruns * (sizeof(bdl_run) + (d->grad_base ? sizeof(int64_t) : 0));
  hipLaunchKernelGGL(kern, dim3((unsigned)bpc, (unsigned)d->chains), dim3(kBlock), lds,
                     (hipStream_t)stream, ca, d->scalars);
  return launched("bdl_chain_step");
}

}  // extern "C"
