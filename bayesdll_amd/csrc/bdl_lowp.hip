// bdl_lowp.hip — the fused SG-MCMC step on bf16 gradients with an fp32 chain
// state and a bf16 shadow of theta (include/bdl_lowp.h: the contract).
//
// The arithmetic is bdl_kernels.hpp's update_core / collect_core on the
// upcast gradient, so theta, momentum and moments are bdl_sgmcmc_step's by
// construction; only the gradient load (8 B per float4 group), the shadow
// store (8 B per group) and the sweep are this unit's own.  One loop shape
// for every method: grid-stride, a per-lane run cursor in the LDS table (as
// chunk_multi), every load of an iteration before its arithmetic.  Philox
// inputs are read from the kernel's own KArgs (this unit is built without
// BDL_PHILOX_KEYS_PER_CALL).
#include "bdl_chain_common.hpp"
#include "bdl_lowp.h"

namespace bdl {
namespace {

constexpr int kLowpBpc = 2;  // default workgroups per CU

typedef unsigned short bf16_t;
typedef bf16_t us4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) us4v gus4v;
typedef __attribute__((address_space(1))) bf16_t gbf16;

// bf16 -> fp32: exact
__device__ __forceinline__ float bf16_up(bf16_t h) { return __uint_as_float((uint32_t)h << 16); }

// fp32 -> bf16, round to nearest even (v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ bf16_t bf16_rne(float x) {
  const __bf16 b = (__bf16)x;
  return __builtin_bit_cast(bf16_t, b);
}

__device__ __forceinline__ us4v bf16_rne4(f4v x) {
  us4v o;
  o.x = bf16_rne(x.x);
  o.y = bf16_rne(x.y);
  o.z = bf16_rne(x.z);
  o.w = bf16_rne(x.w);
  return o;
}

// How a lane handles one float4 group of an iteration.
constexpr int kNone = 0;  // past the end of the vector
constexpr int kVec = 1;   // inside one non-skip run with an 8-B addressable gradient
constexpr int kElem = 2;  // element by element (run boundary, SKIP, unaligned base, tail)

// Run r's gradient base as a byte address (element i at base + 2 * i).
__device__ __forceinline__ const char* lowp_grad(const KArgs& a, int r) {
  return a.gbase ? reinterpret_cast<const char*>(lds_gbase(a.nruns)[r])
                 : reinterpret_cast<const char*>(a.grad);
}

// One block iteration from group gb on.  GUARD: it may reach past the last
// full group (elements >= n are neither read nor written).  rr: the lane's
// run cursor; a lane's groups only move forward.
template <int METHOD, int NOISE, int COLLECT, bool RECIP, int UNROLL, bool GUARD>
__device__ __forceinline__ void lowp_iter(const KArgs& a, const StepConst& c,
                                          bf16_t* __restrict__ shadow, int64_t gb, int& rr,
                                          uint32_t& bad) {
  using T = StepTraits<METHOD, COLLECT>;
  const int64_t n = a.n;
  const int64_t ngroups = (n + 3) >> 2;
  const int last = a.nruns - 1;
  const f4v z = {0.f, 0.f, 0.f, 0.f};
  f4v th[UNROLL], g[UNROLL], v[UNROLL], t0[UNROLL], ep[UNROLL], m1[UNROLL], m2[UNROLL];
  int kind[UNROLL], r0[UNROLL];
  uint32_t skip[UNROLL];  // kElem: bit j set = element j is skipped (or past n)
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    const int64_t gi = gb + (int64_t)u * kBlock + threadIdx.x;
    const int64_t e = gi * 4;
    th[u] = g[u] = v[u] = t0[u] = ep[u] = m1[u] = m2[u] = z;
    kind[u] = kNone;
    r0[u] = rr;
    skip[u] = 0;
    if (GUARD && gi >= ngroups) continue;
    while (rr < last && run_end(rr) <= e) ++rr;
    r0[u] = rr;
    const uint32_t at = run_attr(rr);
    const char* gp = lowp_grad(a, rr);
    const bool whole = !GUARD || e + 4 <= n;
    const bool vec = whole && run_end(rr) >= e + 4 && !(at & kNoFastPath) &&
                     !(reinterpret_cast<uintptr_t>(gp) & 7u);
    kind[u] = vec ? kVec : kElem;
    th[u] = gload<GUARD>(a.theta, e, n);
    if (vec) {
      const us4v h = __builtin_nontemporal_load((const gus4v*)(gp + 2 * e));
      g[u].x = bf16_up(h.x);
      g[u].y = bf16_up(h.y);
      g[u].z = bf16_up(h.z);
      g[u].w = bf16_up(h.w);
    } else {
      int r = rr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e + j >= n) {
          skip[u] |= 1u << j;
          continue;
        }
        while (r < last && run_end(r) <= e + j) ++r;
        if (run_attr(r) & BDL_ATTR_SKIP)
          skip[u] |= 1u << j;
        else
          g[u][j] = bf16_up(*(const gbf16*)(lowp_grad(a, r) + 2 * (e + j)));
      }
    }
    if (T::kMom || (METHOD == BDL_SGLD && c.sgd_mom_read)) v[u] = gload<GUARD>(a.mom, e, n);
    if (T::kReadPrior) t0[u] = gload<GUARD>(a.prior_mean, e, n);
    if (NOISE == BDL_NOISE_BUFFER) ep[u] = gload<GUARD>(a.noise, e, n);
    if (T::kReadMoments) {
      m1[u] = gload<GUARD>(a.mom1, e, n);
      if (c.has_m2) m2[u] = gload<GUARD>(a.mom2, e, n);
    }
  }
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    if (kind[u] == kNone) continue;
    const int64_t gi = gb + (int64_t)u * kBlock + threadIdx.x;
    const int64_t e = gi * 4;
    if constexpr (NOISE == BDL_NOISE_PHILOX) ep[u] = noise_from(a, gi);
    int r = r0[u];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (GUARD && e + j >= n) break;
      if (kind[u] == kElem)
        while (r < last && run_end(r) <= e + j) ++r;
      float xt = th[u][j], xg = g[u][j], xv = v[u][j], x1 = m1[u][j], x2 = m2[u][j];
      update_elem<METHOD, NOISE, COLLECT, RECIP>(a, c, run_attr(r), xt, xg, xv, t0[u][j],
                                                 ep[u][j], x1, x2);
      th[u][j] = xt;
      v[u][j] = xv;
      m1[u][j] = x1;
      m2[u][j] = x2;
    }
    bad |= nonfinite4(th[u]);  // elements past n hold 0: never flagged
    gstore<GUARD>(a.theta, e, n, th[u]);
    if (kind[u] == kVec) {
      // non-temporal like the fp32 streams: the next forward reads the shadow,
      // but at ViT-L/32 size it is 613 MB, past the 256 MiB Infinity Cache.
      // BDL_LOWP_PLAIN_SHADOW: the plain store, for the same-process A/B of
      // tools/lowp_timing.py (make flavor F=plain_shadow D=-DBDL_LOWP_PLAIN_SHADOW)
#ifdef BDL_LOWP_PLAIN_SHADOW
      *(gus4v*)(shadow + e) = bf16_rne4(th[u]);
#else
      __builtin_nontemporal_store(bf16_rne4(th[u]), (gus4v*)(shadow + e));
#endif
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!(skip[u] & (1u << j))) *(gbf16*)(shadow + e + j) = bf16_rne(th[u][j]);
    }
    if (T::kMom || (METHOD == BDL_SGLD && c.sgd_mom)) gstore<GUARD>(a.mom, e, n, v[u]);
    if (T::kCollect) {
      gstore<GUARD>(a.mom1, e, n, m1[u]);
      if (c.has_m2) gstore<GUARD>(a.mom2, e, n, m2[u]);
    }
  }
}

template <int METHOD, int NOISE, int COLLECT, bool RECIP, int UNROLL>
__device__ __forceinline__ void lowp_body(const KArgs& a, bf16_t* __restrict__ shadow) {
  // no GRAD_READY and no clip in this unit: the plain variant
  const StepConst c = make_step_const<METHOD, COLLECT, 0>(a);
  constexpr int64_t kIter = (int64_t)kBlock * UNROLL;
  const int64_t ngroups = (a.n + 3) >> 2, nfull = a.n >> 2;
  const int64_t gstep = (int64_t)gridDim.x * kIter;
  stage_runs(a);
  int64_t gb = (int64_t)blockIdx.x * kIter;
  if (gb >= ngroups) return;
  int rr = find_run_lds(a.nruns, min((gb + (int64_t)threadIdx.x) * 4, a.n - 1));
  uint32_t bad = 0;
  for (; gb < ngroups; gb += gstep) {
    if (gb + kIter <= nfull)
      lowp_iter<METHOD, NOISE, COLLECT, RECIP, UNROLL, false>(a, c, shadow, gb, rr, bad);
    else
      // the block's last, partial iteration: one group per lane at a time, guarded
      // (a rolled loop over the depth-1 body, whatever the launch's depth)
#pragma nounroll
      for (int u = 0; u < UNROLL; ++u)
        lowp_iter<METHOD, NOISE, COLLECT, RECIP, 1, true>(a, c, shadow, gb + (int64_t)u * kBlock,
                                                          rr, bad);
  }
  report_nonfinite(a, bad);
}

template <int METHOD, int NOISE, int COLLECT, int UNROLL>
__global__ __launch_bounds__(kBlock) void bdl_lowp_kernel(const KArgs a, bf16_t* shadow) {
  if (a.flags & BDL_FLAG_RECIP_DIV)
    lowp_body<METHOD, NOISE, COLLECT, true, UNROLL>(a, shadow);
  else
    lowp_body<METHOD, NOISE, COLLECT, false, UNROLL>(a, shadow);
}

// shadow = bf16(theta): four groups per lane and iteration, 16-B loads, 8-B
// stores; the tail n % 4 element by element.
__global__ __launch_bounds__(kBlock) void bdl_lowp_shadow_kernel(const float* __restrict__ theta,
                                                                  bf16_t* __restrict__ shadow,
                                                                  int64_t n) {
  const int64_t nfull = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x; gi < nfull; gi += stride)
    __builtin_nontemporal_store(bf16_rne4(vload(theta + gi * 4)),
                                (gus4v*)(shadow + gi * 4));
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = nfull * 4 + threadIdx.x;
    *(gbf16*)(shadow + i) = bf16_rne(sload(theta + i));
  }
}

using LowpKernel = void (*)(const KArgs, bf16_t*);

template <int METHOD, int NOISE, int COLLECT>
LowpKernel lowp_unroll(int unroll) {
  switch (unroll) {
    case 1:
      return bdl_lowp_kernel<METHOD, NOISE, COLLECT, 1>;
    case 2:
      return bdl_lowp_kernel<METHOD, NOISE, COLLECT, 2>;
    case 4:
      return bdl_lowp_kernel<METHOD, NOISE, COLLECT, 4>;
  }
  return nullptr;
}

// The instances: the collect kinds each method's Runner uses (Welford for
// cSGHMC, running means for SGLD / SGHMC) and, for SGLD / SGHMC, the
// noise-bearing forms only.  Other combinations have no kernel (BDL_ERR_ARG):
// 63 kernels instead of 135 keep this unit's build time beside the others'.
template <int METHOD, int NOISE>
LowpKernel lowp_collect(int collect, int unroll) {
  constexpr bool kWelford = METHOD == BDL_CSGHMC;
  switch (collect) {
    case BDL_COLLECT_NONE:
      return lowp_unroll<METHOD, NOISE, BDL_COLLECT_NONE>(unroll);
    case BDL_COLLECT_WELFORD_INIT:
      if constexpr (kWelford) return lowp_unroll<METHOD, NOISE, BDL_COLLECT_WELFORD_INIT>(unroll);
      break;
    case BDL_COLLECT_WELFORD:
      if constexpr (kWelford) return lowp_unroll<METHOD, NOISE, BDL_COLLECT_WELFORD>(unroll);
      break;
    case BDL_COLLECT_MEAN_INIT:
      if constexpr (!kWelford) return lowp_unroll<METHOD, NOISE, BDL_COLLECT_MEAN_INIT>(unroll);
      break;
    case BDL_COLLECT_MEAN:
      if constexpr (!kWelford) return lowp_unroll<METHOD, NOISE, BDL_COLLECT_MEAN>(unroll);
      break;
  }
  return nullptr;
}

template <int METHOD>
LowpKernel lowp_noise(int noise, int collect, int unroll) {
  switch (noise) {
    case BDL_NOISE_NONE:
      if constexpr (METHOD == BDL_CSGHMC)
        return lowp_collect<METHOD, BDL_NOISE_NONE>(collect, unroll);
      break;
    case BDL_NOISE_BUFFER:
      return lowp_collect<METHOD, BDL_NOISE_BUFFER>(collect, unroll);
    case BDL_NOISE_PHILOX:
      return lowp_collect<METHOD, BDL_NOISE_PHILOX>(collect, unroll);
  }
  return nullptr;
}

LowpKernel pick_lowp(int method, int noise, int collect, int unroll) {
  switch (method) {
    case BDL_CSGHMC:
      return lowp_noise<BDL_CSGHMC>(noise, collect, unroll);
    case BDL_SGHMC:
      return lowp_noise<BDL_SGHMC>(noise, collect, unroll);
    case BDL_SGLD:
      return lowp_noise<BDL_SGLD>(noise, collect, unroll);
  }
  return nullptr;
}

}  // namespace
}  // namespace bdl

using namespace bdl;

extern "C" {

int bdl_lowp_step(const bdl_lowp_args* s, void* stream) {
  const std::string me = "bdl_lowp_step: ";
  if (const int rc = no_redirect("bdl_lowp_step")) return rc;
  if (!s) return fail(BDL_ERR_NULL, me + "null args");
  if (s->n <= 0) return fail(BDL_ERR_ARG, me + "n must be >= 1");
  if (s->method != BDL_CSGHMC && s->method != BDL_SGHMC && s->method != BDL_SGLD)
    return fail(BDL_ERR_ARG, me + "method must be BDL_CSGHMC, BDL_SGHMC or BDL_SGLD (the *_GRAD "
                "and Adam methods have no bf16 form)");
  constexpr int32_t kFlags = BDL_FLAG_FIRST_STEP | BDL_FLAG_RECIP_DIV | BDL_FLAG_MOMENTUM;
  if (s->flags & BDL_FLAG_GRAD_READY)
    return fail(BDL_ERR_ARG, me + "BDL_FLAG_GRAD_READY is not supported (no clipped bf16 step)");
  if (s->flags & ~kFlags) return fail(BDL_ERR_ARG, me + "unknown flag bit");
  if (s->noise_mode < BDL_NOISE_NONE || s->noise_mode > BDL_NOISE_PHILOX)
    return fail(BDL_ERR_ARG, me + "unknown noise mode");
  if (s->collect < BDL_COLLECT_NONE || s->collect > BDL_COLLECT_MEAN)
    return fail(BDL_ERR_ARG, me + "unknown collect mode");
  if (s->unroll != 1 && s->unroll != 2 && s->unroll != 4)
    return fail(BDL_ERR_ARG, me + "unroll must be 1, 2 or 4");
  if (s->blocks < 0 || s->blocks > BDL_LOWP_MAX_BLOCKS)
    return fail(BDL_ERR_ARG, me + "blocks in [0, " + std::to_string(BDL_LOWP_MAX_BLOCKS) + "]");
  if (!s->theta) return fail(BDL_ERR_NULL, me + "theta is required");
  if (!s->shadow) return fail(BDL_ERR_NULL, me + "shadow is required");
  if (!s->runs || s->nruns < 1) return fail(BDL_ERR_NULL, me + "runs are required");
  if (!s->grad && !s->grad_base) return fail(BDL_ERR_NULL, me + "grad or grad_base is required");
  const bool needs_mom = s->method != BDL_SGLD || (s->flags & BDL_FLAG_MOMENTUM);
  if (needs_mom && !s->mom) return fail(BDL_ERR_NULL, me + "mom is required");
  if (s->method != BDL_CSGHMC && !s->prior_mean)
    return fail(BDL_ERR_NULL, me + "prior_mean is required for sghmc/sgld");
  if (s->noise_mode == BDL_NOISE_BUFFER && !s->noise)
    return fail(BDL_ERR_NULL, me + "noise buffer is required");
  if (s->collect != BDL_COLLECT_NONE && !s->mom1)
    return fail(BDL_ERR_NULL, me + "mom1 is required to collect");
  const void* v16[] = {s->theta, s->mom, s->prior_mean, s->noise, s->mom1, s->mom2};
  for (const void* p : v16)
    if (misaligned(p, 15)) return fail(BDL_ERR_ALIGN, me + "fp32 vector not 16-B aligned");
  if (misaligned(s->shadow, 7)) return fail(BDL_ERR_ALIGN, me + "shadow not 8-B aligned");
  if (misaligned(s->grad, 7)) return fail(BDL_ERR_ALIGN, me + "grad not 8-B aligned");
  if (misaligned(s->grad_base, 7)) return fail(BDL_ERR_ALIGN, me + "grad_base not 8-B aligned");
  const size_t lds = (size_t)s->nruns * (sizeof(bdl_run) + (s->grad_base ? sizeof(int64_t) : 0));
  if (lds > (size_t)kMaxRuns * sizeof(bdl_run))
    return fail(BDL_ERR_RUNS, me + "run table exceeds 64 KiB of LDS (4096 runs, 2730 with "
                "grad_base)");
  constexpr uint64_t k2p32 = 1ull << 32;
  const uint64_t groups = (uint64_t)((s->n + 3) / 4);
  if (s->chain_groups || s->noise_mode == BDL_NOISE_PHILOX) {
    if (s->chain_groups >= k2p32 || s->philox_offset >= k2p32 ||
        groups + s->philox_offset >= k2p32)
      return fail(BDL_ERR_ARG, me + "every float4 group index must stay below 2^32 "
                  "(chain_groups, n / 4 + philox_offset)");
  }
  if (s->noise_mode == BDL_NOISE_PHILOX) {
    const uint64_t nchains =
        s->chain_groups ? (groups + s->philox_offset + s->chain_groups - 1) / s->chain_groups : 0;
    if (s->chain >= k2p32 || s->chain + nchains >= k2p32)
      return fail(BDL_ERR_ARG, me + "Philox noise needs every chain id below 2^32 (chain, plus "
                  "the number of stacked chains)");
  }
  LowpKernel k = pick_lowp(s->method, s->noise_mode, s->collect, s->unroll);
  if (!k) return fail(BDL_ERR_ARG, me + "no kernel for this method/noise/collect combination");

  const int64_t grid =
      s->blocks > 0 ? s->blocks
                    : capped_grid(block_iters(s->n, (int64_t)kBlock * s->unroll),
                                  (int64_t)cu_count() * kLowpBpc);

  KArgs a{};
  a.theta = s->theta;
  a.grad = reinterpret_cast<float*>(const_cast<uint16_t*>(s->grad));  // bf16: lowp_grad
  a.mom = s->mom;
  a.prior_mean = s->prior_mean;
  a.noise = s->noise;
  a.mom1 = s->mom1;
  a.mom2 = s->mom2;
  a.runs = s->runs;
  a.gbase = s->grad_base;
  a.nruns = s->nruns;
  a.flags = s->flags;
  a.n = s->n;
  a.groups_per_block = 0;
  a.lr0 = s->lr[0];
  a.lr1 = s->lr[1];
  a.ns0 = s->noise_scale[0];
  a.ns1 = s->noise_scale[1];
  a.one_minus_alpha = s->one_minus_alpha;
  a.prior_sig = s->prior_sig;
  a.sigma2 = s->sigma2;
  a.n_data = s->n_data;
  a.mu = s->mu;
  a.ca = s->collect_a;
  a.cb = s->collect_b;
  a.seed = s->seed;
  a.chain = s->chain;
  a.step = s->step;
  a.clip = nullptr;
  a.nonfinite = s->nonfinite;
  a.goff = s->philox_offset;
  a.cgroups = (uint32_t)s->chain_groups;
  a.inv_s2 = recip_or(s->inv_sigma2, s->sigma2);
  a.inv_nd = recip_or(s->inv_n_data, s->n_data);
  a.inv_ca = recip_or(s->inv_collect_a, s->collect_a);
  a.inv_cb = recip_or(s->inv_collect_b, s->collect_b);

  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), lds, (hipStream_t)stream, a,
                     s->shadow);
  return launched("bdl_lowp_step");
}

int bdl_lowp_shadow(const float* theta, uint16_t* shadow, const bdl_run* runs, int32_t nruns,
                    int64_t n, void* stream) {
  const std::string me = "bdl_lowp_shadow: ";
  (void)runs;  // every element is written, whatever its run's attributes
  if (const int rc = no_redirect("bdl_lowp_shadow")) return rc;
  if (!theta) return fail(BDL_ERR_NULL, me + "null theta");
  if (!shadow) return fail(BDL_ERR_NULL, me + "null shadow");
  if (n <= 0) return fail(BDL_ERR_ARG, me + "n must be >= 1");
  if (nruns < 0) return fail(BDL_ERR_ARG, me + "nruns < 0");
  if (misaligned(theta, 15)) return fail(BDL_ERR_ALIGN, me + "theta not 16-B aligned");
  if (misaligned(shadow, 7)) return fail(BDL_ERR_ALIGN, me + "shadow not 8-B aligned");
  const int64_t want = ((n >> 2) + kBlock - 1) / kBlock;
  const int64_t grid = capped_grid(want, (int64_t)cu_count() * 4);
  hipLaunchKernelGGL(bdl_lowp_shadow_kernel, dim3((unsigned)grid), dim3(kBlock), 0,
                     (hipStream_t)stream, theta, shadow, n);
  return launched("bdl_lowp_shadow");
}

}  // extern "C"
