/* bdl_chain_step.h — one fused step of K stacked chains, each with its own
 * hyperparameters.
 *
 * K chains of one network are stepped by one launch (bayesdll_amd.stacked).
 * bdl_sgmcmc_step with chain_groups gives them one set of scalars; here chain
 * k reads row k of a device table of scalars, so that K chains are a K-point
 * sweep over lr, prior_sig, momentum_decay, nd, Ninflate (or a ladder of
 * noise discounts) in the time of one run.  Purely additive to the ABI of
 * bdl_sgmcmc.h (same status codes, bdl_last_error, stream convention, enums,
 * attribute bits and flags).
 *
 * Layout.  Every vector holds K consecutive slots of 4*chain_groups elements;
 * chain k's element j (0 <= j < n1 <= 4*chain_groups) is at
 * vector + 4*chain_groups*k + j.  The elements of a slot beyond n1 (its
 * padding) are never read and never written.  The run table describes ONE
 * chain in chain-local element indices (last end == n1) and is shared by all
 * chains.
 *
 * Gradients, two forms:
 *   - grad_base == NULL: the stacked gradient vector `grad`, laid out as above;
 *   - grad_base != NULL: a device table of K x nruns byte addresses; chain k
 *     reads run r's gradient for chain-local element j at
 *     ((float*)grad_base[k*nruns + r])[j], i.e. the entry is
 *     &g_t[k, 0] - 4*offset_t for the vmapped [K, numel_t] gradient of the
 *     tensor t that run r covers.  Runs must not span two tensors; SKIP runs
 *     may hold 0; a run for which ANY chain's base is not 16-byte addressable
 *     carries BDL_ATTR_GUNALIGNED in the (shared) run table.  `grad` may be
 *     null.  Serves any K for a network of up to 2730 runs.
 *
 * Values.  Chain k's elements are updated by the per-element update and
 * collect of bdl_sgmcmc_step (the same device functions), with lr,
 * noise_scale, one_minus_alpha, prior_sig, sigma2, n_data, mu and the two
 * reciprocals from scalars[k], the launch-uniform collect_a / collect_b, and
 * — with BDL_NOISE_PHILOX — the stream of a one-chain launch with chain id
 * chain + k: counter (group index inside the chain, chain + k, step), key
 * seed.  Chain k of this launch therefore equals, bit for bit, a one-chain
 * bdl_sgmcmc_step launch over chain k's slot with chain k's scalars.  Values
 * never depend on blocks_per_chain or unroll.
 *
 * In scope:
 *   BDL_CSGHMC  noise NONE / BUFFER / PHILOX, collect NONE / WELFORD_INIT /
 *               WELFORD;
 *   BDL_SGLD    noise BUFFER / PHILOX, collect NONE / MEAN_INIT / MEAN,
 *               BDL_FLAG_MOMENTUM, BDL_FLAG_FIRST_STEP;
 *   BDL_FLAG_RECIP_DIV for both.  mu is per chain but BDL_FLAG_MOMENTUM is one
 *   flag: the caller keeps mu all zero (flag clear) or all non-zero (flag set).
 * Everything else (SGHMC, the *_GRAD methods, BDL_FLAG_GRAD_READY, Adam, the
 * clipped step) is refused with BDL_ERR_ARG. */
#ifndef BDL_CHAIN_STEP_H
#define BDL_CHAIN_STEP_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_CHAIN_STEP_MAX_CHAINS 65535            /* chains <= this (the grid's y extent) */
#define BDL_CHAIN_STEP_MAX_BLOCKS_PER_CHAIN 4096   /* blocks_per_chain <= this             */
#define BDL_CHAIN_STEP_MAX_RUNS 4096               /* nruns <= this ...                    */
#define BDL_CHAIN_STEP_MAX_RUNS_BASES 2730         /* ... and this with grad_base (LDS)    */

typedef struct bdl_chain_scalars {   /* chain k's row, fp32, rounded once from the host's float64 */
  float lr[2], noise_scale[2];       /* as bdl_step_args: index 0 body group, 1 head group        */
  float one_minus_alpha, prior_sig, sigma2, n_data, mu;
  float inv_sigma2, inv_n_data;      /* as bdl_step_args.inv_*; 0 -> 1/fl32(s) */
  float pad;
} bdl_chain_scalars;                  /* 48 B */

typedef struct bdl_chain_step_args {
  /* stacked vectors (device, fp32, 16-B aligned, chains * 4*chain_groups elements) */
  float* theta;               /* in/out                                              */
  float* grad;                /* in; may be null with grad_base                      */
  float* mom;                 /* cSGHMC momentum; SGLD: SGD buffer (BDL_FLAG_MOMENTUM) */
  const float* prior_mean;    /* SGLD: theta0; unused by cSGHMC                      */
  const float* noise;         /* BDL_NOISE_BUFFER only                               */
  float* mom1;                /* collect only                                        */
  float* mom2;                /* collect only; may be null                           */
  int32_t* nonfinite;         /* divergence guard (nullable): one flag, or one per
                                 chain (nonfinite_per_chain), set to 1 (atomic OR)
                                 when chain k writes a theta that is NaN or +-Inf   */
  const bdl_run* runs;        /* DEVICE: one chain's run table, chain-local ends     */
  const int64_t* grad_base;   /* DEVICE: chains x nruns byte bases, or null          */
  const bdl_chain_scalars* scalars; /* DEVICE: chains rows, 16-B aligned             */
  int64_t n1;                 /* elements per chain, 1 .. 4*chain_groups             */
  uint64_t chain_groups;      /* slot size in float4 groups                          */
  int32_t nruns;              /* 1 .. 4096 (2730 with grad_base)                     */
  int32_t chains;             /* K, 1 .. BDL_CHAIN_STEP_MAX_CHAINS                   */
  int32_t method;             /* BDL_CSGHMC or BDL_SGLD                              */
  int32_t noise_mode;         /* bdl_noise_mode                                      */
  int32_t collect;            /* bdl_collect                                         */
  int32_t flags;              /* BDL_FLAG_FIRST_STEP | RECIP_DIV | MOMENTUM          */
  int32_t blocks_per_chain;   /* workgroups per chain, 1 .. BDL_CHAIN_STEP_MAX_BLOCKS_PER_CHAIN
                                 (0: default, about two workgroups per CU over all chains) */
  int32_t unroll;             /* float4 groups in flight per lane: 0 (= 1), 1, 2 or 4,
                                 where bdl_chain_step_unroll_ok says so              */
  int32_t nonfinite_per_chain;/* 0: nonfinite[0] for every chain; 1: nonfinite[k]    */
  int32_t pad0;
  /* launch-uniform: all chains collect on the same steps */
  float collect_a;            /* WELFORD: n; MEAN: multiplier of the old moment      */
  float collect_b;            /* MEAN: divisor                                       */
  float inv_collect_a;        /* as bdl_step_args.inv_*; 0 -> 1/fl32(s)              */
  float inv_collect_b;
  uint64_t seed;              /* Philox key                                          */
  uint64_t chain;             /* chain 0's id; chain k is keyed chain + k            */
  uint64_t step;              /* global step counter                                 */
} bdl_chain_step_args;

/* Host-only: 1 if bdl_chain_step has a kernel instance for this combination
 * at this unroll depth (1, 2 or 4), else 0.  Depth 1 exists for every
 * combination in scope; cSGHMC has every depth; SGLD has depths 2 and 4 only
 * for Philox noise without a collect. */
int bdl_chain_step_unroll_ok(int32_t method, int32_t noise_mode, int32_t collect, int32_t unroll);

/* One launch on hip_stream over a (blocks_per_chain, chains) grid: a workgroup
 * never leaves its chain and reads that chain's scalars once.  No host
 * synchronisation, no allocation.
 *
 * Validation comes before any HIP call: BDL_ERR_NULL (args, theta, runs,
 * scalars, grad and grad_base both null, mom / prior_mean / noise / mom1
 * missing where the method, noise mode or collect needs it), BDL_ERR_ALIGN (a
 * vector or scalars not 16-B aligned, runs or grad_base not 8-B aligned,
 * nonfinite not 4-B aligned), BDL_ERR_RUNS (nruns outside [1, 4096], or above
 * 2730 with grad_base), BDL_ERR_ARG (chains outside [1, 65535], n1 < 1 or
 * n1 > 4*chain_groups, a method / noise mode / collect / flag outside the
 * table above, blocks_per_chain or unroll out of range, a Philox launch whose
 * group index (n1 + 3) / 4 or chain id chain + chains would reach 2^32, or a
 * graph redirect active on the thread).  The run table, the base table and
 * the scalars live in device memory, so their ENTRIES cannot be validated on
 * the host: the caller guarantees sorted chain-local ends with the last equal
 * to n1 and bases that keep every access inside an allocation. */
int bdl_chain_step(const bdl_chain_step_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_CHAIN_STEP_H */
