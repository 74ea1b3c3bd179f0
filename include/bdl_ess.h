/* bdl_ess.h — effective sample size of stacked chains by batch means.
 *
 * K chains of one network keep their state side by side in one buffer (chain
 * k, element j at 4*chain_groups*k + j: bayesdll_amd.stacked).  The thinned
 * samples of an SG-MCMC chain are autocorrelated, and neither the samplers'
 * moments nor R-hat say how many independent samples they stand for.  Batch
 * means does, without a sample history: the variance of the means of batches
 * of b consecutive samples against the variance of the samples.
 * bdl_chain_ess_fold folds one collected sample of every chain into four fp32
 * accumulators laid out like theta; bdl_chain_ess turns them into the
 * per-element ESS, a Monte Carlo standard error of the mean, and a summary
 * over the vector.  Purely additive to the ABI of bdl_sgmcmc.h (same
 * status codes, bdl_last_error, stream convention).
 *
 * Accumulators (each stacked like theta):
 *   bsum   sum of the open batch
 *   smean  Welford mean over all folded samples (the true count)
 *   sM2    Welford M2 over all folded samples
 *   bM2    M2 of the closed batches' means.  Their mean is not stored: at a
 *          close it equals smean, and Welford's update with the new mean alone
 *          is M2 += (y - mean_new)^2 * i/(i-1).
 *
 * Fold arithmetic (part of the contract; tests/chain_ess_ref.py restates it).
 * s = 1-based index of the sample, b = batch length, p = (s-1) % b + 1 its
 * position in the batch, i = s / b at a close; fs = fl32(s), fb = fl32(b),
 * c = fl32(i/(i-1)) formed in float64 by the host.  One fp32 rounding per
 * line, every / the correctly rounded IEEE division:
 *
 *   x = theta
 *   FIRST_SAMPLE:   smean' = x;  sM2' = 0
 *   else:           d = x - smean;  q = d / fs;  smean' = smean + q
 *                   d2 = x - smean';  t = d * d2;  sM2' = sM2 + t
 *   FIRST_IN_BATCH: bs = x           else: bs = bsum + x
 *   not CLOSE:      bsum' = bs
 *   CLOSE:          y = bs / fb
 *     FIRST_BATCH:  bM2' = 0         else: e = y - smean';  t = e * e
 *                                          u = t * c;  bM2' = bM2 + u
 *
 * A vector a fold does not need is neither read nor written (bsum at b == 1,
 * where every fold is FIRST_IN_BATCH and CLOSE; bM2 on a fold that closes no
 * batch; the old smean / sM2 / bM2 / bsum where the flag says they are
 * overwritten): 24-32 bytes per element.  Elements [n, 4*chain_groups) of a
 * chain slot are neither read nor written.
 *
 * Report arithmetic.  S = samples folded per chain, nb = closed batches,
 * chains k ascending from 0, SW = SV = 0 before chain 0, one rounding per line:
 *
 *   SW = SW + sM2_k;  SV = SV + bM2_k
 *   w = SW / fl32(S-1);  v = SV / fl32(nb-1);  r = w / v;  ess = r * fl32(K*nb)
 *   g = v / fl32(K*nb);  mcse = sqrt(g)
 *
 * Per chain this is nb * s^2 / vb = S * s^2 / (b * vb), the batch-means ESS,
 * pooled over chains the way R-hat pools W.  v is the SUM of the chains'
 * batch variances, so mcse = sqrt(mean_k vb_k / nb): the standard error of ONE
 * chain's mean from the pooled batch variance (the mean over all K chains has
 * mcse / sqrt(K); with chains = 1 the two coincide).
 *
 * Conventions (those of bdl_diag.h).  SV == 0 (frozen parameters, chains that
 * never moved) is degenerate: ess is written as NaN and the element stays out
 * of the statistics; mcse is written as computed.  Any other element whose
 * ess is NaN or Inf is counted in n_nonfinite, written as computed, and stays
 * out too.  The summary is reduced without atomics: one partial per workgroup
 * (wavefront shuffles + LDS), then one workgroup combines the partials in a
 * fixed order.  Counts, ess_min and argmin are exact and independent of the
 * launch geometry; ess_sum differs between geometries only in fp64 rounding. */
#ifndef BDL_ESS_H
#define BDL_ESS_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

enum bdl_ess_flag {
  BDL_ESS_FIRST_SAMPLE = 0x1,   /* s == 1                                   */
  BDL_ESS_FIRST_IN_BATCH = 0x2, /* p == 1                                   */
  BDL_ESS_CLOSE = 0x4,          /* p == b: the sample closes its batch      */
  BDL_ESS_FIRST_BATCH = 0x8     /* s == b: the batch closed is the first    */
};

#define BDL_ESS_MAX_COUNT (1 << 24)  /* sample, batch, samples, batches < this: exact in fp32 */
#define BDL_ESS_MAX_CHAINS 65535     /* chains <= this (the fold grid's y extent)             */
#define BDL_ESS_MAX_GRID 2048        /* grid_blocks <= this                                   */

typedef struct bdl_ess_fold_args {
  const float* theta;    /* stacked: chain k, element j at 4*chain_groups*k + j      */
  float* bsum;           /* same layout; nullable when batch == 1 (never touched)    */
  float* smean;
  float* sM2;
  float* bM2;
  int64_t n;             /* elements per chain folded, 1 <= n <= 4*chain_groups       */
  uint64_t chain_groups;
  int64_t sample;        /* s, 1 <= s < BDL_ESS_MAX_COUNT                             */
  int64_t batch;         /* b, 1 <= b < BDL_ESS_MAX_COUNT                             */
  int32_t chains;        /* K, 1 .. BDL_ESS_MAX_CHAINS                                */
  int32_t flags;         /* bdl_ess_flag bits; must be the ones (sample, batch) imply */
  float fs, fb;          /* fl32(s), fl32(b)                                          */
  float c;               /* fl32(i/(i-1)), i = s/b, on a CLOSE that is not the first
                            batch's; ignored otherwise                                */
  int32_t grid_blocks;   /* workgroups per chain, 1 .. BDL_ESS_MAX_GRID (0: default,
                            about two per CU over all chains)                         */
} bdl_ess_fold_args;

typedef struct bdl_ess_summary {    /* written at the start of the workspace */
  int64_t n_eval;        /* elements that entered the statistics                     */
  int64_t n_degenerate;  /* SV == 0                                                  */
  int64_t n_nonfinite;   /* ess NaN/Inf (excluded from the statistics)               */
  int64_t argmin;        /* lowest element index attaining ess_min; -1 if n_eval==0  */
  int64_t n_below[3];    /* ess < thresholds[i], strictly                            */
  double  ess_sum;       /* over the n_eval elements                                 */
  float   ess_min;       /* 0 if n_eval == 0                                         */
  float   pad;
} bdl_ess_summary;

typedef struct bdl_chain_ess_args {
  const float* sM2;      /* stacked: chain k, element j at 4*chain_groups*k + j      */
  const float* bM2;      /* same layout                                              */
  float* ess;            /* nullable; n elements                                     */
  float* mcse;           /* nullable; n elements                                     */
  void*  workspace;      /* bdl_chain_ess_workspace_bytes(n) bytes, 16-B aligned     */
  int64_t n;             /* elements per chain evaluated, 1 <= n <= 4*chain_groups   */
  uint64_t chain_groups;
  int64_t samples;       /* S folded per chain, 2 <= S < BDL_ESS_MAX_COUNT           */
  int64_t batches;       /* nb closed per chain, 2 <= nb <= S                        */
  int32_t chains;        /* K, 1 .. BDL_ESS_MAX_CHAINS (1: one chain's slice alone)  */
  int32_t grid_blocks;   /* workgroups of the sweep, 1 .. BDL_ESS_MAX_GRID (0:
                            default, two per CU)                                     */
  float thresholds[3];
  int32_t pad0;
} bdl_chain_ess_args;

/* One launch on hip_stream over a (grid_blocks, chains) grid; no host
 * synchronisation, no allocation.  Validation comes before any HIP call:
 * BDL_ERR_NULL (args, theta, smean, sM2, bM2; bsum with batch > 1),
 * BDL_ERR_ALIGN (a vector not 16-B aligned), BDL_ERR_ARG (chains, n,
 * chain_groups, sample, batch or grid_blocks out of range; chains *
 * chain_groups overflowing the element index; flags, fs, fb or c that are not
 * what (sample, batch) imply; two vectors overlapping; or a graph redirect
 * active on the thread). */
int bdl_chain_ess_fold(const bdl_ess_fold_args* args, void* hip_stream);

/* Device scratch of one bdl_chain_ess call: the summary, then the
 * per-workgroup partials.  Independent of n today; pass n all the same. */
int64_t bdl_chain_ess_workspace_bytes(int64_t n);

/* Two launches on hip_stream (the sweep, the one-workgroup combine), no host
 * synchronisation, no allocation.  Only elements [0, n) of each output are
 * written, only bdl_chain_ess_workspace_bytes(n) bytes of the workspace, and
 * the padding tail of a chain's slot is never read.  Validation comes before
 * any HIP call: BDL_ERR_NULL (args, sM2, bM2, workspace), BDL_ERR_ALIGN (a
 * vector or the workspace not 16-B aligned), BDL_ERR_ARG (chains, n,
 * chain_groups or grid_blocks out of range; samples < 2, batches < 2,
 * batches > samples, a counter >= BDL_ESS_MAX_COUNT; chains * chain_groups
 * overflowing the element index; an output overlapping an input, the other
 * output or the workspace; or a graph redirect active on the thread). */
int bdl_chain_ess(const bdl_chain_ess_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_ESS_H */
