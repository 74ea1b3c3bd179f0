/* bdl_diag.h — cross-chain convergence diagnostic of stacked chains.
 *
 * K chains of one network keep their posterior moments side by side in one
 * buffer (chain k, element j at 4*chain_groups*k + j: bayesdll_amd.stacked,
 * bdl_step_args.chain_groups).  bdl_chain_diag reads the K chains' (mom1,
 * mom2) once — 8*K bytes per element — and gives, per element, the
 * Gelman-Rubin potential scale reduction (R-hat) and the pooled Gaussian
 * posterior (the moment-matched mixture of the K per-chain Gaussians), plus a
 * summary of R-hat over the vector.  Purely additive to the ABI of
 * bdl_sgmcmc.h (same status codes, bdl_last_error, stream convention).
 *
 * Arithmetic (part of the contract; tests/chain_diag_ref.py restates it).
 * Every line is one fp32 rounding, every / and sqrt is the correctly rounded
 * IEEE operation, k ascends from 0, K and K-1 enter as fp32 values:
 *
 *   v_k  = the variance bdl_posterior_sample takes the sqrt of, from
 *          (mom1_k, mom2_k) under var_mode / ratio / inv_ratio, clamped at
 *          var_floor (NaN stays NaN) — the same device function
 *   S1 = S2 = SW = 0
 *   for k = 0 .. K-1:
 *     d  = m_k - m_0
 *     S1 = S1 + d
 *     t  = d * d
 *     S2 = S2 + t
 *     SW = SW + v_k
 *   q    = S1 / K
 *   mbar = m_0 + q
 *   p    = S1 * S1
 *   r    = p / K
 *   u    = S2 - r
 *   ss   = u < 0 ? 0 : u          (sum of squared deviations from mbar; NaN stays NaN)
 *   Bn   = ss / (K-1)
 *   W    = SW / K
 *   a    = W * c1
 *   b    = a + Bn
 *   c    = b / W
 *   rhat = sqrt(c)
 *   e    = ss / K
 *   pooled_mean = mbar;  pooled_var = W + e
 *
 * c1 = fl32((count-1)/count), count = samples collected per chain.  Shifting
 * by chain 0's own value bounds the cancellation in ss (m_0 is one of the
 * samples) at five VALU ops per (chain, element) and no per-chain division.
 *
 * Conventions.  An element with S2 == 0 (every chain's mean equal to chain
 * 0's: frozen parameters, chains that never moved apart) is degenerate: its
 * rhat is written as NaN and it stays out of the statistics; pooled_* are
 * still written.  Any other element whose rhat is NaN or Inf is counted in
 * n_nonfinite, written as computed, and stays out of the statistics too.
 *
 * The summary is reduced without atomics: one partial per workgroup
 * (wavefront shuffles + LDS; counts, max with lowest index, an fp64 sum of
 * the fp32 rhat values), then one workgroup combines the partials in a fixed
 * order.  Counts, rhat_max and argmax are exact and independent of the launch
 * geometry; rhat_sum differs between geometries only in fp64 rounding. */
#ifndef BDL_DIAG_H
#define BDL_DIAG_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bdl_diag_summary {   /* written at the start of the workspace */
  int64_t n_eval;        /* elements that entered the statistics                    */
  int64_t n_degenerate;  /* every chain's mean bit-equal to chain 0's (S2 == 0)     */
  int64_t n_nonfinite;   /* rhat NaN/Inf (excluded from the statistics)             */
  int64_t argmax;        /* lowest element index attaining rhat_max; -1 if n_eval==0 */
  int64_t n_above[3];    /* rhat > thresholds[i], strictly                          */
  double  rhat_sum;      /* over the n_eval elements                                */
  float   rhat_max;      /* 0 if n_eval == 0                                        */
  float   pad;
} bdl_diag_summary;

typedef struct bdl_chain_diag_args {
  const float* mom1;     /* stacked: chain k, element j at 4*chain_groups*k + j     */
  const float* mom2;     /* same layout; variance source per var_mode               */
  float* pooled_mean;    /* nullable; n elements                                     */
  float* pooled_var;     /* nullable; n elements                                     */
  float* rhat;           /* nullable; n elements                                     */
  void*  workspace;      /* bdl_chain_diag_workspace_bytes(n) bytes, 16-B aligned    */
  int64_t n;             /* elements per chain evaluated, 1 <= n <= 4*chain_groups   */
  uint64_t chain_groups;
  int32_t chains;        /* K >= 2                                                   */
  int32_t var_mode;      /* bdl_var_mode, as bdl_posterior_sample                    */
  float ratio, inv_ratio, var_floor;   /* as bdl_sample_args                         */
  float c1;              /* fl32((count-1)/count), count = samples per chain >= 2    */
  float thresholds[3];
  int32_t blocks_per_cu; /* workgroups per CU, 1-8 (0: default 2)                    */
} bdl_chain_diag_args;

/* Device scratch of one bdl_chain_diag call: the summary, then the
 * per-workgroup partials.  Independent of n today; pass n all the same. */
int64_t bdl_chain_diag_workspace_bytes(int64_t n);

/* Two launches on hip_stream (the sweep, the one-workgroup combine), no host
 * synchronisation, no allocation.  Only elements [0, n) of each output are
 * written, only bdl_chain_diag_workspace_bytes(n) bytes of the workspace, and
 * the padding tail of a chain's slot is never read.  Validation comes before
 * any HIP call: BDL_ERR_NULL (args, mom1, mom2, workspace), BDL_ERR_ALIGN (a
 * vector or the workspace not 16-B aligned), BDL_ERR_ARG (chains < 2, n < 1,
 * n > 4*chain_groups, unknown var_mode, var_floor < 0, blocks_per_cu outside
 * [0, 8], chains * chain_groups overflowing the element index, or a graph
 * redirect active on the thread). */
int bdl_chain_diag(const bdl_chain_diag_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_DIAG_H */
