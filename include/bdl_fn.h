/* bdl_fn.h — function-space convergence of stacked chains: the fold of the
 * chains' class probabilities on a fixed probe batch into batch-means
 * accumulators, in one fused sweep.
 *
 * R-hat and the effective sample size in parameter space (bdl_diag.h,
 * bdl_ess.h) are pessimistic for a neural network: chains that settle in
 * permutation- or sign-equivalent modes differ in every parameter for good and
 * agree on every prediction.  The same two numbers over the predictions
 * themselves need the sampled quantity softmax(f(x_b; theta_t))[c] on a fixed
 * probe batch, per (example, class).  bdl_fn_fold reads the K chains' probe
 * logits once, forms the probabilities and folds them into the four
 * accumulators of bdl_ess.h, with no probability tensor in between; the
 * reports are bdl_chain_diag (mom1 = smean, mom2 = sM2, Welford) and
 * bdl_chain_ess (sM2, bM2) on those accumulators.  Purely additive to the ABI
 * of bdl_sgmcmc.h (same status codes, bdl_last_error, stream convention,
 * graph-redirect refusal).
 *
 * Input.  logits: fp32, contiguous [chains, probe, classes]; chain k, example
 * b starts at (k*probe + b)*classes.
 *
 * Accumulators.  bsum, smean, sM2, bM2 exactly as bdl_ess.h stacks them: chain
 * k, element j at 4*chain_groups*k + j, here j = b*classes + c and
 * n = probe*classes <= 4*chain_groups.  Elements [n, 4*chain_groups) of a
 * chain slot are neither read nor written.  bsum is nullable at batch == 1
 * (never touched).  A vector a fold does not need is neither read nor written,
 * as in bdl_ess.h.
 *
 * Optional output.  probs: nullable, [chains, probe, classes] fp32, the
 * probabilities that were folded.
 *
 * Arithmetic contract (tests/fn_fold_ref.py derives its bound from it).
 * u = 2^-24.  Per row x = logits[k, b, :]:
 *   m = max_c x                       (exact)
 *   d = x - m                         one fp32 rounding
 *   e = expf(d)                       the HIP device library's (ocml exp_f32),
 *                                     documented maximum error 1 ulp
 *   Z = sum_c e                       in fp64, in an order fixed by the kernel
 *                                     and not by the launch geometry (below)
 *   p = (float)((double)e * (1.0 / Z))   fp64 reciprocal and product, one
 *                                     rounding to fp32
 * -ffp-contract=off, nothing is fused.  Then, per element, the fold of
 * bdl_ess.h line for line with x = p (the ONE device function
 * bdl_chain_ess_fold instantiates, bdl_chain_elem.hpp):
 *   FIRST_SAMPLE:   smean' = p;  sM2' = 0
 *   else:           d = p - smean;  q = d / fs;  smean' = smean + q
 *                   d2 = p - smean';  t = d * d2;  sM2' = sM2 + t
 *   FIRST_IN_BATCH: bs = p           else: bs = bsum + p
 *   not CLOSE:      bsum' = bs
 *   CLOSE:          y = bs / fb
 *     FIRST_BATCH:  bM2' = 0         else: e = y - smean';  t = e * e
 *                                          u = t * c;  bM2' = bM2 + u
 * A -inf logit is a masked class (p = 0).  A row holding a NaN, a +inf or no
 * finite entry gives NaN probabilities in every class of that row; they are
 * folded as computed, so the reports later count those elements in
 * n_nonfinite.  No other row is affected.
 *
 * Geometry.  One launch of 256-thread workgroups over the chains * probe rows,
 * grid-strided.  classes <= BDL_FN_WAVE_CLASSES: one WAVE per row (four rows
 * per workgroup trip; lane l owns the 16-B class group l; wave shuffles only;
 * lanes past the last group and waves past the last row idle).  Above: one
 * WORKGROUP per row, thread t owning the class groups t, t + 256, ...; e is
 * kept in LDS (a thread re-reads only what it wrote) between the row's two
 * workgroup reductions.  Rows and accumulators are accessed in 16-B
 * non-temporal loads / stores where classes % 4 == 0 (every row and every
 * accumulator row is then 16-B aligned), else element by element.  Z: a
 * thread adds its groups in ascending order, elements in ascending order; the
 * 64 lanes by a butterfly (offsets 32, 16, .., 1); the four waves in wave
 * order.  Each element is written by exactly one thread, so results are
 * bit-identical for every grid_blocks.  No atomics, no host synchronisation,
 * no allocation. */
#ifndef BDL_FN_H
#define BDL_FN_H

#include <stdint.h>

#include "bdl_ess.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_FN_MAX_CLASSES 8192  /* classes <= this (a row's e in LDS: 32 KiB)     */
#define BDL_FN_WAVE_CLASSES 256  /* classes <= this: one wave per row              */
#define BDL_FN_MAX_GRID 2048     /* grid_blocks <= this                            */

typedef struct bdl_fn_fold_args {
  const float* logits;   /* [chains, probe, classes], 16-B aligned                   */
  float* bsum;           /* stacked as bdl_ess.h; nullable when batch == 1           */
  float* smean;
  float* sM2;
  float* bM2;
  float* probs;          /* nullable; [chains, probe, classes], 16-B aligned         */
  int64_t probe;         /* P >= 1 examples; n = P * classes <= 4*chain_groups       */
  uint64_t chain_groups;
  int64_t sample;        /* s, 1 <= s < BDL_ESS_MAX_COUNT                            */
  int64_t batch;         /* b, 1 <= b < BDL_ESS_MAX_COUNT                            */
  int32_t chains;        /* K, 1 .. BDL_ESS_MAX_CHAINS                               */
  int32_t classes;       /* C, 1 .. BDL_FN_MAX_CLASSES                               */
  int32_t flags;         /* bdl_ess_flag bits; must be the ones (sample, batch) imply */
  float fs, fb;          /* fl32(s), fl32(b)                                         */
  float c;               /* fl32(i/(i-1)), i = s/b, on a CLOSE that is not the first
                            batch's; ignored otherwise                               */
  int32_t grid_blocks;   /* workgroups, 1 .. BDL_FN_MAX_GRID (0: default, one per
                            row trip up to four per CU)                              */
  int32_t pad0;
} bdl_fn_fold_args;

/* One launch on hip_stream; no host synchronisation, no allocation.
 * Validation comes before any HIP call: BDL_ERR_NULL (args, logits, smean,
 * sM2, bM2; bsum with batch > 1), BDL_ERR_ALIGN (a vector not 16-B aligned),
 * BDL_ERR_ARG (chains, probe, classes, chain_groups, sample, batch or
 * grid_blocks out of range; chains * probe * classes or chains * chain_groups
 * overflowing the element index; probe * classes exceeding the chain slot;
 * flags, fs, fb or c that are not what (sample, batch) imply; two vectors
 * overlapping; or a graph redirect active on the thread). */
int bdl_fn_fold(const bdl_fn_fold_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_FN_H */
