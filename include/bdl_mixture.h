/* bdl_mixture.h — the likelihood-weighted cycle mixture of stacked cyclical
 * chains: the cycle-end likelihood pass (bdl_member_score) and the weighted
 * predictive (bdl_mixture), each one fused sweep over member logits.
 *
 * A cyclical sampler scores max(1, nst) posterior draws of a finished cycle on
 * the training set, weighs cycle c by w_c = 1 / mean_j(1 / lik_j) and predicts
 * with that mixture of its cycles.  bdl_member_score keeps the loss sums of
 * every (draw, chain) pair in DEVICE memory over any number of batches, so the
 * pass ends in one host read; bdl_mixture reads every member logit once and
 * gives the weighted log mixture and the weighted expected entropy.  Purely
 * additive to the ABI of bdl_sgmcmc.h (same status codes, bdl_last_error,
 * stream convention, graph-redirect refusal).
 *
 * Input of both.  logits: fp32, contiguous [members, groups, batch, classes],
 * bdl_predict's layout: member i of group g, example b starts at
 * ((i*groups + g)*batch + b)*classes.  labels: int64 [batch] in device memory,
 * shared by the groups.  A -inf logit is a masked class (p = 0).  A row is
 * NON-FINITE if it holds a NaN, a +inf or no finite entry.  u = 2^-24; expf /
 * logf are the HIP device library's (documented maximum error 1 ulp each);
 * -ffp-contract=off, nothing is fused.
 *
 * ---------------------------------------------------------------- bdl_member_score
 * Adds to scores[i*groups + g], per row (i, g, b):
 *   - a label outside [0, classes) skips the row entirely (no field counts it,
 *     the label is never used as an index);
 *   - a non-finite row counts in n_nonfinite only;
 *   - else n += 1, n_wrong += (lowest-index argmax != label), nll_sum += nll.
 * Arithmetic contract:  m = max_c x (exact);  d = x - m and e = expf(d), fp32,
 * one rounding each;  Z = sum_c e in fp64;  lse = m + logf((float)Z) and
 * nll = lse - x[label], fp32, one rounding each (a masked class at the label:
 * nll = +inf);  nll_sum adds the fp32 nll in fp64.
 *
 * --------------------------------------------------------------------- bdl_mixture
 * Member i = c*draws + s is draw s of component c (members = components *
 * draws).  weights: fp64 [components, groups] in device memory, taken as given
 * (the caller normalises them).  Per group g and example b:
 *   - a component with w_c < BDL_MIXTURE_MIN_WEIGHT (1e-10) is SKIPPED: its
 *     rows are not read for any purpose, a NaN there does not make the example
 *     non-finite;
 *   - otherwise p_i = softmax(row_i) under bdl_predict's per-member contract:
 *     fp32 d and e, fp64 Z_i = sum_c e and T_i = sum_c e*d,
 *     H_i = logf((float)Z_i) - T_i * (1/Z_i);
 *   - pbar_c = (sum_s e * (1/Z_i)) / draws, fp64, in draw order;
 *   - expected_entropy = sum_c w_c * ((sum_s H_i) / draws), fp64, in component
 *     order, rounded to fp32 once for the per-example output; the totals add
 *     the fp64 value.
 *   BDL_MIX_ARITHMETIC:  mix = sum_c w_c * pbar_c (fp64, component order);
 *     pbar32 = (float)mix;  logp = logf(pbar32).
 *   BDL_MIX_REFERENCE (a cyclical Runner's rule: the weighted sum of the
 *     components' log-probabilities, renormalised as its cross-entropy does):
 *     l_c = logf((float)pbar_c);  t = sum_c w_c * (double)l_c;
 *     logp = (float)(t - logsumexp(t)), the logsumexp over the classes in fp64
 *     (max, exp, sum, log); a row of t without a finite entry gives -inf.
 *   An example is non-finite if a row of a component that is NOT skipped is:
 *   its logp row and expected_entropy are NaN, it counts in n_nonfinite and
 *   stays out of n and expected_entropy_sum (bdl_predict's convention).  With
 *   every component skipped the sums are empty (arithmetic: logp = -inf).
 *   labels is accepted for symmetry with bdl_predict and validated, not read:
 *   NLL, error and calibration come from bdl_temper_report on logp.
 *   With all weight on one component (w = 1) the arithmetic mode is
 *   bdl_predict on that component's members, bit for bit (same thread layout,
 *   same reduction order).
 *
 * Geometry of both.  Two launches.  (1) The sweep on a (grid_blocks, pairs)
 * grid of 256 threads — pairs = members*groups (score) or groups (mixture) —
 * so a workgroup's partial belongs to exactly one pair; its rows / examples
 * are grid-strided over grid_blocks.  classes <= BDL_MIXTURE_WAVE_CLASSES: one
 * WAVE per row (four per workgroup, wave shuffles only); above: one WORKGROUP
 * per row, thread t owning the 16-B class groups t, t + 256, ... of every
 * member row, so the mixture's two fp64 accumulators per class stay in its
 * registers (that bounds classes by BDL_MIXTURE_MAX_CLASSES, for both entry
 * points).  16-B non-temporal loads where classes % 4 == 0, element loads
 * otherwise; the next row is loaded before the current one is reduced.  One
 * partial per (pair, workgroup) goes to the workspace.  (2) The combine: one
 * workgroup per pair adds its partials in a fixed order (thread t takes t,
 * t + 256, ...; the wave butterfly; the waves in order) and adds the result to
 * — with BDL_MIXTURE_RESET: writes it over — the pair's struct.
 *   - Every integer field is independent of grid_blocks; the fp64 sums differ
 *     between grids only in the order of the sum.  For a fixed grid_blocks a
 *     call is bit-identical run to run.
 *   - No atomics, no host synchronisation, no allocation, no scratch. */
#ifndef BDL_MIXTURE_H
#define BDL_MIXTURE_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_MIXTURE_MAX_CLASSES 4096  /* classes <= this (a thread's registers)         */
#define BDL_MIXTURE_WAVE_CLASSES 256  /* classes <= this: one wave per row              */
#define BDL_MIXTURE_MAX_PAIRS 65535   /* members*groups (score), groups (mixture) <=    */
#define BDL_MIXTURE_MAX_GRID 1024     /* grid_blocks (workgroups per pair) <= this      */
#define BDL_MIXTURE_MIN_WEIGHT 1e-10  /* a component below it is skipped                */

typedef enum bdl_mixture_flag {
  BDL_MIXTURE_RESET = 0x1  /* the structs are overwritten, not added to (no memset needed) */
} bdl_mixture_flag;

typedef enum bdl_mix_combine {
  BDL_MIX_ARITHMETIC = 0,  /* log of the weighted mean of the components' probabilities  */
  BDL_MIX_REFERENCE = 1    /* renormalised weighted sum of their log-probabilities       */
} bdl_mix_combine;

typedef struct bdl_member_score_t {  /* per (member, group); DEVICE memory, 8-B aligned */
  int64_t n;            /* rows scored (label in range, finite)                          */
  int64_t n_nonfinite;  /* rows with a label in range that are non-finite                */
  int64_t n_wrong;      /* scored rows whose lowest-index argmax differs from the label  */
  double nll_sum;       /* over the n rows                                               */
} bdl_member_score_t;

typedef struct bdl_member_score_args {
  const float* logits;    /* [members, groups, batch, classes], 16-B aligned            */
  const int64_t* labels;  /* DEVICE [batch], 8-B aligned                                */
  bdl_member_score_t* scores;  /* DEVICE [members*groups], 8-B aligned: added to        */
  void* workspace;        /* bdl_member_score_workspace_bytes(...) bytes, 16-B aligned  */
  int64_t batch;          /* B >= 1                                                     */
  int32_t members;        /* >= 1                                                       */
  int32_t groups;         /* >= 1; members*groups <= BDL_MIXTURE_MAX_PAIRS              */
  int32_t classes;        /* C, 1 .. BDL_MIXTURE_MAX_CLASSES                            */
  int32_t grid_blocks;    /* workgroups per pair, 1 .. BDL_MIXTURE_MAX_GRID (0: default,
                             one per row slot up to four per CU over all pairs)         */
  int32_t flags;          /* bdl_mixture_flag bits                                      */
  int32_t pad0;
} bdl_member_score_args;

typedef struct bdl_mixture_totals {  /* per group; DEVICE memory, 8-B aligned */
  int64_t n;            /* examples evaluated (finite)                                   */
  int64_t n_nonfinite;  /* examples left out                                             */
  double expected_entropy_sum;  /* over the n examples                                   */
} bdl_mixture_totals;

typedef struct bdl_mixture_args {
  const float* logits;    /* [components*draws, groups, batch, classes], 16-B aligned   */
  const double* weights;  /* DEVICE [components, groups], 8-B aligned                   */
  const int64_t* labels;  /* DEVICE [batch] or null; 8-B aligned; not read              */
  /* per-call outputs, each nullable (a null output is not written) */
  float* logp;            /* [groups, batch, classes], 16-B aligned                     */
  float* expected_entropy;  /* [groups, batch], 8-B aligned                             */
  bdl_mixture_totals* totals;  /* DEVICE [groups], 8-B aligned: added to                */
  void* workspace;        /* bdl_mixture_workspace_bytes(...) bytes, 16-B aligned       */
  int64_t batch;          /* B >= 1                                                     */
  int32_t components;     /* >= 1                                                       */
  int32_t draws;          /* >= 1, members per component                                */
  int32_t groups;         /* G, 1 .. BDL_MIXTURE_MAX_PAIRS                              */
  int32_t classes;        /* C, 1 .. BDL_MIXTURE_MAX_CLASSES                            */
  int32_t combine;        /* bdl_mix_combine                                            */
  int32_t grid_blocks;    /* workgroups per group, as above                             */
  int32_t flags;          /* bdl_mixture_flag bits                                      */
  int32_t pad0;
} bdl_mixture_args;

/* Device scratch of one call: one 32-B partial per (pair, workgroup).
 * grid_blocks = 0 sizes it for BDL_MIXTURE_MAX_GRID workgroups per pair (what
 * the default may use).  0 if an argument is out of range. */
int64_t bdl_member_score_workspace_bytes(int32_t members, int32_t groups, int32_t grid_blocks);
int64_t bdl_mixture_workspace_bytes(int32_t groups, int32_t grid_blocks);

/* Two launches each on hip_stream (the sweep; the combine, one workgroup per
 * pair), no host synchronisation, no allocation.  Only the non-null outputs,
 * the structs and the workspace's stated bytes are written.
 *
 * Validation comes before any HIP call: BDL_ERR_NULL (args, logits, labels of
 * the score, weights, scores / totals, workspace), BDL_ERR_ALIGN (logits, logp
 * or the workspace not 16-B aligned; weights, labels, expected_entropy, scores
 * or totals not 8-B aligned), BDL_ERR_ARG (members / components, draws, groups,
 * batch, classes or grid_blocks out of range; an unknown flag or combine;
 * members*groups*batch*classes*4 not representable in int64; an output, the
 * structs or the workspace overlapping an input or one another; a graph
 * redirect active on the thread). */
int bdl_member_score(const bdl_member_score_args* args, void* hip_stream);
int bdl_mixture(const bdl_mixture_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_MIXTURE_H */
