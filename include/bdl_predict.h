/* bdl_predict.h — predictive uncertainty and calibration of an ensemble of
 * classifiers from its members' logits, in one fused sweep.
 *
 * The stacked samplers average the predictive over M members (chains x
 * collected components x posterior draws).  bdl_predict reads every member
 * logit once and gives, per example, the log mixture, its entropy, the
 * members' mean entropy, their difference (the mutual information between the
 * label and the member), the confidence, the vote and how many members are
 * off it; and, over any number of calls, running totals in DEVICE memory —
 * NLL, error, the entropies, the calibration bins of calibration.calc_bins —
 * that the host reads once.  Purely additive to the ABI of bdl_sgmcmc.h (same
 * status codes, bdl_last_error, stream convention, graph-redirect refusal).
 *
 * Input.  logits: fp32, contiguous [members, groups, batch, classes]; member
 * i of group g, example b starts at ((i*groups + g)*batch + b)*classes.
 * groups = 1 pools all members; groups = K over the samplers'
 * [components, K, B, C] order gives every chain its own mixture.  labels:
 * optional int64 [batch] in device memory, shared by the groups; a label
 * outside [0, classes) makes the example unlabelled: it counts in n and the
 * uncertainty sums, not in n_labelled, nll, error or the bins, and it is never
 * used as an index.
 *
 * Definitions, per group g and example b (natural log, 0 * log 0 = 0):
 *   p_i = softmax(logits[i,g,b,:])          pbar = mean_i p_i
 *   logp = log pbar (-inf where pbar = 0)   entropy = H[pbar]
 *   expected_entropy = mean_i H[p_i]        mutual_info = entropy - expected_entropy
 *   confidence = max_c pbar                 pred = argmax_c pbar (lowest index)
 *   disagree = #{i : argmax_c logits[i] (lowest index) != pred}
 *   nll = -logp[label]  (NaN for an unlabelled example)
 * mutual_info is not clamped.  A -inf logit is a masked class (p = 0).  An
 * example is NON-FINITE if any of its member rows holds a NaN, a +inf or no
 * finite entry: its float outputs and its logp row are NaN, pred and disagree
 * are -1, it is counted in n_nonfinite and left out of every other total (n
 * included) — the convention of bdl_diag.h / bdl_ess.h.
 *
 * Arithmetic contract (tests/predict_ref.py emulates it and derives the
 * bounds from it).  u = 2^-24.
 *   fp32, one rounding each:  m_i = max_c x (exact);  d = x - m_i;
 *     e = expf(d);  log Z_i = logf((float)Z_i);  pbar32 = (float)pbar;
 *     logp = logf(pbar32).  expf / logf are the HIP device library's
 *     (ocml exp_f32 / log_f32), documented maximum error 1 ulp each (HIP math
 *     API, single-precision table); -ffp-contract=off, nothing is fused.
 *   fp64:  Z_i = sum_c e and T_i = sum_c e*d (in-lane, cross-lane and
 *     cross-wave; e*d is exact in fp64);  H[p_i] = log Z_i - T_i * (1/Z_i);
 *     the mixture accumulator acc_c += e * (1/Z_i) over the members in member
 *     order;  pbar = acc_c / M;  entropy = -sum_c pbar32 * logp (the product
 *     exact in fp64);  expected_entropy = (sum_i H[p_i]) / M;
 *     mutual_info = entropy - expected_entropy.  The three are rounded to
 *     fp32 once, for the per-example outputs; the totals add the fp64 values
 *     (nll_sum adds the fp32 nll, bin_conf the fp32 pbar32).
 *   confidence, pred and the bins are decided on pbar32, the bins against the
 *     fp32 edges: bin = #{j : edges[j] <= pbar32}.
 *
 * Geometry.  Two launches.  (1) The sweep: every workgroup (256 threads)
 * walks the groups; of a group it takes examples grid-strided from a first
 * workgroup rotated by the group index, and writes one partial
 * bdl_predict_totals per (group, workgroup that has an example of it) to the
 * workspace.  classes <= BDL_PREDICT_WAVE_CLASSES: one WAVE per example (four
 * examples per workgroup, wave shuffles only); above: one WORKGROUP per
 * example, a thread owning the 16-B groups t, t + 256, ... of every member
 * row, the mixture accumulator (fp64) and the vote counts in its registers, a
 * member costing two workgroup reductions.  Rows are read in 16-B non-temporal
 * loads where classes % 4 == 0 (every row is then 16-B aligned), else element
 * by element.  (2) The combine: one workgroup per group adds the group's
 * partials in a fixed order (four contiguous quarters of the rotated
 * workgroup order, then the quarters in order) and adds the result to — with
 * BDL_PREDICT_RESET: writes it over — totals[g].
 *   - Every integer field, pred, disagree and bin membership is independent of
 *     grid_blocks; the fp64 sums differ between geometries only in the order
 *     of the sum.  For a fixed grid_blocks a call is bit-identical run to run.
 *   - No atomics, no host synchronisation, no allocation. */
#ifndef BDL_PREDICT_H
#define BDL_PREDICT_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_PREDICT_MAX_CLASSES 8192  /* classes <= this (a thread's registers)        */
#define BDL_PREDICT_WAVE_CLASSES 256  /* classes <= this: one wave per example         */
#define BDL_PREDICT_MAX_BINS 64       /* num_bins <= this (a lane owns a bin)          */
#define BDL_PREDICT_MAX_GROUPS 65535  /* groups <= this                                */
#define BDL_PREDICT_MAX_GRID 1024     /* grid_blocks <= this                           */

typedef enum bdl_predict_flag {
  BDL_PREDICT_RESET = 0x1  /* totals[g] is overwritten, not added to (no memset needed) */
} bdl_predict_flag;

typedef struct bdl_predict_totals {  /* per group; DEVICE memory, 8-B aligned */
  int64_t n;             /* examples evaluated (finite), labelled or not               */
  int64_t n_labelled;    /* ... of them with a label in [0, classes)                   */
  int64_t n_nonfinite;   /* examples left out (see above)                              */
  int64_t n_wrong;       /* labelled examples with pred != label                       */
  int64_t disagree_sum;  /* sum of disagree over the n examples                        */
  double nll_sum;        /* over the labelled examples                                 */
  double entropy_sum, expected_entropy_sum, mi_sum;  /* over the n examples            */
  double mi_sum_wrong;   /* mutual_info over the n_wrong examples                      */
  /* calibration bins: EVERY (example, class) probability pbar32[c] of a
   * labelled example, as calibration.calc_bins                                        */
  int64_t bin_count[BDL_PREDICT_MAX_BINS];
  int64_t bin_hits[BDL_PREDICT_MAX_BINS];   /* ... with c == label                     */
  double bin_conf[BDL_PREDICT_MAX_BINS];    /* sum of pbar32[c]                        */
} bdl_predict_totals;

typedef struct bdl_predict_args {
  const float* logits;    /* [members, groups, batch, classes], 16-B aligned           */
  const int64_t* labels;  /* DEVICE [batch] or null (every example unlabelled)         */
  /* per-call outputs, each nullable (a null output is not written) */
  float* logp;            /* [groups, batch, classes], 16-B aligned                    */
  float* entropy;         /* [groups, batch] each, 8-B aligned                         */
  float* expected_entropy;
  float* mutual_info;
  float* confidence;
  float* nll;
  int32_t* pred;
  int32_t* disagree;
  bdl_predict_totals* totals;  /* DEVICE [groups], 8-B aligned: added to               */
  void* workspace;        /* bdl_predict_workspace_bytes(groups, grid_blocks) bytes,
                             16-B aligned, device memory                               */
  int64_t batch;          /* B >= 1                                                    */
  int32_t members;        /* Mg >= 1, members per group                                */
  int32_t groups;         /* G, 1 .. BDL_PREDICT_MAX_GROUPS                            */
  int32_t classes;        /* C, 1 .. BDL_PREDICT_MAX_CLASSES                           */
  int32_t num_bins;       /* nb, 1 .. BDL_PREDICT_MAX_BINS                             */
  int32_t grid_blocks;    /* workgroups of the sweep, 1 .. BDL_PREDICT_MAX_GRID (0:
                             default, one per example of every group up to four per
                             CU, at most BDL_PREDICT_MAX_GRID)                         */
  int32_t flags;          /* bdl_predict_flag bits                                     */
  /* the nb - 1 interior right edges of the bins, strictly increasing in (0, 1):
   * fl32(np.linspace(0, 1 + 1e-8, nb + 1)[1:-1]) for calibration.calc_bins' bins      */
  float edges[BDL_PREDICT_MAX_BINS];
} bdl_predict_args;

/* Device scratch of one call: one partial per (group, workgroup).
 * grid_blocks = 0 sizes it for BDL_PREDICT_MAX_GRID workgroups (what the
 * default may use).  0 if an argument is out of range. */
int64_t bdl_predict_workspace_bytes(int32_t groups, int32_t grid_blocks);

/* Two launches on hip_stream (the sweep; the combine, one workgroup per
 * group), no host synchronisation, no allocation.  Only the non-null outputs,
 * totals[0, groups) and bdl_predict_workspace_bytes(groups, grid_blocks) bytes
 * of the workspace are written.
 *
 * Validation comes before any HIP call: BDL_ERR_NULL (args, logits, totals,
 * workspace), BDL_ERR_ALIGN (logits, logp or the workspace not 16-B aligned;
 * another output, labels or totals not 8-B aligned), BDL_ERR_ARG (members,
 * groups, batch, classes, num_bins or grid_blocks out of range; an unknown
 * flag; members*groups*batch*classes*4 not representable in int64; edges not
 * strictly increasing in (0, 1); an output, totals or the workspace overlapping
 * logits, labels or one another; a graph redirect active on the thread). */
int bdl_predict(const bdl_predict_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_PREDICT_H */
