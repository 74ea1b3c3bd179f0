/* bdl_temper.h — temperature scaling of an ensemble's predictive on the device:
 * a scalar temperature per group fitted on a validation split by a safeguarded
 * Newton iteration, and the calibration report at a temperature.
 *
 * What is scaled is the SAMPLE-AVERAGED log-probability z[b, c] of an example
 * (what bdl_predict writes as logp[g, b, c]), not the member logits:
 *   q = softmax(z / T),   T = argmin mean_b ( lse(z_b / T) - z_b[y_b] / T ).
 * In beta = 1 / T the per-example loss f(beta) = lse(beta z) - beta z[y] is
 * convex, f' = E_q[z] - z[y], f'' = Var_q[z] >= 0: Newton from beta = 1 with a
 * clamped step has one optimum to find and needs no line search.  Purely
 * additive to the ABI of bdl_sgmcmc.h (same status codes, bdl_last_error,
 * stream convention, graph-redirect refusal).
 *
 * Input.  logp: fp32, contiguous [groups, batch, classes]; any finite values
 * (log-probabilities or logits).  labels: optional int64 [batch] in device
 * memory, shared by the groups; a label outside [0, classes) (or null labels)
 * makes the example unlabelled and it is never used as an index.  state: one
 * bdl_temper_state per group in device memory; its beta is an fp32 VALUE (the
 * update rounds every new beta to fp32 once, so the sweeps, the report and the
 * host see the same number).
 *
 * Special values, at the group's current beta:
 *   - A -inf entry is a class of probability zero: it contributes 0 to every
 *     sum over classes and never 0 * inf.
 *   - An example is NON-FINITE if its row holds a NaN or a +inf, has no finite
 *     entry, or fl32(beta * max_c z) is not finite: it is counted in
 *     n_nonfinite (labelled or not) and left out of everything else.
 *   - The fit uses the labelled, finite examples.  One whose own
 *     fl32(beta * z[y]) is -inf (f = +inf) is counted in n_inf_label and left
 *     out of the fit.  The report adds its +inf to nll_sum, as bdl_predict does.
 *
 * Arithmetic contract (tests/temper_ref.py emulates it and derives the bounds
 * from it).  u = 2^-24.
 *   fp32, one rounding each:  t = beta * z;  m = beta * max_c z (= max_c t,
 *     rounding is monotone);  d = t - m;  e = expf(d) (the HIP device library's
 *     ocml exp_f32, documented maximum error 1 ulp); -ffp-contract=off, nothing
 *     is fused.  The report's q32 = (float)((double)e * (1.0 / S0)).
 *   fp64:  every sum over classes, in-lane, cross-lane and cross-wave —
 *     S0 = sum e, S1 = sum e z, S2 = sum e z^2 (the fit; e z is exact),
 *     T1 = sum e d (the report); lse = m + log(S0);  E = S1 / S0;
 *     Var = S2 / S0 - E^2, clamped at 0;  f = lse - t[y];  f' = E - z[y];
 *     f'' = Var;  the report's nll = lse - t[y], entropy = log(S0) - T1 / S0;
 *     every sum over examples.
 *   The report's argmax is the lowest index of max_c z (it does not depend on
 *     T); its confidence is q32 there; the bins are decided on q32 against the
 *     fp32 edges: bin = #{j : edges[j] <= q32}.
 *
 * Geometry (bdl_predict's).  Every entry point is two launches or one, with no
 * atomics, no host synchronisation and no allocation.  A sweep (the fit's, the
 * report's): every workgroup (256 threads) walks the groups; of a group it
 * takes examples grid-strided from a first workgroup rotated by the group
 * index, and writes one partial per (group, workgroup that has an example of
 * it) to the workspace.  classes <= BDL_TEMPER_WAVE_CLASSES: one WAVE per
 * example (four per workgroup, wave shuffles only); above: one WORKGROUP per
 * example, a thread owning the 16-B class groups t, t + 256, ...  Rows are read
 * in 16-B non-temporal loads where classes % 4 == 0, else element by element;
 * the next example's row is loaded before the current one is reduced.  The
 * second launch (bdl_temper_fit_update; the report's combine) is one workgroup
 * per group and adds the group's partials in a fixed order.
 *   - Every integer field and bin membership is independent of grid_blocks; the
 *     fp64 sums differ between geometries only in the order of the sum.  For a
 *     fixed grid_blocks a call is bit-identical run to run. */
#ifndef BDL_TEMPER_H
#define BDL_TEMPER_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_TEMPER_MAX_CLASSES 8192  /* classes <= this (a thread's registers)         */
#define BDL_TEMPER_WAVE_CLASSES 256  /* classes <= this: one wave per example          */
#define BDL_TEMPER_MAX_BINS 64       /* num_bins <= this (a lane owns a bin)           */
#define BDL_TEMPER_MAX_GROUPS 65535  /* groups <= this                                 */
#define BDL_TEMPER_MAX_GRID 1024     /* grid_blocks <= this                            */
#define BDL_TEMPER_MAX_ITER 1024     /* max_iter <= this                               */
#define BDL_TEMPER_MAX_T 100.0f      /* beta >= fl32(1 / 100)                          */
#define BDL_TEMPER_MIN_T 0.01f       /* beta <= 100                                    */

typedef enum bdl_temper_flag {
  BDL_TEMPER_RESET = 0x1  /* totals[g] is overwritten, not added to (as BDL_PREDICT_RESET) */
} bdl_temper_flag;

typedef struct bdl_temper_state {  /* per group; DEVICE memory, 8-B aligned */
  double nll;           /* sum f / n at the beta of the group's last sweep             */
  double nll_first;     /* ... of its first sweep (at the beta the state started with) */
  double d1, d2;        /* sum f' / n, sum f'' / n of the last sweep                   */
  int64_t n;            /* examples the last sweep used (labelled, finite, f finite)   */
  int64_t n_nonfinite;  /* non-finite examples of the last sweep                       */
  int64_t n_inf_label;  /* labelled finite examples with f = +inf, left out            */
  float beta;           /* 1 / T, in [fl32(1 / MAX_T), 1 / MIN_T]                      */
  int32_t iterations;   /* updates that moved beta                                     */
  int32_t sweeps;       /* updates that evaluated the group                            */
  int32_t converged;    /* the last Newton step was within rtol * beta: beta is final  */
  int32_t at_bound;     /* the last step landed on a limit of beta                     */
  int32_t degenerate;   /* n == 0, or f'' <= 0 or a derivative not finite: no step     */
  int32_t done;         /* beta is final: converged, or the step landed on the limit
                           beta already sits on; the sweeps and updates skip the group */
  int32_t pad0;
} bdl_temper_state;

typedef struct bdl_temper_fit_args {
  const float* logp;        /* [groups, batch, classes], 16-B aligned                  */
  const int64_t* labels;    /* DEVICE [batch] or null (every example unlabelled)       */
  bdl_temper_state* state;  /* DEVICE [groups], 8-B aligned                            */
  void* workspace;          /* bdl_temper_workspace_bytes(groups, grid_blocks) bytes,
                               16-B aligned, device memory                             */
  int64_t batch;            /* N >= 1                                                  */
  double rtol;              /* 0 <= rtol < 1: |beta' - beta| <= rtol * beta converges  */
  int32_t groups;           /* G, 1 .. BDL_TEMPER_MAX_GROUPS                           */
  int32_t classes;          /* C, 1 .. BDL_TEMPER_MAX_CLASSES                          */
  int32_t grid_blocks;      /* workgroups of the sweep, 1 .. BDL_TEMPER_MAX_GRID (0:
                               bdl_predict's default)                                  */
  int32_t max_iter;         /* 1 .. BDL_TEMPER_MAX_ITER: beta moves at most this often */
} bdl_temper_fit_args;

typedef struct bdl_temper_totals {  /* per group; DEVICE memory, 8-B aligned */
  int64_t n;               /* examples evaluated (finite), labelled or not             */
  int64_t n_labelled;      /* ... of them with a label in [0, classes)                 */
  int64_t n_nonfinite;     /* examples left out                                        */
  int64_t n_wrong;         /* labelled examples with argmax_c z != label               */
  double nll_sum;          /* -log q[label] over the labelled examples                 */
  double entropy_sum;      /* H[q] over the n examples                                 */
  double confidence_sum;   /* max_c q32 over the n examples                            */
  /* calibration bins: EVERY (example, class) probability q32[c] of a labelled
   * example, as calibration.calc_bins                                                 */
  int64_t bin_count[BDL_TEMPER_MAX_BINS];
  int64_t bin_hits[BDL_TEMPER_MAX_BINS];   /* ... with c == label                      */
  double bin_conf[BDL_TEMPER_MAX_BINS];    /* sum of q32[c]                            */
} bdl_temper_totals;

typedef struct bdl_temper_report_args {
  const float* logp;              /* [groups, batch, classes], 16-B aligned            */
  const int64_t* labels;          /* DEVICE [batch] or null                            */
  const bdl_temper_state* state;  /* DEVICE [groups], 8-B aligned: only beta is read   */
  bdl_temper_totals* totals;      /* DEVICE [groups], 8-B aligned: added to            */
  void* workspace;                /* as bdl_temper_fit_args                            */
  int64_t batch;
  int32_t groups, classes;
  int32_t num_bins;               /* nb, 1 .. BDL_TEMPER_MAX_BINS                      */
  int32_t grid_blocks;
  int32_t flags;                  /* bdl_temper_flag bits                              */
  int32_t pad0;
  /* the nb - 1 interior right edges of the bins, strictly increasing in (0, 1),
   * as bdl_predict_args.edges                                                         */
  float edges[BDL_TEMPER_MAX_BINS];
} bdl_temper_report_args;

/* Device scratch of one call of any of the three entry points: one partial per
 * (group, workgroup).  grid_blocks = 0 sizes it for BDL_TEMPER_MAX_GRID
 * workgroups.  0 if an argument is out of range. */
int64_t bdl_temper_workspace_bytes(int32_t groups, int32_t grid_blocks);

/* One launch: per group that is not done, the partial sums of f, f', f'' and
 * the three counts at state[g].beta into the workspace.  A done group is
 * skipped (nothing of it is read or written).  The state is only read. */
int bdl_temper_fit_sweep(const bdl_temper_fit_args* args, void* hip_stream);

/* One launch, one workgroup per group, after a bdl_temper_fit_sweep with the
 * SAME args on the same stream.  A done group is left as it is.  Else:
 *   1. the group's partials are summed in a fixed order;
 *   2. n, n_nonfinite, n_inf_label, nll = sum f / n, d1, d2 are stored (NaN,
 *      0, 0 at n == 0), nll_first too at the group's first update; sweeps += 1;
 *   3. degenerate = (n == 0 or not d2 > 0 or d1 not finite); then, and once
 *      iterations == max_iter, beta stays;
 *   4. else b = beta - d1 / d2, clamped to [beta / 4, 4 beta], then to
 *      [fl32(1 / BDL_TEMPER_MAX_T), 1 / BDL_TEMPER_MIN_T] — landing on either
 *      limit sets at_bound, anything else clears it — and rounded to fp32;
 *   5. not at_bound and |b - beta| <= rtol * beta: converged = done = 1, beta
 *      stays (nll, d1, d2 ARE those of the final beta); at_bound and
 *      b == beta (the group sits on the limit and the step points beyond it):
 *      done = 1, NOT converged; else if b != beta: beta = b, iterations += 1.
 * A fit is `max_iter` (sweep, update) pairs enqueued back to back and one host
 * read of the state: iterations + 1 sweeps do work, the rest skip.  A group
 * that is neither converged nor degenerate then did not converge, and says so
 * (at_bound: its optimum is at or beyond a limit of beta). */
int bdl_temper_fit_update(const bdl_temper_fit_args* args, void* hip_stream);

/* Two launches (the sweep; the combine): the totals of q = softmax(beta z) at
 * state[g].beta added to — with BDL_TEMPER_RESET: written over — totals[g].
 *
 * Validation of all three comes before any HIP call: BDL_ERR_NULL (args, logp,
 * state, totals, workspace), BDL_ERR_ALIGN (logp or the workspace not 16-B
 * aligned; labels, state or totals not 8-B aligned), BDL_ERR_ARG (groups,
 * batch, classes, num_bins, grid_blocks, max_iter or rtol out of range; an
 * unknown flag; groups*batch*classes*4 not representable in int64; edges not
 * strictly increasing in (0, 1); a written span — state, totals, the workspace
 * — overlapping an input or another one; a graph redirect active on the
 * thread). */
int bdl_temper_report(const bdl_temper_report_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_TEMPER_H */
