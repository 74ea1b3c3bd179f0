/* bdl_stacking.h — Bayesian stacking of predictive distributions (Yao,
 * Vehtari, Simpson, Gelman 2018) for an ensemble's voters, on the device: the
 * weights w on the simplex that maximise the held-out log score of the mixture,
 *   f(w) = (1/n) sum_i log sum_k w_k p_k(y_i | x_i).
 *
 * Two entry points.  bdl_stack_gather turns one batch of the voters' log-
 * probabilities [P, B, C] into columns of the resident score matrix
 * ell [P, cap] (ell[k, i] = log p_k(y_i | x_i)), so that no [P, N, C] tensor
 * stays resident.  bdl_stack_fit runs the EM / multiplicative iteration on that
 * matrix.  Purely additive to the ABI of bdl_sgmcmc.h (same status codes,
 * bdl_last_error, stream convention, graph-redirect refusal).  No atomics, no
 * allocation, no host synchronisation inside an entry point; -ffp-contract=off.
 *
 * ------------------------------------------------------------------ bdl_stack_gather
 * logp: fp32, contiguous [voters, batch, classes] (bdl_predict's logp with
 * groups = voters).  labels: int64 [batch].  For b < batch and column
 * i = off + b:  ell[k*cap + i] = logp[k, b, label_b] and valid[i] = 1, unless the
 * example is EXCLUDED: valid[i] = 0 and its ell column is written as 0.  The
 * causes, tested in this order (an example counts in exactly one):
 *   n_label       the label is outside [0, classes); it is never used as an index;
 *   n_nonfinite   some voter's value is a NaN or +inf;
 *   n_impossible  every voter's value is -inf: no weight gives the example mass.
 * A -inf from some, not all, voters is legal (p = 0).  The three counts are
 * ADDED to counters (int64[3] in that order, device memory; BDL_STACK_RESET:
 * written over).  Two launches: the sweep (an example per thread, grid-strided;
 * a workgroup writes its three counts to the workspace) and the combine (one
 * thread per counter adds the workgroups' in workgroup order).  Everything is
 * an integer or a copy: the result is exact and independent of the grid.
 *
 * --------------------------------------------------------------------- bdl_stack_fit
 * The iteration, over the valid columns i < n_cols (n of them), from the
 * interior start w = 1/P:
 *   s_i = sum_k w_k p_ik      g_k = (1/n) sum_i p_ik / s_i      (g = grad f)
 *   w_k <- w_k g_k, renormalised.
 * f is concave and sum_k w_k g_k = 1 for every w, so for the maximiser w* and
 * any w:  f(w*) - f(w) <= grad f(w) . (w* - w) = sum_k w*_k g_k - 1
 * <= max_k g_k - 1 =: gap.  gap is therefore a CERTIFICATE: a fit that reports
 * gap <= tol is within tol of the optimal log score, whatever path led there.
 * The iteration is EM for the mixture weights: f never decreases.
 *
 * Arithmetic contract (tests/stacking_ref.py restates it literally).  Per
 * valid example, u = 2^-24:
 *   m = max_k ell_k over all P voters (exact; finite, as the column is valid);
 *   d_k = ell_k - m and e_k = expf(d_k) in fp32, one rounding each, -inf giving
 *     0 (expf is the HIP device library's, documented maximum error 1 ulp);
 *   s = sum_k w_k * (double)e_k, fp64, k ascending from 0.0 (the product is
 *     rounded, then the sum: nothing is fused);
 *   r_k = (double)e_k * (1/s), fp64, the reciprocal rounded once;
 *   the example adds r_k to R_k and log(s) + (double)m (fp64 log) to F.
 * s > 0 always: the voter that attains m has e = 1, so s >= w_kmax, and no
 * weight that matters reaches 0 from the interior start — f never decreases
 * and log s_i <= 0, so log s_i >= n f(w) >= n f(1/P) >= -n log P; and a voter
 * that ALONE covers an example (every other e is 0) has r_k = 1/w_k there, so
 * g_k >= 1/(n w_k) and its next weight is >= 1/n.  Should s underflow all the
 * same (n log P beyond the fp64 range), the example is counted and the fit ends
 * with degenerate = 1.
 *
 * Geometry.  Every iteration is two launches.
 * (1) The sweep.  The n_cols columns are cut into fixed TILES of
 * BDL_STACK_TILE = 1024 examples; tile t produces partial t whatever the grid
 * is.  Workgroups of 256 threads take tiles grid-strided over grid_blocks.
 * Thread t of a tile owns its columns t, t + 256, t + 512, t + 768; lanes run
 * over examples, so every voter row is read coalesced, with ordinary cached
 * loads (the matrix is re-read every iteration and lives in L2 / the infinity
 * cache).  Order of every sum of a tile: the thread's (up to) four examples in
 * ascending column order from 0.0; then the wave butterfly (xor 32, 16, .., 1);
 * then the four waves in wave order from wave 0's value.  A partial is
 * P + 3 8-B words: R[P], F, the valid count, the count of examples with s <= 0.
 * (2) The update.  One workgroup: thread k adds word k of the partials in
 * ascending tile order from 0; then one thread:
 *   n == 0 or an s <= 0: degenerate = 1, nothing else changes;
 *   g_k = R_k / n, objective = F / n, gap = max_k g_k - 1 (objective_uniform =
 *     objective in the first pass);
 *   gap <= tol: converged = 1, w stays;
 *   else, unless the pass is evaluation-only: w_k <- w_k * g_k, then
 *     w_k <- w_k / (sum_k w_k, k ascending from 0.0), iterations += 1.
 * Every launch reads the state's converged and degenerate flags first and
 * exits at once when one is set, so launches enqueued past convergence leave
 * the state untouched.  The reported objective and gap are those of the
 * reported w: converged leaves w alone, and BDL_STACK_FINAL appends one
 * evaluation-only pass after the last update.  With P = 1 the first pass has
 * g = 1 exactly: w = [1], converged, 0 iterations.
 *   - The tile partition, every integer field and the order of every sum are
 *     independent of grid_blocks: the whole state is bit-identical for every
 *     grid_blocks and from run to run.
 *
 * Error against the literal reference (correctly rounded exp in place of expf)
 * after T updates, derived in tests/stacking_ref.py from the contract: the two
 * e_k differ by at most 1.5 ulp = 3u relatively, so each r_k, hence each g_k,
 * by 6u; the fp64 sums add (n + P) 2^-52.  The update's Jacobian in log w is
 * I - A with A = D^-1 S, S = (1/n) sum_i q_i q_i^T the second moment of the
 * responsibilities and D = diag(mean_i q_ik): A is row-stochastic and similar to
 * a symmetric positive semi-definite matrix, so the eigenvalues of I - A lie in
 * [0, 1] and a perturbation is not amplified to first order; the T + 1 passes'
 * errors add:
 *   |w_k - w_k^ref| <= (T + 1) (6u + (n + P) 2^-52)                  =: bw
 *   |objective - objective^ref| <= 3u + bw + (n + P) 2^-52 max(1, |objective|)
 *     (sum_k w_k g_k = 1 turns the weights' relative error into the objective's)
 *   |gap - gap^ref| <= (1 + gap) (6u + (n + P) 2^-52 + bw)           =: bg
 *     (d log g = -A d log w, A row-stochastic)
 * and `iterations` lies between the reference's counts at tol + bg and at
 * tol - bg.
 *
 * Limits: P <= BDL_STACK_MAX_VOTERS, classes <= BDL_STACK_MAX_CLASSES,
 * cap <= BDL_STACK_MAX_COLS. */
#ifndef BDL_STACKING_H
#define BDL_STACKING_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_STACK_MAX_VOTERS 64       /* 1 <= voters <= this (as bdl_diversity)      */
#define BDL_STACK_MAX_CLASSES 8192    /* classes <= this                             */
#define BDL_STACK_MAX_COLS (1 << 24)  /* cap <= this                                 */
#define BDL_STACK_TILE 1024           /* examples per tile of the fit's sweep        */
#define BDL_STACK_MAX_GRID 1024       /* grid_blocks <= this                         */
#define BDL_STACK_MAX_CHUNK 65536     /* iterations of one bdl_stack_fit call <= this */

typedef enum bdl_stack_flag {
  BDL_STACK_RESET = 0x1, /* gather: the counters are overwritten, not added to        */
  BDL_STACK_FIRST = 0x2, /* fit: the call starts a fit (w = 1/P; the state need not be
                            initialised, every field is written by the first pass)    */
  BDL_STACK_FINAL = 0x4  /* fit: one evaluation-only pass follows the call's iterations */
} bdl_stack_flag;

/* The state of one fit: DEVICE memory, 8-B aligned. */
typedef struct bdl_stack_state {
  double w[BDL_STACK_MAX_VOTERS]; /* the weights; entries >= voters are 0            */
  double objective;          /* f(w): the mean log score of the mixture              */
  double gap;                /* max_k g_k - 1 at w: f* - f(w) <= gap                 */
  double objective_uniform;  /* f(1/P), from the first pass                          */
  int64_t n;                 /* valid examples                                       */
  int32_t iterations;        /* updates of w                                         */
  int32_t converged;         /* gap <= tol was seen (at the reported w)              */
  int32_t degenerate;        /* n == 0, or an s underflowed: nothing is fitted       */
  int32_t pad;
} bdl_stack_state;

typedef struct bdl_stack_gather_args {
  const float* logp;      /* [voters, batch, classes]                                  */
  const int64_t* labels;  /* DEVICE [batch]                                            */
  float* ell;             /* [voters, cap]: columns off .. off + batch - 1 are written */
  int32_t* valid;         /* [cap]: likewise                                           */
  int64_t* counters;      /* DEVICE int64[3]: n_label, n_nonfinite, n_impossible       */
  void* workspace;        /* bdl_stack_workspace_bytes(voters, cap) bytes, 8-B aligned */
  int64_t batch;          /* B >= 1                                                    */
  int64_t off;            /* first column, 0 <= off, off + batch <= cap                */
  int64_t cap;            /* columns of ell, 1 .. BDL_STACK_MAX_COLS                   */
  int32_t voters;         /* P, 1 .. BDL_STACK_MAX_VOTERS                              */
  int32_t classes;        /* C, 1 .. BDL_STACK_MAX_CLASSES                             */
  int32_t grid_blocks;    /* workgroups of the sweep, 1 .. BDL_STACK_MAX_GRID (0: one
                             per 256 examples up to the maximum)                       */
  int32_t flags;          /* BDL_STACK_RESET or 0                                      */
} bdl_stack_gather_args;

typedef struct bdl_stack_fit_args {
  const float* ell;       /* [voters, cap]                                             */
  const int32_t* valid;   /* [cap]                                                     */
  bdl_stack_state* state; /* DEVICE, 8-B aligned                                       */
  void* workspace;        /* bdl_stack_workspace_bytes(voters, n_cols) bytes, 8-B
                             aligned, device memory                                    */
  int64_t n_cols;         /* N: the columns in use, 1 .. cap                           */
  int64_t cap;            /* columns of ell, 1 .. BDL_STACK_MAX_COLS                   */
  double tol;             /* >= 0 (a NaN is refused)                                   */
  int32_t voters;         /* P, 1 .. BDL_STACK_MAX_VOTERS                              */
  int32_t iterations;     /* (sweep, update) pairs this call enqueues, 0 ..
                             BDL_STACK_MAX_CHUNK; 0 only with BDL_STACK_FINAL          */
  int32_t grid_blocks;    /* workgroups of the sweep, 1 .. BDL_STACK_MAX_GRID (0: one
                             per tile up to two per CU)                                */
  int32_t flags;          /* BDL_STACK_FIRST | BDL_STACK_FINAL                         */
} bdl_stack_fit_args;

/* Device scratch of either entry point for `voters` voters and `cols` columns
 * (gather: cap; fit: n_cols): one partial of voters + 3 words per tile of the
 * fit, and at least the gather's BDL_STACK_MAX_GRID x 3 counts.  0 if an
 * argument is out of range. */
int64_t bdl_stack_workspace_bytes(int32_t voters, int64_t cols);

/* Two launches on hip_stream.  Validation comes before any HIP call:
 * BDL_ERR_NULL (args, logp, labels, ell, valid, counters, workspace),
 * BDL_ERR_ALIGN (logp, ell or valid not 4-B aligned; labels, counters or the
 * workspace not 8-B aligned), BDL_ERR_ARG (voters, batch, classes, cap, off or
 * grid_blocks out of range; off + batch > cap; an unknown flag;
 * voters*batch*classes*4 not representable in int64; a written span — ell,
 * valid, counters, the workspace — overlapping an input or another one; a graph
 * redirect active on the thread). */
int bdl_stack_gather(const bdl_stack_gather_args* args, void* hip_stream);

/* 2 * iterations launches on hip_stream (+ 2 with BDL_STACK_FINAL), no host
 * synchronisation.  The caller enqueues chunks back to back and may read the
 * state's 4-byte `converged` between them.  Validation comes before any HIP
 * call: BDL_ERR_NULL (args, ell, valid, state, workspace), BDL_ERR_ALIGN (ell or
 * valid not 4-B aligned; state or the workspace not 8-B aligned), BDL_ERR_ARG
 * (voters, n_cols, cap, iterations or grid_blocks out of range; n_cols > cap;
 * tol negative or NaN; an unknown flag; nothing to enqueue; the state or the
 * workspace overlapping ell, valid or one another; a graph redirect active on
 * the thread). */
int bdl_stack_fit(const bdl_stack_fit_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_STACKING_H */
