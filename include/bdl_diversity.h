/* bdl_diversity.h — pairwise diversity of an ensemble's voters from their
 * logits, in one fused sweep: for every ordered pair (i, j) of P voters, how
 * often their votes differ, how often both are wrong, the total-variation
 * distance and the Kullback-Leibler divergence between their predictive
 * distributions, summed over any number of calls in DEVICE memory.
 *
 * The stacked samplers leave every chain's own log mixture [K, B, C] on the
 * device (bdl_predict with groups = K).  bdl_diversity reads those rows once and
 * keeps the P x P totals there; the host reads them once, after a whole loader.
 * Purely additive to the ABI of bdl_sgmcmc.h (same status codes,
 * bdl_last_error, stream convention, graph-redirect refusal).
 *
 * Input.  logits: fp32, contiguous [voters, batch, classes]; a log-probability
 * row is a valid logit row.  labels: optional int64 [batch] in device memory; a
 * label outside [0, classes) leaves the example unlabelled: it counts in n,
 * disagree, tv_sum, kl_sum and kl_unbounded, not in n_labelled or both_wrong,
 * and it is never used as an index.
 *
 * Definitions, per example b and voter i (natural log):
 *   m_i = max_c x_i[c]   d = x_i[c] - m_i   e = expf(d)   Z_i = sum_c e
 *   p_i[c] = e / Z_i     lp_i[c] = d - log Z_i
 *   a_i = argmax_c x_i[c] (lowest index)     wrong_i = (a_i != label)
 * A class with d = -inf is MASKED for voter i: p = 0, lp = -inf.  That is a
 * -inf logit (and a finite one more than FLT_MAX below the row's maximum, which
 * no row of a classifier holds).  An example is NON-FINITE if any voter's row
 * holds a NaN, a +inf or no finite entry (bdl_predict's rule): it counts in
 * n_nonfinite and in nothing else.
 *
 * Totals, per ordered cell (i, j), over the evaluated examples:
 *   disagree[i][j]     #{b : a_i != a_j}                   symmetric, diagonal 0
 *   both_wrong[i][j]   #{labelled b : wrong_i and wrong_j} symmetric; the
 *                      diagonal is voter i's error count
 *   tv_sum[i][j]       sum_b 0.5 * sum_c |p_i[c] - p_j[c]| symmetric, diagonal 0
 *   kl_sum[i][j]       sum_b KL(p_i || p_j) = sum_b sum_c p_i[c] (lp_i[c] - lp_j[c]),
 *                      a class masked for i contributing 0; directed, diagonal 0
 *   kl_unbounded[i][j] #{b : KL(p_i || p_j) is infinite}: some class is masked
 *                      for j and not for i.  Decided on d, that is on the input,
 *                      so the count is exact and independent of expf.  Such an
 *                      example is left out of kl_sum[i][j] — of that cell only.
 *
 * Arithmetic contract (tests/diversity_ref.py emulates it and derives the
 * bounds from it).  u = 2^-24.
 *   fp32, one rounding each:  m_i (exact);  d = x - m_i;  e = expf(d);
 *     log Z_i = logf((float)Z_i);  p = (float)(e * (1/Z_i)) (the reciprocal and
 *     the product in fp64);  lp = d - log Z_i;  the differences p_i[c] - p_j[c]
 *     and lp_i[c] - lp_j[c].  expf / logf are the HIP device library's,
 *     documented maximum error 1 ulp each; -ffp-contract=off.
 *   fp64:  Z_i = sum_c e (a lane's classes ascending, then the wave butterfly
 *     of bdl_chain_common.hpp);  an example's sum_c |p_i - p_j| and sum_c p_i *
 *     (lp_i - lp_j) (the product is exact in fp64, so one fused multiply-add
 *     rounds as the separate add would), c ASCENDING in one thread;  the factor
 *     0.5 once per example (exact);  the sums over examples.
 *
 * Geometry.  Two launches.  (1) The sweep.  An example is handled by a TEAM
 * that holds p and lp of all voters for a tile of BDL_DIVERSITY_TILE classes in
 * LDS, rows BDL_DIVERSITY_LDS_STRIDE floats apart: 4 mod 64, so that the 16-B
 * reads of up to 16 different voters' rows at one class fall on 64 different
 * banks.  Pass 1: one wave per voter row finds m_i, a_i, the non-finite flag,
 * then Z_i (wave shuffles only).  Pass 2, per tile: the team re-reads the rows
 * (cache-resident: voters * classes * 4 B <= 2 MiB), writes p and lp into LDS,
 * and thread t of the team runs over the tile's classes for the pairs t, t +
 * team size, ... (i < j in row-major order) it owns.  A thread's pair
 * accumulators stay in its registers over all of the workgroup's examples.
 *   - voters <= BDL_DIVERSITY_WAVE_VOTERS and classes <= BDL_DIVERSITY_TILE: the
 *     team is one WAVE (at most 120 pairs, two per lane; one tile), four examples
 *     per workgroup; the four waves' totals are added in wave order.
 *   - otherwise the team is the WORKGROUP (256 threads, one example at a time;
 *     1, 2, 4 or 8 pairs per thread for voters <= 23, 32, 45, 64).
 *   - rows are read in 16-B loads where classes % 4 == 0 (every row is then
 *     16-B aligned; the last read of a row is non-temporal), else element by
 *     element.
 *   Examples are grid-strided over the workgroups; every workgroup that has an
 *   example writes one partial (the layout of the totals) to the workspace.
 * (2) The combine: thread w of it adds 8-B word w of the partials in workgroup
 * order and adds the result to — with BDL_DIVERSITY_RESET: writes it over —
 * the totals.
 *   - Every integer is independent of grid_blocks and of any order.  An
 *     example's contribution to tv_sum / kl_sum is independent of grid_blocks
 *     (one thread owns a pair over all classes, c ascending); the sums over
 *     examples differ between grid_blocks values only in the fp64 order.  For a
 *     fixed grid_blocks a call is bit-identical run to run.
 *   - No atomics, no host synchronisation, no allocation.
 *
 * Workspace.  A partial is bdl_diversity_totals_bytes(voters) = 32 + 40 * P^2
 * bytes (163,872 B at P = 64).  grid_blocks <= BDL_DIVERSITY_MAX_GRID, and the
 * default grid (one workgroup per team-load of examples up to two per CU) is
 * further capped so that the workspace stays within
 * BDL_DIVERSITY_DEFAULT_WORKSPACE = 32 MiB: 204 workgroups at P = 64, the full
 * 1024 up to P = 28. */
#ifndef BDL_DIVERSITY_H
#define BDL_DIVERSITY_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_DIVERSITY_MAX_VOTERS 64     /* 2 <= voters <= this (2016 pairs, 8 per thread) */
#define BDL_DIVERSITY_MAX_CLASSES 8192  /* classes <= this                                */
#define BDL_DIVERSITY_WAVE_VOTERS 16    /* voters <= this and classes <= TILE: one wave   */
#define BDL_DIVERSITY_TILE 64           /* classes per LDS tile                           */
#define BDL_DIVERSITY_LDS_STRIDE 68     /* floats between two voters' rows of a tile      */
#define BDL_DIVERSITY_MAX_GRID 1024     /* grid_blocks <= this                            */
#define BDL_DIVERSITY_DEFAULT_WORKSPACE (32 << 20) /* the default grid's workspace bound  */

typedef enum bdl_diversity_flag {
  BDL_DIVERSITY_RESET = 0x1  /* the totals are overwritten, not added to (no memset needed) */
} bdl_diversity_flag;

/* The totals: DEVICE memory, 8-B aligned, bdl_diversity_totals_bytes(P) bytes —
 * this header, then five row-major [P][P] matrices of 8-B cells in this order:
 *   int64 disagree, int64 both_wrong, int64 kl_unbounded, double tv_sum,
 *   double kl_sum. */
typedef struct bdl_diversity_header {
  int64_t n;            /* examples evaluated (finite), labelled or not            */
  int64_t n_labelled;   /* ... of them with a label in [0, classes)                */
  int64_t n_nonfinite;  /* examples left out (see above)                           */
  int64_t voters;       /* P, as the call that wrote the totals had it             */
} bdl_diversity_header;

typedef struct bdl_diversity_args {
  const float* logits;    /* [voters, batch, classes], 16-B aligned                    */
  const int64_t* labels;  /* DEVICE [batch] or null (every example unlabelled)         */
  void* totals;           /* DEVICE, bdl_diversity_totals_bytes(voters) bytes, 8-B
                             aligned: added to                                         */
  void* workspace;        /* bdl_diversity_workspace_bytes(voters, grid_blocks) bytes,
                             16-B aligned, device memory                               */
  int64_t batch;          /* B >= 1                                                    */
  int32_t voters;         /* P, 2 .. BDL_DIVERSITY_MAX_VOTERS                          */
  int32_t classes;        /* C, 1 .. BDL_DIVERSITY_MAX_CLASSES                         */
  int32_t grid_blocks;    /* workgroups of the sweep, 1 .. BDL_DIVERSITY_MAX_GRID (0:
                             the default, see above)                                   */
  int32_t flags;          /* bdl_diversity_flag bits                                   */
} bdl_diversity_args;

/* 32 + 40 * voters^2; 0 if voters is out of range. */
int64_t bdl_diversity_totals_bytes(int32_t voters);

/* Device scratch of one call: one partial (rounded up to 16 B) per workgroup.
 * grid_blocks = 0 sizes it for the largest grid the default may use.  0 if an
 * argument is out of range. */
int64_t bdl_diversity_workspace_bytes(int32_t voters, int32_t grid_blocks);

/* Two launches on hip_stream (the sweep; the combine), no host
 * synchronisation, no allocation.  Only the totals and
 * bdl_diversity_workspace_bytes(voters, grid_blocks) bytes of the workspace are
 * written.
 *
 * Validation comes before any HIP call: BDL_ERR_NULL (args, logits, totals,
 * workspace), BDL_ERR_ALIGN (logits or the workspace not 16-B aligned; labels or
 * totals not 8-B aligned), BDL_ERR_ARG (voters, batch, classes or grid_blocks
 * out of range; an unknown flag; voters*batch*classes*4 not representable in
 * int64; totals or the workspace overlapping logits, labels or one another; a
 * graph redirect active on the thread). */
int bdl_diversity(const bdl_diversity_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_DIVERSITY_H */
