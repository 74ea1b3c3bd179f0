/* bdl_rank.h — exact rank statistics of score rows against 0 / 1 marks: the
 * integer pair counts behind AUROC, average precision and the false-positive
 * rate at a true-positive rate, by counting ALL pairs.
 *
 * The stacked samplers' per-example uncertainty scores (bdl_predict's entropy,
 * mutual_info, ...) answer two rank questions: do the misclassified examples
 * rank above the others, do the examples of a shifted set rank above the
 * in-distribution ones.  bdl_rank reads `rows` score rows and their marks and
 * gives, per row, integer totals in DEVICE memory that the host reads once.
 * Counted exactly, they do not depend on the launch geometry or on any order;
 * there is no sort, no atomic and no scratch beyond 12 B per example.  The
 * price is an O(n^2) count per row.  Purely additive to the ABI of
 * bdl_sgmcmc.h (same status codes, bdl_last_error, stream convention,
 * graph-redirect refusal).
 *
 * Input.  scores: fp32, contiguous [rows, n]; higher means "more positive".
 * marks: int32, contiguous [mark_rows, n]; mark_rows = rows / scores_per_group
 * (row r reads mark row r / scores_per_group: the rows of a group share their
 * marks) or 1 (every row reads mark row 0).  Mark 1 is a positive, mark 0 a
 * negative, any other value EXCLUDES the example, and so does a NaN score.
 * +inf and -inf are ordinary ordered values, -0.0 equals +0.0, subnormals are
 * compared as numbers (never flushed: the comparison is on an integer key of
 * the bits, whatever the denormal mode).  An excluded example counts in
 * n_excluded and in nothing else, neither as i nor as j.
 *
 * Definitions, per row over the valid examples (P positives, Nn negatives);
 * every one an integer:
 *   ge_pos_i = #{j : m_j = 1, x_j >= x_i}    ge_neg_i = #{j : m_j = 0, x_j >= x_i}
 *   gt_neg_i = #{j : m_j = 0, x_j >  x_i}    (all three 0 for an excluded i)
 *   u2 = sum over positives i of (2*Nn - ge_neg_i - gt_neg_i): twice the
 *     Mann-Whitney U with ties counted half; AUROC = u2 / (2 * P * Nn).
 *   fp_at_tpr = min over valid i with ge_pos_i >= need of ge_neg_i: the fewest
 *     false positives of a threshold that keeps `need` true positives; -1 where
 *     no i qualifies (P = 0, or need > P).  need: args.need where it is > 0,
 *     else ceil(P * tpr_num / tpr_den) in int64 arithmetic on the device
 *     ((P * tpr_num + tpr_den - 1) / tpr_den; 19 / 20 for the FPR at 95 % TPR) —
 *     no floating point decides it.
 *   ap_sum = sum over positives i of ge_pos_i / (ge_pos_i + ge_neg_i), fp64:
 *     sklearn's average precision times P (tied positives share their
 *     threshold's precision).  Each quotient is one fp64 division of two
 *     exactly converted integers.
 *
 * Geometry.  Two launches.  (1) The count: grid (ceil(n / BDL_RANK_ITILE),
 * rows), 256 threads.  A workgroup holds BDL_RANK_ITILE = 256 * BDL_RANK_U
 * examples i of one row in registers (thread t the examples tile + t + 256*u)
 * and walks the row's j in tiles of BDL_RANK_JTILE staged in LDS as two key
 * arrays (positives, negatives; an excluded j or one past n is a key no
 * comparison accepts); in the inner loop every lane reads the same 16 B (an
 * LDS broadcast).  A tile is loaded in 16-B loads where the row starts 16-B
 * aligned (always when n % 4 == 0), the last group of a row element by
 * element, an unaligned row element by element.  A workgroup with no valid i
 * writes its zeros and leaves.  The counts go to the workspace and to the
 * non-null count outputs.  (2) The finalise: one workgroup per row; thread t
 * takes the examples t, t + 256, ... in ascending order, then the wave
 * butterfly of bdl_chain_common.hpp (off = 32 .. 1) and the waves 0 .. 3 in
 * order — the one order of ap_sum's fp64 sum, so a call is bit-identical run
 * to run (the geometry has no free parameter).  Every integer is independent
 * of all of it.
 *   - No atomics, no host synchronisation, no allocation.
 *
 * Limits: 1 <= n < 2^31 (the counts are uint32); 1 <= rows <=
 * BDL_RANK_MAX_ROWS. */
#ifndef BDL_RANK_H
#define BDL_RANK_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_RANK_U 2                       /* examples i per thread of the count        */
#define BDL_RANK_ITILE (256 * BDL_RANK_U)  /* examples i per workgroup                  */
#define BDL_RANK_JTILE 1024                /* examples j per LDS tile                   */
#define BDL_RANK_MAX_ROWS 65535            /* rows <= this (the grid's second dimension) */

typedef struct bdl_rank_totals {  /* per row; DEVICE memory, 8-B aligned */
  int64_t n_pos;       /* P: valid examples with mark 1                                  */
  int64_t n_neg;       /* Nn: valid examples with mark 0                                 */
  int64_t n_excluded;  /* another mark, or a NaN score                                   */
  int64_t u2;          /* twice the Mann-Whitney U (0 where P = 0 or Nn = 0)             */
  int64_t fp_at_tpr;   /* see above; -1 where no example qualifies                       */
  double ap_sum;       /* average precision times P                                      */
} bdl_rank_totals;

typedef struct bdl_rank_args {
  const float* scores;     /* [rows, n], 16-B aligned                                   */
  const int32_t* marks;    /* [mark_rows, n], 16-B aligned                              */
  /* per-example counts, each nullable (a null output is not written) */
  uint32_t* ge_pos;        /* [rows, n] each, 4-B aligned                               */
  uint32_t* ge_neg;
  uint32_t* gt_neg;
  bdl_rank_totals* totals; /* DEVICE [rows], 8-B aligned: overwritten                   */
  void* workspace;         /* bdl_rank_workspace_bytes(rows, n) bytes, 16-B aligned     */
  int64_t n;               /* 1 .. 2^31 - 1                                             */
  int64_t need;            /* > 0: the true positives fp_at_tpr keeps, for every row;
                              0: ceil(P * tpr_num / tpr_den) of each row                */
  int32_t rows;            /* 1 .. BDL_RANK_MAX_ROWS                                    */
  int32_t scores_per_group;/* >= 1, divides rows                                        */
  int32_t mark_rows;       /* rows / scores_per_group, or 1                             */
  int32_t tpr_num;         /* 1 <= tpr_num <= tpr_den (read where need = 0)             */
  int32_t tpr_den;
  int32_t pad0;            /* must be 0                                                 */
} bdl_rank_args;

/* Device scratch of one call: the three counts of every example (12 B each),
 * rounded up to 16 B.  0 if an argument is out of range. */
int64_t bdl_rank_workspace_bytes(int32_t rows, int64_t n);

/* Two launches on hip_stream (the count; the finalise, one workgroup per row),
 * no host synchronisation, no allocation.  Only the non-null count outputs,
 * totals[0, rows) and bdl_rank_workspace_bytes(rows, n) bytes of the workspace
 * are written.
 *
 * Validation comes before any HIP call: BDL_ERR_NULL (args, scores, marks,
 * totals, workspace), BDL_ERR_ALIGN (scores, marks or the workspace not 16-B
 * aligned; totals not 8-B aligned; a count output not 4-B aligned),
 * BDL_ERR_ARG (rows or n out of range; scores_per_group < 1 or not dividing
 * rows; mark_rows neither rows / scores_per_group nor 1; need < 0; tpr_num /
 * tpr_den not 1 <= tpr_num <= tpr_den; pad0 != 0; a count output, totals or the
 * workspace overlapping scores, marks or one another; a graph redirect active
 * on the thread). */
int bdl_rank(const bdl_rank_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_RANK_H */
