/* bdl_layers.h — per-tensor R-hat and effective sample size of stacked chains.
 *
 * bdl_chain_diag (bdl_diag.h) and bdl_chain_ess (bdl_ess.h) summarise their
 * per-element value over the whole parameter vector.  The two entry points
 * here give the same summary once per tensor — which layers have not mixed —
 * from the same resident vectors in one fused sweep, with no per-element
 * output.  Purely additive to the ABI of bdl_sgmcmc.h (same status codes,
 * bdl_last_error, stream convention, graph-redirect refusal).
 *
 * Segment table: DEVICE memory, one row per tensor, (offset, numel) as two
 * int64, chain-local (chain k, element j of the tensor at
 * vec + k*4*chain_groups + offset + j), rows ascending and non-overlapping,
 * numel >= 1 and offset + numel <= n.  A frozen tensor gets a row too (its
 * elements come out degenerate); a chain's slot padding lies in no row and is
 * never read.  Nothing outside the rows is read.
 *
 * Contract.
 *   - Row t of the table holds what bdl_chain_diag / bdl_chain_ess would
 *     report in its summary if only tensor t's elements existed: the fields
 *     of bdl_diag_summary / bdl_ess_summary, the same conventions (degenerate
 *     and non-finite elements counted and left out; strict thresholds; the
 *     lowest index among equal extremes).
 *   - argmax / argmin are chain-local flat indices, the numbering of the
 *     whole-vector summaries (NOT relative to the tensor's offset).
 *   - A row with nothing evaluated has extreme 0 and arg -1.
 *   - The per-element values come from the same device code as the
 *     whole-vector kernels (one definition, instantiated by both units), so
 *     they are bit-identical to what those kernels write with rhat / ess
 *     requested.
 *   - Counts, extreme and arg are exact and independent of the launch
 *     geometry; *_sum differs between geometries only in the order of an fp64
 *     sum.  For a fixed grid_blocks a table is bit-identical run to run.
 *   - No atomics, no host synchronisation, no allocation.
 *
 * Traversal.  Every workgroup walks the table; of a segment it takes block
 * iterations of 256 float4 groups, grid-strided from a first workgroup that
 * is rotated by the segment index, a lane walking the K chains of its group
 * as in bdl_chain_diag / bdl_chain_ess.  All chains' slices of a tensor share
 * one misalignment mod 16 B (the slot is a multiple of 4 elements): the up to
 * 3 elements before the first and after the last 16-B boundary of the slice
 * are read element by element by one lane each of the rotated first
 * workgroup, the body in non-temporal 16-B loads.  One partial per
 * (workgroup, segment) goes to the workspace — an empty one from a workgroup
 * that takes no iteration of the segment — and a second launch, one workgroup
 * per segment, combines a segment's partials in workgroup order. */
#ifndef BDL_LAYERS_H
#define BDL_LAYERS_H

#include <stdint.h>

#include "bdl_diag.h"
#include "bdl_ess.h"
#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_LAYERS_MAX_SEGMENTS 65536  /* nsegments <= this (as bdl_stats.h)          */
#define BDL_LAYERS_MAX_GRID 1024       /* grid_blocks <= this                         */

typedef struct bdl_layer_segment {  /* a row of the device table: two int64 */
  int64_t offset;        /* the tensor's chain-local offset in the stacked vectors   */
  int64_t numel;         /* elements per chain, >= 1; offset + numel <= n            */
} bdl_layer_segment;

typedef struct bdl_diag_layers_args {
  const float* mom1;     /* stacked: chain k, element j at 4*chain_groups*k + j      */
  const float* mom2;     /* same layout; variance source per var_mode                */
  const bdl_layer_segment* segments;  /* DEVICE memory, 8-B aligned                  */
  bdl_diag_summary* table;            /* DEVICE [nsegments], 8-B aligned: the output */
  void*  workspace;      /* bdl_layers_workspace_bytes(nsegments, grid_blocks) bytes,
                            16-B aligned, device memory                              */
  int64_t n;             /* elements per chain the rows lie in, 1 <= n <= 4*chain_groups */
  uint64_t chain_groups;
  int32_t nsegments;     /* 1 .. BDL_LAYERS_MAX_SEGMENTS                             */
  int32_t chains;        /* K >= 2                                                   */
  int32_t var_mode;      /* bdl_var_mode, as bdl_chain_diag                          */
  int32_t grid_blocks;   /* workgroups of the sweep, 1 .. BDL_LAYERS_MAX_GRID (0:
                            default, two per CU, at most BDL_LAYERS_MAX_GRID)        */
  float ratio, inv_ratio, var_floor;  /* as bdl_chain_diag_args                      */
  float c1;              /* fl32((count-1)/count), count = samples per chain >= 2    */
  float thresholds[3];
  int32_t pad0;
} bdl_diag_layers_args;

typedef struct bdl_ess_layers_args {
  const float* sM2;      /* stacked: chain k, element j at 4*chain_groups*k + j      */
  const float* bM2;      /* same layout                                              */
  const bdl_layer_segment* segments;  /* DEVICE memory, 8-B aligned                  */
  bdl_ess_summary* table;             /* DEVICE [nsegments], 8-B aligned: the output */
  void*  workspace;      /* as bdl_diag_layers_args                                  */
  int64_t n;             /* elements per chain the rows lie in, 1 <= n <= 4*chain_groups */
  uint64_t chain_groups;
  int64_t samples;       /* S folded per chain, 2 <= S < BDL_ESS_MAX_COUNT           */
  int64_t batches;       /* nb closed per chain, 2 <= nb <= S                        */
  int32_t nsegments;     /* 1 .. BDL_LAYERS_MAX_SEGMENTS                             */
  int32_t chains;        /* K, 1 .. BDL_ESS_MAX_CHAINS (1: one chain's slice alone)  */
  int32_t grid_blocks;   /* as bdl_diag_layers_args                                  */
  float thresholds[3];
} bdl_ess_layers_args;

/* Device scratch of one call of either entry point: one partial per
 * (workgroup, segment).  grid_blocks = 0 sizes it for BDL_LAYERS_MAX_GRID
 * workgroups (what the default may use).  0 if an argument is out of range. */
int64_t bdl_layers_workspace_bytes(int32_t nsegments, int32_t grid_blocks);

/* Two launches each on hip_stream (the sweep; the combine, one workgroup per
 * segment), no host synchronisation, no allocation.  Only table[0, nsegments)
 * and bdl_layers_workspace_bytes(nsegments, grid_blocks) bytes of the
 * workspace are written.
 *
 * Validation comes before any HIP call: BDL_ERR_NULL (args, an input vector,
 * segments, table, workspace), BDL_ERR_ALIGN (an input vector or the workspace
 * not 16-B aligned; segments or table not 8-B aligned), BDL_ERR_ARG (the
 * checks bdl_chain_diag / bdl_chain_ess make of the same fields — chains, n,
 * chain_groups, var_mode, var_floor, samples, batches —, nsegments or
 * grid_blocks out of range, the table or the workspace overlapping an input
 * vector, the segment table or each other, or a graph redirect active on the
 * thread).  The segment table lives in device memory, so its ENTRIES cannot be
 * validated on the host: the caller guarantees the rows as described above,
 * and that every chain's slice of every row lies inside the input vectors'
 * allocations. */
int bdl_chain_diag_layers(const bdl_diag_layers_args* args, void* hip_stream);
int bdl_chain_ess_layers(const bdl_ess_layers_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_LAYERS_H */
