/* bdl_stats.h — per-chain, per-tensor sufficient statistics of stacked chains.
 *
 * K chains of one network are stepped by one launch (bayesdll_amd.stacked).
 * A sweep over lr / momentum_decay / nd raises one question first: does each
 * chain sample at the temperature its injected noise stands for, and in which
 * layers is it heated?  The kinetic and the configurational temperature of
 * Wenzel et al. 2020 answer it per tensor; both are ratios of a few inner
 * products of theta, the momentum and the gradient taken at the SAME theta,
 * i.e. between the backward pass and the update.  bdl_chain_stats reduces
 * those inner products for all (chain, tensor) pairs in one sweep and adds
 * them to a device accumulator.  Purely additive to the ABI of bdl_sgmcmc.h
 * (same status codes, bdl_last_error, stream convention).
 *
 * Segments: one row per tensor that has a gradient, holding that tensor of
 * all K chains.  The gradient is addressed as in bdl_clip.h (chain k, element
 * j at grad + k*grad_stride + j: the vmapped [K, *shape] tensor with
 * grad_stride = numel, or a span of the stacked gradient vector with
 * grad_stride = the chain slot); theta, mom and prior_mean are the stacked
 * [K, 4*chain_groups] vectors, the tensor at chain-local `offset`:
 * chain k, element j at vec + k*4*chain_groups + offset + j.  A frozen tensor
 * and a chain's slot padding lie in no row and are never read.
 *
 * Arithmetic (part of the contract; tests/chain_stats_ref.py restates it).
 * Per launch and per (chain k, segment t), over the tensor's elements:
 *
 *   d   = fl32(theta - prior_mean)   (theta itself when prior_mean is NULL;
 *                                     one fp32 rounding, as the step forms it)
 *   G2  = sum g*g   V2 = sum v*v   D2 = sum d*d   DG = sum d*g   VG = sum v*g
 *                                    (V2 and VG are 0 when mom is NULL)
 *   V2L = V2 * (1.0 / (double)lr[k][lr_group])
 *
 * Every factor is a float converted to double, so every product is exact;
 * the sums are accumulated with fp64 fma.  They are reduced without atomics:
 * per-lane accumulators, a 64-lane butterfly, the workgroup's waves through
 * LDS, one partial per (workgroup, segment) in the workspace, and a second
 * launch that combines them in workgroup order and updates
 *
 *   acc[k][t][0..5] = (G2, V2, D2, DG, VG, V2L)      (accumulate == 0)
 *   acc[k][t][q]   += the same                        (accumulate == 1)
 *
 * For a fixed blocks_per_chain the result is bit-identical run to run;
 * between geometries, and between the two load paths below, only the fp64
 * summation order differs.
 *
 * Alignment.  Where chain k's slice of the gradient and of the stacked
 * vectors share one misalignment mod 16 B, the (up to 3) elements before the
 * first 16-B boundary and after the last are read element by element and the
 * rest in 16-B loads; where they differ (row k of a [K, numel] gradient with
 * an odd numel) that (chain, segment) pair is read element by element.  No
 * byte outside the slices is read, and nothing but acc and the workspace is
 * written. */
#ifndef BDL_STATS_H
#define BDL_STATS_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_STATS_MAX_SEGMENTS 65536        /* nsegments <= this                     */
#define BDL_STATS_MAX_CHAINS 65535          /* chains <= this (the grid's y extent)  */
#define BDL_STATS_MAX_BLOCKS_PER_CHAIN 256  /* blocks_per_chain <= this              */
#define BDL_STATS_MAX_CHAIN_GROUPS (1ll << 40)
#define BDL_STATS_SUMS 6                    /* doubles per (chain, segment) of acc   */

typedef struct bdl_stats_segment {  /* one gradient tensor of all K chains: five int64 */
  const float* grad;     /* chain k, element j at grad + k*grad_stride + j          */
  int64_t numel;         /* elements per chain, >= 1                                */
  int64_t grad_stride;   /* elements between chains of the gradient, >= numel       */
  int64_t offset;        /* the tensor's chain-local offset in the stacked vectors  */
  int64_t lr_group;      /* 0: body lr, 1: head lr                                  */
} bdl_stats_segment;

typedef struct bdl_chain_stats_args {
  const float* theta;       /* stacked [K, 4*chain_groups], 16-B aligned               */
  const float* mom;         /* the same shape, or NULL (V2 = VG = V2L = 0)             */
  const float* prior_mean;  /* the same shape, or NULL (d = theta)                     */
  const bdl_stats_segment* segments;  /* DEVICE memory, 8-B aligned                    */
  const float* lr_table;    /* DEVICE memory, 4-B aligned, or NULL: chain k's body /
                               head lr at lr_table[k*lr_row_stride + 0 / 1] (the rows
                               of bdl_chain_scalars: lr_row_stride = 12)               */
  double* acc;              /* DEVICE [chains][nsegments][BDL_STATS_SUMS], 8-B aligned */
  void*   workspace;        /* bdl_chain_stats_workspace_bytes(chains, nsegments)
                               bytes, 16-B aligned, device memory                      */
  uint64_t chain_groups;    /* float4 groups per chain slot, 1 ..
                               BDL_STATS_MAX_CHAIN_GROUPS                              */
  int32_t nsegments;        /* 1 .. BDL_STATS_MAX_SEGMENTS                             */
  int32_t chains;           /* K, 1 .. BDL_STATS_MAX_CHAINS                            */
  int32_t lr_row_stride;    /* floats between rows of lr_table, >= 2 (unused without)  */
  int32_t accumulate;       /* 0: acc is overwritten, 1: added to                      */
  int32_t blocks_per_chain; /* workgroups per chain, 1 .. BDL_STATS_MAX_BLOCKS_PER_CHAIN
                               (0: default, about four per CU over all chains)         */
  int32_t pad0;
  float   lr[2];            /* body / head lr of every chain, both > 0 — or both 0
                               when lr_table is given: exactly one source              */
} bdl_chain_stats_args;

/* Device scratch of one bdl_chain_stats call: five fp64 partial sums per
 * (workgroup, segment) of the largest grid.  0 if an argument is out of range. */
int64_t bdl_chain_stats_workspace_bytes(int32_t chains, int32_t nsegments);

/* Two launches on hip_stream — the sweep on a (blocks_per_chain, chains) grid,
 * so that every workgroup stays inside one chain, and the combine that
 * updates acc.  No host synchronisation, no allocation, no atomics.
 *
 * Validation comes before any HIP call: BDL_ERR_NULL (args, theta, segments,
 * acc, workspace), BDL_ERR_ALIGN (theta, mom, prior_mean or workspace not
 * 16-B aligned; segments or acc not 8-B aligned; lr_table not 4-B aligned),
 * BDL_ERR_ARG (chains, nsegments, chain_groups or blocks_per_chain outside
 * its range; both lr sources or neither; a host lr that is not > 0;
 * lr_row_stride < 2; accumulate not 0 / 1; or a graph redirect active on the
 * thread).  The segment table and lr_table live in device memory, so their
 * ENTRIES cannot be validated on the host: the caller guarantees numel >= 1,
 * grad_stride >= numel, offset + numel <= 4*chain_groups, lr_group 0 or 1,
 * 4-B aligned gradient bases, that every slice lies inside an allocation and
 * that the table's lrs are > 0. */
int bdl_chain_stats(const bdl_chain_stats_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_STATS_H */
