/* bdl_clip.h — per-chain gradient clipping of stacked chains.
 *
 * K chains of one network are stepped by one launch (bayesdll_amd.stacked,
 * bdl_step_args.chain_groups).  They stand for K independent Runners, and a
 * Runner that clips calls clip_grad_norm_ on its own gradient
 * (methods/csgld.py:250-253, methods/adam_csghmc.py:319-322), so each chain
 * is clipped by the norm of ITS OWN gradient.  bdl_chain_clip does that on
 * the device for all K chains: a segmented squared-norm sweep, a per-chain
 * finalize and an in-place scale sweep.  Purely additive to the ABI of
 * bdl_sgmcmc.h (same status codes, bdl_last_error, stream convention).
 *
 * The gradient is described by segments: one per gradient tensor, each
 * holding that tensor of all K chains (chain k, element j at
 * base + k*chain_stride + j).  One form covers both layouts of the stacked
 * state: the vmapped [K, *shape] gradient tensors (base = the tensor,
 * chain_stride = numel) and the stacked gradient vector (base = grad +
 * the tensor's offset, chain_stride = the chain slot).  A tensor without a
 * gradient gets no segment: it is not in the norm and is not scaled.
 * Segments must not overlap.
 *
 * Arithmetic (part of the contract; tests/chain_clip_ref.py restates it; it
 * is that of bdl_sgld_step_clipped's norm and finalize, per chain):
 *
 *   s_k    = sum over chain k's segment elements of (double)g * (double)g
 *            (fp64 fma accumulation)
 *   norm_k = fl32(sqrt(s_k))
 *   coef_k = fminf( fl32( fl32(1 / fl32(norm_k + 1e-6f)) * max_norm ), 1 )
 *   g     <- fl32(g * coef_k)   for every element of chain k, if coef_k < 1
 *
 * A chain with coef_k == 1 (fminf: a NaN norm too) is not written at all:
 * x * 1.0f is x bit for bit.  (norm_k, coef_k), k = 0 .. K-1, stand at the
 * start of the workspace as 2K floats.
 *
 * Non-finite norms (part of the contract; bdl_sgld_step_clipped's one-chain
 * finalize follows the same two rules):
 *   NaN   a NaN among chain k's elements gives norm_k = NaN and, by fminf,
 *         coef_k = 1: the chain is left exactly as it is.  This deviates from
 *         torch.nn.utils.clip_grad_norm_, which multiplies every gradient of
 *         that model by NaN; here the NaN stays where it was and the other
 *         chains are clipped as usual.
 *   +Inf  an infinite element, or a sum of squares whose root exceeds FLT_MAX,
 *         gives norm_k = +Inf and coef_k = 0: finite elements become +-0 with
 *         their sign, infinite ones NaN (as torch).
 *
 * The sum is reduced without atomics: per-lane fp64 accumulators, a 64-lane
 * butterfly, the workgroup's waves through LDS, one partial per workgroup,
 * and per chain one workgroup that combines that chain's partials in a fixed
 * order.  For a fixed geometry (blocks_per_chain) the result is bit-identical
 * run to run; between geometries only the fp64 summation order differs, which
 * leaves norm_k within one fp32 ulp.
 *
 * Alignment.  A chain's slice of a segment need not be 16-B aligned (an odd
 * numel, a base that is a view): its first (up to 3) elements before the
 * first 16-B boundary and its last (up to 3) after the last one are accessed
 * element by element, the rest in 16-B non-temporal accesses.  No byte outside
 * [base + k*chain_stride, base + k*chain_stride + numel) is read or written. */
#ifndef BDL_CLIP_H
#define BDL_CLIP_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_CLIP_MAX_SEGMENTS 65536         /* nsegments <= this                     */
#define BDL_CLIP_MAX_CHAINS 65535           /* chains <= this (the grid's y extent)  */
#define BDL_CLIP_MAX_BLOCKS_PER_CHAIN 1024  /* blocks_per_chain <= this              */

typedef struct bdl_clip_segment {   /* one gradient tensor of all K chains */
  float*  base;          /* chain k, element j at base + k*chain_stride + j   */
  int64_t numel;         /* elements per chain, >= 1                          */
  int64_t chain_stride;  /* elements between chains, >= numel                 */
} bdl_clip_segment;

typedef struct bdl_chain_clip_args {
  const bdl_clip_segment* segments;  /* DEVICE memory, 8-B aligned                    */
  int32_t nsegments;                 /* 1 .. BDL_CLIP_MAX_SEGMENTS                    */
  int32_t chains;                    /* K, 1 .. BDL_CLIP_MAX_CHAINS                   */
  float   max_norm;                  /* > 0                                           */
  int32_t blocks_per_chain;          /* workgroups per chain, 1 ..
                                        BDL_CLIP_MAX_BLOCKS_PER_CHAIN (0: default,
                                        about four workgroups per CU over all chains) */
  void*   workspace;                 /* bdl_chain_clip_workspace_bytes(chains) bytes,
                                        16-B aligned, device memory                   */
} bdl_chain_clip_args;

/* Device scratch of one bdl_chain_clip call: (norm_k, coef_k) as 2*chains
 * floats, then the per-workgroup partial sums.  0 if chains is out of range. */
int64_t bdl_chain_clip_workspace_bytes(int32_t chains);

/* Three launches on hip_stream — the norm sweep and the scale sweep on a
 * (blocks_per_chain, chains) grid, so that every workgroup stays inside one
 * chain, and between them a per-chain finalize; the scale sweep's workgroups
 * of an unclipped chain exit after one scalar read.  No host synchronisation,
 * no allocation; only bdl_chain_clip_workspace_bytes(chains) bytes of the
 * workspace are written.  Values never depend on blocks_per_chain beyond the
 * fp64 summation order.
 *
 * Validation comes before any HIP call: BDL_ERR_NULL (args, segments,
 * workspace), BDL_ERR_ALIGN (workspace not 16-B aligned, segments not 8-B
 * aligned), BDL_ERR_ARG (chains, nsegments or blocks_per_chain outside its
 * range, max_norm not > 0 — NaN included —, or a graph redirect active on the
 * thread).  The segment table lives in device memory, so its ENTRIES cannot
 * be validated on the host: the caller guarantees numel >= 1, chain_stride >=
 * numel, 4-B aligned bases and that every slice lies inside an allocation. */
int bdl_chain_clip(const bdl_chain_clip_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_CLIP_H */
