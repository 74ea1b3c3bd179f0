/* bdl_order.h — the dynamic sweep order of the cSGHMC step and its drift probe.
 *
 * Additive to the ABI of bdl_sgmcmc.h (no version bump; nothing there changes
 * but one more accepted value of an existing argument).  No reference
 * counterpart: the reference has no kernels.
 *
 * bdl_set_launch_config(blocks_per_cu, unroll, order) takes a third order:
 *   0  one contiguous span per workgroup
 *   1  grid-stride (workgroup b runs iterations b, b + grid, ...)
 *   2  dynamic: the vector is cut into claim blocks of BDL_CLAIM_GROUPS float4
 *      groups; workgroup b takes block b first and then claims ascending blocks
 *      from one device counter until none is left.
 * Order 2 applies to bdl_sgmcmc_step / bdl_sgmcmc_step_bare launches of method
 * BDL_CSGHMC only; every other method and entry point treats it as order 1.
 * Results never depend on the order.
 *
 * The counters: the library owns BDL_CLAIM_SLOTS {claim, done} pairs per
 * device, allocated and zeroed once at the first order-2 launch there.  The
 * last workgroup of a launch to finish stores zeros to the launch's pair, so
 * no memset and no second launch runs per step.  A slot is bound to the stream
 * that first launched on it (launches of one stream run in order, so the pair
 * is zero again before the next one starts); a stream holds at most
 * BDL_CLAIM_SLOTS_PER_STREAM slots and takes them in turn.  A launch that
 * cannot be given a slot this way runs order 1 instead: a launch into a stream
 * capture, a graph-node rewrite (bdl_graph_redirect), a launch on a stream
 * with no slot left to bind. */
#ifndef BDL_ORDER_H
#define BDL_ORDER_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#define BDL_CLAIM_GROUPS 2048         /* float4 groups per claim block (32 KiB per stream)  */
#define BDL_CLAIM_SLOTS 16            /* {claim, done} pairs per device                    */
#define BDL_CLAIM_SLOTS_PER_STREAM 4  /* of which one stream binds at most this many       */

#define BDL_DRIFT_EVERY 16   /* a sample at every 16th iteration of a workgroup */
#define BDL_DRIFT_SAMPLES 64 /* at most this many samples per workgroup         */
#define BDL_DRIFT_WORDS (4 + 2 * BDL_DRIFT_SAMPLES)

#ifdef __cplusplus
extern "C" {
#endif

/* The order the calling thread's last bdl_sgmcmc_step / bdl_sgmcmc_step_bare
 * launch ran (0, 1 or 2), and the slot it used (-1: none) in *slot if non-null.
 * -1 before any launch. */
int bdl_order_last(int32_t* slot);

/* Copy the 2 * BDL_CLAIM_SLOTS counters of `device` ({claim, done} per slot)
 * to out after a device synchronize; zeros if none were allocated yet.
 * Between launches every one of them is zero. */
int bdl_order_counters(int32_t device, uint32_t* out);

/* Measurement only.  One launch of the cSGHMC explore sweep of `args`
 * (method BDL_CSGHMC, no noise, no collect: it is a real step) at the current
 * launch configuration, each workgroup recording BDL_DRIFT_WORDS 64-bit words
 * to records[workgroup]: the wall clock (100 MHz) at its first load and after
 * its last store, the samples taken, the iterations run, and (wall clock,
 * global iteration index) at every BDL_DRIFT_EVERY-th of its iterations.
 * order: 0 / 1 / 2 as above (2 needs a slot: BDL_ERR_ARG otherwise).
 * record_bytes must hold the launch's workgroups (returned in *grid). */
int bdl_sweep_drift(const bdl_step_args* args, int32_t order, uint64_t* records,
                    int64_t record_bytes, int32_t* grid, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_ORDER_H */
