/* bdl_exchange.h — replica exchange (parallel tempering) between stacked SGLD
 * chains (Deng et al., ICML 2020: replica exchange SG-MCMC), on the device.
 *
 * K stacked chains whose noise multipliers nd_k differ sample exp(-U / T_k) with
 * T_k = nd_k^2 (momentum 0), U = N * loss + |theta - theta0|^2 / (2 sigma2): a
 * temperature ladder in one buffer.  Three entry points, one launch each, make
 * an exchange attempt between adjacent slots without a host read:
 * bdl_exchange_energy (the prior part of U), bdl_exchange_decide (the even-odd
 * Metropolis decisions and their bookkeeping), bdl_exchange_swap (the accepted
 * pairs' chain slots change places).  Purely additive to the ABI of
 * bdl_sgmcmc.h (same status codes, bdl_last_error, stream convention,
 * graph-redirect refusal).  No floating-point atomics, no allocation, no host
 * synchronisation; -ffp-contract=off; every result is independent of the grid.
 *
 * --------------------------------------------------------------- bdl_exchange_energy
 * The stacked layout of bdl_sgmcmc.h: chain k's slot is elements
 * [4*chain_groups*k, 4*chain_groups*(k+1)), its first n are real, the rest is
 * padding and is never read.  prior may be null (theta0 = 0: d = theta).
 *   q_k = sum_{i < n} d_i^2,  d_i = theta_k[i] - prior_k[i] in fp32 (one
 *   rounding), the square and every sum in fp64 (the square is exact).
 * A chain is cut into fixed TILES of BDL_EXCHANGE_TILE = 1024 elements; (chain
 * k, tile j) produces partial k * tiles + j (tiles = ceil(n / 1024)) whatever
 * the grid is; workgroups of 256 threads take the chains * tiles items
 * grid-strided.  In-tile order: thread t owns the float4 group of elements
 * 1024*j + 4*t .. + 3 and adds its squares x, y, z, w in that order from 0.0 (an
 * element >= n contributes +0.0); then the wave butterfly (xor 32, 16, .., 1);
 * then the four waves in wave order from wave 0's value.  Loads are 16-B
 * non-temporal; the group that holds element n - 1 when n % 4 != 0 is read
 * element-wise.
 * Cross-tile order (done by bdl_exchange_decide, one workgroup): for chain k
 * thread t adds partials t, t + 256, ... of the chain in ascending order from
 * 0.0; then the wave butterfly; then the four waves in wave order from wave 0's
 * value.  q_k is therefore bit-identical for every grid_blocks and every run.
 *
 * --------------------------------------------------------------- bdl_exchange_decide
 * One workgroup of 256 threads, fp64 throughout.  It first forms q_k as above
 * and stores it in state->q.  BDL_EXCHANGE_ENERGY_ONLY stops there: loss, beta
 * and the rest of the state are not read or written.  Otherwise, for attempt
 * index t (the caller counts attempts from 0):
 *   U_k = n_data * (double)loss[k] + q_k / (2.0 * sigma2)      (stored in state->U)
 *   pairs (i, i + 1), 0 <= i < chains - 1, with i % 2 == t % 2 (deterministic
 *     even-odd; the ladder order is the slot order);
 *   db = beta[i] - beta[i+1]  (beta_k = 1 / T_k, fp64, device memory);
 *   la = db * (U_i - U_{i+1}) - (db * db) * var;
 *   u = ((double)w + 0.5) * 2^-32 with w the FIRST word of Philox4x32-10 with
 *     counter (i, chain0 lo32, s lo32, s hi32), s = BDL_EXCHANGE_STEP_BASE + t,
 *     key (seed lo32, seed hi32): the step kernels' layout with the pair in the
 *     place of the float4 group and a step domain no training step (< 2^62) and
 *     no evaluation draw (2^62 + draws) reaches;
 *   accept iff U_i, U_{i+1} and la are finite and log(u) < la.  A non-finite
 *   U or la: no swap, ++refused.  attempts[i] counts every attempt of pair i
 *   (refused ones included), accepts[i] the accepted ones.
 *   partner[k] = k's partner slot for an accepted pair, else k.
 *   replica[s] is the initial replica that sits in slot s: the accepted pairs'
 *   entries change places.  Then, if chains >= 2: the replica r in slot 0 gets
 *   ++round_trips[r] if direction[r] == BDL_EXCHANGE_DOWN, and direction[r] =
 *   BDL_EXCHANGE_UP; the replica in slot chains - 1 gets direction =
 *   BDL_EXCHANGE_DOWN.
 * BDL_EXCHANGE_FIRST: the state is initialised before anything else (replica[s]
 * = s, every counter 0, direction 0 but UP for replica 0 and DOWN for replica
 * chains - 1 when chains >= 2; entries >= chains are 0).
 * With db == 0 (equal temperatures) la = 0 and every attempt is accepted.
 *
 * ----------------------------------------------------------------- bdl_exchange_swap
 * Reads state->partner.  Grid (blocks_per_chain, chains): the workgroups of
 * slot k load partner[k] and exit unless partner[k] > k (only the lower member
 * of an accepted pair works, so no element is touched by two workgroups).  The
 * others exchange the WHOLE slots k and partner[k] — all 4 * chain_groups
 * elements: the padding travels with its slot — of each of the 1 .. 4 vectors,
 * a float4 group per thread, grid-strided: each slot is read once and written
 * once, 16 B of traffic per element of a swapped pair and vector.
 *
 * Limits: chains <= BDL_EXCHANGE_MAX_CHAINS, vectors <= BDL_EXCHANGE_MAX_VECTORS. */
#ifndef BDL_EXCHANGE_H
#define BDL_EXCHANGE_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_EXCHANGE_MAX_CHAINS 64   /* 1 <= chains <= this                          */
#define BDL_EXCHANGE_MAX_VECTORS 4   /* 1 <= vectors of a swap <= this               */
#define BDL_EXCHANGE_TILE 1024       /* elements per tile of the energy sweep        */
#define BDL_EXCHANGE_MAX_GRID 65535  /* grid_blocks <= this                          */
#define BDL_EXCHANGE_STEP_BASE 0x8000000000000000ull /* Philox step domain (2^63)    */

typedef enum bdl_exchange_flag {
  BDL_EXCHANGE_FIRST = 0x1,       /* decide: initialise the state first              */
  BDL_EXCHANGE_ENERGY_ONLY = 0x2  /* decide: form state->q and stop                  */
} bdl_exchange_flag;

enum { BDL_EXCHANGE_UP = 1, BDL_EXCHANGE_DOWN = 2 };

/* DEVICE memory, 8-B aligned. */
typedef struct bdl_exchange_state {
  double q[BDL_EXCHANGE_MAX_CHAINS];             /* per slot: sum (theta - theta0)^2   */
  double U[BDL_EXCHANGE_MAX_CHAINS];             /* per slot: the last energies        */
  uint64_t attempts[BDL_EXCHANGE_MAX_CHAINS];    /* per pair (i, i + 1)                */
  uint64_t accepts[BDL_EXCHANGE_MAX_CHAINS];     /* per pair                           */
  uint64_t round_trips[BDL_EXCHANGE_MAX_CHAINS]; /* per initial replica                */
  uint64_t refused;                              /* attempts with a non-finite U / la  */
  int32_t partner[BDL_EXCHANGE_MAX_CHAINS];      /* per slot: the last decision        */
  int32_t replica[BDL_EXCHANGE_MAX_CHAINS];      /* per slot: the replica it holds     */
  int32_t direction[BDL_EXCHANGE_MAX_CHAINS];    /* per replica: 0, UP or DOWN         */
} bdl_exchange_state;

typedef struct bdl_exchange_energy_args {
  const float* theta;    /* stacked, 16-B aligned                                    */
  const float* prior;    /* stacked, 16-B aligned, or null (theta0 = 0)              */
  void* workspace;       /* bdl_exchange_workspace_bytes(chains, n) bytes, 8-B aligned */
  int64_t n;             /* real elements per chain, 1 .. 4 * chain_groups           */
  uint64_t chain_groups; /* float4 groups per chain slot                             */
  int32_t chains;        /* 1 .. BDL_EXCHANGE_MAX_CHAINS                             */
  int32_t grid_blocks;   /* 1 .. BDL_EXCHANGE_MAX_GRID (0: up to eight per CU)       */
} bdl_exchange_energy_args;

typedef struct bdl_exchange_decide_args {
  bdl_exchange_state* state;
  const void* workspace; /* the partials bdl_exchange_energy wrote for (chains, n)   */
  const float* loss;     /* DEVICE fp32 [chains]: the mean losses (unread with
                            BDL_EXCHANGE_ENERGY_ONLY, then it may be null)           */
  const double* beta;    /* DEVICE fp64 [chains]: 1 / T_k (likewise)                 */
  int64_t n;             /* as the energy call's                                     */
  double n_data;         /* N                                                        */
  double sigma2;         /* > 0                                                      */
  double var;            /* >= 0: the correction for noisy energies (0: Metropolis)  */
  uint64_t seed;
  uint64_t chain0;
  uint64_t attempt;      /* t, < 2^62                                                */
  int32_t chains;
  int32_t flags;         /* BDL_EXCHANGE_FIRST | BDL_EXCHANGE_ENERGY_ONLY            */
} bdl_exchange_decide_args;

typedef struct bdl_exchange_swap_args {
  const bdl_exchange_state* state;
  float* vectors[BDL_EXCHANGE_MAX_VECTORS]; /* stacked, 16-B aligned, disjoint       */
  uint64_t chain_groups;
  int32_t nvectors;      /* 1 .. BDL_EXCHANGE_MAX_VECTORS                            */
  int32_t chains;
  int32_t grid_blocks;   /* workgroups per chain, 1 .. BDL_EXCHANGE_MAX_GRID (0: the
                            library's choice)                                        */
  int32_t pad;
} bdl_exchange_swap_args;

/* 8 * chains * ceil(n / 1024) bytes; 0 if an argument is out of range. */
int64_t bdl_exchange_workspace_bytes(int32_t chains, int64_t n);

/* One launch each on hip_stream.  Validation comes before any HIP call:
 * BDL_ERR_NULL (args or a required pointer), BDL_ERR_ALIGN (a stacked vector not
 * 16-B aligned; state, workspace or beta not 8-B aligned; loss not 4-B
 * aligned), BDL_ERR_ARG (chains, n, chain_groups, nvectors, grid_blocks, sigma2,
 * var or attempt out of range; an unknown flag; overlapping vectors of a swap; a
 * graph redirect active on the thread). */
int bdl_exchange_energy(const bdl_exchange_energy_args* args, void* hip_stream);
int bdl_exchange_decide(const bdl_exchange_decide_args* args, void* hip_stream);
int bdl_exchange_swap(const bdl_exchange_swap_args* args, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_EXCHANGE_H */
