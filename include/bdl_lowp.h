/* bdl_lowp.h — the fused SG-MCMC step for a network that computes in bf16.
 *
 * "Master weights" mixed precision.  The chain keeps its state in fp32 and
 * updates it in fp32 (theta, momentum, prior mean, posterior moments, the
 * Philox stream: the very update_core / collect_core of bdl_sgmcmc_step).  The
 * network computes in bf16: its parameters are views into a bf16 SHADOW of
 * theta and autograd leaves bf16 gradients.  bdl_lowp_step reads those bf16
 * gradients where they are and writes the new shadow in the sweep that writes
 * theta, so a step moves the bytes of the fp32 step (theta r+w 8, momentum
 * r+w 8, gradient r 2, shadow w 2 per element against gradient r 4) and the
 * forward pays no cast kernels.  Purely additive to the ABI of bdl_sgmcmc.h
 * (same status codes, bdl_last_error, stream convention).
 *
 * Contract (tests/test_gpu_lowp.py asserts it bit for bit)
 *   g = fp32(bf16 gradient)                                   (exact)
 *   theta, mom, mom1, mom2, *nonfinite: exactly what bdl_sgmcmc_step writes
 *     on the same inputs with that g as its fp32 gradient — the same (seed,
 *     chain, step, group) Philox stream, the same roundings, the same head /
 *     no-prior semantics, and for BDL_ATTR_SKIP elements the same values
 *     (theta unchanged; the collect sees the unchanged theta; a first
 *     SGD-momentum step leaves 0 in the buffer).
 *   shadow[j] = bf16(theta_new[j]), round to nearest, ties to even: on the fp32
 *     bits u, (u + 0x7FFF + ((u >> 16) & 1)) >> 16.  The fp32 maximum rounds to
 *     inf, subnormals are kept, a NaN gives a NaN: theta.to(torch.bfloat16) for
 *     every value that is not a NaN.  One instruction on gfx950
 *     (v_cvt_pk_bf16_f32, through the compiler's __bf16 conversion).
 *   shadow of a BDL_ATTR_SKIP element is not written (it has no gradient and
 *     its theta does not move; bdl_lowp_shadow wrote it), and the gradient of
 *     such an element is never read: the padding of a stacked slot keeps
 *     whatever it holds in both.
 *   Results never depend on `blocks` or `unroll`.
 *   Known limit: *nonfinite looks at the fp32 theta only (it is the fp32
 *     step's flag), so a finite theta above the largest finite bf16 gives an
 *     infinite shadow element without raising it.
 *
 * Sweep: grid-stride, 256-lane workgroups, the run table (and the gradient
 * bases) staged in LDS.  A lane takes `unroll` float4 groups per iteration,
 * finds each group's run in LDS, issues every load of the iteration (16-B
 * non-temporal for the fp32 streams, one 8-B load for a group's four
 * gradients) before any arithmetic, draws its Philox noise in registers, and
 * stores 16 B per fp32 stream and 8 B of shadow.  A group that crosses a run
 * boundary or touches a SKIP run, a run whose gradient base is not 8-B
 * addressable, and the tail n % 4 read the gradient and write the shadow
 * element by element.
 */
#ifndef BDL_LOWP_H
#define BDL_LOWP_H

#include <stdint.h>

#include "bdl_sgmcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BDL_LOWP_MAX_BLOCKS 65536 /* blocks <= this */

/* The fields bdl_step_args has for BDL_CSGHMC / BDL_SGHMC / BDL_SGLD, with the
 * same meaning and the same host-side rounding, plus shadow, blocks, unroll;
 * grad is bf16. */
typedef struct bdl_lowp_args {
  float* theta;             /* in/out, fp32 master, 16-B aligned                     */
  const uint16_t* grad;     /* bf16, n elements, 8-B aligned; or null with grad_base */
  float* mom;               /* csghmc/sghmc momentum v, or the SGD momentum buffer   */
  const float* prior_mean;  /* theta0 (sghmc/sgld)                                   */
  const float* noise;       /* BDL_NOISE_BUFFER only, fp32                           */
  float* mom1;              /* collect only                                          */
  float* mom2;              /* collect only; may be null                             */
  uint16_t* shadow;         /* out, bf16, n elements, 8-B aligned                    */
  const bdl_run* runs;      /* device run table                                      */
  /* Gradient per run, where autograd left it (null: `grad`).  Device array of
   * nruns byte addresses: run t's gradient for flat element i is
   * ((uint16_t*)grad_base[t])[i], i.e. grad_base[t] = &g_t[0] - 2 * offset_t
   * bytes.  Runs must not span two tensors; SKIP runs may hold 0.  A run whose
   * base is not 8-B addressable (or that carries BDL_ATTR_GUNALIGNED) is read
   * element by element. */
  const int64_t* grad_base;
  int32_t* nonfinite;       /* as bdl_step_args.nonfinite (nullable)                 */
  int64_t n;
  int32_t nruns;
  int32_t method;           /* BDL_CSGHMC, BDL_SGHMC or BDL_SGLD                     */
  int32_t noise_mode;       /* bdl_noise_mode                                        */
  int32_t collect;          /* bdl_collect                                           */
  int32_t flags;            /* BDL_FLAG_FIRST_STEP | RECIP_DIV | MOMENTUM            */
  int32_t blocks;           /* 0: about two workgroups per CU; else exactly this many */
  int32_t unroll;           /* float4 groups per lane and iteration: 1, 2 or 4       */
  int32_t pad0;
  float lr[2];
  float noise_scale[2];
  float one_minus_alpha, prior_sig, sigma2, n_data, mu, collect_a, collect_b;
  float inv_sigma2, inv_n_data, inv_collect_a, inv_collect_b; /* 0: 1/fl32(s) */
  float pad1;
  uint64_t seed, chain, step;
  uint64_t philox_offset;   /* as bdl_step_args.philox_offset                        */
  uint64_t chain_groups;    /* as bdl_step_args.chain_groups (0: one chain)          */
} bdl_lowp_args;

/* One launch on hip_stream; no host synchronisation, no allocation.  Every
 * check comes before the first HIP call:
 *   BDL_ERR_NULL   args, theta, shadow, runs (or nruns < 1); grad and
 *                  grad_base both null; mom where the method needs it (cSGHMC,
 *                  SGHMC, SGLD with BDL_FLAG_MOMENTUM); prior_mean for SGHMC /
 *                  SGLD; noise with BDL_NOISE_BUFFER; mom1 with a collect
 *   BDL_ERR_ALIGN  theta, mom, prior_mean, noise, mom1, mom2 not 16-B aligned;
 *                  shadow, grad or the grad_base table not 8-B aligned
 *   BDL_ERR_RUNS   the run table (24 B per run with grad_base, else 16)
 *                  exceeds 64 KiB of LDS
 *   BDL_ERR_ARG    a graph redirect active on the thread; n <= 0; a method
 *                  other than the three (the *_GRAD and Adam methods are out of
 *                  scope); BDL_FLAG_GRAD_READY or an unknown flag bit (there is
 *                  no clipped form); unknown noise mode or collect kind; a
 *                  combination without a kernel (built: cSGHMC with any noise
 *                  mode and NONE / WELFORD_INIT / WELFORD; SGHMC and SGLD with
 *                  BUFFER or PHILOX noise and NONE / MEAN_INIT / MEAN — what
 *                  the samplers launch); unroll
 *                  not 1, 2 or 4; blocks < 0 or > BDL_LOWP_MAX_BLOCKS;
 *                  chain_groups or the float4 group indices (n / 4 +
 *                  philox_offset) reaching 2^32 with stacked chains or Philox
 *                  noise; a Philox chain id (plus the stacked chains) reaching
 *                  2^32 */
int bdl_lowp_step(const bdl_lowp_args* args, void* hip_stream);

/* shadow[j] = bf16(theta[j]) for every j in [0, n): the one implementation of
 * the rounding above, for a theta written outside the step (a checkpoint load,
 * a cycle restore).  Every element is written whatever its run's attributes —
 * the shadow of a frozen tensor must equal its theta — so the run table is
 * not read: runs may be null (nruns 0).  BDL_ERR_NULL (theta, shadow),
 * BDL_ERR_ALIGN (theta not 16-B, shadow not 8-B aligned), BDL_ERR_ARG (n <= 0,
 * nruns < 0, a graph redirect active on the thread). */
int bdl_lowp_shadow(const float* theta, uint16_t* shadow, const bdl_run* runs, int32_t nruns,
                    int64_t n, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BDL_LOWP_H */
