"""Per-chain, per-tensor health of stacked chains: the host side.

`kernels.chain_stats` (include/bdl_stats.h) accumulates, per (chain k, tensor
t) and over the steps it was launched at, the sums

    G2 = sum g*g   V2 = sum v*v   D2 = sum d*d   DG = sum d*g   VG = sum v*g
    V2L = sum over steps of V2 / lr        (d = theta - prior mean)

between the backward pass and the update, i.e. with the gradient, theta and
the momentum all taken at the same theta.  This module turns a host copy of
that [K, T, 6] accumulator into what a user reads: root-mean-square tables for
every sampler and, for cSGHMC, the kinetic and configurational temperatures of
Wenzel et al. 2020 ("How good is the Bayes posterior in deep neural networks
really?", §4 diagnostics).  float64 NumPy throughout, no device.

Temperatures (cSGHMC: v <- (1-alpha) v - lr (g + prior_sig theta) + noise,
theta += v, noise std nd*sqrt(2*alpha*lr)/N per element, N = ND*Ninflate), in
units of the temperature that noise scale stands for if injected every step:

    t_kin [k,t] = (1 - alpha_k/2) * V2L[k,t] * N_k^2 / (d_t * nd_k^2 * steps)
    t_conf[k,t] = (DG[k,t] + prior_sig_k * D2[k,t]) * N_k^2 / (d_t * nd_k^2 * steps)

Both are 1 for a stationary chain on a quadratic in the small-step limit: the
target is exp(-U * N^2 / nd^2) with grad U = g + prior_sig theta, so the virial
<theta, grad U> is d * nd^2 / N^2 at temperature 1, and the momentum
v <- (1-alpha) v + noise is an AR(1) process of variance
noise^2 / (alpha (2 - alpha)) = lr * nd^2 / (N^2 (1 - alpha/2)) per element:
the factor 1 - alpha/2 is exact, not a small-alpha approximation.  nd = 0 (no
noise: no temperature to compare with) gives NaN.

The reference injects noise only on the thinned sample steps of a cycle
(methods/csghmc.py, quirks Q1 / Q4), so values well below 1 are expected with
thin > 1 and during exploration.  The numbers compare chains and layers of one
run; they are not a pass / fail.
"""
from __future__ import annotations

import numpy as np

SUMS = ("G2", "V2", "D2", "DG", "VG", "V2L")


def rms_table(acc, steps, numel):
    """{grad_rms, mom_rms, dist_rms, grad_mom_cos}: [K, T] float64 arrays from
    the accumulator acc [K, T, 6], the number of accumulated steps and the
    tensors' numel [T].  0 steps (or a zero norm under the cosine) gives NaN."""
    acc = np.asarray(acc, dtype=np.float64)
    d = np.asarray(numel, dtype=np.float64)[None, :]
    G2, V2, D2, VG = acc[..., 0], acc[..., 1], acc[..., 2], acc[..., 4]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = float(steps) * d
        return {"grad_rms": np.sqrt(G2 / den), "mom_rms": np.sqrt(V2 / den),
                "dist_rms": np.sqrt(D2 / den), "grad_mom_cos": VG / np.sqrt(G2 * V2)}


def temperatures(acc, steps, numel, *, alpha, nd, N, prior_sig):
    """{t_kin, t_conf: [K, T]; t_kin_chain, t_conf_chain: [K]} of cSGHMC chains
    (the module docstring's definitions).  alpha (momentum_decay), nd, N
    (= ND * Ninflate) and prior_sig: scalars or [K] arrays, chain k's values.
    The per-chain aggregates are the sums over tensors divided by the sum of
    the tensors' numel."""
    acc = np.asarray(acc, dtype=np.float64)
    K = acc.shape[0]
    d = np.asarray(numel, dtype=np.float64)
    col = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (K,))  # noqa: E731
    alpha, nd, N, prior_sig = col(alpha), col(nd), col(N), col(prior_sig)
    D2, DG, V2L = acc[..., 2], acc[..., 3], acc[..., 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        # nd == 0: x / 0 would be inf (or NaN for 0 / 0); the definition says NaN
        unit = np.where(nd != 0, N * N / (nd * nd * float(steps)), np.nan)
        kin = (1.0 - alpha / 2.0)[:, None] * V2L
        conf = DG + prior_sig[:, None] * D2
        return {"t_kin": kin * unit[:, None] / d[None, :],
                "t_conf": conf * unit[:, None] / d[None, :],
                "t_kin_chain": kin.sum(1) * unit / d.sum(),
                "t_conf_chain": conf.sum(1) * unit / d.sum()}
