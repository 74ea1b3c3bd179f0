"""Host reference of the batch-means effective sample size — TEST INFRASTRUCTURE ONLY.

`fold_f32` and `chain_ess_f32` restate include/bdl_ess.h's two arithmetic
blocks in plain NumPy on np.float32 arrays, one separately rounded operation
per line, chains ascending from 0 (np.sqrt and / on float32 are correctly
rounded): the device's accumulators and outputs are compared with them bit for
bit.  `fold_plan` restates the flag and scalar bookkeeping.  `batch_means_f64`
is the textbook estimate in float64 (two-pass means and variances over stored
samples) and `ar1_ess` the exact finite-b value for an AR(1) series, the
yardsticks of the fp32 formulation and of the estimator.  Nothing is imported
from bayesdll_amd and nothing from torch.

Layout: every vector is stacked, chain k's element j at slot * k + j with
slot = 4 * chain_groups; only elements [0, n) of a chain are touched.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
FIRST_SAMPLE, FIRST_IN_BATCH, CLOSE, FIRST_BATCH = 1, 2, 4, 8
THRESHOLDS = (100.0, 400.0, 1000.0)
VECTORS = ("bsum", "smean", "sM2", "bM2")


def f32(x):
    """The host's float64 scalar as a C float field receives it."""
    return F(float(x))


def fold_plan(s, b):
    """(flags, fl32(s), fl32(b), fl32(i/(i-1))) of folding the s-th sample
    (1-based) with batches of b; the last is None where no fold uses it."""
    p = (s - 1) % b + 1
    flags = 0
    if s == 1:
        flags |= FIRST_SAMPLE
    if p == 1:
        flags |= FIRST_IN_BATCH
    if p == b:
        flags |= CLOSE
        if s == b:
            flags |= FIRST_BATCH
    c = None
    if flags & CLOSE and not flags & FIRST_BATCH:
        i = s // b
        c = f32(i / (i - 1))
    return flags, f32(s), f32(b), c


def new_acc(size, fill=np.nan):
    """The four accumulators, every lane pre-filled with `fill`."""
    return {nm: np.full(size, fill, F) for nm in VECTORS}


def fold_f32(acc, theta, s, b, *, chains, chain_groups, n):
    """Fold sample s (1-based) of every chain into `acc` in place, op for op
    as the device does; a vector the fold does not need is not touched, nor is
    any lane outside [0, n) of a chain slot.  Returns the flags."""
    flags, fs, fb, c = fold_plan(s, b)
    slot = 4 * int(chain_groups)
    theta = np.asarray(theta, dtype=F)
    with np.errstate(all="ignore"):
        for k in range(int(chains)):
            sl = slice(slot * k, slot * k + n)
            x = theta[sl]
            if flags & FIRST_SAMPLE:
                smean = x.copy()
                sM2 = np.zeros(n, F)
            else:
                d = x - acc["smean"][sl]
                q = d / fs
                smean = acc["smean"][sl] + q
                d2 = x - smean
                t = d * d2
                sM2 = acc["sM2"][sl] + t
            acc["smean"][sl] = smean
            acc["sM2"][sl] = sM2
            if flags & FIRST_IN_BATCH:
                bs = x.copy()
            else:
                bs = acc["bsum"][sl] + x
            if not flags & CLOSE:
                acc["bsum"][sl] = bs
            else:
                y = bs / fb
                if flags & FIRST_BATCH:
                    bM2 = np.zeros(n, F)
                else:
                    e = y - smean
                    t = e * e
                    u = t * c
                    bM2 = acc["bM2"][sl] + u
                acc["bM2"][sl] = bM2
    assert all(v.dtype == F for v in acc.values())
    return flags


def chain_ess_f32(sM2, bM2, *, chains, chain_groups, n, samples, batches, thresholds=THRESHOLDS):
    """ess, mcse (fp32 arrays of n) and the summary dict, op for op as the
    device computes them; the summary in a fixed order (math.fsum for the
    sum: the exactly rounded value the device's fp64 sum is held against)."""
    K, slot = int(chains), 4 * int(chain_groups)
    fS1, fnb1, fKnb = F(samples - 1), F(batches - 1), F(K * batches)
    sM2, bM2 = np.asarray(sM2, dtype=F), np.asarray(bM2, dtype=F)
    with np.errstate(all="ignore"):
        SW = np.zeros(n, F)
        SV = np.zeros(n, F)
        for k in range(K):
            SW = SW + sM2[slot * k: slot * k + n]
            SV = SV + bM2[slot * k: slot * k + n]
        w = SW / fS1
        v = SV / fnb1
        r = w / v
        ess = r * fKnb
        g = v / fKnb
        mcse = np.sqrt(g)
        degenerate = SV == 0
        ess = np.where(degenerate, F(np.nan), ess).astype(F)
        nonfinite = ~degenerate & ~np.isfinite(ess)
        ev = ~degenerate & np.isfinite(ess)
        vals = ess[ev]
        thr = [f32(t) for t in thresholds]
        summary = {
            "n_eval": int(ev.sum()), "n_degenerate": int(degenerate.sum()),
            "n_nonfinite": int(nonfinite.sum()),
            "n_below": [int((vals < t).sum()) for t in thr],
            "ess_sum": math.fsum(float(x) for x in vals),
            "ess_min": float(vals.min()) if vals.size else 0.0,
            "argmin": int(np.flatnonzero(ev & (ess == vals.min()))[0]) if vals.size else -1,
        }
    assert ess.dtype == F and mcse.dtype == F
    return ess, mcse, summary


def fold_series(x, b, *, chain_groups=None, fill=0.0):
    """Fold a whole series x [S, K, n] (float32) and return (acc, chain_groups)."""
    S, K, n = x.shape
    cg = (n + 3) // 4 if chain_groups is None else int(chain_groups)
    slot = 4 * cg
    acc = new_acc(K * slot, fill)
    theta = np.zeros(K * slot, F)
    for s in range(S):
        for k in range(K):
            theta[slot * k: slot * k + n] = x[s, k]
        fold_f32(acc, theta, s + 1, b, chains=K, chain_groups=cg, n=n)
    return acc, cg


def batch_means_f64(x, b):
    """Textbook float64 batch means over stored samples x [S, K, n]: two-pass
    sample variance s_k^2 per chain, two-pass variance vb_k of the nb = S // b
    batch means (about the mean of the samples the batches cover), pooled as
    the device pools: ess = K nb mean_k(s_k^2) / mean_k(vb_k), mcse =
    sqrt(sum_k(vb_k) / (K nb)) = sqrt(mean_k(vb_k) / nb), the contract's g.
    S must be a multiple of b."""
    x = np.asarray(x, dtype=np.float64)
    S, K, n = x.shape
    nb = S // b
    assert nb * b == S and nb >= 2
    s2 = x.var(axis=0, ddof=1)                                  # [K, n]
    y = x.reshape(nb, b, K, n).mean(axis=1)                     # [nb, K, n]
    vb = y.var(axis=0, ddof=1)
    w, v = s2.mean(0), vb.mean(0)
    return K * nb * w / v, np.sqrt(v / nb)


def ar1_ess(rho, b, S, K):
    """The value the batch-means ESS estimates for a stationary AR(1) series
    at a finite batch length: K S sigma^2 / (b Var(ybar_b)), Var(ybar_b) =
    (sigma^2 / b) [1 + 2 sum_{k<b} (1 - k/b) rho^k]."""
    k = np.arange(1, b)
    tau_b = 1.0 + 2.0 * np.sum((1.0 - k / b) * float(rho) ** k)
    return K * S / tau_b


def ar1_series(seed, S, K, n, rho, *, loc=0.02, scale=1e-3):
    """x [S, K, n] float32 = loc + scale * z with z a unit-variance stationary
    AR(1) series per (chain, element)."""
    rng = np.random.default_rng(seed)
    z = np.empty((S, K, n))
    z[0] = rng.standard_normal((K, n))
    inn = math.sqrt(1.0 - rho * rho)
    for s in range(1, S):
        z[s] = rho * z[s - 1] + inn * rng.standard_normal((K, n))
    return (loc + scale * z).astype(F)
