"""Host reference of the cross-chain diagnostic — TEST INFRASTRUCTURE ONLY.

`chain_diag_f32` restates include/bdl_diag.h's arithmetic in plain NumPy on
np.float32 arrays, one separately rounded operation per line, k ascending from
0 (np.sqrt and / on float32 are correctly rounded): the device's outputs are
compared with it bit for bit.  `chain_diag_f64` is the textbook two-pass
Gelman-Rubin R-hat and the moment-matched pooled Gaussian in float64, the
yardstick of the fp32 formulation's own error.  Nothing is imported from
bayesdll_amd and nothing from torch.

Layout: mom1 / mom2 are the stacked vectors, chain k's element j at
slot * k + j with slot = 4 * chain_groups; only elements [0, n) of a chain are
read.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
VAR_GIVEN, VAR_RAW_MOMENTS, VAR_WELFORD = 0, 1, 2
THRESHOLDS = (1.01, 1.05, 1.1)


def f32(x):
    """The host's float64 scalar as a C float field receives it."""
    return F(float(x))


def c1_of(count):
    """fl32((count - 1) / count), the quotient formed in float64."""
    return f32((int(count) - 1) / int(count))


def inv_of(ratio):
    """fl32(1 / ratio64): the reciprocal the device multiplies Welford's M2 by."""
    return f32(1.0 / float(ratio))


def variance_f32(m, q, var_mode, ratio, inv_ratio, var_floor):
    """The variance the posterior draw takes the square root of (fp32)."""
    ratio, inv_ratio, var_floor = F(ratio), F(inv_ratio), F(var_floor)
    if var_mode == VAR_RAW_MOMENTS:
        t = m * m
        u = q - t
        var = ratio * u
    elif var_mode == VAR_WELFORD:
        var = q * inv_ratio if inv_ratio != 0 else q / ratio
    else:
        var = q.copy()
    # clamp at the floor; NaN stays NaN
    return np.where(np.isnan(var), var, np.where(var > var_floor, var, var_floor)).astype(F)


def _chain(v, k, slot, n):
    return np.asarray(v, dtype=F)[slot * k: slot * k + n]


def chain_diag_f32(mom1, mom2, *, chains, chain_groups, n, var_mode, ratio=1.0, inv_ratio=0.0,
                   var_floor=1e-12, count=2, thresholds=THRESHOLDS):
    """pooled_mean, pooled_var, rhat (fp32 arrays of n) and the summary dict,
    op for op as the device computes them."""
    K, slot = int(chains), 4 * int(chain_groups)
    fk, fkm1 = F(K), F(K - 1)
    c1 = c1_of(count)
    with np.errstate(all="ignore"):
        m0 = _chain(mom1, 0, slot, n)
        S1 = np.zeros(n, F)
        S2 = np.zeros(n, F)
        SW = np.zeros(n, F)
        for k in range(K):
            m = _chain(mom1, k, slot, n)
            v = variance_f32(m, _chain(mom2, k, slot, n), var_mode, ratio, inv_ratio, var_floor)
            d = m - m0
            S1 = S1 + d
            t = d * d
            S2 = S2 + t
            SW = SW + v
        q = S1 / fk
        mbar = m0 + q
        p = S1 * S1
        r = p / fk
        u = S2 - r
        ss = np.where(u < 0, F(0), u).astype(F)
        Bn = ss / fkm1
        W = SW / fk
        a = W * c1
        b = a + Bn
        c = b / W
        rhat = np.sqrt(c)
        e = ss / fk
        pvar = W + e
        degenerate = S2 == 0
        rhat = np.where(degenerate, F(np.nan), rhat).astype(F)
        nonfinite = ~degenerate & ~np.isfinite(rhat)
        ev = ~degenerate & np.isfinite(rhat)
        vals = rhat[ev]
        thr = [f32(t) for t in thresholds]
        summary = {
            "n_eval": int(ev.sum()), "n_degenerate": int(degenerate.sum()),
            "n_nonfinite": int(nonfinite.sum()),
            "n_above": [int((vals > t).sum()) for t in thr],
            "rhat_sum": math.fsum(float(x) for x in vals),
            "rhat_max": float(vals.max()) if vals.size else 0.0,
            "argmax": int(np.flatnonzero(ev & (rhat == vals.max()))[0]) if vals.size else -1,
        }
    assert mbar.dtype == F and pvar.dtype == F and rhat.dtype == F
    return mbar, pvar, rhat, summary


def chain_diag_f64(mom1, mom2, *, chains, chain_groups, n, var_mode, ratio=1.0, var_floor=1e-12,
                   count=2):
    """Textbook float64: two-pass between-chain variance, R-hat =
    sqrt(((count-1)/count * W + B/count) / W) with B/count the sample variance
    of the chain means, pooled mean / variance of the K-Gaussian mixture."""
    K, slot = int(chains), 4 * int(chain_groups)
    m = np.stack([_chain(mom1, k, slot, n) for k in range(K)]).astype(np.float64)
    q = np.stack([_chain(mom2, k, slot, n) for k in range(K)]).astype(np.float64)
    if var_mode == VAR_RAW_MOMENTS:
        v = float(ratio) * (q - m * m)
    elif var_mode == VAR_WELFORD:
        v = q / float(ratio)
    else:
        v = q
    v = np.maximum(v, float(var_floor))
    mbar = m.mean(0)
    ss = ((m - mbar) ** 2).sum(0)
    W = v.mean(0)
    rhat = np.sqrt((W * ((count - 1) / count) + ss / (K - 1)) / W)
    return mbar, W + ss / K, rhat


def make_case(seed, K, n, *, chain_groups=None, spread=0.05, pad=np.nan):
    """Stacked (mean, variance) of K chains: a common base per element
    (+-U(0.5, 2): a weight the chains agree on to within the spread) plus a
    N(0, spread^2) difference between chains, variances of the spread's order
    (VAR_GIVEN input); the padding of every chain slot is filled with `pad`."""
    rng = np.random.default_rng(seed)
    cg = (n + 3) // 4 if chain_groups is None else int(chain_groups)
    slot = 4 * cg
    base = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    m1 = np.full(K * slot, pad, F)
    m2 = np.full(K * slot, pad, F)
    for k in range(K):
        m1[slot * k: slot * k + n] = base + (spread * rng.standard_normal(n)).astype(F)
        m2[slot * k: slot * k + n] = (spread ** 2 * rng.uniform(0.5, 2.0, n)).astype(F)
    return m1, m2, cg


def to_mode(m1, var, var_mode, ratio, K, slot, n):
    """mom2 for `var_mode` whose variance is (about) `var`: the raw second
    moment var / ratio + m1^2, or Welford's M2 = var * ratio."""
    m2 = var.copy()
    for k in range(K):
        s = slice(slot * k, slot * k + n)
        if var_mode == VAR_RAW_MOMENTS:
            m2[s] = var[s] / F(ratio) + m1[s] * m1[s]
        elif var_mode == VAR_WELFORD:
            m2[s] = var[s] * F(ratio)
    return m2
