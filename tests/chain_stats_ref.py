"""Restatement of bdl_chain_stats (include/bdl_stats.h) and of the health
formulas (bayesdll_amd/health.py) — TEST INFRASTRUCTURE ONLY.  Nothing here
imports bayesdll_amd or torch.

Per (chain, tensor), over the tensor's elements (fp32 arrays):

    d   = fl32(theta - prior_mean)            (theta when there is no prior mean)
    G2 = sum g*g   V2 = sum v*v   D2 = sum d*d   DG = sum d*g   VG = sum v*g
    V2L = V2 * (1.0 / (double)lr)

Every factor is an fp32 value held in float64, so every product is exact
(24 + 24 significand bits); `sums` adds them with math.fsum (the correctly
rounded sum: one rounding), `exact_sums` with Fractions (no rounding at all,
for small tensors).  The device adds the same exact terms with fp64 fmas in
its launch geometry's order: n terms, at most n - 1 roundings of partial sums
that never exceed sum|terms|, so

    |device - fsum| <= (n - 1) * 2^-53 * sum|terms| + the fsum's own 2^-53,

which `bound` states as 2 * n * 2^-53 * sum|terms| (V2L: its two extra
roundings, the reciprocal and the product, fit for n >= 3), and nothing at
all when every term and partial sum is an integer below 2^53.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

ORDER = ("G2", "V2", "D2", "DG", "VG", "V2L")


def _terms(g, theta, mom, prior):
    for a in (g, theta, mom, prior):
        assert a is None or a.dtype == np.float32, a.dtype
    d = theta if prior is None else (theta - prior).astype(np.float32)
    g64, d64 = g.astype(np.float64), d.astype(np.float64)
    v64 = np.zeros_like(g64) if mom is None else mom.astype(np.float64)
    return [g64 * g64, v64 * v64, d64 * d64, d64 * g64, v64 * g64]


def sums(g, theta, mom, prior, lr):
    """(six sums, six sums of |terms|) of one (chain, tensor) as float64 [6]."""
    t = _terms(g, theta, mom, prior)
    inv = 1.0 / float(np.float32(lr))
    s = [math.fsum(x) for x in t]
    a = [math.fsum(np.abs(x)) for x in t]
    return np.array(s + [s[1] * inv]), np.array(a + [a[1] * inv])


def exact_sums(g, theta, mom, prior, lr):
    """The six sums (and the sums of |terms|) as Fractions: no rounding."""
    t = _terms(g, theta, mom, prior)
    lrq = Fraction(float(np.float32(lr)))
    s = [sum((Fraction(float(v)) for v in x), Fraction(0)) for x in t]
    a = [sum((abs(Fraction(float(v))) for v in x), Fraction(0)) for x in t]
    return s + [s[1] / lrq], a + [a[1] / lrq]


def bound(n, abs_sums):
    """2 * n * 2^-53 * sum|terms| per entry (the module docstring)."""
    return 2.0 * n * 2.0 ** -53 * np.asarray(abs_sums, dtype=np.float64)


# --------------------------------------------------------------- formula layer
def rms_table(acc, steps, numel):
    acc = np.asarray(acc, dtype=np.float64)
    K, T = acc.shape[:2]
    out = {k: np.empty((K, T)) for k in ("grad_rms", "mom_rms", "dist_rms", "grad_mom_cos")}
    for k in range(K):
        for t in range(T):
            G2, V2, D2, _, VG, _ = (float(v) for v in acc[k, t])
            den = steps * float(numel[t])
            out["grad_rms"][k, t] = math.sqrt(G2 / den)
            out["mom_rms"][k, t] = math.sqrt(V2 / den)
            out["dist_rms"][k, t] = math.sqrt(D2 / den)
            out["grad_mom_cos"][k, t] = VG / math.sqrt(G2 * V2) if G2 * V2 > 0 else math.nan
    return out


def temperatures(acc, steps, numel, alpha, nd, N, prior_sig, ar1=True):
    """t_kin, t_conf [K, T] and their per-chain aggregates, entry by entry in
    Python floats; alpha, nd, N, prior_sig: one value per chain.  ar1=False
    drops the exact AR(1) factor 1 - alpha/2 (what a small-alpha derivation
    would leave out)."""
    acc = np.asarray(acc, dtype=np.float64)
    K, T = acc.shape[:2]
    kin, conf = np.empty((K, T)), np.empty((K, T))
    kc, cc = np.empty(K), np.empty(K)
    dsum = float(sum(numel))
    for k in range(K):
        a, s, n, ps = float(alpha[k]), float(nd[k]), float(N[k]), float(prior_sig[k])
        f = (1.0 - a / 2.0) if ar1 else 1.0
        unit = n * n / (s * s * steps) if s != 0 else math.nan
        for t in range(T):
            kin[k, t] = f * float(acc[k, t, 5]) * unit / float(numel[t])
            conf[k, t] = (float(acc[k, t, 3]) + ps * float(acc[k, t, 2])) * unit / float(numel[t])
        kc[k] = f * math.fsum(acc[k, :, 5]) * unit / dsum
        cc[k] = math.fsum(acc[k, :, 3] + ps * acc[k, :, 2]) * unit / dsum
    return {"t_kin": kin, "t_conf": conf, "t_kin_chain": kc, "t_conf_chain": cc}


def simulate_quadratic(d, burn, steps, *, lr, alpha, N, nd=1.0, prior_sig=1.0, curv=3.0, seed=0):
    """cSGHMC with noise every step on the target g = curv * theta (float64):
    v <- (1-alpha) v - lr (g + prior_sig theta) + nd sqrt(2 alpha lr)/N eps,
    theta += v; after `burn` steps, the six sums of `steps` steps taken BEFORE
    each update, as a [1, 1, 6] accumulator."""
    rng = np.random.default_rng(seed)
    th, v = np.zeros(d), np.zeros(d)
    sc = nd * math.sqrt(2 * alpha * lr) / N
    acc = np.zeros(6)
    for i in range(burn + steps):
        g = curv * th
        if i >= burn:
            V2 = float(v @ v)
            acc += [float(g @ g), V2, float(th @ th), float(th @ g), float(v @ g), V2 * (1.0 / lr)]
        v = (1 - alpha) * v - lr * (g + prior_sig * th) + sc * rng.standard_normal(d)
        th = th + v
    return acc.reshape(1, 1, 6)
