"""NumPy restatement of bdl_chain_clip (include/bdl_clip.h) — TEST
INFRASTRUCTURE ONLY.  Nothing here imports bayesdll_amd or torch.

Per chain k, over the elements of that chain's segment slices:

    s_k    = sum of (double)g * (double)g                  (float64)
    norm_k = fl32(sqrt(s_k))
    coef_k = min( fl32( fl32(1 / fl32(norm_k + 1e-6f)) * max_norm ), 1 )
    g     <- fl32(g * coef_k)   if coef_k < 1, else untouched

The device accumulates s_k with fp64 fmas in its launch geometry's order; here
it is a float64 dot product per slice, added slice by slice.  The two orders
differ by fp64 rounding only (norm_k within one fp32 ulp), and not at all when
every product and partial sum is an integer below 2^53.  The coefficient is
tests/step_ref.py::clip_coef — the chain of fp32 roundings of the existing
clipped SGLD step."""
from __future__ import annotations

import numpy as np

from step_ref import F, clip_coef


def chain_norm(slices):
    """fl32(sqrt(float64 sum of squares)) over one chain's slices (fp32 arrays)."""
    s = np.float64(0.0)
    for g in slices:
        assert g.dtype == np.float32, g.dtype
        g64 = g.astype(np.float64)
        s += np.dot(g64, g64)
    return F(np.sqrt(s))


def scale(g, coef):
    """fl32(g * coef): one fp32 product per element; coef >= 1 leaves g as it is."""
    coef = F(coef)
    return g if not coef < F(1.0) else (g * coef).astype(np.float32)


def chain_clip(chains, max_norm):
    """chains: per chain, the list of its slices.  Returns (norms [K] fp32,
    coefs [K] fp32, the scaled slices in the same nesting)."""
    norms = np.array([chain_norm(sl) for sl in chains], dtype=np.float32)
    coefs = np.array([clip_coef(n, max_norm) for n in norms], dtype=np.float32)
    return norms, coefs, [[scale(g, c) for g in sl] for sl, c in zip(chains, coefs)]


def within_one_ulp(a, b):
    """|a - b| <= one fp32 ulp of b (both fp32 values)."""
    a, b = F(a), F(b)
    return bool(abs(np.float64(a) - np.float64(b)) <= np.float64(np.spacing(np.abs(b))))
