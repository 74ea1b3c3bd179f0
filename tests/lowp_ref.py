"""bf16 helpers and the host reference of the bf16-gradient step — TEST
INFRASTRUCTURE ONLY (include/bdl_lowp.h states the contract).

bf16 values travel as uint16 bit patterns.  The encode is the header's integer
formula, the decode a 16-bit shift; the step reference upcasts the gradient,
calls tests/step_ref.py (the op-by-op fp32 restatement the fp32 kernels are
anchored to) and encodes the shadow of every element that is not skipped.
Nothing is imported from bayesdll_amd and nothing from torch.
"""
from __future__ import annotations

import numpy as np

import step_ref as SR

F = np.float32


def bf16_encode(x):
    """fp32 -> bf16 bits, round to nearest, ties to even:
    (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the fp32 bits; a NaN gives a quiet
    NaN of its sign (the sum would carry into the sign bit)."""
    x = np.ascontiguousarray(x, dtype=F)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = ((u >> 16) | 0x40).astype(np.uint16)
    return np.where(np.isnan(x), nan, r).astype(np.uint16)


def bf16_decode(h):
    """bf16 bits -> fp32 (exact)."""
    h = np.ascontiguousarray(h, dtype=np.uint16)
    return (h.astype(np.uint32) << 16).view(F)


def bf16_is_nan(h):
    h = np.asarray(h, dtype=np.uint16)
    return ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)


def round_to_bf16(x):
    """fp32 values rounded to the nearest bf16, as fp32."""
    return bf16_decode(bf16_encode(x))


def step(method, th, g16, v, th0, attr, sc, eps, mode, *, momentum=None, collect=SR.NONE,
         m1=None, m2=None, shadow=None):
    """One bdl_lowp_step on the host.  method: "csghmc" | "sghmc" | "sgld";
    g16: the bf16 gradient bits; eps: the noise (None: no noise term; cSGHMC
    only); momentum: SGLD's None | "first" | "later".  Returns (theta, v, m1,
    m2, shadow): shadow is `shadow` with every element that is not skipped
    replaced by bf16(theta_new)."""
    g = bf16_decode(g16)
    if method == "csghmc":
        nth, nv = SR.csghmc(th, g, v, attr, sc, eps)
    elif method == "sghmc":
        nth, nv = SR.sghmc(th, th0, g, v, attr, sc, eps, mode)
    elif method == "sgld":
        nth, nv = SR.sgld(th, th0, g, v, attr, sc, eps, mode, momentum=momentum)
    else:
        raise ValueError(method)
    n1, n2 = SR.collect(collect, nth, m1, m2, sc, mode)
    sh = bf16_encode(nth)
    if shadow is not None:
        sh = np.where((attr & SR.ATTR_SKIP) != 0, np.asarray(shadow, dtype=np.uint16), sh)
    return nth, nv, n1, n2, sh


def rounding_inputs():
    """The fp32 values the rounding tests use: ties both ways, one fp32 ulp
    either side of a tie, +-0, +-inf, the fp32 maximum, subnormals (fp32
    subnormals that round to bf16 subnormals, to zero and up to the smallest
    normal), and 4096 random bit patterns with the NaNs removed."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0xC2F6, 0x0001, 0x0080, 0x7F7E, 0x8000, 0x0000):
        for lo in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF):
            bits.append((hi << 16) | lo)
    bits += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,
             0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF,
             0x807FFFFF, 0x007F8000, 0x00800000]
    rng = np.random.default_rng(20240)
    rnd = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([np.asarray(bits, dtype=np.uint32), rnd]).view(F)
    return x[~np.isnan(x)].copy()
