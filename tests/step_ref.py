"""Host reference of every fused update rule — TEST INFRASTRUCTURE ONLY.

Plain NumPy on np.float32 arrays, one separately rounded operation per line,
written from the upstream sampler's rules (paths relative to the upstream
repository):

  cSGHMC       methods/csghmc.py:759-778
  SGLD         methods/sgld.py:471-484 (== methods/csgld.py:665-680)
  SGHMC        methods/sghmc.py:494-510
  Adam-SGHMC   methods/adam_sghmc.py:512-553, methods/adam_csghmc.py:819-860
  SGD          torch.optim.SGD, single-tensor step (weight decay 0, dampening 0)
  clipping     torch.nn.utils.clip_grad_norm_ (grads.mul_(coef))
  collects     the Runners' Welford update (csghmc.py:333-345) and running
               means (sgld.py:239-246, csgld.py:280-293)

It works on the flat vectors with one attribute per element (ATTR_HEAD: the
readout's lr / noise-scale group; ATTR_PRIOR: the Gaussian-prior term applies;
ATTR_SKIP: no gradient — no update and no SGD step, but the collect still sees
the unchanged theta; a first SGD-momentum step leaves 0 in a skipped element's
buffer, the flat stand-in for torch.optim.SGD holding no buffer for such a
parameter: at its first gradient mu * 0 + g is clone(g)).  Nothing is imported
from bayesdll_amd and nothing from torch.

Rounding rules
  * scalars: every scalar is the host's float64 value rounded to fp32 once,
    as a C float field receives it (Scalars / AdamScalars form the derived
    ones — 1 - beta, 1 - beta**t, 2 * alpha, 1 - alpha, the reciprocals — in
    float64 first, as the host wrapper does);
  * a division by a scalar is x / s ("true": torch on a CPU) or x * inv with
    inv = fl32(1 / float64(s)) ("recip": torch on the device);
  * SGD's param.add_(d, alpha=-lr) is one fused multiply-add, emulated
    correctly rounded (fma32);
  * np.sqrt and / on float32 are correctly rounded.
"""
from __future__ import annotations

import numpy as np

F = np.float32
ATTR_HEAD, ATTR_PRIOR, ATTR_SKIP = 0x1, 0x2, 0x4
NONE, WELFORD_INIT, WELFORD, MEAN_INIT, MEAN = range(5)  # collect kinds


def f32(x):
    """The host's float64 scalar as a C float field receives it."""
    return F(float(x))


class Div:
    """A scalar divisor: s = fl32(s64) and the reciprocal the device multiplies
    by, fl32(1 / s64) from the float64 divisor (or a given one)."""

    def __init__(self, s64, inv=None):
        self.s = f32(s64)
        self.inv = f32(1.0 / float(s64)) if inv is None else F(inv)

    @classmethod
    def fallback(cls, s64):
        """The reciprocal formed in fp32 from the rounded divisor,
        fl32(1 / fl32(s)): what the library uses when the caller leaves the
        reciprocal field 0."""
        s = f32(s64)
        return cls(s64, F(1.0) / s)


def sdiv(x, d, mode):
    return x / d.s if mode == "true" else x * d.inv


class Scalars:
    """The scalars of one step launch (bdl_step_args), from the host's doubles."""

    def __init__(self, *, lrs, noise_scale=(0.0, 0.0), one_minus_alpha=1.0, prior_sig=0.0,
                 sigma2=1.0, n_data=1.0, mu=0.0, collect_a=1.0, collect_b=1.0):
        self.lr = (f32(lrs[0]), f32(lrs[1]))
        self.ns = (f32(noise_scale[0]), f32(noise_scale[1]))
        self.oma = f32(one_minus_alpha)
        self.prior_sig = f32(prior_sig)
        self.sigma2, self.n_data = Div(sigma2), Div(n_data)
        self.mu = f32(mu)
        self.ca, self.cb = Div(collect_a), Div(collect_b)


class AdamScalars:
    """The Adam-SGHMC scalars (bdl_adam_args): derived values formed in
    float64, then rounded once."""

    def __init__(self, *, beta1, beta2, eps, t, momentum_decay, nd, temperature=1.0):
        b1, b2, t = float(beta1), float(beta2), int(t)
        self.b1, self.omb1 = f32(b1), f32(1 - b1)
        self.b2, self.omb2 = f32(b2), f32(1 - b2)
        self.bc1, self.bc2 = Div(1 - b1 ** t), Div(1 - b2 ** t)
        self.eps = f32(eps)
        self.two_alpha = f32(2 * float(momentum_decay))
        self.oma = f32(1 - float(momentum_decay))
        self.nd = f32(nd)
        self.temp = Div(temperature)


def element_attrs(numels, attrs):
    """Per-element attribute vector of a segment table."""
    return np.repeat(np.asarray(attrs, dtype=np.uint8), np.asarray(numels, dtype=np.int64))


def _a32(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x


def _group(attr, pair):
    return np.where((attr & ATTR_HEAD) != 0, pair[1], pair[0]).astype(F)


def _keep(attr, new, old):
    """new where the element is updated, old where it is skipped."""
    return np.where((attr & ATTR_SKIP) != 0, old, new).astype(F)


# ------------------------------------------------------------------------ fma
def fma32(a, b, c):
    """fl32(a * b + c) with one rounding, for float32 inputs.  The product of
    two fp32 values is exact in float64; the float64 sum is taken with its
    TwoSum error term, and where that sum sits exactly on an fp32 rounding
    midpoint while the exact value does not, the error term's sign decides
    the neighbour (the plain cast would round the midpoint to even: a double
    rounding)."""
    a, b, c = (_a32(x).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bv = s - p
        err = (p - (s - bv)) + (c - bv)
        r = s.astype(F)
        d = s - r.astype(np.float64)
        other = np.nextafter(r, np.where(d > 0, F(np.inf), F(-np.inf)).astype(F))
        mid = (r.astype(np.float64) + other.astype(np.float64)) * 0.5
        tie = (d != 0) & np.isfinite(mid) & (s == mid) & (err != 0)
        fix = np.where(err > 0, np.maximum(r, other), np.minimum(r, other))
    return np.where(tie, fix, r).astype(F)


# ------------------------------------------------------------------- SGD step
def sgd_step(th, d_p, buf, attr, sc, momentum=None):
    """torch.optim.SGD: momentum None (no buffer), "first" (buf = clone(d_p))
    or "later" (buf = mu * buf + d_p); param.add_(d, alpha=-lr).
    Returns (theta, buf)."""
    th, d_p = _a32(th), _a32(d_p)
    eta = _group(attr, sc.lr)
    stepv, nbuf = d_p, buf
    with np.errstate(all="ignore"):
        if momentum == "first":
            nbuf = d_p.copy()
        elif momentum == "later":
            t = sc.mu * _a32(buf)
            nbuf = t + d_p
        else:
            assert momentum is None, momentum
        if momentum is not None:
            stepv = nbuf
            # a skipped element: no buffer yet on a first step (0), else as it was
            nbuf = _keep(attr, nbuf, np.zeros_like(th) if momentum == "first" else buf)
        nth = fma32(-eta, stepv, th)
    return _keep(attr, nth, th), nbuf


# --------------------------------------------------------------------- cSGHMC
def csghmc(th, g, v, attr, sc, eps=None):
    """methods/csghmc.py:759-778 (both bias branches: grad + prior_sig * theta).
    eps None: an exploration step (no noise).  Returns (theta, v)."""
    th, g, v = _a32(th), _a32(g), _a32(v)
    eta, ns = _group(attr, sc.lr), _group(attr, sc.ns)
    with np.errstate(all="ignore"):
        t = sc.prior_sig * th
        gU = g + t
        x = v * sc.oma
        y = eta * gU
        vn = x - y
        if eps is not None:
            nz = ns * _a32(eps)
            vn = vn + nz
        nth = th + vn
    return _keep(attr, nth, th), _keep(attr, vn, v)


# ----------------------------------------------------------------------- SGLD
def _prior_term(th, th0, sc, mode):
    d = th - th0
    e = sdiv(d, sc.sigma2, mode)
    return sdiv(e, sc.n_data, mode)


def sgld_grad(th, th0, g, attr, sc, eps, mode):
    """methods/sgld.py:471-484: p.grad = g + (prior + noise), or g + noise for
    an uninformative bias.  Returns the gradient written (SGLD_GRAD)."""
    th, th0, g, eps = _a32(th), _a32(th0), _a32(g), _a32(eps)
    ns = _group(attr, sc.ns)
    with np.errstate(all="ignore"):
        nz = ns * eps
        f = _prior_term(th, th0, sc, mode)
        with_prior = g + (f + nz)
        without = g + nz
    gp = np.where((attr & ATTR_PRIOR) != 0, with_prior, without)
    return _keep(attr, gp, g)


def sgld(th, th0, g, buf, attr, sc, eps, mode, momentum=None, clip_coef=None):
    """The SGLD step: the sampler gradient, clip_grad_norm_'s grads.mul_(coef)
    when a coefficient is given, then the SGD step.  Returns (theta, buf)."""
    gp = sgld_grad(th, th0, g, attr, sc, eps, mode)
    if clip_coef is not None:
        with np.errstate(all="ignore"):
            gp = gp * F(clip_coef)
    return sgd_step(th, gp, buf, attr, sc, momentum)


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient from a total norm: max_norm / (norm + 1e-6)
    as reciprocal() * max_norm, clamped at 1 with fminf.  A NaN norm gives 1
    (fminf returns its other operand): the gradient is left as it is, where
    clip_grad_norm_ would multiply it by NaN (include/bdl_clip.h)."""
    with np.errstate(all="ignore"):
        r = F(1.0) / (F(norm) + F(1e-6))
        c = F(r * f32(max_norm))
    if np.isnan(c):
        return F(1.0)
    return c if c < F(1.0) else F(1.0)


# ---------------------------------------------------------------------- SGHMC
def sghmc_grad(th, th0, g, v, attr, sc, eps, mode):
    """methods/sghmc.py:494-510: v' = v(1-a) + lr * grad_U + noise; p.grad =
    g + v'.  Returns (gradient written, v')."""
    th, th0, g, v, eps = _a32(th), _a32(th0), _a32(g), _a32(v), _a32(eps)
    eta, ns = _group(attr, sc.lr), _group(attr, sc.ns)
    with np.errstate(all="ignore"):
        f = _prior_term(th, th0, sc, mode)
        gU = np.where((attr & ATTR_PRIOR) != 0, g + f, g)
        x = v * sc.oma
        y = eta * gU
        s = x + y
        nz = ns * eps
        vn = s + nz
        gp = g + vn
    return _keep(attr, gp, g), _keep(attr, vn, v)


def sghmc(th, th0, g, v, attr, sc, eps, mode):
    """SGHMC_GRAD followed by SGD(momentum 0).  Returns (theta, v')."""
    gp, vn = sghmc_grad(th, th0, g, v, attr, sc, eps, mode)
    nth, _ = sgd_step(th, gp, None, attr, sc, None)
    return nth, vn


# ----------------------------------------------------------------- Adam-SGHMC
def adam_grad(th, th0, g, vm, m, v, attr, sc, ad, eps, mode, grad_is_mom=False):
    """methods/adam_sghmc.py:512-553 (grad_is_mom False: p.grad + v_mom) and
    methods/adam_csghmc.py:819-860 (grad_is_mom True, g / temperature).
    eps None: no noise term.  Returns (gradient written, v_mom, m, v)."""
    th, th0, g, vm, m, v = (_a32(x) for x in (th, th0, g, vm, m, v))
    eta = _group(attr, sc.lr)
    with np.errstate(all="ignore"):
        gs = sdiv(g, ad.temp, mode)
        f = _prior_term(th, th0, sc, mode)
        gU = np.where((attr & ATTR_PRIOR) != 0, gs + f, gs)
        m_a = m * ad.b1
        m_b = gU * ad.omb1
        mn = m_a + m_b
        v_a = v * ad.b2
        g2 = gU * gU
        v_b = g2 * ad.omb2
        vn = v_a + v_b
        mh = sdiv(mn, ad.bc1, mode)
        vh = sdiv(vn, ad.bc2, mode)
        den = np.sqrt(vh) + ad.eps
        pg = mh / den
        pt = F(1.0) / den
        vm_a = vm * ad.oma
        vm_b = pg * eta
        vmn = vm_a + vm_b
        if eps is not None:
            q = sdiv(pt * ad.two_alpha, sc.n_data, mode)
            nsc = np.sqrt(q) * ad.nd
            nz = nsc * _a32(eps)
            vmn = vmn + nz
        else:
            vmn = vmn + F(0.0)
        gp = vmn if grad_is_mom else g + vmn
    return (_keep(attr, gp, g), _keep(attr, vmn, vm), _keep(attr, mn, m), _keep(attr, vn, v))


def adam(th, th0, g, vm, m, v, buf, attr, sc, ad, eps, mode, grad_is_mom=False, momentum=None):
    """ADAM_SGHMC_GRAD followed by the SGD step.  Returns (theta, v_mom, m, v, buf)."""
    gp, vmn, mn, vn = adam_grad(th, th0, g, vm, m, v, attr, sc, ad, eps, mode, grad_is_mom)
    nth, nbuf = sgd_step(th, gp, buf, attr, sc, momentum)
    return nth, vmn, mn, vn, nbuf


# ------------------------------------------------------------------- collects
def collect(kind, th, m1, m2, sc, mode):
    """The posterior-moment update on the (updated) theta, every element.
    m2 None: no second moment is kept.  Returns (m1, m2)."""
    th = _a32(th)
    with np.errstate(all="ignore"):
        if kind == NONE:
            return m1, m2
        if kind == WELFORD_INIT:
            return th.copy(), (None if m2 is None else np.zeros_like(th))
        if kind == MEAN_INIT:
            return th.copy(), (None if m2 is None else th * th)
        m1 = _a32(m1)
        if kind == WELFORD:  # csghmc.py:340-345
            d = th - m1
            n1 = m1 + sdiv(d, sc.ca, mode)
            if m2 is None:
                return n1, None
            d2 = th - n1
            return n1, _a32(m2) + d * d2
        assert kind == MEAN, kind  # sgld.py:242-245: (x + a * m) / b
        n1 = sdiv(th + sc.ca.s * m1, sc.cb, mode)
        if m2 is None:
            return n1, None
        return n1, sdiv(th * th + sc.ca.s * _a32(m2), sc.cb, mode)
