"""The host reference of the update rules (tests/step_ref.py) checked on its
own: its fused multiply-add against exact rational arithmetic, its rules
against the torch-CPU oracle that is pinned bit-exactly to the upstream
sampler's goldens (oracle/sgmcmc_oracle.py), and its two division modes
against each other.  No GPU: test_gpu_step_reference.py compares the kernels
with this reference."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import step_ref as R
from fakenet import TOY_READOUT, TOY_SEGMENTS, numel_of
from oracle import sgmcmc_oracle as O

F = np.float32


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32, what
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()))


# ------------------------------------------------------------------------ fma
def _round_f32(t):
    """A nonzero Fraction rounded to fp32, nearest-even, exactly."""
    assert t != 0
    a = abs(t)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)
    k = a / q
    n = k.numerator // k.denominator
    rem = k - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    v = n * q
    if v >= Fraction(2) ** 128:
        return F(np.inf) if t > 0 else F(-np.inf)
    out = F(float(v))  # exact: at most 24 significant bits
    return out if t > 0 else -out


def _midpoint_distance(t):
    """(distance of the Fraction t to the nearest fp32 rounding midpoint, one
    float64 ulp at that midpoint)."""
    a = abs(t)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)  # fp32 ulp at t
    k = a / q
    n = k.numerator // k.denominator
    mid = (n + Fraction(1, 2)) * q
    return abs(a - mid), Fraction(2) ** (max(e, -1022) - 52)


def _fma_triples():
    rng = np.random.default_rng(77)
    tri, constructed = [], 0
    # exactly on a midpoint: c = M - a*b, M the product cut to 25 bits with
    # the 25th set; c fits fp32 (it spans the product's low 23 bits)
    while constructed < 700:
        a = F(rng.standard_normal() * 2.0 ** rng.integers(-20, 20))
        b = F(rng.standard_normal() * 2.0 ** rng.integers(-20, 20))
        p = Fraction(float(a)) * Fraction(float(b))
        if p == 0:
            continue
        ap = abs(p)
        e = ap.numerator.bit_length() - ap.denominator.bit_length()
        if Fraction(2) ** e > ap:
            e -= 1
        q = Fraction(2) ** (e - 24)  # the 25th bit
        k = ap / q
        n = k.numerator // k.denominator
        n |= 1
        M = n * q * (1 if p > 0 else -1)
        c = M - p
        c32 = F(float(c))
        if Fraction(float(c32)) != c or c == 0:
            continue
        tri.append((a, b, c32))
        constructed += 1
    # beside a midpoint by 2^(-2j) of half an ulp, j = 12 .. 23: from one
    # float64 ulp beside (j = 14) to far below it (the float64 sum lands on
    # the midpoint: the double-rounding case)
    while constructed < 1400:
        c = F(rng.standard_normal() * 2.0 ** rng.integers(-30, 30))
        if c == 0 or not np.isfinite(c):
            continue
        j = int(rng.integers(12, 24))
        half_ulp = float(np.spacing(np.abs(c))) / 2
        s = 1.0 if c > 0 else -1.0
        side = rng.integers(0, 2)
        if side:  # from below the midpoint above |c|
            a = F(s * (1 + 2.0 ** -j))
            b = F(half_ulp * (1 - 2.0 ** -j))
            cc = c
        else:     # from above it: the next float minus the same product
            cc = np.nextafter(c, F(np.inf) * F(s))
            a = F(-s * (1 + 2.0 ** -j))
            b = F(half_ulp * (1 - 2.0 ** -j))
        if float(b) == 0.0 or np.spacing(np.abs(cc)) != np.spacing(np.abs(c)):
            continue
        tri.append((a, b, F(cc)))
        constructed += 1
    n_constructed = len(tri)
    # random: wide exponents, cancellation, subnormal results
    for _ in range(9000):
        a = F(rng.standard_normal() * 2.0 ** rng.integers(-60, 60))
        b = F(rng.standard_normal() * 2.0 ** rng.integers(-60, 60))
        kind = rng.integers(0, 4)
        if kind == 0:
            c = F(-float(a) * float(b))  # cancellation to the product's low bits
        elif kind == 1:
            c = F(rng.standard_normal() * 2.0 ** -140)
            a, b = F(float(a) * 2.0 ** -70), F(float(b) * 2.0 ** -70)
        else:
            c = F(rng.standard_normal() * 2.0 ** rng.integers(-60, 60))
        tri.append((a, b, c))
    return tri, n_constructed


def test_fma_is_correctly_rounded():
    tri, n_constructed = _fma_triples()
    assert len(tri) >= 10000 and n_constructed >= 1000
    a, b, c = (np.array([t[i] for t in tri], dtype=F) for i in range(3))
    got = R.fma32(a, b, c)
    assert got.dtype == np.float32
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    near = double_rounded = checked = 0
    for i, (x, y, z) in enumerate(tri):
        t = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        if t == 0:
            assert got[i] == 0
            continue
        want = _round_f32(t)
        assert _bits(got[i:i + 1])[0] == _bits(np.array([want], F))[0], (i, x, y, z, got[i], want)
        checked += 1
        if i < n_constructed:
            dist, ulp64 = _midpoint_distance(t)
            near += dist <= ulp64
        double_rounded += _bits(naive[i:i + 1])[0] != _bits(np.array([want], F))[0]
    assert checked >= 10000 - 100
    assert near >= 1000, near        # the construction produced the midpoint cases
    assert double_rounded >= 50, double_rounded  # and the plain float64 route gets some wrong


def test_fma_signed_zeros_and_exact_cases():
    z, nz, one = F(0.0), F(-0.0), F(1.0)
    cases = [(nz, one, z, z), (nz, one, nz, nz), (z, one, nz, z), (F(-1.0), one, one, z),
             (F(-2.0), F(3.0), F(7.0), one), (F(-1e-3), z, nz, nz), (F(-1e-3), nz, nz, z)]
    a, b, c, want = (np.array([t[i] for t in cases], dtype=F) for i in range(4))
    assert np.array_equal(_bits(R.fma32(a, b, c)), _bits(want))


# -------------------------------------------------------------------- oracle
N = numel_of(TOY_SEGMENTS)
NAMES = [nm for nm, _ in TOY_SEGMENTS]
SHAPES = [s for _, s in TOY_SEGMENTS]
NUMELS = [int(np.prod(s)) for s in SHAPES]
LR, LR_HEAD, ND_, NDATA, PRIOR_SIG, ALPHA, MU = 1e-3, 2e-2, 0.5, 1840, 0.8, 0.18, 0.5


def _attrs(bias):
    at = [(R.ATTR_HEAD if TOY_READOUT in nm else 0)
          | (0 if ("bias" in nm and bias == "uninformative") else R.ATTR_PRIOR) for nm in NAMES]
    return R.element_attrs(NUMELS, at)


def _vec(tag, scale):
    rng = np.random.default_rng([11, tag])
    return (rng.standard_normal(N).astype(F) * F(scale)).astype(F)


def _grad(t):
    return _vec(100 + t, 1e-2)


def _noise(t):
    return _vec(200 + t, 1.0)


def _cfg(method, bias, **kw):
    hp = dict(Ninflate=1.0, nd=ND_, prior_sig=PRIOR_SIG, bias=bias, thin=1, nst=1, burnin=0,
              momentum_decay=ALPHA)
    return dict(method=method, hparams=hp, ND=NDATA, lr=LR, lr_head=LR_HEAD, bpe=3, epochs=1, **kw)


def _simulate(cfg):
    return O.simulate(cfg, TOY_SEGMENTS, TOY_READOUT, _vec(1, 0.02), _vec(2, 0.02), _grad, _noise)


@pytest.mark.parametrize("bias", ["informative", "uninformative"])
def test_sgld_sgd_momentum_and_running_means_match_the_oracle(bias):
    out = _simulate(_cfg("sgld", bias, momentum=MU))
    attr = _attrs(bias)
    ns = [ND_ * np.sqrt(2 / (float(NDATA) * lr)) for lr in (LR, LR_HEAD)]
    th, th0, buf = _vec(1, 0.02), _vec(2, 0.02), None
    sc = R.Scalars(lrs=(LR, LR_HEAD), noise_scale=ns, sigma2=PRIOR_SIG ** 2, n_data=float(NDATA),
                   mu=MU)
    m1, m2 = R.collect(R.MEAN_INIT, th, None, np.zeros(0, F), sc, "true")  # sgld.py:95-102
    for t in range(3):
        th, buf = R.sgld(th, th0, _grad(t), buf, attr, sc, _noise(t), "true",
                         momentum="first" if t == 0 else "later")
        _same(th, out["theta"][t + 1], ("theta", t))
        _same(buf, out["mom"][t + 1], ("sgd buffer", t))
        cs = R.Scalars(lrs=(LR, LR_HEAD), collect_a=float(t + 1), collect_b=float(t + 2))
        m1, m2 = R.collect(R.MEAN, th, m1, m2, cs, "true")
    _same(m1, out["post_mom1"], "running mean")
    _same(m2, out["post_mom2"], "running second moment")
    assert out["post_cnt"] == 4


@pytest.mark.parametrize("bias", ["informative", "uninformative"])
def test_sghmc_sgd_matches_the_oracle(bias):
    out = _simulate(_cfg("sghmc", bias))
    attr = _attrs(bias)
    ns = [ND_ * np.sqrt(2 * ALPHA / (float(NDATA) * lr)) for lr in (LR, LR_HEAD)]
    sc = R.Scalars(lrs=(LR, LR_HEAD), noise_scale=ns, one_minus_alpha=1 - ALPHA,
                   sigma2=PRIOR_SIG ** 2, n_data=float(NDATA))
    th, th0, v = _vec(1, 0.02), _vec(2, 0.02), np.zeros(N, F)
    m1, m2 = R.collect(R.MEAN_INIT, th, None, np.zeros(0, F), sc, "true")
    for t in range(3):
        th, v = R.sghmc(th, th0, _grad(t), v, attr, sc, _noise(t), "true")
        _same(th, out["theta"][t + 1], ("theta", t))
        _same(v, out["mom"][t + 1], ("momentum", t))
        cs = R.Scalars(lrs=(LR, LR_HEAD), collect_a=float(t + 1), collect_b=float(t + 2))
        m1, m2 = R.collect(R.MEAN, th, m1, m2, cs, "true")
    _same(m1, out["post_mom1"], "running mean")
    _same(m2, out["post_mom2"], "running second moment")


@pytest.mark.parametrize("bias", ["informative", "uninformative"])
def test_csghmc_and_welford_match_the_oracle(bias):
    """Four steps of one cycle, the first two exploring (no noise, no
    collect), then the cycle-init collect and one Welford update (divisor 3:
    the Runner's doubled samples_per_cycle increment)."""
    cfg = _cfg("csghmc", bias, num_cycles=1, beta=0.5)
    cfg["bpe"] = 4
    out = _simulate(cfg)
    assert list(out["should_sample"]) == [False, False, True, True]
    attr = _attrs(bias)
    th, v = _vec(1, 0.02), np.zeros(N, F)
    m1 = m2 = None
    for t in range(4):
        lrs = [float(x) for x in out["lrs"][t]]
        ns = [ND_ * np.sqrt(2 * ALPHA * lr) / float(NDATA) for lr in lrs]
        sample = bool(out["should_sample"][t])
        sc = R.Scalars(lrs=lrs, noise_scale=ns, one_minus_alpha=1 - ALPHA, prior_sig=PRIOR_SIG,
                       collect_a=3.0)
        th, v = R.csghmc(th, _grad(t), v, attr, sc, _noise(t) if sample else None)
        _same(th, out["theta"][t + 1], ("theta", t))
        _same(v, out["mom"][t + 1], ("momentum", t))
        if sample:
            kind = R.WELFORD_INIT if m1 is None else R.WELFORD
            m1, m2 = R.collect(kind, th, m1, np.zeros(0, F) if m2 is None else m2, sc, "true")
    _same(m1, out["cycle_mom1"][0], "Welford mean")
    _same(m2, out["cycle_mom2"][0], "Welford M2")
    assert int(out["samples_per_cycle"][0]) == 4


def _split(vec):
    return [t.clone() for t in torch.from_numpy(np.ascontiguousarray(vec)).split(NUMELS)]


def _cat(ts):
    return torch.cat([t.reshape(-1) for t in ts]).numpy().copy()


@pytest.mark.parametrize("bias", ["informative", "uninformative"])
def test_clipped_sgld_matches_the_oracle_given_its_coefficient(bias):
    attr = _attrs(bias)
    ns = [ND_ * np.sqrt(2 / (float(NDATA) * lr)) for lr in (LR, LR_HEAD)]
    sc = R.Scalars(lrs=(LR, LR_HEAD), noise_scale=ns, sigma2=PRIOR_SIG ** 2, n_data=float(NDATA),
                   mu=MU)
    is_head = [TOY_READOUT in nm for nm in NAMES]
    th, th0, buf = _vec(1, 0.02), _vec(2, 0.02), None
    params, params0, bufs = _split(th), _split(th0), [None] * len(NAMES)
    clipped = 0
    for t, max_norm in enumerate((1.0, 1e6, 5.0)):
        newg = O.sgld_model(params, params0, _split(_grad(t)), NAMES, TOY_READOUT, [LR, LR_HEAD],
                            PRIOR_SIG, bias, float(NDATA), ND_, _split(_noise(t)))
        _same(R.sgld_grad(th, th0, _grad(t), attr, sc, _noise(t), "true"), _cat(newg),
              ("sampler gradient", t))
        total = O.clip_grad_norm(newg, max_norm)
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        assert coef.dtype == torch.float32
        assert _bits(np.array([R.clip_coef(total.item(), max_norm)], F))[0] == \
            _bits(coef.numpy().reshape(1))[0]
        clipped += coef.item() < 1.0
        bufs = O.sgd_step(params, newg, bufs, [LR_HEAD if h else LR for h in is_head], MU)
        th, buf = R.sgld(th, th0, _grad(t), buf, attr, sc, _noise(t), "true",
                         momentum="first" if t == 0 else "later", clip_coef=F(coef.item()))
        _same(th, _cat(params), ("theta", t))
        _same(buf, _cat(bufs), ("sgd buffer", t))
    assert clipped == 2  # clipping active twice, inactive (coef 1) once


RTOL = 1e-5  # test_gpu_parity.py: torch-CPU's vectorised sqrt is not correctly rounded


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("grad_is_mom,temperature", [(False, 1.0), (True, 0.7)])
@pytest.mark.parametrize("bias", ["informative", "uninformative"])
def test_adam_sghmc_matches_the_oracle(bias, grad_is_mom, temperature):
    """adam_m / adam_v bit-exact (no sqrt on their path) while every step's
    inputs are the oracle's own; momentum and theta within RTOL."""
    attr = _attrs(bias)
    is_head = [TOY_READOUT in nm for nm in NAMES]
    sc = R.Scalars(lrs=(LR, LR_HEAD), sigma2=PRIOR_SIG ** 2, n_data=float(NDATA), mu=MU)
    th0 = _vec(2, 0.02)
    params, params0 = _split(_vec(1, 0.02)), _split(th0)
    vms, ms, vs = (_split(np.zeros(N, F)) for _ in range(3))
    bufs = [None] * len(NAMES)
    th, vm, buf = _vec(1, 0.02), np.zeros(N, F), None
    for t in range(3):
        ad = R.AdamScalars(beta1=0.9, beta2=0.999, eps=1e-8, t=t + 1, momentum_decay=ALPHA,
                           nd=ND_, temperature=temperature)
        # the reference stepped from the oracle's own state: m and v bit-exact
        o_th, o_vm, o_m, o_v = _cat(params), _cat(vms), _cat(ms), _cat(vs)
        o_buf = None if bufs[0] is None else _cat(bufs)
        r = R.adam(o_th, th0, _grad(t), o_vm, o_m, o_v, o_buf, attr, sc, ad, _noise(t), "true",
                   grad_is_mom=grad_is_mom, momentum="first" if t == 0 else "later")
        # and along its own trajectory
        th, vm, m_own, v_own, buf = R.adam(th, th0, _grad(t), vm, o_m if t == 0 else m_own,
                                           o_v if t == 0 else v_own, buf, attr, sc, ad, _noise(t),
                                           "true", grad_is_mom=grad_is_mom,
                                           momentum="first" if t == 0 else "later")
        newg, vms, ms, vs = O.adam_sghmc_model(
            params, params0, _split(_grad(t)), vms, ms, vs, NAMES, TOY_READOUT, [LR, LR_HEAD],
            PRIOR_SIG, bias, ALPHA, 0.9, 0.999, 1e-8, t + 1, float(NDATA), ND_, _split(_noise(t)),
            temperature=temperature, grad_is_mom=grad_is_mom)
        bufs = O.sgd_step(params, newg, bufs, [LR_HEAD if h else LR for h in is_head], MU)
        _same(r[2], _cat(ms), ("adam_m", t))
        _same(r[3], _cat(vs), ("adam_v", t))
        assert _rel(r[1], _cat(vms)) <= RTOL and _rel(r[0], _cat(params)) <= RTOL, t
        assert _rel(r[4], _cat(bufs)) <= RTOL, t
        assert _rel(vm, _cat(vms)) <= RTOL and _rel(th, _cat(params)) <= RTOL, t
        assert _rel(buf, _cat(bufs)) <= RTOL, t


# ------------------------------------------------------------ division modes
def test_division_modes_are_distinct_and_agree_on_powers_of_two():
    attr = np.full(N, R.ATTR_PRIOR, np.uint8)
    th, th0, g, eps, m1, m2 = (_vec(300 + i, s) for i, s in
                               enumerate((0.02, 0.02, 1e-2, 1.0, 0.02, 1e-3)))

    def run(sigma2, n_data, ca, cb, mode):
        # no noise: next to it the prior term (~1e-5) would vanish in the sum
        sc = R.Scalars(lrs=(LR, LR_HEAD), noise_scale=(0.0, 0.0), sigma2=sigma2, n_data=n_data,
                       collect_a=ca, collect_b=cb)
        ad = R.AdamScalars(beta1=0.5, beta2=0.75, eps=1e-8, t=1, momentum_decay=ALPHA, nd=ND_,
                           temperature=sigma2)
        return (R.sgld_grad(th, th0, g * F(1e-4), attr, sc, eps, mode),
                R.collect(R.WELFORD, th, m1, np.abs(m2), sc, mode)[0],
                R.collect(R.MEAN, th, m1, np.abs(m2), R.Scalars(lrs=(LR, LR), collect_a=ca - 1,
                                                                collect_b=cb), mode)[1],
                R.adam_grad(th, th0, g, m1, m1, np.abs(m2), attr, sc, ad, eps, mode)[0])

    for t, r in zip(run(0.8 ** 2, 1840.0, 3.0, 3.0, "true"), run(0.8 ** 2, 1840.0, 3.0, 3.0, "recip")):
        assert (_bits(t) != _bits(r)).any()
    # beta 0.5 / 0.75 at t = 1: bias corrections 0.5 and 0.25 are powers of two as well
    for t, r in zip(run(4.0, 2048.0, 2.0, 4.0, "true"), run(4.0, 2048.0, 2.0, 4.0, "recip")):
        _same(t, r, "power-of-two divisors")
    # the fallback reciprocal fl32(1 / fl32(s)) is a third value for some divisors
    s = 1840.1
    assert R.Div.fallback(s).s == R.Div(s).s
