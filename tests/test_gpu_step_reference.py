"""Every step-kernel instance against the op-by-op fp32 host reference.

tests/step_ref.py restates each update rule in NumPy fp32, one rounding per
line, from the upstream sampler (and is itself pinned to the torch-CPU oracle
in test_step_ref.py).  Here every method variant, crossed with every collect
kind the C-ABI accepts for it, runs on the 39,426-element table of
test_gpu_noise_units.py (fast, multi-run and guarded iterations at every
depth; uninformative biases, a frozen tensor, a head) with buffer noise from
the host, at four launch geometries and in both division modes, and every
vector is compared with the reference as int32 bit patterns over all elements
(NaN positions as NaN-ness).  Vectors a launch must not write are unchanged,
frozen elements untouched, the nonfinite flag 0.  One convention the older
tests already pin (test_gpu_kernels.py ref_clip_sgld): a first step with SGD
momentum stores +0 in the SGD buffer of frozen elements — torch holds no
buffer for a parameter without a gradient, and mu * 0 + g equals clone(g) at
its first one; asserted as exactly that here.

The only tolerance in this file is the clipped step's norm: within one fp32
ulp of fl32(sqrt(S)), S the float64 sum of squares of the reference's fp32
sampler gradient.  The kernel accumulates exact squares (fp64 FMA of fp32
values) in fp64 — relative error about n * 2^-53, far below 2^-24 — so only
the final rounding to fp32 can differ.

Adversarial values (test_adversarial_values): signed zeros, subnormals,
FLT_MIN, theta == +-prior, grad == +-0, m1 == theta, adam_v == 0 with a zero
gradient, a subnormal adam_v, magnitudes of 2^+-60; the expectation is bit
equality, signed zeros included; no value had to be narrowed.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import step_ref as R
from test_gpu_noise_units import FROZEN, VECTORS, WRITTEN, Table

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32

GEOMETRIES = [(1, 1, 1), (1, 2, 1), (1, 4, 1), (2, 4, 0)]
MODES = ["true", "recip"]

# Scalars chosen so that every term of every rule reaches the result: with the
# samplers' own noise scales (and N in the thousands) the noise would swallow
# the prior term's last bits, and a wrong division mode with them.
LRS, N_DATA, SIGMA2, PRIOR_SIG, OMA, MU, TEMP = (1e-3, 2e-2), 7.0, 0.8 ** 2, 0.8, 0.82, 0.5, 0.7

CSG = dict(lrs=LRS, noise_scale=(1e-4, 3e-4), one_minus_alpha=OMA, prior_sig=PRIOR_SIG)
SGLD = dict(lrs=LRS, noise_scale=(3e-3, 7e-3), sigma2=SIGMA2, n_data=N_DATA)
SGHMC = dict(lrs=LRS, noise_scale=(1e-4, 3e-4), one_minus_alpha=OMA, sigma2=SIGMA2, n_data=N_DATA)
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, momentum_decay=0.18, nd=2e-4, lrs=LRS, sigma2=SIGMA2,
            n_data=N_DATA)
_SC_KEYS = ("lrs", "noise_scale", "one_minus_alpha", "prior_sig", "sigma2", "n_data", "mu")
_AD_KEYS = ("beta1", "beta2", "eps", "t", "momentum_decay", "nd", "temperature")


def _first_buf(v):
    """The SGD buffer a first step creates (None on any other launch)."""
    return None if v.mom != "first" else "sgd_buf" if v.family == "adam" else "mom"


def _v(family, method, kw, mom=None, ready=False, noise=True, gim=False):
    return SimpleNamespace(family=family, method=method, kw=kw, mom=mom, ready=ready, noise=noise,
                           gim=gim, grad_only=method.endswith("_GRAD"))


def _sgd(mom):
    return {} if mom is None else dict(mu=MU, momentum=True, first_step=mom == "first")


VARIANTS = {
    "csghmc_noise": _v("csghmc", "CSGHMC", CSG),
    "csghmc_explore": _v("csghmc", "CSGHMC", CSG, noise=False),
    "sgld_no_momentum": _v("sgld", "SGLD", SGLD),
    "sgld_first": _v("sgld", "SGLD", dict(SGLD, **_sgd("first")), mom="first"),
    "sgld_later": _v("sgld", "SGLD", dict(SGLD, **_sgd("later")), mom="later"),
    "sgld_grad": _v("sgld", "SGLD_GRAD", SGLD),
    "sgld_ready_no_momentum": _v("sgld", "SGLD", dict(SGLD, grad_ready=True), ready=True),
    "sgld_ready_first": _v("sgld", "SGLD", dict(SGLD, grad_ready=True, **_sgd("first")),
                           mom="first", ready=True),
    "sgld_ready_later": _v("sgld", "SGLD", dict(SGLD, grad_ready=True, **_sgd("later")),
                           mom="later", ready=True),
    "sghmc": _v("sghmc", "SGHMC", SGHMC),
    "sghmc_grad": _v("sghmc", "SGHMC_GRAD", SGHMC),
    "sghmc_ready": _v("sghmc", "SGHMC", dict(SGHMC, grad_ready=True), ready=True),
    "adam_no_buffer": _v("adam", "ADAM_SGHMC", dict(ADAM, t=3)),
    "adam_first": _v("adam", "ADAM_SGHMC", dict(ADAM, t=1, **_sgd("first")), mom="first"),
    "adam_later": _v("adam", "ADAM_SGHMC", dict(ADAM, t=2, **_sgd("later")), mom="later"),
    "adam_csghmc_later": _v("adam", "ADAM_SGHMC", dict(ADAM, t=4, temperature=TEMP, grad_is_mom=True,
                                                       **_sgd("later")), mom="later", gim=True),
    "adam_csghmc_no_buffer": _v("adam", "ADAM_SGHMC", dict(ADAM, t=2, temperature=TEMP,
                                                           grad_is_mom=True), gim=True),
    "adam_grad": _v("adam", "ADAM_SGHMC_GRAD", dict(ADAM, t=3)),
    "adam_csghmc_grad": _v("adam", "ADAM_SGHMC_GRAD", dict(ADAM, t=3, temperature=TEMP,
                                                           grad_is_mom=True), gim=True),
}

# collect configurations: (kind name, second moment kept, collect_a, collect_b)
COLLECTS = [("NONE", True, 1.0, 1.0), ("WELFORD_INIT", True, 1.0, 1.0), ("WELFORD", True, 3.0, 1.0),
            ("MEAN_INIT", True, 1.0, 2.0), ("MEAN", True, 2.0, 3.0), ("WELFORD", False, 3.0, 1.0),
            ("MEAN", False, 2.0, 3.0)]


def _accepted(v, ck):
    """What the C-ABI's validation admits (bdl_api.hip launch_step /
    bdl_adam_step, bdl_adam.hip pick_adam_collect)."""
    if ck[0] == "NONE":
        return True
    if v.grad_only:
        return False
    return not (v.family == "adam" and ck[0].startswith("WELFORD"))


# ------------------------------------------------------------------- plumbing
_T = {}


def _table():
    if "t" not in _T:
        t = Table()
        t.elem_attr = R.element_attrs(t.numels, t.attrs)
        i = t.names.index(FROZEN)
        t.frozen = slice(t.offsets[i], t.offsets[i] + t.numels[i])
        assert (t.elem_attr[t.frozen] & R.ATTR_SKIP).all()
        assert int((t.elem_attr & R.ATTR_SKIP != 0).sum()) == t.numels[i]
        _T["t"] = t
    return _T["t"]


def _start():
    _table()
    return {nm: Table._init[nm].numpy().copy() for nm in VECTORS}


def _load(t, h):
    for nm in VECTORS:
        t.v[nm].copy_(torch.from_numpy(np.ascontiguousarray(h[nm])))
    t.nonfinite.zero_()


def _read(t):
    torch.cuda.synchronize()
    return {nm: t.v[nm].cpu().numpy() for nm in VECTORS}


def _assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    ok = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        idx = np.flatnonzero(~ok)
        raise AssertionError((what, f"{idx.size} elements differ", idx[:6].tolist(),
                              got[idx[:6]].tolist(), want[idx[:6]].tolist()))


def _check(t, h, exp, what, first_buf=None):
    """Every vector of the table against the expectation (the inputs where the
    launch writes nothing); frozen elements as they were (first_buf: the SGD
    buffer of a first step, +0 there); the flag 0."""
    got = _read(t)
    for nm in VECTORS:
        _assert_bits(got[nm], exp.get(nm, h[nm]), what + (nm,))
    for nm in WRITTEN:
        if nm == first_buf:
            assert not got[nm][t.frozen].view(np.int32).any(), what + (nm, "frozen")
        elif nm not in ("m1", "m2"):  # the collect reads the frozen theta too
            _assert_bits(got[nm][t.frozen], h[nm][t.frozen], what + (nm, "frozen"))
    assert int(t.nonfinite.item()) == 0, what


def _launch(st, v, mode, ck, kw_over=None):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    kw = dict(v.kw, **(kw_over or {}))
    kind, has_m2, ca, cb = ck
    if kind != "NONE":
        kw.update(collect=getattr(L, "COLLECT_" + kind), mom1=st.v["m1"],
                  mom2=st.v["m2"] if has_m2 else None, collect_a=ca, collect_b=cb)
    kw.update(noise_mode=L.NOISE_BUFFER if v.noise else L.NOISE_NONE, div_mode=mode)
    method = getattr(L, v.method)
    if v.family == "adam":
        K.adam_step(st, method, adam_m=st.v["adam_m"], adam_v=st.v["adam_v"],
                    sgd_buf=st.v["sgd_buf"] if v.mom else None, **kw)
    else:
        K.sgmcmc_step(st, method, **kw)


def _scalars(v, ck, kw_over=None, fallback=()):
    kw = dict(v.kw, **(kw_over or {}))
    sc = R.Scalars(**{k: kw[k] for k in _SC_KEYS if k in kw}, collect_a=ck[2], collect_b=ck[3])
    for nm, s64 in fallback:
        setattr(sc, nm, R.Div.fallback(s64))
    ad = R.AdamScalars(**{k: kw[k] for k in _AD_KEYS if k in kw}) if v.family == "adam" else None
    return sc, ad


def _expected(v, h, attr, mode, ck, kw_over=None, fallback=(), clip_coef=None):
    """The vectors the launch writes, from the host reference."""
    sc, ad = _scalars(v, ck, kw_over, fallback)
    th, th0, g, eps = h["theta"], h["prior"], h["grad"], h["noise"]
    exp = {}
    if v.family == "csghmc":
        exp["theta"], exp["mom"] = R.csghmc(th, g, h["mom"], attr, sc, eps if v.noise else None)
    elif v.ready:
        exp["theta"], buf = R.sgd_step(th, g, h["mom"], attr, sc, v.mom)
        if v.mom:
            exp["mom"] = buf
    elif v.method == "SGLD":
        exp["theta"], buf = R.sgld(th, th0, g, h["mom"], attr, sc, eps, mode, v.mom, clip_coef)
        if v.mom:
            exp["mom"] = buf
    elif v.method == "SGLD_GRAD":
        exp["grad"] = R.sgld_grad(th, th0, g, attr, sc, eps, mode)
    elif v.method == "SGHMC":
        exp["theta"], exp["mom"] = R.sghmc(th, th0, g, h["mom"], attr, sc, eps, mode)
    elif v.method == "SGHMC_GRAD":
        exp["grad"], exp["mom"] = R.sghmc_grad(th, th0, g, h["mom"], attr, sc, eps, mode)
    elif v.method == "ADAM_SGHMC":
        r = R.adam(th, th0, g, h["mom"], h["adam_m"], h["adam_v"], h["sgd_buf"], attr, sc, ad, eps,
                   mode, grad_is_mom=v.gim, momentum=v.mom)
        exp["theta"], exp["mom"], exp["adam_m"], exp["adam_v"] = r[:4]
        if v.mom:
            exp["sgd_buf"] = r[4]
    else:
        assert v.method == "ADAM_SGHMC_GRAD"
        exp["grad"], exp["mom"], exp["adam_m"], exp["adam_v"] = R.adam_grad(
            th, th0, g, h["mom"], h["adam_m"], h["adam_v"], attr, sc, ad, eps, mode, grad_is_mom=v.gim)
    kind, has_m2 = ck[0], ck[1]
    if kind != "NONE":
        m1, m2 = R.collect(getattr(R, kind), exp.get("theta", th), h["m1"],
                           h["m2"] if has_m2 else None, sc, mode)
        exp["m1"] = m1
        if has_m2:
            exp["m2"] = m2
    return exp


# --------------------------------------------------------------------- matrix
@pytest.mark.parametrize("case", list(VARIANTS))
def test_step_matches_the_host_reference(case):
    from bayesdll_amd import kernels as K
    v, t, h = VARIANTS[case], _table(), _start()
    st = t.state()
    launches = 0
    try:
        for ck in COLLECTS:
            if not _accepted(v, ck):
                _load(t, h)
                with pytest.raises(RuntimeError):
                    _launch(st, v, "true", ck)
                continue
            for mode in MODES:
                exp = _expected(v, h, t.elem_attr, mode, ck)
                assert any(not np.array_equal(exp[nm].view(np.int32), h[nm].view(np.int32))
                           for nm in exp), (case, ck)  # the launch changes something
                for geo in GEOMETRIES:
                    _load(t, h)
                    K.set_launch_config(*geo)
                    _launch(st, v, mode, ck)
                    _check(t, h, exp, (case, ck[:2], mode, geo), _first_buf(v))
                    launches += 1
    finally:
        K.set_launch_config(0, 0, 0)
    assert launches == len(MODES) * len(GEOMETRIES) * sum(_accepted(v, ck) for ck in COLLECTS)


def test_division_modes_differ_on_this_table():
    """The two modes are two expectations here, not one: each family's
    reference differs between them somewhere on the table."""
    t, h = _table(), _start()
    for case, ck in (("sgld_grad", COLLECTS[0]), ("sghmc_grad", COLLECTS[0]),
                     ("adam_grad", COLLECTS[0]), ("csghmc_noise", COLLECTS[2]),
                     ("sgld_later", COLLECTS[4])):
        a = _expected(VARIANTS[case], h, t.elem_attr, "true", ck)
        b = _expected(VARIANTS[case], h, t.elem_attr, "recip", ck)
        assert any((a[nm].view(np.int32) != b[nm].view(np.int32)).any() for nm in a), case


# --------------------------------------------------------- per-tensor gradients
def _tensor_state(t, h):
    """The table's state with each tensor's gradient in an allocation of its
    own, read through per-run bases (bdl_step_args.grad_base)."""
    from bayesdll_amd import _lib as L
    grads, rows, bases = [], [], []
    for nm, o, k, a in zip(t.names, t.offsets, t.numels, t.attrs):
        if nm == FROZEN:
            grads.append(None)
            rows.append([o + k, a | L.ATTR_SKIP])
            bases.append(0)
            continue
        g = torch.from_numpy(h["grad"][o:o + k].copy()).to(DEV)
        base = g.data_ptr() - 4 * o
        grads.append(g)
        rows.append([o + k, a | (L.ATTR_GUNALIGNED if base % 16 else 0)])
        bases.append(base)
    st = SimpleNamespace(**vars(t.state()))
    st.grad = None
    st.runs = torch.tensor(rows, dtype=torch.int64, device=DEV)
    st.nruns = len(rows)
    st.gbase = torch.tensor(bases, dtype=torch.int64, device=DEV)
    st.tensor_grads = grads
    return st


@pytest.mark.parametrize("case", ["csghmc_noise", "sgld_later", "sgld_grad", "sghmc", "adam_later"])
def test_per_tensor_gradients_match_the_host_reference(case):
    """One representative per family (and one *_GRAD, which writes the
    per-tensor gradients), true division: the gradient of every tensor read
    from its own allocation, some of them not 16-byte addressable."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    v, t, h = VARIANTS[case], _table(), _start()
    steady = COLLECTS[4] if v.family != "csghmc" else COLLECTS[2]
    try:
        for ck in (COLLECTS[0], steady):
            if not _accepted(v, ck):
                continue
            exp = _expected(v, h, t.elem_attr, "true", ck)
            for geo in GEOMETRIES:
                _load(t, h)
                st = _tensor_state(t, h)
                assert any(int(r[1]) & L.ATTR_GUNALIGNED for r in st.runs.tolist())
                K.set_launch_config(*geo)
                _launch(st, v, "true", ck)
                want_g = exp.get("grad", h["grad"])
                flat_exp = {nm: x for nm, x in exp.items() if nm != "grad"}
                _check(t, h, flat_exp, (case, ck[:2], geo))  # the flat grad vector: not touched
                for nm, o, k, g in zip(t.names, t.offsets, t.numels, st.tensor_grads):
                    if g is not None:
                        _assert_bits(g.cpu().numpy(), want_g[o:o + k], (case, ck[:2], geo, nm))
    finally:
        K.set_launch_config(0, 0, 0)


# ----------------------------------------------------------------- multi-step
@pytest.mark.parametrize("family", ["csghmc", "sgld", "sghmc", "adam"])
def test_three_steps_carry_state_like_the_reference(family):
    """First step, later step with the collect init, later step with the
    steady collect — true division, depth 4; the device state is carried from
    launch to launch (SGD buffer, first_step, Adam's t), as is the reference's,
    each step with its own gradient and noise; bit-exact after every step."""
    from bayesdll_amd import kernels as K
    t, h = _table(), _start()
    st = t.state()
    rng = np.random.default_rng(515)
    base = {"csghmc": "csghmc_noise", "sgld": "sgld_later", "sghmc": "sghmc",
            "adam": "adam_later"}[family]
    welford = family == "csghmc"
    cks = [COLLECTS[0], ("WELFORD_INIT", True, 1.0, 1.0) if welford else ("MEAN_INIT", True, 1.0, 2.0),
           ("WELFORD", True, 3.0, 1.0) if welford else ("MEAN", True, 1.0, 2.0)]
    _load(t, h)
    try:
        K.set_launch_config(1, 4, 1)
        for step, ck in enumerate(cks):
            v = VARIANTS[base]
            over = {}
            if v.mom:
                over.update(first_step=step == 0)
                v = SimpleNamespace(**dict(vars(v), mom="first" if step == 0 else "later"))
            if family == "adam":
                over.update(t=step + 1)
            h["grad"] = (rng.standard_normal(t.n).astype(F) * F(1e-2)).astype(F)
            h["noise"] = rng.standard_normal(t.n).astype(F)
            for nm in ("grad", "noise"):
                t.v[nm].copy_(torch.from_numpy(h[nm]))
            exp = _expected(v, h, t.elem_attr, "true", ck, over)
            _launch(st, v, "true", ck, over)
            _check(t, h, exp, (family, step), _first_buf(v))
            h.update(exp)
    finally:
        K.set_launch_config(0, 0, 0)


# -------------------------------------------------------------------- clipping
@pytest.mark.parametrize("max_norm", [1.0, 1e6], ids=["active", "inactive"])
def test_clipped_sgld_norm_coefficient_and_step(max_norm):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    v, t, h = VARIANTS["sgld_later"], _table(), _start()
    st = t.state()
    live = (t.elem_attr & R.ATTR_SKIP) == 0
    try:
        for mode in MODES:
            sc, _ = _scalars(v, COLLECTS[0])
            gp = R.sgld_grad(h["theta"], h["prior"], h["grad"], t.elem_attr, sc, h["noise"], mode)
            S = float(np.sum(gp[live].astype(np.float64) ** 2))
            norm_ref = F(np.sqrt(S))
            for geo in GEOMETRIES:
                _load(t, h)
                K.set_launch_config(*geo)
                ws = K.sgld_step_clipped(st, max_norm, noise_mode=L.NOISE_BUFFER, div_mode=mode,
                                         **v.kw)
                torch.cuda.synchronize()
                norm, coef = (F(x) for x in ws[:2].cpu().numpy())
                print("clip", mode, geo, float(norm), float(norm_ref), float(coef))
                # 1. one fp32 ulp of fl32(sqrt(S)) (derived in the module docstring)
                assert abs(int(norm.view(np.int32)) - int(norm_ref.view(np.int32))) <= 1, (mode, geo)
                # 2. the coefficient from the device's own norm, bit for bit
                want_coef = R.clip_coef(norm, max_norm)
                assert coef.view(np.int32) == F(want_coef).view(np.int32), (mode, geo)
                assert (coef < 1.0) == (max_norm == 1.0)
                # 3. the step with that coefficient
                exp = _expected(v, h, t.elem_attr, mode, COLLECTS[0], clip_coef=coef)
                _check(t, h, exp, ("clipped", max_norm, mode, geo))
    finally:
        K.set_launch_config(0, 0, 0)


# ---------------------------------------------------------- adversarial values
SUB, TINY, FMIN, BIG, SMALL = F(2.0 ** -149), F(2.0 ** -130), F(2.0 ** -126), F(2.0 ** 60), F(2.0 ** -60)
_VALUES = {
    "theta": [0.0, -0.0, SUB, -SUB, TINY, FMIN, -FMIN, 1.5, SMALL, BIG, -BIG, -0.0173],
    "grad": [0.0, -0.0, SUB, -TINY, FMIN, 1e-2, -SMALL, BIG, -1e-2],
    "mom": [0.0, -0.0, -SUB, TINY, 1e-3, -FMIN, SMALL, -BIG, 3e-4, -1e-3],
    "prior": [0.0, -0.0, SUB, 0.02, -FMIN, BIG, -0.02],
    "noise": [0.0, -0.0, 1.0, -1.0, 0.5, SUB, -2.0, 0.25],
    "m1": [0.0, -0.0, SUB, -TINY, 0.02, BIG, -0.02, FMIN, -SMALL],
    "m2": [0.0, SUB, TINY, 1e-3, FMIN, BIG, SMALL],
    # (no 2^60 here: over adam_v == 0 it would put theta^2 past FLT_MAX in the reference)
    "adam_m": [0.0, -0.0, SUB, -TINY, 1e-3, -FMIN, F(2.0 ** 20), -1e-3, SMALL],
    "adam_v": [0.0, SUB, TINY, 1e-6, FMIN, BIG, SMALL, 1e-6],
    "sgd_buf": [0.0, -0.0, -SUB, TINY, 1e-3, FMIN, -BIG, -1e-3, SMALL, 2e-3, -SMALL],
}


def _adversarial(t):
    """The start vectors with a 4,096-element stretch inside the first tensor
    (fast path) and the last three tensors (guarded path, partial final
    group) overwritten with the special values, each vector cycling through
    its own list (lengths mostly coprime: the combinations vary), plus the
    value relations on every eighth triple of elements."""
    h = _start()
    tail = t.offsets[-3]
    idx = np.concatenate([np.arange(4096, 8192), np.arange(tail, t.n)])
    assert t.numels[0] >= 8192 and t.n - tail == sum(t.numels[-3:])
    k = np.arange(idx.size)
    for nm, vals in _VALUES.items():
        h[nm][idx] = np.array(vals, dtype=F)[k % len(vals)]
    cls = (k // 3) % 8
    h["prior"][idx[cls == 0]] = h["theta"][idx[cls == 0]]
    h["prior"][idx[cls == 1]] = -h["theta"][idx[cls == 1]]
    h["m1"][idx[cls == 2]] = h["theta"][idx[cls == 2]]
    z = idx[cls == 3]
    h["adam_v"][z] = 0.0
    h["grad"][z] = np.where(np.arange(z.size) % 2 == 0, F(0.0), F(-0.0))
    h["prior"][z] = h["theta"][z]
    for nm in ("theta", "grad", "adam_v"):  # the relations and specials are really there
        assert (h[nm][idx] == 0).any() and (np.abs(h[nm][idx]) == SUB).any()
    assert np.signbit(h["grad"][z]).any() and not np.signbit(h["grad"][z]).all()
    assert ((h["adam_v"][idx] == 0) & (h["grad"][idx] == 0)).any()
    assert (h["adam_v"][idx] == SUB).any() and (h["theta"][idx] == h["m1"][idx]).any()
    assert (h["theta"][idx] == -h["prior"][idx]).any() and (np.abs(h["theta"][idx]) == BIG).any()
    return h, idx


_ADVERSARIAL = {
    "csghmc": [("csghmc_noise", COLLECTS[2]), ("csghmc_explore", COLLECTS[0])],
    "sgld": [("sgld_later", COLLECTS[4]), ("sgld_grad", COLLECTS[0]), ("sgld_first", COLLECTS[2])],
    "sghmc": [("sghmc", COLLECTS[4]), ("sghmc_grad", COLLECTS[0])],
    "adam": [("adam_later", COLLECTS[4]), ("adam_csghmc_no_buffer", COLLECTS[3]),
             ("adam_grad", COLLECTS[0])],
}


@pytest.mark.parametrize("family", list(_ADVERSARIAL))
def test_adversarial_values(family):
    """Signed zeros, subnormals, FLT_MIN, theta == +-prior, zero gradients,
    m1 == theta, adam_v == 0 with a zero gradient, 2^+-60: bit equality with
    the reference (whose outputs are finite) at depths 1 and 4, both modes."""
    from bayesdll_amd import kernels as K
    t = _table()
    h, idx = _adversarial(t)
    st = t.state()
    try:
        for case, ck in _ADVERSARIAL[family]:
            v = VARIANTS[case]
            for mode in MODES:
                exp = _expected(v, h, t.elem_attr, mode, ck)
                for nm, x in exp.items():
                    assert np.isfinite(x).all(), (case, mode, nm)
                # the expectation holds a -0 (cSGHMC's v(1-a) - lr * grad_U of zeros is +0)
                assert family == "csghmc" or any(np.signbit(x[idx][x[idx] == 0]).any()
                                                 for x in exp.values()), case
                for geo in ((1, 1, 1), (1, 4, 1)):
                    _load(t, h)
                    K.set_launch_config(*geo)
                    _launch(st, v, mode, ck)
                    _check(t, h, exp, (case, ck[:2], mode, geo), _first_buf(v))
    finally:
        K.set_launch_config(0, 0, 0)


# --------------------------------------------------------- reciprocal fallback
def _odd_divisor(start):
    """A float64 divisor s near `start` for which fl32(1 / fl32(s)) differs
    from fl32(1 / s)."""
    for k in range(1, 2000):
        s = start + k * 0.0137
        if R.Div.fallback(s).inv != R.Div(s).inv:
            return s
    raise AssertionError("no such divisor")


@pytest.mark.parametrize("case", ["sgld_prior", "welford"])
def test_zero_reciprocal_fields_fall_back_to_the_fp32_reciprocal(case):
    """BDL_FLAG_RECIP_DIV with the inv_* fields left 0: the library divides by
    1.0f / fl32(s) (recip_or, include/bdl_sgmcmc.h) — for these divisors not
    the float64-formed reciprocal, and the outputs show it."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    t, h = _table(), _start()
    st = t.state()
    if case == "sgld_prior":
        v, ck = VARIANTS["sgld_first"], COLLECTS[0]  # first step: the buffer is the gradient
        s2, nd = _odd_divisor(0.64), _odd_divisor(7.0)
        over = dict(sigma2=s2, n_data=nd)
        fallback = (("sigma2", s2), ("n_data", nd))
    else:
        v = VARIANTS["csghmc_noise"]
        a = _odd_divisor(3.0)
        ck = ("WELFORD", True, a, 1.0)
        over, fallback = {}, (("ca", a),)
    exp = _expected(v, h, t.elem_attr, "recip", ck, over, fallback)
    plain = _expected(v, h, t.elem_attr, "recip", ck, over)
    assert any((exp[nm].view(np.int32) != plain[nm].view(np.int32)).any() for nm in exp)
    kw = dict(v.kw, **over)
    if ck[0] != "NONE":
        kw.update(collect=L.COLLECT_WELFORD, mom1=st.v["m1"], mom2=st.v["m2"], collect_a=ck[2])
    a = K._step_args(st, getattr(L, v.method), noise_mode=L.NOISE_BUFFER, div_mode="recip", **kw)
    assert a.flags & L.FLAG_RECIP_DIV
    a.inv_sigma2 = a.inv_n_data = a.inv_collect_a = a.inv_collect_b = 0.0
    try:
        for geo in ((1, 1, 1), (1, 4, 1)):
            _load(t, h)
            K.set_launch_config(*geo)
            L.check(L.lib().bdl_sgmcmc_step(a, L.current_stream_handle(st.device)), "step")
            _check(t, h, exp, (case, geo), _first_buf(v))
    finally:
        K.set_launch_config(0, 0, 0)
