"""The host reference of the posterior draw and the stand-alone moment update
(tests/draw_ref.py) checked on its own, and what the GPU tests' size table
reaches proven on the CPU.  No GPU: test_gpu_draw_instances.py compares the
kernels with this reference.

* draw / moments against float64 evaluation of the textbook formulas on
  well-conditioned inputs.  Every bound is (1 + 2^-24)^k - 1 (k * 2^-24 to
  first order) times the magnitude of the operands, k the number of fp32
  roundings on the longest path into the output, counted at each use.
* moments bit-equal to the golden-pinned torch-CPU oracle's moment updates
  (true division), the draw's variance bit-equal to the oracle's.
* the loop-shape classifier on hand-counted launches, then the size table at
  256 and 304 compute units at every geometry the GPU tests use.
* the parametrised instance lists equal everything pick_sample / pick_moments
  can return.
"""
import itertools

import numpy as np
import pytest
import torch

import draw_ref as DR
import step_ref as R
import test_step_ref as S
from oracle import sgmcmc_oracle as O

F = np.float32
U = 2.0 ** -24
N = 20000


def g(k):
    """The relative error of k successive fp32 roundings."""
    return (1.0 + U) ** k - 1.0


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.int32)


def _rng(tag):
    return np.random.default_rng([23, tag])


def _inputs(tag):
    r = _rng(tag)
    m1 = (0.5 * r.standard_normal(N)).astype(F)
    v = r.uniform(0.5, 2.0, N)
    eps = r.standard_normal(N).astype(F)
    return m1, v, eps


# ------------------------------------------------------------ draw vs float64
@pytest.mark.parametrize("mode", ["true", "recip"])
@pytest.mark.parametrize("var_mode", [DR.VAR_GIVEN, DR.VAR_WELFORD, None])
def test_draw_without_a_difference_against_float64(var_mode, mode):
    """Roundings into out = m1 + sqrt(var) * eps, relative to |m1| + |t|:
    GIVEN / no m2: sqrt, product, sum = 3.  WELFORD: the quotient (true) or
    the reciprocal and the product (recip) — 1 or 2, halved by the square
    root, counted as 1 — then sqrt, product, sum = 4."""
    m1, v, eps = _inputs(1)
    ratio, floor = 7.0, 1e-12
    inv = float(DR.D.inv_of(ratio)) if mode == "recip" else 0.0
    if var_mode is None:
        m2, k = None, 3
        var64 = np.full(N, float(R.f32(floor)))
        got = DR.draw(m1, None, eps, var_mode=DR.VAR_WELFORD, ratio=ratio, inv_ratio=inv,
                      var_floor=floor)
    else:
        m2 = (v * (ratio if var_mode == DR.VAR_WELFORD else 1.0)).astype(F)
        var64 = m2.astype(np.float64) / (ratio if var_mode == DR.VAR_WELFORD else 1.0)
        k = 4 if var_mode == DR.VAR_WELFORD else 3
        got = DR.draw(m1, m2, eps, var_mode=var_mode, ratio=ratio, inv_ratio=inv, var_floor=floor)
    t64 = np.sqrt(var64) * eps.astype(np.float64)
    want = m1.astype(np.float64) + t64
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= g(k) * (np.abs(m1.astype(np.float64)) + np.abs(t64)))
    assert err.max() > 0  # fp32 arithmetic, not the float64 formula cast down


def test_raw_moments_draw_against_float64():
    """var = ratio * (q - m*m) forms a difference: m*m, the difference and the
    product by the ratio are 3 roundings relative to the operands q + m*m (not
    to the result).  Through the square root the variance's absolute error dv
    becomes at most dv / sqrt(var) (dv < var / 2 here: asserted), then the
    square root, the product and the sum round once each."""
    m1, v, eps = _inputs(2)
    ratio = 1.25
    m64 = m1.astype(np.float64)
    q = (m64 * m64 + v / ratio).astype(F)
    got = DR.draw(m1, q, eps, var_mode=DR.VAR_RAW_MOMENTS, ratio=ratio, var_floor=1e-12)
    q64, e64 = q.astype(np.float64), np.abs(eps.astype(np.float64))
    var64 = ratio * (q64 - m64 * m64)
    assert np.all(var64 > 0.3)
    dv = ratio * g(3) * (q64 + m64 * m64)
    assert np.all(dv < var64 / 2)
    s64 = np.sqrt(var64)
    ds = dv / s64 + g(1) * (s64 + dv / s64)
    dt = e64 * ds + g(1) * e64 * (s64 + ds)
    t64 = s64 * eps.astype(np.float64)
    bound = dt + g(1) * (np.abs(m64) + np.abs(t64) + dt)
    err = np.abs(got.astype(np.float64) - (m64 + t64))
    assert np.all(err <= bound) and err.max() > 0
    # the clamp: a negative variance and one below the floor give the floor
    low = DR.draw(np.array([3.0, 0.0], F), np.array([8.0, 1e-20], F), np.array([1.0, 1.0], F),
                  var_mode=DR.VAR_RAW_MOMENTS, ratio=ratio, var_floor=1e-12)
    s = np.sqrt(R.f32(1e-12))
    assert np.array_equal(_bits(low), _bits(np.array([F(3.0) + s, s], F)))


def test_draw_division_modes_and_nan():
    m1, v, eps = _inputs(3)
    q = (v * 7.0).astype(F)
    kw = dict(var_mode=DR.VAR_WELFORD, ratio=7.0, var_floor=1e-12)
    a = DR.draw(m1, q, eps, inv_ratio=0.0, **kw)
    b = DR.draw(m1, q, eps, inv_ratio=DR.D.inv_of(7.0), **kw)
    assert 0 < int((_bits(a) != _bits(b)).sum()) < N
    # NaN stays NaN: a NaN second moment, and a NaN floor without a second moment
    x = DR.draw(np.zeros(2, F), np.array([np.nan, 4.0], F), np.ones(2, F), var_mode=DR.VAR_GIVEN)
    assert np.isnan(x[0]) and x[1] == 2.0
    assert np.isnan(DR.draw(np.zeros(1, F), None, np.ones(1, F), var_mode=DR.VAR_GIVEN,
                            var_floor=np.nan))[0]


# --------------------------------------------------------- moments vs float64
@pytest.mark.parametrize("mode", ["true", "recip"])
def test_welford_update_against_float64(mode):
    """With S = |x| + |m1| (the operands of the differences; ca >= 1):
    n1 = m1 + (x - m1) / ca: difference, quotient (recip: the reciprocal's own
    rounding too), sum = 3 (4) roundings relative to S.
    M2 = q + d * d2: d is 1 rounding, d2 = x - n1 carries n1's 3 (4) plus its
    own, the product and the sum one each = 7 (8) relative to |q| + S * S."""
    r = _rng(4)
    x, m1 = (r.standard_normal(N).astype(F) for _ in range(2))
    q = r.uniform(0.0, 4.0, N).astype(F)
    ca = 7.0
    k1 = 3 if mode == "true" else 4
    n1, n2 = DR.moments(DR.WELFORD, x, m1, q, ca, 1.0, mode)
    x64, m64, q64 = (a.astype(np.float64) for a in (x, m1, q))
    w1 = m64 + (x64 - m64) / ca
    w2 = q64 + (x64 - m64) * (x64 - w1)
    Sop = np.abs(x64) + np.abs(m64)
    e1, e2 = np.abs(n1 - w1), np.abs(n2 - w2)
    assert np.all(e1 <= g(k1) * Sop) and e1.max() > 0
    assert np.all(e2 <= g(k1 + 4) * (q64 + Sop * Sop)) and e2.max() > 0
    only1, none = DR.moments(DR.WELFORD, x, m1, None, ca, 1.0, mode)
    assert none is None and np.array_equal(_bits(only1), _bits(n1))
    # x == m1: the mean is kept and M2 gains exactly +0
    k1_, k2_ = DR.moments(DR.WELFORD, m1, m1, q, ca, 1.0, mode)
    assert np.array_equal(_bits(k1_), _bits(m1)) and np.array_equal(_bits(k2_), _bits(q))


@pytest.mark.parametrize("mode", ["true", "recip"])
def test_running_mean_against_float64(mode):
    """(x + ca * m) / cb: product, sum, quotient = 3 roundings (recip: the
    reciprocal's too, 4) relative to (|x| + ca * |m|) / cb; the second moment
    likewise with x * x and ca * q rounded side by side: 3 (4) relative to
    (x * x + ca * |q|) / cb."""
    r = _rng(5)
    x, m1 = (r.standard_normal(N).astype(F) for _ in range(2))
    q = r.uniform(0.0, 4.0, N).astype(F)
    ca, cb = 6.0, 7.0
    k = 3 if mode == "true" else 4
    n1, n2 = DR.moments(DR.MEAN, x, m1, q, ca, cb, mode)
    x64, m64, q64 = (a.astype(np.float64) for a in (x, m1, q))
    e1 = np.abs(n1 - (x64 + ca * m64) / cb)
    e2 = np.abs(n2 - (x64 * x64 + ca * q64) / cb)
    assert np.all(e1 <= g(k) * (np.abs(x64) + ca * np.abs(m64)) / cb) and e1.max() > 0
    assert np.all(e2 <= g(k) * (x64 * x64 + ca * q64) / cb) and e2.max() > 0
    assert DR.moments(DR.MEAN, x, m1, None, ca, cb, mode)[1] is None


def test_init_kinds_read_no_moment_and_the_modes_differ():
    """The INIT kinds copy x (exact) and store 0 or x * x (1 rounding); they
    do not read the old moments.  At divisor 7 the two division modes differ
    on random data, and the reciprocal formed from the rounded divisor
    (Div.fallback) differs from the host's for a divisor fp32 cannot hold."""
    r = _rng(6)
    x = r.standard_normal(N).astype(F)
    nan = np.full(N, np.nan, F)
    for mode in ("true", "recip"):
        a1, a2 = DR.moments(DR.WELFORD_INIT, x, nan, nan, 7.0, 7.0, mode)
        b1, b2 = DR.moments(DR.MEAN_INIT, x, nan, nan, 7.0, 7.0, mode)
        assert np.array_equal(_bits(a1), _bits(x)) and np.array_equal(_bits(b1), _bits(x))
        assert np.array_equal(_bits(a2), _bits(np.zeros(N, F)))
        assert np.all(np.abs(b2 - x.astype(np.float64) ** 2) <= g(1) * x.astype(np.float64) ** 2)
        assert DR.moments(DR.MEAN_INIT, x, nan, None, 7.0, 7.0, mode)[1] is None
    m1, q = r.standard_normal(N).astype(F), r.uniform(0, 4, N).astype(F)
    for kind, ca, cb in ((DR.WELFORD, 7.0, 1.0), (DR.MEAN, 6.0, 7.0)):
        t, c = (DR.moments(kind, x, m1, q, ca, cb, mode) for mode in ("true", "recip"))
        assert (_bits(t[0]) != _bits(c[0])).any() and (_bits(t[1]) != _bits(c[1])).any()
    assert R.Div.fallback(4.9).inv != R.Div(4.9).inv
    f = DR.moments(DR.WELFORD, x, m1, q, R.Div.fallback(4.9), 1.0, "recip")
    h = DR.moments(DR.WELFORD, x, m1, q, 4.9, 1.0, "recip")
    assert (_bits(f[0]) != _bits(h[0])).any()


# ---------------------------------------------------------------- the oracle
def test_moments_match_the_oracle_in_true_division():
    """The Runner loops of the torch-CPU oracle (pinned to the upstream
    goldens): SGLD's running means over three steps, cSGHMC's cycle init and
    one Welford update, replayed through draw_ref.moments on the oracle's own
    parameter vectors, bit for bit."""
    out = S._simulate(S._cfg("sgld", "informative", momentum=S.MU))
    m1, m2 = DR.moments(DR.MEAN_INIT, out["theta"][0], None, np.zeros(0, F), 1.0, 1.0, "true")
    for t in range(3):
        m1, m2 = DR.moments(DR.MEAN, out["theta"][t + 1], m1, m2, float(t + 1), float(t + 2), "true")
    S._same(m1, out["post_mom1"], "running mean")
    S._same(m2, out["post_mom2"], "running second moment")
    cfg = S._cfg("csghmc", "informative", num_cycles=1, beta=0.5)
    cfg["bpe"] = 4
    out = S._simulate(cfg)
    assert list(out["should_sample"]) == [False, False, True, True]
    m1, m2 = DR.moments(DR.WELFORD_INIT, out["theta"][3], None, np.zeros(0, F), 3.0, 1.0, "true")
    m1, m2 = DR.moments(DR.WELFORD, out["theta"][4], m1, m2, 3.0, 1.0, "true")
    S._same(m1, out["cycle_mom1"][0], "Welford mean")
    S._same(m2, out["cycle_mom2"][0], "Welford M2")


def test_the_draws_variance_matches_the_oracle():
    """sqrt aside (torch-CPU's vectorised fp32 sqrt is not correctly rounded,
    DESIGN §5), the draw's variance is the oracle's, bit for bit."""
    m1, v, _ = _inputs(7)
    q = (m1.astype(np.float64) ** 2 + v / 1.25).astype(F)
    q[::7] = m1[::7] * m1[::7] - F(1e-3)
    tm, tq = torch.from_numpy(m1), torch.from_numpy(q)
    want = O.posterior_variance_raw(tm, tq, 5).numpy()
    got = DR.D.variance_f32(m1, q, DR.VAR_RAW_MOMENTS, R.f32(5 / 4), F(0), R.f32(1e-12))
    S._same(got, want, "raw-moment variance")
    assert (want == R.f32(1e-12)).sum() >= N // 7
    want = O.posterior_variance_welford(tq, 8, tm).numpy()
    got = DR.D.variance_f32(m1, q, DR.VAR_WELFORD, F(7), F(0), R.f32(1e-12))
    S._same(got, want, "Welford variance")
    one = O.posterior_variance_welford(tq, 1, tm).numpy()
    S._same(DR.draw(m1, None, np.ones(N, F), var_mode=DR.VAR_WELFORD) - m1,
            (m1 + np.sqrt(one)) - m1, "single-sample cycle")


# ------------------------------------------------------------ the stacked form
def test_stacked_noise_counts_groups_inside_each_slot():
    calls = []

    def normals(n, seed, chain, step):
        calls.append((n, seed, chain, step))
        return (np.arange(n) + 1000 * (chain % 10)).astype(F)

    K, cg = 3, 5
    eps = DR.stacked_eps(normals, chains=K, chain_groups=cg, seed=9, chain=2 ** 32 - 4, step=11)
    assert calls == [(20, 9, 2 ** 32 - 4 + k, 11) for k in range(K)]
    assert eps.shape == (60,) and eps[20] == 1000 * ((2 ** 32 - 3) % 10) and eps[59] == eps[40] + 19
    m1 = np.arange(60).astype(F)
    out = DR.draw_stacked(m1, None, normals, chains=K, chain_groups=cg, seed=9, chain=2 ** 32 - 4,
                          step=11, var_mode=DR.VAR_GIVEN, var_floor=4.0)
    assert np.array_equal(out, m1 + F(2.0) * eps)  # padding included: every element is drawn
    with pytest.raises(AssertionError):
        DR.draw_stacked(m1[:58], None, normals, chains=K, chain_groups=cg, seed=9, chain=0, step=0,
                        var_mode=DR.VAR_GIVEN)


# ------------------------------------------------------------- the loop shape
def test_classifier_on_hand_counted_launches():
    # 2 CUs x 1, unroll 1: 256 groups (1024 elements) per block iteration
    assert DR.sweep(1, 2, 1, 1) == [(0, (1,))]
    assert DR.sweep(1023, 2, 1, 1) == [(0, (256,))]          # 255 full groups and a partial one
    assert DR.sweep(1024, 2, 1, 1) == [(1, None)]
    assert DR.sweep(1025, 2, 1, 1) == [(1, None), (0, (1,))]
    assert DR.sweep(2048, 2, 1, 1) == [(1, None), (1, None)]
    # five iterations over two workgroups: 0, 2, 4 (a tail of 10 groups) / 1, 3
    assert DR.sweep(4 * 1024 + 37, 2, 1, 1) == [(2, (10,)), (2, None)]
    # unroll 4: 1024 groups per iteration; 1024 + 256 + 38 groups -> one trip, then slots 256, 38, 0, 0
    assert DR.sweep(4 * (1024 + 256 + 37) + 1, 1, 1, 4) == [(1, (256, 38, 0, 0))]
    assert DR.breaks_of((256, 38, 0, 0)) == {1, 2}
    assert DR.breaks_of((256, 256, 256, 256)) == {None}
    assert DR.breaks_of((7, 0, 0, 0)) == {0, 1}  # 249 lanes leave at once, 7 after slot 0
    assert DR.breaks_of((256, 256, 256, 3)) == {3, None}
    assert DR.grid_of(1, 256, 2, 4) == 1 and DR.grid_of(1 << 30, 256, 2, 4) == 512
    for n in (1, 1023, 4133, 99999):
        for cus, bpc, un in ((2, 1, 1), (3, 2, 4)):
            sw = DR.sweep(n, cus, bpc, un)
            done = sum(t for t, _ in sw) * 256 * un + sum(sum(tl) for _, tl in sw if tl)
            assert done == (n + 3) // 4  # every group exactly once


GEOMETRIES = [(1, 1), (1, 4)]  # the draw's; the moment update runs (1, 4)


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("bpc,unroll", GEOMETRIES)
def test_size_table_reaches_what_the_gpu_tests_claim(cus, bpc, unroll):
    sizes = DR.size_table(cus, bpc, unroll)
    kiter, grid = 256 * unroll, cus * bpc
    for n in (1, 3, 4, 5, 4 * kiter - 1, 4 * kiter, 4 * kiter + 1, 4 * kiter * grid):
        assert n in sizes
    sweeps = DR.check_size_table(sizes, cus, bpc, unroll)
    for r in (1, 2, 3):
        n = 2 * 4 * kiter * grid + 4 * kiter * 3 + 4 * (256 + 37) + r
        sw = sweeps[n]
        assert all(t >= 2 for t, _ in sw)
        tails = [(b, tl) for b, (_, tl) in enumerate(sw) if tl is not None]
        if unroll == 4:  # three workgroups take a third trip, the fourth the tail
            assert [t for t, _ in sw[:4]] == [3, 3, 3, 2]
            assert tails == [(3, (256, 38, 0, 0))]
        else:
            assert tails == [(4, (38,))] and [t for t, _ in sw[:5]] == [3, 3, 3, 3, 2]
    if cus == 256:
        assert max(sizes) < 2_200_000
    # at the library's default of 2 workgroups per CU the largest size still
    # sends workgroups through a second trip and one through a tail
    if unroll == 4:
        d = DR.sweep(max(sizes), cus, 2, 4)
        assert any(t >= 2 for t, _ in d) and any(tl is not None for _, tl in d)


def test_size_table_would_notice_a_missing_case():
    sizes = DR.size_table(256, 1, 4)
    with pytest.raises(AssertionError):
        DR.check_size_table([n for n in sizes if n <= 2 * 4 * 1024 * 256], 256, 1, 4)  # no late tail
    with pytest.raises(AssertionError):
        DR.check_size_table([n for n in sizes if n >= 4], 256, 1, 4)


# ------------------------------------------------------------- the instances
def test_instance_lists_are_everything_the_pickers_return():
    """pick_sample's inputs are (var_mode, mom2 given, inv_ratio != 0, noise
    mode, floor >= 2^-96, unroll); sample_instance maps them to the template
    arguments as pick_sample_n does.  The parametrised lists equal the image
    of every accepted input: an instance added to the library must be added
    here, and to the GPU tests with it."""
    raw = itertools.product((DR.VAR_GIVEN, DR.VAR_RAW_MOMENTS, DR.VAR_WELFORD), (True, False),
                            (True, False), (DR.NOISE_BUFFER, DR.NOISE_PHILOX), (True, False), (1, 4))
    image = {DR.sample_instance(*t) for t in raw}
    assert len(DR.DRAW_INSTANCES) == len(set(DR.DRAW_INSTANCES)) == 40
    assert set(DR.DRAW_INSTANCES) == image
    assert len({DR.draw_id(i) for i in DR.DRAW_INSTANCES}) == 40
    raw = itertools.product((DR.WELFORD_INIT, DR.WELFORD, DR.MEAN_INIT, DR.MEAN), (True, False),
                            (True, False))
    assert len(DR.MOMENTS_INSTANCES) == 16
    assert set(DR.MOMENTS_INSTANCES) == {DR.moments_instance(*t) for t in raw}
    assert len({DR.moments_id(i) for i in DR.MOMENTS_INSTANCES}) == 16


def test_instance_lists_match_the_source():
    """The pickers in bdl_api.hip name as many kernel instances as the lists:
    10 bdl_sample_kernel<...> per (noise, floored, unroll) in pick_sample_n
    minus the GIVEN form listed twice (with and without m2: 5 distinct), and
    4 bdl_moments_kernel<...> per collect kind."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "bayesdll_amd", "csrc", "bdl_api.hip")).read()
    forms = set(re.findall(r"return (?:recip \? )?bdl_sample_kernel<([^>]*), NOISE, FL, U>", src)) | \
        set(re.findall(r": bdl_sample_kernel<([^>]*), NOISE, FL, U>", src))
    assert len(forms) == 5, forms
    assert len(forms) * 2 * 2 * 2 == len(DR.DRAW_INSTANCES)
    assert len(set(re.findall(r"bdl_moments_kernel<COLLECT, (\w+, \w+), U>", src))) * 4 == \
        len(DR.MOMENTS_INSTANCES)
