"""Temperature scaling on the GPU (include/bdl_temper.h): one fit sweep, the
fitted temperature and the report's totals against tests/temper_ref.py within
its derived bounds, over every path of the geometry (wave / workgroup, both
sides of C = 256, C % 4 != 0 on each, the limit; a second grid-stride trip and
a partial last wave or workgroup; 1 and 3 groups), the reference project's
recorded fixtures, the special rows, and the stacked sampler's
fit_temperature() / uncertainty(temperature=...)."""
import os

import numpy as np
import pytest
import torch

import temper_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "calibration.npz"))
INTS = ("n", "n_labelled", "n_nonfinite", "n_wrong")
SUMS = ("nll_sum", "entropy_sum", "confidence_sum")
# (C, N, G, grid_blocks).  N = 4 * grid + 3 at grid 2: a second trip for some
# waves / workgroups and a partial last one; grid 0: the default
SHAPES = [(10, 1, 1, 0), (10, 5, 3, 2), (10, 11, 3, 2), (10, 11, 1, 0), (37, 11, 3, 2), (37, 5, 1, 0),
          (256, 11, 1, 2), (256, 5, 3, 0), (257, 11, 3, 2), (257, 1, 1, 0), (1000, 11, 1, 2),
          (1000, 5, 3, 0), (8192, 3, 1, 0)]
SHARP = (0.6, 1.5, 0.8)   # per group: optima on either side of T = 1


def _group_rows(C, N, G, special):
    zs, lab = [], None
    for g in range(G):
        # (the groups share the labels: group g's rows are drawn around the same labels)
        z, l = R.make_rows(N, C, 100 + C, sharp=SHARP[g], special=special)
        if g:
            rng = np.random.default_rng(900 + g)
            fin = np.isfinite(z)
            z = np.where(fin, z + (0.05 * rng.standard_normal(z.shape)).astype(np.float32), z)
        zs.append(z.astype(np.float32))
        lab = l
    if N == 1:
        # one example has no interior optimum; labelled with its least likely class the optimum
        # is T -> inf, and the fit walks to the lower limit of beta in four clamped steps
        lab = np.array([int(zs[0][0].argmin())], dtype=np.int64)
    return np.stack(zs), lab


def _dev(z, lab):
    return torch.from_numpy(z).cuda().contiguous(), torch.from_numpy(lab).cuda()


def _check_report(tot, z, lab, betas, nb, what):
    rows = tot.read()
    for g, row in enumerate(rows):
        r = R.report_reference(z[g], lab, betas[g], nb)
        assert R.margins(r, nb) > 1, (what, g)        # the bins are decided
        for k in INTS:
            assert int(row[k]) == r[k], (what, g, k)
        assert np.array_equal(row["bin_count"], r["bin_count"]), (what, g)
        assert np.array_equal(row["bin_hits"], r["bin_hits"]), (what, g)
        for k in SUMS:
            if np.isinf(r[k]):      # a -inf at a label: its nll is +inf on both sides
                assert float(row[k]) == r[k], (what, g, k)
                continue
            err = abs(float(row[k]) - r[k])
            print(what, g, k, err, r["b_" + k])
            assert err <= r["b_" + k], (what, g, k, err, r["b_" + k])
        assert (np.abs(row["bin_conf"] - r["bin_conf"]) <= r["b_bin_conf"]).all(), (what, g)
    return rows


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C{}-N{}-G{}-grid{}".format(*s))
def test_fit_and_report_against_the_reference(shape):
    from bayesdll_amd import kernels as K
    C, N, G, grid = shape
    z, lab = _group_rows(C, N, G, special=N >= 8)
    zd, ld = _dev(z, lab)
    # one sweep + update at beta = 1
    one = K.temper_fit(zd, ld, groups=G, max_iter=1, grid_blocks=grid).read()
    for g in range(G):
        s = R.sweep_reference(z[g], lab, 1.0)
        assert (int(one[g]["n"]), int(one[g]["n_nonfinite"]), int(one[g]["n_inf_label"])) == \
            (s["n"], s["n_nonfinite"], s["n_inf_label"]), (g, one[g])
        if s["n"] == 0:
            assert one[g]["degenerate"] and np.isnan(one[g]["nll"])
            continue
        for k, b in (("nll", "b_nll"), ("d1", "b_d1"), ("d2", "b_d2")):
            err = abs(float(one[g][k]) - s[k])
            print(shape, g, k, err, s[b])
            assert err <= s[b], (g, k, err, s[b])
        assert one[g]["sweeps"] == 1 and one[g]["nll_first"] == one[g]["nll"]
    # the whole fit
    st = K.temper_fit(zd, ld, groups=G, grid_blocks=grid)
    rows = st.read()
    temps = st.temperatures().cpu().numpy()
    for g in range(G):
        em = R.newton(z[g], lab)
        if em["degenerate"]:
            assert rows[g]["degenerate"] and not rows[g]["converged"] and rows[g]["beta"] == 1.0
            continue
        fr = R.fit_reference(z[g], lab)
        got = {k: rows[g][k] for k in ("converged", "at_bound", "degenerate", "iterations")}
        print(shape, g, "T", 1.0 / rows[g]["beta"], fr["temperature"], got, em["margin"])
        if em["margin"] > 1:   # no decision of the emulation is within the bound of its threshold
            assert bool(rows[g]["converged"]) == em["converged"]
            assert bool(rows[g]["done"]) == em["done"] and rows[g]["sweeps"] == em["sweeps"]
            assert int(rows[g]["iterations"]) == em["iterations"]
            assert bool(rows[g]["at_bound"]) == em["at_bound"] and not rows[g]["degenerate"]
        if rows[g]["converged"]:
            fit = {"beta": float(rows[g]["beta"])}
            assert abs(1.0 / fit["beta"] - fr["temperature"]) <= R.bound_T(z[g], lab, fit, 1e-6)
            assert temps[g] == np.float32(1.0) / rows[g]["beta"]
            s = R.sweep_reference(z[g], lab, fit["beta"])
            assert abs(float(rows[g]["nll"]) - s["nll"]) <= s["b_nll"]
            assert rows[g]["nll"] <= rows[g]["nll_first"]
    # the report at the fitted temperatures (from the device state), twice into one totals
    nb = 15
    betas = [float(r["beta"]) for r in rows]
    tot = K.temper_report(zd, ld, st, groups=G, num_bins=nb, grid_blocks=grid)
    got = _check_report(tot, z, lab, betas, nb, shape)
    K.temper_report(zd, ld, st, groups=G, totals=tot, num_bins=nb, grid_blocks=grid)
    twice = tot.read()
    for g in range(G):
        assert int(twice[g]["n"]) == 2 * int(got[g]["n"])
        assert np.array_equal(twice[g]["bin_count"], 2 * got[g]["bin_count"])
        assert twice[g]["nll_sum"] == 2 * got[g]["nll_sum"] or np.isinf(got[g]["nll_sum"])
    # integers and bins do not depend on the grid
    other = K.temper_report(zd, ld, st, groups=G, num_bins=nb, grid_blocks=0 if grid else 2).read()
    for g in range(G):
        for k in INTS + ("bin_count", "bin_hits"):
            assert np.array_equal(other[g][k], got[g][k]), (g, k)


def test_groups_converge_at_their_own_pace_and_optimum():
    """Three groups, three optima; group 0 is the fixture at its own optimum
    already (scaled by 1 / T*), so it converges iterations before the others."""
    from bayesdll_amd import kernels as K
    z0, lab = GOLD["c37_vlogits"], GOLD["c37_vlabels"]
    t0 = R.fit_reference(z0, lab)["temperature"]
    z = np.stack([(z0 / np.float32(t0)).astype(np.float32), z0, (3 * z0).astype(np.float32)])
    zd, ld = _dev(z, lab)
    rows = K.temper_fit(zd, ld, groups=3).read()
    its = [int(r["iterations"]) for r in rows]
    print(its, [1 / r["beta"] for r in rows])
    assert all(r["converged"] for r in rows) and its[0] + 2 <= min(its[1:])
    for g in range(3):
        fr = R.fit_reference(z[g], lab)
        fit = {"beta": float(rows[g]["beta"])}
        assert abs(1 / fit["beta"] - fr["temperature"]) <= R.bound_T(z[g], lab, fit, 1e-6)
    assert abs(1 / rows[2]["beta"] - 3 * t0) < 1e-4 and abs(1 / rows[0]["beta"] - 1) < 1e-5


@pytest.mark.parametrize("name", ["c10", "c37"])
def test_golden_fixtures_on_the_device(name):
    from bayesdll_amd import kernels as K
    z, lab = GOLD[name + "_vlogits"], GOLD[name + "_vlabels"]
    zd, ld = _dev(z[None], lab)
    s = K.temper_fit(zd, ld).summary()[0]
    curv = R.curvature_T(z, lab, R.fit_reference(z, lab)["temperature"])
    diff = abs(s["temperature"] - float(GOLD[name + "_topt"][0]))
    print(name, s, diff, 1e-5 / curv)
    assert s["converged"] and not s["at_bound"] and not s["degenerate"] and s["iterations"] <= 8
    assert diff <= 1e-5 / curv
    assert s["nll_after"] < s["nll_before"] and s["n"] == len(lab)
    zt, lt = GOLD[name + "_logits"], GOLD[name + "_labels"]
    ztd, ltd = _dev(zt[None], lt)
    for T in (1.0, 1.7):
        got = K.temper_report(ztd, ltd, T).summary()[0]
        beta = np.float32(1.0 / T)
        r = R.report_reference(zt, lt, beta)
        assert R.margins(r) > 1
        sb, want = R.summary_bound(r), GOLD[f"{name}_analyze_T{T}"]
        # the recorded values are at 1 / T, the device's at fl32(1 / T): a probability moves by
        # at most q |z - E| u beta <= u beta x (the widest row), and so does each of the three
        slack = 0.0 if T == 1.0 else R.U * float(beta) * float((zt.max(-1) - zt.min(-1)).max())
        for k, w in zip(("ece", "mce", "nll"), want):
            print(name, T, k, abs(got[k] - w), sb[k])
            assert abs(got[k] - w) <= sb[k] + slack + 1e-12, (k, got[k], w, sb[k])


def test_special_rows_are_counted_and_change_nothing_else():
    from bayesdll_amd import kernels as K
    for C in (37, 300):
        z, lab = R.make_rows(16, C, 77, sharp=0.7, special=True)
        keep = np.r_[0, 1, 8:16]            # without the six special rows (1 only has a masked class)
        full = K.temper_fit(*_dev(z[None], lab)).read()[0]
        sub = K.temper_fit(*_dev(z[None, keep], lab[keep])).read()[0]
        assert (int(full["n"]), int(full["n_nonfinite"]), int(full["n_inf_label"])) == (10, 3, 1)
        assert (int(sub["n"]), int(sub["n_nonfinite"]), int(sub["n_inf_label"])) == (10, 0, 0)
        assert full["converged"] and full["iterations"] == sub["iterations"]
        # the same examples in another order of the fp64 sum
        assert abs(full["beta"] - sub["beta"]) <= 4 * 2.0 ** -24 * sub["beta"]
        assert abs(full["nll"] - sub["nll"]) <= 1e-12
        rf = K.temper_report(*_dev(z[None], lab), 1.3).read()[0]
        rs = K.temper_report(*_dev(z[None, keep], lab[keep]), 1.3).read()[0]
        # NaN, +inf, all -inf: non-finite; -inf at the label: evaluated, its nll +inf;
        # labels -1 and C: evaluated, unlabelled
        assert (int(rf["n"]), int(rf["n_labelled"]), int(rf["n_nonfinite"])) == (13, 11, 3)
        assert (int(rs["n"]), int(rs["n_labelled"]), int(rs["n_nonfinite"])) == (10, 10, 0)
        assert np.isposinf(rf["nll_sum"]) and np.isfinite(rs["nll_sum"])
        assert np.array_equal(rf["bin_count"] - rs["bin_count"],
                              R.report_reference(z[[5]], lab[[5]], np.float32(1 / 1.3))["bin_count"])


# ------------------------------------------------------------------ the sampler
from test_gpu_chain_diag import Net, _args, loader  # noqa: E402,F401  (loader: a fixture)


def test_sampler_fit_temperature_and_scaled_uncertainty(loader):
    from bayesdll_amd import kernels as K
    from bayesdll_amd import stacked
    torch.manual_seed(23)
    S = stacked.StackedSGLD(Net().cuda(), 2, _args(), init="reinit", seed=4, graph=False)
    S.train_one_epoch(loader, 0)     # past one collect
    val = loader[:2]
    d0 = S.draws
    u0 = S.uncertainty(val)
    d1 = S.draws
    S.draws = d0
    u1 = S.uncertainty(val, temperature=None)
    assert "scaled" not in u0 and u0.keys() == u1.keys()
    np.testing.assert_equal(u0, u1)   # (NaN equals NaN here)
    # the fit is kernels.temper_fit on predict's logp of the same members, batch by batch
    S.draws = d0
    lps, ys, bufs = [], [], {}
    S.net.eval()
    for x, y in val:
        y = y.cuda().to(torch.int64).contiguous()
        outs, _ = K.predict(S._member_logits(x.cuda(), bufs), y, groups=1, want=("logp",))
        lps.append(outs["logp"])
        ys.append(y)
    S.net.train()
    assert S.draws == d1 and len(lps) == 2
    lp, ys = torch.cat(lps, 1).contiguous(), torch.cat(ys)
    assert lp.shape[:2] == (1, len(ys))
    want = K.temper_fit(lp, ys).summary()[0]
    S.draws = d0
    fit = S.fit_temperature(val)
    assert S.draws == d1 and fit == want
    assert fit["converged"] or fit["at_bound"] or fit["degenerate"]
    assert S.temperature_.shape == (1,) and float(S.temperature_[0]) == pytest.approx(
        fit["temperature"], rel=1e-6)
    # on the fitting loader itself the scaled NLL cannot be above the unscaled one
    S.draws = d0
    us = S.uncertainty(val, temperature="fitted")
    assert S.draws == d1
    np.testing.assert_equal({k: v for k, v in us.items() if k != "scaled"}, u0)
    sc = us["scaled"]
    assert set(sc) == {"temperature", "nll", "ece", "mce", "entropy", "confidence"}
    assert sc["temperature"] == fit["temperature"]
    assert sc["nll"] <= us["nll"] + 1e-6 and abs(sc["nll"] - fit["nll_after"]) <= 1e-6
    # T = 1 scales nothing: the report's nll is predict's within fp32 of logp
    S.draws = d0
    one = S.uncertainty(val, temperature=1.0)["scaled"]
    assert abs(one["nll"] - u0["nll"]) <= 1e-5 and abs(one["ece"] - u0["ece"]) <= 1e-5
    # per chain
    S.draws = d0
    fc = S.fit_temperature(val, by_chain=True)
    assert len(fc["temperature"]) == 2 and S.temperature_.shape == (2,)
    S.draws = d0
    uc = S.uncertainty(val, by_chain=True, temperature="fitted")
    assert uc["scaled"]["temperature"] == fc["temperature"] and len(uc["scaled"]["nll"]) == 2
    with pytest.raises(ValueError, match="fitted with by_chain=True"):
        S.uncertainty(val, temperature="fitted")
    with pytest.raises(ValueError, match="the loader is empty"):
        S.fit_temperature([])
    assert not any("temper" in k for k in S.state_dict())
