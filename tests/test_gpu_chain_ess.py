"""bdl_chain_ess_fold / bdl_chain_ess on the GPU: the accumulators after every
fold and the report's outputs equal the fp32 host reference
(tests/chain_ess_ref.py) bit for bit, a vector a fold does not need and the
padding of a chain slot stay bit-unchanged, the summary's counts, minimum and
argmin equal the reference's exactly and do not depend on the launch geometry,
and the stacked samplers' ess() is those kernels on the thetas they collected."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import chain_ess_ref as R

pytestmark = pytest.mark.gpu

EXACT = ("n_eval", "n_degenerate", "n_nonfinite", "n_below", "ess_min", "argmin")
SENTINEL = -123.25
# (n, grid_blocks): fewer lanes than a workgroup; just under / over one workgroup
# iteration (1024 elements); and, at 8 workgroups (8192 elements an iteration),
# two full grid-stride iterations of every workgroup plus a tail whose last
# group is partial (17411 = 2 * 8192 + 1027 = 4 * 4352 + 3)
SIZES = [(24, 0), (1023, 0), (1025, 0), (17411, 8)]


def bits(a):
    """int32 patterns with every NaN mapped to one pattern (NaN as NaN-ness)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def raw(t):
    return t.cpu().numpy().view(np.int32)


def check_summary(got, want):
    for f in EXACT:
        assert got[f] == want[f], (f, got[f], want[f])
    assert abs(got["ess_sum"] - want["ess_sum"]) <= 1e-12 * abs(want["ess_sum"])


# ---------------------------------------------------------------- the fold
@pytest.mark.parametrize("n,grid", SIZES)
@pytest.mark.parametrize("K_", [1, 5])
@pytest.mark.parametrize("b", [1, 3])
def test_fold_equals_the_fp32_reference_bit_for_bit(b, K_, n, grid):
    """Seven samples: with b = 3 every flag set but b = 1's occurs (first
    sample, mid-batch, the first batch's close, first in batch, a later close)
    and the series ends on an open batch; b = 1 is FIRST_IN_BATCH | CLOSE
    throughout.  The chain slot is wider than n and every lane of every
    accumulator starts as a sentinel: after each fold all four vectors equal
    the reference's whole, so padding lanes and the vectors the fold must not
    touch are unchanged."""
    from bayesdll_amd import kernels as K
    cg = (n + 3) // 4 + 3
    slot = 4 * cg
    rng = np.random.default_rng(1000 * b + 10 * K_ + n)
    acc = R.new_acc(K_ * slot, SENTINEL)
    dev = {nm: torch.from_numpy(v.copy()).cuda() for nm, v in acc.items()}
    seen = set()
    for s in range(1, 8):
        theta = (0.02 + 1e-3 * rng.standard_normal(K_ * slot)).astype(np.float32)
        before = {nm: v.copy() for nm, v in acc.items()}
        flags = R.fold_f32(acc, theta, s, b, chains=K_, chain_groups=cg, n=n)
        seen.add(flags)
        got = K.ess_fold(torch.from_numpy(theta).cuda(), dev["bsum"] if b > 1 else None,
                         dev["smean"], dev["sM2"], dev["bM2"], chains=K_, chain_groups=cg, n=n,
                         sample=s, batch=b, grid_blocks=grid)
        assert got == flags
        for nm in R.VECTORS:
            assert np.array_equal(raw(dev[nm]), acc[nm].view(np.int32)), (s, nm)
        # the reference itself left alone what the fold does not need
        if b == 1:
            assert np.array_equal(acc["bsum"].view(np.int32), before["bsum"].view(np.int32))
        if not flags & R.CLOSE:
            assert np.array_equal(acc["bM2"].view(np.int32), before["bM2"].view(np.int32))
            assert np.array_equal(raw(dev["bM2"]), before["bM2"].view(np.int32))
    pad = np.concatenate([np.arange(slot * k + n, slot * (k + 1)) for k in range(K_)])
    for nm in R.VECTORS:
        assert (dev[nm].cpu().numpy()[pad] == np.float32(SENTINEL)).all(), nm
    if b == 1:
        assert (dev["bsum"].cpu().numpy() == np.float32(SENTINEL)).all()
        assert seen == {15, R.FIRST_IN_BATCH | R.CLOSE}
    else:
        assert seen == {R.FIRST_SAMPLE | R.FIRST_IN_BATCH, 0, R.CLOSE | R.FIRST_BATCH,
                        R.FIRST_IN_BATCH, R.CLOSE}


# -------------------------------------------------------------- the report
def report_case(seed, K_, n, cg):
    """Positive accumulators of K chains with planted elements: degenerate
    (bM2 zero in every chain), NaN and Inf, and the minimum twice."""
    rng = np.random.default_rng(seed)
    slot = 4 * cg
    sM2 = np.full(K_ * slot, np.nan, np.float32)
    bM2 = np.full(K_ * slot, np.nan, np.float32)
    for k in range(K_):
        sM2[slot * k: slot * k + n] = rng.uniform(0.5, 2.0, n) * 1e-3
        bM2[slot * k: slot * k + n] = rng.uniform(0.5, 2.0, n) * 1e-5
    idx = rng.permutation(n)[:8].tolist() if n >= 16 else list(range(8))
    deg, nans, infs, (i, j) = idx[:2], idx[2:4], idx[4:6], idx[6:8]
    for k in range(K_):
        o = slot * k
        bM2[[o + e for e in deg]] = 0.0
        sM2[o + nans[0]] = np.nan if k == K_ - 1 else sM2[o + nans[0]]
        bM2[o + nans[1]] = np.nan if k == 0 else bM2[o + nans[1]]
        sM2[o + infs[0]] = np.inf if k == 0 else sM2[o + infs[0]]
        sM2[o + infs[1]] = np.inf if k == K_ - 1 else sM2[o + infs[1]]
        for e in (i, j):                                   # the same small ESS at i and j
            sM2[o + e] = np.float32(1e-6 * (k + 1))
            bM2[o + e] = np.float32(5e-5)
    return sM2, bM2, deg, nans, infs, (i, j)


@pytest.mark.parametrize("n,grid", SIZES)
@pytest.mark.parametrize("K_", [1, 2, 5, 8])
def test_report_equals_the_fp32_reference_bit_for_bit(K_, n, grid):
    """K = 1, 2, 5, 8: the peeled chain alone, the remainder loop (1 chain), one
    unrolled batch of 4, and a batch plus a remainder of 3.  The slot padding
    holds NaN: it reaches no result."""
    from bayesdll_amd import kernels as K
    cg = (n + 3) // 4 + 3
    sM2, bM2, deg, nans, infs, (i, j) = report_case(77 * K_ + n, K_, n, cg)
    samples, batches = 37, 9
    kw = dict(chains=K_, chain_groups=cg, n=n, samples=samples, batches=batches)
    ess, mcse, summ = R.chain_ess_f32(sM2, bM2, **kw)
    assert np.isnan(ess[deg]).all() and summ["n_degenerate"] == 2
    assert np.isnan(ess[nans]).all() and np.isinf(ess[infs]).all() and summ["n_nonfinite"] == 4
    assert summ["n_eval"] == n - 6 and ess[i] == ess[j] == summ["ess_min"]
    assert summ["argmin"] == min(i, j)
    d1, d2 = torch.from_numpy(sM2).cuda(), torch.from_numpy(bM2).cuda()
    seen = []
    for g in sorted({grid, 0, 3}):
        res = K.chain_ess(d1, d2, want=("ess", "mcse"), grid_blocks=g, **kw)
        assert res["ess"].shape == res["mcse"].shape == (n,)
        assert np.array_equal(bits(res["ess"].cpu().numpy()), bits(ess)), g
        assert np.array_equal(bits(res["mcse"].cpu().numpy()), bits(mcse)), g
        check_summary(res.summary, summ)
        seen.append({f: res.summary[f] for f in EXACT})
    assert all(s == seen[0] for s in seen)                 # independent of the geometry
    assert np.array_equal(raw(d1), sM2.view(np.int32)) and np.array_equal(raw(d2), bM2.view(np.int32))
    # thresholds: a value on a threshold is not below it
    srt = np.sort(ess[np.isfinite(ess)])
    thr = tuple(float(srt[int(q * srt.size)]) for q in (0.1, 0.5, 0.9))
    want = R.chain_ess_f32(sM2, bM2, thresholds=thr, **kw)[2]
    res = K.chain_ess(d1, d2, thresholds=thr, **kw)
    assert list(res) == []
    check_summary(res["summary"], want)
    for t, below in zip(thr, want["n_below"]):
        assert below == int((srt < np.float32(t)).sum())
    # chains = 1 on chain k's slice: that chain alone
    slot = 4 * cg
    for k in sorted({0, K_ - 1}):
        e1, m1, s1 = R.chain_ess_f32(sM2[slot * k:], bM2[slot * k:], **dict(kw, chains=1))
        res = K.chain_ess(d1[slot * k:], d2[slot * k:], want=("ess", "mcse"), **dict(kw, chains=1))
        assert np.array_equal(bits(res["ess"].cpu().numpy()), bits(e1)), k
        assert np.array_equal(bits(res["mcse"].cpu().numpy()), bits(m1)), k
        check_summary(res.summary, s1)


def test_report_with_nothing_evaluated_keeps_the_empty_conventions():
    from bayesdll_amd import kernels as K
    n, K_, cg = 1025, 3, 260
    sM2 = torch.full((K_ * 4 * cg,), 2.0, device="cuda")
    bM2 = torch.zeros(K_ * 4 * cg, device="cuda")
    res = K.chain_ess(sM2, bM2, chains=K_, chain_groups=cg, n=n, samples=8, batches=4,
                      want=("ess", "mcse"))
    s = res.summary
    assert (s["n_eval"], s["n_degenerate"], s["n_nonfinite"]) == (0, n, 0)
    assert (s["ess_min"], s["argmin"], s["ess_sum"], s["n_below"]) == (0.0, -1, 0.0, [0, 0, 0])
    assert torch.isnan(res["ess"]).all() and (res["mcse"] == 0).all()


# ---------------------------------------------------------------- samplers
class Net(nn.Module):
    readout_name = "head"

    def __init__(self):  # 13*7+7+7*5+5 = 138: n % 4 != 0, stride 140
        super().__init__()
        self.body = nn.Linear(13, 7)
        self.head = nn.Linear(7, 5)

    def forward(self, x):
        return self.head(torch.tanh(self.body(x)))


def _args(**extra):
    a = SimpleNamespace(
        lr=5e-2, lr_head=1e-1, epochs=2, num_cycles=2, proportion_exploration=0.5, ND=144,
        device="cuda", seed=7, momentum=0.5,
        hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0, "nd": 1.0,
                 "thin": 1, "nst": 2, "bias": "informative", "burnin": 0})
    for k, v in extra.items():
        setattr(a, k, v)
    return a


@pytest.fixture(scope="module")
def loader():
    g = torch.Generator().manual_seed(8)
    xs, ys = torch.randn(144, 13, generator=g), torch.randint(0, 5, (144,), generator=g)
    return [(xs[i:i + 16].cuda(), ys[i:i + 16].cuda()) for i in range(0, 144, 16)]   # 9 batches


def record_collects(S):
    """(collect kind, theta after the step) of every step that carried a collect spec."""
    log, orig = [], S.step

    def step(x, y, *a, **kw):
        r = orig(x, y, *a, **kw)
        if kw.get("collect") is not None:
            log.append((kw["collect"][0], S.state.theta.cpu().numpy().copy()))
        return r

    S.step = step
    return log


def reference_acc(S, thetas, b):
    st = S.state
    acc = R.new_acc(st.n, 0.0)
    for s, th in enumerate(thetas):
        R.fold_f32(acc, th, s + 1, b, chains=S.K, chain_groups=st.chain_groups, n=st.n1)
    return acc


def owned(S):
    st = S.state
    t = {"theta": st.theta, "mom": st.mom, "m1": getattr(S, "m1", None),
         "m2": getattr(S, "m2", None)}
    if hasattr(S, "mom1"):
        t.update({f"mom1[{c}]": v for c, v in S.mom1.items()})
        t.update({f"mom2[{c}]": v for c, v in S.mom2.items()})
    return {k: v.clone() for k, v in t.items() if v is not None}


def assert_acc_equal(S, acc, b):
    names = R.VECTORS if b > 1 else R.VECTORS[1:]
    assert set(S._ess[0]) == set(names)
    for nm in names:
        assert np.array_equal(raw(S._ess[0][nm]), acc[nm].view(np.int32)), nm


def test_sgld_end_to_end_and_the_feature_writes_nothing_the_sampler_owns(loader):
    from bayesdll_amd import stacked

    def run(ess_batch):
        torch.manual_seed(21)
        S = stacked.StackedSGLD(Net().cuda(), 3, _args(), init="reinit", seed=4, chain0=2,
                                graph=False, ess_batch=ess_batch)
        log = record_collects(S)
        S.train_one_epoch(loader, 0)                       # burnin = 0: every step collects
        return S, log

    S, log = run(2)
    assert len(log) == 9 and S.cnt == 10                   # the burn-in seed is not a fold
    assert S._ess[1] == 9
    acc = reference_acc(S, [th for _, th in log], 2)
    assert_acc_equal(S, acc, 2)
    st = S.state
    before = owned(S)
    d = S.ess(ess=True, mcse=True)
    ess, mcse, summ = R.chain_ess_f32(acc["sM2"], acc["bM2"], chains=3,
                                      chain_groups=st.chain_groups, n=st.n1, samples=9, batches=4)
    assert np.array_equal(bits(d["ess"].cpu().numpy()), bits(ess))
    assert np.array_equal(bits(d["mcse"].cpu().numpy()), bits(mcse))
    check_summary(d, summ)
    assert (d["samples"], d["batches"], d["batch"], d["chains"], d["component"]) == (9, 4, 2, 3, 0)
    assert d["ess_mean"] == d["ess_sum"] / d["n_eval"] and d["thresholds"] == [100.0, 400.0, 1000.0]
    assert d["argmin_param"] == S.param_of(summ["argmin"]) and d["argmin_param"] in st.names
    assert set(S.ess()) & {"ess", "mcse"} == set()
    per = S.ess(by_chain=True, ess=True)
    assert len(per) == 3
    for k, r in enumerate(per):
        o = st.stride * k
        e1, _, s1 = R.chain_ess_f32(acc["sM2"][o:], acc["bM2"][o:], chains=1,
                                    chain_groups=st.chain_groups, n=st.n1, samples=9, batches=4)
        assert np.array_equal(bits(r["ess"].cpu().numpy()), bits(e1)) and r["chains"] == 1
        check_summary(r, s1)
    after = owned(S)
    for k in before:
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
    # the same run without the feature: the sampler's own state is bit-identical
    S0, log0 = run(0)
    assert S0._ess is None and len(log0) == 9
    mine, theirs = owned(S), owned(S0)
    assert mine.keys() == theirs.keys()
    for k in mine:
        assert torch.equal(mine[k].view(torch.int32), theirs[k].view(torch.int32)), k
    with pytest.raises(ValueError, match="ess_batch=0"):
        S0.ess()


def test_csghmc_restarts_at_a_cycles_init_collect(loader):
    """Two cycles (one epoch each), b = 3: after the second the accumulators
    hold the second cycle's samples only; the first cycle's open batch is gone."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import stacked
    torch.manual_seed(22)
    S = stacked.StackedCSGHMC(Net().cuda(), 3, _args(), init="reinit", seed=5, graph=False,
                              ess_batch=3)
    log = record_collects(S)
    S.train_one_epoch(loader, 0)
    first = len(log)
    assert first >= 4 and first % 3 != 0 and log[0][0] == L.COLLECT_WELFORD_INIT
    assert_acc_equal(S, reference_acc(S, [th for _, th in log], 3), 3)
    S.train_one_epoch(loader, 1)
    inits = [i for i, (kind, _) in enumerate(log) if kind == L.COLLECT_WELFORD_INIT]
    assert inits == [0, first]
    second = [th for _, th in log[first:]]
    assert S._ess[1] == len(second) and len(S.mom1) == 2
    comp = S._latest_component()
    assert comp == max(S.mom1)
    acc = reference_acc(S, second, 3)
    assert_acc_equal(S, acc, 3)
    st = S.state
    if len(second) // 3 >= 2:
        d = S.ess()
        summ = R.chain_ess_f32(acc["sM2"], acc["bM2"], chains=3, chain_groups=st.chain_groups,
                               n=st.n1, samples=len(second), batches=len(second) // 3)[2]
        check_summary(d, summ)
        assert d["component"] == comp
    else:
        with pytest.raises(ValueError, match=f"{len(second)} samples folded"):
            S.ess()


def test_csghmc_per_chain_reports_every_chain_alone(loader):
    from bayesdll_amd import stacked
    torch.manual_seed(23)
    S = stacked.StackedCSGHMC(Net().cuda(), 3, _args(), init="reinit", seed=6, graph=False,
                              ess_batch=2, per_chain={"lr": [2e-2, 5e-2, 8e-2]})
    log = record_collects(S)
    S.train_one_epoch(loader, 0)
    nsamp = len(log)
    assert nsamp >= 4
    acc = reference_acc(S, [th for _, th in log], 2)
    assert_acc_equal(S, acc, 2)
    with pytest.raises(ValueError, match="by_chain"):
        S.ess()
    st = S.state
    per = S.ess(by_chain=True, ess=True, mcse=True)
    assert len(per) == 3
    for k, r in enumerate(per):
        o = st.stride * k
        e1, m1, s1 = R.chain_ess_f32(acc["sM2"][o:], acc["bM2"][o:], chains=1,
                                     chain_groups=st.chain_groups, n=st.n1, samples=nsamp,
                                     batches=nsamp // 2)
        assert np.array_equal(bits(r["ess"].cpu().numpy()), bits(e1)), k
        assert np.array_equal(bits(r["mcse"].cpu().numpy()), bits(m1)), k
        check_summary(r, s1)
        assert (r["samples"], r["batches"], r["chains"]) == (nsamp, nsamp // 2, 1)


def test_load_ckpt_empties_the_accumulators(loader, tmp_path):
    from bayesdll_amd import stacked
    torch.manual_seed(24)
    S = stacked.StackedSGLD(Net().cuda(), 2, _args(), init="reinit", seed=4, graph=False,
                            ess_batch=2)
    S.train_one_epoch(loader[:5], 0)
    assert S.ess()["samples"] == 5
    path = S.save_ckpt(str(tmp_path / "ck.pt"))
    S.load_ckpt(path)
    with pytest.raises(ValueError, match="nothing is folded yet"):
        S.ess()
    log = record_collects(S)
    S.train_one_epoch(loader[5:8], 1)
    with pytest.raises(ValueError, match="3 samples folded per chain close 1 batch of 2"):
        S.ess()
    S.train_one_epoch(loader[8:], 1)
    d = S.ess()
    assert (d["samples"], d["batches"]) == (4, 2)
    acc = reference_acc(S, [th for _, th in log], 2)       # a first sample again, old sums gone
    assert_acc_equal(S, acc, 2)


def test_train_reports_ess_only_when_asked(loader):
    from bayesdll_amd import stacked

    class Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(msg)

    log = Log()
    torch.manual_seed(25)
    S = stacked.StackedSGLD(Net().cuda(), 3, _args(), init="reinit", seed=4, logger=log,
                            graph=False, ess_batch=8)
    hist = S.train(loader, test_loader=loader[:2])
    el = [ln for ln in log.lines if "ESS" in ln]
    assert len(el) == 2 and "1 batch of 8" in el[0]        # 9 samples: one closed batch
    assert "ess" not in hist[0] and hist[1]["ess"]["samples"] == 18
    assert hist[1]["ess"]["batches"] == 2 and "2 batches of 8" in el[1]
    assert not any(isinstance(v, torch.Tensor) for v in hist[1]["ess"].values())
