"""The stacked samplers' function-space accumulators on the GPU: they equal, bit
for bit, a replay of kernels.fn_fold over the logits the chains gave on the
probe batch after every collect step; function_space() is the existing R-hat /
ESS kernels on those accumulators (held to chain_diag_ref / chain_ess_ref as
their own tests hold them); the probe perturbs nothing the sampler owns; and
the accumulators empty on function_space_reset() and load_ckpt.  The network
is tests/fakenet's MLP at a small width (FakeNet's logits do not depend on
theta), K = 3 chains, P = 5 probe examples, 10 classes."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chain_diag_ref as D
import chain_ess_ref as E
from fakenet import MLP

pytestmark = pytest.mark.gpu

K_, P, CLASSES, DIM = 3, 5, 10, 13
N = P * CLASSES
CG = (N + 3) // 4


def raw(t):
    return t.cpu().numpy().view(np.int32)


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def net():
    return MLP(input_dim=DIM, output_dim=CLASSES, width=16, depth=2).cuda()


def _args():
    return SimpleNamespace(
        lr=5e-2, lr_head=1e-1, epochs=2, num_cycles=2, proportion_exploration=0.5, ND=192,
        device="cuda", seed=7, momentum=0.5,
        hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0, "nd": 1.0,
                 "thin": 1, "nst": 2, "bias": "informative", "burnin": 0})


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(8)
    xs, ys = torch.randn(192, DIM, generator=g), torch.randint(0, CLASSES, (192,), generator=g)
    loader = [(xs[i:i + 16].cuda(), ys[i:i + 16].cuda()) for i in range(0, 192, 16)]  # 12 steps
    return loader, torch.randn(P, DIM, generator=g)


def record_logits(S, probe):
    """chain_logits(probe) after every step that carried a collect spec."""
    log, orig = [], S.step

    def step(x, y, *a, **kw):
        r = orig(x, y, *a, **kw)
        if kw.get("collect") is not None:
            log.append(S.chain_logits(probe.cuda()).float().contiguous().clone())
        return r

    S.step = step
    return log


def replay(logits, b):
    """kernels.fn_fold over recorded logits into fresh accumulators."""
    from bayesdll_amd import kernels as K
    acc = {nm: torch.zeros(K_ * 4 * CG, device="cuda") for nm in E.VECTORS}
    for s, lg in enumerate(logits):
        K.fn_fold(lg, acc["bsum"] if b > 1 else None, acc["smean"], acc["sM2"], acc["bM2"],
                  sample=s + 1, batch=b, chain_groups=CG)
    return {nm: v for nm, v in acc.items() if b > 1 or nm != "bsum"}


def assert_acc_equal(S, acc):
    assert set(S._fn["acc"]) == set(acc)
    for nm in acc:
        assert np.array_equal(raw(S._fn["acc"][nm]), raw(acc[nm])), nm


def owned(S):
    st = S.state
    t = {"theta": st.theta, "mom": st.mom, "m1": getattr(S, "m1", None),
         "m2": getattr(S, "m2", None)}
    if hasattr(S, "mom1"):
        t.update({f"mom1[{c}]": v for c, v in S.mom1.items()})
        t.update({f"mom2[{c}]": v for c, v in S.mom2.items()})
    return {k: v.clone() for k, v in t.items() if v is not None}


def check_reports(d, acc, samples, b, *, rhat=True):
    """function_space()'s parts against the host references on the accumulators."""
    nb = samples // b
    host = {nm: v.cpu().numpy() for nm, v in acc.items()}
    assert (d["samples"], d["batches"], d["batch"], d["probe"], d["classes"]) == (
        samples, nb, b, P, CLASSES)
    ess, mcse, summ = E.chain_ess_f32(host["sM2"], host["bM2"], chains=K_, chain_groups=CG, n=N,
                                      samples=samples, batches=nb)
    e = d["ess"]
    assert e["ess"].shape == e["mcse"].shape == (P, CLASSES)
    assert np.array_equal(bits(e["ess"].cpu().numpy().ravel()), bits(ess))
    assert np.array_equal(bits(e["mcse"].cpu().numpy().ravel()), bits(mcse))
    for f in ("n_eval", "n_degenerate", "n_nonfinite", "n_below", "ess_min", "argmin"):
        assert e[f] == summ[f], f
    assert abs(e["ess_sum"] - summ["ess_sum"]) <= 1e-12 * abs(summ["ess_sum"])
    assert e["argmin_at"] == divmod(summ["argmin"], CLASSES) and e["chains"] == K_
    assert e["ess_mean"] == e["ess_sum"] / e["n_eval"] and e["thresholds"] == [100.0, 400.0, 1000.0]
    if not rhat:
        assert "rhat" not in d
        return
    _, _, rh, rs = D.chain_diag_f32(host["smean"], host["sM2"], chains=K_, chain_groups=CG, n=N,
                                    var_mode=D.VAR_WELFORD, ratio=float(samples - 1),
                                    inv_ratio=D.inv_of(samples - 1), count=samples)
    r = d["rhat"]
    assert r["rhat"].shape == (P, CLASSES)
    assert np.array_equal(bits(r["rhat"].cpu().numpy().ravel()), bits(rh))
    for f in ("n_eval", "n_degenerate", "n_nonfinite", "n_above", "rhat_max", "argmax"):
        assert r[f] == rs[f], f
    assert abs(r["rhat_sum"] - rs["rhat_sum"]) <= N * 2.0 ** -52 * abs(rs["rhat_sum"])
    assert r["rhat_mean"] == r["rhat_sum"] / r["n_eval"] and r["count"] == samples
    assert r["argmax_at"] == divmod(rs["argmax"], CLASSES)
    assert r["n_eval"] == N and e["n_eval"] == N                   # nothing degenerate here


def test_sgld_accumulators_reports_and_an_unperturbed_chain(data):
    from bayesdll_amd import stacked
    loader, probe = data

    def run(fn):
        torch.manual_seed(21)
        kw = {"fn_probe": probe, "fn_batch": 3} if fn else {}
        S = stacked.StackedSGLD(net(), K_, _args(), init="reinit", seed=4, chain0=2, graph=False,
                                **kw)
        log = record_logits(S, probe)
        S.train_one_epoch(loader, 0)                               # burnin = 0: every step collects
        return S, log

    S, log = run(True)
    assert len(log) == 12 and S._fn["samples"] == 12
    assert (S._fn["probe"], S._fn["classes"], S._fn["chain_groups"]) == (P, CLASSES, CG)
    acc = replay(log, 3)
    assert_acc_equal(S, acc)
    before = owned(S)
    d = S.function_space(rhat=True, ess=True, mcse=True)
    check_reports(d, acc, 12, 3)
    plain = S.function_space()
    assert not any(isinstance(v, torch.Tensor) for part in (plain["rhat"], plain["ess"])
                   for v in part.values())
    thr = S.function_space(thresholds=(1.0, 2.0, 1e9), rhat_thresholds=(1.0, 1.5, 1e9))
    assert thr["ess"]["n_below"][2] == N and thr["rhat"]["n_above"][2] == 0
    assert thr["ess"]["thresholds"] == [1.0, 2.0, 1e9]
    per = S.function_space(by_chain=True, ess=True)
    assert len(per["ess"]) == K_ and "rhat" in per
    for k, r in enumerate(per["ess"]):
        o = 4 * CG * k
        e1, _, s1 = E.chain_ess_f32(acc["sM2"].cpu().numpy()[o:], acc["bM2"].cpu().numpy()[o:],
                                    chains=1, chain_groups=CG, n=N, samples=12, batches=4)
        assert np.array_equal(bits(r["ess"].cpu().numpy().ravel()), bits(e1)) and r["chains"] == 1
        assert r["ess_min"] == s1["ess_min"] and r["argmin"] == s1["argmin"]
    after = owned(S)
    for k in before:                                               # the report writes nothing
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
    # the same run without the probe: theta and the moments are bit-identical
    S0, log0 = run(False)
    assert S0._fn is None and S0._fn_probe is None and len(log0) == 12
    mine, theirs = owned(S), owned(S0)
    assert mine.keys() == theirs.keys()
    for k in mine:
        assert torch.equal(mine[k].view(torch.int32), theirs[k].view(torch.int32)), k
    for a, b in zip(log, log0):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError, match="built without fn_probe"):
        S0.function_space()


def test_csghmc_counts_across_cycles_reset_and_checkpoint(data, tmp_path):
    """Two cycles (one epoch each): unlike ess(), the accumulators run over both.
    Then function_space_reset() and load_ckpt leave them empty, and the next
    fold is a first sample."""
    from bayesdll_amd import stacked
    loader, probe = data
    torch.manual_seed(22)
    S = stacked.StackedCSGHMC(net(), K_, _args(), init="reinit", seed=5, graph=False,
                              fn_probe=probe, fn_batch=2, ess_batch=2)
    log = record_logits(S, probe)
    S.train_one_epoch(loader, 0)
    first = len(log)
    assert first >= 3
    with_ckpt = S.save_ckpt(str(tmp_path / "ck.pt"))
    S.train_one_epoch(loader, 1)
    assert len(S.mom1) == 2 and len(log) > first
    assert S._fn["samples"] == len(log) and S._ess[1] == len(log) - first
    acc = replay(log, 2)
    assert_acc_equal(S, acc)
    check_reports(S.function_space(rhat=True, ess=True, mcse=True), acc, len(log), 2)
    S.function_space_reset()
    with pytest.raises(ValueError, match="nothing is folded yet"):
        S.function_space()
    mark = len(log)
    S.train_one_epoch(loader, 1)
    assert S._fn["samples"] == len(log) - mark > 0
    assert_acc_equal(S, replay(log[mark:], 2))
    S.load_ckpt(with_ckpt)
    assert S._fn["samples"] == 0
    with pytest.raises(ValueError, match="nothing is folded yet"):
        S.function_space()
    mark = len(log)
    S.train_one_epoch(loader, 1)
    acc = replay(log[mark:], 2)                                    # a first sample again
    assert_acc_equal(S, acc)
    samples = len(log) - mark
    if samples >= 4:
        check_reports(S.function_space(rhat=True, ess=True, mcse=True), acc, samples, 2)


def test_per_chain_sweep_reports_every_chain_alone(data):
    from bayesdll_amd import stacked
    loader, probe = data
    torch.manual_seed(23)
    S = stacked.StackedCSGHMC(net(), K_, _args(), init="reinit", seed=6, graph=False,
                              fn_probe=probe, fn_batch=1, per_chain={"lr": [2e-2, 5e-2, 8e-2]})
    log = record_logits(S, probe)
    S.train_one_epoch(loader, 0)
    nsamp = len(log)
    assert nsamp >= 4 and set(S._fn["acc"]) == {"smean", "sM2", "bM2"}   # b = 1: no bsum
    acc = replay(log, 1)
    assert_acc_equal(S, acc)
    with pytest.raises(ValueError, match="by_chain"):
        S.function_space()
    with pytest.raises(ValueError, match="R-hat compares chains"):
        S.function_space(rhat=True, by_chain=True)
    d = S.function_space(by_chain=True, ess=True, mcse=True)
    assert "rhat" not in d and len(d["ess"]) == K_ and d["batches"] == nsamp
    for k, r in enumerate(d["ess"]):
        o = 4 * CG * k
        e1, m1, s1 = E.chain_ess_f32(acc["sM2"].cpu().numpy()[o:], acc["bM2"].cpu().numpy()[o:],
                                     chains=1, chain_groups=CG, n=N, samples=nsamp,
                                     batches=nsamp)
        assert np.array_equal(bits(r["ess"].cpu().numpy().ravel()), bits(e1)), k
        assert np.array_equal(bits(r["mcse"].cpu().numpy().ravel()), bits(m1)), k
        for f in ("n_eval", "n_degenerate", "n_nonfinite", "n_below", "ess_min", "argmin"):
            assert r[f] == s1[f], (k, f)
        assert (r["samples"], r["batches"], r["chains"]) == (nsamp, nsamp, 1)


def test_one_chain_returns_the_ess_part_alone(data):
    from bayesdll_amd import stacked
    loader, probe = data
    torch.manual_seed(24)
    S = stacked.StackedSGLD(net(), 1, _args(), init="reinit", seed=4, graph=False,
                            fn_probe=probe, fn_batch=2)
    S.train_one_epoch(loader[:6], 0)
    d = S.function_space(ess=True)
    assert "rhat" not in d and d["ess"]["ess"].shape == (P, CLASSES) and d["samples"] == 6
    with pytest.raises(ValueError, match="K = 1"):
        S.function_space(rhat=True)


def test_train_reports_the_function_space_line_only_when_asked(data):
    from bayesdll_amd import stacked
    loader, probe = data

    class Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(msg)

    def run(fn):
        log = Log()
        torch.manual_seed(25)
        kw = {"fn_probe": probe, "fn_batch": 8} if fn else {}
        S = stacked.StackedSGLD(net(), K_, _args(), init="reinit", seed=4, logger=log,
                                graph=False, **kw)
        return S.train(loader, test_loader=loader[:2]), log.lines

    hist, lines = run(True)
    fl = [ln for ln in lines if "function space" in ln or "function_space" in ln]
    assert len(fl) == 2 and "close 1 batch of 8" in fl[0]          # 12 samples: one closed batch
    assert "function_space" not in hist[0] and hist[1]["function_space"]["samples"] == 24
    assert "24 samples each, 3 batches of 8" in fl[1] and "R-hat max" in fl[1] and "ESS min" in fl[1]
    fs = hist[1]["function_space"]
    assert not any(isinstance(v, torch.Tensor) for part in (fs["rhat"], fs["ess"])
                   for v in part.values())
    hist0, lines0 = run(False)
    assert all("function_space" not in h for h in hist0)
    # line for line the same log, minus those lines (the epoch's seconds aside)
    strip = lambda ls: [re.sub(r"\(\d+\.\d+ s\)", "", ln) for ln in ls]  # noqa: E731
    assert strip([ln for ln in lines if ln not in fl]) == strip(lines0)
