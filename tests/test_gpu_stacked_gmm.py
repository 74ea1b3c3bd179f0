"""The likelihood-weighted cycle mixture of the stacked cyclical samplers on
the GPU (a 138-parameter net, K = 3, two cycles of one epoch each, eight
batches): score_cycle against per-chain cross-entropy on the same draws with
one host read, component_weights against _runner.gmm_weights, the weighted
evaluate_chains against the reference's formula on the exported means, the
weighted uncertainty, the unweighted paths bit-identical with the option on,
and the checkpoint round trip."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mixture_ref as R
from test_gpu_chain_diag import Net, _args, loader  # noqa: F401  (loader: a fixture)

pytestmark = pytest.mark.gpu

K_ = 3


def _sampler(cls, nst, seed=31, **extra):
    from bayesdll_amd import stacked
    torch.manual_seed(seed)
    args = _args(nst=nst, **extra)
    args.hparams.update(beta1=0.9, beta2=0.999, epsilon=1e-8, temperature=2.0)  # (the Adam one's)
    return getattr(stacked, cls)(Net().cuda(), K_, args, init="reinit", seed=4, chain0=3,
                                 graph=False)


def _views(S, buf):
    st = S.state
    return {nm: buf.view(S.K, st.stride)[:, o:o + k].view(S.K, *s)
            for nm, o, k, s in zip(st.names, st.offsets, st.numels, st.shapes)}


def _count_reads(monkeypatch):
    from bayesdll_amd import kernels as K
    calls, read = [], K.MemberScores.read

    def counted(self):
        calls.append(1)
        return read(self)
    monkeypatch.setattr(K.MemberScores, "read", counted)
    return calls


def _draw_logits(S, c, loader):
    """[draws, K, N, C] logits of cycle c's draws from the current draw counter
    (eval mode), as score_cycle takes them."""
    nd = max(1, S.nst)
    m1, m2, var_mode, ratio, _ = S._moment_spec(c)
    was = S.net.training
    S.net.eval()
    try:
        with torch.no_grad():
            bufs = []
            for _ in range(nd):
                buf = torch.empty_like(S.state.theta)
                if S.nst == 0:
                    buf.copy_(m1)
                else:
                    S._sample(buf, m1, m2, var_mode, ratio)
                bufs.append(_views(S, buf))
            return torch.stack([torch.cat([S._fwd(v, x) for x, _ in loader], 1) for v in bufs], 0)
    finally:
        S.net.train(was)


@pytest.mark.parametrize("cls,nst", [("StackedCSGHMC", 2), ("StackedCSGLD", 0),
                                     ("StackedAdamCSGHMC", 2)])
def test_score_cycle_is_cross_entropy_on_the_same_draws_with_one_host_read(cls, nst, loader,
                                                                           monkeypatch):
    from bayesdll_amd._runner import gmm_weights
    S = _sampler(cls, nst)
    calls = _count_reads(monkeypatch)
    ys = torch.cat([y for _, y in loader])
    for ep in range(2):
        S.train_one_epoch(loader, ep)
        d0 = S.draws
        lik = S.score_cycle(loader)
        assert len(calls) == ep + 1                    # one host read per scored cycle
        d1, S.draws = S.draws, d0
        assert d1 - d0 == nst
        c = S._latest_component()
        lg = _draw_logits(S, c, loader)                # the same draws again
        assert S.draws == d1
        nd, N = max(1, nst), len(ys)
        assert lik.shape == (nd, K_) and lik.dtype == np.float64
        assert lik is S.cycle_likelihoods[c]
        sr = R.score_reference(lg.cpu().numpy(), ys.cpu().numpy())
        assert (sr["n"] == N).all()
        for s in range(nd):
            for k in range(K_):
                ce = F.cross_entropy(lg[s, k].double(), ys, reduction="sum").item()
                want, b = np.exp(-ce / N), sr["b_nll_sum"][s, k] / N
                assert abs(lik[s, k] - want) <= want * np.expm1(b) + 1e-15, (s, k)
    keys = S._component_keys()
    assert sorted(S.cycle_likelihoods) == keys and len(keys) == 2
    w = S.component_weights(by_chain=True)
    assert w.shape == (2, K_) and np.allclose(w.sum(0), 1.0, atol=1e-15)
    for k in range(K_):
        want = gmm_weights({c: list(S.cycle_likelihoods[c][:, k]) for c in keys})
        assert np.array_equal(w[:, k], [want[c] for c in keys])
    j = S.component_weights(by_chain=False)
    assert abs(j.sum() - 1) < 1e-15 and (j > 0).all()
    del S.cycle_likelihoods[keys[0]]
    with pytest.raises(ValueError, match=f"cycle {keys[0]} has not been scored"):
        S.component_weights()


def test_weighted_evaluate_chains_is_the_reference_formula_on_the_exported_means(loader):
    """nst = 0, combine="reference": per chain, log_softmax(sum_c w_c logits_c)
    of its exported cycle means (mixture_evaluate's ops), in float64."""
    S = _sampler("StackedCSGHMC", 0)
    for ep in range(2):
        S.train_one_epoch(loader, ep)
        S.score_cycle(loader)
    w = S.component_weights(by_chain=True)
    ys = torch.cat([y for _, y in loader])
    N = len(ys)
    nll, err = S.evaluate_chains(loader, weights="gmm", combine="reference")
    assert nll.shape == err.shape == (K_,)
    exported = [S.export_chain(k)["cycle_theta_mom1"] for k in range(K_)]
    was = S.net.training
    S.net.eval()
    try:
        with torch.no_grad():
            lg = []
            for c in S._component_keys():
                buf = torch.zeros_like(S.state.theta)
                for k in range(K_):
                    buf.view(S.K, S.state.stride)[k, :S.state.n1].copy_(exported[k][c])
                lg.append(torch.cat([S._fwd(_views(S, buf), x) for x, _ in loader], 1))
            lg = torch.stack(lg, 0)                    # [cycles, K, N, C]
    finally:
        S.net.train(was)
    r = R.mixture_reference(lg.cpu().numpy(), w, 1, "reference")
    lab = ys.cpu().numpy()
    for k in range(K_):
        batch_logits = sum(w[c, k] * lg[c, k].double() for c in (0, 1))
        lp = F.log_softmax(batch_logits, dim=1)
        want = F.nll_loss(lp, ys, reduction="sum").item() / N
        b = r["b_logp"][k][np.arange(N), lab].sum() / N + (2 * N + 4) * 2.0 ** -53 * abs(want)
        assert np.isfinite(b) and abs(nll[k] - want) <= b, (k, nll[k], want, b)
        assert err[k] == lp.argmax(-1).ne(ys).double().mean().item()
    # the arithmetic mode: the log of the weighted mean probability
    nll_a, _ = S.evaluate_chains(loader, weights="gmm")
    ra = R.mixture_reference(lg.cpu().numpy(), w, 1, "arithmetic")
    for k in range(K_):
        want = -ra["logp"][k][np.arange(N), lab].mean()
        assert abs(nll_a[k] - want) <= ra["b_logp"][k][np.arange(N), lab].mean() + 1e-13
    # pooled: (cycle, chain) pairs as the components of one group
    nll_p, err_p = S.evaluate(loader, weights="gmm")
    wj = S.component_weights(by_chain=False)
    rp = R.mixture_reference(lg.cpu().numpy().reshape(2 * K_, 1, N, -1), wj.reshape(-1, 1), 1,
                             "arithmetic")
    want = -rp["logp"][0][np.arange(N), lab].mean()
    assert abs(nll_p - want) <= rp["b_logp"][0][np.arange(N), lab].mean() + 1e-13
    assert err_p == float((rp["logp"][0].argmax(-1) != lab).mean())


def test_weighted_uncertainty_agrees_with_temper_report_and_the_reference(loader):
    from bayesdll_amd import kernels as K
    S = _sampler("StackedCSGLD", 2)
    for ep in range(2):
        S.train_one_epoch(loader, ep)
        S.score_cycle(loader)
    w = S.component_weights(by_chain=True)
    ys = torch.cat([y for _, y in loader])
    N, lab = len(ys), ys.cpu().numpy()
    d0 = S.draws
    u = S.uncertainty(loader, by_chain=True, weights="gmm", num_bins=10)
    d1, S.draws = S.draws, d0
    assert "disagreement" not in u and u["members"] == 4 and u["num_bins"] == 10
    # the same members again, through kernels.mixture and temper_report directly
    bufs, ttot, mtot, lgs = {}, None, None, []
    wdev = torch.from_numpy(w).cuda()
    S.net.eval()
    for x, y in loader:
        lg = S._member_logits(x, bufs)
        lgs.append(lg.cpu().numpy())
        outs, mtot = K.mixture(lg, wdev, y, draws=2, groups=K_, want=K.MIXTURE_OUTPUTS, totals=mtot)
        ttot = K.temper_report(outs["logp"], y, 1.0, groups=K_, totals=ttot, num_bins=10)
    S.net.train()
    assert S.draws == d1
    ts, ms = ttot.summary(), mtot.summary()
    r = R.mixture_reference(np.concatenate(lgs, 2), w, 2, "arithmetic")
    for k in range(K_):
        for f in ("nll", "error", "ece", "mce", "entropy", "confidence", "n"):
            assert u[f][k] == ts[k][f], (f, k)
        assert u["expected_entropy"][k] == ms[k]["expected_entropy"]
        assert u["mutual_info"][k] == u["entropy"][k] - u["expected_entropy"][k]
        want = -r["logp"][k][np.arange(N), lab].mean()
        assert abs(u["nll"][k] - want) <= r["b_logp"][k][np.arange(N), lab].mean() + 1e-13
        assert u["error"][k] == float((r["logp"][k].argmax(-1) != lab).mean())
        t = r["totals"][k]
        assert abs(u["expected_entropy"][k] - t["expected_entropy_sum"] / N) <= r["b_totals"][k] / N
    # fit_temperature on the weighted logp runs and reports per chain
    fit = S.fit_temperature(loader, by_chain=True, weights="gmm")
    assert len(fit["temperature"]) == K_ and all(t > 0 for t in fit["temperature"])


def test_unweighted_results_do_not_change_and_the_checkpoint_round_trip(loader, tmp_path):
    """The option off and on, same seeds: evaluate / evaluate_chains /
    uncertainty with weights=None give the same bits (the draw counter
    restored: the likelihood pass draws, as the reference's does)."""
    off = _sampler("StackedCSGHMC", 2)
    on = _sampler("StackedCSGHMC", 2, gmm_weights=True)
    assert not off.gmm_weights and on.gmm_weights
    hist = on.train(loader, loader)
    for ep in range(2):
        off.train_one_epoch(loader, ep)
    keys = on._component_keys()
    assert sorted(on.cycle_likelihoods) == keys and len(keys) == 2
    assert off.cycle_likelihoods == {}
    for i, rec in enumerate(hist):
        assert {"test", "test_gmm", "gmm_weights"} <= set(rec)
        assert np.isfinite(rec["test_gmm"]).all()
        assert rec["gmm_weights"]["cycles"] == keys[:i + 1]
    assert torch.equal(on.state.theta, off.state.theta)
    res = []
    for S in (off, on):
        S.draws = 1000
        a = S.evaluate(loader)
        b = S.evaluate_chains(loader)
        c = S.uncertainty(loader)
        res.append((a, b, c))
    assert res[0][0] == res[1][0]
    assert all(np.array_equal(p, q) for p, q in zip(res[0][1], res[1][1]))
    assert res[0][2] == res[1][2]
    # the checkpoint keeps cycle_likelihoods with the option, and only then
    assert "cycle_likelihoods" not in off.state_dict()
    p_on, p_off = on.save_ckpt(str(tmp_path / "on.pt")), off.save_ckpt(str(tmp_path / "off.pt"))
    fresh = _sampler("StackedCSGHMC", 2, seed=5, gmm_weights=True)
    fresh.load_ckpt(p_on)
    assert sorted(fresh.cycle_likelihoods) == keys
    for c in keys:
        assert np.array_equal(fresh.cycle_likelihoods[c], on.cycle_likelihoods[c])
    assert np.array_equal(fresh.component_weights(), on.component_weights())
    fresh.load_ckpt(p_off)                             # written without the option: loads
    assert fresh.cycle_likelihoods == {}
    with pytest.raises(ValueError, match=f"cycle {keys[0]} has not been scored"):
        fresh.evaluate_chains(loader, weights="gmm")
