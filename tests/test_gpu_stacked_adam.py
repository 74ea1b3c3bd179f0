"""StackedAdamSGHMC / StackedAdamCSGHMC and the per-chain clip of the stacked
cyclical samplers (bayesdll_amd.stacked) on the GPU.

As tests/test_gpu_stacked.py: the launches over K stacked chains must equal K
one-chain launches with chain ids chain0 + k bit for bit, given the same
gradients.  With clip_grad, chain k must equal the one-chain *_GRAD launch,
that chain's gradient times the stacked launch's own coef_k, and the one-chain
grad-ready step — each chain clipped by the norm of its own gradient."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chain_clip_ref as R
from test_gpu_stacked import Net

pytestmark = pytest.mark.gpu
K_ = 3
ADAM_VECS = ("adam_m", "adam_v", "sgd_buf")


def _args(epochs=2, clip_grad=None, **hp):
    return SimpleNamespace(
        lr=5e-2, lr_head=1e-1, epochs=epochs, num_cycles=2, proportion_exploration=0.5,
        ND=64, device="cuda", seed=7, momentum=0.5, clip_grad=clip_grad,
        hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 10.0, "nd": 1.0,
                 "thin": 1, "nst": 2, "bias": "informative", "burnin": 0, "beta1": 0.9,
                 "beta2": 0.999, "epsilon": 1e-8, "temperature": 2.0, **hp})


def _make(cls_name, grad_mode, monkeypatch, clip_grad=None, seed=0):
    from bayesdll_amd import stacked
    if grad_mode == "flat":  # force the stacked-gradient-vector fallback
        monkeypatch.setattr(stacked, "MAX_TENSOR_RUNS", 2)
    torch.manual_seed(seed)
    net0 = Net().cuda()
    S = getattr(stacked, cls_name)(Net().cuda(), K_, _args(clip_grad=clip_grad), chain0=4,
                                   init="reinit", net0=net0, graph=False)
    assert S.state.grad_mode == grad_mode and S.state.stride == 140 and S.state.n1 == 138
    # chains start from different momenta too (their gradient norms then differ widely)
    g = torch.Generator().manual_seed(11)
    for k in range(K_):
        S.state.mom2d[k, :138].copy_(torch.randn(138, generator=g) * 0.05 * 4 ** k)
    return S


def _grads(S, step):
    """Prescribed gradients {name: [K, *shape]}: chain k's scaled by 10^(k-1)."""
    g = torch.Generator().manual_seed(100 + step)
    out = {}
    for nm, s in zip(S.state.names, S.state.shapes):
        t = torch.randn(K_, *s, generator=g)
        for k in range(K_):
            t[k] *= 10.0 ** (k - 1)
        out[nm] = t.cuda()
    return out


def _singles(S, adam):
    """K one-chain states holding chain k's theta, prior and momentum."""
    from bayesdll_amd.flat import FlatState
    st = S.state
    segs = [(nm, sh) for nm, sh in zip(st.names, st.shapes)]
    out = []
    for k in range(K_):
        one = FlatState.from_segments(segs, "head", device="cuda", need_mom=True, need_prior=True,
                                      init=st.chain_vector(k).clone(),
                                      extra=ADAM_VECS if adam else ())
        one.prior.copy_(st.prior.view(K_, -1)[k, :st.n1])
        one.mom.copy_(st.mom2d[k, :st.n1])
        for v in one.extra.values():
            v.zero_()
        out.append(one)
    return out


def _bind(S, one, grads, k):
    one.grad.copy_(torch.cat([grads[nm][k].reshape(-1) for nm in S.state.names]))


def _adam_kw(S, k):
    N = S.args.ND * S.Ninflate
    return dict(beta1=S.beta1, beta2=S.beta2, eps=S.epsilon, t=S.t,
                momentum_decay=S.momentum_decay, nd=S.nd, temperature=S.temperature,
                grad_is_mom=S.grad_is_mom, sigma2=S.prior_sig ** 2, n_data=N, seed=S.seed,
                chain=S.chain0 + k, step=S.step_count - 1)


def _chain(vec, k, n1=138):
    return vec.view(K_, -1)[k, :n1]


def _assert_chain_equal(S, one, k, adam, what):
    st = S.state
    assert torch.equal(st.theta2d[k, :st.n1], one.theta), (what, k, "theta")
    assert torch.equal(st.mom2d[k, :st.n1], one.mom), (what, k, "mom")
    if adam:
        for nm in ADAM_VECS:
            if nm in st.extra:
                assert torch.equal(_chain(st.extra[nm], k), one.extra[nm]), (what, k, nm)


# ------------------------------------------------ stacked == one-chain launches
@pytest.mark.parametrize("grad_mode", ["tensor", "flat"])
@pytest.mark.parametrize("cls_name", ["StackedAdamSGHMC", "StackedAdamCSGHMC"])
def test_stacked_adam_launch_equals_one_chain_launches(cls_name, grad_mode, monkeypatch):
    """A first step, a later step and a collect step on prescribed gradients:
    theta, v_mom, adam_m, adam_v, sgd_buf and the moments of every chain equal
    K one-chain K.adam_step launches, bit for bit."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    S = _make(cls_name, grad_mode, monkeypatch)
    cyc = cls_name == "StackedAdamCSGHMC"
    assert S.grad_is_mom == cyc and S.mu == (0.0 if cyc else 0.5) and S.temperature == 2.0
    assert S.tune_method == "adam" and S.clip_grad is None
    singles = _singles(S, True)
    n = S.state.n
    m1, m2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    m1s = [torch.zeros(138, device="cuda") for _ in range(K_)]
    m2s = [torch.zeros(138, device="cuda") for _ in range(K_)]
    plan = [((0.05, 0.1), None), ((0.04, 0.08), None), ((0.03, 0.06), (L.COLLECT_MEAN_INIT, 1.0, 1.0)),
            ((0.02, 0.04), (L.COLLECT_MEAN, 1.0, 2.0))]
    for step, (lrs, col) in enumerate(plan):
        grads = _grads(S, step)
        first = S.mu != 0 and not S.has_buffer
        S.update(grads, lrs, None if col is None else (col[0], m1, m2, col[1], col[2]))
        assert S.t == step + 1 and S.step_count == step + 1
        for k, one in enumerate(singles):
            _bind(S, one, grads, k)
            mom = S.mu != 0
            ckw = {} if col is None else dict(collect=col[0], mom1=m1s[k], mom2=m2s[k],
                                              collect_a=col[1], collect_b=col[2])
            K.adam_step(one, L.ADAM_SGHMC, adam_m=one.extra["adam_m"], adam_v=one.extra["adam_v"],
                        sgd_buf=one.extra["sgd_buf"] if mom else None, lrs=lrs,
                        noise_mode=L.NOISE_PHILOX, mu=S.mu, first_step=first, momentum=mom,
                        **ckw, **_adam_kw(S, k))
    torch.cuda.synchronize()
    assert ("sgd_buf" in S.state.extra) == (not cyc) and S.has_buffer == (not cyc)
    for k, one in enumerate(singles):
        _assert_chain_equal(S, one, k, True, cls_name)
        assert torch.equal(_chain(m1, k), m1s[k]) and torch.equal(_chain(m2, k), m2s[k]), k
    assert not torch.equal(S.state.theta2d[0], S.state.theta2d[1])
    assert torch.count_nonzero(S.state.theta2d[:, 138:]) == 0       # padding never written
    assert torch.count_nonzero(S.state.extra["adam_v"].view(K_, -1)[:, 138:]) == 0
    assert not S.state.diverged()


def _loader(seed=3, n=256, bs=32):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(13, 5, generator=g)
    xs = torch.randn(n, 13, generator=g)
    ys = (xs @ w).argmax(1)
    return [(xs[i:i + bs], ys[i:i + bs]) for i in range(0, n, bs)]


def test_cycle_end_resets_the_adam_state():
    """One epoch = one cycle (epochs = num_cycles = 2): its last step is a
    last_in_cycle step, after which v_mom, m, v and t are zero."""
    from bayesdll_amd import stacked
    torch.manual_seed(1)
    S = stacked.StackedAdamCSGHMC(Net().cuda(), K_, _args(), init="reinit")
    S.update(_grads(S, 0), (0.05, 0.1))
    torch.cuda.synchronize()
    assert S.t == 1 and all(torch.count_nonzero(v) > 0 for v in
                            (S.state.mom, S.state.extra["adam_m"], S.state.extra["adam_v"]))
    S.train_one_epoch(_loader(), 0)
    assert S.t == 0 and S.step_count == 9
    for v in (S.state.mom, S.state.extra["adam_m"], S.state.extra["adam_v"]):
        assert torch.count_nonzero(v) == 0
    assert sorted(S.mom1) == [1] and S.samples_per_cycle[1] == 4


# ----------------------------------------------------------------- clipped step
@pytest.mark.parametrize("grad_mode", ["tensor", "flat"])
@pytest.mark.parametrize("cls_name", ["StackedAdamCSGHMC", "StackedCSGLD"])
def test_clipped_step_clips_every_chain_by_its_own_norm(cls_name, grad_mode, monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    adam = cls_name == "StackedAdamCSGHMC"
    S = _make(cls_name, grad_mode, monkeypatch, clip_grad=1.0)
    singles = _singles(S, adam)
    N = S.args.ND * S.Ninflate
    n = S.state.n
    m1, m2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    m1s = [torch.zeros(138, device="cuda") for _ in range(K_)]
    m2s = [torch.zeros(138, device="cuda") for _ in range(K_)]
    clipped_seen = []
    for step, (lrs, col) in enumerate([((0.05, 0.1), None),
                                       ((0.04, 0.08), (L.COLLECT_MEAN_INIT, 1.0, 1.0))]):
        grads = _grads(S, step)
        keep = {nm: g.clone() for nm, g in grads.items()}
        # the one-chain *_GRAD launches first: their float64 norms set the threshold
        if adam:
            S.t += 1   # (as update will; undone below)
        norms64 = []
        for k, one in enumerate(singles):
            _bind(S, one, keep, k)
            if adam:
                kw = _adam_kw(S, k)
                kw["step"] = S.step_count
                K.adam_step(one, L.ADAM_SGHMC_GRAD, adam_m=one.extra["adam_m"],
                            adam_v=one.extra["adam_v"], lrs=lrs, noise_mode=L.NOISE_PHILOX, **kw)
            else:
                ns = [S.nd * np.sqrt(2 / (N * v)) for v in lrs]
                K.sgmcmc_step(one, L.SGLD_GRAD, lrs=lrs, noise_scale=ns, noise_mode=L.NOISE_PHILOX,
                              prior_sig=S.prior_sig, sigma2=S.prior_sig ** 2, n_data=N,
                              seed=S.seed, chain=S.chain0 + k, step=S.step_count)
            norms64.append(float(one.grad.double().norm()))
        if adam:
            S.t -= 1
        order = sorted(norms64)
        S.clip_grad = 0.5 * (order[0] + order[1])          # exactly K - 1 chains clip
        first = S.mu != 0 and not S.has_buffer
        S.update(grads, lrs, None if col is None else (col[0], m1, m2, col[1], col[2]))
        tab = S.last_clip.cpu().numpy()
        print(cls_name, grad_mode, step, "norms64", norms64, "clip", S.clip_grad, "table", tab)
        assert tab.shape == (K_, 2)
        for k, one in enumerate(singles):
            assert R.within_one_ulp(tab[k, 0], np.float32(norms64[k])), (k, tab[k, 0], norms64[k])
            assert (tab[k, 1] < 1) == (norms64[k] > S.clip_grad), k
            if tab[k, 1] < 1:
                one.grad.mul_(float(tab[k, 1]))            # the stacked launch's own coef_k
            mom = S.mu != 0
            ckw = {} if col is None else dict(collect=col[0], mom1=m1s[k], mom2=m2s[k],
                                              collect_a=col[1], collect_b=col[2])
            K.sgmcmc_step(one, L.SGLD, lrs=lrs, noise_scale=(0.0, 0.0), noise_mode=L.NOISE_NONE,
                          sigma2=1.0, n_data=1.0, grad_ready=True, mu=S.mu, first_step=first,
                          momentum=mom, seed=S.seed, chain=S.chain0 + k, step=S.step_count - 1,
                          mom_buf=one.extra["sgd_buf"] if (adam and mom) else None, **ckw)
        clipped_seen.append(int((tab[:, 1] < 1).sum()))
        torch.cuda.synchronize()
        for k, one in enumerate(singles):
            _assert_chain_equal(S, one, k, adam, (cls_name, step))
    assert clipped_seen == [K_ - 1, K_ - 1]
    for k in range(K_):
        assert torch.equal(_chain(m1, k), m1s[k]) and torch.equal(_chain(m2, k), m2s[k]), k
    assert not S.state.diverged()


@pytest.mark.parametrize("grad_mode", ["tensor", "flat"])
@pytest.mark.parametrize("cls_name", ["StackedAdamCSGHMC", "StackedCSGLD"])
def test_a_clip_that_never_clips_equals_no_clip(cls_name, grad_mode, monkeypatch):
    """clip_grad = 1e30: the *_GRAD / grad-ready pair around a clip whose every
    coefficient is 1 gives the fused step's bits."""
    from bayesdll_amd import _lib as L
    outs = []
    for clip in (None, 1e30):
        S = _make(cls_name, grad_mode, monkeypatch, clip_grad=clip)
        n = S.state.n
        m1, m2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        for step, (lrs, col) in enumerate([((0.05, 0.1), None), ((0.04, 0.08), None),
                                           ((0.03, 0.06), (L.COLLECT_MEAN_INIT, 1.0, 1.0))]):
            S.update(_grads(S, step), lrs, None if col is None else (col[0], m1, m2, *col[1:]))
        torch.cuda.synchronize()
        if clip is not None:
            assert (S.last_clip[:, 1] == 1).all() and S.last_clip[:, 0].isfinite().all()
        else:
            assert S.last_clip is None
        outs.append([S.state.theta.clone(), S.state.mom.clone(), m1, m2]
                    + [v.clone() for _, v in sorted(S.state.extra.items())])
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_no_clip_issues_no_chain_clip_call(monkeypatch):
    from bayesdll_amd import kernels as K
    from bayesdll_amd import stacked
    calls = []
    real = K.chain_clip
    monkeypatch.setattr(K, "chain_clip", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    for cls_name, clip, want in (("StackedAdamCSGHMC", None, 0), ("StackedCSGLD", None, 0),
                                 ("StackedAdamSGHMC", 0.5, 0),   # the plain Runner never clips
                                 ("StackedAdamCSGHMC", 0.5, 2), ("StackedCSGLD", 0.5, 2)):
        del calls[:]
        torch.manual_seed(2)
        S = getattr(stacked, cls_name)(Net().cuda(), K_, _args(clip_grad=clip), init="reinit",
                                       graph=False)
        for step in range(2):
            S.update(_grads(S, step), (0.05, 0.1))
        torch.cuda.synchronize()
        assert len(calls) == want and (S.last_clip is not None) == (want > 0), cls_name


# --------------------------------------------------------------------- training
@pytest.mark.parametrize("cls_name,clip", [("StackedAdamSGHMC", None),
                                           ("StackedAdamCSGHMC", 5.0)])
def test_training_learns_diagnoses_and_resumes_exactly(cls_name, clip, tmp_path):
    """Two short epochs on a separable synthetic problem: the loss falls, the
    stacked predictive evaluates, diagnostics() gives a finite summary, and a
    save_ckpt / load_ckpt continuation after the first epoch ends on the very
    bits of the uninterrupted run."""
    from bayesdll_amd import stacked
    loader = _loader(n=512)

    def make():
        torch.manual_seed(5)
        args = _args(epochs=2, clip_grad=clip, nd=0.1, temperature=1.0)
        lr = 0.2 if clip else 0.05   # p.grad = v_mom ~ lr * pg / a: the cyclical rule moves by lr^2
        args.lr, args.lr_head, args.ND, args.momentum = lr, lr, 512, 0.5
        return getattr(stacked, cls_name)(Net().cuda(), 4, args, init="reinit", seed=5)

    S = make()
    hist = S.train(loader, test_loader=loader)
    first, last = np.array(hist[0]["loss"]), np.array(hist[-1]["loss"])
    print(cls_name, "loss", first, last, "error", hist[-1]["error"])
    assert np.isfinite(last).all() and last.mean() < first.mean()
    nll, err = S.evaluate(loader)
    assert np.isfinite(nll) and err < 0.6      # chance: 0.8
    d = S.diagnostics()
    assert d["n_eval"] + d["n_degenerate"] + d["n_nonfinite"] == 138 and d["n_eval"] > 0
    assert np.isfinite(d["rhat_max"]) and np.isfinite(d["rhat_mean"]) and d["count"] >= 2
    if clip is not None:
        assert "clip" in hist[-1] and 0 <= hist[-1]["clip"]["clipped"] <= 4
        assert np.isfinite(hist[-1]["clip"]["max_norm"])
    assert not S.state.diverged()

    A = make()
    A.train_one_epoch(loader, 0)
    path = A.save_ckpt(str(tmp_path / "stacked.pt"))
    B = make()
    B.load_ckpt(path)
    assert B.t == A.t and B.has_buffer == A.has_buffer and B.step_count == A.step_count
    B.train(loader, start_epoch=1)
    C = make()
    C.train(loader)
    torch.cuda.synchronize()
    assert torch.equal(B.state.theta, C.state.theta) and torch.equal(B.state.mom, C.state.mom)
    for nm, v in C.state.extra.items():
        assert torch.equal(B.state.extra[nm], v), nm
    assert B.t == C.t and B.step_count == C.step_count


def test_cold_restarts_are_refused():
    from bayesdll_amd import stacked
    with pytest.raises(ValueError, match="perform_cold_restarts"):
        stacked.StackedAdamCSGHMC(Net().cuda(), 2, _args(perform_cold_restarts="true"))
    stacked.StackedAdamCSGHMC(Net().cuda(), 2, _args(perform_cold_restarts="false"))
