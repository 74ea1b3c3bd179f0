"""bf16 compute through the sampler Models: an MLP (13 inputs, two hidden
Linear layers of width 32, 5 classes, batch 8) stepped by the cSGHMC, SGLD,
SGHMC and unclipped cSGLD samplers with compute_dtype = bf16 against a
hand-written loop — a bf16 copy of
the network forward and backward, its gradients upcast, the existing fp32
kernels.sgmcmc_step on a plain fp32 state with Philox noise, theta.to(bf16)
written back — bit for bit in theta, momentum and moments, the shadow equal to
theta.to(bf16) after every step.  Plus: the hand loop is deterministic, the
parameters are bf16 views of the shadow with fp32 losses, a restored state
refreshes its shadow, and a Model without compute_dtype is the fp32 path."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 8
LRS = (0.02, 0.05)


class MLP(nn.Module):
    readout_name = "head"

    def __init__(self):
        super().__init__()
        self.l0 = nn.Linear(13, 32)
        self.l1 = nn.Linear(32, 32)
        self.head = nn.Linear(32, 5)

    def forward(self, x):
        return self.head(torch.relu(self.l1(torch.relu(self.l0(x)))))


def _net():
    torch.manual_seed(3)
    return MLP().to(DEV)


def _batches():
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(8, 13, generator=g).to(DEV), torch.randint(0, 5, (8,), generator=g).to(DEV))
            for _ in range(STEPS)]


# step t: (should_sample / collect kind): explore, sample, Welford init, Welford collects
PLAN = ["explore", "sample", "init", "collect", "explore", "collect", "sample", "collect"]


def _csghmc_kw(kind, m1, m2, count, step):
    from bayesdll_amd import _lib as L
    N, a = 64.0, 0.1
    ck = {"init": L.COLLECT_WELFORD_INIT, "collect": L.COLLECT_WELFORD}.get(kind, L.COLLECT_NONE)
    return dict(lrs=LRS, noise_scale=[1.0 * np.sqrt(2 * a * lr) / N for lr in LRS],
                one_minus_alpha=1 - a, prior_sig=0.9, collect=ck, collect_a=float(count),
                seed=17, chain=2, step=step, div_mode=None,
                noise_mode=L.NOISE_NONE if kind == "explore" else L.NOISE_PHILOX,
                mom1=m1 if ck else None, mom2=m2 if ck else None)


def _hand_loop():
    """bf16 network + the fp32 step on the upcast gradients + theta.to(bf16)."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    from bayesdll_amd.flat import FlatState
    master = _net()
    st = FlatState(master, need_mom=True, grad_mode="flat")  # plain fp32 state
    low = copy.deepcopy(master).to(torch.bfloat16)
    for p in low.parameters():
        p.grad = None
    crit = nn.CrossEntropyLoss()
    m1, m2 = torch.zeros_like(st.theta), torch.zeros_like(st.theta)
    count, losses = 0, []
    for t, ((x, y), kind) in enumerate(zip(_batches(), PLAN)):
        with torch.no_grad():
            for p, v in zip(low.parameters(), st.views(st.theta)):
                p.copy_(v.to(torch.bfloat16))
        for p in low.parameters():
            p.grad = None
        loss = crit(low(x.to(torch.bfloat16)).float(), y)
        loss.backward()
        with torch.no_grad():
            for p, gv in zip(low.parameters(), st.views(st.grad)):
                gv.copy_(p.grad.float())
        if kind in ("init", "collect"):
            count = 1 if kind == "init" else count + 1
        K.sgmcmc_step(st, L.CSGHMC, **_csghmc_kw(kind, m1, m2, count, t))
        losses.append(loss.detach())
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().view(np.int32) for k, v in
            (("theta", st.theta), ("mom", st.mom), ("m1", m1), ("m2", m2))}, \
        [float(v) for v in losses]


@pytest.fixture(scope="module")
def hand():
    return _hand_loop()


def test_premise_the_hand_loop_is_deterministic(hand):
    again, losses = _hand_loop()
    for k in hand[0]:
        assert np.array_equal(hand[0][k], again[k]), k
    assert losses == hand[1]


def _model_run(compute_dtype):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import csghmc
    net = _net()
    model = csghmc.Model(ND=64, prior_sig=0.9, momentum_decay=0.1)
    model.seed, model.chain, model.compute_dtype = 17, 2, compute_dtype
    crit = nn.CrossEntropyLoss()
    st = model.state_for(net)
    m1, m2 = torch.zeros_like(st.theta), torch.zeros_like(st.theta)
    count, losses, shadow_ok = 0, [], []
    for (x, y), kind in zip(_batches(), PLAN):
        collect = None
        if kind in ("init", "collect"):
            count = 1 if kind == "init" else count + 1
            collect = (L.COLLECT_WELFORD_INIT if kind == "init" else L.COLLECT_WELFORD,
                       m1, m2, float(count))
        loss, out = model(x, y, net, None, crit, list(LRS), 1.0, 1.0,
                          should_sample=kind != "explore", collect=collect)
        losses.append(loss)
        assert out.dtype == torch.float32
        if st.shadow is not None:
            shadow_ok.append(torch.equal(st.shadow, st.theta.to(torch.bfloat16)))
    torch.cuda.synchronize()
    bits = {k: v.detach().cpu().numpy().view(np.int32) for k, v in
            (("theta", st.theta), ("mom", st.mom), ("m1", m1), ("m2", m2))}
    return bits, losses, shadow_ok, model, net


def test_csghmc_model_in_bf16_equals_the_hand_loop(hand):
    bits, losses, shadow_ok, model, net = _model_run(torch.bfloat16)
    for k in hand[0]:
        assert np.array_equal(bits[k], hand[0][k]), k
    assert losses == hand[1] and all(np.isfinite(losses))
    assert len(shadow_ok) == STEPS and all(shadow_ok)
    st = model.flat
    for p, o in zip(net.parameters(), st.offsets):
        assert p.dtype == torch.bfloat16 and p.data_ptr() == st.shadow.data_ptr() + 2 * o
        assert p.grad is not None and p.grad.dtype == torch.bfloat16
    st.check_bound()
    assert not st.diverged()


def test_refresh_shadow_after_a_write_to_theta():
    _, _, _, model, net = _model_run(torch.bfloat16)
    st = model.flat
    with torch.no_grad():
        st.theta.mul_(1.37).add_(0.011)
    assert not torch.equal(st.shadow, st.theta.to(torch.bfloat16))
    st.refresh_shadow()
    torch.cuda.synchronize()
    assert torch.equal(st.shadow, st.theta.to(torch.bfloat16))
    assert torch.equal(next(net.parameters()).reshape(-1),
                       st.theta[:st.numels[0]].to(torch.bfloat16))


def test_default_is_the_fp32_path():
    a = _model_run(None)
    b = _model_run("fp32")
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert a[3].flat.shadow is None and a[3].flat.compute_dtype is None
    assert all(p.dtype == torch.float32 for p in a[4].parameters())
    low = _model_run(torch.bfloat16)
    assert not np.array_equal(a[0]["theta"], low[0]["theta"])  # bf16 compute is another chain


# ------------------------------------------------------------------ Runners
# The hand loop at Runner level: a second Runner of the same kind on the plain
# fp32 state and the existing fp32 step, whose forward / backward is the bf16
# copy of the network (weights theta.to(bf16) written back before every step,
# gradients upcast).  Schedule, collect bookkeeping and scalars are the Runner's
# own on both sides, so the comparison isolates the bf16 mode.
def _loader(seed, batches):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(8, 13, generator=g).to(DEV), torch.randint(0, 5, (8,), generator=g).to(DEV))
            for _ in range(batches)]


def _runner(method, logdir, compute_dtype, *, epochs=2, num_cycles=1, **hp_extra):
    import importlib
    import logging
    import os
    mod = importlib.import_module(f"bayesdll_amd.{method}")
    os.makedirs(logdir, exist_ok=True)
    hp = dict(prior_sig=1.0, bias="informative", Ninflate=1.0, nd=0.05, burnin=0, thin=1, nst=2,
              momentum_decay=0.18)
    hp.update(hp_extra)
    args = SimpleNamespace(device=DEV, ND=64, pretrained=None, lr=1e-2, lr_head=2e-2, momentum=0.5,
                           epochs=epochs, num_cycles=num_cycles, proportion_exploration=0.5,
                           full_sample=False, test_eval_freq=1, ece_num_bins=15,
                           log_dir=str(logdir), num_classes=5, noise_mode="philox", seed=77,
                           resume_state=True, compute_dtype=compute_dtype,
                           hparams={k: str(v) for k, v in hp.items()})
    return mod.Runner(_net(), None, args, logging.getLogger("lowp-runner"))


def _as_hand_loop(runner):
    """Replace the fp32 Runner's forward / backward by the bf16 copy's."""
    low = copy.deepcopy(runner.net).to(torch.bfloat16)

    def forward_backward(st, net, x, y, criterion):
        assert st.shadow is None and st.theta.dtype == torch.float32
        with torch.no_grad():
            for p, v in zip(low.parameters(), st.views(st.theta)):
                p.copy_(v.to(torch.bfloat16))
        for p in low.parameters():
            p.grad = None
        low.train(net.training)
        out = low(x.to(torch.bfloat16))
        loss = criterion(out.float(), y)
        st.zero_grad()
        loss.backward()
        for p, q in zip(net.parameters(), low.parameters()):
            p.grad = q.grad.float()
        st.sync_grads()
        return loss, out.float()

    runner.model.forward_backward = forward_backward
    return runner


def _watch_shadow(runner, seen):
    def hook(model, _inp, _out):
        st = model.flat
        seen.append(torch.equal(st.shadow, st.theta.to(torch.bfloat16)))
    runner.model.register_forward_hook(hook)


def _moments(r):
    if hasattr(r, "cycle_theta_mom1"):
        return [v for c in sorted(r.cycle_theta_mom1)
                for v in (r.cycle_theta_mom1[c], r.cycle_theta_mom2[c])]
    return [r.post_theta_mom1, r.post_theta_mom2]


@pytest.mark.parametrize("method", ["csghmc", "sgld"])
def test_runner_in_bf16_equals_the_hand_loop_and_evaluates_in_fp32(method, tmp_path):
    """8 steps (2 epochs of 4 batches): for cSGHMC 4 exploration steps, then a
    Welford init and 3 Welford collects with noise; for SGLD the first
    SGD-momentum step, then mean collects."""
    train, test = _loader(5, 4), _loader(6, 2)
    low = _runner(method, tmp_path / "low", "bf16")
    seen = []
    _watch_shadow(low, seen)
    hand = _as_hand_loop(_runner(method, tmp_path / "hand", None))
    res_l = low.train(train, None, test)
    res_h = hand.train(train, None, test)
    torch.cuda.synchronize()
    sl, sh = low.model.flat, hand.model.flat
    assert low.model.step_count == hand.model.step_count == 8
    assert sl.shadow is not None and sh.shadow is None
    assert torch.equal(sl.theta, sh.theta) and torch.equal(sl.mom, sh.mom)
    ml, mh = _moments(low), _moments(hand)
    assert len(ml) == len(mh) >= 2
    for a, b in zip(ml, mh):
        assert torch.equal(a, b)
    assert len(seen) == 8 and all(seen)
    # dtypes: bf16 parameter views of the shadow, fp32 finite losses
    for p, o in zip(low.net.parameters(), sl.offsets):
        assert p.dtype == torch.bfloat16 and p.data_ptr() == sl.shadow.data_ptr() + 2 * o
    if res_l is not None:  # (the SGLD Runner's train() returns nothing)
        assert np.isfinite(res_l["losses_train"]).all()
        assert np.array_equal(res_l["losses_train"], res_h["losses_train"])
    # evaluation: fp32 logits, equal to the same path on an fp32 network with
    # the same moments (the hand Runner's network is fp32)
    el, eh = low.evaluate(test), hand.evaluate(test)
    logits_l, logits_h = el[3], eh[3]
    assert torch.as_tensor(logits_l).dtype == torch.float32
    assert torch.equal(torch.as_tensor(logits_l), torch.as_tensor(logits_h))
    assert el[0] == eh[0] and el[1] == eh[1]


@pytest.mark.parametrize("method,geo,steps", [("sghmc", dict(epochs=2), 8),
                                              ("csgld", dict(epochs=4, num_cycles=2), 16)],
                         ids=["sghmc", "csgld-two-cycles"])
def test_sghmc_and_unclipped_csgld_runners_in_bf16_equal_the_hand_loop(method, geo, steps,
                                                                       tmp_path):
    """SGHMC (8 steps) and cSGLD without clip_grad over two cycles of 8 steps
    (the cycle boundary lies inside the run: the second cycle collects into
    moments of its own) against the hand loop: fp32 kernels on the upcast
    gradients plus theta.to(bf16)."""
    train, test = _loader(5, 4), _loader(6, 2)
    low = _runner(method, tmp_path / "low", "bf16", **geo)
    seen = []
    _watch_shadow(low, seen)
    hand = _as_hand_loop(_runner(method, tmp_path / "hand", None, **geo))
    low.train(train, None, test)
    hand.train(train, None, test)
    torch.cuda.synchronize()
    sl, sh = low.model.flat, hand.model.flat
    assert low.model.step_count == hand.model.step_count == steps
    assert sl.shadow is not None and sh.shadow is None
    assert torch.equal(sl.theta, sh.theta) and torch.equal(sl.mom, sh.mom)
    assert torch.equal(sl.shadow, sl.theta.to(torch.bfloat16))
    ml, mh = _moments(low), _moments(hand)
    assert len(ml) == len(mh) >= (4 if method == "csgld" else 2)
    for a, b in zip(ml, mh):
        assert torch.equal(a, b)
    if method == "csgld":  # both cycles collected, into different moments
        assert sorted(low.cycle_theta_mom1) == sorted(hand.cycle_theta_mom1)
        assert len(low.cycle_theta_mom1) == 2 and not torch.equal(ml[0], ml[2])
    assert len(seen) == steps and all(seen)
    for p, o in zip(low.net.parameters(), sl.offsets):
        assert p.dtype == torch.bfloat16 and p.data_ptr() == sl.shadow.data_ptr() + 2 * o
    assert not sl.diverged()


def test_checkpoint_roundtrip_and_exact_resume_in_bf16(tmp_path):
    import os
    train, test = _loader(5, 4), _loader(6, 2)
    a = _runner("csghmc", tmp_path / "a", "bf16", epochs=4, num_cycles=2)
    a.train(train, None, test)
    torch.cuda.synchronize()
    ck = os.path.join(tmp_path / "a", "1_ckpt.pt")
    assert os.path.exists(ck)
    from bayesdll_amd._runner import load_checkpoint
    saved = load_checkpoint(ck, "cpu")
    assert saved["last_theta"].dtype == torch.float32  # the master, under the same keys
    assert all(v.dtype == torch.float32 for sd in saved["cycle_states"].values()
               for v in sd.values())
    b = _runner("csghmc", tmp_path / "b", "bf16", epochs=4, num_cycles=2)
    epoch = b.load_ckpt(ck, resume=True)
    assert epoch == 1
    sb = b.model.flat
    assert torch.equal(sb.theta, saved["last_theta"].to(DEV))
    assert torch.equal(sb.shadow, sb.theta.to(torch.bfloat16))
    assert all(p.dtype == torch.bfloat16 for p in b.net.parameters())
    sb.check_bound()
    b.train(train, None, test, start_epoch=epoch + 1)
    torch.cuda.synchronize()
    assert torch.equal(sb.theta, a.model.flat.theta) and torch.equal(sb.mom, a.model.flat.mom)
    assert torch.equal(sb.shadow, a.model.flat.shadow)
    assert b.samples_per_cycle == a.samples_per_cycle
    for c in a.cycle_theta_mom1:
        assert torch.equal(b.cycle_theta_mom1[c].to(DEV), a.cycle_theta_mom1[c])
        assert torch.equal(b.cycle_theta_mom2[c].to(DEV), a.cycle_theta_mom2[c])


def test_sgld_checkpoint_holds_the_fp32_master_and_resumes_exactly(tmp_path):
    import os
    train, test = _loader(5, 4), _loader(6, 2)
    a = _runner("sgld", tmp_path / "a", "bf16", epochs=3)
    a.train(train, None, test)
    full = a.model.flat.theta.clone()
    b = _runner("sgld", tmp_path / "b", "bf16", epochs=2)
    b.train(train, None, test)
    fname = b.save_ckpt(epoch=1)
    from bayesdll_amd._runner import load_checkpoint
    saved = load_checkpoint(fname, "cpu")
    assert all(v.dtype == torch.float32 for v in saved["last_theta"].values())
    c = _runner("sgld", tmp_path / "c", "bf16", epochs=3)
    assert c.load_ckpt(fname, resume=True) == 1
    sc = c.model.flat
    assert torch.equal(sc.theta, b.model.flat.theta)
    assert torch.equal(sc.shadow, sc.theta.to(torch.bfloat16))
    c.train(train, None, test, start_epoch=2)
    torch.cuda.synchronize()
    assert torch.equal(sc.theta, full)
    assert os.path.exists(fname)


def test_runner_without_compute_dtype_is_the_unchanged_fp32_path(tmp_path, monkeypatch):
    """A default Runner against a second fp32 Runner whose forward / backward
    and launch are spelled as before this mode existed: the eager fp32 pass
    and bdl_sgmcmc_step called directly with the step's arguments."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import csghmc
    from bayesdll_amd import kernels as K
    train, test = _loader(5, 4), _loader(6, 2)
    a = _runner("csghmc", tmp_path / "a", None)
    assert a.model.compute_dtype is None
    a.train(train, None, test)
    torch.cuda.synchronize()
    assert a.model.flat.shadow is None
    assert all(p.dtype == torch.float32 for p in a.net.parameters())

    b = _runner("csghmc", tmp_path / "b", None)

    def forward_backward(st, net, x, y, criterion):
        out = net(x)
        loss = criterion(out, y)
        st.zero_grad()
        loss.backward()
        st.sync_grads()
        return loss, out

    def plain_step(state, method, **kw):
        args = K._step_args(state, method, **kw)
        L.check(L.lib().bdl_sgmcmc_step(args, L.current_stream_handle(state.device)), "step")

    b.model.forward_backward = forward_backward
    monkeypatch.setattr(csghmc.K, "sgmcmc_step", plain_step)
    b.train(train, None, test)
    torch.cuda.synchronize()
    assert torch.equal(a.model.flat.theta, b.model.flat.theta)
    assert torch.equal(a.model.flat.mom, b.model.flat.mom)
    for x, y in zip(_moments(a), _moments(b)):
        assert torch.equal(x, y)


def test_csghmc_fs_in_bf16_cold_restarts_and_evaluates_in_fp32(tmp_path):
    """csghmc_fs with cold restarts and a validation loader: point estimates
    and the full-sample BMA run on fp32 networks, the snapshots hold the fp32
    master, and a cold restart draws fp32 values into theta and refreshes the
    shadow."""
    import os
    train, val, test = _loader(5, 4), _loader(7, 2), _loader(6, 2)
    r = _runner("csghmc_fs", tmp_path / "fs", "bf16", epochs=8, num_cycles=2,
                perform_cold_restarts="true")
    restarts = []
    orig = r._reinitialize_network_fresh

    def spy():
        before = r.model.flat.theta.clone()
        orig()
        st = r.model.flat
        restarts.append((not torch.equal(before, st.theta),
                         torch.equal(st.shadow, st.theta.to(torch.bfloat16)),
                         bool((st.theta != st.theta.to(torch.bfloat16).float()).any())))
    r._reinitialize_network_fresh = spy
    res = r.train(train, val, test)
    torch.cuda.synchronize()
    st = r.model.flat
    assert restarts and all(all(t) for t in restarts)  # moved, shadow fresh, fp32 draws
    assert torch.isfinite(st.theta).all() and np.isfinite(res["losses_test"]).all()
    assert torch.equal(st.shadow, st.theta.to(torch.bfloat16))
    st.check_bound()
    snaps = [f for f in os.listdir(tmp_path / "fs") if f.startswith("full_samples_net_ep")]
    assert snaps
    sd = torch.load(os.path.join(tmp_path / "fs", snaps[0]), weights_only=True)
    assert all(v.dtype == torch.float32 for v in sd.values())
