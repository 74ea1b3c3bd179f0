"""Same-seed parity of noise_mode="torch", for every sampler and draw.

The product Models run with noise_mode="torch" and div_mode="recip" on the
same torch.manual_seed as the reference chain of tests/same_seed_ref.py on
the same device (the oracle's per-tensor rules as torch ops, noise from
torch.randn_like exactly where the reference draws it).  Per case:

  * the stream itself: after every product step the flat noise buffer, viewed
    per tensor, equals the reference's recorded draws of that step BIT FOR BIT
    for every tensor that had a gradient — no tolerance, so stream alignment
    is pinned apart from the update arithmetic;
  * theta and every buffer the method owns (momentum, SGD buffer, Adam m and
    v) within RTOL = 1e-5, in the form tests/test_gpu_parity.py uses;
  * tensors without a gradient in a step (frozen, or skipped by that step's
    backward) keep theta and every buffer bit-unchanged, in the flat and the
    tensor gradient mode.

Cases (same_seed_ref.CASES): the seven samplers on the toy table and on a
40-tensor table of odd sizes; cSGHMC with explore and sample steps
interleaved, also through csghmc_fs; a frozen tensor plus alternating
gradient-less tensors; the mlp_mnist-size table.  Then the evaluation draws
of PosteriorDraw (three variance sources, a frozen parameter drawn too) and
train - evaluate - train on one seed.  tests/test_same_seed_host.py shows from
the reference alone that every misalignment these cases can see moves theta by
at least 100 x RTOL.
"""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import same_seed_ref as R
from same_seed_ref import RTOL, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _make_model(c):
    mod = importlib.import_module(f"bayesdll_amd.{c['method']}")
    m = c["method"]
    kw = dict(prior_sig=c["prior_sig"], bias=c["bias"])
    if m not in ("sgld", "csgld"):
        kw["momentum_decay"] = c["alpha"]
    if m.startswith("adam_"):
        kw.update(beta1=c["beta1"], beta2=c["beta2"], epsilon=c["epsilon"])
    if m == "adam_csghmc":
        kw["temperature"] = c["temperature"]
    model = mod.Model(c["N"], **kw)
    model.noise_mode = "torch"
    model.div_mode = "recip"
    return model


class ProductChain:
    """The product Model of a case, stepped as its Runner steps it."""

    def __init__(self, c, grad_mode):
        from bayesdll_amd.sgld import FusedSGD
        self.c = c
        self.net, self.net0 = R.build_nets(c, DEV)
        self.model = _make_model(c)
        m = c["method"]
        # sghmc's and adam_csghmc's Runners step SGD with momentum 0
        # (methods/sghmc.py:53-57, methods/adam_csghmc.py:70); cSGHMC has no SGD
        self.mu = c["momentum"] if m in ("sgld", "csgld", "adam_sghmc") else 0.0
        named = list(self.net.named_parameters())
        opt = torch.optim.SGD(
            [{"params": [p for n, p in named if "classifier" not in n], "lr": c["lr"]},
             {"params": [p for n, p in named if "classifier" in n], "lr": c["lr_head"]}],
            momentum=self.mu)
        self.sgd = FusedSGD(opt, self.mu)
        self.crit = torch.nn.CrossEntropyLoss()
        (self.x, self.y), = R.fake_loader(1, device=DEV)
        old = os.environ.get("BDL_GRAD_MODE")
        os.environ["BDL_GRAD_MODE"] = grad_mode
        try:
            self.st = self.model.state_for(self.net, self.net0)
        finally:
            if old is None:
                os.environ.pop("BDL_GRAD_MODE", None)
            else:
                os.environ["BDL_GRAD_MODE"] = old
        assert self.st.grad_mode == grad_mode
        self.k = 0
        self.noises = []     # per step: the flat noise buffer after the step
        self.disturbed = []  # (step, tensor, buffer) of gradient-less tensors that changed
        torch.manual_seed(c["noise_seed"])

    def buffers(self):
        m, st = self.c["method"], self.st
        out = {"theta": st.theta}
        if m in ("sgld", "csgld"):
            out["sgd_buf"] = st.mom
        else:
            out["mom"] = st.mom
        if m.startswith("adam_"):
            out["adam_m"], out["adam_v"] = self.model.adam_buffers(st)
            if self.mu != 0:
                out["sgd_buf"] = self.model.ensure_sgd_buffer()
        return out

    def step(self, live=None):
        c, k = self.c, self.k
        lrs = [c["lr"], c["lr_head"]]
        args = (self.x, self.y, self.net, self.net0, self.crit, lrs, 1.0, c["nd"])
        before = {key: v.clone() for key, v in self.buffers().items()}
        if c["method"] in ("csghmc", "csghmc_fs"):
            ss = True if c["pattern"] is None else bool(c["pattern"][k])
            self.model(*args, should_sample=ss)
        elif c["clip_grad"] is not None:
            self.model(*args, sgd=self.sgd, clip_grad=c["clip_grad"])
        else:
            self.model(*args, sgd=self.sgd)
        assert self.model.flat is self.st
        self.noises.append(self.st.noise.clone())
        if live is not None:
            st = self.st
            after = self.buffers()
            for i in sorted(set(range(len(st.numels))) - set(live)):
                assert not st.has_grad(i)
                o, n = st.offsets[i], st.numels[i]
                for key, v in before.items():
                    if not torch.equal(after[key][o:o + n], v[o:o + n]):
                        self.disturbed.append((k, st.names[i], key))
            for i in live:
                assert st.has_grad(i)
        self.k += 1

    def run(self, steps, lives=None):
        for _ in range(steps):
            self.step(None if lives is None else lives[self.k])
        return self

    def state(self):
        torch.cuda.synchronize()
        return {key: v.detach().cpu().numpy() for key, v in self.buffers().items()}


@functools.lru_cache(maxsize=None)
def _pair(name, grad_mode):
    """(reference chain, product chain) of a case, each run once."""
    c = R.CASES[name]
    ref = R.reference_chain(c, DEV)
    got = ProductChain(c, grad_mode).run(c["steps"], ref.live)
    return ref, got


PARAMS = [(nm, mode) for nm in R.CASES
          for mode in (("tensor", "flat") if nm in R.NO_GRAD_CASES else ("tensor",))]
NO_GRAD_PARAMS = [(nm, mode) for nm, mode in PARAMS if nm in R.NO_GRAD_CASES]


def _assert_stream(noises, draws, lives, st):
    """Every step's noise buffer, per tensor, against that step's draws."""
    assert len(noises) == len(draws)
    bad = []
    for k, (buf, eps, live) in enumerate(zip(noises, draws, lives)):
        assert sorted(eps) == list(live)
        for i in live:
            o, n = st.offsets[i], st.numels[i]
            if not torch.equal(buf[o:o + n], eps[i].reshape(-1)):
                bad.append((k, st.names[i]))
    assert not bad, f"noise differs from the reference draw at (step, tensor): {bad[:8]}"


def _assert_state(got, want, keys):
    for key in keys:
        e = rel_err(got[key], want[key])
        print(key, f"rel_err {e:.3e}")
        assert e <= RTOL, (key, e)
        np.testing.assert_allclose(got[key], want[key], rtol=RTOL, atol=1e-6, err_msg=key)


@pytest.mark.parametrize("name,grad_mode", PARAMS)
def test_noise_buffer_equals_the_reference_draws_bit_for_bit(name, grad_mode):
    ref, got = _pair(name, grad_mode)
    _assert_stream(got.noises, ref.draws, ref.live, got.st)


@pytest.mark.parametrize("name,grad_mode", PARAMS)
def test_theta_and_every_owned_buffer_match_the_reference(name, grad_mode):
    ref, got = _pair(name, grad_mode)
    state = got.state()
    keys = R.owned_keys(R.CASES[name])
    assert set(keys) == set(state)
    _assert_state(state, ref.state(), keys)


@pytest.mark.parametrize("name,grad_mode", NO_GRAD_PARAMS)
def test_tensors_without_a_gradient_are_bit_unchanged_by_the_step(name, grad_mode):
    ref, got = _pair(name, grad_mode)
    c = R.CASES[name]
    assert all(ref.live[k] == R.expected_live(c, k, ref.names) for k in range(c["steps"]))
    assert any(len(lv) < len(ref.names) for lv in ref.live)
    assert not got.disturbed, got.disturbed[:8]


def test_csghmc_fs_steps_with_the_csghmc_model():
    import bayesdll_amd.csghmc as csghmc
    import bayesdll_amd.csghmc_fs as csghmc_fs
    assert csghmc_fs.Model is csghmc.Model


# --------------------------------------------------------------- evaluation
def _var_args(kind):
    from bayesdll_amd import _lib as L
    if kind == "raw":
        return L.VAR_RAW_MOMENTS, R.EVAL_COUNT / (R.EVAL_COUNT - 1)
    if kind == "welford":
        return L.VAR_WELFORD, float(R.EVAL_COUNT - 1)
    return L.VAR_GIVEN, 1.0


def _assert_sample(draw, want, eps):
    assert torch.equal(draw.noise, eps), "evaluation noise differs from the reference draws"
    got, want = draw.theta.cpu().numpy(), want.cpu().numpy()
    e = rel_err(got, want)
    print(f"sample rel_err {e:.3e}")
    assert e <= RTOL, e
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-6)


@pytest.mark.parametrize("kind", R.EVAL_KINDS)
def test_evaluation_draws_match_the_reference_sample(kind):
    from bayesdll_amd._runner import PosteriorDraw
    c = R.EVAL_CASES["sgld_mom"]
    ch = R.RefChain(c, DEV)
    assert any(not p.requires_grad for p in ch.params)  # the frozen one is drawn too
    n = sum(p.numel() for p in ch.params)
    mean, m2 = R.eval_moments(n, kind, DEV)
    want = [ch.draw(mean, kind, m2, R.EVAL_COUNT) for _ in range(R.EVAL_NST)]

    net, _ = R.build_nets(c, DEV)
    draw = PosteriorDraw(net, "torch", 0, 0)
    torch.manual_seed(c["noise_seed"])
    for j in range(R.EVAL_NST):
        draw.draw(mean, m2, *_var_args(kind))
        _assert_sample(draw, want[j], ch.eval_draws[j])
        flat = torch.cat([p.detach().reshape(-1) for p in draw.net.parameters()])
        assert torch.equal(flat, draw.theta)  # the evaluation copy computes with the sample


@pytest.mark.parametrize("name,kind", [("csghmc", "welford"), ("sgld_mom", "raw"),
                                       ("adam_sghmc_mom", "raw")])
def test_training_continues_on_the_right_stream_after_evaluation_draws(name, kind):
    from bayesdll_amd._runner import PosteriorDraw
    c = R.EVAL_CASES[name]
    before, ndraws, after = R.EVAL_SCHEDULE
    ref, want = R.reference_train_eval_train(c, DEV, kind)

    got = ProductChain(c, "tensor").run(before, ref.live)
    mean, m2 = R.eval_moments(got.st.n, kind, DEV)
    draw = PosteriorDraw(got.net, "torch", 0, 0)
    for j in range(ndraws):
        draw.draw(mean, m2, *_var_args(kind))
        _assert_sample(draw, want[j], ref.eval_draws[j])
    got.run(after, ref.live)

    _assert_stream(got.noises, ref.draws, ref.live, got.st)
    assert not got.disturbed, got.disturbed[:8]
    _assert_state(got.state(), ref.state(), R.owned_keys(c))
