"""_StackedSampler.fit_stacking and weights="stacking" on the device: a K = 4
StackedSGLD sweep over two decades of lr (nst = 0: evaluation is
deterministic), one cyclical sampler with collected cycles, and chains
initialised as copies.

Guaranteed on the loader the weights were fitted on (tol = 1e-4): the weighted
evaluate's NLL is -objective up to the fp32 path of kernels.mixture (a few
u = 2^-24 relative on each probability and logf's ulp: 1e-5 absolute is
generous for NLLs of order 1); objective >= objective_uniform (EM never
decreases f from its start) and, with f* - objective <= gap <= tol,
objective >= every single chain's own log score - tol."""
import numpy as np
import pytest
import torch

from test_gpu_chain_diag import Net, _args

pytestmark = pytest.mark.gpu
N, TOL, FP32 = 200, 1e-4, 1e-5


@pytest.fixture(scope="module")
def data():
    """(training loader, validation loader): labels that depend on the inputs."""
    g = torch.Generator().manual_seed(41)
    xs = torch.randn(2 * N, 13, generator=g)
    ys = (xs[:, :5] + 0.5 * torch.randn(2 * N, 5, generator=g)).argmax(-1)
    cut = range(0, N, 32)
    return ([(xs[i:i + 32].cuda(), ys[i:i + 32].cuda()) for i in cut],
            [(xs[N + i:N + i + 32].cuda(), ys[N + i:N + i + 32].cuda()) for i in cut])


def _sampler(cls="StackedSGLD", nst=0, K_=4, init="reinit", **kw):
    from bayesdll_amd import stacked
    torch.manual_seed(31)
    return getattr(stacked, cls)(Net().cuda(), K_, _args(nst=nst), init=init, seed=4, chain0=2,
                                 graph=False, **kw)


def _check(S, val, d):
    K_ = S.K
    w = d["weights"]
    assert w.shape == (K_,) and w.dtype == np.float64
    assert abs(w.sum() - 1) < 1e-12 and (w > 0).all()
    assert d["n"] == N and (d["n_label"], d["n_nonfinite"], d["n_impossible"]) == (0, 0, 0)
    assert d["converged"] and 0 <= d["gap"] <= TOL
    assert torch.equal(S.stacking_.cpu(), torch.from_numpy(w)) and "stacking_" not in S.state_dict()
    nll_w, err_w = S.evaluate(val, weights="stacking")
    nll_u, _ = S.evaluate(val)
    nll_k, _ = S.evaluate_chains(val)
    print(f"weights {w}, stacked NLL {nll_w:.6f}, uniform {nll_u:.6f}, chains {nll_k}, "
          f"gap {d['gap']:.2e}, iterations {d['iterations']}")
    assert abs(nll_w + d["objective"]) <= FP32
    assert abs(nll_u + d["objective_uniform"]) <= FP32
    assert nll_w <= nll_u + TOL + FP32
    assert (nll_w <= nll_k + TOL + FP32).all()
    assert d["objective"] >= d["objective_uniform"] and 0 <= err_w <= 1
    best = int(np.argmin(nll_k))
    assert d["best_single"] == S.chain0 + best
    assert abs(d["objective_best_single"] + nll_k[best]) <= FP32
    return nll_w


def test_stacking_pools_a_per_chain_sweep(data):
    train, val = data
    S = _sampler(per_chain={"lr": [1e-1, 2e-2, 5e-3, 1e-3], "lr_head": [1e-1, 2e-2, 5e-3, 1e-3]})
    with pytest.raises(ValueError, match=r"needs a fit_stacking\(\) first"):
        S.evaluate(val, weights="stacking")
    for ep in range(3):
        S.train_one_epoch(train, ep)
    d0 = S.draws
    d = S.fit_stacking(val, tol=TOL)
    assert S.draws == d0 and S.net.training                  # nst = 0 draws nothing
    nll_w = _check(S, val, d)
    assert d["weights"].max() > 0.3                          # two decades of lr: not uniform
    # the pooled "gmm" form stays refused under per_chain, word for word
    with pytest.raises(ValueError, match="is not cyclical"):
        S.evaluate(val, weights="gmm")
    with pytest.raises(ValueError, match="pooled form only"):
        S.evaluate_chains(val, weights="stacking")
    with pytest.raises(ValueError, match="pooled form only"):
        S.uncertainty(val, by_chain=True, weights="stacking")
    with pytest.raises(ValueError, match='combine="reference"'):
        S.evaluate(val, weights="stacking", combine="reference")
    u = S.uncertainty(val, weights="stacking")
    assert abs(u["nll"] - nll_w) <= FP32 and u["n"] == N and u["members"] >= S.K
    assert u["mutual_info"] >= -1e-6 and u["entropy"] > 0
    t = S.fit_temperature(val, weights="stacking")
    assert abs(t["nll_before"] - nll_w) <= FP32 and t["nll_after"] <= t["nll_before"] + 1e-9
    with pytest.raises(ValueError, match="the loader is empty"):
        S.fit_stacking([])
    holes = [(x, torch.full_like(y, 99)) for x, y in val]
    with pytest.raises(ValueError, match="n = 0"):
        S.fit_stacking(holes)


def test_identical_chains_converge_at_once_with_uniform_weights(data):
    _, val = data
    S = _sampler(init="copy")
    d = S.fit_stacking(val)
    assert d["converged"] and d["iterations"] == 0 and d["gap"] <= 1e-12
    assert np.array_equal(d["weights"], np.full(4, 0.25))
    assert d["objective"] == d["objective_uniform"]
    assert abs(d["objective_best_single"] - d["objective"]) <= FP32


def test_a_cyclical_sampler_with_collected_cycles(data):
    train, val = data
    S = _sampler("StackedCSGHMC", nst=0, K_=3)
    for ep in range(2):
        S.train_one_epoch(train, ep)
    assert len(S._component_keys()) >= 1
    d = S.fit_stacking(val, tol=TOL)
    _check(S, val, d)
    u = S.uncertainty(val, weights="stacking")
    assert abs(u["nll"] + d["objective"]) <= FP32
    assert u["members"] == len(S._component_keys()) * S.K
