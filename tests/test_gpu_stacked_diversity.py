"""_StackedSampler.diversity on the device: the pair matrices equal
tests/diversity_ref.py applied to chain_logprob(x) of the same batches (the
same sampler with its draw counter put back), the error diagonal is
evaluate_chains' error, chains initialised as copies are at distance exactly
zero, `draws` advances as an evaluate would advance it, K = 1 is refused.

Tolerance.  The reference voters are chain_logprob's fp64 log mixtures; the
kernel reads bdl_predict's fp32 logp of the same members, off by at most
delta = 8u (1 + max |logp|) (u = 2^-24: the mixture's relative error of a few
u, tests/predict_ref.py, and logf's ulp).  A perturbation delta of a voter's
logits changes each of its probabilities by at most 2 delta relatively, an
example's total variation by at most 2 delta and its KL by at most
4 delta (1 + KL); the means over the loader inherit that, on top of the
kernel's own derived bound (diversity_ref)."""
import numpy as np
import pytest
import torch

import diversity_ref as R
from test_gpu_chain_diag import Net, _args

pytestmark = pytest.mark.gpu
N = 200


@pytest.fixture(scope="module")
def data():
    """(training loader, the same inputs with two labels out of range): 200
    examples in batches of 32, the last one short."""
    g = torch.Generator().manual_seed(23)
    xs, ys = torch.randn(N, 13, generator=g), torch.randint(0, 5, (N,), generator=g)
    yu = ys.clone()
    yu[[4, 150]] = 99
    cut = range(0, N, 32)
    return ([(xs[i:i + 32].cuda(), ys[i:i + 32].cuda()) for i in cut],
            [(xs[i:i + 32].cuda(), yu[i:i + 32].cuda()) for i in cut])


def _sampler(cls, nst, loader=None, K_=3, init="reinit"):
    from bayesdll_amd import stacked
    torch.manual_seed(31)
    S = getattr(stacked, cls)(Net().cuda(), K_, _args(nst=nst), init=init, seed=4, chain0=2,
                              graph=False)
    if loader is not None:
        S.train_one_epoch(loader, 0)
    return S


@pytest.mark.parametrize("cls", ["StackedSGLD", "StackedCSGHMC"])
def test_diversity_is_the_reference_on_the_chains_own_predictives(data, cls):
    clean, holes = data
    S = _sampler(cls, 2, clean)
    assert len(S._component_keys()) > 0                       # collected components
    d0 = S.draws
    d = S.diversity(holes)
    d1 = S.draws
    S.draws = d0
    S.net.eval()
    lp = torch.cat([S.chain_logprob(x) for x, _ in holes], 1).cpu().numpy()   # [K, N, C] fp64
    S.net.train()
    assert S.draws == d1 and d1 > d0                          # the same draws, the same count
    yu = torch.cat([y for _, y in holes]).cpu().numpy()
    delta = 8 * R.U * (1 + float(np.abs(lp).max()))
    top = np.sort(lp, -1)
    assert (top[..., -1] - top[..., -2]).min() > 2 * delta    # no vote hangs on the rounding
    ref = R.reference(lp.astype(np.float32), yu, want_bound=True)
    n, nl = ref["n"], ref["n_labelled"]
    assert (d["n"], d["n_labelled"], d["n_nonfinite"]) == (N, N - 2, 0) == (n, nl, 0)
    assert np.array_equal(d["disagreement"], ref["disagree"] / n)
    assert np.array_equal(d["double_fault"], ref["both_wrong"] / nl)
    assert np.array_equal(d["kl_unbounded"], np.zeros((3, 3), dtype=np.int64))
    tv, kl = ref["tv_sum"] / n, ref["kl_sum"] / n
    err_tv, err_kl = np.abs(d["tv"] - tv), np.abs(d["kl"] - kl)
    print(f"{cls}: tv error {err_tv.max():.3g} (allowed {2 * delta:.3g}), "
          f"kl error {err_kl.max():.3g}")
    assert (err_tv <= ref["bound"]["tv_sum"] / n + 2 * delta).all()
    assert (err_kl <= ref["bound"]["kl_sum"] / n + 4 * delta * (1 + kl)).all()
    assert np.array_equal(d["sym_kl"], d["kl"] + d["kl"].T)
    assert d["tv"][0, 1] > 1e-3                               # reinitialised chains do differ
    # the error diagonal is evaluate_chains' error on the labelled examples
    S.draws = d0
    _, err = S.evaluate_chains(clean)
    w = np.argmax(lp, -1) != torch.cat([y for _, y in clean]).cpu().numpy()
    # (the device divides its counts by N through a reciprocal: an ulp may differ)
    assert np.array_equal(np.rint(err * N), w.sum(-1))
    assert np.abs(err - w.sum(-1) / N).max() <= 2.0 ** -52
    assert np.array_equal(d["error"], w[:, yu != 99].sum(-1) / (N - 2))
    # the summary is kernels.diversity_pairs of the matrices
    from bayesdll_amd import kernels as K
    assert d["summary"] == K.diversity_pairs(d)
    s = d["summary"]
    assert s["tv"]["min"] == min(d["tv"][i, j] for i in range(3) for j in range(i + 1, 3))
    assert len(s["nearest"]) == 3 and all(s["nearest"][i] != i for i in range(3))
    # `draws` advances as an evaluate over the loader advances it (the same
    # batches with their labels in range: evaluate's nll_loss indexes by label)
    S.draws = d0
    S.evaluate(clean)
    assert S.draws == d1
    assert S.net.training


def test_copied_chains_are_at_distance_exactly_zero(data):
    clean, _ = data
    S = _sampler("StackedSGLD", 2, None, init="copy")
    d = S.diversity(clean)
    for k in ("disagreement", "tv", "kl", "sym_kl"):
        assert not d[k].any(), k
    assert not d["kl_unbounded"].any() and d["n"] == N
    assert d["summary"]["nearest"] == [1, 0, 0]
    assert d["summary"]["tv"]["min_pair"] == (0, 1) == d["summary"]["tv"]["max_pair"]
    assert np.array_equal(d["double_fault"], np.full((3, 3), d["error"][0]))


def test_one_chain_is_refused_and_nothing_the_sampler_owns_changes(data):
    from test_gpu_chain_diag import _owned
    clean, holes = data
    with pytest.raises(ValueError, match="needs K >= 2"):
        _sampler("StackedSGLD", 0, None, K_=1).diversity(clean)
    S = _sampler("StackedSGLD", 0, clean)
    owned, d0 = _owned(S), S.draws
    before = S.evaluate(clean)
    d = S.diversity(holes)
    assert S.draws == d0                                      # nst = 0 draws nothing
    assert all(torch.equal(v, owned[k]) for k, v in _owned(S).items())
    assert S.evaluate(clean) == before and d["n"] == N
    with pytest.raises(ValueError, match="the loader is empty"):
        S.diversity([])
