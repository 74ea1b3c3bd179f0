"""_StackedSampler.detection on the device: the rank statistics of the
uncertainty scores equal tests/rank_ref.py applied to what
uncertainty(per_example=True) returns for the same members (the same sampler
with its draw counter put back), for both tasks, pooled and by chain; a set
ranked against itself gives AUROC one half; `draws` advances as documented and
nothing the sampler owns changes."""
import numpy as np
import pytest
import torch

import rank_ref as R
from test_gpu_chain_diag import Net, _args

pytestmark = pytest.mark.gpu
SCORES = ("entropy", "mutual_info", "expected_entropy", "neg_confidence", "disagree")
N, UNLABELLED = 200, (5, 77, 199)


@pytest.fixture(scope="module")
def data():
    """(training / evaluate loader, the same inputs with three labels out of
    range, a shifted set without labels): 200 examples, the last batch short."""
    g = torch.Generator().manual_seed(18)
    xs, ys = torch.randn(N, 13, generator=g), torch.randint(0, 5, (N,), generator=g)
    yu = ys.clone()
    yu[list(UNLABELLED)] = 99
    cut = range(0, N, 32)
    clean = [(xs[i:i + 32].cuda(), ys[i:i + 32].cuda()) for i in cut]
    holes = [(xs[i:i + 32].cuda(), yu[i:i + 32].cuda()) for i in cut]
    shifted = [(1.5 * xs[i:i + 48] + 0.5).cuda() for i in range(0, 144, 48)]  # x alone
    return clean, holes, shifted


def _sampler(nst, loader, **kw):
    from bayesdll_amd import stacked
    torch.manual_seed(31)
    S = stacked.StackedSGLD(Net().cuda(), 3, _args(nst=nst), init="reinit", seed=4, chain0=2,
                            graph=False, **kw)
    S.train_one_epoch(loader, 0)
    return S


def _rows(per, g):
    """The five score rows of group g from uncertainty's per-example tensors."""
    p = {k: v[g].cpu().numpy() for k, v in per.items()}
    return {"entropy": p["entropy"], "mutual_info": p["mutual_info"],
            "expected_entropy": p["expected_entropy"], "neg_confidence": -p["confidence"],
            "disagree": p["disagree"].astype(np.float32)}, p["pred"]


def _check(task, rows, marks, k=None):
    pick = (lambda v: v) if k is None else (lambda v: v[k])
    for nm in SCORES:
        ref = R.row_loop(rows[nm], marks)
        P, Nn = ref["n_pos"], ref["n_neg"]
        assert P > 0 and Nn > 0
        got = {f: pick(task[nm][f]) for f in ("auroc", "ap", "fpr95")}
        assert got["auroc"] == ref["u2"] / (2 * P * Nn), (nm, k)
        assert got["fpr95"] == ref["fp_at_tpr"] / Nn, (nm, k)
        assert abs(got["ap"] - ref["ap_sum"] / P) <= 2.0 ** -51, (nm, k)
        assert (pick(task["n_pos"]), pick(task["n_neg"]), pick(task["n_excluded"])) == \
            (P, Nn, ref["n_excluded"])
    return ref


@pytest.mark.parametrize("by_chain", [False, True])
def test_detection_is_the_reference_on_uncertaintys_per_example_scores(data, by_chain):
    clean, holes, shifted = data
    S = _sampler(2, clean)
    yu = torch.cat([y for _, y in holes]).cpu().numpy()
    d0 = S.draws
    det = S.detection(holes, shifted, by_chain=by_chain)
    d2 = S.draws
    S.draws = d0
    u1 = S.uncertainty(holes, by_chain=by_chain, per_example=True)
    d1 = S.draws
    u2 = S.uncertainty([(x, torch.zeros(len(x), dtype=torch.int64, device=x.device))
                        for x in shifted], by_chain=by_chain, per_example=True)
    # `draws` advanced as one uncertainty call per loader advances it
    assert S.draws == d2 and d1 > d0 and d2 - d1 == (d1 - d0) * len(shifted) // len(holes)
    assert sorted(det) == ["members", "misclassification", "shift"]
    assert det["members"] == u1["members"] == u2["members"]
    G = 3 if by_chain else 1
    for g in range(G):
        k = g if by_chain else None
        r1, pred = _rows(u1["per_example"], g)
        marks = np.where(yu == 99, 2, (pred != yu).astype(np.int32)).astype(np.int32)
        ref = _check(det["misclassification"], r1, marks, k)
        assert ref["n_excluded"] == len(UNLABELLED)       # the unlabelled examples, only here
        r2, _ = _rows(u2["per_example"], g)
        both = {nm: np.concatenate([r1[nm], r2[nm]]) for nm in SCORES}
        marks = np.concatenate([np.zeros(N, np.int32), np.ones(144, np.int32)])
        ref = _check(det["shift"], both, marks, k)
        assert (ref["n_pos"], ref["n_neg"], ref["n_excluded"]) == (144, N, 0)
    if by_chain:
        assert all(len(det[t][nm][f]) == 3 for t in ("misclassification", "shift")
                   for nm in SCORES for f in ("auroc", "ap", "fpr95"))
        assert all(len(det["shift"][f]) == 3 for f in ("n_pos", "n_neg", "n_excluded"))


def test_a_set_ranked_against_itself_and_a_subset_of_scores(data):
    clean, holes, _ = data
    S = _sampler(0, clean)                         # nst = 0: the members are deterministic
    d0 = S.draws
    det = S.detection(clean, clean, scores=("mutual_info", "disagree"))
    assert S.draws == d0                           # nst = 0 draws nothing
    assert sorted(det["shift"]) == ["disagree", "mutual_info", "n_excluded", "n_neg", "n_pos"]
    for nm in ("mutual_info", "disagree"):
        assert det["shift"][nm]["auroc"] == 0.5
    assert (det["shift"]["n_pos"], det["shift"]["n_neg"], det["shift"]["n_excluded"]) == (N, N, 0)
    assert det["misclassification"]["n_excluded"] == 0
    assert "shift" not in S.detection(holes)
    with pytest.raises(ValueError, match="a loader is empty"):
        S.detection([])


def test_detection_changes_nothing_evaluate_sees(data):
    from test_gpu_chain_diag import _owned
    clean, holes, shifted = data
    S = _sampler(2, clean, per_chain={"lr": [1e-2, 5e-2, 1e-1]})
    d0 = S.draws
    before = S.evaluate(clean)
    owned = _owned(S)
    S.draws = d0
    det = S.detection(holes, shifted, by_chain=True)
    assert len(det["shift"]["entropy"]["auroc"]) == 3
    assert all(torch.equal(v, owned[k]) for k, v in _owned(S).items())
    assert S.net.training
    S.draws = d0
    assert S.evaluate(clean) == before
