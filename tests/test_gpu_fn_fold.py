"""bdl_fn_fold on the GPU (include/bdl_fn.h): over every path of its geometry
(tests/fn_fold_ref.py CASES, proven to reach them in tests/test_fn_host.py) the
probabilities are within the bound derived from the arithmetic contract of the
float64 softmax, all four accumulators equal chain_ess_ref.fold_f32 applied to
the kernel's own probabilities bit for bit, the bits do not depend on
grid_blocks or on whether probs is asked for, and the padding of a chain slot
is untouched.  Special rows sit beside ordinary rows that stay bit-exact."""
import numpy as np
import pytest
import torch

import chain_diag_ref as D
import chain_ess_ref as E
import fn_fold_ref as R

pytestmark = pytest.mark.gpu


def raw(t):
    return t.cpu().numpy().view(np.int32)


def bits(a):
    """int32 patterns with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def run_sequence(case, special, grid, with_probs):
    """The case's seven folds at b = 3 and two at b = 1 (fresh accumulators,
    bsum None) on the device.  Returns (per-fold probs or None, the b = 3
    accumulators, the b = 1 accumulators, the flags seen)."""
    from bayesdll_amd import kernels as K
    cg = R.chain_groups_of(case)
    folds = R.built(case, special)
    long_ = {nm: torch.from_numpy(v).cuda() for nm, v in R.new_acc(case).items()}
    one = {nm: torch.from_numpy(v).cuda() for nm, v in R.new_acc(case).items()}
    probs, seen = [], []
    for i in range(R.FOLDS + 2):
        x = torch.from_numpy(folds[i][0].copy()).cuda()
        p = torch.full_like(x, R.SENTINEL) if with_probs else None
        if i < R.FOLDS:
            f = K.fn_fold(x, long_["bsum"], long_["smean"], long_["sM2"], long_["bM2"],
                          sample=i + 1, batch=R.B_LONG, chain_groups=cg, probs=p, grid_blocks=grid)
        else:
            f = K.fn_fold(x, None, one["smean"], one["sM2"], one["bM2"], sample=i - R.FOLDS + 1,
                          batch=1, chain_groups=cg, probs=p, grid_blocks=grid)
        seen.append(f)
        probs.append(None if p is None else p.cpu().numpy())
    torch.cuda.synchronize()
    return probs, long_, one, seen


def check_case(case, special):
    C, P, K_ = case
    cg, n = R.chain_groups_of(case), case[0] * case[1]
    slot = 4 * cg
    folds = R.built(case, special)
    probs, long_, one, seen = run_sequence(case, special, R.GRIDS[0], True)
    assert seen == [3, 0, 12, 2, 0, 4, 2, 15, 6]
    # probabilities: within the derived bound of the float64 softmax
    for i, (x, p64, bound) in enumerate(folds):
        got = probs[i].astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(p64)), (i, "NaN rows")
        ok = ~np.isnan(p64)
        err = np.abs(got[ok] - p64[ok])
        print(f"{R.case_id(case)} fold {i}: max err / bound = {(err / bound[ok]).max():.3f}")
        assert (err <= bound[ok]).all(), (i, float((err / bound[ok]).max()))
        assert (got[ok] >= 0).all() and (got[ok] <= 1).all()
        if not special:
            assert ok.all()
    # accumulators: fold_f32 of the kernel's own probabilities, bit for bit,
    # padding and the vectors a fold does not need included
    acc, acc1 = R.new_acc(case), R.new_acc(case)
    for i in range(R.FOLDS):
        R.fold(acc, probs[i], i + 1, R.B_LONG, chain_groups=cg)
    for i in range(R.FOLDS, R.FOLDS + 2):
        R.fold(acc1, probs[i], i - R.FOLDS + 1, 1, chain_groups=cg)
    for nm in E.VECTORS:
        assert np.array_equal(bits(long_[nm].cpu().numpy()), bits(acc[nm])), nm
        assert np.array_equal(bits(one[nm].cpu().numpy()), bits(acc1[nm])), nm
    pad = np.concatenate([np.arange(slot * k + n, slot * (k + 1)) for k in range(K_)])
    for nm in E.VECTORS:
        assert (long_[nm].cpu().numpy()[pad] == np.float32(R.SENTINEL)).all(), nm
    assert (one["bsum"].cpu().numpy() == np.float32(R.SENTINEL)).all()   # never touched at b = 1
    # the same bits for every grid_blocks and with probs = None
    for grid, with_probs in ((R.GRIDS[1], True), (R.GRIDS[2], True), (R.GRIDS[0], False),
                             (R.GRIDS[1], False)):
        p2, l2, o2, _ = run_sequence(case, special, grid, with_probs)
        for nm in E.VECTORS:
            assert np.array_equal(raw(l2[nm]), raw(long_[nm])), (grid, with_probs, nm)
            assert np.array_equal(raw(o2[nm]), raw(one[nm])), (grid, with_probs, nm)
        if with_probs:
            for a, b in zip(p2, probs):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), grid
    return acc, long_, probs


def reports(case, acc, dev):
    """The finishing kernels on the device accumulators against their host
    references on the (bit-equal) host accumulators.  Returns the summaries."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    C, P, K_ = case
    cg, n = R.chain_groups_of(case), C * P
    S_, nb = R.FOLDS, R.FOLDS // R.B_LONG
    res = K.chain_ess(dev["sM2"], dev["bM2"], chains=K_, chain_groups=cg, n=n, samples=S_,
                      batches=nb, want=("ess", "mcse"))
    ess, mcse, summ = E.chain_ess_f32(acc["sM2"], acc["bM2"], chains=K_, chain_groups=cg, n=n,
                                      samples=S_, batches=nb)
    assert np.array_equal(bits(res["ess"].cpu().numpy()), bits(ess))
    assert np.array_equal(bits(res["mcse"].cpu().numpy()), bits(mcse))
    for f in ("n_eval", "n_degenerate", "n_nonfinite", "n_below", "ess_min", "argmin"):
        assert res.summary[f] == summ[f], f
    rsumm = None
    if K_ >= 2:
        rr = K.chain_diag(dev["smean"], dev["sM2"], chains=K_, chain_groups=cg, n=n,
                          var_mode=L.VAR_WELFORD, ratio=float(S_ - 1), count=S_, want=("rhat",))
        _, _, rh, rsumm = D.chain_diag_f32(acc["smean"], acc["sM2"], chains=K_, chain_groups=cg,
                                           n=n, var_mode=D.VAR_WELFORD, ratio=float(S_ - 1),
                                           inv_ratio=D.inv_of(S_ - 1), count=S_)
        assert np.array_equal(bits(rr["rhat"].cpu().numpy()), bits(rh))
        for f in ("n_eval", "n_degenerate", "n_nonfinite", "n_above", "rhat_max", "argmax"):
            assert rr.summary[f] == rsumm[f], f
    return summ, rsumm


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fold_over_every_path(case):
    C, P, K_ = case
    acc, dev, _ = check_case(case, special=False)
    summ, rsumm = reports(case, acc, dev)
    n = C * P
    if C == 1:   # p = 1 everywhere: nothing varies
        assert (summ["n_eval"], summ["n_degenerate"], summ["n_nonfinite"]) == (0, n, 0)
        if rsumm is not None:
            assert (rsumm["n_eval"], rsumm["n_degenerate"], rsumm["n_nonfinite"]) == (0, n, 0)
    else:
        assert (summ["n_eval"], summ["n_degenerate"], summ["n_nonfinite"]) == (n, 0, 0)
        if rsumm is not None:
            assert (rsumm["n_eval"], rsumm["n_degenerate"], rsumm["n_nonfinite"]) == (n, 0, 0)


@pytest.mark.parametrize("case", [(10, 9, 2), (12, 9, 3), (1000, 9, 2), (1027, 9, 2)],
                         ids=R.case_id)
def test_special_rows_beside_ordinary_rows(case):
    """A masked class, an all-equal row, an underflowing spread, a NaN row, a
    +inf row and an all -inf row (fn_fold_ref.make_logits).  check_case holds
    every row — the ordinary ones beside them included — to the bound and the
    accumulators to the bit; here the planted values and the exact counts."""
    C, P, K_ = case
    acc, dev, probs = check_case(case, special=True)
    assert (probs[0][:, 3, C // 2] == 0).all()                        # the masked class
    assert (probs[1][0, 1] == np.float32(1.0 / C)).all()             # all-equal: fl32(fl64(1 / C))
    assert probs[1][0, 2, C - 1] == 0 and probs[1][0, 2, 0] > 0.99    # e underflows to 0
    for k, r in ((0, 5), (1, 6), (0, 7)):
        assert np.isnan(probs[2][k, r]).all()
        assert np.isfinite(probs[2][1 - k, r]).all()                  # the other chain's row
    summ, rsumm = reports(case, acc, dev)
    n = C * P
    assert (summ["n_eval"], summ["n_degenerate"], summ["n_nonfinite"]) == (n - 3 * C - 1, 1, 3 * C)
    assert (rsumm["n_eval"], rsumm["n_degenerate"], rsumm["n_nonfinite"]) == (n - 3 * C - 1, 1,
                                                                               3 * C)
