"""bdl_diversity on the device against tests/diversity_ref.py on table D: every
integer exactly at three grid_blocks values, tv_sum exactly on the dyadic
cases, tv_sum / kl_sum entry by entry within the derived bound elsewhere, on
guarded buffers (sentinels around the totals and the workspace); accumulation
over calls, reset, run-to-run bit identity, every refusal, kernels.diversity."""
import numpy as np
import pytest
import torch

import diversity_ref as R
from test_diversity_host import check_refusals
from test_gpu_rank import FILL, Guarded

pytestmark = pytest.mark.gpu


def _grid(case, g, dev):
    from bayesdll_amd import kernels as K
    return g or K.diversity_default_grid(case[0], case[1], case[2], dev)


def _call(x, lab, grid, dev, guards=None, reset=True):
    """bdl_diversity with guarded totals and workspace -> (totals record, guards)."""
    from bayesdll_amd import _lib as L
    P, B, C = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ld = None if lab is None else torch.from_numpy(np.ascontiguousarray(lab)).to(dev)
    h = L.lib()
    if guards is None:
        guards = {"totals": Guarded(h.bdl_diversity_totals_bytes(P), dev)}
    guards["workspace"] = Guarded(h.bdl_diversity_workspace_bytes(P, grid), dev)
    a = L.DiversityArgs()
    a.logits, a.labels = xd.data_ptr(), (None if ld is None else ld.data_ptr())
    a.totals, a.workspace = guards["totals"].ptr, guards["workspace"].ptr
    a.batch, a.voters, a.classes, a.grid_blocks = B, P, C, grid
    a.flags = L.DIVERSITY_RESET if reset else 0
    L.check(h.bdl_diversity(a, L.current_stream_handle(dev)), "bdl_diversity")
    torch.cuda.synchronize(dev)
    tot = np.frombuffer(guards["totals"].body().tobytes(), dtype=L.diversity_totals_dtype(P))[0]
    return tot, guards


def _check(tot, ref, what, exact_tv=False):
    assert int(tot["voters"]) == ref["disagree"].shape[0], what
    for k in R.HEADER:
        assert int(tot[k]) == ref[k], (what, k, int(tot[k]), ref[k])
    for k in R.INTS:
        assert np.array_equal(tot[k], ref[k]), (what, k)
    worst = 0.0
    for k in R.SUMS:
        err, b = np.abs(tot[k] - ref[k]), ref["bound"][k]
        assert np.isfinite(tot[k]).all(), (what, k)
        ratio = float((err / np.maximum(b, 1e-300)).max())
        print(f"{what} {k}: largest error / bound = {ratio:.3g}")
        assert (err <= b).all(), (what, k, ratio)
        worst = max(worst, ratio)
    if exact_tv:
        assert np.array_equal(tot["tv_sum"], ref["tv_sum"]), what
    return worst


@pytest.mark.parametrize("case", R.D, ids=R.case_id)
def test_diversity_equals_the_reference_at_three_grids(case):
    dev = torch.device("cuda:0")
    x, lab, ref = R.built(case)
    for g in R.GRIDS:
        grid = _grid(case, g, dev)
        tot, guards = _call(x, lab, grid, dev)
        _check(tot, ref, f"{R.case_id(case)} grid {grid}", exact_tv=case[4] == "dyadic")
        assert all(v.intact() for v in guards.values()), (case, grid)
        # symmetric cells hold the same bits, the diagonals their constants
        assert np.array_equal(tot["tv_sum"], tot["tv_sum"].T)
        assert not np.diag(tot["tv_sum"]).any() and not np.diag(tot["kl_sum"]).any()
        # the same call again: bit-identical, the fp64 sums included
        tot2, _ = _call(x, lab, grid, dev)
        assert tot.tobytes() == tot2.tobytes(), (case, grid)


@pytest.mark.parametrize("case", [R.D[3], R.D[10], R.D[18]], ids=R.case_id)
def test_two_accumulated_calls_equal_one_on_the_concatenated_batch(case):
    dev = torch.device("cuda:0")
    x, lab, ref = R.built(case)
    cut = x.shape[1] // 2 + 1
    grid = _grid(case, 0, dev)
    guards = {"totals": Guarded(int(32 + 40 * x.shape[0] ** 2), dev)}
    _call(x[:, :cut], None if lab is None else lab[:cut], grid, dev, guards, reset=True)
    tot, _ = _call(x[:, cut:], None if lab is None else lab[cut:], 3, dev, guards, reset=False)
    _check(tot, ref, f"{R.case_id(case)} two calls")
    one, _ = _call(x, lab, grid, dev)
    for k in R.HEADER + R.INTS:
        assert np.array_equal(tot[k], one[k]), k
    # reset: the second half alone overwrites what the totals held
    half = R.reference(x[:, cut:], None if lab is None else lab[cut:], want_bound=True)
    tot, g = _call(x[:, cut:], None if lab is None else lab[cut:], 3, dev, guards, reset=True)
    _check(tot, half, f"{R.case_id(case)} reset")
    assert guards["totals"].intact() and g["workspace"].intact()


def test_every_refusal_by_its_status_code():
    check_refusals()


@pytest.mark.parametrize("case", [R.D[3], R.D[12], R.D[18]], ids=R.case_id)
def test_kernels_diversity_handle_and_summary(case):
    from bayesdll_amd import kernels as K
    dev = torch.device("cuda:0")
    x, lab, ref = R.built(case)
    xd = torch.from_numpy(x).to(dev)
    ld = None if lab is None else torch.from_numpy(lab).to(dev)
    tot = K.DiversityTotals(x.shape[0], dev)
    with pytest.raises(ValueError, match="hold nothing yet"):
        tot.read()
    tot.buf.fill_(FILL)                                   # the first call resets
    cut = 5
    assert K.diversity(xd[:, :cut].contiguous(), None if ld is None else ld[:cut], totals=tot) \
        is tot
    K.diversity(xd[:, cut:].contiguous(), None if ld is None else ld[cut:], totals=tot,
                grid_blocks=2)
    _check(tot.read(), ref, R.case_id(case))
    s = tot.summary()
    n, nl = ref["n"], ref["n_labelled"]
    assert (s["n"], s["n_labelled"], s["n_nonfinite"]) == (n, nl, ref["n_nonfinite"])
    assert np.array_equal(s["disagreement"], ref["disagree"] / n)
    assert np.array_equal(s["kl_unbounded"], ref["kl_unbounded"])
    if nl:
        assert np.array_equal(s["error"], np.diag(ref["both_wrong"]) / nl)
    else:
        assert np.isnan(s["error"]).all()
    assert np.allclose(s["tv"], ref["tv_sum"] / n, rtol=1e-5, atol=1e-7)
    with pytest.raises(ValueError, match="other voters"):
        K.diversity(xd[:2].contiguous(), ld, totals=tot)
    one = K.diversity(xd, ld, totals=tot, reset=True).read()
    assert int(one["n"]) == n and np.array_equal(one["disagree"], ref["disagree"])
