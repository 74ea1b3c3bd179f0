"""bdl_rank on the device against tests/rank_ref.py on table R: every integer
total and every per-example count exactly, ap_sum within P * 2^-52 and
bit-identical run to run, on guarded buffers (sentinels before and after every
output, the totals and the workspace), through the C entry point and through
kernels.rank."""
import ctypes as C

import numpy as np
import pytest
import torch

import rank_ref as R

pytestmark = pytest.mark.gpu
INTS = ("n_pos", "n_neg", "n_excluded", "u2", "fp_at_tpr")
COUNTS = ("ge_pos", "ge_neg", "gt_neg")
GUARD, FILL = 256, 0xA5


class Guarded:
    """nbytes of device memory between two sentinel blocks, all of it FILL."""

    def __init__(self, nbytes, dev):
        self.nbytes = int(nbytes)
        self.buf = torch.full((2 * GUARD + self.nbytes,), FILL, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + GUARD

    def body(self):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy()

    def intact(self):
        b = self.buf.cpu().numpy()
        return (b[:GUARD] == FILL).all() and (b[GUARD + self.nbytes:] == FILL).all()

    def untouched(self):
        return (self.buf.cpu().numpy() == FILL).all()


def _call(case, dev, want=COUNTS, need=0):
    """bdl_rank on a case with guarded outputs -> (totals array, {count: [rows, n]}, guards)."""
    from bayesdll_amd import _lib as L
    rows, n = case["scores"].shape
    x = torch.from_numpy(case["scores"]).to(dev)
    m = torch.from_numpy(case["marks"]).to(dev)
    g = {w: Guarded(rows * n * 4, dev) for w in COUNTS}
    g["totals"] = Guarded(rows * C.sizeof(L.RankTotals), dev)
    g["workspace"] = Guarded(L.lib().bdl_rank_workspace_bytes(rows, n), dev)
    a = L.RankArgs()
    a.scores, a.marks = x.data_ptr(), m.data_ptr()
    for w in COUNTS:
        setattr(a, w, g[w].ptr if w in want else None)
    a.totals, a.workspace = g["totals"].ptr, g["workspace"].ptr
    a.n, a.need, a.rows, a.scores_per_group = n, need, rows, case["spg"]
    a.mark_rows, a.tpr_num, a.tpr_den = case["marks"].shape[0], *R.TPR
    L.check(L.lib().bdl_rank(a, L.current_stream_handle(dev)), "bdl_rank")
    torch.cuda.synchronize(dev)
    tot = np.frombuffer(g["totals"].body().tobytes(), dtype=np.dtype(L.RankTotals))
    cnt = {w: np.frombuffer(g[w].body().tobytes(), dtype=np.uint32).reshape(rows, n)
           for w in want}
    return tot, cnt, g


def _check_totals(tot, ref, name):
    for r, want in enumerate(ref):
        for k in INTS:
            assert int(tot[r][k]) == want[k], (name, r, k, int(tot[r][k]), want[k])
        err = abs(float(tot[r]["ap_sum"]) - want["ap_sum"])
        assert err <= want["n_pos"] * 2.0 ** -52, (name, r, err)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_rank_equals_the_reference_on_guarded_buffers(name):
    dev = torch.device("cuda:0")
    case, ref = R.CASES[name], R.reference_of(name)
    tot, cnt, g = _call(case, dev)
    _check_totals(tot, ref, name)
    for r, want in enumerate(ref):
        for w in COUNTS:
            assert np.array_equal(cnt[w][r].astype(np.int64), want[w]), (name, r, w)
    assert all(v.intact() for v in g.values()), name
    # the workspace's rounding bytes are not written either
    rows, n = case["scores"].shape
    assert (g["workspace"].body()[rows * n * 12:] == FILL).all()
    # the same call again: bit-identical, ap_sum included
    tot2, cnt2, _ = _call(case, dev)
    assert tot.tobytes() == tot2.tobytes()
    assert all(np.array_equal(cnt[w], cnt2[w]) for w in COUNTS)


@pytest.mark.parametrize("name", [f"n{3 * R.ITILE + 5}-5x3-group-marks", "n257-patterns", "n1-5x1"])
def test_null_count_outputs_are_not_written(name):
    dev = torch.device("cuda:0")
    case, ref = R.CASES[name], R.reference_of(name)
    full, _, _ = _call(case, dev)
    tot, cnt, g = _call(case, dev, want=())
    assert tot.tobytes() == full.tobytes()
    assert all(g[w].untouched() for w in COUNTS) and g["totals"].intact()
    tot, cnt, g = _call(case, dev, want=("ge_neg",))
    assert tot.tobytes() == full.tobytes()
    assert g["ge_pos"].untouched() and g["gt_neg"].untouched() and g["ge_neg"].intact()
    for r, want in enumerate(ref):
        assert np.array_equal(cnt["ge_neg"][r].astype(np.int64), want["ge_neg"])


def test_an_explicit_need_is_used_for_every_row():
    dev = torch.device("cuda:0")
    name = "n257-5x3-group-marks"
    case = R.CASES[name]
    for need in (1, 7, 10 ** 6):
        tot, _, _ = _call(case, dev, want=(), need=need)
        for r in range(case["scores"].shape[0]):
            want = R.row_loop(case["scores"][r], case["marks"][R.mark_row(case, r)], need=need)
            assert int(tot[r]["fp_at_tpr"]) == want["fp_at_tpr"], (need, r)
            assert int(tot[r]["u2"]) == want["u2"]
    assert all(int(t["fp_at_tpr"]) == -1 for t in tot)  # need > P: no threshold qualifies


@pytest.mark.parametrize("name", [f"n{3 * R.ITILE + 5}-patterns", f"n{R.ITILE + 1}-5x3-group-marks",
                                  "n2-1x3-shared-marks"])
def test_kernels_rank_summary_and_shared_totals_buffer(name):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    dev = torch.device("cuda:0")
    case, ref = R.CASES[name], R.reference_of(name)
    x = torch.from_numpy(case["scores"]).to(dev)
    m = torch.from_numpy(case["marks"]).to(dev)
    rows = x.shape[0]
    res = K.rank(x, m, scores_per_group=case["spg"], counts=True)
    _check_totals(res.read(), ref, name)
    for r, (s, want) in enumerate(zip(res.summary(), ref)):
        P, Nn = want["n_pos"], want["n_neg"]
        if P and Nn:
            assert s["auroc"] == want["u2"] / (2 * P * Nn) == R.auroc(want)
            assert s["fpr"] == want["fp_at_tpr"] / Nn
        else:
            assert np.isnan(s["auroc"])
        assert (s["ap"] == s["ap_sum"] / P) if P else np.isnan(s["ap"])
        for w in COUNTS:
            assert np.array_equal(getattr(res, w)[r].cpu().numpy().astype(np.int64), want[w])
    # a slice of a shared buffer as totals; a [n] mark vector where one row is shared
    size = rows * C.sizeof(L.RankTotals)
    buf = torch.full((3 * size,), FILL, dtype=torch.uint8, device=dev)
    mm = m[0] if m.shape[0] == 1 else m
    res2 = K.rank(x, mm, scores_per_group=case["spg"], totals=buf[size:2 * size])
    assert res2.ge_pos is None and res2.read().tobytes() == res.read().tobytes()
    host = buf.cpu().numpy()
    assert (host[:size] == FILL).all() and (host[2 * size:] == FILL).all()
