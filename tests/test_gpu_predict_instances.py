"""bdl_predict on the GPU on table P of tests/predict_geometry_ref.py: every
instance, launch path, bin count and partial count that
tests/test_predict_geometry_host.py proves P reaches, on guarded buffers
against the fp64 reference within the derived bound (tests/predict_ref.py);
every planted maximum, tie and label by its literal answer; lanes 15 .. 63's
bins; accumulation over 1024 partials; and the partials themselves where the
restated traversal says they lie."""
import ctypes as C

import numpy as np
import pytest
import torch

import predict_geometry_ref as Gm
import predict_ref as R
import test_gpu_predict as T
from test_gpu_predict import int_view, run
from test_predict_host import check_against, check_totals

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _arrays(case, nb):
    x, lab, r, b = Gm.built(case, nb)
    return np.array(x), np.array(lab), r, b


@pytest.mark.parametrize("case", Gm.P, ids=Gm.case_id)
def test_every_case_grid_and_bin_count_against_the_reference(case):
    for nb in case.bins:
        x, lab, r, b = _arrays(case, nb)
        first = None
        for grid in case.grids:
            what = (Gm.case_id(case), "nb", nb, "grid", grid)
            outs, rows, _ = run(x, lab, grid=grid, nb=nb)    # (guards and inputs: inside)
            check_against(outs, r, b, what)
            check_totals(rows, r, b, what)
            assert (outs["pred"][r["nonfinite"]] == -1).all(), what
            for row in rows:
                assert not row["bin_count"][nb:].any() and not row["bin_hits"][nb:].any(), what
                assert not row["bin_conf"][nb:].any(), what
            ints = int_view(outs, rows)
            first = first or ints
            assert all(np.array_equal(p, q) for p, q in zip(ints[0], first[0])), what
            assert ints[1] == first[1], what
            again, rows2, _ = run(x, lab, grid=grid, nb=nb)   # a fixed geometry is bit-identical
            for w in outs:
                assert np.array_equal(outs[w].view(np.int32), again[w].view(np.int32)), (what, w)
            assert rows.tobytes() == rows2.tobytes(), what


@pytest.mark.parametrize("case", [c for c in Gm.P if c.plants], ids=Gm.case_id)
def test_every_plant_reports_its_literal_answer(case):
    nb = case.bins[0]
    x, lab, r, b = _arrays(case, nb)
    for grid in case.grids:
        outs, rows, _ = run(x, lab, grid=grid, nb=nb)
        wrong = np.zeros((case.G, case.B), bool)
        for p in case.plants:
            path = (Gm.case_id(case), "grid", grid, p, sorted(Gm.plant_labels(case, p)))
            e = Gm.expected(case, p)
            if e is None:       # the label alone, outside [0, C): unlabelled
                assert np.isnan(outs["nll"][:, p[1]]).all(), path
                continue
            ex, pred, dis, labelled, wr, lb = e
            assert outs["pred"][:, ex].tolist() == [pred] * case.G, path
            assert outs["disagree"][:, ex].tolist() == [dis] * case.G, path
            nll, conf = outs["nll"][:, ex].astype(np.float64), outs["confidence"][:, ex]
            if not labelled:
                assert np.isnan(nll).all(), path
            elif lb == pred or (p[0] == "tie" and p[2] == "pred" and lb == p[4]):
                # the label's probability is the confidence: nll = -logf(confidence), 1 ulp
                want = -np.log(conf.astype(np.float64))
                assert (np.abs(nll - want) <= 4 * R.U * np.maximum(want, 2.0 ** -20)).all(), path
            else:
                assert (nll > -np.log(conf.astype(np.float64))).all(), path
            wrong[:, ex] = wr
        # n_wrong: the planted examples' literal share plus the reference's of the others
        planted = sorted({p[1] for p in case.plants})
        for g, row in enumerate(rows):
            rest = r["totals"][g]["wrong_mask"].copy()
            rest[planted] = False
            assert int(row["n_wrong"]) == int(wrong[g].sum()) + int(rest.sum()), \
                (Gm.case_id(case), grid, g)


@pytest.mark.parametrize("case", [c for c in Gm.P if 64 in c.bins], ids=Gm.case_id)
def test_lanes_15_to_63_hold_their_bins_and_labels_are_optional(case):
    x, lab, r, b = _arrays(case, 64)
    grid = case.grids[-1]
    _, rows, _ = run(x, lab, grid=grid, nb=64, want=())
    for g, row in enumerate(rows):
        t = r["totals"][g]
        for k in range(15, 64):
            assert int(row["bin_count"][k]) == t["bin_count"][k], ("bin", k, g)
            assert int(row["bin_hits"][k]) == t["bin_hits"][k], ("bin", k, g)
        assert row["bin_count"][63] > 0 and row["bin_count"][16:63].sum() > 0
        assert row["bin_count"].sum() == t["n_labelled"] * case.C
        assert row["bin_hits"].sum() == t["n_labelled"]
    # labels = None: every bin of every lane is zero
    outs, rows, _ = run(x, lab, grid=grid, nb=64, want=("nll", "pred"), labels=False)
    assert np.isnan(outs["nll"]).all() and np.array_equal(outs["pred"], r["pred"])
    for g, row in enumerate(rows):
        assert int(row["n"]) == r["totals"][g]["n"] and int(row["n_labelled"]) == 0
        assert int(row["n_wrong"]) == 0 and row["nll_sum"] == 0 and row["mi_sum_wrong"] == 0
        assert not row["bin_count"].any() and not row["bin_hits"].any() and not row["bin_conf"].any()
        assert int(row["n_nonfinite"]) == r["totals"][g]["n_nonfinite"]


@pytest.mark.parametrize("case", Gm.BIG, ids=Gm.case_id)
def test_accumulation_over_1024_partials_and_64_bins(case):
    from bayesdll_amd import _lib as L
    x, lab, r, b = _arrays(case, 64)
    assert Gm.launch(case.C, case.G, case.B, 1024)[1] == 1024
    half = case.B // 2
    kw = dict(grid=1024, nb=64, want=("pred",))
    # RESET on a poisoned (0xA5) totals buffer, then an accumulating call on the other half
    _, _, tot = run(x[:, :, :half], lab[:half], reset=True, **kw)
    _, rows, _ = run(x[:, :, half:], lab[half:], totals=tot, reset=False, **kw)
    check_totals(rows, r, b, "halves")
    _, rows, _ = run(x, lab, totals=tot, reset=False, **kw)
    check_totals(rows, r, b, "halves + whole", scale=2)
    _, rows, _ = run(x, lab, totals=tot, reset=True, **kw)
    check_totals(rows, r, b, "reset")
    assert C.sizeof(L.PredictTotals) * case.G == tot.n


PARTIALS = [(Gm.P[5], 7), (Gm.P[0], 2), (Gm.P[0], 0), (Gm.P[6], 0), (Gm.P[1], 1)]


@pytest.mark.parametrize("case,grid_blocks", PARTIALS,
                         ids=["{}-grid{}".format(Gm.case_id(c), g) for c, g in PARTIALS])
def test_partials_lie_where_the_traversal_says(case, grid_blocks, monkeypatch):
    """partials[g * nw + r] holds exactly the examples the restatement gives
    rotated workgroup r of group g (finite, non-finite and labelled ones
    counted apart); rows from G * nw on are never written (the workspace starts
    as 0xA5 bytes).  nw < grid with G > 1, and G > grid."""
    from bayesdll_amd import _lib as L
    made = []

    class Recorded(T.Guarded):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(T, "Guarded", Recorded)
    nb = case.bins[0]
    x, lab, r, b = _arrays(case, nb)
    run(x, lab, grid=grid_blocks, nb=nb, want=())
    ws = made[-1]
    size = C.sizeof(L.PredictTotals)
    grid, nw, _ = Gm.launch(case.C, case.G, case.B, grid_blocks, _cus())
    assert ws.n == case.G * (grid_blocks or Gm.MAX_GRID) * size and case.G * nw * size <= ws.n
    assert (case.G > 1 and nw < grid) or case.G > grid
    where, count, _ = Gm.walk(case.C, case.G, case.B, grid_blocks, _cus())
    body = ws.body()
    parts = np.frombuffer(body[:case.G * nw * size].tobytes(), dtype=np.dtype(L.PredictTotals))
    assert (body[case.G * nw * size:] == 0xA5).all()
    labelled = (lab >= 0) & (lab < case.C)
    for g in range(case.G):
        for rr in range(nw):
            mine = [bb for (gg, bb), w in where.items() if gg == g and w[0] == rr]
            assert len(mine) == count[g, rr]
            bad = int(r["nonfinite"][g, mine].sum())
            p = parts[g * nw + rr]
            assert (int(p["n"]), int(p["n_nonfinite"])) == (len(mine) - bad, bad), (g, rr)
            nlab = int((labelled[mine] & ~r["nonfinite"][g, mine]).sum())
            assert int(p["n_labelled"]) == nlab and p["bin_count"].sum() == nlab * case.C, (g, rr)
            assert int(p["disagree_sum"]) == int(r["disagree"][g, mine][~r["nonfinite"][g, mine]].sum())


def test_a_probability_on_an_fp32_edge_goes_to_the_upper_bin():
    """bin = #{j : edges[j] <= pbar32} against the fp32 edges: 0.25 is the
    first of four bins' edges in fp32 (the host test holds the construction)."""
    x, lab = Gm.edge_inputs()
    em = R.emulate(x, lab, 4)
    outs, rows, _ = run(x, lab, grid=1, nb=4)
    assert outs["confidence"][0, 0] == np.float32(0.25) and outs["pred"][0, 0] == 0
    assert rows[0]["bin_count"][:5].tolist() == [0, 4, 0, 0, 0] == em["totals"][0]["bin_count"][:5].tolist()
    assert rows[0]["bin_hits"][:5].tolist() == [0, 1, 0, 0, 0]
    assert rows[0]["bin_conf"][1] == 1.0 and int(rows[0]["n_labelled"]) == 1
