"""bdl_member_score and bdl_mixture on the GPU on table P of
tests/mixture_geometry_ref.py: every instance, launch path, skip pattern and
partial count that tests/test_mixture_geometry_host.py proves P reaches, on
guarded buffers against the fp64 reference within the derived bound
(tests/mixture_ref.py); the integer rows and the one-hot rows by their literal
answers (every planted label, argmax and tie owner among them); the partials
where the restated walk says they lie; the combine bit for bit from the
partials it read; the pair limit of the grid's second dimension; skipped
components and the example after a non-finite one."""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_geometry_ref as Gm
import mixture_ref as R
import test_gpu_mixture as T
from test_gpu_mixture import run_mix, run_score

pytestmark = pytest.mark.gpu

INTS = ("n", "n_nonfinite", "n_wrong")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _arr(*vs):
    return tuple(np.array(v) for v in vs)


@pytest.fixture
def recorded(monkeypatch):
    """Every Guarded buffer run_score / run_mix make, in order (the last one is
    the workspace)."""
    made = []

    class Recorded(T.Guarded):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(T, "Guarded", Recorded)
    return made


def _parts(ws, pairs, bpp):
    """([pairs, bpp] partials of a workspace, the bytes behind them)."""
    body = ws.body()
    used = pairs * bpp * Gm.PART.itemsize
    assert used <= ws.n
    return np.frombuffer(body[:used].tobytes(), dtype=Gm.PART).reshape(pairs, bpp), body[used:]


# ------------------------------------------------------------- 1. P against the reference
@pytest.mark.parametrize("case", Gm.P, ids=Gm.case_id)
def test_every_case_and_grid_against_the_reference(case):
    x, lab, w = _arr(*Gm.random_inputs(case))
    sr, mr = Gm.references(case)
    first = None
    for grid in case.grids:
        what = (Gm.case_id(case), "grid", grid)
        rows, _ = run_score(x, lab, grid=grid)              # (guards and inputs: inside)
        R.check_scores(rows, sr, what)
        first = rows if first is None else first
        for k in INTS:                                       # the grid does not change the integers
            assert np.array_equal(rows[k], first[k]), (what, k)
        again, _ = run_score(x, lab, grid=grid)              # a fixed grid: bit-identical
        assert again.tobytes() == rows.tobytes(), what
    for mode in R.COMBINES:
        first = None
        for grid in case.grids:
            what = (Gm.case_id(case), mode, "grid", grid)
            got, _ = run_mix(x, w, case.draws, mode, grid=grid)
            R.check_mixture(got, mr[mode], what)
            first = got if first is None else first
            for k in ("n", "n_nonfinite"):
                assert np.array_equal(got["totals"][k], first["totals"][k]), (what, k)
            for k in ("logp", "expected_entropy"):           # per example: no grid in it
                assert got[k].tobytes() == first[k].tobytes(), (what, k)
            again, _ = run_mix(x, w, case.draws, mode, grid=grid)
            for k in got:
                assert again[k].tobytes() == got[k].tobytes(), (what, k)


# ------------------------------------------------------------- 2. the literal answers
@pytest.mark.parametrize("case", Gm.P, ids=Gm.case_id)
def test_integer_rows_give_their_exact_sums_and_every_plant_its_count(case):
    x, lab, nll, wrong = _arr(*Gm.integer_rows(case))
    planted = [p[1] for p in case.plants]
    for grid in case.grids:
        what = (Gm.case_id(case), "grid", grid)
        rows, _ = run_score(x, lab, grid=grid)
        assert np.array_equal(rows["nll_sum"], nll.sum(-1)), what           # exact in any order
        assert np.array_equal(rows["n_wrong"], wrong.sum(-1)), what
        assert (rows["n"] == case.B).all() and not rows["n_nonfinite"].any(), what
    # each plant on its own: the label's owner, the argmax's, the lower class of a tie
    for p in case.plants:
        b = p[1]
        path = (Gm.case_id(case), p, sorted(Gm.spot_labels(case.C, int(lab[b]))),
                sorted(Gm.tie_kinds(case.C, p[2], p[3])) if p[0] == "tie" else None)
        rows, _ = run_score(x[:, :, b:b + 1], lab[b:b + 1], grid=1)
        assert np.array_equal(rows["nll_sum"], nll[:, :, b]), path
        assert np.array_equal(rows["n_wrong"], wrong[:, :, b].astype(np.int64)), path
        if p[0] == "tie":
            assert (rows["n_wrong"] == (p[4] != p[2])).all(), path
    assert len(set(planted)) == len(planted)


@pytest.mark.parametrize("case", Gm.P, ids=Gm.case_id)
def test_one_hot_rows_give_their_literal_minus_infinity_pattern(case):
    x, _ = _arr(*Gm.one_hot_rows(case))
    w = np.array(Gm.weights(case))
    for mode in R.COMBINES:
        sets = Gm.finite_sets(case, mode)
        r = Gm.one_hot_reference(case, mode)
        for grid in case.grids:
            what = (Gm.case_id(case), mode, "grid", grid)
            got, _ = run_mix(x, w, case.draws, mode, grid=grid)
            assert not np.isnan(got["logp"]).any(), what
            assert np.array_equal(got["logp"] > -np.inf, sets), what
            assert (got["expected_entropy"] == 0).all(), what
            assert (got["totals"]["expected_entropy_sum"] == 0).all(), what
            assert (got["totals"]["n"] == case.B).all() and not got["totals"]["n_nonfinite"].any()
            R.check_mixture(got, r, what)


# ------------------------------------------------------------- 3. the partials
PARTIALS = [(Gm.P[8], 16), (Gm.P[5], 1), (Gm.P[6], 7), (Gm.P[3], 0), (Gm.P[11], 2), (Gm.P[4], 0)]


@pytest.mark.parametrize("case,grid", PARTIALS,
                         ids=["{}-grid{}".format(Gm.case_id(c), g) for c, g in PARTIALS])
def test_partials_lie_where_the_walk_says(case, grid, recorded):
    """partials[pair * bpp + x] holds exactly the rows the restatement gives
    workgroup x (the integer rows: every field exact; the mixture on the random
    rows: n and n_nonfinite); a workgroup or wave without a row adds zeros; the
    bytes behind pairs * bpp partials are never written (0xA5).  idle:block,
    uneven, and the default grids below the row slots."""
    x, lab, nll, wrong = _arr(*Gm.integer_rows(case))
    cus = _cus()
    M, G = x.shape[:2]
    run_score(x, lab, grid=grid)
    one, zero = np.ones(nll.shape, bool), np.zeros(nll.shape, bool)
    _, want = Gm.score_expected(case, grid, nll, one, zero, wrong, cus=cus)
    bpp = Gm.launch(case.C, M * G, case.B, grid, cus)
    assert want.shape == (M * G, bpp)
    got, rest = _parts(recorded[-1], M * G, bpp)
    assert got.tobytes() == want.tobytes()
    assert recorded[-1].n == M * G * (grid or Gm.MAX_GRID) * 32 and (rest == 0xA5).all()
    # the mixture: the examples of a partial, finite and not
    rx, _, w = _arr(*Gm.random_inputs(case))
    bad = Gm.references(case)[1]["arithmetic"]["nonfinite"]          # [G, B]
    run_mix(rx, w, case.draws, "arithmetic", grid=grid, want=())
    wk = Gm.walk(case.C, G, case.B, grid, cus)
    want = Gm.partials(wk, (~bad).astype(np.int64), bad.astype(np.int64),
                       np.zeros(bad.shape, np.int64), np.zeros(bad.shape))
    got, rest = _parts(recorded[-1], G, wk.bpp)
    for k in ("n", "n_nonf", "n_wrong"):
        assert np.array_equal(got[k], want[k]), k
    assert recorded[-1].n == G * (grid or Gm.MAX_GRID) * 32 and (rest == 0xA5).all()


def test_the_partial_cases_reach_what_they_are_there_for():
    cus = _cus()
    seen = set()
    for case, grid in PARTIALS:
        for pairs, entry in ((case.comps * case.draws * case.groups, "score"), (case.groups, "mix")):
            seen |= Gm.geometry_labels(case.C, pairs, case.B, grid, entry, cus)
            ipb = Gm.ipb_of(case.C)
            if grid == 0 and Gm.launch(case.C, pairs, case.B, 0, cus) < -(-case.B // ipb):
                seen.add("bpp<slots")
    assert {"idle:block", "idle:wave", "uneven", "bpp<slots", "trips:>=3"} <= seen


# ------------------------------------------------------------- 4. the combine, bit for bit
@pytest.mark.parametrize("nw", Gm.COMBINE_NW)
def test_the_combine_is_the_restated_one_bit_for_bit(nw, recorded):
    """The device struct against the restated combine of the partials read
    back from the workspace: after a RESET onto 0xA5-poisoned structs, and
    after one accumulating call on top (another batch, so other partials)."""
    from bayesdll_amd import _lib as L
    case = Gm.ROUNDING
    x, lab, w = _arr(*Gm.random_inputs(case))
    M, G, B = x.shape[:3]
    assert C.sizeof(L.MemberScore) == Gm.PART.itemsize
    rows, sc = run_score(x, lab, grid=nw, reset=True)
    parts, _ = _parts(recorded[-1], M * G, nw)
    want = Gm.combine(parts)
    assert rows.tobytes() == want.tobytes()
    assert parts["n"].sum() == rows["n"].sum() > 0 and (nw == 1 or len(set(parts["sum"][0])) > 1)
    half = B // 2 + 3
    rows2, _ = run_score(x[:, :, :half], lab[:half], grid=nw, scores=sc, reset=False)
    parts2, _ = _parts(recorded[-1], M * G, nw)
    assert rows2.tobytes() == Gm.combine(parts2, prior=want, reset=False).tobytes()
    # the mixture's totals: (n, n_nonfinite, expected_entropy_sum) of the same combine
    got, tot = run_mix(x, w, case.draws, "arithmetic", grid=nw, want=(), reset=True)
    parts, _ = _parts(recorded[-1], G, nw)
    want = Gm.combine(parts)
    for k, f in (("n", "n"), ("n_nonfinite", "n_nonf"), ("expected_entropy_sum", "sum")):
        assert got["totals"][k].tobytes() == want[f].tobytes(), k
    got2, _ = run_mix(x[:, :, :half], w, case.draws, "arithmetic", grid=nw, want=(), totals=tot,
                      reset=False)
    parts2, _ = _parts(recorded[-1], G, nw)
    want2 = Gm.combine(parts2, prior=want, reset=False)
    for k, f in (("n", "n"), ("n_nonfinite", "n_nonf"), ("expected_entropy_sum", "sum")):
        assert got2["totals"][k].tobytes() == want2[f].tobytes(), k


# ------------------------------------------------------------- 5. pairs at the limit
def test_pairs_at_the_limit_of_the_grid():
    case = Gm.PAIRS_MAX
    M, G = case.comps * case.draws, case.groups
    assert M * G == G == Gm.MAX_PAIRS == 65535 and case.grids == (1,)
    x, lab, nll, wrong = _arr(*Gm.integer_rows(case))
    rows, _ = run_score(x, lab, grid=1)
    assert rows.shape == (M, G)
    assert (rows["n"] == case.B).all() and not rows["n_nonfinite"].any()
    assert np.array_equal(rows["n_wrong"], wrong.sum(-1))
    assert np.array_equal(rows["nll_sum"], nll.sum(-1))
    assert len(np.unique(rows["nll_sum"])) > G // 2          # every pair its own sum
    xh, _ = _arr(*Gm.one_hot_rows(case))
    for mode in R.COMBINES:
        got, _ = run_mix(xh, np.array(Gm.weights(case)), case.draws, mode, grid=1)
        assert np.array_equal(got["logp"] > -np.inf, Gm.finite_sets(case, mode)), mode
        assert (got["totals"]["n"] == case.B).all() and got["totals"].shape == (G,)
        assert (got["expected_entropy"] == 0).all()


# ------------------------------------------------------------- 6. skips and breaks
SKIPS = [Gm.P[5], Gm.P[8], Gm.P[6]]


@pytest.mark.parametrize("mode", R.COMBINES)
@pytest.mark.parametrize("case", SKIPS, ids=Gm.case_id)
def test_a_skipped_component_is_never_read_and_a_bad_example_leaves_the_next_alone(case, mode):
    x, _, w = _arr(*Gm.random_inputs(case))
    r = Gm.references(case)[1][mode]
    D = case.draws
    assert {"bad:then-good", "bad:skipped"} <= Gm.labels_of(case, _cus())
    got, _ = run_mix(x, w, D, mode, grid=1)
    R.check_mixture(got, r, (Gm.case_id(case), mode))
    bad = r["nonfinite"]
    assert bad.any() and (bad[:, :-1] & ~bad[:, 1:]).any()
    # without the bad rows: every other example is the same bits
    rng = np.random.default_rng(9)
    clean = x.copy()
    rowbad = R.nonfinite_rows(x.astype(np.float64))
    clean[rowbad] = (3.0 * rng.standard_normal((int(rowbad.sum()), case.C))).astype(np.float32)
    ref, _ = run_mix(clean, w, D, mode, grid=1)
    keep = ~rowbad.any(0)                                     # [G, B]: no member row replaced
    assert np.isnan(got["logp"][bad]).all() and np.isnan(got["expected_entropy"][bad]).all()
    for k in ("logp", "expected_entropy"):
        assert got[k][keep].tobytes() == ref[k][keep].tobytes(), k
        assert np.isfinite(ref["expected_entropy"]).all()
    # NaN in every row of every skipped component: nothing changes, nothing is NaN
    filled = clean.copy()
    skipped = np.repeat(w < R.MIN_WEIGHT, D, axis=0)          # [M, G]
    assert skipped.any()
    filled[skipped] = np.nan
    for grid in case.grids:
        a, _ = run_mix(clean, w, D, mode, grid=grid)
        b, _ = run_mix(filled, w, D, mode, grid=grid)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (grid, k)
        assert not np.isnan(b["logp"]).any() and not np.isnan(b["expected_entropy"]).any()
        assert not b["totals"]["n_nonfinite"].any() and (b["totals"]["n"] == case.B).all()
