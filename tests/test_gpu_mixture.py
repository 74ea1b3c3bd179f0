"""bdl_member_score and bdl_mixture on the GPU: the raw entry points on their
own guarded buffers against the fp64 reference within the derived bound
(tests/mixture_ref.py), integers exact and independent of the grid,
accumulation and RESET of the device structs, the planted rows, skipped
components, null outputs, run-to-run identity, and the anchor: all weight on
one component is kernels.predict on that component's members, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64          # bytes of 0xA5 on either side of every written buffer
GRIDS = (1, 2, 0)


class Guarded:
    """A device buffer of nbytes between two 0xA5 guards (16-B aligned)."""

    def __init__(self, nbytes, fill=0xA5):
        self.n = int(nbytes)
        self.raw = torch.full((self.n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.raw[GUARD:GUARD + self.n] = fill
        assert (self.raw.data_ptr() + GUARD) % 16 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def body(self):
        return self.raw[GUARD:GUARD + self.n].cpu().numpy()

    def intact(self):
        h = self.raw.cpu().numpy()
        return (h[:GUARD] == 0xA5).all() and (h[GUARD + self.n:] == 0xA5).all()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_score(x, lab, *, grid, scores=None, reset=True):
    """One bdl_member_score call; returns ([M, G] structured rows, the scores buffer)."""
    from bayesdll_amd import _lib as L
    M, G, B, Cn = x.shape
    h = L.lib()
    dx, dl = _dev(x), _dev(lab)
    before = dx.clone()
    sc = scores if scores is not None else Guarded(M * G * C.sizeof(L.MemberScore))
    ws = Guarded(h.bdl_member_score_workspace_bytes(M, G, grid))
    a = L.MemberScoreArgs()
    a.logits, a.labels, a.scores, a.workspace = dx.data_ptr(), dl.data_ptr(), sc.ptr, ws.ptr
    a.batch, a.members, a.groups, a.classes, a.grid_blocks = B, M, G, Cn, grid
    a.flags = L.MIXTURE_RESET if reset else 0
    L.check(h.bdl_member_score(a, L.current_stream_handle(dx.device)), "bdl_member_score")
    torch.cuda.synchronize()
    assert sc.intact() and ws.intact()
    assert torch.equal(dx.view(torch.int32), before.view(torch.int32))  # (NaN-safe)
    rows = np.frombuffer(sc.body().tobytes(), dtype=np.dtype(L.MemberScore)).reshape(M, G)
    return rows, sc


def run_mix(x, w, draws, combine, *, grid, want=("logp", "expected_entropy"), totals=None,
            reset=True):
    """One bdl_mixture call; returns ({output: host array, "totals": rows}, buffers)."""
    from bayesdll_amd import _lib as L
    M, G, B, Cn = x.shape
    h = L.lib()
    dx, dw = _dev(x), _dev(np.asarray(w, dtype=np.float64))
    bufs = {k: Guarded(G * B * (Cn if k == "logp" else 1) * 4) for k in want}
    tot = totals if totals is not None else Guarded(G * C.sizeof(L.MixtureTotals))
    ws = Guarded(h.bdl_mixture_workspace_bytes(G, grid))
    a = L.MixtureArgs()
    a.logits, a.weights = dx.data_ptr(), dw.data_ptr()
    for k in want:
        setattr(a, k, bufs[k].ptr)
    a.totals, a.workspace = tot.ptr, ws.ptr
    a.batch, a.components, a.draws, a.groups, a.classes = B, M // draws, draws, G, Cn
    a.combine, a.grid_blocks = L.MIX_COMBINE[combine], grid
    a.flags = L.MIXTURE_RESET if reset else 0
    L.check(h.bdl_mixture(a, L.current_stream_handle(dx.device)), "bdl_mixture")
    torch.cuda.synchronize()
    assert tot.intact() and ws.intact() and all(b.intact() for b in bufs.values())
    got = {k: np.frombuffer(bufs[k].body().tobytes(), dtype=np.float32).reshape(
        (G, B, Cn) if k == "logp" else (G, B)) for k in want}
    got["totals"] = np.frombuffer(tot.body().tobytes(), dtype=np.dtype(L.MixtureTotals))
    return got, tot


# ------------------------------------------------------------------ member_score
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_member_score_is_the_reference_on_every_grid(case):
    x, lab, _, sr, _ = R.built(case)
    first = None
    for grid in GRIDS:
        rows, sc = run_score(x, lab, grid=grid)
        R.check_scores(rows, sr, (R.case_id(case), grid))
        if first is None:
            first = rows
        for k in ("n", "n_nonfinite", "n_wrong"):      # the grid does not change the integers
            assert np.array_equal(rows[k], first[k]), (grid, k)
        again, _ = run_score(x, lab, grid=grid)         # a fixed grid: bit-identical
        assert again.tobytes() == rows.tobytes(), grid
        if grid == 2:  # without RESET the same call adds; with it, it overwrites
            rows2, _ = run_score(x, lab, grid=grid, scores=sc, reset=False)
            R.check_scores(rows2, sr, "added", scale=2)
            rows3, _ = run_score(x, lab, grid=1, scores=sc, reset=True)
            R.check_scores(rows3, sr, "reset")


@pytest.mark.parametrize("case", [R.CASES[4], R.CASES[9], R.CASES[15]], ids=R.case_id)
def test_member_score_over_two_calls_is_one_call_on_the_concatenated_batch(case):
    x, lab, _, sr, _ = R.built(case)
    B = x.shape[2]
    cut = B // 2 + 1
    _, sc = run_score(x[:, :, :cut], lab[:cut], grid=0)
    rows, _ = run_score(x[:, :, cut:], lab[cut:], grid=2, scores=sc, reset=False)
    R.check_scores(rows, sr, "two calls")


def test_member_score_planted_rows():
    """One member, one group, C = 6: every special row on its own."""
    inf, nan = np.inf, np.nan
    x = np.array([[0.0, 1.0, 2.0, 3.0, 4.0, 5.0],        # 0 label out of range (6): skipped
                  [0.0, 1.0, 2.0, 3.0, 4.0, 5.0],        # 1 label -1: skipped
                  [0.0, nan, 2.0, 3.0, 4.0, 5.0],        # 2 NaN
                  [0.0, 1.0, inf, 3.0, 4.0, 5.0],        # 3 +inf
                  [-inf] * 6,                            # 4 no finite entry
                  [0.0, 1.0, -inf, 3.0, 4.0, 5.0],       # 5 a masked class at the label
                  [7.0, 1.0, 7.0, 3.0, 4.0, 7.0],        # 6 a tie at the argmax, label 0: right
                  [7.0, 1.0, 7.0, 3.0, 4.0, 7.0],        # 7 the same tie, label 2: wrong
                  [0.0, 1.0, -inf, 3.0, 4.0, 5.0],       # 8 a masked class elsewhere
                  [nan] * 6],                            # 9 a NaN row under a skipped label
                 dtype=np.float32).reshape(1, 1, 10, 6)
    lab = np.array([6, -1, 0, 1, 2, 2, 0, 2, 5, 1 << 40], dtype=np.int64)
    for grid in GRIDS:
        rows, _ = run_score(x, lab, grid=grid)
        r = rows[0, 0]
        assert (r["n"], r["n_nonfinite"], r["n_wrong"]) == (4, 3, 2), grid  # wrong: rows 5, 7
        assert r["nll_sum"] == np.inf                   # row 5: -log 0
    keep = [0, 1, 2, 3, 4, 6, 7, 8, 9]
    rows, _ = run_score(x[:, :, keep], lab[keep], grid=0)
    sr = R.score_reference(x[:, :, keep], lab[keep])
    assert rows[0, 0]["n"] == 3 and np.isfinite(rows[0, 0]["nll_sum"])
    R.check_scores(rows, sr, "planted")


def test_kernels_member_score_accumulates_with_one_host_read():
    from bayesdll_amd import kernels as K
    x, lab, _, sr, _ = R.built(R.CASES[11])
    dx, dl = _dev(x), _dev(lab)
    sc = None
    for lo in range(0, x.shape[2], 4):
        sc = K.member_score(dx[:, :, lo:lo + 4].contiguous(), dl[lo:lo + 4], groups=x.shape[1],
                            scores=sc)
    R.check_scores(sc.read(), sr, "kernels.member_score")
    sc = K.member_score(dx, dl, groups=x.shape[1], scores=sc, reset=True)
    R.check_scores(sc.read(), sr, "reset")
    with pytest.raises(ValueError, match="other members / groups"):
        K.member_score(dx, dl, groups=1, scores=sc)
    with pytest.raises(ValueError, match="hold nothing yet"):
        K.MemberScores(2, 2, dx.device).read()


# ----------------------------------------------------------------------- mixture
@pytest.mark.parametrize("combine", R.COMBINES)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_mixture_is_the_reference_on_every_grid(case, combine):
    x, _, w, _, mr = R.built(case)
    r, D = mr[combine], case[3]
    for grid in GRIDS:
        got, tot = run_mix(x, w, D, combine, grid=grid)
        R.check_mixture(got, r, (R.case_id(case), combine, grid))
        again, _ = run_mix(x, w, D, combine, grid=grid)   # a fixed grid: bit-identical
        for k in got:
            assert again[k].tobytes() == got[k].tobytes(), (grid, k)
        if grid == 2:
            got2, _ = run_mix(x, w, D, combine, grid=grid, totals=tot, reset=False)
            R.check_mixture({"totals": got2["totals"]}, r, "added", scale=2)
            got3, _ = run_mix(x, w, D, combine, grid=1, totals=tot, reset=True)
            R.check_mixture({"totals": got3["totals"]}, r, "reset")
    # null outputs are not written: each output alone equals the full call's
    for only in ("logp", "expected_entropy"):
        one, _ = run_mix(x, w, D, combine, grid=0, want=(only,))
        assert one[only].tobytes() == got[only].tobytes(), only
    none, _ = run_mix(x, w, D, combine, grid=0, want=())
    assert none["totals"].tobytes() == got["totals"].tobytes()


@pytest.mark.parametrize("combine", R.COMBINES)
def test_a_skipped_component_is_not_read_and_a_weighted_one_is(combine):
    rng = np.random.default_rng(3)
    comps, D, G, B, Cn = 3, 2, 2, 5, 10
    x = (3.0 * rng.standard_normal((comps * D, G, B, Cn))).astype(np.float32)
    x[2:4] = np.nan                                     # every row of component 1
    w = np.array([[0.4, 0.3], [0.0, 9e-11], [0.6, 0.7]])
    got, _ = run_mix(x, w, D, combine, grid=0)
    r = R.mixture_reference(x, w, D, combine)
    assert not r["nonfinite"].any() and np.isfinite(got["logp"]).all()
    R.check_mixture(got, r, "skipped")
    assert [int(t["n"]) for t in got["totals"]] == [B, B]
    w[1, 1] = 1e-10                                      # at the threshold: weighted
    got, _ = run_mix(x, w, D, combine, grid=0)
    r = R.mixture_reference(x, w, D, combine)
    R.check_mixture(got, r, "weighted")
    assert np.isfinite(got["logp"][0]).all() and np.isnan(got["logp"][1]).all()
    assert np.isnan(got["expected_entropy"][1]).all()
    assert [(int(t["n"]), int(t["n_nonfinite"])) for t in got["totals"]] == [(B, 0), (0, B)]


@pytest.mark.parametrize("case", [R.CASES[2], R.CASES[7], R.CASES[9], R.CASES[11], R.CASES[15],
                                  R.CASES[18], R.CASES[19], R.CASES[20]], ids=R.case_id)
def test_all_weight_on_one_component_is_predict_on_its_members_bit_for_bit(case):
    from bayesdll_amd import kernels as K
    x, lab, _, _, _ = R.built(case)
    Cn, B, comps, D, G, _ = case
    dx, dl = _dev(x), _dev(lab)
    for c in range(comps):
        w = np.zeros((comps, G))
        w[c] = 1.0
        outs, _ = K.mixture(dx, _dev(w), dl, draws=D, groups=G, want=K.MIXTURE_OUTPUTS)
        pouts, _ = K.predict(dx[c * D:(c + 1) * D].clone(), dl, groups=G,  # (16-B aligned)
                             want=("logp", "expected_entropy"))
        for k in K.MIXTURE_OUTPUTS:
            assert torch.equal(outs[k].view(torch.int32), pouts[k].view(torch.int32)), (c, k)


def test_kernels_mixture_accumulates_with_one_host_read():
    from bayesdll_amd import kernels as K
    case = R.CASES[11]
    x, lab, w, _, mr = R.built(case)
    dx, dl, dw = _dev(x), _dev(lab), _dev(w)
    tot, pieces = None, []
    for lo in range(0, x.shape[2], 4):
        outs, tot = K.mixture(dx[:, :, lo:lo + 4].contiguous(), dw, dl[lo:lo + 4], draws=case[3],
                              groups=case[4], want=K.MIXTURE_OUTPUTS, totals=tot)
        pieces.append(outs)
    got = {k: torch.cat([p[k] for p in pieces], 1).cpu().numpy() for k in K.MIXTURE_OUTPUTS}
    got["totals"] = tot.read()
    R.check_mixture(got, mr["arithmetic"], "kernels.mixture")
    s = tot.summary()
    assert [r["n"] for r in s] == [t["n"] for t in mr["arithmetic"]["totals"]]
    with pytest.raises(ValueError, match="other groups"):
        K.mixture(dx.view(-1, 1, *dx.shape[2:]), _dev(np.ones((18, 1)) / 18), draws=1, groups=1,
                  totals=tot)
