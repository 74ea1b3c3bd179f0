"""bdl_predict on the GPU: the raw entry point on its own guarded buffers
against the fp64 reference within the derived bound (tests/predict_ref.py),
integers exact and independent of the geometry, accumulation and RESET of the
device totals, null outputs, untouched inputs; then the stacked samplers'
uncertainty() on top of it."""
import ctypes as C

import numpy as np
import pytest
import torch

import predict_ref as R
from test_predict_host import check_against, check_totals

pytestmark = pytest.mark.gpu

GUARD = 64          # bytes of 0xA5 on either side of every written buffer
GRIDS = (1, 2, 0)
F32 = ("logp",) + R.FLOATS
# the torch paths' own error (log_softmax and logsumexp in fp32: a few ulp each of a
# log-probability of magnitude <= 16 on the tiny net, 4 * 16 * 2^-24), allowed on top of
# the kernel's bound where the two are compared
TORCH_F32 = 4 * 16 * 2.0 ** -24


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


def run(x, lab, *, grid, nb=R.NB, want=F32 + R.INTS, totals=None, reset=True, labels=True):
    """One bdl_predict call; returns (outs as host arrays, totals rows, buffers)."""
    from bayesdll_amd import _lib as L
    M, G, B, Cn = x.shape
    h = L.lib()
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dl = torch.from_numpy(np.ascontiguousarray(lab)).cuda() if labels else None
    bufs = {w: Guarded(G * B * (Cn if w == "logp" else 1) * 4) for w in want}
    tot = totals if totals is not None else Guarded(G * C.sizeof(L.PredictTotals))
    ws = Guarded(h.bdl_predict_workspace_bytes(G, grid))
    a = L.PredictArgs()
    a.logits, a.labels = dx.data_ptr(), (dl.data_ptr() if labels else None)
    for w in want:
        setattr(a, w, bufs[w].ptr)
    a.totals, a.workspace = tot.ptr, ws.ptr
    a.batch, a.members, a.groups, a.classes, a.num_bins, a.grid_blocks = B, M, G, Cn, nb, grid
    a.flags = L.PREDICT_RESET if reset else 0
    for i, e in enumerate(R.edges32(nb)):
        a.edges[i] = float(e)
    L.check(h.bdl_predict(a, L.current_stream_handle(dx.device)), "bdl_predict")
    torch.cuda.synchronize()
    outs = {}
    for w in want:
        dt = np.int32 if w in R.INTS else np.float32
        outs[w] = bufs[w].body().view(dt).reshape((G, B, Cn) if w == "logp" else (G, B))
        assert bufs[w].intact(), w
    assert tot.intact() and ws.intact()
    # the inputs are bit-unchanged
    assert np.array_equal(dx.cpu().numpy().view(np.int32), x.view(np.int32))
    if labels:
        assert np.array_equal(dl.cpu().numpy(), lab)
    rows = np.frombuffer(tot.body().tobytes(), dtype=np.dtype(L.PredictTotals))
    return outs, rows, tot


def int_view(outs, rows):
    return ([outs[k].copy() for k in R.INTS if k in outs],
            [[int(r[k]) for k in R.INT_TOTALS] + r["bin_count"].tolist() + r["bin_hits"].tolist()
             for r in rows])


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_outputs_and_totals_against_the_reference_in_three_geometries(case):
    x, lab, r, b = R.built(case)
    x, lab = np.array(x), np.array(lab)
    what = R.case_id(case)
    seen = []
    for grid in GRIDS:
        outs, rows, _ = run(x, lab, grid=grid)
        check_against(outs, r, b, (what, grid))
        check_totals(rows, r, b, (what, grid))
        assert (outs["pred"][r["nonfinite"]] == -1).all()
        ints = int_view(outs, rows)
        seen.append(ints)
        assert all(np.array_equal(p, q) for p, q in zip(ints[0], seen[0][0])), (what, grid)
        assert ints[1] == seen[0][1], (what, grid)
        again, rows2, _ = run(x, lab, grid=grid)   # a fixed geometry is bit-identical
        for w in outs:
            assert np.array_equal(outs[w].view(np.int32), again[w].view(np.int32)), (what, grid, w)
        assert rows.tobytes() == rows2.tobytes(), (what, grid)
    if case[1] == 1:   # one member: no mutual information beyond rounding, nobody off the vote
        ok = ~r["nonfinite"]
        assert (np.abs(outs["mutual_info"][ok]) <= b["mutual_info"][ok]).all()
        assert (outs["disagree"][ok] == 0).all()


@pytest.mark.parametrize("case", [R.CASES[4], R.CASES[13]], ids=R.case_id)
def test_two_accumulating_calls_equal_one_and_reset_overwrites(case):
    x, lab, r, b = R.built(case)
    x, lab = np.array(x), np.array(lab)
    from bayesdll_amd import _lib as L
    B = x.shape[2]
    half = B // 2
    # RESET on a poisoned (0xA5) totals buffer, then an accumulating call on the other half
    _, _, tot = run(x[:, :, :half], lab[:half], grid=2, reset=True)
    _, rows, _ = run(x[:, :, half:], lab[half:], grid=2, totals=tot, reset=False)
    check_totals(rows, r, b, "halves")
    # accumulating the whole batch once more doubles everything
    _, rows, _ = run(x, lab, grid=0, totals=tot, reset=False)
    check_totals(rows, r, b, "halves + whole", scale=2)
    # RESET overwrites what has accumulated
    _, rows, _ = run(x, lab, grid=1, totals=tot, reset=True)
    check_totals(rows, r, b, "reset")
    assert C.sizeof(L.PredictTotals) * x.shape[1] == tot.n


def test_null_outputs_stay_untouched_and_labels_are_optional():
    case = R.CASES[11]
    x, lab, r, b = R.built(case)
    x, lab = np.array(x), np.array(lab)
    for want in (("pred",), ("logp", "nll"), ()):
        outs, rows, _ = run(x, lab, grid=2, want=want)
        check_totals(rows, r, b, want)
        for w in want:
            if w in R.INTS:
                assert np.array_equal(outs[w], r[w])
    outs, rows, _ = run(x, lab, grid=2, want=("nll", "entropy"), labels=False)
    assert np.isnan(outs["nll"]).all()
    assert (np.abs(outs["entropy"] - r["entropy"]) <= b["entropy"]).all()
    for g, row in enumerate(rows):
        assert int(row["n"]) == r["totals"][g]["n"] and int(row["n_labelled"]) == 0
        assert int(row["n_wrong"]) == 0 and row["bin_count"].sum() == 0 and row["nll_sum"] == 0
        assert abs(row["mi_sum"] - r["totals"][g]["mi_sum"]) <= b["totals"][g]["mi_sum"]


def test_kernels_predict_accumulates_over_calls_with_one_host_read():
    from bayesdll_amd import kernels as K
    case = R.CASES[4]
    x, lab, r, b = R.built(case)
    M, G, B, Cn = x.shape
    dx, dl = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(lab)).cuda()
    tot = None
    pieces = []
    for lo in range(0, B, 50):
        xs = dx[:, :, lo:lo + 50].contiguous()
        outs, tot = K.predict(xs, dl[lo:lo + 50], groups=G, totals=tot, num_bins=R.NB,
                              want=K.PREDICT_OUTPUTS)
        pieces.append(outs)
    got = {w: torch.cat([p[w] for p in pieces], 1).cpu().numpy() for w in K.PREDICT_OUTPUTS}
    check_against(got, r, b, "kernels.predict")
    check_totals(tot.read(), r, b, "kernels.predict")
    s = tot.summary()
    assert len(s) == G
    for g, t in enumerate(r["totals"]):
        assert s[g]["n"] == t["n"] and s[g]["n_nonfinite"] == t["n_nonfinite"]
        assert s[g]["error"] == t["n_wrong"] / t["n_labelled"]
        assert abs(s[g]["nll"] - t["nll_sum"] / t["n_labelled"]) <= b["totals"][g]["nll_sum"]
        assert s[g]["disagreement"] == t["disagree_sum"] / (t["n"] * M)
    # pooled: the same buffer reinterpreted as one group of M * G members
    outs, tot1 = K.predict(dx, dl, groups=1, num_bins=R.NB)
    r1 = R.reference(np.array(x).reshape(M * G, 1, B, Cn), lab, R.NB)
    b1 = R.bound(r1, lab)
    check_against({w: v.cpu().numpy() for w, v in outs.items()}, r1, b1, "pooled")
    check_totals(tot1.read(), r1, b1, "pooled")
    with pytest.raises(ValueError, match="other groups"):
        K.predict(dx, dl, groups=G, totals=tot1)


# ------------------------------------------------------------------ the samplers
from test_gpu_chain_diag import Net, _args, loader  # noqa: E402,F401  (loader: a fixture)


def _independent_logits(S, loader):
    """[members, K, B, C] per batch, rebuilt through `_components` from the
    draw counter the caller restored (eval mode, as uncertainty())."""
    st = S.state
    out = []
    was = S.net.training
    S.net.eval()
    try:
        with torch.no_grad():
            for x, _ in loader:
                buf = torch.empty_like(st.theta)
                views = {nm: buf.view(S.K, st.stride)[:, o:o + k].view(S.K, *s)
                         for nm, o, k, s in zip(st.names, st.offsets, st.numels, st.shapes)}
                comps = [S._fwd(views, x).clone() for _ in S._components(buf)]
                if not comps:
                    comps = [S.chain_logits(x)]
                out.append(torch.stack(comps, 0).cpu().numpy())
    finally:
        S.net.train(was)
    return out


@pytest.mark.parametrize("cls", ["StackedSGLD", "StackedCSGHMC"])
def test_sampler_uncertainty_is_the_reference_on_its_members(cls, loader):
    from bayesdll_amd import stacked
    torch.manual_seed(21)
    S = getattr(stacked, cls)(Net().cuda(), 4, _args(ece_num_bins=10), init="reinit", seed=4,
                              chain0=3, graph=False)
    S.train_one_epoch(loader, 0)
    ys = torch.cat([y for _, y in loader]).cpu().numpy()
    d0 = S.draws
    u = S.uncertainty(loader, per_example=True)
    d1 = S.draws
    S.draws = d0
    nll, err = S.evaluate(loader)
    assert S.draws == d1 and d1 > d0           # advanced exactly as evaluate advances it
    S.draws = d0
    lg = _independent_logits(S, loader)
    assert S.draws == d1
    full = np.concatenate(lg, 2)               # [members, K, N, C]
    Mm, K_, N, Cn = full.shape
    pooled = full.reshape(Mm * K_, 1, N, Cn)
    r = R.reference(pooled, ys, 10)
    b = R.bound(r, ys)
    t, bt = r["totals"][0], b["totals"][0]
    assert u["n"] == t["n"] == N and u["n_nonfinite"] == 0 and u["members"] == Mm * K_
    assert u["error"] == t["n_wrong"] / N
    assert abs(u["nll"] - t["nll_sum"] / N) <= bt["nll_sum"] / N
    for k, f in (("entropy", "entropy_sum"), ("expected_entropy", "expected_entropy_sum"),
                 ("mutual_info", "mi_sum")):
        assert abs(u[k] - t[f] / N) <= bt[f] / N, k
    assert u["disagreement"] == t["disagree_sum"] / (N * Mm * K_)
    assert u["bins"]["count"] == t["bin_count"][:10].tolist()
    assert u["bins"]["hits"] == t["bin_hits"][:10].tolist()
    assert 0 <= u["ece"] <= u["mce"] <= 1
    check_against({k: u["per_example"][k].cpu().numpy() for k in R.FLOATS + R.INTS}, r, b, cls)
    # evaluate()'s fp32 composition agrees within the bound plus its own fp32 error
    assert abs(u["nll"] - nll) <= bt["nll_sum"] / N + TORCH_F32 and abs(u["error"] - err) < 1e-12
    # by chain: K mixtures, against evaluate_chains
    S.draws = d0
    uc = S.uncertainty(loader, by_chain=True)
    assert S.draws == d1
    S.draws = d0
    cn, ce = S.evaluate_chains(loader)
    rc = R.reference(full, ys, 10)
    bc = R.bound(rc, ys)
    for k in range(K_):
        tk = rc["totals"][k]
        assert uc["error"][k] == tk["n_wrong"] / N == ce[k]
        assert abs(uc["nll"][k] - tk["nll_sum"] / N) <= bc["totals"][k]["nll_sum"] / N
        assert abs(uc["nll"][k] - cn[k]) <= bc["totals"][k]["nll_sum"] / N + TORCH_F32
        assert uc["bins"][k]["count"] == tk["bin_count"][:10].tolist()
    assert len(uc["mutual_info"]) == K_ and uc["members"] == Mm


def test_sampler_uncertainty_before_any_collect_and_with_per_chain(loader):
    from bayesdll_amd import stacked
    torch.manual_seed(22)
    S = stacked.StackedSGLD(Net().cuda(), 3, _args(), init="reinit", seed=4, graph=False,
                            per_chain={"lr": [1e-2, 5e-2, 1e-1]})
    d0 = S.draws
    u = S.uncertainty(loader[:2])              # the chains' current theta: K members
    assert S.draws == d0 and u["members"] == 3 and u["n"] == 32 and len(u["bins"]["count"]) == 15
    S.train_one_epoch(loader, 0)
    d0 = S.draws
    uc = S.uncertainty(loader[:2], by_chain=True)
    assert len(uc["nll"]) == 3 and all(np.isfinite(uc["nll"]))
    d1, S.draws = S.draws, d0                  # the same draws again
    nll, err = S.evaluate_chains(loader[:2])
    assert S.draws == d1 > d0
    assert np.allclose(uc["nll"], nll, atol=1e-5) and np.array_equal(uc["error"], err)
