"""bdl_chain_diag_layers / bdl_chain_ess_layers on the GPU: every row of the
per-tensor tables equals the host reference (tests/layers_ref.py: the
whole-vector references, which the device equals bit for bit, on the tensor's
slice) — integer fields, extreme and arg exactly, the fp64 sum within its
derived bound —, the exact fields do not depend on the launch geometry, the
rows add up to the whole-vector call on the same buffers, nothing around the
table, the workspace or inside the slot padding is touched, and the stacked
samplers' by_tensor keyword and the command line are those kernels on the
samplers' own moments / accumulators.

tests/test_layers_host.py shows on the CPU that table L and table A reach the
segment kinds claimed here at grid 2 and at the default grid, and that the
reference's rows are of the intended kinds."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_diag_ref as DR
import chain_ess_ref as ER
import layers_ref as R
from test_gpu_chain_diag import Net, _args, loader  # noqa: F401  (loader: a fixture)

pytestmark = pytest.mark.gpu

GUARD = 4096                     # bytes of 0xA5 before and after the table and the workspace
CASES = [("l", 2), ("l", 5), ("a", 3)]   # table L: the unrolled chain loop without / with a remainder
MODES = [("welford_recip", DR.VAR_WELFORD, 6.0, True), ("welford", DR.VAR_WELFORD, 6.0, False),
         ("raw", DR.VAR_RAW_MOMENTS, 7 / 6, False)]   # cSGHMC's Welford M2, SGLD's running moments
DIAG = dict(kind="diag", ints=R.DIAG_INT, ext="rhat_max", total="rhat_sum", arg="argmax",
            hits="n_above")
ESS = dict(kind="ess", ints=R.ESS_INT, ext="ess_min", total="ess_sum", arg="argmin",
           hits="n_below")


def table(name):
    return R.table_l() if name == "l" else R.table_a()


@functools.lru_cache(maxsize=None)
def diag_case(name, K_, mode):
    """(table, mom1, mom2, scalars, reference rows): computed once, never modified."""
    _, var_mode, ratio, recip = MODES[mode]
    tab = table(name)
    m1, m2 = R.diag_inputs(tab, K_, var_mode, ratio)
    kw = dict(var_mode=var_mode, ratio=ratio, inv_ratio=DR.inv_of(ratio) if recip else 0.0,
              var_floor=0.0, count=R.COUNT)
    rows = R.diag_layers_ref(m1, m2, tab.segments, chains=K_, chain_groups=tab.chain_groups, **kw)
    for a in (m1, m2):
        a.setflags(write=False)
    return tab, m1, m2, kw, rows


@functools.lru_cache(maxsize=None)
def ess_case(name, K_):
    tab = table(name)
    sM2, bM2 = R.ess_inputs(tab, K_)
    for a in (sM2, bM2):
        a.setflags(write=False)
    return tab, sM2, bM2


def launch(spec, tab, v0, v1, K_, grid, *, segments=None, partials=False, **scalars):
    """One raw call of the entry point on buffers of this test's own: the
    table and the workspace each lie between two guards of 0xA5 bytes.  Returns
    the table as a structured array after checking the guards and that the
    inputs (slot padding included) are bit-unchanged (partials=True: also the
    workspace's [nsegments, workgroups] partials)."""
    from bayesdll_amd import _lib as L
    h = L.lib()
    segs = tab.segments if segments is None else segments
    nseg = len(segs)
    struct = L.DiagSummary if spec["kind"] == "diag" else L.EssSummary
    tb = nseg * C.sizeof(struct)
    wsb = int(h.bdl_layers_workspace_bytes(nseg, grid))
    assert wsb == nseg * (grid or L.LAYERS_MAX_GRID) * C.sizeof(struct)
    d0, d1 = torch.from_numpy(np.array(v0)).cuda(), torch.from_numpy(np.array(v1)).cuda()
    dseg = torch.tensor(segs, dtype=torch.int64).cuda()
    tbuf = torch.full((GUARD + tb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    wbuf = torch.full((GUARD + wsb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    a = L.DiagLayersArgs() if spec["kind"] == "diag" else L.EssLayersArgs()
    if spec["kind"] == "diag":
        a.mom1, a.mom2 = d0.data_ptr(), d1.data_ptr()
        a.var_mode, a.ratio, a.inv_ratio = scalars["var_mode"], scalars["ratio"], scalars["inv_ratio"]
        a.var_floor, a.c1 = scalars["var_floor"], (scalars["count"] - 1) / scalars["count"]
        thr = DR.THRESHOLDS
    else:
        a.sM2, a.bM2 = d0.data_ptr(), d1.data_ptr()
        a.samples, a.batches = scalars["samples"], scalars["batches"]
        thr = ER.THRESHOLDS
    for i, t in enumerate(thr):
        a.thresholds[i] = t
    a.segments, a.table, a.workspace = dseg.data_ptr(), tbuf.data_ptr() + GUARD, wbuf.data_ptr() + GUARD
    a.n, a.chain_groups, a.chains, a.nsegments, a.grid_blocks = (tab.n, tab.chain_groups, K_, nseg,
                                                                 grid)
    fn = getattr(h, f"bdl_chain_{spec['kind']}_layers")
    L.check(fn(a, L.current_stream_handle(d0.device)), fn.__name__)
    torch.cuda.synchronize()
    for buf, nb, what in ((tbuf, tb, "table"), (wbuf, wsb, "workspace")):
        host = buf.cpu().numpy()
        assert (host[:GUARD] == 0xA5).all() and (host[GUARD + nb:] == 0xA5).all(), what
    for d, v in ((d0, v0), (d1, v1)):                    # inputs and slot padding: bit-unchanged
        assert np.array_equal(d.cpu().numpy().view(np.int32), np.asarray(v).view(np.int32))
    assert dseg.cpu().tolist() == [list(s) for s in segs]
    out = np.frombuffer(tbuf.cpu().numpy()[GUARD:GUARD + tb].tobytes(), dtype=np.dtype(struct))
    if not partials:
        return out
    used = grid or min(2 * torch.cuda.get_device_properties(0).multi_processor_count,
                       L.LAYERS_MAX_GRID)
    raw = wbuf.cpu().numpy()[GUARD:GUARD + nseg * used * C.sizeof(struct)].tobytes()
    return out, np.frombuffer(raw, dtype=np.dtype(struct)).reshape(nseg, used)


def exact(spec, row):
    return tuple([row[f].tolist() if f == spec["hits"] else int(row[f]) for f in spec["ints"]]
                 + [float(row[spec["ext"]])])


def check_rows(spec, tab, got, want):
    assert len(got) == len(want) == len(tab.names)
    for nm, (o, m), g, w in zip(tab.names, tab.segments, got, want):
        for f in spec["ints"]:
            gv = g[f].tolist() if f == spec["hits"] else int(g[f])
            assert gv == w[f], (nm, f, gv, w[f])
        assert float(g[spec["ext"]]) == w["ext"], (nm, float(g[spec["ext"]]), w["ext"])
        # an fp64 sum of numel fp32 values in any order against the exactly rounded sum
        assert abs(float(g[spec["total"]]) - w["sum"]) <= m * 2.0 ** -52 * w["sum_abs"], nm
        assert float(g["pad"]) == 0.0


def check_adds_up(spec, got, whole):
    """The rows against the whole-vector summary of the same buffers."""
    for f in ("n_eval", "n_degenerate", "n_nonfinite"):
        assert int(got[f].sum()) == whole[f], f
    assert got[spec["hits"]].sum(axis=0).tolist() == whole[spec["hits"]]
    ev = got[got["n_eval"] > 0]
    best = ev[spec["ext"]].max() if spec is DIAG else ev[spec["ext"]].min()
    assert float(best) == whole[spec["ext"]]
    first = ev[ev[spec["ext"]] == best][0]
    assert int(first[spec["arg"]]) == whole[spec["arg"]]


# ------------------------------------------------------------------- R-hat
@pytest.mark.parametrize("mode", range(len(MODES)), ids=[m[0] for m in MODES])
@pytest.mark.parametrize("name,K_", CASES)
def test_diag_table_equals_the_reference(name, K_, mode):
    from bayesdll_amd import kernels as K
    tab, m1, m2, kw, want = diag_case(name, K_, mode)
    small = launch(DIAG, tab, m1, m2, K_, 2, **kw)
    check_rows(DIAG, tab, small, want)
    dflt = launch(DIAG, tab, m1, m2, K_, 0, **kw)
    check_rows(DIAG, tab, dflt, want)
    assert [exact(DIAG, r) for r in small] == [exact(DIAG, r) for r in dflt]
    # constructed rows, on the device
    by = dict(zip(tab.names, dflt))
    fz = by[tab.frozen]
    assert (int(fz["n_degenerate"]), float(fz["rhat_max"]), int(fz["argmax"])) == \
        (tab.span(tab.frozen)[1], 0.0, -1) and int(fz["n_eval"]) == 0
    if tab.flat:
        assert int(by[tab.flat]["n_nonfinite"]) == tab.span(tab.flat)[1]
        assert int(by["hbt"]["n_nonfinite"]) == 3
        assert int(by["odd"]["n_nonfinite"]) == int(by["big"]["n_nonfinite"]) == 0
    # the wrapper (its own table and workspace), and the whole-vector call on the same buffers
    d1, d2 = torch.from_numpy(np.array(m1)).cuda(), torch.from_numpy(np.array(m2)).cuda()
    seg = torch.tensor(tab.segments, dtype=torch.int64).cuda()
    _, var_mode, ratio, recip = MODES[mode]
    pk = dict(chains=K_, chain_groups=tab.chain_groups, n=tab.n, var_mode=var_mode, ratio=ratio,
              count=R.COUNT, var_floor=0.0, div_mode="recip" if recip else "true")
    wrapped = K.chain_diag_layers(d1, d2, seg, **pk)
    assert wrapped.dtype == dflt.dtype and wrapped.tobytes() == dflt.tobytes()
    check_adds_up(DIAG, dflt, K.chain_diag(d1, d2, want=(), **pk).summary)


# --------------------------------------------------------------------- ESS
@pytest.mark.parametrize("name,K_", CASES)
def test_ess_table_equals_the_reference(name, K_):
    from bayesdll_amd import kernels as K
    tab, sM2, bM2 = ess_case(name, K_)
    kw = dict(samples=R.SAMPLES, batches=R.BATCHES)
    want = R.ess_layers_ref(sM2, bM2, tab.segments, chains=K_, chain_groups=tab.chain_groups, **kw)
    small = launch(ESS, tab, sM2, bM2, K_, 2, **kw)
    check_rows(ESS, tab, small, want)
    dflt = launch(ESS, tab, sM2, bM2, K_, 0, **kw)
    check_rows(ESS, tab, dflt, want)
    assert [exact(ESS, r) for r in small] == [exact(ESS, r) for r in dflt]
    by = dict(zip(tab.names, dflt))
    fz = by[tab.frozen]
    assert (int(fz["n_degenerate"]), float(fz["ess_min"]), int(fz["argmin"])) == \
        (tab.span(tab.frozen)[1], 0.0, -1) and int(fz["n_eval"]) == 0
    if tab.flat:
        assert int(by[tab.flat]["n_nonfinite"]) == tab.span(tab.flat)[1]
        assert int(by["hbt"]["n_nonfinite"]) == 3
        assert int(by["odd"]["n_nonfinite"]) == int(by["big"]["n_nonfinite"]) == 0
    d1, d2 = torch.from_numpy(np.array(sM2)).cuda(), torch.from_numpy(np.array(bM2)).cuda()
    seg = torch.tensor(tab.segments, dtype=torch.int64).cuda()
    pk = dict(chain_groups=tab.chain_groups, n=tab.n, **kw)
    wrapped = K.chain_ess_layers(d1, d2, seg, chains=K_, **pk)
    assert wrapped.dtype == dflt.dtype and wrapped.tobytes() == dflt.tobytes()
    check_adds_up(ESS, dflt, K.chain_ess(d1, d2, chains=K_, **pk).summary)
    # chains = 1 over chain k's slice: that chain alone
    for k in range(K_):
        o = tab.slot * k
        one = R.ess_layers_ref(sM2[o:], bM2[o:], tab.segments, chains=1,
                               chain_groups=tab.chain_groups, **kw)
        got = K.chain_ess_layers(d1[o:], d2[o:], seg, chains=1, grid_blocks=2 if k % 2 else 0, **pk)
        check_rows(ESS, tab, got, one)


@pytest.mark.parametrize("grid", [2, 0])
def test_partials_lie_where_the_traversal_says(grid):
    """Workgroup w's partial of segment i counts exactly the elements
    layers_ref.classify gives it — the rotation, the head / tail owner, the
    block iterations — and a workgroup that takes no part stores an empty one
    (the workspace starts as 0xA5 bytes).  This ties the CPU proof of what the
    tables reach to the device's own traversal."""
    tab, m1, m2, kw, _ = diag_case("l", 5, 0)
    _, parts = launch(DIAG, tab, m1, m2, 5, grid, partials=True, **kw)
    used = parts.shape[1]
    assert used == (grid or used) and used >= 2
    c = R.classify(tab.segments, tab.n, used)
    for i in range(len(tab.segments)):
        for w in range(used):
            p, k = parts[i, w], c[w, i]
            n = int(p["n_eval"]) + int(p["n_degenerate"]) + int(p["n_nonfinite"])
            assert n == k["head"] + k["body"] + k["tail"], (i, w, n, k)
            if not k["part"]:
                assert (int(p["argmax"]), float(p["rhat_max"]), float(p["rhat_sum"])) == \
                    (2 ** 63 - 1, -1.0, 0.0), (i, w)


def test_one_segment_over_the_whole_vector_is_the_whole_vector_summary():
    """A table of one row [0, n): the row IS bdl_chain_diag's / bdl_chain_ess's
    summary (sum apart: another order of the same fp64 additions)."""
    from bayesdll_amd import kernels as K
    tab, m1, m2, kw, _ = diag_case("l", 5, 0)
    row = launch(DIAG, tab, m1, m2, 5, 0, segments=[(0, tab.n)], **kw)[0]
    d1, d2 = torch.from_numpy(np.array(m1)).cuda(), torch.from_numpy(np.array(m2)).cuda()
    whole = K.chain_diag(d1, d2, want=(), chains=5, chain_groups=tab.chain_groups, n=tab.n,
                         var_mode=kw["var_mode"], ratio=kw["ratio"], count=R.COUNT, var_floor=0.0,
                         div_mode="recip").summary
    for f in R.DIAG_INT:
        assert (row[f].tolist() if f == "n_above" else int(row[f])) == whole[f], f
    assert float(row["rhat_max"]) == whole["rhat_max"]
    assert abs(float(row["rhat_sum"]) - whole["rhat_sum"]) <= tab.n * 2.0 ** -52 * whole["rhat_sum"]


# -------------------------------------------------------------- end to end
def _rows_equal(spec, names, numels, got, want):
    assert [r["name"] for r in got] == names and [r["numel"] for r in got] == numels
    for g, w, m in zip(got, want, numels):
        for f in spec["ints"]:
            assert g[f] == w[f], (g["name"], f)
        assert g[spec["ext"]] == w["ext"]
        mean = spec["ext"].split("_")[0] + "_mean"
        share = "share_" + spec["hits"].split("_")[1]
        if w["n_eval"]:
            # the sum's bound (numel * 2^-52 * sum|x|) and the two roundings of / and *
            assert abs(g[mean] * w["n_eval"] - w["sum"]) <= m * 2.0 ** -51 * w["sum_abs"]
            assert g[share] == [v / w["n_eval"] for v in w[spec["hits"]]]
        else:
            assert np.isnan(g[mean])


@pytest.mark.parametrize("cls", ["StackedSGLD", "StackedCSGHMC"])
def test_sampler_by_tensor_is_the_kernels_on_its_own_vectors(cls, loader):  # noqa: F811
    from bayesdll_amd import kernels as K
    from bayesdll_amd import stacked
    torch.manual_seed(31)
    S = getattr(stacked, cls)(Net().cuda(), 3, _args(), init="reinit", seed=4, graph=False,
                              ess_batch=2)
    S.train_one_epoch(loader, 0)
    st = S.state
    segs = list(zip(st.offsets, st.numels))
    assert st.layer_segments().cpu().tolist() == [list(s) for s in segs]
    m1, m2, var_mode, ratio, count = S._moment_spec(S._latest_component())
    plain = S.diagnostics()
    d = S.diagnostics(by_tensor=True)
    assert {k: v for k, v in d.items() if k != "by_tensor"} == plain
    recip = K.DIV_MODE == "recip"
    want = R.diag_layers_ref(m1.cpu().numpy(), m2.cpu().numpy(), segs, chains=3,
                             chain_groups=st.chain_groups, var_mode=var_mode, ratio=ratio,
                             inv_ratio=DR.inv_of(ratio) if recip else 0.0, count=count)
    _rows_equal(DIAG, st.names, st.numels, d["by_tensor"], want)
    assert sum(r["n_eval"] for r in d["by_tensor"]) == d["n_eval"] == st.n1
    assert max(r["rhat_max"] for r in d["by_tensor"]) == d["rhat_max"]
    worst = next(r for r in d["by_tensor"] if r["rhat_max"] == d["rhat_max"])
    assert worst["argmax"] == d["argmax"] and worst["name"] == d["argmax_param"]
    # ESS: pooled, and chain k alone
    v, nsamp = S._ess
    assert nsamp >= 4
    ek = dict(chain_groups=st.chain_groups, samples=nsamp, batches=nsamp // 2)
    s_, b_ = v["sM2"].cpu().numpy(), v["bM2"].cpu().numpy()
    e = S.ess(by_tensor=True)
    assert {k: x for k, x in e.items() if k != "by_tensor"} == S.ess()
    _rows_equal(ESS, st.names, st.numels, e["by_tensor"],
                R.ess_layers_ref(s_, b_, segs, chains=3, **ek))
    per = S.ess(by_chain=True, by_tensor=True)
    assert len(per) == 3
    for k, r in enumerate(per):
        o = st.stride * k
        _rows_equal(ESS, st.names, st.numels, r["by_tensor"],
                    R.ess_layers_ref(s_[o:], b_[o:], segs, chains=1, **ek))
        assert min(t["ess_min"] for t in r["by_tensor"] if t["n_eval"]) == r["ess_min"]


def test_per_chain_sweep_returns_one_table_per_chain(loader):  # noqa: F811
    from bayesdll_amd import stacked
    torch.manual_seed(32)
    S = stacked.StackedCSGHMC(Net().cuda(), 3, _args(), init="reinit", seed=6, graph=False,
                              ess_batch=2, per_chain={"lr": [2e-2, 5e-2, 8e-2]})
    S.train_one_epoch(loader, 0)
    with pytest.raises(ValueError, match="by_chain"):
        S.ess(by_tensor=True)
    with pytest.raises(ValueError, match="per_chain"):
        S.diagnostics(by_tensor=True)
    st = S.state
    v, nsamp = S._ess
    segs = list(zip(st.offsets, st.numels))
    per = S.ess(by_chain=True, by_tensor=True)
    assert len(per) == 3 and all(len(r["by_tensor"]) == len(st.names) for r in per)
    for k, r in enumerate(per):
        o = st.stride * k
        want = R.ess_layers_ref(v["sM2"].cpu().numpy()[o:], v["bM2"].cpu().numpy()[o:], segs,
                                chains=1, chain_groups=st.chain_groups, samples=nsamp,
                                batches=nsamp // 2)
        _rows_equal(ESS, st.names, st.numels, r["by_tensor"], want)


def test_cli_by_tensor(tmp_path):
    from bayesdll_amd.run import main
    hp = ("prior_sig=1.0,Ninflate=1.0,nd=0.01,burnin=0,momentum_decay=0.18,thin=1,"
          "bias=informative,nst=2")
    hist = main(["--method", "csghmc", "--dataset", "mnist", "--backbone", "mlp_mnist",
                 "--epochs", "2", "--num_cycles", "2", "--batch_size", "32", "--lr", "1e-2",
                 "--train_size", "512", "--test_size", "64", "--stacked_chains", "3", "--rhat",
                 "--ess", "2", "--by_tensor", "3", "--hparams", hp, "--log_dir", str(tmp_path)])
    rec = hist[-1]
    rh, es = rec["rhat"]["by_tensor"], rec["ess"]["by_tensor"]
    assert len(rh) == len(es) >= 4 and [r["name"] for r in rh] == [r["name"] for r in es]
    assert sum(r["n_eval"] for r in rh) == rec["rhat"]["n_eval"]
    assert max(r["rhat_max"] for r in rh) == rec["rhat"]["rhat_max"]
    assert min(r["ess_min"] for r in es if r["n_eval"]) == rec["ess"]["ess_min"]
    text = next(tmp_path.rglob("logs.txt")).read_text().splitlines()
    last = [ln for ln in text if "(Epoch 1) " in ln]
    rl = [ln for ln in last if "R-hat over 3 chains, tensor " in ln]
    el = [ln for ln in last if "ESS over 3 chains, tensor " in ln]
    assert len(rl) == len(el) == 3
    worst = max(rh, key=lambda r: r["rhat_max"])
    assert f"tensor {worst['name']} ({worst['numel']} elements): max = " in rl[0] and "> 1.01" in rl[0]
    low = min((r for r in es if r["n_eval"]), key=lambda r: r["ess_min"])
    assert f"tensor {low['name']} ({low['numel']} elements): min = " in el[0] and "< 100" in el[0]
    # the summary lines are still there, one each, before the tensor lines
    assert sum("R-hat over 3 chains, component" in ln for ln in last) == 1
    assert sum("ESS over 3 chains, component" in ln for ln in last) == 1
