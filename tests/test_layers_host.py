"""The per-tensor R-hat / ESS tables (include/bdl_layers.h) without a GPU: the
header's functions, the C struct layouts against the ctypes mirrors, the
exports, every validation path of both entry points and the workspace
function (fake pointers: each call returns before any HIP call), the
traversal's restatement showing that the GPU tests' tables reach the segment
kinds they claim, the reference's row kinds on the GPU tests' inputs, the
samplers' by_tensor keyword on a fake kernels layer, and the command line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import chain_diag_ref as DR
import layers_ref as R
from test_chain_diag_host import Net, _args, host_only  # noqa: F401  (host_only: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

SEG_FIELDS = ["offset", "numel"]
DIAG_FIELDS = ["mom1", "mom2", "segments", "table", "workspace", "n", "chain_groups", "nsegments",
               "chains", "var_mode", "grid_blocks", "ratio", "inv_ratio", "var_floor", "c1",
               "thresholds", "pad0"]
ESS_FIELDS = ["sM2", "bM2", "segments", "table", "workspace", "n", "chain_groups", "samples",
              "batches", "nsegments", "chains", "grid_blocks", "thresholds"]
STRUCTS = (("bdl_layer_segment", SEG_FIELDS), ("bdl_diag_layers_args", DIAG_FIELDS),
           ("bdl_ess_layers_args", ESS_FIELDS))
FUNCS = ["bdl_chain_diag_layers", "bdl_chain_ess_layers", "bdl_layers_workspace_bytes"]
GRIDS = (2, R.DEFAULT_GRID)


# ------------------------------------------------------- 1. header, ctypes, exports
def test_header_declares_exactly_the_three_functions_and_no_abi_version():
    src = open(os.path.join(INCLUDE, "bdl_layers.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(re.findall(r"\b(bdl_\w+)\s*\(", code)) == FUNCS
    assert "BDL_ABI_VERSION" not in code
    for inc in ("bdl_sgmcmc.h", "bdl_diag.h", "bdl_ess.h"):
        assert f'#include "{inc}"' in code
    # the contract is stated where the caller reads it
    for word in ("chain-local", "extreme 0 and arg -1", "same device code", "No atomics",
                 "caller guarantees"):
        assert word in " ".join(src.split()), word


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    lines = []
    for st, fields in STRUCTS:
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    lines.append('printf("limits %d %d\\n", BDL_LAYERS_MAX_SEGMENTS, BDL_LAYERS_MAX_GRID);')
    lines.append('printf("rows %zu %zu\\n", sizeof(bdl_diag_summary), sizeof(bdl_ess_summary));')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_layers.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    out = subprocess.check_output([str(exe)]).decode().strip().splitlines()
    lay = {k: v for k, v in (ln.split(" ", 1) for ln in out)}
    for cls, (name, fields) in zip((L.LayerSegment, L.DiagLayersArgs, L.EssLayersArgs), STRUCTS):
        assert int(lay[name]) == C.sizeof(cls), name
        assert [f for f, _ in cls._fields_] == fields
        for f in fields:
            assert getattr(cls, f).offset == int(lay[f"{name}.{f}"]), (name, f)
    assert lay["limits"] == f"{L.LAYERS_MAX_SEGMENTS} {L.LAYERS_MAX_GRID}" == "65536 1024"
    assert lay["rows"] == f"{C.sizeof(L.DiagSummary)} {C.sizeof(L.EssSummary)}"
    # the structured host array kernels.chain_*_layers returns has the struct's layout
    assert np.dtype(L.DiagSummary).itemsize == C.sizeof(L.DiagSummary)
    assert np.dtype(L.EssSummary).fields["n_below"][0].shape == (3,)


def test_library_exports_the_tables_next_to_the_pinned_abi():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert sorted(L.LAYERS_EXPORTS) == FUNCS
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS, L.CHAIN_STEP_EXPORTS,
                  L.STATS_EXPORTS, L.ESS_EXPORTS, L.LOWP_EXPORTS):
        assert not set(L.LAYERS_EXPORTS) & set(other)
    for name in L.LAYERS_EXPORTS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    row = C.sizeof(L.DiagSummary)
    wb = h.bdl_layers_workspace_bytes
    assert wb(1, 1) == row and wb(296, 512) == 296 * 512 * row
    assert wb(11, 0) == wb(11, L.LAYERS_MAX_GRID) == 11 * 1024 * row
    assert wb(65536, 1024) == 65536 * 1024 * row            # no 32-bit overflow
    for bad in ((0, 1), (-1, 1), (65537, 1), (1, -1), (1, 1025)):
        assert wb(*bad) == 0, bad


# --------------------------------------------------------------- 2. validation
NULL, ALIGN, ARG = -1, -2, -3
ROW = 72


def _good(kind):
    """Three segments (48 B of rows, a 216-B table), vectors of 4 chains x 12
    elements with n = 10 (184 B), an explicit grid of 2 (a 432-B workspace)."""
    from bayesdll_amd import _lib as L
    a = L.DiagLayersArgs() if kind == "diag" else L.EssLayersArgs()
    v0, v1 = ("mom1", "mom2") if kind == "diag" else ("sM2", "bM2")
    setattr(a, v0, 0x10000)
    setattr(a, v1, 0x20000)
    a.segments, a.table, a.workspace = 0x30000, 0x40000, 0x100000
    a.n, a.chain_groups, a.chains, a.nsegments, a.grid_blocks = 10, 3, 4, 3, 2
    if kind == "diag":
        a.var_mode, a.ratio, a.var_floor, a.c1 = 2, 5.0, 1e-12, 5 / 6
    else:
        a.samples, a.batches = 12, 4
    return a


@pytest.mark.parametrize("kind", ["diag", "ess"])
def test_entry_points_validate_before_touching_the_device(kind):
    """Every refusal of the header's list, with its status and a message.  No
    call here passes validation, so none reaches a HIP call."""
    from bayesdll_amd import _lib as L
    h = L.lib()
    fn = getattr(h, f"bdl_chain_{kind}_layers")
    v0, v1 = ("mom1", "mom2") if kind == "diag" else ("sM2", "bM2")

    def refused(status, word, **fields):
        a = _good(kind)
        for k, v in fields.items():
            setattr(a, k, v)
        assert fn(a, None) == status, fields
        msg = h.bdl_last_error()
        assert msg.startswith(f"bdl_chain_{kind}_layers:".encode()) and word in msg, (fields, msg)

    assert fn(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in (v0, v1):
        refused(NULL, f"{v0} and {v1}".encode(), **{f: None})
        refused(ALIGN, b"vector not 16-B aligned", **{f: 0x70008})
    refused(NULL, b"segments", segments=None)
    refused(NULL, b"table", table=None)
    refused(NULL, b"workspace", workspace=None)
    refused(ALIGN, b"workspace not 16-B aligned", workspace=0x100008)
    refused(ALIGN, b"segments not 8-B aligned", segments=0x30004)
    refused(ALIGN, b"table not 8-B aligned", table=0x40004)
    refused(ARG, b"chains", chains=0)
    refused(ARG, b"chains", chains=-2)
    refused(ARG, b"n must be", n=0)
    refused(ARG, b"chain slot", n=13)                          # 4 * chain_groups = 12
    refused(ARG, b"chain slot", chain_groups=0)
    refused(ARG, b"overflows", chain_groups=1 << 60, chains=2)
    refused(ARG, b"nsegments", nsegments=0)
    refused(ARG, b"nsegments", nsegments=65537)
    refused(ARG, b"grid_blocks", grid_blocks=-1)
    refused(ARG, b"grid_blocks", grid_blocks=1025)
    if kind == "diag":
        refused(ARG, b"chains must be >= 2", chains=1)
        refused(ARG, b"var_mode", var_mode=3)
        refused(ARG, b"var_mode", var_mode=-1)
        refused(ARG, b"var_floor", var_floor=-1.0)
        refused(ARG, b"var_floor", var_floor=float("nan"))
    else:
        refused(ARG, b"chains", chains=65536)
        refused(ARG, b"samples must be >= 2 (got 1)", samples=1, batches=1)
        refused(ARG, b"batches must be >= 2 (got 1)", batches=1)
        refused(ARG, b"batches exceeds samples", batches=13)
        refused(ARG, b"below 2^24", samples=1 << 24)
    # the table (216 B) and the workspace (432 B at grid 2; 3 * 1024 * 72 at grid 0) against
    # the inputs (184 B), the segment table (48 B) and each other
    refused(ARG, b"table overlaps", table=0x10000 + 176)
    refused(ARG, b"table overlaps", table=0x20000 - 208)
    refused(ARG, b"table overlaps", table=0x30000 + 40)
    refused(ARG, b"workspace overlaps an input", workspace=0x10000 + 16)
    refused(ARG, b"workspace overlaps an input", workspace=0x20000 - 416)
    refused(ARG, b"workspace overlaps an input", workspace=0x30000 + 32)
    refused(ARG, b"workspace overlaps the table", workspace=0x40000 + 208)
    refused(ARG, b"workspace overlaps the table", table=0x900000,
            workspace=0x900000 - 3 * 1024 * ROW + 16, grid_blocks=0)


def test_both_entry_points_refuse_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        for kind in ("diag", "ess"):
            assert getattr(h, f"bdl_chain_{kind}_layers")(_good(kind), None) == ARG
            assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_chain_diag_layers(None, None) == NULL


def test_kernels_layer_checks_its_arguments_before_any_launch(monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    v = torch.zeros(24)
    seg = torch.tensor([[0, 10]], dtype=torch.int64)
    kw = dict(chains=2, chain_groups=3, n=10)
    dk = dict(kw, var_mode=2, ratio=5.0, count=6)
    ek = dict(kw, samples=12, batches=4)
    with pytest.raises(ValueError, match="second moment is required"):
        K.chain_diag_layers(v, None, seg, **dk)
    with pytest.raises(ValueError, match="at least 2 samples"):
        K.chain_diag_layers(v, v, seg, **dict(dk, count=1))
    with pytest.raises(ValueError, match="at least 2 chains"):
        K.chain_diag_layers(v, v, seg, **dict(dk, chains=1))
    with pytest.raises(ValueError, match="three thresholds"):
        K.chain_diag_layers(v, v, seg, thresholds=(1, 2), **dk)
    with pytest.raises(ValueError, match="2 closed batches"):
        K.chain_ess_layers(v, v, seg, **dict(ek, batches=1))
    with pytest.raises(ValueError, match="three finite"):
        K.chain_ess_layers(v, v, seg, thresholds=(1, 2), **ek)
    with pytest.raises(ValueError, match="4 \\* chain_groups"):
        K.chain_ess_layers(v, v, seg, **dict(ek, n=13))
    for call, k2 in ((K.chain_diag_layers, dk), (K.chain_ess_layers, ek)):
        for bad in (seg.to(torch.int32), seg.view(-1), torch.zeros(1, 3, dtype=torch.int64),
                    seg.numpy()):
            with pytest.raises(ValueError, match=r"int64 \[nsegments, 2\]"):
                call(v, v, bad, **k2)
        with pytest.raises(ValueError, match="grid_blocks"):
            call(v, v, seg, grid_blocks=1025, **k2)


# ------------------------------------------------------ 3. what the tables reach
def _kinds(tab, grid):
    c = R.classify(tab.segments, tab.n, grid)
    return c, {nm: [c[w, i] for w in range(grid)] for i, nm in enumerate(tab.names)}


@pytest.mark.parametrize("grid", GRIDS + (208, 608))
def test_table_l_reaches_every_segment_kind(grid):
    tab = R.table_l()
    assert tab.n == 7245 <= 20000 and tab.n % 4 == 1 and tab.slot == 7248
    c, by = _kinds(tab, grid)
    for i, (o, m) in enumerate(tab.segments):           # every element exactly once
        parts = [c[w, i] for w in range(grid)]
        assert sum(p["head"] + p["body"] + p["tail"] for p in parts) == m
        assert sum(p["head"] > 0 or p["tail"] > 0 for p in parts) <= 1
        assert any(p["part"] for p in parts)

    def total(nm):
        return tuple(sum(p[f] for p in by[nm]) for f in ("head", "body", "tail"))

    # all head: one element, and three elements starting at an offset = 1 mod 4
    assert tab.span("one") == (5, 1) and total("one") == (1, 0, 0)
    assert tab.span("three")[0] % 4 == 1 and total("three") == (3, 0, 0)
    assert total("two") == (2, 0, 1) and total("pre") == (0, 4, 1)
    assert total("hbt") == (1, 996, 3)                   # head, body and tail
    o, m = tab.span("aligned")
    assert o % 4 == 0 and (o + m) % 4 == 0 and total("aligned") == (0, 1024, 0)
    # the largest tensor: at least 2 * 256 * 4 * unroll elements
    assert max(tab.numels) == tab.span("big")[1] >= 2 * R.K_BLOCK * 4 * R.UNROLL
    o, m = tab.span("last")
    assert o + m == tab.n and tab.n % 4 != 0 and total("last")[2] == 1
    # a workgroup that takes no part (every small segment leaves one), at every grid
    assert any(not p["part"] for p in by["one"]) and any(not p["part"] for p in by["hbt"])
    # the head / tail owner rotates with the segment index
    owners = {i: next(w for w in range(grid) if c[w, i]["head"] or c[w, i]["tail"])
              for i, nm in enumerate(tab.names) if total(nm)[0] or total(nm)[2]}
    assert all(w == i % grid for i, w in owners.items()) and len(set(owners.values())) > 1
    if grid == 2:
        # both workgroups make two trips through `big`, the second one partial
        assert [p["iters"] for p in by["big"]] == [2, 2]
        assert sorted(p["body"] for p in by["big"]) == [4 * (256 + 57), 4 * 512]
    else:
        assert sorted(p["iters"] for p in by["big"])[-4:] == [0, 1, 1, 1, 1][-4:]
        assert sum(p["part"] for p in by["big"]) == 4    # 825 groups: four block iterations


@pytest.mark.parametrize("grid", GRIDS)
def test_table_a_is_covered_once_and_has_idle_workgroups(grid):
    tab = R.table_a()
    assert (tab.n, tab.slot) == (39426, 39428)
    c, by = _kinds(tab, grid)
    for i, (o, m) in enumerate(tab.segments):
        assert sum(p["head"] + p["body"] + p["tail"] for p in by[tab.names[i]]) == m
    assert any(o % 4 for o, _ in tab.segments)                         # the odd boundary
    assert max(p["iters"] for p in by["l0.weight"]) == (7 if grid == 2 else 1)
    assert any(not p["part"] for p in by["l5.weight"])


# ----------------------------------------------------------- 4. the row kinds
MODES = [("welford_recip", DR.VAR_WELFORD, 6.0, True), ("welford", DR.VAR_WELFORD, 6.0, False),
         ("raw", DR.VAR_RAW_MOMENTS, 7 / 6, False)]


def _constructed(tab, rows):
    by = dict(zip(tab.names, rows))
    fz = by[tab.frozen]
    assert (fz["n_eval"], fz["n_degenerate"], fz["n_nonfinite"]) == (0, tab.span(tab.frozen)[1], 0)
    assert fz["ext"] == 0.0 and fz["sum"] == 0.0 and min(fz[k] for k in ("argmax", "argmin")
                                                         if k in fz) == -1
    if tab.flat:
        fl = by[tab.flat]
        assert (fl["n_eval"], fl["n_degenerate"], fl["n_nonfinite"]) == (0, 0, tab.span(tab.flat)[1])
        hb = by["hbt"]
        assert (hb["n_eval"], hb["n_degenerate"], hb["n_nonfinite"]) == (997, 0, 3)
    ordinary = [nm for nm in tab.names if nm not in (tab.frozen, tab.flat)]
    for nm in ordinary:
        r, m = by[nm], tab.span(nm)[1]
        assert r["n_eval"] >= 0.9 * m and r["n_degenerate"] == 0, nm
        assert r["n_nonfinite"] == (3 if nm == "hbt" else 0), nm
        o = tab.span(nm)[0]
        arg = r["argmax"] if "argmax" in r else r["argmin"]
        assert o <= arg < o + m, nm                       # chain-local, inside its own tensor
    return ordinary


@pytest.mark.parametrize("table", ["l", "a"])
@pytest.mark.parametrize("mode", MODES, ids=lambda m: m[0])
def test_reference_rows_of_the_diag_inputs(table, mode):
    _, var_mode, ratio, recip = mode
    tab = R.table_l() if table == "l" else R.table_a()
    for K_ in ((2, 5) if table == "l" else (3,)):
        m1, m2 = R.diag_inputs(tab, K_, var_mode, ratio)
        rows = R.diag_layers_ref(m1, m2, tab.segments, chains=K_, chain_groups=tab.chain_groups,
                                 var_mode=var_mode, ratio=ratio, var_floor=0.0, count=R.COUNT,
                                 inv_ratio=DR.inv_of(ratio) if recip else 0.0)
        ordinary = _constructed(tab, rows)
        if table == "l":
            assert tuple(ordinary) == R.ORDINARY_L
        # the thresholds split the values: neither no hit nor all hits in the large rows
        big = rows[tab.names.index("big" if table == "l" else "l0.weight")]
        assert 0 < big["n_above"][2] < big["n_above"][0] < big["n_eval"]


@pytest.mark.parametrize("table", ["l", "a"])
def test_reference_rows_of_the_ess_inputs(table):
    tab = R.table_l() if table == "l" else R.table_a()
    for K_ in ((1, 2, 5) if table == "l" else (3,)):
        sM2, bM2 = R.ess_inputs(tab, K_)
        kw = dict(chain_groups=tab.chain_groups, samples=R.SAMPLES, batches=R.BATCHES)
        rows = R.ess_layers_ref(sM2, bM2, tab.segments, chains=K_, **kw)
        _constructed(tab, rows)
        big = rows[tab.names.index("big" if table == "l" else "l0.weight")]
        thr = big["n_below"]
        assert 0 <= thr[0] <= thr[1] <= thr[2] and thr[2] > 0
    # the rows add up to the whole-vector reference (what the GPU test asks of the device)
    import chain_ess_ref as ER
    whole = ER.chain_ess_f32(sM2, bM2, chains=K_, n=tab.n, **kw)[2]
    for f in ("n_eval", "n_degenerate", "n_nonfinite"):
        assert sum(r[f] for r in rows) == whole[f]
    assert [sum(r["n_below"][j] for r in rows) for j in range(3)] == whole["n_below"]
    evald = [r for r in rows if r["n_eval"]]
    assert min(r["ess_min"] for r in evald) == whole["ess_min"]
    assert next(r for r in evald if r["ess_min"] == whole["ess_min"])["argmin"] == whole["argmin"]


# -------------------------------------------------- 5. the samplers' keyword
def _fake_table(struct, n, ext, arg, hits, total):
    t = np.zeros(n, dtype=np.dtype(struct))
    t["n_eval"] = np.arange(n) * 10                    # row 0: nothing evaluated
    t[ext] = 1.0 + np.arange(n)
    t[arg] = np.arange(n) - 1
    t[total] = 3.0 * np.arange(n) * 10
    t[hits] = np.arange(n)[:, None] * np.array([3, 2, 1])
    return t


@pytest.fixture
def fake_layers(host_only, monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    calls = host_only

    def diag_layers(m1, m2, seg, **kw):
        calls.append(("diag_layers", m1, m2, seg, kw))
        return _fake_table(L.DiagSummary, seg.shape[0], "rhat_max", "argmax", "n_above", "rhat_sum")

    def ess_layers(s, b, seg, **kw):
        calls.append(("ess_layers", s, b, seg, kw))
        return _fake_table(L.EssSummary, seg.shape[0], "ess_min", "argmin", "n_below", "ess_sum")

    class FakeEss(dict):
        summary = {"n_eval": 138, "n_degenerate": 0, "n_nonfinite": 0, "argmin": 100,
                   "n_below": [3, 2, 1], "ess_sum": 1380.0, "ess_min": 7.0}

    def chain_ess(s, b, **kw):
        calls.append(("ess", s, b, kw))
        return FakeEss()

    monkeypatch.setattr(K, "chain_diag_layers", diag_layers)
    monkeypatch.setattr(K, "chain_ess_layers", ess_layers)
    monkeypatch.setattr(K, "chain_ess", chain_ess)
    return calls


def test_layer_segments_is_built_once_over_all_names(host_only):
    from bayesdll_amd import stacked
    net = Net()
    net.body.bias.requires_grad_(False)                  # a frozen tensor gets its row too
    st = stacked.StackedCSGHMC(net, 3, _args()).state
    seg = st.layer_segments()
    assert seg.dtype == torch.int64 and seg.shape == (4, 2) and seg.is_contiguous()
    assert seg.tolist() == [[0, 91], [91, 7], [98, 35], [133, 5]]
    assert seg.tolist() == [list(r) for r in zip(st.offsets, st.numels)]
    assert st.layer_segments() is seg
    assert int(seg[-1].sum()) == st.n1 == 138 < st.stride == 140   # the padding lies in no row


def test_diagnostics_by_tensor_on_a_fake_kernels_layer(fake_layers):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import stacked
    S = stacked.StackedCSGHMC(Net(), 3, _args())
    with pytest.raises(ValueError, match="nothing is collected"):
        S.diagnostics(by_tensor=True)
    S._collect_spec(1)
    S.samples_per_cycle[1] = 2
    with pytest.raises(ValueError, match="at least 2"):
        S.diagnostics(by_tensor=True)
    S.samples_per_cycle[1] = 6
    plain = S.diagnostics()
    assert not any(c[0] == "diag_layers" for c in fake_layers) and S.state._layer_table is None
    assert set(plain) == {"n_eval", "n_degenerate", "n_nonfinite", "argmax", "n_above", "rhat_sum",
                          "rhat_max", "rhat_mean", "share_above", "thresholds", "component",
                          "count", "argmax_param"}
    d = S.diagnostics(by_tensor=True)
    assert {k: v for k, v in d.items() if k != "by_tensor"} == plain
    kind, m1, m2, seg, kw = fake_layers[-1]
    assert kind == "diag_layers" and m1 is S.mom1[1] and m2 is S.mom2[1]
    assert seg is S.state.layer_segments()
    assert kw == dict(chains=3, chain_groups=35, n=138, var_mode=L.VAR_WELFORD, ratio=5.0, count=3)
    rows = d["by_tensor"]
    assert [r["name"] for r in rows] == S.state.names == ["body.weight", "body.bias",
                                                          "head.weight", "head.bias"]
    assert [r["numel"] for r in rows] == S.state.numels
    assert all(list(r) == ["name", "numel", "n_eval", "n_degenerate", "n_nonfinite", "rhat_max",
                           "argmax", "rhat_mean", "n_above", "share_above"] for r in rows)
    assert rows[0]["n_eval"] == 0 and np.isnan(rows[0]["rhat_mean"]) and rows[0]["argmax"] == -1
    assert np.isnan(rows[0]["share_above"]).all()
    assert rows[2] == {"name": "head.weight", "numel": 35, "n_eval": 20, "n_degenerate": 0,
                       "n_nonfinite": 0, "rhat_max": 3.0, "argmax": 1, "rhat_mean": 3.0,
                       "n_above": [6, 4, 2], "share_above": [0.3, 0.2, 0.1]}
    assert all(type(v) in (str, int, float, list) for r in rows for v in r.values())
    # the refusals stay as they are
    for bad, match in ((stacked.StackedSGLD(Net(), 1, _args()), "K = 1"),
                       (stacked.StackedCSGHMC(Net(), 3, _args(),
                                              per_chain={"lr": [1e-2, 2e-2, 3e-2]}), "per_chain")):
        with pytest.raises(ValueError, match=match):
            bad.diagnostics(by_tensor=True)
    S0 = stacked.StackedSGLD(Net(), 2, _args(nst=0))
    S0.seed_moments()
    S0.cnt = 4
    with pytest.raises(ValueError, match="second moment is not kept"):
        S0.diagnostics(by_tensor=True)


def test_ess_by_tensor_on_a_fake_kernels_layer(fake_layers):
    from bayesdll_amd import stacked
    S0 = stacked.StackedSGLD(Net(), 2, _args())
    with pytest.raises(ValueError, match="built with ess_batch=0"):
        S0.ess(by_tensor=True)
    S = stacked.StackedCSGHMC(Net(), 3, _args(), ess_batch=4)
    with pytest.raises(ValueError, match="nothing is folded yet"):
        S.ess(by_tensor=True)
    vec = {nm: torch.zeros(S.state.n) for nm in ("bsum", "smean", "sM2", "bM2")}
    S._ess = [vec, 7]
    with pytest.raises(ValueError, match="close 1 batch of 4"):
        S.ess(by_tensor=True)
    S._ess = [vec, 13]
    plain = S.ess()
    assert not any(c[0] == "ess_layers" for c in fake_layers) and S.state._layer_table is None
    assert set(plain) == {"n_eval", "n_degenerate", "n_nonfinite", "argmin", "ess_min", "ess_sum",
                          "ess_mean", "n_below", "share_below", "thresholds", "samples", "batches",
                          "batch", "chains", "component", "argmin_param"}
    d = S.ess(by_tensor=True)
    assert {k: v for k, v in d.items() if k != "by_tensor"} == plain
    kind, s, b, seg, kw = fake_layers[-1]
    assert kind == "ess_layers" and seg is S.state.layer_segments()
    assert s.data_ptr() == vec["sM2"].data_ptr() and b.data_ptr() == vec["bM2"].data_ptr()
    assert kw == dict(chains=3, chain_groups=35, n=138, samples=13, batches=3,
                      thresholds=(100.0, 400.0, 1000.0))
    rows = d["by_tensor"]
    assert [r["name"] for r in rows] == S.state.names
    assert all(list(r) == ["name", "numel", "n_eval", "n_degenerate", "n_nonfinite", "ess_min",
                           "argmin", "ess_mean", "n_below", "share_below"] for r in rows)
    assert rows[3]["ess_min"] == 4.0 and rows[3]["argmin"] == 2 and rows[3]["ess_mean"] == 3.0
    # by chain: K tables, chain k's from its own slice with chains = 1
    n0 = len(fake_layers)
    per = S.ess(by_chain=True, by_tensor=True)
    assert len(per) == 3 and all(len(r["by_tensor"]) == 4 and r["chains"] == 1 for r in per)
    lay = [c for c in fake_layers[n0:] if c[0] == "ess_layers"]
    assert len(lay) == 3 and all(c[4]["chains"] == 1 for c in lay)
    assert [c[1].data_ptr() - vec["sM2"].data_ptr() for c in lay] == [0, 4 * 140, 8 * 140]
    assert "by_tensor" not in S.ess(by_chain=True)[0]
    SP = stacked.StackedCSGHMC(Net(), 3, _args(), ess_batch=4,
                               per_chain={"lr": [1e-2, 2e-2, 3e-2]})
    SP._ess = [vec, 13]
    with pytest.raises(ValueError, match="per_chain hyperparameters.*by_chain"):
        SP.ess(by_tensor=True)
    assert len(SP.ess(by_chain=True, by_tensor=True)) == 3


def test_reports_log_the_worst_tensors_after_the_unchanged_line(fake_layers):
    from bayesdll_amd import stacked
    lines = []
    a = _args()
    a.by_tensor = 2
    S = stacked.StackedCSGHMC(Net(), 3, a, ess_batch=4)
    S._collect_spec(1)
    S.samples_per_cycle[1] = 6
    S._ess = [{nm: torch.zeros(S.state.n) for nm in ("bsum", "smean", "sM2", "bM2")}, 13]
    rec = {}
    S._report_rhat(5, rec, lines.append)
    S._report_ess(5, rec, lines.append)
    assert len(rec["rhat"]["by_tensor"]) == len(rec["ess"]["by_tensor"]) == 4
    rh = [ln for ln in lines if "R-hat" in ln]
    es = [ln for ln in lines if "ESS" in ln]
    assert len(rh) == len(es) == 3
    # largest rhat_max first; the row with nothing evaluated is never listed
    assert "tensor head.bias (5 elements): max = 4.0000, mean = 3.0000, > 1.01: 30.0 %" in rh[1]
    assert "tensor head.weight (35 elements)" in rh[2]
    # smallest ess_min first
    assert "tensor body.bias (7 elements): min = 2.0, mean = 3.0, < 100: 30.0 %" in es[1]
    assert "tensor head.weight" in es[2]
    # without the flag: the same first lines, nothing after them, no table
    a.by_tensor = 0
    lines2, rec2 = [], {}
    S._report_rhat(5, rec2, lines2.append)
    S._report_ess(5, rec2, lines2.append)
    assert lines2 == [rh[0], es[0]]
    assert "by_tensor" not in rec2["rhat"] and "by_tensor" not in rec2["ess"]


# ----------------------------------------------------------------- 6. the CLI
def test_run_cli_by_tensor_needs_rhat_or_ess(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    assert ap.parse_args([]).by_tensor == 0
    a = ap.parse_args(["--stacked_chains", "4", "--rhat", "--ess", "8", "--by_tensor", "5"])
    assert (a.by_tensor, a.rhat, a.ess) == (5, True, 8) and run.check_by_tensor(ap, a) == 5
    assert run.check_by_tensor(ap, ap.parse_args(["--stacked_chains", "2", "--ess", "2",
                                                  "--by_tensor", "1"])) == 1
    with pytest.raises(SystemExit) as e:
        run.main(["--stacked_chains", "2", "--by_tensor", "3"])
    assert e.value.code == 2 and "it needs --rhat or --ess" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run.main(["--stacked_chains", "2", "--rhat", "--by_tensor", "-1"])
    assert e.value.code == 2 and "N must be >= 0" in capsys.readouterr().err
