"""bdl_diversity on the host: the loop reference against its vectorised second
form, the emulated arithmetic contract within the derived bound, the derived
quantities of kernels.diversity_summary / diversity_pairs on hand-made tables,
the header's constants and layout against the Python binding, and the proof
that table D reaches every launch path and every constructed example."""
import os
import re

import numpy as np
import pytest

import diversity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "bdl_diversity.h")).read()


def _define(name):
    m = re.search(r"#define\s+" + name + r"\s+\(?([^/\n]*?)\)?\s*(/\*|\n)", HDR)
    return eval(m.group(1))  # noqa: S307 — integer expressions of the header


def test_header_constants_match_the_reference_and_the_binding():
    from bayesdll_amd import _lib as L
    want = {"MAX_VOTERS": R.MAX_VOTERS, "MAX_CLASSES": R.MAX_CLASSES,
            "WAVE_VOTERS": R.WAVE_VOTERS, "TILE": R.TILE, "LDS_STRIDE": R.LDS_STRIDE,
            "MAX_GRID": R.MAX_GRID, "DEFAULT_WORKSPACE": R.DEFAULT_WORKSPACE}
    for k, v in want.items():
        assert _define("BDL_DIVERSITY_" + k) == v == getattr(L, "DIVERSITY_" + k), k
    assert R.LDS_STRIDE % 64 == 4 and R.TILE % 4 == 0      # 16 rows x 16 B: 64 banks
    assert re.search(r"BDL_DIVERSITY_RESET\s*=\s*0x1", HDR) and L.DIVERSITY_RESET == 1
    assert sorted(L.DIVERSITY_EXPORTS) == ["bdl_diversity", "bdl_diversity_totals_bytes",
                                           "bdl_diversity_workspace_bytes"]
    for P in (2, 3, 64):
        dt = L.diversity_totals_dtype(P)
        assert dt.itemsize == 32 + 40 * P * P
        assert dt.names == R.HEADER + ("voters",) + R.INTS + R.SUMS
        assert dt.fields["disagree"][1] == 32 and dt.fields["kl_sum"][1] == 32 + 32 * P * P
    # the header's stated workspace figures
    assert R.partial_bytes(64) == 163872 and R.DEFAULT_WORKSPACE // R.partial_bytes(64) == 204
    assert R.DEFAULT_WORKSPACE // R.partial_bytes(28) >= 1024 > R.DEFAULT_WORKSPACE // \
        R.partial_bytes(29)
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_diversity" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "include/bdl_diversity.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    # the args struct as the binding lays it out: four pointers, int64, four int32
    assert [f[0] for f in L.DiversityArgs._fields_] == re.findall(
        r"^\s+(?:const )?\w+\*? (\w+);", HDR.split("typedef struct bdl_diversity_args {")[1]
        .split("}")[0], flags=re.M)


@pytest.mark.parametrize("case", R.D, ids=R.case_id)
def test_loop_reference_equals_the_vectorised_form(case):
    x, lab, r = R.built(case)
    P, B, C = x.shape
    sel = np.arange(B) if P <= 24 else np.array([0, 3, 5, 6, 7, 12])  # the loops are slow
    xs, ls = x[:, sel, :], (None if lab is None else lab[sel])
    a, v = R.reference_loop(xs, ls), (r if len(sel) == B else R.reference(xs, ls))
    for k in R.HEADER:
        assert a[k] == v[k], k
    for k in R.INTS:
        assert np.array_equal(a[k], v[k]), k
    for k in R.SUMS:
        assert np.allclose(a[k], v[k], rtol=1e-12, atol=1e-13), k
    # the structure the header promises
    assert np.array_equal(v["disagree"], v["disagree"].T) and not np.diag(v["disagree"]).any()
    assert np.array_equal(v["both_wrong"], v["both_wrong"].T)
    assert np.array_equal(v["tv_sum"], v["tv_sum"].T) and not np.diag(v["tv_sum"]).any()
    assert not np.diag(v["kl_sum"]).any() and not np.diag(v["kl_unbounded"]).any()
    assert v["n"] + v["n_nonfinite"] == len(sel)


@pytest.mark.parametrize("case", R.D, ids=R.case_id)
def test_emulated_contract_is_within_the_derived_bound(case):
    x, lab, r = R.built(case)
    e = R.reference(x, lab, emulate=True)
    for k in R.HEADER:
        assert e[k] == r[k], k
    for k in R.INTS:
        assert np.array_equal(e[k], r[k]), k
    for k in R.SUMS:
        err = np.abs(e[k] - r[k])
        assert (err <= r["bound"][k]).all(), (k, float((err / np.maximum(r["bound"][k], 1e-300)).max()))
    if case[4] == "dyadic":
        assert np.array_equal(e["tv_sum"], r["tv_sum"])      # every term is exact
    if case[4] == "identical":
        assert not any(np.any(r[k]) for k in ("disagree", "kl_unbounded") + R.SUMS)
    # the bound is tight enough to mean something: far below the entries themselves
    big = r["tv_sum"] > 0.1
    assert (r["bound"]["tv_sum"][big] < 1e-3 * r["tv_sum"][big]).all()


def test_table_reaches_every_path_and_every_constructed_example():
    seen, plants, kinds = set(), set(), set()
    for c in R.D:
        P, B, C, _, kind = c
        for g in R.GRIDS:
            seen |= R.path_labels(P, B, C, g or R.default_grid(P, B, C))
        plants |= R.planted(P, B, C, kind)
        kinds.add(kind)
    want = {"wave", "workgroup", "np1", "np2", "np4", "np8", "vec", "scalar", "one-tile", "tiles",
            "tile-1", "tile", "tile+1", "tile-part", "one-class", "ragged-pairs",
            "several-pairs-per-thread", "edge-classes", "edge-voters", "idle-workgroups",
            "second-trip", "uneven-trips", "idle-waves", "idle-pass1-waves"}
    assert want <= seen, want - seen
    assert plants == set(R.PLANT) and kinds == {"random", "identical", "dyadic", "nolabels"}
    # both instances with one and with two pairs per lane / thread, P = 2, 3 and 64
    inst = {(R.wave_instance(c[0], c[2]), R.pairs_per_thread(c[0], c[2])) for c in R.D}
    assert inst == {(True, 1), (True, 2), (False, 1), (False, 2), (False, 4), (False, 8)}
    assert {2, 3, 64} <= {c[0] for c in R.D}
    assert {(16, 64), (17, 64), (16, 65)} <= {(c[0], c[2]) for c in R.D}   # the dispatch edges
    for c in ((16, 64), (17, 64), (16, 65)):
        assert R.wave_instance(*c) == (c == (16, 64))
    # the dispatch thresholds of the pairs per thread
    assert [R.pairs_per_thread(P, 100) for P in (23, 24, 32, 33, 45, 46, 64)] == \
        [1, 2, 2, 4, 4, 8, 8]
    assert [R.pairs_per_thread(P, 10) for P in (11, 12, 16)] == [1, 2, 2]
    # nothing is at workload size
    assert max(c[0] * c[1] * c[2] for c in R.D) <= 64 * 24 * 200


def test_planted_examples_do_what_they_are_there_for():
    x, lab, r = R.built((17, 13, 65, 11, "random"))
    P = x.shape[0]
    assert r["n_nonfinite"] == 3 and r["n"] == 10 and r["n_labelled"] == 8
    # the tie: voter 0 votes the lower of its two maxima, voter 1 the upper one
    assert x[0, 4, 0] == x[0, 4].max() == x[0, 4, -1] and x[1, 4].argmax() == 64
    one = R.reference(x[:, 4:5, :], lab[4:5])
    assert one["disagree"][0, 1] == 1 and one["both_wrong"][0, 0] == 1 \
        and one["both_wrong"][1, 1] == 0
    # a class masked for voter 0 only: KL(j || 0) is infinite, KL(0 || j) is not
    one = R.reference(x[:, 5:6, :], lab[5:6])
    assert (one["kl_unbounded"][1:, 0] == 1).all() and not one["kl_unbounded"][0].any()
    assert one["kl_unbounded"].sum() == P - 1 and (one["kl_sum"][1:, 0] == 0).all()
    # voters 0 and 1 masked at different classes: unbounded both ways
    one = R.reference(x[:, 6:7, :], lab[6:7])
    assert one["kl_unbounded"][0, 1] == 1 == one["kl_unbounded"][1, 0]
    assert np.isfinite(one["tv_sum"]).all() and np.isfinite(one["kl_sum"]).all()
    # identical rows: exact zeros
    one = R.reference(x[:, 3:4, :], lab[3:4], emulate=True)
    assert not one["tv_sum"].any() and not one["kl_sum"].any() and not one["disagree"].any()
    # every pair index maps to one ordered pair
    for Pn in (2, 3, 17, 64):
        got = [R.pair_of(q, Pn) for q in range(Pn * (Pn - 1) // 2)]
        assert got == [(i, j) for i in range(Pn) for j in range(i + 1, Pn)]


def _raw(n, nl, dis, bw, unb=None, tv=None, kl=None, nonf=0):
    P = len(bw)
    z = np.zeros((P, P))
    return {"n": n, "n_labelled": nl, "n_nonfinite": nonf, "disagree": np.array(dis),
            "both_wrong": np.array(bw), "kl_unbounded": np.array(unb if unb is not None else z,
                                                                 dtype=np.int64),
            "tv_sum": np.array(tv if tv is not None else z, dtype=np.float64),
            "kl_sum": np.array(kl if kl is not None else z, dtype=np.float64)}


def test_summary_on_hand_made_tables():
    from bayesdll_amd import kernels as K
    # 10 labelled examples of 12; voter 0 wrong on 4, voter 1 on 5, both on 2
    s = K.diversity_summary(_raw(12, 10, [[0, 6], [6, 0]], [[4, 2], [2, 5]],
                                 unb=[[0, 2], [12, 0]], tv=[[0, 3.0], [3.0, 0]],
                                 kl=[[0, 5.0], [7.0, 0]], nonf=1))
    assert (s["n"], s["n_labelled"], s["n_nonfinite"]) == (12, 10, 1)
    assert s["disagreement"][0, 1] == 0.5 and s["tv"][0, 1] == 0.25
    assert s["kl"][0, 1] == 0.5 and np.isnan(s["kl"][1, 0]) and s["kl"][0, 0] == 0
    assert np.isnan(s["sym_kl"][0, 1]) and s["kl_unbounded"][1, 0] == 12
    assert s["error"].tolist() == [0.4, 0.5] and s["double_fault"][0, 1] == 0.2
    # phi of the table [[2, 2], [3, 3]]: (10 * 2 - 4 * 5) / sqrt(4 * 6 * 5 * 5) = 0
    assert s["error_correlation"][0, 1] == 0 and s["error_correlation"][0, 0] == 1
    # perfectly correlated and perfectly anti-correlated errors
    s = K.diversity_summary(_raw(8, 8, [[0, 0], [0, 0]], [[3, 3], [3, 3]]))
    assert s["error_correlation"][0, 1] == 1
    s = K.diversity_summary(_raw(8, 8, [[0, 8], [8, 0]], [[4, 0], [0, 4]]))
    assert s["error_correlation"][0, 1] == -1
    # degenerate: a voter never wrong, a voter always wrong, nothing labelled
    s = K.diversity_summary(_raw(8, 8, [[0, 0], [0, 0]], [[0, 0], [0, 8]]))
    assert np.isnan(s["error_correlation"]).all() and s["error"].tolist() == [0, 1]
    s = K.diversity_summary(_raw(8, 0, [[0, 1], [1, 0]], [[0, 0], [0, 0]]))
    assert np.isnan(s["error"]).all() and np.isnan(s["double_fault"]).all()
    assert np.isnan(s["error_correlation"]).all() and s["disagreement"][0, 1] == 0.125


def test_pairs_summary_ties_and_nans():
    from bayesdll_amd import kernels as K
    nan = float("nan")
    tv = np.array([[0, .5, .2, .5], [.5, 0, .2, .1], [.2, .2, 0, .3], [.5, .1, .3, 0]])
    d = {"disagreement": tv, "tv": tv, "double_fault": np.zeros((4, 4)),
         "sym_kl": np.array([[0, nan, 1, nan], [nan, 0, nan, nan], [1, nan, 0, 3.0],
                             [nan, nan, 3.0, 0]])}
    s = K.diversity_pairs(d)
    assert s["tv"]["min"] == .1 and s["tv"]["min_pair"] == (1, 3)
    assert s["tv"]["max"] == .5 and s["tv"]["max_pair"] == (0, 1)      # the lowest of two
    assert abs(s["tv"]["mean"] - 1.8 / 6) < 1e-15
    assert s["double_fault"]["min_pair"] == (0, 1) == s["double_fault"]["max_pair"]
    assert s["sym_kl"]["mean"] == 2 and s["sym_kl"]["min_pair"] == (0, 2)
    assert s["nearest"] == [2, 3, 0, 1]
    z = {k: np.zeros((3, 3)) for k in K.DIVERSITY_PAIR_KEYS}
    assert K.diversity_pairs(z)["nearest"] == [1, 0, 0]               # well defined on ties
    z["sym_kl"] = np.full((3, 3), nan)
    s = K.diversity_pairs(z)
    assert np.isnan(s["sym_kl"]["mean"]) and s["sym_kl"]["min_pair"] is None


def test_cli_refuses_diversity_without_stacked_chains(capsys):
    from bayesdll_amd.run import build_parser, check_diversity
    ap = build_parser()
    for extra in ([], ["--stacked_chains", "1"]):
        with pytest.raises(SystemExit):
            check_diversity(ap, ap.parse_args(["--method", "sgld", "--diversity"] + extra))
        assert "--stacked_chains" in capsys.readouterr().err
    assert check_diversity(ap, ap.parse_args(["--method", "sgld", "--diversity",
                                              "--stacked_chains", "2"]))


# ------------------------------------------------- layout, sizes, validation
NULL, ALIGN, ARG = -1, -2, -3
ARGS = ["logits", "labels", "totals", "workspace", "batch", "voters", "classes", "grid_blocks",
        "flags"]


def test_ctypes_mirror_matches_the_c_header(tmp_path):
    import ctypes as C
    import subprocess

    from bayesdll_amd import _lib as L
    st = "bdl_diversity_args"
    lines = [f'printf("{st} %zu\\n", sizeof({st}));']
    lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in ARGS]
    lines.append('printf("header %zu\\n", sizeof(bdl_diversity_header));')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_diversity.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().strip().splitlines()
    lay = {k: v for k, v in (ln.split(" ", 1) for ln in out)}
    assert int(lay[st]) == C.sizeof(L.DiversityArgs) == 56 and int(lay["header"]) == 32
    assert [f for f, _ in L.DiversityArgs._fields_] == ARGS
    for f in ARGS:
        assert getattr(L.DiversityArgs, f).offset == int(lay[f"{st}.{f}"]), f


def test_sizes_and_exports():
    from bayesdll_amd import _lib as L
    h = L.lib()
    tb, wb = h.bdl_diversity_totals_bytes, h.bdl_diversity_workspace_bytes
    for P in (2, 3, 17, 64):
        assert tb(P) == 32 + 40 * P * P == L.diversity_totals_dtype(P).itemsize
        assert wb(P, 7) == 7 * R.partial_bytes(P)
        cap = max(1, min(R.DEFAULT_WORKSPACE // R.partial_bytes(P), R.MAX_GRID))
        assert wb(P, 0) == cap * R.partial_bytes(P) <= R.DEFAULT_WORKSPACE
    assert wb(64, 0) == 204 * 163872 and wb(3, 1) == 400     # 392 B rounded up to 16
    for bad in (1, 0, -1, 65):
        assert tb(bad) == 0 and wb(bad, 1) == 0
    assert wb(2, -1) == 0 and wb(2, 1025) == 0
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    for other in (L.EXPORTS, L.PREDICT_EXPORTS, L.MIXTURE_EXPORTS, L.RANK_EXPORTS):
        assert not set(L.DIVERSITY_EXPORTS) & set(other)


def _good():
    """P = 3, B = 10, C = 7: logits 840 B, labels 80 B, totals 392 B, the
    workspace (grid_blocks = 2) 800 B."""
    from bayesdll_amd import _lib as L
    a = L.DiversityArgs()
    a.logits, a.labels, a.totals, a.workspace = 0x10000, 0x20000, 0x50000, 0x100000
    a.batch, a.voters, a.classes, a.grid_blocks, a.flags = 10, 3, 7, 2, 0
    return a


def check_refusals():
    """Every refusal of bdl_diversity by its status code; validation comes
    before any HIP call, so the planted addresses are never touched."""
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, **fields):
        a = _good()
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_diversity(a, None) == status, (fields, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_diversity:") and word in msg, (fields, msg)

    assert h.bdl_diversity(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in ("logits", "totals", "workspace"):
        refused(NULL, b"null " + f.encode(), **{f: None})
    for f in ("logits", "workspace"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x700008})
    for f in ("labels", "totals"):
        refused(ALIGN, f.encode() + b" not 8-B aligned", **{f: 0x700004})
    for v in (1, 0, -1, 65):
        refused(ARG, b"voters in", voters=v)
    refused(ARG, b"batch must be", batch=0)
    for v in (0, 8193):
        refused(ARG, b"classes in", classes=v)
    for v in (-1, 1025):
        refused(ARG, b"grid_blocks in", grid_blocks=v)
    refused(ARG, b"unknown flag", flags=2)
    refused(ARG, b"overflows", batch=2 ** 61 // 21 + 1)
    refused(ARG, b"totals overlaps logits", totals=0x10000 + 832)
    refused(ARG, b"totals overlaps labels", totals=0x20000 - 384)
    refused(ARG, b"workspace overlaps logits", workspace=0x10000 - 800 + 16)
    refused(ARG, b"workspace overlaps labels", workspace=0x20000 + 64)
    refused(ARG, b"workspace overlaps totals", workspace=0x50000 + 384)
    # spans just clear of their neighbours, the largest in-range arguments and a
    # null labels pass validation up to a planted last check
    a = _good()
    a.totals, a.workspace, a.labels, a.flags = 0x10000 + 840, 0x50000 + 400, None, 2
    assert h.bdl_diversity(a, None) == ARG and b"unknown flag" in h.bdl_last_error()
    # a graph redirect refuses first
    assert h.bdl_graph_redirect(C_void(0x10), C_void(0x20)) == 0
    try:
        assert h.bdl_diversity(_good(), None) == ARG
        assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_diversity(None, None) == NULL


def C_void(v):
    import ctypes
    return ctypes.c_void_p(v)


def test_diversity_validates_before_touching_the_device():
    check_refusals()


def test_kernels_and_sampler_layers_check_before_any_launch(monkeypatch):
    from types import SimpleNamespace

    import torch

    from bayesdll_amd import _lib as L
    from bayesdll_amd import chains, stacked
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    x = torch.zeros(3, 10, 7)
    with pytest.raises(ValueError, match=r"\[P, B, C\]"):
        K.diversity(torch.zeros(10, 7))
    with pytest.raises(ValueError, match="contiguous"):
        K.diversity(torch.zeros(3, 7, 10).transpose(1, 2))
    with pytest.raises(ValueError, match="2 <= voters <= 64"):
        K.diversity(torch.zeros(1, 10, 7))
    with pytest.raises(ValueError, match="2 <= voters <= 64"):
        K.diversity(torch.zeros(65, 2, 2))
    with pytest.raises(ValueError, match="classes <= 8192"):
        K.diversity(torch.zeros(2, 1, 8193))
    with pytest.raises(ValueError, match="grid_blocks in"):
        K.diversity(x, grid_blocks=1025)
    with pytest.raises(ValueError, match="labels must be"):
        K.diversity(x, torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="labels must be"):
        K.diversity(x, torch.zeros(9, dtype=torch.int64))
    assert K.diversity_bytes_per_example(8, 10) == 328
    S = SimpleNamespace(args=SimpleNamespace(), K=1)
    with pytest.raises(ValueError, match="needs K >= 2"):
        stacked._StackedSampler.diversity(S, [])
    monkeypatch.setattr(chains, "world", lambda: 2)
    with pytest.raises(ValueError, match="this process's chains only"):
        stacked._StackedSampler.diversity(SimpleNamespace(args=SimpleNamespace(), K=3), [])
