"""bdl_predict on the host: the fp64 reference (tests/predict_ref.py) against
independent formulations, the emulation of the header's arithmetic contract
within the derived bound on every GPU case, the input conditions that make the
GPU cases' integer outputs exact, the ctypes mirrors against the C header, and
every validation error (the library loads without a GPU; none of these calls
launches anything)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.special
import scipy.stats
import torch

import predict_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NULL, ALIGN, ARG = -1, -2, -3


# ------------------------------------------------- 1. the reference is the definition
@pytest.mark.parametrize("case", [R.CASES[4], R.CASES[8], R.CASES[11]], ids=R.case_id)
def test_reference_against_scipy_torch_and_calibration(case):
    from bayesdll_amd import calibration
    x, lab, r, _ = R.built(case)
    M, G, B, Cn = x.shape
    ok = ~r["nonfinite"]
    x64 = np.where(ok[None, :, :, None], x.astype(np.float64), 0.0)
    # scipy: softmax per member, its mean; logsumexp of the members' log-softmax
    p = scipy.special.softmax(x64, axis=-1)
    pbar = p.mean(0)
    lsm = x64 - scipy.special.logsumexp(x64, axis=-1, keepdims=True)
    logp = scipy.special.logsumexp(lsm, axis=0) - np.log(M)
    # torch fp64: the existing path's formula
    tl = torch.log_softmax(torch.from_numpy(x64), -1).logsumexp(0) - np.log(M)
    sel = ok[..., None] & (r["pbar"] > 1e-290)
    assert np.allclose(np.where(sel, r["logp"], 0), np.where(sel, logp, 0), rtol=0, atol=1e-10)
    assert np.allclose(np.where(sel, r["logp"], 0), np.where(sel, tl.numpy(), 0), rtol=0,
                       atol=1e-10)
    ent = scipy.stats.entropy(pbar, axis=-1)
    ee = scipy.stats.entropy(p, axis=-1).mean(0)
    for name, want in (("entropy", ent), ("expected_entropy", ee), ("mutual_info", ent - ee),
                       ("confidence", pbar.max(-1))):
        assert np.allclose(r[name][ok], want[ok], rtol=0, atol=1e-10), name
    assert np.array_equal(r["pred"][ok], pbar.argmax(-1)[ok])
    votes = x64.argmax(-1)
    assert np.array_equal(r["disagree"][ok], (votes != pbar.argmax(-1)[None]).sum(0)[ok])
    assert (np.isnan(r["entropy"]) == ~ok).all() and (r["pred"][~ok] == -1).all()
    # calibration.analyze on the gathered logp of the labelled, finite examples: softmax of
    # a log-probability row is the row
    for g in range(G):
        t = r["totals"][g]
        rows = np.nonzero(t["okl_mask"])[0]
        finite_rows = rows[np.isfinite(r["logp"][g][rows]).all(-1)]
        if len(finite_rows) != len(rows):   # a masked class: calc_bins cannot take -inf
            rows = finite_rows
            sub = R.reference(x[:, g:g + 1][:, :, rows], lab[rows], R.NB)["totals"][0]
        else:
            sub = t
        ece, mce, nll = calibration.analyze(lab[rows], r["logp"][g][rows], R.NB)
        from bayesdll_amd.kernels import predict_summary
        s = predict_summary(sub, M, R.NB)
        assert abs(s["ece"] - ece) < 1e-12 and abs(s["mce"] - mce) < 1e-12
        assert abs(s["nll"] - nll) < 1e-10
        _, member, accs, confs, sizes = calibration.calc_bins(lab[rows], r["logp"][g][rows], R.NB)
        assert np.array_equal(sub["bin_count"][:R.NB], sizes.astype(np.int64))
        assert np.allclose(s["bins"]["accuracy"], accs, atol=1e-12)
        assert np.allclose(s["bins"]["confidence"], confs, atol=1e-12)
        assert s["error"] == sub["n_wrong"] / sub["n_labelled"]
        assert s["n"] == sub["n"] and s["n_nonfinite"] == sub["n_nonfinite"]


# ---------------------------- 2. the contract's emulation stays within the derived bound
def check_against(got, r, b, what):
    """Per-example outputs and totals of `got` against the reference within the
    bound; integers exact.  Shared with the GPU test."""
    ok = ~r["nonfinite"]
    for k in R.INTS:
        assert np.array_equal(np.asarray(got[k]), r[k]), (what, k)
    for k in R.FLOATS:
        g, w = np.asarray(got[k], dtype=np.float64), r[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
        sel = ~np.isnan(w) & np.isfinite(b[k])
        err = np.abs(g[sel] - w[sel])
        assert (err <= b[k][sel]).all(), (what, k, float(err.max()), float(b[k][sel].min()))
    if "logp" in got:
        g, w, bb = np.asarray(got["logp"], dtype=np.float64), r["logp"], b["logp"]
        assert np.array_equal(np.isnan(g), ~np.broadcast_to(ok[..., None], g.shape)), what
        sel = np.broadcast_to(ok[..., None], g.shape) & np.isfinite(bb)
        assert (np.abs(g[sel] - w[sel]) <= bb[sel]).all(), (what, "logp")
        loose = np.broadcast_to(ok[..., None], g.shape) & ~np.isfinite(bb)
        assert (g[loose] <= np.maximum(w[loose], np.log(R.TINY)) + 1).all(), (what, "unbounded logp")


def check_totals(got, r, b, what, scale=1):
    """got: a list per group of mappings with bdl_predict_totals' fields;
    `scale`: how many times the case was accumulated."""
    for g, (t, bt) in enumerate(zip(r["totals"], b["totals"])):
        for k in R.INT_TOTALS:
            assert int(got[g][k]) == scale * t[k], (what, g, k, int(got[g][k]), t[k])
        assert np.array_equal(np.asarray(got[g]["bin_count"]), scale * t["bin_count"]), (what, g)
        assert np.array_equal(np.asarray(got[g]["bin_hits"]), scale * t["bin_hits"]), (what, g)
        for k in R.SUM_TOTALS:
            err = abs(float(got[g][k]) - scale * t[k])
            assert err <= scale * bt[k], (what, g, k, err, bt[k])
        err = np.abs(np.asarray(got[g]["bin_conf"]) - scale * t["bin_conf"])
        assert (err <= scale * bt["bin_conf"]).all(), (what, g, "bin_conf")


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_emulation_of_the_contract_is_within_the_bound(case):
    x, lab, r, b = R.built(case)
    em = R.emulate(x, lab, R.NB)
    check_against(em, r, b, R.case_id(case))
    check_totals(em["totals"], r, b, R.case_id(case))
    if case[1] == 1:   # one member: the mixture is the member
        ok = ~r["nonfinite"]
        assert (np.abs(r["mutual_info"][ok]) <= 1e-12).all() and (r["disagree"][ok] == 0).all()
        assert (np.abs(em["mutual_info"][ok]) <= b["mutual_info"][ok]).all()


# ------------------------------------- 3. the GPU cases' inputs are away from every decision
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_input_conditions_of_the_gpu_cases(case):
    """No reference probability within 4 bounds of a bin edge, no example's top
    two mixture probabilities within 4 bounds of each other, no member row with
    two maxima — for ALL examples; only the constructed ties (bit-equal
    logits: examples 3, and 7's all -inf row) are exempt."""
    x, lab, r, b = R.built(case)
    Cn, M, G, B = case[:4]
    m = R.margins(r, b, R.NB)
    assert m["edge"] >= 4, m
    assert m["top2"] >= 4, m
    tied = np.zeros((G, B), bool)
    if B >= 5 and Cn > 1:
        tied[:, 3] = True
    assert np.array_equal(m["tied"] & ~r["nonfinite"], tied), "only the constructed tie"
    mt = R.member_ties(x)
    allowed = np.zeros((M, G, B), bool)
    if B >= 5 and Cn > 1:
        allowed[:, :, 3] = True
    if B >= 8 and Cn > 1:
        allowed[M - 1, :, 7] = True
    assert np.array_equal(mt, allowed)
    # the constructed examples are what the builder says
    if B >= 8:
        assert r["nonfinite"][:, 5:8].all() and r["nonfinite"].sum() == 3 * G
        assert all(t["n_nonfinite"] == 3 and t["n"] == B - 3 for t in r["totals"])
    else:
        assert not r["nonfinite"].any()
    if B >= 5:
        assert (r["pred"][:, 3] == 0).all()
        assert all(t["n_labelled"] == t["n"] - 2 for t in r["totals"])
        if Cn > 1:
            assert (r["pbar"][:, 4, Cn // 2] == 0).all() and (r["logp"][:, 4, Cn // 2] == -np.inf).all()
            assert (r["pbar"][:, 2, Cn - 1] < 1e-90).all()     # the spread underflows in fp32
    if M == 1:
        ok = ~r["nonfinite"]
        assert (r["disagree"][ok] == 0).all()


def test_cases_reach_every_instance_of_launch_by_classes():
    """launch_by_classes' ladder restated (its text is held below): trips 1 on a
    wave, 1, 2, 4, 8 on a workgroup, each in 16-B loads and element by element."""
    def instance(Cn):
        q = (Cn + 3) // 4
        nt = 1 if Cn <= 256 or q <= 256 else 2 if q <= 512 else 4 if q <= 1024 else 8
        return nt, Cn % 4 == 0, Cn <= 256
    flat = " ".join(open(os.path.join(ROOT, "bayesdll_amd", "csrc", "bdl_predict.hip")).read().split())
    for text in ("if (a.classes <= BDL_PREDICT_WAVE_CLASSES) launch<1, VEC, true>",
                 "else if (groups4 <= kBlock) launch<1, VEC, false>",
                 "else if (groups4 <= 2 * kBlock) launch<2, VEC, false>",
                 "else if (groups4 <= 4 * kBlock) launch<4, VEC, false>",
                 "else launch<8, VEC, false>"):
        assert text in flat, text
    every = {(nt, vec, wave) for nt, wave in ((1, True), (1, False), (2, False), (4, False), (8, False))
             for vec in (True, False)}
    assert {instance(c[0]) for c in R.CASES} == every and len(every) == 10
    assert {instance(c[0]) for c in R.CASES[:22]} == every - {(2, False, False), (4, True, False)}


# ------------------------------------------------------- 4. header, ctypes, exports
ARGS_FIELDS = ["logits", "labels", "logp", "entropy", "expected_entropy", "mutual_info",
               "confidence", "nll", "pred", "disagree", "totals", "workspace", "batch", "members",
               "groups", "classes", "num_bins", "grid_blocks", "flags", "edges"]
TOTALS_FIELDS = ["n", "n_labelled", "n_nonfinite", "n_wrong", "disagree_sum", "nll_sum",
                 "entropy_sum", "expected_entropy_sum", "mi_sum", "mi_sum_wrong", "bin_count",
                 "bin_hits", "bin_conf"]
FUNCS = ["bdl_predict", "bdl_predict_workspace_bytes"]


def test_header_declares_the_two_functions_and_states_the_contract():
    src = open(os.path.join(INCLUDE, "bdl_predict.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(re.findall(r"\b(bdl_\w+)\s*\(", code)) == FUNCS
    assert "BDL_ABI_VERSION" not in code and '#include "bdl_sgmcmc.h"' in code
    flat = " ".join(src.split())
    for word in ("Arithmetic contract", "expf", "logf", "1 ulp", "fp64", "No atomics",
                 "BDL_PREDICT_WAVE_CLASSES", "lowest index", "NON-FINITE"):
        assert word in flat, word


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    structs = (("bdl_predict_args", ARGS_FIELDS, L.PredictArgs),
               ("bdl_predict_totals", TOTALS_FIELDS, L.PredictTotals))
    lines = []
    for st, fields, _ in structs:
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    lines.append('printf("limits %d %d %d %d %d %d\\n", BDL_PREDICT_MAX_CLASSES, '
                 'BDL_PREDICT_WAVE_CLASSES, BDL_PREDICT_MAX_BINS, BDL_PREDICT_MAX_GROUPS, '
                 'BDL_PREDICT_MAX_GRID, (int)BDL_PREDICT_RESET);')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_predict.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    out = subprocess.check_output([str(exe)]).decode().strip().splitlines()
    lay = {k: v for k, v in (ln.split(" ", 1) for ln in out)}
    for name, fields, cls in structs:
        assert int(lay[name]) == C.sizeof(cls), name
        assert [f for f, _ in cls._fields_] == fields
        for f in fields:
            assert getattr(cls, f).offset == int(lay[f"{name}.{f}"]), (name, f)
    assert lay["limits"] == (f"{L.PREDICT_MAX_CLASSES} {L.PREDICT_WAVE_CLASSES} "
                             f"{L.PREDICT_MAX_BINS} {L.PREDICT_MAX_GROUPS} {L.PREDICT_MAX_GRID} "
                             f"{L.PREDICT_RESET}") == "8192 256 64 65535 1024 1"
    assert np.dtype(L.PredictTotals).itemsize == C.sizeof(L.PredictTotals) == 1616
    assert np.dtype(L.PredictTotals).fields["bin_conf"][0].shape == (64,)


def test_library_exports_the_unit_next_to_the_pinned_abi():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert sorted(L.PREDICT_EXPORTS) == FUNCS
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS, L.CHAIN_STEP_EXPORTS,
                  L.STATS_EXPORTS, L.ESS_EXPORTS, L.LOWP_EXPORTS, L.LAYERS_EXPORTS):
        assert not set(L.PREDICT_EXPORTS) & set(other)
    for name in FUNCS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    wb = h.bdl_predict_workspace_bytes
    assert wb(1, 1) == 1616 and wb(3, 7) == 3 * 7 * 1616 and wb(2, 0) == wb(2, 1024)
    assert wb(65535, 1024) == 65535 * 1024 * 1616           # no 32-bit overflow
    for bad in ((0, 1), (-1, 1), (65536, 1), (1, -1), (1, 1025)):
        assert wb(*bad) == 0, bad
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_predict" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "include/bdl_predict.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]


# --------------------------------------------------------------- 5. validation
def _good():
    """M = 2, G = 3, B = 5, C = 8: logits 960 B, labels 40 B, logp 480 B, the
    [G, B] outputs 60 B each, totals 3 x 1616 B, the workspace at grid 2
    9696 B."""
    from bayesdll_amd import _lib as L
    a = L.PredictArgs()
    a.logits, a.labels, a.logp = 0x10000, 0x20000, 0x30000
    for i, f in enumerate(("entropy", "expected_entropy", "mutual_info", "confidence", "nll",
                           "pred", "disagree")):
        setattr(a, f, 0x40000 + 0x1000 * i)
    a.totals, a.workspace = 0x50000, 0x100000
    a.batch, a.members, a.groups, a.classes, a.num_bins, a.grid_blocks = 5, 2, 3, 8, 15, 2
    for i, e in enumerate(R.edges32(15)):
        a.edges[i] = float(e)
    return a


def test_entry_point_validates_before_touching_the_device():
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, edges=None, **fields):
        a = _good()
        for k, v in fields.items():
            setattr(a, k, v)
        for i, e in (edges or {}).items():
            a.edges[i] = e
        assert h.bdl_predict(a, None) == status, (fields, edges, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_predict:") and word in msg, (fields, msg)

    assert h.bdl_predict(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in ("logits", "totals", "workspace"):
        refused(NULL, f.encode(), **{f: None})
    for f in ("logits", "logp", "workspace"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x700008})
    for f in ("entropy", "expected_entropy", "mutual_info", "confidence", "nll", "pred",
              "disagree", "labels", "totals"):
        refused(ALIGN, f.encode() + b" not 8-B aligned", **{f: 0x700004})
    refused(ARG, b"members", members=0)
    refused(ARG, b"groups", groups=0)
    refused(ARG, b"groups", groups=65536)
    refused(ARG, b"batch", batch=0)
    refused(ARG, b"classes", classes=0)
    refused(ARG, b"classes", classes=8193)
    refused(ARG, b"num_bins", num_bins=0)
    refused(ARG, b"num_bins", num_bins=65)
    refused(ARG, b"grid_blocks", grid_blocks=-1)
    refused(ARG, b"grid_blocks", grid_blocks=1025)
    refused(ARG, b"unknown flag", flags=2)
    refused(ARG, b"overflows", batch=1 << 58)
    refused(ARG, b"overflows", batch=1 << 40, members=1 << 20, groups=60000, classes=8192)
    refused(ARG, b"edges", edges={0: 0.0})
    refused(ARG, b"edges", edges={3: float(R.edges32(15)[2])})  # equal neighbours: not strict
    refused(ARG, b"edges", edges={13: 1.0})
    refused(ARG, b"edges", edges={5: float("nan")})
    # written spans against the inputs and one another
    refused(ARG, b"logp overlaps logits", logp=0x10000 + 944)
    refused(ARG, b"entropy overlaps logits", entropy=0x10000 - 56)
    refused(ARG, b"pred overlaps labels", pred=0x20000 + 32)
    refused(ARG, b"nll overlaps logp", nll=0x30000 + 472)
    refused(ARG, b"disagree overlaps pred", disagree=0x45000 + 56)
    refused(ARG, b"totals overlaps logits", totals=0x10000 + 8)
    refused(ARG, b"totals overlaps confidence", totals=0x43000 + 56)
    refused(ARG, b"workspace overlaps logits", workspace=0x10000 - 9696 + 16)
    refused(ARG, b"workspace overlaps totals", workspace=0x50000 + 3 * 1616 - 16)
    refused(ARG, b"workspace overlaps totals", totals=0x900000,
            workspace=0x900000 - 3 * 1024 * 1616 + 16, grid_blocks=0)
    # the nullable outputs are nullable
    a = _good()
    a.grid_blocks = 1025
    for f in ("labels", "logp", "entropy", "pred", "disagree"):
        setattr(a, f, None)
    assert h.bdl_predict(a, None) == ARG and b"grid_blocks" in h.bdl_last_error()


def test_entry_point_refuses_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_predict(_good(), None) == ARG
        assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_predict(None, None) == NULL


def test_kernels_layer_checks_its_arguments_before_any_launch(monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    x = torch.zeros(4, 5, 8)
    with pytest.raises(ValueError, match="want from"):
        K.predict(x, want=("probs",))
    with pytest.raises(ValueError, match="members x groups"):
        K.predict(x, groups=3)
    with pytest.raises(ValueError, match="contiguous"):
        K.predict(x.transpose(0, 1))
    with pytest.raises(ValueError, match="classes"):
        K.predict(torch.zeros(1, 1, 8193))
    with pytest.raises(ValueError, match="num_bins"):
        K.predict(x, num_bins=65)
    with pytest.raises(ValueError, match="grid_blocks"):
        K.predict(x, grid_blocks=1025)
    with pytest.raises(ValueError, match="labels"):
        K.predict(x, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="labels"):
        K.predict(x, torch.zeros(4, dtype=torch.int64))
    assert np.array_equal(K.predict_edges(15), R.edges32(15))
    e = K.predict_edges(64)
    assert len(e) == 63 and (np.diff(e) > 0).all() and 0 < e[0] and e[-1] < 1


def test_summary_of_empty_totals_is_nan_not_an_error():
    from bayesdll_amd import _lib as L
    from bayesdll_amd.kernels import predict_summary
    row = np.zeros(1, dtype=np.dtype(L.PredictTotals))[0]
    s = predict_summary(row, 4, 15)
    assert s["n"] == 0 and np.isnan(s["nll"]) and np.isnan(s["ece"]) and np.isnan(s["entropy"])
