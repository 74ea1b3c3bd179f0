"""bdl_rank on the host: the reference's two forms against each other on table
R, a CPU proof that R reaches every launch path of the count kernel, the export
table, the ctypes mirrors against the C header, the workspace size, every
validation refusal of the entry point (the library loads without a GPU; none of
these calls launches anything), the kernels layer's and the sampler's own
checks, and run.py's --detect / --detect_shift argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NULL, ALIGN, ARG = -1, -2, -3
FUNCS = ["bdl_rank", "bdl_rank_workspace_bytes"]
INTS = ("n_pos", "n_neg", "n_excluded", "u2", "fp_at_tpr")
COUNTS = ("ge_pos", "ge_neg", "gt_neg")


# ------------------------------------------------- 1. the reference's two forms
@pytest.mark.parametrize("name", R.CASE_IDS)
def test_the_two_reference_forms_agree(name):
    case = R.CASES[name]
    a, b = R.reference_of(name), R.reference(case, R.row_sorted)
    for r, (x, y) in enumerate(zip(a, b)):
        for k in INTS:
            assert x[k] == y[k], (name, r, k)
        for k in COUNTS:
            assert np.array_equal(x[k], y[k]), (name, r, k)
        assert abs(x["ap_sum"] - y["ap_sum"]) <= x["n_pos"] * 2.0 ** -52, (name, r)
        n = case["scores"].shape[1]
        assert x["n_pos"] + x["n_neg"] + x["n_excluded"] == n
        assert 0 <= x["u2"] <= 2 * x["n_pos"] * x["n_neg"]
        assert -1 <= x["fp_at_tpr"] <= x["n_neg"] and (x["fp_at_tpr"] >= 0) == (x["n_pos"] > 0)


def test_reference_on_cases_worked_by_hand():
    # scores 3 2 2 1, marks + - + -: pairs (3>2, 3>1, 2=2 half, 2>1) -> U = 3.5
    r = R.row_loop([3, 2, 2, 1], [1, 0, 1, 0])
    assert (r["n_pos"], r["n_neg"], r["u2"]) == (2, 2, 7) and R.auroc(r) == 0.875
    assert r["ge_pos"].tolist() == [1, 2, 2, 2] and r["ge_neg"].tolist() == [0, 1, 1, 2]
    assert r["gt_neg"].tolist() == [0, 0, 0, 1]
    assert r["fp_at_tpr"] == 1 and r["ap_sum"] == 1.0 + 2 / 3   # need = ceil(1.9) = 2
    # -0.0 ties +0.0; a NaN and a mark 2 are excluded; the infinities are ordered
    r = R.row_loop([0.0, -0.0, np.nan, np.inf, -np.inf, 5.0], [1, 0, 1, 1, 0, 2])
    assert (r["n_pos"], r["n_neg"], r["n_excluded"], r["u2"]) == (2, 2, 2, 4 + 3)
    # two subnormals are ordered, not flushed to a tie
    r = R.row_loop([R.SUB, 2 * R.SUB], [0, 1])
    assert r["u2"] == 2 and R.row_loop([R.SUB, R.SUB], [0, 1])["u2"] == 1
    # all tied: AUROC one half, whatever the marks
    for name in (n for n in R.CASE_IDS if n.endswith("patterns")):
        row = R.CASES[name]["rows"].index("all_tied")
        ref = R.reference_of(name)[row]
        if ref["n_pos"] and ref["n_neg"]:
            assert R.auroc(ref) == 0.5


def test_average_precision_is_sklearns_definition():
    """AP = sum over distinct thresholds of (R_k - R_{k-1}) * P_k, descending."""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 12, 200).astype(np.float32)
    m = rng.integers(0, 2, 200).astype(np.int32)
    r = R.row_loop(x, m)
    P, ap, prev = int(m.sum()), 0.0, 0
    for v in sorted(set(x.tolist()), reverse=True):
        tp, fp = int(((x >= v) & (m == 1)).sum()), int(((x >= v) & (m == 0)).sum())
        ap += (tp - prev) / P * (tp / (tp + fp))
        prev = tp
    assert abs(r["ap_sum"] / P - ap) < 1e-13


# ---------------------------------------------- 2. R reaches every launch path
def test_table_r_reaches_every_launch_path_of_the_count_kernel():
    assert R.U == 2 and R.ITILE == 512 and R.JTILE == 1024
    flat = " ".join(open(os.path.join(ROOT, "bayesdll_amd", "csrc", "bdl_rank.hip")).read().split())
    # what count_paths restates
    for piece in ("dim3(itiles, (unsigned)d->rows)", "(d->n + kITile - 1) / kITile",
                  "(int64_t)blockIdx.x * kITile + u * kBlock + t",
                  "const bool aligned = ((sbase | mbase) & 3) == 0;",
                  "if (__syncthreads_or(any))", "for (int64_t j0 = 0; j0 < n; j0 += kJTile)",
                  "const int64_t e = j0 + 4 * t;", "if (aligned && e + 4 <= n)",
                  "if (e + c < n)", "left >= kJTile ? kBlock : (int)((left + 3) >> 2)"):
        assert piece in flat, piece
    seen, by_case = set(), {}
    for name in R.CASE_IDS:
        by_case[name] = R.count_paths(R.CASES[name])
        seen |= by_case[name]
    assert seen == R.ALL_PATHS
    big = 3 * R.ITILE + 5
    assert {"i_tile_full", "i_tile_partial", "j_tile_full", "j_tile_partial", "row_unaligned",
            "elementwise_unaligned", "no_valid_i", "load_16B"} <= by_case[f"n{big}-patterns"]
    assert "guarded_tail" in by_case["n257-patterns"] | by_case["n2-patterns"]
    assert by_case[f"n{R.ITILE}-patterns"] >= {"row_aligned", "load_16B", "i_tile_full"}
    assert "row_unaligned" not in by_case[f"n{R.ITILE}-patterns"]
    # every mark layout: per row, per group of 5, one group, shared
    shapes = {(c["scores"].shape[0], c["marks"].shape[0], c["spg"]) for c in R.CASES.values()}
    assert {(15, 3, 5), (5, 1, 5), (3, 1, 1)} <= shapes
    assert {n for c in R.CASES.values() for n in [c["scores"].shape[1]]} == set(R.SIZES)


# ------------------------------------------------ 3. header, ctypes, exports
def test_export_table_is_disjoint_and_the_library_exports_it():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert sorted(L.RANK_EXPORTS) == FUNCS
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS, L.CHAIN_STEP_EXPORTS,
                  L.STATS_EXPORTS, L.ESS_EXPORTS, L.LOWP_EXPORTS, L.LAYERS_EXPORTS,
                  L.PREDICT_EXPORTS, L.FN_EXPORTS, L.TEMPER_EXPORTS, L.MIXTURE_EXPORTS):
        assert not set(L.RANK_EXPORTS) & set(other)
    for name in FUNCS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_rank" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "include/bdl_rank.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "bdl_rank.h")).read(), flags=re.S)
    assert sorted(re.findall(r"\b(bdl_\w+)\s*\(", code)) == FUNCS
    assert "BDL_ABI_VERSION" not in code and '#include "bdl_sgmcmc.h"' in code


ARGS = ["scores", "marks", "ge_pos", "ge_neg", "gt_neg", "totals", "workspace", "n", "need",
        "rows", "scores_per_group", "mark_rows", "tpr_num", "tpr_den", "pad0"]
FIELDS = ["n_pos", "n_neg", "n_excluded", "u2", "fp_at_tpr", "ap_sum"]


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    structs = (("bdl_rank_args", ARGS, L.RankArgs), ("bdl_rank_totals", FIELDS, L.RankTotals))
    lines = []
    for st, fields, _ in structs:
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    lines.append('printf("limits %d %d %d %d\\n", BDL_RANK_U, BDL_RANK_ITILE, BDL_RANK_JTILE, '
                 'BDL_RANK_MAX_ROWS);')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_rank.h\"\n"
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
    assert lay["limits"] == f"{L.RANK_U} {L.RANK_ITILE} {L.RANK_JTILE} {L.RANK_MAX_ROWS}" \
        == "2 512 1024 65535"
    assert C.sizeof(L.RankTotals) == np.dtype(L.RankTotals).itemsize == 48
    assert C.sizeof(L.RankArgs) == 96 and (R.U, R.ITILE, R.JTILE) == (2, 512, 1024)


def test_workspace_size():
    from bayesdll_amd import _lib as L
    wb = L.lib().bdl_rank_workspace_bytes
    assert wb(1, 1) == 16 and wb(1, 4) == 48 and wb(5, 1541) == (5 * 1541 * 12 + 15) // 16 * 16
    assert wb(65535, 2 ** 31 - 1) == (65535 * (2 ** 31 - 1) * 12 + 15) // 16 * 16  # no overflow
    for bad in ((0, 1), (-1, 1), (65536, 1), (1, 0), (1, -1), (1, 2 ** 31)):
        assert wb(*bad) == 0, bad


# --------------------------------------------------------------- 4. validation
def _good():
    """rows = 6 (3 groups of 2), n = 10: scores 240 B, marks 120 B, the counts
    240 B each, totals 288 B, the workspace 720 B."""
    from bayesdll_amd import _lib as L
    a = L.RankArgs()
    a.scores, a.marks, a.totals, a.workspace = 0x10000, 0x20000, 0x50000, 0x100000
    a.ge_pos, a.ge_neg, a.gt_neg = 0x30000, 0x31000, 0x32000
    a.n, a.rows, a.scores_per_group, a.mark_rows, a.tpr_num, a.tpr_den = 10, 6, 2, 3, 19, 20
    return a


def test_rank_validates_before_touching_the_device():
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, **fields):
        a = _good()
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_rank(a, None) == status, (fields, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_rank:") and word in msg, (fields, msg)

    assert h.bdl_rank(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in ("scores", "marks", "totals", "workspace"):
        refused(NULL, b"null " + f.encode(), **{f: None})
    for f in ("scores", "marks", "workspace"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x700008})
    refused(ALIGN, b"totals not 8-B aligned", totals=0x700004)
    for f in COUNTS:
        refused(ALIGN, f.encode() + b" not 4-B aligned", **{f: 0x700002})
    refused(ARG, b"rows in", rows=0)
    refused(ARG, b"rows in", rows=65536)
    refused(ARG, b"n in", n=0)
    refused(ARG, b"n in", n=2 ** 31)
    refused(ARG, b"scores_per_group must be >= 1", scores_per_group=0)
    refused(ARG, b"must divide rows", scores_per_group=4)
    refused(ARG, b"mark_rows", mark_rows=2)
    refused(ARG, b"mark_rows", mark_rows=6)
    refused(ARG, b"mark_rows", mark_rows=0)
    refused(ARG, b"need", need=-1)
    refused(ARG, b"tpr_num", tpr_num=0)
    refused(ARG, b"tpr_num", tpr_num=21)
    refused(ARG, b"tpr_num", tpr_num=1, tpr_den=0)
    refused(ARG, b"pad0", pad0=1)
    refused(ARG, b"ge_pos overlaps scores", ge_pos=0x10000 + 236)
    refused(ARG, b"ge_neg overlaps marks", ge_neg=0x20000 + 116)
    refused(ARG, b"ge_neg overlaps ge_pos", ge_neg=0x30000 + 236)
    refused(ARG, b"gt_neg overlaps ge_neg", gt_neg=0x31000 - 236)
    refused(ARG, b"totals overlaps scores", totals=0x10000 + 8)
    refused(ARG, b"totals overlaps gt_neg", totals=0x32000 + 232)
    refused(ARG, b"workspace overlaps marks", workspace=0x20000 - 720 + 16)
    refused(ARG, b"workspace overlaps totals", workspace=0x50000 + 288 - 16)
    # the allowed forms pass validation: mark_rows = 1, and the counts are nullable
    # (the next check, a planted one, is reached)
    a = _good()
    a.mark_rows, a.pad0 = 1, 1
    a.ge_pos = a.ge_neg = a.gt_neg = None
    assert h.bdl_rank(a, None) == ARG and b"pad0" in h.bdl_last_error()
    # a span just clear of its neighbour is accepted up to the same planted check
    a = _good()
    a.ge_neg, a.pad0 = 0x30000 + 240, 1
    assert h.bdl_rank(a, None) == ARG and b"pad0" in h.bdl_last_error()


def test_rank_refuses_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_rank(_good(), None) == ARG
        assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_rank(None, None) == NULL


def test_kernels_layer_checks_its_arguments_before_any_launch(monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    x = torch.zeros(6, 10)
    m = torch.zeros(3, 10, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"\[rows, n\]"):
        K.rank(torch.zeros(10), m)
    with pytest.raises(ValueError, match="contiguous"):
        K.rank(torch.zeros(10, 6).t(), m)
    with pytest.raises(ValueError, match="must divide rows"):
        K.rank(x, m, scores_per_group=4)
    with pytest.raises(ValueError, match="marks must be"):
        K.rank(x, m.long(), scores_per_group=2)
    with pytest.raises(ValueError, match="marks must be"):
        K.rank(x, torch.zeros(3, 9, dtype=torch.int32), scores_per_group=2)
    with pytest.raises(ValueError, match="marks has 3 rows"):
        K.rank(x, m, scores_per_group=3)
    with pytest.raises(ValueError, match="need >= 1"):
        K.rank(x, m, scores_per_group=2, need=0)
    with pytest.raises(ValueError, match="need >= 1"):
        K.rank(x, m, scores_per_group=2, tpr=(21, 20))
    with pytest.raises(ValueError, match="totals must be"):
        K.rank(x, m, scores_per_group=2, totals=torch.zeros(10, dtype=torch.uint8))
    row = np.zeros(1, dtype=np.dtype(L.RankTotals))[0]
    s = K.rank_summary(row)
    assert s["n_pos"] == 0 and all(np.isnan(s[k]) for k in ("auroc", "ap", "fpr"))
    row["n_pos"], row["n_neg"], row["u2"], row["fp_at_tpr"], row["ap_sum"] = 2, 2, 7, 1, 5 / 3
    s = K.rank_summary(row)
    assert s["auroc"] == 7 / 8 and s["ap"] == (5 / 3) / 2 and s["fpr"] == 0.5
    row["fp_at_tpr"] = -1
    assert np.isnan(K.rank_summary(row)["fpr"])
    assert K.rank_bytes_per_example() == 36 and K.rank_bytes_per_example(counts=True) == 48


# ------------------------------------------------- 5. the sampler and the CLI
def test_sampler_detection_refusals_before_touching_a_device(monkeypatch):
    from types import SimpleNamespace

    from bayesdll_amd import chains, stacked
    S = SimpleNamespace(args=SimpleNamespace(), K=2)
    with pytest.raises(ValueError, match="detection: scores from"):
        stacked._StackedSampler.detection(S, [], scores=("entropy", "variance"))
    with pytest.raises(ValueError, match="detection: scores from"):
        stacked._StackedSampler.detection(S, [], scores=())
    monkeypatch.setattr(chains, "world", lambda: 2)
    with pytest.raises(ValueError, match="this process's chains only"):
        stacked._StackedSampler.detection(S, [])
    assert stacked.DETECTION_SCORES == ("entropy", "mutual_info", "expected_entropy",
                                        "neg_confidence", "disagree")


def test_run_cli_detect_argument_checks(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    d = ap.parse_args([])
    assert d.detect is False and d.detect_shift is None
    a = ap.parse_args(["--stacked_chains", "4", "--detect", "--detect_shift", "0.5"])
    assert run.check_detect(ap, a) == (True, 0.5)
    for argv, word in ((["--detect"], "it needs --stacked_chains >= 1"),
                       (["--stacked_chains", "2", "--detect_shift", "0.5"], "it needs --detect"),
                       (["--stacked_chains", "2", "--detect", "--detect_shift", "0"],
                        "SIGMA must be > 0"),
                       (["--stacked_chains", "2", "--detect", "--detect_shift", "-1"],
                        "SIGMA must be > 0")):
        with pytest.raises(SystemExit) as e:
            run.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


def test_shifted_loader_is_the_same_examples_plus_seeded_noise():
    from bayesdll_amd import run
    base = [(torch.arange(6.0).view(3, 2), torch.tensor([0, 1, 2])),
            (torch.ones(2, 2), torch.tensor([1, 0]))]
    sh = run.ShiftedLoader(base, 0.5, 7)
    one, two = list(sh), list(sh)
    assert len(sh) == 2 and [len(x) for x, _ in one] == [3, 2]
    g = torch.Generator().manual_seed(7)
    for (x, y), (x1, y1), (x2, y2) in zip(base, one, two):
        assert torch.equal(y, y1) and torch.equal(x1, x2)
        assert torch.equal(x1, x + 0.5 * torch.randn(x.shape, generator=g))
