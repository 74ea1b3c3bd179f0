"""bdl_member_score / bdl_mixture on the host: the export table, the ctypes
mirrors against the C header, the workspace sizes, every validation refusal of
both entry points (the library loads without a GPU; none of these calls
launches anything), the reference's own consistency (tests/mixture_ref.py
against _runner.gmm_weights and mixture_evaluate's torch ops, its emulation of
the contract within the derived bound, the excluded-share cap of every GPU
case) and the samplers' refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mixture_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NULL, ALIGN, ARG = -1, -2, -3
FUNCS = ["bdl_member_score", "bdl_member_score_workspace_bytes", "bdl_mixture",
         "bdl_mixture_workspace_bytes"]


# ------------------------------------------------------- 1. header, ctypes, exports
def test_export_table_is_disjoint_and_the_library_exports_it():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert sorted(L.MIXTURE_EXPORTS) == FUNCS
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS, L.CHAIN_STEP_EXPORTS,
                  L.STATS_EXPORTS, L.ESS_EXPORTS, L.LOWP_EXPORTS, L.LAYERS_EXPORTS,
                  L.PREDICT_EXPORTS, L.FN_EXPORTS, L.TEMPER_EXPORTS):
        assert not set(L.MIXTURE_EXPORTS) & set(other)
    for name in FUNCS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_mixture" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "include/bdl_mixture.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    src = open(os.path.join(INCLUDE, "bdl_mixture.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(re.findall(r"\b(bdl_\w+)\s*\(", code)) == FUNCS
    assert "BDL_ABI_VERSION" not in code and '#include "bdl_sgmcmc.h"' in code


def test_workspace_sizes():
    from bayesdll_amd import _lib as L
    h = L.lib()
    sw, mw = h.bdl_member_score_workspace_bytes, h.bdl_mixture_workspace_bytes
    assert sw(1, 1, 1) == 32 and sw(6, 3, 7) == 6 * 3 * 7 * 32 and sw(2, 3, 0) == sw(2, 3, 1024)
    assert sw(65535, 1, 1024) == 65535 * 1024 * 32          # no 32-bit overflow
    assert sw(255, 257, 1) == 65535 * 32
    for bad in ((0, 1, 1), (1, 0, 1), (256, 256, 1), (65536, 1, 1), (1, 1, -1), (1, 1, 1025)):
        assert sw(*bad) == 0, bad
    assert mw(1, 1) == 32 and mw(3, 7) == 3 * 7 * 32 and mw(2, 0) == mw(2, 1024)
    assert mw(65535, 1024) == 65535 * 1024 * 32
    for bad in ((0, 1), (-1, 1), (65536, 1), (1, -1), (1, 1025)):
        assert mw(*bad) == 0, bad


SCORE_ARGS = ["logits", "labels", "scores", "workspace", "batch", "members", "groups", "classes",
              "grid_blocks", "flags", "pad0"]
SCORE_FIELDS = ["n", "n_nonfinite", "n_wrong", "nll_sum"]
MIX_ARGS = ["logits", "weights", "labels", "logp", "expected_entropy", "totals", "workspace",
            "batch", "components", "draws", "groups", "classes", "combine", "grid_blocks", "flags",
            "pad0"]
MIX_FIELDS = ["n", "n_nonfinite", "expected_entropy_sum"]


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    structs = (("bdl_member_score_args", SCORE_ARGS, L.MemberScoreArgs),
               ("bdl_member_score_t", SCORE_FIELDS, L.MemberScore),
               ("bdl_mixture_args", MIX_ARGS, L.MixtureArgs),
               ("bdl_mixture_totals", MIX_FIELDS, L.MixtureTotals))
    lines = []
    for st, fields, _ in structs:
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    lines.append('printf("limits %d %d %d %d %d %d %d %g\\n", BDL_MIXTURE_MAX_CLASSES, '
                 'BDL_MIXTURE_WAVE_CLASSES, BDL_MIXTURE_MAX_PAIRS, BDL_MIXTURE_MAX_GRID, '
                 '(int)BDL_MIXTURE_RESET, (int)BDL_MIX_ARITHMETIC, (int)BDL_MIX_REFERENCE, '
                 'BDL_MIXTURE_MIN_WEIGHT);')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_mixture.h\"\n"
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
    assert lay["limits"] == (f"{L.MIXTURE_MAX_CLASSES} {L.MIXTURE_WAVE_CLASSES} "
                             f"{L.MIXTURE_MAX_PAIRS} {L.MIXTURE_MAX_GRID} {L.MIXTURE_RESET} "
                             f"{L.MIX_ARITHMETIC} {L.MIX_REFERENCE} {L.MIXTURE_MIN_WEIGHT:g}") \
        == "4096 256 65535 1024 1 0 1 1e-10"
    assert L.MIXTURE_MAX_CLASSES >= 4096 and R.MIN_WEIGHT == L.MIXTURE_MIN_WEIGHT
    assert np.dtype(L.MemberScore).itemsize == 32 and np.dtype(L.MixtureTotals).itemsize == 24


# --------------------------------------------------------------- 2. validation
def _good_score():
    """members = 2, G = 3, B = 5, C = 8: logits 960 B, labels 40 B, scores
    6 x 32 B, the workspace at grid 2 384 B."""
    from bayesdll_amd import _lib as L
    a = L.MemberScoreArgs()
    a.logits, a.labels, a.scores, a.workspace = 0x10000, 0x20000, 0x50000, 0x100000
    a.batch, a.members, a.groups, a.classes, a.grid_blocks = 5, 2, 3, 8, 2
    return a


def _good_mix():
    """components = 2, draws = 1, G = 3, B = 5, C = 8: logits 960 B, weights
    48 B, labels 40 B, logp 480 B, expected_entropy 60 B, totals 3 x 24 B, the
    workspace at grid 2 192 B."""
    from bayesdll_amd import _lib as L
    a = L.MixtureArgs()
    a.logits, a.weights, a.labels, a.logp = 0x10000, 0x18000, 0x20000, 0x30000
    a.expected_entropy, a.totals, a.workspace = 0x40000, 0x50000, 0x100000
    a.batch, a.components, a.draws, a.groups, a.classes, a.grid_blocks = 5, 2, 1, 3, 8, 2
    return a


def _refuser(fn, good, prefix):
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, **fields):
        a = good()
        for k, v in fields.items():
            setattr(a, k, v)
        assert getattr(h, fn)(a, None) == status, (fields, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(prefix) and word in msg, (fields, msg)
    return h, refused


def test_member_score_validates_before_touching_the_device():
    h, refused = _refuser("bdl_member_score", _good_score, b"bdl_member_score:")
    assert h.bdl_member_score(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in ("logits", "labels", "scores", "workspace"):
        refused(NULL, f.encode(), **{f: None})
    for f in ("logits", "workspace"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x700008})
    for f in ("labels", "scores"):
        refused(ALIGN, f.encode() + b" not 8-B aligned", **{f: 0x700004})
    refused(ARG, b"members", members=0)
    refused(ARG, b"groups", groups=0)
    refused(ARG, b"members * groups", members=256, groups=256)
    refused(ARG, b"batch", batch=0)
    refused(ARG, b"classes", classes=0)
    refused(ARG, b"classes", classes=4097)
    refused(ARG, b"grid_blocks", grid_blocks=-1)
    refused(ARG, b"grid_blocks", grid_blocks=1025)
    refused(ARG, b"unknown flag", flags=2)
    refused(ARG, b"overflows", batch=1 << 58)
    refused(ARG, b"overflows", batch=1 << 40, members=65535, groups=1, classes=4096)
    refused(ARG, b"scores overlaps logits", scores=0x10000 + 952)
    refused(ARG, b"scores overlaps labels", scores=0x20000 + 32)
    refused(ARG, b"workspace overlaps logits", workspace=0x10000 - 384 + 16)
    refused(ARG, b"workspace overlaps scores", workspace=0x50000 + 6 * 32 - 16)
    refused(ARG, b"workspace overlaps scores", scores=0x900000,
            workspace=0x900000 - 6 * 1024 * 32 + 16, grid_blocks=0)


def test_mixture_validates_before_touching_the_device():
    h, refused = _refuser("bdl_mixture", _good_mix, b"bdl_mixture:")
    assert h.bdl_mixture(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in ("logits", "weights", "totals", "workspace"):
        refused(NULL, f.encode(), **{f: None})
    for f in ("logits", "logp", "workspace"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x700008})
    for f in ("weights", "labels", "expected_entropy", "totals"):
        refused(ALIGN, f.encode() + b" not 8-B aligned", **{f: 0x700004})
    refused(ARG, b"components", components=0)
    refused(ARG, b"draws", draws=0)
    refused(ARG, b"components * draws", components=1 << 20, draws=1 << 12)
    refused(ARG, b"groups", groups=0)
    refused(ARG, b"groups", groups=65536)
    refused(ARG, b"batch", batch=0)
    refused(ARG, b"classes", classes=0)
    refused(ARG, b"classes", classes=4097)
    refused(ARG, b"grid_blocks", grid_blocks=-1)
    refused(ARG, b"grid_blocks", grid_blocks=1025)
    refused(ARG, b"unknown flag", flags=2)
    refused(ARG, b"unknown combine", combine=2)
    refused(ARG, b"unknown combine", combine=-1)
    refused(ARG, b"overflows", batch=1 << 58)
    refused(ARG, b"overflows", batch=1 << 40, components=1 << 20, groups=60000, classes=4096)
    refused(ARG, b"logp overlaps logits", logp=0x10000 + 944)
    refused(ARG, b"logp overlaps weights", logp=0x18000 + 32)
    refused(ARG, b"expected_entropy overlaps labels", expected_entropy=0x20000 + 32)
    refused(ARG, b"expected_entropy overlaps logp", expected_entropy=0x30000 + 472)
    refused(ARG, b"totals overlaps logits", totals=0x10000 + 8)
    refused(ARG, b"totals overlaps expected_entropy", totals=0x40000 + 56)
    refused(ARG, b"workspace overlaps logits", workspace=0x10000 - 192 + 16)
    refused(ARG, b"workspace overlaps totals", workspace=0x50000 + 3 * 24 - 8)
    # the nullable ones are nullable: the next check is reached
    a = _good_mix()
    a.grid_blocks = 1025
    for f in ("labels", "logp", "expected_entropy"):
        setattr(a, f, None)
    assert h.bdl_mixture(a, None) == ARG and b"grid_blocks" in h.bdl_last_error()


def test_entry_points_refuse_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_member_score(_good_score(), None) == ARG
        assert b"graph redirect is active" in h.bdl_last_error()
        assert h.bdl_mixture(_good_mix(), None) == ARG
        assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_mixture(None, None) == NULL


def test_kernels_layer_checks_its_arguments_before_any_launch(monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    x = torch.zeros(4, 5, 8)
    y = torch.zeros(5, dtype=torch.int64)
    w = torch.ones(2, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="labels"):
        K.member_score(x, None, groups=1)
    with pytest.raises(ValueError, match="labels"):
        K.member_score(x, torch.zeros(5, dtype=torch.int32), groups=1)
    with pytest.raises(ValueError, match="members x groups"):
        K.member_score(x, y, groups=3)
    with pytest.raises(ValueError, match="contiguous"):
        K.member_score(x.transpose(0, 1), y, groups=1)
    with pytest.raises(ValueError, match="classes"):
        K.member_score(torch.zeros(1, 1, 4097), torch.zeros(1, dtype=torch.int64), groups=1)
    with pytest.raises(ValueError, match="grid_blocks"):
        K.member_score(x, y, groups=1, grid_blocks=1025)
    with pytest.raises(ValueError, match="pairs"):
        K.member_score(torch.zeros(65536, 1, 1), torch.zeros(1, dtype=torch.int64), groups=1)
    with pytest.raises(ValueError, match="want from"):
        K.mixture(x, w, draws=2, groups=1, want=("probs",))
    with pytest.raises(ValueError, match="combine from"):
        K.mixture(x, w, draws=2, groups=1, combine="geometric")
    with pytest.raises(ValueError, match="components x draws"):
        K.mixture(x, w, draws=3, groups=1)
    with pytest.raises(ValueError, match="weights"):
        K.mixture(x, w.float(), draws=2, groups=1)
    with pytest.raises(ValueError, match="weights"):
        K.mixture(x, torch.ones(4, 1, dtype=torch.float64), draws=2, groups=1)
    with pytest.raises(ValueError, match="labels"):
        K.mixture(x, w, torch.zeros(4, dtype=torch.int64), draws=2, groups=1)
    s = K.mixture_summary(np.zeros(1, dtype=np.dtype(L.MixtureTotals))[0])
    assert s["n"] == 0 and np.isnan(s["expected_entropy"])


# ------------------------------------------- 3. the reference's own consistency
def test_cycle_weights_are_the_runner_formula_per_chain_and_the_joint_one():
    from bayesdll_amd import stacked
    from bayesdll_amd._runner import gmm_weights
    rng = np.random.default_rng(5)
    lik = {c: np.exp(-rng.random((3, 4)) * 3) for c in (0, 2, 5)}
    for c in lik:
        lik[c][:, 3] = 0.0                       # a chain no draw of which explains anything
    keys = [0, 2, 5]
    w = stacked.cycle_weights(lik, keys, by_chain=True)
    assert w.shape == (3, 4) and w.dtype == np.float64
    with np.errstate(divide="ignore"):
        for k in range(4):
            want = gmm_weights({c: list(lik[c][:, k]) for c in keys})
            assert np.array_equal(w[:, k], [want[c] for c in keys])
    assert np.allclose(w.sum(0), 1.0, atol=1e-15)
    assert np.array_equal(w[:, 3], [1 / 3] * 3)  # the all-zero fallback: uniform
    # by hand: w_c = 1 / mean(1 / lik), normalised
    raw = np.array([1.0 / np.mean(1.0 / lik[c][:, 0]) for c in keys])
    assert np.allclose(w[:, 0], raw / raw.sum(), rtol=1e-15)
    j = stacked.cycle_weights(lik, keys, by_chain=False)
    with np.errstate(divide="ignore"):
        rawj = np.stack([1.0 / np.mean(1.0 / lik[c], axis=0) for c in keys])
    assert np.allclose(j, rawj / rawj.sum(), rtol=1e-15) and abs(j.sum() - 1) < 1e-15
    assert (j[:, 3] == 0).all()
    zero = {c: np.zeros((2, 2)) for c in keys}
    assert np.array_equal(stacked.cycle_weights(zero, keys, by_chain=False), np.full((3, 2), 1 / 6))
    with pytest.raises(ValueError, match="cycle 7 has not been scored"):
        stacked.cycle_weights(lik, [0, 7], by_chain=True)
    with pytest.raises(ValueError, match="nothing is collected"):
        stacked.cycle_weights(lik, [], by_chain=True)


@pytest.mark.parametrize("nst", [0, 3])
def test_reference_combine_is_mixture_evaluate_in_torch(nst):
    """mixture_evaluate's ops (bayesdll_amd/_runner.py) on one batch: with nst
    = 0 the weighted sum of the cycles' raw logits, else of logsumexp over the
    draws of log_softmax minus log nst; then the criterion's log_softmax."""
    rng = np.random.default_rng(11)
    comps, D, B, Cn = 3, max(1, nst), 6, 7
    x = (3.0 * rng.standard_normal((comps * D, 1, B, Cn))).astype(np.float32)
    w = np.array([[0.5], [0.0], [0.5]]) if nst else np.array([[0.2], [0.3], [0.5]])
    batch_logits = None
    for c in range(comps):
        if w[c, 0] < 1e-10:
            continue
        comp = torch.stack([torch.from_numpy(x[c * D + s, 0]).double() for s in range(D)], dim=2)
        comp_out = comp.squeeze(2) if nst == 0 else \
            F.log_softmax(comp, dim=1).logsumexp(-1) - np.log(nst)
        batch_logits = w[c, 0] * comp_out if batch_logits is None else \
            batch_logits + w[c, 0] * comp_out
    want = F.log_softmax(batch_logits, dim=1).numpy()
    r = R.mixture_reference(x, w, D, "reference")
    assert np.allclose(r["logp"][0], want, rtol=0, atol=1e-12)
    # and the arithmetic mode is the log of the weighted mean probability
    p = torch.softmax(torch.from_numpy(x).double(), -1).numpy().reshape(comps, D, 1, B, Cn).mean(1)
    ra = R.mixture_reference(x, w, D, "arithmetic")
    assert np.allclose(ra["logp"], np.log((w[:, :, None, None] * p).sum(0)), rtol=0, atol=1e-12)
    H = -(torch.softmax(torch.from_numpy(x).double(), -1)
          * torch.log_softmax(torch.from_numpy(x).double(), -1)).sum(-1).numpy()
    ee = (w[:, :, None] * H.reshape(comps, D, 1, B).mean(1)).sum(0)
    assert np.allclose(ra["expected_entropy"], ee, rtol=0, atol=1e-12)


def test_score_reference_is_cross_entropy():
    x, lab, _, sr, _ = R.built(R.CASES[4])
    M, G, B, Cn = x.shape
    ok = sr["ok"]
    for i in range(M):
        for g in range(G):
            rows = np.nonzero(ok[i, g])[0]
            ce = F.cross_entropy(torch.from_numpy(x[i, g][rows]).double(),
                                 torch.from_numpy(lab[rows]), reduction="sum").item()
            assert abs(sr["nll_sum"][i, g] - ce) < 1e-9
            assert sr["n"][i, g] == len(rows)
    assert (sr["n_nonfinite"].sum(0) == 3).all()   # examples 5, 6, 7: one member each
    assert (sr["n"] + sr["n_nonfinite"] == B - 2).all()  # two labels out of range


# ------------------------- 4. the emulation within the bound, the cap, the inputs
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_emulation_of_the_contracts_is_within_the_bound(case):
    x, lab, w, sr, mr = R.built(case)
    R.check_scores(R.score_emulate(x, lab), sr, R.case_id(case))
    for combine in R.COMBINES:
        R.check_mixture(R.mixture_emulate(x, w, case[3], combine), mr[combine],
                        (R.case_id(case), combine))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_excluded_share_and_input_conditions_of_the_gpu_cases(case):
    """At most 1 % of a case's logp entries have no bound; no member row's
    maximum is attained twice except in the planted tie (example 2) and the
    all -inf row; the planted examples are what the builder says."""
    x, lab, w, sr, mr = R.built(case)
    Cn, B, comps, D, G, _ = case
    assert x.size < 10 ** 6
    for combine in R.COMBINES:
        assert R.excluded_share(mr[combine]) <= R.MAX_EXCLUDED, combine
    assert np.allclose(w.sum(0), 1.0) and ((w >= 0.01) | (w == 0)).all()
    with np.errstate(invalid="ignore"):
        mx = np.nanmax(np.where(np.isnan(x), -np.inf, x), -1, keepdims=True)
        ties = (x == mx).sum(-1) > 1
    allowed = np.zeros(ties.shape, bool)
    if B >= 5 and Cn > 1:
        allowed[:, :, 2] = True
    if B >= 9 and Cn > 1:
        allowed[comps * D - 1, :, 7] = True
    assert np.array_equal(ties, allowed)
    if B >= 9:
        bad = mr["arithmetic"]["nonfinite"]
        skipped = comps == 3      # the last group's middle component holds example 5's NaN
        assert bad[:, 6:8].all() and bad[:G - 1, 5].all() and bad[G - 1, 5] == (not skipped)
        assert bad.sum() == 3 * G - skipped


# ------------------------------------------------- 5. the samplers, without a device
def _bare(cls_name, per_chain=None):
    from bayesdll_amd import stacked
    S = object.__new__(getattr(stacked, cls_name))
    S.K, S.per_chain, S.nst = 2, per_chain, 0
    S.args = type("A", (), {"device": torch.device("cpu"), "ece_num_bins": 15})()
    S.mom1 = {0: None, 1: None}
    S.cycle_likelihoods = {0: np.full((1, 2), 0.5), 1: np.full((1, 2), 0.25)}
    return S


def test_sampler_refusals(monkeypatch):
    from bayesdll_amd import chains, stacked
    for call in (lambda S: S.evaluate([], weights="gmm"),
                 lambda S: S.evaluate_chains([], weights="gmm"),
                 lambda S: S.uncertainty([], weights="gmm"),
                 lambda S: S.fit_temperature([], weights="gmm"),
                 lambda S: S.score_cycle([]),
                 lambda S: S.component_weights()):
        with pytest.raises(ValueError, match="StackedSGLD is not cyclical"):
            call(_bare("StackedSGLD"))
    args = type("A", (), {"gmm_weights": True, "hparams": {}})()
    with pytest.raises(ValueError, match="gmm_weights weighs the cycles of a cyclical sampler"):
        stacked.StackedSGHMC(torch.nn.Linear(2, 2), 2, args)
    S = _bare("StackedCSGLD", per_chain={"lr": np.ones(2)})
    with pytest.raises(ValueError, match="different models"):
        S.evaluate([], weights="gmm")
    with pytest.raises(ValueError, match="different models"):
        S.uncertainty([], weights="gmm")
    S = _bare("StackedCSGHMC")
    with pytest.raises(ValueError, match='combine="reference" is one Runner\'s rule'):
        S.evaluate([], weights="gmm", combine="reference")
    with pytest.raises(ValueError, match='combine="reference" is one Runner\'s rule'):
        S.fit_temperature([], weights="gmm", combine="reference")
    with pytest.raises(ValueError, match="combine from"):
        S.evaluate_chains([], weights="gmm", combine="geometric")
    with pytest.raises(ValueError, match='None \\(uniform\\) or "gmm"'):
        S.evaluate([], weights="uniform")
    with pytest.raises(ValueError, match="no per_example, no temperature"):
        S.uncertainty([], weights="gmm", per_example=True)
    S.cycle_likelihoods = {0: np.full((1, 2), 0.5)}
    with pytest.raises(ValueError, match="cycle 1 has not been scored"):
        S.evaluate_chains([], weights="gmm")
    assert np.array_equal(_bare("StackedAdamCSGHMC").component_weights(),
                          [[2 / 3, 2 / 3], [1 / 3, 1 / 3]])
    monkeypatch.setattr(chains, "world", lambda: 2)
    with pytest.raises(ValueError, match="this process's chains only, and 2 processes"):
        _bare("StackedCSGHMC").evaluate_chains([], weights="gmm")
    with pytest.raises(ValueError, match="this process's chains only, and 2 processes"):
        _bare("StackedCSGHMC").evaluate([], weights="gmm")


def test_cycle_likelihoods_are_checkpointed_only_with_the_option():
    S = _bare("StackedCSGHMC")
    assert S._gmm_state() == {}                    # the option is off: nothing is added
    S.gmm_weights = True
    d = S._gmm_state()
    assert sorted(d) == ["cycle_likelihoods"] and sorted(d["cycle_likelihoods"]) == [0, 1]
    assert d["cycle_likelihoods"][1].dtype == torch.float64
    T = _bare("StackedCSGHMC")
    T._load_gmm_state(d)
    assert all(np.array_equal(T.cycle_likelihoods[c], S.cycle_likelihoods[c]) for c in (0, 1))
    T._load_gmm_state({})                          # a checkpoint without it loads
    assert T.cycle_likelihoods == {}
