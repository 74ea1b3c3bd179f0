"""The function-space fold (include/bdl_fn.h) without a GPU: the header, the C
struct layout against the ctypes mirror, the export and its Makefile
registration, every validation error of bdl_fn_fold (fake pointers: each call
returns before any HIP call), kernels.fn_fold's argument building, the stacked
samplers' refusals on host-only fakes, the command line, a NumPy emulation of
the arithmetic contract inside the derived bound, the input conditions of the
GPU cases, and the proof that the GPU case table reaches every path of the
kernel's geometry (tests/fn_fold_ref.py restates it)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import chain_diag_ref as D
import chain_ess_ref as E
import fn_fold_ref as R
from test_chain_diag_host import Net, _args, host_only  # noqa: F401  (host_only: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NULL, ALIGN, ARG = -1, -2, -3
FIELDS = ["logits", "bsum", "smean", "sM2", "bM2", "probs", "probe", "chain_groups", "sample",
          "batch", "chains", "classes", "flags", "fs", "fb", "c", "grid_blocks", "pad0"]


# ------------------------------------------------- header, ctypes, exports
def test_header_declares_the_function_and_states_the_contract():
    src = open(os.path.join(INCLUDE, "bdl_fn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.findall(r"\b(bdl_\w+)\s*\(", code) == ["bdl_fn_fold"]
    assert "BDL_ABI_VERSION" not in code and '#include "bdl_ess.h"' in code
    flat = " ".join(src.split())
    for word in ("Arithmetic contract", "expf", "1 ulp", "in fp64", "No atomics", "masked class",
                 "BDL_FN_WAVE_CLASSES", "BDL_FN_MAX_CLASSES", "neither read nor written",
                 "bit-identical for every grid_blocks", "FIRST_SAMPLE", "n_nonfinite"):
        assert word in flat, word


def test_ctypes_mirror_matches_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    lines = ['printf("size %zu\\n", sizeof(bdl_fn_fold_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(bdl_fn_fold_args, {f}));' for f in FIELDS]
    lines.append('printf("limits %d %d %d\\n", BDL_FN_MAX_CLASSES, BDL_FN_WAVE_CLASSES, '
                 'BDL_FN_MAX_GRID);')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_fn.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    lay = dict(ln.split(" ", 1) for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(lay["size"]) == C.sizeof(L.FnFoldArgs) == 112
    assert [f for f, _ in L.FnFoldArgs._fields_] == FIELDS
    for f in FIELDS:
        assert getattr(L.FnFoldArgs, f).offset == int(lay[f]), f
    assert lay["limits"] == f"{L.FN_MAX_CLASSES} {L.FN_WAVE_CLASSES} {L.FN_MAX_GRID}" \
        == "8192 256 2048"
    assert (R.MAX_CLASSES, R.WAVE_CLASSES) == (L.FN_MAX_CLASSES, L.FN_WAVE_CLASSES)


def test_library_exports_the_unit_next_to_the_pinned_abi():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert sorted(L.FN_EXPORTS) == ["bdl_fn_fold"]
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS, L.CHAIN_STEP_EXPORTS,
                  L.STATS_EXPORTS, L.ESS_EXPORTS, L.LOWP_EXPORTS, L.LAYERS_EXPORTS,
                  L.PREDICT_EXPORTS):
        assert not set(L.FN_EXPORTS) & set(other)
    assert hasattr(h, "bdl_fn_fold") and h.bdl_fn_fold.argtypes is not None
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_fn" in mk.split("TUS :=")[1].split("DEPS")[0].split()
    assert "include/bdl_fn.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    assert "bdl_fn.hip" in mk.split("ROCM ?=")[0]                  # the header comment
    assert "-ffp-contract=off" in mk.split("CFLAGS :=")[1].splitlines()[0]
    assert "TUFLAGS_bdl_fn" not in mk


# ---------------------------------------------------------------- validation
def _good():
    """K = 3, P = 5, C = 8, slot 48 (chain_groups 12): logits / probs 480 B, an
    accumulator 4 * (2 * 48 + 40) = 544 B.  Sample 6 of batches of 3: a later
    close (flags 4, c = 2)."""
    from bayesdll_amd import _lib as L
    a = L.FnFoldArgs()
    a.logits, a.bsum, a.smean, a.sM2, a.bM2, a.probs = (0x10000, 0x20000, 0x30000, 0x40000,
                                                        0x50000, 0x60000)
    a.probe, a.chain_groups, a.chains, a.classes = 5, 12, 3, 8
    a.sample, a.batch, a.flags, a.fs, a.fb, a.c = 6, 3, E.CLOSE, 6.0, 3.0, 2.0
    a.grid_blocks = 2
    return a


def test_entry_point_validates_before_touching_the_device():
    """Every refusal of the header's table, with its status and a message.
    No call here passes validation, so none reaches a HIP call."""
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, **fields):
        a = _good()
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_fn_fold(a, None) == status, (fields, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_fn_fold:") and word in msg, (fields, msg)

    assert h.bdl_fn_fold(None, None) == NULL and b"null args" in h.bdl_last_error()
    refused(NULL, b"null logits", logits=None)
    for f in ("smean", "sM2", "bM2"):
        refused(NULL, b"smean, sM2 and bM2 are required", **{f: None})
    refused(NULL, b"bsum is required with batch > 1", bsum=None)
    for f in ("logits", "bsum", "smean", "sM2", "bM2", "probs"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x700008})
    refused(ARG, b"chains", chains=0)
    refused(ARG, b"chains", chains=65536)
    refused(ARG, b"probe", probe=0)
    refused(ARG, b"classes", classes=0)
    refused(ARG, b"classes", classes=8193)
    refused(ARG, b"grid_blocks", grid_blocks=-1)
    refused(ARG, b"grid_blocks", grid_blocks=2049)
    refused(ARG, b"chains * probe * classes overflows", probe=1 << 58)
    refused(ARG, b"chains * chain_groups overflows", chain_groups=1 << 62)
    refused(ARG, b"n exceeds the chain slot", chain_groups=9)       # 36 < 40
    refused(ARG, b"n exceeds the chain slot", probe=7)              # 56 > 48
    refused(ARG, b"batch must be in", batch=0)
    refused(ARG, b"batch must be in", batch=1 << 24)
    refused(ARG, b"sample must be in", sample=0)
    refused(ARG, b"sample must be in", sample=1 << 24)
    refused(ARG, b"flags 0 are not what sample 6 of batch 3 implies (4)", flags=0)
    refused(ARG, b"flags", sample=5)                                # flags 4 given, 0 implied
    refused(ARG, b"fs / fb", fs=5.0)
    refused(ARG, b"fs / fb", fb=2.0)
    refused(ARG, b"c is not fl32(i/(i-1))", c=1.5)
    # every pair of spans
    refused(ARG, b"probs overlaps logits", probs=0x10000 + 464)
    refused(ARG, b"bsum overlaps logits", bsum=0x10000 - 528)
    refused(ARG, b"smean overlaps probs", smean=0x60000 + 464)
    refused(ARG, b"sM2 overlaps bsum", sM2=0x20000 + 528)
    refused(ARG, b"bM2 overlaps smean", bM2=0x30000 - 528)
    refused(ARG, b"bM2 overlaps sM2", bM2=0x40000 + 16)
    # the nullable vectors are nullable: probs always, bsum at batch == 1 (where an
    # overlapping or misaligned bsum is not looked at either)
    for extra in ({"probs": None}, {"batch": 1, "flags": 6, "fb": 1.0, "c": 6 / 5, "bsum": None},
                  {"batch": 1, "flags": 6, "fb": 1.0, "c": 6 / 5, "bsum": 0x30008}):
        refused(ARG, b"grid_blocks", grid_blocks=2049, **extra)


def test_entry_point_refuses_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_fn_fold(_good(), None) == ARG
        assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_fn_fold(None, None) == NULL


# ------------------------------------------------------ kernels.fn_fold
def test_kernels_layer_builds_the_arguments_and_checks_them(monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    sent = []

    class FakeLib:
        @staticmethod
        def bdl_fn_fold(a, stream):
            sent.append({f: getattr(a, f) for f in FIELDS})
            return 0

    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    monkeypatch.setattr(L, "lib", lambda: FakeLib)
    monkeypatch.setattr(L, "current_stream_handle", lambda dev=None: None)
    x = torch.zeros(3, 5, 8)
    cg = 12
    v = {nm: torch.zeros(3 * 4 * cg) for nm in E.VECTORS}
    probs = torch.zeros(3, 5, 8)
    for s in range(1, 12):
        for b in (1, 3, 4):
            flags = K.fn_fold(x, v["bsum"], v["smean"], v["sM2"], v["bM2"], sample=s, batch=b,
                              chain_groups=cg, probs=probs, grid_blocks=5)
            want, fs, fb, c = E.fold_plan(s, b)
            a = sent[-1]
            assert flags == want == a["flags"]
            assert (a["chains"], a["probe"], a["classes"], a["chain_groups"]) == (3, 5, 8, cg)
            assert (a["sample"], a["batch"], a["grid_blocks"]) == (s, b, 5)
            assert np.float32(a["fs"]) == fs and np.float32(a["fb"]) == fb
            if c is not None:
                assert np.float32(a["c"]) == c                     # fl32 of the float64 quotient
            assert a["logits"] == x.data_ptr() and a["probs"] == probs.data_ptr()
            assert a["bsum"] == (v["bsum"].data_ptr() if b > 1 else None)
            assert (a["smean"], a["sM2"], a["bM2"]) == tuple(
                v[nm].data_ptr() for nm in ("smean", "sM2", "bM2"))
    K.fn_fold(x, None, v["smean"], v["sM2"], v["bM2"], sample=2, batch=1, chain_groups=cg)
    assert sent[-1]["bsum"] is None and sent[-1]["probs"] is None and sent[-1]["grid_blocks"] == 0
    n = len(sent)
    kw = dict(sample=2, batch=3, chain_groups=cg)
    with pytest.raises(ValueError, match="bsum is required"):
        K.fn_fold(x, None, v["smean"], v["sM2"], v["bM2"], **kw)
    with pytest.raises(ValueError, match=r"\[chains, probe, classes\]"):
        K.fn_fold(x[0], v["bsum"], v["smean"], v["sM2"], v["bM2"], **kw)
    with pytest.raises(ValueError, match="contiguous"):
        K.fn_fold(x.transpose(1, 2), v["bsum"], v["smean"], v["sM2"], v["bM2"], **kw)
    with pytest.raises(ValueError, match="classes"):
        K.fn_fold(torch.zeros(1, 1, 8193), v["bsum"], v["smean"], v["sM2"], v["bM2"], sample=2,
                  batch=3, chain_groups=4096)
    with pytest.raises(ValueError, match="grid_blocks"):
        K.fn_fold(x, v["bsum"], v["smean"], v["sM2"], v["bM2"], grid_blocks=2049, **kw)
    with pytest.raises(ValueError, match="4 \\* chain_groups"):
        K.fn_fold(x, v["bsum"], v["smean"], v["sM2"], v["bM2"], sample=2, batch=3, chain_groups=9)
    with pytest.raises(ValueError, match="at least"):
        K.fn_fold(x, v["bsum"], v["smean"][:100], v["sM2"], v["bM2"], **kw)
    with pytest.raises(ValueError, match="probs"):
        K.fn_fold(x, v["bsum"], v["smean"], v["sM2"], v["bM2"], probs=torch.zeros(3, 5, 4), **kw)
    with pytest.raises(ValueError, match="batch must be in"):
        K.fn_fold(x, v["bsum"], v["smean"], v["sM2"], v["bM2"], sample=2, batch=0,
                  chain_groups=cg)
    assert len(sent) == n                                          # none of them launched


# ------------------------------------------------------- sampler refusals
def test_sampler_refusals_before_touching_a_device(host_only, monkeypatch):
    from bayesdll_amd import chains, stacked
    probe = torch.zeros(5, 13)
    with pytest.raises(ValueError, match="fn_probe needs fn_batch = b >= 1"):
        stacked.StackedSGLD(Net(), 2, _args(), fn_probe=probe)
    with pytest.raises(ValueError, match="needs a probe batch"):
        stacked.StackedSGLD(Net(), 2, _args(), fn_batch=2)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="fn_batch must be an integer >= 0"):
            stacked.StackedSGLD(Net(), 2, _args(), fn_probe=probe, fn_batch=bad)
    with pytest.raises(ValueError, match="non-empty input batch"):
        stacked.StackedSGLD(Net(), 2, _args(), fn_probe=torch.zeros(0, 13), fn_batch=2)
    S0 = stacked.StackedSGLD(Net(), 2, _args())
    assert S0._fn_probe is None and S0._fn is None and S0.fn_batch == 0
    with pytest.raises(ValueError, match="built without fn_probe"):
        S0.function_space()
    S0.function_space_reset()                                      # nothing to empty: no error
    S = stacked.StackedCSGHMC(Net(), 3, _args(), fn_probe=probe, fn_batch=4)
    assert S.fn_batch == 4 and S._fn is None                       # nothing allocated yet
    assert S._fn_probe.shape == (5, 13)
    with pytest.raises(ValueError, match="function_space: ess: nothing is folded yet"):
        S.function_space()
    with pytest.raises(ValueError, match="three finite"):
        S.function_space(thresholds=(1, 2))
    with pytest.raises(ValueError, match="three R-hat thresholds"):
        S.function_space(rhat_thresholds=(1.1,))
    # counted, but too few: one sample (R-hat needs 2), then fewer than two closed batches
    S._fn = {"acc": {}, "samples": 1, "chain_groups": 7, "probe": 5, "classes": 5}
    with pytest.raises(ValueError, match="1 sample folded per chain close 0 batches of 4"):
        S.function_space()
    S._fn["samples"] = 7
    with pytest.raises(ValueError, match="7 samples folded per chain close 1 batch of 4"):
        S.function_space()
    S.function_space_reset()
    assert S._fn["samples"] == 0
    # K = 1: R-hat is refused, the ESS part alone would be returned
    S1 = stacked.StackedSGLD(Net(), 1, _args(), fn_probe=probe, fn_batch=2)
    with pytest.raises(ValueError, match="R-hat compares chains; this sampler runs K = 1"):
        S1.function_space(rhat=True)
    with pytest.raises(ValueError, match="nothing is folded yet"):
        S1.function_space()
    # per_chain: R-hat refused, ESS by_chain only
    SP = stacked.StackedCSGHMC(Net(), 3, _args(), fn_probe=probe, fn_batch=4,
                               per_chain={"lr": [1e-2, 2e-2, 3e-2]})
    with pytest.raises(ValueError, match="per_chain hyperparameters.*different ones.*by_chain"):
        SP.function_space()
    with pytest.raises(ValueError, match="per_chain hyperparameters; R-hat compares chains"):
        SP.function_space(rhat=True, by_chain=True)
    with pytest.raises(ValueError, match="nothing is folded yet"):
        SP.function_space(by_chain=True)
    # the accumulators are no part of the checkpointed state
    assert not any("fn" in k for k in S.state_dict())
    # several processes: refused, as uncertainty() refuses them
    monkeypatch.setattr(chains, "world", lambda: 2)
    with pytest.raises(ValueError, match="this process's chains only"):
        S.function_space()


# ------------------------------------------------------------------ the CLI
def test_run_cli_fn_probe_needs_stacked_chains_and_a_batch(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    d = ap.parse_args([])
    assert (d.fn_probe, d.fn_batch) == (0, 0) and run.check_fn(ap, d) == (0, 0)
    a = ap.parse_args(["--stacked_chains", "4", "--fn_probe", "16", "--fn_batch", "2"])
    assert run.check_fn(ap, a) == (16, 2)
    for argv, word in ((["--fn_probe", "16", "--fn_batch", "2"], "it needs --stacked_chains >= 1"),
                       (["--fn_probe", "16", "--stacked_chains", "2"], "needs --fn_batch B >= 1"),
                       (["--fn_batch", "2", "--stacked_chains", "2"], "it needs --fn_probe P"),
                       (["--fn_probe", "-1", "--stacked_chains", "2"], "must be >= 0")):
        with pytest.raises(SystemExit) as e:
            run.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    loader = [(torch.arange(8.).view(4, 2), None), (torch.arange(8., 16.).view(4, 2), None)]
    assert torch.equal(run.first_examples(loader, 6), torch.arange(12.).view(6, 2))
    with pytest.raises(ValueError, match="holds only 8 examples"):
        run.first_examples(loader, 9)


# --------------------------------------- the contract, emulated, is in the bound
def emulate(x):
    """The header's arithmetic contract step by step in NumPy (np.exp on fp32
    stands in for expf: within its ulp bound of the true value, not bit-equal
    to the device's)."""
    x = np.asarray(x, dtype=np.float32)
    bad = R.bad_rows(x)
    with np.errstate(all="ignore"):
        m = np.where(bad[..., None], np.float32(0), x).max(-1, keepdims=True)
        d = (x - m).astype(np.float32)
        e = np.exp(d).astype(np.float32)
        Z = e.astype(np.float64).sum(-1, keepdims=True)
        p = (e.astype(np.float64) * (1.0 / Z)).astype(np.float32)
    return np.where(bad[..., None], np.float32("nan"), p)


@pytest.mark.parametrize("case", R.CASES + [(10, 9, 2), (1027, 9, 2)], ids=R.case_id)
def test_emulation_of_the_contract_is_within_the_bound(case):
    special = case not in R.CASES
    for x, p64, b in R.built(case, special):
        got = emulate(x).astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(p64))
        ok = ~np.isnan(p64)
        assert (np.abs(got[ok] - p64[ok]) <= b[ok]).all()
        rows = ~R.bad_rows(x)
        assert np.allclose(p64[rows].sum(-1), 1.0, rtol=0, atol=1e-12)
    if special:
        C = case[0]
        x1, p1, _ = R.built(case, True)[1]
        assert (R.built(case, True)[0][1][:, 3, C // 2] == 0).all()      # masked: p = 0
        assert np.allclose(p1[0, 1], 1.0 / C, rtol=1e-15) and p1[0, 2, C - 1] < 1e-90
        p2 = R.built(case, True)[2][1]
        assert np.isnan(p2[0, 5]).all() and np.isnan(p2[1, 6]).all() and np.isnan(p2[0, 7]).all()
        assert np.isnan(p2).sum() == 3 * C


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_input_conditions_of_the_ordinary_gpu_cases(case):
    """By the reference alone (the fold of the fp32-rounded float64 softmax): no
    degenerate and no non-finite element in either report, so the GPU test's
    counts say something — except at classes = 1, where p = 1 everywhere."""
    C, P, K_ = case
    cg, n = R.chain_groups_of(case), C * P
    acc = R.new_acc(case)
    for i in range(R.FOLDS):
        R.fold(acc, R.built(case)[i][1].astype(np.float32), i + 1, R.B_LONG, chain_groups=cg)
    S_, nb = R.FOLDS, R.FOLDS // R.B_LONG
    summ = E.chain_ess_f32(acc["sM2"], acc["bM2"], chains=K_, chain_groups=cg, n=n, samples=S_,
                           batches=nb)[2]
    want = (0, n, 0) if C == 1 else (n, 0, 0)
    assert (summ["n_eval"], summ["n_degenerate"], summ["n_nonfinite"]) == want
    if K_ >= 2:
        rs = D.chain_diag_f32(acc["smean"], acc["sM2"], chains=K_, chain_groups=cg, n=n,
                              var_mode=D.VAR_WELFORD, ratio=float(S_ - 1),
                              inv_ratio=D.inv_of(S_ - 1), count=S_)[3]
        assert (rs["n_eval"], rs["n_degenerate"], rs["n_nonfinite"]) == want
    slot = 4 * cg
    for nm in E.VECTORS:                                           # the padding keeps the sentinel
        for k in range(K_):
            assert (acc[nm][slot * k + n: slot * (k + 1)] == np.float32(R.SENTINEL)).all()


# ----------------------------------------- the case table reaches every path
def test_case_table_reaches_every_path_of_the_geometry():
    reached = {}
    for case in R.CASES:
        Cn, P, K_ = case
        for grid in R.GRIDS:
            got, writes = R.paths(K_, P, Cn, grid)
            assert (writes == 1).all(), (case, grid)               # one thread per element
            reached.setdefault(Cn, set()).update(got)
    assert set(reached) == set(R.CLASSES)
    assert {c for c in R.CLASSES if "wave" in reached[c]} == {1, 3, 10, 12, 256}
    assert {c for c in R.CLASSES if "block" in reached[c]} == {257, 260, 1000, 1027, 2052}
    assert {c for c in R.CLASSES if "vec" in reached[c]} == {12, 256, 260, 1000, 2052}
    # wave path: both access forms, idle lanes and a full wave, idle waves, a second
    # row trip, the partial last group
    assert {"elem", "idle_lane", "partial_group", "row_trip2", "idle_wave"} <= reached[3]
    assert {"elem", "partial_group"} <= reached[10] and {"vec", "idle_lane"} <= reached[12]
    assert "idle_lane" not in reached[256] and "row_trip2" in reached[256]
    assert "idle_wave" in reached[1] and "idle_wave" in reached[256]
    # block path: one past the switch in the element form; the vector form with fewer
    # groups than threads; a thread's second trip in both forms; a second row trip
    assert {"elem", "partial_group", "fewer_groups_than_threads", "row_trip2"} <= reached[257]
    assert "thread_trip2" not in reached[257]
    assert {"vec", "fewer_groups_than_threads"} <= reached[260]
    assert {"vec", "fewer_groups_than_threads", "row_trip2"} <= reached[1000]
    assert {"elem", "thread_trip2", "partial_group", "idle_thread", "row_trip2"} <= reached[1027]
    assert {"vec", "thread_trip2", "idle_thread", "row_trip2"} <= reached[2052]
    assert "partial_group" not in reached[2052] and "partial_group" not in reached[12]
    # the switch itself and the cap
    assert "wave" in R.paths(1, 1, R.WAVE_CLASSES, 0)[0]
    assert "block" in R.paths(1, 1, R.WAVE_CLASSES + 1, 0)[0]
    assert (R.paths(1, 1, R.MAX_CLASSES, 1)[1] == 1).all()
    # grid 1 and 2 take second row trips, the default grid none at these sizes
    for case in R.CASES:
        Cn, P, K_ = case
        assert "row_trip2" not in R.paths(K_, P, Cn, 0)[0], case
    assert "row_trip2" in R.paths(3, 9, 10, 2)[0] and "row_trip2" in R.paths(3, 5, 257, 2)[0]
