"""Temperature scaling of the stacked predictive without a GPU
(include/bdl_temper.h): the fp64 reference (tests/temper_ref.py) against the
reference project's recorded temperatures and against calibration.py, the
emulation of the header's arithmetic contract within the derived bound, the
safeguards of the Newton update, the ctypes mirrors, every validation error
(the library loads without a GPU; none of these calls launches anything), the
Python wrappers', the samplers' and the command line's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import temper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "calibration.npz"))
NULL, ALIGN, ARG = -1, -2, -3
# (N, C, seed, sharp): rows of the class counts the GPU test uses (both paths, both sides of
# the boundary, C % 4 != 0 on each, the limit) — NOT its inputs: those are
# test_gpu_temper._group_rows(SHAPES), held below in test_gpu_shapes_reach_a_decided_state
FIT_CASES = [(11, 10, 2, 0.6), (11, 37, 2, 0.5), (11, 256, 3, 1.5), (11, 257, 4, 0.7),
             (11, 1000, 5, 1.3), (3, 8192, 6, 0.8)]


# ------------------------------------------- 1. the reference against the recorded fits
@pytest.mark.parametrize("name", ["c10", "c37"])
def test_reference_fit_lands_on_the_recorded_temperature(name):
    """scipy BFGS stops at |dF/dT| <= gtol = 1e-5: within 1e-5 / (d2F/dT2) of
    the optimum.  Observed: c10 2.1e-5 of 2.1e-4, c37 6.8e-6 of 1.5e-5."""
    z, lab = GOLD[name + "_vlogits"], GOLD[name + "_vlabels"]
    fit = R.fit_reference(z, lab, rtol=1e-10)
    assert fit["converged"] and fit["iterations"] <= 6
    curv = R.curvature_T(z, lab, fit["temperature"])
    diff = abs(fit["temperature"] - float(GOLD[name + "_topt"][0]))
    print(name, fit["temperature"], diff, 1e-5 / curv, curv)
    assert curv > 0 and diff <= 1e-5 / curv
    # the emulation of the device's fit: converged, within its own bound of the fp64 fit
    em = R.newton(z, lab)
    assert em["converged"] and not em["at_bound"] and not em["degenerate"] and em["margin"] > 1
    assert abs(em["temperature"] - fit["temperature"]) <= R.bound_T(z, lab, em, 1e-6)
    assert em["nll"] <= em["nll_first"]


# --------------------------------------- 2. the report against calibration.analyze / nll
def _report_inputs():
    yield "c10", GOLD["c10_logits"], GOLD["c10_labels"]
    yield "c37", GOLD["c37_logits"], GOLD["c37_labels"]
    for N, Cn, seed in ((40, 10, 11), (23, 37, 12), (9, 300, 13)):
        z, lab = R.make_rows(N, Cn, seed)
        yield f"rows{Cn}", z, lab


@pytest.mark.parametrize("name,z,lab", list(_report_inputs()), ids=lambda v: v if isinstance(v, str) else "")
def test_reference_report_agrees_with_calibration(name, z, lab):
    from bayesdll_amd import calibration
    tfit = R.newton(z, lab)["temperature"]
    for T in (1.0, 1.7, tfit):
        beta = np.float32(1.0 / T)
        r, em = R.report_reference(z, lab, beta), R.report_emulate(z, lab, beta)
        assert R.margins(r) > 1, (name, T, R.margins(r))  # every element, none excused
        s, se, sb = R.summary(r), R.summary(em), R.summary_bound(r)
        ece, mce, nll = calibration.analyze(lab, z.astype(np.float64), 15,
                                            temperature=1.0 / float(beta))
        assert abs(s["ece"] - ece) < 1e-12 and abs(s["mce"] - mce) < 1e-12 and abs(s["nll"] - nll) < 1e-10
        sizes = calibration.calc_bins(lab, z.astype(np.float64), 15, 1.0 / float(beta))[4]
        assert np.array_equal(r["bin_count"][:15], sizes.astype(np.int64))
        # the emulation of the contract: integers and bins equal, sums within the bound
        for k in ("n", "n_labelled", "n_nonfinite", "n_wrong"):
            assert em[k] == r[k], (name, T, k)
        assert np.array_equal(em["bin_count"], r["bin_count"])
        assert np.array_equal(em["bin_hits"], r["bin_hits"])
        for k in ("nll_sum", "entropy_sum", "confidence_sum"):
            assert abs(em[k] - r[k]) <= r["b_" + k], (name, T, k, abs(em[k] - r[k]), r["b_" + k])
        assert (np.abs(em["bin_conf"] - r["bin_conf"]) <= r["b_bin_conf"]).all()
        for k in ("nll", "ece", "mce"):
            assert abs(se[k] - s[k]) <= sb[k], (name, T, k)
    if name in ("c10", "c37"):   # the recorded analyze() of the reference project
        for T in (1.0, 1.7):
            # (fl32(1 / 1.7) is not 1 / 1.7: u x |dNLL/dbeta| x beta, far inside 1e-6)
            s = R.summary(R.report_reference(z, lab, np.float32(1.0 / T)))
            want = GOLD[f"{name}_analyze_T{T}"]
            assert abs(s["ece"] - want[0]) < 1e-6 and abs(s["mce"] - want[1]) < 1e-6
            assert abs(s["nll"] - want[2]) < 1e-6


# ------------------------------------------------- 3. the emulated fit, the safeguards
@pytest.mark.parametrize("case", FIT_CASES, ids=lambda c: "N{}-C{}".format(*c[:2]))
def test_emulated_fit_is_within_the_bound_of_the_fp64_fit(case):
    N, Cn, seed, sharp = case
    z, lab = R.make_rows(N, Cn, seed, sharp=sharp, special=True)
    em, fr = R.newton(z, lab), R.fit_reference(z, lab, rtol=1e-10)
    assert em["converged"] and fr["converged"] and not em["at_bound"] and not em["degenerate"]
    assert abs(em["temperature"] - fr["temperature"]) <= R.bound_T(z, lab, em, 1e-6)
    s, e = R.sweep_reference(z, lab, 1.0), R._emulated_sweep(z, lab, 1.0)
    for k, b in (("nll", "b_nll"), ("d1", "b_d1"), ("d2", "b_d2")):
        assert abs(e[k] - s[k]) <= s[b], (k, abs(e[k] - s[k]), s[b])
    if N >= 8:   # the special rows: counted where the header says, nothing else moves
        assert (em["n"], em["n_nonfinite"], em["n_inf_label"]) == (N - 6, 3, 1)
        keep = np.r_[0, 1, 8:N]
        z2 = z[keep].copy()
        sub = R.newton(z2, lab[keep])
        assert sub["temperature"] == em["temperature"] and sub["nll"] == em["nll"]
        # a masked class contributes zero: the same as a class at -1e30
        z3 = z2.copy()
        z3[np.isneginf(z3)] = -1e30
        assert R._emulated_sweep(z3, lab[keep], 1.0)["d1"] == R._emulated_sweep(z2, lab[keep], 1.0)["d1"]


def test_gpu_shapes_reach_a_decided_state():
    """Every group of every shape of the GPU test ends converged, on a limit
    or degenerate in the emulation, so that its flag checks are live; the
    single-example shapes (label = the row's least likely class: the optimum
    is T -> inf) end on the lower limit of beta, done and not converged."""
    import test_gpu_temper as G
    undecided = []
    for shape in G.SHAPES:
        C, N, Gn, _ = shape
        z, lab = G._group_rows(C, N, Gn, special=N >= 8)
        for g in range(Gn):
            em = R.newton(z[g], lab)
            assert em["done"] or em["degenerate"], (shape, g, em)
            assert em["done"] == (em["converged"] or em["at_bound"])
            if N == 1:
                assert em["at_bound"] and em["done"] and not em["converged"] and em["beta"] == R.BETA_MIN
                assert em["iterations"] == 4 and em["margin"] > 1      # 1/4, 1/16, 1/64, 0.01
            if em["margin"] <= 1:
                undecided.append((shape, g))
    # the one group whose convergence decision is within the bound of its threshold: the GPU
    # test compares its temperature, not its flags
    assert undecided == [((10, 5, 3, 2), 2)]


def test_safeguards_of_the_update():
    rng = np.random.default_rng(5)
    # every label the argmax by a wide margin: the NLL falls for ever as beta grows
    # (wide against the rows' spread, small enough that exp(-100 x margin) is not 0 in fp32)
    z = (0.01 * rng.standard_normal((12, 7))).astype(np.float32)
    lab = z.argmax(-1)
    z[np.arange(12), lab] += np.float32(0.3)
    em = R.newton(z, lab)
    assert em["at_bound"] and em["done"] and not em["converged"] and not em["degenerate"]
    assert em["beta"] == R.BETA_MAX and 4 <= em["iterations"] <= 31   # at best 4, 16, 64, 100
    assert em["sweeps"] == em["iterations"] + 1      # one more sweep finds the step beyond the limit
    # ... and wrong everywhere: to the lower limit
    em = R.newton(z, (lab + 1) % 7)
    assert em["at_bound"] and not em["converged"] and em["beta"] == R.BETA_MIN
    # constant rows: no curvature
    em = R.newton(np.full((5, 6), 0.75, np.float32), np.arange(5))
    assert em["degenerate"] and not em["converged"] and em["beta"] == 1.0 and em["iterations"] == 0
    assert not em["done"]
    assert em["d2"] == 0.0 and abs(em["nll"] - np.log(6)) < 1e-6
    # no labelled example
    em = R.newton(z, np.full(12, -1))
    assert em["degenerate"] and em["n"] == 0 and np.isnan(em["nll"])
    # the step is clamped to [beta / 4, 4 beta]
    z, lab = R.make_rows(30, 10, 3, sharp=0.05)
    one = R.newton(z, lab, max_iter=1)
    assert one["beta"] == 4.0 and one["iterations"] == 1 and not one["converged"]


# ------------------------------------------------------- 4. header, ctypes, exports
FIT_FIELDS = ["logp", "labels", "state", "workspace", "batch", "rtol", "groups", "classes",
              "grid_blocks", "max_iter"]
REPORT_FIELDS = ["logp", "labels", "state", "totals", "workspace", "batch", "groups", "classes",
                 "num_bins", "grid_blocks", "flags", "pad0", "edges"]
STATE_FIELDS = ["nll", "nll_first", "d1", "d2", "n", "n_nonfinite", "n_inf_label", "beta",
                "iterations", "sweeps", "converged", "at_bound", "degenerate", "done", "pad0"]
TOTALS_FIELDS = ["n", "n_labelled", "n_nonfinite", "n_wrong", "nll_sum", "entropy_sum",
                 "confidence_sum", "bin_count", "bin_hits", "bin_conf"]
FUNCS = ["bdl_temper_fit_sweep", "bdl_temper_fit_update", "bdl_temper_report",
         "bdl_temper_workspace_bytes"]


def test_header_declares_the_functions_and_states_the_contract():
    src = open(os.path.join(INCLUDE, "bdl_temper.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(re.findall(r"\b(bdl_\w+)\s*\(", code)) == FUNCS
    assert "BDL_ABI_VERSION" not in code and '#include "bdl_sgmcmc.h"' in code
    flat = " ".join(src.split())
    for word in ("Arithmetic contract", "expf", "1 ulp", "fp64", "atomics", "NON-FINITE",
                 "n_inf_label", "never 0 * inf", "BDL_TEMPER_WAVE_CLASSES", "[beta / 4, 4 beta]",
                 "done = 1, NOT converged"):
        assert word in flat, word


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    structs = (("bdl_temper_fit_args", FIT_FIELDS, L.TemperFitArgs),
               ("bdl_temper_report_args", REPORT_FIELDS, L.TemperReportArgs),
               ("bdl_temper_state", STATE_FIELDS, L.TemperState),
               ("bdl_temper_totals", TOTALS_FIELDS, L.TemperTotals))
    lines = []
    for st, fields, _ in structs:
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    lines.append('printf("limits %d %d %d %d %d %d %d %g %g\\n", BDL_TEMPER_MAX_CLASSES, '
                 'BDL_TEMPER_WAVE_CLASSES, BDL_TEMPER_MAX_BINS, BDL_TEMPER_MAX_GROUPS, '
                 'BDL_TEMPER_MAX_GRID, BDL_TEMPER_MAX_ITER, (int)BDL_TEMPER_RESET, '
                 '(double)BDL_TEMPER_MAX_T, (double)BDL_TEMPER_MIN_T);')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_temper.h\"\n"
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
    assert lay["limits"] == "8192 256 64 65535 1024 1024 1 100 0.01"
    assert (L.TEMPER_MAX_CLASSES, L.TEMPER_WAVE_CLASSES, L.TEMPER_MAX_BINS, L.TEMPER_MAX_GROUPS,
            L.TEMPER_MAX_GRID, L.TEMPER_MAX_ITER, L.TEMPER_RESET, L.TEMPER_MAX_T,
            L.TEMPER_MIN_T) == (8192, 256, 64, 65535, 1024, 1024, 1, 100.0, 0.01)
    assert np.dtype(L.TemperTotals).itemsize == C.sizeof(L.TemperTotals) == 1592
    assert np.dtype(L.TemperState).itemsize == C.sizeof(L.TemperState) == 88
    assert R.BETA_MAX == 1 / L.TEMPER_MIN_T and R.BETA_MIN == float(np.float32(1 / L.TEMPER_MAX_T))


def test_library_exports_the_unit_next_to_the_pinned_abi():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert sorted(L.TEMPER_EXPORTS) == FUNCS
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS, L.CHAIN_STEP_EXPORTS, L.STATS_EXPORTS,
                  L.ESS_EXPORTS, L.LOWP_EXPORTS, L.LAYERS_EXPORTS, L.PREDICT_EXPORTS, L.FN_EXPORTS):
        assert not set(L.TEMPER_EXPORTS) & set(other)
    for name in FUNCS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    wb = h.bdl_temper_workspace_bytes
    assert wb(1, 1) == 1592 and wb(3, 7) == 3 * 7 * 1592 and wb(2, 0) == wb(2, 1024)
    assert wb(65535, 1024) == 65535 * 1024 * 1592           # no 32-bit overflow
    for bad in ((0, 1), (-1, 1), (65536, 1), (1, -1), (1, 1025)):
        assert wb(*bad) == 0, bad
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_temper" in mk.split("TUS :=")[1].split("DEPS")[0].split()
    assert "include/bdl_temper.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    assert "bdl_temper.hip" in mk.split("ROCM ?=")[0] and "TUFLAGS_bdl_temper" not in mk


# --------------------------------------------------------------- 5. validation
def _good_fit():
    """G = 3, N = 5, C = 8: logp 480 B, labels 40 B, state 264 B, the workspace
    at grid 2 9552 B."""
    from bayesdll_amd import _lib as L
    a = L.TemperFitArgs()
    a.logp, a.labels, a.state, a.workspace = 0x10000, 0x20000, 0x30000, 0x100000
    a.batch, a.rtol, a.groups, a.classes, a.grid_blocks, a.max_iter = 5, 1e-6, 3, 8, 2, 32
    return a


def _good_report():
    from bayesdll_amd import _lib as L
    a = L.TemperReportArgs()
    a.logp, a.labels, a.state, a.totals, a.workspace = 0x10000, 0x20000, 0x30000, 0x50000, 0x100000
    a.batch, a.groups, a.classes, a.num_bins, a.grid_blocks = 5, 3, 8, 15, 2
    for i, e in enumerate(R.edges32(15)):
        a.edges[i] = float(e)
    return a


@pytest.mark.parametrize("fn", ["bdl_temper_fit_sweep", "bdl_temper_fit_update"])
def test_fit_entry_points_validate_before_touching_the_device(fn):
    from bayesdll_amd import _lib as L
    h = L.lib()
    call = getattr(h, fn)

    def refused(status, word, **fields):
        a = _good_fit()
        for k, v in fields.items():
            setattr(a, k, v)
        assert call(a, None) == status, (fields, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(fn.encode() + b":") and word in msg, (fields, msg)

    assert call(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in ("logp", "state", "workspace"):
        refused(NULL, f.encode(), **{f: None})
    for f in ("logp", "workspace"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x700008})
    for f in ("labels", "state"):
        refused(ALIGN, f.encode() + b" not 8-B aligned", **{f: 0x700004})
    refused(ARG, b"groups", groups=0)
    refused(ARG, b"groups", groups=65536)
    refused(ARG, b"batch", batch=0)
    refused(ARG, b"classes", classes=0)
    refused(ARG, b"classes", classes=8193)
    refused(ARG, b"grid_blocks", grid_blocks=-1)
    refused(ARG, b"grid_blocks", grid_blocks=1025)
    refused(ARG, b"max_iter", max_iter=0)
    refused(ARG, b"max_iter", max_iter=1025)
    refused(ARG, b"rtol", rtol=-1e-9)
    refused(ARG, b"rtol", rtol=1.0)
    refused(ARG, b"rtol", rtol=float("nan"))
    refused(ARG, b"overflows", batch=1 << 58)
    refused(ARG, b"overflows", batch=1 << 40, groups=60000, classes=8192)
    refused(ARG, b"state overlaps logp", state=0x10000 + 472)
    refused(ARG, b"state overlaps labels", state=0x20000 - 232)
    refused(ARG, b"workspace overlaps logp", workspace=0x10000 - 9552 + 16)
    refused(ARG, b"workspace overlaps state", workspace=0x30000 + 224)
    refused(ARG, b"workspace overlaps state", state=0x900000,
            workspace=0x900000 - 3 * 1024 * 1592 + 16, grid_blocks=0)
    a = _good_fit()     # labels are nullable
    a.labels, a.grid_blocks = None, 1025
    assert call(a, None) == ARG and b"grid_blocks" in h.bdl_last_error()


def test_report_entry_point_validates_before_touching_the_device():
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, edges=None, **fields):
        a = _good_report()
        for k, v in fields.items():
            setattr(a, k, v)
        for i, e in (edges or {}).items():
            a.edges[i] = e
        assert h.bdl_temper_report(a, None) == status, (fields, edges, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_temper_report:") and word in msg, (fields, msg)

    assert h.bdl_temper_report(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in ("logp", "state", "totals", "workspace"):
        refused(NULL, f.encode(), **{f: None})
    for f in ("logp", "workspace"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x700008})
    for f in ("labels", "state", "totals"):
        refused(ALIGN, f.encode() + b" not 8-B aligned", **{f: 0x700004})
    refused(ARG, b"groups", groups=0)
    refused(ARG, b"batch", batch=0)
    refused(ARG, b"classes", classes=8193)
    refused(ARG, b"num_bins", num_bins=0)
    refused(ARG, b"num_bins", num_bins=65)
    refused(ARG, b"grid_blocks", grid_blocks=1025)
    refused(ARG, b"unknown flag", flags=2)
    refused(ARG, b"overflows", batch=1 << 58)
    refused(ARG, b"edges", edges={0: 0.0})
    refused(ARG, b"edges", edges={3: float(R.edges32(15)[2])})
    refused(ARG, b"edges", edges={13: 1.0})
    refused(ARG, b"edges", edges={5: float("nan")})
    refused(ARG, b"totals overlaps logp", totals=0x10000 + 8)
    refused(ARG, b"totals overlaps state", totals=0x30000 + 232)
    refused(ARG, b"workspace overlaps labels", workspace=0x20000 + 32)
    refused(ARG, b"workspace overlaps totals", workspace=0x50000 + 3 * 1592 - 8)


def test_entry_points_refuse_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        for call, a in ((h.bdl_temper_fit_sweep, _good_fit()), (h.bdl_temper_fit_update, _good_fit()),
                        (h.bdl_temper_report, _good_report())):
            assert call(a, None) == ARG
            assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_temper_report(None, None) == NULL


def test_kernels_layer_checks_its_arguments_before_any_launch(monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    x, y = torch.zeros(3, 5, 8), torch.zeros(5, dtype=torch.int64)
    for fn, extra in ((K.temper_fit, ()), (K.temper_report, (1.0,))):
        with pytest.raises(ValueError, match="groups"):
            fn(x, y, *extra, groups=2)
        with pytest.raises(ValueError, match="contiguous"):
            fn(x.transpose(1, 2), y, *extra, groups=3)
        with pytest.raises(ValueError, match="classes"):
            fn(torch.zeros(1, 1, 8193), None, *extra)
        with pytest.raises(ValueError, match="grid_blocks"):
            fn(x, y, *extra, groups=3, grid_blocks=1025)
        with pytest.raises(ValueError, match="labels"):
            fn(x, y.to(torch.int32), *extra, groups=3)
        with pytest.raises(ValueError, match="labels"):
            fn(x, torch.zeros(4, dtype=torch.int64), *extra, groups=3)
        with pytest.raises(ValueError, match=r"\[G, N, C\]"):
            fn(torch.zeros(8), y, *extra)
    assert np.array_equal(K.temper_betas(2.0, 3), np.full(3, 0.5, np.float32))
    assert np.array_equal(K.temper_betas([1.0, 4.0], 2), np.array([1.0, 0.25], np.float32))
    for bad in (0.0, 0.001, 101.0, float("nan"), [1.0, 2.0]):
        with pytest.raises(ValueError, match="temperature"):
            K.temper_betas(bad, 3)


def test_kernels_layer_checks_the_fit_and_report_ranges(monkeypatch):
    """(past the shared checks: these need the library, not a device)"""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    monkeypatch.setattr(K, "_temper_rows", lambda *a, **k: (3, 5, 8, 2, None))
    x, y = torch.zeros(3, 5, 8), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="max_iter"):
        K.temper_fit(x, y, groups=3, max_iter=0)
    with pytest.raises(ValueError, match="max_iter"):
        K.temper_fit(x, y, groups=3, max_iter=1025)
    with pytest.raises(ValueError, match="rtol"):
        K.temper_fit(x, y, groups=3, rtol=1.0)
    with pytest.raises(ValueError, match="num_bins"):
        K.temper_report(x, y, 1.0, groups=3, num_bins=65)
    with pytest.raises(ValueError, match="temperature"):
        K.temper_report(x, y, [1.0, 2.0], groups=3)


def test_summary_of_empty_totals_is_nan_not_an_error():
    from bayesdll_amd import _lib as L
    from bayesdll_amd.kernels import temper_summary
    s = temper_summary(np.zeros(1, dtype=np.dtype(L.TemperTotals))[0], 15)
    assert s["n"] == 0 and np.isnan(s["nll"]) and np.isnan(s["ece"]) and np.isnan(s["confidence"])


# ------------------------------------------------- 6. the samplers, without a device
def _bare_sampler():
    from bayesdll_amd import stacked
    S = object.__new__(stacked.StackedSGLD)
    S.K, S.per_chain = 2, None
    S.args = type("A", (), {"device": torch.device("cpu"), "ece_num_bins": 15})()
    return S


def test_sampler_refusals(monkeypatch):
    from bayesdll_amd import chains
    S = _bare_sampler()
    assert S.temperature_ is None
    with pytest.raises(ValueError, match=r'"fitted" needs a fit_temperature\(\) first'):
        S.uncertainty([], temperature="fitted")
    with pytest.raises(ValueError, match='a float, a sequence or "fitted"'):
        S.uncertainty([], temperature="best")
    S._temper = (False, object())
    with pytest.raises(ValueError, match="fitted with by_chain=False, not by_chain=True"):
        S.uncertainty([], by_chain=True, temperature="fitted")
    with pytest.raises(ValueError, match="temperature"):
        S.uncertainty([], by_chain=True, temperature=[1.0, 2.0, 3.0])
    monkeypatch.setattr(chains, "world", lambda: 2)
    with pytest.raises(ValueError, match="fit_temperature: the report describes this process's "
                                         "chains only, and 2 processes"):
        S.fit_temperature([])
    with pytest.raises(ValueError, match="uncertainty: the report describes this process's "
                                         "chains only"):
        S.uncertainty([], temperature=1.5)


def test_temperature_is_not_checkpointed():
    import inspect
    from bayesdll_amd import stacked
    src = inspect.getsource(stacked._StackedSampler.state_dict)
    assert "temper" not in src
