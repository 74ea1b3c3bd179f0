"""What table T of tests/temper_geometry_ref.py reaches, proven without a GPU:
the restated geometry against the header's constants and the launch code's
text, the literal walk (every (group, example, class) taken exactly once, the
report's source lanes equal to the owners, every partial written once and read
once by both second-stage kernels), T against the full set of path labels, the
exact set the older table of tests/test_gpu_temper.py misses, and the input
conditions that make the GPU tests' exact comparisons legitimate for EVERY
case and beta they use — none is skipped at run time."""
import os
import re

import numpy as np
import pytest

import temper_geometry_ref as Gm
import temper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defines():
    src = open(os.path.join(ROOT, "include", "bdl_temper.h")).read()
    return {k: v for k, v in re.findall(r"#define\s+BDL_TEMPER_(\w+)\s+([0-9.]+)f?", src)}


# ------------------------------------------------------------- 1. the restatement
def test_instance_and_geometry_agree_with_the_header_and_the_launch_code():
    d = _defines()
    assert int(d["MAX_CLASSES"]) == Gm.MAX_CLASSES == 8 * 4 * Gm.BLOCK
    assert int(d["WAVE_CLASSES"]) == Gm.WAVE_CLASSES == 4 * 64
    assert int(d["MAX_GRID"]) == Gm.MAX_GRID and int(d["MAX_BINS"]) == R.MAX_BINS == 64
    assert float(d["MAX_T"]) == 100.0 and float(d["MIN_T"]) == 0.01
    assert (R.BETA_MIN, R.BETA_MAX) == (float(np.float32(1) / np.float32(100)), 100.0)
    hip = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "bdl_temper.hip")).read()
    common = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "bdl_kernels.hpp")).read()
    assert re.search(r"constexpr int kBlock = (\d+);", common).group(1) == str(Gm.BLOCK)
    # by_classes' ladder, in its own words
    flat = " ".join(hip.split())
    for text in ("if (classes <= BDL_TEMPER_WAVE_CLASSES) L<1, VEC, true>::go",
                 "else if (groups4 <= kBlock) L<1, VEC, false>::go",
                 "else if (groups4 <= 2 * kBlock) L<2, VEC, false>::go",
                 "else if (groups4 <= 4 * kBlock) L<4, VEC, false>::go",
                 "else L<8, VEC, false>::go", "if (d->classes % 4 == 0)",
                 "nw = (int)std::min<int64_t>(grid, per_group);",
                 "constexpr int TPI = WAVE ? 64 : kBlock;", "constexpr int IPB = WAVE ? kWaves : 1;"):
        assert text in flat, text
    # every class count: the instance holds the row, the one below would not
    seen = set()
    for C in range(1, Gm.MAX_CLASSES + 1):
        nt, vec, wave = Gm.instance(C)
        seen.add((nt, vec, wave))
        q = (C + 3) // 4
        assert vec == (C % 4 == 0) and wave == (C <= 256)
        assert q <= nt * (64 if wave else 256)
        assert wave or nt == 1 or q > (nt // 2) * 256
    assert seen == set(Gm.INSTANCES) and len(seen) == 10
    for C, want in ((256, (1, True, True)), (257, (1, False, False)), (1024, (1, True, False)),
                    (1025, (2, False, False)), (1028, (2, True, False)), (2048, (2, True, False)),
                    (2049, (4, False, False)), (4096, (4, True, False)), (4097, (8, False, False)),
                    (8192, (8, True, False))):
        assert Gm.instance(C) == want, C
    assert Gm.geometry(11, 3, 10, 2) == (2, 2) and Gm.geometry(3, 2, 10, 4) == (4, 1)
    assert Gm.geometry(259, 2, 260, 259) == (259, 259) and Gm.geometry(1030, 2, 260, 1024) == (1024, 1024)
    assert Gm.geometry(5, 1, 8192, 7) == (7, 5)
    assert len(Gm.ALL_LABELS) == 28


@pytest.mark.parametrize("case", Gm.T, ids=Gm.case_id)
def test_walk_takes_every_group_example_and_class_exactly_once(case):
    C, N, G, grid = case[:4]
    visits, partials, _, _ = Gm.walk(C, N, G, grid)    # (asserts on the way)
    assert visits.shape == (G, N, C) and (visits == 1).all()
    nw = Gm.geometry(N, G, C, grid)[1]
    assert len(partials) == G * nw
    upd, comb = Gm.second_stage(nw)
    assert (upd == 1).all() and (comb == 1).all()


def test_second_stage_takes_every_partial_once_at_every_count():
    for nw in list(range(1, 20)) + [255, 256, 257, 259, 511, 512, 513, 1023, 1024]:
        upd, comb = Gm.second_stage(nw)
        assert (upd == 1).all() and (comb == 1).all(), nw


def test_walk_at_other_grids_of_one_shape_per_mode():
    for C, N, G in ((10, 11, 3), (1030, 7, 3)):
        for grid in (1, 2, 3, 5, 7, 64, 1024):
            assert (Gm.walk(C, N, G, grid)[0] == 1).all(), (C, grid)


# ------------------------------------------------------------- 2. what T reaches
def test_table_reaches_every_label():
    got = set()
    for case in Gm.T:
        got |= Gm.labels(case)
    assert got == set(Gm.ALL_LABELS), sorted(set(Gm.ALL_LABELS) - got)
    # and the plan is what the rows hold: a planted top class is the row's one maximum
    for case in Gm.T:
        z, lab = Gm.rows(case)
        for b, (pl, top) in Gm.plan(case).items():
            assert pl is None or lab[b] == pl
            assert top is None or (z[:, b].argmax(-1) == top).all()


def _small_default_grid(N, G, C):
    """The default grid where it cannot depend on the device: the wanted
    per_group * G workgroups are fewer than four per CU of any gfx9 part."""
    per_group = -(-N // (4 if C <= 256 else 1))
    assert per_group * G <= 4 * 64
    return per_group * G


def test_what_the_older_table_does_not_reach():
    """tests/test_gpu_temper.py: SHAPES with _group_rows' inputs, and the
    special-row test's C = 37 / 300 at N = 16 and its 10-row subset."""
    import test_gpu_temper as Old
    got = set()
    for C, N, G, grid in Old.SHAPES:
        z, lab = Old._group_rows(C, N, G, special=N >= 8)
        grid = grid or _small_default_grid(N, G, C)
        got |= Gm.walk(C, N, G, grid)[2] | Gm.data_labels(C, z, lab)
    for C in (37, 300):
        z, lab = R.make_rows(16, C, 77, sharp=0.7, special=True)
        keep = np.r_[0, 1, 8:16]
        for zz, ll in ((z, lab), (z[keep], lab[keep])):
            n = len(ll)
            got |= Gm.walk(C, n, 1, _small_default_grid(n, 1, C))[2] | Gm.data_labels(C, zz[None], ll)
    missed = set(Gm.ALL_LABELS) - got
    assert missed == {
        "inst:wg:NT2:vec", "inst:wg:NT2:elem", "inst:wg:NT4:vec", "inst:wg:NT4:elem",
        "inst:wg:NT8:elem", "trip2:multi", "late_trip:partial", "late_trip:empty_wave",
        "late_trip:no_group", "late_trip:tail", "label:trip0", "label:last", "nw>256",
        "nw=1024",
    }, sorted(missed)


# ------------------------------------------- 3. the inputs are away from every decision
def _no_ties(z):
    bad = (np.isnan(z) | np.isposinf(z)).any(-1) | ~np.isfinite(z).any(-1)
    zz = np.where(np.isnan(z), -np.inf, z)
    return ((zz == zz.max(-1, keepdims=True)).sum(-1)[~bad] == 1).all()


@pytest.mark.parametrize("case", Gm.T, ids=Gm.case_id)
def test_input_conditions_of_every_case_and_beta(case):
    z, lab = Gm.rows(case)
    assert _no_ties(z)
    for g, beta in enumerate(Gm.betas_of(case)):
        assert beta == float(np.float32(beta))
        assert R.margins(R.report_reference(z[g], lab, beta, 15), 15) > 1, (g, beta)
        em = R.newton(z[g], lab)
        assert em["margin"] > 1, (g, em["margin"])
        assert em["converged"] and not em["at_bound"] and not em["degenerate"], (g, em)
        s = R.sweep_reference(z[g], lab, beta)
        assert s["n"] >= 1 and s["d2"] > 0
    if Gm.has_special(case):
        s = R.sweep_reference(z[0], lab, 1.0)
        assert (s["n_nonfinite"], s["n_inf_label"]) == (3, 1)


@pytest.mark.parametrize("case", Gm.BIN_CASES, ids=Gm.case_id)
def test_input_conditions_of_the_bin_count_cases(case):
    z, lab = Gm.rows(case)
    top = 0
    for nb in Gm.BIN_COUNTS:
        for g, beta in enumerate(Gm.BIN_BETAS):
            r = R.report_reference(z[g], lab, beta, nb)
            assert R.margins(r, nb) > 1, (nb, g)
            assert r["bin_count"][nb:].sum() == 0 and r["bin_count"].sum() == r["n_labelled"] * case[0]
            if nb == 64:
                top += int(r["bin_count"][63])
    assert top > 0      # lane 63 owns a bin that is not empty


def test_input_conditions_of_the_fit_decisions():
    # the upper limit: 1 -> 4 -> 16 -> 64 -> 100 by the 4x clamp, one more sweep stops there
    z, lab = Gm.upper_limit_rows()
    assert _no_ties(z) and (z.argmax(-1) == lab).all()
    em = R.newton(z, lab)
    assert em["at_bound"] and em["done"] and not em["converged"] and not em["degenerate"]
    assert em["beta"] == R.BETA_MAX and em["iterations"] == 4 and em["sweeps"] == 5
    assert em["margin"] > 1
    betas, st = [], None
    for k in range(1, 5):
        st = R.newton(z, lab, max_iter=k)
        betas.append(st["beta"])
    assert betas == [4.0, 16.0, 64.0, 100.0]
    # max_iter = 2 on a case that needs more
    case = Gm.MAX_ITER_CASE
    z, lab = Gm.rows(case)
    for g in range(case[2]):
        full, two = R.newton(z[g], lab), R.newton(z[g], lab, max_iter=2)
        assert full["iterations"] > 2 and full["margin"] > 1
        assert two["iterations"] == 2 and not two["done"] and not two["degenerate"]
        assert two["margin"] > 1
    # rtol = 0: the emulation stops on a step that rounds to beta itself, early
    for g in range(case[2]):
        em = R.newton(z[g], lab, rtol=0.0)
        assert em["converged"] and em["done"] and em["iterations"] <= 12, (g, em)
    # no labels
    em = R.newton(z[0], None)
    assert em["degenerate"] and em["n"] == 0 and np.isnan(em["nll"]) and em["beta"] == 1.0
