"""What table P of tests/predict_geometry_ref.py reaches, proven without a GPU:
the restated geometry against the header's constants and the kernel's text,
the literal walk (every example taken once, every partial written once and
read once by the combine), P against the full set of path labels, the exact set
the older table of tests/test_gpu_predict.py misses, and the input conditions
that make the GPU tests' exact comparisons legitimate for EVERY case and bin
count they use — none is skipped at run time."""
import os
import re

import numpy as np
import pytest

import predict_geometry_ref as Gm
import predict_ref as R
from test_predict_host import check_against, check_totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(c, nb) for c in Gm.P for nb in c.bins]


def run_id(cn):
    return "{}-nb{}".format(Gm.case_id(cn[0]), cn[1])


# ------------------------------------------------------------- 1. the restatement
def test_geometry_agrees_with_the_header_and_the_kernel_text():
    src = open(os.path.join(ROOT, "include", "bdl_predict.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define\s+BDL_PREDICT_(\w+)\s+(\d+)", src)}
    assert d["MAX_CLASSES"] == Gm.MAX_CLASSES == 8 * 4 * Gm.BLOCK
    assert d["WAVE_CLASSES"] == Gm.WAVE_CLASSES == 4 * 64
    assert d["MAX_GRID"] == Gm.MAX_GRID and d["MAX_BINS"] == Gm.MAX_BINS == R.MAX_BINS
    csrc = os.path.join(ROOT, "bayesdll_amd", "csrc")
    common = open(os.path.join(csrc, "bdl_kernels.hpp")).read()
    assert re.search(r"constexpr int kBlock = (\d+);", common).group(1) == str(Gm.BLOCK)
    flat = " ".join(open(os.path.join(csrc, "bdl_predict.hip")).read().split())
    chain = " ".join(open(os.path.join(csrc, "bdl_chain_common.hpp")).read().split())
    for text in (
            "constexpr int kWaves = kBlock / 64;",
            "constexpr int TPI = WAVE ? 64 : kBlock;", "constexpr int IPB = WAVE ? kWaves : 1;",
            "const int ti = WAVE ? lane : t;",
            "const uint32_t r = rotated_block(g);",
            "if ((int64_t)r * IPB >= a.batch) continue;",
            "const int64_t bstride = (int64_t)gridDim.x * IPB;",
            "for (int64_t b = (int64_t)r * IPB + (WAVE ? wave : 0); b < a.batch; b += bstride)",
            "const int c0 = 4 * (q + TPI * u);", "am = 4 * (ti + TPI * u) + j;",
            "if ((ks & 0xff) == lane)",
            "block_total(tot, bn, partials + (int64_t)g * nw + r, false);",
            "const bdl_predict_totals* __restrict__ part = partials + (int64_t)blockIdx.x * nw;",
            "const int lo = (int)((int64_t)w * nw / kWaves), hi = (int)((int64_t)(w + 1) * nw / kWaves);",
            "for (int i = lo; i < hi; ++i)",
            "const int64_t ipb = d->classes <= BDL_PREDICT_WAVE_CLASSES ? kWaves : 1;",
            "const int64_t per_group = (d->batch + ipb - 1) / ipb;",
            "const int64_t want = std::min<int64_t>(per_group, BDL_PREDICT_MAX_GRID) * d->groups;",
            "grid = (int)capped_grid(std::min<int64_t>(want, (int64_t)cu_count() * 4), "
            "BDL_PREDICT_MAX_GRID);",
            "const int nw = (int)std::min<int64_t>(grid, per_group);",
            "if (d->classes % 4 == 0)"):
        assert text in flat, text
    for text in ("return (blockIdx.x + gridDim.x - (uint32_t)i % gridDim.x) % gridDim.x;",
                 "return std::max<int64_t>(1, std::min(want, cap));"):
        assert text in chain, text
    seen = set()
    for C in range(1, Gm.MAX_CLASSES + 1):
        nt, vec, wave = Gm.instance(C)
        seen.add((nt, vec, wave))
        q = (C + 3) // 4
        assert vec == (C % 4 == 0) and wave == (C <= 256)
        assert q <= nt * (64 if wave else 256)
        assert wave or nt == 1 or q > (nt // 2) * 256
    assert seen == set(Gm.INSTANCES) and len(seen) == 10
    assert Gm.launch(5, 3, 9, 0) == (9, 3, 4) and Gm.launch(5, 3, 9, 2) == (2, 2, 4)
    assert Gm.launch(260, 3, 5, 7) == (7, 5, 1) and Gm.launch(257, 2, 7, 0) == (14, 7, 1)
    assert Gm.launch(260, 1, 1024, 259) == (259, 259, 1)
    assert Gm.launch(5, 1, 4096, 1024) == (1024, 1024, 4)
    assert Gm.launch(5, 1, 4096, 0) == (1024, 1024, 4) and Gm.launch(5, 1, 4096, 0, cus=64) == (256, 256, 4)
    assert Gm.launch(8192, 2, 16, 0) == (32, 16, 1) and Gm.launch(1, 1, 1, 0) == (1, 1, 4)


def test_owner_gives_every_class_one_thread_trip_and_slot():
    for C in sorted({c.C for c in Gm.P}):
        nt, _, wave = Gm.instance(C)
        tpi = 64 if wave else 256
        seen = set()
        for c in range(C):
            o = Gm.owner(C, c)
            assert 4 * (o.thread + tpi * o.trip) + o.slot == c and o.trip < nt and o.thread < tpi
            assert o.lane == o.thread % 64 and (wave or o.wave == o.thread // 64)
            assert o.tail == (C % 4 != 0 and c >= C - C % 4)
            seen.add((o.thread, o.trip, o.slot))
        assert len(seen) == C
        assert Gm.trips_used(C) == max(Gm.owner(C, c).trip for c in range(C)) + 1
    o = Gm.owner(1028, 1024)
    assert (o.thread, o.wave, o.lane, o.trip, o.slot, o.tail) == (0, 0, 0, 1, 0, False)
    o = Gm.owner(1028, 1020)
    assert (o.thread, o.wave, o.lane, o.trip, o.slot) == (255, 3, 63, 0, 0)
    o = Gm.owner(255, 254)
    assert (o.thread, o.wave, o.lane, o.trip, o.slot, o.tail) == (63, None, 63, 0, 2, True)
    assert Gm.tie_labels(1028, "am", 1020, 1024) == {"tie:am:waves", "tie:am:trips"}
    assert Gm.tie_labels(1028, "pred", 20, 1024) == {"tie:pred:lanes", "tie:pred:trips"}
    assert Gm.tie_labels(1028, "am", 2, 1025) == {"tie:am:slots"}
    assert Gm.tie_labels(256, "pred", 3, 255) == set()      # wave mode: the lower lane, the lower class


@pytest.mark.parametrize("case", Gm.P, ids=Gm.case_id)
def test_walk_takes_every_example_and_partial_exactly_once(case):
    for grid_blocks in case.grids:
        grid, nw, ipb = Gm.launch(case.C, case.G, case.B, grid_blocks)
        where, count, _ = Gm.walk(case.C, case.G, case.B, grid_blocks)   # (asserts on the way)
        assert count.shape == (case.G, nw) and (count.sum(1) == case.B).all() and (count > 0).all()
        for (g, b), (r, blk, trip, w) in where.items():
            assert b == r * ipb + w + trip * grid * ipb and blk == (r + g) % grid
        assert (Gm.combine(nw)[1] == 1).all()


def test_combine_takes_every_partial_once_at_every_count():
    for nw in range(1, Gm.MAX_GRID + 1):
        quarter, times, empty = Gm.combine(nw)
        assert (times == 1).all() and (np.diff(quarter) >= 0).all(), nw
        assert len(empty) == max(0, 4 - nw)
    assert Gm.combine(1)[2] == [0, 1, 2] and Gm.combine(3)[2] == [0]
    assert Gm.combine(259)[0].tolist().count(3) == 65 and Gm.combine(5)[0].tolist() == [0, 1, 2, 3, 3]


# ------------------------------------------------------------- 2. what P reaches
def test_table_reaches_every_label():
    per_case = {Gm.case_id(c): Gm.labels(c) for c in Gm.P}
    got = set().union(*per_case.values())
    assert got == set(Gm.ALL_LABELS), sorted(set(Gm.ALL_LABELS) - got)
    assert len(Gm.ALL_LABELS) == 82
    # every plant reaches what it is there for
    for c in Gm.P:
        for p in c.plants:
            assert Gm.plant_labels(c, p) <= per_case[Gm.case_id(c)], (Gm.case_id(c), p)
    # the paths that one construction each provides, by name
    for label, cid in (
            ("nw:259", "C5-M2-G1-B4096"), ("nw:1024", "C260-M2-G1-B1024"),
            ("nw<grid:G>1", "C260-M2-G3-B5"), ("G>grid", "C5-M3-G3-B9"), ("nw:3", "C5-M3-G3-B9"),
            ("wave:B%4=3", "C256-M2-G1-B11"), ("wave:B%4=2", "C255-M3-G2-B10"),
            ("bin:lane32", "C255-M3-G2-B10"), ("bin:lane63", "C255-M3-G2-B10"),
            ("bins:1", "C8192-M3-G1-B16"), ("bins:33", "C2052-M3-G2-B16"),
            ("tie:am:lanes", "C1028-M3-G2-B16"), ("tie:pred:lanes", "C1028-M3-G2-B16"),
            ("tie:am:trips", "C1028-M3-G2-B16"), ("tie:pred:waves", "C1028-M3-G2-B16"),
            ("tie:pred:waves", "C257-M2-G2-B7"), ("tie:am:slots", "C1028-M3-G2-B16"),
            ("pred:lane63", "C256-M2-G1-B11"), ("am:lane63", "C255-M3-G2-B10"),
            ("label:C-1:tail", "C1030-M3-G1-B16"), ("label:2^40", "C1030-M3-G1-B16"),
            ("pred:NT4:last", "C2052-M3-G2-B16"), ("am:NT4:last", "C2050-M3-G1-B5"),
            ("label:NT8:last", "C4099-M3-G1-B16"), ("pred:NT8:last", "C8192-M3-G1-B16"),
            ("pred:NT2:last", "C1030-M3-G1-B16"), ("label:NT2:last", "C1028-M3-G2-B16"),
            ("nonfinite:then_finite", "C255-M3-G2-B10"),
            ("nonfinite:shares_workgroup", "C5-M3-G3-B9"),
            ("inst:wg:NT1:elem", "C257-M2-G2-B7"), ("inst:wg:NT4:elem", "C2050-M3-G1-B5")):
        assert label in per_case[cid], (label, cid)
    assert {Gm.instance(c.C) for c in Gm.P} == set(Gm.INSTANCES)
    assert {nb for c in Gm.P for nb in c.bins} == set(Gm.BIN_COUNTS)
    assert all(c.M <= 5 and (c.B <= 16 or c in Gm.BIG) for c in Gm.P)


def test_what_the_older_table_does_not_reach():
    """predict_ref.CASES at grid_blocks 1, 2 and 0 with 15 bins (on any device
    of at least 98 CUs: its largest default grid wants 390 workgroups)."""
    got = set()
    for c in R.CASES:
        x, lab, r, _ = R.built(c)
        Cn, _, G, B = c[:4]
        got |= Gm.data_labels(Cn, x, lab, r) | Gm.bin_labels(r, R.NB)
        for grid in (1, 2, 0):
            got |= Gm.geometry_labels(Cn, G, B, grid, r["nonfinite"])
            assert Gm.launch(Cn, G, B, grid, cus=98) == Gm.launch(Cn, G, B, grid)
    missed = set(Gm.ALL_LABELS) - got
    assert missed == {
        "bins:1", "bins:2", "bins:16", "bins:33", "bins:64",
        "bin:lane>=15", "bin:lane32", "bin:lane63",
        "nw:3", "nw:259", "nw:1024", "wave:B%4=3",
        "am:lane63", "pred:lane63", "label:lane63",
        "am:NT4:last", "pred:NT2:last", "pred:NT4:last",
        "label:NT2:last", "label:NT4:last", "label:NT8:last",
        "tie:am:lanes", "tie:am:waves", "tie:am:trips",
        "tie:pred:lanes", "tie:pred:waves", "tie:pred:trips",
        "label:2^40",
    }, sorted(missed)


# ------------------------------------------- 3. the inputs are away from every decision
@pytest.mark.parametrize("cn", RUNS, ids=run_id)
def test_input_conditions_and_emulation_of_every_case_and_bin_count(cn):
    """No reference probability within 4 bounds of a bin edge, no example's top
    two mixture probabilities within 4 bounds of each other, no member row with
    two maxima — for ALL examples; only the constructed ties are exempt
    (make_case's examples 3 and 7, the planted ones).  And the emulation of
    the header's contract is within the bound of the reference."""
    case, nb = cn
    x, lab, r, b = Gm.built(case, nb)
    m = R.margins(r, b, nb)
    assert m["edge"] >= 4, m
    assert m["top2"] >= 4, m
    mt, pt = Gm.planted_ties(case)
    ok = ~r["nonfinite"]
    assert np.array_equal(m["tied"] & ok, pt & ok), "only the constructed ties"
    assert np.array_equal(R.member_ties(x), mt)
    if case.B >= 8:
        assert r["nonfinite"][:, 5:8].all() and r["nonfinite"].sum() == 3 * case.G
    else:
        assert not r["nonfinite"].any()
    em = R.emulate(x, lab, nb)
    check_against(em, r, b, run_id(cn))
    check_totals(em["totals"], r, b, run_id(cn))
    for t in r["totals"]:
        assert t["bin_count"][nb:].sum() == 0 and t["bin_count"].sum() == t["n_labelled"] * case.C
        if nb == 64:    # lane 63's bin and one of lanes 16 .. 62 are not empty
            assert t["bin_count"][63] > 0 and t["bin_count"][16:63].sum() > 0


@pytest.mark.parametrize("case", [c for c in Gm.P if c.plants], ids=Gm.case_id)
def test_plants_are_what_the_reference_sees(case):
    x, lab, r, _ = Gm.built(case, case.bins[0])
    for p in case.plants:
        e = Gm.expected(case, p)
        if e is None:
            assert lab[p[1]] == p[2] and np.isnan(r["nll"][:, p[1]]).all()
            continue
        b, pred, dis, labelled, wrong, lb = e
        assert (r["pred"][:, b] == pred).all() and (r["disagree"][:, b] == dis).all(), p
        assert lab[b] == lb and np.isnan(r["nll"][:, b]).all() == (not labelled), p
        for t in r["totals"]:
            assert bool(t["wrong_mask"][b]) == wrong, p
        if p[0] == "gap":
            assert np.allclose(r["pbar"][:, b, p[2]], p[4], atol=1e-5)
    assert len({p[1] for p in case.plants}) == len(case.plants)


def test_totals_bound_covers_the_number_of_terms():
    """Beyond 2^8 examples the summation term is (2 n + 4) 2^-53 of the sum of
    magnitudes (predict_ref's docstring); up to 2^8 it is 2^-45 as before."""
    for case in Gm.BIG:
        x, lab, r, b = Gm.built(case, 64)
        t, bt = r["totals"][0], b["totals"][0]
        n = int(t["ok_mask"].sum())
        assert n + t["n_nonfinite"] == case.B > 2 ** 8
        per = b["entropy"][0][t["ok_mask"]].sum()
        f = (bt["entropy_sum"] - per) / np.abs(r["entropy64"][0][t["ok_mask"]]).sum()
        assert abs(f / ((2 * n + 4) * 2.0 ** -53) - 1) < 1e-3 and f > (n - 1 + 4) * 2.0 ** -53 > 2.0 ** -45
    x, lab, r, b = R.built(R.CASES[4])
    t, bt = r["totals"][0], b["totals"][0]
    per = b["entropy"][0][t["ok_mask"]].sum()
    f = (bt["entropy_sum"] - per) / np.abs(r["entropy64"][0][t["ok_mask"]]).sum()
    assert abs(f / 2.0 ** -45 - 1) < 1e-3


def test_a_probability_on_an_fp32_edge_goes_to_the_upper_bin():
    """include/bdl_predict.h: bin = #{j : edges[j] <= pbar32}, against the
    fp32 edges.  Four equal logits give 0.25 exactly, the first of four bins'
    edges rounds to 0.25 in fp32 (it is above 0.25 in fp64): all four classes
    belong in bin 1."""
    flat = " ".join(open(os.path.join(ROOT, "include", "bdl_predict.h")).read().split())
    assert "bin = #{j : edges[j] <= pbar32}" in flat and "against the * fp32 edges" in flat
    e = R.edges32(4)
    assert e[0] == np.float32(0.25) and np.linspace(0, 1 + 1e-8, 5)[1] > 0.25
    x, lab = Gm.edge_inputs()
    em = R.emulate(x, lab, 4)
    assert em["totals"][0]["bin_count"][:4].tolist() == [0, 4, 0, 0]
    assert em["totals"][0]["bin_hits"][:4].tolist() == [0, 1, 0, 0]
    assert em["totals"][0]["bin_conf"][1] == 1.0 and em["confidence"][0, 0] == np.float32(0.25)
    # the fp64 definition with fp64 edges would say bin 0: this input is ON the decision
    assert R.reference(x, lab, 4)["totals"][0]["bin_count"][0] == 4
