"""What table P of tests/mixture_geometry_ref.py reaches, proven without a GPU:
the restated geometry against the header's constants and the kernel's text,
the literal walk (every row taken once, every partial written once and read
once by the combine), P against the full set of path labels at 256 and at 64
CUs, the restatement against tests/mixture_ref.py, the two literal input
builders through the emulation, the break table (wrong variants of the
restatement, each changing the expected answer of a case of P), and the cap on
what check_mixture may leave unchecked."""
import os
import re

import numpy as np
import pytest

import mixture_geometry_ref as Gm
import mixture_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------- 1. the restatement
def test_geometry_agrees_with_the_header_and_the_kernel_text():
    src = open(os.path.join(ROOT, "include", "bdl_mixture.h")).read()
    d = dict(re.findall(r"#define\s+BDL_MIXTURE_(\w+)\s+([\w.\-]+)", src))
    assert int(d["MAX_CLASSES"]) == Gm.MAX_CLASSES == 4 * 4 * Gm.BLOCK
    assert int(d["WAVE_CLASSES"]) == Gm.WAVE_CLASSES == 4 * 64
    assert int(d["MAX_PAIRS"]) == Gm.MAX_PAIRS and int(d["MAX_GRID"]) == Gm.MAX_GRID
    assert float(d["MIN_WEIGHT"]) == R.MIN_WEIGHT == 1e-10
    csrc = os.path.join(ROOT, "bayesdll_amd", "csrc")
    common = open(os.path.join(csrc, "bdl_kernels.hpp")).read()
    assert re.search(r"constexpr int kBlock = (\d+);", common).group(1) == str(Gm.BLOCK)
    flat = " ".join(open(os.path.join(csrc, "bdl_mixture.hip")).read().split())
    chain = " ".join(open(os.path.join(csrc, "bdl_chain_common.hpp")).read().split())
    for text in (
            "constexpr int kWaves = kBlock / 64;",
            "constexpr int TPI = WAVE ? 64 : kBlock;", "constexpr int IPB = WAVE ? kWaves : 1;",
            "const int ti = WAVE ? lane : t;",
            "const int64_t bstride = (int64_t)gridDim.x * IPB;",
            "int64_t b = (int64_t)blockIdx.x * IPB + (WAVE ? wave : 0);",
            "for (; b < a.batch; b += bstride) {",
            "if (b + bstride < a.batch) load_row<NT, VEC, TPI>(nxt, base + (b + bstride) * C, ti, C);",
            "for (int64_t b = (int64_t)blockIdx.x * IPB + (WAVE ? wave : 0); b < a.batch; "
            "b += bstride) {",
            "const int c0 = 4 * (q + TPI * u);", "am = 4 * (ti + TPI * u) + j;",
            "if (ov > v || (ov == v && oi < i)) {",
            "block_total(acc, partials + (int64_t)blockIdx.y * gridDim.x + blockIdx.x);",
            "block_total(tot, partials + (int64_t)g * gridDim.x + blockIdx.x);",
            "while (c < a.components && a.weights[(int64_t)c * a.groups + g] < "
            "BDL_MIXTURE_MIN_WEIGHT) ++c;",
            "const int cn = next_component(a, g, c + 1);",
            "if (s + 1 < D) load_row<NT, VEC, TPI>(nxt, row + (i + 1) * a.member_stride, ti, C);",
            "else if (cn < a.components) load_row<NT, VEC, TPI>(nxt, row + (int64_t)cn * D * "
            "a.member_stride, ti, C);",
            "const Acc* __restrict__ part = partials + (int64_t)blockIdx.x * nw;",
            "for (int i = threadIdx.x; i < nw; i += kBlock) s.add(part[i]);",
            "for (int k = 1; k < kWaves; ++k) s.add(s_acc[k]);",
            "if (a.classes <= BDL_MIXTURE_WAVE_CLASSES)", "else if (groups4 <= kBlock)",
            "else if (groups4 <= 2 * kBlock)",
            "const int64_t ipb = classes <= BDL_MIXTURE_WAVE_CLASSES ? kWaves : 1;",
            "const int64_t slots = (batch + ipb - 1) / ipb;",
            "const int64_t share = ((int64_t)cu_count() * 4 + pairs - 1) / pairs;",
            "return (int)capped_grid(std::min(slots, share), BDL_MIXTURE_MAX_GRID);",
            "const dim3 grid(bpp, (unsigned)pairs);", "const dim3 grid(bpg, (unsigned)d->groups);",
            "if (d->classes % 4 == 0)"):
        assert text in flat, text
    for text in ("for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);",
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
        assert Gm.covered(C).all()
    assert seen == set(Gm.INSTANCES) and len(seen) == 8
    assert len(Gm.ALL_LABELS) == 24 + 14 + 6 + 4 + 4 + 6 + 4 + 7 + 5 + 11 + 8
    assert Gm.launch(3, 1, 4100, 0) == 1024 and Gm.launch(3, 1, 4100, 0, cus=64) == 256
    assert Gm.launch(257, 1, 1030, 0) == 1024 and Gm.launch(257, 1, 1023, 0) == 1023
    assert Gm.launch(5, 100, 50, 0) == 11 and Gm.launch(5, 100, 50, 0, cus=64) == 3
    assert Gm.launch(5, 1100, 5, 0) == 1 and Gm.launch(5, 300, 5, 0, cus=64) == 1
    assert Gm.launch(5, 3, 9, 0) == 3 and Gm.launch(260, 3, 9, 0) == 9
    assert Gm.launch(4, 65535, 2, 1) == 1 and Gm.launch(4, 65535, 2, 0) == 1


def test_owner_gives_every_class_one_thread_trip_and_slot():
    for C in sorted(set(Gm.EDGES) | {1, 3, 4, 5, 1030, 3072, 3073}):
        nt, _, wave = Gm.instance(C)
        tpi = 64 if wave else Gm.BLOCK
        seen = set()
        for c in range(C):
            o = Gm.owner(C, c)
            assert 4 * (o.thread + tpi * o.trip) + o.slot == c and o.trip < nt
            assert o.lane == o.thread % 64 and (wave or o.wave == o.thread // 64)
            assert o.tail == (C % 4 != 0 and c >= C - C % 4)
            seen.add((o.thread, o.trip, o.slot))
        assert len(seen) == C


def test_the_walk_takes_every_row_and_every_partial_once():
    """walk asserts it; here over every row count and grid around the strides,
    and at the pair limit."""
    for C in (5, 260):
        for B in list(range(1, 40)) + [1023, 1024, 1025, 4097]:
            for grid in (0, 1, 2, 3, 7, 16, 1024):
                wk = Gm.walk(C, 3, B, grid)
                assert sum(len(r) for t in wk.taken for r in t) == B
                assert (wk.part >= 0).all() and wk.part.max() < wk.bpp
                for x in range(wk.bpp):             # a slot's rows: x * IPB + w + k * bpp * IPB
                    for w, rows in enumerate(wk.taken[x]):
                        assert np.array_equal(rows, (x * wk.ipb + w)
                                              + wk.bpp * wk.ipb * np.arange(len(rows)))
    wk = Gm.walk(4, Gm.MAX_PAIRS, 2, 1)
    assert wk.bpp == 1 and [len(r) for r in wk.taken[0]] == [1, 1, 0, 0]
    with pytest.raises(AssertionError):
        Gm.launch(4, Gm.MAX_PAIRS + 1, 2, 1)


def test_members_walks_the_unskipped_components_and_prefetches_the_next_row():
    S = Gm.Step
    assert Gm.members((0.5, 0.0, 0.0, 0.5), 2) == [S(0, 0, 0, 1), S(0, 1, 1, 6), S(3, 0, 6, 7),
                                                    S(3, 1, 7, None)]
    assert Gm.members((0.0, 1.0), 1) == [S(1, 0, 1, None)]
    assert Gm.members((0.0, 0.0), 3) == []
    assert Gm.members((1e-10, 9e-11, 0.5), 1) == [S(0, 0, 0, 2), S(2, 0, 2, None)]
    for cols, D in ((Gm.W4, 1), (Gm.W4, 2), (Gm.W4, 4), (Gm.W3, 3), (Gm.W2, 1)):
        for w in cols:
            steps = Gm.members(w, D)
            act = [c for c, v in enumerate(w) if v >= R.MIN_WEIGHT]
            assert [(s.comp, s.draw) for s in steps] == [(c, s) for c in act for s in range(D)]
            assert [s.read for s in steps] == [c * D + s for c in act for s in range(D)]
            assert [s.prefetch for s in steps] == ([s.read for s in steps][1:] + [None])[:len(steps)]
            assert Gm.skip_labels(w) <= Gm.ALL_LABELS
    assert Gm.skip_labels(Gm.W4[6]) == {"skip:middle", "skip:threshold"}
    assert Gm.skip_labels(Gm.W4[4]) == {"skip:middle", "skip:run"}
    assert Gm.skip_labels(Gm.W4[7]) == {"skip:first", "skip:run"}


def test_the_combine_takes_every_partial_once_in_its_order():
    rng = np.random.default_rng(5)
    for nw in list(range(1, 70)) + [255, 256, 257, 511, 512, 513, 1023, 1024]:
        p = np.zeros((2, nw), Gm.PART)
        p["n"] = 1
        p["n_nonf"] = np.arange(nw)[None, :]
        p["n_wrong"][:, nw - 1] = 7                      # the last partial alone
        p["sum"] = rng.integers(-2 ** 30, 2 ** 30, size=(2, nw))      # exact in any order
        got = Gm.combine(p)
        assert got["n"].tolist() == [nw, nw] and got["n_nonf"].tolist() == [nw * (nw - 1) // 2] * 2
        assert got["n_wrong"].tolist() == [7, 7]
        assert np.array_equal(got["sum"], p["sum"].sum(1))
        twice = Gm.combine(p, prior=got, reset=False)
        assert twice["n"].tolist() == [2 * nw] * 2 and np.array_equal(twice["sum"], 2 * got["sum"])
    # the order, literally, at 300 partials of one pair
    v = rng.standard_normal(300)
    p = np.zeros((1, 300), Gm.PART)
    p["sum"][0] = v
    t = np.zeros(256)
    t += v[:256]
    t[:44] += v[256:]
    waves = []
    for w in range(4):
        lane = t[64 * w:64 * w + 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[np.arange(64) ^ off]
        assert len(set(lane.tolist())) == 1               # every lane holds the wave's sum
        waves.append(lane[0])
    want = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert Gm.combine(p)["sum"][0].tobytes() == np.float64(want).tobytes()


# ------------------------------------------------------------- 2. coverage
@pytest.mark.parametrize("cus", [256, 64])
def test_P_reaches_every_label(cus):
    got = set()
    for c in Gm.P:
        assert Gm.logits_of(c) < 10 ** 6, Gm.case_id(c)
        mine = Gm.labels_of(c, cus)
        assert mine <= Gm.ALL_LABELS, mine - Gm.ALL_LABELS
        got |= mine
    # 4 x 64 workgroups are below the cap of 1024: at 64 CUs it cannot decide
    unreachable = {"default:cap"} if 4 * cus < Gm.MAX_GRID else set()
    assert got == Gm.ALL_LABELS - unreachable, sorted(Gm.ALL_LABELS - got)
    assert unreachable <= Gm.CU_LABELS


def test_the_older_table_misses_what_the_issue_lists():
    """mixture_ref.CASES at grids 1, 2, 0: at most 9 partials, 3 trips of a row
    slot, 18 pairs, two draws, one skip pattern."""
    for C, B, comps, D, G, _ in R.CASES:
        for grid in (1, 2, 0):
            for pairs in (comps * D * G, G):
                wk = Gm.walk(C, pairs, B, grid)
                assert wk.bpp <= 9 and pairs <= 18 and D <= 2
                assert wk.ipb == 1 or max(len(r) for t in wk.taken for r in t) <= 3
                if grid == 0:
                    assert Gm.default_label(C, pairs, B) == "default:slots"
        assert C not in (252, 255, 260, 1021, 1024, 1025, 1028, 2049, 2052)


# ------------------------------------------------------------- 3. against the references
@pytest.mark.parametrize("case", Gm.P, ids=Gm.case_id)
def test_the_restatement_agrees_with_the_references(case):
    x, lab, w = Gm.random_inputs(case)
    sr, mr = Gm.references(case)
    M, G = case.comps * case.draws, case.groups
    inr = (lab >= 0) & (lab < case.C)
    bad = R.nonfinite_rows(np.asarray(x, dtype=np.float64)) & inr[None, None, :]
    wrong = sr["ok"] & (np.where(R.nonfinite_rows(np.asarray(x, np.float64))[..., None], 0.0,
                                 x).argmax(-1) != lab[None, None, :])
    fin = sr["ok"] & np.isfinite(sr["nll"])
    for grid in case.grids:
        got, parts = Gm.score_expected(case, grid, sr["nll"], sr["ok"], bad, wrong)
        got = got.reshape(M, G)
        assert np.array_equal(got["n"], sr["n"]) and np.array_equal(got["n_nonf"], sr["n_nonfinite"])
        assert np.array_equal(got["n_wrong"], sr["n_wrong"])
        ok = np.isfinite(sr["nll_sum"])
        assert np.array_equal(got["sum"][~ok], sr["nll_sum"][~ok])
        assert (np.abs(got["sum"][ok] - sr["nll_sum"][ok]) <= sr["b_nll_sum"][ok]).all()
        assert parts["n"].sum() == sr["n"].sum()
    assert fin.any()
    rowbad = R.nonfinite_rows(np.asarray(x, dtype=np.float64))
    xh, h = Gm.one_hot_rows(case)
    for mode in R.COMBINES:
        nonf, _ = Gm.mixture_restated(None, rowbad, w, case.draws, mode)
        assert np.array_equal(nonf, mr[mode]["nonfinite"]), mode
        hr = Gm.one_hot_reference(case, mode)
        assert not hr["nonfinite"].any()
        sets = Gm.finite_sets(case, mode)
        assert np.array_equal(sets, hr["logp"] > -np.inf), mode       # (a NaN is not > -inf)
        assert not np.isnan(hr["logp"]).any() and sets.any(-1).sum() > 0


# ------------------------------------------------------------- 4. the literal inputs
def test_the_three_facts_the_integer_rows_rest_on():
    assert np.exp(np.float32(0.0)) == np.float32(1.0) and np.log(np.float32(1.0)) == 0.0
    assert 1.0 + float(np.exp(np.float32(-200.0))) == 1.0
    top = np.float32(4096.0) + np.log(np.float32(2.0)).astype(np.float32)
    assert float(top) - 4096.0 == Gm.TIE_NLL              # 1 ulp of logf is far from the rounding
    assert abs(np.log(2.0) / 2.0 ** -11 - 1420) < 0.45


@pytest.mark.parametrize("case", Gm.P, ids=Gm.case_id)
def test_the_plants_give_their_literal_answers_through_the_emulation(case):
    x, lab, nll, wrong = Gm.integer_rows(case)
    assert ((lab >= 0) & (lab < case.C)).all() and (nll == np.round(nll * 2048) / 2048).all()
    got = R.score_emulate(x, lab)
    assert np.array_equal(got["nll_sum"], nll.sum(-1))
    assert np.array_equal(got["n_wrong"], wrong.sum(-1))
    assert (np.asarray(got["n"]) == case.B).all() and not np.asarray(got["n_nonfinite"]).any()
    keep = np.ones(case.B, bool)                            # fp64 log 2 is not fl32's: no tie rows
    keep[[p[1] for p in case.plants if p[0] == "tie"]] = False
    got = R.score_reference(x[:, :, keep], lab[keep])
    assert np.array_equal(got["nll_sum"], nll[:, :, keep].sum(-1))
    assert np.array_equal(got["n_wrong"], wrong[:, :, keep].sum(-1))
    R.check_scores(R.score_emulate(x, lab), R.score_reference(x, lab), Gm.case_id(case))
    for p in case.plants:                                  # the lower class of a tie wins
        if p[0] == "tie":
            assert wrong[:, :, p[1]].all() == (p[4] == p[3]) and (nll[:, :, p[1]] == Gm.TIE_NLL).all()
            assert (x[:, :, p[1]] == Gm.TOP).sum() == 2 * x.shape[0] * x.shape[1]
    xh, h = Gm.one_hot_rows(case)
    w = Gm.weights(case)
    for mode in R.COMBINES:
        em = R.mixture_emulate(xh, w, case.draws, mode)
        sets = Gm.finite_sets(case, mode)
        assert np.array_equal(em["logp"] > -np.inf, sets) and not np.isnan(em["logp"]).any()
        assert (em["expected_entropy"] == 0).all()
        assert all(t["expected_entropy_sum"] == 0 and t["n"] == case.B for t in em["totals"])
        R.check_mixture(em, Gm.one_hot_reference(case, mode), (Gm.case_id(case), mode))
    if case.draws > 1 and case.comps > 1:                  # h depends on the component somewhere
        assert (h[0] != h[case.draws + 1]).any() and (h[0] == h[case.draws]).all()


# ------------------------------------------------------------- 5. the break table
def _bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def test_every_break_changes_an_expected_answer_of_P():
    changed = {b: set() for b in Gm.BREAKS}
    for case in Gm.P:
        cid = Gm.case_id(case)
        x, lab, nll, wrong = Gm.integer_rows(case)
        one, zero = np.ones(nll.shape, bool), np.zeros(nll.shape, bool)
        for grid in case.grids:
            good, parts = Gm.score_expected(case, grid, nll, one, zero, wrong)
            for b in ("combine_stride64", "combine_one_trip"):
                if parts.shape[1] > 64 and Gm.combine(parts, breaks=(b,)).tobytes() != good.tobytes():
                    changed[b].add((cid, grid))
            if Gm.score_expected(case, grid, nll, one, zero, wrong,
                                 breaks=("bstride_no_ipb",))[0].tobytes() != good.tobytes():
                changed["bstride_no_ipb"].add((cid, grid))
        for b in ("dispatch_up", "dispatch_down"):
            cov = Gm.covered(case.C, (b,))
            if not cov.all():
                xm = np.array(x)
                xm[..., ~cov] = -np.inf                    # what no thread owns is never read
                e0, e1 = R.score_emulate(x, lab), R.score_emulate(xm, lab)
                if any(not np.array_equal(e0[k], e1[k]) for k in e0):
                    changed[b].add(cid)
        w = Gm.weights(case)
        rx, _, _ = Gm.random_inputs(case)
        rowbad = R.nonfinite_rows(np.asarray(rx, dtype=np.float64))
        for b in ("prefetch_c_plus_1", "skip_le"):
            for mode in R.COMBINES:
                if not np.array_equal(Gm.finite_sets(case, mode, (b,)), Gm.finite_sets(case, mode)):
                    changed[b].add((cid, mode))
        for b in ("bad_skipped_counted", "prefetch_c_plus_1"):
            if not np.array_equal(Gm.mixture_restated(None, rowbad, w, case.draws, "arithmetic",
                                                      (b,))[0],
                                  Gm.mixture_restated(None, rowbad, w, case.draws, "arithmetic")[0]):
                changed[b].add((cid, "nonfinite"))
    # the waves' order shows in the sum's bits only: the rounding-sensitive random case
    case = Gm.ROUNDING
    x, lab, _ = Gm.random_inputs(case)
    sr, _ = Gm.references(case)
    inr = (lab >= 0) & (lab < case.C)
    bad = R.nonfinite_rows(np.asarray(x, dtype=np.float64)) & inr[None, None, :]
    for nw in Gm.COMBINE_NW:
        good, parts = Gm.score_expected(case, nw, sr["nll"], sr["ok"], bad, np.zeros(bad.shape, bool))
        rev = Gm.combine(parts, breaks=("waves_reversed",))
        assert np.array_equal(rev["n"], good["n"])
        if _bits(rev["sum"]) != _bits(good["sum"]):
            changed["waves_reversed"].add(nw)
    # one class group below the bound selects a larger instance that owns the same classes in
    # the same threads, trips and slots: no output can tell — the one variant without an answer
    assert not changed.pop("dispatch_down")
    assert all(Gm.covered(C, ("dispatch_down",)).all() for C in range(1, Gm.MAX_CLASSES + 1))
    for b, where in changed.items():
        assert where, b
    assert {c for c in changed["dispatch_up"]} == {Gm.case_id(c) for c in Gm.P
                                                   if c.C in (1025, 1028, 2049, 2052)}
    # one wave's partials alone (nw <= 64) add up the same either way
    assert changed["waves_reversed"] and min(changed["waves_reversed"]) > 64


# ------------------------------------------------------------- 6. the cap
@pytest.mark.parametrize("case", Gm.P, ids=Gm.case_id)
def test_check_mixture_leaves_out_at_most_the_cap(case):
    _, mr = Gm.references(case)
    for mode in R.COMBINES:
        assert R.unchecked_share(mr[mode]) <= R.MAX_EXCLUDED, mode
        assert R.unchecked_share(mr[mode]) <= R.excluded_share(mr[mode])
        hr = Gm.one_hot_reference(case, mode)
        assert R.unchecked_share(hr) == 0.0, mode
