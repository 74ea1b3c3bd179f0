"""tests/summary_reduce_ref.py on the CPU: the restated reduction equals the
plain definition of a summary at every grid, every element of every sweep is
owned exactly once, the planted ties reach every level of the tree in both
argument orders (literal sets per case), what the older GPU ties reach is
recorded exactly, and every wrong reduction of the break table that can change
a value does so on a planted case."""
import functools
import math

import numpy as np
import pytest

import chain_diag_ref as DR
import layers_ref as LR
import summary_reduce_ref as S

F = np.float32
GRIDS = (1, 2, 3, 7, 255, 256, 257, 511, 512, 513, 1024, 2048)
# the GPU cases of tests/test_gpu_summary_reduce.py: (n, workgroups)
N_MID = 2 * 257 * 1024 + 1027
N_BIG = 2 * 2048 * 1024 + 7
ESS_CASES = ((1025, 2), (3 * 1024 + 5, 3), (N_MID, 257), (N_BIG, 2048))
SIZES = (1, 3, 4, 5, 1023, 1025, 3 * 1024 + 5, N_MID, N_BIG)
BIG_SEGMENTS = S.big_table().segments


def names(levels, orders="ab"):
    return {f"{lv}:{o}" for lv in levels for o in orders}


BFLY = tuple(f"bfly{o}" for o in S.OFFSETS)
FBFLY = tuple(f"fbfly{o}" for o in S.OFFSETS)
# the planted pairs that exist per case, by name: "<level>:a" has its lower index in combine's
# first argument, "<level>:b" in its second
PLANTED = {
    # one trip: no lane, wave or workgroup can own a later trip, so no "b"
    (1025, 2): {"group"} | names(BFLY + ("wave",), "a"),
    # workgroup 0 alone has a second (guarded, 5-element) trip
    (3 * 1024 + 5, 3): {"group", "guarded", "bfly32:b", "fbfly2:a", "fbfly1:a"}
    | names(BFLY + ("wave",), "a"),
    (N_MID, 257): {"group", "guarded", "lane:a"}
    | names(BFLY + ("wave", "fin_trip2") + FBFLY + ("fwave",)),
    (N_BIG, 2048): {"group", "guarded", "lane:a"}
    | names(BFLY + ("wave", "fin_trip2", "fin_trip8") + FBFLY + ("fwave",)),
}


def plain(values, idx, deg, nonf, thr, maximum):
    """A summary by its definition."""
    ev = ~deg & ~nonf
    x = values[ev]
    out = {"n_eval": int(ev.sum()), "n_degenerate": int(deg.sum()), "n_nonfinite": int(nonf.sum())}
    cmp = np.greater if maximum else np.less
    out["hits"] = [int(cmp(x, F(t)).sum()) for t in thr]
    if x.size:
        ext = x.max() if maximum else x.min()
        out["ext"], out["arg"] = float(ext), int(idx[np.flatnonzero(ev & (values == ext))[0]])
    else:
        out["ext"], out["arg"] = 0.0, -1
    out["sum"] = math.fsum(x.astype(np.float64).tolist())
    out["sum_abs"] = float(np.abs(x.astype(np.float64)).sum())
    return out


def random_case(seed, size):
    """Values with many duplicates (63 levels), 2 % degenerate, 2 % non-finite."""
    rng = np.random.default_rng(seed)
    v = (rng.integers(1, 64, size) / 8).astype(F)
    u = rng.random(size)
    return v, u < 0.02, (u >= 0.02) & (u < 0.04)


def check_against_plain(r, values, idx, deg, nonf, thr, maximum):
    want = plain(values, idx, deg, nonf, thr, maximum)
    got = r.summary
    for f in ("n_eval", "n_degenerate", "n_nonfinite", "arg"):
        assert int(got[f]) == want[f], f
    assert got["hits"].tolist() == want["hits"] and float(got["ext"]) == want["ext"]
    assert abs(float(got["sum"]) - want["sum"]) <= want["n_eval"] * 2.0 ** -52 * want["sum_abs"]
    # the partials: every element in exactly one, their extremes bound the summary's
    p = r.partials
    for f in ("n_eval", "n_degenerate", "n_nonfinite"):
        assert int(p[f].sum()) == want[f], f
    assert p["hits"].sum(axis=0).tolist() == want["hits"]
    if want["n_eval"]:
        on = p["n_eval"] > 0
        best = p["ext"][on].max() if maximum else p["ext"][on].min()
        assert float(best) == want["ext"] and int(p["arg"][on & (p["ext"] == best)].min()) == want["arg"]
    assert (p["arg"][p["n_eval"] == 0] == S.I64_MAX).all()


# ------------------------------------------------- reduce == the definition
@pytest.mark.parametrize("n", SIZES)
def test_every_element_is_owned_once_and_reduce_is_the_plain_definition(n):
    """Every grid (as the kernels could be launched: at most one workgroup per
    block iteration is what the host picks, but the restatement holds for any),
    both Extreme<true> and Extreme<false>.  A lane's program order ascends in
    the element index (the header's premise for the strict comparison)."""
    v, deg, nonf = random_case(n, n)
    for grid in GRIDS:
        own = S.owner(n, grid)
        assert (own["count"] == 1).all() and (own["idx"] == np.arange(n)).all()
        assert (own["wg"] < grid).all() and (own["wg"] >= 0).all() and (own["thread"] < 256).all()
        lane = own["wg"] * 256 + own["thread"]
        order = np.lexsort((own["seq"], lane))
        same = lane[order][1:] == lane[order][:-1]
        assert (np.diff(order)[same] > 0).all()
        # the guarded iteration is the last block iteration, and only if it is not a whole one
        g0 = 1024 * ((n >> 2) // 256)
        assert (np.flatnonzero(own["guarded"]) == np.arange(g0, n)).all()
        maximum = grid % 2 == 1
        thr = (0.5, 4.0, 7.875)                      # the last is the largest value: never beyond
        r = S.reduce(v, own, maximum=maximum, thresholds=thr, degenerate=deg, nonfinite=nonf)
        check_against_plain(r, v, own["idx"], deg, nonf, thr, maximum)
        if n <= 5:
            none = np.ones(n, bool)                  # nothing evaluated: the empty conventions
            e = S.reduce(v, own, maximum=maximum, thresholds=thr, degenerate=none, nonfinite=~none)
            assert (int(e.summary["n_eval"]), float(e.summary["ext"]), int(e.summary["arg"]),
                    float(e.summary["sum"])) == (0, 0.0, -1, 0.0)


def test_big_table_has_the_three_misalignments():
    tab = S.big_table()
    big = [(o, m) for o, m in tab.segments if m >= 600 * 1024]
    assert len(big) == 3 and [o % 4 for o, _ in big] == [1, 2, 3]
    assert [LR.split(o, m)[0] for o, m in big] == [3, 2, 1]            # heads
    assert [LR.split(o, m)[2] for o, m in big] == [0, 3, 3]            # tails
    part = [int(own["part"].sum()) for own in S.owner_layers(tab.segments, 1024)]
    assert part == [1, 600, 1, 600, 601]                               # idle workgroups at 1024


@pytest.mark.parametrize("grid", [2, 3, 512, 1024])
@pytest.mark.parametrize("name", ["l", "a", "big"])
def test_layers_elements_are_owned_once_as_classify_says(name, grid):
    segs = {"l": LR.table_l().segments, "a": LR.table_a().segments, "big": list(BIG_SEGMENTS)}[name]
    owns = S.owner_layers(segs, grid)
    n = max(o + m for o, m in segs)
    c = LR.classify(segs, n, grid) if name != "big" or grid <= 3 else None
    for i, ((o, m), own) in enumerate(zip(segs, owns)):
        assert (own["count"] == 1).all() and (own["idx"] == o + np.arange(m)).all()
        h, nbody, tail = LR.split(o, m)
        assert ((own["kind"] == 0).sum(), (own["kind"] == 1).sum(), (own["kind"] == 2).sum()) == \
            (h, 4 * nbody, tail)
        lane = own["wg"] * 256 + own["thread"]
        order = np.lexsort((own["seq"], lane))
        same = lane[order][1:] == lane[order][:-1]
        assert (np.diff(order)[same] > 0).all()       # head first on thread 0, tail last on thread 64
        if c is None:
            continue
        per = [np.bincount(own["wg"][own["kind"] == k], minlength=grid) for k in range(3)]
        for w in range(grid):
            k = c[w, i]
            assert (per[0][w], per[1][w], per[2][w]) == (k["head"], k["body"], k["tail"]), (i, w)
            assert own["part"][w] == k["part"]
    v, deg, nonf = random_case(grid, segs[1][1])
    r = S.reduce(v, owns[1], maximum=True, thresholds=(1, 2, 3), degenerate=deg, nonfinite=nonf)
    check_against_plain(r, v, owns[1]["idx"], deg, nonf, (1, 2, 3), True)


# ------------------------------------------------------------ planted ties
def plant(n, i, j, maximum):
    """Distinct values with the strict extreme at i and j."""
    v = (1.0 + np.arange(n) % 4093 / 8192).astype(F)
    v[i] = v[j] = F(3.0) if maximum else F(0.5)
    return v


def level_of(name):
    return None if ":" not in name else tuple(name.split(":"))


def pair_reduce(own, pos_i, pos_j, maximum, variants=((),)):
    """The reduction of the two elements alone, both at the extreme value:
    whatever else a sweep holds, a strict extreme's tie meets these two only."""
    sub = S.sub_owner(own, [pos_i, pos_j])
    v = np.full(2, 3.0 if maximum else 0.5, F)
    z = np.zeros(2, bool)
    return S.reduce_variants(v, sub, maximum=maximum, thresholds=(0.5, 1, 3), degenerate=z,
                             nonfinite=z, variants=variants)


@functools.lru_cache(maxsize=None)
def traces(n, grid):
    own = S.owner(n, grid)
    z = np.zeros(n, bool)
    out = {}
    for name, i, j in S.ties_whole(n, grid):
        r = pair_reduce(own, i, j, False)[()]
        assert int(r.summary["arg"]) == i and r.summary["hits"].tolist() == [0, 2, 2]
        assert len(r.trace) == 1
        if n < 4096:        # the whole sweep around the pair changes nothing of this
            full = S.reduce(plant(n, i, j, False), own, maximum=False, thresholds=(0.5, 1, 2),
                            degenerate=z, nonfinite=z)
            assert full.trace == r.trace and int(full.summary["arg"]) == i
            assert full.summary["hits"].tolist() == [0, 2, n]
        out[name] = (next(iter(r.trace)), i, j, bool(own["guarded"][i]), i // 4 == j // 4)
    return out


@pytest.mark.parametrize("n,grid", ESS_CASES)
def test_planted_ties_reach_every_level_in_both_orders(n, grid):
    got = traces(n, grid)
    assert set(got) == PLANTED[n, grid]
    for name, (label, i, j, guarded, same_group) in got.items():
        if level_of(name):
            assert label == level_of(name), name
    assert got["group"][0] == ("lane", "a") and got["group"][4]
    if "guarded" in got:
        assert got["guarded"][3]                       # the lower index ran in the guarded iteration
    if "lane:a" in got:
        assert not got["lane:a"][4]                    # two trips of one lane


def test_the_two_large_cases_together_reach_every_label():
    both = {t[0] for case in ((N_MID, 257), (N_BIG, 2048)) for t in traces(*case).values()}
    levels = ("lane",) + BFLY + ("wave", "fin_trip2", "fin_trip8") + FBFLY + ("fwave",)
    assert both == {(lv, o) for lv in levels for o in "ab"} - {("lane", "b")}
    # ("lane", "b") does not exist: a lane's elements ascend and its comparison is strict
    assert set(lv for lv, _ in both) <= set(S.LEVELS)


def test_finalize_thread_with_an_empty_first_partial_and_idle_workgroups():
    n, grid = N_MID, 257
    own = S.owner(n, grid)
    v, _, _ = random_case(3, n)
    deg = own["wg"] == 0                                # workgroup 0 evaluates nothing
    r = S.reduce(v, own, maximum=False, thresholds=(1, 2, 3), degenerate=deg, nonfinite=~deg & False)
    assert {"fin_empty_then_value", "empty_partial"} <= r.marks
    assert int(r.partials["n_eval"][0]) == 0 and int(r.partials["n_eval"][256]) > 0
    check_against_plain(r, v, own["idx"], deg, np.zeros(n, bool), (1, 2, 3), False)
    # a workgroup with no iteration at all: table L at 512 workgroups (its largest body is 4 iterations)
    tab = LR.table_l()
    owns = S.owner_layers(tab.segments, 512)
    assert all((~o["part"]).sum() >= 508 for o in owns)
    m = tab.segments[7][1]
    z = np.zeros(m, bool)
    r = S.reduce(plant(m, 5, 9, True), owns[7], maximum=True, thresholds=(1, 2, 3), degenerate=z,
                 nonfinite=z)
    assert "idle_workgroup" in r.marks and int(r.summary["n_eval"]) == m
    # an idle workgroup's 256 empty lanes, walked through block_combine, are the empty partial
    d = S.reduce(plant(m, 5, 9, True), owns[7], maximum=True, thresholds=(1, 2, 3), degenerate=z,
                 nonfinite=z, dense=True)
    for f in r.summary:
        assert np.array_equal(d.summary[f], r.summary[f]) and np.array_equal(d.partials[f], r.partials[f])
    assert (r.partials["n_eval"] == 0).sum() >= 508 and d.trace == r.trace


LAYER_TIES = {
    # table L: heads, tails and short segments; `big` (index 7, 825 groups) spans four workgroups
    ("l", 3): {"head-body": {("bfly1", "a")}, "tail-body": {("bfly1", "b")},
               "head-tail": {("wave", "a")}, "body-group": {("lane", "a")},
               "two-workgroups": {("fbfly1", "b")}},
    ("l", 512): {"head-body": {("bfly1", "a")}, "tail-body": {("bfly1", "b")},
                 "head-tail": {("wave", "a")}, "body-group": {("lane", "a")},
                 "two-workgroups": {("fbfly1", "b")}},
    # table A at 3 workgroups: a rotation that wraps (lower index in workgroup 2, higher in 0)
    ("a", 3): {"body-group": {("lane", "a")},
               "two-workgroups": {("fbfly1", "a"), ("fbfly1", "b"), ("fbfly2", "b")}},
}


@pytest.mark.parametrize("name,grid", sorted(LAYER_TIES))
def test_layers_ties_reach_head_tail_and_rotated_workgroups(name, grid):
    tab = LR.table_l() if name == "l" else LR.table_a()
    owns = S.owner_layers(tab.segments, grid)
    got = {}
    for nm, s, i, j in S.ties_layers(tab.segments, grid, owns):
        o, m = tab.segments[s]
        z = np.zeros(m, bool)
        r = S.reduce(plant(m, i - o, j - o, True), owns[s], maximum=True, thresholds=(1, 2, 3),
                     degenerate=z, nonfinite=z)
        assert int(r.summary["arg"]) == i and len(r.trace) == 1
        got.setdefault(nm, set()).update(r.trace)
        own = owns[s]
        if nm == "two-workgroups":
            assert own["wg"][i - o] != own["wg"][j - o] and own["wg"][i - o] == s % grid
        if nm.startswith("head"):
            assert own["kind"][i - o] == 0 and own["thread"][i - o] == 0
        if nm.endswith("tail") or nm == "tail-body":
            assert own["kind"][j - o] == 2 and own["thread"][j - o] == 64
    assert got == LAYER_TIES[name, grid]
    if (name, grid) == ("a", 3):
        assert any(nm == "two-workgroups" and s % 3 for nm, s, _, _ in S.ties_layers(tab.segments, 3))


# ------------------------------------------- what the older GPU ties reach
def test_what_the_existing_ess_and_diag_ties_reach():
    """tests/test_gpu_chain_ess.py plants its minimum at two random positions
    per (K, n) and runs at grid_blocks {its own, 0, 3}; tests/test_gpu_chain_diag.py
    plants one pair (i, i + n/2) at n = 1,000,003.  Their levels, exactly: 10
    of the 33 (level, order) labels, no finalize trip and no finalize wave for
    ESS (at most 18 workgroups), and for the diag pair the finalize waves with
    the lower index first at every geometry: no label that needs the
    `b.arg < a.arg` clause above a butterfly.  (A butterfly meets "b" orders
    within one trip too: lanes 1 and 2 meet in lane 0's step 1 as {0, 2} against
    {1, 3}.)  Recorded so that DESIGN.md's table cannot drift."""
    from test_gpu_chain_ess import SIZES as ESS_SIZES, report_case
    reached = {}
    for n, g in ESS_SIZES:
        cg = (n + 3) // 4 + 3
        for K_ in (1, 2, 5, 8):
            i, j = sorted(report_case(77 * K_ + n, K_, n, cg)[5])
            for gb in sorted({g, 0, 3}):
                grid = S.grid_ess(n, gb, 256)
                assert grid == S.grid_ess(n, gb, 304) <= 18
                own = S.owner(n, grid)
                z = np.zeros(n, bool)
                r = S.reduce(plant(n, i, j, False), own, maximum=False, thresholds=(1, 2, 3),
                             degenerate=z, nonfinite=z)
                reached.setdefault(n, set()).update(r.trace)
    assert reached == {
        24: {("bfly1", "a"), ("bfly1", "b"), ("bfly2", "a")},
        1023: {("bfly1", "b"), ("bfly2", "b"), ("wave", "a")},
        1025: {("bfly1", "b"), ("wave", "a")},
        17411: {("bfly16", "a"), ("fbfly1", "a"), ("fbfly1", "b"), ("fbfly2", "b"),
                ("fbfly4", "a"), ("wave", "a")},
    }
    every = set().union(*reached.values())
    assert not any(lv.startswith("fin_trip") for lv, _ in every)
    # the diag pair
    n, K_ = 1_000_003, 3
    m1, var, cg = DR.make_case(7, K_, n)
    m2 = DR.to_mode(m1, var, DR.VAR_RAW_MOMENTS, 1.2, K_, 4 * cg, n)
    rh = DR.chain_diag_f32(m1, m2, chains=K_, chain_groups=cg, n=n, var_mode=DR.VAR_RAW_MOMENTS,
                           ratio=1.2, inv_ratio=0.0, count=6)[2]
    i = int(np.nanargmax(rh))
    i, j = sorted((i, (i + n // 2) % n))
    z = np.zeros(n, bool)
    got = {}
    for cus in (256, 304):
        for bpc in (1, 2, 8):
            grid = S.grid_diag(n, bpc, cus)
            r = S.reduce(plant(n, i, j, True), S.owner(n, grid), maximum=True, thresholds=(1, 2, 3),
                         degenerate=z, nonfinite=z)
            got[cus, bpc] = (grid, sorted(r.trace))
    assert (i, j) == (12568, 512569)
    assert got == {(256, 1): (256, [("fwave", "a")]), (256, 2): (512, [("fwave", "a")]),
                   (256, 8): (977, [("fwave", "a")]), (304, 1): (304, [("fwave", "a")]),
                   (304, 2): (608, [("fwave", "a")]), (304, 8): (977, [("fwave", "a")])}


# --------------------------------------------------------------- the breaks
def test_every_break_that_can_change_a_value_changes_one_on_a_planted_case():
    """Each wrong reduction, applied to the restatement: at least one planted
    pair reports another arg, or the summary's fp64 sum has other bits.

    `same_order` (wave_combine forming combine(s, o) in both partners) is the
    exception, and the test proves why: thread 0 of a wave never takes the
    combine(o, s) branch (no offset bit is set in lane 0), the partner it reads
    at step `off` is lane `off`, which took the combine(s, o) branch at every
    earlier step, and only lane 0 of a wave is read afterwards.  So that break
    changes no stored value, in any field, on any input."""
    variants = [()] + [(b,) for b in S.BREAKS]
    changed = {b: set() for b in S.BREAKS}

    def compare(n, name, rs):
        good = rs[()]
        for b in S.BREAKS:
            bad = rs[b,]
            if int(bad.summary["arg"]) != int(good.summary["arg"]):
                changed[b].add((n, name, "arg"))
            if S.sum_bits(bad.summary["sum"]) != S.sum_bits(good.summary["sum"]):
                changed[b].add((n, name, "sum"))
            if b == "same_order":
                for f in good.summary:
                    assert np.array_equal(bad.summary[f], good.summary[f]), (name, f)
                    assert np.array_equal(bad.partials[f], good.partials[f]), (name, f)

    for n, grid in ((3 * 1024 + 5, 3), (N_MID, 257)):
        own = S.owner(n, grid)
        for name, i, j in S.ties_whole(n, grid):
            rs = pair_reduce(own, i, j, False, variants)
            assert int(rs[()].summary["arg"]) == i
            compare(n, name, rs)
        # the sum: values over 60 binades, so that the order of the fp64 additions shows (fp32
        # values of one magnitude add up exactly in fp64 in any order)
        rng = np.random.default_rng(n)
        v = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-30, 31, n)).astype(F)
        z = np.zeros(n, bool)
        compare(n, "sweep", S.reduce_variants(v, own, maximum=True, thresholds=(1, 2, 3),
                                              degenerate=z, nonfinite=z, variants=variants))
    assert not changed.pop("same_order")
    kinds = {b: {k for _, _, k in hits} for b, hits in changed.items()}
    assert kinds == {"first_wins": {"arg"}, "last_wins": {"arg"}, "fin_stride64": {"sum"},
                     "fin_one_trip": {"arg", "sum"}, "waves_reversed": {"sum"}}
    first = {nm for n, nm, k in changed["first_wins"] if n == N_MID}
    last = {nm for n, nm, k in changed["last_wins"] if n == N_MID}
    assert first == {nm for nm in PLANTED[N_MID, 257] if nm.endswith(":b")}
    assert last == {nm for nm in PLANTED[N_MID, 257] if nm.endswith(":a") and nm != "lane:a"}
    # one trip only: the partials past 256 are lost, whichever pair was planted there
    assert {nm for n, nm, k in changed["fin_one_trip"] if k == "arg"} == {"fin_trip2:b"}
    assert all(n == N_MID for n, _, _ in changed["fin_one_trip"])


def test_the_gpu_inputs_show_the_order_of_the_fp64_additions():
    """The values tests/test_gpu_summary_reduce.py feeds the whole-vector units
    span enough binades that another order of the same additions gives other
    bits: with the waves taken 3..0, 75 of 257 workgroups' partial sums differ
    in the ESS case (its summary's sum happens to round to the same value) and
    the summary's sum differs in the R-hat case, so the device's bit-equal
    partials and sums do pin the documented order at both stages."""
    import test_gpu_summary_reduce as G
    seen = {}
    for kind, case, maximum, grid in (("ess", G.ess_case(N_MID), False, 257),
                                      ("diag", G.diag_case(N_MID), True, 256)):
        v, deg, nonf = case[3]
        rs = S.reduce_variants(v, S.owner(N_MID, grid), maximum=maximum, thresholds=(1, 2, 3),
                               degenerate=deg, nonfinite=nonf, variants=[(), ("waves_reversed",)])
        good, bad = rs[()], rs["waves_reversed",]
        moved = int((S.sum_bits(good.partials["sum"]) != S.sum_bits(bad.partials["sum"])).sum())
        seen[kind] = (moved, bool(S.sum_bits(good.summary["sum"]) != S.sum_bits(bad.summary["sum"])))
        assert int(deg.sum()) > 1000 and int(nonf.sum()) > 1000
    # ESS (40 binades): the workgroups' sums move; R-hat (20 binades): they are exact, the
    # finalize workgroup's additions are not, and the summary's sum moves
    assert seen == {"ess": (75, False), "diag": (0, True)}
