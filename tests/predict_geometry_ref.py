"""The launch geometry of bdl_predict (bdl_predict.hip) restated on the host —
TEST INFRASTRUCTURE ONLY: which of the ten instances a class count selects, the
grid and the partials per group of a grid_blocks (0 by the host code's formula),
a literal walk of the sweep's loops (group, rotated workgroup, grid-strided
example, wave), the owner of every class (thread, wave, lane, trip, slot, the
masked tail group), the combine's quarters, the set of path labels a case
reaches, table P — small shapes that together reach every label — and its
inputs.  Nothing is imported from bayesdll_amd and nothing from torch.

The kernels, in the words the walk follows.  A workgroup has 256 threads (4
waves).  classes <= 256: WAVE, one wave per example (TPI = 64 threads per
example, IPB = 4 examples per workgroup iteration); above: one workgroup per
example (TPI = 256, IPB = 1).  Thread ti of an example owns the class groups
ti + TPI * u, u < NT (classes 4 q .. 4 q + 3 of group q; a class >= C is
masked).  NT is 1 for WAVE and the smallest of 1, 2, 4, 8 with
ceil(C / 4) <= 256 NT otherwise; VEC = (C % 4 == 0).  Workgroup blk takes, of
group g, the examples r * IPB (+ wave), + grid * IPB, ... with
r = (blk - g) mod grid, skips the group if r * IPB >= B, and writes the partial
g * nw + r, nw = min(grid, ceil(B / IPB)).  grid_blocks = 0:
grid = max(1, min(min(ceil(B / IPB), 1024) * G, 4 CUs', 1024)).  Lane j of a
wave owns bin j.  The combine's wave w adds the partials
[w nw / 4, (w + 1) nw / 4) of a group."""
from __future__ import annotations

import collections
import functools

import numpy as np

import predict_ref as R

BLOCK, WAVES, WAVE_CLASSES, MAX_CLASSES, MAX_GRID, MAX_BINS = 256, 4, 256, 8192, 1024, 64
CUS = 256   # the MI355X's; the default grids used here are below 4 x 64 and do not depend on it

INSTANCES = tuple((nt, vec, wave) for nt, wave in ((1, True), (1, False), (2, False), (4, False),
                                                   (8, False)) for vec in (True, False))


def instance(C):
    """(NT, VEC, WAVE) of launch_by_classes."""
    assert 1 <= C <= MAX_CLASSES
    q = (C + 3) // 4
    vec = C % 4 == 0
    if C <= WAVE_CLASSES:
        return 1, vec, True
    for nt in (1, 2, 4):
        if q <= nt * BLOCK:
            return nt, vec, False
    return 8, vec, False


def inst_label(inst):
    nt, vec, wave = inst
    return "inst:{}:NT{}:{}".format("wave" if wave else "wg", nt, "vec" if vec else "elem")


def launch(C, G, B, grid_blocks, cus=CUS):
    """(grid, nw, IPB) as bdl_predict computes them."""
    assert 0 <= grid_blocks <= MAX_GRID
    ipb = WAVES if C <= WAVE_CLASSES else 1
    per_group = (B + ipb - 1) // ipb
    grid = grid_blocks
    if grid == 0:
        want = min(per_group, MAX_GRID) * G
        grid = max(1, min(min(want, cus * 4), MAX_GRID))
    return grid, min(grid, per_group), ipb


def trips_used(C):
    """Trips of an example that hold a class group."""
    tpi = 64 if instance(C)[2] else BLOCK
    return ((C + 3) // 4 + tpi - 1) // tpi


Owner = collections.namedtuple("Owner", "thread wave lane trip slot tail")


def owner(C, c):
    """Who holds class c of an example: the thread of the example (wave mode:
    the lane), its wave in the workgroup (None in wave mode: the example's),
    its lane, the trip u, the slot j, and whether c's class group is the
    masked partial one."""
    assert 0 <= c < C
    wave_mode = instance(C)[2]
    tpi = 64 if wave_mode else BLOCK
    q, j = divmod(c, 4)
    u, ti = divmod(q, tpi)
    return Owner(ti, None if wave_mode else ti // 64, ti % 64, u, j,
                 C % 4 != 0 and q == (C + 3) // 4 - 1)


def walk(C, G, B, grid_blocks, cus=CUS):
    """The sweep's loops literally.  Returns (where: {(g, b): (r, blk, trip,
    wave)}, count [G, nw]: examples per partial, idle: whether a wave of a
    participating workgroup takes no example).  Asserts that every example is
    taken once and every partial g * nw + r, r < nw, is written once."""
    grid, nw, ipb = launch(C, G, B, grid_blocks, cus)
    where, written = {}, set()
    count = np.zeros((G, nw), np.int64)
    idle = False
    for g in range(G):
        for blk in range(grid):
            r = (blk + grid - g % grid) % grid
            if r * ipb >= B:
                continue
            assert r < nw and (g, r) not in written
            written.add((g, r))
            for w in range(ipb):
                b, trip = r * ipb + w, 0
                if b >= B:
                    idle = True
                while b < B:
                    assert (g, b) not in where
                    where[(g, b)] = (r, blk, trip, w)
                    count[g, r] += 1
                    b, trip = b + grid * ipb, trip + 1
    assert len(where) == G * B
    assert written == {(g, r) for g in range(G) for r in range(nw)}
    return where, count, idle


def combine(nw):
    """(quarter [nw]: the wave whose quarter holds partial i (-1: none),
    times [nw]: how often i is taken, empty: the waves without a partial)."""
    quarter, times = np.full(nw, -1), np.zeros(nw, np.int64)
    empty = []
    for w in range(WAVES):
        lo, hi = w * nw // WAVES, (w + 1) * nw // WAVES
        if lo == hi:
            empty.append(w)
        for i in range(lo, hi):
            quarter[i] = w
            times[i] += 1
    return quarter, times, empty


# ------------------------------------------------------------------ the labels
WHAT = ("am", "pred", "label")      # a member row's argmax, the mixture's pred, the label's class
TIES = ("slots", "lanes", "waves", "trips")
BIN_COUNTS = (1, 2, 15, 16, 33, 64)

ALL_LABELS = frozenset(
    [inst_label(i) for i in INSTANCES]
    + ["{}:NT{}:{}".format(w, nt, t) for w in WHAT
       for nt, ts in ((2, ("trip0", "last")), (4, ("trip0", "mid", "last")),
                      (8, ("trip0", "mid", "last"))) for t in ts]
    + ["{}:{}".format(w, s) for w in WHAT for s in ("wave0", "wave3", "lane63", "tail")]
    # an exact two-way tie, the lower class: in the same thread; on a higher lane of the same
    # wave; in another wave; in trip 0 of a higher thread than the later trip of the other
    + ["tie:{}:{}".format(w, t) for w in ("am", "pred") for t in TIES]
    + ["nw:1", "nw:2", "nw:3", "nw:%4", "nw:259", "nw:1024",
       "nw<grid:G>1", "G>grid", "wave:B%4=1", "wave:B%4=2", "wave:B%4=3", "trip2", "trip3",
       "nonfinite:shares_workgroup",   # wave mode: beside finite examples in one iteration
       "nonfinite:then_finite"]        # the next example of the same wave / workgroup is finite
    + ["bins:{}".format(n) for n in BIN_COUNTS]
    + ["bin:lane>=15", "bin:lane32", "bin:lane63"]   # that lane's bin is not empty
    + ["label:-1", "label:C", "label:C-1:tail", "label:2^40"])


def spot_labels(C, what, c):
    """Where class c lies, as labels of `what`."""
    nt, _, wave_mode = instance(C)
    o = owner(C, c)
    out = set()
    if nt > 1:
        last = trips_used(C) - 1
        out.add("{}:NT{}:{}".format(what, nt, "trip0" if o.trip == 0 else
                                    "last" if o.trip == last else "mid"))
    if not wave_mode and o.wave in (0, 3):
        out.add("{}:wave{}".format(what, o.wave))
    if wave_mode and o.lane == 63:
        out.add("{}:lane63".format(what))
    if o.tail:
        out.add("{}:tail".format(what))
    return out


def tie_labels(C, what, c1, c2):
    """How the tie between classes c1 < c2 is decided."""
    assert c1 < c2
    wave_mode = instance(C)[2]
    a, b = owner(C, c1), owner(C, c2)
    out = set()
    if a.thread == b.thread:
        out.add("tie:{}:slots".format(what))
        return out
    if (wave_mode or a.wave == b.wave) and a.lane > b.lane:
        out.add("tie:{}:lanes".format(what))
    if not wave_mode and a.wave != b.wave:
        out.add("tie:{}:waves".format(what))
    if a.trip == 0 and b.trip >= 1 and b.thread < a.thread:
        out.add("tie:{}:trips".format(what))
    return out


def geometry_labels(C, G, B, grid_blocks, bad=None, cus=CUS):
    """The labels of one launch; bad [G, B]: the non-finite examples."""
    grid, nw, ipb = launch(C, G, B, grid_blocks, cus)
    where, _, _ = walk(C, G, B, grid_blocks, cus)
    got = {inst_label(instance(C))}
    if nw in (1, 2, 3, 259, 1024):
        got.add("nw:{}".format(nw))
    if nw > 4 and nw % 4:
        got.add("nw:%4")
    if nw < grid and G > 1:
        got.add("nw<grid:G>1")
    if G > grid:
        got.add("G>grid")
    if ipb == WAVES and B % 4:
        got.add("wave:B%4={}".format(B % 4))
    trips = {t for (_, _, t, _) in where.values()}
    if 1 in trips:
        got.add("trip2")
    if 2 in trips:
        got.add("trip3")
    if bad is not None and bad.any():
        seq = collections.defaultdict(dict)    # (g, blk, wave) -> {trip: b}
        it = collections.defaultdict(list)     # (g, blk, trip) -> [b]
        for (g, b), (r, blk, trip, w) in where.items():
            seq[(g, blk, w)][trip] = b
            it[(g, blk, trip)].append(b)
        for (g, _, _), bs in it.items():
            flags = [bool(bad[g, b]) for b in bs]
            if ipb == WAVES and any(flags) and not all(flags):
                got.add("nonfinite:shares_workgroup")
        for (g, _, _), byt in seq.items():
            for t, b in byt.items():
                if bad[g, b] and t + 1 in byt and not bad[g, byt[t + 1]]:
                    got.add("nonfinite:then_finite")
    return got


def data_labels(C, x, lab, r):
    """The labels that depend on the inputs, over every finite example: where
    each member's argmax, the mixture's pred and the label's class lie, how a
    two-way tie is decided (a row with more than two maxima — the all-equal
    example — decides nothing: class 0 of thread 0 wins under any rule), and
    the label values."""
    M, G, B, _ = x.shape
    got = set()
    lab = np.asarray(lab)
    for v, name in ((-1, "label:-1"), (C, "label:C"), (2 ** 40, "label:2^40")):
        if (lab == v).any():
            got.add(name)
    xs = np.where(np.isnan(x), -np.inf, x)
    mx = xs.max(-1, keepdims=True)
    nmax = (xs == mx).sum(-1)
    pmax = (r["pbar"] == r["pbar"].max(-1, keepdims=True)).sum(-1)
    for g in range(G):
        for b in range(B):
            if r["nonfinite"][g, b]:
                continue
            pred = int(r["pred"][g, b])
            got |= spot_labels(C, "pred", pred)
            if pmax[g, b] == 2:
                c1, c2 = np.nonzero(r["pbar"][g, b] == r["pbar"][g, b].max())[0]
                got |= tie_labels(C, "pred", int(c1), int(c2))
            for i in range(M):
                got |= spot_labels(C, "am", int(xs[i, g, b].argmax()))
                if nmax[i, g, b] == 2:
                    c1, c2 = np.nonzero(xs[i, g, b] == mx[i, g, b])[0]
                    got |= tie_labels(C, "am", int(c1), int(c2))
            if 0 <= lab[b] < C:
                got |= spot_labels(C, "label", int(lab[b]))
                if lab[b] == C - 1 and owner(C, C - 1).tail:
                    got.add("label:C-1:tail")
    return got


def bin_labels(r, nb):
    """r: a reference at nb bins."""
    got = {"bins:{}".format(nb)} if nb in BIN_COUNTS else set()
    cnt = sum(t["bin_count"] for t in r["totals"])
    if cnt[15:].any():
        got.add("bin:lane>=15")
    if cnt[32]:
        got.add("bin:lane32")
    if cnt[63]:
        got.add("bin:lane63")
    return got


# ------------------------------------------------------------------- table P
# plants (of every group, on an example that make_case leaves random):
#   ("top", b, am, pred, label)   member 0's maximum at class am, every other member's at pred
#                                 (4 above the row's maximum): pred, disagree = (am != pred)
#   ("tie", b, what, c1, c2, label)  bit-equal maxima at c1 < c2 — "am": in member 0 only, the
#                                 other members' maximum at c1; "pred": in every member, which
#                                 ties the mixture too.  pred = c1, disagree = 0 either way
#   ("gap", b, c0, c1, p, label)  two dominant classes 25 above the rest in every member, the
#                                 mixture p at c0 and 1 - p at c1
#   ("lab", b, label)             the label alone
Case = collections.namedtuple("Case", "C M G B seed grids bins plants")
PLANT = np.float32(4.0)

P = [
    # wave mode, element form: B % 4 = 1, nw 1, 2 and 3 < grid = 9, G > grid, the tail group
    Case(5, 3, 3, 9, 1, (1, 2, 0), (15, 1), (("top", 0, 4, 4, 4), ("top", 8, 0, 4, 2))),
    # lane 63 and the tail group at once; bins 32 and 63 by construction
    Case(255, 3, 2, 10, 2, (1, 3), (64, 2),
         (("top", 0, 254, 254, 254), ("gap", 8, 253, 1, 0.5078125, 253),
          ("top", 9, 3, 252, 254))),
    Case(256, 2, 1, 11, 3, (2,), (16,),
         (("tie", 0, "pred", 3, 255, 3), ("top", 8, 255, 255, 255),
          ("tie", 9, "am", 250, 254, 250), ("lab", 10, 2 ** 40))),
    Case(252, 2, 1, 5, 4, (1,), (33,), (("top", 0, 251, 251, 0),)),      # lane 63 owns no class
    Case(5, 2, 1, 4096, 5, (259, 1024), (64,), (("lab", 100, 2 ** 40),)),
    # workgroup mode, one trip: nw = 5 < grid = 7 with G = 3; nw 2 (G > grid) and 3
    Case(260, 2, 3, 5, 6, (7, 2, 3), (15, 2), (("top", 0, 259, 259, 259),)),
    Case(257, 2, 2, 7, 7, (1, 0), (15,),
         (("top", 0, 256, 256, 256), ("tie", 5, "pred", 100, 256, 100), ("lab", 6, 2 ** 40))),
    Case(260, 2, 1, 1024, 8, (259, 1024), (64,), ()),
    # two trips, 16-B form: thread 0 alone has a second trip (classes 1024 .. 1027) — every tie
    Case(1028, 3, 2, 16, 9, (2, 1), (15, 64),
         (("tie", 0, "am", 20, 1024, 20), ("tie", 8, "pred", 20, 1024, 1024),
          ("tie", 9, "am", 1020, 1024, 1020), ("tie", 10, "pred", 1020, 1024, 1020),
          ("tie", 11, "am", 2, 1025, 2), ("tie", 12, "pred", 2, 1025, 1025),
          ("top", 13, 6, 801, 1027), ("top", 14, 1026, 1026, 7), ("top", 15, 801, 6, 801))),
    # two trips, element form: the tail group (1028, 1029) on thread 1's second trip
    Case(1030, 3, 1, 16, 10, (3, 1), (15,),
         (("top", 0, 1029, 1029, 1029), ("top", 8, 5, 1029, 1028), ("top", 9, 1025, 900, 1025),
          ("top", 10, 900, 1024, 3), ("lab", 11, 2 ** 40))),
    # four trips declared, three used (trip 2: thread 0 alone)
    Case(2052, 3, 2, 16, 11, (2, 0), (33,),
         (("top", 0, 6, 1307, 2049), ("top", 8, 1307, 2050, 6), ("top", 9, 2048, 801, 1500),
          ("top", 10, 2051, 2051, 2051), ("top", 11, 1030, 1030, 1030))),
    Case(2050, 3, 1, 5, 12, (1,), (15,), (("top", 0, 2049, 2049, 2049),)),
    # eight trips declared, five used; the last is the tail group alone
    Case(4099, 3, 1, 16, 13, (1, 5), (16,),
         (("top", 0, 4098, 4098, 4098), ("top", 8, 6, 4097, 2331), ("top", 9, 2331, 801, 4096),
          ("top", 10, 4096, 2331, 801))),
    Case(8192, 3, 1, 16, 14, (2,), (15, 1),
         (("top", 0, 8191, 8191, 8191), ("top", 8, 6, 7168, 3355), ("top", 9, 3355, 801, 7170),
          ("top", 10, 7169, 3355, 801), ("top", 11, 5116, 5116, 5116))),
]
BIG = (P[4], P[7])        # ceil(B / IPB) = 1024: nw = 259 and 1024
EDGE_CASE = "M1-C4-nb4"   # the exact-edge construction below


def case_id(c):
    return "C{}-M{}-G{}-B{}".format(c.C, c.M, c.G, c.B)


def expected(case, plant):
    """(b, pred, disagree, labelled, wrong, label) a plant must report in every group."""
    kind, b = plant[0], plant[1]
    if kind == "lab":
        return None
    if kind == "top":
        _, _, am, pred, lab = plant
        dis = 0 if am == pred else 1
    elif kind == "tie":
        _, _, _, pred, _, lab = plant
        dis = 0
    else:
        _, _, pred, _, _, lab = plant
        dis = 0
    labelled = 0 <= lab < case.C
    return b, pred, dis, labelled, labelled and lab != pred, lab


def plant_labels(case, plant):
    """The path labels a plant is there for (the failure messages name them)."""
    C, kind = case.C, plant[0]
    if kind == "lab":
        return {"label:2^40"} if plant[2] == 2 ** 40 else set()
    if kind == "top":
        _, _, am, pred, lab = plant
        got = spot_labels(C, "am", am) | spot_labels(C, "pred", pred)
    elif kind == "tie":
        _, _, what, c1, c2, lab = plant
        got = tie_labels(C, what, c1, c2) | spot_labels(C, "pred", c1)
    else:
        _, _, c0, _, _, lab = plant
        got = spot_labels(C, "pred", c0)
    if 0 <= lab < C:
        got |= spot_labels(C, "label", lab)
        if lab == C - 1 and owner(C, lab).tail:
            got.add("label:C-1:tail")
    return got


def _plant(x, lab, plant, rng):
    """Redraw example b of every group and member, then plant."""
    M, G, _, C = x.shape
    kind, b = plant[0], plant[1]
    if kind == "lab":
        lab[b] = plant[2]
        return
    x[:, :, b, :] = (3.0 * rng.standard_normal((M, G, C))).astype(np.float32)
    top = x[:, :, b, :].max(-1) + PLANT          # [M, G]
    if kind == "top":
        _, _, am, pred, lb = plant
        assert am == pred or M >= 3
        x[:, :, b, pred] = top
        if am != pred:
            x[0, :, b, pred] = x[0, :, b, am]    # swap: member 0's planted value goes to am
            x[0, :, b, am] = top[0]
    elif kind == "tie":
        _, _, what, c1, c2, lb = plant
        assert M >= 2
        x[:, :, b, c1] = top
        if what == "pred":
            x[:, :, b, c2] = top
        else:
            x[0, :, b, c2] = top[0]
    else:
        _, _, c0, c1, p, lb = plant
        x[:, :, b, c0] = top + np.float32(21.0)
        x[:, :, b, c1] = x[:, :, b, c0] - np.float32(np.log(p / (1.0 - p)))
    lab[b] = lb


def example_margins(r, bins):
    """[G, B]: the smaller of an example's edge margin (over every bin count
    of `bins`) and top-two margin, as predict_ref.margins defines them (an
    exact tie at the top has no top-two margin)."""
    pbar, eps = r["pbar"], r["eps"]
    m = np.full(pbar.shape[:2], np.inf)
    for nb in bins:
        ed = np.linspace(0, 1 + 1e-8, nb + 1)[1:-1]
        if len(ed):
            ext = np.r_[-np.inf, ed, np.inf]
            k = np.searchsorted(ed, pbar)
            dist = np.minimum(pbar - ext[k], ext[k + 1] - pbar)
            m = np.minimum(m, (dist / (eps + R.U)).min(-1))
    if pbar.shape[-1] > 1:
        top = np.sort(pbar, -1)
        gap = top[..., -1] - top[..., -2]
        m = np.minimum(m, np.where(gap == 0, np.inf, gap / eps.max(-1)))
    return np.where(r["nonfinite"], np.inf, m)


def free_examples(case):
    """The examples that make_case leaves random."""
    return [b for b in range(case.B)
            if not (case.B >= 5 and 1 <= b <= 4) and not (case.B >= 8 and 5 <= b <= 7)]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(logits [M, G, B, C], labels [B]) of a case of P: make_case's examples
    (its all-equal row avoiding the edges of the case's first bin count), the
    plants, and every random or planted example redrawn until it is at least
    8 bounds from every decision at every bin count of the case (the host test
    asserts 4 for all examples, the constructed ones included).  Read-only."""
    C, M, G, B = case[:4]
    x, lab = R.make_case(C, M, G, B, case.seed, nb=case.bins[0])
    rng = np.random.default_rng([77, case.seed])
    plants = {p[1]: p for p in case.plants}
    free = free_examples(case)
    assert set(plants) <= set(free)
    for p in case.plants:
        _plant(x, lab, p, rng)
    for _ in range(40):
        m = example_margins(R.reference(x, lab, case.bins[0]), case.bins).min(0)
        redo = [b for b in free if m[b] < 8]
        if not redo:
            break
        for b in redo:
            if b in plants and plants[b][0] != "lab":
                _plant(x, lab, plants[b], rng)
            else:
                x[:, :, b, :] = (3.0 * rng.standard_normal((M, G, C))).astype(np.float32)
    else:
        raise AssertionError("no settled inputs for " + case_id(case))
    x.setflags(write=False)
    lab.setflags(write=False)
    return x, lab


@functools.lru_cache(maxsize=None)
def built(case, nb):
    """(logits, labels, reference, bound) at nb bins; shared, read-only."""
    x, lab = inputs(case)
    r = R.reference(x, lab, nb)
    return x, lab, r, R.bound(r, lab)


def planted_ties(case):
    """(member ties [M, G, B], mixture ties [G, B]) that the plants and
    make_case construct."""
    C, M, G, B = case[:4]
    mt, pt = np.zeros((M, G, B), bool), np.zeros((G, B), bool)
    if B >= 5 and C > 1:
        mt[:, :, 3] = True
        pt[:, 3] = True
    if B >= 8 and C > 1:
        mt[M - 1, :, 7] = True
    for p in case.plants:
        if p[0] == "tie":
            if p[2] == "pred":
                mt[:, :, p[1]] = True
                pt[:, p[1]] = True
            else:
                mt[0, :, p[1]] = True
    return mt, pt


def labels(case, cus=CUS):
    """The set of path labels a case of P reaches."""
    x, lab = inputs(case)
    got = set()
    for nb in case.bins:
        got |= bin_labels(built(case, nb)[2], nb)
    r = built(case, case.bins[0])[2]
    got |= data_labels(case.C, x, lab, r)
    for grid in case.grids:
        got |= geometry_labels(case.C, case.G, case.B, grid, r["nonfinite"], cus)
    return got


def edge_inputs():
    """M = 1, C = 4, all-equal logits, one example labelled 2: every mixture
    probability is 0.25 = fl32 of the first of four bins' edges."""
    return np.full((1, 1, 1, 4), 0.75, np.float32), np.array([2], np.int64)
