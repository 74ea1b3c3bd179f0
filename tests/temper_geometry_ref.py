"""The geometry of the temperature-scaling sweeps (bdl_temper.hip) restated on
the host — TEST INFRASTRUCTURE ONLY: which of the ten sweep instances a class
count selects, the grid and the partials per group of an explicit grid_blocks,
a literal walk of the kernels' loops (group, rotated workgroup, grid-strided
example, wave, thread, trip, element slot), the set of path labels a case
reaches, table T — the smallest shapes that reach every label — and its inputs.
Nothing is imported from bayesdll_amd and nothing from torch.

The kernels, in the words the walk follows.  A sweep workgroup has 256 threads
(4 waves).  classes <= 256: WAVE, one wave per example (TPI = 64 threads per
example, IPB = 4 examples per workgroup iteration); above: one workgroup per
example (TPI = 256, IPB = 1).  Thread ti of an example owns the class groups
ti + TPI * u, u < NT (classes 4 q .. 4 q + 3 of group q; a class >= C is
masked).  NT is 1 for WAVE and the smallest of 1, 2, 4, 8 with
ceil(C / 4) <= 256 NT otherwise; VEC = (C % 4 == 0).  Workgroup blk takes, of
group g, the examples r * IPB (+ wave), + grid * IPB, ... with
r = (blk - g) mod grid, skips the group if r * IPB >= N, and writes the
partial g * nw + r, nw = min(grid, ceil(N / IPB)).  The report's bins are
collected wave by wave: in trip u the lanes s < nsrc of a wave own a class
group, nsrc = clamp(Q - (wave * 64 (workgroup mode) + TPI * u), 0, 64),
Q = ceil(C / 4).  The update kernel's thread t adds the partials t, t + 256,
...; the combine kernel's wave w the partials [w nw / 4, (w + 1) nw / 4)."""
from __future__ import annotations

import functools

import numpy as np

import temper_ref as R

BLOCK, WAVES, WAVE_CLASSES, MAX_CLASSES, MAX_GRID = 256, 4, 256, 8192, 1024

INSTANCES = tuple((nt, vec, wave) for nt, wave in ((1, True), (1, False), (2, False), (4, False),
                                                   (8, False)) for vec in (True, False))


def instance(C):
    """(NT, VEC, WAVE) of by_classes."""
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


def geometry(N, G, C, grid_blocks):
    """(grid, nw) of an explicit grid_blocks (the default grid depends on the
    device's CU count and is not restated)."""
    assert 1 <= grid_blocks <= MAX_GRID, "explicit grids only"
    ipb = WAVES if C <= WAVE_CLASSES else 1
    per_group = (N + ipb - 1) // ipb
    return grid_blocks, min(grid_blocks, per_group)


ALL_LABELS = frozenset(
    [inst_label(i) for i in INSTANCES]
    + ["trip2:multi",          # a second grid-stride trip (the prefetched row consumed), NT > 1
       "idle_wave",            # wave mode: a wave without an example in a participating workgroup
       "late_trip:partial",    # a trip u >= 1 with 0 < nsrc < 64 in some wave
       "late_trip:empty_wave",  # a trip u >= 1 with nsrc = 0 in a wave while another has work
       "late_trip:no_group",   # a trip u >= 1 of the instance that no class group reaches
       "late_trip:tail",       # the masked tail group (C % 4 != 0) in a trip u >= 1
       "label:trip0", "label:middle", "label:last",   # the label's class in that trip (NT > 1)
       "max:late_trip",        # the row maximum in a trip u >= 1
       "max:tail",             # the row maximum in the masked tail group
       "rotated",              # g % grid != 0
       "groups>grid",          # the rotation wraps
       "skip",                 # nw < grid: workgroups that hold no example of a group
       "nw>256", "nw=1024", "nw<4", "nw%4"])


# ---------------------------------------------------------------- the cases
# (C, N, G, grid_blocks, seed).  Wave mode: nw 1 (three workgroups skip, an idle
# wave), 3 and 2 (a second trip, G > grid), the 16-B form below 256.  Workgroup
# mode NT = 1: 260 at nw = 259 and 1024 (the second-stage kernels' further
# trips), 1023 (element form).  Both sides of every instance boundary on both
# load forms (1028 | 1030, 2048 | 2049, 2052, 4096 | 4097, 4100), a last trip
# whose fourth wave is partial (3002: 47 lanes, the tail group among them;
# 6000: 28 lanes), the last element-form count (8190) and the limit.  N = 3 .. 7
# on one or two workgroups gives every large C a second grid-stride trip.
T = [
    (10, 3, 2, 4, 21), (10, 11, 3, 3, 23), (12, 11, 3, 2, 3), (37, 9, 3, 2, 4),
    (260, 259, 2, 259, 5), (260, 1030, 2, 1024, 526), (1023, 5, 2, 2, 7),
    (1028, 5, 2, 2, 8), (1030, 7, 3, 2, 9), (2048, 4, 1, 1, 110), (2049, 5, 2, 2, 31),
    (2052, 5, 2, 2, 52), (3002, 5, 3, 2, 13), (4096, 3, 1, 1, 14), (4097, 4, 2, 2, 15),
    (4100, 4, 2, 1, 36), (6000, 3, 1, 1, 17), (8190, 3, 2, 2, 38), (8192, 5, 1, 2, 19),
]
# the per-group betas of the one-sweep and report tests (fp32 values)
BETAS = (float(np.float32(0.37)), 2.5, 1.0)
SHARP = (0.6, 1.5, 0.8)
PLANT = 1.0     # a planted top class is this far above the row's maximum


def case_id(c):
    return "C{}-N{}-G{}-grid{}".format(*c[:4])


def betas_of(case):
    return [BETAS[g % 3] for g in range(case[2])]


def has_special(case):
    return 8 <= case[1] <= 16


def free_rows(case):
    """The examples that are not make_rows' special rows 1..7."""
    return [b for b in range(case[1]) if not (has_special(case) and 1 <= b <= 7)]


def trips_used(C):
    """Trips of an example that hold a class group."""
    nt, _, wave = instance(C)
    q = (C + 3) // 4
    return (q + (64 if wave else BLOCK) - 1) // (64 if wave else BLOCK)


def _class_in_trip(C, u, k):
    """A class of trip u (workgroup mode), spread over threads and slots by k."""
    q = (C + 3) // 4
    groups = min(BLOCK, q - BLOCK * u)
    c = 4 * (BLOCK * u + (37 * k + 5) % groups) + k % 4
    return min(c, C - 1)


def plan(case):
    """{example: (label or None, top class or None)} — what `rows` plants.  The
    i-th free example's label goes to trip 0, a middle trip, the last trip in
    turn (the last trip's is class C - 1: the tail group where C % 4 != 0); its
    top class to the label, to class C - 1, to trip 1, to nowhere in turn."""
    C, N = case[:2]
    if instance(C)[2]:
        # wave mode has one trip: the label stays make_rows', the top class goes to the
        # last class (the tail group) for every second free example
        return {b: (None, C - 1 if i % 2 else None) for i, b in enumerate(free_rows(case))}
    last = trips_used(C) - 1
    out = {}
    for i, b in enumerate(free_rows(case)):
        lt = (0, last // 2 if last >= 2 else 0, last)[i % 3]
        lab = C - 1 if (lt == last and last >= 1) else _class_in_trip(C, lt, i)
        top = (lab, C - 1, _class_in_trip(C, min(1, last), i + 1), None)[i % 4]
        out[b] = (lab, top)
    return out


@functools.lru_cache(maxsize=None)
def rows(case):
    """(z [G, N, C] fp32, labels [N]) of a case: temper_ref.make_rows per group
    around shared labels (group g > 0 with its own noise, as the older GPU
    test builds its groups), then the plan's labels and top classes planted in
    every group.  Computed once and shared (read-only)."""
    C, N, G, _, seed = case
    zs, lab = [], None
    for g in range(G):
        z, l = R.make_rows(N, C, 300 + seed, sharp=SHARP[g % 3], special=has_special(case))
        if g:
            rng = np.random.default_rng([seed, g])
            z = np.where(np.isfinite(z), z + (0.05 * rng.standard_normal(z.shape)).astype(np.float32), z)
        zs.append(z.astype(np.float32))
        lab = l
    z = np.stack(zs)
    lab = lab.copy()
    for b, (pl, top) in plan(case).items():
        if pl is not None:
            lab[b] = pl
        if top is not None:
            z[:, b, top] = z[:, b, :].max(-1) + np.float32(PLANT)
    z.setflags(write=False)
    lab.setflags(write=False)
    return z, lab


# the bin counts besides 15 (at 64 lane 63 owns a bin), on one shape per mode
BIN_COUNTS = (1, 2, 64)
BIN_CASES = [T[3], T[8]]
BIN_BETAS = (float(np.float32(0.37)), 2.5, 10.0)   # at 10 a top class reaches the last bin
MAX_ITER_CASE = T[12]   # every group needs three or four moves at rtol = 1e-6


def upper_limit_rows():
    """(z [6, 1030], labels): nearly flat rows whose label is the top class by
    0.05, planted in the second trip of the NT = 2 element-form instance: the
    NLL falls for ever as beta grows, and the margin is small enough that the
    label's probability stays low up to beta = 64 and every Newton step is cut
    to 4 beta."""
    rng = np.random.default_rng(41)
    z = (0.01 * rng.standard_normal((6, 1030))).astype(np.float32)
    lab = np.array([1029, 1024, 1027, 1025, 1028, 1026], dtype=np.int64)
    z[np.arange(6), lab] = z.max(-1) + np.float32(0.05)
    return z, lab


# ------------------------------------------------------------------ the walk
def walk(C, N, G, grid_blocks):
    """The kernels' loops literally.  Returns (visits [G, N, C]: how often every
    (group, example, class) is taken by a thread that owns it, partials: the
    set of (group, r) written, labels: the geometric path labels, nsrc: the set
    of (wave, trip, nsrc)).  Asserts on the way that an example is taken once,
    that lane s of a wave owns a class group of trip u exactly if s < nsrc, and
    that a written partial lies in [0, nw)."""
    nt, vec, wave_mode = instance(C)
    tpi, ipb = (64, WAVES) if wave_mode else (BLOCK, 1)
    grid, nw = geometry(N, G, C, grid_blocks)
    Q = (C + 3) // 4
    got = {inst_label((nt, vec, wave_mode))}
    visits = np.zeros((G, N, C), np.int64)
    taken = np.zeros((G, N), np.int64)
    partials, nsrcs = set(), set()
    if G > grid:
        got.add("groups>grid")
    if nw < grid:
        got.add("skip")
    if nw > 256:
        got.add("nw>256")
    if nw == 1024:
        got.add("nw=1024")
    if nw < 4:
        got.add("nw<4")
    if nw % 4:
        got.add("nw%4")
    # what one example's threads own: [thread-of-example, trip, slot] -> class
    ti = np.arange(tpi)[:, None, None]
    cls = 4 * (ti + tpi * np.arange(nt)[None, :, None]) + np.arange(4)[None, None, :]
    owned = cls[cls < C]
    assert len(np.unique(owned)) == len(owned)
    # the report's source lanes per (wave, trip) against the owners
    for w in range(1 if wave_mode else WAVES):
        for u in range(nt):
            nsrc = max(0, min(64, Q - ((0 if wave_mode else w * 64) + tpi * u)))
            nsrcs.add((w, u, nsrc))
            for s in range(64):
                q = (s if wave_mode else w * 64 + s) + tpi * u
                assert (q < Q) == (s < nsrc), (C, w, u, s)
    for u in range(1, nt):
        per_wave = [n for (w, uu, n) in nsrcs if uu == u]
        if any(0 < n < 64 for n in per_wave):
            got.add("late_trip:partial")
        if any(n == 0 for n in per_wave) and any(n > 0 for n in per_wave):
            got.add("late_trip:empty_wave")
        if all(n == 0 for n in per_wave):
            got.add("late_trip:no_group")
    if C % 4 and (Q - 1) // tpi >= 1:
        got.add("late_trip:tail")
    for g in range(G):
        if g % grid:
            got.add("rotated")
        for blk in range(grid):
            r = (blk + grid - g % grid) % grid
            if r * ipb >= N:
                continue
            assert r < nw
            assert (g, r) not in partials
            partials.add((g, r))
            for w in range(WAVES if wave_mode else 1):
                b, trip = r * ipb + w, 0
                if b >= N:
                    got.add("idle_wave")
                while b < N:
                    if trip and nt > 1:
                        got.add("trip2:multi")
                    taken[g, b] += 1
                    np.add.at(visits[g, b], owned, 1)
                    b, trip = b + grid * ipb, trip + 1
    assert (taken == 1).all()
    assert partials == {(g, r) for g in range(G) for r in range(nw)}
    return visits, partials, got, nsrcs


def second_stage(nw):
    """How often the update kernel's strided loop and the combine kernel's
    quarters take each of a group's nw partials: ([nw], [nw])."""
    upd, comb = np.zeros(nw, np.int64), np.zeros(nw, np.int64)
    for t in range(BLOCK):
        for i in range(t, nw, BLOCK):
            upd[i] += 1
    for w in range(WAVES):
        for i in range(w * nw // WAVES, (w + 1) * nw // WAVES):
            comb[i] += 1
    return upd, comb


def data_labels(C, z, lab):
    """The labels that depend on the inputs: the trip of every labelled, finite
    example's label class, the trip and the group of every row maximum."""
    nt, _, wave_mode = instance(C)
    tpi = 64 if wave_mode else BLOCK
    Q = (C + 3) // 4
    last = trips_used(C) - 1
    got = set()
    for g in range(z.shape[0]):
        bad, _, _, labelled = R.classify(z[g], lab, 1.0)
        for b in np.nonzero(~bad)[0]:
            am = int(np.argmax(z[g, b]))
            if (am // 4) // tpi >= 1:
                got.add("max:late_trip")
            if C % 4 and am // 4 == Q - 1:
                got.add("max:tail")
            if labelled[b] and nt > 1:
                u = (int(lab[b]) // 4) // tpi
                got.add("label:trip0" if u == 0 else "label:last" if u == last else "label:middle")
    return got


def labels(case, z=None, lab=None):
    """The set of path labels a case reaches (its own inputs by default)."""
    if z is None:
        z, lab = rows(case)
    return walk(*case[:4])[2] | data_labels(case[0], z, lab)
