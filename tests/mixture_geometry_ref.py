"""The launch geometry of bdl_member_score / bdl_mixture (bdl_mixture.hip)
restated on the host — TEST INFRASTRUCTURE ONLY: which of the eight instances a
class count selects, the workgroups per pair of a grid_blocks (0 by the host
code's formula), a literal walk of the sweep's loops (pair, workgroup,
grid-strided row, wave), the owner of every class (thread, wave, lane, trip,
slot, the masked tail group), the mixture's member order with the row it
prefetches at each step, the combine in its exact fp64 order, the set of path
labels a case reaches, table P — small shapes that together reach every
label — its inputs (make_case's random rows and two builders whose answers are
literal), and BREAKS: wrong variants applied to this restatement only (nothing
is built for a device).  Nothing is imported from bayesdll_amd and nothing from
torch.

The kernels, in the words the restatement follows.  A workgroup has 256 threads
(4 waves).  classes <= 256: WAVE, one wave per row (TPI = 64 threads per row,
IPB = 4 rows per workgroup iteration); above: one workgroup per row (TPI = 256,
IPB = 1).  Thread ti of a row owns the class groups ti + TPI * u, u < NT
(classes 4 q .. 4 q + 3 of group q; a class >= C is masked); NT is 1 for WAVE
and the smallest of 1, 2, 4 with ceil(C / 4) <= 256 NT otherwise;
VEC = (C % 4 == 0).  The grid is (bpp, pairs): workgroup x of a pair takes the
rows x * IPB (+ wave), + bpp * IPB, ... and writes the partial pair * bpp + x
(its waves' counts added in wave order) whether or not it took a row.
grid_blocks = 0: bpp = max(1, min(ceil(B / IPB), ceil(4 CUs / pairs), 1024)).
The mixture walks the components of its group that are not skipped
(weight < 1e-10), the draws of each in order, and loads the next member's row —
the next draw, else the first draw of the next unskipped component — before it
reduces the current one.  The combine's thread t adds the partials t, t + 256,
... of a pair from zero, six butterfly steps add the lanes of a wave, the waves
are added in order 0 .. 3, and the result is added onto (RESET: written over)
the pair's struct."""
from __future__ import annotations

import collections
import functools

import numpy as np

import mixture_ref as R

BLOCK, WAVES, WAVE_CLASSES, MAX_CLASSES, MAX_GRID, MAX_PAIRS = 256, 4, 256, 4096, 1024, 65535
CUS = 256           # the MI355X's; the GPU tests read the device's
KINDS = ("score", "mix:arithmetic", "mix:reference")
EDGES = (252, 255, 256, 257, 260, 1021, 1024, 1025, 1028, 2048, 2049, 2052, 4093, 4096)
INSTANCES = tuple((nt, vec, wave) for nt, wave in ((1, True), (1, False), (2, False), (4, False))
                  for vec in (True, False))

# wrong variants of the restatement (tests/test_mixture_geometry_host.py: each changes the
# expected answer of a case of P, except dispatch_down, which provably changes none)
BREAKS = ("combine_stride64", "combine_one_trip", "waves_reversed", "bstride_no_ipb",
          "prefetch_c_plus_1", "skip_le", "bad_skipped_counted", "dispatch_up", "dispatch_down")

PART = np.dtype([("n", "<i8"), ("n_nonf", "<i8"), ("n_wrong", "<i8"), ("sum", "<f8")])
assert PART.itemsize == 32


# ------------------------------------------------------------------ geometry
def instance(C, breaks=()):
    """(NT, VEC, WAVE) of score_by_classes / mix_by_classes."""
    assert 1 <= C <= MAX_CLASSES
    q = (C + 3) // 4
    vec = C % 4 == 0
    off = 1 if "dispatch_up" in breaks else -1 if "dispatch_down" in breaks else 0
    if C <= WAVE_CLASSES:
        return 1, vec, True
    if q <= BLOCK + off:
        return 1, vec, False
    if q <= 2 * BLOCK + off:
        return 2, vec, False
    return 4, vec, False


def inst_label(inst, kind):
    nt, vec, wave = inst
    return "inst:{}:NT{}:{}:{}".format("wave" if wave else "wg", nt, "vec" if vec else "elem",
                                       kind)


def covered(C, breaks=()):
    """[C] bool: the classes some thread of the selected instance owns."""
    nt, _, wave = instance(C, breaks)
    return np.arange(C) // 4 < nt * (64 if wave else BLOCK)


Owner = collections.namedtuple("Owner", "thread wave lane trip slot tail")


def owner(C, c):
    """Who holds class c of a row: the thread of the row (wave mode: the lane),
    its wave in the workgroup (None in wave mode: the row's), its lane, the
    trip u, the slot j, and whether c's class group is the masked partial one."""
    assert 0 <= c < C
    wave_mode = instance(C)[2]
    tpi = 64 if wave_mode else BLOCK
    q, j = divmod(c, 4)
    u, ti = divmod(q, tpi)
    return Owner(ti, None if wave_mode else ti // 64, ti % 64, u, j,
                 C % 4 != 0 and q == (C + 3) // 4 - 1)


def ipb_of(C):
    return WAVES if C <= WAVE_CLASSES else 1


def launch(C, pairs, B, grid_blocks, cus=CUS):
    """Workgroups per pair as blocks_per_pair computes them."""
    assert 0 <= grid_blocks <= MAX_GRID and 1 <= pairs <= MAX_PAIRS and B >= 1
    if grid_blocks > 0:
        return grid_blocks
    ipb = ipb_of(C)
    slots = (B + ipb - 1) // ipb
    share = (cus * 4 + pairs - 1) // pairs
    return max(1, min(min(slots, share), MAX_GRID))


def default_label(C, pairs, B, cus=CUS):
    """Which term of the default grid's formula decides."""
    ipb = ipb_of(C)
    slots = (B + ipb - 1) // ipb
    share = (cus * 4 + pairs - 1) // pairs
    if slots <= share and slots <= MAX_GRID:
        return "default:slots"
    if slots > MAX_GRID and share >= MAX_GRID:
        return "default:cap"
    return "default:share1" if share == 1 else "default:share"


Walk = collections.namedtuple("Walk", "bpp ipb taken part trip wave times")


def walk(C, pairs, B, grid_blocks, cus=CUS, breaks=()):
    """The sweep's loops literally (every pair walks alike: blockIdx.y only
    offsets the base).  taken[x][w]: the rows workgroup x's wave w takes, in
    trip order (workgroup mode: w = 0, the whole workgroup); part / trip / wave
    [B]: where each row is taken; times [B]: how often.  Asserts that every row
    of every pair is taken once and every partial pair * bpp + x is written
    once, by the workgroups and waves without a row too."""
    bpp = launch(C, pairs, B, grid_blocks, cus)
    ipb = ipb_of(C)
    bstride = bpp * (1 if "bstride_no_ipb" in breaks else ipb)
    part, trip, wave = (np.full(B, -1, np.int64) for _ in range(3))
    times = np.zeros(B, np.int64)
    taken = []
    for x in range(bpp):
        taken.append([np.arange(x * ipb + w, B, bstride, dtype=np.int64) for w in range(ipb)])
        for w, rows in enumerate(taken[x]):
            times[rows] += 1
            part[rows], trip[rows], wave[rows] = x, np.arange(len(rows)), w
    if "bstride_no_ipb" not in breaks:
        assert (times == 1).all()
    written = (np.arange(pairs, dtype=np.int64)[:, None] * bpp + np.arange(bpp)[None, :]).ravel()
    assert np.array_equal(written, np.arange(pairs * bpp))     # blockIdx.y * gridDim.x + blockIdx.x
    return Walk(bpp, ipb, taken, part, trip, wave, times)


def partials(wk, n, n_nonf, n_wrong, val):
    """[pairs, bpp] PART: every workgroup's partial from per-row arrays
    [pairs, B] — a wave (workgroup mode: thread 0) adds its rows in trip order
    from zero, block_total adds the four waves in order."""
    pairs = n.shape[0]
    out = np.zeros((pairs, wk.bpp), PART)
    for x in range(wk.bpp):
        tot = None
        for w in range(WAVES):
            acc = np.zeros(pairs, PART)
            if w < wk.ipb:
                for b in wk.taken[x][w]:
                    acc["n"] += n[:, b]
                    acc["n_nonf"] += n_nonf[:, b]
                    acc["n_wrong"] += n_wrong[:, b]
                    acc["sum"] = acc["sum"] + val[:, b]
            if tot is None:
                tot = acc
            else:
                for k in PART.names:
                    tot[k] = tot[k] + acc[k]
        out[:, x] = tot
    return out


def combine(parts, prior=None, reset=True, breaks=()):
    """bdl_mixture_combine_kernel on [pairs, nw] PART in its exact order: thread
    t adds t, t + 256, ... from zero; six butterfly steps (offsets 32 .. 1,
    v + partner); the waves 0 .. 3 in order; prior + result unless reset.
    Returns [pairs] PART (fp64 sums: compare as bit patterns)."""
    parts = np.asarray(parts)
    pairs, nw = parts.shape
    step = 64 if "combine_stride64" in breaks else BLOCK
    starts = [0] if "combine_one_trip" in breaks else range(0, nw, step)
    out = np.zeros(pairs, PART)
    for k in PART.names:
        # thread t's partial of a trip is start + t; beyond nw it adds nothing (+0 here: the
        # same bits, a sum that started at +0 is never -0)
        src = np.zeros((pairs, max(nw, max(starts) + BLOCK)), parts.dtype[k])
        src[:, :nw] = parts[k]
        v = np.zeros((pairs, BLOCK), parts.dtype[k])
        for t0 in starts:
            v = v + src[:, t0:t0 + BLOCK]
        for off in (32, 16, 8, 4, 2, 1):         # v + the lane off away, in every lane
            h = v.reshape(pairs, BLOCK // (2 * off), 2, off)
            h = h[:, :, 0, :] + h[:, :, 1, :]
            v = np.repeat(h[:, :, None, :], 2, axis=2).reshape(pairs, BLOCK)
        v = v.reshape(pairs, WAVES, 64)
        order = range(WAVES - 1, -1, -1) if "waves_reversed" in breaks else range(WAVES)
        s = None
        for w in order:
            s = v[:, w, 0].copy() if s is None else s + v[:, w, 0]
        out[k] = s
    if not reset:
        for k in PART.names:
            out[k] = prior[k] + out[k]
    return out


def combine_labels(nw):
    got = set()
    if nw == 1:
        got.add("combine:1")
    got.add("combine:lanes" if nw <= 64 else "combine:waves" if nw <= BLOCK else
            "combine:trips2" if nw <= 2 * BLOCK else "combine:trips4" if nw > 3 * BLOCK else
            "combine:trips3")
    if nw > BLOCK and nw % BLOCK:
        got.add("combine:ragged")
    return got - {"combine:trips3"}


# ------------------------------------------------------------------ the member loop
Step = collections.namedtuple("Step", "comp draw read prefetch")


def next_component(w, c, breaks=()):
    while c < len(w) and (w[c] <= R.MIN_WEIGHT if "skip_le" in breaks else w[c] < R.MIN_WEIGHT):
        c += 1
    return c


def members(weights_g, D, breaks=()):
    """The mixture's member order for one group: per step the component, the
    draw, the member whose row is in `cur` (what the step reduces) and the
    member it prefetches into `nxt` (None: no load)."""
    w = [float(v) for v in weights_g]
    comps = len(w)
    steps = []
    c = next_component(w, 0, breaks)
    cur = c * D if c < comps else None
    while c < comps:
        cn = next_component(w, c + 1, breaks)
        for s in range(D):
            i = c * D + s
            if s + 1 < D:
                nxt = i + 1
            elif cn < comps:
                nxt = (c + 1 if "prefetch_c_plus_1" in breaks else cn) * D
            else:
                nxt = None
            steps.append(Step(c, s, cur, nxt))
            cur = nxt
        c = cn
    return steps


def skip_labels(weights_g):
    w = np.asarray(weights_g, dtype=np.float64)
    sk = w < R.MIN_WEIGHT
    n = len(w)
    got = set()
    if not sk.any():
        got.add("skip:none")
    if sk.all():
        got.add("skip:all")
        return got
    if sk[0]:
        got.add("skip:first")
    if sk[-1]:
        got.add("skip:last")
    act = np.nonzero(~sk)[0]
    if sk[act[0]:act[-1]].any():
        got.add("skip:middle")
    if (sk[1:] & sk[:-1]).any():
        got.add("skip:run")
    for c in range(n):
        if w[c] == R.MIN_WEIGHT and ((c and sk[c - 1]) or (c + 1 < n and sk[c + 1])):
            got.add("skip:threshold")
    return got


def patterns(w):
    """[(a column of w [comps, G], the groups whose column compares alike with
    the threshold)]: the member order depends on nothing else."""
    w = np.asarray(w, dtype=np.float64)
    key = np.where(w < R.MIN_WEIGHT, 0, np.where(w == R.MIN_WEIGHT, 1, 2))
    _, first, inv = np.unique(key, axis=1, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    return [(w[:, f], np.nonzero(inv == k)[0]) for k, f in enumerate(first)]


def mixture_restated(hot, rowbad, w, D, combine_mode, breaks=()):
    """What the member loop reads, per group: nonfinite [G, B] (a step's row is
    bad) and, for one-hot rows with hot [M, G, B] the finite class, finite
    [G, B, C] — the classes whose logp is > -inf: arithmetic, hot in a member
    read; reference, hot in a draw of every component walked (no component:
    every class, t = 0).  hot is given as (h, C), or None for nonfinite alone."""
    M, G, B = rowbad.shape
    w = np.asarray(w, dtype=np.float64)
    nonf = np.zeros((G, B), bool)
    sets = None
    if hot is not None:
        hot, C = hot
        sets = np.zeros((G, B, C), bool)
    for col, gs in patterns(w):
        steps = members(col, D, breaks)
        if "bad_skipped_counted" in breaks:
            nonf[gs] = rowbad[:, gs].any(0)
        else:
            for st in steps:
                nonf[gs] |= rowbad[st.read][gs]
        if sets is None:
            continue
        bi = np.arange(B)[None, :]
        if combine_mode == "arithmetic":
            for st in steps:
                sets[gs[:, None], bi, hot[st.read][gs]] = True
        else:
            allc = np.ones((len(gs), B, C), bool)
            for c in sorted({st.comp for st in steps}):
                one = np.zeros((len(gs), B, C), bool)
                for st in steps:
                    if st.comp == c:
                        one[np.arange(len(gs))[:, None], bi, hot[st.read][gs]] = True
                allc &= one
            sets[gs] = allc
    return nonf, sets


# ------------------------------------------------------------------ the labels
TIES = ("slots", "lanes", "waves", "trips")
ALL_LABELS = frozenset(
    [inst_label(i, k) for i in INSTANCES for k in KINDS]
    + ["edge:{}".format(c) for c in EDGES]
    + ["trips:1", "trips:2", "trips:>=3", "uneven", "idle:wave", "idle:block"]
    + ["default:slots", "default:share", "default:share1", "default:cap"]
    + ["pairs:{}:{}".format(p, e) for p in ("1", "max") for e in ("score", "mix")]
    + ["combine:lanes", "combine:waves", "combine:trips2", "combine:trips4", "combine:ragged",
       "combine:1"]
    + ["draws:1", "draws:2", "draws:>=3", "comps:1"]
    + ["skip:" + s for s in ("none", "first", "middle", "last", "run", "all", "threshold")]
    + ["bad:" + s for s in ("first", "mid", "last", "skipped", "then-good")]
    + ["label:trip{}".format(u) for u in range(4)] + ["label:slot{}".format(j) for j in range(4)]
    + ["label:tail", "label:first", "label:last"]
    + ["tie:{}:{}".format(t, s) for t in TIES for s in ("lower", "higher")])
CU_LABELS = frozenset(["default:share1", "default:cap"])


def spot_labels(C, c):
    """Where the label's class c lies."""
    o = owner(C, c)
    got = {"label:trip{}".format(o.trip), "label:slot{}".format(o.slot)}
    if o.tail:
        got.add("label:tail")
    if c == 0:
        got.add("label:first")
    if c == C - 1:
        got.add("label:last")
    return got


def tie_kinds(C, c1, c2):
    """What decides the tie between classes c1 < c2: the slots of one class
    group, the lanes of a wave (the butterfly), the waves of the workgroup
    (LDS, in order), the trips of a thread's groups."""
    assert c1 < c2
    a, b = owner(C, c1), owner(C, c2)
    got = set()
    if a.thread == b.thread:
        got.add("slots" if a.trip == b.trip else "trips")
        return got
    got.add("lanes" if a.wave == b.wave else "waves")
    if a.trip != b.trip:
        got.add("trips")
    return got


def geometry_labels(C, pairs, B, grid_blocks, entry, cus=CUS, bad=None):
    """The labels of one launch of `entry` ("score" / "mix"); bad [pairs', B]:
    the rows (examples) that are non-finite in some pair."""
    wk = walk(C, pairs, B, grid_blocks, cus)
    got = combine_labels(wk.bpp)
    if grid_blocks == 0:
        got.add(default_label(C, pairs, B, cus))
    if pairs == 1:
        got.add("pairs:1:" + entry)
    if pairs == MAX_PAIRS:
        got.add("pairs:max:" + entry)
    for x in range(wk.bpp):
        lens = [len(r) for r in wk.taken[x]]
        for n in lens:
            if n:
                got.add("trips:1" if n == 1 else "trips:2" if n == 2 else "trips:>=3")
        if not any(lens):
            got.add("idle:block")
        elif 0 in lens:
            got.add("idle:wave")
        if len({n for n in lens if n}) > 1:
            got.add("uneven")
        if bad is not None:
            for rows in wk.taken[x]:
                f = bad[:, rows]
                if (f[:, :-1] & ~f[:, 1:]).any():
                    got.add("bad:then-good")
    return got


# ------------------------------------------------------------------- table P
# weights: None (random positive, every group's summing to 1) or a tuple of columns, one per
# group in turn.  plants (integer rows, every member and group, example b):
#   ("top", b, a, label)       the top class a, the label's class (a == label: nll = 0, right)
#   ("tie", b, c1, c2, label)  bit-equal maxima at c1 < c2 alone; the label is one of them
Case = collections.namedtuple("Case", "C B comps draws groups weights grids plants seed")
W4 = ((0.5, 0.25, 0.125, 0.125),     # none skipped
      (0.0, 0.5, 0.25, 0.25),        # the first
      (0.5, 0.0, 0.25, 0.25),        # a middle one
      (0.5, 0.25, 0.25, 0.0),        # the last
      (0.5, 0.0, 0.0, 0.5),          # a run of two
      (0.0, 0.0, 0.0, 0.0),          # all
      (0.5, 1e-10, 0.0, 0.5),        # exactly the threshold (weighted) beside a skipped one
      (0.0, 0.0, 0.5, 0.5))          # the first two: member 0's planted +inf is never read
W3 = ((0.5, 0.25, 0.25), (0.5, 0.0, 0.5), (0.0, 0.5, 0.5))
W2 = ((0.5, 0.5), (0.0, 1.0), (1.0, 0.0))

P = [
    # wave mode, element form, narrow rows: 1025 row slots — the default grid's cap (256 CUs),
    # 1024 and 300 partials (four trips of the combine, two ragged ones), >= 3 trips of a slot
    Case(3, 4100, 2, 3, 1, None, (0, 100, 300, 1024), (("tie", 0, 0, 1, 0), ("tie", 4, 0, 2, 2)), 1),
    # workgroup mode, element form: 1030 row slots; one pair for both entry points
    Case(257, 1030, 1, 1, 1, None, (0, 1023, 257),
         (("top", 0, 256, 256), ("tie", 8, 3, 256, 256), ("tie", 9, 3, 256, 3)), 2),
    # pairs at blockIdx.y's limit, one workgroup each
    Case(4, 2, 1, 1, 65535, None, (1,), (("tie", 0, 0, 3, 3), ("top", 1, 2, 0)), 3),
    # the default grid's share (100 pairs: 11 of 13 slots at 256 CUs, 3 at 64) and its share
    # of 1 (1100 pairs at either)
    Case(5, 50, 1, 2, 100, None, (0,), (("top", 0, 4, 4),), 4),
    Case(5, 5, 1, 1, 1100, None, (0,), (), 5),
    # every skip pattern, four draws; wave mode on both sides of lane 63's last group
    Case(255, 13, 4, 2, 8, W4, (1, 2, 0),
         (("top", 0, 254, 254), ("tie", 8, 252, 254, 254), ("tie", 9, 3, 7, 3),
          ("tie", 10, 4, 6, 6), ("tie", 11, 4, 6, 4)), 6),
    Case(252, 21, 3, 4, 3, W3, (1, 3, 7), (("top", 0, 0, 251), ("tie", 8, 0, 251, 251)), 7),
    Case(256, 10, 2, 1, 3, W2, (2, 0), (("top", 0, 255, 255), ("tie", 8, 0, 255, 0)), 8),
    # workgroup mode, one trip
    Case(260, 11, 4, 2, 8, W4, (1, 3, 16),
         (("top", 0, 259, 259), ("tie", 8, 10, 250, 250), ("tie", 9, 10, 250, 10),
          ("tie", 10, 10, 259, 259), ("tie", 2, 10, 259, 10)), 9),
    Case(1021, 9, 3, 1, 2, W3, (1, 0), (("top", 0, 5, 1020),), 10),
    Case(1024, 9, 2, 1, 1, W2, (2, 0), (("top", 0, 1023, 1023), ("top", 8, 1020, 1021)), 11),
    # two trips: thread 0 alone has a second trip at 1025 (one class) and 1028
    Case(1025, 9, 2, 2, 3, W2, (1, 2, 0),
         (("top", 0, 1024, 1024), ("tie", 8, 3, 1024, 1024), ("tie", 2, 3, 1024, 3)), 12),
    Case(1028, 9, 3, 1, 3, W3, (1, 0),
         (("top", 0, 1027, 1027), ("tie", 8, 1020, 1024, 1024), ("tie", 2, 1020, 1024, 1020),
          ("top", 3, 1024, 1026)), 13),
    Case(2048, 5, 2, 1, 1, W2, (1, 0), (("top", 0, 2047, 2047), ("top", 3, 2044, 1023)), 14),
    # four trips declared, three used at 2049 / 2052 (thread 0 alone has the third)
    Case(2049, 9, 2, 1, 2, W2, (2, 0),
         (("top", 0, 2048, 2048), ("tie", 8, 5, 2048, 2048), ("tie", 2, 5, 2048, 5)), 15),
    Case(2052, 5, 1, 4, 1, None, (1, 0), (("top", 0, 2051, 2049), ("top", 3, 2050, 2050)), 16),
    Case(4093, 9, 2, 1, 2, W2, (1, 0),
         (("top", 0, 4092, 4092), ("top", 8, 3000, 4090), ("top", 2, 4092, 3072)), 17),
    Case(4096, 9, 2, 2, 1, W2, (1, 4, 0),
         (("top", 0, 4095, 4095), ("top", 8, 7, 1027), ("top", 2, 7, 2050), ("top", 3, 7, 3077),
          ("tie", 1, 1000, 3000, 3000), ("tie", 4, 1000, 3000, 1000)), 18),
]
ROUNDING = P[0]          # the rounding-sensitive random case of the combine's bit-level tests
COMBINE_NW = (1, 2, 64, 65, 256, 257, 1023, 1024)
PAIRS_MAX = P[2]
TOP = np.float32(4096.0)
TIE_NLL = 1420.0 / 2048.0   # fl32(4096 + logf(2)) - 4096: the nll of a two-way tie at the top


def case_id(c):
    return "C{}-B{}-{}x{}-G{}".format(c.C, c.B, c.comps, c.draws, c.groups)


def logits_of(c):
    return c.comps * c.draws * c.groups * c.B * c.C


def weights(c):
    """[comps, G] float64 of a case."""
    if c.weights is None:
        w = np.random.default_rng(8100 + c.seed).random((c.comps, c.groups)) + 0.1
        return w / w.sum(0, keepdims=True)
    cols = np.array(c.weights, dtype=np.float64).T          # [comps, patterns]
    assert cols.shape[0] == c.comps
    return np.ascontiguousarray(cols[:, np.arange(c.groups) % cols.shape[1]])


@functools.lru_cache(maxsize=None)
def random_inputs(c):
    """make_case's rows and labels with the case's weights; read-only."""
    x, lab, _ = R.make_case(c.C, c.B, c.comps, c.draws, c.groups, 100 + c.seed)
    w = weights(c)
    for v in (x, lab, w):
        v.setflags(write=False)
    return x, lab, w


@functools.lru_cache(maxsize=None)
def references(c):
    """(score reference, {combine: mixture reference}) of random_inputs(c)."""
    x, lab, w = random_inputs(c)
    return R.score_reference(x, lab), {m: R.mixture_reference(x, w, c.draws, m)
                                       for m in R.COMBINES}


@functools.lru_cache(maxsize=None)
def integer_rows(c):
    """The score's literal input: every class -inf but a top class a at 4096
    and the label's class at 4096 - k, k an integer in [200, 2^20) per (member,
    group, row) — Z = 1, lse = 4096, nll = k exactly (0 where a is the label;
    1420 / 2048 at a planted two-way tie).  Returns (logits, labels, nll
    [M, G, B] float64, wrong [M, G, B] bool); read-only."""
    rng = np.random.default_rng(8200 + c.seed)
    M, G, B, C = c.comps * c.draws, c.groups, c.B, c.C
    lab = rng.integers(0, C, size=B).astype(np.int64)
    a = rng.integers(0, C, size=(M, G, B))
    a = np.where(rng.random((M, G, B)) < 0.3, lab[None, None, :], a)
    k = rng.integers(200, 2 ** 20, size=(M, G, B)).astype(np.float64)
    tie = np.zeros(B, bool)
    second = np.zeros(B, np.int64)
    for p in c.plants:
        b = p[1]
        if p[0] == "top":
            a[:, :, b], lab[b] = p[2], p[3]
        else:
            _, _, c1, c2, lb = p
            assert lb in (c1, c2) and c1 < c2
            a[:, :, b], second[b], lab[b], tie[b] = c1, c2, lb, True
    x = np.full((M, G, B, C), -np.inf, np.float32)
    mi, gi, bi = np.ix_(np.arange(M), np.arange(G), np.arange(B))
    x[mi, gi, bi, lab[None, None, :]] = (TOP - k).astype(np.float32)
    x[mi, gi, bi, a] = TOP
    x[:, :, tie, second[tie]] = TOP
    right = a == lab[None, None, :]
    nll = np.where(right, 0.0, k)
    nll[:, :, tie] = TIE_NLL
    wrong = ~right
    wrong[:, :, tie] = (lab[tie] != a[0, 0, tie])[None, None, :]   # the lower class wins
    for v in (x, lab, nll, wrong):
        v.setflags(write=False)
    return x, lab, nll, wrong


def hot_class(c):
    """h [M, G, B] of the one-hot rows: draw 0 of every component at the
    example's base class; a later draw at a class of the component's own for
    two examples in three, at the base class for the third."""
    M, G, B, C = c.comps * c.draws, c.groups, c.B, c.C
    i, g, b = np.ix_(np.arange(M), np.arange(G), np.arange(B))
    base = (7 * g + 13 * b + 5) % C
    own = (base + 1 + (i // c.draws) * 3 + (i % c.draws)) % C
    return np.where((i % c.draws == 0) | (b % 3 == 0), base, own)


@functools.lru_cache(maxsize=None)
def one_hot_rows(c):
    """The mixture's literal input: member i, group g, example b has one finite
    class h(i, g, b) (an integer in [-8, 8] there) and -inf elsewhere: every
    member's softmax is one-hot, expected_entropy is 0 and the classes with
    logp > -inf are mixture_restated's sets.  Returns (logits, h); read-only."""
    h = hot_class(c)
    M, G, B = h.shape
    x = np.full((M, G, B, c.C), -np.inf, np.float32)
    mi, gi, bi = np.ix_(np.arange(M), np.arange(G), np.arange(B))
    x[mi, gi, bi, h] = ((mi + 3 * gi + 5 * bi) % 17 - 8).astype(np.float32)
    x.setflags(write=False)
    h.setflags(write=False)
    return x, h


@functools.lru_cache(maxsize=None)
def one_hot_reference(c, combine_mode):
    """mixture_reference of one_hot_rows(c): the bound of its finite entries."""
    return R.mixture_reference(one_hot_rows(c)[0], weights(c), c.draws, combine_mode)


def finite_sets(c, combine_mode, breaks=()):
    """[G, B, C] bool: the literal logp > -inf pattern of one_hot_rows(c)."""
    _, h = one_hot_rows(c)
    return mixture_restated((h, c.C), np.zeros(h.shape, bool), weights(c), c.draws, combine_mode,
                            breaks)[1]


def score_expected(c, grid_blocks, nll, ok, bad, wrong, cus=CUS, breaks=(), prior=None,
                   reset=True):
    """[M * G] PART: walk -> partials -> combine of per-row arrays [M, G, B]."""
    pairs = c.comps * c.draws * c.groups
    wk = walk(c.C, pairs, c.B, grid_blocks, cus, breaks)
    f = lambda v, t: np.asarray(v).reshape(pairs, c.B).astype(t)   # noqa: E731
    val = np.where(f(ok, bool), f(nll, np.float64), 0.0)
    parts = partials(wk, f(ok, np.int64), f(bad, np.int64), f(wrong, np.int64), val)
    return combine(parts, prior, reset, breaks), parts


def labels_of(c, cus=CUS):
    """The set of path labels a case of P reaches, derived from the functions
    above."""
    C, B, D = c.C, c.B, c.draws
    M, G = c.comps * D, c.groups
    inst = instance(C)
    got = {inst_label(inst, k) for k in KINDS}
    if C in EDGES:
        got.add("edge:{}".format(C))
    got.add("draws:1" if D == 1 else "draws:2" if D == 2 else "draws:>=3")
    if c.comps == 1:
        got.add("comps:1")
    w = weights(c)
    x, _, _ = random_inputs(c)
    rowbad = R.nonfinite_rows(np.asarray(x, dtype=np.float64))     # [M, G, B]
    for col, gs in patterns(w):
        got |= skip_labels(col)
        steps = members(col, D)
        read = [st.read for st in steps]
        for pos, i in enumerate(read):
            if rowbad[i][gs].any():
                got.add("bad:first" if pos == 0 else "bad:last" if pos == len(read) - 1 else
                        "bad:mid")
        if any(rowbad[i][gs].any() for i in range(M) if i not in read):
            got.add("bad:skipped")
    mixbad = mixture_restated(None, rowbad, w, D, "arithmetic")[0]  # [G, B]
    for grid in c.grids:
        got |= geometry_labels(C, M * G, B, grid, "score", cus) - {"bad:then-good"}
        got |= geometry_labels(C, G, B, grid, "mix", cus, mixbad)
    _, lab, _, _ = integer_rows(c)
    for p in c.plants:
        got |= spot_labels(C, int(lab[p[1]]))
        if p[0] == "tie":
            _, _, c1, c2, lb = p
            for t in tie_kinds(C, c1, c2):
                got.add("tie:{}:{}".format(t, "lower" if lb == c1 else "higher"))
    return got
