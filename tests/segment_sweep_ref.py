"""Host restatement of the segment traversal that bdl_chain_clip's two sweeps
(bdl_clip.hip) and bdl_chain_stats' sweep (bdl_stats.hip) share, and table T,
built for it — TEST INFRASTRUCTURE ONLY.  Nothing is imported from
bayesdll_amd and nothing from torch.

The traversal, per (chain k, workgroup w of blocks_per_chain, segment i):

  b       = layers_ref.rotated(w, i, bpc): the workgroup's index in segment
            i's rotation.
  W       = 4 when the chain's gradient slice and its theta slice share one
            misalignment mod 16 B (the clip has no theta: always 4), else 1.
  W = 4   layers_ref.split cuts the slice into `head` elements (capped by
            numel), `nbody` float4 groups and `tail` elements; b = 0 gives the
            head to lanes 0 .. head-1 and the tail to lanes 4 .. 4+tail-1.
            A unit is a float4 group, nunits = nbody.
  W = 1   a unit is an element, nunits = numel; no head, no tail.
  body    block iterations of K_ITER = 4 x 256 units: full ones at gb =
            b*K_ITER, + bpc*K_ITER, ... while gb + K_ITER <= nunits, then at
            most one partial iteration (gb < nunits) whose sub-block u holds
            min(256, nunits - gb - 256 u) lanes.
  idle    b != 0 and b*K_ITER >= nunits: nothing of the segment is this
            workgroup's (bdl_chain_stats stores zero partials on that path;
            the clip's loops simply do not run).

`covered` turns a launch into the set of path labels it reaches;
tests/test_segment_sweep_host.py proves on the CPU that table T reaches every
label over the geometries the GPU tests launch, and pins what tables A and B
of tests/stacked_tables.py do not reach.

Path labels (W is 4 or 1):

  ("head", h, capped) ("tail", t) ("nbody", 0 | 1) ("align", mis, numel <= 9)
                          the rotation's first workgroup on the 16-B path
  (W, "full-only") (W, "full+partial") (W, "partial-only") (W, "idle")
  (W, "ends-in", u)       the partial iteration ends inside sub-block u
  (W, "ends-on", j)       ... exactly on the boundary 256 j (j = 4: the last
                          full iteration ends the body, no partial one)
  (W, "second-full", rotated)     a second full trip of the grid-stride loop
  (W, "second-partial", rotated)  one full trip, then the partial iteration;
                          rotated: b != w
  ("pair", gradient misalignment, theta misalignment)     statistics only
"""
from __future__ import annotations

from collections import namedtuple

from layers_ref import K_BLOCK, rotated, split

UNROLL = 4
K_ITER = K_BLOCK * UNROLL   # units per block iteration (kClipIter, kStatsIter)

Visit = namedtuple("Visit", "W b idle head capped tail nunits full partial gb_partial")


def chain_mis(mis, stride, k):
    """Misalignment (elements mod 4) of chain k's slice of a segment."""
    return (mis + k * stride) % 4


def visit(mis_k, numel, b, bpc, W=4):
    """What workgroup b of a segment's rotation does in a chain's slice whose
    misalignment is mis_k: head / tail element counts (lanes 0.. and 4..), the
    number of full iterations, the partial iteration's lane count per
    sub-block (None: no partial iteration) and its first unit."""
    if W == 4:
        h, nunits, tail = split(mis_k, numel)
    else:
        h, nunits, tail = 0, numel, 0
    if b != 0 and b * K_ITER >= nunits:
        return Visit(W, b, True, 0, False, 0, nunits, 0, None, None)
    gb, stride, full = b * K_ITER, bpc * K_ITER, 0
    if gb + K_ITER <= nunits:
        full = (nunits - K_ITER - gb) // stride + 1
        gb += full * stride
    partial = None
    if gb < nunits:
        partial = tuple(max(0, min(K_BLOCK, nunits - gb - K_BLOCK * u)) for u in range(UNROLL))
    first = b == 0
    return Visit(W, b, False, h if first else 0, first and h < (4 - mis_k) % 4,
                 tail if first else 0, nunits, full, partial, gb if partial else None)


def head_lanes(v):
    return tuple(range(v.head))


def tail_lanes(v):
    return tuple(range(4, 4 + v.tail))


def _path(row, k):
    mis, numel, stride = row[:3]
    tmis = row[3] if len(row) > 3 else None
    mk = chain_mis(mis, stride, k)
    return mk, numel, tmis, 4 if tmis is None or tmis == mk else 1


def sweep(table, K, bpc):
    """{(chain, workgroup, segment): Visit}.  table rows: (base misalignment,
    numel, chain stride) for the clip, with theta's misalignment as a fourth
    entry for the statistics."""
    out = {}
    for i, row in enumerate(table):
        assert row[1] >= 1 and row[2] >= row[1]
        for k in range(K):
            mk, numel, _, W = _path(row, k)
            for w in range(bpc):
                out[k, w, i] = visit(mk, numel, rotated(w, i, bpc), bpc, W)
    return out


def labels(v, w, bpc, mis_k, numel, tmis=None):
    """The path labels of one visit (the module docstring)."""
    W, out = v.W, set()
    if tmis is not None and v.b == 0:
        out.add(("pair", mis_k, tmis))
    if v.idle:
        out.add((W, "idle"))
        return out
    if W == 4 and v.b == 0:
        out |= {("head", v.head, v.capped), ("tail", v.tail)}
        if v.nunits <= 1:
            out.add(("nbody", v.nunits))
        if numel <= 9:
            out.add(("align", mis_k, numel))
    rot = v.b != w
    if v.partial is not None:
        out.add((W, "full+partial" if v.full else "partial-only"))
        u = max(j for j in range(UNROLL) if v.partial[j])
        out.add((W, "ends-in", u) if v.partial[u] < K_BLOCK else (W, "ends-on", u + 1))
        if v.full == 1:
            out.add((W, "second-partial", rot))
    elif v.full:
        out.add((W, "full-only"))
        if (v.b + (v.full - 1) * bpc + 1) * K_ITER == v.nunits:
            out.add((W, "ends-on", UNROLL))
    if v.full >= 2:
        out.add((W, "second-full", rot))
    return out


def covered(table, K, bpc):
    """The set of path labels a launch over `table` reaches."""
    out = set()
    for i, row in enumerate(table):
        for k in range(K):
            mk, numel, tmis, W = _path(row, k)
            for w in range(bpc):
                out |= labels(visit(mk, numel, rotated(w, i, bpc), bpc, W), w, bpc, mk, numel, tmis)
    return out


def default_bpc(cus, K, limit, per_cu=4):
    """blocks_per_chain = 0: per_cu workgroups per CU over all chains, at most
    `limit` per chain (bdl_chain_common.hpp blocks_per_chain)."""
    return max(1, min((cus * per_cu + K - 1) // K, limit))


def check_default_geometry(cus):
    """blocks_per_chain = 0 on a device of `cus` compute units, asserted: the
    rotation's first workgroup still reaches every head / tail / alignment /
    pair label, and where there are more workgroups than the largest segment
    has block iterations every workgroup makes at most one trip and some are
    idle — what the default adds is the widest rotation.  Returns the two
    (clip, statistics) geometries."""
    out = []
    for stats, lim in ((False, CLIP_LIMIT), (True, STATS_LIMIT)):
        bpc = default_bpc(cus, K_T, lim)
        cov = covered(PlacedT("tensor").rows(stats), K_T, bpc)
        first = {lb for lb in required(stats) if lb[0] in ("head", "tail", "align", "nbody", "pair")}
        assert first <= cov, (cus, stats, sorted(first - cov, key=str))
        if bpc * K_ITER >= max(s[1] for s in SEGMENTS_T):
            for W in (4, 1) if stats else (4,):
                assert {(W, "idle"), (W, "full-only"), (W, "partial-only")} <= cov, (cus, W)
                assert not any(lb[1] in ("second-full", "second-partial", "full+partial")
                               for lb in cov if lb[0] == W), (cus, W)
        out.append(bpc)
    return tuple(out)


def required(stats):
    """Every label of the traversal: what table T must reach."""
    out = {("head", h, False) for h in range(4)} | {("head", 1, True), ("head", 2, True)}
    out |= {("tail", t) for t in range(4)} | {("nbody", 0), ("nbody", 1)}
    out |= {("align", m, n) for m in range(4) for n in range(1, 10)}
    for W in (4, 1) if stats else (4,):
        out |= {(W, s) for s in ("full-only", "full+partial", "partial-only", "idle")}
        out |= {(W, "ends-in", u) for u in range(UNROLL)}
        out |= {(W, "ends-on", j) for j in range(1, UNROLL + 1)}
        out |= {(W, s, r) for s in ("second-full", "second-partial") for r in (False, True)}
    if stats:
        out |= {("pair", g, t) for g in range(4) for t in range(4)}
    return out


# ------------------------------------------------------------------- table T
K_T = 3
GUARD_WORDS = 8
CLIP_BPC = (1, 2, 3, 7, 1024)    # and 0: the device's default
STATS_BPC = (1, 2, 3, 7, 256)    # and 0
CLIP_LIMIT, STATS_LIMIT = 1024, 256   # BDL_CLIP_ / BDL_STATS_MAX_BLOCKS_PER_CHAIN
BODY_UNITS = (1, 255, 256, 257, 511, 512, 513, 768, 1023, 1024, 1025)
BIG_UNITS = 4 * K_ITER + 300     # b = 1: a full second trip at bpc = 2, a partial one at bpc = 3


def _segments_t():
    segs = []
    # the alignment matrix: in "tensor" placement chains 1.. shift by numel again
    for m in range(4):
        for n in range(1, 10):
            segs.append((f"m{m}n{n}", n, m, m))
    # body shapes on the 16-B path: head 4 - m, tail m, numel a multiple of 4 (every chain alike)
    for j, nb in enumerate(BODY_UNITS):
        m = j % 4
        segs.append((f"b4_{nb}", 4 * nb + (4 if m else 0), m, m))
    # body shapes on the element-wise path in "tensor" placement (chain 0: 1 against 0)
    for nu in BODY_UNITS:
        segs.append((f"b1_{nu}", nu, 1, 0))
    segs.append(("big1", BIG_UNITS, 1, 0))                 # numel % 4 == 0: W = 1 in every chain
    segs.append(("big4a", 1 + 4 * BIG_UNITS + 3, 3, 3))    # odd index; every chain on the 16-B path
    segs.append(("big4b", 2 + 4 * BIG_UNITS + 1, 2, 2))    # even index; chains 1, 2 element-wise
    return segs


SEGMENTS_T = _segments_t()


class PlacedT:
    """Table T placed in an arena of 32-bit words (guard words before, between
    and after everything).  form "tensor": every segment its own [K, numel]
    block (chain stride = numel) whose base is gmis elements past a 16-B
    boundary; "flat": one [K, slot] vector, segment i at the chain-local offset
    the stacked vectors use (offset % 4 = tmis), chain stride = slot.

      offsets, slot   the stacked vectors' layout (gaps and padding between
                      segments belong to no segment)
      segs            [(arena offset, numel, chain stride)] of the gradient
      total           the arena's size in words
    """

    def __init__(self, form, K=K_T):
        self.form, self.K = form, K
        self.names = [s[0] for s in SEGMENTS_T]
        self.numels = [s[1] for s in SEGMENTS_T]
        self.offsets, pos = [], 0
        for _, n, _, tm in SEGMENTS_T:
            pos += (tm - pos) % 4
            self.offsets.append(pos)
            pos += n
        self.slot = (pos + 2 + 3) // 4 * 4
        self.chain_groups = self.slot // 4
        if form == "flat":
            self.segs = [(GUARD_WORDS + o, n, self.slot) for o, n in zip(self.offsets, self.numels)]
            self.total = GUARD_WORDS + K * self.slot + GUARD_WORDS
        else:
            assert form == "tensor", form
            self.segs, pos = [], GUARD_WORDS
            for _, n, gm, _ in SEGMENTS_T:
                self.segs.append((pos + gm, n, n))
                pos = (pos + gm + K * n + GUARD_WORDS + 3) // 4 * 4
            self.total = pos

    def rows(self, stats=False):
        """The table in the restatement's form (the arena's base is 16-B aligned)."""
        if stats:
            return [(a % 4, n, s, o % 4) for (a, n, s), o in zip(self.segs, self.offsets)]
        return [(a % 4, n, s) for a, n, s in self.segs]

    def index(self, name):
        return self.names.index(name)

    def span(self, i, k):
        """Arena slice of chain k's slice of segment i."""
        a, n, s = self.segs[i]
        return slice(a + k * s, a + k * s + n)

    def vec_span(self, i, k):
        """Slice of a flattened [K, slot] stacked vector."""
        o = k * self.slot + self.offsets[i]
        return slice(o, o + self.numels[i])


def element_of(pt, i, k, bpc, kind, *, trip=0, sub=0, lane=0, stats=False):
    """The slice-local element index that a given traversal path of (segment
    i, chain k) reads at geometry bpc — where the planted-value runs put their
    single large element:

      "head" / "tail"   lane `lane` of the head / tail lanes
      "full"            rotation workgroup b = 1's full trip number `trip`
      "partial"         sub-block `sub` of the partial iteration of whichever
                        workgroup has one

    Returns None when the path does not exist there."""
    row = pt.rows(stats)[i]
    mk, numel, _, W = _path(row, k)
    h = split(mk, numel)[0] if W == 4 else 0
    if kind in ("head", "tail"):
        v = visit(mk, numel, 0, bpc, W)
        if W != 4 or lane >= (v.head if kind == "head" else v.tail):
            return None
        return lane if kind == "head" else h + 4 * v.nunits + lane
    if kind == "full":
        b = 1 if bpc > 1 else 0
        v = visit(mk, numel, b, bpc, W)
        if v.idle or trip >= v.full:
            return None
        return h + W * ((b + trip * bpc) * K_ITER + 3 * K_BLOCK + lane)
    assert kind == "partial", kind
    for b in range(bpc):
        v = visit(mk, numel, b, bpc, W)
        if not v.idle and v.partial is not None:
            if lane >= v.partial[sub]:
                return None
            return h + W * (v.gb_partial + sub * K_BLOCK + lane)
    return None
