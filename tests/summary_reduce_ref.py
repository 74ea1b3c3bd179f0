"""Host restatement of the summary reduction — TEST INFRASTRUCTURE ONLY.

bdl_chain_diag, bdl_chain_ess and the two per-tensor tables report through one
reduction (bdl_chain_common.hpp: Extreme, combine, wave_combine, block_combine,
store_partial, finalize_summary).  This file restates it literally in NumPy,
vectorised over (workgroup, thread), so that a device summary can be compared
field for field with no tolerance, the fp64 sum as a bit pattern:

`owner` / `owner_layers` say which (workgroup, thread, trip, slot) evaluates an
element in the whole-vector sweeps (bdl_diag.hip, bdl_ess.hip) and in
bdl_layers_kernel; `reduce` takes the per-element values through the lane's
sequential count_value, the six butterfly steps (the lower lane's value first),
waves 0..3, the partial per workgroup, the finalize threads' t, t + 256, ..
loop from empty(), the butterfly and the waves again and the empty convention.
It also returns a trace: which level decided between two candidates that both
hold the final extreme, and whether the lower index arrived as `combine`'s
first argument ("a") or its second ("b") — the second is what needs the
`b.arg < a.arg` clause.  `ties_whole` / `ties_layers` build pairs of elements
that land on each level, and BREAKS are wrong reductions applied to this
restatement only (nothing is built for a device).

Nothing is imported from bayesdll_amd and nothing from torch.
"""
from __future__ import annotations

import numpy as np

import layers_ref as LR

F = np.float32
K_BLOCK = LR.K_BLOCK      # threads per workgroup, one float4 group a lane and block iteration
WAVE = 64
WAVES = K_BLOCK // WAVE
OFFSETS = (32, 16, 8, 4, 2, 1)
I64_MAX = np.iinfo(np.int64).max
MAX_GRID = 2048           # kMaxDiagPartials, BDL_ESS_MAX_GRID

COUNTS = ("n_eval", "n_deg", "n_nonf", "hit0", "hit1", "hit2")
FIELDS = COUNTS + ("arg", "sum", "ext")
DTYPES = dict({f: np.int64 for f in COUNTS}, arg=np.int64, sum=np.float64, ext=F)

# label of every level at which two equal candidates can meet
LEVELS = (("lane",) + tuple(f"bfly{o}" for o in OFFSETS) + ("wave",)
          + tuple(f"fin_trip{k}" for k in range(2, MAX_GRID // K_BLOCK + 1))
          + tuple(f"fbfly{o}" for o in OFFSETS) + ("fwave",))

# wrong reductions (the break table of tests/test_summary_reduce_host.py)
BREAKS = ("first_wins", "last_wins", "same_order", "fin_stride64", "fin_one_trip",
          "waves_reversed")


# ------------------------------------------------------------------ geometry
def block_iters(n):
    """bdl_chain_common.hpp block_iters(n, kBlock)."""
    return ((n + 3) // 4 + K_BLOCK - 1) // K_BLOCK


def grid_ess(n, grid_blocks, cus):
    """bdl_chain_ess's grid: grid_blocks, or two workgroups per CU, at most 2048."""
    cap = grid_blocks if grid_blocks > 0 else min(cus * 2, MAX_GRID)
    return max(1, min(block_iters(n), cap))


def grid_diag(n, blocks_per_cu, cus):
    """bdl_chain_diag's grid: blocks_per_cu (0: 2) workgroups per CU, at most 2048."""
    cap = min(cus * (blocks_per_cu if blocks_per_cu > 0 else 2), MAX_GRID)
    return max(1, min(block_iters(n), cap))


def grid_layers(grid_blocks, cus):
    """bdl_layers.hip layers_grid."""
    return grid_blocks if grid_blocks > 0 else max(1, min(cus * 2, 1024))


def _new_owner(size):
    own = {k: np.full(size, -1, np.int64) for k in ("idx", "wg", "thread", "trip", "slot", "seq")}
    own["guarded"] = np.zeros(size, bool)
    own["count"] = np.zeros(size, np.int64)
    return own


def _own(own, pos, *, idx, wg, thread, trip, slot, seq, guarded=False):
    own["count"][pos] += 1            # positions are distinct within one call
    for k, v in (("idx", idx), ("wg", wg), ("thread", thread), ("trip", trip), ("slot", slot),
                 ("seq", seq)):
        own[k][pos] = v
    own["guarded"][pos] = guarded


def owner(n, grid):
    """Who evaluates element e of [0, n) in bdl_chain_diag_kernel /
    bdl_chain_ess_kernel on `grid` workgroups: arrays wg, thread, trip, slot
    (j of the float4 group), guarded (the group ran in the guarded iteration),
    seq (the element's place in its lane's program order), idx (the index the
    lane reports: e) and count (how often e was evaluated).  Restates

        gb = blockIdx.x * 256; stride = gridDim.x * 256
        for (; gb + 256 <= nfull; gb += stride) group<false>(gb + threadIdx.x)
        if (gb < ngroups) { gi = gb + threadIdx.x; if (gi < ngroups) group<true>(gi) }

    for all (workgroup, thread) at once, one trip of the loop at a time."""
    n, grid = int(n), int(grid)
    ngroups, nfull = (n + 3) >> 2, n >> 2
    stride = grid * K_BLOCK
    own = _new_owner(n)
    own["nwg"] = grid
    wg = np.repeat(np.arange(grid, dtype=np.int64), K_BLOCK)
    t = np.tile(np.arange(K_BLOCK, dtype=np.int64), grid)
    gb = wg * K_BLOCK
    live = np.ones(grid * K_BLOCK, bool)     # the lane has not left the loop yet
    trip = 0
    while live.any():
        full = live & (gb + K_BLOCK <= nfull)
        for j in range(4):
            e = 4 * (gb[full] + t[full]) + j
            _own(own, e, idx=e, wg=wg[full], thread=t[full], trip=trip, slot=j, seq=4 * trip + j)
        tail = live & ~full                  # the loop ended: the guarded iteration, once
        gi = gb + t
        for j in range(4):
            m = tail & (gb < ngroups) & (gi < ngroups) & (4 * gi + j < n)
            e = 4 * gi[m] + j
            _own(own, e, idx=e, wg=wg[m], thread=t[m], trip=trip, slot=j, seq=4 * trip + j,
                 guarded=True)
        live = full
        gb = gb + stride
        trip += 1
    return own


def owner_layers(segments, grid):
    """[owner of segment i] for bdl_layers_kernel on `grid` workgroups: as
    `owner`, over the segment's elements in ascending order (idx: the
    chain-local index the lane reports), with `kind` 0 / 1 / 2 for head / body /
    tail and `part` [grid]: the workgroup takes part in the segment (else it
    stores an empty partial).  The geometry is layers_ref's: split, rotated.

        b = rotated_block(i)
        if (b == 0 && t == 0 && h > 0)       group<true>(offset, h)
        for (g = b * 256 + t; g < nbody; g += stride) group<false>(body + 4 * g)
        if (b == 0 && t == 64 && tail > 0)   group<true>(body + 4 * nbody, tail)"""
    grid = int(grid)
    out = []
    w = np.repeat(np.arange(grid, dtype=np.int64), K_BLOCK)
    t = np.tile(np.arange(K_BLOCK, dtype=np.int64), grid)
    for i, (o, m) in enumerate(segments):
        o, m = int(o), int(m)
        h, nbody, tail = LR.split(o, m)
        own = _new_owner(m)
        own["kind"] = np.full(m, -1, np.int64)
        own["nwg"] = grid
        b1 = np.array([LR.rotated(v, i, grid) for v in range(grid)], dtype=np.int64)
        own["part"] = (b1 == 0) | (b1 * K_BLOCK < nbody)
        b = np.repeat(b1, K_BLOCK)
        first = int(np.flatnonzero(b1 == 0)[0])
        for j in range(h):
            _own(own, j, idx=o + j, wg=first, thread=0, trip=-1, slot=j, seq=j)
            own["kind"][j] = 0
        g = b * K_BLOCK + t
        trip = 0
        while (g < nbody).any():
            live = g < nbody
            for j in range(4):
                pos = h + 4 * g[live] + j
                _own(own, pos, idx=o + pos, wg=w[live], thread=t[live], trip=trip, slot=j,
                     seq=4 + 4 * trip + j)
                own["kind"][pos] = 1
            g = g + grid * K_BLOCK
            trip += 1
        for j in range(tail):
            pos = h + 4 * nbody + j
            _own(own, pos, idx=o + pos, wg=first, thread=WAVE, trip=trip, slot=j,
                 seq=4 + 4 * trip + j)
            own["kind"][pos] = 2
        out.append(own)
    return out


def big_table():
    """Three tensors of at least 600 x 1024 elements at misalignments 1, 2 and
    3 (two small ones make the gaps; the first is the frozen, degenerate row):
    at 3 workgroups every lane makes 200 trips, at 512 every workgroup takes
    part with a second trip for some, at 1024 some workgroups stay idle."""
    return LR.Table([("g0", 1), ("s0", 600 * 1024 + 3), ("g1", 2), ("s1", 600 * 1024 + 1),
                     ("s2", 601 * 1024)], "g0")


def sub_owner(own, positions):
    """`own` restricted to the elements at `positions` (of its arrays): for
    the trace of a strict extreme, which no other element can take part in."""
    pos = np.asarray(positions, dtype=np.int64)
    return {k: (v[pos] if isinstance(v, np.ndarray) and k != "part" else v) for k, v in own.items()}


# ----------------------------------------------------------------- reduction
def _empty(shape, maximum):
    s = {f: np.zeros(shape, DTYPES[f]) for f in FIELDS}
    s["arg"][...] = I64_MAX
    s["ext"][...] = F(-1.0) if maximum else F(np.inf)
    return s


def _take(s, index):
    return {f: s[f][index] for f in FIELDS}


def _where(m, s, o):
    return {f: np.where(m, s[f], o[f]) for f in FIELDS}


def _beyond(x, y, maximum):
    return x > y if maximum else x < y


class _Ctx:
    def __init__(self, maximum, final, breaks):
        self.maximum, self.final, self.breaks = maximum, final, frozenset(breaks)
        unknown = self.breaks - set(BREAKS)
        assert not unknown, unknown
        self.trace, self.marks = set(), set()


def _combine(a, b, ctx, label):
    """Extreme's combine(a, b), element-wise over arrays of summaries."""
    r = {f: a[f] + b[f] for f in COUNTS}
    r["sum"] = a["sum"] + b["sum"]
    equal = b["ext"] == a["ext"]
    if "first_wins" in ctx.breaks:
        among = np.zeros_like(equal)
    elif "last_wins" in ctx.breaks:
        among = np.ones_like(equal)
    else:
        among = b["arg"] < a["arg"]
    take = _beyond(b["ext"], a["ext"], ctx.maximum) | (equal & among)
    r["ext"] = np.where(take, b["ext"], a["ext"])
    r["arg"] = np.where(take, b["arg"], a["arg"])
    if ctx.final is not None:
        tie = equal & (a["n_eval"] > 0) & (b["n_eval"] > 0) & (a["ext"] == ctx.final)
        if tie.any():
            low_a = a["arg"][tie] < b["arg"][tie]
            if low_a.any():
                ctx.trace.add((label, "a"))
            if (~low_a).any():
                ctx.trace.add((label, "b"))
    return r


def _wave_combine(s, ctx, prefix):
    """wave_combine on arrays shaped [.., 64]: off = 32 .. 1, both partners
    form combine(lower lane's value, higher lane's value)."""
    lane = np.arange(WAVE)
    for off in OFFSETS:
        o = _take(s, (Ellipsis, lane ^ off))
        low = (lane & off) == 0
        if "same_order" in ctx.breaks:       # combine(s, o) in both partners
            s = _combine(s, o, ctx, f"{prefix}bfly{off}")
        else:
            s = _combine(_where(low, s, o), _where(low, o, s), ctx, f"{prefix}bfly{off}")
    return s


def _block_combine(s, ctx, prefix):
    """block_combine on arrays shaped [blocks, 256]: thread 0's value."""
    s = {f: s[f].reshape(-1, WAVES, WAVE) for f in FIELDS}
    s = _wave_combine(s, ctx, prefix)
    waves = [_take(s, (slice(None), w, 0)) for w in range(WAVES)]
    if "waves_reversed" in ctx.breaks:
        waves = waves[::-1]
    r = waves[0]
    for w in range(1, WAVES):
        r = _combine(r, waves[w], ctx, f"{prefix}wave")
    return r


def _lanes(values, own, deg, nonf, thr, ctx, wgs):
    """Every lane's count_value over its elements in program order, for the
    workgroups `wgs` (ascending; they include every owner)."""
    s = _empty(wgs.size * K_BLOCK, ctx.maximum)
    n = values.size
    if n == 0:
        return s
    lane = np.searchsorted(wgs, own["wg"]) * K_BLOCK + own["thread"]
    order = np.lexsort((own["seq"], lane))
    ls = lane[order]
    starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
    counts = np.diff(np.r_[starts, n])
    lanes = ls[starts]
    for k in range(int(counts.max())):
        on = counts > k
        e, L = order[starts[on] + k], lanes[on]
        d, nf = deg[e], nonf[e]
        s["n_deg"][L] += d
        s["n_nonf"][L] += nf
        ev = ~d & ~nf
        e, L = e[ev], L[ev]
        x = values[e]
        s["n_eval"][L] += 1
        s["sum"][L] += x.astype(np.float64)
        for h in range(3):
            s[f"hit{h}"][L] += _beyond(x, thr[h], ctx.maximum)
        if ctx.final is not None and ((x == s["ext"][L]) & (x == ctx.final)).any():
            ctx.trace.add(("lane", "a"))      # a lane's elements ascend: the incumbent is lower
        up = _beyond(x, s["ext"][L], ctx.maximum)
        s["ext"][L[up]] = x[up]
        s["arg"][L[up]] = own["idx"][e[up]]
    return s


def _finalize(parts, ctx):
    """finalize_summary: one workgroup over the partials."""
    nparts = parts["n_eval"].size
    s = _empty(K_BLOCK, ctx.maximum)
    step = WAVE if "fin_stride64" in ctx.breaks else K_BLOCK
    t = np.arange(K_BLOCK)
    k = 0
    while True:
        i = t + k * step
        on = i < nparts
        if not on.any() or (k > 0 and "fin_one_trip" in ctx.breaks):
            break
        a, b = _take(s, t[on]), _take(parts, i[on])
        if k > 0 and ((a["n_eval"] == 0) & (b["n_eval"] > 0)).any():
            ctx.marks.add("fin_empty_then_value")
        r = _combine(a, b, ctx, f"fin_trip{k + 1}")
        for f in FIELDS:
            s[f][t[on]] = r[f]
        k += 1
    s = _block_combine(s, ctx, "f")
    s = {f: s[f][0] for f in FIELDS}
    if s["n_eval"] == 0:
        s["ext"], s["arg"] = F(0.0), np.int64(-1)
    return s


class Reduced:
    """reduce's result: `summary` (the public struct's fields under neutral
    names: n_eval, n_degenerate, n_nonfinite, hits, arg, sum, ext), `partials`
    (the same fields as arrays, one entry per workgroup), `trace` (a frozenset
    of (level, "a" | "b")) and `marks`."""

    def __init__(self, summary, partials, trace, marks):
        self.summary, self.partials, self.trace, self.marks = summary, partials, trace, marks


def public(s):
    return {"n_eval": s["n_eval"], "n_degenerate": s["n_deg"], "n_nonfinite": s["n_nonf"],
            "hits": np.stack([s["hit0"], s["hit1"], s["hit2"]], axis=-1), "arg": s["arg"],
            "sum": s["sum"], "ext": s["ext"]}


def sum_bits(x):
    """An fp64 value (or array) as its 64-bit pattern."""
    return np.asarray(x, dtype=np.float64).view(np.int64)


def reduce_variants(values, own, *, maximum, thresholds, degenerate, nonfinite, variants,
                    dense=False):
    """{breaks: Reduced} for every tuple of BREAKS in `variants` (() is the
    device's reduction): the lanes' sequential stage, which no break touches,
    runs once.  A workgroup that owns no element has the empty partial (256
    empty lanes combine to empty()); unless `dense`, its block_combine is not
    walked — the host test holds both ways equal."""
    values = np.ascontiguousarray(values, dtype=F)
    deg, nonf = np.asarray(degenerate, bool), np.asarray(nonfinite, bool)
    assert values.shape == deg.shape == nonf.shape == own["idx"].shape
    assert not (deg & nonf).any() and (own["count"] == 1).all()
    ev = values[~deg & ~nonf]
    assert np.isfinite(ev).all()
    final = (ev.max() if maximum else ev.min()) if ev.size else None
    thr = [F(float(v)) for v in thresholds]
    lane_ctx = _Ctx(maximum, final, ())
    wgs = np.arange(own["nwg"]) if dense else np.unique(own["wg"])
    lanes = _lanes(values, own, deg, nonf, thr, lane_ctx, wgs)
    out = {}
    for breaks in variants:
        ctx = _Ctx(maximum, final, breaks)
        ctx.trace |= lane_ctx.trace
        some = _block_combine({f: lanes[f].reshape(-1, K_BLOCK) for f in FIELDS}, ctx, "")
        parts = _empty(own["nwg"], maximum)
        for f in FIELDS:
            parts[f][wgs] = some[f]
        total = _finalize(parts, ctx)
        if not parts["n_eval"].all():
            ctx.marks.add("empty_partial")
        if "part" in own and not own["part"].all():
            ctx.marks.add("idle_workgroup")
        out[tuple(breaks)] = Reduced(public(total), public(parts), frozenset(ctx.trace),
                                     frozenset(ctx.marks))
    return out


def reduce(values, own, *, maximum, thresholds, degenerate, nonfinite, breaks=(), dense=False):
    """The device's summary of `values` (fp32, one per element of `own`, in
    its order): degenerate / nonfinite elements are counted and leave the
    statistics, every other one goes through count_value.  thresholds: three
    numbers, taken as fp32."""
    breaks = tuple(breaks)
    return reduce_variants(values, own, maximum=maximum, thresholds=thresholds,
                           degenerate=degenerate, nonfinite=nonfinite, variants=[breaks],
                           dense=dense)[breaks]


# ------------------------------------------------------------- planted ties
def elem(n, grid, wg, thread, trip, slot=0):
    """The element of a whole-vector sweep that (wg, thread) evaluates in
    `trip` at `slot`; None if there is no such element."""
    if wg >= grid:
        return None
    e = 4 * ((trip * grid + wg) * K_BLOCK + thread) + slot
    return e if e < n else None


def _pair(out, name, i, j):
    if i is not None and j is not None:
        assert i < j, (name, i, j)
        out.append((name, int(i), int(j)))


def _pair4(out, name, seg, i, j):
    if i is not None and j is not None:
        assert i < j, (name, seg, i, j)
        out.append((name, seg, int(i), int(j)))


def ties_whole(n, grid):
    """[(name, i, j)], i < j: pairs of elements of a whole-vector sweep of n
    elements on `grid` workgroups whose tie is decided at the level the name
    says — "<level>:a" with the lower index in combine's first argument (the
    lower lane / wave / workgroup / finalize thread owns the lower index),
    "<level>:b" with it in the second: the HIGHER lane, wave, workgroup or
    finalize thread owns trip 0 and the lower one trip 1.  Pairs that do not
    exist at this (n, grid) are left out; what a pair really reaches is
    `reduce`'s trace, asserted per case by the host test."""
    def at(wg, thread, trip, slot=0):
        return elem(n, grid, wg, thread, trip, slot)

    out = []
    w1 = 1 if at(1, K_BLOCK - 1, 0, 3) is not None else 0    # a whole first trip, off workgroup 0
    _pair(out, "group", at(0, 5, 0, 1), at(0, 5, 0, 3))
    _pair(out, "lane:a", at(w1, 7, 0, 2), at(w1, 7, 1, 1))
    g0 = 4 * K_BLOCK * ((n >> 2) // K_BLOCK)       # the guarded iteration's first element
    if g0 < n - 1:
        _pair(out, "guarded", g0, n - 1)
    for k, off in enumerate(OFFSETS):
        lo = WAVE * (k % WAVES) + WAVE - 2 * off     # bit `off` clear; the pair differs in it only
        _pair(out, f"bfly{off}:a", at(w1, lo, 0, 2), at(w1, lo + off, 0, 1))
        _pair(out, f"bfly{off}:b", at(0, lo + off, 0, 3), at(0, lo, 1, 0))
    _pair(out, "wave:a", at(w1, 3, 0, 1), at(w1, 2 * WAVE + 3, 0, 0))
    _pair(out, "wave:b", at(0, 3 * WAVE + 9, 0, 2), at(0, 9, 1, 2))
    for m in sorted({min(1, (grid - 1) // K_BLOCK), (grid - 1) // K_BLOCK} - {0}):
        t = min(5, grid - 1 - K_BLOCK * m)
        _pair(out, f"fin_trip{m + 1}:a", at(t, 11, 0), at(t + K_BLOCK * m, 10, 0))
        _pair(out, f"fin_trip{m + 1}:b", at(t + K_BLOCK * m, 200, 0, 1), at(t, 100, 1, 1))
    for k, off in enumerate(OFFSETS):
        lo = WAVE * ((k + 1) % WAVES) + WAVE - 2 * off
        if lo + off >= grid:
            lo = WAVE - 2 * off
        if lo + off >= grid:
            lo = 0
        _pair(out, f"fbfly{off}:a", at(lo, 17, 0), at(lo + off, 16, 0))
        _pair(out, f"fbfly{off}:b", at(lo + off, 130, 0, 2), at(lo, 70, 1, 2))
    _pair(out, "fwave:a", at(3, 255, 0, 3), at(WAVE + 3, 0, 0, 0))
    _pair(out, "fwave:b", at(3 * WAVE + 3, 33, 0), at(3, 33, 1))
    return out


def ties_layers(segments, grid, owns=None):
    """[(name, segment, i, j)], i < j chain-local: per segment, where they
    exist, a head lane against a body lane, a tail lane against a body lane of
    the wave beside it (the tail's lane 64 is the lower lane and holds the
    higher index: "b"), head against tail, two elements of one body lane, and
    the first elements of the segment's first two workgroups (rotated: for a
    segment index that is no multiple of the grid the first workgroup is not
    workgroup 0, and where the rotation wraps the lower index sits in the
    higher workgroup)."""
    out = []
    for s, own in enumerate(owner_layers(segments, grid) if owns is None else owns):
        idx, kind = own["idx"], own["kind"]
        head, body, tail = (np.flatnonzero(kind == k) for k in range(3))

        def first(mask):
            p = np.flatnonzero(mask)
            return int(idx[p[0]]) if p.size else None

        w0 = int(own["wg"][body[0]]) if body.size else -1     # the rotated first workgroup
        in0 = (kind == 1) & (own["wg"] == w0)
        if head.size:
            _pair4(out, "head-body", s, int(idx[head[0]]), first(in0 & (own["thread"] == 1)))
        if tail.size:
            tb = first(in0 & (own["thread"] == WAVE + 1))
            if tb is None:
                tb = first(in0 & (own["thread"] == 3))
            _pair4(out, "tail-body", s, tb, int(idx[tail[-1]]))
        if head.size and tail.size:
            _pair4(out, "head-tail", s, int(idx[head[-1]]), int(idx[tail[0]]))
        if body.size >= 4:
            _pair4(out, "body-group", s, int(idx[body[1]]), int(idx[body[3]]))
        nxt = (kind == 1) & (own["wg"] == (w0 + 1) % grid) & (own["trip"] == 0)
        if grid > 1:
            _pair4(out, "two-workgroups", s, first(in0 & (own["thread"] == 77)),
                   first(nxt & (own["thread"] == 78)))
    return out
