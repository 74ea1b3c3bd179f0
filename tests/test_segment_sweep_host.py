"""The restatement of the clip / statistics traversal (tests/segment_sweep_ref.py)
checked on its own, what table T reaches proven on the CPU, what tables A and B
do not reach pinned, and the clip coefficient's conventions.  No GPU:
tests/test_gpu_segment_sweeps.py launches the kernels on T.

* restatement against brute force: the loops of bdl_chain_sqnorm_kernel /
  sweep_units walked literally (workgroup by workgroup, iteration by iteration,
  lane by lane); every element of every chain slice is taken exactly once and
  the restatement's counts equal the walk's, at every geometry the GPU tests
  launch.
* coverage of T: every label of segment_sweep_ref.required, and which
  geometry contributes the rotated second trips.
* tables A and B: the exact set of labels they miss.
* blocks_per_chain = 0 at 256 and 304 compute units.
* step_ref.clip_coef at NaN, inf, 0 and on either side of max_norm.
"""
import numpy as np
import pytest

import segment_sweep_ref as SR
import step_ref
from layers_ref import rotated

F = np.float32
CUS = (256, 304)


# ---------------------------------------------------------------- brute force
def walk(mis_k, numel, b, bpc, W):
    """The kernel text for one (chain slice, workgroup): returns (the element
    indices it takes, in order, with repeats; head lanes; tail lanes; full
    iterations; lanes per sub-block of the partial iteration or None; idle)."""
    taken, hl, tl = [], [], []
    if W == 4:
        h0 = (4 - mis_k) & 3
        h = h0 if h0 < numel else numel
        nunits = (numel - h) >> 2
        tail = numel - h - 4 * nunits
    else:
        h, nunits, tail = 0, numel, 0
    idle = not (b == 0 or b * SR.K_ITER < nunits)   # bdl_stats.hip `work`; the clip: no loop runs
    stride = bpc * SR.K_ITER
    gb, full, partial = b * SR.K_ITER, 0, None
    while gb + SR.K_ITER <= nunits:
        for u in range(SR.UNROLL):
            first = gb + u * 256
            taken.append(h + W * np.arange(first, first + 256)[:, None] + np.arange(W)[None, :])
        full += 1
        gb += stride
    if gb < nunits:
        partial = []
        for u in range(SR.UNROLL):
            gi = gb + u * 256 + np.arange(256)
            gi = gi[gi < nunits]
            partial.append(len(gi))
            taken.append(h + W * gi[:, None] + np.arange(W)[None, :])
        partial = tuple(partial)
    if b == 0 and W == 4:
        for t in range(256):
            if t < h:
                hl.append(t)
                taken.append(np.array([t]))
            elif t >= 4 and t - 4 < tail:
                tl.append(t)
                taken.append(np.array([h + 4 * nunits + (t - 4)]))
    flat = np.concatenate([a.reshape(-1) for a in taken]) if taken else np.zeros(0, dtype=np.int64)
    if idle:
        assert flat.size == 0
    return flat, tuple(hl), tuple(tl), full, partial, idle


def _check_against_walk(rows, K, bpc):
    sw = SR.sweep(rows, K, bpc)
    for i, row in enumerate(rows):
        for k in range(K):
            mk, numel, _, W = SR._path(row, k)
            count = np.zeros(numel, dtype=np.int64)
            for w in range(bpc):
                b = rotated(w, i, bpc)
                v = sw[k, w, i]
                if b != 0 and b * SR.K_ITER >= numel:   # past every unit on either path
                    assert v.idle, (i, k, w)
                    continue
                flat, hl, tl, full, partial, idle = walk(mk, numel, b, bpc, W)
                assert flat.size == 0 or (flat.min() >= 0 and flat.max() < numel), (i, k, w)
                np.add.at(count, flat, 1)
                assert (v.idle, SR.head_lanes(v), SR.tail_lanes(v), v.full, v.partial) == \
                    (idle, hl, tl, full, partial), (i, k, w, v)
                assert v.W == W and v.b == b
            assert (count == 1).all(), (i, k, bpc, np.flatnonzero(count != 1)[:8])


@pytest.mark.parametrize("form", ["tensor", "flat"])
@pytest.mark.parametrize("stats", [False, True])
def test_restatement_equals_the_walked_kernel_text_on_t(form, stats):
    pt = SR.PlacedT(form)
    rows = pt.rows(stats)
    lim = SR.STATS_LIMIT if stats else SR.CLIP_LIMIT
    geos = set(SR.STATS_BPC if stats else SR.CLIP_BPC) | {SR.default_bpc(c, SR.K_T, lim) for c in CUS}
    for bpc in sorted(geos):
        _check_against_walk(rows, SR.K_T, bpc)


def test_restatement_on_hand_counted_slices():
    v = SR.visit(1, 2, 0, 1)                     # numel 2 < head 3: capped, nothing else
    assert (v.head, v.capped, v.tail, v.nunits, v.full, v.partial) == (2, True, 0, 0, 0, None)
    v = SR.visit(3, 9, 0, 2)                     # head 1, two groups, no tail
    assert (v.head, v.capped, v.tail, v.nunits, v.partial) == (1, False, 0, 2, (2, 0, 0, 0))
    assert SR.visit(3, 9, 1, 2).idle
    v = SR.visit(0, 4 * (4 * 1024 + 300), 1, 2)  # b = 1 of 2: iterations 1 and 3, no partial
    assert (v.full, v.partial) == (2, None)
    v = SR.visit(0, 4 * (4 * 1024 + 300), 1, 3)  # b = 1 of 3: iteration 1, then 300 units of 4
    assert (v.full, v.partial, v.gb_partial) == (1, (256, 44, 0, 0), 4096)
    v = SR.visit(2, 1025, 0, 1, W=1)             # element-wise: no head, one full, one lane
    assert (v.head, v.tail, v.nunits, v.full, v.partial) == (0, 0, 1025, 1, (1, 0, 0, 0))
    assert SR.head_lanes(SR.visit(1, 9, 0, 1)) == (0, 1, 2)
    assert SR.tail_lanes(SR.visit(1, 9, 0, 1)) == (4, 5)
    assert SR.default_bpc(256, 3, 1024) == 342 and SR.default_bpc(256, 3, 256) == 256
    assert SR.default_bpc(304, 3, 1024) == 406 and SR.default_bpc(1, 64, 1024) == 1


# ------------------------------------------------------------- coverage of T
def _covered(rows, K, geos):
    return {bpc: SR.covered(rows, K, bpc) for bpc in geos}


def test_table_t_holds_what_it_claims():
    names = [s[0] for s in SR.SEGMENTS_T]
    assert len(names) == len(set(names)) == 36 + 2 * len(SR.BODY_UNITS) + 3
    assert set(SR.BODY_UNITS) >= {1, 255, 256, 257, 511, 513, 1023, 1024, 1025}
    assert {(m, n) for _, n, m, t in SR.SEGMENTS_T[:36]} == {(m, n) for m in range(4)
                                                            for n in range(1, 10)}
    a, b = names.index("big4a"), names.index("big4b")
    assert a % 2 == 1 and b % 2 == 0
    for form in ("tensor", "flat"):
        pt = SR.PlacedT(form)
        assert pt.total * 4 < 1 << 20 and pt.slot % 4 == 0
        assert all(o % 4 == s[3] for o, s in zip(pt.offsets, SR.SEGMENTS_T))
        assert pt.offsets[-1] + pt.numels[-1] <= pt.slot - 2   # padding in every slot
        spans = sorted((x + k * s, x + k * s + n) for x, n, s in pt.segs for k in range(pt.K))
        assert spans[0][0] >= SR.GUARD_WORDS and spans[-1][1] <= pt.total - SR.GUARD_WORDS
        assert all(e0 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:]))   # no overlap
        for i in (a, b):   # both large segments: >= 4 block iterations + 300 units on the 16-B path
            assert SR.visit(pt.rows()[i][0], pt.numels[i], 0, 1).nunits >= SR.BIG_UNITS
        if form == "tensor":
            assert all(x % 4 == s[2] and st == n for (x, n, st), s in zip(pt.segs, SR.SEGMENTS_T))
        else:
            assert all((x - SR.GUARD_WORDS) == o for (x, _, _), o in zip(pt.segs, pt.offsets))


@pytest.mark.parametrize("form", ["tensor", "flat"])
def test_t_reaches_every_clip_path(form):
    cov = _covered(SR.PlacedT(form).rows(), SR.K_T, SR.CLIP_BPC)
    missing = SR.required(False) - set().union(*cov.values())
    assert not missing, sorted(missing, key=str)
    # the rotated second trips come from b = 1 at two and three workgroups per chain
    assert (4, "second-full", True) in cov[2] and (4, "second-partial", True) in cov[3]
    assert (4, "second-full", True) not in cov[1] and (4, "idle") not in cov[1]
    assert (4, "idle") in cov[1024]


def test_t_reaches_every_stats_path():
    rows = SR.PlacedT("tensor").rows(True)
    cov = _covered(rows, SR.K_T, SR.STATS_BPC)
    missing = SR.required(True) - set().union(*cov.values())
    assert not missing, sorted(missing, key=str)
    assert (4, "second-full", True) in cov[2] and (4, "second-partial", True) in cov[3]
    # element-wise: big1 (b = 1 of 3: one full trip, then the partial one) and
    # chains 1, 2 of big4b (17 iterations over 7 workgroups)
    assert (1, "second-partial", True) in cov[3] and (1, "second-full", True) in cov[7]
    assert {lb for lb in cov[1] if lb[0] == "pair"} == {("pair", g, t) for g in range(4)
                                                        for t in range(4)}
    # 4 pairs are equal (each head length 0..3 on the 16-B path), 12 element-wise
    sw = SR.sweep(rows, SR.K_T, 1)
    assert {v.head for v in sw.values() if v.W == 4 and not v.capped and v.nunits} == {0, 1, 2, 3}
    # the flat form never leaves the 16-B path: its labels are the clip's plus the equal pairs
    flat = _covered(SR.PlacedT("flat").rows(True), SR.K_T, SR.STATS_BPC)
    got = set().union(*flat.values())
    assert not any(lb[0] == 1 for lb in got)
    assert SR.required(False) <= got and {("pair", m, m) for m in range(4)} <= got


@pytest.mark.parametrize("cus", CUS)
def test_default_geometry_reaches_idle_and_single_trip_paths(cus):
    """blocks_per_chain = 0 at 256 and 304 compute units (the GPU test repeats
    it for the device's count)."""
    assert SR.check_default_geometry(cus) == (-(-4 * cus // 3), 256)
    assert SR.check_default_geometry(8) == (11, 11)   # a small device: second trips remain


def test_coverage_would_notice_a_missing_segment():
    pt = SR.PlacedT("tensor")
    rows = pt.rows()
    small = [r for r in rows if r[1] < 4 * SR.BIG_UNITS]
    got = set().union(*_covered(small, SR.K_T, SR.CLIP_BPC).values())
    assert (4, "second-full", True) in SR.required(False) - got
    no_matrix = SR.PlacedT("flat").rows()[36:]
    got = set().union(*_covered(no_matrix, SR.K_T, SR.CLIP_BPC).values())
    assert ("head", 1, True) in SR.required(False) - got


# ----------------------------------------------------------- tables A and B
def _clip_rows_ab(name):
    import test_gpu_chain_clip as TC
    from stacked_tables import Layout
    segments, K_, mode = TC.CASES[name]
    segs, _ = TC._place(Layout(segments, K_), mode)
    return [(a % 4, n, s) for a, n, s in segs], K_


def _stats_rows_a(form):
    import test_gpu_chain_stats as TS
    lay, idx = TS._layout()
    rows, pos = [], 8
    for i in idx:
        o, n = lay.offsets[i], lay.numels[i]
        if form == "flat":
            rows.append((o % 4, n, lay.stride, o % 4))
        else:   # _Device: blocks 16-B aligned, guard words between
            rows.append((pos % 4, n, n, o % 4))
            pos = (pos + TS.K_ * n + 8 + 3) // 4 * 4
    return rows, TS.K_


CLIP_AB_ALIGN = {(0, 3), (0, 4), (0, 5), (0, 8), (1, 5), (2, 3), (2, 5), (3, 3), (3, 5)}
CLIP_AB_MISSING = {
    ("head", 1, True), ("head", 2, True),
    (4, "ends-in", 2), (4, "ends-in", 3), (4, "ends-on", 2), (4, "ends-on", 3), (4, "ends-on", 4),
    (4, "second-full", True), (4, "second-partial", True)}
STATS_A_ALIGN = {(0, 3), (0, 4), (0, 8), (3, 5)}
STATS_A_MISSING = CLIP_AB_MISSING - {(4, "ends-on", 4)} | {
    ("head", 3, False),
    ("pair", 0, 1), ("pair", 1, 0), ("pair", 1, 1), ("pair", 1, 2), ("pair", 2, 1), ("pair", 3, 1),
    (1, "ends-in", 1), (1, "ends-in", 2), (1, "ends-in", 3),
    (1, "ends-on", 1), (1, "ends-on", 2), (1, "ends-on", 3), (1, "ends-on", 4),
    (1, "second-partial", False)}


def _missing(got, stats, align):
    missing = SR.required(stats) - got
    print("misses", len(missing), sorted(missing, key=str))
    assert {lb[1:] for lb in SR.required(stats) & got if lb[0] == "align"} == align
    return {lb for lb in missing if lb[0] != "align"}


def test_what_the_clip_tests_on_a_and_b_do_not_reach():
    """The exact set of traversal labels that tests/test_gpu_chain_clip.py's
    launches (tables A and B, both placements, one chain and several,
    blocks_per_chain 1, 7, 1024 and the default of a 256-CU device) never
    reach: no capped head, 9 of the 36 (misalignment, numel <= 9) slices, no
    partial iteration ending in its upper half or on a boundary, no rotated
    workgroup's second trip.  A change of those tables shows here."""
    got = set()
    for name in ("A-tensor", "A-flat", "B-tensor", "one-chain", "one-chain-flat"):
        rows, K_ = _clip_rows_ab(name)
        for bpc in (1, 7, 1024, SR.default_bpc(256, K_, SR.CLIP_LIMIT)):
            got |= SR.covered(rows, K_, bpc)
    assert _missing(got, False, CLIP_AB_ALIGN) == CLIP_AB_MISSING


def test_what_the_stats_tests_on_a_do_not_reach():
    """The same for tests/test_gpu_chain_stats.py (table A plus the 4,099-element
    tensor, both gradient forms, blocks_per_chain 1, 3, 5 and the default): 6
    of the 16 misalignment pairs, head 3, and on the element-wise path every
    partial iteration but one that ends in sub-block 0."""
    got = set()
    for form in ("tensor", "flat"):
        rows, K_ = _stats_rows_a(form)
        for bpc in (1, 3, 5, SR.default_bpc(256, K_, SR.STATS_LIMIT)):
            got |= SR.covered(rows, K_, bpc)
    assert _missing(got, True, STATS_A_ALIGN) == STATS_A_MISSING


# ------------------------------------------------------- the clip coefficient
def test_clip_coef_conventions():
    """include/bdl_clip.h: coef = fminf(fl32(fl32(1 / fl32(norm + 1e-6f)) * max_norm), 1), and
    fminf returns its other operand for a NaN: a NaN norm gives 1, the chain is
    left untouched (torch.nn.utils.clip_grad_norm_ would multiply by NaN)."""
    c = step_ref.clip_coef
    one = F(1.0)
    for mx in (1e-7, 0.75, 1.0, 3e38):
        got = c(F(np.nan), mx)
        assert type(got) is F and got == one, mx
    assert c(F(np.inf), 0.75) == F(0.0) and not np.signbit(c(F(np.inf), 0.75))
    assert c(F(0.0), 1.0) == one                      # 1e6 * 1 clamped
    assert c(F(0.0), 1e-7) == F(1.0) / F(1e-6) * F(1e-7) < one   # 1e6 * 1e-7: a zero gradient "clipped"
    mx = F(0.75)
    below, above = np.nextafter(mx, F(0)), np.nextafter(mx, F(2))
    # the 1e-6 in the sum: clipping starts about 1e-6 (17 ulps) below max_norm, not at it
    assert c(below, mx) < one and c(mx, mx) < one and c(above, mx) < one
    assert c(above, mx) <= c(mx, mx) and c(F(0.75 - 3e-6), mx) == one
    for n in (below, mx, above):
        assert c(n, mx) == (one / (n + F(1e-6))) * mx
    assert c(F(0.5), 0.75) == one and c(F(3.0), 0.75) == (one / (F(3.0) + F(1e-6))) * mx
    for n in (0.0, 0.5, 0.75, 3.0, 1e30, np.inf, np.nan):
        got = c(F(n), 0.75)
        assert type(got) is F and not np.isnan(got) and F(0) <= got <= one
    # the stacked reference follows: a NaN chain is returned as it is
    import chain_clip_ref as CR
    g = np.array([1.0, np.nan, -2.0], dtype=F)
    norms, coefs, scaled = CR.chain_clip([[g]], 0.75)
    assert np.isnan(norms[0]) and coefs[0] == one
    assert np.array_equal(scaled[0][0].view(np.int32), g.view(np.int32))
