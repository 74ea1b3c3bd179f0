"""The summary reduction of bdl_chain_diag, bdl_chain_ess and the per-tensor
tables on the GPU against its literal host restatement
(tests/summary_reduce_ref.py): every field of the summary and of every
workgroup's partial is equal, the fp64 sum as a 64-bit pattern — no tolerance
anywhere —, and a tie for the extreme planted at every level of the tree, in
both argument orders of `combine`, reports the lower index.

The grids are computed here from the device's CU count and the headers' rule
and asserted to reach the partial counts the cases are about (beyond 256, and
2048); nothing is skipped.  tests/test_summary_reduce_host.py shows on the CPU
which level every planted pair lands on.

K = 2 chains throughout.  The values span many binades (fp32 values of one
magnitude add up exactly in fp64 in any order, so they could not show the
order of the additions)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_diag_ref as DR
import chain_ess_ref as ER
import layers_ref as LR
import summary_reduce_ref as S
from test_gpu_chain_layers import DIAG, ESS, launch

pytestmark = pytest.mark.gpu

F = np.float32
K_ = 2
N_MID = 2 * 257 * 1024 + 1027
N_BIG = 2 * 2048 * 1024 + 7
ESS_CASES = [(1025, 0, 2), (3 * 1024 + 5, 3, 3), (N_MID, 257, 257), (N_BIG, 2048, 2048)]
SAMPLES, BATCHES, COUNT = 37, 9, 7
INT_FIELDS = ("n_eval", "n_degenerate", "n_nonfinite")


DIAG_KW = dict(var_mode=DR.VAR_GIVEN, ratio=1.0, inv_ratio=0.0, var_floor=0.0, count=COUNT)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------ host values
def ess_values(sM2, bM2, n, slot):
    """(ess, degenerate, nonfinite) per element, from the existing reference."""
    ess, _, summ = ER.chain_ess_f32(sM2, bM2, chains=K_, chain_groups=slot // 4, n=n,
                                    samples=SAMPLES, batches=BATCHES)
    deg = (bM2[:n] + bM2[slot:slot + n]) == 0            # SV == 0, K = 2
    with np.errstate(invalid="ignore"):
        nonf = ~deg & ~np.isfinite(ess)
    assert (int(deg.sum()), int(nonf.sum())) == (summ["n_degenerate"], summ["n_nonfinite"])
    return ess, deg, nonf


def diag_values(m1, m2, n, slot, kw):
    rh = DR.chain_diag_f32(m1, m2, chains=K_, chain_groups=slot // 4, n=n, **kw)
    rh, summ = rh[2], rh[3]
    with np.errstate(invalid="ignore", over="ignore"):
        d = m1[slot:slot + n] - m1[:n]
        deg = d * d == 0                                  # S2 == 0, K = 2
        nonf = ~deg & ~np.isfinite(rh)
    assert (int(deg.sum()), int(nonf.sum())) == (summ["n_degenerate"], summ["n_nonfinite"])
    return rh, deg, nonf


def one_element(first, second):
    """Two chains' inputs of one element (chain_groups = 1)."""
    return (np.array([first[0], 0, 0, 0, first[1], 0, 0, 0], F),
            np.array([second[0], 0, 0, 0, second[1], 0, 0, 0], F))


@functools.lru_cache(maxsize=None)
def ess_planted():
    """The planted ESS element's inputs and its value: far below every other."""
    one = one_element((2.0 ** -60, 2.0 ** -59), (5e-5, 5e-5))
    pv = ER.chain_ess_f32(*one, chains=K_, chain_groups=1, n=1, samples=SAMPLES, batches=BATCHES)[0][0]
    assert np.isfinite(pv) and pv > 0
    return one, pv


@functools.lru_cache(maxsize=None)
def diag_planted():
    """The planted R-hat element: chain means 2^30 apart."""
    one = one_element((1.0, 1.0 + 2.0 ** 30), (2e-3, 2e-3))
    pv = DR.chain_diag_f32(*one, chains=K_, chain_groups=1, n=1, **DIAG_KW)[2][0]
    assert np.isfinite(pv)
    return one, pv


@functools.lru_cache(maxsize=None)
def ess_case(n):
    """Accumulators of two chains whose ESS spans 40 binades, with degenerate
    (bM2 zero in both chains) and non-finite (sM2 infinite) elements."""
    rng = np.random.default_rng(n)
    cg = (n + 3) // 4
    slot = 4 * cg
    sM2 = np.full(K_ * slot, np.nan, F)
    bM2 = np.full(K_ * slot, np.nan, F)
    scale = 2.0 ** rng.integers(-20, 21, n)
    for k in range(K_):
        sM2[slot * k: slot * k + n] = rng.uniform(0.5, 2.0, n) * 1e-3 * scale
        bM2[slot * k: slot * k + n] = rng.uniform(0.5, 2.0, n) * 1e-5
    u = rng.random(n)
    for k in range(K_):
        bM2[slot * k: slot * k + n][u < 0.01] = 0.0
    sM2[:n][(u >= 0.01) & (u < 0.02)] = np.inf
    vals = ess_values(sM2, bM2, n, slot)
    assert vals[1].sum() > 0 or n < 2000
    one, pv = ess_planted()
    assert pv < vals[0][~vals[1] & ~vals[2]].min()
    for a in (sM2, bM2):
        a.setflags(write=False)
    return sM2, bM2, cg, vals, (one, pv)


@functools.lru_cache(maxsize=None)
def diag_case(n):
    """chain_diag_ref.make_case with the chains' difference scaled over 20
    binades in a third of the elements, frozen (degenerate) elements and
    elements of zero variance (var_floor = 0: R-hat infinite)."""
    rng = np.random.default_rng(n + 1)
    m1, m2, cg = DR.make_case(n, K_, n)
    slot = 4 * cg
    wide = np.flatnonzero(rng.random(n) < 0.33)
    m1[slot + wide] = m1[wide] + (0.05 * 2.0 ** rng.integers(0, 21, wide.size)).astype(F)
    u = rng.random(n)
    frozen = np.flatnonzero(u < 0.01)
    m1[slot + frozen] = m1[frozen]
    flat = np.flatnonzero((u >= 0.01) & (u < 0.02))
    for k in range(K_):
        m2[slot * k + flat] = 0.0
    vals = diag_values(m1, m2, n, slot, DIAG_KW)
    assert vals[1].sum() >= frozen.size and vals[2].sum() > 0
    one, pv = diag_planted()
    assert pv > vals[0][~vals[1] & ~vals[2]].max()
    for a in (m1, m2):
        a.setflags(write=False)
    return m1, m2, cg, vals, (one, pv)


def planted(vals, pv, pairs):
    """The host values with every (i, j) of `pairs` at the planted extreme."""
    v, deg, nonf = (a.copy() for a in vals)
    for e in pairs:
        v[e], deg[e], nonf[e] = pv, False, False
    return v, deg, nonf


# ----------------------------------------------------------- device calls
class Whole:
    """One whole-vector unit on device copies of a case's inputs, with a
    workspace of its own from which summary and partials are read."""

    def __init__(self, kind, v0, v1, cg, n, one):
        from bayesdll_amd import _lib as L
        self.L, self.h, self.kind, self.n, self.cg = L, L.lib(), kind, n, cg
        self.d = [torch.from_numpy(np.array(v)).cuda() for v in (v0, v1)]
        self.one = [torch.from_numpy(np.array(o)).cuda() for o in one]
        self.struct = L.EssSummary if kind == "ess" else L.DiagSummary
        self.wsb = int(getattr(self.h, f"bdl_chain_{kind}_workspace_bytes")(n))
        assert self.wsb == 128 + S.MAX_GRID * C.sizeof(self.struct)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")

    def plant(self, i, j):
        """Elements i and j of both chains become the planted element; returns the undo."""
        slot = 4 * self.cg
        at = torch.tensor([slot * k + e for k in range(K_) for e in (i, j)], device="cuda")
        src = torch.tensor([4 * k for k in range(K_) for _ in (i, j)], device="cuda")
        saved = [d[at].clone() for d in self.d]
        for d, o in zip(self.d, self.one):
            d[at] = o[src]
        return at, saved

    def undo(self, token):
        at, saved = token
        for d, s in zip(self.d, saved):
            d[at] = s

    def run(self, geometry, thresholds, nparts=0):
        """(summary, partials[nparts]) as structured arrays."""
        L = self.L
        self.ws.fill_(0xA5)
        if self.kind == "ess":
            a = L.EssArgs()
            a.sM2, a.bM2 = self.d[0].data_ptr(), self.d[1].data_ptr()
            a.samples, a.batches, a.grid_blocks = SAMPLES, BATCHES, geometry
        else:
            a = L.DiagArgs()
            a.mom1, a.mom2 = self.d[0].data_ptr(), self.d[1].data_ptr()
            a.var_mode, a.ratio, a.inv_ratio = DIAG_KW["var_mode"], 1.0, 0.0
            a.var_floor, a.c1, a.blocks_per_cu = 0.0, (COUNT - 1) / COUNT, geometry
        a.workspace = self.ws.data_ptr()
        a.n, a.chain_groups, a.chains = self.n, self.cg, K_
        for k, t in enumerate(thresholds):
            a.thresholds[k] = t
        fn = getattr(self.h, f"bdl_chain_{self.kind}")
        L.check(fn(a, L.current_stream_handle(self.d[0].device)), fn.__name__)
        torch.cuda.synchronize()
        size = C.sizeof(self.struct)
        raw = self.ws[:128 + nparts * size].cpu().numpy()
        dt = np.dtype(self.struct)
        summ = np.frombuffer(raw[:size].tobytes(), dtype=dt)[0]
        assert (raw[size:128] == 0xA5).all()                   # the padding before the partials
        return summ, np.frombuffer(raw[128:].tobytes(), dtype=dt)


def assert_equal(spec, got, want, what):
    """A device struct (or an array of them) against reduce's fields, exactly."""
    for f in INT_FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])
    assert np.array_equal(got[spec["hits"]], want["hits"]), (what, got[spec["hits"]], want["hits"])
    assert np.array_equal(got[spec["arg"]], want["arg"]), (what, got[spec["arg"]], want["arg"])
    assert np.array_equal(np.asarray(got[spec["ext"]]).view(np.int32),
                          np.asarray(want["ext"], dtype=F).view(np.int32)), (what, "ext")
    assert np.array_equal(S.sum_bits(got[spec["total"]]), S.sum_bits(want["sum"])), \
        (what, "sum", got[spec["total"]], want["sum"])


def whole_sweep(kind, spec, case, n, geometries, grid_of, expect_grid=None):
    """Everything this file asserts of one whole-vector unit at one size."""
    v0, v1, cg, vals, (one, pv) = case
    dev = Whole(kind, v0, v1, cg, n, one)
    maximum = kind == "diag"
    finite = vals[0][~vals[1] & ~vals[2]]
    thr = (float(pv), float(np.median(finite)), float(finite.max() if maximum else finite.min()))
    seen = {}
    # the pair of the first geometry's deepest level, planted at every geometry
    name, i, j = S.ties_whole(n, grid_of(n, geometries[0], cus()))[-1]
    for geo in geometries:
        grid = grid_of(n, geo, cus())
        if expect_grid is not None and geo == geometries[0]:
            assert grid == expect_grid, (grid, expect_grid)
        own = S.owner(n, grid)
        ties = S.ties_whole(n, grid)
        # that pair planted: every field of the summary and of every partial
        token = dev.plant(i, j)
        v, deg, nonf = planted(vals, pv, (i, j))
        want = S.reduce(v, own, maximum=maximum, thresholds=thr, degenerate=deg, nonfinite=nonf)
        assert want.summary["arg"] == i and want.summary["ext"] == pv and len(want.trace) == 1
        # a value on a threshold is not beyond it: nothing is beyond the planted extreme, and
        # beyond the unplanted extreme lie the two planted elements only, not that extreme itself
        assert want.summary["hits"][0] == 0 and 0 < want.summary["hits"][1] < want.summary["n_eval"]
        assert want.summary["hits"][2] == 2
        summ, parts = dev.run(geo, thr, grid)
        assert parts.shape == (grid,)
        assert_equal(spec, summ, want.summary, (n, geo, name))
        assert_equal(spec, parts, want.partials, (n, geo, name, "partials"))
        again = dev.run(geo, thr, grid)                        # a repeat: the same bits
        assert again[0].tobytes() == summ.tobytes() and again[1].tobytes() == parts.tobytes()
        seen[geo] = tuple(int(summ[f]) for f in INT_FIELDS) + (
            summ[spec["hits"]].tolist(), float(summ[spec["ext"]]), int(summ[spec["arg"]]))
        dev.undo(token)
        # every planted pair alone: the lower index
        for nm, a, b in ties:
            token = dev.plant(a, b)
            summ, _ = dev.run(geo, thr)
            assert (int(summ[spec["arg"]]), float(summ[spec["ext"]])) == (a, float(pv)), \
                (n, geo, nm, a, b, int(summ[spec["arg"]]))
            assert summ[spec["hits"]][0] == 0
            if n < 4096:
                v, deg, nonf = planted(vals, pv, (a, b))
                want = S.reduce(v, own, maximum=maximum, thresholds=thr, degenerate=deg,
                                nonfinite=nonf)
                assert_equal(spec, summ, want.summary, (n, geo, nm))
            dev.undo(token)
        for d, v in zip(dev.d, (v0, v1)):                      # every plant was undone
            assert np.array_equal(d.cpu().numpy().view(np.int32), np.asarray(v).view(np.int32))
    return seen


# --------------------------------------------------------------------- ESS
@pytest.mark.parametrize("n,grid_blocks,grid", ESS_CASES)
def test_ess_summary_partials_and_planted_ties(n, grid_blocks, grid):
    """(1025, 0): one trip, a one-element guarded iteration.  (3077, 3): a
    second trip in workgroup 0 only.  (N_MID, 257): two whole trips, a finalize
    thread with two partials.  (N_BIG, 2048): the largest input (4.2 M
    elements, 67 MB), eight partials per finalize thread.  Each also at another
    grid: the same counts, extreme and arg."""
    other = 1 if grid_blocks == 0 else 0
    assert S.grid_ess(n, other, cus()) != grid
    seen = whole_sweep("ess", ESS, ess_case(n), n, [grid_blocks, other], S.grid_ess, grid)
    assert seen[grid_blocks] == seen[other]


def test_ess_finalize_thread_whose_first_partial_is_empty():
    """Workgroup 0 of 257 evaluates nothing (every element it owns is
    degenerate): finalize thread 0 combines empty() with an empty partial and
    then with workgroup 256's."""
    n, grid = N_MID, 257
    sM2, bM2, cg, _, (one, _) = ess_case(n)
    own = S.owner(n, grid)
    mine = np.flatnonzero(own["wg"] == 0)
    bM2 = np.array(bM2)
    for k in range(K_):
        bM2[4 * cg * k + mine] = 0.0
    vals = ess_values(np.asarray(sM2), bM2, n, 4 * cg)
    want = S.reduce(*vals[:1], own, maximum=False, thresholds=ER.THRESHOLDS, degenerate=vals[1],
                    nonfinite=vals[2])
    assert "fin_empty_then_value" in want.marks and want.partials["n_eval"][0] == 0
    summ, parts = Whole("ess", sM2, bM2, cg, n, one).run(grid, ER.THRESHOLDS, grid)
    assert_equal(ESS, summ, want.summary, "summary")
    assert_equal(ESS, parts, want.partials, "partials")
    assert (int(parts[0]["argmin"]), float(parts[0]["ess_min"])) == (2 ** 63 - 1, float("inf"))


# ------------------------------------------------------------------- R-hat
def test_diag_summary_partials_and_planted_ties_beyond_256_partials():
    n = N_MID
    grids = {bpc: S.grid_diag(n, bpc, cus()) for bpc in (1, 2, 8)}
    assert max(grids.values()) > 256, \
        f"{cus()} CUs give {grids}: no geometry of bdl_chain_diag reaches more than 256 partials"
    seen = whole_sweep("diag", DIAG, diag_case(n), n, [1, 2, 8], S.grid_diag)
    assert seen[1] == seen[2] == seen[8]


# ------------------------------------------------------------------ layers
def table(name):
    return {"l": LR.table_l, "a": LR.table_a, "big": S.big_table}[name]()


@functools.lru_cache(maxsize=None)
def layers_case(name, kind):
    tab = table(name)
    if kind == "diag":
        v0, v1 = LR.diag_inputs(tab, K_, DR.VAR_GIVEN, 1.0)
        rng = np.random.default_rng(3)
        wide = np.flatnonzero(rng.random(tab.n) < 0.33)
        v0[tab.slot + wide] = v0[wide] + (0.05 * 2.0 ** rng.integers(0, 21, wide.size)).astype(F)
        o, m = tab.span(tab.frozen)
        v0[tab.slot + o: tab.slot + o + m] = v0[o: o + m]
        vals = diag_values(v0, v1, tab.n, tab.slot, DIAG_KW)
        one, pv = diag_planted()
        ok = vals[0][~vals[1] & ~vals[2]].max() < pv
    else:
        v0, v1 = LR.ess_inputs(tab, K_)
        rng = np.random.default_rng(4)
        scale = (2.0 ** rng.integers(-20, 21, tab.n)).astype(F)
        for k in range(K_):
            v0[tab.slot * k: tab.slot * k + tab.n] *= scale
        vals = ess_values(v0, v1, tab.n, tab.slot)
        one, pv = ess_planted()
        ok = vals[0][~vals[1] & ~vals[2]].min() > pv
    assert ok
    return tab, v0, v1, vals, one, pv


def layers_scalars(kind):
    return DIAG_KW if kind == "diag" else dict(samples=SAMPLES, batches=BATCHES)


@pytest.mark.parametrize("grid", [3, 512, 1024])
@pytest.mark.parametrize("kind", ["diag", "ess"])
@pytest.mark.parametrize("name", ["l", "a", "big"])
def test_layers_rows_and_partials_equal_the_restatement(name, kind, grid):
    """Every row of the table and every [segment][workgroup] partial, exactly;
    then (R-hat at 3 and 1024 workgroups, ESS at 512) every planted pair of the
    table in a launch of its own: head against body, tail against body, head
    against tail, one lane's group, two workgroups of a rotated segment."""
    spec = DIAG if kind == "diag" else ESS
    tab, v0, v1, vals, one, pv = layers_case(name, kind)
    maximum = kind == "diag"
    thr = DR.THRESHOLDS if maximum else ER.THRESHOLDS
    owns = S.owner_layers(tab.segments, grid)

    def rows(v, deg, nonf):
        return [S.reduce(v[o:o + m], own, maximum=maximum, thresholds=thr, degenerate=deg[o:o + m],
                         nonfinite=nonf[o:o + m]) for (o, m), own in zip(tab.segments, owns)]

    want = rows(*vals)
    got, parts = launch(spec, tab, v0, v1, K_, grid, partials=True, **layers_scalars(kind))
    assert parts.shape == (len(tab.segments), grid)
    for s, w in enumerate(want):
        assert_equal(spec, got[s], w.summary, (name, grid, s))
        assert_equal(spec, parts[s], w.partials, (name, grid, s, "partials"))
    if grid >= 512:
        assert any("idle_workgroup" in w.marks for w in want)
    if (kind == "diag") == (grid == 512):
        return
    for nm, s, i, j in S.ties_layers(tab.segments, grid, owns):
        a0, a1 = np.array(v0), np.array(v1)
        for k in range(K_):
            for e in (i, j):
                a0[tab.slot * k + e], a1[tab.slot * k + e] = one[0][4 * k], one[1][4 * k]
        row = launch(spec, tab, a0, a1, K_, grid, **layers_scalars(kind))[s]
        assert (int(row[spec["arg"]]), float(row[spec["ext"]])) == (i, float(pv)), (nm, s, i, j)
        if name != "big":
            o, m = tab.segments[s]
            v, deg, nonf = planted(vals, pv, (i, j))
            w = S.reduce(v[o:o + m], owns[s], maximum=maximum, thresholds=thr,
                         degenerate=deg[o:o + m], nonfinite=nonf[o:o + m])
            assert_equal(spec, row, w.summary, (nm, s))
