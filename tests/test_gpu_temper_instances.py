"""Every instance and launch path of the temperature-scaling sweeps on the GPU
(bdl_temper.hip), on table T of tests/temper_geometry_ref.py — what T reaches
is proven on the CPU by tests/test_temper_geometry_host.py, which also holds
the input conditions (margins > 1 for every case and beta used here) that make
the exact comparisons legitimate.  The three entry points are called through
_lib on guarded buffers: NaN words around logp, 0xA5 bytes around labels,
state, totals and workspace, all asserted unchanged after every call.  Every
tolerance is a derived bound of tests/temper_ref.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import temper_geometry_ref as Gm
import temper_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
NAN_WORD = np.array([0x7FC00000], dtype=np.uint32).view(np.uint8)
A5_WORD = np.full(4, 0xA5, dtype=np.uint8)
INTS = ("n", "n_labelled", "n_nonfinite", "n_wrong")
SUMS = ("nll_sum", "entropy_sum", "confidence_sum")
FLAGS = ("converged", "at_bound", "degenerate", "done")


class Guarded:
    """A device buffer of nbytes between two guards of GUARD bytes (a repeated
    4-byte word); the body starts 16-B aligned and is filled with `fill`
    (bytes) or left poisoned with 0xA5."""

    def __init__(self, nbytes, fill=None, word=A5_WORD):
        self.n = int(nbytes)
        pad = -self.n % 4
        host = np.full(self.n + pad + 2 * GUARD, 0xA5, dtype=np.uint8)
        host[:GUARD] = np.tile(word, GUARD // 4)
        host[GUARD + self.n:] = np.tile(word, (GUARD + pad) // 4 + 1)[:GUARD + pad]
        if fill is not None:
            host[GUARD:GUARD + self.n] = np.frombuffer(fill, dtype=np.uint8)
        self.host = host.copy()
        self.raw = torch.from_numpy(host).cuda()
        assert (self.raw.data_ptr() + GUARD) % 16 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def body(self):
        return self.raw[GUARD:GUARD + self.n].cpu().numpy()

    def write(self, data):
        self.raw[GUARD:GUARD + self.n] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()

    def intact(self):
        lo, hi = self.raw[:GUARD].cpu().numpy(), self.raw[GUARD + self.n:].cpu().numpy()
        return np.array_equal(lo, self.host[:GUARD]) and np.array_equal(hi, self.host[GUARD + self.n:])


class Run:
    """One group table on the device and the three entry points on it."""

    def __init__(self, z, lab):
        from bayesdll_amd import _lib as L
        self.L, self.h = L, L.lib()
        self.z = np.ascontiguousarray(z, dtype=np.float32)
        self.lab = None if lab is None else np.ascontiguousarray(lab, dtype=np.int64)
        self.G, self.N, self.C = self.z.shape
        self.logp = Guarded(self.z.nbytes, self.z.tobytes(), NAN_WORD)
        self.labels = None if lab is None else Guarded(self.lab.nbytes, self.lab.tobytes())
        self.state = Guarded(self.G * C.sizeof(L.TemperState))
        self.totals = Guarded(self.G * C.sizeof(L.TemperTotals))
        self.bufs = [self.logp, self.state, self.totals] + ([self.labels] if self.labels else [])
        self.stream = L.current_stream_handle(self.raw_device())

    def raw_device(self):
        return self.logp.raw.device

    def _workspace(self, grid):
        return Guarded(self.h.bdl_temper_workspace_bytes(self.G, grid))

    def _settle(self, ws):
        torch.cuda.synchronize()
        for b in self.bufs + [ws]:
            assert b.intact()
        assert self.logp.body().tobytes() == self.z.tobytes()       # the inputs are bit-unchanged
        if self.labels:
            assert self.labels.body().tobytes() == self.lab.tobytes()

    def set_state(self, betas):
        host = np.zeros(self.G, dtype=np.dtype(self.L.TemperState))
        host["beta"] = np.asarray(betas, dtype=np.float32)
        self.state.write(host.tobytes())

    def read_state(self):
        return np.frombuffer(self.state.body().tobytes(), dtype=np.dtype(self.L.TemperState))

    def pairs(self, count, grid, rtol=1e-6, max_iter=32):
        """`count` (sweep, update) pairs enqueued back to back, as kernels.temper_fit does."""
        ws = self._workspace(grid)
        a = self.L.TemperFitArgs()
        a.logp, a.labels = self.logp.ptr, (self.labels.ptr if self.labels else None)
        a.state, a.workspace = self.state.ptr, ws.ptr
        a.batch, a.rtol, a.groups, a.classes = self.N, rtol, self.G, self.C
        a.grid_blocks, a.max_iter = grid, max_iter
        for _ in range(count):
            self.L.check(self.h.bdl_temper_fit_sweep(a, self.stream), "bdl_temper_fit_sweep")
            self.L.check(self.h.bdl_temper_fit_update(a, self.stream), "bdl_temper_fit_update")
        self._settle(ws)
        return self.read_state()

    def report(self, grid, nb=15, reset=True):
        ws = self._workspace(grid)
        a = self.L.TemperReportArgs()
        a.logp, a.labels = self.logp.ptr, (self.labels.ptr if self.labels else None)
        a.state, a.totals, a.workspace = self.state.ptr, self.totals.ptr, ws.ptr
        a.batch, a.groups, a.classes, a.num_bins, a.grid_blocks = self.N, self.G, self.C, nb, grid
        a.flags = self.L.TEMPER_RESET if reset else 0
        for i, e in enumerate(R.edges32(nb)):
            a.edges[i] = float(e)
        self.L.check(self.h.bdl_temper_report(a, self.stream), "bdl_temper_report")
        self._settle(ws)
        return np.frombuffer(self.totals.body().tobytes(), dtype=np.dtype(self.L.TemperTotals))


def update_rule(beta, d1, d2, n, rtol, iterations, max_iter):
    """bdl_temper_fit_update's steps 3-5 in the same fp64 operations, from the
    stored means: (beta, iterations, converged, at_bound, degenerate, done)."""
    degenerate = n == 0 or not d2 > 0.0 or not math.isfinite(d1)
    if degenerate or iterations >= max_iter:
        return beta, iterations, 0, 0, int(degenerate), 0
    nb = beta - d1 / d2
    nb = min(max(nb, 0.25 * beta), 4.0 * beta)
    at_bound = 0
    if nb <= R.BETA_MIN:
        nb, at_bound = R.BETA_MIN, 1
    if nb >= R.BETA_MAX:
        nb, at_bound = R.BETA_MAX, 1
    nb32 = float(np.float32(nb))
    if not at_bound and abs(nb32 - beta) <= rtol * beta:
        return beta, iterations, 1, 0, 0, 1
    if at_bound and nb32 == beta:
        return beta, iterations, 0, 1, 0, 1
    if nb32 != beta:
        return nb32, iterations + 1, 0, at_bound, 0, 0
    return beta, iterations, 0, at_bound, 0, 0


def check_sweep(row, z, lab, beta, what):
    """One group's stored sweep against the fp64 reference at `beta`."""
    s = R.sweep_reference(z, lab, beta)
    got = (int(row["n"]), int(row["n_nonfinite"]), int(row["n_inf_label"]))
    assert got == (s["n"], s["n_nonfinite"], s["n_inf_label"]), (what, got, s)
    for k, b in (("nll", "b_nll"), ("d1", "b_d1"), ("d2", "b_d2")):
        err = abs(float(row[k]) - s[k])
        print(what, k, err, s[b])
        assert err <= s[b], (what, k, err, s[b])
    return s


def check_report(rows, z, lab, betas, nb, what, scale=1):
    for g, row in enumerate(rows):
        r = R.report_reference(z[g], lab, betas[g], nb)
        for k in INTS:
            assert int(row[k]) == scale * r[k], (what, g, k, int(row[k]), r[k])
        assert np.array_equal(row["bin_count"], scale * r["bin_count"]), (what, g)
        assert np.array_equal(row["bin_hits"], scale * r["bin_hits"]), (what, g)
        for k in SUMS:
            if np.isinf(r[k]):      # a -inf at a label: its nll is +inf on both sides
                assert float(row[k]) == r[k], (what, g, k)
                continue
            err = abs(float(row[k]) - scale * r[k])
            print(what, g, k, err, scale * r["b_" + k])
            assert err <= scale * r["b_" + k], (what, g, k, err, r["b_" + k])
        assert (np.abs(row["bin_conf"] - scale * r["bin_conf"]) <= scale * r["b_bin_conf"]).all(), (what, g)


def ints_of(rows):
    return [[int(r[k]) for k in INTS] + r["bin_count"].tolist() + r["bin_hits"].tolist() for r in rows]


def other_grid(grid):
    return 7 if grid > 3 else grid + 1


# --------------------------------------------- one (sweep, update) pair at beta != 1
@pytest.mark.parametrize("case", Gm.T, ids=Gm.case_id)
def test_one_sweep_and_update_from_per_group_betas(case):
    """nll / f' / f'' at 0.37, 2.5 and 1 (a beta dropped from m, t or t[y], or
    taken from another group, moves them), the counts exact, and the update's
    step reproduced exactly from the stored means."""
    z, lab = Gm.rows(case)
    betas = Gm.betas_of(case)
    run = Run(z, lab)
    run.set_state(betas)
    rows = run.pairs(1, case[3])
    for g, row in enumerate(rows):
        check_sweep(row, z[g], lab, betas[g], (Gm.case_id(case), g))
        assert row["sweeps"] == 1 and row["nll_first"] == row["nll"]
        want = update_rule(betas[g], float(row["d1"]), float(row["d2"]), int(row["n"]), 1e-6, 0, 32)
        got = (float(row["beta"]), int(row["iterations"])) + tuple(int(row[k]) for k in FLAGS)
        assert got == want, (g, got, want)


# ---------------------------------------------------------------- the whole fit
@pytest.mark.parametrize("case", Gm.T, ids=Gm.case_id)
def test_whole_fit_against_the_emulation_and_the_fp64_fit(case):
    z, lab = Gm.rows(case)
    run = Run(z, lab)
    run.set_state(np.ones(case[2]))
    rows = run.pairs(32, case[3])
    for g, row in enumerate(rows):
        em, fr = R.newton(z[g], lab), R.fit_reference(z[g], lab)
        got = tuple(bool(row[k]) for k in FLAGS) + (int(row["iterations"]), int(row["sweeps"]))
        want = tuple(em[k] for k in FLAGS) + (em["iterations"], em["sweeps"])
        print(Gm.case_id(case), g, 1.0 / row["beta"], fr["temperature"], got, em["margin"])
        assert got == want, (g, got, want)
        fit = {"beta": float(row["beta"])}
        assert abs(1.0 / fit["beta"] - fr["temperature"]) <= R.bound_T(z[g], lab, fit, 1e-6)
        s = check_sweep(row, z[g], lab, fit["beta"], (Gm.case_id(case), g, "final"))
        assert row["nll"] <= row["nll_first"] and s["n"] == em["n"]


# ------------------------------------------------ the report at per-group temperatures
@pytest.mark.parametrize("case", Gm.T, ids=Gm.case_id)
def test_report_at_per_group_betas_accumulates_resets_and_ignores_the_grid(case):
    z, lab = Gm.rows(case)
    betas = Gm.betas_of(case)
    what = Gm.case_id(case)
    run = Run(z, lab)
    run.set_state(betas)
    first = run.report(case[3], reset=True).copy()          # RESET over the poisoned totals
    check_report(first, z, lab, betas, 15, what)
    twice = run.report(case[3], reset=False).copy()         # accumulating: everything doubles
    check_report(twice, z, lab, betas, 15, (what, "twice"), scale=2)
    for g in range(case[2]):
        assert ints_of(twice[g:g + 1])[0] == [2 * v for v in ints_of(first[g:g + 1])[0]]
        for k in SUMS:
            assert twice[g][k] == 2 * first[g][k]
        assert np.array_equal(twice[g]["bin_conf"], 2 * first[g]["bin_conf"])
    again = run.report(case[3], reset=True).copy()          # RESET over what has accumulated
    assert again.tobytes() == first.tobytes()               # a fixed geometry is bit-identical
    assert np.array_equal(run.read_state()["beta"], np.asarray(betas, np.float32))
    for grid in (other_grid(case[3]), 0):
        rows = run.report(grid, reset=True)
        check_report(rows, z, lab, betas, 15, (what, grid))
        assert ints_of(rows) == ints_of(first), (what, grid)


# ------------------------------------------------------------- the fit's decisions
def test_fit_walks_to_the_upper_limit_of_beta_and_stops_there():
    z, lab = Gm.upper_limit_rows()
    em = R.newton(z, lab)
    run = Run(z[None], lab)
    run.set_state([1.0])
    for count, beta in ((1, 4.0), (1, 16.0), (1, 64.0)):
        row = run.pairs(count, 2)[0]
        assert float(row["beta"]) == beta and not row["done"] and not row["at_bound"]
    row = run.pairs(29, 2)[0]
    assert float(row["beta"]) == R.BETA_MAX == 100.0
    got = tuple(bool(row[k]) for k in FLAGS) + (int(row["iterations"]), int(row["sweeps"]))
    assert got == (False, True, False, True, 4, 5) == tuple(em[k] for k in FLAGS) + (
        em["iterations"], em["sweeps"])
    check_sweep(row, z, lab, 100.0, "upper limit")


def test_max_iter_exhausted_leaves_the_group_not_done():
    """max_iter = 2 and three pairs: beta moves twice (each move reproduced
    exactly from the stored means), the third sweep evaluates the group at the
    beta it then has and the update leaves it — sweeps counts the pairs, nll
    is that of the current beta.  Then the same three pairs enqueued back to
    back give the same state bit for bit."""
    case = Gm.MAX_ITER_CASE
    z, lab = Gm.rows(case)
    run = Run(z, lab)
    run.set_state(np.ones(case[2]))
    prev = [(1.0, 0)] * case[2]
    for pair in range(3):
        rows = run.pairs(1, case[3], max_iter=2)
        for g, row in enumerate(rows):
            check_sweep(row, z[g], lab, prev[g][0], (g, pair))
            want = update_rule(prev[g][0], float(row["d1"]), float(row["d2"]), int(row["n"]), 1e-6,
                               prev[g][1], 2)
            got = (float(row["beta"]), int(row["iterations"])) + tuple(int(row[k]) for k in FLAGS)
            assert got == want and int(row["sweeps"]) == pair + 1, (g, pair, got, want)
            prev[g] = want[:2]
    for g, row in enumerate(rows):
        em = R.newton(z[g], lab, max_iter=2)
        assert int(row["iterations"]) == 2 == em["iterations"] and int(row["sweeps"]) == 3
        assert tuple(bool(row[k]) for k in FLAGS) == (False, False, False, False)
        check_sweep(row, z[g], lab, float(row["beta"]), (g, "current beta"))
    run.set_state(np.ones(case[2]))
    assert run.pairs(3, case[3], max_iter=2).tobytes() == rows.tobytes()


def test_rtol_zero_ends_as_the_emulation_does():
    case = Gm.MAX_ITER_CASE
    z, lab = Gm.rows(case)
    run = Run(z, lab)
    run.set_state(np.ones(case[2]))
    rows = run.pairs(32, case[3], rtol=0.0)
    for g, row in enumerate(rows):
        em, fr = R.newton(z[g], lab, rtol=0.0), R.fit_reference(z[g], lab)
        got = tuple(bool(row[k]) for k in FLAGS) + (int(row["iterations"]), int(row["sweeps"]))
        want = tuple(em[k] for k in FLAGS) + (em["iterations"], em["sweeps"])
        print(g, got, want, float(row["beta"]), em["beta"])
        assert got == want, (g, got, want)
        fit = {"beta": float(row["beta"])}     # a step of zero is within any rtol
        assert abs(1.0 / fit["beta"] - fr["temperature"]) <= R.bound_T(z[g], lab, fit, 1e-6)


@pytest.mark.parametrize("case", Gm.BIN_CASES, ids=Gm.case_id)
def test_without_labels_the_fit_is_degenerate_and_the_report_has_no_bins(case):
    z, _ = Gm.rows(case)
    betas = Gm.betas_of(case)
    run = Run(z, None)
    run.set_state(np.ones(case[2]))
    for row in run.pairs(2, case[3]):
        assert row["degenerate"] and not row["done"] and not row["converged"]
        assert int(row["n"]) == 0 and np.isnan(row["nll"]) and float(row["beta"]) == 1.0
        assert int(row["iterations"]) == 0 and int(row["sweeps"]) == 2
        assert int(row["n_nonfinite"]) == R.sweep_reference(z[0], None, 1.0)["n_nonfinite"]
    run.set_state(betas)
    rows = run.report(case[3])
    check_report(rows, z, None, betas, 15, "no labels")
    for row in rows:
        assert int(row["n_labelled"]) == 0 and int(row["n_wrong"]) == 0 and row["nll_sum"] == 0
        assert not row["bin_count"].any() and not row["bin_hits"].any() and not row["bin_conf"].any()
        assert int(row["n"]) > 0 and row["entropy_sum"] > 0


# ------------------------------------------------------------------ other bin counts
@pytest.mark.parametrize("nb", Gm.BIN_COUNTS)
@pytest.mark.parametrize("case", Gm.BIN_CASES, ids=Gm.case_id)
def test_report_with_other_bin_counts(case, nb):
    z, lab = Gm.rows(case)
    run = Run(z, lab)
    run.set_state(Gm.BIN_BETAS)
    rows = run.report(case[3], nb=nb)
    check_report(rows, z, lab, Gm.BIN_BETAS, nb, (Gm.case_id(case), nb))
    for row in rows:
        assert not row["bin_count"][nb:].any() and not row["bin_conf"][nb:].any()
    if nb == 64:
        assert sum(int(r["bin_count"][63]) for r in rows) > 0     # lane 63's bin
    assert ints_of(run.report(0, nb=nb)) == ints_of(rows)
