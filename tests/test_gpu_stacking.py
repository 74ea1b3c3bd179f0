"""bdl_stack_gather / bdl_stack_fit on the device against tests/stacking_ref.py,
with guarded buffers (sentinels around ell, valid, the counters, the state and
the workspace).

Bounds (include/bdl_stacking.h, derived in stacking_ref from u = 2^-24, the
1-ulp expf and the fp64 sums; T the device's `iterations`, the reference forced
to the same T):
    |w_k - w_k^ref| <= bw = (T + 1) (6u + (n + P) 2^-52)
    |objective - objective^ref| <= 3u + bw + (n + P) 2^-52 max(1, |objective|)
    |gap - gap^ref| <= bg = (1 + gap) (6u + (n + P) 2^-52 + bw)
`iterations` lies between the free-running reference's first pass with
gap <= tol + bg and its first with gap <= tol - bg (max_iter where it has none):
the slack for a gap that crosses tol within rounding.  The gather, the counters
and every integer are exact; the state is bit-identical across grid_blocks and
runs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import stacking_ref as R
from test_gpu_rank import Guarded
from test_stacking_host import check_refusals

pytestmark = pytest.mark.gpu
TOL = 1e-4
# every P of {1, 2, 3, 8, 64} and every N of {1, 37, 1024, 1025, 2600}
CASES = [(1, 37, "graded"), (2, 1, "graded"), (2, 1025, "graded"), (3, 37, "disjoint"),
         (3, 2600, "graded"), (8, 1024, "disjoint"), (8, 1025, "equal"), (64, 37, "graded"),
         (64, 2600, "graded"), (1, 1024, "equal"), (64, 1, "equal")]
ids = lambda c: f"{c[0]}x{c[1]}-{c[2]}"  # noqa: E731


@functools.lru_cache(maxsize=None)
def built(case):
    """(logp, labels, ell, valid, counts, free-running reference fit), once per case."""
    P, N, kind = case
    logp, y = R.make_case(P, N, kind=kind, seed=7 * P + N)
    ell, valid, counts = R.gather(logp, y)
    return logp, y, ell, valid, counts, R.fit(ell, valid, N, tol=TOL)


def _gather(case, dev, batches, cap_extra=3):
    """The case's logp through bdl_stack_gather in `batches` pieces."""
    from bayesdll_amd import _lib as L
    logp, y, *_ = built(case)
    P, N, Cn = logp.shape
    cap = N + cap_extra
    h = L.lib()
    g = {"ell": Guarded(P * cap * 4, dev), "valid": Guarded(cap * 4, dev),
         "counters": Guarded(24, dev), "workspace": Guarded(h.bdl_stack_workspace_bytes(P, cap), dev)}
    cuts = np.linspace(0, N, batches + 1).astype(int)
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        if hi == lo:
            continue
        xd = torch.from_numpy(np.ascontiguousarray(logp[:, lo:hi])).to(dev)
        yd = torch.from_numpy(np.ascontiguousarray(y[lo:hi])).to(dev)
        a = L.StackGatherArgs()
        a.logp, a.labels = xd.data_ptr(), yd.data_ptr()
        a.ell, a.valid, a.counters = g["ell"].ptr, g["valid"].ptr, g["counters"].ptr
        a.workspace = g["workspace"].ptr
        a.batch, a.off, a.cap, a.voters, a.classes = hi - lo, lo, cap, P, Cn
        a.grid_blocks, a.flags = (0, 1, 3)[i % 3], (L.STACK_RESET if lo == 0 else 0)
        L.check(h.bdl_stack_gather(a, L.current_stream_handle(dev)), "bdl_stack_gather")
        torch.cuda.synchronize(dev)
    return g, cap


def _fit(g, case, cap, dev, grid=0, max_iter=2000, chunk=2000, tol=TOL):
    """bdl_stack_fit on gathered buffers with a guarded state -> (record, guards)."""
    from bayesdll_amd import _lib as L
    P, N, _ = case
    h = L.lib()
    st = Guarded(C.sizeof(L.StackState), dev)
    ws = Guarded(h.bdl_stack_workspace_bytes(P, N), dev)
    a = L.StackFitArgs()
    a.ell, a.valid, a.state, a.workspace = g["ell"].ptr, g["valid"].ptr, st.ptr, ws.ptr
    a.n_cols, a.cap, a.tol, a.voters, a.grid_blocks = N, cap, tol, P, grid
    done = 0
    while done < max_iter:
        a.iterations = min(chunk, max_iter - done)
        done += a.iterations
        a.flags = (L.STACK_FIRST if done == a.iterations else 0) | \
            (L.STACK_FINAL if done == max_iter else 0)
        L.check(h.bdl_stack_fit(a, L.current_stream_handle(dev)), "bdl_stack_fit")
    torch.cuda.synchronize(dev)
    assert st.intact() and ws.intact(), case
    return np.frombuffer(st.body().tobytes(), dtype=np.dtype(L.StackState))[0]


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gather_and_fit_against_the_reference(case):
    dev = torch.device("cuda:0")
    P, N, kind = case
    logp, y, ell, valid, counts, free = built(case)
    g, cap = _gather(case, dev, batches=3)
    # the gather, its counters and what it leaves alone: exact
    got_ell = np.frombuffer(g["ell"].body().tobytes(), dtype=np.float32).reshape(P, cap)
    got_valid = np.frombuffer(g["valid"].body().tobytes(), dtype=np.int32)
    assert np.array_equal(got_ell[:, :N].view(np.uint32), ell.view(np.uint32))
    assert np.array_equal(got_valid[:N], valid)
    assert (g["ell"].body().reshape(P, cap * 4)[:, N * 4:] == 0xA5).all()   # columns >= N untouched
    assert (g["valid"].body()[N * 4:] == 0xA5).all()
    cnt = np.frombuffer(g["counters"].body().tobytes(), dtype=np.int64)
    assert dict(zip(("n_label", "n_nonfinite", "n_impossible"), cnt.tolist())) == counts
    assert all(v.intact() for v in g.values())
    if N >= 37:
        assert counts == {"n_label": 2, "n_nonfinite": 2, "n_impossible": 1}

    # the state: bit-identical across grids and runs, and with the launches past convergence
    r = _fit(g, case, cap, dev, grid=0)
    for grid in (1, 3, 1024, 3):
        assert _fit(g, case, cap, dev, grid=grid).tobytes() == r.tobytes(), (case, grid)
    assert _fit(g, case, cap, dev, chunk=1, max_iter=int(r["iterations"]) + 1).tobytes() \
        == r.tobytes()                       # enqueued no further than the converged pass
    n, T = int(r["n"]), int(r["iterations"])
    assert n == free["n"] == int(valid.sum()) and r["converged"] == 1 and r["degenerate"] == 0
    assert not r["w"][P:].any() and r["pad"] == 0
    w = r["w"][:P]
    # (a dominated voter's weight decays geometrically and may underflow to 0: w >= 0)
    assert abs(w.sum() - 1) < 1e-14 and (w >= 0).all() and r["gap"] <= TOL

    # iterations: the reference's count within the derived slack
    lo, hi = R.iteration_range(free["gaps"], TOL, n, P)
    hi = 2000 if hi is None else hi
    print(f"{ids(case)}: iterations {T} (reference {free['iterations']}, allowed [{lo}, {hi}])")
    assert lo is not None and lo <= T <= hi
    if P == 1:
        assert T == 0 and w.tolist() == [1.0] and r["gap"] == 0

    # w, objective, gap against the literal reference at the same count
    ref = R.fit(ell, valid, N, tol=TOL, updates=T)
    bw, bo = R.bound_w(T, n, P), R.bound_objective(T, n, P, ref["gap"], ref["objective"])
    bg = R.bound_gap(T, n, P, ref["gap"])
    ew, eo = np.abs(w - ref["w"]).max(), abs(r["objective"] - ref["objective"])
    eg = abs(r["gap"] - ref["gap"])
    print(f"{ids(case)}: w error {ew:.3g} ({ew / bw:.2%} of the bound), objective {eo:.3g} "
          f"({eo / bo:.2%}), gap {eg:.3g} ({eg / bg:.2%})")
    assert ew <= bw and eo <= bo and eg <= bg
    assert abs(r["objective_uniform"] - ref["objective_uniform"]) <= R.bound_objective(
        0, n, P, ref["gaps"][0], ref["objective_uniform"])
    # the certificate against the independent solver
    _, f_indep, _ = R.solve(ell, valid)
    assert r["objective"] >= f_indep - TOL - bo
    if P >= 3:  # the two identical voters hold identical weights
        assert w[P - 1] == w[P - 2]
    if P >= 2 and N >= 37:  # the sole coverer of example 13
        assert w[0] >= 1 / n


@pytest.mark.parametrize("case", [(3, 2600, "graded"), (8, 1024, "disjoint"), (64, 2600, "graded")],
                         ids=ids)
def test_max_iter_5_reports_a_consistent_unconverged_state(case):
    dev = torch.device("cuda:0")
    P, N, _ = case
    _, _, ell, valid, _, free = built(case)
    assert free["iterations"] > 8
    g, cap = _gather(case, dev, batches=1)
    r = _fit(g, case, cap, dev, max_iter=5, chunk=2)
    assert r["converged"] == 0 and r["iterations"] == 5 and r["degenerate"] == 0
    ref = R.fit(ell, valid, N, tol=TOL, max_iter=5)
    n, w = int(r["n"]), r["w"][:P]
    assert np.abs(w - ref["w"]).max() <= R.bound_w(5, n, P)
    # (objective, gap) are those of the reported w
    assert abs(r["objective"] - R.objective(ell, valid, w)) <= R.bound_objective(
        0, n, P, r["gap"], r["objective"])
    assert abs(r["gap"] - ref["gap"]) <= R.bound_gap(5, n, P, ref["gap"]) and r["gap"] > TOL
    assert r["objective"] > r["objective_uniform"]
    assert _fit(g, case, cap, dev, max_iter=5, chunk=5, grid=3).tobytes() == r.tobytes()


def test_nothing_valid_is_degenerate_and_refusals():
    from bayesdll_amd import _lib as L
    dev = torch.device("cuda:0")
    P, N = 3, 40
    g = {"ell": Guarded(P * N * 4, dev), "valid": Guarded(N * 4, dev)}
    g["valid"].buf[256:256 + N * 4] = 0
    r = _fit(g, (P, N, ""), N, dev, max_iter=3)
    assert r["degenerate"] == 1 and r["converged"] == 0 and r["n"] == 0 and r["iterations"] == 0
    assert np.allclose(r["w"][:P], 1 / 3) and np.isnan(r["objective"])
    assert g["ell"].untouched()
    check_refusals()
    assert C.sizeof(L.StackState) == 560


def test_kernels_stack_fit_handle_and_host_reads():
    from bayesdll_amd import kernels as K
    dev = torch.device("cuda:0")
    case = (8, 1025, "equal")
    logp, y, ell, valid, counts, free = built(case)
    P, N, _ = case
    e = torch.zeros(P, 2048, device=dev)
    v = torch.zeros(2048, dtype=torch.int32, device=dev)
    cnt = torch.full((3,), 77, dtype=torch.int64, device=dev)
    lp, yd = torch.from_numpy(logp).to(dev), torch.from_numpy(y).to(dev)
    off = K.stack_gather(lp[:, :500].contiguous(), yd[:500].contiguous(), e, v, cnt, 0, reset=True)
    off = K.stack_gather(lp[:, 500:].contiguous(), yd[500:].contiguous(), e, v, cnt, off)
    assert off == N and dict(zip(("n_label", "n_nonfinite", "n_impossible"), cnt.tolist())) == counts
    st = K.stack_fit(e, v, N)
    s = st.summary()
    st1 = K.stack_fit(e, v, N, check_every=1, grid_blocks=3)
    assert st1.buf.cpu().numpy().tobytes() == st.buf.cpu().numpy().tobytes()
    assert s["converged"] and not s["degenerate"] and s["n"] == free["n"] and s["gap"] <= TOL
    assert st.converged_flag() == 1
    w = st.weights()
    assert w.dtype == torch.float64 and w.shape == (P,) and w.is_cuda
    assert np.array_equal(w.cpu().numpy(), s["weights"])
    s5 = K.stack_fit(e, v, N, max_iter=5, check_every=2).summary()
    assert not s5["converged"] and s5["iterations"] == 5
