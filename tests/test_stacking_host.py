"""The stacking unit (include/bdl_stacking.h) without a GPU: the header's
declarations, the export table and the ctypes mirrors against the C layout; the
NumPy reference's own properties (a non-decreasing objective, the gap as a
certificate at every iterate against an independent solver, the tile table's
paths); every refusal of the two entry points by its status code (fake
pointers: each call returns before any HIP call); the refusals of
weights="stacking" and of the Python layers before any device work."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stacking_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NULL, ALIGN, ARG = -1, -2, -3


# ------------------------------------------------------------------ the ABI
def test_header_declares_exactly_the_three_entry_points_and_is_additive():
    text = open(os.path.join(INCLUDE, "bdl_stacking.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fns = re.findall(r"^\s*(?:int|int64_t|void|const char\*)\s+(bdl_\w+)\s*\(", code, flags=re.M)
    assert sorted(fns) == ["bdl_stack_fit", "bdl_stack_gather", "bdl_stack_workspace_bytes"]
    assert '#include "bdl_sgmcmc.h"' in code and "BDL_ABI_VERSION" not in code
    # the header states why gap is a certificate and why s > 0
    assert "CERTIFICATE" in text and "s > 0 always" in text and ">= 1/n" in text
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.STACK_EXPORTS) == set(fns) and all(hasattr(h, f) for f in fns)
    assert h.bdl_version() == L.ABI_VERSION == 8
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_stacking" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "bdl_stacking.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    assert "-ffp-contract=off" in mk.split("CFLAGS :=")[1].splitlines()[0]
    src = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "bdl_stacking.hip")).read()
    assert "atomic" not in src.lower() and "hipMalloc" not in src and "Synchronize" not in src
    assert "nontemporal" not in src  # the matrix is re-read every iteration: cached loads


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    structs = {"bdl_stack_state": L.StackState, "bdl_stack_gather_args": L.StackGatherArgs,
               "bdl_stack_fit_args": L.StackFitArgs}
    lines = []
    for st, cls in structs.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("caps %d %d %d %d %d %d %d %d %d\\n", BDL_STACK_MAX_VOTERS, '
                 'BDL_STACK_MAX_CLASSES, BDL_STACK_MAX_COLS, BDL_STACK_TILE, BDL_STACK_MAX_GRID, '
                 'BDL_STACK_MAX_CHUNK, BDL_STACK_RESET, BDL_STACK_FIRST, BDL_STACK_FINAL);')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_stacking.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    out = subprocess.check_output([str(exe)]).decode().strip().splitlines()
    caps = [int(v) for v in next(ln for ln in out if ln.startswith("caps ")).split()[1:]]
    lay = {k: int(v) for k, v in (ln.rsplit(" ", 1) for ln in out if not ln.startswith("caps "))}
    for st, cls in structs.items():
        assert lay[st] == C.sizeof(cls), st
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[f"{st}.{f}"], (st, f)
    assert caps == [L.STACK_MAX_VOTERS, L.STACK_MAX_CLASSES, L.STACK_MAX_COLS, L.STACK_TILE,
                    L.STACK_MAX_GRID, L.STACK_MAX_CHUNK, L.STACK_RESET, L.STACK_FIRST,
                    L.STACK_FINAL]
    assert caps[:4] == [R.MAX_VOTERS, R.MAX_CLASSES, R.MAX_COLS, R.TILE]
    assert C.sizeof(L.StackState) % 8 == 0 and L.StackState.converged.offset % 4 == 0


def test_workspace_bytes():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_stack_workspace_bytes(64, 50000) == 49 * 67 * 8
    assert h.bdl_stack_workspace_bytes(1, 1) == 1024 * 3 * 8        # the gather's counts
    assert h.bdl_stack_workspace_bytes(64, 1 << 24) == 16384 * 67 * 8
    for P, N in ((0, 5), (65, 5), (3, 0), (3, (1 << 24) + 1)):
        assert h.bdl_stack_workspace_bytes(P, N) == 0


# ------------------------------------------------------------ the refusals
def _good_gather():
    from bayesdll_amd import _lib as L
    a = L.StackGatherArgs()
    # logp 3*10*7*4 = 840 B, labels 80 B, ell 3*64*4 = 768 B, valid 256 B, counters 24 B,
    # workspace 24576 B
    a.logp, a.labels, a.ell, a.valid = 0x10000, 0x20000, 0x30000, 0x40000
    a.counters, a.workspace = 0x50000, 0x60000
    a.batch, a.off, a.cap, a.voters, a.classes = 10, 5, 64, 3, 7
    return a


def _good_fit():
    from bayesdll_amd import _lib as L
    a = L.StackFitArgs()
    a.ell, a.valid, a.state, a.workspace = 0x30000, 0x40000, 0x50000, 0x60000
    a.n_cols, a.cap, a.tol, a.voters, a.iterations = 60, 64, 1e-4, 3, 4
    a.flags = L.STACK_FIRST
    return a


def check_refusals():
    """Every refusal of bdl_stack_gather and bdl_stack_fit by its status code;
    validation comes before any HIP call, so the planted addresses are never
    touched."""
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(fn, good, status, word, **fields):
        a = good()
        for k, v in fields.items():
            setattr(a, k, v)
        assert getattr(h, fn)(a, None) == status, (fn, fields, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(fn.encode() + b":") and word in msg, (fields, msg)

    g = lambda *a, **k: refused("bdl_stack_gather", _good_gather, *a, **k)  # noqa: E731
    f = lambda *a, **k: refused("bdl_stack_fit", _good_fit, *a, **k)  # noqa: E731
    assert h.bdl_stack_gather(None, None) == NULL and b"null args" in h.bdl_last_error()
    assert h.bdl_stack_fit(None, None) == NULL and b"null args" in h.bdl_last_error()
    for name in ("logp", "labels", "ell", "valid", "counters", "workspace"):
        g(NULL, b"null " + name.encode(), **{name: None})
    for name in ("ell", "valid", "state", "workspace"):
        f(NULL, b"null " + name.encode(), **{name: None})
    for name in ("logp", "ell", "valid"):
        g(ALIGN, name.encode() + b" not 4-B aligned", **{name: 0x700002})
    for name in ("labels", "counters", "workspace"):
        g(ALIGN, name.encode() + b" not 8-B aligned", **{name: 0x700004})
    for name in ("ell", "valid"):
        f(ALIGN, name.encode() + b" not 4-B aligned", **{name: 0x700002})
    for name in ("state", "workspace"):
        f(ALIGN, name.encode() + b" not 8-B aligned", **{name: 0x700004})
    for v in (0, -1, 65):
        g(ARG, b"voters in", voters=v)
        f(ARG, b"voters in", voters=v)
    g(ARG, b"batch must be", batch=0)
    for v in (0, 8193):
        g(ARG, b"classes in", classes=v)
    for v in (0, (1 << 24) + 1):
        g(ARG, b"cap in", cap=v)
        f(ARG, b"cap in", cap=v)
    g(ARG, b"must lie in [0, cap)", off=-1)
    g(ARG, b"must lie in [0, cap)", off=55)      # 55 + 10 > 64
    g(ARG, b"must lie in [0, cap)", off=65)
    for v in (-1, 1025):
        g(ARG, b"grid_blocks in", grid_blocks=v)
        f(ARG, b"grid_blocks in", grid_blocks=v)
    g(ARG, b"unknown flag", flags=2)
    f(ARG, b"unknown flag", flags=1)
    for v in (0, 65):
        f(ARG, b"n_cols in", n_cols=v)
    for v in (-1e-9, float("nan")):
        f(ARG, b"tol must be", tol=v)
    for v in (-1, 65537):
        f(ARG, b"iterations in", iterations=v)
    f(ARG, b"nothing to enqueue", iterations=0)
    g(ARG, b"ell overlaps logp", ell=0x10000 + 836)
    g(ARG, b"ell overlaps labels", ell=0x20000 - 764)
    g(ARG, b"valid overlaps ell", valid=0x30000 + 764)
    g(ARG, b"counters overlaps valid", counters=0x40000 + 248)
    g(ARG, b"workspace overlaps counters", workspace=0x50000 - 24568)
    g(ARG, b"workspace overlaps logp", workspace=0x10000 + 832)
    f(ARG, b"state overlaps ell", state=0x30000 + 760)
    f(ARG, b"state overlaps valid", state=0x40000 - 552)
    f(ARG, b"workspace overlaps state", workspace=0x50000 + 552)
    f(ARG, b"workspace overlaps ell", workspace=0x30000 - 24568)
    # spans just clear of their neighbours pass validation up to a planted last check
    a = _good_gather()
    a.ell, a.flags = 0x10000 + 840, 2
    assert h.bdl_stack_gather(a, None) == ARG and b"unknown flag" in h.bdl_last_error()
    # a graph redirect refuses first
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        for fn, good in (("bdl_stack_gather", _good_gather), ("bdl_stack_fit", _good_fit)):
            assert getattr(h, fn)(good(), None) == ARG
            assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)


def test_both_entry_points_validate_before_touching_the_device():
    check_refusals()


# ---------------------------------------------------------- the reference
CASES = [(3, 37, "graded"), (4, 600, "disjoint"), (8, 1500, "equal"), (2, 1025, "graded"),
         (64, 1030, "graded")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_reference_objective_never_decreases_and_gap_certifies_every_iterate(case):
    P, N, kind = case
    logp, y = R.make_case(P, N, kind=kind, seed=P + N)
    ell, valid, counts = R.gather(logp, y)
    assert counts == {"n_label": 2, "n_nonfinite": 2, "n_impossible": 1}
    assert valid.sum() == N - 5 and not ell[:, valid == 0].any()
    assert np.isneginf(ell[:, valid == 1]).any() and np.isfinite(ell[:, valid == 1].max(0)).all()
    f = R.fit(ell, valid, N)
    assert f["converged"] and f["iterations"] <= 702 and f["n"] == N - 5
    obj, gaps = np.array(f["objectives"]), np.array(f["gaps"])
    assert (np.diff(obj) >= -1e-13).all()
    _, f_indep, gap_indep = R.solve(ell, valid)
    assert gap_indep <= (1e-9 if P <= 8 else 1e-4)
    assert (f_indep - obj <= gaps + 1e-12).all()            # the certificate, at every iterate
    assert f["objective"] >= f_indep - 1e-4 and f["objective"] <= f_indep + gap_indep + 1e-12
    assert abs(f["w"].sum() - 1) < 1e-14 and (f["w"] > 0).all()
    assert f["objective"] == pytest.approx(R.objective(ell, valid, f["w"]), abs=1e-6)
    assert f["objective_uniform"] == pytest.approx(
        R.objective(ell, valid, np.full(P, 1 / P)), abs=1e-6)
    # forced to the same count, the fit is the same fit
    f2 = R.fit(ell, valid, N, updates=f["iterations"])
    assert np.array_equal(f2["w"], f["w"]) and f2["gap"] == f["gap"] and f2["converged"]
    # max_iter exhausted: one evaluation-only pass, (w, objective, gap) consistent
    f5 = R.fit(ell, valid, N, max_iter=5)
    if f["iterations"] > 5:
        assert not f5["converged"] and f5["iterations"] == 5 and len(f5["gaps"]) == 6
        assert f5["objective"] == pytest.approx(R.objective(ell, valid, f5["w"]), abs=1e-6)


def test_reference_special_cases():
    logp, y = R.make_case(1, 37)
    ell, valid, _ = R.gather(logp, y)
    f = R.fit(ell, valid, 37)
    assert f["iterations"] == 0 and f["converged"] and f["gap"] == 0 and f["w"].tolist() == [1.0]
    # two identical voters keep identical weights; the sole coverer keeps w >= 1/n
    logp, y = R.make_case(3, 200, kind="disjoint", seed=3)
    ell, valid, _ = R.gather(logp, y)
    assert np.array_equal(ell[2], ell[1]) and np.isneginf(ell[1:, 13]).all() and valid[13]
    for T in range(0, 30, 3):
        w = R.fit(ell, valid, 200, updates=T)["w"]
        assert w[1] == w[2] and w[0] >= 1 / valid.sum()
    # nothing valid: degenerate
    f = R.fit(np.zeros((2, 5), np.float32), np.zeros(5, np.int32), 5)
    assert f["degenerate"] and f["n"] == 0 and not f["converged"]
    # P = 2: the bisection and EM agree
    logp, y = R.make_case(2, 300, seed=9)
    ell, valid, _ = R.gather(logp, y)
    w, fi, gi = R.solve(ell, valid)
    f = R.fit(ell, valid, 300, tol=1e-7, max_iter=20000)
    assert gi < 1e-9 and f["converged"] and abs(f["objective"] - fi) < 1e-7


def test_tile_table_reaches_every_path():
    """N = 1, exactly one tile, one more, several with a short last one, and
    more workgroups than tiles; a tile's partial does not depend on the grid."""
    for N, ntiles, last in ((1, 1, 1), (1024, 1, 1024), (1025, 2, 1), (2600, 3, 552)):
        for grid in (1, 3, 1024):
            tab = R.tile_table(N, grid)
            assert len(tab) == ntiles and tab[-1][3] == last
            assert [t[1:] for t in tab] == [t[1:] for t in R.tile_table(N, 1)]
            assert sum(t[3] for t in tab) == N and all(t[0] < grid for t in tab)
            idle = grid - len({t[0] for t in tab})
            assert (idle > 0) == (grid > ntiles)
    assert len({t[0] for t in R.tile_table(2600, 3)}) == 3
    assert len({t[0] for t in R.tile_table(2600, 1)}) == 1
    # the literal sum order differs from a plain sum only in rounding
    rng = np.random.default_rng(0)
    v = rng.random((2, 3 * 1024))
    assert np.allclose(R._tile_sums(v), v.sum(-1), rtol=1e-13)
    assert R._tile_sums(np.ones((1, 1024)))[0] == 1024.0


def test_bounds_are_the_documented_formulas():
    u = 2.0 ** -24
    assert R.eta(1000, 8) == 6 * u + 1008 * 2.0 ** -52
    assert R.bound_w(9, 1000, 8) == 10 * R.eta(1000, 8)
    assert R.bound_gap(9, 1000, 8, 0.5) == 1.5 * 11 * R.eta(1000, 8)
    assert R.bound_objective(9, 1000, 8, 0.5, -2.0) == 3 * u + R.bound_w(9, 1000, 8) \
        + 1008 * 2.0 ** -52 * 2
    assert R.iteration_range([1.0, 0.5, 1.00001e-4, 0.9e-4, 1e-5], 1e-4, 100, 4) == (2, 3)


# ------------------------------------------------------ the Python layers
def test_kernels_layer_checks_before_any_launch(monkeypatch):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    ell, valid = torch.zeros(3, 64), torch.zeros(64, dtype=torch.int32)
    cnt, y = torch.zeros(3, dtype=torch.int64), torch.zeros(10, dtype=torch.int64)
    lp = torch.zeros(3, 10, 7)
    with pytest.raises(ValueError, match=r"float32 \[P, cap\]"):
        K.stack_fit(torch.zeros(3, 64, dtype=torch.float64), valid, 10)
    with pytest.raises(ValueError, match="voters <= 64"):
        K.stack_fit(torch.zeros(65, 4), torch.zeros(4, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="valid must be"):
        K.stack_fit(ell, torch.zeros(63, dtype=torch.int32), 10)
    with pytest.raises(ValueError, match="n_cols <= cap"):
        K.stack_fit(ell, valid, 65)
    with pytest.raises(ValueError, match="tol >= 0"):
        K.stack_fit(ell, valid, 10, tol=-1.0)
    with pytest.raises(ValueError, match="max_iter >= 1"):
        K.stack_fit(ell, valid, 10, max_iter=0)
    with pytest.raises(ValueError, match="check_every"):
        K.stack_fit(ell, valid, 10, check_every=0)
    with pytest.raises(ValueError, match="grid_blocks in"):
        K.stack_fit(ell, valid, 10, grid_blocks=1025)
    with pytest.raises(ValueError, match="logp must be"):
        K.stack_gather(torch.zeros(2, 10, 7), y, ell, valid, cnt, 0)
    with pytest.raises(ValueError, match="classes <= 8192"):
        K.stack_gather(torch.zeros(3, 1, 8193), y[:1], ell, valid, cnt, 0)
    with pytest.raises(ValueError, match="labels must be"):
        K.stack_gather(lp, y.int(), ell, valid, cnt, 0)
    with pytest.raises(ValueError, match="counters must be"):
        K.stack_gather(lp, y, ell, valid, cnt[:2], 0)
    with pytest.raises(ValueError, match="do not fit cap"):
        K.stack_gather(lp, y, ell, valid, cnt, 55)


def _fake(**kw):
    from bayesdll_amd import stacked
    d = dict(args=SimpleNamespace(device="cpu"), K=3, per_chain=None, cyclical=False,
             stacking_=None, _component_keys=lambda: [], chain0=0)
    d.update(kw)
    S = SimpleNamespace(**d)
    S._stacking_weights = lambda *a: stacked._StackedSampler._stacking_weights(S, *a)
    S._need_cyclical = lambda what: stacked._StackedSampler._need_cyclical(S, what)
    return S


def test_weights_stacking_refusals_come_before_any_device_work(monkeypatch):
    from bayesdll_amd import chains, stacked
    mw = stacked._StackedSampler._mixture_weights
    S = _fake()
    with pytest.raises(ValueError, match=r'needs a fit_stacking\(\) first'):
        mw(S, "evaluate", "stacking", "arithmetic", False)
    with pytest.raises(ValueError, match="pooled form only"):
        mw(S, "evaluate_chains", "stacking", "arithmetic", True)
    with pytest.raises(ValueError, match='combine="reference" is one Runner'):
        mw(S, "evaluate", "stacking", "reference", False)
    with pytest.raises(ValueError, match="combine from"):
        mw(S, "evaluate", "stacking", "geometric", False)
    # every other value keeps the refusal it had, word for word
    with pytest.raises(ValueError) as e:
        mw(S, "evaluate", "bma", "arithmetic", False)
    assert str(e.value) == 'evaluate: weights is None (uniform) or "gmm" (got \'bma\')'
    with pytest.raises(ValueError) as e:
        mw(S, "uncertainty", "gmm", "arithmetic", False)
    assert str(e.value).startswith('uncertainty: weights="gmm": SimpleNamespace is not cyclical')
    with pytest.raises(ValueError) as e:
        mw(_fake(cyclical=True, per_chain={"lr": [1, 2, 3]}), "evaluate", "gmm", "arithmetic",
           False)
    assert "would weigh different models against each other" in str(e.value)
    # allowed under per_chain and for a non-cyclical sampler: the pooled table w_k / components
    w = torch.tensor([0.5, 0.25, 0.25], dtype=torch.float64)
    for comps in (0, 1, 2):
        S = _fake(stacking_=w, per_chain={"lr": [1, 2, 3]},
                  _component_keys=lambda c=comps: list(range(c)))
        t = mw(S, "evaluate", "stacking", "arithmetic", False)
        c = max(1, comps)
        assert t.shape == (c * 3, 1) and t.dtype == torch.float64 and t.is_contiguous()
        assert torch.equal(t.view(c, 3), (w / c).expand(c, 3))
    monkeypatch.setattr(chains, "world", lambda: 2)
    with pytest.raises(ValueError, match="this process's chains only"):
        mw(_fake(stacking_=w), "evaluate", "stacking", "arithmetic", False)
    with pytest.raises(ValueError, match="this process's chains only"):
        stacked._StackedSampler.fit_stacking(_fake(), [])
