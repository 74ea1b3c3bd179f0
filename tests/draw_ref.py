"""Host reference of the posterior draw and the stand-alone moment update —
TEST INFRASTRUCTURE ONLY.

bdl_posterior_sample and bdl_moments_update (bayesdll_amd/csrc/bdl_api.hip)
restated in plain NumPy on np.float32 arrays, one separately rounded operation
per line, from the pieces the other references already hold:

  variance      chain_diag_ref.variance_f32 (posterior_var, bdl_kernels.hpp)
  collects      step_ref.collect / step_ref.Div (moments_elem is collect_core's
                stand-alone twin)
  noise         buffer noise from the host, or the (seed, chain, step) stream
                (tests/philox_ref.py pins the device's generator)

and the two kernels' loop shape (one unguarded grid-stride loop over the full
block iterations, then at most one guarded iteration per workgroup) restated
as a classifier, with the size table the GPU tests launch, so that what the
table reaches is proven on the CPU (tests/test_draw_host.py).  Nothing is
imported from bayesdll_amd and nothing from torch.

Rounding rules: as step_ref.py — scalars are the host's float64 values rounded
to fp32 once; np.sqrt and / on float32 are correctly rounded; the product
s * eps and the sum m1 + t are two roundings (the library is built with
-ffp-contract=off).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import chain_diag_ref as D
import step_ref as R

F = np.float32
VAR_GIVEN, VAR_RAW_MOMENTS, VAR_WELFORD = D.VAR_GIVEN, D.VAR_RAW_MOMENTS, D.VAR_WELFORD
NOISE_BUFFER, NOISE_PHILOX = 1, 2
WELFORD_INIT, WELFORD, MEAN_INIT, MEAN = R.WELFORD_INIT, R.WELFORD, R.MEAN_INIT, R.MEAN
K_BLOCK = 256
FLOORED_MIN = 2.0 ** -96  # var_floor >= this: the FLOORED instances


# ------------------------------------------------------------------- the draw
def draw(m1, m2, eps, *, var_mode, ratio=1.0, inv_ratio=0.0, var_floor=1e-12):
    """out = m1 + sqrt(clamp(var, var_floor)) * eps.  m2 None: no second
    moment, var = var_floor (a NaN floor stays NaN), whatever var_mode says.
    inv_ratio == 0 selects true division of Welford's M2, as
    bdl_posterior_sample does; else var = m2 * inv_ratio."""
    m1, eps = R._a32(m1), R._a32(eps)
    with np.errstate(all="ignore"):
        if m2 is None:
            var = np.full(m1.shape, R.f32(var_floor), F)
        else:
            var = D.variance_f32(m1, R._a32(m2), var_mode, R.f32(ratio), R.f32(inv_ratio),
                                 R.f32(var_floor))
        s = np.sqrt(var)
        t = s * eps
        out = m1 + t
    assert out.dtype == F
    return out


def stacked_eps(normals, *, chains, chain_groups, seed, chain, step):
    """The noise of a stacked draw: chain k's slot [4*cg*k, 4*cg*(k+1)) holds
    the first 4*cg values of the (seed, chain + k, step) stream — the group
    index is counted inside the slot.  normals(n, seed, chain, step) -> the n
    fp32 values of that stream."""
    slot = 4 * int(chain_groups)
    return np.concatenate([np.asarray(normals(slot, seed, int(chain) + k, step), dtype=F)
                           for k in range(int(chains))])


def draw_stacked(m1, m2, normals, *, chains, chain_groups, seed, chain, step, **kw):
    """The stacked draw.  Contract: the launch covers n = K * 4 * chain_groups
    elements, padding of every slot included — the draw reads and writes the
    padding like any other element."""
    n = int(chains) * 4 * int(chain_groups)
    assert len(m1) == n and (m2 is None or len(m2) == n), (len(m1), n)
    eps = stacked_eps(normals, chains=chains, chain_groups=chain_groups, seed=seed, chain=chain,
                      step=step)
    return draw(m1, m2, eps, **kw)


# --------------------------------------------------------- the moment update
def _div(c):
    return c if isinstance(c, R.Div) else R.Div(c)


def moments(kind, x, m1, m2, ca, cb, mode):
    """The stand-alone moment update (bdl_moments_update) of `kind` on x.
    m2 None: no second moment is kept (for the INIT kinds any array stands for
    "kept": neither m1 nor m2 is read).  ca / cb: the host's float64 scalars,
    or step_ref.Div objects (Div.fallback: the reciprocal the library forms
    itself when the caller leaves inv_collect_* 0).  Returns (m1, m2)."""
    sc = SimpleNamespace(ca=_div(ca), cb=_div(cb))
    return R.collect(kind, x, m1, m2, sc, mode)


# ------------------------------------------------------------ kernel instances
# bdl_sample_kernel<VAR, M2, RECIP, NOISE, FLOORED, U> as pick_sample returns
# them, and bdl_moments_kernel<COLLECT, RECIP, M2, 4> as pick_moments does.
def sample_instance(var_mode, m2, recip, noise, floored, unroll):
    """The template arguments pick_sample maps a launch's inputs to."""
    if not m2:
        var_mode, recip = VAR_GIVEN, False
    elif var_mode != VAR_WELFORD:
        recip = False
    return (int(var_mode), bool(m2), bool(recip), int(noise), bool(floored), 1 if unroll == 1 else 4)


def moments_instance(collect, recip, m2):
    return (int(collect), bool(recip), bool(m2))


_VAR_SOURCES = [(VAR_RAW_MOMENTS, True, False), (VAR_WELFORD, True, False),
                (VAR_WELFORD, True, True), (VAR_GIVEN, True, False), (VAR_GIVEN, False, False)]
DRAW_INSTANCES = [(v, m2, rc, nz, fl, u) for v, m2, rc in _VAR_SOURCES
                  for nz in (NOISE_BUFFER, NOISE_PHILOX) for fl in (True, False) for u in (1, 4)]
MOMENTS_INSTANCES = [(c, rc, m2) for c in (WELFORD_INIT, WELFORD, MEAN_INIT, MEAN)
                     for rc in (False, True) for m2 in (True, False)]
_VAR_NAMES = {VAR_GIVEN: "GIVEN", VAR_RAW_MOMENTS: "RAW_MOMENTS", VAR_WELFORD: "WELFORD"}
_COLLECT_NAMES = {WELFORD_INIT: "WELFORD_INIT", WELFORD: "WELFORD", MEAN_INIT: "MEAN_INIT",
                  MEAN: "MEAN"}


def draw_id(inst):
    v, m2, rc, nz, fl, u = inst
    return "%s-%s-%s-%s-%s-U%d" % (_VAR_NAMES[v], "m2" if m2 else "nom2", "recip" if rc else "true",
                                   "buffer" if nz == NOISE_BUFFER else "philox",
                                   "floored" if fl else "unfloored", u)


def moments_id(inst):
    c, rc, m2 = inst
    return "%s-%s-%s" % (_COLLECT_NAMES[c], "recip" if rc else "true", "m2" if m2 else "nom2")


# ------------------------------------------------------------- the loop shape
def grid_of(n, cus, blocks_per_cu, unroll):
    """grid_sample / grid_for: one workgroup per block iteration, capped at
    cus * blocks_per_cu, never empty."""
    per = K_BLOCK * unroll
    want = ((n + 3) // 4 + per - 1) // per
    return max(1, min(want, cus * blocks_per_cu))


def sweep(n, cus, blocks_per_cu, unroll):
    """What every workgroup of a launch over n elements does: a list of
    (full_trips, tail), one entry per workgroup.  tail is None when the
    guarded iteration does not run, else a tuple of `unroll` lane counts: how
    many of the 256 lanes run unrolled slot u (a lane leaves at the first u
    with gb + 256 * u + lane >= ngroups: `break`)."""
    kiter = K_BLOCK * unroll
    nfull, ngroups = n >> 2, (n + 3) >> 2
    grid = grid_of(n, cus, blocks_per_cu, unroll)
    stride = grid * kiter
    out = []
    for b in range(grid):
        gb, trips = b * kiter, 0
        while gb + kiter <= nfull:
            trips += 1
            gb += stride
        tail = None
        if gb < ngroups:
            tail = tuple(max(0, min(K_BLOCK, ngroups - gb - K_BLOCK * u)) for u in range(unroll))
        out.append((trips, tail))
    return out


def breaks_of(tail):
    """The slots at which some lane of a guarded iteration leaves the unrolled
    loop (None: a lane that runs every slot)."""
    prev, at = K_BLOCK, set()
    for u, lanes in enumerate(tail):
        if lanes < prev:
            at.add(u)
        prev = lanes
    if tail[-1] > 0:
        at.add(None)
    return at


def size_table(cus, blocks_per_cu, unroll):
    """The sizes the GPU tests launch at geometry (blocks_per_cu, unroll) on a
    device of `cus` compute units."""
    kiter = K_BLOCK * unroll
    span = 4 * kiter * cus * blocks_per_cu  # elements of one trip of the whole grid
    return [1, 3, 4, 5, 4 * kiter - 1, 4 * kiter, 4 * kiter + 1, span, 2 * span] + \
        [2 * span + 4 * kiter * 3 + 4 * (K_BLOCK + 37) + r for r in (1, 2, 3)]


def check_size_table(sizes, cus, blocks_per_cu, unroll):
    """Assert what the GPU tests claim of their sizes at this geometry."""
    kiter = K_BLOCK * unroll
    span = 4 * kiter * cus * blocks_per_cu
    sweeps = {n: sweep(n, cus, blocks_per_cu, unroll) for n in sizes}
    every = [w for s in sweeps.values() for w in s]
    where = (cus, blocks_per_cu, unroll)
    assert any(t >= 2 and tail is not None for t, tail in every), ("two trips, then a tail", where)
    assert any(t >= 2 and tail is None for t, tail in every), ("two trips, no tail", where)
    breaks = set().union(*[breaks_of(tail) for _, tail in every if tail is not None])
    assert 0 in breaks and None in breaks, ("break at slot 0 / not at all", where, breaks)
    if unroll > 1:
        assert any(u not in (0, None) for u in breaks), ("break inside the unroll", where, breaks)
    assert {n % 4 for n in sizes} >= {1, 2, 3}, where
    assert any(n < 4 for n in sizes), where
    assert any(n % span == 0 for n in sizes), ("an exact multiple of one whole-grid trip", where)
    # the largest sizes: every workgroup takes two full trips
    big = sweeps[max(sizes)]
    assert len(big) == cus * blocks_per_cu and all(t >= 2 for t, _ in big), where
    return sweeps
