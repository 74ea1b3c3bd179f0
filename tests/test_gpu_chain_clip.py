"""bdl_chain_clip (include/bdl_clip.h) on the GPU against its NumPy restatement
(tests/chain_clip_ref.py), over the stacked tables of tests/stacked_tables.py.

Every case lives in ONE arena of 32-bit words preset to a guard pattern (a
NaN: a norm that read it would be NaN); the chains' slices are written into it
and the whole arena is compared as int32 afterwards, so guard words before and
after every buffer, a chain's padding, a frozen tensor's span, the unclipped
chains and the clipped values are all checked by one comparison:

  tensor  every trainable tensor its own [K, numel] block (chain stride =
          numel) between guard words; table A holds numel 3, 5, 4, 8, 12 and
          10 (chain slices that are misaligned and shorter than a float4), and
          one block starts one element past a 16-B boundary (a view's base).
  flat    one [K, stride] buffer (chain stride = the padded chain slot); the
          2-element padding of every chain and the frozen l7.weight span keep
          the guard NaN and belong to no segment.

Chain k's gradient is scaled to a multiple of max_norm (0.25, 1.001 — just on
the clipped side —, 4, 0.9, 1.5 by chain), so the chains straddle the
threshold: a norm taken over all chains would scale the small chain too."""
import functools

import numpy as np
import pytest
import torch

import chain_clip_ref as R
from stacked_tables import FROZEN, SEGMENTS, SEGMENTS_B, Layout
from step_ref import clip_coef

pytestmark = pytest.mark.gpu
DEV = "cuda"

GUARD = np.int32(0x7FC0DEAD)      # a quiet NaN with a payload nothing computes
MISALIGNED = "l3.weight"          # tensor mode: this block starts at 4q + 1
TARGETS = [0.25, 1.001, 4.0, 0.9, 1.5]
MAX_NORM = 0.75
BPC = [1, 1024]                   # one workgroup per chain, and the cap

CASES = {"A-tensor": (SEGMENTS, 3, "tensor"), "A-flat": (SEGMENTS, 3, "flat"),
         "B-tensor": (SEGMENTS_B, 5, "tensor"), "one-chain": (SEGMENTS, 1, "tensor"),
         "one-chain-flat": (SEGMENTS, 1, "flat")}


def _place(lay, mode):
    """[(arena offset, numel, chain stride)] of the trainable tensors, and the
    arena's size in words."""
    segs = []
    if mode == "flat":
        for nm, o, n in zip(lay.names, lay.offsets, lay.numels):
            if nm != FROZEN:
                segs.append((8 + o, n, lay.stride))
        return segs, 8 + lay.K * lay.stride + 8
    pos = 8
    for nm, n in zip(lay.names, lay.numels):
        if nm == FROZEN:
            continue
        off = pos + (1 if nm == MISALIGNED else 0)
        segs.append((off, n, n))
        pos = (off + lay.K * n + 8 + 3) // 4 * 4   # >= 8 guard words, blocks 16-B aligned
    return segs, pos


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """The arena of a case (host, int32), its segments, and the reference's
    (norms, coefs, max_norm).  kind: "random" or "integer"."""
    segments, K_, mode = CASES[name]
    lay = Layout(segments, K_)
    segs, total = _place(lay, mode)
    rng = np.random.default_rng(sum(map(ord, name + kind)))
    arena = np.full(total, GUARD, dtype=np.int32)
    f = arena.view(np.float32)
    if kind == "integer":  # |g| <= 8, chain k drawn from [-(1 + 3k'), 1 + 3k']
        widths = [1, 4, 8, 2, 6]
        for k in range(K_):
            w = widths[k % 5]
            for off, n, stride in segs:
                f[off + k * stride: off + k * stride + n] = rng.integers(-w, w + 1, n)
        chains = [[f[off + k * stride: off + k * stride + n].copy() for off, n, stride in segs]
                  for k in range(K_)]
        nr = sorted(float(R.chain_norm(sl)) for sl in chains)
        max_norm = nr[0] * 0.5 if K_ == 1 else 0.5 * (nr[0] + nr[1])
    else:
        max_norm = MAX_NORM
        for k in range(K_):
            t = TARGETS[k % 5] if K_ > 1 else 4.0
            sl = [rng.standard_normal(n).astype(np.float32) for _, n, _ in segs]
            nrm = np.sqrt(sum(float(np.dot(g.astype(np.float64), g.astype(np.float64)))
                              for g in sl))
            for g, (off, n, stride) in zip(sl, segs):
                f[off + k * stride: off + k * stride + n] = g * np.float32(t * max_norm / nrm)
        chains = [[f[off + k * stride: off + k * stride + n].copy() for off, n, stride in segs]
                  for k in range(K_)]
    norms, coefs, _ = R.chain_clip(chains, max_norm)
    arena.setflags(write=False)
    return arena, tuple(segs), K_, norms, coefs, float(max_norm)


def _run(arena, segs, K_, max_norm, bpc):
    """One bdl_chain_clip over a device copy of the arena, the workspace
    between guard words of its own.  Returns (arena after, table [K, 2]) on
    the host."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    dev = torch.from_numpy(arena.copy()).to(DEV)
    base = dev.data_ptr()
    assert base % 16 == 0
    table = torch.tensor([[base + 4 * off, n, stride] for off, n, stride in segs],
                         dtype=torch.int64).to(DEV)
    nws = int(L.lib().bdl_chain_clip_workspace_bytes(K_)) // 4
    wsbuf = torch.from_numpy(np.full(nws + 16, GUARD, dtype=np.int32)).to(DEV)
    ws = wsbuf[8:8 + nws].view(torch.float32)
    out = K.chain_clip(table, len(segs), K_, max_norm, workspace=ws, blocks_per_chain=bpc)
    assert out.shape == (K_, 2) and out.data_ptr() == ws.data_ptr()
    torch.cuda.synchronize()
    wsh = wsbuf.cpu().numpy()
    # only bdl_chain_clip_workspace_bytes(K) bytes of the workspace are written
    assert (wsh[:8] == GUARD).all() and (wsh[8 + nws:] == GUARD).all()
    return dev.cpu().numpy(), out.cpu().numpy().copy()


def _expected(arena, segs, K_, coefs_dev):
    want = arena.copy()
    f = want.view(np.float32)
    for k in range(K_):
        for off, n, stride in segs:
            sl = slice(off + k * stride, off + k * stride + n)
            f[sl] = R.scale(f[sl].copy(), coefs_dev[k])
    return want


def test_tables_hold_what_the_cases_claim():
    lay = Layout(SEGMENTS, 3)
    segs, _ = _place(lay, "tensor")
    assert len(segs) == 19 and lay.stride == 39428 and lay.stride - lay.n1 == 2
    assert {3, 5, 4, 8, 12, 10} <= {n for _, n, _ in segs}
    # misaligned bases: the view, and chains 1.. of every tensor with numel % 4 != 0
    assert sum(1 for off, _, _ in segs if off % 4) == 1
    assert sum(1 for off, n, s in segs for k in range(3) if (off + k * s) % 4) == 8
    # both sweep paths at both geometries: a body of whole block iterations plus a rest
    assert max(n for _, n, _ in segs) // 4 > 3 * 1024
    fl, total = _place(lay, "flat")
    assert len(fl) == 19 and total == 16 + 3 * 39428 and all(s == 39428 for _, _, s in fl)


@pytest.mark.parametrize("name", list(CASES))
def test_random_gradient_each_chain_by_its_own_norm(name):
    arena, segs, K_, norms, coefs, max_norm = _case(name, "random")
    if K_ > 1:  # the chains straddle the threshold
        assert (coefs < 1).any() and (coefs == 1).any()
    seen = []
    for bpc in BPC:
        after, tab = _run(arena, segs, K_, max_norm, bpc)
        print(name, bpc, "norm dev", tab[:, 0], "ref", norms, "coef dev", tab[:, 1])
        for k in range(K_):
            assert R.within_one_ulp(tab[k, 0], norms[k]), (name, bpc, k, tab[k, 0], norms[k])
            assert tab[k, 1].view(np.int32) == np.float32(
                clip_coef(tab[k, 0], max_norm)).view(np.int32), (name, bpc, k)
            assert (tab[k, 1] < 1) == (coefs[k] < 1), (name, bpc, k)
        want = _expected(arena, segs, K_, tab[:, 1])
        bad = np.flatnonzero(after != want)
        assert bad.size == 0, (name, bpc, bad[:8], bad.size)
        for k in np.flatnonzero(tab[:, 1] == 1):  # unclipped chains kept their words
            for off, n, stride in segs:
                sl = slice(off + k * stride, off + k * stride + n)
                assert np.array_equal(after[sl], arena[sl])
        seen.append(tab)
    for k in range(K_):  # between geometries only the fp64 summation order differs
        assert R.within_one_ulp(seen[0][k, 0], seen[1][k, 0]), (name, k)


@pytest.mark.parametrize("name", ["A-tensor", "A-flat", "B-tensor"])
def test_integer_gradient_is_exact_in_every_geometry(name):
    """|g| <= 8 and integer: every product and partial sum is an integer far
    below 2^53, so the fp64 sum is exact in any order — norm, coefficient and
    every output word equal the reference's and each other's bit for bit."""
    arena, segs, K_, norms, coefs, max_norm = _case(name, "integer")
    assert (coefs < 1).any() and (coefs == 1).any()
    want = _expected(arena, segs, K_, coefs)
    for bpc in BPC + [0, 7]:
        after, tab = _run(arena, segs, K_, max_norm, bpc)
        assert np.array_equal(tab[:, 0].view(np.int32), norms.view(np.int32)), (name, bpc)
        assert np.array_equal(tab[:, 1].view(np.int32), coefs.view(np.int32)), (name, bpc)
        assert np.array_equal(after, want), (name, bpc)


def test_runs_are_bit_identical_at_a_fixed_geometry():
    arena, segs, K_, _, _, max_norm = _case("A-tensor", "random")
    a1, t1 = _run(arena, segs, K_, max_norm, 5)
    a2, t2 = _run(arena, segs, K_, max_norm, 5)
    assert np.array_equal(a1, a2) and np.array_equal(t1.view(np.int32), t2.view(np.int32))


def test_stacked_state_builds_the_segment_table(monkeypatch):
    """StackedState.grad_segments in both gradient modes: one row per tensor
    with a gradient, cached per set of gradient addresses."""
    import torch.nn as nn
    from bayesdll_amd import stacked
    net = nn.Sequential(nn.Linear(13, 7), nn.Tanh(), nn.Linear(7, 5)).cuda()
    net[0].bias.requires_grad_(False)
    for mode in ("tensor", "flat"):
        if mode == "flat":
            monkeypatch.setattr(stacked, "MAX_TENSOR_RUNS", 2)
        st = stacked.StackedState(net, 3, readout_name="2")
        assert st.grad_mode == mode
        with pytest.raises(ValueError, match="before use_grads"):
            st.grad_segments()
        grads = {nm: torch.randn(3, *s, device=DEV) for nm, s, rg in
                 zip(st.names, st.shapes, st.requires_grad) if rg}
        st.use_grads(grads)
        tab, nseg = st.grad_segments()
        assert nseg == 3 and tab.shape == (3, 3) and tab.dtype == torch.int64 and tab.is_cuda
        rows = tab.cpu().tolist()
        names = [nm for nm, rg in zip(st.names, st.requires_grad) if rg]
        for (ptr, n, stride), nm in zip(rows, names):
            i = st.names.index(nm)
            if mode == "tensor":
                assert (ptr, n, stride) == (grads[nm].data_ptr(), st.numels[i], st.numels[i])
            else:
                assert (ptr, n, stride) == (st.grad.data_ptr() + 4 * st.offsets[i], st.numels[i],
                                            st.stride)
        assert st.grad_segments()[0] is tab          # cached
        st.use_grads(grads)
        assert st.grad_segments()[0] is tab
