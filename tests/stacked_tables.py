"""Stacked-chain tables for the step kernels' tests — TEST INFRASTRUCTURE ONLY.

K chains of one segment table, stacked chain-major with every chain's slot
padded to a multiple of 4 elements (bayesdll_amd.stacked.StackedState's
layout), and a pure-Python restatement of how the step sweep cuts a launch
into block iterations and which of its three paths each iteration takes
(bdl_kernels.hpp step_body: chunk_fast / chunk_multi / chunk_slow; the Adam
sweep classifies in the same way).  No launch and no device is needed here:
tests/test_stacked_tables_host.py proves on the CPU that the tables reach the
paths tests/test_gpu_stacked_reference.py claims for them.

  A  K = 3 chains of the 39,426-element table of test_gpu_noise_units.py:
     stride 39,428 (a 2-element SKIP gap per chain), 9,857 groups per chain
     (9,857 mod 256 = 129: every chain starts at another lane phase).
  B  K = 5 chains of one 6,000-element tensor: no padding, equal attributes
     on both sides of every seam, so the whole stack is ONE run and the seams
     lie inside fast-path iterations (lanes of one wave in different chains).
  C  K = 6 chains of a 2,000-element body tensor and a 1,000-element head
     tensor: no padding, 4-aligned runs whose attributes alternate across
     every seam (the multi-run path).
"""
from __future__ import annotations

import numpy as np

from test_gpu_noise_units import FROZEN, SEGMENTS

K_BLOCK = 256  # bdl_kernels.hpp kBlock: float4 groups per unroll step of a block
ATTR_SKIP, ATTR_GUNALIGNED = 0x4, 0x8
NO_FAST_PATH = ATTR_SKIP | ATTR_GUNALIGNED  # bdl_kernels.hpp kNoFastPath

SEGMENTS_B = [("l0.weight", 6000)]
SEGMENTS_C = [("l0.weight", 2000), ("head.weight", 1000)]


class Layout:
    """K chains of `segments`, chain k's element j at k * stride + j."""

    def __init__(self, segments, chains):
        from bayesdll_amd.flat import segment_attrs
        self.names = [nm for nm, _ in segments]
        self.numels = [int(k) for _, k in segments]
        self.offsets = np.concatenate([[0], np.cumsum(self.numels)[:-1]]).astype(int).tolist()
        self.K = int(chains)
        self.n1 = int(sum(self.numels))
        self.stride = (self.n1 + 3) // 4 * 4
        self.chain_groups = self.stride // 4
        self.n = self.K * self.stride
        self.attrs = segment_attrs(self.names, "head", "uninformative",
                                   [nm != FROZEN for nm in self.names])

    def stacked_segments(self):
        """(offset, numel, attr) of every (chain, tensor), in flat order."""
        return [(k * self.stride + o, n, a) for k in range(self.K)
                for o, n, a in zip(self.offsets, self.numels, self.attrs)]

    def flat_runs(self, lo=0, hi=None):
        """The run table of elements [lo, hi) (boundaries of stacked tensors),
        built as StackedState does in "flat" gradient mode: build_runs over
        the K x segments offsets; a chain's padding becomes a SKIP run."""
        from bayesdll_amd.flat import build_runs
        hi = self.n if hi is None else hi
        segs = [s for s in self.stacked_segments() if lo <= s[0] < hi]
        assert segs[0][0] == lo and segs[-1][0] + segs[-1][1] <= hi
        return build_runs([o - lo for o, _, _ in segs], [n for _, n, _ in segs],
                          [a for _, _, a in segs], hi - lo)

    def slot_attr(self):
        """One attribute per element of a chain's slot, padding (SKIP) included."""
        a = np.repeat(np.asarray(self.attrs, dtype=np.uint8), np.asarray(self.numels))
        return np.concatenate([a, np.full(self.stride - self.n1, ATTR_SKIP, dtype=np.uint8)])

    def seams(self):
        """The float4 group at which each chain but the first starts."""
        return [k * self.chain_groups for k in range(1, self.K)]


def table_a():
    return Layout(SEGMENTS, 3)


def table_b():
    return Layout(SEGMENTS_B, 5)


def table_c():
    return Layout(SEGMENTS_C, 6)


# ----------------------------------------------------------------- classifier
def block_iterations(n, depth, grid_cap, grid_stride):
    """(first group, end group) of every block iteration of a step launch
    over n elements at unroll `depth`, with at most grid_cap workgroups
    (launch_step in bdl_api.hip: workgroups per CU x CUs) in either sweep
    order (step_body: one contiguous span per block, or grid-stride)."""
    ngroups = (n + 3) // 4
    per_iter = K_BLOCK * depth
    iters = (ngroups + per_iter - 1) // per_iter
    grid = max(1, min(iters, grid_cap))
    out = []
    if grid_stride:
        for b in range(grid):
            for gb in range(b * per_iter, ngroups, grid * per_iter):
                out.append((gb, min(gb + per_iter, ngroups)))
    else:
        per_block = (iters + grid - 1) // grid
        grid = (iters + per_block - 1) // per_block
        span = per_block * per_iter
        for b in range(grid):
            g0, g1 = b * span, min((b + 1) * span, ngroups)
            for gb in range(g0, g1, per_iter):
                out.append((gb, min(gb + per_iter, g1)))
    return out


def classify(runs, n, gb, gend, depth):
    """The path of the block iteration over groups [gb, gend): "fast" (full,
    inside one run that allows the fast path), "multi" (full, multi_run_ok:
    every run it touches allows the fast path and every boundary inside it is
    a multiple of 4) or "slow".  runs: [(end, attr), ...] as build_runs
    returns them."""
    per_iter, nfull = K_BLOCK * depth, n // 4
    r = 0
    while r < len(runs) - 1 and runs[r][0] <= gb * 4:
        r += 1
    full = gend == gb + per_iter and gend <= nfull
    if full and runs[r][0] >= gend * 4 and not runs[r][1] & NO_FAST_PATH:
        return "fast"
    if full:
        for end, attr in runs[r:]:
            if attr & NO_FAST_PATH:
                break
            if end >= gend * 4:
                return "multi"
            if end & 3:
                break
    return "slow"


def classified(lay, depth, grid_cap, grid_stride, runs=None):
    """[(gb, gend, path)] of a whole launch over the layout's flat run table."""
    runs = [tuple(int(x) for x in r) for r in (lay.flat_runs() if runs is None else runs).tolist()]
    return [(gb, ge, classify(runs, lay.n, gb, ge, depth))
            for gb, ge in block_iterations(lay.n, depth, grid_cap, grid_stride)]
