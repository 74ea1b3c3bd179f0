"""Host reference of the per-tensor R-hat / ESS tables — TEST INFRASTRUCTURE ONLY.

Row t of a table is, by include/bdl_layers.h's contract, what bdl_chain_diag /
bdl_chain_ess would report if only tensor t's elements existed.  So the
reference of a row IS the existing whole-vector reference (chain_diag_ref.py /
chain_ess_ref.py, which the device equals bit for bit) applied to the
tensor's slice of every chain: counts, the extreme with the lowest index, a
math.fsum of the values, strict threshold counts — with the arg moved back to
the chain-local numbering.  `classify` restates the sweep's traversal
(bdl_layers.hip) in plain Python, so that the tables the GPU tests use can be
shown on the CPU to reach the code paths they claim.  Table L and the inputs
of both tests are defined here, once.  Nothing is imported from bayesdll_amd
and nothing from torch.
"""
from __future__ import annotations

import numpy as np

import chain_diag_ref as DR
import chain_ess_ref as ER

F = np.float32
K_BLOCK = 256      # float4 groups per block iteration (bdl_kernels.hpp kBlock, one group a lane)
UNROLL = 1         # groups per lane and block iteration of bdl_layers.hip's traversal
DEFAULT_GRID = 512  # two workgroups per CU on the MI355X's 256 CUs

DIAG_INT = ("n_eval", "n_degenerate", "n_nonfinite", "n_above", "argmax")
ESS_INT = ("n_eval", "n_degenerate", "n_nonfinite", "n_below", "argmin")


# ------------------------------------------------------------------ reference
def _row(summary, values, offset, arg, ext, total):
    """A whole-vector reference summary of one slice as a table row: the arg
    chain-local, and sum|x| over the evaluated values (for the fp64 bound)."""
    row = dict(summary)
    if row[arg] >= 0:
        row[arg] += int(offset)
    with np.errstate(invalid="ignore"):
        ev = np.isfinite(values)          # degenerate elements are written as NaN
    assert int(ev.sum()) == row["n_eval"]
    row["sum_abs"] = float(np.abs(values[ev].astype(np.float64)).sum())
    row["sum"], row["ext"] = row[total], row[ext]
    return row


def diag_layers_ref(mom1, mom2, segments, **kw):
    """[row] of bdl_chain_diag_layers: chain_diag_f32 on every tensor's slice."""
    rows = []
    for o, m in segments:
        _, _, rhat, s = DR.chain_diag_f32(np.asarray(mom1)[o:], np.asarray(mom2)[o:], n=int(m), **kw)
        rows.append(_row(s, rhat, o, "argmax", "rhat_max", "rhat_sum"))
    return rows


def ess_layers_ref(sM2, bM2, segments, **kw):
    """[row] of bdl_chain_ess_layers: chain_ess_f32 on every tensor's slice."""
    rows = []
    for o, m in segments:
        ess, _, s = ER.chain_ess_f32(np.asarray(sM2)[o:], np.asarray(bM2)[o:], n=int(m), **kw)
        rows.append(_row(s, ess, o, "argmin", "ess_min", "ess_sum"))
    return rows


# ----------------------------------------------------------------- traversal
def split(offset, numel):
    """(head, body groups, tail) of a tensor: the elements before the first
    16-B boundary of its slice, the float4 groups, the elements after the last."""
    h = min((4 - offset % 4) % 4, numel)
    nbody = (numel - h) // 4
    return h, nbody, numel - h - 4 * nbody


def rotated(w, i, grid):
    """Workgroup w's index b in segment i's rotation (bdl_chain_common.hpp
    rotated_block): b = 0 starts the segment and owns its head and tail."""
    return (w + grid - i % grid) % grid


def classify(segments, n, grid):
    """{(workgroup, segment): dict(part, iters, head, body, tail)} of one
    sweep: whether the workgroup takes part in the segment (else it stores an
    empty partial), its block iterations of the body, and the head / body /
    tail ELEMENTS it evaluates.  Restates bdl_layers_kernel: workgroup w is
    workgroup b = (w - i) mod grid of segment i's rotation; b takes the block
    iterations b, b + grid, ... of K_BLOCK groups; b = 0 also the head and the
    tail, and takes part even when the body is empty."""
    out = {}
    for i, (o, m) in enumerate(segments):
        assert m >= 1 and o >= 0 and o + m <= n
        h, nbody, tail = split(o, m)
        for w in range(grid):
            b = rotated(w, i, grid)
            starts = range(b * K_BLOCK, nbody, grid * K_BLOCK)
            part = b == 0 or b * K_BLOCK < nbody
            assert part or len(starts) == 0
            out[w, i] = dict(part=part, iters=len(starts),
                             head=h if b == 0 else 0, tail=tail if b == 0 else 0,
                             body=4 * sum(min(K_BLOCK, nbody - g) for g in starts))
    return out


# -------------------------------------------------------------------- tables
# Table L: the segment kinds of the traversal in 7,245 elements (stride 7,248)
SEGMENTS_L = [
    ("pre", 5),          # offset 0: no head, one group, a 1-element tail
    ("one", 1),          # offset 5 = 1 mod 4: all head
    ("two", 3),          # offset 6: a 2-element head and a 1-element tail, no body
    ("three", 3),        # offset 9 = 1 mod 4: all head, the longest one
    ("aligned", 1024),   # offset 12: 16-B aligned at both ends, exactly one block iteration
    ("odd", 7),          # offset 1036: one group and a 3-element tail
    ("hbt", 1000),       # offset 1043: head 1, 249 groups, tail 3; the planted NaNs
    ("big", 3301),       # offset 2043: head 1, 825 groups: grid 2 makes two trips in both workgroups
    ("frozen", 600),     # offset 5344: every chain bit-equal
    ("flat", 300),       # offset 5944: the constructed non-finite row
    ("last", 1001),      # offset 6244: ends at n = 7245 = 1 mod 4
]
ORDINARY_L = ("pre", "one", "two", "three", "aligned", "odd", "hbt", "big", "last")


class Table:
    def __init__(self, segments, frozen, flat=None):
        self.names = [nm for nm, _ in segments]
        self.numels = [int(k) for _, k in segments]
        self.offsets = np.concatenate([[0], np.cumsum(self.numels)[:-1]]).astype(int).tolist()
        self.n = int(sum(self.numels))
        self.chain_groups = (self.n + 3) // 4
        self.slot = 4 * self.chain_groups
        self.segments = list(zip(self.offsets, self.numels))
        self.frozen, self.flat = frozen, flat

    def span(self, name):
        i = self.names.index(name)
        return self.offsets[i], self.numels[i]


def table_l():
    return Table(SEGMENTS_L, "frozen", "flat")


def table_a():
    """Table A of tests/stacked_tables.py: the 39,426-element segment list of
    test_gpu_noise_units.py (stride 39,428, an odd boundary, a frozen tensor)."""
    from test_gpu_noise_units import FROZEN, SEGMENTS
    return Table(SEGMENTS, FROZEN)


SENTINEL = F(-7.75)   # a chain slot's padding: a finite value that would be counted if read
COUNT = 7             # samples per chain of the R-hat inputs
SAMPLES, BATCHES = 37, 9


def nan_spots(tab):
    """Chain-local indices of the NaNs planted in table L's `hbt`: its head
    element, a body element and its last tail element."""
    if "hbt" not in tab.names:
        return []
    o, m = tab.span("hbt")
    return [o, o + 501, o + m - 1]


def diag_inputs(tab, K, var_mode, ratio, seed=5):
    """(mom1, mom2) of K chains over the table: chain_diag_ref.make_case's
    elements (every one evaluated), the frozen tensor bit-equal in all chains
    (degenerate), the `flat` tensor with zero within-chain variance (with
    var_floor = 0: W = 0, rhat = Inf, non-finite), NaN in chain 1's mean at
    nan_spots, and SENTINEL in every slot's padding."""
    m1, var, cg = DR.make_case(seed, K, tab.n, chain_groups=tab.chain_groups, pad=SENTINEL)
    assert cg == tab.chain_groups
    if tab.flat:
        o, m = tab.span(tab.flat)
        for k in range(K):
            var[tab.slot * k + o: tab.slot * k + o + m] = 0.0
    m2 = DR.to_mode(m1, var, var_mode, ratio, K, tab.slot, tab.n)
    o, m = tab.span(tab.frozen)
    for k in range(1, K):
        m1[tab.slot * k + o: tab.slot * k + o + m] = m1[o: o + m]
    for e in nan_spots(tab):
        m1[tab.slot + e] = np.nan
    if var_mode == DR.VAR_RAW_MOMENTS and tab.flat:
        # zero variance in the raw-moment form: mom2 = mom1^2 exactly as the device squares it
        o, m = tab.span(tab.flat)
        for k in range(K):
            s = slice(tab.slot * k + o, tab.slot * k + o + m)
            m2[s] = m1[s] * m1[s]
    return m1, m2


def ess_inputs(tab, K, seed=9):
    """(sM2, bM2) of K chains over the table: positive accumulators (every
    element evaluated), the frozen tensor with bM2 = 0 in all chains
    (degenerate), the `flat` tensor with sM2 = Inf in the last chain
    (non-finite), NaN in chain min(1, K-1)'s bM2 at nan_spots, SENTINEL in the
    padding."""
    rng = np.random.default_rng(seed)
    sM2 = np.full(K * tab.slot, SENTINEL, F)
    bM2 = np.full(K * tab.slot, SENTINEL, F)
    for k in range(K):
        s = slice(tab.slot * k, tab.slot * k + tab.n)
        sM2[s] = rng.uniform(0.5, 2.0, tab.n) * 1e-3
        bM2[s] = rng.uniform(0.5, 2.0, tab.n) * 1e-5
        o, m = tab.span(tab.frozen)
        bM2[tab.slot * k + o: tab.slot * k + o + m] = 0.0
    if tab.flat:
        o, m = tab.span(tab.flat)
        sM2[tab.slot * (K - 1) + o: tab.slot * (K - 1) + o + m] = np.inf
    for e in nan_spots(tab):
        bM2[tab.slot * min(1, K - 1) + e] = np.nan
    return sM2, bM2
