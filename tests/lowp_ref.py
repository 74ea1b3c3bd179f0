"""bf16 helpers and the host reference of the bf16-gradient step — TEST
INFRASTRUCTURE ONLY (include/bdl_lowp.h states the contract).

bf16 values travel as uint16 bit patterns.  The encode is the header's integer
formula, the decode a 16-bit shift; the step reference upcasts the gradient,
calls tests/step_ref.py (the op-by-op fp32 restatement the fp32 kernels are
anchored to) and encodes the shadow of every element that is not skipped.
classify() restates the sweep of bdl_lowp.hip (lowp_body / lowp_iter: which
block iterations are full, and how a lane handles each float4 group) so that
tests/test_lowp_host.py can prove on the CPU which paths a table reaches;
TableD is the small table the instance tests run on.
Nothing is imported from bayesdll_amd and nothing from torch.
"""
from __future__ import annotations

import numpy as np

import step_ref as SR

F = np.float32


def bf16_encode(x):
    """fp32 -> bf16 bits, round to nearest, ties to even:
    (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the fp32 bits; a NaN gives a quiet
    NaN of its sign (the sum would carry into the sign bit)."""
    x = np.ascontiguousarray(x, dtype=F)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = ((u >> 16) | 0x40).astype(np.uint16)
    return np.where(np.isnan(x), nan, r).astype(np.uint16)


def bf16_decode(h):
    """bf16 bits -> fp32 (exact)."""
    h = np.ascontiguousarray(h, dtype=np.uint16)
    return (h.astype(np.uint32) << 16).view(F)


def bf16_is_nan(h):
    h = np.asarray(h, dtype=np.uint16)
    return ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)


def round_to_bf16(x):
    """fp32 values rounded to the nearest bf16, as fp32."""
    return bf16_decode(bf16_encode(x))


def step(method, th, g16, v, th0, attr, sc, eps, mode, *, momentum=None, collect=SR.NONE,
         m1=None, m2=None, shadow=None):
    """One bdl_lowp_step on the host.  method: "csghmc" | "sghmc" | "sgld";
    g16: the bf16 gradient bits; eps: the noise (None: no noise term; cSGHMC
    only); momentum: SGLD's None | "first" | "later".  Returns (theta, v, m1,
    m2, shadow): shadow is `shadow` with every element that is not skipped
    replaced by bf16(theta_new)."""
    g = bf16_decode(g16)
    if method == "csghmc":
        nth, nv = SR.csghmc(th, g, v, attr, sc, eps)
    elif method == "sghmc":
        nth, nv = SR.sghmc(th, th0, g, v, attr, sc, eps, mode)
    elif method == "sgld":
        nth, nv = SR.sgld(th, th0, g, v, attr, sc, eps, mode, momentum=momentum)
    else:
        raise ValueError(method)
    n1, n2 = SR.collect(collect, nth, m1, m2, sc, mode)
    sh = bf16_encode(nth)
    if shadow is not None:
        sh = np.where((attr & SR.ATTR_SKIP) != 0, np.asarray(shadow, dtype=np.uint16), sh)
    return nth, nv, n1, n2, sh


def rounding_inputs():
    """The fp32 values the rounding tests use: ties both ways, one fp32 ulp
    either side of a tie, +-0, +-inf, the fp32 maximum, subnormals (fp32
    subnormals that round to bf16 subnormals, to zero and up to the smallest
    normal), and 4096 random bit patterns with the NaNs removed."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0xC2F6, 0x0001, 0x0080, 0x7F7E, 0x8000, 0x0000):
        for lo in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF):
            bits.append((hi << 16) | lo)
    bits += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,
             0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF,
             0x807FFFFF, 0x007F8000, 0x00800000]
    rng = np.random.default_rng(20240)
    rnd = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([np.asarray(bits, dtype=np.uint32), rnd]).view(F)
    return x[~np.isnan(x)].copy()


# ----------------------------------------------------------------- the sweep
K_BLOCK = 256                      # bdl_kernels.hpp kBlock
K_NONE, K_VEC, K_ELEM = 0, 1, 2    # bdl_lowp.hip: how a lane handles a group
ATTR_GUNALIGNED = 0x8
NO_FAST_PATH = SR.ATTR_SKIP | ATTR_GUNALIGNED  # bdl_kernels.hpp kNoFastPath
# why a group is kElem (bits; several may hold for one group)
R_BOUNDARY = 1  # a run boundary inside the group (before the end of the vector)
R_SKIP = 2      # the group starts in a SKIP (or unaligned-gradient) run
R_BASE = 4      # the run's gradient base is not 8-B addressable
R_TAIL = 8      # the n % 4 tail: the group reaches past the end of the vector
LOWP_BPC = 2    # bdl_lowp.hip kLowpBpc: default workgroups per CU


class Iteration:
    """One block iteration: workgroup, its index within the workgroup, first
    group, full (unguarded, at the launch's depth) or the rolled guarded one,
    and kind / reason of its 256 * unroll groups (group gb + u * 256 + lane at
    index u * 256 + lane)."""

    def __init__(self, wg, index, gb, full, kind, reason):
        self.wg, self.index, self.gb, self.full = wg, index, gb, full
        self.kind, self.reason = kind, reason

    def has(self, kind, reason=0):
        m = self.kind == kind
        return bool((m & ((self.reason & reason) != 0)).any() if reason else m.any())


def run_table(offsets, numels, attrs, n, per_tensor=False):
    """(ends, attrs) of the run table.  Flat: bdl_build_runs (a gap and the
    rest up to n become SKIP runs, equal neighbours merge).  per_tensor: one
    run per tensor, as the base table needs (contiguous tensors only)."""
    ends, out = [], []
    pos = 0

    def push(end, a):
        nonlocal pos
        if end <= pos:
            return
        if out and out[-1] == a and not per_tensor:
            ends[-1] = end
        else:
            ends.append(end)
            out.append(a)
        pos = end

    for o, k, a in zip(offsets, numels, attrs):
        assert o >= pos and o + k <= n and (not per_tensor or o == pos)
        push(o, SR.ATTR_SKIP)
        push(o + k, a & 0xF)
    assert not per_tensor or pos == n
    push(n, SR.ATTR_SKIP)
    return np.asarray(ends, dtype=np.int64), np.asarray(out, dtype=np.int64)


def default_grid(n, unroll, cus):
    """The grid bdl_lowp_step takes for blocks = 0."""
    per_iter = K_BLOCK * unroll
    iters = ((n + 3) // 4 + per_iter - 1) // per_iter
    return max(1, min(iters, cus * LOWP_BPC))


def classify(offsets, numels, attrs, bases_mod8, n, grid, unroll):
    """Every block iteration of a bdl_lowp_step launch over n elements with
    `grid` workgroups at depth `unroll`, as a list of Iteration.  bases_mod8:
    None for the flat gradient (8-B aligned, one base), else run t's
    grad_base[t] mod 8 for the per-tensor run table (0 for SKIP runs)."""
    per_tensor = bases_mod8 is not None
    ends, rattr = run_table(offsets, numels, attrs, n, per_tensor)
    phase = np.asarray(bases_mod8, dtype=np.int64) if per_tensor else np.zeros(len(ends), np.int64)
    assert len(phase) == len(ends)
    last = len(ends) - 1
    ngroups, nfull = (n + 3) // 4, n // 4
    k_iter = K_BLOCK * unroll
    out = []
    for wg in range(grid):
        for index, gb in enumerate(range(wg * k_iter, ngroups, grid * k_iter)):
            full = gb + k_iter <= nfull
            gi = gb + np.arange(k_iter, dtype=np.int64)
            e = gi * 4
            live = gi < ngroups                    # GUARD && gi >= ngroups: kNone
            rr = np.minimum(np.searchsorted(ends, e, side="right"), last)
            whole = e + 4 <= n
            inside = ends[rr] >= e + 4
            slow_attr = (rattr[rr] & NO_FAST_PATH) != 0
            odd_base = phase[rr] != 0
            vec = whole & inside & ~slow_attr & ~odd_base
            kind = np.where(live, np.where(vec, K_VEC, K_ELEM), K_NONE).astype(np.int8)
            reason = (np.where(ends[rr] < np.minimum(e + 4, n), R_BOUNDARY, 0)
                      | np.where(slow_attr, R_SKIP, 0) | np.where(odd_base, R_BASE, 0)
                      | np.where(~whole, R_TAIL, 0))
            reason = np.where(kind == K_ELEM, reason, 0).astype(np.int8)
            assert not full or live.all()
            assert ((kind != K_ELEM) | (reason != 0)).all()
            out.append(Iteration(wg, index, gb, full, kind, reason))
    return out


def waves_in_two_chains(it, chain_groups):
    """The 64-lane waves (of any unroll step) of an iteration whose live groups
    belong to two stacked chains."""
    g = it.gb + np.arange(it.kind.size, dtype=np.int64)
    k = np.where(it.kind != K_NONE, g // chain_groups, -1).reshape(-1, 64)
    return [w for w in range(k.shape[0])
            if len(set(k[w][k[w] >= 0].tolist())) > 1]


def _attrs_of(names, frozen):
    return [(SR.ATTR_HEAD if "head" in nm else 0) | (0 if "bias" in nm else SR.ATTR_PRIOR)
            | (SR.ATTR_SKIP if nm in frozen else 0) for nm in names]


class TableD:
    """13,530 elements (n % 4 = 2) for the instance tests: inside elements
    [2048, 3072) — one depth-1 iteration, inside the first iteration at depths
    2 and 4 — lie vector groups, two run boundaries that are no multiples of 4,
    a frozen tensor and a tensor whose gradient base is 2 B off; a 6,000-element
    tensor carries the cursor through whole iterations; a tensor at an odd
    offset whose base is 8-B addressable; and the last 218 elements, the guarded
    iteration at every depth, hold vector groups, an odd boundary, a frozen
    tensor and the tail.  PHASES: each tensor's grad_base mod 8 in base-table
    mode — all four 2-B phases occur, on tensors in the middle of the table."""
    SEGMENTS = [
        ("l0.weight", 2100), ("l0.bias", 50), ("l1.weight", 300),
        ("l1.bias", 30),        # frozen
        ("l2.weight", 600), ("l2.bias", 20), ("l3.weight", 6000), ("l3.bias", 63),
        ("l4.weight", 2048), ("l4.bias", 9), ("head.weight", 2200), ("head.bias", 11),
        ("l5.weight", 69),      # frozen
        ("l5.bias", 30),
    ]
    FROZEN = ("l1.bias", "l5.weight")
    PHASES = [0, 0, 2, 0, 0, 4, 0, 6, 0, 2, 0, 0, 0, 0]
    BLOCKS = 2  # the literal grid of the instance tests: several iterations per workgroup

    names = [nm for nm, _ in SEGMENTS]
    numels = [k for _, k in SEGMENTS]
    offsets = np.concatenate([[0], np.cumsum(numels)[:-1]]).astype(int).tolist()
    n = int(sum(numels))
    # bayesdll_amd.flat.segment_attrs(names, "head", "uninformative", ...) restated
    attrs = _attrs_of(names, FROZEN)
    # where the adversarial values go (tests/test_lowp_host.py proves the kinds):
    # vector groups and element-wise groups of full iterations (the latter in
    # both gradient modes: groups with a run boundary inside), groups that are
    # element-wise in base-table mode (a base 2 B off), and vector and
    # element-wise groups (odd boundary, tail) of the guarded iteration
    SITE_VEC = list(range(4000, 4016))
    SITE_ELEM = [2148, 2149, 2150, 2151, 9160, 9161, 9162, 9163, 11208, 11209, 11210, 11211]
    SITE_ELEM_BASES = list(range(2200, 2216))
    SITE_GUARDED_VEC = list(range(13320, 13336))
    SITE_GUARDED_ELEM = [13428, 13429, 13430, 13528, 13529]


STACKED_BLOCKS = 2  # the literal grid of the stacked tests on tables B and C
UNROLLS = (1, 2, 4)
# (method, noise, collect, SGLD momentum): every built instance (pick_lowp /
# lowp_collect in bdl_lowp.hip), SGLD in its three momentum forms
INSTANCE_CASES = [("csghmc", nz, c, None) for nz in ("none", "buffer", "philox")
                  for c in ("NONE", "WELFORD_INIT", "WELFORD")]
INSTANCE_CASES += [("sgld", nz, c, m) for nz in ("buffer", "philox")
                   for c in ("NONE", "MEAN_INIT", "MEAN") for m in (None, "first", "later")]
INSTANCE_CASES += [("sghmc", nz, c, None) for nz in ("buffer", "philox")
                   for c in ("NONE", "MEAN_INIT", "MEAN")]
