"""Host reference of bdl_diversity (include/bdl_diversity.h): the fp64
definitions by plain loops over the pairs and in a vectorised second form, a
NumPy emulation of the header's arithmetic contract, the error bound of every
tv_sum / kl_sum entry derived from that contract, the kernel's dispatch and
traversal restated as path labels, and table D of the GPU cases.

Bound derivation.  u = 2^-24 is fp32's unit roundoff; "1 ulp" of expf / logf
(the documented maximum error of the HIP device library) is a relative error
of at most 2u.  For one voter row with d_c = x_c - m <= 0, e_c = exp(d_c), Z =
sum e_c, p_c = e_c / Z, lp_c = d_c - log Z, S1 = sum_c p_c |d_c|:
  - fl(x - m) has relative error u, an absolute error u|d| in the exponent, so
    a relative error u|d| in e; expf adds 2u:   rel(e_c) <= u (|d_c| + 2).
  - Z is an fp64 sum of the e_c in some order (its own rounding, at most
    8192 x 2^-53, is nothing):   rel(Z) <= sum_c p_c rel(e_c) = u (S1 + 2).
  - p_c = fl32(e_c * (1/Z)), product and reciprocal in fp64:
        errp_c := err(p_c) <= p_c u (|d_c| + 5 + S1) + 2^-148
    (the floor: an e or a p that underflows is off by less than that).
  - log Z: rel(Z), the rounding of Z to fp32 and 1 ulp of logf:
    u (S1 + 2) + u + 2u log Z; lp_c adds d's u|d_c| and its own rounding u|lp_c|:
        errlp_c := err(lp_c) <= u (|d_c| + S1 + 3 + 2 log Z + |lp_c|).
  An example's contribution to tv_sum[i][j] is 0.5 sum_c |p_ic - p_jc|, every
  difference rounded once to fp32 (u |p_ic - p_jc|), summed in fp64:
        btv := 0.5 sum_c (errp_ic + errp_jc + u |p_ic - p_jc|)
  and to kl_sum[i][j] it is sum_c p_ic D_c, D_c = lp_ic - lp_jc rounded once
  (the product exact in fp64), over the classes not masked for i:
        bkl := sum_c (errp_ic |D_c| + p_ic (errlp_ic + errlp_jc + u |D_c|)).
  Both are multiplied by 1.001 for the second-order terms and get 2^-45 of the
  sum of the magnitudes for the fp64 sum over at most 8192 classes.  An entry
  of the totals is bounded by the sum of its examples' bounds plus (2 n + 8)
  2^-53 of the sum of the magnitudes: n terms added in any order over any
  number of workgroups and up to four accumulating calls.
Integers have no bound: the argmax is a raw fp32 comparison (only an exact tie
could differ, and the lowest index settles it), and masks are decided on d."""
import functools

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -148
HEADER = ("n", "n_labelled", "n_nonfinite")
INTS = ("disagree", "both_wrong", "kl_unbounded")
SUMS = ("tv_sum", "kl_sum")

# include/bdl_diversity.h
MAX_VOTERS, MAX_CLASSES, WAVE_VOTERS, TILE, LDS_STRIDE = 64, 8192, 16, 64, 68
MAX_GRID, DEFAULT_WORKSPACE, BLOCK = 1024, 32 << 20, 256


def nonfinite_examples(x):
    """[B]: any voter row with a NaN, a +inf or no finite entry."""
    rowbad = (np.isnan(x) | np.isposinf(x)).any(-1) | ~np.isfinite(x).any(-1)
    return rowbad.any(0)


def _labels(labels, B, C):
    lab = np.full(B, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    return lab, (lab >= 0) & (lab < C)


def _empty(P):
    t = {k: 0 for k in HEADER}
    t.update({k: np.zeros((P, P), dtype=np.int64) for k in INTS})
    t.update({k: np.zeros((P, P)) for k in SUMS})
    return t


def _softmax64(row):
    """(p, lp, masked) of one fp64 row; a -inf entry is masked."""
    m = row.max()
    d = row - m
    e = np.exp(d)
    Z = e.sum()
    with np.errstate(divide="ignore"):
        return e / Z, d - np.log(Z), np.isneginf(row)


def reference_loop(logits, labels=None):
    """The definitions in fp64, by plain loops over examples and ordered pairs."""
    x = np.asarray(logits, dtype=np.float64)
    P, B, C = x.shape
    lab, labelled = _labels(labels, B, C)
    bad = nonfinite_examples(x)
    t = _empty(P)
    for b in range(B):
        if bad[b]:
            t["n_nonfinite"] += 1
            continue
        t["n"] += 1
        t["n_labelled"] += int(labelled[b])
        rows = [_softmax64(x[i, b]) for i in range(P)]
        arg = [int(np.argmax(x[i, b])) for i in range(P)]  # the first maximum
        for i in range(P):
            pi, li, mi = rows[i]
            for j in range(P):
                pj, lj, mj = rows[j]
                t["disagree"][i, j] += int(arg[i] != arg[j])
                if labelled[b] and arg[i] != lab[b] and arg[j] != lab[b]:
                    t["both_wrong"][i, j] += 1
                if i == j:
                    continue
                t["tv_sum"][i, j] += 0.5 * np.abs(pi - pj).sum()
                if (mj & ~mi).any():
                    t["kl_unbounded"][i, j] += 1
                else:
                    on = ~mi
                    t["kl_sum"][i, j] += (pi[on] * (li[on] - lj[on])).sum()
    return t


def _example_terms(p, lp, masked):
    """[P, P] tv and kl contributions and the unbounded flags of one example
    from [P, C] arrays (any float type; the sums are taken in fp64)."""
    with np.errstate(invalid="ignore", over="ignore"):
        dp = np.abs(p[:, None, :] - p[None, :, :])
        tv = 0.5 * dp.astype(np.float64).sum(-1)
        dl = lp[:, None, :] - lp[None, :, :]
        on = ~masked[:, None, :] & ~masked[None, :, :]
        term = np.where(on, p[:, None, :].astype(np.float64) * np.where(on, dl, 0).astype(
            np.float64), 0.0)
        unb = (masked[None, :, :] & ~masked[:, None, :]).any(-1)
    return tv, term, unb


def reference(logits, labels=None, emulate=False, want_bound=False):
    """The totals, vectorised over pairs and classes.  emulate: the header's
    arithmetic contract step by step (np.exp / np.log on fp32 stand in for expf
    / logf: both are within their ulp bound of the true value, not bit-equal to
    the device's).  want_bound: also `bound`, {tv_sum, kl_sum: [P, P]}."""
    x = np.asarray(logits, dtype=np.float32 if emulate else np.float64)
    P, B, C = x.shape
    lab, labelled = _labels(labels, B, C)
    bad = nonfinite_examples(x.astype(np.float64))
    t = _empty(P)
    btv, bkl, mtv, mkl = (np.zeros((P, P)) for _ in range(4))
    eye = np.eye(P, dtype=bool)
    for b in range(B):
        if bad[b]:
            t["n_nonfinite"] += 1
            continue
        t["n"] += 1
        t["n_labelled"] += int(labelled[b])
        xb = x[:, b, :]
        arg = xb.argmax(-1)
        with np.errstate(divide="ignore", over="ignore"):
            m = xb.max(-1, keepdims=True)
            d = xb - m                      # fp32 under emulate: one rounding
            masked = np.isneginf(d)
            e = np.exp(d)
            Z = e.astype(np.float64).sum(-1, keepdims=True)
            if emulate:
                p = (e.astype(np.float64) * (1.0 / Z)).astype(np.float32)
                lp = d - np.log(Z.astype(np.float32))
            else:
                p, lp = e / Z, d - np.log(Z)
        tv, term, unb = _example_terms(p, lp, masked)
        kl = term.sum(-1)
        t["disagree"] += arg[:, None] != arg[None, :]
        if labelled[b]:
            w = arg != lab[b]
            t["both_wrong"] += w[:, None] & w[None, :]
        t["tv_sum"] += tv
        t["kl_unbounded"] += unb
        t["kl_sum"] += np.where(unb | eye, 0.0, kl)
        if want_bound:
            p64 = p.astype(np.float64)
            ad = np.where(masked, 0.0, np.abs(np.where(masked, 0.0, d)))
            S1 = (p64 * ad).sum(-1, keepdims=True)
            errp = np.where(masked, 0.0, p64 * U * (ad + 5 + S1) + FLOOR)
            alp = np.where(masked, 0.0, np.abs(np.where(masked, 0.0, lp)))
            errlp = U * (ad + S1 + 3 + 2 * np.log(Z) + alp)
            dp = np.abs(p64[:, None, :] - p64[None, :, :])
            btv += (0.5 * (errp[:, None, :] + errp[None, :, :] + U * dp).sum(-1) * 1.001
                    + 2.0 ** -45 * tv)
            on = ~masked[:, None, :] & ~masked[None, :, :]
            with np.errstate(invalid="ignore"):   # -inf - -inf where both are masked
                aD = np.where(on, np.abs(lp[:, None, :] - lp[None, :, :]), 0.0)
            bk = np.where(on, errp[:, None, :] * aD + p64[:, None, :] * (
                errlp[:, None, :] + errlp[None, :, :] + U * aD), 0.0).sum(-1)
            bk = bk * 1.001 + 2.0 ** -45 * np.abs(term).sum(-1)
            bkl += np.where(unb | eye, 0.0, bk)
            mtv += tv
            mkl += np.where(unb | eye, 0.0, np.abs(term).sum(-1))
    t["tv_sum"][eye] = 0.0
    if want_bound:
        f = (2 * t["n"] + 8) * 2.0 ** -53
        t["bound"] = {"tv_sum": np.where(eye, 0.0, btv + f * mtv),
                      "kl_sum": np.where(eye, 0.0, bkl + f * mkl)}
    return t


def concat(a, b):
    """The totals of two accumulated calls (bounds add)."""
    out = {k: a[k] + b[k] for k in HEADER + INTS + SUMS}
    if "bound" in a and "bound" in b:
        out["bound"] = {k: a["bound"][k] + b["bound"][k] for k in SUMS}
    return out


# ------------------------------------------------------------------ geometry
def wave_instance(P, C):
    return P <= WAVE_VOTERS and C <= TILE


def pairs_per_thread(P, C):
    npairs, team = P * (P - 1) // 2, 64 if wave_instance(P, C) else BLOCK
    for np_ in ((1, 2) if wave_instance(P, C) else (1, 2, 4, 8)):
        if npairs <= np_ * team:
            return np_
    raise ValueError((P, C))


def partial_bytes(P):
    return (32 + 40 * P * P + 15) // 16 * 16


def default_grid(P, B, C, cus=256):
    trips = -(-B // (4 if wave_instance(P, C) else 1))
    cap = max(1, min(DEFAULT_WORKSPACE // partial_bytes(P), MAX_GRID))
    return max(1, min(trips, 2 * cus, cap))


def pair_of(q, P):
    """The q-th pair i < j in row-major order (the kernel's ownership rule)."""
    i = 0
    while q >= P - 1 - i:
        q -= P - 1 - i
        i += 1
    return i, i + 1 + q


def path_labels(P, B, C, grid):
    """What a launch of the sweep does, restated from bdl_diversity.hip."""
    wave = wave_instance(P, C)
    ipb = 4 if wave else 1
    trips = -(-B // ipb)
    npairs = P * (P - 1) // 2
    team = 64 if wave else BLOCK
    lab = {"wave" if wave else "workgroup", f"np{pairs_per_thread(P, C)}",
           "vec" if C % 4 == 0 else "scalar"}
    lab.add("one-tile" if C <= TILE else "tiles")
    lab.add({TILE - 1: "tile-1", 0: "tile", 1: "tile+1"}.get(C % TILE, "tile-part"))
    if C == 1:
        lab.add("one-class")
    if npairs % team:
        lab.add("ragged-pairs")
    if npairs > team:
        lab.add("several-pairs-per-thread")
    if not wave and P <= WAVE_VOTERS:
        lab.add("edge-classes")     # few voters, but more classes than a tile
    if not wave and C <= TILE:
        lab.add("edge-voters")      # one tile, but more voters than a wave's team
    if grid > trips:
        lab.add("idle-workgroups")
    if trips > grid:
        lab.add("second-trip")
        if trips % grid:
            lab.add("uneven-trips")
    if wave and B % 4:
        lab.add("idle-waves")
    if not wave and P < 4:
        lab.add("idle-pass1-waves")
    return lab


# ------------------------------------------------------------------ the cases
# (P, B, C, seed, kind).  kind: "random" (N(0, 3^2) logits with the planted
# examples below), "identical" (every voter the same rows: exact zeros),
# "dyadic" (logits 0 on a support of 1, 2, 4 or 8 classes, -inf elsewhere: every
# p is a power of two and tv_sum is exact), "nolabels" (labels = None).
D = [
    (2, 1, 1, 1, "random"), (2, 13, 1, 2, "random"), (3, 5, 10, 3, "random"),
    (8, 37, 10, 4, "random"), (11, 13, 12, 5, "random"), (12, 13, 63, 6, "random"),
    (16, 14, 64, 7, "random"), (16, 13, 65, 8, "random"), (17, 13, 64, 9, "random"),
    (17, 13, 63, 10, "random"), (17, 13, 65, 11, "random"), (2, 13, 129, 12, "random"),
    (3, 13, 128, 13, "nolabels"), (20, 13, 1, 14, "random"), (23, 13, 10, 15, "random"),
    (24, 13, 37, 16, "random"), (33, 13, 10, 17, "random"), (46, 13, 12, 18, "random"),
    (64, 24, 200, 19, "random"), (8, 37, 10, 20, "identical"), (17, 13, 70, 21, "identical"),
    (8, 37, 10, 22, "dyadic"), (12, 13, 16, 23, "dyadic"), (20, 13, 72, 24, "dyadic"),
    (64, 13, 130, 25, "dyadic"), (4, 13, 1000, 26, "random"),
]
GRIDS = (1, 0, 5)  # 0: the default


def case_id(c):
    return "P{}-B{}-C{}-{}".format(c[0], c[1], c[2], c[4])


# planted examples (where B and C allow): index -> what
PLANT = {"offset": 1, "spread": 2, "same": 3, "tie": 4, "mask-one-way": 5, "mask-both-ways": 6,
         "nan": 7, "pinf": 8, "all-ninf": 9, "label-minus": 10, "label-C": 11}


def planted(P, B, C, kind):
    """The names of the constructed examples a case holds."""
    if kind in ("identical", "dyadic"):
        return set()
    have = set()
    if B >= 12:
        have |= {"offset", "same", "nan", "pinf", "all-ninf"}
        if kind != "nolabels":
            have |= {"label-minus", "label-C"}
        if C >= 2:
            have |= {"spread", "tie"}
        if C >= 3:
            have |= {"mask-one-way", "mask-both-ways"}
    return have


def make_case(P, B, C, seed, kind):
    rng = np.random.default_rng(7000 + seed)
    lab = rng.integers(0, C, size=B).astype(np.int64)
    if kind == "dyadic":
        x = np.full((P, B, C), -np.inf, dtype=np.float32)
        for i in range(P):
            for b in range(B):
                k = min(int(rng.choice([1, 2, 4, 8])), 1 << (C.bit_length() - 1))
                x[i, b, rng.choice(C, size=k, replace=False)] = 0.0
        return x, lab
    x = (3.0 * rng.standard_normal((P, B, C))).astype(np.float32)
    if kind == "identical":
        x[:] = x[0]
        return x, lab
    have = planted(P, B, C, kind)
    if "offset" in have:
        x[:, 1, :] += np.where(rng.random((P, 1)) < 0.5, -1e4, 1e4).astype(np.float32)
    if "spread" in have:
        x[:, 2, :] = (rng.random((P, C)) * 200.0).astype(np.float32)
        x[:, 2, 0] = 230.0
        x[:, 2, C - 1] = 5.0     # exp(-225) is 0 in fp32
        lab[2] = 0
    if "same" in have:
        x[:, 3, :] = x[0, 3, :]
    if "tie" in have:            # voter 0: two equal maxima, the lower index wins
        c1, c2 = 0, C - 1
        x[0, 4, :] = np.minimum(x[0, 4, :], 5.0)
        x[0, 4, c1] = x[0, 4, c2] = np.float32(9.5)
        x[1, 4, c2] = np.float32(40.0)   # voter 1 votes c2: it disagrees with voter 0
        lab[4] = c2
    if "mask-one-way" in have:
        x[0, 5, C // 2] = -np.inf
    if "mask-both-ways" in have:
        x[0, 6, 0] = -np.inf
        x[1, 6, C - 1] = -np.inf
    if "nan" in have:
        x[P // 2, 7, C // 3] = np.nan
    if "pinf" in have:
        x[0, 8, C - 1] = np.inf
    if "all-ninf" in have:
        x[P - 1, 9, :] = -np.inf
    if "label-minus" in have:
        lab[10], lab[11] = -1, C
    return x, (None if kind == "nolabels" else lab)


@functools.lru_cache(maxsize=None)
def built(case):
    """(logits, labels, reference with bounds) of a case, computed once and
    shared (treat as read-only)."""
    x, lab = make_case(*case)
    r = reference(x, lab, want_bound=True)
    x.setflags(write=False)
    if lab is not None:
        lab.setflags(write=False)
    return x, lab, r
