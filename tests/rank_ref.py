"""Host reference of bdl_rank (include/bdl_rank.h) in two independent forms —
a literal O(n^2) loop over the header's definitions and a sort / searchsorted
derivation — the table R of inputs every rank test runs, and a restatement of
the count kernel's launch geometry (which loads, tiles and exits a case
reaches).  NumPy only; the references of a case are computed once and shared."""
import functools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "bdl_rank.h")).read()
BLOCK = 256
U = int(re.search(r"#define BDL_RANK_U (\d+)", _HDR).group(1))
ITILE = BLOCK * U
JTILE = int(re.search(r"#define BDL_RANK_JTILE (\d+)", _HDR).group(1))
TPR = (19, 20)


# ------------------------------------------------------------- the two forms
def _valid(x, m):
    return ((m == 0) | (m == 1)) & ~np.isnan(x)


def _finish(x, m, ge_pos, ge_neg, gt_neg, need, tpr):
    ok = _valid(x, m)
    pos, neg = ok & (m == 1), ok & (m == 0)
    P, Nn = int(pos.sum()), int(neg.sum())
    u2 = sum(2 * Nn - int(a) - int(b) for a, b in zip(ge_neg[pos], gt_neg[pos]))
    if need is None:
        need = (P * tpr[0] + tpr[1] - 1) // tpr[1]
    cand = [int(g) for p, g in zip(ge_pos[ok], ge_neg[ok]) if P and int(p) >= need]
    ap = math.fsum(int(p) / (int(p) + int(g)) for p, g in zip(ge_pos[pos], ge_neg[pos]))
    return {"n_pos": P, "n_neg": Nn, "n_excluded": int((~ok).sum()), "u2": int(u2),
            "fp_at_tpr": min(cand) if cand else -1, "ap_sum": ap,
            "ge_pos": ge_pos, "ge_neg": ge_neg, "gt_neg": gt_neg}


def row_loop(x, m, need=None, tpr=TPR):
    """The header's definitions, literally: for every valid i, count the valid
    j of each mark with x_j >= x_i / x_j > x_i (fp32 comparisons: -0.0 == +0.0,
    the infinities ordered, subnormals as numbers)."""
    x, m = np.asarray(x, np.float32), np.asarray(m, np.int32)
    n = len(x)
    ok = _valid(x, m)
    pos, neg = ok & (m == 1), ok & (m == 0)
    ge_pos, ge_neg, gt_neg = (np.zeros(n, np.int64) for _ in range(3))
    with np.errstate(invalid="ignore"):
        for i in np.nonzero(ok)[0]:
            ge = x >= x[i]
            ge_pos[i] = np.count_nonzero(ge & pos)
            ge_neg[i] = np.count_nonzero(ge & neg)
            gt_neg[i] = np.count_nonzero((x > x[i]) & neg)
    return _finish(x, m, ge_pos, ge_neg, gt_neg, need, tpr)


def row_sorted(x, m, need=None, tpr=TPR):
    """The same numbers from each mark's sorted scores: #{x_j >= v} = len -
    searchsorted(left), #{x_j > v} = len - searchsorted(right)."""
    x, m = np.asarray(x, np.float32), np.asarray(m, np.int32)
    n = len(x)
    ok = _valid(x, m)
    sp, sn = np.sort(x[ok & (m == 1)]), np.sort(x[ok & (m == 0)])
    ge_pos, ge_neg, gt_neg = (np.zeros(n, np.int64) for _ in range(3))
    v = x[ok]
    ge_pos[ok] = len(sp) - np.searchsorted(sp, v, side="left")
    ge_neg[ok] = len(sn) - np.searchsorted(sn, v, side="left")
    gt_neg[ok] = len(sn) - np.searchsorted(sn, v, side="right")
    return _finish(x, m, ge_pos, ge_neg, gt_neg, need, tpr)


def mark_row(case, r):
    return 0 if case["marks"].shape[0] == 1 else r // case["spg"]


def reference(case, form=row_loop):
    """The reference of every row of a case (a list of dicts)."""
    return [form(case["scores"][r], case["marks"][mark_row(case, r)])
            for r in range(case["scores"].shape[0])]


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """row_loop's reference of table R's case `name`, computed once; read-only."""
    return reference(CASES[name])


def auroc(r):
    """kernels.rank_summary's expression."""
    P, Nn = r["n_pos"], r["n_neg"]
    return r["u2"] / (2 * P * Nn) if P and Nn else float("nan")


# ------------------------------------------------------------------ table R
SIZES = (1, 2, 255, 256, 257, ITILE, ITILE + 1, 3 * ITILE + 5)
SUB = np.float32(1e-45)  # the smallest subnormal


def _distinct(rng, n):
    return rng.permutation(n).astype(np.float32) - np.float32(n // 3)


def _patterns(rng, n):
    """{name: (scores [n] fp32, marks [n] int32)}: one row each."""
    rm = lambda: rng.integers(0, 2, n).astype(np.int32)  # noqa: E731
    out = {"distinct": (_distinct(rng, n), rm()),
           "all_tied": (np.full(n, 1.5, np.float32), rm())}
    # a tie block across every i-tile boundary and every LDS (j) tile boundary,
    # or across the middle of a short row
    x = _distinct(rng, n)
    cuts = sorted({c for c in list(range(ITILE, n, ITILE)) + list(range(JTILE, n, JTILE))}) \
        or [n // 2]
    for c in cuts:
        x[max(0, c - 9):min(n, c + 7)] = np.float32(0.25)
    out["tie_block"] = (x, rm())
    out["positives_only"] = (_distinct(rng, n), np.ones(n, np.int32))
    out["negatives_only"] = (_distinct(rng, n), np.zeros(n, np.int32))
    m = np.zeros(n, np.int32)
    m[0] = 1
    out["one_positive_first"] = (_distinct(rng, n), m)
    m = np.zeros(n, np.int32)
    m[-1] = 1
    out["one_positive_last"] = (_distinct(rng, n), m)
    out["excluded_marks"] = (_distinct(rng, n) % np.float32(7),
                             np.resize(np.array([0, 1, 2, -1, 1, 0], np.int32), n))
    x = _distinct(rng, n)
    x[::3] = np.nan
    out["nan_scores"] = (x, rm())
    m = rm()
    m[:ITILE] = 2  # a whole i-tile (a short row: everything) excluded
    out["excluded_tile"] = (_distinct(rng, n), m)
    x = _distinct(rng, n)
    x[::4], x[1::4] = np.inf, -np.inf
    out["infinities"] = (x, rm())
    x = np.resize(np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0], np.float32), n)
    out["signed_zeros"] = (x, np.resize(np.array([0, 1, 1, 0, 1, 0], np.int32), n))
    x = np.resize(np.array([SUB, 2 * SUB, SUB, 0.0, -SUB, 2 * SUB], np.float32), n)
    out["subnormals"] = (x, np.resize(np.array([1, 0, 0, 1, 1, 1, 0], np.int32), n))
    return out


def _build():
    cases = {}
    for n in SIZES:
        rng = np.random.default_rng(1000 + n)
        pats = _patterns(rng, n)
        cases[f"n{n}-patterns"] = {
            "scores": np.stack([v[0] for v in pats.values()]),
            "marks": np.stack([v[1] for v in pats.values()]), "spg": 1,
            "rows": list(pats)}
        # 5 scores per group: 3 groups with their own marks, 1 group, and 3 rows
        # under one shared mark row; ties, exclusions and NaNs mixed in
        x = rng.integers(-4, 5, (15, n)).astype(np.float32) / np.float32(4)
        x[rng.random((15, n)) < 0.05] = np.nan
        m = rng.integers(-1, 3, (3, n)).astype(np.int32)
        cases[f"n{n}-5x3-group-marks"] = {"scores": x, "marks": m, "spg": 5}
        cases[f"n{n}-5x1"] = {"scores": x[:5].copy(), "marks": m[:1].copy(), "spg": 5}
        cases[f"n{n}-1x3-shared-marks"] = {"scores": x[5:8].copy(), "marks": m[1:2].copy(),
                                           "spg": 1}
    return cases


CASES = _build()
CASE_IDS = list(CASES)


# ------------------------------------------- the count kernel's launch geometry
def count_paths(case):
    """What the count kernel does on a case, restated from bdl_rank.hip: grid
    (ceil(n / ITILE), rows); a workgroup's threads hold the examples tile + t +
    256 u; it leaves early when none is valid; else per j-tile thread t stages
    the group j0 + 4t .. + 3 — one 16-B load where both the score row and the
    mark row start 16-B aligned and the group is whole, element by element up
    to n otherwise, nothing past the row — and walks min(256, ceil(left / 4))
    groups.  Returns the set of paths reached."""
    x, marks = case["scores"], case["marks"]
    rows, n = x.shape
    seen = set()
    for r in range(rows):
        mr = mark_row(case, r)
        ok = _valid(x[r], marks[mr])
        aligned = (r * n) % 4 == 0 and (mr * n) % 4 == 0
        seen.add("row_aligned" if aligned else "row_unaligned")
        for it in range(-(-n // ITILE)):
            lo, hi = it * ITILE, min(n, (it + 1) * ITILE)
            seen.add("i_tile_full" if hi - lo == ITILE else "i_tile_partial")
            if not ok[lo:hi].any():
                seen.add("no_valid_i")
                continue
            for j0 in range(0, n, JTILE):
                left = n - j0
                seen.add("j_tile_full" if left >= JTILE else "j_tile_partial")
                for t in range(BLOCK):
                    e = j0 + 4 * t
                    if aligned and e + 4 <= n:
                        seen.add("load_16B")
                    elif e < n:
                        seen.add("guarded_tail" if aligned else "elementwise_unaligned")
                    else:
                        seen.add("group_past_row")
    return seen


ALL_PATHS = {"row_aligned", "row_unaligned", "i_tile_full", "i_tile_partial", "no_valid_i",
             "j_tile_full", "j_tile_partial", "load_16B", "guarded_tail",
             "elementwise_unaligned", "group_past_row"}
