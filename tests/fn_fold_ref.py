"""Host reference of bdl_fn_fold (include/bdl_fn.h) — TEST INFRASTRUCTURE ONLY:
the float64 softmax, the bound on |probs - softmax64| derived from the header's
arithmetic contract, the fold (chain_ess_ref.fold_f32, imported unmodified) of
given probabilities, a restatement of the kernel's geometry, and the builders
of the GPU cases.  Nothing is imported from bayesdll_amd and nothing from torch.

Bound derivation (as predict_ref's for one member row).  u = 2^-24 is fp32's
unit roundoff; "1 ulp" of expf, the documented maximum error of the HIP device
library, is a relative error of at most 2^-23 = 2u.  For a row with
d_c = x_c - m <= 0, e_c = exp(d_c), Z = sum_c e_c, p_c = e_c / Z and
S1 = sum_c p_c |d_c|:
  - m is exact.  fl(x - m) has relative error u, an absolute error u |d| in
    the exponent, so a relative error u |d| in e; expf adds 2u:
        rel(e_c) <= u (|d_c| + 2).
  - Z is an fp64 sum of the e_c (its own rounding, ~C 2^-53, is nothing next
    to u):  rel(Z) <= sum_c p_c rel(e_c) = u (S1 + 2).
  - p_c = e_c * (1/Z) in fp64 (two roundings of 2^-53):
        rel(p_c) <= u (|d_c| + 4 + S1).
  - the final rounding to fp32 adds u (a normal result):
        rel(probs_c) <= u (|d_c| + 5 + S1).
  - an e_c in the denormal range (|d| > ~87.3) is off by at most 1 ulp there,
    2^-149, absolutely; Z >= 1 (the maximum's e is exactly 1), so p_c inherits
    at most that, and its own rounding in the denormal range adds 2^-150:
    together below FLOOR = 2^-148.
The bound is p u (|d| + 5 + S1), multiplied by 1.001 for the second-order
terms, plus 2^-45 p for the fp64 operations, plus FLOOR.
"""
from __future__ import annotations

import functools

import numpy as np

import chain_ess_ref as E

F = np.float32
U = 2.0 ** -24
FLOOR = 2.0 ** -148
WAVE_CLASSES, MAX_CLASSES, BLOCK, WAVES = 256, 8192, 256, 4


def bad_rows(x):
    """[..., 1]-less mask of rows with a NaN, a +inf or no finite entry."""
    x = np.asarray(x, dtype=np.float64)
    return (np.isnan(x) | np.isposinf(x)).any(-1) | ~np.isfinite(x).any(-1)


def softmax64(x):
    """(p, bound): the float64 softmax of fp32 logits [..., C] (NaN in every
    class of a bad row, 0 at a -inf logit) and the bound on |probs - p|."""
    x = np.asarray(x, dtype=np.float64)
    bad = bad_rows(x)
    xs = np.where(bad[..., None], 0.0, x)
    m = xs.max(-1, keepdims=True)
    d = xs - m
    e = np.exp(d)
    p = e / e.sum(-1, keepdims=True)
    ad = np.where(np.isfinite(d), np.abs(d), 0.0)
    S1 = (p * ad).sum(-1, keepdims=True)
    b = p * U * (ad + 5 + S1) * 1.001 + 2.0 ** -45 * p + FLOOR
    nan = np.where(bad[..., None], np.nan, 0.0)
    return p + nan, b + nan


def stack(probs, chain_groups):
    """[K, P, C] probabilities as the stacked fp32 vector fold_f32 reads
    (chain k, element b*C + c at 4*chain_groups*k + b*C + c; padding 0)."""
    probs = np.asarray(probs, dtype=F)
    K, P, C = probs.shape
    slot = 4 * int(chain_groups)
    v = np.zeros(K * slot, F)
    for k in range(K):
        v[slot * k: slot * k + P * C] = probs[k].ravel()
    return v


def fold(acc, probs, s, b, *, chain_groups):
    """Fold sample s (1-based) of the probabilities [K, P, C] into `acc` in
    place by chain_ess_ref.fold_f32.  Returns the flags."""
    K, P, C = np.asarray(probs).shape
    return E.fold_f32(acc, stack(probs, chain_groups), s, b, chains=K, chain_groups=chain_groups,
                      n=P * C)


# ------------------------------------------------------------ the geometry
def default_grid(rows, classes, cus=256):
    rpb = WAVES if classes <= WAVE_CLASSES else 1
    return max(1, min((rows + rpb - 1) // rpb, min(4 * cus, 2048)))


def paths(chains, probe, classes, grid_blocks):
    """The set of branches of bdl_fn.hip a launch takes, restated from the
    kernel: which kernel (wave / block), which access form (vec / elem), and,
    over every (workgroup, trip, wave, thread), idle waves and lanes, second
    row trips, a thread's second class-group trip, fewer class groups than
    threads, and the partial last group of the element form.  Also returns how
    often every (row, class) is written: exactly once."""
    rows, C = chains * probe, classes
    Q = (C + 3) // 4
    wave = C <= WAVE_CLASSES
    grid = grid_blocks if grid_blocks > 0 else default_grid(rows, C)
    rpb = WAVES if wave else 1
    grid = max(1, min((rows + rpb - 1) // rpb, grid))
    got = {"wave" if wave else "block", "vec" if C % 4 == 0 else "elem"}
    writes = np.zeros((rows, C), np.int64)
    for blk in range(grid):
        if wave:
            for w in range(WAVES):
                r, trip = blk * WAVES + w, 0
                if r >= rows:
                    got.add("idle_wave")
                while r < rows:
                    if trip:
                        got.add("row_trip2")
                    if Q < 64:
                        got.add("idle_lane")
                    for lane in range(min(Q, 64)):
                        lo, hi = 4 * lane, min(4 * lane + 4, C)
                        if hi - lo < 4:
                            got.add("partial_group")
                        writes[r, lo:hi] += 1
                    r, trip = r + grid * WAVES, trip + 1
        else:
            r, trip = blk, 0
            while r < rows:
                if trip:
                    got.add("row_trip2")
                if Q % BLOCK:
                    got.add("idle_thread")   # fewer groups than threads in the last trip
                if Q < BLOCK:
                    got.add("fewer_groups_than_threads")
                for q in range(Q):
                    if q >= BLOCK:
                        got.add("thread_trip2")
                    lo, hi = 4 * q, min(4 * q + 4, C)
                    if hi - lo < 4:
                        got.add("partial_group")
                    writes[r, lo:hi] += 1
                r, trip = r + grid, trip + 1
    return got, writes


# ---------------------------------------------------------------- the cases
# (classes, probe, chains).  Wave path: 1 (p = 1 everywhere), 3 (one partial
# group), 10, 12 (vec, idle lanes), 256 (every lane busy).  Block path: 257 (one
# past the switch, element form), 260 (vec, fewer groups than threads), 1000
# (vec, fewer groups than threads), 1027 (element form, a thread's second trip,
# partial last group), 2052 (vec, a second and a third trip).  probe in
# {1, 5, 9}, chains in {1, 2, 3}.
CLASSES = (1, 3, 10, 12, 256, 257, 260, 1000, 1027, 2052)
CASES = [(1, 1, 1), (1, 9, 3), (3, 5, 2), (3, 9, 1), (10, 9, 3), (10, 1, 2), (12, 5, 3),
         (12, 1, 1), (256, 9, 2), (256, 5, 1), (257, 1, 2), (257, 5, 3), (260, 5, 1),
         (260, 9, 2), (1000, 9, 3), (1000, 1, 1), (1027, 5, 2), (1027, 9, 1), (2052, 5, 3),
         (2052, 1, 2)]
GRIDS = (1, 2, 0)
PAD_GROUPS = 3          # every chain slot is 12 elements wider than n
SENTINEL = -123.25
B_LONG, FOLDS = 3, 7    # seven folds at b = 3, then two at b = 1 (flags 15 and 6)


def case_id(c):
    return "C{}-P{}-K{}".format(*c)


def chain_groups_of(case):
    C, P, _ = case
    return (P * C + 3) // 4 + PAD_GROUPS


def make_logits(case, fold, special=False):
    """fp32 logits [K, P, C] ~ N(0, 2^2) of fold `fold` (0-based) of a case.
    special (P = 9, K >= 2, C > 1): row 3 has class C // 2 masked in EVERY fold
    and chain (p = 0 throughout: one degenerate element); in fold 1 row 1 of
    chain 0 is all-equal and row 2 a spread wide enough that e underflows to 0;
    in fold 2 row 5 of chain 0 holds a NaN, row 6 of chain 1 a +inf and row 7
    of chain 0 is all -inf (3 * C non-finite elements)."""
    C, P, K = case
    rng = np.random.default_rng([C, P, K, fold, int(special)])
    x = (2.0 * rng.standard_normal((K, P, C))).astype(F)
    if special:
        assert P == 9 and K >= 2 and C > 1
        x[:, 3, C // 2] = -np.inf
        if fold == 1:
            x[0, 1, :] = F(0.75)
            x[0, 2, :] = (rng.random(C) * 100.0).astype(F)
            x[0, 2, 0], x[0, 2, C - 1] = 230.0, 5.0      # exp(-225) is 0 in fp32
        if fold == 2:
            x[0, 5, C // 3] = np.nan
            x[1, 6, C - 1] = np.inf
            x[0, 7, :] = -np.inf
    return x


@functools.lru_cache(maxsize=None)
def built(case, special=False):
    """[(logits, softmax64, bound)] of the case's FOLDS + 2 folds, computed
    once and shared (treat as read-only)."""
    out = []
    for f in range(FOLDS + 2):
        x = make_logits(case, f, special)
        p, b = softmax64(x)
        for a in (x, p, b):
            a.setflags(write=False)
        out.append((x, p, b))
    return out


def new_acc(case):
    C, P, K = case
    return E.new_acc(K * 4 * chain_groups_of(case), SENTINEL)
