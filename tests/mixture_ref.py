"""Host reference of bdl_member_score and bdl_mixture (include/bdl_mixture.h):
the fp64 definitions, a NumPy emulation of the header's arithmetic contracts,
the error bound of every output derived from those contracts, and the input
builders of the GPU cases.

Bound derivation (as tests/predict_ref.py; u = 2^-24, "1 ulp" of expf / logf is
a relative error of at most 2^-23 = 2u).  For one row with d_c = x_c - m <= 0,
e_c = exp(d_c), Z = sum e_c, p_c = e_c / Z, S1 = sum_c p_c |d_c|,
S2 = sum_c p_c d_c^2:
  rel(e_c) <= u (|d_c| + 2)      (fl(x - m): u |d| in the exponent; expf: 2u)
  rel(Z)   <= u (S1 + 2)         (an fp64 sum; its own rounding is nothing)
  rel(p_c) <= u (|d_c| + 4 + S1) (p_c = e_c * (1/Z) in fp64)
  an e_c that underflows is off by at most FLOOR = 2^-148 absolutely.

member_score.  lse = fl(m + logf(fl32(Z))): the logarithm carries rel(Z), the
rounding of Z to fp32 and 1 ulp of its result, u (S1 + 3) + 2u |log Z|; the
sum's rounding u |lse|; nll = fl(lse - x[label]) another u |nll|:
    b_row = u (S1 + 3) + 2u |log Z| + u |lse| + u |nll|.
nll_sum adds the fp32 values in fp64: the rows' bounds plus the summation's
(2 n + 4) 2^-53 of the sum of the magnitudes (n terms in any order over up to
four calls, as predict_ref derives it).  A masked class at the label gives
nll = +inf exactly (no bound needed: inf == inf).

mixture.  eps(pbar_c) = mean_s p u (|d| + 4 + S1) (the draws' fp64 mean).
  arithmetic:  mix = sum_c w_c pbar_c;  eps = sum_c w_c eps(pbar_c) + u mix
    (the rounding to fp32) + FLOOR;  logp = logf(pbar32): the relative error
    r = eps / mix moves the logarithm by at most -log(1 - r), plus 1 ulp of
    the result, 2u |logp|.  UNDEFINED (inf) where mix = 0 (logp = -inf, which
    the kernel must return exactly) or mix < 2^-126 (pbar32 may be denormal or
    0).
  reference:  l_c = logf(fl32(pbar_c)) with r_c = (eps(pbar_c) + u pbar_c +
    FLOOR) / pbar_c:  b(l_c) = -log(1 - r_c) + 2u |l_c|;  t = sum_c w_c l_c in
    fp64: b(t) = sum_c w_c b(l_c) + 2^-45 sum_c w_c |l_c|;  logsumexp is
    1-Lipschitz in the maximum norm, so logp = t - lse(t) is off by at most
    b(t) + max_k b(t_k) (over the classes with a finite t), plus the fp64 exp /
    log (2^-40 covers them) and the rounding to fp32, u |logp|.  UNDEFINED
    where t = -inf (logp = -inf exactly), and for EVERY class of an example in
    which a weighted component has 0 < pbar_c < 2^-126 at some class (its l_c
    has no bound and enters every class through the logsumexp).
  expected_entropy = sum_c w_c mean_s H_i with b(H_i) = u [(S1 + 3) + 2 log Z
    + S2 + 3 S1 + S1 (S1 + 2)] (predict_ref), plus u |expected_entropy| for the
    per-example output's rounding.
Every bound is multiplied by 1.001 for the second-order terms and gets 2^-40
for the fp64 sums.  Integer outputs are exact provided no member row's maximum
is attained twice except where the builder plants it (tests/test_mixture_host.py
asserts that)."""
import functools

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -148
NORMAL = 2.0 ** -126       # below: no bound on a logarithm of the value
MIN_WEIGHT = 1e-10
MAX_EXCLUDED = 0.01        # the share of a case's logp entries without a bound


def nonfinite_rows(x):
    """[...]: a row with a NaN, a +inf or no finite entry."""
    return (np.isnan(x) | np.isposinf(x)).any(-1) | ~np.isfinite(x).any(-1)


def _rows(x64):
    """Per row of finite-ised logits: m, d, Z, p, |d| where p > 0, S1, S2."""
    m = x64.max(-1, keepdims=True)
    d = x64 - m
    e = np.exp(d)
    Z = e.sum(-1, keepdims=True)
    p = e / Z
    ad = np.where(p > 0, np.abs(np.where(np.isfinite(d), d, 0.0)), 0.0)
    return m[..., 0], d, Z[..., 0], p, ad, (p * ad).sum(-1), (p * ad * ad).sum(-1)


def _labels(lab, C):
    lab = np.asarray(lab, dtype=np.int64)
    inr = (lab >= 0) & (lab < C)
    return lab, inr, np.where(inr, lab, 0)


# ------------------------------------------------------------- member_score
def score_reference(logits, labels):
    """The definitions in fp64.  logits [M, G, B, C] (fp32 values), labels [B].
    Returns n, n_nonfinite, n_wrong ([M, G] int64), nll_sum and its bound
    `b_nll_sum` ([M, G]), and the per-row nll / b_row / ok ([M, G, B])."""
    x = np.asarray(logits, dtype=np.float64)
    M, G, B, C = x.shape
    lab, inr, safe = _labels(labels, C)
    bad = nonfinite_rows(x)
    xs = np.where(bad[..., None], 0.0, x)
    m, d, Z, p, ad, S1, _ = _rows(xs)
    lse = m + np.log(Z)
    xl = np.take_along_axis(xs, np.broadcast_to(safe[None, None, :, None], (M, G, B, 1)), -1)[..., 0]
    nll = lse - xl
    ok = inr[None, None, :] & ~bad
    am = xs.argmax(-1)
    fin = ok & np.isfinite(nll)
    nllf = np.where(fin, nll, 0.0)
    b_row = np.where(fin, (U * (S1 + 3) + 2 * U * np.abs(np.log(Z)) + U * np.abs(lse)
                           + U * np.abs(nllf)) * 1.001 + 2.0 ** -40, 0.0)
    n = ok.sum(-1)
    return {"n": n.astype(np.int64),
            "n_nonfinite": (inr[None, None, :] & bad).sum(-1).astype(np.int64),
            "n_wrong": (ok & (am != lab[None, None, :])).sum(-1).astype(np.int64),
            "nll_sum": np.where(ok, nll, 0.0).sum(-1),
            "b_nll_sum": b_row.sum(-1) + (2 * n + 4) * 2.0 ** -53 * np.abs(nllf).sum(-1),
            "nll": nll, "b_row": b_row, "ok": ok}


def score_emulate(logits, labels):
    """The header's contract step by step (np.exp / np.log on fp32 stand in for
    expf / logf).  Returns the four fields as [M, G] arrays."""
    x = np.asarray(logits, dtype=np.float32)
    M, G, B, C = x.shape
    lab, inr, safe = _labels(labels, C)
    bad = nonfinite_rows(x.astype(np.float64))
    xs = np.where(bad[..., None], np.float32(0), x)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = xs.max(-1, keepdims=True)
        d = (xs - m).astype(np.float32)
        e = np.exp(d).astype(np.float32)
        Z = e.astype(np.float64).sum(-1)
        lse = (m[..., 0] + np.log(Z.astype(np.float32)).astype(np.float32)).astype(np.float32)
        xl = np.take_along_axis(xs, np.broadcast_to(safe[None, None, :, None], (M, G, B, 1)),
                                -1)[..., 0]
        nll = (lse - xl).astype(np.float32)
    ok = inr[None, None, :] & ~bad
    return {"n": ok.sum(-1), "n_nonfinite": (inr[None, None, :] & bad).sum(-1),
            "n_wrong": (ok & (xs.argmax(-1) != lab[None, None, :])).sum(-1),
            "nll_sum": np.where(ok, nll.astype(np.float64), 0.0).sum(-1)}


def check_scores(got, r, what, scale=1):
    """got: a structured / mapping [M, G] result with the struct's fields;
    `scale`: how many times the case was accumulated."""
    for k in ("n", "n_nonfinite", "n_wrong"):
        assert np.array_equal(np.asarray(got[k]), scale * r[k]), (what, k)
    g, w = np.asarray(got["nll_sum"], dtype=np.float64), scale * r["nll_sum"]
    inf = np.isinf(w)
    assert np.array_equal(g[inf], w[inf]), (what, "infinite nll_sum")
    err = np.abs(g[~inf] - w[~inf])
    assert (err <= scale * r["b_nll_sum"][~inf]).all(), (what, "nll_sum", float(err.max()))


# ------------------------------------------------------------------ mixture
def _logsumexp(t):
    mx = t.max(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(np.isfinite(mx), np.exp(t - np.where(np.isfinite(mx), mx, 0.0)), 0.0).sum(
            -1, keepdims=True)
        return np.where(np.isfinite(mx), mx + np.log(s), -np.inf)


def mixture_reference(logits, weights, draws, combine):
    """The definitions in fp64 with the bounds.  logits [comps*draws, G, B, C]
    (fp32 values), weights [comps, G] float64.  Returns logp [G, B, C] / b_logp
    (inf: undefined), expected_entropy [G, B] / b_expected_entropy, nonfinite
    [G, B], totals (a list per group) / b_totals."""
    x = np.asarray(logits, dtype=np.float64)
    M, G, B, C = x.shape
    D = int(draws)
    comps = M // D
    w = np.asarray(weights, dtype=np.float64)
    active = w >= MIN_WEIGHT                                   # [comps, G]
    wa = np.where(active, w, 0.0)
    rowbad = nonfinite_rows(x)                                  # [M, G, B]
    bad = (rowbad & np.repeat(active, D, axis=0)[:, :, None]).any(0)
    xs = np.where(rowbad[..., None], 0.0, x)
    m, d, Z, p, ad, S1, S2 = _rows(xs)
    H = np.log(Z) + (p * ad).sum(-1)
    bH = U * ((S1 + 3) + 2 * np.log(Z) + S2 + 3 * S1 + S1 * (S1 + 2))
    epsm = p * U * (ad + 4 + S1[..., None])
    per = lambda v: v.reshape((comps, D) + v.shape[1:]).mean(1)   # noqa: E731
    pc, epsc, Hc, bHc = per(p), per(epsm), per(H), per(bH)
    wb = wa[:, :, None]
    ee = (wb * Hc).sum(0)
    b_ee = ((wb * bHc).sum(0) + U * np.abs(ee)) * 1.001 + 2.0 ** -40
    with np.errstate(divide="ignore", invalid="ignore"):
        if combine == "arithmetic":
            mix = (wb[..., None] * pc).sum(0)
            eps = ((wb[..., None] * epsc).sum(0) + U * mix + FLOOR) * 1.001 + 2.0 ** -45 * mix
            logp = np.log(mix)
            rel = eps / mix
            b = np.where(mix >= NORMAL, -np.log1p(-np.minimum(rel, 0.5)) * 1.001
                         + 2 * U * np.abs(logp) + 2.0 ** -40, np.inf)
        else:
            act = active[:, :, None, None]
            lc = np.log(pc)
            rc = (epsc + U * pc + FLOOR) / pc
            blc = -np.log1p(-np.minimum(rc, 0.5)) * 1.001 + 2 * U * np.abs(lc)
            t = np.where(act, wb[..., None] * np.where(act, lc, 0.0), 0.0).sum(0)
            fin = np.isfinite(t)
            term = np.where(act & np.isfinite(lc), wb[..., None] * (blc + 2.0 ** -45 * np.abs(lc)),
                            0.0)
            bt = term.sum(0)
            logp = t - _logsumexp(t)
            btmax = np.where(fin, bt, 0.0).max(-1, keepdims=True)
            b = np.where(fin, (bt + btmax + U * np.abs(np.where(fin, logp, 0.0))) * 1.001
                         + 2.0 ** -40, np.inf)
            sub = (act & (pc > 0) & (pc < NORMAL)).any(0).any(-1)   # [G, B]
            b = np.where(sub[..., None], np.inf, b)
    logp = np.where(bad[..., None], np.nan, logp)
    b = np.where(bad[..., None], 0.0, b)
    ee_out = np.where(bad, np.nan, ee)
    tots, btots = [], []
    for g in range(G):
        ok = ~bad[g]
        n = int(ok.sum())
        tots.append({"n": n, "n_nonfinite": int(bad[g].sum()),
                     "expected_entropy_sum": float(ee[g][ok].sum())})
        btots.append(float(b_ee[g][ok].sum() + (2 * n + 4) * 2.0 ** -53 * np.abs(ee[g][ok]).sum()))
    return {"logp": logp, "b_logp": b, "expected_entropy": ee_out, "b_expected_entropy": b_ee,
            "nonfinite": bad, "totals": tots, "b_totals": btots}


def mixture_emulate(logits, weights, draws, combine):
    """The header's contract step by step in NumPy.  Returns logp [G, B, C]
    fp32, expected_entropy [G, B] fp32, totals."""
    x = np.asarray(logits, dtype=np.float32)
    M, G, B, C = x.shape
    D = int(draws)
    comps = M // D
    w = np.asarray(weights, dtype=np.float64)
    active = w >= MIN_WEIGHT
    rowbad = nonfinite_rows(x.astype(np.float64))
    bad = (rowbad & np.repeat(active, D, axis=0)[:, :, None]).any(0)
    xs = np.where(rowbad[..., None], np.float32(0), x)
    mix = np.zeros((G, B, C))
    hmix = np.zeros((G, B))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for c in range(comps):
            acc, hsum = np.zeros((G, B, C)), np.zeros((G, B))
            for s in range(D):
                r = xs[c * D + s]
                m = r.max(-1, keepdims=True)
                d = (r - m).astype(np.float32)
                e = np.exp(d).astype(np.float32)
                e64, d64 = e.astype(np.float64), d.astype(np.float64)
                Z = e64.sum(-1)
                T = np.where(e != 0, e64 * np.where(e != 0, d64, 0.0), 0.0).sum(-1)
                rz = 1.0 / Z
                hsum += np.log(Z.astype(np.float32)).astype(np.float64) - T * rz
                acc += e64 * rz[..., None]
            pb = acc / float(D)
            a = active[c][:, None]
            wc = w[c][:, None]
            if combine == "arithmetic":
                mix += np.where(a[..., None], wc[..., None] * pb, 0.0)
            else:
                l32 = np.log(pb.astype(np.float32)).astype(np.float32).astype(np.float64)
                mix += np.where(a[..., None], wc[..., None] * np.where(a[..., None], l32, 0.0), 0.0)
            hmix += np.where(a, wc * (hsum / float(D)), 0.0)
        if combine == "arithmetic":
            lp = np.log(mix.astype(np.float32)).astype(np.float32)
        else:
            lp = (mix - _logsumexp(mix)).astype(np.float32)
    lp = np.where(bad[..., None], np.float32("nan"), lp)
    ee = np.where(bad, np.float32("nan"), hmix.astype(np.float32))
    tots = [{"n": int((~bad[g]).sum()), "n_nonfinite": int(bad[g].sum()),
             "expected_entropy_sum": float(hmix[g][~bad[g]].sum())} for g in range(G)]
    return {"logp": lp, "expected_entropy": ee, "totals": tots}


def excluded_share(r):
    """The share of a case's logp entries of finite examples without a bound."""
    ok = np.broadcast_to(~r["nonfinite"][..., None], r["logp"].shape)
    return float((ok & ~np.isfinite(r["b_logp"])).sum()) / max(int(ok.sum()), 1)


def unchecked_share(r):
    """The share of a case's logp entries of finite examples that check_mixture
    compares with nothing: without a bound and not -inf in the reference (an
    entry whose reference is -inf is compared exactly)."""
    ok = np.broadcast_to(~r["nonfinite"][..., None], r["logp"].shape)
    checked = np.isfinite(r["b_logp"]) | np.isneginf(r["logp"])
    return float((ok & ~checked).sum()) / max(int(ok.sum()), 1)


def check_mixture(got, r, what, scale=1):
    """Per-example outputs (those present in `got`) and, with got["totals"],
    the totals against the reference within the bound; integers exact; an
    entry without a bound must still agree where the reference is -inf."""
    bad = r["nonfinite"]
    if "logp" in got:
        g, w, b = np.asarray(got["logp"], dtype=np.float64), r["logp"], r["b_logp"]
        assert np.array_equal(np.isnan(g), np.broadcast_to(bad[..., None], g.shape)), what
        sel = ~np.isnan(w) & np.isfinite(b)
        err = np.abs(g[sel] - w[sel])
        assert (err <= b[sel]).all(), (what, "logp", float((err - b[sel]).max()))
        ninf = ~np.isnan(w) & np.isneginf(w)
        assert np.isneginf(g[ninf]).all(), (what, "logp = -inf")
    if "expected_entropy" in got:
        g, w = np.asarray(got["expected_entropy"], dtype=np.float64), r["expected_entropy"]
        assert np.array_equal(np.isnan(g), bad), what
        err = np.abs(g[~bad] - w[~bad])
        assert (err <= r["b_expected_entropy"][~bad]).all(), (what, "expected_entropy")
    if "totals" in got:
        for gi, (t, bt) in enumerate(zip(r["totals"], r["b_totals"])):
            row = got["totals"][gi]
            assert int(row["n"]) == scale * t["n"], (what, gi, "n")
            assert int(row["n_nonfinite"]) == scale * t["n_nonfinite"], (what, gi, "n_nonfinite")
            err = abs(float(row["expected_entropy_sum"]) - scale * t["expected_entropy_sum"])
            assert err <= scale * bt, (what, gi, "expected_entropy_sum", err, bt)


# ------------------------------------------------------------------ the cases
# (classes, batch, components, draws, groups, seed).  classes: scalar and 16-B
# paths, both sides of the wave / workgroup boundary (256 | 257), one trip of
# the workgroup instance (1000, 1001), two (2048, 1030), four (4096, 4093: the
# limit and the element-loaded instance below it); batch 1, 5, 9; components x
# draws 1 x 1, 3 x 2, 2 x 1; groups 1, 3.  Every case is under 10^6 logits.
CASES = [
    (1, 1, 1, 1, 1, 1), (1, 5, 3, 2, 3, 2), (3, 5, 3, 2, 3, 3), (3, 9, 2, 1, 1, 4),
    (10, 9, 3, 2, 3, 5), (10, 5, 1, 1, 1, 6), (10, 1, 2, 1, 3, 7), (256, 9, 3, 2, 1, 8),
    (256, 5, 2, 1, 3, 9), (257, 9, 3, 2, 3, 10), (257, 5, 1, 1, 1, 11), (1000, 9, 3, 2, 3, 12),
    (1000, 5, 2, 1, 1, 13), (1001, 9, 2, 1, 3, 14), (1001, 5, 3, 2, 1, 15),
    (4096, 9, 3, 2, 3, 16), (4096, 5, 1, 1, 1, 17), (4096, 1, 2, 1, 1, 18),
    (2048, 5, 2, 1, 1, 19), (1030, 5, 3, 2, 1, 20), (4093, 5, 2, 1, 3, 21),
]
COMBINES = ("arithmetic", "reference")


def case_id(c):
    return "C{}-B{}-{}x{}-G{}".format(*c[:5])


def make_case(C, B, comps, D, G, seed):
    """logits [comps*D, G, B, C] ~ N(0, 3^2), labels [B] and weights [comps, G]
    (positive, every group's summing to 1; with three components the middle
    one of the last group is 0: skipped), with the planted examples (of every
    group).  B >= 5: 1 rows offset by +-1e4 with one clear top class; 2
    all-equal rows (an exact tie at the argmax: the lowest index wins, and
    its label is 0); 3 (classes >= 256) a masked class in member 0, not at the
    label; 4 a label out of range (= C).  B >= 9: 5 a NaN in member M // 2; 6 a
    +inf in member 0; 7 an all -inf row in member M - 1 (labels in range);
    8 the label -1."""
    rng = np.random.default_rng(7000 + seed)
    M = comps * D
    x = (3.0 * rng.standard_normal((M, G, B, C))).astype(np.float32)
    lab = rng.integers(0, C, size=B).astype(np.int64)
    w = rng.random((comps, G)) + 0.1
    if comps == 3:
        w[1, G - 1] = 0.0
    w /= w.sum(0, keepdims=True)
    if B >= 5:
        off = np.where(rng.random((M, G, 1)) < 0.5, -1e4, 1e4).astype(np.float32)
        x[:, :, 1, C // 5] += 12.0
        x[:, :, 1, :] += off
        x[:, :, 2, :] = np.float32(0.75)
        lab[2] = 0
        if C >= 256:
            x[0, :, 3, C // 2] = -np.inf
            lab[3] = C // 2 + 1
        lab[4] = C
    if B >= 9:
        x[M // 2, :, 5, C // 3] = np.nan
        x[0, :, 6, C - 1] = np.inf
        x[M - 1, :, 7, :] = -np.inf
        lab[8] = -1
    return x, lab, w


@functools.lru_cache(maxsize=None)
def built(case):
    """(logits, labels, weights, score reference, {combine: mixture reference})
    of a case, computed once and shared (treat as read-only)."""
    x, lab, w = make_case(*case)
    for v in (x, lab, w):
        v.setflags(write=False)
    return x, lab, w, score_reference(x, lab), {c: mixture_reference(x, w, case[3], c)
                                                for c in COMBINES}
