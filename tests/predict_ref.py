"""Host reference of bdl_predict (include/bdl_predict.h): the fp64 definitions,
a NumPy emulation of the header's arithmetic contract, the error bound of every
output derived from that contract, and the input builders of the GPU cases.

Bound derivation.  u = 2^-24 is fp32's unit roundoff; "1 ulp" of expf / logf
(the documented maximum error of the HIP device library) is a relative error
of at most 2^-23 = 2u.  For one member row with d_c = x_c - m <= 0, e_c =
exp(d_c), Z = sum e_c, p_c = e_c / Z, S1 = sum_c p_c |d_c|, S2 = sum_c p_c d_c^2:
  - fl(x - m) has relative error u, an absolute error u|d| in the exponent, so
    a relative error u|d| in e; expf adds 2u:   rel(e_c) <= u (|d_c| + 2).
  - Z is an fp64 sum of the e_c (its own rounding ~2^-53 is nothing):
    rel(Z) <= sum_c p_c rel(e_c) = u (S1 + 2).
  - p_c = e_c * (1/Z) in fp64:  rel(p_c) <= u (|d_c| + 4 + S1).
  - an e_c that underflows (|d| > ~87) is off by at most 2^-148 absolutely.
The mixture is the fp64 mean of the p_c, rounded once to fp32:
    eps_c := err(pbar32_c) <= mean_i p_ic u (|d_ic| + 4 + S1_i) + u pbar_c + 2^-148.
confidence is a maximum of such values: max_c eps_c.  logp_c = logf(pbar32_c):
the relative error eps_c / pbar_c becomes absolute (first order, kept only
while it is below 1 %), plus 1 ulp of the result, 2u |logp_c|; where the
reference's pbar_c is below 2^-100 the kernel's pbar32 may be 0 or denormal and
NO bound is given (inf: the GPU test then only asks for a value <= log 2^-100).
entropy = -sum_c t(pbar_c), t(p) = p log p, |t'| = |log p| + 1:
    sum_c eps_c (|log max(pbar_c, 2^-149)| + 2)  +  2u sum_c pbar_c |log pbar_c|  (logf)
    +  u entropy  (the output's rounding).
H[p_i] = log Z - sum_c p_c d_c.  log Z: rel(Z), the rounding of Z to fp32 and
1 ulp of logf, u (S1 + 2) + u + 2u log Z.  sum_c p_c d_c: each term carries
rel(e_c) + rel(d_c) + rel(Z) = u (|d_c| + 3) + u (S1 + 2):
    b_i := u [ (S1 + 3) + 2 log Z + S2 + 3 S1 + S1 (S1 + 2) ].
expected_entropy: mean_i b_i + u expected_entropy.  mutual_info: the sum of the
two, + u |mutual_info|.  Every bound is multiplied by 1.001 for the second-order
terms and gets 2^-40 for the fp64 sums.  A total's bound is the sum of its
examples' bounds plus 2^-45 of the sum of the magnitudes (fp64 summation of at
most 2^8 x ... terms in any order).  That assumes at most 2^8 terms: n terms
added in any order, over any number of accumulating calls, take at most
n - 1 + calls additions, each rounding a partial sum that is at most the sum S
of the magnitudes by 2^-53, so the error is at most (n - 1 + calls) 2^-53 S.
check_totals compares up to two passes over the same examples (scale = 2, up
to four calls): 2 n + 3 additions on magnitudes 2 S against twice this bound,
which therefore takes (2 n + 4) 2^-53 of S.  A group of more than 2^8 examples
gets that factor, with n the terms of the sum (of a bin: the probabilities in
it); up to 2^8 examples the 2^-45 stays as it was (there it covers one
pass over the five sums, n - 1 < 2^8 additions; for a bin of more than 2^8 probabilities it is not a
derived bound, and is kept so that the earlier cases' criterion does not
change — the bin's summed eps is 10^4 times larger).  Integer outputs have no
bound: they are
exact PROVIDED no reference probability is within the margin of a decision —
`margins` reports how far every case is from one, and tests/test_predict_host.py
asserts 4 x the bound everywhere."""
import functools

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -100          # below: no bound on logp / nll
FLOOR = 2.0 ** -148
MAX_BINS = 64
FLOATS = ("entropy", "expected_entropy", "mutual_info", "confidence", "nll")
INTS = ("pred", "disagree")
INT_TOTALS = ("n", "n_labelled", "n_nonfinite", "n_wrong", "disagree_sum")
SUM_TOTALS = ("nll_sum", "entropy_sum", "expected_entropy_sum", "mi_sum", "mi_sum_wrong")


def edges32(nb):
    return np.linspace(0, 1 + 1e-8, nb + 1)[1:-1].astype(np.float32)


def _xlogx(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)


def nonfinite_examples(x):
    """[G, B]: any member row with a NaN, a +inf or no finite entry."""
    rowbad = (np.isnan(x) | np.isposinf(x)).any(-1) | ~np.isfinite(x).any(-1)
    return rowbad.any(0)


def _totals(r, labels, nb, bins_of, pbin):
    """The per-group totals from per-example results r (fp64 sums by math.fsum-like np.sum)."""
    G, B = r["pred"].shape
    C = r["logp"].shape[-1]
    lab = np.full(B, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    labelled = (lab >= 0) & (lab < C)
    out = []
    for g in range(G):
        ok = ~r["nonfinite"][g]
        okl = ok & labelled
        wrong = okl & (r["pred"][g] != lab)
        t = {"n": int(ok.sum()), "n_labelled": int(okl.sum()),
             "n_nonfinite": int((~ok).sum()), "n_wrong": int(wrong.sum()),
             "disagree_sum": int(r["disagree"][g][ok].sum()),
             "nll_sum": float(r["nll"][g][okl].astype(np.float64).sum()),
             "entropy_sum": float(r["entropy64"][g][ok].sum()),
             "expected_entropy_sum": float(r["expected_entropy64"][g][ok].sum()),
             "mi_sum": float(r["mutual_info64"][g][ok].sum()),
             "mi_sum_wrong": float(r["mutual_info64"][g][wrong].sum())}
        cnt, hits, conf = np.zeros(MAX_BINS, np.int64), np.zeros(MAX_BINS, np.int64), \
            np.zeros(MAX_BINS)
        rows = np.nonzero(okl)[0]
        if len(rows):
            k = bins_of[g][rows].ravel()
            pv = pbin[g][rows].astype(np.float64).ravel()
            hit = (np.arange(C)[None, :] == lab[rows][:, None]).ravel()
            cnt[:nb] = np.bincount(k, minlength=nb)[:nb]
            hits[:nb] = np.bincount(k, weights=hit, minlength=nb)[:nb].astype(np.int64)
            conf[:nb] = np.bincount(k, weights=pv, minlength=nb)[:nb]
        t.update(bin_count=cnt, bin_hits=hits, bin_conf=conf)
        t["wrong_mask"], t["ok_mask"], t["okl_mask"] = wrong, ok, okl
        out.append(t)
    return out


def reference(logits, labels=None, nb=15):
    """The definitions in fp64.  logits [M, G, B, C] (fp32 values)."""
    x = np.asarray(logits, dtype=np.float64)
    M, G, B, C = x.shape
    bad = nonfinite_examples(x)
    xs = np.where(bad[None, :, :, None], 0.0, x)
    m = xs.max(-1, keepdims=True)
    d = xs - m
    e = np.exp(d)
    Z = e.sum(-1, keepdims=True)
    p = e / Z
    Hi = -_xlogx(p).sum(-1)
    pbar = p.mean(0)
    with np.errstate(divide="ignore"):
        logp = np.log(pbar)
    ent = -_xlogx(pbar).sum(-1)
    ee = Hi.mean(0)
    pred = pbar.argmax(-1)
    am = xs.argmax(-1)
    lab = np.full(B, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    labelled = (lab >= 0) & (lab < C)
    safe = np.where(labelled, lab, 0)
    nll = np.where(labelled[None, :], -np.take_along_axis(
        logp, np.broadcast_to(safe[None, :, None], (G, B, 1)), -1)[..., 0], np.nan)
    r = {"logp": logp, "entropy64": ent, "expected_entropy64": ee, "mutual_info64": ent - ee,
         "entropy": ent, "expected_entropy": ee, "mutual_info": ent - ee,
         "confidence": pbar.max(-1), "nll": nll, "pred": pred.astype(np.int64),
         "disagree": (am != pred[None]).sum(0).astype(np.int64), "nonfinite": bad,
         "pbar": pbar, "members": M}
    # ---- what the bounds need
    ad = np.where(p > 0, np.abs(np.where(np.isfinite(d), d, 0.0)), 0.0)
    S1 = (p * ad).sum(-1)
    S2 = (p * ad * ad).sum(-1)
    eps = (p * U * (ad + 4 + S1[..., None])).mean(0) + U * pbar + FLOOR
    r["eps"] = eps * 1.001 + 2.0 ** -45 * pbar
    r["b_member"] = U * ((S1 + 3) + 2 * np.log(Z[..., 0]) + S2 + 3 * S1 + S1 * (S1 + 2))
    for k in FLOATS + ("logp",):
        r[k] = np.where(bad[..., None] if k == "logp" else bad, np.nan, r[k])
    r["pred"] = np.where(bad, -1, r["pred"])
    r["disagree"] = np.where(bad, -1, r["disagree"])
    ed = np.linspace(0, 1 + 1e-8, nb + 1)[1:-1]
    bins_of = (pbar[..., None] >= ed).sum(-1)
    r["bins_of"] = bins_of
    r["totals"] = _totals(r, labels, nb, bins_of, pbar)
    return r


def bound(r, labels=None):
    """Absolute error bounds of the fp32 outputs ([G, B]; logp [G, B, C]) and of
    the fp64 totals (a list per group) for a `reference` result."""
    pbar, eps = r["pbar"], r["eps"]
    G, B, C = pbar.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        alog = np.abs(np.log(np.maximum(pbar, 2.0 ** -149)))
        rel = eps / pbar
        blogp = np.where((pbar >= TINY) & (rel < 0.01), rel * 1.01 + 2 * U * alog, np.inf)
    bent = ((eps * (alog + 2)).sum(-1) + 2 * U * np.abs(_xlogx(pbar)).sum(-1)
            + U * np.abs(r["entropy64"])) * 1.001 + 2.0 ** -40
    bee = (r["b_member"].mean(0) + U * np.abs(r["expected_entropy64"])) * 1.001 + 2.0 ** -40
    bmi = bent + bee + U * np.abs(r["mutual_info64"])
    lab = np.full(B, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    labelled = (lab >= 0) & (lab < C)
    safe = np.where(labelled, lab, 0)
    bnll = np.take_along_axis(blogp, np.broadcast_to(safe[None, :, None], (G, B, 1)), -1)[..., 0]
    out = {"logp": blogp, "entropy": bent, "expected_entropy": bee, "mutual_info": bmi,
           "confidence": eps.max(-1), "nll": bnll, "eps": eps}
    tots = []
    for g, t in enumerate(r["totals"]):
        ok, okl, wrong = t["ok_mask"], t["okl_mask"], t["wrong_mask"]

        many = int(ok.sum()) + t["n_nonfinite"] > 2 ** 8

        def sumf(n):
            return (2 * n + 4) * 2.0 ** -53 if many else 2.0 ** -45

        def tot(b, v, sel):
            return float(b[g][sel].sum() + sumf(int(sel.sum())) * np.abs(v[g][sel]).sum())
        bt = {"nll_sum": tot(bnll, np.nan_to_num(r["nll"], posinf=0.0), okl),
              "entropy_sum": tot(bent, r["entropy64"], ok),
              "expected_entropy_sum": tot(bee, r["expected_entropy64"], ok),
              "mi_sum": tot(bmi, r["mutual_info64"], ok),
              "mi_sum_wrong": tot(bmi, r["mutual_info64"], wrong)}
        bc = np.zeros(MAX_BINS)
        rows = np.nonzero(okl)[0]
        if len(rows):
            k = r["bins_of"][g][rows].ravel()
            nbins = int(k.max()) + 1
            fk = np.array([sumf(int(n)) for n in np.bincount(k, minlength=nbins)])
            w = (eps[g][rows].ravel() + fk[k] * pbar[g][rows].ravel())
            bc[:nbins] = np.bincount(k, weights=w, minlength=nbins)
        bt["bin_conf"] = bc
        tots.append(bt)
    out["totals"] = tots
    return out


def emulate(logits, labels=None, nb=15):
    """The header's arithmetic contract step by step in NumPy (np.exp / np.log
    on fp32 stand in for expf / logf: both are within their ulp bound of the
    true value, not bit-equal to the device's).  Returns what `reference`
    returns, for finite inputs."""
    x = np.asarray(logits, dtype=np.float32)
    M, G, B, C = x.shape
    bad = nonfinite_examples(x.astype(np.float64))
    xs = np.where(bad[None, :, :, None], np.float32(0), x)
    acc = np.zeros((G, B, C))
    hsum = np.zeros((G, B))
    am = xs.argmax(-1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in range(M):
            m = xs[i].max(-1, keepdims=True)
            d = (xs[i] - m).astype(np.float32)
            e = np.exp(d).astype(np.float32)
            e64, d64 = e.astype(np.float64), d.astype(np.float64)
            Z = e64.sum(-1)
            T = np.where(e != 0, e64 * np.where(e != 0, d64, 0.0), 0.0).sum(-1)
            rz = 1.0 / Z
            hsum += np.log(Z.astype(np.float32)).astype(np.float64) - T * rz
            acc += e64 * rz[..., None]
        p32 = (acc / float(M)).astype(np.float32)
        lp = np.log(p32).astype(np.float32)
        ent = -np.where(p32 != 0, p32.astype(np.float64) * np.where(p32 != 0, lp, 0).astype(
            np.float64), 0.0).sum(-1)
    ee = hsum / float(M)
    pred = p32.argmax(-1)
    lab = np.full(B, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    labelled = (lab >= 0) & (lab < C)
    safe = np.where(labelled, lab, 0)
    nll = np.where(labelled[None, :], -np.take_along_axis(
        lp, np.broadcast_to(safe[None, :, None], (G, B, 1)), -1)[..., 0], np.float32("nan"))
    r = {"logp": lp, "entropy64": ent, "expected_entropy64": ee, "mutual_info64": ent - ee,
         "entropy": ent.astype(np.float32), "expected_entropy": ee.astype(np.float32),
         "mutual_info": (ent - ee).astype(np.float32), "confidence": p32.max(-1),
         "nll": nll.astype(np.float32), "pred": pred.astype(np.int64),
         "disagree": (am != pred[None]).sum(0).astype(np.int64), "nonfinite": bad, "members": M}
    for k in FLOATS + ("logp",):
        r[k] = np.where(bad[..., None] if k == "logp" else bad, np.float32("nan"), r[k])
    r["pred"] = np.where(bad, -1, r["pred"])
    r["disagree"] = np.where(bad, -1, r["disagree"])
    bins_of = (p32[..., None] >= edges32(nb)).sum(-1)
    r["totals"] = _totals(r, labels, nb, bins_of, p32)
    return r


def margins(r, b, nb=15):
    """How far the reference is from every decision an error could flip, as a
    multiple of the bound there (inf: nothing to flip): a probability of a
    finite example against the nearest bin edge (the edge's own fp32 rounding,
    u, is part of the bound), an example's top two mixture probabilities.
    `tied`: [G, B] examples whose top two are a constructed (exact) tie."""
    pbar, eps = r["pbar"], b["eps"]
    ok = ~r["nonfinite"]
    ed = np.linspace(0, 1 + 1e-8, nb + 1)[1:-1]
    if len(ed):
        dist = np.abs(pbar[..., None] - ed).min(-1)
        edge = np.where(ok[..., None], dist / (eps + U), np.inf).min()
    else:
        edge = np.inf
    C = pbar.shape[-1]
    if C > 1:
        top = np.sort(pbar, -1)
        gap = top[..., -1] - top[..., -2]
        tied = gap == 0
        top2 = np.where(ok & ~tied, gap / eps.max(-1), np.inf).min()
    else:
        tied, top2 = np.zeros(pbar.shape[:2], bool), np.inf
    return {"edge": float(edge), "top2": float(top2), "tied": tied}


def member_ties(logits):
    """[M, G, B]: a member row whose maximum is attained more than once (its
    argmax is exact on the device — raw fp32 compares — so only an exact tie
    can differ, and the lowest index settles it)."""
    x = np.asarray(logits)
    with np.errstate(invalid="ignore"):
        return (x == np.nanmax(np.where(np.isnan(x), -np.inf, x), -1, keepdims=True)).sum(-1) > 1


# ------------------------------------------------------------------ the cases
# (classes, members, groups, batch, seed).  C: scalar and 16-B paths, fewer
# classes than lanes, both sides of the wave / workgroup boundary (256 | 257,
# 260), one trip exactly (1000, 1024), one lane into a second (1028), every
# trip count of the workgroup instance (1, 2, 4, 8) on both load paths (1030
# and 2052 complete the ten instances of launch_by_classes: two trips element
# by element, four in 16-B loads), the limit.  B = 5 on two workgroups gives
# uneven second trips.
CASES = [
    (1, 1, 1, 1, 1), (2, 2, 1, 5, 2), (3, 5, 3, 5, 3), (10, 40, 1, 130, 4), (10, 5, 3, 130, 5),
    (10, 1, 1, 130, 6), (37, 2, 1, 130, 7), (37, 1, 3, 5, 8), (255, 2, 1, 5, 9),
    (256, 5, 1, 5, 10), (257, 5, 1, 5, 11), (260, 2, 3, 5, 12), (1000, 40, 1, 5, 13),
    (1000, 5, 3, 130, 14), (1024, 2, 1, 130, 15), (1024, 1, 1, 5, 16), (1028, 5, 1, 130, 17),
    (1028, 2, 3, 1, 18), (2050, 2, 1, 5, 19), (4099, 2, 1, 5, 20), (4100, 2, 1, 5, 21),
    (8192, 2, 1, 5, 22), (1030, 2, 1, 5, 23), (2052, 2, 1, 5, 24),
]
NB = 15


def case_id(c):
    return "C{}-M{}-G{}-B{}".format(*c[:4])


def make_case(C, M, G, B, seed, nb=NB):
    """logits [M, G, B, C] ~ N(0, 3^2) and labels [B], with the constructed
    examples (of every group): 1 rows offset by +-1e4; 2 a spread of 200 (exp
    underflows to p = 0); 3 all-equal rows (pred = 0; where 1/C sits on a bin
    edge the last class is lowered instead, a two-way tie); 4 a masked class;
    and, with B >= 8, 5 a NaN, 6 a +inf, 7 an all -inf row in one member each.
    Labels: uniform, the spread example's is its top class (so that its nll is
    bounded), one -1 and one C."""
    rng = np.random.default_rng(1000 + seed)
    x = (3.0 * rng.standard_normal((M, G, B, C))).astype(np.float32)
    lab = rng.integers(0, C, size=B).astype(np.int64)
    if B >= 5:
        off = np.where(rng.random((M, G, 1)) < 0.5, -1e4, 1e4).astype(np.float32)
        x[:, :, 1, C // 5] += 12.0   # (fp32's spacing at 1e4 is 1e-3: no accidental tie at the top)
        x[:, :, 1, :] += off
        if C > 1:
            x[:, :, 2, :] = (rng.random((M, G, C)) * 200.0).astype(np.float32)
            x[:, :, 2, 0] = 230.0  # one clear top class in every member
            x[:, :, 2, C - 1] = 5.0  # exp(-225) is 0 in fp32
        x[:, :, 3, :] = np.float32(0.75)
        ed = np.linspace(0, 1 + 1e-8, nb + 1)[1:-1]
        if C >= 3 and np.abs(1.0 / C - ed).min() < 1e-4:
            x[:, :, 3, C - 1] = np.float32(-0.55)
        if C > 1:
            x[:, :, 4, C // 2] = -np.inf
        lab[2] = 0
        lab[1], lab[4] = -1, C
    if B >= 8:
        x[M // 2, :, 5, C // 3] = np.nan
        x[0, :, 6, C - 1] = np.inf
        x[M - 1, :, 7, :] = -np.inf
    return x, lab


@functools.lru_cache(maxsize=None)
def built(case):
    """(logits, labels, reference, bound) of a case, computed once and shared
    (treat as read-only)."""
    x, lab = make_case(*case)
    r = reference(x, lab, NB)
    x.setflags(write=False)
    lab.setflags(write=False)
    return x, lab, r, bound(r, lab)
