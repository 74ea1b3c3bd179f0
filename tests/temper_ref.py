"""Host reference of the temperature-scaling unit (include/bdl_temper.h): the
fp64 definitions (fit by the same safeguarded Newton, report), a NumPy emulation
of the header's arithmetic contract, the error bounds derived from that
contract, and the margins of every decision an error could flip.

Bound derivation.  u = 2^-24; "1 ulp" of expf is a relative error of at most
2u.  For one row at an fp32 beta, t_c = beta z_c, m = max t, d_c = t_c - m,
p_c = softmax(t)_c.  The kernel forms fl(t_c) (error u|t_c|), fl(m), then
fl(fl(t_c) - fl(m)) (error u|d_c| more) and e_c = expf(.) (2u more).  Every
quantity below is invariant under a common shift of the exponents, so the
error of fl(m) cancels and e_c stands for exp(t_c - fl(m)) with a relative
error of at most
    rho_c = u (|t_c| + |d_c| + 2).
With R = sum_c p_c rho_c, E = E_p[z], V = Var_p[z] (first order in rho):
    lse = fl(m) + log S0:            |err| <= R
    f   = lse - fl(t_y):             |err| <= R + u |t_y|
    f'  = S1 / S0 - z_y:             |err| <= sum_c p_c rho_c |z_c - E|
    f'' = S2 / S0 - (S1 / S0)^2:     |err| <= sum_c p_c rho_c |(z_c - E)^2 - V|
                                              + 2^-50 (E^2 + V)   (the fp64 cancellation)
    q_c = e_c / S0, rounded to fp32: eps_c = q_c (rho_c + R + u) + 2^-126
                                     (2^-126: an e_c that underflows)
    entropy = log S0 - T1 / S0 = -sum q' log q' + sum q' (log e - d), |log e - d| <= 2u:
                                     |err| <= sum_c eps_c (|log max(q_c, 2^-149)| + 1) + 2u
Every bound is multiplied by 1.001 + 4 max_c rho_c for the second-order terms
and gets 2^-40 (relative to the magnitudes involved) for the fp64 sums.  A mean
over examples has the mean of the bounds.  The fitted temperature: a converged
fit's last Newton step is within rtol beta, the rounding of beta to fp32 adds
u beta, and the mean f' it saw is within b' of the true F'; F' has slope F'' at
the optimum, so |beta - beta*| <= b' / F'' + (rtol + u) beta and, T = 1 / beta,
    |T - T*| <= (T^2 b' / F'' + (rtol + u) T) 1.01.
Integers and bins have no bound: they are exact PROVIDED no probability is
within eps_c + u of an fp32 edge — `margins` reports the smallest such distance
as a multiple of that."""
import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -126
MAX_BINS = 64
BETA_MIN, BETA_MAX = float(np.float32(1.0) / np.float32(100.0)), 100.0


def edges32(nb):
    return np.linspace(0, 1 + 1e-8, nb + 1)[1:-1].astype(np.float32)


def _labels(labels, N, C):
    lab = np.full(N, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    return lab, (lab >= 0) & (lab < C)


def classify(z, labels, beta):
    """(nonfinite, inf_label, used, labelled) masks [N] of one group's rows at
    an fp32 beta — the header's special values."""
    z = np.asarray(z, dtype=np.float32)
    N, C = z.shape
    lab, labelled = _labels(labels, N, C)
    b32 = np.float32(beta)
    with np.errstate(over="ignore", invalid="ignore"):
        bad = (np.isnan(z) | np.isposinf(z)).any(-1) | ~np.isfinite(z).any(-1)
        zmax = np.where(bad, np.float32(0), np.where(np.isnan(z), -np.inf, z).max(-1))
        bad |= ~np.isfinite((b32 * zmax.astype(np.float32)).astype(np.float32))
        zy = z[np.arange(N), np.where(labelled, lab, 0)]
        ty = (b32 * zy).astype(np.float32)
    infl = ~bad & labelled & np.isneginf(ty)
    return bad, infl, ~bad & labelled & ~infl, labelled


def _rows64(z, beta):
    """fp64 row quantities of finite rows: t, d, p, lse (beta as given: the
    device's is an fp32 value, the fp64 reference fit's is not)."""
    t = float(beta) * z.astype(np.float64)
    m = t.max(-1, keepdims=True)
    d = t - m
    e = np.exp(d)
    S0 = e.sum(-1, keepdims=True)
    return t, d, e / S0, (m + np.log(S0))[:, 0]


def _zfin(z):
    return np.where(np.isfinite(z), z, 0.0)


def fit_terms(z, labels, beta):
    """The definitions in fp64 at an fp32 beta, per used example: f, f', f''
    and their bounds (dicts of arrays over the used examples) + the masks."""
    z = np.asarray(z, dtype=np.float32)
    N, C = z.shape
    lab, _ = _labels(labels, N, C)
    bad, infl, used, labelled = classify(z, lab, beta)
    zz = z[used].astype(np.float64)
    y = lab[used]
    n = len(y)
    with np.errstate(invalid="ignore", over="ignore"):
        t, d, p, lse = _rows64(zz, beta)
    zf = _zfin(zz)
    ty = t[np.arange(n), y]
    E = (p * zf).sum(-1)
    dev = zf - E[:, None]
    V = (p * dev * dev).sum(-1)
    rho = np.where(p > 0, U * (np.abs(_zfin(t)) + np.abs(_zfin(d)) + 2), 0.0)
    R = (p * rho).sum(-1)
    mult = 1.001 + 4 * (rho.max(-1) if C else 0)
    bf = (R + U * np.abs(ty)) * mult + 2.0 ** -40 * (np.abs(lse) + np.abs(ty)) + FLOOR * C
    b1 = (p * rho * np.abs(dev)).sum(-1) * mult + 2.0 ** -40 * (np.abs(E) + np.abs(zf[np.arange(n), y]))
    b2 = ((p * rho * np.abs(dev * dev - V[:, None])).sum(-1) * mult
          + 2.0 ** -50 * (E * E + V) + 2.0 ** -40 * V)
    span = np.abs(dev).max(-1) if C else 0
    b1 = b1 + FLOOR * C * span
    b2 = b2 + FLOOR * C * span * span
    return {"f": lse - ty, "f1": E - zf[np.arange(n), y], "f2": V, "bf": bf, "b1": b1, "b2": b2,
            "n": n, "n_nonfinite": int(bad.sum()), "n_inf_label": int(infl.sum()), "used": used}


def sweep_reference(z, labels, beta):
    """What one fit sweep + update stores for a group: nll, d1, d2 (means), the
    counts, and the bounds of the three means."""
    r = fit_terms(z, labels, beta)
    n = r["n"]
    mean = (lambda a: float(a.sum() / n)) if n else (lambda a: float("nan"))
    return {"nll": mean(r["f"]), "d1": mean(r["f1"]) if n else 0.0, "d2": mean(r["f2"]) if n else 0.0,
            "b_nll": mean(r["bf"]), "b_d1": mean(r["b1"]), "b_d2": mean(r["b2"]), "n": n,
            "n_nonfinite": r["n_nonfinite"], "n_inf_label": r["n_inf_label"]}


def _emulated_sweep(z, labels, beta):
    """The contract step by step (np.exp on fp32 stands in for expf: within its
    ulp bound of the true value, not bit-equal to the device's)."""
    z = np.asarray(z, dtype=np.float32)
    N, C = z.shape
    lab, _ = _labels(labels, N, C)
    bad, infl, used, _ = classify(z, lab, beta)
    b32 = np.float32(beta)
    zz, y = z[used], lab[used]
    n = len(y)
    out = {"n": n, "n_nonfinite": int(bad.sum()), "n_inf_label": int(infl.sum())}
    if n == 0:
        return dict(out, nll=float("nan"), d1=0.0, d2=0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (b32 * zz).astype(np.float32)
        m = (b32 * zz.max(-1, keepdims=True)).astype(np.float32)
        d = (t - m).astype(np.float32)
        e = np.exp(d).astype(np.float32).astype(np.float64)
    z64 = np.where(e != 0, _zfin(zz.astype(np.float64)), 0.0)
    S0, S1, S2 = e.sum(-1), (e * z64).sum(-1), (e * z64 * z64).sum(-1)
    E = S1 / S0
    V = np.maximum(S2 / S0 - E * E, 0.0)
    ty = t[np.arange(n), y].astype(np.float64)
    f = (m[:, 0].astype(np.float64) + np.log(S0)) - ty
    f1 = E - zz[np.arange(n), y].astype(np.float64)
    return dict(out, nll=float(f.sum() / n), d1=float(f1.sum() / n), d2=float(V.sum() / n))


def newton(z, labels, rtol=1e-6, max_iter=32, beta0=1.0, sweep=_emulated_sweep, fp32=True):
    """bdl_temper_fit_update's rule over `max_iter` (sweep, update) pairs for
    one group.  sweep=_emulated_sweep, fp32=True: the emulation of the device;
    sweep=sweep_reference, fp32=False: the fp64 reference fit (beta not rounded).
    Returns the state's fields as a dict, with `margin`: the smallest distance
    of a decision from its threshold — the step against rtol * beta, an
    unclamped new beta against either limit — as a multiple of the bound of the
    Newton step there (inf: no decision to flip)."""
    st = {"beta": float(np.float32(beta0)) if fp32 else float(beta0), "iterations": 0,
          "sweeps": 0, "converged": False, "at_bound": False, "degenerate": False, "done": False,
          "nll_first": float("nan"), "margin": float("inf")}
    for _ in range(max_iter):
        if st["done"]:
            break
        s = sweep(z, labels, st["beta"])
        st.update(nll=s["nll"], d1=s["d1"], d2=s["d2"], n=s["n"], n_nonfinite=s["n_nonfinite"],
                  n_inf_label=s["n_inf_label"])
        if st["sweeps"] == 0:
            st["nll_first"] = s["nll"]
        st["sweeps"] += 1
        st["degenerate"] = s["n"] == 0 or not s["d2"] > 0.0 or not np.isfinite(s["d1"])
        if st["degenerate"] or st["iterations"] >= max_iter:
            break   # (the device sweeps on: the same values every time)
        beta = st["beta"]
        raw = beta - s["d1"] / s["d2"]
        nb = min(max(raw, 0.25 * beta), 4.0 * beta)
        ref = sweep_reference(z, labels, beta)
        step_err = (ref["b_d1"] + abs(s["d1"] / s["d2"]) * ref["b_d2"]) / s["d2"] + U * beta
        if nb == raw:   # (a step cut to beta / 4 or 4 beta lands where it lands)
            st["margin"] = min(st["margin"], abs(nb - BETA_MIN) / step_err,
                               abs(nb - BETA_MAX) / step_err)
        at_bound = False
        if nb <= BETA_MIN:
            nb, at_bound = BETA_MIN, True
        if nb >= BETA_MAX:
            nb, at_bound = BETA_MAX, True
        if fp32:
            nb = float(np.float32(nb))
        st["at_bound"] = at_bound
        if not at_bound:
            st["margin"] = min(st["margin"], abs(abs(nb - beta) - rtol * beta) / step_err)
        if not at_bound and abs(nb - beta) <= rtol * beta:
            st["converged"] = st["done"] = True
        elif at_bound and nb == beta:
            st["done"] = True   # on the limit, the step beyond it
        elif nb != beta:
            st["beta"] = nb
            st["iterations"] += 1
    st["temperature"] = 1.0 / st["beta"]
    return st


def fit_reference(z, labels, rtol=1e-10, max_iter=100):
    """The fp64 fit: the same Newton, beta in fp64, to rtol = 1e-10."""
    return newton(z, labels, rtol=rtol, max_iter=max_iter, sweep=sweep_reference, fp32=False)


def curvature_T(z, labels, T):
    """d^2/dT^2 of the mean NLL at T, in fp64 (beta not rounded)."""
    z = np.asarray(z, dtype=np.float64)
    lab = np.asarray(labels)
    beta = 1.0 / T
    t = beta * z
    p = np.exp(t - t.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    E = (p * z).sum(-1)
    F1 = float((E - z[np.arange(len(lab)), lab]).mean())
    F2 = float(((p * z * z).sum(-1) - E * E).mean())
    return F2 * beta ** 4 + 2 * F1 * beta ** 3   # d beta / dT = -beta^2


def bound_T(z, labels, fit, rtol):
    """|T - T*| of a converged emulated / device fit (the module docstring)."""
    ref = sweep_reference(z, labels, fit["beta"])
    T = 1.0 / fit["beta"]
    return (T * T * ref["b_d1"] / ref["d2"] + (rtol + U) * T) * 1.01


# ------------------------------------------------------------------ the report
def _bins(q, lab_rows, nb, edges):
    cnt, hits, conf = np.zeros(MAX_BINS, np.int64), np.zeros(MAX_BINS, np.int64), np.zeros(MAX_BINS)
    if len(lab_rows):
        C = q.shape[-1]
        k = (q[..., None] >= edges).sum(-1).ravel()
        hit = (np.arange(C)[None, :] == lab_rows[:, None]).ravel()
        cnt[:nb] = np.bincount(k, minlength=nb)[:nb]
        hits[:nb] = np.bincount(k, weights=hit, minlength=nb)[:nb].astype(np.int64)
        conf[:nb] = np.bincount(k, weights=q.astype(np.float64).ravel(), minlength=nb)[:nb]
    return cnt, hits, conf


def report_reference(z, labels, beta, nb=15):
    """The definitions in fp64 for one group: bdl_temper_totals' fields, the
    bounds of its sums (`b_*`, bin_conf's per bin) and what `margins` needs."""
    z = np.asarray(z, dtype=np.float32)
    N, C = z.shape
    lab, labelled = _labels(labels, N, C)
    bad, _, _, _ = classify(z, lab, beta)
    ok = ~bad
    zz = z[ok].astype(np.float64)
    okl = labelled[ok]
    y = lab[ok]
    n = len(zz)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t, d, q, lse = _rows64(zz, beta)
        ty = t[np.arange(n), np.where(okl, y, 0)]
        nll = lse - ty
        rho = np.where(q > 0, U * (np.abs(_zfin(t)) + np.abs(_zfin(d)) + 2), 0.0)
        R = (q * rho).sum(-1)
        mult = (1.001 + 4 * rho.max(-1))[:, None] if n else 1.0
        eps = q * (rho + R[:, None] + U) * mult + FLOOR + 2.0 ** -45 * q
        alog = np.abs(np.log(np.maximum(q, 2.0 ** -149)))
        ent = -np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0).sum(-1)
        bent = (eps * (alog + 1)).sum(-1) + 2 * U + 2.0 ** -40 * (1 + ent)
        bnll = (R + U * np.abs(ty)) * mult[:, 0] + 2.0 ** -40 * (np.abs(lse) + np.abs(ty)) if n \
            else np.zeros(0)
    pred = np.where(np.isnan(z[ok]), -np.inf, z[ok]).argmax(-1) if n else np.zeros(0, np.int64)
    ed = np.linspace(0, 1 + 1e-8, nb + 1)[1:-1]
    cnt, hits, conf = _bins(q[okl], y[okl], nb, ed)
    bconf = np.zeros(MAX_BINS)
    if okl.any():
        k = (q[okl][..., None] >= ed).sum(-1).ravel()
        bconf[:nb] = np.bincount(k, weights=eps[okl].ravel(), minlength=nb)[:nb]
    return {"n": n, "n_labelled": int(okl.sum()), "n_nonfinite": int(bad.sum()),
            "n_wrong": int((okl & (pred != y)).sum()), "nll_sum": float(nll[okl].sum()),
            "entropy_sum": float(ent.sum()), "confidence_sum": float(q.max(-1).sum()) if n else 0.0,
            "bin_count": cnt, "bin_hits": hits, "bin_conf": conf,
            "b_nll_sum": float(np.where(np.isfinite(nll[okl]), bnll[okl], 0.0).sum()),
            "b_entropy_sum": float(bent.sum()),
            "b_confidence_sum": float(eps.max(-1).sum()) if n else 0.0, "b_bin_conf": bconf,
            "q": q, "eps": eps, "okl": okl}


def report_emulate(z, labels, beta, nb=15):
    """The contract step by step for one group."""
    z = np.asarray(z, dtype=np.float32)
    N, C = z.shape
    lab, labelled = _labels(labels, N, C)
    bad, _, _, _ = classify(z, lab, beta)
    ok = ~bad
    zz, okl, y = z[ok], labelled[ok], lab[ok]
    n = len(zz)
    b32 = np.float32(beta)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (b32 * zz).astype(np.float32)
        m = (b32 * zz.max(-1, keepdims=True)).astype(np.float32)
        d = (t - m).astype(np.float32)
        e = np.exp(d).astype(np.float32).astype(np.float64)
        d64 = np.where(e != 0, d.astype(np.float64), 0.0)
        S0, T1 = e.sum(-1), (e * d64).sum(-1)
        rz = 1.0 / S0
        q32 = (e * rz[:, None]).astype(np.float32)
        lz = np.log(S0)
        ty = t[np.arange(n), np.where(okl, y, 0)].astype(np.float64)
        nll = (m[:, 0].astype(np.float64) + lz) - ty
    pred = zz.argmax(-1) if n else np.zeros(0, np.int64)
    cnt, hits, conf = _bins(q32[okl], y[okl], nb, edges32(nb))
    return {"n": n, "n_labelled": int(okl.sum()), "n_nonfinite": int(bad.sum()),
            "n_wrong": int((okl & (pred != y)).sum()), "nll_sum": float(nll[okl].sum()),
            "entropy_sum": float((lz - T1 * rz).sum()),
            "confidence_sum": float(rz.astype(np.float32).astype(np.float64).sum()),
            "bin_count": cnt, "bin_hits": hits, "bin_conf": conf}


def margins(r, nb=15):
    """The smallest distance of a labelled example's probability from a bin
    edge, as a multiple of its bound eps_c + u (the edge's own fp32 rounding is
    the u); inf with one bin or no labelled example."""
    ed = np.linspace(0, 1 + 1e-8, nb + 1)[1:-1]
    q, eps = r["q"][r["okl"]], r["eps"][r["okl"]]
    if not len(ed) or not q.size:
        return float("inf")
    return float((np.abs(q[..., None] - ed).min(-1) / (eps + U)).min())


def summary(tot, nb=15):
    """n, nll, error, ece, mce, entropy, confidence of a totals mapping
    (calibration.analyze's formula on the bins)."""
    cnt = np.asarray(tot["bin_count"][:nb], dtype=np.float64)
    hits = np.asarray(tot["bin_hits"][:nb], dtype=np.float64)
    conf = np.asarray(tot["bin_conf"][:nb], dtype=np.float64)
    full = cnt > 0
    gap = np.abs(np.where(full, hits / np.where(full, cnt, 1), 0.0)
                 - np.where(full, conf / np.where(full, cnt, 1), 0.0))
    nl, n = int(tot["n_labelled"]), int(tot["n"])
    return {"n": n, "nll": float(tot["nll_sum"]) / nl, "error": int(tot["n_wrong"]) / nl,
            "ece": float((gap * cnt / cnt.sum()).sum()), "mce": float(gap.max()),
            "entropy": float(tot["entropy_sum"]) / n, "confidence": float(tot["confidence_sum"]) / n}


def summary_bound(r, nb=15):
    """Bounds of `summary`'s nll / ece / mce for a report_reference result whose
    bins are decided (margins > 1): a bin's mean confidence moves by at most
    b_bin_conf / count."""
    cnt = r["bin_count"][:nb].astype(np.float64)
    per = np.where(cnt > 0, r["b_bin_conf"][:nb] / np.where(cnt > 0, cnt, 1), 0.0)
    return {"nll": r["b_nll_sum"] / max(r["n_labelled"], 1),
            "ece": float((per * cnt / max(cnt.sum(), 1)).sum()) + 1e-15,
            "mce": float(per.max()) + 1e-15}


# ------------------------------------------------------------------ the cases
def make_rows(N, C, seed, scale=3.0, sharp=1.0, special=False):
    """z [N, C] ~ `sharp` x log-softmax of N(0, scale^2) logits (a row of
    log-probabilities, then sharpened or flattened so that the optimum is away
    from T = 1) and labels drawn from softmax of the unsharpened row; with
    special and N >= 8, rows 1..7 are: a masked class, a NaN, a +inf, an all
    -inf row, a -inf at the label, labels -1 and C."""
    rng = np.random.default_rng(7000 + seed)
    x = scale * rng.standard_normal((N, C))
    lp = x - np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)) - x.max(-1, keepdims=True)
    p = np.exp(lp)
    lab = np.array([rng.choice(C, p=pi / pi.sum()) for pi in p], dtype=np.int64)
    z = (sharp * lp).astype(np.float32)
    if special and N >= 8:
        z[1, (lab[1] + 1) % C] = -np.inf if C > 1 else z[1, 0]
        z[2, C // 3] = np.nan
        z[3, C - 1] = np.inf
        z[4, :] = -np.inf
        if C > 1:
            z[5, lab[5]] = -np.inf
        lab[6], lab[7] = -1, C
    return z, lab
