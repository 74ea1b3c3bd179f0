"""NumPy reference of the stacking unit (include/bdl_stacking.h).

1. `gather` and `fit`: a LITERAL restatement of the contract — the exclusion
   rules and their order, fp32 d = ell - m and e = exp(d), fp64 s (voter order,
   product then sum), r = e * (1/s), the tile partition of 1024 columns, the
   thread-strided / wave-butterfly / waves-in-order sums of a tile, the tiles in
   ascending order, the update.  The only licence: e is the correctly rounded
   exp (fp64 exp rounded to fp32) where the device has expf (<= 1 ulp), and
   fp64 log is NumPy's.
2. `solve`: an INDEPENDENT fp64 solver of the same concave problem — for P = 2
   a bisection on f'(w), otherwise plain EM (np.sum) run to gap 1e-9.
3. The error bound of the kernel against (1), derived from the contract.

Bound (u = 2^-24, T updates, n valid examples, P voters).  The device's e_k and
the reference's differ by at most 1 ulp + 0.5 ulp = 3u relatively (d is the
same IEEE subtraction in both).  s is a positive combination of the e_k, so it
moves by at most 3u relatively too, r_k = e_k / s by 6u, and so does
g_k = mean r_k; the fp64 products, sums over P voters and n examples, the
reciprocal and log add at most (n + P) 2^-52.  So ONE pass injects at most
eta = 6u + (n + P) 2^-52 into every log g_k, hence into every log w_k.  An
injected perturbation x of log w is carried through a later update as
(I - A) x (before the renormalisation, which removes a common shift), with
A_kj = sum_i q_ik q_ij / (n D_k), q the responsibilities, D_k = mean_i q_ik:
A is row-stochastic and D^(1/2) A D^(-1/2) is symmetric positive semi-definite,
so the eigenvalues of I - A lie in [0, 1] and, to first order, no perturbation
grows.  The T + 1 passes' injections add:  |delta log w_k| <= (T + 1) eta, and
with w_k <= 1
    |w_k - w_k^ref| <= bw = (T + 1) eta.
For the SAME w the objectives differ by the perturbation of log s, 3u, plus the
fp64 sum's (n + P) 2^-52 max(1, |objective|); the differing w adds, to first
order, |sum_k g_k w_k dlog w_k| <= max_k |dlog w_k| (sum_k w_k g_k = 1):
    |objective - objective^ref| <= bo = 3u + bw + (n + P) 2^-52 max(1, |objective|).
g_k moves by its own eta and through w by d log g = -A dlog w, at most
max_j |dlog w_j| since A is row-stochastic; in absolute terms (g_k <= 1 + gap)
    |gap - gap^ref| <= bg = (1 + gap) (eta + bw).
`iterations` is the first pass at which gap <= tol, so it lies between the
reference's first pass with gap <= tol + bg and its first with gap <= tol - bg
(bg at that pass); where the reference's gap never gets below tol - bg within
max_iter, max_iter is the upper end.
"""
import numpy as np

U = 2.0 ** -24
TILE, BLOCK, MAX_VOTERS, MAX_CLASSES, MAX_COLS = 1024, 256, 64, 8192, 1 << 24


# ----------------------------------------------------------------- the gather
def gather(logp, labels):
    """(ell [P, B] fp32, valid [B] int32, counts {n_label, n_nonfinite,
    n_impossible}) of logp [P, B, C] and int64 labels [B]."""
    logp = np.asarray(logp, dtype=np.float32)
    P, B, C = logp.shape
    ell = np.zeros((P, B), dtype=np.float32)
    valid = np.zeros(B, dtype=np.int32)
    counts = {"n_label": 0, "n_nonfinite": 0, "n_impossible": 0}
    for b in range(B):
        lab = int(labels[b])
        if not 0 <= lab < C:
            counts["n_label"] += 1
            continue
        col = logp[:, b, lab]
        if np.isnan(col).any() or (col == np.inf).any():
            counts["n_nonfinite"] += 1
        elif (col == -np.inf).all():
            counts["n_impossible"] += 1
        else:
            ell[:, b] = col
            valid[b] = 1
    return ell, valid, counts


# ------------------------------------------------------------ the tile table
def tile_table(n_cols, grid_blocks):
    """[(workgroup, tile, first column, columns)]: tile t covers the columns
    [1024 t, min(1024 (t + 1), n_cols)) and is taken by workgroup t % grid."""
    ntiles = -(-int(n_cols) // TILE)
    return [(t % int(grid_blocks), t, t * TILE, min(TILE, int(n_cols) - t * TILE))
            for t in range(ntiles)]


def _tile_sums(v):
    """v [..., ntiles * 1024] (0.0 where there is nothing to add: x + 0.0 = x)
    -> [...]: per tile the thread-strided sums (column t + 256 j, j ascending,
    from 0.0), the wave butterfly (xor 32, .., 1), the waves in order; then the
    tiles in ascending order from 0.0."""
    lead = v.shape[:-1]
    ntiles = v.shape[-1] // TILE
    x = v.reshape(lead + (ntiles, TILE // BLOCK, BLOCK))
    acc = np.zeros(lead + (ntiles, BLOCK))
    for j in range(TILE // BLOCK):
        acc = acc + x[..., j, :]
    acc = acc.reshape(lead + (ntiles, BLOCK // 64, 64))
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ off]
    waves = acc[..., 0]  # every lane holds the same value
    t = waves[..., 0]
    for w in range(1, BLOCK // 64):
        t = t + waves[..., w]
    tot = np.zeros(lead)
    for i in range(ntiles):
        tot = tot + t[..., i]
    return tot


class _Problem:
    """The per-example constants of a fit: m, e (fp32) of the valid columns,
    padded with zeros to whole tiles."""

    def __init__(self, ell, valid, n_cols):
        ell = np.asarray(ell, dtype=np.float32)[:, :n_cols]
        self.P = ell.shape[0]
        ok = np.asarray(valid[:n_cols]) != 0
        pad = -(-n_cols // TILE) * TILE
        self.ok = np.zeros(pad, dtype=bool)
        self.ok[:n_cols] = ok
        self.n = int(ok.sum())
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.where(ok, ell.max(0), np.float32(0))
            d = (ell - m).astype(np.float32)  # one fp32 rounding
            e = np.exp(d.astype(np.float64)).astype(np.float32)  # the correctly rounded expf
        self.e = np.zeros((self.P, pad))
        self.e[:, :n_cols] = np.where(ok, e.astype(np.float64), 0.0)
        self.m = np.zeros(pad)
        self.m[:n_cols] = m.astype(np.float64)

    def sweep(self, w):
        """(R [P], F, bad) of one sweep at w, in the contract's order."""
        s = np.zeros(self.e.shape[1])
        for k in range(self.P):
            s = s + w[k] * self.e[k]  # product rounded, then the sum
        good = self.ok & (s > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(good, 1.0 / np.where(good, s, 1.0), 0.0)
            f = np.where(good, np.log(np.where(good, s, 1.0)) + self.m, 0.0)
        R = _tile_sums(self.e * inv)
        return R, float(_tile_sums(f)), int((self.ok & ~good).sum())


def fit(ell, valid, n_cols, tol=1e-4, max_iter=2000, updates=None):
    """The contract's fit.  updates=T: exactly T updates whatever the gap says
    (the state a device fit with `iterations` = T is compared with), converged
    then reporting gap <= tol at the final w.  Returns the state's fields plus
    `gaps` / `objectives`: pass j's values, those of w after j updates."""
    pr = _Problem(ell, valid, int(n_cols))
    P, n = pr.P, pr.n
    w = np.full(P, 1.0 / P)
    out = {"w": w, "objective": np.nan, "gap": np.nan, "objective_uniform": np.nan, "n": n,
           "iterations": 0, "converged": False, "degenerate": False, "gaps": [], "objectives": []}
    passes = (max_iter if updates is None else updates) + 1
    for j in range(passes):
        R, F, bad = pr.sweep(w)
        if n == 0 or bad:
            out["degenerate"] = True
            break
        g = R / float(n)
        out["objective"], out["gap"] = F / float(n), float(g.max() - 1.0)
        out["gaps"].append(out["gap"])
        out["objectives"].append(out["objective"])
        if j == 0:
            out["objective_uniform"] = out["objective"]
        hit = out["gap"] <= tol
        if hit and updates is None or j == passes - 1:
            out["converged"] = bool(hit)
            break
        w = w * g
        tot = 0.0
        for k in range(P):
            tot = tot + w[k]
        w = w / tot
        out["iterations"] += 1
    out["w"] = w
    return out


# ------------------------------------------------------ the independent solver
def objective(ell, valid, w):
    """f(w) in plain fp64 (np.logaddexp-free: max, exp, dot, log)."""
    ok = np.asarray(valid) != 0
    x = np.asarray(ell, dtype=np.float64)[:, ok]
    m = x.max(0)
    return float(np.mean(np.log(np.asarray(w, dtype=np.float64) @ np.exp(x - m)) + m))


def solve(ell, valid, gap=1e-9, max_iter=3000):
    """(w, f(w), achieved gap), independent of the contract's order and
    precision: P = 2 by bisection on f'(a), w = (a, 1 - a); else fp64 EM until
    max_k g_k - 1 <= gap (or max_iter: f(w) is then still a lower bound of the
    optimum, and the achieved gap says by how much at most)."""
    ok = np.asarray(valid) != 0
    x = np.asarray(ell, dtype=np.float64)[:, ok]
    P, n = x.shape
    p = np.exp(x - x.max(0))

    def grad(w):
        return (p / (w @ p)).mean(1)
    if P == 1:
        w = np.ones(1)
    elif P == 2:
        def slope(a):  # f'(a) along w = (a, 1 - a): decreasing in a
            return float(((p[0] - p[1]) / (a * p[0] + (1 - a) * p[1])).mean())
        lo, hi = 0.0, 1.0
        if slope(1.0 - 1e-300) >= 0:
            lo = hi = 1.0
        elif slope(1e-300) <= 0:
            lo = hi = 0.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if slope(mid) > 0:
                lo = mid
            else:
                hi = mid
        a = 0.5 * (lo + hi)
        w = np.array([a, 1.0 - a])
    else:
        w = np.full(P, 1.0 / P)
        for _ in range(max_iter):
            g = grad(w)
            if g.max() - 1.0 <= gap:
                break
            w = w * g
            w = w / w.sum()
    w = np.maximum(w, 1e-300)  # a boundary solution of the bisection: keep log finite
    return w, objective(ell, valid, w), float(grad(w).max() - 1.0)


# ------------------------------------------------------------------ the bounds
def eta(n, P):
    return 6 * U + (n + P) * 2.0 ** -52


def bound_w(T, n, P):
    return (T + 1) * eta(n, P)


def bound_objective(T, n, P, gap, obj):
    return 3 * U + bound_w(T, n, P) + (n + P) * 2.0 ** -52 * max(1.0, abs(obj))


def bound_gap(T, n, P, gap):
    return (1 + abs(gap)) * (eta(n, P) + bound_w(T, n, P))


def iteration_range(gaps, tol, n, P):
    """(lo, hi): the device's `iterations` lies in [lo, hi] — the reference's
    first pass with gap <= tol + bg and its first with gap <= tol - bg (bg at
    that pass); None where the trajectory never gets there."""
    lo = hi = None
    for j, g in enumerate(gaps):
        bg = bound_gap(j, n, P, g)
        if lo is None and g <= tol + bg:
            lo = j
        if hi is None and g <= tol - bg:
            hi = j
    return lo, hi


# ------------------------------------------------------------------- the cases
def make_case(P, N, C=5, seed=0, kind="graded", plant=True):
    """logp [P, N, C] fp32 and int64 labels [N].  kind: graded (voter k sees the
    label with strength growing in k), disjoint (voter k is an expert on the
    examples i % P == k, noise elsewhere), equal (the same strength).  With
    P >= 3 the last voter duplicates the one before it.  plant (N >= 37): an out-of-range
    label, a NaN, a +inf, an all -inf column, a voter that is -inf on every
    fifth example, an example only voter 0 covers."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, size=N).astype(np.int64)
    z = rng.standard_normal((P, N, C))
    hot = np.eye(C)[labels]
    if kind == "graded":
        strength = np.linspace(0.2, 2.5, P)[:, None, None]
    elif kind == "disjoint":
        strength = np.where((np.arange(N)[None, :] % P) == np.arange(P)[:, None], 4.0, 0.0)[..., None]
    else:
        strength = np.full((P, 1, 1), 1.0)
    z = z + strength * hot
    z = z - z.max(-1, keepdims=True)
    logp = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    if plant and N >= 37:
        labels[3] = C + 2
        labels[4] = -1
        logp[P // 2, 7, labels[7]] = np.nan
        logp[0, 9, labels[9]] = np.inf
        logp[:, 11, labels[11]] = -np.inf
        if P >= 2:
            logp[1, 15::5, :] = -np.inf          # -inf from one voter: legal, p = 0
            logp[1:, 13, labels[13]] = -np.inf   # only voter 0 covers example 13
    if P >= 3:
        logp[P - 1] = logp[P - 2]                # two identical voters
    return logp, labels
