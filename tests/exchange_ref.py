"""Host reference of the replica-exchange unit (numpy only, no GPU): a literal
restatement of include/bdl_exchange.h.

Energy.  q_k = sum_{i < n} d_i^2 with d = theta - prior in fp32 (one rounding;
prior None: d = theta), squares and sums in fp64.  A chain is cut into tiles of
1024 elements.  IN-TILE order: thread t of 256 owns elements 1024*j + 4*t .. + 3
and adds its squares in element order from 0.0 (an element >= n adds +0.0);
the 64 lanes of a wave combine by the butterfly xor 32, 16, 8, 4, 2, 1 (both
partners form a + b, which is commutative, so every lane holds the same bits);
the four waves are added in wave order from wave 0's value.  CROSS-TILE order:
thread t of 256 adds the chain's partials t, t + 256, ... in ascending order
from 0.0; then the same butterfly and the same wave order.

Decision (attempt t, fp64): U_k = N * loss_k + q_k / (2 sigma2); pairs (i, i+1)
with i % 2 == t % 2; db = beta_i - beta_{i+1}; la = db * (U_i - U_{i+1}) -
(db * db) * var; u = (w + 0.5) * 2^-32 with w the first Philox4x32-10 word of
counter (i, chain0, s lo, s hi), s = 2^63 + t, key seed; accept iff everything
is finite and log(u) < la.  Bookkeeping as the header states it.
"""
import numpy as np

from philox_ref import philox4x32_10

TILE, BLOCK, MAX_CHAINS = 1024, 256, 64
STEP_BASE = 1 << 63
UP, DOWN = 1, 2
_LANE = np.arange(64)


def _block_sum(v):
    """[..., 256] fp64 thread values -> the workgroup's sum: the butterfly
    within each wave of 64, then the waves in order from wave 0's value."""
    v = v.reshape(v.shape[:-1] + (4, 64))
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ off]
    out = v[..., 0, 0]
    for w in (1, 2, 3):
        out = out + v[..., w, 0]
    return out


def energy_partials(theta2d, prior2d, n):
    """float64 [K, tiles]: the (chain, tile) partials.  theta2d / prior2d:
    float32 [K, stride]; only the first n elements of a chain are read."""
    K = theta2d.shape[0]
    tiles = (n + TILE - 1) // TILE
    with np.errstate(all="ignore"):
        d = theta2d[:, :n].astype(np.float32)
        if prior2d is not None:
            d = d - prior2d[:, :n].astype(np.float32)  # fp32, one rounding
        sq = np.zeros((K, tiles * TILE), dtype=np.float64)
        sq[:, :n] = d.astype(np.float64) * d.astype(np.float64)  # exact
        sq = sq.reshape(K, tiles, BLOCK, 4)
        th = np.zeros((K, tiles, BLOCK), dtype=np.float64)
        for c in range(4):
            th = th + sq[..., c]
        return _block_sum(th)


def energy_combine(partials):
    """float64 [K]: q_k from the partials in the cross-tile order."""
    K, tiles = partials.shape
    rows = (tiles + BLOCK - 1) // BLOCK
    with np.errstate(all="ignore"):
        p = np.zeros((K, rows * BLOCK), dtype=np.float64)
        p[:, :tiles] = partials
        p = p.reshape(K, rows, BLOCK)
        th = np.zeros((K, BLOCK), dtype=np.float64)
        for r in range(rows):
            th = th + p[:, r]
        return _block_sum(th)


def energy(theta2d, prior2d, n):
    return energy_combine(energy_partials(theta2d, prior2d, n))


def same_bits(a, b):
    """fp64 arrays equal as bit patterns; a NaN equals any NaN (the payload and
    sign of a propagated NaN are not part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())


def new_state(K):
    st = {"attempts": np.zeros(max(K - 1, 0), dtype=np.uint64),
          "accepts": np.zeros(max(K - 1, 0), dtype=np.uint64),
          "round_trips": np.zeros(K, dtype=np.uint64), "refused": 0,
          "partner": np.arange(K, dtype=np.int32), "replica": np.arange(K, dtype=np.int32),
          "direction": np.zeros(K, dtype=np.int32)}
    if K >= 2:
        st["direction"][0], st["direction"][K - 1] = UP, DOWN
    return st


def uniform(pair, seed, chain0, attempt):
    s = STEP_BASE + int(attempt)
    w = philox4x32_10(pair, chain0 & 0xFFFFFFFF, s & 0xFFFFFFFF, s >> 32,
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return (float(int(w)) + 0.5) * 2.0 ** -32


def log_accept(Ui, Uj, bi, bj, var):
    with np.errstate(all="ignore"):
        db = np.float64(bi) - np.float64(bj)
        return db * (np.float64(Ui) - np.float64(Uj)) - (db * db) * np.float64(var)


def decide(st, q, loss, beta, *, n_data, sigma2, var, seed, chain0, attempt):
    """One attempt on the state `st` (in place).  Returns per decided pair
    (i, log u, la): what the margin condition of the tests is about."""
    K = len(q)
    with np.errstate(all="ignore"):
        U = np.float64(n_data) * np.asarray(loss, dtype=np.float32).astype(np.float64) \
            + np.asarray(q, dtype=np.float64) / (2.0 * np.float64(sigma2))
    st["U"] = U
    st["partner"] = np.arange(K, dtype=np.int32)
    seen = []
    for i in range(int(attempt) % 2, K - 1, 2):
        la = log_accept(U[i], U[i + 1], beta[i], beta[i + 1], var)
        st["attempts"][i] += 1
        if not (np.isfinite(U[i]) and np.isfinite(U[i + 1]) and np.isfinite(la)):
            st["refused"] += 1
            continue
        lu = np.log(uniform(i, seed, chain0, attempt))
        seen.append((i, float(lu), float(la)))
        if lu < la:
            st["accepts"][i] += 1
            st["partner"][i], st["partner"][i + 1] = i + 1, i
            st["replica"][[i, i + 1]] = st["replica"][[i + 1, i]]
    if K >= 2:
        r0, r1 = st["replica"][0], st["replica"][K - 1]
        if st["direction"][r0] == DOWN:
            st["round_trips"][r0] += 1
        st["direction"][r0] = UP
        st["direction"][r1] = DOWN
    return seen


def margin_ok(lu, la):
    """The condition on a test input: a last-ulp difference between two fp64
    logs cannot flip the decision."""
    return abs(lu - la) > 1e-6 * max(1.0, abs(la))


def swap(vectors, partner):
    """The permuted copies of [K, stride] arrays: the rows of every accepted
    pair (partner[k] > k) change places, padding included."""
    out = [np.array(v, copy=True) for v in vectors]
    for k, p in enumerate(partner):
        if p > k:
            for v in out:
                v[[k, p]] = v[[p, k]]
    return out


# ---------------------------------------------------------------- test inputs
# (name, K, n1, stride): what the geometry table must reach is asserted in
# tests/test_exchange_host.py
GEOMETRY = [
    ("tiny", 2, 3, 4),              # a chain shorter than one float4
    ("one_tile", 2, 1024, 1024),    # exactly one tile, no padding, n1 % 4 == 0
    ("tail1", 5, 1025, 1028),       # two tiles, n1 % 4 == 1, padded slot
    ("tail2", 3, 2050, 2052),       # three tiles (a second trip at grid 2), n1 % 4 == 2
    ("tail3", 5, 5123, 5124),       # K * tiles = 30 items, n1 % 4 == 3
    ("single", 1, 1500, 1500),      # K = 1: no pair
    ("wide_pad", 2, 1021, 1032),    # padding wider than one group
    ("many_tiles", 2, 300000, 300000),  # 293 tiles: the cross-tile sum takes a second row
]


def make_vectors(name, K, n1, stride, seed=0):
    """(theta2d, prior2d) float32 [K, stride] of a geometry: N(0, 1) values,
    sentinel padding (1e30: a read of it would show), and for the shapes named
    below special values: 2^60, subnormals, a NaN chain."""
    rng = np.random.default_rng(seed + 1000 * K + n1)
    th = rng.standard_normal((K, stride)).astype(np.float32)
    pr = rng.standard_normal((K, stride)).astype(np.float32)
    th[:, n1:], pr[:, n1:] = 1e30, -1e30
    if name == "tail1":
        th[0, 7], pr[0, 7] = 2.0 ** 60, 0.0        # a 2^120 square among O(1) ones
        th[1, :n1], pr[1, :n1] = 1e-40, -2e-41     # fp32 subnormals: the difference is kept
        th[2, 1024] = np.nan                       # a NaN chain (the tail element)
    if name == "tail3":
        th[3, 5122] = np.float32(2.0 ** 60)
    return th, pr


# the decision inputs of the GPU tests: K = 5 slots, 64 consecutive attempts
DECIDE_K, DECIDE_ATTEMPTS, DECIDE_SEED, DECIDE_CHAIN0 = 5, 64, 20241, 7
DECIDE_BETA = 1.0 / np.array([1.0, 1.3, 1.7, 2.2, 3.0]) ** 2
DECIDE_N, DECIDE_SIGMA2 = 2048.0, 1.5
DECIDE_VARS = (0.0, 0.35)


def decide_inputs(attempt):
    """(q [5] float64, loss [5] float32) of one attempt: energies a few units
    apart, so that la is O(1) and both outcomes occur."""
    rng = np.random.default_rng(77 + attempt)
    q = rng.uniform(50.0, 60.0, DECIDE_K)
    loss = (0.7 + 1.5e-3 * rng.standard_normal(DECIDE_K)).astype(np.float32)
    return q, loss


NAN_ATTEMPTS = (64, 65)


def nan_inputs(attempt):
    """decide_inputs with a NaN energy in slot 1 (a pair of either parity
    holds it) and +inf in slot 4."""
    q, loss = decide_inputs(attempt)
    q[1], q[4] = np.nan, np.inf
    return q, loss
