"""Host bookkeeping of the batch-means effective sample size (include/bdl_ess.h).

Nothing here touches a device: from a sample's 1-based index and the batch
length come the fold's flags and its three scalars, from the counters the
report's, and from the raw device summary the dict `ess()` returns.  The
launches are kernels.ess_fold / kernels.chain_ess; the stacked samplers drive
them (stacked._StackedSampler.ess).

Batch means.  With S samples of a chain split into nb = S // b batches of b
consecutive samples, s^2 the sample variance and vb the sample variance of
the batch means, the variance of the chain's mean is estimated by vb / nb and
the effective sample size by nb * s^2 / vb = S * s^2 / (b * vb).  For
independent samples vb is about s^2 / b and ESS is about S; with positive
autocorrelation vb is larger and ESS smaller.  b must be several
autocorrelation times long for the estimate to be honest, and nb large enough
(tens) for vb to be stable: a small b overstates ESS.
"""
from __future__ import annotations

import math

FIRST_SAMPLE, FIRST_IN_BATCH, CLOSE, FIRST_BATCH = 0x1, 0x2, 0x4, 0x8  # bdl_ess_flag
MAX_COUNT = 1 << 24  # counters are handed to the device as exact fp32 values
DEFAULT_THRESHOLDS = (100.0, 400.0, 1000.0)


def check_batch(b, what="ess_batch"):
    """An integer >= 0 (0: the feature is off), below MAX_COUNT."""
    try:
        ok = int(b) == b and 0 <= int(b) < MAX_COUNT
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what} must be an integer >= 0 and < 2^24 (got {b!r})")
    return int(b)


def fold_plan(s, b):
    """(flags, fs, fb, c) of folding sample `s` (1-based index in its
    component) with batch length `b`: the bdl_ess_flag bits, s and b as the
    float64 values ctypes rounds to fp32 (exact below 2^24), and i / (i - 1)
    formed in float64 for the batch i = s / b a CLOSE ends (1.0 where the fold
    does not use it: no close, or the first batch's)."""
    s, b = int(s), int(b)
    if not 1 <= b < MAX_COUNT:
        raise ValueError(f"ess: batch must be in [1, 2^24) (got {b})")
    if not 1 <= s < MAX_COUNT:
        raise ValueError(f"ess: sample index must be in [1, 2^24) (got {s})")
    p = (s - 1) % b + 1
    flags = ((FIRST_SAMPLE if s == 1 else 0) | (FIRST_IN_BATCH if p == 1 else 0)
             | (CLOSE if p == b else 0) | (FIRST_BATCH if s == b else 0))
    c = 1.0
    if flags & CLOSE and not flags & FIRST_BATCH:
        i = s // b
        c = i / (i - 1)
    return flags, float(s), float(b), c


def fold_bytes_per_elem(flags):
    """Algorithmic HBM bytes per element of one fold with these flags: theta
    read; smean and sM2 written, and read unless FIRST_SAMPLE; bsum read
    unless FIRST_IN_BATCH and written unless CLOSE; bM2 written on a CLOSE and
    read unless FIRST_BATCH."""
    b = 4
    b += 8 if flags & FIRST_SAMPLE else 16
    b += 0 if flags & FIRST_IN_BATCH else 4
    if flags & CLOSE:
        b += 4 if flags & FIRST_BATCH else 8
    else:
        b += 4
    return b


def report_bytes_per_elem(chains, outputs):
    """Algorithmic HBM bytes per evaluated element of one report sweep: every
    chain's sM2 and bM2 read once, 4 B per requested output vector written."""
    return 8 * int(chains) + 4 * int(outputs)


def counts(samples, b):
    """(S, nb): samples folded per chain and batches closed."""
    return int(samples), int(samples) // int(b)


def check_report(samples, b):
    """Raise ValueError unless the report is defined: something folded and at
    least two batches closed.  The message names the counts."""
    S, nb = counts(samples, b)
    if S == 0:
        raise ValueError(f"ess: nothing is folded yet (0 samples, batches of {b})")
    if nb < 2:
        raise ValueError(f"ess: {S} sample{'s' if S != 1 else ''} folded per chain close {nb} "
                         f"batch{'es' if nb != 1 else ''} of {b}; the variance of the batch "
                         "means needs at least 2 closed batches")
    return S, nb


def thresholds(t=None):
    """Three finite ESS thresholds (default 100 / 400 / 1000)."""
    t = DEFAULT_THRESHOLDS if t is None else tuple(float(v) for v in t)
    if len(t) != 3 or not all(math.isfinite(v) for v in t):
        raise ValueError(f"ess: thresholds must be three finite numbers (got {t!r})")
    return t


def summary_dict(raw, thr, *, samples, batches, batch, chains):
    """The returned summary from the device struct's fields (`raw`: a mapping
    with n_eval, n_degenerate, n_nonfinite, argmin, n_below, ess_sum,
    ess_min)."""
    ne = int(raw["n_eval"])
    below = [int(v) for v in raw["n_below"]]
    return {"n_eval": ne, "n_degenerate": int(raw["n_degenerate"]),
            "n_nonfinite": int(raw["n_nonfinite"]), "argmin": int(raw["argmin"]),
            "ess_min": float(raw["ess_min"]), "ess_sum": float(raw["ess_sum"]),
            "ess_mean": float(raw["ess_sum"]) / ne if ne else float("nan"),
            "n_below": below, "share_below": [v / ne if ne else float("nan") for v in below],
            "thresholds": list(thr), "samples": int(samples), "batches": int(batches),
            "batch": int(batch), "chains": int(chains)}
