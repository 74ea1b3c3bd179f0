"""Timing of the all-pairs rank count, one process, HIP events.

    python tools/rank_timing.py

Per shape (groups G, 5 scores per group, n examples): kernels.rank on the
[5 G, n] score rows and the [G, n] marks against the torch composition on the
same device tensors — one batched sort of the rows, a gather of the marks, two
cumsums, two batched searchsorted for the ends of every tie run, the counts,
u2 / ap_sum / fp_at_tpr per row and ONE host read of the [5 G, 6] result, the
same integers the kernel reports (checked: `same_integers`).  Four scores are
continuous (ties are rare), the fifth takes 16 values like `disagree`; a fifth
of the examples are positives.  Rounds alternate between the two sides; median
with p10 / p90 over the rounds of the mean over `reps` calls, reps chosen per
side so that a round lasts about `--round_ms`.  `kernel` is the call as
detection() issues it (no host read), `kernel_read` adds the read of the
totals.  The count is O(n^2) per row and the composition O(n log n): the table
shows where the count loses.

Every shape runs under an alarm; a HIP error or an expired alarm ends the
process at once (nothing more is launched).  One JSON line per result."""
from __future__ import annotations

import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesdll_amd import kernels as K  # noqa: E402

SCORES = 5
SHAPES = tuple((g, n) for n in (20_000, 100_000, 200_000) for g in (1, 8))


def _expired(_sig, _frm):
    sys.stderr.write("rank_timing: a shape exceeded its time limit; stopping\n")
    os._exit(124)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(v):
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
            "p90_ms": round(float(np.percentile(v, 90)), 4)}


def composition(x, marks):
    """[rows, 6] int64 / fp64 on the host: n_pos, n_neg, u2, fp_at_tpr and
    ap_sum (as fp64 bits in an int64 column would hide it: returned apart).
    Every example is valid (marks 0 / 1, no NaN), as the timing data are."""
    rows, n = x.shape
    m = marks.repeat_interleave(rows // marks.shape[0], 0).to(torch.int64)
    xs, idx = torch.sort(x, dim=1)
    ms = m.gather(1, idx)
    zero = torch.zeros(rows, 1, dtype=torch.int64, device=x.device)
    cpos = torch.cat([zero, ms.cumsum(1)], 1)            # positives among the first k
    cneg = torch.cat([zero, (1 - ms).cumsum(1)], 1)
    lo = torch.searchsorted(xs, xs, right=False)         # the first of every tie run
    hi = torch.searchsorted(xs, xs, right=True)          # one past its last
    P, Nn = cpos[:, -1:], cneg[:, -1:]
    ge_pos, ge_neg = P - cpos.gather(1, lo), Nn - cneg.gather(1, lo)
    gt_neg = Nn - cneg.gather(1, hi)
    u2 = (ms * (2 * Nn - ge_neg - gt_neg)).sum(1)
    ap = (ms * (ge_pos.double() / (ge_pos + ge_neg).double())).sum(1)
    need = (P * 19 + 19) // 20
    fp = torch.where(ge_pos >= need, ge_neg, torch.full_like(ge_neg, n + 1)).amin(1)
    ints = torch.stack([P[:, 0], Nn[:, 0], u2, fp], 1)
    both = torch.cat([ints.double(), ap.unsqueeze(1)], 1).cpu().numpy()  # the one host read
    return both


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round_ms", type=float, default=300.0)
    ap.add_argument("--max_reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rank_timing needs a HIP device")
    dev = torch.device("cuda", 0)
    signal.signal(signal.SIGALRM, _expired)
    try:
        for G, n in SHAPES:
            signal.alarm(args.limit)
            g = torch.Generator(device=dev).manual_seed(5)
            x = torch.rand(G, SCORES, n, generator=g, device=dev)
            x[:, -1] = torch.randint(0, 16, (G, n), generator=g, device=dev).float()
            x = x.view(G * SCORES, n).contiguous()
            marks = (torch.rand(G, n, generator=g, device=dev) < 0.2).to(torch.int32).contiguous()
            res = [None]

            def kernel():
                res[0] = K.rank(x, marks, scores_per_group=SCORES)

            def kernel_read():
                kernel()
                res[0].read()

            sides = {"composition": lambda: composition(x, marks), "kernel": kernel,
                     "kernel_read": kernel_read}
            reps = {}
            for k, fn in sides.items():   # warm-up (allocator, workspace, code objects), then reps
                fn()
                torch.cuda.synchronize()
                reps[k] = int(min(args.max_reps, max(2, args.round_ms / max(timed(fn, 1), 1e-3))))
            t = {k: [] for k in sides}
            for r in range(args.rounds):
                order = list(sides) if r % 2 == 0 else list(sides)[::-1]
                for k in order:
                    t[k].append(timed(sides[k], reps[k]))
            signal.alarm(0)
            want = composition(x, marks)
            got = res[0].read()
            same = all(np.array_equal(want[:, i].astype(np.int64), got[f].astype(np.int64))
                       for i, f in enumerate(("n_pos", "n_neg", "u2", "fp_at_tpr")))
            ap_err = float(np.max(np.abs(want[:, 4] - got["ap_sum"]) / np.maximum(want[:, 0], 1)))
            km, cm = float(np.median(t["kernel"])), float(np.median(t["composition"]))
            out = {"what": "time", "groups": G, "scores": SCORES, "n": n, "rounds": args.rounds,
                   "reps": reps, **{k: summary(v) for k, v in t.items()},
                   "kernel_over_composition": round(km / cm, 3), "same_integers": bool(same),
                   "ap_max_err_over_P": ap_err,
                   "pair_compares_per_ns": round(3.0 * G * SCORES * n * n / (km * 1e6), 1)}
            print(json.dumps(out), flush=True)
    except Exception as e:  # noqa: BLE001 - a HIP error: nothing more is launched
        sys.stderr.write(f"rank_timing: stopped after an error: {e}\n")
        os._exit(1)


if __name__ == "__main__":
    main()
