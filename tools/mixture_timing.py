"""Timing of the likelihood pass and the weighted mixture, one
process, HIP events.

    python tools/mixture_timing.py

Per shape (members, batch, classes) of §4k — 64 x 128 x 10 (launch-bound),
64 x 128 x 1000 (33 MB: stays in the Infinity Cache between calls),
160 x 512 x 1000 (328 MB: does not) — with members = 8 components x draws x 8
chains:
  score    kernels.member_score on [members / 8, 8, B, C] logits (no host
           read: the scores are read once per cycle) against the torch
           composition per member — log_softmax, gather, sum — with the one
           .item() per batch a composed pass needs.
  mixture  kernels.mixture (by chain: groups = 8) against its composition —
           softmax per member, the mean over a component's draws, the weighted
           sum over the components, log.
Rounds alternate between the two sides; median with p10 / p90 over the rounds
of the mean over `reps` calls.  Every phase runs under an alarm; a HIP error or
an expired alarm ends the process at once (nothing more is launched).  One JSON
line per result."""
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
import torch.nn.functional as F  # noqa: E402

from bayesdll_amd import kernels as K  # noqa: E402

SHAPES = ((64, 128, 10), (64, 128, 1000), (160, 512, 1000))
CHAINS = 8


def _expired(_sig, _frm):
    sys.stderr.write("mixture_timing: phase exceeded its time limit; stopping\n")
    os._exit(124)


def phase(seconds):
    signal.signal(signal.SIGALRM, _expired)
    signal.alarm(int(seconds))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(v):
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
            "p90_ms": round(float(np.percentile(v, 90)), 4)}


def score_composition(x, y, acc):
    """x [members, K, B, C]: the loss sum of every member, one host read."""
    idx = y.view(1, -1, 1)
    for i in range(x.shape[0]):
        lp = F.log_softmax(x[i], dim=-1)
        acc[i] -= lp.gather(-1, idx.expand(x.shape[1], -1, 1)).squeeze(-1).double().sum(-1)
    return acc[0, 0].item()


def mixture_composition(x, w, draws):
    """x [comps * draws, K, B, C], w [comps, K] -> logp [K, B, C]."""
    p = torch.softmax(x, dim=-1)
    p = p.view(-1, draws, *p.shape[1:]).mean(1)
    return (w[:, :, None, None] * p).sum(0).log()


def alternate(sides, args):
    for fn in sides.values():   # warm-up: allocator, workspace, code objects
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for r in range(args.rounds):
        for k in (list(sides) if r % 2 == 0 else list(sides)[::-1]):
            t[k].append(timed(sides[k], args.reps))
    return t


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--draws", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds per phase")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mixture_timing needs a HIP device")
    dev = torch.device("cuda", 0)
    try:
        for M, B, Cn in SHAPES:
            phase(args.limit)
            g = torch.Generator(device=dev).manual_seed(5)
            x = 3.0 * torch.randn(M // CHAINS, CHAINS, B, Cn, generator=g, device=dev)
            y = torch.randint(0, Cn, (B,), generator=g, device=dev)
            comps = M // CHAINS // args.draws
            w = torch.rand(comps, CHAINS, generator=g, device=dev, dtype=torch.float64) + 0.1
            w /= w.sum(0, keepdim=True)
            acc = torch.zeros(M // CHAINS, CHAINS, dtype=torch.float64, device=dev)
            sc, tot = [None], [None]

            def k_score():
                sc[0] = K.member_score(x, y, groups=CHAINS, scores=sc[0])

            def k_mix():
                _, tot[0] = K.mixture(x, w, y, draws=args.draws, groups=CHAINS, totals=tot[0])

            ts = alternate({"composition": lambda: score_composition(x, y, acc),
                            "kernel": k_score}, args)
            tm = alternate({"composition": lambda: mixture_composition(x, w, args.draws),
                            "kernel": k_mix}, args)
            signal.alarm(0)
            mb = x.numel() * 4 / 1e6
            for what, t in (("score", ts), ("mixture", tm)):
                print(json.dumps({
                    "what": what, "members": M, "batch": B, "classes": Cn, "logits_mb": round(mb, 1),
                    "rounds": args.rounds, "reps": args.reps,
                    **{k: summary(v) for k, v in t.items()},
                    "kernel_over_composition": round(float(np.median(t["kernel"]))
                                                     / float(np.median(t["composition"])), 4),
                    "gb_per_s_kernel": round(mb / float(np.median(t["kernel"])), 1)}), flush=True)
    except Exception as e:  # noqa: BLE001 - a HIP error: nothing more is launched
        sys.stderr.write(f"mixture_timing: stopped after an error: {e}\n")
        os._exit(1)


if __name__ == "__main__":
    main()
