#!/usr/bin/env python
"""Time kernels.fn_fold against the composition it replaces — torch.softmax into
a [K, P*C] tensor plus kernels.ess_fold on the same accumulators — in one
process with HIP events, the two alternating round by round.

    python tools/fn_timing.py [--rounds 15] [--reps 200] [--out FILE.json]

Prints one JSON line per shape: the median and range over the rounds of the
mean time per call in microseconds, and the ratio of the medians.  Every shape
is reported, also where the fused sweep loses."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((8, 256, 10), (64, 128, 10), (8, 512, 1000))
BATCH = 4


def timed(fn, reps):
    """Mean microseconds per call of reps calls between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for s in range(reps):
        fn(s)
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def main(argv=None):
    from bayesdll_amd import kernels as K
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fn_timing: needs a HIP device (a CPU run measures nothing)")
    rows = []
    for chains, probe, classes in SHAPES:
        n = probe * classes
        cg = (n + 3) // 4
        g = torch.Generator(device="cuda").manual_seed(chains + probe + classes)
        logits = 2.0 * torch.randn(chains, probe, classes, device="cuda", generator=g)
        acc = [{nm: torch.zeros(chains * 4 * cg, device="cuda") for nm in K.ESS_VECTORS}
               for _ in range(2)]
        assert 4 * cg == n   # these shapes fill their slot: [K, P*C] is the stacked layout
        probs = torch.empty(chains * n, device="cuda")
        probs3 = probs.view(chains, probe, classes)

        def fused(s, v=acc[0]):
            K.fn_fold(logits, v["bsum"], v["smean"], v["sM2"], v["bM2"], sample=s + 1,
                      batch=BATCH, chain_groups=cg)

        def composed(s, v=acc[1]):
            torch.softmax(logits, -1, out=probs3)
            K.ess_fold(probs, v["bsum"], v["smean"], v["sM2"], v["bM2"], chains=chains,
                       chain_groups=cg, n=n, sample=s + 1, batch=BATCH)

        for fn in (fused, composed):   # warm-up: code objects, every flag set of a batch
            timed(fn, 2 * BATCH)
        t = {"fused": [], "composed": []}
        for _ in range(args.rounds):
            t["fused"].append(timed(fused, args.reps))
            t["composed"].append(timed(composed, args.reps))
        row = {"chains": chains, "probe": probe, "classes": classes, "rounds": args.rounds,
               "reps": args.reps}
        for k, v in t.items():
            row[k + "_us"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        row["fused_over_composed"] = row["fused_us"]["median"] / row["composed_us"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
