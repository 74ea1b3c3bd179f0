"""Timing of the fused pairwise-diversity sweep, one process,
HIP events.

    python tools/diversity_timing.py

Per shape (P voters, B examples, C classes): kernels.diversity on the [P, B, C]
rows against the torch composition on the same device tensors — softmax and
log_softmax, the broadcast argmax compare for disagree and both_wrong,
cdist(p=1) over the voters of every example for the total variation, one einsum
for the cross-entropy behind KL, the masks (non-finite examples, masked classes
and the unbounded pairs as a second einsum) and ONE host read of the stacked
[5, P, P] result.  The data are N(0, 3^2) logits with uniform labels, nothing
masked.  Rounds alternate between the two sides; median with p10 / p90 over the
rounds of the mean over `reps` calls, reps chosen per side so that a round
lasts about `--round_ms`.  `kernel` is the call as diversity() issues it per
batch (no host read), `kernel_read` adds the read of the totals.

The kernel's error is reported against the bound tests/diversity_ref.py derives
from the arithmetic contract, on the first `--check` examples of every shape
(the NumPy reference is slow): `max_err_over_bound` must stay below 1.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import diversity_ref as R  # noqa: E402
from bayesdll_amd import kernels as K  # noqa: E402

SHAPES = ((8, 512, 10), (8, 512, 1000), (64, 512, 1000))


def _expired(_sig, _frm):
    sys.stderr.write("diversity_timing: a shape exceeded its time limit; stopping\n")
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


def composition(x, y):
    """[5, P, P] fp64 on the host: disagree, both_wrong, kl_unbounded, tv_sum,
    kl_sum of the finite examples."""
    P, B, C = x.shape
    bad = (torch.isnan(x) | torch.isposinf(x)).any(-1) | ~torch.isfinite(x).any(-1)
    ok = ~bad.any(0)                                           # [B]
    masked = torch.isneginf(x)
    p = torch.softmax(x, -1)
    lp = torch.where(masked, torch.zeros_like(x), torch.log_softmax(x, -1))
    a = x.argmax(-1)                                           # [P, B]
    okf = ok.double()
    dis = ((a[:, None, :] != a[None, :, :]) & ok).sum(-1)
    w = (a != y[None, :]) & ok & (y >= 0)[None, :] & (y < C)[None, :]
    bw = (w[:, None, :] & w[None, :, :]).sum(-1)
    pb = p.transpose(0, 1)                                     # [B, P, C]
    tv = 0.5 * (torch.cdist(pb, pb, p=1).double() * okf[:, None, None]).sum(0)
    pw = p * ok[None, :, None]
    cross = torch.einsum("ibc,jbc->ij", pw, lp).double()       # sum_b sum_c p_i lp_j
    own = (pw * lp).sum((1, 2)).double()
    unb_b = torch.einsum("ibc,jbc->ijb", (~masked).float(), masked.float()) > 0
    unb = (unb_b & ok).sum(-1)
    kl = own[:, None] - cross
    out = torch.stack([dis.double(), bw.double(), unb.double(), tv, kl])
    return out.cpu().numpy()                                   # the one host read


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round_ms", type=float, default=200.0)
    ap.add_argument("--max_reps", type=int, default=50)
    ap.add_argument("--check", type=int, default=24, help="examples of the error check")
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("diversity_timing needs a HIP device")
    dev = torch.device("cuda", 0)
    signal.signal(signal.SIGALRM, _expired)
    try:
        for P, B, C in SHAPES:
            signal.alarm(args.limit)
            g = torch.Generator(device=dev).manual_seed(5)
            x = (3.0 * torch.randn(P, B, C, generator=g, device=dev)).contiguous()
            y = torch.randint(0, C, (B,), generator=g, device=dev)
            tot = [None]

            def kernel():
                tot[0] = K.diversity(x, y, totals=tot[0], reset=True)

            def kernel_read():
                kernel()
                tot[0].read()

            sides = {"composition": lambda: composition(x, y), "kernel": kernel,
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
            want, got = composition(x, y), tot[0].read()
            same = all(np.array_equal(want[i].astype(np.int64), got[f])
                       for i, f in enumerate(R.INTS))
            # the kernel against the derived bound, on a slice the reference can afford
            nb = min(args.check, B)
            xs, ys = x[:, :nb].contiguous(), y[:nb].contiguous()
            small = K.diversity(xs, ys).read()
            ref = R.reference(xs.cpu().numpy(), ys.cpu().numpy(), want_bound=True)
            signal.alarm(0)
            ratio = max(float((np.abs(small[f] - ref[f]) / np.maximum(ref["bound"][f], 1e-300)).max())
                        for f in R.SUMS)
            km, cm = float(np.median(t["kernel"])), float(np.median(t["composition"]))
            out = {"what": "time", "voters": P, "batch": B, "classes": C, "rounds": args.rounds,
                   "reps": reps, **{k: summary(v) for k, v in t.items()},
                   "kernel_over_composition": round(km / cm, 3), "same_integers": bool(same),
                   "composition_tv_max_rel_diff": float(
                       (np.abs(want[3] - got["tv_sum"]) / np.maximum(got["tv_sum"], 1e-30)).max()),
                   "max_err_over_bound": round(ratio, 4), "checked_examples": nb,
                   "grid": K.diversity_default_grid(P, B, C, dev),
                   "GB_per_s": round(K.diversity_bytes_per_example(P, C) * B / (km * 1e6), 1)}
            print(json.dumps(out), flush=True)
    except Exception as e:  # noqa: BLE001 - a HIP error: nothing more is launched
        sys.stderr.write(f"diversity_timing: stopped after an error: {e}\n")
        os._exit(1)


if __name__ == "__main__":
    main()
