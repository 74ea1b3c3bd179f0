"""Timing and accuracy of the fused predictive sweep, one
process, HIP events.

    python tools/predict_timing.py time
    python tools/predict_timing.py accuracy

time      per shape (members, batch, classes): kernels.predict on [M, B, C]
          logits against the composition it replaces on identical inputs —
          `_local_logprob`'s ops (log_softmax of every component, cat,
          logsumexp, - log M) plus evaluate()'s nll_loss / argmax and their two
          .item() reads.  Rounds alternate between the two; median with
          p10 / p90 over the rounds of the mean over `reps` calls.  `kernel` is
          the call as uncertainty() issues it per batch (no host read: the
          totals are read once per loader); `kernel_read` adds a host read of
          the totals to every call.  64 x 128 x 1000 (33 MB) stays in the
          256 MB Infinity Cache between calls; 160 x 512 x 1000 (328 MB) does
          not; 64 x 128 x 10 is launch-bound.
accuracy  the largest error against the fp64 reference (tests/predict_ref.py)
          of the kernel and of the torch fp32 composition on the same N(0, 3^2)
          logits, next to the derived bound.

Every phase runs under an alarm; a HIP error or an expired alarm ends the
process at once (nothing more is launched).  One JSON line per result."""
from __future__ import annotations

import argparse
import json
import math
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bayesdll_amd import kernels as K  # noqa: E402

SHAPES = ((64, 128, 1000), (160, 512, 1000), (64, 128, 10))
COMPONENT_CHAINS = 8  # the composition's list holds [8, B, C] tensors, as K = 8 chains give


def _expired(_sig, _frm):
    sys.stderr.write("predict_timing: phase exceeded its time limit; stopping\n")
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


def composition(comps, y):
    lp = torch.cat([F.log_softmax(c, dim=-1) for c in comps], 0)
    lp = lp.logsumexp(0) - math.log(lp.shape[0])
    return F.nll_loss(lp, y, reduction="sum").item(), lp.argmax(-1).ne(y).sum().item()


def time_(args):
    dev = torch.device("cuda", 0)
    for M, B, Cn in SHAPES:
        phase(args.limit)
        g = torch.Generator(device=dev).manual_seed(5)
        x = 3.0 * torch.randn(M, B, Cn, generator=g, device=dev)
        y = torch.randint(0, Cn, (B,), generator=g, device=dev)
        comps = list(x.view(M // COMPONENT_CHAINS, COMPONENT_CHAINS, B, Cn).unbind(0))
        tot = [None]

        def kernel():
            _, tot[0] = K.predict(x, y, totals=tot[0], want=())

        def kernel_read():
            kernel()
            tot[0].read()

        sides = {"composition": lambda: composition(comps, y), "kernel": kernel,
                 "kernel_read": kernel_read}
        for fn in sides.values():   # warm-up: allocator, workspace, code objects
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in sides}
        for r in range(args.rounds):
            order = list(sides) if r % 2 == 0 else list(sides)[::-1]
            for k in order:
                t[k].append(timed(sides[k], args.reps))
        signal.alarm(0)
        loss, err = composition(comps, y)
        row = tot[0].read()[0]
        out = {"what": "time", "members": M, "batch": B, "classes": Cn,
               "logits_mb": round(x.numel() * 4 / 1e6, 1), "rounds": args.rounds, "reps": args.reps,
               **{k: summary(v) for k, v in t.items()},
               "kernel_over_composition": round(float(np.median(t["kernel"]))
                                                / float(np.median(t["composition"])), 4),
               "same_error_count": int(row["n_wrong"]) * B == int(err) * int(row["n"]),
               "gb_per_s_kernel": round(x.numel() * 4 / 1e6 / float(np.median(t["kernel"])), 1)}
        print(json.dumps(out), flush=True)


def accuracy(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import predict_ref as R
    dev = torch.device("cuda", 0)
    phase(args.limit)
    for M, B, Cn in ((40, 130, 1000), (40, 130, 10), (8, 16, 8192)):
        rng = np.random.default_rng(11)
        x = (3.0 * rng.standard_normal((M, 1, B, Cn))).astype(np.float32)
        lab = rng.integers(0, Cn, size=B)
        r = R.reference(x, lab, 15)
        b = R.bound(r, lab)
        dx, dl = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
        outs, _ = K.predict(dx, dl, want=("logp", "nll"))
        lp = F.log_softmax(dx[:, 0], dim=-1).logsumexp(0) - math.log(M)
        tn = -lp.gather(-1, dl.view(-1, 1)).squeeze(-1)
        fin = np.isfinite(b["logp"][0])
        res = {"what": "accuracy", "members": M, "batch": B, "classes": Cn}
        for name, got_lp, got_nll in (("kernel", outs["logp"][0], outs["nll"][0]),
                                      ("torch_fp32", lp, tn)):
            e_lp = np.abs(got_lp.double().cpu().numpy() - r["logp"][0])
            e_nll = np.abs(got_nll.double().cpu().numpy() - r["nll"][0])
            res[name] = {"logp_max_err": float(e_lp[fin].max()), "nll_max_err": float(e_nll.max()),
                         "logp_max_err_over_bound": float((e_lp[fin] / b["logp"][0][fin]).max())}
        res["bound"] = {"logp_max": float(b["logp"][0][fin].max()), "nll_max": float(b["nll"].max())}
        print(json.dumps(res), flush=True)
    signal.alarm(0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["time", "accuracy"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per phase")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("predict_timing needs a HIP device")
    try:
        (time_ if args.what == "time" else accuracy)(args)
    except Exception as e:  # noqa: BLE001 - a HIP error: nothing more is launched
        sys.stderr.write(f"predict_timing: stopped after an error: {e}\n")
        os._exit(1)


if __name__ == "__main__":
    main()
