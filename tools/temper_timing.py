"""Timing and accuracy of the on-device temperature scaling,
one process, HIP events.

    python tools/temper_timing.py time
    python tools/temper_timing.py accuracy

time      per shape (groups, examples, classes) of log-probabilities: one fit
          sweep + update (`sweep`, max_iter = 1), one report, and a whole fit
          to convergence with its one host read (`fit`), against the two things
          a user can do without the unit: `host` — logp.cpu().numpy() and
          calibration.find_optimal_temperature (scipy BFGS) per group, the copy
          included — and `torch` — the same Newton iteration composed of torch
          ops on the device (log_softmax(beta z), the three sums, one .item()
          per iteration).  A last row draws the labels independently of
          groups 1..: their optimum is beyond T = 100 and they end at_bound.
          Rounds alternate between the sides; median with
          p10 / p90 over the rounds of the mean over `reps` calls.
accuracy  the largest error against the fp64 reference (tests/temper_ref.py)
          of one sweep's nll / d1 / d2 and of the fitted temperature, as a
          share of the derived bound.

Every phase runs under an alarm; a HIP error or an expired alarm ends the
process at once (nothing more is launched).  One JSON line per result."""
from __future__ import annotations

import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesdll_amd import calibration  # noqa: E402
from bayesdll_amd import kernels as K  # noqa: E402

# (groups, examples, classes, independent): independent — the labels are drawn from other
# rows than groups 1.. hold, whose optimum is then beyond T = 100 (they end at_bound)
SHAPES = ((1, 10000, 10, False), (1, 10000, 1000, False), (8, 10000, 1000, False),
          (8, 10000, 1000, True))


def _expired(_sig, _frm):
    sys.stderr.write("temper_timing: phase exceeded its time limit; stopping\n")
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


def make(G, N, Cn, dev, seed=5, independent=False):
    """Log-probabilities of N(0, 3^2) logits and labels drawn from them (the
    groups share the labels: group g is the same rows plus N(0, 0.1^2), as
    chains that agree), sharpened by 1.5 + 0.1 g (optima near T = 1.5 + 0.1 g)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    base = 3.0 * torch.randn(1, N, Cn, generator=g, device=dev)
    y = torch.multinomial(torch.softmax(base[0], -1), 1, generator=g).squeeze(-1)
    noise = torch.randn(G, N, Cn, generator=g, device=dev)
    rows = base + 0.1 * noise
    if independent:
        rows = torch.cat([rows[:1], 3.0 * noise[1:]])
    lp = torch.log_softmax(rows, -1)
    sharp = 1.5 + 0.1 * torch.arange(G, device=dev, dtype=torch.float32).view(G, 1, 1)
    return (sharp * lp).contiguous(), y.contiguous()


def torch_newton(z, y, rtol=1e-6, max_iter=32):
    """The update rule of bdl_temper_fit_update per group, composed of torch
    ops; one .item() per iteration and group."""
    out = []
    idx = y.view(-1, 1)
    for zg in z:
        beta = 1.0
        for _ in range(max_iter):
            lq = torch.log_softmax(beta * zg, -1)
            q = lq.exp()
            E = (q * zg).sum(-1)
            var = (q * zg * zg).sum(-1) - E * E
            d1 = (E - zg.gather(-1, idx).squeeze(-1)).mean()
            step = (d1 / var.mean()).item()
            nb = min(max(beta - step, beta / 4), 4 * beta)
            nb = min(max(nb, 0.01), 100.0)
            if abs(nb - beta) <= rtol * beta:
                break
            beta = nb
        out.append(1.0 / beta)
    return out


def host_fit(z, y):
    zh, yh = z.cpu().numpy(), y.cpu().numpy()
    return [float(calibration.find_optimal_temperature(yh, zg)[0][0]) for zg in zh]


def time_(args):
    dev = torch.device("cuda", 0)
    for G, N, Cn, independent in SHAPES:
        phase(args.limit)
        z, y = make(G, N, Cn, dev, independent=independent)
        tot = [None]

        def report():
            tot[0] = K.temper_report(z, y, 1.5, groups=G, totals=tot[0])

        sides = {"sweep": lambda: K.temper_fit(z, y, groups=G, max_iter=1),
                 "report": report,
                 "fit": lambda: K.temper_fit(z, y, groups=G).read(),
                 "torch": lambda: torch_newton(z, y)}
        for fn in sides.values():   # warm-up: allocator, workspace, code objects
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in sides}
        for r in range(args.rounds):
            order = list(sides) if r % 2 == 0 else list(sides)[::-1]
            for k in order:
                t[k].append(timed(sides[k], args.reps))
        host, host_t = [], [None]

        def host_side():
            host_t[0] = host_fit(z, y)

        for _ in range(2):          # seconds each: single calls, wall clock
            t0 = time.perf_counter()
            host_side()
            host.append((time.perf_counter() - t0) * 1e3)
        signal.alarm(0)
        rows = K.temper_fit(z, y, groups=G).read()
        mb = z.numel() * 4 / 1e6
        out = {"what": "time", "groups": G, "examples": N, "classes": Cn,
               "independent_labels": independent, "logp_mb": round(mb, 1),
               "rounds": args.rounds, "reps": args.reps,
               **{k: summary(v) for k, v in t.items()}, "host": summary(host),
               "iterations": [int(r["iterations"]) for r in rows],
               "converged": [bool(r["converged"]) for r in rows],
               "at_bound": [bool(r["at_bound"]) for r in rows],
               "temperature": [round(1.0 / float(r["beta"]), 6) for r in rows],
               "torch_temperature": [round(v, 6) for v in torch_newton(z, y)],
               "host_temperature": [round(v, 6) for v in host_t[0]],
               "fit_over_torch": round(float(np.median(t["fit"])) / float(np.median(t["torch"])), 4),
               "gb_per_s_sweep": round(mb / float(np.median(t["sweep"])), 1),
               "gb_per_s_report": round(mb / float(np.median(t["report"])), 1)}
        print(json.dumps(out), flush=True)


def accuracy(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import temper_ref as R
    dev = torch.device("cuda", 0)
    phase(args.limit)
    for G, N, Cn in ((1, 2000, 10), (1, 500, 1000), (1, 16, 8192)):
        z, y = make(G, N, Cn, dev, seed=11)
        zh, yh = z[0].cpu().numpy(), y.cpu().numpy()
        one = K.temper_fit(z, y, max_iter=1).read()[0]
        s = R.sweep_reference(zh, yh, 1.0)
        row = K.temper_fit(z, y).read()[0]
        fr = R.fit_reference(zh, yh)
        fit = {"beta": float(row["beta"])}
        res = {"what": "accuracy", "examples": N, "classes": Cn, "converged": bool(row["converged"]),
               "iterations": int(row["iterations"]),
               **{k: {"err": abs(float(one[k]) - s[k]), "bound": s[b],
                      "err_over_bound": abs(float(one[k]) - s[k]) / s[b]}
                  for k, b in (("nll", "b_nll"), ("d1", "b_d1"), ("d2", "b_d2"))},
               "temperature": {"err": abs(1.0 / fit["beta"] - fr["temperature"]),
                               "bound": R.bound_T(zh, yh, fit, 1e-6)}}
        print(json.dumps(res), flush=True)
    signal.alarm(0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["time", "accuracy"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=150, help="seconds per phase")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("temper_timing needs a HIP device")
    try:
        (time_ if args.what == "time" else accuracy)(args)
    except Exception as e:  # noqa: BLE001 - a HIP error: nothing more is launched
        sys.stderr.write(f"temper_timing: stopped after an error: {e}\n")
        os._exit(1)


if __name__ == "__main__":
    main()
