"""bdl_chain_step with K equal rows against the uniform stacked bdl_sgmcmc_step
launch on the same buffers: HIP-event times on one MI355X.

    python tools/chain_step_timing.py [--rounds 7] [--reps 20] [--sizes 8x33554432,64x2803210]

One process, the two launches alternating round by round (each round times
`reps` back-to-back launches of one kind between two events after a warm-up
launch), so drift hits both alike.  Per size and per instance (the cSGHMC
explore step and the Welford collect): the uniform launch at the library's
default geometry, then the per-chain launch for every blocks_per_chain of the
sweep.  Prints one JSON line per measurement: median ms over the rounds, the
spread (max - min) / median, algorithmic GB/s and the ratio to the uniform
launch.  Values are not checked here (tests/test_gpu_chain_step.py does).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesdll_amd import _lib as L  # noqa: E402
from bayesdll_amd import kernels as K  # noqa: E402

DEV = torch.device("cuda", 0)
ROW = dict(lrs=(1e-3, 1e-3), noise_scale=(1e-4, 1e-4), one_minus_alpha=0.82, prior_sig=0.8)


def states(K_, n1):
    stride = (n1 + 3) // 4 * 4
    n = K_ * stride
    v = {nm: torch.randn(n, device=DEV) * 1e-2 for nm in ("theta", "grad", "mom", "m1", "m2")}
    pad = [[(k + 1) * stride, L.ATTR_SKIP] for k in range(K_)] if stride > n1 else None
    rows = []
    for k in range(K_):
        rows.append([k * stride + n1, L.ATTR_PRIOR])
        if pad:
            rows.append(pad[k])
    if not pad:  # equal attributes on both sides of every seam: one run
        rows = [[n, L.ATTR_PRIOR]]
    runs = torch.tensor(rows, dtype=torch.int64, device=DEV)
    nf = torch.zeros(K_, dtype=torch.int32, device=DEV)
    uni = SimpleNamespace(theta=v["theta"], grad=v["grad"], gbase=None, mom=v["mom"], prior=None,
                          noise=None, runs=runs, nruns=len(rows), n=n, device=DEV, nonfinite=nf,
                          timer=None, chain_groups=stride // 4)
    cruns = torch.tensor([[n1, L.ATTR_PRIOR]], dtype=torch.int64, device=DEV)
    per = SimpleNamespace(theta=v["theta"], grad=v["grad"], mom=v["mom"], prior=None, noise=None,
                          nonfinite=nf, K=K_, n1=n1, chain_groups=stride // 4, chain_runs=cruns,
                          chain_nruns=1, chain_gbase=None, timer=None)
    sc = torch.tensor([[ROW["lrs"][0], ROW["lrs"][1], ROW["noise_scale"][0], ROW["noise_scale"][1],
                        ROW["one_minus_alpha"], ROW["prior_sig"], 1, 1, 0, 1, 1, 0]] * K_,
                      dtype=torch.float32, device=DEV)
    return uni, per, sc, v


def timed(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="8x33554432,64x2803210")
    ap.add_argument("--bpc", default="")
    a = ap.parse_args()
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    for size in a.sizes.split(","):
        K_, n1 = (int(x) for x in size.split("x"))
        uni, per, sc, v = states(K_, n1)
        base = max(1, -(-cus // K_))
        bpcs = [int(x) for x in a.bpc.split(",")] if a.bpc else \
            sorted({base, 2 * base, 3 * base, 4 * base, 8 * base})
        for name, noise, ckw, bpe in (
                ("explore", L.NOISE_NONE, {}, 20),
                ("welford", L.NOISE_PHILOX, dict(collect=L.COLLECT_WELFORD, mom1=v["m1"],
                                                 mom2=v["m2"], collect_a=3.0), 36)):
            key = dict(seed=1, chain=0, step=5)
            launch = {"uniform": lambda: K.sgmcmc_step(uni, L.CSGHMC, noise_mode=noise, **ROW,
                                                       **ckw, **key)}
            for b in bpcs:
                launch[f"bpc{b}"] = (lambda b=b: K.chain_step(
                    per, L.CSGHMC, scalars=sc, noise_mode=noise, blocks_per_chain=b, **ckw, **key))
            ms = {nm: [] for nm in launch}
            for _ in range(a.rounds):
                for nm, fn in launch.items():
                    ms[nm].append(timed(fn, a.reps))
            ref = float(np.median(ms["uniform"]))
            for nm, t in ms.items():
                med = float(np.median(t))
                print(json.dumps({"K": K_, "n1": n1, "instance": name, "launch": nm,
                                  "ms": round(med, 4),
                                  "spread": round((max(t) - min(t)) / med, 4),
                                  "gbs": round(bpe * K_ * n1 / med / 1e6, 1),
                                  "ratio_to_uniform": round(med / ref, 4)}), flush=True)
        del uni, per, sc, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
