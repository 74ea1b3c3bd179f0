"""Time the on-device stacking fit (kernels.stack_fit) against the same EM
written as a torch composition on the same [P, N] score matrix with the same
iteration count, at 8 x 10,000 and 64 x 50,000.  Both sides
include their host reads: the kernel path reads the 4-byte converged flag once
per chunk of 128 iterations and the state once; the torch path reads its gap
once per 128 iterations and the weights once.  Wall time around a device
synchronisation, median of `--reps` alternating rounds after a warm-up.

    python tools/stacking_timing.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def torch_em(ell, tol, iters, check_every=128):
    """The same iteration in torch ops: fp32 exp of ell - max, fp64 sums."""
    P, N = ell.shape
    m = ell.max(0).values
    e = torch.exp(ell - m).double()
    w = torch.full((P,), 1.0 / P, dtype=torch.float64, device=ell.device)
    done = 0
    for it in range(iters + 1):
        s = w @ e
        g = (e / s).mean(1)
        gap = g.max() - 1.0
        if it % check_every == check_every - 1 and float(gap) <= tol:  # the host read
            break
        if it == iters:
            break
        w = w * g
        w = w / w.sum()
        done += 1
    obj = (torch.log(s) + m.double()).mean()
    return w.cpu(), float(obj), float(gap), done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import stacking_ref as R
    from bayesdll_amd import kernels as K
    dev = torch.device("cuda:0")
    for P, N in ((8, 10000), (64, 50000)):
        logp, y = R.make_case(P, N, kind="graded", seed=1, plant=False)
        ell_h, valid_h, _ = R.gather(logp, y)
        ell = torch.from_numpy(ell_h).to(dev)
        valid = torch.from_numpy(valid_h).to(dev)
        s = K.stack_fit(ell, valid, N).summary()
        iters = s["iterations"]
        # both sides run exactly `iters` updates: a tolerance no gap reaches
        def fused():
            return K.stack_fit(ell, valid, N, tol=0.0, max_iter=iters).summary()

        def composed():
            return torch_em(ell, 0.0, iters)
        for f in (fused, composed):
            f()
        times = {"fused": [], "torch": []}
        for _ in range(args.reps):
            for name, f in (("fused", fused), ("torch", composed)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t)
        a, b = fused(), composed()
        rec = {"voters": P, "examples": N, "iterations": iters, "converged": s["converged"],
               "gap": s["gap"],
               "fused_ms": 1e3 * float(np.median(times["fused"])),
               "torch_ms": 1e3 * float(np.median(times["torch"])),
               "fused_spread_ms": 1e3 * float(np.max(times["fused"]) - np.min(times["fused"])),
               "torch_spread_ms": 1e3 * float(np.max(times["torch"]) - np.min(times["torch"])),
               "w_diff": float(np.abs(a["weights"] - b[0].numpy()).max())}
        rec["fused_us_per_iteration"] = 1e3 * rec["fused_ms"] / (iters + 1)
        rec["torch_us_per_iteration"] = 1e3 * rec["torch_ms"] / (iters + 1)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
