"""Time one replica-exchange attempt (kernels.exchange_energy, exchange_decide,
exchange_swap: three launches, no host read) against the torch composition on
the same buffers: ((theta - prior)**2).double().sum(1), the decision on the
device with torch.rand, and theta2d[perm] plus a copy back.
Shapes: 8 x 2.8 M (mlp_mnist) and 8 x 33.5 M; theta alone is swapped, as the
samplers do (momentum 0: the SGD buffer is dead).  The temperatures are equal,
so every attempt is accepted on both sides: the swap moves 8 chains on even
attempts and 6 on odd ones, and both sides see both parities in turn.  HIP
events around each side, rounds alternating, the median of `--reps` after a
warm-up; the three launches are also timed one by one, and the bandwidth of a
stand-alone swap is computed from the chains ITS parity moves.

    python tools/exchange_timing.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from bayesdll_amd import kernels as K
    dev = torch.device("cuda:0")
    Kc, N, s2 = 8, 60000.0, 1.0
    for n1 in (2_800_000 - 2, 33_500_000 - 2):
        stride = (n1 + 3) // 4 * 4
        g = torch.Generator(device=dev).manual_seed(1)
        theta2d = torch.randn(Kc, stride, device=dev, generator=g)
        prior2d = torch.randn(Kc, stride, device=dev, generator=g)
        loss = torch.rand(Kc, device=dev, generator=g)
        beta = torch.full((Kc,), 0.5, dtype=torch.float64, device=dev)
        st = K.ExchangeState(Kc, dev)
        box = {"t": 0, "ws": None}
        kw = dict(chains=Kc, chain_groups=stride // 4, n=n1)

        def energy():
            box["ws"] = K.exchange_energy(theta2d.view(-1), prior2d.view(-1), **kw)

        def decide():
            K.exchange_decide(st, box["ws"], loss, beta, n=n1, n_data=N, sigma2=s2, attempt=box["t"])
            box["t"] += 1

        def swap():
            K.exchange_swap(st, [theta2d.view(-1)], chain_groups=stride // 4)

        def fused():
            energy()
            decide()
            swap()

        tt = {"t": 0}
        idx = torch.arange(Kc, device=dev)

        def composed():
            q = ((theta2d[:, :n1] - prior2d[:, :n1]) ** 2).double().sum(1)
            U = N * loss.double() + q / (2 * s2)
            par = tt["t"] % 2
            tt["t"] += 1
            lower = (idx % 2 == par) & (idx < Kc - 1)
            db = beta - beta.roll(-1)
            la = db * (U - U.roll(-1))
            acc = lower & (torch.log(torch.rand(Kc, dtype=torch.float64, device=dev)) < la)
            perm = torch.where(acc, idx + 1, torch.where(acc.roll(1), idx - 1, idx))
            theta2d.copy_(theta2d[perm])

        for f in (fused, composed, fused, composed):
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in ("fused", "torch", "energy", "decide", "swap")}
        swap_gbps, moved = [], {0: 2 * (Kc // 2), 1: 2 * ((Kc - 1) // 2)}
        by_parity = {0: [], 1: []}
        for r in range(args.reps):
            times["fused"].append(timed(fused))
            times["torch"].append(timed(composed))
            if r % 2:  # one untimed attempt: the stand-alone launches see the other parity
                fused()
                composed()
            parity = box["t"] % 2  # of the decision the stand-alone swap executes
            for nm, f in (("energy", energy), ("decide", decide), ("swap", swap)):
                times[nm].append(timed(f))
            # 8 B per element of a moved chain: read once, written once
            swap_gbps.append(8 * moved[parity] * stride / times["swap"][-1] / 1e6)
            by_parity[parity].append(times["swap"][-1])
        s = st.summary()
        rec = {"chains": Kc, "n": n1, "attempts": int(s["attempts"].sum()),
               "accepts": int(s["accepts"].sum())}
        for k, v in times.items():
            rec[f"{k}_ms"] = float(np.median(v))
            rec[f"{k}_spread_ms"] = float(np.max(v) - np.min(v))
        rec["energy_GBps"] = 8 * Kc * n1 / rec["energy_ms"] / 1e6  # theta and prior, read once
        rec["swap_GBps"] = float(np.median(swap_gbps))
        rec["swap_8_chains_ms"] = float(np.median(by_parity[0]))
        rec["swap_6_chains_ms"] = float(np.median(by_parity[1]))
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
