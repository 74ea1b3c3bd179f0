"""How fast is the per-chain clip (kernels.chain_clip)?

Part 1 — the sweeps at size.  Times bdl_chain_clip with HIP events at K = 8 and
K = 64 stacked chains over one stacked gradient of 1 GiB (far beyond the
256 MiB Infinity Cache), one segment per call, at several blocks_per_chain.
The call is three launches; its two sweeps are separated by the threshold:

  norm    max_norm = 1e30: no chain clips, every scale workgroup exits after
          one scalar read — the norm sweep, the finalize and an empty launch.
          4 B per element.
  scale   max_norm = 1e-7, below the 1e-6 in the coefficient's denominator:
          coef = max_norm / (norm + 1e-6) < 0.1 whatever the norm, so every
          chain clips call after call (any larger threshold settles at
          norm = max_norm - 1e-6, coef exactly 1, and stops clipping; the
          gradient decays to zero here, which costs the sweep nothing) — the
          time of that call minus the norm call's.  8 B per element, in place.

Next to them the library's arithmetic-free access mix (bdl_stream_mix) on the
same buffer.  The mix has no 1-read and no in-place instance (its leanest is
2 reads, 1 write), so it sweeps the gradient's two halves into a scratch
vector of half the length — 12 B per element of a half — and the comparison is
in GB/s of algorithmic bytes, the ceiling convention of DESIGN.md §4.

Part 2 — the small-network case the stacked path lives in: the mlp_mnist
tensor list, K chains, chain_clip (three launches) next to the torch
fallback (per tensor flatten(1).square().sum(1), the coefficient, then per
tensor mul_): wall time per call over a queue of calls, which is what the
host-bound stacked step pays.

Alternates the kernels in one process, reports the median of the rounds; one
JSON line per configuration.

    python tools/chain_clip_timing.py [--bytes 1073741824] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesdll_amd import kernels as K  # noqa: E402


NEVER, ALWAYS = 1e30, 1e-7  # max_norm: no chain clips / every chain clips, on every call


def timed(fn, reps):
    """Mean ms per call of `reps` back-to-back calls (HIP events on the launch stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(fn, reps):
    """Mean ms of wall time per call, queue drained before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def table(rows, dev):
    return torch.tensor(rows, dtype=torch.int64).to(dev)


def sweeps(args, dev):
    total = args.bytes // 4
    for chains in args.chains:
        n = total // chains // 4 * 4
        g = torch.randn(chains * n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        half = (chains * n) // 2 // 4 * 4
        scratch = torch.empty(half, device=dev)
        seg = table([[g.data_ptr(), n, n]], dev)
        ws = K.chain_clip_workspace(chains, dev)
        clips = {(m, b): (lambda m=m, b=b: K.chain_clip(seg, 1, chains, m, workspace=ws,
                                                        blocks_per_chain=b))
                 for m in (NEVER, ALWAYS) for b in args.blocks_per_chain}
        mixes = {(b, u): (lambda b=b, u=u: K.stream_mix([g[:half], g[half:2 * half]], [scratch],
                                                        blocks_per_cu=b, unroll=u))
                 for b in (1, 2, 4, 8) for u in (1, 4)}
        for fn in list(clips.values()) + list(mixes.values()):
            fn()
        torch.cuda.synchronize()
        tc, tm = {k: [] for k in clips}, {k: [] for k in mixes}
        for _ in range(args.rounds):
            for k, fn in clips.items():
                tc[k].append(timed(fn, args.reps))
            for k, fn in mixes.items():
                tm[k].append(timed(fn, args.reps))
        mix_ms = {k: statistics.median(v) for k, v in tm.items()}
        best = min(mix_ms, key=mix_ms.get)
        mix_gbs = 12 * half / (mix_ms[best] * 1e-3) / 1e9
        for b in args.blocks_per_chain:
            norm_ms = statistics.median(tc[(NEVER, b)])
            both_ms = statistics.median(tc[(ALWAYS, b)])
            scale_ms = both_ms - norm_ms
            ngbs = 4 * chains * n / (norm_ms * 1e-3) / 1e9
            sgbs = 8 * chains * n / (scale_ms * 1e-3) / 1e9
            print(json.dumps({
                "part": "sweeps", "chains": chains, "n_per_chain": n, "blocks_per_chain": b,
                "norm_ms": round(norm_ms, 4), "norm_gbs": round(ngbs, 1),
                "clipped_call_ms": round(both_ms, 4), "scale_ms": round(scale_ms, 4),
                "scale_gbs": round(sgbs, 1), "mix_2r1w_ms": round(mix_ms[best], 4),
                "mix_geometry": list(best), "mix_gbs": round(mix_gbs, 1),
                "norm_of_mix": round(ngbs / mix_gbs, 3), "scale_of_mix": round(sgbs / mix_gbs, 3)}),
                flush=True)
        del g, scratch
        torch.cuda.empty_cache()


def small_network(args, dev):
    from bayesdll_amd.backbones import backbone
    shapes = [tuple(p.shape) for p in backbone("mlp_mnist").parameters()]
    for chains in args.chains:
        grads = [torch.randn(chains, *s, device=dev) for s in shapes]
        seg = table([[g.data_ptr(), g[0].numel(), g[0].numel()] for g in grads], dev)
        ws = K.chain_clip_workspace(chains, dev)
        bpc = K.clip_blocks_per_chain(sum(g[0].numel() for g in grads), chains, dev)

        def fused(m):
            K.chain_clip(seg, len(grads), chains, m, workspace=ws, blocks_per_chain=bpc)

        def fallback(m):
            sq = torch.stack([g.flatten(1).square().sum(1) for g in grads]).sum(0)
            coef = (m / (sq.sqrt() + 1e-6)).clamp(max=1.0)
            for g in grads:
                g.mul_(coef.view(-1, *([1] * (g.dim() - 1))))

        for m in (NEVER, ALWAYS):
            fused(m)
            fallback(m)
        rec = {"part": "mlp_mnist", "chains": chains, "tensors": len(grads),
               "blocks_per_chain": bpc}
        for nm, m in (("unclipped", NEVER), ("clipped", ALWAYS)):
            tf, tt = [], []
            for _ in range(args.rounds):
                tf.append(wall(lambda: fused(m), 20))
                tt.append(wall(lambda: fallback(m), 20))
            a, b = statistics.median(tf), statistics.median(tt)
            rec.update({f"{nm}_chain_clip_ms": round(a, 4), f"{nm}_torch_ms": round(b, 4),
                        f"{nm}_torch_over_chain_clip": round(b / a, 2)})
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="size of the stacked gradient")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--chains", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--blocks-per-chain", type=int, nargs="+", default=[0, 32, 128, 512])
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    sweeps(args, dev)
    small_network(args, dev)


if __name__ == "__main__":
    main()
