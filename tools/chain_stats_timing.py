"""How fast is the statistics sweep (kernels.chain_stats), and what does it
cost the step it sits in front of?

Part 1 — the sweep at size.  Times bdl_chain_stats with HIP events at K = 8
and K = 64 stacked chains over stacked vectors of 1 GiB each (far beyond the
256 MiB Infinity Cache), one segment, with three streams (gradient, theta,
momentum: 12 B per element) and four (plus the prior mean: 16 B), at several
blocks_per_chain.  Next to it, on the same buffers, the library's
arithmetic-free access mix (bdl_stream_mix at its best geometry: the
gradient's two halves read, a scratch vector of half the length written, 12 B
per element of a half) and bdl_chain_clip's norm sweep (a pure read, 4 B per
element), all in GB/s of algorithmic bytes — the convention of DESIGN.md §4e.

Part 2 — the stats + step pair.  The cSGHMC step launched right after the
sweep re-reads gradient, theta and momentum, so whether the sweep's 16-B loads
should be non-temporal is a measurement: the pair is timed with the library
as built (plain loads) and with a flavour built the other way (--alt-lib:
`make flavor F=stats_nt D=-DBDL_STATS_NT_LOADS` in bayesdll_amd/csrc), at the
mlp_mnist stacked size (K x 2.8 M elements, its tensor list as segments) and
at 1 GiB.

Part 3 — end to end: StackedCSGHMC on mlp_mnist under graph replay,
chain-steps/s with health_every 0, 10 and 1.

Alternates the variants in one process, reports the median of the rounds and
their spread (max - min) / median; one JSON line per configuration.

    python tools/chain_stats_timing.py [--bytes 1073741824] [--rounds 7] [--alt-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesdll_amd import _lib as L  # noqa: E402
from bayesdll_amd import kernels as K  # noqa: E402


def timed(fn, reps):
    """Mean ms per call of `reps` back-to-back calls (HIP events on the launch stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def med(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def table(rows, dev):
    return torch.tensor(rows, dtype=torch.int64).to(dev)


def rounds(fns, n, reps):
    """{key: [ms per round]} of the callables, alternating within every round."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            out[k].append(timed(fn, reps))
    return out


def sweeps(args, dev):
    total = args.bytes // 4
    gen = torch.Generator(device=dev).manual_seed(1)
    for chains in args.chains:
        n = total // chains // 4 * 4
        g, th, mv, pm = (torch.randn(chains * n, device=dev, generator=gen) for _ in range(4))
        half = (chains * n) // 2 // 4 * 4
        scratch = torch.empty(half, device=dev)
        seg = table([[g.data_ptr(), n, n, 0, 0]], dev)
        cseg = table([[g.data_ptr(), n, n]], dev)
        acc = torch.zeros(chains, 1, 6, dtype=torch.float64, device=dev)
        ws = K.chain_stats_workspace(chains, 1, dev)
        cws = K.chain_clip_workspace(chains, dev)
        fns = {("stats", s, b): (lambda s=s, b=b: K.chain_stats(
            seg, 1, chains, n // 4, th, acc, mom=mv, prior_mean=pm if s == 4 else None,
            lr=(0.05, 0.1), accumulate=True, workspace=ws, blocks_per_chain=b))
            for s in (3, 4) for b in args.blocks_per_chain}
        fns.update({("mix", b, u): (lambda b=b, u=u: K.stream_mix(
            [g[:half], g[half:2 * half]], [scratch], blocks_per_cu=b, unroll=u))
            for b in (1, 2, 4, 8) for u in (1, 4)})
        fns[("norm",)] = lambda: K.chain_clip(cseg, 1, chains, 1e30, workspace=cws)
        t = rounds(fns, args.rounds, args.reps)
        mix_key = min((k for k in t if k[0] == "mix"), key=lambda k: statistics.median(t[k]))
        mix_ms, mix_sp = med(t[mix_key])
        mix_gbs = 12 * half / (mix_ms * 1e-3) / 1e9
        norm_ms, norm_sp = med(t[("norm",)])
        norm_gbs = 4 * chains * n / (norm_ms * 1e-3) / 1e9
        for s in (3, 4):
            for b in args.blocks_per_chain:
                ms, sp = med(t[("stats", s, b)])
                gbs = 4 * s * chains * n / (ms * 1e-3) / 1e9
                print(json.dumps({
                    "part": "sweep", "chains": chains, "n_per_chain": n, "streams": s,
                    "blocks_per_chain": b, "ms": round(ms, 4), "spread": round(sp, 4),
                    "gbs": round(gbs, 1), "mix_ms": round(mix_ms, 4),
                    "mix_geometry": list(mix_key[1:]), "mix_gbs": round(mix_gbs, 1),
                    "mix_spread": round(mix_sp, 4), "norm_ms": round(norm_ms, 4),
                    "norm_gbs": round(norm_gbs, 1), "norm_spread": round(norm_sp, 4),
                    "of_mix": round(gbs / mix_gbs, 3), "of_norm": round(gbs / norm_gbs, 3)}),
                    flush=True)
        del g, th, mv, pm, scratch
        torch.cuda.empty_cache()


def stats_call(lib, seg, nseg, chains, cgroups, th, mv, g_acc, ws, bpc, dev):
    """A raw bdl_chain_stats call through `lib` (the built library or a flavour)."""
    a = L.StatsArgs()
    a.theta, a.mom, a.segments = th.data_ptr(), mv.data_ptr(), seg.data_ptr()
    a.acc, a.workspace = g_acc.data_ptr(), ws.data_ptr()
    a.chain_groups, a.nsegments, a.chains = cgroups, nseg, chains
    a.accumulate, a.blocks_per_chain = 1, bpc
    a.lr[0], a.lr[1] = 0.05, 0.1
    stream = L.current_stream_handle(dev)

    def call():
        L.check(lib.bdl_chain_stats(a, stream), "bdl_chain_stats")
    return call


def pair(args, dev):
    from bayesdll_amd.backbones import backbone
    from bayesdll_amd.flat import FlatState
    libs = {"built": L.lib()}
    if args.alt_lib:
        alt = C.CDLL(args.alt_lib)
        alt.bdl_chain_stats.restype, alt.bdl_chain_stats.argtypes = L.STATS_EXPORTS["bdl_chain_stats"]
        libs["alt"] = alt
    numels = [p.numel() for p in backbone("mlp_mnist").parameters()]
    cases = [("mlp_mnist", k, numels) for k in args.chains]
    cases.append(("1GiB", 8, [args.bytes // 4 // 8 // 4 * 4]))
    for name, chains, nums in cases:
        n1 = sum(nums)
        slot = (n1 + 3) // 4 * 4
        st = FlatState.from_segments([(f"c{k}", (slot,)) for k in range(chains)], "head",
                                     device=dev, need_mom=True)
        st.theta.normal_()
        st.grad.normal_().mul_(1e-3)
        offs = [sum(nums[:i]) for i in range(len(nums))]
        seg = table([[st.grad.data_ptr() + 4 * o, n, slot, o, 0] for o, n in zip(offs, nums)], dev)
        acc = torch.zeros(chains, len(nums), 6, dtype=torch.float64, device=dev)
        ws = K.chain_stats_workspace(chains, len(nums), dev)
        bpc = K.stats_blocks_per_chain(n1, chains, dev)

        def step():
            K.sgmcmc_step(st, L.CSGHMC, lrs=(1e-4, 1e-4), noise_scale=(0.0, 0.0),
                          noise_mode=L.NOISE_NONE, one_minus_alpha=0.9, prior_sig=1.0)

        fns = {"step": step}
        for nm, lib in libs.items():
            call = stats_call(lib, seg, len(nums), chains, slot // 4, st.theta, st.mom, acc, ws,
                              bpc, dev)
            fns["stats_" + nm] = call
            fns["pair_" + nm] = (lambda call=call: (call(), step()))
        t = rounds(fns, args.rounds, args.reps * 4)
        rec = {"part": "pair", "size": name, "chains": chains, "n_per_chain": n1,
               "segments": len(nums), "blocks_per_chain": bpc,
               "built_loads": "plain", "alt_loads": "non-temporal"}
        for k, v in t.items():
            m, sp = med(v)
            rec[k + "_ms"], rec[k + "_spread"] = round(m, 4), round(sp, 4)
        print(json.dumps(rec), flush=True)
        del st, acc, ws
        torch.cuda.empty_cache()


def end_to_end(args, dev):
    from bayesdll_amd import stacked
    from bayesdll_amd.backbones import backbone
    from bayesdll_amd.run import SyntheticLoader
    for chains in args.chains:
        res = {}
        for rnd in range(2):
            for he in (0, 10, 1):
                a = SimpleNamespace(
                    lr=1e-2, lr_head=1e-2, epochs=4, num_cycles=2, proportion_exploration=0.5,
                    ND=2048, device=dev, seed=1,
                    hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0, "nd": 1.0,
                             "thin": 10, "nst": 0, "bias": "informative", "burnin": 0})
                torch.manual_seed(0)
                S = stacked.StackedCSGHMC(backbone("mlp_mnist").to(dev), chains, a, init="reinit",
                                          graph=True, health_every=he)
                loader = SyntheticLoader(2048, (1, 28, 28), 10, 128, dev, 1)
                S.train_one_epoch(loader, 0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for ep in (1, 2, 3):
                    S.train_one_epoch(loader, ep)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res.setdefault(he, []).append(chains * 3 * len(loader) / dt)
                S.release_graphs()
                del S
        print(json.dumps({"part": "mlp_mnist", "chains": chains,
                          **{f"health_every_{he}_chain_steps_per_s": [round(v) for v in vs]
                             for he, vs in res.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="size of every stacked vector")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--chains", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--blocks-per-chain", type=int, nargs="+", default=[0, 32, 256])
    ap.add_argument("--alt-lib", type=str, default=None,
                    help="a flavour of the library built with non-temporal stats loads")
    ap.add_argument("--parts", type=str, nargs="+", default=["sweeps", "pair", "end_to_end"])
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    for p in args.parts:
        {"sweeps": sweeps, "pair": pair, "end_to_end": end_to_end}[p](args, dev)


if __name__ == "__main__":
    main()
