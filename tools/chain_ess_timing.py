"""How fast are the two batch-means ESS sweeps (kernels.ess_fold, kernels.chain_ess)?

Times both with HIP events at K = 8 x 33,554,431 and K = 64 x 4,194,303
elements (1 GiB a stacked vector, far beyond the 256 MiB Infinity Cache) and,
next to them, the library's arithmetic-free access mix (bdl_stream_mix) over
the same buffers: the ceiling convention of DESIGN.md §4, compared in GB/s of
algorithmic bytes.

  * The fold is timed in its three steady kinds at b = 3 (mid-batch 28 B /
    element, a close 32 B, first in batch 24 B).  The mix has no (4 reads,
    3 writes) instance; the fold's ceiling is its (4, 2) instance — theta,
    smean, sM2 and bsum read, smean and sM2 written in place, 24 B / element.
  * The report is timed with no output and with both, against the (2, 1) mix
    over the stacked sM2 and bM2 (as tools/chain_diag_timing.py: two long
    streams instead of 2 K streams a chain slot apart).

Alternates the kernels in one process (rounds of fold, report, mix, ...) and
reports the median of the rounds; one JSON line per configuration.  With
--parts step it times a collect-heavy mlp_mnist StackedSGLD epoch (K = 8,
thin = 1: every step collects) with ess_batch off and on, alternating.

    python tools/chain_ess_timing.py [--rounds 7] [--parts sweeps step]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesdll_amd import kernels as K  # noqa: E402

SIZES = {8: 33_554_431, 64: 4_194_303}
FOLD_KINDS = {"mid": 5, "close": 6, "first_in_batch": 7}   # the sample index at b = 3


def timed(fn, reps):
    """Mean ms per call of `reps` back-to-back calls (HIP events on the launch stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def sweeps(args, dev):
    for chains in args.chains:
        n = SIZES.get(chains, (1 << 28) // chains - 1)
        cg = (n + 3) // 4
        slot = 4 * cg
        g = torch.Generator(device=dev).manual_seed(chains)
        theta = 0.02 + 1e-3 * torch.randn(chains * slot, device=dev, generator=g)
        v = {nm: torch.rand(chains * slot, device=dev, generator=g) * 1e-3 + 1e-4
             for nm in K.ESS_VECTORS}
        scratch = torch.empty_like(theta)
        lay = dict(chains=chains, chain_groups=cg, n=n)
        folds = {(kind, gb): (lambda s=s, gb=gb: K.ess_fold(
            theta, v["bsum"], v["smean"], v["sM2"], v["bM2"], sample=s, batch=3, grid_blocks=gb,
            **lay)) for kind, s in FOLD_KINDS.items() for gb in args.fold_grids}
        reports = {(w, gb): (lambda w=w, gb=gb: K.chain_ess(
            v["sM2"], v["bM2"], samples=300, batches=100, want=w, grid_blocks=gb, **lay))
            for w in ((), K.ESS_OUTPUTS) for gb in args.report_grids}
        geoms = [(b, u) for b in (1, 2, 4, 8) for u in (1, 4)]
        mix_fold = {k: (lambda k=k: K.stream_mix(
            [theta, v["smean"], v["sM2"], v["bsum"]], [v["smean"], v["sM2"]], blocks_per_cu=k[0],
            unroll=k[1])) for k in geoms}
        mix_rep = {k: (lambda k=k: K.stream_mix([v["sM2"], v["bM2"]], [scratch],
                                                blocks_per_cu=k[0], unroll=k[1])) for k in geoms}
        groups = (folds, reports, mix_fold, mix_rep)
        for grp in groups:                                  # warm every shape
            for fn in grp.values():
                fn()
        torch.cuda.synchronize()
        t = [{k: [] for k in grp} for grp in groups]
        for _ in range(args.rounds):
            for grp, tt in zip(groups, t):
                for k, fn in grp.items():
                    tt[k].append(timed(fn, args.reps))
        med = [{k: statistics.median(x) for k, x in tt.items()} for tt in t]
        ceil = {}
        for name, m, nbytes in (("fold", med[2], 24), ("report", med[3], 12)):
            best = min(m, key=m.get)
            ceil[name] = (best, m[best], nbytes * chains * slot / (m[best] * 1e-3) / 1e9)
        for (kind, gb), ms in med[0].items():
            flags = K.E.fold_plan(FOLD_KINDS[kind], 3)[0]
            gbs = K.ess_fold_bytes_per_elem(flags) * chains * n / (ms * 1e-3) / 1e9
            x = t[0][(kind, gb)]
            print(json.dumps({
                "sweep": "fold", "kind": kind, "chains": chains, "n_per_chain": n,
                "grid_blocks": gb, "bytes_per_elem": K.ess_fold_bytes_per_elem(flags),
                "ms": round(ms, 4), "ms_min": round(min(x), 4), "ms_max": round(max(x), 4),
                "gbs": round(gbs, 1), "mix_4r2w_ms": round(ceil["fold"][1], 4),
                "mix_geometry": list(ceil["fold"][0]), "mix_gbs": round(ceil["fold"][2], 1),
                "of_ceiling": round(gbs / ceil["fold"][2], 3)}), flush=True)
        for (w, gb), ms in med[1].items():
            gbs = K.ess_bytes_per_elem(chains, len(w)) * n / (ms * 1e-3) / 1e9
            x = t[1][(w, gb)]
            print(json.dumps({
                "sweep": "report", "outputs": len(w), "chains": chains, "n_per_chain": n,
                "grid_blocks": gb, "ms": round(ms, 4), "ms_min": round(min(x), 4),
                "ms_max": round(max(x), 4), "gbs": round(gbs, 1),
                "mix_2r1w_ms": round(ceil["report"][1], 4),
                "mix_geometry": list(ceil["report"][0]), "mix_gbs": round(ceil["report"][2], 1),
                "of_ceiling": round(gbs / ceil["report"][2], 3)}), flush=True)
        del theta, v, scratch, folds, reports, mix_fold, mix_rep, groups
        torch.cuda.empty_cache()


def step(args, dev):
    """Chain-steps per second of mlp_mnist StackedSGLD epochs in which every
    step collects, ess_batch off / on, alternating; K = 8."""
    from bayesdll_amd import stacked
    from bayesdll_amd.backbones import backbone
    from bayesdll_amd.run import SyntheticLoader
    chains, res = 8, {}
    for rnd in range(args.step_rounds):
        for b in (0, 16):
            a = SimpleNamespace(
                lr=1e-2, lr_head=1e-2, epochs=4, momentum=0.5, ND=2048, device=dev, seed=1,
                hparams={"prior_sig": 1.0, "Ninflate": 1.0, "nd": 1.0, "thin": 1, "nst": 2,
                         "bias": "informative", "burnin": 0})
            torch.manual_seed(0)
            S = stacked.StackedSGLD(backbone("mlp_mnist").to(dev), chains, a, init="reinit",
                                    graph=True, ess_batch=b)
            loader = SyntheticLoader(2048, (1, 28, 28), 10, 128, dev, 1)
            S.train_one_epoch(loader, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for ep in (1, 2, 3):
                S.train_one_epoch(loader, ep)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res.setdefault(b, []).append(1e3 * dt / (3 * len(loader)))
            S.release_graphs()
            del S
    print(json.dumps({"part": "step", "model": "mlp_mnist", "chains": chains,
                      **{f"ess_batch_{b}_ms_per_collect_step": [round(v, 4) for v in vs]
                         for b, vs in res.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--chains", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--fold-grids", type=int, nargs="+", default=[0, 128, 512],
                    help="workgroups per chain (0: the default)")
    ap.add_argument("--report-grids", type=int, nargs="+", default=[0, 256, 1024, 2048],
                    help="workgroups of the report sweep (0: the default)")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--parts", type=str, nargs="+", default=["sweeps", "step"])
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    for p in args.parts:
        {"sweeps": sweeps, "step": step}[p](args, dev)


if __name__ == "__main__":
    main()
