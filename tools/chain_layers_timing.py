"""What does the per-tensor R-hat table cost (kernels.chain_diag_layers)?

Times bdl_chain_diag_layers with HIP events at K = 8 and K = 64 stacked chains
on moment vectors of 1 GiB each (far beyond the 256 MiB Infinity Cache), for a
ViT-L/32-shaped segment table (296 tensors, bayesdll_amd.shapes, every tensor
scaled to the chain slot) and for a table of ONE segment over the whole
vector, against two references on the same buffers:

  diag      bdl_chain_diag with no per-element output: it reads the same
            bytes, so it is the reference for "the table costs nothing extra";
  fallback  what a caller had to do before: chain_diag(want=("rhat",)), which
            writes the [n] vector, then per tensor the reductions of a row in
            torch (finite mask, count, max, argmax, sum, three threshold
            counts), and one host copy of the results.

Alternates the variants in one process (rounds of layers-296, layers-1, diag,
fallback, ...), reports the median and the spread of the rounds; one JSON line
per K.  bdl_chain_ess_layers runs the same traversal on the same bytes per
element (sM2, bM2) with less arithmetic; --ess times it too.

    python tools/chain_layers_timing.py [--bytes-per-vector 1073741824] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesdll_amd import _lib as L  # noqa: E402
from bayesdll_amd import kernels as K  # noqa: E402
from bayesdll_amd import shapes  # noqa: E402

THR = (1.01, 1.05, 1.1)


def timed(fn, reps):
    """Mean ms per call of `reps` back-to-back calls (HIP events on the launch stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def scaled_table(n, backbone="vit_l_32"):
    """(offset, numel) rows of the backbone's tensors scaled to n elements in
    all (each at least 1, the largest one takes up the rounding)."""
    sizes = np.array([int(np.prod(s)) for _, s in shapes.segments(backbone)[0]], dtype=np.float64)
    nums = np.maximum(1, np.floor(sizes * (n / sizes.sum()))).astype(np.int64)
    nums[int(np.argmax(nums))] += n - int(nums.sum())
    assert nums.min() >= 1 and int(nums.sum()) == n
    offs = np.concatenate([[0], np.cumsum(nums)[:-1]])
    return np.stack([offs, nums], axis=1)


def torch_rows(rhat, rows):
    """The fallback: a row's fields from the [n] rhat vector, per tensor."""
    out = []
    for o, m in rows:
        x = rhat[o:o + m]
        ok = torch.isfinite(x)
        v = torch.where(ok, x, torch.full_like(x, -1.0))
        out.append(torch.stack([ok.sum(), v.max(), v.argmax() + o,
                                torch.where(ok, x, torch.zeros_like(x)).sum(dtype=torch.float64),
                                (v > THR[0]).sum(), (v > THR[1]).sum(), (v > THR[2]).sum()]))
    return torch.stack(out).cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes-per-vector", type=int, default=1 << 30,
                    help="size of each stacked moment vector (all chains)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--chains", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--ess", action="store_true", help="also time bdl_chain_ess_layers")
    args = ap.parse_args()
    dev = torch.device("cuda")
    total = args.bytes_per_vector // 4
    for chains in args.chains:
        n = total // chains // 4 * 4 - 1            # an element tail; the slot is n + 1
        cg = (n + 3) // 4
        slot = 4 * cg
        g = torch.Generator(device=dev).manual_seed(chains)
        m1 = torch.randn(chains * slot, device=dev, generator=g)
        m2 = m1 * m1 + 0.01                         # raw second moment: var 0.01 + m1^2
        rows = scaled_table(n)
        seg_many = torch.from_numpy(rows).to(dev)
        seg_one = torch.tensor([[0, n]], dtype=torch.int64, device=dev)
        kw = dict(chains=chains, chain_groups=cg, n=n, var_mode=L.VAR_RAW_MOMENTS, ratio=1.25,
                  count=5)
        ek = dict(chains=chains, chain_groups=cg, n=n, samples=64, batches=8)
        host_rows = [(int(o), int(m)) for o, m in rows]
        variants = {
            "layers_296": lambda: K.chain_diag_layers(m1, m2, seg_many, **kw),
            "layers_1": lambda: K.chain_diag_layers(m1, m2, seg_one, **kw),
            "diag": lambda: K.chain_diag(m1, m2, want=(), **kw).summary,
            "fallback": lambda: torch_rows(K.chain_diag(m1, m2, want=("rhat",), **kw)["rhat"],
                                           host_rows),
        }
        if args.ess:   # two non-negative vectors as (sM2, bM2): the same bytes per element
            pos = m1.abs()
            variants["ess_layers_296"] = lambda: K.chain_ess_layers(m2, pos, seg_many, **ek)
            variants["ess"] = lambda: K.chain_ess(m2, pos, **ek).summary
        for fn in variants.values():   # warm every shape
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                t[k].append(timed(fn, 1 if k == "fallback" else args.reps))
        rec = {"chains": chains, "n_per_chain": n, "segments": len(rows),
               "smallest_tensor": int(rows[:, 1].min()), "largest_tensor": int(rows[:, 1].max()),
               "gib_read": round(8 * chains * n / 2 ** 30, 3)}
        for k, v in t.items():
            ms = statistics.median(v)
            rec[k] = {"ms": round(ms, 4), "min": round(min(v), 4), "max": round(max(v), 4),
                      "gbs": round(8 * chains * n / (ms * 1e-3) / 1e9, 1)}
        rec["layers_296_over_diag"] = round(rec["layers_296"]["ms"] / rec["diag"]["ms"], 3)
        rec["layers_296_over_layers_1"] = round(rec["layers_296"]["ms"] / rec["layers_1"]["ms"], 3)
        rec["fallback_over_layers_296"] = round(rec["fallback"]["ms"] / rec["layers_296"]["ms"], 1)
        print(json.dumps(rec), flush=True)
        del m1, m2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
