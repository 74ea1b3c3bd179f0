"""How fast is the cross-chain diagnostic sweep (kernels.chain_diag)?

Times bdl_chain_diag with HIP events at K = 8 and K = 64 stacked chains on
moment vectors of 1 GiB each (far beyond the 256 MiB Infinity Cache), for
R-hat alone and for all three outputs, at each workgroups-per-CU setting, and
next to it the library's arithmetic-free access mix (bdl_stream_mix) over the
same two stacked buffers: the ceiling convention of DESIGN.md §4.

The mix has no instance with 2 K read streams (its widest reads 7), so the
ceiling here is its most read-heavy instance, (2 reads, 1 write), sweeping the
stacked mom1 and mom2 end to end into a scratch vector of the same length,
compared in GB/s of algorithmic bytes: the same bytes read from the same
memory, as two long streams instead of 2 K streams a chain slot apart, and
one third of the traffic written instead of 4 / (8 K + 4).  `of_ceiling` below
1 therefore shows what the K-stream access pattern and the per-element
arithmetic cost against a plain streaming read of the same buffers.

Alternates the two kernels in one process (rounds of diag, mix, diag, ...),
reports the median of the rounds; one JSON line per configuration.

    python tools/chain_diag_timing.py [--bytes-per-vector 1073741824] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes-per-vector", type=int, default=1 << 30,
                    help="size of each stacked moment vector (all chains)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--chains", type=int, nargs="+", default=[8, 64])
    args = ap.parse_args()
    dev = torch.device("cuda")
    total = args.bytes_per_vector // 4
    for chains in args.chains:
        n = total // chains // 4 * 4 - 1            # an element tail; the slot is n + 1
        cg = (n + 3) // 4
        slot = 4 * cg
        g = torch.Generator(device=dev).manual_seed(chains)
        m1 = torch.randn(chains * slot, device=dev, generator=g)
        # raw second moment: var 0.01 + m1^2
        m2 = m1 * m1 + 0.01
        scratch = torch.empty_like(m1)
        kw = dict(chains=chains, chain_groups=cg, n=n, var_mode=L.VAR_RAW_MOMENTS, ratio=1.25,
                  count=5)
        mixes = {(b, u): (lambda b=b, u=u: K.stream_mix([m1, m2], [scratch], blocks_per_cu=b,
                                                        unroll=u))
                 for b in (1, 2, 4, 8) for u in (1, 4)}
        diags = {(w, b): (lambda w=w, b=b: K.chain_diag(m1, m2, want=w, blocks_per_cu=b, **kw))
                 for w in (("rhat",), K.DIAG_OUTPUTS) for b in (1, 2, 4, 8)}
        for fn in list(mixes.values()) + list(diags.values()):   # warm every shape
            fn()
        torch.cuda.synchronize()
        tm = {k: [] for k in mixes}
        td = {k: [] for k in diags}
        for _ in range(args.rounds):
            for k, fn in diags.items():
                td[k].append(timed(fn, args.reps))
            for k, fn in mixes.items():
                tm[k].append(timed(fn, args.reps))
        mix_ms = {k: statistics.median(v) for k, v in tm.items()}
        best_mix = min(mix_ms, key=mix_ms.get)
        mix_gbs = 12 * chains * slot / (mix_ms[best_mix] * 1e-3) / 1e9
        for (w, b), v in td.items():
            ms = statistics.median(v)
            gbs = K.diag_bytes_per_elem(chains, len(w)) * n / (ms * 1e-3) / 1e9
            print(json.dumps({
                "chains": chains, "n_per_chain": n, "outputs": len(w), "blocks_per_cu": b,
                "ms": round(ms, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                "gbs": round(gbs, 1), "mix_2r1w_ms": round(mix_ms[best_mix], 4),
                "mix_geometry": list(best_mix), "mix_gbs": round(mix_gbs, 1),
                "of_ceiling": round(gbs / mix_gbs, 3)}), flush=True)
        del m1, m2, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
