"""Timing of the bf16 compute mode, one process, HIP events.

    python tools/lowp_timing.py kernel [--alt-lib tools/bin/libbdl_plain_shadow.so]
    python tools/lowp_timing.py e2e

kernel  ViT-L/32 size (306,535,400 elements): the cSGHMC explore step (20 B per
        element) and the Welford-collect step (36 B) of bdl_lowp_step against
        bdl_sgmcmc_step on same-size buffers, every geometry of each kernel in
        every round, rounds alternating between the kernels; each kernel is
        reported at the best of its geometries (median over rounds, min - max).
        --alt-lib: a second build of the library in the same process (the
        plain-store flavour of the shadow store, `make flavor F=plain_shadow
        D=-DBDL_LOWP_PLAIN_SHADOW`), timed in the same rounds.
e2e     a ViT-L/32 cSGHMC step at batch 16, eager, synchronised per step, in
        fp32 and in bf16 (alternating rounds), with the forward/backward and
        the update timed apart.

Every phase runs under an alarm; a HIP error or an expired alarm ends the
process at once (nothing more is launched).  One JSON line per result."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesdll_amd import _lib as L  # noqa: E402
from bayesdll_amd import kernels as K  # noqa: E402

N_VIT = 306_535_400
FP32_GEOMETRIES = ((2, 1, 1), (1, 4, 1), (3, 1, 1), (1, 2, 1), (1, 1, 1))
LOWP_GEOMETRIES = ((2, 1), (1, 4), (3, 1), (1, 2), (1, 1), (2, 2), (2, 4))  # (wg / CU, unroll)


def _expired(_sig, _frm):
    sys.stderr.write("lowp_timing: phase exceeded its time limit; stopping\n")
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
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
            "max_ms": round(max(v), 4)}


def best(table):
    """table: {geometry: [ms per round]} -> (geometry, summary) of the lowest median."""
    g = min(table, key=lambda k: statistics.median(table[k]))
    return g, summary(table[g])


def kernel(args):
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = args.n
    f32 = dict(dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    vec = {k: torch.randn(n, generator=g, **f32) * s for k, s in
           (("theta", 0.05), ("mom", 0.01), ("m1", 0.05), ("m2", 0.01), ("grad", 0.1))}
    vec["m2"].abs_()
    g16 = vec["grad"].to(torch.bfloat16)
    shadow = torch.empty(n, dtype=torch.bfloat16, device=dev)
    runs = torch.tensor([[n, L.ATTR_PRIOR]], dtype=torch.int64, device=dev)
    base = dict(n=n, device=dev, theta=vec["theta"], mom=vec["mom"], prior=None, noise=None,
                gbase=None, runs=runs, nruns=1, timer=None,
                nonfinite=torch.zeros(1, dtype=torch.int32, device=dev))
    s32 = SimpleNamespace(grad=vec["grad"], **base)
    s16 = SimpleNamespace(grad=g16, shadow=shadow, **base)
    kinds = {
        "explore": dict(noise_mode=L.NOISE_NONE, collect=L.COLLECT_NONE),
        "collect": dict(noise_mode=L.NOISE_PHILOX, collect=L.COLLECT_WELFORD, mom1=vec["m1"],
                        mom2=vec["m2"], collect_a=5.0),
    }
    common = dict(lrs=(1e-6, 1e-6), noise_scale=(1e-6, 1e-6), one_minus_alpha=0.9,
                  prior_sig=1e-3, seed=7, chain=0)
    alt = None
    if args.alt_lib:
        alt = C.CDLL(os.path.abspath(args.alt_lib))
        alt.bdl_lowp_step.restype = C.c_int
        alt.bdl_lowp_step.argtypes = [C.POINTER(L.LowpArgs), C.c_void_p]
    stream = L.current_stream_handle(dev)
    for kind, kw in kinds.items():
        t32 = {gm: [] for gm in FP32_GEOMETRIES}
        t16 = {gm: [] for gm in LOWP_GEOMETRIES}
        talt = {gm: [] for gm in LOWP_GEOMETRIES}
        step = [0]

        def run32():
            step[0] += 1
            K.sgmcmc_step(s32, L.CSGHMC, step=step[0], **common, **kw)

        def run16(blocks, unroll, lib=None):
            step[0] += 1
            a = K.lowp_args(s16, L.CSGHMC, step=step[0], blocks=blocks, unroll=unroll,
                            **common, **kw)
            rc = (lib or L.lib()).bdl_lowp_step(a, stream)
            if rc != 0:
                raise RuntimeError(f"bdl_lowp_step status {rc}")

        for r in range(args.rounds):
            phase(args.limit)
            order = ("fp32", "bf16", "alt") if r % 2 == 0 else ("alt", "bf16", "fp32")
            for which in order:
                if which == "fp32":
                    for gm in FP32_GEOMETRIES:
                        K.set_launch_config(*gm)
                        t32[gm].append(timed(run32, args.reps))
                elif which == "bf16" or alt is not None:
                    lib, tab = (None, t16) if which == "bf16" else (alt, talt)
                    for gm in LOWP_GEOMETRIES:
                        tab[gm].append(timed(lambda: run16(gm[0] * cus, gm[1], lib), args.reps))
            signal.alarm(0)
        K.set_launch_config(*K.LIBRARY_DEFAULT)
        g32, b32 = best(t32)
        g16_, b16 = best(t16)
        out = {"what": "kernel", "kind": kind, "n": n, "rounds": args.rounds, "reps": args.reps,
               "fp32": {"geometry": list(g32), **b32}, "bf16": {"geometry": list(g16_), **b16},
               "ratio_bf16_over_fp32": round(b16["median_ms"] / b32["median_ms"], 4),
               "bf16_default_geometry": summary(t16[(2, 1)]),
               "bf16_all": {f"{a}x{b}": summary(v) for (a, b), v in t16.items()}}
        if alt is not None:
            ga, ba = best(talt)
            out["plain_shadow_store"] = {"geometry": list(ga), **ba,
                                         "same_geometry_as_bf16": summary(talt[g16_])}
        print(json.dumps(out), flush=True)


def e2e(args):
    from bayesdll_amd import backbones, csghmc
    dev = torch.device("cuda", 0)
    crit = torch.nn.CrossEntropyLoss()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(args.batch, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, 37, (args.batch,), generator=g).to(dev)
    sides = {}
    for name, cdt in (("fp32", None), ("bf16", torch.bfloat16)):
        phase(args.limit)
        torch.manual_seed(0)
        net = backbones.backbone("vit_l_32", num_classes=37).to(dev)
        net.train()
        model = csghmc.Model(ND=3680, prior_sig=1.0, momentum_decay=0.18)
        model.compute_dtype, model.graph, model.overlap = cdt, False, False
        sides[name] = dict(net=net, model=model, total=[], fb=[], upd=[])
        for _ in range(args.warmup):
            model(x, y, net, None, crit, [1e-4, 1e-4], 1.0, 0.01, should_sample=True)
        torch.cuda.synchronize()
        signal.alarm(0)

    def one(side):
        m, net = side["model"], side["net"]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        orig_fb = type(m).forward_backward

        def fb(st, net_, x_, y_, c_):
            ev[0].record()
            out = orig_fb(m, st, net_, x_, y_, c_)
            ev[1].record()
            return out
        m.forward_backward = fb
        m(x, y, net, None, crit, [1e-4, 1e-4], 1.0, 0.01, should_sample=True)
        ev[2].record()
        ev[2].synchronize()
        del m.forward_backward
        return ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    for r in range(args.rounds):
        phase(args.limit)
        for name in (("fp32", "bf16") if r % 2 == 0 else ("bf16", "fp32")):
            s = sides[name]
            ts = [one(s) for _ in range(args.steps)]
            for k, i in (("total", 0), ("fb", 1), ("upd", 2)):
                s[k].append(float(np.median([t[i] for t in ts])))
        signal.alarm(0)
    out = {"what": "e2e", "model": "vit_l_32", "batch": args.batch, "rounds": args.rounds,
           "steps_per_round": args.steps}
    for name, s in sides.items():
        out[name] = {"step": summary(s["total"]), "forward_backward": summary(s["fb"]),
                     "update": summary(s["upd"])}
    out["speedup"] = round(out["fp32"]["step"]["median_ms"] / out["bf16"]["step"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["kernel", "e2e"])
    ap.add_argument("--n", type=int, default=N_VIT)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--limit", type=int, default=120, help="seconds per phase")
    ap.add_argument("--alt-lib", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lowp_timing needs a HIP device")
    try:
        (kernel if args.what == "kernel" else e2e)(args)
    except Exception as e:  # noqa: BLE001 - a HIP error: nothing more is launched
        sys.stderr.write(f"lowp_timing: stopped after an error: {e}\n")
        os._exit(1)


if __name__ == "__main__":
    main()
