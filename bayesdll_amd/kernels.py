"""Python-side calls into the fused HIP kernels (libbdl_sgmcmc.so).

Every scalar is handed over as the float64 value the reference computes on
the host; ctypes rounds it to fp32 (round-to-nearest), which is exactly the
cast torch applies to a Python/NumPy scalar at an fp32 op.  Launches go on
torch's current HIP stream, so ordering with autograd is implicit and no host
synchronisation happens here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from . import ess as E

# Scalar-division rounding: "recip" = x * fl(1/s), what torch's HIP kernels do
# for a tensor / Python-scalar division (so a chain is bit-compatible with the
# reference sampler running on the same GPU) and ~22 % faster for the SGLD /
# SGHMC sweeps than a correctly rounded divide; "true" = x / s, torch CPU's
# rounding (the golden fixtures were generated on a CPU).
DIV_MODE = os.environ.get("BDL_DIV_MODE", "recip")


def _div_flag(div_mode=None):
    return L.FLAG_RECIP_DIV if (div_mode or DIV_MODE) == "recip" else 0


def _inv(s):
    """fl32(1/s) of the float64 divisor s: torch on a HIP device forms the
    reciprocal of a Python-scalar divisor in double and multiplies by it
    (tools/div_probe.py); ctypes does the final fp32 rounding."""
    s = float(s)
    return 1.0 / s if s != 0.0 else 0.0


def _step_args(state, method, *, lrs, noise_scale, noise_mode, one_minus_alpha=1.0,
               prior_sig=0.0, sigma2=1.0, n_data=1.0, mu=0.0, first_step=False,
               momentum=False, collect=L.COLLECT_NONE, mom1=None, mom2=None, collect_a=1.0,
               collect_b=1.0, seed=0, chain=0, step=0, div_mode=None, noise=None, grad_ready=False,
               mom_buf=None, philox_offset=0):
    a = L.StepArgs()
    a.theta = state.theta.data_ptr()
    g = getattr(state, "grad", None)
    a.grad = None if g is None else g.data_ptr()
    gb = getattr(state, "gbase", None)  # per-tensor gradients ("tensor" grad mode)
    a.grad_base = None if gb is None else gb.data_ptr()
    nf = getattr(state, "nonfinite", None)  # divergence flag (FlatState.nonfinite)
    a.nonfinite = None if nf is None else nf.data_ptr()
    mb = state.mom if mom_buf is None else mom_buf  # mom_buf: a separate SGD buffer
    a.mom = None if mb is None else mb.data_ptr()
    a.prior_mean = None if state.prior is None else state.prior.data_ptr()
    nz = noise if noise is not None else state.noise
    a.noise = None if nz is None else nz.data_ptr()
    a.mom1 = None if mom1 is None else mom1.data_ptr()
    a.mom2 = None if mom2 is None else mom2.data_ptr()
    a.runs = state.runs.data_ptr()
    a.nruns = state.nruns
    a.method = int(method)
    a.noise_mode = int(noise_mode)
    a.collect = int(collect)
    a.flags = ((L.FLAG_FIRST_STEP if first_step else 0) | (L.FLAG_MOMENTUM if momentum else 0)
               | (L.FLAG_GRAD_READY if grad_ready else 0) | _div_flag(div_mode))
    a.n = state.n
    a.lr[0], a.lr[1] = float(lrs[0]), float(lrs[1])
    a.noise_scale[0], a.noise_scale[1] = float(noise_scale[0]), float(noise_scale[1])
    a.one_minus_alpha = float(one_minus_alpha)
    a.prior_sig = float(prior_sig)
    a.sigma2 = float(sigma2)
    a.n_data = float(n_data)
    a.mu = float(mu)
    a.collect_a = float(collect_a)
    a.collect_b = float(collect_b)
    a.inv_sigma2, a.inv_n_data = _inv(sigma2), _inv(n_data)
    a.inv_collect_a, a.inv_collect_b = _inv(collect_a), _inv(collect_b)
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.chain = int(chain) & 0xFFFFFFFFFFFFFFFF
    a.step = int(step) & 0xFFFFFFFFFFFFFFFF
    a.philox_offset = int(philox_offset)
    a.chain_groups = int(getattr(state, "chain_groups", 0))  # stacked chains (StackedState)
    return a


def alg_bytes_per_elem(a, adam=None):
    """Algorithmic HBM bytes per element of one step launch: 4 B
    per vector read, 4 B per vector written, from the launch's own arguments."""
    grad_only = a.method in (L.SGHMC_GRAD, L.SGLD_GRAD, L.ADAM_SGHMC_GRAD)
    b = 4 + (0 if grad_only else 4)                      # theta r (+w)
    b += 4 + (4 if grad_only else 0)                     # grad r (+w)
    if a.method in (L.CSGHMC, L.SGHMC, L.SGHMC_GRAD, L.ADAM_SGHMC, L.ADAM_SGHMC_GRAD):
        b += 8                                           # momentum v r+w
    elif a.method == L.SGLD and a.flags & L.FLAG_MOMENTUM:
        b += 4 if a.flags & L.FLAG_FIRST_STEP else 8     # SGD buffer (w | r+w)
    if a.method != L.CSGHMC and a.prior_mean:
        b += 4                                           # theta0 r
    if a.noise_mode == L.NOISE_BUFFER:
        b += 4
    if adam is not None:
        b += 16                                          # Adam m, v r+w
        if adam.sgd_buf:
            b += 4 if a.flags & L.FLAG_FIRST_STEP else 8
    nmom = 2 if a.mom2 else 1
    if a.collect in (L.COLLECT_WELFORD, L.COLLECT_MEAN):
        b += 8 * nmom
    elif a.collect in (L.COLLECT_WELFORD_INIT, L.COLLECT_MEAN_INIT):
        b += 4 * nmom
    return b


def diag_bytes_per_elem(chains, outputs):
    """Algorithmic HBM bytes per evaluated element of one chain_diag sweep
    (DESIGN §4d): every chain's mom1 and mom2 read once, 4 B per requested
    output vector written."""
    return 8 * int(chains) + 4 * int(outputs)


class StepTimer:
    """Sampled HIP-event timing of the fused update launches (BDL_STEP_TIMING=k:
    every k-th launch), on the launch stream; summary() once per epoch gives
    launches, mean ms and algorithmic GB/s (expose step counters
    and GB/s).  Off by default; never synchronises per step."""

    def __init__(self, every):
        self.every, self.count, self.recs = max(1, int(every)), 0, []

    def begin(self):
        self.count += 1
        if (self.count - 1) % self.every:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return e0

    def end(self, e0, nbytes):
        if e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.recs.append((e0, e1, nbytes))

    def summary(self, reset=True):
        if not self.recs:
            return {"launches": self.count, "timed": 0}
        self.recs[-1][1].synchronize()
        ms = [a.elapsed_time(b) for a, b, _ in self.recs]
        gbs = [nb / (t * 1e-3) / 1e9 for t, (_, _, nb) in zip(ms, self.recs)]
        out = {"launches": self.count, "timed": len(ms), "avg_ms": sum(ms) / len(ms),
               "gbs": sum(gbs) / len(gbs)}
        if reset:
            self.count, self.recs = 0, []
        return out


def launch_kind(collect):
    """The geometry kind of a launch: "collect" for the steady-state moment
    updates (m1 / m2 read and written), "init" for a cycle's first collect
    (m1 / m2 only written), "step" otherwise; each is tuned on its own."""
    if collect in (L.COLLECT_WELFORD, L.COLLECT_MEAN):
        return "collect"
    if collect in (L.COLLECT_WELFORD_INIT, L.COLLECT_MEAN_INIT):
        return "init"
    return "step"


def _launch(state, fn, a, adam=None, written=None):
    kind = launch_kind(a.collect)
    pend = getattr(state, "_tune_pending", None)
    # a first step (SGD buffer written, not read) is not the steady-state
    # access mix: the kind stays pending until a later launch
    if pend and written is not None and int(a.n) == int(state.n) and kind in pend and \
            not (a.flags & L.FLAG_FIRST_STEP) and \
            not torch.cuda.is_current_stream_capturing():
        _tune_kind(state, fn, kind, written)
    _use_geometry(state, kind, sub=getattr(state, "bucket", False))
    t = getattr(state, "timer", None)
    e0 = t.begin() if t is not None else None
    fn()
    if e0 is not None:
        t.end(e0, alg_bytes_per_elem(a, adam) * int(a.n))


def _written(state, method, *, grad_only, mom, extra=(), mom1=None, mom2=None):
    """The vectors a full step launch writes (saved and restored while it is
    tuned on the state's own buffers), or None when they are not all flat
    vectors of the state (per-tensor gradients written by a *_GRAD method)."""
    if grad_only:
        if getattr(state, "grad", None) is None:
            return None
        out = [state.grad]
    else:
        out = [state.theta]
    out += [t for t in (mom,) + tuple(extra) + (mom1, mom2) if t is not None]
    return out


# the bf16 step's depth: two workgroups per CU x 4 groups per lane was the fastest of the
# seven geometries timed at ViT-L/32 size (tools/lowp_timing.py)
LOWP_UNROLL = 4


def lowp_args(state, method, *, blocks=0, unroll=LOWP_UNROLL, **kw):
    """bdl_lowp_args of one step over a bf16-compute state (FlatState with
    compute_dtype=torch.bfloat16, or any object with its vectors and a bf16
    `shadow`): the fields of _step_args, gradient and shadow in bf16."""
    if method not in (L.CSGHMC, L.SGHMC, L.SGLD):
        raise ValueError("bayesdll_amd: compute_dtype=bf16 covers the cSGHMC, SGHMC and SGLD "
                         "steps; the *_GRAD contract (the caller steps) and Adam have no bf16 form")
    if kw.get("grad_ready"):
        raise ValueError("bayesdll_amd: the bf16 step has no GRAD_READY form (no clipped step)")
    if kw.get("mom_buf") is not None:
        raise ValueError("bayesdll_amd: the bf16 step takes its SGD buffer from state.mom")
    s = _step_args(state, method, **kw)
    a = L.LowpArgs()
    for f in ("theta", "grad", "mom", "prior_mean", "noise", "mom1", "mom2", "runs", "grad_base",
              "nonfinite", "n", "nruns", "method", "noise_mode", "collect", "flags",
              "one_minus_alpha", "prior_sig", "sigma2", "n_data", "mu", "collect_a", "collect_b",
              "inv_sigma2", "inv_n_data", "inv_collect_a", "inv_collect_b", "seed", "chain",
              "step", "philox_offset", "chain_groups"):
        setattr(a, f, getattr(s, f))
    for i in range(2):
        a.lr[i], a.noise_scale[i] = s.lr[i], s.noise_scale[i]
    a.shadow = state.shadow.data_ptr()
    a.blocks, a.unroll = int(blocks), int(unroll)
    return a


def lowp_step(state, method, **kw):
    """One fused update over a bf16-compute state (bdl_lowp_step): bf16
    gradients read in place, fp32 theta / momentum / moments updated exactly as
    sgmcmc_step would on the upcast gradient, the bf16 shadow written in the
    same sweep.  Default geometry (no per-state tuning); blocks / unroll for
    tests and the timing tool.  Asynchronous."""
    a = lowp_args(state, method, **kw)
    t = getattr(state, "timer", None)
    e0 = t.begin() if t is not None else None
    L.check(L.lib().bdl_lowp_step(a, L.current_stream_handle(state.device)), "bdl_lowp_step")
    if e0 is not None:
        s = _step_args(state, method, **{k: v for k, v in kw.items()
                                         if k not in ("blocks", "unroll")})
        t.end(e0, alg_bytes_per_elem(s) * int(a.n))  # grad r 2 + shadow w 2 = the fp32 grad r 4


def lowp_shadow(theta, shadow):
    """shadow = bf16(theta), round to nearest even (bdl_lowp_shadow). Asynchronous."""
    if shadow.dtype != torch.bfloat16 or shadow.numel() != theta.numel():
        raise ValueError("lowp_shadow: shadow must be a bf16 tensor of theta's length")
    L.require_hip(theta, "theta")
    L.check(L.lib().bdl_lowp_shadow(theta.data_ptr(), shadow.data_ptr(), None, 0,
                                    int(theta.numel()), L.current_stream_handle(theta.device)),
            "bdl_lowp_shadow")


def sgmcmc_step(state, method, **kw):
    """One fused update over `state` (a FlatState). Asynchronous."""
    if getattr(state, "shadow", None) is not None:  # bf16 compute, fp32 chain state
        return lowp_step(state, method, **kw)
    a = _step_args(state, method, **kw)
    mb = kw.get("mom_buf")
    wr = _written(state, method, grad_only=method in (L.SGHMC_GRAD, L.SGLD_GRAD),
                  mom=state.mom if mb is None else mb,
                  mom1=kw.get("mom1") if kw.get("collect", L.COLLECT_NONE) else None,
                  mom2=kw.get("mom2") if kw.get("collect", L.COLLECT_NONE) else None)
    _launch(state, lambda: L.check(L.lib().bdl_sgmcmc_step(a, L.current_stream_handle(state.device)),
                                   "bdl_sgmcmc_step"), a, written=wr)


def sgmcmc_step_bare(state, **kw):
    """The cSGHMC step of these arguments with its arithmetic removed
    (bdl_sgmcmc_step_bare, include/bdl_measure.h): measurement only — the
    production kernel's own loop, loads and stores, at the launch
    configuration currently installed (set_launch_config; no tuning, no
    geometry switch).  theta / mom / steady-state moments keep their values.
    Asynchronous."""
    a = _step_args(state, L.CSGHMC, **kw)
    L.check(L.lib().bdl_sgmcmc_step_bare(a, L.current_stream_handle(state.device)),
            "bdl_sgmcmc_step_bare")


def last_order():
    """(order, slot) of this thread's last bdl_sgmcmc_step / _bare launch
    (include/bdl_order.h): 2 only where the launch ran the dynamic order on
    counter pair `slot`; a launch into a capture or a graph node reports 1."""
    slot = C.c_int32(-1)
    return int(L.lib().bdl_order_last(C.byref(slot))), int(slot.value)


def order_counters(device=None):
    """The dynamic order's {claim, done} counters of `device` after a device
    synchronize, [CLAIM_SLOTS, 2]: all zero between launches."""
    dev = _device(device)
    out = (C.c_uint32 * (2 * L.CLAIM_SLOTS))()
    L.check(L.lib().bdl_order_counters(int(dev.index or 0), out), "bdl_order_counters")
    return np.ctypeslib.as_array(out).reshape(L.CLAIM_SLOTS, 2).copy()


def sweep_drift(state, order, **kw):
    """One explore sweep of `state` under the drift probe (bdl_sweep_drift,
    include/bdl_order.h; measurement only, a real cSGHMC step without noise)
    at the installed workgroups/CU and depth, in sweep order `order`.  Returns
    the per-workgroup records as an int64 tensor [grid, DRIFT_WORDS] on the
    host: wall clock (100 MHz) at the first load and after the last store,
    samples taken, iterations run, then (wall clock, global iteration index)
    pairs at every DRIFT_EVERY-th iteration.  Synchronous."""
    a = _step_args(state, L.CSGHMC, noise_mode=L.NOISE_NONE, **kw)
    cap = 16 * 1024  # more workgroups than any launch geometry has
    rec = torch.zeros(cap, L.DRIFT_WORDS, dtype=torch.int64, device=state.device)
    grid = C.c_int32(0)
    L.check(L.lib().bdl_sweep_drift(a, int(order), rec.data_ptr(),
                                    rec.numel() * rec.element_size(), C.byref(grid),
                                    L.current_stream_handle(state.device)), "bdl_sweep_drift")
    torch.cuda.synchronize(state.device)
    return rec[:grid.value].cpu()


def drift_summary(rec, fractions=(0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875)):
    """tail_loss = 1 - sum(busy) / (workgroups x span) and, at each fraction of
    the launch's span, the spread (max - min over workgroups) of the global
    iteration index each workgroup last sampled, also in sweep rows (/ grid)."""
    rec = rec.numpy().astype(np.int64)
    t0, t1, ns = rec[:, 0], rec[:, 1], rec[:, 2]
    start, end = int(t0.min()), int(t1.max())
    span = end - start
    grid = rec.shape[0]
    out = {"workgroups": int(grid), "span_ticks": int(span),
           "iterations": int(rec[:, 3].sum()),
           "iterations_min_max": [int(rec[:, 3].min()), int(rec[:, 3].max())],
           "tail_loss": float(1.0 - (t1 - t0).sum() / (grid * span)),
           "ramp_loss": float((t0 - start).sum() / (grid * span)),
           "end_loss": float((end - t1).sum() / (grid * span)),
           "truncated": bool((rec[:, 3] > L.DRIFT_EVERY * L.DRIFT_SAMPLES).any()),
           "spread": []}
    ts, it = rec[:, 4::2], rec[:, 5::2]
    valid = np.arange(L.DRIFT_SAMPLES)[None, :] < ns[:, None]
    for f in fractions:
        T = start + f * span
        seen = valid & (ts <= T)
        have = seen.any(axis=1)
        last = np.where(seen, it, -1).max(axis=1)[have]
        sp = int(last.max() - last.min()) if last.size else 0
        out["spread"].append({"at": f, "iterations": sp, "rows": round(sp / grid, 2),
                              "workgroups_sampled": int(have.sum())})
    return out


def adam_step(state, method, *, adam_m, adam_v, sgd_buf=None, beta1, beta2, eps, t,
              momentum_decay, nd, temperature=1.0, grad_is_mom=False, lrs, noise_mode,
              sigma2, n_data, mu=0.0, first_step=False, momentum=False, collect=L.COLLECT_NONE,
              mom1=None, mom2=None, collect_a=1.0, collect_b=1.0, seed=0, chain=0, step=0,
              div_mode=None, noise=None, philox_offset=0):
    """One fused Adam-preconditioned SGHMC step (methods/adam_sghmc.py:500-553,
    adam_csghmc.py:812-860) + SGD step.  The host-side scalars are formed in
    float64 exactly as the reference's Python does (1 - beta1, 1 - beta1**t,
    2 * momentum_decay, 1 - momentum_decay); ctypes rounds them to fp32."""
    a = _step_args(state, method, lrs=lrs, noise_scale=(0.0, 0.0), noise_mode=noise_mode,
                   one_minus_alpha=1 - momentum_decay, sigma2=sigma2, n_data=n_data, mu=mu,
                   first_step=first_step, momentum=momentum, collect=collect, mom1=mom1,
                   mom2=mom2, collect_a=collect_a, collect_b=collect_b, seed=seed, chain=chain,
                   step=step, div_mode=div_mode, noise=noise, philox_offset=philox_offset)
    ad = L.AdamArgs()
    ad.adam_m = adam_m.data_ptr()
    ad.adam_v = adam_v.data_ptr()
    ad.sgd_buf = None if sgd_buf is None else sgd_buf.data_ptr()
    ad.beta1, ad.one_minus_beta1 = float(beta1), 1 - float(beta1)
    ad.beta2, ad.one_minus_beta2 = float(beta2), 1 - float(beta2)
    bc1, bc2 = 1 - float(beta1) ** int(t), 1 - float(beta2) ** int(t)
    ad.bias_corr1, ad.bias_corr2 = bc1, bc2
    ad.eps = float(eps)
    ad.two_alpha = 2 * float(momentum_decay)
    ad.nd = float(nd)
    ad.temperature = float(temperature)
    ad.inv_bias_corr1, ad.inv_bias_corr2 = _inv(bc1), _inv(bc2)
    ad.inv_temperature = _inv(temperature)
    ad.grad_is_mom = 1 if grad_is_mom else 0
    wr = _written(state, method, grad_only=method == L.ADAM_SGHMC_GRAD, mom=state.mom,
                  extra=(adam_m, adam_v) + ((sgd_buf,) if sgd_buf is not None else ()),
                  mom1=mom1 if collect != L.COLLECT_NONE else None,
                  mom2=mom2 if collect != L.COLLECT_NONE else None)
    _launch(state, lambda: L.check(L.lib().bdl_adam_step(a, ad, L.current_stream_handle(state.device)),
                                   "bdl_adam_step"), a, ad, written=wr)


def stream_mix(reads, writes, blocks_per_cu=1, unroll=4, schedule=L.MIX_BARE):
    """The bare access mix of a sweep over these buffers in one issue schedule
    (bdl_stream_mix_schedule, include/bdl_measure.h: L.MIX_BARE, MIX_PIPELINED,
    MIX_PACED): measurement only — the written tensors' contents are
    destroyed.  Asynchronous, on the current stream."""
    n = reads[0].numel()
    dev = reads[0].device
    rp = (C.c_void_p * len(reads))(*[t.data_ptr() for t in reads])
    wp = (C.c_void_p * len(writes))(*[t.data_ptr() for t in writes])
    L.check(L.lib().bdl_stream_mix_schedule(rp, len(reads), wp, len(writes), int(n),
                                            int(blocks_per_cu), int(unroll), int(schedule),
                                            L.current_stream_handle(dev)), "bdl_stream_mix")


def clip_workspace(state):
    """Device scratch for sgld_step_clipped: (total_norm, coef) then per-workgroup
    partial sums.  Cached on the FlatState."""
    ws = getattr(state, "_clip_ws", None)
    if ws is None:
        nbytes = int(L.lib().bdl_clip_workspace_bytes(int(state.n)))
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=state.device)
        state._clip_ws = ws
    return ws


def sgld_step_clipped(state, max_norm, **kw):
    """SGLD step with torch.nn.utils.clip_grad_norm_(max_norm) applied to the
    sampler gradient first (methods/csgld.py:250-253), all on device: a norm
    pass, a one-workgroup finalize and the update pass.  Returns the workspace
    whose first two floats are (total_norm, clip_coef)."""
    a = _step_args(state, L.SGLD, **kw)
    _use_geometry(state)
    ws = clip_workspace(state)
    L.check(L.lib().bdl_sgld_step_clipped(a, float(max_norm), ws.data_ptr(),
                                          L.current_stream_handle(state.device)),
            "bdl_sgld_step_clipped")
    return ws


def moments_update(theta, mom1, mom2, collect, collect_a=1.0, collect_b=1.0, div_mode=None):
    """Stand-alone posterior-moment update of flat vectors (no parameter update)."""
    L.require_hip(theta, "theta")
    a = L.MomentsArgs()
    a.theta, a.mom1 = theta.data_ptr(), mom1.data_ptr()
    a.mom2 = None if mom2 is None else mom2.data_ptr()
    a.n = theta.numel()
    a.collect = int(collect)
    a.flags = _div_flag(div_mode)
    a.collect_a, a.collect_b = float(collect_a), float(collect_b)
    a.inv_collect_a, a.inv_collect_b = _inv(collect_a), _inv(collect_b)
    L.check(L.lib().bdl_moments_update(a, L.current_stream_handle(theta.device)),
            "bdl_moments_update")


# (workgroups per CU, float4 groups per lane) tried for a vector's draw
SAMPLE_GEOMETRIES = ((1, 4), (2, 4), (3, 4), (4, 4), (4, 1), (6, 1))
SAMPLE_TUNE_MIN = 1 << 22          # smaller draws keep the default (2 x 4)
_SAMPLE_GEOM = {}                  # (device index, n) -> (workgroups per CU, unroll)


def sample_geometry(n, device):
    """The posterior draw's tuned (workgroups per CU, unroll) for an n-element
    vector on `device` (None until posterior_sample tuned it)."""
    return _SAMPLE_GEOM.get((torch.device(device).index, int(n)))


def _tune_sample(a, out):
    """Time the draw at each SAMPLE_GEOMETRIES entry with its own arguments
    (each launch writes the same values: same keys), keep the fastest.  Why:
    the bare access mix of the draw's buffers ranked 3 workgroups/CU x 4
    first at ViT-L/32 size and 4 x 1 at ResNet-101 size on one box (bench.py
    aux_kernels.posterior_sample.mix_ceiling, profiles/round4/methods/), and
    round 2's probes ranked 2 x 4 first on two others; in round 4's
    same-process A/Bs on ViT-L/32 draws 1 x 4 ran 0.587-0.600 ms against
    0.635-0.653 for the best of the others on three boxes
    (profiles/round4/philox_ab/)."""
    stream = L.current_stream_handle(out.device)
    ts = torch.cuda.current_stream(out.device)  # the stream the draws are launched on
    best = None
    for bpc, u in SAMPLE_GEOMETRIES:
        a.blocks_per_cu, a.unroll = bpc, u
        L.check(L.lib().bdl_posterior_sample(a, stream), "bdl_posterior_sample")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(ts)
        for _ in range(3):
            L.check(L.lib().bdl_posterior_sample(a, stream), "bdl_posterior_sample")
        ev[1].record(ts)
        ev[1].synchronize()
        ms = ev[0].elapsed_time(ev[1])
        if best is None or ms < best[0]:
            best = (ms, (bpc, u))
    return best[1]


def posterior_sample(out, mom1, mom2, *, var_mode, ratio=1.0, var_floor=1e-12, noise=None,
                     seed=0, chain=0, step=0, div_mode=None, chain_groups=0, geometry=None):
    """out = mom1 + sqrt(clamp(var(mom1, mom2), var_floor)) * eps (eps: buffer or Philox;
    chain_groups > 0: stacked chains keyed chain + k, bdl_sample_args.chain_groups).
    geometry: (workgroups per CU, unroll 1 or 4) of the launch; None = tuned
    once per device and size on the first draw of >= SAMPLE_TUNE_MIN elements
    (outside graph capture), 2 x 4 below.  Values never depend on it."""
    L.require_hip(out, "out")
    a = L.SampleArgs()
    a.out, a.mom1 = out.data_ptr(), mom1.data_ptr()
    a.mom2 = None if mom2 is None else mom2.data_ptr()
    a.noise = None if noise is None else noise.data_ptr()
    a.n = out.numel()
    a.var_mode = int(var_mode)
    a.noise_mode = L.NOISE_BUFFER if noise is not None else L.NOISE_PHILOX
    a.ratio = float(ratio)
    a.var_floor = float(var_floor)
    # WELFORD M2 / (n-1): torch-on-GPU multiplies by the reciprocal
    a.inv_ratio = _inv(ratio) if _div_flag(div_mode) else 0.0
    a.seed, a.chain, a.step = int(seed), int(chain), int(step) & 0xFFFFFFFFFFFFFFFF
    a.chain_groups = int(chain_groups)
    if geometry is None:
        key = (out.device.index, int(a.n))
        geometry = _SAMPLE_GEOM.get(key)
        if geometry is None and a.n >= SAMPLE_TUNE_MIN and \
                not torch.cuda.is_current_stream_capturing():
            geometry = _SAMPLE_GEOM[key] = _tune_sample(a, out)
    a.blocks_per_cu, a.unroll = (int(x) for x in (geometry or (0, 0)))
    L.check(L.lib().bdl_posterior_sample(a, L.current_stream_handle(out.device)),
            "bdl_posterior_sample")


DIAG_OUTPUTS = ("pooled_mean", "pooled_var", "rhat")
_SCRATCH = {}  # (kind, device index, ...) -> a cached device workspace


def _scratch(key, make):
    """The cached device workspace under `key`, made on first use."""
    ws = _SCRATCH.get(key)
    if ws is None:
        ws = _SCRATCH[key] = make()
    return ws


def _byte_scratch(kind, dev, nbytes):
    return _scratch((kind, dev.index),
                    lambda: torch.empty(int(nbytes()), dtype=torch.uint8, device=dev))


def _stacked_layout(what, vectors, chains, chain_groups, n, chains_error=None,
                    device_error="all vectors must be on one device"):
    """The checks every stacked diagnostic makes of its layout and vectors
    ((name, tensor) pairs): chains in range (chains_error(chains): the unit's
    own bound and text, else 1 .. ESS_MAX_CHAINS), 1 <= n <= 4 * chain_groups,
    each vector a contiguous HIP tensor that holds every chain's n elements,
    all on one device.  Returns (chains, chain_groups, n, device)."""
    chains, chain_groups, n = int(chains), int(chain_groups), int(n)
    if chains_error is not None:
        why = chains_error(chains)
        if why:
            raise ValueError(f"{what}: {why}")
    elif not 1 <= chains <= L.ESS_MAX_CHAINS:
        raise ValueError(f"{what}: 1 <= chains <= {L.ESS_MAX_CHAINS} is required")
    if not 1 <= n <= 4 * chain_groups:
        raise ValueError(f"{what}: 1 <= n <= 4 * chain_groups is required")
    need = 4 * chain_groups * (chains - 1) + n
    dev = None
    for nm, t in vectors:
        L.require_hip(t, nm)
        if not t.is_contiguous() or t.numel() < need:
            raise ValueError(f"{what}: {nm} must be contiguous with at least {need} elements")
        if dev is not None and t.device != dev:
            raise ValueError(f"{what}: {device_error}")
        dev = t.device
    return chains, chain_groups, n, dev


class _LazySummary(dict):
    """A stacked diagnostic's result: the requested output tensors by name and
    `summary`, read lazily — the first access copies the struct from the
    device (one D2H copy, one sync of the launch stream) and is cached.
    decode(raw bytes, thresholds) -> the summary dict."""

    def __init__(self, outs, ws, event, thresholds, decode):
        super().__init__(outs)
        self._ws, self._event, self._thresholds, self._summary = ws, event, thresholds, None
        self._decode = decode

    def __missing__(self, key):
        if key != "summary":
            raise KeyError(key)
        return self.summary

    @property
    def summary(self):
        if self._summary is None:
            self._event.synchronize()
            self._summary = self._decode(self._ws.cpu().numpy().tobytes(), self._thresholds)
            self._ws = None
        return self._summary


def _diag_summary(raw, thresholds):
    s = L.DiagSummary.from_buffer_copy(raw)
    ne = int(s.n_eval)
    above = [int(v) for v in s.n_above]
    return {"n_eval": ne, "n_degenerate": int(s.n_degenerate),
            "n_nonfinite": int(s.n_nonfinite), "argmax": int(s.argmax), "n_above": above,
            "rhat_sum": float(s.rhat_sum), "rhat_max": float(s.rhat_max),
            "rhat_mean": float(s.rhat_sum) / ne if ne else float("nan"),
            "share_above": [v / ne if ne else float("nan") for v in above],
            "thresholds": list(thresholds)}


class DiagResult(_LazySummary):
    """chain_diag's result (summary: bdl_diag_summary plus rhat_mean,
    share_above and `thresholds`)."""

    def __init__(self, outs, ws, event, thresholds):
        super().__init__(outs, ws, event, thresholds, _diag_summary)


def chain_diag(mom1, mom2, *, chains, chain_groups, n, var_mode, ratio, count, var_floor=1e-12,
               thresholds=(1.01, 1.05, 1.1), want=("rhat",), blocks_per_cu=0, div_mode=None):
    """Cross-chain R-hat and pooled posterior of `chains` stacked chains
    (bdl_chain_diag, include/bdl_diag.h): chain k's element j at
    4*chain_groups*k + j of mom1 / mom2, n elements per chain evaluated,
    (var_mode, ratio) as the posterior draw's, count = samples collected per
    chain.  want: any of DIAG_OUTPUTS — each an [n] tensor in the result;
    result["summary"] is read on first access.  One sweep and a one-workgroup
    combine on the current stream, no host synchronisation here.  Values never
    depend on blocks_per_cu (1-8, 0: default)."""
    if mom2 is None:
        raise ValueError("chain_diag: the second moment is required (mom2 is None)")
    if mom1 is None:
        raise ValueError("chain_diag: mom1 is required")
    L.require_hip(mom1, "mom1")
    L.require_hip(mom2, "mom2")
    if int(count) < 2:
        raise ValueError(f"chain_diag: R-hat needs at least 2 samples per chain (count = {count})")
    chains, chain_groups, n, dev = _stacked_layout(
        "chain_diag", (("mom1", mom1), ("mom2", mom2)), chains, chain_groups, n,
        chains_error=lambda k: f"at least 2 chains are required (chains = {k})" if k < 2 else None,
        device_error="mom1 and mom2 must be on one device")
    want = tuple(want)
    if len(thresholds) != 3 or any(w not in DIAG_OUTPUTS for w in want):
        raise ValueError(f"chain_diag: three thresholds, and want from {DIAG_OUTPUTS}")
    ws = _byte_scratch("diag", dev, lambda: L.lib().bdl_chain_diag_workspace_bytes(n))
    outs = {w: torch.empty(n, dtype=torch.float32, device=dev) for w in want}
    a = L.DiagArgs()
    a.mom1, a.mom2 = mom1.data_ptr(), mom2.data_ptr()
    a.pooled_mean, a.pooled_var, a.rhat = (
        outs[w].data_ptr() if w in outs else None for w in DIAG_OUTPUTS)
    a.workspace = ws.data_ptr()
    a.n, a.chain_groups, a.chains = n, chain_groups, chains
    a.var_mode = int(var_mode)
    a.ratio = float(ratio)
    # WELFORD M2 / (n-1): torch-on-GPU multiplies by the reciprocal (as posterior_sample)
    a.inv_ratio = _inv(ratio) if _div_flag(div_mode) else 0.0
    a.var_floor = float(var_floor)
    a.c1 = (int(count) - 1) / int(count)
    for i, t in enumerate(thresholds):
        a.thresholds[i] = float(t)
    a.blocks_per_cu = int(blocks_per_cu)
    L.check(L.lib().bdl_chain_diag(a, L.current_stream_handle(dev)), "bdl_chain_diag")
    # the struct leaves the shared workspace in stream order, so a later call
    # on this device cannot overwrite a summary that was not read yet
    snap = ws[:C.sizeof(L.DiagSummary)].clone()
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    return DiagResult(outs, snap, ev, thresholds)


ESS_OUTPUTS = ("ess", "mcse")
ESS_VECTORS = ("bsum", "smean", "sM2", "bM2")


def ess_fold_bytes_per_elem(flags):
    """Algorithmic HBM bytes per element of one ess_fold with these
    bdl_ess_flag bits: 24-32 outside a component's first sample."""
    return E.fold_bytes_per_elem(int(flags))


def ess_bytes_per_elem(chains, outputs):
    """Algorithmic HBM bytes per evaluated element of one chain_ess sweep."""
    return E.report_bytes_per_elem(chains, outputs)


def ess_fold(theta, bsum, smean, sM2, bM2, *, chains, chain_groups, n, sample, batch,
             grid_blocks=0):
    """Fold one collected sample of every chain into the batch-means
    accumulators (bdl_chain_ess_fold, include/bdl_ess.h): `sample` is its
    1-based index in the component, `batch` the batch length b; flags and
    scalars come from ess.fold_plan.  All vectors are stacked like theta
    (chain k, element j at 4*chain_groups*k + j); bsum may be None at b == 1.
    One launch on the current stream, no host synchronisation.  Values never
    depend on grid_blocks (workgroups per chain, 0: default).  Returns the
    flags."""
    flags, fs, fb, c = E.fold_plan(sample, batch)
    vecs = [("theta", theta), ("smean", smean), ("sM2", sM2), ("bM2", bM2)]
    if int(batch) > 1:
        if bsum is None:
            raise ValueError("ess_fold: bsum is required with batch > 1")
        vecs.append(("bsum", bsum))
    chains, chain_groups, n, dev = _stacked_layout("ess_fold", vecs, chains, chain_groups, n)
    a = L.EssFoldArgs()
    a.theta, a.smean, a.sM2, a.bM2 = (t.data_ptr() for t in (theta, smean, sM2, bM2))
    a.bsum = bsum.data_ptr() if int(batch) > 1 else None
    a.n, a.chain_groups, a.chains = n, chain_groups, chains
    a.sample, a.batch, a.flags = int(sample), int(batch), flags
    a.fs, a.fb, a.c = fs, fb, c
    a.grid_blocks = int(grid_blocks)
    L.check(L.lib().bdl_chain_ess_fold(a, L.current_stream_handle(dev)), "bdl_chain_ess_fold")
    return flags


def fn_fold(logits, bsum, smean, sM2, bM2, *, sample, batch, chain_groups, probs=None,
            grid_blocks=0):
    """Fold the class probabilities of every chain on a probe batch into the
    batch-means accumulators (bdl_fn_fold, include/bdl_fn.h): logits is the
    contiguous fp32 [chains, probe, classes] of one collected sample, softmax
    and fold are one sweep with no probability tensor in between.  The
    accumulators are stacked as ess_fold's (chain k, element b*classes + c at
    4*chain_groups*k + b*classes + c); `sample`, `batch`, flags and scalars as
    there; bsum may be None at b == 1.  probs: an optional [chains, probe,
    classes] fp32 tensor that receives the folded probabilities.  One launch on
    the current stream, no host synchronisation.  Values never depend on
    grid_blocks (workgroups, 0: default).  Returns the flags."""
    flags, fs, fb, c = E.fold_plan(sample, batch)
    if not torch.is_tensor(logits) or logits.dim() != 3:
        raise ValueError("fn_fold: logits must be a [chains, probe, classes] tensor")
    L.require_hip(logits, "logits")
    if not logits.is_contiguous():
        raise ValueError("fn_fold: logits must be contiguous")
    chains, probe, classes = (int(v) for v in logits.shape)
    if probe < 1:
        raise ValueError("fn_fold: the probe batch is empty")
    if not 1 <= classes <= L.FN_MAX_CLASSES:
        raise ValueError(f"fn_fold: 1 <= classes <= {L.FN_MAX_CLASSES} is required")
    if not 0 <= int(grid_blocks) <= L.FN_MAX_GRID:
        raise ValueError(f"fn_fold: grid_blocks in [0, {L.FN_MAX_GRID}]")
    vecs = [("smean", smean), ("sM2", sM2), ("bM2", bM2)]
    if int(batch) > 1:
        if bsum is None:
            raise ValueError("fn_fold: bsum is required with batch > 1")
        vecs.append(("bsum", bsum))
    chains, chain_groups, n, dev = _stacked_layout("fn_fold", vecs, chains, chain_groups,
                                                   probe * classes)
    if logits.device != dev:
        raise ValueError("fn_fold: all vectors must be on one device")
    if probs is not None:
        L.require_hip(probs, "probs")
        if not probs.is_contiguous() or probs.shape != logits.shape or probs.device != dev:
            raise ValueError("fn_fold: probs must be a contiguous tensor of the logits' shape on "
                             "their device")
    a = L.FnFoldArgs()
    a.logits = logits.data_ptr()
    a.smean, a.sM2, a.bM2 = (t.data_ptr() for t in (smean, sM2, bM2))
    a.bsum = bsum.data_ptr() if int(batch) > 1 else None
    a.probs = None if probs is None else probs.data_ptr()
    a.probe, a.chain_groups, a.chains, a.classes = probe, chain_groups, chains, classes
    a.sample, a.batch, a.flags = int(sample), int(batch), flags
    a.fs, a.fb, a.c = fs, fb, c
    a.grid_blocks = int(grid_blocks)
    L.check(L.lib().bdl_fn_fold(a, L.current_stream_handle(dev)), "bdl_fn_fold")
    return flags


def chain_ess_workspace(device):
    """The report's device scratch (summary + per-workgroup partials), one per device."""
    return _byte_scratch("ess", torch.device(device),
                         lambda: L.lib().bdl_chain_ess_workspace_bytes(1))


def _ess_summary(raw, thresholds):
    s = L.EssSummary.from_buffer_copy(raw)
    return {"n_eval": int(s.n_eval), "n_degenerate": int(s.n_degenerate),
            "n_nonfinite": int(s.n_nonfinite), "argmin": int(s.argmin),
            "n_below": [int(v) for v in s.n_below], "ess_sum": float(s.ess_sum),
            "ess_min": float(s.ess_min), "thresholds": list(thresholds)}


class EssResult(_LazySummary):
    """chain_ess's result (summary: the raw fields of bdl_ess_summary plus
    `thresholds`)."""

    def __init__(self, outs, ws, event, thresholds):
        super().__init__(outs, ws, event, thresholds, _ess_summary)


def chain_ess(sM2, bM2, *, chains, chain_groups, n, samples, batches,
              thresholds=E.DEFAULT_THRESHOLDS, want=(), grid_blocks=0):
    """Batch-means effective sample size of `chains` stacked chains
    (bdl_chain_ess, include/bdl_ess.h) from the accumulators ess_fold keeps:
    samples = S folded per chain, batches = nb closed.  chains = 1 on one
    chain's slice reports that chain alone.  want: any of ESS_OUTPUTS — each an
    [n] tensor in the result; result["summary"] is read on first access.  One
    sweep and a one-workgroup combine on the current stream, no host
    synchronisation here.  Values never depend on grid_blocks (workgroups of
    the sweep, 0: default)."""
    samples, batches = int(samples), int(batches)
    if samples < 2 or batches < 2:
        raise ValueError(f"chain_ess: at least 2 samples and 2 closed batches are required "
                         f"(samples = {samples}, batches = {batches})")
    want = tuple(want)
    thresholds = E.thresholds(thresholds)
    if any(w not in ESS_OUTPUTS for w in want):
        raise ValueError(f"chain_ess: want from {ESS_OUTPUTS}")
    chains, chain_groups, n, dev = _stacked_layout("chain_ess", (("sM2", sM2), ("bM2", bM2)), chains,
                                               chain_groups, n)
    ws = chain_ess_workspace(dev)
    outs = {w: torch.empty(n, dtype=torch.float32, device=dev) for w in want}
    a = L.EssArgs()
    a.sM2, a.bM2 = sM2.data_ptr(), bM2.data_ptr()
    a.ess, a.mcse = (outs[w].data_ptr() if w in outs else None for w in ESS_OUTPUTS)
    a.workspace = ws.data_ptr()
    a.n, a.chain_groups, a.chains = n, chain_groups, chains
    a.samples, a.batches = samples, batches
    for i, t in enumerate(thresholds):
        a.thresholds[i] = t
    a.grid_blocks = int(grid_blocks)
    L.check(L.lib().bdl_chain_ess(a, L.current_stream_handle(dev)), "bdl_chain_ess")
    # the struct leaves the shared workspace in stream order (as chain_diag's)
    snap = ws[:C.sizeof(L.EssSummary)].clone()
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    return EssResult(outs, snap, ev, thresholds)


def _layers_call(what, vectors, segments, *, chains, chain_groups, n, grid_blocks, chains_error,
                 summary_type):
    """What chain_diag_layers / chain_ess_layers share: the layout checks, the
    segment table's shape, the grid (0: two workgroups per CU), the workspace
    and the output table.  Returns (chains, chain_groups, n, device, nsegments,
    grid, workspace, table)."""
    chains, chain_groups, n, dev = _stacked_layout(what, vectors, chains, chain_groups, n,
                                                   chains_error=chains_error)
    if (not torch.is_tensor(segments) or segments.dtype != torch.int64 or segments.dim() != 2
            or segments.shape[1] != 2 or not segments.is_contiguous()):
        raise ValueError(f"{what}: segments must be a contiguous int64 [nsegments, 2] tensor of "
                         "(offset, numel) rows")
    if segments.device != dev:
        raise ValueError(f"{what}: segments must be on the vectors' device")
    nseg = int(segments.shape[0])
    if not 1 <= nseg <= L.LAYERS_MAX_SEGMENTS:
        raise ValueError(f"{what}: 1 <= nsegments <= {L.LAYERS_MAX_SEGMENTS} is required")
    grid = int(grid_blocks)
    if not 0 <= grid <= L.LAYERS_MAX_GRID:
        raise ValueError(f"{what}: grid_blocks in [0, {L.LAYERS_MAX_GRID}]")
    if grid == 0:
        grid = max(1, min(2 * torch.cuda.get_device_properties(dev).multi_processor_count,
                          L.LAYERS_MAX_GRID))
    nbytes = int(L.lib().bdl_layers_workspace_bytes(nseg, grid))
    ws = _scratch(("layers", dev.index, nbytes),
                  lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
    table = torch.empty(nseg * C.sizeof(summary_type), dtype=torch.uint8, device=dev)
    return chains, chain_groups, n, dev, nseg, grid, ws, table


def _layers_table(table, summary_type):
    """The device table as a structured host array (one wait: the copy)."""
    return np.frombuffer(table.cpu().numpy().tobytes(), dtype=np.dtype(summary_type))


def chain_diag_layers(mom1, mom2, segments, *, chains, chain_groups, n, var_mode, ratio, count,
                      var_floor=1e-12, thresholds=(1.01, 1.05, 1.1), grid_blocks=0, div_mode=None):
    """Per-tensor R-hat of `chains` stacked chains (bdl_chain_diag_layers,
    include/bdl_layers.h): chain_diag's inputs and a device table of
    (chain-local offset, numel) rows, one per tensor.  Row t of the result is
    the summary chain_diag would report if only tensor t's elements existed
    (argmax chain-local), as a structured host array with bdl_diag_summary's
    fields.  One sweep and a per-segment combine on the current stream, then
    one wait for the table; no per-element output.  Counts, rhat_max and
    argmax never depend on grid_blocks (workgroups of the sweep, 0: default)."""
    if mom2 is None:
        raise ValueError("chain_diag_layers: the second moment is required (mom2 is None)")
    if mom1 is None:
        raise ValueError("chain_diag_layers: mom1 is required")
    if int(count) < 2:
        raise ValueError("chain_diag_layers: R-hat needs at least 2 samples per chain "
                         f"(count = {count})")
    if len(thresholds) != 3:
        raise ValueError("chain_diag_layers: three thresholds")
    chains, chain_groups, n, dev, nseg, grid, ws, table = _layers_call(
        "chain_diag_layers", (("mom1", mom1), ("mom2", mom2)), segments, chains=chains,
        chain_groups=chain_groups, n=n, grid_blocks=grid_blocks, summary_type=L.DiagSummary,
        chains_error=lambda k: f"at least 2 chains are required (chains = {k})" if k < 2 else None)
    a = L.DiagLayersArgs()
    a.mom1, a.mom2 = mom1.data_ptr(), mom2.data_ptr()
    a.segments, a.table, a.workspace = segments.data_ptr(), table.data_ptr(), ws.data_ptr()
    a.n, a.chain_groups, a.nsegments, a.chains = n, chain_groups, nseg, chains
    a.var_mode, a.grid_blocks = int(var_mode), grid
    a.ratio = float(ratio)
    a.inv_ratio = _inv(ratio) if _div_flag(div_mode) else 0.0  # as chain_diag
    a.var_floor = float(var_floor)
    a.c1 = (int(count) - 1) / int(count)
    for i, t in enumerate(thresholds):
        a.thresholds[i] = float(t)
    L.check(L.lib().bdl_chain_diag_layers(a, L.current_stream_handle(dev)),
            "bdl_chain_diag_layers")
    return _layers_table(table, L.DiagSummary)


def chain_ess_layers(sM2, bM2, segments, *, chains, chain_groups, n, samples, batches,
                     thresholds=E.DEFAULT_THRESHOLDS, grid_blocks=0):
    """Per-tensor batch-means effective sample size of `chains` stacked chains
    (bdl_chain_ess_layers, include/bdl_layers.h): chain_ess's inputs and the
    segment table of chain_diag_layers.  Row t of the result is the summary
    chain_ess would report if only tensor t's elements existed (argmin
    chain-local), as a structured host array with bdl_ess_summary's fields.
    chains = 1 on one chain's slice reports that chain alone.  One sweep and a
    per-segment combine on the current stream, then one wait for the table."""
    samples, batches = int(samples), int(batches)
    if samples < 2 or batches < 2:
        raise ValueError("chain_ess_layers: at least 2 samples and 2 closed batches are required "
                         f"(samples = {samples}, batches = {batches})")
    thresholds = E.thresholds(thresholds)
    chains, chain_groups, n, dev, nseg, grid, ws, table = _layers_call(
        "chain_ess_layers", (("sM2", sM2), ("bM2", bM2)), segments, chains=chains,
        chain_groups=chain_groups, n=n, grid_blocks=grid_blocks, summary_type=L.EssSummary,
        chains_error=None)
    a = L.EssLayersArgs()
    a.sM2, a.bM2 = sM2.data_ptr(), bM2.data_ptr()
    a.segments, a.table, a.workspace = segments.data_ptr(), table.data_ptr(), ws.data_ptr()
    a.n, a.chain_groups, a.nsegments, a.chains = n, chain_groups, nseg, chains
    a.samples, a.batches, a.grid_blocks = samples, batches, grid
    for i, t in enumerate(thresholds):
        a.thresholds[i] = t
    L.check(L.lib().bdl_chain_ess_layers(a, L.current_stream_handle(dev)), "bdl_chain_ess_layers")
    return _layers_table(table, L.EssSummary)


PREDICT_OUTPUTS = ("logp", "entropy", "expected_entropy", "mutual_info", "confidence", "nll",
                   "pred", "disagree")
PREDICT_DEFAULT_WANT = PREDICT_OUTPUTS[1:]


def predict_edges(num_bins):
    """The num_bins - 1 interior right edges of calibration.calc_bins' bins, as
    the fp32 values bdl_predict compares against."""
    return np.linspace(0, 1 + 1e-8, int(num_bins) + 1)[1:-1].astype(np.float32)


def predict_summary(row, members, num_bins):
    """One group's host-read bdl_predict_totals as a dict: n, nll, error, ece /
    mce (calibration.analyze's formula on the bins), entropy, expected_entropy,
    mutual_info, mutual_info_wrong / mutual_info_correct (over the labelled
    examples the vote gets wrong / over every other evaluated example),
    disagreement (the mean share of members off the vote), bins, n_nonfinite.
    A mean over nothing is NaN."""
    def over(s, k):
        return float(s) / k if k else float("nan")
    nb = int(num_bins)
    n, nl, nw = int(row["n"]), int(row["n_labelled"]), int(row["n_wrong"])
    cnt = np.asarray(row["bin_count"][:nb], dtype=np.float64)
    hits = np.asarray(row["bin_hits"][:nb], dtype=np.float64)
    conf = np.asarray(row["bin_conf"][:nb], dtype=np.float64)
    full = cnt > 0
    accs = np.where(full, hits / np.where(full, cnt, 1), 0.0)
    confs = np.where(full, conf / np.where(full, cnt, 1), 0.0)
    gap = np.abs(accs - confs)
    tot = cnt.sum()
    return {"n": n, "n_labelled": nl, "n_nonfinite": int(row["n_nonfinite"]),
            "nll": over(row["nll_sum"], nl), "error": over(nw, nl),
            "ece": float((gap * (cnt / tot)).sum()) if tot else float("nan"),
            "mce": float(gap.max()) if tot else float("nan"),
            "entropy": over(row["entropy_sum"], n),
            "expected_entropy": over(row["expected_entropy_sum"], n),
            "mutual_info": over(row["mi_sum"], n),
            "mutual_info_wrong": over(row["mi_sum_wrong"], nw),
            "mutual_info_correct": over(float(row["mi_sum"]) - float(row["mi_sum_wrong"]), n - nw),
            "disagreement": over(row["disagree_sum"], n * int(members)),
            "bins": {"count": cnt.astype(np.int64).tolist(),
                     "hits": hits.astype(np.int64).tolist(), "conf_sum": conf.tolist(),
                     "accuracy": accs.tolist(), "confidence": confs.tolist()}}


class PredictTotals:
    """The running totals of `predict` calls: bdl_predict_totals[groups] in
    device memory.  `read()` is the one host read (a structured array with the
    struct's fields), `summary()` the dict(s) of predict_summary."""

    def __init__(self, groups, members, num_bins, device):
        self.groups, self.members, self.num_bins = int(groups), int(members), int(num_bins)
        self.buf = torch.empty(self.groups * C.sizeof(L.PredictTotals), dtype=torch.uint8,
                               device=device)
        self.fresh = True  # nothing accumulated: the first call resets

    def read(self):
        if self.fresh:
            raise ValueError("predict: these totals hold nothing yet")
        return np.frombuffer(self.buf.cpu().numpy().tobytes(), dtype=np.dtype(L.PredictTotals))

    def summary(self):
        return [predict_summary(r, self.members, self.num_bins) for r in self.read()]


def predict(logits, labels=None, *, groups=1, totals=None, reset=False, num_bins=15,
            want=PREDICT_DEFAULT_WANT, grid_blocks=0):
    """Predictive uncertainty and calibration of an ensemble from its member
    logits in one fused sweep (bdl_predict, include/bdl_predict.h: the
    definitions and the arithmetic contract).  logits: fp32, contiguous
    [..., B, C] whose leading dimensions flatten to members x groups in that
    order ([M, B, C] with groups=1 pools all members; [components, K, B, C]
    with groups=K gives every chain its own mixture).  labels: int64 [B] on the
    device or None; a label outside [0, C) leaves the example unlabelled.
    Returns (outs, totals): outs[w] for w in want — `logp` [G, B, C], the
    others [G, B] — and the PredictTotals handle the call ADDED to (a new one,
    or the one passed in; reset=True overwrites it).  Two launches on the
    current stream, no host read here: totals.read() / .summary() is the one."""
    want = tuple(want)
    if any(w not in PREDICT_OUTPUTS for w in want):
        raise ValueError(f"predict: want from {PREDICT_OUTPUTS}")
    if not torch.is_tensor(logits) or logits.dim() < 2:
        raise ValueError("predict: logits must be a [..., B, C] tensor")
    L.require_hip(logits, "logits")
    if not logits.is_contiguous():
        raise ValueError("predict: logits must be contiguous")
    G, nb = int(groups), int(num_bins)
    B, Cn = int(logits.shape[-2]), int(logits.shape[-1])
    lead = logits.numel() // max(B * Cn, 1)
    if not 1 <= G <= L.PREDICT_MAX_GROUPS or B < 1 or lead < 1 or lead % G:
        raise ValueError(f"predict: {tuple(logits.shape)} is not members x groups ({G}) x B x C")
    if not 1 <= Cn <= L.PREDICT_MAX_CLASSES:
        raise ValueError(f"predict: 1 <= classes <= {L.PREDICT_MAX_CLASSES} (got {Cn})")
    if not 1 <= nb <= L.PREDICT_MAX_BINS:
        raise ValueError(f"predict: 1 <= num_bins <= {L.PREDICT_MAX_BINS} (got {nb})")
    grid = int(grid_blocks)
    if not 0 <= grid <= L.PREDICT_MAX_GRID:
        raise ValueError(f"predict: grid_blocks in [0, {L.PREDICT_MAX_GRID}]")
    M, dev = lead // G, logits.device
    if labels is not None:
        if (not torch.is_tensor(labels) or labels.dtype != torch.int64 or labels.shape != (B,)
                or not labels.is_contiguous() or labels.device != dev):
            raise ValueError("predict: labels must be a contiguous int64 [B] tensor on the logits' "
                             "device")
    if totals is None:
        totals = PredictTotals(G, M, nb, dev)
    elif (totals.groups, totals.members, totals.num_bins) != (G, M, nb) or totals.buf.device != dev:
        raise ValueError("predict: these totals were started with other groups / members / "
                         "num_bins or on another device")
    if grid == 0:  # the library's default, so that the workspace is sized for it
        per_group = -(-B // (4 if Cn <= L.PREDICT_WAVE_CLASSES else 1))
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        grid = max(1, min(min(per_group, L.PREDICT_MAX_GRID) * G, 4 * cus, L.PREDICT_MAX_GRID))
    nbytes = int(L.lib().bdl_predict_workspace_bytes(G, grid))
    ws = _scratch(("predict", dev.index, nbytes),
                  lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
    outs = {}
    for w in want:
        shape = (G, B, Cn) if w == "logp" else (G, B)
        outs[w] = torch.empty(shape, device=dev,
                              dtype=torch.int32 if w in ("pred", "disagree") else torch.float32)
    a = L.PredictArgs()
    a.logits = logits.data_ptr()
    a.labels = None if labels is None else labels.data_ptr()
    for w in PREDICT_OUTPUTS:
        setattr(a, w, outs[w].data_ptr() if w in outs else None)
    a.totals, a.workspace = totals.buf.data_ptr(), ws.data_ptr()
    a.batch, a.members, a.groups, a.classes, a.num_bins = B, M, G, Cn, nb
    a.grid_blocks = grid
    a.flags = L.PREDICT_RESET if (reset or totals.fresh) else 0
    for i, e in enumerate(predict_edges(nb)):
        a.edges[i] = float(e)
    L.check(L.lib().bdl_predict(a, L.current_stream_handle(dev)), "bdl_predict")
    totals.fresh = False
    return outs, totals


def rank_bytes_per_example(counts=False):
    """Algorithmic HBM bytes per example of one rank call: the
    score and its mark read, the three counts written to the workspace and read
    by the finalise with the mark, 12 B more where the count vectors are asked
    for.  (The O(n^2) count itself re-reads the row from L2 / LDS, not HBM.)"""
    return 8 + 12 + 12 + 4 + (12 if counts else 0)


def rank_summary(row):
    """One row's host-read bdl_rank_totals as a dict: n_pos (P), n_neg (Nn),
    n_excluded, u2, fp_at_tpr, ap_sum and auroc = u2 / (2 * P * Nn), ap =
    ap_sum / P, fpr = fp_at_tpr / Nn — NaN where the denominator is 0 (or no
    threshold keeps the true positives asked for)."""
    P, Nn, u2 = int(row["n_pos"]), int(row["n_neg"]), int(row["u2"])
    fp, aps = int(row["fp_at_tpr"]), float(row["ap_sum"])
    nan = float("nan")
    return {"n_pos": P, "n_neg": Nn, "n_excluded": int(row["n_excluded"]), "u2": u2,
            "fp_at_tpr": fp, "ap_sum": aps,
            "auroc": u2 / (2 * P * Nn) if P and Nn else nan,
            "ap": aps / P if P else nan,
            "fpr": fp / Nn if Nn and fp >= 0 else nan}


class RankResult:
    """What `rank` returns: bdl_rank_totals[rows] in device memory (`buf`) and,
    with counts=True, the uint32-valued [rows, n] tensors `ge_pos`, `ge_neg`,
    `gt_neg` (stored as int32: n < 2^31).  `read()` is the one host read (a
    structured array with the struct's fields), `summary()` the list of
    rank_summary dicts, one per row."""

    def __init__(self, rows, device, buf=None):
        self.rows = int(rows)
        nbytes = self.rows * C.sizeof(L.RankTotals)
        if buf is None:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        elif (not torch.is_tensor(buf) or buf.dtype != torch.uint8 or buf.numel() != nbytes
              or not buf.is_contiguous() or buf.device != device):
            raise ValueError(f"rank: totals must be a contiguous uint8 tensor of {nbytes} bytes "
                             "on the scores' device")
        self.buf = buf
        self.ge_pos = self.ge_neg = self.gt_neg = None

    def read(self):
        return np.frombuffer(self.buf.cpu().numpy().tobytes(), dtype=np.dtype(L.RankTotals))

    def summary(self):
        return [rank_summary(r) for r in self.read()]


def rank(scores, marks, *, scores_per_group=1, need=None, tpr=(19, 20), counts=False,
         totals=None):
    """Exact rank statistics of score rows against 0 / 1 marks (bdl_rank,
    include/bdl_rank.h: the definitions): the integer pair counts behind AUROC,
    average precision and the false-positive rate at a true-positive rate, by
    counting all pairs — no sort, every integer independent of geometry and
    order.  scores: fp32, contiguous [rows, n], higher = more positive.  marks:
    int32, contiguous [rows / scores_per_group, n] (the rows of a group share
    their marks) or [1, n] / [n] (shared by all rows); 1 positive, 0 negative,
    anything else — and a NaN score — excludes the example.  need: the true
    positives fp_at_tpr must keep, for every row; None: ceil(P * tpr[0] /
    tpr[1]) of each row in integer arithmetic on the device (19 / 20: FPR at
    95 % TPR).  counts=True keeps the three per-example count vectors.  totals:
    a uint8 device tensor of rows * 48 bytes to write into (e.g. a slice of one
    buffer several calls share, read once).  Two launches on the current
    stream, no host read here: .read() / .summary() of the result is the one."""
    if not torch.is_tensor(scores) or scores.dim() != 2:
        raise ValueError("rank: scores must be a [rows, n] tensor")
    L.require_hip(scores, "scores")
    if not scores.is_contiguous():
        raise ValueError("rank: scores must be contiguous")
    rows, n = int(scores.shape[0]), int(scores.shape[1])
    spg = int(scores_per_group)
    if not 1 <= rows <= L.RANK_MAX_ROWS or not 1 <= n <= L.RANK_MAX_N:
        raise ValueError(f"rank: 1 <= rows <= {L.RANK_MAX_ROWS} and 1 <= n < 2^31 "
                         f"(got {tuple(scores.shape)})")
    if spg < 1 or rows % spg:
        raise ValueError(f"rank: scores_per_group ({spg}) must divide rows ({rows})")
    dev = scores.device
    if (not torch.is_tensor(marks) or marks.dtype != torch.int32 or not marks.is_contiguous()
            or marks.device != dev or marks.dim() not in (1, 2) or int(marks.shape[-1]) != n):
        raise ValueError("rank: marks must be a contiguous int32 [mark_rows, n] tensor on the "
                         "scores' device")
    mrows = 1 if marks.dim() == 1 else int(marks.shape[0])
    if mrows not in (1, rows // spg):
        raise ValueError(f"rank: marks has {mrows} rows; rows / scores_per_group "
                         f"({rows // spg}) or 1")
    num, den = int(tpr[0]), int(tpr[1])
    if (need is not None and int(need) < 1) or not 1 <= num <= den < 2 ** 31:
        raise ValueError("rank: need >= 1 or None, and 1 <= tpr[0] <= tpr[1] < 2^31")
    need = 0 if need is None else int(need)
    res = RankResult(rows, dev, totals)
    nbytes = int(L.lib().bdl_rank_workspace_bytes(rows, n))
    ws = _scratch(("rank", dev.index, nbytes),
                  lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
    a = L.RankArgs()
    a.scores, a.marks = scores.data_ptr(), marks.data_ptr()
    if counts:
        for w in ("ge_pos", "ge_neg", "gt_neg"):
            t = torch.empty((rows, n), dtype=torch.int32, device=dev)
            setattr(res, w, t)
            setattr(a, w, t.data_ptr())
    a.totals, a.workspace = res.buf.data_ptr(), ws.data_ptr()
    a.n, a.need, a.rows, a.scores_per_group, a.mark_rows = n, need, rows, spg, mrows
    a.tpr_num, a.tpr_den = num, den
    L.check(L.lib().bdl_rank(a, L.current_stream_handle(dev)), "bdl_rank")
    return res


def diversity_bytes_per_example(voters, classes):
    """Algorithmic HBM bytes per example of one diversity call:
    every voter's row read once (its two re-reads come from the caches) and the
    label."""
    return 4 * int(voters) * int(classes) + 8


def diversity_summary(raw):
    """One host-read totals block of bdl_diversity (a record of
    _lib.diversity_totals_dtype, or a dict of its fields) as [P, P] NumPy
    matrices: disagreement (the rate over n), tv (the mean total variation), kl
    (directed: kl[i, j] is the mean KL(p_i || p_j) over the examples where it is
    bounded, NaN where there is none), sym_kl = kl + kl.T, kl_unbounded (the
    counts), double_fault = both_wrong / n_labelled, error_correlation (the phi
    coefficient of the 2 x 2 table of i wrong against j wrong that both_wrong
    and its diagonal determine; NaN where a voter is always or never wrong);
    error [P] (the diagonal of double_fault); n, n_labelled, n_nonfinite.  A
    mean over nothing is NaN."""
    n, nl = int(raw["n"]), int(raw["n_labelled"])
    dis = np.asarray(raw["disagree"], dtype=np.float64)
    bw = np.asarray(raw["both_wrong"], dtype=np.float64)
    unb = np.asarray(raw["kl_unbounded"], dtype=np.int64)
    tv = np.asarray(raw["tv_sum"], dtype=np.float64)
    kls = np.asarray(raw["kl_sum"], dtype=np.float64)
    nan = float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        bounded = n - unb
        kl = np.where(bounded > 0, kls / np.where(bounded > 0, bounded, 1), nan)
        e = np.diag(bw)
        # phi = (N n11 - e_i e_j) / sqrt(e_i (N - e_i) e_j (N - e_j))
        var = e * (nl - e)
        den = np.sqrt(np.outer(var, var))
        phi = np.where(den > 0, (nl * bw - np.outer(e, e)) / np.where(den > 0, den, 1), nan)
        out = {"disagreement": dis / n if n else np.full_like(dis, nan),
               "tv": tv / n if n else np.full_like(tv, nan),
               "kl": kl, "sym_kl": kl + kl.T, "kl_unbounded": unb,
               "error": e / nl if nl else np.full_like(e, nan),
               "double_fault": bw / nl if nl else np.full_like(bw, nan),
               "error_correlation": phi}
    out.update(n=n, n_labelled=nl, n_nonfinite=int(raw["n_nonfinite"]))
    return out


DIVERSITY_PAIR_KEYS = ("disagreement", "tv", "sym_kl", "double_fault")


def diversity_pairs(d):
    """What a reader of `diversity_summary`'s symmetric matrices asks first: for
    each of DIVERSITY_PAIR_KEYS the mean over the pairs i < j and the smallest
    and the largest pair, {"mean", "min", "min_pair", "max", "max_pair"} — the
    lowest pair in row-major order among equals, NaN entries left out (None / NaN
    where every pair is NaN) — and `nearest`: for every voter the other voter
    with the smallest tv to it (the lowest index among equals)."""
    P = int(np.asarray(d["tv"]).shape[0])
    out = {}
    for key in DIVERSITY_PAIR_KEYS:
        m = np.asarray(d[key], dtype=np.float64)
        lo = hi = None
        vals = []
        for i in range(P):
            for j in range(i + 1, P):
                v = float(m[i, j])
                if v != v:
                    continue
                vals.append(v)
                if lo is None or v < lo[0]:
                    lo = (v, (i, j))
                if hi is None or v > hi[0]:
                    hi = (v, (i, j))
        nan = float("nan")
        out[key] = {"mean": float(np.mean(vals)) if vals else nan,
                    "min": lo[0] if lo else nan, "min_pair": lo[1] if lo else None,
                    "max": hi[0] if hi else nan, "max_pair": hi[1] if hi else None}
    tv = np.asarray(d["tv"], dtype=np.float64)
    nearest = []
    for i in range(P):
        row = [(tv[i, j] if tv[i, j] == tv[i, j] else np.inf, j) for j in range(P) if j != i]
        nearest.append(min(row)[1])
    out["nearest"] = nearest
    return out


class DiversityTotals:
    """The running totals of `diversity` calls: the header and the five [P, P]
    matrices of include/bdl_diversity.h in device memory.  `read()` is the one
    host read (a record of _lib.diversity_totals_dtype(P)), `summary()` the
    dict of diversity_summary."""

    def __init__(self, voters, device):
        self.voters = int(voters)
        self.buf = torch.empty(L.diversity_totals_dtype(self.voters).itemsize, dtype=torch.uint8,
                               device=device)
        self.fresh = True  # nothing accumulated: the first call resets

    def read(self):
        if self.fresh:
            raise ValueError("diversity: these totals hold nothing yet")
        return np.frombuffer(self.buf.cpu().numpy().tobytes(),
                             dtype=L.diversity_totals_dtype(self.voters))[0]

    def summary(self):
        return diversity_summary(self.read())


def diversity_default_grid(voters, batch, classes, device):
    """The grid bdl_diversity launches with grid_blocks = 0: one workgroup per
    team-load of examples, at most two per CU, within the workspace bound."""
    P = int(voters)
    wave = P <= L.DIVERSITY_WAVE_VOTERS and int(classes) <= L.DIVERSITY_TILE
    trips = -(-int(batch) // (4 if wave else 1))
    part = (L.diversity_totals_dtype(P).itemsize + 15) // 16 * 16
    cap = max(1, min(L.DIVERSITY_DEFAULT_WORKSPACE // part, L.DIVERSITY_MAX_GRID))
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(trips, 2 * cus, cap))


def diversity(logits, labels=None, *, totals=None, reset=False, grid_blocks=0):
    """Pairwise diversity of an ensemble's voters in one fused sweep
    (bdl_diversity, include/bdl_diversity.h: the definitions and the arithmetic
    contract): per ordered pair (i, j) the count of examples on which the votes
    differ, on which both are wrong, the summed total variation and KL(p_i ||
    p_j) between the voters' softmaxes, and how often that KL is infinite.
    logits: fp32, contiguous [P, B, C], 2 <= P <= 64 (a log-probability row is
    a valid logit row).  labels: int64 [B] on the device or None; a label
    outside [0, C) leaves the example unlabelled.  Returns the DiversityTotals
    handle the call ADDED to (a new one, or the one passed in; reset=True
    overwrites it).  Two launches on the current stream, no host read here:
    totals.read() / .summary() is the one."""
    if not torch.is_tensor(logits) or logits.dim() != 3:
        raise ValueError("diversity: logits must be a [P, B, C] tensor")
    L.require_hip(logits, "logits")
    if not logits.is_contiguous():
        raise ValueError("diversity: logits must be contiguous")
    P, B, Cn = (int(v) for v in logits.shape)
    if not 2 <= P <= L.DIVERSITY_MAX_VOTERS:
        raise ValueError(f"diversity: 2 <= voters <= {L.DIVERSITY_MAX_VOTERS} (got {P})")
    if B < 1 or not 1 <= Cn <= L.DIVERSITY_MAX_CLASSES:
        raise ValueError(f"diversity: batch >= 1 and 1 <= classes <= {L.DIVERSITY_MAX_CLASSES} "
                         f"(got {tuple(logits.shape)})")
    grid = int(grid_blocks)
    if not 0 <= grid <= L.DIVERSITY_MAX_GRID:
        raise ValueError(f"diversity: grid_blocks in [0, {L.DIVERSITY_MAX_GRID}]")
    dev = logits.device
    if labels is not None:
        if (not torch.is_tensor(labels) or labels.dtype != torch.int64 or labels.shape != (B,)
                or not labels.is_contiguous() or labels.device != dev):
            raise ValueError("diversity: labels must be a contiguous int64 [B] tensor on the "
                             "logits' device")
    if totals is None:
        totals = DiversityTotals(P, dev)
    elif totals.voters != P or totals.buf.device != dev:
        raise ValueError("diversity: these totals were started with other voters or on another "
                         "device")
    if grid == 0:  # the library's default, so that the workspace is sized for it
        grid = diversity_default_grid(P, B, Cn, dev)
    nbytes = int(L.lib().bdl_diversity_workspace_bytes(P, grid))
    ws = _scratch(("diversity", dev.index, nbytes),
                  lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
    a = L.DiversityArgs()
    a.logits = logits.data_ptr()
    a.labels = None if labels is None else labels.data_ptr()
    a.totals, a.workspace = totals.buf.data_ptr(), ws.data_ptr()
    a.batch, a.voters, a.classes, a.grid_blocks = B, P, Cn, grid
    a.flags = L.DIVERSITY_RESET if (reset or totals.fresh) else 0
    L.check(L.lib().bdl_diversity(a, L.current_stream_handle(dev)), "bdl_diversity")
    totals.fresh = False
    return totals


def stack_workspace(voters, cols, device):
    """The cached device scratch of stack_gather / stack_fit for `voters`
    voters and `cols` columns (bdl_stack_workspace_bytes)."""
    nbytes = int(L.lib().bdl_stack_workspace_bytes(int(voters), int(cols)))
    if nbytes <= 0:
        raise ValueError(f"stacking: 1 <= voters <= {L.STACK_MAX_VOTERS} and 1 <= columns <= "
                         f"{L.STACK_MAX_COLS} (got {voters}, {cols})")
    return _scratch(("stacking", device.index, nbytes),
                    lambda: torch.empty(nbytes, dtype=torch.uint8, device=device))


def _stack_matrix(what, ell, valid):
    """The checks of the resident score matrix: fp32 [P, cap] and int32 [cap]
    on one HIP device; returns (P, cap)."""
    if not torch.is_tensor(ell) or ell.dim() != 2 or ell.dtype != torch.float32:
        raise ValueError(f"{what}: ell must be a float32 [P, cap] tensor")
    L.require_hip(ell, "ell")
    P, cap = (int(v) for v in ell.shape)
    if not ell.is_contiguous() or not 1 <= P <= L.STACK_MAX_VOTERS \
            or not 1 <= cap <= L.STACK_MAX_COLS:
        raise ValueError(f"{what}: ell must be contiguous with 1 <= voters <= "
                         f"{L.STACK_MAX_VOTERS} and 1 <= cap <= {L.STACK_MAX_COLS} (got "
                         f"{tuple(ell.shape)})")
    if (not torch.is_tensor(valid) or valid.dtype != torch.int32 or valid.shape != (cap,)
            or not valid.is_contiguous() or valid.device != ell.device):
        raise ValueError(f"{what}: valid must be a contiguous int32 [cap] tensor on ell's device")
    return P, cap


def stack_gather(logp, labels, ell, valid, counters, off, *, reset=False, grid_blocks=0):
    """One batch of the voters' log-probabilities into the resident score
    matrix of a stacking fit (bdl_stack_gather, include/bdl_stacking.h):
    ell[p, off + b] = logp[p, b, labels[b]] and valid[off + b] = 1, or a zero
    column with valid = 0 for an example whose label is outside [0, C), for
    which a voter gives a NaN or +inf, or for which every voter gives -inf; the
    three causes are ADDED to `counters` (int64 [3] on the device:
    _lib.STACK_COUNTERS; reset=True overwrites them).  logp: fp32, contiguous
    [P, B, C] (predict's `logp` with groups = P); labels: int64 [B].  Two
    launches on the current stream, no host read.  Returns off + B."""
    P, cap = _stack_matrix("stack_gather", ell, valid)
    dev = ell.device
    if (not torch.is_tensor(logp) or logp.dim() != 3 or logp.dtype != torch.float32
            or not logp.is_contiguous() or logp.device != dev or int(logp.shape[0]) != P):
        raise ValueError(f"stack_gather: logp must be a contiguous float32 [{P}, B, C] tensor on "
                         "ell's device")
    B, Cn = int(logp.shape[1]), int(logp.shape[2])
    if B < 1 or not 1 <= Cn <= L.STACK_MAX_CLASSES:
        raise ValueError(f"stack_gather: batch >= 1 and 1 <= classes <= {L.STACK_MAX_CLASSES} "
                         f"(got {tuple(logp.shape)})")
    if (not torch.is_tensor(labels) or labels.dtype != torch.int64 or labels.shape != (B,)
            or not labels.is_contiguous() or labels.device != dev):
        raise ValueError("stack_gather: labels must be a contiguous int64 [B] tensor on the logp's "
                         "device")
    if (not torch.is_tensor(counters) or counters.dtype != torch.int64 or counters.shape != (3,)
            or not counters.is_contiguous() or counters.device != dev):
        raise ValueError("stack_gather: counters must be a contiguous int64 [3] tensor on ell's "
                         "device")
    off, grid = int(off), int(grid_blocks)
    if off < 0 or off + B > cap:
        raise ValueError(f"stack_gather: columns {off} .. {off + B - 1} do not fit cap = {cap}")
    if not 0 <= grid <= L.STACK_MAX_GRID:
        raise ValueError(f"stack_gather: grid_blocks in [0, {L.STACK_MAX_GRID}]")
    ws = stack_workspace(P, cap, dev)
    a = L.StackGatherArgs()
    a.logp, a.labels, a.ell, a.valid = (logp.data_ptr(), labels.data_ptr(), ell.data_ptr(),
                                        valid.data_ptr())
    a.counters, a.workspace = counters.data_ptr(), ws.data_ptr()
    a.batch, a.off, a.cap, a.voters, a.classes, a.grid_blocks = B, off, cap, P, Cn, grid
    a.flags = L.STACK_RESET if reset else 0
    L.check(L.lib().bdl_stack_gather(a, L.current_stream_handle(dev)), "bdl_stack_gather")
    return off + B


class StackState:
    """bdl_stack_state of one stacking fit in device memory.  `read()` /
    `summary()` is the one host read (w as a float64 [P] array, objective, gap,
    objective_uniform, n, iterations, converged, degenerate); `weights()` the
    device fp64 [P] view of w (no host read)."""

    def __init__(self, voters, device):
        self.voters = int(voters)
        self.buf = torch.empty(C.sizeof(L.StackState), dtype=torch.uint8, device=device)

    def read(self):
        return np.frombuffer(self.buf.cpu().numpy().tobytes(), dtype=np.dtype(L.StackState))[0]

    def weights(self):
        return self.buf.view(torch.float64)[:self.voters]

    def converged_flag(self):
        """The 4-byte `converged` field (a host read of those 4 bytes only)."""
        o = L.StackState.converged.offset
        return int(self.buf[o:o + 4].view(torch.int32).item())

    def summary(self):
        r = self.read()
        return {"weights": np.array(r["w"][:self.voters], dtype=np.float64),
                "objective": float(r["objective"]), "gap": float(r["gap"]),
                "objective_uniform": float(r["objective_uniform"]), "n": int(r["n"]),
                "iterations": int(r["iterations"]), "converged": bool(r["converged"]),
                "degenerate": bool(r["degenerate"])}


def stack_fit(ell, valid, n_cols, *, tol=1e-4, max_iter=2000, check_every=128, grid_blocks=0):
    """Bayesian stacking weights of P voters from their held-out scores, fitted
    on the device (bdl_stack_fit, include/bdl_stacking.h: the iteration, its
    arithmetic contract and why `gap` certifies objective* - objective <= gap).
    ell: fp32 [P, cap] with ell[p, i] = log p_p(y_i | x_i) and valid: int32 [cap]
    (what stack_gather fills); the first n_cols columns are used.  Up to
    max_iter (sweep, update) pairs are enqueued back to back on the current
    stream in chunks of check_every; between chunks the host reads the state's
    4-byte converged flag and nothing else.  Returns the StackState handle;
    `.summary()` is the single read of the state."""
    P, cap = _stack_matrix("stack_fit", ell, valid)
    N, iters, every, grid, tl = int(n_cols), int(max_iter), int(check_every), int(grid_blocks), \
        float(tol)
    if not 1 <= N <= cap:
        raise ValueError(f"stack_fit: 1 <= n_cols <= cap = {cap} (got {N})")
    if not tl >= 0.0:
        raise ValueError(f"stack_fit: tol >= 0 (got {tol})")
    if iters < 1 or not 1 <= every <= L.STACK_MAX_CHUNK:
        raise ValueError(f"stack_fit: max_iter >= 1 and 1 <= check_every <= {L.STACK_MAX_CHUNK} "
                         f"(got {max_iter}, {check_every})")
    if not 0 <= grid <= L.STACK_MAX_GRID:
        raise ValueError(f"stack_fit: grid_blocks in [0, {L.STACK_MAX_GRID}]")
    dev = ell.device
    ws = stack_workspace(P, N, dev)
    state = StackState(P, dev)
    a = L.StackFitArgs()
    a.ell, a.valid, a.state, a.workspace = (ell.data_ptr(), valid.data_ptr(), state.buf.data_ptr(),
                                            ws.data_ptr())
    a.n_cols, a.cap, a.tol, a.voters, a.grid_blocks = N, cap, tl, P, grid
    h, st = L.lib(), L.current_stream_handle(dev)
    done = 0
    while done < iters:
        a.iterations = min(every, iters - done)
        done += a.iterations
        a.flags = (L.STACK_FIRST if done == a.iterations else 0) | \
            (L.STACK_FINAL if done == iters else 0)
        L.check(h.bdl_stack_fit(a, st), "bdl_stack_fit")
        if done < iters and state.converged_flag():
            break
    return state


def _exchange_chains_error(chains):
    if not 1 <= chains <= L.EXCHANGE_MAX_CHAINS:
        return f"1 <= chains <= {L.EXCHANGE_MAX_CHAINS} is required"
    return None


def exchange_workspace(chains, n, device):
    """The cached device partials of exchange_energy / exchange_decide for
    `chains` chains of `n` elements (bdl_exchange_workspace_bytes)."""
    nbytes = int(L.lib().bdl_exchange_workspace_bytes(int(chains), int(n)))
    if nbytes <= 0:
        raise ValueError(f"exchange: 1 <= chains <= {L.EXCHANGE_MAX_CHAINS} and n >= 1 (got "
                         f"{chains}, {n})")
    return _scratch(("exchange", device.index, nbytes),
                    lambda: torch.empty(nbytes, dtype=torch.uint8, device=device))


class ExchangeState:
    """bdl_exchange_state of one ladder of `chains` stacked chains in device
    memory (include/bdl_exchange.h).  `fresh`: the next exchange_decide
    initialises it (BDL_EXCHANGE_FIRST).  `read()` / `summary()` is the one
    host read; `q()` the device fp64 [chains] view of the last energies' prior
    part (no host read)."""

    def __init__(self, chains, device):
        self.chains = int(chains)
        why = _exchange_chains_error(self.chains)
        if why:
            raise ValueError(f"ExchangeState: {why}")
        self.buf = torch.zeros(C.sizeof(L.ExchangeState), dtype=torch.uint8, device=device)
        self.fresh = True

    def read(self):
        return np.frombuffer(self.buf.cpu().numpy().tobytes(), dtype=np.dtype(L.ExchangeState))[0]

    def q(self):
        return self.buf.view(torch.float64)[:self.chains]

    def summary(self):
        r, Kc = self.read(), self.chains
        return {"q": np.array(r["q"][:Kc]), "U": np.array(r["U"][:Kc]),
                "attempts": np.array(r["attempts"][:max(Kc - 1, 0)]),
                "accepts": np.array(r["accepts"][:max(Kc - 1, 0)]),
                "round_trips": np.array(r["round_trips"][:Kc]), "refused": int(r["refused"]),
                "partner": np.array(r["partner"][:Kc]), "replica": np.array(r["replica"][:Kc]),
                "direction": np.array(r["direction"][:Kc])}


def exchange_energy(theta, prior, *, chains, chain_groups, n, grid_blocks=0):
    """The (chain, tile) partials of q_k = sum_i (theta_k[i] - prior_k[i])^2
    over each chain's n real elements (bdl_exchange_energy,
    include/bdl_exchange.h: fp32 difference, fp64 square and sums over fixed
    tiles of 1024 elements in a literal order; prior None: theta0 = 0).  One
    launch on the current stream; `exchange_decide` adds the partials.  Returns
    the workspace."""
    vecs = [("theta", theta)] + ([] if prior is None else [("prior", prior)])
    chains, chain_groups, n, dev = _stacked_layout("exchange_energy", vecs, chains, chain_groups, n,
                                                   chains_error=_exchange_chains_error)
    for nm, t in vecs:
        if t.dtype != torch.float32:
            raise ValueError(f"exchange_energy: {nm} must be float32")
    grid = int(grid_blocks)
    if not 0 <= grid <= L.EXCHANGE_MAX_GRID:
        raise ValueError(f"exchange_energy: grid_blocks in [0, {L.EXCHANGE_MAX_GRID}]")
    ws = exchange_workspace(chains, n, dev)
    a = L.ExchangeEnergyArgs()
    a.theta, a.prior = theta.data_ptr(), None if prior is None else prior.data_ptr()
    a.workspace, a.n, a.chain_groups, a.chains, a.grid_blocks = (ws.data_ptr(), n, chain_groups,
                                                                 chains, grid)
    L.check(L.lib().bdl_exchange_energy(a, L.current_stream_handle(dev)), "bdl_exchange_energy")
    return ws


def exchange_decide(state, workspace, loss=None, beta=None, *, n, n_data=1.0, sigma2=1.0, var=0.0,
                    seed=0, chain0=0, attempt=0, energy_only=False):
    """Attempt `attempt` of the deterministic even-odd exchange between
    adjacent slots (bdl_exchange_decide, include/bdl_exchange.h): q_k from the
    partials in the fixed order, U_k = n_data * loss[k] + q_k / (2 sigma2), the
    Metropolis rule with one Philox word per pair in the exchange step domain,
    partner / replica / counters / round trips in `state`.  loss: device fp32
    [chains]; beta: device fp64 [chains] (1 / T_k).  energy_only: only state.q
    is formed (loss and beta are not read).  One launch, no host read."""
    if not isinstance(state, ExchangeState):
        raise ValueError("exchange_decide: state must be an ExchangeState")
    dev, Kc = state.buf.device, state.chains
    if not torch.is_tensor(workspace) or workspace.device != dev or workspace.numel() < \
            int(L.lib().bdl_exchange_workspace_bytes(Kc, int(n))) or int(n) < 1:
        raise ValueError("exchange_decide: workspace must be exchange_energy's for (chains, n)")
    if not energy_only:
        for nm, t, dt in (("loss", loss, torch.float32), ("beta", beta, torch.float64)):
            if (not torch.is_tensor(t) or t.dtype != dt or t.shape != (Kc,) or not t.is_contiguous()
                    or t.device != dev):
                raise ValueError(f"exchange_decide: {nm} must be a contiguous {dt} [{Kc}] tensor "
                                 "on the state's device")
        if not float(sigma2) > 0 or not float(var) >= 0:
            raise ValueError(f"exchange_decide: sigma2 > 0 and var >= 0 (got {sigma2}, {var})")
        if not 0 <= int(attempt) < 1 << 62:
            raise ValueError("exchange_decide: 0 <= attempt < 2^62")
    a = L.ExchangeDecideArgs()
    a.state, a.workspace = state.buf.data_ptr(), workspace.data_ptr()
    a.loss = None if energy_only else loss.data_ptr()
    a.beta = None if energy_only else beta.data_ptr()
    a.n, a.n_data, a.sigma2, a.var = int(n), float(n_data), float(sigma2), float(var)
    a.seed, a.chain0 = int(seed) & (2 ** 64 - 1), int(chain0) & (2 ** 64 - 1)
    a.attempt, a.chains = int(attempt), Kc
    a.flags = L.EXCHANGE_ENERGY_ONLY if energy_only else \
        (L.EXCHANGE_FIRST if state.fresh else 0)
    L.check(L.lib().bdl_exchange_decide(a, L.current_stream_handle(dev)), "bdl_exchange_decide")
    if not energy_only:
        state.fresh = False


def exchange_swap(state, vectors, *, chain_groups, grid_blocks=0):
    """Exchange the whole chain slots (padding included) of every pair
    `state.partner` accepted, in each of the 1 .. 4 stacked fp32 `vectors`
    (bdl_exchange_swap, include/bdl_exchange.h).  One launch, no host read."""
    if not isinstance(state, ExchangeState):
        raise ValueError("exchange_swap: state must be an ExchangeState")
    vectors = list(vectors)
    if not 1 <= len(vectors) <= L.EXCHANGE_MAX_VECTORS:
        raise ValueError(f"exchange_swap: 1 .. {L.EXCHANGE_MAX_VECTORS} vectors (got "
                         f"{len(vectors)})")
    vecs = [(f"vectors[{i}]", v) for i, v in enumerate(vectors)]
    chains, chain_groups, _, dev = _stacked_layout("exchange_swap", vecs, state.chains, chain_groups,
                                                   4 * int(chain_groups),
                                                   chains_error=_exchange_chains_error)
    for nm, t in vecs:
        if t.dtype != torch.float32 or t.device != state.buf.device:
            raise ValueError(f"exchange_swap: {nm} must be float32 on the state's device")
    grid = int(grid_blocks)
    if not 0 <= grid <= L.EXCHANGE_MAX_GRID:
        raise ValueError(f"exchange_swap: grid_blocks in [0, {L.EXCHANGE_MAX_GRID}]")
    a = L.ExchangeSwapArgs()
    a.state = state.buf.data_ptr()
    for i, v in enumerate(vectors):
        a.vectors[i] = v.data_ptr()
    a.chain_groups, a.nvectors, a.chains, a.grid_blocks = chain_groups, len(vectors), chains, grid
    L.check(L.lib().bdl_exchange_swap(a, L.current_stream_handle(dev)), "bdl_exchange_swap")


def _temper_rows(what, logp, labels, groups, grid_blocks):
    """The checks `temper_fit` and `temper_report` share, worded as predict's;
    returns (G, N, C, grid, workspace)."""
    if not torch.is_tensor(logp) or logp.dim() < 2:
        raise ValueError(f"{what}: logp must be a [G, N, C] tensor")
    L.require_hip(logp, "logp")
    if not logp.is_contiguous():
        raise ValueError(f"{what}: logp must be contiguous")
    G = int(groups)
    N, Cn = int(logp.shape[-2]), int(logp.shape[-1])
    lead = logp.numel() // max(N * Cn, 1)
    if not 1 <= G <= L.TEMPER_MAX_GROUPS or N < 1 or lead != G:
        raise ValueError(f"{what}: {tuple(logp.shape)} is not groups ({G}) x N x C")
    if not 1 <= Cn <= L.TEMPER_MAX_CLASSES:
        raise ValueError(f"{what}: 1 <= classes <= {L.TEMPER_MAX_CLASSES} (got {Cn})")
    grid = int(grid_blocks)
    if not 0 <= grid <= L.TEMPER_MAX_GRID:
        raise ValueError(f"{what}: grid_blocks in [0, {L.TEMPER_MAX_GRID}]")
    dev = logp.device
    if labels is not None:
        if (not torch.is_tensor(labels) or labels.dtype != torch.int64 or labels.shape != (N,)
                or not labels.is_contiguous() or labels.device != dev):
            raise ValueError(f"{what}: labels must be a contiguous int64 [N] tensor on the logp's "
                             "device")
    if grid == 0:  # the library's default, so that the workspace is sized for it
        per_group = -(-N // (4 if Cn <= L.TEMPER_WAVE_CLASSES else 1))
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        grid = max(1, min(min(per_group, L.TEMPER_MAX_GRID) * G, 4 * cus, L.TEMPER_MAX_GRID))
    nbytes = int(L.lib().bdl_temper_workspace_bytes(G, grid))
    ws = _scratch(("temper", dev.index, nbytes),
                  lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
    return G, N, Cn, grid, ws


def temper_betas(temperature, groups):
    """[G] fp32 beta = 1 / T of a float or a length-G sequence of temperatures
    in [TEMPER_MIN_T, TEMPER_MAX_T] (the value the kernels multiply by)."""
    t = np.asarray(temperature, dtype=np.float64)
    if t.ndim == 0:
        t = np.full(int(groups), float(t))
    if t.shape != (int(groups),):
        raise ValueError(f"temper: temperature must be a float or {int(groups)} values, one per "
                         "group")
    if not (np.isfinite(t).all() and (t >= L.TEMPER_MIN_T).all() and (t <= L.TEMPER_MAX_T).all()):
        raise ValueError(f"temper: {L.TEMPER_MIN_T} <= temperature <= {L.TEMPER_MAX_T}")
    return (1.0 / t).astype(np.float32)


class TemperState:
    """bdl_temper_state[groups] in device memory: the per-group beta = 1 / T and
    what the fit's last sweep found.  `read()` is the one host read (a
    structured array with the struct's fields), `summary()` one dict per group,
    `temperatures()` the [G] temperatures as a device tensor (no host read)."""

    def __init__(self, betas, device):
        host = np.zeros(len(betas), dtype=np.dtype(L.TemperState))
        host["beta"] = betas
        self.groups = len(betas)
        self.buf = torch.from_numpy(host.view(np.uint8).copy()).to(device)

    def read(self):
        return np.frombuffer(self.buf.cpu().numpy().tobytes(), dtype=np.dtype(L.TemperState))

    def betas(self):
        """[G] fp32 view of the struct's beta fields (device memory)."""
        words = self.buf.view(torch.float32).view(self.groups, -1)
        return words[:, L.TemperState.beta.offset // 4]

    def temperatures(self):
        return 1.0 / self.betas()

    def summary(self):
        return [{"temperature": 1.0 / float(r["beta"]), "nll_before": float(r["nll_first"]),
                 "nll_after": float(r["nll"]), "iterations": int(r["iterations"]),
                 "converged": bool(r["converged"]), "at_bound": bool(r["at_bound"]),
                 "degenerate": bool(r["degenerate"]), "n": int(r["n"]),
                 "n_nonfinite": int(r["n_nonfinite"]), "n_inf_label": int(r["n_inf_label"])}
                for r in self.read()]


def temper_fit(logp, labels, groups=1, rtol=1e-6, max_iter=32, grid_blocks=0):
    """One scalar temperature per group, fitted on the device to the
    sample-averaged log-probabilities `logp` [G, N, C] (what predict's `logp`
    output is) and int64 labels [N]: a safeguarded Newton iteration in
    beta = 1 / T from T = 1 (include/bdl_temper.h: the definitions, the special
    values, the update rule).  `max_iter` (sweep, update) pairs are enqueued
    back to back on the current stream with no host read in between; the
    TemperState handle returned reads the device once, in `.summary()`: per
    group temperature, nll_before (at T = 1), nll_after, iterations, converged,
    at_bound, degenerate, n, n_nonfinite, n_inf_label.  A group that is neither
    converged nor degenerate did not converge (at_bound: its optimum is at or
    beyond a limit of T, and it stopped sweeping once it sat there)."""
    G, N, Cn, grid, ws = _temper_rows("temper_fit", logp, labels, groups, grid_blocks)
    iters, rt = int(max_iter), float(rtol)
    if not 1 <= iters <= L.TEMPER_MAX_ITER:
        raise ValueError(f"temper_fit: 1 <= max_iter <= {L.TEMPER_MAX_ITER} (got {iters})")
    if not 0.0 <= rt < 1.0:
        raise ValueError(f"temper_fit: 0 <= rtol < 1 (got {rtol})")
    dev = logp.device
    state = TemperState(np.ones(G, dtype=np.float32), dev)
    a = L.TemperFitArgs()
    a.logp = logp.data_ptr()
    a.labels = None if labels is None else labels.data_ptr()
    a.state, a.workspace = state.buf.data_ptr(), ws.data_ptr()
    a.batch, a.rtol, a.groups, a.classes, a.grid_blocks, a.max_iter = N, rt, G, Cn, grid, iters
    h, st = L.lib(), L.current_stream_handle(dev)
    for _ in range(iters):
        L.check(h.bdl_temper_fit_sweep(a, st), "bdl_temper_fit_sweep")
        L.check(h.bdl_temper_fit_update(a, st), "bdl_temper_fit_update")
    return state


def temper_summary(row, num_bins):
    """One group's host-read bdl_temper_totals as a dict: n, nll, error, ece /
    mce (calibration.analyze's formula on the bins), entropy, confidence, bins,
    n_labelled, n_nonfinite.  A mean over nothing is NaN."""
    full = predict_summary({**{k: row[k] for k in ("n", "n_labelled", "n_nonfinite", "n_wrong",
                                                    "nll_sum", "entropy_sum", "bin_count",
                                                    "bin_hits", "bin_conf")},
                            "expected_entropy_sum": 0.0, "mi_sum": 0.0, "mi_sum_wrong": 0.0,
                            "disagree_sum": 0}, 1, num_bins)
    out = {k: full[k] for k in ("n", "n_labelled", "n_nonfinite", "nll", "error", "ece", "mce",
                                "entropy", "bins")}
    n = int(row["n"])
    out["confidence"] = float(row["confidence_sum"]) / n if n else float("nan")
    return out


class TemperTotals:
    """The running totals of `temper_report` calls: bdl_temper_totals[groups] in
    device memory.  `read()` is the one host read, `summary()` the dict(s) of
    temper_summary."""

    def __init__(self, groups, num_bins, device):
        self.groups, self.num_bins = int(groups), int(num_bins)
        self.buf = torch.empty(self.groups * C.sizeof(L.TemperTotals), dtype=torch.uint8,
                               device=device)
        self.fresh = True  # nothing accumulated: the first call resets

    def read(self):
        if self.fresh:
            raise ValueError("temper_report: these totals hold nothing yet")
        return np.frombuffer(self.buf.cpu().numpy().tobytes(), dtype=np.dtype(L.TemperTotals))

    def summary(self):
        return [temper_summary(r, self.num_bins) for r in self.read()]


def temper_report(logp, labels, temperature, groups=1, totals=None, num_bins=15, grid_blocks=0):
    """NLL, error, ECE / MCE, entropy and confidence of q = softmax(logp / T)
    per group (bdl_temper_report, include/bdl_temper.h), added to `totals` in
    device memory (a new TemperTotals, or the one passed in).  temperature: a TemperState (a fitted temperature never
    visits the host), a float, or a length-G sequence.  Two launches on the
    current stream, no host read here: totals.read() / .summary() is the one."""
    G, N, Cn, grid, ws = _temper_rows("temper_report", logp, labels, groups, grid_blocks)
    nb = int(num_bins)
    if not 1 <= nb <= L.TEMPER_MAX_BINS:
        raise ValueError(f"temper_report: 1 <= num_bins <= {L.TEMPER_MAX_BINS} (got {nb})")
    dev = logp.device
    state = temperature
    if not isinstance(state, TemperState):
        state = TemperState(temper_betas(temperature, G), dev)
    elif state.groups != G or state.buf.device != dev:
        raise ValueError("temper_report: this state was fitted with other groups or on another "
                         "device")
    if totals is None:
        totals = TemperTotals(G, nb, dev)
    elif (totals.groups, totals.num_bins) != (G, nb) or totals.buf.device != dev:
        raise ValueError("temper_report: these totals were started with other groups / num_bins "
                         "or on another device")
    a = L.TemperReportArgs()
    a.logp = logp.data_ptr()
    a.labels = None if labels is None else labels.data_ptr()
    a.state, a.totals, a.workspace = state.buf.data_ptr(), totals.buf.data_ptr(), ws.data_ptr()
    a.batch, a.groups, a.classes, a.num_bins, a.grid_blocks = N, G, Cn, nb, grid
    a.flags = L.TEMPER_RESET if totals.fresh else 0
    for i, e in enumerate(predict_edges(nb)):
        a.edges[i] = float(e)
    L.check(L.lib().bdl_temper_report(a, L.current_stream_handle(dev)), "bdl_temper_report")
    totals.fresh = False
    totals.state = state  # keeps an uploaded temperature alive until the launches ran
    return totals


def _mixture_rows(what, logits, labels, groups, grid_blocks, pairs_of):
    """The checks `member_score` and `mixture` share, worded as predict's;
    returns (members, G, B, C, grid_blocks); pairs_of(members, G) is the
    number of pairs the sweep's grid has."""
    if not torch.is_tensor(logits) or logits.dim() < 2:
        raise ValueError(f"{what}: logits must be a [..., B, C] tensor")
    L.require_hip(logits, "logits")
    if not logits.is_contiguous():
        raise ValueError(f"{what}: logits must be contiguous")
    G = int(groups)
    B, Cn = int(logits.shape[-2]), int(logits.shape[-1])
    lead = logits.numel() // max(B * Cn, 1)
    if G < 1 or B < 1 or lead < 1 or lead % G:
        raise ValueError(f"{what}: {tuple(logits.shape)} is not members x groups ({G}) x B x C")
    if not 1 <= Cn <= L.MIXTURE_MAX_CLASSES:
        raise ValueError(f"{what}: 1 <= classes <= {L.MIXTURE_MAX_CLASSES} (got {Cn})")
    M = lead // G
    pairs = pairs_of(M, G)
    if not 1 <= pairs <= L.MIXTURE_MAX_PAIRS:
        raise ValueError(f"{what}: at most {L.MIXTURE_MAX_PAIRS} (member, group) pairs / groups "
                         f"(got {pairs})")
    grid = int(grid_blocks)
    if not 0 <= grid <= L.MIXTURE_MAX_GRID:
        raise ValueError(f"{what}: grid_blocks in [0, {L.MIXTURE_MAX_GRID}]")
    dev = logits.device
    if labels is not None:
        if (not torch.is_tensor(labels) or labels.dtype != torch.int64 or labels.shape != (B,)
                or not labels.is_contiguous() or labels.device != dev):
            raise ValueError(f"{what}: labels must be a contiguous int64 [B] tensor on the logits' "
                             "device")
    return M, G, B, Cn, grid


def _mixture_grid(grid, B, Cn, pairs, dev):
    """grid_blocks, or the library's default (so that the workspace is sized
    for it): one workgroup per row slot of a pair, up to four per CU over all
    pairs."""
    if grid:
        return grid
    slots = -(-B // (4 if Cn <= L.MIXTURE_WAVE_CLASSES else 1))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return max(1, min(slots, -(-4 * cus // pairs), L.MIXTURE_MAX_GRID))


class MemberScores:
    """The running loss sums of `member_score` calls: bdl_member_score_t
    [members, groups] in device memory.  `read()` is the one host read (a
    structured [members, groups] array with the struct's fields)."""

    def __init__(self, members, groups, device):
        self.members, self.groups = int(members), int(groups)
        self.buf = torch.empty(self.members * self.groups * C.sizeof(L.MemberScore),
                               dtype=torch.uint8, device=device)
        self.fresh = True  # nothing accumulated: the first call resets

    def read(self):
        if self.fresh:
            raise ValueError("member_score: these scores hold nothing yet")
        raw = np.frombuffer(self.buf.cpu().numpy().tobytes(), dtype=np.dtype(L.MemberScore))
        return raw.reshape(self.members, self.groups)


def member_score(logits, labels, *, groups, scores=None, reset=False, grid_blocks=0):
    """The likelihood pass of a cycle end in one fused sweep per batch
    (bdl_member_score, include/bdl_mixture.h: the arithmetic contract): the
    cross-entropy sum, the scored, wrong and non-finite row counts of every
    (member, group) pair of fp32 logits [..., B, C] (leading dimensions
    flattening to members x groups) against int64 labels [B], ADDED to the
    MemberScores handle (a new one, or the one passed in; reset=True overwrites
    it).  Two launches on the current stream, no host read here:
    scores.read() is the one."""
    if labels is None:
        raise ValueError("member_score: labels must be a contiguous int64 [B] tensor on the "
                         "logits' device")
    M, G, B, Cn, grid = _mixture_rows("member_score", logits, labels, groups, grid_blocks,
                                      lambda m, g: m * g)
    dev = logits.device
    if scores is None:
        scores = MemberScores(M, G, dev)
    elif (scores.members, scores.groups) != (M, G) or scores.buf.device != dev:
        raise ValueError("member_score: these scores were started with other members / groups or "
                         "on another device")
    grid = _mixture_grid(grid, B, Cn, M * G, dev)
    nbytes = int(L.lib().bdl_member_score_workspace_bytes(M, G, grid))
    ws = _scratch(("member_score", dev.index, nbytes),
                  lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
    a = L.MemberScoreArgs()
    a.logits, a.labels = logits.data_ptr(), labels.data_ptr()
    a.scores, a.workspace = scores.buf.data_ptr(), ws.data_ptr()
    a.batch, a.members, a.groups, a.classes, a.grid_blocks = B, M, G, Cn, grid
    a.flags = L.MIXTURE_RESET if (reset or scores.fresh) else 0
    L.check(L.lib().bdl_member_score(a, L.current_stream_handle(dev)), "bdl_member_score")
    scores.fresh = False
    return scores


MIXTURE_OUTPUTS = ("logp", "expected_entropy")


class MixtureTotals:
    """The running totals of `mixture` calls: bdl_mixture_totals[groups] in
    device memory.  `read()` is the one host read (a structured array with the
    struct's fields), `summary()` one dict per group: n, n_nonfinite,
    expected_entropy (the mean; NaN over nothing)."""

    def __init__(self, groups, device):
        self.groups = int(groups)
        self.buf = torch.empty(self.groups * C.sizeof(L.MixtureTotals), dtype=torch.uint8,
                               device=device)
        self.fresh = True  # nothing accumulated: the first call resets

    def read(self):
        if self.fresh:
            raise ValueError("mixture: these totals hold nothing yet")
        return np.frombuffer(self.buf.cpu().numpy().tobytes(), dtype=np.dtype(L.MixtureTotals))

    def summary(self):
        return [mixture_summary(r) for r in self.read()]


def mixture_summary(row):
    n = int(row["n"])
    return {"n": n, "n_nonfinite": int(row["n_nonfinite"]),
            "expected_entropy": float(row["expected_entropy_sum"]) / n if n else float("nan")}


def mixture(logits, weights, labels=None, *, draws, groups, combine="arithmetic",
            want=("logp",), totals=None, reset=False, grid_blocks=0):
    """The weighted predictive of a mixture of components in one fused sweep
    (bdl_mixture, include/bdl_mixture.h: the definitions and the arithmetic
    contract).  logits: fp32, contiguous [..., B, C] whose leading dimensions
    flatten to (components x draws) x groups — member c * draws + s is draw s
    of component c.  weights: float64 [components, groups] on the device, taken
    as given; a component below 1e-10 is skipped and its rows are not read.
    combine: "arithmetic" (log of the weighted mean probability) or
    "reference" (a cyclical Runner's renormalised weighted sum of component
    log-probabilities).  labels: accepted as predict takes them, not read.
    Returns (outs, totals): outs[w] for w in want — `logp` [G, B, C],
    `expected_entropy` [G, B] — and the MixtureTotals handle the call ADDED to
    (reset=True overwrites it).  Two launches on the current stream, no host
    read here: totals.read() / .summary() is the one."""
    want = tuple(want)
    if any(w not in MIXTURE_OUTPUTS for w in want):
        raise ValueError(f"mixture: want from {MIXTURE_OUTPUTS}")
    if combine not in L.MIX_COMBINE:
        raise ValueError(f"mixture: combine from {tuple(L.MIX_COMBINE)} (got {combine!r})")
    M, G, B, Cn, grid = _mixture_rows("mixture", logits, labels, groups, grid_blocks,
                                      lambda m, g: g)
    D = int(draws)
    if D < 1 or M % D:
        raise ValueError(f"mixture: {M} members are not components x draws ({D})")
    comps, dev = M // D, logits.device
    if (not torch.is_tensor(weights) or weights.dtype != torch.float64
            or tuple(weights.shape) != (comps, G) or not weights.is_contiguous()
            or weights.device != dev):
        raise ValueError(f"mixture: weights must be a contiguous float64 [{comps}, {G}] tensor on "
                         "the logits' device")
    if totals is None:
        totals = MixtureTotals(G, dev)
    elif totals.groups != G or totals.buf.device != dev:
        raise ValueError("mixture: these totals were started with other groups or on another "
                         "device")
    grid = _mixture_grid(grid, B, Cn, G, dev)
    nbytes = int(L.lib().bdl_mixture_workspace_bytes(G, grid))
    ws = _scratch(("mixture", dev.index, nbytes),
                  lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
    outs = {w: torch.empty((G, B, Cn) if w == "logp" else (G, B), device=dev, dtype=torch.float32)
            for w in want}
    a = L.MixtureArgs()
    a.logits, a.weights = logits.data_ptr(), weights.data_ptr()
    a.labels = None if labels is None else labels.data_ptr()
    for w in MIXTURE_OUTPUTS:
        setattr(a, w, outs[w].data_ptr() if w in outs else None)
    a.totals, a.workspace = totals.buf.data_ptr(), ws.data_ptr()
    a.batch, a.components, a.draws, a.groups, a.classes = B, comps, D, G, Cn
    a.combine, a.grid_blocks = L.MIX_COMBINE[combine], grid
    a.flags = L.MIXTURE_RESET if (reset or totals.fresh) else 0
    L.check(L.lib().bdl_mixture(a, L.current_stream_handle(dev)), "bdl_mixture")
    totals.fresh = False
    return outs, totals


def clip_bytes_per_elem(clipped_share=1.0):
    """Algorithmic HBM bytes per gradient element of one chain_clip call
    (DESIGN §4e): every element read once for the norm; the elements of the
    clipped chains read and written once more."""
    return 4 + 8 * float(clipped_share)


def chain_clip_workspace(chains, device):
    """A fresh workspace for chain_clip over `chains` chains (a float tensor
    whose first 2 * chains elements are the (norm, coef) table)."""
    nbytes = int(L.lib().bdl_chain_clip_workspace_bytes(int(chains)))
    if nbytes <= 0:
        raise ValueError(f"chain_clip: chains must be in [1, {L.CLIP_MAX_CHAINS}] (got {chains})")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def clip_blocks_per_chain(numel, chains, device=None):
    """Workgroups per chain for a gradient of `numel` elements per chain: one
    per 4096 elements (a full block iteration of the sweep), at most about four
    per CU over all chains — a small network gets a small grid."""
    cus = torch.cuda.get_device_properties(_device(device)).multi_processor_count
    cap = max(1, -(-4 * cus // max(1, int(chains))))
    return int(max(1, min(-(-int(numel) // 4096), cap, L.CLIP_MAX_BLOCKS_PER_CHAIN)))


def chain_clip(segments, nsegments, chains, max_norm, workspace=None, blocks_per_chain=0):
    """torch.nn.utils.clip_grad_norm_(max_norm) of every one of `chains`
    stacked chains by the norm of its own gradient, in place on the device
    (bdl_chain_clip, include/bdl_clip.h).  segments: the device table
    (StackedState.grad_segments: an int64 [nsegments, 3] tensor of (base
    address, numel, chain stride) rows).  Three launches on the current
    stream, no host synchronisation.  Returns the [chains, 2] float view of
    the workspace: (norm_k, coef_k) per chain.  workspace None: one cached per
    device and chain count (the view is then overwritten by the next such
    call).  Values do not depend on blocks_per_chain (0: the library's
    default) beyond the fp64 summation order of the norm."""
    if segments.dtype != torch.int64 or not segments.is_cuda or not segments.is_contiguous() \
            or segments.numel() < 3 * int(nsegments):
        raise ValueError("chain_clip: segments must be a contiguous int64 device tensor of "
                         "nsegments x 3")
    if not float(max_norm) > 0:
        raise ValueError(f"chain_clip: max_norm must be > 0 (got {max_norm})")
    chains, dev = int(chains), segments.device
    if workspace is None:
        workspace = _scratch(("clip", dev.index, chains),
                             lambda: chain_clip_workspace(chains, dev))
    else:
        L.require_hip(workspace, "workspace")
        if workspace.device != dev or not workspace.is_contiguous() or \
                4 * workspace.numel() < int(L.lib().bdl_chain_clip_workspace_bytes(chains)):
            raise ValueError("chain_clip: workspace must be a contiguous float tensor of "
                             "bdl_chain_clip_workspace_bytes(chains) bytes on the segments' device")
    a = L.ClipArgs()
    a.segments = segments.data_ptr()
    a.nsegments, a.chains = int(nsegments), chains
    a.max_norm = float(max_norm)
    a.blocks_per_chain = int(blocks_per_chain)
    a.workspace = workspace.data_ptr()
    L.check(L.lib().bdl_chain_clip(a, L.current_stream_handle(dev)), "bdl_chain_clip")
    return workspace[:2 * chains].view(chains, 2)


def stats_bytes_per_elem(mom=True, prior=False):
    """Algorithmic HBM bytes per element of one chain_stats call:
    the gradient and theta, the momentum and the prior mean where bound, each
    read once; nothing per element is written."""
    return 8 + (4 if mom else 0) + (4 if prior else 0)


def chain_stats_workspace(chains, nsegments, device):
    """A fresh workspace for chain_stats over `chains` chains and `nsegments`
    segments (a float64 tensor: the per-workgroup partial sums)."""
    nbytes = int(L.lib().bdl_chain_stats_workspace_bytes(int(chains), int(nsegments)))
    if nbytes <= 0:
        raise ValueError(f"chain_stats: chains must be in [1, {L.STATS_MAX_CHAINS}] and nsegments "
                         f"in [1, {L.STATS_MAX_SEGMENTS}] (got {chains}, {nsegments})")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def stats_blocks_per_chain(numel, chains, device=None):
    """Workgroups per chain for chain_stats over `numel` elements per chain:
    one per 4096 elements (a full block iteration of the sweep), at most about
    four per CU over all chains (clip_blocks_per_chain's rule, this sweep's cap)."""
    cus = torch.cuda.get_device_properties(_device(device)).multi_processor_count
    cap = max(1, -(-4 * cus // max(1, int(chains))))
    return int(max(1, min(-(-int(numel) // 4096), cap, L.STATS_MAX_BLOCKS_PER_CHAIN)))


def chain_stats(segments, nsegments, chains, chain_groups, theta, acc, *, mom=None,
                prior_mean=None, lr=None, lr_table=None, lr_row_stride=12, accumulate=False,
                workspace=None, blocks_per_chain=0):
    """The per-(chain, tensor) sums G2, V2, D2, DG, VG and V2L = V2 / lr of K
    stacked chains in one fused sweep (bdl_chain_stats, include/bdl_stats.h),
    written into (accumulate False) or added to (True) `acc`, a device float64
    [chains, nsegments, 6] tensor.  segments: the device table
    (StackedState.stat_segments: an int64 [nsegments, 5] tensor of (gradient
    base, numel, gradient chain stride, chain-local offset, lr group) rows);
    theta / mom / prior_mean: the stacked [K * 4 * chain_groups] vectors.  The
    lr comes from exactly one source: `lr` = (body, head) host floats for all
    chains, or `lr_table`, a device float32 tensor whose row k (lr_row_stride
    floats apart: 12 for a [K, 12] bdl_chain_scalars block) starts with chain
    k's body / head lr.  Two launches on the current stream, no host
    synchronisation.  Values do not depend on blocks_per_chain (0: the
    library's default) beyond the fp64 summation order."""
    if segments.dtype != torch.int64 or not segments.is_cuda or not segments.is_contiguous() \
            or segments.numel() < 5 * int(nsegments):
        raise ValueError("chain_stats: segments must be a contiguous int64 device tensor of "
                         "nsegments x 5")
    chains, nsegments, dev = int(chains), int(nsegments), segments.device
    slot = 4 * int(chain_groups)
    for nm, v in (("theta", theta), ("mom", mom), ("prior_mean", prior_mean)):
        if v is None and nm != "theta":
            continue
        L.require_hip(v, nm)
        if v.device != dev or not v.is_contiguous() or v.numel() < chains * slot:
            raise ValueError(f"chain_stats: {nm} must be a contiguous stacked vector of "
                             "chains * 4 * chain_groups elements on the segments' device")
    if acc.dtype != torch.float64 or acc.device != dev or not acc.is_contiguous() \
            or acc.numel() < chains * nsegments * len(L.STATS_SUMS):
        raise ValueError("chain_stats: acc must be a contiguous float64 device tensor of "
                         "chains x nsegments x 6")
    if (lr is None) == (lr_table is None):
        raise ValueError("chain_stats: give exactly one lr source (lr or lr_table)")
    a = L.StatsArgs()
    if lr is not None:
        l0, l1 = (float(v) for v in lr)
        if not (l0 > 0 and l1 > 0):
            raise ValueError(f"chain_stats: lr must be > 0 for both groups (got {lr})")
        a.lr[0], a.lr[1] = l0, l1
    else:
        L.require_hip(lr_table, "lr_table")
        if lr_table.device != dev or int(lr_row_stride) < 2 or \
                lr_table.numel() < (chains - 1) * int(lr_row_stride) + 2:
            raise ValueError("chain_stats: lr_table must hold chains rows of lr_row_stride >= 2 "
                             "floats on the segments' device")
        a.lr_table, a.lr_row_stride = lr_table.data_ptr(), int(lr_row_stride)
    if workspace is None:
        workspace = _STATS_WS.get((dev.index, chains, nsegments))
        if workspace is None:
            workspace = _STATS_WS[(dev.index, chains, nsegments)] = \
                chain_stats_workspace(chains, nsegments, dev)
    elif workspace.dtype != torch.float64 or workspace.device != dev \
            or not workspace.is_contiguous() or 8 * workspace.numel() < int(
                L.lib().bdl_chain_stats_workspace_bytes(chains, nsegments)):
        raise ValueError("chain_stats: workspace must be a contiguous float64 tensor of "
                         "bdl_chain_stats_workspace_bytes(chains, nsegments) bytes on the "
                         "segments' device")
    a.theta = theta.data_ptr()
    a.mom = None if mom is None else mom.data_ptr()
    a.prior_mean = None if prior_mean is None else prior_mean.data_ptr()
    a.segments, a.acc, a.workspace = segments.data_ptr(), acc.data_ptr(), workspace.data_ptr()
    a.chain_groups, a.nsegments, a.chains = int(chain_groups), nsegments, chains
    a.accumulate, a.blocks_per_chain = 1 if accumulate else 0, int(blocks_per_chain)
    L.check(L.lib().bdl_chain_stats(a, L.current_stream_handle(dev)), "bdl_chain_stats")
    return acc


_STATS_WS = {}  # (device index, chains, nsegments) -> workspace (per-workgroup partials)


CHAIN_STEP_WG_PER_CU = 2  # default grid of chain_step: about this many workgroups per CU


def chain_step_blocks_per_chain(n1, chains, device=None, unroll=1):
    """Workgroups per chain for chain_step over `n1` elements per chain: about
    CHAIN_STEP_WG_PER_CU per CU over all chains, never more than the chain has
    block iterations (256 * unroll float4 groups each)."""
    cus = torch.cuda.get_device_properties(_device(device)).multi_processor_count
    iters = -(-((int(n1) + 3) // 4) // (256 * max(1, int(unroll))))
    want = -(-CHAIN_STEP_WG_PER_CU * cus // max(1, int(chains)))
    return int(max(1, min(want, iters, L.CHAIN_STEP_MAX_BLOCKS_PER_CHAIN)))


def chain_step_unrolls(method, noise_mode, collect=L.COLLECT_NONE):
    """The unroll depths bdl_chain_step offers for this combination."""
    return tuple(u for u in (1, 2, 4)
                 if L.lib().bdl_chain_step_unroll_ok(int(method), int(noise_mode), int(collect), u))


def chain_step_args(state, method, *, scalars, noise_mode, collect=L.COLLECT_NONE, mom1=None,
                    mom2=None, collect_a=1.0, collect_b=1.0, first_step=False, momentum=False,
                    seed=0, chain=0, step=0, div_mode=None, noise=None, blocks_per_chain=0,
                    unroll=0, nonfinite_per_chain=None):
    """The bdl_chain_step_args of a launch over `state` (see chain_step)."""
    a = L.ChainStepArgs()
    a.theta = state.theta.data_ptr()
    g = getattr(state, "grad", None)
    a.grad = None if g is None else g.data_ptr()
    gb = getattr(state, "chain_gbase", None)
    a.grad_base = None if gb is None else gb.data_ptr()
    nf = getattr(state, "nonfinite", None)
    a.nonfinite = None if nf is None else nf.data_ptr()
    if nonfinite_per_chain is None:
        nonfinite_per_chain = nf is not None and nf.numel() == int(state.K) and int(state.K) > 1
    a.nonfinite_per_chain = 1 if nonfinite_per_chain else 0
    a.mom = None if state.mom is None else state.mom.data_ptr()
    a.prior_mean = None if state.prior is None else state.prior.data_ptr()
    nz = noise if noise is not None else getattr(state, "noise", None)
    a.noise = None if nz is None else nz.data_ptr()
    a.mom1 = None if mom1 is None else mom1.data_ptr()
    a.mom2 = None if mom2 is None else mom2.data_ptr()
    a.runs = state.chain_runs.data_ptr()
    a.nruns = int(state.chain_nruns)
    a.scalars = scalars.data_ptr()
    a.n1, a.chain_groups, a.chains = int(state.n1), int(state.chain_groups), int(state.K)
    a.method, a.noise_mode, a.collect = int(method), int(noise_mode), int(collect)
    a.flags = ((L.FLAG_FIRST_STEP if first_step else 0) | (L.FLAG_MOMENTUM if momentum else 0)
               | _div_flag(div_mode))
    a.blocks_per_chain, a.unroll = int(blocks_per_chain), int(unroll)
    a.collect_a, a.collect_b = float(collect_a), float(collect_b)
    a.inv_collect_a, a.inv_collect_b = _inv(collect_a), _inv(collect_b)
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.chain = int(chain) & 0xFFFFFFFFFFFFFFFF
    a.step = int(step) & 0xFFFFFFFFFFFFFFFF
    return a


def chain_step(state, method, *, scalars, **kw):
    """One fused step of K stacked chains, each with its own hyperparameters
    (bdl_chain_step, include/bdl_chain_step.h).  `state`: the stacked vectors
    (theta, grad or None, mom, prior, noise, nonfinite), K, n1, chain_groups and
    ONE chain's run table in chain-local indices (chain_runs, chain_nruns;
    chain_gbase: the [K, nruns] gradient-base table or None) — a StackedState
    built with chain_tables=True.  `scalars`: a device [K, 12] float32 row
    block (L.CHAIN_SCALAR_COLUMNS; per_chain.csghmc_rows / sgld_rows), 16-B
    aligned; row k is chain k's lr, noise scale, 1 - alpha, prior_sig, sigma2,
    n_data, mu and reciprocals.  method: L.CSGHMC or L.SGLD.  One launch on the
    current stream, no host synchronisation, no copy.  blocks_per_chain 0: from
    K, n1 and the CU count (chain_step_blocks_per_chain); values never depend
    on it, nor on unroll."""
    K_ = int(state.K)
    if (scalars.dtype != torch.float32 or not scalars.is_cuda or not scalars.is_contiguous()
            or scalars.numel() != K_ * 12 or scalars.device != state.theta.device):
        raise ValueError("chain_step: scalars must be a contiguous float32 [K, 12] tensor on the "
                         "state's device")
    if not kw.get("blocks_per_chain"):
        kw["blocks_per_chain"] = chain_step_blocks_per_chain(state.n1, K_, state.theta.device,
                                                             kw.get("unroll") or 1)
    a = chain_step_args(state, method, scalars=scalars, **kw)
    dev = state.theta.device
    t = getattr(state, "timer", None)
    e0 = t.begin() if t is not None else None
    L.check(L.lib().bdl_chain_step(a, L.current_stream_handle(dev)), "bdl_chain_step")
    if e0 is not None:
        t.end(e0, alg_bytes_per_elem(a) * int(a.n1) * K_)


def philox_normal(n, seed, chain, step, device="cuda"):
    """The N(0,1) values the step kernel draws in Philox mode, as a tensor."""
    out = torch.empty(n, dtype=torch.float32, device=device)
    L.check(L.lib().bdl_philox_normal(out.data_ptr(), int(n), int(seed), int(chain), int(step),
                                      L.current_stream_handle(out.device)), "bdl_philox_normal")
    return out


_ACTIVE = [None]  # the geometry last installed through set_launch_config (None: defaults)
LIBRARY_DEFAULT = (2, 1, 1)  # what the library launches with before any set_launch_config


def set_launch_config(blocks_per_cu=0, unroll=0, grid_stride=0):
    _ACTIVE[0] = (int(blocks_per_cu), int(unroll), int(grid_stride))
    return L.lib().bdl_set_launch_config(int(blocks_per_cu), int(unroll), int(grid_stride))


def restore_launch_config(packed):
    """Re-install the geometry a set_launch_config call returned (packed as
    (grid_stride << 24) | (blocks_per_cu << 8) | unroll)."""
    return set_launch_config((packed >> 8) & 0xFFFF, packed & 0xFF, (packed >> 24) & 0xFF)


def _use_geometry(state, kind="step", sub=False):
    """Install the geometry tuned for this state's size and launch kind
    (state.launch_cfg for plain steps; state.collect_cfg for the steps that
    also read and update the posterior moments, state.init_cfg for a cycle's
    first collect, when tuned; else the plain step's) if another is active:
    the library's launch configuration is process-wide, and a process may hold
    states of very different sizes (e.g. a one-chain sampler and a stacked
    one)."""
    cfg = getattr(state, {"collect": "collect_cfg", "init": "init_cfg"}.get(kind, "launch_cfg"),
                  None)
    if cfg is None:
        cfg = getattr(state, "launch_cfg", None)
    if sub:
        # the overlap mode's per-bucket launches (FlatState.bucket_state) keep
        # the grid-stride order: the dynamic order is tuned on whole sweeps
        act = cfg or _ACTIVE[0]
        if act is not None and act[2] == L.ORDER_DYNAMIC:
            cfg = (act[0], act[1], L.ORDER_GRID_STRIDE)
    if cfg is not None and cfg != _ACTIVE[0]:
        set_launch_config(*cfg)


# Launch geometries worth trying on gfx950 (workgroups/CU, float4 groups in
# flight per lane, grid-stride): the sweep (profiles/round1/kernel_v1) shows the optimum
# moving between these from one device to the next.  The production kernels
# of every method (cSGHMC; SGLD / SGHMC / Adam with noise) exist at unroll
# depths 1, 2 and 4.
AUTOTUNE_CANDIDATES = ((2, 1, 1), (1, 4, 1), (3, 1, 1), (2, 4, 1), (1, 2, 1), (2, 2, 1))
# per sampler family, the geometries that won somewhere in the interleaved
# 13-geometry probe on a ViT-L/32 state (tools/geom_methods.py,
# profiles/round3/aux/geom_methods.jsonl): SGLD 3 x 4 by 0.5 % over 2 x 4;
# Adam-SGHMC 1 x 1 by 1.5 % and 4 x 4 by 0.3 % over 2 x 4 (seven streams: fewer
# accesses in flight per CU pay); cSGHMC 1 x 4 by >= 1.9 % over every other
AUTOTUNE_BY_METHOD = {
    # + 1 x 1 and 3 x 4: the bare access mix of the SGLD buffers ran 1 x 1 8 %
    # ahead of the tuned 2 x 1 at ResNet-101 size, and of the explore buffers
    # 3 x 4 first at ViT-L/32 size (bench.py mix_ceiling, profiles/round4/methods/)
    # + 1 x 1: the bare mix of the explore buffers ran fastest there on the
    # round-5 box (1.038 ms vs 1.064 for the kernel's tuned 1 x 4)
    # + every geometry again in the dynamic sweep order (order 2, include/bdl_order.h:
    # the cSGHMC sweeps only); installed only where it is the fastest on the chain's vectors
    "csghmc": (AUTOTUNE_CANDIDATES + ((3, 4, 1), (1, 1, 1))
               + tuple((b, u, L.ORDER_DYNAMIC)
                       for b, u, _ in AUTOTUNE_CANDIDATES + ((3, 4, 1), (1, 1, 1)))),
    "sgld": AUTOTUNE_CANDIDATES + ((3, 4, 1), (4, 4, 1), (1, 1, 1)),
    "adam": AUTOTUNE_CANDIDATES + ((1, 1, 1), (4, 4, 1)),
}
_TUNED = {}
_TUNED_COLLECT = {}
# the collect steps (the step plus the posterior-moment update: cSGHMC Welford
# m1 / M2, SGLD / Adam running m1 / m2 — four to six more streams) are tuned
# separately over the method's candidates plus 1 x 1: the cSGHMC Welford
# collect ran 1.778 ms at 1 x 1 vs 1.800 at the explore's 1 x 4 and >= 1.83 at
# every other geometry (tools/geom_methods.py METHODS=collect,
# profiles/round3/aux/geom_collect.jsonl; round 1's sweep: 1 x 1 best too)
COLLECT_EXTRA = ((1, 1, 1),)


ADAM_EXTRA = ("adam_m", "adam_v", "sgd_buf")  # adam_sghmc.Model.extra_vectors


def _scratch_launcher(n, dev, method):
    """A closure launching `method`'s production kernel over scratch buffers of
    n elements (the buffers live as long as the closure)."""
    return _scratch_launchers(n, dev, method)[0]


def _scratch_launchers(n, dev, method):
    """Closures launching `method`'s production kernel over scratch buffers of
    n elements — (plain step, collect step: the same with the posterior-moment
    update; its m1 / m2 are allocated at its first call, for cSGHMC as the
    Runner allocates a cycle's Welford pair) — the buffers live as long as the
    closures."""
    from .flat import FlatState, moment_pair
    st = FlatState.from_segments([("w", (int(n),))], None, device=dev,
                                 need_prior=method != "csghmc",
                                 extra=ADAM_EXTRA if method == "adam" else ())
    st.theta.zero_()
    if method == "csghmc":
        kw = dict(lrs=(1e-4, 1e-4), noise_scale=(0.0, 0.0), noise_mode=L.NOISE_NONE,
                  one_minus_alpha=0.9, prior_sig=1.0)

        def launch():
            sgmcmc_step(st, L.CSGHMC, **kw)
    elif method == "sgld":
        st.prior.zero_()
        kw = dict(lrs=(1e-4, 1e-4), noise_scale=(1e-3, 1e-3), noise_mode=L.NOISE_PHILOX,
                  sigma2=1.0, n_data=1e6, mu=0.5, momentum=True)

        def launch():
            sgmcmc_step(st, L.SGLD, **kw)
    elif method == "adam":
        st.prior.zero_()
        m, v, buf = (st.extra[k] for k in ADAM_EXTRA)
        kw = dict(adam_m=m, adam_v=v, sgd_buf=buf, beta1=0.9, beta2=0.999, eps=1e-8, t=3,
                  momentum_decay=0.1, nd=0.01, lrs=(1e-4, 1e-4), noise_mode=L.NOISE_PHILOX,
                  sigma2=1.0, n_data=1e6, mu=0.5, momentum=True)

        def launch():
            adam_step(st, L.ADAM_SGHMC, **kw)
    else:
        raise ValueError(f"unknown method {method!r}")
    moms = []

    def launch_collect():
        if not moms:
            moms.extend(moment_pair(int(n), dev) if method == "csghmc" else
                        (torch.zeros_like(st.theta), torch.zeros_like(st.theta)))
            moms[0].copy_(st.theta)
            moms[1].zero_()
        if method == "csghmc":
            sgmcmc_step(st, L.CSGHMC, lrs=(1e-4, 1e-4), noise_scale=(1e-7, 1e-7),
                        noise_mode=L.NOISE_PHILOX, one_minus_alpha=0.9, prior_sig=1.0,
                        collect=L.COLLECT_WELFORD, mom1=moms[0], mom2=moms[1], collect_a=3.0)
        elif method == "sgld":
            sgmcmc_step(st, L.SGLD, collect=L.COLLECT_MEAN, mom1=moms[0], mom2=moms[1],
                        collect_a=2.0, collect_b=3.0, **kw)
        else:
            adam_step(st, L.ADAM_SGHMC, collect=L.COLLECT_MEAN, mom1=moms[0], mom2=moms[1],
                      collect_a=2.0, collect_b=3.0, **kw)
    return launch, launch_collect


def _device(device):
    return torch.device(device) if device is not None else torch.device(
        "cuda", torch.cuda.current_device())


def autotune(n, device=None, reps=6, candidates=None, method="csghmc", collect=False):
    """Pick the fastest launch geometry for an n-element sweep on this device.

    The update of every element is independent of the launch geometry (noise
    is keyed by element index), so the choice changes speed only, never
    results.  Times the method's production kernel (cSGHMC exploration; SGLD
    + SGD momentum with Philox noise; Adam-SGHMC + SGD momentum) on scratch
    buffers (freed afterwards) and installs the winner process-wide.  Returns
    (config, {config: ms}); with collect=True, (config, {config: ms},
    collect config, {config: ms}) — the collect step tuned on the same
    scratch state over the candidates plus COLLECT_EXTRA (not installed)."""
    import numpy as np
    dev = _device(device)
    if candidates is None:
        candidates = AUTOTUNE_BY_METHOD.get(method, AUTOTUNE_CANDIDATES)
    launch, launch_collect = _scratch_launchers(n, dev, method)

    def pick(fn, cands):
        # round 1: every candidate; round 2: the three fastest again with twice
        # the repetitions, averaged with round 1 (damps the +-1-2 % burst-to-burst noise)
        times = measure(fn, cands, reps)
        top = sorted(times, key=times.get)[:3]
        again = measure(fn, top, 2 * reps)
        for cfg in top:
            times[cfg] = 0.5 * (times[cfg] + again[cfg])
        return min(top, key=times.get), times

    def measure(fn, cfgs, k):
        out = {}
        for cfg in cfgs:
            set_launch_config(*cfg)
            for _ in range(2):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(k)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize(dev)
            out[cfg] = float(np.median([a.elapsed_time(b) for a, b in ev]))
        return out

    best, times = pick(launch, candidates)
    res = (best, times)
    if collect:
        cbest, ctimes = pick(launch_collect, tuple(candidates) + tuple(
            c for c in COLLECT_EXTRA if c not in candidates))
        res = (best, times, cbest, ctimes)
    set_launch_config(*best)
    del launch, launch_collect
    torch.cuda.empty_cache()
    return res


TUNE_ON_STATE_MIN = 1 << 16  # smaller states keep the default geometry
TUNE_SNAPSHOT_FRACTION = 0.25  # the tuning's snapshot of the written vectors, at most this share of free HBM


def request_state_tuning(state, method):
    """Tune `state`'s launch geometry on its OWN buffers at the first full
    launch of each kind (the plain step; the collect step), with that launch's
    own arguments, restoring every vector it writes after each candidate (so
    the chain is unchanged; the update never depends on geometry anyway).
    Why not scratch vectors (autotune): which geometry is fastest depends on
    where the vectors sit in HBM — on one box the SGLD sweep over ResNet-101
    ran 2 x 4 fastest on scratch vectors while the bare access mix of the
    chain's own buffers ran 1 x 1 8 % ahead of it, and the Adam sweep's best
    moved from 2 x 4 to 1 x 4 (bench.py mix_ceiling, profiles/round4/methods_b/).
    cSGHMC: every geometry is tried in the grid-stride and in the dynamic sweep
    order (AUTOTUNE_BY_METHOD), and the dynamic order is installed, per kind,
    only where it is the fastest here.  BDL_AUTOTUNE=0: the defaults."""
    if os.environ.get("BDL_AUTOTUNE", "1") == "0" or int(state.n) < TUNE_ON_STATE_MIN:
        return
    state._tune_pending = {"step", "collect", "init"}
    state._tune_method = method
    state.tuned = {}


def _tune_kind(state, fn, kind, written):
    state._tune_pending.discard(kind)
    cands = tuple(AUTOTUNE_BY_METHOD.get(state._tune_method, AUTOTUNE_CANDIDATES))
    if kind != "step":
        cands += tuple(c for c in COLLECT_EXTRA if c not in cands)
    nf = getattr(state, "nonfinite", None)
    written = list(written) + ([nf] if nf is not None else [])
    # the snapshot of what the launch writes must fit comfortably: otherwise
    # keep the current geometry (a model this large is tuned on nothing)
    need = sum(w.numel() * w.element_size() for w in written)
    free, _ = torch.cuda.mem_get_info(state.device)
    if need > TUNE_SNAPSHOT_FRACTION * free:
        state.tuned[kind] = {"skipped": f"snapshot {need >> 20} MiB > "
                                        f"{TUNE_SNAPSHOT_FRACTION:g} x free {free >> 20} MiB"}
        return
    best, times = tune_on_state(fn, written, cands, state.device)
    setattr(state, {"collect": "collect_cfg", "init": "init_cfg"}.get(kind, "launch_cfg"), best)
    state.tuned[kind] = {"best": best,
                         "ms": {f"{c[0]}wg/cu x{c[1]}" + (" dynamic" if c[2] == L.ORDER_DYNAMIC
                                                          else ""): round(t, 4)
                                for c, t in times.items()}}


def tune_on_state(launch, written, candidates, device, reps=4):
    """Time `launch` (a zero-argument launch over a state's own buffers) at
    each candidate geometry — round 1 every candidate, round 2 the three
    fastest again with twice the repetitions, averaged — restoring the
    `written` tensors after every candidate.  Returns (best, {cfg: ms}); the
    previous geometry is re-installed."""
    import numpy as np
    saved = [w.clone() for w in written]
    prev = _ACTIVE[0]
    ts = torch.cuda.current_stream(device)  # the stream `launch` enqueues on

    def measure(cfgs, k):
        out = {}
        for cfg in cfgs:
            set_launch_config(*cfg)
            launch()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(k)]
            for e0, e1 in ev:
                e0.record(ts)
                launch()
                e1.record(ts)
            torch.cuda.synchronize(device)
            out[cfg] = float(np.median([x.elapsed_time(y) for x, y in ev]))
            for w, s in zip(written, saved):
                w.copy_(s)
        return out

    try:
        times = measure(candidates, reps)
        top = sorted(times, key=times.get)[:3]
        again = measure(top, 2 * reps)
        for cfg in top:
            times[cfg] = 0.5 * (times[cfg] + again[cfg])
        best = min(top, key=times.get)
    finally:
        for w, s in zip(written, saved):
            w.copy_(s)
        del saved
        if prev is not None:
            set_launch_config(*prev)
    return best, times


def prewarm(n, device=None, method="csghmc", seconds=2.5):
    """Run the method's kernel back to back on scratch buffers for `seconds`
    (untimed setup before a measurement): the GPU's clocks ramp over the first
    ~0.8 s of sustained load (tools/drift.py, round 5: 1.058 ms per ViT-L/32
    explore sweep in the first 0.25 s, 1.032-1.035 from ~0.8 s on), so a
    short measurement from idle would read the ramp, not the steady state.
    Returns the number of launches."""
    import time
    dev = _device(device)
    launch = _scratch_launcher(n, dev, method)
    t_end, k = time.perf_counter() + float(seconds), 0
    while time.perf_counter() < t_end:
        for _ in range(20):
            launch()
        k += 20
        torch.cuda.synchronize(dev)
    del launch
    torch.cuda.empty_cache()
    return k


def autotune_once(n, device, method):
    """autotune() (plain and collect steps) once per (n, device, method) in this
    process; later calls only re-install the cached winner.  Returns the plain
    step's geometry (collect_config: the collect step's).  BDL_AUTOTUNE=0
    keeps the defaults."""
    if os.environ.get("BDL_AUTOTUNE", "1") == "0":
        return None
    key = (int(n), str(device), method)
    if key not in _TUNED:
        best, _, cbest, _ = autotune(n, device, method=method, collect=True)
        _TUNED[key], _TUNED_COLLECT[key] = best, cbest
    else:
        set_launch_config(*_TUNED[key])
    return _TUNED[key]


def collect_config(n, device, method):
    """The collect step's geometry autotune_once found for (n, device, method),
    or None (not tuned: the plain step's geometry is used)."""
    return _TUNED_COLLECT.get((int(n), str(device), method))
