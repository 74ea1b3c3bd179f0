"""Stacked chains: K independent SG-MCMC chains of one network on one device.

The reference runs one chain per process (methods/csghmc.py:41); its own
recipe for more chains is more processes.  On an MI355X a small network
leaves the device idle between launches, so K chains here share every
launch instead:

  * the K chains' flat vectors are stacked chain-major in one buffer
    (`theta[k]` = parameters_to_vector of chain k, padded to a multiple of 4
    elements so every chain starts on a float4 group);
  * forward and backward run once for all chains, `torch.func.vmap` over
    `functional_call` with the chains' parameters as strided views of the
    stacked theta (the data batch shared, or one batch per chain);
  * ONE fused update launch (`bdl_sgmcmc_step` with `chain_groups`, ABI v6)
    covers all chains, reading each chain's gradient in place from the vmapped
    gradient tensors through the per-run base table (one run per chain and
    tensor), with the Welford collect of methods/csghmc.py:327-345 fused.

Chain k draws the Philox noise of a one-chain sampler with chain id
`chain0 + k` (same seed, same step keys): its update equals the one-chain
update bit for bit given the same gradient (tests/test_gpu_stacked.py).  The
gradients come from batched GEMMs, so a stacked chain agrees with a separately
run chain to rounding, not bitwise.

Scope: StackedCSGHMC (the north-star sampler: cyclical schedule, thinning,
per-cycle Welford moments), StackedSGLD (SGLD + SGD momentum, prior mean
theta0, burn-in, thinned running moments), StackedSGHMC (the same loop with
the SGHMC momentum update), StackedCSGLD (cyclical SGLD, per-cycle running
moments), StackedAdamSGHMC (Adam-preconditioned SGHMC under SGLD's loop) and
StackedAdamCSGHMC (its cyclical variant, Adam state reset at every cycle end);
the cyclical SGLD / Adam samplers honour args.clip_grad per chain, each chain by
the norm of its own gradient (kernels.chain_clip).  The predictive averages
probabilities uniformly over chains and (nst posterior draws of) the collected
components.  Networks with BatchNorm running statistics are refused (vmap cannot
update shared buffers per chain), and every trainable parameter must take part
in the forward pass (torch.func returns zeros, not None, for unused inputs).
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np
import torch
import torch.nn.functional as F
from torch.func import functional_call, grad_and_value, vmap

from . import _lib as L
from . import ess as ESS
from . import kernels as K
from . import per_chain as PC
from ._base import no_gc
from ._runner import EVAL_STEP_BASE
from .cyclical import CyclicalSGMCMC
from .flat import MAX_TENSOR_RUNS, build_runs, segment_attrs


def _upload_table(device, *parts):
    """Rows -> one pinned int64 host table (the parts, flattened, end to end)
    -> one non-blocking upload.  Returns the flat device tensor."""
    flat = [np.asarray(p, dtype=np.int64).reshape(-1) for p in parts]
    host = torch.empty(sum(f.size for f in flat), dtype=torch.int64).pin_memory()
    np.concatenate(flat, out=host.numpy())
    return host.to(device, non_blocking=True)


def _cached_table(cache, key, build, keep=8):
    """cache[key], built on a miss; the oldest of `keep` entries makes room."""
    tab = cache.get(key)
    if tab is None:
        tab = build()
        if len(cache) >= keep:
            cache.pop(next(iter(cache)))
        cache[key] = tab
    return tab


class StackedState:
    """K chains' flat cSGHMC state of one network, stacked chain-major.

    theta2d / mom2d are [K, stride] (stride = n rounded up to 4); `params`
    maps every parameter name to its [K, *shape] strided view of theta2d.  The
    launchable attributes (theta, grad / gbase, mom, runs, nruns, n,
    chain_groups, nonfinite) are what kernels._step_args reads."""

    def __init__(self, net, K_, *, readout_name=None, bias="informative", init="copy",
                 seed=0, need_mom=True, need_prior=False, net0=None, chain_tables=False):
        import torch.nn as nn
        # chain_tables: describe the launch per chain (kernels.chain_step): ONE
        # chain's run table in chain-local indices (chain_runs, chain_nruns)
        # and a [K, nruns] gradient-base table (chain_gbase), one divergence
        # flag per chain
        self.chain_tables = bool(chain_tables)
        if K_ < 1:
            raise ValueError("StackedState: K must be >= 1")
        for m in net.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.track_running_stats:
                raise ValueError("StackedState: BatchNorm running statistics cannot be stacked "
                                 "(use track_running_stats=False or one chain per process)")
        named = list(net.named_parameters())
        if not named:
            raise ValueError("StackedState: the network has no parameters")
        dev = named[0][1].device
        for nm, p in named:
            L.require_hip(p.data, f"parameter {nm!r}")
        self.K = int(K_)
        self.device = dev
        self.names = [nm for nm, _ in named]
        self.shapes = [tuple(p.shape) for _, p in named]
        self.numels = [p.numel() for _, p in named]
        self.offsets = np.concatenate([[0], np.cumsum(self.numels)[:-1]]).astype(np.int64).tolist()
        self.n1 = int(sum(self.numels))
        self.stride = (self.n1 + 3) // 4 * 4
        self.n = self.K * self.stride
        self.chain_groups = self.stride // 4
        if (self.n + 3) // 4 >= 1 << 32:
            raise ValueError("StackedState: K * n too large for stacked Philox keys")
        self.requires_grad = [p.requires_grad for _, p in named]
        self.readout_name = readout_name if readout_name is not None else getattr(
            net, "readout_name", None)
        self.attrs = segment_attrs(self.names, self.readout_name, bias, self.requires_grad)

        f32 = dict(dtype=torch.float32, device=dev)
        self.theta2d = torch.zeros(self.K, self.stride, **f32)
        with torch.no_grad():
            src = torch.cat([p.detach().reshape(-1).float() for _, p in named])
            self.theta2d[:, :self.n1].copy_(src)
            if init == "reinit":
                import copy
                from ._runner import reinit_network
                tmp = copy.deepcopy(net)
                for k in range(self.K):
                    with torch.random.fork_rng(devices=[dev] if dev.type == "cuda" else []):
                        torch.manual_seed(int(seed) + k)
                        reinit_network(tmp)
                    self.theta2d[k, :self.n1].copy_(
                        torch.cat([p.detach().reshape(-1) for p in tmp.parameters()]))
            elif init != "copy":
                raise ValueError("StackedState: init must be 'copy' or 'reinit'")
        self.theta = self.theta2d.view(-1)
        self.mom2d = torch.zeros(self.K, self.stride, **f32) if need_mom else None
        self.mom = None if self.mom2d is None else self.mom2d.view(-1)
        self.noise = None
        # prior mean theta0 (SGLD): net0's parameters (zeros without one) in
        # every chain's slot
        self.prior = None
        if need_prior:
            p2 = torch.zeros(self.K, self.stride, **f32)
            if net0 is not None:
                p0 = [q.detach().reshape(-1).float() for q in net0.parameters()]
                if [q.numel() for q in p0] != self.numels:
                    raise ValueError("StackedState: net0 does not match net's parameter shapes")
                with torch.no_grad():
                    p2[:, :self.n1].copy_(torch.cat(p0).to(dev))
            self.prior = p2.view(-1)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=dev)
        self.params = {nm: self.theta2d[:, o:o + k].view(self.K, *s)
                       for nm, o, k, s in zip(self.names, self.offsets, self.numels, self.shapes)}
        # gradient source: per-run bases into the vmapped gradient tensors
        # ("tensor"), or a stacked gradient vector the gradients are copied into
        # ("flat", when K x tensors runs would not fit the LDS run table)
        gap = 1 if self.stride > self.n1 else 0
        self.grad_mode = "tensor" if self.K * (len(self.names) + gap) <= MAX_TENSOR_RUNS else "flat"
        self.grad, self.gbase, self._tables = None, None, {}
        self._gbound, self._seg_tables = None, {}  # grad_segments: what use_grads bound last
        self._stat_tables = {}                     # stat_segments, per bound gradient set
        self._layer_table = None                   # layer_segments: built once
        self.chain_runs, self.chain_nruns, self.chain_gbase = None, 0, None
        if self.chain_tables:
            # one run per tensor whatever K is: the in-place form serves any K
            self.grad_mode = "tensor" if len(self.names) <= L.CHAIN_STEP_MAX_RUNS_BASES else "flat"
            self.nonfinite = torch.zeros(self.K, dtype=torch.int32, device=dev)
            self.runs, self.nruns = None, 0
            if self.grad_mode == "flat":
                self.grad2d = torch.zeros(self.K, self.stride, **f32)
                self.grad = self.grad2d.view(-1)
                self.chain_runs = build_runs(self.offsets, self.numels, self.attrs, self.n1).to(dev)
                self.chain_nruns = int(self.chain_runs.shape[0])
        elif self.grad_mode == "flat":
            self.grad2d = torch.zeros(self.K, self.stride, **f32)
            self.grad = self.grad2d.view(-1)
            offs, nums, ats = [], [], []
            for k in range(self.K):
                for o, kk, a in zip(self.offsets, self.numels, self.attrs):
                    offs.append(k * self.stride + o)
                    nums.append(kk)
                    ats.append(a)
            self.runs = build_runs(offs, nums, ats, self.n).to(dev)
            self.nruns = int(self.runs.shape[0])
        else:
            self.runs, self.nruns = None, 0
        self.timer = None
        self.extra = {}

    def chain_vector(self, k):
        """parameters_to_vector of chain k (a view)."""
        return self.theta2d[k, :self.n1]

    def load_chain(self, net, k):
        """Copy chain k's parameters into `net` (same architecture)."""
        with torch.no_grad():
            for p, o, n in zip(net.parameters(), self.offsets, self.numels):
                p.copy_(self.theta2d[k, o:o + n].view(p.shape))

    def use_grads(self, grads):
        """Point the next launch at the vmapped gradients {name: [K, *shape]}
        (None or a missing name: that tensor is frozen / has no gradient)."""
        gl = [grads.get(nm) for nm in self.names]
        if self.grad_mode == "flat":
            for g, o, k in zip(gl, self.offsets, self.numels):
                if g is not None:
                    self.grad2d[:, o:o + k].copy_(g.reshape(self.K, k))
            self._gbound = tuple(g is not None for g in gl)
            return
        ptrs = []
        for g, k in zip(gl, self.numels):
            if g is None:
                ptrs.append(0)
                continue
            if (g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous()
                    or g.numel() != self.K * k):
                raise ValueError("StackedState: gradients must be contiguous fp32 [K, *shape]")
            ptrs.append(g.data_ptr())
        key = self._gbound = tuple(ptrs)
        build = self._build_chain_table if self.chain_tables else self._build_table
        tab = _cached_table(self._tables, key, lambda: build(ptrs))
        if self.chain_tables:
            self.chain_runs, self.chain_nruns, self.chain_gbase = tab
        else:
            self.runs, self.nruns, self.gbase = tab

    def _build_chain_table(self, ptrs):
        """The per-chain form (include/bdl_chain_step.h): ONE chain's runs in
        chain-local indices, one per tensor and no padding run (the launch
        ends at n1), and a [K, nruns] base table whose row k holds
        &g_t[k, 0] - 4 * offset_t; a tensor for which any chain's base is not
        16-byte addressable is marked GUNALIGNED in the shared run table."""
        rows, bases = [], np.zeros((self.K, len(ptrs)), dtype=np.int64)
        for i, (o, n, a, ptr) in enumerate(zip(self.offsets, self.numels, self.attrs, ptrs)):
            at = a | (0 if ptr else L.ATTR_SKIP)
            if ptr:
                b = ptr + 4 * n * np.arange(self.K, dtype=np.int64) - 4 * o
                bases[:, i] = b
                if (b % 16).any():
                    at |= L.ATTR_GUNALIGNED
            rows.append((o + n, at))
        nt = len(rows)
        dev = _upload_table(self.device, rows, bases)
        return dev[:2 * nt].view(nt, 2), nt, dev[2 * nt:].view(self.K, nt)

    def _build_table(self, ptrs):
        """One run per (chain, tensor) — a run must not span two gradient
        tensors — plus a SKIP run over each chain's padding; chain k of tensor
        i reads ptrs[i] + 4*(k*numel_i + j), i.e. base = that - 4*(flat index)."""
        rows, bases = [], []
        for k in range(self.K):
            for o, n, a, ptr in zip(self.offsets, self.numels, self.attrs, ptrs):
                start = k * self.stride + o
                base = ptr + 4 * k * n - 4 * start if ptr else 0
                at = a | (0 if ptr else L.ATTR_SKIP)
                if ptr and base % 16:
                    at |= L.ATTR_GUNALIGNED
                rows.append((start + n, at))
                bases.append(base)
            if self.stride > self.n1:
                rows.append(((k + 1) * self.stride, L.ATTR_SKIP))
                bases.append(0)
        nt = len(rows)
        dev = _upload_table(self.device, rows, bases)
        return dev[:2 * nt].view(nt, 2), nt, dev[2 * nt:]

    def grad_segments(self):
        """(device table, nsegments) of kernels.chain_clip for the gradients
        `use_grads` last bound: one (base address, numel, chain stride) row per
        tensor that has a gradient (include/bdl_clip.h) — the vmapped
        [K, *shape] tensor itself ("tensor" mode: stride = numel) or its span
        of the stacked gradient vector ("flat": stride = the chain slot).  A
        frozen tensor / a missing gradient gets no row, a chain's padding lies
        in none.  Cached per set of gradient addresses, as the run tables."""
        key = self._gbound
        if key is None:
            raise ValueError("StackedState: grad_segments before use_grads")

        def build():
            if self.grad_mode == "flat":
                rows = [(self.grad.data_ptr() + 4 * o, n, self.stride)
                        for o, n, have in zip(self.offsets, self.numels, key) if have]
            else:
                rows = [(ptr, n, n) for n, ptr in zip(self.numels, key) if ptr]
            if not rows:
                raise ValueError("StackedState: no tensor has a gradient to clip")
            return _upload_table(self.device, rows).view(len(rows), 3), len(rows)

        return _cached_table(self._seg_tables, key, build)

    def stat_segments(self):
        """(device table, nsegments, tensor indices) of kernels.chain_stats for
        the gradients `use_grads` last bound: one (gradient base, numel,
        gradient chain stride, chain-local offset, lr group) row per tensor
        that has a gradient (include/bdl_stats.h); the gradient addressed as in
        `grad_segments`, the lr group 1 for the readout (ATTR_HEAD), else 0.  A
        frozen tensor / a missing gradient gets no row, a chain's padding lies
        in none.  Cached per set of gradient addresses, as the run tables."""
        key = self._gbound
        if key is None:
            raise ValueError("StackedState: stat_segments before use_grads")

        def build():
            flat = self.grad_mode == "flat"
            idx = [i for i, have in enumerate(key) if have]
            if not idx:
                raise ValueError("StackedState: no tensor has a gradient to take statistics of")
            rows = [(self.grad.data_ptr() + 4 * self.offsets[i] if flat else key[i],
                     self.numels[i], self.stride if flat else self.numels[i], self.offsets[i],
                     1 if self.attrs[i] & L.ATTR_HEAD else 0) for i in idx]
            return _upload_table(self.device, rows).view(len(rows), 5), len(rows), tuple(idx)

        return _cached_table(self._stat_tables, key, build)

    def layer_segments(self):
        """The device table of kernels.chain_diag_layers / chain_ess_layers: one
        (chain-local offset, numel) int64 row per tensor of `names`, in
        parameter order, frozen tensors included (include/bdl_layers.h); a
        chain's padding lies in no row.  It depends on nothing that changes:
        built once."""
        if self._layer_table is None:
            rows = list(zip(self.offsets, self.numels))
            self._layer_table = _upload_table(self.device, rows).view(len(rows), 2)
        return self._layer_table

    def diverged(self, reset=True):
        bad = bool(self.nonfinite.any().item())
        if bad and reset:
            self.nonfinite.zero_()
        return bad

    def diverged_chains(self, reset=True):
        """The chains that wrote a non-finite theta (per-chain flags:
        chain_tables); with one shared flag, all chains or none."""
        nf = self.nonfinite.cpu().numpy() != 0
        if nf.any() and reset:
            self.nonfinite.zero_()
        return [k for k in range(self.K) if nf[k if nf.size == self.K else 0]]


def st_big(st):
    """Worth tuning the launch geometry for (small sweeps are launch-bound)."""
    return st.device.type == "cuda" and st.n >= 1 << 20


DETECTION_SCORES = ("entropy", "mutual_info", "expected_entropy", "neg_confidence", "disagree")


def _single_process(what):
    """uncertainty / fit_temperature describe this process's chains only."""
    from . import chains
    if chains.world() > 1:
        raise ValueError(f"{what}: the report describes this process's chains only, and "
                         f"{chains.world()} processes share the predictive (run it in one "
                         "process, or per process on its own chains before init)")


def cycle_weights(cycle_likelihoods, keys, by_chain=True):
    """float64 [len(keys), K] mixture weights of the cycles `keys` from
    {cycle: float64 [draws, K] likelihoods} (score_cycle).  by_chain=True: every
    chain gets the reference's w_c = 1 / mean_j(1 / lik_j), normalised over ITS
    cycles (_runner.gmm_weights on the chain's column: K Runners).
    by_chain=False: normalised jointly over all (cycle, chain), as
    chains.chain_gmm_weights does over processes; uniform when no weight is
    positive."""
    from ._runner import gmm_weights
    keys = list(keys)
    if not keys:
        raise ValueError("component_weights: nothing is collected yet")
    for c in keys:
        if c not in cycle_likelihoods:
            raise ValueError(f"component_weights: cycle {c} has not been scored (score_cycle)")
    lik = {c: np.asarray(cycle_likelihoods[c], dtype=np.float64) for c in keys}
    K_ = lik[keys[0]].shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        if by_chain:
            out = np.empty((len(keys), K_), dtype=np.float64)
            for k in range(K_):
                w = gmm_weights({c: list(lik[c][:, k]) for c in keys})
                out[:, k] = [w[c] for c in keys]
            return out
        raw = np.stack([1.0 / np.mean(1.0 / lik[c], axis=0) for c in keys])
    tot = raw.sum()
    if not tot > 0:
        return np.full(raw.shape, 1.0 / raw.size)
    return raw / tot


class _StackedSampler:
    """What every stacked sampler shares: K chains' state, the vmapped
    forward/backward (optionally replayed from a HIP graph), the predictive
    over chains and collected posterior components, the epoch driver."""

    need_prior = False
    tune_method = "csghmc"  # the production kernel autotune_once times
    # per-chain clip_grad_norm_ threshold (the cyclical SGLD / Adam samplers set
    # it from args.clip_grad) and the [K, 2] (norm, coef) device table of the
    # last clipped step
    clip_grad = None
    last_clip = None
    _clip_ws = None

    # the family of per-chain hyperparameters this sampler sweeps
    # (per_chain.NAMES), None where no per-chain launch exists
    per_chain_family = None
    per_chain = None   # {name: float64 [K]} over the family's names, or None (uniform)
    swept = ()         # the names the caller gave

    # the likelihood-weighted cycle mixture (cyclical samplers): score every
    # finished cycle in train() (args.gmm_weights), and {cycle: float64
    # [draws, K] likelihoods} of `score_cycle`
    cyclical = False
    gmm_weights = False
    cycle_likelihoods = None

    def _init_per_chain(self, per_chain, K_, args):
        """Validate `per_chain` before anything touches the device."""
        if per_chain is None or len(per_chain) == 0:
            return
        fam = self.per_chain_family
        if fam is None:
            raise ValueError(f"{type(self).__name__}: per_chain is not supported (the per-chain "
                             "launch covers cSGHMC and SGLD / cSGLD; SGHMC and the Adam samplers "
                             "share one set of hyperparameters)")
        if isinstance(self, StackedCSGLD) and getattr(args, "clip_grad", None) is not None:
            raise ValueError(f"{type(self).__name__}: per_chain cannot be combined with clip_grad "
                             "(the clipped step has no per-chain launch)")
        self.per_chain = PC.parse(per_chain, K_, fam, PC.defaults(args, fam))
        self.swept = tuple(nm for nm in PC.NAMES[fam] if nm in per_chain)

    def __init__(self, net, K_, args, *, chain0=None, seed=None, init="copy", criterion=None,
                 per_chain_batches=False, logger=None, graph=None, net0=None, per_chain=None,
                 health_every=0, ess_batch=0, fn_probe=None, fn_batch=0, exchange_every=0,
                 exchange_var=0.0):
        from . import chains
        from ._base import default_compute_dtype, default_graph, refuse_compute_dtype
        refuse_compute_dtype(getattr(args, "compute_dtype", None) or default_compute_dtype(),
                             "the stacked samplers (bayesdll_amd.stacked)")
        self._check_exchange_sampler(exchange_every)
        self._init_per_chain(per_chain, K_, args)
        self._init_exchange(exchange_every, exchange_var, K_, per_chain_batches, net, args)
        self.gmm_weights = bool(getattr(args, "gmm_weights", False))
        if self.gmm_weights and not self.cyclical:
            raise ValueError(f"{type(self).__name__}: gmm_weights weighs the cycles of a cyclical "
                             "sampler (StackedCSGHMC, StackedCSGLD, StackedAdamCSGHMC); this one "
                             "collects one component")
        self.cycle_likelihoods = {}
        if int(health_every) != health_every or int(health_every) < 0:
            raise ValueError(f"health_every must be an integer >= 0 (got {health_every!r})")
        # batch length b of the batch-means ESS accumulators every collected
        # sample is folded into after `update` (0: never; then step() is
        # unchanged and nothing is allocated)
        self.ess_batch = ESS.check_batch(ess_batch)
        self._ess = None  # [{bsum, smean, sM2, bM2}, samples folded into the latest component]
        # function-space convergence: after `update` of every collect step the
        # chains' class probabilities on the probe batch fn_probe [P, ...] are
        # folded into batch-means accumulators of batch length fn_batch (None:
        # never; then step() is unchanged and nothing is allocated)
        self.fn_batch = ESS.check_batch(fn_batch, "fn_batch")
        if fn_probe is None:
            if self.fn_batch:
                raise ValueError(f"fn_batch = {self.fn_batch} needs a probe batch (fn_probe)")
        else:
            if not torch.is_tensor(fn_probe) or fn_probe.dim() < 1 or fn_probe.shape[0] < 1:
                raise ValueError("fn_probe must be a non-empty input batch [P, ...]")
            if self.fn_batch < 1:
                raise ValueError("fn_probe needs fn_batch = b >= 1, the batch length of the "
                                 f"batch-means accumulators (got {fn_batch!r})")
        self._fn = None  # {acc: {bsum, smean, sM2, bM2}, samples, chain_groups, probe, classes}
        # every m-th step the statistics sweep runs between gradients() and
        # update() (0: never; then step() is unchanged and nothing is allocated)
        self.health_every = int(health_every)
        self._health = None  # [acc [K, T, 6] float64, workspace, steps, tensor indices, bpc]
        self._rows_dev = None  # (epoch key, [batches, K, 12] device rows) of a per_chain epoch
        self.args, self.logger = args, logger
        # replay the vmapped forward/backward from a captured HIP graph (per
        # input shape): the vmap dispatch costs ~1.2 ms of host time per step
        self.graph = default_graph() if graph is None else bool(graph)
        self._graphs = {}
        hp = args.hparams
        self.net = net.to(args.device)
        self._fn_probe = None if fn_probe is None else fn_probe.detach().to(args.device)
        self.prior_sig = float(hp["prior_sig"])
        self.Ninflate, self.nd = float(hp["Ninflate"]), float(hp["nd"])
        self.thin, self.nst = int(hp["thin"]), int(hp["nst"])
        self.seed = int(getattr(args, "seed", 0) or 0) if seed is None else int(seed)
        self.chain0 = chains.rank() * K_ if chain0 is None else int(chain0)
        # re-initialisation seeds seed + chain id: distinct across processes too
        self.state = StackedState(self.net, K_, bias=str(hp["bias"]), init=init,
                                  seed=self.seed + self.chain0, need_prior=self.need_prior,
                                  net0=net0, chain_tables=self.per_chain is not None)
        self.K = K_
        # launch geometry tuned for the stacked size (speed only; the per-chain
        # launch has its own, kernels.chain_step_blocks_per_chain)
        if st_big(self.state) and self.per_chain is None:
            # (scratch on plain allocations, as the stacked state's own vectors)
            self.state.launch_cfg = K.autotune_once(self.state.n, self.state.device,
                                                    self.tune_method)
            if self.state.launch_cfg is not None:  # the collect steps' own geometry
                self.state.collect_cfg = K.collect_config(self.state.n, self.state.device,
                                                          self.tune_method)
        self.criterion = criterion or torch.nn.CrossEntropyLoss()
        if self.exchange_every:
            self._xstate = K.ExchangeState(K_, self.state.device)
            self._xbeta = torch.tensor(1.0 / self.per_chain["nd"] ** 2, dtype=torch.float64,
                                       device=self.state.device)
        self.step_count = 0
        self.draws = 0
        st = self.state
        self.trainable = [nm for nm, rg in zip(st.names, st.requires_grad) if rg]
        self.buffers = dict(self.net.named_buffers())
        xdim = 0 if per_chain_batches else None

        # the closures hold the module, not the sampler: no reference cycle,
        # so a dropped sampler (and its graphs) is freed at once, never by a
        # later garbage collection
        net_, bufs_, crit_ = self.net, self.buffers, self.criterion

        def loss_fn(tp, fp, x, y):
            out = functional_call(net_, ({**tp, **fp}, bufs_), (x,))
            return crit_(out, y), out

        self._grad = vmap(grad_and_value(loss_fn, has_aux=True),
                          in_dims=(0, 0, xdim, xdim), randomness="different")
        # evaluation: every chain sees the same batch
        self._fwd = vmap(lambda p, x: functional_call(net_, (p, bufs_), (x,)),
                         in_dims=(0, None), randomness="different")

    def _split(self):
        p = self.state.params
        return ({nm: p[nm] for nm in self.trainable},
                {nm: p[nm] for nm in p if nm not in self.trainable})

    # ----------------------------------------------------------------- step
    def gradients(self, x, y):
        """Vmapped forward/backward of all chains: ({name: [K, *shape]},
        loss [K], logits [K, B, C]).  In graph mode these are the graph's
        static outputs, overwritten by the next step."""
        if self.graph:
            return self._graphed_gradients(x, y)
        tp, fp = self._split()
        grads, (loss, out) = self._grad(tp, fp, x, y)
        return grads, loss.detach(), out.detach()

    def _graphed_gradients(self, x, y):
        """Capture once per input shape (after two warm-up runs on a side
        stream), then copy the batch into the static inputs and replay.  The
        graph reads the chains' parameters in place (views of the stacked
        theta), so the fused update between replays is seen by the next one."""
        key = (tuple(x.shape), x.dtype, tuple(y.shape), y.dtype)
        g = self._graphs.get(key)
        if g is None:
            import gc
            gc.collect()  # pending garbage (old graphs' pools) goes before the capture
            tp, fp = self._split()
            sx, sy = x.clone(), y.clone()
            side = torch.cuda.Stream(device=self.state.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._grad(tp, fp, sx, sy)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with no_gc(), torch.cuda.graph(graph):
                grads, (loss, out) = self._grad(tp, fp, sx, sy)
            g = self._graphs[key] = (graph, sx, sy, grads, loss.detach(), out.detach())
        graph, sx, sy, grads, loss, out = g
        sx.copy_(x)
        sy.copy_(y)
        graph.replay()
        return grads, loss, out

    def release_graphs(self):
        """Drop the captured graphs (and their memory pools) now, after the
        device has finished with them — not whenever a collection happens."""
        graphs, self._graphs = self._graphs, {}
        if graphs:
            torch.cuda.synchronize(self.state.device)
        graphs.clear()

    def step(self, x, y, *a, **kw):
        """One step of all K chains: vmapped forward/backward, then one fused
        launch (`update`).  Returns per-chain (loss [K], logits [K, B, C]) on
        the device, without a host sync."""
        grads, loss, out = self.gradients(x, y)
        if self.health_every and self.step_count % self.health_every == 0:
            kw = self._health_sweep(grads, a, kw)
        self.update(grads, *a, **kw)
        if self.ess_batch and kw.get("collect") is not None:
            self._ess_fold(kw["collect"][0])
        if self._fn_probe is not None and kw.get("collect") is not None:
            self._fn_fold()
        if self.exchange_every and self.step_count % self.exchange_every == 0:
            self._exchange_attempt(x, y)
        return loss, out

    # ------------------------------------------------------ replica exchange
    exchange_ok = False  # the samplers a temperature is derived for (SGLD / cSGLD)
    exchange_every = 0   # an exchange attempt after every m-th step (0: never)
    exchange_var = 0.0
    _xstate = _xbeta = None
    _xattempt = 0

    def _check_exchange_sampler(self, every):
        if int(every) != every or int(every) < 0:
            raise ValueError(f"exchange_every must be an integer >= 0 (got {every!r})")
        if every and not self.exchange_ok:
            raise ValueError(f"{type(self).__name__}: exchange_every needs a temperature per "
                             "chain, and none is derived for this sampler (cSGHMC, SGHMC and the "
                             "Adam samplers: only SGLD / cSGLD with momentum 0 sample "
                             "exp(-U / nd^2))")

    def _init_exchange(self, every, var, K_, per_chain_batches, net, args):
        """Validate replica exchange before anything touches the device: the K
        chains must be one target at K temperatures T_k = nd_k^2, and the
        energy of the exchange rule must be the one the update descends."""
        import torch.nn as nn
        from . import chains
        if not every:
            return
        who = f"{type(self).__name__}: exchange_every"
        bias = str(args.hparams["bias"])
        if bias != "informative":
            raise ValueError(f"{who}: bias={bias!r}: the update puts no prior on the bias "
                             "tensors, but the exchange energy sums (theta - theta0)^2 over every "
                             "element; only bias='informative' makes them the same target")
        frozen = [nm for nm, p in net.named_parameters() if not p.requires_grad]
        if frozen:
            raise ValueError(f"{who}: frozen tensors ({', '.join(frozen[:3])}"
                             f"{', ...' if len(frozen) > 3 else ''}): they are not sampled, yet "
                             "they would enter the energy and travel with a swap")
        drop = [nm for nm, m in net.named_modules() if isinstance(m, nn.modules.dropout._DropoutNd)]
        if drop:
            raise ValueError(f"{who}: dropout layers ({', '.join(drop[:3])}): the extra forward "
                             "would give a randomly masked energy and consume torch's generator")
        if not float(var) >= 0.0:
            raise ValueError(f"{who}: exchange_var must be >= 0 (got {var!r})")
        if self.per_chain is None:
            raise ValueError(f"{who} needs a per_chain table with an nd ladder (no per_chain: "
                             "every chain has the same temperature)")
        pc = self.per_chain
        if (pc["momentum"] != 0).any():
            raise ValueError(f"{who} needs momentum == 0: with SGD momentum chain k does not "
                             "sample exp(-U / nd_k^2)")
        for nm in ("prior_sig", "Ninflate"):
            if (pc[nm] != pc[nm][0]).any():
                raise ValueError(f"{who}: {nm} differs between chains, so their targets differ "
                                 "in more than temperature")
        nd = pc["nd"]
        if not (nd > 0).all():
            raise ValueError(f"{who}: every nd must be > 0 (T = nd^2 is a temperature)")
        d = np.diff(nd)
        if K_ > 1 and not ((d > 0).all() or (d < 0).all()):
            raise ValueError(f"{who}: nd must be strictly monotone in slot order (the ladder "
                             "order is the slot order)")
        if per_chain_batches:
            raise ValueError(f"{who}: one batch per chain (per_chain_batches): the energies of a "
                             "pair must come from the same batch")
        if chains.world() > 1:
            raise ValueError(f"{who}: {chains.world()} processes: the ladder is this process's "
                             "chains only")
        if K_ > L.EXCHANGE_MAX_CHAINS:
            raise ValueError(f"{who}: at most {L.EXCHANGE_MAX_CHAINS} chains")
        self.exchange_every, self.exchange_var = int(every), float(var)

    def _exchange_attempt(self, x, y):
        """One exchange attempt after `update`: an extra no_grad vmapped
        forward on the same batch gives every chain's mean loss at the updated
        theta (eager also in graph mode), then the three launches of
        include/bdl_exchange.h back to back.  No host read."""
        st = self.state
        crit = self.criterion
        with torch.no_grad():
            out = self._fwd(st.params, x)
            loss = torch.stack([crit(out[k], y) for k in range(self.K)]).float().contiguous()
        N = self.args.ND * float(self.per_chain["Ninflate"][0])
        ws = K.exchange_energy(st.theta, st.prior, chains=self.K, chain_groups=st.chain_groups,
                               n=st.n1)
        K.exchange_decide(self._xstate, ws, loss, self._xbeta, n=st.n1, n_data=N,
                          sigma2=float(self.per_chain["prior_sig"][0]) ** 2,
                          var=self.exchange_var, seed=self.seed, chain0=self.chain0,
                          attempt=self._xattempt)
        # momentum == 0 is required, so the launch neither reads nor writes the SGD
        # buffer: theta is the whole of a replica's state
        K.exchange_swap(self._xstate, [st.theta], chain_groups=st.chain_groups)
        self._xattempt += 1

    def cold_slots(self):
        """The slots whose nd is the minimum (the target's own temperature)."""
        if self.per_chain is None:
            raise ValueError("cold_slots: no per_chain table (every chain has the same nd)")
        nd = self.per_chain["nd"]
        return [int(k) for k in np.flatnonzero(nd == nd.min())]

    def exchange(self):
        """The replica-exchange record (one host read): per adjacent pair the
        attempts, accepts, rate and both temperatures; `replica` (which initial
        replica sits in which slot), `round_trips` per replica and in total,
        `refused` (attempts with a non-finite energy), `attempt` and `cold`."""
        if not self.exchange_every:
            raise ValueError("exchange: exchange_every is 0 (replica exchange is off)")
        d = self._xstate.summary()
        T = self.per_chain["nd"] ** 2
        if self._xstate.fresh:  # no attempt yet: the state is still zeros
            d["replica"] = np.arange(self.K)
        pairs = [{"slots": (i, i + 1), "attempts": int(d["attempts"][i]),
                  "accepts": int(d["accepts"][i]),
                  "rate": float(d["accepts"][i]) / max(1, int(d["attempts"][i])),
                  "temperatures": (float(T[i]), float(T[i + 1]))} for i in range(self.K - 1)]
        return {"pairs": pairs, "replica": [int(r) for r in d["replica"]],
                "round_trips": [int(r) for r in d["round_trips"]],
                "round_trips_total": int(d["round_trips"].sum()), "refused": d["refused"],
                "attempt": self._xattempt, "cold": self.cold_slots()}

    def _exchange_ckpt(self):
        """The exchange state for `_extra_state`, only when the option is on."""
        if not self.exchange_every:
            return {}
        return {"exchange_state": self._xstate.buf.clone(), "exchange_attempt": self._xattempt,
                "exchange_fresh": self._xstate.fresh}

    def _load_exchange_ckpt(self, d):
        if not self.exchange_every:
            return
        if "exchange_state" not in d:
            raise ValueError("load_ckpt: the checkpoint was written without exchange_every")
        self._xstate.buf.copy_(d["exchange_state"])
        self._xattempt, self._xstate.fresh = int(d["exchange_attempt"]), bool(d["exchange_fresh"])

    def _report_exchange(self, ep, rec, log):
        """run.py --exchange: one log line per evaluation and rec["exchange"]."""
        d = rec["exchange"] = self.exchange()
        rates = ", ".join(f"{p['slots'][0]}-{p['slots'][1]}: {p['accepts']}/{p['attempts']}"
                          for p in d["pairs"])
        log(f"(Epoch {ep}) replica exchange after {d['attempt']} attempts: accepted {rates}; "
            f"replica = {d['replica']}, round trips = {d['round_trips_total']}, refused = "
            f"{d['refused']}")

    # ------------------------------------------------------------------ ess
    def _ess_fold(self, kind):
        """Fold the theta this step's collect just accumulated into the
        batch-means accumulators (kernels.ess_fold: one launch, no host sync).
        An init collect opens a new component: the counters restart, so the
        accumulators always describe the latest component and a batch never
        straddles two (an open partial batch is dropped)."""
        st, e = self.state, self._ess
        if e is None:
            names = K.ESS_VECTORS if self.ess_batch > 1 else K.ESS_VECTORS[1:]
            e = self._ess = [{nm: torch.zeros_like(st.theta) for nm in names}, 0]
        if kind in (L.COLLECT_WELFORD_INIT, L.COLLECT_MEAN_INIT):
            e[1] = 0
        v = e[0]
        K.ess_fold(st.theta, v.get("bsum"), v["smean"], v["sM2"], v["bM2"], chains=self.K,
                   chain_groups=st.chain_groups, n=st.n1, sample=e[1] + 1, batch=self.ess_batch)
        e[1] += 1

    def ess(self, *, by_chain=False, ess=False, mcse=False, thresholds=None, by_tensor=False):
        """How many independent samples do the collected samples of the latest
        component stand for?  The batch-means effective sample size per
        element, pooled over the K chains the way R-hat pools the within-chain
        variance, from accumulators every collected sample was folded into
        (ess_batch = b: batches of b consecutive samples; bayesdll_amd.ess,
        include/bdl_ess.h) in one fused sweep (kernels.chain_ess).  Returns
        the summary (n_eval, n_degenerate, n_nonfinite, ess_min, argmin and
        its parameter name, ess_mean, n_below / share_below the thresholds —
        default 100 / 400 / 1000 —, samples folded and batches closed per
        chain, batch, chains, component) plus, when asked for, the [n1]
        tensors `ess` and `mcse` (the Monte Carlo standard error of one chain's
        mean from the pooled batch variance; the mean over all K chains has
        mcse / sqrt(K)).  by_chain=True: a list of K such results, chain k's from its own
        accumulators alone (K launches) — the only form under per_chain
        hyperparameters, whose chains target different posteriors.
        by_tensor=True: the result gains `by_tensor`, a list in parameter
        order of {name, numel, n_eval, n_degenerate, n_nonfinite, ess_min,
        argmin (chain-local, as the summary's), ess_mean, n_below,
        share_below} — the summary of each tensor alone, from one more fused
        sweep (kernels.chain_ess_layers) with no per-element output; with
        by_chain each of the K results carries its own table.

        The accumulators count true samples (no double count, no burn-in
        seed), restart at a component's init collect, are no part of
        state_dict / checkpoints and restart empty after load_ckpt.  Reads the
        accumulators only: nothing the sampler owns is written."""
        if not self.ess_batch:
            raise ValueError("ess: this sampler was built with ess_batch=0")
        if self.per_chain is not None and not by_chain:
            raise ValueError("ess: this sampler runs per_chain hyperparameters; the pooled ESS "
                             "pools chains that target ONE posterior, and these chains target "
                             "different ones (ask for by_chain=True)")
        thr = ESS.thresholds(thresholds)
        S_, nb = ESS.check_report(0 if self._ess is None else self._ess[1], self.ess_batch)
        st, v = self.state, self._ess[0]
        want = (("ess",) if ess else ()) + (("mcse",) if mcse else ())
        comp = self._latest_component()

        def report(sl, chains):
            res = K.chain_ess(v["sM2"][sl:], v["bM2"][sl:], chains=chains,
                              chain_groups=st.chain_groups, n=st.n1, samples=S_, batches=nb,
                              thresholds=thr, want=want)
            return res

        def finish(res, chains, sl):
            out = ESS.summary_dict(res.summary, thr, samples=S_, batches=nb,
                                   batch=self.ess_batch, chains=chains)
            out["component"] = comp
            out["argmin_param"] = self.param_of(out["argmin"]) if out["argmin"] >= 0 else None
            out.update({w: res[w] for w in want})
            if by_tensor:
                tab = K.chain_ess_layers(v["sM2"][sl:], v["bM2"][sl:], st.layer_segments(),
                                         chains=chains, chain_groups=st.chain_groups, n=st.n1,
                                         samples=S_, batches=nb, thresholds=thr)
                out["by_tensor"] = self._tensor_rows(tab, "ess_min", "argmin", "n_below",
                                                     "ess_mean", "share_below")
            return out

        if not by_chain:
            return finish(report(0, self.K), self.K, 0)
        launched = [report(k * st.stride, 1) for k in range(self.K)]  # K launches, then one wait
        return [finish(r, 1, k * st.stride) for k, r in enumerate(launched)]

    def _report_ess(self, ep, rec, log):
        """One log line (one per chain under per_chain) and rec["ess"] from
        `ess()` (run.py --ess); an evaluation that comes before two batches are
        closed says so and goes on."""
        try:
            d = self.ess(by_chain=self.per_chain is not None,
                         **({"by_tensor": True} if self._by_tensor() else {}))
        except ValueError as e:
            log(f"(Epoch {ep}) ESS: {e}")
            return
        rec["ess"] = d
        for k, r in enumerate(d if isinstance(d, list) else [d]):
            who = f"over {self.K} chains"
            if isinstance(d, list):
                who = f"chain {self.chain0 + k}: {PC.describe(self.per_chain, self.swept, k)}"
            shares = ", ".join(f"< {t:g}: {100 * s:.1f} %"
                               for t, s in zip(r["thresholds"], r["share_below"]))
            log(f"(Epoch {ep}) ESS {who}, component {r['component']} ({r['samples']} samples "
                f"each, {r['batches']} batches of {r['batch']}): min = {r['ess_min']:.1f} "
                f"({r['argmin_param']}), mean = {r['ess_mean']:.1f}, {shares}; "
                f"{r['n_eval']} evaluated, {r['n_degenerate']} degenerate, "
                f"{r['n_nonfinite']} non-finite")
            self._log_tensors(ep, log, f"ESS {who}", r, "ess_min", "ess_mean", "share_below",
                              "<", ".1f", worst=min)

    # ------------------------------------------------------- function space
    def _fn_fold(self):
        """Fold the chains' class probabilities on the probe batch, at the
        theta this step's collect just accumulated, into the function-space
        accumulators: one no-grad forward of the K chains and one launch
        (kernels.fn_fold), no host sync.  The counters run over the whole run:
        predictions, unlike the per-cycle Gaussians, are comparable across
        components."""
        lg = self.chain_logits(self._fn_probe)
        if lg.dim() != 3:
            raise ValueError("fn_probe: the network must map the probe batch to [P, classes] "
                             f"logits (got {tuple(lg.shape[1:])} per chain)")
        lg = lg.float().contiguous()
        f = self._fn
        if f is None:
            _, P, Cn = (int(v) for v in lg.shape)
            cg = (P * Cn + 3) // 4
            names = K.ESS_VECTORS if self.fn_batch > 1 else K.ESS_VECTORS[1:]
            acc = {nm: torch.zeros(self.K * 4 * cg, dtype=torch.float32, device=lg.device)
                   for nm in names}
            f = self._fn = {"acc": acc, "samples": 0, "chain_groups": cg, "probe": P,
                            "classes": Cn}
        v = f["acc"]
        K.fn_fold(lg, v.get("bsum"), v["smean"], v["sM2"], v["bM2"], sample=f["samples"] + 1,
                  batch=self.fn_batch, chain_groups=f["chain_groups"])
        f["samples"] += 1

    def function_space_reset(self):
        """Empty the function-space accumulators: the next fold is a first sample."""
        if self._fn is not None:
            self._fn["samples"] = 0

    def function_space(self, *, rhat=False, ess=False, mcse=False, by_chain=False,
                       thresholds=None, rhat_thresholds=None):
        """Have the chains converged where it matters, in their predictions?
        R-hat across the K chains and the batch-means effective sample size
        within them of softmax(f(x_b; theta_t))[c] on the probe batch, per
        (example, class), over every sample collected since the sampler was
        built (or `function_space_reset`), from accumulators a fused sweep
        folds the probe probabilities into at every collect step
        (kernels.fn_fold, include/bdl_fn.h).  Chains that sit in permutation-
        or sign-equivalent modes disagree in every parameter and agree here.

        Returns {"rhat": `diagnostics()`'s summary fields (count = samples,
        argmax_at = (example, class) of argmax), "ess": `ess()`'s summary
        fields (argmin_at likewise), samples, batches, batch, probe, classes}.
        rhat / ess / mcse=True add the [P, C] tensors of those names to the
        part they belong to.  R-hat needs K >= 2 and 2 folded samples, ESS 2
        closed batches; with K = 1 only the "ess" part is returned.
        by_chain=True: "ess" is a list of K results, chain k's from its own
        accumulators alone — the only form under per_chain hyperparameters,
        whose chains target different posteriors, where R-hat is refused.  The
        accumulators are no part of state_dict / checkpoints and restart empty
        after load_ckpt.  This process's chains only."""
        from . import chains
        if self._fn_probe is None:
            raise ValueError("function_space: this sampler was built without fn_probe")
        if chains.world() > 1:
            raise ValueError("function_space: the report describes this process's chains only, "
                             f"and {chains.world()} processes run chains (run it in one process)")
        if self.per_chain is not None:
            if rhat:
                raise ValueError("function_space: this sampler runs per_chain hyperparameters; "
                                 "R-hat compares chains that target ONE posterior, and these "
                                 "chains target different ones")
            if not by_chain:
                raise ValueError("function_space: this sampler runs per_chain hyperparameters; "
                                 "the pooled report pools chains that target ONE posterior, and "
                                 "these chains target different ones (ask for by_chain=True)")
        if rhat and self.K < 2:
            raise ValueError("function_space: R-hat compares chains; this sampler runs K = 1")
        thr = ESS.thresholds(thresholds)
        rthr = (1.01, 1.05, 1.1) if rhat_thresholds is None else tuple(
            float(t) for t in rhat_thresholds)
        if len(rthr) != 3:
            raise ValueError(f"function_space: three R-hat thresholds (got {rthr!r})")
        f = self._fn
        try:
            S_, nb = ESS.check_report(0 if f is None else f["samples"], self.fn_batch)
        except ValueError as e:
            raise ValueError(f"function_space: {e}") from None
        v, cg, P, Cn = f["acc"], f["chain_groups"], f["probe"], f["classes"]
        n, slot = P * Cn, 4 * cg
        at = lambda i: (i // Cn, i % Cn) if i >= 0 else None  # noqa: E731
        out = {"samples": S_, "batches": nb, "batch": self.fn_batch, "probe": P, "classes": Cn}
        rres = None
        if self.K >= 2 and self.per_chain is None:
            # Welford moments of the true count, as `_moment_spec` hands them over
            rres = K.chain_diag(v["smean"], v["sM2"], chains=self.K, chain_groups=cg, n=n,
                                var_mode=L.VAR_WELFORD, ratio=float(S_ - 1), count=S_,
                                thresholds=rthr, want=("rhat",) if rhat else ())
        want = (("ess",) if ess else ()) + (("mcse",) if mcse else ())
        launched = [K.chain_ess(v["sM2"][sl:], v["bM2"][sl:], chains=k, chain_groups=cg, n=n,
                                samples=S_, batches=nb, thresholds=thr, want=want)
                    for sl, k in ([(j * slot, 1) for j in range(self.K)] if by_chain
                                  else [(0, self.K)])]
        if rres is not None:
            r = dict(rres.summary)
            r["count"], r["argmax_at"] = S_, at(r["argmax"])
            if rhat:
                r["rhat"] = rres["rhat"].view(P, Cn)
            out["rhat"] = r
        parts = []
        for res in launched:
            e = ESS.summary_dict(res.summary, thr, samples=S_, batches=nb, batch=self.fn_batch,
                                 chains=self.K if not by_chain else 1)
            e["argmin_at"] = at(e["argmin"])
            e.update({w: res[w].view(P, Cn) for w in want})
            parts.append(e)
        out["ess"] = parts if by_chain else parts[0]
        return out

    def _report_function_space(self, ep, rec, log):
        """One log line and rec["function_space"] from `function_space()`
        (run.py --fn_probe); an evaluation that comes before the counts suffice
        says so and goes on."""
        by_chain = self.per_chain is not None
        try:
            d = self.function_space(by_chain=by_chain)
        except ValueError as e:
            log(f"(Epoch {ep}) {e}")
            return
        rec["function_space"] = d
        es = d["ess"] if by_chain else [d["ess"]]
        msg = (f"(Epoch {ep}) function space over {self.K} chains, {d['probe']} probe examples x "
               f"{d['classes']} classes ({d['samples']} samples each, {d['batches']} batches of "
               f"{d['batch']})")
        if "rhat" in d:
            r = d["rhat"]
            msg += (f": R-hat max = {r['rhat_max']:.4f} at {r['argmax_at']}, mean = "
                    f"{r['rhat_mean']:.4f}, > {r['thresholds'][0]:g}: "
                    f"{100 * r['share_above'][0]:.1f} %")
        msg += ("; ESS min = " + ", ".join(f"{e['ess_min']:.1f} at {e['argmin_at']}" for e in es)
                + ", mean = " + ", ".join(f"{e['ess_mean']:.1f}" for e in es)
                + f", < {es[0]['thresholds'][0]:g}: "
                + ", ".join(f"{100 * e['share_below'][0]:.1f} %" for e in es)
                + f"; {sum(e['n_degenerate'] for e in es)} degenerate, "
                + f"{sum(e['n_nonfinite'] for e in es)} non-finite")
        log(msg)

    def _by_tensor(self):
        """How many tensors the reports list (run.py --by_tensor N; 0: none)."""
        return int(getattr(self.args, "by_tensor", 0) or 0)

    def _log_tensors(self, ep, log, what, r, ext, mean, share, sign, fmt, worst):
        """One log line per tensor for the --by_tensor N worst tensors of a
        report `r` that carries `by_tensor`: those with the largest rhat_max /
        smallest ess_min among the tensors with something evaluated."""
        n = self._by_tensor()
        rows = [t for t in r.get("by_tensor", ()) if t["n_eval"] > 0]
        rows.sort(key=lambda t: t[ext], reverse=worst is max)
        for t in rows[:n]:
            log(f"(Epoch {ep}) {what}, tensor {t['name']} ({t['numel']} elements): "
                f"{worst.__name__} = {t[ext]:{fmt}}, mean = {t[mean]:{fmt}}, "
                f"{sign} {r['thresholds'][0]:g}: {100 * t[share][0]:.1f} %")

    # --------------------------------------------------------------- health
    def _health_lr(self, lrs, collect=None, rows=None):
        """The sweep's lr source for a step with `update`'s arguments: ((body,
        head) host floats, None, False) for uniform chains, (None, the [K, 12]
        device rows of this step, whether they were formed and uploaded here
        because the caller passed none) under per_chain.  The SGLD family's
        form; cSGHMC has its own."""
        if self.per_chain is None:
            return (float(lrs[0]), float(lrs[1])), None, False
        if rows is not None:
            return None, rows, False
        l0, l1 = (np.broadcast_to(np.asarray(v, dtype=np.float64), (self.K,)) for v in lrs)
        return None, self._upload_rows(self.chain_rows(l0, l1)), True

    def _health_sweep(self, grads, a, kw):
        """One kernels.chain_stats launch over the raw gradients of this step
        (before any clip), theta and the momentum as they stand before the
        update, accumulated on the device; no host sync.  Returns update's
        keywords (with the per_chain rows formed here, so that update does not
        upload them again)."""
        st = self.state
        st.use_grads(grads)
        seg, nseg, idx = st.stat_segments()
        lr, rows, formed = self._health_lr(*a, **kw)
        if formed:
            kw = dict(kw, rows=rows)
        h = self._health
        if h is None:
            h = self._health = [torch.zeros(self.K, nseg, len(L.STATS_SUMS), dtype=torch.float64,
                                            device=st.device),
                                K.chain_stats_workspace(self.K, nseg, st.device), 0, idx,
                                K.stats_blocks_per_chain(st.n1, self.K, st.device)]
        elif h[3] != idx:
            raise ValueError("health: the set of tensors that have a gradient changed between "
                             "accumulated steps (call health() before changing it)")
        K.chain_stats(seg, nseg, self.K, st.chain_groups, st.theta, h[0], mom=st.mom,
                      prior_mean=st.prior, lr=lr, lr_table=rows, lr_row_stride=PC.COLUMNS,
                      accumulate=True, workspace=h[1], blocks_per_chain=h[4])
        h[2] += 1
        return kw

    def _health_temperatures(self, acc, steps, numel):
        """The temperature entries of `health()`; none here (see its docstring)."""
        return {}

    def health(self, reset=True):
        """Per-chain, per-tensor health over the steps the statistics sweep
        ran at (health_every=m: the steps with step_count % m == 0; the sweep
        sits between gradients() and update(), so gradient, theta and momentum
        are taken at the same theta, the gradient before any clip).  One host
        read.  Returns `steps` (sweeps accumulated), `names` and `numel` of the
        T tensors that have a gradient, `sums` (the raw [K, T, 6] accumulator:
        G2, V2, D2, DG, VG, V2L of include/bdl_stats.h) and [K, T] float64 arrays:
        grad_rms = sqrt(G2 / (steps * numel)), mom_rms, dist_rms (the distance
        from the prior mean; from 0 where the sampler has none) and
        grad_mom_cos = VG / sqrt(G2 * V2), the cosine between gradient and
        momentum (bayesdll_amd.health).

        StackedCSGHMC adds t_kin and t_conf [K, T], the kinetic and
        configurational temperature of every (chain, tensor) in units of the
        temperature the sampler's own noise scale nd * sqrt(2 alpha lr) / N
        stands for if injected every step, and their per-chain aggregates
        t_kin_chain / t_conf_chain [K]; under per_chain chain k's values use
        chain k's momentum_decay, nd, Ninflate and prior_sig.  Both are 1 for
        a stationary chain on a quadratic in the small-step limit and rise
        with the step size and with gradient noise.  The reference adds noise
        only on the thinned sample steps, so values well below 1 are expected
        with thin > 1 and during exploration; the numbers compare chains and
        layers, they are not a pass / fail.  The other samplers return the rms
        table only: their `mom` is not a physical momentum (SGD's buffer, the
        Adam samplers' preconditioned v), and StackedSGHMC's friction momentum
        lives in lr-scaled gradient units whose temperature is not defined
        here.

        reset: empty the accumulators afterwards.  They are not part of
        state_dict / checkpoints and restart empty after load_ckpt."""
        from . import health as H
        if not self.health_every:
            raise ValueError("health: this sampler was built with health_every=0")
        st, h = self.state, self._health
        if h is None:
            idx = tuple(i for i, rg in enumerate(st.requires_grad) if rg)
            acc, steps = np.zeros((self.K, len(idx), len(L.STATS_SUMS))), 0
        else:
            acc, steps, idx = h[0].cpu().numpy(), h[2], h[3]
            if reset:
                h[0].zero_()
                h[2] = 0
        numel = [st.numels[i] for i in idx]
        out = {"steps": int(steps), "names": [st.names[i] for i in idx], "numel": numel,
               "sums": acc}
        out.update(H.rms_table(acc, steps, numel))
        out.update(self._health_temperatures(acc, steps, numel))
        return out

    def _report_health(self, ep, rec, log):
        """One log line per chain and rec["health"] from `health()` (run.py
        --health): the chain's aggregate temperatures and its hottest tensor
        (cSGHMC), else its largest gradient rms."""
        d = self.health()
        keep = ("grad_rms", "mom_rms", "dist_rms", "grad_mom_cos", "t_kin", "t_conf",
                "t_kin_chain", "t_conf_chain")
        rec["health"] = {"steps": d["steps"], "names": d["names"],
                         **{k: d[k].tolist() for k in keep if k in d}}
        if d["steps"] == 0:
            log(f"(Epoch {ep}) health: no step accumulated")
            return
        for k in range(self.K):
            who = f"(Epoch {ep}) chain {self.chain0 + k}"
            if self.per_chain is not None:
                who += f": {PC.describe(self.per_chain, self.swept, k)}"
            if "t_kin" in d:
                hot = np.where(np.isfinite(d["t_kin"][k]), d["t_kin"][k], -np.inf)
                t = int(np.argmax(hot))
                log(f"{who}: t_kin_chain = {d['t_kin_chain'][k]:.4g}, t_conf_chain = "
                    f"{d['t_conf_chain'][k]:.4g} over {d['steps']} steps; hottest tensor "
                    f"{d['names'][t]} (t_kin = {d['t_kin'][k, t]:.4g})")
            else:
                t = int(np.argmax(np.nan_to_num(d["grad_rms"][k], nan=-np.inf)))
                log(f"{who}: largest gradient rms {d['grad_rms'][k, t]:.4g} in {d['names'][t]} "
                    f"over {d['steps']} steps")

    def _clip_chains(self):
        """clip_grad_norm_(self.clip_grad) of every chain by the norm of its
        own sampler gradient — K stacked chains stand for K Runners, each
        clipping its own (methods/csgld.py:250-253, adam_csghmc.py:319-322) —
        in place in the gradients `use_grads` bound (kernels.chain_clip: three
        launches, no sync).  Keeps the (norm, coef) table in `last_clip`."""
        st = self.state
        seg, nseg = st.grad_segments()
        if self._clip_ws is None:
            self._clip_ws = K.chain_clip_workspace(self.K, st.device)
            self._clip_bpc = K.clip_blocks_per_chain(st.n1, self.K, st.device)
        self.last_clip = K.chain_clip(seg, nseg, self.K, self.clip_grad, workspace=self._clip_ws,
                                      blocks_per_chain=self._clip_bpc)

    def _upload_rows(self, rows):
        """Host fp32 rows ([K, 12] or [batches, K, 12]) to the device in one
        asynchronous copy from pinned memory; a row block is 48 * K bytes, so
        every block of the device array is 16-byte aligned."""
        host = torch.from_numpy(np.array(rows, dtype=np.float32, order="C")).pin_memory()
        return host.to(self.state.device, non_blocking=True)

    def _accumulate(self, acc, loss, out, y):
        """Per-chain running (loss sum, error count, examples) on the device."""
        bs = y.shape[-1]
        acc[0] += loss.double() * bs
        acc[1] += out.argmax(-1).ne(y).sum(-1)
        acc[2] += bs

    def _new_acc(self):
        dev = self.args.device
        return [torch.zeros(self.K, dtype=torch.float64, device=dev),
                torch.zeros(self.K, dtype=torch.int64, device=dev), 0]

    @staticmethod
    def _epoch_result(acc):
        nb = max(acc[2], 1)
        return (acc[0] / nb).cpu().numpy(), (acc[1].double() / nb).cpu().numpy()

    # ----------------------------------------------------------- predictive
    def chain_logits(self, x):
        """[K, B, C] logits of every chain at its current theta."""
        with torch.no_grad():
            return self._fwd(self.state.params, x)

    def predictive_logprob(self, x):
        """log of the predictive probability averaged uniformly over the K
        chains x the collected posterior components (`_components`: posterior
        draws or means); the chains' current theta while none is collected.
        With one process per GPU (torch.distributed initialised) the
        processes' stacked predictives are averaged too
        (chains.average_predictive: one all-reduce).  With per_chain the chains
        are different models, so this uniform mixture mixes different models
        (an ensemble over the sweep); `evaluate_chains` scores each alone."""
        from . import chains
        lp = self._local_logprob(x)
        return chains.average_predictive(lp) if chains.world() > 1 else lp

    def _component_logprobs(self, x):
        """[K, B, C] log-probabilities of every chain under each collected
        component (`_components`: its draws, its keys), or under the chains'
        current theta while nothing is collected."""
        st = self.state
        with torch.no_grad():
            buf = torch.empty_like(st.theta)
            views = {nm: buf.view(self.K, st.stride)[:, o:o + k].view(self.K, *s)
                     for nm, o, k, s in zip(st.names, st.offsets, st.numels, st.shapes)}
            comps = [F.log_softmax(self._fwd(views, x), dim=-1) for _ in self._components(buf)]
            if not comps:
                comps = [F.log_softmax(self.chain_logits(x), dim=-1)]
            return comps

    def _local_logprob(self, x):
        with torch.no_grad():
            lp = torch.cat(self._component_logprobs(x), 0)  # [K * components, B, C]
            return lp.logsumexp(0) - math.log(lp.shape[0])

    def chain_logprob(self, x):
        """[K, B, C]: every chain's OWN predictive, log of its probability
        averaged uniformly over that chain's components."""
        with torch.no_grad():
            lp = torch.stack(self._component_logprobs(x), 0).double()  # [components, K, B, C]
            return lp.logsumexp(0) - math.log(lp.shape[0])

    def evaluate_chains(self, loader, weights=None, combine="arithmetic"):
        """(nll [K], err [K]) over a data loader, chain by chain: each chain is
        scored from its own collected components (the draws and keys
        `_components` uses) or from its current theta while nothing is
        collected.  What ranks a per_chain sweep; applies to any stacked
        sampler.  One host read at the end.  weights="gmm" (cyclical samplers):
        every chain's cycles weighted by `component_weights(by_chain=True)`,
        combined as `combine` says (kernels.mixture) — K Runners."""
        if weights is not None:
            return self._weighted_scores("evaluate_chains", loader, weights, combine, True)
        dev = self.args.device
        nll = torch.zeros(self.K, dtype=torch.float64, device=dev)
        err = torch.zeros(self.K, dtype=torch.int64, device=dev)
        nb = 0
        was = self.net.training
        self.net.eval()
        try:
            for x, y in loader:
                x, y = x.to(dev), y.to(dev)
                lp = self.chain_logprob(x)
                nll -= lp.gather(-1, y.view(1, -1, 1).expand(self.K, -1, 1)).squeeze(-1) \
                    .double().sum(-1)
                err += lp.argmax(-1).ne(y).sum(-1)
                nb += len(y)
        finally:
            self.net.train(was)
        return (nll / nb).cpu().numpy(), (err.double() / nb).cpu().numpy()

    def _sample(self, out, mean, m2, var_mode, ratio):
        """One posterior draw of every chain into `out` ([K*stride]); chain k
        keyed chain0 + k (= the one-chain PosteriorDraw of that chain id)."""
        K.posterior_sample(out, mean, m2, var_mode=var_mode, ratio=ratio, seed=self.seed,
                           chain=self.chain0, step=EVAL_STEP_BASE + self.draws,
                           chain_groups=self.state.chain_groups)
        self.draws += 1

    # ---------------------------------------------------------- diagnostics
    def _component_keys(self):
        """The collected posterior components' keys, in draw order."""
        raise NotImplementedError

    def _components(self, buf):
        """Every collected component in turn: nst posterior draws into `buf`
        from its `_moment_spec` (the method's variance form and ratio), or,
        with nst = 0, its mean; yields the component's key per draw."""
        for c in self._component_keys():
            m1, m2, var_mode, ratio, _ = self._moment_spec(c)
            for _ in range(max(1, self.nst)):
                if self.nst == 0:
                    buf.copy_(m1)
                else:
                    self._sample(buf, m1, m2, var_mode, ratio)
                yield c

    def _latest_component(self):
        """The component collected last (None while nothing is collected)."""
        keys = self._component_keys()
        return keys[-1] if keys else None

    def _moment_spec(self, component):
        """(m1, m2, var_mode, ratio, count) of a collected component: the K
        chains' stacked moments, the very (var_mode, ratio) `_components`
        draws from them with, and the number of collects into them (m1 None:
        not collected; m2 None: the second moment is not kept / not used)."""
        raise NotImplementedError

    def _tensor_rows(self, table, ext, arg, hits, mean, share):
        """A per-tensor device table (kernels.chain_*_layers) as a list of
        dicts in parameter order; ext / arg / hits name the struct's fields,
        mean / share the derived keys (ext's own name prefixes sum and mean)."""
        st, rows = self.state, []
        for nm, numel, r in zip(st.names, st.numels, table):
            ne, hit = int(r["n_eval"]), [int(v) for v in r[hits]]
            rows.append({"name": nm, "numel": int(numel), "n_eval": ne,
                         "n_degenerate": int(r["n_degenerate"]),
                         "n_nonfinite": int(r["n_nonfinite"]), ext: float(r[ext]),
                         arg: int(r[arg]),
                         mean: float(r[ext.split("_")[0] + "_sum"]) / ne if ne else float("nan"),
                         hits: hit, share: [v / ne if ne else float("nan") for v in hit]})
        return rows

    def param_of(self, index):
        """Name of the parameter tensor holding flat element `index` of a chain."""
        st = self.state
        i = int(np.searchsorted(np.asarray(st.offsets), int(index), side="right")) - 1
        return st.names[max(i, 0)]

    def diagnostics(self, component=None, *, rhat=False, pooled=False, by_tensor=False):
        """Do the K chains agree?  The cross-chain Gelman-Rubin R-hat and the
        pooled Gaussian posterior of a collected component (default: the
        latest), from the chains' moments in one fused sweep
        (kernels.chain_diag).  Returns the summary (n_eval, n_degenerate,
        n_nonfinite, rhat_max, argmax and its parameter name, rhat_mean,
        n_above / share_above the thresholds 1.01 / 1.05 / 1.1, count,
        component) plus, when asked for, the [n1] tensors `rhat` and
        `pooled_mean` / `pooled_var`.  by_tensor=True: the result gains
        `by_tensor`, a list in parameter order of {name, numel, n_eval,
        n_degenerate, n_nonfinite, rhat_max, argmax (chain-local, as the
        summary's), rhat_mean, n_above, share_above} — the summary of each
        tensor alone, from one more fused sweep (kernels.chain_diag_layers)
        with no per-element output.  Reads the moments only: nothing the
        sampler owns is written."""
        if self.K < 2:
            raise ValueError("diagnostics: R-hat compares chains; this sampler runs K = 1")
        if self.per_chain is not None:
            raise ValueError("diagnostics: this sampler runs per_chain hyperparameters; R-hat "
                             "compares chains that target ONE posterior, and these chains "
                             "target different ones (rank them with evaluate_chains)")
        if component is None:
            component = self._latest_component()
        m1 = None
        if component is not None:
            m1, m2, var_mode, ratio, count = self._moment_spec(component)
        if m1 is None:
            raise ValueError("diagnostics: nothing is collected yet"
                             + ("" if component is None else f" for component {component!r}"))
        if count < 2:
            raise ValueError(f"diagnostics: component {component!r} holds {count} sample per "
                             "chain; the within-chain variance needs at least 2")
        if m2 is None:
            raise ValueError("diagnostics: the second moment is not kept (nst = 0), so there is "
                             "no within-chain variance")
        st = self.state
        want = (("rhat",) if rhat else ()) + (("pooled_mean", "pooled_var") if pooled else ())
        res = K.chain_diag(m1, m2, chains=self.K, chain_groups=st.chain_groups, n=st.n1,
                           var_mode=var_mode, ratio=ratio, count=count, want=want)
        out = dict(res.summary)
        out["component"], out["count"] = component, int(count)
        out["argmax_param"] = self.param_of(out["argmax"]) if out["argmax"] >= 0 else None
        out.update({w: res[w] for w in want})
        if by_tensor:
            tab = K.chain_diag_layers(m1, m2, st.layer_segments(), chains=self.K,
                                      chain_groups=st.chain_groups, n=st.n1, var_mode=var_mode,
                                      ratio=ratio, count=count)
            out["by_tensor"] = self._tensor_rows(tab, "rhat_max", "argmax", "n_above", "rhat_mean",
                                                 "share_above")
        return out

    def evaluate(self, loader, weights=None, combine="arithmetic"):
        """(NLL, error) of the stacked predictive over a data loader (the
        network in eval mode, as the reference's evaluate).  weights="gmm"
        (cyclical samplers): the (cycle, chain) components weighted jointly by
        `component_weights(by_chain=False)` (kernels.mixture)."""
        if weights is not None:
            nll, err = self._weighted_scores("evaluate", loader, weights, combine, False)
            return float(nll[0]), float(err[0])
        dev = self.args.device
        loss, err, nb = 0.0, 0, 0
        was = self.net.training
        self.net.eval()
        try:
            for x, y in loader:
                x, y = x.to(dev), y.to(dev)
                lp = self.predictive_logprob(x)
                loss += F.nll_loss(lp, y, reduction="sum").item()
                err += lp.argmax(-1).ne(y).sum().item()
                nb += len(y)
        finally:
            self.net.train(was)
        return loss / nb, err / nb

    def _member_logits(self, x, bufs, pooled=False):
        """[members, K, B, C] raw logits of the members `_component_logprobs`
        averages over — the same draws in the same order from the same keys,
        or the chains' current theta while nothing is collected — written into
        one buffer per batch shape (kept in `bufs`).  pooled (the weighted
        mixture over all chains): [components, K, draws, B, C], so that the
        (cycle, chain) pairs are the contiguous components of one group."""
        st = self.state
        nd = max(1, self.nst)
        n = len(self._component_keys()) * nd
        with torch.no_grad():
            if n == 0:
                return self.chain_logits(x).float().contiguous().unsqueeze(0)
            buf = torch.empty_like(st.theta)
            views = {nm: buf.view(self.K, st.stride)[:, o:o + k].view(self.K, *s)
                     for nm, o, k, s in zip(st.names, st.offsets, st.numels, st.shapes)}
            out = None
            for i, _ in enumerate(self._components(buf)):
                lg = self._fwd(views, x)
                if out is None:
                    key = (n,) + tuple(lg.shape)
                    if pooled:
                        key = (n // nd, self.K, nd) + tuple(lg.shape[1:])
                    out = bufs.get(key)
                    if out is None:
                        out = bufs[key] = torch.empty(key, dtype=torch.float32, device=lg.device)
                if pooled:
                    out[i // nd, :, i % nd].copy_(lg)
                else:
                    out[i].copy_(lg)
            return out

    # ------------------------------------- likelihood-weighted cycle mixture
    def score_cycle(self, train_loader, c=None):
        """The reference's cycle-end likelihood pass (methods/csghmc.py:568-638)
        for all K chains at once: max(1, nst) posterior draws of every chain
        from cycle c's moments (`_moment_spec`; the latest collected cycle by
        default; with nst = 0 the means), the vmapped forward in eval mode over
        the loader, kernels.member_score per batch with groups = K — the loss
        sums stay on the device until ONE host read at the end.  Stores and
        returns cycle_likelihoods[c]: float64 [draws, K] of exp(-nll_sum / n)."""
        self._need_cyclical("score_cycle")
        c = self._latest_component() if c is None else c
        m1, m2, var_mode, ratio, _ = self._moment_spec(c) if c is not None else (None,) * 5
        if m1 is None:
            raise ValueError(f"score_cycle: cycle {c} is not collected")
        st, dev, nd = self.state, self.args.device, max(1, self.nst)
        scores, out = None, {}
        was = self.net.training
        self.net.eval()
        try:
            with torch.no_grad():
                views = []
                for _ in range(nd):
                    buf = torch.empty_like(st.theta)
                    if self.nst == 0:
                        buf.copy_(m1)
                    else:
                        self._sample(buf, m1, m2, var_mode, ratio)
                    views.append({nm: buf.view(self.K, st.stride)[:, o:o + k].view(self.K, *s)
                                  for nm, o, k, s in zip(st.names, st.offsets, st.numels,
                                                         st.shapes)})
                for x, y in train_loader:
                    x, y = x.to(dev), y.to(dev).to(torch.int64).contiguous()
                    for s, v in enumerate(views):
                        lg = self._fwd(v, x)
                        key = (nd,) + tuple(lg.shape)
                        if key not in out:
                            out[key] = torch.empty(key, dtype=torch.float32, device=lg.device)
                        out[key][s].copy_(lg)
                    scores = K.member_score(out[key], y, groups=self.K, scores=scores)
        finally:
            self.net.train(was)
        if scores is None:
            raise ValueError("score_cycle: the loader is empty")
        r = scores.read()  # the one host read
        with np.errstate(divide="ignore", invalid="ignore"):
            lik = np.exp(-r["nll_sum"] / r["n"])
        self.cycle_likelihoods[c] = lik.astype(np.float64)
        return self.cycle_likelihoods[c]

    def component_weights(self, by_chain=True):
        """float64 [components, K] weights of the collected cycles
        (`cycle_weights`): per chain (K Runners) or, by_chain=False, jointly
        over all (cycle, chain).  Raises, naming the cycle, if a collected
        cycle has not been scored."""
        self._need_cyclical("component_weights")
        return cycle_weights(self.cycle_likelihoods or {}, self._component_keys(), by_chain)

    def _need_cyclical(self, what):
        if not self.cyclical:
            raise ValueError(f"{what}: {type(self).__name__} is not cyclical (it collects one "
                             "component: there are no cycles to weigh)")

    def _mixture_weights(self, what, weights, combine, by_chain):
        """Every refusal of the weights= / combine= keywords, then the device
        table kernels.mixture takes: float64 [components, K] by chain,
        [components * K, 1] pooled."""
        from . import chains
        if weights == "stacking":
            return self._stacking_weights(what, combine, by_chain)
        if weights == "cold":
            return self._stacking_weights(what, combine, by_chain, cold=True)
        if weights != "gmm":
            raise ValueError(f'{what}: weights is None (uniform) or "gmm" (got {weights!r})')
        if combine not in L.MIX_COMBINE:
            raise ValueError(f"{what}: combine from {tuple(L.MIX_COMBINE)} (got {combine!r})")
        self._need_cyclical(f'{what}: weights="gmm"')
        if chains.world() > 1:
            raise ValueError(f'{what}: weights="gmm" weighs this process\'s chains only, and '
                             f"{chains.world()} processes share the predictive")
        if not by_chain and self.per_chain is not None:
            raise ValueError(f'{what}: weights="gmm" over all chains would weigh different models '
                             "against each other (per_chain hyperparameters); use the by-chain "
                             "form")
        if not by_chain and combine == "reference":
            raise ValueError(f'{what}: combine="reference" is one Runner\'s rule (a weighted sum '
                             "of ITS cycles' log-probabilities); it is defined by chain, not over "
                             "pooled (cycle, chain) components")
        w = self.component_weights(by_chain)
        if not by_chain:
            w = w.reshape(-1, 1)
        return torch.from_numpy(np.ascontiguousarray(w)).to(self.args.device)

    # ------------------------------------------------- stacking weights
    stacking_ = None     # fit_stacking's [K] fp64 device tensor (not checkpointed)
    stacking_val = None  # run.py --stacking: the validation loader `_report_stacking` fits on

    def fit_stacking(self, loader, *, tol=1e-4, max_iter=2000):
        """Bayesian stacking of the K chains' predictive distributions (Yao et
        al. 2018) on a held-out loader, on the device: the weights w on the
        simplex that maximise the mean log score of sum_k w_k p_k(y | x) — what
        a per_chain sweep (K different models) or chains in modes of different
        quality should be pooled with.  A voter is a chain's OWN predictive
        (`evaluate`'s members, the same Philox keys and the same advance of
        `draws`): per batch kernels.predict with groups = K, then
        kernels.stack_gather keeps only every chain's log-probability of the
        true label, a [K, N] matrix; kernels.stack_fit runs the EM iteration
        there (include/bdl_stacking.h).  Stores `stacking_` (device fp64 [K];
        not part of state_dict) for evaluate / uncertainty / fit_temperature
        (..., weights="stacking") and returns weights (float64 [K]), objective
        (the mean log score at the weights), objective_uniform (at 1/K),
        objective_best_single and best_single (the best chain alone), gap
        (objective* - objective <= gap), iterations, converged, n and the
        exclusion counts n_label, n_nonfinite, n_impossible.  This process's
        chains only."""
        _single_process("fit_stacking")
        dev, Kc = self.args.device, self.K
        cap, off, bufs = 4096, 0, {}
        ell = torch.zeros(Kc, cap, dtype=torch.float32, device=dev)
        valid = torch.zeros(cap, dtype=torch.int32, device=dev)
        counters = torch.zeros(3, dtype=torch.int64, device=dev)
        was = self.net.training
        self.net.eval()
        try:
            for x, y in loader:
                x, y = x.to(dev), y.to(dev).to(torch.int64).contiguous()
                outs, _ = K.predict(self._member_logits(x, bufs), y, groups=Kc, want=("logp",))
                if off + len(y) > cap:  # grow the resident matrix
                    while off + len(y) > cap:
                        cap *= 2
                    ell2 = torch.zeros(Kc, cap, dtype=torch.float32, device=dev)
                    valid2 = torch.zeros(cap, dtype=torch.int32, device=dev)
                    ell2[:, :off].copy_(ell[:, :off])
                    valid2[:off].copy_(valid[:off])
                    ell, valid = ell2, valid2
                off = K.stack_gather(outs["logp"], y, ell, valid, counters, off)
        finally:
            self.net.train(was)
        if off == 0:
            raise ValueError("fit_stacking: the loader is empty")
        state = K.stack_fit(ell, valid, off, tol=tol, max_iter=max_iter)
        # every chain's own mean log score, read with the state and the counters
        ok = valid[:off].bool()
        single = torch.where(ok, ell[:, :off].double(), torch.zeros((), dtype=torch.float64,
                                                                    device=dev)).sum(1)
        both = torch.cat([state.buf, counters.view(torch.uint8),
                          single.view(torch.uint8)]).cpu().numpy().tobytes()  # the one host read
        n1 = state.buf.numel()
        r = np.frombuffer(both[:n1], dtype=np.dtype(L.StackState))[0]
        cnt = np.frombuffer(both[n1:n1 + 24], dtype=np.int64)
        n = int(r["n"])
        if n == 0:
            raise ValueError("fit_stacking: no example can be scored (n = 0: "
                             + ", ".join(f"{k} = {int(v)}" for k, v in zip(L.STACK_COUNTERS, cnt))
                             + ")")
        if r["degenerate"]:
            raise ValueError("fit_stacking: the fit is degenerate (a mixture probability "
                             "underflowed)")
        single = np.frombuffer(both[n1 + 24:], dtype=np.float64) / n
        best = int(np.argmax(np.where(np.isfinite(single), single, -np.inf)))
        self.stacking_ = state.weights().clone()
        res = {"weights": np.array(r["w"][:Kc], dtype=np.float64),
               "objective": float(r["objective"]),
               "objective_uniform": float(r["objective_uniform"]),
               "objective_best_single": float(single[best]), "best_single": self.chain0 + best,
               "iterations": int(r["iterations"]), "converged": bool(r["converged"]),
               "gap": float(r["gap"]), "n": n}
        res.update({k: int(v) for k, v in zip(L.STACK_COUNTERS, cnt)})
        return res

    def _stacking_weights(self, what, combine, by_chain, cold=False):
        """The refusals of weights="stacking", then kernels.mixture's pooled
        table: float64 [components * K, 1] with w_{c,k} = w_k / components, so
        that the arithmetic mixture is exactly sum_k w_k p_k.  cold
        (weights="cold"): the same refusals and the same table with w = 1 on
        the cold slot (`cold_slots`; shared equally if several) and 0 elsewhere."""
        from . import chains
        kind = "cold" if cold else "stacking"
        if combine not in L.MIX_COMBINE:
            raise ValueError(f"{what}: combine from {tuple(L.MIX_COMBINE)} (got {combine!r})")
        if chains.world() > 1:
            raise ValueError(f'{what}: weights="{kind}" weighs this process\'s chains only, and '
                             f"{chains.world()} processes share the predictive")
        if by_chain:
            raise ValueError(f'{what}: weights="{kind}" weighs the chains against each other: '
                             "it is the pooled form only (there is nothing to weigh within one "
                             "chain)")
        if combine == "reference":
            raise ValueError(f'{what}: combine="reference" is one Runner\'s rule (a weighted sum '
                             "of ITS cycles' log-probabilities); "
                             + ("the cold slot's weight is a weight of the arithmetic mixture"
                                if cold else "stacking weights maximise the log score of the "
                                "arithmetic mixture"))
        if cold:
            if self.per_chain is None:
                raise ValueError(f'{what}: weights="cold" needs a per_chain table (the cold slot '
                                 "is the one with the smallest nd)")
            slots = self.cold_slots()
            w = torch.zeros(self.K, dtype=torch.float64)
            w[slots] = 1.0 / len(slots)
            w = w.to(self.args.device)
        else:
            if self.stacking_ is None:
                raise ValueError(f'{what}: weights="stacking" needs a fit_stacking() first')
            w = self.stacking_
        comps = max(1, len(self._component_keys()))
        w = (w / comps).repeat(comps)  # [components, K] row-major
        return w.reshape(-1, 1).contiguous()

    def _report_stacking(self, ep, rec, val_loader, test_loader, log):
        """run.py --stacking: fit on the validation split, log the weights
        line, and with a test loader the stacked predictive under them
        (rec["stacking"], rec["test_stacking"])."""
        try:
            d = self.fit_stacking(val_loader)
            rec["stacking"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v)
                               for k, v in d.items()}
            log(f"(Epoch {ep}) stacking weights: "
                f"{ {self.chain0 + k: float(w) for k, w in enumerate(d['weights'])} } "
                f"(gap = {d['gap']:.2e}, iterations = {d['iterations']}, converged = "
                f"{d['converged']})")
            if test_loader is None:
                return
            rec["test_stacking"] = self.evaluate(test_loader, weights="stacking")
            log(f"(Epoch {ep}) stacked predictive, stacking weights: loss = "
                f"{rec['test_stacking'][0]:.4f}, error = {rec['test_stacking'][1]:.4f}")
        except ValueError as e:
            log(f"(Epoch {ep}) stacking weights: {e}")

    def _weighted_batches(self, what, loader, weights, combine, by_chain, want=("logp",)):
        """Per batch of the loader (eval mode): (mixture outputs, labels,
        MixtureTotals) of the weighted predictive — `evaluate`'s members, the
        same Philox keys and the same advance of `draws`."""
        wdev = self._mixture_weights(what, weights, combine, by_chain)
        dev, nd, bufs, tot = self.args.device, max(1, self.nst), {}, None
        if not self._component_keys():  # nothing collected: the chains' current theta, one draw
            nd = 1
        was = self.net.training
        self.net.eval()
        try:
            for x, y in loader:
                x, y = x.to(dev), y.to(dev).to(torch.int64).contiguous()
                lg = self._member_logits(x, bufs, pooled=not by_chain)
                outs, tot = K.mixture(lg, wdev, y, draws=nd, groups=self.K if by_chain else 1,
                                      combine=combine, want=want, totals=tot)
                yield outs, y, tot
        finally:
            self.net.train(was)

    def _weighted_scores(self, what, loader, weights, combine, by_chain):
        """(nll [G], err [G]) of the weighted logp over the loader; one host
        read at the end."""
        G, dev = self.K if by_chain else 1, self.args.device
        nll = torch.zeros(G, dtype=torch.float64, device=dev)
        err = torch.zeros(G, dtype=torch.int64, device=dev)
        nb = 0
        for outs, y, _ in self._weighted_batches(what, loader, weights, combine, by_chain):
            lp = outs["logp"]
            nll -= lp.gather(-1, y.view(1, -1, 1).expand(G, -1, 1)).squeeze(-1).double().sum(-1)
            err += lp.argmax(-1).ne(y).sum(-1)
            nb += len(y)
        if nb == 0:
            raise ValueError(f"{what}: the loader is empty")
        both = torch.stack([nll, err.double()]).cpu().numpy() / nb
        return both[0], both[1]

    def _gmm_state(self):
        """cycle_likelihoods for `_extra_state`, only when the option is on."""
        if not self.gmm_weights:
            return {}
        return {"cycle_likelihoods": {int(c): torch.from_numpy(np.array(v, dtype=np.float64))
                                      for c, v in self.cycle_likelihoods.items()}}

    def _load_gmm_state(self, d):
        """... and back; a checkpoint without it loads with nothing scored."""
        self.cycle_likelihoods = {int(c): v.cpu().numpy().astype(np.float64)
                                  for c, v in (d.get("cycle_likelihoods") or {}).items()}

    def _report_gmm(self, ep, rec, train_loader, test_loader, log):
        """run.py --gmm_weights: score the finished cycle, log every chain's
        `GMM component weights: {...}` line (the reference's), and with a test
        loader the weighted NLL and error under rec["test_gmm"] (per chain
        under per_chain: rec["chains_gmm"])."""
        try:
            c = self._latest_component()
            self.score_cycle(train_loader, c)
            w = self.component_weights(by_chain=True)
            keys = self._component_keys()
            rec["gmm_weights"] = {"cycles": [int(k) for k in keys], "weights": w.tolist()}
            for k in range(self.K):
                log(f"(Epoch {ep}) chain {self.chain0 + k}: GMM component weights: "
                    f"{ {int(c): float(w[i, k]) for i, c in enumerate(keys)} }")
            if test_loader is None:
                return
            if self.per_chain is None:
                rec["test_gmm"] = self.evaluate(test_loader, weights="gmm")
                log(f"(Epoch {ep}) stacked predictive, GMM weights: loss = "
                    f"{rec['test_gmm'][0]:.4f}, error = {rec['test_gmm'][1]:.4f}")
            else:
                nll, err = self.evaluate_chains(test_loader, weights="gmm")
                rec["chains_gmm"] = {"nll": nll.tolist(), "error": err.tolist()}
                for k in range(self.K):
                    log(f"(Epoch {ep}) chain {self.chain0 + k}, GMM weights: loss = {nll[k]:.4f}, "
                        f"error = {err[k]:.4f}")
        except ValueError as e:
            log(f"(Epoch {ep}) GMM weights: {e}")

    temperature_ = None   # fit_temperature's [G] device tensor (not checkpointed)
    _temper = None        # (by_chain, kernels.TemperState) of the last fit

    def _loader_logp(self, loader, G, weights=None, combine="arithmetic", by_chain=False):
        """(logp [G, N, C], labels [N]) of `evaluate`'s members over the loader,
        both on the device: predict's log mixture per batch, concatenated (the
        weighted mixture's with weights="gmm")."""
        dev = self.args.device
        lps, ys, bufs = [], [], {}
        if weights is not None:
            for outs, y, _ in self._weighted_batches("fit_temperature", loader, weights, combine,
                                                     by_chain):
                lps.append(outs["logp"])
                ys.append(y)
            if not lps:
                return None, None
            return torch.cat(lps, 1).contiguous(), torch.cat(ys).contiguous()
        was = self.net.training
        self.net.eval()
        try:
            for x, y in loader:
                x, y = x.to(dev), y.to(dev).to(torch.int64).contiguous()
                outs, _ = K.predict(self._member_logits(x, bufs), y, groups=G, want=("logp",))
                lps.append(outs["logp"])
                ys.append(y)
        finally:
            self.net.train(was)
        if not lps:
            return None, None
        return torch.cat(lps, 1).contiguous(), torch.cat(ys).contiguous()

    def fit_temperature(self, loader, *, by_chain=False, rtol=1e-6, max_iter=32, weights=None,
                        combine="arithmetic"):
        """Fit one scalar temperature (per chain with by_chain=True) to the
        stacked predictive on a held-out loader, on the device: T minimises the
        NLL of softmax(logp / T), logp the sample-averaged log-probabilities of
        `evaluate`'s members (the same Philox keys and the same advance of
        `draws` as `uncertainty`) — the reference's temperature scaling.  logp
        [G, N, C] and the labels stay on the device, the Newton iteration
        (kernels.temper_fit) runs there, and its state is read once.  Stores
        `temperature_` ([G] device tensor) for `uncertainty(...,
        temperature="fitted")` and returns the fit's summary (temperature,
        nll_before, nll_after, iterations, converged, at_bound, degenerate, n,
        n_nonfinite, n_inf_label; lists of K under by_chain).  Not part of
        state_dict.  This process's chains only.  weights="gmm" (cyclical
        samplers) fits on the likelihood-weighted mixture's logp instead
        (`combine` as kernels.mixture takes it)."""
        _single_process("fit_temperature")
        G = self.K if by_chain else 1
        logp, y = self._loader_logp(loader, G, weights, combine, by_chain)
        if logp is None:
            raise ValueError("fit_temperature: the loader is empty")
        state = K.temper_fit(logp, y, groups=G, rtol=rtol, max_iter=max_iter)
        rows = state.summary()  # the one host read
        self._temper = (bool(by_chain), state)
        self.temperature_ = state.temperatures()
        return {k: [r[k] for r in rows] for k in rows[0]} if by_chain else rows[0]

    def _temperature_state(self, temperature, by_chain, G):
        """The kernels.TemperState `uncertainty` reports at."""
        if isinstance(temperature, str):
            if temperature != "fitted":
                raise ValueError('uncertainty: temperature is a float, a sequence or "fitted"')
            if self._temper is None:
                raise ValueError('uncertainty: temperature="fitted" needs a fit_temperature() '
                                 "first")
            if self._temper[0] != bool(by_chain):
                raise ValueError(f"uncertainty: the temperature was fitted with by_chain="
                                 f"{self._temper[0]}, not by_chain={bool(by_chain)} (fit it again)")
            return self._temper[1]
        return K.TemperState(K.temper_betas(temperature, G), self.args.device)

    def uncertainty(self, loader, *, by_chain=False, num_bins=None, per_example=False,
                    temperature=None, weights=None, combine="arithmetic"):
        """What the ensemble is for, over a data loader (the network in eval
        mode, as `evaluate`): NLL, error, ECE / MCE over `num_bins` confidence
        bins of every (example, class) probability (default args.ece_num_bins,
        else 15), the predictive's total entropy, the members' expected entropy,
        their difference (the mutual information: how much of the uncertainty
        is the members disagreeing), that on the wrongly against the other
        examples, and the mean share of members off the vote — from one fused
        sweep per batch over the members' logits (kernels.predict), the totals
        staying on the device until one host read at the end.  The members are
        `evaluate`'s: chains x collected components x nst draws (the same
        Philox keys; `draws` advances as an `evaluate` over the loader would
        advance it), uniformly weighted.  by_chain=True: every chain's own
        mixture (the form for per_chain sweeps, cf. `evaluate_chains`), every
        value a list of K.  per_example=True adds `per_example`: the [G, N]
        tensors entropy, expected_entropy, mutual_info, confidence, nll, pred
        and disagree, concatenated over the loader.  temperature: None (nothing
        else happens), a float, a length-G sequence or "fitted"
        (`fit_temperature`'s, of the same by_chain): adds `scaled` = {temperature,
        nll, ece, mce, entropy, confidence} of softmax(logp / T), from
        kernels.temper_report on every batch's log mixture — its totals are
        read in the same single host read.  This process's chains only.
        weights="gmm" (cyclical samplers): the likelihood-weighted cycle
        mixture instead (kernels.mixture, `combine` as it takes it) — nll,
        error, ece, mce, entropy and confidence from kernels.temper_report at
        T = 1 on the weighted logp, expected_entropy and mutual_info = entropy
        - expected_entropy from the mixture's totals, one host read;
        disagreement is not defined under weights and is omitted, and
        per_example / temperature are not offered there."""
        _single_process("uncertainty")
        nb = int(num_bins if num_bins is not None else getattr(self.args, "ece_num_bins", None) or 15)
        if weights is not None:
            return self._weighted_uncertainty(loader, by_chain, nb, per_example, temperature,
                                              weights, combine)
        dev = self.args.device
        G = self.K if by_chain else 1
        want = K.PREDICT_DEFAULT_WANT if per_example else ()
        tstate = None if temperature is None else self._temperature_state(temperature, by_chain, G)
        tot, ttot, pieces, bufs = None, None, [], {}
        was = self.net.training
        self.net.eval()
        try:
            for x, y in loader:
                x, y = x.to(dev), y.to(dev).to(torch.int64).contiguous()
                lg = self._member_logits(x, bufs)
                outs, tot = K.predict(lg, y, groups=G, totals=tot, num_bins=nb,
                                      want=want if tstate is None else want + ("logp",))
                if tstate is not None:
                    ttot = K.temper_report(outs.pop("logp"), y, tstate, groups=G, totals=ttot,
                                           num_bins=nb)
                pieces.append(outs)
        finally:
            self.net.train(was)
        if tot is None:
            raise ValueError("uncertainty: the loader is empty")
        if tstate is None:
            rows = tot.summary()  # the one host read
        else:  # ... of both: one buffer, one copy
            both = torch.cat([tot.buf, ttot.buf, tstate.buf]).cpu().numpy().tobytes()
            n1, n2 = tot.buf.numel(), ttot.buf.numel()
            rows = [K.predict_summary(r, tot.members, nb)
                    for r in np.frombuffer(both[:n1], dtype=np.dtype(L.PredictTotals))]
            trows = [K.temper_summary(r, nb)
                     for r in np.frombuffer(both[n1:n1 + n2], dtype=np.dtype(L.TemperTotals))]
            betas = np.frombuffer(both[n1 + n2:], dtype=np.dtype(L.TemperState))["beta"]
            for r, beta in zip(trows, betas):
                r["temperature"] = 1.0 / float(beta)
        res = {k: [r[k] for r in rows] for k in rows[0]} if by_chain else rows[0]
        res["members"], res["num_bins"] = tot.members, nb
        if tstate is not None:
            keys = ("temperature", "nll", "ece", "mce", "entropy", "confidence")
            res["scaled"] = ({k: [r[k] for r in trows] for k in keys} if by_chain
                             else {k: trows[0][k] for k in keys})
        if per_example:
            res["per_example"] = {w: torch.cat([p[w] for p in pieces], 1) for w in want}
        return res

    def _weighted_uncertainty(self, loader, by_chain, nb, per_example, temperature, weights,
                              combine):
        if per_example or temperature is not None:
            raise ValueError('uncertainty: weights="gmm" reports the totals at T = 1 only '
                             "(no per_example, no temperature)")
        G, tstate, ttot, mtot = self.K if by_chain else 1, None, None, None
        for outs, y, mtot in self._weighted_batches("uncertainty", loader, weights, combine,
                                                    by_chain, want=("logp", "expected_entropy")):
            if tstate is None:
                tstate = K.TemperState(K.temper_betas(1.0, G), self.args.device)
            ttot = K.temper_report(outs["logp"], y, tstate, groups=G, totals=ttot, num_bins=nb)
        if ttot is None:
            raise ValueError("uncertainty: the loader is empty")
        both = torch.cat([ttot.buf, mtot.buf]).cpu().numpy().tobytes()  # the one host read
        n1 = ttot.buf.numel()
        rows = []
        for t, m in zip(np.frombuffer(both[:n1], dtype=np.dtype(L.TemperTotals)),
                        np.frombuffer(both[n1:], dtype=np.dtype(L.MixtureTotals))):
            r = K.temper_summary(t, nb)
            r["expected_entropy"] = K.mixture_summary(m)["expected_entropy"]
            r["mutual_info"] = r["entropy"] - r["expected_entropy"]
            rows.append(r)
        res = {k: [r[k] for r in rows] for k in rows[0]} if by_chain else rows[0]
        comps = len(self._component_keys())
        res["members"] = comps * max(1, self.nst) * (1 if by_chain else self.K)
        if not comps:  # weights="stacking" with nothing collected: the K current thetas
            res["members"] = self.K
        res["num_bins"], res["combine"] = nb, combine
        return res

    def _report_uncertainty(self, ep, rec, loader, log):
        """One log line (one per chain under per_chain) and rec["uncertainty"]
        from `uncertainty()` (run.py --uncertainty)."""
        by_chain = self.per_chain is not None
        try:
            d = self.uncertainty(loader, by_chain=by_chain)
        except ValueError as e:
            log(f"(Epoch {ep}) uncertainty: {e}")
            return
        rec["uncertainty"] = d
        for k in range(self.K if by_chain else 1):
            r = {f: (v[k] if by_chain else v) for f, v in d.items() if f not in ("members",
                                                                                   "num_bins")}
            who = f"over {self.K} chains"
            if by_chain:
                who = f"chain {self.chain0 + k}: {PC.describe(self.per_chain, self.swept, k)}"
            log(f"(Epoch {ep}) uncertainty {who} ({d['members']} members, {r['n']} examples): "
                f"NLL = {r['nll']:.4f}, error = {r['error']:.4f}, ECE = {r['ece']:.4f}, "
                f"MCE = {r['mce']:.4f} ({d['num_bins']} bins), entropy = {r['entropy']:.4f} "
                f"(expected {r['expected_entropy']:.4f}), mutual information = "
                f"{r['mutual_info']:.4f} (wrong {r['mutual_info_wrong']:.4f}, other "
                f"{r['mutual_info_correct']:.4f}), disagreement = {r['disagreement']:.4f}; "
                f"{r['n_nonfinite']} non-finite")

    # ------------------------------------------------------------ detection
    detect_shifted = None  # run.py --detect_shift: the shifted loader `_report_detection` ranks

    def _detection_outputs(self, loader, G, labelled):
        """`uncertainty`'s sweep over a loader, keeping the per-example outputs
        the detection scores are made of on the device: ({output: [G, N]},
        labels [N] or None, classes, members).  A batch is (x, y) or, where
        labels are not needed, x alone."""
        dev = self.args.device
        want = ("entropy", "expected_entropy", "mutual_info", "confidence", "pred", "disagree")
        tot, pieces, ys, bufs, classes = None, [], [], {}, 0
        was = self.net.training
        self.net.eval()
        try:
            for batch in loader:
                x, y = batch if isinstance(batch, (tuple, list)) else (batch, None)
                x = x.to(dev)
                if labelled:
                    y = y.to(dev).to(torch.int64).contiguous()
                    ys.append(y)
                lg = self._member_logits(x, bufs)
                classes = int(lg.shape[-1])
                outs, tot = K.predict(lg, y if labelled else None, groups=G, totals=tot,
                                      want=want)
                pieces.append(outs)
        finally:
            self.net.train(was)
        if tot is None:
            raise ValueError("detection: a loader is empty")
        outs = {w: torch.cat([p[w] for p in pieces], 1) for w in want}
        return outs, (torch.cat(ys) if labelled else None), classes, tot.members

    @staticmethod
    def _detection_rows(outs, names):
        """[G * len(names), N] score rows, the scores of a group adjacent."""
        make = {"entropy": lambda o: o["entropy"], "mutual_info": lambda o: o["mutual_info"],
                "expected_entropy": lambda o: o["expected_entropy"],
                "neg_confidence": lambda o: -o["confidence"],
                "disagree": lambda o: o["disagree"].float()}
        s = torch.stack([make[nm](outs) for nm in names], 1)  # [G, S, N]
        return s.reshape(-1, s.shape[-1]).contiguous()

    def detection(self, loader, shifted=None, *, by_chain=False, scores=None):
        """How well do the ensemble's uncertainty scores RANK the examples?
        AUROC, average precision and the false-positive rate at 95 % true
        positives of every score in `scores` (default DETECTION_SCORES:
        entropy, mutual_info, expected_entropy, neg_confidence = -confidence,
        disagree as a float; higher = more suspect) for two tasks.
        `misclassification`: over `loader`, the positives are the examples the
        vote gets wrong (pred != label); unlabelled and non-finite examples
        are excluded.  `shift` (only with `shifted`, a second loader whose
        labels, if any, are not read): the scores of both loaders concatenated
        on the device, the examples of `shifted` the positives; only
        non-finite examples are excluded.  The scores are `uncertainty`'s
        per-example outputs of `evaluate`'s members, uniformly weighted
        (`draws` advances as one `uncertainty` call per loader would advance
        it; with nst > 0 the two loaders are scored by the same mixture in
        distribution, not by the same draws).  They stay on the device; one
        kernels.rank call per task counts all pairs exactly (every integer is
        independent of geometry and order), and ONE host read at the end
        fetches both tasks' totals.  Returns {task: {score: {auroc, ap, fpr95},
        n_pos, n_neg, n_excluded}, members}; by_chain=True: every chain's own
        mixture, every value a list of K.  There is no weights="gmm" and no
        temperature here: a rank statistic is invariant under a monotone map
        of the score, but not under a change of the mixture, and the weighted
        mixture has no per-example outputs.  This process's chains only."""
        _single_process("detection")
        names = tuple(DETECTION_SCORES if scores is None else scores)
        if not names or any(nm not in DETECTION_SCORES for nm in names):
            raise ValueError(f"detection: scores from {DETECTION_SCORES}")
        G, S = self.K if by_chain else 1, len(names)
        outs, y, classes, members = self._detection_outputs(loader, G, True)
        bad = outs["pred"] < 0  # non-finite: its disagree (-1) is no score
        lab = (y >= 0) & (y < classes)
        marks = torch.where(bad | ~lab.unsqueeze(0), 2, outs["pred"].ne(y.unsqueeze(0)).int())
        tasks = [("misclassification", self._detection_rows(outs, names),
                  marks.to(torch.int32).contiguous())]
        if shifted is not None:
            outs2, _, _, _ = self._detection_outputs(shifted, G, False)
            both = {w: torch.cat([outs[w], outs2[w]], 1) for w in outs}
            marks = torch.cat([torch.zeros_like(outs["pred"]), torch.ones_like(outs2["pred"])], 1)
            marks = torch.where(both["pred"] < 0, 2, marks)
            tasks.append(("shift", self._detection_rows(both, names),
                          marks.to(torch.int32).contiguous()))
        size = G * S * C.sizeof(L.RankTotals)
        buf = torch.empty(len(tasks) * size, dtype=torch.uint8, device=self.args.device)
        for i, (_, rows, marks) in enumerate(tasks):
            K.rank(rows, marks, scores_per_group=S, totals=buf[i * size:(i + 1) * size])
        host = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=np.dtype(L.RankTotals))  # the read
        res = {"members": members}
        for i, (task, _, _) in enumerate(tasks):
            rows = [K.rank_summary(r) for r in host[i * G * S:(i + 1) * G * S]]
            d = {}
            for s, nm in enumerate(names):
                per = [{"auroc": rows[g * S + s]["auroc"], "ap": rows[g * S + s]["ap"],
                        "fpr95": rows[g * S + s]["fpr"]} for g in range(G)]
                d[nm] = {k: [p[k] for p in per] for k in per[0]} if by_chain else per[0]
            for k in ("n_pos", "n_neg", "n_excluded"):  # the same for every score of a group
                v = [rows[g * S][k] for g in range(G)]
                d[k] = v if by_chain else v[0]
            res[task] = d
        return res

    def _report_detection(self, ep, rec, loader, log):
        """One log line per task (one per chain and task under per_chain) and
        rec["detection"] from `detection()` (run.py --detect, --detect_shift)."""
        by_chain = self.per_chain is not None
        try:
            d = self.detection(loader, self.detect_shifted, by_chain=by_chain)
        except ValueError as e:
            log(f"(Epoch {ep}) detection: {e}")
            return
        rec["detection"] = d
        for task in ("misclassification", "shift"):
            if task not in d:
                continue
            for k in range(self.K if by_chain else 1):
                pick = (lambda v: v[k]) if by_chain else (lambda v: v)
                who = f"over {self.K} chains"
                if by_chain:
                    who = f"chain {self.chain0 + k}: {PC.describe(self.per_chain, self.swept, k)}"
                t = d[task]
                parts = [f"{nm}: AUROC = {pick(t[nm]['auroc']):.4f}, AP = {pick(t[nm]['ap']):.4f}, "
                         f"FPR95 = {pick(t[nm]['fpr95']):.4f}" for nm in DETECTION_SCORES]
                log(f"(Epoch {ep}) {task} detection {who} ({d['members']} members, "
                    f"{pick(t['n_pos'])} positives, {pick(t['n_neg'])} negatives, "
                    f"{pick(t['n_excluded'])} excluded): " + "; ".join(parts))

    # ------------------------------------------------------------ diversity
    def diversity(self, loader):
        """WHICH chains predict the same function?  The pairwise view of the K
        chains over a data loader (the network in eval mode, as `evaluate`):
        [K, K] NumPy matrices `disagreement` (the share of examples on which
        two chains vote differently), `tv` (the mean total variation between
        their predictive distributions), `kl` (directed, kl[i, j] the mean
        KL(chain i || chain j) over the examples where it is finite) with
        `sym_kl` and the `kl_unbounded` counts, `double_fault` (both wrong),
        `error_correlation` (phi of the two chains' errors), `error` [K], and
        n, n_labelled, n_nonfinite (kernels.diversity_summary) — plus `summary`
        (kernels.diversity_pairs): the mean, closest and furthest pair of
        disagreement, tv, sym_kl and double_fault, and `nearest[i]`, the chain
        with the smallest tv to chain i.  A voter is a chain's OWN predictive:
        the uniform mixture of that chain's collected components x nst draws
        (`chain_logprob`'s members, the same Philox keys; `draws` advances as
        an `evaluate` over the loader would advance it), the chain's current
        theta while nothing is collected.  Per batch one kernels.predict sweep
        (groups = K) leaves the K log mixtures on the device and one
        kernels.diversity sweep adds their pair totals there; ONE host read at
        the end.  Works under per_chain (the voters are then different models).
        This process's chains only; K >= 2."""
        _single_process("diversity")
        if self.K < 2:
            raise ValueError("diversity: compares the stacked chains pairwise: it needs K >= 2 "
                             f"(got {self.K})")
        dev = self.args.device
        ptot, tot, bufs = None, None, {}
        was = self.net.training
        self.net.eval()
        try:
            for x, y in loader:
                x, y = x.to(dev), y.to(dev).to(torch.int64).contiguous()
                lg = self._member_logits(x, bufs)
                outs, ptot = K.predict(lg, y, groups=self.K, totals=ptot, want=("logp",))
                tot = K.diversity(outs["logp"], y, totals=tot)
        finally:
            self.net.train(was)
        if tot is None:
            raise ValueError("diversity: the loader is empty")
        res = tot.summary()  # the one host read
        res["summary"] = K.diversity_pairs(res)
        return res

    def _report_diversity(self, ep, rec, loader, log):
        """One [Diversity] log line and rec["diversity"] (the matrices as
        lists) from `diversity()` (run.py --diversity)."""
        try:
            d = self.diversity(loader)
        except ValueError as e:
            log(f"(Epoch {ep}) [Diversity] {e}")
            return
        rec["diversity"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v)
                            for k, v in d.items()}
        s = d["summary"]

        def pair(p):
            return "none" if p is None else f"chains {self.chain0 + p[0]} and {self.chain0 + p[1]}"
        dis = s["disagreement"]
        log(f"(Epoch {ep}) [Diversity] {self.K} chains, {d['n']} examples: disagreement = "
            f"{dis['mean']:.4f} (closest {pair(dis['min_pair'])}: {dis['min']:.4f}, furthest "
            f"{pair(dis['max_pair'])}: {dis['max']:.4f}), tv = {s['tv']['mean']:.4f}, sym_kl = "
            f"{s['sym_kl']['mean']:.4f}, double_fault = {s['double_fault']['mean']:.4f}; "
            f"{d['n_nonfinite']} non-finite")

    # ---------------------------------------------------------- checkpoint
    def state_dict(self):
        """Everything an exact continuation of all K chains needs: the stacked
        theta / momentum / prior, the sampler's step counter (the Philox step
        key), draw counter and the method's moments and counters."""
        st = self.state
        d = {"stacked": type(self).__name__, "K": self.K, "chain0": self.chain0,
             "seed": self.seed, "n": st.n1, "stride": st.stride, "theta": st.theta,
             "mom": st.mom, "prior": st.prior, "step_count": self.step_count,
             "draws": self.draws,
             "per_chain": None if self.per_chain is None else PC.table_for_state(self.per_chain)}
        d.update(self._extra_state())
        return d

    def save_ckpt(self, path):
        torch.save(self.state_dict(), path)
        return path

    def load_ckpt(self, path):
        """Restore a save_ckpt file (weights-only load) into this sampler."""
        d = torch.load(path, map_location=self.state.device, weights_only=True)
        st = self.state
        if (d.get("stacked") != type(self).__name__ or d["K"] != self.K or d["n"] != st.n1
                or d["stride"] != st.stride):
            raise ValueError("load_ckpt: checkpoint of a different stacked sampler / network")
        mine = None if self.per_chain is None else PC.table_for_state(self.per_chain)
        if d.get("per_chain") != mine:
            raise ValueError("load_ckpt: the checkpoint's per_chain table differs from this "
                             "sampler's (the chains would continue under other hyperparameters)")
        with torch.no_grad():
            st.theta.copy_(d["theta"])
            for mine, theirs in ((st.mom, d["mom"]), (st.prior, d["prior"])):
                if mine is not None and theirs is not None:
                    mine.copy_(theirs)
        self.chain0, self.seed = d["chain0"], d["seed"]
        self.step_count, self.draws = d["step_count"], d["draws"]
        self._load_extra_state(d)
        if self._health is not None:  # not checkpointed: the accumulators restart empty
            self._health[0].zero_()
            self._health[2] = 0
        if self._ess is not None:     # nor are these: the next fold is a first sample
            self._ess[1] = 0
        self.function_space_reset()   # nor the function-space ones
        return d

    def train(self, train_loader, test_loader=None, start_epoch=0):
        """Run epochs start_epoch .. args.epochs-1 (start_epoch > 0 continues
        after load_ckpt); logs per-chain losses and, after the epochs
        `_evaluate_after` names, the stacked predictive on test_loader."""
        log = self.logger.info if self.logger is not None else (lambda *_: None)
        hist = []
        for ep in range(start_epoch, self.args.epochs):
            tic = time.time()
            lt, et = self.train_one_epoch(train_loader, ep)
            if self.state.diverged():
                log(f"[Epoch {ep}] a chain wrote a non-finite theta")
            rec = {"epoch": ep, "loss": lt.tolist(), "error": et.tolist(),
                   "seconds": time.time() - tic}
            log(f"[Epoch {ep}/{self.args.epochs}] {self.K} chains: loss = {lt.mean():.4f} "
                f"(min {lt.min():.4f}, max {lt.max():.4f}), error = {et.mean():.4f} "
                f"({rec['seconds']:.2f} s)")
            if self.clip_grad is not None and self.last_clip is not None:
                # (the epoch's sync is behind us: train_one_epoch read its losses)
                lc = self.last_clip.cpu().numpy()
                rec["clip"] = {"clipped": int((lc[:, 1] < 1).sum()), "max_norm": float(lc[:, 0].max())}
                log(f"[Epoch {ep}] clip_grad {self.clip_grad:g}: {rec['clip']['clipped']} of "
                    f"{self.K} chains clipped at the last step, largest gradient norm = "
                    f"{rec['clip']['max_norm']:.4g}")
            if self.gmm_weights and self._evaluate_after(ep, train_loader):
                # opt-in (run.py --gmm_weights): before the evaluation, as the reference
                self._report_gmm(ep, rec, train_loader, test_loader, log)
            if test_loader is not None and self._evaluate_after(ep, train_loader):
                rec["test"] = self.evaluate(test_loader)
                log(f"(Epoch {ep}) stacked predictive: loss = {rec['test'][0]:.4f}, "
                    f"error = {rec['test'][1]:.4f}")
                if getattr(self.args, "uncertainty", False):  # opt-in (run.py --uncertainty)
                    self._report_uncertainty(ep, rec, test_loader, log)
                if getattr(self.args, "detect", False):  # opt-in (run.py --detect)
                    self._report_detection(ep, rec, test_loader, log)
                if getattr(self.args, "diversity", False):  # opt-in (run.py --diversity)
                    self._report_diversity(ep, rec, test_loader, log)
                if getattr(self.args, "stacking", False) and self.stacking_val is not None:
                    # opt-in (run.py --stacking)
                    self._report_stacking(ep, rec, self.stacking_val, test_loader, log)
                if self.per_chain is not None:
                    self._report_chains(ep, rec, test_loader, log)
                if self.exchange_every:  # opt-in (run.py --exchange)
                    self._report_exchange(ep, rec, log)
                if getattr(self.args, "rhat", False):  # opt-in (run.py --rhat)
                    self._report_rhat(ep, rec, log)
                if self.ess_batch:  # opt-in (run.py --ess)
                    self._report_ess(ep, rec, log)
                if self._fn_probe is not None:  # opt-in (run.py --fn_probe)
                    self._report_function_space(ep, rec, log)
            if self.health_every:  # opt-in (run.py --health)
                self._report_health(ep, rec, log)
            hist.append(rec)
        return hist

    def _report_chains(self, ep, rec, loader, log):
        """One log line per chain of a per_chain sweep — its swept values, NLL
        and error (`evaluate_chains`) — and rec["chains"]; the best chain so
        far by NLL in rec["best"]."""
        nll, err = self.evaluate_chains(loader)
        rec["chains"] = {"nll": nll.tolist(), "error": err.tolist()}
        for k in range(self.K):
            log(f"(Epoch {ep}) chain {self.chain0 + k}: {PC.describe(self.per_chain, self.swept, k)}"
                f": loss = {nll[k]:.4f}, error = {err[k]:.4f}")
        ok = np.where(np.isfinite(nll), nll, np.inf)
        rec["best"] = int(np.argmin(ok))

    def _report_rhat(self, ep, rec, log):
        """One log line and rec["rhat"] from `diagnostics()`; an evaluation
        that comes before the diagnostic is defined says so and goes on."""
        try:
            d = self.diagnostics(**({"by_tensor": True} if self._by_tensor() else {}))
        except ValueError as e:
            log(f"(Epoch {ep}) R-hat: {e}")
            return
        rec["rhat"] = d
        shares = ", ".join(f"> {t:g}: {100 * s:.1f} %"
                           for t, s in zip(d["thresholds"], d["share_above"]))
        log(f"(Epoch {ep}) R-hat over {self.K} chains, component {d['component']} "
            f"({d['count']} samples each): max = {d['rhat_max']:.4f} ({d['argmax_param']}), "
            f"mean = {d['rhat_mean']:.4f}, {shares}; {d['n_eval']} evaluated, "
            f"{d['n_degenerate']} degenerate, {d['n_nonfinite']} non-finite")
        self._log_tensors(ep, log, f"R-hat over {self.K} chains", d, "rhat_max", "rhat_mean",
                          "share_above", ">", ".4f", worst=max)


class StackedCSGHMC(_StackedSampler):
    """K cyclical-SGHMC chains of `net` on one device, stepped together.

    `args` carries the csghmc Runner's fields (lr, lr_head, epochs,
    num_cycles, proportion_exploration, ND, hparams with prior_sig,
    momentum_decay, Ninflate, nd, thin, nst, bias; device).  Chains are
    keyed chain0 + k (default: rank * K, so chains stay distinct across
    processes) with Philox seed `seed`."""

    def __init__(self, net, K_, args, **kw):
        super().__init__(net, K_, args, **kw)
        self.momentum_decay = float(args.hparams["momentum_decay"])
        self.sched = CyclicalSGMCMC(base_lr=args.lr, nbr_of_cycles=getattr(args, "num_cycles", 10),
                                    epochs=args.epochs,
                                    proportion_exploration=getattr(args, "proportion_exploration",
                                                                   0.5))
        self.samples_per_cycle, self.mom1, self.mom2 = {}, {}, {}
        if self.per_chain is not None:
            # chain k's own schedule: its lr is a one-chain sampler's with lr_k
            self.scheds = PC.schedules(self.per_chain, args.epochs, self.sched.number_of_cycles,
                                       self.sched.proportion_exploration)

    per_chain_family = "csghmc"
    cyclical = True

    def chain_rows(self, lr):
        """[..., K, 12] fp32 scalar rows for body lrs `lr` ([..., K] float64)."""
        return PC.csghmc_rows(self.per_chain, lr, self.args.ND)

    def epoch_rows(self, epoch, bpe):
        """The [bpe, K, 12] rows of one epoch: every chain's cyclical lr at
        every batch, expanded on the host."""
        lrs = np.stack([PC.cyclical_lrs(self.scheds, epoch, b, bpe) for b in range(bpe)])
        return self.chain_rows(lrs)

    def _health_lr(self, lr, should_sample=False, collect=None, rows=None):
        if self.per_chain is None:
            return (float(lr), float(lr * (self.args.lr_head / self.args.lr))), None, False
        if rows is not None:
            return None, rows, False
        lr_k = np.broadcast_to(np.asarray(lr, dtype=np.float64), (self.K,))
        return None, self._upload_rows(self.chain_rows(lr_k)), True

    def _health_temperatures(self, acc, steps, numel):
        from . import health as H
        pc, ND = self.per_chain, self.args.ND
        if pc is None:
            return H.temperatures(acc, steps, numel, alpha=self.momentum_decay, nd=self.nd,
                                  N=ND * self.Ninflate, prior_sig=self.prior_sig)
        return H.temperatures(acc, steps, numel, alpha=pc["momentum_decay"], nd=pc["nd"],
                              N=np.asarray([ND * float(v) for v in pc["Ninflate"]]),
                              prior_sig=pc["prior_sig"])

    def update(self, grads, lr, should_sample=False, collect=None, rows=None):
        """The fused launch over all chains for given gradients (step's second
        half): v <- v(1-a) - lr(g + prior_sig theta) [+ noise]; theta += v;
        Welford collect on sample steps.  With per_chain, `lr` is the body lr
        per chain ([K]; a scalar is every chain's) and the launch reads chain
        k's scalars from `rows` (a device [K, 12] block; None: formed from lr
        and uploaded here)."""
        args, st = self.args, self.state
        st.use_grads(grads)
        if self.per_chain is not None:
            if rows is None:
                lr_k = np.broadcast_to(np.asarray(lr, dtype=np.float64), (self.K,))
                rows = self._upload_rows(self.chain_rows(lr_k))
            ckind, m1, m2, ca = (L.COLLECT_NONE, None, None, 1.0) if collect is None else collect
            K.chain_step(st, L.CSGHMC, scalars=rows,
                         noise_mode=L.NOISE_PHILOX if should_sample else L.NOISE_NONE,
                         collect=ckind, mom1=m1, mom2=m2, collect_a=ca, seed=self.seed,
                         chain=self.chain0, step=self.step_count)
            self.step_count += 1
            return
        lrs = (lr, lr * (args.lr_head / args.lr))
        N = args.ND * self.Ninflate
        ns = [self.nd * np.sqrt(2 * self.momentum_decay * v) / N for v in lrs]
        ckind, m1, m2, ca = (L.COLLECT_NONE, None, None, 1.0) if collect is None else collect
        K.sgmcmc_step(st, L.CSGHMC, lrs=lrs, noise_scale=ns,
                      noise_mode=L.NOISE_PHILOX if should_sample else L.NOISE_NONE,
                      one_minus_alpha=1 - self.momentum_decay, prior_sig=self.prior_sig,
                      collect=ckind, mom1=m1, mom2=m2, collect_a=ca, seed=self.seed,
                      chain=self.chain0, step=self.step_count)
        self.step_count += 1

    def _collect_spec(self, c):
        """Welford bookkeeping of methods/csghmc.py:333-348 (quirk Q2 double
        count), shared by all chains (they sample on the same steps)."""
        st = self.state
        if c not in self.mom1:
            self.mom1[c] = torch.zeros(st.n, dtype=torch.float32, device=st.device)
            self.mom2[c] = torch.zeros(st.n, dtype=torch.float32, device=st.device)
            return (L.COLLECT_WELFORD_INIT, self.mom1[c], self.mom2[c], 1.0), 1
        n = self.samples_per_cycle.get(c, 0) + 1
        return (L.COLLECT_WELFORD, self.mom1[c], self.mom2[c], float(n)), n

    def train_one_epoch(self, loader, epoch):
        """All batches of one epoch under the cyclical schedule
        (methods/csghmc.py:246-384).  Returns per-chain (loss, error) arrays;
        one host sync per epoch."""
        dev, sched = self.args.device, self.sched
        self.net.train()
        sched.current_epoch = epoch
        bpe = len(loader)
        acc = self._new_acc()
        # per_chain: the epoch's rows in one upload, row b handed to step b
        rows = None if self.per_chain is None else self._upload_rows(self.epoch_rows(epoch, bpe))
        for b, (x, y) in enumerate(loader):
            x, y = x.to(dev, non_blocking=True), y.to(dev, non_blocking=True)
            lr = sched.calculate_lr(epoch=epoch, batch=b, batches_per_epoch=bpe)
            ss = sched.should_sample(epoch=epoch, batch=b, batches_per_epoch=bpe) \
                and b % self.thin == 0
            collect, cnt, c = None, None, None
            if ss:
                c = sched.get_cycle_number(epoch=epoch, batch=b, batches_per_epoch=bpe)
                collect, cnt = self._collect_spec(c)
            kw = {} if rows is None else {"rows": rows[b]}
            loss, out = self.step(x, y, lr, should_sample=ss, collect=collect, **kw)
            if ss:  # Q2: the reference bumps the count twice per sample
                self.samples_per_cycle[c] = cnt + 1
            self._accumulate(acc, loss, out, y)
        return self._epoch_result(acc)

    def _component_keys(self):
        return sorted(self.mom1)  # every collected cycle

    def _moment_spec(self, c):
        """Cycle c: Welford mean and M2 / (n - 1) with n the stored count —
        doubled by quirk Q2, so the cycle holds n // 2 collects per chain (a
        count of 1 or less draws with the variance floor alone, no M2)."""
        if c not in self.mom1:
            return None, None, L.VAR_GIVEN, 1.0, 0
        n = self.samples_per_cycle.get(c, 0)
        if n > 1:
            return self.mom1[c], self.mom2[c], L.VAR_WELFORD, float(n - 1), n // 2
        return self.mom1[c], None, L.VAR_GIVEN, 1.0, n // 2

    def _evaluate_after(self, ep, loader):
        return self.sched.last_in_cycle(epoch=ep, batch=len(loader) - 1,
                                        batches_per_epoch=len(loader))

    def _extra_state(self):
        return {"samples_per_cycle": dict(self.samples_per_cycle), "mom1": dict(self.mom1),
                "mom2": dict(self.mom2), "epoch": self.sched.current_epoch, **self._gmm_state()}

    def _load_extra_state(self, d):
        self.samples_per_cycle = dict(d["samples_per_cycle"])
        self.mom1, self.mom2 = dict(d["mom1"]), dict(d["mom2"])
        self.sched.current_epoch = d["epoch"]
        self._load_gmm_state(d)

    def export_chain(self, k, epoch=None):
        """Chain k as a one-chain csghmc checkpoint (the keys of
        methods/csghmc.py:530-549 / bayesdll_amd.csghmc.Runner.save_ckpt, flat
        vectors in parameters_to_vector order): `torch.save` it and a
        Runner's load_ckpt takes it."""
        st, n1 = self.state, self.state.n1
        sl = (lambda v: v.view(self.K, st.stride)[k, :n1].clone())
        return {"last_theta": st.chain_vector(k).clone(),
                "cycle_theta_mom1": {c: sl(v) for c, v in self.mom1.items()},
                "cycle_theta_mom2": {c: sl(v) for c, v in self.mom2.items()},
                "cycle_likelihoods": {}, "cycle_states": {},
                "epoch": self.sched.current_epoch if epoch is None else epoch,
                "current_cycle": max(self.mom1) if self.mom1 else 0,
                "samples_per_cycle": dict(self.samples_per_cycle)}


class StackedSGLD(_StackedSampler):
    """K SGLD chains of `net` on one device (methods/sgld.py:69-250 per chain):
    sampler gradient g + (theta - theta0)/sigma^2/N + nd*sqrt(2/(N lr))*eps,
    then torch.optim.SGD(momentum=args.momentum) — one fused launch for all
    chains — with the running posterior moments (m1, m2) after burn-in every
    `thin` iterations fused into the same sweep.  `args` carries the sgld
    Runner's fields (lr, lr_head, epochs, momentum, ND, hparams with
    prior_sig, Ninflate, nd, burnin, thin, nst, bias; device); `net0` is the
    prior mean (zeros when None)."""

    need_prior = True
    tune_method = "sgld"
    per_chain_family = "sgld"
    exchange_ok = True  # momentum 0: chain k samples exp(-U / nd_k^2)

    def __init__(self, net, K_, args, **kw):
        super().__init__(net, K_, args, **kw)
        self.burnin = int(args.hparams["burnin"])
        self.mu = float(getattr(args, "momentum", 0.0))
        if self.per_chain is not None:  # all zero or all non-zero (per_chain.parse)
            self.mu = float(self.per_chain["momentum"][0])
        self.has_buffer = False
        self.bi = 0                      # global iteration count thinning uses
        self.m1 = self.m2 = None
        self.cnt = 0

    def chain_rows(self, lr, lr_head):
        """[..., K, 12] fp32 scalar rows for body / head lrs ([..., K] float64)."""
        return PC.sgld_rows(self.per_chain, lr, lr_head, self.args.ND)

    def epoch_rows(self, epoch, bpe):
        """The [bpe, K, 12] rows of one epoch (constant lr: the same row block
        at every batch)."""
        r = self.chain_rows(self.per_chain["lr"], self.per_chain["lr_head"])
        return np.broadcast_to(r, (bpe,) + r.shape)

    def update(self, grads, lrs, collect=None, rows=None):
        """The fused SGLD + SGD(momentum mu) launch over all chains
        (methods/sgld.py:469-484 + :226), optional running-moment collect.
        With per_chain, lrs = (body, head) lr per chain ([K] each; a scalar is
        every chain's) and the launch reads chain k's scalars from `rows` (a
        device [K, 12] block; None: formed from lrs and uploaded here)."""
        args, st = self.args, self.state
        st.use_grads(grads)
        mom = self.mu != 0
        ckind, m1, m2, ca, cb = (L.COLLECT_NONE, None, None, 1.0, 1.0) if collect is None \
            else collect
        if self.per_chain is not None:
            if rows is None:
                l0, l1 = (np.broadcast_to(np.asarray(v, dtype=np.float64), (self.K,)) for v in lrs)
                rows = self._upload_rows(self.chain_rows(l0, l1))
            K.chain_step(st, L.SGLD, scalars=rows, noise_mode=L.NOISE_PHILOX,
                         first_step=mom and not self.has_buffer, momentum=mom, collect=ckind,
                         mom1=m1, mom2=m2, collect_a=ca, collect_b=cb, seed=self.seed,
                         chain=self.chain0, step=self.step_count)
            self.has_buffer = self.has_buffer or mom
            self.step_count += 1
            return
        N = args.ND * self.Ninflate
        ns = [self.nd * np.sqrt(2 / (N * v)) for v in lrs]
        key = dict(seed=self.seed, chain=self.chain0, step=self.step_count)
        sgd_kw = dict(mu=self.mu, first_step=mom and not self.has_buffer, momentum=mom,
                      collect=ckind, mom1=m1, mom2=m2, collect_a=ca, collect_b=cb)
        if self.clip_grad is not None:
            # methods/csgld.py:250-253: clip_grad_norm_ on p.grad between
            # Model.forward and optimizer.step, per chain: the sampler gradient
            # in place, each chain's own norm and scale, then SGD's step alone
            K.sgmcmc_step(st, L.SGLD_GRAD, lrs=lrs, noise_scale=ns, noise_mode=L.NOISE_PHILOX,
                          prior_sig=self.prior_sig, sigma2=self.prior_sig ** 2, n_data=N, **key)
            self._clip_chains()
            K.sgmcmc_step(st, L.SGLD, lrs=lrs, noise_scale=(0.0, 0.0), noise_mode=L.NOISE_NONE,
                          sigma2=1.0, n_data=1.0, grad_ready=True, **sgd_kw, **key)
        else:
            K.sgmcmc_step(st, L.SGLD, lrs=lrs, noise_scale=ns, noise_mode=L.NOISE_PHILOX,
                          prior_sig=self.prior_sig, sigma2=self.prior_sig ** 2, n_data=N,
                          **sgd_kw, **key)
        self.has_buffer = self.has_buffer or mom
        self.step_count += 1

    def seed_moments(self):
        """methods/sgld.py:95-102 at the end of burn-in: m1 = theta,
        m2 = theta^2, count 1 (one stand-alone sweep over all chains)."""
        st = self.state
        self.m1 = torch.empty_like(st.theta)
        self.m2 = torch.empty_like(st.theta) if self.nst > 0 else None
        K.moments_update(st.theta, self.m1, self.m2, L.COLLECT_MEAN_INIT)
        self.cnt = 1

    def train_one_epoch(self, loader, epoch):
        args, dev = self.args, self.args.device
        self.net.train()
        if epoch == self.burnin:
            self.seed_moments()
        collect = epoch >= self.burnin
        lrs = (args.lr, args.lr_head)
        acc = self._new_acc()
        # per_chain: the epoch's rows in one upload (one block: the lr is constant)
        kw = {} if self.per_chain is None else \
            {"rows": self._upload_rows(self.epoch_rows(epoch, 1))[0]}
        for x, y in loader:
            x, y = x.to(dev, non_blocking=True), y.to(dev, non_blocking=True)
            spec = None
            do_collect = collect and (self.bi + 1) % self.thin == 0
            if do_collect:  # methods/sgld.py:239-246
                spec = (L.COLLECT_MEAN, self.m1, self.m2, float(self.cnt), float(self.cnt + 1))
            loss, out = self.step(x, y, lrs, collect=spec, **kw)
            if do_collect:
                self.cnt += 1
            self.bi += 1
            self._accumulate(acc, loss, out, y)
        return self._epoch_result(acc)

    def _component_keys(self):
        return [] if self.m1 is None else [0]  # the one running component

    def _moment_spec(self, component=0):
        """The one component: running (m1, m2) over cnt collects, the burn-in
        seed included; var = cnt/(cnt-1) * (m2 - m1^2), ratio 1 for one sample."""
        if self.m1 is None or component != 0:
            return None, None, L.VAR_RAW_MOMENTS, 1.0, 0
        ratio = self.cnt / (self.cnt - 1) if self.cnt > 1 else 1.0
        return self.m1, self.m2, L.VAR_RAW_MOMENTS, ratio, self.cnt

    def _evaluate_after(self, ep, loader):
        freq = int(getattr(self.args, "test_eval_freq", 1) or 1)
        return ep >= self.burnin and ((ep + 1) % freq == 0 or ep + 1 == self.args.epochs)

    def _extra_state(self):
        return {"m1": self.m1, "m2": self.m2, "cnt": self.cnt, "bi": self.bi,
                "has_buffer": self.has_buffer, **self._exchange_ckpt()}

    def _load_extra_state(self, d):
        self.m1, self.m2 = d["m1"], d["m2"]
        self.cnt, self.bi, self.has_buffer = d["cnt"], d["bi"], d["has_buffer"]
        self._load_exchange_ckpt(d)


class StackedCSGLD(StackedSGLD):
    """K cyclical-SGLD chains (methods/csgld.py:195-331 per chain): SGLD + SGD
    momentum under the cyclical step size, per-cycle running moments
    (m1 = theta, m2 = theta^2 at a cycle's first sample, then the running
    mean) on the sample steps.  No burn-in; `args` as the csgld Runner's,
    args.clip_grad included (:250-253): every chain is clipped by the norm of
    its own sampler gradient (`_clip_chains`)."""

    cyclical = True

    def __init__(self, net, K_, args, **kw):
        super().__init__(net, K_, args, **kw)
        self.burnin = -1  # cSGLD collects per cycle, not after a burn-in
        clip = getattr(args, "clip_grad", None)
        if clip is not None and not float(clip) > 0:
            raise ValueError(f"clip_grad must be > 0 (got {clip})")
        self.clip_grad = None if clip is None else float(clip)
        self.sched = CyclicalSGMCMC(base_lr=args.lr, nbr_of_cycles=getattr(args, "num_cycles", 10),
                                    epochs=args.epochs,
                                    proportion_exploration=getattr(args, "proportion_exploration",
                                                                   0.5))
        self.samples_per_cycle, self.mom1, self.mom2 = {}, {}, {}
        if self.per_chain is not None:
            # chain k's own schedule: its lr is a one-chain sampler's with lr_k
            self.scheds = PC.schedules(self.per_chain, args.epochs, self.sched.number_of_cycles,
                                       self.sched.proportion_exploration)

    def epoch_rows(self, epoch, bpe):
        """The [bpe, K, 12] rows of one epoch: every chain's cyclical lr (and
        head lr = lr * (lr_head / lr_base)) at every batch."""
        lrs = np.stack([PC.cyclical_lrs(self.scheds, epoch, b, bpe) for b in range(bpe)])
        return self.chain_rows(lrs, PC.head_lrs(self.per_chain, lrs))

    def train_one_epoch(self, loader, epoch):
        args, dev, sched = self.args, self.args.device, self.sched
        self.net.train()
        sched.current_epoch = epoch
        bpe = len(loader)
        acc = self._new_acc()
        st = self.state
        rows = None if self.per_chain is None else self._upload_rows(self.epoch_rows(epoch, bpe))
        for b, (x, y) in enumerate(loader):
            x, y = x.to(dev, non_blocking=True), y.to(dev, non_blocking=True)
            lr = sched.calculate_lr(epoch=epoch, batch=b, batches_per_epoch=bpe)
            ss = sched.should_sample(epoch=epoch, batch=b, batches_per_epoch=bpe) \
                and b % self.thin == 0
            spec, c = None, None
            if ss:  # methods/csgld.py:280-293
                c = sched.get_cycle_number(epoch=epoch, batch=b, batches_per_epoch=bpe)
                if c not in self.mom1:
                    self.mom1[c] = torch.zeros_like(st.theta)
                    self.mom2[c] = torch.zeros_like(st.theta)
                    spec = (L.COLLECT_MEAN_INIT, self.mom1[c], self.mom2[c], 1.0, 1.0)
                else:
                    cc = self.samples_per_cycle.get(c, 0) + 1
                    spec = (L.COLLECT_MEAN, self.mom1[c], self.mom2[c], float(cc - 1), float(cc))
            kw = {} if rows is None else {"rows": rows[b]}
            loss, out = self.step(x, y, (lr, lr * (args.lr_head / args.lr)), collect=spec, **kw)
            if ss:
                self.samples_per_cycle[c] = self.samples_per_cycle.get(c, 0) + 1
            if sched.last_in_cycle(epoch=epoch, batch=b, batches_per_epoch=bpe):
                self._cycle_end()
            self._accumulate(acc, loss, out, y)
        return self._epoch_result(acc)

    def _cycle_end(self):
        """Hook at every last_in_cycle step, after the step and its collect
        (bayesdll_amd.csgld.Runner._cycle_end)."""

    def _component_keys(self):
        return sorted(self.mom1)  # every collected cycle

    def _moment_spec(self, c):
        """Cycle c: running (m1, m2) over its spc collects; var = spc/(spc-1) *
        (m2 - m1^2), ratio 1 for a one-sample cycle."""
        if c not in self.mom1:
            return None, None, L.VAR_RAW_MOMENTS, 1.0, 0
        spc = self.samples_per_cycle.get(c, 0)
        return (self.mom1[c], self.mom2[c], L.VAR_RAW_MOMENTS,
                spc / (spc - 1) if spc > 1 else 1.0, spc)

    def _evaluate_after(self, ep, loader):
        return self.sched.last_in_cycle(epoch=ep, batch=len(loader) - 1,
                                        batches_per_epoch=len(loader))

    def _extra_state(self):
        return {"samples_per_cycle": dict(self.samples_per_cycle), "mom1": dict(self.mom1),
                "mom2": dict(self.mom2), "has_buffer": self.has_buffer,
                "epoch": self.sched.current_epoch, **self._gmm_state(), **self._exchange_ckpt()}

    def _load_extra_state(self, d):
        self.samples_per_cycle = dict(d["samples_per_cycle"])
        self.mom1, self.mom2 = dict(d["mom1"]), dict(d["mom2"])
        self.has_buffer, self.sched.current_epoch = d["has_buffer"], d["epoch"]
        self._load_gmm_state(d)
        self._load_exchange_ckpt(d)


class StackedSGHMC(StackedSGLD):
    """K SGHMC chains (methods/sghmc.py:16-512 per chain): momentum
    v' = v(1-a) + lr-scaled sampler gradient with the prior pull and
    nd*sqrt(2a/(N lr)) noise, then SGD(momentum 0) on g + v' — one fused
    launch for all chains — and the SGLD Runner's burn-in / thinned running
    moments.  `args` as the sghmc Runner's (hparams with momentum_decay)."""

    per_chain_family = None  # no per-chain SGHMC launch
    exchange_ok = False       # and no temperature is derived for it

    def __init__(self, net, K_, args, **kw):
        super().__init__(net, K_, args, **kw)
        self.momentum_decay = float(args.hparams["momentum_decay"])
        self.mu = 0.0

    def update(self, grads, lrs, collect=None):
        args, st = self.args, self.state
        st.use_grads(grads)
        N = args.ND * self.Ninflate
        ns = [self.nd * np.sqrt(2 * self.momentum_decay / (N * v)) for v in lrs]
        ckind, m1, m2, ca, cb = (L.COLLECT_NONE, None, None, 1.0, 1.0) if collect is None \
            else collect
        K.sgmcmc_step(st, L.SGHMC, lrs=lrs, noise_scale=ns, noise_mode=L.NOISE_PHILOX,
                      one_minus_alpha=1 - self.momentum_decay, prior_sig=self.prior_sig,
                      sigma2=self.prior_sig ** 2, n_data=N, collect=ckind, mom1=m1, mom2=m2,
                      collect_a=ca, collect_b=cb, seed=self.seed, chain=self.chain0,
                      step=self.step_count)
        self.step_count += 1


class _AdamStep:
    """The Adam-preconditioned SGHMC step of K stacked chains
    (bayesdll_amd.adam_sghmc.Model.forward's `sgd is not None` branch, per
    chain): v_mom in the state's momentum vector, the stacked adam_m / adam_v /
    sgd_buf in `state.extra` (kernels.ADAM_EXTRA), one step counter t for all
    chains — they step together —, incremented before the launch.  Mixed into
    the SGLD / cSGLD stacked samplers, whose loops, moments and evaluation
    stay as they are."""

    tune_method = "adam"
    per_chain_family = None  # no per-chain Adam launch
    exchange_ok = False       # and no temperature is derived for it
    grad_is_mom = False  # the cyclical variant's p.grad = v_mom (adam_csghmc.py:834)

    def _init_adam(self):
        hp, st = self.args.hparams, self.state
        self.momentum_decay = float(hp["momentum_decay"])
        self.beta1 = float(hp.get("beta1", 0.9))
        self.beta2 = float(hp.get("beta2", 0.999))
        self.epsilon = float(hp.get("epsilon", 1e-8))
        self.temperature = float(hp.get("temperature", 1.0))
        self.t = 0
        for nm in K.ADAM_EXTRA[:2]:
            st.extra[nm] = torch.zeros_like(st.theta)

    def _sgd_buffer(self):
        """The stacked torch.optim.SGD momentum buffer (allocated when SGD
        momentum is in use: adam_sghmc.Model.ensure_sgd_buffer)."""
        ex = self.state.extra
        if "sgd_buf" not in ex:
            ex["sgd_buf"] = torch.zeros_like(self.state.theta)
        return ex["sgd_buf"]

    def update(self, grads, lrs, collect=None):
        """One fused Adam-SGHMC + SGD launch over all chains
        (methods/adam_sghmc.py:500-553 + :229), optional running-moment
        collect; with clip_grad, adam_sghmc.Model.forward's clip branch: the
        ADAM_SGHMC_GRAD launch, every chain's own clip, SGD's step."""
        args, st = self.args, self.state
        st.use_grads(grads)
        self.t += 1
        N = args.ND * self.Ninflate
        key = dict(seed=self.seed, chain=self.chain0, step=self.step_count)
        common = dict(adam_m=st.extra["adam_m"], adam_v=st.extra["adam_v"], beta1=self.beta1,
                      beta2=self.beta2, eps=self.epsilon, t=self.t,
                      momentum_decay=self.momentum_decay, nd=self.nd,
                      temperature=self.temperature, grad_is_mom=self.grad_is_mom, lrs=lrs,
                      noise_mode=L.NOISE_PHILOX, sigma2=self.prior_sig ** 2, n_data=N, **key)
        ckind, m1, m2, ca, cb = (L.COLLECT_NONE, None, None, 1.0, 1.0) if collect is None \
            else collect
        mom = self.mu != 0
        buf = self._sgd_buffer() if mom else None
        sgd_kw = dict(mu=self.mu, first_step=mom and not self.has_buffer, momentum=mom,
                      collect=ckind, mom1=m1, mom2=m2, collect_a=ca, collect_b=cb)
        if self.clip_grad is not None:
            # adam_csghmc.py:319-322: clip_grad_norm_ on p.grad between
            # Model.forward and optimizer.step, per chain
            K.adam_step(st, L.ADAM_SGHMC_GRAD, **common)
            self._clip_chains()
            K.sgmcmc_step(st, L.SGLD, lrs=lrs, noise_scale=(0.0, 0.0), noise_mode=L.NOISE_NONE,
                          sigma2=1.0, n_data=1.0, grad_ready=True, mom_buf=buf, **sgd_kw, **key)
        else:
            K.adam_step(st, L.ADAM_SGHMC, sgd_buf=buf, **common, **sgd_kw)
        self.has_buffer = self.has_buffer or mom
        self.step_count += 1

    def reset_adam(self):
        """Zero v_mom, m, v and t (adam_sghmc.Model.reset_adam;
        methods/adam_csghmc.py:372-378, :119-131)."""
        st = self.state
        st.mom.zero_()
        st.extra["adam_m"].zero_()
        st.extra["adam_v"].zero_()
        self.t = 0

    def _extra_state(self):
        ex = self.state.extra
        return dict(super()._extra_state(), adam_m=ex["adam_m"], adam_v=ex["adam_v"],
                    sgd_buf=ex.get("sgd_buf"), t=self.t, has_buffer=self.has_buffer)

    def _load_extra_state(self, d):
        super()._load_extra_state(d)
        ex = self.state.extra
        with torch.no_grad():
            ex["adam_m"].copy_(d["adam_m"])
            ex["adam_v"].copy_(d["adam_v"])
            if d["sgd_buf"] is not None:
                self._sgd_buffer().copy_(d["sgd_buf"])
        self.t, self.has_buffer = int(d["t"]), bool(d["has_buffer"])


class StackedAdamSGHMC(_AdamStep, StackedSGLD):
    """K Adam-preconditioned SGHMC chains (methods/adam_sghmc.py:16-556 per
    chain; bayesdll_amd.adam_sghmc): the Adam-SGHMC momentum update and
    SGD(momentum=args.momentum) in one fused launch for all chains, under the
    SGLD Runner's burn-in / thinned running moments.  `args` as the adam_sghmc
    Runner's (hparams with momentum_decay, beta1, beta2, epsilon,
    temperature).  No clipping: the reference's Runner has none."""

    def __init__(self, net, K_, args, **kw):
        super().__init__(net, K_, args, **kw)
        self._init_adam()


class StackedAdamCSGHMC(_AdamStep, StackedCSGLD):
    """K cyclical Adam-SGHMC chains (methods/adam_csghmc.py:17-863 per chain;
    bayesdll_amd.adam_csghmc): grad_U = g / temperature + prior pull,
    p.grad = v_mom, SGD momentum forced to 0 (:70), the cyclical step size and
    csgld's per-cycle running moments; v_mom, m, v and t zeroed at every
    last_in_cycle step (:372-378); args.clip_grad clips every chain by its own
    norm (:319-322).  Cold restarts (perform_cold_restarts: a per-chain
    re-initialisation mid-run) are not stacked."""

    grad_is_mom = True

    def __init__(self, net, K_, args, **kw):
        if str(args.hparams.get("perform_cold_restarts", False)).lower() == "true":
            raise ValueError("StackedAdamCSGHMC: perform_cold_restarts=true is not supported by "
                             "stacked chains (run one chain per process for cold restarts)")
        super().__init__(net, K_, args, **kw)
        self._init_adam()
        self.mu = 0.0  # :70 "Force SGD optimizer momentum to 0"

    def _cycle_end(self):
        self.reset_adam()
