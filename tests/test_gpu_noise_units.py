"""Every step unit's Philox instances tied to the reference-checked stream.

The generator is compiled differently per translation unit (csrc/Makefile:
three-input bit op or two xors, round keys hoisted or per call), and inside
the units its inputs are held in SGPRs, re-read per call, or read through the
re-read argument view, depending on method, collect kind and unroll depth.
test_gpu_noise_stream.py pins bdl_philox_normal to the host reference; here
each instance must consume exactly that stream:

* one step with NOISE_PHILOX equals, bit for bit in every vector it writes,
  the same step from the same state with NOISE_BUFFER fed
  philox_normal(n, seed, chain, step) — every method and collect kind, at
  unroll depths 1, 2 and 4, with a 64-bit seed and a step above 2^32;
* stepped as two launches split at a 4-aligned run boundary, the second with
  philox_offset = split / 4, it equals the single launch;
* *_GRAD followed by the grad-ready step equals the fused step (buffer noise,
  depths 1, 2, 4), and the plain buffer-noise steps, the clipped step and the
  *_GRAD -> grad-ready pair give the depth-1 bits at every geometry.

One segment table of 39,426 elements (n % 4 = 2) serves all of it: a tensor
of 3 x 4096 + 1024 elements at the start (whole depth-4 iterations inside one
run: the fast path), 4-aligned tensors of 4 to 1024 elements (iterations that
cross run boundaries on float4 groups: the multi-run path), two adjacent odd
sizes 3 and 5 and a frozen tensor (the guarded path), a readout head, and
uninformative biases (every bias its own run).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SEGMENTS = [
    ("l0.weight", 13312), ("l0.bias", 1024), ("l1.weight", 4), ("l1.bias", 256),
    ("l2.weight", 64), ("l2.bias", 100), ("l3.weight", 1000), ("l3.bias", 512),
    ("l4.weight", 8), ("l4.bias", 12), ("l5.weight", 3), ("l5.bias", 5),
    ("l6.weight", 9000), ("l6.bias", 1000),
    ("l7.weight", 2048),  # frozen (BDL_ATTR_SKIP)
    ("l7.bias", 48), ("l8.weight", 10000), ("l8.bias", 20),
    ("head.weight", 1000), ("head.bias", 10),
]
FROZEN = "l7.weight"
SPLIT_AFTER = "l6.bias"  # the two-launch split: a run boundary on a float4 group
SEED, CHAIN, STEP = 0x9E3779B97F4A7C15, 3, 2 ** 32 + 9

# (workgroups per CU, unroll depth, grid-stride): depth 1 holds the SGLD / SGHMC
# collects' generator inputs in SGPRs, depth 2 / 4 read them through the re-read
# argument view (collect and buffer instances) or per call
DEPTHS = [(1, 1, 1), (1, 2, 1), (1, 4, 1), (2, 4, 0)]
GEOMETRIES = [(1, 1, 0), (1, 2, 1), (1, 4, 1), (2, 1, 1), (2, 4, 0), (3, 2, 1), (4, 4, 1)]

VECTORS = ("theta", "grad", "mom", "prior", "noise", "m1", "m2", "adam_m", "adam_v", "sgd_buf")
WRITTEN = ("theta", "grad", "mom", "m1", "m2", "adam_m", "adam_v", "sgd_buf")
_SCALE = dict(theta=0.02, grad=1e-2, mom=1e-3, prior=0.02, noise=1.0, m1=0.02, m2=1e-3,
              adam_m=1e-3, adam_v=1e-6, sgd_buf=1e-3)


class Table:
    """The flat vectors of one chain over SEGMENTS and the run table of any
    range of whole tensors (states for kernels.sgmcmc_step and friends)."""
    _init = None

    def __init__(self):
        from bayesdll_amd.flat import segment_attrs
        self.names = [nm for nm, _ in SEGMENTS]
        self.numels = [k for _, k in SEGMENTS]
        self.offsets = np.concatenate([[0], np.cumsum(self.numels)[:-1]]).tolist()
        self.n = int(sum(self.numels))
        self.attrs = segment_attrs(self.names, "head", "uninformative",
                                   [nm != FROZEN for nm in self.names])
        if Table._init is None:  # one set of start values for every state
            rng = np.random.default_rng(2024)
            init = {}
            for nm in VECTORS:
                x = rng.standard_normal(self.n).astype(np.float32) * np.float32(_SCALE[nm])
                init[nm] = torch.from_numpy(np.abs(x) if nm in ("m2", "adam_v") else x)
            Table._init = init
        self.v = {nm: t.to(DEV) for nm, t in Table._init.items()}
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.split = self.offsets[self.names.index(SPLIT_AFTER) + 1]
        self._states = {}

    def state(self, lo=0, hi=None):
        """A launchable state over elements [lo, hi) (tensor boundaries)."""
        from bayesdll_amd.flat import build_runs
        hi = self.n if hi is None else hi
        st = self._states.get((lo, hi))
        if st is None:
            idx = [i for i, o in enumerate(self.offsets) if lo <= o < hi]
            assert self.offsets[idx[0]] == lo and self.offsets[idx[-1]] + self.numels[idx[-1]] == hi
            runs = build_runs([self.offsets[i] - lo for i in idx], [self.numels[i] for i in idx],
                              [self.attrs[i] for i in idx], hi - lo).to(DEV)
            v = {nm: t[lo:hi] for nm, t in self.v.items()}
            st = SimpleNamespace(theta=v["theta"], grad=v["grad"], gbase=None, mom=v["mom"],
                                 prior=v["prior"], noise=v["noise"], runs=runs,
                                 nruns=int(runs.shape[0]), n=hi - lo, device=torch.device(DEV, 0),
                                 nonfinite=self.nonfinite, timer=None, v=v)
            self._states[(lo, hi)] = st
        return st

    def written(self):
        return {nm: self.v[nm].clone() for nm in WRITTEN}


def test_table_reaches_every_path():
    t = Table()
    assert t.n == 39426 and t.n % 4 == 2
    assert t.numels[0] >= 3 * 4096 + 4 and t.offsets[0] == 0  # whole depth-4 iterations in one run
    assert t.split % 4 == 0 and 0 < t.split < t.n
    assert sum(1 for o, k in zip(t.offsets, t.numels) if o % 4 == 0 and k % 4 == 0 and k <= 1024) >= 6
    i = t.names.index("l5.weight")
    assert t.numels[i:i + 2] == [3, 5] and t.offsets[i + 1] % 4 == 3
    st = t.state()
    assert st.nruns >= 15  # uninformative biases, the frozen tensor and the head split the runs
    assert any(a & 4 for a in t.attrs) and any(a & 1 for a in t.attrs)


# --------------------------------------------------------------------- cases
LRS, N_DATA, ND = (1e-3, 2e-2), 1840.0, 0.5


def _ns(f):
    return [ND * f(lr) for lr in LRS]


def _cases():
    """case -> list of launches (entry, method name, keyword arguments); launch
    t is keyed step STEP + t."""
    csg = dict(lrs=LRS, noise_scale=_ns(lambda lr: np.sqrt(2 * 0.18 * lr)), one_minus_alpha=0.82,
               prior_sig=1.0)
    sgld = dict(lrs=LRS, noise_scale=_ns(lambda lr: np.sqrt(2 / (N_DATA * lr))), sigma2=1.0,
                n_data=N_DATA)
    sghmc = dict(lrs=LRS, noise_scale=_ns(lambda lr: np.sqrt(2 * 0.18 / (N_DATA * lr))),
                 one_minus_alpha=0.82, sigma2=1.0, n_data=N_DATA)
    adam = dict(beta1=0.9, beta2=0.999, eps=1e-8, momentum_decay=0.18, nd=ND, lrs=LRS,
                sigma2=1.0, n_data=N_DATA)
    mom = dict(mu=0.5, momentum=True)
    return {
        "csghmc_sample": [("step", "CSGHMC", csg)],
        "csghmc_welford": [
            ("step", "CSGHMC", dict(csg, collect="WELFORD_INIT", collect_a=1.0)),
            ("step", "CSGHMC", dict(csg, collect="WELFORD", collect_a=2.0))],
        "sgld_momentum": [("step", "SGLD", dict(sgld, first_step=True, **mom)),
                          ("step", "SGLD", dict(sgld, **mom))],
        "sgld_collect_mean": [
            ("step", "SGLD", dict(sgld, collect="MEAN", collect_a=2.0, collect_b=3.0, **mom))],
        "sgld_grad": [("step", "SGLD_GRAD", sgld)],
        "sgld_clipped": [("clipped", "SGLD", dict(sgld, **mom))],
        "sghmc": [("step", "SGHMC", sghmc)],
        "sghmc_collect_mean": [
            ("step", "SGHMC", dict(sghmc, collect="MEAN_INIT", collect_a=1.0, collect_b=2.0)),
            ("step", "SGHMC", dict(sghmc, collect="MEAN", collect_a=2.0, collect_b=3.0))],
        "sghmc_grad": [("step", "SGHMC_GRAD", sghmc)],
        "adam": [("adam", "ADAM_SGHMC", dict(adam, t=3, sgd=False))],
        "adam_sgd_buffer": [
            ("adam", "ADAM_SGHMC", dict(adam, t=1, sgd=True, first_step=True, **mom)),
            ("adam", "ADAM_SGHMC", dict(adam, t=2, sgd=True, collect="MEAN", collect_a=2.0,
                                        collect_b=3.0, **mom))],
        "adam_grad": [("adam", "ADAM_SGHMC_GRAD", dict(adam, t=3, sgd=False))],
    }


CASES = _cases()
MAX_NORM = 1.0  # clips: the sampler gradient's norm over the table is ~100x that


def _launch(st, spec, noise_mode, step, philox_offset=0, max_norm=MAX_NORM):
    """One launch of `spec` over the state `st`; returns the clipped step's
    (norm, coef) workspace, else None."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    entry, method, kw = spec
    kw = dict(kw)
    sgd = kw.pop("sgd", False)
    if "collect" in kw:
        kw.update(collect=getattr(L, "COLLECT_" + kw["collect"]), mom1=st.v["m1"], mom2=st.v["m2"])
    kw.update(noise_mode=noise_mode, seed=SEED, chain=CHAIN, step=step, philox_offset=philox_offset)
    method = getattr(L, method)
    if entry == "adam":
        K.adam_step(st, method, adam_m=st.v["adam_m"], adam_v=st.v["adam_v"],
                    sgd_buf=st.v["sgd_buf"] if sgd else None, **kw)
    elif entry == "clipped":
        return K.sgld_step_clipped(st, max_norm, **kw)
    else:
        K.sgmcmc_step(st, method, **kw)
    return None


def _run_case(case, mode, max_norm=MAX_NORM):
    """The case's launches from the table's start values.  mode: "philox";
    "buffer" (NOISE_BUFFER fed bdl_philox_normal's stream); "offset" (Philox,
    each launch as two sub-range launches).  Returns the written vectors and
    the clip workspaces' (norm, coef)."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    t = Table()
    clips = []
    for i, spec in enumerate(CASES[case]):
        step = STEP + i
        if mode == "buffer":
            t.v["noise"].copy_(K.philox_normal(t.n, SEED, CHAIN, step, device=DEV))
            ws = [_launch(t.state(), spec, L.NOISE_BUFFER, step, max_norm=max_norm)]
        elif mode == "offset":
            ws = [_launch(t.state(0, t.split), spec, L.NOISE_PHILOX, step, max_norm=max_norm),
                  _launch(t.state(t.split, t.n), spec, L.NOISE_PHILOX, step,
                          philox_offset=t.split // 4, max_norm=max_norm)]
        else:
            ws = [_launch(t.state(), spec, L.NOISE_PHILOX, step, max_norm=max_norm)]
        clips += [w[:2].clone() for w in ws if w is not None]
    torch.cuda.synchronize()
    assert int(t.nonfinite.item()) == 0
    return t.written(), clips


def _assert_same(a, b, what):
    for nm in WRITTEN:
        assert torch.equal(a[nm], b[nm]), (what, nm)


@pytest.mark.parametrize("geo", DEPTHS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("case", list(CASES))
def test_philox_step_consumes_the_reference_checked_stream(case, geo):
    from bayesdll_amd import kernels as K
    try:
        K.set_launch_config(*geo)
        philox, clip_p = _run_case(case, "philox")
        buffer, clip_b = _run_case(case, "buffer")
    finally:
        K.set_launch_config(0, 0, 0)
    _assert_same(philox, buffer, (case, geo))
    start = Table._init
    for nm in WRITTEN:  # the case wrote what it is about (the noise reached it)
        if nm in _CASE_WRITES[case]:
            assert not torch.equal(philox[nm].cpu(), start[nm]), (case, nm)
    for p, b in zip(clip_p, clip_b):
        assert torch.equal(p, b) and p[1].item() < 1.0, (case, geo)  # clipping active


_CASE_WRITES = {
    "csghmc_sample": ("theta", "mom"), "csghmc_welford": ("theta", "mom", "m1", "m2"),
    "sgld_momentum": ("theta", "mom"), "sgld_collect_mean": ("theta", "mom", "m1", "m2"),
    "sgld_grad": ("grad",), "sgld_clipped": ("theta", "mom"), "sghmc": ("theta", "mom"),
    "sghmc_collect_mean": ("theta", "mom", "m1", "m2"), "sghmc_grad": ("grad", "mom"),
    "adam": ("theta", "mom", "adam_m", "adam_v"),
    "adam_sgd_buffer": ("theta", "mom", "adam_m", "adam_v", "sgd_buf", "m1", "m2"),
    "adam_grad": ("grad", "mom", "adam_m", "adam_v"),
}


@pytest.mark.parametrize("geo", DEPTHS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("case", list(CASES))
def test_philox_offset_split_equals_one_launch(case, geo):
    """Two launches split at a 4-aligned run boundary, the second with
    philox_offset = split / 4, equal the single launch.  The clipped step's
    norm is over the launch's own range: with max_norm far above it (coef
    exactly 1 in every launch) the update is the single launch's, and the two
    sub-range norms add up to the whole one (a norm over another stream's
    draws would differ by ~1 / sqrt(n), a thousand times the bound here)."""
    from bayesdll_amd import kernels as K
    max_norm = 1e30 if case == "sgld_clipped" else MAX_NORM
    try:
        K.set_launch_config(*geo)
        one, clip_one = _run_case(case, "philox", max_norm)
        two, clip_two = _run_case(case, "offset", max_norm)
    finally:
        K.set_launch_config(0, 0, 0)
    _assert_same(one, two, (case, geo))
    if case == "sgld_clipped":
        (whole,), (lo, hi) = clip_one, clip_two
        assert whole[1].item() == lo[1].item() == hi[1].item() == 1.0
        parts = float(np.hypot(lo[0].item(), hi[0].item()))
        # the sums of squares are carried in fp64; each of the three norms is
        # rounded to fp32 once (relative 2^-24 each): the two sides differ by
        # at most 2 x 2^-24, asserted at twice that
        assert abs(parts - whole[0].item()) <= 4 * 2.0 ** -24 * whole[0].item()


# -------------------------------------------- split == fused, and geometries
def _buffer_pair(family, geo, fused):
    """One later-step SGLD (momentum) / SGHMC update on buffer noise: fused, or
    as *_GRAD followed by the grad-ready step.  Returns the written vectors."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    spec = {"sgld": CASES["sgld_momentum"][1], "sghmc": CASES["sghmc"][0]}[family]
    t = Table()
    st = t.state()
    K.set_launch_config(*geo)
    if fused:
        _launch(st, spec, L.NOISE_BUFFER, STEP)
    else:
        _launch(st, ("step", spec[1] + "_GRAD", {k: v for k, v in spec[2].items()
                                                 if k not in ("mu", "momentum")}),
                L.NOISE_BUFFER, STEP)
        _launch(st, ("step", spec[1], dict(spec[2], grad_ready=True)), L.NOISE_BUFFER, STEP)
    torch.cuda.synchronize()
    assert int(t.nonfinite.item()) == 0
    return t.written()


@pytest.mark.parametrize("geo", DEPTHS[:3], ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("family", ["sgld", "sghmc"])
def test_grad_then_grad_ready_equals_the_fused_step(family, geo):
    """SGLD_GRAD + SGLD(grad_ready) and SGHMC_GRAD + SGHMC(grad_ready) round
    the same operations in the same order as the fused step (update_core)."""
    from bayesdll_amd import kernels as K
    try:
        fused = _buffer_pair(family, geo, True)
        split = _buffer_pair(family, geo, False)
    finally:
        K.set_launch_config(0, 0, 0)
    for nm in ("theta", "mom"):  # (the split leaves the sampler gradient in grad)
        assert torch.equal(fused[nm], split[nm]), (family, geo, nm)
        assert not torch.equal(fused[nm].cpu(), Table._init[nm])
    assert not torch.equal(split["grad"], fused["grad"])


@pytest.mark.parametrize("case", ["sgld_buffer", "sghmc_buffer", "sgld_clipped_buffer",
                                  "sgld_grad_then_ready"])
def test_plain_buffer_steps_do_not_depend_on_launch_geometry(case):
    """The plain (COLLECT_NONE) buffer-noise SGLD / SGHMC steps, the clipped
    step with clipping active and the SGLD_GRAD -> grad-ready pair: at depth 2
    and 4 they run on the re-read argument view (the clipped body re-reads
    clip[1] per iteration); every geometry gives the depth-1 bits."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    outs = []
    try:
        for geo in GEOMETRIES:
            if case == "sgld_grad_then_ready":
                outs.append((_buffer_pair("sgld", geo, False), None))
                continue
            spec = {"sgld_buffer": CASES["sgld_momentum"][1], "sghmc_buffer": CASES["sghmc"][0],
                    "sgld_clipped_buffer": CASES["sgld_clipped"][0]}[case]
            t = Table()
            K.set_launch_config(*geo)
            ws = _launch(t.state(), spec, L.NOISE_BUFFER, STEP)
            torch.cuda.synchronize()
            outs.append((t.written(), None if ws is None else ws[:2].clone()))
    finally:
        K.set_launch_config(0, 0, 0)
    assert GEOMETRIES[0][1] == 1
    base, clip0 = outs[0]
    assert not torch.equal(base["theta"].cpu(), Table._init["theta"])
    if case == "sgld_clipped_buffer":
        assert clip0[1].item() < 1.0  # clipping active
    for geo, (o, clip) in zip(GEOMETRIES[1:], outs[1:]):
        _assert_same(base, o, (case, geo))
        if clip0 is not None:
            assert torch.equal(clip, clip0), (case, geo)
