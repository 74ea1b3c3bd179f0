"""bdl_lowp_step / bdl_lowp_shadow on the device, bit for bit (no tolerance):
against the production fp32 kernel on the upcast gradient, against the host
reference (tests/lowp_ref.py over tests/step_ref.py) on the device's own Philox
stream, across launch geometries, flat gradient against the per-run base
table, split launches, stacked keying with sentinels in the padding, SKIP
elements, the shadow rounding and the divergence flag.

One table serves this file: test_gpu_noise_units.py's 39,426 elements
(n % 4 = 2; one run boundary that is no multiple of 4, at 16,295, so one
float4 group spans two runs; a head run; uninformative biases; a frozen tensor
in the middle).  In base-table mode every tensor's gradient is a bf16 tensor
of its own, the first one placed one bf16 element off 8-B alignment (that
tensor alone is read element by element).  With blocks = 2 every workgroup
runs 5 to 20 iterations; with the default grid every workgroup runs one.

What this file does NOT reach — most instances at their own depth, launches
without mom2, an iteration that holds a boundary group, a SKIP run and an
unaligned base together — tests/test_gpu_lowp_instances.py covers on a table
built for it, and tests/test_lowp_host.py proves on the CPU (lowp_ref.classify)
which groups of which iterations take which path on both tables."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lowp_ref as LR
import step_ref as SR
from test_gpu_noise_units import FROZEN, SEGMENTS

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SEED, CHAIN, STEP = 0x9E3779B97F4A7C15, 3, 2 ** 32 + 9
SENTINEL = 7.0

NAMES = [nm for nm, _ in SEGMENTS]
NUMELS = [int(k) for _, k in SEGMENTS]
OFFSETS = np.concatenate([[0], np.cumsum(NUMELS)[:-1]]).astype(int).tolist()
N = int(sum(NUMELS))

SCAL = dict(lrs=(0.0125, 0.05), noise_scale=(0.0371, 0.0113), one_minus_alpha=0.9, prior_sig=0.7,
            sigma2=0.49, n_data=640.0, mu=0.85, collect_a=3.0, collect_b=4.0)

# (method, noise, collect, momentum): what the header lists as in scope
CASES = [("csghmc", nz, c, None) for nz in ("none", "philox", "buffer")
         for c in ("NONE", "WELFORD_INIT", "WELFORD")]
CASES += [("sgld", nz, c, m) for nz in ("philox", "buffer")
          for c in ("NONE", "MEAN_INIT", "MEAN") for m in (None, "first", "later")]
CASES += [("sghmc", "philox", "NONE", None), ("sghmc", "buffer", "MEAN", None)]


def _attrs():
    from bayesdll_amd.flat import segment_attrs
    return segment_attrs(NAMES, "head", "uninformative", [nm != FROZEN for nm in NAMES])


@pytest.fixture(scope="module")
def data():
    """Host start values (never modified), the element attributes, the flat run
    table and the device's Philox stream of (SEED, CHAIN, STEP)."""
    from bayesdll_amd import kernels as K
    from bayesdll_amd.flat import build_runs
    rng = np.random.default_rng(11)
    h = {k: rng.standard_normal(N).astype(F) * s for k, s in
         (("theta", 0.5), ("mom", 0.05), ("prior", 0.3), ("m1", 0.4), ("m2", 0.2))}
    h["m2"] = np.abs(h["m2"])
    h["g16"] = LR.bf16_encode(rng.standard_normal(N).astype(F) * 0.8)
    h["shadow"] = LR.bf16_encode(np.full(N, 3.0, dtype=F))
    attrs = _attrs()
    return SimpleNamespace(h=h, attrs=attrs, attr=SR.element_attrs(NUMELS, attrs),
                           runs=build_runs(OFFSETS, NUMELS, attrs, N).to(DEV),
                           eps=K.philox_normal(N, SEED, CHAIN, STEP, device=DEV).cpu().numpy())


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bf(bits):
    return _t(bits.view(np.int16)).view(torch.bfloat16)


def _state(d, *, lowp, tensors=False, lo=0, hi=N, eps=None):
    """A launchable state over elements [lo, hi) (4-aligned lo): fresh device
    copies of the start values."""
    from bayesdll_amd.flat import build_runs
    h = d.h
    st = SimpleNamespace(n=hi - lo, device=torch.device(DEV, torch.cuda.current_device()),
                         theta=_t(h["theta"][lo:hi]), mom=_t(h["mom"][lo:hi]),
                         prior=_t(h["prior"][lo:hi]), noise=None, gbase=None, timer=None,
                         nonfinite=torch.zeros(1, dtype=torch.int32, device=DEV),
                         m1=_t(h["m1"][lo:hi]), m2=_t(h["m2"][lo:hi]))
    if eps is not None:
        st.noise = _t(eps[lo:hi])
    if (lo, hi) == (0, N):
        st.runs = d.runs
    else:
        segs = [(o - lo, k, a) for o, k, a in zip(OFFSETS, NUMELS, d.attrs) if lo <= o < hi]
        st.runs = build_runs([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs],
                             hi - lo).to(DEV)
    st.nruns = int(st.runs.shape[0])
    if not lowp:
        st.grad = _t(LR.bf16_decode(h["g16"][lo:hi]))
        return st
    st.shadow = _bf(h["shadow"][lo:hi])
    if not tensors:
        st.grad = _bf(h["g16"][lo:hi])
        return st
    # one bf16 gradient tensor (and one run) per parameter tensor; the first
    # one starts one element past an 8-B boundary
    assert (lo, hi) == (0, N)
    st.grad, st.gtensors, rows, bases = None, [], [], []
    for i, (o, k, a) in enumerate(zip(OFFSETS, NUMELS, d.attrs)):
        frozen = bool(a & SR.ATTR_SKIP)
        buf = torch.zeros(k + 8, dtype=torch.bfloat16, device=DEV)
        g = buf[1:1 + k] if i == 0 else buf[:k]
        g.copy_(_bf(h["g16"][o:o + k]))
        st.gtensors.append(buf)
        rows.append((o + k, a))
        bases.append(0 if frozen else g.data_ptr() - 2 * o)
    assert (st.gtensors[0].data_ptr() + 2) % 8 == 2
    st.runs = torch.tensor(rows, dtype=torch.int64, device=DEV)
    st.nruns = len(rows)
    st.gbase = torch.tensor(bases, dtype=torch.int64, device=DEV)
    return st


def _kw(case, st, step=STEP, chain=CHAIN, div_mode="recip", **extra):
    from bayesdll_amd import _lib as L
    method, noise, collect, momentum = case
    kw = dict(SCAL, noise_mode={"none": L.NOISE_NONE, "philox": L.NOISE_PHILOX,
                                "buffer": L.NOISE_BUFFER}[noise],
              collect=getattr(L, "COLLECT_" + collect), seed=SEED, chain=chain, step=step,
              div_mode=div_mode, momentum=momentum is not None, first_step=momentum == "first")
    if collect != "NONE":
        kw.update(mom1=st.m1, mom2=st.m2)
    kw.update(extra)
    return getattr(L, method.upper()), kw


def _run(d, case, *, lowp, **opt):
    from bayesdll_amd import kernels as K
    geo = {k: opt.pop(k) for k in ("blocks", "unroll") if k in opt}
    kwx = {k: opt.pop(k) for k in ("div_mode",) if k in opt}
    st = _state(d, lowp=lowp, eps=d.eps if case[1] == "buffer" else None, **opt)
    method, kw = _kw(case, st, **kwx)
    if lowp:
        K.lowp_step(st, method, **geo, **kw)
    else:
        K.sgmcmc_step(st, method, **kw)
    torch.cuda.synchronize()
    return st


def _bits(st, names=("theta", "mom", "m1", "m2")):
    out = {k: getattr(st, k).cpu().numpy().view(np.int32) for k in names}
    if getattr(st, "shadow", None) is not None:
        out["shadow"] = st.shadow.view(torch.int16).cpu().numpy().view(np.uint16)
    out["nonfinite"] = int(st.nonfinite.item())
    return out


def _same(a, b, keys=None):
    for k in keys or a:
        if k in b:
            assert np.array_equal(a[k], b[k]), (k, int(np.sum(a[k] != b[k])))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_equals_the_production_kernel_and_the_host_reference(data, case):
    d = data
    got = _bits(_run(d, case, lowp=True, blocks=2, unroll=2))
    want = _bits(_run(d, case, lowp=False))
    _same(want, got, ("theta", "mom", "m1", "m2", "nonfinite"))
    assert got["nonfinite"] == 0
    # the per-run base table over separate bf16 tensors (one off 8-B alignment)
    _same(got, _bits(_run(d, case, lowp=True, blocks=2, unroll=2, tensors=True)))
    # the host reference, shadow included
    method, noise, collect, momentum = case
    h = d.h
    sc = SR.Scalars(**SCAL)
    nth, nv, n1, n2, sh = LR.step(method, h["theta"], h["g16"], h["mom"], h["prior"], d.attr, sc,
                                  None if noise == "none" else d.eps, "recip", momentum=momentum,
                                  collect=getattr(SR, collect), m1=h["m1"], m2=h["m2"],
                                  shadow=h["shadow"])
    assert np.array_equal(got["theta"], nth.view(np.int32))
    if nv is not None and (method != "sgld" or momentum is not None):
        assert np.array_equal(got["mom"], nv.view(np.int32))
    if collect != "NONE":
        assert np.array_equal(got["m1"], n1.view(np.int32))
        assert np.array_equal(got["m2"], n2.view(np.int32))
    assert np.array_equal(got["shadow"], sh)
    on_dev = torch.from_numpy(nth).to(DEV).to(torch.bfloat16).view(torch.int16).cpu().numpy()
    live = (d.attr & SR.ATTR_SKIP) == 0
    assert np.array_equal(got["shadow"][live], on_dev.view(np.uint16)[live])


@pytest.mark.parametrize("case", [("csghmc", "philox", "WELFORD", None),
                                  ("sgld", "philox", "MEAN", "later"),
                                  ("sghmc", "philox", "NONE", None)],
                         ids=lambda c: c[0])
def test_true_division_mode_equals_the_production_kernel(data, case):
    got = _bits(_run(data, case, lowp=True, blocks=2, unroll=1, div_mode="true"))
    want = _bits(_run(data, case, lowp=False, div_mode="true"))
    _same(want, got, ("theta", "mom", "m1", "m2", "nonfinite"))
    if case[0] == "sgld":
        # the flag reaches the kernel: SGLD adds the prior term to a noise term
        # of its own size, so the two roundings of the division show in theta
        # (SGHMC's prior term is absorbed by the far larger gradient here)
        rec = _bits(_run(data, case, lowp=True, blocks=2, unroll=1))
        assert not np.array_equal(rec["theta"], got["theta"])


@pytest.mark.parametrize("tensors", [False, True], ids=["flat", "bases"])
@pytest.mark.parametrize("case", [("csghmc", "philox", "WELFORD", None),
                                  ("sgld", "buffer", "MEAN_INIT", "first")], ids=lambda c: c[0])
def test_results_do_not_depend_on_the_geometry(data, case, tensors):
    ref = _bits(_run(data, case, lowp=True, blocks=1, unroll=1))
    for blocks in (1, 2, 7, 0):
        for unroll in (1, 2, 4):
            got = _bits(_run(data, case, lowp=True, blocks=blocks, unroll=unroll,
                             tensors=tensors))
            _same(ref, got)


def test_two_launches_split_by_philox_offset_equal_one(data):
    from bayesdll_amd import kernels as K
    case = ("csghmc", "philox", "WELFORD", None)
    one = _bits(_run(data, case, lowp=True, blocks=2, unroll=2))
    split = OFFSETS[NAMES.index("l7.weight")]  # a run boundary on a float4 group
    assert split % 4 == 0
    parts = []
    for lo, hi in ((0, split), (split, N)):
        st = _state(data, lowp=True, lo=lo, hi=hi)
        method, kw = _kw(case, st, philox_offset=lo // 4)
        K.lowp_step(st, method, blocks=2, unroll=2, **kw)
        torch.cuda.synchronize()
        parts.append(_bits(st))
    for k in ("theta", "mom", "m1", "m2", "shadow"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), one[k]), k


def test_stacked_chains_are_keyed_chain_plus_k_and_padding_is_intact(data):
    """Three chains side by side, slots padded to a multiple of 4 with a SKIP
    run, the padding pre-filled with a sentinel in every vector."""
    from bayesdll_amd import kernels as K
    from bayesdll_amd.flat import build_runs
    d, Kc = data, 3
    stride = (N + 3) // 4 * 4
    case = ("csghmc", "philox", "NONE", None)
    pad = np.zeros(stride, dtype=bool)
    pad[N:] = True

    def stack(x, fill):
        out = np.full(Kc * stride, fill, dtype=x.dtype)
        for k in range(Kc):
            out[k * stride:k * stride + N] = x
        return out

    sent16 = LR.bf16_encode(np.array([SENTINEL], dtype=F))[0]
    st = SimpleNamespace(n=Kc * stride, device=torch.device(DEV, torch.cuda.current_device()),
                         theta=_t(stack(d.h["theta"], F(SENTINEL))),
                         mom=_t(stack(d.h["mom"], F(SENTINEL))), prior=None, noise=None,
                         gbase=None, timer=None, chain_groups=stride // 4,
                         grad=_bf(stack(d.h["g16"], sent16)), shadow=_bf(stack(d.h["shadow"], sent16)),
                         nonfinite=torch.zeros(1, dtype=torch.int32, device=DEV))
    offs = [k * stride + o for k in range(Kc) for o in OFFSETS]
    st.runs = build_runs(offs, NUMELS * Kc, d.attrs * Kc, Kc * stride).to(DEV)
    st.nruns = int(st.runs.shape[0])
    method, kw = _kw(case, st)
    K.lowp_step(st, method, blocks=3, unroll=4, **kw)
    torch.cuda.synchronize()
    got = _bits(st, ("theta", "mom"))
    grad_after = st.grad.view(torch.int16).cpu().numpy().view(np.uint16)
    for k in range(Kc):
        one = _state(d, lowp=True)
        m1, kw1 = _kw(case, one, chain=CHAIN + k)
        K.lowp_step(one, m1, **kw1)
        torch.cuda.synchronize()
        w = _bits(one, ("theta", "mom"))
        sl = slice(k * stride, k * stride + N)
        for name in ("theta", "mom", "shadow"):
            assert np.array_equal(got[name][sl], w[name]), (k, name)
        p = slice(k * stride + N, (k + 1) * stride)
        assert (got["theta"][p].view(F) == SENTINEL).all() and (got["mom"][p].view(F) == SENTINEL).all()
        assert (got["shadow"][p] == sent16).all() and (grad_after[p] == sent16).all()
    assert got["nonfinite"] == 0


def test_skip_elements_keep_theta_momentum_and_shadow(data):
    d = data
    frozen = (d.attr & SR.ATTR_SKIP) != 0
    assert 0 < frozen.sum() < N
    for case in (("csghmc", "philox", "WELFORD", None), ("sgld", "philox", "MEAN", "later")):
        got = _bits(_run(d, case, lowp=True, blocks=2, unroll=4, tensors=True))
        assert np.array_equal(got["theta"][frozen], d.h["theta"].view(np.int32)[frozen])
        assert np.array_equal(got["mom"][frozen], d.h["mom"].view(np.int32)[frozen])
        assert np.array_equal(got["shadow"][frozen], d.h["shadow"][frozen])
        assert not np.array_equal(got["theta"][~frozen], d.h["theta"].view(np.int32)[~frozen])
        # the moments of a frozen element are the production kernel's: the
        # collect sees its unchanged theta
        want = _bits(_run(d, case, lowp=False))
        assert np.array_equal(got["m1"], want["m1"]) and np.array_equal(got["m2"], want["m2"])


def test_shadow_kernel_rounds_as_the_reference_and_as_torch():
    from bayesdll_amd import kernels as K
    x = LR.rounding_inputs()
    x = np.tile(x, 10_001 // x.size + 1)[:10_001]  # n % 4 = 1
    nans = np.array([0x7FC00000, 0xFFFFFFFF, 0x7F800001, 0xFF800100], dtype=np.uint32).view(F)
    x[100:104] = nans
    x[-1] = nans[1]
    theta = _t(x)
    shadow = torch.zeros(x.size, dtype=torch.bfloat16, device=DEV)
    K.lowp_shadow(theta, shadow)
    torch.cuda.synchronize()
    got = shadow.view(torch.int16).cpu().numpy().view(np.uint16)
    isnan = np.isnan(x)
    assert LR.bf16_is_nan(got[isnan]).all()
    assert np.array_equal(got[~isnan], LR.bf16_encode(x)[~isnan])
    on_dev = theta.to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got[~isnan], on_dev[~isnan])


def test_a_nonfinite_gradient_sets_the_flag(data):
    d = data
    case = ("csghmc", "none", "NONE", None)
    g16 = d.h["g16"].copy()
    g16[12345] = 0x7F80  # +inf in bf16
    d2 = SimpleNamespace(h=dict(d.h, g16=g16), attrs=d.attrs, attr=d.attr, runs=d.runs, eps=d.eps)
    got = _bits(_run(d2, case, lowp=True, blocks=2, unroll=2))
    want = _bits(_run(d2, case, lowp=False))
    assert got["nonfinite"] == 1 and want["nonfinite"] == 1
    _same(want, got, ("theta", "mom"))


def _stacked_state(d, Kc, *, lowp):
    """Kc chains side by side, every vector's padding pre-filled with the sentinel."""
    from bayesdll_amd.flat import build_runs
    stride = (N + 3) // 4 * 4
    sent16 = LR.bf16_encode(np.array([SENTINEL], dtype=F))[0]

    def stack(x, fill):
        out = np.full(Kc * stride, fill, dtype=x.dtype)
        for k in range(Kc):
            out[k * stride:k * stride + N] = x
        return out

    st = SimpleNamespace(n=Kc * stride, device=torch.device(DEV, torch.cuda.current_device()),
                         noise=None, gbase=None, timer=None, chain_groups=stride // 4,
                         nonfinite=torch.zeros(1, dtype=torch.int32, device=DEV),
                         **{k: _t(stack(d.h[k], F(SENTINEL)))
                            for k in ("theta", "mom", "prior", "m1", "m2")})
    if lowp:
        st.grad = _bf(stack(d.h["g16"], sent16))
        st.shadow = _bf(stack(d.h["shadow"], sent16))
    else:
        st.grad = _t(stack(LR.bf16_decode(d.h["g16"]), F(SENTINEL)))
    offs = [k * stride + o for k in range(Kc) for o in OFFSETS]
    st.runs = build_runs(offs, NUMELS * Kc, d.attrs * Kc, Kc * stride).to(DEV)
    st.nruns = int(st.runs.shape[0])
    pad = np.zeros(Kc * stride, dtype=bool)
    for k in range(Kc):
        pad[k * stride + N:(k + 1) * stride] = True
    return st, pad, sent16


@pytest.mark.parametrize("case", [("sgld", "philox", "MEAN_INIT", "first"),
                                  ("sgld", "philox", "MEAN", "later"),
                                  ("csghmc", "philox", "WELFORD_INIT", None)],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_padding_and_skip_elements_get_what_the_fp32_kernel_writes(data, case):
    """The limit the header states: theta, momentum and moments of SKIP elements
    — a stacked slot's padding included — receive the fp32 kernel's values (theta
    unchanged; a first SGD-momentum step stores 0 in the buffer; the collect
    sees the unchanged theta), so every fp32 vector equals bdl_sgmcmc_step's
    over the whole stacked buffer.  Gradient and shadow of the padding keep the
    sentinel."""
    from bayesdll_amd import kernels as K
    d = data
    low, pad, sent16 = _stacked_state(d, 2, lowp=True)
    ref, _, _ = _stacked_state(d, 2, lowp=False)
    for st, fn, geo in ((low, K.lowp_step, dict(blocks=3, unroll=2)), (ref, K.sgmcmc_step, {})):
        method, kw = _kw(case, st)
        fn(st, method, **geo, **kw)
    torch.cuda.synchronize()
    got, want = _bits(low), _bits(ref)
    _same(want, got, ("theta", "mom", "m1", "m2", "nonfinite"))
    assert (got["theta"][pad].view(F) == SENTINEL).all()
    assert (got["shadow"][pad] == sent16).all()
    grad_after = low.grad.view(torch.int16).cpu().numpy().view(np.uint16)
    assert (grad_after[pad] == sent16).all()
    if case[3] == "first":
        assert (got["mom"][pad] == 0).all()  # +0: no SGD buffer yet for a skipped element
    else:
        assert (got["mom"][pad].view(F) == SENTINEL).all()
