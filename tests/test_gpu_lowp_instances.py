"""Every built instance of bdl_lowp_step at its own depth, bit for bit (int32 /
uint16 patterns, no tolerance) against the host reference — tests/lowp_ref.py
over tests/step_ref.py, with the device's own bdl_philox_normal stream where
the noise is Philox.

* the whole matrix of pick_lowp / lowp_collect (lowp_ref.INSTANCE_CASES x
  unroll 1 / 2 / 4; tests/test_lowp_host.py proves by name that the library
  holds exactly these kernels), each at a literal grid of 2 workgroups
  (several iterations per workgroup) and at blocks = 0, in both division
  modes, collects with and without mom2, flat bf16 gradient and per-tensor
  base table with tensors at all four 2-B phases of 8-B alignment;
* chains of three launches whose next gradient is formed from the shadow;
* adversarial values (bf16 ties of the updated theta and one fp32 ulp either
  side, +-0, subnormals, bf16 extremes of the gradient) in vector, element-wise
  and guarded groups; a NaN gradient; a finite theta that rounds to an
  infinite shadow;
* stacked keying on the seamless tables B and C of tests/stacked_tables.py.

Table D (lowp_ref.TableD, 13,530 elements) serves the first three: what it
reaches at these grids is proven on the CPU in tests/test_lowp_host.py.  Every
shadow buffer is followed by sentinel elements for the groups past the end of
the vector of the last, guarded iteration; they must stay untouched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lowp_ref as LR
import stacked_tables as ST
import step_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
D = LR.TableD
SEED, CHAIN, STEP = 0x9E3779B97F4A7C15, 3, 2 ** 32 + 9
SCAL = dict(lrs=(0.0125, 0.05), noise_scale=(0.0371, 0.0113), one_minus_alpha=0.9, prior_sig=0.7,
            sigma2=0.49, n_data=640.0, mu=0.85, collect_a=3.0, collect_b=4.0)
GUARD = 4 * 256 * 4 + 8          # elements one depth-4 iteration can reach past n
SENT16 = 0x40E0                  # bf16(7.0)
M2_GUARD = F(-123.25)
VECS = ("theta", "mom", "m1", "m2", "shadow")


def _id(c):
    return "-".join(str(x) for x in c)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bf(bits):
    return _t(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _start(n, seed):
    rng = np.random.default_rng(seed)
    h = {k: rng.standard_normal(n).astype(F) * s for k, s in
         (("theta", 0.5), ("mom", 0.05), ("prior", 0.3), ("m1", 0.4), ("m2", 0.2))}
    h["m2"] = np.abs(h["m2"])
    h["g16"] = LR.bf16_encode(rng.standard_normal(n).astype(F) * 0.8)
    h["shadow"] = LR.bf16_encode(np.full(n, 3.0, dtype=F))
    return h


def _philox(n, chain=CHAIN, step=STEP):
    from bayesdll_amd import kernels as K
    return K.philox_normal(n, SEED, chain, step, device=DEV).cpu().numpy()


@pytest.fixture(scope="module")
def rig():
    """Table D: host start values (never modified), element attributes, the
    flat run table, the device's Philox stream and a cache of references."""
    from bayesdll_amd.flat import build_runs
    return SimpleNamespace(h=_start(D.n, 11), attr=SR.element_attrs(D.numels, D.attrs),
                           runs=build_runs(D.offsets, D.numels, D.attrs, D.n).to(DEV),
                           eps=_philox(D.n), refs={})


def _set_grad(st, g16):
    """Write the bf16 gradient where the launch reads it: the flat vector, or
    every tensor's own slot of the arena (tensor t at 2-B phase D.PHASES[t])."""
    if st.gbase is None:
        st.grad = _bf(g16)
        return
    arena = np.zeros(st.arena_len, dtype=np.uint16)
    for o, k, s in zip(D.offsets, D.numels, st.slots):
        arena[s:s + k] = g16[o:o + k]
    st.arena.copy_(_bf(arena))


def _state(rig, h, *, tensors, noise=None, m2=True):
    """A launchable bf16 state over table D: fresh device copies of h."""
    dev = torch.device(DEV, torch.cuda.current_device())
    st = SimpleNamespace(n=D.n, device=dev, theta=_t(h["theta"]), mom=_t(h["mom"]),
                         prior=_t(h["prior"]), noise=None if noise is None else _t(noise),
                         grad=None, gbase=None, timer=None, runs=rig.runs,
                         nonfinite=torch.zeros(1, dtype=torch.int32, device=DEV),
                         m1=_t(h["m1"]),
                         m2=_t(h["m2"] if m2 else np.full(D.n, M2_GUARD, dtype=F)), has_m2=m2)
    st.nruns = int(st.runs.shape[0])
    st.shadow_buf = _bf(np.concatenate([h["shadow"], np.full(GUARD, SENT16, dtype=np.uint16)]))
    st.shadow = st.shadow_buf[:D.n]
    if tensors:
        # one run per tensor; tensor t's gradient starts `shift` elements into an
        # 8-B aligned slot, so that grad_base[t] mod 8 is D.PHASES[t]
        st.slots, pos = [], 0
        for o, k, p in zip(D.offsets, D.numels, D.PHASES):
            st.slots.append(pos + (o + p // 2) % 4)
            pos += (k + 3 + 3) // 4 * 4
        st.arena_len = pos
        st.arena = torch.zeros(pos, dtype=torch.bfloat16, device=DEV)
        assert st.arena.data_ptr() % 8 == 0
        bases = [0 if a & SR.ATTR_SKIP else st.arena.data_ptr() + 2 * s - 2 * o
                 for o, s, a in zip(D.offsets, st.slots, D.attrs)]
        assert [b % 8 for b in bases] == D.PHASES
        st.runs = torch.tensor([(o + k, a) for o, k, a in zip(D.offsets, D.numels, D.attrs)],
                               dtype=torch.int64, device=DEV)
        st.nruns = len(D.offsets)
        st.gbase = torch.tensor(bases, dtype=torch.int64, device=DEV)
    _set_grad(st, h["g16"])
    return st


def _kw(case, st, *, step=STEP, chain=CHAIN, div_mode="recip", **extra):
    from bayesdll_amd import _lib as L
    method, noise, collect, momentum = case
    kw = dict(SCAL, noise_mode={"none": L.NOISE_NONE, "philox": L.NOISE_PHILOX,
                                "buffer": L.NOISE_BUFFER}[noise],
              collect=getattr(L, "COLLECT_" + collect), seed=SEED, chain=chain, step=step,
              div_mode=div_mode, momentum=momentum is not None, first_step=momentum == "first")
    if collect != "NONE":
        kw.update(mom1=st.m1, mom2=st.m2 if st.has_m2 else None)
    kw.update(extra)
    return getattr(L, method.upper()), kw


def _launch(case, st, *, blocks, unroll, **opt):
    from bayesdll_amd import kernels as K
    method, kw = _kw(case, st, **opt)
    K.lowp_step(st, method, blocks=blocks, unroll=unroll, **kw)
    torch.cuda.synchronize()


def _got(st):
    out = {k: getattr(st, k).cpu().numpy().view(np.int32) for k in ("theta", "mom", "m1", "m2")}
    buf = _u16(st.shadow_buf)
    out["shadow"], out["guard"] = buf[:st.n], buf[st.n:]
    out["nonfinite"] = int(st.nonfinite.item())
    return out


def _reference(case, h, attr, eps, mode, m2=True, sc=None):
    """The host step on h: every vector the launch may write, as bit patterns
    (a vector it does not write keeps its start values)."""
    method, noise, collect, momentum = case
    nth, nv, n1, n2, sh = LR.step(method, h["theta"], h["g16"], h["mom"], h["prior"], attr,
                                  sc or SR.Scalars(**SCAL), None if noise == "none" else eps, mode,
                                  momentum=momentum, collect=getattr(SR, collect), m1=h["m1"],
                                  m2=h["m2"] if m2 else None, shadow=h["shadow"])
    nv = h["mom"] if nv is None else nv
    n2 = n2 if m2 else np.full(nth.size, M2_GUARD, dtype=F)
    return {"theta": nth.view(np.int32), "mom": np.asarray(nv, dtype=F).view(np.int32),
            "m1": np.asarray(n1, dtype=F).view(np.int32),
            "m2": np.asarray(n2, dtype=F).view(np.int32), "shadow": sh}


def _check(got, want, ctx, nonfinite=0):
    for k in VECS:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (ctx, k, int(bad.size), bad[:8].tolist())
    assert (got["guard"] == SENT16).all(), (ctx, "shadow written past n")
    assert got["nonfinite"] == nonfinite, ctx


# ------------------------------------------------- every instance, every depth
@pytest.mark.parametrize("unroll", LR.UNROLLS)
@pytest.mark.parametrize("case", LR.INSTANCE_CASES, ids=_id)
def test_every_instance_at_every_depth_equals_the_host_reference(rig, case, unroll):
    h, frozen = rig.h, (rig.attr & SR.ATTR_SKIP) != 0
    collects = case[2] != "NONE"
    for mode in ("recip", "true"):
        for m2 in ((True, False) if collects else (True,)):
            key = (case, mode, m2)
            if key not in rig.refs:
                rig.refs[key] = _reference(case, h, rig.attr, rig.eps, mode, m2)
            want = rig.refs[key]
            # skipped elements: theta and shadow as they were; momentum too (a
            # first SGD-momentum step leaves +0: no buffer yet)
            assert np.array_equal(want["theta"][frozen], h["theta"].view(np.int32)[frozen])
            assert np.array_equal(want["shadow"][frozen], h["shadow"][frozen])
            assert (want["mom"][frozen] == 0).all() if case[3] == "first" else \
                np.array_equal(want["mom"][frozen], h["mom"].view(np.int32)[frozen])
            assert not np.array_equal(want["theta"][~frozen], h["theta"].view(np.int32)[~frozen])
            if not m2:  # the guard-filled m2 buffer is expected untouched
                assert (want["m2"].view(F) == M2_GUARD).all()
            for tensors in (False, True):
                for blocks in (D.BLOCKS, 0):
                    st = _state(rig, h, tensors=tensors, m2=m2,
                                noise=rig.eps if case[1] == "buffer" else None)
                    _launch(case, st, blocks=blocks, unroll=unroll, div_mode=mode)
                    _check(_got(st), want, (case, unroll, mode, m2, tensors, blocks))


# ------------------------------------------------------- chains of three steps
CHAINS = {
    "csghmc": [("csghmc", "none", "NONE", None), ("csghmc", "philox", "WELFORD_INIT", None),
               ("csghmc", "philox", "WELFORD", None)],
    "sgld": [("sgld", "philox", "NONE", "first"), ("sgld", "philox", "MEAN_INIT", "later"),
             ("sgld", "philox", "MEAN", "later")],
    "sghmc": [("sghmc", "philox", "NONE", None), ("sghmc", "philox", "MEAN_INIT", None),
              ("sghmc", "philox", "MEAN", None)],
}
COLLECT_A = [1.0, 1.0, 2.0]  # the collect scalars of steps 0, 1, 2 (count of samples so far)


def _next_grad(shadow16):
    """The gradient of step t + 1 from the shadow of step t."""
    with np.errstate(all="ignore"):
        p = LR.bf16_decode(shadow16) * F(-0.75)
        return LR.bf16_encode(p + F(0.0625))


@pytest.mark.parametrize("unroll,tensors", [(4, True), (4, False), (1, True)],
                         ids=["depth4-bases", "depth4-flat", "depth1-bases"])
@pytest.mark.parametrize("family", list(CHAINS))
def test_three_steps_with_the_gradient_formed_from_the_shadow(rig, family, unroll, tensors):
    h = dict(rig.h)
    st = _state(rig, h, tensors=tensors)
    for t, case in enumerate(CHAINS[family]):
        scal = dict(SCAL, collect_a=COLLECT_A[t], collect_b=COLLECT_A[t] + 1.0)
        eps = _philox(D.n, step=STEP + t)
        _launch(case, st, blocks=D.BLOCKS, unroll=unroll, step=STEP + t,
                collect_a=scal["collect_a"], collect_b=scal["collect_b"])
        want = _reference(case, h, rig.attr, eps, "recip", sc=SR.Scalars(**scal))
        got = _got(st)
        _check(got, want, (family, t, unroll, tensors))
        # both sides go on from their own state; the gradient comes from the shadow
        h = {k: want[k].view(F) for k in ("theta", "mom", "m1", "m2")}
        h.update(prior=rig.h["prior"], shadow=want["shadow"], g16=_next_grad(want["shadow"]))
        _set_grad(st, _next_grad(got["shadow"]))
    assert not np.array_equal(h["g16"], rig.h["g16"])


# ----------------------------------------------------------- adversarial values
ADVERSARIAL = [("csghmc", "philox", "WELFORD", None), ("csghmc", "none", "NONE", None),
               ("sgld", "philox", "MEAN", "later"), ("sgld", "buffer", "MEAN_INIT", "first"),
               ("sghmc", "philox", "MEAN", None)]
SITES = [D.SITE_VEC, D.SITE_ELEM, D.SITE_ELEM_BASES, D.SITE_GUARDED_VEC, D.SITE_GUARDED_ELEM]
# the updated theta's fp32 bits: a bf16 tie whose even neighbour lies below
# (0x3F80) and above (0x3F81 -> 0x3F82), and one fp32 ulp either side of each
TIES = [(hi << 16) | lo for hi in (0x3F80, 0x3F81) for lo in (0x8000, 0x7FFF, 0x8001)]
# (theta bits, gradient bf16 bits): +-0, fp32 subnormals; the gradient at the
# bf16 maximum, a bf16 subnormal and -0
FIXED = [(0x00000000, 0x8000), (0x80000000, 0x0000), (0x00000001, 0x0001), (0x807FFFFF, 0x8001),
         (0x00400000, 0x8000), (None, 0x7F7F), (None, 0xFF7F), (None, 0x0001), (None, 0x8000)]


def _theta_for(case, mode, h, attr, eps, idx, lo_bits, hi_bits):
    """Choose theta (and, where no theta will do, a neighbouring bf16 gradient)
    of element idx in h so that the updated theta, by the reference, has fp32
    bits in [lo_bits, hi_bits]: a search over the reference, 256 fp32
    neighbours either side of a fixed point."""
    def nth_of(cands):
        hh = {k: np.repeat(h[k][idx:idx + 1], cands.size) for k in h}
        hh["theta"] = cands
        r = _reference(case, hh, np.repeat(attr[idx:idx + 1], cands.size),
                       np.repeat(eps[idx:idx + 1], cands.size), mode)
        return r["theta"].view(np.uint32)

    target = np.array([(lo_bits + hi_bits) // 2], dtype=np.uint32).view(F)
    g0 = int(h["g16"][idx])
    for dg in range(16):  # rounding can make the update skip a value: try the next gradient
        h["g16"][idx] = g0 + dg
        guess = target * F(0.9)  # from below: the update is finite there for every target
        for _ in range(8):  # the update's slope in theta is close to 1: a fixed-point iteration
            step = target.astype(np.float64) - nth_of(guess).view(F).astype(np.float64)
            guess = (guess.astype(np.float64) + step).astype(F)
        cands = (guess.view(np.uint32)[0].astype(np.int64) + np.arange(-256, 257)).astype(np.uint32)
        out = nth_of(cands.view(F))
        hit = np.flatnonzero((out >= lo_bits) & (out <= hi_bits))
        if hit.size:
            h["theta"][idx] = cands.view(F)[hit[0]]
            return
    raise AssertionError((case, idx, hex(lo_bits)))


def _adversarial_h(rig, case, mode, rot):
    """rig.h with the adversarial values on every site, value (i + rot) on the
    site's i-th element."""
    h = {k: v.copy() for k, v in rig.h.items()}
    n = len(TIES) + len(FIXED)
    for site in SITES:
        for i, idx in enumerate(site):
            j = (i + rot) % n
            if j < len(TIES):
                _theta_for(case, mode, h, rig.attr, rig.eps, idx, TIES[j], TIES[j])
            else:
                tb, gb = FIXED[j - len(TIES)]
                if case[0] == "sghmc" and gb & 0x7FFF == 0x7F7F:
                    # SGHMC steps along g + v' = (1 + lr) g + ...: past FLT_MAX at the bf16
                    # maximum (the flag's case, below); 0x7F70 is 3.19e38, the update finite
                    gb = (gb & 0x8000) | 0x7F70
                if tb is not None:
                    h["theta"][idx] = np.array([tb], dtype=np.uint32).view(F)[0]
                h["g16"][idx] = gb
    return h


@pytest.mark.parametrize("case", ADVERSARIAL, ids=_id)
def test_adversarial_values_in_vector_elementwise_and_guarded_groups(rig, case):
    n = len(TIES) + len(FIXED)
    seen = set()
    for rot in range(0, n, 3):  # the shortest site holds 3 elements: every value visits every site
        for mode in ("recip", "true"):
            h = _adversarial_h(rig, case, mode, rot)
            want = _reference(case, h, rig.attr, rig.eps, mode)
            assert np.isfinite(want["theta"].view(F)).all()
            for site in SITES:
                seen |= {int(x) for x in want["theta"].view(np.uint32)[site]} & set(TIES)
            for unroll, tensors in ((4, True), (4, False), (1, True)):
                st = _state(rig, h, tensors=tensors,
                            noise=rig.eps if case[1] == "buffer" else None)
                _launch(case, st, blocks=D.BLOCKS, unroll=unroll, div_mode=mode)
                _check(_got(st), want, (case, rot, mode, unroll, tensors))
    assert seen == set(TIES)  # the search did construct every tie and its neighbours


def _fp32_kernel(rig, case, h, mode="recip"):
    """bdl_sgmcmc_step on the upcast gradient: what the contract names."""
    from bayesdll_amd import kernels as K
    st = SimpleNamespace(n=D.n, device=torch.device(DEV, torch.cuda.current_device()),
                         theta=_t(h["theta"]), mom=_t(h["mom"]), prior=_t(h["prior"]), noise=None,
                         grad=_t(LR.bf16_decode(h["g16"])), gbase=None, timer=None, runs=rig.runs,
                         nruns=int(rig.runs.shape[0]), m1=_t(h["m1"]), m2=_t(h["m2"]), has_m2=True,
                         nonfinite=torch.zeros(1, dtype=torch.int32, device=DEV))
    method, kw = _kw(case, st, div_mode=mode)
    K.sgmcmc_step(st, method, **kw)
    torch.cuda.synchronize()
    out = {k: getattr(st, k).cpu().numpy().view(np.int32) for k in ("theta", "mom", "m1", "m2")}
    out["nonfinite"] = int(st.nonfinite.item())
    return out


@pytest.mark.parametrize("case", [("csghmc", "philox", "WELFORD", None),
                                  ("sgld", "philox", "MEAN", "later")], ids=_id)
def test_a_nan_gradient_sets_the_flag_and_gives_a_nan_shadow(rig, case):
    h = {k: v.copy() for k, v in rig.h.items()}
    where = [s[1] for s in SITES]
    h["g16"][where] = 0x7FC0
    fp32 = _fp32_kernel(rig, case, h)
    assert fp32["nonfinite"] == 1
    want = _reference(case, h, rig.attr, rig.eps, "recip")
    clean = np.ones(D.n, dtype=bool)
    clean[where] = False
    for unroll, tensors in ((4, True), (1, False)):
        st = _state(rig, h, tensors=tensors)
        _launch(case, st, blocks=D.BLOCKS, unroll=unroll)
        got = _got(st)
        assert got["nonfinite"] == 1
        for k in ("theta", "mom", "m1", "m2"):  # NaNs included: the fp32 kernel's bits
            assert np.array_equal(got[k], fp32[k]), (k, unroll)
        assert np.isnan(got["theta"].view(F)[where]).all()
        assert LR.bf16_is_nan(got["shadow"][where]).all()
        assert np.array_equal(got["shadow"][clean], want["shadow"][clean])
        assert (got["guard"] == SENT16).all()


def test_a_finite_theta_above_the_bf16_maximum_gives_an_infinite_shadow_and_no_flag(rig):
    """The limit include/bdl_lowp.h states: the flag is bdl_sgmcmc_step's and
    looks at the fp32 theta only, so a finite master weight above the largest
    finite bf16 (0x7F7F0000) rounds to an infinite network weight without
    raising it."""
    case = ("csghmc", "none", "NONE", None)
    h = {k: v.copy() for k, v in rig.h.items()}
    where = [s[2] for s in SITES]
    for idx in where:
        h["g16"][idx] = LR.bf16_encode(np.array([-3.2e38], dtype=F))[0]
        _theta_for(case, "recip", h, rig.attr, rig.eps, idx, 0x7F7F8000, 0x7F7FFFFF)
    want = _reference(case, h, rig.attr, rig.eps, "recip")
    assert np.isfinite(want["theta"].view(F)).all()
    assert (want["theta"].view(F)[where] > LR.bf16_decode(np.array([0x7F7F], np.uint16))[0]).all()
    assert (want["shadow"][where] == 0x7F80).all()  # the reference's +inf
    fp32 = _fp32_kernel(rig, case, h)
    assert fp32["nonfinite"] == 0
    for unroll, tensors in ((4, True), (1, False)):
        st = _state(rig, h, tensors=tensors)
        _launch(case, st, blocks=D.BLOCKS, unroll=unroll)
        _check(_got(st), want, (unroll, tensors), nonfinite=fp32["nonfinite"])


# ------------------------------------------- stacked keying on seamless tables
STACKED = [("csghmc", "philox", "WELFORD", None), ("sgld", "philox", "MEAN", "later"),
           ("sghmc", "philox", "NONE", None)]


def _stacked(lay, h, lo=0, hi=None):
    """A bf16 state over elements [lo, hi) of the stacked layout."""
    hi = lay.n if hi is None else hi
    st = SimpleNamespace(n=hi - lo, device=torch.device(DEV, torch.cuda.current_device()),
                         noise=None, grad=_bf(h["g16"][lo:hi]), gbase=None, timer=None,
                         chain_groups=lay.chain_groups, has_m2=True,
                         nonfinite=torch.zeros(1, dtype=torch.int32, device=DEV),
                         **{k: _t(h[k][lo:hi]) for k in ("theta", "mom", "prior", "m1", "m2")})
    st.runs = lay.flat_runs(lo, hi).to(DEV)
    st.nruns = int(st.runs.shape[0])
    st.shadow_buf = _bf(np.concatenate([h["shadow"][lo:hi],
                                        np.full(GUARD, SENT16, dtype=np.uint16)]))
    st.shadow = st.shadow_buf[:st.n]
    return st


@pytest.fixture(scope="module", params=["b", "c"])
def stack(request):
    """Table B or C: start values that differ from chain to chain and the
    host reference of every case, chain k on the stream of (seed, chain + k,
    step) — computed once."""
    lay = {"b": ST.table_b, "c": ST.table_c}[request.param]()
    assert lay.stride == lay.n1  # seamless: no padding
    h = _start(lay.n, 23)
    attr = np.tile(lay.slot_attr(), lay.K)
    eps = np.concatenate([_philox(lay.stride, chain=CHAIN + k) for k in range(lay.K)])
    want = {c: _reference(c, h, attr, eps, "recip") for c in STACKED}
    return SimpleNamespace(lay=lay, h=h, want=want, name=request.param)


@pytest.mark.parametrize("unroll", LR.UNROLLS)
@pytest.mark.parametrize("case", STACKED, ids=_id)
def test_stacked_chains_on_seamless_tables_are_keyed_chain_plus_k(stack, case, unroll):
    st = _stacked(stack.lay, stack.h)
    _launch(case, st, blocks=LR.STACKED_BLOCKS, unroll=unroll)
    got, want, lay = _got(st), stack.want[case], stack.lay
    for k in range(lay.K):  # chain k's slot against its own stream
        sl = slice(k * lay.stride, (k + 1) * lay.stride)
        for name in VECS:
            assert np.array_equal(got[name][sl], want[name][sl]), (stack.name, k, name)
    _check(got, want, (stack.name, case, unroll))


def test_a_stacked_launch_split_by_philox_offset_equals_one(stack):
    """Two launches over [0, split) and [split, n), the second with
    philox_offset = split / 4: on table C the split lies inside chain 1 (its
    head tensor), on table B on the seam of chain 2."""
    case, lay = STACKED[0], stack.lay
    split = {"b": 2 * lay.stride, "c": lay.stride + 2000}[stack.name]
    assert split % 4 == 0
    parts = []
    for lo, hi in ((0, split), (split, lay.n)):
        st = _stacked(lay, stack.h, lo, hi)
        _launch(case, st, blocks=LR.STACKED_BLOCKS, unroll=4, philox_offset=lo // 4)
        parts.append(_got(st))
        assert (parts[-1]["guard"] == SENT16).all() and parts[-1]["nonfinite"] == 0
    for name in VECS:
        assert np.array_equal(np.concatenate([p[name] for p in parts]), stack.want[case][name]), name
