"""Every posterior-draw and moment-update kernel instance against the host
reference (tests/draw_ref.py), as int32 bit patterns over every element; NaN
is compared as "NaN where and only where the reference has NaN".  No
tolerance appears in this file.

Buffer noise comes from the host.  Philox instances are compared with the
reference fed the device's own bdl_philox_normal output for the same key —
the stream test_gpu_noise_stream.py pins to tests/philox_ref.py.

Sizes come from draw_ref.size_table at the device's CU count and at explicit
geometries of one workgroup per CU, the smallest that still send workgroups
through a second trip of the grid-stride loop; what the table reaches
(two full trips then a guarded tail, two trips and no tail, a `break` at slot
0, inside the unroll and not at all, n % 4 in {1, 2, 3}, n < 4, an exact
multiple of a whole-grid trip) is asserted by draw_ref.check_size_table here
for the device's count and in tests/test_draw_host.py for 256 and 304 CUs.
"""
import itertools

import numpy as np
import pytest
import torch

import draw_ref as DR
import step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SEED, CHAIN, STEP = 0x1234_5678_9ABC, 5, (7 << 32) | 11


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _same(got, want, what):
    """Bit equality over every element; NaN exactly where the reference has it."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == F and want.dtype == F and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", int((gn != wn).sum()))
    bad = (_bits(got) != _bits(want)) & ~wn
    assert not bad.any(), (what, int(bad.sum()), int(np.flatnonzero(bad)[0]))


def _differ(a, b):
    return bool(((_bits(a) != _bits(b)) & ~(np.isnan(a) & np.isnan(b))).any())


def _floor_hit(ratio, floor):
    """A second moment q with fl32(ratio) * q == fl32(floor) exactly."""
    r, fl = R.f32(ratio), R.f32(floor)
    q = F(fl / r)
    for _ in range(8):
        if r * q == fl:
            return q
        q = np.nextafter(q, F(np.inf) if r * q < fl else F(0))
    raise AssertionError("no second moment maps onto the floor")


# ---------------------------------------------------------------- shared data
_D = {}


def _data():
    """Host vectors of the largest size any test launches, their device
    copies, generated once.  m1 is exactly 0 on a quarter of the elements, so
    that every bit of sqrt(var) * eps reaches the output there; elsewhere it
    is of the order of the deviation, so that the sum rounds.  Variances span
    2^-110 .. 2^20 on half of the elements (the clamp, and sqrt below and
    above 2^-96) and are about 1e-4 on the rest."""
    if not _D:
        n = max(DR.size_table(_cus(), 1, 4))
        rng = np.random.default_rng(77)
        m1 = (0.02 * rng.standard_normal(n)).astype(F)
        m1[rng.random(n) < 0.25] = 0.0
        wide = rng.random(n) < 0.5
        v = np.where(wide, rng.random(n) * 2.0 ** rng.integers(-110, 21, n),
                     1e-4 * rng.uniform(0.5, 2.0, n)).astype(F)
        h = dict(m1=m1, v=v, eps=rng.standard_normal(n).astype(F),
                 x=rng.standard_normal(n).astype(F), a1=rng.standard_normal(n).astype(F),
                 a2=rng.random(n).astype(F))
        _D["h"] = h
        _D["d"] = {k: _dev(a) for k, a in h.items()}
        _D["z"] = {}
    return _D["h"], _D["d"]


def _philox(n, chain=CHAIN):
    """The device's stream for the key, host copy of the first n values."""
    from bayesdll_amd import kernels as K
    _data()
    key = (chain,)
    z = _D["z"].get(key)
    if z is None or len(z) < n:
        z = _D["z"][key] = K.philox_normal(max(n, max(DR.size_table(_cus(), 1, 4))), SEED, chain,
                                           STEP, device=DEV).cpu().numpy()
    return z[:n]


def _second_moment(var_mode, ratio, floor):
    """The second-moment vector of a variance form: every 7th variance is
    negative before the clamp, every 11th (from 5) lands on the floor exactly
    in the raw-moment form."""
    h, _ = _data()
    key = ("q", var_mode, ratio, floor)
    if key not in _D:
        m1, v = h["m1"], h["v"]
        with np.errstate(all="ignore"):
            if var_mode == DR.VAR_RAW_MOMENTS:
                q = m1 * m1 + v / R.f32(ratio)
                q[::7] = m1[::7] * m1[::7] - F(1e-3)
                hit = np.arange(5, len(q), 11)
                hit = hit[m1[hit] == 0]
                q[hit] = _floor_hit(ratio, floor)
            elif var_mode == DR.VAR_WELFORD:
                q = v * R.f32(ratio)
                q[::7] = -q[::7]
            else:
                q = v.copy()
                q[::7] = -q[::7]
        _D[key] = (q.astype(F), _dev(q.astype(F)))
    return _D[key]


# -------------------------------------------------------------------- the draw
@pytest.mark.parametrize("inst", DR.DRAW_INSTANCES, ids=DR.draw_id)
def test_every_draw_instance_matches_the_host_reference(inst):
    from bayesdll_amd import kernels as K
    var_mode, has_m2, recip, noise, floored, unroll = inst
    floor = 1e-12 if floored else 2.0 ** -97
    ratios = {DR.VAR_RAW_MOMENTS: (1.25,), DR.VAR_WELFORD: (3.0, 7.0), DR.VAR_GIVEN: (1.0,)}[var_mode]
    cus = _cus()
    sizes = DR.size_table(cus, 1, unroll)
    DR.check_size_table(sizes, cus, 1, unroll)
    h, d = _data()
    for ratio in ratios:
        q, qd = _second_moment(var_mode, ratio, floor) if has_m2 else (None, None)
        inv = float(DR.D.inv_of(ratio)) if recip else 0.0
        # the launch's own inputs select this very instance
        assert DR.sample_instance(var_mode, has_m2, inv != 0.0, noise, R.f32(floor) >= DR.FLOORED_MIN,
                                  unroll) == inst
        for n in sizes:
            eps = h["eps"][:n] if noise == DR.NOISE_BUFFER else _philox(n)
            out = torch.full((n,), float("nan"), device=DEV)
            kw = dict(noise=d["eps"][:n]) if noise == DR.NOISE_BUFFER else \
                dict(seed=SEED, chain=CHAIN, step=STEP)
            K.posterior_sample(out, d["m1"][:n], None if qd is None else qd[:n], var_mode=var_mode,
                               ratio=ratio, var_floor=floor, div_mode="recip" if recip else "true",
                               geometry=(1, unroll), **kw)
            ref = DR.draw(h["m1"][:n], None if q is None else q[:n], eps, var_mode=var_mode,
                          ratio=ratio, inv_ratio=inv, var_floor=floor)
            _same(out, ref, (DR.draw_id(inst), ratio, n))
        n = max(sizes)
        if has_m2:  # what the data holds, at the largest size
            m1 = h["m1"][:n]
            with np.errstate(all="ignore"):
                raw = DR.D.variance_f32(m1, q[:n], var_mode, R.f32(ratio), F(inv), F(-np.inf))
            assert int((raw < 0).sum()) >= n // 7 - n // 28  # the 7th elements, bar m1 == 0 luck
            if var_mode == DR.VAR_RAW_MOMENTS:
                assert int((raw == R.f32(floor)).sum()) >= n // 11 // 8
            if not floored:
                assert ((raw > 0) & (raw < DR.FLOORED_MIN)).sum() > n // 200
        if var_mode == DR.VAR_WELFORD and ratio == 7.0:
            other = DR.draw(h["m1"][:n], q[:n], eps, var_mode=var_mode, ratio=ratio,
                            inv_ratio=0.0 if recip else float(DR.D.inv_of(ratio)), var_floor=floor)
            assert _differ(ref, other)  # the other division mode would not pass
    # the inputs are read only
    nmax = max(sizes)
    assert torch.equal(d["m1"][:nmax].cpu(), torch.from_numpy(h["m1"][:nmax]))


# ------------------------------------------------------------ the moment update
def _launch_moments(x, m1, m2, kind, ca, cb, mode, inv=None):
    """bdl_moments_update through the C-ABI; inv: (inv_collect_a,
    inv_collect_b) as the caller fills them (None: the host's fl32(1 / s))."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    a = L.MomentsArgs()
    a.theta, a.mom1 = x.data_ptr(), m1.data_ptr()
    a.mom2 = None if m2 is None else m2.data_ptr()
    a.n, a.collect = x.numel(), int(kind)
    a.flags = L.FLAG_RECIP_DIV if mode == "recip" else 0
    a.collect_a, a.collect_b = float(ca), float(cb)
    a.inv_collect_a, a.inv_collect_b = (K._inv(ca), K._inv(cb)) if inv is None else inv
    L.check(L.lib().bdl_moments_update(a, L.current_stream_handle(x.device)), "bdl_moments_update")


def _moments_case(inst, n, ca, cb, fallback=False):
    kind, recip, has_m2 = inst
    h, d = _data()
    mode = "recip" if recip else "true"
    init = kind in (DR.WELFORD_INIT, DR.MEAN_INIT)
    x = h["x"][:n]
    if init:  # the INIT kinds must not read the moments
        m1h = m2h = np.full(n, np.nan, F)
    else:
        m1h, m2h = h["a1"][:n], h["a2"][:n]
    m1, m2 = _dev(m1h), _dev(m2h)  # m2: the sentinel when no second moment is passed
    _launch_moments(d["x"][:n], m1, m2 if has_m2 else None, kind, ca, cb, mode,
                    inv=(0.0, 0.0) if fallback else None)
    div = R.Div.fallback if fallback else R.Div
    e1, e2 = DR.moments(kind, x, m1h, m2h if has_m2 else None, div(ca), div(cb), mode)
    what = (DR.moments_id(inst), n, "fallback" if fallback else "")
    _same(m1, e1, what + ("mom1",))
    if has_m2:
        _same(m2, e2, what + ("mom2",))
    else:
        assert e2 is None
        _same(m2, m2h, what + ("mom2 is not written",))
    _same(d["x"][:n], x, what + ("theta is not written",))
    return e1, e2


@pytest.mark.parametrize("inst", DR.MOMENTS_INSTANCES, ids=DR.moments_id)
def test_every_moments_instance_matches_the_host_reference(inst):
    from bayesdll_amd import kernels as K
    kind, recip, has_m2 = inst
    ca, cb = (7.0, 1.0) if kind in (DR.WELFORD_INIT, DR.WELFORD) else (6.0, 7.0)
    cus = _cus()
    sizes = DR.size_table(cus, 1, 4)
    DR.check_size_table(sizes, cus, 1, 4)
    assert DR.moments_instance(kind, recip, has_m2) == inst
    prev = K.set_launch_config(1, 1, 1)  # one workgroup per CU (the update always runs unroll 4)
    try:
        for n in sizes:
            e1, e2 = _moments_case(inst, n, ca, cb)
        if recip:  # inv_collect_* left 0: the library's own 1 / fl32(s)
            _moments_case(inst, 4 * 1024 + 1, 4.9, 4.9, fallback=True)
    finally:
        K.restore_launch_config(prev)
    n = max(sizes)
    _moments_case(inst, n, ca, cb)  # and once at the library's default of 2 workgroups per CU
    d2 = DR.sweep(n, cus, 2, 4)
    assert any(t >= 2 for t, _ in d2) and any(tl is not None for _, tl in d2)
    if kind in (DR.WELFORD, DR.MEAN):  # the other division mode would not pass
        h, _ = _data()
        o1, o2 = DR.moments(kind, h["x"][:n], h["a1"][:n], h["a2"][:n] if has_m2 else None, ca, cb,
                            "true" if recip else "recip")
        assert _differ(e1, o1) and (not has_m2 or _differ(e2, o2))


# -------------------------------------------------------------- special values
_FMAX, _FMIN, _DEN = np.finfo(F).max, np.finfo(F).tiny, F(2.0 ** -149)
_MAGS = [F(0.0), _DEN, _FMIN, F(2.0 ** -60), F(2.0 ** 60), _FMAX, F(np.inf)]
SPECIALS = np.array([s * m for m in _MAGS for s in (F(1), F(-1))] + [F(np.nan)], F)
CHUNK = 1020  # elements of a launch that lies wholly in the guarded iteration at unroll 1 and 4


def _triples(extra):
    t = np.array(list(itertools.product(SPECIALS, repeat=3)) + extra, F)
    pad = (-len(t)) % 4096  # a multiple of the largest block iteration: full trips only
    t = np.concatenate([t, np.ones((pad, 3), F)])
    return (np.ascontiguousarray(t[:, i]) for i in range(3))


def _placements(n):
    """(slices launched) with the vector wholly in full trips, then wholly in
    guarded iterations (launches of fewer elements than one block iteration)."""
    assert n % 4096 == 0 and CHUNK % 4 == 0 and CHUNK < 4 * 256
    return [[slice(0, n)], [slice(o, min(o + CHUNK, n)) for o in range(0, n, CHUNK)]]


@pytest.mark.parametrize("unroll", [1, 4])
def test_special_values_of_the_draw(unroll):
    """Every (m1, second moment, eps) triple of +-0, the smallest subnormal,
    FLT_MIN, 2^+-60, FLT_MAX, +-inf and NaN — each has a defined IEEE result —
    plus q == m * m exactly, in every variance form at both floors."""
    from bayesdll_amd import kernels as K
    m1, q, eps = _triples([(3.0, 9.0, 1.5), (-0.5, 0.25, -2.0), (2.0 ** 60, 2.0 ** 120, 1.0)])
    n = len(m1)
    cus = _cus()
    full = DR.sweep(n, cus, 1, unroll)
    assert all(tl is None for _, tl in full) and sum(t for t, _ in full) * 256 * unroll * 4 == n
    assert DR.sweep(CHUNK, cus, 1, unroll) == [(0, tuple(
        max(0, min(256, CHUNK // 4 - 256 * u)) for u in range(unroll)))]
    md, qd, ed = _dev(m1), _dev(q), _dev(eps)
    for (var_mode, has_m2, recip), floor in itertools.product(DR._VAR_SOURCES, (1e-12, 2.0 ** -97)):
        ratio = {DR.VAR_RAW_MOMENTS: 1.25, DR.VAR_WELFORD: 7.0, DR.VAR_GIVEN: 1.0}[var_mode]
        inv = float(DR.D.inv_of(ratio)) if recip else 0.0
        ref = DR.draw(m1, q if has_m2 else None, eps, var_mode=var_mode, ratio=ratio, inv_ratio=inv,
                      var_floor=floor)
        assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).any()
        for slices in _placements(n):
            out = torch.full((n,), 7.0, device=DEV)
            for s in slices:
                K.posterior_sample(out[s], md[s], qd[s] if has_m2 else None, var_mode=var_mode,
                                   ratio=ratio, var_floor=floor, noise=ed[s],
                                   div_mode="recip" if recip else "true", geometry=(1, unroll))
            _same(out, ref, (var_mode, has_m2, recip, floor, len(slices)))


def test_special_values_of_the_moment_update():
    """Every (x, m1, m2) triple of the special values, plus x == m1 and a
    Welford d * d2 that overflows to inf, for all 16 instances, once in full
    trips and once in guarded iterations."""
    x, m1, m2 = _triples([(1.5, 1.5, 2.0), (-0.0, 0.0, 1.0), (2.0 ** 100, 0.0, 1.0),
                          (-(2.0 ** 100), 2.0 ** 90, 3.0)])
    n = len(x)
    xd = _dev(x)
    w1, w2 = DR.moments(DR.WELFORD, x, m1, m2, 7.0, 1.0, "true")
    i = np.flatnonzero((x == F(2.0 ** 100)) & (m1 == 0))[0]  # d * d2 = 2^100 * (6/7) 2^100
    assert np.isposinf(w2[i]) and np.isfinite(w1[i])
    for inst in DR.MOMENTS_INSTANCES:
        kind, recip, has_m2 = inst
        ca, cb = (7.0, 1.0) if kind in (DR.WELFORD_INIT, DR.WELFORD) else (6.0, 7.0)
        mode = "recip" if recip else "true"
        e1, e2 = DR.moments(kind, x, m1, m2 if has_m2 else None, ca, cb, mode)
        for slices in _placements(n):
            a1, a2 = _dev(m1), _dev(m2)
            for s in slices:
                _launch_moments(xd[s], a1[s], a2[s] if has_m2 else None, kind, ca, cb, mode)
            _same(a1, e1, (DR.moments_id(inst), len(slices), "mom1"))
            _same(a2, e2 if has_m2 else m2, (DR.moments_id(inst), len(slices), "mom2"))
        _same(xd, x, "theta is not written")


# ------------------------------------------------------------ the stacked draw
def _stacked_cases(cus, unroll):
    """(K, chain_groups): seams inside block iterations of a small launch, and
    a seam strictly inside a workgroup's second full trip."""
    kiter = 256 * unroll
    stride = cus * kiter                     # groups of one whole-grid trip at 1 workgroup / CU
    cg = -(-(stride + kiter // 2) // 3)      # 3 * cg: the middle of workgroup 0's second trip
    assert stride < 3 * cg < stride + kiter and stride + kiter <= 5 * cg
    sw = DR.sweep(5 * 4 * cg, cus, 1, unroll)
    assert sw[0][0] >= 2  # workgroup 0 takes that second trip unguarded
    return [(3, 257), (5, cg)]


@pytest.mark.parametrize("unroll", [1, 4])
@pytest.mark.parametrize("form", ["RAW_MOMENTS", "WELFORD-recip"])
def test_stacked_draw_matches_the_host_reference_chain_by_chain(form, unroll):
    """chain_groups > 0: chain k's slot is drawn with the (seed, chain + k,
    step) stream, the group index counted inside the slot; the padding of a
    slot is part of the launch (n = K * 4 * chain_groups) and is drawn like
    any element.  Chain ids run up to the largest the entry point accepts."""
    from bayesdll_amd import kernels as K
    var_mode, ratio, recip = (DR.VAR_RAW_MOMENTS, 1.25, False) if form == "RAW_MOMENTS" else \
        (DR.VAR_WELFORD, 7.0, True)
    h, _ = _data()
    q_all, _ = _second_moment(var_mode, ratio, 1e-12)
    for chains, cg in _stacked_cases(_cus(), unroll):
        n = chains * 4 * cg
        chain0 = 2 ** 32 - chains - 1  # chain0 + K - 1 == 2^32 - 2, the last id accepted
        m1, q = h["m1"][:n], q_all[:n]

        def normals(k, seed, chain, step):
            assert seed == SEED and step == STEP and chain0 <= chain < 2 ** 32 - 1
            return K.philox_normal(k, seed, chain, step, device=DEV).cpu().numpy()

        ref = DR.draw_stacked(m1, q, normals, chains=chains, chain_groups=cg, seed=SEED, chain=chain0,
                              step=STEP, var_mode=var_mode, ratio=ratio, var_floor=1e-12,
                              inv_ratio=float(DR.D.inv_of(ratio)) if recip else 0.0)
        out = torch.full((n,), float("nan"), device=DEV)
        K.posterior_sample(out, _dev(m1), _dev(q), var_mode=var_mode, ratio=ratio, seed=SEED,
                           chain=chain0, step=STEP, div_mode="recip" if recip else "true",
                           chain_groups=cg, geometry=(1, unroll))
        _same(out, ref, (form, unroll, chains, cg))
        # not the one-chain stream: the slots of chains 1.. differ from it
        one = DR.draw(m1, q, normals(n, SEED, chain0, STEP), var_mode=var_mode, ratio=ratio,
                      inv_ratio=float(DR.D.inv_of(ratio)) if recip else 0.0)
        assert np.array_equal(_bits(one[:4 * cg]), _bits(ref[:4 * cg])) and _differ(one, ref)


def test_the_draw_refuses_group_and_chain_ids_reaching_2_to_32():
    """Validation only: every call returns before any launch."""
    from bayesdll_amd import _lib as L
    buf, src = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)

    def call(n, chain, chain_groups):
        a = L.SampleArgs()
        a.out, a.mom1 = buf.data_ptr(), src.data_ptr()
        a.n, a.var_mode, a.noise_mode = n, L.VAR_GIVEN, L.NOISE_PHILOX
        a.ratio, a.var_floor = 1.0, 1e-12
        a.seed, a.chain, a.step, a.chain_groups = 1, chain, 2, chain_groups
        rc = L.lib().bdl_posterior_sample(a, L.current_stream_handle(buf.device))
        return rc, (L.lib().bdl_last_error() or b"").decode()

    g32 = 1 << 32
    for n, chain, cg, word in ((4 * g32 + 1, 0, 0, "group index"),        # one chain: group 2^32
                               (4 * g32, 0, 1 << 20, "group index"),      # stacked: 2^32 groups
                               (16, g32, 0, "chain id"),
                               (16, g32 - 4, 1, "chain id"),              # chain + 4 chains == 2^32
                               (16, g32 - 1, 4, "chain id")):
        rc, msg = call(n, chain, cg)
        assert rc != L.BDL_OK and word in msg, (n, chain, cg, rc, msg)
    rc, msg = call(16, g32 - 5, 1)  # chains 2^32 - 5 .. 2^32 - 2: accepted
    assert rc == L.BDL_OK, msg
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the tuner
def test_repeated_draws_and_the_tuner_write_the_same_bits():
    """geometry=None on SAMPLE_TUNE_MIN elements: the first call times every
    geometry with the caller's own arguments, then draws; a second call reuses
    the choice.  Both equal the reference."""
    from bayesdll_amd import kernels as K
    n = K.SAMPLE_TUNE_MIN
    rng = np.random.default_rng(5)
    m1 = (0.02 * rng.standard_normal(n)).astype(F)
    q = (1e-4 * 7.0 * rng.uniform(0.5, 2.0, n)).astype(F)
    eps = K.philox_normal(n, SEED, CHAIN, STEP, device=DEV).cpu().numpy()
    ref = DR.draw(m1, q, eps, var_mode=DR.VAR_WELFORD, ratio=7.0, inv_ratio=DR.D.inv_of(7.0))
    md, qd = _dev(m1), _dev(q)
    key = (md.device.index, n)
    K._SAMPLE_GEOM.pop(key, None)
    for call in range(2):
        out = torch.full((n,), float("nan"), device=DEV)
        K.posterior_sample(out, md, qd, var_mode=DR.VAR_WELFORD, ratio=7.0, seed=SEED, chain=CHAIN,
                           step=STEP, div_mode="recip")
        assert K.sample_geometry(n, md.device) in K.SAMPLE_GEOMETRIES
        _same(out, ref, ("tuned draw", call))
