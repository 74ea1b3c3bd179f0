"""bdl_chain_clip and bdl_chain_stats on table T of tests/segment_sweep_ref.py:
every path of the traversal they share (head / tail lanes, full and partial
block iterations, rotated second trips, idle workgroups, the element-wise
path), reached at geometries the CPU tests prove (tests/test_segment_sweep_host.py).

Every clip launch works in the guard-NaN arena of tests/test_gpu_chain_clip.py
and the whole arena is compared as int32: an overread puts a NaN into a norm,
an overwrite changes a guard word.  The statistics read their vectors between
NaNs (gaps, slot padding, guard words) and must leave every word as it was.

Criteria: integer, power-of-two, planted and special-value inputs make the
fp64 sums exact in any order — norm, coefficient, every word and every sum
equal the reference bit for bit.  Random inputs: the norm within one fp32 ulp
of the float64 reference (chain_clip_ref.within_one_ulp), coefficient and
words exact from the device's own norm / coefficient; the statistics within
chain_stats_ref's summation bound 2 n 2^-53 sum|terms|."""
import functools
import math

import numpy as np
import pytest
import torch

import chain_clip_ref as CR
import chain_stats_ref as SRF
import segment_sweep_ref as SR
import test_gpu_chain_clip as TC
from step_ref import clip_coef

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
K_ = SR.K_T
GUARD = TC.GUARD
FORMS = ("tensor", "flat")
BOUND = [(True, True), (True, False), (False, True), (False, False)]  # (mom, prior)
LR = (0.05, 0.125)


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.int32)


@functools.lru_cache(maxsize=None)
def _pt(form):
    return SR.PlacedT(form)


def test_default_geometry_on_this_device():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("compute units", cus, "blocks_per_chain = 0 ->", SR.check_default_geometry(cus))


# ======================================================================= clip
def _arena(form, fill):
    """The arena with chain k's slice of segment i set to fill(i, k, numel)."""
    pt = _pt(form)
    arena = np.full(pt.total, GUARD, dtype=np.int32)
    f = arena.view(F)
    for i in range(len(pt.segs)):
        for k in range(K_):
            f[pt.span(i, k)] = fill(i, k, pt.numels[i])
    return arena


def _chains(pt, arena):
    f = arena.view(F)
    return [[f[pt.span(i, k)].copy() for i in range(len(pt.segs))] for k in range(K_)]


def _reference(pt, arena, max_norm):
    with np.errstate(all="ignore"):
        norms, coefs, _ = CR.chain_clip(_chains(pt, arena), max_norm)
    return norms, coefs


def _expected(pt, arena, coefs):
    with np.errstate(all="ignore"):
        return TC._expected(arena, pt.segs, K_, coefs)


def _clip_exact(form, arena, max_norm, bpc, nan_at=()):
    """One launch whose sum of squares is exact in any order: norm,
    coefficient and every arena word equal the reference's bit for bit.
    nan_at: arena words where the product is a NaN (inf * 0) — its sign is the
    platform's, so those are compared as NaN."""
    pt = _pt(form)
    norms, coefs = _reference(pt, arena, max_norm)
    after, tab = TC._run(arena, pt.segs, K_, max_norm, bpc)
    what = (form, max_norm, bpc)
    assert np.array_equal(_bits(tab[:, 0]), _bits(norms)), (what, tab[:, 0], norms)
    assert np.array_equal(_bits(tab[:, 1]), _bits(coefs)), (what, tab[:, 1], coefs)
    want = _expected(pt, arena, coefs)
    for w in nan_at:
        assert np.isnan(after.view(F)[w]) and np.isnan(want.view(F)[w]), (what, w)
        after[w] = want[w] = 0
    bad = np.flatnonzero(after != want)
    assert bad.size == 0, (what, bad[:8], bad.size)
    return tab, after


@functools.lru_cache(maxsize=None)
def _clip_case(form, kind):
    rng = np.random.default_rng([3, FORMS.index(form), len(kind)])
    if kind == "integer":   # |g| <= 8; chain k drawn from [-w, w]: three different norms
        widths = (1, 8, 3)
        arena = _arena(form, lambda i, k, n: rng.integers(-widths[k], widths[k] + 1, n))
        nr = sorted(float(CR.chain_norm(sl)) for sl in _chains(_pt(form), arena))
        max_norm = 0.5 * (nr[0] + nr[1])
    else:
        max_norm = TC.MAX_NORM
        arena = _arena(form, lambda i, k, n: rng.standard_normal(n))
        pt, f = _pt(form), arena.view(F)
        for k, sl in enumerate(_chains(pt, arena)):
            nrm = math.sqrt(sum(float(np.dot(g.astype(np.float64), g.astype(np.float64)))
                                for g in sl))
            for i in range(len(pt.segs)):
                f[pt.span(i, k)] *= F(TC.TARGETS[k] * max_norm / nrm)
    arena.setflags(write=False)
    return arena, float(max_norm)


@pytest.mark.parametrize("form", FORMS)
def test_clip_integer_gradient_is_exact_on_every_path(form):
    arena, max_norm = _clip_case(form, "integer")
    _, coefs = _reference(_pt(form), arena, max_norm)
    assert (coefs < 1).any() and (coefs == 1).any()   # the chains straddle max_norm
    for bpc in SR.CLIP_BPC + (0,):
        _clip_exact(form, arena, max_norm, bpc)


@pytest.mark.parametrize("form", FORMS)
def test_clip_random_gradient_on_every_path(form):
    arena, max_norm = _clip_case(form, "random")
    pt = _pt(form)
    norms, coefs = _reference(pt, arena, max_norm)
    assert (coefs < 1).any() and (coefs == 1).any()
    for bpc in SR.CLIP_BPC + (0,):
        after, tab = TC._run(arena, pt.segs, K_, max_norm, bpc)
        print(form, bpc, "norm dev", tab[:, 0], "ref", norms, "coef dev", tab[:, 1])
        for k in range(K_):
            assert CR.within_one_ulp(tab[k, 0], norms[k]), (form, bpc, k, tab[k, 0], norms[k])
            assert _bits(tab[k, 1]) == _bits(clip_coef(tab[k, 0], max_norm)), (form, bpc, k)
            assert (tab[k, 1] < 1) == (coefs[k] < 1), (form, bpc, k)
        bad = np.flatnonzero(after != _expected(pt, arena, tab[:, 1]))
        assert bad.size == 0, (form, bpc, bad[:8], bad.size)


# (segment, geometry, path, trip / sub-block, lane): where the single large
# element goes.  SR.element_of maps it to the element the restatement says
# that path reads; None would mean the path does not exist there (asserted).
PLANTED = [
    ("m1n9", 3, "head", 0, 2), ("m3n4", 7, "head", 0, 0), ("m0n7", 3, "tail", 0, 2),
    ("m2n9", 2, "tail", 0, 0),
    ("m2n1", 3, "head", 0, 0), ("m1n2", 2, "head", 0, 1),          # numel < head
    ("big4a", 2, "full", 0, 17), ("big4a", 2, "full", 1, 255),      # b = 1: first, rotated second trip
    ("big4b", 3, "full", 0, 0),
    ("big4a", 3, "partial", 0, 5), ("big4b", 3, "partial", 1, 43),  # after one full trip
    ("b4_1023", 1, "partial", 0, 0), ("b4_1023", 1, "partial", 1, 100),
    ("b4_1023", 2, "partial", 2, 255), ("b4_1023", 7, "partial", 3, 254),
    ("b4_257", 1, "partial", 1, 0), ("b4_1025", 1, "partial", 0, 0),
]


@pytest.mark.parametrize("form,chain", [("flat", 1), ("tensor", 0)])
def test_clip_one_planted_element_per_path(form, chain):
    """All elements 1, one element 2^20: s = 2^40 + (count - 1) exactly.  A path
    that is skipped leaves norm ~ sqrt(count), one read twice sqrt(2) * 2^20."""
    pt = _pt(form)
    ones = _arena(form, lambda i, k, n: np.ones(n, F))
    for name, bpc, kind, where, lane in PLANTED:
        i = pt.index(name)
        e = SR.element_of(pt, i, chain, bpc, kind, trip=where, sub=where, lane=lane)
        assert e is not None and 0 <= e < pt.numels[i], (name, bpc, kind, where, lane)
        arena = ones.copy()
        arena.view(F)[pt.span(i, chain)][e] = F(2.0 ** 20)
        tab, _ = _clip_exact(form, arena, 1.0, bpc)
        assert tab[chain, 0] == F(2.0 ** 20) and tab[(chain + 1) % K_, 0] < 300, (name, tab)


# ------------------------------------------------------------- special values
def _region(pt, k, region):
    """Arena words of chain k that head / tail lanes read ("lanes") or that
    block iterations read ("body")."""
    out = []
    for i, row in enumerate(pt.rows()):
        h, nbody, tail = SR.split(SR.chain_mis(row[0], row[2], k), row[1])
        s = pt.span(i, k)
        idx = np.arange(s.start, s.stop)
        out.append(idx[h:h + 4 * nbody] if region == "body" else
                   np.concatenate([idx[:h], idx[h + 4 * nbody:]]))
    return np.concatenate(out)


def _special(region, values, others=0.0):
    """Chain 1: `others` everywhere, `values` (cycled, alternating sign) over
    the region; chains 0 and 2: +-2^-30 (an exact sum, a norm of about 2.5e-7:
    unclipped at any max_norm >= 1e-5), compared with the reference like chain 1."""
    pt = _pt("tensor")
    rng = np.random.default_rng(17)
    arena = _arena("tensor", lambda i, k, n: np.full(n, others, F) if k == 1
                   else (2 * rng.integers(0, 2, n) - 1) * 2.0 ** -30)
    w = _region(pt, 1, region)
    v = np.resize(np.asarray(values, dtype=F), w.size)
    v[1::2] = -v[1::2]
    arena.view(F)[w] = v
    return pt, arena, w


REGIONS = ("lanes", "body")


@pytest.mark.parametrize("region", REGIONS)
def test_clip_zero_and_negative_zero(region):
    """An all-zero chain: norm 0, coef = fl32(1e6 * max_norm) clamped.  At
    max_norm = 1e-7 the zero chain IS scaled (by 0.1): -0.0 keeps its sign."""
    pt, arena, w = _special(region, [0.0])          # the region alternates +0 / -0
    assert np.signbit(arena.view(F)[w]).any()
    for max_norm in (1e-7, 1.0):
        tab, after = _clip_exact("tensor", arena, max_norm, 3)
        assert tab[1, 0] == 0 and (tab[1, 1] < 1) == (max_norm < 1e-6)
        assert np.array_equal(after[w], arena[w])


@pytest.mark.parametrize("region", REGIONS)
def test_clip_subnormals_and_large_magnitudes(region):
    pt, arena, w = _special(region, [2.0 ** -140, 2.0 ** -149])
    tab, _ = _clip_exact("tensor", arena, 1e-7, 2)   # fp32 squares would all be 0
    assert 0 < tab[1, 0] < 2.0 ** -126 and tab[1, 1] < 1
    pt, arena, w = _special(region, [2.0 ** 100])    # fp32 squares would be inf
    tab, _ = _clip_exact("tensor", arena, 1.0, 2)
    assert np.isfinite(tab[1, 0]) and tab[1, 0] == F(2.0 ** 100 * math.sqrt(w.size))
    pt, arena, w = _special(region, [2.0 ** 127])    # s = 2^254 * count > FLT_MAX^2
    assert w.size >= 8
    tab, after = _clip_exact("tensor", arena, 1.0, 2)
    assert np.isinf(tab[1, 0]) and tab[1, 1] == 0
    got = after.view(F)[w]
    assert (got == 0).all() and np.array_equal(np.signbit(got), np.signbit(arena.view(F)[w]))


@pytest.mark.parametrize("region", REGIONS)
def test_clip_one_infinity(region):
    pt, arena, w = _special(region, [1.5], others=-0.25)
    arena.view(F)[w[len(w) // 2]] = np.inf
    tab, after = _clip_exact("tensor", arena, 1.0, 3, nan_at=(w[len(w) // 2],))
    assert np.isinf(tab[1, 0]) and tab[1, 1] == 0
    rest = np.concatenate([after.view(F)[pt.span(i, 1)] for i in range(len(pt.segs))])
    assert (rest == 0).all()   # the inf's own word, a NaN, was checked and zeroed by _clip_exact
    for k in (0, 2):   # the neighbours: unclipped, bit-unchanged
        assert tab[k, 1] == 1
        for i in range(len(pt.segs)):
            assert np.array_equal(after[pt.span(i, k)], arena[pt.span(i, k)])


def _one_chain_finalize(poison):
    """(norm, coef) of bdl_sgld_step_clipped's finalize (bdl_api.hip) over a
    gradient holding one `poison` element."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    from test_gpu_kernels import _state
    st = _state([("fc.weight", (64,))], "fc", need_noise=True, need_prior=True)
    st.grad[5] = poison
    ws = K.sgld_step_clipped(st, 0.75, lrs=(1e-3, 2e-3), noise_scale=(0.1, 0.1),
                             noise_mode=L.NOISE_BUFFER, sigma2=0.64, n_data=500.0, mu=0.5,
                             first_step=False, momentum=True, div_mode="recip")
    torch.cuda.synchronize()
    return ws[:2].cpu().numpy(), st.theta.cpu().numpy()


@pytest.mark.parametrize("region", REGIONS)
def test_clip_nan_leaves_the_chain_untouched_in_both_finalize_kernels(region):
    """include/bdl_clip.h: fminf(NaN, 1) = 1 — a NaN norm gives coefficient 1
    and the chain is not written (clip_grad_norm_ would multiply it by NaN).
    The stacked finalize, the one-chain finalize of bdl_sgld_step_clipped and
    step_ref.clip_coef agree."""
    pt, arena, w = _special(region, [1.5], others=-0.25)
    arena.view(F)[w[len(w) // 3]] = np.nan
    assert _bits(clip_coef(F(np.nan), 0.75)) == _bits(F(1.0))
    after, tab = TC._run(arena, pt.segs, K_, 0.75, 3)
    assert np.isnan(tab[1, 0]) and _bits(tab[1, 1]) == _bits(clip_coef(tab[1, 0], 0.75))
    assert np.array_equal(after, arena)   # NaN payload, neighbours and guards: no word changed
    assert (tab[[0, 2], 1] == 1).all() and np.isfinite(tab[[0, 2], 0]).all()
    one, theta = _one_chain_finalize(float("nan"))
    assert np.isnan(one[0]) and _bits(one[1]) == _bits(tab[1, 1]) == _bits(F(1.0))
    assert np.isnan(theta).sum() == 1 and np.isnan(theta[5])   # stepped with coef 1: only the NaN's element
    one, _ = _one_chain_finalize(float("inf"))
    assert np.isinf(one[0]) and _bits(one[1]) == _bits(clip_coef(F(np.inf), 0.75)) == _bits(F(0.0))


@pytest.mark.parametrize("region", REGIONS)
def test_clip_norm_at_and_around_max_norm(region):
    """One non-zero element x: norm = |x| exactly.  max_norm = x and its two
    neighbours; the 1e-6 of the denominator makes all three clip, by
    coefficients the reference gives bit for bit."""
    pt, arena, w = _special(region, [0.0])
    x = F(0.8125) + np.spacing(F(0.8125))
    arena.view(F)[w[len(w) // 2]] = -x
    for max_norm in (np.nextafter(x, F(0)), x, np.nextafter(x, F(2)), F(x - F(4e-6))):
        tab, _ = _clip_exact("tensor", arena, float(max_norm), 7)
        assert tab[1, 0] == x
        assert _bits(tab[1, 1]) == _bits((F(1.0) / (x + F(1e-6))) * F(max_norm))
    tab, after = _clip_exact("tensor", arena, float(x + F(4e-6)), 7)
    assert tab[1, 1] == 1 and np.array_equal(after, arena)


# ====================================================================== stats
def _fill_stats(kind, rng, shape, i, which):
    if kind == "integer":
        return rng.integers(-64, 65, shape)
    if kind == "pow2":   # one exponent per segment and vector, subnormal and 2^60 among them
        e = {"g": (-140, -126, -60, -10, 0, 7, 30, 60), "theta": (3, -131, 59, 0, -20, 11, -70, 1),
             "mom": (-149, 60, 0, -33, 5, -127, 21, -2)}[which][i % 8]
        return np.where(rng.integers(0, 2, shape) == 1, 1.0, -1.0) * 2.0 ** e
    if kind == "rounding":   # theta - prior rounds: two exponents apart
        return rng.standard_normal(shape) * {"g": 1e-2, "theta": 0.3, "mom": 1e-3, "prior": 11.0}[which]
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _stats_data(kind):
    """Host data over T (read-only): stacked vectors [K, slot] with NaN in
    gaps and padding, the gradient per segment [K, numel]."""
    pt = _pt("flat")
    rng = np.random.default_rng([29, len(kind)])
    vec = {nm: np.full((K_, pt.slot), np.nan, dtype=F) for nm in ("theta", "mom", "prior")}
    grads = []
    for i, (o, n) in enumerate(zip(pt.offsets, pt.numels)):
        if kind == "ones":
            g = np.ones((K_, n), F)
            th, mv, pm = g, g, 0 * g
        else:
            g = _fill_stats(kind, rng, (K_, n), i, "g").astype(F)
            th = _fill_stats(kind, rng, (K_, n), i, "theta").astype(F)
            mv = _fill_stats(kind, rng, (K_, n), i, "mom").astype(F)
            pm = -th if kind == "pow2" else _fill_stats(kind, rng, (K_, n), i, "prior").astype(F)
        vec["theta"][:, o:o + n], vec["mom"][:, o:o + n], vec["prior"][:, o:o + n] = th, mv, pm
        grads.append(g)
    for v in list(vec.values()) + grads:
        v.setflags(write=False)
    return vec, grads


LR_ROWS = np.array([[0.01, 0.03], [0.02, 0.01], [0.04, 0.08]], dtype=F)


def _stats_ref(vec, grads, mom, prior, src):
    """([K, T, 6] sums, sums of |terms|) by chain_stats_ref.sums."""
    pt = _pt("flat")
    T = len(grads)
    s, a = np.zeros((K_, T, 6)), np.zeros((K_, T, 6))
    for k in range(K_):
        for i, (o, n) in enumerate(zip(pt.offsets, pt.numels)):
            lr = LR[i % 2] if src == "host" else LR_ROWS[k, i % 2]
            s[k, i], a[k, i] = SRF.sums(grads[i][k], vec["theta"][k, o:o + n],
                                        vec["mom"][k, o:o + n] if mom else None,
                                        vec["prior"][k, o:o + n] if prior else None, lr)
    return s, a


class _Stats:
    """A data set on the device in one gradient form: the stacked vectors, the
    gradient in T's guard arena, the segment table (lr group: i % 2)."""

    def __init__(self, kind, form):
        pt = self.pt = _pt(form)
        self.host_vec, self.grads = _stats_data(kind)
        self.vec = {nm: torch.from_numpy(v.copy()).to(DEV) for nm, v in self.host_vec.items()}
        arena = np.full(pt.total, np.nan, dtype=F)
        for i in range(len(pt.segs)):
            for k in range(K_):
                arena[pt.span(i, k)] = self.grads[i][k]
        self.grad = torch.from_numpy(arena).to(DEV)
        base = self.grad.data_ptr()
        assert base % 16 == 0 and all(v.data_ptr() % 16 == 0 for v in self.vec.values())
        self.table = torch.tensor([[base + 4 * a, n, s, o, i % 2] for i, ((a, n, s), o) in
                                   enumerate(zip(pt.segs, pt.offsets))], dtype=torch.int64).to(DEV)
        self.lr_rows = torch.from_numpy(LR_ROWS.copy()).to(DEV)
        self.before = {nm: v.clone() for nm, v in self.vec.items()}
        self.grad_before = self.grad.clone()
        self.T, self._ref = len(pt.segs), {}

    def ref(self, mom, prior, src):
        key = (mom, prior, src)
        if key not in self._ref:
            self._ref[key] = _stats_ref(self.host_vec, self.grads, mom, prior, src)
        return self._ref[key]

    def run(self, mom=True, prior=True, src="host", bpc=0, acc=None, accumulate=False):
        from bayesdll_amd import kernels as K
        if acc is None:
            acc = torch.full((K_, self.T, 6), float("nan"), dtype=torch.float64, device=DEV)
        kw = {"lr": LR} if src == "host" else {"lr_table": self.lr_rows, "lr_row_stride": 2}
        K.chain_stats(self.table, self.T, K_, self.pt.chain_groups, self.vec["theta"].view(-1), acc,
                      mom=self.vec["mom"].view(-1) if mom else None,
                      prior_mean=self.vec["prior"].view(-1) if prior else None,
                      accumulate=accumulate, blocks_per_chain=bpc, **kw)
        torch.cuda.synchronize()
        return acc, acc.cpu().numpy()

    def unchanged(self):
        same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731
        return same(self.grad, self.grad_before) and all(
            same(self.vec[nm], self.before[nm]) for nm in self.vec)


def _same_bits(got, want):
    return np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("mom,prior", BOUND)
@pytest.mark.parametrize("form", FORMS)
def test_stats_integer_inputs_are_exact_on_every_path(form, mom, prior):
    """|x| <= 64 and integer: all five sums and V2L equal the reference at every
    geometry and lr source; a second, accumulating launch doubles them."""
    d = _Stats("integer", form)
    for src in ("host", "table"):
        want = d.ref(mom, prior, src)[0]
        assert np.isfinite(want).all()
        if not mom:
            assert not want[..., [1, 4, 5]].any()
        for bpc in SR.STATS_BPC + (0,):
            acc, got = d.run(mom, prior, src, bpc)
            assert np.array_equal(got, want), (form, mom, prior, src, bpc,
                                               np.argwhere(got != want)[:4])
            _, got = d.run(mom, prior, src, bpc, acc=acc, accumulate=True)
            assert np.array_equal(got, 2 * want), (form, mom, prior, src, bpc, "accumulate")
    assert d.unchanged()


@pytest.mark.parametrize("form", FORMS)
def test_stats_powers_of_two_are_bit_equal_at_every_geometry(form):
    """Within a segment every term of a sum has one magnitude (2^-280 .. 2^120),
    so every partial sum is exact in any order."""
    d = _Stats("pow2", form)
    g0 = np.abs(np.concatenate([g.reshape(-1) for g in d.grads]))
    assert (g0 < 2.0 ** -126).any() and (g0 == 2.0 ** 60).any()
    for mom, prior in ((True, True), (False, False)):
        want = d.ref(mom, prior, "table")[0]
        assert np.isfinite(want).all() and (want[..., 0] > 0).all()
        for bpc in SR.STATS_BPC + (0,):
            _, got = d.run(mom, prior, "table", bpc)
            assert _same_bits(got, want), (form, mom, prior, bpc, np.argwhere(got != want)[:4])
    assert d.unchanged()


@pytest.mark.parametrize("form", FORMS)
def test_stats_difference_is_rounded_once_to_fp32(form):
    """d = fl32(theta - prior) (include/bdl_stats.h).  On this data the fp32
    difference is inexact in most elements; D2 and DG must match the sums of
    the ROUNDED d within the summation bound, and the sums of the exact
    difference lie outside it — a kernel subtracting in double would fail."""
    d = _Stats("rounding", form)
    pt, vec = d.pt, d.host_vec
    inexact = total = 0
    for mom in (True, False):
        want, absum = d.ref(mom, True, "host")
        numel = np.asarray(pt.numels, dtype=np.float64)
        bound = 2.0 * numel[None, :, None] * 2.0 ** -53 * absum
        if mom:   # the exact-difference reference, and that it is distinguishable
            outside = []
            for k in range(K_):
                for i, (o, n) in enumerate(zip(pt.offsets, pt.numels)):
                    t64 = vec["theta"][k, o:o + n].astype(np.float64)
                    p64 = vec["prior"][k, o:o + n].astype(np.float64)
                    x = t64 - p64   # exact: both fp32, exponents 2^-149 .. 2^7 apart fit 53 bits
                    assert all(math.fsum((a, -b)) == c for a, b, c in zip(t64[:64], p64[:64], x[:64]))
                    r = (vec["theta"][k, o:o + n] - vec["prior"][k, o:o + n]).astype(np.float64)
                    inexact += int((x != r).sum())
                    total += n
                    g64 = d.grads[i][k].astype(np.float64)
                    ex = np.array([math.fsum(x * x), math.fsum(x * g64)])
                    if n >= 64:
                        outside.append((np.abs(ex - want[k, i, 2:4]) > bound[k, i, 2:4]).all())
            assert 2 * inexact >= total, (inexact, total)
            assert len(outside) > 20 and all(outside)
        for bpc in (1, 3, 0):
            _, got = d.run(mom, True, "host", bpc)
            err = np.abs(got - want)
            print(form, mom, bpc, "max err / bound",
                  float(np.max(err / np.where(bound > 0, bound, 1))))
            assert np.isfinite(got).all()
            assert (err <= bound).all(), (form, mom, bpc, np.argwhere(err > bound)[:4])
    assert d.unchanged()


STATS_PLANTED = PLANTED + [
    ("b1_1023", 1, "partial", 0, 7), ("b1_1023", 2, "partial", 1, 0), ("b1_1023", 3, "partial", 2, 255),
    ("b1_1023", 7, "partial", 3, 254), ("b1_1025", 1, "partial", 0, 0), ("b1_1024", 1, "full", 0, 255),
    ("big1", 2, "full", 0, 1), ("big1", 2, "full", 1, 200), ("big1", 3, "partial", 1, 43),
]


def test_stats_one_planted_element_per_path():
    """All ones, one gradient element 2^10 in chain 0 ("tensor" form: the
    element-wise path exists): G2 of its (chain, segment) is numel - 1 + 2^20,
    every other entry its count — a skipped or doubled path shows in G2."""
    pt = _pt("tensor")
    d = _Stats("ones", "tensor")
    base = d.ref(True, True, "host")[0]
    theta, mom, prior = (d.host_vec[nm] for nm in ("theta", "mom", "prior"))
    for name, bpc, kind, where, lane in STATS_PLANTED:
        i = pt.index(name)
        e = SR.element_of(pt, i, 0, bpc, kind, trip=where, sub=where, lane=lane, stats=True)
        assert e is not None and 0 <= e < pt.numels[i], (name, bpc, kind, where, lane)
        assert (SR._path(pt.rows(True)[i], 0)[3] == 1) == name.startswith(("b1_", "big1"))
        g = d.grads[i][0].copy()
        g[e] = F(2.0 ** 10)
        o, n = pt.offsets[i], pt.numels[i]
        want = base.copy()
        want[0, i] = SRF.sums(g, theta[0, o:o + n], mom[0, o:o + n], prior[0, o:o + n], LR[i % 2])[0]
        assert want[0, i, 0] == n - 1 + 2.0 ** 20
        word = pt.span(i, 0).start + e
        d.grad[word] = 2.0 ** 10
        _, got = d.run(True, True, "host", bpc)
        d.grad[word] = 1.0
        assert np.array_equal(got, want), (name, bpc, kind, where, np.argwhere(got != want)[:4],
                                           got[0, i, 0], want[0, i, 0])
    assert d.unchanged()
