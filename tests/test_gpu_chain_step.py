"""bdl_chain_step (include/bdl_chain_step.h): K stacked chains stepped by one
launch, each with its own scalars, against the fp32 host reference
(tests/step_ref.py), the one-chain and the uniform stacked bdl_sgmcmc_step
launches, and the per_chain samplers against K = 1 samplers.

Every comparison of vectors is bit for bit, as int32 patterns over every
element (NaN positions as NaN-ness).  Conventions:
  * the padding of every slot (elements n1 .. 4*chain_groups - 1) is
    pre-filled with SENTINEL in EVERY vector and must come back untouched: the
    per-chain launch ends at n1;
  * frozen (SKIP) elements hold FROZEN_VALUE in theta, grad and mom and stay
    untouched there; their m1 / m2 are what the reference's collect gives (it
    reads the unchanged theta, as in test_gpu_step_reference.py); a first SGD
    step stores +0 in their buffer (the same file's convention);
  * chain k's Philox stream is K.philox_normal(n1, SEED, CHAIN + k, STEP), the
    device stream test_gpu_noise_stream.py pins to philox_ref.
The only tolerance here is evaluate_chains against its torch rebuild, 1e-6 as
the issue sets it (both sides are fp32 log-softmax sums over a few examples).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stacked_tables as T
import step_ref as R
from test_gpu_noise_units import CHAIN, SEED, STEP
from test_gpu_step_reference import COLLECTS, VARIANTS, _assert_bits, _expected, _first_buf
from test_stacked_host import Net

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL, FROZEN_VALUE = F(7.0), F(5.0)
VEC = ("theta", "grad", "mom", "prior", "noise", "m1", "m2")
SCALE = dict(theta=0.02, grad=1e-2, mom=1e-3, prior=0.02, noise=1.0, m1=0.02, m2=1e-3)
NONE, WELFORD_INIT, WELFORD, MEAN_INIT, MEAN, WELFORD_1, MEAN_1 = COLLECTS
BPCS = (1, 3, 64)


def chain_kw(k, family):
    """Chain k's scalars (doubles): every chain differs in every one."""
    s = 1.0 + 0.37 * k
    kw = dict(lrs=(1e-3 * s, 2e-2 / s), noise_scale=(1e-4 * s, 3e-4 / s))
    if family == "csghmc":
        kw.update(one_minus_alpha=0.82 - 0.05 * k, prior_sig=0.8 + 0.3 * k)
    else:
        kw.update(sigma2=(0.8 + 0.3 * k) ** 2, n_data=7.0 + 2.5 * k, mu=0.5 + 0.1 * k,
                  noise_scale=(3e-3 * s, 7e-3 / s))
    return kw


def row_of(kw, fallback=False):
    sc = R.Scalars(**kw)
    inv = (0.0, 0.0) if fallback else (sc.sigma2.inv, sc.n_data.inv)
    return [sc.lr[0], sc.lr[1], sc.ns[0], sc.ns[1], sc.oma, sc.prior_sig, sc.sigma2.s,
            sc.n_data.s, sc.mu, inv[0], inv[1], 0.0]


class Chains:
    """K stacked chains over a stacked_tables.Layout: vectors, one chain's run
    table, per-chain scalars and the host expectation."""

    def __init__(self, lay, seed, n1=None):
        from bayesdll_amd.flat import build_runs
        self.lay, self.K = lay, lay.K
        self.n1, self.stride = lay.n1, lay.stride
        self.attr1 = lay.slot_attr()[:lay.n1]
        skip1 = (self.attr1 & R.ATTR_SKIP) != 0
        self.skip = np.tile(np.concatenate([skip1, np.zeros(lay.stride - lay.n1, bool)]), lay.K)
        self.pad = np.tile(np.arange(lay.stride) >= lay.n1, lay.K)
        rng = np.random.default_rng(seed)
        self.h0 = {}
        for nm in VEC:
            x = rng.standard_normal(lay.n).astype(F) * F(SCALE[nm])
            x = np.abs(x) if nm == "m2" else x
            if nm in ("theta", "grad", "mom"):
                x[self.skip] = FROZEN_VALUE
            x[self.pad] = SENTINEL
            self.h0[nm] = x
        self.v = {nm: torch.from_numpy(x).to(DEV) for nm, x in self.h0.items()}
        self.nonfinite = torch.zeros(lay.K, dtype=torch.int32, device=DEV)
        self.runs = build_runs(lay.offsets, lay.numels, lay.attrs, lay.n1).to(DEV)
        self.state = SimpleNamespace(
            theta=self.v["theta"], grad=self.v["grad"], mom=self.v["mom"], prior=self.v["prior"],
            noise=self.v["noise"], nonfinite=self.nonfinite, K=lay.K, n1=lay.n1,
            chain_groups=lay.chain_groups, chain_runs=self.runs,
            chain_nruns=int(self.runs.shape[0]), chain_gbase=None, timer=None)

    def load(self, h=None):
        for nm in VEC:
            self.v[nm].copy_(torch.from_numpy((h or self.h0)[nm]))
        self.nonfinite.zero_()

    def slot(self, h, k, n=None):
        n = self.n1 if n is None else n
        return {nm: x[k * self.stride:k * self.stride + n] for nm, x in h.items()}

    def rows(self, kws, fallback=False):
        return torch.tensor([row_of(kw, fallback) for kw in kws], dtype=torch.float32, device=DEV)

    def expected(self, v, kws, mode, ck, h=None, fallback=()):
        """The whole stacked vectors after the launch: chain k's n1 elements
        from the host reference with chain k's scalars, the rest as before."""
        h = h or self.h0
        out = {}
        for k in range(self.K):
            e = _expected(v, self.slot(h, k), self.attr1, mode, ck, kw_over=kws[k],
                          fallback=fallback)
            for nm, x in e.items():
                out.setdefault(nm, h[nm].copy())[k * self.stride:k * self.stride + self.n1] = x
        return out

    def tensor_state(self):
        """The same launch with every tensor's gradients of all chains in a
        [K, numel] allocation of its own, through StackedState's own table."""
        from bayesdll_amd.stacked import StackedState
        lay = self.lay
        g2 = self.h0["grad"].reshape(lay.K, lay.stride)
        grads, ptrs = [], []
        for o, n, a in zip(lay.offsets, lay.numels, lay.attrs):
            if a & R.ATTR_SKIP:
                grads.append(None)
                ptrs.append(0)
                continue
            g = torch.from_numpy(np.ascontiguousarray(g2[:, o:o + n])).to(DEV)
            grads.append(g)
            ptrs.append(g.data_ptr())
        ss = StackedState.__new__(StackedState)
        ss.K, ss.offsets, ss.numels, ss.attrs = lay.K, lay.offsets, lay.numels, lay.attrs
        ss.device = torch.device(DEV, 0)
        runs, nruns, gbase = ss._build_chain_table(ptrs)
        st = SimpleNamespace(**vars(self.state))
        st.grad, st.chain_runs, st.chain_nruns, st.chain_gbase = None, runs, nruns, gbase
        st.tensor_grads = grads
        return st

    def check(self, exp, what, first_buf=None, flags=0):
        torch.cuda.synchronize()
        got = {nm: self.v[nm].cpu().numpy() for nm in VEC}
        for nm in VEC:
            _assert_bits(got[nm], exp.get(nm, self.h0[nm]), what + (nm,))
            assert (got[nm][self.pad] == SENTINEL).all(), what + (nm, "padding")
        for nm in ("theta", "grad", "mom"):
            if nm == first_buf:
                assert not got[nm][self.skip].view(np.int32).any(), what + (nm, "frozen")
            else:
                assert (got[nm][self.skip] == FROZEN_VALUE).all(), what + (nm, "frozen")
        assert self.nonfinite.cpu().tolist() == ([flags] * self.K if isinstance(flags, int)
                                                 else flags), what


_C = {}


def _chains(name):
    if name not in _C:
        lay, seed = {"A": (T.table_a, 811), "B": (T.table_b, 812), "C": (T.table_c, 813)}[name]
        _C[name] = Chains(lay(), seed)
    return _C[name]


def _launch(st, v, mode, ck, rows, noise="BUFFER", m1=None, m2=None, **kw):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    kind, has_m2, ca, cb = ck
    if kind != "NONE":
        kw.update(collect=getattr(L, "COLLECT_" + kind), mom1=m1, mom2=m2 if has_m2 else None,
                  collect_a=ca, collect_b=cb)
    if v.mom:
        kw.update(momentum=True, first_step=v.mom == "first")
    nm = getattr(L, "NOISE_" + (noise if v.noise else "NONE"))
    K.chain_step(st, getattr(L, v.method), scalars=rows, noise_mode=nm, div_mode=mode, **kw)


def _collects(v):
    return [NONE, WELFORD_INIT, WELFORD, WELFORD_1] if v.family == "csghmc" else \
        [NONE, MEAN_INIT, MEAN, MEAN_1]


def _unrolls(v, ck, noise="BUFFER"):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    nm = getattr(L, "NOISE_" + (noise if v.noise else "NONE"))
    return K.chain_step_unrolls(getattr(L, v.method), nm, getattr(L, "COLLECT_" + ck[0]))


CASES = ["csghmc_explore", "csghmc_noise", "sgld_no_momentum", "sgld_first", "sgld_later"]


# ----------------------------------------------------------- 1. host reference
@pytest.mark.parametrize("case", CASES)
def test_every_chain_matches_the_host_reference_with_its_own_scalars(case):
    """Table A (K = 3, 39,426 elements in slots of 39,428: a frozen tensor, a
    head group, multi-run and guarded iterations, a partial last group),
    buffer noise, every chain other scalars: every collect kind with and
    without m2, both division modes, blocks_per_chain 1, 3 and 64 (more
    workgroups than block iterations) and every unroll offered."""
    v, c = VARIANTS[case], _chains("A")
    assert (c.K, c.n1, c.stride) == (3, 39426, 39428) and c.skip.any()
    kws = [chain_kw(k, v.family) for k in range(c.K)]
    rows = c.rows(kws)
    launches = 0
    for ck in _collects(v):
        unrolls = _unrolls(v, ck)
        assert 1 in unrolls and (v.family != "csghmc" or unrolls == (1, 2, 4))
        for mode in ("true", "recip"):
            exp = c.expected(v, kws, mode, ck)
            assert any(not np.array_equal(exp[nm].view(np.int32), c.h0[nm].view(np.int32))
                       for nm in exp)
            for bpc in BPCS:
                for u in unrolls:
                    c.load()
                    _launch(c.state, v, mode, ck, rows, m1=c.v["m1"], m2=c.v["m2"],
                            blocks_per_chain=bpc, unroll=u)
                    c.check(exp, (case, ck[:2], mode, bpc, u), _first_buf(v))
                    launches += 1
    assert launches >= 4 * 2 * 3
    # chains really differ: chain 1's scalars on chain 0's slot give another theta
    e0 = _expected(v, c.slot(c.h0, 0), c.attr1, "true", NONE, kw_over=kws[0])
    e1 = _expected(v, c.slot(c.h0, 0), c.attr1, "true", NONE, kw_over=kws[1])
    assert (e0["theta"].view(np.int32) != e1["theta"].view(np.int32)).any()


def test_reciprocal_fallback_is_formed_per_chain():
    """inv_sigma2 = inv_n_data = 0 in a row: the kernel uses 1 / fl32(s) of
    that chain's own divisors (step_ref.Div.fallback)."""
    v, c = VARIANTS["sgld_later"], _chains("A")
    kws = [chain_kw(k, "sgld") for k in range(c.K)]
    fb = lambda kw: (("sigma2", kw["sigma2"]), ("n_data", kw["n_data"]))  # noqa: E731
    out = {}
    for k in range(c.K):
        e = _expected(v, c.slot(c.h0, k), c.attr1, "recip", MEAN, kw_over=kws[k],
                      fallback=fb(kws[k]))
        for nm, x in e.items():
            out.setdefault(nm, c.h0[nm].copy())[k * c.stride:k * c.stride + c.n1] = x
    c.load()
    _launch(c.state, v, "recip", MEAN, c.rows(kws, fallback=True), m1=c.v["m1"], m2=c.v["m2"])
    c.check(out, ("fallback",))


@pytest.mark.parametrize("case", ["csghmc_noise", "sgld_later"])
def test_per_tensor_gradients_through_the_base_table(case):
    """The gradients read in place from [K, numel] tensors through the K x
    nruns base table; some bases are not 16-byte addressable."""
    from bayesdll_amd import _lib as L
    v, c = VARIANTS[case], _chains("A")
    kws = [chain_kw(k, v.family) for k in range(c.K)]
    rows = c.rows(kws)
    steady = WELFORD if v.family == "csghmc" else MEAN
    for ck in (NONE, steady):
        exp = c.expected(v, kws, "true", ck)
        for bpc in (1, 3):
            for u in _unrolls(v, ck):
                c.load()
                st = c.tensor_state()
                assert st.chain_nruns == len(c.lay.names) and tuple(st.chain_gbase.shape) == \
                    (c.K, st.chain_nruns)
                assert any(int(r[1]) & L.ATTR_GUNALIGNED for r in st.chain_runs.tolist())
                assert (st.chain_gbase.cpu().numpy() % 16 != 0).any()
                _launch(st, v, "true", ck, rows, m1=c.v["m1"], m2=c.v["m2"],
                        blocks_per_chain=bpc, unroll=u)
                c.check(exp, ("tensor", case, ck[:2], bpc, u))
                g2 = c.h0["grad"].reshape(c.K, c.stride)
                for o, n, g in zip(c.lay.offsets, c.lay.numels, st.tensor_grads):
                    if g is not None:  # read, never written
                        _assert_bits(g.cpu().numpy(), np.ascontiguousarray(g2[:, o:o + n]), (o,))


# ------------------------------------------------------------------ 2. Philox
def _one_chain_state(c, h, k):
    """A one-chain launchable state over a copy of chain k's slot."""
    v = {nm: torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for nm, x in c.slot(h, k).items()}
    return SimpleNamespace(theta=v["theta"], grad=v["grad"], gbase=None, mom=v["mom"],
                           prior=v["prior"], noise=v["noise"], runs=c.runs,
                           nruns=int(c.runs.shape[0]), n=c.n1, device=torch.device(DEV, 0),
                           nonfinite=torch.zeros(1, dtype=torch.int32, device=DEV), timer=None, v=v)


@pytest.mark.parametrize("case,ck", [("csghmc_noise", NONE), ("csghmc_noise", WELFORD),
                                     ("sgld_later", NONE), ("sgld_later", MEAN),
                                     ("sgld_first", MEAN_INIT)])
def test_philox_chain_equals_the_one_chain_launch_and_the_reference(case, ck):
    """Chain k of a Philox launch == bdl_sgmcmc_step over a copy of chain k's
    slot with chain id CHAIN + k and chain k's scalars == step_ref fed
    bdl_philox_normal(n1, SEED, CHAIN + k, STEP); a 64-bit seed, a step above
    2^32."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    assert SEED >> 32 and STEP >> 32
    v, c = VARIANTS[case], _chains("A")
    kws = [chain_kw(k, v.family) for k in range(c.K)]
    eps = np.full(c.lay.n, SENTINEL, dtype=F)
    for k in range(c.K):
        eps[k * c.stride:k * c.stride + c.n1] = \
            K.philox_normal(c.n1, SEED, CHAIN + k, STEP, device=DEV).cpu().numpy()
    exp = c.expected(v, kws, "recip", ck, h=dict(c.h0, noise=eps))
    for u in _unrolls(v, ck, "PHILOX"):
        c.load()
        _launch(c.state, v, "recip", ck, c.rows(kws), noise="PHILOX", m1=c.v["m1"], m2=c.v["m2"],
                seed=SEED, chain=CHAIN, step=STEP, unroll=u, blocks_per_chain=3)
        c.check(exp, ("philox", case, ck[:2], u), _first_buf(v))
    got = {nm: c.v[nm].cpu().numpy() for nm in VEC}
    kind, has_m2, ca, cb = ck
    for k in range(c.K):
        st = _one_chain_state(c, c.h0, k)
        kw = dict(v.kw, **kws[k])
        if kind != "NONE":
            kw.update(collect=getattr(L, "COLLECT_" + kind), mom1=st.v["m1"], mom2=st.v["m2"],
                      collect_a=ca, collect_b=cb)
        K.sgmcmc_step(st, getattr(L, v.method), noise_mode=L.NOISE_PHILOX, div_mode="recip",
                      seed=SEED, chain=CHAIN + k, step=STEP, **kw)
        torch.cuda.synchronize()
        for nm in ("theta", "mom", "m1", "m2"):
            _assert_bits(st.v[nm].cpu().numpy(), c.slot(got, k)[nm], ("one-chain", case, k, nm))


# ------------------------------------------------------------ 3. uniform rows
@pytest.mark.parametrize("table", ["A", "B", "C"])
@pytest.mark.parametrize("case,ck", [("csghmc_explore", NONE), ("csghmc_noise", WELFORD),
                                     ("sgld_later", MEAN)])
def test_equal_rows_equal_the_uniform_stacked_launch(table, case, ck):
    """K equal rows: the launch equals today's stacked bdl_sgmcmc_step
    (chain_groups) launch on the same inputs, over every chain's n1 elements
    (that launch also collects over the padding, a SKIP run; this one never
    touches it)."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    v, c = VARIANTS[case], _chains(table)
    lay = c.lay
    kw1 = {k: v.kw[k] for k in ("lrs", "noise_scale", "one_minus_alpha", "prior_sig", "sigma2",
                                "n_data", "mu") if k in v.kw}
    kind, has_m2, ca, cb = ck
    ref = {nm: torch.from_numpy(c.h0[nm]).to(DEV) for nm in VEC}
    runs = lay.flat_runs().to(DEV)
    st = SimpleNamespace(theta=ref["theta"], grad=ref["grad"], gbase=None, mom=ref["mom"],
                         prior=ref["prior"], noise=ref["noise"], runs=runs,
                         nruns=int(runs.shape[0]), n=lay.n, device=torch.device(DEV, 0),
                         nonfinite=torch.zeros(1, dtype=torch.int32, device=DEV), timer=None,
                         chain_groups=lay.chain_groups)
    kw = dict(v.kw)
    if kind != "NONE":
        kw.update(collect=getattr(L, "COLLECT_" + kind), mom1=ref["m1"], mom2=ref["m2"],
                  collect_a=ca, collect_b=cb)
    noise = L.NOISE_PHILOX if v.noise else L.NOISE_NONE
    K.sgmcmc_step(st, getattr(L, v.method), noise_mode=noise, div_mode="recip", seed=SEED,
                  chain=CHAIN, step=STEP, **kw)
    c.load()
    _launch(c.state, v, "recip", ck, c.rows([kw1] * c.K), noise="PHILOX", m1=c.v["m1"],
            m2=c.v["m2"], seed=SEED, chain=CHAIN, step=STEP)
    torch.cuda.synchronize()
    live = ~c.pad
    changed = False
    for nm in VEC:
        a, b = c.v[nm].cpu().numpy(), ref[nm].cpu().numpy()
        _assert_bits(a[live], b[live], (table, case, nm))
        assert (a[c.pad] == SENTINEL).all()
        changed |= not np.array_equal(a.view(np.int32), c.h0[nm].view(np.int32))
    assert changed and c.nonfinite.cpu().tolist() == [0] * c.K


# ----------------------------------------------------------- 4. state carried
@pytest.mark.parametrize("family", ["sgld", "csghmc"])
def test_three_consecutive_steps_carry_their_state(family):
    """SGLD: the first SGD step, a momentum step with MEAN_INIT, a momentum
    step with MEAN.  cSGHMC: an explore step, a sample step with WELFORD_INIT,
    a WELFORD collect with the doubled count (3: quirk Q2).  Fresh buffer noise
    per step; the expectation is the host reference applied three times."""
    c = _chains("A")
    kws = [chain_kw(k, family) for k in range(c.K)]
    rows = c.rows(kws)
    if family == "sgld":
        plan = [("sgld_first", NONE), ("sgld_later", MEAN_INIT), ("sgld_later", ("MEAN", True, 1.0, 2.0))]
    else:
        plan = [("csghmc_explore", NONE), ("csghmc_noise", WELFORD_INIT),
                ("csghmc_noise", ("WELFORD", True, 3.0, 1.0))]
    rng = np.random.default_rng(77)
    h = dict(c.h0)
    c.load()
    for i, (case, ck) in enumerate(plan):
        v = VARIANTS[case]
        eps = rng.standard_normal(c.lay.n).astype(F)
        eps[c.pad] = SENTINEL
        h["noise"] = eps
        c.v["noise"].copy_(torch.from_numpy(eps))
        exp = c.expected(v, kws, "recip", ck, h=h)
        if _first_buf(v):  # the buffer a first step creates: +0 in frozen elements
            exp["mom"][c.skip] = 0.0
        _launch(c.state, v, "recip", ck, rows, m1=c.v["m1"], m2=c.v["m2"], unroll=1)
        torch.cuda.synchronize()
        h.update(exp)
        for nm in VEC:
            _assert_bits(c.v[nm].cpu().numpy(), h[nm], (family, i, nm))
    assert c.nonfinite.cpu().tolist() == [0] * c.K


# -------------------------------------------------------------------- 5. edges
@pytest.mark.parametrize("K_", [1, 2, 5])
def test_small_and_odd_sizes(K_):
    """n1 in {1, 3, 4, 5, 7, 1023, 4097}: one group and less, a partial last
    group, one block iteration and its guarded tail; K = 1 equals the
    one-chain launch as well."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    for n1 in (1, 3, 4, 5, 7, 1023, 4097):
        c = Chains(T.Layout([("l0.weight", n1)], K_), 900 + n1)
        for case, ck in (("csghmc_noise", WELFORD), ("sgld_later", MEAN)):
            v = VARIANTS[case]
            kws = [chain_kw(k, v.family) for k in range(K_)]
            exp = c.expected(v, kws, "true", ck)
            for u in _unrolls(v, ck):
                for bpc in (0, 2):
                    c.load()
                    _launch(c.state, v, "true", ck, c.rows(kws), m1=c.v["m1"], m2=c.v["m2"],
                            unroll=u, blocks_per_chain=bpc)
                    c.check(exp, (K_, n1, case, u, bpc))
            if K_ == 1:
                st = _one_chain_state(c, c.h0, 0)
                kind, _, ca, cb = ck
                K.sgmcmc_step(st, getattr(L, v.method), noise_mode=L.NOISE_BUFFER, div_mode="true",
                              collect=getattr(L, "COLLECT_" + kind), mom1=st.v["m1"],
                              mom2=st.v["m2"], collect_a=ca, collect_b=cb, **dict(v.kw, **kws[0]))
                torch.cuda.synchronize()
                for nm in ("theta", "mom", "m1", "m2"):
                    _assert_bits(st.v[nm].cpu().numpy(), c.v[nm].cpu().numpy()[:n1], (n1, nm))


# ---------------------------------------------------------- 6. divergence guard
@pytest.mark.parametrize("per_chain_flags", [True, False])
def test_one_diverging_chain_sets_the_flag_and_leaves_the_others(per_chain_flags):
    v, c = VARIANTS["csghmc_noise"], _chains("A")
    kws = [chain_kw(k, "csghmc") for k in range(c.K)]
    # lr * (g + prior_sig * theta) overflows in chain 1: theta = +-Inf
    kws[1] = dict(kws[1], lrs=(3e38, 3e38), prior_sig=3e38)
    exp = c.expected(v, kws, "true", NONE)
    sl = slice(c.stride, c.stride + c.n1)
    assert not np.isfinite(exp["theta"][sl]).all()
    assert np.isfinite(exp["theta"][:c.n1]).all() and np.isfinite(exp["theta"][2 * c.stride:]).all()
    c.load()
    _launch(c.state, v, "true", NONE, c.rows(kws), nonfinite_per_chain=per_chain_flags)
    c.check(exp, ("diverged", per_chain_flags), flags=[0, 1, 0] if per_chain_flags else [1, 0, 0])


# ------------------------------------------------------------------ 7. samplers
def _args(**over):
    a = SimpleNamespace(lr=5e-2, lr_head=1e-1, epochs=2, num_cycles=2, momentum=0.5,
                        proportion_exploration=0.5, ND=64, device=torch.device(DEV, 0), seed=7,
                        hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0,
                                 "nd": 1.0, "thin": 1, "nst": 2, "bias": "informative",
                                 "burnin": 0})
    hp = over.pop("hparams", {})
    for k, v in over.items():
        setattr(a, k, v)
    a.hparams.update(hp)
    return a


SWEEP = {
    "csghmc": {"lr": [5e-2, 1e-2, 3e-3], "lr_head": [0.1, 0.03, 3e-3], "prior_sig": [1.0, 0.3, 2.5],
               "momentum_decay": [0.1, 0.18, 0.05], "nd": [1.0, 0.01, 0.3],
               "Ninflate": [1.0, 1e3, 7.0]},
    "sgld": {"lr": [5e-2, 1e-2, 3e-3], "lr_head": [0.1, 0.03, 3e-3], "prior_sig": [1.0, 0.3, 2.5],
             "nd": [1.0, 0.01, 0.3], "Ninflate": [1.0, 1e3, 7.0], "momentum": [0.5, 0.9, 0.1]},
}


def _one_chain_args(family, k):
    s = {nm: v[k] for nm, v in SWEEP[family].items()}
    hp = {nm: s[nm] for nm in ("prior_sig", "momentum_decay", "nd", "Ninflate") if nm in s}
    return _args(lr=s["lr"], lr_head=s["lr_head"], momentum=s.get("momentum", 0.5), hparams=hp)


def _prescribe(S, grads_k, bs=8):
    """Feed the sampler prescribed gradients through update(): `gradients`
    returns step t's tensors (chains lo .. lo + K) instead of a backward."""
    t = [0]

    def gradients(x, y):
        g = {nm: v[t[0] % len(v)] for nm, v in grads_k.items()}
        t[0] += 1
        return g, torch.zeros(S.K, device=DEV), torch.zeros(S.K, bs, 5, device=DEV)
    S.gradients = gradients


@pytest.mark.parametrize("cls_name,family", [("StackedCSGHMC", "csghmc"), ("StackedSGLD", "sgld"),
                                             ("StackedCSGLD", "sgld")])
def test_sampler_chain_equals_a_one_chain_sampler_with_its_values(cls_name, family):
    """Two cycles over two epochs of four batches, prescribed gradients: chain
    k of the per_chain sampler equals a K = 1 sampler built with chain k's
    values and chain0 + k: theta, momentum and every collected moment."""
    from bayesdll_amd import stacked
    cls = getattr(stacked, cls_name)
    torch.manual_seed(3)
    net = Net().to(DEV)
    P = cls(net, 3, _args(), chain0=11, seed=5, graph=False, per_chain=SWEEP[family])
    st = P.state
    gen = torch.Generator(device=DEV).manual_seed(1)
    grads = {nm: [torch.randn(3, *s, device=DEV, generator=gen) * 0.1 for _ in range(8)]
             for nm, s in zip(st.names, st.shapes)}
    loader = [(torch.zeros(8, 13, device=DEV), torch.zeros(8, dtype=torch.long, device=DEV))] * 4
    _prescribe(P, grads)
    for ep in range(2):
        P.train_one_epoch(loader, ep)
    torch.cuda.synchronize()

    def moments(S):
        if hasattr(S, "mom1") and isinstance(S.mom1, dict):
            return {(c, i): m for c in S.mom1 for i, m in enumerate((S.mom1[c], S.mom2[c]))}
        return {(0, 0): S.m1, (0, 1): S.m2}
    assert moments(P) and all(m is not None for m in moments(P).values())
    for k in range(3):
        Q = cls(net, 1, _one_chain_args(family, k), chain0=11 + k, seed=5, graph=False)
        _prescribe(Q, {nm: [g[k:k + 1].contiguous() for g in v] for nm, v in grads.items()})
        for ep in range(2):
            Q.train_one_epoch(loader, ep)
        torch.cuda.synchronize()
        sl = lambda t: t.view(3, st.stride)[k].cpu().numpy()  # noqa: E731
        _assert_bits(sl(st.theta), Q.state.theta.cpu().numpy(), (cls_name, k, "theta"))
        if st.mom is not None and (family == "csghmc" or Q.mu != 0):
            _assert_bits(sl(st.mom), Q.state.mom.cpu().numpy(), (cls_name, k, "mom"))
        mq = moments(Q)
        assert set(mq) == set(moments(P))
        for key, m in moments(P).items():
            _assert_bits(sl(m), mq[key].cpu().numpy(), (cls_name, k, key))
        assert (P.step_count, P.draws) == (Q.step_count, Q.draws)
    assert not np.array_equal(st.theta2d[0].cpu().numpy(), st.theta2d[1].cpu().numpy())


def _loader(n, bs, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [(torch.randn(bs, 13, device=DEV, generator=g),
             torch.randint(0, 5, (bs,), device=DEV, generator=g)) for _ in range(n)]


def test_train_runs_end_to_end_and_evaluate_chains_scores_each_chain(tmp_path):
    """train() on a small MLP: finite per-chain results and a per-chain
    report; evaluate_chains equals a per-chain evaluation rebuilt in torch from
    the same components (the same draws: the draw counter is rewound), to 1e-6;
    a checkpoint continues bit for bit and a mismatched table is refused."""
    import torch.nn.functional as Fn
    from torch.func import functional_call
    from bayesdll_amd import stacked
    torch.manual_seed(4)
    args = _args()
    tr, te = _loader(4, 16, 1), _loader(2, 16, 2)
    sweep = {"lr": [5e-2, 1e-2, 3e-3], "prior_sig": [1.0, 0.3, 2.5]}
    P = stacked.StackedCSGHMC(Net().to(DEV), 3, args, chain0=2, seed=9, init="reinit", graph=False,
                              per_chain=sweep)
    hist = P.train(tr, te)
    assert len(hist) == 2 and all(np.isfinite(h["loss"]).all() for h in hist)
    last = hist[-1]
    assert len(last["chains"]["nll"]) == 3 and np.isfinite(last["chains"]["nll"]).all()
    assert last["best"] == int(np.argmin(last["chains"]["nll"]))
    assert not P.state.diverged_chains()
    # evaluate_chains against a plain per-chain torch evaluation of the same components
    d0 = P.draws
    nll, err = P.evaluate_chains(te)
    assert P.draws > d0
    P.draws = d0
    st, net = P.state, Net().to(DEV).eval()
    tot, wrong, nb = np.zeros(3), np.zeros(3), 0
    with torch.no_grad():
        for x, y in te:
            buf = torch.empty_like(st.theta)
            comps = []
            for _ in P._components(buf):
                b2 = buf.view(3, st.stride)
                comps.append(torch.stack([Fn.log_softmax(functional_call(
                    net, {nm: b2[k, o:o + n].view(s) for nm, o, n, s in
                          zip(st.names, st.offsets, st.numels, st.shapes)}, (x,)), -1)
                    for k in range(3)]))
            lp = torch.stack(comps).double().exp().mean(0).log()      # [K, B, C]
            for k in range(3):
                tot[k] += Fn.nll_loss(lp[k], y, reduction="sum").item()
                wrong[k] += lp[k].argmax(-1).ne(y).sum().item()
            nb += len(y)
    assert len(comps) >= 2
    print("evaluate_chains", nll.tolist(), (tot / nb).tolist())
    assert np.abs(nll - tot / nb).max() <= 1e-6 and np.array_equal(err, wrong / nb)
    # checkpoint: continue epoch 1 again from the state after epoch 0
    A = stacked.StackedCSGHMC(Net().to(DEV), 3, args, chain0=2, seed=9, init="reinit", graph=False,
                              per_chain=sweep)
    A.train_one_epoch(tr, 0)
    path = A.save_ckpt(str(tmp_path / "a.pt"))
    B = stacked.StackedCSGHMC(Net().to(DEV), 3, args, chain0=2, seed=9, graph=False,
                              per_chain=sweep)
    B.load_ckpt(path)
    for S in (A, B):
        S.train_one_epoch(tr, 1)
    torch.cuda.synchronize()
    _assert_bits(A.state.theta.cpu().numpy(), B.state.theta.cpu().numpy(), ("ckpt", "theta"))
    _assert_bits(A.state.mom.cpu().numpy(), B.state.mom.cpu().numpy(), ("ckpt", "mom"))
    for c_ in A.mom1:
        _assert_bits(A.mom1[c_].cpu().numpy(), B.mom1[c_].cpu().numpy(), ("ckpt", "m1", c_))
        _assert_bits(A.mom2[c_].cpu().numpy(), B.mom2[c_].cpu().numpy(), ("ckpt", "m2", c_))
    other = stacked.StackedCSGHMC(Net().to(DEV), 3, args, chain0=2, seed=9, graph=False,
                                  per_chain=dict(sweep, lr=[5e-2, 1e-2, 4e-3]))
    with pytest.raises(ValueError, match="per_chain table differs"):
        other.load_ckpt(path)


# ---------------------------------------------------------------------- 8. CLI
def test_cli_sweep(tmp_path):
    from bayesdll_amd.run import main
    hp = ("prior_sig=1.0,Ninflate=1.0,nd=0.01,burnin=0,momentum_decay=0.18,thin=1,"
          "bias=informative,nst=2")
    hist = main(["--method", "csghmc", "--dataset", "mnist", "--backbone", "mlp_mnist",
                 "--epochs", "2", "--num_cycles", "2", "--batch_size", "64", "--lr", "1e-2",
                 "--train_size", "256", "--test_size", "64", "--val_heldout", "0.25",
                 "--stacked_chains", "4", "--sweep", "lr=1e-2,5e-3,2e-3,1e-3", "--sweep",
                 "prior_sig=1.0,0.5,2.0,1.0", "--hparams", hp, "--log_dir", str(tmp_path)])
    assert len(hist) == 2 and all(np.isfinite(h["loss"]).all() for h in hist)
    text = next(tmp_path.rglob("logs.txt")).read_text()
    lines = [ln for ln in text.splitlines() if "(Epoch 1) chain " in ln]
    assert len(lines) == 4 and all("lr=" in ln and "prior_sig=" in ln and "loss = " in ln
                                   for ln in lines)
    assert "lr=0.005 prior_sig=0.5" in lines[1]
    assert "best chain by validation NLL: chain " in text
