"""Stacked-chain step launches (bdl_step_args.chain_groups) against the fp32
host reference, on every sweep path.

One launch updates K chains stacked in one buffer; noise_from
(bdl_kernels.hpp) splits each float4 group into (chain, group within chain)
and keys chain k as chain + k.  That split is compiled into every Philox step
instance, which read its inputs held in SGPRs, per call through the kernarg
pointer, through the re-read argument view, or inside the Adam sweep's
software pipeline.  Here every one of them runs it on stacked tables
(tests/stacked_tables.py; tests/test_stacked_tables_host.py proves which paths
each table reaches):

  A         3 chains of the 39,426-element table of test_gpu_noise_units.py,
            padded (stride 39,428), flat gradient: fast, multi-run and guarded
            iterations inside the chains (at depth 4 chain 0 owns no multi-run
            one: table C covers it), every chain at another lane phase;
  B         5 chains of one tensor, no padding, one run: the seams lie inside
            fast-path iterations, lanes of one wave in different chains;
  C         6 chains of a body and a head tensor, no padding: the seams lie
            inside multi-run iterations;
  A-tensor  table A with one [K, numel] gradient allocation per tensor, runs
            and bases formed by StackedState._build_table.

Expectation: for chain k, tests/step_ref.py applied to that chain's slot of
`stride` elements (padding included, as SKIP elements), with eps =
K.philox_normal(stride, SEED, CHAIN + k, STEP) read back from the device.
That stream is pinned to philox_ref by test_gpu_noise_stream.py, and
test_gpu_noise_units.py establishes that a Philox step equals the
buffer-noise step fed it, so the comparison is bit for bit, as int32 patterns
over all K * stride elements of every vector (NaN positions as NaN-ness).
After every launch: vectors it must not write are unchanged, frozen elements
and the padding (pre-filled with 7.0) are untouched, the nonfinite flag is 0;
m1 / m2 of a SKIP element are what the reference's collect gives (it reads
the unchanged theta); a first step stores +0 in the SGD buffer of every SKIP
element, the padding included (test_gpu_step_reference._first_buf).

No tolerance is added here.  The two in use are imported or cited: each
chain's device stream within test_gpu_noise_stream.TOL of
philox_ref.normals(stride, SEED, CHAIN + k, STEP) (the chains really carry
ids CHAIN + k), and the clipped step's norm within one fp32 ulp of
fl32(sqrt(S)), derived in test_gpu_step_reference.py's docstring.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import philox_ref as P
import stacked_tables as T
import step_ref as R
from test_gpu_noise_stream import TOL, _dist
from test_gpu_noise_units import (CHAIN, FROZEN, SEED, STEP, VECTORS, WRITTEN, Table, _SCALE)
from test_gpu_step_reference import (COLLECTS, VARIANTS, _accepted, _assert_bits, _expected,
                                     _first_buf, _scalars)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32

GEOMETRIES = [(1, 1, 1), (1, 2, 1), (1, 4, 1), (2, 4, 0)]
SENTINEL = F(7.0)  # the padding's start value in every vector (finite: the guarded
#                    path's divergence guard looks at every lane's theta)
NONE, WELFORD_INIT, WELFORD, MEAN_INIT, MEAN = COLLECTS[:5]


# ------------------------------------------------------------------ plumbing
class Stack:
    """The flat vectors of K stacked chains over a stacked_tables.Layout and
    launchable states (what kernels._step_args reads, chain_groups set)."""

    def __init__(self, lay, rng_seed):
        from bayesdll_amd import kernels as K
        self.lay = lay
        self.attr = np.tile(lay.slot_attr(), lay.K)
        self.skip = (self.attr & R.ATTR_SKIP) != 0
        self.pad = np.tile(np.arange(lay.stride) >= lay.n1, lay.K)
        assert int(self.pad.sum()) == lay.K * (lay.stride - lay.n1) and self.skip[self.pad].all()
        rng = np.random.default_rng(rng_seed)
        self.h0 = {}
        for nm in VECTORS:
            x = rng.standard_normal(lay.n).astype(F) * F(_SCALE[nm])
            x = np.abs(x) if nm in ("m2", "adam_v") else x
            x[self.pad] = SENTINEL
            self.h0[nm] = x
        self.v = {nm: torch.from_numpy(x).to(DEV) for nm, x in self.h0.items()}
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=DEV)
        # the expectation's noise: chain k's device stream, keyed CHAIN + k
        self.eps = np.concatenate([K.philox_normal(lay.stride, SEED, CHAIN + k, STEP, device=DEV)
                                   .cpu().numpy() for k in range(lay.K)])
        self.h = dict(self.h0, noise=self.eps)
        self._states, self._exp = {}, {}

    def state(self, lo=0, hi=None):
        """A launchable state over elements [lo, hi), its run table built as
        test_gpu_noise_units.Table.state builds a sub-range's."""
        hi = self.lay.n if hi is None else hi
        st = self._states.get((lo, hi))
        if st is None:
            runs = self.lay.flat_runs(lo, hi).to(DEV)
            v = {nm: t[lo:hi] for nm, t in self.v.items()}
            st = SimpleNamespace(theta=v["theta"], grad=v["grad"], gbase=None, mom=v["mom"],
                                 prior=v["prior"], noise=v["noise"], runs=runs,
                                 nruns=int(runs.shape[0]), n=hi - lo, device=torch.device(DEV, 0),
                                 nonfinite=self.nonfinite, timer=None, v=v,
                                 chain_groups=self.lay.chain_groups)
            self._states[(lo, hi)] = st
        return st

    def tensor_state(self):
        """The whole stack with every tensor's gradient in one [K, numel]
        allocation of its own (as vmap leaves them), runs and bases formed by
        StackedState._build_table itself."""
        from bayesdll_amd.stacked import StackedState
        lay = self.lay
        g2 = self.h0["grad"].reshape(lay.K, lay.stride)
        grads, ptrs = [], []
        for nm, o, k in zip(lay.names, lay.offsets, lay.numels):
            if nm == FROZEN:
                grads.append(None)
                ptrs.append(0)
                continue
            g = torch.from_numpy(np.ascontiguousarray(g2[:, o:o + k])).to(DEV)
            grads.append(g)
            ptrs.append(g.data_ptr())
        ss = StackedState.__new__(StackedState)
        ss.K, ss.offsets, ss.numels, ss.attrs = lay.K, lay.offsets, lay.numels, lay.attrs
        ss.stride, ss.n1, ss.device = lay.stride, lay.n1, torch.device(DEV, 0)
        runs, nruns, gbase = ss._build_table(ptrs)
        st = SimpleNamespace(**vars(self.state()))
        st.grad, st.runs, st.nruns, st.gbase, st.tensor_grads = None, runs, nruns, gbase, grads
        return st

    def load(self):
        for nm in VECTORS:
            self.v[nm].copy_(torch.from_numpy(self.h0[nm]))
        self.nonfinite.zero_()

    def expected(self, case, ck, mode, clip_coef=None):
        """The vectors the launch writes: the host reference applied chain by
        chain to the chain's slot, with the chain's own stream.  Cached (it
        does not depend on the launch geometry)."""
        key = (case, ck, mode, None if clip_coef is None else int(F(clip_coef).view(np.int32)))
        if key not in self._exp:
            lay, parts = self.lay, []
            for k in range(lay.K):
                sl = slice(k * lay.stride, (k + 1) * lay.stride)
                hk = {nm: x[sl] for nm, x in self.h.items()}
                parts.append(_expected(VARIANTS[case], hk, lay.slot_attr(), mode, ck,
                                       clip_coef=clip_coef))
            self._exp[key] = {nm: np.concatenate([p[nm] for p in parts]) for nm in parts[0]}
        return self._exp[key]


_S = {}


def _stack(name):
    if name not in _S:
        lay, seed = {"A": (T.table_a, 611), "B": (T.table_b, 612), "C": (T.table_c, 613)}[name]
        _S[name] = Stack(lay(), seed)
    return _S[name]


def _launch(st, v, mode, ck, philox_offset=0, max_norm=None):
    """One NOISE_PHILOX launch of the variant over `st`, keyed (SEED, CHAIN,
    STEP); max_norm: the clipped SGLD step (returns its workspace)."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    assert v.noise
    kw = dict(v.kw)
    kind, has_m2, ca, cb = ck
    if kind != "NONE":
        kw.update(collect=getattr(L, "COLLECT_" + kind), mom1=st.v["m1"],
                  mom2=st.v["m2"] if has_m2 else None, collect_a=ca, collect_b=cb)
    kw.update(noise_mode=L.NOISE_PHILOX, div_mode=mode, seed=SEED, chain=CHAIN, step=STEP,
              philox_offset=philox_offset)
    if max_norm is not None:
        return K.sgld_step_clipped(st, max_norm, **kw)
    method = getattr(L, v.method)
    if v.family == "adam":
        K.adam_step(st, method, adam_m=st.v["adam_m"], adam_v=st.v["adam_v"],
                    sgd_buf=st.v["sgd_buf"] if v.mom else None, **kw)
    else:
        K.sgmcmc_step(st, method, **kw)
    return None


def _check(s, exp, what, first_buf=None):
    """Every vector over all K * stride elements against the expectation (the
    start values where the launch writes nothing); SKIP elements — the frozen
    tensor and the padding — as they were (first_buf: +0 there; m1 / m2: the
    collect reads the unchanged theta, compared above); the flag 0."""
    torch.cuda.synchronize()
    got = {nm: s.v[nm].cpu().numpy() for nm in VECTORS}
    h = s.h0
    for nm in VECTORS:
        _assert_bits(got[nm], exp.get(nm, h[nm]), what + (nm,))
    for nm in WRITTEN:
        if nm == first_buf:
            assert not got[nm][s.skip].view(np.int32).any(), what + (nm, "skip")
        elif nm not in ("m1", "m2"):
            _assert_bits(got[nm][s.skip], h[nm][s.skip], what + (nm, "skip"))
            assert (got[nm][s.pad] == SENTINEL).all(), what + (nm, "padding")
    assert int(s.nonfinite.item()) == 0, what


def _changes_something(s, exp):
    return any(not np.array_equal(exp[nm].view(np.int32), s.h0[nm].view(np.int32)) for nm in exp)


# ------------------------------------------------------------------ the stream
@pytest.mark.parametrize("table", ["A", "B", "C"])
def test_each_chain_carries_its_own_reference_checked_stream(table):
    """The eps of the expectations: chain k's device stream is within the
    stream test's bound of philox_ref's (SEED, CHAIN + k, STEP) stream."""
    s = _stack(table)
    lay = s.lay
    for k in range(lay.K):
        dev = s.eps[k * lay.stride:(k + 1) * lay.stride].astype(np.float64)
        d = _dist(dev, P.normals(lay.stride, SEED, CHAIN + k, STEP))
        print(f"table {table} chain {k}: max distance {d.max():.3e}; bound {TOL:.3e}")
        assert d.max() <= TOL, (table, k, int(d.argmax()))


def test_chains_are_distinct():
    """The expectation depends on k: from EQUAL inputs, chain 0's and chain
    1's stream give different theta, and so do the two slots of table B."""
    s = _stack("B")
    lay, v = s.lay, VARIANTS["csghmc_noise"]
    h0 = {nm: x[:lay.stride] for nm, x in s.h.items()}
    h1 = dict(h0, noise=s.eps[lay.stride:2 * lay.stride])
    e0 = _expected(v, h0, lay.slot_attr(), "true", NONE)
    e1 = _expected(v, h1, lay.slot_attr(), "true", NONE)
    assert (e0["theta"].view(np.int32) != e1["theta"].view(np.int32)).any()
    exp = s.expected("csghmc_noise", NONE, "true")["theta"].reshape(lay.K, lay.stride)
    _assert_bits(exp[0], e0["theta"], ("chain 0",))
    assert (exp[0].view(np.int32) != exp[1].view(np.int32)).any()


# ------------------------------------------------------------ matrix, table A
A_CASES = ["csghmc_noise", "sgld_no_momentum", "sgld_first", "sgld_later", "sgld_grad", "sghmc",
           "sghmc_grad", "adam_no_buffer", "adam_later", "adam_csghmc_later", "adam_grad"]


def _collects(case):
    """NONE, the init and the steady kind of the family (Welford for cSGHMC,
    MEAN for the rest, WELFORD as well for sgld_later and sghmc), less what
    the C-ABI rejects."""
    v = VARIANTS[case]
    cks = [NONE] + ([WELFORD_INIT, WELFORD] if v.family == "csghmc" else [MEAN_INIT, MEAN])
    if case in ("sgld_later", "sghmc"):
        cks.append(WELFORD)
    return [ck for ck in cks if _accepted(v, ck)]


@pytest.mark.parametrize("case", A_CASES)
def test_padded_stack_matches_the_host_reference(case):
    from bayesdll_amd import kernels as K
    v, s = VARIANTS[case], _stack("A")
    st = s.state()
    assert st.chain_groups == 9857 and st.n == 118284
    launches = 0
    try:
        for ck in _collects(case):
            for mode, geos in (("true", GEOMETRIES), ("recip", [(1, 4, 1)])):
                exp = s.expected(case, ck, mode)
                assert _changes_something(s, exp), (case, ck)
                for geo in geos:
                    s.load()
                    K.set_launch_config(*geo)
                    _launch(st, v, mode, ck)
                    _check(s, exp, (case, ck[:2], mode, geo), _first_buf(v))
                    launches += 1
    finally:
        K.set_launch_config(0, 0, 0)
    assert launches == 5 * len(_collects(case))


# ------------------------------------------- matrix, tables B, C and A-tensor
REPRESENTATIVES = [("csghmc_noise", (NONE, WELFORD)), ("sgld_later", (MEAN,)), ("sgld_grad", (NONE,)),
                   ("sghmc", (NONE,)), ("adam_later", (NONE, MEAN)), ("adam_grad", (NONE,))]


@pytest.mark.parametrize("case,cks", REPRESENTATIVES, ids=[c for c, _ in REPRESENTATIVES])
@pytest.mark.parametrize("table", ["B", "C"])
def test_seamless_stacks_match_the_host_reference(table, case, cks):
    """B: the seams inside fast-path iterations (one run); C: inside
    multi-run iterations."""
    from bayesdll_amd import kernels as K
    v, s = VARIANTS[case], _stack(table)
    st = s.state()
    assert not s.pad.any() and (table != "B" or st.nruns == 1)
    try:
        for ck in cks:
            exp = s.expected(case, ck, "true")
            assert _changes_something(s, exp), (case, ck)
            for geo in GEOMETRIES:
                s.load()
                K.set_launch_config(*geo)
                _launch(st, v, "true", ck)
                _check(s, exp, (table, case, ck[:2], geo), _first_buf(v))
    finally:
        K.set_launch_config(0, 0, 0)


@pytest.mark.parametrize("case,cks", REPRESENTATIVES, ids=[c for c, _ in REPRESENTATIVES])
def test_per_tensor_gradients_of_stacked_chains(case, cks):
    """Table A with every tensor's gradients of all chains in one [K, numel]
    allocation, read (and for *_GRAD written) through the per-run bases of
    StackedState._build_table; some bases are not 16-byte addressable."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    v, s = VARIANTS[case], _stack("A")
    lay = s.lay
    try:
        for ck in cks:
            exp = s.expected(case, ck, "true")
            want_g = exp.get("grad", s.h0["grad"]).reshape(lay.K, lay.stride)
            flat_exp = {nm: x for nm, x in exp.items() if nm != "grad"}
            for geo in GEOMETRIES:
                s.load()
                st = s.tensor_state()
                rows = st.runs.tolist()
                assert st.nruns == lay.K * (len(lay.names) + 1) == len(rows)
                assert any(r[1] & L.ATTR_GUNALIGNED for r in rows)
                assert [r[0] for r in rows if r[1] == L.ATTR_SKIP] == \
                    [(k + 1) * lay.stride for k in range(lay.K)]  # the padding runs
                K.set_launch_config(*geo)
                _launch(st, v, "true", ck)
                _check(s, flat_exp, ("tensor", case, ck[:2], geo))  # the flat grad vector: untouched
                for nm, o, k, g in zip(lay.names, lay.offsets, lay.numels, st.tensor_grads):
                    if g is not None:
                        _assert_bits(g.cpu().numpy(), np.ascontiguousarray(want_g[:, o:o + k]),
                                     ("tensor", case, ck[:2], geo, nm))
    finally:
        K.set_launch_config(0, 0, 0)


# --------------------------------------------------- split launch with an offset
@pytest.mark.parametrize("case", ["csghmc_noise", "sgld_later", "sghmc", "adam_later"])
def test_split_stacked_launch_with_philox_offset(case):
    """Two launches split at the 4-aligned run boundary after l6.bias inside
    chain 1 (neither on a seam nor at the start), the second with
    philox_offset = split / 4, the same chain_groups and chain = CHAIN: the
    single launch's expectation, bit for bit (plain step and steady collect,
    depths 1 and 4)."""
    from bayesdll_amd import kernels as K
    v, s = VARIANTS[case], _stack("A")
    lay = s.lay
    split = lay.stride + Table().split
    assert split % 4 == 0 and lay.stride < split < 2 * lay.stride
    assert split in [o for o, _, _ in lay.stacked_segments()]
    lo, hi = s.state(0, split), s.state(split, lay.n)
    assert lo.chain_groups == hi.chain_groups == lay.chain_groups
    try:
        for ck in (NONE, WELFORD if v.family == "csghmc" else MEAN):
            exp = s.expected(case, ck, "true")
            for geo in ((1, 1, 1), (1, 4, 1)):
                s.load()
                K.set_launch_config(*geo)
                _launch(lo, v, "true", ck)
                _launch(hi, v, "true", ck, philox_offset=split // 4)
                _check(s, exp, ("split", case, ck[:2], geo), _first_buf(v))
    finally:
        K.set_launch_config(0, 0, 0)


# -------------------------------------------------------------------- clipping
@pytest.mark.parametrize("max_norm", [1.0, 1e6], ids=["active", "inactive"])
def test_clipped_sgld_over_stacked_chains(max_norm):
    """The norm is over all K chains' live elements: within one fp32 ulp of
    fl32(sqrt(S)), S the float64 sum of squares of the reference's fp32
    sampler gradient (the tolerance derived in test_gpu_step_reference.py's
    docstring); the coefficient from the device's own norm and the step with
    that coefficient, bit for bit."""
    from bayesdll_amd import kernels as K
    v, s = VARIANTS["sgld_later"], _stack("A")
    st = s.state()
    live = ~s.skip
    try:
        for mode in ("true", "recip"):
            sc, _ = _scalars(v, NONE)
            gp = R.sgld_grad(s.h["theta"], s.h["prior"], s.h["grad"], s.attr, sc, s.h["noise"], mode)
            norm_ref = F(np.sqrt(float(np.sum(gp[live].astype(np.float64) ** 2))))
            for geo in GEOMETRIES:
                s.load()
                K.set_launch_config(*geo)
                ws = _launch(st, v, mode, NONE, max_norm=max_norm)
                torch.cuda.synchronize()
                norm, coef = (F(x) for x in ws[:2].cpu().numpy())
                print("stacked clip", mode, geo, float(norm), float(norm_ref), float(coef))
                assert abs(int(norm.view(np.int32)) - int(norm_ref.view(np.int32))) <= 1, (mode, geo)
                assert coef.view(np.int32) == F(R.clip_coef(norm, max_norm)).view(np.int32), (mode, geo)
                assert (coef < 1.0) == (max_norm == 1.0)
                exp = s.expected("sgld_later", NONE, mode, clip_coef=coef)
                _check(s, exp, ("clipped", max_norm, mode, geo))
    finally:
        K.set_launch_config(0, 0, 0)
