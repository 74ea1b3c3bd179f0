"""bdl_chain_diag on the GPU: the device's pooled mean / variance and R-hat
equal the fp32 host reference (tests/chain_diag_ref.py) bit for bit, the
summary's counts, maximum and argmax equal the reference's exactly and do not
depend on the launch geometry, nothing outside [0, n) of an output or outside
the workspace is written, the padding of a chain slot is never read, and the
stacked samplers' diagnostics() is that kernel on their own moments."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import chain_diag_ref as R

pytestmark = pytest.mark.gpu

OUTPUTS = ("pooled_mean", "pooled_var", "rhat")
COUNT = 6
# (var_mode, ratio, recip): all three variance forms, Welford both with the
# reciprocal (torch-on-GPU rounding) and with the division
MODES = [(R.VAR_GIVEN, 1.0, False), (R.VAR_RAW_MOMENTS, 1.2, False),
         (R.VAR_WELFORD, 5.0, True), (R.VAR_WELFORD, 5.0, False)]
EXACT = ("n_eval", "n_degenerate", "n_nonfinite", "n_above", "rhat_max", "argmax")


def bits(a):
    """int32 patterns with every NaN mapped to one pattern (NaN as NaN-ness)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def case(seed, K_, n, var_mode, ratio, chain_groups=None):
    m1, var, cg = R.make_case(seed, K_, n, chain_groups=chain_groups)
    return m1, R.to_mode(m1, var, var_mode, ratio, K_, 4 * cg, n), cg


def device_diag(m1, m2, *, K_, cg, n, var_mode, ratio, recip, want=OUTPUTS, bpc=0, **kw):
    from bayesdll_amd import kernels as K
    d1, d2 = torch.from_numpy(m1).cuda(), torch.from_numpy(m2).cuda()
    res = K.chain_diag(d1, d2, chains=K_, chain_groups=cg, n=n, var_mode=var_mode, ratio=ratio,
                       count=COUNT, want=want, blocks_per_cu=bpc,
                       div_mode="recip" if recip else "true", **kw)
    return res, d1, d2


def reference(m1, m2, *, K_, cg, n, var_mode, ratio, recip, **kw):
    inv = R.inv_of(ratio) if recip else 0.0
    return R.chain_diag_f32(m1, m2, chains=K_, chain_groups=cg, n=n, var_mode=var_mode,
                            ratio=ratio, inv_ratio=inv, count=COUNT, **kw)


def check_summary(got, want, n):
    for f in EXACT:
        assert got[f] == want[f], (f, got[f], want[f])
    assert abs(got["rhat_sum"] - want["rhat_sum"]) <= n * 2.0 ** -52 * abs(want["rhat_sum"])
    ne = want["n_eval"]
    if ne:
        assert got["rhat_mean"] == got["rhat_sum"] / ne
        assert got["share_above"] == [v / ne for v in want["n_above"]]


# n: one element; fewer than one float4 group... one workgroup; several
# workgroups with an element tail (4099 = 5 workgroups, 39427 = 39, both
# n % 4 == 3); and a chain slot larger than n needs
@pytest.mark.parametrize("n,chain_groups", [(1, None), (7, None), (4099, None), (39427, None),
                                            (1026, 300)])
def test_outputs_equal_the_fp32_reference_bit_for_bit(n, chain_groups):
    """K = 2 .. 9 walks the chain loop's peeled first chain, its remainder
    alone (K - 1 = 1, 2, 3), one unrolled batch (4) and two (8); every
    variance form; three geometries; each output alone and all together.
    The slot padding holds NaN: it reaches no result."""
    for K_ in (2, 3, 4, 5, 9):
        for mi, (var_mode, ratio, recip) in enumerate(MODES):
            m1, m2, cg = case(100 * K_ + mi, K_, n, var_mode, ratio, chain_groups)
            kw = dict(K_=K_, cg=cg, n=n, var_mode=var_mode, ratio=ratio, recip=recip)
            pm, pv, rh, summ = reference(m1, m2, **kw)
            assert summ["n_nonfinite"] == 0 and summ["n_eval"] + summ["n_degenerate"] == n
            want = dict(zip(OUTPUTS, (bits(pm), bits(pv), bits(rh))))
            for bpc in (1, 2, 8):
                res, d1, d2 = device_diag(m1, m2, bpc=bpc, **kw)
                for w in OUTPUTS:
                    assert res[w].shape == (n,)
                    assert np.array_equal(bits(res[w].cpu().numpy()), want[w]), (K_, mi, bpc, w)
                check_summary(res.summary, summ, n)
                assert np.array_equal(bits(d1.cpu().numpy()), bits(m1))   # inputs untouched
                assert np.array_equal(d1.cpu().numpy().view(np.int32), m1.view(np.int32))
                assert np.array_equal(d2.cpu().numpy().view(np.int32), m2.view(np.int32))
            if mi == K_ % len(MODES):  # each output requested alone, and none at all
                for w in OUTPUTS:
                    res, _, _ = device_diag(m1, m2, want=(w,), **kw)
                    assert list(res) == [w]
                    assert np.array_equal(bits(res[w].cpu().numpy()), want[w]), (K_, mi, w)
                    check_summary(res.summary, summ, n)
                res, _, _ = device_diag(m1, m2, want=(), **kw)
                assert list(res) == []
                check_summary(res["summary"], summ, n)


def test_summary_is_exact_and_independent_of_the_geometry():
    """A vector large enough that 1, 2 and 8 workgroups per CU are different
    grids (and a workgroup sweeps several iterations), with a planted tie for
    the maximum: counts, maximum and argmax (the lowest index) are the
    reference's in every geometry; rhat_sum within n 2^-52 of math.fsum."""
    n, K_ = 1_000_003, 3
    var_mode, ratio, recip = MODES[1]
    m1, m2, cg = case(7, K_, n, var_mode, ratio)
    kw = dict(K_=K_, cg=cg, n=n, var_mode=var_mode, ratio=ratio, recip=recip)
    rh = reference(m1, m2, **kw)[2]
    i = int(np.nanargmax(rh))
    j = (i + n // 2) % n
    for k in range(K_):  # element j becomes a copy of the maximum's element
        m1[4 * cg * k + j] = m1[4 * cg * k + i]
        m2[4 * cg * k + j] = m2[4 * cg * k + i]
    pm, pv, rh, summ = reference(m1, m2, **kw)
    assert rh[i] == rh[j] == summ["rhat_max"] and summ["argmax"] == min(i, j)
    assert summ["n_above"][0] > summ["n_above"][1] > summ["n_above"][2] > 0
    seen = []
    for bpc in (1, 2, 8):
        res, _, _ = device_diag(m1, m2, bpc=bpc, **kw)
        assert np.array_equal(bits(res["rhat"].cpu().numpy()), bits(rh)), bpc
        assert np.array_equal(bits(res["pooled_mean"].cpu().numpy()), bits(pm)), bpc
        assert np.array_equal(bits(res["pooled_var"].cpu().numpy()), bits(pv)), bpc
        check_summary(res.summary, summ, n)
        seen.append({f: res.summary[f] for f in EXACT})
    assert seen[0] == seen[1] == seen[2]


def test_planted_degenerate_nonfinite_and_threshold_elements():
    """Frozen elements (bit-equal across chains) are degenerate: rhat NaN, out
    of the statistics, pooled_* still right.  var_floor = 0 with zero variance
    in every chain: counted in n_nonfinite.  A value exactly on a threshold is
    not above it."""
    n, K_ = 4099, 5
    m1, m2, cg = case(11, K_, n, R.VAR_GIVEN, 1.0)
    slot = 4 * cg
    frozen, zerovar = [0, 5, 1023, 1024, 4098], [3, 2048, 4097]
    for k in range(K_):
        for j in frozen:
            m1[slot * k + j] = m1[j]
        for j in zerovar:
            m2[slot * k + j] = 0.0
    kw = dict(K_=K_, cg=cg, n=n, var_mode=R.VAR_GIVEN, ratio=1.0, recip=False)
    rh0 = reference(m1, m2, var_floor=0.0, **kw)[2]
    srt = np.sort(rh0[np.isfinite(rh0)])
    thr = tuple(float(srt[int(q * srt.size)]) for q in (0.25, 0.5, 0.9))
    pm, pv, rh, summ = reference(m1, m2, var_floor=0.0, thresholds=thr, **kw)
    assert summ["n_degenerate"] == len(frozen) and summ["n_nonfinite"] == len(zerovar)
    assert np.isnan(rh[frozen]).all() and np.isinf(rh[zerovar]).all()
    for t, above in zip(thr, summ["n_above"]):
        assert (rh == np.float32(t)).sum() >= 1                  # the value sits on it
        assert above == int((rh[np.isfinite(rh)] > np.float32(t)).sum())
    res, _, _ = device_diag(m1, m2, var_floor=0.0, thresholds=thr, **kw)
    got = res["rhat"].cpu().numpy()
    assert np.isnan(got[frozen]).all() and np.isinf(got[zerovar]).all()
    for w, ref in zip(OUTPUTS, (pm, pv, rh)):
        assert np.array_equal(bits(res[w].cpu().numpy()), bits(ref)), w
    assert np.array_equal(res["pooled_mean"].cpu().numpy()[frozen], m1[frozen])
    check_summary(res.summary, summ, n)
    assert res.summary["n_eval"] == n - len(frozen) - len(zerovar)
    # everything frozen: nothing evaluated, the empty conventions
    for k in range(1, K_):
        m1[slot * k: slot * k + n] = m1[:n]
    res, _, _ = device_diag(m1, m2, **kw)
    s = res.summary
    assert (s["n_eval"], s["n_degenerate"], s["n_nonfinite"]) == (0, n, 0)
    assert (s["rhat_max"], s["argmax"], s["rhat_sum"], s["n_above"]) == (0.0, -1, 0.0, [0, 0, 0])
    assert math.isnan(s["rhat_mean"]) and torch.isnan(res["rhat"]).all()


@pytest.mark.parametrize("n", [1, 7, 4099])
def test_nothing_outside_the_outputs_and_the_workspace_is_written(n):
    """The C entry point on sub-ranges of sentinel-filled allocations: every
    byte outside [0, n) of each output and outside
    bdl_chain_diag_workspace_bytes(n) of the workspace is unchanged."""
    from bayesdll_amd import _lib as L
    h = L.lib()
    K_ = 3
    var_mode, ratio, recip = MODES[2]
    m1, m2, cg = case(21, K_, n, var_mode, ratio)
    pm, pv, rh, summ = reference(m1, m2, K_=K_, cg=cg, n=n, var_mode=var_mode, ratio=ratio,
                                 recip=recip)
    d1, d2 = torch.from_numpy(m1).cuda(), torch.from_numpy(m2).cuda()
    SENT = 0x7F
    lead = 64                                            # floats before each output
    span = lead + (n + 3) // 4 * 4 + 64
    outs = torch.full((3 * span * 4,), SENT, dtype=torch.uint8, device="cuda")
    wsb = int(h.bdl_chain_diag_workspace_bytes(n))
    ws = torch.full((256 + wsb + 256,), SENT, dtype=torch.uint8, device="cuda")
    a = L.DiagArgs()
    a.mom1, a.mom2 = d1.data_ptr(), d2.data_ptr()
    base = outs.data_ptr()
    a.pooled_mean, a.pooled_var, a.rhat = (base + 4 * (i * span + lead) for i in range(3))
    a.workspace = ws.data_ptr() + 256
    a.n, a.chain_groups, a.chains, a.var_mode = n, cg, K_, var_mode
    a.ratio, a.inv_ratio, a.var_floor = ratio, 1.0 / ratio, 1e-12
    a.c1 = (COUNT - 1) / COUNT
    for i, t in enumerate(R.THRESHOLDS):
        a.thresholds[i] = t
    L.check(h.bdl_chain_diag(a, L.current_stream_handle(torch.device("cuda"))), "bdl_chain_diag")
    torch.cuda.synchronize()
    ho, hw = outs.cpu().numpy(), ws.cpu().numpy()
    for i, ref in enumerate((pm, pv, rh)):
        lo = 4 * (i * span + lead)
        assert np.array_equal(bits(ho[lo: lo + 4 * n].view(np.float32)), bits(ref)), i
        assert (ho[4 * i * span: lo] == SENT).all() and (ho[lo + 4 * n: 4 * (i + 1) * span] == SENT).all()
    assert (hw[:256] == SENT).all() and (hw[256 + wsb:] == SENT).all()
    s = L.DiagSummary.from_buffer_copy(hw[256: 256 + C.sizeof(L.DiagSummary)].tobytes())
    assert (s.n_eval, s.n_degenerate, s.argmax) == (summ["n_eval"], summ["n_degenerate"],
                                                    summ["argmax"])
    assert s.rhat_max == summ["rhat_max"]


# ---------------------------------------------------------------- samplers
class Net(nn.Module):
    readout_name = "head"

    def __init__(self):  # 13*7+7+7*5+5 = 138: n % 4 != 0, stride 140
        super().__init__()
        self.body = nn.Linear(13, 7)
        self.head = nn.Linear(7, 5)

    def forward(self, x):
        return self.head(torch.tanh(self.body(x)))


def _args(nst=2, **extra):
    a = SimpleNamespace(
        lr=5e-2, lr_head=1e-1, epochs=2, num_cycles=2, proportion_exploration=0.5, ND=128,
        device="cuda", seed=7, momentum=0.5,
        hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0, "nd": 1.0,
                 "thin": 1, "nst": nst, "bias": "informative", "burnin": 0})
    for k, v in extra.items():
        setattr(a, k, v)
    return a


@pytest.fixture(scope="module")
def loader():
    g = torch.Generator().manual_seed(8)
    xs, ys = torch.randn(128, 13, generator=g), torch.randint(0, 5, (128,), generator=g)
    return [(xs[i:i + 16].cuda(), ys[i:i + 16].cuda()) for i in range(0, 128, 16)]


def _owned(S):
    """Everything the sampler owns on the device, cloned."""
    st = S.state
    t = {"theta": st.theta, "mom": st.mom, "prior": st.prior}
    if hasattr(S, "mom1"):
        t.update({f"mom1[{c}]": v for c, v in S.mom1.items()})
        t.update({f"mom2[{c}]": v for c, v in S.mom2.items()})
    t.update({"m1": getattr(S, "m1", None), "m2": getattr(S, "m2", None)})
    return {k: v.clone() for k, v in t.items() if v is not None}


@pytest.mark.parametrize("cls", ["StackedSGLD", "StackedCSGHMC"])
def test_sampler_diagnostics_is_the_kernel_on_its_own_moments(cls, loader):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    from bayesdll_amd import stacked
    from bayesdll_amd._runner import EVAL_STEP_BASE
    torch.manual_seed(11)
    S = getattr(stacked, cls)(Net().cuda(), 4, _args(), init="reinit", seed=4, chain0=3,
                              graph=False)
    with pytest.raises(ValueError, match="nothing is collected"):
        S.diagnostics()
    S.train_one_epoch(loader, 0)           # well past the first two collects
    st = S.state
    comp = S._latest_component()
    m1, m2, var_mode, ratio, count = S._moment_spec(comp)
    if cls == "StackedSGLD":
        assert (comp, count, var_mode) == (0, 1 + len(loader), L.VAR_RAW_MOMENTS)
    else:
        assert count == S.samples_per_cycle[comp] // 2 >= 2 and var_mode == L.VAR_WELFORD
    before = _owned(S)
    d = S.diagnostics(rhat=True, pooled=True)
    torch.cuda.synchronize()
    after = _owned(S)
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
    recip = K.DIV_MODE == "recip"
    pm, pv, rh, summ = R.chain_diag_f32(
        m1.cpu().numpy(), m2.cpu().numpy(), chains=4, chain_groups=st.chain_groups, n=st.n1,
        var_mode=var_mode, ratio=ratio, inv_ratio=R.inv_of(ratio) if recip else 0.0, count=count)
    for w, ref in zip(OUTPUTS, (pm, pv, rh)):
        assert d[w].shape == (st.n1,)
        assert np.array_equal(bits(d[w].cpu().numpy()), bits(ref)), w
    check_summary(d, summ, st.n1)
    assert d["n_eval"] == st.n1 and d["component"] == comp and d["count"] == count
    assert d["argmax_param"] == S.param_of(summ["argmax"]) and d["argmax_param"] in st.names
    assert set(S.diagnostics()) & set(OUTPUTS) == set()
    # the draw is the spec's draw, before and after the _components refactor
    d0 = S.draws
    want = torch.empty_like(st.theta)
    K.posterior_sample(want, m1, m2, var_mode=var_mode, ratio=ratio, seed=S.seed, chain=S.chain0,
                       step=EVAL_STEP_BASE + d0, chain_groups=st.chain_groups)
    got = torch.full_like(st.theta, float("nan"))
    S._sample(got, m1, m2, var_mode, ratio)
    assert S.draws == d0 + 1
    comp_buf = torch.full_like(st.theta, float("nan"))
    S.draws = d0
    gen = S._components(comp_buf)
    assert next(gen) == sorted(getattr(S, "mom1", {0: None}))[0]
    if cls == "StackedSGLD":
        assert torch.equal(comp_buf.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    gen.close()


def test_sampler_diagnostics_refusals(loader):
    from bayesdll_amd import stacked
    torch.manual_seed(12)
    S = stacked.StackedSGLD(Net().cuda(), 2, _args(), graph=False)
    S.seed_moments()                                        # one sample per chain
    with pytest.raises(ValueError, match="at least 2"):
        S.diagnostics()
    S0 = stacked.StackedSGLD(Net().cuda(), 2, _args(nst=0), init="reinit", graph=False)
    S0.train_one_epoch(loader[:3], 0)
    assert S0.cnt == 4 and S0.m2 is None
    with pytest.raises(ValueError, match="second moment is not kept"):
        S0.diagnostics()
    S1 = stacked.StackedSGLD(Net().cuda(), 1, _args(), graph=False)
    S1.train_one_epoch(loader[:3], 0)
    with pytest.raises(ValueError, match="K = 1"):
        S1.diagnostics()


def test_train_reports_rhat_only_when_asked(loader):
    from bayesdll_amd import stacked

    class Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(msg)

    def run(**extra):
        torch.manual_seed(13)
        log = Log()
        S = stacked.StackedSGLD(Net().cuda(), 4, _args(**extra), init="reinit", seed=4,
                                logger=log, graph=False)
        return S, S.train(loader, test_loader=loader[:2]), log.lines

    S, hist, lines = run(rhat=True)
    assert [("test" in r, "rhat" in r) for r in hist] == [(True, True), (True, True)]
    r = hist[-1]["rhat"]
    assert r["count"] == S.cnt == 1 + 2 * len(loader) and r["n_eval"] == S.state.n1
    assert r["rhat_max"] >= r["rhat_mean"] > 0 and r["argmax_param"] in S.state.names
    assert not any(isinstance(v, torch.Tensor) for v in r.values())
    rl = [ln for ln in lines if "R-hat" in ln]
    assert len(rl) == 2 and r["argmax_param"] in rl[-1] and "> 1.05" in rl[-1]
    S2, hist2, lines2 = run()
    assert all("rhat" not in r for r in hist2) and not any("R-hat" in ln for ln in lines2)
    assert [ln for ln in lines if "R-hat" not in ln and "chains: loss" not in ln] == \
        [ln for ln in lines2 if "chains: loss" not in ln]   # (the epoch lines carry seconds)
    assert torch.equal(S.state.theta, S2.state.theta)      # the report changes no chain
