"""The cross-chain diagnostic (include/bdl_diag.h) without a GPU: the C struct
layouts against the ctypes mirrors, the exports, every validation path of
bdl_chain_diag (fake pointers: each call returns before any HIP call), the
fp32 formulation's own error against the textbook float64 formulas, and the
stacked samplers' `_moment_spec` / `diagnostics` bookkeeping on host-only
fakes."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import chain_diag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

SUMMARY_FIELDS = ["n_eval", "n_degenerate", "n_nonfinite", "argmax", "n_above", "rhat_sum",
                  "rhat_max", "pad"]
ARGS_FIELDS = ["mom1", "mom2", "pooled_mean", "pooled_var", "rhat", "workspace", "n",
               "chain_groups", "chains", "var_mode", "ratio", "inv_ratio", "var_floor", "c1",
               "thresholds", "blocks_per_cu"]


def _c_layout(tmp_path):
    lines = ['printf("bdl_diag_summary %zu\\nbdl_chain_diag_args %zu\\n", '
             'sizeof(bdl_diag_summary), sizeof(bdl_chain_diag_args));']
    for st, fields in (("bdl_diag_summary", SUMMARY_FIELDS), ("bdl_chain_diag_args", ARGS_FIELDS)):
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_diag.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    out = subprocess.check_output([str(exe)]).decode()
    return {k: int(v) for k, v in (ln.rsplit(" ", 1) for ln in out.strip().splitlines())}


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    lay = _c_layout(tmp_path)
    assert lay["bdl_diag_summary"] == C.sizeof(L.DiagSummary)
    assert lay["bdl_chain_diag_args"] == C.sizeof(L.DiagArgs)
    assert [f for f, _ in L.DiagSummary._fields_] == SUMMARY_FIELDS
    assert [f for f, _ in L.DiagArgs._fields_] == ARGS_FIELDS
    for cls, name in ((L.DiagSummary, "bdl_diag_summary"), (L.DiagArgs, "bdl_chain_diag_args")):
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[f"{name}.{f}"], (name, f)


def test_library_exports_the_diagnostic_next_to_the_pinned_abi():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.DIAG_EXPORTS) == {"bdl_chain_diag", "bdl_chain_diag_workspace_bytes"}
    assert not set(L.DIAG_EXPORTS) & set(L.EXPORTS)
    for name in L.DIAG_EXPORTS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    nb = h.bdl_chain_diag_workspace_bytes(10 ** 9)
    assert nb >= C.sizeof(L.DiagSummary) and nb % 8 == 0
    assert nb == h.bdl_chain_diag_workspace_bytes(1)


def _good_args():
    from bayesdll_amd import _lib as L
    a = L.DiagArgs()
    a.mom1, a.mom2, a.workspace = 0x10000, 0x20000, 0x30000
    a.pooled_mean, a.pooled_var, a.rhat = 0x40000, 0x50000, 0x60000
    a.n, a.chain_groups, a.chains, a.var_mode = 10, 3, 4, L.VAR_WELFORD
    a.ratio, a.var_floor, a.c1 = 3.0, 1e-12, 0.75
    return a


def test_chain_diag_validates_before_touching_the_device():
    """Every refusal of the header's table, with its status and a message.
    No call here passes validation, so none reaches a HIP call."""
    from bayesdll_amd import _lib as L
    h = L.lib()
    NULL, ALIGN, ARG = -1, -2, -3

    def refused(status, word, **fields):
        a = _good_args()
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_chain_diag(a, None) == status, fields
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_diag:") and word in msg, (fields, msg)

    assert h.bdl_chain_diag(None, None) == NULL and b"null args" in h.bdl_last_error()
    refused(NULL, b"mom1", mom1=None)
    refused(NULL, b"mom2", mom2=None)
    refused(NULL, b"workspace", workspace=None)
    for f in ("mom1", "mom2", "pooled_mean", "pooled_var", "rhat"):
        refused(ALIGN, b"vector not 16-B aligned", **{f: 0x70008})
    refused(ALIGN, b"workspace not 16-B aligned", workspace=0x30004)
    refused(ARG, b"chains", chains=1)
    refused(ARG, b"chains", chains=0)
    refused(ARG, b"chains", chains=-3)
    refused(ARG, b"n must be", n=0)
    refused(ARG, b"n must be", n=-5)
    refused(ARG, b"chain slot", n=13)                     # 4 * chain_groups = 12
    refused(ARG, b"chain slot", chain_groups=0)
    refused(ARG, b"var_mode", var_mode=3)
    refused(ARG, b"var_mode", var_mode=-1)
    refused(ARG, b"var_floor", var_floor=-1e-12)
    refused(ARG, b"var_floor", var_floor=float("nan"))
    refused(ARG, b"blocks_per_cu", blocks_per_cu=9)
    refused(ARG, b"overflows", chain_groups=1 << 60, chains=2)   # 4 * 2^60 * 2 = 2^63
    refused(ARG, b"overflows", chain_groups=(1 << 64) - 1)
    refused(ARG, b"overflows", chain_groups=((1 << 61) - 1) // 4 + 1)  # just past INT64_MAX / 4 / 4


def test_chain_diag_refuses_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_chain_diag(_good_args(), None) == -3
        assert b"graph redirect is active" in h.bdl_last_error()
        assert h.bdl_chain_diag(None, None) == -3
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_chain_diag(None, None) == -1  # back to ordinary validation


def test_python_wrapper_refuses_before_any_launch():
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    m = torch.zeros(16)
    kw = dict(chains=2, chain_groups=2, n=8, var_mode=L.VAR_GIVEN, ratio=1.0)
    with pytest.raises(ValueError, match="second moment"):
        K.chain_diag(m, None, count=5, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        K.chain_diag(m, m, count=5, **kw)                  # CPU tensors: no CPU path
    assert K.diag_bytes_per_elem(8, 1) == 68 and K.diag_bytes_per_elem(64, 3) == 524
    # the remaining refusals come after the device check: reach them with it waved through
    real, L.require_hip = L.require_hip, lambda *a, **k: None
    try:
        with pytest.raises(ValueError, match="at least 2 samples"):
            K.chain_diag(m, m, count=1, **kw)
        with pytest.raises(ValueError, match="at least 2 chains"):
            K.chain_diag(m, m, count=5, **dict(kw, chains=1))
        with pytest.raises(ValueError, match="at least 24 elements"):
            K.chain_diag(m, m, count=5, **dict(kw, chains=3))
        with pytest.raises(ValueError, match="want from"):
            K.chain_diag(m, m, count=5, want=("rhat", "ess"), **kw)
    finally:
        L.require_hip = real


# measured maxima of this very test (200,000 elements per case, seeds as below)
@pytest.mark.parametrize("K_", [2, 3, 8, 64])
def test_fp32_formulation_against_float64_two_pass(K_):
    """The fp32 shifted-sum arithmetic of include/bdl_diag.h against the
    textbook float64 two-pass formulas: per-chain means = a common base
    +-U(0.5, 2) + N(0, 0.05^2) spread between chains, variances
    0.05^2 * U(0.5, 2) (of the spread's order, VAR_GIVEN), count = 20,
    200,000 elements.

    Bounds: R-hat relative error <= 4 K 2^-24 (the shifted sum's bound: K
    roundings of S2 / SW and O(1) further ones) and |mbar - mean64| <=
    4 * 2^-24 * max_k |m_k|.  Measured with exactly this arithmetic (max over
    the elements; bound in brackets):
        K = 2   R-hat 1.38e-07 (4.8e-07)   mean error 0.25 of its bound
        K = 3   R-hat 2.23e-07 (7.2e-07)   mean error 0.25
        K = 8   R-hat 5.87e-07 (1.9e-06)   mean error 0.27
        K = 64  R-hat 3.09e-06 (1.5e-05)   mean error 0.42
    None of the inputs is degenerate or non-finite, so no element escapes.

    Why the base stays away from zero: mbar = m_0 + S1 / K carries the K
    roundings of S1, each up to 2^-25 |S1| with |S1| up to K max|d|, so its
    error is about 2^-24 (|mbar| / 2 + |q| / 2 + c sqrt(K) max|d|) — inside
    4 * 2^-24 max|m| when the chains' differences d are small against the
    value they share, which is what a common base plus spread means.  An
    element whose base is below the spread is all spread: there a K-term fp32
    sum cannot meet a K-free bound (with a N(0, 1) base the K = 64 case came
    out at 1.17 of the mean bound on the elements with |m| < 0.1; R-hat, which
    only sees differences, stayed inside its bound there too)."""
    n, count = 200_000, 20
    m1, m2, cg = R.make_case(1000 + K_, K_, n)
    kw = dict(chains=K_, chain_groups=cg, n=n, var_mode=R.VAR_GIVEN, count=count)
    mbar, pvar, rhat, s = R.chain_diag_f32(m1, m2, **kw)
    assert (s["n_eval"], s["n_degenerate"], s["n_nonfinite"]) == (n, 0, 0)
    mbar64, pvar64, rhat64 = R.chain_diag_f64(m1, m2, **kw)
    rel = np.abs(rhat.astype(np.float64) - rhat64) / rhat64
    mmax = np.abs(np.stack([m1[4 * cg * k: 4 * cg * k + n] for k in range(K_)])).max(0)
    merr = np.abs(mbar.astype(np.float64) - mbar64) / (4 * 2.0 ** -24 * mmax.astype(np.float64))
    print(f"K={K_}: rhat rel max {rel.max():.3e} (bound {4 * K_ * 2.0 ** -24:.3e}), "
          f"mean err / bound max {merr.max():.3f}, "
          f"pooled var rel max {(np.abs(pvar - pvar64) / pvar64).max():.3e}")
    assert rel.max() <= 4 * K_ * 2.0 ** -24
    assert merr.max() <= 1.0
    assert s["rhat_max"] == float(rhat.max()) and rhat[s["argmax"]] == rhat.max()


def test_reference_conventions_degenerate_nonfinite_threshold_and_tie():
    """The reference's own conventions on a hand-made case (what the GPU test
    then demands of the device): frozen elements degenerate, zero variance at
    floor 0 non-finite, a value on a threshold not above it, the lowest index
    among equal maxima."""
    K_, n = 3, 8
    m1 = np.zeros(K_ * 8, R.F)
    m2 = np.full(K_ * 8, 0.25, R.F)
    for k in range(K_):
        m1[8 * k: 8 * k + 8] = [1.0, 2.0 + k, 5.0, 2.0 + k, -1.0 + 0.5 * k, 7.0, 3.0 - k, 0.0]
    for k in range(K_):
        m2[8 * k + 6] = 0.0                                 # zero variance, spread: Inf
    mbar, pvar, rhat, s = R.chain_diag_f32(m1, m2, chains=K_, chain_groups=2, n=n,
                                           var_mode=R.VAR_GIVEN, var_floor=0.0, count=4)
    assert np.isnan(rhat[[0, 2, 5, 7]]).all() and s["n_degenerate"] == 4
    assert np.isinf(rhat[6]) and s["n_nonfinite"] == 1 and s["n_eval"] == 3
    assert rhat[1] == rhat[3] == s["rhat_max"] and s["argmax"] == 1
    assert mbar[0] == 1.0 and pvar[0] == 0.25 and mbar[1] == 3.0
    thr = (float(rhat[4]), float(rhat[1]), 0.0)
    s2 = R.chain_diag_f32(m1, m2, chains=K_, chain_groups=2, n=n, var_mode=R.VAR_GIVEN,
                          var_floor=0.0, count=4, thresholds=thr)[3]
    assert s2["n_above"] == [2, 0, 3]                      # on a threshold: not above it


# ------------------------------------------------------------ stacked fakes
class Net(nn.Module):
    readout_name = "head"

    def __init__(self):
        super().__init__()
        self.body = nn.Linear(13, 7)
        self.head = nn.Linear(7, 5)    # n = 138, stride 140

    def forward(self, x):
        return self.head(torch.tanh(self.body(x)))


def _args(nst=2):
    return SimpleNamespace(lr=5e-2, lr_head=1e-1, epochs=2, num_cycles=2,
                           proportion_exploration=0.5, ND=64, device="cpu", seed=7, momentum=0.5,
                           hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0,
                                    "nd": 1.0, "thin": 1, "nst": nst, "bias": "informative",
                                    "burnin": 0})


@pytest.fixture
def host_only(monkeypatch):
    """State on the CPU; launches recorded instead of made."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    calls = []
    monkeypatch.setattr(L, "require_hip", lambda *a, **k: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    monkeypatch.setattr(K, "sgmcmc_step", lambda st, m, **kw: calls.append(("step", kw)))
    monkeypatch.setattr(K, "moments_update", lambda *a, **kw: calls.append(("moments", a)))
    monkeypatch.setattr(K, "posterior_sample",
                        lambda out, m1, m2, **kw: calls.append(("sample", m1, m2, kw)))

    class FakeResult(dict):
        summary = {"n_eval": 138, "n_degenerate": 0, "n_nonfinite": 0, "argmax": 100,
                   "n_above": [3, 2, 1], "rhat_sum": 140.0, "rhat_max": 1.5, "rhat_mean": 1.01,
                   "share_above": [3 / 138, 2 / 138, 1 / 138], "thresholds": [1.01, 1.05, 1.1]}

    def fake_diag(m1, m2, **kw):
        calls.append(("diag", m1, m2, kw))
        return FakeResult({w: torch.zeros(kw["n"]) for w in kw["want"]})

    monkeypatch.setattr(K, "chain_diag", fake_diag)
    return calls


def test_csghmc_moment_spec_halves_the_doubled_count(host_only):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import stacked
    S = stacked.StackedCSGHMC(Net(), 3, _args())
    assert S._latest_component() is None
    assert S._moment_spec(1)[0] is None and S._moment_spec(1)[4] == 0
    with pytest.raises(ValueError, match="nothing is collected"):
        S.diagnostics()
    # three collects into cycle 1, bookkept as train_one_epoch does (quirk Q2)
    for want_kind, want_n in ((L.COLLECT_WELFORD_INIT, 1), (L.COLLECT_WELFORD, 3),
                              (L.COLLECT_WELFORD, 5)):
        (kind, m1, m2, ca), cnt = S._collect_spec(1)
        assert (kind, cnt) == (want_kind, want_n)
        S.samples_per_cycle[1] = cnt + 1
        if want_n == 1:  # one collect: stored count 2, the draw's divisor 1, but one sample
            assert S._moment_spec(1)[2:] == (L.VAR_WELFORD, 1.0, 1)
            with pytest.raises(ValueError, match="at least 2"):
                S.diagnostics()
    assert S.samples_per_cycle[1] == 6
    m1, m2, var_mode, ratio, count = S._moment_spec(1)
    assert m1 is S.mom1[1] and m2 is S.mom2[1]
    assert (var_mode, ratio, count) == (L.VAR_WELFORD, 5.0, 3)
    # the draw uses the very same spec
    list(S._components(torch.empty_like(S.state.theta)))
    kind, dm1, dm2, kw = host_only[-1]
    assert kind == "sample" and dm1 is m1 and dm2 is m2
    assert (kw["var_mode"], kw["ratio"]) == (var_mode, ratio)
    # a later cycle becomes the default component
    S._collect_spec(2)
    S.samples_per_cycle[2] = 4
    d = S.diagnostics(rhat=True)
    kind, dm1, dm2, kw = host_only[-1]
    assert kind == "diag" and dm1 is S.mom1[2] and dm2 is S.mom2[2]
    assert (kw["chains"], kw["chain_groups"], kw["n"]) == (3, 35, 138)
    assert (kw["var_mode"], kw["ratio"], kw["count"], kw["want"]) == (L.VAR_WELFORD, 3.0, 2,
                                                                       ("rhat",))
    assert d["component"] == 2 and d["count"] == 2 and d["rhat"].shape == (138,)
    assert d["argmax_param"] == "head.weight" and "pooled_mean" not in d   # 100 in [98, 133)
    assert S.diagnostics(1, pooled=True)["component"] == 1
    assert host_only[-1][3]["want"] == ("pooled_mean", "pooled_var")


def test_sgld_and_csgld_moment_specs(host_only):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import stacked
    S = stacked.StackedSGLD(Net(), 2, _args())
    assert S._latest_component() is None and S._moment_spec(0)[0] is None
    with pytest.raises(ValueError, match="nothing is collected"):
        S.diagnostics()
    S.seed_moments()
    assert S._moment_spec(0)[2:] == (L.VAR_RAW_MOMENTS, 1.0, 1)
    with pytest.raises(ValueError, match="at least 2"):
        S.diagnostics()
    S.cnt = 5
    m1, m2, var_mode, ratio, count = S._moment_spec(0)
    assert m1 is S.m1 and m2 is S.m2 and (var_mode, ratio, count) == (L.VAR_RAW_MOMENTS, 1.25, 5)
    assert S.diagnostics()["count"] == 5 and host_only[-1][3]["want"] == ()
    with pytest.raises(ValueError, match="nothing is collected"):
        S.diagnostics(3)
    # nst = 0 keeps no second moment
    S0 = stacked.StackedSGLD(Net(), 2, _args(nst=0))
    S0.seed_moments()
    S0.cnt = 4
    with pytest.raises(ValueError, match="second moment is not kept"):
        S0.diagnostics()
    # one chain has nobody to agree with
    S1 = stacked.StackedSGLD(Net(), 1, _args())
    S1.seed_moments()
    S1.cnt = 4
    with pytest.raises(ValueError, match="K = 1"):
        S1.diagnostics()
    # SGHMC shares SGLD's moments
    assert stacked.StackedSGHMC._moment_spec is stacked.StackedSGLD._moment_spec
    # cSGLD: per-cycle moments, the plain count
    SC = stacked.StackedCSGLD(Net(), 2, _args())
    assert SC._latest_component() is None
    SC.mom1[0] = torch.zeros(SC.state.n)
    SC.mom2[0] = torch.zeros(SC.state.n)
    SC.samples_per_cycle[0] = 4
    SC.mom1[1], SC.mom2[1] = torch.zeros(SC.state.n), torch.zeros(SC.state.n)
    SC.samples_per_cycle[1] = 1
    assert SC._latest_component() == 1
    assert SC._moment_spec(0)[2:] == (L.VAR_RAW_MOMENTS, 4 / 3, 4)
    assert SC._moment_spec(1)[2:] == (L.VAR_RAW_MOMENTS, 1.0, 1)
    assert SC._moment_spec(0)[0] is SC.mom1[0] and SC._moment_spec(0)[1] is SC.mom2[0]
    assert SC.diagnostics(0)["count"] == 4


def test_run_cli_rhat_needs_stacked_chains(capsys):
    from bayesdll_amd import run
    assert run.build_parser().parse_args(["--stacked_chains", "4", "--rhat"]).rhat is True
    assert run.build_parser().parse_args([]).rhat is False
    for argv in (["--rhat"], ["--rhat", "--stacked_chains", "1"]):
        with pytest.raises(SystemExit):
            run.main(argv)
        assert "--stacked_chains >= 2" in capsys.readouterr().err
