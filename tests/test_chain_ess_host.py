"""The batch-means effective sample size (include/bdl_ess.h) without a GPU: the
header's functions, the C struct layouts against the ctypes mirrors, the
exports, every validation path of both entry points (fake pointers: each call
returns before any HIP call), the flag / scalar bookkeeping of
bayesdll_amd.ess, the fp32 formulation's own error against textbook float64
batch means and the exact AR(1) value, the stacked samplers' refusals on
host-only fakes, and the command line."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import chain_ess_ref as R
from test_chain_diag_host import Net, _args, host_only  # noqa: F401  (host_only: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

FOLD_FIELDS = ["theta", "bsum", "smean", "sM2", "bM2", "n", "chain_groups", "sample", "batch",
               "chains", "flags", "fs", "fb", "c", "grid_blocks"]
SUMMARY_FIELDS = ["n_eval", "n_degenerate", "n_nonfinite", "argmin", "n_below", "ess_sum",
                  "ess_min", "pad"]
ARGS_FIELDS = ["sM2", "bM2", "ess", "mcse", "workspace", "n", "chain_groups", "samples",
               "batches", "chains", "grid_blocks", "thresholds", "pad0"]
STRUCTS = (("bdl_ess_fold_args", FOLD_FIELDS), ("bdl_ess_summary", SUMMARY_FIELDS),
           ("bdl_chain_ess_args", ARGS_FIELDS))


def test_header_declares_exactly_the_three_functions_and_no_abi_version():
    src = open(os.path.join(INCLUDE, "bdl_ess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    funcs = re.findall(r"\b(bdl_\w+)\s*\(", code)
    assert sorted(funcs) == ["bdl_chain_ess", "bdl_chain_ess_fold", "bdl_chain_ess_workspace_bytes"]
    assert "BDL_ABI_VERSION" not in code
    assert '#include "bdl_sgmcmc.h"' in code


def _c_layout(tmp_path):
    lines = []
    for st, fields in STRUCTS:
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    lines.append('printf("flags %d\\n", BDL_ESS_FIRST_SAMPLE | BDL_ESS_FIRST_IN_BATCH << 4 | '
                 'BDL_ESS_CLOSE << 8 | BDL_ESS_FIRST_BATCH << 12);')
    lines.append('printf("limits %d %d %d\\n", BDL_ESS_MAX_COUNT, BDL_ESS_MAX_CHAINS, '
                 'BDL_ESS_MAX_GRID);')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_ess.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    out = subprocess.check_output([str(exe)]).decode().strip().splitlines()
    lay = {k: v for k, v in (ln.split(" ", 1) for ln in out)}
    return lay


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import ess as E
    lay = _c_layout(tmp_path)
    for cls, (name, fields) in zip((L.EssFoldArgs, L.EssSummary, L.EssArgs), STRUCTS):
        assert int(lay[name]) == C.sizeof(cls), name
        assert [f for f, _ in cls._fields_] == fields
        for f in fields:
            assert getattr(cls, f).offset == int(lay[f"{name}.{f}"]), (name, f)
    assert int(lay["flags"]) == 0x8421
    assert (L.ESS_FIRST_SAMPLE, L.ESS_FIRST_IN_BATCH, L.ESS_CLOSE, L.ESS_FIRST_BATCH) == \
        (E.FIRST_SAMPLE, E.FIRST_IN_BATCH, E.CLOSE, E.FIRST_BATCH) == (1, 2, 4, 8)
    assert lay["limits"] == f"{L.ESS_MAX_COUNT} {L.ESS_MAX_CHAINS} {L.ESS_MAX_GRID}"
    assert E.MAX_COUNT == L.ESS_MAX_COUNT == 1 << 24


def test_library_exports_the_ess_next_to_the_pinned_abi():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.ESS_EXPORTS) == {"bdl_chain_ess_fold", "bdl_chain_ess",
                                  "bdl_chain_ess_workspace_bytes"}
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS, L.CHAIN_STEP_EXPORTS,
                  L.STATS_EXPORTS):
        assert not set(L.ESS_EXPORTS) & set(other)
    for name in L.ESS_EXPORTS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    nb = h.bdl_chain_ess_workspace_bytes(10 ** 9)
    assert nb >= C.sizeof(L.EssSummary) * (1 + L.ESS_MAX_GRID) and nb % 8 == 0
    assert nb == h.bdl_chain_ess_workspace_bytes(1)


NULL, ALIGN, ARG = -1, -2, -3


def _good_fold():
    from bayesdll_amd import _lib as L
    a = L.EssFoldArgs()
    a.theta, a.bsum, a.smean, a.sM2, a.bM2 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.n, a.chain_groups, a.chains = 10, 3, 4                 # 46 elements = 184 bytes a vector
    a.sample, a.batch, a.flags = 6, 3, L.ESS_CLOSE           # closes batch i = 2
    a.fs, a.fb, a.c = 6.0, 3.0, 2.0
    return a


def test_fold_validates_before_touching_the_device():
    """Every refusal of the header's table, with its status and a message.
    No call here passes validation, so none reaches a HIP call."""
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, **fields):
        a = _good_fold()
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_chain_ess_fold(a, None) == status, fields
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_ess_fold:") and word in msg, (fields, msg)

    assert h.bdl_chain_ess_fold(None, None) == NULL and b"null args" in h.bdl_last_error()
    refused(NULL, b"theta", theta=None)
    for f in ("smean", "sM2", "bM2"):
        refused(NULL, b"smean, sM2 and bM2", **{f: None})
    refused(NULL, b"bsum is required", bsum=None)
    for f in ("theta", "bsum", "smean", "sM2", "bM2"):
        refused(ALIGN, b"vector not 16-B aligned", **{f: 0x70008})
    refused(ARG, b"chains", chains=0)
    refused(ARG, b"chains", chains=-3)
    refused(ARG, b"chains", chains=65536)
    refused(ARG, b"n must be", n=0)
    refused(ARG, b"n must be", n=-5)
    refused(ARG, b"chain slot", n=13)                          # 4 * chain_groups = 12
    refused(ARG, b"chain slot", chain_groups=0)
    refused(ARG, b"grid_blocks", grid_blocks=-1)
    refused(ARG, b"grid_blocks", grid_blocks=2049)
    refused(ARG, b"overflows", chain_groups=1 << 60, chains=2)
    refused(ARG, b"overflows", chain_groups=(1 << 64) - 1)
    refused(ARG, b"batch must be", batch=0)
    refused(ARG, b"batch must be", batch=1 << 24)
    refused(ARG, b"sample must be", sample=0)
    refused(ARG, b"sample must be", sample=1 << 24)
    # counters inconsistent with the flags, and scalars inconsistent with the counters
    refused(ARG, b"flags 0 are not what sample 6 of batch 3 implies (4)", flags=0)
    refused(ARG, b"flags", flags=L.ESS_CLOSE | L.ESS_FIRST_BATCH)
    refused(ARG, b"flags", flags=L.ESS_CLOSE | L.ESS_FIRST_SAMPLE)
    refused(ARG, b"flags", flags=16 | L.ESS_CLOSE)
    refused(ARG, b"flags", sample=5)                           # p = 2 of 3: no close
    refused(ARG, b"flags", sample=1, flags=L.ESS_FIRST_IN_BATCH)   # the first sample says so
    refused(ARG, b"fs / fb", fs=5.0)
    refused(ARG, b"fs / fb", fb=2.0)
    refused(ARG, b"fs / fb", fs=float("nan"))
    refused(ARG, b"c is not", c=1.5)
    refused(ARG, b"c is not", c=float("nan"))
    refused(ARG, b"c is not", sample=9, fs=9.0)                # i = 3: c must be 1.5
    # two vectors sharing a byte: 184 bytes each
    refused(ARG, b"overlap", smean=0x20000)
    refused(ARG, b"overlap", smean=0x20000 + 176)
    refused(ARG, b"overlap", bM2=0x10000 + 96)
    refused(ARG, b"overlap", sM2=0x50000 - 176)
    # at batch == 1 bsum is never touched: null, misaligned or overlapping is fine there, and the
    # call goes on to the next refusal
    refused(ARG, b"overlap", batch=1, sample=6, fs=6.0, fb=1.0, c=1.2,
            flags=L.ESS_FIRST_IN_BATCH | L.ESS_CLOSE, bsum=0x30004, sM2=0x30000)


def _good_report():
    from bayesdll_amd import _lib as L
    a = L.EssArgs()
    a.sM2, a.bM2, a.ess, a.mcse, a.workspace = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000
    a.n, a.chain_groups, a.chains = 10, 3, 4
    a.samples, a.batches = 12, 4
    return a


def test_report_validates_before_touching_the_device():
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, **fields):
        a = _good_report()
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_chain_ess(a, None) == status, fields
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_ess:") and word in msg, (fields, msg)

    assert h.bdl_chain_ess(None, None) == NULL and b"null args" in h.bdl_last_error()
    refused(NULL, b"sM2 and bM2", sM2=None)
    refused(NULL, b"sM2 and bM2", bM2=None)
    refused(NULL, b"workspace", workspace=None)
    for f in ("sM2", "bM2", "ess", "mcse"):
        refused(ALIGN, b"vector not 16-B aligned", **{f: 0x70008})
    refused(ALIGN, b"workspace not 16-B aligned", workspace=0x100004)
    refused(ARG, b"chains", chains=0)
    refused(ARG, b"chains", chains=65536)
    refused(ARG, b"n must be", n=0)
    refused(ARG, b"chain slot", n=13)
    refused(ARG, b"chain slot", chain_groups=0)
    refused(ARG, b"grid_blocks", grid_blocks=-1)
    refused(ARG, b"grid_blocks", grid_blocks=2049)
    refused(ARG, b"overflows", chain_groups=1 << 60, chains=2)
    refused(ARG, b"samples must be >= 2 (got 1)", samples=1, batches=1)
    refused(ARG, b"samples must be", samples=0)
    refused(ARG, b"batches must be >= 2 (got 1)", batches=1)
    refused(ARG, b"batches must be", batches=0)
    refused(ARG, b"batches exceeds samples", batches=13)
    refused(ARG, b"below 2^24", samples=1 << 24)
    refused(ARG, b"below 2^24", samples=(1 << 24) + 5, batches=1 << 24)
    refused(ARG, b"overlaps", ess=0x10000 + 16)               # inside sM2 (184 bytes)
    refused(ARG, b"overlaps", mcse=0x20000 + 176)
    refused(ARG, b"overlaps", ess=0x100000 + 64)              # inside the workspace
    refused(ARG, b"ess and mcse overlap", mcse=0x30000 + 32)  # 40 bytes each
    refused(ARG, b"workspace overlaps", sM2=0x100000 + 1024)


def test_both_entry_points_refuse_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_chain_ess_fold(_good_fold(), None) == ARG
        assert b"graph redirect is active" in h.bdl_last_error()
        assert h.bdl_chain_ess(_good_report(), None) == ARG
        assert b"graph redirect is active" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_chain_ess(None, None) == NULL


# ------------------------------------------------------------- bookkeeping
FS, FIB, CL, FB = 1, 2, 4, 8
EXPECTED_FLAGS = {
    1: [FS | FIB | CL | FB] + [FIB | CL] * 10,
    2: [FS | FIB, CL | FB, FIB, CL, FIB, CL, FIB, CL, FIB, CL, FIB],
    5: [FS | FIB, 0, 0, 0, CL | FB, FIB, 0, 0, 0, CL, FIB],
}


@pytest.mark.parametrize("b", [1, 2, 5])
def test_fold_plan_flags_and_scalars_over_eleven_samples(b):
    from bayesdll_amd import ess as E
    from bayesdll_amd import kernels as K
    for s in range(1, 12):
        flags, fs, fb, c = E.fold_plan(s, b)
        assert flags == EXPECTED_FLAGS[b][s - 1], (b, s)
        assert (fs, fb) == (float(s), float(b))
        rflags, rfs, rfb, rc = R.fold_plan(s, b)
        assert (flags, np.float32(fs), np.float32(fb)) == (rflags, rfs, rfb)
        if flags & CL and not flags & FB:
            i = s // b
            assert np.float32(c) == np.float32(i / (i - 1)) == rc
            assert C.c_float(c).value == float(rc)       # what the C field receives
        else:
            assert rc is None and c == 1.0
        # bytes per element: 24-32 once a component is under way
        nbytes = K.ess_fold_bytes_per_elem(flags)
        assert nbytes == E.fold_bytes_per_elem(flags)
        if not flags & FS:
            assert 24 <= nbytes <= 32 or (b == 1 and nbytes == 28)
    assert E.fold_bytes_per_elem(0) == 28 and E.fold_bytes_per_elem(FIB) == 24
    assert E.fold_bytes_per_elem(CL) == 32 and E.fold_bytes_per_elem(FIB | CL) == 28
    assert E.fold_bytes_per_elem(FS | FIB) == 16 and E.fold_bytes_per_elem(15) == 16
    assert K.ess_bytes_per_elem(8, 0) == 64 and K.ess_bytes_per_elem(64, 2) == 520
    # i/(i-1) is formed in float64 and rounded once: 3/2, 4/3, 11/10
    assert [E.fold_plan(i * 7, 7)[3] for i in (3, 4, 11)] == [1.5, 4 / 3, 1.1]
    for bad in ((0, 1), (1, 0), (1 << 24, 1), (5, 1 << 24)):
        with pytest.raises(ValueError, match="2\\^24"):
            E.fold_plan(*bad)


def test_counts_thresholds_and_summary_dict():
    from bayesdll_amd import ess as E
    assert E.counts(11, 5) == (11, 2) and E.counts(9, 5) == (9, 1)
    with pytest.raises(ValueError, match="nothing is folded yet"):
        E.check_report(0, 4)
    with pytest.raises(ValueError, match="7 samples folded per chain close 1 batch of 4"):
        E.check_report(7, 4)
    with pytest.raises(ValueError, match="1 sample folded per chain close 0 batches of 4"):
        E.check_report(1, 4)
    assert E.check_report(8, 4) == (8, 2)
    assert E.thresholds() == (100.0, 400.0, 1000.0) and E.thresholds([1, 2, 3]) == (1.0, 2.0, 3.0)
    for bad in ((1, 2), (1, 2, float("nan")), (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="three finite"):
            E.thresholds(bad)
    for ok in (0, 1, 7, np.int64(3), 4.0):
        assert E.check_batch(ok) == int(ok)
    for bad in (-1, 1.5, "x", None, 1 << 24):
        with pytest.raises(ValueError, match="ess_batch must be an integer >= 0"):
            E.check_batch(bad)
    raw = {"n_eval": 4, "n_degenerate": 1, "n_nonfinite": 2, "argmin": 3, "n_below": [1, 2, 4],
           "ess_sum": 100.0, "ess_min": 12.5}
    d = E.summary_dict(raw, (100.0, 400.0, 1000.0), samples=12, batches=4, batch=3, chains=2)
    assert d["ess_mean"] == 25.0 and d["share_below"] == [0.25, 0.5, 1.0]
    assert (d["samples"], d["batches"], d["batch"], d["chains"]) == (12, 4, 3, 2)
    empty = E.summary_dict(dict(raw, n_eval=0, argmin=-1), (1, 2, 3), samples=4, batches=2,
                           batch=2, chains=1)
    assert math.isnan(empty["ess_mean"]) and all(math.isnan(v) for v in empty["share_below"])


# ------------------------------------------------- the formulation's own error
def _ar1_expectations(rho, b, S):
    """E[s^2] / sigma^2 and E[vb] / sigma^2 of a stationary unit-variance AR(1)
    series: the sample variance of n correlated values with autocovariances g_h
    has expectation g_0 - 2 / (n (n-1)) sum_{h=1}^{n-1} (n - h) g_h; for the
    batch means g_j = b^-2 sum_{p,q<b} rho^|j b + q - p|."""
    h = np.arange(1, S)
    es2 = 1.0 - 2.0 / (S * (S - 1)) * np.sum((S - h) * float(rho) ** h)
    nb = S // b
    p = np.arange(b)
    lag = p[None, :] - p[:, None]
    g = np.array([np.sum(float(rho) ** np.abs(j * b + lag)) / b ** 2 if rho else
                  (1.0 / b if j == 0 else 0.0) for j in range(nb)])
    j = np.arange(1, nb)
    evb = g[0] - 2.0 / (nb * (nb - 1)) * np.sum((nb - j) * g[1:])
    return es2, evb


@pytest.mark.parametrize("rho", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("K_", [2, 8])
def test_fp32_formulation_against_float64_batch_means_and_exact_ar1(K_, rho):
    """The fp32 fold + report of include/bdl_ess.h (the host reference, op for
    op) against textbook float64 batch means over the stored samples, and the
    textbook estimate against the exact AR(1) value.  x = 0.02 + 1e-3 z (the
    cancellation of real weights: |x| / sigma = 20, |x| / sigma_batch up to
    80), b = 16, nb = 64 (S = 1024), 4096 elements.

    Bound on the per-element relative error of ess, in units of u = 2^-24, from
    the operation count (first order; m = max |x| of the element, sb / s the
    smallest float64 batch-mean / sample standard deviation over its chains):
      * smean carries one rounding of size <= u m per fold (q's own is
        u |q| << u m), damped by (1 - 1/s) at every later fold: at most
        u m ((S+1)/2 + 1) at any time;
      * bsum carries b - 1 roundings of partial sums <= p m, so y = bsum / b is
        off by at most u m ((b+1)/2 + 1); y - smean' is exact or one more u;
      * a term (y - smean')^2 with the difference off by D changes by
        2 |e| D, and sum |e_i| <= sqrt(nb sum e_i^2) (Cauchy-Schwarz): bM2 is
        off by at most 2 D / sb relative, plus its nb additions of
        non-negative terms, the square, the product with c and c's own
        rounding: (nb + 3) u;
      * sM2 likewise by 2 D_m / s + (S + 2) u;
      * K - 1 additions each for SW and SV of non-negative terms, then four
        roundings (w, v, r, ess).
    bound = u [2 (m/sb) ((S+1)/2 + (b+1)/2 + 2) + 2 (m/s) ((S+1)/2 + 1)
               + S + nb + 2 K + 10].
    It is a worst case (every rounding of a 1024-step recursion aligned); the
    measured maxima of max_j err_j / bound_j, this very test:
        K = 2:  rho 0: 3.6e-03   rho 0.5: 2.4e-03   rho 0.9: 1.4e-03
        K = 8:  rho 0: 1.4e-03   rho 0.5: 9.9e-04   rho 0.9: 5.5e-04
    (largest relative error itself: 427 u = 2.5e-5 at K = 2, rho = 0, where the
    bound is 1.1e5-1.7e5 u; mcse, held to the same bound, at most 227 u.)

    The estimator against theory.  Batch means estimates S sigma^2 / (b
    Var(ybar_b)) = S / tau_b per chain, tau_b = 1 + 2 sum_{k<b} (1 - k/b)
    rho^k.  The 4096 elements are independent replicates, so their mean is
    held to five standard errors taken from the textbook estimate's own spread
    across elements.  At that precision (0.1-0.2 %) two finite-sample effects
    of the textbook estimator itself show, neither of them arithmetic: the
    mean of a ratio exceeds the ratio of means by CV^2(vb) ~ 2 / (K (nb - 1))
    (1.6 % at K = 2), and with S = 1024 the sample variances of correlated
    values are biased low (s^2 by 1.8 % at rho = 0.9, vb by its batch means'
    own correlation).  So the check is made where the theory is exact: the
    element-pooled ratio K nb mean_j(w_j) / mean_j(v_j) against K nb E[s^2] /
    E[vb] with the closed-form expectations (_ar1_expectations), its standard
    error from the elements' spread of the linearised ratio; and those
    expectations must agree with S / tau_b to the size of the effects above
    (2.5 %).  Measured: the pooled ratio lies at z = -0.8, -0.8, -1.6 (K = 2)
    and +0.6, -1.6, -1.1 (K = 8) standard errors; plain mean_j(ess_j) against
    K S / tau_b, for the record, at +6.8, +6.5, +3.3 and +4.4, +1.6, -3.7."""
    S, b, n = 1024, 16, 4096
    nb = S // b
    x = R.ar1_series(10 * K_ + int(10 * rho), S, K_, n, rho)
    acc, cg = R.fold_series(x, b)
    ess32, mcse32, summ = R.chain_ess_f32(acc["sM2"], acc["bM2"], chains=K_, chain_groups=cg, n=n,
                                          samples=S, batches=nb)
    assert (summ["n_eval"], summ["n_degenerate"], summ["n_nonfinite"]) == (n, 0, 0)
    ess64, mcse64 = R.batch_means_f64(x, b)
    x64 = x.astype(np.float64)
    s_min = x64.std(axis=0, ddof=1).min(0)
    sb_min = x64.reshape(nb, b, K_, n).mean(1).std(axis=0, ddof=1).min(0)
    m = np.abs(x64).max(axis=(0, 1))
    u = 2.0 ** -24
    bound = u * (2 * (m / sb_min) * ((S + 1) / 2 + (b + 1) / 2 + 2)
                 + 2 * (m / s_min) * ((S + 1) / 2 + 1) + S + nb + 2 * K_ + 10)
    rel = np.abs(ess32.astype(np.float64) - ess64) / ess64
    relm = np.abs(mcse32.astype(np.float64) - mcse64) / mcse64
    print(f"K={K_} rho={rho}: ess rel max {rel.max() / u:.1f} u, max err/bound "
          f"{(rel / bound).max():.2e} (bound {bound.min() / u:.0f}-{bound.max() / u:.0f} u), "
          f"mcse rel max {relm.max() / u:.1f} u")
    assert (rel <= bound).all()
    assert (relm <= bound).all()               # mcse sees half of bM2's error alone
    assert summ["ess_min"] == float(ess32.min()) and ess32[summ["argmin"]] == ess32.min()

    # the textbook estimate against the exact AR(1) value
    w = x64.var(axis=0, ddof=1).mean(0)                               # [n], mean over chains
    v = x64.reshape(nb, b, K_, n).mean(1).var(axis=0, ddof=1).mean(0)
    assert np.allclose(K_ * nb * w / v, ess64, rtol=1e-12)
    es2, evb = _ar1_expectations(rho, b, S)
    exact = R.ar1_ess(rho, b, S, K_)                                  # K S / tau_b
    expect = K_ * nb * es2 / evb
    assert abs(expect / exact - 1) < 0.025
    pooled = K_ * nb * w.mean() / v.mean()
    lin = K_ * nb * (w - (w.mean() / v.mean()) * v) / v.mean()       # the ratio, linearised
    se = lin.std(ddof=1) / math.sqrt(n)
    z_plain = (ess64.mean() - exact) / (ess64.std(ddof=1) / math.sqrt(n))
    print(f"K={K_} rho={rho}: exact {exact:.1f}, with finite-S expectations {expect:.1f}, "
          f"pooled {pooled:.1f} (z = {(pooled - expect) / se:+.2f}); plain mean "
          f"{ess64.mean():.1f} (z = {z_plain:+.2f})")
    assert abs(pooled - expect) <= 5 * se


def test_reference_conventions_degenerate_nonfinite_threshold_and_tie():
    """The reference's own conventions on a hand-made case (what the GPU test
    then demands of the device)."""
    K_, n = 2, 8
    sM2 = np.full(K_ * 8, 3.0, R.F)
    bM2 = np.zeros(K_ * 8, R.F)
    for k in range(K_):
        bM2[8 * k: 8 * k + 8] = [0.0, 1.0, 0.5, 1.0, 0.25, 2.0, np.nan, 0.0]
    sM2[8 + 5] = np.inf
    kw = dict(chains=K_, chain_groups=2, n=n, samples=13, batches=4)
    ess, mcse, s = R.chain_ess_f32(sM2, bM2, **kw)
    assert np.isnan(ess[[0, 7]]).all() and s["n_degenerate"] == 2          # SV == 0
    assert np.isinf(ess[5]) and np.isnan(ess[6]) and s["n_nonfinite"] == 2
    assert s["n_eval"] == 4 and ess[1] == ess[3] == s["ess_min"] and s["argmin"] == 1
    # per chain: w = 3/12, v = 1/3, K nb = 8 pooled over two equal chains
    assert ess[1] == np.float32(np.float32(np.float32(6 / 12) / np.float32(np.float32(2) / 3)) * 8)
    assert mcse[0] == 0.0
    thr = (float(ess[1]), float(ess[2]), 1e9)
    s2 = R.chain_ess_f32(sM2, bM2, thresholds=thr, **kw)[2]
    assert s2["n_below"] == [0, 2, 4]                      # on a threshold: not below it
    e1, _, s1 = R.chain_ess_f32(sM2[8:], bM2[8:], **dict(kw, chains=1))
    assert s1["n_eval"] == 4 and e1[1] == np.float32(np.float32(np.float32(3 / 12) /
                                                                np.float32(1 / 3)) * 4)
    empty = R.chain_ess_f32(sM2, np.zeros_like(bM2), **kw)[2]
    assert (empty["n_eval"], empty["argmin"], empty["ess_min"], empty["ess_sum"]) == (0, -1, 0.0, 0.0)


# ---------------------------------------------------------- sampler refusals
def test_sampler_refusals_before_touching_a_device(host_only):
    from bayesdll_amd import stacked
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="ess_batch must be an integer >= 0"):
            stacked.StackedSGLD(Net(), 2, _args(), ess_batch=bad)
    S0 = stacked.StackedSGLD(Net(), 2, _args())
    assert S0.ess_batch == 0 and S0._ess is None
    with pytest.raises(ValueError, match="built with ess_batch=0"):
        S0.ess()
    S = stacked.StackedCSGHMC(Net(), 3, _args(), ess_batch=4)
    assert S.ess_batch == 4 and S._ess is None                 # nothing allocated yet
    with pytest.raises(ValueError, match="nothing is folded yet"):
        S.ess()
    with pytest.raises(ValueError, match="nothing is folded yet"):
        S.ess(by_chain=True)
    with pytest.raises(ValueError, match="three finite"):
        S.ess(thresholds=(1, 2))
    SP = stacked.StackedCSGHMC(Net(), 3, _args(), ess_batch=4,
                               per_chain={"lr": [1e-2, 2e-2, 3e-2]})
    with pytest.raises(ValueError, match="per_chain hyperparameters.*different ones.*by_chain"):
        SP.ess()
    with pytest.raises(ValueError, match="nothing is folded yet"):
        SP.ess(by_chain=True)
    # counted, but fewer than two closed batches: the message names the counts
    S._ess = [{}, 7]
    with pytest.raises(ValueError, match="7 samples folded per chain close 1 batch of 4"):
        S.ess()
    # the accumulators are no part of the checkpointed state
    assert not any("ess" in k for k in S.state_dict())


def test_run_cli_ess_needs_stacked_chains(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    a = ap.parse_args(["--stacked_chains", "4", "--ess", "8", "--health", "3", "--sweep",
                       "lr=0.1,0.2,0.3,0.4", "--method", "csghmc"])
    assert (a.ess, a.health, a.sweep) == (8, 3, ["lr=0.1,0.2,0.3,0.4"])
    assert run.check_ess(ap, a) == 8 and run.parse_sweep(ap, a) is not None
    assert ap.parse_args([]).ess == 0
    with pytest.raises(SystemExit) as e:
        run.main(["--ess", "4"])
    assert e.value.code == 2
    assert "--ess folds the stacked chains' collected samples" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run.main(["--ess", "-1", "--stacked_chains", "2"])
    assert e.value.code == 2 and "B must be >= 0" in capsys.readouterr().err
