"""The statistics sweep (include/bdl_stats.h) without a GPU: the header's
surface, the C struct layouts against the ctypes mirrors, the exports, every
validation path of bdl_chain_stats (fake pointers: each call returns before
any HIP call), the Python wrapper's refusals, the temperature formulas on a
simulated quadratic, and the --health flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import chain_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

SEGMENT_FIELDS = ["grad", "numel", "grad_stride", "offset", "lr_group"]
ARGS_FIELDS = ["theta", "mom", "prior_mean", "segments", "lr_table", "acc", "workspace",
               "chain_groups", "nsegments", "chains", "lr_row_stride", "accumulate",
               "blocks_per_chain", "pad0", "lr"]
NULL, ALIGN, ARG = -1, -2, -3


def test_header_declares_two_functions_and_no_abi_version():
    text = open(os.path.join(INCLUDE, "bdl_stats.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\b(bdl_\w+)\s*\(", code) == ["bdl_chain_stats_workspace_bytes",
                                                      "bdl_chain_stats"]
    assert "BDL_ABI_VERSION" not in code and '#include "bdl_sgmcmc.h"' in code
    base = open(os.path.join(INCLUDE, "bdl_sgmcmc.h")).read()
    assert re.search(r"#define\s+BDL_ABI_VERSION\s+8\b", base)
    assert "bdl_chain_stats" not in base and "bdl_stats" not in base


def _c_layout(tmp_path):
    lines = ['printf("bdl_stats_segment %zu\\nbdl_chain_stats_args %zu\\n", '
             'sizeof(bdl_stats_segment), sizeof(bdl_chain_stats_args));',
             'printf("caps %d %d %d %lld %d\\n", BDL_STATS_MAX_SEGMENTS, BDL_STATS_MAX_CHAINS, '
             'BDL_STATS_MAX_BLOCKS_PER_CHAIN, (long long)BDL_STATS_MAX_CHAIN_GROUPS, '
             'BDL_STATS_SUMS);']
    for st, fields in (("bdl_stats_segment", SEGMENT_FIELDS),
                       ("bdl_chain_stats_args", ARGS_FIELDS)):
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_stats.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    out = subprocess.check_output([str(exe)]).decode().strip().splitlines()
    caps = [int(v) for v in next(ln for ln in out if ln.startswith("caps ")).split()[1:]]
    lay = {k: int(v) for k, v in (ln.rsplit(" ", 1) for ln in out if not ln.startswith("caps "))}
    return lay, caps


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    lay, caps = _c_layout(tmp_path)
    assert lay["bdl_stats_segment"] == C.sizeof(L.StatsSegment) == 40  # a row of five int64
    assert lay["bdl_chain_stats_args"] == C.sizeof(L.StatsArgs)
    assert [f for f, _ in L.StatsSegment._fields_] == SEGMENT_FIELDS
    assert [f for f, _ in L.StatsArgs._fields_] == ARGS_FIELDS
    for cls, name in ((L.StatsSegment, "bdl_stats_segment"), (L.StatsArgs, "bdl_chain_stats_args")):
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[f"{name}.{f}"], (name, f)
    assert caps == [L.STATS_MAX_SEGMENTS, L.STATS_MAX_CHAINS, L.STATS_MAX_BLOCKS_PER_CHAIN,
                    L.STATS_MAX_CHAIN_GROUPS, len(L.STATS_SUMS)]


def test_library_exports_the_sweep_next_to_the_pinned_abi():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.STATS_EXPORTS) == {"bdl_chain_stats", "bdl_chain_stats_workspace_bytes"}
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS, L.CHAIN_STEP_EXPORTS):
        assert not set(L.STATS_EXPORTS) & set(other)
    for name in L.STATS_EXPORTS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_stats" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "bdl_stats.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    for k, t in ((1, 1), (3, 20), (64, 6)):
        # five fp64 partials per (workgroup, segment) of the largest grid
        assert h.bdl_chain_stats_workspace_bytes(k, t) == \
            k * L.STATS_MAX_BLOCKS_PER_CHAIN * t * 5 * 8
    for k, t in ((0, 1), (1, 0), (L.STATS_MAX_CHAINS + 1, 1), (1, L.STATS_MAX_SEGMENTS + 1)):
        assert h.bdl_chain_stats_workspace_bytes(k, t) == 0


def _good_args():
    from bayesdll_amd import _lib as L
    a = L.StatsArgs()
    a.theta, a.mom, a.prior_mean = 0x100000, 0x200000, 0x300000
    a.segments, a.acc, a.workspace = 0x10008, 0x20008, 0x30000
    a.chain_groups, a.nsegments, a.chains = 9857, 19, 3
    a.lr[0], a.lr[1] = 0.05, 0.1
    return a


def test_chain_stats_validates_before_touching_the_device():
    """Every refusal of the header's list, with its status and a prefixed
    message.  No call here passes validation, so none reaches a HIP call."""
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, lr=None, **fields):
        a = _good_args()
        for k, v in fields.items():
            setattr(a, k, v)
        if lr is not None:
            a.lr[0], a.lr[1] = lr
        assert h.bdl_chain_stats(a, None) == status, (fields, lr)
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_stats:") and word in msg, (fields, lr, msg)

    assert h.bdl_chain_stats(None, None) == NULL and b"null args" in h.bdl_last_error()
    for f in ("theta", "segments", "acc", "workspace"):
        refused(NULL, f.encode(), **{f: None})
    for f in ("theta", "mom", "prior_mean", "workspace"):
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x400008})
        refused(ALIGN, f.encode() + b" not 16-B aligned", **{f: 0x400004})
    refused(ALIGN, b"segments not 8-B aligned", segments=0x10004)
    refused(ALIGN, b"acc not 8-B aligned", acc=0x20004)
    refused(ALIGN, b"lr_table not 4-B aligned", lr_table=0x50002, lr_row_stride=12, lr=(0, 0))
    for v in (0, -3, L.STATS_MAX_CHAINS + 1):
        refused(ARG, b"chains", chains=v)
    for v in (0, -1, L.STATS_MAX_SEGMENTS + 1):
        refused(ARG, b"nsegments", nsegments=v)
    for v in (0, L.STATS_MAX_CHAIN_GROUPS + 1):
        refused(ARG, b"chain_groups", chain_groups=v)
    for v in (-1, L.STATS_MAX_BLOCKS_PER_CHAIN + 1):
        refused(ARG, b"blocks_per_chain", blocks_per_chain=v)
    refused(ARG, b"both lr sources", lr_table=0x50000, lr_row_stride=12)
    refused(ARG, b"neither lr source", lr=(0, 0))
    refused(ARG, b"host lr must be > 0", lr=(0.05, 0))
    refused(ARG, b"host lr must be > 0", lr=(-0.05, 0.1))
    refused(ARG, b"host lr must be > 0", lr=(float("nan"), 0.1))
    for v in (1, 0, -12):
        refused(ARG, b"lr_row_stride", lr_table=0x50000, lr_row_stride=v, lr=(0, 0))
    for v in (2, -1):
        refused(ARG, b"accumulate", accumulate=v)


def test_chain_stats_refuses_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_chain_stats(_good_args(), None) == ARG
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_stats:") and b"graph redirect is active" in msg
        assert h.bdl_chain_stats(None, None) == ARG
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_chain_stats(None, None) == NULL  # back to ordinary validation


def test_python_wrapper_refuses_before_any_launch():
    from bayesdll_amd import kernels as K
    seg = torch.zeros(2, 5, dtype=torch.int64)
    th, acc = torch.zeros(24), torch.zeros(3, 2, 6, dtype=torch.float64)
    with pytest.raises(ValueError, match="int64 device tensor"):
        K.chain_stats(seg, 2, 3, 2, th, acc, lr=(0.1, 0.1))      # a host table: no CPU path
    with pytest.raises(ValueError, match="int64 device tensor"):
        K.chain_stats(torch.zeros(10), 2, 3, 2, th, acc, lr=(0.1, 0.1))
    assert K.stats_bytes_per_elem(mom=False) == 8 and K.stats_bytes_per_elem() == 12
    assert K.stats_bytes_per_elem(prior=True) == 16
    from bayesdll_amd import stacked
    import inspect
    assert inspect.signature(stacked._StackedSampler.__init__).parameters["health_every"].default == 0


def test_health_every_is_validated_before_the_device_is_touched():
    from types import SimpleNamespace
    from bayesdll_amd import stacked
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="health_every"):
            stacked.StackedSGLD(torch.nn.Linear(2, 2), 2, SimpleNamespace(), health_every=bad)


QUAD = dict(lr=1e-3, alpha=0.18, N=2048.0)


@pytest.fixture(scope="module")
def quadratic():
    return R.simulate_quadratic(20000, 3000, 3000, **QUAD)


def test_temperatures_are_one_on_a_stationary_quadratic(quadratic):
    """g = 3 theta, prior_sig = 1, noise every step, small lr: both
    temperatures are 1 (measured 1.0013 / 1.0009 when the formulas were
    written; the tolerance 0.02 catches a wrong factor, not noise)."""
    t = R.temperatures(quadratic, 3000, [20000], [0.18], [1.0], [2048.0], [1.0])
    print("t_kin", t["t_kin"][0, 0], "t_conf", t["t_conf"][0, 0])
    assert abs(t["t_kin"][0, 0] - 1) < 0.02
    assert abs(t["t_conf"][0, 0] - 1) < 0.02
    assert t["t_kin_chain"][0] == pytest.approx(t["t_kin"][0, 0], rel=1e-12)
    # the product's formulas are the restatement's
    from bayesdll_amd import health as H
    got = H.temperatures(quadratic, 3000, [20000], alpha=0.18, nd=1.0, N=2048.0, prior_sig=1.0)
    for k in ("t_kin", "t_conf", "t_kin_chain", "t_conf_chain"):
        np.testing.assert_allclose(got[k], t[k], rtol=1e-12)
    rr, hr = R.rms_table(quadratic, 3000, [20000]), H.rms_table(quadratic, 3000, [20000])
    for k in rr:
        np.testing.assert_allclose(hr[k], rr[k], rtol=1e-12)


def test_the_ar1_factor_is_needed(quadratic):
    """Without 1 - alpha/2 the kinetic temperature of the same run reads
    1 / (1 - 0.09) = 1.10: the check above fails without the factor."""
    t = R.temperatures(quadratic, 3000, [20000], [0.18], [1.0], [2048.0], [1.0], ar1=False)
    print("t_kin without the factor", t["t_kin"][0, 0])
    assert not abs(t["t_kin"][0, 0] - 1) < 0.02
    assert abs(t["t_kin"][0, 0] - 1 / 0.91) < 0.02


def test_zero_noise_has_no_temperature():
    from bayesdll_amd import health as H
    acc = np.ones((2, 3, 6))
    t = H.temperatures(acc, 4, [5, 6, 7], alpha=0.1, nd=[0.0, 1.0], N=64.0, prior_sig=1.0)
    assert np.isnan(t["t_kin"][0]).all() and np.isnan(t["t_conf_chain"][0])
    assert np.isfinite(t["t_kin"][1]).all() and np.isfinite(t["t_conf_chain"][1])
    r = R.temperatures(acc, 4, [5, 6, 7], [0.1] * 2, [0.0, 1.0], [64.0] * 2, [1.0] * 2)
    np.testing.assert_allclose(t["t_conf"][1], r["t_conf"][1], rtol=1e-12)


def test_cli_parses_health_and_refuses_it_without_stacked_chains(capsys):
    from bayesdll_amd.run import build_parser, check_health, main
    ap = build_parser()
    assert ap.parse_args([]).health == 0
    args = ap.parse_args(["--stacked_chains", "3", "--health", "10", "--sweep", "lr=1e-2"])
    assert check_health(ap, args) == 10
    for argv, word in ((["--health", "5"], "needs --stacked_chains"),
                       (["--stacked_chains", "2", "--health", "-1"], "must be >= 0")):
        with pytest.raises(SystemExit):
            main(argv)
        assert word in capsys.readouterr().err
