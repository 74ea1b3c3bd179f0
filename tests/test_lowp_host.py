"""The bf16-gradient step (include/bdl_lowp.h) and the bf16 compute mode without
a GPU: the header's declarations, the export table, the C struct layout against
the ctypes mirror, every validation path of bdl_lowp_step / bdl_lowp_shadow
(fake pointers: each call returns before any HIP call), the reference rounding
against torch's on the CPU, and the refusals of FlatState, the samplers and the
CLI."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import lowp_ref as LR
from test_stacked_host import Net, host_only  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NULL, ALIGN, ARG, RUNS = -1, -2, -3, -5

FIELDS = ["theta", "grad", "mom", "prior_mean", "noise", "mom1", "mom2", "shadow", "runs",
          "grad_base", "nonfinite", "n", "nruns", "method", "noise_mode", "collect", "flags",
          "blocks", "unroll", "pad0", "lr", "noise_scale", "one_minus_alpha", "prior_sig",
          "sigma2", "n_data", "mu", "collect_a", "collect_b", "inv_sigma2", "inv_n_data",
          "inv_collect_a", "inv_collect_b", "pad1", "seed", "chain", "step", "philox_offset",
          "chain_groups"]


# ------------------------------------------------------------------ the ABI
def test_header_declares_exactly_the_two_entry_points():
    text = open(os.path.join(INCLUDE, "bdl_lowp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fns = re.findall(r"^\s*(?:int|int64_t|void|const char\*)\s+(bdl_\w+)\s*\(", code, flags=re.M)
    assert sorted(fns) == ["bdl_lowp_shadow", "bdl_lowp_step"]
    assert '#include "bdl_sgmcmc.h"' in code and "BDL_ABI_VERSION" not in code  # additive
    base = open(os.path.join(INCLUDE, "bdl_sgmcmc.h")).read()
    assert "#define BDL_ABI_VERSION 8" in base and "bdl_lowp" not in base


def test_export_table_is_disjoint_and_exported():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.LOWP_EXPORTS) == {"bdl_lowp_step", "bdl_lowp_shadow"}
    others = [getattr(L, k) for k in dir(L) if k.endswith("EXPORTS") and k != "LOWP_EXPORTS"]
    assert len(others) >= 6
    for other in others:
        assert not set(L.LOWP_EXPORTS) & set(other)
    for name in L.LOWP_EXPORTS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_lowp" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "bdl_lowp.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    flags = re.search(r"^TUFLAGS_bdl_lowp := (.*)$", mk, flags=re.M).group(1).split()
    assert "-ffp-contract=off" in flags and "-DBDL_PHILOX_KEYS_PER_CALL" not in flags


def test_ctypes_mirror_matches_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    lines = ['printf("size %zu\\n", sizeof(bdl_lowp_args));',
             'printf("cap %d\\n", BDL_LOWP_MAX_BLOCKS);']
    lines += [f'printf("{f} %zu\\n", offsetof(bdl_lowp_args, {f}));' for f in FIELDS]
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_lowp.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    lay = dict(ln.rsplit(" ", 1) for ln in
               subprocess.check_output([str(exe)]).decode().strip().splitlines())
    assert int(lay["size"]) == C.sizeof(L.LowpArgs)
    assert int(lay["cap"]) == L.LOWP_MAX_BLOCKS
    assert [f for f, _ in L.LowpArgs._fields_] == FIELDS
    for f in FIELDS:
        assert getattr(L.LowpArgs, f).offset == int(lay[f]), f


def _good(method="CSGHMC", noise="PHILOX", collect="NONE"):
    from bayesdll_amd import _lib as L
    a = L.LowpArgs()
    for i, f in enumerate(("theta", "grad", "mom", "prior_mean", "noise", "mom1", "mom2",
                           "shadow", "runs")):
        setattr(a, f, 0x100000 * (i + 1))
    a.nonfinite = 0xA00004
    a.n, a.nruns, a.unroll = 39426, 19, 1
    a.method, a.noise_mode = getattr(L, method), getattr(L, "NOISE_" + noise)
    a.collect = getattr(L, "COLLECT_" + collect)
    a.collect_a = a.collect_b = 1.0
    a.seed, a.chain, a.step = 5, 2, 9
    return a


def test_lowp_step_validates_before_touching_the_device():
    """Every refusal of the header's table, with its status and a prefixed
    message.  No call here passes validation, so none reaches a HIP call."""
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, base=None, **fields):
        a = _good(**(base or {}))
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_lowp_step(a, None) == status, (fields, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_lowp_step:") and word in msg, (fields, msg)

    assert h.bdl_lowp_step(None, None) == NULL and b"null args" in h.bdl_last_error()
    # pointers
    refused(NULL, b"theta", theta=None)
    refused(NULL, b"shadow", shadow=None)
    refused(NULL, b"runs", runs=None)
    refused(NULL, b"runs", nruns=0)
    refused(NULL, b"grad or grad_base", grad=None)
    refused(NULL, b"mom is required", mom=None)
    refused(NULL, b"mom is required", base=dict(method="SGHMC"), mom=None)
    refused(NULL, b"mom is required", base=dict(method="SGLD"), mom=None, flags=L.FLAG_MOMENTUM)
    refused(NULL, b"prior_mean", base=dict(method="SGLD"), prior_mean=None)
    refused(NULL, b"prior_mean", base=dict(method="SGHMC"), prior_mean=None)
    refused(NULL, b"noise buffer", base=dict(noise="BUFFER"), noise=None)
    refused(NULL, b"mom1 is required", base=dict(collect="WELFORD"), mom1=None)
    refused(NULL, b"mom1 is required", base=dict(method="SGLD", collect="MEAN_INIT"), mom1=None)
    # alignment: 16 B for the fp32 vectors, 8 B for shadow, grad and the base table
    for f in ("theta", "mom", "prior_mean", "noise", "mom1", "mom2"):
        refused(ALIGN, b"fp32 vector not 16-B aligned", **{f: 0x100008})
        refused(ALIGN, b"fp32 vector not 16-B aligned", **{f: 0x100004})
    refused(ALIGN, b"shadow not 8-B aligned", shadow=0x800004)
    refused(ALIGN, b"shadow not 8-B aligned", shadow=0x800002)
    refused(ALIGN, b"grad not 8-B aligned", grad=0x200004)
    refused(ALIGN, b"grad_base not 8-B aligned", grad_base=0xC00004)
    # out of scope
    for m in (L.SGHMC_GRAD, L.SGLD_GRAD, L.ADAM_SGHMC, L.ADAM_SGHMC_GRAD, 9, -1):
        refused(ARG, b"method must be BDL_CSGHMC, BDL_SGHMC or BDL_SGLD", method=m)
    refused(ARG, b"BDL_FLAG_GRAD_READY", base=dict(method="SGLD"), flags=L.FLAG_GRAD_READY)
    refused(ARG, b"no clipped", flags=L.FLAG_GRAD_READY | L.FLAG_MOMENTUM)
    refused(ARG, b"unknown flag", flags=0x10)
    refused(ARG, b"unknown noise mode", noise_mode=3)
    refused(ARG, b"unknown noise mode", noise_mode=-1)
    refused(ARG, b"unknown collect mode", collect=5)
    refused(ARG, b"unknown collect mode", collect=-1)
    for u in (0, 3, 5, 8, -1):
        refused(ARG, b"unroll must be 1, 2 or 4", unroll=u)
    refused(ARG, b"blocks in [0, 65536]", blocks=-1)
    refused(ARG, b"blocks in [0, 65536]", blocks=L.LOWP_MAX_BLOCKS + 1)
    refused(ARG, b"n must be >= 1", n=0)
    refused(ARG, b"n must be >= 1", n=-4)
    refused(RUNS, b"64 KiB", nruns=4097)
    refused(RUNS, b"2730 with grad_base", nruns=2731, grad_base=0xC00008)
    # the Philox 2^32 limits
    refused(ARG, b"float4 group index", n=4 * (1 << 32))
    refused(ARG, b"float4 group index", philox_offset=(1 << 32) - 100)
    refused(ARG, b"float4 group index", base=dict(noise="NONE"), chain_groups=1 << 32)
    refused(ARG, b"chain id below 2^32", chain=1 << 32)
    refused(ARG, b"chain id below 2^32", chain=(1 << 32) - 3, chain_groups=9857 // 3 + 1)
    # combinations without a kernel
    refused(ARG, b"no kernel", base=dict(method="SGLD", noise="NONE"))
    refused(ARG, b"no kernel", base=dict(method="SGLD", collect="WELFORD"))
    refused(ARG, b"no kernel", base=dict(collect="MEAN"))


def test_lowp_shadow_validates_before_touching_the_device():
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, *args):
        assert h.bdl_lowp_shadow(*args, None) == status, (args, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_lowp_shadow:") and word in msg, msg

    refused(NULL, b"theta", None, 0x200000, None, 0, 100)
    refused(NULL, b"shadow", 0x100000, None, None, 0, 100)
    refused(ARG, b"n must be >= 1", 0x100000, 0x200000, None, 0, 0)
    refused(ARG, b"nruns", 0x100000, 0x200000, None, -1, 100)
    refused(ALIGN, b"theta not 16-B", 0x100008, 0x200000, None, 0, 100)
    refused(ALIGN, b"shadow not 8-B", 0x100000, 0x200004, None, 0, 100)


def test_entry_points_refuse_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x1000), C.c_void_p(0x2000)) == 0
    try:
        assert h.bdl_lowp_step(_good(), None) == ARG
        assert b"graph redirect" in h.bdl_last_error()
        assert h.bdl_lowp_shadow(0x100000, 0x200000, None, 0, 100, None) == ARG
        assert h.bdl_last_error().startswith(b"bdl_lowp_shadow:")
        assert b"graph redirect" in h.bdl_last_error()
    finally:
        h.bdl_graph_redirect(None, None)


# ------------------------------------------------------------- the rounding
def test_reference_rounding_is_torchs_bfloat16_cast():
    x = LR.rounding_inputs()
    assert x.size > 4000 and not np.isnan(x).any()
    got = LR.bf16_encode(x)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    one = lambda b: LR.bf16_encode(np.array([b], dtype=np.uint32).view(np.float32))[0]  # noqa: E731
    assert one(0x3F808000) == 0x3F80 and one(0x3F818000) == 0x3F82  # ties, to even both ways
    assert one(0x3F807FFF) == 0x3F80 and one(0x3F808001) == 0x3F81  # one ulp either side
    assert one(0x7F7FFFFF) == 0x7F80 and one(0xFF7FFFFF) == 0xFF80  # the maximum -> inf
    assert one(0x00000000) == 0x0000 and one(0x80000000) == 0x8000
    assert one(0x00018000) == 0x0002 and one(0x00008000) == 0x0000  # subnormals kept, ties even
    assert one(0x007FFFFF) == 0x0080                                # up to the smallest normal
    nan = LR.bf16_encode(np.array([0x7FC00000, 0xFFFFFFFF, 0x7F800001], dtype=np.uint32)
                         .view(np.float32))
    assert LR.bf16_is_nan(nan).all()
    assert np.array_equal(LR.bf16_decode(got).view(np.uint32), got.astype(np.uint32) << 16)


# ---------------------------------------------------------------- refusals
class BNNet(nn.Module):
    readout_name = "head"

    def __init__(self):
        super().__init__()
        self.body = nn.Linear(13, 7)
        self.bn = nn.BatchNorm1d(7)
        self.head = nn.Linear(7, 5)


def test_flatstate_refuses_what_bf16_compute_does_not_cover(host_only, monkeypatch):
    from bayesdll_amd import flat
    with pytest.raises(ValueError, match="compute_dtype must be fp32 or bf16"):
        flat.FlatState(Net(), compute_dtype=torch.float16)
    with pytest.raises(ValueError, match="flat gradient vector"):
        flat.FlatState(Net(), compute_dtype=torch.bfloat16, grad_mode="flat")
    monkeypatch.setenv("BDL_GRAD_MODE", "flat")
    with pytest.raises(ValueError, match="flat gradient vector"):
        flat.FlatState(Net(), compute_dtype=torch.bfloat16)
    monkeypatch.delenv("BDL_GRAD_MODE")
    monkeypatch.setattr(flat, "MAX_TENSOR_RUNS", 3)
    with pytest.raises(ValueError, match="one run per tensor"):
        flat.FlatState(Net(), compute_dtype=torch.bfloat16)
    monkeypatch.setattr(flat, "MAX_TENSOR_RUNS", 2730)
    monkeypatch.setenv("BDL_GRAD_ARENA", "1")
    with pytest.raises(ValueError, match="gradient arena"):
        flat.FlatState(Net(), compute_dtype=torch.bfloat16)
    monkeypatch.delenv("BDL_GRAD_ARENA")
    net = BNNet()
    with pytest.raises(ValueError, match="floating-point buffers"):
        flat.FlatState(net, compute_dtype=torch.bfloat16)
    assert all(p.dtype == torch.float32 for p in net.parameters())  # refused before rebinding


def _args(**kw):
    a = SimpleNamespace(lr=5e-2, lr_head=1e-1, epochs=2, num_cycles=2, momentum=0.0,
                        proportion_exploration=0.5, ND=64, device="cpu", seed=7, pretrained=None,
                        log_dir=None, clip_grad=None, compute_dtype="bf16",
                        hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0,
                                 "nd": 1.0, "thin": 1, "nst": 0, "bias": "informative",
                                 "burnin": 0})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_samplers_refuse_what_bf16_compute_does_not_cover(host_only, monkeypatch, tmp_path):
    import logging
    from bayesdll_amd import _lib as L
    from bayesdll_amd import (adam_csghmc, adam_sghmc, csghmc, csgld, kernels, sgld, stacked)
    log = logging.getLogger("lowp-host")
    for mod in (adam_sghmc, adam_csghmc):
        with pytest.raises(ValueError, match="compute_dtype=bf16 is not supported by .*adam"):
            mod.Runner(Net(), None, _args(log_dir=str(tmp_path)), log)
    with pytest.raises(ValueError, match="clip_grad"):
        csgld.Runner(Net(), None, _args(log_dir=str(tmp_path), clip_grad=1.0), log)
    for cls in (stacked.StackedCSGHMC, stacked.StackedSGLD):
        with pytest.raises(ValueError, match="stacked samplers"):
            cls(Net(), 2, _args(), init="reinit", seed=1)
    for extra, word in ((dict(graph=True), "graph mode"), (dict(overlap=True), "overlapped")):
        with pytest.raises(ValueError, match=word):
            csghmc.Runner(Net(), None, _args(log_dir=str(tmp_path), **extra), log)
    # accepted: the Model carries the mode; fp32 stays the default
    r = sgld.Runner(Net(), None, _args(log_dir=str(tmp_path)), log)
    assert r.model.compute_dtype is torch.bfloat16
    r = sgld.Runner(Net(), None, _args(log_dir=str(tmp_path), compute_dtype=None), log)
    assert r.model.compute_dtype is None
    monkeypatch.setenv("BDL_COMPUTE_DTYPE", "bf16")
    assert csghmc.Model(ND=10).compute_dtype is torch.bfloat16
    monkeypatch.delenv("BDL_COMPUTE_DTYPE")
    assert csghmc.Model(ND=10).compute_dtype is None
    # an explicit fp32 overrides the environment; no argument leaves it in force
    monkeypatch.setenv("BDL_COMPUTE_DTYPE", "bf16")
    r = sgld.Runner(Net(), None, _args(log_dir=str(tmp_path), compute_dtype="fp32"), log)
    assert r.model.compute_dtype is None
    r = sgld.Runner(Net(), None, _args(log_dir=str(tmp_path), compute_dtype=None), log)
    assert r.model.compute_dtype is torch.bfloat16
    monkeypatch.delenv("BDL_COMPUTE_DTYPE")
    # the *_GRAD contract (Model.forward without sgd) and the clipped step are
    # refused by the Model before the state is built or the network rebound
    from bayesdll_amd import sghmc
    x, y, crit = torch.randn(4, 13), torch.randint(0, 5, (4,)), torch.nn.CrossEntropyLoss()
    for mod in (sgld, sghmc):
        net, m = Net(), mod.Model(ND=10)
        m.compute_dtype = torch.bfloat16
        with pytest.raises(ValueError, match="GRAD contract"):
            m(x, y, net, Net(), crit, [0.1, 0.1])
        assert m.flat is None and all(p.dtype == torch.float32 for p in net.parameters())
    m = sgld.Model(ND=10)
    m.compute_dtype = torch.bfloat16
    with pytest.raises(ValueError, match="clip_grad"):
        m(x, y, Net(), Net(), crit, [0.1, 0.1], sgd=object(), clip_grad=1.0)
    assert m.flat is None
    # the *_GRAD contract and the clipped step have no bf16 form
    st = SimpleNamespace(shadow=torch.zeros(4, dtype=torch.bfloat16))
    for m in (L.SGLD_GRAD, L.SGHMC_GRAD):
        with pytest.raises(ValueError, match="GRAD contract"):
            kernels.lowp_args(st, m, lrs=(0.1, 0.1), noise_scale=(0, 0), noise_mode=L.NOISE_PHILOX)


def test_cli_parses_compute_dtype_and_refuses_it_with_stacked_chains(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    base = ["--method", "csghmc", "--dataset", "mnist", "--backbone", "mlp_mnist"]
    try:
        args = ap.parse_args(base)
    except SystemExit:  # other required options: parse only what this test is about
        base = []
        args = ap.parse_known_args(base)[0]
    assert args.compute_dtype is None  # fp32, unless BDL_COMPUTE_DTYPE says otherwise
    assert ap.parse_known_args(base + ["--compute_dtype", "fp32"])[0].compute_dtype == "fp32"
    args = ap.parse_known_args(base + ["--compute_dtype", "bf16"])[0]
    assert args.compute_dtype == "bf16" and run.check_compute_dtype(ap, args) == "bf16"
    with pytest.raises(SystemExit):
        ap.parse_known_args(base + ["--compute_dtype", "fp16"])
    args = ap.parse_known_args(base + ["--compute_dtype", "bf16", "--stacked_chains", "2"])[0]
    with pytest.raises(SystemExit):
        run.check_compute_dtype(ap, args)
    assert "stacked samplers have no bf16 step" in capsys.readouterr().err
