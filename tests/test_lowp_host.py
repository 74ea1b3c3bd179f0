"""The bf16-gradient step (include/bdl_lowp.h) and the bf16 compute mode without
a GPU: the header's declarations, the export table, the C struct layout against
the ctypes mirror, every validation path of bdl_lowp_step / bdl_lowp_shadow
(fake pointers: each call returns before any HIP call), the reference rounding
against torch's on the CPU, and the refusals of FlatState, the samplers and the
CLI.

And what the bf16 step's GPU tests rely on, proven on the CPU (the second half
of this file): lowp_ref.classify restates the sweep of bdl_lowp.hip (full or
guarded iteration, kVec / kElem / kNone per float4 group and the reason of
every kElem) and is itself checked on hand-written tables with literal
answers; table D (lowp_ref.TableD) at the instance tests' grid, and tables B
and C at the stacked tests' geometry, reach the conditions those tests claim,
at every depth, for the flat gradient and for the per-tensor base table.
These are conditions, not measurements: a change of table, grid or sweep that
loses one fails here.  Also: the library holds exactly the kernel instances
the instance tests launch (by name)."""
import ctypes as C
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import lowp_ref as LR
import stacked_tables as ST
import step_ref as SR
from test_gpu_noise_units import SEGMENTS
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


# ===================================================== the sweep, classified
D = LR.TableD
DEPTHS = [1, 2, 4]
MODES = {"flat": None, "bases": D.PHASES}
VEC, ELEM, NONE = LR.K_VEC, LR.K_ELEM, LR.K_NONE
PRIOR, SKIP = SR.ATTR_PRIOR, SR.ATTR_SKIP


# ------------------------------------------------------------- the classifier
def test_classifier_on_hand_written_tables():
    # 1. one tensor of 2 x 1024 + 6 elements, depth 1, one workgroup: two full
    #    iterations of vector groups, then the guarded one: one whole group,
    #    the tail group (2 elements), 254 lanes past the end
    it = LR.classify([0], [2054], [PRIOR], None, 2054, 1, 1)
    assert [(i.wg, i.index, i.gb, i.full) for i in it] == [(0, 0, 0, True), (0, 1, 256, True),
                                                           (0, 2, 512, False)]
    assert all((i.kind == VEC).all() for i in it[:2])
    assert it[2].kind.tolist() == [VEC, ELEM] + [NONE] * 254
    assert it[2].reason.tolist() == [0, LR.R_TAIL] + [0] * 254
    # 2. two workgroups at depth 2 over 4096 + 2048 elements: grid-stride order
    it = LR.classify([0], [6144], [PRIOR], None, 6144, 2, 2)
    assert [(i.wg, i.index, i.gb, i.full) for i in it] == [(0, 0, 0, True), (0, 1, 1024, True),
                                                           (1, 0, 512, True)]
    # 3. 16 elements in 4 groups: a boundary at 6 (inside group 1), a SKIP
    #    tensor [8, 12), then a tensor whose base is 2 B off; per-tensor runs
    args = ([0, 6, 8, 12], [6, 2, 4, 4], [PRIOR, 0, PRIOR | SKIP, PRIOR])
    k = LR.classify(*args, [0, 0, 0, 2], 16, 1, 1)[0]
    assert not k.full  # 4 groups are no whole iteration
    assert k.kind.tolist()[:5] == [VEC, ELEM, ELEM, ELEM, NONE]
    assert k.reason.tolist()[:4] == [0, LR.R_BOUNDARY, LR.R_SKIP, LR.R_BASE]
    #    the flat gradient: the last tensor is a vector group
    k = LR.classify(*args, None, 16, 1, 1)[0]
    assert k.kind.tolist()[:4] == [VEC, ELEM, ELEM, VEC]
    # 4. flat runs merge equal neighbours (no boundary at 6), per-tensor runs do not
    args = ([0, 6], [6, 1018], [PRIOR, PRIOR])
    assert LR.classify(*args, None, 1024, 1, 1)[0].kind.tolist() == [VEC] * 256
    k = LR.classify(*args, [0, 0], 1024, 1, 1)[0]
    assert k.full and k.kind.tolist() == [VEC, ELEM] + [VEC] * 254
    # 5. a gap between tensors and the rest up to n are SKIP runs (a stacked slot's padding)
    k = LR.classify([0, 8], [6, 4], [PRIOR, PRIOR], None, 16, 1, 1)[0]
    assert k.kind.tolist()[:4] == [VEC, ELEM, VEC, ELEM]
    assert k.reason.tolist()[:4] == [0, LR.R_BOUNDARY, 0, LR.R_SKIP]


def test_run_table_equals_bdl_build_runs_and_attrs_equal_segment_attrs():
    from bayesdll_amd.flat import build_runs, segment_attrs
    assert D.attrs == segment_attrs(D.names, "head", "uninformative",
                                    [nm not in D.FROZEN for nm in D.names])
    for lay in (ST.table_a(), ST.table_b(), ST.table_c()):
        segs = lay.stacked_segments()
        o, k, a = ([s[i] for s in segs] for i in range(3))
        ends, attrs = LR.run_table(o, k, a, lay.n)
        assert np.column_stack([ends, attrs]).tolist() == lay.flat_runs().tolist()
    ends, attrs = LR.run_table(D.offsets, D.numels, D.attrs, D.n)
    assert np.column_stack([ends, attrs]).tolist() == \
        build_runs(D.offsets, D.numels, D.attrs, D.n).tolist()
    ends, _ = LR.run_table(D.offsets, D.numels, D.attrs, D.n, per_tensor=True)
    assert ends.tolist() == [o + k for o, k in zip(D.offsets, D.numels)]


def test_table_d_layout():
    assert (D.n, D.n % 4, len(D.SEGMENTS)) == (13530, 2, 14)
    live = [p for p, a in zip(D.PHASES, D.attrs) if not a & SKIP]
    assert set(live) == {0, 2, 4, 6} and D.PHASES[0] == 0  # every phase, not on the first tensor
    assert all(p == 0 for p, a in zip(D.PHASES, D.attrs) if a & SKIP)
    # a tensor at an odd offset whose base is 8-B addressable all the same
    i = D.names.index("l4.weight")
    assert D.offsets[i] % 4 == 3 and D.PHASES[i] == 0


# --------------------------------------------- table D at the instance tests' grid
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("depth", DEPTHS)
def test_table_d_reaches_every_path_at_the_tests_grid(depth, mode):
    it = LR.classify(D.offsets, D.numels, D.attrs, MODES[mode], D.n, D.BLOCKS, depth)
    # the cursor is carried between full iterations of one workgroup
    assert any(sum(1 for i in it if i.wg == w and i.full) >= 2 for w in range(D.BLOCKS))
    # and from a full iteration into the guarded one
    guarded = [i for i in it if not i.full]
    assert len(guarded) == 1 and guarded[0].index >= 1
    # one full iteration with vector groups and element-wise groups of every
    # reason the mode can have: the flat gradient has one 8-B aligned base
    # (bdl_lowp_step refuses another), so R_BASE cannot occur there
    reasons = [LR.R_BOUNDARY, LR.R_SKIP] + ([LR.R_BASE] if mode == "bases" else [])
    rich = [i for i in it if i.full and i.has(VEC) and all(i.has(ELEM, r) for r in reasons)]
    assert rich and rich[0].gb <= 512 < rich[0].gb + 256 * depth  # elements [2048, 3072)
    if mode == "flat":
        assert not any(i.has(ELEM, LR.R_BASE) for i in it)
    else:  # every odd phase is read element by element in a full iteration
        ends = np.cumsum(D.numels)
        for t, p in enumerate(D.PHASES):
            if p:
                g = (D.offsets[t] + 3) // 4  # the tensor's first whole group
                own = [i for i in it if i.full and i.gb <= g < i.gb + i.kind.size]
                assert own and own[0].reason[g - own[0].gb] & LR.R_BASE, (t, p)
                assert ends[t] - D.offsets[t] >= 8
    # the guarded iteration holds all three kinds, an odd boundary, a SKIP run and the tail
    g = guarded[0]
    assert g.has(VEC) and g.has(ELEM) and g.has(NONE)
    assert g.has(ELEM, LR.R_BOUNDARY) and g.has(ELEM, LR.R_SKIP) and g.has(ELEM, LR.R_TAIL)
    assert sum(int(((i.reason & LR.R_TAIL) != 0).sum()) for i in it) == 1
    # every group exactly once
    seen = np.concatenate([i.gb + np.flatnonzero(i.kind != NONE) for i in it])
    assert sorted(seen.tolist()) == list(range((D.n + 3) // 4))


@pytest.mark.parametrize("depth", DEPTHS)
def test_default_grids_give_every_workgroup_one_iteration(depth):
    """blocks = 0 on these tables (256 CUs or more, 2 workgroups per CU): as
    many workgroups as iterations, so no cursor is carried there — why the
    instance tests also run a literal grid of 2."""
    for n in (D.n, int(sum(k for _, k in SEGMENTS))):
        grid = LR.default_grid(n, depth, 256)
        it = LR.classify([0], [n], [PRIOR], None, n, grid, depth)
        assert len(it) == grid and all(i.index == 0 for i in it)


def test_the_older_table_misses_the_combined_condition():
    """Why table D exists: on the 39,426-element table the only run boundary
    that is no multiple of 4 (16,295) and the frozen tensor never share an
    iteration, at any depth."""
    names = [nm for nm, _ in SEGMENTS]
    numels = [k for _, k in SEGMENTS]
    offsets = np.concatenate([[0], np.cumsum(numels)[:-1]]).astype(int).tolist()
    attrs = LR._attrs_of(names, ("l7.weight",))
    for depth in DEPTHS:
        it = LR.classify(offsets, numels, attrs, None, sum(numels), 2, depth)
        assert not any(i.has(ELEM, LR.R_BOUNDARY) and i.has(ELEM, LR.R_SKIP) for i in it if i.full)


# -------------------------------------------------------- the adversarial sites
def test_adversarial_sites_lie_where_the_test_says():
    for depth in (1, 4):
        for mode, bases in MODES.items():
            it = LR.classify(D.offsets, D.numels, D.attrs, bases, D.n, D.BLOCKS, depth)

            def at(e):
                i = [x for x in it if x.gb <= e // 4 < x.gb + x.kind.size][0]
                return i.full, int(i.kind[e // 4 - i.gb])

            assert all(at(e) == (True, VEC) for e in D.SITE_VEC)
            assert all(at(e) == (True, ELEM) for e in D.SITE_ELEM)
            if mode == "bases":
                assert all(at(e) == (True, ELEM) for e in D.SITE_ELEM_BASES)
            assert all(at(e) == (False, VEC) for e in D.SITE_GUARDED_VEC)
            assert all(at(e) == (False, ELEM) for e in D.SITE_GUARDED_ELEM)
    attr = SR.element_attrs(D.numels, D.attrs)
    sites = D.SITE_VEC + D.SITE_ELEM + D.SITE_ELEM_BASES + D.SITE_GUARDED_VEC + D.SITE_GUARDED_ELEM
    assert len(set(sites)) == len(sites) and not (attr[sites] & SKIP).any()


# ------------------------------------------------ tables B and C, stacked tests
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("table", ["b", "c"])
def test_seamless_tables_put_two_chains_into_one_wave_of_a_full_iteration(table, depth):
    lay = {"b": ST.table_b, "c": ST.table_c}[table]()
    segs = lay.stacked_segments()
    o, k, a = ([s[i] for s in segs] for i in range(3))
    it = LR.classify(o, k, a, None, lay.n, LR.STACKED_BLOCKS, depth)
    split = [i for i in it if i.full and LR.waves_in_two_chains(i, lay.chain_groups)]
    assert split, (table, depth)
    # those waves take the vector path: the seam is no kElem group
    for i in split:
        for w in LR.waves_in_two_chains(i, lay.chain_groups):
            assert (i.kind[64 * w:64 * w + 64] == VEC).all()
    assert lay.chain_groups % 64  # a seam never falls on a wave boundary
    assert any(sum(1 for i in it if i.wg == w and i.full) >= 2 for w in range(LR.STACKED_BLOCKS))


# ------------------------------------------------------------ the built instances
def test_the_library_holds_exactly_the_instances_the_matrix_launches():
    """Names only: the set of bdl_lowp_kernel<method, noise, collect, unroll>
    in the built library equals the instance tests' matrix, so a newly built
    instance cannot go untested (nor a tested one vanish)."""
    from bayesdll_amd import _lib as L
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    assert os.path.exists(L.LIB_PATH), "build the library first"
    out = subprocess.run([nm, "-C", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    built = {tuple(int(x) for x in m.groups())
             for m in re.finditer(r"bdl_lowp_kernel<(\d+), (\d+), (\d+), (\d+)>", out)}
    noise = {"none": L.NOISE_NONE, "buffer": L.NOISE_BUFFER, "philox": L.NOISE_PHILOX}
    want = {(getattr(L, m.upper()), noise[nz], getattr(L, "COLLECT_" + c), u)
            for m, nz, c, _mom in LR.INSTANCE_CASES for u in LR.UNROLLS}
    assert built == want
    assert len(want) == 63 and len(LR.INSTANCE_CASES) * len(LR.UNROLLS) == 99
