"""The per-chain step (include/bdl_chain_step.h) and the per_chain sampler
layer without a GPU: the header's declarations, the export table, the C struct
layouts against the ctypes mirrors, every validation path of bdl_chain_step
(fake pointers: each call returns before any HIP call), the expansion of a
per_chain table into scalar rows against a float64 restatement of the uniform
samplers' update() formulas, uniform rows against the scalars the uniform
launch gets, and the refusals of the samplers and of the CLI."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_stacked_host import Net, host_only  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NULL, ALIGN, ARG, RUNS = -1, -2, -3, -5

SCALAR_FIELDS = ["lr", "noise_scale", "one_minus_alpha", "prior_sig", "sigma2", "n_data", "mu",
                 "inv_sigma2", "inv_n_data", "pad"]
ARGS_FIELDS = ["theta", "grad", "mom", "prior_mean", "noise", "mom1", "mom2", "nonfinite", "runs",
               "grad_base", "scalars", "n1", "chain_groups", "nruns", "chains", "method",
               "noise_mode", "collect", "flags", "blocks_per_chain", "unroll",
               "nonfinite_per_chain", "pad0", "collect_a", "collect_b", "inv_collect_a",
               "inv_collect_b", "seed", "chain", "step"]


# ------------------------------------------------------------------ the ABI
def test_header_declares_exactly_the_step_and_its_helper():
    text = open(os.path.join(INCLUDE, "bdl_chain_step.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fns = re.findall(r"^\s*(?:int|int64_t|void|const char\*)\s+(bdl_\w+)\s*\(", code, flags=re.M)
    assert sorted(fns) == ["bdl_chain_step", "bdl_chain_step_unroll_ok"]
    assert '#include "bdl_sgmcmc.h"' in code and "BDL_ABI_VERSION" not in code  # additive
    base = open(os.path.join(INCLUDE, "bdl_sgmcmc.h")).read()
    assert "#define BDL_ABI_VERSION 8" in base and "bdl_chain_step" not in base


def test_export_table_is_disjoint_and_exported():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.CHAIN_STEP_EXPORTS) == {"bdl_chain_step", "bdl_chain_step_unroll_ok"}
    for other in (L.EXPORTS, L.DIAG_EXPORTS, L.CLIP_EXPORTS):
        assert not set(L.CHAIN_STEP_EXPORTS) & set(other)
    for name in L.CHAIN_STEP_EXPORTS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_chain_step" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "bdl_chain_step.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    # the unit must not re-read its arguments from the kernarg segment
    flags = re.search(r"^TUFLAGS_bdl_chain_step := (.*)$", mk, flags=re.M).group(1)
    assert "-DBDL_PHILOX_KEYS_PER_CALL" not in flags.split()


def _c_layout(tmp_path):
    lines = ['printf("bdl_chain_scalars %zu\\nbdl_chain_step_args %zu\\n", '
             'sizeof(bdl_chain_scalars), sizeof(bdl_chain_step_args));',
             'printf("caps %d %d %d %d\\n", BDL_CHAIN_STEP_MAX_CHAINS, '
             'BDL_CHAIN_STEP_MAX_BLOCKS_PER_CHAIN, BDL_CHAIN_STEP_MAX_RUNS, '
             'BDL_CHAIN_STEP_MAX_RUNS_BASES);']
    for st, fields in (("bdl_chain_scalars", SCALAR_FIELDS), ("bdl_chain_step_args", ARGS_FIELDS)):
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_chain_step.h\"\n"
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
    assert lay["bdl_chain_scalars"] == C.sizeof(L.ChainScalars) == 48  # a row of 12 floats
    assert lay["bdl_chain_step_args"] == C.sizeof(L.ChainStepArgs)
    assert [f for f, _ in L.ChainScalars._fields_] == SCALAR_FIELDS
    assert [f for f, _ in L.ChainStepArgs._fields_] == ARGS_FIELDS
    for cls, name in ((L.ChainScalars, "bdl_chain_scalars"), (L.ChainStepArgs, "bdl_chain_step_args")):
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[f"{name}.{f}"], (name, f)
    assert caps == [L.CHAIN_STEP_MAX_CHAINS, L.CHAIN_STEP_MAX_BLOCKS_PER_CHAIN,
                    L.CHAIN_STEP_MAX_RUNS, L.CHAIN_STEP_MAX_RUNS_BASES]
    # the row's columns in the order the Python layer fills them
    assert len(L.CHAIN_SCALAR_COLUMNS) == 12
    assert [getattr(L.ChainScalars, f).offset // 4 for f in
            ("lr", "noise_scale", "one_minus_alpha", "prior_sig", "sigma2", "n_data", "mu",
             "inv_sigma2", "inv_n_data")] == [0, 2, 4, 5, 6, 7, 8, 9, 10]


def _good_args(method="CSGHMC", noise="PHILOX", collect="NONE"):
    from bayesdll_amd import _lib as L
    a = L.ChainStepArgs()
    for i, f in enumerate(("theta", "grad", "mom", "prior_mean", "noise", "mom1", "mom2")):
        setattr(a, f, 0x100000 * (i + 1))
    a.nonfinite, a.runs, a.scalars = 0x900004, 0xA00008, 0xB00010
    a.n1, a.chain_groups, a.nruns, a.chains = 39426, 9857, 19, 3
    a.method, a.noise_mode = getattr(L, method), getattr(L, "NOISE_" + noise)
    a.collect = getattr(L, "COLLECT_" + collect)
    a.collect_a = a.collect_b = 1.0
    a.seed, a.chain, a.step = 5, 2, 9
    return a


def test_chain_step_validates_before_touching_the_device():
    """Every refusal of the header's table, with its status and a prefixed
    message.  No call here passes validation, so none reaches a HIP call."""
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, base=None, **fields):
        a = _good_args(**(base or {}))
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_chain_step(a, None) == status, (fields, h.bdl_last_error())
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_step:") and word in msg, (fields, msg)

    assert h.bdl_chain_step(None, None) == NULL and b"null args" in h.bdl_last_error()
    # pointers
    refused(NULL, b"theta", theta=None)
    refused(NULL, b"runs", runs=None)
    refused(NULL, b"scalars", scalars=None)
    refused(NULL, b"grad or grad_base", grad=None)
    refused(NULL, b"mom is required", mom=None)
    refused(NULL, b"mom is required", base=dict(method="SGLD"), mom=None, flags=L.FLAG_MOMENTUM)
    refused(NULL, b"prior_mean", base=dict(method="SGLD"), prior_mean=None)
    refused(NULL, b"noise buffer", base=dict(noise="BUFFER"), noise=None)
    refused(NULL, b"mom1 is required", base=dict(collect="WELFORD"), mom1=None)
    refused(NULL, b"mom1 is required", base=dict(method="SGLD", collect="MEAN_INIT"), mom1=None)
    for f in ("theta", "grad", "mom", "prior_mean", "noise", "mom1", "mom2"):
        refused(ALIGN, b"vector not 16-B aligned", **{f: 0x100008})
    refused(ALIGN, b"scalars not 16-B aligned", scalars=0xB00008)
    refused(ALIGN, b"runs not 8-B aligned", runs=0xA00004)
    refused(ALIGN, b"grad_base not 8-B aligned", grad_base=0xC00004)
    refused(ALIGN, b"nonfinite not 4-B aligned", nonfinite=0x900002)
    # sizes
    for k in (0, -1, L.CHAIN_STEP_MAX_CHAINS + 1):
        refused(ARG, b"chains in [1, 65535]", chains=k)
    refused(ARG, b"n1 in [1, 4 * chain_groups]", n1=0)
    refused(ARG, b"n1 in [1, 4 * chain_groups]", n1=-4)
    refused(ARG, b"n1 in [1, 4 * chain_groups]", n1=4 * 9857 + 1)
    refused(ARG, b"n1 in [1, 4 * chain_groups]", chain_groups=0)
    refused(RUNS, b"nruns in [1, 4096]", nruns=0)
    refused(RUNS, b"nruns in [1, 4096]", nruns=4097)
    refused(RUNS, b"2730 with grad_base", nruns=2731, grad_base=0xC00008)
    # the method / noise / collect table
    for m in (L.SGHMC, L.SGHMC_GRAD, L.SGLD_GRAD, L.ADAM_SGHMC, L.ADAM_SGHMC_GRAD, 9, -1):
        refused(ARG, b"method must be BDL_CSGHMC or BDL_SGLD", method=m)
    refused(ARG, b"unknown noise mode", noise_mode=3)
    refused(ARG, b"unknown noise mode", noise_mode=-1)
    refused(ARG, b"BDL_SGLD needs", base=dict(method="SGLD"), noise_mode=L.NOISE_NONE)
    for c in (L.COLLECT_MEAN_INIT, L.COLLECT_MEAN, 5, -1):
        refused(ARG, b"collect must be", collect=c)
    for c in (L.COLLECT_WELFORD_INIT, L.COLLECT_WELFORD):
        refused(ARG, b"collect must be", base=dict(method="SGLD"), collect=c)
    refused(ARG, b"BDL_FLAG_GRAD_READY", flags=L.FLAG_GRAD_READY)
    refused(ARG, b"BDL_FLAG_GRAD_READY", base=dict(method="SGLD"),
            flags=L.FLAG_GRAD_READY | L.FLAG_MOMENTUM)
    refused(ARG, b"unknown flag", flags=0x10)
    refused(ARG, b"nonfinite_per_chain", nonfinite_per_chain=2)
    # Philox ranges: the group index inside a chain and chain + chains below 2^32
    refused(ARG, b"float4 group index", n1=4 * (1 << 32) + 1, chain_groups=(1 << 32) + 1)
    refused(ARG, b"chain id below 2^32", chain=1 << 32)
    refused(ARG, b"chain id below 2^32", chain=(1 << 32) - 3)          # + 3 chains reaches 2^32
    refused(ARG, b"blocks_per_chain", blocks_per_chain=-1)
    refused(ARG, b"blocks_per_chain", blocks_per_chain=L.CHAIN_STEP_MAX_BLOCKS_PER_CHAIN + 1)
    for u in (-1, 3, 8):
        refused(ARG, b"unroll is 0, 1, 2 or 4", unroll=u)
    # depths at which the production body would re-read the kernarg segment do not exist
    refused(ARG, b"no kernel instance at this unroll", base=dict(method="SGLD", noise="BUFFER"),
            unroll=2)
    refused(ARG, b"no kernel instance at this unroll", base=dict(method="SGLD", collect="MEAN"),
            unroll=4)


def test_unroll_depths_on_offer():
    from bayesdll_amd import _lib as L
    ok = L.lib().bdl_chain_step_unroll_ok
    for noise in (L.NOISE_NONE, L.NOISE_BUFFER, L.NOISE_PHILOX):
        for col in (L.COLLECT_NONE, L.COLLECT_WELFORD_INIT, L.COLLECT_WELFORD):
            assert [ok(L.CSGHMC, noise, col, u) for u in (1, 2, 4, 3)] == [1, 1, 1, 0]
    for col in (L.COLLECT_NONE, L.COLLECT_MEAN_INIT, L.COLLECT_MEAN):
        assert [ok(L.SGLD, L.NOISE_BUFFER, col, u) for u in (1, 2, 4)] == [1, 0, 0]
        want = [1, 1, 1] if col == L.COLLECT_NONE else [1, 0, 0]
        assert [ok(L.SGLD, L.NOISE_PHILOX, col, u) for u in (1, 2, 4)] == want
    assert ok(L.SGHMC, L.NOISE_PHILOX, L.COLLECT_NONE, 1) == 0
    assert ok(L.SGLD, L.NOISE_NONE, L.COLLECT_NONE, 1) == 0
    assert ok(L.CSGHMC, L.NOISE_PHILOX, L.COLLECT_MEAN, 1) == 0


def test_chain_step_refuses_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_chain_step(_good_args(), None) == ARG
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_step:") and b"graph redirect is active" in msg
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_chain_step(None, None) == NULL  # back to ordinary validation


def test_python_wrapper_refuses_before_any_launch():
    from bayesdll_amd import kernels as K
    st = SimpleNamespace(K=3, theta=torch.zeros(12))
    with pytest.raises(ValueError, match=r"float32 \[K, 12\]"):
        K.chain_step(st, 0, scalars=torch.zeros(3, 12))                     # a host table
    with pytest.raises(ValueError, match=r"float32 \[K, 12\]"):
        K.chain_step(st, 0, scalars=torch.zeros(3, 12, dtype=torch.float64))


# ------------------------------------------------------------ the expansion
PER_CHAIN = {
    "csghmc": {"lr": [5e-2, 1e-2, 3e-3, 0.2], "lr_head": [0.1, 0.03, 3e-3, 0.05],
               "prior_sig": [1.0, 0.3, 2.5, 0.0], "momentum_decay": [0.1, 0.18, 0.05, 0.5],
               "nd": [1.0, 0.01, 0.3, 0.0], "Ninflate": [1.0, 1e3, 7.0, 0.5]},
    "sgld": {"lr": [5e-2, 1e-2, 3e-3, 0.2], "lr_head": [0.1, 0.03, 3e-3, 0.05],
             "prior_sig": [1.0, 0.3, 2.5, 0.7], "nd": [1.0, 0.01, 0.3, 0.0],
             "Ninflate": [1.0, 1e3, 7.0, 0.5], "momentum": [0.5, 0.9, 0.1, 0.99]},
}


def _args(**over):
    a = SimpleNamespace(lr=5e-2, lr_head=1e-1, epochs=2, num_cycles=2, momentum=0.5,
                        proportion_exploration=0.5, ND=64, device="cpu", seed=7,
                        hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0,
                                 "nd": 1.0, "thin": 1, "nst": 0, "bias": "informative",
                                 "burnin": 0})
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _f32(x):
    return np.float32(C.c_float(float(x)).value)  # as a C float field receives the double


def _restated(family, v, lr, lr_head, ND):
    """One chain's row from today's update() expressions, in Python floats:
    StackedCSGHMC.update / StackedSGLD.update with this chain's values."""
    N = ND * v["Ninflate"]
    if family == "csghmc":
        lrs = (lr, lr * (v["lr_head"] / v["lr"]))
        ns = [v["nd"] * np.sqrt(2 * v["momentum_decay"] * x) / N for x in lrs]
        row = [lrs[0], lrs[1], ns[0], ns[1], 1 - v["momentum_decay"], v["prior_sig"], 1.0, 1.0, 0.0,
               1.0 / 1.0, 1.0 / 1.0]
    else:
        lrs = (lr, lr_head)
        ns = [v["nd"] * np.sqrt(2 / (N * x)) for x in lrs]
        s2 = v["prior_sig"] ** 2
        row = [lrs[0], lrs[1], ns[0], ns[1], 1.0, v["prior_sig"], s2, N, v["momentum"],
               1.0 / s2, 1.0 / N]
    return np.asarray([_f32(x) for x in row] + [np.float32(0)])


@pytest.mark.parametrize("family", ["csghmc", "sgld"])
def test_expansion_matches_the_float64_restatement(family):
    """Every chain's row, value for value (fp32 bit patterns), for the swept
    values above and for a cyclical two-cycle schedule's lrs; a partial table
    takes the shared values for the names it leaves out."""
    from bayesdll_amd import per_chain as PC
    from bayesdll_amd.cyclical import CyclicalSGMCMC
    args = _args()
    tab = PC.parse(PER_CHAIN[family], 4, family, PC.defaults(args, family))
    bpe = 5
    scheds = PC.schedules(tab, args.epochs, args.num_cycles, args.proportion_exploration)
    for epoch in range(args.epochs):
        lrs = np.stack([PC.cyclical_lrs(scheds, epoch, b, bpe) for b in range(bpe)])
        rows = PC.csghmc_rows(tab, lrs, args.ND) if family == "csghmc" else \
            PC.sgld_rows(tab, lrs, PC.head_lrs(tab, lrs), args.ND)
        assert rows.shape == (bpe, 4, 12) and rows.dtype == np.float32
        for b in range(bpe):
            for k in range(4):
                v = {nm: PER_CHAIN[family][nm][k] for nm in PER_CHAIN[family]}
                own = CyclicalSGMCMC(base_lr=v["lr"], nbr_of_cycles=args.num_cycles,
                                     epochs=args.epochs, proportion_exploration=0.5)
                lr = own.calculate_lr(epoch=epoch, batch=b, batches_per_epoch=bpe)
                want = _restated(family, v, lr, lr * (v["lr_head"] / v["lr"]), args.ND)
                assert rows[b, k].view(np.int32).tolist() == want.view(np.int32).tolist(), \
                    (family, epoch, b, k, rows[b, k], want)
    # a partial table
    part = PC.parse({"prior_sig": [0.1, 0.2, 0.3, 0.4]}, 4, family, PC.defaults(args, family))
    assert part["lr"].tolist() == [args.lr] * 4 and part["prior_sig"].tolist() == [0.1, 0.2, 0.3, 0.4]
    assert set(part) == set(PC.NAMES[family])


def _patched(monkeypatch, calls):
    from bayesdll_amd import kernels as K
    monkeypatch.setattr(K, "chain_step", lambda st, m, **kw: calls.append((st, m, kw)))


@pytest.mark.parametrize("cls_name,family", [("StackedCSGHMC", "csghmc"), ("StackedSGLD", "sgld"),
                                             ("StackedCSGLD", "sgld")])
def test_uniform_rows_equal_the_uniform_launch_scalars(host_only, monkeypatch, cls_name, family):  # noqa: F811
    """K equal per_chain values: every row the sampler hands the per-chain
    launch equals the scalars bdl_step_args carries in the uniform sampler's
    launch of the same step (and the keys, flags and collect agree)."""
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    from bayesdll_amd import stacked
    chain_calls = []
    _patched(monkeypatch, chain_calls)
    cls = getattr(stacked, cls_name)
    args = _args(lr=3e-2, lr_head=7e-2, momentum=0.9)
    args.hparams.update(prior_sig=0.7, Ninflate=3.0, nd=0.4, momentum_decay=0.18)
    same = {nm: [v] * 3 for nm, v in (("lr", 3e-2), ("prior_sig", 0.7), ("nd", 0.4))}
    torch.manual_seed(0)
    U = cls(Net(), 3, args, chain0=4)
    P = cls(Net(), 3, args, chain0=4, per_chain=same)
    assert P.state.chain_tables and P.per_chain is not None and P.swept == ("lr", "prior_sig", "nd")
    x, y = torch.randn(8, 13), torch.randint(0, 5, (8,))
    steps = [(0.011, False), (0.004, True)]
    for lr, ss in steps:
        for S in (U, P):
            grads, _, _ = S.gradients(x, y)
            if family == "csghmc":
                S.update(grads, lr, should_sample=ss)
            else:
                S.update(grads, (lr, lr * (args.lr_head / args.lr)))
    assert len(host_only) == len(chain_calls) == 2
    for (ust, um, ukw), (pst, pm, pkw) in zip(host_only, chain_calls):
        a = K._step_args(ust, um, **ukw)
        want = [a.lr[0], a.lr[1], a.noise_scale[0], a.noise_scale[1], a.one_minus_alpha,
                a.prior_sig, a.sigma2, a.n_data, a.mu, a.inv_sigma2, a.inv_n_data, 0.0]
        rows = pkw["scalars"].numpy()
        assert rows.shape == (3, 12)
        for k in range(3):
            assert rows[k].view(np.int32).tolist() == \
                np.asarray(want, dtype=np.float32).view(np.int32).tolist(), (cls_name, k)
        assert pm == um and pkw["noise_mode"] == ukw["noise_mode"]
        assert (pkw["seed"], pkw["chain"], pkw["step"]) == (ukw["seed"], ukw["chain"], ukw["step"])
        assert pkw.get("momentum", False) == ukw.get("momentum", False)
        assert pkw.get("first_step", False) == ukw.get("first_step", False)
    # the per-chain table: one chain's runs, chain-local, and [K, nruns] bases
    st = P.state
    assert st.chain_runs[:, 0].tolist() == [91, 98, 133, 138] and st.chain_nruns == 4
    assert tuple(st.chain_gbase.shape) == (3, 4) and st.nonfinite.numel() == 3
    grads, _, _ = P.gradients(x, y)
    P.state.use_grads(grads)
    bases = P.state.chain_gbase.numpy()
    for k in range(3):
        for i, nm in enumerate(st.names):
            assert bases[k, i] == grads[nm].data_ptr() + 4 * k * st.numels[i] - 4 * st.offsets[i]
    for i in range(4):
        assert bool(st.chain_runs[i, 1] & L.ATTR_GUNALIGNED) == bool((bases[:, i] % 16).any())


def test_epoch_rows_are_one_block_per_batch(host_only, monkeypatch):  # noqa: F811
    """train_one_epoch forms the epoch's rows once ([batches, K, 12]) and hands
    row b to step b: the block step b receives is chain k's own schedule at b."""
    from bayesdll_amd import per_chain as PC
    from bayesdll_amd import stacked
    calls = []
    _patched(monkeypatch, calls)
    args = _args()
    S = stacked.StackedCSGHMC(Net(), 4, args, per_chain=PER_CHAIN["csghmc"])
    loader = [(torch.randn(8, 13), torch.randint(0, 5, (8,))) for _ in range(3)]
    uploads = []
    orig = S._upload_rows
    monkeypatch.setattr(S, "_upload_rows", lambda r: uploads.append(r.shape) or orig(r))
    S.train_one_epoch(loader, 1)
    assert uploads == [(3, 4, 12)] and len(calls) == 3           # one upload, three launches
    want = S.epoch_rows(1, 3)
    for b, (_, _, kw) in enumerate(calls):
        assert np.array_equal(kw["scalars"].numpy().view(np.int32), want[b].view(np.int32))
    assert (want[0, :, 0] != want[1, :, 0]).all()                   # the lr moves with the schedule
    lr1 = PC.cyclical_lrs(S.scheds, 1, 1, 3)
    assert want[1, :, 0].tolist() == [float(np.float32(v)) for v in lr1]


# ---------------------------------------------------------------- refusals
def test_per_chain_tables_that_are_refused():
    from bayesdll_amd import per_chain as PC
    args = _args()
    for fam in ("csghmc", "sgld"):
        d = PC.defaults(args, fam)
        with pytest.raises(ValueError, match="unknown name 'burnin'"):
            PC.parse({"burnin": [1, 2, 3]}, 3, fam, d)
        with pytest.raises(ValueError, match="wrong length"):
            PC.parse({"lr": [1e-2, 2e-2]}, 3, fam, d)
        with pytest.raises(ValueError, match="non-finite"):
            PC.parse({"lr": [1e-2, float("nan"), 1e-2]}, 3, fam, d)
    with pytest.raises(ValueError, match="unknown name 'momentum'"):
        PC.parse({"momentum": [0.5] * 3}, 3, "csghmc", PC.defaults(args, "csghmc"))
    with pytest.raises(ValueError, match="unknown name 'momentum_decay'"):
        PC.parse({"momentum_decay": [0.5] * 3}, 3, "sgld", PC.defaults(args, "sgld"))
    with pytest.raises(ValueError, match="mixes zero and non-zero"):
        PC.parse({"momentum": [0.5, 0.0, 0.9]}, 3, "sgld", PC.defaults(args, "sgld"))
    PC.parse({"momentum": [0.0] * 3}, 3, "sgld", PC.defaults(args, "sgld"))  # all zero: fine


def test_samplers_that_refuse_per_chain(host_only):  # noqa: F811
    """The refusals come before the sampler touches a device or its network."""
    from bayesdll_amd import stacked
    args = _args()
    args.hparams.update(beta1=0.9, beta2=0.999)
    pc = {"lr": [1e-2, 2e-2]}
    for name in ("StackedSGHMC", "StackedAdamSGHMC", "StackedAdamCSGHMC"):
        with pytest.raises(ValueError, match="per_chain is not supported"):
            getattr(stacked, name)(None, 2, args, per_chain=pc)
    with pytest.raises(ValueError, match="cannot be combined with clip_grad"):
        stacked.StackedCSGLD(None, 2, _args(clip_grad=1.0), per_chain=pc)
    with pytest.raises(ValueError, match="unknown name"):
        stacked.StackedCSGHMC(None, 2, args, per_chain={"thin": [1, 2]})
    with pytest.raises(ValueError, match="wrong length"):
        stacked.StackedSGLD(None, 2, args, per_chain={"lr": [1e-2]})
    with pytest.raises(ValueError, match="mixes zero and non-zero"):
        stacked.StackedSGLD(None, 2, args, per_chain={"momentum": [0.0, 0.5]})
    S = stacked.StackedCSGHMC(Net(), 2, args, per_chain=pc)
    with pytest.raises(ValueError, match="target different ones"):
        S.diagnostics()
    # the table travels with the checkpoint
    assert S.state_dict()["per_chain"]["lr"] == [1e-2, 2e-2]
    assert stacked.StackedCSGHMC(Net(), 2, args).state_dict()["per_chain"] is None


def test_checkpoint_with_another_table_is_refused(host_only, tmp_path):  # noqa: F811
    from bayesdll_amd import stacked
    args = _args()
    A = stacked.StackedCSGHMC(Net(), 2, args, per_chain={"lr": [1e-2, 2e-2]})
    path = A.save_ckpt(str(tmp_path / "a.pt"))
    B = stacked.StackedCSGHMC(Net(), 2, args, per_chain={"lr": [1e-2, 3e-2]})
    with pytest.raises(ValueError, match="per_chain table differs"):
        B.load_ckpt(path)
    with pytest.raises(ValueError, match="per_chain table differs"):
        stacked.StackedCSGHMC(Net(), 2, args).load_ckpt(path)
    stacked.StackedCSGHMC(Net(), 2, args, per_chain={"lr": [1e-2, 2e-2]}).load_ckpt(path)


@pytest.mark.parametrize("argv,word", [
    (["--sweep", "lr=1e-2,2e-2"], "needs --stacked_chains"),
    (["--stacked_chains", "3", "--sweep", "lr=1e-2,2e-2"], "length mismatch"),
    (["--stacked_chains", "2", "--sweep", "thin=1,2"], "does not sweep 'thin'"),
    (["--stacked_chains", "2", "--sweep", "momentum=0.1,0.2"], "does not sweep 'momentum'"),
    (["--stacked_chains", "2", "--method", "sgld", "--sweep", "momentum_decay=0.1,0.2"],
     "does not sweep 'momentum_decay'"),
    (["--stacked_chains", "2", "--method", "sghmc", "--sweep", "lr=1e-2,2e-2"],
     "no per-chain launch"),
    (["--stacked_chains", "2", "--method", "csgld", "--clip_grad", "1.0", "--sweep", "lr=1e-2"],
     "--clip_grad"),
    (["--stacked_chains", "2", "--rhat", "--sweep", "lr=1e-2,2e-2"], "--rhat"),
    (["--stacked_chains", "2", "--sweep", "lr"], "expected NAME="),
    (["--stacked_chains", "2", "--sweep", "lr=a,b"], "must be numbers"),
])
def test_cli_refuses_a_sweep_it_cannot_run(argv, word, capsys):
    from bayesdll_amd.run import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_parses_a_sweep():
    from bayesdll_amd.run import build_parser, parse_sweep
    ap = build_parser()
    args = ap.parse_args(["--stacked_chains", "3", "--sweep", "lr=1e-2,2e-2,3e-2", "--sweep",
                          "prior_sig=0.5"])
    assert parse_sweep(ap, args) == {"lr": [1e-2, 2e-2, 3e-2], "prior_sig": [0.5] * 3}  # broadcast
    assert parse_sweep(ap, ap.parse_args([])) is None
