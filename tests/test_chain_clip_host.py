"""The per-chain clip (include/bdl_clip.h) without a GPU: the C struct layouts
against the ctypes mirrors, the exports, every validation path of
bdl_chain_clip (fake pointers: each call returns before any HIP call), and the
NumPy restatement (tests/chain_clip_ref.py) against
torch.nn.utils.clip_grad_norm_ run per chain in float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import chain_clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

SEGMENT_FIELDS = ["base", "numel", "chain_stride"]
ARGS_FIELDS = ["segments", "nsegments", "chains", "max_norm", "blocks_per_chain", "workspace"]
NULL, ALIGN, ARG = -1, -2, -3


def _c_layout(tmp_path):
    lines = ['printf("bdl_clip_segment %zu\\nbdl_chain_clip_args %zu\\n", '
             'sizeof(bdl_clip_segment), sizeof(bdl_chain_clip_args));',
             'printf("caps %d %d %d\\n", BDL_CLIP_MAX_SEGMENTS, BDL_CLIP_MAX_CHAINS, '
             'BDL_CLIP_MAX_BLOCKS_PER_CHAIN);']
    for st, fields in (("bdl_clip_segment", SEGMENT_FIELDS), ("bdl_chain_clip_args", ARGS_FIELDS)):
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_clip.h\"\n"
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
    assert lay["bdl_clip_segment"] == C.sizeof(L.ClipSegment) == 24  # a row of three int64
    assert lay["bdl_chain_clip_args"] == C.sizeof(L.ClipArgs)
    assert [f for f, _ in L.ClipSegment._fields_] == SEGMENT_FIELDS
    assert [f for f, _ in L.ClipArgs._fields_] == ARGS_FIELDS
    for cls, name in ((L.ClipSegment, "bdl_clip_segment"), (L.ClipArgs, "bdl_chain_clip_args")):
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[f"{name}.{f}"], (name, f)
    assert caps == [L.CLIP_MAX_SEGMENTS, L.CLIP_MAX_CHAINS, L.CLIP_MAX_BLOCKS_PER_CHAIN]


def test_library_exports_the_clip_next_to_the_pinned_abi():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.CLIP_EXPORTS) == {"bdl_chain_clip", "bdl_chain_clip_workspace_bytes"}
    assert not set(L.CLIP_EXPORTS) & set(L.EXPORTS)
    assert not set(L.CLIP_EXPORTS) & set(L.DIAG_EXPORTS)
    for name in L.CLIP_EXPORTS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    for k in (1, 3, 8, 64):
        nb = h.bdl_chain_clip_workspace_bytes(k)
        # the (norm, coef) table, then one fp64 partial per workgroup of the largest grid
        assert nb % 16 == 0 and nb >= 8 * k + 8 * k * L.CLIP_MAX_BLOCKS_PER_CHAIN
    assert h.bdl_chain_clip_workspace_bytes(0) == 0
    assert h.bdl_chain_clip_workspace_bytes(L.CLIP_MAX_CHAINS + 1) == 0


def _good_args():
    from bayesdll_amd import _lib as L
    a = L.ClipArgs()
    a.segments, a.workspace = 0x10008, 0x30000
    a.nsegments, a.chains, a.max_norm, a.blocks_per_chain = 19, 3, 1.0, 0
    return a


def test_chain_clip_validates_before_touching_the_device():
    """Every refusal of the header's table, with its status and a prefixed
    message.  No call here passes validation, so none reaches a HIP call."""
    from bayesdll_amd import _lib as L
    h = L.lib()

    def refused(status, word, **fields):
        a = _good_args()
        for k, v in fields.items():
            setattr(a, k, v)
        assert h.bdl_chain_clip(a, None) == status, fields
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_clip:") and word in msg, (fields, msg)

    assert h.bdl_chain_clip(None, None) == NULL and b"null args" in h.bdl_last_error()
    assert h.bdl_last_error().startswith(b"bdl_chain_clip:")
    refused(NULL, b"segments", segments=None)
    refused(NULL, b"workspace", workspace=None)
    refused(ALIGN, b"workspace not 16-B aligned", workspace=0x30008)
    refused(ALIGN, b"workspace not 16-B aligned", workspace=0x30004)
    refused(ALIGN, b"segments not 8-B aligned", segments=0x10004)
    refused(ARG, b"chains", chains=0)
    refused(ARG, b"chains", chains=-3)
    refused(ARG, b"chains", chains=L.CLIP_MAX_CHAINS + 1)
    refused(ARG, b"nsegments", nsegments=0)
    refused(ARG, b"nsegments", nsegments=-1)
    refused(ARG, b"nsegments", nsegments=L.CLIP_MAX_SEGMENTS + 1)
    refused(ARG, b"max_norm", max_norm=0.0)
    refused(ARG, b"max_norm", max_norm=-1.0)
    refused(ARG, b"max_norm", max_norm=float("nan"))
    refused(ARG, b"blocks_per_chain", blocks_per_chain=-1)
    refused(ARG, b"blocks_per_chain", blocks_per_chain=L.CLIP_MAX_BLOCKS_PER_CHAIN + 1)


def test_chain_clip_refuses_while_a_graph_redirect_is_active():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_graph_redirect(C.c_void_p(0x10), C.c_void_p(0x20)) == 0
    try:
        assert h.bdl_chain_clip(_good_args(), None) == ARG
        msg = h.bdl_last_error()
        assert msg.startswith(b"bdl_chain_clip:") and b"graph redirect is active" in msg
        assert h.bdl_chain_clip(None, None) == ARG
    finally:
        h.bdl_graph_redirect(None, None)
    assert h.bdl_chain_clip(None, None) == NULL  # back to ordinary validation


def test_python_wrapper_refuses_before_any_launch():
    from bayesdll_amd import kernels as K
    seg = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="int64 device tensor"):
        K.chain_clip(seg, 2, 3, 1.0)                       # a host table: no CPU path
    with pytest.raises(ValueError, match="int64 device tensor"):
        K.chain_clip(torch.zeros(6), 2, 3, 1.0)
    assert K.clip_bytes_per_elem(0.0) == 4 and K.clip_bytes_per_elem(1.0) == 12


@pytest.mark.parametrize("K_", [1, 3, 5])
def test_reference_against_clip_grad_norm_in_float64(K_):
    """The restatement's fp32 chain of roundings against clip_grad_norm_ run
    per chain on float64 copies.  Bounds: the norm is one rounding of the
    float64 value (within one fp32 ulp); the coefficient carries that rounding
    and three of its own (the sum, the reciprocal, the product): 4 * 2^-24
    relative; a scaled element one more: 5 * 2^-24.  Chain k's gradient is
    scaled to 0.25, 1.001, 4, 0.9, 1.5 x max_norm: clipped and unclipped
    chains both present (K = 1: the clipped 4 x)."""
    rng = np.random.default_rng(50 + K_)
    numels = [13312, 1024, 3, 5, 4, 8, 12, 10, 1000]
    max_norm = 0.75  # exact in fp32: no rounding of the threshold itself
    targets = [4.0] if K_ == 1 else [0.25, 1.001, 4.0, 0.9, 1.5][:K_]
    chains = []
    for t in targets:
        sl = [rng.standard_normal(n).astype(np.float32) for n in numels]
        nrm = np.sqrt(sum(float(np.dot(g.astype(np.float64), g.astype(np.float64))) for g in sl))
        chains.append([(g * np.float32(t * max_norm / nrm)).astype(np.float32) for g in sl])
    norms, coefs, scaled = R.chain_clip(chains, max_norm)
    assert [bool(c < 1) for c in coefs] == [t > 1 for t in targets]
    if K_ > 1:
        assert any(c < 1 for c in coefs) and any(c == 1 for c in coefs)
    for k, sl in enumerate(chains):
        ps = [torch.nn.Parameter(torch.zeros(g.size, dtype=torch.float64)) for g in sl]
        for p, g in zip(ps, sl):
            p.grad = torch.from_numpy(g.astype(np.float64))
        total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        assert abs(float(norms[k]) - total) <= float(np.spacing(norms[k])), k
        coef64 = min(max_norm / (total + 1e-6), 1.0)
        assert abs(float(coefs[k]) - coef64) <= 4 * 2.0 ** -24 * coef64, k
        for p, g, s in zip(ps, sl, scaled[k]):
            want = p.grad.numpy()
            if coefs[k] < 1:
                assert np.all(np.abs(s.astype(np.float64) - want) <= 5 * 2.0 ** -24 * np.abs(want))
            else:  # unclipped: torch multiplies by 1.0, the restatement does not touch it
                assert np.array_equal(s, g) and np.array_equal(want, g.astype(np.float64))
