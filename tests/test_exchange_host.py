"""The replica-exchange unit (include/bdl_exchange.h) without a GPU: the
header's declarations, the export table and the ctypes mirrors against the C
layout; what the geometry table reaches; the NumPy reference's own properties
(the margin condition of EVERY decision the GPU tests compare, the acceptance
frequency, a hand-worked round trip); the refusals of the entry points by
status code (fake pointers: each call returns before any HIP call) and of the
samplers before any device work."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import exchange_ref as R
from philox_ref import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NULL, ALIGN, ARG = -1, -2, -3


# ------------------------------------------------------------------ the ABI
def test_header_declares_the_four_entry_points_and_is_additive():
    text = open(os.path.join(INCLUDE, "bdl_exchange.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fns = re.findall(r"^\s*(?:int|int64_t|void|const char\*)\s+(bdl_\w+)\s*\(", code, flags=re.M)
    assert sorted(fns) == ["bdl_exchange_decide", "bdl_exchange_energy", "bdl_exchange_swap",
                           "bdl_exchange_workspace_bytes"]
    assert '#include "bdl_sgmcmc.h"' in code and "BDL_ABI_VERSION" not in code
    # the header states both orders and that the padding travels
    assert "In-tile order" in text and "Cross-tile order" in text
    assert "the padding travels with its slot" in text
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.EXCHANGE_EXPORTS) == set(fns) and all(hasattr(h, f) for f in fns)
    mk = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "Makefile")).read()
    assert "bdl_exchange" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "bdl_exchange.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]
    src = open(os.path.join(ROOT, "bayesdll_amd", "csrc", "bdl_exchange.hip")).read()
    assert "atomic" not in src.lower() and "hipMalloc" not in src and "Synchronize" not in src
    # the shared helpers, not copies of them
    assert '#include "bdl_chain_common.hpp"' in src and "wave_sum(" in src and "ld4(" in src
    for helper in ("double wave_sum", "f4v ld4", "bool misaligned", "bool overlap", "int launched"):
        assert helper not in src


def test_ctypes_mirrors_match_the_c_header(tmp_path):
    from bayesdll_amd import _lib as L
    structs = {"bdl_exchange_state": L.ExchangeState,
               "bdl_exchange_energy_args": L.ExchangeEnergyArgs,
               "bdl_exchange_decide_args": L.ExchangeDecideArgs,
               "bdl_exchange_swap_args": L.ExchangeSwapArgs}
    lines = []
    for st, cls in structs.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("caps %d %d %d %d %d %d %d %d\\n", BDL_EXCHANGE_MAX_CHAINS, '
                 'BDL_EXCHANGE_MAX_VECTORS, BDL_EXCHANGE_TILE, BDL_EXCHANGE_MAX_GRID, '
                 'BDL_EXCHANGE_FIRST, BDL_EXCHANGE_ENERGY_ONLY, BDL_EXCHANGE_UP, '
                 'BDL_EXCHANGE_DOWN);')
    lines.append('printf("base %llu\\n", (unsigned long long)BDL_EXCHANGE_STEP_BASE);')
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"bdl_exchange.h\"\n"
           "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(c), "-o",
                           str(exe)])
    out = subprocess.check_output([str(exe)]).decode().strip().splitlines()
    caps = [int(v) for v in next(ln for ln in out if ln.startswith("caps ")).split()[1:]]
    base = int(next(ln for ln in out if ln.startswith("base ")).split()[1])
    lay = {k: int(v) for k, v in (ln.rsplit(" ", 1) for ln in out
                                  if not ln.startswith(("caps ", "base ")))}
    for st, cls in structs.items():
        assert lay[st] == C.sizeof(cls), st
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[f"{st}.{f}"], (st, f)
    assert caps == [L.EXCHANGE_MAX_CHAINS, L.EXCHANGE_MAX_VECTORS, L.EXCHANGE_TILE,
                    L.EXCHANGE_MAX_GRID, L.EXCHANGE_FIRST, L.EXCHANGE_ENERGY_ONLY, L.EXCHANGE_UP,
                    L.EXCHANGE_DOWN]
    assert (caps[0], caps[2], caps[6], caps[7]) == (R.MAX_CHAINS, R.TILE, R.UP, R.DOWN)
    # a step domain of its own: above every training step and evaluation draw
    from bayesdll_amd._runner import EVAL_STEP_BASE
    assert base == L.EXCHANGE_STEP_BASE == R.STEP_BASE == 1 << 63
    assert EVAL_STEP_BASE + (1 << 62) <= base and base + (1 << 62) <= 1 << 64


def test_workspace_bytes():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert h.bdl_exchange_workspace_bytes(8, 1024) == 8 * 8
    assert h.bdl_exchange_workspace_bytes(8, 1025) == 8 * 8 * 2
    assert h.bdl_exchange_workspace_bytes(5, 3) == 5 * 8
    for K_, n in ((0, 5), (65, 5), (3, 0), (3, -1)):
        assert h.bdl_exchange_workspace_bytes(K_, n) == 0


def _energy(**f):
    from bayesdll_amd import _lib as L
    a = L.ExchangeEnergyArgs()
    a.theta, a.prior, a.workspace = 0x10000, 0x20000, 0x30000
    a.n, a.chain_groups, a.chains = 1025, 257, 5
    for k, v in f.items():
        setattr(a, k, v)
    return a


def _decide(**f):
    from bayesdll_amd import _lib as L
    a = L.ExchangeDecideArgs()
    a.state, a.workspace, a.loss, a.beta = 0x10000, 0x30000, 0x40000, 0x50000
    a.n, a.n_data, a.sigma2, a.var, a.chains = 1025, 100.0, 1.0, 0.0, 5
    for k, v in f.items():
        setattr(a, k, v)
    return a


def _swap(**f):
    from bayesdll_amd import _lib as L
    a = L.ExchangeSwapArgs()
    a.state, a.chain_groups, a.nvectors, a.chains = 0x10000, 257, 2, 5
    a.vectors[0], a.vectors[1] = 0x100000, 0x200000
    for k, v in f.items():
        if k.startswith("v"):
            a.vectors[int(k[1:])] = v
        else:
            setattr(a, k, v)
    return a


def test_entry_points_refuse_by_status_code_before_any_hip_call():
    from bayesdll_amd import _lib as L
    h = L.lib()
    cases = [
        (h.bdl_exchange_energy, _energy(theta=None), NULL, "null theta"),
        (h.bdl_exchange_energy, _energy(workspace=None), NULL, "null workspace"),
        (h.bdl_exchange_energy, _energy(chains=0), ARG, "chains in"),
        (h.bdl_exchange_energy, _energy(chains=65), ARG, "chains in"),
        (h.bdl_exchange_energy, _energy(n=0), ARG, ">= 1"),
        (h.bdl_exchange_energy, _energy(n=1029), ARG, "exceeds the chain slot"),
        (h.bdl_exchange_energy, _energy(grid_blocks=65536), ARG, "grid_blocks"),
        (h.bdl_exchange_energy, _energy(theta=0x10004), ALIGN, "theta not 16-B"),
        (h.bdl_exchange_energy, _energy(prior=0x20008), ALIGN, "prior not 16-B"),
        (h.bdl_exchange_energy, _energy(workspace=0x30004), ALIGN, "workspace not 8-B"),
        (h.bdl_exchange_decide, _decide(state=None), NULL, "null state"),
        (h.bdl_exchange_decide, _decide(loss=None), NULL, "null loss"),
        (h.bdl_exchange_decide, _decide(beta=None), NULL, "null beta"),
        (h.bdl_exchange_decide, _decide(flags=8), ARG, "unknown flag"),
        (h.bdl_exchange_decide, _decide(sigma2=0.0), ARG, "sigma2"),
        (h.bdl_exchange_decide, _decide(sigma2=float("nan")), ARG, "sigma2"),
        (h.bdl_exchange_decide, _decide(var=-1.0), ARG, "var"),
        (h.bdl_exchange_decide, _decide(attempt=1 << 62), ARG, "attempt"),
        (h.bdl_exchange_decide, _decide(beta=0x50004), ALIGN, "beta not 8-B"),
        (h.bdl_exchange_decide, _decide(loss=0x40002), ALIGN, "loss not 4-B"),
        (h.bdl_exchange_decide, _decide(workspace=0x10008), ARG, "overlaps"),
        (h.bdl_exchange_swap, _swap(state=None), NULL, "null state"),
        (h.bdl_exchange_swap, _swap(v1=None), NULL, "null vector"),
        (h.bdl_exchange_swap, _swap(nvectors=0), ARG, "nvectors"),
        (h.bdl_exchange_swap, _swap(nvectors=5), ARG, "nvectors"),
        (h.bdl_exchange_swap, _swap(chain_groups=0), ARG, "chain_groups"),
        (h.bdl_exchange_swap, _swap(v1=0x200004), ALIGN, "not 16-B"),
        (h.bdl_exchange_swap, _swap(v1=0x100000 + 16 * 257 * 5 - 16), ARG, "two vectors overlap"),
        (h.bdl_exchange_swap, _swap(v0=0x10000 - 16), ARG, "overlaps the state"),
    ]
    for fn, a, status, word in cases:
        assert fn(a, None) == status, word
        assert word in h.bdl_last_error().decode(), (word, h.bdl_last_error())


# ------------------------------------------------------------- the geometry
def test_geometry_table_reaches_every_path():
    G = R.GEOMETRY
    tiles = lambda n: (n + R.TILE - 1) // R.TILE  # noqa: E731
    assert any(K_ * tiles(n) > 2 for _, K_, n, _ in G)            # a second trip at grid 2
    assert any(n == 3 for _, _, n, _ in G)                        # shorter than one float4
    assert {n % 4 for _, _, n, _ in G} == {0, 1, 2, 3}
    assert any(s > n for _, _, n, s in G) and any(s == n for _, _, n, s in G)
    assert any(s - n > 4 for _, _, n, s in G)
    assert any(n == R.TILE for _, _, n, _ in G) and any(tiles(n) > 1 for _, _, n, _ in G)
    assert any(tiles(n) > R.BLOCK for _, _, n, _ in G)            # a second cross-tile row
    assert {1, 2, 5} <= {K_ for _, K_, _, _ in G}
    for _, K_, n, s in G:
        assert s % 4 == 0 and 0 < n <= s and 1 <= K_ <= R.MAX_CHAINS


def test_reference_energy_is_the_plain_sum_to_rounding_and_ignores_padding():
    for name, K_, n, s in R.GEOMETRY:
        th, pr = R.make_vectors(name, K_, n, s)
        q = R.energy(th, pr, n)
        with np.errstate(all="ignore"):
            d = (th[:, :n] - pr[:, :n]).astype(np.float64)
            want = np.array([np.sum(r * r) for r in d])
        ok = np.isfinite(want)
        assert np.array_equal(np.isnan(q), np.isnan(want)), name
        # pairwise-like sums of n non-negative terms: n * 2^-52 relative is generous
        assert np.all(np.abs(q[ok] - want[ok]) <= n * 2.0 ** -52 * want[ok]), name
        th2, pr2 = th.copy(), pr.copy()
        th2[:, n:], pr2[:, n:] = 7.0, np.nan                      # other padding: the same bits
        assert R.same_bits(R.energy(th2, pr2, n), q), name
        assert R.same_bits(R.energy(th, None, n), R.energy(th, np.zeros_like(th), n)), name
    th, pr = R.make_vectors(*R.GEOMETRY[2])
    q = R.energy(th, pr, 1025)
    assert q[0] >= 2.0 ** 120 and np.isnan(q[2]) and 0 < q[1] < 1e-70  # 2^60, NaN, subnormals


# ------------------------------------------------------------ the decisions
def _run_reference(var, beta=R.DECIDE_BETA, inputs=R.decide_inputs):
    st, seen = R.new_state(R.DECIDE_K), []
    for t in range(R.DECIDE_ATTEMPTS):
        q, loss = inputs(t)
        seen += R.decide(st, q, loss, beta, n_data=R.DECIDE_N, sigma2=R.DECIDE_SIGMA2, var=var,
                         seed=R.DECIDE_SEED, chain0=R.DECIDE_CHAIN0, attempt=t)
    return st, seen


def test_every_decision_of_the_gpu_tests_has_the_margin():
    """A condition on the INPUTS: |log u - la| > 1e-6 * max(1, |la|) for every
    decision the GPU tests compare, none left out — both values of var, and the
    equal-temperature run (la = 0: log u must not be within 1e-6 of 0)."""
    for var in R.DECIDE_VARS:
        st, seen = _run_reference(var)
        assert len(seen) == 32 * 2 + 32 * 2 and st["refused"] == 0  # 2 pairs at either parity
        assert all(R.margin_ok(lu, la) for _, lu, la in seen)
        acc = int(st["accepts"].sum())
        assert 0 < acc < len(seen)                                  # both outcomes occur
    st, seen = _run_reference(0.0, beta=np.full(R.DECIDE_K, 0.5))
    assert all(la == 0.0 and R.margin_ok(lu, la) for _, lu, la in seen)
    assert np.array_equal(st["accepts"], st["attempts"]) and st["attempts"].sum() == 128
    # the attempts with a NaN / inf energy: their remaining finite decisions
    for t in R.NAN_ATTEMPTS:
        q, loss = R.nan_inputs(t)
        st = R.new_state(R.DECIDE_K)
        seen = R.decide(st, q, loss, R.DECIDE_BETA, n_data=R.DECIDE_N, sigma2=R.DECIDE_SIGMA2,
                        var=0.0, seed=R.DECIDE_SEED, chain0=R.DECIDE_CHAIN0, attempt=t)
        assert st["refused"] == (1 if t % 2 == 0 else 2) and len(seen) == (1 if t % 2 == 0 else 0)
        assert all(R.margin_ok(lu, la) for _, lu, la in seen)


def test_acceptance_frequency_matches_the_metropolis_rule():
    n = 20000
    t = np.arange(n, dtype=np.uint64) + np.uint64(R.STEP_BASE)
    w = philox4x32_10(0, 3, t & np.uint64(0xFFFFFFFF), t >> np.uint64(32), 99, 0)[0]
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    assert u.min() > 0 and u.max() < 1
    assert u[5] == R.uniform(0, 99, 3, 5)                           # the scalar form's stream
    for la in (-2.0, -0.3, 0.5):
        p = min(1.0, np.exp(la))
        share = np.mean(np.log(u) < la)
        assert abs(share - p) <= 4 * np.sqrt(p * (1 - p) / n), (la, share, p)


def _forced(st, accept, t, K_=3):
    """One attempt with energies that force every decided pair's outcome:
    beta descends (db > 0), so U_i - U_{i+1} = +-1e9 decides."""
    q = np.cumsum(np.full(K_, -1e9 if accept else 1e9))
    return R.decide(st, q, np.zeros(K_, np.float32), np.array([1.0, 0.5, 0.25]), n_data=1.0,
                    sigma2=0.5, var=0.0, seed=1, chain0=0, attempt=t)


def test_bookkeeping_counts_a_hand_worked_round_trip():
    st = R.new_state(3)
    assert list(st["direction"]) == [R.UP, 0, R.DOWN]
    _forced(st, False, 0)                       # (0,1) rejected: nothing moves
    assert list(st["replica"]) == [0, 1, 2] and list(st["partner"]) == [0, 1, 2]
    _forced(st, True, 1)                        # (1,2): replica 2 down to slot 1
    assert list(st["replica"]) == [0, 2, 1] and list(st["partner"]) == [0, 2, 1]
    assert list(st["direction"]) == [R.UP, R.DOWN, R.DOWN] and st["round_trips"].sum() == 0
    _forced(st, True, 2)                        # (0,1): replica 2 reaches slot 0: one trip
    assert list(st["replica"]) == [2, 0, 1] and list(st["round_trips"]) == [0, 0, 1]
    assert list(st["direction"]) == [R.UP, R.DOWN, R.UP]
    _forced(st, True, 3)                        # (1,2): replica 0 reaches the hot end
    assert list(st["replica"]) == [2, 1, 0] and list(st["direction"]) == [R.DOWN, R.DOWN, R.UP]
    _forced(st, True, 4)                        # (0,1): replica 1, DOWN since attempt 1: a trip
    assert list(st["replica"]) == [1, 2, 0] and list(st["round_trips"]) == [0, 1, 1]
    _forced(st, True, 5)                        # (1,2): slot 0 keeps replica 1: no new trip
    assert list(st["replica"]) == [1, 0, 2] and list(st["round_trips"]) == [0, 1, 1]
    assert list(st["direction"]) == [R.DOWN, R.UP, R.DOWN]
    assert list(st["attempts"]) == [3, 3] and list(st["accepts"]) == [2, 3] and st["refused"] == 0
    # a NaN energy: counted, nothing moves
    before = st["replica"].copy()
    R.decide(st, np.array([np.nan, 1.0, 2.0]), np.zeros(3, np.float32), np.ones(3), n_data=1.0,
             sigma2=0.5, var=0.0, seed=1, chain0=0, attempt=6)
    assert st["refused"] == 1 and np.array_equal(st["replica"], before)
    assert list(st["attempts"]) == [4, 3] and list(st["accepts"]) == [2, 3]


def test_reference_swap_moves_whole_slots():
    a = np.arange(20, dtype=np.float32).reshape(5, 4)
    (b,) = R.swap([a], [1, 0, 2, 4, 3])
    assert np.array_equal(b, a[[1, 0, 2, 4, 3]]) and np.array_equal(a[0], [0, 1, 2, 3])


# ------------------------------------------------- the samplers' refusals
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.head = torch.nn.Linear(3, 2)

    def forward(self, x):
        return self.head(x)


def _args(momentum=0.0, bias="informative"):
    return SimpleNamespace(lr=1e-2, lr_head=1e-2, epochs=2, num_cycles=2,
                           proportion_exploration=0.5, ND=64, device="cpu", seed=1,
                           momentum=momentum,
                           hparams={"prior_sig": 1.0, "momentum_decay": 0.1, "Ninflate": 1.0,
                                    "nd": 1.0, "thin": 1, "nst": 0, "bias": bias,
                                    "burnin": 0})


REFUSALS = [
    ("StackedSGLD", {}, {}, "needs a per_chain table"),
    ("StackedSGLD", {"per_chain": {"nd": [1, 2, 3]}}, {"momentum": 0.5}, "needs momentum == 0"),
    ("StackedSGLD", {"per_chain": {"nd": [1, 2, 3], "prior_sig": [1, 1, 2]}}, {},
     "prior_sig differs between chains"),
    ("StackedCSGLD", {"per_chain": {"nd": [1, 2, 3], "Ninflate": [1, 2, 1]}}, {},
     "Ninflate differs between chains"),
    ("StackedSGLD", {"per_chain": {"nd": [1, 3, 2]}}, {}, "strictly monotone"),
    ("StackedSGLD", {"per_chain": {"nd": [1, 1, 2]}}, {}, "strictly monotone"),
    ("StackedSGLD", {"per_chain": {"nd": [0, 1, 2]}}, {}, "must be > 0"),
    ("StackedSGLD", {"per_chain": {"nd": [1, 2, 3]}, "per_chain_batches": True}, {},
     "one batch per chain"),
    ("StackedCSGHMC", {"per_chain": {"nd": [1, 2, 3]}}, {}, "none is derived for this sampler"),
    ("StackedSGHMC", {}, {}, "none is derived for this sampler"),
    ("StackedAdamSGHMC", {}, {}, "none is derived for this sampler"),
    ("StackedAdamCSGHMC", {}, {}, "none is derived for this sampler"),
    ("StackedSGLD", {"per_chain": {"nd": [1, 2, 3]}, "exchange_var": -1.0}, {}, "exchange_var"),
    ("StackedSGLD", {"per_chain": {"nd": [1, 2, 3]}}, {"bias": "uninformative"},
     "the update puts no prior on the bias"),
    ("StackedCSGLD", {"per_chain": {"nd": [1, 2, 3]}}, {"bias": "uninformative"},
     "the update puts no prior on the bias"),
]


def frozen_net(net):
    """`net` with its first parameter frozen."""
    next(net.parameters()).requires_grad_(False)
    return net


class _DropNet(_Net):
    def __init__(self):
        super().__init__()
        self.drop = torch.nn.Dropout(0.1)

    def forward(self, x):
        return self.head(self.drop(x))


def test_exchange_every_is_refused_for_frozen_tensors_and_dropout():
    """A frozen tensor is not sampled but would enter the energy and travel;
    a dropout layer would make the energy a randomly masked loss."""
    from bayesdll_amd import stacked
    kw = dict(exchange_every=2, graph=False, per_chain={"nd": [1, 2, 3]})
    with pytest.raises(ValueError, match=r"frozen tensors \(head.weight\)"):
        stacked.StackedSGLD(frozen_net(_Net()), 3, _args(), **kw)
    with pytest.raises(ValueError, match=r"dropout layers \(drop\)"):
        stacked.StackedSGLD(_DropNet(), 3, _args(), **kw)


@pytest.mark.parametrize("cls,kw,akw,why", REFUSALS)
def test_exchange_every_is_refused_with_its_reason(cls, kw, akw, why):
    """Each refusal names its reason and comes before any device work (the
    network is on the CPU here)."""
    from bayesdll_amd import stacked
    with pytest.raises(ValueError, match=why):
        getattr(stacked, cls)(_Net(), 3, _args(**akw), exchange_every=2, graph=False, **kw)


def test_exchange_every_is_refused_across_processes(monkeypatch):
    from bayesdll_amd import chains, stacked
    monkeypatch.setattr(chains, "world", lambda: 2)
    with pytest.raises(ValueError, match="2 processes"):
        stacked.StackedSGLD(_Net(), 3, _args(), exchange_every=1, graph=False, chain0=0,
                            per_chain={"nd": [1, 2, 3]})
    with pytest.raises(ValueError, match="integer >= 0"):
        stacked.StackedSGLD(_Net(), 3, _args(), exchange_every=-1, graph=False, chain0=0)


def test_cold_weights_refusals_and_table():
    from bayesdll_amd import stacked
    S = SimpleNamespace(per_chain={"nd": np.array([2.0, 0.5, 1.0])}, K=3,
                        args=SimpleNamespace(device="cpu"), _component_keys=lambda: [0, 1])
    S.cold_slots = lambda: stacked._StackedSampler.cold_slots(S)


    def cw(S_, what, combine, by_chain):  # the one helper both weight kinds go through
        return stacked._StackedSampler._stacking_weights(S_, what, combine, by_chain, cold=True)
    w = cw(S, "evaluate", "arithmetic", False)
    assert w.dtype == torch.float64 and w.shape == (6, 1)
    assert w.reshape(2, 3).tolist() == [[0, 0.5, 0], [0, 0.5, 0]] and S.cold_slots() == [1]
    with pytest.raises(ValueError, match="pooled form only"):
        cw(S, "evaluate_chains", "arithmetic", True)
    with pytest.raises(ValueError, match='combine="reference"'):
        cw(S, "evaluate", "reference", False)
    S.per_chain = None
    with pytest.raises(ValueError, match="needs a per_chain table"):
        cw(S, "evaluate", "arithmetic", False)
