"""The replica-exchange unit on the device against tests/exchange_ref.py: the
energy bit for bit at two grids on every shape of the geometry table, 64
consecutive decisions of K = 5 field by field (their margin condition is
asserted on the CPU in tests/test_exchange_host.py), the swap bit for bit on
guarded buffers, and the samplers: a permutation and the attempt counts after
40 steps, bit-identity with the option off when nothing is accepted, an exact
continuation from a checkpoint, weights="cold", the refusals."""
import numpy as np
import pytest
import torch

import exchange_ref as R
from test_exchange_host import REFUSALS
from test_gpu_chain_diag import Net, _args

pytestmark = pytest.mark.gpu
GUARD = 64  # sentinel elements before and after a guarded buffer (256 B: alignment is kept)


def _guarded(host, sentinel):
    """(device view of `host`, whole buffer): `host` (numpy, C-contiguous)
    between GUARD sentinel elements on either side."""
    t = torch.from_numpy(np.ascontiguousarray(host).reshape(-1))
    whole = torch.full((t.numel() + 2 * GUARD,), sentinel, dtype=t.dtype).cuda()
    whole[GUARD:GUARD + t.numel()].copy_(t)
    return whole[GUARD:GUARD + t.numel()].view(host.shape), whole


def _guards_intact(whole, sentinel):
    w = whole.cpu()
    return bool((w[:GUARD] == sentinel).all() and (w[-GUARD:] == sentinel).all())


def _state(K_):
    """An ExchangeState whose buffer lies between sentinel bytes."""
    from bayesdll_amd import kernels as Kn
    st = Kn.ExchangeState(K_, torch.device("cuda"))
    view, whole = _guarded(np.zeros(st.buf.numel(), dtype=np.uint8), 0xA5)
    st.buf = view
    return st, whole


# ------------------------------------------------------------------- energy
@pytest.mark.parametrize("name,K_,n,stride", R.GEOMETRY, ids=[g[0] for g in R.GEOMETRY])
def test_energy_is_bit_identical_to_the_reference_at_every_grid(name, K_, n, stride):
    from bayesdll_amd import kernels as Kn
    th, pr = R.make_vectors(name, K_, n, stride)
    want_p, want_q = R.energy_partials(th, pr, n), R.energy(th, pr, n)
    dth, wth = _guarded(th, 3e33)
    dpr, wpr = _guarded(pr, -3e33)
    for prior, wp, wq in ((dpr, want_p, want_q),
                          (None, R.energy_partials(th, None, n), R.energy(th, None, n))):
        for grid in (2, 0):
            st, wst = _state(K_)
            ws = Kn.exchange_energy(dth.view(-1), None if prior is None else prior.view(-1),
                                    chains=K_, chain_groups=stride // 4, n=n, grid_blocks=grid)
            # energy_only: loss and beta are not even given, so they stay unread
            Kn.exchange_decide(st, ws, n=n, energy_only=True)
            got_p = ws.view(torch.float64)[:wp.size].cpu().numpy().reshape(wp.shape)
            got_q = st.q().cpu().numpy()
            assert R.same_bits(got_p, wp), (name, grid)
            assert R.same_bits(got_q, wq), (name, grid, got_q, wq)
            assert st.fresh and _guards_intact(wst, 0xA5)
            # nothing but q was written
            rest = st.buf.cpu().numpy()[8 * R.MAX_CHAINS:]
            assert not rest.any()
    assert _guards_intact(wth, 3e33) and _guards_intact(wpr, -3e33)
    assert np.array_equal(dth.cpu().numpy().view(np.uint32), th.view(np.uint32))  # read only


# ------------------------------------------------------------------- decide
def _planted(q):
    """A one-tile workspace whose partials are q: the cross-tile sum of one
    partial is that partial."""
    return torch.from_numpy(np.asarray(q, dtype=np.float64)).cuda().view(torch.uint8)


def _compare(st, ref, what):
    got = st.summary()
    for f in ("attempts", "accepts", "round_trips", "partner", "replica", "direction"):
        assert np.array_equal(got[f].astype(np.int64), np.asarray(ref[f]).astype(np.int64)), \
            (what, f, got[f], ref[f])
    assert got["refused"] == ref["refused"], what
    assert R.same_bits(got["U"], ref["U"]), (what, got["U"], ref["U"])


@pytest.mark.parametrize("var", R.DECIDE_VARS)
def test_64_consecutive_decisions_equal_the_reference(var):
    from bayesdll_amd import kernels as Kn
    st, wst = _state(R.DECIDE_K)
    ref = R.new_state(R.DECIDE_K)
    beta = torch.from_numpy(R.DECIDE_BETA).cuda()
    for t in range(R.DECIDE_ATTEMPTS):
        q, loss = R.decide_inputs(t)
        R.decide(ref, q, loss, R.DECIDE_BETA, n_data=R.DECIDE_N, sigma2=R.DECIDE_SIGMA2, var=var,
                 seed=R.DECIDE_SEED, chain0=R.DECIDE_CHAIN0, attempt=t)
        Kn.exchange_decide(st, _planted(q), torch.from_numpy(loss).cuda(), beta, n=R.TILE,
                           n_data=R.DECIDE_N, sigma2=R.DECIDE_SIGMA2, var=var,
                           seed=R.DECIDE_SEED, chain0=R.DECIDE_CHAIN0, attempt=t)
        _compare(st, ref, (var, t))
    assert not st.fresh and _guards_intact(wst, 0xA5)
    print(f"var = {var}: accepts {ref['accepts']} of {ref['attempts']}, round trips "
          f"{ref['round_trips']}")


def test_equal_temperatures_accept_every_attempt_and_a_nan_energy_swaps_nothing():
    from bayesdll_amd import kernels as Kn
    st, wst = _state(R.DECIDE_K)
    ref = R.new_state(R.DECIDE_K)
    b = np.full(R.DECIDE_K, 0.5)
    kw = dict(n_data=R.DECIDE_N, sigma2=R.DECIDE_SIGMA2, var=0.0, seed=R.DECIDE_SEED,
              chain0=R.DECIDE_CHAIN0)
    for t in range(R.DECIDE_ATTEMPTS):
        q, loss = R.decide_inputs(t)
        R.decide(ref, q, loss, b, attempt=t, **kw)
        Kn.exchange_decide(st, _planted(q), torch.from_numpy(loss).cuda(),
                           torch.from_numpy(b).cuda(), n=R.TILE, attempt=t, **kw)
    _compare(st, ref, "db = 0")
    got = st.summary()
    assert np.array_equal(got["accepts"], got["attempts"]) and got["attempts"].sum() == 128
    # a NaN energy in slot 1 (both parities meet it), +inf in slot 4: refused, nothing moves
    for t in R.NAN_ATTEMPTS:
        q, loss = R.nan_inputs(t)
        before = st.summary()
        R.decide(ref, q, loss, R.DECIDE_BETA, attempt=t, **kw)
        Kn.exchange_decide(st, _planted(q), torch.from_numpy(loss).cuda(),
                           torch.from_numpy(R.DECIDE_BETA).cuda(), n=R.TILE, attempt=t, **kw)
        _compare(st, ref, ("nan", t))
        got = st.summary()
        touched = [0, 1] if t % 2 == 0 else [1, 2]  # slots of the pair that holds the NaN
        assert all(got["partner"][k] == k for k in touched)
        assert got["refused"] == before["refused"] + (1 if t % 2 == 0 else 2)
        assert np.array_equal(got["accepts"][touched[0]], before["accepts"][touched[0]])
    assert _guards_intact(wst, 0xA5)


# --------------------------------------------------------------------- swap
@pytest.mark.parametrize("nvec", [1, 2, 3, 4])
@pytest.mark.parametrize("K_,stride,partner", [
    (5, 1028, [1, 0, 2, 4, 3]), (5, 1028, [0, 2, 1, 3, 4]), (5, 1028, [0, 1, 2, 3, 4]),
    (2, 4, [1, 0]), (1, 1500, [0]), (3, 300000, [0, 2, 1])])
def test_swap_equals_the_reference_permutation_bit_for_bit(nvec, K_, stride, partner):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as Kn
    rng = np.random.default_rng(5 * nvec + K_)
    hosts = [rng.standard_normal((K_, stride)).astype(np.float32) for _ in range(nvec)]
    for h in hosts:
        h[:, -1] = 1e30 * (1 + np.arange(K_))  # a padding sentinel per slot: it must travel
    want = R.swap(hosts, partner)
    for grid in (2, 0):
        pairs = [_guarded(h, 4e33) for h in hosts]
        st, wst = _state(K_)
        raw = np.zeros(1, dtype=np.dtype(L.ExchangeState))
        raw["partner"][0, :K_] = partner
        st.buf.copy_(torch.from_numpy(raw.view(np.uint8).reshape(-1)))
        before = st.buf.clone()
        Kn.exchange_swap(st, [v.view(-1) for v, _ in pairs], chain_groups=stride // 4,
                         grid_blocks=grid)
        for (v, whole), w in zip(pairs, want):
            assert np.array_equal(v.cpu().numpy().view(np.uint32), w.view(np.uint32))
            assert _guards_intact(whole, 4e33)
        assert torch.equal(st.buf, before) and _guards_intact(wst, 0xA5)
    if partner == [1, 0, 2, 4, 3]:  # the padding travelled, the staying chain stayed
        assert want[0][0, -1] == np.float32(2e30) and np.array_equal(want[0][2], hosts[0][2])


# ------------------------------------------------------------------ sampler
LADDER = [1.0, 1.4, 2.0, 2.8]


@pytest.fixture(scope="module")
def loader():
    g = torch.Generator().manual_seed(8)
    xs = torch.randn(160, 13, generator=g)
    ys = (xs[:, :5] + 0.5 * torch.randn(160, 5, generator=g)).argmax(-1)
    return [(xs[i:i + 16].cuda(), ys[i:i + 16].cuda()) for i in range(0, 160, 16)]  # 10 batches


def _sampler(cls="StackedSGLD", nd=LADDER, hp=None, **kw):
    from bayesdll_amd import stacked
    torch.manual_seed(31)
    a = _args(nst=0, momentum=0.0, epochs=4)
    a.hparams.update(hp or {})
    return getattr(stacked, cls)(Net().cuda(), len(nd), a, init="reinit",
                                 seed=4, chain0=2, graph=False, per_chain={"nd": nd}, **kw)


@pytest.mark.parametrize("cls", ["StackedSGLD", "StackedCSGLD"])
def test_forty_steps_leave_a_permutation_and_count_every_attempt(loader, cls):
    S = _sampler(cls, exchange_every=1)
    for ep in range(4):
        S.train_one_epoch(loader, ep)
    d = S.exchange()
    print(d)
    assert S.step_count == 40 and d["attempt"] == 40
    assert sorted(d["replica"]) == [0, 1, 2, 3] and d["refused"] == 0
    assert [p["attempts"] for p in d["pairs"]] == [20, 20, 20]     # pairs 0, 2 even; pair 1 odd
    assert all(0 <= p["accepts"] <= p["attempts"] for p in d["pairs"])
    assert [p["temperatures"] for p in d["pairs"]] == [(n0 * n0, n1 * n1)
                                                       for n0, n1 in zip(LADDER, LADDER[1:])]
    assert d["cold"] == [0] and d["round_trips_total"] == sum(d["round_trips"])
    assert torch.isfinite(S.state.theta).all()
    # every other step only: half the attempts
    S2 = _sampler(cls, exchange_every=2)
    S2.train_one_epoch(loader, 0)
    assert S2.exchange()["attempt"] == 5


def test_without_an_accepted_swap_theta_is_bit_identical_to_exchange_off(loader):
    """exchange_var so large that la = -db^2 * var rejects everything: the
    exchange draws share no Philox key with the training noise."""
    S_on, S_off = _sampler(exchange_every=1, exchange_var=1e30), _sampler()
    for x, y in (loader + loader)[:10]:
        S_on.step(x, y, (5e-2, 1e-1))
        S_off.step(x, y, (5e-2, 1e-1))
    d = S_on.exchange()
    assert d["attempt"] == 10 and sum(p["accepts"] for p in d["pairs"]) == 0
    assert sum(p["attempts"] for p in d["pairs"]) == 15 and d["replica"] == [0, 1, 2, 3]
    assert torch.equal(S_on.state.theta, S_off.state.theta)
    assert torch.equal(S_on.state.mom, S_off.state.mom) and S_on.draws == S_off.draws
    assert "exchange_state" not in S_off.state_dict()             # existing checkpoints keep their keys
    with pytest.raises(ValueError, match="replica exchange is off"):
        S_off.exchange()


def test_a_checkpoint_continues_bit_for_bit(loader, tmp_path):
    A = _sampler(exchange_every=1)
    A.train_one_epoch(loader, 0)
    path = A.save_ckpt(str(tmp_path / "x.pt"))
    A.train_one_epoch(loader, 1)
    B = _sampler(exchange_every=1)
    B.load_ckpt(path)
    B.train_one_epoch(loader, 1)
    assert torch.equal(A.state.theta, B.state.theta) and A.exchange() == B.exchange()
    assert A.exchange()["attempt"] == 20
    print(A.exchange())
    C = _sampler()
    C.train_one_epoch(loader, 0)
    with pytest.raises(ValueError, match="without exchange_every"):
        _sampler(exchange_every=1).load_ckpt(C.save_ckpt(str(tmp_path / "c.pt")))


@pytest.mark.parametrize("nd,cold", [(LADDER, 0), (LADDER[::-1], 3)])
def test_cold_weights_equal_the_cold_slots_row_of_evaluate_chains(loader, nd, cold):
    """kernels.mixture with all weight on one chain against torch's fp64
    logsumexp of the same chain: fp32 probabilities and logf, a few 2^-24
    relative on an NLL of order 1 (1e-5 absolute, as the stacking tests)."""
    S = _sampler(nd=nd, exchange_every=2)
    for ep in range(2):
        S.train_one_epoch(loader, ep)
    assert S.cold_slots() == [cold]
    nll_c, err_c = S.evaluate(loader, weights="cold")
    nll_k, err_k = S.evaluate_chains(loader)
    print(f"cold {nll_c:.7f} {err_c:.4f}; chains {nll_k} {err_k}")
    assert abs(nll_c - nll_k[cold]) <= 1e-5 and abs(err_c - err_k[cold]) < 1e-12
    u = S.uncertainty(loader, weights="cold")
    assert abs(u["nll"] - nll_c) <= 1e-5
    t = S.fit_temperature(loader, weights="cold")
    assert abs(t["nll_before"] - nll_c) <= 1e-5
    with pytest.raises(ValueError, match="pooled form only"):
        S.evaluate_chains(loader, weights="cold")
    with pytest.raises(ValueError, match='combine="reference"'):
        S.evaluate(loader, weights="cold", combine="reference")


@pytest.mark.parametrize("cls,kw,akw,why", REFUSALS)
def test_refusals_name_their_reason_on_the_device(cls, kw, akw, why):
    from bayesdll_amd import stacked
    a = _args(nst=0, momentum=akw.get("momentum", 0.0))
    a.hparams["bias"] = akw.get("bias", "informative")
    with pytest.raises(ValueError, match=why):
        getattr(stacked, cls)(Net().cuda(), 3, a, exchange_every=2, graph=False, **kw)


def test_frozen_tensors_and_dropout_are_refused_on_the_device():
    from bayesdll_amd import stacked
    from test_exchange_host import frozen_net
    kw = dict(exchange_every=2, graph=False, per_chain={"nd": [1, 2, 3]})
    with pytest.raises(ValueError, match="frozen tensors"):
        stacked.StackedSGLD(frozen_net(Net()).cuda(), 3, _args(nst=0, momentum=0.0), **kw)

    class DropNet(Net):
        def __init__(self):
            super().__init__()
            self.drop = torch.nn.Dropout(0.1)

    with pytest.raises(ValueError, match="dropout layers"):
        stacked.StackedSGLD(DropNet().cuda(), 3, _args(nst=0, momentum=0.0), **kw)


def test_the_sampler_hands_the_kernels_the_energy_of_its_own_update(loader):
    """U of an attempt against N * loss + q / (2 sigma2) recomputed in torch
    from the UPDATED theta, the prior and the same batch, with N = ND *
    Ninflate, sigma2 = prior_sig^2 (both != 1 here) and beta = 1 / nd^2.
    exchange_var rejects every swap, so theta after the step is the theta the
    energy was taken at.  Bound: the loss is the same fp32 ops on the same
    inputs (4 ulp of fp32 allowed for a differently scheduled GEMM), q differs
    by the order of an fp64 sum of n non-negative terms (n * 2^-52 relative)."""
    S = _sampler(hp={"prior_sig": 0.7, "Ninflate": 3.0}, exchange_every=1, exchange_var=1e30)
    st = S.state
    assert np.array_equal(S._xbeta.cpu().numpy(), 1.0 / np.asarray(LADDER) ** 2)
    for i, (x, y) in enumerate(loader[:3]):
        before = st.theta.clone()
        pre_loss, _ = S.step(x, y, (5e-2, 1e-1))
        assert not torch.equal(before, st.theta)
        got = S._xstate.summary()
        with torch.no_grad():
            out = S._fwd(st.params, x)
            loss = torch.stack([S.criterion(out[k], y) for k in range(S.K)]).double()
            d = (st.theta2d[:, :st.n1] - st.prior.view(S.K, st.stride)[:, :st.n1]).double()
            q = (d * d).sum(1)
        N, s2 = S.args.ND * 3.0, 0.7 ** 2
        want = (N * loss + q / (2 * s2)).cpu().numpy()
        bound = 4 * 2.0 ** -24 * N * loss.abs().cpu().numpy() \
            + st.n1 * 2.0 ** -52 * (q / (2 * s2)).cpu().numpy()
        print(f"step {i}: U {got['U']}, recomputed {want}, bound {bound}")
        assert (np.abs(got["U"] - want) <= bound).all()
        assert R.same_bits(got["q"], R.energy(st.theta2d.cpu().numpy(),
                                              st.prior.view(S.K, st.stride).cpu().numpy(), st.n1))
        # the loss of the step itself (before the update) is another number
        stale = (N * pre_loss.double() + q / (2 * s2)).cpu().numpy()
        assert (np.abs(stale - want) > 100 * bound).all()
        assert sum(p["accepts"] for p in S.exchange()["pairs"]) == 0
