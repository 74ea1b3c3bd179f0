"""bdl_chain_stats (include/bdl_stats.h) on the GPU against its restatement
(tests/chain_stats_ref.py), and the samplers' health() built on it.

Kernel cases: table A of tests/stacked_tables.py (3 padded chains, one frozen
tensor, numel 3, 4, 5, 8, 10, 12 among them) plus one tensor of 4,099
elements — odd and longer than a block iteration, so rows 1 and 2 of its
[K, numel] gradient are misaligned against theta and take the element-wise
path with a full and a partial iteration.  Two gradient forms:

  tensor  every trainable tensor its own [K, numel] block (chain stride =
          numel) in one arena between guard NaNs;
  flat    one [K, slot] stacked gradient vector (chain stride = the slot).

Slot padding and the frozen tensor's span hold NaN in every vector: a sum
that read them would be NaN."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import chain_stats_ref as R
from stacked_tables import FROZEN, SEGMENTS, Layout
from test_gpu_stacked import Net, _args

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_ = 3
ODD = ("l9.weight", 4099)
LR = (0.05, 0.125)
FORMS = ("tensor", "flat")
BOUND = [(True, True), (True, False), (False, True), (False, False)]  # (mom, prior)


@functools.lru_cache(maxsize=None)
def _layout():
    lay = Layout(SEGMENTS + [ODD], K_)
    idx = [i for i, nm in enumerate(lay.names) if nm != FROZEN]
    return lay, idx


def _lr_rows():
    """A real [K, 12] scalar block of a per_chain cSGHMC step (lr in columns 0, 1)."""
    from bayesdll_amd import per_chain as PC
    a = _args()
    tab = PC.parse({"lr": [0.01, 0.02, 0.04], "lr_head": [0.03, 0.01, 0.08]}, K_, "csghmc",
                   PC.defaults(a, "csghmc"))
    return PC.csghmc_rows(tab, tab["lr"], a.ND)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """Host data of a case (read-only): the stacked vectors [K, slot] with NaN
    on padding and the frozen span, the gradient per tensor [K, numel], and
    the reference sums / sums of |terms| [mom][prior][lr source] -> [K, T, 6]."""
    lay, idx = _layout()
    rng = np.random.default_rng(7 if kind == "integer" else 11)
    vec = {nm: np.full((K_, lay.stride), np.nan, dtype=np.float32)
           for nm in ("theta", "mom", "prior")}
    grads = {}
    for i in idx:
        o, n = lay.offsets[i], lay.numels[i]
        for nm, sc in (("theta", 0.3), ("mom", 1e-3), ("prior", 0.3)):
            vec[nm][:, o:o + n] = rng.integers(-64, 65, (K_, n)) if kind == "integer" \
                else sc * rng.standard_normal((K_, n))
        grads[i] = (rng.integers(-64, 65, (K_, n)) if kind == "integer"
                    else 1e-2 * rng.standard_normal((K_, n))).astype(np.float32)
    rows = _lr_rows()
    ref = {}
    for mom, prior in BOUND:
        for src in ("host", "table"):
            s = np.zeros((K_, len(idx), 6))
            a = np.zeros_like(s)
            for k in range(K_):
                for t, i in enumerate(idx):
                    o, n = lay.offsets[i], lay.numels[i]
                    grp = 1 if lay.names[i].startswith("head") else 0
                    lr = LR[grp] if src == "host" else rows[k, grp]
                    s[k, t], a[k, t] = R.sums(
                        grads[i][k], vec["theta"][k, o:o + n],
                        vec["mom"][k, o:o + n] if mom else None,
                        vec["prior"][k, o:o + n] if prior else None, lr)
            ref[(mom, prior, src)] = (s, a)
    for v in list(vec.values()) + list(grads.values()):
        v.setflags(write=False)
    return vec, grads, ref


class _Device:
    """A case on the device: the stacked vectors, the gradient in one form and
    its segment table."""

    def __init__(self, kind, form):
        lay, idx = _layout()
        vec, grads, self.ref = _case(kind)
        self.lay, self.idx = lay, idx
        self.vec = {nm: torch.from_numpy(v.copy()).to(DEV) for nm, v in vec.items()}
        rows = []
        if form == "flat":
            g = np.full((K_, lay.stride), np.nan, dtype=np.float32)
            for i in idx:
                g[:, lay.offsets[i]:lay.offsets[i] + lay.numels[i]] = grads[i]
            self.grad = torch.from_numpy(g).to(DEV)
            for i in idx:
                rows.append((self.grad.data_ptr() + 4 * lay.offsets[i], lay.numels[i], lay.stride))
        else:
            pos, place = 8, {}
            for i in idx:
                place[i] = pos
                pos = (pos + K_ * lay.numels[i] + 8 + 3) // 4 * 4  # guard words, 16-B aligned blocks
            g = np.full(pos, np.nan, dtype=np.float32)
            for i in idx:
                g[place[i]:place[i] + K_ * lay.numels[i]] = grads[i].reshape(-1)
            self.grad = torch.from_numpy(g).to(DEV)
            assert self.grad.data_ptr() % 16 == 0
            for i in idx:
                rows.append((self.grad.data_ptr() + 4 * place[i], lay.numels[i], lay.numels[i]))
        self.rows = [r + (lay.offsets[i], 1 if lay.names[i].startswith("head") else 0)
                     for r, i in zip(rows, idx)]
        self.table = torch.tensor(self.rows, dtype=torch.int64).to(DEV)
        self.lr_rows = torch.from_numpy(_lr_rows()).to(DEV)
        assert self.lr_rows.shape == (K_, 12)
        self.before = {nm: v.clone() for nm, v in self.vec.items()}
        self.grad_before = self.grad.clone()

    def run(self, mom=True, prior=True, src="host", bpc=0, acc=None, accumulate=False):
        from bayesdll_amd import kernels as K
        T = len(self.idx)
        if acc is None:
            acc = torch.full((K_, T, 6), float("nan"), dtype=torch.float64, device=DEV)
        kw = {"lr": LR} if src == "host" else {"lr_table": self.lr_rows, "lr_row_stride": 12}
        K.chain_stats(self.table, T, K_, self.lay.chain_groups, self.vec["theta"].view(-1), acc,
                      mom=self.vec["mom"].view(-1) if mom else None,
                      prior_mean=self.vec["prior"].view(-1) if prior else None,
                      accumulate=accumulate, blocks_per_chain=bpc, **kw)
        torch.cuda.synchronize()
        return acc.cpu().numpy()

    def unchanged(self):
        same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731
        return same(self.grad, self.grad_before) and all(
            same(self.vec[nm], self.before[nm]) for nm in self.vec)


def test_table_holds_what_the_cases_claim():
    lay, idx = _layout()
    assert lay.stride - lay.n1 == 3 and len(idx) == 20 and lay.numels[-1] == 4099
    assert lay.n1 == 39426 + 4099 and lay.offsets[-1] == 39426
    d = _Device("integer", "tensor")
    # (chain, tensor) pairs whose gradient and theta slices are misaligned alike / differently
    alike = sum(1 for ptr, n, gs, o, _ in d.rows for k in range(K_)
                if (ptr // 4 + k * gs) % 4 == (k * lay.stride + o) % 4)
    assert 0 < alike < K_ * len(idx)
    ptr, n, gs, o, _ = d.rows[-1]   # the odd tensor: chains 1 and 2 differ from theta
    assert [(ptr // 4 + k * gs) % 4 != (k * lay.stride + o) % 4 for k in range(K_)] == \
        [True, True, False]
    assert n > 4096  # a full block iteration on the element-wise path at one workgroup
    f = _Device("integer", "flat")
    assert all((p // 4 + k * gs) % 4 == (k * lay.stride + o) % 4
               for p, _, gs, o, _ in f.rows for k in range(K_))  # flat: always the 16-B path
    assert sum(g for *_, g in d.rows) == 2  # head.weight, head.bias


@pytest.mark.parametrize("form", FORMS)
def test_integer_inputs_are_exact_in_every_configuration(form):
    """|x| <= 64 and integer: every product and partial sum is an integer far
    below 2^53, so all six sums equal the reference bit for bit on every load
    path, geometry, stream set and lr source (V2L: the same two fp64 ops)."""
    d = _Device("integer", form)
    for mom, prior in BOUND:
        for src in ("host", "table"):
            want = d.ref[(mom, prior, src)][0]
            for bpc in (1, 3, 0):
                got = d.run(mom, prior, src, bpc)
                assert np.isfinite(got).all(), (form, mom, prior, src, bpc)
                assert np.array_equal(got, want), (form, mom, prior, src, bpc,
                                                   np.argwhere(got != want)[:4])
            if not mom:
                assert not want[..., [1, 4, 5]].any()
    assert d.unchanged()


@pytest.mark.parametrize("form", FORMS)
def test_random_inputs_within_the_summation_bound(form):
    d = _Device("random", form)
    numel = np.asarray([d.lay.numels[i] for i in d.idx], dtype=np.float64)
    for mom, prior in BOUND:
        for src in ("host", "table"):
            want, absum = d.ref[(mom, prior, src)]
            bound = 2.0 * numel[None, :, None] * 2.0 ** -53 * absum
            for bpc in (1, 3, 0):
                got = d.run(mom, prior, src, bpc)
                err = np.abs(got - want)
                print(form, mom, prior, src, bpc, "max err / bound",
                      float(np.max(err / np.where(bound > 0, bound, 1))))
                assert np.isfinite(got).all()
                assert (err <= bound).all(), (form, mom, prior, src, bpc,
                                              np.argwhere(err > bound)[:4])
    a1, a2 = d.run(bpc=5), d.run(bpc=5)
    assert np.array_equal(a1.view(np.int64), a2.view(np.int64))  # same geometry: bit-identical
    assert d.unchanged()


def test_accumulate_adds_and_overwrite_overwrites():
    d = _Device("integer", "tensor")
    want = d.ref[(True, True, "host")][0]
    T = len(d.idx)
    garbage = torch.full((K_, T, 6), 12345.678, dtype=torch.float64, device=DEV)
    garbage[0, 0, 0] = float("nan")
    assert np.array_equal(d.run(acc=garbage, accumulate=False), want)
    acc = torch.zeros(K_, T, 6, dtype=torch.float64, device=DEV)
    d.run(acc=acc, accumulate=True)
    assert np.array_equal(d.run(acc=acc, accumulate=True), 2 * want)
    assert d.unchanged()


# ------------------------------------------------------------------ samplers
PLAN = [(0.05, False), (0.04, True), (0.03, False), (0.02, True)]
PER_CHAIN = {"lr": [0.05, 0.02, 0.08], "momentum_decay": [0.1, 0.3, 0.05], "nd": [1.0, 0.5, 2.0]}


def _pair(cls, graph=False, per_chain=None, every=1):
    from bayesdll_amd import stacked
    out = []
    for he in (every, 0):
        torch.manual_seed(0)
        kw = {} if per_chain is None else {"per_chain": per_chain}
        out.append(getattr(stacked, cls)(Net().cuda(), K_, _args(), chain0=5, init="reinit",
                                         graph=graph, health_every=he, **kw))
    return out


def _collect(S, m1, m2, n):
    from bayesdll_amd import _lib as L
    return (L.COLLECT_WELFORD_INIT if n == 1 else L.COLLECT_WELFORD, m1, m2, float(n))


def _drive(S, T_, x, y, lr_of):
    """PLAN through S.step (health on) and through the twin's gradients() /
    update() with snapshots before each update.  Returns the twin's snapshots
    [(grads {name: [K, numel]}, theta [K, slot], mom [K, slot], lr)]."""
    bufs = [[torch.zeros(S.state.n, device=DEV) for _ in range(2)] for _ in range(2)]
    snaps, n = [], 0
    for lr, ss in PLAN:
        n += ss
        lr = lr_of(lr)
        S.step(x, y, lr, should_sample=ss, collect=_collect(S, *bufs[0], n) if ss else None)
        grads, _, _ = T_.gradients(x, y)
        st = T_.state
        snaps.append(({nm: g.detach().reshape(K_, -1).cpu().numpy().copy()
                       for nm, g in grads.items()},
                      st.theta2d.cpu().numpy().copy(), st.mom2d.cpu().numpy().copy(), lr))
        T_.update(grads, lr, ss, _collect(T_, *bufs[1], n) if ss else None)
    torch.cuda.synchronize()
    return snaps


def _exact_reference(T_, snaps, lr_rows_of):
    """Exact (Fraction) sums over the twin's snapshots: [K][T][6] and |terms|."""
    st = T_.state
    idx = [i for i, rg in enumerate(st.requires_grad) if rg]
    tot = [[[Fraction(0)] * 6 for _ in idx] for _ in range(K_)]
    ab = [[[Fraction(0)] * 6 for _ in idx] for _ in range(K_)]
    for grads, th, mv, lr in snaps:
        rows = lr_rows_of(lr)
        for k in range(K_):
            for t, i in enumerate(idx):
                o, n = st.offsets[i], st.numels[i]
                grp = 1 if st.names[i].startswith("head") else 0
                s, a = R.exact_sums(grads[st.names[i]][k], th[k, o:o + n], mv[k, o:o + n], None,
                                    rows[k][grp])
                tot[k][t] = [p + q for p, q in zip(tot[k][t], s)]
                ab[k][t] = [p + q for p, q in zip(ab[k][t], a)]
    return idx, tot, ab


def _check_sums(h, T_, idx, tot, ab):
    """The random-input bound per entry, in exact arithmetic: the device adds
    n exact terms per launch and one accumulate per launch (n - 1 + steps
    roundings <= 2n for these shapes: n >= 5, 4 steps, V2L's two more)."""
    st = T_.state
    assert h["names"] == [st.names[i] for i in idx] and h["numel"] == [st.numels[i] for i in idx]
    worst = 0.0
    for k in range(K_):
        for t, i in enumerate(idx):
            for q in range(6):
                err = abs(Fraction(float(h["sums"][k, t, q])) - tot[k][t][q])
                bound = 2 * st.numels[i] * Fraction(1, 2 ** 53) * ab[k][t][q]
                worst = max(worst, float(err / bound) if bound else float(err))
                assert err <= bound, (k, st.names[i], R.ORDER[q], float(err), float(bound))
    print("sampler sums: max err / bound", worst)


def _check_twin(S, T_):
    assert torch.equal(S.state.theta.view(torch.int32), T_.state.theta.view(torch.int32))
    assert torch.equal(S.state.mom.view(torch.int32), T_.state.mom.view(torch.int32))
    assert S.step_count == T_.step_count == len(PLAN)


def _xy():
    g = torch.Generator(device=DEV).manual_seed(3)
    return (torch.randn(16, 13, device=DEV, generator=g),
            torch.randint(0, 5, (16,), device=DEV, generator=g))


def test_csghmc_health_equals_the_twin_reference_uniform():
    S, T_ = _pair("StackedCSGHMC")
    a = S.args
    x, y = _xy()
    snaps = _drive(S, T_, x, y, lambda lr: lr)
    lrs = lambda lr: [[np.float32(lr), np.float32(lr * (a.lr_head / a.lr))]] * K_  # noqa: E731
    idx, tot, ab = _exact_reference(T_, snaps, lrs)
    h = S.health(reset=False)
    assert h["steps"] == 4
    _check_sums(h, T_, idx, tot, ab)
    _check_twin(S, T_)
    ref_acc = np.array([[[float(v) for v in tot[k][t]] for t in range(len(idx))]
                        for k in range(K_)])
    want = R.temperatures(ref_acc, 4, h["numel"], [0.1] * K_, [1.0] * K_, [64.0] * K_, [1.0] * K_)
    want.update(R.rms_table(ref_acc, 4, h["numel"]))
    for key, w in want.items():
        print(key, np.max(np.abs(h[key] - w) / np.abs(w)))
        np.testing.assert_allclose(h[key], w, rtol=1e-12, err_msg=key)
    # reset empties the accumulators; the next sweep starts from zero
    assert S.health(reset=True)["steps"] == 4
    h0 = S.health()
    assert h0["steps"] == 0 and not h0["sums"].any() and np.isnan(h0["t_kin"]).all()


def test_csghmc_health_per_chain_uses_each_chains_values():
    from bayesdll_amd import per_chain as PC
    S, T_ = _pair("StackedCSGHMC", per_chain=PER_CHAIN)
    x, y = _xy()
    base = np.asarray(PER_CHAIN["lr"])
    snaps = _drive(S, T_, x, y, lambda lr: base * (lr / 0.05))
    rows_of = lambda lr: PC.csghmc_rows(T_.per_chain, lr, T_.args.ND)  # noqa: E731
    idx, tot, ab = _exact_reference(T_, snaps, rows_of)
    h = S.health()
    assert h["steps"] == 4
    _check_sums(h, T_, idx, tot, ab)
    _check_twin(S, T_)
    ref_acc = np.array([[[float(v) for v in tot[k][t]] for t in range(len(idx))]
                        for k in range(K_)])
    want = R.temperatures(ref_acc, 4, h["numel"], PER_CHAIN["momentum_decay"], PER_CHAIN["nd"],
                          [64.0] * K_, [1.0] * K_)
    for key, w in want.items():
        np.testing.assert_allclose(h[key], w, rtol=1e-12, err_msg=key)
    # chain k's own values matter: the uniform defaults give other temperatures
    other = R.temperatures(ref_acc, 4, h["numel"], [0.1] * K_, [1.0] * K_, [64.0] * K_, [1.0] * K_)
    assert not np.allclose(h["t_kin"][1:], other["t_kin"][1:], rtol=1e-3)


def test_other_samplers_return_the_rms_table_only():
    S, T_ = _pair("StackedSGLD", every=2)
    x, y = _xy()
    for _ in range(4):
        S.step(x, y, (0.05, 0.1))
        T_.step(x, y, (0.05, 0.1))
    torch.cuda.synchronize()
    h = S.health()
    assert h["steps"] == 2                     # cadence: steps 0 and 2 of 4
    assert not any(k.startswith("t_") for k in h)
    for k in ("grad_rms", "mom_rms", "dist_rms", "grad_mom_cos"):
        assert h[k].shape == (K_, len(h["names"]))
    assert np.isfinite(h["grad_rms"]).all() and (h["grad_rms"] > 0).all()
    assert torch.equal(S.state.theta.view(torch.int32), T_.state.theta.view(torch.int32))
    with pytest.raises(ValueError, match="health_every=0"):
        T_.health()
    assert T_._health is None                  # off: nothing allocated


class _IntNet(torch.nn.Module):
    readout_name = "head"

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Linear(6, 5)
        self.head = torch.nn.Linear(5, 3)

    def forward(self, x):
        return self.head(self.body(x))


def test_graph_mode_on_and_off_agree_on_integer_exact_sums():
    """A linear network, integer parameters, momentum and inputs and the loss
    sum(logits): every gradient is an integer, so the first step's sums are
    exact — the same bits from the eager and the graph-replayed backward, and
    the reference's."""
    from bayesdll_amd import stacked
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randint(-4, 5, (8, 6), device=DEV, generator=g).float()
    y = torch.zeros(8, dtype=torch.int64, device=DEV)
    sums = []
    for graph in (False, True):
        torch.manual_seed(0)
        S = stacked.StackedCSGHMC(_IntNet().cuda(), K_, _args(), chain0=5, graph=graph,
                                  health_every=1, criterion=lambda out, yy: out.sum())
        st = S.state
        gi = torch.Generator(device=DEV).manual_seed(9)
        st.theta2d[:, :st.n1] = torch.randint(-3, 4, (K_, st.n1), device=DEV, generator=gi).float()
        st.mom2d[:, :st.n1] = torch.randint(-3, 4, (K_, st.n1), device=DEV, generator=gi).float()
        th, mv = st.theta2d.cpu().numpy().copy(), st.mom2d.cpu().numpy().copy()
        grads, _, _ = S.gradients(x, y)
        gh = {nm: v.detach().reshape(K_, -1).cpu().numpy().copy() for nm, v in grads.items()}
        S.step(x, y, 0.0625)
        torch.cuda.synchronize()
        h = S.health()
        assert h["steps"] == 1
        want = np.zeros_like(h["sums"])
        for k in range(K_):
            for t, nm in enumerate(h["names"]):
                i = st.names.index(nm)
                o, n = st.offsets[i], st.numels[i]
                assert np.array_equal(gh[nm][k], np.round(gh[nm][k]))
                lr = 0.0625 * (2.0 if nm.startswith("head") else 1.0)  # lr_head / lr = 2
                want[k, t] = R.sums(gh[nm][k], th[k, o:o + n], mv[k, o:o + n], None, lr)[0]
        assert np.array_equal(h["sums"], want), graph
        sums.append(h["sums"])
        S.release_graphs()
    assert np.array_equal(sums[0], sums[1])
