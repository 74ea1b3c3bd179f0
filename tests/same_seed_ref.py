"""Same-seed reference chains — TEST INFRASTRUCTURE ONLY.

The reference samplers run step by step on a `FakeNet`, on "cpu" or "cuda",
with nothing but the oracle's per-tensor rules (oracle/sgmcmc_oracle.py) and
`torch.randn_like(p)` drawn from torch's global generator exactly where the
reference draws it:

  * per tensor, in named_parameters order, inside the Model's loop
    (methods/csghmc.py:766, methods/sgld.py:474/:479, methods/sghmc.py,
    methods/adam_sghmc.py);
  * only for tensors whose .grad is not None after zero_grad + backward
    (`if p.grad is not None`, e.g. methods/csghmc.py:749);
  * on every step, cSGHMC's explore steps included (the draw at :766 is made
    and then dropped);
  * cyclical SGLD with clip_grad: Model.forward draws while it forms the
    sampler gradient (methods/csgld.py:674/:679), and the Runner clips that
    noisy gradient afterwards (:250-251) — the clip makes no generator call;
  * evaluation draws: one randn_like per parameter, frozen ones included, per
    posterior sample (methods/sgld.py:292-296), from the same global generator
    the training steps use.

`RefChain` records the draws of every step, so a test can compare the
product's noise buffer with them bit for bit, apart from any arithmetic.
`misalign=` runs a deliberately WRONG stream (see MISALIGNMENTS): the host
tests use it to show that each comparison would notice such a slip.

Nothing here imports the product.
"""
from __future__ import annotations

import numpy as np
import torch

from fakenet import TOY_READOUT, TOY_SEGMENTS, FakeNet, fake_loader, init_vector, numel_of
from oracle import sgmcmc_oracle as O

RTOL = 1e-5  # north-star tolerance on the updated parameter vector (fp32)


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


# ------------------------------------------------------------------- tables
MANY_SIZES = (1, 2, 3, 5, 7, 64, 129, 1027)


def many_segments(count=40):
    """`count` tensors, sizes cycling through MANY_SIZES (flat offsets are
    rarely multiples of 4), weight / bias names in pairs, a two-tensor readout."""
    segs = []
    for i in range(count - 2):
        segs.append((f"layer{i // 2}.{'bias' if i % 2 else 'weight'}", (MANY_SIZES[i % 8],)))
    return segs + [("classifier.weight", (10, 13)), ("classifier.bias", (10,))]


def mlp_segments():
    """The mlp_mnist configuration's table (fakenet.MLP: 8 tensors, 2,797,010)."""
    from fakenet import MLP
    return [(nm, tuple(p.shape)) for nm, p in MLP().named_parameters()]


_TABLES = {"toy": lambda: list(TOY_SEGMENTS), "many": many_segments, "mlp": mlp_segments}


def segments_of(table):
    return _TABLES[table]()


# -------------------------------------------------------------------- cases
def case(method, table="toy", steps=6, **kw):
    """One chain: sampler, table, scalars.  pattern: should_sample per step
    (cSGHMC; None = sample every step).  frozen: names built with
    requires_grad=False.  skip: a cycle of name tuples, skip[k % len(skip)]
    being the tensors whose backward returns None in step k."""
    c = dict(method=method, table=table, steps=steps, grad_seed=77, noise_seed=4242, init_seed=3,
             prior_seed=4, lr=0.03, lr_head=0.07, prior_sig=0.9, alpha=0.2, N=60.0, nd=0.7,
             bias="informative", momentum=0.0, clip_grad=None, temperature=1.0, beta1=0.9,
             beta2=0.999, epsilon=1e-8, pattern=None, frozen=(), skip=None)
    unknown = set(kw) - set(c)
    if unknown:
        raise KeyError(f"unknown case fields {sorted(unknown)}")
    c.update(kw)
    if c["pattern"] is not None and len(c["pattern"]) != steps:
        raise ValueError("pattern: one should_sample flag per step")
    return c


INTERLEAVED = (False, False, True, False, True, True)

# the seven samplers; csgld's bound is far below the sampler gradient's norm
# (tests/test_same_seed_host.py asserts that every step clips)
SAMPLERS = {
    "csghmc": dict(method="csghmc"),
    "sghmc": dict(method="sghmc"),
    "sgld_mom": dict(method="sgld", momentum=0.5),
    "sgld_uninf": dict(method="sgld", bias="uninformative", momentum=0.5),
    "csgld_clip": dict(method="csgld", momentum=0.5, clip_grad=2.0),
    "adam_sghmc_mom": dict(method="adam_sghmc", momentum=0.5),
    "adam_csghmc_temp": dict(method="adam_csghmc", temperature=1.7),
}

# a frozen tensor in the middle, one tensor without a gradient on even steps,
# another on odd steps, and tensors after all of them
NO_GRAD_TOY = dict(frozen=("layer1.weight",), skip=(("layer0.bias",), ("layer2.weight",)))
NO_GRAD_MANY = dict(table="many", frozen=("layer7.bias",),
                    skip=(("layer3.weight",), ("layer11.bias", "layer12.weight")))

CASES = {}
for _nm, _kw in SAMPLERS.items():
    CASES[f"{_nm}-toy"] = case(**_kw)
    CASES[f"{_nm}-many"] = case(table="many", **_kw)
CASES["csghmc-interleaved-toy"] = case("csghmc", pattern=INTERLEAVED)
CASES["csghmc-interleaved-many"] = case("csghmc", table="many", pattern=INTERLEAVED)
CASES["csghmc_fs-interleaved-toy"] = case("csghmc_fs", pattern=INTERLEAVED)
for _nm in ("csghmc", "sghmc", "sgld_mom", "csgld_clip", "adam_sghmc_mom", "adam_csghmc_temp"):
    CASES[f"{_nm}-nograd-toy"] = case(**SAMPLERS[_nm], **NO_GRAD_TOY)
CASES["csghmc-interleaved-nograd-many"] = case("csghmc", pattern=INTERLEAVED, **NO_GRAD_MANY)
CASES["adam_sghmc_mom-nograd-many"] = case(**SAMPLERS["adam_sghmc_mom"], **NO_GRAD_MANY)
CASES["csghmc-mlp"] = case("csghmc", table="mlp", steps=3)
CASES["adam_sghmc-mlp"] = case("adam_sghmc", table="mlp", steps=3, momentum=0.5)

# cases with tensors that get no gradient run in both gradient modes
NO_GRAD_CASES = [nm for nm, c in CASES.items() if c["frozen"] or c["skip"]]

# what each method owns next to theta
OWNED = {"csghmc": ("mom",), "csghmc_fs": ("mom",), "sghmc": ("mom",), "sgld": ("sgd_buf",),
         "csgld": ("sgd_buf",), "adam_sghmc": ("mom", "adam_m", "adam_v", "sgd_buf"),
         "adam_csghmc": ("mom", "adam_m", "adam_v")}


def owned_keys(c):
    keys = ("theta",) + OWNED[c["method"]]
    if c["momentum"] == 0:
        keys = tuple(k for k in keys if k != "sgd_buf")
    return keys


def expected_live(c, k, names):
    """The tensors with a gradient in step k, from the case alone."""
    skip = c["skip"][k % len(c["skip"])] if c["skip"] else ()
    return [i for i, nm in enumerate(names) if nm not in c["frozen"] and nm not in skip]


def build_nets(c, device):
    """(net, net0) of a case: the chain's FakeNet and its prior-mean twin."""
    segs = segments_of(c["table"])
    n = numel_of(segs)
    skip = c["skip"]
    no_grad = None if not skip else (lambda k: skip[k % len(skip)])
    net = FakeNet(segs, TOY_READOUT, grad_seed=c["grad_seed"], grad_scale=0.5,
                  init=init_vector(c["init_seed"], n, 0.5), frozen=c["frozen"],
                  no_grad=no_grad).to(device)
    net0 = FakeNet(segs, TOY_READOUT, init=init_vector(c["prior_seed"], n, 0.3),
                   frozen=c["frozen"]).to(device)
    return net, net0


# ---------------------------------------------------------- wrong streams
MISALIGNMENTS = (
    "reversed",            # the step's draws made in the reverse tensor order
    "explore_skipped",     # cSGHMC: no draw in explore steps
    "draw_without_grad",   # a draw for every tensor, with a gradient or not
    "clip_first",          # csgld: the raw gradient clipped, the draw added after
    "eval_not_consumed",   # evaluation draws leave the training stream where it was
    "eval_trainable_only",  # evaluation draws only for parameters that require grad
)


def applicable(c, evaluation=False):
    """The misalignments that change this case's stream or update."""
    out = ["reversed"]
    if c["pattern"] is not None and not all(c["pattern"]):
        out.append("explore_skipped")
    if c["frozen"] or c["skip"]:
        out.append("draw_without_grad")
    if c["clip_grad"] is not None:
        out.append("clip_first")
    if evaluation:
        out.append("eval_not_consumed")
        if c["frozen"]:
            out.append("eval_trainable_only")
    return out


def _rng_state(device):
    dev = torch.device(device)
    return torch.cuda.get_rng_state(dev) if dev.type == "cuda" else torch.get_rng_state()


def _set_rng_state(state, device):
    dev = torch.device(device)
    if dev.type == "cuda":
        torch.cuda.set_rng_state(state, dev)
    else:
        torch.set_rng_state(state)


# ------------------------------------------------------------------ chain
class RefChain:
    """One reference chain.  `step()` is one training step, `draw()` one
    evaluation draw; both consume torch's global generator on `device`, seeded
    with the case's noise_seed when the chain is built."""

    def __init__(self, c, device, misalign=None):
        if misalign is not None and misalign not in MISALIGNMENTS:
            raise ValueError(f"misalign must be one of {MISALIGNMENTS}")
        self.c, self.device, self.misalign = c, device, misalign
        self.net, self.net0 = build_nets(c, device)
        self.names = [nm for nm, _ in self.net.named_parameters()]
        self.params = list(self.net.parameters())
        self.params0 = list(self.net0.parameters())
        self.crit = torch.nn.CrossEntropyLoss()
        (self.x, self.y), = fake_loader(1, device=device)
        zeros = lambda: [torch.zeros_like(p) for p in self.params]  # noqa: E731
        self.mom, self.adam_m, self.adam_v = zeros(), zeros(), zeros()
        self.sgd_buf = [None] * len(self.params)
        self.t = 0           # Adam's step counter
        self.k = 0           # training steps done
        self.live = []       # per step: indices of the tensors with a gradient
        self.draws = []      # per step: {tensor index: its randn_like draw}
        self.clip_norms = []  # per clipped step: total norm of the sampler gradient
        self.eval_draws = []  # per evaluation draw: the per-parameter draws, all parameters
        torch.manual_seed(c["noise_seed"])

    # ---------------------------------------------------------- training
    def _draw(self, live, should_sample):
        p = self.params
        if self.misalign == "explore_skipped" and not should_sample:
            return {i: torch.zeros_like(p[i]) for i in live}
        if self.misalign == "draw_without_grad":
            every = [torch.randn_like(q) for q in p]
            return {i: every[i] for i in live}
        if self.misalign == "reversed":
            return {i: torch.randn_like(p[i]) for i in reversed(live)}
        return {i: torch.randn_like(p[i]) for i in live}

    def step(self):
        c, k = self.c, self.k
        ss = True if c["pattern"] is None else bool(c["pattern"][k])
        out = self.net(self.x)
        loss = self.crit(out, self.y)
        self.net.zero_grad()
        loss.backward()
        live = [i for i, p in enumerate(self.params) if p.grad is not None]
        pick = lambda seq: [seq[i] for i in live]  # noqa: E731
        P, P0, names = pick(self.params), pick(self.params0), pick(self.names)
        G = [p.grad for p in P]
        lrs = [c["lr"], c["lr_head"]]
        lr_of = [c["lr_head"] if TOY_READOUT in nm else c["lr"] for nm in names]
        method = c["method"]
        with torch.no_grad():
            eps = self._draw(live, ss)
            E = pick(eps)
            newg, mu = None, 0.0
            if method in ("csghmc", "csghmc_fs"):
                new = O.csghmc_update(P, G, pick(self.mom), names, TOY_READOUT, lrs,
                                      c["prior_sig"], c["alpha"], c["N"], c["nd"], ss, E)
                self._put(self.mom, live, new)
            elif method == "sghmc":
                newg, new = O.sghmc_model(P, P0, G, pick(self.mom), names, TOY_READOUT, lrs,
                                          c["prior_sig"], c["bias"], c["alpha"], c["N"], c["nd"], E)
                self._put(self.mom, live, new)
            elif method in ("sgld", "csgld"):
                clip = c["clip_grad"]
                if clip is not None and self.misalign == "clip_first":
                    O.clip_grad_norm(G, clip)
                newg = O.sgld_model(P, P0, G, names, TOY_READOUT, lrs, c["prior_sig"], c["bias"],
                                    c["N"], c["nd"], E)
                if clip is not None and self.misalign != "clip_first":
                    self.clip_norms.append(float(O.clip_grad_norm(newg, clip)))
                mu = c["momentum"]
            elif method in ("adam_sghmc", "adam_csghmc"):
                self.t += 1
                cyc = method == "adam_csghmc"
                newg, vm, m, v = O.adam_sghmc_model(
                    P, P0, G, pick(self.mom), pick(self.adam_m), pick(self.adam_v), names,
                    TOY_READOUT, lrs, c["prior_sig"], c["bias"], c["alpha"], c["beta1"],
                    c["beta2"], c["epsilon"], self.t, c["N"], c["nd"], E,
                    temperature=c["temperature"] if cyc else 1.0, grad_is_mom=cyc)
                self._put(self.mom, live, vm)
                self._put(self.adam_m, live, m)
                self._put(self.adam_v, live, v)
                mu = 0.0 if cyc else c["momentum"]  # adam_csghmc.py:70 forces momentum 0
            else:
                raise ValueError(f"unknown method {method!r}")
            if newg is not None:
                bufs = O.sgd_step(P, newg, pick(self.sgd_buf), lr_of, mu)
                self._put(self.sgd_buf, live, bufs)
        self.live.append(live)
        self.draws.append(eps)
        self.k += 1

    @staticmethod
    def _put(dst, live, new):
        for i, t in zip(live, new):
            dst[i] = t

    def run(self, steps=None):
        for _ in range(self.c["steps"] if steps is None else steps):
            self.step()
        return self

    # -------------------------------------------------------- evaluation
    def draw(self, mean, kind, m2=None, count=None):
        """One posterior sample mean + sqrt(var) * eps as a flat tensor.  kind:
        "raw" (m2 the second raw moment, `count` samples: methods/sgld.py:337-345),
        "welford" (m2 the sum of squared deviations of `count` samples:
        methods/csghmc.py:451-459) or "none" (no second moment: variance 1e-12)."""
        saved = _rng_state(self.device) if self.misalign == "eval_not_consumed" else None
        if self.misalign == "eval_trainable_only":
            eps = [torch.randn_like(p) if p.requires_grad else torch.zeros_like(p)
                   for p in self.params]
        else:
            eps = [torch.randn_like(p) for p in self.params]  # frozen parameters included
        if saved is not None:
            _set_rng_state(saved, self.device)
        if kind == "raw":
            var = O.posterior_variance_raw(mean, m2, count)
        elif kind == "welford":
            var = O.posterior_variance_welford(m2, count, mean)
        elif kind == "none":
            var = O.posterior_variance_welford(None, 1, mean)
        else:
            raise ValueError(f"unknown variance source {kind!r}")
        flat = torch.cat([e.reshape(-1) for e in eps])
        self.eval_draws.append(flat)
        return O.posterior_sample(mean, var, flat)

    # ------------------------------------------------------------- state
    def state(self):
        """theta and every buffer as flat fp32 numpy vectors (a tensor that
        never had an SGD buffer counts as zeros)."""
        cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()  # noqa: E731
        bufs = [torch.zeros_like(p) if b is None else b for p, b in zip(self.params, self.sgd_buf)]
        return {"theta": cat(self.params), "mom": cat(self.mom), "adam_m": cat(self.adam_m),
                "adam_v": cat(self.adam_v), "sgd_buf": cat(bufs)}


def reference_chain(c, device, misalign=None):
    """The finished chain of a case."""
    return RefChain(c, device, misalign).run()


# ------------------------------------------------------ evaluation moments
EVAL_KINDS = ("raw", "welford", "none")
EVAL_COUNT = 5   # samples behind the moments
EVAL_NST = 3     # successive draws


def eval_moments(n, kind, device):
    """(mean, m2) for an n-element draw: a mean of O(0.5) and a variance of
    O(0.05 .. 0.3), so that the noise term is a visible share of the sample."""
    mean = torch.from_numpy(init_vector(11, n, 0.5)).to(device)
    var = torch.from_numpy(np.abs(init_vector(12, n, 0.3)) + np.float32(0.05)).to(device)
    if kind == "raw":
        return mean, mean ** 2 + var * ((EVAL_COUNT - 1) / EVAL_COUNT)
    if kind == "welford":
        return mean, var * (EVAL_COUNT - 1)
    return mean, None


# train - evaluate - train on one seed: the steps before, the draws, the steps after
EVAL_SCHEDULE = (3, 2, 3)
EVAL_CASES = {
    "csghmc": case("csghmc", pattern=INTERLEAVED, frozen=("layer1.weight",)),
    "sgld_mom": case("sgld", momentum=0.5, frozen=("layer1.weight",)),
    "adam_sghmc_mom": case("adam_sghmc", momentum=0.5, frozen=("layer1.weight",)),
}


def reference_train_eval_train(c, device, kind="raw", misalign=None):
    """EVAL_SCHEDULE on one seed: returns (chain, [samples])."""
    ch = RefChain(c, device, misalign)
    before, ndraws, after = EVAL_SCHEDULE
    ch.run(before)
    n = sum(p.numel() for p in ch.params)
    mean, m2 = eval_moments(n, kind, device)
    samples = [ch.draw(mean, kind, m2, EVAL_COUNT) for _ in range(ndraws)]
    ch.run(after)
    return ch, samples
