"""Per-chain hyperparameters of stacked chains: the host side of a sweep.

K stacked chains may each carry their own lr, lr_head, prior_sig,
momentum_decay / momentum, nd and Ninflate (`per_chain={name: K values}` on
StackedCSGHMC / StackedSGLD / StackedCSGLD).  This module holds what needs no
device: the validation of such a table and its expansion into the scalar rows
the per-chain launch reads (include/bdl_chain_step.h bdl_chain_scalars, 12
floats per chain).

Chain k's row is the expressions of the uniform samplers' update(), evaluated
in float64 with chain k's values and rounded once to fp32 (np.float32 rounds
to nearest even, as a ctypes c_float field does), so it equals the scalars a
one-chain sampler built with chain k's values hands to bdl_sgmcmc_step.  The
structure of a run (epochs, num_cycles, proportion_exploration, thin, nst,
burnin, bias) stays shared: all chains explore, sample and collect on the same
steps.
"""
from __future__ import annotations

import numpy as np

from .cyclical import CyclicalSGMCMC

# what each sampler family sweeps
NAMES = {
    "csghmc": ("lr", "lr_head", "prior_sig", "momentum_decay", "nd", "Ninflate"),
    "sgld": ("lr", "lr_head", "prior_sig", "nd", "Ninflate", "momentum"),
}
COLUMNS = 12  # floats per row (bdl_chain_scalars)


def defaults(args, family):
    """The shared value of every sweepable name, from the sampler's args."""
    hp = args.hparams
    d = {"lr": float(args.lr), "lr_head": float(args.lr_head),
         "prior_sig": float(hp["prior_sig"]), "nd": float(hp["nd"]),
         "Ninflate": float(hp["Ninflate"])}
    if family == "csghmc":
        d["momentum_decay"] = float(hp["momentum_decay"])
    else:
        d["momentum"] = float(getattr(args, "momentum", 0.0))
    return d


def parse(per_chain, K, family, shared):
    """Validate `per_chain` ({name: K values}) for a sampler family and return
    {name: float64 [K]} over ALL of the family's names (`shared` fills the
    names not swept).  Refuses an unknown name, a wrong length, a non-finite
    value and a `momentum` column mixing zero and non-zero values (SGD
    momentum is one flag of the launch)."""
    if family not in NAMES:
        raise ValueError(f"per_chain: no per-chain launch for {family!r}")
    K = int(K)
    tab = {}
    for nm, vals in dict(per_chain).items():
        if nm not in NAMES[family]:
            raise ValueError(f"per_chain: unknown name {nm!r}; {family} chains sweep "
                             + ", ".join(NAMES[family]))
        v = np.asarray(list(vals) if not np.isscalar(vals) else [vals], dtype=np.float64).reshape(-1)
        if v.size != K:
            raise ValueError(f"per_chain: {nm!r} has {v.size} values for {K} chains (wrong length)")
        if not np.isfinite(v).all():
            raise ValueError(f"per_chain: {nm!r} holds a non-finite value")
        tab[nm] = v
    for nm in NAMES[family]:
        tab.setdefault(nm, np.full(K, float(shared[nm]), dtype=np.float64))
    for nm in ("lr", "lr_head"):
        if not (tab[nm] > 0).all():
            raise ValueError(f"per_chain: {nm!r} must be > 0 for every chain")
    if family == "sgld":
        nz = tab["momentum"] != 0
        if nz.any() and not nz.all():
            raise ValueError("per_chain: 'momentum' mixes zero and non-zero values; SGD momentum "
                             "is one flag of the launch, so it is on for all chains or for none")
    return tab


def table_for_state(tab):
    """The table as plain lists (what state_dict stores and load_ckpt compares)."""
    return {nm: [float(x) for x in v] for nm, v in sorted(tab.items())}


def _finish(r):
    with np.errstate(over="ignore"):
        return r.astype(np.float32)


def csghmc_rows(tab, lr, ND):
    """[K, 12] fp32 rows of one cSGHMC step; lr: the step's body lr per chain
    (float64 [K]).  StackedCSGHMC.update's expressions per chain:
    lrs = (lr, lr * (lr_head / lr_base)), N = ND * Ninflate,
    ns = nd * sqrt(2 * momentum_decay * lr) / N, 1 - momentum_decay, prior_sig;
    sigma2, n_data = 1 and mu = 0 as the uniform launch leaves them."""
    # lr may carry leading axes ([batches, K]): float64 numpy arithmetic is the
    # IEEE arithmetic of the Python floats update() uses, element for element
    l0 = np.asarray(lr, dtype=np.float64)
    K = l0.shape[-1]
    ratio = np.asarray([float(tab["lr_head"][k]) / float(tab["lr"][k]) for k in range(K)])
    N = np.asarray([ND * float(tab["Ninflate"][k]) for k in range(K)])
    md, nd = tab["momentum_decay"], tab["nd"]
    l1 = l0 * ratio
    r = np.zeros(l0.shape + (COLUMNS,), dtype=np.float64)
    r[..., 0], r[..., 1] = l0, l1
    r[..., 2] = nd * np.sqrt(2 * md * l0) / N
    r[..., 3] = nd * np.sqrt(2 * md * l1) / N
    r[..., 4] = 1 - md
    r[..., 5] = tab["prior_sig"]
    r[..., 6] = r[..., 7] = r[..., 9] = r[..., 10] = 1.0
    return _finish(r)


def sgld_rows(tab, lr, lr_head, ND):
    """[K, 12] fp32 rows of one SGLD / cSGLD step; lr / lr_head: the step's
    body and head lr per chain.  StackedSGLD.update's expressions per chain:
    N = ND * Ninflate, ns = nd * sqrt(2 / (N * lr)), sigma2 = prior_sig ** 2,
    n_data = N, mu = momentum, and the float64 reciprocals of both divisors."""
    l0, l1 = np.asarray(lr, dtype=np.float64), np.asarray(lr_head, dtype=np.float64)
    K = l0.shape[-1]
    N = np.asarray([ND * float(tab["Ninflate"][k]) for k in range(K)])
    s2 = np.asarray([float(tab["prior_sig"][k]) ** 2 for k in range(K)])  # Python's **, as update()
    inv = lambda s: np.asarray([1.0 / float(x) if x != 0.0 else 0.0 for x in s])  # noqa: E731
    nd = tab["nd"]
    r = np.zeros(l0.shape + (COLUMNS,), dtype=np.float64)
    r[..., 0], r[..., 1] = l0, l1
    r[..., 2] = nd * np.sqrt(2 / (N * l0))
    r[..., 3] = nd * np.sqrt(2 / (N * l1))
    r[..., 4] = 1.0
    r[..., 5], r[..., 6], r[..., 7] = tab["prior_sig"], s2, N
    r[..., 8] = tab["momentum"]
    r[..., 9], r[..., 10] = inv(s2), inv(N)
    return _finish(r)


def schedules(tab, epochs, num_cycles, proportion_exploration):
    """Chain k's own CyclicalSGMCMC(base_lr=lr_k, ...): the step's lr of chain
    k is what a one-chain cyclical sampler built with lr_k computes."""
    return [CyclicalSGMCMC(base_lr=float(b), nbr_of_cycles=num_cycles, epochs=epochs,
                           proportion_exploration=proportion_exploration) for b in tab["lr"]]


def cyclical_lrs(scheds, epoch, batch, batches_per_epoch):
    """float64 [K]: every chain's body lr at one step."""
    return np.asarray([s.calculate_lr(epoch=epoch, batch=batch,
                                      batches_per_epoch=batches_per_epoch) for s in scheds],
                      dtype=np.float64)


def head_lrs(tab, lr):
    """The head group's lr of a cyclical step: lr * (lr_head / lr_base) per chain."""
    lr = np.asarray(lr, dtype=np.float64)
    ratio = np.asarray([float(tab["lr_head"][k]) / float(tab["lr"][k])
                        for k in range(lr.shape[-1])])
    return lr * ratio


def describe(tab, swept, k):
    """'lr=0.01 prior_sig=1' for chain k over the swept names (log lines)."""
    return " ".join(f"{nm}={tab[nm][k]:g}" for nm in swept)
