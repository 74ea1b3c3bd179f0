"""Command-line driver for the fused SG-MCMC samplers with the reference's flag
and hparams surface (demo_mnist.py / demo_vision.py: --method, --hparams
"k=v,k=v", --epochs, --batch_size, --lr, --lr_head, --momentum, --num_cycles,
--proportion_exploration, --val_heldout, --seed, --log_dir, ...).

    python -m bayesdll_amd.run --method sgld --dataset mnist --backbone mlp_mnist \
        --hparams prior_sig=1.0,Ninflate=1e3,nd=1.0,burnin=5,thin=10,bias=informative,nst=5 \
        --lr 1e-2 --momentum 0.5
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m bayesdll_amd.run --method csghmc --dataset pets --backbone vit_l_32 ...

Differences, all forced by the environment rather than chosen: the datasets
are synthetic tensors of the real datasets' shapes and split sizes (there is
no network for downloads, datasets.py:26-43); --pretrained takes a local
state_dict file loaded with weights_only=True (no URL fetch,
networks/__init__.py:66-130); wandb is not available.  Only the SG-MCMC
methods exist here (the VI / MC-dropout / Laplace / vanilla families are not
part of this framework).  With several processes (torch.distributed.run),
each rank samples its own chain (seed + rank) and evaluation averages the
posterior predictive across chains.
"""
from __future__ import annotations

import argparse
import importlib
import logging
import os
import sys
from datetime import datetime

import numpy as np
import torch

METHODS = ("sgld", "csgld", "sghmc", "csghmc", "csghmc_fs", "adam_sghmc", "adam_csghmc")

# (input shape, classes, train-set size, test-set size) of the reference's datasets
DATASETS = {
    "mnist": ((1, 28, 28), 10, 60000, 10000),
    "pets": ((3, 224, 224), 37, 3680, 3669),
    "imagenet": ((3, 224, 224), 1000, 1281167, 50000),
    "cifar100": ((3, 32, 32), 100, 50000, 10000),
    "cifar10": ((3, 32, 32), 10, 50000, 10000),
}


# pretrain_resnet101.py:122-134 defaults, used when --hparams is empty
DEFAULT_HPARAMS = {
    "csgld": "prior_sig=1.0,Ninflate=1.0,nd=0.01,burnin=50,thin=10,bias=informative,nst=5,temp=1.0",
    "sgld": "prior_sig=1.0,Ninflate=1e3,nd=1.0,burnin=50,thin=10,bias=informative,nst=5,temp=1.0",
    "csghmc": "prior_sig=1.0,Ninflate=1.0,nd=0.01,burnin=50,momentum_decay=0.18,thin=10,"
              "bias=informative,nst=5,temp=1.0",
    "sghmc": "prior_sig=1.0,Ninflate=1e3,nd=1.0,burnin=5,momentum_decay=0.18,thin=1,"
             "bias=informative,nst=5,temp=1.0",
    "adam_sghmc": "prior_sig=1.0,Ninflate=1e3,nd=1.0,momentum_decay=0.05,burnin=50,thin=10,"
                  "bias=informative,nst=5,temp=1.0,beta1=0.9,beta2=0.999",
}
DEFAULT_HPARAMS["csghmc_fs"] = DEFAULT_HPARAMS["csghmc"]
DEFAULT_HPARAMS["adam_csghmc"] = DEFAULT_HPARAMS["adam_sghmc"]


def parse_hparams(s):
    """demo_mnist.py:77-86: strip quotes, split on ',', keep 'k=v' items, values
    stay strings; also returns the directory tag (',' -> '_')."""
    s = s.replace('"', "")
    tag = s.replace(",", "_")
    out = {}
    for opt in s.split(","):
        if "=" in opt:
            k, v = opt.split("=")
            out[k] = v
    return out, tag


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--method", type=str, default="csghmc", choices=METHODS)
    ap.add_argument("--hparams", type=str, default="")
    ap.add_argument("--pretrained", type=str, default=None,
                    help="local state_dict file of the backbone (prior mean net0)")
    ap.add_argument("--dataset", type=str, default="mnist", choices=sorted(DATASETS))
    ap.add_argument("--backbone", type=str, default="mlp_mnist",
                    choices=["mlp_mnist", "resnet101", "vit_l_32"])
    ap.add_argument("--val_heldout", type=float, default=0.1)
    ap.add_argument("--ece_num_bins", type=int, default=15)
    ap.add_argument("--num_cycles", type=int, default=1)
    ap.add_argument("--proportion_exploration", type=float, default=0.5)
    ap.add_argument("--full_sample", type=bool, default=False)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--lr_head", type=float, default=None)
    ap.add_argument("--momentum", type=float, default=0.5)
    ap.add_argument("--clip_grad", type=float, default=None)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--log_dir", type=str, default="results")
    ap.add_argument("--test_eval_freq", type=int, default=1)
    # synthetic data (the reference downloads the real sets)
    ap.add_argument("--train_size", type=int, default=None,
                    help="synthetic training examples (default: the dataset's size)")
    ap.add_argument("--test_size", type=int, default=None)
    # MI355X path options
    ap.add_argument("--noise_mode", type=str, default="philox", choices=["philox", "torch"])
    ap.add_argument("--graph", action="store_true", help="replay forward/backward from a HIP graph")
    ap.add_argument("--overlap", action="store_true",
                    help="overlap the fused update with backward, bucket by bucket (cSGHMC)")
    ap.add_argument("--compute_dtype", type=str, default=None, choices=["fp32", "bf16"],
                    help="fp32 (the default, unless BDL_COMPUTE_DTYPE=bf16 is set) or bf16: the "
                         "network computes in bf16 over an fp32 chain state (csghmc, csghmc_fs, "
                         "sghmc, sgld, unclipped csgld; not with --stacked_chains)")
    ap.add_argument("--resume_state", action="store_true",
                    help="checkpoints carry what an exact resume needs")
    ap.add_argument("--stacked_chains", type=int, default=0,
                    help="csghmc / sghmc / sgld / csgld / adam_sghmc / adam_csghmc: K > 0 chains "
                         "per device stepped together (bayesdll_amd.stacked; no BatchNorm "
                         "statistics; csgld and adam_csghmc honour --clip_grad per chain)")
    ap.add_argument("--rhat", action="store_true",
                    help="with --stacked_chains >= 2: log the cross-chain R-hat of the collected "
                         "moments at every evaluation (stacked diagnostics())")
    ap.add_argument("--sweep", action="append", default=[], metavar="NAME=v1,...,vK",
                    help="with --stacked_chains K (csghmc, sgld, csgld): chain k runs with the "
                         "k-th value of NAME (lr, lr_head, prior_sig, nd, Ninflate, and "
                         "momentum_decay or momentum); one value is broadcast; repeatable. "
                         "Every chain is scored on its own at each evaluation")
    ap.add_argument("--health", type=int, default=0, metavar="M",
                    help="with --stacked_chains >= 1: every M-th step, accumulate the per-chain, "
                         "per-tensor statistics between backward and update (one fused sweep) "
                         "and log every chain's health after each epoch: kinetic and "
                         "configurational temperature and the hottest tensor (csghmc), the "
                         "largest gradient rms otherwise; works with --sweep")
    ap.add_argument("--ess", type=int, default=0, metavar="B",
                    help="with --stacked_chains >= 1: fold every collected sample into "
                         "batch-means accumulators (batches of B samples) and log the effective "
                         "sample size of the latest component at every evaluation (stacked "
                         "ess()); per chain with --sweep")
    ap.add_argument("--by_tensor", type=int, default=0, metavar="N",
                    help="with --rhat and / or --ess: after their log line, also log the N "
                         "tensors with the largest R-hat maximum and the N with the smallest "
                         "ESS minimum (one fused per-tensor sweep each, by_tensor=True), and "
                         "keep the whole per-tensor table in the epoch record")
    ap.add_argument("--uncertainty", action="store_true",
                    help="with --stacked_chains >= 1: at every evaluation, log the stacked "
                         "predictive's NLL, error, ECE / MCE (--ece_num_bins), total and expected "
                         "entropy, mutual information (overall, on wrong against other examples) "
                         "and member disagreement from one fused sweep over the members' logits "
                         "(stacked uncertainty()); per chain with --sweep")
    ap.add_argument("--detect", action="store_true",
                    help="with --stacked_chains >= 1: at every evaluation, log how the "
                         "predictive's uncertainty scores (entropy, mutual information, expected "
                         "entropy, -confidence, disagreement) rank the misclassified test "
                         "examples: exact AUROC, average precision and FPR at 95 %% TPR from an "
                         "all-pairs count on the device (stacked detection()); per chain with "
                         "--sweep")
    ap.add_argument("--detect_shift", type=float, default=None, metavar="SIGMA",
                    help="with --detect: also rank a shifted copy of the test split (its inputs "
                         "plus SIGMA x standard normal noise from a generator seeded by the run's "
                         "seed; the same examples in the same order) against the test split")
    ap.add_argument("--diversity", action="store_true",
                    help="with --stacked_chains >= 2: at every evaluation, log which chains "
                         "predict the same function: the mean pairwise disagreement of the "
                         "chains' own predictives with its closest and furthest pair, the mean "
                         "total variation, symmetric KL and double fault, from one fused sweep "
                         "per batch (stacked diversity()); the K x K matrices go to the epoch "
                         "record; works with --sweep")
    ap.add_argument("--stacking", action="store_true",
                    help="with --stacked_chains >= 2 and --val_heldout > 0: at every evaluation, "
                         "fit Bayesian stacking weights of the chains' predictive distributions "
                         "on the validation split (stacked fit_stacking(): the simplex weights "
                         "that maximise the held-out log score, fitted on the device), log them "
                         "with their optimality gap, and score the test split under them "
                         "(evaluate(..., weights=\"stacking\")); what pools a --sweep")
    ap.add_argument("--exchange", type=int, default=0, metavar="M",
                    help="with --stacked_chains >= 2, --method sgld or csgld, --momentum 0 and "
                         "--sweep nd=...: replica exchange (parallel tempering) between the "
                         "chains, whose temperatures are T_k = nd_k^2 — after every M-th step one "
                         "extra forward and three launches attempt to swap adjacent slots "
                         "(even-odd Metropolis, no host read); one log line per evaluation and "
                         "the record in the epoch record (stacked exchange())")
    ap.add_argument("--exchange_var", type=float, default=0.0, metavar="V",
                    help="with --exchange: the variance correction of noisy minibatch energies "
                         "(log acceptance -= (1/T_i - 1/T_j)^2 * V; 0: the plain Metropolis rule)")
    ap.add_argument("--gmm_weights", action="store_true",
                    help="with --stacked_chains >= 1 and a cyclical method: at every cycle end, "
                         "score max(1, nst) posterior draws of all chains on the training set "
                         "(stacked score_cycle(): one fused sweep per batch, one host read), log "
                         "every chain's GMM component weights and add the likelihood-weighted "
                         "mixture's NLL and error to the epoch record (test_gmm; per chain with "
                         "--sweep: chains_gmm)")
    ap.add_argument("--temperature_scale", action="store_true",
                    help="with --stacked_chains >= 1 and --val_heldout > 0: after training, fit a "
                         "scalar temperature to the stacked predictive on the validation split "
                         "on the device (stacked fit_temperature()) and log the test split's "
                         "ECE / MCE / NLL at T = 1 and at the fitted temperature (what the "
                         "one-chain Runners' calibration block reports, under this path's "
                         "own line for T = 1); per chain with --sweep")
    ap.add_argument("--fn_probe", type=int, default=0, metavar="P",
                    help="with --stacked_chains >= 1: fold the chains' class probabilities on "
                         "the first P test examples into batch-means accumulators at every "
                         "collect step (batches of --fn_batch samples) and log the function-space "
                         "R-hat and effective sample size at every evaluation (stacked "
                         "function_space()); ESS per chain with --sweep")
    ap.add_argument("--fn_batch", type=int, default=0, metavar="B",
                    help="with --fn_probe: the batch length of its batch-means accumulators "
                         "(>= 1; several autocorrelation times long)")
    return ap


def check_fn(ap, args):
    """--fn_probe P needs stacked chains and --fn_batch B >= 1; --fn_batch
    needs --fn_probe (ap.error otherwise)."""
    if args.fn_probe < 0 or args.fn_batch < 0:
        ap.error("--fn_probe / --fn_batch: P and B must be >= 0")
    if args.fn_probe and args.stacked_chains < 1:
        ap.error("--fn_probe folds the stacked chains' probe predictions: it needs "
                 "--stacked_chains >= 1")
    if args.fn_probe and args.fn_batch < 1:
        ap.error("--fn_probe needs --fn_batch B >= 1 (the batch length of its accumulators)")
    if args.fn_batch and not args.fn_probe:
        ap.error("--fn_batch is the batch length of --fn_probe's accumulators: it needs "
                 "--fn_probe P")
    return args.fn_probe, args.fn_batch


def first_examples(loader, n):
    """The first n inputs of a loader, as one batch."""
    xs, have = [], 0
    for x, _ in loader:
        xs.append(x)
        have += len(x)
        if have >= n:
            break
    if have < n:
        raise ValueError(f"--fn_probe {n}: the test split holds only {have} examples")
    return torch.cat(xs)[:n]


def check_uncertainty(ap, args):
    """--uncertainty needs stacked chains (ap.error otherwise)."""
    if args.uncertainty and args.stacked_chains < 1:
        ap.error("--uncertainty reports the stacked chains' predictive: it needs "
                 "--stacked_chains >= 1")
    return args.uncertainty


def check_detect(ap, args):
    """--detect needs stacked chains; --detect_shift SIGMA needs --detect and
    SIGMA > 0 (ap.error otherwise)."""
    if args.detect and args.stacked_chains < 1:
        ap.error("--detect ranks the stacked chains' uncertainty scores: it needs "
                 "--stacked_chains >= 1")
    if args.detect_shift is not None and not args.detect:
        ap.error("--detect_shift builds the shifted set of --detect: it needs --detect")
    if args.detect_shift is not None and not args.detect_shift > 0:
        ap.error("--detect_shift: SIGMA must be > 0")
    return args.detect, args.detect_shift


def check_diversity(ap, args):
    """--diversity compares stacked chains pairwise (ap.error otherwise)."""
    if args.diversity and args.stacked_chains < 2:
        ap.error("--diversity compares the stacked chains pairwise: it needs "
                 "--stacked_chains >= 2")
    return args.diversity


class ShiftedLoader:
    """The batches of `loader` with sigma x N(0, 1) noise added to the inputs,
    from a generator seeded by `seed` at every pass (the same shifted set every
    time; the same examples in the same order, the labels passed through)."""

    def __init__(self, loader, sigma, seed):
        self.loader, self.sigma, self.seed = loader, float(sigma), int(seed)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        g = None
        for x, y in self.loader:
            if g is None:
                g = torch.Generator(device=x.device).manual_seed(self.seed)
            yield x + self.sigma * torch.randn(x.shape, device=x.device, dtype=x.dtype,
                                               generator=g), y


def check_gmm_weights(ap, args):
    """--gmm_weights needs stacked chains of a cyclical method (ap.error
    otherwise)."""
    if args.gmm_weights and args.stacked_chains < 1:
        ap.error("--gmm_weights weighs the stacked chains' cycles: it needs --stacked_chains >= 1 "
                 "(a one-chain cyclical Runner always weighs its cycles)")
    if args.gmm_weights and args.method not in ("csghmc", "csgld", "adam_csghmc"):
        ap.error(f"--gmm_weights weighs the cycles of a cyclical method (csghmc, csgld, "
                 f"adam_csghmc), not {args.method}")
    return args.gmm_weights


def check_exchange(ap, args):
    """--exchange needs stacked SGLD / cSGLD chains with an nd ladder (ap.error
    otherwise; the sampler checks the ladder itself)."""
    if args.exchange_var != 0.0 and not args.exchange:
        ap.error("--exchange_var corrects the exchange rule: it needs --exchange M")
    if not args.exchange:
        return 0
    if args.exchange < 0:
        ap.error("--exchange M: M must be >= 1 (steps between exchange attempts)")
    if not args.exchange_var >= 0.0:
        ap.error("--exchange_var must be >= 0")
    if args.stacked_chains < 2:
        ap.error("--exchange swaps the stacked chains of one device: it needs "
                 "--stacked_chains >= 2")
    if args.method not in ("sgld", "csgld"):
        ap.error(f"--exchange: no temperature is derived for {args.method} (sgld or csgld)")
    if not any(item.split("=", 1)[0].strip() == "nd" for item in args.sweep):
        ap.error("--exchange needs a temperature ladder: it needs --sweep nd=v1,...,vK "
                 "(T_k = nd_k^2)")
    if args.momentum != 0 and not any(item.split("=", 1)[0].strip() == "momentum"
                                      for item in args.sweep):
        ap.error("--exchange needs --momentum 0 (with SGD momentum a chain does not sample "
                 "exp(-U / nd^2))")
    return args.exchange


def check_stacking(ap, args):
    """--stacking needs at least two stacked chains and a validation split
    (ap.error otherwise)."""
    if args.stacking and args.stacked_chains < 2:
        ap.error("--stacking weighs the stacked chains against each other: it needs "
                 "--stacked_chains >= 2")
    if args.stacking and not args.val_heldout > 0:
        ap.error("--stacking fits the weights on the validation split: it needs "
                 "--val_heldout > 0")
    return args.stacking


def check_temperature_scale(ap, args):
    """--temperature_scale needs stacked chains and a validation split
    (ap.error otherwise)."""
    if args.temperature_scale and args.stacked_chains < 1:
        ap.error("--temperature_scale fits the stacked chains' predictive: it needs "
                 "--stacked_chains >= 1")
    if args.temperature_scale and not args.val_heldout > 0:
        ap.error("--temperature_scale fits the temperature on the validation split: it needs "
                 "--val_heldout > 0")
    return args.temperature_scale


def report_temperature_scale(S, val_loader, test_loader, rec, log):
    """What the reference Runners' calibration block reports, for the stacked
    predictive: the test split's ECE / MCE / NLL at T = 1 (this path's own
    line, `[Calibration - No temp scaling]`; the Runners print `[Calibration -
    Default T=1]`), then at the temperature fitted on the validation split
    (the reference's `Temp-scaled` line, or its failure line), one pair per
    chain under a per_chain sweep, and both in rec["calibration"]."""
    by_chain = S.per_chain is not None
    fit = S.fit_temperature(val_loader, by_chain=by_chain)
    d = S.uncertainty(test_loader, by_chain=by_chain, temperature="fitted")
    rec["calibration"] = {"fit": fit, "T1": {k: d[k] for k in ("ece", "mce", "nll")},
                          "Topt": d["scaled"]}
    for k in range(S.K if by_chain else 1):
        f, r, s = ({key: (v[k] if by_chain else v) for key, v in m.items()}
                   for m in (fit, rec["calibration"]["T1"], d["scaled"]))
        who = f" chain {S.chain0 + k}" if by_chain else ""
        log(f"[Calibration - No temp scaling]{who} ECE = {r['ece']:.4f}, MCE = {r['mce']:.4f}, "
            f"NLL = {r['nll']:.4f}")
        if f["converged"]:
            log(f"[Calibration - Temp-scaled Topt={s['temperature']:.4f}]{who} ECE = "
                f"{s['ece']:.4f}, MCE = {s['mce']:.4f}, NLL = {s['nll']:.4f}")
        else:
            log(f"!! Temperature scaling optimization failed !!{who}")
    return rec["calibration"]


def check_by_tensor(ap, args):
    """--by_tensor N needs N >= 0 and --rhat or --ess (ap.error otherwise)."""
    if args.by_tensor < 0:
        ap.error("--by_tensor: N must be >= 0")
    if args.by_tensor and not (args.rhat or args.ess):
        ap.error("--by_tensor lists the tensors of the R-hat / ESS reports: it needs --rhat "
                 "or --ess")
    return args.by_tensor


def check_ess(ap, args):
    """--ess B needs stacked chains and B >= 0 (ap.error otherwise)."""
    if args.ess < 0:
        ap.error("--ess: B must be >= 0")
    if args.ess and args.stacked_chains < 1:
        ap.error("--ess folds the stacked chains' collected samples: it needs "
                 "--stacked_chains >= 1")
    return args.ess


def check_compute_dtype(ap, args):
    """--compute_dtype bf16 is a one-chain mode (ap.error with stacked chains)."""
    if args.compute_dtype == "bf16" and args.stacked_chains > 0:
        ap.error("--compute_dtype bf16: the stacked samplers have no bf16 step "
                 "(drop --stacked_chains)")
    return args.compute_dtype


def check_health(ap, args):
    """--health M needs stacked chains and M >= 0 (ap.error otherwise)."""
    if args.health < 0:
        ap.error("--health: M must be >= 0")
    if args.health and args.stacked_chains < 1:
        ap.error("--health reads the stacked chains' statistics sweep: it needs "
                 "--stacked_chains >= 1")
    return args.health


def parse_sweep(ap, args):
    """--sweep NAME=v1,...,vK items -> {name: K floats} (ap.error on anything
    the per-chain launch cannot run)."""
    from .per_chain import NAMES
    if not args.sweep:
        return None
    K = args.stacked_chains
    if K <= 0:
        ap.error("--sweep gives every stacked chain its own hyperparameters: it needs "
                 "--stacked_chains K > 0")
    fam = {"csghmc": "csghmc", "sgld": "sgld", "csgld": "sgld"}.get(args.method)
    if fam is None:
        ap.error(f"--sweep: {args.method} has no per-chain launch (csghmc, sgld or csgld)")
    if args.clip_grad is not None:
        ap.error("--sweep cannot be combined with --clip_grad (the clipped step has no per-chain "
                 "launch)")
    if args.rhat:
        ap.error("--sweep cannot be combined with --rhat (R-hat compares chains that target one "
                 "posterior)")
    out = {}
    for item in args.sweep:
        name, eq, vals = item.partition("=")
        if not eq or not vals:
            ap.error(f"--sweep {item!r}: expected NAME=v1,...,vK")
        if name not in NAMES[fam]:
            ap.error(f"--sweep: {args.method} does not sweep {name!r} (" + ", ".join(NAMES[fam]) + ")")
        if name in out:
            ap.error(f"--sweep: {name!r} given twice")
        try:
            v = [float(x) for x in vals.split(",")]
        except ValueError:
            ap.error(f"--sweep {item!r}: values must be numbers")
        if len(v) == 1:
            v = v * K
        if len(v) != K:
            ap.error(f"--sweep {name}: {len(v)} values for --stacked_chains {K} (length mismatch)")
        out[name] = v
    return out


class SyntheticLoader:
    """Batches of N(0,1) inputs and uniform labels of a dataset's shape,
    generated on the device from a fixed seed (the same batches every epoch,
    like iterating a fixed dataset without shuffling)."""

    def __init__(self, n, shape, classes, batch_size, device, seed):
        self.n, self.shape, self.classes, self.bs = int(n), tuple(shape), classes, batch_size
        self.device, self.seed = device, seed

    def __len__(self):
        return (self.n + self.bs - 1) // self.bs

    def __iter__(self):
        g = torch.Generator(device=self.device).manual_seed(self.seed)
        for i in range(0, self.n, self.bs):
            b = min(self.bs, self.n - i)
            x = torch.randn((b,) + self.shape, device=self.device, generator=g)
            y = torch.randint(0, self.classes, (b,), device=self.device, generator=g)
            yield x, y


def prepare(args, device):
    """datasets.prepare's split arithmetic (val_heldout carved from train)
    over synthetic tensors; returns loaders and ND = train-set size."""
    shape, classes, ntrain, ntest = DATASETS[args.dataset]
    ntrain = args.train_size if args.train_size is not None else ntrain
    ntest = args.test_size if args.test_size is not None else ntest
    nval = int(args.val_heldout * ntrain) if args.val_heldout > 0 else 0
    ntr = ntrain - nval
    args.num_classes = classes
    mk = lambda n, s: SyntheticLoader(n, shape, classes, args.batch_size, device, s)  # noqa: E731
    return mk(ntr, args.seed), (mk(nval, args.seed + 1) if nval else None), \
        mk(ntest, args.seed + 2), ntr


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.rhat and args.stacked_chains < 2:
        ap.error("--rhat compares the chains of one device: it needs --stacked_chains >= 2")
    sweep = parse_sweep(ap, args)
    check_health(ap, args)
    check_ess(ap, args)
    check_uncertainty(ap, args)
    check_detect(ap, args)
    check_diversity(ap, args)
    check_gmm_weights(ap, args)
    check_stacking(ap, args)
    check_exchange(ap, args)
    check_temperature_scale(ap, args)
    check_by_tensor(ap, args)
    check_fn(ap, args)
    check_compute_dtype(ap, args)
    from . import chains
    rank, world, device = chains.init_chains()
    if device.type != "cuda":
        raise RuntimeError("bayesdll_amd.run needs a HIP device (the samplers have no CPU path)")
    args.device = device
    seed = chains.chain_seed(args.seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    np.random.seed(seed)
    args.hparams, hpstr = parse_hparams(args.hparams or DEFAULT_HPARAMS[args.method])
    if args.lr_head is None:
        args.lr_head = args.lr
    args.seed = seed
    pretr = 1 if args.pretrained is not None else 0
    main_dir = (f"{args.dataset}_val_heldout{args.val_heldout}/{args.backbone}/"
                f"{args.method}_{hpstr}_pretr{pretr}/ep{args.epochs}_bs{args.batch_size}_"
                f"lr{args.lr}_lrh{args.lr_head}_mo{args.momentum}/seed{args.seed}_"
                + datetime.now().strftime("%Y_%m%d_%H%M%S"))
    args.log_dir = os.path.join(args.log_dir, main_dir)
    os.makedirs(args.log_dir, exist_ok=True)
    logging.basicConfig(handlers=[logging.FileHandler(os.path.join(args.log_dir, "logs.txt")),
                                  logging.StreamHandler()],
                        format="[%(asctime)s,%(msecs)03d %(levelname)s] %(message)s",
                        datefmt="%H:%M:%S", level=logging.INFO, force=True)
    logger = logging.getLogger()
    logger.info(f"Command :: {' '.join(sys.argv)}  (chain {rank} of {world})\n")

    train_loader, val_loader, test_loader, args.ND = prepare(args, device)
    if args.temperature_scale and val_loader is None:  # before any training is spent
        raise ValueError("--temperature_scale: the validation split is empty "
                         "(--val_heldout x the training set rounds to 0)")
    if args.stacking and val_loader is None:  # before any training is spent
        raise ValueError("--stacking: the validation split is empty "
                         "(--val_heldout x the training set rounds to 0)")
    from .backbones import create_backbone
    net = create_backbone(args)
    logger.info("Total params in the backbone: %.2fM"
                % (sum(p.numel() for p in net.parameters()) / 1e6))
    net0 = None
    if args.pretrained is not None:
        # feat-ext params = pretrained; net0 with a zero head, net with a random head
        state = torch.load(args.pretrained, map_location="cpu", weights_only=True)
        net0 = create_backbone(args)
        for m in (net, net0):
            own = m.state_dict()
            # networks/__init__.py:66-130: feature extractor from the file; the
            # readout stays as created (random in net, zeroed in net0 below)
            m.load_state_dict({k: v for k, v in state.items()
                               if k in own and own[k].shape == v.shape
                               and not k.startswith(m.readout_name + ".")}, strict=False)
        with torch.no_grad():
            for nm, p in net0.named_parameters():
                if net0.readout_name in nm:
                    p.zero_()
        net0 = net0.to(device)
    net = net.to(device)

    if args.stacked_chains > 0:
        from . import stacked
        cls = {"csghmc": stacked.StackedCSGHMC, "sgld": stacked.StackedSGLD,
               "csgld": stacked.StackedCSGLD, "sghmc": stacked.StackedSGHMC,
               "adam_sghmc": stacked.StackedAdamSGHMC,
               "adam_csghmc": stacked.StackedAdamCSGHMC}.get(args.method)
        if cls is None:
            raise ValueError(f"--stacked_chains: {args.method} is not stacked (csghmc, sghmc, "
                             "sgld, csgld, adam_sghmc or adam_csghmc; csghmc_fs runs one chain "
                             "per process)")
        kw = {} if sweep is None else {"per_chain": sweep}
        if args.health:
            kw["health_every"] = args.health
        if args.ess:
            kw["ess_batch"] = args.ess
        if args.exchange:
            kw["exchange_every"], kw["exchange_var"] = args.exchange, args.exchange_var
        if args.fn_probe:
            kw["fn_probe"] = first_examples(test_loader, args.fn_probe)
            kw["fn_batch"] = args.fn_batch
        S = cls(net, args.stacked_chains, args, logger=logger, init="reinit", graph=args.graph,
                net0=net0, **kw)
        if args.detect_shift is not None:
            S.detect_shifted = ShiftedLoader(test_loader, args.detect_shift, args.seed)
        if args.stacking:
            S.stacking_val = val_loader
        logger.info(f"{args.stacked_chains} stacked chains on this device "
                    f"(chain ids {S.chain0}..{S.chain0 + S.K - 1})")
        hist = S.train(train_loader, test_loader)
        if args.temperature_scale:
            if not hist:  # --epochs 0: the chains as initialised
                hist.append({})
            report_temperature_scale(S, val_loader, test_loader, hist[-1], logger.info)
        if sweep is not None:
            # rank the sweep on held-out data (the test split without one)
            from .per_chain import describe
            which, loader = ("validation", val_loader) if val_loader is not None \
                else ("test", test_loader)
            nll, err = S.evaluate_chains(loader)
            best = int(np.argmin(np.where(np.isfinite(nll), nll, np.inf)))
            logger.info(f"best chain by {which} NLL: chain {S.chain0 + best} "
                        f"({describe(S.per_chain, S.swept, best)}): loss = {nll[best]:.4f}, "
                        f"error = {err[best]:.4f}")
        return hist
    runner_cls = importlib.import_module(f"bayesdll_amd.{args.method}").Runner
    runner = runner_cls(net, net0, args, logger)
    return runner.train(train_loader, val_loader, test_loader)


if __name__ == "__main__":
    main()
