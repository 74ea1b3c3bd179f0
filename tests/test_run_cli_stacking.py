"""bayesdll_amd.run --stacking: the parser's refusals (no device), the two log
lines and records of _report_stacking with a stub sampler, and one stacked run
on the device."""
import numpy as np
import pytest


def test_run_cli_stacking_needs_two_stacked_chains_and_a_validation_split(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    assert not ap.parse_args([]).stacking
    a = ap.parse_args(["--stacked_chains", "4", "--stacking"])
    assert run.check_stacking(ap, a) is True and a.val_heldout > 0
    for argv in (["--stacking"], ["--stacking", "--stacked_chains", "1"]):
        with pytest.raises(SystemExit) as e:
            run.main(argv)
        assert e.value.code == 2 and "it needs --stacked_chains >= 2" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run.main(["--method", "sgld", "--stacked_chains", "4", "--stacking", "--val_heldout", "0"])
    assert e.value.code == 2 and "it needs --val_heldout > 0" in capsys.readouterr().err


class _Stub:
    """What _report_stacking asks of a stacked sampler, with canned answers."""
    chain0, K = 5, 3

    def __init__(self, fail=None):
        self.calls, self.fail = [], fail

    def fit_stacking(self, loader):
        self.calls.append(("fit", loader))
        if self.fail:
            raise ValueError(self.fail)
        return {"weights": np.array([0.5, 0.125, 0.375]), "objective": -1.25,
                "objective_uniform": -1.5, "objective_best_single": -1.375, "best_single": 5,
                "iterations": 17, "converged": True, "gap": 7.5e-5, "n": 64, "n_label": 0,
                "n_nonfinite": 0, "n_impossible": 0}

    def evaluate(self, loader, weights=None):
        self.calls.append(("evaluate", loader, weights))
        return 1.23456, 0.25


def test_report_logs_the_two_lines_and_keeps_both_records():
    from bayesdll_amd import stacked
    S, rec, lines = _Stub(), {"epoch": 3}, []
    stacked._StackedSampler._report_stacking(S, 3, rec, "VAL", "TEST", lines.append)
    assert S.calls == [("fit", "VAL"), ("evaluate", "TEST", "stacking")]
    assert lines == ["(Epoch 3) stacking weights: {5: 0.5, 6: 0.125, 7: 0.375} (gap = 7.50e-05, "
                     "iterations = 17, converged = True)",
                     "(Epoch 3) stacked predictive, stacking weights: loss = 1.2346, "
                     "error = 0.2500"]
    assert rec["stacking"]["weights"] == [0.5, 0.125, 0.375] and rec["stacking"]["n"] == 64
    assert rec["test_stacking"] == (1.23456, 0.25) and rec["epoch"] == 3
    # without a test loader: the weights line only
    S, rec, lines = _Stub(), {}, []
    stacked._StackedSampler._report_stacking(S, 0, rec, "VAL", None, lines.append)
    assert len(lines) == 1 and "test_stacking" not in rec and "stacking" in rec
    # a refused fit is logged, not raised
    S, rec, lines = _Stub(fail="fit_stacking: the loader is empty"), {}, []
    stacked._StackedSampler._report_stacking(S, 1, rec, "VAL", "TEST", lines.append)
    assert lines == ["(Epoch 1) stacking weights: fit_stacking: the loader is empty"] and not rec


@pytest.mark.gpu
def test_cli_stacked_sweep_logs_the_stacking_lines(tmp_path):
    from bayesdll_amd.run import main
    argv = ["--method", "sgld", "--dataset", "mnist", "--backbone", "mlp_mnist", "--epochs", "2",
            "--batch_size", "64", "--lr", "1e-2", "--train_size", "256", "--test_size", "64",
            "--val_heldout", "0.25", "--stacked_chains", "3",
            "--hparams", "prior_sig=1.0,Ninflate=1.0,nd=1.0,burnin=0,thin=1,nst=0,bias=informative,temp=1.0",
            "--stacking", "--log_dir", str(tmp_path / "s")]
    hist = main(argv)
    assert len(hist) == 2 and all("stacking" in h and "test_stacking" in h for h in hist)
    d = hist[-1]["stacking"]
    assert d["n"] == 64 and len(d["weights"]) == 3 and abs(sum(d["weights"]) - 1) < 1e-12
    assert d["objective"] >= d["objective_uniform"] and d["gap"] >= 0
    text = next((tmp_path / "s").rglob("logs.txt")).read_text().splitlines()
    wl = [ln for ln in text if ") stacking weights: {" in ln]
    pl = [ln for ln in text if "stacked predictive, stacking weights: loss = " in ln]
    assert len(wl) == 2 and len(pl) == 2 and "converged = " in wl[-1] and "gap = " in wl[-1]
    assert f"loss = {hist[-1]['test_stacking'][0]:.4f}" in pl[-1]
    hist0 = main(argv[:-3] + ["--log_dir", str(tmp_path / "p")])
    assert all("stacking" not in h for h in hist0)
