"""bayesdll_amd.run --temperature_scale: the parser's refusals (no device) and
one stacked run that logs the reference's two calibration lines."""
import numpy as np
import pytest


def test_run_cli_temperature_scale_needs_stacked_chains_and_a_validation_split(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    assert not ap.parse_args([]).temperature_scale
    a = ap.parse_args(["--stacked_chains", "4", "--temperature_scale"])
    assert run.check_temperature_scale(ap, a) is True and a.val_heldout > 0
    with pytest.raises(SystemExit) as e:
        run.main(["--temperature_scale"])
    assert e.value.code == 2 and "it needs --stacked_chains >= 1" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run.main(["--method", "sgld", "--stacked_chains", "4", "--temperature_scale",
                  "--val_heldout", "0"])
    assert e.value.code == 2 and "it needs --val_heldout > 0" in capsys.readouterr().err


class _StubSampler:
    """What report_temperature_scale asks of a stacked sampler, with canned
    answers (and a record of the calls)."""

    def __init__(self, K, per_chain, fit, unc):
        self.K, self.per_chain, self.chain0 = K, per_chain, 5
        self._fit, self._unc, self.calls = fit, unc, []

    def fit_temperature(self, loader, *, by_chain=False):
        self.calls.append(("fit", loader, by_chain))
        return self._fit

    def uncertainty(self, loader, *, by_chain=False, temperature=None):
        self.calls.append(("uncertainty", loader, by_chain, temperature))
        return self._unc


def _canned(temperature, converged, at_bound=False, degenerate=False):
    fit = {"temperature": temperature, "nll_before": 2.5, "nll_after": 2.25, "iterations": 4,
           "converged": converged, "at_bound": at_bound, "degenerate": degenerate, "n": 64,
           "n_nonfinite": 0, "n_inf_label": 0}
    unc = {"n": 64, "nll": 2.45531, "error": 0.9, "ece": 0.05604, "mce": 0.12949, "entropy": 2.2,
           "members": 8, "num_bins": 15,
           "scaled": {"temperature": temperature, "nll": 2.35194, "ece": 0.02706, "mce": 0.02841,
                      "entropy": 2.29, "confidence": 0.13}}
    return fit, unc


def test_report_logs_both_lines_for_a_converged_fit():
    from bayesdll_amd import run
    fit, unc = _canned(2.01099, True)
    S, rec, lines = _StubSampler(4, None, fit, unc), {"epoch": 1}, []
    out = run.report_temperature_scale(S, "VAL", "TEST", rec, lines.append)
    assert S.calls == [("fit", "VAL", False), ("uncertainty", "TEST", False, "fitted")]
    assert lines == ["[Calibration - No temp scaling] ECE = 0.0560, MCE = 0.1295, NLL = 2.4553",
                     "[Calibration - Temp-scaled Topt=2.0110] ECE = 0.0271, MCE = 0.0284, "
                     "NLL = 2.3519"]
    assert out is rec["calibration"] and rec["epoch"] == 1
    assert rec["calibration"] == {"fit": fit, "T1": {"ece": 0.05604, "mce": 0.12949, "nll": 2.45531},
                                  "Topt": unc["scaled"]}


@pytest.mark.parametrize("flags", [dict(at_bound=True), dict(degenerate=True), dict()],
                         ids=["at_bound", "degenerate", "unconverged"])
def test_report_logs_the_failure_line_and_no_scaled_line(flags):
    from bayesdll_amd import run
    fit, unc = _canned(100.0, False, **flags)
    S, rec, lines = _StubSampler(4, None, fit, unc), {}, []
    run.report_temperature_scale(S, "VAL", "TEST", rec, lines.append)
    assert lines == ["[Calibration - No temp scaling] ECE = 0.0560, MCE = 0.1295, NLL = 2.4553",
                     "!! Temperature scaling optimization failed !!"]
    assert rec["calibration"]["fit"] is fit and rec["calibration"]["Topt"] is unc["scaled"]


def test_report_logs_one_pair_per_chain_under_a_sweep():
    """K = 2 under per_chain: every value a list of 2; chain 5 converged, chain 6 on a limit."""
    from bayesdll_amd import run
    fit = {"temperature": [1.5, 100.0], "nll_before": [2.5, 2.6], "nll_after": [2.25, 2.4],
           "iterations": [4, 4], "converged": [True, False], "at_bound": [False, True],
           "degenerate": [False, False], "n": [64, 64], "n_nonfinite": [0, 0], "n_inf_label": [0, 0]}
    unc = {"n": [64, 64], "nll": [2.4, 2.5], "error": [0.9, 0.8], "ece": [0.05, 0.06],
           "mce": [0.125, 0.25], "members": 4, "num_bins": 15,
           "scaled": {"temperature": [1.5, 100.0], "nll": [2.3, 2.35], "ece": [0.02, 0.03],
                      "mce": [0.0625, 0.5], "entropy": [2.2, 2.3], "confidence": [0.2, 0.1]}}
    S, rec, lines = _StubSampler(2, {"lr": [1e-2, 2e-2]}, fit, unc), {}, []
    run.report_temperature_scale(S, "VAL", "TEST", rec, lines.append)
    assert S.calls == [("fit", "VAL", True), ("uncertainty", "TEST", True, "fitted")]
    assert lines == [
        "[Calibration - No temp scaling] chain 5 ECE = 0.0500, MCE = 0.1250, NLL = 2.4000",
        "[Calibration - Temp-scaled Topt=1.5000] chain 5 ECE = 0.0200, MCE = 0.0625, NLL = 2.3000",
        "[Calibration - No temp scaling] chain 6 ECE = 0.0600, MCE = 0.2500, NLL = 2.5000",
        "!! Temperature scaling optimization failed !! chain 6"]
    assert rec["calibration"] == {"fit": fit, "T1": {"ece": [0.05, 0.06], "mce": [0.125, 0.25],
                                                     "nll": [2.4, 2.5]}, "Topt": unc["scaled"]}


@pytest.mark.gpu
def test_cli_stacked_sgld_logs_the_two_calibration_lines(tmp_path):
    from bayesdll_amd.run import main
    argv = ["--method", "sgld", "--dataset", "mnist", "--backbone", "mlp_mnist", "--epochs", "2",
            "--batch_size", "64", "--lr", "1e-2", "--train_size", "256", "--test_size", "64",
            "--val_heldout", "0.25", "--stacked_chains", "4", "--ece_num_bins", "10",
            "--hparams", "prior_sig=1.0,Ninflate=1.0,nd=1.0,burnin=0,thin=1,nst=2,bias=informative,temp=1.0",
            "--temperature_scale", "--log_dir", str(tmp_path / "t")]
    hist = main(argv)
    assert len(hist) == 2 and "calibration" not in hist[0]
    c = hist[-1]["calibration"]
    assert set(c) == {"fit", "T1", "Topt"} and set(c["T1"]) == {"ece", "mce", "nll"}
    assert set(c["Topt"]) == {"temperature", "nll", "ece", "mce", "entropy", "confidence"}
    assert c["fit"]["n"] == 64 and c["fit"]["n_nonfinite"] == 0       # 0.25 x 256 validation examples
    assert c["Topt"]["temperature"] == c["fit"]["temperature"]
    assert c["fit"]["nll_after"] <= c["fit"]["nll_before"]
    # the synthetic labels are independent of the inputs: whether the validation NLL has an
    # optimum inside [0.01, 100] is the draw's business, and either outcome has its line
    ok = c["fit"]["converged"]
    assert ok or c["fit"]["at_bound"] or c["fit"]["degenerate"]
    assert np.isfinite([c["T1"]["nll"], c["Topt"]["nll"], c["Topt"]["ece"], c["Topt"]["mce"]]).all()
    text = next((tmp_path / "t").rglob("logs.txt")).read_text().splitlines()
    plain = [ln for ln in text if "[Calibration - No temp scaling] ECE = " in ln]
    scaled = [ln for ln in text if "[Calibration - Temp-scaled Topt=" in ln]
    failed = [ln for ln in text if "!! Temperature scaling optimization failed !!" in ln]
    assert len(plain) == 1 and f"NLL = {c['T1']['nll']:.4f}" in plain[0]
    assert (len(scaled), len(failed)) == ((1, 0) if ok else (0, 1))
    last = (scaled + failed)[0]
    assert text.index(plain[0]) < text.index(last)
    if ok:
        assert f"Topt={c['Topt']['temperature']:.4f}] ECE = {c['Topt']['ece']:.4f}, MCE = " in last
        assert f"NLL = {c['Topt']['nll']:.4f}" in last
