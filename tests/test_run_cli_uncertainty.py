"""bayesdll_amd.run --uncertainty: it needs stacked chains (host), and a tiny
stacked SGLD run logs the line and fills rec["uncertainty"] (GPU)."""
import numpy as np
import pytest


def test_run_cli_uncertainty_needs_stacked_chains(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    assert ap.parse_args([]).uncertainty is False
    a = ap.parse_args(["--stacked_chains", "4", "--uncertainty"])
    assert a.uncertainty is True and run.check_uncertainty(ap, a) is True
    with pytest.raises(SystemExit) as e:
        run.main(["--uncertainty"])
    assert e.value.code == 2 and "it needs --stacked_chains >= 1" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run.main(["--method", "sgld", "--uncertainty", "--stacked_chains", "0"])
    assert e.value.code == 2


def test_sampler_uncertainty_refuses_several_processes(monkeypatch):
    """Checked before anything touches the device."""
    from types import SimpleNamespace

    from bayesdll_amd import chains, stacked
    monkeypatch.setattr(chains, "world", lambda: 2)
    S = SimpleNamespace(args=SimpleNamespace())
    with pytest.raises(ValueError, match="this process's chains only"):
        stacked._StackedSampler.uncertainty(S, [])


@pytest.mark.gpu
def test_cli_stacked_sgld_logs_the_uncertainty_line(tmp_path):
    from bayesdll_amd.run import main
    argv = ["--method", "sgld", "--dataset", "mnist", "--backbone", "mlp_mnist", "--epochs", "2",
            "--batch_size", "64", "--lr", "1e-2", "--train_size", "256", "--test_size", "64",
            "--val_heldout", "0", "--stacked_chains", "3", "--ece_num_bins", "10",
            "--hparams", "prior_sig=1.0,Ninflate=1.0,nd=1.0,burnin=0,thin=1,nst=2,bias=informative,temp=1.0",
            "--log_dir"]
    hist = main(argv + [str(tmp_path / "u"), "--uncertainty"])
    assert len(hist) == 2 and all("test" in h and "uncertainty" in h for h in hist)
    u = hist[-1]["uncertainty"]
    assert u["n"] == 64 and u["num_bins"] == 10 and len(u["bins"]["count"]) == 10
    assert sum(u["bins"]["count"]) == 64 * 10 and sum(u["bins"]["hits"]) == 64
    # (its posterior draws come after evaluate()'s: the same members only in distribution)
    assert np.isfinite(u["nll"]) and 0 <= u["error"] <= 1
    assert np.isfinite([u["ece"], u["mce"], u["entropy"], u["mutual_info"]]).all()
    assert 0 <= u["disagreement"] <= 1 and u["entropy"] >= u["expected_entropy"] - 1e-6
    text = next((tmp_path / "u").rglob("logs.txt")).read_text().splitlines()
    lines = [ln for ln in text if "uncertainty over 3 chains" in ln]
    assert len(lines) == 2
    for word in ("NLL =", "error =", "ECE =", "MCE =", "(10 bins)", "entropy =", "(expected",
                 "mutual information =", "(wrong", "disagreement ="):
        assert word in lines[-1], word
    # without the flag: no line, no record, the same chains
    hist0 = main(argv + [str(tmp_path / "p")])
    assert all("uncertainty" not in h for h in hist0)
    assert not any("uncertainty" in ln for ln in
                   next((tmp_path / "p").rglob("logs.txt")).read_text().splitlines()[1:])
