"""bayesdll_amd.run --diversity: a tiny stacked SGLD run logs one [Diversity]
line at every evaluation and keeps the matrices in rec["diversity"] as lists
(GPU); without --stacked_chains the flag is refused by name."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ARGV = ["--method", "sgld", "--dataset", "mnist", "--backbone", "mlp_mnist", "--epochs", "2",
        "--batch_size", "64", "--lr", "1e-2", "--train_size", "256", "--test_size", "96",
        "--val_heldout", "0",
        "--hparams", "prior_sig=1.0,Ninflate=1.0,nd=1.0,burnin=0,thin=1,nst=2,bias=informative,temp=1.0",
        "--log_dir"]
MATRICES = ("disagreement", "tv", "kl", "sym_kl", "kl_unbounded", "double_fault",
            "error_correlation")


def _lines(path, word):
    return [ln for ln in next(path.rglob("logs.txt")).read_text().splitlines()[1:] if word in ln]


def test_cli_stacked_sgld_logs_the_diversity_line_and_keeps_the_matrices(tmp_path):
    from bayesdll_amd.run import main
    hist = main(ARGV + [str(tmp_path / "d"), "--stacked_chains", "3", "--diversity"])
    assert len(hist) == 2 and all("test" in h and "diversity" in h for h in hist)
    d = hist[-1]["diversity"]
    assert sorted(d) == sorted(MATRICES + ("error", "n", "n_labelled", "n_nonfinite", "summary"))
    assert (d["n"], d["n_labelled"], d["n_nonfinite"]) == (96, 96, 0)
    for k in MATRICES:
        assert isinstance(d[k], list) and np.asarray(d[k]).shape == (3, 3), k
    assert isinstance(d["error"], list) and len(d["error"]) == 3
    tv = np.asarray(d["tv"])
    assert np.array_equal(tv, tv.T) and not np.diag(tv).any() and (tv >= 0).all() and tv[0, 1] > 0
    assert (np.asarray(d["kl"]) >= -1e-6).all()
    s = d["summary"]
    assert sorted(s) == ["disagreement", "double_fault", "nearest", "sym_kl", "tv"]
    assert 0 <= s["disagreement"]["min"] <= s["disagreement"]["mean"] <= s["disagreement"]["max"] <= 1
    assert len(s["nearest"]) == 3
    lines = _lines(tmp_path / "d", "[Diversity]")
    assert len(lines) == 2
    for word in ("3 chains, 96 examples", "disagreement =", "closest chains", "furthest chains",
                 "tv =", "sym_kl =", "double_fault =", "0 non-finite"):
        assert word in lines[-1], word
    # without the flag: no line, no record
    hist0 = main(ARGV + [str(tmp_path / "p"), "--stacked_chains", "3"])
    assert all("diversity" not in h for h in hist0) and not _lines(tmp_path / "p", "[Diversity]")


def test_cli_refuses_diversity_without_stacked_chains(tmp_path, capsys):
    from bayesdll_amd.run import main
    with pytest.raises(SystemExit):
        main(ARGV + [str(tmp_path / "r"), "--diversity"])
    assert "--stacked_chains" in capsys.readouterr().err
