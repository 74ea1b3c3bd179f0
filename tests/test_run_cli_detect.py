"""bayesdll_amd.run --detect / --detect_shift: a tiny stacked SGLD run logs one
line per task at every evaluation and fills rec["detection"] (GPU); under
--sweep one line per chain and task."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SCORES = ("entropy", "mutual_info", "expected_entropy", "neg_confidence", "disagree")
ARGV = ["--method", "sgld", "--dataset", "mnist", "--backbone", "mlp_mnist", "--epochs", "2",
        "--batch_size", "64", "--lr", "1e-2", "--train_size", "256", "--test_size", "96",
        "--val_heldout", "0", "--stacked_chains", "3",
        "--hparams", "prior_sig=1.0,Ninflate=1.0,nd=1.0,burnin=0,thin=1,nst=2,bias=informative,temp=1.0",
        "--log_dir"]


def _lines(path, word):
    return [ln for ln in next(path.rglob("logs.txt")).read_text().splitlines()[1:] if word in ln]


def test_cli_stacked_sgld_logs_both_detection_lines(tmp_path):
    from bayesdll_amd.run import main
    hist = main(ARGV + [str(tmp_path / "d"), "--detect", "--detect_shift", "0.5"])
    assert len(hist) == 2 and all("test" in h and "detection" in h for h in hist)
    d = hist[-1]["detection"]
    assert sorted(d) == ["members", "misclassification", "shift"] and d["members"] == 6
    mis, sh = d["misclassification"], d["shift"]
    assert mis["n_pos"] + mis["n_neg"] == 96 and mis["n_excluded"] == 0
    assert (sh["n_pos"], sh["n_neg"], sh["n_excluded"]) == (96, 96, 0)
    for t in (mis, sh):
        for nm in SCORES:
            assert 0 <= t[nm]["auroc"] <= 1 and 0 < t[nm]["ap"] <= 1 and 0 <= t[nm]["fpr95"] <= 1
    for task in ("misclassification", "shift"):
        lines = _lines(tmp_path / "d", f"{task} detection over 3 chains")
        assert len(lines) == 2
        for word in ("(6 members,", "positives", "negatives", "excluded") + tuple(
                f"{nm}: AUROC =" for nm in SCORES) + ("AP =", "FPR95 ="):
            assert word in lines[-1], word
    # --detect alone: the misclassification line only
    hist1 = main(ARGV + [str(tmp_path / "m"), "--detect"])
    assert all("shift" not in h["detection"] for h in hist1)
    assert len(_lines(tmp_path / "m", "misclassification detection")) == 2
    assert not _lines(tmp_path / "m", "shift detection")
    # without the flag: no line, no record
    hist0 = main(ARGV + [str(tmp_path / "p")])
    assert all("detection" not in h for h in hist0) and not _lines(tmp_path / "p", "detection")


def test_cli_sweep_logs_one_detection_line_per_chain(tmp_path):
    from bayesdll_amd.run import main
    hist = main(ARGV + [str(tmp_path / "s"), "--detect", "--sweep", "lr=1e-3,1e-2,5e-2"])
    d = hist[-1]["detection"]["misclassification"]
    assert len(d["entropy"]["auroc"]) == 3 and len(d["n_pos"]) == 3
    assert np.isfinite(d["entropy"]["ap"]).all()
    lines = _lines(tmp_path / "s", "misclassification detection chain")
    assert len(lines) == 2 * 3 and "lr=" in lines[-1]
