"""bayesdll_amd.run --fn_probe P --fn_batch B on the GPU: a tiny stacked SGLD
run logs the function-space line and fills rec["function_space"] at every
evaluation; without the flags the log is line for line the same, minus that
line (the parse and its refusals: tests/test_fn_host.py)."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu


def _lines(root):
    text = next(root.rglob("logs.txt")).read_text().splitlines()[1:]   # [0]: the command
    body = [re.sub(r"^\[[^\]]*\] ", "", ln) for ln in text if ln.strip()]
    return [re.sub(r"\(\d+\.\d+ s\)", "", ln) for ln in body]


def test_cli_stacked_sgld_logs_the_function_space_line(tmp_path):
    from bayesdll_amd.run import main
    argv = ["--method", "sgld", "--dataset", "mnist", "--backbone", "mlp_mnist", "--epochs", "2",
            "--batch_size", "64", "--lr", "1e-2", "--train_size", "256", "--test_size", "64",
            "--val_heldout", "0", "--stacked_chains", "3",
            "--hparams", "prior_sig=1.0,Ninflate=1.0,nd=1.0,burnin=0,thin=1,nst=2,bias=informative,temp=1.0",
            "--log_dir"]
    hist = main(argv + [str(tmp_path / "f"), "--fn_probe", "16", "--fn_batch", "2"])
    assert len(hist) == 2 and all("test" in h and "function_space" in h for h in hist)
    for h, samples in zip(hist, (4, 8)):                           # four collect steps an epoch
        fs = h["function_space"]
        assert (fs["probe"], fs["classes"], fs["batch"]) == (16, 10, 2)
        assert (fs["samples"], fs["batches"]) == (samples, samples // 2)
        assert fs["rhat"]["n_eval"] + fs["rhat"]["n_degenerate"] + fs["rhat"]["n_nonfinite"] == 160
        assert fs["ess"]["n_eval"] + fs["ess"]["n_degenerate"] + fs["ess"]["n_nonfinite"] == 160
        assert fs["rhat"]["n_nonfinite"] == fs["ess"]["n_nonfinite"] == 0
        assert fs["rhat"]["rhat_max"] >= 0 and fs["ess"]["ess_min"] >= 0
        assert not any(isinstance(v, torch.Tensor) for part in (fs["rhat"], fs["ess"])
                       for v in part.values())
    with_flags = _lines(tmp_path / "f")
    mine = [ln for ln in with_flags if "function space over 3 chains" in ln]
    assert len(mine) == 2
    for word in ("16 probe examples x 10 classes", "8 samples each, 4 batches of 2", "R-hat max =",
                 "ESS min =", "degenerate", "non-finite"):
        assert word in mine[-1], word
    # each sits right after its evaluation's predictive line
    for ln in mine:
        assert "stacked predictive" in with_flags[with_flags.index(ln) - 1]
    # without the flags: no record, and the same log minus those lines
    hist0 = main(argv + [str(tmp_path / "p")])
    assert all("function_space" not in h for h in hist0)
    assert [h["test"] for h in hist0] == [h["test"] for h in hist]
    assert _lines(tmp_path / "p") == [ln for ln in with_flags if ln not in mine]
