"""bayesdll_amd.run --stacked_chains with the Adam samplers and --clip_grad:
one tiny end-to-end run through the CLI on the GPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_cli_stacked_adam_csghmc_with_clip(tmp_path):
    """--stacked_chains 4 --method adam_csghmc --clip_grad 1.0: two epochs (two
    cycles), the stacked-chains line and one clip line per epoch in the log."""
    from bayesdll_amd.run import main
    hist = main(["--method", "adam_csghmc", "--dataset", "mnist", "--backbone", "mlp_mnist",
                 "--epochs", "2", "--num_cycles", "2", "--batch_size", "64", "--lr", "1e-2",
                 "--train_size", "256", "--test_size", "64", "--val_heldout", "0",
                 "--stacked_chains", "4", "--clip_grad", "1.0",
                 "--hparams", "prior_sig=1.0,Ninflate=1.0,nd=0.01,momentum_decay=0.05,burnin=0,"
                              "thin=1,bias=informative,nst=2,beta1=0.9,beta2=0.999",
                 "--log_dir", str(tmp_path)])
    assert len(hist) == 2 and all(len(h["loss"]) == 4 for h in hist)
    assert all(np.isfinite(h["loss"]).all() for h in hist)
    assert all("test" in h and np.isfinite(h["test"][0]) for h in hist)
    assert all(0 <= h["clip"]["clipped"] <= 4 and np.isfinite(h["clip"]["max_norm"]) for h in hist)
    text = next(tmp_path.rglob("logs.txt")).read_text()
    assert "4 stacked chains" in text
    assert text.count("clip_grad 1: ") == 2 and "of 4 chains clipped at the last step" in text


def test_cli_names_the_methods_that_stack(tmp_path):
    from bayesdll_amd.run import main
    with pytest.raises(ValueError, match="csghmc_fs is not stacked.*adam_csghmc"):
        main(["--method", "csghmc_fs", "--dataset", "mnist", "--backbone", "mlp_mnist",
              "--epochs", "1", "--train_size", "64", "--test_size", "64", "--val_heldout", "0",
              "--stacked_chains", "2", "--log_dir", str(tmp_path)])
