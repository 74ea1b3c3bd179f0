"""bayesdll_amd.run --exchange: the parser's refusals (no device), the log line
and record of _report_exchange with a stub sampler, and one stacked run on the
device."""
import pytest

LADDER = ["--stacked_chains", "3", "--sweep", "nd=1,1.5,2.2", "--momentum", "0"]


def test_run_cli_exchange_parses_and_needs_an_nd_ladder(capsys):
    from bayesdll_amd import run
    ap = run.build_parser()
    a = ap.parse_args([])
    assert a.exchange == 0 and a.exchange_var == 0.0 and run.check_exchange(ap, a) == 0
    a = ap.parse_args(["--method", "sgld", "--exchange", "4", "--exchange_var", "0.5"] + LADDER)
    assert run.check_exchange(ap, a) == 4 and a.exchange_var == 0.5
    a = ap.parse_args(["--method", "csgld", "--exchange", "1"] + LADDER)
    assert run.check_exchange(ap, a) == 1
    for argv, why in (
            (["--method", "sgld", "--exchange", "2", "--stacked_chains", "3", "--momentum", "0"],
             "it needs --sweep nd="),
            (["--method", "sgld", "--exchange", "2", "--stacked_chains", "3", "--momentum", "0",
              "--sweep", "lr=1e-2,1e-3,1e-4"], "it needs --sweep nd="),
            (["--method", "sgld", "--exchange", "2"], "it needs --stacked_chains >= 2"),
            (["--method", "csghmc", "--exchange", "2"] + LADDER, "no temperature is derived for"),
            (["--method", "sgld", "--exchange", "2", "--stacked_chains", "3", "--sweep",
              "nd=1,2,3"], "needs --momentum 0"),
            (["--method", "sgld", "--exchange", "-1"] + LADDER, "M must be >= 1"),
            (["--method", "sgld", "--exchange_var", "0.5"] + LADDER, "it needs --exchange M"),
            (["--method", "sgld", "--exchange", "2", "--exchange_var", "-1"] + LADDER,
             "--exchange_var must be >= 0")):
        with pytest.raises(SystemExit) as e:
            run.main(argv)
        assert e.value.code == 2 and why in capsys.readouterr().err, why


class _Stub:
    def exchange(self):
        return {"pairs": [{"slots": (0, 1), "attempts": 10, "accepts": 4, "rate": 0.4,
                           "temperatures": (1.0, 2.25)},
                          {"slots": (1, 2), "attempts": 9, "accepts": 0, "rate": 0.0,
                           "temperatures": (2.25, 4.0)}],
                "replica": [1, 0, 2], "round_trips": [0, 1, 0], "round_trips_total": 1,
                "refused": 0, "attempt": 19, "cold": [0]}


def test_report_logs_one_line_and_keeps_the_record():
    from bayesdll_amd import stacked
    rec, lines = {"epoch": 2}, []
    stacked._StackedSampler._report_exchange(_Stub(), 2, rec, lines.append)
    assert lines == ["(Epoch 2) replica exchange after 19 attempts: accepted 0-1: 4/10, 1-2: 0/9; "
                     "replica = [1, 0, 2], round trips = 1, refused = 0"]
    assert rec["exchange"] == _Stub().exchange() and rec["epoch"] == 2


@pytest.mark.gpu
def test_cli_stacked_ladder_logs_the_exchange_line_and_writes_the_record(tmp_path):
    from bayesdll_amd.run import main
    argv = ["--method", "sgld", "--dataset", "mnist", "--backbone", "mlp_mnist", "--epochs", "2",
            "--batch_size", "64", "--lr", "1e-2", "--train_size", "256", "--test_size", "64",
            "--val_heldout", "0.25", "--stacked_chains", "3", "--momentum", "0",
            "--sweep", "nd=1,1.5,2.2",
            "--hparams", "prior_sig=1.0,Ninflate=1.0,nd=1.0,burnin=0,thin=1,nst=0,bias=informative,temp=1.0",
            "--exchange", "2", "--log_dir", str(tmp_path / "x")]
    hist = main(argv)
    assert len(hist) == 2 and all("exchange" in h for h in hist)
    d = hist[-1]["exchange"]
    steps = d["attempt"] * 2
    assert d["attempt"] >= 2 and sorted(d["replica"]) == [0, 1, 2] and d["cold"] == [0]
    assert sum(p["attempts"] for p in d["pairs"]) == d["attempt"]   # K = 3: one pair per attempt
    assert [p["temperatures"] for p in d["pairs"]] == [(1.0, 2.25), (2.25, 2.2 * 2.2)]
    text = next((tmp_path / "x").rglob("logs.txt")).read_text().splitlines()
    xl = [ln for ln in text if ") replica exchange after " in ln]
    assert len(xl) == 2 and f"after {d['attempt']} attempts" in xl[-1] and steps > 0
    hist0 = main(argv[:-4] + ["--log_dir", str(tmp_path / "p")])
    assert all("exchange" not in h for h in hist0)
