"""The same-seed reference chains (tests/same_seed_ref.py) on the CPU, alone.

1. Draw count: in every case the GPU tests run, each step makes exactly one
   randn_like call per tensor with a gradient in that step, of that tensor's
   shape, in named_parameters order — counted at torch.randn_like itself.
2. Sensitivity: the GPU tests compare theta at RTOL = 1e-5.  For that to
   notice a misaligned stream, the misalignment has to move theta by much
   more: every deliberately wrong reference (same_seed_ref.MISALIGNMENTS) that
   applies to a case must differ from the right one by at least 100 x RTOL in
   rel_err on theta.  This is a condition on the cases' scalars, checked from
   the reference alone; a case that misses it gets a larger noise scale, never
   a wider tolerance.
"""
import numpy as np
import pytest
import torch

import same_seed_ref as R

MIN_RATIO = 100.0  # x RTOL


@pytest.fixture(scope="module")
def right():
    """The right chain of every case, computed once."""
    return {nm: R.reference_chain(c, "cpu") for nm, c in R.CASES.items()}


@pytest.mark.parametrize("name", list(R.CASES))
def test_one_draw_per_tensor_with_a_gradient(name, monkeypatch):
    c = R.CASES[name]
    calls = []
    real = torch.randn_like

    def counting(t, *a, **kw):
        calls.append(tuple(t.shape))
        return real(t, *a, **kw)

    monkeypatch.setattr(torch, "randn_like", counting)
    ch = R.RefChain(c, "cpu")
    shapes = [tuple(p.shape) for p in ch.params]
    for k in range(c["steps"]):
        del calls[:]
        ch.step()
        want = R.expected_live(c, k, ch.names)
        assert ch.live[k] == want
        assert list(ch.draws[k]) == want  # drawn in named_parameters order
        assert calls == [shapes[i] for i in want]
        for i in want:
            assert ch.draws[k][i].shape == ch.params[i].shape
    if c["frozen"] or c["skip"]:
        assert any(len(lv) < len(shapes) for lv in ch.live)
        assert len({tuple(lv) for lv in ch.live}) > (1 if c["skip"] else 0)


def test_tables_are_what_the_gpu_tests_expect():
    many = R.many_segments()
    assert len(many) == 40
    sizes = [int(np.prod(s)) for _, s in many[:-2]]
    assert sizes == [R.MANY_SIZES[i % 8] for i in range(38)]
    offsets = np.cumsum([0] + [int(np.prod(s)) for _, s in many])[:-1]
    assert np.count_nonzero(offsets % 4) > len(many) // 2
    mlp = R.mlp_segments()
    assert len(mlp) == 8 and R.numel_of(mlp) == 2797010


def test_the_clipped_case_clips_every_step(right):
    for name, c in R.CASES.items():
        if c["clip_grad"] is not None:
            norms = right[name].clip_norms
            assert len(norms) == c["steps"]
            assert min(norms) > 2 * c["clip_grad"], (name, norms)


def test_skipped_tensors_are_left_alone_by_the_reference():
    c = R.CASES["adam_sghmc_mom-nograd-toy"]
    ch = R.RefChain(c, "cpu")
    for k in range(c["steps"]):
        before = {key: v.copy() for key, v in ch.state().items()}
        ch.step()
        after = ch.state()
        off = np.cumsum([0] + [p.numel() for p in ch.params])
        for i in set(range(len(ch.params))) - set(ch.live[k]):
            for key in before:
                np.testing.assert_array_equal(after[key][off[i]:off[i + 1]],
                                              before[key][off[i]:off[i + 1]], err_msg=f"{key} {i}")


_RATIOS = {}


def _ratios(name, right):
    if name not in _RATIOS:
        _RATIOS[name] = _compute_ratios(name, right)
    return _RATIOS[name]


def _compute_ratios(name, right):
    c = R.CASES[name]
    want = right[name].state()["theta"]
    out = {}
    for mis in R.applicable(c):
        got = R.reference_chain(c, "cpu", misalign=mis).state()["theta"]
        out[mis] = R.rel_err(got, want) / R.RTOL
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_a_misaligned_stream_moves_theta_far_beyond_the_tolerance(name, right):
    ratios = _ratios(name, right)
    print(name, {k: f"{v:.0f} x RTOL" for k, v in ratios.items()})
    assert ratios, "no misalignment applies: the case checks nothing about the stream"
    for mis, r in ratios.items():
        assert r >= MIN_RATIO, (name, mis, r)


@pytest.mark.parametrize("kind", R.EVAL_KINDS)
@pytest.mark.parametrize("name", list(R.EVAL_CASES))
def test_misaligned_evaluation_draws_move_theta_and_the_samples(name, kind):
    c = R.EVAL_CASES[name]
    ch, samples = R.reference_train_eval_train(c, "cpu", kind)
    n = sum(p.numel() for p in ch.params)
    assert len(samples) == R.EVAL_SCHEDULE[1] and len(ch.draws) == c["steps"]
    assert all(e.numel() == n for e in ch.eval_draws)  # frozen parameters drawn too
    want = ch.state()["theta"]
    for mis in R.applicable(c, evaluation=True):
        bad, bad_samples = R.reference_train_eval_train(c, "cpu", kind, misalign=mis)
        if mis == "eval_trainable_only" and kind != "none":
            # the first sample already differs (variance 1e-12: it is the mean either way)
            rs = R.rel_err(bad_samples[0].numpy(), samples[0].numpy()) / R.RTOL
            print(name, kind, mis, f"sample {rs:.0f} x RTOL")
            assert rs >= MIN_RATIO, (name, kind, mis, rs)
        # the training stream after the evaluation shifts
        r = R.rel_err(bad.state()["theta"], want) / R.RTOL
        print(name, kind, mis, f"theta {r:.0f} x RTOL")
        assert r >= MIN_RATIO, (name, kind, mis, r)


def test_smallest_sensitivity_ratio(right):
    """The figure the tolerance rests on: the smallest theta shift any
    applicable misalignment causes in any case, in units of RTOL."""
    worst = min((r, nm, mis) for nm in R.CASES for mis, r in _ratios(nm, right).items())
    print("smallest misalignment / RTOL:", worst)
    assert worst[0] >= MIN_RATIO
