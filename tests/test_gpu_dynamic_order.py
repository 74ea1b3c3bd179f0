"""The dynamic sweep order of the cSGHMC sweeps (bdl_set_launch_config order 2,
include/bdl_order.h; csg_sweep in bdl_kernels.hpp): workgroups claim blocks of
BDL_CLAIM_GROUPS float4 groups from a device counter instead of owning a fixed
stride.  The update is elementwise and the Philox draw keyed by element, so
order 2 must give bit for bit what order 1 gives on theta, mom, m1 and m2:

* every kind (explore, Philox sample, Welford init, steady Welford) at depths
  1 / 2 / 4 and 1 / 2 workgroups per CU, on a flat 2-run table at the sizes
  where the claim logic changes path (more claims than workgroups with a
  partial last group; less than one claim block; a half last block; n = 5)
  and on a table of per-tensor gradients whose boundaries (4-aligned, and one
  that is not) fall inside claimed blocks: the multi-run and guarded paths;
* the counter pairs over 3 x (slots) + 1 launches of alternating kinds: the
  same chain as order 1, the stream walks its own slots as a ring, and every
  counter reads zero afterwards;
* two states on two streams back to back equal the serial run;
* a launch captured into a graph runs order 1 (bdl_order_last) and replays
  bit-identically to eager.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

KINDS = ["explore", "sample", "init", "steady"]
DEPTHS = [1, 2, 4]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _per_claim():
    from bayesdll_amd import _lib as L
    return 4 * L.CLAIM_GROUPS  # elements of one claim block: 4 * kBlock * U * C at every depth U


def _grid(bpc):
    return torch.cuda.get_device_properties(0).multi_processor_count * bpc


def _flat_sizes(bpc):
    per, grid = _per_claim(), _grid(bpc)
    return {"many_claims": per * (grid + 3) + 1, "under_one_block": per - 4,
            "half_last_block": per * grid + per // 2, "five": 5}


_CACHE = {}


def _flat_state(n):
    """A 2-run state (body, head) of n elements and its initial vectors."""
    from bayesdll_amd.flat import FlatState
    key = ("flat", n)
    if key not in _CACHE:
        head = max(1, min(1000, n // 3))
        segs = [("body.weight", (n - head,)), ("head.weight", (head,))]
        st = FlatState.from_segments(segs, "head", device=DEV, need_mom=True)
        assert st.nruns == 2
        _CACHE[key] = (st, _init_vectors(st.n, 3))
    return _CACHE[key]


def _init_vectors(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    v = {k: torch.empty(n, device=DEV).normal_(0.0, s, generator=g)
         for k, s in (("theta", 0.02), ("grad", 1e-2), ("mom", 1e-4), ("m1", 0.02))}
    v["m2"] = torch.empty(n, device=DEV).uniform_(0.0, 1e-3, generator=g)
    return v


def _table_state():
    """21 per-tensor-gradient runs over more claim blocks than one workgroup
    per CU has workgroups: 20 tensors at 4-aligned offsets, their boundaries
    inside claimed blocks (the multi-run path), the last of them 3 elements
    long, so that the head after it starts off a float4 boundary (the guarded
    path)."""
    from bayesdll_amd.flat import FlatState
    if "table" not in _CACHE:
        per = _per_claim()
        sizes = [per * (_grid(1) + 6) // 19 // 4 * 4 + 4 * (i + 1) for i in range(19)]
        sizes = sizes + [3]  # the head after it starts off a float4 boundary
        segs = [(f"layer{i}.weight", (k,)) for i, k in enumerate(sizes)] + [("head.weight", (1000,))]
        st = FlatState.from_segments(segs, "head", device=DEV, need_mom=True)
        init = _init_vectors(st.n, 4)
        grads = [init["grad"][o:o + k].clone() for o, k in zip(st.offsets, st.numels)]
        st.use_tensor_grads(grads)
        st._keep = grads
        offs = np.asarray(st.offsets)
        assert st.nruns == 21 and st.gbase is not None
        assert (offs[:20] % 4 == 0).all() and offs[20] % 4 != 0
        assert st.n > per * (_grid(1) + 3)
        _CACHE["table"] = (st, init)
    return _CACHE["table"]


def _step(st, kind, m1, m2, t=3):
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    noise = kind != "explore"
    collect = {"init": L.COLLECT_WELFORD_INIT, "steady": L.COLLECT_WELFORD}.get(kind, L.COLLECT_NONE)
    K.sgmcmc_step(st, L.CSGHMC, lrs=(1e-3, 2e-2), noise_scale=(1e-4, 2e-4) if noise else (0.0, 0.0),
                  noise_mode=L.NOISE_PHILOX if noise else L.NOISE_NONE, one_minus_alpha=0.82,
                  prior_sig=1.0, collect=collect, mom1=m1 if collect else None,
                  mom2=m2 if collect else None, collect_a=float(t), seed=11, chain=2, step=t)


def _run(st, init, kind, geo):
    """One launch of `kind` from the initial vectors at geometry geo; returns
    (theta | mom | m1 | m2, (order, slot) the launch ran)."""
    from bayesdll_amd import kernels as K
    st.theta.copy_(init["theta"])
    st.mom.copy_(init["mom"])
    if st.grad is not None:
        st.grad.copy_(init["grad"])
    m1, m2 = init["m1"].clone(), init["m2"].clone()
    K.set_launch_config(*geo)
    _step(st, kind, m1, m2)
    ran = K.last_order()
    torch.cuda.synchronize()
    assert int(st.nonfinite.item()) == 0
    return torch.cat([st.theta, st.mom, m1, m2]), ran


def _reference(name, st, init, kind):
    key = ("ref", name, kind)
    if key not in _CACHE:
        out, ran = _run(st, init, kind, (2, 1, 1))
        assert ran == (1, -1)
        _CACHE[key] = out.clone()
    return _CACHE[key]


def _compare(name, st, init, bpc):
    from bayesdll_amd import kernels as K
    try:
        for kind in KINDS:
            want = _reference(name, st, init, kind)
            for depth in DEPTHS:
                got, ran = _run(st, init, kind, (bpc, depth, 2))
                assert ran[0] == 2 and ran[1] >= 0, (kind, depth, ran)
                assert torch.equal(got, want), (name, kind, depth, bpc)
    finally:
        K.set_launch_config(0, 0, 0)


@pytest.mark.parametrize("bpc", [1, 2])
@pytest.mark.parametrize("shape", ["many_claims", "under_one_block", "half_last_block", "five"])
def test_dynamic_order_equals_grid_stride_on_flat_tables(shape, bpc):
    n = _flat_sizes(bpc)[shape]
    st, init = _flat_state(n)
    _compare(f"{shape}-{n}", st, init, bpc)


@pytest.mark.parametrize("bpc", [1, 2])
def test_dynamic_order_equals_grid_stride_inside_claimed_blocks_of_a_tensor_table(bpc):
    st, init = _table_state()
    _compare("table", st, init, bpc)


def _chain(st, init, geo, launches, streams=None):
    """`launches` steps of alternating kinds on one state; returns the final
    vectors and the (order, slot) of every launch."""
    from bayesdll_amd import kernels as K
    st.theta.copy_(init["theta"])
    st.mom.copy_(init["mom"])
    st.grad.copy_(init["grad"])
    m1, m2 = init["m1"].clone(), init["m2"].clone()
    K.set_launch_config(*geo)
    ran = []
    for t in range(launches):
        _step(st, ["init", "explore", "steady", "sample"][t % 4], m1, m2, t=t + 1)
        ran.append(K.last_order())
    torch.cuda.synchronize()
    return torch.cat([st.theta, st.mom, m1, m2]).clone(), ran


def test_counter_pairs_over_three_ring_lengths_and_one():
    from bayesdll_amd import _lib as L
    from bayesdll_amd import kernels as K
    st, init = _flat_state(_flat_sizes(1)["many_claims"])
    launches = 3 * L.CLAIM_SLOTS + 1
    try:
        want, ran1 = _chain(st, init, (1, 4, 1), launches)
        got, ran2 = _chain(st, init, (1, 4, 2), launches)
    finally:
        K.set_launch_config(0, 0, 0)
    assert all(r == (1, -1) for r in ran1)
    assert all(r[0] == 2 for r in ran2)
    slots = [r[1] for r in ran2]
    # one stream binds at most CLAIM_SLOTS_PER_STREAM slots and walks them in turn
    assert len(set(slots)) <= L.CLAIM_SLOTS_PER_STREAM
    period = len(set(slots))
    assert all(slots[i] == slots[i + period] for i in range(len(slots) - period))
    assert torch.equal(got, want)
    assert not K.order_counters().any()


def test_two_states_on_two_streams_equal_the_serial_run():
    from bayesdll_amd import kernels as K
    n = _flat_sizes(1)["many_claims"]
    st_a, init = _flat_state(n)
    from bayesdll_amd.flat import FlatState
    st_b = FlatState.from_segments([("body.weight", (n - 1000,)), ("head.weight", (1000,))], "head",
                                   device=DEV, need_mom=True)
    init_b = _init_vectors(n, 8)
    try:
        serial = [_chain(st, i, (1, 4, 2), 6)[0] for st, i in ((st_a, init), (st_b, init_b))]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        K.set_launch_config(1, 4, 2)
        states = []
        for st, i in ((st_a, init), (st_b, init_b)):
            st.theta.copy_(i["theta"])
            st.mom.copy_(i["mom"])
            st.grad.copy_(i["grad"])
            states.append((st, i["m1"].clone(), i["m2"].clone()))
        torch.cuda.synchronize()
        slots = {s1: set(), s2: set()}
        for t in range(6):
            for s, (st, m1, m2) in zip((s1, s2), states):
                with torch.cuda.stream(s):
                    _step(st, ["init", "explore", "steady", "sample"][t % 4], m1, m2, t=t + 1)
                    order, slot = K.last_order()
                    assert order == 2
                    slots[s].add(slot)
        torch.cuda.synchronize()
    finally:
        K.set_launch_config(0, 0, 0)
    assert not slots[s1] & slots[s2]  # a counter pair never serves two streams
    for (st, m1, m2), want in zip(states, serial):
        assert torch.equal(torch.cat([st.theta, st.mom, m1, m2]), want)
    assert not K.order_counters().any()


def test_a_captured_launch_runs_grid_stride_and_replays_as_eager():
    from bayesdll_amd import kernels as K
    st, init = _flat_state(_flat_sizes(1)["many_claims"])
    try:
        want, ran = _run(st, init, "sample", (1, 4, 2))
        assert ran[0] == 2
        want = want.clone()
        st.theta.copy_(init["theta"])
        st.mom.copy_(init["mom"])
        st.grad.copy_(init["grad"])
        m1, m2 = init["m1"].clone(), init["m2"].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _step(st, "sample", m1, m2)
            captured = K.last_order()
        assert captured == (1, -1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([st.theta, st.mom, m1, m2]), want)
    finally:
        K.set_launch_config(0, 0, 0)
    assert not K.order_counters().any()
