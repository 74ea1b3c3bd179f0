"""The stacked tables of tests/stacked_tables.py reach the sweep paths that
tests/test_gpu_stacked_reference.py claims for them — proven on the CPU, so
that the GPU tests cannot pass vacuously after a geometry change.

classify() restates the three conditions of step_body (bdl_kernels.hpp) over
the run table bdl_build_runs returns (a host function: no device needed) and
is itself checked on hand-written run tables with literal answers.  Block
iterations always start on a multiple of 256 * depth groups, in both sweep
orders and for every grid, so the classes do not depend on order or grid; the
tests run all of them all the same.
"""
import pytest

import stacked_tables as T

DEPTHS = [1, 2, 4]
LAUNCHES = [(grid, order) for order in (0, 1) for grid in (1, 8)]  # (grid cap, grid-stride)


def _inside(lay, it, k):
    """The paths of the iterations lying wholly inside chain k."""
    lo, hi = k * lay.chain_groups, (k + 1) * lay.chain_groups
    return [p for gb, ge, p in it if gb >= lo and ge <= hi]


def _with_seam(lay, it):
    """(seam, path) of every iteration that holds groups of two chains."""
    return [(s, p) for gb, ge, p in sorted(it) for s in lay.seams() if gb < s < ge]


# ------------------------------------------------------------- the classifier
def test_classifier_on_hand_written_run_tables():
    PRIOR, HEAD, SKIP, GUN = 0x2, 0x1, T.ATTR_SKIP, T.ATTR_GUNALIGNED
    # 1. one run of 3 x 1024 + 6 elements at depth 1 (1024 elements per
    #    iteration): three full iterations inside the run, then the tail
    runs = [(3078, PRIOR)]
    got = [T.classify(runs, 3078, gb, ge, 1) for gb, ge in T.block_iterations(3078, 1, 8, 1)]
    assert got == ["fast", "fast", "fast", "slow"]
    # 2. boundaries at 1000 (4-aligned), 2050 (not), a SKIP run from 4096 to
    #    5120, an unaligned-gradient run to 6144, then 2048 plain elements
    runs = [(1000, PRIOR), (2050, PRIOR | HEAD), (4096, PRIOR), (5120, SKIP), (6144, PRIOR | GUN),
            (8192, PRIOR)]
    got = [T.classify(runs, 8192, gb, ge, 1) for gb, ge in T.block_iterations(8192, 1, 1, 0)]
    assert got == ["multi", "fast", "slow", "fast", "slow", "slow", "fast", "fast"]
    #    depth 2 (2048 elements per iteration): across 1000 / across 2050 / SKIP and GUN / one run
    got = [T.classify(runs, 8192, gb, ge, 2) for gb, ge in T.block_iterations(8192, 2, 8, 0)]
    assert got == ["multi", "slow", "slow", "fast"]
    # 3. two full iterations that differ only in where the boundary falls,
    #    and a last iteration that is full in groups but partial in elements
    assert T.classify([(512, PRIOR), (2048, HEAD)], 2048, 0, 256, 1) == "multi"
    assert T.classify([(514, PRIOR), (2048, HEAD)], 2048, 0, 256, 1) == "slow"
    assert T.classify([(2046, PRIOR)], 2046, 256, 512, 1) == "slow"
    assert T.classify([(2048, PRIOR)], 2048, 256, 512, 1) == "fast"


def test_block_iterations_cover_every_group_once():
    for n in (3078, 118284, 30000, 18000):
        for depth in DEPTHS:
            for grid, order in LAUNCHES:
                it = sorted(T.block_iterations(n, depth, grid, order))
                assert it[0][0] == 0 and it[-1][1] == (n + 3) // 4
                assert all(a[1] == b[0] for a, b in zip(it, it[1:]))
                assert all(gb % (T.K_BLOCK * depth) == 0 for gb, _ in it)


# ------------------------------------------------------------------ the tables
def test_layouts():
    a, b, c = T.table_a(), T.table_b(), T.table_c()
    assert (a.K, a.n1, a.stride, a.chain_groups, a.n) == (3, 39426, 39428, 9857, 118284)
    assert a.chain_groups % 256 == 129
    assert (b.K, b.stride, b.chain_groups, b.n) == (5, 6000, 1500, 30000)
    assert b.seams() == [1500, 3000, 4500, 6000]
    assert (c.K, c.stride, c.chain_groups, c.n) == (6, 3000, 750, 18000)
    ra, rb, rc = (x.flat_runs().tolist() for x in (a, b, c))
    assert rb == [[30000, b.attrs[0]]]  # seamless: the whole stack is one run
    # A: each chain's 2-element gap is a SKIP run ending on the seam
    for k in range(3):
        assert [(k + 1) * a.stride, T.ATTR_SKIP] in ra
        assert any(end == k * a.stride + a.n1 for end, _ in ra)
    # C: 4-aligned runs, attributes alternating across every seam
    assert [end for end, _ in rc] == [e for k in range(6) for e in (3000 * k + 2000, 3000 * k + 3000)]
    assert [at for _, at in rc] == [c.attrs[0], c.attrs[1]] * 6 and c.attrs[0] != c.attrs[1]
    assert not any(at & T.NO_FAST_PATH for _, at in rc)


# chains that own a multi iteration lying wholly inside them, per depth.  At
# depth 4 chain 0 owns none: it starts at group 0, where the table's depth-4
# iterations inside the chain are 7 fast and 2 slow (the only one that crosses
# 4-aligned boundaries, elements [12288, 16384), also holds the odd boundary at
# 16295, and the table is fixed: test_gpu_noise_units.SEGMENTS); chains 1 and 2
# start at other lane phases and own 2 and 1.
MULTI_OWNERS = {1: {0, 1, 2}, 2: {0, 1, 2}, 4: {1, 2}}


@pytest.mark.parametrize("depth", DEPTHS)
def test_table_a_every_chain_owns_fast_and_multi_iterations(depth):
    """At every depth, sweep order and grid: every chain k = 0..2 owns at
    least one fast iteration lying wholly inside it, exactly the chains of
    MULTI_OWNERS own a multi one, and every iteration that holds a seam is
    slow.  Over the depths every chain owns both kinds, and where chain 0 owns
    no multi iteration of its own (depth 4) table C sends all of its groups
    through one."""
    lay = T.table_a()
    for grid, order in LAUNCHES:
        it = T.classified(lay, depth, grid, order)
        own = [_inside(lay, it, k) for k in range(lay.K)]
        assert all("fast" in o for o in own), (depth, grid, order)
        assert {k for k, o in enumerate(own) if "multi" in o} == MULTI_OWNERS[depth]
        seams = _with_seam(lay, it)
        assert [s for s, _ in seams] == lay.seams() and all(p == "slow" for _, p in seams)
    assert set.union(*MULTI_OWNERS.values()) == set(range(lay.K))
    for d, owners in MULTI_OWNERS.items():
        if 0 not in owners:  # chain 0's groups on the multi path at that depth: table C
            c = T.table_c()
            assert c.chain_groups <= T.K_BLOCK * d
            for grid, order in LAUNCHES:
                assert sorted(T.classified(c, d, grid, order))[0] == (0, T.K_BLOCK * d, "multi")


def test_table_a_depth_4_multi_iterations():
    """What table A reaches at depth 4, stated exactly: every chain owns fast
    and slow iterations, chains 1 and 2 own multi iterations, chain 0 owns
    none (its groups take the multi path at depth 4 on table C, whose first
    iteration holds all of chain 0)."""
    lay, c = T.table_a(), T.table_c()
    for grid, order in LAUNCHES:
        it = T.classified(lay, 4, grid, order)
        count = [{p: _inside(lay, it, k).count(p) for p in ("fast", "multi", "slow")}
                 for k in range(lay.K)]
        assert count == [{"fast": 7, "multi": 0, "slow": 2}, {"fast": 5, "multi": 2, "slow": 2},
                         {"fast": 4, "multi": 1, "slow": 4}]
        first = sorted(T.classified(c, 4, grid, order))[0]
        assert first == (0, 1024, "multi") and c.chain_groups < 1024


@pytest.mark.parametrize("depth", DEPTHS)
def test_table_b_seams_lie_in_fast_iterations(depth):
    lay = T.table_b()
    assert lay.flat_runs().shape[0] == 1
    for grid, order in LAUNCHES:
        seams = _with_seam(lay, T.classified(lay, depth, grid, order))
        assert [s for s, _ in seams] == lay.seams()  # every seam strictly inside an iteration
        assert all(p == "fast" for _, p in seams), (depth, seams)


@pytest.mark.parametrize("depth", DEPTHS)
def test_table_c_seams_lie_in_multi_iterations(depth):
    lay = T.table_c()
    for grid, order in LAUNCHES:
        seams = _with_seam(lay, T.classified(lay, depth, grid, order))
        assert seams and all(p == "multi" for _, p in seams), (depth, seams)
        # the seams of the last, partial iteration aside, every seam is in one
        full = (lay.n // 4) // (T.K_BLOCK * depth) * (T.K_BLOCK * depth)
        assert [s for s, _ in seams] == [s for s in lay.seams() if s < full]
        assert len(seams) >= 4
