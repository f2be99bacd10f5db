"""The LDS chain phase of the bucketised table (HJ_ALGO_HTM behind buildVariant 3: k_htm_chain_count / k_htm_chain_fill and
the router of the deferred phase) on the directed cases of htm_chain_cases.py. For every case: the phase reports the state
and the cause that chain_plan -- evaluated on the device's own seams -- predicts; hj_result.compactFallback bit 8 agrees;
and whether the phase held or handed over to the generic chain kernels, every counter, the primary buckets tuple for tuple
and every chain in walk order are the sequential oracle's. No tolerance anywhere."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from gpu_harness import ctx  # noqa: F401
import htm_chain_cases as cc
from htm_chain_device import run_case, run_relation

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", cc.ONE_PART, ids=lambda c: c.name)
def test_one_part_cases(ctx, case):
    assert ctx.htm_chain_layout_info(cc.SMALL)["parts"] == 1
    run_case(ctx, case, cc.SMALL)


@pytest.mark.parametrize("case", cc.TWO_PARTS, ids=lambda c: c.name)
def test_two_part_cases(ctx, case):
    n = cc.smallest_n_with_parts(2, None, below=1 << 25, ctx=ctx)
    if n is None:
        pytest.skip("this device's compute units give no relation below 2^25 tuples whose slices have two parts")
    run_case(ctx, case, n)


def test_hold_hand_over_hold_on_one_context():
    """htmGenericChains / htmChainsFellBack and the saved cause mask belong to one build: a build that holds after one that
    handed over reports state 1, cause 0 and no bit 8, and the other way round"""
    with hj.HashJoinContext(0) as c:
        seen = []
        for name in ("tail_counts", "slice_over", "image_at_cap", "sub_over_cap", "image_over_cap", "empty_slices"):
            plan, info, got = run_case(c, cc.BY_NAME[name], cc.SMALL)
            seen.append((info["state"], info["cause"], got["compactFallback"] & 0x100))
        assert seen == [(1, 0, 0), (2, cc.BIT_SLICE_FULL, 0x100), (1, 0, 0), (2, cc.BIT_SUB, 0x100), (2, cc.BIT_IMAGE, 0x100), (1, 0, 0)]
        # another build variant on the same context after a hand-over: not tried, nothing left over
        R = cc.build_case(cc.BY_NAME["slice_over"], cc.SMALL, c.wave_layout_info(cc.SMALL), c.htm_chain_layout_info(cc.SMALL))[0]
        run_relation(c, R, "slice_over through 3", variant=3)
        run_relation(c, R, "slice_over through 2", variant=2)
        run_relation(c, R, "slice_over through 1", variant=1)


def test_where_the_rings_start_to_take_the_table_and_contexts_without_an_htm_table():
    """State 0. The issue's "n so small that the host rule does not try the phase" cannot be reached behind buildVariant 3:
    the scratch rule of build_htm (htm_chain_tries) fails only for tables of one or two buckets, and the rings need a table
    of one ring of slots (256 buckets), below which a request for 3 is settled to the window or to global atomics -- the
    rule guards two arrays and decides nothing (hj_htm_chain_layout_info reports the combined rule; the CPU suite pins
    both terms). What CAN be run is the real boundary: the largest n the rings refuse (not 3, state 0, bit 8 clear)
    against the smallest they take (3, the phase tried and held), on relations with duplicates, so that chains exist."""
    with hj.HashJoinContext(0) as c:
        with pytest.raises(hj.HashJoinError) as e:
            c.htm_chain_info()
        assert e.value.status == _lib.HJ_ERR_STATE
        below, first = cc.rings_boundary(ctx=c)
        for n, tries in ((below, 0), (first, 1), (5, 0)):
            R = cc.duplicates(n)
            assert c.htm_chain_layout_info(n)["tries"] == tries
            plan, info, got = run_relation(c, R, ("rings boundary", n))
            assert got["htmOverflowBuckets"] > 0 and got["compactFallback"] & 0x100 == 0, (n, got)
            if tries:
                assert got["buildVariant"] == 3 and info["state"] == cc.HELD and info["groups"] == got["htmOverflowBuckets"], (n, info)
            else:
                assert got["buildVariant"] in (1, 2) and info == {"state": 0, "cause": 0, "groups": 0}, (n, info, got)
        # an open-addressing table is no htm table
        c.run("atomic", np.arange(1, 1025, dtype=np.uint64), None)
        with pytest.raises(hj.HashJoinError) as e:
            c.htm_chain_info()
        assert e.value.status == _lib.HJ_ERR_STATE
