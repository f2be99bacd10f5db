"""The directed cases of the workgroup-window build (tests/own_cases.py), checked without a GPU. own_plan, the restatement
of phase A, is the reference of test_gpu_own_window.py; its own check is here, all integers and no tolerance: the blocks it
says phase A writes, plus its deferred entries finished one after the other, must be the sequential oracle's table and
conflicts -- for either way the contested claims can go. Every constructor must then produce the property it is named for,
judged from the plan: the in / out twins differ in exactly the tuples the case moved, each cause shows a count in the out
twin and none in the in twin. Sizes come from hj_own_layout_info without a context."""
import ctypes

import numpy as np
import pytest

import htm_hashjoin_amd as hj
import own_cases as oc
from oracle import oracle


def test_layout_call_is_pinned():
    """host-only arithmetic: chunks of whole sample tiles that cover the relation, at most two per compute unit; the
    constants hang together the way the kernel uses them; argument errors"""
    for cu in (1, 64, 104, 256, 304):
        for n in (1, 4095, 1 << 14, (1 << 14) + 1, 1 << 15, 1 << 16, 1 << 20, 1 << 22, (1 << 27) + 5, 1 << 30, (1 << 32) - 1):
            lay = oc.layout(n, cu)
            assert lay["computeUnits"] == cu
            assert lay["nChunks"] * lay["chunkLen"] >= n > (lay["nChunks"] - 1) * lay["chunkLen"]
            assert lay["nChunks"] <= 2 * cu and lay["chunkLen"] % 4096 == 0 and lay["chunkLen"] >= 16384
            assert lay["tileTuples"] % 64 == 0 and lay["tileTuples"] % lay["blockSlots"] == 0
            assert lay["minTableSlots"] == lay["windowBlocks"] * lay["blockSlots"]
            assert lay["backBlocks"] < lay["windowBlocks"] and lay["windowBlocks"] & (lay["windowBlocks"] - 1) == 0
            # a tile of sorted keys in a table of twice as many slots fits the window behind the back blocks
            assert 2 * lay["tileTuples"] <= (lay["windowBlocks"] - lay["backBlocks"]) * lay["blockSlots"]
            assert lay["maxProbeLength"] == lay["blockSlots"] + 1
            assert lay["deferredParts"] == max(1, 4096 // lay["nChunks"])
    # what the case table is built on: 1, 2 and 4 chunks; a slice of phase B is walked more than once only from 2^21 on
    assert [oc.layout(n)["nChunks"] for n in (oc.N1, oc.N2, oc.N4)] == [1, 2, 4]
    lay = oc.layout(oc.N1)
    assert (lay["tileTuples"], lay["blockSlots"], lay["windowBlocks"], lay["backBlocks"], lay["seamDivisor"]) == (3072, 512, 16, 2, 4)
    for n, passes in ((1 << 20, 1), (1 << 21, 2), (1 << 22, 4)):          # 256 threads per workgroup of phase B
        lay = oc.layout(n)
        assert -(-lay["chunkLen"] // (lay["deferredParts"] * 256)) == passes
    out = (ctypes.c_uint64 * 16)()
    assert hj.lib.hj_own_layout_info(None, 0, 1 << 16, out) == hj.HJ_ERR_INVALID           # neither a context nor a count
    assert hj.lib.hj_own_layout_info(None, 256, 1 << 32, out) == hj.HJ_ERR_INVALID
    assert hj.lib.hj_own_layout_info(None, 256, 0, out) == hj.HJ_ERR_INVALID
    assert hj.lib.hj_own_layout_info(None, 256, 1 << 16, None) == hj.HJ_ERR_INVALID
    assert hj.lib.hj_own_layout_info(None, 256, 1 << 16, out) == hj.HJ_OK and list(out[11:]) == [0] * 5


def test_own_info_refuses_a_null_context():
    buf = np.zeros(4, dtype=np.uint32)
    out = (ctypes.c_uint64 * 4)()
    assert hj.lib.hj_own_info(None, buf.ctypes.data, 4, buf.ctypes.data, 4, out) == hj.HJ_ERR_INVALID


def test_plan_by_hand():
    """the restatement on a relation small enough to follow: one chunk, sorted dense homes from block 4 on"""
    lay = oc.layout(oc.N1)
    ts = 2 * oc.N1
    plan = oc.own_plan(oc.relation(oc.base_dense(oc.N1, 4 * 512), ts), lay, ts)
    # six tiles; tile t's homes start at block 4 + 6 t, the window two blocks below. Block 36 holds nothing and is wanted
    # all the same: the walks of the last three slots of block 35 could straddle into it
    assert plan.windows == [[2, 8, 14, 20, 26, 32]] and plan.wanted == [list(range(4, 37))] and not plan.contested
    o = plan.outcome(0)
    assert (o.deferred, o.drops, o.used_lo, o.used_hi1) == ([], [], 4, 37)
    assert plan.valid_range([o]) == (4 * 512, 38 * 512)
    # the same relation descending: the first tile places the window, which never moves back -- its own 3072 tuples and the
    # 1024 in the two back blocks go in, the rest is deferred where it is homed
    plan = oc.own_plan(oc.defer_all(oc.N1), lay, ts)
    o = plan.outcome(0)
    assert len(set(plan.windows[0])) == 1 and len(o.deferred) == oc.N1 - 3072 - 2 * 512 and not o.drops
    assert all(pos == (key & (ts - 1)) for pos, key, _ in o.deferred)


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name)
def test_plan_is_the_oracles_table(case):
    """phase A's blocks + the deferred entries finished sequentially = the sequential build, whoever wins the contested
    claims; and the case sits where it says"""
    plan = oc.plan_of(case)
    if case.htm:
        want = oracle.htm_build_probe_seq(case.rel, None, want_buckets=True)
        assert 4 * want["numBuckets"] == case.table_size
    else:
        want = oracle.build_probe_seq_ts(case.rel, None, case.table_size, case.shift, case.probe, want_table=True)
    for pick in (oc.first_wanter, oc.last_wanter):
        outs = plan.assignment(pick)
        table, slots, drops = plan.finish(outs)
        if case.htm:
            tuples, count, chains = oc.htm_view(slots, drops, want["numBuckets"])
            assert np.array_equal(tuples, want["buckets"]["tuples"]) and np.array_equal(count, want["buckets"]["count"])
            assert chains == oc.oracle_htm_chains(want)
            assert (len(drops), sum(k for k, _ in drops)) == (want["conflictCount"], want["conflictSum"])
        else:
            assert np.array_equal(table, want["table"])
            assert (len(drops), sum(k for k, _ in drops)) == (want["conflicts"], want["conflictSum"])
        # every tuple ends somewhere, once
        assert len(slots) + len(drops) == case.n
        if case.cause is not None:
            assert oc.moved_deferred(case, outs) == case.cause, case.aim
    if case.total is not None:
        assert sum(plan.bounds(c)[0] for c in range(plan.n_chunks)) == case.total, case.aim
    if not plan.contested:
        assert all(lo == hi for lo, hi in (plan.bounds(c) for c in range(plan.n_chunks)))


TWINS = [c for c in oc.CASES if c.twin and c.cause == 0]


@pytest.mark.parametrize("case", TWINS, ids=lambda c: f"{c.name}/{c.twin}")
def test_twins_straddle_their_boundary(case):
    """the in twin defers none of its moved tuples; the out twin defers what the in twin does plus exactly `cause` of its
    moved tuples, nothing else"""
    twin = oc.BY_NAME[case.twin]
    assert twin.twin == case.name and twin.cause > 0 and (case.n, case.probe, case.htm) == (twin.n, twin.probe, twin.htm)
    differ = int(np.count_nonzero(case.rel != twin.rel))
    assert differ == (1 if case.family in ("window", "quarter", "htm") else len(case.moved))       # one tuple, or one block for all moved
    a = {d[2] for o in oc.plan_of(case).assignment(oc.first_wanter) for d in o.deferred}
    b = {d[2] for o in oc.plan_of(twin).assignment(oc.first_wanter) for d in o.deferred}
    assert a <= b and not a & set(case.moved)
    assert b - a <= set(twin.moved) and len(b - a) == twin.cause


def test_what_the_families_are_aimed_at():
    """the geometry each family leans on, from the plan of its cases"""
    lay = oc.layout(oc.N1)
    blk, win = lay["blockSlots"], lay["windowBlocks"]
    # slides: the window bases of chunk 0's tiles 1 and 2 differ by the case's number; nothing is lost over it
    for d in (15, 16, 17, 40):
        plan = oc.plan_of(oc.BY_NAME[f"slide_{d}"])
        assert plan.windows[0][2] - plan.windows[0][1] == d and plan.bounds(0) == (0, 0)
    # the table's end: the clamp holds the window for the last three tiles; the deferred walks wrapped to slot 0, and the
    # valid range is the whole table
    plan = oc.plan_of(oc.BY_NAME["table_end"])
    nb = plan.geo["numBlocks"]
    assert plan.windows[0][-3:] == [nb - win] * 3
    outs = plan.assignment(min)
    assert [d[0] for d in outs[0].deferred] == [0, 0] and plan.valid_range(outs) == (0, plan.geo["tableSize"])
    # straddle: the deferred pair of straddle_last waits at the first slot past the window
    plan = oc.plan_of(oc.BY_NAME["straddle_last"])
    wb = plan.windows[0][2]
    assert [d[0] for d in plan.outcome(0).deferred] == [(wb + win) * blk] * 2
    # look: the moved tuple is dropped, eight slots on, in the next block for the two that start at the block's end
    for name, crosses in (("look_508", True), ("look_509", True), ("skip4_recheck", False)):
        case = oc.BY_NAME[name]
        o = oc.plan_of(case).outcome(0)
        (key, idx), = o.drops
        assert idx == case.moved[0]
        home = key & (case.table_size - 1)
        assert ((home + 7) // blk != home // blk) == crosses
    # contested seam: every inner seam block has its two neighbours as wanters
    plan = oc.plan_of(oc.BY_NAME["contested_seam"])
    assert sorted(plan.contested) == [32, 64, 96] and all(plan.wanters[b] == [b // 32 - 1, b // 32] for b in plan.contested)
    assert [plan.bounds(c) for c in range(4)] == [(0, 256), (0, 512), (0, 512), (0, 256)]
    # early stragglers: deferred at their home slots, which chunk 1 owns; phase B has to displace what chunk 1 stored
    for probe in (1, 2, 4, 8):
        case = oc.BY_NAME[f"early_straggler_p{probe}"]
        plan = oc.plan_of(case)
        outs = plan.assignment(min)
        homes = {d[0] for d in outs[0].deferred}
        assert len(homes) == 100 and all(outs[1].slots[h] >> 32 >= oc.layout(case.n)["chunkLen"] for h in homes)
        assert len(plan.finish(outs)[2]) > len(outs[0].drops) + len(outs[1].drops)          # drops at budget end in phase B
    # the bucketised table: phase A lists conflicts, and phase B makes more of them out of stored tuples
    plan = oc.plan_of(oc.BY_NAME["htm_bucket_full"])
    assert len(plan.outcome(0).drops) >= 3
    plan = oc.plan_of(oc.BY_NAME["htm_deferred_conflicts"])
    outs = plan.assignment(min)
    assert len(plan.finish(outs)[2]) - len(outs[0].drops) >= 4
    plan = oc.plan_of(oc.BY_NAME["htm_contested_seam"])
    (b,) = plan.contested
    assert plan.wanters[b] == [0, 1] and [plan.bounds(c) for c in range(2)] == [(64, 256), (64, 256)]
    plan = oc.plan_of(oc.BY_NAME["htm_early_straggler"])
    assert not plan.contested and {d[2] for d in plan.outcome(0).deferred} == set(oc.BY_NAME["htm_early_straggler"].moved)
    # duplicates: the two long runs really cross a tile end inside a chunk / a chunk end
    lay2 = oc.layout(oc.N2)
    tl, cl = lay2["tileTuples"], lay2["chunkLen"]
    mv = oc.BY_NAME["dup_across_tile"].moved
    assert mv[0] // tl + 1 == mv[-1] // tl and mv[0] // cl == mv[-1] // cl and mv[0] % tl and (mv[-1] + 1) % tl
    mv = oc.BY_NAME["dup_across_chunk"].moved
    assert mv[0] // cl + 1 == mv[-1] // cl and mv[0] % cl and (mv[-1] + 1) % cl
    for name, k in (("dup_64", 64), ("dup_65", 65), ("dup_tile", tl), ("dup_tile_plus_1", tl + 1)):
        assert len(oc.BY_NAME[name].moved) == k
    # duplicates: the runs drop all but probeLength copies
    for name, k in (("dup_64", 64), ("dup_65", 65), ("dup_tile", 3072), ("dup_tile_plus_1", 3073)):
        plan = oc.plan_of(oc.BY_NAME[name])
        assert len(plan.finish(plan.assignment(min))[2]) == k - 4
