"""R-side match marks on the resident radix join (HJ_FLAG_TRACK_R_MATCHES with hj_prj_build_dev / hj_prj_probe_join_dev,
hj_r_rows_dev) through ctypes -> C ABI on an MI355X. As in test_gpu_r_marks.py the expected rows come from numpy alone:
the inner pairs of the complete equi-join on the key word (r_marks_common.join_expected), the matched R rows -- positions
in the relation given to the build -- as their unique R words. Every probe call goes through join_kinds_common.Calls
(rows, hj_pairs_info, totalMatches and sSize as without the flag). Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from gpu_harness import Device, ctx, status  # noqa: F401
import prj_cases as pc

from r_marks_common import (SENTINEL, GUARD, U64, INNER, LEFT, SEMI, ANTI, UNMATCHED, MATCHED, SWEEP_ROWS, SCAN_TILE, Calls,
                            Marks, inner_expected, r_rows_of)

pytestmark = pytest.mark.gpu

PAIR_BLOCK_TUPLES = 11520        # kPairBlockTuples: R tuples of one LDS build of the pairs join
STAGE = 4096                     # kStagePairs: rows per stage
ROUND = 2 * 1024                 # kPairElems * kJoinThreads: S elements of one round of a workgroup


def expected(R, S, s_base=0):
    return inner_expected("prj", R, S, s_base=s_base)


def tracked(ctx, dev, R, s_max, bits=0):
    """reserve with both flags, build R -> (dR, Calls, Marks)"""
    ctx.reserve("prj", R.size, max(s_max, 1), radixBits=bits, keepRowIds=True, trackRMatches=True)
    dR = dev.put(R)
    ctx.prj_build(dR, R.size)
    return dR, Calls(ctx, dev, ctx.prj_probe_pairs), Marks(ctx, dev, R.size)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_last_word_of_the_plane(ctx, n):
    R = np.arange(1, n + 1, dtype=U64)
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, 2 * n)
        marks.check((n, "no probe"))
        for S in (np.concatenate([R[::2], R[:1] + U64(5000)]), R):
            inner = expected(R, S, s_base=4242)                          # a non-zero sIdxBase must not leak into R rows
            calls.call(INNER, dev.put(S), S.size, inner, s_base=4242, tag=n)
            marks.add(inner)
            marks.check((n, S.size))
        assert marks.expected(UNMATCHED).size == 0 and marks.expected(MATCHED).size == n


def test_marks_accumulate_over_inner_and_left_slices_only(ctx):
    n = 1 << 12
    R = pc.unique_shuffled(n, 3)
    keys = np.arange(1, 2 * n + 1, dtype=U64)
    slices = [keys[0:900], keys[1000:1700], keys[2500:3001]]             # INNER, LEFT, INNER
    other = np.concatenate([keys[3200:3900], keys[n + 5: n + 50]])       # SEMI, ANTI, counting: rows no slice above names
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, 1024)
        d_other, inner_other = dev.put(other), expected(R, other)
        assert inner_other.size > 0
        off = 0
        for step, (kind, S) in enumerate(zip((INNER, LEFT, INNER), slices)):
            inner = expected(R, S, s_base=off)
            assert not np.isin(r_rows_of(inner), marks.seen).any() and inner.size > 0
            calls.call(kind, dev.put(S), S.size, inner, s_base=off, tag=step)
            marks.add(inner)
            marks.check(step)
            off += S.size
            if step == 0:
                calls.call(SEMI, d_other, other.size, inner_other, tag="semi")
            elif step == 1:
                calls.call(ANTI, d_other, other.size, inner_other, tag="anti")
            else:
                before = ctx.pairs_info()
                ctx.prj_probe(d_other, other.size)                       # the counting probe of a rows context
                calls.matches += inner_other.size
                calls.s += other.size
                got = ctx.fetch()
                assert (got["totalMatches"], got["sSize"]) == (calls.matches, calls.s)
                assert ctx.pairs_info()[:2] == before[:2]
            marks.check((step, "after a call that does not mark"))
        assert not np.isin(r_rows_of(inner_other), marks.seen).any()


def test_rows_cut_by_the_capacity_mark_too(ctx):
    n = 1 << 13
    R = pc.uniform(n, n // 4, 5)                                         # ~4 rows per key
    S = pc.uniform(n - 7, n // 2, 6)
    inner = expected(R, S)
    assert inner.size > S.size
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, S.size)
        dS = dev.put(S)
        marks.add(inner)
        calls.count_only(INNER, dS, S.size, inner.size, np.unique(inner >> U64(32)).size, tag="capacity 0")
        marks.check("capacity 0, NULL planes")
        for kind, capacity in ((INNER, inner.size // 3), (LEFT, 1)):
            ctx.r_marks_clear()
            calls.call(kind, dS, S.size, inner, capacity=capacity, tag=capacity)
            marks.check(("capacity", capacity))


def test_an_r_partition_of_several_lds_builds(ctx):
    """one key 30 000 times: its partition takes three LDS builds, and one S tuple with that key names every one of those
    rows; the rows of the other keys S holds are marked, the rest is not"""
    hot = U64(123457)
    R = pc.shuffled([np.arange(1, 4097, dtype=U64), np.full(30000, hot, dtype=U64)], 7)
    assert 30000 > 2 * PAIR_BLOCK_TUPLES
    S = np.concatenate([np.arange(1, 2049, dtype=U64)[::2], np.array([hot, 999999], dtype=U64)])
    inner = expected(R, S)
    assert inner.size == 1024 + 30000
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, S.size)
        calls.call(INNER, dev.put(S), S.size, inner, tag="blocks")
        marks.add(inner)
        marks.check("blocks")


@pytest.mark.parametrize("full_capacity", [True, False])
def test_the_direct_write_round_marks(ctx, full_capacity):
    """duplicate keys on both sides: 64 keys, 40 times each in R, and an S of 2^12 draws from them: a round of 2048 S
    elements has 40 rows per element, far more than a stage holds, so it claims its run and writes straight to the planes.
    Those rows mark in the `put` of that round -- with the planes there, and with capacity 0."""
    keys = pc.hot_keys(5, 14, 1, 64)                                     # one partition at the engine's 14 bits
    R = pc.shuffled([np.repeat(keys, 40), np.arange(1, 1025, dtype=U64) << U64(3)], 8)
    S = pc.shuffled([keys[pc.uniform(1 << 12, 32, 9).astype(np.int64) - 1], np.array([7, 8, 16], dtype=U64)], 10)
    inner = expected(R, S)
    assert inner.size >= 40 * (1 << 12) and 40 * ROUND > STAGE
    rows = r_rows_of(inner)
    assert 32 * 40 <= rows.size < R.size                                 # 32 of the 64 keys are drawn, and key 8 and 16
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, S.size)
        dS = dev.put(S)
        if full_capacity:
            calls.call(LEFT, dS, S.size, inner, tag="direct")
        else:
            calls.count_only(LEFT, dS, S.size, inner.size, np.unique(inner >> U64(32)).size, tag="direct, capacity 0")
        marks.add(inner)
        marks.check(("direct", full_capacity))


def test_partitions_with_s_and_no_r_under_left(ctx):
    n = 1 << 14
    R = np.array([3, 700, 701, 5000, 9999, 12000, 16000, 16384], dtype=U64)
    S = pc.uniform(n, n, 1000, 11)
    inner = expected(R, S)
    assert 0 < inner.size < 64
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, S.size, bits=11)
        calls.call(LEFT, dev.put(S), S.size, inner, tag="r-less")
        marks.add(inner)
        marks.check("r-less")


def test_zipf_probe_marks_exactly(ctx):
    n = 1 << 12
    R = pc.unique_shuffled(n, 4)
    S = hj.generate_relation("zipf", 1 << 16, n, 0, 1.0, 54321)
    inner = expected(R, S)
    assert np.bincount((inner & U64(0xFFFFFFFF)).astype(np.int64)).max() > 3000 and r_rows_of(inner).size < n
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, S.size)
        calls.call(INNER, dev.put(S), S.size, inner, tag="zipf")
        marks.add(inner)
        marks.check("zipf")


def test_nothing_everything_and_clearing(ctx):
    n = 1 << 12
    R = pc.unique_shuffled(n, 5)
    absent = np.arange(3 * n, 4 * n - 3, dtype=U64)
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, n)
        marks.check("no probe at all")
        calls.call(LEFT, dev.put(absent), absent.size, expected(R, absent), tag="nothing")
        marks.check("no S key in R")
        every = expected(R, R)
        calls.call(INNER, dR, n, every, tag="everything")
        marks.add(every)
        assert marks.expected(UNMATCHED).size == 0
        marks.check("every row matched")
        marks.check("the same rows twice in a row")
        ctx.r_marks_clear()
        marks.clear()
        marks.check("after hj_r_marks_clear")
        calls.call(INNER, dR, n // 2, expected(R, R[: n // 2]), tag="half")
        marks.add(expected(R, R[: n // 2]))
        marks.check("half")
        ctx.prj_build(dR, n)                                            # a rebuild on the same context
        marks.clear()
        marks.check("after a rebuild")


def test_sweep_of_several_blocks(ctx):
    n = 100003
    assert n > 12 * SWEEP_ROWS and n % 32
    rng = np.random.default_rng(20261019)
    R = rng.permutation(np.arange(1, n + 1, dtype=U64))
    S = np.arange(1, n + 1, dtype=U64)[rng.random(n) < 0.25]
    inner = expected(R, S)
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, S.size)
        calls.count_only(INNER, dev.put(S), S.size, inner.size, S.size)
        marks.add(inner)
        marks.check("100003")
        want = marks.expected(UNMATCHED)
        capacity = int((want < 3 * SWEEP_ROWS).sum()) + 5                # cut inside the fourth workgroup's run
        produced, written, got = marks.sweep(UNMATCHED, capacity)          # no word behind the rows written: Marks.sweep
        assert (produced, written) == (want.size, capacity) and produced > written
        assert np.array_equal(got.astype(U64), want[:capacity])


def test_sweep_whose_block_counts_take_the_second_level_of_the_scan(ctx):
    """The sweep counts per workgroup of SWEEP_ROWS = 32 * kSweepWords = 8192 rows and scans those counts together with one
    word behind them, which ends as the total: blocks + 1 entries. launch_exclusive_scan_u32 works in tiles of kScanTile =
    4096 entries and needs its second level (the scan of the tile sums, added back) from 4097 entries on, i.e. from 4096
    workgroups on: the smallest rSize is 4095 * 8192 + 1 = 33 546 241 rows (below 2^26). Rows of workgroups behind the
    first tile are probed, so that their places in the output depend on the second level."""
    n = (SCAN_TILE - 1) * SWEEP_ROWS + 1
    assert (n + SWEEP_ROWS - 1) // SWEEP_ROWS + 1 == SCAN_TILE + 1 and n < 1 << 26
    R = np.arange(1, n + 1, dtype=U64)                                   # key k is row k - 1
    rows = np.unique(np.concatenate([np.arange(0, n, 7919, dtype=U64), np.array([SWEEP_ROWS - 1, n - SWEEP_ROWS - 1, n - 2, n - 1], dtype=U64)]))
    S = rows + U64(1)
    inner = (np.arange(S.size, dtype=U64) << U64(32)) | rows             # S is sorted and unique: S row i names R row rows[i]
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, R, S.size)
        calls.call(INNER, dev.put(S), S.size, inner, tag="second level")
        marks.seen = rows
        produced, written, got = marks.sweep(MATCHED, rows.size + 64)
        assert (produced, written) == (rows.size, rows.size)
        assert np.array_equal(got.astype(U64), rows)
        assert marks.sweep(UNMATCHED, 0, null_plane=True)[:2] == (n - rows.size, 0)
        produced, written, got = marks.sweep(UNMATCHED, n)
        assert (produced, written) == (n - rows.size, n - rows.size)
        assert np.array_equal(got, np.delete(np.arange(n, dtype=np.uint32), rows.astype(np.int64)))


def test_errors():
    n = 1 << 10
    R = np.arange(1, n + 1, dtype=U64)
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        dR = dev.put(R)
        d_rows = dev.put(np.full(n + GUARD, SENTINEL, dtype=np.uint32))
        for algo in ("prj", "auto"):                                    # the flag without the row ids: refused at hj_reserve
            assert status(c.reserve, algo, n, n, trackRMatches=True) == _lib.HJ_ERR_INVALID
        c.reserve("prj", n, n, keepRowIds=True)                         # reserved without the flag
        c.prj_build(dR, n)
        assert status(c.r_rows, UNMATCHED, d_rows, n) == _lib.HJ_ERR_STATE
        assert status(c.r_marks_clear) == _lib.HJ_ERR_STATE
        c.reserve("prj", n, n, keepRowIds=True, trackRMatches=True)
        assert status(c.r_rows, UNMATCHED, d_rows, n) == _lib.HJ_ERR_STATE      # that R was built without marks
        c.prj_build(dR, n)
        assert status(c.r_rows, 2, d_rows, n) == _lib.HJ_ERR_INVALID
        assert status(c.r_rows, MATCHED, 0, 1) == _lib.HJ_ERR_INVALID
        c.r_rows(MATCHED, d_rows, n)
        assert c.r_rows_info()[:2] == (0, 0) and c.r_rows_info()[3] == n
        assert (dev.get(d_rows, n + GUARD) == SENTINEL).all()
        dS = dev.put(R)
        c.prj_join(dR, n, dS, n)                                        # the one-shot join: the last build is no longer hj_prj_build_dev
        assert status(c.r_rows, UNMATCHED, d_rows, n) == _lib.HJ_ERR_STATE


def test_radix_outer_join_pairs_end_to_end():
    """2^12 x 2^12 in slices of 1500: half of S is absent from R, a quarter of R is not probed"""
    n = 1 << 12
    R = pc.unique_shuffled(n, 6)
    keys = np.concatenate([np.arange(1, 3 * n // 4 + 1, dtype=U64)[::2], np.arange(2 * n + 1, 2 * n + n // 2 + 1, dtype=U64)])
    S = np.random.default_rng(7).permutation(np.concatenate([keys, keys[: n - keys.size]]))
    inner = expected(R, S)
    matched = r_rows_of(inner)
    unmatched = np.setdiff1d(np.arange(n, dtype=U64), matched, assume_unique=True)
    s_matched = np.unique(inner >> U64(32))
    assert unmatched.size >= n // 4 and s_matched.size == n // 2
    left = np.sort(np.concatenate([inner, (np.setdiff1d(np.arange(n, dtype=U64), s_matched) << U64(32)) | U64(hj.NO_ROW)]))
    for how, head, tail in (("right", inner, unmatched), ("full", left, unmatched)):
        s_idx, r_idx = hj.radix_outer_join_pairs(R, S, slice_tuples=1500, how=how)
        assert s_idx.dtype == r_idx.dtype == np.uint32 and s_idx.size == r_idx.size == head.size + tail.size
        k = head.size
        assert np.array_equal(np.sort((s_idx[:k].astype(U64) << U64(32)) | r_idx[:k]), head), how
        assert (s_idx[k:] == hj.NO_ROW).all() and np.array_equal(r_idx[k:].astype(U64), tail), how
    for how, want in (("right_semi", matched), ("right_anti", unmatched)):
        s_idx, r_idx = hj.radix_outer_join_pairs(R, S, slice_tuples=1500, how=how)
        assert s_idx is None and r_idx.dtype == np.uint32 and np.array_equal(r_idx.astype(U64), want), how
