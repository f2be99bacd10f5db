"""hj_pairs_agg_dev -- the reduction over a pair list -- against numpy (np.add.at, np.minimum.at, np.maximum.at). The
accumulators are the caller's: every one is prefilled (identity, or a running value) and has guard words behind it."""
import numpy as np
import pytest

from htm_hashjoin_amd import _lib
from gpu_harness import Device, ctx, status  # noqa: F401
from join_kinds_common import planes
import prj_cases as pc
from agg_common import COUNT, SUM, MIN, MAX, SIGNED, U64, Col, expected, get64, put64
from r_marks_common import inner_expected

pytestmark = pytest.mark.gpu
NO_ROW = 0xFFFFFFFF


def vals(dtype, n, seed):
    info = np.iinfo(dtype)
    v = np.random.default_rng([20261020, seed]).integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
    v[::5] = info.max
    return v


def run(ctx, map_g, map_v, g_rows, v_rows, cols, g_base=0, v_base=0, tag=None, null_v=False, skipped=0, want_pairs=None):
    """one hj_pairs_agg_dev over the two maps (raw entries, bases included) -> checked against numpy over want_pairs
    (default: every pair, bases off)"""
    map_g, n = np.ascontiguousarray(map_g, dtype=np.uint32), len(map_g)
    with Device(ctx) as dev:
        d_g = dev.put(map_g)
        d_v = 0 if null_v else dev.put(np.ascontiguousarray(map_v, dtype=np.uint32))
        d_acc = [put64(dev, g_rows, c.identity) for c in cols]
        d_cnt = put64(dev, g_rows, U64(0))
        args = []
        for c, d in zip(cols, d_acc):
            w = c.words()
            args.append((dev.put(c.poisoned()) if c.op != COUNT else 0, dev.put(w) if w is not None else 0, d) + c.spec)
        ctx.pairs_agg(d_g, d_v, n, g_base, g_rows, v_base, v_rows, args, d_cnt)
        info = ctx.pairs_agg_info()
        assert info[0] == n and info[1] == n - skipped and info[3] == skipped, (tag, info)
        g, v = want_pairs if want_pairs is not None else (map_g.astype(np.int64) - g_base, np.asarray(map_v, dtype=np.int64) - v_base)
        want_count, want = expected(g_rows, g, v, cols)
        assert np.array_equal(get64(ctx, d_cnt, g_rows, tag), want_count), (tag, "count")
        for i, (d, w) in enumerate(zip(d_acc, want)):
            got = get64(ctx, d, g_rows, tag)
            assert np.array_equal(got, w), (tag, "column", i, cols[i].spec, np.flatnonzero(got != w)[:8])


def four(v64, v32, valid=None):
    return [Col(SUM, v64, valid), Col(MIN, v32), Col(MAX, v64), Col(COUNT, v64, valid)]


def test_maps_of_the_radix_join_in_both_directions(ctx):
    n = 1 << 12
    R, S = pc.uniform(n, n // 2, 1), pc.uniform(3 * n, n // 2 + 50, 2)
    inner = inner_expected("prj", R, S)
    with Device(ctx) as dev:
        ctx.reserve("prj", n, S.size, keepRowIds=True)
        ctx.prj_build(dev.put(R), n)
        cap = inner.size + 64
        d_s, d_r = (p.ptr for p in planes(dev, cap))
        ctx.prj_probe_pairs(dev.put(S), S.size, d_s, d_r, cap)
        assert ctx.pairs_info()[0] == inner.size
        map_s, map_r = dev.get(d_s, inner.size), dev.get(d_r, inner.size)
    assert np.array_equal(np.sort((map_s.astype(U64) << U64(32)) | map_r.astype(U64)), inner)
    valid = np.random.default_rng(3).random(S.size) > 0.3
    run(ctx, map_r, map_s, n, S.size, four(vals(np.int64, S.size, 4), vals(np.int32, S.size, 5), valid), tag="group by R")
    run(ctx, map_s, map_r, S.size, n, four(vals(np.int64, n, 6), vals(np.int32, n, 7)), tag="group by S")


@pytest.mark.parametrize("run_len", [1, 63, 64, 65, 4097])
def test_run_lengths(ctx, run_len):
    groups = 37
    map_g = np.repeat(np.random.default_rng(run_len).permutation(groups), run_len).astype(np.uint32)
    map_g = np.concatenate([map_g[:5], map_g])                 # runs that do not start on a wavefront's first lane
    n = map_g.size
    map_v = np.random.default_rng(run_len + 1).integers(0, 1000, n).astype(np.uint32)
    valid = np.random.default_rng(run_len + 2).random(1000) > 0.5
    run(ctx, map_g, map_v, groups, 1000, four(vals(np.int64, 1000, 8), vals(np.int32, 1000, 9), valid), tag=("run", run_len))


def test_one_group_and_two_alternating(ctx):
    n = 1 << 16
    map_v = np.random.default_rng(11).integers(0, 5000, n).astype(np.uint32)
    cols = four(vals(np.int64, 5000, 10), vals(np.int32, 5000, 11))
    run(ctx, np.full(n, 2, dtype=np.uint32), map_v, 4, 5000, cols, tag="one group")
    run(ctx, (np.arange(n) & 1).astype(np.uint32) * 3, map_v, 4, 5000, cols, tag="alternating")


def test_null_and_out_of_range_entries_are_skipped_and_counted(ctx):
    n, g_rows, v_rows, g_base, v_base = 10000, 300, 700, 1000, 50
    rng = np.random.default_rng(12)
    map_g = (rng.integers(0, g_rows, n) + g_base).astype(np.uint32)
    map_v = (rng.integers(0, v_rows, n) + v_base).astype(np.uint32)
    bad = rng.permutation(n)[:800].reshape(8, 100)
    map_g[bad[0]] = NO_ROW; map_v[bad[1]] = NO_ROW
    map_g[bad[2]] = g_base + g_rows; map_v[bad[3]] = v_base + v_rows          # the first row behind the range
    map_g[bad[4]] = g_base - 1; map_v[bad[5]] = v_base - 1                    # below the base: wraps to a huge row
    map_g[bad[6]] = 0xFFFFFFFE; map_v[bad[7]] = 0xFFFFFFFE
    live = np.ones(n, dtype=bool)
    live[bad.ravel()] = False
    want = (map_g[live].astype(np.int64) - g_base, map_v[live].astype(np.int64) - v_base)
    cols = four(vals(np.int64, v_rows, 13), vals(np.int32, v_rows, 14), rng.random(v_rows) > 0.4)
    run(ctx, map_g, map_v, g_rows, v_rows, cols, g_base, v_base, tag="skipped", skipped=800, want_pairs=want)


def test_count_only_without_a_value_map(ctx):
    n = 5000
    map_g = np.sort(np.random.default_rng(15).integers(0, 64, n)).astype(np.uint32)
    map_g[::97] = NO_ROW
    live = map_g != NO_ROW
    want = (map_g[live].astype(np.int64), np.zeros(int(live.sum()), dtype=np.int64))
    run(ctx, map_g, None, 64, 0, [Col(COUNT)], tag="count only", null_v=True, skipped=int((~live).sum()), want_pairs=want)
    run(ctx, map_g, None, 64, 0, [], tag="dCount alone", null_v=True, skipped=int((~live).sum()), want_pairs=want)


def test_argument_errors(ctx):
    INVALID = _lib.HJ_ERR_INVALID
    with Device(ctx) as dev:
        d_map, d_src, d_acc = dev.put(np.zeros(64, dtype=np.uint32)), dev.put(np.zeros(64, dtype=np.int64)), put64(dev, 64, U64(0))
        ok = (d_src, 0, d_acc, SUM, 8, SIGNED)
        ctx.pairs_agg(d_map, d_map, 64, 0, 64, 0, 64, [ok])
        ctx.pairs_agg(d_map, d_map, 0, 0, 64, 0, 64, [ok])                   # no pairs: a call that applied nothing
        assert ctx.pairs_agg_info()[:2] == (0, 0)
        for bad in ([ok] * 5, [(d_src, 0, d_acc, 4, 8, 0)], [(d_src, 0, d_acc, SUM, 2, 0)], [(d_src, 0, d_acc, COUNT, 8, 0)],
                    [(d_src, 0, d_acc, SUM, 8, 2)], [(d_src, 0, d_acc, SUM, 8, 0, 1)], [(d_src, 0, 0, SUM, 8, 0)],
                    [(d_src, 0, d_acc + 4, SUM, 8, 0)], [(0, 0, d_acc, SUM, 8, 0)], [(d_src + 4, 0, d_acc, SUM, 8, 0)],
                    [(d_src, d_src + 2, d_acc, SUM, 8, 0)]):
            assert status(ctx.pairs_agg, d_map, d_map, 64, 0, 64, 0, 64, bad) == INVALID, bad
        assert status(ctx.pairs_agg, 0, d_map, 64, 0, 64, 0, 64, [ok]) == INVALID                 # dMapG NULL
        assert status(ctx.pairs_agg, d_map, 0, 64, 0, 64, 0, 64, [ok]) == INVALID                 # dMapV NULL, a column reads values
        assert status(ctx.pairs_agg, d_map, d_map, 64, 0, 64, 0, 64, []) == INVALID               # neither a column nor dCount
        assert status(ctx.pairs_agg, d_map, d_map, 64, 0, 64, 0, 64, [ok], d_acc + 4) == INVALID
        assert status(ctx.pairs_agg, d_map, d_map, 1 << 32, 0, 64, 0, 64, [ok]) == INVALID
        assert status(ctx.pairs_agg, d_map, d_map, 64, 0, 1 << 32, 0, 64, [ok]) == INVALID
