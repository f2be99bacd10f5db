"""The fused group-join of the resident radix join -- hj_prj_agg_begin / hj_prj_probe_agg_dev / hj_prj_agg_rows_dev -- against
numpy: np.add.at, np.minimum.at and np.maximum.at over the pairs r_marks_common.inner_expected("prj", ...) gives. Every
output plane is prefilled with a sentinel and has guard words behind it (agg_common.PrjAgg.rows). Everything is exact."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from gpu_harness import Device, ctx, status  # noqa: F401
from join_kinds_common import planes
import prj_cases as pc
from agg_common import COUNT, SUM, MIN, MAX, SIGNED, U64, Col, PrjAgg, expected_join, get64, put64
from r_marks_common import Marks, inner_expected

pytestmark = pytest.mark.gpu

I32_MIN, I64_MAX, U64_MAX = -(1 << 31), (1 << 63) - 1, (1 << 64) - 1


def resident(ctx, dev, R, s_max, bits=0, track=False):
    ctx.reserve("prj", R.size, max(s_max, 1), radixBits=bits, keepRowIds=True, trackRMatches=track)
    ctx.prj_build(dev.put(np.ascontiguousarray(R)), R.size)


def rng_of(*seed):
    return np.random.default_rng([20261019, *seed])


def values_of(dtype, n, *seed):
    """n random values of the type with its extremes sprinkled in: -1 and the minimum of a signed type, the maximum of any"""
    info, rng = np.iinfo(dtype), rng_of(*seed)
    v = rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
    v[::7] = info.max                                # often enough that a group's SUM passes 2^64
    if info.min < 0:
        v[1::11] = -1
        v[2::13] = info.min
    return v


def slices_of(S, lens):
    lo = 0
    for n in lens:
        yield lo, S[lo:lo + n]
        lo += n


def run_case(ctx, R, S, lens, cols, bits=0, tag=None, between=False):
    """build R, one aggregation of `cols`, S in slices of `lens`; the rows against numpy at the end (between: after every slice)"""
    with Device(ctx) as dev:
        resident(ctx, dev, R, max(lens), bits)
        agg = PrjAgg(ctx, dev, R.size, cols)
        for lo, part in slices_of(S, lens):
            agg.probe(part, lo)
            if between:
                seen = lo + part.size
                head = [Col(c.op, None if c.values is None else c.values[:seen], None if c.valid is None else c.valid[:seen]) for c in cols]
                agg.check(expected_join(R.size, inner_expected("prj", R, S[:seen]), head), (tag, "after", seen))
        inner = inner_expected("prj", R, S)
        agg.check(expected_join(R.size, inner, cols), tag)
        agg.check(expected_join(R.size, inner, cols), (tag, "again"))         # rows changes no accumulator
        info = ctx.prj_agg_info()
        assert info["nCols"] == len(cols) and info["probes"] == len(lens) and info["rows"] == R.size, info
        assert info["matches"] == inner_expected("prj", R, S[sum(lens[:-1]):]).size, info
        return inner


@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64, np.uint64])
def test_every_op_and_type_over_accumulating_slices(ctx, dtype):
    n = 1 << 12
    R = pc.unique_shuffled(n, 5)
    S = pc.uniform(5000, n + 500, 21)
    v = values_of(dtype, S.size, 1)
    if dtype == np.int32:
        assert (v == -1).any() and (v == I32_MIN).any()
    if dtype == np.int64:
        assert (v == I64_MAX).sum() > 500
    if dtype == np.uint64:
        assert (v == U64_MAX).any()
    cols = [Col(op, v) for op in (COUNT, SUM, MIN, MAX)]
    assert [c.spec[2] for c in cols[1:]] == [SIGNED if np.dtype(dtype).kind == "i" else 0] * 3
    inner = run_case(ctx, R, S, [1700, 1301, 1999], cols, tag=np.dtype(dtype).name, between=True)
    if dtype == np.int32:                            # -1 and INT32_MIN add as negatives: some sum lies below zero
        _, planes = expected_join(n, inner, cols)
        assert (planes[1].view(np.int64) < 0).any()


def test_duplicate_r_keys(ctx):
    R = pc.uniform(1 << 13, 1 << 11, 31)
    S = pc.uniform(5000, (1 << 11) + 100, 32)
    cols = [Col(SUM, values_of(np.int64, S.size, 2)), Col(MAX, values_of(np.int32, S.size, 3)), Col(COUNT)]
    inner = run_case(ctx, R, S, [S.size], cols, tag="dup")
    assert inner.size > 3 * S.size                   # about four R rows per S tuple, each of them served


@pytest.mark.parametrize("n_cols", [1, 4])
def test_an_r_partition_of_several_lds_builds(ctx, n_cols):
    B = hj.prj_agg_layout_info(n_cols)["blockTuples"]
    R = pc.shuffled([np.full(2 * B + 5, 77, dtype=U64), np.arange(1000, 2000, dtype=U64)], 41, n_cols)
    S = pc.shuffled([np.full(7, 77, dtype=U64), np.arange(1000, 2000, dtype=U64)], 42)
    v = values_of(np.int64, S.size, 4)
    cols = [Col(SUM, v)] if n_cols == 1 else [Col(COUNT), Col(SUM, v), Col(MIN, v), Col(MAX, values_of(np.uint32, S.size, 5))]
    inner = run_case(ctx, R, S, [S.size], cols, tag=("blocks", n_cols))
    assert inner.size == 7 * (2 * B + 5) + 1000      # each of those R rows got the 7 values once


def test_many_blocks_per_partition(ctx):
    n = 1 << 16
    assert hj.prj_agg_layout_info(4)["blockTuples"] < n >> 4      # at 4 bits every partition takes more than one build
    R, S = pc.unique_shuffled(n, 6), pc.uniform(n, n, 43)
    v = values_of(np.int64, n, 6)
    run_case(ctx, R, S, [n], [Col(COUNT), Col(SUM, v), Col(MIN, v), Col(MAX, v)], bits=4, tag="bits 4")


@pytest.mark.parametrize("bits", [14, 16])
def test_a_split_s_partition(ctx, bits):
    item = hj.prj_agg_layout_info(3)["itemS"]
    hot, cold = pc.hot_keys(5, bits, 1, 300), pc.hot_keys(9, bits, 1, 500)
    R = pc.shuffled([hot, cold], 51, bits)
    rng = rng_of(52, bits)
    S = pc.shuffled([hot[rng.integers(0, hot.size, 2 * item + 1)], cold[rng.integers(0, cold.size, 1 << 11)],
                     pc.uniform(1 << 11, 1 << 20, 53)], 54, bits)
    cols = [Col(SUM, values_of(np.int64, S.size, 7)), Col(MIN, values_of(np.int32, S.size, 8)), Col(MAX, values_of(np.uint64, S.size, 9))]
    with Device(ctx) as dev:
        resident(ctx, dev, R, S.size, bits)
        agg = PrjAgg(ctx, dev, R.size, cols)
        agg.probe(S)
        info = ctx.prj_resident_info()
        assert info["maxSPartition"] >= 2 * item + 1 and info["splitPartitions"] >= 1, info       # three items, the last one short
        agg.check(expected_join(R.size, inner_expected("prj", R, S), cols), ("split", bits))


def test_zipf(ctx):
    n = 1 << 12
    R = pc.unique_shuffled(n, 7)
    S = hj.generate_relation("zipf", 1 << 16, n, 0, 1.0, 54321)
    v = values_of(np.int64, S.size, 10)
    cols = [Col(COUNT), Col(SUM, v), Col(MIN, v), Col(MAX, values_of(np.uint32, S.size, 11))]
    inner = inner_expected("prj", R, S)
    want = expected_join(n, inner, cols)
    assert int(want[0].max()) > 3000                 # the hottest row: thousands of adds to one LDS entry
    with Device(ctx) as dev:
        resident(ctx, dev, R, S.size)
        agg = PrjAgg(ctx, dev, n, cols)
        agg.probe(S)
        agg.check(want, "zipf")


@pytest.mark.parametrize("delta", [None, -1, 1, "2r+1"])
def test_padding_lanes_add_nothing(ctx, delta):
    rnd = hj.prj_agg_layout_info(2)["roundS"]
    s_size = 1 if delta is None else 2 * rnd + 1 if delta == "2r+1" else rnd + delta
    R = pc.unique_shuffled(1 << 12, 8)
    keys = np.arange(5, 1 << 12, 16, dtype=U64)      # one partition at 4 bits: one work item whose last round is ragged
    S = keys[rng_of(61, s_size).integers(0, keys.size, s_size)]
    cols = [Col(SUM, values_of(np.int64, s_size, 12)), Col(COUNT)]
    inner = run_case(ctx, R, S, [s_size], cols, bits=4, tag=("padding", s_size))
    assert inner.size == s_size                      # every S tuple matches once: the counts sum to sSize


def test_null_s_values(ctx):
    n = 1 << 12
    R = pc.unique_shuffled(n, 9)
    S = pc.uniform(5003, n, 71)                      # 5003: the last validity word is partial
    valid = rng_of(72).random(S.size) > 0.3
    none = np.zeros(S.size, dtype=bool)
    v64, v32 = values_of(np.int64, S.size, 13), values_of(np.int32, S.size, 14)
    first = [Col(COUNT, v64, valid), Col(COUNT), Col(SUM, v64, valid), Col(MIN, v32, none)]
    inner = run_case(ctx, R, S, [3000, 2003], first, tag="nulls")
    count, planes = expected_join(n, inner, first)
    assert (planes[0] < count).any() and (planes[0] <= count).all()          # COUNT(col) and COUNT(*) differ
    assert (planes[3] == first[3].identity).all()                            # nothing valid: the identity stays
    second = [Col(MAX, v64, none), Col(MAX, values_of(np.uint64, S.size, 15), valid), Col(MIN, v32, valid)]
    run_case(ctx, R, S, [S.size], second, tag="nulls 2")


def test_rows_never_probed_and_s_partitions_without_r(ctx):
    n = 1 << 14
    R = np.array([3, 700, 701, 5000, 9999, 12000, 16000, 16384], dtype=U64)
    S = pc.uniform(n, n, 1000, 11)
    v = values_of(np.int64, n, 16)
    cols = [Col(COUNT), Col(SUM, v), Col(MIN, v), Col(MAX, v)]
    inner = inner_expected("prj", R, S)
    assert 0 < inner.size < 64
    with Device(ctx) as dev:
        resident(ctx, dev, R, n, bits=11)
        agg = PrjAgg(ctx, dev, R.size, cols)
        count, planes = agg.rows("no probe")                                 # every row written once, at its identity
        assert (count == 0).all() and all((p == c.identity).all() for p, c in zip(planes, cols))
        agg.probe(S)
        want = expected_join(R.size, inner, cols)
        assert (want[0] == 0).any()
        agg.check(want, "sparse")
        _, planes = agg.rows("no count plane", with_count=False)
        assert all(np.array_equal(p, w) for p, w in zip(planes, want[1]))


def test_state_and_arguments(ctx):
    n = 1 << 10
    R = pc.unique_shuffled(n, 10)
    S = pc.uniform(n, n, 81)
    v = values_of(np.int64, n, 17)
    INVALID, STATE = _lib.HJ_ERR_INVALID, _lib.HJ_ERR_STATE
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        dR, dS, dV = dev.put(R), dev.put(S), dev.put(v)
        d_out, sum64 = put64(dev, n), [(SUM, 8, SIGNED)]
        c.reserve("prj", n, n)                                               # no row ids
        assert status(c.prj_agg_begin, sum64) == STATE                      # no resident R
        c.prj_build(dR, n)
        assert status(c.prj_agg_begin, sum64) == STATE                      # an R without row ids
        c.reserve("prj", n, n, keepRowIds=True, trackRMatches=True)
        c.prj_build(dR, n)
        assert status(c.prj_probe_agg, dS, n, [(dV, 0)]) == STATE           # before begin
        assert status(c.prj_agg_rows, [d_out]) == STATE
        for bad in ([], [(COUNT, 0, 0)] * 5, [(4, 8, 0)], [(SUM, 2, 0)], [(SUM, 0, 0)], [(COUNT, 8, 0)], [(SUM, 8, 2)], [(SUM, 8, 0, 1)]):
            assert status(c.prj_agg_begin, bad) == INVALID, bad
        assert status(c.prj_probe_agg, dS, n, [(dV, 0)]) == STATE           # a refused begin begins nothing
        c.prj_agg_begin(sum64)
        assert status(c.prj_probe_agg, dS, n, [(dV, 0), (dV, 0)]) == INVALID        # nCols mismatch
        assert status(c.prj_probe_agg, dS, n, []) == INVALID
        assert status(c.prj_probe_agg, dS, n, [(0, 0)]) == INVALID          # NULL src for SUM
        assert status(c.prj_probe_agg, dS, n, [(dV + 4, 0)]) == INVALID     # misaligned src
        assert status(c.prj_probe_agg, dS, n, [(dV, dV + 2)]) == INVALID    # misaligned srcValid
        assert status(c.prj_agg_rows, []) == INVALID                        # NULL dOut
        assert status(c.prj_agg_rows, [0]) == INVALID
        assert status(c.prj_probe_agg, dS, n + 1, [(dV, 0)]) == STATE       # above the reserved slice
        # pairs_info and the marks before ...
        cap = 2 * n
        d_s, d_r = (p.ptr for p in planes(dev, cap))
        c.prj_probe_pairs(dS, n // 2, d_s, d_r, cap)
        pairs_before, marks = c.pairs_info(), Marks(c, dev, n)
        marks.add(inner_expected("prj", R, S[:n // 2]))
        marks.check("before")
        base = c.fetch()
        # ... the aggregation grows totalMatches and sSize as prj_probe does and touches neither
        cols = [Col(SUM, v)]
        inner = inner_expected("prj", R, S)
        c.prj_probe_agg(dS, n, [(dV, 0)])
        got = c.fetch()
        assert got["totalMatches"] == base["totalMatches"] + inner.size and got["sSize"] == base["sSize"] + n
        c.prj_probe(dS, n)
        again = c.fetch()
        assert again["totalMatches"] == got["totalMatches"] + inner.size and again["sSize"] == got["sSize"] + n
        assert c.pairs_info()[:2] == pairs_before[:2] and c.pairs_info()[3] == pairs_before[3]
        marks.check("after")
        c.prj_agg_rows([d_out])
        assert np.array_equal(get64(c, d_out, n), expected_join(n, inner, cols)[1][0])
        # a second begin starts over
        c.prj_agg_begin(sum64)
        assert c.prj_agg_info()["probes"] == 0
        c.prj_agg_rows([d_out])
        assert (get64(c, d_out, n) == 0).all()
        # every call that starts a new operation ends the aggregation
        c.prj_build(dR, n)
        assert status(c.prj_probe_agg, dS, n, [(dV, 0)]) == STATE and status(c.prj_agg_rows, [d_out]) == STATE
        c.prj_agg_begin(sum64)
        c.prj_join(dR, n, dS, n)
        assert status(c.prj_probe_agg, dS, n, [(dV, 0)]) == STATE and status(c.prj_agg_rows, [d_out]) == STATE
        assert status(c.prj_agg_begin, sum64) == STATE
        assert c.prj_agg_info()["nCols"] == 0


@pytest.mark.parametrize("index", range(12))
def test_seeded_random(ctx, index):
    R, S, _lens, bits, shape = pc.random_relations(index % pc.FUZZ_BLOCKS, index)
    R, S = R[:(1 << 18) - 1], S[:(1 << 18) - 1]
    rng = rng_of(91, index)
    lens = pc.ragged(rng, S.size, int(rng.integers(1, 5)))
    valid = rng.random(S.size) > 0.2
    cols = [Col(SUM, values_of(np.int64, S.size, 18, index)), Col(MAX, values_of(np.uint32, S.size, 19, index), valid)]
    print(index, shape, "bits", bits, "R", R.size, "S", S.size, "slices", lens)
    run_case(ctx, R, S, lens, cols, bits=bits, tag=("random", index, shape))
