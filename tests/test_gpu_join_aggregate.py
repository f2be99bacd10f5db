"""The two wrappers: radix_join_aggregate against numpy over the pairs of the key word, aggregate_on against a numpy group-by
over the rows join_on_columns(how="inner") returns -- at key_mask 0 and at key_mask 0xFF, which must give the SAME result:
a reduction over the candidate pairs instead of the kept ones fails that."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
import prj_cases as pc
from agg_common import COUNT, SUM, MIN, MAX, U64, Col, expected, expected_join
from r_marks_common import inner_expected

pytestmark = pytest.mark.gpu
OPS = {"count": COUNT, "sum": SUM, "min": MIN, "max": MAX}


def rng_of(*seed):
    return np.random.default_rng([20261021, *seed])


def check(res, aggs, sources, want_count, want_planes, n_r, tag):
    """the result dict against (count, planes) of agg_common.expected for the same aggregates, in the order of `aggs`"""
    assert sorted(res) == sorted(["count", *aggs]), tag
    assert res["count"].dtype == np.uint64 and np.array_equal(res["count"], want_count), (tag, "count")
    for (name, (op, src)), plane in zip(aggs.items(), want_planes):
        got = res[name]
        if op == "count":
            assert got.dtype == np.uint64 and np.array_equal(got, plane), (tag, name)
            continue
        values, valid = sources[src]
        seen = np.zeros(n_r, dtype=bool)             # the group saw at least one valid value
        seen[:] = want_count > 0 if valid is None else want_planes[list(aggs).index("_n_" + src)] > 0
        assert isinstance(got, hj.KeyColumn) and np.array_equal(got.valid, seen), (tag, name, "validity")
        assert got.values.dtype == (np.int64 if values.dtype.kind == "i" else np.uint64), (tag, name)
        assert np.array_equal(got.values.view(U64)[seen], plane[seen]) and not got.values[~seen].any(), (tag, name)


def request(n_s, seed):
    """six aggregates over three sources, one of them nullable, and COUNT(col) of each nullable source for the check"""
    rng = rng_of(seed)
    a = rng.integers(-(1 << 62), 1 << 62, n_s, dtype=np.int64)
    a[::9] = (1 << 63) - 1
    b = rng.integers(0, 1 << 32, n_s, dtype=np.uint32)
    c = rng.integers(-(1 << 31), 1 << 31, n_s, dtype=np.int32)
    c_valid = rng.random(n_s) > 0.3
    sources = {"a": (a, None), "b": (b, None), "c": (c, c_valid)}
    aggs = {"n": ("count", None), "sum_a": ("sum", "a"), "max_b": ("max", "b"), "min_c": ("min", "c"), "sum_c": ("sum", "c"),
            "_n_c": ("count", "c")}
    s_cols = {"a": a, "b": b, "c": hj.KeyColumn(c, c_valid)}
    cols = [Col(OPS[op], None if src is None else sources[src][0], None if src is None else sources[src][1]) for op, src in aggs.values()]
    return sources, aggs, s_cols, cols


def test_radix_join_aggregate_in_slices_and_two_rounds():
    n = 1 << 12
    R, S = pc.unique_shuffled(n, 11), pc.uniform(3 * n, n + 300, 101)
    sources, aggs, s_cols, cols = request(S.size, 1)
    assert len(aggs) == 6 and len(aggs) > hj.HJ_AGG_MAX_COLS          # six device columns and the wrapper's own COUNT(c): two rounds
    res = hj.radix_join_aggregate(R, S, s_cols, aggs, slice_tuples=1500)
    want_count, want = expected_join(n, inner_expected("prj", R, S), cols)
    check(res, aggs, sources, want_count, want, n, "radix")
    assert not res["min_c"].valid.all() and res["min_c"].valid.any()


def strings(rng, n, distinct, null_every):
    words = [None if null_every and i % null_every == 0 else "k%d" % (rng.integers(0, distinct)) * int(rng.integers(1, 4)) for i in range(n)]
    return hj.KeyColumn.from_list(words)


def key_cases():
    rng = rng_of(7)
    n_r, n_s = 700, 2600
    yield "strings with NULLs", [strings(rng, n_r, 400, 11)], [strings(rng, n_s, 400, 13)]
    r64, s64 = rng.integers(0, 40, n_r).astype(np.int64) << 33, rng.integers(0, 40, n_s).astype(np.int64) << 33
    yield "int64 + string", [r64, strings(rng, n_r, 12, 17)], [s64, strings(rng, n_s, 12, 19)]


@pytest.mark.parametrize("case", range(2))
@pytest.mark.parametrize("nulls_equal", [False, True])
def test_aggregate_on_equals_a_group_by_over_join_on_columns(case, nulls_equal):
    tag, r_keys, s_keys = list(key_cases())[case]
    n_r, n_s = len(r_keys[0]), len(s_keys[0])
    sources, aggs, s_cols, cols = request(n_s, 2 + case)
    joined = hj.join_on_columns(r_keys, s_keys, how="inner", nulls_equal=nulls_equal, slice_tuples=1000)
    r_idx, s_idx = joined["r_idx"], joined["s_idx"]
    assert r_idx.size > n_s // 4, (tag, r_idx.size)
    want_count, want = expected(n_r, r_idx, s_idx, cols)
    results = [hj.aggregate_on(r_keys, s_keys, s_cols, aggs, nulls_equal=nulls_equal, slice_tuples=1000, key_mask=mask) for mask in (0, 0xFF)]
    for res, mask in zip(results, (0, 0xFF)):
        check(res, aggs, sources, want_count, want, n_r, (tag, nulls_equal, mask))
    for name in results[0]:                          # identical, element for element, validity and values under NULL included
        a, b = results[0][name], results[1][name]
        if isinstance(a, hj.KeyColumn):
            assert np.array_equal(a.values, b.values) and np.array_equal(a.valid, b.valid), name
        else:
            assert np.array_equal(a, b), name
