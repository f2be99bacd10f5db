"""range_join and interval_join on the device against the brute-force O(|S| |R|) join of range_common: all eight kinds, whole
and in slices, with where= and without, with a nullable payload column; and against range_join_host."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj

import range_common as rc

pytestmark = pytest.mark.gpu
HOWS = ("inner", "left", "semi", "anti", "right", "full", "right_semi", "right_anti")


def _tables(seed, dtype, n_r=200, n_s=300):
    rng = np.random.default_rng(seed)
    r, rv, lo, hi, lv, hv = rc.fuzz_case(seed, dtype, n_r, n_s)
    r_cols = {"a": rng.integers(0, 1 << 40, n_r).astype(np.uint64), "n": hj.KeyColumn(rng.integers(0, 99, n_r).astype(np.int32), rng.random(n_r) > 0.2)}
    s_cols = {"b": rng.integers(0, 1 << 15, n_s).astype(np.uint16)}
    wr, ws = rng.integers(0, 9, n_r).astype(np.int16), rng.integers(0, 9, n_s).astype(np.int16)
    return hj.KeyColumn(r, rv), hj.KeyColumn(lo, lv), hj.KeyColumn(hi, hv), r_cols, s_cols, [(ws, "<=", wr)]


@pytest.mark.parametrize("how", HOWS)
def test_range_join_equals_the_brute_force_join(how):
    for seed, dtype in ((1, np.int32), (2, np.float64)):
        r, lo, hi, r_cols, s_cols, where = _tables(seed, dtype)
        for w in (None, where):
            m = rc.brute_matches(r, lo, hi, False, True, "all", w)
            for slice_rows in (None, 77):
                res = hj.range_join(r, lo, hi, hi_open=True, r_cols=r_cols, s_cols=s_cols, how=how, where=w, slice_rows=slice_rows)
                rc.assert_join(res, m, how, r_cols, s_cols, (seed, w is not None, slice_rows))
        res = hj.range_join(r, None, hi, pick="last", r_cols=r_cols, how=how, slice_rows=128)
        rc.assert_join(res, rc.brute_matches(r, None, hi, pick="last"), how, r_cols, None, "the keyless as-of")
        host = hj.range_join_host(r, None, hi, pick="last", r_cols=r_cols, how=how)
        for k in ("s_idx", "r_idx"):
            assert (res[k] is None) == (host[k] is None)
        assert np.array_equal(rc.packed(*(res[k] if res[k] is not None else 0 for k in ("s_idx", "r_idx"))),
                              rc.packed(*(host[k] if host[k] is not None else 0 for k in ("s_idx", "r_idx"))))


@pytest.mark.parametrize("how", HOWS)
def test_interval_join_equals_the_brute_force_join(how):
    pts, lo, hi, p_cols, i_cols, where = _tables(4, np.int64)                  # the points are S's, the intervals R's
    for w in (None, [(where[0][2], ">=", where[0][0])]):
        m = rc.brute_matches(pts, lo, hi, True, False, "all", None if w is None else where)       # m[interval, point]
        for slice_rows in (None, 100):
            res = hj.interval_join(lo, hi, pts, lo_open=True, r_cols=i_cols, s_cols=p_cols, how=how, where=w, slice_rows=slice_rows)
            rc.assert_join(res, m.T, how, i_cols, p_cols, (w is not None, slice_rows))
