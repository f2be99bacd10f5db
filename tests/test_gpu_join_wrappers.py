"""What the five host wrappers (join_pairs, radix_join_pairs, outer_join_pairs, radix_outer_join_pairs, join_tables) share
below their argument checks, on an MI355X: the planes sized for a foreign-key join are enlarged to the reported count and
the slice probed once more, and the table paths fetch the counters, which refuses an R tuple outside the DataGen layout.
Expected rows come from numpy alone (inner_expected of r_marks_common, derive of join_kinds_common). Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from gpu_harness import status
from join_kinds_common import U64, INNER, LEFT, SEMI, ANTI, derive
from r_marks_common import inner_expected, r_rows_of, unmatched_r

pytestmark = pytest.mark.gpu

N = 1 << 12
SLICE = 1000                                    # five slices of S, the last one ragged
S_HOWS = {"inner": INNER, "left": LEFT, "semi": SEMI, "anti": ANTI}
R_HOWS = {"right": INNER, "full": LEFT, "right_semi": None, "right_anti": None}
PATHS = [("htm", None), ("atomic", None), ("radix", None), ("radix", SLICE)]
PATH_IDS = ["htm", "atomic", "radix", "radix_sliced"]


@pytest.fixture(scope="module")
def data():
    """R: 1024 keys four times each, shuffled; the keys are 8 apart, so open addressing keeps every copy within
    probeLength 4 of its home slot. S: 2^12 draws from R's keys. The inner pairs per meaning of a match, computed once."""
    rng = np.random.default_rng(412)
    keys = np.arange(N // 4, dtype=U64) * U64(8) + U64(1)
    R = rng.permutation(np.repeat(keys, 4))
    S = rng.choice(keys, N)
    inner = {"htm": inner_expected("htm", R, S), "atomic": inner_expected("atomic", R, S), "radix": inner_expected("prj", R, S)}
    return R, S, inner


def slices(S, slice_tuples):
    step = slice_tuples or S.size
    return [(lo, S[lo:lo + step]) for lo in range(0, S.size, step)]


def call(wrapper, R, S, how, path, slice_tuples):
    """(s_idx, r_idx) of one wrapper call"""
    if wrapper == "join_tables":
        out = hj.join_tables(R, S, how=how, path=path, slice_tuples=slice_tuples)
        assert out["s"] == ({} if out["s_idx"] is not None else None) and out["r"] == ({} if out["r_idx"] is not None else None)
        return out["s_idx"], out["r_idx"]
    if path == "radix":
        fn = hj.radix_join_pairs if how in S_HOWS else hj.radix_outer_join_pairs
        return fn(R, S, slice_tuples=slice_tuples, how=how)
    fn = hj.join_pairs if how in S_HOWS else hj.outer_join_pairs
    return fn(R, S, algo=path, how=how)


def check(how, s_idx, r_idx, inner, n_r, n_s):
    """sorted packed rows element for element; the R-only rows last, ascending"""
    packed = lambda s, r: np.sort((s.astype(U64) << U64(32)) | r.astype(U64))        # noqa: E731
    if how in S_HOWS:
        want = derive(S_HOWS[how], inner, n_s)
        if how in ("semi", "anti"):
            assert r_idx is None and s_idx.dtype == np.uint32 and np.array_equal(np.sort(s_idx).astype(U64), want), how
        else:
            assert s_idx.dtype == r_idx.dtype == np.uint32 and np.array_equal(packed(s_idx, r_idx), want), how
        return
    tail = r_rows_of(inner) if how == "right_semi" else unmatched_r(inner, n_r)
    if R_HOWS[how] is None:
        assert s_idx is None and r_idx.dtype == np.uint32 and np.array_equal(r_idx.astype(U64), tail), how
        return
    head = derive(R_HOWS[how], inner, n_s)
    k = head.size
    assert s_idx.dtype == r_idx.dtype == np.uint32 and s_idx.size == r_idx.size == k + tail.size, how
    assert np.array_equal(packed(s_idx[:k], r_idx[:k]), head), how
    assert (s_idx[k:] == hj.NO_ROW).all() and np.array_equal(r_idx[k:].astype(U64), tail), how


CASES = ([("pairs", how) for how in S_HOWS] + [("outer_pairs", how) for how in R_HOWS] +
         [("join_tables", how) for how in list(S_HOWS) + list(R_HOWS)])


@pytest.mark.parametrize("path,slice_tuples", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("wrapper,how", CASES, ids=["%s-%s" % c for c in CASES])
def test_enlarge_once(data, wrapper, how, path, slice_tuples):
    """Every slice's INNER and LEFT probe reports more rows than the slice has tuples, so the planes the wrapper starts
    with are too small in every slice of every wrapper."""
    R, S, inner = data
    key = "prj" if path == "radix" else path
    for lo, part in slices(S, slice_tuples):
        rows = inner_expected(key, R, part, s_base=lo).size
        assert rows > part.size, (path, lo, rows, part.size)
    s_idx, r_idx = call(wrapper, R, S, how, path, slice_tuples)
    check(how, s_idx, r_idx, inner[path], R.size, S.size)


@pytest.mark.parametrize("path", ["htm", "atomic"])
@pytest.mark.parametrize("wrapper,how", [("pairs", "inner"), ("outer_pairs", "right"), ("outer_pairs", "right_semi"),
                                         ("join_tables", "inner"), ("join_tables", "full")])
def test_key_range_table_paths_refuse(data, wrapper, how, path):
    """one R tuple with bit 40 set is outside the DataGen layout: the table paths say so"""
    R, S, _ = data
    R = R.copy()
    R[7] |= U64(1) << U64(40)
    assert status(call, wrapper, R, S, how, path, None) == _lib.HJ_ERR_KEY_RANGE


@pytest.mark.parametrize("slice_tuples", [None, SLICE])
@pytest.mark.parametrize("wrapper,how", [("pairs", "inner"), ("outer_pairs", "right"), ("join_tables", "full")])
def test_key_range_radix_joins_on_the_key_word(data, wrapper, how, slice_tuples):
    R, S, _ = data
    R = R.copy()
    R[7] |= U64(1) << U64(40)
    s_idx, r_idx = call(wrapper, R, S, how, "radix", slice_tuples)
    check(how, s_idx, r_idx, inner_expected("prj", R, S), R.size, S.size)
