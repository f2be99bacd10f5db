"""join_tables on an MI355X: all eight kinds over the table probes and the resident radix join, whole and in slices. The
expected rows come from numpy: the inner pairs of r_marks_common (sort + searchsorted, or the plain-Python walk for open
addressing), the kinds derived from them, and the payload rows built with numpy indexing. Compared as multisets of rows
(S payloads, R payloads and the two validity flags), byte for byte. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj

from r_marks_common import U64, LOW, inner_expected, unmatched_r, r_rows_of
from join_kinds_common import matched_rows, unmatched_rows

pytestmark = pytest.mark.gpu

N = 1 << 12
HOWS = ("inner", "left", "semi", "anti", "right", "full", "right_semi", "right_anti")
PATHS = [("htm", None), ("atomic", None), ("radix", None), ("radix", 1000)]
PAIR = np.dtype([("a", np.uint64), ("b", np.float64)])         # a 16-byte structured element
NULL = -1


@pytest.fixture(scope="module")
def data():
    """|R| = |S| = 2^12: R with duplicate keys, half of S absent from R, a quarter of R (and more) never probed; two payload
    columns per side; the inner pairs per meaning of a match, computed once"""
    rng = np.random.default_rng(2024)
    R = hj.generate_data("uniform", N, N, 16)
    S = np.concatenate([rng.choice(R[:3 * N // 4], N // 2), np.arange(N + 1, N + 1 + N // 2, dtype=U64)])
    rng.shuffle(S)
    r16 = np.zeros(N, dtype=PAIR)
    r16["a"], r16["b"] = rng.integers(1, 1 << 62, N), rng.random(N)
    r_cols = {"r4": rng.integers(1, 1 << 31, N).astype(np.uint32), "r16": r16}
    s_cols = {"s2": rng.integers(1, 1 << 15, S.size).astype(np.int16), "s8": rng.random(S.size) + 1.0}
    inner = {"htm": inner_expected("htm", R, S), "atomic": inner_expected("atomic", R, S), "radix": inner_expected("prj", R, S)}
    assert np.unique(R).size < N and inner["htm"].size > N // 2
    for pairs in inner.values():
        assert unmatched_rows(pairs, S.size).size >= N // 2 and unmatched_r(pairs, N).size >= N // 4
    return R, S, r_cols, s_cols, inner


def expected_rows(how, inner, n_r, n_s):
    """(S row, R row) of every result row, NULL where the side has no tuple; None for a side the kind has no plane for"""
    s = (inner >> U64(32)).astype(np.int64)
    r = (inner & LOW).astype(np.int64)
    lone_s = unmatched_rows(inner, n_s).astype(np.int64)
    lone_r = unmatched_r(inner, n_r).astype(np.int64)
    nulls = lambda n: np.full(n, NULL, dtype=np.int64)        # noqa: E731
    if how == "inner":
        return s, r
    if how == "left":
        return np.concatenate([s, lone_s]), np.concatenate([r, nulls(lone_s.size)])
    if how == "semi":
        return matched_rows(inner).astype(np.int64), None
    if how == "anti":
        return lone_s, None
    if how == "right":
        return np.concatenate([s, nulls(lone_r.size)]), np.concatenate([r, lone_r])
    if how == "full":
        return (np.concatenate([s, lone_s, nulls(lone_r.size)]), np.concatenate([r, nulls(lone_s.size), lone_r]))
    if how == "right_semi":
        return None, r_rows_of(inner).astype(np.int64)
    return None, lone_r


def side_records(rows, cols):
    """one packed record per result row: the validity flag and the side's columns, all-zero bytes where the row is NULL"""
    dt = np.dtype([("valid", np.bool_)] + [(name, col.dtype) for name, col in cols.items()])
    rec = np.zeros(rows.size, dtype=dt)
    ok = rows != NULL
    rec["valid"] = ok
    for name, col in cols.items():
        rec[name][ok] = col[rows[ok]]
    return rec


def got_records(valid, got, cols):
    dt = np.dtype([("valid", np.bool_)] + [(name, col.dtype) for name, col in cols.items()])
    rec = np.zeros(valid.size, dtype=dt)
    rec["valid"] = valid
    for name in cols:
        rec[name] = got[name]
    return rec


def sorted_rows(*recs):
    """the records of the sides next to each other, as bytes, sorted: a multiset of rows"""
    rows = np.concatenate([np.ascontiguousarray(r).view(np.uint8).reshape(r.size, r.dtype.itemsize) for r in recs], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("path,slice_tuples", PATHS)
@pytest.mark.parametrize("how", HOWS)
def test_join_tables(data, how, path, slice_tuples):
    R, S, r_cols, s_cols, inner = data
    want_s, want_r = expected_rows(how, inner[path], R.size, S.size)
    out = hj.join_tables(R, S, r_cols=r_cols, s_cols=s_cols, how=how, path=path, slice_tuples=slice_tuples)
    assert set(out) == {"s_idx", "r_idx", "s", "r", "s_valid", "r_valid"}
    want, got = [], []
    for side, rows, rel_cols in (("s", want_s, s_cols), ("r", want_r, r_cols)):
        idx, cols, valid = out[side + "_idx"], out[side], out[side + "_valid"]
        if rows is None:
            assert idx is None and cols is None and valid is None, (how, side)
            continue
        print(how, path, slice_tuples, side, "rows", idx.size, "want", rows.size, "NULL", int((~valid).sum()))
        assert idx.dtype == np.uint32 and valid.dtype == np.bool_ and idx.shape == valid.shape == (rows.size,)
        assert set(cols) == set(rel_cols)
        # the maps are consistent with the columns: a NULL row is HJ_NO_ROW and all-zero bytes, any other the source row
        assert np.array_equal(valid, idx != hj.NO_ROW)
        for name, col in rel_cols.items():
            assert cols[name].dtype == col.dtype and cols[name].shape == idx.shape, (how, side, name)
            assert cols[name][valid].tobytes() == col[idx[valid]].tobytes(), (how, side, name)
            assert not np.frombuffer(cols[name][~valid].tobytes(), dtype=np.uint8).any(), (how, side, name)
        want.append(side_records(rows, rel_cols))
        got.append(got_records(valid, cols, rel_cols))
    assert np.array_equal(sorted_rows(*got), sorted_rows(*want)), (how, path, slice_tuples)
    if how in ("right", "full"):                                # the R-only rows come last, R ascending
        tail = unmatched_r(inner[path], R.size).astype(np.uint32)
        assert np.array_equal(out["r_idx"][-tail.size:], tail) and (out["s_idx"][-tail.size:] == hj.NO_ROW).all()


def test_more_than_eight_columns_and_none(data):
    """nine columns on a side take two gather calls; a side without columns still has its map and its validity"""
    R, S, r_cols, s_cols, inner = data
    rng = np.random.default_rng(5)
    many = {f"c{k}": rng.integers(0, 256, R.size * w, dtype=np.uint8).view(f"V{w}") for k, w in enumerate((1, 2, 4, 8, 16, 16, 8, 4, 2))}
    out = hj.join_tables(R, S, r_cols=many, how="full", path="htm")
    want_s, want_r = expected_rows("full", inner["htm"], R.size, S.size)
    assert out["s"] == {} and np.array_equal(np.sort(out["s_valid"]), np.sort(want_s != NULL))
    assert np.array_equal(out["r_valid"], out["r_idx"] != hj.NO_ROW)
    for name, col in many.items():
        assert out["r"][name].dtype == col.dtype
        assert out["r"][name][out["r_valid"]].tobytes() == col[out["r_idx"][out["r_valid"]]].tobytes(), name
        assert not np.frombuffer(out["r"][name][~out["r_valid"]].tobytes(), dtype=np.uint8).any(), name
    pairs = (out["s_idx"].astype(U64) << U64(32)) | out["r_idx"].astype(U64)
    both = out["s_valid"] & out["r_valid"]
    assert np.array_equal(np.sort(pairs[both]), inner["htm"])
