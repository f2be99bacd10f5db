"""What the tests of join_on and join_on_columns share (test_gpu_join_on.py, test_gpu_join_on_columns.py): the rows every
kind must give, derived from the inner pairs, and the check of a result dict against them -- multisets of rows with their
gathered payload columns, byte for byte. No test in here, and nothing that asks the library what a result should be."""
import numpy as np

import htm_hashjoin_amd as hj

from join_kinds_common import matched_rows, unmatched_rows
from keys_common import PAIR  # noqa: F401  (the 16-byte payload element of both files)
from r_marks_common import U64, LOW, unmatched_r, r_rows_of

NULL = -1
WEAK = 0x3F                                                     # six bits of the join word: 64 values


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


def records(rows, valid, cols, take):
    """one packed record per result row: the validity flag and the side's columns"""
    dt = np.dtype([("valid", np.bool_)] + [(name, col.dtype) for name, col in cols.items()])
    rec = np.zeros(rows, dtype=dt)
    rec["valid"] = valid
    for name in cols:
        take(rec[name], name)
    return rec


def sorted_rows(*recs):
    """the records of the sides next to each other, as bytes, sorted: a multiset of rows"""
    rows = np.concatenate([np.ascontiguousarray(r).view(np.uint8).reshape(r.size, r.dtype.itemsize) for r in recs], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def check(out, how, inner, n_r, n_s, r_cols, s_cols, tag):
    """the result of a join_on call against the inner pairs it must rest on"""
    want_s, want_r = expected_rows(how, inner, n_r, n_s)
    assert set(out) == {"s_idx", "r_idx", "s", "r", "s_valid", "r_valid"}
    want, got = [], []
    for side, rows, rel_cols in (("s", want_s, s_cols), ("r", want_r, r_cols)):
        idx, cols, valid = out[side + "_idx"], out[side], out[side + "_valid"]
        if rows is None:
            assert idx is None and cols is None and valid is None, (tag, side)
            continue
        print(tag, side, "rows", idx.size, "want", rows.size, "NULL", int((~valid).sum()))
        assert idx.dtype == np.uint32 and valid.dtype == np.bool_ and idx.shape == valid.shape == (rows.size,), (tag, side)
        assert set(cols) == set(rel_cols)
        # the maps are consistent with the columns: a NULL row is HJ_NO_ROW and all-zero bytes, any other the source row
        assert np.array_equal(valid, idx != hj.NO_ROW), (tag, side)
        for name, col in rel_cols.items():
            assert cols[name].dtype == col.dtype and cols[name].shape == idx.shape, (tag, side, name)
            assert cols[name][valid].tobytes() == col[idx[valid]].tobytes(), (tag, side, name)
            assert not np.frombuffer(cols[name][~valid].tobytes(), dtype=np.uint8).any(), (tag, side, name)
        ok = rows != NULL

        def from_source(dst, name, ok=ok, rows=rows, rel_cols=rel_cols):
            dst[ok] = rel_cols[name][rows[ok]]

        def from_result(dst, name, cols=cols):
            dst[...] = cols[name]

        # the row numbers are part of the record: a join that hands out the right payloads of the wrong rows fails
        want.append(records(rows.size, ok, rel_cols, from_source))
        want.append(np.where(ok, rows, hj.NO_ROW).astype(np.uint32))
        got.append(records(idx.size, valid, rel_cols, from_result))
        got.append(idx)
    assert np.array_equal(sorted_rows(*got), sorted_rows(*want)), tag
    if how in ("right", "full"):                                # the R-only rows come last, R ascending
        tail = unmatched_r(inner, n_r).astype(np.uint32)
        assert np.array_equal(out["r_idx"][out["r_idx"].size - tail.size:], tail), tag
        assert (out["s_idx"][out["s_idx"].size - tail.size:] == hj.NO_ROW).all(), tag
