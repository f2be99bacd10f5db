"""Randomised differential tests of the relational layer on an MI355X: join_on_columns, join_on, join_tables, where=, asof=,
the payload gathers, aggregate_on, radix_join_aggregate, key_groups, distinct_on and group_by_columns on the problems of
fuzz_tables.py -- sizes on the lane, workgroup and validity-word edges, slices against those edges, the options in
combination, and the degenerate tables the Python driver treats on branches of its own. Every expectation comes from the
models of where_common, asof_common, keys2_common, agg_common and groups_common (test_fuzz_tables.py holds generator and
models to each other without a device); rows are compared exactly, payload byte for byte, and the order of the rows slice
by slice as the join_on docstring states it. Every assertion carries a tag from which the case can be drawn again:
fuzz_tables.problems(block, cases). HJ_FUZZ_CASES (default fuzz_tables.CASES = 96, twelve per test id: measured on an
MI355X, the slowest id here then takes 1.3 s and the slowest id of test_gpu_fuzz.py 2.3 s) sets the number of cases per
test; the seeds are fixed, 20267000 + block. Run with -m gpu."""
import os

import numpy as np
import pytest

import htm_hashjoin_amd as hj

import asof_common as asc
import fuzz_tables as ft
import groups_common as gc
import where_common as wc

pytestmark = pytest.mark.gpu

NO_ROW = wc.NO_ROW
BLOCKS = ft.BLOCKS
S_PLANE = ("inner", "left", "semi", "anti", "right", "full")
R_PLANE = ("inner", "left", "right", "full", "right_semi", "right_anti")


def cases():
    return int(os.environ.get("HJ_FUZZ_CASES", str(ft.CASES)))


def model_rows(how, r_keys, s_keys, where, asof):
    if asof is not None:
        return asc.model_join_asof(how, r_keys, s_keys, where, asof)[0]
    return wc.model_join(how, r_keys, s_keys, where)[0]


def check_payload(res, side, idx, cols, cols_model, tag):
    """valid == (idx != NO_ROW); every valid row is its source row (bytes for arrays, to_list() for KeyColumns, a NULL source
    stays NULL); every invalid row is all-zero bytes, or empty and NULL"""
    ok = idx != NO_ROW
    assert res[side + "_valid"].dtype == np.bool_ and np.array_equal(res[side + "_valid"], ok), (tag, side)
    assert set(res[side]) == set(cols_model), (tag, side)
    src_rows = idx[ok].astype(np.int64)
    for name, (kind, src) in cols_model.items():
        got = res[side][name]
        if kind == "bytes":
            assert isinstance(got, np.ndarray) and got.dtype == np.asarray(cols[name]).dtype and got.shape == idx.shape, (tag, side, name)
            raw = np.ascontiguousarray(got).view(np.uint8).reshape(idx.size, src.shape[1])
            assert np.array_equal(raw[ok], src[src_rows]), (tag, side, name)
            assert not raw[~ok].any(), (tag, side, name, "a row without a tuple is not all-zero")
            continue
        assert isinstance(got, hj.KeyColumn) and got.rows == idx.size and got.width == cols[name].width, (tag, side, name)
        assert got.to_list() == [None if i == NO_ROW else src[i] for i in idx.tolist()], (tag, side, name)
        if got.offsets is None:
            raw = np.ascontiguousarray(got.values).view(np.uint8).reshape(idx.size, got.width)
            assert not raw[~ok].any(), (tag, side, name, "a row without a tuple is not all-zero")
        else:
            assert not np.diff(got.offsets.astype(np.int64))[~ok].any(), (tag, side, name, "a row without a tuple is not empty")


def check_order(res, how, step, tag, pairs_first=True):
    """join_on's order: per S slice the kept pairs first, then the slice's unmatched S rows ascending (left / full); semi /
    anti ascending per slice; the R-only rows last, R ascending. pairs_first False (join_tables without a condition: the
    probe's own rows per slice): the slices in order and the R-only rows last."""
    s, r = res["s_idx"], res["r_idx"]
    if how in ("right_semi", "right_anti"):
        assert (np.diff(r.astype(np.int64)) > 0).all(), (tag, "R rows not ascending")
        return
    if how in ("semi", "anti"):
        s = s.astype(np.int64)
        assert (np.diff(s if pairs_first else s // max(step, 1)) >= (1 if pairs_first else 0)).all(), (tag, "S rows not ascending")
        return
    r_only = s == NO_ROW
    body = s.size - int(r_only.sum())
    assert not r_only[:body].any(), (tag, "an R-only row before the last probe row")
    assert (np.diff(r[body:].astype(np.int64)) > 0).all(), (tag, "R-only rows not ascending")
    s, lone = s[:body].astype(np.int64), r[:body] == NO_ROW
    slices = s // max(step, 1)
    assert (np.diff(slices) >= 0).all(), (tag, "a slice's rows behind a later slice's")
    if pairs_first:
        assert (np.diff(2 * slices + lone) >= 0).all(), (tag, "an unmatched S row before a pair of its slice")
        assert (np.diff(s[lone]) > 0).all(), (tag, "unmatched S rows not ascending")


def check_join(res, how, want, p, step, tag, pairs_first=True):
    for side, plane in (("s", how in S_PLANE), ("r", how in R_PLANE)):
        if not plane:
            assert res[side + "_idx"] is None and res[side] is None and res[side + "_valid"] is None, (tag, side)
    got = wc.rows_of(res)
    assert got == want, (tag, len(got), len(want), [x for x in got if x not in set(want)][:4], [x for x in want if x not in set(got)][:4])
    check_order(res, how, step, tag, pairs_first)
    if how in S_PLANE:
        check_payload(res, "s", res["s_idx"], p.s_cols, p.s_cols_model, tag)
    if how in R_PLANE:
        check_payload(res, "r", res["r_idx"], p.r_cols, p.r_cols_model, tag)


def conditions(p):
    """the drawn where and asof, and neither"""
    drawn = (p.where or None, p.asof, p.where_model, p.asof_model)
    return [drawn] if not p.where and p.asof is None else [drawn, (None, None, [], None)]


# ---- 1. joins on key columns ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(BLOCKS))
def test_joins_on_key_columns(block):
    """join_on_columns for the drawn kind and for full (every pair and both kinds of lone rows), with the drawn where / asof
    and with neither; join_on on the same columns as plain arrays whenever the problem has no NULL key and no string"""
    for case, p in ft.problems(block, cases()):
        kw = dict(r_cols=p.r_cols, s_cols=p.s_cols, radixBits=p.radix_bits, slice_tuples=p.slice_tuples, key_mask=p.key_mask)
        for where, asof, where_model, asof_model in conditions(p):
            for how in dict.fromkeys((p.how, "full")):
                tag = ft.tag_of(p, block, case, call="join_on_columns", how_run=how, cond=where is not None or asof is not None)
                want = model_rows(how, p.r_rowkeys, p.s_rowkeys, where_model, asof_model)
                res = hj.join_on_columns(p.r_keys, p.s_keys, how=how, nulls_equal=p.nulls_equal, where=where, asof=asof, **kw)
                check_join(res, how, want, p, p.step, tag)
                if p.plain_keys and how == p.how:
                    tag["call"] = "join_on"
                    res = hj.join_on([c.values for c in p.r_keys], [c.values for c in p.s_keys], how=how, where=where, asof=asof, **kw)
                    check_join(res, how, want, p, p.step, tag)


# ---- 2. join_tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(BLOCKS))
def test_join_tables(block):
    """the problem on one 32-bit key word (fuzz_tables.reduced_keys): path "radix" with the drawn slices and "htm" in one
    piece, the same models on the integer keys, the same payload and order checks"""
    for case, p in ft.problems(block, cases()):
        where, asof, where_model, asof_model = conditions(p)[case % len(conditions(p))]
        cond = where is not None or asof is not None
        want = model_rows(p.how, p.r_ids, p.s_ids, where_model, asof_model)
        for path in ("radix", "htm"):
            tag = ft.tag_of(p, block, case, call="join_tables", path=path, cond=cond)
            res = hj.join_tables(p.relR, p.relS, r_cols=p.r_cols, s_cols=p.s_cols, how=p.how, path=path, radixBits=p.radix_bits,
                                 slice_tuples=p.slice_tuples, where=where, asof=asof)
            check_join(res, p.how, want, p, p.step if path == "radix" else max(p.n_s, 1), tag, pairs_first=cond)


# ---- 3. aggregates -------------------------------------------------------------------------------------------------------------
def check_aggregates(got, want, aggs, tag):
    assert set(got) == set(want), tag
    assert got["count"].dtype == np.uint64 and np.array_equal(got["count"], want["count"]), (tag, "count")
    for out, (op, _) in aggs.items():
        if op == "count":
            assert np.array_equal(got[out], want[out]), (tag, out)
            continue
        values, valid = want[out]
        col = got[out]
        assert isinstance(col, hj.KeyColumn) and col.rows == values.size, (tag, out)
        assert np.array_equal(col.valid if col.valid is not None else np.ones(col.rows, dtype=bool), valid), (tag, out, "validity")
        assert np.array_equal(np.asarray(col.values).view(np.uint64), values), (tag, out)


@pytest.mark.parametrize("block", range(BLOCKS))
def test_aggregating_joins(block):
    """aggregate_on against agg_common.expected over the model's inner pairs; radix_join_aggregate on the reduced keys; and
    the match counts against np.bincount of the R rows of the inner join_on_columns result of the same problem"""
    for case, p in ft.problems(block, cases()):
        tag = ft.tag_of(p, block, case, aggs=p.aggs)
        pairs = wc.model_join("inner", p.r_rowkeys, p.s_rowkeys, [])[0]
        want = ft.agg_expected(p, p.n_r, [r for _, r in pairs], [s for s, _ in pairs])
        got = hj.aggregate_on(p.r_keys, p.s_keys, p.agg_cols, p.aggs, nulls_equal=p.nulls_equal, radixBits=p.radix_bits,
                              slice_tuples=p.slice_tuples, key_mask=p.key_mask)
        check_aggregates(got, want, p.aggs, dict(tag, call="aggregate_on"))
        got = hj.radix_join_aggregate(p.relR, p.relS, p.agg_cols, p.aggs, radixBits=p.radix_bits, slice_tuples=p.slice_tuples)
        check_aggregates(got, want, p.aggs, dict(tag, call="radix_join_aggregate"))
        inner = hj.join_on_columns(p.r_keys, p.s_keys, nulls_equal=p.nulls_equal, slice_tuples=p.slice_tuples, key_mask=p.key_mask)
        assert np.array_equal(got["count"], np.bincount(inner["r_idx"], minlength=p.n_r).astype(np.uint64)), (tag, "bincount")


# ---- 4. groups -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(BLOCKS))
def test_groups(block):
    """key_groups on the S side's key columns against groups_common.model_groups; distinct_on with the payload columns (the
    first rows' source rows and keys); group_by_columns against agg_common.expected grouped by the model's ids; and the
    self-join that pairs row i with row j exactly when they are in one group"""
    for case, p in ft.problems(block, cases()):
        tag = ft.tag_of(p, block, case)
        keys = gc.model_keys(p.s_model, p.nulls)
        want = gc.model_groups(keys)
        gc.same(hj.key_groups(p.s_keys, nulls=p.nulls, key_mask=p.key_mask), want, dict(tag, call="key_groups"))
        first = want["first_rows"]
        first_keys = [[c.items[i] for i in first.tolist()] for c in p.s_model]
        # distinct_on
        got = hj.distinct_on(p.s_keys, p.s_cols, nulls=p.nulls, key_mask=p.key_mask)
        t = dict(tag, call="distinct_on")
        assert (got["n_groups"], got["null_rows"]) == (want["n_groups"], want["null_rows"]) and np.array_equal(got["first_rows"], first), t
        assert [k.to_list() for k in got["keys"]] == first_keys, t
        check_payload({"s": got["cols"], "s_valid": np.ones(first.size, dtype=bool)}, "s", first, p.s_cols, p.s_cols_model, t)
        # group_by_columns
        got = hj.group_by_columns(p.s_keys, p.agg_cols, p.aggs, nulls=p.nulls, key_mask=p.key_mask)
        t = dict(tag, call="group_by_columns", aggs=p.aggs)
        assert (got["n_groups"], got["null_rows"]) == (want["n_groups"], want["null_rows"]) and np.array_equal(got["first_rows"], first), t
        assert [k.to_list() for k in got["keys"]] == first_keys, t
        rows = np.flatnonzero(want["group"] != NO_ROW)
        exp = ft.agg_expected(p, want["n_groups"], want["group"][rows], rows)
        check_aggregates({k: got[k] for k in exp}, exp, p.aggs, t)
        # the self-join: (i, j) is a pair exactly when group[i] == group[j]
        if sum(int(c) ** 2 for c in np.bincount(want["group"][rows], minlength=1)) <= ft.PAIR_CAP:
            res = hj.join_on_columns(p.s_keys, p.s_keys, nulls_equal=(p.nulls == "group"), slice_tuples=p.slice_tuples, key_mask=p.key_mask)
            members = {}
            for i in rows.tolist():
                members.setdefault(int(want["group"][i]), []).append(i)
            assert wc.rows_of(res) == sorted((i, j) for m in members.values() for i in m for j in m), dict(tag, call="self-join")
