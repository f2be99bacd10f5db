"""where= through join_tables (path "htm" and "radix"), join_on and join_on_columns on an MI355X: all eight kinds against
the nested-loop model of where_common.py. A pair is a match iff the keys are equal and every term holds, so a row whose
pairs all fail the condition is an unmatched row -- which a filter behind the join could not say. Run with -m gpu."""
import functools
import types

import numpy as np
import pytest

import htm_hashjoin_amd as hj

import where_common as wc

pytestmark = pytest.mark.gpu

N_R, N_S = 301, 1003
SLICE = 400                     # three slices of S, the last ragged
NO_ROW = wc.NO_ROW
FLOWS = ("tables-htm", "tables-radix", "join_on", "join_on_columns")


@functools.lru_cache(maxsize=None)
def data():
    """a versioned dimension: R rows (key, valid_from, valid_to), several versions per key; S rows (key, ts). NULLs in ts
    and in valid_to; keys of S that R does not have, and the other way round"""
    rng = np.random.default_rng(2024)
    d = types.SimpleNamespace()
    d.r_key = rng.integers(1, 90, N_R).astype(np.uint64)            # about three versions per key
    d.s_key = rng.integers(10, 110, N_S).astype(np.uint64)
    d.r_from = rng.integers(0, 60, N_R).astype(np.int32)
    d.r_to = (d.r_from + rng.integers(0, 40, N_R)).astype(np.float64)
    d.r_to_valid = rng.random(N_R) < 0.93
    d.s_ts = rng.integers(0, 100, N_S).astype(np.int32)
    d.s_ts_valid = rng.random(N_S) < 0.93
    # ts >= valid_from AND ts < valid_to, the second term on a float64 copy of ts
    d.terms = [wc.term_of(d.s_ts, ">=", d.r_from, d.s_ts_valid, None),
               wc.term_of(d.s_ts.astype(np.float64), "<", d.r_to, d.s_ts_valid, d.r_to_valid)]
    d.where = [(np.ma.MaskedArray(d.s_ts, mask=~d.s_ts_valid), ">=", d.r_from),
               (hj.KeyColumn(d.s_ts.astype(np.float64), d.s_ts_valid), "<", np.ma.MaskedArray(d.r_to, mask=~d.r_to_valid))]
    # join_on_columns: a string key and a nullable key; a NULL in the second makes the row NULL-keyed
    d.r_k2_valid, d.s_k2_valid = rng.random(N_R) < 0.95, rng.random(N_S) < 0.95
    d.r_cols = {"w": np.arange(N_R, dtype=np.uint32) * 3}
    d.s_cols = {"v": np.arange(N_S, dtype=np.uint64) * 5}
    return d


def keys_of(flow, d):
    """the model's keys of both sides for a flow (None: a NULL key)"""
    if flow != "join_on_columns":
        return d.r_key.tolist(), d.s_key.tolist()
    return ([int(k) if ok else None for k, ok in zip(d.r_key, d.r_k2_valid)], [int(k) if ok else None for k, ok in zip(d.s_key, d.s_k2_valid)])


def join(flow, d, how, **kw):
    if flow.startswith("tables"):
        path = flow.split("-")[1]
        return hj.join_tables(d.r_key, d.s_key, d.r_cols, d.s_cols, how=how, path=path, slice_tuples=SLICE if path == "radix" else None, **kw)
    if flow == "join_on":
        wide = np.uint64(0x100000001)           # the key in both halves of a 64-bit word; 64 join words: false candidates reach the step
        return hj.join_on(d.r_key * wide, d.s_key * wide, d.r_cols, d.s_cols, how=how, slice_tuples=SLICE, key_mask=0x3F, **kw)
    r_keys = [hj.KeyColumn.from_list([f"key-{k}" for k in d.r_key]), np.ma.MaskedArray(d.r_key.astype(np.uint16), mask=~d.r_k2_valid)]
    s_keys = [hj.KeyColumn.from_list([f"key-{k}" for k in d.s_key]), np.ma.MaskedArray(d.s_key.astype(np.uint16), mask=~d.s_k2_valid)]
    return hj.join_on_columns(r_keys, s_keys, d.r_cols, d.s_cols, how=how, slice_tuples=SLICE, key_mask=0x3F, **kw)


@pytest.mark.parametrize("flow", FLOWS)
def test_the_input_cannot_pass_vacuously(flow):
    d = data()
    r_keys, s_keys = keys_of(flow, d)
    _rows, m = wc.model_join("inner", r_keys, s_keys, d.terms)
    s_cand, r_cand = {s for s, _ in m["cand"]}, {r for _, r in m["cand"]}
    assert len(s_cand - m["s_hit"]) > 20, "S rows whose key matches but no pair passes"
    assert len(r_cand - m["r_hit"]) > 20, "R rows whose key matches but no pair passes"
    failed = {s for (s, _), k in zip(m["cand"], m["keep"]) if not k}
    assert len(failed & m["s_hit"]) > 20, "S rows with some pairs passing and some failing"
    assert len(set(range(N_S)) - s_cand) > 20 and len(set(range(N_R)) - r_cand) > 5, "rows without a key partner"
    assert not d.s_ts_valid.all() and not d.r_to_valid.all(), "NULLs in the term columns"
    null_s = {s for s in s_cand if not d.s_ts_valid[s]}
    assert null_s and not (null_s & m["s_hit"]), "an S row with a NULL ts matches nothing"
    assert len(m["inner"]) > 100 and len(set(r_keys)) < N_R and len(set(s_keys)) < N_S      # duplicate keys on both sides


@pytest.mark.parametrize("how", wc.HOWS)
@pytest.mark.parametrize("flow", FLOWS)
def test_all_eight_kinds_against_the_nested_loops(flow, how):
    d = data()
    r_keys, s_keys = keys_of(flow, d)
    want, _m = wc.model_join(how, r_keys, s_keys, d.terms)
    got = join(flow, d, how, where=d.where)
    assert wc.rows_of(got) == want, (flow, how)
    # the payload columns went through the same maps
    if got["s"] is not None:
        ok = got["s_valid"]
        assert np.array_equal(ok, got["s_idx"] != NO_ROW) and np.array_equal(got["s"]["v"][ok], d.s_cols["v"][got["s_idx"][ok]])
    if got["r"] is not None:
        ok = got["r_valid"]
        assert np.array_equal(ok, got["r_idx"] != NO_ROW) and np.array_equal(got["r"]["w"][ok], d.r_cols["w"][got["r_idx"][ok]])
    # and the condition is not a filter behind the join: without it the kind has other rows
    plain, _m = wc.model_join(how, r_keys, s_keys, [])
    assert plain != want


def canon(result):
    """a result dict with its rows in one order: the pairs of a slice come in the order the kernels claimed their runs"""
    s_idx, r_idx = result["s_idx"], result["r_idx"]
    n = s_idx.size if s_idx is not None else r_idx.size
    order = np.lexsort((r_idx if r_idx is not None else np.zeros(n), s_idx if s_idx is not None else np.zeros(n)))
    take = lambda v: None if v is None else {k: a[order] for k, a in v.items()} if isinstance(v, dict) else v[order]     # noqa: E731
    return {k: take(v) for k, v in result.items()}


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            assert a[k].keys() == b[k].keys() and all(np.array_equal(a[k][c], b[k][c]) for c in a[k]), k
        else:
            assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("flow", FLOWS)
def test_no_condition_is_the_call_without_the_argument(flow):
    d = data()
    for how in ("full", "anti"):
        plain = canon(join(flow, d, how))
        same(canon(join(flow, d, how, where=None)), plain)
        same(canon(join(flow, d, how, where=[])), plain)
        r_keys, s_keys = keys_of(flow, d)
        assert wc.rows_of(plain) == wc.model_join(how, r_keys, s_keys, [])[0]


def test_one_side_empty_needs_no_device_work():
    d = data()
    none64, none32 = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int32)
    for how in wc.HOWS:
        same(hj.join_tables(d.r_key, none64, how=how, where=[(none32, "<", d.r_from)]), hj.join_tables(d.r_key, none64, how=how))
        same(hj.join_on(none64, d.s_key, how=how, where=[(d.s_ts, "<", none32)]), hj.join_on(none64, d.s_key, how=how))
        same(hj.join_on_columns(d.r_key, none64, how=how, where=[(none32, "<", d.r_from)]), hj.join_on_columns(d.r_key, none64, how=how))
    with pytest.raises(ValueError):
        hj.join_tables(d.r_key, d.s_key, where=[(d.s_ts, "<", d.r_to)])          # int32 against float64: no implicit cast


def test_atomic_candidates_are_that_paths_own_matches():
    """"atomic": an R tuple that ran out of probeLength is not in the table. The condition applies to the pairs the path
    gives: with a term that always holds the result is the path's own"""
    R = hj.generate_data("local_shuffle", 256, 256, 16)
    S = np.random.default_rng(3).integers(1, 300, 700).astype(np.uint64)
    ones_s, ones_r = np.zeros(S.size, np.uint8), np.ones(R.size, np.uint8)
    for how in ("inner", "left", "right_anti"):
        same(canon(hj.join_tables(R, S, how=how, path="atomic", where=[(ones_s, "<", ones_r)])), canon(hj.join_tables(R, S, how=how, path="atomic")))
        got = hj.join_tables(R, S, how=how, path="atomic", where=[(ones_s, ">", ones_r)])
        assert (got["s_idx"] is None or (got["r_idx"] == NO_ROW).all()) and (how != "right_anti" or got["r_idx"].size == R.size)
