"""asof= through join_tables (path "htm" and "radix"), join_on and join_on_columns on an MI355X: all eight kinds against the
nested-loop model of asof_common.py, alone and together with where=. A pair is a match iff the keys are equal, every where
term holds and it is the as-of pair of its S row among such pairs; an S row without an eligible pair is an unmatched S row,
an R row that wins no S row an unmatched R row. Run with -m gpu."""
import functools
import types

import numpy as np
import pytest

import htm_hashjoin_amd as hj

import asof_common as ac
import where_common as wc

pytestmark = pytest.mark.gpu

N_S = 603
SLICE = 250                     # three slices of S, the last ragged
NO_ROW = wc.NO_ROW
FLOWS = ("tables-htm", "tables-radix", "join_on", "join_on_columns")


@functools.lru_cache(maxsize=None)
def data():
    """a versioned dimension: R rows (key, ts, level), 0 to 5 versions per key in random row order, timestamps from a small
    range so that versions of a key tie; S rows (key, ts, level). NULLs in both timestamp columns; keys of S that R does not
    have, and the other way round"""
    rng = np.random.default_rng(2025)
    d = types.SimpleNamespace()
    versions = rng.integers(0, 6, 120)
    d.r_key = rng.permutation(np.repeat(np.arange(1, 121), versions)).astype(np.uint64)
    d.n_r = d.r_key.size
    d.s_key = rng.integers(10, 151, N_S).astype(np.uint64)
    d.r_ts = rng.integers(0, 12, d.n_r).astype(np.int64)
    d.s_ts = rng.integers(0, 16, N_S).astype(np.int64)
    d.r_ts_valid, d.s_ts_valid = rng.random(d.n_r) < 0.93, rng.random(N_S) < 0.93
    d.r_level, d.s_level = rng.integers(0, 4, d.n_r).astype(np.uint8), rng.integers(0, 4, N_S).astype(np.uint8)
    d.where_terms = [wc.term_of(d.s_level, "<=", d.r_level)]
    d.where = [(d.s_level, "<=", d.r_level)]
    d.r_k2_valid, d.s_k2_valid = rng.random(d.n_r) < 0.95, rng.random(N_S) < 0.95
    d.r_cols = {"w": np.arange(d.n_r, dtype=np.uint32) * 3}
    d.s_cols = {"v": np.arange(N_S, dtype=np.uint64) * 5}
    return d


def term(d, op):
    """(the model's as-of term, the wrappers' asof=) for S.ts op R.ts"""
    return (wc.term_of(d.s_ts, op, d.r_ts, d.s_ts_valid, d.r_ts_valid),
            (np.ma.MaskedArray(d.s_ts, mask=~d.s_ts_valid), op, hj.KeyColumn(d.r_ts, d.r_ts_valid)))


def keys_of(flow, d):
    """the model's keys of both sides for a flow (None: a NULL key)"""
    if flow != "join_on_columns":
        return d.r_key.tolist(), d.s_key.tolist()
    return ([int(k) if ok else None for k, ok in zip(d.r_key, d.r_k2_valid)], [int(k) if ok else None for k, ok in zip(d.s_key, d.s_k2_valid)])


def join(flow, d, how, key_mask=0x3F, **kw):
    if flow.startswith("tables"):
        path = flow.split("-")[1]
        return hj.join_tables(d.r_key, d.s_key, d.r_cols, d.s_cols, how=how, path=path, slice_tuples=SLICE if path == "radix" else None, **kw)
    if flow == "join_on":
        wide = np.uint64(0x100000001)           # the key in both halves of a 64-bit word
        return hj.join_on(d.r_key * wide, d.s_key * wide, d.r_cols, d.s_cols, how=how, slice_tuples=SLICE, key_mask=key_mask, **kw)
    r_keys = [hj.KeyColumn.from_list([f"key-{k}" for k in d.r_key]), np.ma.MaskedArray(d.r_key.astype(np.uint16), mask=~d.r_k2_valid)]
    s_keys = [hj.KeyColumn.from_list([f"key-{k}" for k in d.s_key]), np.ma.MaskedArray(d.s_key.astype(np.uint16), mask=~d.s_k2_valid)]
    return hj.join_on_columns(r_keys, s_keys, d.r_cols, d.s_cols, how=how, slice_tuples=SLICE, key_mask=key_mask, **kw)


@pytest.mark.parametrize("flow", FLOWS)
def test_the_input_cannot_pass_vacuously(flow):
    d = data()
    r_keys, s_keys = keys_of(flow, d)
    model_term, _ = term(d, ">=")
    _rows, m = ac.model_join_asof("inner", r_keys, s_keys, [], model_term)
    per_s = {}
    for (s, r), ok in zip(m["cand"], m["eligible"]):
        per_s.setdefault(s, []).append((r, bool(ok)))
    assert 200 < d.n_r < 400 and SLICE < N_S
    assert sum(1 for v in per_s.values() if sum(ok for _, ok in v) > 1) > 50, "S rows with several eligible pairs: one wins"
    assert sum(1 for v in per_s.values() if not any(ok for _, ok in v)) > 20, "S rows whose key matches but no pair is eligible"
    assert len({r for _, r in m["cand"]} - m["r_hit"]) > 20, "R rows that are candidates and win nothing"
    tied = [s for s, r in m["inner"] if sum(1 for r2, ok in per_s[s] if ok and d.r_ts[r2] == d.r_ts[r]) > 1]
    assert len(tied) > 10, "winners that tie on the value: the lowest R row is kept"
    assert len(set(range(N_S)) - set(per_s)) > 20 and len(set(range(d.n_r)) - {r for _, r in m["cand"]}) > 5, "rows without a key partner"
    null_s = {s for s in per_s if not d.s_ts_valid[s]}
    assert null_s and not (null_s & m["s_hit"]), "an S row with a NULL timestamp matches nothing"
    assert any(not d.r_ts_valid[r] for _, r in m["cand"]) and all(d.r_ts_valid[r] for r in m["r_hit"])
    assert len(m["inner"]) == len(m["s_hit"]) > 100 and len(set(r_keys)) < d.n_r and len(set(s_keys)) < N_S
    with_where, _m = ac.model_join_asof("inner", r_keys, s_keys, d.where_terms, model_term)
    assert with_where != m["inner"] and len(with_where) > 50, "the condition changes who wins"
    # the as-of pair among the pairs that pass the condition is not the as-of pair filtered by the condition
    filtered = [p for p in m["inner"] if wc.holds(d.where_terms[0], np.array([p[0]]), np.array([p[1]]))[0]]
    assert filtered != with_where


def check_payload(got, d):
    if got["s"] is not None:
        ok = got["s_valid"]
        assert np.array_equal(ok, got["s_idx"] != NO_ROW) and np.array_equal(got["s"]["v"][ok], d.s_cols["v"][got["s_idx"][ok]])
    if got["r"] is not None:
        ok = got["r_valid"]
        assert np.array_equal(ok, got["r_idx"] != NO_ROW) and np.array_equal(got["r"]["w"][ok], d.r_cols["w"][got["r_idx"][ok]])


@pytest.mark.parametrize("how", wc.HOWS)
@pytest.mark.parametrize("flow", FLOWS)
def test_all_eight_kinds_against_the_nested_loops(flow, how):
    """backward alone, forward together with where="""
    d = data()
    r_keys, s_keys = keys_of(flow, d)
    model_term, asof = term(d, ">=")
    want, _m = ac.model_join_asof(how, r_keys, s_keys, [], model_term)
    got = join(flow, d, how, asof=asof)
    assert wc.rows_of(got) == want, (flow, how)
    check_payload(got, d)
    if how not in ("semi", "anti"):     # (which S rows have a match is the condition's answer too; which R row, and which R rows win, is not)
        assert want != wc.model_join(how, r_keys, s_keys, [model_term])[0]
    model_term, asof = term(d, "<")
    want, _m = ac.model_join_asof(how, r_keys, s_keys, d.where_terms, model_term)
    got = join(flow, d, how, where=d.where, asof=asof)
    assert wc.rows_of(got) == want, (flow, how, "with where=")
    check_payload(got, d)


@pytest.mark.parametrize("op", ac.ASOF_OPS)
def test_a_crippled_key_mask_changes_nothing(op):
    """4 bits of the join word: sixteen candidates' worth of false pairs reach the verify step, none the as-of step"""
    d = data()
    model_term, asof = term(d, op)
    want, _m = ac.model_join_asof("full", d.r_key.tolist(), d.s_key.tolist(), [], model_term)
    assert wc.rows_of(join("join_on", d, "full", key_mask=0xF, asof=asof)) == want
    assert wc.rows_of(join("join_on", d, "full", key_mask=0, asof=asof)) == want


def test_float_timestamps_one_slice_and_the_whole_of_s():
    """float32 timestamps with both zeros and NaN through join_tables; every slice size gives the same rows"""
    d = data()
    rng = np.random.default_rng(9)
    pool = np.array([0.0, -0.0, np.nan, 1.5, -1.5, 2.5, np.inf, -np.inf], dtype=np.float32)
    r_ts, s_ts = pool[rng.integers(0, pool.size, d.n_r)], pool[rng.integers(0, pool.size, N_S)]
    want, m = ac.model_join_asof("left", d.r_key.tolist(), d.s_key.tolist(), [], wc.term_of(s_ts, ">=", r_ts))
    assert len(m["inner"]) > 100
    for step in (None, N_S, 100):
        got = hj.join_tables(d.r_key, d.s_key, how="left", path="radix", slice_tuples=step, asof=(s_ts, ">=", r_ts))
        assert wc.rows_of(got) == want, step
