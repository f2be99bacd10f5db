"""KeyColumn payload columns -- strings and nullable fixed columns -- through join_on_columns and join_tables on an MI355X:
R of 300 rows, S of 500, slice_tuples = 128 so that the S side goes up in four slices with its offsets rebased and its
validity repacked each time. Expected values come from the model columns of keys2_common (plain Python lists) and the
dict join there, never from the library. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj

from keys2_common import HOWS, LENGTHS, ModelCol, expected_rows, fixed_col, inner_pairs, key_column, row_keys

pytestmark = pytest.mark.gpu

N_R, N_S, SLICE = 300, 500, 128
S_PLANE = ("inner", "left", "semi", "anti", "right", "full")
R_PLANE = ("inner", "left", "right", "full", "right_semi", "right_anti")


def pool_of(rng, size, shift):
    """`size` distinct strings, their lengths cycling through LENGTHS (+ 1: none is empty)"""
    return [rng.integers(0, 256, LENGTHS[(k * 7 + shift) % len(LENGTHS)] + 1, dtype=np.uint8).tobytes() for k in range(size)]


def pooled(rng, n, pool, nulls):
    """n strings out of the pool, a share `nulls` of them None"""
    pool_size = len(pool)
    gone = rng.random(n) < nulls
    return ModelCol(0, [None if g else pool[p] for p, g in zip(rng.integers(0, pool_size, n), gone)], False)


@pytest.fixture(scope="module")
def tables():
    """the model of both sides, made once: a string key and, as payload, a string column with NULLs and a nullable 8-byte one"""
    rng = np.random.default_rng(77)
    out, keys, texts = {}, pool_of(rng, 120, 0), pool_of(rng, 40, 4)    # both sides draw from the same strings
    for side, n in (("r", N_R), ("s", N_S)):
        out[side] = {"key": pooled(rng, n, keys, 0.1), "text": pooled(rng, n, texts, 0.3), "num": fixed_col(rng, 8, n, nulls=0.3)}
    assert any(e is None for e in out["s"]["text"].items) and any(len(e) > 200 for e in out["s"]["text"].items if e is not None)
    return out


def payload(model):
    return {"text": key_column(model["text"], lead=3), "num": key_column(model["num"])}


def check_side(res, side, idx, model, tag):
    """every result row's payload against the model items its index names: None for NO_ROW or a NULL element"""
    for name in ("text", "num"):
        got = res[side][name]
        assert isinstance(got, hj.KeyColumn) and got.rows == idx.size and got.width == model[name].width, (tag, side, name)
        want = [None if i == hj.NO_ROW else model[name].items[i] for i in idx]
        assert got.to_list() == want, (tag, side, name)
        assert (got.valid is None) == all(w is not None for w in want), (tag, side, name)
    assert np.array_equal(res[side + "_valid"], idx != hj.NO_ROW), (tag, side)


def check_rows(res, how, pairs, model, tag):
    want_s, want_r = expected_rows(how, pairs, N_R, N_S)
    signed = lambda a: np.where(a == hj.NO_ROW, -1, a.astype(np.int64))     # noqa: E731
    planes = [(signed(res[k]).tolist(), w.tolist()) for k, w in (("s_idx", want_s), ("r_idx", want_r)) if w is not None]
    got, want = sorted(zip(*(g for g, _ in planes))), sorted(zip(*(w for _, w in planes)))
    assert got == want, (tag, len(got), len(want))
    for side, plane, idx_name in (("s", how in S_PLANE, "s_idx"), ("r", how in R_PLANE, "r_idx")):
        if plane:
            check_side(res, side, res[idx_name], model[side], tag)
        else:
            assert res[side] is None and res[idx_name] is None


@pytest.mark.parametrize("how", HOWS)
def test_join_on_columns_on_a_string_key(tables, how):
    pairs = inner_pairs(row_keys([tables["r"]["key"]]), row_keys([tables["s"]["key"]]))
    assert len(pairs) > 300
    res = hj.join_on_columns(key_column(tables["r"]["key"]), key_column(tables["s"]["key"], lead=1), r_cols=payload(tables["r"]),
                             s_cols=payload(tables["s"]), how=how, slice_tuples=SLICE)
    check_rows(res, how, pairs, tables, ("join_on_columns", how))


@pytest.mark.parametrize("path", ["htm", "radix"])
@pytest.mark.parametrize("how", HOWS)
def test_join_tables(tables, how, path):
    rng = np.random.default_rng(78)
    R = hj.generate_data("uniform", N_R, N_R, 16)                       # DataGen tuples, duplicate keys among them
    S = np.concatenate([rng.choice(R, 350), np.arange(N_R + 1, N_R + 151, dtype=np.uint64)])
    rng.shuffle(S)
    pairs = inner_pairs([(int(k),) for k in R], [(int(k),) for k in S])
    assert len(pairs) >= 350 and S.size == N_S
    plain = np.arange(N_S, dtype=np.uint32) * 7                         # a numpy column next to them, as before
    res = hj.join_tables(R, S, r_cols=payload(tables["r"]), s_cols=dict(payload(tables["s"]), plain=plain), how=how, path=path,
                         slice_tuples=SLICE)
    check_rows(res, how, pairs, tables, ("join_tables", path, how))
    if how in S_PLANE:
        ok = res["s_idx"] != hj.NO_ROW
        assert np.array_equal(res["s"]["plain"][ok], plain[res["s_idx"][ok]]) and (res["s"]["plain"][~ok] == 0).all()


def test_the_columns_of_a_full_join_are_the_keys_of_the_next(tables):
    first = hj.join_on_columns(key_column(tables["r"]["key"]), key_column(tables["s"]["key"]), r_cols=payload(tables["r"]),
                               s_cols=payload(tables["s"]), how="full", slice_tuples=SLICE)
    r_key, s_key = first["r"]["text"], first["s"]["text"]               # nullable string columns: unmatched rows and NULL elements
    assert r_key.valid is not None and s_key.valid is not None
    r_model, s_model = ModelCol(0, r_key.to_list(), False), ModelCol(0, s_key.to_list(), False)
    n = r_key.rows
    pairs = inner_pairs(row_keys([r_model]), row_keys([s_model]))
    assert len(pairs) > n
    for how in ("inner", "full"):
        res = hj.join_on_columns(r_key, s_key, r_cols={"num": first["r"]["num"]}, s_cols={"num": first["s"]["num"]}, how=how, slice_tuples=SLICE)
        want_s, want_r = expected_rows(how, pairs, n, n)
        signed = lambda a: np.where(a == hj.NO_ROW, -1, a.astype(np.int64))     # noqa: E731
        assert sorted(zip(signed(res["s_idx"]), signed(res["r_idx"]))) == sorted(zip(want_s, want_r)), how
        for side, src in (("s", first["s"]["num"]), ("r", first["r"]["num"])):
            items = src.to_list()
            assert res[side]["num"].to_list() == [None if i == hj.NO_ROW else items[i] for i in res[side + "_idx"]], (how, side)
