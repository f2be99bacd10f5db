"""join_on_columns on an MI355X: joins on nullable and variable-length (string) key columns, all eight kinds, whole and in
slices that do not start at a multiple of 32, under a full and a crippled hash. The expected rows come from the model in
keys2_common -- a dict join over tuples of `bytes | None`, a NULL-keyed row matching nothing -- and are compared as
multisets of rows with their gathered payload columns, as test_gpu_join_on.py compares join_on's. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj

from gpu_harness import alloc
from join_on_common import PAIR, WEAK, check
from keys2_common import HOWS, ModelCol, inner_pairs, key_column, row_keys

pytestmark = pytest.mark.gpu

U64 = np.uint64
N_R, N_S = 4000, 5000
KINDS = ("int64", "string", "composite")


def packed(pairs):
    """[(s, r)] -> s << 32 | r, sorted: what test_gpu_join_on's check takes as the inner pairs"""
    a = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    return np.sort((a[:, 0].astype(U64) << U64(32)) | a[:, 1].astype(U64))


def string_pool(rng, n):
    """n distinct strings of length 0 to 9 over three letters (so many are prefixes of others), then a few of length 31 to
    33 and 257 that share all but their last byte"""
    pool = {b""}
    while len(pool) < n:
        pool.add(rng.integers(97, 100, size=int(rng.integers(0, 10)), dtype=np.uint8).tobytes())
    stem = rng.integers(65, 91, size=257, dtype=np.uint8).tobytes()
    return sorted(pool) + [stem[:k] for k in (31, 32, 33, 257)] + [stem[:k - 1] + b"#" for k in (31, 32, 33, 257)]


def draw(rng, pool, n, nulls=0.1):
    gone = rng.random(n) < nulls
    return [None if g else pool[k] for k, g in zip(rng.integers(0, len(pool), n), gone)]


def make_data():
    """per kind of key: the model columns of R and S, about a tenth of each NULL; payload columns; the inner pairs of the
    model with NULL != NULL and with NULL == NULL"""
    rng = np.random.default_rng(2026)
    strings = string_pool(rng, 500)
    i64 = [int(v).to_bytes(8, "little", signed=True) for v in np.concatenate([[0, -1], rng.integers(-(1 << 62), 1 << 62, 1500)])]
    i32 = [int(v).to_bytes(4, "little", signed=True) for v in range(-3, 27)]
    few = [strings[k] for k in rng.integers(0, len(strings), 60)] + strings[-8:]
    part = lambda pool: [e for k, e in enumerate(pool[:-8]) if k % 5] + pool[-8:]        # noqa: E731  (R lacks a fifth of the values)
    models = {
        "int64": ([ModelCol(8, draw(rng, part(i64), N_R), False)], [ModelCol(8, draw(rng, i64, N_S), False)]),
        "string": ([ModelCol(0, draw(rng, part(strings), N_R), False)], [ModelCol(0, draw(rng, strings, N_S), False)]),
        "composite": ([ModelCol(4, draw(rng, i32, N_R), False), ModelCol(0, draw(rng, part(few), N_R), False)],
                      [ModelCol(4, draw(rng, i32, N_S), False), ModelCol(0, draw(rng, few, N_S), False)])}
    r16 = np.zeros(N_R, dtype=PAIR)
    r16["a"], r16["b"] = rng.integers(1, 1 << 62, N_R), rng.random(N_R)
    r_cols = {"r4": rng.integers(1, 1 << 31, N_R).astype(np.uint32), "r16": r16}
    s_cols = {"s2": rng.integers(1, 1 << 15, N_S).astype(np.int16), "s8": rng.random(N_S) + 1.0}
    out = {"r_cols": r_cols, "s_cols": s_cols}
    for kind, (r, s) in models.items():
        inner = {ne: packed(inner_pairs(row_keys(r, ne), row_keys(s, ne))) for ne in (False, True)}
        nulls_r, nulls_s = sum(k is None for k in row_keys(r)), sum(k is None for k in row_keys(s))
        print(kind, "inner pairs", inner[False].size, "with NULL == NULL", inner[True].size, "NULL-keyed rows", nulls_r, nulls_s)
        # the properties the cases rest on
        assert inner[False].size > N_S // 4 and inner[True].size > inner[False].size + nulls_s
        assert nulls_r > N_R // 20 and nulls_s > N_S // 20
        assert np.unique(inner[False] >> U64(32)).size < N_S - nulls_s, "some S rows with a key have no partner"
        # lead: offsets[0] != 0 on both sides, the two sides' elements at different alignments
        out[kind] = ([key_column(c, lead=1 + k) for k, c in enumerate(r)], [key_column(c, lead=2 + k) for k, c in enumerate(s)], inner)
    lens = [len(e) for e in models["string"][1][0].items if e is not None]
    assert {31, 32, 33, 257} <= set(lens) and min(lens) == 0
    return out


@pytest.fixture(scope="module")
def data():
    return make_data()


@pytest.mark.parametrize("key_mask", [0, WEAK])
@pytest.mark.parametrize("slice_tuples", [None, 333])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", HOWS)
def test_join_on_columns(data, how, kind, slice_tuples, key_mask):
    """every join kind on every kind of key; 333-row slices start in the middle of validity words and of the bytes; under
    the weak mask the verify step sees about 2^18 candidates and the result is the same one"""
    r_keys, s_keys, inner = data[kind]
    out = hj.join_on_columns(r_keys, s_keys, r_cols=data["r_cols"], s_cols=data["s_cols"], how=how, slice_tuples=slice_tuples,
                             key_mask=key_mask)
    check(out, how, inner[False], N_R, N_S, data["r_cols"], data["s_cols"], (kind, how, slice_tuples, key_mask))


@pytest.mark.parametrize("slice_tuples,key_mask", [(None, 0), (333, WEAK)])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["inner", "full"])
def test_nulls_equal(data, how, kind, slice_tuples, key_mask):
    """nulls_equal=True: a NULL matches a NULL in the same column and nothing else"""
    r_keys, s_keys, inner = data[kind]
    out = hj.join_on_columns(r_keys, s_keys, r_cols=data["r_cols"], s_cols=data["s_cols"], how=how, nulls_equal=True,
                             slice_tuples=slice_tuples, key_mask=key_mask)
    check(out, how, inner[True], N_R, N_S, data["r_cols"], data["s_cols"], (kind, how, "nulls_equal", slice_tuples, key_mask))


def test_null_rows_do_not_explode_the_candidates():
    """4096 x 4096 rows, half of each side NULL-keyed, the full join word: the candidate join hands the verify step exactly
    sum over words w of count_R(w) * count_S(w) pairs, the words being key_hash2_host's -- NULL rows spread by position,
    they do not meet on one word -- and the verify step accounts for every one of them"""
    n = 4096
    rng = np.random.default_rng(31)
    pool = rng.integers(1, 1 << 62, 700).astype(np.int64)
    cols = {}
    for side in "rs":
        valid = rng.permutation(n) < n // 2
        cols[side] = hj.KeyColumn(pool[rng.integers(0, 700, n)], valid=valid)
    words_r, words_s = hj.key_hash2_host(cols["r"]), hj.key_hash2_host(cols["s"])
    uniq, counts = np.unique(words_r, return_counts=True)
    pos = np.searchsorted(uniq, words_s)
    hit = (pos < uniq.size) & (uniq[np.minimum(pos, uniq.size - 1)] == words_s)
    want = int(counts[pos[hit]].sum())
    both = cols["s"].valid[:, None] & cols["r"].valid[None, :] & (cols["s"].values[:, None] == cols["r"].values[None, :])
    kept_want = int(both.sum())
    # all NULL rows on one word would be (n / 2)^2 candidates more
    assert kept_want <= want < kept_want + n and want < (n // 2) ** 2 // 8
    with hj.HashJoinContext(0) as ctx:
        ptrs = []

        def put(a):
            ptrs.append(alloc(ctx, max(a.nbytes, 4)))
            ctx.copy_h2d(ptrs[-1], a)
            return ptrs[-1]

        try:
            (r_vals, _, r_valid), (s_vals, _, s_valid) = cols["r"].take(0, n), cols["s"].take(0, n)
            desc = [(put(s_vals), put(r_vals), 8, 0, 0, put(s_valid), put(r_valid), 0)]
            d_tr, d_ts = put(np.zeros(n, dtype=U64)), put(np.zeros(n, dtype=U64))
            d_ms, d_mr, d_ks, d_kr = (put(np.zeros(want + 64, dtype=np.uint32)) for _ in range(4))
            ctx.reserve("prj", n, n, keepRowIds=True)
            ctx.key_hash2(desc, hj.HJ_KEY_SIDE_R, n, d_tr)
            ctx.prj_build(d_tr, n)
            ctx.key_hash2(desc, hj.HJ_KEY_SIDE_S, n, d_ts)
            ctx.prj_probe_pairs(d_ts, n, d_ms, d_mr, want + 64)
            n_pairs = ctx.pairs_info()[0]
            ctx.pairs_verify2(d_ms, d_mr, n_pairs, 0, n, n, desc, d_ks, d_kr, want + 64)
            kept, wrote, _us, dropped = ctx.verify_info()
            rejected = n_pairs - kept - dropped
            print("candidates", n_pairs, "expected", want, "kept", kept, "rejected", rejected, "dropped", dropped)
            assert kept + rejected + dropped == n_pairs == want
            assert (kept, wrote, dropped) == (kept_want, kept_want, 0)
        finally:
            for p in ptrs:
                ctx.dev_free(p)


def test_a_two_join_pipeline():
    """A left-join B gives a nullable column of B; joining it with C on that column is right only when its NULLs are
    NULLs. Through plain join_on the filler under them (all-zero bytes) matches C's real zeros: the reason for KeyColumn."""
    rng = np.random.default_rng(17)
    a_key = rng.integers(0, 600, 3000).astype(np.int64)                        # two thirds of A find no B
    b_key = rng.permutation(1000)[:200].astype(np.int64)
    b_ref = rng.integers(0, 50, 200).astype(np.int64)                          # B's reference to C: real zeros among them
    c_key = np.concatenate([np.arange(0, 40), [0, 0, 7]]).astype(np.int64)
    c_pay = {"c": np.arange(100, 100 + c_key.size, dtype=np.uint32)}
    ab = hj.join_on(b_key, a_key, r_cols={"ref": b_ref}, s_cols={"a": np.arange(3000, dtype=np.uint32)}, how="left")
    ref, ref_valid, a_row = ab["r"]["ref"], ab["r_valid"], ab["s"]["a"]
    assert ref.size >= 3000 and 1000 < (~ref_valid).sum() < 2900 and not ref[~ref_valid].any(), "the filler is all-zero bytes"
    assert (ref[ref_valid] == 0).any() and (c_key == 0).sum() == 3
    # the model: a row of A-B whose B side is NULL joins nothing
    table = {}
    for j, k in enumerate(c_key.tolist()):
        table.setdefault(k, []).append(j)
    want = sorted((int(a_row[i]), int(ref[i]), j) for i in range(ref.size) if ref_valid[i] for j in table.get(int(ref[i]), ()))
    assert want
    s_cols = {"a": a_row, "ref": ref}
    for slice_tuples in (None, 777):
        out = hj.join_on_columns(c_key, hj.KeyColumn(ref, valid=ref_valid), r_cols=c_pay, s_cols=s_cols, slice_tuples=slice_tuples)
        got = sorted(zip(out["s"]["a"].tolist(), out["s"]["ref"].tolist(), (out["r"]["c"] - 100).tolist()))
        assert got == want, slice_tuples
        assert np.array_equal(c_key[out["r_idx"]], out["s"]["ref"]) and ref_valid[out["s_idx"]].all()
    left = hj.join_on_columns(c_key, hj.KeyColumn(ref, valid=ref_valid), r_cols=c_pay, s_cols=s_cols, how="left")
    lone = ~left["r_valid"]
    assert set(np.flatnonzero(~ref_valid).tolist()) <= set(left["s_idx"][lone].tolist()), "every NULL-keyed row is an unmatched S row"
    # the same bytes through join_on: every filler row matches C's three zeros
    plain = hj.join_on(c_key, ref, r_cols=c_pay, s_cols=s_cols)
    assert plain["s_idx"].size == len(want) + 3 * int((~ref_valid).sum()) != len(want)
    assert sorted(zip(plain["s"]["a"].tolist(), plain["s"]["ref"].tolist(), (plain["r"]["c"] - 100).tolist())) != want
