"""join_on on an MI355X: joins on 64-bit and composite keys through hash -> candidate join -> verify, all eight kinds, whole
and in slices, under a full and a crippled hash. The expected rows come from numpy: the inner pairs by sort + searchsorted
on a void view of the concatenated key bytes (bytewise equality, as join_on defines a match), the kinds derived from them,
the payload rows built with numpy indexing. Compared as multisets of rows (S payloads, R payloads and the two validity
flags), byte for byte. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj

from gpu_harness import alloc
from join_kinds_common import unmatched_rows
from join_on_common import PAIR, WEAK, check
from r_marks_common import U64, LOW, unmatched_r

pytestmark = pytest.mark.gpu

N = 1 << 12
HOWS = ("inner", "left", "semi", "anti", "right", "full", "right_semi", "right_anti")


def key_bytes(cols):
    """one void element per row: the bytes of its key columns, concatenated"""
    cols = [cols] if isinstance(cols, np.ndarray) else cols
    raw = np.concatenate([np.ascontiguousarray(c).view(np.uint8).reshape(c.size, c.dtype.itemsize) for c in cols], axis=1)
    return np.ascontiguousarray(raw).view(f"V{raw.shape[1]}").reshape(-1)


def inner_pairs(r_keys, s_keys):
    """all (i, j) with the key bytes of S row i == those of R row j, packed s << 32 | r and sorted"""
    R, S = key_bytes(r_keys), key_bytes(s_keys)
    order = np.argsort(R, kind="stable")
    Rs = R[order]
    lo = np.searchsorted(Rs, S, "left")
    cnt = np.searchsorted(Rs, S, "right") - lo
    total = int(cnt.sum())
    s_idx = np.repeat(np.arange(S.size, dtype=np.int64), cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    r_idx = order[np.repeat(lo, cnt) + within]
    return np.sort((s_idx.astype(U64) << U64(32)) | r_idx.astype(U64))


def candidate_count(r_keys, s_keys, key_mask):
    """pairs that agree on the masked join word: what the candidate join produces"""
    wr, ws = hj.key_hash_host(r_keys, key_mask=key_mask), hj.key_hash_host(s_keys, key_mask=key_mask)
    words, counts = np.unique(wr, return_counts=True)
    pos = np.searchsorted(words, ws)
    hit = (pos < words.size) & (words[np.minimum(pos, words.size - 1)] == ws)
    return int(counts[pos[hit]].sum())


@pytest.fixture(scope="module")
def data():
    """|R| = |S| = 2^12, uint64 keys. Pool A (1024 keys, probed) and pool C (1024 keys, only in S) share their low words
    pairwise and differ above them; pool B (512 keys) is only in the last quarter of R. Two payload columns per side."""
    rng = np.random.default_rng(2025)
    low = rng.permutation(np.unique(rng.integers(0, 1 << 32, 2000)))[:1536].astype(U64)
    hi_a = rng.integers(0, 1 << 31, 1024).astype(U64)
    A = low[:1024] | (hi_a << U64(32))
    C = low[:1024] | ((hi_a + U64(1) + rng.integers(0, 1 << 30, 1024).astype(U64)) << U64(32))
    B = low[1024:] | (rng.integers(1, 1 << 31, 512).astype(U64) << U64(32))
    R = np.concatenate([A[rng.integers(0, 1024, 3 * N // 4)], B[rng.integers(0, 512, N // 4)]])
    S = np.concatenate([rng.choice(R[:3 * N // 4], N // 2), C[rng.integers(0, 1024, N // 2)]])
    rng.shuffle(S)
    r16 = np.zeros(N, dtype=PAIR)
    r16["a"], r16["b"] = rng.integers(1, 1 << 62, N), rng.random(N)
    r_cols = {"r4": rng.integers(1, 1 << 31, N).astype(np.uint32), "r16": r16}
    s_cols = {"s2": rng.integers(1, 1 << 15, N).astype(np.int16), "s8": rng.random(N) + 1.0}
    inner = inner_pairs(R, S)
    # the properties the cases rest on
    keys = np.unique(np.concatenate([R, S]))
    lows, per_low = np.unique(keys & LOW, return_counts=True)
    shared = per_low[np.searchsorted(lows, keys & LOW)] > 1
    assert 4 * int(shared.sum()) >= keys.size, "a quarter of the distinct keys share their low word with a key that differs above it"
    assert np.unique(R).size < N, "R has duplicate keys"
    assert unmatched_rows(inner, N).size >= N // 2, "half of S is absent from R"
    assert unmatched_r(inner, N).size >= N // 4, "a quarter of R is never probed"
    assert inner.size > N // 2
    # a join on the low word alone would be wrong here
    assert inner_pairs((R & LOW).astype(np.uint32), (S & LOW).astype(np.uint32)).size > inner.size
    # under the weak mask the candidates are about 2^18, and the verify step rejects almost all of them
    weak = candidate_count(R, S, WEAK)
    print("inner pairs", inner.size, "candidates at full mask", candidate_count(R, S, 0), "under 0x3F", weak)
    assert 1 << 17 <= weak <= 1 << 19 and weak - inner.size > inner.size
    return R, S, r_cols, s_cols, inner


@pytest.mark.parametrize("key_mask", [0, WEAK])
@pytest.mark.parametrize("slice_tuples", [None, 1000])
@pytest.mark.parametrize("how", HOWS)
def test_join_on_64_bit_keys(data, how, slice_tuples, key_mask):
    """every kind; under the weak mask the verify step sees about 2^18 candidates and the result is the same one"""
    R, S, r_cols, s_cols, inner = data
    out = hj.join_on(R, S, r_cols=r_cols, s_cols=s_cols, how=how, slice_tuples=slice_tuples, key_mask=key_mask)
    check(out, how, inner, N, N, r_cols, s_cols, (how, slice_tuples, key_mask))


def test_verify_rejects_most_candidates_under_the_weak_mask(data):
    """the steps of join_on by hand on one context: the candidate join under 0x3F yields what the host count says, and
    verify_info splits it into the kept pairs and the rejected rest"""
    R, S, _, _, inner = data
    want = candidate_count(R, S, WEAK)
    with hj.HashJoinContext(0) as ctx:
        d_r, d_s, d_tr, d_ts = (alloc(ctx, 8 * N) for _ in range(4))
        d_ms, d_mr, d_ks, d_kr = (alloc(ctx, 4 * want) for _ in range(4))
        try:
            ctx.copy_h2d(d_r, R)
            ctx.copy_h2d(d_s, S)
            cols = [(d_s, d_r, 8)]
            ctx.reserve("prj", N, N, keepRowIds=True)
            ctx.key_hash(cols, hj.HJ_KEY_SIDE_R, N, d_tr, WEAK)
            ctx.prj_build(d_tr, N)
            ctx.key_hash(cols, hj.HJ_KEY_SIDE_S, N, d_ts, WEAK)
            ctx.prj_probe_pairs(d_ts, N, d_ms, d_mr, want)
            found, written = ctx.pairs_info()[:2]
            assert found == written == want
            ctx.pairs_verify(d_ms, d_mr, want, 0, N, N, cols, d_ks, d_kr, want)
            kept, wrote, _us, dropped = ctx.verify_info()
            print("candidates", want, "kept", kept, "rejected", want - kept - dropped)
            assert (kept, wrote, dropped) == (inner.size, inner.size, 0)
            assert want - kept - dropped > kept
            got_s, got_r = np.empty(kept, dtype=np.uint32), np.empty(kept, dtype=np.uint32)
            ctx.copy_d2h(got_s, d_ks)
            ctx.copy_d2h(got_r, d_kr)
            assert np.array_equal(np.sort((got_s.astype(U64) << U64(32)) | got_r.astype(U64)), inner)
        finally:
            for p in (d_r, d_s, d_tr, d_ts, d_ms, d_mr, d_ks, d_kr):
                ctx.dev_free(p)


@pytest.mark.parametrize("how", ["inner", "left", "anti", "right_anti"])
def test_a_true_32_bit_collision_is_no_match(how):
    """two distinct 64-bit keys with the same join word at full mask, one in R, the other in S, next to keys that match"""
    pool_bits = 18
    while True:
        pool = np.unique(np.random.default_rng(7).integers(0, 1 << 63, 1 << pool_bits, dtype=np.uint64))
        words = hj.key_hash_host(pool)
        order = np.argsort(words, kind="stable")
        twins = np.flatnonzero(words[order][1:] == words[order][:-1])
        if twins.size:
            break
        pool_bits += 1                  # a seed that gives none: a larger pool
    k_r, k_s = pool[order[twins[0]]], pool[order[twins[0] + 1]]
    assert k_r != k_s and hj.key_hash_host(np.array([k_r]))[0] == hj.key_hash_host(np.array([k_s]))[0]
    rng = np.random.default_rng(11)
    common = pool[(pool != k_r) & (pool != k_s)][:40]
    R = np.concatenate([common[:20], [k_r], common[10:30]]).astype(np.uint64)
    S = np.concatenate([common[5:25], [k_s], common[:8]]).astype(np.uint64)
    rng.shuffle(R)
    rng.shuffle(S)
    r_cols = {"r": np.arange(100, 100 + R.size, dtype=np.uint32)}
    s_cols = {"s": np.arange(500, 500 + S.size, dtype=np.uint64)}
    inner = inner_pairs(R, S)
    s_row, r_row = int(np.flatnonzero(S == k_s)[0]), int(np.flatnonzero(R == k_r)[0])
    assert inner.size and s_row not in (inner >> U64(32)) and r_row not in (inner & LOW)
    assert candidate_count(R, S, 0) > inner.size, "the collision is a candidate"
    out = hj.join_on(R, S, r_cols=r_cols, s_cols=s_cols, how=how)
    check(out, how, inner, R.size, S.size, r_cols, s_cols, ("collision", how))


KEY16 = np.dtype([("lo", np.uint64), ("hi", np.int64)])


@pytest.mark.parametrize("how", ["inner", "full"])
def test_composite_key(how):
    """(uint32, int16, 16-byte structured): S rows that agree with an R row in all three columns, and S rows that agree in
    two of them but not in the third -- for every choice of the third"""
    rng = np.random.default_rng(99)
    n = 600
    k16 = np.zeros(n, dtype=KEY16)
    k16["lo"], k16["hi"] = rng.integers(0, 1 << 63, n), rng.integers(-(1 << 62), 1 << 62, n)
    # few values per column: many rows agree in one or two columns by chance as well
    base = [rng.integers(0, 40, n).astype(np.uint32), rng.integers(-3, 4, n).astype(np.int16), k16[rng.integers(0, 50, n)]]
    R = [c.copy() for c in base]
    pick = rng.integers(0, n, 800)
    S = [c[pick].copy() for c in base]
    S[0][200:400] += np.uint32(1000)                     # differs in the first column only
    S[1][400:600] += np.int16(100)                       # ... the second
    S[2]["hi"][600:800] ^= np.int64(1) << np.int64(40)   # ... one bit of the third
    perm = rng.permutation(800)
    S = [c[perm] for c in S]
    r_cols = {"r": rng.integers(0, 1 << 62, n).astype(np.uint64)}
    s_cols = {"s1": rng.integers(0, 255, 800).astype(np.uint8), "s16": k16[rng.integers(0, n, 800)]}
    inner = inner_pairs(R, S)
    assert np.unique(inner >> U64(32)).size == 200 and unmatched_rows(inner, 800).size == 600 and inner.size > 200
    for drop in range(3):                                 # two columns alone would match more
        two = [c for i, c in enumerate(R) if i != drop], [c for i, c in enumerate(S) if i != drop]
        assert inner_pairs(*two).size > inner.size, drop
    for slice_tuples, key_mask in ((None, 0), (333, 0xFF)):
        out = hj.join_on(R, S, r_cols=r_cols, s_cols=s_cols, how=how, slice_tuples=slice_tuples, key_mask=key_mask)
        check(out, how, inner, n, 800, r_cols, s_cols, ("composite", how, slice_tuples, key_mask))
