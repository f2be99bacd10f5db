"""The pair-filter frame on an MI355X: hj_pairs_verify_dev, hj_pairs_verify2_dev with validity planes and hj_pairs_where_dev
with one EQ term share one shape (kFilter*, hj_pairs.h: map loads, drops, spare rows, stage, drop count, flush, marks around
a column or term loop), so one set of maps drives all three through its seams -- a step of 64 pairs, a wavefront's 256, a
workgroup's 1024, two workgroups plus one pair. Expected values come from numpy (and, for the condition, from
pairs_where_host as well), never from the device. The same file holds hj_key_hash_dev to the header's wording
(test_keys_abi.py's restatement) across the hash kernel's seams. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from join_kinds_common import SENTINEL, U64, Dev
from test_keys_abi import key_words, murmur3_words, random_column

pytestmark = pytest.mark.gpu

NO_ROW = 0xFFFFFFFF
GUARD = 64                      # sentinel words around a plane
ROWS = 300                      # sRows = rRows
BASE = 7                        # sRowBase
WORDS = -(-ROWS // 32)
N_PAIRS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
ENTRIES = ("verify", "verify2", "where")


@pytest.fixture(scope="module")
def ctx():
    c = hj.HashJoinContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def relations():
    """S row i and R row i hold the same 8-byte key, all keys distinct and different above bit 32; every 5th S row and every
    7th R row is NULL in the validity planes (which only hj_pairs_verify2_dev is given)"""
    rng = np.random.default_rng(2024)
    keys = (rng.permutation(ROWS).astype(U64) << U64(32)) | U64(11)
    valid_s, valid_r = np.arange(ROWS) % 5 != 4, np.arange(ROWS) % 7 != 6
    return keys, valid_s, valid_r


def plane_words(bits):
    padded = np.zeros(-(-bits.size // 32) * 32, dtype=bool)
    padded[:bits.size] = bits
    return np.packbits(padded, bitorder="little").view(np.uint32)


def maps_of(n):
    """n pairs: every 7th one of the five kinds of entry the frame drops unread, in turn; of the others about three in four
    point at two rows with the same key"""
    rng = np.random.default_rng(1000 + n)
    r = rng.integers(0, ROWS, n).astype(np.uint32)
    s = np.where(rng.random(n) < 0.75, r, rng.integers(0, ROWS, n)).astype(np.uint32) + np.uint32(BASE)
    for k in range(3, n, 7):
        kind = (k // 7) % 5
        if kind == 0:
            s[k] = NO_ROW
        elif kind == 1:
            r[k] = NO_ROW
        elif kind == 2:
            s[k] = BASE - 1                 # below the base: wraps far above sRows
        elif kind == 3:
            s[k] = BASE + ROWS              # at sRows exactly
        else:
            r[k] = ROWS                     # at rRows exactly
    return s, r


def expected(entry, relations, map_s, map_r, s_rows):
    """(kept mask, dropped count) by the header's wording"""
    keys, valid_s, valid_r = relations
    s = (map_s.astype(np.int64) - BASE) % (1 << 32)
    r = map_r.astype(np.int64)
    ok = (map_s != NO_ROW) & (map_r != NO_ROW) & (s < s_rows) & (r < ROWS)
    keep = ok.copy()
    keep[ok] = keys[s[ok]] == keys[r[ok]]
    if entry == "verify2":
        keep[ok] &= valid_s[s[ok]] & valid_r[r[ok]]
    return keep, int((~ok).sum())


def packed(s, r):
    return np.sort((s.astype(U64) << U64(32)) | r.astype(U64))


def guarded(words):
    return np.concatenate([np.full(GUARD, SENTINEL, np.uint32), np.zeros(words, np.uint32), np.full(GUARD, SENTINEL, np.uint32)])


def run(ctx, entry, relations, map_s, map_r, s_rows, capacity, tag):
    """one call of the entry point over the maps, checked in full: info, the written run, both planes, the guard words"""
    keys, valid_s, valid_r = relations
    n = map_s.size
    keep, dropped = expected(entry, relations, map_s, map_r, s_rows)
    kept = int(keep.sum())
    sw = -(-s_rows // 32)
    with Dev(ctx) as dev:
        d_ms, d_mr, d_ks, d_kr = dev.put(map_s), dev.put(map_r), dev.put(keys), dev.put(keys)
        fill = np.full(capacity + GUARD, SENTINEL, dtype=np.uint32)
        d_os, d_or = (dev.put(fill), dev.put(fill)) if capacity else (0, 0)
        plane_s, plane_r = guarded(sw), guarded(WORDS)
        d_ps, d_pr = dev.put(plane_s), dev.put(plane_r)
        args = (d_ms, d_mr, n, BASE, s_rows, ROWS)
        outs = (d_os, d_or, capacity, d_ps + 4 * GUARD if sw else 0, d_pr + 4 * GUARD)
        if entry == "verify":
            ctx.pairs_verify(*args, [(d_ks, d_kr, 8)], *outs)
            info = ctx.verify_info()
        elif entry == "verify2":
            d_vs, d_vr = dev.put(plane_words(valid_s)), dev.put(plane_words(valid_r))
            ctx.pairs_verify2(*args, [(d_ks, d_kr, 8, 0, 0, d_vs, d_vr, 0)], *outs)
            info = ctx.verify_info()
        else:
            ctx.pairs_where(*args, [(d_ks, d_kr, 8, _lib.HJ_VAL_UINT, _lib.CMP_OPS["=="])], *outs)
            info = ctx.where_info()
        print(tag, "info", info, "expected kept", kept, "dropped", dropped)
        assert (info[0], info[1], info[3]) == (kept, min(kept, capacity), dropped), (tag, info, kept, capacity, dropped)
        written = min(kept, capacity)
        got_s = got_r = np.empty(0, dtype=np.uint32)
        if capacity:
            out_s, out_r = dev.get(d_os, fill.size), dev.get(d_or, fill.size)
            assert (out_s[written:] == SENTINEL).all() and (out_r[written:] == SENTINEL).all(), (tag, "a word behind the run was written")
            got_s, got_r = out_s[:written], out_r[:written]
        got_ps, got_pr = dev.get(d_ps, plane_s.size), dev.get(d_pr, plane_r.size)
    for got, words in ((got_ps, sw), (got_pr, WORDS)):
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + words:] == SENTINEL).all(), (tag, "a word outside a marks plane was written")
    want_ps = plane_words(np.isin(np.arange(s_rows), map_s[keep].astype(np.int64) - BASE))
    want_pr = plane_words(np.isin(np.arange(ROWS), map_r[keep]))
    assert np.array_equal(got_ps[GUARD:GUARD + sw], want_ps), (tag, "S marks")
    assert np.array_equal(got_pr[GUARD:GUARD + WORDS], want_pr), (tag, "R marks")
    want, got = packed(map_s[keep], map_r[keep]), packed(got_s, got_r)
    if capacity >= kept:
        assert np.array_equal(got, want), (tag, "the kept pairs")
    else:                       # the capacity cuts: a sub-multiset of the kept pairs, `written` of them
        uniq, cnt = np.unique(want, return_counts=True)
        gu, gc = np.unique(got, return_counts=True)
        pos = np.minimum(np.searchsorted(uniq, gu), max(uniq.size - 1, 0))
        assert got.size == written and (uniq.size or not gu.size) and np.array_equal(uniq[pos], gu) and (gc <= cnt[pos]).all(), (tag, "cut")
    if entry == "where":        # the same code in a host loop
        host = hj.pairs_where_host(map_s, map_r, BASE, [(keys[:s_rows], "==", keys)], capacity=capacity, marks=True)
        assert host["info"] == (kept, written, 0, dropped), (tag, host["info"])
        assert np.array_equal(host["s_marks"], want_ps) and np.array_equal(host["r_marks"], want_pr), (tag, "host marks")
        if capacity >= kept:
            assert np.array_equal(packed(host["s_idx"], host["r_idx"]), got), (tag, "host pairs")
    return kept


@pytest.mark.parametrize("n", N_PAIRS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_frames_seams(ctx, relations, entry, n):
    map_s, map_r = maps_of(n)
    kept = run(ctx, entry, relations, map_s, map_r, ROWS, n, (entry, n, "capacity >= kept"))
    if n >= 63:
        assert 0.3 * n < kept < 0.7 * n, (entry, n, kept, "about half the pairs are to be kept")
    run(ctx, entry, relations, map_s, map_r, ROWS, max(kept - 1, 0), (entry, n, "capacity = kept - 1"))
    run(ctx, entry, relations, map_s, map_r, ROWS, 0, (entry, n, "capacity 0: the planes alone"))
    assert run(ctx, entry, relations, map_s, map_r, 0, n, (entry, n, "sRows 0: every pair dropped")) == 0


# ---- the hash ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [(1,), (2,), (4,), (8,), (16,), (16, 2, 8, 1)])
def test_device_hash_equals_the_headers_wording(ctx, widths):
    rng = np.random.default_rng(5 + sum(widths))
    for n in (1, 255, 256, 257, 1025):
        cols = [random_column(rng, w, n) for w in widths]
        for mask in (0, 0x3FF):
            with Dev(ctx) as dev:
                d_out = dev.put(np.full(n + GUARD, 0xA5A5A5A5A5A5A5A5, dtype=U64))
                ctx.key_hash([(dev.put(c), 0, w) for c, w in zip(cols, widths)], hj.HJ_KEY_SIDE_S, n, d_out, mask)
                got = np.empty(n + GUARD, dtype=U64)
                ctx.copy_d2h(got, d_out)
            assert (got[n:] == 0xA5A5A5A5A5A5A5A5).all(), (widths, n, "a tuple behind the last row was written")
            assert np.array_equal(got[:n], murmur3_words(key_words(cols), mask)), (widths, n, mask)
