"""The pair-filter frame on an MI355X: hj_pairs_verify_dev, hj_pairs_verify2_dev with validity planes and hj_pairs_where_dev
with one EQ term share one shape (kFilter*, hj_pairs.h: map loads, drops, spare rows, stage, drop count, flush, marks around
a column or term loop), so one set of maps drives all three through its seams -- a step of 64 pairs, a wavefront's 256, a
workgroup's 1024, two workgroups plus one pair. Expected values come from numpy (and, for the condition, from
pairs_where_host as well), never from the device. The same file holds hj_key_hash_dev to the header's wording
(keys_common.py's restatement) across the hash kernel's seams. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from gpu_harness import U64, Device, GuardedPlane, check_pair_filter, ctx, packed, plane_words  # noqa: F401
from keys_common import key_words, murmur3_words, random_column

pytestmark = pytest.mark.gpu

NO_ROW = 0xFFFFFFFF
GUARD = 64                      # sentinel words around a plane
ROWS = 300                      # sRows = rRows
BASE = 7                        # sRowBase
WORDS = -(-ROWS // 32)
N_PAIRS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
ENTRIES = ("verify", "verify2", "where")


@pytest.fixture(scope="module")
def relations():
    """S row i and R row i hold the same 8-byte key, all keys distinct and different above bit 32; every 5th S row and every
    7th R row is NULL in the validity planes (which only hj_pairs_verify2_dev is given)"""
    rng = np.random.default_rng(2024)
    keys = (rng.permutation(ROWS).astype(U64) << U64(32)) | U64(11)
    valid_s, valid_r = np.arange(ROWS) % 5 != 4, np.arange(ROWS) % 7 != 6
    return keys, valid_s, valid_r


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


def run(ctx, entry, relations, map_s, map_r, s_rows, capacity, tag):
    """one call of the entry point over the maps, checked in full: info, the written run, both planes, the guard words"""
    keys, valid_s, valid_r = relations
    n = map_s.size
    keep, dropped = expected(entry, relations, map_s, map_r, s_rows)
    kept = int(keep.sum())
    want = {"kept": packed(map_s[keep], map_r[keep]), "info": (kept, min(kept, capacity), 0, dropped),
            "s_marks": plane_words(np.isin(np.arange(s_rows), map_s[keep].astype(np.int64) - BASE)),
            "r_marks": plane_words(np.isin(np.arange(ROWS), map_r[keep]))}
    host = None
    if entry == "where":        # the same code in a host loop
        host = lambda: hj.pairs_where_host(map_s, map_r, BASE, [(keys[:s_rows], "==", keys)], capacity=capacity, marks=True)      # noqa: E731
    with Device(ctx) as dev:
        d_ks, d_kr = dev.put(keys), dev.put(keys)
        if entry == "verify":
            filter_, info, cols = ctx.pairs_verify, ctx.verify_info, [(d_ks, d_kr, 8)]
        elif entry == "verify2":
            filter_, info, cols = ctx.pairs_verify2, ctx.verify_info, [(d_ks, d_kr, 8, 0, 0, dev.put(plane_words(valid_s)), dev.put(plane_words(valid_r)), 0)]
        else:
            filter_, info, cols = ctx.pairs_where, ctx.where_info, [(d_ks, d_kr, 8, _lib.HJ_VAL_UINT, _lib.CMP_OPS["=="])]
        call = lambda ms, mr, os, o_r, c, ps, pr: filter_(ms, mr, n, BASE, s_rows, ROWS, cols, os, o_r, c, ps if s_rows else 0, pr)      # noqa: E731
        check_pair_filter(dev, call, info, map_s, map_r, s_rows, ROWS, want, capacity, GUARD, host=host, tag=tag)
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
            with Device(ctx) as dev:
                out = GuardedPlane(dev, n, U64, 0xA5A5A5A5A5A5A5A5, behind=GUARD, what="a tuple behind the last row was written")
                ctx.key_hash([(dev.put(c), 0, w) for c, w in zip(cols, widths)], hj.HJ_KEY_SIDE_S, n, out.ptr, mask)
                got = out.read(n, (widths, n))
            assert np.array_equal(got, murmur3_words(key_words(cols), mask)), (widths, n, mask)
