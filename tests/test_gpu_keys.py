"""hj_key_hash_dev, hj_pairs_verify_dev / hj_verify_info and hj_mark_rows_dev / hj_mark_rows_info through ctypes -> C ABI
on an MI355X. Expected values come from numpy and from hj_key_hash_host (which test_keys_abi.py checks against the
header's wording without a GPU), never from the device. Every output plane and every marks plane has sentinel words around
it that must survive. Run with -m gpu.

hj_keys.hip: a workgroup of k_pairs_verify2 takes kFilterBlockPairs = 1024 consecutive candidates (hj_pairs.h), a
wavefront 256 of them as four steps of 64. hj_r_marks.hip: a workgroup of the sweep takes 256 words of a plane = 8192 rows."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from gpu_harness import SENTINEL, U64, Device, GuardedPlane, check_pair_filter, ctx, packed, plane_words, row_bits, status  # noqa: F401

pytestmark = pytest.mark.gpu

NO_ROW = 0xFFFFFFFF
GUARD = 64                      # sentinel words around a plane
N = 1 << 10                     # rows of the relations the candidates point into
CANDIDATES = 3 * 4096 + 17      # several workgroups, a ragged last one
PAIR = np.dtype([("a", np.uint64), ("b", np.uint64)])
WIDTH_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64, 16: PAIR}
INVALID = _lib.HJ_ERR_INVALID


def random_column(rng, width, n):
    return rng.integers(0, 256, size=n * width, dtype=np.uint8).view(WIDTH_DTYPES[width]).reshape(n).copy()


# ---- key_hash ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [(1,), (2,), (4,), (8,), (16,), (16, 1, 8, 2), (4, 16, 2, 8)])
def test_device_hash_equals_host_hash(ctx, widths):
    rng = np.random.default_rng(sum(widths))
    for n in (1, 63, 64, 65, 1023, 1025, 4097):
        cols = [random_column(rng, w, n) for w in widths]
        for side, mask in ((hj.HJ_KEY_SIDE_S, 0), (hj.HJ_KEY_SIDE_R, 0), (hj.HJ_KEY_SIDE_R, 0x3F), (hj.HJ_KEY_SIDE_S, 0xFFFF0000)):
            with Device(ctx) as dev:
                d_cols = [dev.put(c) for c in cols]
                out = GuardedPlane(dev, n, U64, 0xA5A5A5A5A5A5A5A5, behind=GUARD, what="a tuple behind the last row was written")
                # only the pointers of the side in use are given
                ctx.key_hash([(d, 0, w) if side == hj.HJ_KEY_SIDE_S else (0, d, w) for d, w in zip(d_cols, widths)], side, n, out.ptr, mask)
                got = out.read(n, (widths, n))
            assert np.array_equal(got, hj.key_hash_host(cols, key_mask=mask)), (widths, n, side, mask)


# ---- pairs_verify -----------------------------------------------------------------------------------------------------------
class Verify:
    """one hj_pairs_verify_dev over numpy inputs, checked in full against numpy"""

    def __init__(self, ctx, s_keys, r_keys, s_rows=None, r_rows=None):
        self.ctx, self.s_keys, self.r_keys = ctx, s_keys, r_keys
        self.s_rows = s_keys[0].size if s_rows is None else s_rows
        self.r_rows = r_keys[0].size if r_rows is None else r_rows

    def expected(self, map_s, map_r, base):
        s = (map_s.astype(np.int64) - base) % (1 << 32)
        r = map_r.astype(np.int64)
        ok = (map_s != NO_ROW) & (map_r != NO_ROW) & (s < self.s_rows) & (r < self.r_rows)
        keep = ok.copy()
        for a, b in zip(self.s_keys, self.r_keys):
            w = a.dtype.itemsize
            keep[ok] &= (a.view(np.uint8).reshape(-1, w)[s[ok]] == b.view(np.uint8).reshape(-1, w)[r[ok]]).all(axis=1)
        return keep, int((~ok).sum())

    def run(self, map_s, map_r, base=0, capacity=None, marks=True, offset=0, tag=None):
        """-> (kept S entries, kept R rows as written, S plane, R plane). capacity None: room for every candidate; offset:
        words the output planes start behind a 16-byte boundary. The marks planes start as SENTINEL-guarded zeros."""
        ctx, n = self.ctx, map_s.size
        keep, dropped = self.expected(map_s, map_r, base)
        kept = int(keep.sum())
        cap = n if capacity is None else capacity
        s = (map_s[keep].astype(np.int64) - base) % (1 << 32)
        want = {"kept": packed(map_s[keep], map_r[keep]), "info": (kept, min(kept, cap), 0, dropped),
                "s_marks": plane_words(row_bits(s, self.s_rows)), "r_marks": plane_words(row_bits(map_r[keep], self.r_rows))}
        with Device(ctx) as dev:
            cols = [(dev.put(a), dev.put(b), a.dtype.itemsize) for a, b in zip(self.s_keys, self.r_keys)]
            call = lambda ms, mr, os, o_r, c, ps, pr: ctx.pairs_verify(ms, mr, n, base, self.s_rows, self.r_rows, cols, os, o_r, c, ps, pr)      # noqa: E731
            got = check_pair_filter(dev, call, ctx.verify_info, map_s, map_r, self.s_rows, self.r_rows, want, cap, GUARD, offset=offset, marks=marks,
                                    tag=tag)
            # the relations are inputs as the maps are: untouched
            for (d_a, d_b, w), a, b in zip(cols, self.s_keys, self.r_keys):
                back_a, back_b = dev.get(d_a, a.size, a.dtype), dev.get(d_b, b.size, b.dtype)
                assert back_a.tobytes() == a.tobytes() and back_b.tobytes() == b.tobytes(), (tag, "a key column was written")
        return got


@pytest.fixture(scope="module")
def relations():
    """2^10-row relations with 64-bit keys: S row i and R row i hold the same key, keys differ above bit 32 only"""
    rng = np.random.default_rng(42)
    keys = (rng.permutation(N).astype(U64) << U64(32)) | U64(7)
    return [keys.copy()], [keys.copy()]


def candidates(rng, how, n=CANDIDATES):
    s = rng.integers(0, N, n).astype(np.uint32)
    r = s.copy()
    if how == "none":
        r = ((s + 1 + rng.integers(0, N - 1, n)) % N).astype(np.uint32)
    elif how == "half":
        flip = rng.random(n) < 0.5
        r[flip] = ((s[flip] + 1 + rng.integers(0, N - 1, int(flip.sum()))) % N).astype(np.uint32)
    return s, r


@pytest.mark.parametrize("how", ["all", "none", "half"])
def test_verify_keeps_exactly_the_equal_pairs(ctx, relations, how):
    s, r = candidates(np.random.default_rng(5), how)
    v = Verify(ctx, *relations)
    v.run(s, r, tag=how)
    v.run(s[:1], r[:1], tag=how + " one candidate")
    v.run(s + np.uint32(1000), r, base=1000, tag=how + " base 1000")
    v.run(s, r, offset=1, tag=how + " planes 4 bytes behind a 16-byte boundary")


def test_verify_cut_by_the_capacity_marks_like_the_uncut_call(ctx, relations):
    s, r = candidates(np.random.default_rng(6), "half")
    v = Verify(ctx, *relations)
    _, _, ps, pr = v.run(s, r, tag="uncut")
    for cap in (1, 1000, 4099):
        _, _, cs, cr = v.run(s, r, capacity=cap, offset=3, tag=f"capacity {cap}")
        assert np.array_equal(cs, ps) and np.array_equal(cr, pr), cap
    _, _, cs, cr = v.run(s, r, capacity=0, tag="mark only: capacity 0, NULL outputs")
    assert np.array_equal(cs, ps) and np.array_equal(cr, pr)
    v.run(s, r, marks=False, tag="no marks planes")


def test_verify_drops_null_and_out_of_range_candidates_unread(ctx):
    """the relations are windows of 1000 rows; the 24 rows behind them hold the keys that WOULD match"""
    rng = np.random.default_rng(8)
    keys = (rng.permutation(N).astype(U64) << U64(32)) | U64(9)
    rows = 1000
    s, r = candidates(rng, "half")
    s[rng.random(s.size) < 0.05] = NO_ROW
    r[rng.random(s.size) < 0.05] = NO_ROW
    v = Verify(ctx, [keys.copy()], [keys.copy()], s_rows=rows, r_rows=rows)
    keep, dropped = v.expected(s, r, 0)
    assert dropped > 1000 and ((s >= rows) & (s != NO_ROW)).any() and ((r >= rows) & (r != NO_ROW)).any() and keep.sum() > 1000
    v.run(s, r, tag="NULL and out of range")
    # under a base: entries below it wrap to large rows and are out of range too
    v.run(s + np.uint32(500), r, base=777, tag="base 777 over entries from 500")
    # a relation of no rows: everything is dropped, nothing is read (the column pointers may be NULL)
    with Device(ctx) as dev:
        d_s, d_r = dev.put(s), dev.put(r)
        ctx.pairs_verify(d_s, d_r, s.size, 0, 0, rows, [(0, dev.put(keys), 8)], 0, 0, 0)
        assert ctx.verify_info()[0::3] == (0, s.size)


@pytest.mark.parametrize("widths", [(16, 16, 16, 16), (1, 2, 4, 8), (8, 1, 16, 2), (2,), (1, 1)])
def test_verify_compares_every_column(ctx, widths):
    """R row i = S row i except that row i differs in exactly column i % (nCols + 1) (none for the last residue), in one byte"""
    rng = np.random.default_rng(sum(widths) + len(widths))
    s_keys = [random_column(rng, w, N) for w in widths]
    r_keys = [c.copy() for c in s_keys]
    for i in range(N):
        c = i % (len(widths) + 1)
        if c < len(widths):
            raw = r_keys[c].view(np.uint8).reshape(N, widths[c])
            raw[i, rng.integers(0, widths[c])] ^= np.uint8(1 << rng.integers(0, 8))
    s, r = candidates(rng, "all")
    v = Verify(ctx, s_keys, r_keys)
    keep, _ = v.expected(s, r, 0)
    assert 0 < keep.sum() < s.size
    v.run(s, r, tag=str(widths))


# ---- mark_rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 777])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 8191, 8193])
def test_mark_rows(ctx, rows, base):
    rng = np.random.default_rng(rows + base)
    bits = rng.random(rows) < 0.4
    words = -(-rows // 32)
    plane = np.full(words + GUARD, 0xFFFFFFFF, dtype=np.uint32)      # the words behind the plane are not rows
    plane[:words] = plane_words(bits)
    if rows % 32 and base == 0:          # ... nor are those of the last word (base 777: clear bits there are no rows either)
        plane[words - 1] |= np.uint32((0xFFFFFFFF << (rows % 32)) & 0xFFFFFFFF)
    with Device(ctx) as dev:
        d_plane = dev.put(plane)
        for which in (0, 1):
            want = (np.flatnonzero(bits == bool(which)) + base).astype(np.uint32)
            for cap in (rows + 5, max(want.size // 2, 1), 0):
                out = GuardedPlane(dev, cap, behind=GUARD) if cap else None
                ctx.mark_rows(d_plane, rows, base, which, out.ptr if cap else 0, cap)
                info = ctx.mark_rows_info()
                print("rows", rows, "base", base, "which", which, "capacity", cap, "info", info)
                written = min(want.size, cap)
                assert (info[0], info[1], info[3]) == (want.size, written, rows), (rows, base, which, cap, info)
                if cap:     # ascending: the first `capacity` rows, and no word behind them
                    assert np.array_equal(out.read(written, (rows, base, which, cap)), want[:written]), (rows, base, which, cap)
        assert np.array_equal(dev.get(d_plane, plane.size), plane), "the sweep wrote the plane"


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing_and_keep_the_infos(ctx, relations):
    s_keys, r_keys = relations
    s, r = candidates(np.random.default_rng(3), "half", 5000)
    Verify(ctx, s_keys, r_keys).run(s, r, tag="the call the infos speak of")
    with Device(ctx) as dev:
        d_plane = dev.put(plane_words(row_bits(np.arange(0, N, 3), N)))
        d_rows = dev.put(np.full(N, SENTINEL, dtype=np.uint32))
        ctx.mark_rows(d_plane, N, 0, 1, d_rows, N)
        before = ctx.verify_info(), ctx.mark_rows_info()
        d_ms, d_mr, d_k = dev.put(s), dev.put(r), dev.put(s_keys[0])
        d_out = dev.put(np.full(2 * N, SENTINEL, dtype=np.uint32))          # room for N tuples
        ok = [(d_k, d_k, 8)]
        big = 1 << 32

        def lib_cols(width=8, reserved=0, ptr=d_k):
            cols = (_lib.hj_key_col * 5)()
            for c in cols:
                c.s, c.r, c.width, c.reserved = ptr, ptr, width, reserved
            return cols

        h = ctx._h
        verify = lambda *a: hj.lib.hj_pairs_verify_dev(h, *a)       # noqa: E731
        bad = [
            hj.lib.hj_key_hash_dev(h, lib_cols(), 0, 0, N, 0, d_out), hj.lib.hj_key_hash_dev(h, lib_cols(), 5, 0, N, 0, d_out),
            hj.lib.hj_key_hash_dev(h, None, 1, 0, N, 0, d_out), hj.lib.hj_key_hash_dev(h, lib_cols(), 1, 2, N, 0, d_out),
            hj.lib.hj_key_hash_dev(h, lib_cols(width=3), 1, 0, N, 0, d_out), hj.lib.hj_key_hash_dev(h, lib_cols(reserved=1), 1, 0, N, 0, d_out),
            hj.lib.hj_key_hash_dev(h, lib_cols(ptr=None), 1, 0, N, 0, d_out), hj.lib.hj_key_hash_dev(h, lib_cols(ptr=d_k + 4), 1, 1, N, 0, d_out),
            hj.lib.hj_key_hash_dev(h, lib_cols(), 1, 0, N, 0, None), hj.lib.hj_key_hash_dev(h, lib_cols(), 1, 0, big, 0, d_out),
            verify(None, d_mr, 10, 0, N, N, lib_cols(), 1, None, None, 0, None, None),
            verify(d_ms, None, 10, 0, N, N, lib_cols(), 1, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, lib_cols(), 1, None, d_rows, 10, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, lib_cols(), 1, d_rows, None, 10, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, lib_cols(), 0, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, lib_cols(), 5, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, None, 1, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, lib_cols(width=12), 1, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, lib_cols(reserved=7), 1, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, lib_cols(ptr=None), 1, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, N, N, lib_cols(width=16, ptr=d_k + 8), 1, None, None, 0, None, None),
            verify(d_ms, d_mr, big, 0, N, N, lib_cols(), 1, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, big, N, lib_cols(), 1, None, None, 0, None, None),
            verify(d_ms, d_mr, 10, 0, N, big, lib_cols(), 1, None, None, 0, None, None),
            hj.lib.hj_mark_rows_dev(h, d_plane, N, 0, 2, d_rows, N), hj.lib.hj_mark_rows_dev(h, None, N, 0, 0, d_rows, N),
            hj.lib.hj_mark_rows_dev(h, d_plane, N, 0, 0, None, N), hj.lib.hj_mark_rows_dev(h, d_plane, big, 0, 0, d_rows, N),
            hj.lib.hj_mark_rows_dev(h, d_plane, N, 0xFFFFFFFF - N + 1, 0, d_rows, N),
            hj.lib.hj_verify_info(h, None), hj.lib.hj_mark_rows_info(h, None)]
        assert bad == [INVALID] * len(bad), bad
        assert status(ctx.key_hash, ok * 5, 0, N, d_out) == INVALID and status(ctx.mark_rows, d_plane, N, 0, 3, d_rows, N) == INVALID
        after = ctx.verify_info(), ctx.mark_rows_info()
        assert after == before, (before, after)
        assert after[0][0] > 0 and after[1][0] > 0
        rows3, got = np.arange(0, N, 3, dtype=np.uint32), dev.get(d_rows, N)
        assert (dev.get(d_out, 2 * N) == SENTINEL).all(), "a refused key_hash wrote tuples"
        assert np.array_equal(got[:rows3.size], rows3) and (got[rows3.size:] == SENTINEL).all(), "a refused call wrote rows"
        # rows 0 / nRows 0 / nPairs 0 need no pointers
        assert hj.lib.hj_key_hash_dev(h, lib_cols(ptr=None), 1, 0, 0, 0, None) == _lib.HJ_OK
        assert hj.lib.hj_mark_rows_dev(h, None, 0, 0, 0, None, 0) == _lib.HJ_OK and ctx.mark_rows_info() == (0, 0, ctx.mark_rows_info()[2], 0)
        assert verify(None, None, 0, 0, 0, 0, lib_cols(ptr=None), 1, None, None, 0, None, None) == _lib.HJ_OK
        assert ctx.verify_info()[0::3] == (0, 0)
