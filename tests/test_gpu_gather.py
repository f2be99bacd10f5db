"""hj_gather_dev / hj_gather_info through ctypes -> C ABI on an MI355X. Expected values come from numpy, never from the
library; the copies are exact, so every comparison is byte for byte. Every output buffer and every validity plane has
sentinel bytes behind its end that must survive. Run with -m gpu.

hj_gather.hip: a wavefront step is kGatherStepRows = 64 rows (two validity words), a lane holds kGatherLaneRows = 4 rows
that lie one step apart, a wavefront therefore 256 consecutive rows and a workgroup of 4 wavefronts kGatherBlockRows = 1024."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from gather_common import (BIG, BLOCK_ROWS, GUARD_BYTES, GUARD_WORDS, NO_ROW, SEAM_ROWS, STEP_ROWS, WIDTHS, _null_patterns, column, expected,
                           fill_of)
from gpu_harness import SENTINEL, U64, Device, GuardedPlane, ctx, plane_bits, plane_words  # noqa: F401
from join_kinds_common import planes, unmatched_rows
from r_marks_common import LEFT, UNMATCHED, inner_expected, unmatched_r

pytestmark = pytest.mark.gpu


class Gather:
    """one hj_gather_dev over numpy inputs, checked in full against numpy: columns = [(src array of V<width> or None, width,
    fill)]; d_srcs overrides the device sources (windows into larger allocations)"""

    def __init__(self, ctx, dev):
        self.ctx, self.dev = ctx, dev

    def run(self, m, src_rows, columns, row_base=0, with_valid=True, d_srcs=None, valid_offset=0, tag=None):
        ctx, dev, n = self.ctx, self.dev, m.size
        d_map = dev.put(m)
        if d_srcs is None:
            d_srcs = [dev.put(src) if src is not None and src.size else 0 for src, _, _ in columns]
        dsts = [GuardedPlane(dev, n * w, np.uint8, 0xA5, behind=GUARD_BYTES, what="a byte behind the column's end was written") for _, w, _ in columns]
        words = (n + 31) // 32
        valid = GuardedPlane(dev, words, front=valid_offset, behind=1 + GUARD_WORDS - valid_offset,
                             what="a validity word outside ceil(n / 32) was written") if with_valid else None
        ctx.gather(d_map, n, src_rows, [(s, d.ptr, w, f) for s, d, (_, w, f) in zip(d_srcs, dsts, columns)],
                   d_valid=valid.ptr if with_valid else 0, row_base=row_base)
        info = ctx.gather_info()
        got = []
        want_ok, n_null, n_oor = expected(m, row_base, src_rows, None, 1, bytes(16))[1:] if not columns else (None, 0, 0)
        for (src, w, f), d in zip(columns, dsts):
            want, want_ok, n_null, n_oor = expected(m, row_base, src_rows, src, w, f)
            raw = d.read(n * w, (tag, w))
            assert raw.tobytes() == want.tobytes(), (tag, w, n)
            got.append(raw.view(f"V{w}"))
        print(tag, "rows", n, "info", info)
        assert (info[0], info[1], info[3]) == (n, n_null, n_oor), (tag, info, n, n_null, n_oor)
        if with_valid:
            # whole words: the bits at or behind n in the last one are zero
            assert np.array_equal(valid.read(words, tag), plane_words(want_ok)), (tag, n)
        dev.free(d_map, *[d.base for d in dsts], *([valid.base] if with_valid else []))
        return got


# ---------------------------------------------------------------------------------------------------------------------
# seams: every width at every row count around a step, a wavefront and a workgroup
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_seams(ctx, width):
    rng = np.random.default_rng(100 + width)
    src_rows = 777
    src = column(rng, src_rows, width)
    with Device(ctx) as dev:
        g = Gather(ctx, dev)
        d_src = dev.put(src)
        for n in SEAM_ROWS:
            m = rng.integers(0, src_rows, n).astype(np.uint32)          # a random map, repeats included
            g.run(m, src_rows, [(src, width, fill_of(width, 1))], d_srcs=[d_src], tag=("seams", width, n))


def test_validity_plane_at_a_4_byte_boundary(ctx):
    """the plane one word into its allocation: its 8-byte stores must not reach the word in front or the words behind"""
    rng = np.random.default_rng(7)
    src = column(rng, 500, 4)
    with Device(ctx) as dev:
        for n in (33, STEP_ROWS + 1, BLOCK_ROWS + 1, BIG):
            m = rng.integers(0, 500, n).astype(np.uint32)
            m[rng.integers(0, n, n // 3)] = NO_ROW
            Gather(ctx, dev).run(m, 500, [(src, 4, fill_of(4, 2))], valid_offset=1, tag=("valid+4", n))


# ---------------------------------------------------------------------------------------------------------------------
# NULL rows, in an 8-byte and a 1-byte column with a fill pattern each
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [BIG, STEP_ROWS + 1])
def test_null_rows(ctx, n):
    rng = np.random.default_rng(n)
    src_rows = 1000
    src8, src1 = column(rng, src_rows, 8), column(rng, src_rows, 1)
    cols = [(src8, 8, fill_of(8, 3)), (src1, 1, fill_of(1, 4))]
    with Device(ctx) as dev:
        g = Gather(ctx, dev)
        for name, null in _null_patterns(BIG):
            null = null[:n].copy()
            m = rng.integers(0, src_rows, n).astype(np.uint32)
            m[null] = NO_ROW
            got = g.run(m, src_rows, cols, tag=("nulls", name, n))
            assert got[0][null].tobytes() == fill_of(8, 3)[:8] * int(null.sum())
            assert got[1][null].tobytes() == fill_of(1, 4)[:1] * int(null.sum())
        # every row NULL needs no source at all
        m = np.full(n, NO_ROW, dtype=np.uint32)
        g.run(m, 0, [(None, 8, fill_of(8, 5)), (None, 1, fill_of(1, 6))], d_srcs=[0, 0], tag=("nulls", "no source", n))


# ---------------------------------------------------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------------------------------------------------
def test_eight_columns_in_one_call_equal_eight_calls(ctx):
    rng = np.random.default_rng(8)
    widths = (1, 2, 4, 8, 16, 16, 8, 4)
    src_rows, n = 2000, BIG
    cols = [(column(rng, src_rows, w), w, fill_of(w, 10 + k)) for k, w in enumerate(widths)]
    m = rng.integers(0, src_rows, n).astype(np.uint32)
    m[rng.integers(0, n, n // 5)] = NO_ROW
    with Device(ctx) as dev:
        g = Gather(ctx, dev)
        together = g.run(m, src_rows, cols, tag="eight columns")
        for k, col in enumerate(cols):
            alone = g.run(m, src_rows, [col], tag=("one column", k))
            assert alone[0].tobytes() == together[k].tobytes(), k
        # the instantiations between one column and eight, mixed widths and one width
        for cut in (2, 3, 4, 5):
            g.run(m, src_rows, cols[:cut], tag=("mixed", cut))
        for w in WIDTHS:
            same = [(column(rng, src_rows, w), w, fill_of(w, 30 + k)) for k in range(8)]
            for cut in (2, 4, 7, 8):
                g.run(m, src_rows, same[:cut], tag=("one width", w, cut))


def test_validity_plane_alone_and_no_validity_plane(ctx):
    rng = np.random.default_rng(9)
    src = column(rng, 300, 2)
    with Device(ctx) as dev:
        g = Gather(ctx, dev)
        for n in (1, STEP_ROWS + 1, BIG):
            m = rng.integers(0, 300, n).astype(np.uint32)
            m[::3] = NO_ROW
            m[1::7] = 300 + 5                                   # out of range: no bit either
            g.run(m, 300, [], tag=("validity alone", n))        # nCols 0
            g.run(m, 300, [(src, 2, fill_of(2, 7))], with_valid=False, tag=("no validity", n))


# ---------------------------------------------------------------------------------------------------------------------
# map shapes; the row base
# ---------------------------------------------------------------------------------------------------------------------
def test_map_shapes(ctx):
    rng = np.random.default_rng(10)
    n = BIG
    src = column(rng, 3 * n, 8)
    maps = {"identity": np.arange(n), "reverse": np.arange(n)[::-1], "one source row": np.full(n, 1234),
            "ascending with gaps": np.cumsum(rng.integers(1, 4, n)) - 1}
    with Device(ctx) as dev:
        g = Gather(ctx, dev)
        for name, m in maps.items():
            assert m.max() < 3 * n
            g.run(np.ascontiguousarray(m, dtype=np.uint32), 3 * n, [(src, 8, fill_of(8, 8)), (src.view("V4")[:3 * n], 4, fill_of(4, 9))],
                  tag=name)


def test_row_base(ctx):
    """the entries come back minus the base; HJ_NO_ROW stays NULL whatever the base (also a base that would make it a row)"""
    rng = np.random.default_rng(11)
    n, src_rows = 2 * BLOCK_ROWS + 5, 900
    src = column(rng, src_rows, 8)
    with Device(ctx) as dev:
        g = Gather(ctx, dev)
        for base in (5000, NO_ROW - 10):
            m = (rng.integers(0, min(src_rows, NO_ROW - base), n) + base).astype(np.uint32)
            m[::5] = NO_ROW
            got = g.run(m, src_rows, [(src, 8, fill_of(8, 12))], row_base=base, tag=("row base", base))
            ok = m != NO_ROW
            assert got[0][ok].tobytes() == src[m[ok].astype(np.int64) - base].tobytes()


def test_out_of_range_entries_are_never_read(ctx):
    """The source is a window in the middle of a larger allocation, so that even a kernel that did read an out-of-range
    entry would stay inside this test's own buffer: src points 4096 elements in, srcRows is 100, the entries reach 2000 rows
    above the window and, under rowBase 3000, 2000 rows below it."""
    rng = np.random.default_rng(12)
    width, lead, src_rows, n = 8, 4096, 100, 2 * BLOCK_ROWS + 33
    whole = column(rng, 2 * lead, width)
    src = whole[lead:lead + src_rows]
    with Device(ctx) as dev:
        g = Gather(ctx, dev)
        d_whole = dev.put(whole)
        d_src = d_whole + lead * width
        for base, ranges in ((0, [(100, 2000)]), (3000, [(3100, 5000), (1000, 3000)])):
            m = (rng.integers(0, src_rows, n) + base).astype(np.uint32)
            stray = rng.random(n) < 0.4
            lo, hi = zip(*ranges)
            pick = rng.integers(0, len(ranges), n)
            m[stray] = rng.integers(np.array(lo)[pick], np.array(hi)[pick])[stray]
            m[::11] = NO_ROW
            n_stray = int((stray & (m != NO_ROW)).sum())
            assert n_stray > 100
            got = g.run(m, src_rows, [(src, width, fill_of(width, 13))], row_base=base, d_srcs=[d_src], tag=("out of range", base))
            assert ctx.gather_info()[3] == n_stray and ctx.gather_info()[1] == int((m == NO_ROW).sum())
            assert got[0][stray].tobytes() == fill_of(width, 13)[:width] * int(stray.sum())


# ---------------------------------------------------------------------------------------------------------------------
# refused calls
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(ctx):
    rng = np.random.default_rng(13)
    n, src_rows = 100, 50
    m = rng.integers(0, src_rows, n).astype(np.uint32)
    src = column(rng, src_rows, 16)
    with Device(ctx) as dev:
        d_map, d_src = dev.put(m), dev.put(src)
        dst, valid = GuardedPlane(dev, n * 16, np.uint8, 0xA5, behind=GUARD_BYTES), GuardedPlane(dev, 4, behind=GUARD_WORDS)
        d_dst, d_valid = dst.ptr, valid.ptr
        ctx.gather(d_map, n, src_rows, [(d_src, d_dst, 4, 0)])          # a call to remember
        before = ctx.gather_info()
        assert before[0] == n
        ctx.copy_h2d(d_dst, np.full(n * 16 + GUARD_BYTES, 0xA5, dtype=np.uint8))

        def raw(d_map_, n_rows, row_base, rows, cols, n_cols, valid):
            arr = (_lib.hj_gather_col * max(len(cols), 1))()
            for c, (s, d, w, reserved) in zip(arr, cols):
                c.src, c.dst, c.width, c.reserved = s or None, d or None, w, reserved
            return hj.lib.hj_gather_dev(ctx._h, d_map_ or None, n_rows, row_base, rows, arr if cols else None,
                                        n_cols, valid or None)

        one = [(d_src, d_dst, 8, 0)]
        refused = {
            "nine columns": (d_map, n, 0, src_rows, one * 9, 9, d_valid),
            "width 3": (d_map, n, 0, src_rows, [(d_src, d_dst, 3, 0)], 1, d_valid),
            "width 0": (d_map, n, 0, src_rows, [(d_src, d_dst, 0, 0)], 1, d_valid),
            "width 32": (d_map, n, 0, src_rows, [(d_src, d_dst, 32, 0)], 1, d_valid),
            "a bad width behind a good one": (d_map, n, 0, src_rows, one + [(d_src, d_dst, 5, 0)], 2, d_valid),
            "reserved": (d_map, n, 0, src_rows, [(d_src, d_dst, 8, 1)], 1, d_valid),
            "src NULL": (d_map, n, 0, src_rows, [(0, d_dst, 8, 0)], 1, d_valid),
            "dst NULL": (d_map, n, 0, src_rows, [(d_src, 0, 8, 0)], 1, d_valid),
            "dst NULL without rows to read": (d_map, n, 0, 0, [(0, 0, 8, 0)], 1, d_valid),
            "map NULL": (0, n, 0, src_rows, one, 1, d_valid),
            "cols NULL": (d_map, n, 0, src_rows, [], 1, d_valid),
            "nRows 2^32": (d_map, 1 << 32, 0, src_rows, one, 1, d_valid),
            "srcRows 2^32": (d_map, n, 0, 1 << 32, one, 1, d_valid),
            "nothing to write": (d_map, n, 0, src_rows, [], 0, 0),
        }
        for w in (2, 4, 8, 16):                                  # src or dst not aligned to the width
            refused[f"src + 1, width {w}"] = (d_map, n, 0, src_rows, [(d_src + 1, d_dst, w, 0)], 1, d_valid)
            refused[f"dst + {w // 2}, width {w}"] = (d_map, n, 0, src_rows, [(d_src, d_dst + w // 2, w, 0)], 1, d_valid)
        for name, args in refused.items():
            assert raw(*args) == _lib.HJ_ERR_INVALID, name
            assert ctx.gather_info() == before, name
        # nRows 0 is a no-op, whatever else is given
        assert raw(d_map, 0, 0, src_rows, one, 1, d_valid) == _lib.HJ_OK
        assert raw(0, 0, 0, 0, [], 0, 0) == _lib.HJ_OK
        assert ctx.gather_info() == before
        dst.read(0, "a refused call wrote a byte")
        valid.read(0, "a refused call wrote a validity word")
        # and the context still gathers
        Gather(ctx, dev).run(m, src_rows, [(src, 16, fill_of(16, 14))], tag="after the refused calls")


def test_info_is_zero_before_the_first_call():
    with hj.HashJoinContext(0) as fresh:
        assert fresh.gather_info() == (0, 0, 0, 0)
        with Device(fresh) as dev:
            Gather(fresh, dev).run(np.arange(5, dtype=np.uint32), 5, [(np.arange(5, dtype=np.uint64).view("V8"), 8, bytes(16))],
                                   tag="no reserve, no table")
        assert fresh.gather_info()[0] == 5


# ---------------------------------------------------------------------------------------------------------------------
# the library's own maps, left on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_the_librarys_own_maps(ctx, algo):
    """LEFT probe with idxBase 5000 and sIdxBase 77777, then the unmatched R rows; the key tuples of S and R themselves are
    the 8-byte columns, the bases the rowBase. The maps never leave the device on their way into the gather."""
    n, r_base, s_base = 1 << 12, 5000, 77777
    rng = np.random.default_rng(14)
    R = hj.generate_data("uniform", n, n, 16)                           # duplicate keys
    S = np.concatenate([rng.choice(R[:3 * n // 4], n // 2), np.arange(n + 1, n + 1 + n // 2, dtype=U64)])
    rng.shuffle(S)
    inner = inner_expected(algo, R, S, r_base=r_base, s_base=s_base)
    no_match = unmatched_rows(inner, S.size, s_base)
    r_only = unmatched_r(inner, n, r_base)
    assert inner.size and no_match.size >= n // 2 and r_only.size >= n // 8
    rows = inner.size + no_match.size
    with Device(ctx) as dev:
        ctx.reserve(algo, n, S.size, keepRowIds=True, trackRMatches=True)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, n, r_base)
        d_s, d_r = (p.ptr for p in planes(dev, rows))
        ctx.probe_pairs(dS, S.size, d_s, d_r, rows, s_idx_base=s_base, kind=LEFT)
        assert ctx.pairs_info()[:2] == (rows, rows)
        d_rows = dev.put(np.full(n, SENTINEL, dtype=np.uint32))
        ctx.r_rows(UNMATCHED, d_rows, n)
        assert ctx.r_rows_info()[:2] == (r_only.size, r_only.size)

        def gather(d_map, n_rows, d_src, src_rows, base):
            d_dst, d_valid = dev.alloc(8 * n_rows), dev.alloc(4 * ((n_rows + 31) // 32))
            ctx.gather(d_map, n_rows, src_rows, [(d_src, d_dst, 8, 0)], d_valid=d_valid, row_base=base)
            info = ctx.gather_info()
            assert info[0] == n_rows and info[3] == 0, info
            keys, words = np.empty(n_rows, dtype=U64), np.empty((n_rows + 31) // 32, dtype=np.uint32)
            ctx.copy_d2h(keys, d_dst)
            ctx.copy_d2h(words, d_valid)
            return keys, plane_bits(words, n_rows), info

        s_keys, s_valid, s_info = gather(d_s, rows, dS, S.size, s_base)
        r_keys, r_valid, r_info = gather(d_r, rows, dR, n, r_base)
        t_keys, t_valid, t_info = gather(d_rows, r_only.size, dR, n, r_base)
        s_map = dev.get(d_s, rows).astype(np.int64) - s_base
    assert s_valid.all() and s_info[1] == 0 and np.array_equal(s_keys, S[s_map])
    assert r_info[1] == no_match.size == int((~r_valid).sum())
    assert np.array_equal(s_keys[r_valid], r_keys[r_valid]) and (r_keys[~r_valid] == 0).all()
    assert np.array_equal(np.sort(s_map[~r_valid]), (no_match - U64(s_base)).astype(np.int64))
    assert t_valid.all() and t_info[1] == 0 and np.array_equal(t_keys, R[(r_only - U64(r_base)).astype(np.int64)])
