"""hj_gather2_dev / hj_gather2_info through ctypes -> C ABI on an MI355X: payload columns in the Arrow layout, a source
validity plane and 32-bit offsets per column. Expected values come from numpy and plain Python, never from the library;
the copies are exact, so every comparison is byte for byte. Every output buffer, offsets array and validity plane has
sentinel bytes in front of it and behind it that must survive. Run with -m gpu.

hj_gather.hip: the row-to-lane layout is k_gather's (test_gpu_gather.py: steps of 64 rows, 256 per wavefront, 1024 per
workgroup). The copy of a variable-length column is driven by the output: a lane assembles one 16-byte block of the
destination (COPY_BLOCK_BYTES), a workgroup walks the output range of its 1024 rows in passes of 256 such blocks
(COPY_PASS_BYTES). There is no LDS tile an element could overflow and no threshold above which a wavefront takes an
element over from a lane: an element longer than a block is copied by as many lanes as it has blocks, one longer than a
pass in several passes. The long-element tests put an element just above each of the two constants."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from gather_common import (BIG, BLOCK_ROWS, GUARD_WORDS, NO_ROW, SEAM_ROWS, STEP_ROWS, WAVE_ROWS, WIDTHS, _null_patterns, column, fill_of, fixed,
                           rows_of, strings, want_of)
from gather_common import expected as plain_expected
from gpu_harness import SENTINEL, Device, GuardedPlane, ctx, plane_words  # noqa: F401
from keys2_common import LENGTHS

pytestmark = pytest.mark.gpu

COPY_BLOCK_BYTES = 16
COPY_PASS_BYTES = 256 * COPY_BLOCK_BYTES
GUARD = 256                      # bytes in front of and behind every output (a multiple of 16: the alignment stays)
SENT = 0xA5


class Gather2:
    """one hj_gather2_dev over numpy inputs, checked in full. Columns are the dicts fixed() / strings() make; further
    keys: capacity (variable length: dstCapacity; None = exactly the total), dst_lead (bytes the dst is moved off its
    16-byte alignment), dst_valid_offset (words the dstValid plane lies into its allocation), d_src (device pointers
    (values, offsets, validity) that override the upload)."""

    def __init__(self, ctx, dev):
        self.ctx, self.dev = ctx, dev

    def run(self, m, src_rows, cols, row_base=0, with_valid=True, valid_offset=0, tag=None):
        ctx, dev, n = self.ctx, self.dev, m.size
        i, null, oor, ok = rows_of(m, row_base, src_rows)
        words = (n + 31) // 32
        d_map = dev.put(m)
        valid = GuardedPlane(dev, words, front=valid_offset, behind=1 + GUARD_WORDS - valid_offset, what="dValid guard") if with_valid else None
        descs, wants, held = [], [], [d_map] + ([valid.base] if with_valid else [])
        for col in cols:
            el, raw, off = want_of(col, i, ok, n)
            total = len(raw) if not col["width"] else 0
            cap = total if col.get("capacity") is None else col["capacity"]
            room = n * col["width"] if col["width"] else cap
            lead = col.get("dst_lead", 0)
            if "d_src" in col:
                d_values, d_off, d_ok = col["d_src"]
            else:
                d_values = dev.put(col["src"] if col["width"] else col["data"]) if src_rows else 0
                d_off = dev.put(col["offsets"].astype(np.uint32)) if not col["width"] else 0
                d_ok = dev.put(plane_words(col["valid"])) if col["valid"] is not None else 0
                held += [p for p in (d_values, d_off, d_ok) if p]
            dst = GuardedPlane(dev, room, np.uint8, SENT, front=GUARD + lead, behind=GUARD, what="a byte outside the column's output was written")
            doff = GuardedPlane(dev, n + 1, front=GUARD_WORDS, behind=GUARD_WORDS, what="dstOffsets guard") if not col["width"] else None
            vo = col.get("dst_valid_offset", 0)
            dvalid = GuardedPlane(dev, words, front=vo, behind=1 + GUARD_WORDS - vo, what="dstValid guard") if col["dst_valid"] else None
            held += [p.base for p in (dst, doff, dvalid) if p]
            null_dst = not col["width"] and cap == 0 and col.get("null_dst", False)
            descs.append(dict(src=d_values, dst=0 if null_dst else dst.ptr, width=col["width"], fill=col.get("fill", 0),
                              src_offsets=d_off, dst_offsets=doff.ptr if doff else 0, src_valid=d_ok,
                              dst_valid=dvalid.ptr if dvalid else 0, dst_capacity=0 if col["width"] else cap))
            wants.append((el, raw, off, total, cap, room, dst, doff, dvalid))
        ctx.gather2(d_map, n, src_rows, descs, d_valid=valid.ptr if with_valid else 0, row_base=row_base)
        info = ctx.gather2_info()
        print(tag, "rows", n, "info", info)
        assert info[:2] == (n, int(null.sum())) and info[3] == int(oor.sum()), (tag, info, n, int(null.sum()), int(oor.sum()))
        assert info[4:] == tuple([w[3] for w in wants] + [0] * (8 - len(wants))), (tag, info)
        if with_valid:
            assert np.array_equal(valid.read(words, tag), plane_words(ok)), (tag, "dValid")
        got = []
        for col, (el, raw, off, total, cap, room, dst, doff, dvalid) in zip(cols, wants):
            kept = room if col["width"] else min(total, cap)
            body = dst.read(kept, (tag, col["width"]))
            assert body.tobytes() == raw[:kept], (tag, col["width"], n, "bytes")
            if doff:
                assert np.array_equal(doff.read(n + 1, tag).astype(np.int64), off), (tag, "dstOffsets")
            if dvalid:
                assert np.array_equal(dvalid.read(words, tag), plane_words(el)), (tag, "dstValid")
            got.append((body.tobytes(), None if off is None else off.copy(), el))
        dev.free(*held)
        return got


def cycled_lengths(rows, shift=3):
    return [LENGTHS[(k * 7 + shift) % len(LENGTHS)] for k in range(rows)]


# ---------------------------------------------------------------------------------------------------------------------
# row seams, every length, every pair of alignments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_row_seams_lengths_and_alignments(ctx, lead):
    rng = np.random.default_rng(200 + lead)
    src_rows = 150
    col = strings(rng, cycled_lengths(src_rows), lead=lead)
    pairs = set()
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        d_src = (dev.put(col["data"]), dev.put(col["offsets"].astype(np.uint32)), 0)
        for n in SEAM_ROWS:
            m = rng.integers(0, src_rows, n).astype(np.uint32)
            got = g.run(m, src_rows, [dict(col, d_src=d_src)], tag=("seams", lead, n))
            off = got[0][1]
            has = off[1:] > off[:-1]
            pairs |= set(zip((col["offsets"][m[has]] % 4).tolist(), (off[:-1][has] % 4).tolist()))
    # device allocations are 16-byte aligned: the offsets' residues are the addresses'
    assert len(pairs) == 16, sorted(pairs)


# ---------------------------------------------------------------------------------------------------------------------
# map shapes; NULL rows; the row base; out-of-range entries
# ---------------------------------------------------------------------------------------------------------------------
def test_map_shapes(ctx):
    rng = np.random.default_rng(21)
    n = BIG
    col = strings(rng, cycled_lengths(3 * n), lead=1)
    num = fixed(column(rng, 3 * n, 8), 8, fill_of(8, 1), valid=rng.random(3 * n) < 0.7, dst_valid=True)
    maps = {"identity": np.arange(n), "reverse": np.arange(n)[::-1], "ascending with gaps": np.cumsum(rng.integers(1, 4, n)) - 1,
            "one source row": np.full(n, 8)}                 # a 257-byte element: the output is larger than the source
    assert cycled_lengths(3 * n)[8] == 257
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        for name, m in maps.items():
            got = g.run(np.ascontiguousarray(m, dtype=np.uint32), 3 * n, [col, num], tag=name)
            if name == "one source row":
                assert len(got[0][0]) == n * 257


@pytest.mark.parametrize("n", [BIG, STEP_ROWS + 1])
def test_null_rows(ctx, n):
    rng = np.random.default_rng(n)
    src_rows = 400
    col = strings(rng, cycled_lengths(src_rows, 5), lead=2, dst_valid=True)
    num = fixed(column(rng, src_rows, 4), 4, fill_of(4, 2), dst_valid=True)
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        for name, null in _null_patterns(BIG):
            null = null[:n].copy()
            m = rng.integers(0, src_rows, n).astype(np.uint32)
            m[null] = NO_ROW
            g.run(m, src_rows, [col, num], tag=("nulls", name, n))


def test_row_base(ctx):
    """HJ_NO_ROW stays NULL whatever the base, also under a base that would make it a row"""
    rng = np.random.default_rng(22)
    n, src_rows = 2 * BLOCK_ROWS + 5, 900
    col = strings(rng, cycled_lengths(src_rows), valid=rng.random(src_rows) < 0.8, dst_valid=True)
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        for base in (5000, NO_ROW - 10):
            m = (rng.integers(0, min(src_rows, NO_ROW - base), n) + base).astype(np.uint32)
            m[::5] = NO_ROW
            g.run(m, src_rows, [col], row_base=base, tag=("row base", base))


def test_out_of_range_entries_are_never_read(ctx):
    """Values, offsets and validity are windows in the middle of larger allocations, as in test_gpu_gather.py: a kernel
    that did read an out-of-range entry's offsets or validity word would stay inside this test's own buffers -- and would
    give lengths the model does not have, because the words around the windows are not zero."""
    rng = np.random.default_rng(23)
    lead_rows, src_rows, n = 4096, 100, 2 * BLOCK_ROWS + 33
    whole = strings(rng, cycled_lengths(2 * lead_rows))
    off = whole["offsets"]
    win = dict(whole, offsets=off[lead_rows:lead_rows + src_rows + 1], valid=rng.random(src_rows) < 0.7, dst_valid=True)
    whole_valid = np.ones(2 * lead_rows, dtype=bool)
    whole_valid[lead_rows:lead_rows + src_rows] = win["valid"]
    num_whole = column(rng, 2 * lead_rows, 8)
    num = fixed(num_whole[lead_rows:lead_rows + src_rows], 8, fill_of(8, 3), valid=win["valid"], dst_valid=True)
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        d_data, d_off, d_ok, d_num = dev.put(whole["data"]), dev.put(off.astype(np.uint32)), dev.put(plane_words(whole_valid)), dev.put(num_whole)
        assert lead_rows % 32 == 0
        win["d_src"] = (d_data, d_off + 4 * lead_rows, d_ok + lead_rows // 8)
        num["d_src"] = (d_num + 8 * lead_rows, 0, d_ok + lead_rows // 8)
        for base, ranges in ((0, [(100, 2000)]), (3000, [(3100, 5000), (1000, 3000)])):
            m = (rng.integers(0, src_rows, n) + base).astype(np.uint32)
            stray = rng.random(n) < 0.4
            lo, hi = zip(*ranges)
            pick = rng.integers(0, len(ranges), n)
            m[stray] = rng.integers(np.array(lo)[pick], np.array(hi)[pick])[stray]
            m[::11] = NO_ROW
            assert int((stray & (m != NO_ROW)).sum()) > 100
            g.run(m, src_rows, [win, num], row_base=base, tag=("out of range", base))
            assert ctx.gather2_info()[3] == int((stray & (m != NO_ROW)).sum())


# ---------------------------------------------------------------------------------------------------------------------
# empty elements
# ---------------------------------------------------------------------------------------------------------------------
def test_empty_elements(ctx):
    rng = np.random.default_rng(24)
    n = BIG
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        for start, run in ((STEP_ROWS + 5, STEP_ROWS), (WAVE_ROWS - 9, WAVE_ROWS), (BLOCK_ROWS - 100, BLOCK_ROWS + 300), (0, n)):
            lens = np.array(cycled_lengths(n))
            lens[lens == 0] = 1
            lens[start:start + run] = 0                          # a run of empty elements across a step, a wavefront, a workgroup; all
            col = strings(rng, lens, lead=3, dst_valid=True)
            g.run(np.arange(n, dtype=np.uint32), n, [col], tag=("empty run", start, run))
            g.run(rng.integers(0, n, n).astype(np.uint32), n, [col], tag=("empty run, random map", start, run))
        # all rows NULL: no source row is named, the values and validity pointers are 0 (the offsets of no row: one word)
        m = np.full(n, NO_ROW, dtype=np.uint32)
        none = dict(width=0, offsets=np.zeros(1, dtype=np.int64), data=np.zeros(0, dtype=np.uint8), valid=None, dst_valid=True)
        none["d_src"] = (0, dev.put(np.zeros(1, dtype=np.uint32)), 0)
        num = fixed(None, 8, fill_of(8, 4), dst_valid=True, d_src=(0, 0, 0))
        g.run(m, 0, [none, num], tag="all rows NULL, no source")
        g.run(m, 0, [dict(none, null_dst=True, capacity=0)], tag="all rows NULL, dst NULL")


# ---------------------------------------------------------------------------------------------------------------------
# long elements among short ones
# ---------------------------------------------------------------------------------------------------------------------
def test_long_elements(ctx):
    rng = np.random.default_rng(25)
    src_rows = 300
    lens = np.array(cycled_lengths(src_rows))
    long_row, block_row = 77, 201
    lens[long_row] = COPY_PASS_BYTES + 904                       # longer than a pass of the workgroup
    lens[block_row] = COPY_BLOCK_BYTES + 1                       # just above one lane's block
    col = strings(rng, lens, lead=1)
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        for n in (BLOCK_ROWS + 200, 300):
            m = rng.integers(0, src_rows, n).astype(np.uint32)
            m[(m == long_row) | (m == block_row)] = 0
            m[[5, n // 2, n // 2 + 1]] = long_row                # named three times, twice by neighbours
            m[[6, 70, n - 40]] = block_row
            for last in (long_row, block_row):
                m[n - 1] = last                                  # ... and once as the last row
                g.run(m, src_rows, [col], tag=("long", n, last))
                g.run(m, src_rows, [dict(col, dst_lead=7)], tag=("long, dst + 7", n, last))


# ---------------------------------------------------------------------------------------------------------------------
# cuts: dstCapacity below the total
# ---------------------------------------------------------------------------------------------------------------------
def test_cuts(ctx):
    rng = np.random.default_rng(26)
    src_rows, n = 500, 2 * BLOCK_ROWS + 100
    col = strings(rng, cycled_lengths(src_rows), lead=2)
    m = rng.integers(0, src_rows, n).astype(np.uint32)
    i, _, _, ok = rows_of(m, 0, src_rows)
    _, raw, off = want_of(col, i, ok, n)
    total = len(raw)
    mid = int(np.flatnonzero((off[1:] - off[:-1]) > 40)[3])         # a row of 64 or 257 bytes
    cuts = {"sizing": 0, "one byte": 1, "middle of an element": int(off[mid]) + 20, "middle of a 16-byte store": 16 * 50 + 7,
            "a workgroup's first byte": int(off[BLOCK_ROWS]), "total - 1": total - 1, "total": total, "more than the total": total + 100}
    assert 0 < cuts["middle of an element"] < total and 0 < cuts["a workgroup's first byte"] < total
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        for name, cap in cuts.items():
            for lead in (0, 5):
                g.run(m, src_rows, [dict(col, capacity=cap, dst_lead=lead)], tag=("cut", name, cap, lead))
        g.run(m, src_rows, [dict(col, capacity=0, null_dst=True)], tag="sizing pass with dst NULL")


# ---------------------------------------------------------------------------------------------------------------------
# totals are exact in 64 bits
# ---------------------------------------------------------------------------------------------------------------------
def test_totals_beyond_32_bits(ctx):
    """1100 rows naming one element of 4 MiB + 1 bytes: the first workgroup's 1024 rows alone take 2^32 + 1024 bytes"""
    size, n = (4 << 20) + 1, 1100
    assert BLOCK_ROWS * size > 1 << 32
    m = np.zeros(n, dtype=np.uint32)
    with Device(ctx) as dev:
        d_data = dev.alloc(size + 3)
        d_off = dev.put(np.array([0, size], dtype=np.uint32))
        d_map = dev.put(m)
        d_doff = dev.put(np.full(2 * GUARD_WORDS + n + 1, SENTINEL, dtype=np.uint32))
        d_dst = dev.put(np.full(2 * GUARD + 64, SENT, dtype=np.uint8))
        d_dvalid = dev.put(np.full(1 + (n + 31) // 32 + GUARD_WORDS, SENTINEL, dtype=np.uint32))
        desc = dict(src=d_data, width=0, src_offsets=d_off, dst_offsets=d_doff + 4 * GUARD_WORDS, dst_valid=d_dvalid)
        for cap in (0, 64):                                      # the sizing call; a copy call, of which nothing may be written
            ctx.gather2(d_map, n, 1, [dict(desc, dst=d_dst + GUARD if cap else 0, dst_capacity=cap)])
            info = ctx.gather2_info()
            assert info[:2] == (n, 0) and info[3] == 0 and info[4] == n * size and info[4] > 0xFFFFFFFF, info
            assert (dev.get(d_dst, 2 * GUARD + 64, np.uint8) == SENT).all()
            offs = dev.get(d_doff, 2 * GUARD_WORDS + n + 1)      # unspecified inside, untouched outside
            assert (offs[:GUARD_WORDS] == SENTINEL).all() and (offs[GUARD_WORDS + n + 1:] == SENTINEL).all()
            plane = dev.get(d_dvalid, 1 + (n + 31) // 32 + GUARD_WORDS)
            assert np.array_equal(plane[:(n + 31) // 32], plane_words(np.ones(n, dtype=bool))) and (plane[(n + 31) // 32:] == SENTINEL).all()
        # below the limit the same call is exact again: 1023 rows are 2^32 - 4 MiB + 1023 bytes
        ctx.gather2(d_map, 1023, 1, [dict(desc, dst_capacity=0)])
        assert ctx.gather2_info()[4] == 1023 * size
        assert dev.get(d_doff, GUARD_WORDS + 1024)[-1] == 1023 * size


# ---------------------------------------------------------------------------------------------------------------------
# source validity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", (0,) + WIDTHS)
def test_source_validity(ctx, width):
    rng = np.random.default_rng(300 + width)
    src_rows = 777

    def make(valid, **kw):
        if width:
            return fixed(column(rng, src_rows, width), width, fill_of(width, 5), valid=valid, **kw)
        return strings(rng, cycled_lengths(src_rows), lead=1, valid=valid, **kw)

    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        for share in (0.3, 1.0):                                 # 30 % NULLs; every source row NULL
            valid = rng.random(src_rows) >= share
            for n in (33, STEP_ROWS + 1, BLOCK_ROWS + 1, BIG):
                m = rng.integers(0, src_rows, n).astype(np.uint32)
                m[rng.integers(0, n, n // 4)] = NO_ROW
                i, _, _, ok = rows_of(m, 0, src_rows)
                got = g.run(m, src_rows, [make(valid, dst_valid=True)], tag=("validity", width, share, n))
                el = got[0][2]
                assert not (el & ~ok).any() and np.array_equal(el[ok], valid[i[ok]])      # dstValid against dValid
                if width:
                    under = np.frombuffer(got[0][0], dtype=f"V{width}")[~el]
                    assert under.tobytes() == fill_of(width, 5)[:width] * int((~el).sum())
                # the plane one word into its allocation; no plane at all; no call-level plane
                g.run(m, src_rows, [make(valid, dst_valid=True, dst_valid_offset=1)], valid_offset=1, tag=("validity + 4", width, n))
                g.run(m, src_rows, [make(valid, dst_valid=False)], tag=("srcValid without dstValid", width, n))
                g.run(m, src_rows, [make(None, dst_valid=True)], with_valid=False, tag=("dstValid without srcValid", width, n))


# ---------------------------------------------------------------------------------------------------------------------
# mixed columns
# ---------------------------------------------------------------------------------------------------------------------
def test_eight_mixed_columns_in_one_call_equal_eight_calls(ctx):
    rng = np.random.default_rng(27)
    src_rows, n = 2000, BIG
    some = lambda: rng.random(src_rows) < 0.7       # noqa: E731
    cols = [fixed(column(rng, src_rows, 4), 4, fill_of(4, 10)),                                           # plain: k_gather's
            strings(rng, cycled_lengths(src_rows), lead=1, valid=some(), dst_valid=True),
            fixed(column(rng, src_rows, 16), 16, fill_of(16, 11), valid=some(), dst_valid=True),
            fixed(column(rng, src_rows, 1), 1, fill_of(1, 12), valid=some()),
            strings(rng, cycled_lengths(src_rows, 9), lead=2),
            fixed(column(rng, src_rows, 8), 8, fill_of(8, 13)),                                           # plain
            fixed(column(rng, src_rows, 2), 2, fill_of(2, 14), dst_valid=True),
            strings(rng, cycled_lengths(src_rows, 4), valid=some(), capacity=1000)]
    m = rng.integers(0, src_rows, n).astype(np.uint32)
    m[rng.integers(0, n, n // 5)] = NO_ROW
    with Device(ctx) as dev:
        g = Gather2(ctx, dev)
        together = g.run(m, src_rows, cols, tag="eight mixed columns")
        for k, col in enumerate(cols):
            alone = g.run(m, src_rows, [col], tag=("one column", k))
            assert alone[0][0] == together[k][0] and np.array_equal(alone[0][2], together[k][2]), k
        for cut in (2, 3, 5):                                    # no plain column at all among the first (the plane's owner changes)
            g.run(m, src_rows, cols[1:1 + cut], tag=("mixed", cut))
        g.run(m, src_rows, [], tag="the plane alone")


def test_plain_columns_equal_hj_gather_dev(ctx):
    rng = np.random.default_rng(28)
    src_rows, n = 1500, BIG
    widths = (1, 2, 4, 8, 16, 16, 8, 4)
    srcs = [column(rng, src_rows, w) for w in widths]
    m = rng.integers(0, src_rows + 50, n).astype(np.uint32)     # some out of range
    m[rng.integers(0, n, n // 5)] = NO_ROW
    words = (n + 31) // 32
    with Device(ctx) as dev:
        d_map = dev.put(m)
        d_srcs = [dev.put(s) for s in srcs]
        outs = []
        for call in ("gather", "gather2"):
            d_dsts = [dev.put(np.full(n * w + GUARD, SENT, dtype=np.uint8)) for w in widths]
            d_valid = dev.put(np.full(words + GUARD_WORDS, SENTINEL, dtype=np.uint32))
            if call == "gather":
                ctx.gather(d_map, n, src_rows, [(s, d, w, fill_of(w, k)) for k, (s, d, w) in enumerate(zip(d_srcs, d_dsts, widths))], d_valid=d_valid)
                info = ctx.gather_info()
            else:
                before = ctx.gather_info()
                ctx.gather2(d_map, n, src_rows, [dict(src=s, dst=d, width=w, fill=fill_of(w, k)) for k, (s, d, w) in enumerate(zip(d_srcs, d_dsts, widths))],
                            d_valid=d_valid)
                info = ctx.gather2_info()
                assert info[4:] == (0,) * 8 and ctx.gather_info() == before       # two records
            outs.append(([dev.get(d, n * w + GUARD, np.uint8).tobytes() for d, w in zip(d_dsts, widths)],
                         dev.get(d_valid, words + GUARD_WORDS).tobytes(), (info[0], info[1], info[3])))
        assert outs[0] == outs[1]
        for k, (w, s) in enumerate(zip(widths, srcs)):
            want = plain_expected(m, 0, src_rows, s, w, fill_of(w, k))[0]
            assert outs[1][0][k] == want.tobytes() + bytes([SENT]) * GUARD


# ---------------------------------------------------------------------------------------------------------------------
# refused calls
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(ctx):
    rng = np.random.default_rng(29)
    n, src_rows = 100, 50
    m = rng.integers(0, src_rows, n).astype(np.uint32)
    words = (n + 31) // 32
    col = strings(rng, cycled_lengths(src_rows))
    num = column(rng, src_rows, 16)
    with Device(ctx) as dev:
        d_map, d_data, d_off, d_num = dev.put(m), dev.put(col["data"]), dev.put(col["offsets"].astype(np.uint32)), dev.put(num)
        d_ok = dev.put(plane_words(np.ones(src_rows, dtype=bool)))
        room = 16 * n + 4096
        d_dst, d_dst2 = dev.put(np.full(room, SENT, dtype=np.uint8)), dev.put(np.full(room, SENT, dtype=np.uint8))
        d_doff = dev.put(np.full(n + 1 + GUARD_WORDS, SENTINEL, dtype=np.uint32))
        d_dvalid = dev.put(np.full(words + GUARD_WORDS, SENTINEL, dtype=np.uint32))
        d_valid = dev.put(np.full(words + GUARD_WORDS, SENTINEL, dtype=np.uint32))
        ctx.gather(d_map, n, src_rows, [(d_num, d_dst, 4, 0)])                      # two calls to remember
        ctx.gather2(d_map, n, src_rows, [dict(src=d_data, width=0, src_offsets=d_off, dst_offsets=d_doff)])
        before, before2 = ctx.gather_info(), ctx.gather2_info()
        assert before[0] == n and before2[0] == n and before2[4] > 0
        ctx.copy_h2d(d_dst, np.full(room, SENT, dtype=np.uint8))
        ctx.copy_h2d(d_doff, np.full(n + 1 + GUARD_WORDS, SENTINEL, dtype=np.uint32))

        F = ("src", "dst", "srcOffsets", "dstOffsets", "srcValid", "dstValid", "dstCapacity", "width", "flags")

        def raw(cols, d_map_=d_map, n_rows=n, rows=src_rows, n_cols=None, valid=d_valid, null_cols=False):
            arr = (_lib.hj_gather_col2 * max(len(cols), 1))()
            for c, d in zip(arr, cols):
                for f in F:
                    v = d.get(f, 0)
                    setattr(c, f, v if f in ("dstCapacity", "width", "flags") else (v or None))
            return hj.lib.hj_gather2_dev(ctx._h, d_map_ or None, n_rows, 0, rows, None if null_cols else arr,
                                         len(cols) if n_cols is None else n_cols, valid or None)

        var = dict(src=d_data, dst=d_dst, srcOffsets=d_off, dstOffsets=d_doff, srcValid=d_ok, dstValid=d_dvalid, dstCapacity=4096, width=0)
        fix = dict(src=d_num, dst=d_dst2, srcValid=d_ok, dstValid=0, width=8)
        assert raw([var, fix]) == _lib.HJ_OK                                       # the two are fine as they stand
        before2 = ctx.gather2_info()
        for d, size in ((d_dst, room), (d_dst2, room)):
            ctx.copy_h2d(d, np.full(size, SENT, dtype=np.uint8))
        ctx.copy_h2d(d_doff, np.full(n + 1 + GUARD_WORDS, SENTINEL, dtype=np.uint32))
        ctx.copy_h2d(d_dvalid, np.full(words + GUARD_WORDS, SENTINEL, dtype=np.uint32))
        ctx.copy_h2d(d_valid, np.full(words + GUARD_WORDS, SENTINEL, dtype=np.uint32))
        refused = {
            # everything hj_gather_dev refuses
            "nine columns": dict(cols=[fix] * 9),
            "width 3": dict(cols=[dict(fix, width=3)]),
            "width 32": dict(cols=[dict(fix, width=32)]),
            "a bad width behind a good one": dict(cols=[fix, dict(fix, width=5)]),
            "src NULL": dict(cols=[dict(fix, src=0)]),
            "dst NULL": dict(cols=[dict(fix, dst=0)]),
            "dst NULL without rows to read": dict(cols=[dict(fix, src=0, dst=0)], rows=0),
            "map NULL": dict(cols=[fix], d_map_=0),
            "cols NULL": dict(cols=[], n_cols=1, null_cols=True),
            "nRows 2^32": dict(cols=[fix], n_rows=1 << 32),
            "srcRows 2^32": dict(cols=[fix], rows=1 << 32),
            "nothing to write": dict(cols=[], valid=0),
            "a variable-length src NULL": dict(cols=[dict(var, src=0)]),
            # what the descriptor adds
            "width 0 without srcOffsets": dict(cols=[dict(var, srcOffsets=0)]),
            "width 0 without dstOffsets": dict(cols=[dict(var, dstOffsets=0)]),
            "width 0 without either": dict(cols=[dict(fix, width=0)]),
            "srcOffsets on a fixed column": dict(cols=[dict(fix, srcOffsets=d_off)]),
            "dstOffsets on a fixed column": dict(cols=[dict(fix, dstOffsets=d_doff)]),
            "a flag": dict(cols=[dict(var, flags=1)]),
            "a high flag on a fixed column": dict(cols=[dict(fix, flags=0x80000000)]),
            "srcOffsets + 2": dict(cols=[dict(var, srcOffsets=d_off + 2)]),
            "dstOffsets + 1": dict(cols=[dict(var, dstOffsets=d_doff + 1)]),
            "srcValid + 2": dict(cols=[dict(fix, srcValid=d_ok + 2)]),
            "dstValid + 3": dict(cols=[dict(var, dstValid=d_dvalid + 3)]),
            "capacity with dst NULL": dict(cols=[dict(var, dst=0)]),
            "capacity on a fixed column": dict(cols=[dict(fix, dstCapacity=8)]),
            "a variable-length dst inside a fixed column's": dict(cols=[dict(var, dst=d_dst2 + 8), fix]),
            "two variable-length dsts that overlap": dict(cols=[var, dict(var, dst=d_dst + 4095, dstOffsets=d_dst2, dstValid=0)]),
            "a variable-length dst over its own offsets": dict(cols=[dict(var, dst=d_doff - 4000)]),
            "a variable-length dst over the call's plane": dict(cols=[dict(var, dst=d_valid + 1)]),
        }
        for w in (2, 4, 8, 16):
            refused[f"src + 1, width {w}"] = dict(cols=[dict(fix, src=d_num + 1, width=w)])
            refused[f"dst + {w // 2}, width {w}"] = dict(cols=[dict(fix, dst=d_dst2 + w // 2, width=w)])
        for name, args in refused.items():
            assert raw(**args) == _lib.HJ_ERR_INVALID, name
            assert ctx.gather2_info() == before2 and ctx.gather_info() == before, name
        # nRows 0 is a no-op, whatever else is given
        assert raw([var, fix], n_rows=0) == _lib.HJ_OK and raw([], d_map_=0, n_rows=0, rows=0, valid=0) == _lib.HJ_OK
        assert ctx.gather2_info() == before2 and ctx.gather_info() == before
        for d, size in ((d_dst, room), (d_dst2, room)):
            assert (dev.get(d, size, np.uint8) == SENT).all()
        for d, size in ((d_doff, n + 1 + GUARD_WORDS), (d_dvalid, words + GUARD_WORDS), (d_valid, words + GUARD_WORDS)):
            assert (dev.get(d, size) == SENTINEL).all()
        # and the context still gathers
        Gather2(ctx, dev).run(m, src_rows, [col, fixed(num, 16, fill_of(16, 6), dst_valid=True)], tag="after the refused calls")


def test_info_is_zero_before_the_first_call():
    with hj.HashJoinContext(0) as fresh:
        assert fresh.gather2_info() == (0,) * 12
        with Device(fresh) as dev:
            rng = np.random.default_rng(30)
            Gather2(fresh, dev).run(np.arange(5, dtype=np.uint32), 5, [strings(rng, [3, 0, 9, 1, 40])], tag="no reserve, no table")
        assert fresh.gather2_info()[0] == 5 and fresh.gather_info() == (0, 0, 0, 0)
