"""What the gather tests share (test_gpu_gather.py, test_gpu_gather2.py, test_gpu_stream_order.py): the row seams of
hj_gather.hip, random columns, and the models of hj_gather_dev and hj_gather2_dev in numpy and plain Python -- which rows are
NULL, out of range or copied, the bytes, offsets and validity a call must leave. No test in here, and nothing that asks
the library what a result should be."""
import numpy as np

STEP_ROWS = 64
LANE_ROWS = 4
WAVE_ROWS = STEP_ROWS * LANE_ROWS
BLOCK_ROWS = 4 * WAVE_ROWS
assert BLOCK_ROWS == 1024
WIDTHS = (1, 2, 4, 8, 16)
NO_ROW = 0xFFFFFFFF
GUARD_BYTES = 256
GUARD_WORDS = 16
SEAM_ROWS = (1, 31, 32, 33, STEP_ROWS - 1, STEP_ROWS, STEP_ROWS + 1, WAVE_ROWS - 1, WAVE_ROWS, WAVE_ROWS + 1, BLOCK_ROWS - 1,
             BLOCK_ROWS, BLOCK_ROWS + 1, 4 * BLOCK_ROWS + 1, 3 * BLOCK_ROWS + 77)
BIG = 3 * BLOCK_ROWS + 77


# ---- hj_gather_dev: fixed-width columns, a fill pattern under NULL rows ----------------------------------------------------------
def column(rng, rows, width):
    """`rows` random elements of `width` bytes"""
    return rng.integers(0, 256, rows * width, dtype=np.uint8).view(f"V{width}")


def fill_of(width, salt):
    """a non-zero fill pattern of its own per column: 16 bytes, of which the low `width` count"""
    return bytes((17 * salt + 3 * i + 1) % 255 + 1 for i in range(16))


def expected(m, row_base, src_rows, src, width, fill):
    """-> (the column, valid, NULL rows, out-of-range entries) as the header defines them"""
    e = m.astype(np.int64)
    null = e == NO_ROW
    i = (e - row_base) % (1 << 32)
    oor = ~null & (i >= src_rows)
    ok = ~null & ~oor
    out = np.empty(m.size, dtype=f"V{width}")
    out[:] = np.frombuffer(fill[:width], dtype=f"V{width}")[0]
    if src is not None and ok.any():
        out[ok] = src[i[ok]]
    return out, ok, int(null.sum()), int(oor.sum())


def _null_patterns(n):
    every = np.zeros(n, dtype=bool)
    ends = every.copy()
    ends[[0, n - 1]] = True
    yield "first and last", ends
    for start in (STEP_ROWS, STEP_ROWS + 5):                    # a whole step of a wavefront; the same run across two steps
        run = every.copy()
        run[start:start + STEP_ROWS] = True
        yield f"run of {STEP_ROWS} at {start}", run
    for start in (BLOCK_ROWS, BLOCK_ROWS + 3 * STEP_ROWS + 9):  # a whole workgroup; the same run across two workgroups
        run = every.copy()
        run[start:start + BLOCK_ROWS] = True
        yield f"run of {BLOCK_ROWS} at {start}", run
    second = every.copy()
    second[::2] = True
    yield "every second", second
    yield "every row", ~every


# ---- hj_gather2_dev: columns in the Arrow layout, as dicts -----------------------------------------------------------------------
def rows_of(m, row_base, src_rows):
    """-> (source row per output row, NULL rows, out-of-range entries, rows with a source row)"""
    e = m.astype(np.int64)
    null = e == NO_ROW
    i = (e - row_base) % (1 << 32)
    oor = ~null & (i >= src_rows)
    return i, null, oor, ~null & ~oor


def fixed(src, width, fill, valid=None, dst_valid=False, **kw):
    return dict(width=width, src=src, fill=fill, valid=valid, dst_valid=dst_valid, **kw)


def strings(rng, lengths, lead=0, valid=None, dst_valid=False, **kw):
    """a variable-length source: `lead` bytes in front of the first element (offsets[0] = lead), three behind the last"""
    off = lead + np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    data = rng.integers(0, 256, int(off[-1]) + 3, dtype=np.uint8)
    return dict(width=0, offsets=off, data=data, valid=valid, dst_valid=dst_valid, **kw)


def want_of(col, i, ok, n):
    """-> (rows with a valid element, the output bytes, the output offsets or None)"""
    el = ok.copy()
    if col["valid"] is not None:
        el[ok] = col["valid"][i[ok]]
    if col["width"]:
        w = col["width"]
        out = np.empty(n, dtype=f"V{w}")
        out[:] = np.frombuffer(col["fill"][:w], dtype=f"V{w}")[0]
        if el.any():
            out[el] = col["src"][i[el]]
        return el, out.tobytes(), None
    off, data = col["offsets"], col["data"]
    lens = np.zeros(n, dtype=np.int64)
    lens[el] = off[i[el] + 1] - off[i[el]]
    raw = b"".join(data[off[j]:off[j + 1]].tobytes() for j in i[el])
    return el, raw, np.concatenate([[0], np.cumsum(lens)])
