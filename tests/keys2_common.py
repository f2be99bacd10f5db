"""What the tests of the Arrow-layout key columns share: a column as a plain Python list of `bytes | None` per row (the
model's view), its KeyColumn, the header's hash restated on such rows, and the join as a dict join over tuples of
`bytes | None` with the NULL rules of join_on_columns. Nothing here calls the library's hash, verify or join."""
from collections import namedtuple

import numpy as np

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from keys_common import MIXES

M32 = 0xFFFFFFFF
NULL_SEED = 0x4E554C4C
LENGTHS = list(range(10)) + [31, 32, 33, 64, 257]
ROWS = [1, 31, 32, 33, 63, 64, 65, 1025]
MASKS = [0, 0x3F, 0xFFFF0000]
HOWS = ("inner", "left", "semi", "anti", "right", "full", "right_semi", "right_anti")

# width: 1, 2, 4, 8, 16, or 0 for variable length; items: one bytes (of `width` bytes, or of any length) or None per row
ModelCol = namedtuple("ModelCol", "width items nulls_equal")


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def mm3_mix(h, k):
    k = (k * 0xcc9e2d51) & M32
    k = (_rotl(k, 15) * 0x1b873593) & M32
    return (_rotl(h ^ k, 13) * 5 + 0xe6546b64) & M32


def mm3_final(h, length):
    h ^= length
    h = ((h ^ (h >> 16)) * 0x85ebca6b) & M32
    h = ((h ^ (h >> 13)) * 0xc2b2ae35) & M32
    return h ^ (h >> 16)


def le_words(b):
    """the bytes as little-endian 32-bit words, the last one zero-padded"""
    b = b + b"\0" * (-len(b) % 4)
    return [int.from_bytes(b[i:i + 4], "little") for i in range(0, len(b), 4)]


def row_word(cols, i, key_mask=0):
    """the join word of row i as the header words it"""
    words = []
    for c in cols:
        e = c.items[i]
        if e is None:
            if not c.nulls_equal:                        # NULL-keyed: the row's position, not its columns
                return mm3_final(mm3_mix(NULL_SEED, i & M32), 4) & (key_mask or M32)
            words.append(M32)
        elif c.width:
            assert len(e) == c.width
            words += le_words(e)                         # width 1 and 2: zero-extended to one word
        else:
            words += [len(e)] + le_words(e)
    h = 0
    for k in words:
        h = mm3_mix(h, k)
    return mm3_final(h, 4 * len(words)) & (key_mask or M32)


def model_words(cols, key_mask=0):
    return np.array([row_word(cols, i, key_mask) for i in range(len(cols[0].items))], dtype=np.uint64)


def key_column(c, lead=0, filler=0xA5):
    """the KeyColumn of a model column. Variable length: `lead` bytes in front of the first element, so offsets[0] = lead
    and every element starts `lead` bytes later; a NULL keeps an empty range. Fixed: a NULL's element is `filler` bytes."""
    valid = np.array([e is not None for e in c.items], dtype=bool)
    valid = None if valid.all() else valid
    if c.width:
        raw = b"".join(bytes([filler]) * c.width if e is None else e for e in c.items)
        values = np.frombuffer(raw, dtype=np.uint8).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64, 16: "V16"}[c.width])
        return hj.KeyColumn(values.copy(), valid, nulls_equal=c.nulls_equal)
    lens = [0 if e is None else len(e) for e in c.items]
    off = lead + np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
    data = bytes([0xEE]) * lead + b"".join(e or b"" for e in c.items) + b"\xEE" * 3
    return hj.KeyColumn.varlen(off, data, valid, nulls_equal=c.nulls_equal)


def fixed_col(rng, width, n, nulls=0.0, nulls_equal=False, distinct=None):
    """n random elements of `width` bytes (out of `distinct` values, if given), a share `nulls` of them None"""
    pool = rng.integers(0, 256, size=((distinct or n), width), dtype=np.uint8)
    pick = rng.integers(0, pool.shape[0], n) if distinct else np.arange(n)
    gone = rng.random(n) < nulls
    return ModelCol(width, [None if g else pool[p].tobytes() for p, g in zip(pick, gone)], nulls_equal)


def varlen_col(rng, lengths, nulls=0.0, nulls_equal=False):
    """one random element per entry of `lengths`, a share `nulls` of them None"""
    gone = rng.random(len(lengths)) < nulls
    return ModelCol(0, [None if g else rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n, g in zip(lengths, gone)],
                    nulls_equal)


def hash_matrix(rng, n):
    """the column lists of n rows the hash is checked on, host and device: the fixed mixes plain, nullable and with
    NULLs that are equal; every length of LENGTHS (cycled over the rows, so they start at changing alignments), alone,
    nullable and next to fixed columns"""
    lens = [LENGTHS[(i * 7 + 3) % len(LENGTHS)] for i in range(n)]
    out = [[fixed_col(rng, w, n) for w in widths] for widths in MIXES]
    out += [[fixed_col(rng, w, n, nulls=0.3) for w in widths] for widths in MIXES[::3]]
    out += [[fixed_col(rng, w, n, nulls=0.3, nulls_equal=(k % 2 == 0)) for k, w in enumerate(widths)] for widths in MIXES[1::3]]
    out += [[varlen_col(rng, lens)], [varlen_col(rng, lens, nulls=0.3)], [varlen_col(rng, lens, nulls=0.3, nulls_equal=True)],
            [fixed_col(rng, 4, n, nulls=0.2), varlen_col(rng, lens, nulls=0.2, nulls_equal=True)],
            [varlen_col(rng, lens), fixed_col(rng, 16, n), varlen_col(rng, lens[::-1], nulls=0.1), fixed_col(rng, 1, n, nulls=0.5, nulls_equal=True)]]
    return out


# ---- the join ------------------------------------------------------------------------------------------------------------
def row_keys(cols, nulls_equal=False):
    """one tuple of bytes | None per row, or None for a NULL-keyed row (a NULL in a column where NULLs are not equal)"""
    keys = []
    for i in range(len(cols[0].items)):
        k = tuple(c.items[i] for c in cols)
        null_keyed = any(e is None and not (nulls_equal or c.nulls_equal) for e, c in zip(k, cols))
        keys.append(None if null_keyed else k)
    return keys


def inner_pairs(r_keys, s_keys):
    """[(s row, r row)] of the dict join; a NULL-keyed row matches nothing. A None inside a tuple equals a None."""
    table = {}
    for j, k in enumerate(r_keys):
        if k is not None:
            table.setdefault(k, []).append(j)
    return [(i, j) for i, k in enumerate(s_keys) if k is not None for j in table.get(k, ())]


def expected_rows(how, pairs, n_r, n_s):
    """(S rows, R rows) of the result, -1 where the side has no tuple; None for a side the kind has no plane for"""
    s_hit, r_hit = {i for i, _ in pairs}, {j for _, j in pairs}
    lone_s = [i for i in range(n_s) if i not in s_hit]
    lone_r = [j for j in range(n_r) if j not in r_hit]
    s, r = [i for i, _ in pairs], [j for _, j in pairs]
    rows = {"inner": (s, r), "left": (s + lone_s, r + [-1] * len(lone_s)), "semi": (sorted(s_hit), None), "anti": (lone_s, None),
            "right": (s + [-1] * len(lone_r), r + lone_r),
            "full": (s + lone_s + [-1] * len(lone_r), r + [-1] * len(lone_s) + lone_r),
            "right_semi": (None, sorted(r_hit)), "right_anti": (None, lone_r)}[how]
    return tuple(None if x is None else np.array(x, dtype=np.int64) for x in rows)


# ---- argument errors of the entry points that take hj_key_col2 ----------------------------------------------------------------
def _bad_columns(n):
    """(name, keyword changes) of every column the three entry points refuse, on top of a good one"""
    keys = np.arange(2 * n, dtype=np.uint64)
    off = np.arange(n + 2, dtype=np.uint32)
    valid = np.full(n // 32 + 2, M32, dtype=np.uint32)
    good_fixed = dict(ptr=keys.ctypes.data, width=8, off=0, valid=valid.ctypes.data, flags=1)
    good_var = dict(ptr=keys.ctypes.data + 1, width=0, off=off.ctypes.data, valid=0, flags=0)
    bad = [dict(good_fixed, width=w) for w in (3, 5, 12, 32)]
    bad += [dict(good_fixed, width=w, ptr=keys.ctypes.data + w // 2) for w in (2, 4, 8, 16)]       # misaligned for its width
    bad += [dict(good_fixed, ptr=0), dict(good_var, ptr=0),
            dict(good_var, off=0),                                                                  # width 0 without offsets
            dict(good_fixed, off=off.ctypes.data),                                                  # offsets with a width
            dict(good_fixed, flags=2), dict(good_var, flags=0x80000001),                            # unknown flag bits
            dict(good_var, off=off.ctypes.data + 2), dict(good_fixed, valid=valid.ctypes.data + 1),  # not 4-byte aligned
            dict(good_var, valid=valid.ctypes.data + 2)]
    return (keys, off, valid), good_fixed, good_var, bad


def _col2(n_cols, side_s, side_r, ptr, width, off, valid, flags):
    cols = (_lib.hj_key_col2 * 5)()
    for c in cols:
        c.width, c.flags = width, flags
        if side_s:
            c.s, c.sOffsets, c.sValid = ptr or None, off or None, valid or None
        if side_r:
            c.r, c.rOffsets, c.rValid = ptr or None, off or None, valid or None
    return cols
