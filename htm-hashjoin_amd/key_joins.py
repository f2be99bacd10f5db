"""Joins on real key columns: hash, candidate join, verify (join_on, join_on_columns)."""
import numpy as np

from . import _lib
from .columns import KeyColumn, _DevColumn, _as_key_columns, _join_key_args, _key_columns, _table_columns
from .conditions import _PairStep, _RowChain, _asof_term, _condition_steps, _where_terms
from .joins import _TableRows, _drive_join, _slice_step, _table_how, _where_keyword


class _ColumnKeys(_PairStep):
    """What join_on, join_on_columns and aggregate_on share: the key columns of both sides on the device (R's whole, a slice of
    S's in the room kept for one), the hash of either side as _drive_join's `fill`, and the verify step of a _PairChain
    over a slice's candidates; its put() has nothing to do, the slice's columns went up with its hash. cols: the hj_key_col2
    tuples."""

    def __init__(self, r_keys, s_keys, nulls_equal, key_mask, step):
        self.r_keys, self.s_keys, self.key_mask, self.step = r_keys, s_keys, key_mask, step
        self.flags = [_lib.HJ_KEY_NULLS_EQUAL if nulls_equal or r.nulls_equal or s.nulls_equal else 0 for r, s in zip(r_keys, s_keys)]

    def hash_keys(self, ctx, held, d_tuples, lo, n):
        """R's key columns go up whole, a slice's into the room kept for one; either is hashed where it lies"""
        if lo is None:
            r_dev = [_DevColumn.whole(ctx, held, c) for c in self.r_keys]
            self.s_dev = [_DevColumn(held, c, self.step) for c in self.s_keys]
            self.cols = [(s.parts[0], r.parts[0], r.col.width, s.parts[1], r.parts[1], s.parts[2], r.parts[2], f)
                         for s, r, f in zip(self.s_dev, r_dev, self.flags)]
            ctx.key_hash2(self.cols, _lib.HJ_KEY_SIDE_R, n, d_tuples, self.key_mask)
        else:
            for dev in self.s_dev:
                dev.put(ctx, lo, n)
            ctx.key_hash2(self.cols, _lib.HJ_KEY_SIDE_S, n, d_tuples, self.key_mask)

    def filter(self, ctx, lo, n, n_r, d_s, d_r, n_pairs, d_ks, d_kr, capacity, d_s_marks, d_r_marks):
        ctx.pairs_verify2(d_s, d_r, n_pairs, lo, n, n_r, self.cols, d_ks, d_kr, capacity, d_s_marks, d_r_marks)

    def info(self, ctx):
        return ctx.verify_info()


def _join_key_columns(fn, r_keys, s_keys, widths_differ, nulls_equal, r_cols, s_cols, how, radixBits, slice_tuples, device, key_mask, where,
                      asof):
    """The driver of join_on (fn "join_on") and join_on_columns: hash, candidate join, verify, the rows of the kind. r_keys /
    s_keys: lists of KeyColumn of one length per side; widths_differ: the caller's text for columns that do not pair up;
    `how` is one of _TABLE_HOWS."""
    n_r, n_s = _join_key_args(fn, r_keys, s_keys, key_mask, widths_differ)
    r_cols = _table_columns(fn, "R", r_cols, n_r)
    s_cols = _table_columns(fn, "S", s_cols, n_s)
    step = _slice_step(fn, n_s, slice_tuples) if n_s else 0
    conditions = _condition_steps(_where_terms(fn, where, n_s, n_r), _asof_term(fn, asof, n_s, n_r), step)
    rows = _TableRows(how, r_cols, s_cols, n_r, step)
    trivial = rows.without_device(n_s)
    if trivial is not None:
        return trivial
    keys = _ColumnKeys(r_keys, s_keys, nulls_equal, key_mask, step)
    chain = _RowChain([keys] + conditions, rows, n_r, step)
    # the candidate join is INNER whatever the kind, and the context's own R marks stay out of it: a candidate that the
    # verify step rejects would have set them. Its tuples are made on the device (_drive_join's fill): the two arrays stand
    # for the relations' lengths alone
    _drive_join(np.empty(n_r, dtype=np.uint8), np.empty(n_s, dtype=np.uint8), "radix", _lib.HJ_JOIN_INNER, None, step, chain.slice,
                device, radixBits=radixBits, fill=keys.hash_keys, after=chain.after)
    return rows.joined()


def _join_on_arrays(r_keys, s_keys, r_cols=None, s_cols=None, how="inner", radixBits=0, slice_tuples=None, device=0, key_mask=0, where=None,
                    asof=None):
    """join_on, and join_on with a condition (_where_keyword): its own checks, then the driver of join_on_columns on the
    arrays as plain KeyColumns"""
    fn = "join_on"
    _table_how(fn, how)
    r_keys, s_keys = _key_columns(fn, "R", r_keys), _key_columns(fn, "S", s_keys)
    return _join_key_columns(fn, [KeyColumn(a) for a in r_keys], [KeyColumn(a) for a in s_keys],
                             "the key columns of R have {}-byte elements, those of S {}", False, r_cols, s_cols, how, radixBits,
                             slice_tuples, device, key_mask, where, asof)


@_where_keyword(_join_on_arrays)
def join_on(r_keys, s_keys, r_cols=None, s_cols=None, how="inner", radixBits=0, slice_tuples=None, device=0, key_mask=0):
    """join_tables for keys that are not one 32-bit word: r_keys / s_keys are each one 1-D numpy array or a sequence of 1
    to HJ_KEY_MAX_COLS of them (all of a side of one length; column c of both sides of the same itemsize out of 1, 2, 4,
    8, 16 bytes -- 64-bit integers, several columns, 16-byte structured elements), and two rows match when every key
    column is BYTEWISE equal. For float keys that means -0.0 != 0.0, and a NaN equals the same NaN bit pattern.
    The method is hash, candidate join, verify, all on the device: the key columns are hashed to a 32-bit join word
    (HashJoinContext.key_hash), the resident radix join gives the candidate pairs on that word, pairs_verify compares
    the real key bytes of every candidate and marks the S and R rows of the pairs it keeps, and the kind follows from the
    kept pairs and the sweeps of those marks (mark_rows). key_mask (0: none) keeps only those bits of the join word: more
    candidates, the same result -- for tests; the result never depends on the hash's quality.
    how, r_cols / s_cols, radixBits, slice_tuples and the result -- {"s_idx", "r_idx", "s", "r", "s_valid", "r_valid"} -- as
    in join_tables(path="radix"). Per slice, left and full give the kept pairs first, then the slice's unmatched S rows
    ascending; semi and anti give their S rows ascending; for right / full the R-only rows come last, R ascending.
    where (keyword only): as in join_tables -- a pair is a match iff the keys are equal and every term holds. The verify step then runs
    without mark planes and with its pairs kept whatever the kind, and HashJoinContext.pairs_where over those pairs sets the
    marks and keeps the pairs of the result.
    asof (keyword only): as in join_tables -- per S row the one pair with equal keys, every where term holding, whose R value is
    nearest on the permitted side. The verify step and the condition step then keep their pairs and mark nothing, and
    HashJoinContext.pairs_asof sets the marks and keeps the pairs of the result."""
    return _join_on_arrays(r_keys, s_keys, r_cols, s_cols, how, radixBits, slice_tuples, device, key_mask)


_COLUMN_WIDTHS_DIFFER = "the key columns of R have widths {} (0: variable-length), those of S {}"


def _join_on_columns(r_keys, s_keys, r_cols=None, s_cols=None, how="inner", nulls_equal=False, radixBits=0, slice_tuples=None,
                     device=0, key_mask=0, where=None, asof=None):
    """join_on_columns, and join_on_columns with a condition or an as-of term (_where_keyword)"""
    fn = "join_on_columns"
    _table_how(fn, how)
    r_keys, s_keys = _as_key_columns(fn, "R", r_keys), _as_key_columns(fn, "S", s_keys)
    return _join_key_columns(fn, r_keys, s_keys, _COLUMN_WIDTHS_DIFFER, nulls_equal, r_cols, s_cols, how, radixBits, slice_tuples, device,
                             key_mask, where, asof)


@_where_keyword(_join_on_columns)
def join_on_columns(r_keys, s_keys, r_cols=None, s_cols=None, how="inner", nulls_equal=False, radixBits=0, slice_tuples=None,
                    device=0, key_mask=0):
    """join_on for key columns that may hold NULLs and variable-length elements (strings): r_keys / s_keys are each one
    KeyColumn or a sequence of 1 to HJ_KEY_MAX_COLS of them, all of a side of one length; a plain 1-D numpy array stands
    for KeyColumn(array), a numpy.ma.MaskedArray brings its mask. Column c of both sides is of one kind: fixed with the
    same itemsize, or variable-length. Two rows match when every column is equal: fixed elements bytewise (as join_on),
    variable-length ones in length and bytes.
    NULLs: a row with a NULL in any key column is NULL-keyed and matches nothing, not even another NULL (SQL's =). A
    NULL-keyed S row is an unmatched S row: it appears in left, full and anti. A NULL-keyed R row is an unmatched R row:
    it appears in right, full and right_anti. nulls_equal=True sets HJ_KEY_NULLS_EQUAL on every column: a NULL equals a
    NULL and nothing else (the pandas reading); a column built with nulls_equal=True has it by itself.
    The method is join_on's with HashJoinContext.key_hash2 / pairs_verify2 in place of key_hash / pairs_verify; per S
    slice the validity bits are repacked from the slice's first row and the offsets rebased to the slice's own bytes.
    how, r_cols / s_cols, radixBits, slice_tuples, key_mask, where and asof (keyword only), the result dict and the order of its rows: as in join_on."""
    return _join_on_columns(r_keys, s_keys, r_cols, s_cols, how, nulls_equal, radixBits, slice_tuples, device, key_mask)
