"""What the tests of hj_sort_rows_dev / hj_sort_rows_host share: the model, the case families and the comparison. No test
in here.

The model is numpy and knows nothing of the library's order key. Per column the valid values get DENSE RANKS from
np.unique(return_inverse=True); where the values need it the ranks are fixed by hand -- every NaN in one class above +inf,
-0.0 with 0.0 --, reversed for a descending column, and the NULLs get rank -1 (first) or max + 1 (last). np.lexsort over
the rank columns with the row number as the last key is then the one stable order the header defines."""
import ctypes as C
import functools

import numpy as np

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

from gpu_harness import plane_words

U32, U64 = np.uint32, np.uint64
DTYPES = ("uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64", "float32", "float64")
_TYPE = {"u": _lib.HJ_VAL_UINT, "i": _lib.HJ_VAL_INT, "f": _lib.HJ_VAL_FLOAT}


class Col:
    """one sort column of a case: the values (any bytes under a NULL), one bool per row or None, direction, NULL placement"""

    def __init__(self, values, valid=None, desc=False, nulls="last"):
        self.values = np.ascontiguousarray(values)
        self.valid = None if valid is None else np.ascontiguousarray(valid, dtype=bool)
        self.desc, self.nulls = bool(desc), nulls
        assert self.values.ndim == 1 and nulls in ("last", "first") and (valid is None or self.valid.shape == self.values.shape)

    @property
    def width(self):
        return self.values.dtype.itemsize

    @property
    def type(self):
        return _TYPE[self.values.dtype.kind]

    @property
    def flags(self):
        return (_lib.HJ_SORT_DESC if self.desc else 0) | (_lib.HJ_SORT_NULLS_FIRST if self.nulls == "first" else 0)

    def plane(self, garbage=None):
        """the validity as the C ABI takes it (None: no plane); garbage: an rng that sets the bits of the last word beyond the rows"""
        if self.valid is None:
            return None
        n = self.valid.size
        words = plane_words(self.valid) if n else np.zeros(1, dtype=U32)
        if garbage is not None and n % 32:
            words[-1] |= U32(int(garbage.integers(0, 1 << 32)) & ~((1 << (n % 32)) - 1) & 0xFFFFFFFF)
        return words

    def key(self):
        """as the Python wrappers take the column"""
        return hj.KeyColumn(self.values, self.valid) if self.valid is not None else self.values

    def passes(self):
        return self.width + (self.valid is not None)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _ranks(col):
    """dense ranks of one column in ITS order: NULLs -1 or max + 1, ties equal"""
    v, n = col.values, col.values.size
    ok = np.ones(n, dtype=bool) if col.valid is None else col.valid
    rank = np.zeros(n, dtype=np.int64)
    vals = v[ok]
    if vals.dtype.kind == "f":
        nan = np.isnan(vals)
        plain = np.where(vals[~nan] == 0, np.zeros((), dtype=vals.dtype), vals[~nan])      # -0.0 with 0.0
        uniq, inv = np.unique(plain, return_inverse=True)
        r = np.empty(vals.size, dtype=np.int64)
        r[~nan] = inv
        r[nan] = uniq.size                                                                  # every NaN: one class above +inf
    else:
        r = np.unique(vals, return_inverse=True)[1].astype(np.int64)
    top = int(r.max()) if r.size else 0
    if col.desc:
        r = top - r
    rank[ok] = r
    rank[~ok] = -1 if col.nulls == "first" else top + 1
    return rank


def model_perm(cols):
    """the permutation the header defines, uint32"""
    n = cols[0].values.size
    keys = [np.arange(n, dtype=np.int64)] + [_ranks(c) for c in reversed(cols)]            # lexsort: the LAST key is the primary one
    return np.lexsort(keys).astype(U32)


def same(got, want, tag=None):
    got = np.asarray(got)
    assert got.dtype == U32 and got.shape == want.shape, (tag, got.dtype, got.shape)
    assert np.array_equal(np.sort(got), np.arange(want.size, dtype=U32)), (tag, "not a permutation")
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, f"{bad.size} positions differ, the first at {bad[:1]}: {got[bad[:4]]} for {want[bad[:4]]}")


# ---- the library on host pointers, through ctypes (raw planes, so that garbage bits reach it) ---------------------------------
def sort_col_array(cols, pointers):
    """pointers: [(values_ptr, valid_ptr or 0)] -> (hj_sort_col array, its length)"""
    arr = (_lib.hj_sort_col * max(len(cols), 1))()
    for a, c, (v, w) in zip(arr, cols, pointers):
        a.values, a.valid, a.width, a.type, a.flags, a.reserved = v or None, w or None, c.width, c.type, c.flags, 0
    return arr, len(cols)


def host_perm(cols, garbage=None):
    """hj_sort_rows_host -> (perm, out[8])"""
    n = cols[0].values.size
    planes = [c.plane(garbage) for c in cols]
    arr, k = sort_col_array(cols, [(c.values.ctypes.data, p.ctypes.data if p is not None else 0) for c, p in zip(cols, planes)])
    perm, out = np.full(n, 0xA5A5A5A5, dtype=U32), (C.c_uint64 * 8)()
    rc = lib.hj_sort_rows_host(arr, k, n, perm.ctypes.data if n else None, out)
    assert rc == _lib.HJ_OK, rc
    return perm, [int(x) for x in out]


def layout(n):
    """hj_sort_layout_info -> (tile rows, chunk rows, chunks, workspace bytes)"""
    out = (C.c_uint64 * 4)()
    assert lib.hj_sort_layout_info(n, out) == _lib.HJ_OK
    return tuple(int(x) for x in out)


# ---- case families ---------------------------------------------------------------------------------------------------------------
_F_SPECIAL = {"float32": np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7FC00000,
                                   0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FC12345, 0x3F800000, 0xBF800000], dtype=U32),
              "float64": np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001,
                                   0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
                                   0xFFFFFFFFFFFFFFFF, 0x7FF8000012345678, 0x3FF0000000000000, 0xBFF0000000000000], dtype=U64)}


def typed_values(rng, dtype, n, distinct=None):
    """n values of a dtype over its whole range, the corner values among them (INT: min, max, -1, 0; floats: +-0.0, +-inf,
    denormals, NaNs of both signs with different payloads); distinct: drawn from that many values, so that there are ties"""
    dt = np.dtype(dtype)
    m = n if distinct is None else distinct
    if dt.kind == "f":
        pool = rng.integers(0, 1 << (8 * dt.itemsize - 1), m, dtype=U64).astype(_F_SPECIAL[dt.name].dtype)
        pool |= (rng.integers(0, 2, m).astype(pool.dtype) << pool.dtype.type(8 * dt.itemsize - 1))
        pool[:min(m, 14)] = _F_SPECIAL[dt.name][:min(m, 14)]
        pool = pool.view(dt)
    else:
        info = np.iinfo(dt)
        pool = rng.integers(info.min, info.max, m, dtype=dt, endpoint=True)
        corners = np.array([info.min, info.max, 0, info.max if dt.kind == "u" else -1], dtype=dt)
        pool[:min(m, 4)] = corners[:min(m, 4)]
    return pool[rng.integers(0, m, n)] if distinct is not None else pool[rng.permutation(m)]


def nullable(rng, values, frac):
    """`values` with about frac of its rows NULL and random bytes under them"""
    valid = rng.random(values.size) >= frac if frac < 1 else np.zeros(values.size, dtype=bool)
    v = values.copy()
    raw = v.view(np.uint8).reshape(v.size, -1)
    raw[~valid] = rng.integers(0, 256, (int((~valid).sum()), raw.shape[1]), dtype=np.uint8)
    return v, valid


FAMILIES = ("equal", "perm", "ascending", "descending", "alternating", "low_byte", "high_byte", "ends", "small_i64") + \
    tuple("type_" + d for d in DTYPES) + ("ties_f32", "ties_f64") + \
    tuple(f"null{p}_{w}_{d}" for p in (0, 10, 100) for w in ("last", "first") for d in ("asc", "desc")) + \
    ("multi2", "multi3", "multi4", "lead_const")


def make(name, n, seed=0):
    """the columns of a family at n rows"""
    rng = np.random.default_rng([sum(map(ord, name)), n, seed])
    if name == "equal":
        return [Col(np.full(n, -12345678901, dtype=np.int64))]
    if name == "perm":
        return [Col(rng.permutation(n).astype(np.int32))]
    if name == "ascending":
        return [Col(np.arange(n, dtype=U32) * U32(3))]
    if name == "descending":
        return [Col((np.arange(n, dtype=np.int64)[::-1] - n // 2).astype(np.int16 if n < 30000 else np.int32))]
    if name == "alternating":
        return [Col(np.where(np.arange(n) % 2 == 0, 0xBEEF, 0x0102).astype(np.uint16))]
    if name == "low_byte":
        return [Col(np.int64(0x0123456789ABCD00) + rng.integers(0, 256, n))]
    if name == "high_byte":
        return [Col((rng.integers(0, 256, n).astype(U64) << U64(56)) | U64(0x00C0FFEE12345678))]
    if name == "ends":                                                                      # digits 0x00 and 0xFF alone: first and last bin
        return [Col((rng.integers(0, 2, (n, 4)).astype(np.uint8) * np.uint8(0xFF)).view(U32).reshape(n))]
    if name == "small_i64":                                                                 # six passes whose digit is one value
        return [Col(rng.integers(0, 1000, n).astype(np.int64))]
    if name.startswith("type_"):
        return [Col(typed_values(rng, name[5:], n))]
    if name.startswith("ties_"):                                                            # few values: -0.0 / 0.0 and the NaNs tie
        return [Col(typed_values(rng, "float" + name[6:], n, distinct=14), desc=bool(n & 1))]
    if name.startswith("null"):
        pct, where, d = name[4:].split("_")
        dtype = {"0": "int32", "10": "float64", "100": "uint16"}[pct]
        v, valid = nullable(rng, typed_values(rng, dtype, n, distinct=max(n // 4, 1)), int(pct) / 100)
        return [Col(v, valid, desc=d == "desc", nulls=where)]
    if name == "multi2":
        a, av = nullable(rng, typed_values(rng, "int8", n, distinct=5), 0.1)
        return [Col(a, av, desc=True, nulls="first"), Col(typed_values(rng, "float32", n, distinct=14))]
    if name == "multi3":
        b, bv = nullable(rng, typed_values(rng, "int64", n, distinct=4), 0.1)
        return [Col(typed_values(rng, "uint16", n, distinct=3)), Col(b, bv, nulls="last"), Col(typed_values(rng, "uint8", n, distinct=6), desc=True)]
    if name == "multi4":
        a, av = nullable(rng, typed_values(rng, "float64", n, distinct=14), 0.1)
        d, dv = nullable(rng, typed_values(rng, "int32", n, distinct=7), 0.1)
        return [Col(typed_values(rng, "int16", n, distinct=2), desc=True), Col(a, av, desc=True, nulls="last"),
                Col(typed_values(rng, "uint64", n, distinct=3)), Col(d, dv, nulls="first")]
    if name == "lead_const":
        return [Col(np.full(n, 7, dtype=U32)), Col(typed_values(rng, "int16", n, distinct=40), desc=True)]
    raise KeyError(name)


@functools.lru_cache(maxsize=256)
def case(name, n, seed=0):
    """-> (the columns, the model's permutation), computed once and shared; nobody writes into either"""
    cols = make(name, n, seed)
    want = model_perm(cols)
    want.setflags(write=False)
    for c in cols:
        c.values.setflags(write=False)
    return cols, want


def fuzz_case(seed, max_rows=20_000):
    """one random case: 1 to 4 columns of random dtypes, flags, NULL fractions and tie densities"""
    rng = np.random.default_rng([0x50F7, seed])
    n = int(rng.integers(1, max_rows + 1))
    cols = []
    for _ in range(int(rng.integers(1, 5))):
        dtype = DTYPES[int(rng.integers(0, len(DTYPES)))]
        distinct = [None, 2, 14, max(n // 3, 1)][int(rng.integers(0, 4))]
        v, valid = typed_values(rng, dtype, n, distinct), None
        if rng.random() < 0.5:
            v, valid = nullable(rng, v, [0.0, 0.1, 0.5, 1.0][int(rng.integers(0, 4))])
        cols.append(Col(v, valid, desc=bool(rng.integers(0, 2)), nulls=("last", "first")[int(rng.integers(0, 2))]))
    return cols
