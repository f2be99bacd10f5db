"""What the tests of the aggregating joins share (test_gpu_prj_agg.py, test_gpu_pairs_agg.py, test_gpu_join_aggregate.py):
the expectation -- numpy alone: np.add.at, np.minimum.at and np.maximum.at over pairs that come from numpy -- and the device
buffers with their sentinel fill and guard words. No test in here, and nothing that asks the library what a result should be."""
import numpy as np

from htm_hashjoin_amd import _lib

from gpu_harness import plane_words

U64 = np.uint64
COUNT, SUM, MIN, MAX = _lib.HJ_AGG_COUNT, _lib.HJ_AGG_SUM, _lib.HJ_AGG_MIN, _lib.HJ_AGG_MAX
SIGNED = _lib.HJ_AGG_SIGNED
SENT64 = U64(0xA5A5A5A5A5A5A5A5)
GUARD64 = 512                    # 64-bit guard words behind every output and accumulator plane
POISON = 0x7FFFFFFFFFFFFFFF      # what lies under a NULL: a value that would win a MAX and wreck a SUM
I64_MAX, U64_MAX, I64_MIN = U64(0x7FFFFFFFFFFFFFFF), U64(0xFFFFFFFFFFFFFFFF), U64(0x8000000000000000)


def identity(op, signed):
    if op == MIN:
        return I64_MAX if signed else U64_MAX
    if op == MAX:
        return I64_MIN if signed else U64(0)
    return U64(0)


def widen(a):
    """the 64-bit pattern of every element: sign- or zero-extended"""
    a = np.asarray(a)
    return a.astype(np.int64).view(U64) if a.dtype.kind == "i" else a.astype(U64)


class Col:
    """one aggregate of a test: the op, the S values (None: COUNT) and their validity (bools or None)"""

    def __init__(self, op, values=None, valid=None):
        self.op, self.values, self.valid = op, (None if values is None else np.ascontiguousarray(values)), valid
        self.signed = values is not None and op != COUNT and self.values.dtype.kind == "i"
        self.width = 0 if op == COUNT else self.values.dtype.itemsize

    @property
    def spec(self):
        return (self.op, self.width, SIGNED if self.signed else 0)

    @property
    def identity(self):
        return identity(self.op, self.signed)

    def poisoned(self):
        """the values as they go to the device: POISON (cut to the width) under every NULL"""
        if self.values is None or self.valid is None:
            return self.values
        v = self.values.copy()
        v[~self.valid] = v.dtype.type(POISON >> (64 - 8 * v.dtype.itemsize))
        return v

    def words(self, lo=0, n=None):
        """the validity bits of rows [lo, lo + n) from bit 0, as uint32 words"""
        if self.valid is None:
            return None
        part = self.valid[lo:] if n is None else self.valid[lo:lo + n]
        return plane_words(part) if part.size else np.zeros(1, dtype=np.uint32)


def reduce_at(acc, op, signed, idx, vals):
    """acc[idx] op= vals, unbuffered; acc and vals are uint64 patterns"""
    if op in (COUNT, SUM):
        np.add.at(acc, idx, vals)                    # uint64: wraps modulo 2^64
    elif op == MIN:
        np.minimum.at(acc.view(np.int64) if signed else acc, idx, vals.view(np.int64) if signed else vals)
    else:
        np.maximum.at(acc.view(np.int64) if signed else acc, idx, vals.view(np.int64) if signed else vals)


def expected(n_groups, g_idx, v_idx, cols):
    """(count, [one uint64 plane per column]) of the pairs (g_idx[k], v_idx[k]): group row, value row"""
    g_idx, v_idx = np.asarray(g_idx, dtype=np.int64), np.asarray(v_idx, dtype=np.int64)
    count = np.zeros(n_groups, dtype=U64)
    np.add.at(count, g_idx, U64(1))
    planes = []
    for c in cols:
        acc = np.full(n_groups, c.identity, dtype=U64)
        ok = np.ones(g_idx.size, dtype=bool) if c.valid is None else c.valid[v_idx]
        vals = np.ones(int(ok.sum()), dtype=U64) if c.op == COUNT else widen(c.values[v_idx[ok]])
        reduce_at(acc, c.op, c.signed, g_idx[ok], vals)
        planes.append(acc)
    return count, planes


def expected_join(n_r, inner, cols):
    """the same from packed inner pairs s << 32 | r (r_marks_common.inner_expected), grouped by R row"""
    return expected(n_r, inner & U64(0xFFFFFFFF), inner >> U64(32), cols)


def put64(dev, n, fill=SENT64):
    """a device plane of n 64-bit words at `fill` with GUARD64 sentinel words behind it"""
    a = np.full(n + GUARD64, SENT64, dtype=U64)
    a[:n] = fill
    return dev.put(a)


def get64(ctx, d, n, tag=None):
    """the plane back, its guard words checked"""
    a = np.empty(n + GUARD64, dtype=U64)
    ctx.copy_d2h(a, d)
    assert (a[n:] == SENT64).all(), (tag, "a word behind the plane was written")
    return a[:n]


class PrjAgg:
    """One aggregation over the resident R of `ctx`: begin, probes of slices, rows with sentinels and guards."""

    def __init__(self, ctx, dev, n_r, cols):
        self.ctx, self.dev, self.n_r, self.cols = ctx, dev, n_r, cols
        ctx.prj_agg_begin([c.spec for c in cols])

    def probe(self, S, lo=0):
        """S: the slice; the columns' rows [lo, lo + len(S)) go with it"""
        n, dev, held, srcs = S.size, self.dev, [], []
        for c in self.cols:
            v, w = c.poisoned(), c.words(lo, n)
            d_v = dev.put(np.ascontiguousarray(v[lo:lo + n])) if c.op != COUNT else 0
            d_w = dev.put(w) if w is not None else 0
            held += [p for p in (d_v, d_w) if p]
            srcs.append((d_v, d_w))
        dS = dev.put(np.ascontiguousarray(S))
        self.ctx.prj_probe_agg(dS, n, srcs)
        self.ctx.synchronize()
        dev.free(dS, *held)

    def rows(self, tag=None, with_count=True):
        """-> (count or None, planes): every plane prefilled with the sentinel, guards checked, every row written"""
        ctx, dev, n = self.ctx, self.dev, self.n_r
        d_out = [put64(dev, n) for _ in self.cols]
        d_cnt = put64(dev, n) if with_count else 0
        ctx.prj_agg_rows(d_out, d_cnt)
        planes = [get64(ctx, d, n, tag) for d in d_out]
        count = get64(ctx, d_cnt, n, tag) if with_count else None
        dev.free(*d_out, *([d_cnt] if with_count else []))
        return count, planes

    def check(self, want, tag=None):
        want_count, want_planes = want
        count, planes = self.rows(tag)
        assert np.array_equal(count, want_count), (tag, "count", np.flatnonzero(count != want_count)[:8])
        for i, (got, exp) in enumerate(zip(planes, want_planes)):
            assert np.array_equal(got, exp), (tag, "column", i, self.cols[i].spec, np.flatnonzero(got != exp)[:8])
