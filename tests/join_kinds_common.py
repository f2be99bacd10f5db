"""What the join-kind tests of both materialising probes share (test_gpu_join_kinds.py, test_gpu_prj_join_kinds.py): the
derivation of every kind from the inner pairs, and the full check of one call. No test in here, and nothing that asks the
library what the rows should be: `inner` always comes from numpy / plain Python."""
import numpy as np

import htm_hashjoin_amd as hj

from gpu_harness import SENTINEL, GuardedPlane  # noqa: F401

GUARD = 4096
U64 = np.uint64
INNER, LEFT, SEMI, ANTI = 0, 1, 2, 3
KINDS = (INNER, LEFT, SEMI, ANTI)
NAMES = {INNER: "inner", LEFT: "left", SEMI: "semi", ANTI: "anti"}
NO_ROW = U64(0xFFFFFFFF)


def planes(dev, capacity):
    """two output planes of `capacity` words, GUARD sentinel words directly behind each"""
    return GuardedPlane(dev, capacity, behind=GUARD), GuardedPlane(dev, capacity, behind=GUARD)


def zipf(n, alphabet, theta, seed):
    return hj.generate_relation("zipf", n, alphabet, 0, theta, seed)


def matched_rows(inner):
    return np.unique(inner >> U64(32))


def unmatched_rows(inner, n, s_base=0):
    return np.setdiff1d(np.arange(s_base, s_base + n, dtype=U64), matched_rows(inner), assume_unique=True)


def derive(kind, inner, n, s_base=0):
    """the rows of `kind` over the slice of S rows [s_base, s_base + n), from the slice's sorted inner pairs: packed and
    sorted for INNER and LEFT, sorted S rows for SEMI and ANTI"""
    if kind == INNER:
        return inner
    if kind == LEFT:
        return np.sort(np.concatenate([inner, (unmatched_rows(inner, n, s_base) << U64(32)) | NO_ROW]))
    if kind == SEMI:
        return matched_rows(inner)
    return unmatched_rows(inner, n, s_base)


class Calls:
    """the kind calls on one context since its last build: every call is checked in full, the counters after it too"""

    def __init__(self, ctx, dev, probe=None):
        self.ctx, self.dev = ctx, dev
        self.probe = probe or ctx.probe_pairs
        self.matches = self.s = 0

    def call(self, kind, dS, n, inner, s_base=0, capacity=None, tag=None):
        """one call of `kind` over n tuples at dS whose sorted inner pairs are `inner` -> the rows as written (unsorted)"""
        tag = (tag, NAMES[kind], n, s_base, capacity)
        want = derive(kind, inner, n, s_base)
        cap = want.size + 64 if capacity is None else capacity
        ds = GuardedPlane(self.dev, cap, behind=GUARD, what="a word behind the last S row was written")
        dr = GuardedPlane(self.dev, cap, behind=GUARD, what="the R plane was written" if kind in (SEMI, ANTI) else "a word behind the last R row was written")
        self.probe(dS, n, ds.ptr, dr.ptr, cap, s_base, kind=kind)
        found, written, _us, unmatched = self.ctx.pairs_info()
        self.matches += inner.size
        self.s += n
        got = self.ctx.fetch()
        print(tag, "found", found, "written", written, "unmatched", unmatched, "totalMatches", got["totalMatches"])
        assert found == want.size and written == min(found, cap), (tag, found, written, want.size)
        assert unmatched == (0 if kind == INNER else n - matched_rows(inner).size), (tag, unmatched)
        assert (got["totalMatches"], got["sSize"]) == (self.matches, self.s), (tag, got["totalMatches"], self.matches)
        s, r = ds.read(written, tag), dr.read(0 if kind in (SEMI, ANTI) else written, tag)
        rows = s.astype(U64) if kind in (SEMI, ANTI) else (s.astype(U64) << U64(32)) | r.astype(U64)
        ds.free()
        dr.free()
        if cap >= want.size:
            assert np.array_equal(np.sort(rows), want), tag
        else:
            assert np.unique(rows).size == rows.size and np.isin(rows, want).all(), tag
        return rows

    def count_only(self, kind, dS, n, n_inner, n_matched, s_base=0, tag=None):
        """one call of `kind` with capacity 0 and NULL planes, for a slice whose rows are too many to sort: the counts alone"""
        rows = {INNER: n_inner, LEFT: n_inner + n - n_matched, SEMI: n_matched, ANTI: n - n_matched}[kind]
        self.probe(dS, n, 0, 0, 0, s_base, kind=kind)
        found, written, _us, unmatched = self.ctx.pairs_info()
        self.matches += n_inner
        self.s += n
        got = self.ctx.fetch()
        assert (found, written) == (rows, 0), (tag, found, written, rows)
        assert unmatched == (0 if kind == INNER else n - n_matched), (tag, unmatched)
        assert (got["totalMatches"], got["sSize"]) == (self.matches, self.s), (tag, got["totalMatches"], self.matches)
