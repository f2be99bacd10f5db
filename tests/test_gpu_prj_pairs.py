"""The materialising radix join (hj_prj_build_dev on a context reserved with HJ_FLAG_KEEP_ROW_IDS, hj_prj_probe_pairs_dev)
through ctypes -> C ABI on an MI355X. The expected pairs come from numpy alone, never from the library: sort R by its key
word, searchsorted the key words of S, expand the runs. Pairs are compared as sorted arrays of s << 32 | r, element for
element: no pair missing, none twice. Every output plane has sentinel words behind its capacity and is checked for them
behind the written part as well. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import Device, alloc, status
import prj_cases as pc
from htm_hashjoin_amd import _lib

pytestmark = pytest.mark.gpu

from join_kinds_common import SENTINEL, GUARD, U64, planes
from r_marks_common import LOW
COUNTERS = ("totalMatches", "sSize", "prjChecksum", "radixBits", "prjPartitions")
COUNT_ONLY_ABOVE = 1 << 25       # a slice with more reference pairs may be checked by count only (raised HJ_FUZZ_CASES)


def probe_pairs(ctx, dev, dS, n, capacity, s_idx_base=0):
    """one hj_prj_probe_pairs_dev call -> (found, packed pairs as written (unsorted), guard words intact)"""
    ds, dr = (p.ptr for p in planes(dev, capacity))
    ctx.prj_probe_pairs(dS, n, ds, dr, capacity, s_idx_base)
    found, written, _us, zero = ctx.pairs_info()
    assert written == min(found, capacity) and zero == 0
    s, r = dev.get(ds, capacity + GUARD), dev.get(dr, capacity + GUARD)
    dev.free(ds, dr)
    guard_ok = bool((s[capacity:] == SENTINEL).all() and (r[capacity:] == SENTINEL).all())
    if written < capacity:          # nothing behind the last pair either
        guard_ok = guard_ok and bool((s[written:capacity] == SENTINEL).all() and (r[written:capacity] == SENTINEL).all())
    packed = (s[:written].astype(U64) << U64(32)) | r[:written].astype(U64)
    return found, packed, guard_ok


class Expected:
    """the join against one R, slice by slice: all (i, j) with low32(S[i]) == low32(R[j]), packed and sorted"""

    def __init__(self, R):
        keys = np.ascontiguousarray(R, dtype=U64) & LOW
        self.order = np.argsort(keys, kind="stable")
        self.keys = keys[self.order]

    def runs(self, S):
        k = np.ascontiguousarray(S, dtype=U64) & LOW
        lo = np.searchsorted(self.keys, k, "left")
        return lo, np.searchsorted(self.keys, k, "right") - lo

    def count(self, S):
        return int(self.runs(S)[1].sum())

    def pairs(self, S, s_base=0):
        lo, cnt = self.runs(S)
        total = int(cnt.sum())
        s_idx = np.repeat(np.arange(S.size, dtype=np.int64), cnt)
        within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        r_idx = self.order[np.repeat(lo, cnt) + within]
        return np.sort(((s_idx + s_base).astype(U64) << U64(32)) | r_idx.astype(U64))


def counters(ctx):
    got = ctx.fetch()
    return tuple(got[k] for k in COUNTERS)


# ---------------------------------------------------------------------------------------------------------------------
# the case table of the counting join, every probe materialised
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_case_table_pairs_are_exact_at_every_probe(case):
    """Every step on two contexts side by side: `c` reserved with the flag (pairs), `plain` without it (counts). After
    every probe the slice's pairs are exact and found == reference_matches; at the end of every build's steps the
    counters of the two contexts are equal."""
    steps = case.steps()
    n_r, n_s = pc.reserve_sizes(steps)
    kw = dict(radixBits=case.bits, prjMode=case.mode)
    with hj.HashJoinContext(0) as c, hj.HashJoinContext(0) as plain, Device(c) as dev:
        c.reserve("prj", n_r, n_s, keepRowIds=True, **kw)
        plain.reserve("prj", n_r, n_s, **kw)
        dR, dS = dev.alloc(n_r * 8), dev.alloc(n_s * 8)
        pR, pS = alloc(plain, n_r * 8), alloc(plain, n_s * 8)
        try:
            R = exp = r_counts = None
            total = 0
            for k, st in enumerate(steps):
                tag = (case.name, k, st.op)
                if st.op == "build":
                    if R is not None:
                        assert counters(c) == counters(plain), tag
                    R, total = st.arr, 0
                    exp = Expected(R)
                    r_counts = case.once((k, "counts"), lambda: pc.key_counts(st.arr))
                    c.copy_h2d(dR, R); plain.copy_h2d(pR, R)
                    c.prj_build(dR, R.size); plain.prj_build(pR, R.size)
                    got = c.fetch()
                    assert got["totalMatches"] == 0 and got["sSize"] == 0 and got["prjPath"] == 0, (tag, got)
                    assert counters(c) == counters(plain), tag
                    info = c.prj_resident_info()
                    assert info["rPath"] == 0 and info["residentBytes"] >= 8 * R.size, (tag, info)
                    continue
                if st.op == "reserve":
                    c.reserve("prj", n_r, n_s, keepRowIds=True, **kw)      # reallocates nothing: R stays resident
                    plain.reserve("prj", n_r, n_s, **kw)
                    continue
                if st.op == "empty":
                    c.prj_probe_pairs(dS, 0, 0, 0, 0)
                    plain.prj_probe(pS, 0)
                    assert c.fetch()["totalMatches"] == total, tag
                    continue
                S = st.arr
                c.copy_h2d(dS, S); plain.copy_h2d(pS, S)
                want = exp.pairs(S)
                found, packed, guard_ok = probe_pairs(c, dev, dS, S.size, want.size + 64)
                plain.prj_probe(pS, S.size)
                ref = case.once((k, "matches"), lambda: pc.reference_matches(R, S, r_counts))
                print(case.name, k, "pairs", found, "reference_matches", ref)
                assert found == ref == want.size, (tag, found, ref, want.size)
                assert guard_ok, tag
                assert np.array_equal(np.sort(packed), want), tag
                total += found
                got = c.fetch()
                assert got["totalMatches"] == total and got["prjPath"] == 0, (tag, got, total)
                assert c.prj_resident_info()["sPath"] == 0, tag
            assert counters(c) == counters(plain), (case.name, "end")
        finally:
            plain.dev_free(pR); plain.dev_free(pS)


# ---------------------------------------------------------------------------------------------------------------------
# seeded random relations, ragged slices with a running sIdxBase
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(pc.FUZZ_BLOCKS))
def test_random_relations_in_ragged_slices(block):
    """Every slice's pairs, written with the slice's offset in S as sIdxBase, are exactly the slice's part of the join of
    the whole S -- so the concatenation over the slices is that join. One prjMode per case (index % 3)."""
    slices = count_only = ran = 0
    with hj.HashJoinContext(0) as c:
        for index in range(block, pc.fuzz_case_count(), pc.FUZZ_BLOCKS):
            R, S, lens, bits, shape = pc.random_relations(block, index)
            mode = index % 3
            exp = Expected(R)
            with Device(c) as dev:
                c.reserve("prj", R.size, max(lens), radixBits=bits, prjMode=mode, keepRowIds=True)
                dR, dS = dev.put(R), dev.alloc(8 * max(lens))
                c.prj_build(dR, R.size)
                off = total = 0
                for m in lens:
                    part = S[off:off + m]
                    tag = (block, index, shape, bits, mode, off, m)
                    c.copy_h2d(dS, part)
                    slices += 1
                    n_ref = exp.count(part)
                    if n_ref > COUNT_ONLY_ABOVE:
                        count_only += 1
                        c.prj_probe_pairs(dS, m, 0, 0, 0, off)
                        assert c.pairs_info()[:2] == (n_ref, 0), tag
                    else:
                        want = exp.pairs(part, s_base=off)
                        found, packed, guard_ok = probe_pairs(c, dev, dS, m, want.size + 64, s_idx_base=off)
                        print("random", *tag, "pairs", found)
                        assert found == want.size and guard_ok, (tag, found, want.size)
                        assert np.array_equal(np.sort(packed), want), tag
                    total += n_ref
                    off += m
                got = c.fetch()
                assert (got["totalMatches"], got["sSize"]) == (total, S.size), (block, index, got)
                assert total == pc.reference_matches(R & LOW, S & LOW), (block, index)
            ran += 1
    assert ran == len(range(block, pc.fuzz_case_count(), pc.FUZZ_BLOCKS))
    if pc.fuzz_case_count() <= 36:
        assert count_only == 0, "no slice of the default cases is large enough to be checked by count only"
    assert 10 * count_only <= slices, (count_only, slices)


# ---------------------------------------------------------------------------------------------------------------------
# capacity
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_cuts_the_output_and_nothing_else():
    n = 1 << 18
    R = pc.uniform(n, n // 2, 900)                          # duplicate keys: pairs per S tuple vary
    S = pc.uniform(n // 2 + 7, n // 2 + n // 8, 901)
    exp = Expected(R)
    want = exp.pairs(S)
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        c.reserve("prj", R.size, S.size, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        c.prj_build(dR, R.size)
        for capacity in (want.size, want.size + 1, want.size - 1, 0):
            found, packed, guard_ok = probe_pairs(c, dev, dS, S.size, capacity)
            assert found == want.size and packed.size == min(found, capacity), (capacity, found, packed.size)
            assert guard_ok, f"a word at or behind dOut*[{capacity}] was written"
            if capacity >= want.size:
                assert np.array_equal(np.sort(packed), want)
            else:
                assert np.unique(packed).size == packed.size and np.isin(packed, want).all()
        c.prj_probe_pairs(dS, S.size, 0, 0, 0)             # capacity 0 with NULL outputs: counts only
        assert c.pairs_info()[:2] == (want.size, 0)
        got = c.fetch()
    assert got["totalMatches"] == 5 * want.size and got["sSize"] == 5 * S.size


# ---------------------------------------------------------------------------------------------------------------------
# heavy duplicates in R: several LDS builds of one partition, with equal keys
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [14, 16])
def test_one_key_a_hundred_thousand_times(bits):
    dense = 1 << 18
    hot = U64(dense + 77)
    R = pc.shuffled([np.arange(1, dense + 1, dtype=U64), np.full(100000, hot, dtype=U64)], 910, bits)
    S = pc.shuffled([pc.uniform(1 << 16, dense, 911, bits), np.full(20, hot, dtype=U64)], 912, bits)
    want = Expected(R).pairs(S)
    assert want.size == 20 * 100000 + (1 << 16)
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        c.reserve("prj", R.size, S.size, radixBits=bits, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        c.prj_build(dR, R.size)
        found, packed, guard_ok = probe_pairs(c, dev, dS, S.size, want.size + 64)
        got = c.fetch()
    assert found == want.size == got["totalMatches"] and guard_ok
    assert np.array_equal(np.sort(packed), want)


# ---------------------------------------------------------------------------------------------------------------------
# the key word alone
# ---------------------------------------------------------------------------------------------------------------------
def test_upper_tuple_bits_are_ignored_and_key_zero_is_a_key():
    n = 1 << 16
    R = hj.generate_relation("nonunique", n, 1 << 12, seed=12345)
    S = hj.generate_relation("nonunique", n // 2 + 3, 1 << 12, seed=54321)
    assert (R == 0).any() and (S == 0).any()
    rng = np.random.default_rng(920)
    Rup = R | (rng.integers(0, 1 << 31, size=R.size, dtype=U64) << U64(32))        # R's own upper word is dropped
    Sup = S | (rng.integers(1, 1 << 31, size=S.size, dtype=U64) << U64(32))
    want = Expected(R).pairs(S)
    zero_pairs = int((R == 0).sum()) * int((S == 0).sum())
    assert zero_pairs > 0
    for r_in, s_in in ((R, S), (R, Sup), (Rup, Sup)):
        with hj.HashJoinContext(0) as c, Device(c) as dev:
            c.reserve("prj", n, S.size, keepRowIds=True)
            dR, dS = dev.put(r_in), dev.put(s_in)
            c.prj_build(dR, n)
            found, packed, guard_ok = probe_pairs(c, dev, dS, S.size, want.size + 64)
        assert found == want.size and guard_ok
        assert np.array_equal(np.sort(packed), want)
        s_idx, r_idx = (packed >> U64(32)).astype(np.int64), (packed & LOW).astype(np.int64)
        assert int(((S[s_idx] == 0) & (R[r_idx] == 0)).sum()) == zero_pairs


# ---------------------------------------------------------------------------------------------------------------------
# errors, no-ops, the counting probe on the same context, rebuilds
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_noops():
    n = 1 << 14
    R = pc.unique_shuffled(n)
    S = pc.uniform(n, n + n // 4, 930)
    exp = Expected(R)
    want = exp.pairs(S)
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        dR, dS = dev.put(R), dev.put(S)
        ds, dr = (p.ptr for p in planes(dev, n))
        # no resident R
        c.reserve("prj", n, n, keepRowIds=True)
        assert status(c.prj_probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        c.prj_join(dR, n, dS, n)                                     # the one-shot join leaves nothing resident
        assert status(c.prj_probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        # a resident R built without the flag; the table probe's entry point keeps refusing a PRJ context
        c.reserve("prj", n, n)
        c.prj_build(dR, n)
        assert status(c.prj_probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        assert status(c.probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        c.prj_probe(dS, n)
        assert c.fetch()["totalMatches"] == want.size
        assert (dev.get(ds, n) == SENTINEL).all()
        # with the flag
        c.reserve("prj", n, n, keepRowIds=True)
        c.prj_build(dR, n)
        assert status(c.probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        assert status(c.prj_probe_pairs, dS, n + 1, ds, dr, n) == _lib.HJ_ERR_STATE         # above the reserved slice
        assert status(c.prj_probe_pairs, dS, n, 0, dr, n) == _lib.HJ_ERR_INVALID
        assert status(c.prj_probe_pairs, dS, n, ds, 0, n) == _lib.HJ_ERR_INVALID
        assert status(c.prj_probe_pairs, dS, n, ds, dr, n, s_idx_base=(1 << 32) - n) == _lib.HJ_ERR_INVALID
        assert c.fetch()["totalMatches"] == 0                         # nothing of the refused calls was counted
        assert status(c.prj_probe_pairs, dS, n, ds, dr, n, s_idx_base=(1 << 32) - 1 - n) == _lib.HJ_OK
        found, written = c.pairs_info()[:2]
        assert found == written == want.size
        s = dev.get(ds, n)[:written]
        assert s.min() >= (1 << 32) - 1 - n and s.max() <= (1 << 32) - 2
        assert np.array_equal(np.sort(s.astype(U64) - U64((1 << 32) - 1 - n)), want >> U64(32))
        # sSize 0: outputs, counters and the last call's facts stay as they are
        c.prj_probe_pairs(dS, n, ds, dr, n)
        before, info = c.fetch(), c.pairs_info()
        s0, r0 = dev.get(ds, n + GUARD), dev.get(dr, n + GUARD)
        c.prj_probe_pairs(dS, 0, ds, dr, n)
        c.prj_probe_pairs(0, 0, 0, 0, 0)
        after = c.fetch()
        assert (after["totalMatches"], after["sSize"]) == (before["totalMatches"], before["sSize"]) == (2 * want.size, 2 * n)
        assert c.pairs_info()[:2] == info[:2] == (want.size, want.size)
        assert np.array_equal(dev.get(ds, n + GUARD), s0) and np.array_equal(dev.get(dr, n + GUARD), r0)
        # the counting probe on the same context: counts the same, leaves the planes and the last pairs call's facts alone
        c.prj_probe(dS, n)
        c.prj_probe(dS, 1000)
        after = c.fetch()
        assert after["totalMatches"] == 3 * want.size + exp.count(S[:1000]) and after["sSize"] == 3 * n + 1000
        assert c.pairs_info()[:2] == (want.size, want.size)
        assert np.array_equal(dev.get(ds, n + GUARD), s0) and np.array_equal(dev.get(dr, n + GUARD), r0)
        found, packed, guard_ok = probe_pairs(c, dev, dS, n, want.size + 64)       # and pairs again after it
        assert found == want.size and guard_ok and np.array_equal(np.sort(packed), want)


@pytest.mark.parametrize("algo", ["prj", "auto"])
def test_rebuilds_leave_the_pairs_correct(algo):
    n = 1 << 17
    R1 = pc.unique_shuffled(n)
    R2 = pc.uniform(n - 1001, n // 3, 940)                  # another size, duplicate keys
    S = pc.uniform(n // 2, n, 941)
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        c.reserve(algo, n, S.size, keepRowIds=True)
        d1, d2, dS = dev.put(R1), dev.put(R2), dev.put(S)
        for R, dR in ((R1, d1), (R1, d1), (R2, d2), (R1, d1)):
            want = Expected(R).pairs(S)
            c.prj_build(dR, R.size)
            found, packed, guard_ok = probe_pairs(c, dev, dS, S.size, want.size + 64)
            got = c.fetch()
            assert found == want.size == got["totalMatches"] and got["rSize"] == R.size and guard_ok
            assert np.array_equal(np.sort(packed), want)


# ---------------------------------------------------------------------------------------------------------------------
# one larger run, checked without sorting
# ---------------------------------------------------------------------------------------------------------------------
def test_foreign_key_join_of_2p26_tuples():
    n = 1 << 26
    R = pc.unique_shuffled(n)
    S = R[np.random.default_rng(950).integers(0, n, size=n)]          # foreign keys into R
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        c.reserve("prj", n, n, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        c.prj_build(dR, n)
        ds, dr = (p.ptr for p in planes(dev, n))
        c.prj_probe_pairs(dS, n, ds, dr, n)
        found, written = c.pairs_info()[:2]
        s_idx, r_idx = dev.get(ds, n + GUARD), dev.get(dr, n + GUARD)
        got = c.fetch()
    assert found == written == n == got["totalMatches"]
    assert (s_idx[n:] == SENTINEL).all() and (r_idx[n:] == SENTINEL).all()
    s_idx, r_idx = s_idx[:n], r_idx[:n]
    assert np.array_equal(S[s_idx] & LOW, R[r_idx] & LOW)
    assert (np.bincount(s_idx, minlength=n) == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# host-buffer convenience
# ---------------------------------------------------------------------------------------------------------------------
def test_radix_join_pairs_round_trip():
    n = 1 << 14
    R = pc.uniform(12345, n // 4, 960)
    S = pc.uniform(n, n // 4, 961)                          # ~3 R copies per S key: more than |S| pairs, so the outputs grow once
    want = Expected(R).pairs(S)
    assert want.size > S.size
    for kw in ({}, {"slice_tuples": 5000}, {"slice_tuples": n, "radixBits": 11}, {"slice_tuples": 3 * n}):
        s_idx, r_idx = hj.radix_join_pairs(R, S, **kw)
        assert s_idx.dtype == r_idx.dtype == np.uint32 and s_idx.size == r_idx.size == want.size, kw
        assert np.array_equal(S[s_idx], R[r_idx]), kw                  # the gather maps do what they are for
        assert np.array_equal(np.sort((s_idx.astype(U64) << U64(32)) | r_idx), want), kw
    e_s, e_r = hj.radix_join_pairs(R, S[:0])
    assert e_s.size == e_r.size == 0
    with pytest.raises(ValueError):
        hj.join_pairs(R, S, algo="prj")                     # the table probe's convenience keeps refusing the radix join
