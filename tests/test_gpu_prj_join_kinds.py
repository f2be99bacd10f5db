"""Left-outer, semi and anti joins out of the materialising radix join (hj_prj_probe_join_dev) through ctypes -> C ABI on
an MI355X. The inner pairs come from numpy alone (Expected: restated from test_gpu_prj_pairs.py), every kind is derived
from them (join_kinds_common.derive), and every call is checked in full: the rows element for element, the guard words of
both planes (the whole R plane for SEMI and ANTI), found, the unmatched count of hj_pairs_info, and totalMatches -- which
is the INNER count whatever the kind. The relations come from the generators of prj_cases.py. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
import prj_cases as pc
from gpu_harness import Device, alloc
from join_kinds_common import SENTINEL, GUARD, U64, INNER, LEFT, SEMI, ANTI, KINDS, NAMES, Calls, derive, matched_rows, planes

pytestmark = pytest.mark.gpu

LOW = U64(0xFFFFFFFF)
COUNTERS = ("totalMatches", "sSize", "prjChecksum", "radixBits", "prjPartitions")
COUNT_ONLY_ABOVE = 1 << 25       # a slice with more reference rows may be checked by count only (raised HJ_FUZZ_CASES)
PAIR_BLOCK_TUPLES = 11520        # kPairBlockTuples: R tuples of one LDS build of the pairs join
STAGE = 4096                     # kStagePairs: rows per stage


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


def all_kinds(R, S, bits, kinds=KINDS, tag=None, inner=None):
    """build R, then every kind over S on one context; -> {kind: work items of its probe}"""
    inner = Expected(R).pairs(S) if inner is None else inner
    items = {}
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        c.reserve("prj", R.size, S.size, radixBits=bits, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        c.prj_build(dR, R.size)
        calls = Calls(c, dev, c.prj_probe_pairs)
        for kind in kinds:
            calls.call(kind, dS, S.size, inner, tag=tag)
            items[kind] = c.prj_resident_info()["items"]
    return items


# ---------------------------------------------------------------------------------------------------------------------
# partitions with S tuples and no R tuple
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [11, 0])
def test_partitions_without_r_tuples(bits):
    """R = 8 keys: almost every partition of S has no R tuple and, for INNER and SEMI, no work item. LEFT and ANTI must
    return every one of those S tuples."""
    n = 1 << 14
    R = np.array([3, 700, 701, 5000, 9999, 12000, 16000, 16384], dtype=U64)
    S = pc.uniform(n, n, 1000, bits)
    inner = Expected(R).pairs(S)
    assert 0 < inner.size < 64
    items = all_kinds(R, S, bits, tag=("r-less", bits))
    P = 1 << pc.resolved_bits(R.size, bits)
    parts_r, parts_s = np.unique(R & U64(P - 1)), np.unique(S & U64(P - 1))
    with_both = np.intersect1d(parts_r, parts_s).size
    assert parts_s.size > 8 * parts_r.size and with_both > 0
    assert items[INNER] == items[SEMI] == with_both and items[LEFT] == items[ANTI] == parts_s.size


# ---------------------------------------------------------------------------------------------------------------------
# an R partition built in several LDS blocks: "matched" has to survive the block loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [14, 16])
def test_one_key_a_hundred_thousand_times(bits):
    """The hot key's partition takes 9 LDS builds. S holds, in that partition: (a) the hot key 20 times (matches in every
    block: SEMI once), (b) keys R holds once (a match in one block, which need not be the last: no NO_ROW row in the last
    one), (c) keys R does not hold (unmatched in every block: one row, in the last)."""
    dense = 1 << 18
    hot = U64(dense + 77)
    R = pc.shuffled([np.arange(1, dense + 1, dtype=U64), np.full(100000, hot, dtype=U64)], 910, bits)
    per = dense >> bits                                       # keys of partition 77 inside 1..dense
    once = pc.hot_keys(77, bits, 0, per)
    absent = pc.hot_keys(77, bits, per + 1, 50)
    assert int(hot) == 77 + (per << bits) and np.isin(once, R).all() and not np.isin(absent, R).any()
    assert (100000 + per) > 8 * PAIR_BLOCK_TUPLES
    rest = pc.uniform(1 << 12, dense + (1 << 16), 911, bits)
    rest = rest[(rest & U64((1 << bits) - 1)) != 77]           # the other partitions; some of these keys are absent from R too
    S = pc.shuffled([rest, np.full(20, hot, dtype=U64), once, once[:2], absent, absent[:3]], 912, bits)
    inner = Expected(R).pairs(S)
    s_hot, s_once, s_absent = (np.flatnonzero(np.isin(S, k)).astype(U64) for k in (hot, once, absent))
    assert (s_hot.size, s_once.size, s_absent.size) == (20, per + 2, 53)
    assert np.isin(s_hot, derive(SEMI, inner, S.size)).all() and np.isin(s_once, derive(SEMI, inner, S.size)).all()
    assert np.isin(s_absent, derive(ANTI, inner, S.size)).all()
    assert inner.size >= 20 * 100000 + per + 2
    all_kinds(R, S, bits, tag=("blocks", bits), inner=inner)


# ---------------------------------------------------------------------------------------------------------------------
# an S partition split over several items
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,n_items", list(zip(pc.BOUNDARY_SIZES, pc.BOUNDARY_ITEMS)))
def test_split_s_partitions(size, n_items):
    """`size` S tuples in ONE partition (low 8 key bits constant, 8 radix bits), half of their keys absent from R: every S
    tuple is a row of exactly one of the partition's items."""
    hi, low = 1 << 12, 0x5A
    R = pc.shuffled([(np.arange(1, hi // 2 + 1, dtype=U64) << U64(8)) | U64(low), pc.uniform(1000, 1 << 20, 1010)], 1011)
    S = pc.const_low_bits(size, hi, low, 1012)
    inner = Expected(R).pairs(S)
    assert S.size // 3 < matched_rows(inner).size < 2 * S.size // 3
    items = all_kinds(R, S, 8, tag=("split", size), inner=inner)
    assert all(items[k] == n_items for k in KINDS)


# ---------------------------------------------------------------------------------------------------------------------
# padding lanes hold a clamped copy of the item's last element
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("none_match", [False, True])
@pytest.mark.parametrize("size", [1, 2047, 2049, pc.ITEM_S + 1])
def test_clamped_copies_of_the_last_tuple_write_no_rows(size, none_match):
    """One partition again, so that the slice is one item (two for ITEM_S + 1: the second holds one tuple). The last tuple
    of the slice is unmatched; none_match: so is every other one, which makes the last element of the item unmatched
    whatever order the partitioning leaves the item in."""
    hi, low = 1 << 12, 0x33
    R = (np.arange(1, hi // 2 + 1, dtype=U64) << U64(8)) | U64(low)
    S = pc.const_low_bits(size, hi, low, 1020, size).copy()
    if none_match:
        S += U64(hi) << U64(8)
    S[-1] = (U64(hi + 5) << U64(8)) | U64(low)
    inner = Expected(R).pairs(S)
    assert size - 1 not in matched_rows(inner) and (inner.size == 0) == (none_match or size == 1)
    all_kinds(R, S, 8, tag=("clamp", size, none_match), inner=inner)


# ---------------------------------------------------------------------------------------------------------------------
# rounds with more rows than a stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 5])
def test_duplicates_on_both_sides_left(bits):
    n = 1 << 17
    R = pc.uniform(1 << 18, n, 1030)
    S = pc.uniform(n + 7, n + (1 << 15), 1031)
    all_kinds(R, S, bits, kinds=(LEFT, INNER), tag=("dups", bits))


def test_rounds_above_a_stage_left():
    """Eight R copies per key in partitions of 2^14 R tuples (two LDS builds, about four copies in each) and 2^12 S tuples:
    a round of 2048 S elements brings about 6500 inner rows, more than a stage, so the lanes write straight to the planes
    at offsets computed from the rows of the kind -- in the last block the unmatched rows among them."""
    R = pc.uniform(1 << 18, 1 << 15, 1040)
    S = pc.uniform(1 << 16, (1 << 15) + (1 << 13), 1041)
    exp = Expected(R)
    inner = exp.pairs(S)
    # partition 0 takes two LDS builds, and 2048 of its S elements have more than two stages of inner rows in all: in one
    # of the two builds they have more than one stage
    in_p0 = (S & U64(15)) == 0
    assert PAIR_BLOCK_TUPLES < int(((R & U64(15)) == 0).sum()) <= 2 * PAIR_BLOCK_TUPLES
    assert int(exp.runs(S[in_p0][:2048])[1].sum()) > 2 * STAGE
    all_kinds(R, S, 4, kinds=(LEFT, SEMI, ANTI), tag="direct", inner=inner)


# ---------------------------------------------------------------------------------------------------------------------
# seeded random relations, ragged slices with a running sIdxBase
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [0, 1])
def test_random_relations_in_ragged_slices(block):
    """Every slice's rows, written with the slice's offset in S as sIdxBase, are the kind applied to the slice -- so the
    union over the slices is the kind applied to the whole S. One kind per case (1 + index % 3)."""
    slices = count_only = 0
    with hj.HashJoinContext(0) as c:
        for index in range(block, pc.fuzz_case_count(), pc.FUZZ_BLOCKS):
            R, S, lens, bits, shape = pc.random_relations(block, index)
            kind = 1 + index % 3
            exp = Expected(R)
            with Device(c) as dev:
                c.reserve("prj", R.size, max(lens), radixBits=bits, prjMode=index % 3, keepRowIds=True)
                dR, dS = dev.put(R), dev.alloc(8 * max(lens))
                c.prj_build(dR, R.size)
                calls = Calls(c, dev, c.prj_probe_pairs)
                off = 0
                for m in lens:
                    part = S[off:off + m]
                    tag = (block, index, shape, bits, off, m)
                    c.copy_h2d(dS, part)
                    slices += 1
                    cnt = exp.runs(part)[1]
                    n_inner, n_matched = int(cnt.sum()), int((cnt > 0).sum())
                    if max(n_inner + m - n_matched, n_inner) > COUNT_ONLY_ABOVE:
                        count_only += 1
                        calls.count_only(kind, dS, m, n_inner, n_matched, s_base=off, tag=tag)
                    else:
                        calls.call(kind, dS, m, exp.pairs(part, s_base=off), s_base=off, tag=tag)
                    off += m
                assert calls.s == S.size and calls.matches == pc.reference_matches(R & LOW, S & LOW), (block, index)
    if pc.fuzz_case_count() <= 36:
        assert count_only == 0, "no slice of the default cases is large enough to be checked by count only"
    assert 10 * count_only <= slices, (count_only, slices)


# ---------------------------------------------------------------------------------------------------------------------
# the other probes on the same context
# ---------------------------------------------------------------------------------------------------------------------
def test_other_probes_on_the_same_context():
    """After kind calls, hj_prj_probe_dev and hj_prj_probe_pairs_dev count and write what they did before (R-less items
    and the unmatched word do not linger), and a plain context fed the same slices ends with equal counters."""
    n = 1 << 15
    R = pc.uniform(n, 1 << 13, 1050)                          # keys up to 2^13: half of the 2^14 partitions hold no R tuple
    S = pc.uniform(n, 1 << 14, 1051)
    cuts = [0, 5000, 5001, n]
    exp = Expected(R)
    with hj.HashJoinContext(0) as c, hj.HashJoinContext(0) as plain, Device(c) as dev:
        c.reserve("prj", n, n, radixBits=14, keepRowIds=True)
        plain.reserve("prj", n, n, radixBits=14)
        dR, dS = dev.put(R), dev.put(S)
        pR, pS = alloc(plain, 8 * n), alloc(plain, 8 * n)
        try:
            plain.copy_h2d(pR, R); plain.copy_h2d(pS, S)
            c.prj_build(dR, n); plain.prj_build(pR, n)
            calls = Calls(c, dev, c.prj_probe_pairs)
            for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                inner = exp.pairs(S[a:b], s_base=a)
                for kind in (KINDS[(k + 1) % 4], ANTI, LEFT):
                    calls.call(kind, dS + 8 * a, b - a, inner, s_base=a, tag=("same", k))
                    plain.prj_probe(pS + 8 * a, b - a)
                items_left = c.prj_resident_info()["items"]
                # the counting probe on the row-id context: the INNER join with capacity 0; the last kind call's facts stay
                info = c.pairs_info()
                c.prj_probe(dS + 8 * a, b - a); plain.prj_probe(pS + 8 * a, b - a)
                calls.matches += inner.size; calls.s += b - a
                assert c.pairs_info()[:2] == info[:2] and c.pairs_info()[3] == info[3]
                items_count = c.prj_resident_info()["items"]
                # the pairs probe through its old entry point
                ds, dr = (p.ptr for p in planes(dev, inner.size + 64))
                assert hj.lib.hj_prj_probe_pairs_dev(c._h, dS + 8 * a, b - a, a, ds, dr, inner.size + 64) == 0
                plain.prj_probe(pS + 8 * a, b - a)
                calls.matches += inner.size; calls.s += b - a
                assert c.pairs_info()[:2] == (inner.size, inner.size) and c.pairs_info()[3] == 0
                assert c.prj_resident_info()["items"] == items_count <= items_left
                s, r = dev.get(ds, inner.size + 64 + GUARD), dev.get(dr, inner.size + 64 + GUARD)
                dev.free(ds, dr)
                assert (s[inner.size:] == SENTINEL).all() and (r[inner.size:] == SENTINEL).all()
                assert np.array_equal(np.sort((s[:inner.size].astype(U64) << U64(32)) | r[:inner.size].astype(U64)), inner)
                got = c.fetch()
                assert (got["totalMatches"], got["sSize"]) == (calls.matches, calls.s)
            assert counters(c) == counters(plain)
        finally:
            plain.dev_free(pR); plain.dev_free(pS)


# ---------------------------------------------------------------------------------------------------------------------
# host-buffer convenience
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", [NAMES[k] for k in KINDS])
def test_radix_join_pairs_round_trip(how):
    n = 1 << 14
    R = pc.uniform(12345, n // 4, 960)
    S = pc.uniform(n, n // 2, 961)                          # ~3 R copies per key, half of the S keys absent from R
    kind = {v: k for k, v in NAMES.items()}[how]
    inner = Expected(R).pairs(S)
    assert inner.size > S.size                               # the outputs grow once for inner and left
    want = derive(kind, inner, S.size)
    for kw in ({}, {"slice_tuples": 5000}, {"slice_tuples": n, "radixBits": 11}, {"slice_tuples": 3 * n}):
        s_idx, r_idx = hj.radix_join_pairs(R, S, how=how, **kw)
        assert s_idx.dtype == np.uint32 and s_idx.size == want.size, kw
        if kind in (SEMI, ANTI):
            assert r_idx is None, kw
            assert np.array_equal(np.sort(s_idx.astype(U64)), want), kw
            continue
        assert r_idx.dtype == np.uint32 and r_idx.size == s_idx.size, kw
        assert np.array_equal(np.sort((s_idx.astype(U64) << U64(32)) | r_idx), want), kw
        hit = r_idx != hj.NO_ROW
        assert np.array_equal(S[s_idx[hit]], R[r_idx[hit]]), kw               # the gather maps do what they are for
        assert hit.all() if kind == INNER else (~hit).sum() == S.size - matched_rows(inner).size, kw
