"""The constructors and the plan of htm_chain_cases.py on the CPU: every case has the property it is named for and the cause
mask its row of the table says, the plan files no conflict under a chunk that does not own its bucket -- for the directed
cases and for the relations of the bucketised fuzz --, the plan's totals are the sequential oracle's, and the vectorised
chain view is oracle.htm_chains. Layouts are host arithmetic (hj_wave_layout_info / hj_htm_chain_layout_info with no
context) for a fixed number of compute units."""
import numpy as np
import pytest

import htm_chain_cases as cc
from oracle import oracle
from fuzz_relations import make_relation

CU = 256            # the one-part cases
CU_SMALL = 32       # the cases with several parts per slice: the same slices at an eighth of the tuples


def test_layout_info_reports_the_kernels_geometry():
    lay, cl = cc.layouts(cc.SMALL, CU)
    assert (cl["slices"], cl["sliceLen"]) == (lay["nChunks"], lay["sliceLen"]) and cl["parts"] == 1 and cl["tries"] == 1
    assert cl["chainCap"] % 3 == 0 and cl["chainCountCap"] >= cl["chainCap"] and cl["chainMaxParts"] >= 5
    # parts = ceil(sliceLen / partTuples), capped
    for n in (1, 1000, 1 << 20, 1 << 24, 1 << 26, 1 << 27, 1 << 30, (1 << 32) - 1):
        for cu in (CU_SMALL, CU):
            lay, cl = cc.layouts(n, cu)
            assert cl["parts"] == min(cl["chainMaxParts"], -(-lay["sliceLen"] // cl["partTuples"])), (n, cu)
    # `tries`: the rings take the table (one ring of slots) and the scratch fits -- against the restated rule at every small
    # n, around every power of two of the bucket count, and at large sizes; the boundary is where the table reaches a ring
    for cu in (CU_SMALL, CU, 304):
        sizes = list(range(1, 1200)) + [3 * (1 << k) + d for k in range(8, 30) for d in (-4, -3, -2, -1, 0, 1)] + [(1 << 32) - 1]
        for n in sizes:
            lay, cl = cc.layouts(n, cu)
            assert cl["tries"] == cc.tries_rule(n, lay, cl), (n, cu)
        below, first = cc.rings_boundary(cu)
        lay, cl = cc.layouts(first, cu)
        assert 4 * cc.num_buckets(first) == lay["ringGranules"] * lay["granuleSlots"] == 8 * cc.num_buckets(below)
    # the scratch term alone (build_htm keeps it as a guard of its arrays): false only for tables of one or two buckets,
    # n = 5 against n = 6 -- far below the rings, so behind buildVariant 3 it never decides
    def scratch(n):
        lay, cl = cc.layouts(n, CU)
        nb = cc.num_buckets(n)
        return cl["slices"] * cl["parts"] + 1 <= nb and 2 * cl["slices"] * (1 + cl["parts"]) <= nb
    assert [scratch(n) for n in (1, 2, 3, 5, 6, 7)] == [False, False, False, False, True, True]
    assert all(scratch(n) for n in range(6, 1200)) and cc.rings_boundary(CU)[0] > 100
    import htm_hashjoin_amd as hj
    with pytest.raises(hj.HashJoinError):
        hj.htm_chain_layout_info(1 << 32, CU)
    with pytest.raises(hj.HashJoinError):
        hj.htm_chain_layout_info(1000, 0)
    n2 = cc.smallest_n_with_parts(2, CU)
    assert n2 is not None and cc.layouts(n2, CU)[1]["parts"] == 2 and cc.layouts(n2 - 1, CU)[1]["parts"] == 1
    assert cc.smallest_n_with_parts(2, CU, below=1 << 20) is None


@pytest.mark.parametrize("case", cc.ONE_PART, ids=lambda c: c.name)
def test_one_part_case_has_its_property(case):
    lay, cl = cc.layouts(cc.SMALL, CU)
    assert cl["parts"] == 1 and cl["tries"] == 1
    R, what, plan = cc.build_case(case, cc.SMALL, lay, cl)
    want = oracle.htm_build_probe_seq(R, cc.probe_side(R))
    assert (plan.conflicts.size, plan.total_groups) == (want["conflictCount"], want["overflowBuckets"])
    assert want["totalMatches"] == R.size
    assert int(plan.m.sum()) == plan.conflicts.size


@pytest.mark.parametrize("case", cc.TWO_PARTS + cc.FIVE_PARTS, ids=lambda c: c.name)
def test_case_with_several_parts_has_its_property(case):
    parts = 5 if case in cc.FIVE_PARTS else 2
    n = cc.smallest_n_with_parts(parts, CU_SMALL, below=1 << 25)
    lay, cl = cc.layouts(n, CU_SMALL)
    assert cl["parts"] == parts and cl["tries"] == 1
    R, what, plan = cc.build_case(case, n, lay, cl)
    want = oracle.htm_build_probe_seq(R)
    assert (plan.conflicts.size, plan.total_groups) == (want["conflictCount"], want["overflowBuckets"])


def test_the_plan_files_no_fuzz_conflict_under_the_wrong_chunk():
    """the relations test_bucketised_table_on_random_near_sorted_relations runs (same seeds, same draws)"""
    seen = set()
    for block in range(2):
        rng = np.random.default_rng(20261000 + block)
        for case in range(block, 18, 2):
            n = 1 << int(rng.integers(10, 19))
            R, w = make_relation(rng, n)
            R = np.ascontiguousarray(R[: n - int(rng.integers(0, 3))])
            if rng.integers(0, 2):
                rng.permutation(R)
            for cu in (CU, CU_SMALL):
                plan = cc.plan_for(R, cu)
                assert plan.strays == 0 and plan.mask & cc.BIT_STRAY == 0, (block, case, n, w, cu)
                seen.add(plan.mask)
            want = oracle.htm_build_probe_seq(R)
            assert (plan.conflicts.size, plan.total_groups) == (want["conflictCount"], want["overflowBuckets"]), (block, case)
    assert 0 in seen and len(seen) > 1          # the fuzz has relations on both sides


def test_vectorised_chain_view_is_the_oracles():
    rng = np.random.default_rng(11)
    lay, cl = cc.layouts(cc.SMALL, CU)
    rels = [rng.integers(1, 50, size=4097, dtype=np.uint64),                    # a few very long chains
            rng.integers(1, 1 << 13, size=1 << 13, dtype=np.uint64),
            np.arange(1, 1001, dtype=np.uint64),                                # no chain at all
            np.full(7, 5, dtype=np.uint64),
            cc.tail_counts(cc.SMALL, lay, cl)[0]]
    for R in rels:
        got = oracle.htm_build_probe_seq(R, None, want_buckets=True)
        a, ao = cc.chains_view(got["buckets"], got["overflows"])
        b, bo = oracle.htm_chains(got["buckets"], got["overflows"])
        assert np.array_equal(ao, bo) and np.array_equal(a, b)
        assert a.size == R.size and np.array_equal(np.sort(a), np.sort(R))      # every tuple once
    # the view follows the links, not the physical order: the same chains with the overflow buckets renumbered
    R = rels[0]
    got = oracle.htm_build_probe_seq(R, None, want_buckets=True)
    ov, bk = got["overflows"].copy(), got["buckets"].copy()
    k = ov.size - 1
    perm = np.concatenate([[0], 1 + rng.permutation(k)])                          # old index -> new index
    new = np.zeros_like(ov)
    new[perm] = ov
    new["nextIndex"] = perm[new["nextIndex"]]
    bk["nextIndex"] = perm[bk["nextIndex"]]
    a, ao = cc.chains_view(bk, new)
    b, bo = oracle.htm_chains(got["buckets"], got["overflows"])
    assert np.array_equal(ao, bo) and np.array_equal(a, b)
    # ... and tells a reversed chain from the real one
    long_chain = int(np.argmax(np.diff(bo)))
    assert bo[long_chain + 1] - bo[long_chain] > 9
    rev = got["overflows"].copy()
    ids, cur = [], int(got["buckets"]["nextIndex"][long_chain])
    while cur:
        ids.append(cur)
        cur = int(rev["nextIndex"][cur])
    rev["tuples"][ids] = rev["tuples"][ids[::-1]]
    a2, _ = cc.chains_view(got["buckets"], rev)
    assert not np.array_equal(a2, b)
