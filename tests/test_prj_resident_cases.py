"""The case table of the resident radix join's differential tests (tests/prj_cases.py), checked without a GPU: the table
must reach every branch the GPU tests are there for -- judged from the partition histograms (expected_plan) and the
host-side planner (planned), not from a device run -- and its plain numpy reference must agree with the oracle's
independent join cardinality. No cell of the coverage below is allowed to be missing."""
import ctypes
import itertools

import numpy as np
import pytest

import htm_hashjoin_amd as hj
import prj_cases as pc
from oracle import oracle

CROSS_CHECK_MAX = 1 << 22          # |R|, |S| up to which oracle.true_cardinality is run next to reference_matches


@pytest.fixture(scope="module")
def survey():
    """One walk over the table (the relations of a case are generated once): what every probe of every case must do."""
    seen = {"cells": {}, "r_c2": {}, "r_unplanned": [], "r_tail": [], "s_tail": [], "no_items": [], "boundary": {},
            "cross": [], "paths": set()}
    for case in pc.CASES:
        steps = case.steps()
        bits = pc.resolved_bits(pc.reserve_sizes(steps)[0], case.bits)
        R = r_counts = None
        for k, st in enumerate(steps):
            if st.op == "build":
                R, r_counts = st.arr, None
                g = pc.planned(R.size, bits, case.mode)
                if g.planned:
                    seen["r_c2"].setdefault(g.C2, []).append(case.name)
                    if g.tail:
                        seen["r_tail"].append(case.name)
                else:
                    seen["r_unplanned"].append(case.name)
                seen["paths"].add(("r", tuple(sorted(st.paths))))
            elif st.op == "probe":
                S = st.arr
                plan = pc.expected_plan(R, S, bits)
                for cell in plan["cells"]:
                    seen["cells"].setdefault(cell, []).append((case.name, k))
                if plan["items"] == 0:
                    seen["no_items"].append((case.name, k))
                if pc.planned(S.size, bits, case.mode).tail:
                    seen["s_tail"].append((case.name, k))
                seen["paths"].add(("s", tuple(sorted(st.paths))))
                if case.name.startswith("boundaries"):
                    parts = pc.boundary_partitions(bits)
                    seen["boundary"][case.name] = ([int(plan["sSizes"][p]) for p in parts],
                                                   [int(plan["itemsPerPartition"][p]) for p in parts], plan)
                if R.size <= CROSS_CHECK_MAX and S.size <= CROSS_CHECK_MAX:
                    if r_counts is None:
                        r_counts = pc.key_counts(R)
                    seen["cross"].append((case.name, k, pc.reference_matches(R, S, r_counts), oracle.true_cardinality(R, S)))
    return seen


def test_reference_matches_by_hand():
    R = np.array([5, 5, 7, 9, 2**32 - 1, 11], dtype=np.uint64)
    S = np.array([5, 7, 7, 7, 8, 2**32 - 1, 2**32 - 1, 5], dtype=np.uint64)
    assert pc.reference_matches(R, S) == 2 * 2 + 1 * 3 + 1 * 2
    assert pc.reference_matches(R, S, pc.key_counts(R)) == 9
    assert pc.reference_matches(R, np.array([1, 3], dtype=np.uint64)) == 0
    assert pc.reference_matches(R, np.array([12], dtype=np.uint64)) == 0              # beyond R's largest key
    assert pc.reference_matches(R, S[:0]) == 0
    brute = sum(int(r == s) for r, s in itertools.product(R.tolist(), S.tolist()))
    assert brute == 9


def test_expected_plan_by_hand():
    """bits 16, partition 3: 70000 R tuples (beyond the counters: blocks) against 2^16 + 1 S tuples (2 items); partition 4:
    30000 R tuples (counters) against 2^16 S tuples (1 item); partition 5: S only; partition 6: R only."""
    P = 1 << 16
    R = np.concatenate([np.full(70000, 3 + P), np.full(30000, 4 + 7 * P), np.full(9, 6)]).astype(np.uint64)
    S = np.concatenate([np.full(pc.ITEM_S + 1, 3), np.full(pc.ITEM_S, 4), np.full(200000, 5 + P)]).astype(np.uint64)
    plan = pc.expected_plan(R, S, 16)
    assert (plan["items"], plan["splitPartitions"], plan["maxSPartition"]) == (3, 1, 200000)
    assert dict(plan["cells"]) == {("blocks", True): 2, ("direct", False): 1}
    plan14 = pc.expected_plan(R, S, 14)                      # no counters below 16 bits: 30000 > 24576 is blocks as well
    assert dict(plan14["cells"]) == {("blocks", True): 2, ("blocks", False): 1}
    small = pc.expected_plan(R[:70000:4], S, 14)             # 17500 R tuples of partition 3 alone
    assert dict(small["cells"]) == {("hashed", True): 2} and small["items"] == 2


def test_frag_tail_case_asserts_its_geometry():
    """the fragments of the frag-tail case hold more keys than the join's register prefetch covers (cap2 > 1024 * 16 / C2);
    a change of the fragment geometry that ends this fails here instead of emptying the case"""
    tails = [c for c in pc.CASES if c.must_tail]
    assert tails and any(c.one_shot for c in tails)
    for c in tails:
        for n in c.must_tail:
            g = pc.planned(n, c.bits, c.mode)
            assert g.planned and g.cap2 > 1024 * 16 // g.C2 and g.tail, (c, n, g)
            assert g.C2 == 16, (c, n, g)                     # one prefetch slot per fragment (spfShift = 0)
        if c.one_shot:                                       # R and the first slice: planned in the one-shot join too
            steps = c.steps()
            assert [s.op for s in steps[:2]] == ["build", "probe"] and steps[1].arr.size in c.must_tail
            assert pc.one_shot_planned(steps[0].arr.size, steps[1].arr.size, c.bits, c.mode), c
            assert not pc.one_shot_planned(steps[0].arr.size, sum(s.arr.size for s in steps[1:]), c.bits, c.mode)
    assert not pc.planned(1 << 23, 14, 2).tail               # what every smaller test of the suite runs


def test_workspace_regrow_case_outgrows_its_reservation():
    """R is not planned, so hj_reserve's workspace holds no fragment counters; its histogram scratch is the first slice's
    own (hj_prj_workspace_info, which plans no fragments at these sizes: equal for (R, slice) and (slice, slice)); the
    slice is planned, so its probe needs that scratch plus the counters -- more than was reserved."""
    case = next(c for c in pc.CASES if c.name == "workspace-regrow")
    steps = case.steps()
    n_r, n_s = pc.reserve_sizes(steps)
    assert [s.op for s in steps[:2]] == ["build", "probe"] and steps[1].arr.size == n_s and pc.RESERVE in steps[2:-1]
    assert not pc.planned(n_r, case.bits, case.mode).planned and pc.planned(n_s, case.bits, case.mode).planned
    assert not pc.one_shot_planned(n_r, n_s, case.bits, case.mode)
    reserved, slice_scratch = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    assert hj.lib.hj_prj_workspace_info(n_r, n_s, case.bits, reserved) == 0
    assert hj.lib.hj_prj_workspace_info(n_s, n_s, case.bits, slice_scratch) == 0
    assert reserved[0] == slice_scratch[0] > 0


def test_planned_follows_the_mode():
    assert not pc.planned(1 << 23, 14, 1).planned            # exact passes asked for
    assert not pc.planned(1 << 23, 14, 0).planned            # the size rule: nothing below 2^25
    assert pc.planned(1 << 25, 14, 0).planned
    assert pc.planned(1 << 23, 14, 2)[:2] == (True, 2)
    assert not pc.planned(1 << 20, 8, 2).planned             # a single pass has no fragments


@pytest.mark.slow
def test_every_join_mode_with_and_without_a_split_s_partition(survey):
    for mode in ("direct", "hashed", "blocks"):
        for split in (False, True):
            assert survey["cells"].get((mode, split)), (mode, split, sorted(survey["cells"]))


@pytest.mark.slow
def test_every_fragment_count_and_an_unplanned_r(survey):
    for c2 in (1, 2, 4, 8, 16):
        assert survey["r_c2"].get(c2), (c2, survey["r_c2"])
    assert survey["r_unplanned"]
    assert survey["r_tail"] and survey["s_tail"], (survey["r_tail"], survey["s_tail"])
    assert survey["no_items"]
    # R and slices on each of the three paths (0 exact, 1 histogram-free, 2 fell back)
    for side in "rs":
        for path in (0, 1, 2):
            assert (side, (path,)) in survey["paths"], (side, path, survey["paths"])


@pytest.mark.slow
def test_boundary_cases_hold_every_boundary_size(survey):
    assert sorted(survey["boundary"]) == ["boundaries-b14", "boundaries-b16"]
    for name, (sizes, items, plan) in survey["boundary"].items():
        assert tuple(sizes) == pc.BOUNDARY_SIZES, (name, sizes)
        assert tuple(items) == pc.BOUNDARY_ITEMS, (name, items)
        assert plan["splitPartitions"] == 3 and plan["maxSPartition"] == 2 * pc.ITEM_S + 1, name


@pytest.mark.slow
def test_reference_matches_agrees_with_the_oracle_cardinality(survey):
    """two independent references (numpy's sort-based counts, the oracle's C hash join), neither the code under test"""
    assert len({name for name, *_ in survey["cross"]}) >= 12
    for name, k, mine, theirs in survey["cross"]:
        assert mine == theirs, (name, k, mine, theirs)
    assert any(mine == 0 for *_, mine, _ in survey["cross"]) and any(mine > 1 << 20 for *_, mine, _ in survey["cross"])


def test_random_cases_add_planned_and_unplanned_relations(monkeypatch):
    """With the default HJ_FUZZ_CASES the generator reaches R relations with and without the histogram-free layout in
    mode 2. Mode 1 never plans it, and mode 0 plans nothing below 2^25 tuples, far above the generator's sizes: in
    those modes every random relation takes the exact passes, which is all there is to say about them here."""
    monkeypatch.delenv("HJ_FUZZ_CASES", raising=False)
    assert pc.fuzz_case_count() == 36
    r_plan, s_plan, names, bits_seen, shapes = {0: set(), 1: set(), 2: set()}, set(), [], set(), set()
    for block in range(pc.FUZZ_BLOCKS):
        for index in range(block, pc.fuzz_case_count(), pc.FUZZ_BLOCKS):
            R, S, lens, bits, shape = pc.random_relations(block, index)
            assert sum(lens) == S.size and min(lens) >= 1 and 1 <= len(lens) <= 7
            assert (1 << 10) <= R.size < (1 << 21) and int(R.max()) < 1 << 32 and int(R.min()) >= 1
            names.append((block, index)); bits_seen.add(bits); shapes.add(shape)
            for mode in (0, 1, 2):
                r_plan[mode].add(pc.planned(R.size, bits if bits else 14, mode).planned)
                s_plan |= {(mode, pc.planned(m, bits if bits else 14, mode).planned) for m in lens}
    assert len(names) == 36 and len(set(names)) == 36
    assert r_plan[2] == {False, True}, r_plan
    assert r_plan[0] == {False} and r_plan[1] == {False}
    assert (2, True) in s_plan and (2, False) in s_plan
    assert shapes == set(pc.FUZZ_SHAPES) and len(bits_seen) >= 6, (shapes, bits_seen)
    first = [c.name for c in itertools.islice(pc.random_cases(0), 3)]
    assert first == [c.name for c in itertools.islice(pc.random_cases(0), 3)] and first[0].endswith("-m0")      # seeded
