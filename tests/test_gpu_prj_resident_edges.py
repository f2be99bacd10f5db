"""Differential tests of the resident-R radix join (hj_prj_build_dev / hj_prj_probe_dev: k_prj_items_count,
k_prj_items_fill, k_prj_probe_items) on the case table of tests/prj_cases.py and on seeded random relations.

After every build: counters reset, R's checksum (oracle.prj_join(R, None, bits)), the predicted path. After EVERY probe:
the increase of totalMatches against the numpy reference of that slice alone (two slices that lose and double count
cannot cancel), the running sSize, and hj_prj_resident_info's work items, split partitions and largest S partition
exactly as the two partition histograms give them. At the end the total against the reference of the concatenated
slices and, where affordable, against the oracle's radix join. HJ_FUZZ_CASES (default 36) sets the number of random
cases, as in test_gpu_fuzz.py; the seeds are fixed.

What the table is there to catch, each tried once as a one-line change of hj_prj.hip (counts only, no address moves):
the loop behind the register prefetch skipped for fragments (frag-tail-b9, at the build's checksum for k_prj_join and at
the first probe for k_prj_probe_items); an item of a split partition one tuple short (every case with a split S
partition); the loop over the LDS blocks of an oversized R partition ended after its first block (the blocks-* cases,
direct-kernel-blocks, narrow-b4, mixed-paths-r-fallback, rebuild); a work item too many for an S partition of a whole
multiple of 2^16 tuples (boundaries-*: nothing but hj_prj_resident_info's numbers shows it, the matches stay right)."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
import prj_cases as pc
from oracle import oracle

from gpu_harness import alloc

pytestmark = pytest.mark.gpu


def run_case(c, case):
    """the steps of one case on context c; every assertion carries the case, bits, mode, step and the info dict"""
    steps = case.steps()
    n_r, n_s = pc.reserve_sizes(steps)
    bits = pc.resolved_bits(n_r, case.bits)
    kw = dict(radixBits=case.bits, prjMode=case.mode)
    c.reserve("prj", n_r, n_s, **kw)
    dR, dS = alloc(c, n_r * 8), alloc(c, n_s * 8)
    R = r_counts = checksum = r_path = None
    total = s_sum = b = 0                                       # b: step of the current build
    slices = []

    def end_of_build():
        """the running total of the build that ends here, against the references of all its slices at once"""
        if R is None or not slices:
            return
        S = np.concatenate(slices)
        tag = (case.name, bits, case.mode, "total")
        assert total == case.once((b, "total"), lambda: pc.reference_matches(R, S, r_counts)), tag
        if case.oracle_total:
            want = case.once((b, "oracle"), lambda: oracle.prj_join(R, S, bits))
            assert (total, checksum) == (want["matches"], want["checksum"]), (tag, want)

    for k, st in enumerate(steps):
        tag = (case.name, bits, case.mode, k, st.op)
        if st.op == "build":
            end_of_build()
            R, slices, total, s_sum, b = st.arr, [], 0, 0, k
            r_counts = case.once((k, "counts"), lambda: pc.key_counts(st.arr))
            checksum = case.once((k, "checksum"), lambda: oracle.prj_join(st.arr, None, bits)["checksum"])
            c.copy_h2d(dR, R)
            c.prj_build(dR, R.size)
            got = c.fetch()
            assert (got["totalMatches"], got["sSize"], got["rSize"]) == (0, 0, R.size), (tag, got)
            assert (got["radixBits"], got["prjPartitions"]) == (bits, 1 << bits), (tag, got)
            assert got["prjChecksum"] == checksum, (tag, got["prjChecksum"], checksum)
            assert got["prjPath"] in st.paths, (tag, got["prjPath"], sorted(st.paths))
            assert (got["prjPath"] != 0) == pc.planned(R.size, bits, case.mode).planned, (tag, got["prjPath"])
            r_path = got["prjPath"]
            continue
        if st.op == "reserve":
            c.reserve("prj", n_r, n_s, **kw)                   # reallocates nothing: R stays resident
            continue
        if st.op == "empty":
            c.prj_probe(dS, 0)
            want_inc, S = 0, None
        else:
            S = st.arr
            c.copy_h2d(dS, S)
            c.prj_probe(dS, S.size)
            want_inc = case.once((k, "matches"), lambda: pc.reference_matches(R, S, r_counts))
            slices.append(S)
            s_sum += S.size
        got = c.fetch()
        info = c.prj_resident_info()
        print(case.name, k, st.op, "matches +", got["totalMatches"] - total, "want +", want_inc, info)
        assert got["totalMatches"] - total == want_inc, (tag, got["totalMatches"] - total, want_inc, info)
        total = got["totalMatches"]
        assert (got["sSize"], got["rSize"]) == (s_sum, R.size), (tag, got["sSize"], s_sum, info)
        assert got["prjChecksum"] == checksum, (tag, got["prjChecksum"], checksum, info)
        assert got["prjPath"] == r_path and info["rPath"] == r_path, (tag, got["prjPath"], r_path, info)
        again = c.fetch()                                       # reading the result twice changes nothing
        assert (again["totalMatches"], again["sSize"], again["prjChecksum"]) == (total, s_sum, checksum), (tag, again, info)
        if S is not None:
            plan = case.once((k, "plan"), lambda: pc.expected_plan(R, S, bits))
            want_info = (plan["items"], plan["splitPartitions"], plan["maxSPartition"])
            assert (info["items"], info["splitPartitions"], info["maxSPartition"]) == want_info, (tag, want_info, info)
            assert info["sPath"] in st.paths, (tag, sorted(st.paths), info)
            assert (info["sPath"] != 0) == pc.planned(S.size, bits, case.mode).planned, (tag, info)
    end_of_build()
    c.dev_free(dR); c.dev_free(dS)
    return R, slices, bits, total, checksum


@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_case(case):
    for n in case.must_tail:                                    # the case keeps reaching the loop behind the register prefetch
        g = pc.planned(n, case.bits, case.mode)
        assert g.planned and g.cap2 > 1024 * 16 // g.C2, (case, n, g)
    with hj.HashJoinContext(0) as c:
        R, slices, bits, total, checksum = run_case(c, case)
    if case.one_shot:
        # R and the first slice through the one-shot join: k_prj_join's own walk over fragments with a tail, on both sides
        # (all slices at once would be too large an S for the histogram-free passes, and the join would not be planned)
        S = slices[0]
        assert pc.planned(S.size, bits, case.mode).tail and pc.one_shot_planned(R.size, S.size, bits, case.mode), case
        with hj.HashJoinContext(0) as c:
            got = c.run("prj", R, S, radixBits=case.bits, prjMode=case.mode)
        want = case.once((1, "matches"), lambda: pc.reference_matches(R, S))
        tag = (case.name, bits, case.mode, "one-shot", got["prjPath"])
        assert got["prjPath"] == 1, tag
        assert (got["totalMatches"], got["prjChecksum"], got["sSize"]) == (want, checksum, S.size), (tag, got, want)


@pytest.mark.parametrize("block", range(pc.FUZZ_BLOCKS))
def test_resident_radix_join_on_random_relations(block):
    """|R| of any size in [2^10, 2^21), 1..7 ragged slices, dense / 31-bit / constant low bits / constant middle bits /
    repeated keys, radix widths from one pass of 4 bits to 16 and the engine's pick, modes 0, 1 and 2 -- one context
    per block, so that every case also builds over what the previous one left resident."""
    ran = 0
    with hj.HashJoinContext(0) as c:
        for case in pc.random_cases(block):
            run_case(c, case)
            ran += 1
    assert ran == 3 * len(range(block, pc.fuzz_case_count(), pc.FUZZ_BLOCKS))
