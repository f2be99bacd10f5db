"""What test_gpu_htm_chains.py and the full-size case of test_gpu_fullsize.py do with a relation on the device: build it
through a HashJoinContext, evaluate chain_plan (htm_chain_cases.py) on the device's own seams, compare state, cause and
hj_result.compactFallback bit 8 with the plan and the whole table with the sequential oracle. No test in here."""
import numpy as np

import htm_chain_cases as cc
from gpu_harness import alloc
from oracle import oracle


def assert_table_is_the_oracles(c, got, want, tag, bucket_range=None):
    """the counters test_htm_bucket_table_matches_sequential_oracle checks, the primary buckets, every chain in walk order
    (bucket_range = (lo, hi): the chains of those buckets only, everything else in full)"""
    assert got["algoUsed"] == "htm" and got["htmBuckets"] == want["numBuckets"], tag
    assert (got["conflicts"], got["conflictSum"], got["totalMatches"], got["inputSum"], got["tableSumFull"],
            got["htmOverflowBuckets"], got["htmOverflowSum"], got["outputSum"]) == (
        want["conflictCount"], want["conflictSum"], want["totalMatches"], want["inputSum"], want["bucketSum"],
        want["overflowBuckets"], want["overflowSum"], want["outputSum"]), tag
    buckets, overflows = c.export_buckets(want["numBuckets"])
    assert np.array_equal(buckets["tuples"], want["buckets"]["tuples"]) and np.array_equal(buckets["count"], want["buckets"]["count"]), tag
    assert np.array_equal(buckets["nextIndex"] != 0, want["buckets"]["nextIndex"] != 0), tag
    assert overflows.size == want["overflows"].size, tag
    wb = want["buckets"]
    if bucket_range is not None:
        lo, hi = bucket_range
        buckets, wb = buckets[lo:hi], wb[lo:hi]
    a, ao = cc.chains_view(buckets, overflows)
    b, bo = cc.chains_view(wb, want["overflows"])
    assert np.array_equal(ao, bo) and np.array_equal(a, b), tag


def run_relation(c, R, tag, want=None, variant=3, bucket_range=None):
    """R through hj_reserve / hj_build_dev / hj_probe_dev on context c; the plan on the device's seams; state, cause and
    bit 8 against it; the table against the oracle. Returns (plan, chain info, result)."""
    n = R.size
    S = cc.probe_side(R)
    if want is None:
        want = oracle.htm_build_probe_seq(R, S, want_buckets=True)
    dR, dS = alloc(c, n * 8), alloc(c, S.size * 8)
    try:
        c.copy_h2d(dR, R); c.copy_h2d(dS, S)
        c.reserve("htm", n, S.size, buildVariant=variant)
        c.build(dR, n)
        c.probe(dS, S.size)
        c.checksums()
        got = c.fetch()
        info = c.htm_chain_info()
        lay, cl = c.wave_layout_info(n), c.htm_chain_layout_info(n)
        assert cl["tries"] == cc.tries_rule(n, lay, cl), tag
        # a request for the rings runs the rings exactly where the layout says the phase is tried (a smaller table: 2 or 1)
        ran = got["buildVariant"]
        assert (ran == variant) if (variant != 3 or cl["tries"]) else (ran in (1, 2)), (tag, ran)
        plan = None
        if ran == 3:
            starts, bounds, _ = c.wave_seams()
            es, eb = cc.seams(R, lay)
            assert np.array_equal(starts, es) and np.array_equal(bounds, eb), tag
            plan = cc.chain_plan(R, lay, cl, bounds)
            print(tag, "plan mask", plan.mask, "device", info, "compactFallback", hex(got["compactFallback"]))
            assert plan.strays == 0, tag
            if plan.mask == 0:
                assert info == {"state": cc.HELD, "cause": 0, "groups": plan.total_groups}, (tag, info)
            else:
                assert info["state"] == cc.HANDED_OVER and info["cause"] != 0 and info["cause"] & ~plan.mask == 0, (tag, info, plan.mask)
        else:
            assert info == {"state": 0, "cause": 0, "groups": 0}, tag
        assert (got["compactFallback"] & 0x100 != 0) == (info["state"] == cc.HANDED_OVER), (tag, got["compactFallback"], info)
        assert got["totalMatches"] == n == want["totalMatches"], tag                       # every tuple stored once, every key asked for once
        assert_table_is_the_oracles(c, got, want, tag, bucket_range)
        return plan, info, got
    finally:
        c.dev_free(dR); c.dev_free(dS)


def run_case(c, case, n, bucket_range=None):
    lay, cl = c.wave_layout_info(n), c.htm_chain_layout_info(n)
    R, what, cpu_plan = cc.build_case(case, n, lay, cl)                   # the case's property, on this device's geometry
    if bucket_range is not None:
        bucket_range = bucket_range(what)
    plan, info, got = run_relation(c, R, case.name, bucket_range=bucket_range)
    assert plan.mask == cpu_plan.mask and np.array_equal(plan.m, cpu_plan.m), case.name
    assert info["state"] == case.state, (case.name, info)
    if case.state == cc.HANDED_OVER:
        assert info["cause"] & case.bit, (case.name, info)
    return plan, info, got
