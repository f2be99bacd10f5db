"""The workgroup-window build (buildVariant 2: k_build_own, k_finalize_range, k_clear_unowned, k_build_deferred) on the
directed cases of own_cases.py: every cause of a deferral on purpose. tests/test_own_cases.py has shown on the CPU that
own_plan, the restatement of phase A, gives the sequential oracle's table on every case and that every case sits where it
says. Here, for every case: the table slot for slot and every counter are the oracle's; the owner table, the per-chunk
deferred counts and the valid slot range are the plan's -- evaluated for the claims the device's own owner table shows
where a block was contested. No tolerance anywhere. Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from gpu_harness import alloc, ctx  # noqa: F401
import own_cases as oc
from htm_chain_device import assert_table_is_the_oracles
from oracle import oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum")


@pytest.fixture(scope="module")
def cu(ctx):
    return ctx.own_layout_info(oc.N1)["computeUnits"]


_WANT = {}


def want_of(case):
    """the sequential oracle's answer for a case and its probe side, computed once"""
    if case.name not in _WANT:
        S = oc.probe_side(case.rel)
        if case.htm:
            _WANT[case.name] = oracle.htm_build_probe_seq(case.rel, S, want_buckets=True)
        else:
            _WANT[case.name] = oracle.build_probe_seq_ts(case.rel, S, case.table_size, case.shift, case.probe, want_table=True)
    return _WANT[case.name]


def device_run(c, case, variant, keys32=None, reserve=True):
    """one build + probe of the case on context c -> hj_result as a dict"""
    keys32 = case.keys32 if keys32 is None else keys32
    S = oc.probe_side(case.rel)
    n = case.n
    width = 4 if keys32 else 8
    dR, dS = alloc(c, width * n + 16), alloc(c, width * S.size + 16)
    try:
        c.copy_h2d(dR, case.rel.astype(np.uint32) if keys32 else case.rel)
        c.copy_h2d(dS, S.astype(np.uint32) if keys32 else S)
        if case.htm:
            if reserve:
                c.reserve("htm", n, S.size, buildVariant=variant)
            c.build(dR, n, case.idx_base)
            c.probe(dS, S.size)
        elif keys32:
            if reserve:
                c.reserve("atomic", case.table_size // 2, S.size, probeLength=case.probe, buildVariant=variant)
            c.build_keys(dR, n, case.shift, case.table_size)
            c.probe_keys(dS, S.size)
        else:
            assert case.table_size == 2 * n and case.shift == 0
            if reserve:
                c.reserve("atomic", n, S.size, probeLength=case.probe, buildVariant=variant)
            c.build(dR, n, case.idx_base)
            c.probe(dS, S.size)
        c.checksums()
        return c.fetch()
    finally:
        c.dev_free(dR)
        c.dev_free(dS)


def check_exact(c, case, got, tag):
    want = want_of(case)
    if case.htm:
        assert_table_is_the_oracles(c, got, want, tag)
        return
    for k in COUNTERS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert got["outputSum"] == want["outputSumAtomic"], tag
    assert np.array_equal(c.export_table(case.table_size), want["table"]), tag


def check_window_build(c, case, got, cu, tag):
    """what the window build left against the plan: owner table, per-chunk deferred counts, valid range"""
    plan = oc.plan_of(case, cu)
    assert got["buildVariant"] == 2, tag
    owner, counts, total = c.own_info()
    assert owner.size == plan.geo["numBlocks"] and counts.size == plan.n_chunks, tag
    assert got["buildDeferred"] == total == int(counts.sum()), (tag, got["buildDeferred"], total)
    bounds = [plan.bounds(k) for k in range(plan.n_chunks)]
    print(f"{case.name}: plan's deferred per chunk {bounds}, device {counts.tolist()}")
    # owner table: an uncontested wanted block is its chunk's, a contested one one of its wanters', every other block nobody's
    for b in range(owner.size):
        w = plan.wanters.get(b, [])
        assert (int(owner[b]) - 1 in w) if w else owner[b] == 0, (tag, "owner", b, int(owner[b]), w)
    for k, (lo, hi) in enumerate(bounds):
        assert lo <= counts[k] <= hi, (tag, "deferred", k, int(counts[k]), (lo, hi))
    # given who won the contested claims, phase A is determined: counts and valid range exactly
    outs = plan.assignment_from(owner)
    assert [len(o.deferred) for o in outs] == counts.tolist(), (tag, "deferred for the device's claims")
    assert np.array_equal(plan.owner_table(outs), owner), tag
    dbg = c.table_debug()
    assert (dbg["validLo"], dbg["validHiEx"]) == plan.valid_range(outs), (tag, dbg, plan.valid_range(outs))
    assert dbg["tableSlots"] == case.table_size and dbg["tableFormat"] == 0, tag


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name)
def test_directed_cases(ctx, cu, case):
    """every case under buildVariant 2 against oracle and plan, then under 0, 1 and 3 for exactness alone"""
    got = device_run(ctx, case, 2)
    check_exact(ctx, case, got, (case.name, 2))
    check_window_build(ctx, case, got, cu, case.name)
    for variant in (0, 1, 3):
        got = device_run(ctx, case, variant)
        check_exact(ctx, case, got, (case.name, variant))


@pytest.mark.parametrize("inst", ("tuples", "keys", "tuples_check", "keys_check", "htm"))
def test_every_instantiation(cu, inst):
    """k_build_own<KEY32, CHECK, HTM> as the launcher can instantiate it: tuples or bare keys, with and without the shard
    check, and the bucketised table -- each on a case that defers nothing beyond its base and on one that defers"""
    G, shard = 4, 1
    foreign = lambda A: int(((A & np.uint64(G - 1)) != shard).sum())                      # noqa: E731
    names = ("htm_base", "htm_deferred_conflicts") if inst == "htm" else ("ahead_in", "behind_out_advanced")
    with hj.HashJoinContext(0) as c:
        for name in names:
            case = oc.BY_NAME[name]
            if inst.endswith("check"):
                c.set_shard_check(G, 0, shard)
            got = device_run(c, case, 2, keys32=inst.startswith("keys"))
            check_exact(c, case, got, (inst, name))
            check_window_build(c, case, got, cu, (inst, name))
            assert got["foreignTuples"] == (foreign(case.rel) + foreign(oc.probe_side(case.rel)) if inst.endswith("check") else 0)
            c.set_shard_check(0)


def test_context_reused_across_defer_heavy_none_defer_heavy(cu):
    """one reserved context, five builds (defer-heavy, none, everything deferred, none, defer-heavy): each step's owner
    table, counts and valid range are its own -- no stale owner word, no stale queue entry"""
    steps = [oc.BY_NAME[k] for k in ("behind_out_advanced", "ahead_in", "defer_all_small", "quarter_at_last", "behind_out_first")]
    with hj.HashJoinContext(0) as c:
        c.reserve("atomic", oc.N1, oc.probe_side(steps[0].rel).size, buildVariant=2)
        seen = []
        for case in steps:
            got = device_run(c, case, 2, reserve=False)
            check_exact(c, case, got, ("reuse", case.name))
            check_window_build(c, case, got, cu, ("reuse", case.name))
            seen.append(got["buildDeferred"])
        assert seen[1] == 0 and seen[3] == 0 and min(seen[0], seen[2], seen[4]) > 1000, seen


def test_key_range_in_a_first_tile(ctx, cu):
    """a tuple with key 0 or payload bits in a chunk's first tile: HJ_ERR_KEY_RANGE, and the next valid build on the context is
    exact. A first tile with no valid tuple at all (the window is placed by the second tile) gives the same."""
    case = oc.BY_NAME["contested_seam_idx_base"]
    lay = oc.layout(case.n, cu)
    S = oc.probe_side(case.rel)
    bads = []
    for pos in (0, 5, lay["chunkLen"], lay["chunkLen"] + lay["tileTuples"] - 1):
        for value in (np.uint64(0), case.rel[pos] | (np.uint64(1) << np.uint64(40))):
            bad = case.rel.copy()
            bad[pos] = value
            bads.append(bad)
    for a in (0, lay["chunkLen"]):
        bad = case.rel.copy()
        bad[a:a + lay["tileTuples"]] = 0
        bads.append(bad)
    for bad in bads:
        with pytest.raises(hj.HashJoinError) as e:
            ctx.run("atomic", bad, S, buildVariant=2)
        assert e.value.status == _lib.HJ_ERR_KEY_RANGE
    got = device_run(ctx, case, 2)
    check_exact(ctx, case, got, "after the key range errors")
    check_window_build(ctx, case, got, cu, "after the key range errors")


@pytest.mark.parametrize("copies,probe", ((1, 4), (2, 1)))
def test_defer_all_where_phase_b_loops_over_its_slices(ctx, copies, probe):
    """a descending relation of 2^22 tuples, the smallest size at which a workgroup of phase B walks its slice more than
    once (three to four times): everything below each chunk's first window is deferred. With every key twice at
    probeLength 1, half of the deferred tuples run out of budget in phase B. Table and counters; the counts add up and are
    the closed form's"""
    n = 1 << 22
    lay = ctx.own_layout_info(n)
    assert lay["chunkLen"] >= 4 * lay["deferredParts"] * 256
    rel = oc.defer_all(n, copies)
    S = rel[::5].copy()
    want = oracle.build_probe_seq_ts(rel, S, 2 * n, 0, probe, want_table=True)
    assert want["conflicts"] == (n // 2 if copies == 2 else 0)
    got = ctx.run("atomic", rel, S, probeLength=probe, buildVariant=2)
    for k in COUNTERS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["buildVariant"] == 2 and got["outputSum"] == want["outputSumAtomic"]
    assert np.array_equal(ctx.export_table(2 * n), want["table"])
    owner, counts, total = ctx.own_info()
    assert total == got["buildDeferred"] == int(counts.sum())
    expect = oc.defer_all_counts(rel, lay, 2 * n)
    assert counts.tolist() == expect and min(expect) > 2 * lay["deferredParts"] * 256            # more than two passes per slice


def test_own_info_needs_the_window_build(ctx):
    """hj_own_info: HJ_ERR_STATE before any build, after buildVariant 1, 3 and 4, after a radix join, after buildVariant 0
    picked another build and once hj_reserve has replaced the owner table; the data after buildVariant 0 picked the
    window, on open addressing and on the bucketised table"""
    def refused(c):
        with pytest.raises(hj.HashJoinError) as e:
            c.own_info()
        return e.value.status == _lib.HJ_ERR_STATE

    case = oc.BY_NAME["ahead_out"]
    with hj.HashJoinContext(0) as fresh:
        assert refused(fresh)
        assert fresh.own_layout_info(oc.N4) == oc.layout(oc.N4, fresh.own_layout_info(oc.N4)["computeUnits"])
        got = device_run(fresh, case, 2)
        assert fresh.own_info()[2] == got["buildDeferred"] == 1
        # short capacities: HJ_ERR_INVALID, and the sizes needed are reported
        buf, out = np.zeros(8, dtype=np.uint32), (ctypes.c_uint64 * 4)()
        h = fresh._h
        assert hj.lib.hj_own_info(h, buf.ctypes.data, 8, buf.ctypes.data, 8, out) == _lib.HJ_ERR_INVALID
        assert (out[0], out[1]) == (case.table_size // 512, 1)
        assert hj.lib.hj_own_info(h, None, 0, buf.ctypes.data, 8, out) == _lib.HJ_ERR_INVALID
        assert hj.lib.hj_own_info(h, buf.ctypes.data, 8, buf.ctypes.data, 8, None) == _lib.HJ_ERR_INVALID
        fresh.reserve("atomic", 1 << 20, 16, buildVariant=2)            # a larger owner table: the old words are gone
        assert refused(fresh)
    for variant in (1, 3, 4):
        assert device_run(ctx, case, variant)["buildVariant"] in ((variant,) if variant != 4 else (3, 4))     # 4 may hand over to 3
        assert refused(ctx)
    assert device_run(ctx, case, 2)["buildVariant"] == 2
    assert ctx.own_info()[2] == 1
    ctx.run("prj", case.rel, oc.probe_side(case.rel), radixBits=8)
    assert refused(ctx)
    # the pre-round picks: loose locality -> the window; a random permutation -> global atomics
    n = 1 << 20
    loose, shuffled = oracle.generate_data("local_shuffle", n, n, 1024), oracle.generate_data("shuffle", n, n, 16)
    with hj.HashJoinContext(0) as fresh:
        got = fresh.run("atomic", loose, None)
        assert got["buildVariant"] == 2
        owner, counts, total = fresh.own_info()
        assert total == got["buildDeferred"] == int(counts.sum()) and owner.size == 2 * n // 512 and owner.max() <= counts.size
    with hj.HashJoinContext(0) as fresh:
        assert fresh.run("atomic", shuffled, None)["buildVariant"] == 1
        assert refused(fresh)
    n = 1 << 16
    with hj.HashJoinContext(0) as fresh:
        got = fresh.run("htm", oracle.generate_data("local_shuffle", n, n, 1024), None)
        assert got["buildVariant"] == 2
        assert fresh.own_info()[2] == got["buildDeferred"]
