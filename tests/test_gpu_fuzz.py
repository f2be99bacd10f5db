"""Randomised differential test of the open-addressing builds against the sequential oracle: inputs the DataGen
distributions do not produce -- near-sorted multisets with bursts of equal keys, key domains from a quarter of the
relation (most tuples are dropped) to the whole table (sparse keys, wrap-around at the table's end), disorder from none
to far beyond what the rings hold, every probe length -- through the device's pick (0), the workgroup window (2), the
classic rings (3) and the compact rings (4; where they cannot hold they must hand over, and the table must still be the sequential one).
Counters and the whole table, slot for slot. The classic rings run again on a context that keeps row ids (the packed
build), and the slot-code road -- one code byte per slot, 4-byte ring words -- has random relations of its own with key
bits above the table size: forced onto small tables, and once by the size rule at 2^25 slots. HJ_FUZZ_CASES (default 36) sets the number of cases; the seed is fixed."""
import os

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import Device, alloc
import htm_chain_cases as cc
from fuzz_relations import make_relation, slot_code_case
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("block", range(4))
def test_ring_builds_on_random_near_sorted_relations(block):
    cases = int(os.environ.get("HJ_FUZZ_CASES", "36"))
    rng = np.random.default_rng(20260000 + block)
    with hj.HashJoinContext(0) as ctx:
        for case in range(block, cases, 4):
            n = 1 << int(rng.integers(12, 21))
            R, w = make_relation(rng, n)
            plen = int(rng.choice([1, 2, 3, 4, 4, 4, 5, 8]))
            S = np.ascontiguousarray(rng.permutation(R)[: n]) if rng.integers(0, 2) else np.arange(1, n + 1, dtype=np.uint64)
            want = oracle.build_probe_seq(R, S, plen, want_table=True)
            for variant in (0, 2, 3, 4):
                got = ctx.run("atomic", R, S, probeLength=plen, buildVariant=variant)
                tag = (block, case, n, w, plen, variant, got["buildVariant"], got["compactFallback"])
                for k in ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum"):
                    assert got[k] == want[k], (k, got[k], want[k], tag)
                assert np.array_equal(ctx.export_table(2 * n), want["table"]), tag
                if variant == 4 and got["buildVariant"] == 3:
                    assert got["compactFallback"] != 0, tag              # a hand-over always says why
                if variant == 3:
                    assert got["buildVariant"] == 3 and got["compactFallback"] == 0, tag
            # the classic rings once more on a context that keeps row ids: the packed build, the table probe_pairs reads
            got = ctx.run("atomic", R, S, probeLength=plen, buildVariant=3, keepRowIds=True)
            tag = (block, case, n, w, plen, "keepRowIds", got["buildVariant"], got["compactFallback"])
            for k in ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum"):
                assert got[k] == want[k], (k, got[k], want[k], tag)
            assert np.array_equal(ctx.export_table(2 * n), want["table"]), tag
            assert got["buildVariant"] == 3 and got["compactFallback"] == 0, tag


COUNTERS = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum")
LOG_OVERFLOW, CODE_OVERFLOW = 1, 4                       # slot_codes_info()["cause"]


def build_probe_codes(c, R, S, plen, variant, slot_codes, idx_base=0):
    """one build + probe + checksums through the split API (test_gpu_slot_codes.build_probe) -> (result, table, info)"""
    c.reserve("atomic", R.size, S.size, probeLength=plen, buildVariant=variant, slotCodes=slot_codes)
    with Device(c) as dev:
        c.build(dev.put(R), R.size, idx_base)
        c.probe(dev.put(S), S.size)
        c.checksums()
        got = c.fetch()
        return got, c.export_table(2 * R.size), c.slot_codes_info()


def check_road(got, table, info, want, road, uncodable, tag):
    """the oracle's result whatever the road; on the rings, what slot_codes_info says about the road against what the
    host knows. -> whether the build stayed on the slot-code road"""
    for k in COUNTERS:
        assert got[k] == want[k], (k, got[k], want[k], tag)
    assert got["outputSum"] == want["outputSumAtomic"], tag
    assert np.array_equal(table, want["table"]), tag
    if got["buildVariant"] != 3:
        return False                                         # the device's pick was another build: nothing about the road
    assert info["road"] == road, tag
    assert bool(info["cause"] & CODE_OVERFLOW) == uncodable, tag
    assert info["cause"] & ~(LOG_OVERFLOW | CODE_OVERFLOW) == 0, tag
    if info["cause"] == 0:
        assert (info["codes"], info["tableFormat"]) == (True, 2), tag
    else:                                                    # a hand-over says so: the 8-byte build redid the table
        assert (info["codes"], info["tableFormat"]) == (False, 0), tag
    return info["cause"] == 0


@pytest.mark.parametrize("block", range(4))
def test_slot_code_road_on_random_near_sorted_relations(block):
    """The road production takes, k_build_wave<PLANAR, CODES>, forced onto small tables (slotCodes=True) through the classic
    rings (3) and the device's pick (0): 1 to 512 chunks, every probe length with its own displacement bits, keys with
    high parts above the table (fuzz_relations.make_relation(high=True)) so that codes, ring words and decoded keys carry
    them, idxBase 0 and near 2^32, S asking for every high-part variant of some home slots. Counters, outputSum and the
    whole table against the sequential oracle; then the road: cause 4 exactly when R holds a key without a code (the host
    knows: keyLimit = hiCap << tableBits), a hand-over for the dirty log (cause 1) permitted but reported, and otherwise
    (codes, road, tableFormat) == (True, 2, 2). At least half of the cases without an uncodable key must have stayed on the
    road (test_fuzz_tables.py shows from the drawn W that the seeds allow it)."""
    cases = int(os.environ.get("HJ_FUZZ_CASES", "36"))
    rng = np.random.default_rng(20265000 + block)
    stayed = codable = 0
    with hj.HashJoinContext(0) as ctx:
        for case in range(block, cases, 4):
            n, plen, idx_base, R, S, w, hi = slot_code_case(rng)
            lay = ctx.wave_layout_info(n)
            uncodable = bool((R >= np.uint64(hi["keyLimit"])).any())
            assert uncodable == (hi["over"] > 0)
            want = oracle.build_probe_seq(R, S, plen, want_table=True)
            for variant in (3, 0):
                got, table, info = build_probe_codes(ctx, R, S, plen, variant, True, idx_base)
                tag = (block, case, n, w, plen, idx_base, hi["mode"], hi["over"], lay["nChunks"], lay["chunkLen"], variant,
                       got["buildVariant"], got["compactFallback"], info)
                if variant == 3:
                    assert got["buildVariant"] == 3 and got["compactFallback"] == 0, tag
                on_road = check_road(got, table, info, want, 2, uncodable, tag)
                if variant == 3 and not uncodable:
                    codable += 1
                    stayed += on_road
    print(f"slot-code road: block {block}: {stayed} of {codable} codable cases stayed")
    assert 2 * stayed >= codable, (block, stayed, codable)


def test_slot_code_road_by_the_size_rule():
    """The one large case: 2^25 slots at probeLength 1, where a byte holds any 32-bit key -- no flag, the road by the size
    rule (road 1) -- on a random relation of 2^24 tuples whose high parts take all 128 values."""
    n, plen = 1 << 24, 1
    assert hj.slot_codes_info(2 * n, plen)["fitsAuto"]
    rng = np.random.default_rng(20266000)
    R, w, hi = make_relation(rng, n, high=True, plen=plen, hi_mode="uniform")
    assert hi["hiCap"] == 128 and hi["over"] == 0 and np.unique(R >> np.uint64(25)).size == 128
    S = np.ascontiguousarray(np.concatenate([rng.permutation(R)[: n // 4], R[:4096] ^ np.uint64(1 << 31)]))
    want = oracle.build_probe_seq(R, S, plen, want_table=True)
    with hj.HashJoinContext(0) as ctx:
        got, table, info = build_probe_codes(ctx, R, S, plen, 3, False)
        tag = (n, w, plen, got["buildVariant"], got["compactFallback"], info)
        assert got["buildVariant"] == 3 and got["compactFallback"] == 0 and info["fitsAuto"], tag
        check_road(got, table, info, want, 1, False, tag)


@pytest.mark.parametrize("block", range(2))
def test_bucketised_table_on_random_near_sorted_relations(block):
    """The same relations through --algo htm: rings with the chain phase in LDS (or, where that gives up, the generic
    chain kernels: bit 8 of compactFallback), window, global atomics, and the device's pick -- every counter, the primary
    buckets tuple for tuple, the overflow buckets as a multiset, and (small cases) every chain in walk order. Through the
    rings the LDS phase must hand over exactly when the plan of htm_chain_cases.py, evaluated on the device's own seams,
    finds a cause, and for causes of the plan's only: no spurious hand-over, no missing one."""
    cases = int(os.environ.get("HJ_FUZZ_CASES", "36")) // 2
    rng = np.random.default_rng(20261000 + block)
    with hj.HashJoinContext(0) as ctx:
        for case in range(block, cases, 2):
            n = 1 << int(rng.integers(10, 19))
            R, w = make_relation(rng, n)
            R = np.ascontiguousarray(R[: n - int(rng.integers(0, 3))])          # htm takes any size
            S = np.ascontiguousarray(rng.permutation(R)) if rng.integers(0, 2) else np.arange(1, R.size + 1, dtype=np.uint64)
            want = oracle.htm_build_probe_seq(R, S, want_buckets=True)
            key = lambda o: np.sort(o[1:].view(np.uint64).reshape(-1, 4)[:, :3].sum(axis=1))          # noqa: E731
            for variant in (0, 3, 2, 1):
                got = ctx.run("htm", R, S, buildVariant=variant)
                tag = (block, case, R.size, w, variant, got["buildVariant"], got["compactFallback"])
                assert (got["conflicts"], got["conflictSum"], got["totalMatches"], got["inputSum"], got["tableSumFull"],
                        got["htmOverflowBuckets"], got["htmOverflowSum"], got["outputSum"]) == (
                    want["conflictCount"], want["conflictSum"], want["totalMatches"], want["inputSum"], want["bucketSum"],
                    want["overflowBuckets"], want["overflowSum"], want["outputSum"]), tag
                buckets, overflows = ctx.export_buckets(want["numBuckets"])
                assert np.array_equal(buckets["tuples"], want["buckets"]["tuples"]) and np.array_equal(buckets["count"], want["buckets"]["count"]), tag
                assert overflows.size == want["overflows"].size and np.array_equal(key(overflows), key(want["overflows"])), tag
                if R.size <= 1 << 13:
                    a, ao = oracle.htm_chains(buckets, overflows)
                    b, bo = oracle.htm_chains(want["buckets"], want["overflows"])
                    assert np.array_equal(ao, bo) and np.array_equal(a, b), tag
                if variant == 3:
                    assert got["buildVariant"] == 3, tag                 # at least 1022 tuples: a table the rings take
                    info = ctx.htm_chain_info()
                    chain_lay = ctx.htm_chain_layout_info(R.size)
                    plan = cc.chain_plan(R, ctx.wave_layout_info(R.size), chain_lay, ctx.wave_seams()[1])
                    tag += (info, plan.mask)
                    assert chain_lay["tries"] == 1 and plan.strays == 0, tag
                    assert info["state"] == (2 if plan.mask else 1), tag
                    assert (info["cause"] != 0) == (plan.mask != 0) and info["cause"] & ~plan.mask == 0, tag
                    assert (got["compactFallback"] & 0x100 != 0) == (info["state"] == 2), tag
                    if info["state"] == 1:
                        assert info["groups"] == want["overflowBuckets"] == plan.total_groups, tag


@pytest.mark.parametrize("block", range(2))
def test_radix_join_on_random_relations(block):
    """--algo prj on relations of any size and shape: |R| != |S|, key domains from dense to 31 bits, skew in the low key bits
    (pass 1 of the histogram-free path must give up and the exact passes redo the join), in the middle bits (pass 2 gives
    up), many equal keys (partitions beyond one LDS table), through prjMode 0 (the size rule), 1 (exact passes) and 2
    (histogram-free at any size) and several radix widths. Match count and the fork's checksum against the oracle."""
    cases = int(os.environ.get("HJ_FUZZ_CASES", "36")) // 2
    rng = np.random.default_rng(20262000 + block)
    with hj.HashJoinContext(0) as ctx:
        for case in range(block, cases, 2):
            nr = int(rng.integers(1 << 10, 1 << 21))
            ns = int(rng.integers(1 << 10, 1 << 21))
            shape = int(rng.integers(0, 5))
            if shape == 0:                                   # dense domain
                hi = max(nr, ns)
                R = rng.integers(1, hi + 1, size=nr, dtype=np.uint64); S = rng.integers(1, hi + 1, size=ns, dtype=np.uint64)
            elif shape == 1:                                 # 31-bit keys (few matches)
                R = rng.integers(1, 1 << 31, size=nr, dtype=np.uint64); S = np.concatenate([R[: min(nr, ns) // 2], rng.integers(1, 1 << 31, size=ns - min(nr, ns) // 2, dtype=np.uint64)])
            elif shape == 2:                                 # low bits constant: one pass-1 bin takes everything
                c = int(rng.integers(0, 256))
                R = (rng.integers(1, 1 << 20, size=nr, dtype=np.uint64) << np.uint64(8)) | np.uint64(c); S = (rng.integers(1, 1 << 20, size=ns, dtype=np.uint64) << np.uint64(8)) | np.uint64(c)
            elif shape == 3:                                 # middle bits constant: pass 2 cannot spread a partition
                R = (rng.integers(1, 1 << 12, size=nr, dtype=np.uint64) << np.uint64(16)) | rng.integers(0, 256, size=nr, dtype=np.uint64)
                S = (rng.integers(1, 1 << 12, size=ns, dtype=np.uint64) << np.uint64(16)) | rng.integers(0, 256, size=ns, dtype=np.uint64)
            else:                                            # repeated keys: ~2 ... 64 tuples per key (more is quadratic work for any hash join, the oracle's included)
                d = int(rng.integers(max(nr, ns) // 64 + 1, max(nr, ns)))
                R = rng.integers(1, d + 1, size=nr, dtype=np.uint64); S = rng.integers(1, d + 1, size=ns, dtype=np.uint64)
            R[R == 0] = 1; S[S == 0] = 1
            bits = int(rng.choice([0, 8, 11, 12, 14, 16]))
            for mode in (0, 1, 2):
                got = ctx.run("prj", R, S, radixBits=bits, prjMode=mode)
                want = oracle.prj_join(R, S, got["radixBits"])
                tag = (block, case, nr, ns, shape, bits, mode, got["prjPath"])
                assert (got["totalMatches"], got["prjChecksum"]) == (want["matches"], want["checksum"]), tag
            if shape in (0, 1):
                assert got["totalMatches"] == oracle.true_cardinality(R, S), (block, case)


@pytest.mark.parametrize("block", range(2))
def test_key_builds_of_a_radix_shard_on_random_keys(block):
    """hj_build_keys_dev / hj_probe_keys_dev (what a radix shard runs on the 32-bit keys it received): any number of keys,
    any home shift 0..6, tables from tight to roomy, unaligned key buffers, every probe length, all build variants --
    counters and the whole table against the sequential oracle with the shard's table size and shift."""
    cases = int(os.environ.get("HJ_FUZZ_CASES", "36")) // 2
    rng = np.random.default_rng(20263000 + block)
    for case in range(block, cases, 2):
        n2 = 1 << int(rng.integers(11, 20))
        keys64, w = make_relation(rng, n2)
        shift = int(rng.integers(0, 7))
        m = int(rng.integers(n2 // 2 + 1, n2 + 1))                          # the shard's share: any count
        keys = np.ascontiguousarray(((keys64[:m] << np.uint64(shift)) | np.uint64(rng.integers(0, 1 << shift))).astype(np.uint32))
        keys = keys[keys != 0]
        m = keys.size
        table_size = 2 * n2
        plen = int(rng.choice([1, 2, 4, 4, 4, 8]))
        S = np.ascontiguousarray(rng.permutation(keys)[: max(1, m // 2)])
        want = oracle.build_probe_seq_ts(keys.astype(np.uint64), S.astype(np.uint64), table_size, shift, plen, want_table=True)
        for variant in (0, 1, 2, 3, 4):
            with hj.HashJoinContext(0) as c:
                c.reserve("atomic", n2, S.size, buildVariant=variant, probeLength=plen)
                ro, so = 4 * int(rng.integers(0, 4)), 4 * int(rng.integers(0, 4))
                d_r = alloc(c, (m + 8) * 4); d_s = alloc(c, (S.size + 8) * 4)
                c.copy_h2d(d_r + ro, keys); c.copy_h2d(d_s + so, S)
                c.build_keys(d_r + ro, m, shift, table_size)
                c.probe_keys(d_s + so, S.size)
                c.checksums()
                got = c.fetch()
                tag = (block, case, n2, m, w, shift, plen, variant, got["buildVariant"], got["compactFallback"])
                for k in ("conflicts", "totalMatches", "inputSum", "tableSumFull", "conflictSum"):
                    assert got[k] == want[k], (k, got[k], want[k], tag)
                assert np.array_equal(c.export_table(table_size), want["table"]), tag
                c.dev_free(d_r); c.dev_free(d_s)


@pytest.mark.parametrize("block", range(2))
def test_a_reused_context_on_a_random_sequence_of_relations(block):
    """hj_build_dev with the device's pick on ONE reserved context while the relation changes at random from step to step
    (tight, loose, no locality, duplicate-heavy, unique): only the kernels of the previously preferred variant are enqueued,
    so every step runs on whatever the last sample left -- and must still produce the sequential table."""
    steps = int(os.environ.get("HJ_FUZZ_CASES", "36"))
    rng = np.random.default_rng(20264000 + block)
    n = 1 << (16 + block)
    S = np.arange(1, n + 1, dtype=np.uint64)
    seen = set()
    with hj.HashJoinContext(0) as c:
        dR = alloc(c, n * 8); dS = alloc(c, n * 8)
        c.copy_h2d(dS, S)
        c.reserve("atomic", n, n)
        for step in range(steps):
            if rng.integers(0, 4) == 0:
                R = rng.permutation(np.arange(1, n + 1, dtype=np.uint64))          # no locality at all
            else:
                R, _ = make_relation(rng, n)
            R = np.ascontiguousarray(R)
            c.copy_h2d(dR, R)
            c.build(dR, n); c.probe(dS, n); c.checksums()
            got = c.fetch()
            want = oracle.build_probe_seq(R, S, 4, want_table=True)
            seen.add(got["buildVariant"])
            for k in ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum"):
                assert got[k] == want[k], (block, step, k, got[k], want[k], got["buildVariant"], got["compactFallback"])
            assert np.array_equal(c.export_table(2 * n), want["table"]), (block, step, got["buildVariant"])
        c.dev_free(dR); c.dev_free(dS)
    assert steps < 20 or len(seen) >= 3, seen                                      # the sequence really moved between the builds
