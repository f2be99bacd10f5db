"""The materialising probe (hj_probe_pairs_dev) through ctypes -> C ABI on an MI355X: the (S row, R row) pairs it writes
against pairs computed HERE with numpy / plain Python, never by the library; the CPU oracle pins the counts
independently. Pairs are compared as sorted arrays of s << 32 | r, element for element: no pair missing, none twice.
Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from oracle import oracle

pytestmark = pytest.mark.gpu

from gpu_harness import Device, ctx, status  # noqa: F401
from join_kinds_common import SENTINEL, GUARD, zipf, planes
from r_marks_common import join_expected, walk_expected


def probe_pairs(ctx, dev, dS, n, capacity, s_idx_base=0):
    """one hj_probe_pairs_dev call -> (found, packed pairs as written (unsorted), guard words intact)"""
    ds, dr = (p.ptr for p in planes(dev, capacity))
    ctx.probe_pairs(dS, n, ds, dr, capacity, s_idx_base)
    found, written, _us, zero = ctx.pairs_info()
    assert written == min(found, capacity) and zero == 0
    s, r = dev.get(ds, capacity + GUARD), dev.get(dr, capacity + GUARD)
    guard_ok = bool((s[capacity:] == SENTINEL).all() and (r[capacity:] == SENTINEL).all())
    if written < capacity:          # nothing behind the last pair either
        guard_ok = guard_ok and bool((s[written:capacity] == SENTINEL).all() and (r[written:capacity] == SENTINEL).all())
    packed = (s[:written].astype(np.uint64) << np.uint64(32)) | r[:written].astype(np.uint64)
    return found, packed, guard_ok


# ---------------------------------------------------------------------------------------------------------------------
# htm: the complete equi-join
# ---------------------------------------------------------------------------------------------------------------------
def _htm_case(name):
    g = oracle.generate_data
    if name == "uniform_1000_x_sorted_1500":                  # rSize not a power of two; S keys absent from R
        return g("uniform", 1 << 10, 1 << 10, 16)[:1000], g("sorted", 2048)[:1500]
    if name == "random_2p16_x_self_and_sorted":               # 32-bit keys; half of S is absent from R
        R = g("random", 1 << 16, 1 << 16, 16)
        return R, np.concatenate([R[::2], g("sorted", 1 << 15)[:30000]])
    if name == "local_shuffle_3M_x_uniform_2p22":
        return g("local_shuffle", 1 << 22, 1 << 22, 16)[:3 * (1 << 20) + 17], g("uniform", 1 << 22, 1 << 22, 16)
    if name == "sorted_2p22_x_zipf_2p21":
        return g("sorted", 1 << 22), zipf(1 << 21, 1 << 22, 0.9, 54321)
    if name == "uniform_2p20_x_uniform_2p18":                 # duplicate keys on both sides
        return g("uniform", 1 << 20, 1 << 20, 16), g("uniform", 1 << 18, 1 << 19, 16)
    if name == "zipf_2p16_x_zipf_2p12_long_chains":           # the hot key: thousands of R copies, a chain of > 1000 buckets
        return zipf(1 << 16, 1 << 12, 1.0, 12345), zipf(1 << 12, 1 << 12, 1.0, 12345)
    if name == "zipf_2p20_x_sorted_2p13":                     # long chains met by few S tuples
        return zipf(1 << 20, 1 << 13, 0.9, 12345), g("sorted", 1 << 13)
    raise KeyError(name)


HTM_CASES = ["uniform_1000_x_sorted_1500", "random_2p16_x_self_and_sorted", "local_shuffle_3M_x_uniform_2p22",
             "sorted_2p22_x_zipf_2p21", "uniform_2p20_x_uniform_2p18", "zipf_2p16_x_zipf_2p12_long_chains",
             "zipf_2p20_x_sorted_2p13"]


@pytest.mark.parametrize("name", HTM_CASES)
def test_htm_pairs_are_the_complete_join(ctx, name):
    R, S = _htm_case(name)
    assert R.size != S.size and R.min() >= 1
    want = join_expected(R, S)
    if "long_chains" in name:
        assert np.bincount(R.astype(np.int64)).max() > 1000
    if name in ("uniform_1000_x_sorted_1500", "random_2p16_x_self_and_sorted"):
        assert not np.isin(S, R).all()
    with Device(ctx) as dev:
        ctx.reserve("htm", R.size, S.size)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, R.size)
        found, packed, guard_ok = probe_pairs(ctx, dev, dS, S.size, want.size + 64)
        res = ctx.fetch()
    assert found == want.size == res["totalMatches"] and res["sSize"] == S.size
    assert found == oracle.htm_build_probe_seq(R, S)["totalMatches"]
    assert guard_ok
    assert np.array_equal(np.sort(packed), want)


# ---------------------------------------------------------------------------------------------------------------------
# open addressing: the reference's walk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("dist", ["sorted", "shuffle", "local_shuffle"])
@pytest.mark.parametrize("n", [1 << 10, 1 << 16, 1 << 22])
def test_open_addressing_unique_keys(ctx, dist, n, variant):
    """keys 1..N in a table of 2N slots have distinct home slots: every R tuple sits in its home slot, an S key in 1..N
    matches exactly the position of that key in R, a key in N+1..2N finds its home slot empty"""
    R = oracle.generate_data(dist, n, n, 16)
    S = oracle.generate_data("sorted", 2 * n)[: n + n // 2 + 3]
    pos = np.empty(n + 1, dtype=np.uint64)
    pos[R.astype(np.int64)] = np.arange(n, dtype=np.uint64)
    want = (np.arange(n, dtype=np.uint64) << np.uint64(32)) | pos[S[:n].astype(np.int64)]       # already sorted by S row
    with Device(ctx) as dev:
        ctx.reserve("atomic", n, S.size, buildVariant=variant, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, n)
        found, packed, guard_ok = probe_pairs(ctx, dev, dS, S.size, n + 16)
        res = ctx.fetch()
    assert res["buildVariant"] != 4 and res["buildVariant"] in (1, 2, 3)
    assert found == n == res["totalMatches"] == oracle.build_probe_seq(R, S, 4)["totalMatches"]
    assert guard_ok
    assert np.array_equal(np.sort(packed), want)


@pytest.mark.parametrize("probe_length", [1, 2, 4, 8])
@pytest.mark.parametrize("dist", ["uniform", "random"])
@pytest.mark.parametrize("n", [1 << 10, 1 << 14])
def test_open_addressing_duplicate_keys(ctx, dist, n, probe_length):
    R = oracle.generate_data(dist, n, n, 16)
    S = np.concatenate([R[: n // 2 + 1], oracle.generate_data("sorted", n)])
    want = walk_expected(R, S, probe_length)
    for variant in (0, 1, 3, 4):
        with Device(ctx) as dev:
            ctx.reserve("atomic", n, S.size, probeLength=probe_length, buildVariant=variant, keepRowIds=True)
            dR, dS = dev.put(R), dev.put(S)
            ctx.build(dR, n)
            found, packed, guard_ok = probe_pairs(ctx, dev, dS, S.size, want.size + 16)
            res = ctx.fetch()
        assert res["buildVariant"] != 4
        assert found == want.size == res["totalMatches"] == oracle.build_probe_seq(R, S, probe_length)["totalMatches"]
        assert guard_ok
        assert np.array_equal(np.sort(packed), want), (variant, probe_length)


# ---------------------------------------------------------------------------------------------------------------------
# bases and slices, truncation, errors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_bases_and_slices(ctx, algo):
    n = 1 << 16
    R = oracle.generate_data("uniform", n, n, 16)
    S = oracle.generate_data("uniform", n, n // 2, 16)[: n - 5]
    base = join_expected(R, S) if algo == "htm" else walk_expected(R, S, 4)
    cuts = [0, 1001, 1001 + 40000, S.size]                   # unequal slices; the second and third start at odd rows
    with Device(ctx) as dev:
        ctx.reserve(algo, n, S.size, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, n, idx_base=1000)
        found, packed, guard_ok = probe_pairs(ctx, dev, dS, S.size, base.size)
        one = ctx.fetch()
        assert guard_ok and found == base.size == one["totalMatches"] and one["sSize"] == S.size
        assert np.array_equal(np.sort(packed), base + np.uint64(1000))          # r shifted by idx_base
        parts, total = [], 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            f, p, ok = probe_pairs(ctx, dev, dS + 8 * a, b - a, base.size, s_idx_base=a)
            assert ok and f == p.size
            parts.append(p)
            total += f
        res = ctx.fetch()
    assert total == base.size
    assert np.array_equal(np.sort(np.concatenate(parts)), base + np.uint64(1000))
    assert res["totalMatches"] == 2 * base.size and res["sSize"] == 2 * S.size     # the one call + the three slices


@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_truncation_never_writes_past_capacity(ctx, algo):
    n = 1 << 18
    R = oracle.generate_data("uniform", n, n, 16)
    S = oracle.generate_data("sorted", n)
    want = join_expected(R, S) if algo == "htm" else walk_expected(R, S, 4)
    with Device(ctx) as dev:
        ctx.reserve(algo, n, n, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, n)
        found, full, ok = probe_pairs(ctx, dev, dS, n, n + n)
        assert ok and found == full.size
        if algo == "atomic":
            assert found == oracle.build_probe_seq(R, S, 4)["totalMatches"]
        assert np.array_equal(np.sort(full), want)
        for capacity in (found // 2, 1, 0):
            f, part, ok = probe_pairs(ctx, dev, dS, n, capacity)
            assert f == found and part.size == capacity
            assert ok, "a word at or behind dOut*[capacity] was written"
            assert np.unique(part).size == part.size and np.isin(part, want).all()
        # capacity 0 with NULL outputs: counts only
        ctx.probe_pairs(dS, n, 0, 0, 0)
        assert ctx.pairs_info()[:2] == (found, 0)


def test_errors_and_noops():
    n = 1 << 12
    R = oracle.generate_data("local_shuffle", n, n, 16)
    S = oracle.generate_data("sorted", n)
    want_count = oracle.build_probe_seq(R, S, 4)
    with hj.HashJoinContext(0) as ctx, Device(ctx) as dev:
        dR, dS = dev.put(R), dev.put(S)
        ds, dr = (p.ptr for p in planes(dev, n))
        # no build yet
        ctx.reserve("atomic", n, n, keepRowIds=True)
        assert status(ctx.probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        # a PRJ context
        ctx.reserve("prj", n, n)
        assert status(ctx.probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        ctx.prj_join(dR, n, dS, n)
        assert status(ctx.probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        # open addressing without the flag: refused, and the context still counts as before
        ctx.reserve("atomic", n, n)
        ctx.build(dR, n)
        assert status(ctx.probe_pairs, dS, n, ds, dr, n) == _lib.HJ_ERR_STATE
        ctx.probe(dS, n)
        ctx.checksums()
        got = ctx.fetch()
        for k in ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum"):
            assert got[k] == want_count[k], k
        assert (dev.get(ds, n) == SENTINEL).all()
        # with the flag: argument errors
        ctx.reserve("atomic", n, n, keepRowIds=True)
        ctx.build(dR, n)
        assert status(ctx.probe_pairs, dS, n, 0, dr, n) == _lib.HJ_ERR_INVALID
        assert status(ctx.probe_pairs, dS, n, ds, 0, n) == _lib.HJ_ERR_INVALID
        assert status(ctx.probe_pairs, dS, n, ds, dr, n, s_idx_base=(1 << 32) - n) == _lib.HJ_ERR_INVALID
        assert status(ctx.probe_pairs, dS, n, ds, dr, n, s_idx_base=(1 << 32) - 1 - n) == _lib.HJ_OK
        s = dev.get(ds, n)
        assert s.min() == (1 << 32) - 1 - n and s.max() == (1 << 32) - 2
        # sSize 0: outputs, counters and the last call's facts stay as they are
        ctx.probe_pairs(dS, n, ds, dr, n)
        before, info = ctx.fetch(), ctx.pairs_info()
        s0, r0 = dev.get(ds, n + GUARD), dev.get(dr, n + GUARD)
        ctx.probe_pairs(dS, 0, ds, dr, n)
        ctx.probe_pairs(0, 0, 0, 0, 0)
        after = ctx.fetch()
        assert (after["totalMatches"], after["sSize"]) == (before["totalMatches"], before["sSize"])
        assert ctx.pairs_info()[:2] == info[:2] == (n, n)
        assert np.array_equal(dev.get(ds, n + GUARD), s0) and np.array_equal(dev.get(dr, n + GUARD), r0)


@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_tuples_outside_the_layout_match_nothing(ctx, algo):
    n = 1 << 12
    R = oracle.generate_data("sorted", n)
    S = oracle.generate_data("sorted", n).copy()
    S[5] = 0
    S[6] |= np.uint64(1) << np.uint64(32)
    S[7] = np.uint64(7) << np.uint64(32)
    S[n - 1] |= np.uint64(1) << np.uint64(63)
    for off in (0, 1):                                     # 16-byte aligned start, and a start on the odd tuple
        Sx = S[off:]
        want = join_expected(R, Sx)
        assert want.size == n - 4 - off
        with Device(ctx) as dev:
            ctx.reserve(algo, n, n, keepRowIds=True)
            dR, dS = dev.put(R), dev.put(S)
            ctx.build(dR, n)
            found, packed, ok = probe_pairs(ctx, dev, dS + 8 * off, Sx.size, n)
        assert ok and found == want.size
        assert np.array_equal(np.sort(packed), want)


def test_shard_check_counts_through_the_pairs_probe(ctx):
    n = 1 << 14
    R = oracle.generate_data("local_shuffle", n, n, 16)
    S = oracle.generate_data("uniform", n, n, 16)[: n - 3]

    def foreign(A):                 # 4 shards on the low key bits, this context is shard 1
        return int(((A & np.uint64(3)) != 1).sum())

    with Device(ctx) as dev:
        try:
            ctx.set_shard_check(4, 0, 1)
            ctx.reserve("atomic", n, n, keepRowIds=True)
            dR, dS = dev.put(R), dev.put(S)
            ctx.build(dR, n)
            assert ctx.fetch()["foreignTuples"] == foreign(R)
            ctx.probe(dS, S.size)
            assert ctx.fetch()["foreignTuples"] == foreign(R) + foreign(S)
            found, packed, ok = probe_pairs(ctx, dev, dS, S.size, n)
            assert ok and ctx.fetch()["foreignTuples"] == foreign(R) + 2 * foreign(S)
            found1, packed1, ok1 = probe_pairs(ctx, dev, dS + 8, S.size - 1, n)
            assert ok1 and ctx.fetch()["foreignTuples"] == foreign(R) + 2 * foreign(S) + foreign(S[1:])
        finally:
            ctx.set_shard_check(0)
    assert np.array_equal(np.sort(packed), walk_expected(R, S, 4))


# ---------------------------------------------------------------------------------------------------------------------
# nothing else moved
# ---------------------------------------------------------------------------------------------------------------------
def _check_oa(got, want):
    for k in ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["outputSum"] == want["outputSumAtomic"]


@pytest.mark.parametrize("dist", ["uniform", "local_shuffle"])
def test_counting_paths_are_untouched(ctx, dist):
    n = 1 << 20
    R = oracle.generate_data(dist, n, n, 16)
    S = oracle.generate_data("sorted", n)
    want = oracle.build_probe_seq(R, S, 4, want_table=True)
    got = ctx.run("atomic", R, S)                                  # flag unset: today's path
    _check_oa(got, want)
    plain = ctx.export_table(2 * n)
    assert np.array_equal(plain, want["table"])
    if dist == "local_shuffle":
        forced = ctx.run("atomic", R, S, buildVariant=4)
        assert forced["buildVariant"] == 4 and forced["compactFallback"] == 0      # the compact table still holds when asked for
        _check_oa(forced, want)
        assert np.array_equal(ctx.export_table(2 * n), want["table"])
    for variant in (0, 4):
        kept = ctx.run("atomic", R, S, buildVariant=variant, keepRowIds=True)      # flag set: same counters, same table, never compact
        _check_oa(kept, want)
        assert kept["buildVariant"] == 3 and kept["compactFallback"] == 0
        assert np.array_equal(ctx.export_table(2 * n), plain)


# ---------------------------------------------------------------------------------------------------------------------
# host-buffer convenience
# ---------------------------------------------------------------------------------------------------------------------
def test_join_pairs_round_trip():
    n = 1 << 14
    R = oracle.generate_data("uniform", n, n // 4, 16)[:12345]
    S = oracle.generate_data("uniform", n, n // 4, 16)                # ~3 R copies per S key: more than |S| pairs, so the outputs grow once
    s_idx, r_idx = hj.join_pairs(R, S)
    want = join_expected(R, S)
    assert want.size > S.size
    assert s_idx.dtype == r_idx.dtype == np.uint32 and s_idx.size == r_idx.size == want.size
    assert np.array_equal(S[s_idx], R[r_idx])                          # the gather maps do what they are for
    assert np.array_equal(np.sort((s_idx.astype(np.uint64) << np.uint64(32)) | r_idx), want)
    Rp = oracle.generate_data("uniform", n, n // 4, 16)
    for algo in ("atomic", "nocc"):
        s_idx, r_idx = hj.join_pairs(Rp, S, algo=algo, probeLength=2)
        assert np.array_equal(np.sort((s_idx.astype(np.uint64) << np.uint64(32)) | r_idx), walk_expected(Rp, S, 2))
        assert np.array_equal(S[s_idx], Rp[r_idx])
    e_s, e_r = hj.join_pairs(R, S[:0])
    assert e_s.size == e_r.size == 0
    with pytest.raises(ValueError):
        hj.join_pairs(R, S, algo="prj")
