"""The counting probe's tuple loop (k_probe<false>, hj_kernels.hip) at the shapes where it can go wrong. On a table of 4-byte
keys a lane issues the windows of its two tuples together and unconditionally: a tuple that can match nothing (payload bits
set, home slot outside the valid range) reads the window at a dummy slot and must count nothing; on 8-byte slots and for
probeLength != 4 the tuples are walked one after the other. Around the 16-byte body one thread takes the head and the tail.
Every count is compared with the sequential oracle (oracle.build_probe_seq) on the same relations; a context's counters add
up over its probes, so each probe is judged by what it added. Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from gpu_harness import Device, ctx  # noqa: F401
import valid_range_cases as vc
from oracle import oracle

pytestmark = pytest.mark.gpu

U64 = np.uint64
N = 1 << 16
T = 2 * N
TUPLES_PER_LANE = 2                          # one 16-byte vector per lane and iteration
SWEEP = 2048 * 256 * TUPLES_PER_LANE         # tuples one pass of the probe's largest launch takes (grid_for: 2048 workgroups)

# every table the tuple path reads: how R is built, what R is, the table format that build must leave (1 = 4-byte keys)
TABLES = {
    "planar": dict(variant=3, keep=False, dist="uniform", fmt=1),
    "compact": dict(variant=4, keep=False, dist="local_shuffle", fmt=1),
    "packed_rings": dict(variant=3, keep=True, dist="uniform", fmt=0),
    "window": dict(variant=2, keep=False, dist="uniform", fmt=0),
    "atomics": dict(variant=1, keep=False, dist="uniform", fmt=0),
}


@pytest.fixture(scope="module")
def relations():
    """R per distribution, read-only; "_end" = the same with keys 2N-4 .. 2N-1, homed in the table's last four slots"""
    out = {}
    for dist in ("uniform", "local_shuffle"):
        R = oracle.generate_data(dist, N, N, 16)
        end = R.copy()
        end[-4:] = np.arange(T - 4, T, dtype=U64)
        for r in (R, end):
            r.setflags(write=False)
        out[dist], out[dist + "_end"] = R, end
    return out


def build(c, dev, table, R, probe=4):
    """R through the table's build on context c -> hj_table_debug; the format is asserted, the planar road too"""
    t = TABLES[table]
    c.reserve("atomic", R.size, R.size, buildVariant=t["variant"], probeLength=probe, keepRowIds=t["keep"])
    c.build(dev.put(R), R.size)
    dbg = c.table_debug()
    got = c.fetch()
    tag = (table, probe, got["buildVariant"], got["compactFallback"], dbg)
    assert dbg["tableFormat"] == t["fmt"] and dbg["tableSlots"] == 2 * R.size, ("vacuous: not the table the case is about", tag)
    if table == "planar":
        assert c.wave_planar_info() == {"planar": True, "planarFallback": 0, "tableFormat": 1}, tag
    return dbg


def probe_adds(c, dev, S, offset=0):
    """one hj_probe_dev over S at a device pointer that is `offset` bytes past a 16-byte boundary -> (matches, foreign) added"""
    S = np.ascontiguousarray(S, dtype=U64)
    buf = dev.alloc(S.nbytes + 32)
    assert buf % 16 == 0 and offset in (0, 8)
    if S.size:
        c.copy_h2d(buf + offset, S)
    before = c.fetch()
    c.probe(buf + offset, S.size)
    after = c.fetch()
    dev.free(buf)
    return after["totalMatches"] - before["totalMatches"], after["foreignTuples"] - before["foreignTuples"]


def want_matches(R, S, probe=4):
    return oracle.build_probe_seq(R, S, probe)["totalMatches"]


def homed_outside(lo, hi_ex, table):
    """one key per slot outside [lo, hi_ex): the slot number with a bit above the table's mask, so it is no key of R"""
    slots = np.concatenate([np.arange(0, lo, dtype=U64), np.arange(hi_ex, table, dtype=U64)])
    return slots + U64(table)


def mixed_side(R, size, dbg, seed):
    """S of `size` tuples: keys of R, the same + 2^20 (same home slot, no member), keys of R under payload bits, and keys
    homed outside the valid range the build reported -- in random order, so every mix meets inside a vector and a lane"""
    rng = np.random.default_rng(seed)
    S = R[rng.integers(0, R.size, size)].copy()
    kind = rng.integers(0, 4, size)
    S[kind == 1] += U64(1 << 20)
    S[kind == 2] |= rng.integers(1, 1 << 31, int((kind == 2).sum())).astype(U64) << U64(32)
    out = homed_outside(dbg["validLo"], dbg["validHiEx"], dbg["tableSlots"])
    assert out.size > 0, ("vacuous: the whole table is valid", dbg)
    S[kind == 3] = out[rng.integers(0, out.size, int((kind == 3).sum()))]
    return S


# ---- the 16-byte body's edges: head, tail, nothing in between ----------------------------------------------------------------
@pytest.mark.parametrize("table", ("planar", "packed_rings"))
def test_vector_edges(ctx, relations, table):
    """S of 0 .. 9 tuples at an aligned pointer (head 0) and 8 bytes behind one (head 1): the body has 0 to 4 vectors, the
    tail 0 or 1 tuples. Every tuple of S is a key of R, the last one a key R holds more than once where there is one."""
    R = relations["uniform"]
    keys, counts = np.unique(R, return_counts=True)
    dup = keys[counts > 1][:1]
    with Device(ctx) as dev:
        build(ctx, dev, table, R)
        total = 0
        for size in (0, 1, 2, 3, 4, 5, 7, 8, 9):
            S = np.concatenate([R[100:100 + size], dup])[-size:] if size else R[:0]
            want = want_matches(R, S)
            total += want
            for offset in (0, 8):
                got, _ = probe_adds(ctx, dev, S, offset)
                print(table, size, offset, got, want)
                assert got == want, (table, size, offset, got, want)
        assert total > 9


# ---- more than one pass of the grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ("planar", "packed_rings"))
def test_grid_stride_with_shard_check(ctx, relations, table):
    """2.5 sweeps of the largest launch + 3 tuples: some lanes run three iterations, some two, thread 0 has a tail (and at
    +8 bytes a head). Members, misses on the same home slots, payload tuples and tuples homed outside the valid range, mixed.
    The shard check is on (4 shards, this one is shard 0): foreignTuples counts the low words of ALL tuples, whatever their
    windows do."""
    R = relations["uniform"]
    size = 5 * SWEEP // 2 + 3
    with Device(ctx) as dev:
        ctx.set_shard_check(4)
        try:
            dbg = build(ctx, dev, table, R)
            S = mixed_side(R, size, dbg, seed=7)
            want = want_matches(R, S)
            foreign = int(((S & U64(3)) != U64(0)).sum())
            assert 0 < want and 0 < foreign < size
            for offset in (0, 8):
                got = probe_adds(ctx, dev, S, offset)
                print(table, offset, got, (want, foreign))
                assert got == (want, foreign), (table, offset, got, want, foreign)
        finally:
            ctx.set_shard_check(0)


# ---- tuples that must read the dummy window ---------------------------------------------------------------------------------
def alternations(valid, invalid):
    """valid and invalid tuples taking turns inside a vector (v i, i v) and inside a lane's neighbouring vectors (v v i i,
    i i v v, v i i v), 64 lanes' worth of each"""
    k = 256
    v, i = valid[:k], invalid[:k]
    assert v.size == k and i.size == k
    a = np.empty(2 * k, dtype=U64)
    a[0::2], a[1::2] = v, i
    b = np.empty(2 * k, dtype=U64)
    b[0::2], b[1::2] = i, v
    c = np.stack([v[0::2], v[1::2], i[0::2], i[1::2]], axis=1).ravel()
    d = np.stack([i[0::2], i[1::2], v[0::2], v[1::2]], axis=1).ravel()
    e = np.stack([v[0::2], i[0::2], i[1::2], v[1::2]], axis=1).ravel()
    return np.concatenate([a, b, c, d, e])


@pytest.mark.parametrize("table", ("planar", "compact", "packed_rings", "window"))
def test_tuples_that_can_match_nothing(ctx, table):
    """R's home slots are a band in the middle of a table on which an earlier build left a key on EVERY slot, so what lies
    outside the range the build reports is stale and full. S asks for every stale key, for keys homed on the slots at both
    ends of the range, for R's keys under payload bits, and for all of R -- valid and invalid tuples alternating inside a
    vector and inside a lane. The oracle knows R alone."""
    t = TABLES[table]
    band = vc.band_relation(N, T, T // 4, shuffle=16)
    assert vc.classify(band) == "interior"
    P = vc.poison_for(band, "sorted" if t["fmt"] else "perm", htm=False)
    with Device(ctx) as dev:
        ctx.reserve("atomic", N, 0, buildVariant=4 if t["fmt"] else 1)
        ctx.build_keys(dev.put(P.astype(np.uint32)), P.size, 0, T)
        dbg = ctx.table_debug()
        assert (dbg["validLo"], dbg["validHiEx"], dbg["tableFormat"]) == (0, T, t["fmt"]), ("vacuous: no stale keys in this format", dbg)
        R = band.R
        ctx.reserve("atomic", N, N, buildVariant=t["variant"], keepRowIds=t["keep"])
        ctx.build(dev.put(R), N)
        dbg = ctx.table_debug()
        lo, hi = dbg["validLo"], dbg["validHiEx"]
        assert dbg["tableFormat"] == t["fmt"] and 0 < lo <= band.lo and band.hi_ex <= hi and hi + vc.BLOCK < T, ("vacuous: the range is not interior", dbg)
        stale = np.unique(P)
        homes = vc.homes(stale, T)
        outside = stale[(homes < U64(lo)) | (homes >= U64(hi))]
        assert outside.size > 1024
        payload = R | (U64(0x5A5A5A5A) << U64(32))
        edges = vc.keys_homed_at(band, vc.edge_slots(lo, hi, T))
        S = np.concatenate([alternations(R, outside), alternations(R[300:], payload[300:]), alternations(outside[300:], payload),
                            edges, outside, R, band.twins, payload[:1001]])
        want = want_matches(R, S)
        assert want >= R.size
        for offset in (0, 8):
            got, _ = probe_adds(ctx, dev, S, offset)
            print(table, offset, got, want, (lo, hi))
            assert got == want, (table, offset, got, want, lo, hi)
        assert probe_adds(ctx, dev, np.concatenate([outside, payload]))[0] == 0


# ---- the table's end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
def test_windows_at_the_table_end(ctx, relations, table):
    """R holds keys 2N-4 .. 2N-1, homed in the last four slots: the windows of 2N-3 .. 2N-1 reach one to three slots past
    the table, into the slack, and must find it empty. 2N-5 is no member and walks over all four."""
    t = TABLES[table]
    R = relations[t["dist"] + "_end"]
    S = np.concatenate([np.arange(T - 5, T, dtype=U64), R[:11], np.arange(T - 5, T, dtype=U64)[::-1],
                        np.arange(T - 5, T, dtype=U64) | U64(1 << 32)])
    want = want_matches(R, S)
    assert want >= 8
    with Device(ctx) as dev:
        ctx.reserve("atomic", N, N, buildVariant=t["variant"], keepRowIds=t["keep"])
        ctx.build(dev.put(R), N)
        dbg = ctx.table_debug()
        # a relation that reaches the table's end may make the ring builds hand over: whichever build took it, the format
        # is what the probe branches on
        print(table, ctx.fetch()["buildVariant"], dbg)
        assert dbg["validHiEx"] == T, dbg              # the last slots are home slots of R
        for offset in (0, 8):
            got, _ = probe_adds(ctx, dev, S, offset)
            assert got == want, (table, offset, got, want, dbg)


# ---- every table, every probe length -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
def test_every_table_the_tuple_path_reads(ctx, relations, table):
    """sorted S (the benchmark's), a mixed S of a few vectors more than one workgroup takes, on each format and build"""
    R = relations[TABLES[table]["dist"]]
    with Device(ctx) as dev:
        dbg = build(ctx, dev, table, R)
        sides = {"sorted": oracle.relS_for("uniform", R)}
        if dbg["validHiEx"] < dbg["tableSlots"]:
            sides["mixed"] = mixed_side(R, 2 * 256 * 3 + 5, dbg, seed=11)
        for name, S in sides.items():
            want = want_matches(R, S)
            for offset in (0, 8):
                got, _ = probe_adds(ctx, dev, S, offset)
                assert got == want > 0, (table, name, offset, got, want)


@pytest.mark.parametrize("probe", (1, 2, 8))
@pytest.mark.parametrize("table", ("planar", "packed_rings"))
def test_other_probe_lengths(ctx, relations, table, probe):
    """probeLength 1, 2 and 8 walk slot by slot inside the same loop, on one table of each format"""
    R = relations["uniform"]
    with Device(ctx) as dev:
        dbg = build(ctx, dev, table, R, probe)
        for name, S in (("sorted", oracle.relS_for("uniform", R)), ("mixed", mixed_side(R, 2 * 256 * 3 + 5, dbg, seed=13))):
            want = want_matches(R, S, probe)
            for offset in (0, 8):
                got, _ = probe_adds(ctx, dev, S, offset)
                assert got == want > 0, (table, probe, name, offset, got, want)
