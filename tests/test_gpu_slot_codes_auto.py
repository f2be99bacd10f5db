"""Slot codes by the size rule (road 1 of hj_slot_codes_info): the road every large table join of a context without row ids
takes, at the smallest tables where (32 - log2 tableSize) + ceil(log2 probeLength) <= 7 holds by itself -- 2^25 slots at
probeLength 1, 2^26 at 2, 2^27 at 3 and 4 -- with keys ABOVE the table size, so that the high part of every code, of every
probed key and of every decoded slot is something other than 0. test_gpu_slot_codes.py forces the road onto 2^15-slot tables
(road 2); no case here passes slotCodes=True (but the last leg of the bare-key probe, which says so), and every case asserts
through slot_codes_info() that the size rule took the road, that the table one size smaller would not have, and that the
classic rings built it. probeLength 8 needs 2^28 slots and a 1 GiB relation: left out; its byte walk is the one
probeLength 3 takes here.

A relation is home + hi * tableSize in plain numpy arithmetic: near-sorted homes (the rings keep them), equal and
neighbouring homes (conflicts, walks, deferrals), hi over every value the table leaves room for, neighbours with different
high parts. Every expected value is the sequential oracle's on the same arrays. Where many small probe sides meet ONE
table (the probe's edges), the oracle's own table is walked by np_probe, the oracle's probe loop in numpy, which is held to
the oracle's totalMatches on the large probe side first. Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import Device, alloc, ctx  # noqa: F401
import valid_range_cases as vc
from oracle import oracle

pytestmark = pytest.mark.gpu

U64 = np.uint64
I64 = np.int64
COUNTERS = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum")
TBITS = {1: 25, 2: 26, 3: 27, 4: 27}         # probeLength -> log2(table slots): the smallest table the rule takes by itself
FREE_HEAD = 16                               # no home slot below it: walks that wrap past the table's end land on free slots
ALL_ONES = 0xFFFFFFFF


# ---- relations ------------------------------------------------------------------------------------------------------------
def base_relation(tbits):
    """n = 2^(tbits - 1) tuples for a table of T = 2^tbits slots. Homes 2 i + (0..7) + FREE_HEAD: out of order by up to 7
    slots, equal and neighbouring homes everywhere; every 64 positions six tuples share ONE home (two of them are conflicts at
    probeLength 4, the others displace their neighbours); one tuple in 1024 is its predecessor again (a duplicate KEY); one
    in 2^15 is homed 4096 slots ahead of its neighbours, outside any ring: deferred. The last dozen homes are clipped to the
    table's last slot: their walks wrap. hi = 37 i + i / 2048 (mod 2^(32 - tbits)): every value, neighbours differ."""
    T = 1 << tbits
    n = T >> 1
    nhi = 1 << (32 - tbits)
    i = np.arange(n, dtype=I64)
    home = 2 * i + (((i * 2654435761) >> 16) & 7) + FREE_HEAD
    hi = (37 * i + (i >> 11)) & (nhi - 1)
    g = np.arange(40, n - 8, 64)
    for k in range(1, 6):
        home[g + k] = home[g]
    d = np.arange(517, n, 1024)
    home[d], hi[d] = home[d - 1], hi[d - 1]
    e = np.arange(7001, n - 4096, 1 << 15)
    home[e] += 4096
    np.minimum(home, T - 1, out=home)
    return (home + hi * T).astype(U64)


def with_tail(rel, tbits, keys):
    """a copy whose last 32 positions are homed on the slots from T - 64 on, one each, and end in `keys`: nothing but
    `keys` is homed in the table's last 32 slots, and slots 0 .. FREE_HEAD - 1 are free for what wraps"""
    T, n, nhi = 1 << tbits, rel.size, 1 << (32 - tbits)
    keys = np.asarray(keys, dtype=U64)
    t = np.arange(32 - keys.size, dtype=I64)
    out = rel.copy()
    out[n - 32:n - keys.size] = ((T - 64 + t) + ((5 * t + 3) % nhi) * T).astype(U64)
    out[n - keys.size:] = keys
    return out


def variants_of(homes, tbits, nhi=None):
    """every key homed on these slots: all 2^(32 - tbits) high parts (or the first nhi)"""
    homes = np.asarray(homes, dtype=U64)
    his = np.arange(nhi or 1 << (32 - tbits), dtype=U64) << U64(tbits)
    return (homes[:, None] + his[None, :]).ravel()


def probe_side(rel, tbits, third=3):
    """every third tuple of R; for 2048 of R's home slots and for the table's last five slots EVERY high-part variant (a
    key matches only itself); R's keys under payload bits, which match nothing"""
    T = 1 << tbits
    homes = np.concatenate([rel[4000:4000 + 3 * 2048:3] & U64(T - 1), np.arange(T - 5, T, dtype=U64)])
    payload = np.concatenate([rel[1::4096] | (U64(0x5A5A5A5A) << U64(32)), rel[2::4096] | (U64(1) << U64(32))])
    return np.concatenate([rel[::third], variants_of(homes, tbits), payload])


def np_probe(table, S, probe):
    """the oracle's probe loop (no wrap: past the table's end is empty) on the oracle's own table -> matches"""
    T = table.size
    S = np.asarray(S, dtype=U64)
    home = (S & U64(T - 1)).astype(I64)
    alive = np.ones(S.size, dtype=bool)
    matches = 0
    for j in range(probe):
        at = home + j
        v = np.where(at < T, table[np.minimum(at, T - 1)], U64(0))
        alive &= v != 0
        matches += int(np.count_nonzero(alive & (v == S)))
    return matches


def decode_restated(raw, slots, tbits, probe):
    """the format as the header states it (test_code_round_trip_restated), in numpy: code bytes -> keys, 0 = empty"""
    dbits = hj.slot_codes_info(1 << tbits, probe)["dbits"]
    code = raw.astype(I64)
    key = ((np.asarray(slots, dtype=I64) - (code & ((1 << dbits) - 1))) & ((1 << tbits) - 1)) | ((code >> dbits) << tbits)
    return np.where(raw == 0xFF, 0, key).astype(U64)


# ---- checks ---------------------------------------------------------------------------------------------------------------
def check_boundary(tbits, probe):
    """the case sits on the rule's boundary: this table fits by itself, the one half its size does not"""
    assert hj.slot_codes_info(1 << tbits, probe)["fitsAuto"], (tbits, probe)
    assert not hj.slot_codes_info(1 << (tbits - 1), probe)["fitsAuto"], (tbits, probe)


def check_road1(got, info, tag, tbits=27, probe=4):
    """the size rule took the road, on its boundary, and the classic rings kept it: one code byte per slot, no hand-over.
    (Where a case can, it checks its results first: they hold on any road, and a rule that regressed fails here alone.)"""
    check_boundary(tbits, probe)
    assert (info["fitsAuto"], info["codes"], info["road"], info["cause"], info["tableFormat"]) == (True, True, 1, 0, 2), (tag, info)
    assert (got["buildVariant"], got["compactFallback"]) == (3, 0), (tag, got["buildVariant"], got["compactFallback"])


def check_exact(got, table, want, tag):
    for k in COUNTERS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert got["outputSum"] == want["outputSumAtomic"], tag
    if table is not None:
        assert np.array_equal(table, want["table"]), tag


def build_probe(c, rel, S, probe, variant=3, export=True):
    """one build + probe + checksums through the split API -> (result, exported table, slot_codes_info)"""
    c.reserve("atomic", rel.size, S.size, probeLength=probe, buildVariant=variant)
    with Device(c) as dev:
        c.build(dev.put(np.ascontiguousarray(rel, dtype=U64)), rel.size)
        c.probe(dev.put(np.ascontiguousarray(S, dtype=U64)), S.size)
        c.checksums()
        got = c.fetch()
        return got, (c.export_table(2 * rel.size) if export else None), c.slot_codes_info()


def raw_codes(c, first, count):
    """`count` bytes of the code plane from slot `first` on"""
    raw = np.empty(count, dtype=np.uint8)
    c.copy_d2h(raw, c.table_debug()["tableAddr"] + first)
    return raw


def probe_adds(c, dev, S, offset=0, keys32=False):
    """one hj_probe_dev (hj_probe_keys_dev) over S at a device pointer `offset` bytes past a 16-byte boundary -> matches added"""
    S = np.ascontiguousarray(S, dtype=np.uint32 if keys32 else U64)
    buf = dev.alloc(S.nbytes + 32)
    assert buf % 16 == 0 and offset % S.itemsize == 0 and offset < 16
    if S.size:
        c.copy_h2d(buf + offset, S)
    before = c.fetch()["totalMatches"]
    (c.probe_keys if keys32 else c.probe)(buf + offset, S.size)
    added = c.fetch()["totalMatches"] - before
    dev.free(buf)
    return added


# ---- fixtures: one relation per size, one oracle table and one device table at 2^27 slots ------------------------------------
@pytest.fixture(scope="module")
def world():
    cache = {}

    def get(tbits):
        if tbits not in cache:
            cache[tbits] = base_relation(tbits)
            cache[tbits].setflags(write=False)
        return cache[tbits]
    return get


@pytest.fixture(scope="module")
def oracle27(world):
    """the base relation at 2^27 slots, its probe side and the oracle's answer with its table, probeLength 4; np_probe held
    to the oracle's count"""
    rel = world(27)
    S = probe_side(rel, 27)
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    assert np_probe(want["table"], S, 4) == want["totalMatches"]
    return rel, S, want


@pytest.fixture(scope="module")
def built27(oracle27):
    """a context of its own that keeps the 2^27-slot code table of the base relation, built once: the probe's edges run on it"""
    rel = oracle27[0]
    c = hj.HashJoinContext(0)
    c.reserve("atomic", rel.size, rel.size, probeLength=4, buildVariant=3)
    dR = alloc(c, rel.nbytes)
    c.copy_h2d(dR, rel)
    c.build(dR, rel.size)
    info, got = c.slot_codes_info(), c.fetch()
    starts, bounds, _ = c.wave_seams()
    yield {"ctx": c, "info": info, "got": got, "starts": starts.astype(I64), "bounds": bounds.astype(I64), "lay": c.wave_layout_info(rel.size)}
    c.dev_free(dR)
    c.close()


# ---- parity per shape -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", (1, 2, 3, 4))
def test_parity_on_the_size_rule(ctx, world, oracle27, probe):
    """every counter, the three sums and the exported table slot for slot, at the smallest table of each probeLength"""
    tbits = TBITS[probe]
    if probe == 4:
        rel, S, want = oracle27
    else:
        rel = world(tbits)
        S = probe_side(rel, tbits)
        want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    assert want["conflicts"] > 0 and 0 < want["totalMatches"] < S.size, (want["conflicts"], want["totalMatches"], S.size)
    got, table, info = build_probe(ctx, rel, S, probe)
    print("parity", probe, "conflicts", got["conflicts"], "totalMatches", got["totalMatches"], "of", S.size, "deferred", got["buildDeferred"], info)
    check_exact(got, table, want, probe)
    check_road1(got, info, probe, tbits, probe)
    assert (info["tableBits"], info["dbits"], info["hiCap"]) == (tbits, {1: 0, 2: 1, 3: 2, 4: 2}[probe], 1 << (32 - tbits)), info
    assert got["buildDeferred"] > 0, probe


# ---- the largest code ---------------------------------------------------------------------------------------------------------
def top_run(tbits, probe, last=ALL_ONES):
    """probeLength keys on the table's last slot, the last of them `last` (0xFFFFFFFF: the highest high part)"""
    T, nhi = 1 << tbits, 1 << (32 - tbits)
    return [T - 1 + h * T for h in (0, 1, nhi // 2)[:probe - 1]] + [last]


@pytest.mark.parametrize("probe", (4, 1, 2))
def test_largest_code_is_all_ones_key(ctx, world, probe):
    """key 0xFFFFFFFF is a key like any other here. A run of probeLength keys on its home slot -- the table's last -- ends in
    it: it lands on displacement probeLength - 1 (past the table's end, wrapped), its code byte is 127, the largest there
    is and one below the empty test's bit 7. The build keeps the road. S asks for it twice and for 0xFFFFFFFF - T."""
    tbits = TBITS[probe]
    T = 1 << tbits
    rel = with_tail(world(tbits), tbits, top_run(tbits, probe))
    ask = np.array([ALL_ONES, ALL_ONES, ALL_ONES - T], dtype=U64)
    S = np.concatenate([ask, rel[-40:], variants_of([T - 1, T - 2, 0, 1, 2], tbits), probe_side(rel, tbits, 64)])
    want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    slot = (T - 1 + probe - 1) & (T - 1)
    assert want["table"][slot] == ALL_ONES and (slot - ALL_ONES) & (T - 1) == probe - 1, "vacuous: the key is not on the last displacement"
    got, table, info = build_probe(ctx, rel, S, probe)
    check_exact(got, table, want, ("largest", probe))
    check_road1(got, info, ("largest", probe), tbits, probe)
    code = int(raw_codes(ctx, slot & ~15, 16)[slot & 15])
    print("largest code", probe, "slot", slot, "code", code, "totalMatches", got["totalMatches"])
    assert code == 127, (probe, slot, code)


@pytest.mark.parametrize("probe", (4, 1, 2))
def test_all_ones_key_in_s_alone_matches_nothing(ctx, world, probe):
    """the mirror image: the slot holds the key with the high part one below (a code that differs in one bit), S asks for
    0xFFFFFFFF"""
    tbits = TBITS[probe]
    T = 1 << tbits
    rel = with_tail(world(tbits), tbits, top_run(tbits, probe, last=ALL_ONES - T))
    assert not (rel == ALL_ONES).any()
    ask = np.array([ALL_ONES, ALL_ONES, ALL_ONES - T, ALL_ONES, ALL_ONES - 2 * T], dtype=U64)
    assert oracle.build_probe_seq(rel, ask, probe)["totalMatches"] == (1 if probe == 1 else 0)   # found only where no walk wraps
    S = np.concatenate([ask, rel[-40:], probe_side(rel, tbits, 64)])
    want = oracle.build_probe_seq(rel, S, probe)
    got, _, info = build_probe(ctx, rel, S, probe, export=False)
    check_exact(got, None, want, ("mirror", probe))
    with Device(ctx) as dev:
        assert probe_adds(ctx, dev, np.full(37, ALL_ONES, dtype=U64)) == 0
        assert probe_adds(ctx, dev, np.full(37, ALL_ONES, dtype=U64), 8) == 0
    check_road1(got, info, ("mirror", probe), tbits, probe)


# ---- directed runs at 2^27 slots: one relation, one build ------------------------------------------------------------------------
RUN_HI = (0, 31, 16, 0, 31, 16)              # bit 4 of the high part, and the top value
CROSS_HI = 21
CROSS_COPIES = 8


@pytest.fixture(scope="module")
def directed(ctx, oracle27, built27):
    """The base relation at probeLength 4 with, planned on the seams the base build reported (wave_seams):
      * six tuples k, k + 31 T, k + 16 T, k, k + 31 T, k + 16 T on ONE home slot in the middle of a chunk, on the slot two
        below a range's first slot in the six positions before that seam, and on slot T - 3 at the relation's end;
      * family A of tests/wave_cases.py at another seam: CROSS_COPIES copies of the key homed on the last slot below the
        range, high part 21, in the positions before the seam -- all but the first walk across it and displace tuples with
        other high parts."""
    base = oracle27[0]
    T, n = 1 << 27, base.size
    starts, bounds, lay = built27["starts"], built27["bounds"], built27["lay"]
    gran, nc = lay["granuleSlots"], lay["nChunks"]
    c1, c2, c3 = nc // 3, (2 * nc) // 3, nc // 2
    q1, L1 = int(starts[c1]), int(bounds[c1]) * gran
    q2, L2 = int(starts[c2]), int(bounds[c2]) * gran
    mid = int(starts[c3]) + lay["chunkLen"] // 2
    Hm = 2 * mid + FREE_HEAD + 10              # ahead of every walk of the tuples before it: the run meets free slots
    rel = with_tail(base, 27, [T - 3 + h * T for h in RUN_HI])
    rel[q1 - 6:q1] = [L1 - 2 + h * T for h in RUN_HI]
    rel[mid:mid + 6] = [Hm + h * T for h in RUN_HI]
    K = L2 - 1 + CROSS_HI * T
    rel[q2 - CROSS_COPIES:q2] = K
    homes = [L1 - 2, Hm, T - 3, L2 - 1]
    near = np.concatenate([np.arange(h - 2, h + 10) for h in homes]) & (T - 1)
    S = np.concatenate([variants_of(near, 27), rel[q1 - 40:q1 + 40], rel[q2 - 40:q2 + 40], rel[-40:], probe_side(rel, 27, 64)])
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    got, table, info = build_probe(ctx, rel, S, 4)
    s2, b2, _ = ctx.wave_seams()
    raw = {name: raw_codes(ctx, lo, 64) for name, lo in (("seam", L1 - 16), ("cross", L2 - 16), ("end", T - 64), ("start", 0))}
    return {"rel": rel, "want": want, "got": got, "table": table, "info": info, "raw": raw, "K": K, "Hm": Hm,
            "seam": (c1, q1, L1), "cross": (c2, q2, L2), "seen": (s2.astype(I64), b2.astype(I64), gran)}


def test_runs_that_differ_only_above_the_table(directed):
    """what is stored and what is a conflict is the oracle's business; what the cases are about is checked on its table: all
    three high parts of a run are stored, the run before the seam reaches into the next range, the one at the table's end
    wraps"""
    d = directed
    T = 1 << 27
    tab = d["want"]["table"]
    c1, q1, L1 = d["seam"]
    s2, b2, gran = d["seen"]
    assert (int(s2[c1]), int(b2[c1]) * gran) == (q1, L1), "vacuous: the seam moved"
    for name, home in (("seam", L1 - 2), ("middle", d["Hm"]), ("end", T - 3)):
        held = tab[(home + np.arange(4)) & (T - 1)]
        mine = held[(held & U64(T - 1)) == U64(home)]
        assert {int(k) >> 27 for k in mine} == {0, 16, 31}, (name, held)
    assert (tab[L1:L1 + 2] & U64(T - 1) == U64(L1 - 2)).any(), "vacuous: no walk of the run crosses the seam"
    assert int(tab[0]) & (T - 1) == T - 3, "vacuous: the run at the table's end does not wrap"
    assert d["want"]["conflicts"] >= 6 and d["got"]["buildDeferred"] > 0
    check_exact(d["got"], d["table"], d["want"], "runs")
    check_road1(d["got"], d["info"], "runs")
    for name, lo in (("seam", L1 - 16), ("end", T - 64), ("start", 0)):
        slots = lo + np.arange(64)
        assert np.array_equal(decode_restated(d["raw"][name], slots, 27, 4), tab[slots]), name


def test_fixed_up_bytes_carry_the_high_part(directed):
    """the copies of the crossing key (high part 21) that walk across the seam are deferred tuples: the slots they take, and
    the slots of the tuples they displace, are written by the fix-up's byte stores. Raw bytes around the seam decode, in
    numpy, to the oracle's keys."""
    d = directed
    tab, K = d["want"]["table"], d["K"]
    c2, q2, L2 = d["cross"]
    s2, b2, gran = d["seen"]
    assert (int(s2[c2]), int(b2[c2]) * gran) == (q2, L2), "vacuous: the seam moved"
    walkers = int(np.count_nonzero(tab[L2:L2 + 3] == U64(K)))
    assert walkers == 3 and tab[L2 - 1] == U64(K), ("vacuous: the copies do not cross the seam", tab[L2 - 2:L2 + 4])
    others = tab[L2 + 3:L2 + 12]
    assert {int(k) >> 27 for k in others[others != 0]} - {CROSS_HI}, "vacuous: nothing with another high part behind the walkers"
    assert d["got"]["buildDeferred"] >= 4 - 1
    slots = L2 - 16 + np.arange(64)
    assert np.array_equal(d["table"][slots], tab[slots])
    check_road1(d["got"], d["info"], "fixup")
    back = decode_restated(d["raw"]["cross"], slots, 27, 4)
    assert np.array_equal(back, tab[slots]), (back, tab[slots])
    assert (back[16:19] >> U64(27) == U64(CROSS_HI)).all()


# ---- the rotated probe loop at the real shift ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pools27(oracle27):
    """R's keys by high part, for the four high parts a probe vector mixes"""
    rel = oracle27[0]
    hi = (rel >> U64(27)).astype(np.uint8)
    return [rel[hi == h] for h in (0, 1, 16, 31)]


def mixed_side(pools, size, start):
    """keys of R with high parts 0, 1, 16, 31 in turn -- both tuples of every 16-byte vector differ in bit 4 or bit 0 of the
    high part --, every fifth moved one slot on (the same high part on the neighbouring home: held or not, the table says)"""
    S = np.empty(size, dtype=U64)
    for k, pool in enumerate(pools):
        part = S[k::4]
        part[:] = pool[start:start + part.size]
    S[4::5] += U64(1)
    return S


def test_rotated_probe_loop_at_the_real_shift(oracle27, built27, pools27):
    """probe_body_codes, probeLength 4, 8-byte tuples: hiShift = 25 and hiMask = 0x7C. S of 0 .. 9 tuples at an aligned pointer
    and 8 bytes behind one (head and tail by lane 0), then S of exactly one, two and three grid strides of vectors plus one
    vector: the turn whose second vector does not exist (hasB false) and the load that reads the last vector again.
    launch_probe starts grid_for(n / 2 + 1, kBlock) = min(ceil((n / 2 + 1) / 256), 2048) workgroups of kBlock = 256 lanes,
    so from 2^20 tuples on a grid stride is 2048 * 256 = 524288 vectors of two tuples."""
    c, table = built27["ctx"], oracle27[2]["table"]
    stride = 2048 * 256
    total = 0
    with Device(c) as dev:
        for size in (0, 1, 2, 3, 4, 5, 7, 8, 9):
            S = mixed_side(pools27, size, 1000 * size)
            want = np_probe(table, S, 4)
            total += want
            for offset in (0, 8):
                assert probe_adds(c, dev, S, offset) == want, (size, offset)
        assert total >= 20
        for strides in (1, 2, 3):
            size = 2 * (strides * stride + 1)
            assert min(-(-(size // 2 + 1) // 256), 2048) * 256 == stride
            S = mixed_side(pools27, size, 50000 * strides)
            want = np_probe(table, S, 4)
            assert size // 2 < want < size
            for offset in (0, 8):
                got = probe_adds(c, dev, S, offset)
                print("rotated", strides, offset, got, want)
                assert got == want, (strides, offset, got, want)
    check_road1(built27["got"], built27["info"], "rotated")


# ---- stale codes outside the valid range ----------------------------------------------------------------------------------------
def test_stale_codes_outside_the_valid_range(ctx):
    """test_tuples_that_can_match_nothing at 2^27 slots without the flag: R's home slots are the band [T / 4, 3 T / 4) of a code
    plane that was filled, before the build, with "the key homed here with high part 31, displacement 0" (0x7C) on EVERY
    slot. S asks for those keys, for twins whose high part differs from 31 in one bit, for keys homed at both edges of the
    range, for the band's twins and for R under payload bits. The oracle knows R alone."""
    probe, T = 4, 1 << 27
    n = T // 2
    band = vc.band_relation(n, T, T // 4, shuffle=16)
    assert vc.classify(band, probe) == "interior"
    R = band.R
    stale_code = 31 << hj.slot_codes_info(T, probe)["dbits"]
    assert stale_code == 0x7C

    def build(dR):
        ctx.reserve("atomic", n, n, probeLength=probe, buildVariant=3)
        ctx.build(dR, n)
        info = ctx.slot_codes_info()
        check_road1(ctx.fetch(), info, "stale")
        return ctx.table_debug()

    with Device(ctx) as dev:
        dR = dev.put(R)
        dbg = build(dR)
        ctx.synchronize()
        ctx.copy_h2d(dbg["tableAddr"], np.full(T, stale_code, dtype=np.uint8))
        dbg = build(dR)
        lo, hi = dbg["validLo"], dbg["validHiEx"]
        assert 0 < lo <= band.lo and band.hi_ex <= hi and hi + vc.BLOCK < T, ("vacuous: the range is not interior", dbg)
        raw = raw_codes(ctx, 0, T)
        assert (raw[:lo - vc.BLOCK] == stale_code).all() and (raw[hi + 2 * vc.BLOCK:] == stale_code).all(), "vacuous: nothing stale"
        del raw
        slots = np.concatenate([np.arange(0, lo, 61), np.arange(lo - 4096, lo), np.arange(hi, hi + 4096), np.arange(hi, T, 61)]).astype(U64)
        outside = slots + U64(31 * T)
        near_twins = np.concatenate([slots + U64(15 * T), slots + U64(30 * T)])
        payload = R[::64] | (U64(0x5A5A5A5A) << U64(32))
        edges = vc.keys_homed_at(band, vc.edge_slots(lo, hi, T))
        mix = np.empty(4096, dtype=U64)
        mix[0::2], mix[1::2] = R[:2048], outside[:2048]
        mix2 = np.empty(4096, dtype=U64)
        mix2[0::2], mix2[1::2] = payload[:2048], R[2048:4096]
        S = np.concatenate([mix, mix2, edges, outside, R[::16], near_twins, band.twins[::16], payload[:1001]])
        want = oracle.build_probe_seq(R, S, probe, want_table=True)
        assert want["totalMatches"] >= R.size // 16
        for offset in (0, 8):
            assert probe_adds(ctx, dev, S, offset) == want["totalMatches"], (offset, lo, hi)
        assert probe_adds(ctx, dev, np.concatenate([outside, near_twins, payload])) == 0
        # the sums and the export stop at the range too
        ctx.checksums()
        got = ctx.fetch()
        assert (got["tableSumFull"], got["tableSumHalf"]) == (want["tableSumFull"], want["tableSumHalf"])
        assert np.array_equal(ctx.export_table(T), want["table"])


# ---- bare-key probe of a code table ---------------------------------------------------------------------------------------------
KEY_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 4099)


def bare_key_side(rel, tbits, extra, nhi=None):
    """32-bit probe keys: keys of R, every high-part variant (or the first nhi) of some of its homes and of the table's last
    slots, `extra`"""
    T = 1 << tbits
    homes = np.concatenate([rel[300:364] & U64(T - 1), np.arange(T - 4, T, dtype=U64)])
    pool = np.concatenate([rel[200:3200], variants_of(homes, tbits, nhi), np.asarray(extra, dtype=U64)])
    assert pool.dtype == U64 and pool.size > KEY_LENGTHS[-1]
    assert int(pool.max()) <= ALL_ONES
    return pool[(np.arange(pool.size) * 7919) % pool.size]          # mixed: every vector of four holds keys of several kinds


def test_bare_key_probe_on_the_size_rule(oracle27, built27):
    """hj_probe_keys_dev on the code table a tuple build left (probe_body_codes<KEY32>: the byte walk, four keys per vector),
    lengths 0 to 9 and a few thousand, at an aligned pointer and 4, 8 and 12 bytes behind one"""
    c, (rel, _, want) = built27["ctx"], oracle27
    pool = bare_key_side(rel, 27, [ALL_ONES, ALL_ONES - (1 << 27)])
    total = 0
    with Device(c) as dev:
        for size in KEY_LENGTHS:
            S = pool[11 * size:12 * size] if size < 4099 else pool[:size]
            expect = np_probe(want["table"], S, 4)
            total += expect
            for offset in (0, 4, 8, 12):
                assert probe_adds(c, dev, S, offset, keys32=True) == expect, (size, offset)
    assert 1000 < total < pool.size
    check_road1(built27["got"], built27["info"], "keys")


@pytest.mark.parametrize("probe", (4, 8))
def test_bare_key_probe_on_the_forced_road(ctx, probe):
    """the same on the FORCED road (reserve(..., slotCodes=True), 2^15 slots), where a key can overflow: 32-bit probe keys
    with a high part at or above hiCap -- 0xFFFFFFFF among them -- match nothing, whatever they alias to"""
    n, tbits = 1 << 14, 15
    T = 1 << tbits
    cap = hj.slot_codes_info(T, probe)["hiCap"]
    rel = oracle.generate_data("uniform", n, n, 16)
    rel[-4:] = np.arange(T - 4, T, dtype=U64)
    rel = rel + (((rel * U64(2654435761)) >> U64(7)) % U64(cap)) * U64(T)
    over = np.concatenate([rel[:300] + U64(cap * T), rel[300:600] + U64(2 * cap * T), np.array([ALL_ONES, ALL_ONES - T, cap * T + 5], dtype=U64)])
    pool = bare_key_side(rel, tbits, over, nhi=4 * cap)
    assert (pool >> U64(tbits) >= U64(cap)).sum() > 600
    with Device(ctx) as dev:
        ctx.reserve("atomic", n, n, probeLength=probe, buildVariant=3, slotCodes=True)
        ctx.build(dev.put(rel), n)
        info = ctx.slot_codes_info()
        assert (info["codes"], info["cause"], info["road"], info["tableFormat"], info["fitsAuto"]) == (True, 0, 2, 2, False), info
        total = 0
        for size in KEY_LENGTHS:
            S = pool[11 * size:12 * size] if size < 4099 else pool[:size]
            expect = oracle.build_probe_seq(rel, S, probe)["totalMatches"]
            total += expect
            for offset in (0, 4, 8, 12):
                assert probe_adds(ctx, dev, S, offset, keys32=True) == expect, (probe, size, offset)
        assert 500 < total < pool.size


# ---- the auto variant on the benchmark's distribution --------------------------------------------------------------------------
def test_auto_variant_on_the_benchmark_distribution():
    """`uniform` W=16 at 2^24 with a high part per key value (equal keys stay equal), probeLength 1, buildVariant 0: the
    pre-round picks the classic rings on the duplicate keys and the size rule follows. Then, on the same context, a `sorted`
    unique relation -- the compact rings: 4-byte keys, the rule still says road 1, no code plane --, then the first one
    again. Every reader -- probe, sums, export -- on each of the three builds."""
    tbits, probe = 25, 1
    T = 1 << tbits
    n = T // 2
    uniform = oracle.generate_data("uniform", n, n, 16)
    uniform = uniform + (((uniform * U64(2654435761)) >> U64(9)) & U64(127)) * U64(T)
    assert np.unique(uniform >> U64(tbits)).size == 128 and np.unique(uniform).size < n
    unique = oracle.generate_data("sorted", n)
    with hj.HashJoinContext(0) as c:
        for step, (rel, variant, fmt) in enumerate(((uniform, 3, 2), (unique, 4, 1), (uniform, 3, 2))):
            S = np.concatenate([probe_side(rel, tbits), uniform[:5000], unique[:5000]])
            want = oracle.build_probe_seq(rel, S, probe, want_table=True)
            assert 0 < want["totalMatches"] < S.size
            got, table, info = build_probe(c, rel, S, probe, variant=0)
            print("auto", step, got["buildVariant"], info)
            check_exact(got, table, want, step)
            check_boundary(tbits, probe)
            assert (got["buildVariant"], got["compactFallback"]) == (variant, 0), (step, got["buildVariant"], got["compactFallback"])
            assert (info["fitsAuto"], info["road"], info["codes"], info["cause"], info["tableFormat"]) == (True, 1, fmt == 2, 0, fmt), (step, info)
            assert c.table_debug()["tableFormat"] == fmt
