"""Slot codes (table format 2, hj_table.h SlotCode): the classic ring build of a context without row ids leaves ONE BYTE per
slot -- code = (hi << dbits) | d for the key homed d slots below with bits `hi` above the table size, 0xFF = empty -- and the
probe, the checksums and the export read that byte. The road is taken by itself only from 2^27 slots on (where a byte holds
any 32-bit key); here it is forced onto small tables with reserve(..., slotCodes=True) and every case asserts through
slot_codes_info() that it really was taken, so none can pass on the 4-byte road. Every result -- exported table, conflicts,
totalMatches, the three sums -- is the sequential oracle's. The seam relations come from tests/wave_cases.py, the band
relations from tests/valid_range_cases.py. The size rule at the end needs no device. Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import Device, ctx  # noqa: F401
import valid_range_cases as vc
import wave_cases as wc
from oracle import oracle

gpu = pytest.mark.gpu

U64 = np.uint64
N = 1 << 14                                  # eight chunks of 2048 tuples: seven seams
T = 2 * N
COUNTERS = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum")
LOG_OVERFLOW, EMPTY_PATTERN, CODE_OVERFLOW = 1, 2, 4         # slot_codes_info()["cause"]


def build_probe(c, rel, S, probe=4, variant=3, slot_codes=True, idx_base=0):
    """one build + probe + checksums through the split API -> (result, exported table, slot_codes_info)"""
    c.reserve("atomic", rel.size, S.size, probeLength=probe, buildVariant=variant, slotCodes=slot_codes)
    with Device(c) as dev:
        c.build(dev.put(np.ascontiguousarray(rel, dtype=U64)), rel.size, idx_base)
        c.probe(dev.put(np.ascontiguousarray(S, dtype=U64)), S.size)
        c.checksums()
        got = c.fetch()
        return got, c.export_table(2 * rel.size), c.slot_codes_info()


def check_exact(got, table, want, tag):
    for k in COUNTERS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert got["outputSum"] == want["outputSumAtomic"], tag
    assert np.array_equal(table, want["table"]), tag


def check_codes(got, info, tag):
    """the forced road taken and kept: one code byte per slot, no hand-over"""
    assert (got["buildVariant"], got["compactFallback"]) == (3, 0), tag
    assert (info["codes"], info["cause"], info["road"], info["tableFormat"]) == (True, 0, 2, 2), (tag, info)


def probe_side(rel):
    """every third tuple, and keys on the same home slots that the relation does not hold (other high bits)"""
    return np.concatenate([rel[::3], rel[:64] + U64(7 * T)])


# ---- parity with seams, deferrals and dirty slots ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("probe", (1, 2, 3, 4, 8))
def test_uniform_parity(ctx, probe):
    """`uniform` W=16 at 2^14: eight chunks, stragglers at every seam (deferred walks, slots fixed up by byte stores)"""
    rel = oracle.generate_data("uniform", N, N, 16)
    S = oracle.relS_for("uniform", rel)
    want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    for variant in (3, 0):
        got, table, info = build_probe(ctx, rel, S, probe, variant)
        check_exact(got, table, want, (probe, variant))
        check_codes(got, info, (probe, variant))
        assert info["dbits"] == {1: 0, 2: 1, 3: 2, 4: 2, 8: 3}[probe] and info["hiCap"] == 128 >> info["dbits"] and not info["fitsAuto"]
        if probe > 1:
            assert got["buildDeferred"] > 0, probe


# ---- directed seam cases ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(ctx):
    lay = ctx.wave_layout_info(N)
    assert lay["nChunks"] == 8
    return {"lay": lay, "cases": [c for c in wc.cases(N, lay, full=True) if not c.keys32]}


@gpu
@pytest.mark.parametrize("family", ("A", "A1", "B", "C", "D", "H", "R"))
def test_seam_and_deferral_cases(ctx, world, family):
    """tests/wave_cases.py on the forced road (tuples; bare keys never take it). Family A puts up to 200 copies of one key
    right before a seam: all but probeLength of them... walk across it as deferred tuples and take CONSECUTIVE slots from
    the next range's first slot on, displacing what sits there -- neighbouring dirty slots, several inside one 4-byte word
    of the code plane, each fixed up by its own byte store. R: one deferred walk displaces every later tuple of the dense
    base by one slot, up to the relation's end."""
    todo = [c for c in world["cases"] if c.family == family]
    assert todo
    for case in todo:
        rel = wc.relation(case.homes)
        S = probe_side(rel)
        want = oracle.build_probe_seq(rel, S, case.probe, want_table=True)
        got, table, info = build_probe(ctx, rel, S, case.probe)
        check_exact(got, table, want, case.name)
        check_codes(got, info, case.name)
        if family == "R":
            # at this size the one long walk fits its slice's log: thousands of neighbouring slots fixed up byte by byte
            assert got["buildDeferred"] >= 1 and got["conflicts"] == 0, case.name
        if family == "A" and case.crossing is not None:
            assert got["buildDeferred"] >= min(case.crossing, case.probe - 1), case.name
            if case.crossing >= 2 and case.probe >= 4:
                # the walkers' slots: L and L + 1 at least hold copies of the crossing key -- two dirty slots of one word
                L = case.seam.L
                assert L % 4 == 0 and table[L] == table[L + 1] == U64(L - 1), case.name


# ---- high bits alias nothing ----------------------------------------------------------------------------------------------
@gpu
def test_high_bits_alias_nothing(ctx):
    """keys k, k + T, k + 2T share a home slot and differ in the code's high part alone. R takes one of the three per home
    slot (odd homes, sorted), plus runs where all three -- and second copies of them -- sit on ONE home slot and displace each
    other. S asks for all three variants of every home: a key matches only itself."""
    i = np.arange(N, dtype=np.int64)
    homes = 2 * i + 1
    hi = i % 3
    for a in (1000, 5000, 5001, 12000):                        # six tuples on one home slot: k, k+T, k+2T, k, k+T, k+2T
        homes[a:a + 6] = homes[a]
        hi[a:a + 6] = np.arange(6) % 3
    rel = (homes + hi * T).astype(U64)
    S = np.concatenate([(homes + j * T).astype(U64) for j in range(3)])
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    assert 0 < want["conflicts"] and N // 2 < want["totalMatches"] < S.size // 2
    got, table, info = build_probe(ctx, rel, S)
    check_exact(got, table, want, "alias")
    check_codes(got, info, "alias")


# ---- the bounds of a code ---------------------------------------------------------------------------------------------------
def with_run(keys_at_home):
    """the odd base with the four tuples from position 5000 on replaced by keys on that position's home slot"""
    homes = wc.base_odd(N)
    rel = wc.relation(homes)
    H = int(homes[5000])
    rel[5000:5000 + len(keys_at_home)] = [H + h * T for h in keys_at_home]
    return rel, H


@gpu
def test_largest_code_holds(ctx):
    """probeLength 4 on 2^15 slots: hiCap = 32. The key with hi = 31 that lands on displacement 3 has code 127, the largest
    there is: it holds, is found, and is not read as empty (a tuple behind it... does not exist: the walk ends there)"""
    info = hj.slot_codes_info(T, 4)
    assert (info["dbits"], info["hiCap"], info["fitsAuto"]) == (2, 32, False)
    rel, H = with_run([0, 1, 2, 31])
    top = U64(H + 31 * T)
    S = np.concatenate([rel[4990:5010], [top, top, U64(H + 30 * T)], probe_side(rel)])
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    assert want["table"][H + 3] == top and want["conflicts"] == 0
    got, table, info = build_probe(ctx, rel, S)
    check_exact(got, table, want, "largest code")
    check_codes(got, info, "largest code")


@gpu
@pytest.mark.parametrize("key", (32 * T + 12345, 0xFFFFFFFF), ids=("hiCap", "all-ones"))
def test_key_without_a_code_hands_over(ctx, key):
    """one key with hi = hiCap, and key 0xFFFFFFFF (hi = 2^17 - 1 on this table: the same cause, not the 4-byte road's empty
    pattern): cause 4, the 8-byte build redoes the table, exact. S asks for the key and for keys whose high parts are equal
    to a stored one's modulo 2^5 and 2^6."""
    rel = wc.relation(wc.base_odd(N))
    rel[7000] = key
    S = np.concatenate([[key, key], rel[6990:7010], rel[6990:7010] + U64(32 * T), rel[6990:7010] + U64(64 * T), probe_side(rel)]).astype(U64)
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    got, table, info = build_probe(ctx, rel, S)
    check_exact(got, table, want, key)
    assert got["buildVariant"] == 3 and got["compactFallback"] == 0
    assert (info["codes"], info["cause"], info["road"], info["tableFormat"]) == (False, CODE_OVERFLOW, 2, 0), info
    # S may hold such keys on a table that does not: they match nothing, whatever their high parts alias to
    rel = wc.relation(wc.base_odd(N))
    got, table, info = build_probe(ctx, rel, S)
    check_exact(got, table, oracle.build_probe_seq(rel, S, 4, want_table=True), "S only")
    check_codes(got, info, "S only")


# ---- the probe's edges --------------------------------------------------------------------------------------------------------
def probe_adds(c, dev, S, offset=0):
    """one hj_probe_dev over S at a device pointer `offset` bytes past a 16-byte boundary -> matches added"""
    S = np.ascontiguousarray(S, dtype=U64)
    buf = dev.alloc(S.nbytes + 32)
    assert buf % 16 == 0 and offset in (0, 8)
    if S.size:
        c.copy_h2d(buf + offset, S)
    before = c.fetch()["totalMatches"]
    c.probe(buf + offset, S.size)
    added = c.fetch()["totalMatches"] - before
    dev.free(buf)
    return added


def build_codes(c, dev, R, probe=4):
    c.reserve("atomic", R.size, R.size, buildVariant=3, probeLength=probe, slotCodes=True)
    c.build(dev.put(R), R.size)
    info = c.slot_codes_info()
    assert info["codes"] and info["tableFormat"] == 2, ("vacuous: not the table the case is about", info)
    return c.table_debug()


@gpu
@pytest.mark.parametrize("probe", (4, 8))
def test_vector_edges_and_the_table_end(ctx, probe):
    """S of 0 .. 9 tuples at an aligned pointer and 8 bytes behind one; then R with keys homed in the table's last four slots:
    their windows reach into the slack bytes behind the code plane and must find them empty"""
    R = oracle.generate_data("uniform", N, N, 16)
    R[-4:] = np.arange(T - 4, T, dtype=U64)
    keys, counts = np.unique(R, return_counts=True)
    dup = keys[counts > 1][:1]
    with Device(ctx) as dev:
        dbg = build_codes(ctx, dev, R, probe)
        assert dbg["validHiEx"] == T
        total = 0
        for size in (0, 1, 2, 3, 4, 5, 7, 8, 9):
            S = np.concatenate([R[100:100 + size], dup])[-size:] if size else R[:0]
            want = oracle.build_probe_seq(R, S, probe)["totalMatches"]
            total += want
            for offset in (0, 8):
                assert probe_adds(ctx, dev, S, offset) == want, (size, offset)
        assert total > 9
        end = np.arange(T - 5, T, dtype=U64)
        S = np.concatenate([end, R[:11], end[::-1], end | U64(1 << 32), end + U64(T)])
        want = oracle.build_probe_seq(R, S, probe)["totalMatches"]
        assert want >= 8
        for offset in (0, 8):
            assert probe_adds(ctx, dev, S, offset) == want, offset


@gpu
@pytest.mark.parametrize("probe", (4, 2))
def test_tuples_that_can_match_nothing(ctx, probe):
    """R's home slots are a band in the middle of a code plane that was filled, before the build, with the code "the key
    homed here with high part 1" on EVERY slot: outside the range the build reports the plane is stale and full of
    valid-looking codes. S asks for every one of those keys, for keys homed at both ends of the range, for R's keys under
    payload bits, for twins with other high bits and for all of R, alternating inside a vector. The oracle knows R alone."""
    band = vc.band_relation(N, T, T // 4, shuffle=16)
    assert vc.classify(band, probe) == "interior"
    R = band.R
    stale_code = 1 << hj.slot_codes_info(T, probe)["dbits"]                      # hi = 1, d = 0: slot s holds key s + T
    with Device(ctx) as dev:
        dbg = build_codes(ctx, dev, R, probe)
        ctx.synchronize()
        ctx.copy_h2d(dbg["tableAddr"], np.full(T, stale_code, dtype=np.uint8))
        dbg = build_codes(ctx, dev, R, probe)
        lo, hi = dbg["validLo"], dbg["validHiEx"]
        assert 0 < lo <= band.lo and band.hi_ex <= hi and hi + vc.BLOCK < T, ("vacuous: the range is not interior", dbg)
        raw = np.empty(T, dtype=np.uint8)
        ctx.copy_d2h(raw, dbg["tableAddr"])
        assert (raw[:lo - vc.BLOCK] == stale_code).all() and (raw[hi + 2 * vc.BLOCK:] == stale_code).all(), "vacuous: nothing stale"
        slots = np.concatenate([np.arange(0, lo, dtype=U64), np.arange(hi, T, dtype=U64)])
        outside = slots + U64(T)
        payload = R | (U64(0x5A5A5A5A) << U64(32))
        edges = vc.keys_homed_at(band, vc.edge_slots(lo, hi, T))
        mix = np.empty(4096, dtype=U64)
        mix[0::2], mix[1::2] = R[:2048], outside[:2048]
        mix2 = np.empty(4096, dtype=U64)
        mix2[0::2], mix2[1::2] = payload[:2048], R[2048:4096]
        S = np.concatenate([mix, mix2, edges, outside, R, band.twins, payload[:1001]])
        want = oracle.build_probe_seq(R, S, probe)["totalMatches"]
        assert want >= R.size // 2
        for offset in (0, 8):
            assert probe_adds(ctx, dev, S, offset) == want, (offset, lo, hi)
        assert probe_adds(ctx, dev, np.concatenate([outside, payload])) == 0
        # the sums and the export stop at the range too
        ctx.checksums()
        got = ctx.fetch()
        full = oracle.build_probe_seq(R, None, probe, want_table=True)
        assert (got["tableSumFull"], got["tableSumHalf"]) == (full["tableSumFull"], full["tableSumHalf"])
        assert np.array_equal(ctx.export_table(T), full["table"])


# ---- retire shapes ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("per_tile", (1, 2, 3))
def test_retire_shapes(ctx, per_tile):
    """sorted homes at per_tile / 4 slots per tuple: a tile of 512 tuples moves the ring by 1, 2 or 3 granules, a chunk's
    range is 4, 8 or 12 granules; started from granule 1 and from granule 2, the ranges begin on odd granules in one run and
    on even ones in the other. (With four tuples per slot at per_tile = 1 every key fills its window exactly.)"""
    parities = set()
    for first_granule in (1, 2):
        homes = 128 * first_granule + (np.arange(N, dtype=np.int64) * per_tile) // 4
        rel = wc.relation(homes)
        S = probe_side(rel)
        want = oracle.build_probe_seq(rel, S, 4, want_table=True)
        got, table, info = build_probe(ctx, rel, S)
        check_exact(got, table, want, (per_tile, first_granule))
        check_codes(got, info, (per_tile, first_granule))
        _, bounds, _ = ctx.wave_seams()
        inner = bounds[1:-1].astype(np.int64)                  # the first granule of chunks 1 .. 7
        assert (np.diff(inner) == 4 * per_tile).all(), bounds
        parities.add(int(inner[0]) % 2)
    assert parities == {0, 1}


# ---- one context across the roads ------------------------------------------------------------------------------------------
@gpu
def test_one_context_across_roads():
    """codes -> a key without a code (8-byte slots) -> codes again -> the same context reserved without the flag (4-byte
    keys): every reader -- probe, sums, export -- on each, and the info calls say which road it was"""
    uniform = oracle.generate_data("uniform", N, N, 16)
    over = uniform.copy()
    over[9000] = U64(40 * T + 77)
    with hj.HashJoinContext(0) as c:
        for step, (rel, flag, fmt, cause) in enumerate(((uniform, True, 2, 0), (over, True, 0, CODE_OVERFLOW), (uniform, True, 2, 0),
                                                        (uniform, False, 1, 0), (over, False, 1, 0), (uniform, True, 2, 0))):
            S = np.concatenate([oracle.relS_for("uniform", rel), probe_side(rel), [U64(40 * T + 77)]])
            want = oracle.build_probe_seq(rel, S, 4, want_table=True)
            got, table, info = build_probe(c, rel, S, slot_codes=flag)
            check_exact(got, table, want, step)
            assert got["buildVariant"] == 3 and got["compactFallback"] == 0, step
            assert (info["tableFormat"], info["cause"], info["codes"], info["road"]) == (fmt, cause, fmt == 2, 2 if flag else 0), (step, info)
            assert c.table_debug()["tableFormat"] == fmt
            assert c.wave_planar_info() == {"planar": fmt == 1, "planarFallback": cause, "tableFormat": fmt}, step


@gpu
def test_log_overflow_stays_a_cause(ctx):
    """the rings forced onto `shuffle` (no locality: nearly every tuple is deferred, the dirty logs cannot fit): the planar
    build's own hand-over, cause 1, on this road too; the 8-byte build redoes the table, exact"""
    n = 1 << 16
    rel = oracle.generate_data("shuffle", n, n, 16)
    S = probe_side(rel)
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    got, table, info = build_probe(ctx, rel, S)
    check_exact(got, table, want, "shuffle")
    assert got["buildVariant"] == 3 and got["buildDeferred"] > n // 2
    assert (info["codes"], info["cause"], info["road"], info["tableFormat"]) == (False, LOG_OVERFLOW, 2, 0), info


@gpu
def test_flag_is_refused_where_no_code_plane_exists(ctx):
    for kw in (dict(algo="atomic", keepRowIds=True), dict(algo="htm"), dict(algo="prj"), dict(algo="atomic", probeLength=129)):
        algo = kw.pop("algo")
        with pytest.raises(hj.HashJoinError):
            ctx.reserve(algo, N, N, slotCodes=True, **kw)
    ctx.reserve("nocc", N, N, slotCodes=True, probeLength=128)


# ---- the size rule: host arithmetic, no device --------------------------------------------------------------------------------
def test_auto_rule():
    """(32 - log2(tableSize)) + ceil(log2(probeLength)) <= 7"""
    for probe, no, yes in ((4, 26, 27), (8, 27, 28), (3, 26, 27), (2, 25, 26), (1, 24, 25), (16, 28, 29)):
        assert not hj.slot_codes_info(1 << no, probe)["fitsAuto"], (probe, no)
        assert hj.slot_codes_info(1 << yes, probe)["fitsAuto"], (probe, yes)
    top = hj.slot_codes_info(1 << 32, 4)
    assert top["fitsAuto"] and (top["tableBits"], top["dbits"], top["hiCap"]) == (32, 2, 32)
    assert hj.slot_codes_info(1 << 32, 128)["fitsAuto"] and not hj.slot_codes_info(1 << 32, 129)["fitsAuto"]
    assert hj.slot_codes_info(1 << 30, 4) == {"fitsAuto": True, "dbits": 2, "hiCap": 32, "tableBits": 30, "codes": False, "cause": 0,
                                              "road": 0, "tableFormat": 0}
    for bad in ((0, 4), (3 << 20, 4), (1 << 33, 4), (1 << 20, 0)):
        with pytest.raises(hj.HashJoinError):
            hj.slot_codes_info(*bad)


def test_code_round_trip_restated():
    """the format as the header states it, in numpy: every key with hi < hiCap placed d < probeLength slots above its home
    decodes to itself, no code reaches 0x80, and keys that differ only above the table size get different codes"""
    rng = np.random.default_rng(5)
    for bits, probe in ((15, 4), (27, 4), (28, 8), (32, 4), (20, 1), (16, 3)):
        info = hj.slot_codes_info(1 << bits, probe)
        dbits, cap, mask = info["dbits"], info["hiCap"], (1 << bits) - 1
        hi = rng.integers(0, min(cap, 1 << (32 - bits)), 4096)
        home = rng.integers(0, 1 << bits, 4096)
        d = rng.integers(0, probe, 4096)
        key = (hi << bits) | home
        slot = (home + d) & mask
        code = (hi << dbits) | ((slot - home) & mask)
        assert code.max() < 0x80 and ((slot - home) & mask).max() < 1 << dbits
        back = ((slot - (code & ((1 << dbits) - 1))) & mask) | ((code >> dbits) << bits)
        assert np.array_equal(back, key), (bits, probe)
