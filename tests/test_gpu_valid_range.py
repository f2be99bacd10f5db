"""The valid slot range of the LDS builds, seen by every reader of the table (hj_common.h, Counters): a context first builds a
POISON relation that leaves a key on every slot outside a band, then builds R -- whose home slots are that band -- through
the path under test, which writes only [validLo, validHiEx + 512). What lies outside is then really stale (asserted on the
raw table words, hj_table_debug + hj_copy_d2h), the probe side asks for every stale key and for keys homed at the edges of
the range the device reported, and every reader -- counting probe, checksums, exports, the four join kinds of the pairs
probe, the R-side match marks -- must give what the sequential oracle gives for R ALONE. Relations: valid_range_cases.py;
pair, kind and mark references: join_kinds_common.py, r_marks_common.py. Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import Device
import r_marks_common as rm
import valid_range_cases as vc
from join_kinds_common import INNER, LEFT, KINDS, NO_ROW, Calls, derive
from oracle import oracle

pytestmark = pytest.mark.gpu

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
EMPTY = U64(0xFFFFFFFFFFFFFFFF)
SLACK = 16                                  # kTableSlack: 8-byte words behind the table
INDEX_GAP = 32                              # kPlanarIndexGap: 4-byte words between the key plane and the index plane
SMALL, LARGE = 1 << 16, 1 << 18             # the smallest sizes at which every LDS build runs with more than one chunk

# name -> how R is built: entry point, buildVariant, keepRowIds (packed slots, pairs and marks), home shift
PATHS = {
    "atomic2": dict(entry="atomic", variant=2, keep=True),
    "atomic3_packed": dict(entry="atomic", variant=3, keep=True),
    "atomic3_planar": dict(entry="atomic", variant=3, keep=False),
    "atomic4": dict(entry="atomic", variant=4, keep=False),
    "atomic0": dict(entry="atomic", variant=0, keep=False),
    "keys2": dict(entry="keys", variant=2, shift=0),
    "keys3": dict(entry="keys", variant=3, shift=0),
    "keys4": dict(entry="keys", variant=4, shift=0),
    "keys2_shift3": dict(entry="keys", variant=2, shift=3),
    "keys3_shift3": dict(entry="keys", variant=3, shift=3),
    "keys4_shift3": dict(entry="keys", variant=4, shift=3),
    "htm2": dict(entry="htm", variant=2),
    "htm3": dict(entry="htm", variant=3),
    "htm0": dict(entry="htm", variant=0),
}
CONTROLS = {"atomic1": dict(entry="atomic", variant=1, keep=True), "htm1": dict(entry="htm", variant=1)}
PLACEMENTS = ("control", "mid", "below", "above", "straddle")


def band_for(path, n, a, copies=1, shuffle=16):
    p = {**PATHS, **CONTROLS}[path]
    htm = p["entry"] == "htm"
    T = vc.htm_table(n) if htm else 2 * n
    return vc.band_relation(n, T, a, copies=copies, shuffle=shuffle, shift=p.get("shift", 0), htm=htm)


def read_raw(c, dbg):
    """the whole table buffer as the device holds it: tableSlots + slack 8-byte words"""
    raw = np.empty(dbg["tableSlots"] + SLACK, dtype=U64)
    assert dbg["tableBytes"] >= raw.nbytes, dbg
    c.copy_d2h(raw, dbg["tableAddr"])
    return raw


def build_poison(c, dev, band, kind, n):
    """step 1 and 2: the poison alone makes the whole table valid and leaves a key on each of its slots -> (P, raw words)"""
    T = band.table
    if kind == "htm":
        P = vc.poison_for(band, "perm", htm=True)
        c.reserve("htm", max(n, P.size), 0, buildVariant=1)
        c.build(dev.put(P), P.size)
    else:
        P = vc.poison_for(band, "perm" if kind == "packed" else "sorted", htm=False)
        if band.htm:
            # Open-addressing slots under a bucketised R: a bucket reader would take the index word of every fourth stale
            # slot for a chain link. Those tuples go first, so their indices stay inside the overflow area that a chain
            # poison, built before, has made the context allocate: a reader that lost its range test then walks stale
            # buckets and reports wrong numbers, it does not read outside the context's buffers.
            Q = vc.poison_for(band, "perm", htm=True)
            c.reserve("htm", max(n, Q.size), 0, buildVariant=1)
            c.build(dev.put(Q), Q.size)
            links = (vc.homes(P, T) & U64(3)) == U64(3)
            assert int(links.sum()) < c.fetch()["conflicts"], ("the overflow area is smaller than the stale link words reach", kind)
            P = np.ascontiguousarray(np.concatenate([P[links], P[~links]]))
        shift = 0 if band.htm else band.shift
        c.reserve("atomic", n, 0, buildVariant=1 if kind == "packed" else 4)
        c.build_keys(dev.put(P.astype(np.uint32)), P.size, shift, T)
    dbg = c.table_debug()
    got = c.fetch()
    tag = ("poison", kind, P.size, dbg, got["buildVariant"], got["compactFallback"])
    assert (dbg["validLo"], dbg["validHiEx"], dbg["tableSlots"]) == (0, T, T), ("vacuous: the poison does not cover the table", tag)
    assert dbg["tableFormat"] == (1 if kind == "compact" else 0), ("vacuous: the poison is not in the format the case is about", tag)
    assert kind == "htm" or got["conflicts"] == 0, tag
    raw = read_raw(c, dbg)
    u = np.unique(P)
    if kind == "htm":
        h = vc.homes(u, T, htm=True).astype(np.int64)
        landed = np.zeros(u.size, dtype=bool)
        for j in range(3):
            landed |= (raw[h + j] != EMPTY) & ((raw[h + j] & M32) == u)
        linked = int((raw[np.unique(h) + 3] != EMPTY).sum())
        assert landed.all() and linked > 0 and got["htmOverflowBuckets"] >= linked, ("vacuous: no stale overflow chains", tag, linked)
    else:
        h = vc.homes(u, T, 0 if band.htm else band.shift).astype(np.int64)
        words = raw[:T] & M32 if kind == "packed" else raw.view(np.uint32)[:T].astype(U64)
        assert np.array_equal(words[h], u), ("vacuous: a poison key is not on its home slot", tag)
    return P, raw


def build_r(c, dev, band, path, probe, idx_base):
    p = {**PATHS, **CONTROLS}[path]
    entry, keep = p["entry"], bool(p.get("keep"))
    if entry == "htm":
        c.reserve("htm", band.n, 0, buildVariant=p["variant"], trackRMatches=True)
        c.build(dev.put(band.R), band.n, idx_base)
    elif entry == "atomic":
        c.reserve("atomic", band.n, 0, buildVariant=p["variant"], probeLength=probe, keepRowIds=keep, trackRMatches=keep)
        c.build(dev.put(band.R), band.n, idx_base)
    else:
        assert idx_base == 0
        c.reserve("atomic", band.n, 0, buildVariant=p["variant"], probeLength=probe)
        c.build_keys(dev.put(band.R.astype(np.uint32)), band.n, band.shift, band.table)


def range_class(dbg):
    lo, hi, T = dbg["validLo"], dbg["validHiEx"], dbg["tableSlots"]
    if (lo, hi) == (0, T):
        return "whole"
    if hi + vc.BLOCK < T:
        return "interior" if lo > 0 else "control"
    return "other"                              # a top that reaches the last block without the whole table: never legal


def assert_stale_outside(raw0, raw1, dbg, P, poison, band, tag):
    """the words outside [validLo, validHiEx + 512) are byte for byte the poison build's -- and poison keys live there"""
    T, lo, top = dbg["tableSlots"], dbg["validLo"], min(dbg["tableSlots"], dbg["validHiEx"] + vc.BLOCK)
    out = np.ones(T, dtype=bool)
    out[lo:top] = False
    if dbg["tableFormat"] == 0:
        same = np.array_equal(raw1[:T][out], raw0[:T][out])
    else:                                       # 4-byte keys, and (planar) the index plane behind them
        a, b = raw0.view(np.uint32), raw1.view(np.uint32)
        same = np.array_equal(b[:T][out], a[:T][out]) and np.array_equal(b[T + INDEX_GAP:2 * T + INDEX_GAP][out], a[T + INDEX_GAP:2 * T + INDEX_GAP][out])
    assert same, ("vacuous: the build wrote outside the range it reports", tag)
    hp = vc.homes(P, T, 0 if (poison != "htm" and band.htm) else band.shift, poison == "htm").astype(np.int64)
    stale = int(out[hp].sum())
    assert stale > 0 and not np.array_equal(raw0[:T], raw1[:T]), ("vacuous: no stale key outside the range", tag)
    return stale


def check_counting_readers(c, dev, band, S, want, path, placement, tag):
    """counting probe, checksums and the export, against the oracle of R alone -> the device pointer of S"""
    p = {**PATHS, **CONTROLS}[path]
    T = band.table
    if p["entry"] == "keys":
        dS = dev.put(S.astype(np.uint32))
        c.probe_keys(dS, S.size)
    else:
        dS = dev.put(S)
        c.probe(dS, S.size)
    c.checksums()
    got = c.fetch()
    if band.htm:
        assert (got["conflicts"], got["conflictSum"], got["totalMatches"], got["inputSum"], got["tableSumFull"],
                got["htmOverflowBuckets"], got["htmOverflowSum"], got["outputSum"]) == (
            want["conflictCount"], want["conflictSum"], want["totalMatches"], want["inputSum"], want["bucketSum"],
            want["overflowBuckets"], want["overflowSum"], want["outputSum"]), (tag, got, want)
        buckets, overflows = c.export_buckets(want["numBuckets"])
        assert np.array_equal(buckets["tuples"], want["buckets"]["tuples"]) and np.array_equal(buckets["count"], want["buckets"]["count"]), tag
        key = lambda o: np.sort(o[1:].view(U64).reshape(-1, 4)[:, :3].sum(axis=1))          # noqa: E731
        assert overflows.size == want["overflows"].size and np.array_equal(key(overflows), key(want["overflows"])), tag
        if band.n <= SMALL:                                   # every chain in walk order
            a, ao = oracle.htm_chains(buckets, overflows)
            b, bo = oracle.htm_chains(want["buckets"], want["overflows"])
            assert np.array_equal(ao, bo) and np.array_equal(a, b), tag
    else:
        half, full = int(want["table"][:T // 2].sum()), int(want["table"].sum())
        assert full == want["tableSumFull"]
        print(tag, "matches", got["totalMatches"], want["totalMatches"], "half", got["tableSumHalf"], half, "full", got["tableSumFull"], full)
        for k in ("conflicts", "totalMatches", "inputSum", "conflictSum", "tableSumFull"):
            assert got[k] == want[k], (tag, k, got[k], want[k])
        assert got["tableSumHalf"] == half and got["outputSum"] == full + want["conflictSum"], (tag, got["tableSumHalf"], half)
        if placement == "below":
            assert got["tableSumHalf"] == got["tableSumFull"] > 0, tag
        if placement == "above":
            assert got["tableSumHalf"] == 0 < got["tableSumFull"], tag
        assert np.array_equal(c.export_table(T), want["table"]), tag
    return dS, got


def check_pairs_and_marks(c, dev, band, S, dS, want, probe, idx_base, tag):
    """probe_pairs for the four kinds as sets, pairs_info()'s unmatched count (Calls.call), and the R rows matched and
    unmatched after the INNER call"""
    inner = rm.inner_expected("htm" if band.htm else "atomic", band.R, S, probe, r_base=idx_base)
    assert inner.size == want["totalMatches"], (tag, inner.size, want["totalMatches"])
    calls = Calls(c, dev)
    calls.matches, calls.s = want["totalMatches"], S.size           # the counting probe came first
    marks = rm.Marks(c, dev, band.n, idx_base)
    for kind in KINDS:
        calls.call(kind, dS, S.size, inner, tag=tag)
        if kind == INNER:
            marks.add(inner)
            marks.check(tag)
    return inner


def run_case(path, band, placement, want_class, probe=4, poison=None, idx_base=0):
    """The common procedure on one context: poison, raw table, R through `path`, table_debug and raw table again, probe.
    want_class: "interior" | "whole" | "control" (asserted), or "device" (the sweeps: returned). -> (class, tag)"""
    p = {**PATHS, **CONTROLS}[path]
    poison = poison or ("htm" if band.htm else "packed")
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        P, raw0 = build_poison(c, dev, band, poison, band.n)
        build_r(c, dev, band, path, probe, idx_base)
        dbg = c.table_debug()
        raw1 = read_raw(c, dbg)
        built = c.fetch()
        planar = None if band.htm else c.wave_planar_info()
        cls = range_class(dbg)
        tag = (path, placement, band.n, probe, poison, idx_base, "ran", built["buildVariant"], "fallback", built["compactFallback"],
               planar, "range", dbg["validLo"], dbg["validHiEx"], cls, "band", band.lo, band.hi_ex)
        print(tag)
        assert dbg["tableSlots"] == band.table, tag
        if want_class == "device":
            assert cls != "other", tag
        else:
            assert cls == want_class, ("vacuous: the range is not what the case was designed for", want_class, tag)
        if cls != "whole":
            assert dbg["validLo"] <= band.lo and band.hi_ex <= dbg["validHiEx"], tag
            stale = assert_stale_outside(raw0, raw1, dbg, P, poison, band, tag)
            tag += ("stale", stale)
        S = vc.probe_side(band, np.unique(P), dbg["validLo"], dbg["validHiEx"], key32=p["entry"] == "keys")
        want = vc.expected(band, S, probe)
        dS, _ = check_counting_readers(c, dev, band, S, want, path, placement, tag)
        if band.htm or p.get("keep"):
            check_pairs_and_marks(c, dev, band, S, dS, want, probe, idx_base, tag)
        return cls, tag, built, dbg, planar


# ---- hj_table_debug itself ------------------------------------------------------------------------------------------------
def test_table_debug_contract():
    n = 1 << 12
    R = np.arange(1, n + 1, dtype=U64)
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        with pytest.raises(hj.HashJoinError) as e:
            c.table_debug()
        assert e.value.status == -7                           # HJ_ERR_STATE before any build
        c.reserve("atomic", n, n, buildVariant=1)
        dR = dev.put(R)
        c.build(dR, n)
        c.probe(dR, n)
        c.checksums()
        before = c.fetch()
        dbg = c.table_debug()
        assert dbg == {"validLo": 0, "validHiEx": 2 * n, "tableFormat": 0, "tableSlots": 2 * n, "tableAddr": dbg["tableAddr"],
                       "tableBytes": (2 * n + SLACK) * 8}, dbg
        assert dbg["tableAddr"] != 0
        raw = read_raw(c, dbg)
        assert np.array_equal(raw[1:n + 1], (np.arange(n, dtype=U64) << U64(32)) | R) and (raw[n + 1:] == EMPTY).all() and raw[0] == EMPTY
        after = c.fetch()
        counters = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum", "outputSum", "sSize", "buildVariant")
        assert [before[k] for k in counters] == [after[k] for k in counters]      # read-only
        assert np.array_equal(c.export_table(2 * n)[1:n + 1], R)
        c.reserve("htm", n, n, buildVariant=1)
        c.build(dR, n)
        dbg = c.table_debug()
        assert (dbg["validLo"], dbg["validHiEx"], dbg["tableFormat"], dbg["tableSlots"]) == (0, vc.htm_table(n), 0, vc.htm_table(n)), dbg
        c.reserve("prj", n, n)
        c.prj_join(dR, n, dR, n)
        with pytest.raises(hj.HashJoinError) as e:
            c.table_debug()
        assert e.value.status == -7                           # a radix join leaves no table


# ---- the band placements, every path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n,probe", ((SMALL, 4), (LARGE, 8)), ids=("n16_probe4", "n18_probe8"))
def test_band_placements(n, probe, path, placement):
    """every build path on every placement, at both sizes; probeLength 8 on the open-addressing paths at the larger one"""
    a, copies = vc.placements(2 * n)[placement]
    band = band_for(path, n, a, copies)
    want_class = vc.classify(band, probe)
    assert want_class in ("interior", "whole", "control")
    run_case(path, band, placement, want_class, probe=probe)


@pytest.mark.parametrize("path", ("atomic2", "atomic3_packed", "keys3_shift3"))
def test_probe_length_8_at_the_smaller_size(path):
    for placement in ("control", "above"):
        a, copies = vc.placements(2 * SMALL)[placement]
        band = band_for(path, SMALL, a, copies)
        run_case(path, band, placement, vc.classify(band, 8), probe=8)


@pytest.mark.parametrize("path", CONTROLS)
def test_global_atomics_make_the_whole_table_valid_and_clear_the_poison(path):
    """buildVariant 1, the control: whatever the band, the range is the whole table and no stale key is left"""
    for placement in ("mid", "above"):
        a, copies = vc.placements(2 * SMALL)[placement]
        run_case(path, band_for(path, SMALL, a, copies), placement, "whole")


@pytest.mark.parametrize("path", ("atomic2", "atomic3_packed", "atomic3_planar", "atomic4", "htm3"))
def test_a_non_zero_idx_base(path):
    band = band_for(path, SMALL, vc.placements(2 * SMALL)["mid"][0])
    run_case(path, band, "mid", "interior", idx_base=1000003)


# ---- the sweeps across set_valid_range's switch and across block 0 ----------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_band_top_swept_over_the_last_six_blocks(path):
    """Each step is interior or whole and exact either way; the sweep crosses hiEx + 512 >= tableSize, so it shows both.
    Where arithmetic decides (valid_range_cases.classify: three blocks of room, or a top in the last block) it is asserted."""
    T = 2 * SMALL
    seen = []
    for a in vc.top_sweep(T, vc.band_slots(SMALL, 1, PATHS[path]["entry"] == "htm")):
        band = band_for(path, SMALL, a)
        cls, tag = run_case(path, band, "top_sweep", vc.classify(band))[:2]
        assert cls in ("interior", "whole"), tag
        seen.append(cls)
    print(path, seen)
    assert "interior" in seen and "whole" in seen, (path, seen)


@pytest.mark.parametrize("path", PATHS)
def test_band_bottom_swept_over_blocks_0_to_3(path):
    """The mirror: validLo is 0 while the band starts in block 0 and leaves 0 as the band moves up; exact either way."""
    seen = []
    for a in vc.bottom_sweep():
        band = band_for(path, SMALL, a)
        cls, tag = run_case(path, band, "bottom_sweep", vc.classify(band))[:2]
        assert cls in ("control", "interior"), tag
        seen.append(cls)
    print(path, seen)
    assert "control" in seen and "interior" in seen, (path, seen)


# ---- stale contents in another format -----------------------------------------------------------------------------------------
STALE = {
    # name: (path, placement, poison, table format R must leave)
    "packed_to_compact": ("atomic4", "mid", "packed", 1),
    "packed_to_planar": ("atomic3_planar", "mid", "packed", 1),
    "compact_to_window": ("atomic2", "mid", "compact", 0),
    "compact_to_packed_rings": ("atomic3_packed", "mid", "compact", 0),
    "compact_to_planar": ("atomic3_planar", "mid", "compact", 1),
    "compact_to_compact": ("atomic4", "mid", "compact", 1),
    "htm_chains_to_htm_rings": ("htm3", "below", "htm", 0),
    "htm_chains_to_htm_window": ("htm2", "above", "htm", 0),
    "atomic_to_htm_rings": ("htm3", "mid", "packed", 0),
    "atomic_to_htm_window": ("htm2", "below", "packed", 0),
    "htm_chains_to_atomic_window": ("atomic2", "mid", "htm", 0),
    "htm_chains_to_atomic_rings": ("atomic3_packed", "mid", "htm", 0),
    "htm_chains_to_atomic_planar": ("atomic3_planar", "mid", "htm", 1),
}


@pytest.mark.parametrize("case", STALE)
def test_stale_contents_of_another_format(case):
    path, placement, poison, fmt = STALE[case]
    a, copies = vc.placements(2 * SMALL)[placement]
    band = band_for(path, SMALL, a, copies)
    cls, tag, built, dbg, planar = run_case(path, band, placement, "interior", poison=poison)
    assert dbg["tableFormat"] == fmt, ("vacuous: R is not in the format the case is about", tag)
    if case.endswith("planar"):
        assert planar["planar"], ("vacuous: the planar build handed over", tag)
    if case.startswith("htm_chains_to_htm"):
        assert built["htmOverflowBuckets"] > 0, ("vacuous: R reuses no overflow bucket", tag)


# ---- the wrapper, end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table_path", ("htm", "atomic", "nocc"))
def test_full_outer_join_tables_on_an_interior_band(table_path):
    """join_tables(how="full") over an interior band: the left rows, then the R-only rows, payloads through the maps"""
    n = 1 << 14
    htm = table_path == "htm"
    T = vc.htm_table(n) if htm else 2 * n
    band = vc.band_relation(n, T, T // 4, shuffle=16, htm=htm)
    assert vc.classify(band) == "interior"
    P = vc.poison_for(band, "perm", chains=False)
    # without the first half of R: those rows (but for their duplicates) are R-only
    S = vc.probe_side(band, P[::4], (band.lo // vc.BLOCK) * vc.BLOCK, (band.hi_ex // vc.BLOCK + 2) * vc.BLOCK)[n // 2:]
    r_pay, s_pay = np.arange(n, dtype=np.uint32) * np.uint32(7) + np.uint32(1), np.arange(S.size, dtype=U64) + U64(5)
    out = hj.join_tables(band.R, S, r_cols={"v": r_pay}, s_cols={"w": s_pay}, how="full", path=table_path)
    inner = rm.inner_expected(table_path, band.R, S, 4)
    lone_r = rm.unmatched_r(inner, n)
    want = np.sort(np.concatenate([derive(LEFT, inner, S.size), (NO_ROW << U64(32)) | lone_r]))
    got = (out["s_idx"].astype(U64) << U64(32)) | out["r_idx"].astype(U64)
    assert got.size == want.size and np.array_equal(np.sort(got), want), (table_path, got.size, want.size)
    assert lone_r.size > 0 and inner.size > 0
    s_ok, r_ok = out["s_idx"] != hj.NO_ROW, out["r_idx"] != hj.NO_ROW
    assert np.array_equal(out["s_valid"], s_ok) and np.array_equal(out["r_valid"], r_ok)
    assert np.array_equal(out["s"]["w"][s_ok], s_pay[out["s_idx"][s_ok]]) and np.array_equal(out["r"]["v"][r_ok], r_pay[out["r_idx"][r_ok]])
    assert (out["s"]["w"][~s_ok] == 0).all() and (out["r"]["v"][~r_ok] == 0).all()
