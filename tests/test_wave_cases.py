"""The directed seam cases of the ring builds (tests/wave_cases.py), checked without a GPU: every constructor must produce the
property it is named for -- judged from the restated pre-pass (expected_seams), the host-only layout call
(hj_wave_layout_info) and the sequential oracle, not from a device run. test_gpu_wave_seams.py then runs the same table on
the device and may rely on all of it."""
import ctypes

import numpy as np
import pytest

import htm_hashjoin_amd as hj
import wave_cases as wc
from oracle import oracle

N = 1 << 16
CU_COUNTS = (256, 64)


@pytest.fixture(scope="module", params=CU_COUNTS)
def world(request):
    """layout, cases, base seams and base oracle tables for one compute-unit count"""
    lay = wc.layout(N, request.param)
    base = {}
    for name, f in wc.BASES.items():
        rel = wc.relation(f(N))
        base[name] = {"rel": rel, "seams": wc.expected_seams(rel, lay, 2 * N),
                      "want": {p: oracle.build_probe_seq(rel, None, p, want_table=True) for p in (1, 4)}}
    return {"lay": lay, "cases": wc.cases(N, lay), "base": base}


def test_layout_call_is_pinned():
    """chunk length: a multiple of the tile, at least four tiles, the chunks cover the relation; the zones are the kernel's:
    shadow + overlap = one tile, the shadow reaches back past look + tail, a seam moves by less than the shortest chunk"""
    for cu in (1, 64, 104, 256, 304):
        for n in (1, 2047, 2048, 2049, 1 << 15, 1 << 16, (1 << 16) + 1, 1 << 20, 1 << 22, (1 << 27) + 5, 1 << 30, (1 << 32) - 1):
            lay = wc.layout(n, cu)
            assert lay["computeUnits"] == cu
            assert lay["chunkLen"] % lay["tileTuples"] == 0 and lay["chunkLen"] >= 4 * lay["tileTuples"]
            assert lay["nChunks"] * lay["chunkLen"] >= n > (lay["nChunks"] - 1) * lay["chunkLen"]
            assert lay["nChunks"] <= 16 * 8 * cu or lay["chunkLen"] == 4 * lay["tileTuples"]
            assert lay["sliceLen"] == lay["chunkLen"] + lay["look"] + lay["overlap"]
            assert lay["shadow"] + lay["overlap"] == lay["tileTuples"]
            assert lay["shadow"] >= lay["look"] + lay["tail"]
            assert lay["look"] + lay["overlap"] < 4 * lay["tileTuples"]
            assert lay["crosserCap"] <= lay["sliceLen"] and lay["compactMaxProbeLength"] < lay["granuleSlots"]
            assert lay["ringGranules"] * lay["granuleSlots"] >= 2 * lay["tileTuples"]
    assert wc.layout(0, 256)["nChunks"] == 0
    # 2^16 tuples are 32 chunks on any device, 2^22 more chunks than one workgroup of the bounds scan takes
    assert wc.layout(1 << 16, 256)["nChunks"] == 32 and wc.layout(1 << 15, 256)["nChunks"] == 16
    assert wc.layout(1 << 20, 256)["nChunks"] > 256 and wc.layout(1 << 22, 256)["nChunks"] > 256
    out = (ctypes.c_uint64 * 16)()
    assert hj.lib.hj_wave_layout_info(None, 0, 1 << 16, out) == hj.HJ_ERR_INVALID          # neither a context nor a count
    assert hj.lib.hj_wave_layout_info(None, 256, 1 << 32, out) == hj.HJ_ERR_INVALID
    assert hj.lib.hj_wave_layout_info(None, 256, 1 << 16, None) == hj.HJ_ERR_INVALID


def test_expected_seams_by_hand():
    """the restatement on relations small enough to follow by hand (granule 128, look 256, chunk 2048)"""
    lay = wc.layout(3 * 2048, 256)
    assert (lay["chunkLen"], lay["nChunks"], lay["granuleSlots"], lay["look"]) == (2048, 3, 128, 256)
    T = 1 << 14
    # dense keys 1 .. n: the seam sits where the home slots cross into the next granule, 127 positions on
    starts, bounds = wc.expected_seams(np.arange(1, 3 * 2048 + 1, dtype=np.uint64), lay, T)
    assert starts.tolist() == [0, 2048 + 127, 4096 + 127, 6144] and bounds.tolist() == [0, 17, 33, T // 128]
    # one key everywhere: no crossing inside the look, every seam stays nominal and every range starts in the same granule
    starts, bounds = wc.expected_seams(np.full(3 * 2048, 300, dtype=np.uint64), lay, T)
    assert starts.tolist() == [0, 2048, 4096, 6144] and bounds.tolist() == [2, 2, 2, T // 128]
    # a crossing at the look's last position counts, one position later does not
    rel = np.full(3 * 2048, 300, dtype=np.uint64)
    rel[2048 + 255] = 384
    rel[4096 + 256] = 384
    starts, bounds = wc.expected_seams(rel, lay, T)
    assert starts.tolist() == [0, 2048 + 255, 4096, 6144] and bounds.tolist() == [2, 3, 3, T // 128]
    # invalid tuples (payload bits, key 0) are no samples: a chunk without one inherits, leading ones take the first valid one's
    rel = np.arange(1, 3 * 2048 + 1, dtype=np.uint64)
    rel[:64] = 0
    rel[2048:2048 + 64] |= np.uint64(1) << np.uint64(40)
    starts, bounds = wc.expected_seams(rel, lay, T)
    assert starts.tolist() == [0, 2048, 4096 + 127, 6144] and bounds.tolist() == [33, 33, 33, T // 128]
    rel[4096:4096 + 64] = 0
    assert wc.expected_seams(rel, lay, T)[1].tolist() == [0, 0, 0, T // 128]
    # the prefix maximum: a sample below its predecessors' does not pull the range back
    rel = np.arange(1, 3 * 2048 + 1, dtype=np.uint64)
    rel[4096:] = 5
    assert wc.expected_seams(rel, lay, T)[1].tolist() == [0, 17, 17, T // 128]
    # homes in the table's last granule: the slot after it is the table's end, nothing reaches it, the seam stays nominal
    rel = np.arange(1, 3 * 2048 + 1, dtype=np.uint64)
    rel[4096:] = T - 5
    starts, bounds = wc.expected_seams(rel, lay, T)
    assert starts.tolist() == [0, 2048 + 127, 4096, 6144] and bounds.tolist() == [0, 17, T // 128 - 1, T // 128]
    # ... and with a table of 2^32 slots that slot is 2^32 = 0 in 32 bits: no crossing either
    rel = np.arange(1, 3 * 2048 + 1, dtype=np.uint64)
    rel[2048:] = 0xFFFFFFF0
    starts, bounds = wc.expected_seams(rel, lay, 1 << 32)
    assert starts.tolist() == [0, 2048, 4096, 6144] and bounds.tolist() == [0, (1 << 25) - 1, (1 << 25) - 1, 1 << 25]
    # a last chunk shorter than the look starts at the relation's end and owns the table behind its tuples' highest home
    for r, short in ((1, True), (255, True), (256, False), (257, False)):
        n = 2 * 2048 + r
        lay2 = wc.layout(n, 256)
        starts, bounds = wc.expected_seams(np.arange(1, n + 1, dtype=np.uint64), lay2, T)
        if short:
            assert starts.tolist() == [0, 2048 + 127, n, n] and bounds.tolist() == [0, 17, n // 128 + 1, T // 128]
        else:
            assert starts.tolist() == [0, 2048 + 127, 4096 + 127, n] and bounds.tolist() == [0, 17, 33, T // 128]


def test_bases_are_what_they_claim(world):
    lay, base = world["lay"], world["base"]
    for name, b in base.items():
        home, valid = wc.homes_of(b["rel"], 2 * N)
        assert valid.all() and (np.diff(home) > 0).all(), name            # sorted, unique
        for p in (1, 4):
            assert b["want"][p]["conflicts"] == 0
            assert np.array_equal(np.flatnonzero(b["want"][p]["table"]), home)      # every tuple at its home slot
        starts, bounds = b["seams"]
        for c in range(1, lay["nChunks"]):
            sm = wc.seam_of(starts, bounds, lay, c)
            assert sm.p < sm.q < sm.p + lay["look"] and home[sm.q - 1] == sm.L - 1 and home[sm.q] >= sm.L
    assert wc.homes_of(base["dense"]["rel"], 2 * N)[0][-1] == N
    assert wc.homes_of(base["odd"]["rel"], 2 * N)[0][-1] == 2 * N - 1             # the whole table
    g = wc.homes_of(base["odd"]["rel"], 2 * N)[0] // lay["granuleSlots"]
    assert (np.bincount(g) == 64).all()


def _ring_holds(home, starts, lay, c, pos, slot):
    """would chunk c's ring hold `slot` while the tile that contains position pos is inserted: the ring never moves past the
    lowest home slot of the tile, and spans ringGranules granules from there"""
    shadow = min(lay["shadow"], int(starts[c])) if c else 0
    first = int(starts[c]) - shadow
    lo = first + (pos - first) // lay["tileTuples"] * lay["tileTuples"]
    gmin = int(home[lo:lo + lay["tileTuples"]].min()) // lay["granuleSlots"]
    return 0 <= slot // lay["granuleSlots"] - gmin < lay["ringGranules"]


def test_every_case_keeps_its_seams_and_sits_where_it_says(world):
    lay, base = world["lay"], world["base"]
    seen = set()
    for case in world["cases"]:
        rel = wc.relation(case.homes, case.shift)
        b = base[case.base]
        starts, bounds = wc.expected_seams(rel, lay, 2 * N, case.shift)
        assert np.array_equal(starts, b["seams"][0]) and np.array_equal(bounds, b["seams"][1]), case.name
        sm = case.seam
        assert sm == wc.seam_of(starts, bounds, lay, sm.c) and sm.c in wc.seams_to_test(lay)
        home, valid = wc.homes_of(rel, 2 * N, case.shift)
        assert valid.all() and np.array_equal(home, case.homes)
        changed = np.flatnonzero(home != wc.homes_of(b["rel"], 2 * N)[0])
        assert set(changed.tolist()) <= set(case.moved) and home.size == N
        prev = sm.c - 1
        if case.family in ("A", "A1"):
            k = len(case.moved)
            assert case.moved == list(range(sm.q - k, sm.q)) and (home[case.moved] == sm.L - 1).all()
            assert int(np.count_nonzero(home == sm.L - 1)) == k and k <= lay["shadow"]
            # the previous wavefront has every copy in its ring; the next one reads them all
            assert all(_ring_holds(home, starts, lay, prev, q, sm.L - 1) for q in (case.moved[0], case.moved[-1])), case.name
        elif case.family in ("B", "R"):
            dist = sm.q - case.moved[0]
            assert dist in (lay["shadow"], lay["shadow"] + 1) and home[case.moved[0]] == sm.L - 1
            assert (dist == lay["shadow"]) == (case.cause == 0 or case.family == "R")
            assert int(np.count_nonzero(home == sm.L - 1)) == 2
            assert _ring_holds(home, starts, lay, prev, case.moved[0], sm.L - 1), case.name
        elif case.family == "C":
            dist = case.moved[0] - sm.q
            assert dist in (lay["overlap"] - 1, lay["overlap"]) and (dist == lay["overlap"] - 1) == (case.cause == 0)
            assert sm.L - lay["granuleSlots"] <= home[case.moved[0]] < sm.L
            assert not (wc.homes_of(b["rel"], 2 * N)[0] == home[case.moved[0]]).any()          # a free slot: nothing is displaced
            assert _ring_holds(home, starts, lay, prev, case.moved[0], int(home[case.moved[0]])) or case.cause
        elif case.family == "H":
            # chunk c's own tail zone starts here: the tile holds a zone edge, so it is no full tile
            assert case.moved[0] == (sm.c + 1) * lay["chunkLen"] - lay["tail"] and sm.c + 1 < lay["nChunks"]
            assert sm.q + lay["overlap"] <= case.moved[0] < starts[sm.c + 1]
            assert sm.L - lay["granuleSlots"] <= home[case.moved[0]] < sm.L
            assert not (wc.homes_of(b["rel"], 2 * N)[0] == home[case.moved[0]]).any()
        elif case.family == "D":
            dist = sm.p - case.moved[0]
            assert dist in (lay["tail"], lay["tail"] + 1) and (dist == lay["tail"]) == (case.cause == 0)
            assert home[case.moved[0]] in (sm.L, sm.L + 5)
            assert case.moved[0] >= sm.q - lay["shadow"]                                        # the next wavefront reads it
        seen.add((case.family, case.base, sm.c, case.cause))
    first, middle, last = wc.seams_to_test(lay)
    for c in (first, middle, last):
        for fam, bases, causes in (("A", ("gapped",), (0, wc.BIT_CROSSERS)), ("B", ("gapped",), (0, wc.BIT_SEAM)),
                                   ("C", ("gapped", "odd"), (0, wc.BIT_OUTSIDE)), ("D", ("gapped", "odd"), (0, wc.BIT_OUTSIDE))):
            for bname in bases:
                for cause in causes:
                    assert (fam, bname, c, cause) in seen, (fam, bname, c, cause)
    assert ("A", "odd", middle, wc.BIT_CROSSERS) in seen and ("A", "odd", last, 0) in seen
    assert ("R", "dense", middle, wc.BIT_SEAM) in seen and ("A1", "gapped", first, 0) in seen
    assert all(("H", bname, c, wc.BIT_BELOW) in seen for bname in ("gapped", "odd") for c in (first, middle))


def test_case_a_crosses_exactly_as_often_as_it_says(world):
    """the oracle's table: exactly k - 1 tuples homed below L sit at or beyond L or were dropped after trying a slot there;
    and whatever the walks displace is back in place a granule before the next seam's range (nothing enters the next
    shadow granule from below)"""
    lay, base = world["lay"], world["base"]
    checked = 0
    for case in world["cases"]:
        if case.family not in ("A", "A1", "B") or case.probe > lay["compactMaxProbeLength"]:
            continue
        rel = wc.relation(case.homes, case.shift)
        want = oracle.build_probe_seq_ts(rel, None, 2 * N, case.shift, case.probe, want_table=True)
        sm = case.seam
        n_cross = wc.crossers_in_table(want["table"], rel, 2 * N, case.shift, sm.L, case.probe)
        if case.family == "B":
            assert n_cross == 1, case.name                     # the base's own tuple walks: seen or not is the wavefront's matter
        else:
            assert n_cross == case.crossing == (len(case.moved) - 1 if case.probe > 1 else 0), case.name
        starts, bounds = base[case.base]["seams"]
        if sm.c + 1 < lay["nChunks"]:
            calm = int(bounds[sm.c + 1] - 1) * lay["granuleSlots"]
            ref = base[case.base]["want"][4]["table"]
            got = want["table"] if case.shift == 0 else want["table"] >> np.uint64(case.shift)
            assert np.array_equal(got[calm:], ref[calm:]), case.name
        checked += 1
    assert checked > 40


def test_ripple_case_reaches_the_next_seam(world):
    """case R: on the dense base one displaced tuple displaces every later one -- the next seam is crossed by a walk whose
    cause lies a whole chunk back"""
    lay, base = world["lay"], world["base"]
    (case,) = [c for c in world["cases"] if c.family == "R"]
    want = oracle.build_probe_seq(wc.relation(case.homes), None, case.probe, want_table=True)
    nxt = wc.seam_of(*base["dense"]["seams"], lay, case.seam.c + 1)
    assert wc.crossers_in_table(want["table"], wc.relation(case.homes), 2 * N, 0, case.seam.L, case.probe) == 1
    assert wc.crossers_in_table(want["table"], wc.relation(case.homes), 2 * N, 0, nxt.L, case.probe) == 1
    assert want["conflicts"] == 0


def test_case_e_f_g_and_the_last_granule(world):
    lay = world["lay"]
    for twin in (False, True):
        rel = wc.empty_pattern(N, twin)
        home, valid = wc.homes_of(rel, 2 * N)
        assert valid.all() and int(rel[-1]) == 0xFFFFFFFF - twin and (np.diff(home) == 1).all()
        assert home[-1] == 2 * N - 1 - twin
    h = wc.run_over_chunks(N, lay)
    starts, bounds = wc.expected_seams(wc.relation(h), lay, 2 * N)
    run = np.flatnonzero(h == h[5 * lay["chunkLen"] + 37])
    assert run.size == 2 * lay["chunkLen"] + 100
    c0 = int(run[0]) // lay["chunkLen"]
    # the chunk the run starts in and the next one see no crossing inside their look: nominal seams, and the first of the
    # two owns an empty range; the chunk the run ends in starts where it ends
    assert starts[c0] == c0 * lay["chunkLen"] and starts[c0 + 1] == (c0 + 1) * lay["chunkLen"]
    assert bounds[c0] == bounds[c0 + 1] and starts[c0 + 2] == run[-1] + 1 and bounds[c0 + 2] == bounds[c0] + 1
    h = wc.last_granule(N, lay)
    starts, bounds = wc.expected_seams(wc.relation(h), lay, 2 * N)
    assert starts[-2] == (lay["nChunks"] - 1) * lay["chunkLen"] and bounds[-2] == bounds[-1] - 1
    for m in wc.short_last_chunk_sizes(lay):
        lay_m = wc.layout(m, lay["computeUnits"])
        starts, bounds = wc.expected_seams(np.arange(1, m + 1, dtype=np.uint64), lay_m, 1 << 16)
        assert lay_m["nChunks"] == 9
        assert (starts[-2] == m) == (m - 8 * lay_m["chunkLen"] < lay["look"])
