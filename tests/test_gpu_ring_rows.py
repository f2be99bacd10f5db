"""The ring build on the slot-code road issues a tile's home-slot attempts and pushes its rows in two batches of four rows
(hj_build_wave.hip, kWvWordRows): rows 0-3 -- the tile's first 256 positions -- are attempted and pushed, perhaps have a
round, and only then are rows 4-7 attempted. What can newly go wrong is that boundary inside a tile, and every case here puts
something on it: copies of one key on both sides, second-half tuples that walk into slots the first half holds (and the mirror
image), rounds between the halves, tiles whose positions end at the boundary, a seam zone across it. The harness is that of
test_gpu_ring_words.py: the forced road at N = 2^14 (tables of 2^15 slots, reserve(..., slotCodes=True), eight chunks of four
tiles), once the size rule's own road (2^27 slots); the road is asserted through slot_codes_info(); every expected value -- the
exported table slot for slot, conflicts, conflictSum, totalMatches, the sums -- is the sequential oracle's on the same arrays,
and a case about one cause first shows, from the oracle's table, the seams or the build's counters, that the cause happened.

Where a tile lies: on the odd base (homes 2i + 1, 64 tuples per granule) chunk c > 0 starts at position 2048 c + 64 and
chunk 0 at 0 (asserted from wave_seams()), so tile t of chunk c > 0 covers positions 2048 c + 64 + 512 t + [0, 512); row j of
a tile is its positions [64 j, 64 j + 64). Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import Device, ctx  # noqa: F401
import wave_cases as wc
from oracle import oracle

pytestmark = pytest.mark.gpu

U64 = np.uint64
I64 = np.int64
N = 1 << 14
T = 2 * N
CHUNK, TILE, ROW, HALF = 2048, 512, 64, 256
COUNTERS = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum")
PROBES = (1, 2, 3, 4, 8)


def build_probe(c, rel, S, probe, variant=3):
    """one build + probe + checksums through the split API -> (result, exported table, slot_codes_info, starts)"""
    c.reserve("atomic", rel.size, S.size, probeLength=probe, buildVariant=variant, slotCodes=True)
    with Device(c) as dev:
        c.build(dev.put(np.ascontiguousarray(rel, dtype=U64)), rel.size)
        c.probe(dev.put(np.ascontiguousarray(S, dtype=U64)), S.size)
        c.checksums()
        got = c.fetch()
        starts = c.wave_seams()[0].astype(I64) if got["buildVariant"] == 3 else None
        return got, c.export_table(2 * rel.size), c.slot_codes_info(), starts


def check_exact(got, table, want, tag):
    for k in COUNTERS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert got["outputSum"] == want["outputSumAtomic"], tag
    assert np.array_equal(table, want["table"]), tag


def check_codes(got, info, tag, road=2):
    assert (got["buildVariant"], got["compactFallback"]) == (3, 0), tag
    assert (info["codes"], info["cause"], info["road"], info["tableFormat"]) == (True, 0, road, 2), (tag, info)


def probe_side(rel):
    """every third tuple, and keys on the same home slots that the relation does not hold (other high bits)"""
    return np.concatenate([rel[::3], rel[:64] + U64(7 * T)])


def run_case(c, rel, probe, tag):
    S = probe_side(rel)
    want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    got, table, info, starts = build_probe(c, rel, S, probe)
    check_exact(got, table, want, tag)
    check_codes(got, info, tag)
    return got, want, starts


def tile_start(c, t):
    """first position of tile t of chunk c on the odd base (module docstring)"""
    return CHUNK * c + (ROW if c else 0) + TILE * t


def odd_base_starts():
    return np.array([0] + [CHUNK * c + ROW for c in range(1, 8)] + [N], dtype=I64)


@pytest.fixture(scope="module")
def plain(ctx):
    """the layout the cases of this file are written for; then the odd base by itself: its seams are where the cases count
    their tiles from, nothing is deferred or dropped"""
    lay = ctx.wave_layout_info(N)
    assert (lay["nChunks"], lay["chunkLen"], lay["tileTuples"], lay["granuleSlots"], lay["overlap"]) == (8, CHUNK, TILE, 128, ROW), lay
    got, want, starts = run_case(ctx, wc.relation(wc.base_odd(N)), 4, "odd base")
    assert np.array_equal(starts, odd_base_starts()), starts
    assert (want["conflicts"], got["buildDeferred"]) == (0, 0)
    return got


# ---- duplicates across both halves ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("rows", ((0, 1, 2, 3, 4, 5, 6, 7), (3, 4), (0, 7)), ids=("every-row", "rows-3-4", "rows-0-7"))
def test_one_key_on_both_sides_of_the_boundary(ctx, plain, rows, probe):
    """one key in every lane of the given rows of one tile (512 or 128 copies), homed where the first of those rows' own
    tuples were (their slots are vacant, the even ones between them free): the probeLength earliest copies are placed on
    H .. H + probeLength - 1 and every other copy drops, whichever batch attempted it and whether it met the slot taken at
    its home attempt (second batch, after a round) or lost it in a round"""
    homes = wc.base_odd(N)
    t0 = tile_start(3, 1)
    H = int(homes[t0 + ROW * rows[0] + 10])
    key = H + 5 * T
    rel = wc.relation(homes)
    for j in rows:
        rel[t0 + ROW * j:t0 + ROW * (j + 1)] = key
    got, want, starts = run_case(ctx, rel, probe, ("copies", rows, probe))
    assert np.array_equal(starts, odd_base_starts())
    copies = ROW * len(rows)
    assert (want["table"][H:H + probe] == U64(key)).all() and int((want["table"] == U64(key)).sum()) == probe
    assert (want["conflicts"], want["conflictSum"]) == (copies - probe, (copies - probe) * key)


# ---- second-half homes below first-half homes, and the mirror image ------------------------------------------------------------
def halves_relation(delta, off, mirror):
    """one tile (chunk 2, tile 1; its first slot B is a granule's first) whose one half holds 256 tuples homed on
    h_k = B + 4 k + off, every fourth slot, and whose other half holds groups of delta + 1 copies of a key homed delta slots
    below h_k for k = 1, 3, 5, ...: a group fills h_k - delta .. h_k - 1 and its last copy walks on into h_k. mirror=False:
    the singles sit in rows 0-3 (earlier: they keep h_k, the walker passes on to h_k + 1); mirror=True: the groups sit in
    rows 0-3 (earlier: the walker TAKES h_k, and the single homed there, attempted by the second batch, moves on). off = 1:
    every walk stays inside its granule; off = 3: h_31, h_63, ... are a granule's last slot, and those walks cross the edge.
    The high part is a function of the home slot, so the copies of a group are one key.
    -> (relation, first position of the tile, B, copies per group)"""
    homes = wc.base_odd(N)
    t0 = tile_start(2, 1)
    B = 2 * t0
    assert B % 128 == 0 and homes[t0] == B + 1
    singles = B + 4 * np.arange(HALF, dtype=I64) + off
    per = delta + 1
    g = np.arange(HALF, dtype=I64) // per           # group number of a position of the other half
    groups = B + 4 * (2 * g + 1) + off - delta
    assert 2 * g.max() + 1 < HALF and 2 * g.max() + 1 >= 31
    homes[t0:t0 + HALF], homes[t0 + HALF:t0 + TILE] = (groups, singles) if mirror else (singles, groups)
    return (homes + ((homes >> 2) % 3) * T).astype(U64), t0, B, per


@pytest.mark.parametrize("probe", (2, 4, 8))
@pytest.mark.parametrize("mirror", (False, True), ids=("second-half-below", "first-half-below"))
@pytest.mark.parametrize("off", (1, 3), ids=("mid-granule", "granule-end"))
@pytest.mark.parametrize("delta", (1, 2, 3))
def test_one_half_walks_into_the_others_slots(ctx, plain, delta, off, mirror, probe):
    rel, t0, B, per = halves_relation(delta, off, mirror)
    S = probe_side(rel)
    want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    # the cause, from the oracle's table, at the group of k = 1 and (granule-end) at the one of k = 31, whose h_k is the
    # granule's last slot: the slots below h_k hold the group's key; h_k holds the tuple of rows 0-3, and the one of rows 4-7
    # that wanted it sits behind it when its budget reaches that far
    tab = want["table"]
    for k in (1, 31) if off == 3 else (1,):
        hk = B + 4 * k + off
        assert off != 3 or k != 31 or hk % 128 == 127
        single = int(rel[t0 + (HALF if mirror else 0) + k])
        group = int(rel[t0 + (0 if mirror else HALF) + per * (k // 2)])
        assert group % T == hk - delta and single % T == hk
        assert all(int(x) == group for x in tab[hk - delta:hk][:probe]), (k, tab[hk - delta:hk + 2])
        if not mirror:
            assert int(tab[hk]) == single and (int(tab[hk + 1]) == group) == (probe >= delta + 2), (k, tab[hk - delta:hk + 2])
        elif probe >= delta + 1:
            assert (int(tab[hk]), int(tab[hk + 1])) == (group, single), (k, tab[hk - delta:hk + 2])
        else:
            assert int(tab[hk]) == single, (k, tab[hk - delta:hk + 2])
    got, table, info, starts = build_probe(ctx, rel, S, probe)
    check_exact(got, table, want, (delta, off, mirror, probe))
    check_codes(got, info, (delta, off, mirror, probe))
    assert np.array_equal(starts, odd_base_starts())


# ---- rounds between the halves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", (2, 4))
def test_rounds_run_between_the_batches(ctx, plain, probe):
    """a tile of pairs: positions 2 m and 2 m + 1 of the tile share a home slot, so in every row 32 home attempts fail and
    32 entries are queued. After rows 0 and 1 the queue holds 64: a round runs before row 2 is pushed, and again before row 4
    is -- between the first batch's push rows and the second batch's -- so the second batch pushes onto a queue that stands
    at its round threshold. That the entries were there is read from the oracle's table (a tuple that does not sit on its
    home slot was queued); that the rounds finished them inside the ring is read from buildDeferred, which stays the odd
    base's 0; nothing drops (the slot behind every pair is free)."""
    homes = wc.base_odd(N)
    t0 = tile_start(4, 2)
    assert (2 * t0) % 128 == 0
    homes[t0:t0 + TILE] = 2 * t0 + 4 * (np.arange(TILE, dtype=I64) // 2) + 1     # the tile's 1024 slots: one ring
    rel = (homes + (1 + np.arange(N, dtype=I64) % 2) * T).astype(U64)          # the two tuples of a pair are different keys
    got, want, starts = run_case(ctx, rel, probe, ("pairs", probe))
    assert np.array_equal(starts, odd_base_starts())
    slot_of = {int(k): i for i, k in enumerate(want["table"]) if k}
    off_home = [int(r) for r in rel[t0:t0 + 3 * ROW] if slot_of[int(r)] != int(r) % T]
    assert len(off_home) == 3 * ROW // 2 >= 64, ("vacuous: rows 0-2 queue fewer than a round's worth", len(off_home))
    assert want["conflicts"] == 0
    assert got["buildDeferred"] == plain["buildDeferred"] == 0, ("the rounds did not finish the pairs in the ring", got["buildDeferred"])


# ---- tiles whose positions end at the batch boundary; a seam zone across it -------------------------------------------------------
def move_seam(homes, c, d):
    """seam c of the odd base, moved: the chunk starts d positions past its nominal seam p = 2048 c instead of 64. d > 64: the
    d tuples from p on are all homed inside p's granule (twice per slot: some drop, the oracle says which); d = 1: the tuple
    at p is homed on the last slot of the granule before, so the very next position is the first of the range. A seam moves
    by less than the look, 256 positions. -> the chunk's first position"""
    p = CHUNK * c
    if d == 1:
        homes[p] = 2 * p - 1
    else:
        assert 64 < d < 256
        homes[p:p + d] = 2 * p + 1 + (np.arange(d, dtype=I64) * 126) // (d - 1)
    return p + d


def stragglers(homes, c, q, which):
    """the given positions of the zone [q, q + 64) behind seam c become stragglers of the range below: pairs on every fourth
    slot of the granule below the seam's own (free even slots between the base's tuples, inside the previous wavefront's
    ring): the first of a pair stays, the second walks two slots on when its budget allows"""
    assert which.min() > q and which.max() < q + ROW
    homes[which] = 2 * CHUNK * c - 2 - 4 * (np.arange(which.size, dtype=I64) // 2)
    assert (homes[which] >= 2 * CHUNK * c - 128).all()


@pytest.mark.parametrize("probe", (1, 4))
@pytest.mark.parametrize("ends", (255, 256, 257, 1))
def test_a_chunk_whose_positions_end_at_the_boundary(ctx, plain, ends, probe):
    """chunk 3 reads `ends` positions of its fifth tile, the last 64 of them its overlap zone, whose tuples behind the seam's
    first are homed below the seam (stragglers: live in THIS chunk): the live lanes end one lane before, exactly at, and one
    lane past the boundary between the batches (255, 256, 257), or rows 1-7 have nothing at all (1). With chunk 3 starting
    one position past its nominal seam (255 - 257) or at the odd base's 64 (1), seam 4 is moved by ends - 63, respectively by
    1. (rSize is a power of two on this road and a seam moves by less than 256 positions, so the relation's own last tile
    holds 257 to 512 positions: test_the_relations_last_tile.)"""
    homes = wc.base_odd(N)
    s3 = move_seam(homes, 3, 1) if ends != 1 else 3 * CHUNK + ROW
    q = move_seam(homes, 4, ends - 63 if ends != 1 else 1)
    stragglers(homes, 4, q, np.arange(q + 1, q + ROW))
    rel = wc.relation(homes)
    got, want, starts = run_case(ctx, rel, probe, ("ends", ends, probe))
    assert (int(starts[3]), int(starts[4])) == (s3, q), starts
    assert q + ROW - s3 == 4 * TILE + ends
    assert want["table"][2 * CHUNK * 4 - 2] == rel[q + 1]            # a straggler on its home slot: chunk 3 inserted it


@pytest.mark.parametrize("probe", (1, 4))
def test_the_relations_last_tile(ctx, plain, probe):
    """the last seam moved by 255 positions: the last chunk's fourth tile holds 257 positions, rows 0-3 and one lane of row 4"""
    homes = wc.base_odd(N)
    q = move_seam(homes, 7, 255)
    got, want, starts = run_case(ctx, wc.relation(homes), probe, ("last tile", probe))
    assert int(starts[7]) == q and N - q == 3 * TILE + 257, starts


@pytest.mark.parametrize("probe", (2, 4))
def test_the_overlap_zone_across_the_boundary(ctx, plain, probe):
    """chunk 3 starts one position past its nominal seam and seam 4 is moved by 225: chunk 3's overlap zone is positions
    [224, 288) of its fifth tile, 32 lanes of row 3 and 32 of row 4 -- the zone tests and the stragglers' attempts run in both
    batches -- and the same 64 positions are chunk 4's head zone, row 0 of its first tile. Every other tuple of the zone behind
    its first is a straggler, in pairs (the second of a pair walks past an earlier tuple, or drops at probeLength 2); the
    tuples between them belong to chunk 4's range."""
    homes = wc.base_odd(N)
    s3 = move_seam(homes, 3, 1)
    q = move_seam(homes, 4, 225)
    which = np.arange(q + 1, q + ROW, 2)
    stragglers(homes, 4, q, which)
    rel = wc.relation(homes)
    got, want, starts = run_case(ctx, rel, probe, ("zone", probe))
    assert (int(starts[3]), int(starts[4])) == (s3, q), starts
    zone = q - s3 - 4 * TILE
    assert (zone, zone + ROW) == (224, 288)
    row_of = (which - s3 - 4 * TILE) // ROW
    assert set(row_of.tolist()) == {3, 4}                            # stragglers on both sides of the boundary
    for pos in (which[0], which[-2]):                                # the first of a pair, one in row 3 and one in row 4
        assert want["table"][int(homes[pos])] == rel[pos], pos
    assert (want["table"][int(homes[which[1]]) + 2] == rel[which[1]]) == (probe >= 3)   # the second of a pair walked


# ---- the oracle's relation: every tile runs the loop -----------------------------------------------------------------------------
@pytest.mark.parametrize("probe", PROBES)
def test_uniform(ctx, probe):
    """`uniform` W=16 (the relation of test_gpu_ring_words.py): displacements and drops in every tile, on both sides of every
    boundary; the rings and the window build"""
    rel = oracle.generate_data("uniform", N, N, 16)
    S = oracle.relS_for("uniform", rel)
    want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    assert want["conflicts"] > 0
    for variant in (3, 0):
        got, table, info, _ = build_probe(ctx, rel, S, probe, variant)
        check_exact(got, table, want, (probe, variant))
        check_codes(got, info, (probe, variant))
    if probe > 1:
        assert got["buildDeferred"] > 0, probe


# ---- the size rule's own road: more than one round of workgroups ------------------------------------------------------------------
def test_the_size_rule_road(ctx):
    """2^27 slots at probeLength 4, no flag: the road production takes, and the one place in the suite where the launch at
    the road's occupancy runs more than one round of workgroups. Homes out of order by up to 7 slots; six tuples on one home
    every 64 positions, placed so that they lie across a row's end -- every eighth group across the boundary between the
    batches -- (two drop); a tuple 4096 slots ahead of its neighbours every 2^15 (deferred); every high part the table
    leaves room for"""
    tbits = 27
    TT, n, nhi = 1 << tbits, 1 << (tbits - 1), 1 << (32 - tbits)
    assert hj.slot_codes_info(TT, 4)["fitsAuto"]
    i = np.arange(n, dtype=I64)
    home = 2 * i + (((i * 2654435761) >> 16) & 7) + 16
    hi = (37 * i + (i >> 11)) & (nhi - 1)
    g = np.arange(61, n - 8, 64)
    for k in range(1, 6):
        home[g + k] = home[g]
    e = np.arange(7001, n - 4096, 1 << 15)
    home[e] += 4096
    np.minimum(home, TT - 1, out=home)
    rel = (home + hi * TT).astype(U64)
    S = np.concatenate([rel[::3], rel[5::64] ^ U64(TT)])
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    assert want["conflicts"] > n // 64 and 0 < want["totalMatches"] < S.size
    ctx.reserve("atomic", rel.size, S.size, probeLength=4, buildVariant=3)
    with Device(ctx) as dev:
        ctx.build(dev.put(rel), rel.size)
        ctx.probe(dev.put(S), S.size)
        ctx.checksums()
        got, table, info = ctx.fetch(), ctx.export_table(TT), ctx.slot_codes_info()
    check_exact(got, table, want, "2^27")
    assert info["fitsAuto"]
    check_codes(got, info, "2^27", road=1)
    assert got["buildDeferred"] > 0
