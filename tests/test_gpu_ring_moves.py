"""The ring build on the slot-code road moves its ring before EACH batch of four rows (hj_build_wave.hip, CODES): before rows
0-3 only as far as their highest home slot needs, before rows 4-7 as far as the tile's, both capped by the tile's lowest home
slot and by the range's end. What can newly go wrong is the move between the batches, and every case here puts something
there: entries a tile left queued in the granules the first move keeps, an entry already behind the ring, an outlier ahead
of it, a low outlier in the second batch, batches without a live tuple, a seam inside a tile. The harness is that of
test_gpu_ring_rows.py: the forced road at N = 2^14 (tables of 2^15 slots, reserve(..., slotCodes=True), eight chunks of four
tiles), once the size rule's own road (2^27 slots); the road is asserted through slot_codes_info(); every expected value --
the exported table slot for slot, conflicts, conflictSum, totalMatches, the sums -- is the sequential oracle's on the same
arrays, and a case about one cause first shows, from the oracle's table, the seams or buildDeferred, that the cause happened.

Where a tile lies: on the odd base (homes 2i + 1, 64 tuples per granule) chunk c > 0 starts at position 2048 c + 64 and
chunk 0 at 0 (asserted from wave_seams()), so tile t of chunk c > 0 covers positions 2048 c + 64 + 512 t + [0, 512) and the
1024 slots from B = 2 * (its first position), a granule's first: one whole ring of eight granules. A half tile spans four
granules, so on this base the ring moves before every batch: before rows 0-3 of a tile to the granule of B - 384 (three
granules of the tile before stay as history), before rows 4-7 to B's. Run with -m gpu on an MI355X."""
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
CHUNK, TILE, ROW, HALF, GRAN = 2048, 512, 64, 256, 128
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


def run_case(c, rel, probe, tag, want=None):
    S = probe_side(rel)
    if want is None:
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
    assert (lay["nChunks"], lay["chunkLen"], lay["tileTuples"], lay["granuleSlots"], lay["overlap"]) == (8, CHUNK, TILE, GRAN, ROW), lay
    got, want, starts = run_case(ctx, wc.relation(wc.base_odd(N)), 4, "odd base")
    assert np.array_equal(starts, odd_base_starts()), starts
    assert (want["conflicts"], got["buildDeferred"]) == (0, 0)
    return got


# ---- a move between the batches that would strand queued entries ------------------------------------------------------------------
def stranded_relation():
    """Tile 1 of chunk 4 leaves 63 entries queued at its end, all in its last two granules; tile 2 is the plain odd base but
    for one pair.
    In tile 1 positions 2 m and 2 m + 1 of rows 0-1 share a home slot (64 failed home attempts: the round runs before row 2
    is pushed, so the tile has had its round), and so do 63 pairs of positions of rows 6-7 (the last pair is two singles):
    63 entries, one short of a round, wait at home + 1 when the tile ends. Tile 2's rows 0-3 reach four granules up from
    B + 1024: the move before them retires tile 1's granules up to B + 640 and keeps the three with the entries. Positions
    0 and 1 of tile 2 share a home slot: the 64th entry, so the round is due before row 1 is pushed and finishes all of
    them inside the ring, before the move in front of rows 4-7 retires their granules. (Without that pair no round is due
    in rows 0-3, and the second move leaves the 63 behind: rounds in front of a move were measured and not kept,
    profiles/ring_moves.md.) -> (relation, first position of tile 1, B)"""
    homes = wc.base_odd(N)
    t0 = tile_start(4, 1)
    B = 2 * t0
    assert B % GRAN == 0 and homes[t0] == B + 1
    homes[t0:t0 + 2 * ROW] = B + 4 * (np.arange(2 * ROW, dtype=I64) // 2) + 1
    homes[t0 + 6 * ROW:t0 + TILE - 2] = B + 6 * GRAN + 4 * (np.arange(2 * ROW - 2, dtype=I64) // 2) + 1
    assert homes[t0 + TILE - 2] == B + 8 * GRAN - 3 and homes[t0 + TILE - 1] == B + 8 * GRAN - 1
    homes[t0 + TILE + 1] = homes[t0 + TILE]
    rel = (homes + (1 + np.arange(N, dtype=I64) % 2) * T).astype(U64)          # the two tuples of a pair are different keys
    return rel, t0, B


@pytest.mark.parametrize("probe", (2, 4))
def test_the_first_move_keeps_what_the_last_tile_left_queued(ctx, plain, probe):
    """the entries a tile leaves queued lie below the next tile's second move and above its first: the granules they stand in
    stay through rows 0-3, whose first failed attempt makes the round due, and they finish inside the ring -- buildDeferred
    stays the odd base's 0. A ring that moved once per tile, all the way, deferred all 63."""
    rel, t0, B = stranded_relation()
    want = oracle.build_probe_seq(rel, probe_side(rel), probe, want_table=True)
    slot_of = {int(k): i for i, k in enumerate(want["table"]) if k}
    queued = [int(r) for r in rel[t0 + 6 * ROW:t0 + TILE] if slot_of[int(r)] != int(r) % T]
    first = [int(r) for r in rel[t0:t0 + 2 * ROW] if slot_of[int(r)] != int(r) % T]
    assert (len(first), len(queued)) == (ROW, ROW - 1), ("vacuous", len(first), len(queued))
    assert all(B + 6 * GRAN < slot_of[r] < B + 8 * GRAN for r in queued)       # below tile 2's second move, above its first
    assert slot_of[int(rel[t0 + TILE + 1])] == int(rel[t0 + TILE + 1]) % T + 1          # the 64th entry
    assert want["conflicts"] == 0
    got, _, starts = run_case(ctx, rel, probe, ("stranded", probe), want)
    assert np.array_equal(starts, odd_base_starts())
    assert got["buildDeferred"] == plain["buildDeferred"] == 0, ("the first move left queued entries behind", got["buildDeferred"])


# ---- entries no move can keep ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", (3, 4))
def test_an_entry_already_behind_the_ring(ctx, plain, probe):
    """three copies of a key homed 1500 tuples (3000 slots: more than any ring) behind their position, in row 1 of a tile of
    their own chunk: pushed unattempted, they wait in the queue behind the ring through the move before rows 4-7, the next
    round defers them, and they walk in HBM over slots that hold earlier tuples: two find the free even slots (probeLength
    4; one at 3), the rest drop. They are also the tile's lowest home slot, which holds both moves back: the tile's upper
    rows are ahead of the ring and deferred with them."""
    homes = wc.base_odd(N)
    rel = wc.relation(homes)
    at = tile_start(3, 3) + ROW + 20
    H = int(homes[at - 1500])
    assert CHUNK * 3 + ROW <= at - 1500                                  # inside chunk 3's own range
    key = H + 9 * T
    rel[at:at + 3] = key
    got, want, _ = run_case(ctx, rel, probe, ("behind", probe))
    placed = 2 if probe == 4 else 1
    assert (want["conflicts"], want["conflictSum"]) == (3 - placed, (3 - placed) * key)
    assert want["table"][H + 1] == U64(key) and (want["table"][H + 3] == U64(key)) == (probe == 4)
    assert got["buildDeferred"] >= 3, ("vacuous: the ring still held the slots", got["buildDeferred"])


@pytest.mark.parametrize("row", (1, 5))
def test_an_outlier_ahead_of_the_ring(ctx, plain, row):
    """a tuple homed three chunks AHEAD of its neighbours, in the first or the second batch: it is the highest home slot of its
    batch, but the ring never passes the tile's lowest, so it is pushed unattempted and waits ahead of the ring until a round
    defers it. The wavefront that owns the slot fills it long before the
    deferred phase, where the outlier, the earlier tuple, takes it and the tuple it finds moves on to the free slot behind"""
    homes = wc.base_odd(N)
    at = tile_start(2, 1) + ROW * row + 7
    ahead = int(homes[CHUNK * 5 + 300])
    rel = wc.relation(homes)
    rel[at] = ahead + 3 * T
    got, want, starts = run_case(ctx, rel, 4, ("ahead", row))
    assert np.array_equal(starts, odd_base_starts())
    assert want["table"][ahead] == U64(ahead + 3 * T) and want["table"][ahead + 1] == U64(ahead) and want["conflicts"] == 0
    assert got["buildDeferred"] >= 1


# ---- a low outlier in the second batch ------------------------------------------------------------------------------------------
def test_a_low_outlier_in_rows_4_to_7(ctx):
    """the gapped base (homes 1, 2, ... without the slots = 16 mod 32: a tile spans 529 slots, so the ring keeps history). The
    cap by the tile's lowest home slot binds on a tile that still fits the ring only when the tile's highest home slot lies
    in the last probeLength + 8 slots of its granule g (the move then makes room for granule g + 1 as well): so the last
    tuple of a tile of chunk 5 is moved up to such a slot, and a tuple of row 5 is homed on a free slot of granule g - 7,
    below everything rows 0-3 hold, in a granule the ring still has when the tile starts. Uncapped, the move before rows
    4-7 would go to granule g - 6 and retire it; capped it stays, the tuple takes its slot in the ring, and buildDeferred
    is that of the same relation without the outlier."""
    homes = wc.base_gapped(N)
    lay = ctx.wave_layout_info(N)
    seams = wc.expected_seams(wc.relation(homes), lay, T)[0]
    t0 = int(seams[5]) + 2 * TILE                                        # a full tile in the middle of chunk 5
    assert int(seams[5]) + ROW <= t0 and t0 + TILE <= int(seams[6])
    h = int(homes[t0 + TILE - 1])
    X = (h | (GRAN - 1)) - 5
    assert h < X and X + 4 + 8 >= (X | (GRAN - 1)) + 1
    homes[t0 + TILE - 1] = X
    g = X // GRAN
    uncapped = (X + 4 + 8) // GRAN + 1 - 8                               # where the move before rows 4-7 goes without the cap
    low = (g - 7) * GRAN + 16                                            # a free slot of the base
    assert uncapped == g - 6 > low // GRAN and low % 32 == 16 and low < int(homes[t0])
    assert (int(homes[t0 - 1]) + 4 + 8) // GRAN + 1 - 8 <= low // GRAN   # the tile before kept the granule
    assert (int(homes[t0 + HALF - 1]) + 4 + 8) // GRAN + 1 - 8 <= low // GRAN       # ... and so does the move before rows 0-3
    base, want0, starts = run_case(ctx, wc.relation(homes), 4, "gapped base")
    assert np.array_equal(starts, seams)
    at = t0 + 5 * ROW + 11
    homes[at] = low
    rel = wc.relation(homes)
    rel[at] += U64(2 * T)
    got, want, starts2 = run_case(ctx, rel, 4, "low outlier")
    assert np.array_equal(starts2, seams)
    assert want["table"][low] == rel[at] and want["conflicts"] == want0["conflicts"]
    assert got["buildDeferred"] == base["buildDeferred"], (got["buildDeferred"], base["buildDeferred"])


# ---- empty and partial batches; a seam inside a tile -------------------------------------------------------------------------------
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
    assert (homes[which] >= 2 * CHUNK * c - GRAN).all()


@pytest.mark.parametrize("probe", (1, 4))
@pytest.mark.parametrize("ends", (255, 256, 257, 1))
def test_a_batch_without_a_live_tuple(ctx, plain, ends, probe):
    """chunk 3 reads `ends` positions of its fifth tile, the last 64 of them its overlap zone, whose tuples behind the seam's
    first are stragglers of chunk 3's range: the tile's live tuples end one lane before, exactly at, and one lane past the
    boundary between the batches (255, 256, 257) -- the second batch has no live tuple, or one, and its move must go nowhere
    new -- or rows 1-7 have nothing at all (1). The same 64 positions are chunk 4's head zone: row 0 of ITS first tile
    belongs to the previous range but for one tuple, and the first batch's highest home slot comes from rows 1-3."""
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
    """the last seam moved by 255 positions: the last chunk's fourth tile holds 257 positions, rows 0-3 and one lane of row 4,
    and the last range is open to the table's end"""
    homes = wc.base_odd(N)
    q = move_seam(homes, 7, 255)
    got, want, starts = run_case(ctx, wc.relation(homes), probe, ("last tile", probe))
    assert int(starts[7]) == q and N - q == 3 * TILE + 257, starts


@pytest.mark.parametrize("probe", (2, 4))
def test_a_seam_inside_a_tile(ctx, plain, probe):
    """chunk 3 starts one position past its nominal seam and seam 4 is moved by 225: chunk 3's overlap zone is positions
    [224, 288) of its fifth tile, 32 lanes of row 3 and 32 of row 4, so both batches of that tile hold live stragglers and
    tuples of the next range side by side, and both of its moves are bounded by the range's end; the same 64 positions are
    chunk 4's head zone. Every other tuple of the zone behind its first is a straggler, in pairs (the second of a pair
    walks past an earlier tuple, or drops at probeLength 2)."""
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


# ---- the oracle's relation: every tile moves its ring twice -------------------------------------------------------------------------
@pytest.mark.parametrize("probe", PROBES)
def test_uniform(ctx, probe):
    """`uniform` W=16: displacements and drops in every tile; the rings and the window build. What is still deferred are the
    seams' stragglers and a few entries behind the ring (tools/sim/ring_moves.c counts 1, 4, 2 and 31 deferred tuples at
    probeLength 2, 3, 4 and 8 on this relation, of which 1, 2, 2 and 11 at seams, against 1, 14, 17 and 70 under one move
    per tile; the device gives the same figures)"""
    rel = oracle.generate_data("uniform", N, N, 16)
    S = oracle.relS_for("uniform", rel)
    want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    assert want["conflicts"] > 0
    for variant in (3, 0):
        got, table, info, _ = build_probe(ctx, rel, S, probe, variant)
        check_exact(got, table, want, (probe, variant))
        check_codes(got, info, (probe, variant))
        print("uniform probeLength", probe, "variant", variant, "buildDeferred", got["buildDeferred"])
    if probe > 1:
        assert 0 < got["buildDeferred"], probe


# ---- the size rule's own road: more than one round of workgroups ------------------------------------------------------------------
def test_the_size_rule_road(ctx):
    """2^27 slots at probeLength 4, no flag: the road production takes, more than one round of workgroups. Homes out of order
    by up to 7 slots; six tuples on one home every 64 positions, placed so that they lie across a row's end -- every eighth
    group across the boundary between the batches -- (two drop); a tuple 4096 slots ahead of its neighbours every 2^15
    (deferred); every high part the table leaves room for"""
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
