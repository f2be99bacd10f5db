"""The ring build on the slot-code road keeps 4-byte ring words in LDS (hj_table.h RingWord; tests/test_ring_words.py has the
word's arithmetic): (offset in the chunk << 7 | code) instead of (index << 32 | key). What a wavefront does with them --
home attempts, looks, displacement, the budget decided before the step, the key read back for a drop and for a deferred
tuple, the retire -- is checked here on the forced road (tables of 2^15 slots, reserve(..., slotCodes=True)) and once on the
road the size rule takes by itself (2^27 slots at probeLength 4). Every case asserts through slot_codes_info() that the road
was taken; every expected value -- the exported table slot for slot, conflicts, conflictSum, totalMatches, the sums -- is the
sequential oracle's on the same arrays, and a case about one cause first shows, from the oracle's table or the build's
counters, that the cause happened. Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import Device, ctx  # noqa: F401
import wave_cases as wc
from oracle import oracle

pytestmark = pytest.mark.gpu

U64 = np.uint64
I64 = np.int64
N = 1 << 14                                  # eight chunks of 2048 tuples: seven seams, and a ring shorter than a chunk's range
T = 2 * N
COUNTERS = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum")
LOG_OVERFLOW, CODE_OVERFLOW = 1, 4           # slot_codes_info()["cause"]


def build_probe(c, rel, S, probe=4, variant=3, slot_codes=True):
    """one build + probe + checksums through the split API -> (result, exported table, slot_codes_info)"""
    c.reserve("atomic", rel.size, S.size, probeLength=probe, buildVariant=variant, slotCodes=slot_codes)
    with Device(c) as dev:
        c.build(dev.put(np.ascontiguousarray(rel, dtype=U64)), rel.size)
        c.probe(dev.put(np.ascontiguousarray(S, dtype=U64)), S.size)
        c.checksums()
        got = c.fetch()
        return got, c.export_table(2 * rel.size), c.slot_codes_info()


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


def dropped_keys(rel, table):
    """the keys the build dropped, with multiplicity: what the relation holds and the table does not"""
    keys, cnt = np.unique(rel, return_counts=True)
    tk, tc = np.unique(table[table != 0], return_counts=True)
    left = dict(zip(keys.tolist(), cnt.tolist()))
    for k, c in zip(tk.tolist(), tc.tolist()):
        left[k] -= c
    return sorted(k for k, c in left.items() for _ in range(c))


def run_case(c, rel, probe, tag, S=None):
    S = probe_side(rel) if S is None else S
    want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    got, table, info = build_probe(c, rel, S, probe)
    check_exact(got, table, want, tag)
    check_codes(got, info, tag)
    return got, want


# ---- the oracle's relations, seams included -------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", (1, 2, 3, 4, 8))
def test_uniform(ctx, probe):
    """`uniform` W=16: 37 % of the tuples repeat a key -- displacements and drops in every tile, stragglers at every seam"""
    rel = oracle.generate_data("uniform", N, N, 16)
    S = oracle.relS_for("uniform", rel)
    want = oracle.build_probe_seq(rel, S, probe, want_table=True)
    assert want["conflicts"] > 0
    for variant in (3, 0):
        got, table, info = build_probe(ctx, rel, S, probe, variant)
        check_exact(got, table, want, (probe, variant))
        check_codes(got, info, (probe, variant))
    if probe > 1:
        assert got["buildDeferred"] > 0, probe


@pytest.fixture(scope="module")
def seam_cases(ctx):
    lay = ctx.wave_layout_info(N)
    assert lay["nChunks"] == 8
    return [c for c in wc.cases(N, lay, full=True) if not c.keys32]


@pytest.mark.parametrize("family", ("A", "A1", "B", "C", "D", "H", "R"))
def test_directed_seam_cases(ctx, seam_cases, family):
    """tests/wave_cases.py (tuples). A: copies of one key right before a seam walk across it -- the deferred tuple of the
    first kind, a seam crosser, rebuilt from (pos, word) as (pos, index << 32 | key)"""
    todo = [c for c in seam_cases if c.family == family]
    assert todo
    for case in todo:
        got, _ = run_case(ctx, wc.relation(case.homes), case.probe, case.name)
        if family == "A" and case.crossing is not None:
            assert got["buildDeferred"] >= min(case.crossing, case.probe - 1), case.name
        if family == "R":
            assert got["buildDeferred"] >= 1, case.name


def test_keys_that_differ_only_above_the_table_size(ctx):
    """k, k + T, k + 2T share a home slot and differ in the word's code alone: six of them on ONE home slot displace each
    other, in four places; S asks for all three variants of every home"""
    i = np.arange(N, dtype=I64)
    homes, hi = 2 * i + 1, i % 3
    for a in (1000, 5000, 5001, 12000):
        homes[a:a + 6] = homes[a]
        hi[a:a + 6] = np.arange(6) % 3
    rel = (homes + hi * T).astype(U64)
    S = np.concatenate([(homes + j * T).astype(U64) for j in range(3)])
    got, want = run_case(ctx, rel, 4, "alias", S)
    assert 0 < want["conflicts"] and N // 2 < want["totalMatches"] < S.size // 2


# ---- the budget: decided before the step ------------------------------------------------------------------------------------
def last_slot_relation(hi, copies=True):
    """the odd base with, from position 5000 on: a tuple homed on H + 1, the base's own on H + 2, then three copies of the key
    homed on H = 10001 with high part hi (copies=False: the base's own tuples stay in those three places)"""
    homes = wc.base_odd(N)
    rel = wc.relation(homes)
    at, H = 5000, int(homes[5000])
    assert H & 127 <= 123 and homes[at + 1] == H + 2
    rel[at] = H + 1
    if copies:
        rel[at + 2:at + 5] = H + hi * T
    return rel, H, H + hi * T


@pytest.mark.parametrize("hi", (0, 31))
def test_the_last_slot_is_lost_to_an_earlier_tuple(ctx, hi):
    """probeLength 4, the carry trap itself, inside the ring. Two earlier tuples hold H + 1 and H + 2; of the three copies
    of H that follow in the same tile one takes H, and the other two are queued at (H + 1, d = 1). In the tile's round both
    look, see two earlier tuples, skip them and try H + 3 with d = 3, their last slot, in the same instruction: one is
    placed, and the other -- whether its own try fails or it is the one displaced -- is carried with no try left and
    must drop THERE, with the key read from (H + 3, word). One step more would carry out of the displacement's two bits into
    the high part, and with hi = 31 on into rel: a foreign key placed on H + 4. That the drop was the ring's and not the
    deferred phase's is shown by the deferred count, which the same relation without the copies has too."""
    rel, H, key = last_slot_relation(hi)
    plain, _, _ = last_slot_relation(hi, copies=False)
    got0, want0 = run_case(ctx, plain, 4, ("last slot, no copies", hi))
    assert want0["conflicts"] == 0
    got, want = run_case(ctx, rel, 4, ("last slot", hi))
    assert (want["conflicts"], want["conflictSum"]) == (1, key)
    assert [int(x) for x in want["table"][H:H + 5]] == [key, H + 1, H + 2, key, 0]
    assert got["buildDeferred"] == got0["buildDeferred"], ("vacuous: a copy left the ring", got["buildDeferred"], got0["buildDeferred"])


@pytest.mark.parametrize("probe", (3, 4))
@pytest.mark.parametrize("hi", (0, 31))
@pytest.mark.parametrize("at", (5000, 4990), ids=("mid-granule", "granule-end"))
def test_a_run_longer_than_the_budget_drops_its_tail(ctx, probe, hi, at):
    """probeLength + 5 copies of one key in the middle of a chunk (home slot the granule's 18th, or its 126th, where the
    walk crosses into the next granule): probeLength of them end on H .. H + probeLength - 1, five drop, conflictSum is five
    times the key. In the odd base a tile's homes span the whole ring, and a queue this short gets one round per tile: the
    copies are at d = 2 at most when the ring moves on, so most of them leave as deferred tuples -- this case holds the
    entry rebuilt from (pos, word), high part and displacement included, and the deferred phase's drops, not the ring's
    (test_the_last_slot_is_lost_to_an_earlier_tuple holds those)."""
    homes = wc.base_odd(N)
    rel = wc.relation(homes)
    H = int(homes[at])
    assert H % 128 == (125 if at == 4990 else 17)
    key = H + hi * T
    rel[at:at + probe + 5] = key
    got, want = run_case(ctx, rel, probe, ("run", probe, hi, at))
    assert (want["conflicts"], want["conflictSum"]) == (5, 5 * key)
    assert (want["table"][H:H + probe] == U64(key)).all()


@pytest.mark.parametrize("probe", (3, 4, 8))
def test_a_displacement_chain_that_ends_in_a_drop(ctx, probe):
    """a dense block (64 tuples on 64 consecutive slots, free slots behind it) in the odd base, with probeLength copies of one
    key BEFORE the tuples homed on the slots they take: every later tuple of the block is pushed probeLength - 1 slots on, to
    its last slot. One tuple more, earlier than all of them and homed 39 slots further on, holds a slot of that row: the
    tuples in front of it are pushed up to it with one try left, and the one that drops there is a bystander, not a copy of
    anything. (Whether the ring or the deferred phase drops it depends on when the ring moves on; the case holds the result.)"""
    homes = wc.base_odd(N)
    at = 5000
    homes[at - 8:at + 56] = homes[at - 8] + np.arange(64)
    H, early = int(homes[at]), int(homes[at + 39])
    homes[at - probe + 1:at] = H                 # probeLength copies of H (the base's own is the last)
    homes[at - probe] = early                    # index below every tuple it gets in the way of
    rel = wc.relation(homes)
    want = oracle.build_probe_seq(rel, probe_side(rel), probe, want_table=True)
    gone = dropped_keys(rel, want["table"])
    assert gone and H not in gone and early not in gone, ("vacuous: no bystander dropped", gone[:8])
    assert want["conflictSum"] == sum(gone)
    run_case(ctx, rel, probe, ("chain", probe))


def test_a_walk_that_wraps_at_the_tables_end(ctx):
    """three copies of the key homed on the table's last slot, with hi = 5: one stays, two leave the last range through the
    table's end as deferred tuples and land on slots 0 and 2 (slot 1 is the first tuple's); their keys come out of a slot
    number BELOW the displacement (SlotCode::decode's wrap)"""
    rel = wc.relation(wc.base_odd(N))
    key = (T - 1) + 5 * T
    rel[-3:] = key
    got, want = run_case(ctx, rel, 4, "wrap")
    assert want["conflicts"] == 0 and want["table"][T - 1] == want["table"][0] == want["table"][2] == U64(key)
    assert got["buildDeferred"] >= 2


# ---- deferred tuples of the second kind: the ring has moved on ----------------------------------------------------------------
@pytest.mark.parametrize("probe", (3, 4))
def test_a_key_far_behind_its_neighbours(ctx, probe):
    """three copies of a key homed 1500 tuples (3000 slots: more than any ring) behind their position, inside their own
    chunk's range: the slots they want have left the ring, so they are deferred at their home slot with d = 0 and walk in
    HBM over slots that hold earlier tuples -- two find the free even slots (probeLength 4; one at 3), the rest drop"""
    homes = wc.base_odd(N)
    rel = wc.relation(homes)
    at = 2048 * 3 + 1900                         # late in chunk 3
    H = int(homes[at - 1500])
    key = H + 9 * T
    rel[at:at + 3] = key
    got, want = run_case(ctx, rel, probe, ("behind", probe))
    placed = 2 if probe == 4 else 1
    assert (want["conflicts"], want["conflictSum"]) == (3 - placed, (3 - placed) * key)
    assert want["table"][H + 1] == U64(key) and (want["table"][H + 3] == U64(key)) == (probe == 4)
    assert got["buildDeferred"] >= 3, ("vacuous: the ring still held the slots", got["buildDeferred"])


def test_a_chain_that_outlives_the_ring(ctx):
    """a tuple homed three chunks AHEAD of its neighbours is deferred at its home slot (an outlier is deferred, not the
    tile). The wavefront that owns the slot fills and retires it long before the deferred phase, where the outlier, the
    earlier tuple, takes it: the tuple it finds there and the ones behind that are displaced in HBM, slot after slot up to
    the next free one (the gapped base has one every 32), their keys read from R"""
    homes = wc.base_gapped(N)
    at = 2048 * 2 + 700
    ahead = int(homes[2048 * 5 + 300])
    assert ahead % 32 < 12                       # the chain is a few slots long and ends inside the granule's run of tuples
    rel = wc.relation(homes)
    rel[at] = ahead + 3 * T
    want = oracle.build_probe_seq(rel, probe_side(rel), 4, want_table=True)
    assert want["table"][ahead] == U64(ahead + 3 * T) and want["table"][ahead + 1] == U64(ahead) and want["table"][ahead + 2] == U64(ahead + 1)
    got, _ = run_case(ctx, rel, 4, "ahead")
    assert got["buildDeferred"] >= 1


# ---- the hand-over causes stay what they are ------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", (32 * T + 12345, 0xFFFFFFFF), ids=("hiCap", "all-ones"))
def test_a_key_without_a_code_hands_over(ctx, key):
    """cause 4: the tile raises it whatever its lanes put into the ring afterwards (the word keeps its rel whole); the 8-byte
    build redoes the table, exact"""
    rel = wc.relation(wc.base_odd(N))
    rel[7000] = key
    rel[7001:7004] = rel[7004]                   # and displacements right behind it, in the same tile
    S = np.concatenate([[key, key], rel[6990:7010], rel[6990:7010] + U64(32 * T), probe_side(rel)]).astype(U64)
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    got, table, info = build_probe(ctx, rel, S)
    check_exact(got, table, want, key)
    assert got["buildVariant"] == 3 and got["compactFallback"] == 0
    assert (info["codes"], info["cause"], info["road"], info["tableFormat"]) == (False, CODE_OVERFLOW, 2, 0), info


def test_log_overflow_stays_a_cause(ctx):
    """the rings forced onto `shuffle`: nearly every tuple is deferred out of its ring word, the dirty logs cannot fit --
    cause 1, the 8-byte build redoes the table, exact"""
    n = 1 << 16
    rel = oracle.generate_data("shuffle", n, n, 16)
    S = probe_side(rel)
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    got, table, info = build_probe(ctx, rel, S)
    check_exact(got, table, want, "shuffle")
    assert got["buildVariant"] == 3 and got["buildDeferred"] > n // 2
    assert (info["codes"], info["cause"], info["road"], info["tableFormat"]) == (False, LOG_OVERFLOW, 2, 0), info


def test_one_context_across_the_roads():
    """ring words -> a key without a code (8-byte slots) -> ring words -> the same context without the flag (the 8-byte
    ring retiring 4-byte keys) -> ring words: every reader on each, and the info calls say which road it was"""
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


# ---- the size rule's own road -----------------------------------------------------------------------------------------------
def test_the_size_rule_at_its_smallest_table(ctx):
    """2^27 slots at probeLength 4, no flag: the road production takes. Homes out of order by up to 7 slots with equal and
    neighbouring homes everywhere, six tuples on one home every 64 positions (two drop), a tuple 4096 slots ahead of its
    neighbours every 2^15 (deferred), the last homes clipped to the table's last slot (walks that wrap), and every high part
    the table leaves room for"""
    tbits = 27
    TT, n, nhi = 1 << tbits, 1 << (tbits - 1), 1 << (32 - tbits)
    assert hj.slot_codes_info(TT, 4)["fitsAuto"] and not hj.slot_codes_info(TT >> 1, 4)["fitsAuto"]
    i = np.arange(n, dtype=I64)
    home = 2 * i + (((i * 2654435761) >> 16) & 7) + 16
    hi = (37 * i + (i >> 11)) & (nhi - 1)
    g = np.arange(40, n - 8, 64)
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
