"""Case table and plain restatement for the workgroup-window build (buildVariant 2: k_build_own, k_finalize_range,
k_clear_unowned, k_build_deferred in hj_build_own.hip).

No GPU and no pytest fixtures in here: test_own_cases.py checks on the CPU that the restatement gives the sequential oracle's
table and that every constructor produces the property it is named for, test_gpu_own_window.py runs the table on the device.

own_plan restates phase A chunk by chunk from the rules in the kernel's comments: per tile the lowest home block, the slide
of the window (back blocks, forward only, clamped at the table's end), the blocks the tile wants (home block, straddle
flag, counting with the quarter rule in a chunk's first and last tile), the claims, the inserts. The index-priority
protocol is confluent, so the inserts of a tile are applied one tuple after the other in input order -- no lanes, no retry
queue, no look-ahead: a tuple walks from its home slot, takes a free slot or a slot held by a later tuple (which walks on
in its place), is dropped when its budget of probeLength slots is used up, and is DEFERRED, with the slot it has reached,
when that slot lies in a block the chunk does not hold in its window. Which blocks a chunk WANTS does not depend on who wins
a claim; a block wanted by one chunk is that chunk's, a block wanted by several is contested, and for those the plan
evaluates both outcomes. No size is written down here: tile, block, window, back blocks and the quarter come from
hj_own_layout_info, which reports the kernel's own constants.

A relation is described by its HOME SLOTS (relation() turns them into keys) or, for the bucketised table of --algo htm, by
its keys (home = first slot of bucket key / 3).
"""
import collections

import numpy as np

import htm_hashjoin_amd as hj
import wave_cases as wc

U64 = np.uint64
I64 = np.int64
EMPTY = (1 << 64) - 1


def layout(n, compute_units=256):
    """hj_own_layout_info without a device"""
    return hj.own_layout_info(n, compute_units)


def relation(homes, table_size, shift=0):
    """keys whose home slot is homes[i] in a table of table_size slots: ((home + table_size) << shift) | ones below the shift
    -- never 0, home slot 0 included"""
    h = np.asarray(homes, dtype=I64)
    assert h.min() >= 0 and h.max() < table_size
    keys = ((h + table_size).astype(U64) << U64(shift)) | U64((1 << shift) - 1)
    assert int(keys.max()) < 1 << 32
    return keys


def htm_table_size(n):
    nb = 1
    while nb < n // 3 + 1:
        nb *= 2
    return 4 * nb


# ---------------------------------------------------------------------------------------------------------------------
# phase A, restated
# ---------------------------------------------------------------------------------------------------------------------
Outcome = collections.namedtuple("Outcome", "deferred drops claimed slots used_lo used_hi1")
# deferred: [(slot reached, key, index)], drops: [(key, index)] in the order met, claimed: blocks the chunk got, slots: {slot:
# index << 32 | key} of those blocks, used_lo / used_hi1: lowest block and highest block + 1 claimed or deferred into (None, 0)


class Plan:
    """own_plan's answer. wanted[c] = blocks chunk c asks for, in the order it asks; wanters[b] = chunks that ask for block
    b; contested = blocks with more than one wanter; windows[c] = window base per tile (None before the first valid tuple)"""

    def __init__(self, geo, wanted, windows, simulate):
        self.geo = geo
        self.wanted, self.windows, self._simulate = wanted, windows, simulate
        self.n_chunks = len(wanted)
        self.wanters = collections.defaultdict(list)
        for c, blocks in enumerate(wanted):
            for b in blocks:
                self.wanters[b].append(c)
        self.contested = {b for b, w in self.wanters.items() if len(w) > 1}
        self._cache = {}

    def outcome(self, c, lost=frozenset()):
        """chunk c's phase A when it loses the claims on the blocks `lost` (and wins every other block it wants)"""
        lost = frozenset(lost) & set(self.wanted[c])
        if (c, lost) not in self._cache:
            self._cache[(c, lost)] = self._simulate(c, lost)
        return self._cache[(c, lost)]

    def chunk_contested(self, c):
        return self.contested & set(self.wanted[c])

    def bounds(self, c):
        """(lower, upper) deferred count of chunk c: it wins every contested block it wants / it loses every one. One
        tuple arriving at a block leaves at most one tuple (itself or the one it displaced) walking out of it, so holding
        more blocks never defers more."""
        return len(self.outcome(c).deferred), len(self.outcome(c, self.chunk_contested(c)).deferred)

    def assignment(self, pick):
        """one consistent run of phase A: contested block b goes to pick(wanters[b]); per chunk its Outcome"""
        winner = {b: pick(self.wanters[b]) for b in self.contested}
        return [self.outcome(c, {b for b in self.chunk_contested(c) if winner[b] != c}) for c in range(self.n_chunks)]

    def assignment_from(self, owner):
        """the run of phase A in which every contested block went to the chunk an owner table (0, or chunk + 1) names"""
        return self.assignment(lambda w: int(owner[next(b for b in self.contested if self.wanters[b] is w)]) - 1)

    def owner_table(self, outcomes):
        own = np.zeros(self.geo["numBlocks"], dtype=np.uint32)
        for c, o in enumerate(outcomes):
            for b in o.claimed:
                assert own[b] == 0
                own[b] = c + 1
        return own

    def valid_range(self, outcomes):
        """k_finalize_range: blocks [lo, hi + 1] of the blocks claimed or deferred into are probed; the whole table when
        that comes within a block of its end; nothing when nothing was touched"""
        los = [o.used_lo for o in outcomes if o.used_hi1]
        if not los:
            return 0, 0
        blk, ts = self.geo["blockSlots"], self.geo["tableSize"]
        lo, hi_ex = min(los) * blk, (max(o.used_hi1 for o in outcomes) + 1) * blk
        return (0, ts) if hi_ex + blk >= ts else (lo, hi_ex)

    def finish(self, outcomes):
        """phase B on top of the blocks phase A wrote: every deferred entry finishes its walk, sequentially. ->
        (table in the reference's format: key, 0 = empty; slots {slot: packed}; drops [(key, index)] of both phases)"""
        g = self.geo
        slots = {}
        for o in outcomes:
            slots.update(o.slots)
        drops = [d for o in outcomes for d in o.drops]
        for o in outcomes:
            for pos, key, idx in o.deferred:
                _walk(pos, (idx << 32) | key, slots, g, None, drops, None)
        table = np.zeros(g["tableSize"], dtype=U64)
        if slots:
            at = np.fromiter(slots.keys(), dtype=I64, count=len(slots))
            table[at] = np.fromiter((v & 0xFFFFFFFF for v in slots.values()), dtype=U64, count=len(slots))
        return table, slots, drops


def _home(key, g):
    if g["htm"]:
        return ((key // 3) << 2) & g["mask"]
    return (key >> g["shift"]) & g["mask"]


def _walk(pos, value, slots, g, held, drops, deferred):
    """one "insert tuple `value` from slot pos with what is left of its budget". held(block) -> the chunk holds the block in
    its window (None: phase B, every block is everybody's)"""
    mask, probe, bshift = g["mask"], g["probe"], g["blockShift"]
    while True:
        key = value & 0xFFFFFFFF
        if probe - ((pos - _home(key, g)) & mask) <= 0:
            drops.append((key, value >> 32))
            return
        if held is not None and not held(pos >> bshift):
            deferred.append((pos, key, value >> 32))
            return
        old = slots.get(pos, EMPTY)
        if old == EMPTY:
            slots[pos] = value
            return
        if old > value:
            slots[pos], value = value, old
        pos = (pos + 1) & mask


def own_plan(rel, lay, table_size, shift=0, probe=4, htm=False, idx_base=0):
    rel = np.asarray(rel, dtype=U64)
    n = rel.size
    blk, win, back, div, tile = lay["blockSlots"], lay["windowBlocks"], lay["backBlocks"], lay["seamDivisor"], lay["tileTuples"]
    chunk_len, n_chunks = lay["chunkLen"], lay["nChunks"]
    assert n_chunks == -(-n // chunk_len) and table_size >= lay["minTableSlots"] and probe <= lay["maxProbeLength"]
    assert blk & (blk - 1) == 0 and table_size % blk == 0
    num_blocks = table_size // blk
    geo = {"tableSize": table_size, "mask": table_size - 1, "shift": shift, "probe": probe, "htm": htm, "blockSlots": blk,
           "blockShift": blk.bit_length() - 1, "numBlocks": num_blocks}
    home_np, valid_np = wc.homes_of(rel, table_size, shift, htm)
    home, valid, keys = home_np.tolist(), valid_np.tolist(), (rel & U64(0xFFFFFFFF)).tolist()
    hb_np = home_np // blk
    eb_np = ((home_np + probe - 1) & (table_size - 1)) // blk

    # ---- which window each tile gets and which blocks it asks for: independent of who wins a claim
    tiles = []                                           # per chunk: [(first position, end, window base, blocks asked for)]
    for c in range(n_chunks):
        cb, ce = c * chunk_len, min((c + 1) * chunk_len, n)
        wb, tried, mine = None, set(), []
        for tb in range(cb, ce, tile):
            te = min(tb + tile, ce)
            v = valid_np[tb:te]
            hb, eb = hb_np[tb:te][v], eb_np[tb:te][v]
            if hb.size:
                nb = max(int(hb.min()) - back, 0)
                if nb + win > num_blocks:
                    nb = num_blocks - win
                if wb is None or nb > wb:                # never backwards
                    wb = nb
                    tried = {b for b in tried if b >= wb}            # the ring positions vacated stand for new blocks
            ask = []
            if wb is not None and hb.size:
                seam_tile = tb == cb or te == ce
                inside = (hb >= wb) & (hb < wb + win)
                flagged = set(np.unique(eb[(eb != hb) & (eb >= wb) & (eb < wb + win)]).tolist())     # straddle: always wanted
                blocks, counts = np.unique(hb[inside], return_counts=True)
                if seam_tile:
                    counted = {b: k for b, k in zip(blocks.tolist(), counts.tolist()) if b not in flagged}
                    mx = max(counted.values(), default=0)                # flags are not counts
                    flagged |= {b for b, k in counted.items() if k * div >= mx}
                else:
                    flagged |= set(blocks.tolist())
                ask = sorted(b for b in flagged if b not in tried)
                tried |= set(ask)
            mine.append((tb, te, wb, ask))
        tiles.append(mine)

    def simulate(c, lost):
        slots, deferred, drops, claimed = {}, [], [], set()
        used = []
        for tb, te, wb, ask in tiles[c]:
            got = [b for b in ask if b not in lost]
            claimed.update(got)
            used.extend(got)
            if wb is None:
                continue                                 # no valid tuple yet: nothing live in this tile either
            held = lambda b, wb=wb: wb <= b < wb + win and b in claimed         # noqa: E731
            before = len(deferred)
            for i in range(tb, te):
                if valid[i]:
                    _walk(home[i], ((idx_base + i) << 32) | keys[i], slots, geo, held, drops, deferred)
            used.extend(d[0] // blk for d in deferred[before:])
        return Outcome(deferred, drops, claimed, slots, min(used) if used else None, max(used) + 1 if used else 0)

    wanted = [[b for t in tiles[c] for b in t[3]] for c in range(n_chunks)]
    windows = [[t[2] for t in tiles[c]] for c in range(n_chunks)]
    return Plan(geo, wanted, windows, simulate)


def first_wanter(w):
    return min(w)


def last_wanter(w):
    return max(w)


# ---------------------------------------------------------------------------------------------------------------------
# bases: sorted home slots. off = slots before the first home (a multiple of the block keeps chunk seams on block ends)
# ---------------------------------------------------------------------------------------------------------------------
def base_dense(n, off=0):
    """homes off, off + 1, ...: every slot taken, a tile = tileTuples / blockSlots blocks (6)"""
    return off + np.arange(n, dtype=I64)


def base_gapped(n, off=0):
    """wave_cases' gapped base: dense without the slots = 16 (mod 32) -- a free slot every 32 ends a displacement"""
    return off + wc.base_gapped(n) - 1


def base_sparse(n, off=0):
    """two of every three slots (slots = 2 (mod 3) stay free): a tile spans 1.5 tileTuples slots (9 blocks), a chunk of
    16384 exactly 48 blocks"""
    i = np.arange(n, dtype=I64)
    return off + i + i // 2


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
# rel       8-byte tuples (value = key) or, keys32, the same keys as they go through hj_build_keys_dev
# moved     positions the constructor overwrote; twin = name of the case on the other side of the boundary (None: none)
# cause     tuples among `moved` (or, aim given, tuples at all) the plan must show deferred: the out twin's count, 0 for the in twin;
#           None = the case is about table and counters, not about a count
# aim       free text: what the case is aimed at
class Case:
    def __init__(self, name, family, rel, table_size, moved=(), probe=4, shift=0, keys32=False, htm=False, idx_base=0, twin=None,
                 cause=None, total=None, aim=""):
        self.name, self.family, self.rel, self.table_size = name, family, np.asarray(rel, dtype=U64), table_size
        self.moved, self.probe, self.shift, self.keys32, self.htm, self.idx_base = list(moved), probe, shift, keys32, htm, idx_base
        self.twin, self.cause, self.total, self.aim = twin, cause, total, aim
        self.n = self.rel.size

    def plan(self, lay=None):
        lay = lay or layout(self.n)
        return own_plan(self.rel, lay, self.table_size, self.shift, self.probe, self.htm, self.idx_base)

    def __repr__(self):
        return self.name


def moved_deferred(case, outcomes):
    """how many of the case's moved tuples phase A deferred"""
    want = {case.idx_base + p for p in case.moved}
    return sum(1 for o in outcomes for d in o.deferred if d[2] in want)


N1, N2, N4 = 1 << 14, 1 << 15, 1 << 16          # 1, 2 and 4 chunks on 256 compute units (asserted from the layout)


def _geo(n):
    lay = layout(n)
    return lay, lay["tileTuples"], lay["blockSlots"], lay["windowBlocks"], lay["backBlocks"]


def window_cases():
    """ahead_in / ahead_out, behind_in / behind_out on the sparse base, one chunk: tile t's homes fill blocks
    off/blk + 9 t .. + 8, its window starts backBlocks below"""
    out = []
    lay, tile, blk, win, back = _geo(N1)
    ts, off = 2 * N1, 4 * blk
    base = base_sparse(N1, off)
    first = lambda t: int(base[t * tile]) // blk            # noqa: E731   lowest home block of tile t
    free = lambda b: b * blk + (2 - (b * blk - off)) % 3    # noqa: E731   a slot of block b the base leaves free
    # a tuple of the middle tile homed in the window's last block / the first block past it, at a free slot
    t = 2
    wb = first(t) - back
    for name, block in (("ahead_in", wb + win - 1), ("ahead_out", wb + win)):
        h = base.copy()
        pos = t * tile + 1000
        h[pos] = free(block)
        assert h[pos] // blk == block and h[pos] not in base
        out.append(Case(name, "window", relation(h, ts), ts, [pos], twin="ahead_out" if name == "ahead_in" else "ahead_in",
                        cause=0 if name == "ahead_in" else 1, total=0 if name == "ahead_in" else 1,
                        aim=f"tile {t} (window {wb}..{wb + win - 1}): one tuple homed in block {block}"))
    # the NEXT tile's lowest home backBlocks / backBlocks + 1 below this tile's lowest: the window's first block against the
    # block before it. Behind the first window (tile 1 against tile 0's) and behind a window that has advanced (tile 3
    # against tile 2's). The straggler also holds the window back: the tile's own tuples past it are deferred in both
    # twins, the twins differ by the straggler alone.
    for tag, t in (("first", 0), ("advanced", 2)):
        wb = first(t) - back
        for side, block in (("in", wb), ("out", wb - 1)):
            h = base.copy()
            pos = (t + 1) * tile + 500
            h[pos] = free(block)
            beyond = int(np.count_nonzero(h[(t + 1) * tile:(t + 2) * tile] // blk >= wb + win))
            assert beyond > 0
            name = f"behind_{side}_{tag}"
            out.append(Case(name, "window", relation(h, ts), ts, [pos], twin=f"behind_{'out' if side == 'in' else 'in'}_{tag}",
                            cause=0 if side == "in" else 1, total=beyond + (0 if side == "in" else 1),
                            aim=f"tile {t + 1} holds a tuple homed in block {block}; the window stays at {wb}"))
    return out


def slide_cases():
    """consecutive tiles whose lowest home blocks differ by 15, 16, 17 and 40: dense base, two chunks; from tile 2 of chunk 0
    on every home is pushed up. Nothing is deferred: what leaves the window is complete, what enters is claimed afresh."""
    out = []
    lay, tile, blk, win, back = _geo(N2)
    ts = 2 * N2
    per_tile = tile // blk
    for d in (15, 16, 17, 40):
        h = base_dense(N2, 4 * blk)
        h[2 * tile:] += (d - per_tile) * blk
        assert int(h.max()) < ts and (int(h[2 * tile]) - int(h[tile])) // blk == d
        out.append(Case(f"slide_{d}", "slide", relation(h, ts), ts, total=0, aim=f"tile 2 of chunk 0 starts {d} blocks above tile 1"))
    return out


def table_end_cases():
    """dense homes up to the table's last slot (the clamp holds the window at the last windowBlocks blocks for the last
    tiles), and two more copies of the key homed in the last slot: their walks wrap and are deferred at slot 0"""
    out = []
    lay, tile, blk, win, back = _geo(N1)
    ts = 2 * N1
    h = base_dense(N1, ts - N1)
    h[-3:] = ts - 1
    for name, shift, keys32 in (("table_end", 0, False), ("table_end_keys_s0", 0, True), ("table_end_keys_s3", 3, True)):
        out.append(Case(name, "table_end", relation(h, ts, shift), ts, [N1 - 2, N1 - 1], shift=shift, keys32=keys32, cause=2, total=2,
                        aim="homes in the last blocks; two walks wrap from the last slot to slot 0"))
    return out


def straddle_cases():
    """four copies of a key homed two slots before a block's end, probeLength 4: two walk into the next block. In the middle
    of the window the next block is wanted through the straddle flag; from the window's LAST block the next one is outside
    and the two must be deferred, not written to ring position 0"""
    out = []
    lay, tile, blk, win, back = _geo(N1)
    ts, off = 2 * N1, 4 * blk
    base = base_sparse(N1, off)
    t = 2
    wb = int(base[t * tile]) // blk - back
    for name, block, cause in (("straddle_mid", wb + win - 2, 0), ("straddle_last", wb + win - 1, 2)):
        h = base.copy()
        pos = list(range(t * tile + 2000, t * tile + 2004))
        h[pos] = block * blk + blk - 2
        out.append(Case(name, "straddle", relation(h, ts), ts, pos, twin="straddle_last" if cause == 0 else "straddle_mid", cause=cause,
                        total=cause, aim=f"walks from slot {blk - 2} of block {block} (window {wb}..{wb + win - 1})"))
    # the same from the slots blk - 4 .. blk - 1, eight copies each at probeLength 8, inside the tile's own blocks
    h = base.copy()
    pos = []
    for k, s in enumerate(range(blk - 4, blk)):
        p = list(range(t * tile + 2000 + 8 * k, t * tile + 2008 + 8 * k))
        h[p] = (wb + back + 1 + k) * blk + s
        pos += p
    out.append(Case("straddle_508_511", "straddle", relation(h, ts), ts, pos, probe=8, cause=0, total=0,
                    aim="eight copies each from the last four slots of four blocks inside the window"))
    return out


def look_cases():
    """probeLength 8 on the dense base: a later copy of a key whose next slots all hold earlier tuples. Entering the retry
    round at slot blk - 4 (the last one that looks ahead: four slots, all lower, a recheck in the next block, where the
    budget runs out inside the look), at blk - 3 (no look: one slot at a time to the block's end) and well inside a block
    (skip 4, recheck, the budget ends in the second look). All are dropped; nothing is deferred."""
    out = []
    lay, tile, blk, win, back = _geo(N1)
    ts, off = 2 * N1, 4 * blk
    for name, slot in (("look_508", blk - 5), ("look_509", blk - 4), ("skip4_recheck", blk // 2)):
        h = base_dense(N1, off)
        t = 1
        home = (int(h[t * tile]) // blk + 1) * blk + slot           # held by a tuple of tile 1
        pos = t * tile + tile - 1                                      # the tile's last position: every slot ahead is lower
        assert home in h[t * tile:pos] and home + 8 in h[t * tile:pos]
        h[pos] = home
        out.append(Case(name, "look", relation(h, ts), ts, [pos], probe=8, cause=0, total=0,
                        aim=f"a later copy of the key homed at slot {slot} of a full block: enters the retry round at slot {slot + 1}"))
    return out


def quarter_cases():
    """seam tiles claim a block only if it holds at least 1/seamDivisor of the fullest block's tuples. One chunk, dense:
    the first tile's (and the last tile's) last tuples are split over two blocks so that the second holds exactly
    ceil(mx / 4) -- or one fewer, which are then deferred. And a chunk of ONE tile (first and last at once), as bare keys."""
    out = []
    lay, tile, blk, win, back = _geo(N1)
    div = lay["seamDivisor"]
    ts, off = 2 * N1, 4 * blk
    q = -(-blk // div)
    for where in ("first", "last"):
        for side, k in (("at", q), ("below", q - 1)):
            h = base_dense(N1, off)
            e = tile if where == "first" else N1        # the end of the first tile / of the last (short) one
            assert e % blk == 0 and (N1 // tile) * tile < N1 - blk
            nxt = int(h[e - 1]) + 1                     # first slot of the next block
            h[e - k:e] = nxt + q - k + np.arange(k)     # the tile's last block keeps blk - k tuples, the next block gets k
            h[e:] = nxt + q + np.arange(N1 - e)         # (first tile) the rest follows behind them: the twins differ in ONE tuple
            name = f"quarter_{side}_{where}"
            out.append(Case(name, "quarter", relation(h, ts), ts, list(range(e - k, e)),
                            twin=f"quarter_{'below' if side == 'at' else 'at'}_{where}", cause=0 if side == "at" else k,
                            total=0 if side == "at" else k, aim=f"{where} tile: a block with {k} tuples beside full blocks of {blk}"))
    # a chunk of one tile: 16384 + 1024 bare keys, chunk 1 = one tile of two full blocks... split the same way
    m = lay["chunkLen"] + 2 * blk
    lay_m = layout(m)
    assert lay_m["nChunks"] == 2 and m - lay_m["chunkLen"] <= tile
    ts_m = 1 << 16
    for side, k in (("at", q), ("below", q - 1)):
        h = base_dense(m, off)
        h[m - k:] = int(h[m - 1]) + 1 + q - k + np.arange(k)
        name = f"quarter_{side}_one_tile"
        out.append(Case(name, "quarter", relation(h, ts_m), ts_m, list(range(m - k, m)), keys32=True,
                        twin=f"quarter_{'below' if side == 'at' else 'at'}_one_tile", cause=0 if side == "at" else k,
                        total=0 if side == "at" else k, aim=f"a chunk of one tile: blocks of {blk}, {blk - k} and {k} tuples"))
    return out


def seam_cases():
    """chunk seams. contested_seam: dense keys with every seam in the middle of a block -- both neighbours want it.
    early_straggler: the last tuples of chunk 0 carry the keys of chunk 1's first tuples (lower index, same home slots):
    too few for chunk 0 to claim the block, so they are deferred, and phase B displaces what chunk 1 stored."""
    out = []
    lay, tile, blk, win, back = _geo(N4)
    ts = 2 * N4
    out.append(Case("contested_seam", "seam", relation(base_dense(N4, blk // 2), ts), ts, cause=None,
                    aim="dense keys, every chunk seam in the middle of a block"))
    out.append(Case("contested_seam_idx_base", "seam", relation(base_dense(N2, blk // 2), 2 * N2), 2 * N2, idx_base=12345, cause=None,
                    aim="the same on two chunks with idxBase = 12345"))
    lay, tile, blk, win, back = _geo(N2)
    ts, cl = 2 * N2, lay["chunkLen"]
    k = 100
    assert k * lay["seamDivisor"] < blk
    for probe in (1, 2, 4, 8):
        h = np.concatenate([base_dense(cl), base_gapped(N2 - cl, cl)])       # the seam on a block end; chunk 1 with free slots
        h[cl - k:cl] = h[cl:cl + k]
        out.append(Case(f"early_straggler_p{probe}", "seam", relation(h, ts), ts, list(range(cl - k, cl)), probe=probe, cause=k,
                        aim=f"{k} stragglers at the end of chunk 0 with the keys of chunk 1's first {k} tuples"))
    return out


def dup_cases():
    """one key 64, 65, tile and tile + 1 times and over a chunk seam (dense base, probeLength 4): the retry queue at its
    drain mark and beyond, drops"""
    out = []
    lay, tile, blk, win, back = _geo(N2)
    ts, cl = 2 * N2, lay["chunkLen"]
    for name, a, k in (("dup_64", tile + 100, 64), ("dup_65", tile + 100, 65), ("dup_tile", tile, tile), ("dup_tile_plus_1", tile, tile + 1),
                       ("dup_across_tile", 2 * tile - 700, 1500), ("dup_across_chunk", cl - 2000, 4000)):
        h = base_dense(N2, 4 * blk)
        h[a:a + k] = h[a]
        out.append(Case(name, "dup", relation(h, ts), ts, list(range(a, a + k)), cause=None, aim=f"one key {k} times from position {a}"))
    return out


def short_last_chunk_cases():
    """m = chunkLen + r bare keys, r around the wavefront and the tile"""
    out = []
    lay, tile, blk, win, back = _geo(N1)
    for r in (1, 63, 64, 65, tile - 1, tile, tile + 1):
        m = lay["chunkLen"] + r
        out.append(Case(f"short_last_chunk_r{r}", "short", relation(base_dense(m, 4 * blk), 1 << 16), 1 << 16, keys32=True, cause=None,
                        aim=f"a last chunk of {r} tuples"))
    return out


def htm_cases():
    """the bucketised table (home = first slot of bucket key / 3, probeLength 3; three keys per bucket, so sorted keys spread
    4/3 as wide: a tile spans 8 blocks)"""
    out = []
    lay, tile, blk, win, back = _geo(N1)
    ts = htm_table_size(N1)
    per_block = blk // 4 * 3                            # keys per block
    base = np.arange(1, N1 + 1, dtype=I64) + 4 * per_block
    hb = lambda key: ((int(key) // 3) << 2) // blk      # noqa: E731
    t = 2
    wb = hb(base[t * tile]) - back
    out.append(Case("htm_base", "htm", base.astype(U64), ts, htm=True, probe=3, cause=0, total=1,
                    aim="sorted keys, three per bucket; the first tile's last key is alone in its block: below the quarter"))
    for name, block in (("htm_ahead_in", wb + win - 1), ("htm_ahead_out", wb + win)):
        r = base.copy()
        pos = t * tile + 1000
        r[pos] = block * per_block + 4                   # bucket of a later tile: shares it with that tile's keys
        assert hb(r[pos]) == block
        out.append(Case(name, "htm", r.astype(U64), ts, [pos], htm=True, probe=3, twin="htm_ahead_out" if name == "htm_ahead_in" else "htm_ahead_in",
                        cause=0 if name == "htm_ahead_in" else 1, total=1 if name == "htm_ahead_in" else 2,
                        aim=f"tile {t}: one tuple homed in block {block} (window from {wb})"))
    # a bucket filled by in-window tuples, more copies (phase A's conflicts, in the chunk's slice) ...
    r = base.copy()
    r[t * tile + 500:t * tile + 506] = r[t * tile + 500]
    out.append(Case("htm_bucket_full", "htm", r.astype(U64), ts, list(range(t * tile + 500, t * tile + 506)), htm=True, probe=3, cause=0,
                    aim="six copies of one key inside a tile: the bucket is full, phase A lists the rest"))
    # ... and deferred ones: copies ahead of the window, earlier than the tuples that fill the bucket later -- phase B
    # displaces the stored ones, which become conflicts in the LAST slice
    r = base.copy()
    pos = list(range(t * tile + 1000, t * tile + 1005))
    r[pos] = (wb + win) * per_block + 7
    assert hb(r[pos[0]]) == wb + win
    out.append(Case("htm_deferred_conflicts", "htm", r.astype(U64), ts, pos, htm=True, probe=3, cause=5,
                    aim="five copies deferred past the window into a bucket a later tile fills: phase B's conflicts"))
    # the window's first block against the block before it: the NEXT tile holds a straggler homed backBlocks / backBlocks + 1
    # below this tile's lowest home block -- behind the first window and behind one that has advanced. The straggler holds
    # the window back, so the tile's own tuples past it are deferred in both twins; the twins differ by the straggler alone
    # (behind the advanced window its bucket is full of earlier tuples: a conflict of phase A inside, of phase B outside)
    aligned = np.arange(N1, dtype=I64) + 4 * per_block          # tiles start on block ends: a tile = 8 blocks of 384 keys
    assert tile % per_block == 0 and hb(aligned[tile]) == 4 + tile // per_block
    for tag, t in (("first", 0), ("advanced", 2)):
        wb = hb(aligned[t * tile]) - back
        for side, block in (("in", wb), ("out", wb - 1)):
            r = aligned.copy()
            pos = (t + 1) * tile + 500
            r[pos] = block * per_block + 5
            beyond = sum(1 for k in r[(t + 1) * tile:(t + 2) * tile] if hb(k) >= wb + win)
            assert hb(r[pos]) == block and beyond > 0
            out.append(Case(f"htm_behind_{side}_{tag}", "htm", r.astype(U64), ts, [pos], htm=True, probe=3,
                            twin=f"htm_behind_{'out' if side == 'in' else 'in'}_{tag}", cause=0 if side == "in" else 1,
                            total=beyond + (0 if side == "in" else 1),
                            aim=f"tile {t + 1} holds a tuple homed in block {block}; the window stays at {wb}"))
    # the quarter rule: the last keys of the first (last) tile move into the next block, exactly ceil(384 / 4) of them or one
    # fewer; the twins differ in one tuple
    q = -(-per_block // lay["seamDivisor"])
    for where in ("first", "last"):
        for side, k in (("at", q), ("below", q - 1)):
            r = aligned.copy()
            e = tile if where == "first" else N1
            nxt = (int(r[e - 1]) // per_block + 1) * per_block          # first key of the next block
            assert hb(r[e - q]) == hb(r[e - 1]) and int(r[e - 1]) - (nxt - per_block) + 1 - q >= q     # what stays is no straggler itself
            r[e - k:e] = nxt + q - k + np.arange(k)
            r[e:] = nxt + q + np.arange(N1 - e)
            out.append(Case(f"htm_quarter_{side}_{where}", "htm", r.astype(U64), ts, list(range(e - k, e)), htm=True, probe=3,
                            twin=f"htm_quarter_{'below' if side == 'at' else 'at'}_{where}", cause=0 if side == "at" else k,
                            total=0 if side == "at" else k, aim=f"{where} tile: a block with {k} keys beside blocks of {per_block}"))
    # a contested seam and early stragglers on two chunks
    lay2 = layout(N2)
    ts2 = htm_table_size(N2)
    cl = lay2["chunkLen"]
    base2 = np.arange(1, N2 + 1, dtype=I64)
    base2 += 4 * per_block + (per_block // 2 - int(base2[cl])) % per_block       # the seam in the middle of a block
    assert int(base2[cl]) % per_block == per_block // 2
    out.append(Case("htm_contested_seam", "htm", base2.astype(U64), ts2, htm=True, probe=3, cause=None,
                    aim="sorted keys on two chunks, the seam in the middle of a block"))
    r = np.arange(1, N2 + 1, dtype=I64) + 4 * per_block + (-int(cl + 1)) % per_block       # the seam on a block end
    assert int(r[cl]) % per_block == 0 and 60 * lay2["seamDivisor"] < per_block
    r[cl - 60:cl] = r[cl:cl + 60]
    out.append(Case("htm_early_straggler", "htm", r.astype(U64), ts2, list(range(cl - 60, cl)), htm=True, probe=3, cause=60, total=60,
                    aim="60 stragglers at the end of chunk 0 with the keys of chunk 1's first tuples"))
    return out


def defer_cases():
    lay, tile, blk, win, back = _geo(N1)
    return [Case("defer_all_small", "defer", defer_all(N1), 2 * N1, cause=None, total=N1 - tile - back * blk,
                 aim="a descending relation: the window never moves back, everything below it is deferred")]


def all_cases():
    out = []
    for f in (window_cases, slide_cases, table_end_cases, straddle_cases, look_cases, quarter_cases, seam_cases, dup_cases,
              short_last_chunk_cases, htm_cases, defer_cases):
        out += f()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def defer_all(n, copies=1):
    """a descending relation: every tile's lowest home is below the window, which never moves back -- everything but the
    first window's tuples is deferred. copies > 1: every key that many times, so that deferred tuples run out of budget"""
    return relation((np.arange(n - 1, -1, -1, dtype=I64) // copies) + n // 2, 2 * n)


def defer_all_counts(rel, lay, table_size):
    """deferred tuples per chunk of a descending relation, in closed form: the chunk's first tile places the window, and
    what is homed below it is deferred where it is homed"""
    home, _ = wc.homes_of(rel, table_size)
    blk = lay["blockSlots"]
    out = []
    for c in range(lay["nChunks"]):
        hb = home[c * lay["chunkLen"]:(c + 1) * lay["chunkLen"]] // blk
        wb = max(int(hb[:lay["tileTuples"]].min()) - lay["backBlocks"], 0)
        assert wb + lay["windowBlocks"] <= table_size // blk and int(hb.max()) < wb + lay["windowBlocks"]
        out.append(int(np.count_nonzero(hb < wb)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# shared by the CPU and the GPU tests: every case's plan, computed once; the plan against the sequential oracle
# ---------------------------------------------------------------------------------------------------------------------
CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}
_PLANS = {}


def plan_of(case, compute_units=256):
    key = (case.name, compute_units)
    if key not in _PLANS:
        _PLANS[key] = case.plan(layout(case.n, compute_units))
    return _PLANS[key]


def probe_side(rel):
    """every third tuple, and a few keys the relation does not hold"""
    rel = np.asarray(rel, dtype=U64)
    return np.concatenate([rel[::3], rel[:64] + U64(1 << 30)])


def htm_view(slots, drops, num_buckets):
    """a finished plan as the bucketised table: (tuples[bucket][3] in slot order, count per bucket, {bucket: sorted conflict
    keys})"""
    tuples = np.zeros((num_buckets, 3), dtype=U64)
    count = np.zeros(num_buckets, dtype=np.uint32)
    for slot, v in slots.items():
        assert slot % 4 < 3
        tuples[slot // 4, slot % 4] = v & 0xFFFFFFFF
        count[slot // 4] += 1
    chains = collections.defaultdict(list)
    for key, _ in drops:
        chains[(key // 3) % num_buckets].append(key)
    return tuples, count, {b: sorted(v) for b, v in chains.items()}


def oracle_htm_chains(want):
    """{bucket: sorted keys of its overflow chain} of an oracle.htm_build_probe_seq(..., want_buckets=True) result"""
    out = {}
    for b in np.flatnonzero(want["buckets"]["nextIndex"]).tolist():
        keys, cur = [], want["overflows"][want["buckets"][b]["nextIndex"]]
        while True:
            keys += [int(x) for x in cur["tuples"][:cur["count"]]]
            if cur["nextIndex"] == 0:
                break
            cur = want["overflows"][cur["nextIndex"]]
        out[b] = sorted(keys)
    return out
