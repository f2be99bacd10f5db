"""Case table and a plain plan for the LDS chain phase of the bucketised table (HJ_ALGO_HTM behind buildVariant 3:
k_htm_chain_count / k_htm_chain_fill in hj_htm.hip, and the router of the deferred phase in hj_build_wave.hip).

No GPU and no pytest fixtures in here: test_htm_chain_cases.py checks on the CPU that every constructor has the property it
is named for, test_gpu_htm_chains.py runs the table on the device. What a build must give comes from the sequential oracle;
WHETHER the LDS phase must hold or hand over, and for which cause, comes from chain_plan, a numpy restatement written from
the kernels' comments. No cap is written down here: they come from hj_htm_chain_layout_info (the kernel's own constants),
the chunk geometry from hj_wave_layout_info, the seams from wave_cases.expected_seams (or the device's hj_wave_seams).

The rules restated (hj_htm.hip "chains along the rings", hj_table.h the table of causes):
  * a conflict is a tuple that finds its bucket (key / 3) & (numBuckets - 1) full: all but the three lowest-indexed tuples
    of a bucket;
  * the conflict list has one slice of sliceLen places per chunk; a conflict is filed under the chunk that owns its
    bucket's granule (32 buckets): the LAST chunk whose first granule bounds[c] is not above it, chunk 0 for everything
    below (the router's binary search); what the wavefront of a chunk lists itself lies in its own range, so slice c holds
    exactly the conflicts of the granules [bounds[c], bounds[c + 1]) -- chunk 0 also what lies below, the last chunk what
    lies above. A chunk whose range is empty (equal bounds) gets nothing;
  * per slice, in this order: m conflicts > sliceLen: bit 0, nothing else is looked at. A conflict outside
    [B0, B1) = [c ? 32 * bounds[c] : 0, last ? numBuckets : 32 * bounds[c + 1]): bit 1; E0 = lowest conflict bucket,
    span = highest - E0 + 1 > chainCountCap: bit 2; sub = ceil(span / parts) > chainCap: bit 3 (bits 1 to 3 together).
    Else part p takes the buckets [E0 + p * sub, E0 + (p + 1) * sub) and needs the sum of ceil(conflicts / 3) over them
    overflow buckets; three times that > chainCap: bit 4;
  * the mask the device reports is a non-empty subset of the union over the slices (later workgroups return early).

Relations are near-sorted keys (value = key): a dense base 1 .. n (key k at position k - 1: three keys per bucket, no
conflict anywhere) with a few stretches overwritten. The constructors keep n."""
import collections

import numpy as np

import htm_hashjoin_amd as hj
import wave_cases as wc

U64 = np.uint64
I64 = np.int64

# hj_htm_chain_info: out[1]
BIT_SLICE_FULL, BIT_STRAY, BIT_SPAN, BIT_SUB, BIT_IMAGE = 1, 2, 4, 8, 16
HELD, HANDED_OVER = 1, 2

SMALL = 1 << 16                     # the size of the one-part cases: 32 chunks on 256 compute units


def num_buckets(n):
    nb = 1
    while nb < n // 3 + 1:
        nb *= 2
    return nb


def layouts(n, compute_units):
    """(hj_wave_layout_info, hj_htm_chain_layout_info) without a device"""
    return hj.wave_layout_info(n, compute_units), hj.htm_chain_layout_info(n, compute_units)


def buckets_of(keys, nb):
    return ((np.asarray(keys, dtype=U64) & U64(0xFFFFFFFF)) // U64(3)).astype(I64) & I64(nb - 1)


def seams(R, lay):
    """the ring pre-pass on the bucketised home slots: (starts, bounds)"""
    return wc.expected_seams(R, lay, 4 * num_buckets(R.size), htm=True)


def tries_rule(n, lay, chain_lay):
    """hj_htm_chain_layout_info's `tries`, restated from build_htm: a request for buildVariant 3 tries the LDS phase when the
    rings take the table at all (4 slots per bucket, at least one ring of slots) and the phase's scratch -- a word per part
    and one more; two words per slice and per part -- fits an array of one word per bucket. Returns 0 or 1."""
    nb = num_buckets(n)
    rings = 4 * nb >= lay["ringGranules"] * lay["granuleSlots"]
    n_parts = chain_lay["slices"] * chain_lay["parts"]
    scratch = n_parts + 1 <= nb and 2 * chain_lay["slices"] * (1 + chain_lay["parts"]) <= nb
    return int(rings and scratch)


def rings_boundary(compute_units=None, ctx=None):
    """(the largest n whose table the rings refuse, that n + 1) by the layout call"""
    info = (lambda n: ctx.htm_chain_layout_info(n)) if ctx is not None else (lambda n: hj.htm_chain_layout_info(n, compute_units))
    n = max(k for k in range(1, 1 << 13) if not info(k)["tries"])
    assert info(n + 1)["tries"] and all(info(k)["tries"] for k in (n + 2, n + 100, 1 << 13, 1 << 20))
    return n, n + 1


def duplicates(n, seed=3):
    """n near-sorted keys with many duplicates (a third as many distinct keys): chains of several overflow buckets"""
    rng = np.random.default_rng(seed)
    return np.sort(rng.integers(1, max(2, n // 3), size=n, dtype=U64))


def smallest_n_with_parts(parts, compute_units, below=1 << 25, ctx=None):
    """the smallest n whose slices are cut into `parts` parts (bisection on hj_htm_chain_layout_info: sliceLen grows with n),
    or None when there is none below `below`"""
    info = (lambda n: ctx.htm_chain_layout_info(n)) if ctx is not None else (lambda n: hj.htm_chain_layout_info(n, compute_units))
    if info(below - 1)["parts"] < parts:
        return None
    lo, hi = 1, below - 1                       # parts(lo) < parts <= parts(hi)
    if info(lo)["parts"] >= parts:
        return lo
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if info(mid)["parts"] >= parts:
            hi = mid
        else:
            lo = mid
    return hi if info(hi)["parts"] == parts else None


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
def conflicts_of(R, nb):
    """positions (ascending) of the oracle's conflicts: all but the three lowest-indexed tuples of every bucket"""
    R = np.asarray(R, dtype=U64)
    assert ((R >> U64(32)) == 0).all() and (R != 0).all()
    b = buckets_of(R, nb)
    per = np.bincount(b, minlength=nb)
    pos = np.flatnonzero(per[b] > 3)            # only tuples of buckets that overflow are looked at
    order = np.argsort(b[pos], kind="stable")
    pos, bs = pos[order], b[pos][order]
    first = np.flatnonzero(np.r_[True, bs[1:] != bs[:-1]])
    rank = np.arange(bs.size) - np.repeat(first, np.diff(np.r_[first, bs.size]))
    return np.sort(pos[rank >= 3])


Plan = collections.namedtuple(
    "Plan", "parts m E0 span sub slice_cause groups mask strays conflicts owner bucket cb_owner cb_bucket cb_count total_groups")
# parts         parts per slice
# m, E0, span, sub   per slice (int64; E0 = span = sub = 0 where m == 0 or the slice is over its length)
# slice_cause   per slice: the bits that slice's workgroup raises
# groups        [slices, parts]: overflow buckets per part (0 for a slice that raises bits 0 to 3)
# mask          union of slice_cause: 0 = the phase must hold
# strays        conflicts outside the bucket range of the slice they are filed under (bit 1's count)
# conflicts, owner, bucket   per conflict: position in R, slice, bucket
# cb_*          per (slice, bucket) with conflicts: slice, bucket, conflicts
# total_groups  overflow buckets of the whole table (= the oracle's overflowBuckets)


def chain_plan(R, lay, chain_lay, bounds):
    R = np.asarray(R, dtype=U64)
    nb = num_buckets(R.size)
    n_slices, slice_len, parts = chain_lay["slices"], chain_lay["sliceLen"], chain_lay["parts"]
    assert n_slices == lay["nChunks"] and slice_len == lay["sliceLen"]
    per_gran = lay["granuleSlots"] // 4                                      # buckets per granule
    bounds = np.asarray(bounds, dtype=I64)
    assert bounds.size == n_slices + 1
    conf = conflicts_of(R, nb)
    bkt = buckets_of(R[conf], nb)
    # the router: the last chunk whose first granule is not above the conflict's, chunk 0 below every range
    owner = np.maximum(np.searchsorted(bounds[:n_slices], bkt // per_gran, side="right") - 1, 0)
    # the count kernel's own idea of what a slice owns
    B0 = bounds[:n_slices] * per_gran
    B0[0] = 0
    B1 = bounds[1:] * per_gran
    B1[-1] = nb
    stray = (bkt < B0[owner]) | (bkt >= B1[owner])
    m = np.bincount(owner, minlength=n_slices).astype(I64)
    E0, span, sub = (np.zeros(n_slices, dtype=I64) for _ in range(3))
    cause = np.zeros(n_slices, dtype=I64)
    groups = np.zeros((n_slices, parts), dtype=I64)
    cause[m > slice_len] = BIT_SLICE_FULL
    key = owner * nb + bkt
    ukey, cnt = np.unique(key, return_counts=True)
    cb_owner, cb_bucket = ukey // nb, ukey % nb
    stray_in = np.bincount(owner, weights=stray, minlength=n_slices)
    cut = np.searchsorted(cb_owner, np.arange(n_slices + 1))                  # ukey is sorted by slice, then bucket
    for c in np.flatnonzero((m > 0) & (m <= slice_len)).tolist():
        bs, ks = cb_bucket[cut[c]:cut[c + 1]], cnt[cut[c]:cut[c + 1]]
        E0[c], span[c] = bs[0], bs[-1] - bs[0] + 1
        sub[c] = -(-span[c] // parts)
        if stray_in[c]:
            cause[c] |= BIT_STRAY
        if span[c] > chain_lay["chainCountCap"]:
            cause[c] |= BIT_SPAN
        if sub[c] > chain_lay["chainCap"]:
            cause[c] |= BIT_SUB
        if cause[c]:
            continue
        np.add.at(groups[c], (bs - E0[c]) // sub[c], (ks + 2) // 3)
        if (3 * groups[c] > chain_lay["chainCap"]).any():
            cause[c] |= BIT_IMAGE
    return Plan(parts, m, E0, span, sub, cause, groups, int(np.bitwise_or.reduce(cause)) if n_slices else 0, int(stray.sum()),
                conf, owner, bkt, cb_owner, cb_bucket, cnt, int(((cnt + 2) // 3).sum()))


def plan_for(R, compute_units):
    lay, chain_lay = layouts(R.size, compute_units)
    return chain_plan(R, lay, chain_lay, seams(R, lay)[1])


# ---------------------------------------------------------------------------------------------------------------------
# a vectorised chain view
# ---------------------------------------------------------------------------------------------------------------------
def chains_view(buckets, overflows):
    """oracle.htm_chains without a Python loop per bucket: (flat tuple array, offsets) -- per primary bucket the tuples it
    holds, then those of its overflow chain in walk order. One numpy step per chain LEVEL, over the buckets whose chain
    goes on; a chain longer than the overflow area has a cycle."""
    nbk = buckets.size
    ids = np.flatnonzero(buckets["nextIndex"])
    nxt = buckets["nextIndex"][ids].astype(I64)
    total = np.minimum(buckets["count"].astype(I64), 3)                        # (oracle.htm_chains: tuples[:count] of three)
    levels = [(np.arange(nbk), buckets["tuples"], total.copy())]
    while ids.size:
        assert len(levels) <= overflows.size, "a chain that does not end"
        assert (nxt < overflows.size).all(), "a link beyond the overflow area"
        node = overflows[nxt]
        count = np.minimum(node["count"].astype(I64), 3)
        levels.append((ids, node["tuples"], count))
        np.add.at(total, ids, count)
        keep = node["nextIndex"] != 0
        ids, nxt = ids[keep], node["nextIndex"][keep].astype(I64)
    off = np.concatenate([[0], np.cumsum(total)]).astype(I64)
    flat = np.zeros(off[-1], dtype=U64)
    pos = off[:-1].copy()
    for ids, tuples, count in levels:
        for j in range(3):
            sel = count > j
            flat[pos[ids[sel]] + j] = tuples[sel, j]
        pos[ids] += count
    return flat, off


# ---------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------
def dense(n, first_key=1):
    """keys first_key .. first_key + n - 1 in order: three per bucket, no conflict"""
    return np.arange(first_key, first_key + n, dtype=U64)


def run_keys(runs):
    """[(bucket, tuples), ...] -> that many keys of each bucket (3b, 3b + 1, 3b + 2, 3b, ...), in the order given"""
    return np.concatenate([U64(3 * b) + (np.arange(k, dtype=U64) % U64(3)) for b, k in runs])


def write_run(R, pos, runs):
    """overwrite R from position pos on with run_keys(runs); returns the first position behind the run"""
    keys = run_keys(runs)
    assert 0 <= pos and pos + keys.size <= R.size and all(b > 0 for b, _ in runs)
    R[pos:pos + keys.size] = keys
    return pos + keys.size


def bucket_at(R, pos):
    return int(R[pos]) // 3


def far_positions(lay, chunks, count, offset=None):
    """`count` positions in the middle of the given chunks (spread evenly over them, ascending): behind the positions the
    seam of the chunk is placed among (its first `look`), before its tail"""
    offset = lay["look"] + 64 if offset is None else offset
    per = -(-count // len(chunks))
    assert offset + per <= lay["chunkLen"] - lay["tail"] - 64, (per, lay["chunkLen"])
    pos = np.concatenate([c * lay["chunkLen"] + offset + np.arange(per) for c in chunks])[:count]
    return pos.astype(I64)


def sparse_chunk(n, lay, c, stride):
    """the dense relation with chunk c's positions `stride` buckets apart (one tuple per bucket it touches); the chunks
    behind it go on densely above it"""
    L = lay["chunkLen"]
    R = dense(n)
    p = c * L
    k0 = int(R[p])
    k0 += (-k0) % 3                                                          # the first key of a bucket
    R[p:p + L] = U64(k0) + U64(3 * stride) * np.arange(L, dtype=U64)
    top = k0 + 3 * stride * L
    R[p + L:] = U64(top) + np.arange(n - p - L, dtype=U64)
    assert int(R.max()) // 3 < num_buckets(n), "the keys wrap around the table"
    return R


# ---------------------------------------------------------------------------------------------------------------------
# constructors, one part per slice
# ---------------------------------------------------------------------------------------------------------------------
TAIL_COUNTS = (3, 4, 5, 6, 7, 9, 10)


def tail_counts(n, lay, chain_lay):
    """buckets with 3, 4, 5, 6, 7, 9 and 10 tuples side by side, in the middle of a chunk: last overflow buckets with 1, 2
    and 3 tuples, chains of 0, 1, 2 and 3 buckets"""
    R = dense(n)
    pos = 7 * lay["chunkLen"] + lay["chunkLen"] // 2
    b = bucket_at(R, pos) + 1
    pos = 3 * b - 1
    write_run(R, pos, [(b + i, k) for i, k in enumerate(TAIL_COUNTS)])
    return R, dict(first_bucket=b)


def span_pair(n, lay, chain_lay, c, gap):
    """a sparse chunk c (a tuple in every second bucket) with two conflict buckets `gap` buckets apart (span = gap + 1),
    four tuples each, written over four neighbouring positions so that the keys stay sorted"""
    R = sparse_chunk(n, lay, c, 2)
    p = c * lay["chunkLen"] + lay["look"] + 64
    a = bucket_at(R, p)
    q = p + gap // 2
    assert q + 4 < (c + 1) * lay["chunkLen"] - lay["tail"] - 64 and bucket_at(R, q - 1) < a + gap < bucket_at(R, q + 4)
    write_run(R, p, [(a, 4)])
    write_run(R, q, [(a + gap, 4)])
    return R, dict(chunk=c, lo=a, hi=a + gap)


def sub_at_cap(n, lay, chain_lay, over=False):
    """one part per slice: sub = span = chainCap (over: chainCap + 1, bit 3)"""
    assert chain_lay["parts"] == 1
    return span_pair(n, lay, chain_lay, 9, chain_lay["chainCap"] - 1 + (1 if over else 0))


def slice_full(n, lay, chain_lay, over=False):
    """one bucket with 3 + sliceLen copies of a key (over: one more, bit 0): some in the chunk that owns the bucket, the
    rest in two far chunks, whose conflicts the router files under the owner"""
    R = dense(n)
    L, S = lay["chunkLen"], lay["sliceLen"]
    own = 5
    pos = own * L + L // 4
    b = bucket_at(R, pos) + 1
    here = L // 2
    write_run(R, 3 * b - 1, [(b, here)])
    rest = 3 + S + (1 if over else 0) - here
    far = far_positions(lay, (lay["nChunks"] - 12, lay["nChunks"] - 6), rest)
    R[far] = run_keys([(b, rest)])
    return R, dict(chunk=own, bucket=b, routed=rest)


def image_at_cap(n, lay, chain_lay, over=False):
    """chainCap / 3 overflow buckets in one part (over: one more, bit 4), one conflict each: a chunk with one tuple per
    bucket, and three more tuples for each of the first chainCap / 3 buckets of its range in two far chunks -- the last of
    the four is the conflict, routed to the owner"""
    assert chain_lay["parts"] == 1
    c = 6
    R = sparse_chunk(n, lay, c, 1)
    want = chain_lay["chainCap"] // 3 + (1 if over else 0)
    bounds = seams(R, lay)[1]
    per_gran = lay["granuleSlots"] // 4
    lo = int(bounds[c]) * per_gran + 8
    assert lo + want <= int(bounds[c + 1]) * per_gran, "the chunk's range is too short for the case"
    extra = np.repeat(np.arange(lo, lo + want, dtype=U64) * U64(3), 3) + np.tile(np.arange(3, dtype=U64), want)
    far_chunks = (lay["nChunks"] - 14, lay["nChunks"] - 10, lay["nChunks"] - 6)
    R[far_positions(lay, far_chunks, extra.size)] = extra
    return R, dict(chunk=c, lo=lo, buckets=want)


def outside_ranges(n, lay, chain_lay):
    """keys from bucket 600 on, so that chunk 0's range starts well above the table's first granules; conflicts in bucket 5
    (below every range: chunk 0's) and far above the last chunk's keys (the last chunk's), one more conflict bucket inside
    each of the two ranges"""
    R = dense(n, 3 * 600)
    nb = num_buckets(n)
    L = lay["chunkLen"]
    write_run(R, L // 2, [(bucket_at(R, L // 2) + 1, 8)])                                   # inside chunk 0's range
    last = lay["nChunks"] - 1
    p = last * L + L // 2
    inside = bucket_at(R, p) + 1
    write_run(R, 3 * (inside - 600) , [(inside, 7)])                                        # inside the last chunk's range
    above = int(R.max()) // 3 + 1000
    assert above < nb
    far = far_positions(lay, (3, last - 3), 12)
    R[far[:6]] = run_keys([(5, 6)])
    R[far[6:]] = run_keys([(above, 6)])
    return R, dict(below=5, above=above)


def empty_slices(n, lay, chain_lay):
    """loaded slices with empty ones between them, and three chunks with equal bounds: chunks e + 1 and e + 2 hold keys of
    the table's (free) low buckets, so their samples lie below chunk e's range and the prefix maximum gives all three the
    same first granule. Chunks e and e + 1 own nothing; the conflicts of chunk e's keys belong under chunk e + 2"""
    L = lay["chunkLen"]
    e = 12
    assert lay["nChunks"] >= e + 8
    first = 3 * (2 * L // 3 + 64)                                                          # the base starts above 2 L free keys
    R = np.empty(n, dtype=U64)
    low = np.arange((e + 1) * L, (e + 3) * L)
    normal = np.ones(n, dtype=bool)
    normal[low] = False
    R[normal] = dense(n - low.size, first)
    R[low] = dense(low.size, 3)
    for c, k in ((3, 5), (6, 11), (9, 4), (e, 9), (e + 5, 6)):
        p = c * L + L // 2
        write_run(R, p, [(bucket_at(R, p) + 1, k), (bucket_at(R, p) + 2, 3), (bucket_at(R, p) + 3, 7)])
    assert int(R.max()) // 3 < num_buckets(n)
    return R, dict(equal=(e, e + 1, e + 2), loaded=(3, 6, 9, e + 2, e + 5))


# ---------------------------------------------------------------------------------------------------------------------
# constructors, two or more parts per slice
# ---------------------------------------------------------------------------------------------------------------------
def _mid(lay, c):
    return c * lay["chunkLen"] + lay["chunkLen"] // 2


def part_boundary(n, lay, chain_lay):
    """chains in the buckets E0, E0 + sub - 1 (the last of part 0), E0 + sub (the first of part 1) and E0 + 2 sub - 1"""
    assert chain_lay["parts"] >= 2
    R = dense(n)
    c, s = 40, 50
    b = bucket_at(R, _mid(lay, c)) + 1
    write_run(R, 3 * b - 1, [(b, 5)])
    write_run(R, 3 * (b + s - 1) - 1, [(b + s - 1, 7), (b + s, 4)])
    write_run(R, 3 * (b + 2 * s - 1) - 1, [(b + 2 * s - 1, 10)])
    return R, dict(chunk=c, E0=b, sub=s, span=2 * s)


def ragged_span(n, lay, chain_lay):
    """span = 2 s + 1 is no multiple of two parts: sub = s + 1, part 1 is one bucket shorter; chains in the first and the
    last bucket of the span and on both sides of the boundary"""
    assert chain_lay["parts"] == 2
    R = dense(n)
    c, s = 50, 37
    b = bucket_at(R, _mid(lay, c)) + 1
    write_run(R, 3 * b - 1, [(b, 6)])
    write_run(R, 3 * (b + s) - 1, [(b + s, 5), (b + s + 1, 8)])
    write_run(R, 3 * (b + 2 * s) - 1, [(b + 2 * s, 7)])
    return R, dict(chunk=c, E0=b, sub=s + 1, span=2 * s + 1)


def empty_part(n, lay, chain_lay):
    """a slice whose conflicts lie in one bucket: span = sub = 1, every part but the first has no groups"""
    assert chain_lay["parts"] >= 2
    R = dense(n)
    c = 60
    b = bucket_at(R, _mid(lay, c)) + 1
    write_run(R, 3 * b - 1, [(b, 11)])
    return R, dict(chunk=c, E0=b)


def interleaved_parts(n, lay, chain_lay, seed=7):
    """2 s neighbouring buckets with six tuples each, shuffled over a window of 128 positions: the conflicts of the two parts
    are mixed in input order around the boundary, so the parts' stretches of the list overlap and the fill's bucket filter
    decides"""
    assert chain_lay["parts"] == 2
    R = dense(n)
    c, s = 70, 20
    b = bucket_at(R, _mid(lay, c)) + 1
    keys = run_keys([(b + i, 6) for i in range(2 * s)])
    rng = np.random.default_rng(seed)
    keys = keys[np.argsort(np.arange(keys.size) + rng.uniform(0, 128, size=keys.size), kind="stable")]
    p = 3 * b - 1
    R[p:p + keys.size] = keys
    return R, dict(chunk=c, E0=b, sub=s, span=2 * s)


def one_key_image(n, lay, chain_lay, over=False):
    """3 + chainCap copies of one key in a single chunk (over: one more, bit 4): one bucket with k = chainCap conflicts --
    the largest count the packed counter word of the fill has to carry -- and chainCap / 3 overflow buckets in one chain"""
    assert chain_lay["parts"] >= 2 and 3 + chain_lay["chainCap"] + 1 + lay["look"] + lay["tail"] + 192 < lay["chunkLen"]
    R = dense(n)
    c = 80
    p = c * lay["chunkLen"] + lay["look"] + 128
    b = bucket_at(R, p) + 1
    write_run(R, 3 * b - 1, [(b, 3 + chain_lay["chainCap"] + (1 if over else 0))])
    return R, dict(chunk=c, bucket=b)


def span_at_cap(n, lay, chain_lay, over=False):
    """five or more parts: a sparse chunk whose two conflict buckets span exactly chainCountCap buckets (over: one more,
    bit 2 -- sub stays below chainCap)"""
    assert chain_lay["chainCountCap"] // chain_lay["parts"] < chain_lay["chainCap"]
    return span_pair(n, lay, chain_lay, 100, chain_lay["chainCountCap"] - 1 + (1 if over else 0))


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
# name -> (constructor, keyword arguments, state the LDS phase must report, the bit a hand-over must carry)
Case = collections.namedtuple("Case", "name make kw state bit")

ONE_PART = [
    Case("tail_counts", tail_counts, {}, HELD, 0),
    Case("sub_at_cap", sub_at_cap, {}, HELD, 0),
    Case("sub_over_cap", sub_at_cap, dict(over=True), HANDED_OVER, BIT_SUB),
    Case("slice_full", slice_full, {}, HELD, 0),
    Case("slice_over", slice_full, dict(over=True), HANDED_OVER, BIT_SLICE_FULL),
    Case("image_at_cap", image_at_cap, {}, HELD, 0),
    Case("image_over_cap", image_at_cap, dict(over=True), HANDED_OVER, BIT_IMAGE),
    Case("outside_ranges", outside_ranges, {}, HELD, 0),
    Case("empty_slices", empty_slices, {}, HELD, 0),
]
TWO_PARTS = [
    Case("part_boundary", part_boundary, {}, HELD, 0),
    Case("interleaved_parts", interleaved_parts, {}, HELD, 0),
    Case("empty_part", empty_part, {}, HELD, 0),
    Case("ragged_span", ragged_span, {}, HELD, 0),
    Case("one_key_image_at_cap", one_key_image, {}, HELD, 0),
    Case("one_key_image_over_cap", one_key_image, dict(over=True), HANDED_OVER, BIT_IMAGE),
]
FIVE_PARTS = [
    Case("span_at_cap", span_at_cap, {}, HELD, 0),
    Case("span_over_cap", span_at_cap, dict(over=True), HANDED_OVER, BIT_SPAN),
]
BY_NAME = {c.name: c for c in ONE_PART + TWO_PARTS + FIVE_PARTS}


def check_property(case, R, what, plan, lay, chain_lay):
    """the property the case is named for, on the plan (assertions): a device run of the case is never vacuous"""
    name = case.name
    assert plan.strays == 0, (name, "a conflict filed under a chunk that does not own its bucket")
    assert plan.mask == (case.bit if case.state == HANDED_OVER else 0), (name, plan.mask)
    nb = num_buckets(R.size)
    per = np.bincount(buckets_of(R, nb), minlength=nb)
    conf_per = dict(zip(plan.cb_bucket.tolist(), plan.cb_count.tolist()))
    if name == "tail_counts":
        b = what["first_bucket"]
        assert per[b:b + len(TAIL_COUNTS)].tolist() == list(TAIL_COUNTS)
        assert [conf_per.get(b + i, 0) for i in range(len(TAIL_COUNTS))] == [k - 3 for k in TAIL_COUNTS]
        assert len({int(o) for o in plan.cb_owner[(plan.cb_bucket >= b) & (plan.cb_bucket < b + len(TAIL_COUNTS))]}) == 1
    elif name in ("sub_at_cap", "sub_over_cap", "span_at_cap", "span_over_cap"):
        c = what["chunk"]
        cap = chain_lay["chainCap"] if name.startswith("sub") else chain_lay["chainCountCap"]
        assert plan.m[c] == 2 and plan.span[c] == cap + (1 if case.state == HANDED_OVER else 0), (name, plan.m[c], plan.span[c])
        if name.startswith("sub"):
            assert plan.sub[c] == plan.span[c] and plan.span[c] <= chain_lay["chainCountCap"]
        else:
            assert plan.sub[c] <= chain_lay["chainCap"]
        assert np.count_nonzero(plan.m) == 1
    elif name in ("slice_full", "slice_over"):
        c = what["chunk"]
        assert plan.m[c] == lay["sliceLen"] + (1 if name == "slice_over" else 0) and np.count_nonzero(plan.m) == 1
        assert per[what["bucket"]] == 3 + plan.m[c]
        far = plan.conflicts[plan.conflicts >= (c + 2) * lay["chunkLen"]]
        assert far.size == what["routed"] and far.size > lay["chunkLen"] // 2            # filed by the router, not by the chunk
        if name == "slice_full":
            assert 3 * plan.groups[c, 0] <= chain_lay["chainCap"]
    elif name in ("image_at_cap", "image_over_cap"):
        c = what["chunk"]
        assert plan.groups[c, 0] == plan.m[c] == what["buckets"] and np.count_nonzero(plan.m) == 1
        assert 3 * plan.groups[c, 0] == chain_lay["chainCap"] + (3 if name == "image_over_cap" else 0)
        assert plan.m[c] <= lay["sliceLen"] and plan.sub[c] <= chain_lay["chainCap"]
        assert (plan.conflicts >= (c + 2) * lay["chunkLen"]).all()                         # every one of them routed
    elif name == "outside_ranges":
        bounds = seams(R, lay)[1]
        per_gran = lay["granuleSlots"] // 4
        last = lay["nChunks"] - 1
        assert what["below"] < bounds[0] * per_gran and plan.E0[0] == what["below"] and plan.m[0] > 3
        top = int(R[(last - 1) * lay["chunkLen"]:].max()) // 3
        assert what["above"] > top and plan.E0[last] + plan.span[last] - 1 == what["above"] and plan.m[last] > 3
        assert plan.span[0] > 500 and plan.span[last] > 500                                # own conflicts and outside ones in one slice
    elif name == "empty_slices":
        bounds = seams(R, lay)[1]
        e0, e1, e2 = what["equal"]
        assert bounds[e0] == bounds[e1] == bounds[e2] < bounds[e2 + 1]
        assert plan.m[e0] == 0 and plan.m[e1] == 0 and plan.m[e2] > 0
        mine = (plan.owner == e2)
        assert ((plan.conflicts[mine] // lay["chunkLen"]) == e0).all()                     # chunk e's tuples, under the last of the equal chunks
        assert sorted(np.flatnonzero(plan.m).tolist()) == sorted(what["loaded"])
    elif name in ("part_boundary", "ragged_span", "interleaved_parts"):
        c = what["chunk"]
        assert (plan.E0[c], plan.span[c], plan.sub[c]) == (what["E0"], what["span"], what["sub"]), (name, plan.E0[c], plan.span[c], plan.sub[c])
        E0, sub = what["E0"], what["sub"]
        assert (plan.groups[c, :2] > 0).all()
        if name == "part_boundary":
            assert all(conf_per.get(b, 0) > 0 for b in (E0, E0 + sub - 1, E0 + sub, E0 + 2 * sub - 1))
        elif name == "ragged_span":
            assert what["span"] % plan.parts != 0
            assert all(conf_per.get(b, 0) > 0 for b in (E0, E0 + sub - 1, E0 + sub, E0 + what["span"] - 1))
        else:
            mine = plan.owner == c
            p0 = plan.conflicts[mine & (plan.bucket < E0 + sub)]
            p1 = plan.conflicts[mine & (plan.bucket >= E0 + sub)]
            assert np.count_nonzero(p0 > p1.min()) >= 3 and np.count_nonzero(p1 < p0.max()) >= 3   # mixed in input order
    elif name == "empty_part":
        c = what["chunk"]
        assert plan.span[c] == 1 and plan.groups[c, 0] > 0 and (plan.groups[c, 1:] == 0).all() and plan.parts >= 2
    elif name in ("one_key_image_at_cap", "one_key_image_over_cap"):
        c = what["chunk"]
        k = chain_lay["chainCap"] + (1 if name.endswith("over_cap") else 0)
        assert conf_per[what["bucket"]] == k == plan.m[c] and plan.m[c] <= lay["sliceLen"] and plan.span[c] == 1
        assert ((plan.conflicts[plan.owner == c] // lay["chunkLen"]) == c).all()            # all in the chunk that owns the bucket
    else:
        raise AssertionError(name)


def build_case(case, n, lay, chain_lay):
    """(R, what the constructor says about it, the plan on the expected seams), with the case's property asserted"""
    R, what = case.make(n, lay, chain_lay, **case.kw)
    R = np.ascontiguousarray(R, dtype=U64)
    assert R.size == n
    plan = chain_plan(R, lay, chain_lay, seams(R, lay)[1])
    check_property(case, R, what, plan, lay, chain_lay)
    return R, what, plan


def probe_side(R):
    """every key of R once, and the keys up to 100 above the largest that R lacks"""
    return np.arange(1, int(R.max()) + 101, dtype=U64)
