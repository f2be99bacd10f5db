"""The relations of the randomised differential tests (test_gpu_fuzz.py); the CPU test of the chain plan evaluates the same
ones (test_htm_chain_cases.py). No GPU and no test in here."""
import numpy as np

HI_MODES = ("zero", "uniform", "neighbours")                               # how make_relation(high=True) draws the high parts
W_POOL = (1, 2, 4, 8, 16, 16, 16, 32, 48, 64, 100, 300, 2000)               # the disorder W a relation is displaced by


def make_relation(rng, n, high=False, plen=4, hi_mode=None, w_pool=W_POOL):
    """A near-sorted relation of n tuples (value = key, as DataGen's): sorted keys with bursts, then displaced by < W.
    -> (keys, W), W drawn out of w_pool. high=False draws what it always drew for a seed. high=True: every key gets a high part above the table
    of 2n slots, key = home + hi * table (near-sorted by home slot as before, below 2^32 - 1), hi per case (hi_mode, or
    drawn out of HI_MODES): all zero; uniform over [0, hiCap) of slot_codes_info(table, plen); neighbours, where half of the
    tuples take the home slot of the tuple before them and hi comes out of four values, so that keys differ in hi alone
    (or not at all). One case out of six gets up to five keys at or above hiCap * table as well: keys without a slot code.
    -> (keys, W, {"mode", "over": how many such keys, "hiCap", "keyLimit": hiCap * table})."""
    table = 2 * n
    kind = rng.integers(0, 5)
    if kind == 0:          # dense unique keys
        keys = np.arange(1, n + 1, dtype=np.uint64)
    elif kind == 1:        # random multiset over a domain of n * f keys
        f = rng.choice([0.25, 0.5, 1.0, 1.5, 1.99])
        keys = np.sort(rng.integers(1, max(2, int(n * f)), size=n, dtype=np.uint64))
    elif kind == 2:        # bursts: few distinct keys, geometric multiplicities
        distinct = np.sort(rng.choice(np.arange(1, table, dtype=np.uint64), size=max(1, n // int(rng.integers(2, 9))), replace=False))
        counts = rng.geometric(0.3, size=distinct.size)
        keys = np.repeat(distinct, counts)[:n]
        if keys.size < n:
            keys = np.concatenate([keys, np.arange(1, n - keys.size + 1, dtype=np.uint64) + keys[-1]])
        keys = np.sort(keys)
    elif kind == 3:        # sparse keys over the whole table (walks wrap around its end) and a dense stretch at the very top
        keys = np.sort(np.concatenate([rng.integers(1, table, size=n - n // 8, dtype=np.uint64),
                                       np.arange(table - n // 8, table, dtype=np.uint64)]))
    else:                  # two interleaved dense runs (every key twice, far apart in value order only by 1)
        keys = np.sort(np.concatenate([np.arange(1, n // 2 + 1, dtype=np.uint64)] * 2))
    keys = keys[:n].astype(np.uint64)
    keys = np.sort((keys - np.uint64(1)) % np.uint64(table - 1) + np.uint64(1))        # into [1, table - 1], still sorted
    w = int(rng.choice(list(w_pool)))
    if w > 1:
        order = np.argsort(np.arange(n) + rng.uniform(0, w, size=n), kind="stable")
        keys = keys[order]
    if not high:
        return np.ascontiguousarray(keys), w
    import htm_hashjoin_amd as hj
    cap = hj.slot_codes_info(table, plen)["hiCap"]
    top = (1 << 32) // table                               # high parts a 32-bit key has room for
    mode = hi_mode or HI_MODES[int(rng.integers(0, len(HI_MODES)))]
    if mode == "zero":
        hi = np.zeros(n, dtype=np.uint64)
    elif mode == "uniform":
        hi = rng.integers(0, min(cap, top), size=n, dtype=np.uint64)
    else:
        twin = np.flatnonzero(rng.integers(0, 2, size=n) == 1)
        twin = twin[twin > 0]
        keys[twin] = keys[twin - 1]                        # the home slot its left neighbour had
        hi = rng.integers(0, min(cap, top, 4), size=n, dtype=np.uint64)
    over = 0
    if top > cap and rng.integers(0, 6) == 0:
        at = rng.choice(n, size=min(n, int(rng.integers(1, 6))), replace=False)
        hi[at] = rng.integers(cap, top, size=at.size, dtype=np.uint64)
        over = int(at.size)
    keys = np.minimum(keys + hi * np.uint64(table), np.uint64(0xFFFFFFFE))
    return np.ascontiguousarray(keys), w, {"mode": mode, "over": over, "hiCap": cap, "keyLimit": cap * table}


# the slot-code road's fuzz: disorder beyond what the rings hold (W >= 300: the dirty log may overflow, a permitted hand-over)
# in one case out of ten, so that most cases can stay on the road
ROAD_W_POOL = W_POOL[:11] + (2, 8, 16, 32, 64, 100, 100) + W_POOL[11:]


def slot_code_case(rng):
    """One case of the slot-code road's fuzz: -> (n, probeLength, idx_base, R, S, W, what make_relation says about the high
    parts). S is a permutation of part of R, plus every high-part variant of some of R's home slots (and one beyond what
    a code holds), so that a key matches only itself."""
    n = 1 << int(rng.integers(10, 21))
    plen = int(rng.choice([1, 2, 3, 4, 8]))
    idx_base = int(rng.choice([0, 0xFFFFFFFF - n]))
    R, w, hi = make_relation(rng, n, high=True, plen=plen, w_pool=ROAD_W_POOL)
    table = np.uint64(2 * n)
    homes = rng.choice(R, size=32, replace=False) % table
    variants = (homes[:, None] + np.arange(hi["hiCap"] + 1, dtype=np.uint64)[None, :] * table).ravel()
    S = np.concatenate([rng.permutation(R)[: int(rng.integers(1, n + 1))], variants[variants < np.uint64(1 << 32)]])
    return n, plen, idx_base, R, np.ascontiguousarray(S, dtype=np.uint64), w, hi
