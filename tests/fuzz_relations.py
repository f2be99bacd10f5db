"""The relations of the randomised differential tests (test_gpu_fuzz.py); the CPU test of the chain plan evaluates the same
ones (test_htm_chain_cases.py). No GPU and no test in here."""
import numpy as np


def make_relation(rng, n):
    """A near-sorted relation of n tuples (value = key, as DataGen's): sorted keys with bursts, then displaced by < W."""
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
    w = int(rng.choice([1, 2, 4, 8, 16, 16, 16, 32, 48, 64, 100, 300, 2000]))
    if w > 1:
        order = np.argsort(np.arange(n) + rng.uniform(0, w, size=n), kind="stable")
        keys = keys[order]
    return np.ascontiguousarray(keys), w
