"""What the tests of the key columns share (test_keys_abi.py, test_keys2_abi.py, test_groups_abi.py, test_gather2_abi.py,
test_gpu_keys2.py, test_gpu_pair_filter_frame.py): the readers of include/htm_hashjoin.h that the ABI tests compare the
bindings with, and the header's hash restated in numpy -- MurmurHash3_x86_32 over the 32-bit words of a row. No test in
here, and nothing that asks the library what a result should be."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR = np.dtype([("a", np.uint64), ("b", np.float64)])         # a 16-byte structured element
WIDTH_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64, 16: PAIR}
MIXES = [(1,), (2,), (4,), (8,), (16,), (8, 4), (1, 16), (2, 8, 1), (4, 4, 4), (16, 2, 8, 1), (1, 2, 4, 8), (16, 16, 16, 16)]


# ---- the header ------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def _declared_args(symbol):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, _code())
    assert decl, f"{symbol} is not declared in include/htm_hashjoin.h"
    return [a.strip() for a in decl.group(1).split(",")]


# ---- the hash: the header's wording, restated ----------------------------------------------------------------------------
def _rotl(x, r):
    return ((x << np.uint32(r)) | (x >> np.uint32(32 - r))).astype(np.uint32)


def murmur3_words(words, key_mask=0):
    """MurmurHash3_x86_32, seed 0, of every row of words[rows, nWords] (uint32); len = 4 * nWords; & key_mask (0: all)"""
    words = np.asarray(words, dtype=np.uint32)
    h = np.zeros(words.shape[0], dtype=np.uint32)
    with np.errstate(over="ignore"):
        for j in range(words.shape[1]):
            k = words[:, j] * np.uint32(0xcc9e2d51)
            k = _rotl(k, 15) * np.uint32(0x1b873593)
            h = _rotl(h ^ k, 13) * np.uint32(5) + np.uint32(0xe6546b64)
        h = h ^ np.uint32(4 * words.shape[1])
        h = (h ^ (h >> np.uint32(16))) * np.uint32(0x85ebca6b)
        h = (h ^ (h >> np.uint32(13))) * np.uint32(0xc2b2ae35)
        h = h ^ (h >> np.uint32(16))
    return (h & np.uint32(key_mask or 0xFFFFFFFF)).astype(np.uint64)


def key_words(cols):
    """the 32-bit words of every row: width 1 and 2 zero-extended to one word, wider elements their little-endian words"""
    parts = []
    for a in cols:
        a = np.ascontiguousarray(a)
        w = a.dtype.itemsize
        raw = a.view(np.uint8).reshape(a.size, w)
        if w < 4:
            raw = np.concatenate([raw, np.zeros((a.size, 4 - w), dtype=np.uint8)], axis=1)
        parts.append(np.ascontiguousarray(raw).view("<u4").reshape(a.size, -1))
    return np.concatenate(parts, axis=1)


def random_column(rng, width, n):
    raw = rng.integers(0, 256, size=n * width, dtype=np.uint8)
    return raw.view(WIDTH_DTYPES[width]).reshape(n).copy()
