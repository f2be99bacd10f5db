"""The join problems of the randomised differential tests of the relational layer (test_gpu_fuzz_tables.py); the CPU test
of the generator and of the host twins evaluates the same ones (test_fuzz_tables.py). No GPU and no test in here.

make_problem(rng) draws one problem: two tables of 0 to 3000 rows with sizes on the lane (64), workgroup (256) and
validity-word (32) edges, one to three key columns of one kind per column on both sides (fixed 1 to 16 bytes, strings), NULLs,
payload columns of every kind the gather takes, where terms, an as-of term, aggregates, and the options of the wrappers.
Everything exists twice: as the library takes it (KeyColumns, arrays, masked arrays) and as the models of where_common,
asof_common, keys2_common, agg_common and groups_common take it (lists of bytes | None, numpy terms). Nothing in here asks
the library what a result should be."""
import math
from types import SimpleNamespace

import numpy as np

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

import agg_common as ac
import asof_common as asc
import keys2_common as k2
import where_common as wc

BLOCKS = 8                                           # test ids per GPU test
CASES = 96                                           # problems per GPU test, over its ids (HJ_FUZZ_CASES)
SEED = 20267000                                      # + block
EDGE_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257)
MAX_ROWS = 3000
PAIR_CAP = 200000
KEY_KINDS = (1, 2, 4, 8, 16, 0)                      # fixed widths; 0: variable length
NULL_RATES = (0.0,) * 8 + (0.1,) * 6 + (0.5,) * 5 + (1.0,)         # per column and side: 1.0 makes a table of NULL-keyed rows
KEY_MASKS = (0, 0x3F, 0xF, 1)
RADIX_BITS = (0, 8, 11, 12, 14, 16)                  # what test_gpu_fuzz.py draws
PAIR16 = np.dtype([("a", "<u8"), ("b", "<f8")])
PAYLOAD_KINDS = ("u1", "u2", "u4", "u8", "v16", "masked", "key_fixed", "key_varlen")
AGG_DTYPES = (np.int32, np.uint32, np.int64, np.uint64)
NULLS = ("group", "drop")


def draw_size(rng):
    """0 at a small fixed rate; otherwise an edge size or a log-uniform one up to MAX_ROWS"""
    if rng.random() < 0.04:
        return 0
    if rng.random() < 0.5:
        return int(rng.choice(EDGE_SIZES))
    return int(math.exp(rng.uniform(0.0, math.log(MAX_ROWS))))


def draw_slice(rng, n_s):
    choices = [None, 31, 32, 33, 64, 250, n_s - 1, n_s, n_s + 1] + ([1] if n_s <= 300 else [])
    s = choices[int(rng.integers(0, len(choices)))]
    return None if s is None or s < 1 else int(s)


# ---- key columns -------------------------------------------------------------------------------------------------------------
def string_values(rng, m):
    """m strings of 0 to 40 bytes over three letters, so that many are prefixes of others, and the 31 / 32 / 33 / 257-byte
    ones of test_gpu_join_on_columns.string_pool, which share all but their last byte"""
    stem = rng.integers(65, 91, size=257, dtype=np.uint8).tobytes()
    long = [stem[:k] for k in (31, 32, 33, 257)] + [stem[:k - 1] + b"#" for k in (31, 32, 33, 257)]
    short = [rng.integers(97, 100, size=int(rng.integers(0, 41)), dtype=np.uint8).tobytes() for _ in range(m)]
    return short + [long[k] for k in rng.integers(0, len(long), size=max(1, m // 8))]


def column_values(rng, width, m):
    """the values one key column draws from: about m of them (fewer where the width has fewer)"""
    if width == 0:
        return string_values(rng, m)
    return [row.tobytes() for row in rng.integers(0, 256, size=(min(m, 256 ** min(width, 2)), width), dtype=np.uint8)]


def key_pool(rng, widths, size):
    """up to `size` distinct key tuples; every column draws from its own small set, so tuples agree in some columns"""
    per = max(2, int(math.ceil(size ** (1.0 / len(widths)))) + 1)
    values = [column_values(rng, w, per) for w in widths]
    pool = {}
    for _ in range(4 * size):
        pool.setdefault(tuple(v[int(rng.integers(0, len(v)))] for v in values), None)
        if len(pool) >= size:
            break
    return list(pool)


def key_side(rng, widths, pool, n, rates, clustered=False):
    """n rows out of the pool as one ModelCol per column, NULLs at the column's rate; clustered: equal keys side by side,
    in the pool's order -- the keys the other side lacks then fill whole slices"""
    pick = rng.integers(0, len(pool), size=n) if n else np.zeros(0, dtype=np.int64)
    if clustered:
        pick = np.sort(pick)
    cols = []
    for c, (w, rate) in enumerate(zip(widths, rates)):
        gone = rng.random(n) < rate if rate < 1.0 else np.ones(n, dtype=bool)
        cols.append(k2.ModelCol(w, [None if g else pool[p][c] for p, g in zip(pick, gone)], False))
    return cols


def count_pairs(r_keys, s_keys):
    seen = {}
    for k in r_keys:
        if k is not None:
            seen[k] = seen.get(k, 0) + 1
    return sum(seen.get(k, 0) for k in s_keys if k is not None)


def draw_keys(rng, p):
    """the key columns of both sides: model columns, row keys and KeyColumns, the inner pairs at or below PAIR_CAP"""
    n_cols = int(rng.integers(1, 4))
    p.widths = [int(KEY_KINDS[int(rng.integers(0, len(KEY_KINDS)))]) for _ in range(n_cols)]
    p.nulls_equal = bool(rng.integers(0, 2))
    rates_r = [float(NULL_RATES[int(rng.integers(0, len(NULL_RATES)))]) for _ in range(n_cols)]
    rates_s = [float(NULL_RATES[int(rng.integers(0, len(NULL_RATES)))]) for _ in range(n_cols)]
    if rng.random() < 0.3:                         # no NULL at all: with fixed columns, what join_on takes too
        rates_r, rates_s = [0.0] * n_cols, [0.0] * n_cols
    clustered = rng.random() < 0.3
    big = max(p.n_r, p.n_s, 1)
    # multiplicity from "all unique" (a pool of twice the rows) to "one key for the whole table" (a pool of one), as far
    # as the cap on the pairs lets it
    floor = max(1, -(-p.n_r * p.n_s // (PAIR_CAP // 2)))
    size = max(floor, int(math.exp(rng.uniform(0.0, math.log(2 * big)))))
    if rng.random() < 0.15:
        size = floor
    for attempt in range(16):
        pool = key_pool(rng, p.widths, size)
        # R lacks part of S's pool and the other way round
        a, b = int(rng.integers(0, len(pool) // 3 + 1)), int(rng.integers(0, len(pool) // 3 + 1))
        r_pool, s_pool = pool[: len(pool) - a] or pool, pool[b:] or pool
        p.r_model, p.s_model = key_side(rng, p.widths, r_pool, p.n_r, rates_r), key_side(rng, p.widths, s_pool, p.n_s, rates_s, clustered)
        p.r_rowkeys, p.s_rowkeys = k2.row_keys(p.r_model, p.nulls_equal), k2.row_keys(p.s_model, p.nulls_equal)
        p.inner_pairs = count_pairs(p.r_rowkeys, p.s_rowkeys)
        if p.inner_pairs <= PAIR_CAP:
            break
        if len(pool) < size or attempt >= 2:       # the columns have no more values, or the NULLs pair up: fewer rows instead
            p.n_r, p.n_s = max(1, p.n_r // 2), max(1, p.n_s // 2)
        size *= 4
    assert p.inner_pairs <= PAIR_CAP
    p.pool_size = len(pool)
    p.lead = [int(rng.integers(0, 4)) for _ in range(n_cols)]
    p.r_keys = [k2.key_column(c, lead=l) for c, l in zip(p.r_model, p.lead)]
    p.s_keys = [k2.key_column(c, lead=(l + 1) % 4 if l else 0) for c, l in zip(p.s_model, p.lead)]
    p.plain_keys = all(w for w in p.widths) and all(e is not None for c in p.r_model + p.s_model for e in c.items)


# ---- payload columns -----------------------------------------------------------------------------------------------------------
def draw_payload(rng, n, side):
    """zero to three columns -> ({name: what the wrappers take}, {name: ("bytes", uint8 rows) | ("items", bytes | None per row)})"""
    cols, model = {}, {}
    for k in range(int(rng.integers(0, 4))):
        kind = PAYLOAD_KINDS[int(rng.integers(0, len(PAYLOAD_KINDS)))]
        name = f"{side}{k}_{kind}"
        if kind in ("u1", "u2", "u4", "u8", "masked"):
            width = int(kind[1]) if kind != "masked" else 4
            a = rng.integers(1, 256, size=(n, width), dtype=np.uint8).view(f"<u{width}").reshape(n)
            cols[name] = np.ma.MaskedArray(a, mask=rng.random(n) < 0.3) if kind == "masked" else a
            model[name] = ("bytes", np.ascontiguousarray(a).view(np.uint8).reshape(n, width))        # a masked array is gathered as its data
        elif kind == "v16":
            a = np.zeros(n, dtype=PAIR16)
            a["a"], a["b"] = rng.integers(1, 1 << 62, size=n), rng.random(n) + 1.0
            cols[name], model[name] = a, ("bytes", a.view(np.uint8).reshape(n, 16))
        else:
            if kind == "key_fixed":
                c = k2.fixed_col(rng, int(rng.choice([1, 2, 4, 8, 16])), n, nulls=float(rng.choice([0.0, 0.3, 1.0])))
            else:
                values = string_values(rng, 16)
                gone = rng.random(n) < float(rng.choice([0.0, 0.3, 1.0]))
                c = k2.ModelCol(0, [None if g else values[v] for v, g in zip(rng.integers(0, len(values), size=n), gone)], False)
            cols[name], model[name] = k2.key_column(c, lead=int(rng.integers(0, 4))), ("items", c.items)
    return cols, model


# ---- where and as-of terms -----------------------------------------------------------------------------------------------------
def term_values(rng, dtype, n, asof=False):
    """n values: a small range, so that every op holds for some pairs and fails for others (and as-of values tie), mixed
    with the dtype's ladder (where terms) or, for floats, both zeros, NaN and the infinities"""
    dtype = np.dtype(dtype)
    lo = 0 if dtype.kind == "u" else -3
    vals = rng.integers(lo, lo + 7, size=n).astype(dtype)
    if asof:
        special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf], dtype=dtype) if dtype.kind == "f" else wc.ladder(dtype)[:3]
        share = 0.15
    else:
        special, share = wc.ladder(dtype), 0.3
    swap = rng.random(n) < share
    vals[swap] = special[rng.integers(0, special.size, size=int(swap.sum()))]
    return vals


def draw_valid(rng, n):
    return None if rng.integers(0, 2) else rng.random(n) >= float(rng.choice([0.1, 0.5]))


def api_side(rng, values, valid):
    """one side of a term as the wrappers take it: a plain array, a masked array or a KeyColumn"""
    if valid is None:
        return values if rng.integers(0, 2) else hj.KeyColumn(values)
    return np.ma.MaskedArray(values, mask=~valid) if rng.integers(0, 2) else hj.KeyColumn(values, valid)


def draw_term(rng, p, ops, asof=False):
    dtype = wc.DTYPES[int(rng.integers(0, len(wc.DTYPES)))]
    op = ops[int(rng.integers(0, len(ops)))]
    s, r = term_values(rng, dtype, p.n_s, asof), term_values(rng, dtype, p.n_r, asof)
    sv, rv = draw_valid(rng, p.n_s), draw_valid(rng, p.n_r)
    return (api_side(rng, s, sv), op, api_side(rng, r, rv)), wc.term_of(s, op, r, sv, rv)


def draw_conditions(rng, p, index=None):
    """zero to HJ_WHERE_MAX_TERMS where terms and, for every other problem, an as-of term (index None: drawn); under an
    as-of term fewer where terms, so that S rows keep several eligible pairs"""
    if index is None:
        with_asof, op = bool(rng.integers(0, 2)), None
    else:                                          # every other problem of a test id, the ops in turn
        with_asof, op = (index // BLOCKS) % 2 == 0, asc.ASOF_OPS[(index // (2 * BLOCKS)) % len(asc.ASOF_OPS)]
    n_terms = int(rng.choice([0, 1, 1, 2] if with_asof else [0, 0, 1, 1, 2, 3, _lib.HJ_WHERE_MAX_TERMS]))
    terms = [draw_term(rng, p, list(wc.OPS)) for _ in range(n_terms)]
    p.where, p.where_model = [t[0] for t in terms], [t[1] for t in terms]
    p.asof, p.asof_model = draw_term(rng, p, [op] if op else list(asc.ASOF_OPS), asof=True) if with_asof else (None, None)


# ---- aggregates ---------------------------------------------------------------------------------------------------------------
def draw_aggregates(rng, p):
    """one to six aggregates over S: the source columns as the wrappers take them (POISON under every NULL), the {output:
    (op, source)} dict, and one agg_common.Col per output"""
    p.agg_cols, p.aggs, p.agg_model = {}, {}, {}
    for k in range(int(rng.integers(1, 7))):
        op = ("count", "count", "sum", "min", "max")[int(rng.integers(0, 5))]
        out = f"a{k}_{op}"
        if op == "count" and rng.integers(0, 2):
            p.aggs[out], p.agg_model[out] = ("count", None), ac.Col(ac.COUNT)
            continue
        dtype = np.dtype(AGG_DTYPES[int(rng.integers(0, len(AGG_DTYPES)))])
        info = np.iinfo(dtype)
        ends = np.array([info.min, info.min + 1, info.max, info.max - 1, 0, 1], dtype=dtype)       # SUM wraps; signed MIN != unsigned MIN
        values = ends[rng.integers(0, ends.size, size=p.n_s)]
        small = rng.random(p.n_s) < 0.3
        values[small] = rng.integers(0, 100, size=int(small.sum())).astype(dtype)
        valid = draw_valid(rng, p.n_s)
        col = ac.Col(_lib.AGG_OPS[op], values, valid)
        name = f"v{k}"
        p.agg_cols[name] = col.poisoned() if valid is None else hj.KeyColumn(col.poisoned(), valid)
        p.aggs[out], p.agg_model[out] = (op, name), col


def agg_expected(p, n_groups, g_idx, v_idx):
    """agg_common.expected in the form the wrappers return: {"count", per COUNT a uint64 plane, per SUM / MIN / MAX
    (values with 0 under a NULL, valid: the group saw a valid value)}"""
    outs = list(p.agg_model)
    cols = [p.agg_model[o] for o in outs]
    seen = [ac.Col(ac.COUNT, c.values, c.valid) for c in cols]
    count, planes = ac.expected(n_groups, g_idx, v_idx, cols + seen)
    res = {"count": count}
    for k, (out, c) in enumerate(zip(outs, cols)):
        if c.op == ac.COUNT:
            res[out] = planes[k]
        else:
            valid = planes[len(cols) + k] > 0
            res[out] = (np.where(valid, planes[k], ac.U64(0)), valid)
    return res


# ---- the problem ---------------------------------------------------------------------------------------------------------------
def reduced_keys(p):
    """the problem on one 32-bit key word, as uint64 tuples for join_tables / radix_join_aggregate: every distinct key is
    a number from 1 on; a NULL-keyed row gets a number of its own, which matches nothing"""
    ids, nxt = {}, 1
    out = []
    for keys in (p.r_rowkeys, p.s_rowkeys):
        rel = np.zeros(len(keys), dtype=np.uint64)
        for i, k in enumerate(keys):
            if k is None:
                rel[i], nxt = nxt, nxt + 1
            else:
                if k not in ids:
                    ids[k], nxt = nxt, nxt + 1
                rel[i] = ids[k]
        out.append(rel)
    return out


def make_problem(rng, index=None):
    """one problem. index (the case's number in its test): the join kind, whether there is an as-of term, and its op go
    round with it, so that a few dozen problems hold every one of them; None: they are drawn like everything else"""
    p = SimpleNamespace()
    p.n_r, p.n_s = draw_size(rng), draw_size(rng)
    draw_keys(rng, p)                                  # (may halve the sizes to keep the pairs under the cap)
    p.slice_tuples = draw_slice(rng, p.n_s)
    p.step = p.n_s if not p.slice_tuples else min(p.slice_tuples, p.n_s)
    drawn = int(rng.integers(0, len(wc.HOWS)))
    p.how = wc.HOWS[drawn if index is None else (index + index // len(wc.HOWS)) % len(wc.HOWS)]
    p.key_mask = int(KEY_MASKS[int(rng.integers(0, len(KEY_MASKS)))])
    p.radix_bits = int(RADIX_BITS[int(rng.integers(0, len(RADIX_BITS)))])
    p.nulls = NULLS[int(rng.integers(0, 2))]
    p.r_cols, p.r_cols_model = draw_payload(rng, p.n_r, "r")
    p.s_cols, p.s_cols_model = draw_payload(rng, p.n_s, "s")
    draw_conditions(rng, p, index)
    draw_aggregates(rng, p)
    p.relR, p.relS = reduced_keys(p)
    p.r_ids, p.s_ids = [int(k) for k in p.relR], [int(k) for k in p.relS]
    return p


def tag_of(p, block=None, case=None, **more):
    """what a failing assertion says: enough to draw the problem again"""
    return dict(block=block, case=case, n_r=p.n_r, n_s=p.n_s, widths=p.widths, how=p.how, slice_tuples=p.slice_tuples,
                key_mask=hex(p.key_mask), radix_bits=p.radix_bits, nulls_equal=p.nulls_equal, nulls=p.nulls, pool=p.pool_size,
                where=[(t[0].dtype.name, t[1]) for t in p.where_model],
                asof=None if p.asof_model is None else (p.asof_model[0].dtype.name, p.asof_model[1]), **more)


def problems(block, cases=CASES, blocks=BLOCKS, seed=SEED):
    """the problems of one test id: (case, problem) for case = block, block + blocks, ... below cases"""
    rng = np.random.default_rng(seed + block)
    for case in range(block, cases, blocks):
        yield case, make_problem(rng, case)
