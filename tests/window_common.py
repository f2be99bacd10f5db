"""What the tests of hj_window_rows_dev / hj_window_rows_host share: the model, the case families, the library on host
pointers and the comparison. No test in here.

The model restates the header's definitions by RUNS in numpy and plain Python and never calls the library: which
positions are skipped, where a partition and a peer run start (peers: equal dense ranks per order column, sort_common's
own model of a tie), start / end / peerStart by running maxima and minima, the running sums modulo 2^64 by differences of
one cumulative sum, the running minima and maxima by a loop over Python integers."""
import ctypes as C

import numpy as np

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import sort_common as sc

U32, U64 = np.uint32, np.uint64
NO_ROW = 0xFFFFFFFF
SENT32, SENT64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
M64 = (1 << 64) - 1
W = _lib
NUMBER_OPS = (W.HJ_WIN_ROW_NUMBER, W.HJ_WIN_RANK, W.HJ_WIN_DENSE_RANK, W.HJ_WIN_PART_ROWS)
MAP_OPS = (W.HJ_WIN_LAG, W.HJ_WIN_LEAD, W.HJ_WIN_FIRST_ROW, W.HJ_WIN_LAST_ROW)
RUN_OPS = (W.HJ_WIN_RUN_COUNT, W.HJ_WIN_RUN_SUM, W.HJ_WIN_RUN_MIN, W.HJ_WIN_RUN_MAX)


def layout(n_pos):
    """hj_window_layout_info -> (tile positions, chunk positions, chunks, workspace bytes)"""
    out = (C.c_uint64 * 4)()
    assert lib.hj_window_layout_info(n_pos, out) == _lib.HJ_OK
    return tuple(int(x) for x in out)


class Func:
    """one function of a call: the op, LAG / LEAD's offset, a RUN_* op's source (values per ROW, any bytes under a NULL)"""

    def __init__(self, op, offset=0, src=None, valid=None, width=None):
        self.op, self.offset = op, offset
        self.src = None if src is None else np.ascontiguousarray(src)
        self.valid = None if valid is None else np.ascontiguousarray(valid, dtype=bool)
        self.width = (0 if self.src is None else self.src.dtype.itemsize) if width is None else width
        self.flags = _lib.HJ_AGG_SIGNED if self.src is not None and self.src.dtype.kind == "i" else 0
        self.run = op in RUN_OPS

    @property
    def dtype(self):
        return U64 if self.run else U32

    @property
    def sentinel(self):
        return SENT64 if self.run else SENT32

    def plane(self, n_rows, garbage=None):
        return None if self.valid is None else sc.Col(np.zeros(n_rows, dtype=np.uint8), self.valid).plane(garbage)


class Case:
    """perm: uint32 per position or None (the identity); part: uint32 per ROW or None; order: sort_common.Col per column,
    values per ROW; funcs: at most HJ_WIN_MAX_FUNCS Func"""

    def __init__(self, n_pos, n_rows, perm, part, order, funcs):
        self.n_pos, self.n_rows, self.perm, self.part, self.order, self.funcs = n_pos, n_rows, perm, part, list(order), list(funcs)
        assert perm is None or (perm.dtype == U32 and perm.size >= n_pos)
        assert part is None or (part.dtype == U32 and part.size == n_rows)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def model_runs(case):
    """(rows per position, in-range mask, partition heads, peer heads) by the header's definitions"""
    n = case.n_pos
    rows = (case.perm[:n] if case.perm is not None else np.arange(n, dtype=U32)).astype(np.int64)
    inr = rows < case.n_rows
    head, peer = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    if n > 1:
        both = inr[1:] & inr[:-1]
        a, b = np.where(both, rows[1:], 0), np.where(both, rows[:-1], 0)
        same_part = both if case.part is None or case.n_rows == 0 else both & (case.part[a] == case.part[b])
        same_peer = same_part.copy()
        for col in case.order:
            rank = sc._ranks(col)                    # ties equal, every NULL one class of its own; the direction does not matter
            same_peer &= rank[a] == rank[b]
        head[1:], peer[1:] = ~same_part, ~same_peer
    return rows, inr, head, peer


def _value(f, row):
    """what ROW brings to a RUN_* op as a Python integer (signed sources sign-extended), None under a NULL"""
    if f.valid is not None and not f.valid[row]:
        return None
    return 1 if f.op == W.HJ_WIN_RUN_COUNT else int(f.src[row])


def model(case):
    """-> ([one array per function, indexed by row, the sentinel where nothing is written], info: partitions, peer runs, skipped)"""
    n = case.n_pos
    rows, inr, head, peer = model_runs(case)
    pos = np.arange(n, dtype=np.int64)
    info = (int((head & inr).sum()), int((peer & inr).sum()), int((~inr).sum()))
    outs = [np.full(case.n_rows, f.sentinel, dtype=f.dtype) for f in case.funcs]
    if n == 0:
        return outs, info
    start = np.maximum.accumulate(np.where(head, pos, 0))
    peer_start = np.maximum.accumulate(np.where(peer, pos, 0))
    tail = np.append(head[1:], True)
    end = np.minimum.accumulate(np.where(tail, pos, n)[::-1])[::-1]
    runs = np.cumsum(peer)
    dense = runs - runs[start] + 1
    live = np.flatnonzero(inr)
    for f, out in zip(case.funcs, outs):
        if f.op == W.HJ_WIN_ROW_NUMBER:
            val = pos - start + 1
        elif f.op == W.HJ_WIN_RANK:
            val = peer_start - start + 1
        elif f.op == W.HJ_WIN_DENSE_RANK:
            val = dense
        elif f.op == W.HJ_WIN_PART_ROWS:
            val = end - start + 1
        elif f.op == W.HJ_WIN_LAG:
            q = pos - f.offset                       # Python-sized integers: nothing wraps
            val = np.where(q >= start, rows[np.clip(q, 0, n - 1)], NO_ROW)
        elif f.op == W.HJ_WIN_LEAD:
            q = pos + f.offset
            val = np.where(q <= end, rows[np.clip(q, 0, n - 1)], NO_ROW)
        elif f.op == W.HJ_WIN_FIRST_ROW:
            val = rows[start]
        elif f.op == W.HJ_WIN_LAST_ROW:
            val = rows[end]
        elif f.op in (W.HJ_WIN_RUN_COUNT, W.HJ_WIN_RUN_SUM):
            x, r = np.zeros(n, dtype=U64), rows[live]
            ok = np.ones(r.size, dtype=bool) if f.valid is None else f.valid[r]
            # a signed source is sign-extended to 64 bits, an unsigned one zero-extended
            v = np.ones(r.size, dtype=U64) if f.op == W.HJ_WIN_RUN_COUNT else f.src[r].astype(np.int64).view(U64) if f.flags else f.src[r].astype(U64)
            x[live] = np.where(ok, v, U64(0))
            total = np.cumsum(x, dtype=U64)          # modulo 2^64, as the header says
            val = total - np.where(start > 0, total[np.maximum(start, 1) - 1], U64(0))
        else:
            signed, low = bool(f.flags), f.op == W.HJ_WIN_RUN_MIN
            ident = ((1 << 63) - 1 if signed else M64) if low else (-(1 << 63) if signed else 0)
            val, acc = np.zeros(n, dtype=U64), ident
            for p in range(n):
                if head[p]:
                    acc = ident
                v = _value(f, rows[p]) if inr[p] else None
                if v is not None:
                    acc = min(acc, v) if low else max(acc, v)
                val[p] = acc & M64
        out[rows[live]] = np.asarray(val)[live].astype(f.dtype)
    return outs, info


# ---- the library on host pointers ------------------------------------------------------------------------------------------------
def func_array(funcs, pointers):
    """pointers: [(out_ptr, src_ptr or 0, valid_ptr or 0)] -> (hj_win_func array, its length)"""
    arr = (_lib.hj_win_func * max(len(funcs), 1))()
    for a, f, (out, src, valid) in zip(arr, funcs, pointers):
        a.src, a.srcValid, a.out = src or None, valid or None, out or None
        a.op, a.width, a.flags, a.offset = f.op, f.width, f.flags, f.offset
    return arr, len(funcs)


def host_call(case, garbage=None):
    """hj_window_rows_host over sentinel-filled outputs -> ([one array per function], out[8])"""
    outs = [np.full(case.n_rows, f.sentinel, dtype=f.dtype) for f in case.funcs]
    planes = [f.plane(case.n_rows, garbage) for f in case.funcs]
    o_planes = [c.plane(garbage) for c in case.order]
    f_arr, n_funcs = func_array(case.funcs, [(o.ctypes.data, f.src.ctypes.data if f.src is not None else 0, p.ctypes.data if p is not None else 0)
                                             for f, o, p in zip(case.funcs, outs, planes)])
    o_arr, n_order = sc.sort_col_array(case.order, [(c.values.ctypes.data, p.ctypes.data if p is not None else 0) for c, p in zip(case.order, o_planes)])
    info = (C.c_uint64 * 8)()
    rc = lib.hj_window_rows_host(case.perm.ctypes.data if case.perm is not None else None, case.n_pos, case.n_rows,
                                 case.part.ctypes.data if case.part is not None else None, o_arr, n_order, f_arr, n_funcs, info)
    assert rc == _lib.HJ_OK, rc
    return outs, [int(x) for x in info]


def same(got, want, tag=None):
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, i, g.dtype, g.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (tag, f"function {i}: {bad.size} rows differ, the first at {bad[:4]}: {g[bad[:4]]} for {w[bad[:4]]}")


def check_info(info, case, want, tag=None):
    """out[8] of hj_window_rows_info / hj_window_rows_host against the model's counts and the layout"""
    if case.n_pos == 0:
        assert info[:3] == [0, 0, 0] and info[4:] == [0, 0, 0, 0], (tag, info)
        return
    _, _, chunks, nbytes = layout(case.n_pos)
    assert (info[0], info[1], info[2], info[4]) == (case.n_pos,) + want, (tag, info, want)
    assert (info[5], info[6], info[7]) == (chunks, nbytes, 0), (tag, info)


# ---- the case families -----------------------------------------------------------------------------------------------------------
def lengths_to_ids(lengths, n):
    """partition lengths (repeated as long as needed) -> one id per position, equal neighbours' ids different"""
    lengths = np.asarray(lengths, dtype=np.int64)
    reps = -(-n // int(lengths.sum())) if lengths.size else 0
    lens = np.tile(lengths, max(reps, 1))
    return np.repeat(np.arange(lens.size, dtype=np.int64), lens)[:n].astype(U32)


def shape_ids(name, n, seed=0):
    """the partition id of every POSITION for a named shape"""
    T, L = layout(1)[:2]
    rng = np.random.default_rng(seed)
    if name == "one":
        return np.zeros(n, dtype=U32)
    if name == "each":
        return np.arange(n, dtype=U32)
    if name.startswith("fixed"):
        return lengths_to_ids([int(name[5:])], n)
    if name == "geometric":
        return lengths_to_ids(rng.geometric(0.05, size=max(n // 4, 4)), n)
    if name == "seams":
        # heads exactly at the first and at the last position of a wavefront, a tile and a chunk
        heads = np.zeros(n, dtype=bool)
        for unit in (64, T, L):
            heads[0::unit] = True
            heads[unit - 1::unit] = True
        return (np.cumsum(heads) - 1).astype(U32)
    if name == "long":
        # one partition over at least three whole chunks between two short ones
        assert n >= 5 * L
        ids = np.ones(n, dtype=U32)
        ids[:L // 2 + 3] = 0
        ids[n - (L // 2 + 5):] = 2
        return ids
    raise KeyError(name)


def peer_values(name, n, seed=0):
    """the order columns as POSITION-indexed (values, valid) lists for a named peer shape"""
    T, L = layout(1)[:2]
    rng = np.random.default_rng(seed + 1000)
    if name == "none":
        return []
    if name == "const":
        return [(np.full(n, 7, dtype=np.int32), None)]
    if name == "distinct":
        return [(np.arange(n, dtype=np.int64) * 3 - n, None)]
    if name == "runs":
        # peer runs of 1 .. 130 positions: they straddle wavefront, tile and chunk seams
        return [(lengths_to_ids(rng.integers(1, 131, size=max(n // 8, 4)), n).astype(np.uint16), None)]
    if name in ("f32", "f64"):
        dt = np.float32 if name == "f32" else np.float64
        bits = np.uint32 if name == "f32" else np.uint64
        nan = [0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFF800001] if name == "f32" else [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000123]
        pool = np.concatenate([np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf], dtype=dt), np.array(nan, dtype=bits).view(dt)])
        # blocks of 1 .. 5 draws from one class (the zeros, the NaNs, a plain value): peers by value, different bits
        cls = np.repeat(rng.integers(0, 4, size=n), rng.integers(1, 6, size=n))[:n]
        pick = np.where(cls == 0, rng.integers(0, 2, n), np.where(cls == 1, rng.integers(6, 10, n), np.where(cls == 2, 2, rng.integers(3, 6, n))))
        return [(pool[pick], None)]
    if name == "nulls":
        valid = np.repeat(rng.random(n) < 0.5, rng.integers(1, 4, size=n))[:n]
        return [(rng.integers(0, 1 << 62, n).astype(np.int64) * np.where(valid, 0, 1) + np.where(valid, 5, 0), valid)]   # random bytes under the NULLs
    if name in ("two", "four"):
        k = 2 if name == "two" else 4
        dts = (np.uint8, np.int64, np.float32, np.int16)[:k]
        cols = []
        for i, dt in enumerate(dts):
            v = np.repeat(rng.integers(0, 3, size=n), rng.integers(1, 3 + 2 * i, size=n))[:n].astype(dt)
            valid = (np.repeat(rng.random(n) < 0.8, rng.integers(1, 4, size=n))[:n]) if i % 2 else None
            cols.append((v, valid))
        return cols
    raise KeyError(name)


def run_funcs(n_rows, seed=0, null_pct=10):
    """eight RUN_* functions over the four source types: sums that wrap, signed extremes, counts with and without a plane"""
    rng = np.random.default_rng(seed + 2000)
    valid = None if null_pct == 0 else rng.random(n_rows) >= null_pct / 100.0
    i32 = rng.integers(-1 << 31, 1 << 31, n_rows).astype(np.int32)
    u32 = rng.integers(0, 1 << 32, n_rows).astype(np.uint32)
    i64 = rng.integers(-1 << 63, 1 << 63, n_rows).astype(np.int64)
    u64 = rng.integers(0, 1 << 64, n_rows, dtype=np.uint64)
    for a in (i32, i64):
        a[::7] = np.iinfo(a.dtype).min
        a[3::11] = np.iinfo(a.dtype).max
    u64[::5] = M64                                   # three of them wrap a sum
    return [Func(W.HJ_WIN_RUN_COUNT), Func(W.HJ_WIN_RUN_COUNT, src=i32, valid=valid, width=4), Func(W.HJ_WIN_RUN_SUM, src=i32, valid=valid),
            Func(W.HJ_WIN_RUN_SUM, src=u64, valid=valid), Func(W.HJ_WIN_RUN_MIN, src=i64, valid=valid), Func(W.HJ_WIN_RUN_MAX, src=i32, valid=valid),
            Func(W.HJ_WIN_RUN_MIN, src=u32), Func(W.HJ_WIN_RUN_MAX, src=u64, valid=valid)]


def number_funcs(lag=1, lead=1):
    return [Func(W.HJ_WIN_ROW_NUMBER), Func(W.HJ_WIN_RANK), Func(W.HJ_WIN_DENSE_RANK), Func(W.HJ_WIN_PART_ROWS), Func(W.HJ_WIN_LAG, lag),
            Func(W.HJ_WIN_LEAD, lead), Func(W.HJ_WIN_FIRST_ROW), Func(W.HJ_WIN_LAST_ROW)]


def build(n_pos, shape="geometric", peers="runs", perm="random", extra_rows=0, holes=0, seed=0, funcs=None, null_pct=10):
    """A case out of POSITION-indexed partition ids and order values, carried to the rows through the permutation.
    perm: "random" | "identity" (an explicit identity plane) | None (dPerm NULL). extra_rows: rows that stand at no position.
    holes: that many positions (the first, the last and the chunk seams among them) hold HJ_NO_ROW or a row >= nRows."""
    rng = np.random.default_rng(seed + 3000)
    n_rows = n_pos + extra_rows
    order_of_rows = rng.permutation(n_rows) if perm == "random" else np.arange(n_rows)
    rows = order_of_rows[:n_pos].astype(np.int64)
    ids, cols = shape_ids(shape, n_pos, seed), peer_values(peers, n_pos, seed)
    part = rng.integers(0, 1 << 32, n_rows).astype(U32)
    part[rows] = ids
    order = []
    for v, valid in cols:
        full = rng.integers(0, 100, n_rows).astype(v.dtype)
        full[rows] = v
        ok = None
        if valid is not None:
            ok = rng.random(n_rows) < 0.5
            ok[rows] = valid
        order.append(sc.Col(full, ok))
    plane = None if perm is None else rows.astype(U32)
    if holes:
        assert plane is not None
        L = layout(1)[1]
        at = {0, n_pos - 1} | {p for p in (L - 1, L, 2 * L - 1, 2 * L) if p < n_pos} | {int(p) for p in rng.integers(0, n_pos, size=holes)}
        for k, p in enumerate(sorted(at)):
            plane[p] = NO_ROW if k % 2 == 0 else n_rows + int(rng.integers(0, 1000))
    if funcs is None:
        funcs = number_funcs()
    elif funcs == "run":
        funcs = run_funcs(n_rows, seed, null_pct)
    return Case(n_pos, n_rows, plane, None if shape == "one" and seed % 2 else part, order, funcs)


# ---- the wrapper against a per-partition loop ------------------------------------------------------------------------------------------
def _loop_reference(keys, order, descending, nulls, null_keys, cols, funcs):
    """partition rows by their key tuples (None: NULL) in a dict, sort each partition with Python's stable sort over
    sort_common's ranks, walk it"""
    n = len(keys)
    ranks = [sc._ranks(sc.Col(v, valid, d, w)) for (v, valid), d, w in zip(order, descending, nulls)]
    parts, dropped = {}, []
    for i, key in enumerate(keys):
        if null_keys == "drop" and any(k is None for k in key):
            dropped.append(i)
            continue
        parts.setdefault(key, []).append(i)
    res = {name: [None] * n for name in funcs}
    for name, spec in funcs.items():
        if spec in ("row_number", "rank", "dense_rank", "count"):
            res[name] = [0] * n
    for rows in parts.values():
        rows.sort(key=lambda i: tuple(int(r[i]) for r in ranks))
        tie = [tuple(int(r[i]) for r in ranks) for i in rows]
        for name, spec in funcs.items():
            op = spec if isinstance(spec, str) else spec[0]
            col = cols[spec[1]] if not isinstance(spec, str) and spec[1] is not None else None
            acc, cnt, rank, dense = None, 0, 0, 0
            for j, i in enumerate(rows):
                if j == 0 or tie[j] != tie[j - 1]:
                    rank, dense = j + 1, dense + 1
                if op == "row_number":
                    res[name][i] = j + 1
                elif op == "rank":
                    res[name][i] = rank
                elif op == "dense_rank":
                    res[name][i] = dense
                elif op == "count":
                    res[name][i] = len(rows)
                elif op in ("lag", "lead"):
                    q = j - spec[2] if op == "lag" else j + spec[2]
                    res[name][i] = col[rows[q]] if 0 <= q < len(rows) else None
                elif op in ("first", "last"):
                    res[name][i] = col[rows[0 if op == "first" else -1]]
                else:
                    v = 1 if col is None else col[i]
                    if v is not None:
                        cnt += 1
                        acc = v if acc is None else acc + v if op == "cumsum" else min(acc, v) if op == "cummin" else max(acc, v)
                    res[name][i] = cnt if op == "cumcount" else acc
    for name, spec in funcs.items():
        if not isinstance(spec, str) and spec[0] == "cumcount":
            res[name] = [0 if v is None else v for v in res[name]]
    return res, len(parts), len(dropped)


def wrapper_table(n, seed):
    """a table with a string and an integer partition key (NULLs in both), two order columns and three payload columns"""
    rng = np.random.default_rng(seed)
    names = [None if rng.random() < 0.1 else "k%d" % rng.integers(0, 6) for _ in range(n)]
    num_valid = rng.random(n) < 0.9
    num = rng.integers(0, 3, n).astype(np.int64)
    o1_valid = rng.random(n) < 0.8
    o1 = rng.integers(-4, 4, n).astype(np.int64)
    o2 = rng.integers(0, 3, n).astype(np.float32)
    words = [None if rng.random() < 0.15 else "w%d" % i for i in range(n)]
    v_valid = rng.random(n) < 0.7
    v = rng.integers(-1000, 1000, n).astype(np.int32)
    u = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return dict(names=names, num=num, num_valid=num_valid, o1=o1, o1_valid=o1_valid, o2=o2, words=words, v=v, v_valid=v_valid, u=u)


WRAPPER_FUNCS = {"rn": "row_number", "rk": "rank", "dr": "dense_rank", "c": "count", "prev_w": ("lag", "w", 1), "next_v": ("lead", "v", 2),
                 "first_w": ("first", "w"), "last_u": ("last", "u"), "seen": ("cumcount", None), "seen_v": ("cumcount", "v"),
                 "sum_v": ("cumsum", "v"), "min_v": ("cummin", "v"), "max_u": ("cummax", "u"), "sum_u": ("cumsum", "u")}


def wrapper_call(fn, t, null_keys, **kw):
    return fn(WRAPPER_FUNCS, partition_by=[hj.KeyColumn.from_list(t["names"]), hj.KeyColumn(t["num"], t["num_valid"])],
              order_by=[hj.KeyColumn(t["o1"], t["o1_valid"]), t["o2"]], descending=[True, False], nulls=["first", "last"],
              cols={"w": hj.KeyColumn.from_list(t["words"]), "v": hj.KeyColumn(t["v"], t["v_valid"]), "u": t["u"]}, null_keys=null_keys, **kw)


def wrapper_check(got, t, null_keys):
    n = len(t["names"])
    keys = [(t["names"][i], int(t["num"][i]) if t["num_valid"][i] else None) for i in range(n)]
    cols = {"w": [None if w is None else w.encode() for w in t["words"]], "v": [int(x) if ok else None for x, ok in zip(t["v"], t["v_valid"])],
            "u": [int(x) for x in t["u"]]}
    want, n_parts, n_dropped = _loop_reference(keys, [(t["o1"], t["o1_valid"]), (t["o2"], None)], [True, False], ["first", "last"], null_keys, cols,
                                               WRAPPER_FUNCS)
    assert (got["n_partitions"], got["null_rows"]) == (n_parts, n_dropped) and got["perm"].size == n - n_dropped
    for name in ("rn", "rk", "dr", "c"):
        assert got[name].dtype == U32 and got[name].tolist() == want[name], name
    for name in ("seen", "seen_v"):
        assert got[name].dtype == U64 and got[name].tolist() == want[name], name
    for name in ("prev_w", "first_w"):
        assert got[name].to_list() == want[name], name
    for name, dtype in (("next_v", np.int32), ("last_u", U64), ("sum_v", np.int64), ("min_v", np.int64), ("max_u", U64), ("sum_u", U64)):
        col = got[name]
        assert isinstance(col, hj.KeyColumn) and col.values.dtype == dtype, (name, col.values.dtype)
        ok = col.valid if col.valid is not None else np.ones(n, dtype=bool)
        assert ok.tolist() == [x is not None for x in want[name]], name
        mod = 1 << (8 * col.values.dtype.itemsize)
        assert [int(x) % mod for x in col.values[ok]] == [x % mod for x in want[name] if x is not None], name
    rows = got["perm"].astype(np.int64)
    assert np.array_equal(np.sort(rows), np.setdiff1d(np.arange(n), np.flatnonzero(got["rn"] == 0)))
