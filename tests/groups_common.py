"""What the tests of hj_key_groups_dev / hj_key_groups_host share: the model -- a Python dict on the key's bytes -- and the
tables it is run on. A key is one `bytes | None` per key column (a None inside it: a NULL that equals NULLs), or None for a
NULL-keyed row. Nothing here calls the library's hash, its compare or its grouping."""
import numpy as np

import keys2_common as k2

NO_ROW = 0xFFFFFFFF
U32 = np.uint32
MASKS = [0, 0xFFFF, 0xF, 0x1]


def model_groups(keys, capacity=None):
    """keys: one hashable or None (NULL-keyed) per row -> {"rep", "group", "first_rows" (cut at capacity), "n_groups",
    "null_rows"} as hj_key_groups_dev defines them: the lowest row of the key, the dense id in order of first occurrence"""
    first, rep, group, rows, nulls = {}, [], [], [], 0
    for i, k in enumerate(keys):
        if k is None:
            rep.append(NO_ROW)
            group.append(NO_ROW)
            nulls += 1
            continue
        if k not in first:
            first[k] = (i, len(rows))
            rows.append(i)
        rep.append(first[k][0])
        group.append(first[k][1])
    cut = len(rows) if capacity is None else min(capacity, len(rows))
    return {"rep": np.array(rep, dtype=U32), "group": np.array(group, dtype=U32), "first_rows": np.array(rows[:cut], dtype=U32),
            "n_groups": len(rows), "null_rows": nulls}


def model_keys(cols, nulls):
    """the keys of a table of keys2_common.ModelCol columns under nulls = "group" | "drop" """
    return k2.row_keys(cols, nulls_equal=(nulls == "group"))


def array_keys(arrays):
    """the keys of plain numpy columns: the bytes of the row's elements, one per column"""
    raws = [(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)) for a in arrays]
    rec = np.ascontiguousarray(np.concatenate(raws, axis=1))
    raw, w = rec.tobytes(), rec.shape[1]
    return [raw[i * w:(i + 1) * w] for i in range(rec.shape[0])]


def same(got, want, tag=None):
    """a result dict of key_groups / key_groups_host against the model's, bit for bit"""
    for k in ("rep", "group", "first_rows"):
        assert got[k].dtype == U32 and np.array_equal(got[k], want[k]), (tag, k)
    assert (got["n_groups"], got["null_rows"]) == (want["n_groups"], want["null_rows"]), (tag, got["n_groups"], got["null_rows"])


# ---- tables ----------------------------------------------------------------------------------------------------------------
def fixed_table(rng, widths, n, distinct, nulls=0.0):
    """n rows of fixed columns of `widths`, about `distinct` distinct rows: every column draws from its own small pool, so
    rows agree in some columns and differ in others"""
    per = max(2, int(round(distinct ** (1.0 / len(widths)))))
    return [k2.fixed_col(rng, w, n, nulls=nulls, distinct=per) for w in widths]


def string_col(rng, n, distinct, nulls=0.0, lo=0, hi=40):
    """n strings of lo .. hi bytes out of `distinct`, some a prefix of another, a share `nulls` of them None"""
    pool = [rng.integers(97, 100, size=int(rng.integers(lo, hi + 1)), dtype=np.uint8).tobytes() for _ in range(distinct)]
    pool += [p[:len(p) // 2] for p in pool[:distinct // 4] if len(p) // 2 >= lo]
    pick = rng.integers(0, len(pool), n)
    gone = rng.random(n) < nulls
    return k2.ModelCol(0, [None if g else pool[p] for p, g in zip(pick, gone)], False)


def key_columns(cols, nulls_equal=False):
    """the KeyColumns of model columns; variable-length ones start at changing, unaligned offsets"""
    return [k2.key_column(c._replace(nulls_equal=nulls_equal), lead=1 + k % 3) for k, c in enumerate(cols)]
