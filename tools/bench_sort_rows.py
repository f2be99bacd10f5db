#!/usr/bin/env python3
"""Times hj_sort_rows_dev against what a user writes today with torch, on the same device, in the same process and on the
same tensors: development tool (profiles/sort_rows.md).

    python tools/bench_sort_rows.py [--log2n 27] [--cases ...] [--reps 5] [--out profiles/sort_rows.jsonl]

The yardstick: one column -- torch.sort(x, stable=True) for the indices; several columns -- the chain of stable sorts from the
last column to the first with index_select between them; NULLs -- the values under them set to 0 and one more stable sort on
the flag; DESC -- descending=True; floats -- the NaNs made one NaN first, so that a negative one does not sort by its sign
bit. Before anything is timed the tool checks that our permutation equals torch's element for element (both are stable, so
they must be equal; `equal` in every row -- it also shows that torch's descending sort is stable). One warm-up round, then --reps rounds, ours and the yardstick alternating, each between two events on the stream.

Per case one JSON line:
  sort_us       hj_sort_rows_dev, median (min..max as _min / _max); info_us: its own out[2]; passes, chunks, chunk_rows
  torch_us      the yardstick likewise; ratio = sort_us / torch_us
  model_bytes   the algorithmic bytes of the call (below); model_GBps = model_bytes over sort_us -- bytes the algorithm has
                to move over the call's time, not a kernel's share of the memory system's peak

The byte model, per column: the keys kernel reads the element (and 4 B of row where it gathers, 1/8 B of validity) and writes
the key (and 4 B of row where the rows are the identity); per pass a histogram read of the key plane, a record read (key + 4
B) and a record write (the last byte pass of a column writes 4 B of rows alone); a validity pass reads 4 B twice and writes 4.
"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: it ships its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib  # noqa: E402

CASES = ("i64_perm", "i64_k1024", "i32_rand", "f32_nan", "i64_null10", "i32desc_i64", "four_i32_k256")
_TYPE = {torch.int64: _lib.HJ_VAL_INT, torch.int32: _lib.HJ_VAL_INT, torch.float32: _lib.HJ_VAL_FLOAT}


def timed_alternating(fns, reps):
    """-> one list of microseconds per function: reps rounds after one warm-up round, the functions taking turns, each
    launch between two events on the current stream"""
    out = [[] for _ in fns]
    for k in range(reps + 1):
        for i, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if k:
                out[i].append(t0.elapsed_time(t1) * 1000.0)
    return out


def stats(prefix, us):
    return {prefix + "_us": round(statistics.median(us), 1), prefix + "_us_min": round(min(us), 1), prefix + "_us_max": round(max(us), 1)}


def make_case(name, n, dev, g):
    """-> [(values tensor, null mask or None, descending)], the most significant column first"""
    ri = lambda lo, hi, dt: torch.randint(lo, hi, (n,), dtype=dt, device=dev, generator=g)      # noqa: E731
    if name == "i64_perm":
        return [(torch.randperm(n, device=dev, generator=g) - n // 2, None, False)]
    if name == "i64_k1024":
        return [(ri(0, 1 << 10, torch.int64), None, False)]
    if name == "i32_rand":
        return [(ri(-(1 << 31), 1 << 31, torch.int32), None, False)]
    if name == "f32_nan":
        x = torch.randn(n, dtype=torch.float32, device=dev, generator=g)
        r = torch.rand(n, device=dev, generator=g)
        x[r < 0.005] = float("nan")
        x[r > 0.995] = -float("nan")
        return [(x, None, False)]
    if name == "i64_null10":
        return [(ri(-(1 << 62), 1 << 62, torch.int64), torch.rand(n, device=dev, generator=g) < 0.1, False)]
    if name == "i32desc_i64":
        return [(ri(0, 1 << 16, torch.int32), None, True), (ri(-(1 << 62), 1 << 62, torch.int64), None, False)]
    return [(ri(0, 1 << 8, torch.int32), None, False) for _ in range(4)]


def pack_plane(valid):
    """one bool per row -> the validity plane of the C ABI (bit i & 31 of word i >> 5), as an int32 tensor"""
    n = valid.numel()
    bits = torch.zeros((n + 31) // 32 * 32, dtype=torch.int64, device=valid.device)
    bits[:n] = valid
    words = (bits.view(-1, 32) << torch.arange(32, device=valid.device)).sum(1)
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)          # the same 32 bits as an int32


def torch_order(cols):
    """the chain a user composes: stable sorts from the last column to the first -> int64 indices"""
    idx = None
    for x, null, desc in reversed(cols):
        v = x if null is None else x.masked_fill(null, 0)
        if v.is_floating_point():
            v = torch.where(v != v, float("nan"), v)           # one NaN for all of them: NaNs last whatever their sign, as numpy has it
        if idx is not None:
            v = v.index_select(0, idx)
        step = torch.sort(v, stable=True, descending=desc).indices
        idx = step if idx is None else idx.index_select(0, step)
        if null is not None:
            step = torch.sort(null.index_select(0, idx), stable=True).indices          # False (valid) first: NULLs last
            idx = idx.index_select(0, step)
    return idx


def model_bytes(cols, n):
    kb = 8 if any(x.element_size() == 8 for x, _, _ in cols) else 4
    total = 0
    for i, (x, null, _) in enumerate(reversed(cols)):
        w = x.element_size()
        k = 8 if w == 8 else 4
        total += n * (w + k + 4 + (0.125 if null is not None else 0))          # the keys kernel: element, key, 4 B of row read or written
        for d in range(w):
            total += n * (k + (k + 4) + ((k + 4) if d + 1 < w else 4))
        if null is not None:
            total += n * (4 + 0.125 + 4 + 0.125 + 4)
    return int(total), kb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--cases", nargs="+", choices=CASES, default=list(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--tag", default="", help="copied into every row")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    sink = open(a.out, "a") if a.out else None
    n = 1 << a.log2n

    with hj.HashJoinContext(0, stream=torch.cuda.current_stream().cuda_stream) as c:
        for name in a.cases:
            cols = make_case(name, n, dev, g)
            planes = [None if null is None else pack_plane(~null) for _, null, _ in cols]
            desc = [(x.data_ptr(), p.data_ptr() if p is not None else 0, x.element_size(), _TYPE[x.dtype], _lib.HJ_SORT_DESC if d else 0)
                    for (x, _, d), p in zip(cols, planes)]
            perm = torch.empty(n, dtype=torch.int32, device=dev)
            state = {}

            def ours():
                c.sort_rows(desc, n, perm.data_ptr())

            def yardstick():
                state["idx"] = torch_order(cols)

            ours()
            info = c.sort_rows_info()
            row = {"case": name, "log2n": a.log2n, "cols": [(str(x.dtype).replace("torch.", ""), null is not None, d) for x, null, d in cols],
                   "passes": info["passes"], "chunks": info["chunks"], "chunk_rows": info["chunk_rows"], "workspace_bytes": info["workspace_bytes"],
                   "reps": a.reps}
            if a.tag:
                row["tag"] = a.tag
            if not a.no_yardstick:
                yardstick()
                c.synchronize()
                row["equal"] = bool(torch.equal(state["idx"].to(torch.int32), perm))          # rows < 2^31: int32 holds them
                state.clear()
            times = timed_alternating([ours] if a.no_yardstick else [ours, yardstick], a.reps)
            row.update(stats("sort", times[0]))
            row["info_us"] = c.sort_rows_info()["us"]
            total, _ = model_bytes(cols, n)
            row["model_bytes"] = total
            row["model_GBps"] = round(total / statistics.median(times[0]) / 1e3, 1)
            if not a.no_yardstick:
                row.update(stats("torch", times[1]))
                row["ratio"] = round(statistics.median(times[0]) / statistics.median(times[1]), 3)
            line = json.dumps(row)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
            del cols, planes, desc, perm
            state.clear()
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
