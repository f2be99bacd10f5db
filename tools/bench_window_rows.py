#!/usr/bin/env python3
"""Times hj_window_rows_dev against what a user writes today with torch, on the same device, in the same process and on the
same tensors: development tool (profiles/window_rows.md).

    python tools/bench_window_rows.py [--log2n 27] [--shapes ...] [--perms random identity] [--funcs 1 8] [--reps 5] [--out FILE]

Both sides start from the ALREADY SORTED partition ids (position p holds the id of row perm[p]) and end with every result in
ROW order. The yardstick is the composition on those ids: unique_consecutive(return_counts=True), cumsum and
repeat_interleave give start, end and the size of every position's partition; index arithmetic gives ROW_NUMBER and the lag /
lead / first / last maps; cumsum(v[perm]) minus the gathered partition offsets gives the running sum; out[perm] = ... puts
each result in row order. Before anything is timed the tool checks that every output equals the yardstick's element for
element (`equal` in every row). One warm-up round, then --reps rounds, ours and the yardstick alternating, each between two
events on the stream.

--funcs 1: ROW_NUMBER alone. --funcs 8: ROW_NUMBER, PART_ROWS, LAG 1, LEAD 1, FIRST_ROW, LAST_ROW, RUN_SUM of an int64 column,
RUN_COUNT -- one call. Shapes: one partition, 2^10 and 2^20 equal partitions, every row its own, Zipf(1.0) sizes over 2^20 ids.

Per case one JSON line:
  window_us     hj_window_rows_dev, median (min..max as _min / _max); info_us: its own out[3]; partitions, chunks
  torch_us      the yardstick likewise; ratio = window_us / torch_us
  model_bytes   the algorithmic bytes of the call (below); model_GBps = model_bytes over window_us -- bytes the algorithm has
                to move over the call's time, a scattered access counted as its element, not as the line it moves

The byte model, per position: heads -- dPerm 4 B, two dPart rows 8 B, the head byte 1 B; summary -- the head byte and its
neighbour 2 B (the values behind a chunk's last head are left out); ends, where a function needs end -- 1 B read, 4 B written,
4 B read again; apply -- dPerm 4 B, the head byte 1 B, per function its entry (4 or 8 B) and, for RUN_SUM, the source 8 B.
"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: it ships its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib as W  # noqa: E402

SHAPES = ("one", "k1024", "k1048576", "each", "zipf")
EIGHT = ("row_number", "part_rows", "lag", "lead", "first", "last", "run_sum", "run_count")
_OPS = {"row_number": W.HJ_WIN_ROW_NUMBER, "part_rows": W.HJ_WIN_PART_ROWS, "lag": W.HJ_WIN_LAG, "lead": W.HJ_WIN_LEAD, "first": W.HJ_WIN_FIRST_ROW,
        "last": W.HJ_WIN_LAST_ROW, "run_sum": W.HJ_WIN_RUN_SUM, "run_count": W.HJ_WIN_RUN_COUNT}


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


def sorted_ids(shape, n, dev):
    """the partition id of every POSITION, non-decreasing, int32"""
    pos = torch.arange(n, dtype=torch.int64, device=dev)
    if shape == "one":
        return torch.zeros(n, dtype=torch.int32, device=dev)
    if shape == "each":
        return pos.to(torch.int32)
    if shape.startswith("k"):
        k = min(int(shape[1:]), n)
        return (pos // (n // k)).to(torch.int32)
    ids = min(1 << 20, n)                                        # Zipf(1.0): the size of id r is proportional to 1 / (r + 1)
    w = 1.0 / torch.arange(1, ids + 1, dtype=torch.float64, device=dev)
    sizes = (w / w.sum() * n).floor().to(torch.int64)
    sizes[0] += n - sizes.sum()
    return torch.repeat_interleave(torch.arange(ids, dtype=torch.int32, device=dev), sizes)


def yardstick(ids, perm, v, names):
    """the torch composition -> {name: result in row order}; the maps and numbers as int32 (NO_ROW is -1), the sums as int64"""
    n = ids.numel()
    _, counts = torch.unique_consecutive(ids, return_counts=True)
    offs = torch.cumsum(counts, 0) - counts
    start = torch.repeat_interleave(offs, counts)
    pos = torch.arange(n, dtype=torch.int64, device=ids.device)
    out, need_end = {}, any(k in names for k in ("part_rows", "lead", "last"))
    if need_end:
        size = torch.repeat_interleave(counts, counts)
        end = start + size - 1
    rows = perm.to(torch.int64)

    def in_row_order(x, dtype):
        o = torch.empty(n, dtype=dtype, device=ids.device)
        o[rows] = x.to(dtype)
        return o

    for name in names:
        if name in ("row_number", "run_count"):
            out[name] = in_row_order(pos - start + 1, torch.int32 if name == "row_number" else torch.int64)
        elif name == "part_rows":
            out[name] = in_row_order(size, torch.int32)
        elif name == "lag":
            out[name] = in_row_order(torch.where(pos - 1 >= start, perm[(pos - 1).clamp(min=0)], -1), torch.int32)
        elif name == "lead":
            out[name] = in_row_order(torch.where(pos + 1 <= end, perm[(pos + 1).clamp(max=n - 1)], -1), torch.int32)
        elif name == "first":
            out[name] = in_row_order(perm[start], torch.int32)
        elif name == "last":
            out[name] = in_row_order(perm[end], torch.int32)
        else:
            total = torch.cumsum(v[rows], 0)
            before = torch.where(start > 0, total[(start - 1).clamp(min=0)], 0)
            out[name] = in_row_order(total - before, torch.int64)
    return out


def model_bytes(n, names, has_part):
    need_end = any(k in names for k in ("part_rows", "lead", "last"))
    per = 4 + (8 if has_part else 0) + 1 + 2 + (9 if need_end else 0) + 5
    per += sum(8 if k in ("run_sum", "run_count") else 4 for k in names) + (8 if "run_sum" in names else 0)
    return n * per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--shapes", nargs="+", choices=SHAPES, default=list(SHAPES))
    ap.add_argument("--perms", nargs="+", choices=("random", "identity"), default=["random", "identity"])
    ap.add_argument("--funcs", nargs="+", type=int, choices=(1, 8), default=[1, 8])
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
        for shape in a.shapes:
            for how in a.perms:
                ids = sorted_ids(shape, n, dev)
                perm = (torch.randperm(n, device=dev, generator=g) if how == "random" else torch.arange(n, device=dev)).to(torch.int32)
                part = torch.empty(n, dtype=torch.int32, device=dev)
                part[perm.to(torch.int64)] = ids                     # the id of every ROW: what hj_key_groups_dev leaves
                v = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=dev, generator=g)
                for k in a.funcs:
                    names = EIGHT[:k]
                    outs = {name: torch.empty(n, dtype=torch.int64 if name.startswith("run") else torch.int32, device=dev) for name in names}
                    desc = [(_OPS[name], outs[name].data_ptr(), v.data_ptr() if name == "run_sum" else 0, 0, 8 if name == "run_sum" else 0,
                             W.HJ_AGG_SIGNED if name == "run_sum" else 0, 1 if name in ("lag", "lead") else 0) for name in names]
                    state = {}

                    def ours():
                        c.window_rows(perm.data_ptr(), n, n, part.data_ptr(), [], desc)

                    def theirs():
                        state["out"] = yardstick(ids, perm, v, names)

                    ours()
                    info = c.window_rows_info()
                    row = {"shape": shape, "perm": how, "funcs": k, "log2n": a.log2n, "partitions": info["partitions"], "chunks": info["chunks"],
                           "workspace_bytes": info["workspace_bytes"], "reps": a.reps}
                    if a.tag:
                        row["tag"] = a.tag
                    if not a.no_yardstick:
                        theirs()
                        c.synchronize()
                        row["equal"] = all(bool(torch.equal(state["out"][name], outs[name])) for name in names)
                        state.clear()
                    times = timed_alternating([ours] if a.no_yardstick else [ours, theirs], a.reps)
                    row.update(stats("window", times[0]))
                    row["info_us"] = c.window_rows_info()["us"]
                    row["model_bytes"] = model_bytes(n, names, True)
                    row["model_GBps"] = round(row["model_bytes"] / statistics.median(times[0]) / 1e3, 1)
                    if not a.no_yardstick:
                        row.update(stats("torch", times[1]))
                        row["ratio"] = round(statistics.median(times[0]) / statistics.median(times[1]), 3)
                    line = json.dumps(row)
                    print(line, flush=True)
                    if sink:
                        sink.write(line + "\n")
                        sink.flush()
                    del outs, desc
                    state.clear()
                    torch.cuda.empty_cache()
                del ids, perm, part, v
                torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
