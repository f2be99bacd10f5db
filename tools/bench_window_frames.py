#!/usr/bin/env python3
"""Times hj_window_frames_dev against what a user writes today with torch, on the same device, in the same process and on the
same tensors: development tool (profiles/window_frames.md).

    python tools/bench_window_frames.py [--log2n 27] [--widths 7 64 4096 1048576 0] [--ops sum min] [--shapes ...]
                                        [--perms random identity] [--funcs 1 8] [--reps 5] [--out FILE]

Both sides start from the ALREADY SORTED partition ids (position p holds the id of row perm[p]) and end with every result in
ROW order. A width W is the trailing frame ROWS BETWEEN W - 1 PRECEDING AND CURRENT ROW; width 0 is the whole partition (both
sides unbounded). --funcs 8: eight functions of one call over one int64 column, trailing frames of W, W + 1, .. W + 7.
The yardstick:
  sum       cumsum(v[perm]) differences, the lower end clamped to the partition's start (unique_consecutive, cumsum,
            repeat_interleave on the sorted ids); out[perm] = ... for row order
  min       W <= 64: W - 1 shifted torch.minimum steps, each masked by the partition's start. Above 64, and for the whole
            partition, torch has no composition a user would write: the row holds our time and the byte model alone.
Before anything is timed the tool checks that every output equals the yardstick's element for element (`equal`). One warm-up
round, then --reps rounds, ours and the yardstick alternating, each between two events on the stream.

Per case one JSON line: frames_us (median, _min, _max), info_us (the call's own out[3]), torch_us likewise and ratio =
frames_us / torch_us where there is a yardstick, model_bytes and model_GBps = model_bytes over frames_us.

The byte model, per position, a scattered access counted as its element: once per call -- heads: dPerm 4 B, two dPart rows 8 B,
the head byte 1 B; summary 2 B; ends 1 B read, 4 B written. Per function -- values: dPerm 4 B, the source 8 B, the value plane
8 B; each scan that runs (two with both sides bounded, one otherwise): the head byte 1 B, 8 B read, 8 B written; combine: the
head byte 1 B, the end 4 B, dPerm 4 B, G and / or H 8 B each, the output 8 B.
"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: it ships its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib as W  # noqa: E402
from bench_window_rows import sorted_ids, stats, timed_alternating  # noqa: E402

SHAPES = ("one", "k1024", "k1048576", "zipf")
BIG = (1 << 63) - 1


def frames_of(width, k):
    """the k frames of a case: (lo, hi), None for an unbounded side"""
    return [(None, None)] * k if width == 0 else [(-(width - 1 + i), 0) for i in range(k)]


def yardstick(ids, perm, v, op, frames):
    """the torch composition -> [result in row order per frame], or None where torch has none"""
    if op == "min" and any(lo is None or -lo + 1 > 64 for lo, _ in frames):
        return None
    n = ids.numel()
    _, counts = torch.unique_consecutive(ids, return_counts=True)
    offs = torch.cumsum(counts, 0) - counts
    start = torch.repeat_interleave(offs, counts)
    pos = torch.arange(n, dtype=torch.int64, device=ids.device)
    rows = perm.to(torch.int64)
    x = v[rows]
    res = []
    if op == "sum":
        total = torch.cumsum(x, 0)
        for lo, hi in frames:
            if lo is None:
                end = start + torch.repeat_interleave(counts, counts) - 1
                r = total[end] - torch.where(start > 0, total[(start - 1).clamp(min=0)], 0)
            else:
                left = torch.maximum(start, pos + lo)
                r = total - torch.where(left > 0, total[(left - 1).clamp(min=0)], 0)
            o = torch.empty(n, dtype=torch.int64, device=ids.device)
            o[rows] = r
            res.append(o)
        return res
    for lo, hi in frames:
        acc = x.clone()
        for k in range(1, -lo + 1):
            acc[k:] = torch.minimum(acc[k:], torch.where(start[k:] <= pos[k:] - k, x[:-k], BIG))
        o = torch.empty(n, dtype=torch.int64, device=ids.device)
        o[rows] = acc
        res.append(o)
    return res


def model_bytes(n, frames):
    per = 13 + 2 + 5
    for lo, hi in frames:
        scans = 2 if lo is not None and hi is not None else 1
        per += 20 + 17 * scans + 17 + 8 * scans
    return n * per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--widths", nargs="+", type=int, default=[7, 64, 1 << 12, 1 << 20, 0])
    ap.add_argument("--ops", nargs="+", choices=("sum", "min"), default=["sum", "min"])
    ap.add_argument("--shapes", nargs="+", choices=SHAPES, default=list(SHAPES))
    ap.add_argument("--perms", nargs="+", choices=("random", "identity"), default=["random", "identity"])
    ap.add_argument("--funcs", nargs="+", type=int, choices=(1, 8), default=[1, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    sink = open(a.out, "a") if a.out else None
    n = 1 << a.log2n
    ops = {"sum": W.HJ_AGG_SUM, "min": W.HJ_AGG_MIN}

    with hj.HashJoinContext(0, stream=torch.cuda.current_stream().cuda_stream) as c:
        for shape in a.shapes:
            for how in a.perms:
                ids = sorted_ids(shape, n, dev)
                perm = (torch.randperm(n, device=dev, generator=g) if how == "random" else torch.arange(n, device=dev)).to(torch.int32)
                part = torch.empty(n, dtype=torch.int32, device=dev)
                part[perm.to(torch.int64)] = ids                     # the id of every ROW: what hj_key_groups_dev leaves
                v = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=dev, generator=g)
                for op in a.ops:
                    for width in a.widths:
                        for k in a.funcs:
                            frames = frames_of(width, k)
                            outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in frames]
                            desc = [(ops[op], o.data_ptr(), lo, hi, v.data_ptr(), 0, 8, W.HJ_AGG_SIGNED) for o, (lo, hi) in zip(outs, frames)]
                            state = {}

                            def ours():
                                c.window_frames(perm.data_ptr(), n, n, part.data_ptr(), desc)

                            def theirs():
                                state["out"] = yardstick(ids, perm, v, op, frames)

                            ours()
                            info = c.window_frames_info()
                            row = {"shape": shape, "perm": how, "op": op, "width": width, "funcs": k, "log2n": a.log2n, "partitions": info["partitions"],
                                   "chunks": info["chunks"], "workspace_bytes": info["workspace_bytes"], "reps": a.reps}
                            has = False
                            if not a.no_yardstick:
                                theirs()
                                c.synchronize()
                                has = state["out"] is not None
                                if has:
                                    row["equal"] = all(bool(torch.equal(t, o)) for t, o in zip(state["out"], outs))
                                state.clear()
                            times = timed_alternating([ours, theirs] if has else [ours], a.reps)
                            row.update(stats("frames", times[0]))
                            row["info_us"] = c.window_frames_info()["us"]
                            row["model_bytes"] = model_bytes(n, frames)
                            row["model_GBps"] = round(row["model_bytes"] / statistics.median(times[0]) / 1e3, 1)
                            if has:
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
