#!/usr/bin/env python3
"""Times hj_key_groups_dev and the group-by built on it against what a user writes today with torch, on the same device,
in the same process and on the same data: development tool (profiles/key_groups.md).

    python tools/bench_key_groups.py [--log2n 27] [--log2s 24] [--cases all n16 k1024 zipf strings] [--reps 5]
                                     [--no-yardstick] [--out FILE]

One context created with hj_create_on_stream on torch's current stream; every buffer is a torch tensor whose data_ptr() goes
to the C ABI. The cases -- n = 2^log2n rows of one 8-byte column:
  all      n distinct keys (a random permutation)
  n16      n / 16 distinct keys, uniform draws
  k1024    2^10 distinct keys, uniform draws
  zipf     draws from n keys with P(k) ~ 1 / rank(k)^theta (--theta, default 1.0), by inverse CDF with torch
and 2^log2s rows of one string column:
  strings  strings of 8 to 24 bytes drawn from 2^log2s / 16 distinct ones, in the Arrow layout (offsets + bytes)
Per case one JSON line; every time is the median with minimum and maximum over `reps` launches after one warm-up launch, each
launch between two events on the stream, ours and the yardstick alternating:
  groups_us     hj_key_groups_dev with all three outputs (the table's fill included); groups_info_us: its own out[2]
  unique_us     the yardstick: torch.unique(keys, return_inverse=True) -- for the strings, over the rows padded to 24 bytes
                with their length as 4 int64 columns, torch.unique(dim=0, return_inverse=True)
  groupby_us    hj_key_groups_dev + hj_pairs_agg_dev (dMapG = the ids, dMapV = the identity) for SUM, MIN, MAX of one int64
                column and COUNT; agg_us: that hj_pairs_agg_dev alone
  torch_groupby_us  the yardstick: torch.unique(return_inverse=True) + index_add_ (SUM, COUNT) + scatter_reduce_ (amin, amax);
                torch_agg_us: those reductions alone
  equal         our groups are torch's (same number, rep = the lowest row of torch's class, every row's first row holds its
                key) and our aggregates are torch's, reordered by first occurrence -- checked before anything is timed
  model_GBps    the byte model of profiles/key_groups.md over groups_us
--no-yardstick leaves torch out (for a profiler run over our kernels alone)."""
import argparse
import json
import os
import statistics
import sys

import torch  # first: it ships its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib  # noqa: E402

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
OPS = [(_lib.HJ_AGG_SUM, 8, _lib.HJ_AGG_SIGNED), (_lib.HJ_AGG_MIN, 8, _lib.HJ_AGG_SIGNED), (_lib.HJ_AGG_MAX, 8, _lib.HJ_AGG_SIGNED),
       (_lib.HJ_AGG_COUNT, 0, 0)]
IDENTITY = [0, I64_MAX, I64_MIN, 0]
CASES = ("all", "n16", "k1024", "zipf", "strings")


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


def zipf_keys(n, theta, dev, g):
    w = torch.arange(1, n + 1, dtype=torch.float64, device=dev).pow_(-theta)
    cdf = torch.cumsum(w, 0)
    cdf /= cdf[-1].clone()
    ranks = torch.searchsorted(cdf, torch.rand(n, dtype=torch.float64, device=dev, generator=g)).clamp_(max=n - 1)
    return torch.randperm(n, device=dev, generator=g)[ranks] + 1


def fixed_case(name, n, theta, dev, g):
    """-> (the hj_key_col2 tuples, what torch.unique takes, its dim, what keeps the buffers alive, key bytes per row)"""
    if name == "all":
        keys = torch.randperm(n, device=dev, generator=g) + (1 << 40)
    elif name == "zipf":
        keys = zipf_keys(n, theta, dev, g)
    else:
        distinct = n // 16 if name == "n16" else 1 << 10
        keys = torch.randint(0, distinct, (n,), dtype=torch.int64, device=dev, generator=g) * 0x9E3779B97F4A7C1 + 12345
    return [(keys.data_ptr(), 0, 8)], keys, None, [keys], 8.0


def string_case(n, dev, g):
    """strings of 8 to 24 bytes out of n / 16 distinct ones: the Arrow column for us, the padded rows for torch"""
    pool = max(n // 16, 1)
    pool_len = torch.randint(8, 25, (pool,), dtype=torch.int64, device=dev, generator=g)
    pool_bytes = torch.randint(0, 256, (pool, 24), dtype=torch.uint8, device=dev, generator=g)
    pool_bytes *= (torch.arange(24, device=dev)[None, :] < pool_len[:, None])          # zero behind the end: the padded form
    pick = torch.randint(0, pool, (n,), dtype=torch.int64, device=dev, generator=g)
    lens = pool_len[pick]
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=offsets[1:])
    total = int(offsets[-1])
    row = torch.repeat_interleave(torch.arange(n, device=dev), lens, output_size=total)
    data = pool_bytes[pick[row], torch.arange(total, device=dev) - offsets[row]].contiguous()
    data = torch.cat([data, torch.zeros(4, dtype=torch.uint8, device=dev)])            # whole words behind the last element
    off32 = offsets.to(torch.int32)                                                     # total < 2^31 at these sizes
    padded = torch.cat([pool_bytes[pick].contiguous().view(torch.int64), lens[:, None]], 1).contiguous()
    return [(data.data_ptr(), 0, 0, off32.data_ptr(), 0)], padded, 0, [data, off32, padded], total / n + 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--log2s", type=int, default=24)
    ap.add_argument("--cases", nargs="+", choices=CASES, default=list(CASES))
    ap.add_argument("--theta", type=float, default=1.0)
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

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    with hj.HashJoinContext(0, stream=torch.cuda.current_stream().cuda_stream) as c:
        for name in a.cases:
            n = 1 << (a.log2s if name == "strings" else a.log2n)
            cols, keys, dim, held, key_bytes = string_case(n, dev, g) if name == "strings" else fixed_case(name, n, a.theta, dev, g)
            vals = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=dev, generator=g)
            ident = torch.arange(n, dtype=torch.int32, device=dev)
            ones = torch.ones(n, dtype=torch.int64, device=dev)
            rep, group, first = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))

            def run_groups():
                c.key_groups(cols, hj.HJ_KEY_SIDE_S, n, rep.data_ptr(), group.data_ptr(), first.data_ptr(), n)

            run_groups()
            info = c.key_groups_info()
            assert info["failure"] == 0, info
            m = info["groups"]
            acc = [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(4)]
            base = [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(4)]

            def run_agg():
                for k in range(4):
                    acc[k].fill_(IDENTITY[k])
                c.pairs_agg(group.data_ptr(), ident.data_ptr(), n, 0, m, 0, n,
                            [(vals.data_ptr() if OPS[k][1] else 0, 0, acc[k].data_ptr()) + OPS[k] for k in range(4)])

            def run_groupby():
                run_groups()
                run_agg()

            state = {}

            def run_unique():
                state["uniq"], state["inv"] = torch.unique(keys, return_inverse=True, dim=dim)

            def run_torch_agg():
                inv = state["inv"]
                for k in range(4):
                    base[k].fill_(IDENTITY[k])
                base[0].index_add_(0, inv, vals)
                base[1].scatter_reduce_(0, inv, vals, "amin", include_self=True)
                base[2].scatter_reduce_(0, inv, vals, "amax", include_self=True)
                base[3].index_add_(0, inv, ones)

            def run_torch_groupby():
                run_unique()
                run_torch_agg()

            row = {"case": name, "log2n": a.log2s if name == "strings" else a.log2n, "groups": m, "slots": info["slots"], "reps": a.reps}
            if a.tag:
                row["tag"] = a.tag
            run_agg()
            if not a.no_yardstick:
                run_torch_groupby()
                c.synchronize()
                inv, rows = state["inv"], torch.arange(n, dtype=torch.int64, device=dev)
                lowest = torch.full((state["uniq"].shape[0],), n, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, rows, "amin")
                rep64, group64, first64 = rep.to(torch.int64), group.to(torch.int64), first[:m].to(torch.int64)
                same_key = torch.equal(keys[first64[group64]], keys)
                equal = (state["uniq"].shape[0] == m and torch.equal(lowest[inv], rep64) and torch.equal(first64[group64], rep64) and same_key
                         and bool((first64[1:] > first64[:-1]).all()) and all(torch.equal(base[k][inv[first64]], acc[k]) for k in range(4)))
                row["equal"] = bool(equal)
                del lowest, rep64, group64, first64, rows
            c.synchronize()
            fns = [run_groups, run_groupby, run_agg] + ([] if a.no_yardstick else [run_unique, run_torch_groupby, run_torch_agg])
            times = timed_alternating(fns, a.reps)
            info = c.key_groups_info()
            row.update(stats("groups", times[0]))
            row.update(stats("groupby", times[1]))
            row.update(stats("agg", times[2]))
            row.update({"groups_info_us": info["us"], "probe_steps_per_row": round(info["probe_steps"] / n, 3), "collisions": info["collisions"]})
            # per slot 8 B of fill; per row: the key bytes (and offsets), one 8-byte slot read and one written (the insert), the slot
            # number written and read back, the slot read again (the resolve), rep written and read (the ids), group written
            model = 8 * info["slots"] + n * (key_bytes + 8 + 8 + 4 + 4 + 8 + 4 + 4 + 4) + 4 * m
            row["model_GBps"] = round(model / statistics.median(times[0]) / 1e3, 1)
            if not a.no_yardstick:
                row.update(stats("unique", times[3]))
                row.update(stats("torch_groupby", times[4]))
                row.update(stats("torch_agg", times[5]))
                row["groups_ratio"] = round(statistics.median(times[0]) / statistics.median(times[3]), 3)
                row["groupby_ratio"] = round(statistics.median(times[1]) / statistics.median(times[4]), 3)
                row["agg_ratio"] = round(statistics.median(times[2]) / statistics.median(times[5]), 3)
            emit(row)
            del held, keys, vals, ident, ones, rep, group, first, acc, base
            state.clear()
            torch.cuda.empty_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
