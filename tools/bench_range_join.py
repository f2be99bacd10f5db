#!/usr/bin/env python3
"""Times hj_range_index_dev and hj_range_pairs_dev against the composition a user writes today with torch -- torch.sort, two
torch.searchsorted, cumsum, repeat_interleave and the arithmetic that turns them into the two maps -- on the same device, in
the same process and on the same data: development tool (profiles/range_join.md).

    python tools/bench_range_join.py [--log2n 27] [--dtypes int64 float32] [--cases avg0 avg1 avg8 skew marks last] [--reps 5]
                                     [--out FILE]

One context created with hj_create_on_stream on torch's current stream; every buffer is a torch tensor whose data_ptr() goes
to the C ABI. |R| = |S| = n = 2^log2n. R's values are uniform with one row per unit of the domain on average:
  avg0 / avg1 / avg8  every S row's closed interval holds 0 (lo > hi), 1 and 8 R rows on average
  skew   eight S rows cover all of R, the others one row on average; the capacity (n pairs) bounds what is written
  marks  avg8 as the mark-only pass of the semi / anti kinds: capacity 0, both mark planes
  last   pick = LAST with lo unbounded (the keyless backward as-of) against ONE torch.searchsorted on the sorted values
Per case one JSON line; every time is the median with minimum and maximum over `reps` launches after one warm-up launch, each
launch between two events on the stream, ours and the yardstick alternating:
  index_us / sort_us      hj_range_index_dev against torch.sort(values) (values and permutation)
  size_us                 the sizing pass: capacity 0, no planes
  range_us                the call at the exact capacity (info_us: its own out[2])
  torch_us                the yardstick from the sorted values to the two maps, its .item() for the total included, as size_us +
                          range_us include ours; at `marks`: the two searches and two scatter passes that set the planes
  equal                   the totals agree and so does a 64-bit checksum over the pairs -- checked before anything is timed
  model_GBps              the byte model of profiles/range_join.md over range_us"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: it ships its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402

CASES = ("avg0", "avg1", "avg8", "skew", "marks", "last")
DTYPES = {"int64": (torch.int64, 8, hj.HJ_VAL_INT), "float32": (torch.float32, 4, hj.HJ_VAL_FLOAT)}
C1, C2 = 0x9E3779B97F4A7C15 - (1 << 64), 0x632BE59BD9B4E019


def timed_alternating(fns, reps):
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


def checksum(s, r):
    return int(((s.to(torch.int64) * C1) ^ (r.to(torch.int64) * C2)).sum())


def make(case, n, dtype, dev, g):
    """-> (R values, lo or None, hi)"""
    k = {"avg0": 0, "avg1": 1, "avg8": 8, "skew": 1, "marks": 8, "last": 1}[case]
    if dtype == torch.int64:
        r = torch.randint(0, n, (n,), dtype=dtype, device=dev, generator=g)
        lo = torch.randint(0, n, (n,), dtype=dtype, device=dev, generator=g)
        hi = lo + (k - 1)
        top = 1 << 62
    else:
        r = torch.rand(n, dtype=dtype, device=dev, generator=g)
        lo = torch.rand(n, dtype=dtype, device=dev, generator=g)
        hi = lo + (k / n if k else -1e-3)
        top = 2.0
    if case == "skew":
        at = torch.randint(0, n, (8,), device=dev, generator=g)
        lo[at], hi[at] = -top, top
    return r, (None if case == "last" else lo), hi


def torch_pairs(sorted_r, perm, lo, hi):
    a = torch.searchsorted(sorted_r, lo)
    b = torch.searchsorted(sorted_r, hi, right=True)
    cnt = (b - a).clamp_(min=0)
    off = torch.cumsum(cnt, 0)
    total = int(off[-1].item())
    s_idx = torch.repeat_interleave(torch.arange(lo.numel(), device=lo.device), cnt, output_size=total)
    r_pos = torch.arange(total, device=lo.device) - (off - cnt)[s_idx] + a[s_idx]
    return s_idx, perm[r_pos], total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--dtypes", nargs="+", choices=list(DTYPES), default=list(DTYPES))
    ap.add_argument("--cases", nargs="+", choices=CASES, default=list(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    n = 1 << a.log2n
    layout = hj.range_layout_info(n, n)
    steps = layout["stride"].bit_length() - 1
    rows = []
    with hj.HashJoinContext(0, stream=torch.cuda.current_stream().cuda_stream) as ctx:
        for name in a.dtypes:
            dtype, width, vtype = DTYPES[name]
            for case in a.cases:
                g.manual_seed(1234)
                r, lo, hi = make(case, n, dtype, dev, g)
                perm = torch.empty(n, dtype=torch.int32, device=dev)
                keys = torch.empty(n, dtype=torch.int64 if width == 8 else torch.int32, device=dev)
                head = torch.empty(4, dtype=torch.int32, device=dev)
                pick = hj.HJ_RANGE_LAST if case == "last" else hj.HJ_RANGE_ALL
                term = (lo.data_ptr() if lo is not None else 0, hi.data_ptr(), width, vtype, 0, pick)
                index = lambda: ctx.range_index((r.data_ptr(), 0, width, vtype), n, perm.data_ptr(), keys.data_ptr(), head.data_ptr())  # noqa: E731
                index()
                row = {"case": case, "dtype": name, "log2n": a.log2n, "tag": a.tag, "stride": layout["stride"], "pivots": layout["pivots"]}
                sorted_r, t_perm = torch.sort(r)
                if case == "marks":
                    s_marks, r_marks = torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev), torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev)
                    ours = lambda: ctx.range_pairs(keys.data_ptr(), perm.data_ptr(), head.data_ptr(), n, term, n, 0, 0, 0, 0, s_marks.data_ptr(), r_marks.data_ptr())  # noqa: E731

                    def yard():
                        x, y = torch.searchsorted(sorted_r, lo), torch.searchsorted(sorted_r, hi, right=True)
                        s_hit = y > x
                        diff = torch.zeros(n + 1, dtype=torch.int32, device=dev)
                        diff.index_add_(0, x, s_hit.to(torch.int32))
                        diff.index_add_(0, y, -s_hit.to(torch.int32))
                        r_hit = torch.zeros(n, dtype=torch.bool, device=dev)
                        r_hit[t_perm] = torch.cumsum(diff, 0)[:-1] > 0
                        return s_hit, r_hit

                    ours()
                    info = ctx.range_pairs_info()
                    s_hit, r_hit = yard()
                    bits = lambda w: ((w[:, None] >> torch.arange(32, device=dev, dtype=torch.int32)[None, :]) & 1).bool().reshape(-1)[:n]  # noqa: E731
                    row["equal"] = bool(torch.equal(bits(s_marks), s_hit) and torch.equal(bits(r_marks), r_hit)) and info[3] == int(s_hit.sum())
                    row["pairs"] = info[0]
                    t_idx, t_sort, t_ours, t_yard = timed_alternating([index, lambda: torch.sort(r), ours, yard], a.reps)
                    row.update(stats("index", t_idx), **stats("sort", t_sort), **stats("range", t_ours), **stats("torch", t_yard))
                    pairs_rw = 0
                elif case == "last":
                    cap = n
                    out_s, out_r = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
                    ours = lambda: ctx.range_pairs(keys.data_ptr(), perm.data_ptr(), head.data_ptr(), n, term, n, 0, out_s.data_ptr(), out_r.data_ptr(), cap)  # noqa: E731
                    yard = lambda: torch.searchsorted(sorted_r, hi, right=True)  # noqa: E731
                    ours()
                    info = ctx.range_pairs_info()
                    b = yard()
                    hit = b > 0
                    # the winner's VALUE is what the yardstick's position gives; its row is ours alone (ties to the lowest row)
                    got = torch.zeros(n, dtype=dtype, device=dev)
                    got[out_s[:info[1]].long()] = r[out_r[:info[1]].long()]
                    row["equal"] = info[0] == int(hit.sum()) and bool(torch.equal(got[hit], sorted_r[(b - 1).clamp_(min=0)][hit]))
                    row["pairs"] = info[0]
                    t_idx, t_sort, t_ours, t_yard = timed_alternating([index, lambda: torch.sort(r), ours, yard], a.reps)
                    row.update(stats("index", t_idx), **stats("sort", t_sort), **stats("range", t_ours), **stats("torch", t_yard))
                    pairs_rw = info[1]
                else:
                    size = lambda: ctx.range_pairs(keys.data_ptr(), perm.data_ptr(), head.data_ptr(), n, term, n, 0, 0, 0, 0)  # noqa: E731
                    size()
                    total = ctx.range_pairs_info()[0]
                    cap = min(total, n) if case == "skew" else total
                    out_s, out_r = torch.empty(max(cap, 1), dtype=torch.int32, device=dev), torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
                    ours = lambda: ctx.range_pairs(keys.data_ptr(), perm.data_ptr(), head.data_ptr(), n, term, n, 0, out_s.data_ptr(), out_r.data_ptr(), cap)  # noqa: E731
                    ours()
                    info = ctx.range_pairs_info()
                    row["pairs"], row["written"] = info[0], info[1]
                    if case == "skew":      # the yardstick cannot bound its output: it is given the rows that do not cover R
                        narrow = (hi - lo) < (n // 2 if dtype == torch.int64 else 0.5)
                        y_lo, y_hi = lo[narrow], hi[narrow]
                        row["equal"] = info[1] == cap and bool((out_s[:cap].long() < n).all()) and bool((out_r[:cap].long() < n).all())
                        row["yardstick"] = "the rows that do not cover R: the covering rows alone hold %d pairs" % (8 * n)
                    else:
                        y_lo, y_hi = lo, hi
                        t_s, t_r, t_total = torch_pairs(sorted_r, t_perm, lo, hi)
                        row["equal"] = t_total == info[0] == info[1] and checksum(out_s[:cap], out_r[:cap]) == checksum(t_s, t_r)
                        del t_s, t_r
                    yard = lambda: torch_pairs(sorted_r, t_perm, y_lo, y_hi)  # noqa: E731
                    t_idx, t_sort, t_size, t_ours, t_yard = timed_alternating([index, lambda: torch.sort(r), size, ours, yard], a.reps)
                    row.update(stats("index", t_idx), **stats("sort", t_sort), **stats("size", t_size), **stats("range", t_ours), **stats("torch", t_yard))
                    pairs_rw = info[1]
                row["info_us"] = ctx.range_pairs_info()[2]
                searches = 1 if lo is None else 2
                model = n * width * searches + pairs_rw * 12 + n * (searches + (case == "last")) * steps * 64
                row["model_bytes"] = model
                row["model_GBps"] = round(model / row["range_us"] / 1e3, 1)
                ours_us = row["range_us"] + row.get("size_us", 0.0)
                row["torch_over_ours"] = round(row["torch_us"] / ours_us, 2)
                row["sort_over_index"] = round(row["sort_us"] / row["index_us"], 2)
                print(json.dumps(row), flush=True)
                rows.append(row)
                del r, lo, hi, perm, keys, sorted_r, t_perm
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
