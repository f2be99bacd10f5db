#!/usr/bin/env python3
"""Times hj_gather_dev against torch.index_select on the same device, the same maps and the same columns: development tool.

    python tools/gather_bench.py [--log2n 27] [--reps 7] [--out FILE] [--only plain|columns]

One context created with hj_create_on_stream on torch's current stream; every buffer is a torch tensor whose data_ptr()
goes to the C ABI. |R| = |S| = n = 2^log2n output rows from an n-row source.
Maps, all written by the engine on the device and never copied to the host:
  ascending   hj_r_rows_dev(HJ_R_UNMATCHED) after a build that no probe has marked: every R row, ascending
  s_sorted    the S plane of hj_probe_join_dev(INNER) over a sorted S
  r_random    the R plane of the same probe; R is a random permutation (generate_relation "pk"), so the plane is one too
NULL share 0.5: the same map with every second entry replaced by HJ_NO_ROW (index_select cannot take it: no baseline).
Columns: 1 and 4 columns of 4, 8 and 16 bytes (index_select: int32, int64, complex128; one call per column).
Per configuration one JSON line: the median, minimum and maximum over `reps` launches after one warm-up launch, each
launch between two events on the stream, for the gather (gather_us*) and for index_select (select_us*); gather_GBps =
(4 B of map + 2 x width per column: read and written) x n / the median, the algorithmic bytes, not the lines fetched; ratio
= gather median / index_select median; equal = the two outputs are the same bytes (checked once per configuration).

--only columns (or no --only: both parts) adds the rows of hj_gather2_dev, "kind" telling them apart, over the same maps:
  plain2      one and four plain 8-byte columns through hj_gather2_dev against hj_gather_dev on the same map (it launches
              the same kernels): within_spread = its median lies between the minimum and the maximum of hj_gather_dev's
  nullable    one 8-byte column with a source validity plane (30 % NULLs) and a dstValid plane
  strings     one string column, elements of 8 to 24 bytes at n rows, and of 256 bytes at 2^23 rows from a 2^23-row source
              (32-bit offsets bound a column to 2^32 - 1 bytes; the map is the first 2^23 entries of the shape, modulo
              2^23): copy_us = one call with dst at its exact capacity, sizing_us = the call with dstCapacity 0 that a
              caller without the total makes first. Baseline, what a user would write in torch today: index_select of the
              lengths, cumsum, and a byte-level index_select through repeat_interleave (the map as int64 made outside the
              timing); equal = torch.equal on the bytes and the offsets. model_GBps = the byte model of
              profiles/gather_columns.md over copy_us."""
import argparse
import json
import os
import statistics
import sys

import torch  # first: it ships its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib  # noqa: E402

SELECT_DTYPE = {4: torch.int32, 8: torch.int64, 16: torch.complex128}


def timed(fn, reps):
    """-> microseconds of reps launches of fn after one warm-up launch, each between two events on the current stream"""
    out = []
    for k in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if k:
            out.append(t0.elapsed_time(t1) * 1000.0)
    return out


def stats(prefix, us):
    return {prefix + "_us": round(statistics.median(us), 1), prefix + "_us_min": round(min(us), 1), prefix + "_us_max": round(max(us), 1)}


def torch_strings(data, off, m64):
    """the torch composition: -> (bytes, offsets behind the first)"""
    lens = off[1:] - off[:-1]
    taken = lens.index_select(0, m64)
    ends = torch.cumsum(taken, 0)
    total = int(ends[-1])
    delta = off.index_select(0, m64) - (ends - taken)
    idx = torch.repeat_interleave(delta, taken, output_size=total) + torch.arange(total, device=data.device)
    return data.index_select(0, idx), ends


def columns_rows(c, maps, n, a, emit, dev, g, srcs, dsts):
    """the rows of hj_gather2_dev (see the head of this file)"""
    words = (n + 31) // 32
    src_valid = (torch.rand(n, device=dev, generator=g) >= 0.3)
    bits = src_valid.view(-1, 32).to(torch.int64) << torch.arange(32, device=dev)
    d_src_valid = bits.sum(1).to(torch.int32)                      # bit i & 31 of word i >> 5 (the cast wraps: the bits stay)
    d_dst_valid = torch.empty(words, dtype=torch.int32, device=dev)
    for name, m in maps.items():
        base = {"map": name, "log2n": a.log2n, "reps": a.reps}
        for n_cols in (1, 4):
            cols = [(srcs[k].data_ptr(), dsts[k].data_ptr(), 8, 0) for k in range(n_cols)]
            cols2 = [dict(src=s, dst=d, width=w) for s, d, w, _ in cols]
            one = timed(lambda: c.gather(m.data_ptr(), n, n, cols), a.reps)
            two = timed(lambda: c.gather2(m.data_ptr(), n, n, cols2), a.reps)
            row = dict(base, kind="plain2", width=8, cols=n_cols)
            row.update(stats("gather", one))
            row.update(stats("gather2", two))
            row["within_spread"] = bool(min(one) <= statistics.median(two) <= max(one))
            emit(row)
        col = dict(src=srcs[0].data_ptr(), dst=dsts[0].data_ptr(), width=8, src_valid=d_src_valid.data_ptr(), dst_valid=d_dst_valid.data_ptr())
        us = timed(lambda: c.gather2(m.data_ptr(), n, n, [col]), a.reps)
        row = dict(base, kind="nullable", width=8, cols=1, null_share=0.3)
        row.update(stats("gather2", us))
        row["gather2_GBps"] = round((4.0 + 4.0 + 16.0 * 0.7 + 8.0 * 0.3) * n / statistics.median(us) / 1e3, 1)
        emit(row)
    for lo, hi, rows in ((8, 24, n), (256, 256, min(n, 1 << 23))):
        lens = torch.randint(lo, hi + 1, (rows,), dtype=torch.int64, device=dev, generator=g)
        off = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(lens, 0)
        assert int(off[-1]) <= 0xFFFFFFFF
        data = torch.randint(0, 256, (int(off[-1]) + 3,), dtype=torch.uint8, device=dev, generator=g)
        off32 = off.to(torch.int32)                                  # wraps above 2^31: the 32 bits are the offsets'
        d_off = torch.empty(rows + 1, dtype=torch.int32, device=dev)
        for name, whole in maps.items():
            m = whole if rows == n else (whole[:rows] & (rows - 1)).contiguous()
            m64 = m.to(torch.int64)
            col = dict(src=data.data_ptr(), width=0, src_offsets=off32.data_ptr(), dst_offsets=d_off.data_ptr())
            sizing = timed(lambda: c.gather2(m.data_ptr(), rows, rows, [col]), a.reps)
            total = c.gather2_info()[4]
            assert total <= 0xFFFFFFFF, total
            dst = torch.empty(total + 16, dtype=torch.uint8, device=dev)
            full = dict(col, dst=dst.data_ptr(), dst_capacity=total)
            us = timed(lambda: c.gather2(m.data_ptr(), rows, rows, [full]), a.reps)
            keep = {}

            def select():
                keep["out"] = torch_strings(data, off, m64)

            sel = timed(select, a.reps)
            want, ends = keep["out"]
            med = statistics.median(us)
            row = dict(base, map=name, kind="strings", bytes_lo=lo, bytes_hi=hi, rows=rows, total_bytes=total)
            row.update(stats("copy", us))
            row.update(stats("sizing", sizing))
            row.update(stats("select", sel))
            row["ratio"] = round(med / statistics.median(sel), 3)
            row["model_GBps"] = round((40.0 * rows + 2.0 * total) / med / 1e3, 1)
            row["equal"] = bool(want.numel() == total and torch.equal(dst[:total], want)
                                and torch.equal(d_off[1:].to(torch.int64) & 0xFFFFFFFF, ends))
            emit(row)
            del dst, want, ends, keep
        del data, off, off32, d_off, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", choices=("plain", "columns"), default="")
    a = ap.parse_args()
    n = 1 << a.log2n
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    with hj.HashJoinContext(0, stream=torch.cuda.current_stream().cuda_stream) as c:
        # ---- the maps, from the engine ----
        R = torch.from_numpy(hj.generate_relation("pk", n).view("int64")).to(dev)
        S = torch.arange(1, n + 1, dtype=torch.int64, device=dev)
        maps = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("ascending", "s_sorted", "r_random")}
        c.reserve("htm", n, n, keepRowIds=True, trackRMatches=True)
        c.build(R.data_ptr(), n)
        c.r_rows(_lib.HJ_R_UNMATCHED, maps["ascending"].data_ptr(), n)
        assert c.r_rows_info()[:2] == (n, n)
        c.probe_pairs(S.data_ptr(), n, maps["s_sorted"].data_ptr(), maps["r_random"].data_ptr(), n)
        assert c.pairs_info()[:2] == (n, n)
        c.fetch()
        del R, S
        # ---- the columns: four sources and four outputs of 16 bytes an element, narrower columns are their front ----
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        srcs = [torch.randint(0, 1 << 62, (2 * n,), dtype=torch.int64, device=dev, generator=g) for _ in range(4)]
        dsts = [torch.empty(2 * n, dtype=torch.int64, device=dev) for _ in range(4)]
        check = torch.empty(2 * n, dtype=torch.int64, device=dev)
        if a.only != "plain":
            columns_rows(c, maps, n, a, emit, dev, g, srcs, dsts)
        for name, base in maps.items() if a.only != "columns" else ():
            for null_share in (0.0, 0.5):
                m = base
                if null_share:
                    m = base.clone()
                    m[::2] = -1                                 # HJ_NO_ROW
                for width in (4, 8, 16):
                    for n_cols in (1, 4):
                        cols = [(srcs[k].data_ptr(), dsts[k].data_ptr(), width, 0) for k in range(n_cols)]
                        us = timed(lambda: c.gather(m.data_ptr(), n, n, cols), a.reps)
                        info = c.gather_info()
                        assert info[0] == n and info[3] == 0 and info[1] == (n // 2 if null_share else 0), info
                        med = statistics.median(us)
                        row = {"map": name, "null_share": null_share, "width": width, "cols": n_cols, "log2n": a.log2n, "reps": a.reps}
                        row.update(stats("gather", us))
                        row["gather_GBps"] = round((4.0 + 2.0 * width * n_cols) * n / med / 1e3, 1)
                        row["last_gather_info_us"] = info[2]
                        if not null_share:
                            dt = SELECT_DTYPE[width]
                            words = n * width // 8
                            views = [(srcs[k][:words].view(dt), check[:words].view(dt) if k == 0 else dsts[k][:words].view(dt))
                                     for k in range(n_cols)]
                            idx = m                             # int32: the uint32 map as it lies, its entries are below 2^31

                            def select():
                                for src, dst in views:
                                    torch.index_select(src, 0, idx, out=dst)

                            sel = timed(select, a.reps)
                            row.update(stats("select", sel))
                            row["ratio"] = round(med / statistics.median(sel), 3)
                            c.gather(m.data_ptr(), n, n, cols[:1])  # column 0 again: index_select wrote the others' outputs
                            c.synchronize()
                            row["equal"] = bool(torch.equal(dsts[0][:words], check[:words]))
                        emit(row)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
