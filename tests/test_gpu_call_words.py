"""The counter words behind every *_info of the calls that need no table, on ONE context without a reserve, through ctypes ->
C ABI on an MI355X: hj_gather_dev, hj_gather2_dev, hj_pairs_verify_dev, hj_pairs_verify2_dev (the two share hj_verify_info),
hj_pairs_where_dev, hj_pairs_asof_dev, hj_pairs_agg_dev, hj_mark_rows_dev, hj_key_groups_dev, hj_sort_rows_dev and
hj_window_rows_dev. test_gpu_call_records.py follows five records through builds and reserves; this file asks whether the
words of one kind can reach another's.

Every call takes N = 300 pairs or rows: more than one wavefront, less than one workgroup of 1024 pairs, no multiple of 64.
The inputs of a round (plan) are chosen so that every word a call counts is non-zero and differs from every other call's:
other numbers of HJ_NO_ROW and out-of-range entries per kind, capacities below what the call finds, and hj_gather2_dev with
HJ_GATHER_MAX_COLS variable-length columns of different total bytes, so that all ten of its words are written.

    1. round 0: the eleven calls one behind the other, then every *_info
    2. round 1: the eleven calls in reverse order on other inputs
    3. around each single call of round 1: exactly that kind's info changed (time words apart), into what the round expects

The expected words come from the host twins (hj_key_groups_host, hj_sort_rows_host, hj_window_rows_host) and the numpy models
of tests/*_common.py; plan() needs no device. What hj_key_groups_info reports of its table's probing (probe steps, word
collisions) depends on the order in which the rows arrive: those two words are held to be non-zero, and to stay as they are
while other kinds are called. Its failure word is 0 by contract. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

import agg_common as ac
import asof_common as asc
import gather_common as gth
import groups_common as gc
import sort_common as sc
import where_common as wc
import window_common as wn
from gpu_harness import Device, plane_bits, plane_words

pytestmark = pytest.mark.gpu

N = 300
S_ROWS, R_ROWS, BASE = 211, 157, 40          # the two relations of the pair lists; S's rows start at BASE
NO_ROW, U32, U64 = 0xFFFFFFFF, np.uint32, np.uint64
KINDS = ("gather", "gather2", "verify", "verify2", "where", "asof", "pairs_agg", "mark_rows", "key_groups", "sort_rows", "window_rows")
INFO_OF = {"verify2": "verify"}              # the info that reports the kind, where it does not carry its name
TIME_WORD = {"window_rows": 3}                    # hj_window_rows_info has its time in word 3, every other info in word 2


def with_holes(rng, m, nulls, stray, beyond):
    """m with `nulls` entries HJ_NO_ROW and `stray` entries at or behind `beyond`, at random places"""
    at = rng.permutation(m.size)[:nulls + stray]
    m[at[:nulls]] = NO_ROW
    m[at[nulls:]] = beyond + rng.integers(0, 1000, stray).astype(U32)
    return m


def pair_maps(rng, k, v):
    """the two maps of a pair list: kind k of round v drops 2 * k + 9 * v + 3 pairs as HJ_NO_ROW and as many + 1 as out of range"""
    nulls = 2 * k + 9 * v + 3
    map_s = with_holes(rng, (BASE + rng.integers(0, S_ROWS, N)).astype(U32), nulls, nulls // 2, BASE + S_ROWS)
    map_r = with_holes(rng, rng.integers(0, R_ROWS, N).astype(U32), 0, nulls + 1 - nulls // 2, R_ROWS)
    return map_s, map_r


def plan(v):
    """round v: per kind its inputs on the host and the words its info must hold behind the call, the time word taken out"""
    p = {}
    for k, kind in enumerate(KINDS):
        rng = np.random.default_rng([0xCA11, k, v])
        if kind == "gather":
            m = with_holes(rng, rng.integers(0, R_ROWS, N).astype(U32), 5 + 4 * v, 7 + 5 * v, R_ROWS)
            p[kind] = dict(map=m, src=rng.integers(0, 1 << 62, R_ROWS).astype(U64),
                           want=(N, int((m == NO_ROW).sum()), int(((m != NO_ROW) & (m >= R_ROWS)).sum())))
        elif kind == "gather2":
            m = with_holes(rng, rng.integers(0, R_ROWS, N).astype(U32), 14 + 4 * v, 16 + 4 * v, R_ROWS)
            i, null, oor, ok = gth.rows_of(m, 0, R_ROWS)
            cols = [gth.strings(rng, rng.integers(1, 3 + c + 4 * v, R_ROWS), lead=c % 3) for c in range(_lib.HJ_GATHER_MAX_COLS)]
            totals = tuple(int((c["offsets"][i[ok] + 1] - c["offsets"][i[ok]]).sum()) for c in cols)
            p[kind] = dict(map=m, cols=cols, want=(N, int(null.sum()), int(oor.sum())) + totals)
        elif kind in ("verify", "verify2", "where", "asof"):
            map_s, map_r = pair_maps(rng, k, v)
            dtype, op, values = {"verify": (U64, "==", 3), "verify2": (U32, "==", 4), "where": (np.int32, "<", 50),
                                 "asof": (np.float64, ">=", 9)}[kind]
            term = wc.term_of(rng.integers(0, values, S_ROWS).astype(dtype), op, rng.integers(0, values, R_ROWS).astype(dtype))
            cap = 11 + 2 * k + v
            model = (asc.model_call(map_s, map_r, BASE, S_ROWS, R_ROWS, term, cap) if kind == "asof" else
                     wc.model_call(map_s, map_r, BASE, S_ROWS, R_ROWS, [term], cap))
            kept, written, _, dropped = model["info"]
            assert kept > cap
            p[kind] = dict(map_s=map_s, map_r=map_r, term=term, cap=cap, want=(kept, written, dropped))
        elif kind == "pairs_agg":
            map_g, map_v = pair_maps(rng, k, v)
            g, val = (map_g.astype(np.int64) - BASE) % (1 << 32), map_v.astype(np.int64)
            ok = (map_g != NO_ROW) & (map_v != NO_ROW) & (g < S_ROWS) & (val < R_ROWS)
            p[kind] = dict(map_g=map_g, map_v=map_v, src=rng.integers(0, 1 << 30, R_ROWS).astype(U64),
                           want=(N, int(ok.sum()), int((~ok).sum())))
        elif kind == "mark_rows":
            words = plane_words(rng.random(N) < 0.3 + 0.3 * v)
            cap = 41 + v
            produced = int(plane_bits(words, N).sum())
            assert produced > cap
            p[kind] = dict(words=words, cap=cap, want=(produced, cap, N))
        elif kind == "key_groups":
            values, valid = rng.integers(0, 70 + 40 * v, N).astype(U32), np.ones(N, dtype=bool)
            valid[rng.permutation(N)[:23 + 15 * v]] = False
            cap = 31 + v
            host = hj.key_groups_host([hj.KeyColumn(values, valid)], nulls="drop", key_mask=0xF, capacity=cap)
            model = gc.model_groups([int(x) if ok else None for x, ok in zip(values, valid)], cap)
            gc.same(host, model, (kind, v))
            assert model["n_groups"] > cap
            p[kind] = dict(values=values, valid=valid, cap=cap, want=(model["n_groups"], cap, model["null_rows"]))
        elif kind == "sort_rows":
            cols = [sc.Col(rng.integers(-99, 99, N).astype(np.int16), rng.random(N) < 0.9, desc=bool(v))]
            cols += [sc.Col(rng.integers(0, 9, N).astype(np.uint8))] * v           # round 1: another number of passes
            info = sc.host_perm(cols)[1]
            p[kind] = dict(cols=cols, want=tuple(info[:2] + info[3:]))
        else:
            case = wn.build(N, holes=19 + 12 * v, seed=5 * v, extra_rows=7, peers=("runs", "distinct")[v])
            info = wn.host_call(case)[1]
            wn.check_info(info, case, wn.model(case)[1], (kind, v))
            p[kind] = dict(case=case, want=tuple(info[:3] + info[4:]))
    return p


def counted(p):
    """the words of a round that a call counts on the device and the host can foretell, by name"""
    words = {}
    for kind in KINDS:
        w = p[kind]["want"]
        mine = {"gather": w[1:], "gather2": w[1:], "pairs_agg": w[1:], "mark_rows": w[:1], "key_groups": (w[0], w[2]), "sort_rows": (),
                "window_rows": w[1:4]}.get(kind, (w[0], w[2]))               # the four pair filters: kept, dropped
        words.update({(kind, i): x for i, x in enumerate(mine)})
    return words


def test_the_plans_count_nothing_twice():
    """every counted word of either round is non-zero, and no two calls of the two rounds count the same number"""
    words = {(v,) + key: x for v in (0, 1) for key, x in counted(plan(v)).items()}
    assert len(words) == 2 * (2 + 10 + 4 * 2 + 2 + 1 + 2 + 3)
    assert all(words.values()), words
    assert len(set(words.values())) == len(words), sorted(words.items(), key=lambda kv: kv[1])


def call(ctx, dev, kind, a):
    """the one call of `kind` on the inputs a of its plan"""
    def outs(cap):
        return dev.alloc(4 * cap), dev.alloc(4 * cap)

    def term(t):
        return (dev.put(t[0]), dev.put(t[2]), t[0].dtype.itemsize, wc.TYPE_OF[t[0].dtype.kind], _lib.CMP_OPS[t[1]], 0, 0)

    if kind == "gather":
        ctx.gather(dev.put(a["map"]), N, R_ROWS, [(dev.put(a["src"]), dev.alloc(8 * N), 8, 0)])
    elif kind == "gather2":
        descs = []
        for c, total in zip(a["cols"], a["want"][3:]):
            descs.append(dict(src=dev.put(c["data"]), src_offsets=dev.put(c["offsets"].astype(U32)), width=0, dst=dev.alloc(total),
                              dst_offsets=dev.alloc(4 * (N + 1)), dst_capacity=total))
        ctx.gather2(dev.put(a["map"]), N, R_ROWS, descs)
    elif kind in ("verify", "verify2"):
        t = a["term"]
        col = (dev.put(t[0]), dev.put(t[2]), t[0].dtype.itemsize)
        (ctx.pairs_verify if kind == "verify" else ctx.pairs_verify2)(dev.put(a["map_s"]), dev.put(a["map_r"]), N, BASE, S_ROWS, R_ROWS, [col],
                                                                     *outs(a["cap"]), a["cap"])
    elif kind == "where":
        ctx.pairs_where(dev.put(a["map_s"]), dev.put(a["map_r"]), N, BASE, S_ROWS, R_ROWS, [term(a["term"])], *outs(a["cap"]), a["cap"])
    elif kind == "asof":
        ctx.pairs_asof(dev.put(a["map_s"]), dev.put(a["map_r"]), N, BASE, S_ROWS, R_ROWS, term(a["term"]), dev.alloc(8 * S_ROWS),
                       dev.alloc(4 * S_ROWS), *outs(a["cap"]), a["cap"])
    elif kind == "pairs_agg":
        acc, count = dev.put(np.zeros(S_ROWS, dtype=U64)), dev.put(np.zeros(S_ROWS, dtype=U64))
        ctx.pairs_agg(dev.put(a["map_g"]), dev.put(a["map_v"]), N, BASE, S_ROWS, 0, R_ROWS, [(dev.put(a["src"]), 0, acc, ac.SUM, 8, 0)], count)
    elif kind == "mark_rows":
        ctx.mark_rows(dev.put(a["words"]), N, BASE, _lib.HJ_R_MATCHED, dev.alloc(4 * a["cap"]), a["cap"])
    elif kind == "key_groups":
        col = (dev.put(a["values"]), 0, 4, 0, 0, dev.put(plane_words(a["valid"])), 0, 0)
        ctx.key_groups([col], hj.HJ_KEY_SIDE_S, N, dev.alloc(4 * N), dev.alloc(4 * N), dev.alloc(4 * a["cap"]), a["cap"], 0xF)
    elif kind == "sort_rows":
        desc = [(dev.put(c.values), dev.put(c.plane()) if c.valid is not None else 0, c.width, c.type, c.flags) for c in a["cols"]]
        ctx.sort_rows(desc, N, dev.alloc(4 * N))
    else:
        case = a["case"]
        order = [(dev.put(c.values), dev.put(c.plane()) if c.valid is not None else 0, c.width, c.type, c.flags) for c in case.order]
        funcs = [(f.op, dev.alloc(4 * case.n_rows), 0, 0, f.width, f.flags, f.offset) for f in case.funcs]
        ctx.window_rows(dev.put(case.perm), case.n_pos, case.n_rows, dev.put(case.part), order, funcs)


def infos(ctx):
    """every *_info of the eleven kinds: {its name: (all its words, its words without the time)}"""
    out = {}
    for kind in KINDS:
        if kind in INFO_OF:
            continue
        words = getattr(ctx, kind + "_info")()
        words = tuple(words.values()) if isinstance(words, dict) else tuple(words)
        t = TIME_WORD.get(kind, 2)
        out[kind] = words[:t] + words[t + 1:]
    return out


def check(kind, got, want, tag):
    """the info of `kind` without its time against the plan's words"""
    if kind == "key_groups":
        groups, written, nulls, slots, steps, collisions, failure = got
        assert (groups, written, nulls) == want and failure == 0, (tag, kind, got, want)
        assert slots >= 2 * N and steps > 0 and collisions > 0, (tag, kind, got)
    else:
        assert got == want, (tag, kind, got, want)


def test_every_kind_keeps_its_own_words():
    plans = plan(0), plan(1)
    with hj.HashJoinContext(0) as ctx, Device(ctx) as dev:
        blank = infos(ctx)
        assert all(not any(words) for words in blank.values()), blank
        # 1. one call of every kind, then every info
        for kind in KINDS:
            call(ctx, dev, kind, plans[0][kind])
            if kind in INFO_OF:
                continue
            check(kind, infos(ctx)[kind], plans[0][kind]["want"], "behind its own call")
        first = infos(ctx)
        print("round 0", first)
        for kind, got in first.items():
            by = "verify2" if kind == "verify" else kind                   # the last call the info reports
            check(kind, got, plans[0][by]["want"], "behind all eleven")
        # 2. and 3. the other inputs in reverse order: a call changes the info of its kind and no other
        before = first
        for kind in reversed(KINDS):
            call(ctx, dev, kind, plans[1][kind])
            after, name = infos(ctx), INFO_OF.get(kind, kind)
            print("round 1", kind, after[name])
            for other in after:
                if other != name:
                    assert after[other] == before[other], (kind, "changed the info of", other, before[other], after[other])
            assert after[name] != before[name], (kind, "left its info as it was", after[name])
            check(name, after[name], plans[1][kind]["want"], "round 1")
            before = after
