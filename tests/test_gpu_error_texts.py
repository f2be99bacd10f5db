"""The exact hj_last_error text of every rejected call whose message names its entry point: the materialising probes
under both of their names, the match-marks calls, the key-column checks of hj_key_hash_dev and hj_pairs_verify_dev, and the
gather's pointer checks. Every case is an argument or call-order error that returns before anything is enqueued; the
builds in here only bring a context into the state a later check needs. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from gpu_harness import Device, ctx  # noqa: F401


pytestmark = pytest.mark.gpu

INVALID, STATE = _lib.HJ_ERR_INVALID, _lib.HJ_ERR_STATE
N = 1024
BIG = 1 << 16                                    # a marks plane of 8 KiB: more than the 128 bytes reserved for N rows
lib = hj.lib


def refused(ctx, rc, status, text):
    assert (rc, lib.hj_last_error(ctx._h).decode()) == (status, text)


def p(d):
    return d or None


def probe_join(ctx, name, kind, dS, n, base, d_s, d_r, cap):
    """one of the four materialising entry points by name; the *_pairs_dev ones take no kind"""
    if name.endswith("_join_dev"):
        return getattr(lib, name)(ctx._h, kind, p(dS), n, base, p(d_s), p(d_r), cap)
    return getattr(lib, name)(ctx._h, p(dS), n, base, p(d_s), p(d_r), cap)


@pytest.fixture(scope="module")
def mem(ctx):
    """R = S = the keys 1 .. 1024 on the device, and two output planes"""
    with Device(ctx) as dev:
        d = dev.put(np.arange(1, N + 1, dtype=np.uint64))
        yield {"R": d, "S": d, "s": dev.alloc(4 * N), "r": dev.alloc(4 * N), "big": dev.alloc(8 * (BIG + 2))}


TABLE_NAMES = ("hj_probe_join_dev", "hj_probe_pairs_dev")
PRJ_NAMES = ("hj_prj_probe_join_dev", "hj_prj_probe_pairs_dev")


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_table_probe(ctx, mem, name):
    R, S, s, r = mem["R"], mem["S"], mem["s"], mem["r"]
    ctx.reserve("prj", N, N, radixBits=4, keepRowIds=True)
    refused(ctx, probe_join(ctx, name, 0, S, N, 0, s, r, N), STATE, name + ": a PRJ context keeps no row ids")
    with hj.HashJoinContext(0) as fresh:
        fresh.reserve("atomic", N, N, keepRowIds=True)
        refused(fresh, probe_join(fresh, name, 0, S, N, 0, s, r, N), STATE, name + ": no table (call hj_build_dev first)")
    ctx.reserve("atomic", N, N, buildVariant=1)
    ctx.build(R, N)
    refused(ctx, probe_join(ctx, name, 0, S, N, 0, s, r, N), STATE,
            name + ": open-addressing context reserved without HJ_FLAG_KEEP_ROW_IDS")
    ctx.reserve("atomic", N, N, buildVariant=1, probeLength=9, keepRowIds=True)
    ctx.build(R, N)
    refused(ctx, probe_join(ctx, name, 0, S, N, 0, s, r, N), INVALID, name + ": probeLength above 8")
    ctx.reserve("atomic", N, N, buildVariant=1, keepRowIds=True)
    ctx.build(R, N)
    if name == "hj_probe_join_dev":
        refused(ctx, probe_join(ctx, name, 4, S, N, 0, s, r, N), INVALID, name + ": kind must be an hj_join_kind")
        refused(ctx, probe_join(ctx, name, 1, S, N, 0, s, 0, N), INVALID, name + ": output pointer NULL with capacity > 0")
    refused(ctx, probe_join(ctx, name, 0, S, N, 0, 0, r, N), INVALID, name + ": output pointer NULL with capacity > 0")
    refused(ctx, probe_join(ctx, name, 0, S, N, 0, s, 0, N), INVALID, name + ": output pointer NULL with capacity > 0")
    refused(ctx, probe_join(ctx, name, 0, S, N, 1 << 32, s, r, N), INVALID, name + ": S row range exceeds 2^32 - 1")
    refused(ctx, probe_join(ctx, name, 0, S, N, (1 << 32) - N, s, r, N), INVALID, name + ": S row range exceeds 2^32 - 1")
    assert probe_join(ctx, name, 0, S, N, 0, s, r, N) == _lib.HJ_OK           # and the context still probes
    assert ctx.pairs_info()[:2] == (N, N)


@pytest.mark.parametrize("name", PRJ_NAMES)
def test_radix_probe(ctx, mem, name):
    R, S, s, r = mem["R"], mem["S"], mem["s"], mem["r"]
    with hj.HashJoinContext(0) as fresh:
        fresh.reserve("prj", N, N, radixBits=4, keepRowIds=True)
        refused(fresh, probe_join(fresh, name, 0, S, N, 0, s, r, N), STATE, name + ": no resident R (call hj_prj_build_dev first)")
    ctx.reserve("prj", N, N, radixBits=4)
    ctx.prj_build(R, N)
    refused(ctx, probe_join(ctx, name, 0, S, N, 0, s, r, N), STATE, name + ": R was built without HJ_FLAG_KEEP_ROW_IDS")
    ctx.reserve("prj", N, N, radixBits=4, keepRowIds=True)
    ctx.prj_build(R, N)
    refused(ctx, probe_join(ctx, name, 0, S, N + 1, 0, s, r, N), STATE,
            name + ": slice larger than the sSize given to hj_reserve()")
    if name == "hj_prj_probe_join_dev":
        refused(ctx, probe_join(ctx, name, 4, S, N, 0, s, r, N), INVALID, name + ": kind must be an hj_join_kind")
        refused(ctx, probe_join(ctx, name, 1, S, N, 0, s, 0, N), INVALID, name + ": output pointer NULL with capacity > 0")
    refused(ctx, probe_join(ctx, name, 0, S, N, 0, 0, r, N), INVALID, name + ": output pointer NULL with capacity > 0")
    refused(ctx, probe_join(ctx, name, 0, S, N, 0, s, 0, N), INVALID, name + ": output pointer NULL with capacity > 0")
    refused(ctx, probe_join(ctx, name, 0, S, N, 1 << 32, s, r, N), INVALID, name + ": S row range exceeds 2^32 - 1")
    refused(ctx, probe_join(ctx, name, 0, S, N, (1 << 32) - N, s, r, N), INVALID, name + ": S row range exceeds 2^32 - 1")
    assert probe_join(ctx, name, 0, S, N, 0, s, r, N) == _lib.HJ_OK
    assert ctx.pairs_info()[:2] == (N, N)


def marks_calls(ctx):
    out = (_lib.C.c_uint64 * 4)()
    return {"hj_r_marks_clear": lambda: lib.hj_r_marks_clear(ctx._h),
            "hj_r_rows_dev": lambda: lib.hj_r_rows_dev(ctx._h, 0, None, 0),
            "hj_r_rows_info": lambda: lib.hj_r_rows_info(ctx._h, out)}


def test_marks_state(ctx, mem):
    ctx.reserve("atomic", N, N, keepRowIds=True)
    ctx.build(mem["R"], N)
    for name, call in marks_calls(ctx).items():
        refused(ctx, call(), STATE, name + ": context reserved without HJ_FLAG_TRACK_R_MATCHES")
    ctx.reserve("atomic", BIG, N, keepRowIds=True, trackRMatches=True)       # a new plane: the build above is not in it
    for name, call in marks_calls(ctx).items():
        refused(ctx, call(), STATE, name + ": the last build was not hj_build_dev / hj_prj_build_dev (or there was none)")
    with hj.HashJoinContext(0) as fresh:
        fresh.reserve("htm", N, N, trackRMatches=True)
        for name, call in marks_calls(fresh).items():
            refused(fresh, call(), STATE, name + ": the last build was not hj_build_dev / hj_prj_build_dev (or there was none)")


def test_marks_begin(mem):
    """a table (a resident R) large enough for 2^16 rows on a context whose marks plane was reserved for 1024"""
    with hj.HashJoinContext(0) as c:
        c.reserve("atomic", BIG, N, keepRowIds=True)
        c.reserve("atomic", N, N, keepRowIds=True, trackRMatches=True)
        refused(c, lib.hj_build_dev(c._h, mem["big"], BIG, 0), STATE,
                "hj_build_dev: hj_reserve() not called for this rSize (match marks)")
    with hj.HashJoinContext(0) as c:
        c.reserve("prj", BIG, N, radixBits=4, keepRowIds=True)
        c.reserve("prj", N, N, radixBits=4, keepRowIds=True, trackRMatches=True)
        refused(c, lib.hj_prj_build_dev(c._h, mem["big"], BIG), STATE,
                "hj_prj_build_dev: hj_reserve() not called for this rSize (match marks)")


def key_cols(cols):
    arr = (_lib.hj_key_col * max(len(cols), 1))()
    for c, (s, r, width, reserved) in zip(arr, cols):
        c.s, c.r, c.width, c.reserved = p(s), p(r), width, reserved
    return arr


# (columns as (s, r, width, reserved) with "S" / "R" for the device relation, nCols or None for len(columns)) -> the text
KEY_COLS = [
    ([], None, "nCols must be 1 .. HJ_KEY_MAX_COLS"),
    ([("S", "R", 8, 0)] * 5, None, "nCols must be 1 .. HJ_KEY_MAX_COLS"),
    (None, 1, "cols NULL"),
    ([("S", "R", 3, 0)], None, "a width that is not 1, 2, 4, 8 or 16"),
    ([("S", "R", 8, 0), ("S", "R", 0, 0)], None, "a width that is not 1, 2, 4, 8 or 16"),
    ([("S", "R", 8, 1)], None, "hj_key_col.reserved must be 0"),
    ([(0, "R", 8, 0)], None, "an S column that is NULL or not aligned to its width"),
    ([("S+4", "R", 8, 0)], None, "an S column that is NULL or not aligned to its width"),
    ([("S", 0, 8, 0)], None, "an R column that is NULL or not aligned to its width"),
    ([("S", "R+2", 4, 0)], None, "an R column that is NULL or not aligned to its width"),
]


def resolve(cols, mem):
    at = {"S": mem["S"], "R": mem["R"], "S+4": mem["S"] + 4, "R+2": mem["R"] + 2, 0: 0}
    return [(at[s], at[r], w, res) for s, r, w, res in cols]


@pytest.mark.parametrize("cols,n_cols,what", KEY_COLS)
def test_key_columns(ctx, mem, cols, n_cols, what):
    arr = None if cols is None else key_cols(resolve(cols, mem))
    n = len(cols) if n_cols is None else n_cols
    out = mem["big"]
    if "R column" not in what:
        refused(ctx, lib.hj_key_hash_dev(ctx._h, arr, n, _lib.HJ_KEY_SIDE_S, N, 0, out), INVALID, "hj_key_hash_dev: " + what)
    if "S column" not in what:
        refused(ctx, lib.hj_key_hash_dev(ctx._h, arr, n, _lib.HJ_KEY_SIDE_R, N, 0, out), INVALID, "hj_key_hash_dev: " + what)
    refused(ctx, lib.hj_pairs_verify_dev(ctx._h, mem["s"], mem["r"], N, 0, N, N, arr, n, mem["s"], mem["r"], 0, None, None), INVALID,
            "hj_pairs_verify_dev: " + what)


def test_key_hash_arguments(ctx, mem):
    arr = key_cols([(mem["S"], mem["R"], 8, 0)])
    refused(ctx, lib.hj_key_hash_dev(ctx._h, arr, 1, 2, N, 0, mem["big"]), INVALID,
            "hj_key_hash_dev: side must be HJ_KEY_SIDE_S or HJ_KEY_SIDE_R")
    refused(ctx, lib.hj_key_hash_dev(ctx._h, arr, 1, 0, 1 << 32, 0, mem["big"]), INVALID, "hj_key_hash_dev: nRows above 2^32 - 1")
    refused(ctx, lib.hj_key_hash_dev(ctx._h, arr, 1, 0, N, 0, None), INVALID, "hj_key_hash_dev: output pointer NULL with nRows > 0")


def test_gather_pointers(ctx, mem):
    def gather(src, dst, width, src_rows=N):
        arr = (_lib.hj_gather_col * 1)()
        arr[0].src, arr[0].dst, arr[0].width = p(src), p(dst), width
        return lib.hj_gather_dev(ctx._h, mem["s"], N, 0, src_rows, arr, 1, None)

    dst_text = "hj_gather_dev: a dst that is NULL or not aligned to its width"
    src_text = "hj_gather_dev: a src that is NULL or not aligned to its width"
    refused(ctx, gather(mem["R"], 0, 8), INVALID, dst_text)
    refused(ctx, gather(0, 0, 8, src_rows=0), INVALID, dst_text)
    refused(ctx, gather(0, mem["big"], 8), INVALID, src_text)
    for w in (2, 4, 8, 16):
        refused(ctx, gather(mem["R"], mem["big"] + w // 2, w), INVALID, dst_text)
        refused(ctx, gather(mem["R"] + 1, mem["big"], w), INVALID, src_text)
