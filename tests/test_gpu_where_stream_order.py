"""hj_pairs_where_dev behind a delayed caller's stream (hj_create_on_stream), on an MI355X, with the harness of
stream_order.py as it stands: when the call is enqueued the maps still hold HJ_NO_ROW and the term's columns decoys that keep
nothing; the real inputs arrive behind the delay on the same stream and a torch copy on that stream takes the results. A
call that left the stream's order kept nothing. The expected result is where_common's numpy model. Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import stream_order as so
from gpu_harness import fl, packed, plane_words  # noqa: F401
import where_common as wc

pytestmark = pytest.mark.gpu

U32 = np.uint32
N_S, N_R, N_PAIRS, BASE = 3001, 2003, 9001, 500
SLACK = 64                       # map words behind the exact count: they keep the HJ_NO_ROW prefill


def vp(p):
    return C.c_void_p(p) if p else None


def test_pairs_where_behind_a_delay(fl):
    rng = np.random.default_rng(5)
    s, r = rng.integers(-50, 50, N_S).astype(np.int32), rng.integers(-50, 50, N_R).astype(np.int32)
    s_valid = rng.random(N_S) < 0.9
    map_s, map_r = (BASE + rng.integers(0, N_S, N_PAIRS)).astype(U32), rng.integers(0, N_R, N_PAIRS).astype(U32)
    map_s[::37] = so.NO_ROW
    want = wc.model_call(map_s, map_r, BASE, N_S, N_R, [wc.term_of(s, "<", r, s_valid, None)])
    n_kept = want["info"][0]
    assert 1000 < n_kept < N_PAIRS - 1000
    sw, rw = -(-N_S // 32), -(-N_R // 32)
    assert lib._hj_signatures["hj_pairs_where_dev"] and so.contract()["hj_pairs_where_dev"][0] == "asynchronous"
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        st = so.Stage(fl.stream)
        # decoys: maps of HJ_NO_ROW, an S column above everything in R, an all-NULL validity -- three times "keeps nothing"
        bMS = st.buf(np.full(N_PAIRS, so.NO_ROW, dtype=U32), real=map_s, warm=np.roll(map_s, 1))
        bMR = st.buf(np.full(N_PAIRS, so.NO_ROW, dtype=U32), real=map_r, warm=np.roll(map_r, 2))
        bS = st.buf(np.full(N_S, np.iinfo(np.int32).max, dtype=np.int32), real=s, warm=s[::-1].copy())
        bR = st.buf(np.full(N_R, np.iinfo(np.int32).min, dtype=np.int32), real=r, warm=r[::-1].copy())
        bV = st.buf(np.zeros(sw, dtype=U32), real=plane_words(s_valid), warm=plane_words(~s_valid))
        oS, oR = st.out(n_kept + SLACK, U32, so.NO_ROW), st.out(n_kept + SLACK, U32, so.NO_ROW)
        pS, pR = st.out(sw, U32, 0), st.out(rw, U32, 0)              # the planes, cleared by the caller

        def seq(which):
            arr = (_lib.hj_where_term * 1)()
            arr[0].s, arr[0].r, arr[0].sValid, arr[0].rValid = bS.ptr, bR.ptr, bV.ptr, None
            arr[0].width, arr[0].type, arr[0].op = 4, _lib.HJ_VAL_INT, _lib.HJ_CMP_LT
            rc = lib.hj_pairs_where_dev(ctx._h, vp(bMS.ptr), vp(bMR.ptr), N_PAIRS, BASE, N_S, N_R, arr, 1, vp(oS.ptr), vp(oR.ptr),
                                        n_kept + SLACK, vp(pS.ptr), vp(pR.ptr))
            C.memset(arr, 0, C.sizeof(arr))                          # the descriptor was read before the call returned
            assert rc == _lib.HJ_OK, lib.hj_last_error(ctx._h)

        so.run_delayed([st], seq, True, f"where.{fl.name}")          # asserts pending() after the enqueue: the call did not block
        st.check_inputs_intact()
        info = ctx.where_info()
    assert (info[0], info[1], info[3]) == (n_kept, n_kept, want["info"][3]), (info, want["info"])
    got_s, got_r = st.result(oS, U32, "kept S"), st.result(oR, U32, "kept R")
    assert (got_s[n_kept:] == so.NO_ROW).all() and (got_r[n_kept:] == so.NO_ROW).all(), "a word behind the last pair was written"
    assert np.array_equal(packed(got_s[:n_kept], got_r[:n_kept]), want["kept"])
    assert np.array_equal(st.result(pS, U32, "S marks"), want["s_marks"]) and np.array_equal(st.result(pR, U32, "R marks"), want["r_marks"])
