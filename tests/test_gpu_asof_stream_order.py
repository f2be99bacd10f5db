"""hj_pairs_asof_dev behind a delayed caller's stream (hj_create_on_stream), on an MI355X, with the harness of
stream_order.py as it stands: when the call is enqueued the maps still hold HJ_NO_ROW and the term's columns decoys that make
no pair eligible; the real inputs arrive behind the delay on the same stream and a torch copy on that stream takes the
results. The two best planes travel with the inputs: behind the delay they are loaded with words that defeat every later
pass -- a bestVal no key exceeds, a bestRow of 0 no row undercuts -- so the call's own initialisations must run behind that
load, on the stream, and all three kernels behind them. The expected result is asof_common's model. Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

from gpu_harness import fl, packed, plane_words  # noqa: F401
import asof_common as ac
import stream_order as so
import where_common as wc

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
N_S, N_R, N_PAIRS, BASE = 3001, 2003, 9001, 500
SLACK = 64                       # output words behind the exact count: they keep the HJ_NO_ROW prefill


def vp(p):
    return C.c_void_p(p) if p else None


def test_pairs_asof_behind_a_delay(fl):
    rng = np.random.default_rng(6)
    s, r = rng.integers(-50, 50, N_S).astype(np.int32), rng.integers(-50, 50, N_R).astype(np.int32)
    s_valid = rng.random(N_S) < 0.9
    cells = rng.choice(N_S * (N_R - 1), N_PAIRS, replace=False)         # each (s, r) once, and no pair names R row 0
    map_s, map_r = (BASE + cells // (N_R - 1)).astype(U32), (1 + cells % (N_R - 1)).astype(U32)
    map_s[::37] = so.NO_ROW
    want = ac.model_call(map_s, map_r, BASE, N_S, N_R, wc.term_of(s, ">=", r, s_valid, None))
    n_kept = want["info"][0]
    assert 1000 < n_kept < N_S and want["best_row"].min() > 0        # no S row keeps R row 0: a bestRow left at 0 shows
    sw, rw = -(-N_S // 32), -(-N_R // 32)
    assert lib._hj_signatures["hj_pairs_asof_dev"] and so.contract()["hj_pairs_asof_dev"][0] == "asynchronous"
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        st = so.Stage(fl.stream)
        # decoys: maps of HJ_NO_ROW, an S column below everything in R, an all-NULL validity -- three times "nothing eligible"
        bMS = st.buf(np.full(N_PAIRS, so.NO_ROW, dtype=U32), real=map_s, warm=np.roll(map_s, 1))
        bMR = st.buf(np.full(N_PAIRS, so.NO_ROW, dtype=U32), real=map_r, warm=np.roll(map_r, 2))
        bS = st.buf(np.full(N_S, np.iinfo(np.int32).min, dtype=np.int32), real=s, warm=s[::-1].copy())
        bR = st.buf(np.full(N_R, np.iinfo(np.int32).max, dtype=np.int32), real=r, warm=r[::-1].copy())
        bV = st.buf(np.zeros(sw, dtype=U32), real=plane_words(s_valid), warm=plane_words(~s_valid))
        # the best planes: what arrives behind the delay must be overwritten by the call's own initialisation
        bBV = st.buf(np.full(N_S, 0x1111111111111111, dtype=U64), real=np.full(N_S, ~U64(0), dtype=U64), warm=np.full(N_S, ~U64(0), dtype=U64), fetch=True)
        bBR = st.buf(np.full(N_S, 0x22222222, dtype=U32), real=np.zeros(N_S, dtype=U32), warm=np.zeros(N_S, dtype=U32), fetch=True)
        oS, oR = st.out(n_kept + SLACK, U32, so.NO_ROW), st.out(n_kept + SLACK, U32, so.NO_ROW)
        pS, pR = st.out(sw, U32, 0), st.out(rw, U32, 0)              # the mark planes, cleared by the caller

        def seq(which):
            t = _lib.hj_asof_term()
            t.s, t.r, t.sValid, t.rValid = bS.ptr, bR.ptr, bV.ptr, None
            t.width, t.type, t.op = 4, _lib.HJ_VAL_INT, _lib.HJ_CMP_GE
            rc = lib.hj_pairs_asof_dev(ctx._h, vp(bMS.ptr), vp(bMR.ptr), N_PAIRS, BASE, N_S, N_R, C.byref(t), vp(bBV.ptr), vp(bBR.ptr),
                                       vp(oS.ptr), vp(oR.ptr), n_kept + SLACK, vp(pS.ptr), vp(pR.ptr))
            C.memset(C.byref(t), 0, C.sizeof(t))                     # the descriptor was read before the call returned
            assert rc == _lib.HJ_OK, lib.hj_last_error(ctx._h)

        so.run_delayed([st], seq, True, f"asof.{fl.name}")           # asserts pending() after the enqueue: the call did not block
        st.check_inputs_intact()
        info = ctx.asof_info()
    assert (info[0], info[1], info[3]) == (n_kept, n_kept, want["info"][3]), (info, want["info"])
    got_s, got_r = st.result(oS, U32, "kept S"), st.result(oR, U32, "kept R")
    assert (got_s[n_kept:] == so.NO_ROW).all() and (got_r[n_kept:] == so.NO_ROW).all(), "a word behind the last pair was written"
    assert np.array_equal(packed(got_s[:n_kept], got_r[:n_kept]), want["kept"])
    assert np.array_equal(st.result(pS, U32, "S marks"), want["s_marks"]) and np.array_equal(st.result(pR, U32, "R marks"), want["r_marks"])
    assert np.array_equal(st.result(bBR, U32, "bestRow"), want["best_row"])
    assert (st.result(bBV, U64, "bestVal")[want["best_row"] == wc.NO_ROW] == 0).all()
