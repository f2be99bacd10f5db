"""hj_range_index_dev and hj_range_pairs_dev enqueued back to back behind a delayed caller's stream (stream_order.py as it
stands): the range call reads dHead on the device, so no host wait stands between the index and its probes. Before the delay
R's column and the bounds hold decoys that pair nothing; the real inputs arrive behind it on the same stream. A call that
left the stream's order, or read the head on the host, computes on the decoys and returns no pair."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj

import range_common as rc
import stream_order as so
from gpu_harness import fl  # noqa: F401

pytestmark = pytest.mark.gpu
U32, U64 = np.uint32, np.uint64
SLACK = 64
N_R, N_S = 20011, 9001


def test_index_and_range_call_back_to_back(fl):
    contract = so.contract()
    assert contract["hj_range_index_dev"][0] == "asynchronous" and contract["hj_range_pairs_dev"][0] == "asynchronous"

    def inputs(seed):
        g = np.random.default_rng(seed)
        r = g.integers(-5000, 5000, N_R).astype(np.int64)
        lo = g.integers(-5200, 5200, N_S).astype(np.int64)
        return r, lo, lo + g.integers(-1, 4, N_S)

    (r, lo, hi), (wr, wlo, whi) = inputs(1), inputs(2)
    want = rc.model_call(r, lo, hi, hi_open=True)
    total = want["info"][0]
    assert total > 4 * hj.range_layout_info(N_R, N_S)["tile"]
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        st = so.Stage(fl.stream)
        # the decoys pair nothing, with each other or with the real columns: R far above every bound, every interval empty
        bR = st.buf(np.full(N_R, 1 << 40, dtype=np.int64), real=r, warm=wr)
        bLo = st.buf(np.full(N_S, 7, dtype=np.int64), real=lo, warm=wlo)
        bHi = st.buf(np.full(N_S, 7, dtype=np.int64), real=hi, warm=whi)
        perm, keys, head = st.out(N_R, U32, so.SENT32), st.out(N_R, U64, so.SENT64), st.out(4, U32, so.SENT32)
        out_s, out_r = st.out(total + SLACK, U32, so.NO_ROW), st.out(total + SLACK, U32, so.NO_ROW)
        s_marks, r_marks = st.out(-(-N_S // 32), U32, 0), st.out(-(-N_R // 32), U32, 0)

        def seq(which):
            ctx.range_index((bR.ptr, 0, 8, hj.HJ_VAL_INT), N_R, perm.ptr, keys.ptr, head.ptr)
            ctx.range_pairs(keys.ptr, perm.ptr, head.ptr, N_R, (bLo.ptr, bHi.ptr, 8, hj.HJ_VAL_INT, hj.HJ_RANGE_HI_OPEN), N_S, 100, out_s.ptr, out_r.ptr,
                            total + SLACK, s_marks.ptr, r_marks.ptr)

        so.run_delayed([st], seq, True, f"range.index_pairs.{fl.name}")          # asserts pending() after the enqueue
        st.check_inputs_intact()
        info = ctx.range_pairs_info()
    assert info[:2] == (total, total) and info[3:] == want["info"][3:], (info, want["info"])
    assert np.array_equal(st.result(perm, U32, "perm"), want["index"]["perm"]) and tuple(st.result(head, U32, "head")) == (N_R, 0, 0, 8)
    s, r_rows = st.result(out_s, U32, "S map"), st.result(out_r, U32, "R map")
    assert (s[total:] == so.NO_ROW).all() and (r_rows[total:] == so.NO_ROW).all(), "a word behind the last pair was written"
    assert np.array_equal(rc.packed(s[:total] - 100, r_rows[:total]), want["kept"])
    assert np.array_equal(st.result(s_marks, U32, "S marks"), want["s_marks"]) and np.array_equal(st.result(r_marks, U32, "R marks"), want["r_marks"])
