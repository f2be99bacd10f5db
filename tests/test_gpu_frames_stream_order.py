"""hj_window_frames_dev behind a delayed caller's stream (stream_order.py as it stands). Before the delay the inputs hold
decoys -- a dPerm of HJ_NO_ROW (nothing would be written), one partition id, zero values under an all-NULL plane --, the
real inputs arrive behind it on the same stream. A call that left the stream's order computes on the decoys and writes
nothing."""
import ctypes as C

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import frames_common as fc
import stream_order as so
from gpu_harness import fl  # noqa: F401

pytestmark = pytest.mark.gpu
U32, U64 = np.uint32, np.uint64
A = _lib
T, L = fc.layout(1)[:2]


def test_frames_behind_a_delayed_stream(fl):
    n = 2 * L + 5
    base = fc.build(n, [(0, 0)], "geometric", seed=14)
    rng = np.random.default_rng(15)
    src, valid = rng.integers(-99, 99, n).astype(np.int32), rng.random(n) < 0.8
    frames = [(A.HJ_AGG_SUM, -6, 0), (A.HJ_AGG_MIN, -(T + 1), 2), (A.HJ_AGG_MAX, None, None), (A.HJ_AGG_COUNT, -1, L + 1), (A.HJ_AGG_SUM, 1, None)]
    case = fc.Case(n, n, base.perm, base.part, [fc.Func(op, lo, hi, src, valid) for op, lo, hi in frames])
    want, counts = fc.model(case)
    plane = case.funcs[0].plane(n)
    assert counts[0] > 10
    vp = lambda p: C.c_void_p(p) if p else None     # noqa: E731
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        st = so.Stage(fl.stream)
        b_perm = st.buf(np.full(n, so.NO_ROW, dtype=U32), real=case.perm, warm=np.roll(case.perm, 7))
        b_part = st.buf(np.zeros(n, dtype=U32), real=case.part, warm=np.roll(case.part, 3))
        b_src = st.buf(np.zeros(n, dtype=np.int32), real=src, warm=src[::-1].copy())
        b_plane = st.buf(np.zeros_like(plane), real=plane, warm=~plane)
        outs = [st.out(n, U64, fc.SENT64) for _ in case.funcs]

        def seq(which):
            arr, k = fc.func_array(case.funcs, [(o.ptr, b_src.ptr, b_plane.ptr) for o in outs])
            rc = lib.hj_window_frames_dev(ctx._h, vp(b_perm.ptr), n, n, vp(b_part.ptr), arr, k)
            C.memset(arr, 0, C.sizeof(arr))                   # the descriptors were read before the call returned
            if rc != _lib.HJ_OK:
                raise hj.HashJoinError(rc, lib.hj_last_error(ctx._h).decode())

        assert so.contract()["hj_window_frames_dev"][0] == "asynchronous"
        so.run_delayed([st], seq, True, f"window_frames.{fl.name}")
        st.check_inputs_intact()
        info = ctx.window_frames_info()
    assert (info["positions"], info["partitions"], info["peer_runs"], info["skipped"]) == (n, counts[0], 0, counts[1])
    fc.same([st.result(o, U64, i) for i, o in enumerate(outs)], want, "behind the delay")
