"""window_rows on an MI355X with the framed specs ("sum" | "min" | "max" | "count" | "mean", column, lo, hi) beside the old
ones, against window_rows_host and against the per-partition loop of frames_common: more than HJ_FRAME_MAX_FUNCS framed
device functions, so that two rounds of hj_window_frames_dev run behind the rounds of hj_window_rows_dev, on the same ids
and permutation."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from frames_common import BESIDE, FRAMED, framed_call, framed_check
from window_common import wrapper_table

pytestmark = pytest.mark.gpu
assert len(FRAMED) > _lib.HJ_FRAME_MAX_FUNCS


def _same(got, host):
    assert got.keys() == host.keys() and set(FRAMED) | set(BESIDE) < set(got)
    for name, h in host.items():
        g = got[name]
        if isinstance(h, hj.KeyColumn):
            assert isinstance(g, hj.KeyColumn) and g.values.dtype == h.values.dtype and g.to_list() == h.to_list(), name
        elif isinstance(h, np.ndarray):
            assert g.dtype == h.dtype and np.array_equal(g, h), name
        else:
            assert g == h, name


@pytest.mark.parametrize("null_keys", ["group", "drop"])
def test_window_rows_with_frames_equals_its_host_form(null_keys):
    t = wrapper_table(400, 7)
    t["u"] = t["u"] >> np.uint64(8)
    got, host = framed_call(hj.window_rows, t, null_keys), framed_call(hj.window_rows_host, t, null_keys)
    _same(got, host)
    if null_keys == "drop":
        assert got["null_rows"] > 0 and (got["rn"] == 0).sum() == got["null_rows"]
    framed_check(got, t, null_keys)


def test_framed_specs_alone_without_a_sort():
    """no window function of the old kind: n_partitions comes from the frames' own info; no partition, no order: no sort"""
    v = np.arange(5000, dtype=np.int64)
    got = hj.window_rows({"s": ("sum", "v", -6, 0), "m": ("max", "v", None, None), "c": ("count", None, 1, 3)}, cols={"v": v})
    want = np.cumsum(v) - np.concatenate([np.zeros(7, dtype=np.int64), np.cumsum(v)[:-7]])
    assert np.array_equal(got["s"].values, want) and (got["m"].values == 4999).all() and got["n_partitions"] == 1
    assert got["c"].tolist() == [3] * 4996 + [3, 2, 1, 0]
