"""The resident-R radix join's entry points without a GPU: declared, bound, and failing loudly (no CPU fallback)."""
import ctypes

import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

NEW = ("hj_prj_build_dev", "hj_prj_probe_dev", "hj_prj_resident_info")


def test_entry_points_are_exported_with_signatures():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name)
        assert name in hj.lib._hj_signatures


def test_null_context_is_rejected():
    out = (ctypes.c_uint64 * 8)()
    assert hj.lib.hj_prj_build_dev(None, None, 16) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_prj_probe_dev(None, None, 0) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_prj_resident_info(None, out) == _lib.HJ_ERR_INVALID


def test_python_methods_raise_without_a_device_context():
    """A context that holds no device handle (what a failed or closed hj_create leaves) raises HashJoinError from every
    new method instead of computing anything on the host."""
    if hj.device_count() == 0:
        with pytest.raises(hj.HashJoinError) as e:
            hj.HashJoinContext(0)
        assert e.value.status == _lib.HJ_ERR_NO_DEVICE
    ctx = object.__new__(hj.HashJoinContext)
    ctx._h = None
    for call in (lambda: ctx.prj_build(0x1000, 64), lambda: ctx.prj_probe(0x1000, 64), ctx.prj_resident_info):
        with pytest.raises(hj.HashJoinError):
            call()
