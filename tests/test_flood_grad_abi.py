"""ABI of the witness entry points (csrc/flood_grad.hip): the parameter block against the header, the declarations."""

import ctypes
import os

import pytest

from flooder_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_witness_search_block_has_the_layout_of_the_header():
    """(size and offsets against the header: test_host.py, test_parameter_block_has_the_layout_of_the_header)"""
    cls = _native.WitnessSearch
    blk = cls(n_pts=7, R=3)
    assert blk.size == ctypes.sizeof(cls) and blk.abi == 1 and blk.n_pts == 7 and not blk.q_d2
    with pytest.raises(TypeError):
        cls(no_such_field=1)


def test_witness_entry_points_are_declared_and_short():
    header = open(os.path.join(ROOT, "include", "flooder_hip.h")).read()
    for name in ("flooder_face_argmax_f32", "flooder_witness_search", "flooder_segment_sum_f32"):
        assert f"{name}(" in header
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) <= 12
    assert os.path.exists(_native.LIB_PATH), "libflooder_hip.so not built (python -m flooder_amd.build)"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("flooder_face_argmax_f32", "flooder_witness_search", "flooder_segment_sum_f32"):
        assert hasattr(lib, name)


def test_witness_search_refuses_a_foreign_block():
    lib = _native.load()
    blk = _native.WitnessSearch()
    blk.abi = 2
    assert lib.flooder_witness_search(ctypes.byref(blk), None) != 0
    blk = _native.WitnessSearch()
    blk.size = ctypes.sizeof(blk) + 8
    assert lib.flooder_witness_search(ctypes.byref(blk), None) != 0
