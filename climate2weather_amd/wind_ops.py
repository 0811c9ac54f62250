"""ctypes wrappers of the wind-power entry points of libc2w_hip.so (include/c2w_hip.h: c2w_wind_*), in the style of ``ops.py``; the
host side that calls them is ``windpower.py``."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .ops import _accepted, _nbytes, _p, _stream


def wind_supported(hw: int, K: int) -> bool:
    return bool(_lib.load().c2w_wind_supported(hw, K))


def wind_table_bytes(K: int) -> int:
    """bytes of the packed table of a curve of K knots (0 for K outside 2 .. 256)"""
    return int(_lib.load().c2w_wind_table_bytes(K))


def wind_table(xs: np.ndarray, ps: np.ndarray):
    """The packed table of the curve ``(xs, ps)`` (float64, K knots each) as a uint8 array on the host, or None where the library
    refuses the curve: K outside 2 .. 256, or knots that no longer increase strictly once rounded to fp32.  Pure host code."""
    xs, ps = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ps, dtype=np.float64)
    K = int(xs.shape[0])
    nbytes = wind_table_bytes(K)
    if nbytes == 0:
        return None
    buf = np.zeros(nbytes // 16, dtype=[("a", "<u8"), ("b", "<u8")])  # 16-byte items: NumPy aligns them
    assert buf.ctypes.data % 16 == 0
    rc = _lib.load().c2w_wind_table(xs.ctypes.data_as(ctypes.c_void_p), ps.ctypes.data_as(ctypes.c_void_p), K, buf.ctypes.data_as(ctypes.c_void_p))
    if rc == -1:
        return None
    check(rc, "c2w_wind_table")
    return buf.view(np.uint8)


def wind_scratch_bytes(planes: int, hw: int) -> int:
    """bytes of scratch ``wind_power`` needs for ``planes`` planes of hw cells (0 while a plane is one chunk)"""
    return int(_lib.load().c2w_wind_scratch_bytes(planes, hw))


def wind_power(fields, F, u_index, v_index, table, K, hub, sums, derived, scratch, planes, hw) -> bool:
    """sums (planes, 2) float64 = per plane the sums over its hw cells of the hub-height speed and of the power, from the u and v planes
    of fields (planes, F, hw) -- dense fp32, 16-byte aligned (include/c2w_hip.h::c2w_wind_power: the definition, the table, the fixed
    summation order); table: the device copy of ``wind_table``'s bytes; derived, if not None: (planes, 2, hw) fp32, speed and power per
    cell.  scratch: a float64 device tensor of at least ``wind_scratch_bytes`` bytes, or None where that is 0.  False if hw or K is not
    supported -- nothing is written and the caller takes the general definition (windpower.wind_fields)."""
    rc = _lib.load().c2w_wind_power(_p(fields), F, u_index, v_index, _p(table), K, hub, _p(sums), _p(derived), _p(scratch), _nbytes(scratch), planes, hw,
                                    _stream())
    return _accepted(rc, "c2w_wind_power")
