"""amt_peak_markers without a GPU: the symbol is exported and declared, the constant of the LDS tier agrees between the
header and the binding, and bad arguments are refused before a device is touched."""
import os
import re

import numpy as np

from arcadia_microscopy_tools_amd import _hip, hipops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    assert re.search(r"^int amt_peak_markers\s*\(", header, flags=re.M)
    assert "amt_peak_markers" in _hip.exported_names()
    assert hasattr(_hip.load_library(), "amt_peak_markers")
    tier = re.search(r"#define\s+AMT_PEAK_MARKERS_LDS_TIER\s+(\d+)", header)
    assert tier and int(tier.group(1)) == _hip.PEAK_MARKERS_LDS_TIER == hipops.PEAK_MARKERS_LDS_TIER


def test_bad_arguments_return_minus_one():
    lib = _hip.load_library()
    buf = np.zeros(7 * 64, np.int32)
    # every operand in 256 bytes of its own: an output that overlapped another operand would be refused for that instead
    d2, mask, peaks, markers, count, klist, kcount = (buf[k * 64:].ctypes.data for k in range(7))
    #       ctx   d2 mask peaks markers count n  H  W  m  conn cap list count
    good = [None, d2, mask, peaks, markers, count, 1, 4, 4, 1, 1, 4, klist, kcount]
    assert lib.amt_peak_markers(*good) == -1
    assert lib.amt_last_error() == b"null context"  # every argument passed: only the context is missing

    def refused(index, value, message):
        args = list(good)
        args[index] = value
        assert lib.amt_peak_markers(*args) == -1, (index, value)
        assert message in lib.amt_last_error(), (index, value, lib.amt_last_error())

    refused(12, None, b"go together")
    refused(13, None, b"go together")
    for index in (1, 2, 3, 4, 5):
        refused(index, None, b"bad arguments")
    refused(6, -1, b"bad arguments")
    refused(7, 0, b"bad arguments")
    refused(8, 0, b"bad arguments")
    refused(9, -1, b"min_distance")
    refused(9, 17, b"min_distance")
    refused(10, 0, b"connectivity")
    refused(10, 3, b"connectivity")
    refused(11, 0, b"capacity")
    huge = list(good)
    huge[7] = huge[8] = 65536  # 2^32 pixels do not fit the int32 pixel indices of the lists
    for k, index in enumerate((1, 2, 3, 4, 5, 12, 13)):
        huge[index] = (k + 1) << 40  # planes of 2^34 bytes at addresses of their own (nothing is read: refused first)
    assert lib.amt_peak_markers(*huge) == -1 and b"too large" in lib.amt_last_error()
    assert not buf.any()
