"""Z-stacks without a GPU: the numpy reference against hand-worked examples and its own invariants, the header's statement
of the five codes and four columns, every refusal of the C ABI that needs no device (null context), the Python layers'
argument errors before any device access, and ``project_z``'s metadata handling on its error paths.  The focus rule is this
project's own: nothing here claims parity with another program's stack focuser."""
import os
import re
import warnings
from fractions import Fraction

import numpy as np
import pytest

import zstack_cases as cases
import zstack_reference as ref
from arcadia_microscopy_tools_amd import _hip, hipops, operations
from arcadia_microscopy_tools_amd.channels import DAPI, FITC
from arcadia_microscopy_tools_amd.device import DeviceArray
from arcadia_microscopy_tools_amd.exceptions import MetadataWarning
from arcadia_microscopy_tools_amd.metadata_structures import ChannelMetadata, DimensionFlags, NominalDimensions
from arcadia_microscopy_tools_amd.microscopy import DeviceImage, InstrumentMetadata, Metadata, MicroscopyImage, _ZPlan
from arcadia_microscopy_tools_amd.pipeline import ImageOperation, Pipeline, is_device_operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "amt_hip.h")).read()


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_reference_gives_the_hand_results():
    # a single bright pixel in the middle of 3 x 3: L = 4 c there, -c at the four edge neighbours, 0 in the corners
    p = np.zeros((3, 3), np.uint16)
    p[1, 1] = 10
    assert ref.laplacian(p).tolist() == [[0, -10, 0], [-10, 40, -10], [0, -10, 0]]
    # r = 0: E = L^2; r = 1: the window clipped to the image -- a corner sees four positions, the centre all nine
    assert ref.energy(p, 0).tolist() == [[0, 100, 0], [100, 1600, 100], [0, 100, 0]]
    assert ref.energy(p, 1).tolist() == [[1800, 1900, 1800], [1900, 2000, 1900], [1800, 1900, 1800]]
    assert ref.energy(p, 15).tolist() == [[2000] * 3] * 3
    # edge replication: a ramp along x has L = 0 inside and +-1 at the two ends
    ramp = np.tile(np.arange(3, dtype=np.uint16), (3, 1))
    assert ref.laplacian(ramp).tolist() == [[-1, 0, 1]] * 3
    # the four sums of the bright pixel: 10, 100, 1600 + 4 * 100, and Brenner's (0 - 0)^2 per row
    assert ref.focus_sums(p[None]).tolist() == [[10, 100, 2000, 0]]
    assert ref.focus_sums(ramp[None]).tolist() == [[9, 15, 6, 12]]
    # scores: 2000 / 9, (9 * 100 - 100) / (9 * 10), Brenner
    assert ref.focus_scores(p[None], "laplacian_variance")[0] == float(Fraction(2000, 9))
    assert ref.focus_scores(p[None], "normalized_variance")[0] == float(Fraction(800, 90))
    assert ref.focus_scores(ramp[None], "brenner")[0] == 12.0
    assert ref.focus_scores(np.zeros((1, 3, 3), np.uint16), "normalized_variance")[0] == 0.0
    # the smallest z wins among equals, a strictly larger E later takes over
    flat = np.full((3, 3), 7, np.uint16)
    stack = np.stack([flat, p, p, flat])
    assert ref.focus_index(stack, 1).tolist() == [[1] * 3] * 3 and ref.focus_index(stack, 1).dtype == np.uint16
    assert ref.focus_index(np.stack([flat, flat]), 0).tolist() == [[0] * 3] * 3
    assert ref.focus_index(stack, 0).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert ref.focus_stack(stack, 0).tolist() == [[7, 0, 7], [0, 10, 0], [7, 0, 7]]
    assert ref.z_take(stack, np.full((3, 3), 9, np.uint16)).tolist() == flat.tolist()  # clamped to Z - 1
    assert ref.median_nearest(np.array([[0, 0, 0], [0, 5, 0], [0, 0, 0]], np.uint16), 3).tolist() == [[0] * 3] * 3


def test_the_laplacian_sums_to_zero_on_every_case():
    seen = 0
    for name, stack, r in cases.cases():
        if r is None:
            continue
        for s in stack:
            for plane in s:
                assert int(ref.laplacian(plane).sum()) == 0, name
                seen += 1
    assert seen > 100


def test_numpy_mean_is_the_stated_mean():
    for name, stack, r in cases.cases():
        if stack.dtype == np.uint8:
            continue
        for s, want in zip(stack, cases.reference((name, stack, r))["mean"]):
            got = np.mean(s, axis=0)
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), name
    assert sum(1 for c in cases.cases() if c[1].dtype == np.float64) >= 2


def test_the_reference_recovers_the_planted_depth_map():
    """a sanity condition on the reference (it measured 99.1 %), not a tolerance for the device"""
    stack = [c for c in cases.cases() if c[0] == "planted depth map"][0][1][0]
    assert stack.shape == (5, 70, 131)
    share = float((ref.focus_index(stack, 4) == cases.planted_z0((70, 131))).mean())
    assert share >= 0.95, share


def test_the_table_is_not_vacuous():
    table = {c[0]: c for c in cases.cases()}
    TH, TW = hipops.zstack_tile()
    shapes = {c[1].shape[2:] for c in table.values()}
    for shape in ((TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (70, 131), (3, 5), (1, 1), (1, 131), (70, 1), (9, 11)):
        assert shape in shapes, shape
    for small in ((3, 5), (1, 1)):  # every radius, so the window is larger than the plane
        assert {c[2] for c in table.values() if c[1].shape[2:] == small and c[2] is not None} == {0, 1, 4, 15}
    assert {c[1].shape[1] for c in table.values()} >= {1, 2, 5, 257}
    assert {c[1].dtype for c in table.values()} == {np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float64)}
    # an 8-bit index would fail: planes past 255 win somewhere
    assert int(cases.reference(table["Z 257 9 x 11"])["index"].max()) > 255
    # 32-bit arithmetic would fail: L^2 needs 37 bits, and the window sum more
    board = table["checkerboard r 15"][1][0]
    assert int(np.abs(ref.laplacian(board[1])).max()) == 262140 and int(ref.energy(board[1], 15).max()) > 2**40
    assert cases.reference(table["checkerboard r 15"])["index"].tolist() == np.ones((1, 70, 131), int).tolist()
    # equal planes: index 0 everywhere; values in 0..3: tied maxima exist, and the smallest z wins them
    assert not cases.reference(table["equal planes"])["index"].any()
    ties = cases.tie_stack()
    E = np.stack([ref.energy(p, 1) for p in ties])
    tied = (E == E.max(axis=0)).sum(axis=0) > 1
    assert tied.mean() > 0
    assert np.array_equal(cases.reference(table["ties 0..3"])["index"][0][tied], np.argmax(E, axis=0)[tied])
    # the gather's index maps reach past the stack
    assert all(int(cases.take_index(c).max()) >= c[1].shape[1] for c in table.values() if c[1].shape[2:] == (70, 131))
    # the batch's stacks differ
    batch = table["batch of three"][1]
    assert len(batch) == 3 and not np.array_equal(batch[0], batch[1]) and not np.array_equal(batch[1], batch[2])


# ---- the header and the codes ---------------------------------------------------------------------------------------------
def test_header_defines_and_documents_the_codes():
    for name, value in (("AMT_RANK_Z_PROJECT", 10), ("AMT_RANK_Z_FOCUS_SUMS", 11), ("AMT_RANK_Z_FOCUS_INDEX", 12),
                        ("AMT_RANK_Z_FOCUS_STACK", 13), ("AMT_RANK_Z_TAKE", 14), ("AMT_ZF_NCOLS", 4),
                        ("AMT_ZSTACK_TILE_H", _hip.ZSTACK_TILE[0]), ("AMT_ZSTACK_TILE_W", _hip.ZSTACK_TILE[1]),
                        ("AMT_ZSTACK_MAX_RADIUS", _hip.ZSTACK_MAX_RADIUS)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", HEADER, re.M), name
    for i, col in enumerate(_hip.ZF_COLS):
        assert re.search(rf"^#define\s+AMT_ZF_{col.upper()}\s+{i}\s*$", HEADER, re.M), col
    block = HEADER[:HEADER.index("int amt_rank_filter(")]
    block = block[block.rindex("/* grey erosion"):]
    for word in ("AMT_RANK_Z_PROJECT", "AMT_RANK_Z_FOCUS_SUMS", "AMT_RANK_Z_FOCUS_INDEX", "AMT_RANK_Z_FOCUS_STACK",
                 "AMT_RANK_Z_TAKE", "AMT_ZF_SUM", "AMT_ZF_SUMSQ", "AMT_ZF_LAP_SUMSQ", "AMT_ZF_BRENNER", "1..65535",
                 "0 = max, 1 = min, 2 = mean", "edge replication", "smallest z", "2^27", "262140", "2^46", "clamped",
                 "nplanes == 0", "AMT_EINVAL", "asynchronous", "unpinned offline", "never reaches memory", "64-bit",
                 "op 7 is not an op"):
        assert word in block, word


def test_python_constants_agree_with_the_header():
    assert (_hip.RANK_Z_PROJECT, _hip.RANK_Z_FOCUS_SUMS, _hip.RANK_Z_FOCUS_INDEX, _hip.RANK_Z_FOCUS_STACK,
            _hip.RANK_Z_TAKE) == (10, 11, 12, 13, 14)
    assert _hip.ZF_COLS == ref.COLS and _hip.ZF_NCOLS == 4
    assert _hip.Z_PROJECT_METHODS == {"max": 0, "min": 1, "mean": 2}
    assert hipops.zstack_tile() == _hip.ZSTACK_TILE
    for name in ("z_project", "focus_sums", "focus_index", "focus_stack", "z_take", "zstack_tile"):
        assert callable(getattr(hipops, name))
    for name in ("z_project", "best_focus", "extended_depth_of_field"):
        assert is_device_operator(getattr(operations, name))
    assert callable(operations.focus_scores)
    for doc in (hipops.focus_index.__doc__, operations.extended_depth_of_field.__doc__):
        assert "package's own" in doc


def test_no_new_prototype():
    """The capability rides on amt_rank_filter: the C ABI has the names it had."""
    bare = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    names = re.findall(r"^(?:int|const char\s*\*)\s*(amt_\w+)\s*\(", bare, flags=re.M)
    assert len(names) == len(set(names)) == len(_hip._SIGS) and set(names) == set(_hip._SIGS)
    assert not [n for n in names if "zstack" in n or "focus" in n or "project" in n or "z_take" in n]
    lib = _hip.load_library()
    for hidden in ("amt_z_project", "amt_focus_index", "amt_focus_stack", "amt_focus_sums", "amt_z_take", "amt_i_zstack"):
        assert not hasattr(lib, hidden)


# ---- the C ABI with a null context ------------------------------------------------------------------------------------------
_BUF = np.zeros(1 << 16, np.uint8)
_A = (_BUF.ctypes.data + 255) & ~255
_B = _A + (1 << 15)
_M = _A + (1 << 14)
ONE = np.ones((1, 1), np.uint8)
OPS = (10, 11, 12, 13, 14)


def _call(op, *, dtype=_hip.U16, fp=ONE, Z=3, cval=0.0, inp=None, out=None, minuend="default", H=4, W=4, nplanes=1):
    lib = _hip.load_library()
    fp = np.ascontiguousarray(fp, np.uint8)
    if minuend == "default":
        minuend = _M if op == 14 else None
    rc = lib.amt_rank_filter(None, _A if inp is None else inp, _B if out is None else out, dtype, nplanes, H, W,
                             fp.ctypes.data, fp.shape[0], fp.shape[1], op, Z, float(cval), minuend)
    return rc, lib.amt_last_error().decode()


def test_complete_calls_reach_the_context():
    for op in OPS:
        for Z in (1, 2, 65535):
            assert _call(op, Z=Z, inp=1 << 40, out=3 << 40, minuend=(5 << 40) if op == 14 else None) == (-1, "null context")
        assert _call(op, nplanes=0) == (-1, "null context")
        assert _call(op, dtype=_hip.U8) == (-1, "null context")
    for op in (10, 14):
        assert _call(op, dtype=_hip.F64) == (-1, "null context")
    for cval in (0.0, 1.0, 2.0):
        assert _call(10, cval=cval) == (-1, "null context")
    for op in (12, 13):
        for r in (0, 1, 4, 15):
            assert _call(op, fp=np.full((2 * r + 1, 2 * r + 1), 1 + r)) == (-1, "null context")
    for op in (10, 11, 14):  # the footprint is ignored
        assert _call(op, fp=np.zeros((3, 5))) == (-1, "null context")


@pytest.mark.parametrize("op", OPS)
def test_refusals_need_no_device(op):
    for dtype in (_hip.I32, _hip.F32, _hip.I64, 17) + ((_hip.F64,) if op in (11, 12, 13) else ()):
        code, msg = _call(op, dtype=dtype)
        assert code == -1 and "dtype" in msg and "null context" not in msg, msg
    for Z in (0, -1, 65536, 2**31 - 1):  # far apart: the aliasing check comes first, and it reads Z planes per stack
        code, msg = _call(op, Z=Z, inp=1 << 40, out=3 << 40, minuend=(5 << 40) if op == 14 else None)
        assert code == -1 and "Z (mode)" in msg and "null context" not in msg, msg
    code, msg = _call(op, minuend=None if op == 14 else _M)
    assert code == -1 and "minuend" in msg and "null context" not in msg, msg
    code, msg = _call(op, H=65536, W=32768, inp=1 << 40, out=3 << 40, minuend=(5 << 40) if op == 14 else None)
    assert code == -1 and "plane too large" in msg, msg
    if op in (12, 13):
        for fp in (np.ones((3, 5)), np.ones((33, 33)), np.eye(3), np.zeros((3, 3)), np.ones((2, 2)),
                   [[1, 1, 1], [1, 0, 1], [1, 1, 1]]):
            code, msg = _call(op, fp=fp)
            assert code == -1 and "footprint" in msg and "null context" not in msg, msg
    if op == 10:
        for cval in (3.0, -1.0, 0.5, float("nan")):
            code, msg = _call(op, cval=cval)
            assert code == -1 and "cval" in msg and "null context" not in msg, msg
    if op == 11:
        code, msg = _call(op, H=16384, W=8193, inp=1 << 40, out=3 << 40)
        assert code == -1 and "2^27" in msg, msg
        assert _call(op, H=16384, W=8192, inp=1 << 40, out=3 << 40) == (-1, "null context")


def test_aliasing_is_refused_with_the_span_each_op_has():
    plane = 4 * 4 * 2  # uint16
    for op in OPS:
        # `in` is nplanes x Z planes: an output that begins inside the last plane of the last stack overlaps
        for s in (0, 8, 2 * 3 * plane - 2):
            code, msg = _call(op, nplanes=2, out=_A + s)
            assert code == -1 and "alias" in msg and msg.startswith("amt_rank_filter: "), (op, s, msg)
        assert _call(op, nplanes=2, out=_A + 2 * 3 * plane) == (-1, "null context")  # right behind the stacks
    # the outputs' own lengths: max keeps the dtype, mean writes float64, the sums are nplanes x Z x 4 x 8 bytes
    assert _call(10, nplanes=2, out=_A - 2 * plane) == (-1, "null context")
    code, msg = _call(10, nplanes=2, cval=2.0, out=_A - 2 * plane)
    assert code == -1 and "alias" in msg, msg
    assert _call(10, nplanes=2, cval=2.0, out=_A - 2 * 4 * 4 * 8) == (-1, "null context")
    sums = 2 * 3 * 4 * 8
    assert _call(11, nplanes=2, out=_A - sums) == (-1, "null context")
    code, msg = _call(11, nplanes=2, out=_A - sums + 8)
    assert code == -1 and "alias" in msg, msg
    # uint8 stacks with a uint16 index map: twice the bytes of a plane
    code, msg = _call(12, nplanes=2, dtype=_hip.U8, out=_A - 2 * 16 * 2 + 2)
    assert code == -1 and "alias" in msg, msg
    assert _call(12, nplanes=2, dtype=_hip.U8, out=_A - 2 * 16 * 2) == (-1, "null context")
    # op 14: `out` must not overlap the index map either, which is uint16 whatever the stack is
    for s in (0, 2, 2 * plane - 2):
        code, msg = _call(14, nplanes=2, dtype=_hip.F64, out=_M - 2 * 16 * 8 + 2 + s if s else _M)
        assert code == -1 and ("alias" in msg or "differ from out" in msg), (s, msg)
    assert _call(14, nplanes=2, dtype=_hip.F64, out=_M + 2 * plane) == (-1, "null context")
    assert _call(14, nplanes=2, inp=_M) == (-1, "null context")  # inputs may overlap inputs


def test_the_other_ops_keep_their_answers():
    three = np.ones((3, 3), np.uint8)
    for op in (0, 1, 2, 7, -1, 15, 100):  # 7 and the codes past 14 reach the filter's own checks, behind the context
        assert _call(op, fp=three, Z=1) == (-1, "null context")
    for op in (3, 4):
        assert _call(op, fp=three, Z=1, minuend=_M) == (-1, "null context")
    for op in (8, 9):
        assert _call(op, fp=three, Z=1, dtype=_hip.I32) == (-1, "null context")


# ---- the Python layers' argument errors -------------------------------------------------------------------------------------
class _NoDevice:
    """Stands where a DeviceArray would: any attribute access means validation did not come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the array was touched ({name}) before the arguments were validated")


class _NoContext:
    """Stands where a Context would: an operator that reaches for it (allocation, handle, stream) fails."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}): a device call before the refusal")


_CTX = _NoContext()


def _HostOnly(shape, dtype, ptr=4096):
    """A DeviceArray that owns nothing, at a made-up address, on a context that refuses every use."""
    return DeviceArray(_CTX, ptr, shape, dtype)


def test_hipops_scalar_errors_come_before_any_device_access():
    for bad in ("median", "MAX", None, 0, "sum"):
        with pytest.raises(ValueError, match="method"):
            hipops.z_project(_NoDevice(), bad)
    for fn in (hipops.focus_index, hipops.focus_stack):
        for bad in (-1, 16, 100, 1.5, "4", None, True, np.True_):
            with pytest.raises(ValueError, match="radius"):
                fn(_NoDevice(), bad)
    for fn in (hipops.z_project, hipops.focus_sums, hipops.focus_index, hipops.focus_stack):
        with pytest.raises(ValueError, match="DeviceArray"):
            fn(np.zeros((1, 2, 4, 4), np.uint16))


def test_hipops_array_errors_come_before_any_device_access():
    every = (hipops.z_project, hipops.focus_sums, hipops.focus_index, hipops.focus_stack,
             lambda s: hipops.z_take(s, _NoDevice()))
    for fn in every:
        for shape in ((2, 4, 4), (4, 4), (1, 1, 2, 4, 4)):
            with pytest.raises(ValueError, match=r"\(N, Z, H, W\)"):
                fn(_HostOnly(shape, np.uint16))
        for dtype in (np.int32, np.float32, np.int64):
            with pytest.raises(ValueError, match="stacks must be"):
                fn(_HostOnly((1, 2, 4, 4), dtype))
        for shape in ((1, 0, 4, 4), (1, 65536, 1, 1)):
            with pytest.raises(ValueError, match="Z must be"):
                fn(_HostOnly(shape, np.uint16))
        with pytest.raises(ValueError, match="H \\* W"):
            fn(_HostOnly((1, 2, 0, 4), np.uint16))
    for fn in (hipops.focus_sums, hipops.focus_index, hipops.focus_stack):
        with pytest.raises(ValueError, match="raw data"):
            fn(_HostOnly((1, 2, 4, 4), np.float64))
    with pytest.raises(ValueError, match="2\\^27"):
        hipops.focus_sums(_HostOnly((1, 1, 16384, 8193), np.uint16))
    s = _HostOnly((2, 3, 4, 4), np.uint16)
    for bad in (_HostOnly((2, 4, 4), np.uint8, ptr=1 << 20), _HostOnly((2, 4, 5), np.uint16, ptr=1 << 20),
                _HostOnly((1, 4, 4), np.uint16, ptr=1 << 20), _HostOnly((2, 3, 4, 4), np.uint16, ptr=1 << 20),
                np.zeros((2, 4, 4), np.uint16), None):
        with pytest.raises(ValueError, match="index must be"):
            hipops.z_take(s, bad)
    # out= of the wrong shape or dtype, and overlapping operands through _no_alias
    far = 1 << 20
    for fn, shape, dtype in ((hipops.z_project, (2, 4, 4), np.uint16), (hipops.focus_sums, (2, 3, 4), np.int64),
                             (hipops.focus_index, (2, 4, 4), np.uint16), (hipops.focus_stack, (2, 4, 4), np.uint16)):
        with pytest.raises(ValueError, match="out has shape"):
            fn(s, out=_HostOnly(shape + (1,), dtype, ptr=far))
        with pytest.raises(ValueError, match="out has shape"):
            fn(s, out=_HostOnly(shape, np.float32, ptr=far))
        for ptr in (4096, 4096 + 8, 4096 + s.nbytes - 2):
            with pytest.raises(ValueError, match="alias"):
                fn(s, out=_HostOnly(shape, dtype, ptr=ptr))
        with pytest.raises(AssertionError, match="the context was used"):  # neighbours that touch: as far as the call
            fn(s, out=_HostOnly(shape, dtype, ptr=4096 + s.nbytes))
    with pytest.raises(ValueError, match="out has shape"):
        hipops.z_project(s, "mean", out=_HostOnly((2, 4, 4), np.uint16, ptr=far))
    index = _HostOnly((2, 4, 4), np.uint16, ptr=far)
    for o in (index, _HostOnly((2, 4, 4), np.uint16, ptr=far + 2), _HostOnly((2, 4, 4), np.uint16, ptr=4096 + 32)):
        with pytest.raises(ValueError, match="alias"):
            hipops.z_take(s, index, out=o)


def test_operations_errors_come_before_any_device_access():
    every = (operations.z_project, operations.focus_scores, operations.best_focus, operations.extended_depth_of_field)
    for fn in every:
        for shape in ((4, 4), (1, 2, 4, 4), (7,)):
            with pytest.raises(ValueError, match=r"\(Z, Y, X\)"):
                fn(np.zeros(shape, np.uint16))
            with pytest.raises(ValueError, match=r"\(Z, Y, X\)"):
                fn(_HostOnly(shape, np.uint16))
        for dtype in (np.int32, np.float32, bool):
            with pytest.raises(TypeError, match="stack must be"):
                fn(np.zeros((2, 4, 4), dtype))
        for shape in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
            with pytest.raises(ValueError, match="must not be empty"):
                fn(np.zeros(shape, np.uint16))
    for fn in every[1:]:
        with pytest.raises(TypeError, match="raw data"):
            fn(np.zeros((2, 4, 4), np.float64))
    for bad in ("median", None, 3):
        with pytest.raises(ValueError, match="method"):
            operations.z_project(_NoDevice(), bad)
        with pytest.raises(ValueError, match="method"):
            operations.focus_scores(_NoDevice(), bad)
        with pytest.raises(ValueError, match="method"):
            operations.best_focus(_NoDevice(), bad)
    for bad in (-1, 16, 2.0, "4", True):
        with pytest.raises(ValueError, match="radius"):
            operations.extended_depth_of_field(_NoDevice(), radius=bad)
    for bad in (1, 2, 4, 17, -3, 3.0, True):
        with pytest.raises(ValueError, match="smooth"):
            operations.extended_depth_of_field(_NoDevice(), smooth=bad)


def test_scores_are_exact_rationals_rounded_once():
    sums = np.array([[10, 100, 2000, 0], [0, 0, 0, 0], [3, 2**62, 2**62 + 1, 2**53 + 1]], np.int64)
    lap = operations._scores_from_sums(sums, 9, "laplacian_variance")
    assert lap.dtype == np.float64 and lap.tolist() == [float(Fraction(2000, 9)), 0.0, float(Fraction(2**62 + 1, 9))]
    nv = operations._scores_from_sums(sums, 9, "normalized_variance")
    assert nv.tolist() == [float(Fraction(800, 90)), 0.0, float(Fraction(9 * 2**62 - 9, 27))]
    assert operations._scores_from_sums(sums, 9, "brenner").tolist() == [0.0, 0.0, float(2**53)]


def test_the_operations_are_image_operations():
    pipe = Pipeline([ImageOperation(operations.z_project, method="mean"), ImageOperation(operations.apply_threshold, "otsu")])
    assert len(pipe) == 2 and not pipe._device_chain_applies(np.zeros((3, 8, 8), np.uint16))
    with pytest.raises(ValueError, match=r"\(Z, Y, X\)"):  # a plane reaches the operator through the ordinary call path
        ImageOperation(operations.extended_depth_of_field, radius=2)(np.zeros((8, 8), np.uint16))


# ---- project_z: metadata and error paths ------------------------------------------------------------------------------------
def _image(axes="CZYX", shape=(2, 3, 6, 7), dtype=np.uint16, resolution=True):
    sizes = dict(zip(axes, shape))
    flags = DimensionFlags(0)
    if "Z" in sizes:
        flags |= DimensionFlags.Z_STACK
    if "T" in sizes:
        flags |= DimensionFlags.TIMELAPSE
    metas = []
    for ch in (DAPI, FITC)[:sizes.get("C", 1)]:
        res = None
        if resolution:
            res = NominalDimensions(x_size_px=sizes["X"], y_size_px=sizes["Y"], xy_step_um=0.5, z_size_px=sizes.get("Z"),
                                    z_step_um=1.5 if "Z" in sizes else None, t_size_px=sizes.get("T"),
                                    t_step_ms=100.0 if "T" in sizes else None)
        metas.append(ChannelMetadata(ch, dimensions=flags, resolution=res))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", MetadataWarning)
        return MicroscopyImage(np.zeros(shape, dtype), Metadata(InstrumentMetadata(sizes, metas), {"well": "B2"}))


def test_project_z_plans_the_metadata():
    img = _image("TZCYX", (2, 3, 2, 6, 7))
    plan = _ZPlan(img, "max", None, {})
    assert plan.batch_shape == (4, 3, 6, 7) and plan.out_shape == (2, 2, 6, 7) and plan.z_axis == 1 and plan.source is None
    meta = plan.metadata
    assert list(meta.instrument.sizes.items()) == [("T", 2), ("C", 2), ("Y", 6), ("X", 7)]
    assert meta.sample == {"well": "B2"}
    assert [cm.channel for cm in meta.instrument.channel_metadata_list] == [DAPI, FITC]
    for cm, old in zip(meta.instrument.channel_metadata_list, img.metadata.instrument.channel_metadata_list):
        assert not cm.dimensions.is_zstack and cm.dimensions.is_timelapse
        assert cm.resolution.z_size_px is None and cm.resolution.z_step_um is None
        assert (cm.resolution.xy_step_um, cm.resolution.t_size_px, cm.resolution.t_step_ms) == (0.5, 2, 100.0)
        assert old.dimensions.is_zstack and old.resolution.z_step_um == 1.5  # the source image is left as it was
    assert not meta.instrument.dimensions.is_zstack and meta.instrument.dimensions.is_multichannel
    # the reference channel: stack n = t * 2 + c takes its choice from stack t * 2 + ref
    assert _ZPlan(img, "edf", FITC, {}).source.tolist() == [1, 1, 3, 3]
    assert _ZPlan(img, "best_focus", "DAPI", {}).source.tolist() == [0, 0, 2, 2]
    assert _ZPlan(_image("CZYX"), "edf", "FITC", {"radius": 2, "smooth": 3}).source.tolist() == [1, 1]
    assert _ZPlan(_image("ZYX", (3, 6, 7)), "edf", "DAPI", {}).source is None  # one channel: nothing to share
    plan = _ZPlan(_image("ZYX", (1, 6, 7), resolution=False), "min", None, {})  # Z == 1 works
    assert plan.batch_shape == (1, 1, 6, 7) and plan.out_shape == (6, 7)
    assert plan.metadata.instrument.channel_metadata_list[0].resolution is None


def test_project_z_refuses_before_any_device_access():
    for img in (_image("CYX", (2, 6, 7)), _image("TCYX", (2, 2, 6, 7))):
        with pytest.raises(ValueError, match="no 'Z' axis"):
            img.project_z()
        with pytest.raises(ValueError, match="no 'Z' axis"):
            DeviceImage(_NoDevice(), img).project_z("edf")
    img = _image()
    for bad in ("median", "sum", None):
        with pytest.raises(ValueError, match="method must be one of"):
            img.project_z(bad)
    with pytest.raises(ValueError, match="Channel 'TRITC' not found"):
        img.project_z("edf", reference_channel="TRITC")
    for m in ("max", "min", "mean"):
        with pytest.raises(ValueError, match="reference_channel goes with"):
            img.project_z(m, reference_channel="DAPI")
        with pytest.raises(TypeError, match="takes no argument 'radius'"):
            img.project_z(m, radius=3)
    with pytest.raises(TypeError, match="takes no argument 'focus_method'"):
        img.project_z("edf", focus_method="brenner")
    with pytest.raises(TypeError, match="takes no argument 'smooth'"):
        img.project_z("best_focus", smooth=3)
    with pytest.raises(ValueError, match="radius"):
        img.project_z("edf", radius=16)
    with pytest.raises(ValueError, match="smooth"):
        img.project_z("edf", smooth=4)
    with pytest.raises(ValueError, match="method must be one of"):
        img.project_z("best_focus", focus_method="tenengrad")
    with pytest.raises(ValueError, match="last two axes"):
        _image("CYXZ", (2, 6, 7, 3)).project_z()
    # a device image whose stacks are not contiguous is sent to the host image
    with pytest.raises(NotImplementedError, match="right before"):
        DeviceImage(_NoDevice(), _image("ZCYX", (3, 2, 6, 7))).project_z()
