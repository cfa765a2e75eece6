"""Per-cell skeletons without a GPU: the two test-side statements of the rule against each other on the whole case table,
the header's statement of the rule and the codes, every refusal of the C ABI that needs no device (null context), and the
Python layers' argument errors before any device access.  Parity with scikit-image or CellProfiler is unpinned offline:
nothing here claims it."""
import os
import re

import numpy as np
import pytest

import label_skeleton_cases as cases
import label_skeleton_reference as ref
import skeleton_reference as binary
from arcadia_microscopy_tools_amd import _hip, hipops, operations, segment
from arcadia_microscopy_tools_amd.device import DeviceArray
from arcadia_microscopy_tools_amd.masks import SegmentationMask
from arcadia_microscopy_tools_amd.pipeline import is_device_operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "amt_hip.h")).read()


# ---- the two references ---------------------------------------------------------------------------------------------------
def test_the_label_rule_equals_every_label_alone():
    """(a) the label-aware rule == (b) the binary rule on labels == l per label, merged: planes and iteration counts"""
    for case in cases.skeleton_cases():
        name, k, stack, names = case
        got, its = cases.skeleton_reference(case)
        assert got.dtype == np.int32 and got.shape == stack.shape
        for i, plane in enumerate(stack):
            alone, n = ref.skeletonize_isolated(plane, k)
            assert np.array_equal(got[i], alone), (name, names[i])
            assert its[i] == n, (name, names[i], its[i], n)


def test_reference_gives_the_hand_results():
    two = np.zeros((6, 8), np.int32)
    two[1:5, 1:4], two[1:5, 4:7] = 1, -9  # two 4 x 3 blocks side by side: each thins as if alone
    out, n = ref.skeletonize(two)
    for block, value in ((two == 1), 1), ((two == -9), -9):
        alone = binary.skeletonize(block)[0]
        assert np.array_equal(out == value, alone != 0) and 0 < alone.sum() < block.sum()
    assert out.dtype == np.int32 and n == max(binary.skeletonize(two == 1)[1], binary.skeletonize(two == -9)[1])
    seven = np.full((33, 40), 7, np.int32)
    out, n = ref.skeletonize(seven)
    assert np.array_equal(out, 7 * binary.skeletonize(seven)[0]) and n == 17
    out, n = ref.skeletonize(np.zeros((4, 5), np.int32))
    assert not out.any() and n == 1
    assert np.array_equal(ref.census(cases.l_and_staircase(), 3), cases.HAND_TABLE)
    full = ref.census(np.ones((4, 5), np.int32), 2)
    assert full.tolist() == [[20, 0, 0, 0, 20, 4 * 4 + 3 * 5, 0], [0] * 7]  # deg >= 3 everywhere, no unbridged diagonal
    assert ref.census(np.ones((5, 5), np.int32), 1)[0, 4] == 25
    lone = np.zeros((3, 3), np.int32)
    lone[1, 1] = 2
    assert ref.census(lone, 2).tolist() == [[0] * 7, [1, 1, 0, 0, 0, 0, 0]]
    assert ref.census(lone, 1).tolist() == [[0] * 7] and ref.census(lone, 0).shape == (0, 7)


def test_the_table_is_not_vacuous():
    differs = 0
    for case in cases.skeleton_cases():
        if not case[0].startswith("contents"):
            continue
        got = cases.skeleton_reference(case)[0]
        for i, plane in enumerate(case[2]):
            differs += not np.array_equal(got[i] != 0, binary.skeletonize(plane != 0)[0] != 0)
    assert differs > 20  # touching cells do not share a skeleton
    rich = [c for c in cases.census_cases()
            if (cases.census_reference(c)[..., [2, 4, 6]].sum(axis=(0, 1)) > 0).all()]
    assert rich, "no census case has ends, junctions and diagonal links"
    assert any((cases.census_reference(c)[..., 4] == c[2].shape[1] * c[2].shape[2]).any() for c in cases.census_cases())


def test_case_table_covers_the_seams():
    rows, words, T = hipops.label_skeleton_block()
    assert (rows, words, T) == (cases.ROWS, cases.WORDS, cases.T)
    assert T % 2 == 0 and 2 <= T <= 64
    assert {s[1] for s in cases.SHAPES} == {1, 2, 63, 64, 65, 127, 128, 129, 64 * words - 1, 64 * words + 1}
    assert {s[0] for s in cases.SHAPES} == {1, 2, 3, rows - 1, rows + 1, 2 * rows + 1}
    assert cases.HALF_THICK == 2 * T + 6 and cases.BAR_WIDE > 2 * 64 * words
    assert cases.bar_iterations() > T // 2  # more sub-iterations than one launch runs
    assert {1, T // 2, T // 2 + 2, cases.bar_iterations() - 1, cases.bar_iterations() + 1} <= set(cases.max_iter_values())
    names = [c[0] for c in cases.skeleton_cases()] + [c[0] for c in cases.census_cases()]
    assert len(names) == len(set(names))
    batch = next(c for c in cases.skeleton_cases() if c[0] == "batch of three")
    counts = cases.skeleton_reference(batch)[1]
    assert counts[0] == 1 and counts[1] < counts[2] == cases.bar_iterations()
    values = {int(v) for c in cases.skeleton_cases() for v in np.unique(c[2])}
    assert set(cases.EXOTIC) <= values and min(values) < 0
    for c in cases.census_cases():  # below, at and above the largest label
        if c[0].startswith("census of contents 65 x 129"):
            assert c[1] in (11, 12, 14)


# ---- the header and the codes -----------------------------------------------------------------------------------------------
def test_header_defines_and_documents_the_codes():
    for name, value in (("AMT_RANK_LABEL_SKELETON", 8), ("AMT_RANK_LABEL_CENSUS", 9), ("AMT_LCEN_NCOLS", 7),
                        ("AMT_LABEL_SKELETON_TILE_ROWS", _hip.LABEL_SKELETON_TILE_ROWS),
                        ("AMT_LABEL_SKELETON_TILE_WORDS", _hip.LABEL_SKELETON_TILE_WORDS),
                        ("AMT_LABEL_SKELETON_BLOCK_SUBITERS", _hip.LABEL_SKELETON_BLOCK_SUBITERS)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", HEADER, re.M), name
    for i, col in enumerate(_hip.LCEN_COLS):
        assert re.search(rf"^#define\s+AMT_LCEN_{col.upper()}\s+{i}\s*$", HEADER, re.M), col
    block = HEADER[:HEADER.index("int amt_rank_filter(")]
    block = block[block.rindex("/* grey erosion"):]
    for word in ("AMT_RANK_LABEL_SKELETON", "AMT_RANK_LABEL_CENSUS", "same label", "max_iter", "waits for the device",
                 "DIAG_LINKS", "ORTH_LINKS", "unpinned offline", "AMT_I32", "negative ones included", "AMT_EINVAL",
                 "nplanes == 0", "2^31 - 1", "65535", "AMT_DEBUG_SKELETONIZE", "row l - 1", "seven zeros",
                 "AMT_MORPH_SKELETONIZE", "never set"):
        assert word in block, word


def test_python_constants_agree_with_the_header():
    assert (_hip.RANK_LABEL_SKELETON, _hip.RANK_LABEL_CENSUS) == (8, 9)
    assert _hip.LCEN_COLS == ref.LCEN_COLS and _hip.LCEN_NCOLS == 7
    assert hipops.label_skeleton_block() == (_hip.LABEL_SKELETON_TILE_ROWS, _hip.LABEL_SKELETON_TILE_WORDS,
                                             _hip.LABEL_SKELETON_BLOCK_SUBITERS)
    for name in ("label_skeleton", "label_census", "label_skeleton_block"):
        assert callable(getattr(hipops, name))
    assert is_device_operator(operations.skeletonize_labels)
    for doc in (hipops.label_skeleton.__doc__, operations.skeletonize_labels.__doc__, SegmentationMask.cell_skeleton.__doc__):
        assert "unpinned" in doc and "offline" in doc


def test_prototypes_are_unchanged():
    """The capability rides on amt_rank_filter: the C ABI has the names it had."""
    bare = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    names = re.findall(r"^(?:int|const char\s*\*)\s*(amt_\w+)\s*\(", bare, flags=re.M)
    assert len(names) == len(set(names)) == len(_hip._SIGS) and set(names) == set(_hip._SIGS)
    assert not [n for n in names if "skelet" in n or "census" in n]
    lib = _hip.load_library()
    for hidden in ("amt_label_skeleton", "amt_label_census"):
        assert not hasattr(lib, hidden)


# ---- the C ABI with a null context --------------------------------------------------------------------------------------------
_BUF = np.zeros(1 << 16, np.uint8)
_A = (_BUF.ctypes.data + 255) & ~255  # room for two 4 x 4 x 3 int32 planes and a table, far apart
_B = _A + (1 << 15)
FULL = np.ones((3, 3), np.uint8)


def _call(op, *, dtype=_hip.I32, fp=FULL, mode=0, inp=None, out=None, minuend=None, H=4, W=4, nplanes=1):
    lib = _hip.load_library()
    fp = np.ascontiguousarray(fp, np.uint8)
    rc = lib.amt_rank_filter(None, _A if inp is None else inp, _B if out is None else out, dtype, nplanes, H, W,
                             fp.ctypes.data, fp.shape[0], fp.shape[1], op, mode, 0.0, minuend)
    return rc, lib.amt_last_error().decode()


def test_complete_calls_reach_the_context():
    for mode in (0, 1, 7, 2**31 - 1):
        assert _call(8, mode=mode) == (-1, "null context")
    for mode in (0, 1, 12, 1000):
        assert _call(9, mode=mode) == (-1, "null context")
    for op in (8, 9):
        assert _call(op, nplanes=0) == (-1, "null context")
        assert _call(op, fp=FULL * 5) == (-1, "null context")  # a truth value per cell
        assert _call(op, nplanes=3, mode=2) == (-1, "null context")


@pytest.mark.parametrize("op", [8, 9])
def test_refusals_need_no_device(op):
    for dtype in (_hip.U8, _hip.U16, _hip.F64, _hip.F32, _hip.I64):
        code, msg = _call(op, dtype=dtype)
        assert code == -1 and "dtype" in msg and "AMT_I32" in msg and "null context" not in msg, msg
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
    for fp in (np.ones((3, 5)), np.ones((5, 5)), np.eye(3), np.zeros((3, 3)), np.ones((1, 1)), cross,
               [[0, 1, 0], [1, 1, 1], [0, 1, 1]], [[1, 1, 1], [1, 0, 1], [1, 1, 1]]):
        code, msg = _call(op, fp=fp)
        assert code == -1 and "footprint" in msg and "null context" not in msg, msg
    for bad in (-1, -7, -2**31):
        code, msg = _call(op, mode=bad)
        assert code == -1 and ("max_iter" if op == 8 else "max_label") in msg and "null context" not in msg, msg
    code, msg = _call(op, minuend=_A + 8192)
    assert code == -1 and "minuend" in msg and "null context" not in msg, msg
    code, msg = _call(op, H=65536, W=32768, inp=1 << 40, out=3 << 40, mode=1)
    assert code == -1 and "plane too large" in msg, msg
    code, msg = _call(op, nplanes=65536, mode=1, inp=1 << 40, out=3 << 40)
    assert code == -1 and "65535" in msg, msg


def test_aliasing_is_refused_with_the_span_each_op_has():
    plane = 4 * 4 * 4
    for s in (0, 8, plane, -plane):  # exactly, shifted by 8 bytes, by one plane
        code, msg = _call(8, nplanes=3, out=_A + s)
        assert code == -1 and "alias" in msg and msg.startswith("amt_rank_filter: "), (s, msg)
    for s in (3 * plane, -3 * plane):  # neighbours that touch
        assert _call(8, nplanes=3, out=_A + s) == (-1, "null context")
    # op 9: `out` is the table of nplanes x max_label x 7 int32, not a plane
    table = 3 * 5 * 7 * 4
    for s in (0, 8, 3 * plane - 4, -(table - 4)):
        code, msg = _call(9, nplanes=3, mode=5, out=_A + s)
        assert code == -1 and "alias" in msg, (s, msg)
    assert _call(9, nplanes=3, mode=5, out=_A + 3 * plane) == (-1, "null context")  # right behind its planes
    assert _call(9, nplanes=3, mode=5, out=_A - table) == (-1, "null context")  # right in front of them
    # a table longer than the planes, which begins in front of them and ends inside them
    big = 3 * 100 * 7 * 4
    assert big > 3 * plane
    code, msg = _call(9, nplanes=3, mode=100, out=_A - big + 4)
    assert code == -1 and "alias" in msg, msg
    # a plane-sized view of `out` would have called this apart: one row of the table is all that the planes' span leaves
    assert _call(9, nplanes=3, mode=100, out=_A - big) == (-1, "null context")
    # max_label 0 writes nothing: no operand
    assert _call(9, nplanes=3, mode=0, out=_A) == (-1, "null context")
    # the line about the minuend stays first
    code, msg = _call(8, out=_B, minuend=_B)
    assert code == -1 and "differ from out" in msg, msg


def test_the_filter_ops_keep_their_answers():
    for op in (0, 1, 2, 7, -1):
        assert _call(op, dtype=_hip.U16) == (-1, "null context")
    for op in (3, 4):  # and the reconstructions theirs
        assert _call(op, dtype=_hip.U16, minuend=_A + 8192) == (-1, "null context")


# ---- the Python layers' argument errors ---------------------------------------------------------------------------------------
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


def test_scalar_errors_come_before_any_device_access():
    for bad in (1.5, "3", None, [2], 2.0):
        with pytest.raises(TypeError, match="max_iter"):
            hipops.label_skeleton(_NoDevice(), bad)
        with pytest.raises(TypeError, match="max_label"):
            hipops.label_census(_NoDevice(), bad)
    for bad in (True, False, np.True_):
        with pytest.raises(TypeError, match="bool"):
            hipops.label_skeleton(_NoDevice(), bad)
        with pytest.raises(TypeError, match="bool"):
            hipops.label_census(_NoDevice(), bad)
        with pytest.raises(TypeError, match="bool"):
            operations.skeletonize_labels(_NoDevice(), bad)
    for bad in (-1, -100, np.int64(-2), 2**31):
        with pytest.raises(ValueError, match="max_iter"):
            hipops.label_skeleton(_NoDevice(), bad)
        with pytest.raises(ValueError, match="max_label"):
            hipops.label_census(_NoDevice(), bad)
    for bad in (0, -1):  # the operator spells "no limit" as None
        with pytest.raises(ValueError, match="max_iter"):
            operations.skeletonize_labels(_NoDevice(), bad)
        with pytest.raises(ValueError, match="max_iter"):
            operations.skeletonize_labels(np.ones((4, 4), np.int32), max_iter=bad)
    for bad in (1.5, "3", 2.0):
        with pytest.raises(TypeError, match="max_iter"):
            operations.skeletonize_labels(np.ones((4, 4), np.int32), bad)


def test_array_errors_come_before_any_device_access():
    for dtype in (np.uint8, np.uint16, np.float64, np.float32, np.int64):
        with pytest.raises(TypeError, match="int32"):
            hipops.label_skeleton(_HostOnly((8, 8), dtype))
        with pytest.raises(TypeError, match="int32"):
            hipops.label_census(_HostOnly((8, 8), dtype), 3)
    for shape in ((2, 2, 8, 8), (8,)):
        with pytest.raises(ValueError, match="label planes"):
            hipops.label_skeleton(_HostOnly(shape, np.int32))
        with pytest.raises(ValueError, match="label planes"):
            hipops.label_census(_HostOnly(shape, np.int32), 3)
    a = _HostOnly((8, 8), np.int32)
    with pytest.raises(ValueError, match="alias"):
        hipops.label_skeleton(a, out=a)
    for wrong in (_HostOnly((8, 9), np.int32, ptr=8192), _HostOnly((8, 8), np.uint8, ptr=8192),
                  _HostOnly((1, 8, 8), np.int32, ptr=8192)):
        with pytest.raises(ValueError, match="out has shape"):
            hipops.label_skeleton(a, out=wrong)
    for wrong in (_HostOnly((1, 3, 6), np.int32, ptr=8192), _HostOnly((1, 3, 7), np.float64, ptr=8192),
                  _HostOnly((3, 7), np.int32, ptr=8192), _HostOnly((1, 4, 7), np.int32, ptr=8192)):
        with pytest.raises(ValueError, match="out has shape"):
            hipops.label_census(a, 3, out=wrong)
    lo, hi = _HostOnly((2, 8, 8), np.int32, ptr=4096), _HostOnly((2, 8, 8), np.int32, ptr=4096 + 256)
    for x, o in ((lo, hi), (hi, lo), (lo, _HostOnly((2, 8, 8), np.int32, ptr=4096 + 8))):
        with pytest.raises(ValueError, match="alias"):
            hipops.label_skeleton(x, out=o)
    for ptr in (4096, 4096 + 8, 4096 + 2 * 256 - 4, 4096 - 2 * 3 * 7 * 4 + 4):
        with pytest.raises(ValueError, match="alias"):
            hipops.label_census(lo, 3, out=_HostOnly((2, 3, 7), np.int32, ptr=ptr))
    for ptr in (4096 + 2 * 256, 4096 - 2 * 3 * 7 * 4):  # neighbours that touch: as far as the device call
        with pytest.raises(AssertionError, match="the context was used"):
            hipops.label_census(lo, 3, out=_HostOnly((2, 3, 7), np.int32, ptr=ptr))
    with pytest.raises(AssertionError, match="the context was used"):
        hipops.label_skeleton(lo, out=_HostOnly((2, 8, 8), np.int32, ptr=4096 + 2 * 256))


def test_operator_errors_come_before_any_device_access():
    op = operations.skeletonize_labels
    for bad in (np.zeros((4, 4), bool), _bool_device()):
        with pytest.raises(TypeError, match="use skeletonize"):
            op(bad)
    for dtype in (np.float64, np.float32):
        with pytest.raises(TypeError, match="integer dtype"):
            op(np.zeros((4, 4), dtype))
        with pytest.raises(TypeError, match="int32, uint16 or uint8"):
            op(_HostOnly((4, 4), dtype))
    for shape in ((2, 4, 4), (5,), (1, 2, 4, 4)):
        with pytest.raises(ValueError, match="must be a 2D array"):
            op(np.zeros(shape, np.int32))
        with pytest.raises(ValueError, match="must be a 2D array"):
            op(_HostOnly(shape, np.int32))
    with pytest.raises(ValueError, match="fit int32"):
        op(np.full((3, 3), 2**31, np.int64))
    with pytest.raises(ValueError, match="fit int32"):
        op(np.full((3, 3), 2**32 - 1, np.uint32))
    for shape in ((0, 5), (3, 0)):
        for dtype in (np.int64, np.uint16):
            out = op(np.zeros(shape, dtype))
            assert out.shape == shape and out.dtype == dtype


def _bool_device():
    d = _HostOnly((4, 4), np.uint8)
    d.is_bool = True
    return d


def test_skeleton_keys():
    keys = segment.skeleton_keys()
    assert keys == ["skeleton_pixels", "skeleton_isolated", "skeleton_ends", "skeleton_path_pixels",
                    "skeleton_junction_pixels", "skeleton_length"]
    lab = cases.voronoi((40, 50), 6, 3)
    want, skel = ref.cell_skeleton(lab, 6)
    assert list(want) == keys and np.array_equal(skel, ref.skeletonize(lab)[0])
    assert all(want[k].dtype == np.int64 and want[k].shape == (6,) for k in keys[:5])
    assert want["skeleton_length"].dtype == np.float64
    assert want["skeleton_pixels"].sum() == np.count_nonzero(skel)
    assert callable(SegmentationMask.cell_skeleton) and callable(SegmentationMask.skeleton_image)
