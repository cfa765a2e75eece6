"""``binary_fill_holes`` without a GPU: the C ABI's new operation code, the Python interface's validation (before any
device call), and the test-side reference itself -- every generator of tests/fill_holes_reference.py has its stated
property under scipy, and the component rule the device implements equals scipy on every shape."""
import os
import re

import numpy as np
import pytest

import fill_holes_reference as ref
from arcadia_microscopy_tools_amd import hipops, operations
from arcadia_microscopy_tools_amd.model import SegmentationModel
from arcadia_microscopy_tools_amd.pipeline import is_device_operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = [s for s in ref.SHAPES if s[0] >= 3 and s[1] >= 3]


def test_header_defines_and_documents_the_code():
    text = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    assert re.search(r"^#define\s+AMT_MORPH_FILL_HOLES\s+4\s*$", text, re.M)
    block = text[:text.index("int amt_binary_morph(")]
    block = block[block.rindex("/* Footprint"):]
    for word in ("AMT_MORPH_FILL_HOLES", "binary_fill_holes", "4-connected", "8-connected", "frame", "alias", "AMT_EINVAL"):
        assert word in block, word


def test_python_interface_exists():
    assert hipops._MORPH_OPS["fill_holes"] == 4
    assert {k: hipops._MORPH_OPS[k] for k in ("erode", "dilate", "open", "close")} == {"erode": 0, "dilate": 1, "open": 2,
                                                                                     "close": 3}
    assert callable(hipops.binary_fill_holes)
    assert callable(operations.binary_fill_holes) and is_device_operator(operations.binary_fill_holes)


class _NoDevice:
    """Stands where a DeviceArray would: any attribute access means validation did not come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the array was touched ({name}) before the structure was validated")


@pytest.mark.parametrize("structure", [np.ones((3, 5)), np.ones((5, 5)), np.eye(3), np.zeros((3, 3)), np.ones(3),
                                       [[0, 1, 0], [1, 1, 1], [0, 1, 1]], [[1, 1, 1], [1, 0, 1], [1, 1, 1]]])
def test_other_structures_are_refused_before_any_device_call(structure):
    with pytest.raises(ValueError, match="structure"):
        hipops.binary_fill_holes(_NoDevice(), structure)
    with pytest.raises(ValueError, match="structure"):
        operations.binary_fill_holes(np.zeros((4, 4), bool), structure)


def test_accepted_structures():
    assert np.array_equal(hipops._fill_structure(None), ref.CROSS)
    assert np.array_equal(hipops._fill_structure(ref.CROSS.astype(bool)), ref.CROSS)
    assert np.array_equal(hipops._fill_structure(ref.CROSS * 7.5), ref.CROSS)  # the != 0 pattern counts
    assert np.array_equal(hipops._fill_structure(np.full((3, 3), -2)), ref.FULL)


def test_stacks_and_dtypes_are_refused_before_any_device_call():
    with pytest.raises(ValueError, match="must be a 2D array"):
        operations.binary_fill_holes(np.zeros((2, 4, 4), bool))
    with pytest.raises(ValueError, match="must be a 2D array"):
        operations.binary_fill_holes(np.zeros(5, bool))
    with pytest.raises(TypeError):
        operations.binary_fill_holes(np.zeros((4, 4), np.float64))


def test_empty_array_gives_an_empty_bool_array():
    for shape in ((0, 5), (3, 0), (0, 0)):
        out = operations.binary_fill_holes(np.zeros(shape, np.uint8))
        assert out.shape == shape and out.dtype == np.bool_


def test_model_field():
    with pytest.raises(ValueError, match="fill_holes"):
        SegmentationModel(backend="cellpose", fill_holes=True)
    with pytest.raises(ValueError, match="fill_holes"):
        SegmentationModel(backend="cellpose-hip", network="standin", fill_holes=True)
    assert SegmentationModel(backend="classical").fill_holes is False
    assert SegmentationModel(backend="classical", fill_holes=True).fill_holes is True
    import dataclasses

    names = [f.name for f in dataclasses.fields(SegmentationModel) if f.init]
    assert names[-2:] == ["compute_dtype", "fill_holes"]


# ---- the reference itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_component_rule_equals_scipy(shape):
    for name, plane in ref.planes(shape):
        for sname, st in ref.STRUCTURES:
            assert np.array_equal(ref.component_fill(plane, st), ref.scipy_fill(plane, st)), (shape, name, sname)


def test_random_planes_hold_holes():
    """A condition on the inputs: a device that copied its input would fail on most random planes."""
    with_hole = total = 0
    for shape in ref.SHAPES:
        for i, seed in enumerate(ref.SEEDS):
            p = ref.random(shape, ref.DENSITIES[i], seed)
            assert 0.5 <= ref.DENSITIES[i] <= 0.8
            total += 1
            with_hole += not np.array_equal(ref.scipy_fill(p, ref.CROSS), p)
    print(f"{with_hole} of {total} random planes hold a hole")
    assert total == 51 and 2 * with_hole >= total


def test_checkerboard_counts():
    p = ref.checkerboard((9, 9))
    assert int(ref.scipy_fill(p, ref.CROSS).sum()) == 65 and int(ref.scipy_fill(p, ref.FULL).sum()) == 41
    for shape in BIG:
        p = ref.checkerboard(shape)
        want = p.copy()
        want[1:-1, 1:-1] = 1  # every interior background pixel is its own hole
        assert np.array_equal(ref.scipy_fill(p, ref.CROSS), want), shape
        assert np.array_equal(ref.scipy_fill(p, ref.FULL), p), shape
    row = ref.checkerboard((64, 64))[1]
    assert int(((1 - row)[1:] > (1 - row)[:-1]).sum()) + int(1 - row[0]) == 32  # complement runs of a 64-pixel row


def test_simple_generators():
    for shape in ref.SHAPES:
        for _, st in ref.STRUCTURES:
            assert not ref.scipy_fill(ref.all_zero(shape), st).any()
            assert ref.scipy_fill(ref.all_one(shape), st).all()
            assert np.array_equal(ref.scipy_fill(ref.stripes_1px(shape), st), ref.stripes_1px(shape))
            f = ref.frame_only(shape)
            if shape[0] >= 3 and shape[1] >= 3:
                assert not f.all() and ref.scipy_fill(f, st).all()
            else:
                assert f.all()


def test_spiral_flips_with_its_mouth():
    assert (256, 256) in ref.SPIRAL_SHAPES
    for shape in ref.SPIRAL_SHAPES:
        opened, closed = ref.spiral(shape, True), ref.spiral(shape, False)
        assert opened[1, 0] == 0 and closed[1, 0] == 1 and int((opened != closed).sum()) == 1
        corridor = int((opened == 0).sum())
        assert corridor >= (shape[0] * shape[1]) // 4, (shape, corridor)  # it winds through the whole plane
        lab, k = ref.ndi.label(opened == 0, structure=ref.CROSS)
        assert k == 1  # one corridor
        for _, st in ref.STRUCTURES:
            assert np.array_equal(ref.scipy_fill(opened, st), opened), shape
            assert ref.scipy_fill(closed, st).all(), shape


def test_nested_diagonal_corner_row1_seams():
    for shape in ref.SHAPES:
        p = ref.nested(shape)
        if p is not None:
            assert int((p == 0)[1:-1, 1:-1].sum()) > 0
            for _, st in ref.STRUCTURES:
                assert np.array_equal(ref.scipy_fill(p, st), ref.nested_solid(shape)), shape
        p = ref.diagonal_leak(shape)
        if p is not None:
            want = np.ones(shape, np.uint8)
            want[0, 0] = 0
            assert np.array_equal(ref.scipy_fill(p, ref.CROSS), want), shape
            assert np.array_equal(ref.scipy_fill(p, ref.FULL), p), shape
        p = ref.corner_touch(shape)
        if p is not None:
            want = np.ones(shape, np.uint8)
            want[-1, -1] = 0
            assert np.array_equal(ref.scipy_fill(p, ref.CROSS), want), shape
            assert np.array_equal(ref.scipy_fill(p, ref.FULL), p), shape
            lab, _ = ref.ndi.label(p == 0, structure=ref.FULL)
            comp = lab == lab[-1, -1]
            frame = np.ones(shape, bool)
            frame[1:-1, 1:-1] = False
            assert int((comp & frame).sum()) == 1  # its only frame pixel is the corner
        p = ref.row1_hole(shape)
        if p is not None:
            assert p[0].all() and not p[1].all()
            for _, st in ref.STRUCTURES:
                assert ref.scipy_fill(p, st).all(), shape
        p = ref.seam_holes(shape)
        if p is not None:
            for _, st in ref.STRUCTURES:
                assert np.array_equal(ref.scipy_fill(p, st), ref.seam_bay(shape)), shape
    assert int(ref.scipy_fill(ref.diagonal_leak((5, 5)), ref.CROSS).sum()) == 24
    assert int(ref.scipy_fill(ref.diagonal_leak((5, 5)), ref.FULL).sum()) == 22
    p = ref.seam_holes((70, 131))
    assert not p[67:69, 62:66].any() and not p[62:66, 1:3].any() and not p[35, 127:130].any()
    assert p[63, 63] == 0 and p[64, 64] == 0


def test_truth_bytes_keep_the_pattern():
    p = ref.random((33, 40), 0.6, 1)
    t = ref.truth_bytes(p, 3)
    assert np.array_equal(t != 0, p != 0) and set(np.unique(t)) == {0, 1, 2, 255}


def test_annuli_field_needs_the_fill():
    fov, centres = ref.annuli_field()
    assert fov.shape == (4, 256, 256) and fov.dtype == np.uint16 and len(centres) == 12
    assert all(14 <= r <= 18 for _, _, r in centres)
    rings = fov[1] > 4000
    filled = ref.scipy_fill(rings, ref.CROSS)
    lab, k = ref.ndi.label(filled)
    assert k == 12 and int(filled.sum()) > int(rings.sum()) + 12 * 100  # twelve discs, each with a centre to fill
