"""Per-cell Haralick texture without a GPU: the reference (tests/texture_reference.py) is pinned to Haralick's worked
example and to the identities of the definition, the keys and their order, the argument errors that need no device, and
the declared interface."""
import os
import re

import numpy as np
import pytest

import texture_cases as tc
import texture_reference as tr
from arcadia_microscopy_tools_amd import _hip, hipops
from arcadia_microscopy_tools_amd.channels import DAPI, FITC
from arcadia_microscopy_tools_amd.device import DeviceArray
from arcadia_microscopy_tools_amd.masks import SegmentationMask
from arcadia_microscopy_tools_amd.segment import texture_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARALICK = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]])


def test_reference_on_haralicks_worked_example():
    table, counts = tr.texture_stack(np.ones((4, 4), np.int32), HARALICK[None].astype(np.uint16), 1, levels=4, distance=1,
                                     ranges=(0, 4))
    assert counts.dtype == np.uint32 and counts.shape == (1, 1, 4, 4, 4)
    assert counts[0, 0, 0].tolist() == [[4, 2, 1, 0], [2, 4, 0, 0], [1, 0, 6, 1], [0, 0, 1, 2]]
    assert counts[0, 0, 1].tolist() == [[4, 1, 0, 0], [1, 2, 2, 0], [0, 2, 4, 1], [0, 0, 1, 0]]
    assert counts[0, 0, 2].tolist() == [[6, 0, 2, 0], [0, 4, 2, 0], [2, 2, 2, 2], [0, 0, 2, 0]]
    assert counts[0, 0, 3].tolist() == [[2, 1, 3, 0], [1, 2, 1, 0], [3, 1, 0, 2], [0, 0, 2, 0]]
    want = [0.145833, 0.583333, 0.719533, 1.039931, 0.808333, 2.583333, 3.576389, 2.459148, 3.022055, 0.409722, 1.188722,
            -0.427479, 0.898115]
    assert np.abs(table[0, 0, 0] - want).max() <= 1e-6, table[0, 0, 0]
    assert np.array_equal(tr.glcm_loops(np.ones((4, 4), bool), HARALICK, 4, 1), counts[0, 0])


def test_quantisation_edges():
    assert tr.quantise([0, 65535, 32768, 100], 0, 65535, 64).tolist() == [0, 63, 32, 0]
    assert tr.quantise([5, 9, 12], 6, 10, 4).tolist() == [0, 3, 3]
    assert tr.quantise([5, 9, 12], 7, 7, 4).tolist() == [0, 0, 0]      # hi == lo
    assert tr.quantise([5, 9, 12], 9, 7, 4).tolist() == [0, 0, 0]      # hi < lo
    assert tr.quantise(np.array([-3.5, 8.25]), -3.5, 8.25, 8).tolist() == [0, 7]   # a value exactly at hi
    assert tr.quantise(np.array([0, 65535], np.uint16), 0, 65535, 2).dtype == np.int64


@pytest.mark.parametrize("kind", tc.KINDS)
def test_identities_of_the_definition(kind):
    shape = (33, 40)
    for name in ("blobs", "levels_64", "two_pieces", "no_pairs", "checkerboard", "channels_5_ranges"):
        lab, stack, k, p = tc.cases(shape, kind)[name]
        table, counts = tc.reference(shape, kind, name)
        assert table.shape == (k, stack.shape[0], 4, 13) and counts.shape[:3] == (k, stack.shape[0], 4)
        assert np.array_equal(counts, counts.swapaxes(-1, -2))                 # G is symmetric
        assert not (counts.astype(np.int64).sum(axis=(-1, -2)) % 2).any()      # every pair counts twice
        empty = counts.sum(axis=(-1, -2)) == 0
        assert np.array_equal(np.isnan(table).all(axis=-1), empty) and np.array_equal(np.isnan(table).any(axis=-1), empty)
        for c in range(stack.shape[0]):  # the vectorised count equals the pair-by-pair one
            rng = tr.default_ranges(stack) if p["ranges"] is None else np.broadcast_to(p["ranges"], (stack.shape[0], 2))
            q = tr.quantise(stack[c], rng[c, 0], rng[c, 1], p["levels"])
            assert np.array_equal(tr.glcm_loops(lab == 1, q, p["levels"], p["distance"]), counts[0, c])
    # what the cases are there for
    _, counts = tc.reference(shape, kind, "no_pairs")
    assert counts.sum(axis=(-1, -2))[:, 0].tolist() == [[0, 0, 0, 0], [4, 0, 0, 0], [0, 0, 4, 0], [4, 2, 4, 2]]
    assert tc.reference(shape, kind, "distance_beyond_box")[1].sum() == 0
    _, counts = tc.reference(shape, kind, "checkerboard")
    assert (counts.sum(axis=(-1, -2))[:, 0, [0, 2]] == 0).all() and (counts.sum(axis=(-1, -2))[:, 0, [1, 3]] > 0).all()
    _, counts = tc.reference(shape, kind, "two_pieces")
    assert counts[0, 0, 0].sum() == 2 * 33 and counts[1, 0, 0].sum() == 0     # only across the gap; label 2 is 2 wide
    table, counts = tc.reference(shape, kind, "blobs")
    assert np.isnan(table[-1]).all() and counts[-1].sum() == 0                 # the absent label


def test_constant_cell():
    lab = np.ones((6, 9), np.int32)
    table, counts = tr.texture_stack(lab, np.full((1, 6, 9), 40.0), 1, levels=8, distance=1, ranges=(0.0, 64.0))
    assert counts[0, 0, :, 5, 5].tolist() == [2 * 6 * 8, 2 * 5 * 8, 2 * 5 * 9, 2 * 5 * 8] and counts.sum() == counts[0, 0, :, 5, 5].sum()
    for a in range(4):
        assert np.array_equal(table[0, 0, a], [1, 0, 1, 0, 1, 10, 0, 0, 0, 0, 0, 0, 0])
    # sum p = 1 in the large case too, whose diagonal counter is beyond 16 bits
    _, counts = tc.reference(tc.BIG, "u16", "one_constant_label")
    assert counts[0, 0, 0, 6, 6] == 134680 and counts[0, 0, 0].sum() == 134680


def test_mean_over_the_directions_that_have_pairs():
    t = np.full((2, 1, 4, 13), np.nan)
    t[0, 0, 0], t[0, 0, 2] = 1.0, 3.0
    m = tr.nanmean_angles(t)
    assert m.shape == (2, 1, 13) and (m[0] == 2.0).all() and np.isnan(m[1]).all()


def test_keys_and_their_order():
    assert _hip.TEX_COLS == tr.COLS and _hip.TEX_ANGLES == tr.ANGLES == ("0", "45", "90", "135") and _hip.TEX_NCOLS == 13
    keys = texture_keys([FITC, DAPI])
    assert len(keys) == 2 * 4 * 13 and len(set(keys)) == len(keys)
    assert keys[:2] == ["texture_angular_second_moment_fitc_1_0", "texture_contrast_fitc_1_0"]
    assert keys[13] == "texture_angular_second_moment_fitc_1_45" and keys[14] == "texture_contrast_fitc_1_45"
    assert keys[52] == "texture_angular_second_moment_dapi_1_0" and keys[-1] == "texture_info_measure_2_dapi_1_135"
    assert "texture_contrast_dapi_1_45" in keys
    mean = texture_keys(["DAPI"], distance=3, angles="mean")
    assert mean == [f"texture_{f}_dapi_3" for f in tr.COLS]
    with pytest.raises(ValueError, match="angles"):
        texture_keys(["DAPI"], angles="all")
    with pytest.raises(TypeError, match="distance"):
        texture_keys(["DAPI"], distance=1.5)


def test_declared_interface():
    header = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    # the capability rides on amt_regionprops_ext: no entry point of its own
    assert "amt_regionprops_ext" in _hip._SIGS and not [name for name in _hip._SIGS if "texture" in name]
    assert not [name for name in re.findall(r"^int\s+(amt_\w+)\s*\(", header, flags=re.M) if "texture" in name]
    assert re.search(r"#define AMT_RPX_TEXTURE \(1u << 12\)", header) and _hip.RPX_TEXTURE == 1 << 12
    assert re.search(r"#define AMT_RPX_TEXTURE_COUNTS \(1u << 13\)", header) and _hip.RPX_TEXTURE_COUNTS == 1 << 13
    assert re.search(r"#define AMT_RPX_TEXTURE_LEVELS_SHIFT 14\b", header) and _hip.RPX_TEXTURE_LEVELS_SHIFT == 14
    assert re.search(r"#define AMT_RPX_TEXTURE_DISTANCE_SHIFT 21\b", header) and _hip.RPX_TEXTURE_DISTANCE_SHIFT == 21
    assert _hip.rpx_texture_columns(64, 255) == (1 << 12) | (64 << 14) | (255 << 21)
    # the counts call sets bit 13 INSTEAD of bit 12; the fields hold more than the accepted ranges, so 65 and 256 can be
    # stated (and are refused), and the whole stays a positive int
    assert _hip.rpx_texture_columns(127, 1023, True) == (1 << 13) | (127 << 14) | (1023 << 21) < 2 ** 31
    assert not _hip.RPX_TEXTURE & (0xff | _hip.RPX_RELATE | _hip.RPX_ROBUST | _hip.RPX_NEIGHBORS | _hip.RPX_NEAREST)
    for i, name in enumerate(_hip.TEX_COLS):
        assert re.search(rf"#define AMT_TEX_{name.upper()} {i}\b", header), name
    assert re.search(r"#define AMT_TEX_NCOLS 13\b", header) and "parity with that module is unpinned offline" in header
    lib = _hip.load_library()
    # refused before the context is looked at: levels, distance, element type, channels, null operands, other bits
    p = 1 << 24
    cols = _hip.rpx_texture_columns(8, 1)
    ok = [None, p, 2 * p, _hip.U16, 1, cols, 3 * p, 4 * p, 1, 4, 6, 2]
    assert lib.amt_regionprops_ext(*ok) == -1 and lib.amt_last_error() == b"null context"
    assert lib.amt_regionprops_ext(*(ok[:5] + [_hip.rpx_texture_columns(8, 1, True)] + ok[6:])) == -1
    assert lib.amt_last_error() == b"null context"
    for at, bad in ((5, _hip.rpx_texture_columns(1, 1)), (5, _hip.rpx_texture_columns(65, 1)), (5, _hip.rpx_texture_columns(0, 1)),
                    (5, _hip.rpx_texture_columns(8, 0)), (5, _hip.rpx_texture_columns(8, 256)),
                    (5, _hip.rpx_texture_columns(8, 1023, True)), (5, cols | 1), (5, cols | _hip.RPX_ROBUST),
                    (5, cols | _hip.RPX_TEXTURE_COUNTS), (5, cols & ~_hip.RPX_TEXTURE), (3, _hip.U8), (3, _hip.I32), (4, 0),
                    (1, None), (2, None), (6, None), (7, None)):
        args = list(ok)
        args[at] = bad
        assert lib.amt_regionprops_ext(*args) == -1 and lib.amt_last_error() != b"null context", (at, bad)
    args = list(ok)
    args[7] = 3 * p + 8  # the features on the ranges
    assert lib.amt_regionprops_ext(*args) == -1 and b"must not alias" in lib.amt_last_error()
    # the output's length follows the call: 1 x 2 x 1 x 4 x 13 doubles of features, 1 x 2 x 1 x 4 x 8 x 8 uint32 of counts
    args = list(ok)
    args[2] = 4 * p + 832 + 8
    assert lib.amt_regionprops_ext(*args) == -1 and lib.amt_last_error() == b"null context"
    args[5] = _hip.rpx_texture_columns(8, 1, True)
    assert lib.amt_regionprops_ext(*args) == -1 and b"must not alias" in lib.amt_last_error()
    args[2] = 4 * p + 2048
    assert lib.amt_regionprops_ext(*args) == -1 and lib.amt_last_error() == b"null context"


class _NoContext:
    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}): a device call before the refusal")


_CTX = _NoContext()


def _arr(shape, dtype, ptr):
    return DeviceArray(_CTX, ptr, shape, dtype)


def test_argument_errors_of_hipops_need_no_device():
    lab = _arr((7, 5), np.int32, 1 << 20)
    img = _arr((1, 7, 5), np.uint16, 1 << 22)
    with pytest.raises(TypeError, match="int32"):
        hipops.texture(_arr((7, 5), np.uint16, 1 << 20), img, 1)
    for dt in (np.uint8, np.float32):
        with pytest.raises(TypeError):
            hipops.texture(lab, _arr((1, 7, 5), dt, 1 << 22), 1)
    for shape in ((1, 5, 7), (7, 5), (2, 1, 7, 5)):  # other planes, no channel axis, two stacks for one label plane
        with pytest.raises(ValueError):
            hipops.texture(lab, _arr(shape, np.uint16, 1 << 22), 1)
    for bad in (1, 65, 0, -8):
        with pytest.raises(ValueError, match="levels"):
            hipops.texture(lab, img, 1, levels=bad)
    for bad in (0, 256, -1):
        with pytest.raises(ValueError, match="distance"):
            hipops.texture(lab, img, 1, distance=bad)
    for kw in ({"levels": 8.0}, {"levels": True}, {"distance": 1.0}, {"distance": "1"}):
        with pytest.raises(TypeError):
            hipops.texture(lab, img, 1, **kw)
    with pytest.raises(ValueError, match="max_label"):
        hipops.texture(lab, img, -1)
    for bad in ((1.0, 2.0, 3.0), np.zeros((2, 1, 2)), np.zeros((1, 3, 2)), "ab"):
        with pytest.raises(ValueError, match="ranges"):
            hipops.texture(lab, img, 1, ranges=bad)
    with pytest.raises(ValueError, match="device ranges"):
        hipops.texture(lab, img, 1, ranges=_arr((1, 1, 2), np.float32, 1 << 24))
    with pytest.raises(ValueError, match="device ranges"):
        hipops.texture(lab, img, 1, ranges=_arr((1, 2), np.float64, 1 << 24))
    with pytest.raises(TypeError, match="glcm"):
        hipops.texture(lab, img, 1, glcm=np.zeros((1, 1, 1, 4, 8, 8), np.uint32))
    with pytest.raises(ValueError, match="out has shape"):
        hipops.texture(lab, img, 1, out=_arr((1, 1, 1, 4, 12), np.float64, 1 << 24))
    for bad in (_arr((1, 1, 1, 4, 8, 7), np.uint32, 1 << 24), _arr((1, 1, 1, 4, 8, 8), np.int32, 1 << 24)):
        with pytest.raises(ValueError, match="out has shape"):
            hipops.texture(lab, img, 1, glcm=bad)
    # out and glcm are two buffers, each judged against every other operand before any device access
    table, counts = _arr((1, 1, 1, 4, 13), np.float64, 1 << 24), _arr((1, 1, 1, 4, 8, 8), np.uint32, 1 << 26)
    for kw in ({"out": _arr((1, 1, 1, 4, 13), np.float64, (1 << 22) + 8)},           # on the image
               {"glcm": _arr((1, 1, 1, 4, 8, 8), np.uint32, (1 << 20) - 1020)},      # its last word on the labels
               {"out": table, "glcm": _arr((1, 1, 1, 4, 8, 8), np.uint32, (1 << 24) + 408)},   # on the table
               {"out": table, "glcm": counts, "ranges": _arr((1, 1, 2), np.float64, (1 << 26) + 16)}):
        with pytest.raises(ValueError, match="alias"):
            hipops.texture(lab, img, 1, **kw)
    with pytest.raises(AssertionError, match="the context was used"):  # apart: as far as the device
        hipops.texture(lab, img, 1, out=table, glcm=counts)
    with pytest.raises(ValueError, match="hipops.texture"):
        hipops.regionprops_ext(lab, 1, _hip.RPX_TEXTURE)


def test_argument_errors_of_cell_texture_need_no_device():
    nuclei = np.zeros((16, 16), np.int64)
    nuclei[2:9, 3:11] = 1
    images = {DAPI: np.arange(256, dtype=np.uint16).reshape(16, 16)}
    with pytest.raises(ValueError, match="intensity images"):
        SegmentationMask(nuclei, remove_edge_cells=False).cell_texture()
    mask = SegmentationMask(nuclei, images, remove_edge_cells=False)
    with pytest.raises(ValueError, match="angles"):
        mask.cell_texture(angles="both")
    with pytest.raises(ValueError, match="levels"):
        mask.cell_texture(levels=1)
    with pytest.raises(ValueError, match="levels"):
        mask.cell_texture(levels=65)
    with pytest.raises(ValueError, match="distance"):
        mask.cell_texture(distance=0)
    with pytest.raises(TypeError, match="distance"):
        mask.cell_texture(distance=2.0)
    with pytest.raises(TypeError, match="pair"):
        mask.cell_texture(ranges=5.0)
    with pytest.raises(TypeError, match="pair"):
        mask.cell_texture(ranges=(1, 2, 3))
    with pytest.raises(ValueError, match="no intensity image"):
        mask.cell_texture(ranges={FITC: (0, 1)})
    with pytest.raises(TypeError, match="pair"):
        mask.cell_texture(ranges={DAPI: 7})
