"""Per-cell radial distribution without a GPU: the reference (tests/radial_reference.py) against a hand-worked example and
the properties the case table (tests/radial_cases.py) is there for, the keys, the declared interface and the argument
errors that need no device."""
import math
import os
import re

import numpy as np
import pytest

import radial_cases as rc
import radial_reference as rr
from arcadia_microscopy_tools_amd import _hip, hipops
from arcadia_microscopy_tools_amd.channels import DAPI, FITC
from arcadia_microscopy_tools_amd.device import DeviceArray
from arcadia_microscopy_tools_amd.masks import SegmentationMask
from arcadia_microscopy_tools_amd.segment import radial_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_on_a_hand_worked_example():
    """A cell that fills a 5 x 5 plane, three rings, the channel v = x^2.  Distances to the frame: 1 on the rim, 2 on the
    inner 3 x 3, 3 in the middle, so dmax2 = 9 and the rings hold 1, 8 and 16 pixels; the ring sums are 4, 38 and 108 of
    150.  Ring 1 (the eight pixels around the centre) has six wedges with the means 1, 1, 9, 9, 4, 4: mu = 14 / 3,
    var = 98 / 9, cv = 1 / sqrt(2)."""
    lab = np.ones((5, 5), np.int32)
    ys, xs, d2 = rr.distances(lab, 1)
    assert d2.reshape(5, 5).tolist() == [[1, 1, 1, 1, 1], [1, 4, 4, 4, 1], [1, 4, 9, 4, 1], [1, 4, 4, 4, 1], [1, 1, 1, 1, 1]]
    assert rr.rings(d2, 3).reshape(5, 5).tolist() == [[2, 2, 2, 2, 2], [2, 1, 1, 1, 2], [2, 1, 0, 1, 2], [2, 1, 1, 1, 2],
                                                        [2, 2, 2, 2, 2]]
    assert rr.wedges(ys, xs).reshape(5, 5)[1:4, 1:4].tolist() == [[0, 4, 2], [0, 0, 2], [1, 5, 3]]
    v = (np.arange(5) ** 2)[None, :].repeat(5, axis=0).astype(np.uint16)
    geom, table = rr.radial_stack(lab, v[None], 1, bins=3)
    assert geom.shape == (1, rr.GEOM_NCOLS) and table.shape == (1, 1, 3, 3)
    assert geom[0].tolist() == [3.0, 1.4] + [1.0, 8.0, 16.0] + [0.0] * 13
    assert table[0, 0, :, 0].tolist() == [4 / 150, 38 / 150, 108 / 150]
    assert table[0, 0, :, 1].tolist() == [(4 / 150) / (1 / 25), (38 / 150) / (8 / 25), (108 / 150) / (16 / 25)]
    assert table[0, 0, 0, 2] == 0.0 and abs(table[0, 0, 1, 2] - 1 / math.sqrt(2)) <= 1e-15
    # the float64 stack goes the same way
    geom64, table64 = rr.radial_stack(lab, v[None].astype(np.float64), 1, bins=3)
    assert geom64.tobytes() == geom.tobytes() and np.allclose(table64, table, rtol=1e-15, atol=0)
    # no intensity: the geometry alone; an absent label: NaN radii, zero counts, NaN columns
    g0, t0 = rr.radial_stack(lab, None, 2, bins=3)
    assert t0 is None and g0[0].tobytes() == geom[0].tobytes()
    assert np.isnan(g0[1, :2]).all() and not g0[1, 2:].any()
    assert np.isnan(rr.radial_stack(lab, v[None], 2, bins=3)[1][1]).all()


def test_what_the_cases_are_there_for():
    cases = rc.cases()
    # the neighbour counts as outside: the rows equal those of the same shape with background in its place
    a, b = rc.reference("shared_edge"), rc.reference("shared_edge_alone")
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[1][0].tobytes() == b[1][0].tobytes()
    assert a[0][0, 0] == 3.0  # five wide: the middle column is 3 from either side
    # a gap and a hole are outside
    assert rc.reference("two_pieces")[0][0, 0] == 3.0 and rc.reference("hole")[0][0, 0] == 2.0
    assert rc.reference("single_pixel")[0][0, :2].tolist() == [1.0, 1.0]
    assert rc.reference("fills_plane")[0][0, 0] == 3.0  # 7 x 5: the frame is the edge
    # the U: a pixel whose nearest outside pixel is in neither its row nor its column
    lab = cases["u_shape"]["lab"]
    ys, xs, d2 = rr.distances(lab, 1)
    at = int(np.nonzero((ys == 8) & (xs == 4))[0][0])
    row = min(abs(4 - x) for x in range(-1, 14) if x in (-1, 13) or lab[8, x] != 1)
    col = min(abs(8 - y) for y in range(-1, 13) if y in (-1, 12) or lab[y, 4] != 1)
    assert d2[at] == 8 < min(row * row, col * col)
    # widths and heights on both sides of every layout switch, boxes on both sides of the tier
    for w in rc.WIDTHS:
        xs = np.nonzero(cases[f"width_{w}"]["lab"])[1]
        assert xs.max() - xs.min() + 1 == w
    ys = np.nonzero(cases["tall_65x3"]["lab"])[0]
    assert ys.max() - ys.min() + 1 == 65
    tile = rc.lds_tile()
    for name, inside in (("disk_tier_in", True), ("disk_tier_out", False), ("full_scale_square", True),
                         ("full_scale_square_plus", False)):
        ys, xs = np.nonzero(cases[name]["lab"])
        cells = (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1)
        assert (cells <= tile) == inside, (name, cells)
    both = cases["tier_out_touching"]["lab"]
    assert (both > 0).all() and (both == 1).sum() == (both == 2).sum() > tile
    ys, xs = np.nonzero(cases["full_scale_square"]["lab"])
    assert (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1) == tile and cases["full_scale_square"]["stack"].min() == 65535
    # absent rows, every bins and channel count
    for bins in (1, 4, 16):
        for C in (0, 1, 3):
            c = cases[f"bins_{bins}_channels_{C}"]
            assert c["bins"] == bins and (c["stack"] is None if C == 0 else c["stack"].shape[0] == C)
            geom, table = rc.reference(f"bins_{bins}_channels_{C}")
            assert np.isnan(geom[:, 0]).tolist() == [False, True, False, True, True]
            assert (geom[:, 2:2 + bins].sum(axis=1) == [(c["lab"] == l).sum() for l in range(1, 6)]).all()
            assert not geom[:, 2 + bins:].any() and (table is None) == (C == 0)
    # an all-zero channel is NaN in every column, its neighbours are not
    table = rc.reference("zero_channel")[1]
    assert np.isnan(table[0, 1]).all() and not np.isnan(table[0, 0, :3]).any() and not np.isnan(table[0, 2, :3]).any()
    # 6 x 7 pixels: d is 1, 2 or 3, so no pixel has d / dmax < 1 / 4 -- the outermost of four rings is empty
    assert rc.reference("zero_channel")[0][0, 2:6].tolist() == [6.0, 14.0, 22.0, 0.0]
    assert table[0, 0, 3, 0] == 0.0 and np.isnan(table[0, 0, 3, 1:]).all()
    assert len([n for n in cases if n.startswith("random_")]) == 20
    touching = 0
    for seed in range(20):
        lab = cases[f"random_{seed:02d}"]["lab"]
        assert lab.shape == (48, 64)
        pair = (lab[:, 1:] != lab[:, :-1]) & (lab[:, 1:] > 0) & (lab[:, :-1] > 0)
        touching += bool(pair.any())
    assert touching >= 10
    # frac_at_d sums to 1 and the ring counts to the area, wherever a label exists
    for name in ("annulus", "random_03", "disk_tier_out"):
        geom, table = rc.reference(name)
        here = ~np.isnan(geom[:, 0])
        assert np.allclose(np.nansum(table[here][..., 0], axis=-1), 1.0, rtol=1e-12)
        assert (geom[here, 2:].sum(axis=1) == [(cases[name]["lab"] == l + 1).sum() for l in np.nonzero(here)[0]]).all()


def test_ring_ties_a_float_rule_gets_wrong():
    """The integer rule puts a pixel exactly on a ring boundary into the outer ring; floor(B (1 - sqrt(d2) / sqrt(dmax2)))
    in float64 puts the named pixels one ring too far in."""
    for name, bins, dmax2, tied, count, ring in (("tie_disk17_bins3", 3, 18, 8, 8, 1), ("tie_disk20_bins5", 5, 25, 16, 4, 1)):
        c = rc.cases()[name]
        _, _, d2 = rr.distances(c["lab"], 1)
        assert d2.max() == dmax2 and (d2 == tied).sum() == count
        exact, floated = rr.rings(d2, bins), rr.float_rings(d2, bins)
        assert (exact[d2 == tied] == ring).all() and (floated[d2 == tied] == ring - 1).all(), name
        assert (exact[d2 != tied] == floated[d2 != tied]).all()
    _, _, d2 = rr.distances(rc.cases()["tie_square9_bins5"]["lab"], 1)
    assert sorted(set(d2.tolist())) == [1, 4, 9, 16, 25]
    assert rr.rings(d2, 5).tolist() == [5 - int(math.isqrt(d)) for d in d2.tolist()]  # every pixel lies on a boundary


def test_wedge_ties_are_strict():
    c = rc.cases()["wedge_ties_square"]
    ys, xs, _ = rr.distances(c["lab"], 1)
    w = rr.wedges(ys, xs).reshape(5, 5)
    # the centroid's row (ey = 0), column (ex = 0) and diagonals (|ey| = |ex|) fall to the side of the strict comparisons
    assert w.tolist() == [[0, 4, 4, 6, 2], [0, 0, 4, 2, 2], [0, 0, 0, 2, 2], [1, 1, 5, 3, 3], [1, 5, 5, 7, 3]]


def test_keys_and_their_order():
    assert _hip.RAD_COLS == rr.COLS == ("frac_at_d", "mean_frac", "radial_cv") and _hip.RAD_NCOLS == 3
    assert _hip.RAD_GEOM_NCOLS == rr.GEOM_NCOLS == 18 and _hip.RAD_MAX_BINS == rr.MAX_BINS == 16
    keys = radial_keys([FITC, DAPI])
    assert len(keys) == 2 + 2 * 4 * 3 and len(set(keys)) == len(keys)
    assert keys[:5] == ["maximum_radius", "mean_radius", "radial_frac_at_d_fitc_1of4", "radial_mean_frac_fitc_1of4",
                        "radial_radial_cv_fitc_1of4"]
    assert keys[5] == "radial_frac_at_d_fitc_2of4" and keys[14] == "radial_frac_at_d_dapi_1of4"
    assert keys[-1] == "radial_radial_cv_dapi_4of4"
    assert radial_keys([], bins=7) == ["maximum_radius", "mean_radius"]
    assert radial_keys(["DAPI"], bins=1) == ["maximum_radius", "mean_radius"] + [f"radial_{m}_dapi_1of1" for m in rr.COLS]
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="bins"):
            radial_keys(["DAPI"], bins=bad)
    for bad in (True, 4.0, "4"):
        with pytest.raises(TypeError, match="bins"):
            radial_keys(["DAPI"], bins=bad)


def test_declared_interface():
    header = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    # the capability rides on amt_regionprops_ext: no entry point of its own
    assert "amt_regionprops_ext" in _hip._SIGS and not [name for name in _hip._SIGS if "radial" in name]
    assert not [name for name in re.findall(r"^int\s+(amt_\w+)\s*\(", header, flags=re.M) if "radial" in name]
    assert re.search(r"#define AMT_RPX_RADIAL \(1u << 31\)", header) and _hip.RPX_RADIAL == 1 << 31
    assert re.search(r"#define AMT_RPX_RADIAL_COLUMNS\(bins\)", header)
    for i, name in enumerate(_hip.RAD_COLS):
        assert re.search(rf"#define AMT_RAD_{name.upper()} {i}\b", header), name
    assert re.search(r"#define AMT_RAD_NCOLS 3\b", header) and re.search(r"#define AMT_RAD_GEOM_NCOLS 18\b", header)
    assert re.search(r"#define AMT_RAD_MAX_BINS 16\b", header)
    assert "parity with CellProfiler is unpinned offline" in header
    # the value is negative as an int, and the binding passes that signed value
    assert _hip.rpx_radial_columns(4) == ((1 << 31) | (4 << 14)) - (1 << 32) < 0
    assert _hip.rpx_radial_columns(16) & 0xffffffff == (1 << 31) | (16 << 14)
    assert not _hip.RPX_RADIAL & (0xff | _hip.RPX_RELATE | _hip.RPX_ROBUST | _hip.RPX_NEIGHBORS | _hip.RPX_NEAREST
                                  | _hip.RPX_TEXTURE | _hip.RPX_TEXTURE_COUNTS)
    lib = _hip.load_library()
    p = 1 << 24
    cols = _hip.rpx_radial_columns(4)
    ok = [None, p, 2 * p, _hip.U16, 1, cols, 3 * p, 4 * p, 1, 4, 6, 2]
    assert lib.amt_regionprops_ext(*ok) == -1 and lib.amt_last_error() == b"null context"
    for code in (_hip.U16, _hip.F64):
        for bins in (1, 16):
            args = list(ok)
            args[3], args[5] = code, _hip.rpx_radial_columns(bins)
            assert lib.amt_regionprops_ext(*args) == -1 and lib.amt_last_error() == b"null context"
    geometry_only = [None, p, None, 0, 0, cols, 3 * p, None, 1, 4, 6, 2]
    assert lib.amt_regionprops_ext(*geometry_only) == -1 and lib.amt_last_error() == b"null context"
    # refused before the context is looked at
    bad_calls = [(5, _hip.rpx_radial_columns(0)), (5, _hip.rpx_radial_columns(17)), (5, _hip.rpx_radial_columns(127)),
                 (3, _hip.U8), (3, _hip.I32), (2, None), (7, None), (6, None), (4, 0), (1, None)]
    for bit in list(range(0, 14)) + list(range(21, 31)):  # every other bit, the field in bits 21-30 included
        bad_calls.append((5, cols | (1 << bit)))
    bad_calls.append((5, cols | _hip.rpx_texture_columns(4, 1)))
    for at, bad in bad_calls:
        args = list(ok)
        args[at] = bad
        assert lib.amt_regionprops_ext(*args) == -1 and lib.amt_last_error() != b"null context", (at, bad)
    for at, bad in ((2, 2 * p), (7, 4 * p), (4, 1)):  # C == 0 with planes, with a table, C >= 1 with neither
        args = list(geometry_only)
        args[at] = bad
        assert lib.amt_regionprops_ext(*args) == -1 and lib.amt_last_error() != b"null context", (at, bad)
    # overlapping operands, under the entry point's name: 1 x 2 x 18 doubles of geometry, 1 x 2 x 1 x 4 x 3 of columns
    for at, where in ((7, 3 * p + 8), (7, 3 * p + 280), (6, p + 8), (7, 2 * p - 184), (6, 4 * p - 280)):
        args = list(ok)
        args[at] = where
        assert lib.amt_regionprops_ext(*args) == -1
        msg = lib.amt_last_error()
        assert b"amt_regionprops_ext: " in msg and b"must not alias" in msg, (at, where, msg)
    args = list(ok)
    args[7] = 3 * p + 288  # right behind the geometry
    assert lib.amt_regionprops_ext(*args) == -1 and lib.amt_last_error() == b"null context"
    # the existing bits are as they were: parameters without a bit, and texture with bit 31
    assert lib.amt_regionprops_ext(*(ok[:5] + [4 << 14] + ok[6:])) == -1 and lib.amt_last_error() != b"null context"
    assert lib.amt_regionprops_ext(*(ok[:5] + [_hip.rpx_texture_columns(8, 1) | (1 << 31)] + ok[6:])) == -1
    assert lib.amt_last_error() != b"null context"


class _NoContext:
    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}): a device call before the refusal")


_CTX = _NoContext()


def _arr(shape, dtype, ptr):
    return DeviceArray(_CTX, ptr, shape, dtype)


def test_argument_errors_of_hipops_need_no_device():
    lab = _arr((7, 5), np.int32, 1 << 20)
    img = _arr((1, 7, 5), np.uint16, 1 << 22)
    for bad in (0, 17, -4):
        with pytest.raises(ValueError, match="bins"):
            hipops.radial_distribution(lab, img, 1, bins=bad)
        with pytest.raises(ValueError, match="bins"):
            hipops.radial_parameters(bad)
    for bad in (True, 4.0, "4", None):
        with pytest.raises(TypeError, match="bins"):
            hipops.radial_distribution(lab, img, 1, bins=bad)
    assert hipops.radial_parameters(np.int64(16)) == 16 and hipops.radial_parameters(1) == 1
    with pytest.raises(TypeError, match="int32"):
        hipops.radial_distribution(_arr((7, 5), np.uint16, 1 << 20), img, 1)
    for dt in (np.uint8, np.float32):
        with pytest.raises(TypeError):
            hipops.radial_distribution(lab, _arr((1, 7, 5), dt, 1 << 22), 1)
    for shape in ((1, 5, 7), (7, 5), (2, 1, 7, 5)):
        with pytest.raises(ValueError):
            hipops.radial_distribution(lab, _arr(shape, np.uint16, 1 << 22), 1)
    with pytest.raises(ValueError, match="max_label"):
        hipops.radial_distribution(lab, img, -1)
    with pytest.raises(ValueError, match="out has shape"):
        hipops.radial_distribution(lab, img, 1, out=_arr((1, 1, 1, 4, 4), np.float64, 1 << 24))
    with pytest.raises(ValueError, match="out has shape"):
        hipops.radial_distribution(lab, img, 1, geometry_out=_arr((1, 1, 17), np.float64, 1 << 24))
    with pytest.raises(ValueError, match="without them"):
        hipops.radial_distribution(lab, None, 1, out=_arr((1, 1, 0, 4, 3), np.float64, 1 << 24))
    table, geom = _arr((1, 1, 1, 4, 3), np.float64, 1 << 24), _arr((1, 1, 18), np.float64, 1 << 26)
    for kw in ({"out": _arr((1, 1, 1, 4, 3), np.float64, (1 << 22) + 8)},                  # on the image
               {"geometry_out": _arr((1, 1, 18), np.float64, (1 << 20) - 136)},            # its last word on the labels
               {"out": table, "geometry_out": _arr((1, 1, 18), np.float64, (1 << 24) + 88)},  # on the table
               {"out": table, "geometry_out": _arr((1, 1, 18), np.float64, (1 << 24) - 136)}):
        with pytest.raises(ValueError, match="alias"):
            hipops.radial_distribution(lab, img, 1, **kw)
    with pytest.raises(ValueError, match="alias"):
        hipops.radial_distribution(lab, None, 1, geometry_out=_arr((1, 1, 18), np.float64, (1 << 20) + 8))
    with pytest.raises(AssertionError, match="the context was used"):  # apart: as far as the device
        hipops.radial_distribution(lab, img, 1, out=table, geometry_out=geom)
    with pytest.raises(AssertionError, match="the context was used"):
        hipops.radial_distribution(lab, None, 1, geometry_out=geom)
    with pytest.raises(ValueError, match="hipops.radial_distribution"):
        hipops.regionprops_ext(lab, 1, _hip.RPX_RADIAL | 4 << 14)
    with pytest.raises(ValueError, match="hipops.radial_distribution"):
        hipops.regionprops_ext(lab, 1, _hip.rpx_radial_columns(4))


def test_argument_errors_of_cell_radial_distribution_need_no_device():
    nuclei = np.zeros((16, 16), np.int64)
    nuclei[2:9, 3:11] = 1
    images = {DAPI: np.arange(256, dtype=np.uint16).reshape(16, 16)}
    for mask in (SegmentationMask(nuclei, remove_edge_cells=False), SegmentationMask(nuclei, images, remove_edge_cells=False)):
        for bad in (0, 17):
            with pytest.raises(ValueError, match="bins"):
                mask.cell_radial_distribution(bins=bad)
        for bad in (True, 2.0):
            with pytest.raises(TypeError, match="bins"):
                mask.cell_radial_distribution(bins=bad)
