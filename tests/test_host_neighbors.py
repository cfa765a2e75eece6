"""Cell neighbours (AMT_RPX_NEIGHBORS, AMT_RPX_NEAREST), the parts that need no device: the numpy reference on
hand-written planes with the expected rows written out, the ring against scipy's dilation, the symmetry of touching, the
header's and the binding's constants, the key names, and what the case list holds."""
import os
import re

import numpy as np
import pytest

import neighbors_cases as nc
import neighbors_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "amt_hip.h")) as f:
        return f.read()


def _define(header, name):
    m = re.search(r"#define\s+" + name + r"\s+(\S+.*)", header)
    assert m, name
    return m.group(1).strip()


def _rows(a):
    return [[None if isinstance(v, float) and np.isnan(v) else v for v in row] for row in np.asarray(a).tolist()]


def test_reference_on_hand_written_planes():
    # a diagonal-only contact counts (8-connectivity); label 3 sits on the border, its ring is clipped to the plane
    lab = np.array([[1, 1, 0, 0, 0],
                    [1, 1, 0, 0, 0],
                    [0, 0, 2, 2, 0],
                    [0, 0, 2, 2, 0],
                    [0, 0, 0, 0, 3]])
    assert nr.census_columns(lab, lab, 3).tolist() == [[1, 1, 5, 2], [2, 2, 12, 1], [1, 1, 3, 2]]
    assert nr.neighbor_sets(lab, lab, 3) == [{2}, {1, 3}, {2}]
    s8, s4p5 = np.sqrt(8.0), np.sqrt(4.5)
    assert s4p5 == np.sqrt(1.5 * 1.5 + 1.5 * 1.5)
    assert _rows(nr.nearest_columns(lab, 3)) == [[2.0, s8, 3.0, np.sqrt(24.5)], [3.0, s4p5, 1.0, s8],
                                                 [2.0, s4p5, 1.0, np.sqrt(24.5)]]
    # a label split into pieces: one ring around all of them, one centroid
    lab = np.array([[1, 0, 0, 0, 1],
                    [0, 0, 2, 0, 0],
                    [0, 0, 2, 0, 0],
                    [0, 0, 0, 0, 0],
                    [1, 0, 3, 0, 1]])
    assert nr.census_columns(lab, lab, 4).tolist() == [[0, 0, 12, 0], [0, 0, 10, 0], [0, 0, 5, 0], [0, 0, 0, 0]]
    # label 1's centroid (2, 2) is nearer to label 2's (1.5, 2) than to label 3's (4, 2); label 4 is absent
    assert _rows(nr.nearest_columns(lab, 4)) == [[2.0, 0.5, 3.0, 2.0], [1.0, 0.5, 3.0, 2.5], [1.0, 2.0, 2.0, 2.5],
                                                 [0.0, None, 0.0, None]]
    # a tie for MAIN: labels 2 and 3 hold two ring pixels each, the smaller value wins; 4 holds one
    lab = np.array([[0, 0, 0, 0, 0],
                    [0, 3, 2, 2, 0],
                    [0, 3, 1, 4, 0],
                    [0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0]])
    assert nr.census_columns(lab, lab, 4)[0].tolist() == [3, 5, 8, 2]
    comp = np.where(lab == 2, 9, lab)  # a companion plane with other values: now 3 stands alone among equals
    assert nr.census_columns(lab, comp, 4)[0].tolist() == [3, 5, 8, 3]
    assert nr.census_columns(lab, comp, 4)[2].tolist() == [2, 2, 10, 1]  # label 3 on the companion: 1 and 9, one each
    # a label is not its own neighbour, on a companion plane either; values <= 0 are background
    comp = np.array([[1, 1, 1, 1, 1],
                     [1, 1, 1, 1, 1],
                     [1, 1, 7, 1, -4],
                     [1, 1, 1, 1, 1],
                     [1, 1, 1, 1, 1]])
    assert nr.census_columns(lab, comp, 1).tolist() == [[0, 0, 8, 0]]
    # a plane filled by one label: no ring, nobody near
    full = np.ones((5, 5), np.int64)
    assert nr.census_columns(full, full, 2).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]
    assert _rows(nr.nearest_columns(full, 2)) == [[0.0, None, 0.0, None]] * 2
    cells = nr.cell_neighbors(full, 1)
    assert list(cells) == list(nr.KEYS) and np.isnan(cells["percent_touching"]).all()
    cells = nr.cell_neighbors(lab, 4)
    assert cells["percent_touching"].tolist() == [62.5, 100.0 * 4 / 10, 100.0 * 2 / 10, 100.0 * 3 / 8]
    assert cells["number_of_neighbors"].dtype == np.int64 and cells["first_closest_label"].dtype == np.int64


def test_ring_equals_scipy_dilation():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in nc.SHAPES:
        for name in ("blobs", "voronoi", "pieces", "out_of_range_labels", "column_and_row"):
            lab, _, k = nc.cases(shape)[name]
            for l in range(1, k + 1):
                want = ndi.binary_dilation(lab == l, np.ones((3, 3), bool)) & (lab != l)
                assert np.array_equal(nr.ring_mask(lab, l), want), (shape, name, l)


def test_touching_is_symmetric_on_self_companion_planes():
    pairs = 0
    for shape in nc.SHAPES:
        for name in ("blobs", "voronoi", "gaps", "pieces", "column_and_row"):
            lab, comp, k = nc.cases(shape)[name]
            assert comp is None
            sets = nr.neighbor_sets(lab, lab, k)
            for l, s in enumerate(sets, start=1):
                assert l not in s
                for m in s:
                    if 1 <= m <= k:
                        assert l in sets[m - 1], (shape, name, l, m)
                        pairs += 1
    assert pairs > 100


def test_header_defines_and_documents_the_neighbours():
    h = _header()
    assert eval(_define(h, "AMT_RPX_NEIGHBORS").replace("u", "")) == 1024
    assert eval(_define(h, "AMT_RPX_NEAREST").replace("u", "")) == 2048
    assert _define(h, "AMT_RPX_ALL") == "0xffu"
    assert [int(_define(h, "AMT_RPX_NCOL_" + n)) for n in ("COUNT", "TOUCHING", "RING", "MAIN")] == [0, 1, 2, 3]
    assert [int(_define(h, "AMT_RPX_DCOL_" + n))
            for n in ("FIRST", "FIRST_DISTANCE", "SECOND", "SECOND_DISTANCE")] == [0, 1, 2, 3]
    # the new defines follow AMT_ROBUST_LDS_BINS, the new block stands before the robust block
    assert (h.index("#define AMT_ROBUST_LDS_BINS") < h.index("#define AMT_RPX_NEIGHBORS")
            < h.index("#define AMT_RPX_NEAREST") < h.index("#define AMT_RPX_COL_EULER"))
    start = h.index("AMT_RPX_NEIGHBORS and AMT_RPX_NEAREST ----")
    assert start < h.index("AMT_RPX_ROBUST ----") < h.index("AMT_RPX_RELATE ----")
    block = h[start:h.index("AMT_RPX_ROBUST ----")]
    for word in ("8-neighbour", "labels[q] != l", "not its own neighbour", "distinct", "smallest", "AMT_I32", "NULL",
                 "C == 1", "AMT_EINVAL", "AMT_RELATE_LDS_PARTNERS", "identical bytes", "NaN", "fused multiply-add",
                 "(d2, m)", "sqrt(d2)", "AMT_RPX_NCOL_COUNT", "AMT_RPX_NCOL_TOUCHING", "AMT_RPX_NCOL_RING",
                 "AMT_RPX_NCOL_MAIN", "AMT_RPX_DCOL_FIRST", "AMT_RPX_DCOL_FIRST_DISTANCE", "AMT_RPX_DCOL_SECOND",
                 "AMT_RPX_DCOL_SECOND_DISTANCE", "AMT_RPX_CENTROID_WEIGHTED", "AMT_RPX_RELATE", "AMT_RPX_ROBUST",
                 "AMT_RPX_ALL | AMT_RPX_RELATE | AMT_RPX_ROBUST | AMT_RPX_NEIGHBORS | AMT_RPX_NEAREST",
                 "before the first launch"):
        assert word in block, word
    # the capability rides on amt_regionprops_ext: no entry point of its own
    protos = re.findall(r"^int\s+(amt_\w+)\s*\(", h, flags=re.M)
    assert protos.count("amt_regionprops_ext") == 1
    assert not [name for name in protos if "neighbor" in name or "neighbour" in name or "nearest" in name]


def test_binding_constants_equal_the_header():
    from arcadia_microscopy_tools_amd import _hip

    h = _header()
    assert _hip.RPX_NEIGHBORS == 1024 == 1 << 10 and _hip.RPX_NEAREST == 2048 == 1 << 11
    assert _hip.RPX_NCOLS4 == ("count", "touching", "ring", "main") == nr.NCOLS
    assert _hip.RPX_DCOLS == ("first", "first_distance", "second", "second_distance") == nr.DCOLS
    for i, n in enumerate(_hip.RPX_NCOLS4):
        assert int(_define(h, "AMT_RPX_NCOL_" + n.upper())) == i
    for i, n in enumerate(_hip.RPX_DCOLS):
        assert int(_define(h, "AMT_RPX_DCOL_" + n.upper())) == i
    assert _hip.RPX_BITS == {
        "euler_number": 1, "perimeter_crofton": 2, "area_filled": 4, "feret_diameter_max": 8, "centroid_local": 16,
        "inertia_tensor": 32, "inertia_tensor_eigvals": 64, "centroid_weighted": 128, "centroid_weighted_local": 128}
    assert _hip.RPX_RELATE == 256 and _hip.RPX_ROBUST == 512 and _hip.RPX_NCOLS == 12
    assert "amt_regionprops_ext" in _hip._SIGS
    assert not [name for name in _hip._SIGS if "neighbor" in name or "nearest" in name]
    with open(os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc", "amt_relate.hip")) as f:
        src = f.read()
    # one table for the relation and the census: the kernels share its helpers
    assert src.count("__shared__ int keys[RL_SLOTS]") == 2 and src.count("bool rl_table_add(") == 1
    assert "rpx_neighbors_kernel" in src and "rpx_nearest_kernel" in src


def test_hipops_has_the_two_functions():
    from arcadia_microscopy_tools_amd import hipops

    assert callable(hipops.neighbor_census) and callable(hipops.nearest_labels)


def test_neighbor_keys():
    from arcadia_microscopy_tools_amd import segment
    from arcadia_microscopy_tools_amd.masks import SegmentationMask

    assert segment.neighbor_keys() == list(nr.KEYS)
    assert segment.neighbor_keys() == [
        "number_of_neighbors", "touching_pixels", "ring_pixels", "percent_touching", "main_neighbor",
        "first_closest_label", "first_closest_distance", "second_closest_label", "second_closest_distance"]
    assert callable(SegmentationMask.cell_neighbors)
    # cell_properties keeps its names: none of the new ones is accepted or produced there
    assert not [k for k in segment.cell_property_keys(["DAPI"]) if "neighbor" in k or "closest" in k or "touching" in k]


def test_the_cases_hold_what_they_are_named_for():
    P = nc._partners()
    with_neighbour = isolated = 0
    for shape in nc.SHAPES:
        cs = nc.cases(shape)
        assert {"blobs", "voronoi", "gaps", "pieces", "out_of_range_labels", "column_and_row", "full_plane",
                "zero_companion", "special_values"} <= set(cs)
        for name, (lab, comp, k) in cs.items():
            assert lab.dtype == np.int32 and lab.shape == shape and k >= 1, name
            assert comp is None or (comp.dtype == np.int32 and comp.shape == shape), name
        census, nearest = nc.reference(shape, "blobs")
        present = census[:, 2] > 0
        with_neighbour += int((census[present, 0] > 0).sum())
        isolated += int((census[present, 0] == 0).sum())
        census, _ = nc.reference(shape, "voronoi")
        assert np.array_equal(census[:, 1], census[:, 2])  # no background: every ring pixel belongs to somebody
        gaps, near = nc.reference(shape, "gaps")
        assert not gaps[1::3].any() and not gaps[-2:].any() and np.isnan(near[1::3, 1]).all()
        assert set(near[:, 0].astype(int).tolist()) <= {0} | set(range(3, gaps.shape[0] + 1, 3))
        assert nc.reference(shape, "full_plane")[0].tolist() == [[0, 0, 0, 0]] * 2
        assert not nc.reference(shape, "zero_companion")[0][:, [0, 1, 3]].any()
        lab = cs["out_of_range_labels"][0]
        if shape[0] * shape[1] >= 35:
            assert lab.min() < 0 and lab.max() > 4
            sets = nr.neighbor_sets(lab, lab, 4)  # values above max_label are neighbours, negative ones are not
            assert all(max(s) > 4 and min(s) > 0 for s in sets)
        if "main_ties" in cs:
            lab, comp, _ = cs["main_ties"]
            vals = nr.neighbor_values(lab, comp, 1)
            assert (vals == 3).sum() == (vals == 9).sum() >= 1 and (vals == 7).sum() <= 1
            assert nc.reference(shape, "main_ties")[0][0, 3] == 3
    assert with_neighbour > 0 and isolated > 0  # blobs that touch and blobs that stand alone both occur
    assert "main_ties" in nc.cases((7, 5)) and "main_ties" in nc.cases((70, 131))
    sp = nc.cases((16, 16))["special_values"]
    assert {1, nc.BIG, P, 2 * P, -7} <= set(np.unique(sp[1]).tolist())
    assert nc.BIG in nr.neighbor_values(sp[0], sp[1], 1) and 1 not in nr.neighbor_values(sp[0], sp[1], 1)
    lab = nc.cases((70, 131))["column_and_row"][0]
    assert (lab == 2).any(axis=0).sum() > 64 and (lab == 1).any(axis=0).sum() == 1
    # around the table's capacity: label 1's ring is the 16 odd rows, label 2 has three neighbours
    shape = nc.overflow_shape()
    assert shape == (33, 40) and (shape[0] // 2) * shape[1] == 640 >= 4 * P
    for d in (P - 1, P, P + 1, 4 * P):
        for kind in ("random", "congruent"):
            census, _ = nc.reference(shape, f"{kind}_{d}_neighbors")
            assert census[0].tolist()[:3] == [d, 640, 640] and census[1, 0] == 3, (kind, d)
    comp = nc.cases(shape)["congruent_%d_neighbors" % (P + 1)][1]
    assert len(np.unique(comp[comp > 0] % P)) == 1
    # the lattice: every first distance is 5 and shared by several candidates, the smallest label wins
    _, near = nc.reference(nc.LATTICE_SHAPE, "lattice")
    assert (near[:, 1] == 5.0).all()
    assert near[:, 0].tolist() == [2, 1, 2, 1, 2, 3, 4, 5, 6] and near[4].tolist() == [2.0, 5.0, 4.0, 5.0]
    _, near = nc.reference(nc.LATTICE_SHAPE, "one_label")
    assert _rows(near) == [[0.0, None, 0.0, None]] * 3
    _, near = nc.reference(nc.LATTICE_SHAPE, "two_labels")
    assert near[1, 0] == 3 and near[2, 0] == 2 and near[1, 1] == near[2, 1] > 0
    assert _rows(near[:, 2:]) == [[0.0, None]] * 3 and _rows(near[:1]) == [[0.0, None, 0.0, None]]
