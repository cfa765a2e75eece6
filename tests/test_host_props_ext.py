"""Host side of the extended regionprops columns: the key layout of ``cell_properties`` (split indices, channel
suffixes, order) for the extended names, checked against the golden file without loading the library."""
import numpy as np

from arcadia_microscopy_tools_amd import _hip
from arcadia_microscopy_tools_amd.segment import assemble_cell_properties, cell_property_keys, ext_columns


def test_key_layout_matches_the_golden_file(golden):
    g = golden("props_ext")
    props, iprops = [str(p) for p in g["props"]], [str(p) for p in g["iprops"]]
    assert cell_property_keys(["BRIGHTFIELD", "DAPI", "FITC", "TRITC"], props, iprops) == [str(k) for k in g["nuc__keys"]]
    assert cell_property_keys(["DAPI", "FITC"], props, iprops) == [str(k) for k in g["syn__keys"]]


def test_split_keys_and_suffixes():
    keys = cell_property_keys(["DAPI"], ["label", "inertia_tensor", "euler_number", "circularity"],
                              ["centroid_weighted_local", "intensity_mean"])
    assert keys == ["label", "inertia_tensor-0-0", "inertia_tensor-0-1", "inertia_tensor-1-0", "inertia_tensor-1-1",
                    "euler_number", "circularity", "centroid_weighted_local-0_dapi",
                    "centroid_weighted_local-1_dapi", "intensity_mean_dapi"]


def test_ext_columns_and_host_columns():
    assert ext_columns(["label", "area_bbox", "feret_diameter_max", "centroid_weighted"],
                       ["centroid_weighted", "intensity_mean"]) == ["feret_diameter_max", "centroid_weighted"]
    assert set(ext_columns(list(_hip.RPX_BITS), list(_hip.RPX_BITS))) == set(_hip.RPX_BITS)
    # area_bbox / extent / equivalent_diameter_area come from the area and the bounding box
    morph = np.zeros((2, _hip.RP_NCOLS))
    c = {n: i for i, n in enumerate(_hip.RP_COLS)}
    morph[:, c["area"]] = [6.0, 1.0]
    morph[:, c["bbox-2"]], morph[:, c["bbox-3"]] = [3.0, 5.0], [4.0, 8.0]
    morph[:, c["bbox-0"]], morph[:, c["bbox-1"]] = [0.0, 4.0], [1.0, 7.0]
    t = assemble_cell_properties(morph, None, [], ["area_bbox", "extent", "equivalent_diameter_area"])
    np.testing.assert_array_equal(t["area_bbox"], [9.0, 1.0])
    np.testing.assert_array_equal(t["extent"], [6.0 / 9.0, 1.0])
    np.testing.assert_allclose(t["equivalent_diameter_area"], np.sqrt(4 * np.array([6.0, 1.0]) / np.pi), rtol=1e-15)
    assert all(v.dtype == np.float64 for v in t.values())
