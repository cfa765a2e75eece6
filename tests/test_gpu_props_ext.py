"""Extended regionprops columns of ``SegmentationMask.cell_properties`` (euler_number, perimeter_crofton, area_filled,
feret_diameter_max, area_bbox, extent, equivalent_diameter_area, centroid_local, inertia_tensor(_eigvals) and the
weighted centroids) against scikit-image, pinned by tests/golden/props_ext.npz (tools/make_golden_props.py)."""
import numpy as np
import pytest

from arcadia_microscopy_tools_amd.channels import BRIGHTFIELD, DAPI, FITC, TRITC
from arcadia_microscopy_tools_amd.masks import DEFAULT_CELL_PROPERTY_NAMES, SegmentationMask

pytestmark = pytest.mark.gpu

EXACT = ("euler_number", "area_filled", "area_bbox", "extent", "feret_diameter_max", "centroid_local")
NUC_CHANNELS = (BRIGHTFIELD, DAPI, FITC, TRITC)


def _case(g, case):
    if case == "nuc":
        fov = g["nuc__fov"]
        return g["nuc__labels"], {c: fov[i] for i, c in enumerate(NUC_CHANNELS)}
    return g["syn__labels"], {DAPI: g["syn__dapi"], FITC: g["syn__fitc"]}


def _mask(g, case, **kw):
    labels, channels = _case(g, case)
    kw.setdefault("property_names", [str(p) for p in g["props"]])
    kw.setdefault("intensity_property_names", [str(p) for p in g["iprops"]])
    return SegmentationMask(labels, channels, remove_edge_cells=False, **kw)


def _check_against_golden(props, g, case):
    keys = [str(k) for k in g[f"{case}__keys"]]
    assert list(props) == keys
    for k in keys:
        want, got = g[f"{case}__{k}"], props[k]
        assert got.dtype == want.dtype, k
        if k.startswith(EXACT):
            assert np.array_equal(got, want, equal_nan=True), k
        elif k in ("orientation", "eccentricity"):
            # default columns, pinned elsewhere: 0.18.3's orientation of exactly symmetric regions is unpinned
            # (SURVEY.md A.9), eccentricity agrees to ~2e-11 absolute (A.12)
            sym = np.isclose(np.abs(want), np.pi / 4) if k == "orientation" else np.zeros(want.shape, bool)
            np.testing.assert_allclose(got[~sym], want[~sym], rtol=0, atol=1e-8, err_msg=k)
            np.testing.assert_allclose(np.abs(got[sym]), np.pi / 4, err_msg=k)
        else:
            assert np.array_equal(np.isnan(got), np.isnan(want)), k
            scale = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 1.0
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * max(scale, 1.0), err_msg=k)


@pytest.mark.parametrize("case", ["nuc", "syn"])
def test_extended_columns_match_scikit_image(golden, case):
    g = golden("props_ext")
    _check_against_golden(_mask(g, case).cell_properties, g, case)


def test_golden_covers_the_corner_cases(golden):
    g = golden("props_ext")
    assert (g["syn__euler_number"] < 0).any() and (g["syn__area_filled"] > g["syn__area"]).any()
    assert np.isnan(g["syn__centroid_weighted-0_dapi"]).any() and np.isnan(g["syn__centroid_weighted-0_fitc"]).any()
    labels = g["syn__labels"]
    spans = [(np.ptp(ys) + 1, np.ptp(xs) + 1) for ys, xs in (np.nonzero(labels == lab) for lab in range(1, labels.max() + 1))]
    assert any(h > 48 and w > 250 for h, w in spans), "a cell beyond the LDS hull class"
    assert any(h > 64 or w > 64 for h, w in spans) and any(h <= 64 and w <= 64 for h, w in spans)


def test_default_columns_unchanged_by_extended_names(golden):
    g = golden("props_ext")
    for case in ("nuc", "syn"):
        ext = _mask(g, case).cell_properties
        base = _mask(g, case, property_names=None, intensity_property_names=None).cell_properties
        for k, v in base.items():
            assert ext[k].dtype == v.dtype and np.array_equal(ext[k], v, equal_nan=True), (case, k)


def test_batch_masks_extended_columns_equal_the_mask_of_its_labels(golden):
    from arcadia_microscopy_tools_amd import synth
    from arcadia_microscopy_tools_amd.model import SegmentationModel

    g = golden("props_ext")
    props = list(DEFAULT_CELL_PROPERTY_NAMES) + [str(p) for p in g["props"] if p not in DEFAULT_CELL_PROPERTY_NAMES]
    iprops = [str(p) for p in g["iprops"]]
    model = SegmentationModel(backend="classical")
    fovs = [synth.synth_fov(40 + i, size=320) for i in range(3)]
    got = model.batch_masks(fovs, NUC_CHANNELS, nuclear=DAPI, batch_size=2, property_names=props,
                            intensity_property_names=iprops)
    assert "_rows" in got[0].__dict__
    for m, f in zip(got, fovs):
        want = SegmentationMask(m.label_image, dict(zip(NUC_CHANNELS, f)), remove_edge_cells=False,
                                property_names=props, intensity_property_names=iprops).cell_properties
        have = m.cell_properties
        assert list(have) == list(want)
        for k in want:
            assert have[k].dtype == want[k].dtype and np.array_equal(have[k], want[k], equal_nan=True), k


def test_filter_on_extended_columns(golden):
    g = golden("props_ext")
    m = _mask(g, "syn")
    euler, filled, area = g["syn__euler_number"], g["syn__area_filled"], g["syn__area"]
    holed = m.filter("euler_number", max_value=0)
    assert holed.num_cells == int((euler <= 0).sum())
    np.testing.assert_array_equal(holed.cell_properties["euler_number"], euler[euler <= 0])
    kept = np.isin(m.label_image, np.nonzero(euler <= 0)[0] + 1)
    assert np.array_equal(holed.label_image > 0, kept)
    big = m.filter("area_filled", min_value=100.0)
    assert big.num_cells == int((filled >= 100).sum())
    np.testing.assert_array_equal(big.cell_properties["area"], area[filled >= 100])


def test_micron_conversion_leaves_extended_keys_alone(golden):
    g = golden("props_ext")
    m = _mask(g, "syn")
    um = m.convert_properties_to_microns(0.5)
    props = m.cell_properties
    for k in props:
        base = k.split("-")[0]
        if base in ("inertia_tensor", "inertia_tensor_eigvals", "euler_number", "perimeter_crofton", "area_filled",
                    "feret_diameter_max", "area_bbox", "extent", "equivalent_diameter_area", "centroid_local",
                    "centroid_weighted", "centroid_weighted_local"):
            assert k in um and um[k] is props[k], k


def test_names_outside_the_table_still_raise(golden):
    g = golden("props_ext")
    for name in ("moments_hu", "image", "filled_area", "centroid_weighted"):
        with pytest.raises(AttributeError):
            _mask(g, "syn", property_names=["label", name]).cell_properties
    with pytest.raises(AttributeError):
        _mask(g, "syn", property_names=["label"], intensity_property_names=["moments_weighted"]).cell_properties


def test_regionprops_ext_batch_equals_one_call_per_plane(golden):
    from arcadia_microscopy_tools_amd import _hip, hipops
    from arcadia_microscopy_tools_amd.device import get_context

    g = golden("props_ext")
    ctx = get_context()
    syn = g["syn__labels"].astype(np.int32)
    nuc = np.zeros_like(syn)
    nuc[:, :256] = g["nuc__labels"][:110]
    gaps = np.where(syn > 0, syn * 3 + 2, 0).astype(np.int32)  # labels 5, 8, ...: most numbers absent
    planes = np.stack([syn, np.zeros_like(syn), gaps, nuc])
    inten = np.stack([np.stack([g["syn__dapi"], g["syn__dapi"][::-1]])] * 4)
    mx = int(planes.max())
    names = list(_hip.RPX_BITS)
    t, w = hipops.regionprops_ext(ctx.asarray(planes), mx, names, intensity=ctx.asarray(inten))
    t, w = t.numpy(), w.numpy()
    for i in range(planes.shape[0]):
        t1, w1 = hipops.regionprops_ext(ctx.asarray(planes[i]), mx, names, intensity=ctx.asarray(inten[i]))
        assert np.array_equal(t[i], t1.numpy()[0], equal_nan=True), i
        assert np.array_equal(w[i], w1.numpy()[0], equal_nan=True), i
    assert not t[1].any() and not w[1].any()  # the empty plane
    present = np.isin(np.arange(1, mx + 1), planes[2])
    assert not t[2][~present].any()
    # the renumbered plane measures what the sequential one does (positions do not depend on the numbers)
    seq = np.arange(1, syn.max() + 1) * 3 + 2
    assert np.array_equal(t[2][seq - 1], t[0][:syn.max()], equal_nan=True)
    assert np.array_equal(w[2][seq - 1], w[0][:syn.max()], equal_nan=True)
