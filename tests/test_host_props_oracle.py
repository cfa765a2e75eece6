"""The oracle's extended region properties (oracle/regionprops.py) against scikit-image 0.18.3, pinned by
tests/golden/props_ext.npz (cases nuc, syn) and tests/golden/props_frag.npz (tools/make_golden_props.py).  No GPU."""
import numpy as np
import pytest
from scipy import ndimage as ndi

from oracle import regionprops as orp

# exact: integer counts, the exact integer hull, feret_diameter_max (its square is a multiple of 1/4) and the local
# centroid (exact moment sums, one rounding)
EXACT = ("label", "area", "bbox", "area_convex", "euler_number", "area_filled", "feret_diameter_max",
         "centroid_local", "area_bbox")
CHANNELS = {"nuc": ("BRIGHTFIELD", "DAPI", "FITC", "TRITC"), "syn": ("DAPI", "FITC"), "frag": ("DAPI", "FITC")}


def _case(golden, case):
    g = golden("props_frag" if case == "frag" else "props_ext")
    if case == "nuc":
        fov = g["nuc__fov"]
        channels = {n: fov[i] for i, n in enumerate(CHANNELS[case])}
    else:
        channels = {n: g[f"{case}__{n.lower()}"] for n in CHANNELS[case]}
    return g, g[f"{case}__labels"], channels


@pytest.mark.parametrize("case", ["nuc", "syn", "frag"])
def test_oracle_extended_columns_match_scikit_image(golden, case):
    g, labels, channels = _case(golden, case)
    t = orp.cell_properties(labels, channels, [str(p) for p in g["props"]], [str(p) for p in g["iprops"]])
    keys = [str(k) for k in g[f"{case}__keys"]]
    assert list(t) == keys
    for k in keys:
        want, got = g[f"{case}__{k}"], t[k]
        assert got.dtype == want.dtype, k
        if k.startswith(EXACT):
            assert np.array_equal(got, want), k
        elif k == "orientation":
            sym = np.isclose(np.abs(want), np.pi / 4)  # unpinned for exactly symmetric regions
            np.testing.assert_allclose(got[~sym], want[~sym], rtol=0, atol=1e-9, err_msg=k)
        else:
            assert np.array_equal(np.isnan(got), np.isnan(want)), k
            scale = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 1.0
            # 1e-12 relative; entries that cancel to ~0 (inertia_tensor-0-1 of symmetric cells, eccentricity of
            # disks) against the column's scale
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * max(scale, 1.0), err_msg=k)


def test_frag_golden_covers_its_corner_cases(golden):
    g, labels, _ = _case(golden, "frag")
    boxes = ndi.find_objects(labels)
    spans = [(sl[0].stop - sl[0].start, sl[1].stop - sl[1].start) for sl in boxes]
    assert sum(h for h, _ in spans) > labels.size
    for n in (63, 64, 65, 128, 129):
        assert any(n in s for s in spans), n
    assert any(h == 48 and w == 250 for h, w in spans) and any(h == 49 for h, _ in spans)
    assert any(w == 251 for _, w in spans)
    assert max(sl[0].stop for sl in boxes) == labels.shape[0] and max(sl[1].stop for sl in boxes) == labels.shape[1]
    assert (g["frag__area_filled"] > g["frag__area"]).sum() >= 8
    assert g["frag__dapi"].max() == 65535 and (g["frag__fitc"] < 0).any()
    assert np.isnan(g["frag__centroid_weighted-0_dapi"]).any() and np.isnan(g["frag__centroid_weighted-0_fitc"]).any()


def test_convex_image_is_the_area_convex_region():
    rng = np.random.default_rng(4)
    for _ in range(50):
        m = rng.random(tuple(rng.integers(1, 30, 2))) < rng.random()
        m[0, 0] = True
        img = orp.convex_image_exact(m)
        assert img.dtype == bool and img.shape == m.shape
        assert (img | ~m).all()  # contains the region
        assert orp.convex_area_exact(m) == int(img.sum())


def test_feret_of_small_shapes():
    one = np.ones((1, 1), bool)
    assert orp.feret_diameter_max(one) == 1.0  # the contour of one pixel is a diamond of half-width 1/2
    bar = np.ones((1, 7), bool)
    assert orp.feret_diameter_max(bar) == 7.0
    sq = np.ones((3, 4), bool)  # midpoints (0, -1/2) - (2, 7/2): scikit-image 0.18.3 gives sqrt(20) too
    assert orp.feret_diameter_max(sq) == np.sqrt(20.0)
