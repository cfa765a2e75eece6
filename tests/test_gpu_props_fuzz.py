"""Seeded corner cases of the region-property kernels (amt_regionprops, amt_regionprops_ext) against scikit-image
(tests/golden/props_frag.npz) and the numpy/scipy oracle (oracle/regionprops.py): fragmented integer labels whose
bounding boxes exceed the row-extent scratch, hole boxes on 64-bit word seams, more than 256 large labels on a plane,
2x2 configuration codes on noise, a 2048 x 2048 plane, float64 weights, column-bit gating and batches of planes."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage as ndi

from arcadia_microscopy_tools_amd import _hip, hipops
from arcadia_microscopy_tools_amd.channels import DAPI, FITC
from arcadia_microscopy_tools_amd.masks import DEFAULT_CELL_PROPERTY_NAMES, SegmentationMask
from oracle import regionprops as orp
from oracle import skops

pytestmark = pytest.mark.gpu

EXTENDED = ["euler_number", "perimeter_crofton", "area_filled", "feret_diameter_max", "area_bbox", "extent",
            "equivalent_diameter_area", "centroid_local", "inertia_tensor", "inertia_tensor_eigvals"]
PROPS = list(DEFAULT_CELL_PROPERTY_NAMES) + EXTENDED
IPROPS = ["intensity_mean", "intensity_max", "intensity_min", "intensity_std", "centroid_weighted",
          "centroid_weighted_local"]
# exact on both sides: integer counts, exact integer hulls, feret_diameter_max (its square is a multiple of 1/4) and
# centroid_local (exact integer moment sums, one rounding)
EXACT = ("label", "area", "bbox", "area_convex", "solidity", "euler_number", "area_filled", "feret_diameter_max",
         "centroid_local", "area_bbox", "extent")
REL12 = ("perimeter_crofton", "inertia_tensor")


def _ulp_close(got, exact, ulps=2):
    """|got - exact| <= ulps * ulp(exact) for every entry; ``exact`` holds Fractions (or None for NaN)."""
    for i, (g, e) in enumerate(zip(got.tolist(), exact)):
        if e is None:
            assert np.isnan(g), i
            continue
        assert np.isfinite(g), i
        assert abs(Fraction(g) - e) <= ulps * Fraction(np.spacing(abs(float(e)))), (i, g, float(e))


def _exact_weighted(labels, inten):
    """centroid_weighted-0/-1 and centroid_weighted_local-0/-1 per label as exact rationals (None: zero weight)."""
    out = {k: [] for k in _hip.RPX_WCOLS}
    for i, sl in enumerate(ndi.find_objects(labels)):
        if sl is None:
            continue
        img = labels[sl] == i + 1
        s, sy, sx = orp.weighted_sums_exact(img, inten[sl])
        ly, lx = (None, None) if s == 0 else (Fraction(sy, s), Fraction(sx, s))
        out["centroid_weighted_local-0"].append(ly)
        out["centroid_weighted_local-1"].append(lx)
        out["centroid_weighted-0"].append(None if ly is None else ly + sl[0].start)
        out["centroid_weighted-1"].append(None if lx is None else lx + sl[1].start)
    return out


def _height_sum(labels):
    """Sum of the bounding-box heights of the labels (the row-extent entries the hull kernels need)."""
    return sum(sl[0].stop - sl[0].start for sl in ndi.find_objects(np.asarray(labels)) if sl is not None)


def _compare(got, want, exact_weighted=None):
    """Device table vs expected table (scikit-image golden or the oracle) at the tolerances of each column."""
    assert list(got) == list(want)
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, k
        if k.startswith("centroid_weighted") and exact_weighted is not None and k.rsplit("_", 1)[1] in exact_weighted:
            _ulp_close(g, exact_weighted[k.rsplit("_", 1)[1]][k.rsplit("_", 1)[0]])
        elif k.startswith(EXACT):
            assert np.array_equal(g, w, equal_nan=True), (k, np.nonzero(~((g == w) | (np.isnan(g) & np.isnan(w)))))
        elif k.startswith(REL12):
            scale = np.abs(w).max() if w.size else 1.0
            np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12 * scale, err_msg=k)
        elif k == "axis_minor_length":
            # 4 sqrt(l2): scikit-image's eigvalsh leaves ~1e-16 l1 of rounding in l2 of collinear pixels, which the
            # square root lifts to ~1e-6 where the device's exact moments give 0; compare l2 = (length / 4)^2 at the
            # tolerance of inertia_tensor_eigvals
            l2g, l2w = (g / 4) ** 2, (w / 4) ** 2
            scale = np.abs(l2w).max() if w.size else 1.0
            np.testing.assert_allclose(l2g, l2w, rtol=1e-12, atol=1e-12 * scale, err_msg=k)
        elif k.startswith("orientation"):
            # 0.18.3's orientation of exactly symmetric regions is unpinned
            sym = np.isclose(np.abs(w), np.pi / 4)
            np.testing.assert_allclose(g[~sym], w[~sym], rtol=0, atol=1e-8, err_msg=k)
        else:
            assert np.array_equal(np.isnan(g), np.isnan(w)), k
            scale = np.nanmax(np.abs(w)) if np.isfinite(w).any() else 1.0
            np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-12 * max(scale, 1.0), err_msg=k)


def _oracle(labels, channels, props=PROPS, iprops=IPROPS, remove_edge_cells=False):
    lab = np.asarray(labels, np.int64)
    if remove_edge_cells:
        lab = skops.clear_border(lab)
    lab = skops.relabel_sequential(lab)
    chans = {c.name: v for c, v in channels.items()}
    return lab, orp.cell_properties(lab, chans, props, iprops if chans else [])


def _frag(golden):
    g = golden("props_frag")
    return g, g["frag__labels"], {DAPI: g["frag__dapi"], FITC: g["frag__fitc"]}


def test_frag_golden_matches_scikit_image(golden):
    g, labels, channels = _frag(golden)
    assert _height_sum(labels) > labels.size  # past the row-extent scratch of the hull kernels
    m = SegmentationMask(labels, channels, remove_edge_cells=False, property_names=PROPS,
                         intensity_property_names=IPROPS)
    want = {str(k): g[f"frag__{k}"] for k in g["frag__keys"]}
    _compare(m.cell_properties, want, {"dapi": _exact_weighted(labels, g["frag__dapi"])})
    for k in ("area_convex", "solidity", "feret_diameter_max"):
        assert np.isfinite(m.cell_properties[k]).all(), k


def test_frag_default_columns_and_remove_edge_cells(golden):
    g, labels, channels = _frag(golden)
    m = SegmentationMask(labels, channels, remove_edge_cells=False)
    want = {str(k): g[f"frag__{k}"] for k in g["frag__keys"]}
    got = m.cell_properties
    _compare(got, {k: want[k] for k in got})
    cleared = SegmentationMask(labels, channels, remove_edge_cells=True, property_names=PROPS,
                               intensity_property_names=IPROPS)
    lab, ref = _oracle(labels, channels, remove_edge_cells=True)
    assert np.array_equal(cleared.label_image, lab)
    assert _height_sum(lab) > lab.size
    _compare(cleared.cell_properties, ref, {"dapi": _exact_weighted(lab, g["frag__dapi"])})


@pytest.mark.parametrize("seed,shape,k", [(0, (32, 32), 100), (1, (40, 72), 150), (2, (23, 61), 97),
                                          (3, (64, 65), 400)])
def test_random_fragmented_labels(seed, shape, k):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, k + 1, shape)
    labels[rng.random(shape) < 0.3] = 0
    labels[labels == k // 2] = 0  # a gap in the numbering
    inten = rng.integers(0, 65536, shape).astype(np.uint16)
    m = SegmentationMask(labels, {DAPI: inten}, remove_edge_cells=False, property_names=PROPS,
                         intensity_property_names=IPROPS)
    lab, ref = _oracle(labels, {DAPI: inten})
    assert _height_sum(lab) > lab.size
    _compare(m.cell_properties, ref, {"dapi": _exact_weighted(lab, inten)})


def test_smallest_fragmented_case_from_the_issue():
    labels = np.random.default_rng(0).integers(1, 101, (32, 32))
    props = SegmentationMask(labels, remove_edge_cells=False).cell_properties
    _, ref = _oracle(labels, {}, props=list(DEFAULT_CELL_PROPERTY_NAMES))
    for k in ("area_convex", "solidity"):
        assert np.array_equal(props[k], ref[k]), k


def _frame_plane(rng, sizes, H, W):
    """Rectangular frames of the given (h, w) with random interior noise, packed left to right, top to bottom."""
    labels = np.zeros((H, W), np.int64)
    y = x = 1
    row_h = 0
    for i, (h, w) in enumerate(sizes):
        if x + w + 1 > W:
            y, x, row_h = y + row_h + 1, 1, 0
        assert y + h + 1 <= H
        box = rng.random((h, w)) < rng.uniform(0.3, 0.7)
        box[0, :] = box[-1, :] = box[:, 0] = box[:, -1] = True
        # walls around the word seams so that holes sit next to them
        for c in (62, 63, 64, 65, 126, 127, 128, 129):
            if c < w - 1 and rng.random() < 0.5:
                box[1:-1, c] = rng.random(h - 2) < 0.5
        labels[y:y + h, x:x + w][box] = i + 1
        x += w + 1
        row_h = max(row_h, h)
    return labels


@pytest.mark.parametrize("seed", [0, 1])
def test_hole_boxes_at_word_boundaries(seed):
    rng = np.random.default_rng(seed)
    dims = [63, 64, 65, 128, 129]
    sizes = [(h, w) for h in dims for w in dims]
    rng.shuffle(sizes)
    labels = _frame_plane(rng, sizes[:12], 420, 530)
    m = SegmentationMask(labels, remove_edge_cells=False, property_names=["label", "area"] + EXTENDED)
    _, ref = _oracle(labels, {}, props=["label", "area"] + EXTENDED)
    _compare(m.cell_properties, ref)
    assert (ref["area_filled"] > ref["area"]).sum() >= 10


def test_more_than_256_large_labels_on_one_plane():
    rng = np.random.default_rng(5)
    H, W = 300, 300
    labels = np.zeros((H, W), np.int64)
    n = 0
    for y in range(0, H - 3, 4):
        for x in range(0, W - 70, 72):
            n += 1
            labels[y:y + 3, x:x + 70] = n  # a 3 x 70 frame with a hole of random length in its middle row
            a = int(rng.integers(1, 60))
            labels[y + 1, x + a:x + a + int(rng.integers(1, 69 - a))] = 0
    assert n > 256
    names = ["label", "area", "area_filled", "euler_number", "feret_diameter_max"]
    m = SegmentationMask(labels, remove_edge_cells=False, property_names=names)
    _, ref = _oracle(labels, {}, props=names)
    _compare(m.cell_properties, ref)


@pytest.mark.parametrize("case", ["noise", "checker", "diagonal"])
def test_configuration_codes(case):
    rng = np.random.default_rng(11)
    H, W = 61, 130
    if case == "noise":
        labels = skops.label(rng.random((H, W)) < 0.45)  # 8-connected components, many on the frame
    elif case == "checker":
        yy, xx = np.mgrid[:H, :W]
        labels = np.where((yy + xx) % 2 == 0, 1 + (xx >= W - 17), 0)  # one 8-connected checkerboard to x = W - 1
    else:
        labels = np.zeros((H, W), np.int64)
        for i in range(30):  # pieces of one label touching only at corners, and two labels meeting at a corner
            y, x = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 4))
            labels[y:y + 2, x:x + 2] = 1 + i % 3
            labels[y + 2:y + 4, x + 2:x + 4] = 1 + (i + i % 2) % 3
        labels[H - 3:, W - 3:] = 2
        labels[H - 4, W - 4] = 2
    names = ["label", "area", "euler_number", "perimeter_crofton", "area_filled"]
    m = SegmentationMask(labels, remove_edge_cells=False, property_names=names)
    _, ref = _oracle(labels, {}, props=names)
    _compare(m.cell_properties, ref)


def test_2048_plane_with_huge_labels():
    H = W = 2048
    yy, xx = np.mgrid[:H, :W]
    labels = np.zeros((H, W), np.int64)
    r2 = (yy - 1023.5) ** 2 + (xx - 1100.25) ** 2
    labels[(r2 <= 1024.0 ** 2) & (r2 >= 990.0 ** 2)] = 1  # a ring over the full height, clipped at the frame
    box = np.zeros((600, 600), bool)  # a closed square spiral: one long corridor of background
    for i in range(0, 300, 4):
        box[i, i:600 - i] = box[599 - i, i:600 - i] = True
        box[i:600 - i, i] = box[i:600 - i, 599 - i] = True
        if i + 2 < 300:
            box[i + 2, i + 1] = False if i else True
    labels[700:1300, 750:1350][box] = 2
    labels[100:140, 1900:2048] = 3  # on the right frame
    inten = np.full((H, W), 65535, np.uint16)
    inten[labels == 3] = np.arange((labels == 3).sum()) % 65536
    names = ["label", "area", "bbox", "area_convex", "euler_number", "area_filled", "feret_diameter_max",
             "centroid_local"]
    m = SegmentationMask(labels, {DAPI: inten}, remove_edge_cells=False, property_names=names,
                         intensity_property_names=["centroid_weighted", "centroid_weighted_local"])
    _, ref = _oracle(labels, {DAPI: inten}, props=names, iprops=["centroid_weighted", "centroid_weighted_local"])
    assert ref["bbox-2"][0] - ref["bbox-0"][0] == H and ref["area_filled"][1] > ref["area"][1]
    _compare(m.cell_properties, ref, {"dapi": _exact_weighted(labels, inten)})


def test_float64_weights_with_negative_values_and_zero_total():
    rng = np.random.default_rng(3)
    labels = _frame_plane(rng, [(20, 30), (65, 70), (5, 5), (1, 9)], 100, 200)
    labels[labels == 3] = 0
    labels[50:53, 150:160] = 3
    inten = rng.normal(0.0, 100.0, labels.shape)
    inten[labels == 3] = 0.0
    m = SegmentationMask(labels, {FITC: inten}, remove_edge_cells=False, property_names=["label"],
                         intensity_property_names=["centroid_weighted", "centroid_weighted_local"])
    _, ref = _oracle(labels, {FITC: inten}, props=["label"], iprops=["centroid_weighted", "centroid_weighted_local"])
    got = m.cell_properties
    assert np.isnan(got["centroid_weighted-0_fitc"]).sum() == 1
    _compare(got, ref)


def test_each_column_bit_alone_equals_all_bits_together(golden):
    from arcadia_microscopy_tools_amd.device import get_context

    ctx = get_context()
    g = golden("props_ext")
    syn = g["syn__labels"].astype(np.int32)
    mx = int(syn.max())
    inten = ctx.asarray(np.stack([g["syn__dapi"]])[None])
    planes = ctx.asarray(syn[None])
    names = list(_hip.RPX_BITS)
    t_all, w_all = hipops.regionprops_ext(planes, mx, names, intensity=inten)
    t_all, w_all = t_all.numpy(), w_all.numpy()
    col = {c: i for i, c in enumerate(_hip.RPX_COLS)}
    for name in names:
        if name in ("centroid_weighted", "centroid_weighted_local"):
            _, w = hipops.regionprops_ext(planes, mx, [name], intensity=inten)
            assert np.array_equal(w.numpy(), w_all, equal_nan=True), name
            continue
        t, _ = hipops.regionprops_ext(planes, mx, [name])
        t = t.numpy()
        cols = [i for c, i in col.items() if c == name or c.startswith(name + "-")]
        assert cols, name
        assert np.array_equal(t[..., cols], t_all[..., cols], equal_nan=True), name


def test_batch_with_one_overflowing_plane_equals_one_call_per_plane(golden):
    from arcadia_microscopy_tools_amd.device import get_context

    ctx = get_context()
    g = golden("props_frag")
    frag = g["frag__labels"].astype(np.int32)
    rng = np.random.default_rng(9)
    conn = _frame_plane(rng, [(30, 70), (65, 64), (10, 129), (48, 250)], frag.shape[0], frag.shape[1])
    gaps = np.where(conn > 0, conn * 7 + 3, 0).astype(np.int32)
    planes = np.stack([gaps, frag, conn.astype(np.int32), np.zeros_like(frag)])
    mx = int(planes.max())
    names = list(_hip.RPX_BITS)[:7]
    t = hipops.regionprops_ext(ctx.asarray(planes), mx, names)[0].numpy()
    base = hipops.regionprops(ctx.asarray(planes), mx).numpy()
    feret = _hip.RPX_COLS.index("feret_diameter_max")
    ac = _hip.RP_COLS.index("area_convex")
    for i in range(planes.shape[0]):
        t1 = hipops.regionprops_ext(ctx.asarray(planes[i]), mx, names)[0].numpy()[0]
        assert np.array_equal(t[i], t1, equal_nan=True), i
        b1 = hipops.regionprops(ctx.asarray(planes[i]), mx).numpy()[0]
        assert np.array_equal(base[i], b1, equal_nan=True), i
    # the planes beside the overflowing one measure what the oracle does
    ref = orp.regionprops_table(conn, properties=["area_convex", "feret_diameter_max"])
    present = np.unique(gaps[gaps > 0]) - 1
    assert np.array_equal(t[0][present, feret], ref["feret_diameter_max"])
    assert np.array_equal(base[0][present, ac], ref["area_convex"])
    assert np.array_equal(t[2][:conn.max(), feret], ref["feret_diameter_max"])
    assert not t[3].any()
