"""``expand_labels`` on the device (``hipops`` / ``operations`` / ``SegmentationMask.expanded`` / ``.ring``) against the
test-side reference of tests/expand_labels_reference.py: the two-pass evaluation of the rule on every pixel, and
scipy's support on every pixel."""
import numpy as np
import pytest

import expand_labels_reference as ref
from arcadia_microscopy_tools_amd import hipops, operations
from arcadia_microscopy_tools_amd.channels import BRIGHTFIELD, DAPI, FITC, TRITC
from arcadia_microscopy_tools_amd.device import DeviceArray, get_context
from arcadia_microscopy_tools_amd.masks import SegmentationMask
from arcadia_microscopy_tools_amd.pipeline import ImageOperation, Pipeline

pytestmark = pytest.mark.gpu

NUC_CHANNELS = (BRIGHTFIELD, DAPI, FITC, TRITC)
# (shape, discs): 1x1, 1xN, Nx1, widths on either side of the 64-pixel word seams, a width with W % 16 != 0
SHAPES = [((1, 1), 1), ((1, 70), 3), ((70, 1), 3), ((37, 63), 6), ((40, 64), 8), ((33, 65), 9), ((50, 129), 14),
          ((45, 77), 9), ((130, 200), 25)]


def _device_expand(labels, distance, ring=False):
    d = get_context().asarray(np.ascontiguousarray(labels), dtype=np.int32)
    return hipops.expand_labels(d, distance, ring=ring).numpy(dtype=labels.dtype)


def _check_plane(labels, distances):
    d2, nearest, _ = ref.nearest_two_pass(labels)
    dev = get_context().asarray(np.ascontiguousarray(labels), dtype=np.int32)
    for distance in distances:
        want = ref.apply_bound(labels, d2, nearest, distance)
        got = hipops.expand_labels(dev, distance).numpy(dtype=labels.dtype)
        diff = int((got != want).sum())
        print(f"shape {labels.shape} distance {distance}: {diff} pixels differ from the two-pass rule")
        assert diff == 0, (labels.shape, distance)
        assert np.array_equal(got != 0, ref.expand_scipy(labels, distance) != 0), (labels.shape, distance)
        annulus = hipops.expand_labels(dev, distance, ring=True).numpy(dtype=labels.dtype)
        assert np.array_equal(annulus, np.where(labels == 0, got, 0)), (labels.shape, distance)


@pytest.mark.parametrize("shape,n_discs", SHAPES)
def test_exact_on_small_planes(shape, n_discs):
    labels = ref.disc_scene(shape, n_discs, seed=100 + shape[0] + shape[1])
    larger_than_the_image = 2 * max(shape) + 3
    _check_plane(labels, ref.DISTANCES + (larger_than_the_image,))


def _nuclei_plane_2048(golden):
    """tests/golden/props_ext.npz::nuc__labels (256 x 256, 22 nuclei) tiled 8 x 8, every tile with labels of its own."""
    tile = golden("props_ext")["nuc__labels"]
    k = int(tile.max())
    plane = np.zeros((2048, 2048), np.int64)
    for ty in range(8):
        for tx in range(8):
            plane[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256] = np.where(tile > 0, tile + k * (ty * 8 + tx), 0)
    return plane


def test_exact_on_a_2048_nuclei_plane(golden):
    _check_plane(_nuclei_plane_2048(golden), ref.DISTANCES + (3000,))


def test_label_values():
    rng = np.random.default_rng(5)
    # non-sequential values up to 2**31 - 2, discs drawn over one another (touching labels)
    labels = ref.disc_scene((90, 150), 30, seed=3, max_label=2 ** 31 - 2)
    labels[labels == labels.max()] = 2 ** 31 - 2
    assert labels.max() == 2 ** 31 - 2 and len(np.unique(labels)) > 10
    _check_plane(labels, (1, 3, 7, 40))
    # two labels that touch along a line, and single labelled pixels
    touching = np.zeros((40, 100), np.int64)
    touching[10:30, 20:50] = 70000
    touching[10:30, 50:80] = 9
    touching[rng.integers(0, 40, 6), rng.integers(0, 100, 6)] = rng.integers(1, 10 ** 6, 6)
    _check_plane(touching, (0, 1, 2.9999, 12, 300))
    for distance in (0, 3, 50):
        empty = np.zeros((70, 131), np.int64)
        assert not _device_expand(empty, distance).any()
        full = rng.integers(1, 1000, (70, 131))
        assert np.array_equal(_device_expand(full, distance), full)
        assert not _device_expand(full, distance, ring=True).any()
    assert not _device_expand(full, -1).any()


def test_batch_equals_single_planes_and_repeats_bit_for_bit():
    planes = np.stack([ref.disc_scene((75, 140), 4 + 5 * i, seed=40 + i) for i in range(5)])
    planes[3] = 0
    ctx = get_context()
    stack = ctx.asarray(planes, dtype=np.int32)
    for distance in (1.5, 3, 12, 40):
        whole = hipops.expand_labels(stack, distance).numpy()
        again = hipops.expand_labels(stack, distance).numpy()
        assert whole.dtype == np.int32 and whole.shape == planes.shape
        assert np.array_equal(whole, again)
        for i in range(len(planes)):
            single = hipops.expand_labels(ctx.asarray(planes[i], dtype=np.int32), distance).numpy()
            assert np.array_equal(whole[i], single), (distance, i)
            assert np.array_equal(whole[i], ref.expand_two_pass(planes[i], distance)), (distance, i)
        rings = hipops.expand_labels(stack, distance, ring=True).numpy()
        assert np.array_equal(rings, np.where(planes == 0, whole, 0))


def test_hipops_argument_checks():
    ctx = get_context()
    lab = ctx.asarray(np.zeros((8, 8), np.int32))
    with pytest.raises(TypeError):
        hipops.expand_labels(ctx.asarray(np.zeros((8, 8), np.uint16)), 1)
    with pytest.raises(ValueError):
        hipops.expand_labels(lab, 1, out=lab)
    with pytest.raises(ValueError):
        hipops.expand_labels(lab, 1, out=ctx.empty((8, 9), np.int32))
    with pytest.raises(ValueError):
        hipops.expand_labels(ctx.asarray(np.zeros((2, 2, 8, 8), np.int32)), 1)
    out = ctx.empty((8, 8), np.int32)
    assert hipops.expand_labels(lab, 1, out=out) is out


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.uint16, np.bool_])
def test_pipeline_on_numpy_and_device_input(dtype):
    labels = ref.disc_scene((96, 130), 12, seed=9)
    image = (labels > 0) if dtype is np.bool_ else labels.astype(dtype)
    want = ref.expand_two_pass(image.astype(np.int64), 3).astype(dtype)
    pipe = Pipeline([ImageOperation(operations.expand_labels, distance=3)])
    got = pipe(image)
    assert isinstance(got, np.ndarray) and got.dtype == np.dtype(dtype) and np.array_equal(got, want)
    direct = operations.expand_labels(image, 3)
    assert direct.dtype == np.dtype(dtype) and np.array_equal(direct, want)
    resident = pipe(get_context().asarray(image.astype(np.int32)))
    assert isinstance(resident, DeviceArray) and resident.dtype == np.int32
    assert np.array_equal(resident.numpy(), want.astype(np.int32))
    assert np.array_equal(operations.expand_labels(image), ref.expand_two_pass(image.astype(np.int64), 1).astype(dtype))


def _nuclei_mask(golden, **kw):
    g = golden("props_ext")
    fov = g["nuc__fov"]
    channels = {c: fov[i] for i, c in enumerate(NUC_CHANNELS)}
    kw.setdefault("property_names", [str(p) for p in g["props"]])
    kw.setdefault("intensity_property_names", [str(p) for p in g["iprops"]])
    return SegmentationMask(g["nuc__labels"], channels, remove_edge_cells=False, **kw), channels, kw


@pytest.mark.parametrize("distance", [3, 12])
def test_expanded_mask(golden, distance):
    parent, channels, kw = _nuclei_mask(golden)
    grown = parent.expanded(distance)
    assert grown.num_cells == parent.num_cells
    assert np.array_equal(grown.parent_labels, np.arange(1, parent.num_cells + 1)) and grown.parent_labels.dtype == np.int64
    assert parent.parent_labels is None
    assert grown.remove_edge_cells is False and grown.outline_extractor == parent.outline_extractor
    assert grown.property_names == parent.property_names
    assert grown.intensity_property_names == parent.intensity_property_names
    assert list(grown.intensity_image_dict) == list(parent.intensity_image_dict)
    props = grown.cell_properties
    assert "mask_image" not in grown.__dict__ and "label_image" not in grown.__dict__  # measured without a download
    want_image = operations.expand_labels(parent.label_image, distance)
    assert want_image.dtype == np.int64
    assert np.array_equal(want_image, ref.expand_two_pass(parent.label_image, distance))
    assert np.array_equal(grown.label_image, want_image) and grown.label_image.dtype == np.int64
    assert np.array_equal(grown.mask_image, want_image)
    host = SegmentationMask(want_image, channels, remove_edge_cells=False, **kw).cell_properties
    assert list(props) == list(host)
    for key in ("euler_number", "feret_diameter_max", "inertia_tensor-0-1", "centroid_weighted-0_dapi", "intensity_mean_fitc"):
        assert key in props
    for key, column in host.items():
        assert props[key].dtype == column.dtype and np.array_equal(props[key], column, equal_nan=True), key
    assert (props["area"] > parent.cell_properties["area"]).all()
    assert len(grown.cell_outlines) == parent.num_cells
    assert "SegmentationMask(shape=(256, 256)" in repr(parent.expanded(1))
    with pytest.raises(AttributeError):
        grown.mask_image = want_image
    with pytest.raises(ValueError):
        parent.expanded(-1)


def _enclosed_scene():
    """A disc (label 1) inside a closed band of label 2 that touches it, and a free disc (label 3)."""
    yy, xx = np.mgrid[0:80, 0:120]
    rr = (yy - 40) ** 2 + (xx - 40) ** 2
    labels = np.zeros((80, 120), np.int64)
    labels[rr <= 14 ** 2] = 2
    labels[rr <= 8 ** 2] = 1
    labels[(yy - 30) ** 2 + (xx - 95) ** 2 <= 6 ** 2] = 3
    return labels


def test_ring_mask(golden):
    parent, channels, kw = _nuclei_mask(golden)
    distance = 5
    ring = parent.ring(distance)
    grown = ref.expand_two_pass(parent.label_image, distance)
    annulus = np.where(parent.label_image == 0, grown, 0)
    present = np.unique(annulus[annulus > 0])
    lut = np.zeros(parent.num_cells + 1, np.int64)
    lut[present] = np.arange(1, len(present) + 1)
    props = ring.cell_properties
    assert "mask_image" not in ring.__dict__
    assert ring.num_cells == len(present)
    assert np.array_equal(ring.parent_labels, present) and ring.parent_labels.dtype == np.int64
    assert np.array_equal(ring.label_image, lut[annulus]) and ring.label_image.dtype == np.int64
    big, small = parent.expanded(distance).cell_properties["area"], parent.cell_properties["area"]
    assert np.array_equal(props["area"], big[ring.parent_labels - 1] - small[ring.parent_labels - 1])
    host = SegmentationMask(lut[annulus], channels, remove_edge_cells=False, **kw).cell_properties
    assert list(props) == list(host)
    for key, column in host.items():
        assert np.array_equal(props[key], column, equal_nan=True), key


def test_ring_skips_enclosed_cells_and_raises_when_none_is_left():
    labels = _enclosed_scene()
    parent = SegmentationMask(labels, remove_edge_cells=False)
    ring = parent.ring(3)
    assert ring.num_cells == 2 and np.array_equal(ring.parent_labels, [2, 3])
    annulus = np.where(labels == 0, ref.expand_two_pass(labels, 3), 0)
    assert not (annulus == 1).any()
    assert np.array_equal(ring.label_image, np.where(annulus == 2, 1, np.where(annulus == 3, 2, 0)))
    grown = parent.expanded(3)
    assert grown.num_cells == 3
    assert grown.cell_properties["area"][0] == parent.cell_properties["area"][0]
    assert np.array_equal(ring.cell_properties["area"],
                          (grown.cell_properties["area"] - parent.cell_properties["area"])[[1, 2]])
    filled = np.ones((40, 60), np.int64)
    filled[:, 30:] = 2
    with pytest.raises(ValueError, match="contains no cells"):
        SegmentationMask(filled, remove_edge_cells=False).ring(4)
    with pytest.raises(ValueError, match="contains no cells"):
        parent.ring(0)
