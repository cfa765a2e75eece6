"""``remove_small_objects`` / ``remove_small_holes`` on the device against the reference (scipy.ndimage.label +
np.bincount) and scikit-image's golden answers, byte for byte: the sweep of tests/area_filters_cases.py (every shape,
generator, structure, operator and size, three ways each); both sides of the count on spirals and on components chosen
from random planes, on the run-table and on the general path; connectivity; truth-value bytes; the C ABI's refusals and
the unchanged codes 0..4; ``operations.*`` and a ``Pipeline``; the classical chain with ``min_size``; and all sweep cases
once more in a child process with the scratch arena poisoned."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage as ndi

import area_filters_cases as cases
import area_filters_reference as ref
import poison_child
from arcadia_microscopy_tools_amd import _hip, hipops, operations
from arcadia_microscopy_tools_amd.device import DeviceArray, get_context
from arcadia_microscopy_tools_amd.model import SegmentationModel
from arcadia_microscopy_tools_amd.pipeline import ImageOperation, Pipeline
from arcadia_microscopy_tools_amd.segment import FovSegmenter

pytestmark = pytest.mark.gpu

# meant to be ten times the in-process run of all sweep cases on the MI355X.  That run is not measured yet: until it is,
# the limit of the fill-holes child (tests/test_gpu_fill_holes.py), whose sweep has the same shapes and fewer calls
CHILD_TIMEOUT_S = 120
DEVICE = {"objects": hipops.remove_small_objects, "holes": hipops.remove_small_holes}
_RESULTS: dict = {}
_GOLDEN: dict = {}


@pytest.fixture(scope="module")
def ctx():
    return get_context()


def _shape_result(ctx, shape):
    if shape not in _RESULTS:
        if not _GOLDEN:
            _GOLDEN.update(cases.golden_cases())
        _RESULTS[shape] = cases.run_shape(ctx, shape, golden=_GOLDEN)
    return _RESULTS[shape]


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sweep_matches_the_reference(ctx, shape):
    res = _shape_result(ctx, shape)
    nplanes = len(ref.planes(shape))
    assert nplanes >= 6 and res["calls"] == 2 * 2 * 6 * (2 * nplanes + (nplanes + 2) // 3), shape
    assert not res["mismatches"], f"{len(res['mismatches'])} outputs differ; the first: {res['mismatches'][:10]}"


def test_sweep_meets_the_golden_file(ctx):
    """The sweep holds the golden planes of (70, 131), (33, 40) and (64, 64) at sizes 2, 5 and 17."""
    hits = sum(_shape_result(ctx, s)["golden"] for s in ref.GOLDEN_SHAPES)
    assert hits == 4 * 2 * 2 * 3  # four golden planes are sweep planes; structures, operators, sizes


def _offset_view(ctx, plane, offset):
    """The plane on the device at an address ``offset`` bytes past a 256-byte boundary."""
    H, W = plane.shape
    flat = np.zeros(offset + H * W, np.uint8)
    flat[offset:] = plane.reshape(-1)
    return ctx.asarray(flat)[offset:offset + H * W].reshape(H, W)


def _both_paths(ctx, plane):
    """[(path name, device plane)]: 16-byte aligned (the run tables, where the width allows them) and one byte further
    on (always the general path)."""
    aligned, moved = ctx.asarray(plane), _offset_view(ctx, plane, 1)
    assert aligned.ptr % 16 == 0 and moved.ptr % 16 == 1
    return [("aligned", aligned), ("offset 1", moved)]


@pytest.mark.parametrize("shape", ref.SPIRAL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_spiral_both_sides_of_the_count(ctx, shape):
    """One wall component and one corridor component that wind through every tile and seam: a partial sum lost or added
    twice moves the count off the exact size."""
    p = ref.spiral(shape, open=True)
    wall, corridor = int(p.sum()), int((p == 0).sum())
    for path, d in _both_paths(ctx, p):
        for conn in (1, 2):
            got = lambda fn, s: fn(d, s, conn).numpy(dtype=np.uint8)  # noqa: E731
            assert np.array_equal(got(hipops.remove_small_objects, wall), p), (shape, path, conn, "wall kept")
            assert not got(hipops.remove_small_objects, wall + 1).any(), (shape, path, conn, "wall removed")
            assert np.array_equal(got(hipops.remove_small_holes, corridor), p), (shape, path, conn, "corridor kept")
            assert got(hipops.remove_small_holes, corridor + 1).all(), (shape, path, conn, "corridor filled")
            if wall > 2:
                assert np.array_equal(got(hipops.remove_small_objects, wall - 1), p)
                assert np.array_equal(got(hipops.remove_small_holes, corridor - 1), p)


@pytest.mark.parametrize("shape", [(16, 16), (33, 40), (64, 64), (65, 128), (70, 131), (66, 320), (256, 256)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_component_both_sides_of_the_count(ctx, shape):
    """The largest component of each polarity of every random plane: kept at exactly its size, gone at one more."""
    for i, seed in enumerate(ref.SEEDS):
        P = ref.Plane(ref.random(shape, ref.DENSITIES[i], seed))
        for path, d in _both_paths(ctx, P.plane):
            for sname, _ in ref.STRUCTURES:
                conn = ref.CONNECTIVITY[sname]
                for op, areas in (("objects", P.fg[sname]), ("holes", P.bg[sname])):
                    a = int(areas.max())
                    if a == 0:
                        continue
                    comp = areas == a
                    at = DEVICE[op](d, a, conn).numpy(dtype=np.uint8)
                    above = DEVICE[op](d, a + 1, conn).numpy(dtype=np.uint8)
                    tag = (shape, seed, path, sname, op, a)
                    assert np.array_equal(at, P.want(op, sname, a)), tag
                    assert np.array_equal(above, P.want(op, sname, a + 1)), tag
                    keep = 1 if op == "objects" else 0  # an object kept stays 1, a hole kept stays 0
                    assert (at[comp] == keep).all() and (above[comp] == 1 - keep).all(), tag


def test_checkerboard_connectivity(ctx):
    """Singletons under the cross, one component (of each colour) under all-ones."""
    for shape in ((16, 16), (33, 40), (70, 131), (64, 64)):
        p = ref.checkerboard(shape)
        ones, zeros = int(p.sum()), int((p == 0).sum())
        for path, d in _both_paths(ctx, p):
            assert not hipops.remove_small_objects(d, 2, 1).numpy().any(), (shape, path)
            assert hipops.remove_small_holes(d, 2, 1).numpy().all(), (shape, path)
            assert np.array_equal(hipops.remove_small_objects(d, ones, 2).numpy(dtype=np.uint8), p), (shape, path)
            assert not hipops.remove_small_objects(d, ones + 1, 2).numpy().any(), (shape, path)
            assert np.array_equal(hipops.remove_small_holes(d, zeros, 2).numpy(dtype=np.uint8), p), (shape, path)
            assert hipops.remove_small_holes(d, zeros + 1, 2).numpy().all(), (shape, path)


@pytest.mark.parametrize("shape", [(16, 16), (17, 32), (33, 40), (65, 128), (70, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_truth_value_bytes(ctx, shape):
    """Foreground is byte != 0: bytes from {1, 2, 255} give the result of the 0 / 1 plane, size 1 included."""
    for name, plane in ref.planes(shape):
        loud = ref.truth_bytes(plane, 7)
        P = ref.Plane(plane)
        for path, d in _both_paths(ctx, loud) + [("stack", ctx.asarray(np.stack([loud, loud]))[1])]:
            for sname, _ in ref.STRUCTURES:
                for op in ref.OPERATORS:
                    for size in (1, 3, 17):
                        got = DEVICE[op](d, size, ref.CONNECTIVITY[sname]).numpy(dtype=np.uint8)
                        assert np.array_equal(got, P.want(op, sname, size)), (shape, name, path, sname, op, size)


def test_result_is_a_bool_mask_out_is_used_and_repeats_are_identical(ctx):
    plane = ref.random((70, 131), 0.65, 1)
    d = ctx.asarray(plane.astype(bool))
    for op, fn in DEVICE.items():
        got = fn(d, 5)
        assert got.is_bool and got.dtype == np.uint8 and got.numpy().dtype == np.bool_
        assert np.array_equal(got.numpy(dtype=np.uint8), ref.apply(op, plane, 5, ref.CROSS))
        out = ctx.empty(plane.shape, np.uint8)
        assert fn(d, 5, 2, out=out) is out and out.is_bool
        assert np.array_equal(out.numpy(dtype=np.uint8), ref.apply(op, plane, 5, ref.FULL))
        # sizes that can remove nothing copy a bool mask; a size beyond the plane is clamped
        for size in (1, 0, -4):
            same = fn(d, size, out=out)
            assert same is out and np.array_equal(out.numpy(dtype=np.uint8), plane)
        huge = fn(d, 2**40).numpy(dtype=np.uint8)
        assert np.array_equal(huge, ref.apply(op, plane, plane.size + 1, ref.CROSS))
        for shape in ((256, 256), (70, 131)):
            big = ctx.asarray(ref.random(shape, 0.5, 0))
            first = fn(big, 17).numpy(dtype=np.uint8)
            for _ in range(3):
                assert np.array_equal(fn(big, 17).numpy(dtype=np.uint8), first)
    for shape in ((0, 33, 40), (0, 5), (3, 0)):
        got = hipops.remove_small_objects(ctx.empty(shape, np.uint8), 4)
        assert got.shape == shape and got.is_bool and got.numpy().shape == shape


def test_c_abi(ctx):
    plane = ref.random((33, 40), 0.65, 1)
    d = ctx.asarray(plane)
    stack = ctx.asarray(np.stack([plane] * 3))
    lib = _hip.load_library()

    def call(fp, op, out, size, src=d, n=1):
        fp = np.ascontiguousarray(fp, np.uint8)
        return lib.amt_binary_morph(ctx.handle, src.ptr, out.ptr, n, 33, 40, fp.ctypes.data_as(ctypes.c_void_p), fp.shape[0],
                                    fp.shape[1], op, size)

    o = ctx.empty((33, 40), np.uint8)
    for code, op in ((5, "objects"), (6, "holes")):
        for sname, st in ref.STRUCTURES:
            for size in (1, 4, 33 * 40 + 1):
                assert call(st, code, o, size) == 0
                assert np.array_equal(o.numpy(dtype=np.uint8), ref.apply(op, plane, size, st)), (code, sname, size)
        assert call(ref.CROSS, code, o, 0) == -1
        assert "size" in lib.amt_last_error().decode()
        assert call(ref.CROSS, code, o, -3) == -1
        assert call(hipops.disk(2), code, o, 4) == -1
        assert "cross" in lib.amt_last_error().decode() and "all-ones" in lib.amt_last_error().decode()
        assert call(np.eye(3), code, o, 4) == -1
        assert call([[0, 1, 0], [1, 0, 1], [0, 1, 0]], code, o, 4) == -1
        assert call(ref.CROSS, code, d, 4) == -1  # out is in
        assert "alias" in lib.amt_last_error().decode()
        assert call(ref.CROSS, code, stack[1:3], 4, src=stack[0:2], n=2) == -1  # overlapping in part
        assert call(ref.CROSS, code, stack[0:2], 4, src=stack[1:3], n=2) == -1
        assert call(ref.CROSS, code, stack[1:2], 4, src=stack[0:1]) == 0  # neighbours that do not overlap
        assert call(ref.CROSS, code, o, 4, n=0) == 0
    assert call(ref.CROSS, 7, o, 4) == -1 and call(ref.CROSS, -1, o, 4) == -1 and call(ref.CROSS, 7, o, 0) == -1


def test_codes_0_to_4_are_unchanged(ctx):
    """The five earlier codes through the raw entry point give the bytes of their named operators."""
    import fill_holes_reference as fh

    plane = ref.random((70, 131), 0.65, 1)
    d = ctx.asarray(plane)
    lib = _hip.load_library()
    named = {0: hipops.binary_erosion, 1: hipops.binary_dilation, 2: hipops.binary_opening, 3: hipops.binary_closing}
    fp = hipops.disk(2)
    for op, fn in named.items():
        o = ctx.empty(plane.shape, np.uint8)
        assert lib.amt_binary_morph(ctx.handle, d.ptr, o.ptr, 1, 70, 131, fp.ctypes.data_as(ctypes.c_void_p), fp.shape[0],
                                    fp.shape[1], op, 1 if op == 0 else 0) == 0
        assert np.array_equal(o.numpy(dtype=np.uint8), fn(d, fp).numpy(dtype=np.uint8)), op
    for st in (ref.CROSS, ref.FULL):
        o = ctx.empty(plane.shape, np.uint8)
        for border in (0, 9):  # ignored by code 4
            assert lib.amt_binary_morph(ctx.handle, d.ptr, o.ptr, 1, 70, 131, st.ctypes.data_as(ctypes.c_void_p), 3, 3, 4,
                                        border) == 0
            assert np.array_equal(o.numpy(dtype=np.uint8), hipops.binary_fill_holes(d, st).numpy(dtype=np.uint8))
            assert np.array_equal(o.numpy(dtype=np.uint8), fh.scipy_fill(plane, st))


def test_operations(ctx):
    plane = ref.frame_bays((70, 131)) & ref.random((70, 131), 0.97, 3)
    m = plane.astype(bool)
    for name, op in (("remove_small_objects", "objects"), ("remove_small_holes", "holes")):
        fn = getattr(operations, name)
        for size, conn in ((2, 1), (5, 2), (64, 1)):
            st = ref.CROSS if conn == 1 else ref.FULL
            want = ref.apply(op, plane, size, st).astype(bool)
            got = fn(m, size, conn)
            assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and np.array_equal(got, want), (name, size)
            dev = fn(ctx.asarray(m), size, connectivity=conn)
            assert isinstance(dev, DeviceArray) and dev.is_bool and np.array_equal(dev.numpy(), want), (name, size)
            assert np.array_equal(fn(m, size, conn), got)  # a repeat call is bit-identical
        assert np.array_equal(fn(m), ref.apply(op, plane, 64, ref.CROSS).astype(bool))  # the defaults: 64, connectivity 1
        with pytest.raises(ValueError, match="must be a 2D array"):
            fn(ctx.asarray(np.zeros((2, 8, 8), np.uint8)))
        for shape in ((0, 5), (3, 0)):
            got = fn(ctx.empty(shape, np.uint8))
            assert isinstance(got, DeviceArray) and got.shape == shape and got.is_bool
    # inside a Pipeline, after apply_threshold: the mask stays on the device
    fov, centres, blobs = ref.blobs_field()
    raw = operations.apply_threshold(fov[1], "otsu")
    assert ndi.label(raw)[1] >= len(centres) + len(blobs)
    pipe = Pipeline([ImageOperation(operations.apply_threshold, "otsu"),
                     ImageOperation(operations.remove_small_objects, 200),
                     ImageOperation(operations.remove_small_holes, area_threshold=30, connectivity=2)])
    assert pipe._device_chain_applies(fov[1])
    got = pipe(fov[1])
    want = ref.remove_small_holes(ref.remove_small_objects(raw, 200, ref.CROSS), 30, ref.FULL).astype(bool)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert ndi.label(got)[1] == len(centres) and int(got.sum()) < int(raw.sum())


# ---- the classical chain ------------------------------------------------------------------------------------------------
MIN_DISTANCE, MAX_CELLS, MIN_SIZE = 5, 256, 200


def _compose(ctx, mask, clear):
    """What the chain does behind its mask, operator by operator: EDT -> peaks -> markers -> seeded watershed ->
    (clear_border +) relabel_sequential."""
    d2, _ = hipops.edt(mask, want_edt=False)
    peaks = hipops.peak_mask(d2, mask, MIN_DISTANCE)
    markers, nmark = hipops.label(peaks, connectivity=1)
    ws = hipops.watershed_edt(d2, markers, mask, seeds_first=True)
    k = int(nmark.numpy().max())
    if clear:
        labels, _ = hipops.clear_border_relabel(ws, max(k, 1))
    else:
        labels, _ = hipops.relabel_sequential(ws, max(k, 1))
    return labels.numpy()


@pytest.fixture(scope="module")
def field():
    return ref.blobs_field()


def _model_mask(ctx, model, dapi):
    """_segment_classical's own mask, before any area filter."""
    g = hipops.gaussian(ctx.asarray(dapi), model.sigma)
    m0 = hipops.greater_than(g, hipops.threshold_otsu(g))
    fp = hipops.disk(model.opening_radius)
    return hipops.binary_closing(hipops.binary_opening(m0, fp), fp).numpy(dtype=np.uint8)


def test_segmentation_model_with_min_size(ctx, field):
    fov, centres, blobs = field
    dapi = fov[1]
    model = SegmentationModel(backend="classical", min_size=MIN_SIZE)
    plain = SegmentationModel(backend="classical")
    assert MIN_DISTANCE == max(1, int(round(model.default_cell_diameter_px / 6.0)))
    # the host restatement first: without the filter the field has discs + blobs cells, with it the discs
    m1 = _model_mask(ctx, model, dapi)
    lab, k = ndi.label(m1, structure=ref.CROSS)
    areas = np.sort(np.bincount(lab.ravel())[1:])
    assert k == len(centres) + len(blobs)
    assert areas[len(blobs) - 1] < MIN_SIZE // 2 and areas[len(blobs)] > 2 * MIN_SIZE  # blobs well below, discs well above
    want0 = _compose(ctx, ctx.asarray(m1), clear=False)
    assert int(want0.max()) == len(centres) + len(blobs)
    filtered = ref.remove_small_objects(m1, MIN_SIZE, ref.CROSS)
    assert ndi.label(filtered, structure=ref.CROSS)[1] == len(centres)
    want = _compose(ctx, ctx.asarray(filtered), clear=False)
    # the model
    got = model.segment(dapi)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert int(got.max()) == len(centres)
    assert np.array_equal(plain.segment(dapi), want0)  # min_size=0: today's result
    assert np.array_equal(SegmentationModel(backend="classical", min_size=1).segment(dapi), want0)
    images = [dapi, dapi[::-1].copy(), dapi[:, ::-1].copy(), dapi]
    batch = model.batch_segment(images, show_progress=False)
    assert np.array_equal(batch[0], got) and np.array_equal(batch[3], got)
    for im, lab_im in zip(images, batch):
        assert np.array_equal(lab_im, model.segment(im)) and int(lab_im.max()) == len(centres)
    for im, lab_im in zip(images, plain.batch_segment(images, show_progress=False)):
        assert np.array_equal(lab_im, plain.segment(im)) and int(lab_im.max()) == len(centres) + len(blobs)


def test_run_c3_and_batch_masks_with_min_size(ctx, field):
    from arcadia_microscopy_tools_amd.channels import BRIGHTFIELD, DAPI, FITC, TRITC

    fov, centres, blobs = field
    d = ctx.asarray(fov[None])
    kw = dict(ctx=ctx, max_cells=MAX_CELLS, min_distance=MIN_DISTANCE, profile=True)
    seg = FovSegmenter(1, 4, 256, 256, min_size=MIN_SIZE, **kw)
    labels = seg.run_c3(d).numpy()[0]
    assert "remove_small" in seg.times.ms() and "fill_holes" not in seg.times.ms()
    raw = seg.mask_a.numpy(dtype=np.uint8)[0]  # mask_chain's result; the filtered mask went to the spare mask_b
    filtered = ref.remove_small_objects(raw, MIN_SIZE, ref.CROSS)
    assert np.array_equal(seg.mask_b.numpy(dtype=np.uint8)[0], filtered)
    assert ndi.label(raw, structure=ref.CROSS)[1] == len(centres) + len(blobs)
    assert np.array_equal(labels, _compose(ctx, ctx.asarray(filtered[None]), clear=True)[0])
    assert int(labels.max()) == len(centres)
    # with the hole filling in front, the filter writes mask_a
    both = FovSegmenter(1, 4, 256, 256, min_size=MIN_SIZE, fill_holes=True, **kw)
    assert np.array_equal(both.run_c3(d).numpy()[0], labels)  # solid discs: nothing to fill
    assert list(both.times.ms()).index("fill_holes") < list(both.times.ms()).index("remove_small")
    assert np.array_equal(both.mask_a.numpy(dtype=np.uint8)[0], filtered)
    # min_size 0 / 1: nothing is launched, today's result
    for m in (0, 1):
        plain = FovSegmenter(1, 4, 256, 256, min_size=m, **kw)
        labels0 = plain.run_c3(d).numpy()[0]
        assert "remove_small" not in plain.times.ms()
        assert np.array_equal(labels0, _compose(ctx, ctx.asarray(raw[None]), clear=True)[0])
        assert int(labels0.max()) == len(centres) + len(blobs)
    # batch_masks: the same label image as segment (no disc touches the frame)
    model = SegmentationModel(backend="classical", min_size=MIN_SIZE)
    flipped = fov[:, ::-1].copy()
    masks = model.batch_masks([fov, flipped], (BRIGHTFIELD, DAPI, FITC, TRITC), nuclear=1)
    assert masks[0] is not None and np.array_equal(masks[0].mask_image, labels)
    assert np.array_equal(masks[0].mask_image, model.segment(fov[1]))
    assert masks[1] is not None and np.array_equal(masks[1].mask_image, model.segment(flipped[1]))
    assert masks[0].num_cells == len(centres) and masks[1].num_cells == len(centres)
    unfiltered = SegmentationModel(backend="classical").batch_masks([fov], (BRIGHTFIELD, DAPI, FITC, TRITC), nuclear=1)
    assert unfiltered[0].num_cells == len(centres) + len(blobs)


def test_all_cases_under_poison(ctx, tmp_path):
    out = tmp_path / "area_filters.json"
    res = poison_child.run_module("tests.area_filters_cases", out, CHILD_TIMEOUT_S, "the poisoned area filter cases")
    assert not res["mismatches"], f"{len(res['mismatches'])} outputs differ under poison: {res['mismatches'][:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for shape in ref.SHAPES:
        here.update(_shape_result(ctx, shape)["digests"])
    poison_child.assert_unmoved(here, res["digests"])
