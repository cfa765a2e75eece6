"""``binary_fill_holes`` on the device against ``scipy.ndimage.binary_fill_holes``, byte for byte: every generator of
tests/fill_holes_reference.py on every shape it fits, both structures, as a single plane, as plane 1 of a stack and
inside a batch (tests/fill_holes_cases.py); truth-value bytes; the run-table and the general path on the same plane;
the identity with ``remove_small_holes`` where no background touches the frame; refusals; the unchanged operations 0..3; ``operations.binary_fill_holes``; the classical chain with ``fill_holes``; and
all cases once more in a child process with the scratch arena poisoned."""
import ctypes

import numpy as np
import pytest

import fill_holes_cases as cases
import fill_holes_reference as ref
import poison_child
from arcadia_microscopy_tools_amd import _hip, hipops, operations
from arcadia_microscopy_tools_amd.device import DeviceArray, get_context
from arcadia_microscopy_tools_amd.model import SegmentationModel
from arcadia_microscopy_tools_amd.pipeline import ImageOperation, Pipeline
from arcadia_microscopy_tools_amd.segment import FovSegmenter, segment_fovs

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 120
_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    return get_context()


def _shape_result(ctx, shape):
    if shape not in _RESULTS:
        _RESULTS[shape] = cases.run_shape(ctx, shape)
    return _RESULTS[shape]


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_generator_matches_scipy(ctx, shape):
    res = _shape_result(ctx, shape)
    assert res["calls"] >= 2 * (2 * 8 + 3), shape
    assert not res["mismatches"], f"{len(res['mismatches'])} outputs differ from scipy; the first: {res['mismatches'][:10]}"


def _offset_view(ctx, plane, offset):
    """The plane on the device at an address ``offset`` bytes past a 256-byte boundary."""
    H, W = plane.shape
    flat = np.zeros(offset + H * W, np.uint8)
    flat[offset:] = plane.reshape(-1)
    return ctx.asarray(flat)[offset:offset + H * W].reshape(H, W)


@pytest.mark.parametrize("shape", [(16, 16), (64, 64), (65, 128), (40, 256), (66, 320), (256, 256)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_run_table_and_general_path_agree(ctx, shape):
    """W % 16 == 0 and H * W % 16 == 0: an aligned plane takes the run tables; the same plane one byte (or eight) further
    on, or written to an output that is not 16-byte aligned, takes the byte union-find."""
    assert shape[1] % 16 == 0 and (shape[0] * shape[1]) % 16 == 0
    for name, plane in ref.planes(shape):
        for sname, st in ref.STRUCTURES:
            want = ref.scipy_fill(plane, st)
            aligned = ctx.asarray(plane)
            assert aligned.ptr % 16 == 0
            a = hipops.binary_fill_holes(aligned, st).numpy(dtype=np.uint8)
            assert np.array_equal(a, want), (shape, name, sname, "run tables")
            for offset in (1, 8):
                moved = _offset_view(ctx, plane, offset)
                assert moved.ptr % 16 == offset
                b = hipops.binary_fill_holes(moved, st).numpy(dtype=np.uint8)
                assert np.array_equal(b, a), (shape, name, sname, "input offset", offset)
            out = _offset_view(ctx, np.zeros(shape, np.uint8), 4)
            c = hipops.binary_fill_holes(aligned, st, out=out)
            assert c is out and np.array_equal(out.numpy(dtype=np.uint8), a), (shape, name, sname, "output offset")


@pytest.mark.parametrize("shape", [(65, 128), (70, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_truth_value_bytes(ctx, shape):
    """Foreground is byte != 0: bytes from {1, 2, 255} give the result of the 0 / 1 plane, and the output holds 0 / 1."""
    for name, plane in ref.planes(shape):
        loud = ref.truth_bytes(plane, 7)
        for sname, st in ref.STRUCTURES:
            want = ref.scipy_fill(plane, st)
            got = hipops.binary_fill_holes(ctx.asarray(loud), st).numpy(dtype=np.uint8)
            assert np.array_equal(got, want), (shape, name, sname)
            stack = ctx.asarray(np.stack([loud, loud]))
            assert np.array_equal(hipops.binary_fill_holes(stack, st).numpy(dtype=np.uint8)[1], want), (shape, name, sname)


@pytest.mark.parametrize("shape", [(64, 64), (65, 128), (70, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fill_holes_is_remove_small_holes_where_no_background_touches_the_frame(ctx, shape):
    """Both operators are one component filter on the device; what ties them together, on one tile, across a seam of
    the run tables and on the general path (W % 16 != 0).  Where no background component holds a frame pixel every one is
    a hole, which is what ``remove_small_holes`` fills with a size above the plane's pixel count.  Conversely, where the
    only background component touches the frame, nothing is filled by either: it is no hole, and no component is smaller
    than 1."""
    from scipy import ndimage as ndi

    import area_filters_reference as aref

    H, W = shape
    frame = np.ones(shape, bool)
    frame[1:-1, 1:-1] = False
    for gen in (ref.nested, ref.seam_holes):
        m = np.pad(gen((H - 2, W - 2)), 1, constant_values=1)  # inside a 1-pixel foreground frame
        assert m.shape == shape
        d = ctx.asarray(m)
        for sname, st in ref.STRUCTURES:
            lab, k = ndi.label(m == 0, structure=st)
            assert k >= 2 and not lab[frame].any()  # the premise
            want = ref.scipy_fill(m, st)
            assert np.array_equal(want, aref.remove_small_holes(m, H * W + 1, st))
            filled = hipops.binary_fill_holes(d, st).numpy(dtype=np.uint8)
            by_area = hipops.remove_small_holes(d, H * W + 1, aref.CONNECTIVITY[sname]).numpy(dtype=np.uint8)
            assert np.array_equal(filled, want), (shape, gen.__name__, sname)
            assert np.array_equal(by_area, filled), (shape, gen.__name__, sname)
    m = ref.nested_solid(shape)
    d = ctx.asarray(m)
    for sname, st in ref.STRUCTURES:
        lab, k = ndi.label(m == 0, structure=st)
        assert k == 1 and lab[frame].any()  # the premise
        assert np.array_equal(hipops.binary_fill_holes(d, st).numpy(dtype=np.uint8), m), (shape, sname)
        assert np.array_equal(hipops.remove_small_holes(d, 1, aref.CONNECTIVITY[sname]).numpy(dtype=np.uint8), m), (shape, sname)


def test_result_is_a_bool_mask_and_out_is_used(ctx):
    plane = ref.nested((33, 40))
    d = ctx.asarray(plane.astype(bool))
    got = hipops.binary_fill_holes(d)
    assert got.is_bool and got.dtype == np.uint8 and got.numpy().dtype == np.bool_
    assert np.array_equal(got.numpy(), ref.scipy_fill(plane, ref.CROSS).astype(bool))
    out = ctx.empty((33, 40), np.uint8)
    assert hipops.binary_fill_holes(d, ref.FULL, out=out) is out and out.is_bool


def test_empty_device_arrays(ctx):
    """Empty in, empty bool mask out, as for numpy arrays: no plane, or planes without pixels."""
    for shape in ((0, 33, 40), (0, 5), (3, 0), (2, 0, 7)):
        got = hipops.binary_fill_holes(ctx.empty(shape, np.uint8))
        assert got.shape == shape and got.is_bool and got.numpy().shape == shape
    for shape in ((0, 5), (3, 0)):
        got = operations.binary_fill_holes(ctx.empty(shape, np.uint8))
        assert isinstance(got, DeviceArray) and got.shape == shape and got.is_bool


def test_refusals(ctx):
    d = ctx.asarray(ref.nested((33, 40)))
    with pytest.raises(ValueError, match="structure"):
        hipops.binary_fill_holes(d, np.ones((5, 5)))
    with pytest.raises(ValueError, match="alias"):
        hipops.binary_fill_holes(d, out=d)
    with pytest.raises(TypeError):
        hipops.binary_fill_holes(ctx.asarray(np.zeros((8, 8), np.uint16)))
    with pytest.raises(ValueError):
        hipops.binary_fill_holes(ctx.asarray(np.zeros((2, 2, 8, 8), np.uint8)))
    # an output that overlaps the input in part: planes 1..2 of a stack written from planes 0..1
    stack = ctx.asarray(np.stack([ref.nested((33, 40))] * 3))
    with pytest.raises(ValueError, match="alias"):
        hipops.binary_fill_holes(stack[0:2], out=stack[1:3])
    with pytest.raises(ValueError, match="alias"):
        hipops.binary_fill_holes(stack[1:3], out=stack[0:2])
    # the C ABI itself: another footprint, out aliasing in, an operation code beyond 4
    lib = _hip.load_library()

    def call(fp, op, out):
        fp = np.ascontiguousarray(fp, np.uint8)
        return lib.amt_binary_morph(ctx.handle, d.ptr, out.ptr, 1, 33, 40, fp.ctypes.data_as(ctypes.c_void_p), fp.shape[0],
                                    fp.shape[1], op, 0)

    o = ctx.empty((33, 40), np.uint8)
    assert call(ref.CROSS, 4, o) == 0 and call(ref.FULL, 4, o) == 0
    assert call(hipops.disk(2), 4, o) == -1
    assert "cross" in lib.amt_last_error().decode() and "all-ones" in lib.amt_last_error().decode()
    assert call(np.eye(3), 4, o) == -1
    assert call(ref.CROSS, 4, d) == -1
    fp = np.ascontiguousarray(ref.CROSS)
    for src, dst in ((stack[0:2], stack[1:3]), (stack[1:3], stack[0:2])):
        assert lib.amt_binary_morph(ctx.handle, src.ptr, dst.ptr, 2, 33, 40, fp.ctypes.data_as(ctypes.c_void_p), 3, 3, 4,
                                    0) == -1
    assert lib.amt_binary_morph(ctx.handle, stack[0:1].ptr, stack[1:2].ptr, 1, 33, 40, fp.ctypes.data_as(ctypes.c_void_p),
                                3, 3, 4, 0) == 0  # neighbours that do not overlap
    assert call(ref.CROSS, 5, o) == -1 and call(ref.CROSS, -1, o) == -1
    assert lib.amt_binary_morph(ctx.handle, d.ptr, o.ptr, 0, 33, 40, ref.CROSS.ctypes.data_as(ctypes.c_void_p), 3, 3, 4,
                                0) == 0


def test_operations_0_to_3_are_unchanged(ctx):
    """The four earlier codes through the raw entry point equal the named operators, which equal scipy."""
    from scipy import ndimage as ndi

    plane = ref.random((70, 131), 0.65, 1)
    d = ctx.asarray(plane)
    fp = hipops.disk(2)
    lib = _hip.load_library()
    named = {0: hipops.binary_erosion, 1: hipops.binary_dilation, 2: hipops.binary_opening, 3: hipops.binary_closing}
    m, f = plane.astype(bool), fp.astype(bool)
    host = {0: ndi.binary_erosion(m, f, border_value=1), 1: ndi.binary_dilation(m, f),
            2: ndi.binary_dilation(ndi.binary_erosion(m, f, border_value=1), f),
            3: ndi.binary_erosion(ndi.binary_dilation(m, f), f, border_value=1)}
    for op, fn in named.items():
        o = ctx.empty(plane.shape, np.uint8)
        border = 1 if op == 0 else 0
        rc = lib.amt_binary_morph(ctx.handle, d.ptr, o.ptr, 1, 70, 131, fp.ctypes.data_as(ctypes.c_void_p), fp.shape[0],
                                  fp.shape[1], op, border)
        assert rc == 0
        got = o.numpy(dtype=np.uint8)
        assert np.array_equal(got, fn(d, fp).numpy(dtype=np.uint8)), op
        assert np.array_equal(got.astype(bool), host[op]), op


def test_operations_binary_fill_holes(ctx):
    plane = ref.seam_holes((70, 131))
    for st in (None, ref.CROSS, ref.FULL):
        want = ref.scipy_fill(plane, ref.CROSS if st is None else st).astype(bool)
        for given in (plane.astype(bool), plane, plane.astype(np.int64) * 9, ref.truth_bytes(plane, 2)):
            got = operations.binary_fill_holes(given, st)
            assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and np.array_equal(got, want)
        on_device = operations.binary_fill_holes(ctx.asarray(plane.astype(bool)), st)
        assert isinstance(on_device, DeviceArray) and on_device.is_bool and np.array_equal(on_device.numpy(), want)
    with pytest.raises(ValueError, match="must be a 2D array"):
        operations.binary_fill_holes(ctx.asarray(np.zeros((2, 8, 8), np.uint8)))
    # inside a Pipeline, after apply_threshold: one upload, one download
    fov, _ = ref.annuli_field()
    pipe = Pipeline([ImageOperation(operations.apply_threshold, "otsu"), ImageOperation(operations.binary_fill_holes)])
    assert pipe._device_chain_applies(fov[1])
    got = pipe(fov[1])
    rings = operations.apply_threshold(fov[1], "otsu")
    assert got.dtype == np.bool_ and np.array_equal(got, ref.scipy_fill(rings, ref.CROSS).astype(bool))
    assert int(got.sum()) > int(rings.sum())
    full = Pipeline([ImageOperation(operations.apply_threshold, "otsu"),
                     ImageOperation(operations.binary_fill_holes, structure=ref.FULL)])(fov[1])
    assert np.array_equal(full, ref.scipy_fill(rings, ref.FULL).astype(bool))


# ---- the classical chain ------------------------------------------------------------------------------------------------
MIN_DISTANCE, MAX_CELLS = 5, 256


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
    return ref.annuli_field()


def test_run_c3_with_fill_holes(ctx, field):
    fov, centres = field
    d = ctx.asarray(fov[None])
    seg = FovSegmenter(1, 4, 256, 256, ctx=ctx, max_cells=MAX_CELLS, min_distance=MIN_DISTANCE, fill_holes=True, profile=True)
    labels = seg.run_c3(d).numpy()[0]
    assert "fill_holes" in seg.times.ms()
    rings = seg.mask_a.numpy(dtype=np.uint8)[0]  # mask_chain's result; the filled mask went to the spare mask_b
    filled = ref.scipy_fill(rings, ref.CROSS)
    assert int(filled.sum()) > int(rings.sum()) + 12 * 50  # the closing did not bridge the centres
    assert np.array_equal(seg.mask_b.numpy(dtype=np.uint8)[0], filled)
    want = _compose(ctx, ctx.asarray(filled[None]), clear=True)[0]
    assert np.array_equal(labels, want)
    assert int(labels.max()) == len(centres)  # one label per nucleus: no ring is cut into arcs
    # fill_holes=False: today's chain, operator by operator
    plain = FovSegmenter(1, 4, 256, 256, ctx=ctx, max_cells=MAX_CELLS, min_distance=MIN_DISTANCE, profile=True)
    labels0 = plain.run_c3(d).numpy()[0]
    assert "fill_holes" not in plain.times.ms()
    assert np.array_equal(labels0, _compose(ctx, ctx.asarray(rings[None]), clear=True)[0])
    assert int(labels0.max()) > len(centres)  # the rings do come out in arcs without the fill
    # config 2 labels the filled mask as well
    from scipy import ndimage as ndi

    c2 = seg.run_c2(d).numpy()[0]
    assert np.array_equal(c2 != 0, filled != 0) and int(c2.max()) == ndi.label(filled, structure=ref.FULL)[1]
    res = segment_fovs(fov[None], ctx=ctx, max_cells=MAX_CELLS, min_distance=MIN_DISTANCE, fill_holes=True)
    assert np.array_equal(res.labels_numpy()[0], want)


def test_segmentation_model_with_fill_holes(ctx, field):
    fov, centres = field
    dapi = fov[1]
    model = SegmentationModel(backend="classical", fill_holes=True)
    got = model.segment(dapi)
    assert got.dtype == np.int64
    # _segment_classical's own mask, filled on the host
    g = hipops.gaussian(ctx.asarray(dapi), model.sigma)
    m0 = hipops.greater_than(g, hipops.threshold_otsu(g))
    fp = hipops.disk(model.opening_radius)
    m1 = hipops.binary_closing(hipops.binary_opening(m0, fp), fp).numpy(dtype=np.uint8)
    filled = ref.scipy_fill(m1, ref.CROSS)
    assert int(filled.sum()) > int(m1.sum())
    want = _compose(ctx, ctx.asarray(filled), clear=False)
    assert np.array_equal(got, want)
    assert int(got.max()) == len(centres)
    # batch routes: batch_segment equals segment image by image, with and without the fill
    images = [dapi, dapi[::-1].copy(), dapi[:, ::-1].copy()]
    batch = model.batch_segment(images, show_progress=False)
    for im, lab in zip(images, batch):
        assert np.array_equal(lab, model.segment(im))
    plain = SegmentationModel(backend="classical")
    want0 = _compose(ctx, ctx.asarray(m1), clear=False)
    assert np.array_equal(plain.segment(dapi), want0)
    for im, lab in zip(images, plain.batch_segment(images, show_progress=False)):
        assert np.array_equal(lab, plain.segment(im))
    assert not np.array_equal(got, want0)


def test_batch_masks_with_fill_holes(ctx, field):
    from arcadia_microscopy_tools_amd.channels import BRIGHTFIELD, DAPI, FITC, TRITC

    fov, centres = field
    model = SegmentationModel(backend="classical", fill_holes=True)
    masks = model.batch_masks([fov, fov[:, ::-1].copy()], (BRIGHTFIELD, DAPI, FITC, TRITC), nuclear=1)
    seg = FovSegmenter(1, 4, 256, 256, ctx=ctx, max_cells=MAX_CELLS, min_distance=MIN_DISTANCE, fill_holes=True)
    for im, mask in zip([fov, fov[:, ::-1].copy()], masks):
        want = seg.run_c3(ctx.asarray(im[None])).numpy()[0]
        assert mask is not None and np.array_equal(mask.mask_image, want)


def test_all_cases_under_poison(ctx, tmp_path):
    out = tmp_path / "fill_holes.json"
    res = poison_child.run_module("tests.fill_holes_cases", out, CHILD_TIMEOUT_S, "the poisoned fill_holes cases")
    assert not res["mismatches"], f"{len(res['mismatches'])} outputs differ from scipy under poison: {res['mismatches'][:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for shape in ref.SHAPES:
        here.update(_shape_result(ctx, shape)["digests"])
    poison_child.assert_unmoved(here, res["digests"])
