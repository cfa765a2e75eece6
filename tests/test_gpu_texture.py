"""Per-cell Haralick texture on the device (``AMT_RPX_TEXTURE``, ``hipops.texture``, ``SegmentationMask.cell_texture``) against
tests/texture_reference.py.  The co-occurrence counts are compared byte for byte (``tobytes``); the feature table within
rtol 1e-9 / atol 1e-12 with NaNs in the same places, info_measure_2 on its square (tests/texture_cases.py ``compare``).  The
case list runs once more in a child process with the scratch arena poisoned."""
import json

import numpy as np
import pytest

import poison_child
import texture_cases as tc
import texture_reference as tr

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 120

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _shape_run(ctx, shape, kind):
    if (shape, kind) not in _RESULTS:
        _RESULTS[(shape, kind)] = tc.run(ctx, [shape], kinds=(kind,))
    return _RESULTS[(shape, kind)]


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("shape", tc.SHAPES + [tc.BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cases_match_the_reference(ctx, shape, kind):
    res = _shape_run(ctx, shape, kind)
    names = set(tc.cases(shape, kind))
    if shape == tc.BIG:
        assert names == {"one_constant_label"} and len(res["records"]) == 2
    else:
        assert {"blobs", "blobs_noise", "no_pairs", "distance_beyond_box", "shared_edge", "checkerboard", "two_pieces",
                "constant_default_ranges", "constant_level_5", "two_levels", "levels_2", "levels_5", "levels_32", "levels_64",
                "distance_2", "distance_3", "distance_7", "ranges_narrow", "ranges_equal", "ranges_value_at_hi",
                "channels_2", "channels_5", "channels_5_ranges"} <= names
        assert {f"width_{w}" for w in tc.WIDTHS if w <= shape[1]} <= names
        assert {f"width_{w}_mirrored" for w in tc.WIDTHS if w <= shape[1]} <= names
        # each case alone, as plane 1 of a stack, and the three batch planes
        assert len(res["records"]) == 2 * len(names) + len(tc.BATCH)
    err = np.max([r["err"] for r in res["records"]], axis=0)
    print(f"{shape} {kind}: largest absolute error per column", dict(zip(tr.COLS, err.tolist())))
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} of {len(res['records'])} results differ from the reference; the first: {bad[:10]}"


def test_every_width_case_is_on_its_side_of_the_layout_switch():
    widths = [w for w in tc.WIDTHS if w <= 131]
    assert widths == [7, 8, 9, 16, 17, 32, 33, 64, 65]
    lab = tc.cases((70, 131), "u16")["width_65"][0]
    for label in (1, 2, 3, 4):
        ys, xs = np.nonzero(lab == label)
        assert xs.max() - xs.min() + 1 == 65
    assert lab[0, 0] == 1 and lab[-1, -1] == 4 and (lab[:, -1] == 2).any() and (lab[:, 0] == 3).any()
    mirrored = tc.cases((70, 131), "u16")["width_65_mirrored"][0]
    assert mirrored[0, -1] == 1 and mirrored[-1, 0] == 4


@pytest.mark.parametrize("kind", tc.KINDS)
def test_absent_labels_and_directions_without_a_pair(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    shape = (33, 40)
    lab, stack, k, p = tc.cases(shape, kind)["blobs"]
    t, g = hipops.texture(ctx.asarray(lab[None]), ctx.asarray(stack[None]), k, glcm=True)
    t, g = t.numpy(), g.numpy()
    assert t.shape == (1, k, 1, 4, 13) and g.shape == (1, k, 1, 4, 8, 8) and g.dtype == np.uint32
    assert not (lab == k).any() and np.isnan(t[0, k - 1]).all() and not g[0, k - 1].any()
    assert t[0, k - 1].tobytes() == np.full((1, 4, 13), np.nan).tobytes()  # the canonical quiet NaN
    lab, stack, k, p = tc.cases(shape, kind)["no_pairs"]
    t, g = hipops.texture(ctx.asarray(lab[None]), ctx.asarray(stack[None]), k, glcm=True)
    t, g = t.numpy()[0, :, 0], g.numpy()[0, :, 0]
    assert np.isnan(t).all(axis=-1).tolist() == [[True] * 4, [False, True, True, True], [True, True, False, True], [False] * 4]
    assert g.sum(axis=(-1, -2)).tolist() == [[0, 0, 0, 0], [4, 0, 0, 0], [0, 0, 4, 0], [4, 2, 4, 2]]
    without = hipops.texture(ctx.asarray(lab[None]), ctx.asarray(stack[None]), k).numpy()
    assert without[0, :, 0].tobytes() == t.tobytes()  # the table does not depend on whether the counts are asked for


@pytest.mark.parametrize("kind", tc.KINDS)
def test_default_ranges_are_the_images_own_extrema(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    shape = (70, 131)
    lab, stack, k, p = tc.cases(shape, kind)["channels_5"]
    labels = ctx.asarray(np.stack([lab, np.flipud(lab)]))
    both = np.ascontiguousarray(np.stack([stack, stack[::-1, :, ::-1] // 2 if kind == "u16" else stack[::-1, :, ::-1] * 0.5]))
    images = ctx.asarray(both)
    t0, g0 = hipops.texture(labels, images, k, glcm=True)
    ranges = np.stack([tr.default_ranges(both[0]), tr.default_ranges(both[1])])
    t1, g1 = hipops.texture(labels, images, k, ranges=ranges, glcm=True)
    t2, g2 = hipops.texture(labels, images, k, ranges=ctx.asarray(ranges), glcm=True)
    assert t0.numpy().tobytes() == t1.numpy().tobytes() == t2.numpy().tobytes()
    assert g0.numpy().tobytes() == g1.numpy().tobytes() == g2.numpy().tobytes()
    # a (lo, hi) pair serves every image
    pair = (float(both.min()), float(both.max()))
    t3 = hipops.texture(labels, images, k, ranges=pair).numpy()
    t4 = hipops.texture(labels, images, k, ranges=np.broadcast_to(np.array(pair), (2, 5, 2))).numpy()
    assert t3.tobytes() == t4.tobytes()


@pytest.mark.parametrize("kind", tc.KINDS)
def test_every_channel_equals_its_own_call(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    shape = (33, 40)
    for C in (1, 2, 5):
        lab, stack, k, p = tc.cases(shape, kind)["blobs" if C == 1 else f"channels_{C}"]
        assert stack.shape[0] == C
        labels = ctx.asarray(np.stack([lab, np.flipud(lab)]))
        both = np.ascontiguousarray(np.stack([stack, stack[::-1, :, ::-1]]))  # the second plane: reversed and mirrored
        t, g = hipops.texture(labels, ctx.asarray(both), k, levels=5, distance=2, glcm=True)
        t, g = t.numpy(), g.numpy()
        assert t.shape == (2, k, C, 4, 13) and g.shape == (2, k, C, 4, 5, 5)
        for c in range(C):
            one, gone = hipops.texture(labels, ctx.asarray(np.ascontiguousarray(both[:, c:c + 1])), k, levels=5, distance=2,
                                       glcm=True)
            assert t[:, :, c].tobytes() == one.numpy()[:, :, 0].tobytes()
            assert g[:, :, c].tobytes() == gone.numpy()[:, :, 0].tobytes()
            for i, plane in enumerate((lab, np.flipud(lab))):
                want = tr.texture_stack(plane, both[i, c:c + 1], k, 5, 2)
                assert tc.compare(t[i, :, c:c + 1], g[i, :, c:c + 1], *want)[0], (C, c, i)


@pytest.mark.parametrize("kind", tc.KINDS)
def test_two_runs_give_identical_bytes(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    shape = (70, 131)
    names = ["blobs", "blobs_noise", "shared_edge", "checkerboard", "two_levels", "width_65", "width_33"]
    k = max(tc.cases(shape, kind)[n][2] for n in names)
    lab = ctx.asarray(np.stack([tc.cases(shape, kind)[n][0] for n in names]))
    stack = ctx.asarray(np.stack([tc.cases(shape, kind)[n][1] for n in names]))
    for L in (8, 64):
        t, g = hipops.texture(lab, stack, k, levels=L, glcm=True)
        first = (t.numpy().tobytes(), g.numpy().tobytes())
        t, g = hipops.texture(lab, stack, k, levels=L, glcm=True)
        assert (t.numpy().tobytes(), g.numpy().tobytes()) == first


def _raw(ctx, lab, inten, code, C, ranges, columns, out, n, H, W, k):
    from arcadia_microscopy_tools_amd import _hip

    p = lambda a: None if a is None else a.ptr  # noqa: E731
    return _hip.load_library().amt_regionprops_ext(ctx.handle, p(lab), p(inten), code, C, columns, p(ranges), p(out), n, H,
                                                   W, k)


def test_argument_errors_of_the_c_abi(ctx):
    from arcadia_microscopy_tools_amd import _hip

    cols = _hip.rpx_texture_columns
    lab = ctx.asarray(np.ones((1, 7, 5), np.int32))
    u16 = ctx.asarray(np.full((1, 1, 7, 5), 9, np.uint16))
    u8 = ctx.asarray(np.ones((1, 1, 7, 5), np.uint8))
    ranges = ctx.asarray(np.array([[[0.0, 16.0]]]))
    out = ctx.asarray(np.full((1, 1, 1, 4, 13), 5.0))
    glcm = ctx.asarray(np.full((1, 1, 1, 4, 2, 2), 7, np.uint32))
    U = _hip.U16
    for L in (1, 0, 65, 127):
        assert _raw(ctx, lab, u16, U, 1, ranges, cols(L, 1), out, 1, 7, 5, 1) == -1
    for d in (0, 256, 1023):
        assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, d), out, 1, 7, 5, 1) == -1
        assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, d, True), glcm, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u8, _hip.U8, 1, ranges, cols(2, 1), out, 1, 7, 5, 1) == -1  # neither AMT_U16 nor AMT_F64
    assert _raw(ctx, lab, lab, _hip.I32, 1, ranges, cols(2, 1), out, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u16, U, 0, ranges, cols(2, 1), out, 1, 7, 5, 1) == -1  # C < 1
    assert _raw(ctx, None, u16, U, 1, ranges, cols(2, 1), out, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, None, U, 1, ranges, cols(2, 1), out, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u16, U, 1, None, cols(2, 1), out, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, 1), None, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, 1, True), None, 1, 7, 5, 1) == -1
    # no other column bit goes with it, the two texture bits do not go together, the parameters not without a bit
    for other in (1, _hip.RPX_WEIGHTED, _hip.RPX_RELATE, _hip.RPX_ROBUST, _hip.RPX_NEIGHBORS, _hip.RPX_NEAREST,
                  _hip.RPX_TEXTURE_COUNTS, 1 << 31):
        assert _raw(ctx, lab, u16, U, 1, ranges, (cols(2, 1) | other) - (other >> 31 << 32), out, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, 1) & ~_hip.RPX_TEXTURE, out, 1, 7, 5, 1) == -1
    # overlapping operands, as every other call of the entry point refuses them
    assert _raw(ctx, lab, u16, U, 1, out, cols(2, 1), out, 1, 7, 5, 1) == -1
    msg = _hip.load_library().amt_last_error()
    assert b"amt_regionprops_ext: " in msg and b"must not alias" in msg
    assert _raw(ctx, glcm, u16, U, 1, ranges, cols(2, 1, True), glcm, 1, 7, 5, 1) == -1
    # no plane / no label: nothing to do, nothing written
    for counts, buf in ((False, out), (True, glcm)):
        assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, 1, counts), buf, 0, 7, 5, 1) == 0
        assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, 1, counts), buf, 1, 7, 5, 0) == 0
    assert out.numpy().ravel().tolist() == [5.0] * 52 and glcm.numpy().ravel().tolist() == [7] * 16
    # the calls themselves: one constant label in level 1 of 2; each writes its own output and nothing else
    assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, 1), out, 1, 7, 5, 1) == 0
    assert out.numpy()[0, 0, 0].tolist() == [[1, 0, 1, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0]] * 4
    assert glcm.numpy().ravel().tolist() == [7] * 16
    out2 = ctx.asarray(np.full((1, 1, 1, 4, 13), 5.0))
    assert _raw(ctx, lab, u16, U, 1, ranges, cols(2, 1, True), glcm, 1, 7, 5, 1) == 0
    assert glcm.numpy()[0, 0, 0, :, 1, 1].tolist() == [2 * 7 * 4, 2 * 6 * 4, 2 * 6 * 5, 2 * 6 * 4] and glcm.numpy().sum() == 212
    assert out2.numpy().ravel().tolist() == [5.0] * 52
    # the existing bits are as they were
    wtable = ctx.empty((1, 1, 1, 4), np.float64)
    assert _raw(ctx, lab, u16, U, 1, None, _hip.RPX_ROBUST, wtable, 1, 7, 5, 1) == 0
    assert wtable.numpy().ravel().tolist() == [9.0, 9.0, 9.0, 0.0]


def test_argument_errors_of_hipops(ctx):
    from arcadia_microscopy_tools_amd import hipops
    from arcadia_microscopy_tools_amd.device import DeviceArray

    lab = ctx.asarray(np.ones((7, 5), np.int32))
    img = ctx.asarray(np.full((1, 7, 5), 3, np.uint16))
    with pytest.raises(TypeError):
        hipops.texture(lab, ctx.asarray(np.ones((1, 7, 5), np.uint8)), 1)
    with pytest.raises(TypeError):
        hipops.texture(ctx.asarray(np.ones((7, 5), np.uint16)), img, 1)
    with pytest.raises(ValueError):
        hipops.texture(lab, ctx.asarray(np.ones((1, 5, 7), np.uint16)), 1)
    with pytest.raises(ValueError, match="levels"):
        hipops.texture(lab, img, 1, levels=65)
    with pytest.raises(ValueError, match="distance"):
        hipops.texture(lab, img, 1, distance=0)
    with pytest.raises(ValueError, match="distance"):
        hipops.texture(lab, img, 1, distance=256)
    with pytest.raises(ValueError, match="ranges"):
        hipops.texture(lab, img, 1, ranges=(1, 2, 3))
    with pytest.raises(ValueError):
        hipops.texture(lab, img, 1, out=ctx.empty((1, 1, 1, 4, 12), np.float64))
    with pytest.raises(ValueError):
        hipops.texture(lab, img, 1, glcm=ctx.empty((1, 1, 1, 4, 8, 7), np.uint32))
    with pytest.raises(ValueError):
        hipops.texture(lab, img, 1, glcm=ctx.empty((1, 1, 1, 4, 8, 8), np.int32))
    # an out / glcm that overlaps an input: refused, nothing written
    big = ctx.asarray(np.ones((4 * 13 + 35,), np.float64))  # room for the table behind a float64 "image"
    f64 = big[:35].reshape((1, 7, 5))
    with pytest.raises(ValueError, match="alias"):
        hipops.texture(lab, f64, 1, out=big[8:60].reshape((1, 1, 1, 4, 13)))
    words = ctx.asarray(np.ones((4 * 64 + 35,), np.int32))
    inside = DeviceArray(ctx, words.ptr + 64, (1, 1, 1, 4, 8, 8), np.uint32, base=words)  # 256 words from word 16
    with pytest.raises(ValueError, match="alias"):
        hipops.texture(words[:35].reshape((7, 5)), img, 1, glcm=inside)
    assert big.numpy().tolist() == [1.0] * 87 and words.numpy().tolist() == [1] * 291
    shape0 = hipops.texture(lab, img, 0, glcm=True)
    assert shape0[0].shape == (1, 0, 1, 4, 13) and shape0[1].shape == (1, 0, 1, 4, 8, 8)  # max_label == 0 writes nothing
    out = ctx.empty((1, 1, 1, 4, 13), np.float64)
    counts = ctx.empty((1, 1, 1, 4, 8, 8), np.uint32)
    got = hipops.texture(lab, img, 1, out=out, glcm=counts, ranges=(0, 8))
    assert got[0] is out and got[1] is counts
    assert out.numpy()[0, 0, 0, 0].tolist() == [1, 0, 1, 0, 1, 6, 0, 0, 0, 0, 0, 0, 0] and counts.numpy()[0, 0, 0, 0, 3, 3] == 56
    assert hipops.texture(lab, img, 1, ranges=(0, 8)).numpy().tobytes() == out.numpy().tobytes()


def _images(shape, dtype):
    from arcadia_microscopy_tools_amd.channels import DAPI, FITC

    rng = np.random.RandomState(31)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    wave = 0.5 + 0.25 * np.sin(yy / 2.3) * np.cos(xx / 3.1)

    def make():
        v = wave + 0.25 * rng.uniform(-1, 1, shape)
        if dtype == np.uint8:
            return (v * 255).astype(np.uint8)
        if dtype == np.uint16:
            return (v * 65535).astype(np.uint16)
        return (v - 0.5) * 100.0

    return {FITC: make(), DAPI: make()}


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float64], ids=lambda d: np.dtype(d).name)
def test_cell_texture_on_plain_expanded_and_ring_masks(ctx, dtype):
    from arcadia_microscopy_tools_amd.channels import DAPI, FITC
    from arcadia_microscopy_tools_amd.masks import SegmentationMask
    from arcadia_microscopy_tools_amd.segment import texture_keys

    shape = (64, 64)
    nuclei = tc.blobs(shape, 77, 9, 5.0).astype(np.int64)
    images = _images(shape, dtype)
    stack = np.stack([images[FITC], images[DAPI]])
    mask = SegmentationMask(nuclei, images, remove_edge_cells=False)
    keys_before = list(mask.cell_properties)
    for m in (mask, mask.expanded(4), mask.ring(4)):
        lab, k = m.label_image, m.num_cells
        assert k >= 2
        got = m.cell_texture()
        assert list(got) == texture_keys([FITC, DAPI]) and len(got) == 2 * 4 * 13
        want, _ = tr.texture_stack(lab, stack, k)
        table = np.stack([got[key] for key in got], axis=1).reshape(k, 2, 4, 13)
        assert all(v.dtype == np.float64 and v.shape == (k,) for v in got.values())
        assert tc.compare(table, np.zeros((0,), np.uint32), want, np.zeros((0,), np.uint32))[0]
        # other parameters, the mean over the directions, ranges as a mapping (FITC keeps its own extrema)
        got = m.cell_texture(levels=16, distance=3, ranges={DAPI: (float(stack[1].min()) + 3, float(stack[1].max()) - 7)},
                             angles="mean")
        assert list(got) == texture_keys([FITC, DAPI], 3, "mean") and len(got) == 2 * 13
        rng = tr.default_ranges(stack)
        rng[1] = (rng[1, 0] + 3, rng[1, 1] - 7)
        want = tr.nanmean_angles(tr.texture_stack(lab, stack, k, 16, 3, rng)[0])
        table = np.stack([got[key] for key in got], axis=1).reshape(k, 2, 13)
        assert tc.compare(table, np.zeros((0,), np.uint32), want, np.zeros((0,), np.uint32))[0]
        pair = m.cell_texture(ranges=(float(stack.min()), float(stack.max())))
        want, _ = tr.texture_stack(lab, stack, k, ranges=(float(stack.min()), float(stack.max())))
        table = np.stack([pair[key] for key in pair], axis=1).reshape(k, 2, 4, 13)
        assert tc.compare(table, np.zeros((0,), np.uint32), want, np.zeros((0,), np.uint32))[0]
    ring = mask.ring(4)
    assert len(ring.parent_labels) == ring.num_cells == len(ring.cell_texture()["texture_entropy_dapi_1_90"])
    with pytest.raises(ValueError, match="intensity images"):
        SegmentationMask(nuclei, remove_edge_cells=False).cell_texture()
    # cell_properties and its names stay as they were
    assert list(mask.cell_properties) == keys_before and not [key for key in mask.cell_properties if "texture" in key]


def test_mean_of_a_cell_without_any_pair_is_nan_without_a_warning(ctx):
    import warnings

    from arcadia_microscopy_tools_amd.channels import DAPI
    from arcadia_microscopy_tools_amd.masks import SegmentationMask

    nuclei = np.zeros((16, 16), np.int64)
    nuclei[3, 4] = 1            # a single pixel: no pair anywhere
    nuclei[8, 2:9] = 2          # a row: direction 0 only
    image = np.arange(256, dtype=np.uint16).reshape(16, 16)
    mask = SegmentationMask(nuclei, {DAPI: image}, remove_edge_cells=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mean = mask.cell_texture(angles="mean")
        each = mask.cell_texture()
    assert np.isnan(mean["texture_contrast_dapi_1"][0]) and mean["texture_contrast_dapi_1"][1] == each["texture_contrast_dapi_1_0"][1]
    assert np.isnan(each["texture_contrast_dapi_1_90"]).all() and not np.isnan(each["texture_contrast_dapi_1_0"][1])


def test_cases_under_poison(ctx, tmp_path):
    out = tmp_path / "texture.json"
    res = poison_child.run_module("tests.texture_cases", out, CHILD_TIMEOUT_S, "the poisoned texture cases")
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} results differ from the reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for shape in tc.SHAPES + [tc.BIG]:
        for kind in tc.KINDS:
            here.update({json.dumps(r["key"]): r["sha256"] for r in _shape_run(ctx, shape, kind)["records"]})
    there = {json.dumps(r["key"]): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
