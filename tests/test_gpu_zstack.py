"""Z-stacks on the device: every case of tests/zstack_cases.py byte-equal to the plain numpy rule of
tests/zstack_reference.py for the five ops (the float64 mean included), focus_stack against z_take of focus_index, two runs
identical, batch stacks equal to their single runs, ``out=``, the raw entry point with its refusals on a live context, the
``operations`` functions on numpy and device input and in a Pipeline, ``project_z`` for every method, and the table once
more in a child process under AMT_DEBUG_POISON=1."""
import ctypes
import warnings

import numpy as np
import pytest

import poison_child
import zstack_cases as cases
import zstack_reference as ref
from arcadia_microscopy_tools_amd import _hip, hipops, operations
from arcadia_microscopy_tools_amd.channels import DAPI, FITC
from arcadia_microscopy_tools_amd.device import DeviceArray
from arcadia_microscopy_tools_amd.exceptions import MetadataWarning
from arcadia_microscopy_tools_amd.microscopy import DeviceImage, MicroscopyImage
from arcadia_microscopy_tools_amd.pipeline import ImageOperation, Pipeline

pytestmark = pytest.mark.gpu

# the child imports the package, creates a context and runs the table (about a second in process, references included)
CHILD_TIMEOUT_S = 120

_DIGESTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _case(name):
    return [c for c in cases.cases() if c[0] == name][0]


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c[0])
def test_every_op_equals_the_rule(ctx, case):
    want = cases.reference(case)
    got = cases.run_case(ctx, case)
    assert set(got) == set(want)
    for key in want:
        _DIGESTS[f"{case[0]} / {key}"] = cases.digest(got[key])
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        differ = got[key] != want[key]
        assert got[key].tobytes() == want[key].tobytes(), \
            f"{key}: {int(differ.sum())} entries differ, the first at {tuple(np.argwhere(differ)[0]) if differ.any() else None}"


@pytest.mark.parametrize("name", ["odd 70 x 131 Z 5 r 4", f"seam {cases.TH + 1} x {cases.TW + 1} r 15", "ties 0..3", "Z 257 9 x 11 uint8",
                                  "batch of three"])
def test_focus_stack_is_take_of_index_and_two_runs_agree(ctx, name):
    _, stack, r = _case(name)
    d = ctx.asarray(stack)
    index = hipops.focus_index(d, r)
    fused = hipops.focus_stack(d, r).numpy()
    assert fused.tobytes() == hipops.z_take(d, index).numpy().tobytes()
    assert hipops.focus_index(d, r).numpy().tobytes() == index.numpy().tobytes()
    assert hipops.focus_stack(d, r).numpy().tobytes() == fused.tobytes()
    assert hipops.focus_sums(d).numpy().tobytes() == hipops.focus_sums(d).numpy().tobytes()


def test_batch_stacks_equal_single_runs(ctx):
    case = _case("batch of three")
    _, stack, r = case
    whole = cases.run_case(ctx, case)
    index = cases.take_index(case)
    for n in range(len(stack)):
        d = ctx.asarray(stack[n:n + 1])
        for m in ("max", "min", "mean"):
            assert hipops.z_project(d, m).numpy().tobytes() == whole[m][n:n + 1].tobytes(), (n, m)
        assert hipops.focus_sums(d).numpy().tobytes() == whole["sums"][n:n + 1].tobytes(), n
        assert hipops.focus_index(d, r).numpy().tobytes() == whole["index"][n:n + 1].tobytes(), n
        assert hipops.focus_stack(d, r).numpy().tobytes() == whole["stack"][n:n + 1].tobytes(), n
        assert hipops.z_take(d, ctx.asarray(index[n:n + 1])).numpy().tobytes() == whole["take"][n:n + 1].tobytes(), n
    # a view of the batch: stacks at an offset
    tail = ctx.asarray(stack)[1:]
    assert hipops.focus_stack(tail, r).numpy().tobytes() == whole["stack"][1:].tobytes()


def test_out_is_used(ctx):
    case = _case("odd 70 x 131 Z 5 r 1")
    _, stack, r = case
    want = cases.reference(case)
    d = ctx.asarray(stack)
    N, Z, H, W = stack.shape
    for key, call, shape, dtype in (
            ("max", lambda o: hipops.z_project(d, "max", out=o), (N, H, W), np.uint16),
            ("mean", lambda o: hipops.z_project(d, "mean", out=o), (N, H, W), np.float64),
            ("sums", lambda o: hipops.focus_sums(d, out=o), (N, Z, 4), np.int64),
            ("index", lambda o: hipops.focus_index(d, r, out=o), (N, H, W), np.uint16),
            ("stack", lambda o: hipops.focus_stack(d, r, out=o), (N, H, W), np.uint16),
            ("take", lambda o: hipops.z_take(d, ctx.asarray(cases.take_index(case)), out=o), (N, H, W), np.uint16)):
        o = ctx.empty(shape, dtype)
        assert call(o) is o
        assert o.numpy().tobytes() == want[key].tobytes(), key
    with pytest.raises(ValueError, match="alias"):
        hipops.z_project(d, "max", out=d[0][0:1])
    empty = hipops.focus_stack(ctx.empty((0, 3, 5, 7), np.uint16), 2)
    assert isinstance(empty, DeviceArray) and empty.shape == (0, 5, 7)


def test_raw_entry_point(ctx):
    lib = _hip.load_library()
    case = _case("odd 70 x 131 Z 5 r 1")
    _, stack, r = case
    want = cases.reference(case)
    d = ctx.asarray(stack)
    o16 = ctx.empty((1, 70, 131), np.uint16)
    o64 = ctx.empty((1, 70, 131), np.float64)
    sums = ctx.empty((1, 5, 4), np.int64)
    index = ctx.asarray(cases.take_index(case))
    one, three = np.ones((1, 1), np.uint8), np.ones((3, 3), np.uint8)
    room = ctx.zeros((4, 5, 70, 131), np.uint16)  # a source that is long enough under every dtype code

    def call(op, dst, fp=one, Z=5, cval=0.0, minuend=None, n=1, dtype=_hip.U16, src=d):
        fp = np.ascontiguousarray(fp, np.uint8)
        return lib.amt_rank_filter(ctx.handle, src.ptr, dst.ptr, dtype, n, 70, 131, fp.ctypes.data_as(ctypes.c_void_p),
                                   fp.shape[0], fp.shape[1], op, Z, float(cval), minuend)

    def err():
        return lib.amt_last_error().decode()

    assert call(10, o16) == 0 and o16.numpy().tobytes() == want["max"].tobytes()
    assert call(10, o16, cval=1.0) == 0 and o16.numpy().tobytes() == want["min"].tobytes()
    assert call(10, o64, cval=2.0) == 0 and o64.numpy().tobytes() == want["mean"].tobytes()
    assert call(11, sums) == 0 and sums.numpy().tobytes() == want["sums"].tobytes()
    assert call(12, o16, fp=three) == 0 and o16.numpy().tobytes() == want["index"].tobytes()
    assert call(13, o16, fp=three * 9) == 0 and o16.numpy().tobytes() == want["stack"].tobytes()
    assert call(14, o16, minuend=index.ptr) == 0 and o16.numpy().tobytes() == want["take"].tobytes()
    # nplanes == 0 writes nothing
    poison = np.full((1, 70, 131), 0xBEEF, np.uint16)
    ctx.copy_from_host_async(o16, poison)
    for op in (10, 12, 13):
        assert call(op, o16, fp=three, n=0) == 0
    assert call(14, o16, minuend=index.ptr, n=0) == 0
    assert np.array_equal(o16.numpy(), poison)
    # the refusals, with a live context
    for op in (10, 11, 12, 13, 14):
        dst = sums if op == 11 else o16
        m = index.ptr if op == 14 else None
        assert call(op, dst, fp=three, Z=0, minuend=m) == -1 and "Z (mode)" in err()
        assert call(op, dst, fp=three, Z=65536, minuend=m) == -1
        assert call(op, dst, fp=three, dtype=_hip.I32, minuend=m, src=room) == -1 and "dtype" in err()
        assert call(op, d, fp=three, minuend=m) == -1 and "alias" in err()
        assert call(op, dst, fp=three, minuend=None if op == 14 else index.ptr) == -1 and "minuend" in err()
    for op in (11, 12, 13):
        assert call(op, o16, fp=three, dtype=_hip.F64, src=room) == -1 and "dtype" in err()
    for op in (12, 13):
        for fp in (np.ones((3, 5)), np.ones((33, 33)), np.eye(3), np.ones((2, 2))):
            assert call(op, o16, fp=fp) == -1 and "footprint" in err()
    assert call(10, o16, cval=3.0) == -1 and "cval" in err()
    assert call(14, index, minuend=index.ptr) == -1
    assert np.array_equal(o16.numpy(), poison)  # no refusal wrote
    # op 7 is still no op of this call, and the filters are what they were on one plane
    plane = ctx.asarray(stack[0, 0])
    assert call(7, o16, fp=three, Z=1, src=plane) == -1 and "op must be" in err()
    from scipy import ndimage as ndi

    for op, fn in ((0, ndi.grey_erosion), (1, ndi.grey_dilation), (2, ndi.median_filter)):
        assert call(op, o16, fp=three, Z=_hip.MODE_NEAREST, src=plane) == 0
        assert np.array_equal(o16.numpy()[0], fn(stack[0, 0], footprint=three, mode="nearest")), op


def test_operations_on_numpy_and_device_input(ctx):
    stack = _case("planted depth map")[1][0]
    for m in ("max", "min", "mean"):
        got = operations.z_project(stack, m)
        assert isinstance(got, np.ndarray) and got.tobytes() == ref.z_project(stack, m).tobytes() and got.shape == (70, 131)
    small = stack.astype(np.uint8)
    assert operations.z_project(small, "max").tobytes() == small.max(axis=0).tobytes()
    floats = _case("float64 70 x 131")[1][0]
    assert operations.z_project(floats, "mean").tobytes() == np.mean(floats, axis=0).tobytes()
    for method in operations.FOCUS_METHODS:
        got = operations.focus_scores(stack, method)
        assert got.dtype == np.float64 and got.tobytes() == ref.focus_scores(stack, method).tobytes(), method
        z = ref.best_focus_index(stack, method)
        plane, zi = operations.best_focus(stack, method, return_index=True)
        assert zi == z and np.array_equal(plane, stack[z])
    equal = _case("equal planes")[1][0]
    assert operations.best_focus(equal, return_index=True)[1] == 0  # the smallest z among equals
    for radius, smooth in ((4, 0), (1, 3), (0, 5), (15, 15)):
        want, windex = ref.extended_depth_of_field(stack, radius, smooth)
        got = operations.extended_depth_of_field(stack, radius=radius, smooth=smooth)
        assert got.dtype == np.uint16 and got.tobytes() == want.tobytes(), (radius, smooth)
        got, gindex = operations.extended_depth_of_field(stack, radius, smooth, return_index=True)
        assert got.tobytes() == want.tobytes() and gindex.dtype == np.uint16 and gindex.tobytes() == windex.tobytes()
    # device input stays on the device; best_focus is a view of the stack, not a copy
    d = ctx.asarray(stack)
    proj = operations.z_project(d, "mean")
    assert isinstance(proj, DeviceArray) and proj.shape == (70, 131) and proj.numpy().tobytes() == ref.z_project(stack, "mean").tobytes()
    plane, z = operations.best_focus(d, return_index=True)
    assert isinstance(plane, DeviceArray) and plane.ptr == d.ptr + z * 70 * 131 * 2 and np.array_equal(plane.numpy(), stack[z])
    edf, index = operations.extended_depth_of_field(d, 4, 3, return_index=True)
    want, windex = ref.extended_depth_of_field(stack, 4, 3)
    assert isinstance(edf, DeviceArray) and isinstance(index, DeviceArray)
    assert edf.numpy().tobytes() == want.tobytes() and index.numpy().tobytes() == windex.tobytes()
    assert operations.focus_scores(d).tobytes() == ref.focus_scores(stack, "laplacian_variance").tobytes()


def test_operations_in_a_pipeline(ctx):
    stack = _case("planted depth map")[1][0]
    for op, plane in ((ImageOperation(operations.z_project, "max"), ref.z_project(stack, "max")),
                      (ImageOperation(operations.best_focus, method="brenner"), stack[ref.best_focus_index(stack, "brenner")]),
                      (ImageOperation(operations.extended_depth_of_field, radius=2), ref.focus_stack(stack, 2))):
        pipe = Pipeline([op, ImageOperation(operations.apply_threshold, "otsu")])
        got = pipe(stack)
        want = operations.apply_threshold(plane, "otsu")
        assert got.dtype == np.bool_ and got.shape == (70, 131) and np.array_equal(got, want) and 0 < got.mean() < 1


def _project_reference(arr, axes, method, ref_channel=None, **kw):
    """project_z's expectation, stack by stack from the reference"""
    zax, cax = axes.index("Z"), axes.index("C")
    lead = np.moveaxis(arr, zax, -3)
    lead_axes = [a for a in axes[:-2] if a != "Z"]
    out = np.empty(lead.shape[:-3] + lead.shape[-2:], np.float64 if method == "mean" else arr.dtype)
    for at in np.ndindex(*lead.shape[:-3]):
        stack = lead[at]
        chooser = stack
        if ref_channel is not None:
            src = list(at)
            src[lead_axes.index("C")] = ref_channel
            chooser = lead[tuple(src)]
        if method in ("max", "min", "mean"):
            out[at] = ref.z_project(stack, method)
        elif method == "best_focus":
            out[at] = stack[ref.best_focus_index(chooser, kw.get("focus_method", "laplacian_variance"))]
        else:
            out[at] = ref.z_take(stack, ref.extended_depth_of_field(chooser, kw.get("radius", 4), kw.get("smooth", 0))[1])
    return out


@pytest.mark.parametrize("axes,shape", [("CZYX", (2, 3, 70, 131)), ("TZCYX", (2, 3, 2, 70, 131))], ids=["CZYX", "TZCYX"])
def test_project_z(ctx, axes, shape):
    rng = np.random.default_rng(len(axes))
    planted = cases.planted_stack((70, 131), 3, 7)
    arr = rng.integers(0, 65536, size=shape, dtype=np.uint16)
    # channel 0 carries a planted depth map, so that the reference channel's choice differs from channel 1's own
    zax, cax = axes.index("Z"), axes.index("C")
    view = np.moveaxis(arr, (cax, zax), (0, 1))
    view[0][...] = planted.reshape((3,) + (1,) * (arr.ndim - 4) + (70, 131))
    img = MicroscopyImage.from_array(arr, [DAPI, FITC], axes=axes)
    sizes = {a: s for a, s in zip(axes, shape) if a != "Z"}
    runs = [("max", None, {}), ("min", None, {}), ("best_focus", None, {}), ("best_focus", None, {"focus_method": "brenner"}),
            ("best_focus", 0, {}), ("best_focus", 1, {}), ("edf", None, {}), ("edf", None, {"radius": 1, "smooth": 3}),
            ("edf", 0, {"radius": 2}), ("edf", 1, {"radius": 2, "smooth": 3})]
    for method, ref_channel, kw in runs:
        got = img.project_z(method, reference_channel=None if ref_channel is None else (DAPI, FITC)[ref_channel], **kw)
        want = _project_reference(arr, axes, method, ref_channel, **kw)
        assert isinstance(got, MicroscopyImage) and dict(got.sizes) == sizes and list(got.sizes) == list(sizes)
        assert got.intensities.dtype == np.uint16 and got.intensities.tobytes() == want.tobytes(), (method, ref_channel, kw)
        assert got.channels == [DAPI, FITC] and not got.dimensions.is_zstack
    with pytest.warns(MetadataWarning):
        mean = img.project_z("mean")
    assert mean.intensities.dtype == np.float64 and mean.intensities.tobytes() == _project_reference(arr, axes, "mean").tobytes()
    # the choice on the reference channel is not channel 1's own
    assert img.project_z("edf", reference_channel=DAPI).intensities.tobytes() != img.project_z("edf").intensities.tobytes()
    if axes == "CZYX":  # the device image: stacks contiguous
        dimg = img.to_device(ctx)
        for method, ref_channel, kw in runs:
            got = dimg.project_z(method, reference_channel=None if ref_channel is None else (DAPI, FITC)[ref_channel], **kw)
            assert isinstance(got, DeviceImage) and isinstance(got.data, DeviceArray) and dict(got.image.sizes) == sizes
            assert got.data.numpy().tobytes() == _project_reference(arr, axes, method, ref_channel, **kw).tobytes()
        assert np.array_equal(dimg.project_z("max").get_channel_intensities(FITC).numpy(), arr[1].max(axis=0))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert dimg.project_z("mean").data.dtype == np.float64
    assert zax == 1
    one = MicroscopyImage.from_array(np.ascontiguousarray(arr[:, :1]), [DAPI, FITC], axes=axes)
    assert one.sizes["Z"] == 1  # Z == 1 works
    for method in ("max", "best_focus", "edf"):
        assert np.array_equal(one.project_z(method).intensities, np.squeeze(one.intensities, axis=zax))


def test_table_under_poison(ctx, tmp_path):
    """The whole table in a fresh child process with scratch and allocations poisoned: every result equals its reference,
    no scratch check comes back dirty, and every digest equals this process's."""
    here = dict(_DIGESTS)
    for case in cases.cases():
        if f"{case[0]} / max" not in here:
            for key, arr in cases.run_case(ctx, case).items():
                here[f"{case[0]} / {key}"] = cases.digest(arr)
    planted = _case("planted depth map")[1][0]
    here["planted depth map / edf smooth 3"] = cases.digest(operations.extended_depth_of_field(planted, radius=4, smooth=3))
    out = tmp_path / "zstack.json"
    res = poison_child.run_module("tests.zstack_cases", out, CHILD_TIMEOUT_S, "the poisoned table")
    there = res["cases"]
    wrong = [k for k, v in there.items() if not v["equal"]]
    assert not wrong, f"{len(wrong)} results differ from the rule under poison; the first: {wrong[:10]}"
    dirty = [(k, v["dirty"]) for k, v in there.items() if v["dirty"] is not None]
    assert not dirty, f"{len(dirty)} scratch checks came back dirty; the first: {dirty[:5]}"
    poison_child.assert_unmoved(here, {k: v["sha256"] for k, v in there.items()})
