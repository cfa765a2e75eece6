"""skeletonize / neighbor_classes on the device: every case of tests/skeleton_cases.py byte-equal to the plain numpy rule of
tests/skeleton_reference.py, two runs identical, the library's own iteration count, the earlier codes of amt_binary_morph
unchanged, the operators in a Pipeline, and the table once more in a child process under AMT_DEBUG_POISON=1 (a result that
depends on what LDS padding or scratch held is the thinning kernel's most likely defect)."""
import ctypes
import os
import re

import numpy as np
import pytest

import skeleton_cases as cases
import skeleton_reference as ref
import poison_child
from arcadia_microscopy_tools_amd import _hip, hipops, operations
from arcadia_microscopy_tools_amd.device import DeviceArray
from arcadia_microscopy_tools_amd.pipeline import ImageOperation, Pipeline

pytestmark = pytest.mark.gpu

# the child imports the package, creates a context and runs the table (a few seconds in process, references included)
CHILD_TIMEOUT_S = 120

_DIGESTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _first_difference(got, want, names):
    for i, name in enumerate(names):
        if not np.array_equal(got[i], want[i]):
            y, x = np.argwhere(got[i] != want[i])[0]
            return f"plane {i} ({name}): {int((got[i] != want[i]).sum())} pixels differ, the first at ({y}, {x})"
    return None


@pytest.mark.parametrize("case", cases.skeleton_cases(), ids=lambda c: c[0])
def test_skeleton_equals_the_rule(ctx, case):
    want, _ = cases.skeleton_reference(case)
    got = cases.run_skeleton(ctx, case)
    _DIGESTS[case[0]] = cases.digest(got)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert _first_difference(got, want, case[3]) is None


@pytest.mark.parametrize("case", cases.class_cases(), ids=lambda c: c[0])
def test_classes_equal_the_count(ctx, case):
    want = cases.class_reference(case)
    got = cases.run_classes(ctx, case)
    _DIGESTS[case[0]] = cases.digest(got)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert _first_difference(got, want, case[3]) is None


def test_two_runs_give_identical_bytes(ctx):
    for case in cases.skeleton_cases():
        if case[0] in ("seam disks", "bar in a frame", "batch of three", f"contents {cases.ROWS + 1} x {cases.TILE_W + 1}"):
            a, b = cases.run_skeleton(ctx, case), cases.run_skeleton(ctx, case)
            assert np.array_equal(a, b), case[0]


def test_batch_planes_equal_their_single_plane_results(ctx):
    case = next(c for c in cases.skeleton_cases() if c[0] == "batch of three")
    together = cases.run_skeleton(ctx, case)
    counts = cases.skeleton_reference(case)[1]
    assert counts[0] == 1 and counts[1] < counts[2] and counts[2] == cases.bar_iterations()
    for i, name in enumerate(case[3]):
        alone = hipops.skeletonize(ctx.asarray(case[2][i])).numpy(dtype=np.uint8)
        assert np.array_equal(together[i], alone), name


def test_iteration_count_is_the_rules(ctx, capfd):
    """AMT_DEBUG_SKELETONIZE=1: the library's count on the bar equals the reference's, with and without a limit."""
    d = ctx.asarray(cases.bar_framed())
    n = cases.bar_iterations()
    old = os.environ.get("AMT_DEBUG_SKELETONIZE")
    os.environ["AMT_DEBUG_SKELETONIZE"] = "1"
    try:
        for k, want in ((0, n), (n + 1, n), (n, n), (n - 1, n - 1), (3, 3)):
            capfd.readouterr()
            hipops.skeletonize(d, k)
            line = capfd.readouterr().err
            m = re.search(r"amt skeletonize: iterations=(\d+) launches=(\d+) syncs=(\d+)", line)
            assert m, line
            assert int(m.group(1)) == want, (k, line)
            if k:
                assert int(m.group(2)) <= -(-2 * k // cases.T), (k, line)
    finally:
        if old is None:
            del os.environ["AMT_DEBUG_SKELETONIZE"]
        else:
            os.environ["AMT_DEBUG_SKELETONIZE"] = old


def test_out_argument_and_truth_values(ctx):
    p = cases.random((cases.ROWS + 1, 129), 0.65, 3)
    want = ref.skeletonize(p)[0]
    d = ctx.asarray((p * 200).astype(np.uint8))  # a truth value per pixel, not 0 / 1
    o = ctx.empty(p.shape, np.uint8)
    assert hipops.skeletonize(d, out=o) is o
    assert np.array_equal(o.numpy(dtype=np.uint8), want)
    assert hipops.neighbor_classes(d, 2, out=o) is o
    assert np.array_equal(o.numpy(dtype=np.uint8), ref.neighbor_classes(p, 2))
    empty = hipops.skeletonize(ctx.empty((0, 5, 7), np.uint8))
    assert empty.shape == (0, 5, 7)


def test_raw_entry_point(ctx):
    """Codes 7 and 8 through amt_binary_morph itself, their refusals with a live context, and codes 0-6 unchanged."""
    import area_filters_reference as af

    lib = _hip.load_library()
    plane = cases.random((70, 131), 0.65, 1)
    d = ctx.asarray(plane)
    o = ctx.empty(plane.shape, np.uint8)

    def call(fp, op, value, dst=o, n=1):
        fp = np.ascontiguousarray(fp, np.uint8)
        return lib.amt_binary_morph(ctx.handle, d.ptr, dst.ptr, n, 70, 131, fp.ctypes.data_as(ctypes.c_void_p), fp.shape[0],
                                    fp.shape[1], op, value)

    assert call(ref.FULL, 7, 0) == 0
    assert np.array_equal(o.numpy(dtype=np.uint8), ref.skeletonize(plane)[0])
    assert call(ref.FULL, 7, 2) == 0
    assert np.array_equal(o.numpy(dtype=np.uint8), ref.skeletonize(plane, 2)[0])
    for fp, conn in ((ref.CROSS, 1), (ref.FULL, 2)):
        assert call(fp, 8, -5) == 0  # border_value is ignored
        assert np.array_equal(o.numpy(dtype=np.uint8), ref.neighbor_classes(plane, conn))
    assert call(ref.CROSS, 7, 0) == -1 and "footprint" in lib.amt_last_error().decode()
    assert call(hipops.disk(2), 7, 0) == -1 and call(hipops.disk(2), 8, 0) == -1
    assert call(ref.FULL, 7, -1) == -1 and "max_iter" in lib.amt_last_error().decode()
    assert call(ref.FULL, 9, 0) == -1 and "0..8" in lib.amt_last_error().decode()
    assert call(ref.FULL, 7, 0, dst=d) == -1 and "alias" in lib.amt_last_error().decode()
    assert call(ref.FULL, 7, 0, n=0) == 0 and call(ref.CROSS, 8, 0, n=0) == 0
    named = {0: hipops.binary_erosion, 1: hipops.binary_dilation, 2: hipops.binary_opening, 3: hipops.binary_closing}
    for op, fn in named.items():
        assert call(hipops.disk(2), op, 1 if op == 0 else 0) == 0
        assert np.array_equal(o.numpy(dtype=np.uint8), fn(d, hipops.disk(2)).numpy(dtype=np.uint8)), op
    for st in (ref.CROSS, ref.FULL):
        conn = 1 if st is ref.CROSS else 2
        assert call(st, 4, 0) == 0
        assert np.array_equal(o.numpy(dtype=np.uint8), hipops.binary_fill_holes(d, st).numpy(dtype=np.uint8))
        assert call(st, 5, 6) == 0
        assert np.array_equal(o.numpy(dtype=np.uint8), hipops.remove_small_objects(d, 6, conn).numpy(dtype=np.uint8))
        assert np.array_equal(o.numpy(dtype=np.uint8), af.remove_small_objects(plane, 6, st))
        assert call(st, 6, 6) == 0
        assert np.array_equal(o.numpy(dtype=np.uint8), hipops.remove_small_holes(d, 6, conn).numpy(dtype=np.uint8))


def test_operators_in_a_pipeline(ctx):
    rng = np.random.default_rng(11)
    img = (rng.random((cases.ROWS + 9, 150)) * 1000).astype(np.uint16)
    img[20:50, 30:120] += 3000  # a slab the threshold keeps
    mask = img > 2000
    want = ref.skeletonize(mask)[0]
    got = operations.skeletonize(mask)
    assert got.dtype == np.bool_ and np.array_equal(got, want.astype(bool))
    assert np.array_equal(operations.skeletonize(mask, max_iter=2), ref.skeletonize(mask, 2)[0].astype(bool))
    nodes = operations.skeleton_nodes(got)
    assert nodes.dtype == np.uint8 and np.array_equal(nodes, ref.neighbor_classes(want, 2))
    assert np.array_equal(operations.skeleton_nodes(got, connectivity=1), ref.neighbor_classes(want, 1))
    # after apply_threshold in a Pipeline: the mask and the skeleton stay on the device, one download at the end
    thr = operations.apply_threshold(img, "otsu")
    want = ref.skeletonize(thr)[0]
    assert 0 < want.sum() < thr.sum()
    thin = Pipeline([ImageOperation(operations.apply_threshold, "otsu"), ImageOperation(operations.skeletonize)])
    assert thin._device_chain_applies(img)
    got = thin(img)
    assert got.dtype == np.bool_ and np.array_equal(got, want.astype(bool))
    pipe = Pipeline([ImageOperation(operations.apply_threshold, "otsu"), ImageOperation(operations.skeletonize, max_iter=40),
                     ImageOperation(operations.skeleton_nodes, connectivity=2)])
    assert pipe._device_chain_applies(img)
    got = pipe(img)
    assert got.dtype == np.uint8 and np.array_equal(got, ref.neighbor_classes(want, 2))
    # device input: a DeviceArray stays on the device
    d = ctx.asarray(thr)
    skel = operations.skeletonize(d)
    assert isinstance(skel, DeviceArray) and skel.is_bool and np.array_equal(skel.numpy(), want.astype(bool))
    nodes = operations.skeleton_nodes(skel, 1)
    assert isinstance(nodes, DeviceArray) and np.array_equal(nodes.numpy(dtype=np.uint8), ref.neighbor_classes(want, 1))
    with pytest.raises(ValueError, match="must be a 2D array"):
        operations.skeletonize(ctx.asarray(np.zeros((2, 8, 8), np.uint8)))
    for shape in ((0, 5), (3, 0)):
        e = operations.skeletonize(ctx.empty(shape, np.uint8))
        assert isinstance(e, DeviceArray) and e.shape == shape


def test_table_under_poison(ctx, tmp_path):
    """The whole table in a fresh child process with scratch and allocations poisoned: every result equals its reference,
    no scratch check comes back dirty, and every digest equals this process's."""
    here = dict(_DIGESTS)
    for case in cases.skeleton_cases():
        if case[0] not in here:
            here[case[0]] = cases.digest(cases.run_skeleton(ctx, case))
    for case in cases.class_cases():
        if case[0] not in here:
            here[case[0]] = cases.digest(cases.run_classes(ctx, case))
    out = tmp_path / "skeleton.json"
    res = poison_child.run_module("tests.skeleton_cases", out, CHILD_TIMEOUT_S, "the poisoned table")
    there = res["cases"]
    wrong = [k for k, v in there.items() if not v["equal"]]
    assert not wrong, f"{len(wrong)} cases differ from the rule under poison; the first: {wrong[:10]}"
    dirty = [(k, v["dirty"]) for k, v in there.items() if v["dirty"] is not None]
    assert not dirty, f"{len(dirty)} scratch checks came back dirty; the first: {dirty[:5]}"
    poison_child.assert_unmoved(here, {k: v["sha256"] for k, v in there.items()})
