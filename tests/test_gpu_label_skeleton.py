"""Per-cell skeletons on the device: every case of tests/label_skeleton_cases.py byte-equal to the plain numpy rule of
tests/label_skeleton_reference.py, two runs identical, batch planes equal to their single-plane results, the library's own
iteration count, the raw entry point, the operator in a Pipeline, SegmentationMask.cell_skeleton on touching cells, and the
table once more in a child process under AMT_DEBUG_POISON=1 (the thinning keeps six tiles in LDS and five packed planes
in scratch: a result that depends on what their padding held is its most likely defect)."""
import ctypes
import os
import re

import numpy as np
import pytest

import label_skeleton_cases as cases
import label_skeleton_reference as ref
import poison_child
from arcadia_microscopy_tools_amd import _hip, hipops, operations, segment
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
            where = np.argwhere(got[i] != want[i])[0]
            return f"plane {i} ({name}): {int((got[i] != want[i]).sum())} entries differ, the first at {tuple(where)}"
    return None


@pytest.mark.parametrize("case", cases.skeleton_cases(), ids=lambda c: c[0])
def test_skeleton_equals_the_rule(ctx, case):
    want, _ = cases.skeleton_reference(case)
    got = cases.run_skeleton(ctx, case)
    _DIGESTS[case[0]] = cases.digest(got)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert _first_difference(got, want, case[3]) is None


@pytest.mark.parametrize("case", cases.census_cases(), ids=lambda c: c[0])
def test_census_equals_the_count(ctx, case):
    want = cases.census_reference(case)
    got = cases.run_census(ctx, case)
    _DIGESTS[case[0]] = cases.digest(got)
    assert got.dtype == np.int32 and got.shape == want.shape == (len(case[2]), case[1], 7)
    assert _first_difference(got, want, case[3]) is None


def test_two_runs_give_identical_bytes(ctx):
    for case in cases.skeleton_cases():
        if case[0] in ("seam disks", "bar in a frame", "batch of three", f"contents {cases.ROWS + 1} x {cases.TILE_W + 1}"):
            a, b = cases.run_skeleton(ctx, case), cases.run_skeleton(ctx, case)
            assert np.array_equal(a, b), case[0]
    for case in cases.census_cases():
        if "seam disks" in case[0] or f"contents {cases.ROWS + 1} x {cases.TILE_W + 1}" in case[0]:
            a, b = cases.run_census(ctx, case), cases.run_census(ctx, case)
            assert np.array_equal(a, b), case[0]


def test_batch_planes_equal_their_single_plane_results(ctx):
    case = next(c for c in cases.skeleton_cases() if c[0] == "batch of three")
    together = cases.run_skeleton(ctx, case)
    counts = cases.skeleton_reference(case)[1]
    assert counts[0] == 1 and counts[1] < counts[2] and counts[2] == cases.bar_iterations()
    table = hipops.label_census(ctx.asarray(together), 3).numpy()
    for i, name in enumerate(case[3]):
        alone = hipops.label_skeleton(ctx.asarray(case[2][i]))
        assert np.array_equal(together[i], alone.numpy()), name
        assert np.array_equal(table[i], hipops.label_census(alone, 3).numpy()[0]), name


def test_iteration_count_is_the_rules(ctx, capfd):
    """AMT_DEBUG_SKELETONIZE=1: the library's count on the two-label bar equals the reference's, with and without a limit."""
    d = ctx.asarray(cases.bar_framed())
    n = cases.bar_iterations()
    old = os.environ.get("AMT_DEBUG_SKELETONIZE")
    os.environ["AMT_DEBUG_SKELETONIZE"] = "1"
    try:
        for k, want in ((0, n), (n + 1, n), (n, n), (n - 1, n - 1), (3, 3)):
            capfd.readouterr()
            hipops.label_skeleton(d, k)
            line = capfd.readouterr().err
            m = re.search(r"amt label_skeleton: iterations=(\d+) launches=(\d+) syncs=(\d+)", line)
            assert m, line
            assert int(m.group(1)) == want, (k, line)
            if k:
                assert int(m.group(2)) <= -(-2 * k // cases.T), (k, line)
            else:
                assert int(m.group(2)) > 1, line  # deeper than one launch reaches
    finally:
        if old is None:
            del os.environ["AMT_DEBUG_SKELETONIZE"]
        else:
            os.environ["AMT_DEBUG_SKELETONIZE"] = old


def test_out_argument(ctx):
    p = cases.voronoi((cases.ROWS + 1, 129), 9, 3)
    want = ref.skeletonize(p)[0]
    d = ctx.asarray(p)
    o = ctx.empty(p.shape, np.int32)
    assert hipops.label_skeleton(d, out=o) is o
    assert np.array_equal(o.numpy(), want)
    t = ctx.empty((1, 9, 7), np.int32)
    assert hipops.label_census(o, 9, out=t) is t
    assert np.array_equal(t.numpy()[0], ref.census(want, 9))
    odd = ctx.asarray(np.stack([p, p]))[1:]  # a plane at an address that is no multiple of 16: 65 x 129 x 4 bytes in
    assert odd.ptr % 16 != 0 and np.array_equal(hipops.label_skeleton(odd).numpy()[0], want)
    empty = hipops.label_skeleton(ctx.empty((0, 5, 7), np.int32))
    assert empty.shape == (0, 5, 7)
    assert hipops.label_census(ctx.empty((0, 5, 7), np.int32), 4).shape == (0, 4, 7)
    assert hipops.label_census(d, 0).shape == (1, 0, 7)
    assert not hipops.label_census(ctx.empty((2, 0, 7), np.int32), 3).numpy().any()


def test_raw_entry_point(ctx):
    """Ops 8 and 9 through amt_rank_filter itself, nplanes == 0 and max_label == 0, their refusals with a live context."""
    lib = _hip.load_library()
    plane = cases.noise((70, 131), 0.65, 1)
    want = ref.skeletonize(plane)[0]
    d = ctx.asarray(plane)
    o = ctx.empty(plane.shape, np.int32)
    poison = np.full((4, 7), -77, np.int32)
    t = ctx.asarray(poison)
    full = np.ones((3, 3), np.uint8)

    def call(op, mode, dst=o, n=1, fp=full, dtype=_hip.I32, minuend=None):
        fp = np.ascontiguousarray(fp, np.uint8)
        return lib.amt_rank_filter(ctx.handle, d.ptr, dst.ptr, dtype, n, 70, 131, fp.ctypes.data_as(ctypes.c_void_p),
                                   fp.shape[0], fp.shape[1], op, mode, 0.0, minuend)

    assert call(8, 0) == 0
    assert np.array_equal(o.numpy(), want)
    assert call(8, 2) == 0
    assert np.array_equal(o.numpy(), ref.skeletonize(plane, 2)[0])
    assert call(9, 4, dst=t) == 0
    assert np.array_equal(t.numpy(), ref.census(plane, 4))  # any label plane, not only a skeleton
    ctx.copy_from_host_async(t, poison)
    assert call(9, 0, dst=t) == 0 and call(9, 4, dst=t, n=0) == 0 and call(8, 0, n=0) == 0
    assert np.array_equal(t.numpy(), poison)  # nothing was written
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
    for op in (8, 9):
        assert call(op, 1, fp=cross) == -1 and "footprint" in lib.amt_last_error().decode()
        assert call(op, -1) == -1 and "mode" in lib.amt_last_error().decode()
        assert call(op, 1, dtype=_hip.U16) == -1 and "dtype" in lib.amt_last_error().decode()
        assert call(op, 1, minuend=t.ptr) == -1 and "minuend" in lib.amt_last_error().decode()
        assert call(op, 1, dst=d) == -1 and "alias" in lib.amt_last_error().decode()
    assert call(7, 0, dtype=_hip.U16) == -1 and "op must be" in lib.amt_last_error().decode()  # still no op of this call


def test_operator_in_a_pipeline(ctx):
    lab = cases.voronoi((cases.ROWS + 9, 150), 10, 11)
    want = ref.skeletonize(lab)[0]
    assert not np.array_equal(want != 0, ref.binary.skeletonize(lab != 0)[0] != 0)
    for dtype in (np.int64, np.int32, np.uint16, np.uint8):
        got = operations.skeletonize_labels(lab.astype(dtype))
        assert got.dtype == dtype and np.array_equal(got, want.astype(dtype)), dtype
    assert np.array_equal(operations.skeletonize_labels(lab.astype(np.int64), max_iter=2), ref.skeletonize(lab, 2)[0])
    signed = np.where(lab == 3, -4, lab).astype(np.int64)
    assert np.array_equal(operations.skeletonize_labels(signed), np.where(want == 3, -4, want))
    # after expand_labels in a Pipeline: the planes stay on the device, one download at the end
    seeds = np.where(cases.noise(lab.shape, 0.02, 5) != 0, lab, 0).astype(np.uint16)
    grown = operations.expand_labels(seeds, 4)
    pipe = Pipeline([ImageOperation(operations.expand_labels, 4), ImageOperation(operations.skeletonize_labels)])
    assert pipe._device_chain_applies(seeds)
    got = pipe(seeds)
    assert got.dtype == np.uint16 and np.array_equal(got, ref.skeletonize(grown)[0])
    # device input: a DeviceArray stays on the device
    skel = operations.skeletonize_labels(ctx.asarray(lab))
    assert isinstance(skel, DeviceArray) and skel.dtype == np.int32 and np.array_equal(skel.numpy(), want)
    small = operations.skeletonize_labels(ctx.asarray(lab.astype(np.uint8)))
    assert isinstance(small, DeviceArray) and small.dtype == np.uint8 and np.array_equal(small.numpy(), want)
    with pytest.raises(ValueError, match="must be a 2D array"):
        operations.skeletonize_labels(ctx.asarray(np.zeros((2, 8, 8), np.int32)))
    for shape in ((0, 5), (3, 0)):
        e = operations.skeletonize_labels(ctx.empty(shape, np.int32))
        assert isinstance(e, DeviceArray) and e.shape == shape


def _assert_cell_skeleton(got, label_image, num_cells, image=None):
    want, skel = ref.cell_skeleton(label_image, num_cells)
    assert list(got) == segment.skeleton_keys() == list(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == (num_cells,), key
        assert got[key].tobytes() == want[key].tobytes(), key
    if image is not None:
        assert image.dtype == np.int64 and np.array_equal(image, skel)
        assert got["skeleton_pixels"].sum() == np.count_nonzero(image)


def test_cell_skeleton_of_touching_cells(ctx):
    from arcadia_microscopy_tools_amd.masks import SegmentationMask

    field = cases.voronoi((90, 140), 14, 21, holes=0.01).astype(np.int64)
    field[:4] = field[:, :5] = 0
    mask = SegmentationMask(field, remove_edge_cells=False)
    lab = mask.label_image
    assert mask.num_cells >= 10
    got = mask.cell_skeleton()
    _assert_cell_skeleton(got, lab, mask.num_cells, mask.skeleton_image())
    assert got["skeleton_ends"].sum() > 0 and got["skeleton_junction_pixels"].sum() > 0
    assert not np.array_equal(mask.skeleton_image() != 0, ref.binary.skeletonize(lab != 0)[0] != 0)
    grown = mask.expanded(3)
    _assert_cell_skeleton(grown.cell_skeleton(), grown.label_image, grown.num_cells, grown.skeleton_image())
    ring = mask.ring(3)
    _assert_cell_skeleton(ring.cell_skeleton(), ring.label_image, ring.num_cells)


def test_table_under_poison(ctx, tmp_path):
    """The whole table in a fresh child process with scratch and allocations poisoned: every result equals its reference,
    no scratch check comes back dirty, and every digest equals this process's."""
    here = dict(_DIGESTS)
    for case in cases.skeleton_cases():
        if case[0] not in here:
            here[case[0]] = cases.digest(cases.run_skeleton(ctx, case))
    for case in cases.census_cases():
        if case[0] not in here:
            here[case[0]] = cases.digest(cases.run_census(ctx, case))
    out = tmp_path / "label_skeleton.json"
    res = poison_child.run_module("tests.label_skeleton_cases", out, CHILD_TIMEOUT_S, "the poisoned table")
    there = res["cases"]
    wrong = [k for k, v in there.items() if not v["equal"]]
    assert not wrong, f"{len(wrong)} cases differ from the rule under poison; the first: {wrong[:10]}"
    dirty = [(k, v["dirty"]) for k, v in there.items() if v["dirty"] is not None]
    assert not dirty, f"{len(dirty)} scratch checks came back dirty; the first: {dirty[:5]}"
    poison_child.assert_unmoved(here, {k: v["sha256"] for k, v in there.items()})
