"""Spot detection on the device: every case of tests/spots_cases.py against the plain numpy rules of
tests/spots_reference.py (byte for byte; only the float64 sums of spot_measure within the bound the reference computes per
row), two runs identical, batches equal to their single runs, ``out=``, the raw entry point with its refusals on a live
context, ``operations.peak_local_max`` / ``detect_spots`` on numpy and device input and in a Pipeline, ``mask.spots`` /
``mask.cell_spots`` against the reference composed on the host, the planted-spot fixture, and the table once more in a
child process under AMT_DEBUG_POISON=1."""
import ctypes

import numpy as np
import pytest

import poison_child
import spots_cases as cases
import spots_reference as ref
from arcadia_microscopy_tools_amd import _hip, hipops, operations
from arcadia_microscopy_tools_amd.channels import DAPI, FITC
from arcadia_microscopy_tools_amd.device import DeviceArray
from arcadia_microscopy_tools_amd.masks import SegmentationMask
from arcadia_microscopy_tools_amd.pipeline import ImageOperation, Pipeline

pytestmark = pytest.mark.gpu

# ten times the in-process table's time on the MI355X (profiles/spots.json: "table_in_process_s"), rounded up to a minute
CHILD_TIMEOUT_S = 60

_DIGESTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c["name"])
def test_every_op_equals_the_rule(ctx, case):
    want = cases.reference(case)
    got = cases.run_case(ctx, case)
    assert set(got) == set(want) - {"bound"}
    for key, arr in got.items():
        _DIGESTS[f"{case['name']} / {key}"] = cases.digest(arr)
    assert cases.mismatch(case, got, want) is None


@pytest.mark.parametrize("name", ["maxima ties 70 x 131 r 2 float64", "maxima ties 65 x 129 r 15 uint16", "maxima per-plane thresholds",
                                  "list batch of three", "measure maxima float64 k 15", "measure overfull and holes uint16",
                                  "take int32 labels"])
def test_two_runs_agree_and_a_batch_equals_single_runs(ctx, name):
    c = cases.case(name)
    first = cases.run_case(ctx, c)
    again = cases.run_case(ctx, c)
    for key in first:
        assert first[key].tobytes() == again[key].tobytes(), key
    n = len(c["a"] if "a" in c else c["mask"])
    for i in range(n):
        one = dict(c)
        for key in ("a", "mask", "spots"):
            if key in c:
                one[key] = c[key][i:i + 1]
        if isinstance(c.get("t"), np.ndarray):
            one["t"] = c["t"][i:i + 1]
        for key, arr in cases.run_case(ctx, one).items():
            assert arr.tobytes() == first[key][i:i + 1].tobytes(), (key, i)


def test_out_is_used_and_an_empty_batch_is_empty(ctx):
    c = cases.case("maxima per-plane thresholds")
    a, want = ctx.asarray(c["a"]), cases.reference(c)["mask"]
    o = ctx.empty(c["a"].shape, np.uint8)
    assert hipops.local_maxima(a, c["r"], ctx.asarray(c["t"]), c["b"], out=o) is o and o.is_bool
    assert o.numpy().astype(np.uint8).tobytes() == want.tobytes()
    lst = ctx.empty((3, 601), np.int32)
    assert hipops.mask_list(o, 600, out=lst) is lst
    assert lst.numpy().tobytes() == np.stack([ref.mask_list(m, 600) for m in want]).tobytes()
    table = ctx.empty((3, 600, 7), np.float64)
    assert hipops.spot_measure(a, lst, 2, out=table) is table
    assert table.numpy().tobytes() == np.stack([ref.spot_measure(p, s, 2) for p, s in zip(c["a"], lst.numpy())]).tobytes()
    taken = ctx.empty((3, 600), np.uint16)
    assert hipops.take_at(a, lst, out=taken) is taken
    assert taken.numpy().tobytes() == np.stack([ref.take_at(p, s) for p, s in zip(c["a"], lst.numpy())]).tobytes()
    with pytest.raises(ValueError, match="alias"):
        hipops.local_maxima(a, out=DeviceArray(ctx, a.ptr + a.nbytes - 1, (3, 70, 131), np.uint8))
    none = ctx.empty((0, 5, 7), np.uint16)
    assert hipops.local_maxima(none).shape == (0, 5, 7)
    assert hipops.mask_list(ctx.empty((0, 5, 7), np.uint8), 4).shape == (0, 5)
    assert hipops.spot_measure(none, ctx.empty((0, 5), np.int32)).shape == (0, 4, 7)
    assert hipops.take_at(none, ctx.empty((0, 5), np.int32)).shape == (0, 4)


def test_raw_entry_point(ctx):
    lib = _hip.load_library()
    c = cases.case("maxima ties 70 x 131 r 2 uint16")
    plane = c["a"]
    want = cases.reference(c)["mask"]
    d = ctx.asarray(plane)
    mask = ctx.empty((1, 70, 131), np.uint8)
    cap = 40
    lst = ctx.empty((1, cap + 1), np.int32)
    table = ctx.empty((1, cap, 7), np.float64)
    taken = ctx.empty((1, cap), np.uint16)
    five = np.ones((5, 5), np.uint8)
    room = ctx.zeros((1, 70, 131), np.float64)  # a source that is long enough under every dtype code

    def call(op, src, dst, fp=five, mode=0, cval=0.0, minuend=None, n=1, dtype=_hip.U16):
        fp = np.ascontiguousarray(fp, np.uint8)
        return lib.amt_rank_filter(ctx.handle, src.ptr, dst.ptr, dtype, n, 70, 131, fp.ctypes.data_as(ctypes.c_void_p),
                                   fp.shape[0], fp.shape[1], op, mode, float(cval), None if minuend is None else minuend.ptr)

    def err():
        return lib.amt_last_error().decode()

    assert call(15, d, mask) == 0 and mask.numpy().tobytes() == want.tobytes()
    assert call(16, mask, lst, mode=cap, dtype=_hip.U8) == 0
    wlist = ref.mask_list(want[0], cap)
    assert wlist[0] > cap and lst.numpy()[0].tobytes() == wlist.tobytes()  # truncated: the true count, no -1 tail
    assert call(17, d, table, mode=cap, minuend=lst) == 0
    assert table.numpy()[0].tobytes() == ref.spot_measure(plane[0], wlist, 2).tobytes()
    assert call(18, d, taken, mode=cap, minuend=lst) == 0 and taken.numpy()[0].tobytes() == ref.take_at(plane[0], wlist).tobytes()
    # nplanes == 0 and every refusal write nothing
    poison = {id(b): np.frombuffer(bytes([0x5A]) * b.nbytes, b.dtype).reshape(b.shape).copy() for b in (mask, lst, table, taken)}
    keep = lst.numpy()
    kept_list = ctx.asarray(keep)
    for b in (mask, lst, table, taken):
        ctx.copy_from_host_async(b, poison[id(b)])
    assert call(15, d, mask, n=0) == 0 and call(16, d, lst, mode=cap, dtype=_hip.U8, n=0) == 0
    assert call(17, d, table, mode=cap, minuend=kept_list, n=0) == 0 and call(18, d, taken, mode=cap, minuend=kept_list, n=0) == 0
    for op, dst in ((15, mask), (16, lst), (17, table), (18, taken)):
        m = kept_list if op in (17, 18) else None
        mode = 0 if op == 15 else cap
        good = _hip.U8 if op == 16 else _hip.U16
        assert call(op, room, dst, mode=mode, minuend=m, dtype=_hip.F32) == -1 and "dtype" in err()
        assert call(op, room, dst, mode=-1, minuend=m, dtype=good) == -1 and ("border" in err() or "capacity" in err())
        assert call(op, dst, dst, mode=mode, minuend=m, dtype=good) == -1 and "alias" in err()
        if op != 15:
            assert call(op, room, dst, mode=0, minuend=m, dtype=good) == -1 and "capacity" in err()
            assert call(op, room, dst, mode=mode, minuend=None if m is not None else kept_list, dtype=good) == -1 and "minuend" in err()
        if op in (15, 17):
            for fp in (np.ones((3, 5)), np.ones((33, 33)), np.eye(3), np.ones((2, 2))):
                assert call(op, room, dst, fp=fp, mode=mode, minuend=m, dtype=good) == -1 and "footprint" in err()
    assert call(15, room, mask, fp=np.ones((1, 1))) == -1 and "footprint" in err()
    for b in (mask, lst, table, taken):
        assert b.numpy().tobytes() == poison[id(b)].tobytes()
    # op 7 is still no op of this call, 19 is none either, and the filters are what they were on one plane
    o16 = ctx.empty((1, 70, 131), np.uint16)
    three = np.ones((3, 3), np.uint8)
    for op in (7, 19):
        assert call(op, d, o16, fp=three, mode=1) == -1 and "op must be" in err()
    from scipy import ndimage as ndi

    for op, fn in ((0, ndi.grey_erosion), (1, ndi.grey_dilation), (2, ndi.median_filter)):
        assert call(op, d, o16, fp=three, mode=_hip.MODE_NEAREST) == 0
        assert np.array_equal(o16.numpy()[0], fn(plane[0], footprint=three, mode="nearest")), op


def _same_table(got, want, exact=True):
    assert list(got) == list(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if exact or key in ("row", "col", "y", "x", "response", "label"):
            assert got[key].tobytes() == want[key].tobytes(), key
        else:
            # float64 sums of at most 81 + 88 positive terms in two fixed orders: 2 n 2^-52 relative, and the three
            # derived columns combine two such sums
            np.testing.assert_allclose(got[key], want[key], rtol=8 * 88 * 2.0 ** -52, atol=0)


def test_operations_on_numpy_and_device_input_and_in_a_pipeline(ctx):
    image = cases.blob_plane((70, 131), np.uint16, 70)
    for kw in ({}, {"min_distance": 3, "threshold_abs": 400}, {"threshold_rel": 0.5, "exclude_border": False},
               {"min_distance": 2, "exclude_border": 7, "num_peaks": 5}, {"threshold_abs": 70000}):
        want = ref.peak_local_max(image, **kw)
        got = operations.peak_local_max(image, **kw)
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), kw
        assert np.array_equal(operations.peak_local_max(ctx.asarray(image), **kw), want), kw
    ties = cases.tied_plane((37, 53), np.uint16, 5)
    assert np.array_equal(operations.peak_local_max(ties, 2), ref.peak_local_max(ties, 2))  # raster order among equals
    floats = cases.blob_plane((70, 131), np.float64, 70)
    assert np.array_equal(operations.peak_local_max(floats, 2, threshold_rel=0.2), ref.peak_local_max(floats, 2, threshold_rel=0.2))
    labels = (np.arange(70)[:, None] // 10 * 14 + np.arange(131)[None, :] // 10 + 1).astype(np.int32)
    for kw in ({}, {"sigma": 1.0, "min_distance": 3, "snr": 3.0, "radius": 1}, {"sigma": None, "threshold": 600, "exclude_border": 0},
               {"threshold": 1e-4, "radius": 4, "labels": labels}, {"intensity": (image // 3).astype(np.uint16)}):
        want = ref.detect_spots(image, **kw)
        assert len(want["row"]) > 0
        _same_table(operations.detect_spots(image, **kw), want)
        dev = dict(kw)
        if "intensity" in dev:
            dev["intensity"] = ctx.asarray(dev["intensity"])
        _same_table(operations.detect_spots(ctx.asarray(image), **dev), want)
    want = ref.detect_spots(floats, sigma=None, threshold=0.0, radius=4)
    _same_table(operations.detect_spots(floats, sigma=None, threshold=0.0, radius=4), want, exact=False)
    empty = operations.detect_spots(image, threshold=1e9, labels=labels)
    assert list(empty) == list(operations.SPOT_KEYS) + ["label"] and all(len(v) == 0 for v in empty.values())
    assert operations.peak_local_max(np.zeros((9, 9), np.uint16)).shape == (0, 2)
    with pytest.raises(ValueError, match="shape"):
        operations.detect_spots(image, labels=labels[:-1])
    with pytest.raises(ValueError, match="shape"):
        operations.detect_spots(image, intensity=image[:, :-1])
    pipe = Pipeline([ImageOperation(operations.crop_to_center, (64, 100)), ImageOperation(operations.detect_spots, sigma=1.0)])
    cropped = operations.crop_to_center(image, (64, 100))
    _same_table(pipe(image), ref.detect_spots(np.ascontiguousarray(cropped), sigma=1.0))
    pipe = Pipeline([ImageOperation(operations.crop_to_center, (64, 100)), ImageOperation(operations.peak_local_max, 2)])
    assert np.array_equal(pipe(image), ref.peak_local_max(np.ascontiguousarray(cropped), 2))


def _touching_cells(shape=(70, 131)):
    """a label image of touching rectangles with a background margin"""
    H, W = shape
    lab = np.zeros(shape, np.int64)
    k = 0
    for y in range(4, H - 12, 15):
        for x in range(5, W - 20, 20):
            k += 1
            lab[y:y + 15, x:x + 20] = k
    return lab


def test_mask_spots_and_cell_spots(ctx):
    image = cases.blob_plane((70, 131), np.uint16, 70, n=30)
    other = cases.blob_plane((70, 131), np.uint16, 71)
    lab = _touching_cells()
    mask = SegmentationMask(lab, {DAPI: other, FITC: image}, remove_edge_cells=False)
    kw = {"sigma": 1.0, "snr": 3.0}
    for m in (mask, mask.expanded(3), mask.ring(3)):
        labels = np.asarray(m.label_image)
        want = ref.detect_spots(image, labels=labels, **kw)
        assert (want["label"] > 0).any() and len(want["row"]) > 5
        _same_table(m.spots(FITC, **kw), want)
        cells = m.cell_spots(FITC, **kw)
        wcells = ref.cell_spots(want, m.num_cells, "fitc")
        assert list(cells) == list(wcells)
        for key in wcells:
            assert cells[key].dtype == wcells[key].dtype and cells[key].shape == (m.num_cells,)
            assert cells[key].tobytes() == wcells[key].tobytes(), key
        assert cells["spot_count_fitc"].sum() == int((want["label"] > 0).sum()) > 0
        assert np.isnan(cells["spot_intensity_mean_fitc"][cells["spot_count_fitc"] == 0]).all()
    with pytest.raises(ValueError, match="no intensity image"):
        mask.spots("TRITC")
    with pytest.raises(TypeError, match="labels"):
        mask.spots(FITC, labels=lab)
    # a mask whose label plane was made on the device (batch_masks): nothing is downloaded for it
    born = SegmentationMask._from_device(ctx.asarray(lab.astype(np.int32)), int(lab.max()), None, None,
                                         intensity_image_dict={DAPI: other, FITC: image})
    want = ref.detect_spots(image, labels=lab, **kw)
    _same_table(born.spots(FITC, **kw), want)
    got = born.cell_spots(FITC, **kw)
    for key, w in ref.cell_spots(want, int(lab.max()), "fitc").items():
        assert got[key].tobytes() == w.tobytes(), key
    assert "mask_image" not in born.__dict__


def test_the_planted_spots_are_found(ctx):
    image, truth = cases.planted_plane()
    want = ref.detect_spots(image, **cases.PLANTED_ARGS)
    # the reference alone: exactly the planted spots, each within 0.25 px (measured: 0.087 at most, median 0.044)
    assert len(want["row"]) == 40
    found = np.stack([want["y"], want["x"]], axis=1)
    nearest = np.hypot(*(found[:, None, :] - truth[None, :, :]).transpose(2, 0, 1))
    assert sorted(nearest.argmin(axis=1).tolist()) == list(range(40)) and nearest.min(axis=1).max() <= 0.25
    _same_table(operations.detect_spots(image, **cases.PLANTED_ARGS), want)
    _same_table(operations.detect_spots(ctx.asarray(image), **cases.PLANTED_ARGS), want)


def test_table_under_poison(ctx, tmp_path):
    """The whole table in a fresh child process with scratch and allocations poisoned: every result matches its
    reference, no scratch check comes back dirty, and every digest equals this process's."""
    here = dict(_DIGESTS)
    for c in cases.cases():
        for key, arr in ([] if any(k.startswith(c["name"] + " / ") for k in here) else cases.run_case(ctx, c).items()):
            here[f"{c['name']} / {key}"] = cases.digest(arr)
    out = tmp_path / "spots.json"
    res = poison_child.run_module("tests.spots_cases", out, CHILD_TIMEOUT_S, "the poisoned table")
    there = res["cases"]
    wrong = [k for k, v in there.items() if not v["equal"]]
    assert not wrong, f"{len(wrong)} results differ from the rule under poison; the first: {wrong[:10]}"
    dirty = [(k, v["dirty"]) for k, v in there.items() if v["dirty"] is not None]
    assert not dirty, f"{len(dirty)} scratch checks came back dirty; the first: {dirty[:5]}"
    poison_child.assert_unmoved(here, {k: v["sha256"] for k, v in there.items()})
