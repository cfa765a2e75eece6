"""Relating two label images on the device (AMT_RPX_RELATE, ``hipops.relate_labels``, ``SegmentationMask.relate`` /
``child_counts``, ``metrics``) against tests/relate_reference.py.  Every comparison is bit equality: the four columns
are exact integers, and ``overlap_fraction`` / ``iou`` are the same float64 expression over them on both sides.
The case list (tests/relate_cases.py) runs once more in a child process with the scratch arena poisoned."""
import ctypes
import json

import numpy as np
import pytest

import poison_child
import relate_cases as rc
import relate_reference as rr

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 60

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _shape_run(ctx, shape):
    if shape not in _RESULTS:
        _RESULTS[shape] = rc.run(ctx, [shape])
    return _RESULTS[shape]


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cases_match_the_reference(ctx, shape):
    res = _shape_run(ctx, shape)
    names = set(rc.cases(shape))
    assert {"blobs", "zero_companion", "gaps", "pieces", "dense", "special_values", "column_and_row"} <= names
    if shape == rc.overflow_shape():
        P = rc._partners()
        assert {f"{kind}_{d}_partners" for kind in ("random", "congruent") for d in (P - 1, P, P + 1, 4 * P)} <= names
    # each case alone, as plane 1 of a stack, and the three batch planes
    assert len(res["records"]) == 2 * len(names) + len(rc.BATCH)
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} of {len(res['records'])} results differ from the reference; the first: {bad[:10]}"


def test_the_cases_hold_what_they_are_named_for():
    P = rc._partners()
    shape = rc.overflow_shape()
    for d in (P - 1, P, P + 1, 4 * P):
        for kind in ("random", "congruent"):
            ref = rc.reference(shape, f"{kind}_{d}_partners")
            assert ref[0, 2] == d and ref[0, 3] == shape[0] * shape[1] - shape[1]
    a, b, _ = rc.cases(shape)["congruent_%d_partners" % (P + 1)]
    assert len(np.unique(b % P)) == 1
    ties = rc.reference((7, 5), "ties")
    assert ties[:, 0].tolist() == [3, 7] and ties[:, 2].tolist() == [2, 3] and ties[0, 1] * 2 == ties[0, 3]
    sp = rc.cases((16, 16))["special_values"][1]
    assert {1, rc.BIG, P, 2 * P} <= set(np.unique(sp).tolist())
    lab = rc.cases((70, 131))["column_and_row"][0]
    assert (lab == 2).any(axis=0).sum() > 64 and (lab == 1).any(axis=0).sum() == 1
    gaps = rc.reference((16, 16), "gaps")
    assert (gaps[1::3] == 0).all() and (gaps[-2:] == 0).all() and gaps[:, 3].sum() > 0


@pytest.mark.parametrize("C", [1, 2, 3])
def test_every_companion_equals_its_own_call(ctx, C):
    from arcadia_microscopy_tools_amd import hipops

    shape = (33, 40)
    a, _, k = rc.cases(shape)["blobs"]
    comps = [rc.cases(shape)[n][1] for n in ("blobs", "dense", "special_values")][:C]
    lab = ctx.asarray(np.stack([a, np.flipud(a)]))
    stack = np.stack([np.stack(comps), np.stack([np.fliplr(c) for c in comps])])  # (2, C, Y, X)
    got = hipops.relate_labels(lab, k, ctx.asarray(stack)).numpy()
    assert got.shape == (2, k, C, 4) and got.dtype == np.float64
    for c in range(C):
        one = hipops.relate_labels(lab, k, ctx.asarray(np.ascontiguousarray(stack[:, c]))).numpy()
        assert np.array_equal(got[:, :, c], one[:, :, 0])
        assert np.array_equal(got[0, :, c], rr.relate_columns(a, comps[c], k).astype(np.float64))
        assert np.array_equal(got[1, :, c], rr.relate_columns(np.flipud(a), np.fliplr(comps[c]), k).astype(np.float64))


def test_a_label_image_related_to_itself(ctx):
    from arcadia_microscopy_tools_amd import _hip, hipops

    a, _, k = rc.cases((65, 128))["gaps"]
    lab = ctx.asarray(a)
    got = hipops.relate_labels(lab, k, lab).numpy()[0, :, 0, :]
    area = hipops.regionprops(lab, k).numpy()[0][:, _hip.RP_COLS.index("area")]
    present = area > 0
    assert present.any() and not present.all()
    assert np.array_equal(got[:, 3], area)
    assert np.array_equal(got[:, 1], area)
    assert np.array_equal(got[:, 0], np.where(present, np.arange(1, k + 1), 0).astype(np.float64))
    assert np.array_equal(got[:, 2], present.astype(np.float64))


def test_two_runs_give_identical_bytes(ctx):
    from arcadia_microscopy_tools_amd import hipops

    shape = rc.overflow_shape()
    names = list(rc.cases(shape))
    lab = ctx.asarray(np.stack([rc.cases(shape)[n][0] for n in names]))
    comp = ctx.asarray(np.stack([rc.cases(shape)[n][1] for n in names]))
    first = hipops.relate_labels(lab, 5, comp).numpy().tobytes()
    assert hipops.relate_labels(lab, 5, comp).numpy().tobytes() == first


def _raw(ctx, lab, comp, code, C, bits, table, wtable, n, H, W, k):
    from arcadia_microscopy_tools_amd import _hip

    p = lambda a: None if a is None else a.ptr  # noqa: E731
    return _hip.load_library().amt_regionprops_ext(ctx.handle, lab.ptr, p(comp), code, C, bits, p(table), p(wtable), n, H,
                                                   W, k)


def test_relate_combined_with_euler_number(ctx):
    from arcadia_microscopy_tools_amd import _hip, hipops

    shape = (64, 64)
    a, b, k = rc.cases(shape)["blobs"]
    lab, comp = ctx.asarray(a[None]), ctx.asarray(b[None, None])
    table = ctx.zeros((1, k, _hip.RPX_NCOLS), np.float64)
    wtable = ctx.empty((1, k, 1, 4), np.float64)
    bits = _hip.RPX_RELATE | _hip.RPX_BITS["euler_number"]
    assert _raw(ctx, lab, comp, _hip.I32, 1, bits, table, wtable, 1, 64, 64, k) == 0
    alone, _ = hipops.regionprops_ext(lab, k, ["euler_number"], out=ctx.zeros((1, k, _hip.RPX_NCOLS), np.float64))
    assert np.array_equal(table.numpy(), alone.numpy())
    assert np.array_equal(wtable.numpy(), hipops.relate_labels(lab, k, comp).numpy())
    assert np.array_equal(wtable.numpy()[0, :, 0], rc.reference(shape, "blobs").astype(np.float64))


def test_argument_errors_of_hipops(ctx):
    from arcadia_microscopy_tools_amd import _hip, hipops

    lab = ctx.asarray(np.ones((7, 5), np.int32))
    with pytest.raises(TypeError):
        hipops.relate_labels(lab, 1, ctx.asarray(np.ones((7, 5), np.uint16)))
    with pytest.raises(TypeError):
        hipops.relate_labels(ctx.asarray(np.ones((7, 5), np.uint16)), 1, lab)
    with pytest.raises(ValueError):
        hipops.relate_labels(lab, 1, ctx.asarray(np.ones((5, 7), np.int32)))
    with pytest.raises(ValueError):  # two stacks for one label plane
        hipops.relate_labels(lab, 1, ctx.asarray(np.ones((2, 1, 7, 5), np.int32)))
    with pytest.raises(ValueError):
        hipops.relate_labels(lab, 1, lab, out=ctx.empty((1, 1, 1, 3), np.float64))
    with pytest.raises(ValueError, match="relate_labels"):
        hipops.regionprops_ext(lab, 1, _hip.RPX_RELATE)
    with pytest.raises(ValueError, match="relate_labels"):
        hipops.regionprops_ext(lab, 1, _hip.RPX_RELATE | 1)
    assert hipops.relate_labels(lab, 0, lab).shape == (1, 0, 1, 4)  # max_label == 0 is fine and writes nothing


def test_argument_errors_of_the_c_abi(ctx):
    from arcadia_microscopy_tools_amd import _hip

    lab = ctx.asarray(np.ones((1, 7, 5), np.int32))
    u16 = ctx.asarray(np.ones((1, 1, 7, 5), np.uint16))
    wtable = ctx.empty((1, 1, 1, 4), np.float64)
    table = ctx.empty((1, 1, _hip.RPX_NCOLS), np.float64)
    weighted = _hip.RPX_WEIGHTED
    assert _raw(ctx, lab, lab, _hip.I32, 1, _hip.RPX_RELATE | weighted, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u16, _hip.U16, 1, _hip.RPX_RELATE, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, lab, _hip.I32, 1, weighted, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, None, _hip.I32, 0, 1, table, None, 1, 7, 5, 1) == -1  # AMT_I32 without the bit, no planes
    assert _raw(ctx, lab, None, _hip.I32, 0, _hip.RPX_RELATE, None, None, 1, 7, 5, 1) == -1  # the bit without planes
    assert _raw(ctx, lab, lab, _hip.I32, 1, _hip.RPX_RELATE | (1 << 9), None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, lab, _hip.I32, 1, _hip.RPX_RELATE, None, wtable, 0, 7, 5, 1) == 0  # no plane: nothing to do
    assert _raw(ctx, lab, lab, _hip.I32, 1, _hip.RPX_RELATE, None, wtable, 1, 7, 5, 1) == 0
    assert wtable.numpy().ravel().tolist() == [1.0, 35.0, 1.0, 35.0]


def _masks(shape=(64, 64)):
    from arcadia_microscopy_tools_amd.masks import SegmentationMask

    nuclei = rc.blobs(shape, 77, 9, 5.0).astype(np.int64)
    cells = rc.blobs(shape, 78, 7, 13.0).astype(np.int64)
    return (SegmentationMask(nuclei, remove_edge_cells=False), SegmentationMask(cells, remove_edge_cells=False))


def _assert_relation(got, want):
    assert list(got) == ["parent", "overlap", "partners", "area", "overlap_fraction"]
    for name in got:
        assert got[name].dtype == (np.float64 if name == "overlap_fraction" else np.int64), name
        assert np.array_equal(got[name], want[name]), name


def test_mask_relate_and_child_counts(ctx):
    nuclei, cells = _masks()
    n, c = nuclei.label_image, cells.label_image
    want = rr.relation(n, c, nuclei.num_cells)
    _assert_relation(nuclei.relate(cells), want)
    assert (want["partners"] > 1).any() and (want["parent"] > 0).any()
    # a raw label array: its values are the parents
    raw = (c * 1000003).astype(np.int64)
    _assert_relation(nuclei.relate(raw), rr.relation(n, raw, nuclei.num_cells))
    _assert_relation(cells.relate(n.astype(np.uint16)), rr.relation(c, n, cells.num_cells))
    counts = cells.child_counts(nuclei)
    assert counts.dtype == np.int64 and counts.shape == (cells.num_cells,)
    assert np.array_equal(counts, np.bincount(want["parent"], minlength=cells.num_cells + 1)[1:])
    assert counts.sum() == (want["parent"] > 0).sum() and counts.max() >= 1
    with pytest.raises(ValueError):
        nuclei.relate(np.zeros((5, 5), np.int64))
    with pytest.raises(ValueError):
        nuclei.relate(-c)
    with pytest.raises(ValueError):
        nuclei.relate(c + (2**31 - 1) * (c > 0))
    with pytest.raises(TypeError):
        nuclei.relate(c.astype(np.float64))
    with pytest.raises(TypeError):
        cells.child_counts(n)


def test_expanded_and_ring_masks_relate_to_their_nuclei(ctx):
    nuclei, _ = _masks()
    grown = nuclei.expanded(4)
    rel = grown.relate(nuclei)
    assert np.array_equal(rel["parent"], grown.parent_labels)
    _assert_relation(rel, rr.relation(grown.label_image, nuclei.label_image, grown.num_cells))
    back = nuclei.relate(grown)
    assert np.array_equal(back["overlap"], back["area"]) and (back["overlap_fraction"] == 1.0).all()
    assert np.array_equal(grown.child_counts(nuclei), np.ones(nuclei.num_cells, np.int64))
    ring = nuclei.ring(4)
    _assert_relation(ring.relate(grown), rr.relation(ring.label_image, grown.label_image, ring.num_cells))
    assert np.array_equal(ring.relate(grown)["parent"], ring.parent_labels)
    assert (ring.relate(nuclei)["parent"] == 0).all()


def test_metrics_on_device_masks(ctx):
    from arcadia_microscopy_tools_amd import metrics

    nuclei, cells = _masks()
    grown = nuclei.expanded(1)
    thresholds = (0.5, 0.6, 0.75, 0.9)
    for true, pred in ((nuclei, grown), (nuclei, cells), (cells, cells)):
        t, p = true.label_image, pred.label_image
        host = metrics.average_precision_from_relations(rr.relation(t, p, true.num_cells),
                                                        rr.relation(p, t, pred.num_cells), thresholds)
        want = rr.average_precision_assignment(t, p, thresholds)
        for got in (metrics.average_precision(true, pred, thresholds), metrics.average_precision(t, p, thresholds)):
            for g, h, w in zip(got, host, want):
                assert np.array_equal(g, h) and np.array_equal(g, w)
    ap, tp, fp, fn = metrics.average_precision(nuclei, nuclei.label_image)
    assert ap.tolist() == [1.0, 1.0, 1.0] and tp.tolist() == [nuclei.num_cells] * 3 and not fp.any() and not fn.any()
    ap, tp, fp, fn = metrics.average_precision(nuclei, np.zeros((64, 64), np.int64))
    assert ap.tolist() == [0.0] * 3 and fn.tolist() == [nuclei.num_cells] * 3 and not fp.any()
    with pytest.raises(ValueError, match="0.5"):
        metrics.average_precision(nuclei, cells, thresholds=(0.4,))
    iou = metrics.intersection_over_union(nuclei, grown)
    want = rr.iou_matrix(nuclei.label_image, grown.label_image)
    assert np.array_equal(iou["parent_a"], np.arange(1, nuclei.num_cells + 1))
    assert np.array_equal(iou["iou_a"], want[np.arange(nuclei.num_cells), iou["parent_a"] - 1])
    assert np.array_equal(iou["iou_b"], want[iou["parent_b"] - 1, np.arange(grown.num_cells)])


def test_cases_under_poison(ctx, tmp_path):
    out = tmp_path / "relate.json"
    res = poison_child.run_module("tests.relate_cases", out, CHILD_TIMEOUT_S, "the poisoned relate cases")
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} results differ from the reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for shape in rc.SHAPES:
        here.update({json.dumps(r["key"]): r["sha256"] for r in _shape_run(ctx, shape)["records"]})
    there = {json.dumps(r["key"]): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
