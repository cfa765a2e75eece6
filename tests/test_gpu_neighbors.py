"""Cell neighbours on the device (AMT_RPX_NEIGHBORS, AMT_RPX_NEAREST, ``hipops.neighbor_census`` /
``nearest_labels``, ``SegmentationMask.cell_neighbors``) against tests/neighbors_reference.py.  Every comparison is bit
equality (NaN compared as NaN): the census columns and the labels are exact integers, the distances are ``np.sqrt`` of
the same float64 ``d2`` on both sides, and ``percent_touching`` is the same float64 expression over the integer columns.
The case list (tests/neighbors_cases.py) runs once more in a child process with the scratch arena poisoned."""
import json

import numpy as np
import pytest

import neighbors_cases as nc
import neighbors_reference as nr
import poison_child

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 60

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _shape_run(ctx, shape):
    if shape not in _RESULTS:
        _RESULTS[shape] = nc.run(ctx, [shape])
    return _RESULTS[shape]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("shape", nc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cases_match_the_reference(ctx, shape):
    res = _shape_run(ctx, shape)
    names = set(nc.cases(shape))
    assert {"blobs", "voronoi", "gaps", "pieces", "out_of_range_labels", "column_and_row", "full_plane",
            "zero_companion", "special_values"} <= names
    if shape == nc.overflow_shape():
        P = nc._partners()
        assert {f"{kind}_{d}_neighbors" for kind in ("random", "congruent") for d in (P - 1, P, P + 1, 4 * P)} <= names
    if shape == nc.LATTICE_SHAPE:
        assert {"lattice", "one_label", "two_labels"} <= names
    # census and nearest; each case alone, as plane 1 of a stack, and the three batch planes
    assert len(res["records"]) == 2 * (2 * len(names) + len(nc.BATCH))
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} of {len(res['records'])} results differ from the reference; the first: {bad[:10]}"


def test_distances_are_the_square_roots_of_the_reference(ctx):
    from arcadia_microscopy_tools_amd import hipops

    for shape, name in (((64, 64), "blobs"), ((70, 131), "voronoi"), ((33, 40), "pieces"), (nc.LATTICE_SHAPE, "lattice")):
        a, _, k = nc.cases(shape)[name]
        got = hipops.nearest_labels(ctx.asarray(a), k).numpy()
        assert got.shape == (1, k, 1, 4) and got.dtype == np.float64
        who, d2 = nr.nearest_d2(a, k)
        assert np.array_equal(got[0, :, 0, 0::2], who.astype(np.float64)), (shape, name)
        assert _same(got[0, :, 0, 1::2], np.sqrt(d2)), (shape, name)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_every_companion_equals_its_own_call(ctx, C):
    from arcadia_microscopy_tools_amd import hipops

    shape = (33, 40)
    a, _, k = nc.cases(shape)["blobs"]
    comps = [a, nc.cases(shape)["special_values"][1], nc.cases(shape)["voronoi"][0]][:C]
    lab = ctx.asarray(np.stack([a, np.flipud(a)]))
    stack = np.stack([np.stack(comps), np.stack([np.fliplr(c) for c in comps])])  # (2, C, Y, X)
    got = hipops.neighbor_census(lab, k, ctx.asarray(stack)).numpy()
    assert got.shape == (2, k, C, 4) and got.dtype == np.float64
    for c in range(C):
        one = hipops.neighbor_census(lab, k, ctx.asarray(np.ascontiguousarray(stack[:, c]))).numpy()
        assert np.array_equal(got[:, :, c], one[:, :, 0])
        assert np.array_equal(got[0, :, c], nr.census_columns(a, comps[c], k).astype(np.float64))
        assert np.array_equal(got[1, :, c], nr.census_columns(np.flipud(a), np.fliplr(comps[c]), k).astype(np.float64))
    # the labels as their own companion: the same buffer and a copy of it give the same table
    own = hipops.neighbor_census(lab, k).numpy()
    assert np.array_equal(own, hipops.neighbor_census(lab, k, ctx.asarray(np.stack([a, np.flipud(a)]))).numpy())
    assert np.array_equal(own[0, :, 0], nc.reference(shape, "blobs")[0].astype(np.float64))


def test_two_runs_give_identical_bytes(ctx):
    from arcadia_microscopy_tools_amd import hipops

    shape = nc.overflow_shape()
    names = list(nc.cases(shape))
    planes = [nc.cases(shape)[n] for n in names]
    lab = ctx.asarray(np.stack([p[0] for p in planes]))
    comp = ctx.asarray(np.stack([p[0] if p[1] is None else p[1] for p in planes]))
    first = hipops.neighbor_census(lab, 5, comp).numpy().tobytes()
    assert hipops.neighbor_census(lab, 5, comp).numpy().tobytes() == first
    first = hipops.nearest_labels(lab, 12).numpy().tobytes()
    assert hipops.nearest_labels(lab, 12).numpy().tobytes() == first


def _raw(ctx, lab, comp, code, C, bits, table, wtable, n, H, W, k):
    from arcadia_microscopy_tools_amd import _hip

    p = lambda a: None if a is None else a.ptr  # noqa: E731
    return _hip.load_library().amt_regionprops_ext(ctx.handle, lab.ptr, p(comp), code, C, bits, p(table), p(wtable), n, H,
                                                   W, k)


@pytest.mark.parametrize("which", ["neighbors", "nearest"])
def test_combined_with_euler_number(ctx, which):
    from arcadia_microscopy_tools_amd import _hip, hipops

    shape = (64, 64)
    a, _, k = nc.cases(shape)["blobs"]
    lab = ctx.asarray(a[None])
    table = ctx.zeros((1, k, _hip.RPX_NCOLS), np.float64)
    wtable = ctx.empty((1, k, 1, 4), np.float64)
    euler = _hip.RPX_BITS["euler_number"]
    if which == "neighbors":
        assert _raw(ctx, lab, lab, _hip.I32, 1, _hip.RPX_NEIGHBORS | euler, table, wtable, 1, 64, 64, k) == 0
        alone, want = hipops.neighbor_census(lab, k).numpy(), nc.reference(shape, "blobs")[0].astype(np.float64)
    else:
        assert _raw(ctx, lab, None, 0, 1, _hip.RPX_NEAREST | euler, table, wtable, 1, 64, 64, k) == 0
        alone, want = hipops.nearest_labels(lab, k).numpy(), nc.reference(shape, "blobs")[1]
    morph, _ = hipops.regionprops_ext(lab, k, ["euler_number"], out=ctx.zeros((1, k, _hip.RPX_NCOLS), np.float64))
    assert np.array_equal(table.numpy(), morph.numpy())
    assert _same(wtable.numpy(), alone) and _same(wtable.numpy()[0, :, 0], want)


def test_argument_errors_of_hipops(ctx):
    from arcadia_microscopy_tools_amd import _hip, hipops

    lab = ctx.asarray(np.ones((7, 5), np.int32))
    u16 = ctx.asarray(np.ones((7, 5), np.uint16))
    with pytest.raises(TypeError):
        hipops.neighbor_census(lab, 1, u16)
    with pytest.raises(TypeError):
        hipops.neighbor_census(u16, 1, lab)
    with pytest.raises(TypeError):
        hipops.neighbor_census(u16, 1)
    with pytest.raises(TypeError):
        hipops.nearest_labels(u16, 1)
    with pytest.raises(ValueError):
        hipops.neighbor_census(lab, 1, ctx.asarray(np.ones((5, 7), np.int32)))
    with pytest.raises(ValueError):  # two stacks for one label plane
        hipops.neighbor_census(lab, 1, ctx.asarray(np.ones((2, 1, 7, 5), np.int32)))
    with pytest.raises(ValueError):
        hipops.neighbor_census(lab, 1, out=ctx.empty((1, 1, 1, 3), np.float64))
    with pytest.raises(ValueError):
        hipops.nearest_labels(lab, 1, out=ctx.empty((1, 1, 2, 4), np.float64))
    for bits in (_hip.RPX_NEIGHBORS, _hip.RPX_NEAREST, _hip.RPX_NEIGHBORS | 1, _hip.RPX_NEAREST | 1):
        with pytest.raises(ValueError, match="neighbor_census.*nearest_labels"):
            hipops.regionprops_ext(lab, 1, bits)
    assert hipops.neighbor_census(lab, 0).shape == (1, 0, 1, 4)  # max_label == 0 is fine and writes nothing
    assert hipops.nearest_labels(lab, 0).shape == (1, 0, 1, 4)


def test_argument_errors_of_the_c_abi(ctx):
    from arcadia_microscopy_tools_amd import _hip

    lab = ctx.asarray(np.ones((1, 7, 5), np.int32))
    u16 = ctx.asarray(np.ones((1, 1, 7, 5), np.uint16))
    wtable = ctx.asarray(np.full((1, 1, 1, 4), 5.0))
    wtable2 = ctx.empty((1, 1, 2, 4), np.float64)
    N, D = _hip.RPX_NEIGHBORS, _hip.RPX_NEAREST
    assert _raw(ctx, lab, lab, _hip.I32, 1, N | D, None, wtable, 1, 7, 5, 1) == -1  # the two bits together
    assert _raw(ctx, lab, None, 0, 1, N | D, None, wtable, 1, 7, 5, 1) == -1
    for other, code, planes in ((_hip.RPX_RELATE, _hip.I32, lab), (_hip.RPX_ROBUST, _hip.U16, u16),
                                (_hip.RPX_WEIGHTED, _hip.U16, u16)):
        assert _raw(ctx, lab, planes, code, 1, N | other, None, wtable, 1, 7, 5, 1) == -1
        assert _raw(ctx, lab, lab, _hip.I32, 1, N | other, None, wtable, 1, 7, 5, 1) == -1
        assert _raw(ctx, lab, planes, code, 1, D | other, None, wtable, 1, 7, 5, 1) == -1
        assert _raw(ctx, lab, None, 0, 1, D | other, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u16, _hip.U16, 1, N, None, wtable, 1, 7, 5, 1) == -1  # the census takes AMT_I32 planes
    assert _raw(ctx, lab, None, _hip.I32, 1, N, None, wtable, 1, 7, 5, 1) == -1  # ... and does not go without them
    assert _raw(ctx, lab, None, 0, 0, N, None, None, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, lab, _hip.I32, 0, N, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, lab, _hip.I32, 1, N, None, None, 1, 7, 5, 1) == -1  # no table
    assert _raw(ctx, lab, lab, _hip.I32, 1, D, None, wtable, 1, 7, 5, 1) == -1  # nearest with planes
    assert _raw(ctx, lab, lab, 0, 1, D, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, None, _hip.I32, 1, D, None, wtable, 1, 7, 5, 1) == -1  # ... or their element code
    assert _raw(ctx, lab, None, 0, 2, D, None, wtable2, 1, 7, 5, 1) == -1  # C != 1
    assert _raw(ctx, lab, None, 0, 0, D, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, None, 0, 1, D, None, None, 1, 7, 5, 1) == -1  # no table
    assert wtable.numpy().ravel().tolist() == [5.0] * 4  # every refusal stands before the first launch
    assert _raw(ctx, lab, lab, _hip.I32, 1, N, None, wtable, 0, 7, 5, 1) == 0  # no plane: nothing to do
    assert _raw(ctx, lab, None, 0, 1, D, None, wtable, 0, 7, 5, 1) == 0
    assert _raw(ctx, lab, lab, _hip.I32, 1, N, None, wtable, 1, 7, 5, 0) == 0  # no label either
    assert wtable.numpy().ravel().tolist() == [5.0] * 4
    assert _raw(ctx, lab, lab, _hip.I32, 1, N, None, wtable, 1, 7, 5, 1) == 0
    assert wtable.numpy().ravel().tolist() == [0.0] * 4  # one label fills the plane
    assert _raw(ctx, lab, None, 0, 1, D, None, wtable, 1, 7, 5, 1) == 0
    assert np.array_equal(wtable.numpy().ravel(), [0.0, np.nan, 0.0, np.nan], equal_nan=True)


def _masks(shape=(64, 64)):
    from arcadia_microscopy_tools_amd.masks import SegmentationMask

    nuclei = nc.blobs(shape, 77, 9, 5.0).astype(np.int64)
    cells = nc.blobs(shape, 78, 7, 13.0).astype(np.int64)
    return (SegmentationMask(nuclei, remove_edge_cells=False), SegmentationMask(cells, remove_edge_cells=False))


def _assert_neighbors(got, want):
    from arcadia_microscopy_tools_amd import segment

    assert list(got) == segment.neighbor_keys() == list(want)
    for name in got:
        floating = name == "percent_touching" or name.endswith("_distance")
        assert got[name].dtype == (np.float64 if floating else np.int64), name
        assert _same(got[name], want[name]), name
    touching, ring = got["touching_pixels"], got["ring_pixels"]
    with np.errstate(invalid="ignore", divide="ignore"):
        assert _same(got["percent_touching"], 100.0 * touching.astype(np.float64) / ring.astype(np.float64))


CENSUS_KEYS = ("number_of_neighbors", "touching_pixels", "ring_pixels", "percent_touching", "main_neighbor")
CLOSEST_KEYS = ("first_closest_label", "first_closest_distance", "second_closest_label", "second_closest_distance")


def test_mask_cell_neighbors(ctx):
    nuclei, cells = _masks()
    n, c = nuclei.label_image, cells.label_image
    got = cells.cell_neighbors()
    _assert_neighbors(got, nr.cell_neighbors(c, cells.num_cells))
    assert (got["number_of_neighbors"] > 1).any() and (got["percent_touching"] > 0).any()
    alone = nuclei.cell_neighbors()
    _assert_neighbors(alone, nr.cell_neighbors(n, nuclei.num_cells))
    # grown by 4 pixels: the census of the expanded mask, the closest cells of the mask itself
    grown = nuclei.expanded(4)
    near = nuclei.cell_neighbors(distance=4)
    _assert_neighbors(near, nr.cell_neighbors(n, nuclei.num_cells, census_labels=grown.label_image))
    of_grown = grown.cell_neighbors()
    for name in CENSUS_KEYS:
        assert _same(near[name], of_grown[name]), name
    for name in CLOSEST_KEYS:
        assert _same(near[name], alone[name]), name
    assert near["number_of_neighbors"].sum() > alone["number_of_neighbors"].sum()
    # another label image on the rings: a mask and a raw array whose values are used as they are
    _assert_neighbors(nuclei.cell_neighbors(other=cells), nr.cell_neighbors(n, nuclei.num_cells, other=c))
    raw = (c * 1000003).astype(np.int64)
    _assert_neighbors(nuclei.cell_neighbors(other=raw), nr.cell_neighbors(n, nuclei.num_cells, other=raw))
    _assert_neighbors(nuclei.cell_neighbors(distance=2, other=c.astype(np.uint16)),
                      nr.cell_neighbors(n, nuclei.num_cells, census_labels=nuclei.expanded(2).label_image, other=c))
    ring = nuclei.ring(4)
    _assert_neighbors(ring.cell_neighbors(), nr.cell_neighbors(ring.label_image, ring.num_cells))
    _assert_neighbors(ring.cell_neighbors(other=nuclei),
                      nr.cell_neighbors(ring.label_image, ring.num_cells, other=n))
    # a mask whose label plane was made on the device (batch_masks): nothing is downloaded for it
    from arcadia_microscopy_tools_amd.masks import SegmentationMask

    born = SegmentationMask._from_device(ctx.asarray(c.astype(np.int32)), cells.num_cells, None, None)
    _assert_neighbors(born.cell_neighbors(distance=3), cells.cell_neighbors(distance=3))
    assert "mask_image" not in born.__dict__
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            nuclei.cell_neighbors(distance=bad)
    with pytest.raises(ValueError):
        nuclei.cell_neighbors(other=np.zeros((5, 5), np.int64))
    with pytest.raises(ValueError):
        nuclei.cell_neighbors(other=-c)
    with pytest.raises(TypeError):
        nuclei.cell_neighbors(other=c.astype(np.float64))


def test_cases_under_poison(ctx, tmp_path):
    out = tmp_path / "neighbors.json"
    res = poison_child.run_module("tests.neighbors_cases", out, CHILD_TIMEOUT_S, "the poisoned neighbour cases")
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} results differ from the reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for shape in nc.SHAPES:
        here.update({json.dumps(r["key"]): r["sha256"] for r in _shape_run(ctx, shape)["records"]})
    there = {json.dumps(r["key"]): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
