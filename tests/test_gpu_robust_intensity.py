"""Robust per-cell intensity statistics on the device (AMT_RPX_ROBUST, ``hipops.robust_intensity``,
``SegmentationMask.cell_robust_intensity``) against tests/robust_reference.py.  Every comparison is bit equality
(``tobytes``): uint16 results are exact multiples of 1/4, float64 results repeat numpy's lerp on the selected order
statistics; absent labels give the canonical NaN on both sides.  The case list (tests/robust_cases.py) runs once more in
a child process with the scratch arena poisoned."""
import json

import numpy as np
import pytest

import poison_child
import robust_cases as qc
import robust_reference as qr

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 60

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _shape_run(ctx, shape, kind):
    if (shape, kind) not in _RESULTS:
        _RESULTS[(shape, kind)] = qc.run(ctx, [shape], kinds=(kind,))
    return _RESULTS[(shape, kind)]


@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("shape", qc.SHAPES + [qc.BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cases_match_the_reference(ctx, shape, kind):
    res = _shape_run(ctx, shape, kind)
    names = set(qc.cases(shape, kind))
    if shape == qc.BIG:
        assert names == {"one_label"} and len(res["records"]) == 2
    else:
        assert {"blobs", "gaps", "pieces", "small_counts", "column_and_row", "constants", "channels_2", "channels_3",
                "channels_5"} <= names
        if kind == "u16":
            assert {f"levels_{n}" for n in qc.LEVELS} | {"ranks_one_bin", "ranks_three_bins", "rank_straddle",
                                                         "mad_keys_wide"} <= names
        else:
            assert "float_specials" in names
        # each case alone, as plane 1 of a stack, and the three batch planes
        assert len(res["records"]) == 2 * len(names) + len(qc.BATCH)
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} of {len(res['records'])} results differ from the reference; the first: {bad[:10]}"


@pytest.mark.parametrize("kind", qc.KINDS)
def test_every_channel_equals_its_own_call(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    shape = (33, 40)
    lab, stack, k = qc.cases(shape, kind)["channels_5"]
    labels = ctx.asarray(np.stack([lab, np.flipud(lab)]))
    both = np.stack([stack, stack[::-1, :, ::-1]])  # (2, 5, Y, X): the second plane's channels reversed and mirrored
    got = hipops.robust_intensity(labels, ctx.asarray(np.ascontiguousarray(both)), k).numpy()
    assert got.shape == (2, k, 5, 4) and got.dtype == np.float64
    for c in range(5):
        one = hipops.robust_intensity(labels, ctx.asarray(np.ascontiguousarray(both[:, c:c + 1])), k).numpy()
        assert got[:, :, c].tobytes() == one[:, :, 0].tobytes()
        assert got[0, :, c].tobytes() == qr.robust_columns(lab, both[0, c], k).tobytes()
        assert got[1, :, c].tobytes() == qr.robust_columns(np.flipud(lab), both[1, c], k).tobytes()


@pytest.mark.parametrize("kind", qc.KINDS)
def test_two_runs_give_identical_bytes(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    shape = (70, 131)
    names = [n for n, (_, stack, _) in qc.cases(shape, kind).items() if stack.shape[0] == 1]
    k = max(qc.cases(shape, kind)[n][2] for n in names)
    lab = ctx.asarray(np.stack([qc.cases(shape, kind)[n][0] for n in names]))
    stack = ctx.asarray(np.stack([qc.cases(shape, kind)[n][1] for n in names]))
    first = hipops.robust_intensity(lab, stack, k).numpy().tobytes()
    assert hipops.robust_intensity(lab, stack, k).numpy().tobytes() == first


def _raw(ctx, lab, inten, code, C, bits, table, wtable, n, H, W, k):
    from arcadia_microscopy_tools_amd import _hip

    p = lambda a: None if a is None else a.ptr  # noqa: E731
    return _hip.load_library().amt_regionprops_ext(ctx.handle, lab.ptr, p(inten), code, C, bits, p(table), p(wtable), n, H,
                                                   W, k)


@pytest.mark.parametrize("kind", qc.KINDS)
def test_robust_combined_with_euler_number(ctx, kind):
    from arcadia_microscopy_tools_amd import _hip, hipops

    shape = (64, 64)
    lab, stack, k = qc.cases(shape, kind)["blobs"]
    labels, inten = ctx.asarray(lab[None]), ctx.asarray(stack[None])
    table = ctx.zeros((1, k, _hip.RPX_NCOLS), np.float64)
    wtable = ctx.empty((1, k, 1, 4), np.float64)
    bits = _hip.RPX_ROBUST | _hip.RPX_BITS["euler_number"]
    code = _hip.U16 if kind == "u16" else _hip.F64
    assert _raw(ctx, labels, inten, code, 1, bits, table, wtable, 1, 64, 64, k) == 0
    alone, _ = hipops.regionprops_ext(labels, k, ["euler_number"], out=ctx.zeros((1, k, _hip.RPX_NCOLS), np.float64))
    assert np.array_equal(table.numpy(), alone.numpy())
    assert wtable.numpy().tobytes() == hipops.robust_intensity(labels, inten, k).numpy().tobytes()
    assert wtable.numpy()[0].tobytes() == qc.reference(shape, kind, "blobs").tobytes()


def test_argument_errors_of_the_c_abi(ctx):
    from arcadia_microscopy_tools_amd import _hip

    lab = ctx.asarray(np.ones((1, 7, 5), np.int32))
    u16 = ctx.asarray(np.full((1, 1, 7, 5), 9, np.uint16))
    u8 = ctx.asarray(np.ones((1, 1, 7, 5), np.uint8))
    wtable = ctx.empty((1, 1, 1, 4), np.float64)
    table = ctx.empty((1, 1, _hip.RPX_NCOLS), np.float64)
    Q = _hip.RPX_ROBUST
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q | _hip.RPX_WEIGHTED, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, lab, _hip.I32, 1, Q | _hip.RPX_RELATE, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q | _hip.RPX_RELATE, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, u8, _hip.U8, 1, Q, None, wtable, 1, 7, 5, 1) == -1  # neither AMT_U16 nor AMT_F64
    assert _raw(ctx, lab, lab, _hip.I32, 1, Q, None, wtable, 1, 7, 5, 1) == -1
    assert _raw(ctx, lab, None, _hip.U16, 0, Q, None, None, 1, 7, 5, 1) == -1  # the bit without planes
    assert _raw(ctx, lab, u16, _hip.U16, 0, Q, None, wtable, 1, 7, 5, 1) == -1  # C < 1
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q, None, None, 1, 7, 5, 1) == -1  # no table to write
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q, table, wtable, 1, 7, 5, 1) == -1  # a morphology table without its bits
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q | 1, None, wtable, 1, 7, 5, 1) == -1  # morphology bits without their table
    assert _raw(ctx, lab, u16, _hip.U16, 1, 1, table, wtable, 1, 7, 5, 1) == -1  # planes without a bit that reads them
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q | (1 << 10), None, wtable, 1, 7, 5, 1) == -1  # outside the accepted mask
    # no plane / no label: nothing to do, nothing written
    wtable = ctx.asarray(np.full((1, 1, 1, 4), 5.0))
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q, None, wtable, 0, 7, 5, 1) == 0
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q, None, wtable, 1, 7, 5, 0) == 0
    assert wtable.numpy().ravel().tolist() == [5.0] * 4
    assert _raw(ctx, lab, u16, _hip.U16, 1, Q, None, wtable, 1, 7, 5, 1) == 0
    assert wtable.numpy().ravel().tolist() == [9.0, 9.0, 9.0, 0.0]


def test_argument_errors_of_hipops(ctx):
    from arcadia_microscopy_tools_amd import _hip, hipops

    lab = ctx.asarray(np.ones((7, 5), np.int32))
    img = ctx.asarray(np.ones((1, 7, 5), np.uint16))
    with pytest.raises(TypeError):
        hipops.robust_intensity(lab, ctx.asarray(np.ones((1, 7, 5), np.uint8)), 1)
    with pytest.raises(TypeError):
        hipops.robust_intensity(lab, ctx.asarray(np.ones((1, 7, 5), np.float32)), 1)
    with pytest.raises(TypeError):  # int32 labels only
        hipops.robust_intensity(ctx.asarray(np.ones((7, 5), np.uint16)), img, 1)
    with pytest.raises(ValueError):
        hipops.robust_intensity(lab, ctx.asarray(np.ones((1, 5, 7), np.uint16)), 1)
    with pytest.raises(ValueError):  # no channel axis
        hipops.robust_intensity(lab, ctx.asarray(np.ones((7, 5), np.uint16)), 1)
    with pytest.raises(ValueError):  # two stacks for one label plane
        hipops.robust_intensity(lab, ctx.asarray(np.ones((2, 1, 7, 5), np.uint16)), 1)
    with pytest.raises(ValueError):
        hipops.robust_intensity(lab, img, 1, out=ctx.empty((1, 1, 1, 3), np.float64))
    with pytest.raises(ValueError, match="robust_intensity"):
        hipops.regionprops_ext(lab, 1, _hip.RPX_ROBUST)
    with pytest.raises(ValueError, match="robust_intensity"):
        hipops.regionprops_ext(lab, 1, _hip.RPX_ROBUST | 1)
    assert hipops.robust_intensity(lab, img, 0).shape == (1, 0, 1, 4)  # max_label == 0 is fine and writes nothing
    out = ctx.empty((1, 1, 1, 4), np.float64)
    assert hipops.robust_intensity(lab, img, 1, out=out) is out and out.numpy().ravel().tolist() == [1.0, 1.0, 1.0, 0.0]


def _images(shape, dtype):
    from arcadia_microscopy_tools_amd.channels import DAPI, FITC

    rng = np.random.RandomState(31)
    if dtype == np.uint8:
        make = lambda: rng.randint(0, 256, shape).astype(np.uint8)  # noqa: E731
    elif dtype == np.uint16:
        make = lambda: rng.randint(0, 65536, shape).astype(np.uint16)  # noqa: E731
    else:
        make = lambda: rng.normal(0.0, 50.0, shape)  # noqa: E731
    return {FITC: make(), DAPI: make()}


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float64], ids=lambda d: np.dtype(d).name)
def test_cell_robust_intensity_on_plain_expanded_and_ring_masks(ctx, dtype):
    from arcadia_microscopy_tools_amd.masks import SegmentationMask

    shape = (64, 64)
    nuclei = qc.blobs(shape, 77, 9, 5.0).astype(np.int64)
    images = _images(shape, dtype)
    mask = SegmentationMask(nuclei, images, remove_edge_cells=False)
    for m in (mask, mask.expanded(4), mask.ring(4)):
        got = m.cell_robust_intensity()
        assert list(got) == [f"intensity_{s}_{c}" for c in ("fitc", "dapi") for s in ("q25", "median", "q75", "mad")]
        lab = m.label_image
        assert m.num_cells >= 2
        for channel, img in images.items():
            want = qr.robust_columns(lab, img, m.num_cells)
            for i, stat in enumerate(qr.COLS):
                col = got[f"intensity_{stat}_{channel.name.lower()}"]
                assert col.dtype == np.float64 and col.shape == (m.num_cells,)
                assert col.tobytes() == np.ascontiguousarray(want[:, i]).tobytes(), (stat, channel.name)
    ring = mask.ring(4)
    assert len(ring.parent_labels) == ring.num_cells == len(ring.cell_robust_intensity()["intensity_mad_dapi"])
    with pytest.raises(ValueError, match="intensity images"):
        SegmentationMask(nuclei, remove_edge_cells=False).cell_robust_intensity()
    # cell_properties and its names stay as they were
    assert not [k for k in mask.cell_properties if "median" in k or "q25" in k or "q75" in k or "_mad_" in k]


def test_cases_under_poison(ctx, tmp_path):
    out = tmp_path / "robust.json"
    res = poison_child.run_module("tests.robust_cases", out, CHILD_TIMEOUT_S, "the poisoned robust cases")
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} results differ from the reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for shape in qc.SHAPES + [qc.BIG]:
        for kind in qc.KINDS:
            here.update({json.dumps(r["key"]): r["sha256"] for r in _shape_run(ctx, shape, kind)["records"]})
    there = {json.dumps(r["key"]): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
