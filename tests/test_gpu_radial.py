"""Per-cell radial distribution on the device (``AMT_RPX_RADIAL``, ``hipops.radial_distribution``,
``SegmentationMask.cell_radial_distribution``) against tests/radial_reference.py over the case table of
tests/radial_cases.py.  The geometry rows -- both radii and the ring counts -- are compared bit for bit, and so are the
three intensity columns of uint16 channels (NaNs in the same places); float64 channels within rtol 1e-9 / atol 1e-12,
the project's bound for float64 per-label sums."""
import json

import numpy as np
import pytest

import poison_child
import radial_cases as rc
import radial_reference as rr

pytestmark = pytest.mark.gpu

SENTINEL = -77.25


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _raw(ctx, lab, inten, code, C, columns, geom, table, n, H, W, k):
    from arcadia_microscopy_tools_amd import _hip

    p = lambda a: None if a is None else a.ptr  # noqa: E731
    return _hip.load_library().amt_regionprops_ext(ctx.handle, p(lab), p(inten), code, C, columns, p(geom), p(table), n, H,
                                                   W, k)


def _code(kind):
    from arcadia_microscopy_tools_amd import _hip

    return _hip.U16 if kind == "u16" else _hip.F64


def _check(kind, name, geom, table, want_geom, want_table):
    assert geom.shape == want_geom.shape, name
    if not rc.same_bits(geom, want_geom):
        at = np.argwhere(~((geom == want_geom) | (np.isnan(geom) & np.isnan(want_geom))))
        raise AssertionError(f"{name} {kind}: geometry differs at {at[:5].tolist()}: got {geom[tuple(at[0])]!r}, "
                             f"want {want_geom[tuple(at[0])]!r}")
    if want_table is None:
        assert table is None, name
        return
    assert table.shape == want_table.shape, name
    same = rc.same_bits(table, want_table) if kind == "u16" else rc.close(table, want_table)
    if not same:
        with np.errstate(invalid="ignore"):
            err = np.nanmax(np.abs(table - want_table))
        raise AssertionError(f"{name} {kind}: columns differ (NaN places equal: "
                             f"{np.array_equal(np.isnan(table), np.isnan(want_table))}, largest difference {err!r})")


# every case with both element types; a case without channels has one
_RUNS = [(name, kind) for name, c in rc.cases().items() for kind in rc.KINDS if c["stack"] is not None or kind == "u16"]


@pytest.mark.parametrize("name,kind", _RUNS, ids=[f"{n}-{k}" for n, k in _RUNS])
def test_case_through_the_c_abi_and_hipops(ctx, name, kind):
    from arcadia_microscopy_tools_amd import _hip, hipops

    c = rc.cases()[name]
    lab, k, bins, stack = c["lab"], c["k"], c["bins"], rc.stack_of(c, kind)
    H, W = lab.shape
    C = 0 if stack is None else stack.shape[0]
    want_geom, want_table = rc.reference(name, kind)
    dlab = ctx.asarray(lab[None])
    dstack = None if stack is None else ctx.asarray(stack[None])
    geom, table = hipops.radial_distribution(dlab, dstack, k, bins=bins)
    assert geom.shape == (1, k, _hip.RAD_GEOM_NCOLS) and (table is None) == (C == 0)
    assert table is None or table.shape == (1, k, C, bins, _hip.RAD_NCOLS)
    _check(kind, name, geom.numpy()[0], None if table is None else table.numpy()[0], want_geom, want_table)
    # the C ABI, into buffers of its own
    g = ctx.asarray(np.full((1, k, _hip.RAD_GEOM_NCOLS), SENTINEL))
    t = None if C == 0 else ctx.asarray(np.full((1, k, C, bins, _hip.RAD_NCOLS), SENTINEL))
    assert _raw(ctx, dlab, dstack, _code(kind) if C else 0, C, _hip.rpx_radial_columns(bins), g, t, 1, H, W, k) == 0
    assert g.numpy().tobytes() == geom.numpy().tobytes()
    assert t is None or t.numpy().tobytes() == table.numpy().tobytes()


@pytest.mark.parametrize("kind", rc.KINDS)
def test_two_planes_with_different_content(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    names = ["random_00", "random_03", "random_06"]  # the same bins and channel count
    cs = [rc.cases()[n] for n in names]
    assert len({(c["bins"], c["stack"].shape, c["k"]) for c in cs}) == 1
    lab = ctx.asarray(np.stack([c["lab"] for c in cs]))
    stack = ctx.asarray(np.stack([rc.stack_of(c, kind) for c in cs]))
    geom, table = hipops.radial_distribution(lab, stack, cs[0]["k"], bins=cs[0]["bins"])
    for i, n in enumerate(names):
        _check(kind, n, geom.numpy()[i], table.numpy()[i], *rc.reference(n, kind))
    # max_label beyond every label: the rows of before, then absent ones
    more, tmore = hipops.radial_distribution(lab, stack, cs[0]["k"] + 3, bins=cs[0]["bins"])
    assert more.numpy()[:, :cs[0]["k"]].tobytes() == geom.numpy().tobytes()
    assert tmore.numpy()[:, :cs[0]["k"]].tobytes() == table.numpy().tobytes()
    assert np.isnan(more.numpy()[:, cs[0]["k"]:, :2]).all() and not more.numpy()[:, cs[0]["k"]:, 2:].any()
    assert np.isnan(tmore.numpy()[:, cs[0]["k"]:]).all()


@pytest.mark.parametrize("kind", rc.KINDS)
def test_two_runs_give_identical_bytes(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    for name in ("random_02", "disk_tier_in", "disk_tier_out", "annulus"):
        c = rc.cases()[name]
        lab, stack = ctx.asarray(c["lab"][None]), ctx.asarray(rc.stack_of(c, kind)[None])
        first = [a.numpy().tobytes() for a in hipops.radial_distribution(lab, stack, c["k"], bins=c["bins"])]
        again = [a.numpy().tobytes() for a in hipops.radial_distribution(lab, stack, c["k"], bins=c["bins"])]
        assert first == again, name


def test_nothing_to_do_writes_nothing(ctx):
    from arcadia_microscopy_tools_amd import _hip, hipops

    c = rc.cases()["one_border"]
    lab, stack = ctx.asarray(c["lab"][None]), ctx.asarray(c["stack"][None])
    H, W = c["lab"].shape
    g = ctx.asarray(np.full((1, 3, _hip.RAD_GEOM_NCOLS), SENTINEL))
    t = ctx.asarray(np.full((1, 3, 3, 4, _hip.RAD_NCOLS), SENTINEL))
    cols = _hip.rpx_radial_columns(4)
    assert _raw(ctx, lab, stack, _hip.U16, 3, cols, g, t, 0, H, W, 3) == 0
    assert _raw(ctx, lab, stack, _hip.U16, 3, cols, g, t, 1, H, W, 0) == 0
    assert _raw(ctx, lab, None, 0, 0, cols, g, None, 0, H, W, 3) == 0
    assert (g.numpy() == SENTINEL).all() and (t.numpy() == SENTINEL).all()
    # refusals leave them alone too: bad bins, another bit, overlapping outputs
    assert _raw(ctx, lab, stack, _hip.U16, 3, _hip.rpx_radial_columns(17), g, t, 1, H, W, 3) == -1
    assert _raw(ctx, lab, stack, _hip.U16, 3, cols | _hip.RPX_ROBUST, g, t, 1, H, W, 3) == -1
    assert _raw(ctx, lab, stack, _hip.U16, 3, cols, t, t, 1, H, W, 3) == -1
    msg = _hip.load_library().amt_last_error()
    assert b"amt_regionprops_ext: " in msg and b"must not alias" in msg
    assert (g.numpy() == SENTINEL).all() and (t.numpy() == SENTINEL).all()
    empty = hipops.radial_distribution(lab, stack, 0)
    assert empty[0].shape == (1, 0, _hip.RAD_GEOM_NCOLS) and empty[1].shape == (1, 0, 3, 4, _hip.RAD_NCOLS)
    # out and geometry_out are filled and returned
    got = hipops.radial_distribution(lab, stack, 3, out=t, geometry_out=g)
    assert got[0] is g and got[1] is t
    _check("u16", "one_border", g.numpy()[0], t.numpy()[0], *rc.reference("one_border"))


def test_geometry_does_not_depend_on_the_channels(ctx):
    from arcadia_microscopy_tools_amd import hipops

    for bins in (1, 4, 16):
        none, three = rc.cases()[f"bins_{bins}_channels_0"], rc.cases()[f"bins_{bins}_channels_3"]
        assert np.array_equal(none["lab"], three["lab"])
        lab = ctx.asarray(none["lab"][None])
        g0, t0 = hipops.radial_distribution(lab, None, none["k"], bins=bins)
        assert t0 is None
        for kind in rc.KINDS:
            g3, _ = hipops.radial_distribution(lab, ctx.asarray(rc.stack_of(three, kind)[None]), three["k"], bins=bins)
            assert g0.numpy().tobytes() == g3.numpy().tobytes(), (bins, kind)


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
        return v * 100.0

    return {FITC: make(), DAPI: make()}


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float64], ids=lambda d: np.dtype(d).name)
def test_cell_radial_distribution_on_plain_expanded_and_ring_masks(ctx, dtype):
    from arcadia_microscopy_tools_amd.channels import DAPI, FITC
    from arcadia_microscopy_tools_amd.masks import SegmentationMask
    from arcadia_microscopy_tools_amd.segment import radial_keys

    shape = (64, 64)
    nuclei = np.zeros(shape, np.int64)
    for i, (cy, cx, r2) in enumerate(((12, 14, 40), (15, 40, 65), (40, 20, 90), (44, 47, 30), (30, 33, 20))):
        nuclei[(rc.disk(shape, cy, cx, r2) == 1) & (nuclei == 0)] = i + 1
    images = _images(shape, dtype)
    stack = np.stack([images[FITC], images[DAPI]])
    kind = "f64" if dtype == np.float64 else "u16"
    mask = SegmentationMask(nuclei, images, remove_edge_cells=False)
    keys_before = list(mask.cell_properties)
    for m in (mask, mask.expanded(3), mask.ring(3)):
        lab, k = np.asarray(m.label_image), m.num_cells
        assert k == 5
        for bins in (4, 3):
            got = m.cell_radial_distribution(bins=bins)
            assert list(got) == radial_keys([FITC, DAPI], bins) and len(got) == 2 + 2 * bins * 3
            assert all(v.dtype == np.float64 and v.shape == (k,) for v in got.values())
            want_geom, want_table = rr.radial_stack(lab, stack if kind == "f64" else stack.astype(np.uint16), k, bins)
            cols = np.stack([got[key] for key in got], axis=1)
            _check(kind, "mask", np.concatenate([cols[:, :2], want_geom[:, 2:]], axis=1), cols[:, 2:].reshape(k, 2, bins, 3),
                   want_geom, want_table)
        # without intensity images: the two radii alone
        alone = SegmentationMask(lab, remove_edge_cells=False).cell_radial_distribution()
        assert list(alone) == ["maximum_radius", "mean_radius"]
        assert alone["maximum_radius"].tobytes() == m.cell_radial_distribution()["maximum_radius"].tobytes()
        assert alone["mean_radius"].tobytes() == want_geom[:, 1].tobytes()
    ring = mask.ring(3)
    assert len(ring.parent_labels) == ring.num_cells == len(ring.cell_radial_distribution()["mean_radius"])
    # cell_properties and its names stay as they were
    assert list(mask.cell_properties) == keys_before and not [key for key in mask.cell_properties if "radi" in key]


CHILD_TIMEOUT_S = 120


def test_cases_under_poison(ctx, tmp_path):
    """The whole table once more in a process whose scratch arena and allocations are filled with 0xCD: the results keep
    their bits, so nothing is read that the call did not write first, and no padding of the scratch planes is written."""
    res = poison_child.run_module("tests.radial_cases", tmp_path / "radial.json", CHILD_TIMEOUT_S, "the poisoned radial cases")
    bad = [r["key"] for r in res["records"] if not r["ok"]]
    assert not bad, f"{len(bad)} results differ from the reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {json.dumps(r["key"]): r["sha256"] for r in rc.run(ctx)["records"]}
    there = {json.dumps(r["key"]): r["sha256"] for r in res["records"]}
    assert set(here) == {json.dumps([n, k]) for n, k in _RUNS}
    poison_child.assert_unmoved(here, there)
