"""Grey reconstruction on the device (ops 3 .. 6 of amt_rank_filter, ``hipops.reconstruction`` / ``h_reconstruction`` /
``h_maxima`` / ``h_minima``, ``operations.*``) against tests/reconstruction_reference.py over the case table of
tests/reconstruction_cases.py.  Everything is compared byte for byte: the fixed point is unique, no tolerance applies."""
import ctypes

import numpy as np
import pytest

import poison_child
import reconstruction_cases as rc
import reconstruction_reference as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not rc.same(got, want):
        with np.errstate(invalid="ignore"):
            at = np.argwhere(got != want)
        if len(at) == 0:  # equal values, other bytes: a zero's sign
            at = np.argwhere(np.signbit(got) != np.signbit(want))
        i = tuple(at[0])
        raise AssertionError(f"{what}: {len(at)} pixels differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


_RUNS = [(kind, i, method) for kind in rc.KINDS for i in range(len(rc.cases(kind))) for method in ("dilation", "erosion")]


@pytest.mark.parametrize("kind,i,method", _RUNS,
                         ids=[f"{k}-{rc.cases(k)[i][0]}-{rc.cases(k)[i][1]}-{m}".replace(" ", "_") for k, i, m in _RUNS])
def test_case_equals_the_reference(ctx, kind, i, method):
    from arcadia_microscopy_tools_amd import hipops

    name, fpn, seeds, masks = rc.cases(kind)[i]
    want = rc.expected(kind)[i]
    if method == "erosion":
        seeds, masks, want = rr.dual(seeds), rr.dual(masks), rr.dual(want)
    got = hipops.reconstruction(ctx.asarray(seeds), ctx.asarray(masks), method, rr.FOOTPRINTS[fpn]).numpy()
    _assert_same(got, want, f"{kind} {name} {fpn} {method}")


@pytest.mark.parametrize("kind", list(rc.KINDS))
def test_two_runs_give_identical_bytes(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    for name, fpn, seeds, masks in rc.cases(kind):
        if name not in ("serpentine", "full range", "batch"):
            continue
        s, m = ctx.asarray(seeds), ctx.asarray(masks)
        a = hipops.reconstruction(s, m, "dilation", rr.FOOTPRINTS[fpn]).numpy()
        out = ctx.empty(seeds.shape, seeds.dtype)
        ctx._lib.amt_memset(ctx.handle, out.ptr, 0x5A, out.nbytes)  # whatever `out` held does not matter
        b = hipops.reconstruction(s, m, "dilation", rr.FOOTPRINTS[fpn], out=out).numpy()
        assert rc.same(a, b), (kind, name, fpn)


@pytest.mark.parametrize("kind", list(rc.KINDS))
def test_h_operators_equal_the_reconstruction_of_their_seed(ctx, kind):
    """Ops 5 / 6 against ops 3 / 4 on materialised seeds and against the reference, with saturation at both ends
    (uint16: h = 1, h = 65535, image values below h = 300); the minuend path against a separate subtraction."""
    from arcadia_microscopy_tools_amd import hipops

    img = rc.h_image(kind)
    a = ctx.asarray(img)
    for h in rc.H_CASES[kind]:
        for method in ("dilation", "erosion"):
            seed = rr.h_seed(img, h, method)
            got = hipops.h_reconstruction(a, h, method).numpy()
            via = hipops.reconstruction(ctx.asarray(seed), a, method).numpy()
            _assert_same(got, via, f"{kind} h={h} {method} against op {3 if method == 'dilation' else 4}")
            _assert_same(got, rr.flood(seed[0], img[0], rr.ONES, method)[None], f"{kind} h={h} {method}")
            if h == rc.H_CASES[kind][-1]:
                got4 = hipops.h_reconstruction(a, h, method, rr.CROSS).numpy()
                _assert_same(got4, rr.flood(seed[0], img[0], rr.CROSS, method)[None], f"{kind} h={h} {method} cross")
        r = hipops.h_reconstruction(a, h, "dilation").numpy()
        dome = hipops.h_reconstruction(a, h, "dilation", minuend=a).numpy()
        _assert_same(dome, (img - r).astype(img.dtype), f"{kind} h={h} h-dome")
        other = (img // 2 + 7).astype(img.dtype) if kind == "u16" else img * 0.5 + 7.0
        sub = hipops.h_reconstruction(a, h, "dilation", minuend=ctx.asarray(other)).numpy()
        _assert_same(sub, (other - r).astype(img.dtype), f"{kind} h={h} minuend")  # uint16 wraps, as amt_subtract does


@pytest.mark.parametrize("kind", list(rc.KINDS))
def test_h_maxima_and_minima_follow_the_rule(ctx, kind):
    from arcadia_microscopy_tools_amd import hipops

    img = rc.h_image(kind)
    a = ctx.asarray(img)
    marked = 0
    for h in rc.H_CASES[kind]:
        for fpn, fp in rr.FOOTPRINTS.items():
            if fpn == "cross" and h != rc.H_CASES[kind][-1]:
                continue
            mx = hipops.h_maxima(a, h, fp)
            mn = hipops.h_minima(a, h, fp)
            assert mx.dtype == np.uint8 and mx.is_bool and mn.is_bool
            gx, gn = mx.numpy(dtype=np.uint8), mn.numpy(dtype=np.uint8)
            _assert_same(gx, rr.h_extrema(img[0], h, fp, True)[None], f"{kind} h_maxima h={h} {fpn}")
            _assert_same(gn, rr.h_extrema(img[0], h, fp, False)[None], f"{kind} h_minima h={h} {fpn}")
            marked += int(gx.sum()) + int(gn.sum())
    assert marked > 0


def test_float64_peak_whose_height_rounds_below_h_is_marked(ctx):
    """A peak of height exactly h over a flat floor: a - fl(a - h) rounds below h for these values, so a residue >= h
    test in floating point would miss it; R == seed marks it."""
    from arcadia_microscopy_tools_amd import hipops

    h = 0.1
    peak = next(v for v in (0.3 + 0.1 * k for k in range(200)) if v - (v - h) < h)
    img = np.full((1, 9, 11), peak - 5.0)
    img[0, 4, 5] = peak
    assert peak - (peak - h) < h and (peak - h) > peak - 5.0
    got = hipops.h_maxima(ctx.asarray(img), h).numpy(dtype=np.uint8)
    want = np.zeros((1, 9, 11), np.uint8)
    want[0, 4, 5] = 1
    _assert_same(got, want, "rounded peak")
    _assert_same(rr.h_extrema(img[0], h, rr.ONES, True)[None], want, "the rule itself")
    low = hipops.h_minima(ctx.asarray(-img), h).numpy(dtype=np.uint8)
    _assert_same(low, want, "rounded pit")


def _raw(ctx, op, x, out, fp, mode=1, cval=0.0, minuend=None):
    from arcadia_microscopy_tools_amd import _hip

    n, H, W = x.shape
    return ctx._lib.amt_rank_filter(ctx.handle, x.ptr, out.ptr, _hip.U16 if x.dtype == np.uint16 else _hip.F64, n, H, W,
                                    fp.ctypes.data_as(ctypes.c_void_p), fp.shape[0], fp.shape[1], op, mode, float(cval),
                                    None if minuend is None else minuend.ptr)


def test_filter_ops_are_unchanged_on_one_plane(ctx):
    from scipy import ndimage as ndi

    rng = np.random.default_rng(9)
    for dt in (np.uint16, np.float64):
        x = rng.integers(0, 5000, (1, 37, 45)).astype(dt)
        d = ctx.asarray(x)
        for fp in (rr.ONES, rr.CROSS):
            want = (ndi.grey_erosion(x[0], footprint=fp, mode="reflect"), ndi.grey_dilation(x[0], footprint=fp, mode="reflect"),
                    ndi.median_filter(x[0], footprint=fp, mode="reflect"))
            for op in (0, 1, 2):
                out = ctx.empty(x.shape, dt)
                assert _raw(ctx, op, d, out, fp) == 0
                _assert_same(out.numpy()[0], want[op].astype(dt), f"op {op} {np.dtype(dt)}")
        out = ctx.empty(x.shape, dt)
        assert _raw(ctx, 1, d, out, rr.ONES, minuend=d) == 0  # the minuend keeps its meaning
        assert rc.same(out.numpy()[0], (x[0] - ndi.grey_dilation(x[0], footprint=rr.ONES, mode="reflect")).astype(dt))
        assert _raw(ctx, 7, d, out, rr.ONES) == -1


@pytest.mark.parametrize("method", ["dilation", "erosion"])
def test_seed_beyond_the_mask_names_the_first_plane(ctx, method):
    from arcadia_microscopy_tools_amd import hipops

    th, tw = rc.tile("u16")
    mask = np.full((3, th + 5, tw + 9), 100, np.uint16)
    seed = np.full_like(mask, 50)
    seed[1, th + 2, tw + 3] = 101
    seed[2, 0, 0] = 500
    seed[2, 3, 3] = 500
    if method == "erosion":
        seed, mask = rr.dual(seed), rr.dual(mask)
    word = "less" if method == "dilation" else "greater"
    with pytest.raises(ValueError, match=rf"Intensity of seed image must be {word} than that of the mask image.*plane 1: 1 "):
        hipops.reconstruction(ctx.asarray(seed), ctx.asarray(mask), method)
    # the same planes without the violations go through
    ok = np.where(seed > mask, 50, seed) if method == "dilation" else np.where(seed < mask, 65535 - 50, seed)
    ok = ok.astype(np.uint16)
    got = hipops.reconstruction(ctx.asarray(ok), ctx.asarray(mask), method).numpy()
    assert (got == (50 if method == "dilation" else 65535 - 50)).all()


def test_empty_batch_and_one_buffer_for_seed_and_mask(ctx):
    from arcadia_microscopy_tools_amd import hipops

    e = hipops.reconstruction(ctx.empty((0, 8, 8), np.uint16), ctx.empty((0, 8, 8), np.uint16))
    assert e.shape == (0, 8, 8)
    x = ctx.asarray(rc.h_image("u16"))
    out = ctx.zeros((1, 4, 4), np.uint16)
    from arcadia_microscopy_tools_amd import _hip

    for op, cval, second in ((3, 0.0, x.ptr), (4, 0.0, x.ptr), (5, 2.0, None), (6, 2.0, None)):  # nplanes == 0
        assert ctx._lib.amt_rank_filter(ctx.handle, x.ptr, out.ptr, _hip.U16, 0, 4, 4, rr.ONES.ctypes.data_as(ctypes.c_void_p),
                                        3, 3, op, 0, cval, second) == 0
    assert not out.numpy().any()
    _assert_same(hipops.reconstruction(x, x).numpy(), rc.h_image("u16"), "seed is mask")


def test_operations_on_numpy_and_in_a_pipeline(ctx):
    from arcadia_microscopy_tools_amd import operations
    from arcadia_microscopy_tools_amd.device import DeviceArray
    from arcadia_microscopy_tools_amd.pipeline import ImageOperation, Pipeline

    img = rc.h_image("u16")[0]
    seed = rr.h_seed(img, 300)
    want = rr.flood(seed, img, rr.ONES)
    got = operations.reconstruction(seed, img)
    _assert_same(got, want, "numpy in, numpy out")
    d = operations.reconstruction(ctx.asarray(seed), img)  # a device seed stays on the device; the mask may be numpy
    assert isinstance(d, DeviceArray)
    _assert_same(d.numpy(), want, "device in, device out")
    _assert_same(operations.reconstruction(rr.dual(seed), rr.dual(img), method="erosion", footprint=rr.CROSS),
                 rr.dual(rr.flood(seed, img, rr.CROSS)), "erosion, cross")
    with pytest.raises(ValueError, match="Intensity of seed image must be less"):
        operations.reconstruction(ctx.asarray(img), seed)
    # uint8 travels as uint16 and comes back as uint8; float64 as it is
    s8, m8 = (seed >> 8).astype(np.uint8), (img >> 8).astype(np.uint8)
    g8 = operations.reconstruction(s8, m8)
    _assert_same(g8, rr.flood(s8.astype(np.uint16), m8.astype(np.uint16), rr.ONES).astype(np.uint8), "uint8")
    f = rc.h_image("f64")[0]
    _assert_same(operations.reconstruction(f - 2.0, f), rr.flood(f - 2.0, f, rr.ONES), "float64")
    for fn, maxima in ((operations.h_maxima, True), (operations.h_minima, False)):
        _assert_same(fn(img, 300), rr.h_extrema(img, 300, rr.ONES, maxima), fn.__name__)
        _assert_same(fn(f, 2.0, rr.CROSS), rr.h_extrema(f, 2.0, rr.CROSS, maxima), fn.__name__ + " float64")
        _assert_same(fn(m8, 3), rr.h_extrema(m8.astype(np.uint16), 3, rr.ONES, maxima), fn.__name__ + " uint8")
        dev = fn(ctx.asarray(img), 300)
        assert isinstance(dev, DeviceArray) and dev.dtype == np.uint8 and dev.is_bool
        # in a Pipeline: one upload, the operators chained on the device, one download
        pipe = Pipeline([ImageOperation(operations.reconstruction, img), ImageOperation(fn, 300)])
        _assert_same(np.asarray(pipe(seed)).astype(np.uint8), rr.h_extrema(want, 300, rr.ONES, maxima), "pipeline")
    flat = np.full((6, 7), 9, np.uint16)
    assert not operations.h_maxima(ctx.asarray(flat), 1).numpy().any()  # h above the range: the early exit, on the device


CHILD_TIMEOUT_S = 120


def test_cases_under_poison(ctx, tmp_path):
    """The whole table once more in a process whose scratch arena and allocations are filled with 0xCD: the results keep
    their bits (nothing is read that the call did not write first), and no padding of the scratch buffers is written."""
    res = poison_child.run_module("tests.reconstruction_cases", tmp_path / "reconstruction.json", CHILD_TIMEOUT_S,
                                  "the poisoned reconstruction cases")
    assert res["dirty"] == [], res["dirty"]
    here = rc.run(ctx)
    assert [r["key"] for r in res["records"]] == [r["key"] for r in here["records"]] and len(here["records"]) > 80

    def by_position(run):  # the records are compared pairwise, in order
        return {f"{i} {r['key']}": r["sha256"] for i, r in enumerate(run["records"])}

    poison_child.assert_unmoved(by_position(here), by_position(res))
