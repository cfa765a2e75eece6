"""amt_gaussian_otsu_codes with a prefix plane (one Gaussian pass, the upper 32 bits of every float64 sample stored, the
undecided samples recomputed exactly) against its two-pass form and against the separate float64 operators: every output
bit for bit, on planes where nearly every sample decides and on planes where a third or all of them do not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _outputs(ctx, n, shape):
    return dict(codes=ctx.empty((n,) + shape, np.uint16), thr=ctx.empty((n,), np.float64),
                thr_code=ctx.empty((n,), np.float64), minmax=ctx.empty((n, 2), np.float64),
                hist=ctx.empty((n, 256), np.uint32))


def _compare(ctx, d, sigma, mode="nearest", channel=None, tag=""):
    """prefix form == two-pass form on all five outputs; its mask == gaussian -> threshold_otsu -> open/close on float64."""
    from arcadia_microscopy_tools_amd import hipops

    assert hipops.gaussian_otsu_codes_supported(d, sigma, mode=mode, channel=channel), tag
    H, W = d.shape[-2:]
    n = d.shape[0] if channel is not None else int(np.prod(d.shape[:-2]))
    two, one = _outputs(ctx, n, (H, W)), _outputs(ctx, n, (H, W))
    prefix = ctx.empty((n, H, W), np.uint32)
    hipops.gaussian_otsu_codes(d, sigma, two["codes"], two["thr"], two["thr_code"], two["minmax"], two["hist"],
                               mode=mode, channel=channel)
    hipops.gaussian_otsu_codes(d, sigma, one["codes"], one["thr"], one["thr_code"], one["minmax"], one["hist"],
                               mode=mode, channel=channel, prefix=prefix)
    mm = two["minmax"].numpy()
    const = mm[:, 0] == mm[:, 1]
    for k in ("minmax", "hist", "thr", "thr_code", "codes"):
        assert np.array_equal(one[k].numpy(), two[k].numpy()), (tag, k)
    assert int(one["hist"].numpy()[~const].sum()) == int((~const).sum()) * H * W, (tag, "hist total")
    g = hipops.gaussian(d, sigma, mode=mode, channel=channel)
    gn = g.numpy()
    assert np.array_equal(mm, np.stack([gn.min(axis=(1, 2)), gn.max(axis=(1, 2))], axis=1)), (tag, "minmax f64")
    assert np.array_equal((gn.view(np.uint64) >> np.uint64(32)).astype(np.uint32), prefix.numpy()), (tag, "prefix")
    thr = hipops.threshold_otsu(g)
    assert np.array_equal(one["thr"].numpy(), thr.numpy()), (tag, "thr f64")
    fp = hipops.disk(2)
    want = hipops.threshold_open_close(g, thr, fp).numpy()
    got = hipops.threshold_open_close(one["codes"], one["thr_code"], fp).numpy()
    assert np.array_equal(got, want), (tag, "mask")
    return gn, mm


def _undecided_share(plane, sigma=2.0):
    """Share of samples that must take the exact path, from the CPU oracle's Gaussian."""
    from arcadia_microscopy_tools_amd._thresholds import prefix_rule
    from oracle import skops

    v = skops.gaussian(plane, sigma)
    return float(prefix_rule(v, float(v.min()), float(v.max()))[2].mean())


def _adversarial(H, W, seed=5):
    rng = np.random.default_rng(seed)
    one = np.full((H, W), 1000, np.uint16)
    one[H // 3, W // 2] += 1
    return {"noise": rng.integers(0, 65536, (H, W)).astype(np.uint16),
            "grey_level": (1000 + rng.integers(0, 2, (H, W))).astype(np.uint16),
            "one_pixel": one,
            "constant": np.full((H, W), 1000, np.uint16)}


@pytest.mark.parametrize("shape", [(256, 256), (512, 768), (2048, 2048)])
def test_synthetic_fovs(ctx, shape):
    from arcadia_microscopy_tools_amd import synth

    H, W = shape
    planes = np.stack([np.ascontiguousarray(synth.synth_fov(i, size=max(H, W))[1, :H, :W]) for i in (0, 1)])
    _compare(ctx, ctx.asarray(planes), 2.0, tag=str(shape))


def test_strided_channel_view(ctx):
    from arcadia_microscopy_tools_amd import synth

    fovs = np.stack([synth.synth_fov(i, size=512) for i in (2, 3, 4)])
    for ch in (0, 1, 3):
        _compare(ctx, ctx.asarray(fovs), 2.0, channel=ch, tag=f"channel {ch}")


@pytest.mark.parametrize("mode", ["nearest", "reflect", "mirror"])
@pytest.mark.parametrize("sigma,radius", [(0.25, 1), (1.0, 4), (2.0, 8), (3.0, 12)])
def test_modes_and_radii(ctx, mode, sigma, radius):
    from arcadia_microscopy_tools_amd import hipops, synth

    assert (len(hipops.gaussian_weights(sigma)) - 1) // 2 == radius
    H, W = 300, 520  # partial last tile in both directions
    adv = _adversarial(H, W)
    planes = np.stack([np.ascontiguousarray(synth.synth_fov(6, size=520)[1, :H, :]), adv["noise"], adv["grey_level"],
                       adv["one_pixel"], adv["constant"]])
    _compare(ctx, ctx.asarray(planes), sigma, mode=mode, tag=f"{mode} r{radius}")


@pytest.mark.parametrize("size", [512, 2048])
def test_adversarial_planes(ctx, size):
    """Full-range noise (a few hundred undecided samples: the list), a range of one grey level and a single raised pixel
    (a third / all of the samples undecided: the list overflows and the plane is redone), a constant plane -- in ONE
    batch with an ordinary field of view on either side, so that a redone plane must leave its neighbours alone."""
    from arcadia_microscopy_tools_amd import synth

    adv = _adversarial(size, size)
    assert _undecided_share(adv["grey_level"]) > 0.1 and _undecided_share(adv["one_pixel"]) > 0.1
    assert 0.0 < _undecided_share(adv["noise"]) < 8192 / size**2
    fov = synth.synth_fov(7, size=size)[1]
    planes = np.stack([fov, adv["grey_level"], adv["noise"], adv["one_pixel"], adv["constant"], fov[::-1].copy()])
    _, mm = _compare(ctx, ctx.asarray(planes), 2.0, tag=f"adversarial {size}")
    assert mm[4, 0] == mm[4, 1]  # the constant plane stayed constant


def test_maximum_on_border_and_corner(ctx):
    """The plane's maximum is a single pixel on the border / in a corner: the samples next to it sit near the last edges
    and are recomputed through the boundary mapping of rows and columns."""
    H, W = 264, 512
    rng = np.random.default_rng(9)
    for mode in ("nearest", "reflect", "mirror"):
        planes = []
        for y, x in ((0, 200), (H - 1, 31), (100, 0), (77, W - 1), (0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)):
            p = np.full((H, W), 1000, np.uint16)
            p[y, x] = 1001
            planes.append(p)
            q = (2000 + rng.integers(0, 2, (H, W))).astype(np.uint16)
            q[y, x] = 60000
            planes.append(q)
        stack = np.stack(planes)
        assert _undecided_share(stack[0]) > 0.1
        for sigma in (1.0, 2.0):
            _compare(ctx, ctx.asarray(stack), sigma, mode=mode, tag=f"border {mode} {sigma}")


def test_segmenter_default_equals_float64_path(ctx):
    from arcadia_microscopy_tools_amd import synth
    from arcadia_microscopy_tools_amd.segment import FovSegmenter

    for size, ids in ((256, (0, 1, 2)), (512, (3, 4)), (2048, (5,))):
        fovs = np.stack([synth.synth_fov(i, size=size) for i in ids])
        if size == 512:
            fovs[1, 1] = _adversarial(size, size)["grey_level"]  # a redone plane inside the chain
        d = ctx.asarray(fovs)
        a = FovSegmenter(len(ids), 4, size, size, ctx=ctx, max_cells=2048)
        b = FovSegmenter(len(ids), 4, size, size, ctx=ctx, max_cells=2048, prefix_plane=False)
        la, lb = a.run_c3(d).numpy(), b.run_c3(d).numpy()
        assert a.prefix_path and not a.codes_path and not b.prefix_path and not b.codes_path
        assert a._gauss is None and a._bins is None  # neither the float64 plane nor the byte bins were allocated
        assert np.array_equal(a.thr.numpy(), b.thr.numpy()) and np.array_equal(a.gmm.numpy(), b.gmm.numpy())
        assert np.array_equal(a.mask_a.numpy(), b.mask_a.numpy()), size
        assert np.array_equal(la, lb) and np.array_equal(a.ncells.numpy(), b.ncells.numpy()), size
        k = int(a.ncells.numpy().max())
        assert np.array_equal(a.table.numpy()[:, :k], b.table.numpy()[:, :k], equal_nan=True)
        assert np.array_equal(a.itable.numpy()[:, :k], b.itable.numpy()[:, :k], equal_nan=True)
        assert np.array_equal(a.run_c2(d).numpy(), b.run_c2(d).numpy()) and np.array_equal(a.count8.numpy(), b.count8.numpy())
    # a shape the fused path does not take keeps the float64 + bins path
    odd = np.ascontiguousarray(synth.synth_fov(8, size=384)[None, :, :301, :333])
    c = FovSegmenter(1, 4, 301, 333, ctx=ctx, max_cells=256)
    c.run_c3(ctx.asarray(odd))
    assert not c.prefix_path and c._bins is not None


def test_uint16_comparison_of_any_threshold(ctx):
    """amt_threshold_open_close on a raw uint16 plane whose width is a multiple of 64 takes the 16-pixels-per-lane
    comparison, which decides `(double)v > t` on integers: fractional, negative, saturating and NaN thresholds against
    numpy's comparison followed by the oracle's opening and closing; a width off the fast path must agree too."""
    from arcadia_microscopy_tools_amd import hipops
    from oracle import skops

    rng = np.random.default_rng(31)
    fp = hipops.disk(2)
    thresholds = [1000.5, 999.999999, 1000.0, 0.0, 0.25, -0.5, -1e300, 65534.0, 65534.5, 65535.0, 65535.5, 1e300,
                  float("inf"), float("-inf"), float("nan")]
    for H, W in ((96, 128), (70, 520)):
        base = rng.integers(990, 1012, (H, W)).astype(np.uint16)
        base[rng.random((H, W)) < 0.05] = 65535
        base[rng.random((H, W)) < 0.05] = 0
        base[10:40, 20:90] = 65534
        planes = np.stack([base] * len(thresholds))
        thr = np.array(thresholds)
        got = hipops.threshold_open_close(ctx.asarray(planes), ctx.asarray(thr), fp).numpy()
        for k, t in enumerate(thresholds):
            mask = base.astype(np.float64) > t
            want = skops.binary_closing(skops.binary_opening(mask, skops.disk(2)), skops.disk(2))
            assert np.array_equal(got[k].astype(bool), want), (H, W, t)
