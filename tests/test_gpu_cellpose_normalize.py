"""CellposeModel.eval's image normalisation on the network + HIP route (``cellpose_hip.normalize_image``,
``hipops.normalize_planes``, ``segment(..., normalize=, invert=)``) against a numpy restatement of the four steps.

Equality with the restatement is bit for bit and derived, not measured: both sides round the same exact percentile to
float32 and then perform the same correctly rounded float32 operations (a subtraction, a division, a subtraction)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def restate(image, percentile=(1.0, 99.0), lowhigh=None, invert=False):
    """Steps 1-4 of cellpose 4.0.x normalize_img / normalize99 on an ([C], H, W) image (restated; parity unpinned)."""
    a = np.asarray(image)
    a = a[None] if a.ndim == 2 else a
    out = np.empty(a.shape, np.float32)
    for c in range(a.shape[0]):
        x32 = a[c].astype(np.float32)
        if lowhigh is not None:
            lh = np.asarray(lowhigh).astype(np.float32)
            lo, hi = (lh if lh.ndim == 1 else lh[c])
        else:
            lo, hi = (np.percentile(x32.astype(np.float64), p).astype(np.float32) for p in percentile)
        d = np.float32(hi) - np.float32(lo)
        assert d.dtype == np.float32
        if d > np.float32(1e-3):
            y = (x32 - np.float32(lo)) / d
        else:
            y = np.zeros(x32.shape, np.float32)
        if invert:
            y = np.float32(1.0) - y
        assert y.dtype == np.float32
        out[c] = y
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_image(dtype, C, H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    chans = []
    for c in range(C):
        blob = np.exp(-((yy - H * (0.3 + 0.2 * c)) ** 2 + (xx - W * 0.6) ** 2) / (0.05 * H * W + 1))
        if dtype == np.uint16:
            v = np.clip(rng.normal(400 + 300 * c, 40, (H, W)) + blob * (9000 + 20000 * c), 0, 65535).astype(np.uint16)
        elif dtype == np.uint8:
            v = np.clip(rng.normal(20 + 10 * c, 4, (H, W)) + blob * 180, 0, 255).astype(np.uint8)
        elif dtype == np.float32:
            v = (rng.normal(0.0, 1.0, (H, W)) * (3.0 + c) + blob * 50 - 7.5 * c).astype(np.float32)
        else:  # float64 whose samples are not float32 values: rounded once
            v = rng.random((H, W)) * 1e4 / 3.0 + blob * 777.7 + c
        chans.append(v)
    return np.stack(chans) if C > 1 else chans[0]


def run(image, normalize=True, invert=False):
    from arcadia_microscopy_tools_amd import cellpose_hip as ch

    shape = np.shape(image)
    plan = ch.resolve_normalize(normalize, invert, 1 if len(shape) == 2 else shape[0])
    y = ch.normalize_image(image, plan)
    assert y.is_cuda and y.dtype.is_floating_point and y.element_size() == 4 and y.dim() == 3
    return y.cpu().numpy()


OPTIONS = [
    (True, False, {}),
    (True, True, dict(invert=True)),
    ({"percentile": (0.5, 99.9)}, False, dict(percentile=(0.5, 99.9))),
    ({"percentile": (0, 100), "invert": True}, False, dict(percentile=(0.0, 100.0), invert=True)),
    ({"percentile": (25, 60.5)}, True, dict(percentile=(25.0, 60.5), invert=True)),
]


@pytest.mark.parametrize("shape", [(67, 93), (300, 333)])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.float32, np.float64])
def test_tensor_equals_the_restatement_bit_for_bit(dtype, C, shape):
    """67 x 93 and 300 x 333 samples per plane: neither divisible by 8, so later planes start off a 16-byte boundary;
    the larger takes the sampled-bracket percentile path for float images, the smaller the radix select."""
    img = make_image(dtype, C, *shape, seed=11 + C)
    for normalize, invert, kw in OPTIONS:
        got, want = run(img, normalize, invert), restate(img, **kw)
        assert got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), (normalize, invert, int((bits(got) != bits(want)).sum()))
    # lowhigh: one pair for all channels, and one per channel
    pairs = {np.uint16: (350.5, 9000.25), np.uint8: (3, 200), np.float32: (-4.1, 31.7), np.float64: (100.1, 3000.3)}[dtype]
    for inv in (False, True):
        got = run(img, {"lowhigh": pairs, "invert": inv})
        assert np.array_equal(bits(got), bits(restate(img, lowhigh=pairs, invert=inv)))
    per = [(pairs[0] + 0.37 * c, pairs[1] * (1 + 0.5 * c)) for c in range(C)]
    got = run(img, {"lowhigh": per}, True)
    assert np.array_equal(bits(got), bits(restate(img, lowhigh=per, invert=True)))


@pytest.mark.parametrize("dtype,C,normalize,invert,kw", [
    (np.uint16, 3, True, False, {}),
    (np.float32, 1, {"percentile": (2, 98)}, True, dict(percentile=(2.0, 98.0), invert=True)),
    (np.uint16, 2, {"lowhigh": [(300, 20000), (500.5, 41000)]}, False, dict(lowhigh=[(300, 20000), (500.5, 41000)])),
])
def test_tensor_at_2048(dtype, C, normalize, invert, kw):
    img = make_image(dtype, C, 2048, 2048, seed=5)
    got, want = run(img, normalize, invert), restate(img, **kw)
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())


def test_degenerate_and_tied_channels():
    rng = np.random.default_rng(3)
    H, W = 200, 331
    live = rng.normal(100, 10, (H, W)).astype(np.float32)
    const = np.full((H, W), 1234.5, np.float32)
    narrow = (5.0 + rng.random((H, W)) * 4e-4).astype(np.float32)  # 1st and 99th percentile less than 1e-3 apart
    img = np.stack([const, live, narrow])
    p = np.percentile(narrow.astype(np.float64), (1, 99)).astype(np.float32)
    assert 0 < p[1] - p[0] < np.float32(1e-3)
    got = run(img)
    assert np.array_equal(bits(got), bits(restate(img)))
    assert not got[0].any() and not got[2].any() and got[1].any()
    inv = run(img, True, True)
    assert np.array_equal(bits(inv), bits(restate(img, invert=True)))
    assert np.all(inv[0] == 1) and np.all(inv[2] == 1)
    const16 = np.full((2, 64, 70), 777, np.uint16)
    assert not run(const16).any() and np.all(run(const16, {"invert": True}) == 1)
    # 88 % exact zeros: the clipped difference-of-Gaussians output the percentile kernels were hardened for
    for shape, dtype in (((512, 520), np.float32), ((512, 520), np.float64), ((96, 100), np.float32)):
        g = rng.normal(0, 1, shape)
        clipped = np.clip(g - 1.175, 0, None).astype(dtype)
        assert 0.87 < (clipped == 0).mean() < 0.89
        for normalize, invert, kw in OPTIONS:
            got = run(clipped, normalize, invert)
            assert np.array_equal(bits(got), bits(restate(clipped, **kw))), (shape, dtype, normalize)


def test_channels_are_independent():
    a = make_image(np.uint16, 3, 150, 203, seed=8)
    b = a.copy()
    b[1] = np.random.default_rng(1).integers(0, 65535, b[1].shape).astype(np.uint16)
    b[2] = 9
    ya, yb = run(a), run(b)
    assert np.array_equal(bits(ya[0]), bits(yb[0]))
    assert not np.array_equal(bits(ya[1]), bits(yb[1]))
    assert np.array_equal(bits(yb), bits(restate(b)))


def test_normalize_planes_batch_equals_single_and_checks_its_arguments():
    """hipops.normalize_planes: a (B * C, H, W) batch equals B separate calls; every input dtype of the kernel and both
    table dtypes against numpy; shape / dtype / context refusals."""
    from arcadia_microscopy_tools_amd import hipops
    from arcadia_microscopy_tools_amd.device import Context, get_context

    ctx = get_context()
    rng = np.random.default_rng(21)
    B, C, H, W = 3, 2, 61, 45  # 2,745 samples per plane: odd
    for dtype in (np.uint16, np.float32, np.float64):
        if dtype == np.uint16:
            x = rng.integers(0, 65535, (B * C, H, W)).astype(np.uint16)
        else:
            x = (rng.normal(0, 1, (B * C, H, W)) * 1000 / 7).astype(dtype)
        table = np.stack([np.percentile(x[p].astype(np.float32).astype(np.float64), (1, 99)) for p in range(B * C)])
        table[3] = (5.0, 5.0)  # a degenerate plane in the middle of the batch
        for tdtype in (np.float64, np.float32):
            t = table.astype(tdtype)
            dx, dt = ctx.asarray(x), ctx.asarray(t)
            for invert in (False, True):
                whole = hipops.normalize_planes(dx, dt, invert=invert)
                assert whole.dtype == np.float32 and whole.shape == x.shape
                whole = whole.numpy()
                want = np.stack([restate(x[p], lowhigh=t[p].astype(np.float32), invert=invert)[0] for p in range(B * C)])
                assert np.array_equal(bits(whole), bits(want)), (dtype, tdtype, invert)
                for b in range(B):
                    part = hipops.normalize_planes(ctx.asarray(x[b * C:(b + 1) * C]), ctx.asarray(t[b * C:(b + 1) * C]),
                                                   invert=invert).numpy()
                    assert np.array_equal(bits(part), bits(whole[b * C:(b + 1) * C]))
    # out= is filled in place; refusals
    dx, dt = ctx.asarray(x.astype(np.float32)), ctx.asarray(table)
    out = ctx.empty(x.shape, np.float32)
    assert hipops.normalize_planes(dx, dt, out=out) is out
    with pytest.raises(ValueError, match="out has shape"):
        hipops.normalize_planes(dx, dt, out=ctx.empty(x.shape, np.float64))
    with pytest.raises(ValueError, match="pair"):
        hipops.normalize_planes(dx, ctx.asarray(table[:-1]))
    with pytest.raises(TypeError, match="lohi"):
        hipops.normalize_planes(dx, ctx.asarray(table.astype(np.int32)))
    with pytest.raises(TypeError, match="uint16, float32 or float64"):
        hipops.normalize_planes(ctx.asarray(x.astype(np.int32)), dt)
    other = Context(ctx.device)
    try:
        with pytest.raises(ValueError, match="another context"):
            hipops.normalize_planes(dx, dt, out=other.empty(x.shape, np.float32))
        with pytest.raises(ValueError, match="another context"):
            hipops.normalize_planes(dx, other.asarray(table))
    finally:
        other.close()
    # float32 -> float64 on the device is exact (the way of float32 images into the percentile kernels)
    f = (rng.normal(0, 1, (3, 37, 41)) * 1e3).astype(np.float32)
    assert np.array_equal(hipops.to_float64(ctx.asarray(f)).numpy(), f.astype(np.float64))


def _flow_image_and_network(H, W, seed):
    """A uint16 image whose three channels carry a synthetic flow field (dY, dX, cellprob) as counts, and a
    deterministic pointwise fp32 network that turns the NORMALISED image back into flows -- its output depends on its
    input alone, so tiles and resized images map to the matching flows."""
    import torch

    from arcadia_microscopy_tools_amd import synth

    dP, prob, _ = synth.synthetic_flows((H, W), 14, seed=seed, noise=0.3)
    f = np.concatenate([dP, prob[None]])
    img16 = np.clip(np.rint((f + 8.0) * 2500.0 + 1000.0), 0, 65535).astype(np.uint16)  # 2,500 counts per flow unit
    zero, scale = [], []
    for c in range(3):
        lo, hi = (np.float32(np.percentile(img16[c].astype(np.float64), p)) for p in (1, 99))
        zero.append((21000.0 - float(lo)) / float(hi - lo))  # where a flow of 0 lands after normalisation
        scale.append(float(hi - lo) / 2500.0)

    class Pointwise(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("zero", torch.tensor(zero, dtype=torch.float32)[None, :, None, None])
            self.register_buffer("scale", torch.tensor(scale, dtype=torch.float32)[None, :, None, None])

        def forward(self, x):
            return (x.float() - self.zero) * self.scale

    return img16, Pointwise()


def test_segment_with_normalize_equals_segment_of_the_restatement():
    from arcadia_microscopy_tools_amd.model import SegmentationModel

    H, W = 160, 208
    img16, net = _flow_image_and_network(H, W, seed=6)
    model = SegmentationModel(backend="cellpose-hip", network=net, compute_dtype="fp32")
    host = restate(img16)
    for diameter in (30, 60):
        for tiling in (dict(bsize=0), dict(bsize=64, batch_size=5)):
            kw = dict(cell_diameter_px=diameter, num_iterations=100, **tiling)
            got = model.segment(img16, normalize=True, **kw)
            want = model.segment(host, **kw)
            assert got.dtype == np.int64 and got.shape == (H, W) and got.max() >= 5, (diameter, tiling, got.max())
            assert np.array_equal(got, want), (diameter, tiling)
    # the dict form and invert reach the route
    kw = dict(num_iterations=100, bsize=0)
    opts = {"percentile": (2, 97.5), "invert": True}
    assert np.array_equal(model.segment(img16, normalize=opts, **kw),
                          model.segment(restate(img16, percentile=(2.0, 97.5), invert=True), **kw))
    assert np.array_equal(model.segment(img16, normalize={"percentile": (2, 97.5)}, invert=True, **kw),
                          model.segment(img16, normalize=opts, **kw))
    # batch_segment inherits the options
    single = model.segment(img16, normalize=True, **kw)
    batch = model.batch_segment([img16, img16[:, :96, :112]], normalize=True, show_progress=False, **kw)
    assert len(batch) == 2 and np.array_equal(batch[0], single)
    assert np.array_equal(batch[1], model.segment(restate(img16[:, :96, :112]), **kw))
    # the default stays un-normalised: naming normalize=False changes nothing
    assert np.array_equal(model.segment(img16, **kw), model.segment(img16, normalize=False, **kw))
    assert np.array_equal(model.segment(img16, **kw), model.segment(img16.astype(np.float32), **kw))
    # refusals surface as the route's RuntimeError
    with pytest.raises(RuntimeError, match="Cellpose segmentation failed.*tile_norm_blocksize"):
        model.segment(img16, normalize={"tile_norm_blocksize": 100}, **kw)
    with pytest.raises(RuntimeError, match="Cellpose segmentation failed.*invert"):
        model.segment(img16, invert=True, **kw)
    with pytest.raises(RuntimeError, match="Cellpose segmentation failed.*unknown key"):
        model.segment(img16, normalize={"percentiles": (1, 99)}, **kw)
    from arcadia_microscopy_tools_amd.exceptions import SegmentationWarning

    with pytest.warns(SegmentationWarning):
        assert model.batch_segment([img16], normalize={"lowhigh": (5, 5)}, show_progress=False, **kw) == [None]
    with pytest.raises(RuntimeError, match="takes no CellposeModel.eval options"):
        SegmentationModel(backend="classical").segment(img16[0], normalize=True)
