"""hipops.peak_markers (amt_peak_markers: the peak search lists its peaks, one workgroup per plane sorts and labels the
list) against hipops.peak_mask + hipops.label_sparse on the same inputs: both planes, the counts and the first `count`
entries of the kept lists, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _keep(ctx, n, cap):
    return ctx.empty((n, cap), np.int32), ctx.zeros((n,), np.int32)


def _reference(ctx, d2, mask, m, conn, cap):
    """peak_mask + label_sparse with keep lists on fresh buffers: peaks, markers, counts, list counts, lists."""
    from arcadia_microscopy_tools_amd import hipops

    n = d2.shape[0]
    dd2, dm = ctx.asarray(d2), ctx.asarray(mask)
    peaks, markers = ctx.zeros(d2.shape, np.uint8), ctx.zeros(d2.shape, np.int32)
    keep, status = _keep(ctx, n, cap), ctx.zeros((n,), np.int32)
    hipops.peak_mask(dd2, dm, m, out=peaks, keep=keep, status=status)
    hipops.label_sparse(peaks, conn, capacity=cap, out=markers, count=status, keep=keep)
    return peaks.numpy(), markers.numpy(), status.numpy(), keep[1].numpy(), keep[0].numpy()


def _check(got, ref, tag):
    """got / ref = (peaks, markers, counts, list counts, lists) as numpy arrays; planes that overflowed (count -1) are
    compared on their peaks and their count only, and must hold no markers."""
    pk, mk, cnt, kc, kl = got
    rpk, rmk, rcnt, rkc, rkl = ref
    assert np.array_equal(pk, rpk), (tag, "peaks")
    assert np.array_equal(cnt, rcnt), (tag, "count", cnt, rcnt)
    for b in range(pk.shape[0]):
        if rcnt[b] < 0:
            assert not mk[b].any(), (tag, b, "markers of an overflowed plane")
            continue
        assert np.array_equal(mk[b], rmk[b]), (tag, b, "markers")
        assert kc[b] == rkc[b], (tag, b, "keep_count", kc[b], rkc[b])
        assert np.array_equal(kl[b, : kc[b]], rkl[b, : kc[b]]), (tag, b, "keep_list")


def _run(ctx, d2, mask, m, conn, cap, bufs=None):
    """peak_markers on fresh persistent buffers, or on `bufs` = (peaks, markers, count, keep) of an earlier run."""
    from arcadia_microscopy_tools_amd import hipops

    n = d2.shape[0]
    if bufs is None:
        bufs = (ctx.zeros(d2.shape, np.uint8), ctx.zeros(d2.shape, np.int32), ctx.zeros((n,), np.int32), _keep(ctx, n, cap))
    peaks, markers, count, keep = bufs
    hipops.peak_markers(ctx.asarray(d2), ctx.asarray(mask), m, conn, capacity=cap, peaks=peaks, markers=markers,
                        count=count, keep=keep)
    return (peaks.numpy(), markers.numpy(), count.numpy(), keep[1].numpy(), keep[0].numpy()), bufs


def _plateau_planes(H, W, seed):
    """Three hand-made d2 planes: isolated maxima; horizontal / vertical pairs and L-shapes over three rows; diagonal
    pairs of both orientations -- plateaus of equal values, so every pixel of one is a peak.  Some sit in the first and
    last column of a 62-column strip of the search kernel and right next to the cleared frame."""
    rng = np.random.default_rng(seed)
    d2 = np.zeros((3, H, W), np.int32)

    def put(b, y, x, shape, v):
        for dy, dx in shape:
            if 0 <= y + dy < H and 0 <= x + dx < W:
                d2[b, y + dy, x + dx] = v

    shapes = {
        0: [[(0, 0)]],
        1: [[(0, 0), (0, 1)], [(0, 0), (1, 0)], [(0, 0), (1, 0), (2, 0), (2, 1)], [(0, 1), (1, 1), (2, 1), (2, 0)]],
        2: [[(0, 0), (1, 1)], [(0, 1), (1, 0)], [(0, 0), (1, 1), (2, 0)]],
    }
    for b in range(3):
        # a coarse grid with jitter keeps the shapes at least 8 pixels apart, so min_distance 0 / 1 see every one
        for gy in range(0, H - 3, 12):
            for gx in range(0, W - 3, 12):
                if rng.random() < 0.5:
                    continue
                y, x = gy + int(rng.integers(0, 4)), gx + int(rng.integers(0, 4))
                put(b, y, x, shapes[b][int(rng.integers(0, len(shapes[b])))], int(rng.integers(20, 90)))
        # strip edges of the search (62 output columns per wave) and the pixels next to the frame of width m = 0, 1, 5
        for x in (61, 62, 123, 124):
            if x + 1 < W:
                put(b, 30 + b, x, shapes[b][0], 95)
        for k in (0, 1, 2, 5, 6):
            put(b, k, 40 + 2 * k, [(0, 0)], 99)
            put(b, 50, k, [(0, 0)], 99)
            put(b, H - 1 - k, 20 + 2 * k, [(0, 0)], 99)
            put(b, 60, W - 1 - k, [(0, 0)], 99)
    return d2


@pytest.mark.parametrize("shape", [(96, 128), (70, 131)])
@pytest.mark.parametrize("m", [0, 1, 5])
def test_plateaus_and_merging(ctx, shape, m):
    H, W = shape
    d2 = _plateau_planes(H, W, seed=H + m)
    mask = np.ones((3, H, W), np.uint8)
    mask[:, :, W // 2] = 0  # peaks outside the mask are no peaks
    for conn in (1, 2):
        ref = _reference(ctx, d2, mask, m, conn, 4096)
        got, _ = _run(ctx, d2, mask, m, conn, 4096)
        _check(got, ref, (shape, m, conn))
        assert (ref[2] > 0).all()
    # the diagonal pairs of plane 2 merge at connectivity 2 and stay apart at connectivity 1
    c1 = _run(ctx, d2, mask, m, 1, 4096)[0][2]
    c2 = _run(ctx, d2, mask, m, 2, 4096)[0][2]
    assert c2[2] < c1[2] and c2[0] == c1[0]


def test_real_reliefs(ctx):
    """The chain's own setting: edt of two synthetic masks, min_distance 5, connectivity 1."""
    from arcadia_microscopy_tools_amd import hipops, synth
    from arcadia_microscopy_tools_amd.segment import FovSegmenter

    fovs = np.stack([synth.synth_fov(i, size=256) for i in (3, 4)])
    seg = FovSegmenter(2, fovs.shape[1], 256, 256, ctx=ctx, max_cells=256)
    mask = seg.mask_chain(ctx.asarray(fovs))
    d2 = hipops.edt(mask, want_edt=False)[0].numpy()
    mk = mask.numpy()
    cap = hipops.label_sparse_capacity(256, 256)
    ref = _reference(ctx, d2, mk, 5, 1, cap)
    got, _ = _run(ctx, d2, mk, 5, 1, cap)
    _check(got, ref, "reliefs")
    assert (ref[2] > 0).all()
    # without keep lists both planes are cleared whole: garbage in the output arrays must not survive
    pk, mkr, cnt = hipops.peak_markers(ctx.asarray(d2), mask, 5, 1, peaks=ctx.asarray(np.full(d2.shape, 7, np.uint8)),
                                       markers=ctx.asarray(np.full(d2.shape, -3, np.int32)))
    assert np.array_equal(pk.numpy(), ref[0]) and np.array_equal(mkr.numpy(), ref[1])
    assert np.array_equal(cnt.numpy(), ref[2])


def _isolated(H, W, count, seed):
    """One d2 plane with exactly `count` isolated maxima on odd rows and columns, the last row and column included: with
    min_distance 0 no frame is cleared and each of them is a peak."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(1, H, 2), np.arange(1, W, 2), indexing="ij")
    pos = rng.choice(ys.size, size=count, replace=False)
    d2 = np.zeros((1, H, W), np.int32)
    d2[0, ys.ravel()[pos], xs.ravel()[pos]] = rng.integers(1, 1000, count)
    return d2


def test_lds_tier_edge(ctx):
    """Lists of T - 1, T, T + 1 and 3 T peaks (T = the longest list labelled from LDS): both paths of the marker kernel."""
    from arcadia_microscopy_tools_amd import hipops

    T = hipops.PEAK_MARKERS_LDS_TIER
    H, W = 192, 256
    mask = np.ones((1, H, W), np.uint8)
    assert (H // 2) * (W // 2) == 3 * T  # every odd position taken: the longest list of the test
    cap = hipops.label_sparse_capacity(H, W)
    for count in (T - 1, T, T + 1, 3 * T):
        d2 = _isolated(H, W, count, seed=count)
        ref = _reference(ctx, d2, mask, 0, 1, cap)
        assert ref[2][0] == count and ref[3][0] == count
        got, _ = _run(ctx, d2, mask, 0, 1, cap)
        _check(got, ref, count)
    # merging on the slow path: every positive pixel of a plane of equal values is a peak, so 3 T maxima plus random
    # pixels between them make clusters joined along rows, along columns and diagonally
    rng = np.random.default_rng(5)
    d2 = np.where(_isolated(H, W, 3 * T, seed=5) > 0, 50, 0).astype(np.int32)
    extra = rng.random((H, W)) < 0.08
    d2[0][extra] = 50
    counts = []
    for conn in (1, 2):
        ref = _reference(ctx, d2, mask, 0, conn, cap)
        assert ref[3][0] > 3 * T
        got, _ = _run(ctx, d2, mask, 0, conn, cap)
        _check(got, ref, ("merge", conn))
        counts.append(int(got[2][0]))
    assert 0 < counts[1] < counts[0] < int(ref[3][0])


def _random_maxima(rng, H, W, density):
    """Mask and relief of the existing reuse test: isolated random maxima inside a frame of 4."""
    m = np.zeros((1, H, W), np.uint8)
    m[0, 4:-4, 4:-4] = 1
    d2 = np.zeros((1, H, W), np.int32)
    pts = rng.random((1, H, W)) < density
    pts[:, ::2, :] = False
    pts[:, :, ::2] = False
    pts &= m.astype(bool)
    d2[pts] = 50
    return d2, m


def test_overflow_and_recovery(ctx):
    """Persistent buffers with 64-entry lists: the dense run reports -1 and leaves no markers, and every run after it
    equals a fresh one."""
    rng = np.random.default_rng(2)
    H, W, cap = 96, 128, 64
    bufs, seen = None, set()
    for it, density in enumerate((0.002, 0.2, 0.003, 0.0, 0.004)):
        d2, m = _random_maxima(rng, H, W, density)
        ref = _reference(ctx, d2, m, 1, 1, cap)
        got, bufs = _run(ctx, d2, m, 1, 1, cap, bufs)
        _check(got, ref, it)
        fresh, _ = _run(ctx, d2, m, 1, 1, cap)
        for a, b in zip(got[:3], fresh[:3]):
            assert np.array_equal(a, b), it
        seen.add(bool(got[2][0] >= 0))
    assert seen == {True, False}  # the dense run overflowed the 64-entry lists, the others did not


def test_reuse_and_determinism(ctx):
    """Inputs A, B, A through the same persistent buffers equal fresh runs; the same call twice gives identical lists."""
    H, W, cap = 96, 128, 4096
    a = _plateau_planes(H, W, seed=1)
    b = _plateau_planes(H, W, seed=2)
    mask = np.ones((3, H, W), np.uint8)
    bufs = None
    for tag, d2 in (("A", a), ("B", b), ("A again", a)):
        got, bufs = _run(ctx, d2, mask, 1, 2, cap, bufs)
        _check(got, _reference(ctx, d2, mask, 1, 2, cap), tag)
    again, _ = _run(ctx, a, mask, 1, 2, cap, bufs)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]) and np.array_equal(got[2], again[2])
    assert np.array_equal(got[3], again[3])
    for p in range(3):
        assert np.array_equal(got[4][p, : got[3][p]], again[4][p, : again[3][p]]), p
