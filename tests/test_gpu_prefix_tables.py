"""prefix_codes_kernel classifies the 32-bit prefixes with per-plane integer tables and counts once per trip
(csrc/amt_filters.hip; host model ``_thresholds.prefix_rule_tables``).  Every output of ``gaussian_otsu_codes`` with a
prefix plane -- codes, histogram, threshold, threshold code, min / max -- must equal, exactly, the two-pass form, the CPU
oracle (oracle.skops Gaussian -> np.histogram -> 2 * bin + (v > centre)), the same plane elsewhere in the batch and the
same plane run alone (the tables are per plane).

Shapes: the fused call takes planes with W % 8 == 0, W >= 256 and H > 2 * radius only
(``amt_gaussian_otsu_codes_supported``), so the three sizes are the smallest supported ones with the properties that
matter here: 17 x 256 (4,352 samples: the least height at sigma 2, exactly one 256-column tile, W % 16 == 0, fewer
samples than a block's lanes x 4 x 8), 24 x 272 (6,528 samples, W % 16 != 0, a partial second tile) -- neither can fill
the 8,192-entry list of undecided samples, so their grey-level plane takes the list path -- and 72 x 512 (36,864
samples, more than one block per plane), whose grey-level plane overflows the list and is redone as a whole."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIGMA = 2.0
SHAPES = [(17, 256), (24, 272), (72, 512)]
PFX_CAP = 8192
_ORACLE: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _planes(shape):
    H, W = shape
    rng = np.random.default_rng([H, W, 41])
    yy, xx = np.mgrid[:H, :W]
    blobs = np.zeros(shape)
    for _ in range(max(3, H * W // 1500)):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2.0, 7.0)
        blobs += rng.uniform(0.2, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    blobs = blobs / blobs.max() * 65535.0
    blobs.flat[rng.integers(0, H * W)] = 65535.0
    blobs.flat[rng.integers(0, H * W)] = 0.0
    field = blobs.astype(np.uint16)  # a blob field over the full range
    constant = np.full(shape, 1000, np.uint16)
    grey = (1000 + rng.integers(0, 2, shape)).astype(np.uint16)
    # 16383 / 16384 and 32767 / 32768 regions: the smoothed values cross 0.25 and 0.5, a binade boundary inside [min, max]
    binade = np.where(xx < W // 2, 16383 + ((yy // 5 + xx // 7) % 2), 32767 + ((yy // 4 + xx // 9) % 2)).astype(np.uint16)
    return np.stack([field, constant, grey, binade, field.copy()])


def _oracle(shape):
    """Per plane: (codes, hist, thr, thr_code, minmax, undecided count) from the CPU oracle; computed once per shape."""
    if shape in _ORACLE:
        return _ORACLE[shape]
    from arcadia_microscopy_tools_amd._thresholds import prefix_rule
    from oracle import skops

    planes = _planes(shape)
    out = []
    for p in planes:
        g = skops.gaussian(p, SIGMA)
        lo, hi = float(g.min()), float(g.max())
        if lo == hi:
            out.append((np.zeros(shape, np.uint16), np.zeros(256, np.uint32), lo, 0.0, (lo, hi), 0))
            continue
        hist, edges = np.histogram(g, bins=256)
        assert np.array_equal(edges, np.linspace(lo, hi, 257))
        bins = np.clip(np.searchsorted(edges, g, side="right") - 1, 0, 255)
        centres = (edges[:-1] + edges[1:]) / 2.0
        codes = (2 * bins + (g > centres[bins])).astype(np.uint16)
        thr = float(skops.threshold_otsu(g))
        k = np.flatnonzero(centres == thr)
        assert k.size == 1
        out.append((codes, hist.astype(np.uint32), thr, float(2 * k[0]), (lo, hi), int(prefix_rule(g, lo, hi)[2].sum())))
    _ORACLE[shape] = (planes, out)
    return _ORACLE[shape]


def _run(ctx, planes, prefix):
    from arcadia_microscopy_tools_amd import hipops

    n, H, W = planes.shape
    d = ctx.asarray(planes)
    assert hipops.gaussian_otsu_codes_supported(d, SIGMA)
    o = dict(codes=ctx.empty((n, H, W), np.uint16), thr=ctx.empty((n,), np.float64), thr_code=ctx.empty((n,), np.float64),
             gmm=ctx.empty((n, 2), np.float64), ghist=ctx.empty((n, 256), np.uint32))
    pre = ctx.empty((n, H, W), np.uint32) if prefix else None
    hipops.gaussian_otsu_codes(d, SIGMA, o["codes"], o["thr"], o["thr_code"], o["gmm"], o["ghist"], prefix=pre)
    return {k: v.numpy() for k, v in o.items()}


KEYS = ("codes", "ghist", "thr", "thr_code", "gmm")


@pytest.mark.parametrize("shape", SHAPES)
def test_prefix_form_equals_two_pass_oracle_and_itself(ctx, shape):
    planes, want = _oracle(shape)
    und = [w[5] for w in want]
    print(f"{shape}: undecided samples per plane {und}")
    if shape == SHAPES[-1]:
        assert und[2] > PFX_CAP  # the grey-level plane overflows the list: redone as a whole
    else:
        assert 0 < und[2] <= shape[0] * shape[1] <= PFX_CAP  # cannot overflow: its many undecided samples are listed
    assert und[0] + und[3] <= PFX_CAP and und[1] == 0  # ordinary planes: a handful at most, all listed
    one = _run(ctx, planes, prefix=True)
    two = _run(ctx, planes, prefix=False)
    for k in KEYS:
        assert np.array_equal(one[k], two[k]), (shape, k, "two-pass form")
    for i, (codes, hist, thr, thr_code, mm, _) in enumerate(want):
        assert np.array_equal(one["codes"][i], codes), (shape, i, "codes vs oracle")
        assert np.array_equal(one["ghist"][i], hist), (shape, i, "ghist vs oracle")
        assert one["thr"][i] == thr and one["thr_code"][i] == thr_code, (shape, i, "thr vs oracle")
        assert tuple(one["gmm"][i]) == mm, (shape, i, "gmm vs oracle")
    for k in KEYS:
        assert np.array_equal(one[k][0], one[k][4]), (shape, k, "plane 0 == plane 4")
    for i in range(len(planes)):
        alone = _run(ctx, planes[i:i + 1], prefix=True)
        for k in KEYS:
            assert np.array_equal(alone[k][0], one[k][i]), (shape, i, k, "plane alone")


def test_unsupported_width_keeps_the_float64_path(ctx):
    """W % 8 != 0: the fused call does not take the plane (and says so), the segmenter keeps the float64 + bins path,
    and that path's mask is the oracle's."""
    from arcadia_microscopy_tools_amd import hipops
    from arcadia_microscopy_tools_amd.segment import FovSegmenter
    from oracle import skops

    H, W = 33, 50
    rng = np.random.default_rng(7)
    fov = rng.integers(0, 65536, (1, 4, H, W)).astype(np.uint16)
    fov[0, :, 8:20, 10:30] //= 8
    plane = ctx.asarray(np.ascontiguousarray(fov[:, 1]))
    assert not hipops.gaussian_otsu_codes_supported(plane, SIGMA)
    with pytest.raises(ValueError, match="unsupported shape"):
        hipops.gaussian_otsu_codes(plane, SIGMA, ctx.empty((1, H, W), np.uint16), ctx.empty((1,), np.float64),
                                   ctx.empty((1,), np.float64), ctx.empty((1, 2), np.float64),
                                   ctx.empty((1, 256), np.uint32), prefix=ctx.empty((1, H, W), np.uint32))
    seg = FovSegmenter(1, 4, H, W, ctx=ctx, max_cells=256)
    seg.run_c3(ctx.asarray(fov))
    assert not seg.prefix_path and seg._bins is not None
    g = skops.gaussian(fov[0, seg.dapi_index], SIGMA)
    assert float(seg.thr.numpy()[0]) == float(skops.threshold_otsu(g))
    assert tuple(seg.gmm.numpy()[0]) == (float(g.min()), float(g.max()))
