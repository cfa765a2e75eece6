"""One table of small cases that reaches every image operator of libamt_hip.so, and its runner.

A case is an operator call on one input plus the reference for it (oracle/*, scipy, numpy, tests/expand_labels_reference.py,
tests/colocalization_reference.py), compared by the rule of the operator's existing test: bit equality where that test
asserts it, its rtol / atol where it has one.  Every operator runs on every shape of SHAPES unless EXCLUDED says why not;
each shape sits on one side of a switch in the kernels' dispatch (the comments next to SHAPES name them).

Each case runs as
  single  one plane,
  view    plane 1 of a two-plane stack (a base pointer offset by one plane: (70, 131) planes lose their 16-byte
          alignment there),
  batch   three heterogeneous planes in one call -- one like the others, one all-zero / constant, one dense -- whose planes
          must equal, bit for bit, the single-plane results (operators that take ``nplanes`` only).

``run(ctx, families, scratch_check)`` returns one record per case (pass / mismatch with operator, shape and first
differing index, and a sha256 of the output bytes).  A mismatch is recorded and the sweep goes on; an exception from the
library ends it at once.  With ``scratch_check`` the runner asks ``Context.scratch_check()`` after every library call
(AMT_DEBUG_POISON=1: the padding behind every scratch buffer and the arena's tail must still hold the poison).

``python -m tests.operator_sweep --json PATH`` runs everything and writes the records, the scratch findings and the set
of entry points that were called.  Not collected by pytest (tests/test_gpu_operator_sweep.py and
tests/test_host_operator_sweep.py are)."""
from __future__ import annotations

import hashlib
import json
import math
import os
import sys
import time

import numpy as np
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import colocalization_reference as coloc_ref  # noqa: E402
import expand_labels_reference as expand_ref  # noqa: E402
import poison_child  # noqa: E402
from oracle import blending as oblend  # noqa: E402
from oracle import cellpose_dynamics as cd  # noqa: E402
from oracle import contours as ocontours  # noqa: E402
from oracle import regionprops as orp  # noqa: E402
from oracle import skops  # noqa: E402

FAMILIES = ("filters", "stats and thresholds", "binary morphology", "rank filters", "labels",
            "edt, peaks and watershed", "props, colocalisation and outlines", "cellpose", "overlay and plate")

SHAPES = [
    # smaller than every reach; one-row / one-column planes take n == 1 in amt_map_index; no seam jobs in ccl_tileroots,
    # gb.y == 0
    (1, 1), (1, 17), (19, 1), (2, 2), (7, 5),
    # the smallest plane of the uint16 register rank kernels (H, W >= 16) and of the run-table label path (W % 16, n % 16)
    (16, 16),
    # H below and just above 16; W % 8 == 0 with and without W % 16 == 0
    (15, 24), (17, 32), (33, 40),
    # exactly one 64 x 64 label tile, and one row plus one segment more; one and two 64-pixel words of binary
    # morphology; the 32-row bands of toc_fused_kernel
    (64, 64), (65, 128),
    # ragged: the last word holds 3 pixels, plane 1 of a stack is not 16-byte aligned
    (70, 131),
    # the LDS Gaussian (W % 8 == 0 && W >= 256 && H > 2R), the two-pass vertical LDS-DMA pass (W % 64 == 0 && H > 2r), its
    # horizontal pass (W >= 256 + 2r); gaussian_otsu_codes_supported flips across these
    (9, 256), (40, 256), (40, 264), (66, 320),
]
# percentile and histogram cases only: 65,535 / 65,536 samples are the two sides of the sampled-path switch (PQ_MIN_N)
PERCENTILE_SHAPES = [(255, 257), (256, 256)]

SIGMAS = (0.6, 2.0, 3.0, 3.2, 4.0)  # radii 2, 8, 12 (FR_MAX), 13 (the first two-pass radius), 16
MODES = ("nearest", "reflect", "mirror", "constant", "wrap")

# (operator, shape) pairs that do not run, each with its reason
EXCLUDED: dict = {}
_IN_CACHE: dict = {}
_REF_CACHE: dict = {}

_F64, _U16, _I32, _U8, _F32 = np.float64, np.uint16, np.int32, np.uint8, np.float32


# ---------------------------------------------------------------------------------------------------------------------
# inputs: kind 0 = a plane like the others, 1 = all-zero / constant, 2 = dense
# ---------------------------------------------------------------------------------------------------------------------
SEED = 0  # of every input plane; tests/campaigns/fuzz_tiny.py moves it from case to case (set_seed)


def set_seed(seed):
    """Other planes for the same shapes: forgets the inputs and references made so far."""
    global SEED
    SEED = int(seed)
    _IN_CACHE.clear()
    _REF_CACHE.clear()


def _rng(shape, kind, salt=0):
    return np.random.default_rng([shape[0], shape[1], kind, salt, SEED])


def img_u16(shape, kind, salt=0):
    rng = _rng(shape, kind, salt)
    if kind == 1:
        return np.full(shape, 1234, _U16)
    if kind == 2:  # few values, both ends of the range: ties everywhere
        return (rng.integers(0, 4, shape) * 21845).astype(_U16)
    img = rng.integers(0, 65536, shape).astype(_U16)
    if (shape[0] + shape[1]) % 3 == 0:  # smooth content: plateaus
        img = (ndi.uniform_filter(img.astype(_F64), 3) // 257 * 257).astype(_U16)
    return img


def img_f64(shape, kind, salt=0):
    rng = _rng(shape, kind, salt + 100)
    if kind == 1:
        return np.full(shape, 0.25)
    if kind == 2:
        return rng.integers(0, 3, shape).astype(_F64) / 2.0
    return rng.random(shape)


def img(dt, shape, kind, salt=0):
    return img_u16(shape, kind, salt) if dt == "u16" else img_f64(shape, kind, salt)


def mask_of(shape, kind, salt=0):
    rng = _rng(shape, kind, salt + 200)
    H, W = shape
    if kind == 1:
        return np.zeros(shape, bool)
    if kind == 2:
        return rng.random(shape) < 0.93
    m = np.zeros(shape, bool)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(int(rng.integers(1, 6))):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, min(H, W) // 2 + 1))
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    m |= rng.random(shape) < min(0.12, 40.0 / (H * W))  # a few specks (one-pixel components), not thousands of them
    return m


def labels_of(shape, kind, salt=0):
    """int32 labels 1..k, each one 8-connected component."""
    return skops.label(mask_of(shape, kind, salt), 2).astype(_I32)


def values_of(shape, kind, salt=0):
    """int32 label VALUES (touching regions of different values, labels in several pieces, gaps in the numbering)."""
    rng = _rng(shape, kind, salt + 300)
    if kind == 1:
        return np.zeros(shape, _I32)
    v = rng.integers(0, 6, shape) * 3
    if kind == 0:
        v = v * (rng.random(shape) < 0.7)
    return v.astype(_I32)


# ---------------------------------------------------------------------------------------------------------------------
# comparison rules
# ---------------------------------------------------------------------------------------------------------------------
def exact(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False, ("shape", got.shape, want.shape)
    if got.dtype.kind == "f" or want.dtype.kind == "f":
        bad = ~((got == want) | (np.isnan(got.astype(_F64)) & np.isnan(want.astype(_F64))))
    else:
        bad = got != want
    if bad.any():
        return False, tuple(int(i) for i in np.argwhere(bad)[0])
    return True, None


def same_bits(got, want):
    """Equality of the values' bits: what the float32 normalisation tests assert."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False, ("shape / dtype", got.shape, str(got.dtype))
    return exact(got.view(np.uint8), want.view(np.uint8))


def close(rtol, atol):
    def rule(got, want):
        got, want = np.asarray(got, _F64), np.asarray(want, _F64)
        if got.shape != want.shape:
            return False, ("shape", got.shape, want.shape)
        bad = ~np.isclose(got, want, rtol=rtol, atol=atol, equal_nan=True)
        if bad.any():
            return False, tuple(int(i) for i in np.argwhere(bad)[0])
        return True, None
    return rule


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
class Op:
    """make(shape, kind, p) -> tuple of host arrays of ONE plane; dev(ctx, D, Hs, p) -> tuple of numpy arrays with the
    planes on axis 0 (D: the device arrays, Hs: the host arrays, both with the planes stacked on axis 0);
    ref(ins, p) -> the same tuple for one plane; rules: one rule, or one per output."""

    def __init__(self, name, family, make, dev, ref, rules=exact, params=(None,), planes=True, inkey=None, extra_shapes=(),
                 rules_for=None):
        self.name, self.family, self.make, self.dev, self.ref = name, family, make, dev, ref
        self.params, self.planes = tuple(params), planes
        self.rules_for = rules_for or (lambda p: rules)  # rules_for(p): the rule(s) of one parameter set
        self.inkey = inkey or (lambda p: None)
        self.extra_shapes = tuple(extra_shapes)
        assert family in FAMILIES, family

    def shapes(self):
        return [s for s in SHAPES + list(self.extra_shapes) if (self.name, s) not in EXCLUDED]


OPS: list[Op] = []


def add(*a, **kw):
    OPS.append(Op(*a, **kw))


def _hipops():
    from arcadia_microscopy_tools_amd import hipops

    return hipops


def _np(*arrays):
    return tuple(a.numpy() if hasattr(a, "numpy") else np.asarray(a) for a in arrays)


def _ragged(items):
    """Per-plane results of different sizes (tables of each plane's own labels, lists) as one object array."""
    out = np.empty((len(items),), object)
    for i, it in enumerate(items):
        out[i] = it
    return out


def _per_plane(D, fn):
    """An operator of ONE 2-D plane over the planes of the stack: the outputs stacked on axis 0."""
    outs = [fn(*[d[i] for d in D]) for i in range(D[0].shape[0])]
    return tuple(np.stack([np.asarray(o[k]) for o in outs]) for k in range(len(outs[0])))


# ---- filters ----------------------------------------------------------------------------------------------------------
def _gauss_ref(ins, p):
    dt, sigma, mode = p
    x = skops.img_as_float(ins[0]) if dt == "u16" else ins[0]
    return (ndi.gaussian_filter(x, sigma, mode=mode, cval=0.25),)


add("gaussian", "filters",
    lambda s, k, p: (img(p[0], s, k),),
    lambda ctx, D, Hs, p: _np(_hipops().gaussian(D[0], p[1], mode=p[2], cval=0.25)),
    _gauss_ref, exact, [(dt, sg, md) for dt in ("u16", "f64") for sg in SIGMAS for md in MODES], inkey=lambda p: p[0])


def _gauss_mm_dev(ctx, D, Hs, p):
    n = D[0].shape[0]
    mm = ctx.empty((n, 2), _F64)
    g = _hipops().gaussian(D[0], 2.0, minmax_out=mm)
    return _np(g, mm)


def _gauss_mm_ref(ins, p):
    g = skops.gaussian(ins[0], 2.0)
    return g, np.array([g.min(), g.max()])


add("gaussian minmax_out", "filters", lambda s, k, p: (img_u16(s, k),), _gauss_mm_dev, _gauss_mm_ref)
add("gaussian channel", "filters",
    lambda s, k, p: (np.stack([img_u16(s, k, 1), img_u16(s, k), img_u16(s, 2, 2)]),),
    lambda ctx, D, Hs, p: _np(_hipops().gaussian(D[0], 2.0, channel=1)),
    lambda ins, p: (skops.gaussian(ins[0][1], 2.0),))
add("difference_of_gaussians", "filters",
    lambda s, k, p: (img(p, s, k),),
    lambda ctx, D, Hs, p: _np(_hipops().difference_of_gaussians(D[0], 0.6, 3.0)),
    lambda ins, p: (skops.difference_of_gaussians(ins[0], 0.6, 3.0),), exact, ("u16", "f64"), inkey=lambda p: p)


def _nd_ref(ins, p):
    dt, mode, what = p
    f = skops.img_as_float(ins[0]) if dt == "u16" else ins[0]
    if what == "gaussian":
        return (ndi.gaussian_filter(f, 1.0, mode=mode, truncate=4.0),)
    return (ndi.gaussian_filter(f, 0.6, mode=mode, truncate=4.0) - ndi.gaussian_filter(f, 2.0, mode=mode, truncate=4.0),)


def _nd_dev(ctx, D, Hs, p):
    h = _hipops()
    if p[2] == "gaussian":
        return _per_plane(D, lambda v: _np(h.gaussian_nd(v, 1.0, mode=p[1])))
    return _per_plane(D, lambda v: _np(h.difference_of_gaussians_nd(v, 0.6, 2.0, mode=p[1])))


# ONE (3, H, W) volume per case: every axis is filtered (amt_convolve_axis0, then amt_gaussian; amt_subtract for the DoG)
add("gaussian_nd", "filters",
    lambda s, k, p: (np.stack([img(p[0], s, k), img(p[0], s, 2, 5), img(p[0], s, 0, 6)]),),
    _nd_dev, _nd_ref, exact,
    [(dt, md, w) for dt in ("u16", "f64") for md in ("nearest", "reflect", "wrap") for w in ("gaussian", "dog")],
    planes=False, inkey=lambda p: p[0])


def _elementwise_make(s, k, p):
    if p == "sub_clip0":
        return img_f64(s, k), np.asarray(0.4)
    if p in ("rescale u16", "rescale f64"):
        x = img(p[-3:], s, k)
        p1, p2 = np.percentile(x, (1, 99))
        return x, np.array([p1, p2 if p2 != p1 else p1 + 1.0])
    if p == "to_float64 f32":
        return (img_f64(s, k).astype(_F32),)
    if p == "to_float64 u16":
        return (img_u16(s, k),)
    return (img_f64(s, k),)  # add_scalar


def _elementwise_dev(ctx, D, Hs, p):
    h = _hipops()
    if p == "sub_clip0":
        return _np(h.sub_clip0(D[0], D[1]))
    if p.startswith("rescale"):
        return _np(h.rescale(D[0], D[1], (0.0, 1.0)))
    if p == "to_float64 u16":
        return _np(h.to_float64(D[0], 1.0 / 65535))
    if p == "to_float64 f32":
        return _np(h.to_float64(D[0]))
    return _np(h.add_scalar(D[0], -3.5))


def _elementwise_ref(ins, p):
    if p == "sub_clip0":
        return (np.clip(ins[0] - ins[1], 0, None),)
    if p.startswith("rescale"):
        return (skops.rescale_intensity(ins[0], (ins[1][0], ins[1][1]), (0.0, 1.0)),)
    if p == "to_float64 u16":
        return (ins[0] * (1.0 / 65535),)
    if p == "to_float64 f32":
        return (ins[0].astype(_F64),)
    return (ins[0] + -3.5,)


add("elementwise", "filters", _elementwise_make, _elementwise_dev, _elementwise_ref, exact,
    ("sub_clip0", "rescale u16", "rescale f64", "to_float64 u16", "to_float64 f32", "add_scalar"), inkey=lambda p: p)


def _crop_pad_dev(ctx, D, Hs, p):
    h = _hipops()
    H, W = D[0].shape[-2:]
    if p[0] == "pad":
        return _np(h.pad_edge(D[0], 2, 1))
    return _np(h.crop(D[0], H // 3, W // 4, H - H // 3 - H // 5, W - W // 4 - W // 5))


def _crop_pad_ref(ins, p):
    x = ins[0]
    H, W = x.shape
    if p[0] == "pad":
        return (np.pad(x, ((2, 2), (1, 1)), mode="edge"),)
    return (x[H // 3:H - H // 5, W // 4:W - W // 5],)


add("crop and pad_edge", "filters",
    lambda s, k, p: ({"u8": mask_of(s, k).view(_U8), "u16": img_u16(s, k), "f64": img_f64(s, k)}[p[1]],),
    _crop_pad_dev, _crop_pad_ref, exact, [(w, dt) for w in ("pad", "crop") for dt in ("u8", "u16", "f64")],
    inkey=lambda p: p[1])


def _codes_supported(shape, sigma, mode):
    H, W = shape
    r = int(4.0 * sigma + 0.5)
    return 1 <= r <= 12 and mode in ("nearest", "reflect", "mirror") and W % 8 == 0 and W >= 256 and H > 2 * r


def _codes_dev(ctx, D, Hs, p):
    """gaussian_otsu_codes in both forms where it takes the plane, and the answer of ..._supported everywhere."""
    h = _hipops()
    sigma, mode = p
    d = D[0]
    n, H, W = d.shape
    sup = bool(h.gaussian_otsu_codes_supported(d, sigma, mode=mode))
    flag = np.full((n, 1), sup)
    if not sup:
        return (flag,) + tuple(np.zeros((n, 0)) for _ in range(5))
    outs = []
    for with_prefix in (False, True):
        o = dict(codes=ctx.empty((n, H, W), _U16), thr=ctx.empty((n,), _F64), thr_code=ctx.empty((n,), _F64),
                 minmax=ctx.empty((n, 2), _F64), hist=ctx.empty((n, 256), np.uint32))
        prefix = ctx.empty((n, H, W), np.uint32) if with_prefix else None
        h.gaussian_otsu_codes(d, sigma, o["codes"], o["thr"], o["thr_code"], o["minmax"], o["hist"], mode=mode, prefix=prefix)
        mask = (o["codes"].numpy() > o["thr_code"].numpy()[:, None, None])
        outs.append((mask, o["thr"].numpy(), o["minmax"].numpy(), o["hist"].numpy(),
                     prefix.numpy() if with_prefix else None))
    two, one = outs
    same = all(np.array_equal(a, b) for a, b in zip(two[:4], one[:4]))
    if not same:  # the two forms differ: report the prefix form, whose comparison then fails where they differ
        two = one
    return (flag, two[0], two[1], two[2], two[3], one[4])


def _codes_ref(ins, p):
    sigma, mode = p
    shape = ins[0].shape
    # plane 1 of a (40, 264) stack stays 16-byte aligned (H * W * 2 bytes is a multiple of 16 for every W % 8 == 0)
    if not _codes_supported(shape, sigma, mode):
        return (np.array([False]),) + tuple(np.zeros((0,)) for _ in range(5))
    g = ndi.gaussian_filter(skops.img_as_float(ins[0]), sigma, mode=mode)
    mm = np.array([g.min(), g.max()])
    if mm[0] == mm[1]:
        thr, hist = g.flat[0], None
    else:
        thr = skops.threshold_otsu(g)
        hist = skops.histogram(g)[0]
    return (np.array([True]), g > thr, np.asarray(thr), mm, hist, (g.view(np.uint64) >> np.uint64(32)).astype(np.uint32))


def _hist_or_const(got, want):
    return (True, None) if want is None or want.dtype == object else exact(got, want)


add("gaussian_otsu_codes", "filters", lambda s, k, p: (img_u16(s, k),), _codes_dev, _codes_ref,
    (exact, exact, exact, exact, _hist_or_const, exact),
    [(2.0, "nearest"), (0.6, "reflect"), (3.0, "mirror"), (3.2, "nearest"), (2.0, "wrap")])


# ---- stats and thresholds -----------------------------------------------------------------------------------------------
def _stats_make(s, k, p):
    if p == "hist_range":
        return ((img_u16(s, k).astype(_F64) % 700.0) - 100.0,)
    return (img(p[-3:], s, k),)


def _stats_dev(ctx, D, Hs, p):
    h = _hipops()
    if p == "hist u16":
        return _np(h.histogram_u16(D[0]))
    if p == "hist f64":
        return _np(*h.histogram_f64(D[0]))
    if p == "minmax f64":
        return _np(h.minmax(D[0]))
    if p == "hist_range":
        return _np(h.histogram_range(D[0], -100, 700))
    return _np(h.threshold_otsu(D[0]))  # "otsu u16" / "otsu f64"


def _stats_ref(ins, p):
    x = ins[0]
    if p == "hist u16":
        return (np.bincount(x.ravel(), minlength=65536).astype(np.uint32),)
    if p == "hist f64":
        mm = np.array([x.min(), x.max()])
        return (skops.histogram(x)[0].astype(np.uint32), mm)
    if p == "minmax f64":
        return (np.array([x.min(), x.max()]),)
    if p == "hist_range":
        return (np.bincount((x + 100).astype(np.int64).ravel(), minlength=700).astype(np.uint32),)
    return (np.asarray(float(x.flat[0]) if x.min() == x.max() else skops.threshold_otsu(x), _F64),)


# regression case "hist f64" on (1, 1) and on the constant plane of every batch: amt_hist_f64 walked the samples of a
# constant plane (min == max: infinite scaling, every edge equal) into the LAST bin; np.histogram counts them in bin nbins / 2
add("histograms and otsu", "stats and thresholds", _stats_make, _stats_dev, _stats_ref, exact,
    ("hist u16", "hist f64", "minmax f64", "hist_range", "otsu u16", "otsu f64"), inkey=lambda p: p,
    extra_shapes=PERCENTILE_SHAPES)

_QS = ((0, 100), (1, 99), (50,), (0.1, 37.123, 50, 62.5, 99.9, 100))
add("percentile", "stats and thresholds",
    lambda s, k, p: (img(p[0], s, k),),
    lambda ctx, D, Hs, p: _np(_hipops().percentile(D[0], p[1])),
    lambda ins, p: (np.atleast_1d(np.percentile(ins[0], p[1])),), exact,
    [(dt, q) for dt in ("u16", "f64") for q in _QS], inkey=lambda p: p[0], extra_shapes=PERCENTILE_SHAPES)


def _masked_sums_rule(got, want):
    """masked_sums has no test of its own.  want = (fsum of x <= t, count, fsum of x > t, count, sum of |x|): the counts
    are exact; a sum of n float64 terms in ANY order differs from the exactly rounded sum (math.fsum) by at most
    (n - 1) u sum|x| to first order (u = 2^-53), plus the final rounding of fsum itself: bound n 2^-53 sum|x|."""
    n = want[1] + want[3]
    bound = n * 2.0 ** -53 * want[4]
    for i in (1, 3):
        if got[i] != want[i]:
            return False, (i,)
    for i in (0, 2):
        if not abs(got[i] - want[i]) <= bound:
            return False, (i,)
    return True, None


def _masked_sums_ref(ins, p):
    x, t = ins[0].ravel(), float(ins[1])
    le = x[x <= t] if np.isfinite(t) else x
    gt = x[x > t] if np.isfinite(t) else x[:0]
    return (np.array([math.fsum(le), le.size, math.fsum(gt), gt.size, math.fsum(np.abs(x))]),)


add("masked_sums", "stats and thresholds",
    lambda s, k, p: (img_f64(s, k) - 0.3, np.asarray(p, _F64)),
    lambda ctx, D, Hs, p: _np(_hipops().masked_sums(D[0], D[1])),
    _masked_sums_ref, _masked_sums_rule, (0.1, np.inf), extra_shapes=PERCENTILE_SHAPES)

add("greater_than", "stats and thresholds",
    lambda s, k, p: (img(p, s, k), np.asarray(np.median(img(p, s, k)), _F64)),
    lambda ctx, D, Hs, p: _np(_hipops().greater_than(D[0], D[1])),
    lambda ins, p: (ins[0] > ins[1],), exact, ("u16", "f64"), inkey=lambda p: p)
add("greater_than_image", "stats and thresholds",
    lambda s, k, p: (img(p, s, k), img_f64(s, 0, 9) * (65535 if p == "u16" else 1)),
    lambda ctx, D, Hs, p: _np(_hipops().greater_than_image(D[0], D[1])),
    lambda ins, p: (ins[0] > ins[1],), exact, ("u16", "f64"), inkey=lambda p: p)


def _apply_threshold_dev(ctx, D, Hs, p):
    from arcadia_microscopy_tools_amd.operations import apply_threshold

    dt, method, kw = p
    if "method" in kw:  # threshold_local's own method: apply_threshold's signature has no room for it
        from arcadia_microscopy_tools_amd.operations import _local_threshold

        return _per_plane(D, lambda d: _np(_hipops().greater_than_image(d, _local_threshold(d, **kw))))
    return _per_plane(D, lambda d: _np(apply_threshold(d, method, **kw)))


def _apply_threshold_ref(ins, p):
    dt, method, kw = p
    x = ins[0]
    if "method" in kw:  # threshold_local's mean / median straight from the filters: no shortcut for constant images
        return (x > skops.threshold_local(x, **kw),)
    if x.min() == x.max():  # a constant image has nothing above its threshold (the operator answers before any method)
        return (np.zeros(x.shape, bool),)
    if method == "local":
        return (x > skops.threshold_local(x, **kw),)
    if method in ("niblack", "sauvola"):
        return (x > getattr(skops, "threshold_" + method)(x, **kw),)
    return (x > getattr(skops, "threshold_" + method)(x),)


_GLOBAL = [(dt, m, {}) for dt in ("u16", "f64") for m in ("otsu", "li", "yen", "isodata", "triangle", "mean")]
# float64 li / mean: the class means come from the device's masked sums, whose order differs from numpy's pairwise one in
# the last ulps; the rule is that of tests/test_gpu_api.py (apply_threshold(gz, "MEAN" / "LI")): the MASK is bit-equal
add("apply_threshold global", "stats and thresholds", lambda s, k, p: (img(p[0], s, k),), _apply_threshold_dev,
    _apply_threshold_ref, exact, _GLOBAL, planes=False, inkey=lambda p: p[0])
add("apply_threshold local", "stats and thresholds", lambda s, k, p: (img_u16(s, k),), _apply_threshold_dev,
    _apply_threshold_ref, exact,
    [("u16", "local", dict(block_size=3)), ("u16", "local", dict(block_size=11)),
     ("u16", "local", dict(block_size=5, method="mean")), ("u16", "local", dict(block_size=7, method="mean", mode="nearest")),
     ("u16", "local", dict(block_size=3, method="median")), ("u16", "local", dict(block_size=5, method="median", offset=2.5))],
    planes=False)


def _window_dev(ctx, D, Hs, p):
    h = _hipops()
    dt, method, w = p
    t = h.window_threshold(D[0], w, method, 0.2)
    if dt == "u16":  # the rule of the uint16 tests: the MASK of image > threshold is exact
        return _np(h.greater_than_image(D[0], t))
    return _np(t)


def _window_ref(ins, p):
    dt, method, w = p
    t = getattr(skops, "threshold_" + method)(ins[0], window_size=w, k=0.2)
    return (ins[0] > t,) if dt == "u16" else (t,)


# float64 window thresholds: the window sums run in another order than scikit-image's integral images
# (test_edt_without_background_and_windows_beyond_the_image: rtol 1e-7, atol 1e-12)
add("window_threshold", "stats and thresholds", lambda s, k, p: (img(p[0], s, k),), _window_dev, _window_ref,
    params=[(dt, m, w) for dt in ("u16", "f64") for m in ("niblack", "sauvola") for w in (3, 15, (5, 9))],
    inkey=lambda p: p[0], rules_for=lambda p: exact if p[0] == "u16" else close(1e-7, 1e-12))


def _window_nd_dev(ctx, D, Hs, p):
    h = _hipops()
    return _per_plane(D, lambda v: _np(h.window_threshold(v, p[1], p[0], 0.2, r=32767.5 if p[0] == "sauvola" else None,
                                                          nd=True)))


# ONE (3, H, W) volume whose window spans every axis (amt_window_threshold_nd; test_operators_on_stacks_and_other_dtypes:
# rtol 1e-9, atol 1e-9)
add("window_threshold nd", "stats and thresholds",
    lambda s, k, p: (np.stack([img_u16(s, k), img_u16(s, 2, 5), img_u16(s, 0, 6)]),),
    _window_nd_dev, lambda ins, p: (getattr(skops, "threshold_" + p[0])(ins[0], window_size=p[1]),), close(1e-9, 1e-9),
    [("niblack", 3), ("sauvola", (3, 5, 7))], planes=False)


# ---- binary morphology -------------------------------------------------------------------------------------------------
_BFPS = {"cross": None, "disk1": skops.disk(1), "disk2": skops.disk(2), "sq3": np.ones((3, 3), _U8),
         "sq2": np.ones((2, 2), _U8), "r3x4": np.ones((3, 4), _U8), "disk4": skops.disk(4)}
add("binary morphology", "binary morphology",
    lambda s, k, p: (mask_of(s, k),),
    lambda ctx, D, Hs, p: _np(getattr(_hipops(), "binary_" + p[0])(D[0], _BFPS[p[1]])),
    lambda ins, p: (getattr(skops, "binary_" + p[0])(ins[0], _BFPS[p[1]]),), exact,
    [(o, f) for o in ("erosion", "dilation", "opening", "closing") for f in _BFPS])


def _toc_dev(ctx, D, Hs, p):
    h = _hipops()
    fp = skops.disk(p[1])
    if p[0] == "f64":
        return _np(h.threshold_open_close(D[0], D[1], fp))
    n, H, W = D[0].shape
    mm = h.minmax(D[0])
    thr, code, bins = ctx.empty((n,), _F64), ctx.empty((n,), _F64), ctx.empty((n, H, W), _U8)
    h.threshold_otsu_bins(D[0], mm, thr, code, bins)
    return _np(h.threshold_open_close(D[0], thr, fp, bins=bins, thr_code=code))


def _toc_make(s, k, p):
    x = skops.gaussian(img_u16(s, k), 1.5) if k != 1 else np.full(s, 0.25)
    t = float(np.quantile(x, 0.55)) if p[0] == "f64" else (float(x.flat[0]) if x.min() == x.max() else skops.threshold_otsu(x))
    return x, np.asarray(t, _F64)


# the fused '>' + opening + closing chain, by the float64 plane and by the byte bins of amt_otsu_f64_bins
add("threshold_open_close", "binary morphology", _toc_make, _toc_dev,
    lambda ins, p: (skops.binary_closing(skops.binary_opening(ins[0] > ins[1], skops.disk(p[1])), skops.disk(p[1])),),
    exact, [("f64", 1), ("f64", 2), ("f64", 6), ("bins", 2)], inkey=lambda p: p[0])


# ---- rank filters --------------------------------------------------------------------------------------------------------
_GFPS = {"disk1": skops.disk(1), "disk2": skops.disk(2), "disk3": skops.disk(3), "sq3": np.ones((3, 3), _U8),
         "row5": np.ones((1, 5), _U8), "col5": np.ones((5, 1), _U8), "sq2": np.ones((2, 2), _U8),
         "r4x3": np.ones((4, 3), _U8), "disk7": skops.disk(7)}
add("grey morphology", "rank filters",
    lambda s, k, p: (img(p[0], s, k),),
    lambda ctx, D, Hs, p: _np(getattr(_hipops(), p[1])(D[0], _GFPS[p[2]])),
    lambda ins, p: (getattr(skops, p[1])(ins[0], _GFPS[p[2]]),), exact,
    [(dt, o, f) for dt in ("u16", "f64") for o in ("erosion", "dilation", "opening", "closing", "white_tophat")
     for f in (_GFPS if dt == "u16" else ("disk2", "sq2", "disk7"))], inkey=lambda p: p[0])
add("median", "rank filters",
    lambda s, k, p: (img(p[0], s, k),),
    lambda ctx, D, Hs, p: _np(_hipops().median(D[0], _GFPS[p[1]], mode=p[2], cval=40000 if p[2] == "constant" else 0)),
    lambda ins, p: (ndi.median_filter(ins[0], footprint=_GFPS[p[1]], mode=p[2], cval=40000 if p[2] == "constant" else 0),),
    exact, [(dt, f, m) for dt in ("u16", "f64") for f, m in (("sq3", "nearest"), ("disk2", "reflect"), ("disk1", "constant"),
                                                              ("row5", "nearest"), ("col5", "reflect"), ("disk3", "nearest"))],
    inkey=lambda p: p[0])
# the boundary modes only the rank kernel itself takes (grey morphology uses 'reflect')
add("rank filter modes", "rank filters",
    lambda s, k, p: (img_u16(s, k),),
    lambda ctx, D, Hs, p: _np(_hipops()._rank(D[0], _GFPS[p[1]], p[0], p[2], p[3], None)),
    lambda ins, p: ((ndi.minimum_filter, ndi.maximum_filter)[p[0]](ins[0], footprint=_GFPS[p[1]], mode=p[2], cval=p[3]),),
    exact, [(o, f, m, c) for o in (0, 1) for f in ("disk2", "disk7") for m, c in (("nearest", 0), ("constant", 40000))])


# ---- labels --------------------------------------------------------------------------------------------------------------
def _label_make(s, k, p):
    if p[0] == "mask":
        return (mask_of(s, k),)
    if p[0] == "bytes":  # uint8 images that are NOT 0 / 1 masks are labelled by equal value
        return (values_of(s, k).astype(_U8),)
    return (values_of(s, k),)


def _label_ref(ins, p):
    x = ins[0] if ins[0].dtype == bool else ins[0].astype(_I32)
    lab = skops.label(x, p[1])
    return lab.astype(_I32), np.asarray(lab.max(), _I32)


add("label", "labels", _label_make, lambda ctx, D, Hs, p: _np(*_hipops().label(D[0], connectivity=p[1])), _label_ref, exact,
    [(k, c) for k in ("mask", "bytes", "int32") for c in (1, 2)], inkey=lambda p: p[0])
add("label_sparse", "labels", lambda s, k, p: (mask_of(s, k),),
    lambda ctx, D, Hs, p: _np(*_hipops().label_sparse(D[0], connectivity=p)), lambda ins, p: _label_ref(ins, (0, p)),
    exact, (1, 2))


def _cbr_ref(lab):
    cleared = skops.clear_border(lab)
    out = skops.relabel_sequential(cleared) if cleared.max() > 0 else cleared
    return out.astype(_I32), np.asarray(out.max(), _I32)


def _labelops_dev(ctx, D, Hs, p):
    h = _hipops()
    mx = max(int(Hs[0].max()), 1)
    if p == "clear_border":
        return _np(h.clear_border(D[0]))
    if p == "relabel_sequential":
        return _np(*h.relabel_sequential(D[0], mx))
    if p == "clear_border_relabel":
        return _np(*h.clear_border_relabel(D[0], mx))
    if p == "clear_border_relabel nlabels":
        return _np(*h.clear_border_relabel(D[0], mx, nlabels=D[1]))
    if p == "keep_labels":
        keep = np.zeros((Hs[0].shape[0], mx + 1), _U8)
        keep[:, 1::2] = 1
        return _np(h.keep_labels(D[0], ctx.asarray(keep), mx))
    if p == "to_int64":
        return _np(h.to_int64(D[0]))
    if p == "max_per_plane":
        return _np(h.max_per_plane(D[0]))
    if p == "cast u16":
        return _np(h.cast_labels(h.cast_labels(D[0], _U16), _I32), h.cast_labels(D[0], _U16))
    return _np(h.cast_labels(D[0], _U8))  # "cast u8"


def _labelops_ref(ins, p):
    x = ins[0]
    if p == "clear_border":
        return (skops.clear_border(x),)
    if p == "relabel_sequential":
        return skops.relabel_sequential(x).astype(_I32), np.asarray(len(np.unique(x[x != 0])), _I32)
    if p.startswith("clear_border_relabel"):
        return _cbr_ref(x)
    if p == "keep_labels":
        return (np.where(x % 2 == 1, x, 0),)
    if p == "to_int64":
        return (x.astype(np.int64),)
    if p == "max_per_plane":
        return (np.asarray(x.max(), _I32),)
    if p == "cast u16":
        return x, x.astype(_U16)
    return (x.astype(_U8),)


def _labelops_make(s, k, p):
    if p in ("clear_border", "relabel_sequential"):  # any label VALUES
        return (values_of(s, k) * (7 if p == "relabel_sequential" else 1),)
    lab = labels_of(s, k)
    if p == "clear_border_relabel nlabels":
        return lab, np.asarray(lab.max(), _I32)
    return (lab,)


add("label operators", "labels", _labelops_make, _labelops_dev, _labelops_ref, exact,
    ("clear_border", "relabel_sequential", "clear_border_relabel", "clear_border_relabel nlabels", "keep_labels", "to_int64",
     "max_per_plane", "cast u16", "cast u8"), inkey=lambda p: p)
add("expand_labels", "labels", lambda s, k, p: (labels_of(s, k),),
    lambda ctx, D, Hs, p: _np(_hipops().expand_labels(D[0], p[0], ring=p[1])),
    lambda ins, p: ((lambda g: np.where(ins[0] == 0, g, 0) if p[1] else g)(expand_ref.expand_two_pass(ins[0], p[0])),),
    exact, [(1, False), (2 ** 0.5, False), (4.2, True), (40, False), (-1, False)])


# ---- edt, peaks and watershed ------------------------------------------------------------------------------------------------
def _edt_ref(ins, p):
    e = skops.distance_transform_edt(ins[0])
    return np.rint(e * e).astype(_I32), e


add("edt", "edt, peaks and watershed", lambda s, k, p: (mask_of(s, k) if p == "mask" else np.ones(s, bool),),
    lambda ctx, D, Hs, p: _np(*_hipops().edt(D[0])), _edt_ref, exact, ("mask", "no background"))


def _relief_make(s, k, p):
    """An integer relief with plateaus and ties, and a mask unrelated to it."""
    rng = _rng(s, k, 400)
    if k == 1:
        d2 = np.zeros(s, _I32)
    elif k == 2:
        d2 = rng.integers(1, 4, s).astype(_I32)
    else:
        d2 = (ndi.uniform_filter(rng.integers(0, 41, s).astype(_F64), 5) * 3).astype(_I32)
    return d2, rng.random(s) < 0.85


def _peaks_ref(d2, mask, m):
    pk = (d2 == ndi.maximum_filter(d2, size=2 * m + 1, mode="constant")) & mask & (d2 > 0)
    if m > 0:
        pk[:m, :] = False
        pk[-m:, :] = False
        pk[:, :m] = False
        pk[:, -m:] = False
    return pk


add("peak_mask", "edt, peaks and watershed", _relief_make,
    lambda ctx, D, Hs, p: _np(_hipops().peak_mask(D[0], D[1], p)),
    lambda ins, p: (_peaks_ref(ins[0], ins[1], p),), exact, (0, 1, 5))


def _peak_markers_ref(ins, p):
    pk = _peaks_ref(ins[0], ins[1], p[0])
    lab = skops.label(pk, p[1])
    return pk, lab.astype(_I32), np.asarray(lab.max(), _I32)


# m = 0 on the dense plane lists every pixel: more than 4,096 peaks from (66, 320) on, the lists in arena scratch
# (AMT_PEAK_MARKERS_LDS_TIER)
add("peak_markers", "edt, peaks and watershed", _relief_make,
    lambda ctx, D, Hs, p: _np(*_hipops().peak_markers(D[0], D[1], p[0], p[1])), _peak_markers_ref, exact,
    [(0, 1), (1, 2), (2, 1), (5, 1)])


def _ws_make(s, k, p):
    m = mask_of(s, k)
    if p[0] == "f64":
        rng = _rng(s, k, 500)
        relief = ndi.gaussian_filter(rng.random(s), 2.0)
        mk = np.zeros(s, _I32)
        n = int(min(8, max(1, s[0] * s[1] // 6)))
        idx = rng.choice(s[0] * s[1], n, replace=False)  # distinct pixels, distinct smooth relief values: no ties
        mk.ravel()[idx] = np.arange(1, n + 1)
        return relief, mk, (m | (mk > 0)) if k != 1 else np.ones(s, bool)
    e = skops.distance_transform_edt(m)
    mk, n = skops.peak_markers(e, m, 1)
    return np.rint(e * e).astype(_I32), mk.astype(_I32), m, np.asarray(n, _I32)


def _ws_dev(ctx, D, Hs, p):
    h = _hipops()
    if p[0] == "f64":
        return _np(h.watershed(D[0], D[1], D[2], connectivity=p[1]))
    if p[0] == "edt":
        return _np(h.watershed_edt(D[0], D[1], D[2], seeds_first=True))
    mx = max(int(Hs[1].max()), 1)
    marker_list = None
    if p[0] == "cleared list":
        # every marker pixel per plane, as label_sparse(keep=) lists them: with W % 16 == 0 (and n % 16 == 0) the stage then
        # works from the mask's run tables instead of the parent plane
        n = Hs[1].shape[0]
        klist, kcount = np.zeros((n, max(int(np.count_nonzero(m)) for m in Hs[1]) + 8), _I32), np.zeros(n, _I32)
        for i, m in enumerate(Hs[1]):
            idx = np.flatnonzero(m)
            klist[i, :idx.size], kcount[i] = idx, idx.size
        marker_list = (ctx.asarray(klist), ctx.asarray(kcount))
    return _np(*h.watershed_edt_cleared(D[0], D[1], D[2], D[3], mx, ctx.empty(D[0].shape, _I32), marker_list=marker_list))


def _ws_ref(ins, p):
    from oracle.watershed import watershed

    if p[0] == "f64":
        return (watershed(ins[0], ins[1], mask=ins[2], connectivity=p[1]),)
    e = skops.distance_transform_edt(ins[2])
    ws = watershed(skops.seeded_flood_image(e, ins[1]), ins[1], mask=ins[2]) if ins[1].any() else np.zeros(ins[1].shape, _I32)
    return (ws.astype(_I32),) if p[0] == "edt" else _cbr_ref(ws.astype(_I32))


add("watershed", "edt, peaks and watershed", _ws_make, _ws_dev, _ws_ref, exact,
    [("f64", 1), ("f64", 2), ("edt", 1), ("cleared", 1), ("cleared list", 1)], inkey=lambda p: p[0].split()[0])


# ---- props, colocalisation and outlines ------------------------------------------------------------------------------------
PROPS_EXACT = ("label", "area", "bbox", "area_convex", "solidity", "euler_number", "area_filled", "feret_diameter_max",
               "centroid_local", "area_bbox", "extent")
PROPS_REL12 = ("perimeter_crofton", "inertia_tensor")
EXT_NAMES = ["euler_number", "perimeter_crofton", "area_filled", "feret_diameter_max", "area_bbox", "extent",
             "equivalent_diameter_area", "centroid_local", "inertia_tensor", "inertia_tensor_eigvals"]
IPROPS = ["intensity_mean", "intensity_max", "intensity_min", "intensity_std", "centroid_weighted", "centroid_weighted_local"]


def props_rule(got, want):
    """The column rules of tests/test_gpu_props_fuzz.py (_compare), on (keys, columns) tables."""
    gk, gv = got
    wk, wv = want
    if list(gk) != list(wk):
        return False, ("keys",)
    for k, g, w in zip(wk, gv, wv):
        g, w = np.asarray(g, _F64), np.asarray(w, _F64)
        if g.shape != w.shape:
            return False, (k, "shape")
        if k.startswith(PROPS_EXACT):
            ok = np.array_equal(g, w, equal_nan=True)
        elif k.startswith(PROPS_REL12):
            scale = np.abs(w).max() if w.size else 1.0
            ok = np.allclose(g, w, rtol=1e-12, atol=1e-12 * scale)
        elif k == "axis_minor_length":
            l2g, l2w = (g / 4) ** 2, (w / 4) ** 2
            scale = np.abs(l2w).max() if w.size else 1.0
            ok = np.allclose(l2g, l2w, rtol=1e-12, atol=1e-12 * scale)
        elif k.startswith("orientation"):
            # _compare's rule (direct, atol 1e-8; exactly symmetric regions are unpinned, SURVEY.md A.9, and must give
            # |pi / 4| as tests/test_gpu_props_ext.py asks), with ONE addition: a region whose reference is +-pi / 2 sits
            # on the branch cut of atan2 -- mu11 is exactly 0 on the device's integer moments and +-1e-17 in the oracle's
            # float ones, and the sign of that rounding error picks -pi / 2 or +pi / 2, the same axis.  Only there the
            # difference is taken modulo pi (the form of tests/test_gpu_plate.py's comparison with the oracle's tables).
            # Regression case: label 23 of the (40, 264) plane.
            sym = np.isclose(np.abs(w), np.pi / 4)
            cut = np.isclose(np.abs(w), np.pi / 2)
            d = g - w
            d[cut] = (d[cut] + np.pi / 2) % np.pi - np.pi / 2
            ok = np.allclose(d[~sym], 0, rtol=0, atol=1e-8) and np.allclose(np.abs(g[sym]), np.pi / 4)
        else:
            scale = np.nanmax(np.abs(w)) if np.isfinite(w).any() else 1.0
            ok = np.array_equal(np.isnan(g), np.isnan(w)) and np.allclose(g, w, rtol=1e-9, atol=1e-12 * max(scale, 1.0),
                                                                        equal_nan=True)
        if not ok:
            bad = ~np.isclose(g, w, rtol=0, atol=0, equal_nan=True)
            return False, (k, int(np.flatnonzero(bad)[0]) if bad.any() else -1)
    return True, None


def _props_make(s, k, p):
    return labels_of(s, k), np.stack([img_u16(s, 0, 11), img_u16(s, 2, 12)])


def _props_dev(ctx, D, Hs, p):
    """Every plane's table through the batch entry points, as (keys, columns) per plane (an object array over planes)."""
    from arcadia_microscopy_tools_amd.masks import DEFAULT_CELL_PROPERTY_NAMES
    from arcadia_microscopy_tools_amd.segment import assemble_cell_properties, ext_columns

    h = _hipops()
    n = Hs[0].shape[0]
    K = max(int(Hs[0].max()), 1)
    inten = D[1] if p == "u16" else ctx.asarray(Hs[1].astype(_F64) / 7.0)
    names = list(DEFAULT_CELL_PROPERTY_NAMES) + EXT_NAMES
    if p == "u16":
        mt, it = h.regionprops_full(D[0], inten, K)
    else:
        mt, it = h.regionprops(D[0], K), h.regionprops_intensity(D[0], inten, K)
    xt, wt = h.regionprops_ext(D[0], K, ext_columns(names, IPROPS), intensity=inten)
    mt, it, xt, wt = mt.numpy(), it.numpy(), xt.numpy(), wt.numpy()
    out, raw = [], []
    for i in range(n):
        k = int(Hs[0][i].max())
        d = assemble_cell_properties(mt[i][:k], it[i][:k], ("A", "B"), names, IPROPS, ext=xt[i][:k], wext=wt[i][:k])
        out.append((list(d), [np.asarray(v) for v in d.values()]))
        raw.append(np.concatenate([t[i][:k].ravel() for t in (mt, it, xt, wt)]))  # the tables' bytes, for the digest
    return _ragged(out), _ragged(raw)


def _props_ref(ins, p):
    from arcadia_microscopy_tools_amd.masks import DEFAULT_CELL_PROPERTY_NAMES

    lab = ins[0].astype(np.int64)
    chans = ins[1] if p == "u16" else ins[1].astype(_F64) / 7.0
    d = orp.cell_properties(lab, {"A": chans[0], "B": chans[1]}, list(DEFAULT_CELL_PROPERTY_NAMES) + EXT_NAMES, IPROPS)
    d.update(_inertia_tensor_exact(lab))
    return ((list(d), [np.asarray(v) for v in d.values()]), None)


def _inertia_tensor_exact(lab):
    """inertia_tensor-i-j of the labels 1..k as exactly rounded quotients of integer moment sums.  The oracle's float
    moments leave ~1e-17 in the off-diagonal entry of a mirror-symmetric region whose true value is 0; on a plane where
    that is the only entry of its column, the column's own scale (the atol of the rule) is that rounding error.  Regression
    case: label 23 of the (40, 264) plane."""
    from fractions import Fraction

    k = int(lab.max())
    yy, xx = np.nonzero(lab)
    l = lab[yy, xx]
    sums = [np.bincount(l, weights=None, minlength=k + 1)] + [
        np.array([int(v) for v in np.bincount(l, weights=w.astype(np.float64), minlength=k + 1)], object)
        for w in (yy, xx, yy * yy, xx * xx, yy * xx)]  # every sum is an integer far below 2^53: exact in float64
    out = {f"inertia_tensor-{i}-{j}": np.zeros(k) for i in (0, 1) for j in (0, 1)}
    for i in range(1, k + 1):
        n, sy, sx, syy, sxx, sxy = (int(s[i]) for s in sums)
        mu20, mu02, mu11 = Fraction(syy) - Fraction(sy * sy, n), Fraction(sxx) - Fraction(sx * sx, n), \
            Fraction(sxy) - Fraction(sy * sx, n)
        out["inertia_tensor-0-0"][i - 1] = float(mu02 / n)
        out["inertia_tensor-1-1"][i - 1] = float(mu20 / n)
        out["inertia_tensor-0-1"][i - 1] = out["inertia_tensor-1-0"][i - 1] = float(-mu11 / n)
    return out


add("regionprops", "props, colocalisation and outlines", _props_make, _props_dev, _props_ref,
    (props_rule, lambda g, w: (True, None)), ("u16", "f64"))


def _coloc_rule(p):
    def exact_rule(got, want):  # tests/test_gpu_colocalization.py: _assert_exact
        if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
            return False, ("NaNs sit elsewhere",)
        if not np.array_equal(got[..., 2:], want[..., 2:], equal_nan=True):
            return exact(got[..., 2:], want[..., 2:])
        g, w = got[..., :2], want[..., :2]
        ok = ~np.isnan(w)
        err = np.abs(g[ok] - w[ok]) / np.abs(w[ok]).clip(1e-300)
        err[g[ok] == w[ok]] = 0.0
        return (True, None) if not err.size or err.max() <= 1e-14 else (False, (int(np.argmax(err)),))

    def float_rule(got, want):  # _assert_float
        if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
            return False, ("NaNs sit elsewhere",)
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
        return (True, None) if not err.size or err.max() <= 1e-9 else (False, (int(np.argmax(err)),))

    return exact_rule if p == "u16" else float_rule


_COLOC_THR = {"u16": (1000, 20000.0, 40000.25), "f64": (0.0, 0.25, 0.5)}


def _coloc_make(s, k, p):
    stack = np.stack([img_u16(s, 0, 21), img_u16(s, 2, 22), img_u16(s, 0, 23)])
    return labels_of(s, k), stack if p == "u16" else stack.astype(_F64) / 65535.0


def _coloc_dev(ctx, D, Hs, p):
    K = max(int(Hs[0].max()), 1)
    t = _hipops().colocalization(D[0], D[1], K, thresholds=_COLOC_THR[p]).numpy()
    return (_ragged([t[i][:int(Hs[0][i].max())] for i in range(t.shape[0])]),)  # the rows of the plane's own labels


def _coloc_ref(ins, p):
    return (coloc_ref.table(ins[0].astype(np.int64), ins[1], int(ins[0].max()), _COLOC_THR[p]),)


add("colocalization", "props, colocalisation and outlines", _coloc_make, _coloc_dev, _coloc_ref, params=("u16", "f64"),
    inkey=lambda p: p, rules_for=_coloc_rule)


def _outline_rule(got, want):
    got, want = list(got), list(want)
    if len(got) != len(want):
        return False, ("count", len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g.tolist() != np.asarray(w).tolist():
            return False, (i,)
    return True, None


def _outlines_dev(fn):
    return lambda ctx, D, Hs, p: (_ragged([getattr(_hipops(), fn)(D[0][i], max(int(Hs[0][i].max()), 1))
                                           for i in range(D[0].shape[0])]),)


add("cell_outlines", "props, colocalisation and outlines", lambda s, k, p: (labels_of(s, k),),
    _outlines_dev("cell_outlines"), lambda ins, p: (ocontours.extract_outlines_skimage(ins[0]),), _outline_rule, planes=False)
for _s in ((1, 1), (1, 17), (19, 1)):
    EXCLUDED[("cell_outlines", _s)] = ("marching squares needs 2 x 2 samples: skimage.measure.find_contours, and the "
                                       "oracle with it, refuses a one-row or one-column plane")
add("cell_outlines_borders", "props, colocalisation and outlines", lambda s, k, p: (labels_of(s, k),),
    _outlines_dev("cell_outlines_borders"), lambda ins, p: (ocontours.extract_outlines_cellpose(ins[0]),), _outline_rule,
    planes=False)
add("label_bboxes", "props, colocalisation and outlines", lambda s, k, p: (labels_of(s, k),),
    lambda ctx, D, Hs, p: (_ragged([b[:int(Hs[0][i].max())] for i, b in
                                    enumerate(_hipops().label_bboxes(D[0], max(int(Hs[0].max()), 1)))]),),
    lambda ins, p: (np.array([[sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1]
                              for sl in ndi.find_objects(ins[0])], _I32).reshape(-1, 4),))


# ---- cellpose ----------------------------------------------------------------------------------------------------------------
def _flows_of(s, k):
    """Flows of the kind synth.synthetic_flows makes (unit vectors towards the centre of each disc times a smooth
    profile, a logit-like probability), with discs small enough for the plane: kind 1 has no cell, kind 2 many and noise."""
    rng = _rng(s, k, 700)
    H, W = s
    yy, xx = np.mgrid[0:H, 0:W].astype(_F32)
    dP, prob, taken = np.zeros((2, H, W), _F32), np.full(s, -6.0, _F32), np.zeros(s, bool)
    for _ in range((max(1, H * W // 900), 0, max(2, H * W // 300))[k]):
        r = float(rng.integers(2, max(3, min(9, min(H, W) // 2 + 1))))
        cy, cx = float(rng.uniform(0, H)), float(rng.uniform(0, W))
        d = np.hypot(yy - cy, xx - cx)
        inside = (d < r) & ~taken
        taken |= inside
        norm = np.maximum(d, 1e-3)
        dP[0][inside] = (-(yy - cy) / norm)[inside] * 5.0 * np.minimum(d / 2.0, 1.0)[inside]
        dP[1][inside] = (-(xx - cx) / norm)[inside] * 5.0 * np.minimum(d / 2.0, 1.0)[inside]
        prob[inside] = 6.0
    if k == 2:
        dP += rng.normal(0, 0.3, dP.shape).astype(_F32)
    return dP, prob


# parity unpinned (oracle/cellpose_dynamics.py): masks identical, per-mask flow errors within rtol 1e-9 / atol 1e-12
# (tests/test_gpu_cellpose.py)
def _cp_masks_ref(ins, p):
    m = cd.compute_masks(ins[0], ins[1], niter=60, min_size=p[0], flow_threshold=p[1], fill_holes=p[2])
    return m.astype(_I32), np.asarray(m.max(), _I32)


add("cellpose_masks", "cellpose", lambda s, k, p: _flows_of(s, k),
    lambda ctx, D, Hs, p: _np(*_hipops().cellpose_masks(D[0], D[1], niter=60, min_size=p[0], flow_threshold=p[1],
                                                        fill_holes=p[2])),
    _cp_masks_ref, exact, [(15, 0.0, False), (0, 0.0, True), (15, 0.4, False)], inkey=lambda p: 0)
for _s in ((1, 1), (1, 17), (19, 1)):
    EXCLUDED[("cellpose_masks", _s)] = ("cellpose's follow_flows scales the flows by H / (H - 1) and W / (W - 1): the "
                                        "published algorithm, and the oracle with it, divides by zero on one row or column")


def _flow_error_dev(ctx, D, Hs, p):
    K = max(int(Hs[0].max()), 1)
    e = _hipops().cellpose_flow_error(D[0], D[1], K).numpy()
    return (_ragged([e[i][:int(Hs[0][i].max())] for i in range(e.shape[0])]),)


add("cellpose_flow_error", "cellpose", lambda s, k, p: (labels_of(s, k), _flows_of(s, 2)[0]), _flow_error_dev,
    lambda ins, p: (cd.flow_error(ins[0], ins[1]) if ins[0].any() else np.zeros(0),), close(1e-9, 1e-12))
add("fill_holes_remove_small", "cellpose", lambda s, k, p: (labels_of(s, k),),
    lambda ctx, D, Hs, p: _np(_hipops().fill_holes_remove_small(D[0], max(int(Hs[0].max()), 1), p[0], p[1])[0]),
    lambda ins, p: (cd.fill_holes_and_remove_small_masks(ins[0], p[0], p[1]).astype(_I32),), exact,
    [(15, True), (0, False), (3, True)], inkey=lambda p: 0)


def _normalize_make(s, k, p):
    x = {"u16": img_u16(s, k), "f32": (img_f64(s, k) * 1000 / 7).astype(_F32), "f64": img_f64(s, k) * 1e4 / 3.0}[p[0]]
    lohi = np.percentile(x.astype(_F32).astype(_F64), (1, 99))
    return x, lohi.astype(_F32 if p[1] == "f32" else _F64)


def _normalize_ref(ins, p):
    x32 = ins[0].astype(_F32)
    lo, hi = ins[1].astype(_F32)
    d = _F32(hi) - _F32(lo)
    y = (x32 - _F32(lo)) / d if d > _F32(1e-3) else np.zeros(x32.shape, _F32)
    return (_F32(1.0) - y if p[2] else y,)


add("normalize_planes", "cellpose", _normalize_make,
    lambda ctx, D, Hs, p: _np(_hipops().normalize_planes(D[0], D[1], invert=p[2])), _normalize_ref, same_bits,
    [("u16", "f64", False), ("f32", "f32", True), ("f64", "f64", False), ("u16", "f32", True)], inkey=lambda p: p[:2])


# ---- overlay and plate --------------------------------------------------------------------------------------------------------
_LAYERS = (("#00ff00", 1.0, True, "alpha"), ("#ff00ff", 0.6, False, "additive"), ("#3366cc", 0.3, True, "additive"))


def _overlay_dev(ctx, D, Hs, p):
    from arcadia_microscopy_tools_amd import BlendMode, Channel, Layer, create_overlay

    def one(bg, *planes):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # values outside [0, 1] are part of the case: clipped inside the kernel
            layers = [Layer(Channel(f"c{i}", color=c), x, o, z, BlendMode.ADDITIVE if m == "additive" else BlendMode.ALPHA)
                      for i, ((c, o, z, m), x) in enumerate(zip(_LAYERS[:p], planes))]
            return _np(create_overlay(bg, layers))
    return _per_plane(D, one)


add("overlay", "overlay and plate",
    lambda s, k, p: tuple(img_f64(s, k if i == 0 else (k + i) % 3, 30 + i) * 1.2 - 0.1 for i in range(1 + p)),
    _overlay_dev,
    lambda ins, p: (oblend.create_overlay(ins[0], [(c, x, o, z, m) for (c, o, z, m), x in zip(_LAYERS[:p], ins[1:])]),),
    exact, (0, 1, 3), planes=False)
add("deinterleave", "overlay and plate",
    lambda s, k, p: (np.stack([img_u16(s, k, 40 + c) for c in range(p)], axis=-1),),
    lambda ctx, D, Hs, p: _np(_hipops().deinterleave(D[0], p)),
    lambda ins, p: (np.ascontiguousarray(ins[0].transpose(2, 0, 1)),), exact, (1, 3, 4))


def _pack_make(s, k, p):
    """One "plane" = one field of view: a (K, 14) table, a (K, C, 4) table and its cell count, K from the shape."""
    from arcadia_microscopy_tools_amd import _hip

    rng = _rng(s, k, 600)
    K = min(s[0] * s[1], 40)
    n = (int(rng.integers(0, K + 1)), 0, K)[k]
    return rng.normal(size=(K, _hip.RP_NCOLS)), rng.normal(size=(K, 2, 4)), np.asarray(n, _I32)


def _pack_dev(ctx, D, Hs, p):
    rows, nrows = _hipops().pack_plate_rows(D[0], D[1] if p else None, D[2], fov_index0=9)
    n = int(nrows.numpy()[0])
    got = rows.numpy()[:n]
    cuts = np.cumsum(Hs[2])[:-1]
    per = []
    for i, blk in enumerate(np.split(got, cuts)):
        blk = blk.copy()
        blk[:, 0] -= i  # the FOV index counts the planes of the call: plane i of a batch carries 9 + i
        per.append(blk)
    return (_ragged(per),)


add("pack_plate_rows", "overlay and plate", _pack_make, _pack_dev,
    lambda ins, p: (np.array([np.concatenate([[9, r + 1], ins[0][r]] + ([ins[1][r].ravel()] if p else []))
                              for r in range(int(ins[2]))], _F64).reshape(int(ins[2]), 16 + (8 if p else 0)),),
    params=(True, False))


def operators():
    return [o.name for o in OPS]


def case_count():
    """(operator, shape) pairs in the table and excluded from it."""
    total = sum(len(SHAPES) + len(o.extra_shapes) for o in OPS)
    return total, len(EXCLUDED)


def check_table():
    """The conditions on EXCLUDED: at most 5 % of the (operator, shape) pairs, no operator with fewer than ten shapes, every
    pair a real one with a reason that says more than "fails"."""
    total, excluded = case_count()
    assert excluded <= 0.05 * total, (excluded, total)
    names = {o.name: o for o in OPS}
    for (name, shape), reason in EXCLUDED.items():
        assert name in names and shape in SHAPES + list(names[name].extra_shapes), (name, shape)
        assert isinstance(reason, str) and len(reason) > 20 and reason.strip().lower() not in ("fails", "fail"), (name, shape)
    for o in OPS:
        assert len(o.shapes()) >= 10, (o.name, len(o.shapes()))


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
def inputs(op, pi, shape, kind):
    """The host arrays of one plane; made once and shared (read-only)."""
    key = (op.name, pi, shape, kind)
    if key not in _IN_CACHE:
        ins = tuple(np.array(a, order="C") for a in op.make(shape, kind, op.params[pi]))
        for a in ins:
            a.setflags(write=False)
        _IN_CACHE[key] = ins
    return _IN_CACHE[key]


def reference(op, pi, shape, kind):
    """The expected outputs of one plane; computed once and shared."""
    key = (op.name, pi, shape, kind)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = op.ref(inputs(op, pi, shape, kind), op.params[pi])
    return _REF_CACHE[key]


def variants(op):
    return ("single", "view", "batch") if op.planes else ("single", "view")


def kinds_checked(op):
    """The plane kinds whose reference a sweep needs (the leading plane of a view is only there to be skipped)."""
    return (0, 1, 2) if op.planes else (0,)


def _rules(op, p, nout):
    r = op.rules_for(p)
    return r if isinstance(r, tuple) else (r,) * nout


def _digest(outs):
    h = hashlib.sha256()
    for o in outs:
        if isinstance(o, np.ndarray) and o.dtype != object:
            h.update(str(o.dtype).encode() + str(o.shape).encode() + np.ascontiguousarray(o).tobytes())
        else:  # per-plane results of different sizes: tables of each plane's own labels, lists of outlines
            items = o.ravel() if isinstance(o, np.ndarray) else [o]
            for item in items:
                h.update(repr(_plain(item)).encode())
    return h.hexdigest()


def _plain(x):
    if isinstance(x, (np.ndarray, np.generic)):
        x = np.asarray(x)
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes().hex())
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def _plane_of(out, i):
    return out[i]


def _compare(op, p, outs, i, want):
    rules = _rules(op, p, len(want))
    for k, (rule, w) in enumerate(zip(rules, want)):
        ok, idx = rule(_plane_of(outs[k], i), w)
        if not ok:
            return False, (k, idx)
    return True, None


def _upload(ctx, planes_ins, view):
    """planes_ins: one tuple of host arrays per plane -> (device arrays, host arrays), planes stacked on axis 0; view:
    behind one more plane of which the result is a slice."""
    Hs = [np.stack([pl[j] for pl in planes_ins]) for j in range(len(planes_ins[0]))]
    D = [ctx.asarray(h)[1:] if view else ctx.asarray(h) for h in Hs]
    if view:
        Hs = [h[1:] for h in Hs]
    return D, Hs


class Recorder:
    """Wraps the functions of the loaded library for the duration of the sweep: notes which entry points were called and,
    with ``scratch_check``, looks at the scratch padding after every call that may have used scratch."""

    # context, memory, stream, event, timer and host helpers: they reserve no scratch
    HELPERS = ("amt_device_count", "amt_ctx_", "amt_last_error", "amt_version", "amt_device_name", "amt_malloc", "amt_free",
               "amt_memcpy_", "amt_memset", "amt_sync", "amt_stream_wait", "amt_event_", "amt_host_", "amt_timer_",
               "amt_debug_scratch_check")

    def __init__(self, ctx, scratch_check):
        from arcadia_microscopy_tools_amd import _hip

        self.ctx, self.check, self.lib = ctx, scratch_check, _hip.load_library()
        self.names = _hip.exported_names()
        self.called: set = set()
        self.dirty: list = []
        self.where = None
        self._orig = {}

    def __enter__(self):
        for name in self.names:
            fn = getattr(self.lib, name)
            self._orig[name] = fn
            setattr(self.lib, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self._orig.items():
            setattr(self.lib, name, fn)
        return False

    def _wrap(self, name, fn):
        helper = name.startswith(self.HELPERS)

        def call(*args):
            self.called.add(name)
            rc = fn(*args)
            if self.check and not helper and rc == 0:
                found = self.ctx.scratch_check()
                if found is not None:
                    self.dirty.append({"entry": name, "slot": found[0], "offset": found[1], "case": self.where})
            return rc
        return call


def run(ctx, families=None, scratch_check=False, ops=None, shapes=None, only=None, pick=None):
    """Every case of the families (default: all): {"records": [...], "called": [...], "dirty": [...], "seconds": s}.
    ``ops``: only these operators; ``shapes``: these shapes instead of the table's (EXCLUDED still holds for the kind of
    plane it names: callers pass shapes the operators take); ``only``: only these variants; ``pick(op, p)``: only the
    parameter sets it answers True for."""
    families = FAMILIES if families is None else tuple(families)
    records = []
    t0 = time.perf_counter()
    with Recorder(ctx, scratch_check) as rec:
        for op in OPS:
            if op.family not in families or (ops is not None and op.name not in ops):
                continue
            for shape in (op.shapes() if shapes is None else shapes):
                cache = {}
                for pi, p in enumerate(op.params):
                    if pick is not None and not pick(op, p):
                        continue
                    for variant in variants(op):
                        if only is not None and variant not in only:
                            continue
                        rec.where = [op.name, repr(p), list(shape), variant]
                        records.append(_run_case(ctx, op, pi, p, shape, variant, cache))
    return {"records": records, "called": sorted(rec.called), "dirty": rec.dirty, "seconds": time.perf_counter() - t0}


def _run_case(ctx, op, pi, p, shape, variant, cache):
    kinds = {"single": (0,), "view": (2, 0), "batch": (0, 1, 2)}[variant]
    ins_all = [inputs(op, pi, shape, k) for k in kinds]
    key = (op.inkey(p), variant) if op.inkey(p) is not None else None
    if key is not None and key in cache:
        D, Hs = cache[key]
    else:
        D, Hs = _upload(ctx, ins_all, variant == "view")
        if key is not None:
            cache[key] = (D, Hs)
    outs = op.dev(ctx, D, Hs, p)
    record = {"family": op.family, "op": op.name, "param": repr(p), "shape": list(shape), "variant": variant,
              "status": "pass", "index": None, "sha256": _digest(outs)}
    checked = kinds[1:] if variant == "view" else kinds
    for i, kind in enumerate(checked):
        ins, want = inputs(op, pi, shape, kind), reference(op, pi, shape, kind)
        ok, idx = _compare(op, p, outs, i, want)
        if ok and variant == "batch":
            # the plane of the batch against the same plane alone: bit for bit, whatever the rule against the reference
            D1, H1 = _upload(ctx, [ins], False)
            alone = op.dev(ctx, D1, H1, p)
            if _digest([_plane_of(o, i) for o in outs]) != _digest([_plane_of(o, 0) for o in alone]):
                ok, idx = False, ("batch plane differs from the single-plane result", i)
        if not ok:
            record.update(status="mismatch", index=repr((i, idx)))
            break
    return record


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", required=True, help="where to write the records, the scratch findings and the entry points")
    ap.add_argument("--family", action="append", help="only this family (repeatable)")
    ap.add_argument("--profile", help="also write the sweep's time, its cases per family and the entry points reached here")
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison = poison_child.poisoned()
    res = run(get_context(), args.family, scratch_check=poison)
    poison_child.write(args.json, res)
    if args.profile:
        per = {f: sum(r["family"] == f for r in res["records"]) for f in FAMILIES}
        with open(args.profile, "w") as f:
            json.dump({"device": get_context().device_name(), "poison": poison, "sweep_seconds": round(res["seconds"], 2),
                       "cases": len(res["records"]), "cases_per_family": per, "entry_points": res["called"]}, f, indent=1)
            f.write("\n")
    bad = [r for r in res["records"] if r["status"] != "pass"]
    for r in bad[:20]:
        print("MISMATCH", r["op"], r["param"], r["shape"], r["variant"], r["index"], flush=True)
    for d in res["dirty"][:20]:
        print("DIRTY SCRATCH", d, flush=True)
    print(f"{len(res['records'])} cases, {len(bad)} mismatches, {len(res['dirty'])} dirty scratch checks, "
          f"{res['seconds']:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
