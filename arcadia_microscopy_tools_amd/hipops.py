"""Batch device operators: thin, shape-checked Python wrappers over the C ABI (include/amt_hip.h).

Every function takes ``DeviceArray`` inputs whose LAST TWO axes are (Y, X); all leading axes are
independent planes processed by one launch.  ``out=`` lets a caller reuse buffers (no allocation, no
implicit synchronisation inside a pipeline).  Nothing here touches the host except where stated
(small parameter tables; results are only copied back by ``DeviceArray.numpy()``).

The functions mirror the scikit-image / scipy calls the reference makes (file:line in each docstring).
"""
from __future__ import annotations

import ctypes
import operator

import numpy as np

from . import _hip
from .device import Context, DeviceArray

_c_double_p = ctypes.POINTER(ctypes.c_double)


def _lib():
    return _hip.load_library()


def _planes(a: DeviceArray):
    if a.ndim < 2:
        raise ValueError(f"expected at least a 2-D array, got shape {a.shape}")
    H, W = a.shape[-2:]
    return a.nplanes, int(H), int(W)


def _out(ctx: Context, out, shape, dtype) -> DeviceArray:
    if out is None:
        return ctx.empty(shape, dtype)
    if tuple(out.shape) != tuple(shape) or out.dtype != np.dtype(dtype):
        raise ValueError(f"out has shape {out.shape} dtype {out.dtype}, need {tuple(shape)} {np.dtype(dtype)}")
    if out.ctx is not ctx:
        # the operator runs on the INPUT's stream: an output owned by another context would be written without any
        # ordering against that context's work
        raise ValueError("out belongs to another context than the input; bind the input with DeviceArray.on(ctx)")
    return out


def _span(x):
    """(start, byte length, element size) of a DeviceArray; an explicit triple stands for a strided view."""
    if x is None or isinstance(x, tuple):
        return x
    return int(x.ptr), int(x.nbytes), int(x.dtype.itemsize)


def _no_alias(op: str, ins: dict, outs: dict, inplace=()):
    """The aliasing rule of include/amt_hip.h (Conventions) on ``DeviceArray.ptr`` / ``nbytes``, before any device access:
    inputs may overlap inputs; an output must not overlap any other operand, not even in part, except that the
    (output, input) pairs named in ``inplace`` may coincide exactly -- same start, same byte length, same element size."""
    spans = [(n, _span(a), False) for n, a in ins.items()] + [(n, _span(a), True) for n, a in outs.items()]
    spans = [s for s in spans if s[1] is not None and s[1][1] > 0]
    for i, (na, sa, oa) in enumerate(spans):
        for nb, sb, ob in spans[i + 1:]:
            if not (oa or ob) or sa[0] + sa[1] <= sb[0] or sb[0] + sb[1] <= sa[0]:
                continue
            o, x = (na, nb) if oa else (nb, na)
            if oa != ob and (o, x) in inplace:
                if sa == sb:
                    continue
                raise ValueError(f"{op}: {o} may alias {x} only in place (same start, same length, same element size); "
                                 "this overlap is partial")
            raise ValueError(f"{op}: {o} must not alias {x}, nor overlap it in part")


def _in_code(a: DeviceArray) -> int:
    if a.dtype == np.uint16:
        return _hip.U16
    if a.dtype == np.float64:
        return _hip.F64
    raise TypeError(f"device filters accept uint16 or float64 images, got {a.dtype}")


def _channel_stack(labels: DeviceArray, intensity: DeviceArray, n: int, H: int, W: int):
    """(C, in_code) of ``intensity`` (..., C, Y, X) uint16 or float64, one (C, Y, X) stack per plane of ``labels``"""
    if intensity.dtype not in (np.uint16, np.float64):
        raise TypeError("intensity images must be uint16 or float64 on the device path")
    if intensity.ndim < 3 or intensity.shape[-2:] != labels.shape[-2:]:
        raise ValueError("intensity must be (..., C, Y, X) matching the label planes")
    C = int(intensity.shape[-3])
    if intensity.size != n * C * H * W:
        raise ValueError("intensity / labels plane count mismatch")
    return C, _hip.U16 if intensity.dtype == np.uint16 else _hip.F64


def _host_f64(arr):
    a = np.ascontiguousarray(arr, dtype=np.float64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


# --------------------------------------------------------------------------------------------------
# filters
# --------------------------------------------------------------------------------------------------
def gaussian_weights(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """The 1-D kernel scipy builds (SP/_filters.py:226-236,314-323); computed with the host's numpy so the
    device shares np.exp's rounding with the CPU path."""
    sigma = float(sigma)
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x**2)
    return phi / phi.sum()


def gaussian(a: DeviceArray, sigma: float, mode: str = "nearest", cval: float = 0.0, truncate: float = 4.0,
             scale: float | None = None, out: DeviceArray | None = None, channel: int | None = None,
             minmax_out: DeviceArray | None = None) -> DeviceArray:
    """``skimage.filters.gaussian`` per plane (SK/filters/_gaussian.py:119-126): uint16 input is first
    converted like ``img_as_float`` (x * (1/65535), SK/util/dtype.py:319) unless ``scale`` is given."""
    ctx = a.ctx
    n, H, W = _planes(a)
    ptr, stride, oshape = a.ptr, 0, a.shape
    if channel is not None:  # a is (..., C, Y, X): filter that channel of every stack in one launch
        if a.ndim < 3:
            raise ValueError("channel= needs a (..., C, Y, X) array")
        C = a.shape[-3]
        n, stride, oshape = n // C, C * H * W, a.shape[:-3] + (H, W)
        ptr = a.ptr + int(channel) * H * W * a.dtype.itemsize
    o = _out(ctx, out, oshape, np.float64)
    if sigma <= 1e-15:  # scipy skips axes with sigma <= 1e-15 (SP/_filters.py:423)
        w = np.ones(1)
    else:
        w = gaussian_weights(sigma, truncate)
    r = (len(w) - 1) // 2
    wa, wp = _host_f64(w)
    if scale is None:
        scale = 1.0 / 65535 if a.dtype == np.uint16 else 1.0
    if minmax_out is not None and (minmax_out.dtype != np.float64 or minmax_out.size != 2 * n):
        raise ValueError("minmax_out must be a float64 DeviceArray with 2 values per output plane")
    isz = a.dtype.itemsize  # the planes of a channel lie `stride` elements apart: first plane to the end of the last
    src = (int(ptr), ((n - 1) * stride + H * W) * isz if stride and n else n * H * W * isz, isz)
    _no_alias("gaussian", {"a": src}, {"out": o, "minmax_out": minmax_out})
    _hip.check(_lib().amt_gaussian(ctx.handle, ptr, _in_code(a), float(scale), o.ptr, n, H, W, wp, r,
                                   _hip.MODES[mode], float(cval), stride,
                                   minmax_out.ptr if minmax_out is not None else None), "amt_gaussian")
    return o


def gaussian_nd(a: DeviceArray, sigma: float, mode: str = "nearest", cval: float = 0.0, truncate: float = 4.0,
                out: DeviceArray | None = None, scale: float | None = None) -> DeviceArray:
    """``skimage.filters.gaussian`` of ONE n-D image the way scikit-image / scipy filter it: EVERY axis, leading axes
    first (SP/_filters.py:412-430), the intermediate kept in float64 -- unlike ``gaussian``, whose leading axes are
    independent planes.  2-D arrays go straight to ``gaussian``."""
    if a.ndim <= 2:
        return gaussian(a, sigma, mode, cval, truncate, scale=scale, out=out)
    ctx = a.ctx
    if sigma <= 1e-15:
        return gaussian(a, sigma, mode, cval, truncate, scale=scale, out=out)
    w = gaussian_weights(sigma, truncate)
    r = (len(w) - 1) // 2
    wa, wp = _host_f64(w)
    if scale is None:
        scale = 1.0 / 65535 if a.dtype == np.uint16 else 1.0
    cur, cur_scale = a, scale
    shape = a.shape
    for k in range(a.ndim - 2):  # the leading axes, one 1-D pass each
        outer = int(np.prod(shape[:k], dtype=np.int64)) if k else 1
        L, inner = int(shape[k]), int(np.prod(shape[k + 1:], dtype=np.int64))
        nxt = ctx.empty(shape, np.float64)
        _hip.check(_lib().amt_convolve_axis0(ctx.handle, cur.ptr, _in_code(cur), float(cur_scale), nxt.ptr, outer, L, inner,
                                             wp, r, _hip.MODES[mode], float(cval)), "amt_convolve_axis0")
        cur, cur_scale = nxt, 1.0
    return gaussian(cur, sigma, mode, cval, truncate, scale=cur_scale, out=out)


def gaussian_otsu_codes_supported(a: DeviceArray, sigma: float, mode: str = "nearest", truncate: float = 4.0,
                                  channel: int | None = None) -> bool:
    """Whether ``gaussian_otsu_codes`` can take this batch (uint16, fused-radius Gaussian, aligned rows)."""
    if a.dtype != np.uint16 or sigma <= 1e-15:
        return False
    _, H, W = _planes(a)
    r = int(truncate * float(sigma) + 0.5)
    stride = a.shape[-3] * H * W if channel is not None else 0
    ptr = a.ptr + (int(channel) * H * W * 2 if channel is not None else 0)
    return bool(_lib().amt_gaussian_otsu_codes_supported(H, W, r, _hip.MODES[mode], stride)) and ptr % 16 == 0


def gaussian_otsu_codes(a: DeviceArray, sigma: float, codes: DeviceArray, thr: DeviceArray, thr_code: DeviceArray,
                        minmax: DeviceArray, hist: DeviceArray, mode: str = "nearest", truncate: float = 4.0,
                        channel: int | None = None, prefix: DeviceArray | None = None) -> DeviceArray:
    """``threshold_otsu(gaussian(a, sigma))`` per plane WITHOUT the float64 image: ``thr`` receives the thresholds,
    ``codes`` (uint16, one per pixel) and ``thr_code`` continue the chain -- ``gaussian(a) > thr`` is exactly
    ``codes > thr_code`` (csrc/amt_filters.hip, gauss_lds_kernel EPI 2), so ``threshold_open_close(codes, thr_code)``
    yields the mask of the separate operators.  ``minmax`` (n, 2) and ``hist`` (n, 256) receive np.histogram's range
    and counts.  All outputs are caller-owned device arrays (nothing is allocated per call).

    ``prefix`` (uint32, one word per pixel, scratch): the Gaussian runs ONCE and leaves the upper half of every float64
    sample there; histogram and codes come from a streaming pass over that plane, and the few samples whose 32 bits do
    not decide their bin are recomputed exactly.  Without it the Gaussian runs twice.  Same outputs either way."""
    ctx = a.ctx
    n, H, W = _planes(a)
    ptr, stride = a.ptr, 0
    if channel is not None:
        C = a.shape[-3]
        n, stride = n // C, C * H * W
        ptr = a.ptr + int(channel) * H * W * a.dtype.itemsize
    if a.dtype != np.uint16:
        raise TypeError("gaussian_otsu_codes takes uint16 images")
    for name, arr, dt, size in (("codes", codes, np.uint16, n * H * W), ("thr", thr, np.float64, n),
                                ("thr_code", thr_code, np.float64, n), ("minmax", minmax, np.float64, 2 * n),
                                ("hist", hist, np.uint32, 256 * n), ("prefix", prefix, np.uint32, n * H * W)):
        if arr is None and name == "prefix":
            continue
        if arr.dtype != dt or arr.size != size:
            raise ValueError(f"{name} must be a {np.dtype(dt).name} DeviceArray of {size} elements")
        if arr.ctx is not ctx:
            raise ValueError(f"{name} belongs to another context than the input")
    src = (int(ptr), ((n - 1) * stride + H * W) * 2 if stride and n else n * H * W * 2, 2)
    _no_alias("gaussian_otsu_codes", {"a": src}, {"codes": codes, "thr": thr, "thr_code": thr_code, "minmax": minmax,
                                                  "hist": hist, "prefix": prefix})
    w = gaussian_weights(sigma, truncate)
    r = (len(w) - 1) // 2
    wa, wp = _host_f64(w)
    _hip.check(_lib().amt_gaussian_otsu_codes(ctx.handle, ptr, 1.0 / 65535, n, H, W, wp, r, _hip.MODES[mode], stride,
                                              minmax.ptr, hist.ptr, thr.ptr, thr_code.ptr, codes.ptr,
                                              prefix.ptr if prefix is not None else None),
               "amt_gaussian_otsu_codes")
    return codes


def difference_of_gaussians(a: DeviceArray, low_sigma: float, high_sigma: float, mode: str = "nearest",
                            cval: float = 0.0, truncate: float = 4.0, out: DeviceArray | None = None,
                            scale: float | None = None) -> DeviceArray:
    """``skimage.filters.difference_of_gaussians`` (SK/filters/_gaussian.py:258-290; R/operations.py:91).  ``scale``:
    the factor of ``img_as_float`` (default: 1/65535 for uint16 planes, 1 for float64)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, a.shape, np.float64)
    _no_alias("difference_of_gaussians", {"a": a}, {"out": o})
    wl, wh = gaussian_weights(low_sigma, truncate), gaussian_weights(high_sigma, truncate)
    wla, wlp = _host_f64(wl)
    wha, whp = _host_f64(wh)
    if scale is None:
        scale = 1.0 / 65535 if a.dtype == np.uint16 else 1.0
    _hip.check(_lib().amt_dog(ctx.handle, a.ptr, _in_code(a), scale, o.ptr, n, H, W, wlp, (len(wl) - 1) // 2, whp,
                              (len(wh) - 1) // 2, _hip.MODES[mode], float(cval)), "amt_dog")
    return o


def difference_of_gaussians_nd(a: DeviceArray, low_sigma: float, high_sigma: float, mode: str = "nearest",
                               cval: float = 0.0, truncate: float = 4.0, out: DeviceArray | None = None,
                               scale: float | None = None) -> DeviceArray:
    """``skimage.filters.difference_of_gaussians`` of ONE n-D image: both Gaussians filter EVERY axis
    (SK/filters/_gaussian.py:284-290), unlike ``difference_of_gaussians``, whose leading axes are independent planes."""
    ctx = a.ctx
    lo = gaussian_nd(a, low_sigma, mode, cval, truncate, scale=scale)
    hi = gaussian_nd(a, high_sigma, mode, cval, truncate, scale=scale)
    o = _out(ctx, out, a.shape, np.float64)
    _hip.check(_lib().amt_subtract(ctx.handle, lo.ptr, hi.ptr, o.ptr, _hip.F64, a.size), "amt_subtract")
    return o


def sub_clip0(a: DeviceArray, level: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    """``np.clip(a - level, 0, None)`` with one level per plane (R/operations.py:97)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, a.shape, np.float64)
    _no_alias("sub_clip0", {"a": a, "level": level}, {"out": o}, inplace={("out", "a")})
    _hip.check(_lib().amt_sub_clip0_f64(ctx.handle, a.ptr, level.ptr, o.ptr, n, H * W), "amt_sub_clip0_f64")
    return o


def rescale(a: DeviceArray, in_range: DeviceArray, out_range=(0.0, 1.0), out: DeviceArray | None = None):
    """``skimage.exposure.rescale_intensity(a, in_range=(p1, p2), out_range=(lo, hi))`` per plane with the
    (p1, p2) pairs on the device (SK/exposure/exposure.py:405-428; R/operations.py:50)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, a.shape, np.float64)
    _no_alias("rescale", {"a": a, "in_range": in_range}, {"out": o}, inplace={("out", "a")})  # float64 planes only: the sizes
    _hip.check(_lib().amt_rescale(ctx.handle, a.ptr, _in_code(a), in_range.ptr, float(out_range[0]),
                                  float(out_range[1]), o.ptr, n, H * W), "amt_rescale")
    return o


def uniform_filter(a: DeviceArray, size: int, mode: str = "reflect", cval: float = 0.0, out=None) -> DeviceArray:
    """``ndi.convolve1d(x, ones(size)/size)`` along axis 0 then axis 1 (threshold_local's 'mean',
    SK/filters/thresholding.py:224-229); the image is NOT rescaled (no img_as_float)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    if size % 2 == 0:
        raise ValueError("uniform_filter: size must be odd")
    o = _out(ctx, out, a.shape, np.float64)
    _no_alias("uniform_filter", {"a": a}, {"out": o})
    w = 1.0 / size * np.ones((size,))
    wa, wp = _host_f64(w)
    _hip.check(_lib().amt_gaussian(ctx.handle, a.ptr, _in_code(a), 1.0, o.ptr, n, H, W, wp, (size - 1) // 2,
                                   _hip.MODES[mode], float(cval), 0, None), "amt_gaussian")
    return o


def to_float64(a: DeviceArray, scale: float = 1.0, out=None) -> DeviceArray:
    """uint16 -> float64 (``x * scale``; ``img_as_float`` uses 1/65535, SK/util/dtype.py:319), or float32 -> float64
    (exact; no scale)."""
    if a.dtype == np.float32:
        if scale != 1.0:
            raise ValueError("to_float64 of a float32 array takes no scale")
        o = _out(a.ctx, out, a.shape, np.float64)
        _no_alias("to_float64", {"a": a}, {"out": o})
        _hip.check(_lib().amt_convert_f32_f64(a.ctx.handle, a.ptr, o.ptr, a.size), "amt_convert_f32_f64")
        return o
    if a.dtype != np.uint16:
        raise TypeError("to_float64 expects uint16 or float32")
    o = _out(a.ctx, out, a.shape, np.float64)
    _no_alias("to_float64", {"a": a}, {"out": o})
    _hip.check(_lib().amt_convert_u16_f64(a.ctx.handle, a.ptr, float(scale), o.ptr, a.size), "amt_convert_u16_f64")
    return o


def normalize_planes(planes: DeviceArray, lohi: DeviceArray, invert: bool = False,
                     out: DeviceArray | None = None) -> DeviceArray:
    """``CellposeModel.eval``'s image normalisation per plane (R/model.py:206-215; cellpose 4.0.x ``normalize99``,
    restated, parity unpinned): with ``lo, hi = float32(lohi[plane])`` and ``d = hi - lo``, ``(x - lo) / d`` in float32
    (one subtraction, one correctly rounded division) where ``d > 1e-3`` and 0 for the whole plane otherwise;
    ``invert``: 1 minus that.  ``planes``: uint16, float32 or float64 (rounded once to float32), last two axes (Y, X);
    ``lohi``: one (lo, hi) pair per plane on the device, float64 (``percentile``'s output as it is) or float32.
    Returns float32 of ``planes``' shape."""
    ctx = planes.ctx
    n, H, W = _planes(planes)
    if planes.dtype not in (np.uint16, np.float32, np.float64):
        raise TypeError(f"normalize_planes accepts uint16, float32 or float64 planes, got {planes.dtype}")
    if lohi.dtype not in (np.float32, np.float64):
        raise TypeError(f"normalize_planes: lohi must be float32 or float64, got {lohi.dtype}")
    if lohi.size != 2 * n:
        raise ValueError(f"normalize_planes: lohi has shape {lohi.shape}, need one (lo, hi) pair for each of {n} planes")
    if lohi.ctx is not ctx:
        raise ValueError("lohi belongs to another context than the planes; bind it with DeviceArray.on(ctx)")
    o = _out(ctx, out, planes.shape, np.float32)
    _no_alias("normalize_planes", {"planes": planes, "lohi": lohi}, {"out": o})
    codes ={np.dtype(np.uint16): _hip.U16, np.dtype(np.float32): _hip.F32, np.dtype(np.float64): _hip.F64}
    _hip.check(_lib().amt_normalize_planes_f32(ctx.handle, planes.ptr, codes[planes.dtype], lohi.ptr, codes[lohi.dtype],
                                               1 if invert else 0, o.ptr, n, H * W), "amt_normalize_planes_f32")
    return o


def add_scalar(a: DeviceArray, s: float, out=None) -> DeviceArray:
    o = _out(a.ctx, out, a.shape, np.float64)
    _no_alias("add_scalar", {"a": a}, {"out": o}, inplace={("out", "a")})
    _hip.check(_lib().amt_add_scalar_f64(a.ctx.handle, a.ptr, float(s), o.ptr, a.size), "amt_add_scalar_f64")
    return o


def deinterleave(yxc: DeviceArray, C: int, out: DeviceArray | None = None) -> DeviceArray:
    """(..., Y, X, C) interleaved ND2 frames -> (..., C, Y, X) (R/nikon.py:25-43)."""
    ctx = yxc.ctx
    if yxc.ndim < 3 or yxc.shape[-1] != C:
        raise ValueError("deinterleave expects (..., Y, X, C)")
    H, W = yxc.shape[-3:-1]
    lead = yxc.shape[:-3]
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    o = _out(ctx, out, tuple(lead) + (C, H, W), np.uint16)
    _no_alias("deinterleave", {"yxc": yxc}, {"out": o})
    _hip.check(_lib().amt_deinterleave_u16(ctx.handle, yxc.ptr, o.ptr, n, H, W, C), "amt_deinterleave_u16")
    return o


# --------------------------------------------------------------------------------------------------
# statistics and thresholds
# --------------------------------------------------------------------------------------------------
def histogram_u16(a: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    """65536-bin uint32 histogram per plane (np.bincount of SK/exposure/exposure.py:70)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, (n, 65536), np.uint32)
    _no_alias("histogram_u16", {"a": a}, {"out": o})
    _hip.check(_lib().amt_hist_u16(ctx.handle, a.ptr, o.ptr, n, H * W), "amt_hist_u16")
    return o


def histogram_range(a: DeviceArray, lo: int, nbins: int) -> DeviceArray:
    """One bin per integer ``lo .. lo + nbins - 1`` of an integer-valued float64 array (per plane): scikit-image's
    histogram of integer images whose range exceeds uint16 (SK/exposure/exposure.py:63-74)."""
    ctx = a.ctx
    if a.dtype != np.float64:
        raise TypeError("histogram_range expects the float64 image an integer image beyond uint16 travels as")
    n, H, W = _planes(a)
    o = ctx.empty((n, int(nbins)), np.uint32)
    _hip.check(_lib().amt_hist_range_f64(ctx.handle, a.ptr, float(lo), int(nbins), o.ptr, n, H * W), "amt_hist_range_f64")
    return o


def minmax(a: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, (n, 2), np.float64)
    _no_alias("minmax", {"a": a}, {"out": o})
    _hip.check(_lib().amt_minmax_f64(ctx.handle, a.ptr, o.ptr, n, H * W), "amt_minmax_f64")
    return o


def histogram_f64(a: DeviceArray, nbins: int = 256, mm: DeviceArray | None = None, out: DeviceArray | None = None):
    """``np.histogram(a, bins=nbins)`` counts per plane + the (min, max) pairs (SK/exposure/exposure.py:139)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    if mm is None:
        mm = minmax(a)
    o = _out(ctx, out, (n, nbins), np.uint32)
    _no_alias("histogram_f64", {"a": a, "mm": mm}, {"out": o})
    _hip.check(_lib().amt_hist_f64(ctx.handle, a.ptr, mm.ptr, o.ptr, nbins, n, H * W), "amt_hist_f64")
    return o, mm


def percentile(a: DeviceArray, q, out: DeviceArray | None = None) -> DeviceArray:
    """``np.percentile(a, q)`` (method 'linear') per plane -> (nplanes, len(q)) float64 on the device."""
    ctx = a.ctx
    n, H, W = _planes(a)
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.any(qa < 0) or np.any(qa > 100):
        raise ValueError("Percentiles must be in the range [0, 100]")
    o = _out(ctx, out, (n, len(qa)), np.float64)
    _no_alias("percentile", {"a": a}, {"out": o})
    qh, qp = _host_f64(qa)
    if a.dtype == np.uint16:
        _hip.check(_lib().amt_percentile_u16(ctx.handle, a.ptr, qp, len(qa), o.ptr, n, H * W), "amt_percentile_u16")
    elif a.dtype == np.float64:
        _hip.check(_lib().amt_percentile_f64(ctx.handle, a.ptr, qp, len(qa), o.ptr, n, H * W), "amt_percentile_f64")
    else:
        raise TypeError(f"percentile: unsupported dtype {a.dtype}")
    return o


def masked_sums(a: DeviceArray, thr: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    """Per plane {sum(a <= t), count(a <= t), sum(a > t), count(a > t)} for float64 images (bit-reproducible)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    if a.dtype != np.float64:
        raise TypeError("masked_sums expects float64")
    o = _out(ctx, out, (n, 4), np.float64)
    _no_alias("masked_sums", {"a": a, "thr": thr}, {"out": o})
    _hip.check(_lib().amt_masked_sums_f64(ctx.handle, a.ptr, thr.ptr, o.ptr, n, H * W), "amt_masked_sums_f64")
    return o


def crop(a: DeviceArray, top: int, left: int, h: int, w: int, out: DeviceArray | None = None) -> DeviceArray:
    """``a[..., top:top+h, left:left+w]`` as a new device array (R/operations.py:132)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, a.shape[:-2] + (h, w), a.dtype)
    _no_alias("crop", {"a": a}, {"out": o})
    _hip.check(_lib().amt_copy_rect(ctx.handle, a.ptr, o.ptr, a.dtype.itemsize, n, H, W, int(top), int(left), int(h),
                                    int(w)), "amt_copy_rect")
    o.is_bool = a.is_bool
    return o


def pad_edge(a: DeviceArray, py: int, px: int) -> DeviceArray:
    """``np.pad(a, ((py, py), (px, px)), mode='edge')`` per plane."""
    ctx = a.ctx
    n, H, W = _planes(a)
    o = ctx.empty(a.shape[:-2] + (H + 2 * py, W + 2 * px), a.dtype)
    _hip.check(_lib().amt_pad_edge(ctx.handle, a.ptr, o.ptr, a.dtype.itemsize, n, H, W, int(py), int(px)), "amt_pad_edge")
    o.is_bool = a.is_bool
    return o


def threshold_otsu(a: DeviceArray, nbins: int = 256, out: DeviceArray | None = None,
                   minmax: DeviceArray | None = None) -> DeviceArray:
    """``skimage.filters.threshold_otsu`` per plane, value stays on the device (SK/filters/thresholding.py:321-350).
    ``minmax`` = per-plane [min, max] already known for a float64 image (``gaussian(..., minmax_out=)``)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, (n,), np.float64)
    if minmax is not None and (a.dtype != np.float64 or minmax.dtype != np.float64 or minmax.size != 2 * n):
        raise ValueError("minmax needs a float64 image and 2 float64 values per plane")
    _no_alias("threshold_otsu", {"a": a, "minmax": minmax}, {"out": o})
    _hip.check(_lib().amt_threshold_value(ctx.handle, a.ptr, _in_code(a), _hip.THR_OTSU, nbins, o.ptr, None, n, H * W,
                                          minmax.ptr if minmax is not None else None), "amt_threshold_value")
    return o


def greater_than(a: DeviceArray, thr: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    """``a > thr[plane]`` -> uint8 0/1 mask (R/operations.py:216)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, a.shape, np.uint8)
    _no_alias("greater_than", {"a": a, "thr": thr}, {"out": o})
    _hip.check(_lib().amt_threshold_gt(ctx.handle, a.ptr, _in_code(a), thr.ptr, o.ptr, n, H * W), "amt_threshold_gt")
    o.is_bool = True
    return o


def window_threshold(a: DeviceArray, window_size=15, method: str = "niblack", k: float = 0.2, r=None,
                     out: DeviceArray | None = None, nd: bool = False) -> DeviceArray:
    """``skimage.filters.threshold_niblack`` / ``threshold_sauvola`` threshold image (float64)
    (SK/filters/thresholding.py:967-1087).  Default: per plane, ``window_size`` an odd integer or (rows, columns).
    ``nd=True``: ``a`` is ONE n-D image and the window spans every axis, as scikit-image treats a stack -- an odd
    integer (the same on every axis) or one value per axis.  ``r`` defaults to half the dtype range as in scikit-image."""
    ctx = a.ctx
    n, H, W = _planes(a)
    nlead = a.ndim - 2 if nd else 0
    if isinstance(window_size, (tuple, list, np.ndarray)):
        if len(window_size) != 2 + nlead:
            raise ValueError("window_size must be an integer or one value per image axis"
                             + ("" if nd else " (rows, columns)"))
        ws = [int(v) for v in window_size]
    else:
        ws = [int(window_size)] * (2 + nlead)
    for v in ws:
        if v % 2 == 0:
            raise ValueError(f"Window size {v} is even.")
    wy, wx = ws[-2], ws[-1]
    if r is None:
        r = 0.5 * 65535 if a.dtype == np.uint16 else 1.0  # 0.5 * (imax - imin); float range is (-1, 1)
    o = _out(ctx, out, a.shape, np.float64)
    _no_alias("window_threshold", {"a": a}, {"out": o})
    meth = 0 if method == "niblack" else 1
    if nlead and any(v != 1 for v in ws[:nlead]):
        import ctypes

        shp = (ctypes.c_int * nlead)(*[int(v) for v in a.shape[:nlead]])
        win = (ctypes.c_int * nlead)(*ws[:nlead])
        _hip.check(_lib().amt_window_threshold_nd(ctx.handle, a.ptr, _in_code(a), o.ptr, nlead, shp, win, H, W, wy, wx,
                                                  meth, float(k), float(r)), "amt_window_threshold")
    else:  # windows of one sample along the leading axes: every plane on its own
        _hip.check(_lib().amt_window_threshold(ctx.handle, a.ptr, _in_code(a), o.ptr, n, H, W, wy, wx, meth, float(k),
                                               float(r)), "amt_window_threshold")
    return o


def greater_than_image(a: DeviceArray, thr_image: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    ctx = a.ctx
    o = _out(ctx, out, a.shape, np.uint8)
    _no_alias("greater_than_image", {"a": a, "thr_image": thr_image}, {"out": o})
    _hip.check(_lib().amt_threshold_gt_image(ctx.handle, a.ptr, _in_code(a), thr_image.ptr, o.ptr, a.size),
               "amt_threshold_gt_image")
    o.is_bool = True
    return o


# --------------------------------------------------------------------------------------------------
# morphology
# --------------------------------------------------------------------------------------------------
def disk(radius: int) -> np.ndarray:
    """``skimage.morphology.disk`` (X**2 + Y**2 <= r**2)."""
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X**2 + Y**2) <= radius**2, dtype=np.uint8)


def cross3() -> np.ndarray:
    """skimage's default footprint: ndi.generate_binary_structure(2, 1)."""
    return np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=np.uint8)


def _fp(footprint, even: str = "scipy"):
    """The footprint as a C-contiguous uint8 array with ODD sides (what the C ABI takes).  An even side is padded with
    a zero row / column, which is exact: scipy centres a filter of even size s at s // 2, i.e. where the odd filter
    of size s + 1 with the zero line APPENDED is centred (``even="scipy"``: ndi.grey_erosion / grey_dilation /
    median_filter / binary_erosion / binary_dilation all agree with their padded form, dilation's origin shift
    included); scikit-image's grey erosion / dilation PREPEND it (``even="skimage"``, SK/morphology/grey.py:14-50
    with shift_x = shift_y = False) and the second halves of its opening / closing append it (``"skimage-shift"``)."""
    fp = np.asarray(cross3() if footprint is None else np.asarray(footprint) != 0, dtype=np.uint8)
    if fp.ndim != 2:
        raise ValueError("footprint must be 2-D")
    m, n = fp.shape
    if m % 2 == 0:
        z = np.zeros((1, n), np.uint8)
        fp = np.vstack((z, fp)) if even == "skimage" else np.vstack((fp, z))
        m += 1
    if n % 2 == 0:
        z = np.zeros((m, 1), np.uint8)
        fp = np.hstack((z, fp)) if even == "skimage" else np.hstack((fp, z))
    return np.ascontiguousarray(fp)


_MORPH_OPS = {"erode": 0, "dilate": 1, "open": 2, "close": 3, "fill_holes": 4, "remove_small_objects": 5,
              "remove_small_holes": 6, "skeletonize": _hip.MORPH_SKELETONIZE,
              "neighbor_classes": _hip.MORPH_NEIGHBOR_CLASSES}  # AMT_MORPH_*


def _binary(which: str, a: DeviceArray, footprint, out, border_value=None):
    ctx = a.ctx
    if a.dtype != np.uint8:
        raise TypeError("binary morphology expects a uint8 / bool mask on the device")
    n, H, W = _planes(a)
    fp = _fp(footprint)
    o = _out(ctx, out, a.shape, np.uint8)
    _no_alias("binary_" + which, {"a": a}, {"out": o})
    op = _MORPH_OPS[which]
    if border_value is None or op >= _MORPH_OPS["open"]:  # open / close apply skimage's border rules themselves
        border_value = 1 if which == "erode" else 0
    _hip.check(_lib().amt_binary_morph(ctx.handle, a.ptr, o.ptr, n, H, W, fp.ctypes.data_as(ctypes.c_void_p),
                                       fp.shape[0], fp.shape[1], op, int(border_value)), "amt_binary_morph")
    o.is_bool = True
    return o


def binary_erosion(a, footprint=None, out=None):
    """``skimage.morphology.binary_erosion`` (SK/morphology/binary.py:42; outside counts as True)."""
    return _binary("erode", a, footprint, out)


def binary_dilation(a, footprint=None, out=None):
    """``skimage.morphology.binary_dilation`` (SK/morphology/binary.py:77)."""
    return _binary("dilate", a, footprint, out)


def binary_opening(a, footprint=None, out=None):
    """``skimage.morphology.binary_opening`` = dilation(erosion(a)), fused (SK/morphology/binary.py:82-113)."""
    return _binary("open", a, footprint, out)


def binary_closing(a, footprint=None, out=None):
    """``skimage.morphology.binary_closing`` = erosion(dilation(a)), fused (SK/morphology/binary.py:116-147)."""
    return _binary("close", a, footprint, out)


def _fill_structure(structure) -> np.ndarray:
    """The structure of ``binary_fill_holes`` as uint8 (3, 3): None is the cross; any array whose ``!= 0`` pattern is the
    3 x 3 cross or 3 x 3 all-ones is taken, anything else refused (no device call is made)."""
    if structure is None:
        return cross3()
    st = np.ascontiguousarray(np.asarray(structure) != 0, dtype=np.uint8)
    if st.shape != (3, 3) or not (np.array_equal(st, cross3()) or st.all()):
        raise ValueError("binary_fill_holes: structure must be the 3 x 3 cross (generate_binary_structure(2, 1)) or "
                         "3 x 3 all-ones (generate_binary_structure(2, 2))")
    return st


def binary_fill_holes(a: DeviceArray, structure=None, out: DeviceArray | None = None) -> DeviceArray:
    """``scipy.ndimage.binary_fill_holes(a != 0, structure)`` per plane of a (H, W) or (N, H, W) uint8 / bool mask: a
    background pixel is filled when its background component (4-connected for the cross, 8-connected for all-ones)
    holds no pixel of the image's 1-pixel frame (amt_binary_morph, AMT_MORPH_FILL_HOLES)."""
    st = _fill_structure(structure)
    if a.dtype != np.uint8:
        raise TypeError("binary_fill_holes expects a uint8 / bool mask on the device")
    if a.ndim not in (2, 3):
        raise ValueError(f"binary_fill_holes takes (H, W) or (N, H, W) masks, got shape {a.shape}")
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, a.shape, np.uint8)
    if o is a:
        raise ValueError("binary_fill_holes: out must not alias the input")
    # any overlap, not only the same address: the write-out of one plane would land in input still to be read
    _no_alias("binary_fill_holes", {"a": a}, {"out": o})
    if a.size == 0:
        o.is_bool = True
        return o
    _hip.check(_lib().amt_binary_morph(ctx.handle, a.ptr, o.ptr, n, H, W, st.ctypes.data_as(ctypes.c_void_p), 3, 3,
                                       _MORPH_OPS["fill_holes"], 0), "amt_binary_morph")
    o.is_bool = True
    return o


def _area_filter(which: str, a: DeviceArray, size, connectivity, out) -> DeviceArray:
    """Both area filters: every refusal comes before the first device call; the size travels in ``border_value``."""
    if connectivity not in (1, 2):
        raise ValueError(f"{which}: connectivity must be 1 (4-connected) or 2 (8-connected), got {connectivity!r}")
    size = int(operator.index(size))
    if a.dtype != np.uint8:
        raise TypeError(f"{which} expects a uint8 / bool mask on the device")
    if a.ndim not in (2, 3):
        raise ValueError(f"{which} takes (H, W) or (N, H, W) masks, got shape {a.shape}")
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, a.shape, np.uint8)
    if o is a:
        raise ValueError(f"{which}: out must not alias the input")
    _no_alias(which, {"a": a}, {"out": o})
    o.is_bool = True
    if a.size == 0:
        return o
    if size <= 1 and a.is_bool:
        # nothing can be removed (no component has fewer than one pixel): the 0 / 1 mask as it is
        _hip.check(_lib().amt_memcpy_d2d(ctx.handle, o.ptr, a.ptr, a.nbytes), "amt_memcpy_d2d")
        return o
    # a uint8 plane that is not known to hold 0 / 1 goes through the filter at size 1, which writes its truth values
    size = min(max(size, 1), H * W + 1)  # beyond H * W every size removes everything alike
    st = cross3() if connectivity == 1 else np.ones((3, 3), np.uint8)
    _hip.check(_lib().amt_binary_morph(ctx.handle, a.ptr, o.ptr, n, H, W, st.ctypes.data_as(ctypes.c_void_p), 3, 3,
                                       _MORPH_OPS[which], size), "amt_binary_morph")
    return o


def remove_small_objects(a: DeviceArray, min_size: int = 64, connectivity: int = 1,
                         out: DeviceArray | None = None) -> DeviceArray:
    """``skimage.morphology.remove_small_objects(a != 0, min_size, connectivity)`` per plane of a (H, W) or (N, H, W)
    uint8 / bool mask: a foreground pixel stays when its component (``connectivity`` 1: 4-connected, 2: 8-connected) has
    at least ``min_size`` pixels (amt_binary_morph, AMT_MORPH_REMOVE_SMALL_OBJECTS)."""
    return _area_filter("remove_small_objects", a, min_size, connectivity, out)


def remove_small_holes(a: DeviceArray, area_threshold: int = 64, connectivity: int = 1,
                       out: DeviceArray | None = None) -> DeviceArray:
    """``skimage.morphology.remove_small_holes(a != 0, area_threshold, connectivity)`` per plane: a background pixel is
    filled when its background component has fewer than ``area_threshold`` pixels, whether or not the component touches
    the frame (amt_binary_morph, AMT_MORPH_REMOVE_SMALL_HOLES)."""
    return _area_filter("remove_small_holes", a, area_threshold, connectivity, out)


def skeleton_block() -> tuple[int, int, int]:
    """(tile rows, tile words of 64 pixels, sub-iterations per launch) of the thinning kernel (AMT_SKELETON_*): planes
    larger than a tile cross tile seams, and shapes thicker than twice the depth take several launches."""
    return _hip.SKELETON_TILE_ROWS, _hip.SKELETON_TILE_WORDS, _hip.SKELETON_BLOCK_SUBITERS


def _skeleton_op(which: str, a: DeviceArray, st: np.ndarray, value: int, out) -> DeviceArray:
    """Ops 7 / 8 of amt_binary_morph once the scalar arguments are checked: every other refusal, then the call."""
    if a.dtype != np.uint8:
        raise TypeError(f"{which} expects a uint8 / bool mask on the device")
    if a.ndim not in (2, 3):
        raise ValueError(f"{which} takes (H, W) or (N, H, W) masks, got shape {a.shape}")
    ctx = a.ctx
    n, H, W = _planes(a)
    if out is a:
        raise ValueError(f"{which}: out must not alias the input")
    o = _out(ctx, out, a.shape, np.uint8)  # allocates only when no `out` was given, and then nothing is left to refuse
    _no_alias(which, {"a": a}, {"out": o})
    o.is_bool = which == "skeletonize"
    if a.size == 0:
        return o
    _hip.check(_lib().amt_binary_morph(ctx.handle, a.ptr, o.ptr, n, H, W, st.ctypes.data_as(ctypes.c_void_p), 3, 3,
                                       _MORPH_OPS[which], value), "amt_binary_morph")
    return o


def skeletonize(a: DeviceArray, max_iter: int = 0, out: DeviceArray | None = None) -> DeviceArray:
    """Thinning of every plane of a (H, W) or (N, H, W) uint8 / bool mask to its centre lines by Zhang and Suen's 1984
    rule, the one ``skimage.morphology.skeletonize`` cites for 2-D input (amt_binary_morph, AMT_MORPH_SKELETONIZE;
    include/amt_hip.h states the rule in full).  Foreground is ``a != 0``, outside the image is background, the result
    holds 0 / 1.  ``max_iter``: at most that many iterations (two sub-iterations each) per plane, 0 = until an iteration
    clears nothing.  The fixed point is unique, so two runs give identical bytes.  scikit-image applies the rule through
    a 256-entry table; parity with that table is unpinned offline.  The call waits for the device."""
    if isinstance(max_iter, (bool, np.bool_)):
        raise TypeError("skeletonize: max_iter must be an integer, got a bool")
    try:
        k = int(operator.index(max_iter))
    except TypeError:
        raise TypeError(f"skeletonize: max_iter must be an integer, got {type(max_iter).__name__}") from None
    if k < 0 or k > 2**31 - 1:
        raise ValueError(f"skeletonize: max_iter must be 0 (no limit) or a positive int32, got {k}")
    return _skeleton_op("skeletonize", a, np.ones((3, 3), np.uint8), k, out)


def neighbor_classes(a: DeviceArray, connectivity: int = 2, out: DeviceArray | None = None) -> DeviceArray:
    """Per pixel of a (H, W) or (N, H, W) uint8 / bool mask: 0 where ``a == 0``, else 1 + the number of set neighbours
    (``connectivity`` 2: the eight neighbours, values 1..9; 1: the four edge neighbours, values 1..5); outside the image
    is background (amt_binary_morph, AMT_MORPH_NEIGHBOR_CLASSES).  On a skeleton with connectivity 2: 1 an isolated
    pixel, 2 an end, 3 a path pixel, 4 and more a junction."""
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (1, 2):
        raise ValueError(f"neighbor_classes: connectivity must be 1 (four neighbours) or 2 (eight), got {connectivity!r}")
    st = cross3() if connectivity == 1 else np.ones((3, 3), np.uint8)
    return _skeleton_op("neighbor_classes", a, st, 0, out)


def label_skeleton_block() -> tuple[int, int, int]:
    """(tile rows, tile words of 64 pixels, sub-iterations per launch) of the label thinning (AMT_LABEL_SKELETON_*), as
    ``skeleton_block`` gives them for the binary one."""
    return _hip.LABEL_SKELETON_TILE_ROWS, _hip.LABEL_SKELETON_TILE_WORDS, _hip.LABEL_SKELETON_BLOCK_SUBITERS


def _label_planes(which: str, labels: DeviceArray):
    """(nplanes, H, W) of the int32 (H, W) or (N, H, W) label planes of a per-cell skeleton op"""
    if labels.dtype != np.int32:
        raise TypeError(f"{which} expects int32 label planes on the device, got {labels.dtype}")
    if labels.ndim not in (2, 3):
        raise ValueError(f"{which} takes (H, W) or (N, H, W) label planes, got shape {labels.shape}")
    return _planes(labels)


def _label_skeleton_op(which: str, labels: DeviceArray, o: DeviceArray, n: int, H: int, W: int, code: int, mode: int):
    """Ops 8 / 9 of amt_rank_filter once everything is checked"""
    st = np.ones((3, 3), np.uint8)
    _hip.check(_lib().amt_rank_filter(labels.ctx.handle, labels.ptr, o.ptr, _hip.I32, n, H, W,
                                      st.ctypes.data_as(ctypes.c_void_p), 3, 3, code, mode, 0.0, None), "amt_rank_filter")
    return o


def label_skeleton(labels: DeviceArray, max_iter: int = 0, out: DeviceArray | None = None) -> DeviceArray:
    """The skeleton of every label of (H, W) or (N, H, W) int32 label planes, touching cells included (amt_rank_filter,
    AMT_RANK_LABEL_SKELETON; include/amt_hip.h states the rule): Zhang and Suen's thinning as in ``skeletonize``, but a
    neighbour counts as set only when it carries the same label as the centre pixel, which gives exactly the union of the
    skeletons each label would get alone in its plane.  Every non-zero value is a label (negative ones too: only
    equality is looked at).  The result holds ``labels[p]`` on the skeleton of p's label and 0 elsewhere.  ``max_iter``:
    at most that many iterations per plane, 0 = until an iteration clears nothing.  Two runs give identical bytes.
    Parity with scikit-image's ``skeletonize`` per label is unpinned offline.  The call waits for the device."""
    if isinstance(max_iter, (bool, np.bool_)):
        raise TypeError("label_skeleton: max_iter must be an integer, got a bool")
    try:
        k = int(operator.index(max_iter))
    except TypeError:
        raise TypeError(f"label_skeleton: max_iter must be an integer, got {type(max_iter).__name__}") from None
    if k < 0 or k > 2**31 - 1:
        raise ValueError(f"label_skeleton: max_iter must be 0 (no limit) or a positive int32, got {k}")
    n, H, W = _label_planes("label_skeleton", labels)
    if out is labels:
        raise ValueError("label_skeleton: out must not alias the input")
    o = _out(labels.ctx, out, labels.shape, np.int32)
    _no_alias("label_skeleton", {"labels": labels}, {"out": o})
    if labels.size == 0:
        return o
    return _label_skeleton_op("label_skeleton", labels, o, n, H, W, _hip.RANK_LABEL_SKELETON, k)


def label_census(labels: DeviceArray, max_label: int, out: DeviceArray | None = None) -> DeviceArray:
    """The census of the same-label pixel graph of (H, W) or (N, H, W) int32 label planes, usually the result of
    ``label_skeleton`` (amt_rank_filter, AMT_RANK_LABEL_CENSUS) -> (N, max_label, 7) int32 in ``_hip.LCEN_COLS`` order,
    row ``l - 1`` for label ``l``.  With deg(p) the number of the eight neighbours carrying p's label: ``pixels``,
    ``isolated`` (deg 0), ``ends`` (deg 1), ``path`` (deg 2), ``junctions`` (deg >= 3; a property of pixels, not of graph
    nodes), ``orth_links`` (horizontally or vertically adjacent pairs) and ``diag_links`` (diagonal pairs that no
    orthogonal pair bridges), so that ``orth_links + sqrt(2) * diag_links`` is the skeleton's length.  Values outside
    1..max_label own no row; a label absent from its plane gives zeros.  Exact integers; two runs give identical bytes."""
    if isinstance(max_label, (bool, np.bool_)):
        raise TypeError("label_census: max_label must be an integer, got a bool")
    try:
        k = int(operator.index(max_label))
    except TypeError:
        raise TypeError(f"label_census: max_label must be an integer, got {type(max_label).__name__}") from None
    if k < 0 or k > 2**31 - 1:
        raise ValueError(f"label_census: max_label must be a non-negative int32, got {k}")
    n, H, W = _label_planes("label_census", labels)
    o = _out(labels.ctx, out, (n, k, _hip.LCEN_NCOLS), np.int32)
    _no_alias("label_census", {"labels": labels}, {"out": o})
    if labels.size == 0 or k == 0:
        if o.nbytes:  # planes without pixels: every label is absent
            _hip.check(_lib().amt_memset(labels.ctx.handle, o.ptr, 0, o.nbytes), "amt_memset")
        return o
    return _label_skeleton_op("label_census", labels, o, n, H, W, _hip.RANK_LABEL_CENSUS, k)


def threshold_otsu_bins(a: DeviceArray, minmax: DeviceArray, thr: DeviceArray, thr_code: DeviceArray,
                        bins: DeviceArray) -> DeviceArray:
    """``threshold_otsu`` of float64 planes whose [min, max] is known, leaving every sample's 256-bin index in the uint8
    plane ``bins`` and the threshold's bin (times two) in ``thr_code``: ``threshold_open_close(a, thr, bins=bins,
    thr_code=thr_code)`` then compares by the byte plane (amt_otsu_f64_bins)."""
    ctx = a.ctx
    n, H, W = _planes(a)
    if a.dtype != np.float64 or bins.dtype != np.uint8 or bins.size != a.size:
        raise ValueError("threshold_otsu_bins: float64 image and a uint8 bin plane of the same size")
    for arr, size in ((minmax, 2 * n), (thr, n), (thr_code, n)):
        if arr.dtype != np.float64 or arr.size != size:
            raise ValueError("threshold_otsu_bins: minmax (n, 2), thr (n,), thr_code (n,) must be float64")
    _no_alias("threshold_otsu_bins", {"a": a, "minmax": minmax}, {"thr": thr, "thr_code": thr_code, "bins": bins})
    _hip.check(_lib().amt_otsu_f64_bins(ctx.handle, a.ptr, minmax.ptr, thr.ptr, thr_code.ptr, bins.ptr, n, H * W),
               "amt_otsu_f64_bins")
    return thr


def threshold_open_close(a: DeviceArray, thr: DeviceArray, footprint=None, out=None, bins=None, thr_code=None) -> DeviceArray:
    """``binary_closing(binary_opening(a > thr[plane], fp), fp)`` as one packed chain (no intermediate masks).
    ``bins`` / ``thr_code`` from ``threshold_otsu_bins``: the comparison reads 1 byte per pixel instead of 8."""
    ctx = a.ctx
    n, H, W = _planes(a)
    fp = _fp(footprint)
    o = _out(ctx, out, a.shape, np.uint8)
    _no_alias("threshold_open_close", {"a": a, "thr": thr, "bins": bins, "thr_code": thr_code}, {"out": o})
    _hip.check(_lib().amt_threshold_open_close(ctx.handle, a.ptr, _in_code(a), thr.ptr, o.ptr, n, H, W,
                                               fp.ctypes.data_as(ctypes.c_void_p), fp.shape[0], fp.shape[1],
                                               None if bins is None else bins.ptr,
                                               None if thr_code is None else thr_code.ptr),
               "amt_threshold_open_close")
    o.is_bool = True
    return o


def _rank(a: DeviceArray, footprint, op: int, mode: str, cval: float, out, minuend: DeviceArray | None = None):
    """The rank filter of ``a``, or ``minuend - filter(a)`` in the same pass when ``minuend`` is given."""
    ctx = a.ctx
    n, H, W = _planes(a)
    fp = _fp(footprint)  # callers that follow scikit-image's even-size rule pass an odd footprint already
    o = _out(ctx, out, a.shape, a.dtype)
    _no_alias("rank filter", {"a": a, "minuend": minuend}, {"out": o})
    _hip.check(_lib().amt_rank_filter(ctx.handle, a.ptr, o.ptr, _in_code(a), n, H, W,
                                      fp.ctypes.data_as(ctypes.c_void_p), fp.shape[0], fp.shape[1], op,
                                      _hip.MODES[mode], float(cval), None if minuend is None else minuend.ptr),
               "amt_rank_filter")
    return o


def erosion(a, footprint=None, out=None, shift: bool = False):
    """``skimage.morphology.erosion`` -> ndi.grey_erosion(footprint), mode 'reflect' (SK/morphology/grey.py:185);
    ``shift`` = scikit-image's shift_x = shift_y (only matters for even-sized footprints)."""
    return _rank(a, _fp(footprint, "skimage-shift" if shift else "skimage"), 0, "reflect", 0.0, out)


def dilation(a, footprint=None, out=None, shift: bool = False):
    """``skimage.morphology.dilation``: skimage mirrors the footprint and scipy mirrors it back
    (SK/morphology/grey.py:242-251), i.e. max over in[p + s] for s in the ORIGINAL (odd-padded) footprint."""
    fp = _fp(footprint, "skimage-shift" if shift else "skimage")
    return _rank(a, np.ascontiguousarray(fp[::-1, ::-1]), 1, "reflect", 0.0, out)


def _eccentric(a, footprint, first, second, out):
    """scikit-image's opening / closing: the second half runs with shift_x = shift_y = True, and for a footprint with an
    even side the image is first edge-padded by (side - 1) pixels along that axis and the result cropped back
    (SK/morphology/grey.py:84-127, :255-353)."""
    shape = (3, 3) if footprint is None else np.shape(footprint)
    py = shape[0] - 1 if shape[0] % 2 == 0 else 0
    px = shape[1] - 1 if shape[1] % 2 == 0 else 0
    if not (py or px):
        return second(first(a, footprint), footprint, out=out, shift=True)
    H, W = a.shape[-2:]
    res = second(first(pad_edge(a, py, px), footprint), footprint, shift=True)
    return crop(res, py, px, H, W, out=out)


def opening(a, footprint=None, out=None):
    """``skimage.morphology.opening`` = dilation(erosion(a), shift_x=True, shift_y=True) (SK/morphology/grey.py:255-303)."""
    return _eccentric(a, footprint, erosion, dilation, out)


def closing(a, footprint=None, out=None):
    """``skimage.morphology.closing`` = erosion(dilation(a), shift_x=True, shift_y=True) (SK/morphology/grey.py:305-353)."""
    return _eccentric(a, footprint, dilation, erosion, out)


def white_tophat(a, footprint=None, out=None):
    """``skimage.morphology.white_tophat`` -> ndi.white_tophat = a - grey_opening(a) with scipy's own
    opening (grey_erosion then grey_dilation, both with the footprint as given; SK/morphology/grey.py:425)."""
    fp = _fp(footprint)
    er = _rank(a, fp, 0, "reflect", 0.0, None)
    # the dilation stores image - dilation(erosion) directly
    return _rank(er, fp, 1, "reflect", 0.0, out, minuend=a)


def median(a, footprint=None, mode: str = "nearest", cval: float = 0.0, out=None):
    """``skimage.filters.median`` -> ndi.median_filter(footprint, mode='nearest') (SK/filters/_median.py)."""
    fp = np.ones((3, 3), dtype=np.uint8) if footprint is None else footprint
    return _rank(a, fp, 2, mode, cval, out)


# ---- Z-stacks (amt_rank_filter ops 10 .. 14; include/amt_hip.h states the definitions) ------------------------------
def zstack_tile() -> tuple[int, int]:
    """(rows, columns) of the output tile one workgroup of the focus kernel owns (AMT_ZSTACK_TILE_*): planes larger than
    this cross tile seams."""
    return _hip.ZSTACK_TILE


_Z_CODES = {np.dtype(np.uint8): _hip.U8, np.dtype(np.uint16): _hip.U16, np.dtype(np.float64): _hip.F64}


def _zstack(op: str, stack, integer_only: bool = False):
    """(code, N, Z, H, W) of an (N, Z, H, W) stack batch, refused before any device access"""
    if not isinstance(stack, DeviceArray):
        raise ValueError(f"{op}: stack must be a DeviceArray, got {type(stack).__name__}")
    if stack.ndim != 4:
        raise ValueError(f"{op} takes (N, Z, H, W) stacks, got shape {stack.shape}")
    if stack.dtype not in _Z_CODES or (integer_only and stack.dtype == np.float64):
        want = "uint8 or uint16 (focus is judged on raw data)" if integer_only else "uint8, uint16 or float64"
        raise ValueError(f"{op}: stacks must be {want}, got {stack.dtype}")
    N, Z, H, W = stack.shape
    if not 1 <= Z <= 65535:
        raise ValueError(f"{op}: Z must be in 1..65535, got {Z}")
    if H < 1 or W < 1 or H * W >= 2**31:
        raise ValueError(f"{op}: planes must have 1 <= H * W < 2^31 pixels, got {H} x {W}")
    return _Z_CODES[stack.dtype], int(N), int(Z), int(H), int(W)


def _zstack_radius(op: str, radius) -> int:
    if isinstance(radius, (bool, np.bool_)):
        raise ValueError(f"{op}: radius must be an integer in 0..{_hip.ZSTACK_MAX_RADIUS}, got a bool")
    try:
        r = int(operator.index(radius))
    except TypeError:
        raise ValueError(f"{op}: radius must be an integer in 0..{_hip.ZSTACK_MAX_RADIUS}, got {radius!r}") from None
    if not 0 <= r <= _hip.ZSTACK_MAX_RADIUS:
        raise ValueError(f"{op}: radius must be in 0..{_hip.ZSTACK_MAX_RADIUS}, got {r}")
    return r


def _zstack_call(stack, o, code, N, Z, H, W, fp, op, cval=0.0, minuend=None):
    if N == 0:
        return o
    fh = int(fp.shape[0])
    _hip.check(_lib().amt_rank_filter(stack.ctx.handle, stack.ptr, o.ptr, code, N, H, W, fp.ctypes.data_as(ctypes.c_void_p),
                                      fh, fh, op, Z, float(cval), None if minuend is None else minuend.ptr), "amt_rank_filter")
    return o


def z_project(stack: DeviceArray, method: str = "max", out: DeviceArray | None = None) -> DeviceArray:
    """The projection of every (Z, H, W) stack of an (N, Z, H, W) uint8 / uint16 / float64 batch along z -> (N, H, W)
    (amt_rank_filter, AMT_RANK_Z_PROJECT).  ``method``: "max" and "min" keep the dtype; "mean" gives float64, the sum over
    z = 0, 1, ... divided once by Z.  All three equal numpy's ``max`` / ``min`` / ``mean(axis=0)`` bit for bit (NaN is
    unsupported)."""
    if method not in _hip.Z_PROJECT_METHODS:
        raise ValueError(f"z_project: method must be 'max', 'min' or 'mean', got {method!r}")
    code, N, Z, H, W = _zstack("z_project", stack)
    o = _out(stack.ctx, out, (N, H, W), np.float64 if method == "mean" else stack.dtype)
    _no_alias("z_project", {"stack": stack}, {"out": o})
    return _zstack_call(stack, o, code, N, Z, H, W, np.ones((1, 1), np.uint8), _hip.RANK_Z_PROJECT,
                        _hip.Z_PROJECT_METHODS[method])


def focus_sums(stack: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    """Four exact integer sums per plane of an (N, Z, H, W) uint8 / uint16 batch -> (N, Z, 4) int64 in ``_hip.ZF_COLS``
    order (amt_rank_filter, AMT_RANK_Z_FOCUS_SUMS): the sum of the plane, of its squares, of the squared Laplacian (four
    neighbours, edge replication) and Brenner's sum of (P(y, x + 2) - P(y, x))^2.  H * W <= 2^27."""
    code, N, Z, H, W = _zstack("focus_sums", stack, integer_only=True)
    if H * W > 2**27:
        raise ValueError(f"focus_sums: H * W must not exceed 2^27, got {H} x {W}")
    o = _out(stack.ctx, out, (N, Z, _hip.ZF_NCOLS), np.int64)
    _no_alias("focus_sums", {"stack": stack}, {"out": o})
    return _zstack_call(stack, o, code, N, Z, H, W, np.ones((1, 1), np.uint8), _hip.RANK_Z_FOCUS_SUMS)


def focus_index(stack: DeviceArray, radius: int = 4, out: DeviceArray | None = None) -> DeviceArray:
    """Per pixel of every stack of an (N, Z, H, W) uint8 / uint16 batch, the plane in best focus -> (N, H, W) uint16
    (amt_rank_filter, AMT_RANK_Z_FOCUS_INDEX): the smallest z at which the sum of the squared Laplacian over the
    (2 radius + 1)^2 window, clipped to the image, is largest.  Exact 64-bit integers: two runs give identical bytes.
    ``radius`` in 0..15.  The rule is this package's own (include/amt_hip.h states it)."""
    r = _zstack_radius("focus_index", radius)
    code, N, Z, H, W = _zstack("focus_index", stack, integer_only=True)
    o = _out(stack.ctx, out, (N, H, W), np.uint16)
    _no_alias("focus_index", {"stack": stack}, {"out": o})
    return _zstack_call(stack, o, code, N, Z, H, W, np.ones((2 * r + 1, 2 * r + 1), np.uint8), _hip.RANK_Z_FOCUS_INDEX)


def focus_stack(stack: DeviceArray, radius: int = 4, out: DeviceArray | None = None) -> DeviceArray:
    """The all-in-focus composite of every stack of an (N, Z, H, W) uint8 / uint16 batch -> (N, H, W) of the same dtype
    (amt_rank_filter, AMT_RANK_Z_FOCUS_STACK): ``stack[focus_index(stack, radius)[y, x], y, x]`` in one pass, without
    the index map in memory."""
    r = _zstack_radius("focus_stack", radius)
    code, N, Z, H, W = _zstack("focus_stack", stack, integer_only=True)
    o = _out(stack.ctx, out, (N, H, W), stack.dtype)
    _no_alias("focus_stack", {"stack": stack}, {"out": o})
    return _zstack_call(stack, o, code, N, Z, H, W, np.ones((2 * r + 1, 2 * r + 1), np.uint8), _hip.RANK_Z_FOCUS_STACK)


def z_take(stack: DeviceArray, index: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    """``stack[n, min(index[n, y, x], Z - 1), y, x]`` of an (N, Z, H, W) uint8 / uint16 / float64 batch and an (N, H, W)
    uint16 index map -> (N, H, W) of the stack's dtype (amt_rank_filter, AMT_RANK_Z_TAKE).  An index past the stack is
    clamped."""
    code, N, Z, H, W = _zstack("z_take", stack)
    if not isinstance(index, DeviceArray) or tuple(index.shape) != (N, H, W) or index.dtype != np.uint16:
        raise ValueError(f"z_take: index must be a uint16 DeviceArray of shape {(N, H, W)}, got "
                         f"{getattr(index, 'shape', None)} {getattr(index, 'dtype', type(index).__name__)}")
    if index.ctx is not stack.ctx:
        raise ValueError("z_take: stack and index belong to different contexts")
    o = _out(stack.ctx, out, (N, H, W), stack.dtype)
    _no_alias("z_take", {"stack": stack, "index": index}, {"out": o})
    return _zstack_call(stack, o, code, N, Z, H, W, np.ones((1, 1), np.uint8), _hip.RANK_Z_TAKE, minuend=index)


# ---- spot detection (amt_rank_filter ops 15 .. 18; include/amt_hip.h states the rules) ------------------------------
def spot_tile() -> tuple[int, int]:
    """(rows, columns) of the output tile one workgroup of the local-maximum kernel owns (AMT_SPOT_TILE_*)."""
    return _hip.SPOT_TILE


def _spot_int(op: str, name: str, value, lo: int, hi: int | None) -> int:
    rng = f"{lo}..{hi}" if hi is not None else f"at least {lo}"
    if isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{op}: {name} must be an integer ({rng}), got a bool")
    try:
        v = int(operator.index(value))
    except TypeError:
        raise ValueError(f"{op}: {name} must be an integer ({rng}), got {value!r}") from None
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"{op}: {name} must be {rng}, got {v}")
    return v


def spot_capacity(H: int, W: int, min_distance: int = 1) -> int:
    """The most marks ``local_maxima`` can leave in an H x W plane: marks are more than ``min_distance`` apart
    (Chebyshev), so ceil(H / (min_distance + 1)) * ceil(W / (min_distance + 1))."""
    r = _spot_int("spot_capacity", "min_distance", min_distance, 1, _hip.SPOT_MAX_RADIUS)
    H, W = _spot_int("spot_capacity", "H", H, 1, None), _spot_int("spot_capacity", "W", W, 1, None)
    return -(-H // (r + 1)) * -(-W // (r + 1))


def _spot_planes(op: str, a, dtypes, name: str = "a"):
    """(N, H, W) of an (N, H, W) batch, refused before any device access"""
    if not isinstance(a, DeviceArray):
        raise ValueError(f"{op}: {name} must be a DeviceArray, got {type(a).__name__}")
    if a.ndim != 3:
        raise ValueError(f"{op} takes (N, H, W) batches, got shape {a.shape} for {name}")
    if a.dtype not in [np.dtype(d) for d in dtypes]:
        raise ValueError(f"{op}: {name} must be {' or '.join(np.dtype(d).name for d in dtypes)}, got {a.dtype}")
    N, H, W = (int(v) for v in a.shape)
    if H < 1 or W < 1 or H * W >= 2**31:
        raise ValueError(f"{op}: planes must have 1 <= H * W < 2^31 pixels, got {H} x {W}")
    return N, H, W


def _spot_list(op: str, spots, N: int, ctx) -> int:
    """the capacity of an (N, capacity + 1) int32 list of spots as ``mask_list`` writes it"""
    if not isinstance(spots, DeviceArray) or spots.ndim != 2 or spots.dtype != np.int32 or spots.shape[0] != N \
            or spots.shape[1] < 2:
        raise ValueError(f"{op}: spots must be an int32 DeviceArray of shape ({N}, capacity + 1) as mask_list writes it, got "
                         f"{getattr(spots, 'shape', None)} {getattr(spots, 'dtype', type(spots).__name__)}")
    if spots.ctx is not ctx:
        raise ValueError(f"{op}: the image and spots belong to different contexts")
    return int(spots.shape[1]) - 1


_SPOT_CODES = {np.dtype(np.uint8): _hip.U8, np.dtype(np.uint16): _hip.U16, np.dtype(np.int32): _hip.I32,
               np.dtype(np.float64): _hip.F64}
_ONE = np.ones((1, 1), np.uint8)


def _spot_call(a, o, N, H, W, fp, op, mode, cval=0.0, minuend=None):
    if N == 0:
        return o
    fh = int(fp.shape[0])
    _hip.check(_lib().amt_rank_filter(a.ctx.handle, a.ptr, o.ptr, _SPOT_CODES[a.dtype], N, H, W,
                                      fp.ctypes.data_as(ctypes.c_void_p), fh, fh, op, int(mode), float(cval),
                                      None if minuend is None else minuend.ptr), "amt_rank_filter")
    return o


def local_maxima(a: DeviceArray, min_distance: int = 1, threshold=0.0, exclude_border: int = 0,
                 out: DeviceArray | None = None) -> DeviceArray:
    """The local maxima of every plane of an (N, H, W) uint16 / float64 batch -> (N, H, W) uint8 0 / 1 with ``is_bool``
    set (amt_rank_filter, AMT_RANK_LOCAL_MAXIMA).  A pixel is marked iff it exceeds ``threshold`` (a number, or an (N,)
    float64 DeviceArray with one threshold per plane), is >= every pixel within ``min_distance`` (Chebyshev) and > those
    of them that precede it in raster order, and lies at least ``exclude_border`` pixels from every edge.  Marks are more
    than ``min_distance`` apart; a plateau yields one mark, at its first pixel.  The rule is this package's own
    (include/amt_hip.h states it); NaN is unsupported."""
    r = _spot_int("local_maxima", "min_distance", min_distance, 1, _hip.SPOT_MAX_RADIUS)
    b = _spot_int("local_maxima", "exclude_border", exclude_border, 0, 2**31 - 1)
    per_plane = isinstance(threshold, DeviceArray)
    if not per_plane:
        try:
            t = float(threshold)
        except (TypeError, ValueError):
            raise ValueError(f"local_maxima: threshold must be a number or an (N,) float64 DeviceArray, got {threshold!r}") from None
        if np.isnan(t):
            raise ValueError("local_maxima: threshold must not be NaN")
    N, H, W = _spot_planes("local_maxima", a, (np.uint16, np.float64))
    if per_plane:
        if tuple(threshold.shape) != (N,) or threshold.dtype != np.float64:
            raise ValueError(f"local_maxima: per-plane thresholds must be float64 of shape ({N},), got {threshold.shape} "
                             f"{threshold.dtype}")
        if threshold.ctx is not a.ctx:
            raise ValueError("local_maxima: the image and threshold belong to different contexts")
    o = _out(a.ctx, out, (N, H, W), np.uint8)
    _no_alias("local_maxima", {"a": a, "threshold": threshold if per_plane else None}, {"out": o})
    o.is_bool = True
    return _spot_call(a, o, N, H, W, np.ones((2 * r + 1, 2 * r + 1), np.uint8), _hip.RANK_LOCAL_MAXIMA, b,
                      0.0 if per_plane else t, threshold if per_plane else None)


def mask_list(mask: DeviceArray, capacity: int | None = None, out: DeviceArray | None = None) -> DeviceArray:
    """``np.flatnonzero`` of every plane of an (N, H, W) uint8 mask batch, truncated -> (N, capacity + 1) int32
    (amt_rank_filter, AMT_RANK_MASK_LIST): column 0 the true number of set pixels (also when it exceeds ``capacity``),
    then their raster indices y * W + x ascending, then -1.  ``capacity`` defaults to H * W."""
    if capacity is not None:
        capacity = _spot_int("mask_list", "capacity", capacity, 1, 2**31 - 2)
    N, H, W = _spot_planes("mask_list", mask, (np.uint8,), "mask")
    cap = H * W if capacity is None else capacity
    o = _out(mask.ctx, out, (N, cap + 1), np.int32)
    _no_alias("mask_list", {"mask": mask}, {"out": o})
    return _spot_call(mask, o, N, H, W, _ONE, _hip.RANK_MASK_LIST, cap)


def spot_measure(a: DeviceArray, spots: DeviceArray, radius: int = 2, out: DeviceArray | None = None) -> DeviceArray:
    """One row per entry of a list of spots (as ``mask_list`` writes it) on an (N, H, W) uint16 / float64 batch ->
    (N, capacity, 7) float64 in ``_hip.SPOT_COLS`` order (amt_rank_filter, AMT_RANK_SPOT_MEASURE): the value, the
    sub-pixel offsets (dy, dx) of the parabola through three samples per axis (0 on the image's edge and where the
    samples are not concave, clamped to +-0.5), sum and count over the (2 radius + 1)^2 window and over the frame at
    distance radius + 1 .. radius + 2, both clipped to the image.  Rows past the count are NaN."""
    k = _spot_int("spot_measure", "radius", radius, 0, _hip.SPOT_MAX_RADIUS)
    N, H, W = _spot_planes("spot_measure", a, (np.uint16, np.float64))
    cap = _spot_list("spot_measure", spots, N, a.ctx)
    o = _out(a.ctx, out, (N, cap, _hip.SPOT_NCOLS), np.float64)
    _no_alias("spot_measure", {"a": a, "spots": spots}, {"out": o})
    return _spot_call(a, o, N, H, W, np.ones((2 * k + 1, 2 * k + 1), np.uint8), _hip.RANK_SPOT_MEASURE, cap, minuend=spots)


def take_at(a: DeviceArray, spots: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    """The values of an (N, H, W) uint8 / uint16 / int32 / float64 batch at the entries of a list of spots ->
    (N, capacity) of the same dtype, 0 past the count (amt_rank_filter, AMT_RANK_TAKE_AT)."""
    N, H, W = _spot_planes("take_at", a, (np.uint8, np.uint16, np.int32, np.float64))
    cap = _spot_list("take_at", spots, N, a.ctx)
    o = _out(a.ctx, out, (N, cap), a.dtype)
    _no_alias("take_at", {"a": a, "spots": spots}, {"out": o})
    return _spot_call(a, o, N, H, W, _ONE, _hip.RANK_TAKE_AT, cap, minuend=spots)


# ---- grey reconstruction (amt_rank_filter ops 3 .. 6; include/amt_hip.h states the definitions) --------------------
def reconstruct_tile(dtype) -> tuple[int, int]:
    """(rows, columns) of the tile one workgroup of the reconstruction kernel owns (AMT_RECONSTRUCT_TILE_*): planes
    larger than this cross tile seams and take several rounds."""
    dt = np.dtype(dtype)
    if dt == np.uint16:
        return _hip.RECONSTRUCT_TILE_U16
    if dt == np.float64:
        return _hip.RECONSTRUCT_TILE_F64
    raise TypeError(f"reconstruction runs on uint16 or float64 images, got {dt}")


def _recon_footprint(footprint) -> np.ndarray:
    """None (scikit-image's default, 3 x 3 all-ones), the 3 x 3 cross or 3 x 3 all-ones -> uint8 (3, 3)."""
    if footprint is None:
        return np.ones((3, 3), np.uint8)
    fp = np.ascontiguousarray(np.asarray(footprint) != 0, dtype=np.uint8)
    if fp.shape != (3, 3) or not (np.array_equal(fp, cross3()) or fp.all()):
        raise ValueError("reconstruction: footprint must be None, the 3 x 3 cross (4-connected) or 3 x 3 all-ones "
                         "(8-connected)")
    return fp


def _recon_method(method: str) -> bool:
    if method not in ("dilation", "erosion"):
        raise ValueError(f"Reconstruction method can be one of 'erosion' or 'dilation'. Got '{method}'.")
    return method == "dilation"


def _recon_image(op: str, a: DeviceArray, what: str = "image"):
    if a.dtype not in (np.uint16, np.float64):
        raise TypeError(f"{op}: the {what} must be uint16 or float64 on the device, got {a.dtype}")
    if a.ndim not in (2, 3):
        raise ValueError(f"{op} takes (H, W) or (N, H, W) images, got shape {a.shape}")


def _recon_h(op: str, dtype, h) -> float:
    """``h`` as the C ABI takes it: an integer in 1..65535 for uint16 images, finite and > 0 for float64."""
    if isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, float, np.integer, np.floating)):
        raise ValueError(f"{op}: h must be a number, got {h!r}")
    hf = float(h)
    if not np.isfinite(hf) or hf <= 0:
        raise ValueError(f"{op}: h must be finite and > 0, got {h!r}")
    if np.dtype(dtype) == np.uint16 and (hf != int(hf) or hf > 65535):
        raise ValueError(f"{op}: h of an integer image must be an integer in 1..65535, got {h!r}")
    return hf


def _recon_call(op: str, a: DeviceArray, o: DeviceArray, fp: np.ndarray, code: int, h: float, second):
    n, H, W = _planes(a)
    if a.size == 0:
        return o
    _hip.check(_lib().amt_rank_filter(a.ctx.handle, a.ptr, o.ptr, _in_code(a), n, H, W, fp.ctypes.data_as(ctypes.c_void_p),
                                      3, 3, code, _hip.MODE_CONSTANT, float(h), None if second is None else second.ptr),
               "amt_rank_filter")
    return o


def reconstruction(seed: DeviceArray, mask: DeviceArray, method: str = "dilation", footprint=None,
                   out: DeviceArray | None = None) -> DeviceArray:
    """``skimage.morphology.reconstruction(seed, mask, method, footprint)`` per plane of (H, W) or (N, H, W) uint16 or
    float64 images: by dilation the least image R >= seed with R = min(mask, max over the footprint of R), by erosion
    the dual.  ``footprint``: None (3 x 3 all-ones, scikit-image's default), the cross or all-ones.  ``seed`` above
    (below) ``mask`` anywhere raises ValueError.  The call waits for the device (amt_rank_filter,
    AMT_RANK_RECONSTRUCT_DILATION / _EROSION)."""
    dil = _recon_method(method)
    fp = _recon_footprint(footprint)
    _recon_image("reconstruction", seed, "seed")
    _recon_image("reconstruction", mask, "mask")
    if seed.dtype != mask.dtype or tuple(seed.shape) != tuple(mask.shape):
        raise ValueError(f"reconstruction: seed ({seed.shape} {seed.dtype}) and mask ({mask.shape} {mask.dtype}) must have "
                         "the same shape and dtype")
    if mask.ctx is not seed.ctx:
        raise ValueError("reconstruction: seed and mask belong to different contexts")
    o = _out(seed.ctx, out, seed.shape, seed.dtype)
    _no_alias("reconstruction", {"seed": seed, "mask": mask}, {"out": o})
    return _recon_call("reconstruction", seed, o, fp,
                       _hip.RANK_RECONSTRUCT_DILATION if dil else _hip.RANK_RECONSTRUCT_EROSION, 0.0, mask)


def h_reconstruction(a: DeviceArray, h, method: str = "dilation", footprint=None, out: DeviceArray | None = None,
                     minuend: DeviceArray | None = None) -> DeviceArray:
    """The reconstruction behind h-maxima / h-minima, with ``a`` as the mask and a seed that is never in memory:
    ``method="dilation"`` reconstructs ``max(a - h, 0)`` (uint16) / ``a - h`` (float64) under ``a``, ``"erosion"``
    ``min(a + h, 65535)`` / ``a + h`` over ``a``.  ``minuend`` (dilation only) stores ``minuend - R`` instead:
    ``minuend=a`` is the h-dome.  ``h``: an integer in 1..65535 for uint16, finite and > 0 for float64."""
    dil = _recon_method(method)
    fp = _recon_footprint(footprint)
    _recon_image("h_reconstruction", a)
    hf = _recon_h("h_reconstruction", a.dtype, h)
    if minuend is not None:
        if not dil:
            raise ValueError("h_reconstruction: minuend goes with method='dilation' only")
        if minuend.dtype != a.dtype or tuple(minuend.shape) != tuple(a.shape):
            raise ValueError("h_reconstruction: minuend must have the image's shape and dtype")
    o = _out(a.ctx, out, a.shape, a.dtype)
    _no_alias("h_reconstruction", {"a": a, "minuend": minuend}, {"out": o})
    return _recon_call("h_reconstruction", a, o, fp, _hip.RANK_HMAX_RECONSTRUCT if dil else _hip.RANK_HMIN_RECONSTRUCT,
                       hf, minuend)


def _h_extrema(op: str, a: DeviceArray, h, footprint, out, maxima: bool) -> DeviceArray:
    fp = _recon_footprint(footprint)
    _recon_image(op, a)
    hf = _recon_h(op, a.dtype, h)
    ctx = a.ctx
    n, H, W = _planes(a)
    o = _out(ctx, out, a.shape, np.uint8)
    _no_alias(op, {"a": a}, {"out": o})
    o.is_bool = True
    if a.size == 0:
        return o
    lib = _lib()
    code = _in_code(a)
    if a.dtype == np.uint16:
        # residue >= h  <=>  residue > h - 1 (integers)
        if maxima:
            res = h_reconstruction(a, hf, "dilation", fp, minuend=a)  # a - R
        else:
            res = h_reconstruction(a, hf, "erosion", fp)
            _hip.check(lib.amt_subtract(ctx.handle, res.ptr, a.ptr, res.ptr, code, a.size), "amt_subtract")  # R - a
        thr = ctx.asarray(np.full(n, hf - 1.0))
    else:
        # R == seed exactly  <=>  seed - R (maxima: <= 0) resp. R - seed (minima: <= 0) is zero  <=>  it is above the
        # largest negative double
        seed = add_scalar(a, -hf if maxima else hf)
        r = reconstruction(seed, a, "dilation" if maxima else "erosion", fp)
        first, second = (seed, r) if maxima else (r, seed)
        _hip.check(lib.amt_subtract(ctx.handle, first.ptr, second.ptr, r.ptr, code, a.size), "amt_subtract")
        res = r
        thr = ctx.asarray(np.full(n, -np.nextafter(0.0, 1.0)))
    _hip.check(lib.amt_threshold_gt(ctx.handle, res.ptr, code, thr.ptr, o.ptr, n, H * W), "amt_threshold_gt")
    return o


def h_maxima(a: DeviceArray, h, footprint=None, out: DeviceArray | None = None) -> DeviceArray:
    """``skimage.morphology.h_maxima(a, h, footprint)`` per plane -> uint8 0 / 1 (``is_bool``): the maxima whose height
    over their surroundings is at least ``h``.  uint16: a pixel is marked iff ``a - R >= h`` with R the reconstruction by
    dilation of ``max(a - h, 0)`` under ``a`` (scikit-image's rule).  float64 (finite values): iff ``R == seed`` exactly,
    with ``seed = a - h`` as rounded -- the same set in exact arithmetic, and no tolerance is involved.  The early exit
    of scikit-image for ``h`` above the image's range is the caller's (``operations.h_maxima`` makes it)."""
    return _h_extrema("h_maxima", a, h, footprint, out, True)


def h_minima(a: DeviceArray, h, footprint=None, out: DeviceArray | None = None) -> DeviceArray:
    """``skimage.morphology.h_minima``: the dual of ``h_maxima`` (reconstruction by erosion of ``min(a + h, 65535)`` /
    ``a + h`` over ``a``; uint16 marks ``R - a >= h``, float64 ``R == seed``)."""
    return _h_extrema("h_minima", a, h, footprint, out, False)


# --------------------------------------------------------------------------------------------------
# labelling
# --------------------------------------------------------------------------------------------------
def label(a: DeviceArray, connectivity: int = 2, out: DeviceArray | None = None, count: DeviceArray | None = None):
    """``skimage.measure.label`` per plane (default 8-connected; raster numbering) -> (int32 labels, counts).
    R/masks.py:63; SURVEY.md A.5."""
    ctx = a.ctx
    n, H, W = _planes(a)
    if a.dtype == np.uint8:
        code = _hip.U8
    elif a.dtype == np.int32:
        code = _hip.I32
    else:
        raise TypeError(f"label: unsupported dtype {a.dtype}")
    o = _out(ctx, out, a.shape, np.int32)
    c = _out(ctx, count, (n,), np.int32)
    _no_alias("label", {"a": a}, {"out": o, "count": c})
    if code == _hip.U8 and a.is_bool:
        # a bool array (0 / 1 bytes by construction): the truth-value entry point, whose run-table path launches nothing
        # that stands by for other byte values
        _hip.check(_lib().amt_label_mask(ctx.handle, a.ptr, o.ptr, c.ptr, n, H, W, int(connectivity)), "amt_label_mask")
        return o, c
    _hip.check(_lib().amt_label(ctx.handle, a.ptr, code, o.ptr, c.ptr, n, H, W, int(connectivity)), "amt_label")
    return o, c


def label_sparse_capacity(H: int, W: int) -> int:
    return max(65536, (H * W) // 16)


def label_sparse(a: DeviceArray, connectivity: int = 2, capacity: int | None = None, out=None, count=None, keep=None):
    """``label`` for sparse uint8 masks (at most ``capacity`` foreground pixels per plane, default max(65536,
    plane size / 16)); a plane that overflows reports count -1.

    ``keep`` = (int32 (n, capacity) list, int32 (n,) counts), both owned by the caller, turns the full-plane clear of
    ``out`` into a clear of the pixels the previous call wrote: ``out`` must then be the same array every time, zeroed
    once together with the counts."""
    ctx = a.ctx
    n, H, W = _planes(a)
    if a.dtype != np.uint8:
        raise TypeError("label_sparse expects a uint8 / bool mask")
    if capacity is None:
        capacity = label_sparse_capacity(H, W)
    o = _out(ctx, out, a.shape, np.int32)
    c = _out(ctx, count, (n,), np.int32)
    klist_ptr = kcount_ptr = None
    if keep is not None:
        klist, kcount = keep
        if out is None:
            raise ValueError("keep= needs the caller's persistent out= plane")
        if klist.dtype != np.int32 or klist.size != n * int(capacity) or kcount.dtype != np.int32 or kcount.size != n:
            raise ValueError("keep must be (int32 (n, capacity), int32 (n,))")
        klist_ptr, kcount_ptr = klist.ptr, kcount.ptr
    _no_alias("label_sparse", {"a": a}, {"out": o, "count": c, "keep list": keep and keep[0], "keep counts": keep and keep[1]})
    _hip.check(_lib().amt_label_sparse(ctx.handle, a.ptr, o.ptr, c.ptr, n, H, W, int(connectivity), int(capacity),
                                       klist_ptr, kcount_ptr), "amt_label_sparse")
    return o, c


def clear_border(labels: DeviceArray, out: DeviceArray | None = None) -> DeviceArray:
    """``skimage.segmentation.clear_border`` (buffer_size 0) per plane (R/masks.py:56)."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    if labels.dtype != np.int32:
        raise TypeError("clear_border expects int32 labels on the device")
    o = _out(ctx, out, labels.shape, np.int32)
    _no_alias("clear_border", {"labels": labels}, {"out": o}, inplace={("out", "labels")})
    _hip.check(_lib().amt_clear_border(ctx.handle, labels.ptr, o.ptr, n, H, W), "amt_clear_border")
    return o


def relabel_sequential(labels: DeviceArray, max_label: int, out=None, count=None):
    """``skimage.segmentation.relabel_sequential`` per plane -> (labels, counts) (R/masks.py:65)."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    o = _out(ctx, out, labels.shape, np.int32)
    c = _out(ctx, count, (n,), np.int32)
    _no_alias("relabel_sequential", {"labels": labels}, {"out": o, "count": c}, inplace={("out", "labels")})
    _hip.check(_lib().amt_relabel_sequential(ctx.handle, labels.ptr, o.ptr, c.ptr, n, H * W, int(max_label)),
               "amt_relabel_sequential")
    return o, c


def clear_border_relabel(labels: DeviceArray, max_label: int, out=None, count=None, nlabels: DeviceArray | None = None):
    """``relabel_sequential(clear_border(labels))`` in one pass (R/masks.py:56,65) for label images whose
    labels are each one connected component (outputs of ``label`` / ``watershed``).  ``nlabels`` (int32 per
    plane, on the device): the caller vouches that each plane holds exactly the labels 1..nlabels[plane], which
    spares the pass that looks for the labels present."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    o = _out(ctx, out, labels.shape, np.int32)
    c = _out(ctx, count, (n,), np.int32)
    if nlabels is not None and (nlabels.dtype != np.int32 or nlabels.size != n):
        raise ValueError("nlabels must hold one int32 per plane")
    _no_alias("clear_border_relabel", {"labels": labels, "nlabels": nlabels}, {"out": o, "count": c}, inplace={("out", "labels")})
    _hip.check(_lib().amt_clear_border_relabel(ctx.handle, labels.ptr, o.ptr, c.ptr, n, H, W, int(max_label),
                                               nlabels.ptr if nlabels is not None else None),
               "amt_clear_border_relabel")
    return o, c


def keep_labels(labels: DeviceArray, keep: DeviceArray, max_label: int, out=None) -> DeviceArray:
    """``np.where(np.isin(labels, kept), labels, 0)`` with keep = (nplanes, max_label+1) uint8 (R/masks.py:399-403)."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    o = _out(ctx, out, labels.shape, np.int32)
    _no_alias("keep_labels", {"labels": labels, "keep": keep}, {"out": o}, inplace={("out", "labels")})
    _hip.check(_lib().amt_keep_labels(ctx.handle, labels.ptr, keep.ptr, o.ptr, n, H * W, int(max_label)),
               "amt_keep_labels")
    return o


def to_int64(labels: DeviceArray, out=None) -> DeviceArray:
    o = _out(labels.ctx, out, labels.shape, np.int64)
    _no_alias("to_int64", {"labels": labels}, {"out": o})
    _hip.check(_lib().amt_cast_i32_i64(labels.ctx.handle, labels.ptr, o.ptr, labels.size), "amt_cast_i32_i64")
    return o


def max_per_plane(labels: DeviceArray, out=None) -> DeviceArray:
    ctx = labels.ctx
    n, H, W = _planes(labels)
    o = _out(ctx, out, (n,), np.int32)
    _no_alias("max_per_plane", {"labels": labels}, {"out": o})
    _hip.check(_lib().amt_max_i32(ctx.handle, labels.ptr, o.ptr, n, H * W), "amt_max_i32")
    return o


def cast_labels(labels: DeviceArray, dtype, out=None) -> DeviceArray:
    """Label planes between uint8 / uint16 and the int32 the label kernels take (values copied; narrowing is the
    caller's promise that they fit)."""
    o = _out(labels.ctx, out, labels.shape, dtype)
    pair = (labels.dtype, o.dtype)
    if np.dtype(np.int32) not in pair or not all(d in (np.uint8, np.uint16, np.int32) for d in pair) or pair[0] == pair[1]:
        raise TypeError(f"cast_labels converts uint8 / uint16 to int32 and back, not {pair[0]} to {pair[1]}")
    codes = {np.dtype(np.uint8): _hip.U8, np.dtype(np.uint16): _hip.U16, np.dtype(np.int32): _hip.I32}
    _no_alias("cast_labels", {"labels": labels}, {"out": o})
    _hip.check(_lib().amt_cast_labels(labels.ctx.handle, labels.ptr, codes[pair[0]], o.ptr, codes[pair[1]], labels.size),
               "amt_cast_labels")
    return o


def expand_nmax(distance: float) -> int:
    """The integer bound of ``expand_labels``: the largest n with ``np.sqrt(np.float64(n)) <= distance`` (-1 when there
    is none, i.e. ``distance < 0`` or NaN), so that ``D2 <= nmax`` on exact integer squared distances is scikit-image's
    ``distances <= distance`` on their float64 square roots.  ``floor(distance**2)`` is off by at most one."""
    d = float(distance)
    if not d >= 0.0:
        return -1
    if d >= 2.0 ** 31:  # beyond any squared distance on a plane the device takes (sides <= 32768)
        return 2 ** 62
    n = int(np.floor(d * d))
    while n > 0 and not np.sqrt(np.float64(n)) <= d:
        n -= 1
    while np.sqrt(np.float64(n + 1)) <= d:
        n += 1
    return n


def expand_labels(labels: DeviceArray, distance: float, ring: bool = False, out=None) -> DeviceArray:
    """``skimage.segmentation.expand_labels(labels, distance)`` per plane (SK/segmentation/_expand_labels.py): every
    label grows by up to ``distance`` pixels into the background without overlapping its neighbours.  ``labels`` is an
    int32 (H, W) or (N, H, W) array of non-negative labels; the planes are independent.

    A background pixel is labelled iff the float64 square root of its exact squared distance to the nearest labelled
    pixel is ``<= distance`` (any float distance: the bound is turned into an integer by ``expand_nmax``), with the
    label of that nearest pixel.  Where pixels of several labels are equally near, the SMALLEST label is written:
    scipy's feature transform picks whichever tied pixel its scan meets first, which is an artefact of its algorithm;
    this rule is deterministic and independent of tiling, plane size and batch position.  The support and every
    untied pixel equal scikit-image's.  ``distance < 0`` gives zeros, as that expression does.

    ``ring=True`` writes 0 inside the input's labels: the annulus each label gains."""
    ctx = labels.ctx
    if labels.ndim not in (2, 3):
        raise ValueError(f"expand_labels expects an (H, W) or (N, H, W) array, got shape {labels.shape}")
    if labels.dtype != np.int32:
        raise TypeError("expand_labels expects int32 labels on the device")
    n, H, W = _planes(labels)
    o = _out(ctx, out, labels.shape, np.int32)
    _no_alias("expand_labels", {"labels": labels}, {"out": o})  # cannot work in place: out is another buffer than labels
    _hip.check(_lib().amt_expand_labels(ctx.handle, labels.ptr, o.ptr, n, H, W, expand_nmax(distance), int(bool(ring))),
               "amt_expand_labels")
    return o


# --------------------------------------------------------------------------------------------------
# distance transform, markers, watershed
# --------------------------------------------------------------------------------------------------
def edt(mask: DeviceArray, want_d2: bool = True, want_edt: bool = True, d2_out=None, edt_out=None):
    """``scipy.ndimage.distance_transform_edt`` per plane -> (d2 int32 | None, edt float64 | None)."""
    ctx = mask.ctx
    n, H, W = _planes(mask)
    d2 = _out(ctx, d2_out, mask.shape, np.int32) if want_d2 else None
    e = _out(ctx, edt_out, mask.shape, np.float64) if want_edt else None
    _no_alias("edt", {"mask": mask}, {"d2_out": d2, "edt_out": e})
    _hip.check(_lib().amt_edt(ctx.handle, mask.ptr, d2.ptr if d2 else None, e.ptr if e else None, n, H, W), "amt_edt")
    return d2, e


def peak_mask(d2: DeviceArray, mask: DeviceArray, min_distance: int = 5, out=None, keep=None, status=None) -> DeviceArray:
    """Peaks of the EDT per the config-3 marker recipe.  ``keep`` (the lists ``label_sparse(keep=)``
    maintains) + ``status`` (that call's counts) turn the clear of the persistent ``out`` plane into a clear of the
    previous run's peaks."""
    ctx = d2.ctx
    n, H, W = _planes(d2)
    o = _out(ctx, out, d2.shape, np.uint8)
    prev = (None, None, 0, None)  # list, counts, capacity, status
    if keep is not None:
        if out is None or status is None:
            raise ValueError("keep= needs the caller's persistent out= plane and the previous counts (status=)")
        klist, kcount = keep
        prev = (klist.ptr, kcount.ptr, klist.size // n, status.ptr)
    _no_alias("peak_mask", {"d2": d2, "mask": mask, "keep list": keep and keep[0], "keep counts": keep and keep[1],
                            "status": status}, {"out": o})
    _hip.check(_lib().amt_peak_mask(ctx.handle, d2.ptr, mask.ptr, o.ptr, n, H, W, int(min_distance), *prev),
               "amt_peak_mask")
    o.is_bool = True
    return o


PEAK_MARKERS_LDS_TIER = _hip.PEAK_MARKERS_LDS_TIER  # peak lists up to this length are labelled from LDS


def peak_markers(d2: DeviceArray, mask: DeviceArray, min_distance: int = 5, connectivity: int = 1,
                 capacity: int | None = None, peaks=None, markers=None, count=None, keep=None):
    """``peak_mask`` followed by ``label_sparse`` in one call (``amt_peak_markers``): the peak search lists the peaks it
    finds and the markers are labelled from that list, so neither plane is read again.  Returns (peaks, markers, count),
    bit for bit what the two operators give; a plane with more than ``capacity`` peaks reports count -1 and gets no
    markers.

    ``keep`` = (int32 (n, capacity) list, int32 (n,) counts) as ``label_sparse(keep=)`` takes it: ``peaks``, ``markers``
    and ``count`` must then be the caller's persistent arrays, zeroed once together with the counts, and every call clears
    only the pixels the previous call wrote."""
    ctx = d2.ctx
    n, H, W = _planes(d2)
    if capacity is None:
        capacity = label_sparse_capacity(H, W)
    klist_ptr = kcount_ptr = None
    if keep is not None:
        klist, kcount = keep
        if peaks is None or markers is None or count is None:
            raise ValueError("keep= needs the caller's persistent peaks=, markers= and count= arrays")
        if klist.dtype != np.int32 or klist.size != n * int(capacity) or kcount.dtype != np.int32 or kcount.size != n:
            raise ValueError("keep must be (int32 (n, capacity), int32 (n,))")
        klist_ptr, kcount_ptr = klist.ptr, kcount.ptr
    pk = _out(ctx, peaks, d2.shape, np.uint8)
    mk = _out(ctx, markers, d2.shape, np.int32)
    c = _out(ctx, count, (n,), np.int32)
    _no_alias("peak_markers", {"d2": d2, "mask": mask}, {"peaks": pk, "markers": mk, "count": c, "keep list": keep and keep[0],
                                                         "keep counts": keep and keep[1]})
    _hip.check(_lib().amt_peak_markers(ctx.handle, d2.ptr, mask.ptr, pk.ptr, mk.ptr, c.ptr, n, H, W, int(min_distance),
                                       int(connectivity), int(capacity), klist_ptr, kcount_ptr), "amt_peak_markers")
    pk.is_bool = True
    return pk, mk, c


def _ws_ties(ctx, n: int, ties_policy: str, ties_out):
    """The per-plane tie flags: the caller's array, a fresh one when the policy needs them, else none (the hot path
    allocates nothing)."""
    if ties_policy not in _hip.WS_TIES:
        raise ValueError(f"ties must be one of {sorted(_hip.WS_TIES)}, got {ties_policy!r}")
    if ties_out is not None:
        return _out(ctx, ties_out, (n,), np.int32)
    return ctx.empty((n,), np.int32) if ties_policy in ("report", "refuse") else None


def _ws_finish(ctx, ties_policy: str, ties, what: str):
    if ties_policy == "refuse":
        t = ties.numpy()
        if t.any():
            raise ValueError(
                f"{what}: equal-valued markers inside one mask component in plane(s) {np.flatnonzero(t).tolist()}: "
                "scikit-image orders them by the moves of its binary heap; use ties='exact' (sequential emulation, "
                "bit-identical, slow) or ties='raster'")


def watershed_edt(d2: DeviceArray, markers: DeviceArray, mask: DeviceArray, seeds_first: bool = True, out=None,
                  connectivity: int = 1, ties: str = "exact", ties_out: DeviceArray | None = None):
    """``skimage.segmentation.watershed(-sqrt(d2), markers, connectivity, mask=mask)`` on the exact integer d2.
    ``seeds_first``: the config-3 recipe (the seeded relief of oracle/skops.py:seeded_flood_image; no ties possible).
    ``ties``: what to do with equal-valued markers inside one component (include/amt_hip.h): 'exact' (default;
    bit-identical to scikit-image through a sequential emulation of its heap for the affected planes), 'raster'
    (fast, documented deviation), 'report' (raster + per-plane flags in ``ties_out``), 'refuse' (raise)."""
    ctx = d2.ctx
    n, H, W = _planes(d2)
    o = _out(ctx, out, d2.shape, np.int32)
    t = _ws_ties(ctx, n, ties, ties_out)
    _no_alias("watershed_edt", {"d2": d2, "markers": markers, "mask": mask}, {"out": o, "ties_out": t})
    _hip.check(_lib().amt_watershed_edt(ctx.handle, d2.ptr, markers.ptr, mask.ptr, o.ptr, n, H, W,
                                        1 if seeds_first else 0, int(connectivity), _hip.WS_TIES[ties],
                                        None if t is None else t.ptr),
               "amt_watershed_edt")
    _ws_finish(ctx, ties, t, "watershed_edt")
    return o


def watershed_edt_cleared(d2: DeviceArray, markers: DeviceArray, mask: DeviceArray, nlabels: DeviceArray,
                          max_label: int, scratch: DeviceArray, out=None, count=None, marker_list=None):
    """``relabel_sequential(clear_border(watershed(seeded relief, markers, mask=mask)))`` in one call (the tail of
    config 3; R/masks.py:56,65): identical to ``watershed_edt(seeds_first=True)`` + ``clear_border_relabel`` but the
    watershed image is never written out.  ``markers`` are numbered 1..nlabels[plane]; ``scratch`` is an int32 plane
    batch the flood may use.  Returns (int32 labels, counts)."""
    ctx = d2.ctx
    n, H, W = _planes(d2)
    o = _out(ctx, out, d2.shape, np.int32)
    c = _out(ctx, count, (n,), np.int32)
    if scratch.dtype != np.int32 or scratch.size != d2.size or scratch.ctx is not ctx:
        raise ValueError("scratch must be an int32 array of the batch's size on the same context")
    mk = (None, None, 0)  # list, counts, capacity
    if marker_list is not None:
        # (list, counts) as label_sparse(keep=) leaves them: every non-zero pixel of `markers`; the component statistics
        # then skip the marker plane
        klist, kcount = marker_list
        if klist.dtype != np.int32 or kcount.dtype != np.int32 or kcount.size != n or klist.size % n:
            raise ValueError("marker_list must be (int32 (n, capacity), int32 (n,))")
        mk = (klist.ptr, kcount.ptr, klist.size // n)
    _no_alias("watershed_edt_cleared", {"d2": d2, "markers": markers, "mask": mask, "nlabels": nlabels,
                                        "marker list": marker_list and marker_list[0],
                                        "marker counts": marker_list and marker_list[1]},
              {"scratch": scratch, "out": o, "count": c})
    _hip.check(_lib().amt_watershed_edt_cleared(ctx.handle, d2.ptr, markers.ptr, mask.ptr, scratch.ptr, o.ptr, c.ptr, n, H,
                                                W, int(max_label), nlabels.ptr, *mk), "amt_watershed_edt_cleared")
    return o, c


def watershed(relief: DeviceArray, markers: DeviceArray, mask: DeviceArray, out=None, connectivity: int = 1,
              ties: str = "exact", ties_out: DeviceArray | None = None):
    """``skimage.segmentation.watershed(relief, markers, connectivity, mask=mask)`` for float64 relief
    (``ties`` as in ``watershed_edt``; connectivity 2 always runs the sequential emulation)."""
    ctx = relief.ctx
    n, H, W = _planes(relief)
    o = _out(ctx, out, relief.shape, np.int32)
    t = _ws_ties(ctx, n, ties, ties_out)
    _no_alias("watershed", {"relief": relief, "markers": markers, "mask": mask}, {"out": o, "ties_out": t})
    _hip.check(_lib().amt_watershed_f64(ctx.handle, relief.ptr, markers.ptr, mask.ptr, o.ptr, n, H, W,
                                        int(connectivity), _hip.WS_TIES[ties], None if t is None else t.ptr),
               "amt_watershed_f64")
    _ws_finish(ctx, ties, t, "watershed")
    return o


# --------------------------------------------------------------------------------------------------
# region properties
# --------------------------------------------------------------------------------------------------
def regionprops(labels: DeviceArray, max_label: int, out=None) -> DeviceArray:
    """Morphology table (nplanes, max_label, RP_NCOLS) float64; column order ``_hip.RP_COLS``."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    o = _out(ctx, out, (n, max_label, _hip.RP_NCOLS), np.float64)
    _no_alias("regionprops", {"labels": labels}, {"out": o})
    _hip.check(_lib().amt_regionprops(ctx.handle, labels.ptr, None, 0, o.ptr, None, n, H, W, int(max_label)),
               "amt_regionprops")
    return o


def regionprops_full(labels: DeviceArray, intensity: DeviceArray, max_label: int, out=None, iout=None):
    """Morphology table + intensity table in one call (shared bounding-box pass and per-label scan)."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    if intensity.dtype != np.uint16:
        raise TypeError("intensity images must be uint16 on the device path")
    C, _ = _channel_stack(labels, intensity, n, H, W)
    o = _out(ctx, out, (n, max_label, _hip.RP_NCOLS), np.float64)
    io = _out(ctx, iout, (n, max_label, C, 4), np.float64)
    _no_alias("regionprops_full", {"labels": labels, "intensity": intensity}, {"out": o, "iout": io})
    _hip.check(_lib().amt_regionprops(ctx.handle, labels.ptr, intensity.ptr, C, o.ptr, io.ptr, n, H, W, int(max_label)),
               "amt_regionprops")
    return o, io


def pack_plate_rows(table: DeviceArray, itable, ncells: DeviceArray, fov_index0: int = 0, fov_index=None,
                    out=None, nrows_out=None):
    """Dense per-FOV tables (B, K, RP_NCOLS) [+ (B, K, C, 4)] + cell counts (B,) -> one row per cell,
    ``[fov index, label, morphology columns, C x {mean, max, min, std}]``: the block a rank contributes to the
    plate's all-gather.  Returns (rows (B*K, 16 + 4C) float64 of which the first ``nrows`` are
    written, nrows (1,) int64; -1 flags a field of view whose table overflowed)."""
    ctx = table.ctx
    if table.ndim != 3 or table.shape[2] != _hip.RP_NCOLS or table.dtype != np.float64:
        raise ValueError(f"table must be (B, K, {_hip.RP_NCOLS}) float64, got {table.shape} {table.dtype}")
    B, K = int(table.shape[0]), int(table.shape[1])
    C = 0
    if itable is not None:
        if itable.ndim != 4 or itable.shape[:2] != (B, K) or itable.shape[3] != 4 or itable.dtype != np.float64:
            raise ValueError(f"itable must be (B, K, C, 4) float64, got {itable.shape} {itable.dtype}")
        C = int(itable.shape[2])
    if ncells.dtype != np.int32 or ncells.size != B:
        raise ValueError("ncells must be (B,) int32")
    if fov_index is not None and (fov_index.dtype != np.int32 or fov_index.size != B):
        raise ValueError("fov_index must be (B,) int32")
    ncols = 2 + _hip.RP_NCOLS + 4 * C
    if out is None:
        out = ctx.empty((max(B * K, 1), ncols), np.float64)
    elif out.dtype != np.float64 or out.ndim != 2 or out.shape[1] != ncols or out.shape[0] < B * K:
        raise ValueError(f"out must be (>= {B * K}, {ncols}) float64, got {out.shape} {out.dtype}")
    nr = _out(ctx, nrows_out, (1,), np.int64)
    _no_alias("pack_plate_rows", {"table": table, "itable": itable, "ncells": ncells, "fov_index": fov_index},
              {"out": out, "nrows_out": nr})
    _hip.check(_lib().amt_pack_plate_rows(ctx.handle, table.ptr, None if itable is None else itable.ptr, ncells.ptr,
                                          B, K, C, None if fov_index is None else fov_index.ptr, int(fov_index0),
                                          out.ptr, int(out.shape[0]), nr.ptr), "amt_pack_plate_rows")
    return out, nr


def regionprops_intensity(labels: DeviceArray, intensity: DeviceArray, max_label: int, out=None) -> DeviceArray:
    """Intensity table (nplanes, max_label, C, 4) = {mean, max, min, std}; ``intensity`` is (..., C, Y, X)
    uint16 or float64 with one (C, Y, X) stack per label plane."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    C, code = _channel_stack(labels, intensity, n, H, W)
    o = _out(ctx, out, (n, max_label, C, 4), np.float64)
    _no_alias("regionprops_intensity", {"labels": labels, "intensity": intensity}, {"out": o})
    if code == _hip.U16:  # exact integer accumulation
        _hip.check(_lib().amt_regionprops(ctx.handle, labels.ptr, intensity.ptr, C, None, o.ptr, n, H, W,
                                          int(max_label)), "amt_regionprops")
    else:  # float64 images: two-sweep mean / std as numpy computes them
        _hip.check(_lib().amt_regionprops_intensity_f64(ctx.handle, labels.ptr, intensity.ptr, C, o.ptr, n, H, W,
                                                        int(max_label)), "amt_regionprops_intensity_f64")
    return o


def regionprops_ext(labels: DeviceArray, max_label: int, columns, intensity: DeviceArray | None = None, out=None,
                    wout=None):
    """Extended region properties (include/amt_hip.h ``amt_regionprops_ext``) of every label plane in one call.

    ``columns`` is an iterable of scikit-image 0.25.2 names from ``_hip.RPX_BITS`` (or the OR of their bits).
    Returns (table, wtable): table (nplanes, max_label, RPX_NCOLS) float64 in ``_hip.RPX_COLS`` order, None when only
    weighted centroids are asked for; wtable (nplanes, max_label, C, 4) float64 in ``_hip.RPX_WCOLS`` order, from
    ``intensity`` (..., C, Y, X) uint16 or float64 with one (C, Y, X) stack per label plane, None without it.
    Columns that were not asked for are left unwritten."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    if labels.dtype != np.int32:
        raise TypeError("regionprops_ext expects int32 labels")
    if isinstance(columns, (int, np.integer)):
        bits = int(columns)
    else:
        bits = 0
        for name in columns:
            if name not in _hip.RPX_BITS:
                raise ValueError(f"unknown extended region property {name!r}")
            bits |= _hip.RPX_BITS[name]
    if bits & _hip.RPX_RELATE:
        raise ValueError("bit 8 (AMT_RPX_RELATE) relates two label images: call hipops.relate_labels")
    if bits & _hip.RPX_ROBUST:
        raise ValueError("bit 9 (AMT_RPX_ROBUST) measures quartiles and MAD per channel: call hipops.robust_intensity")
    if bits & (_hip.RPX_NEIGHBORS | _hip.RPX_NEAREST):
        raise ValueError("bits 10 and 11 (AMT_RPX_NEIGHBORS, AMT_RPX_NEAREST) measure a label's surroundings: call "
                         "hipops.neighbor_census or hipops.nearest_labels")
    if bits & (_hip.RPX_TEXTURE | _hip.RPX_TEXTURE_COUNTS):
        raise ValueError("bits 12 and 13 (AMT_RPX_TEXTURE, AMT_RPX_TEXTURE_COUNTS) measure Haralick texture: call hipops.texture")
    if bits & _hip.RPX_RADIAL or bits < 0:
        raise ValueError("bit 31 (AMT_RPX_RADIAL) measures the radial distribution: call hipops.radial_distribution")
    want_w = bool(bits & _hip.RPX_WEIGHTED)
    if want_w != (intensity is not None):
        raise ValueError("weighted centroids need intensity images, and intensity images are only used for them")
    code, C = 0, 0
    if intensity is not None:
        C, code = _channel_stack(labels, intensity, n, H, W)
    o = _out(ctx, out, (n, max_label, _hip.RPX_NCOLS), np.float64) if bits & ~_hip.RPX_WEIGHTED else None
    wo = _out(ctx, wout, (n, max_label, C, 4), np.float64) if want_w else None
    _no_alias("regionprops_ext", {"labels": labels, "intensity": intensity}, {"out": o, "wout": wo})
    _hip.check(_lib().amt_regionprops_ext(ctx.handle, labels.ptr, None if intensity is None else intensity.ptr, code, C,
                                          bits, None if o is None else o.ptr, None if wo is None else wo.ptr, n, H, W,
                                          int(max_label)), "amt_regionprops_ext")
    return o, wo


def relate_labels(labels: DeviceArray, max_label: int, companions: DeviceArray, out=None) -> DeviceArray:
    """How the labels of ``labels`` lie on other label images (``amt_regionprops_ext`` with ``AMT_RPX_RELATE``).

    ``labels`` is int32 (..., Y, X); ``companions`` is int32 (..., C, Y, X) with one (C, Y, X) stack per label plane,
    or (..., Y, X) of the labels' own shape for C = 1; values 0 (background) to 2**31 - 2.  A companion may be
    ``labels`` itself.  Returns (nplanes, max_label, C, 4) float64 in ``_hip.RPX_RCOLS`` order: for label ``l`` and
    companion ``B``, ``parent`` = the non-zero value of ``B`` that covers most pixels of ``l`` (the smallest among
    equal counts, 0 when ``B`` is zero on all of ``l``), ``overlap`` = that count, ``partners`` = the number of
    distinct non-zero values of ``B`` on ``l``, ``area`` = the pixel count of ``l``.  A label absent from its plane
    gives four zeros.  All values are exact integers; two runs give identical bytes."""
    return _companion_table("relate_labels", _hip.RPX_RELATE, labels, max_label, *_label_stack("relate_labels", labels, companions), out)


def _companion_table(op: str, bit: int, labels: DeviceArray, max_label: int, planes, in_code: int, C: int, out):
    """``amt_regionprops_ext`` with one of the bits that fill the table of four columns per companion: ``planes`` (None
    for ``AMT_RPX_NEAREST``) are the ``C`` companion planes of element code ``in_code`` per label plane, already checked
    -> (nplanes, max_label, C, 4) float64"""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    o = _out(ctx, out, (n, max_label, C, 4), np.float64)
    name = "companions" if in_code == _hip.I32 else "intensity"
    _no_alias(op, {"labels": labels, name: planes}, {"out": o})  # a companion may be `labels`
    _hip.check(_lib().amt_regionprops_ext(ctx.handle, labels.ptr, None if planes is None else planes.ptr, in_code, C, bit,
                                          None, o.ptr, n, H, W, int(max_label)), "amt_regionprops_ext")
    return o


def _int32_labels(op: str, labels: DeviceArray):
    """(nplanes, H, W) of the label planes of ``op``, which must be int32"""
    if labels.dtype != np.int32:
        raise TypeError(f"{op} expects int32 labels")
    return _planes(labels)


def _label_stack(op: str, labels: DeviceArray, companions: DeviceArray):
    """(companions, AMT_I32, C) of int32 companion label planes (..., C, Y, X), or (..., Y, X) of the labels' own shape"""
    n, H, W = _int32_labels(op, labels)
    if companions.dtype != np.int32:
        raise TypeError("companion label images must be int32 on the device path")
    if companions.ndim < 2 or companions.shape[-2:] != labels.shape[-2:]:
        raise ValueError("companions must be (..., C, Y, X) or (..., Y, X) matching the label planes")
    if tuple(companions.shape) == tuple(labels.shape):
        C = 1
    else:
        if companions.ndim < 3:
            raise ValueError("companions must be (..., C, Y, X) or (..., Y, X) matching the label planes")
        C = int(companions.shape[-3])
    if C < 1 or companions.size != n * C * H * W:
        raise ValueError("companions / labels plane count mismatch")
    return companions, _hip.I32, C


def neighbor_census(labels: DeviceArray, max_label: int, companions: DeviceArray | None = None, out=None) -> DeviceArray:
    """Which objects touch every label (``amt_regionprops_ext`` with ``AMT_RPX_NEIGHBORS``; CellProfiler's
    MeasureObjectNeighbors).

    ``labels`` is int32 (..., Y, X); ``companions`` as for ``relate_labels``, ``None`` for ``labels`` itself (the usual
    call: the neighbours among the labels' own plane).  The RING of label ``l`` is the set of pixels that do not carry
    ``l`` and have an 8-neighbour that does (clipped by the plane's border); its neighbour values are the positive
    companion values other than ``l`` on the ring.  Returns (nplanes, max_label, C, 4) float64 in ``_hip.RPX_NCOLS4``
    order: ``count`` = the number of distinct neighbour values, ``touching`` = the ring pixels that hold one, ``ring`` =
    the ring's pixel count, ``main`` = the value on most ring pixels (the smallest among equal counts, 0 without a
    neighbour).  A label absent from its plane gives four zeros.  All values are exact integers; two runs give
    identical bytes."""
    return _companion_table("neighbor_census", _hip.RPX_NEIGHBORS, labels, max_label,
                            *_label_stack("neighbor_census", labels, labels if companions is None else companions), out)


def nearest_labels(labels: DeviceArray, max_label: int, out=None) -> DeviceArray:
    """The two nearest labels of every label by centroid distance (``amt_regionprops_ext`` with ``AMT_RPX_NEAREST``).

    Returns (nplanes, max_label, 1, 4) float64 in ``_hip.RPX_DCOLS`` order: ``first`` / ``second`` = the labels of
    1..max_label present in the plane whose centroids (pixel-coordinate means) are nearest, ordered by (squared
    distance, label) so that the smallest label wins among equal distances; ``first_distance`` / ``second_distance`` =
    the Euclidean distances.  Where there is no such label, and for a label absent from its plane, the label is 0 and
    the distance NaN.  Every pair of labels of a plane is compared; two runs give identical bytes."""
    _int32_labels("nearest_labels", labels)
    return _companion_table("nearest_labels", _hip.RPX_NEAREST, labels, max_label, None, 0, 1, out)


def robust_intensity(labels: DeviceArray, intensity: DeviceArray, max_label: int, out=None) -> DeviceArray:
    """Robust intensity table (nplanes, max_label, C, 4) float64 in ``_hip.RPX_QCOLS`` order (``amt_regionprops_ext``
    with ``AMT_RPX_ROBUST``): ``np.percentile(V, 25 | 50 | 75)`` (method ``linear``) and the raw median absolute
    deviation ``np.percentile(|V - median|, 50)`` of every channel over the pixels ``V`` of every label, bit for bit.

    ``labels`` is int32 (..., Y, X); ``intensity`` is (..., C, Y, X) uint16 (exact selection on integers) or float64
    (without NaN or infinities) with one (C, Y, X) stack per label plane.  A label absent from its plane gives four
    NaNs; two runs give identical bytes."""
    C, code = _channel_stack(labels, intensity, *_int32_labels("robust_intensity", labels))
    if C < 1:
        raise ValueError("intensity / labels plane count mismatch")
    return _companion_table("robust_intensity", _hip.RPX_ROBUST, labels, max_label, intensity, code, C, out)


def colocalization_pairs(C: int, pairs=None) -> np.ndarray:
    """The (npairs, 2) int32 channel-index pairs ``colocalization`` measures: every i < j in channel order for
    ``pairs=None``, else the given (i, j) with i != j, both below ``C``, in the given order."""
    if pairs is None:
        return np.array([(i, j) for i in range(C) for j in range(i + 1, C)], dtype=np.int32).reshape(-1, 2)
    listed = [tuple(p) for p in pairs]
    if not listed:
        raise ValueError("pairs must name at least one pair of channels")
    for p in listed:
        if len(p) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in p):
            raise TypeError(f"pairs must be (i, j) tuples of channel indices, got {p!r}")
        i, j = int(p[0]), int(p[1])
        if not (0 <= i < C and 0 <= j < C):
            raise ValueError(f"pair {p!r} names a channel outside 0..{C - 1}")
        if i == j:
            raise ValueError(f"pair {p!r} names the same channel twice")
    return np.array(listed, dtype=np.int32).reshape(-1, 2)


def colocalization(labels: DeviceArray, intensity: DeviceArray, max_label: int, thresholds=None, pairs=None,
                   out=None) -> DeviceArray:
    """Per-label colocalisation of channel pairs (include/amt_hip.h ``amt_colocalization``): table (nplanes, max_label,
    npairs, COLOC_NCOLS) float64 in ``_hip.COLOC_COLS`` order -- Pearson, Manders' overlap, M1, M2 and the two
    intersection coefficients, as ``skimage.measure`` (0.20 and later) defines them, of every label 1..max_label.

    ``labels`` is int32 (..., Y, X); ``intensity`` is (..., C, Y, X) uint16 (exact integer sums, reproducible bit for
    bit) or float64, one (C, Y, X) stack per label plane, C >= 2.  ``thresholds`` (a pixel is positive when its value
    is > the threshold of its channel): None = 0 for every channel, a number, an array broadcastable to (nplanes, C),
    or a float64 ``DeviceArray`` of that shape, which is used as it is (no synchronisation).  ``pairs``: None = every
    i < j in channel order, or a list of (i, j), i != j; for pair (i, j) channel i is A and channel j is B.  A label
    absent from its plane gives NaN, NaN, 0, 0, 0, 0."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    if labels.dtype != np.int32:
        raise TypeError("colocalization expects int32 labels")
    C, code = _channel_stack(labels, intensity, n, H, W)
    if C < 2:
        raise ValueError("colocalization needs at least two channels")
    if isinstance(thresholds, DeviceArray):
        if thresholds.dtype != np.float64 or tuple(thresholds.shape) != (n, C):
            raise ValueError(f"device thresholds must be ({n}, {C}) float64, got {thresholds.shape} {thresholds.dtype}")
        thr = thresholds
    else:
        try:
            host = np.broadcast_to(np.asarray(0.0 if thresholds is None else thresholds, dtype=np.float64), (n, C))
        except ValueError:
            raise ValueError(f"thresholds must be broadcastable to ({n}, {C})") from None
        thr = ctx.asarray(np.ascontiguousarray(host))
    pr = colocalization_pairs(C, pairs)
    o = _out(ctx, out, (n, max_label, len(pr), _hip.COLOC_NCOLS), np.float64)
    _no_alias("colocalization", {"labels": labels, "intensity": intensity, "thresholds": thr}, {"out": o})
    _hip.check(_lib().amt_colocalization(ctx.handle, labels.ptr, intensity.ptr, code, C, thr.ptr,
                                         pr.ctypes.data_as(ctypes.c_void_p), len(pr), o.ptr, n, H, W, int(max_label)),
               "amt_colocalization")
    return o


def texture_parameters(levels, distance) -> tuple[int, int]:
    """(levels, distance) of ``texture`` as ints: integers in 2..TEX_MAX_LEVELS and 1..TEX_MAX_DISTANCE (no device needed)"""
    for name, v in (("levels", levels), ("distance", distance)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer, got {v!r}")
    if not 2 <= int(levels) <= _hip.TEX_MAX_LEVELS:
        raise ValueError(f"levels must be in 2..{_hip.TEX_MAX_LEVELS}, got {levels}")
    if not 1 <= int(distance) <= _hip.TEX_MAX_DISTANCE:
        raise ValueError(f"distance must be in 1..{_hip.TEX_MAX_DISTANCE}, got {distance}")
    return int(levels), int(distance)


def texture(labels: DeviceArray, intensity: DeviceArray, max_label: int, levels: int = 8, distance: int = 1, ranges=None,
            out=None, glcm=False):
    """Per-label Haralick texture (``amt_regionprops_ext`` with ``AMT_RPX_TEXTURE``): table (nplanes, max_label, C, 4,
    TEX_NCOLS) float64 -- for every label 1..max_label, channel and direction of ``_hip.TEX_ANGLES`` (0, 45, 90, 135 degrees at
    ``distance`` pixels) the thirteen features of ``_hip.TEX_COLS`` of the symmetric grey-level co-occurrence matrix, as
    ``mahotas.features.haralick`` (CellProfiler's MeasureTexture) defines them.

    ``labels`` is int32 (..., Y, X); ``intensity`` is (..., C, Y, X) uint16 or float64 (without NaN or infinities), one
    (C, Y, X) stack per label plane.  A value v of an image with the range (lo, hi) falls into level
    ``min(levels - 1, floor((clip(v, lo, hi) - lo) / (hi - lo) * levels))``; ``hi <= lo`` puts everything into level 0.
    ``ranges``: None = every (plane, channel) image's own minimum and maximum, found on the device (no
    synchronisation); a (lo, hi) pair for all images; an array broadcastable to (nplanes, C, 2); or a float64
    ``DeviceArray`` of that shape, which is used as it is.  ``levels`` 2..64, ``distance`` 1..255.
    ``glcm=True`` returns ``(table, counts)`` with counts (nplanes, max_label, C, 4, levels, levels) uint32, the raw
    matrices (exact integers; a uint32 ``DeviceArray`` of that shape is filled and returned); they come from a second
    call of the entry point, which the table does not depend on.  ``out`` is always the table.  A direction in which a
    label has no pair gives NaN features and zero counts for that direction, a label absent from its plane for all
    four.  Two runs give identical bytes."""
    n, H, W = _int32_labels("texture", labels)
    C, code = _channel_stack(labels, intensity, n, H, W)
    if C < 1:
        raise ValueError("intensity / labels plane count mismatch")
    L, d = texture_parameters(levels, distance)
    K = int(max_label)
    if K < 0:
        raise ValueError("max_label must not be negative")
    host = None
    if isinstance(ranges, DeviceArray):
        if ranges.dtype != np.float64 or tuple(ranges.shape) != (n, C, 2):
            raise ValueError(f"device ranges must be ({n}, {C}, 2) float64, got {ranges.shape} {ranges.dtype}")
    elif ranges is not None:
        try:
            host = np.broadcast_to(np.asarray(ranges, dtype=np.float64), (n, C, 2))
        except (ValueError, TypeError):
            raise ValueError(f"ranges must be None, a (lo, hi) pair or broadcastable to ({n}, {C}, 2)") from None
    ctx = labels.ctx
    want_glcm = glcm is not None and glcm is not False
    if want_glcm and glcm is not True and not isinstance(glcm, DeviceArray):
        raise TypeError("glcm must be False, True or a uint32 DeviceArray for the counts")
    # the caller's own buffers are judged before anything is reserved or launched; what is made here overlaps nothing
    o = None if out is None else _out(ctx, out, (n, K, C, 4, _hip.TEX_NCOLS), np.float64)
    g = _out(ctx, glcm, (n, K, C, 4, L, L), np.uint32) if isinstance(glcm, DeviceArray) else None
    _no_alias("texture", {"labels": labels, "intensity": intensity,
                          "ranges": ranges if isinstance(ranges, DeviceArray) else None}, {"out": o, "glcm": g})
    if isinstance(ranges, DeviceArray):
        rng = ranges
    elif host is not None:
        rng = ctx.asarray(np.ascontiguousarray(host))
    else:  # the extrema of every (plane, channel) image: percentiles 0 and 100 of a uint16 plane are its min and max
        rng = ctx.empty((n, C, 2), np.float64)
        if code == _hip.F64:
            _hip.check(_lib().amt_minmax_f64(ctx.handle, intensity.ptr, rng.ptr, n * C, H * W), "amt_minmax_f64")
        else:
            q, qp = _host_f64([0.0, 100.0])
            _hip.check(_lib().amt_percentile_u16(ctx.handle, intensity.ptr, qp, 2, rng.ptr, n * C, H * W),
                       "amt_percentile_u16")
    if o is None:
        o = ctx.empty((n, K, C, 4, _hip.TEX_NCOLS), np.float64)
    if want_glcm and g is None:
        g = ctx.empty((n, K, C, 4, L, L), np.uint32)
    # one call per output: the features, then (when asked for) the counts from a second sweep of the same boxes
    for counts, buf in ((False, o), (True, g)):
        if buf is not None:
            _hip.check(_lib().amt_regionprops_ext(ctx.handle, labels.ptr, intensity.ptr, code, C,
                                                  _hip.rpx_texture_columns(L, d, counts), rng.ptr, buf.ptr, n, H, W, K),
                       "amt_regionprops_ext")
    return o if g is None else (o, g)


def radial_parameters(bins) -> int:
    """``bins`` of ``radial_distribution`` as an int: an integer in 1..RAD_MAX_BINS (no device needed)"""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)):
        raise TypeError(f"bins must be an integer, got {bins!r}")
    if not 1 <= int(bins) <= _hip.RAD_MAX_BINS:
        raise ValueError(f"bins must be in 1..{_hip.RAD_MAX_BINS}, got {bins}")
    return int(bins)


def radial_distribution(labels: DeviceArray, intensity: DeviceArray | None, max_label: int, bins: int = 4, out=None,
                        geometry_out=None):
    """Per-label radial intensity distribution and inscribed radii (``amt_regionprops_ext`` with ``AMT_RPX_RADIAL``; after
    CellProfiler's MeasureObjectIntensityDistribution and the radius columns of MeasureObjectSizeShape).

    ``labels`` is int32 (..., Y, X); ``intensity`` is (..., C, Y, X) uint16 (exact integer sums, every column
    reproducible bit for bit) or float64 (without NaN or infinities), one (C, Y, X) stack per label plane, or None.
    Returns ``(geometry, table)``: geometry (nplanes, max_label, RAD_GEOM_NCOLS) float64 -- ``maximum_radius`` (the
    radius of the largest inscribed circle), ``mean_radius`` (the mean distance of the label's pixels to its edge), then
    the pixel counts of the rings 0 (innermost) .. bins - 1 and zeros up to sixteen; table (nplanes, max_label, C, bins,
    RAD_NCOLS) float64 in ``_hip.RAD_COLS`` order, None without ``intensity``.  The distance of a pixel is the exact
    Euclidean distance to the nearest pixel that does not carry its label (background, a touching neighbour, or the
    frame outside the image); a pixel at distance d of a label whose largest distance is dmax lies in ring
    ``floor(bins * (1 - d / dmax))``, decided on integers; include/amt_hip.h states every column.  ``out`` is the table,
    ``geometry_out`` the geometry.  A label absent from its plane gives NaN radii, zero counts and NaN columns.  Two
    runs give identical bytes."""
    n, H, W = _int32_labels("radial_distribution", labels)
    B = radial_parameters(bins)
    K = int(max_label)
    if K < 0:
        raise ValueError("max_label must not be negative")
    C, code = 0, 0
    if intensity is not None:
        C, code = _channel_stack(labels, intensity, n, H, W)
        if C < 1:
            raise ValueError("intensity / labels plane count mismatch")
    elif out is not None:
        raise ValueError("out is the table of the intensity images: without them there is none")
    ctx = labels.ctx
    g = None if geometry_out is None else _out(ctx, geometry_out, (n, K, _hip.RAD_GEOM_NCOLS), np.float64)
    o = None if out is None else _out(ctx, out, (n, K, C, B, _hip.RAD_NCOLS), np.float64)
    _no_alias("radial_distribution", {"labels": labels, "intensity": intensity}, {"geometry_out": g, "out": o})
    if g is None:
        g = ctx.empty((n, K, _hip.RAD_GEOM_NCOLS), np.float64)
    if o is None and C:
        o = ctx.empty((n, K, C, B, _hip.RAD_NCOLS), np.float64)
    _hip.check(_lib().amt_regionprops_ext(ctx.handle, labels.ptr, None if intensity is None else intensity.ptr, code, C,
                                          _hip.rpx_radial_columns(B), g.ptr, None if o is None else o.ptr, n, H, W, K),
               "amt_regionprops_ext")
    return g, o


def cellpose_masks(dP: DeviceArray, cellprob: DeviceArray, cellprob_threshold: float = 0.0, niter: int = 200,
                   min_size: int = 15, max_size_fraction: float = 0.4, max_seeds: int = 16384, out=None, count=None,
                   flow_threshold: float = 0.0, fill_holes: bool = False):
    """Cellpose's flow -> mask post-processing on the device (include/amt_hip.h ``amt_cellpose_masks_ex``; parity
    unpinned): ``dP`` (..., 2, Y, X) float32 flows (dY, dX), ``cellprob`` (..., Y, X) float32 -> (int32 labels, counts).
    ``flow_threshold`` > 0 adds the flow-error filter (``remove_bad_flow_masks``), ``fill_holes`` the hole filling of
    ``fill_holes_and_remove_small_masks``; with neither, only the dynamics and the size filters run.  A plane that
    produces more than ``max_seeds`` seeds reports count -1.  The size ceiling is ``int(Y * X * max_size_fraction)`` in
    float64 (the fraction crosses the C interface as a double)."""
    ctx = dP.ctx
    if dP.dtype != np.float32 or cellprob.dtype != np.float32:
        raise TypeError("cellpose_masks expects float32 flows and cell probabilities")
    n, H, W = _planes(cellprob)
    if dP.ndim < 3 or dP.shape[-3] != 2 or dP.shape[-2:] != cellprob.shape[-2:] or dP.size != 2 * cellprob.size:
        raise ValueError(f"dP must be (..., 2, Y, X) matching cellprob (..., Y, X); got {dP.shape} and {cellprob.shape}")
    if flow_threshold is None:
        flow_threshold = 0.0
    if flow_threshold < 0:
        raise ValueError(f"flow_threshold must be non-negative, got {flow_threshold}")
    o = _out(ctx, out, cellprob.shape, np.int32)
    c = _out(ctx, count, (n,), np.int32)
    _no_alias("cellpose_masks", {"dP": dP, "cellprob": cellprob}, {"out": o, "count": c})
    _hip.check(_lib().amt_cellpose_masks_ex(ctx.handle, dP.ptr, cellprob.ptr, o.ptr, c.ptr, n, H, W,
                                            float(cellprob_threshold), int(niter), int(min_size),
                                            float(max_size_fraction), int(max_seeds), float(flow_threshold),
                                            1 if fill_holes else 0), "amt_cellpose_masks_ex")
    return o, c


def cellpose_flow_error(labels: DeviceArray, dP: DeviceArray, max_label: int, nlabels: DeviceArray | None = None):
    """``cellpose.metrics.flow_error`` on the device: (..., Y, X) int32 labels carrying 1..K and (..., 2, Y, X) float32
    network flows -> (nplanes, max_label) float64 errors (absent labels 0).  Parity unpinned."""
    ctx = labels.ctx
    if labels.dtype != np.int32 or dP.dtype != np.float32:
        raise TypeError("cellpose_flow_error expects int32 labels and float32 flows")
    n, H, W = _planes(labels)
    if dP.ndim < 3 or dP.shape[-3] != 2 or dP.shape[-2:] != labels.shape[-2:] or dP.size != 2 * labels.size:
        raise ValueError(f"dP must be (..., 2, Y, X) matching labels (..., Y, X); got {dP.shape} and {labels.shape}")
    if nlabels is None:
        nlabels = ctx.asarray(np.full((n,), int(max_label), np.int32))
    err = ctx.empty((n, int(max_label)), np.float64)
    _hip.check(_lib().amt_cellpose_flow_error(ctx.handle, labels.ptr, dP.ptr, nlabels.ptr, err.ptr, n, H, W,
                                              int(max_label)), "amt_cellpose_flow_error")
    return err


def fill_holes_remove_small(labels: DeviceArray, max_label: int, min_size: int = 15, fill_holes: bool = True,
                            nlabels: DeviceArray | None = None):
    """``cellpose.utils.fill_holes_and_remove_small_masks`` on (..., Y, X) int32 labels carrying 1..max_label ->
    (new int32 labels, counts).  Parity unpinned (oracle/cellpose_dynamics.py)."""
    ctx = labels.ctx
    if labels.dtype != np.int32:
        raise TypeError("fill_holes_remove_small expects int32 labels")
    n, H, W = _planes(labels)
    out = labels.copy()
    if nlabels is None:
        nlabels = ctx.asarray(np.full((n,), int(max_label), np.int32))
    c = ctx.empty((n,), np.int32)
    _hip.check(_lib().amt_fill_holes_remove_small(ctx.handle, out.ptr, nlabels.ptr, c.ptr, n, H, W, int(max_label),
                                                  int(min_size), 1 if fill_holes else 0), "amt_fill_holes_remove_small")
    return out, c


def label_bboxes(labels: DeviceArray, max_label: int) -> np.ndarray:
    """(nplanes, max_label, 4) int32 {min row, min col, max row, max col}, inclusive; absent labels have max < min."""
    ctx = labels.ctx
    n, H, W = _planes(labels)
    if labels.dtype != np.int32:
        raise TypeError("label_bboxes expects int32 labels")
    o = ctx.empty((n, int(max_label), 4), np.int32)
    _hip.check(_lib().amt_label_bboxes(ctx.handle, labels.ptr, o.ptr, n, H, W, int(max_label)), "amt_label_bboxes")
    return o.numpy()


def cell_outlines(labels: DeviceArray, max_label: int) -> list[np.ndarray]:
    """Outline of every label present in ONE int32 label plane, as ``_extract_outlines_skimage`` returns them
    (R/masks.py:82-115): marching squares at level 0.5 on the bounding box padded by one pixel, longest contour,
    (row, col) float64 vertices in image coordinates, ascending label order, empty (0, 2) arrays where no
    contour exists.  The walks run on the device; the host only sizes the scratch and output buffers."""
    ctx = labels.ctx
    if labels.ndim != 2 or labels.dtype != np.int32:
        raise TypeError("cell_outlines expects one (Y, X) int32 label plane")
    H, W = labels.shape
    bb = label_bboxes(labels, max(int(max_label), 1))[0]
    present = np.nonzero(bb[:, 2] >= bb[:, 0])[0]
    nlab = len(present)
    if nlab == 0:
        return []
    boxes = np.empty((nlab, 5), dtype=np.int32)
    boxes[:, 0] = present + 1
    boxes[:, 1] = np.maximum(bb[present, 0] - 1, 0)
    boxes[:, 2] = np.maximum(bb[present, 1] - 1, 0)
    boxes[:, 3] = np.minimum(bb[present, 2] + 2, H)
    boxes[:, 4] = np.minimum(bb[present, 3] + 2, W)
    squares = np.maximum(boxes[:, 3] - boxes[:, 1] - 1, 0).astype(np.int64) * np.maximum(
        boxes[:, 4] - boxes[:, 2] - 1, 0)
    voff = np.concatenate([[0], np.cumsum(squares)]).astype(np.int64)
    d_boxes, d_voff = ctx.asarray(boxes), ctx.asarray(voff)
    nvis = int(voff[-1])
    d_vis = ctx.empty((max(nvis, 1),), np.uint8)
    d_info = ctx.empty((nlab, 4), np.int32)
    _hip.check(_lib().amt_contours_find(ctx.handle, labels.ptr, H, W, nlab, d_boxes.ptr, d_voff.ptr, d_vis.ptr, nvis,
                                        d_info.ptr), "amt_contours_find")
    info = d_info.numpy()
    poff = np.concatenate([[0], np.cumsum(info[:, 0].astype(np.int64))]).astype(np.int64)
    total = int(poff[-1])
    if total == 0:
        return [np.array([]).reshape(0, 2) for _ in range(nlab)]
    d_poff = ctx.asarray(poff)
    d_pts = ctx.empty((total, 2), np.float64)
    _hip.check(_lib().amt_contours_emit(ctx.handle, labels.ptr, H, W, nlab, d_boxes.ptr, d_info.ptr, d_poff.ptr,
                                        d_pts.ptr), "amt_contours_emit")
    pts = d_pts.numpy()
    return [pts[poff[i]:poff[i + 1]].copy() if poff[i + 1] > poff[i] else np.array([]).reshape(0, 2)
            for i in range(nlab)]


def cell_outlines_borders(labels: DeviceArray, max_label: int, skip_first_value: bool = True) -> list[np.ndarray]:
    """Outline of every label of ONE int32 label plane as the reference's default "cellpose" extractor returns
    them (R/masks.py:68-79): ``cellpose.utils.outlines_list`` = OpenCV ``findContours(masks == n, RETR_EXTERNAL,
    CHAIN_APPROX_NONE)`` per label, contour with the most points, (y, x) int64 pixel coordinates after the
    reference's column swap, ``np.zeros((0, 2))`` when the border has fewer than five points.  ``outlines_list``
    iterates ``np.unique(masks)[1:]``, i.e. it drops the smallest value present whatever it is; with
    ``skip_first_value`` the same happens here (label 1 is dropped when the plane has no background pixel).
    Border following runs on the device.  Parity unpinned (no OpenCV offline), see oracle/contours.py."""
    ctx = labels.ctx
    if labels.ndim != 2 or labels.dtype != np.int32:
        raise TypeError("cell_outlines_borders expects one (Y, X) int32 label plane")
    H, W = labels.shape
    bb = label_bboxes(labels, max(int(max_label), 1))[0]
    present = np.nonzero(bb[:, 2] >= bb[:, 0])[0]
    if skip_first_value and len(present):
        area = (bb[present, 2] - bb[present, 0] + 1).astype(np.int64) * (bb[present, 3] - bb[present, 1] + 1)
        # a background pixel exists unless the labels tile the plane; only then is it worth counting pixels
        if area.sum() >= H * W:
            cols = list(_hip.RP_COLS)
            tab = regionprops(labels, max(int(max_label), 1)).numpy()[0]
            if int(round(tab[:, cols.index("area")].sum())) >= H * W:
                present = present[1:]
    nlab = len(present)
    if nlab == 0:
        return []
    boxes = np.empty((nlab, 5), dtype=np.int32)
    boxes[:, 0] = present + 1
    boxes[:, 1] = bb[present, 0]
    boxes[:, 2] = bb[present, 1]
    boxes[:, 3] = bb[present, 2] + 1
    boxes[:, 4] = bb[present, 3] + 1
    d_boxes = ctx.asarray(boxes)
    d_marks = ctx.empty((H, W), np.int8)
    d_info = ctx.empty((nlab, 3), np.int32)
    _hip.check(_lib().amt_borders_find(ctx.handle, labels.ptr, H, W, nlab, d_boxes.ptr, d_marks.ptr, d_info.ptr),
               "amt_borders_find")
    info = d_info.numpy()
    npts = np.where(info[:, 0] > 4, info[:, 0], 0).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)
    total = int(poff[-1])
    if total == 0:
        return [np.zeros((0, 2)) for _ in range(nlab)]
    d_poff = ctx.asarray(poff)
    d_pts = ctx.empty((total, 2), np.int32)
    _hip.check(_lib().amt_borders_emit(ctx.handle, labels.ptr, H, W, nlab, d_boxes.ptr, d_info.ptr, d_poff.ptr,
                                       d_pts.ptr), "amt_borders_emit")
    pts = d_pts.numpy().astype(np.int64)
    return [pts[poff[i]:poff[i + 1]].copy() if poff[i + 1] > poff[i] else np.zeros((0, 2)) for i in range(nlab)]
