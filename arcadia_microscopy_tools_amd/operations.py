"""Image operations of the reference (R/operations.py:10-216) on the GPU.

``rescale_by_percentile``, ``subtract_background_dog``, ``crop_to_center`` and ``apply_threshold`` keep the
reference's signatures, validation, error messages and edge-case results.  Each accepts a numpy array
(uploaded, processed, downloaded: a drop-in call) or a ``DeviceArray`` (stays in HBM, so a ``Pipeline``
of these functions makes one upload and one download).  All pixel-sized arithmetic runs in HIP kernels
behind the C ABI; there is no CPU fallback.

n-D inputs follow the reference, which hands whatever array it is given to numpy / scikit-image: percentiles and
global thresholds are taken over the WHOLE stack, a difference of Gaussians filters EVERY axis (leading axes first, as
scipy does), ``crop_to_center`` crops the last two axes.  To treat a (T, Y, X) / (Z, Y, X) stack plane by plane use
``Pipeline(parallel=True)``, which maps the operations over axis 0 as the reference does (R/pipeline.py:139-149).
The local thresholds follow suit: Niblack / Sauvola windows span every axis of a stack (``window_size`` an odd integer
or one per axis), ``threshold_local`` filters every axis with its Gaussian; its ``mean`` / ``median`` methods are 2-D only.

dtypes: uint8 / uint16 / float64 are computed as the reference computes them (bit-exact).  Other integer
types are converted on upload: to uint16 when the values fit (exact), otherwise to float64 (exact below 2^53).  The
histogram thresholds bin integers one bin per value as scikit-image does: an integer image beyond the uint16 range
travels as ``x - min`` when its RANGE fits 65,536 values, as float64 with one device bin per value up to a range of
2^26 values (``amt_hist_range_f64``), and is refused beyond that (scikit-image itself would need gigabytes per array).
Where scikit-image's result depends on the dtype itself -- ``img_as_float`` inside the Gaussians of the DoG, Sauvola's
default ``r`` -- the CALLER's dtype decides (``_img_as_float_plan``, ``_sauvola_r``), not the type the data travels as.
float32 / float16 are computed in float64: numpy / scikit-image keep float32 arithmetic for them, so results agree
to float32 rounding (~1e-7 relative), inside the 1e-5 bar for float outputs but not bit for bit.
"""
from __future__ import annotations

from typing import Literal

import numpy as np

from . import _thresholds, hipops
from .device import DeviceArray, get_context
from .pipeline import device_operator
from .typing import BoolArray, Float64Array, ScalarArray

_MAX_INTEGER_BINS = 1 << 26  # one uint32 bin per integer value: 256 MB on the device, 512 MB per float64 host array

_SUPPORTED_METHODS = ("otsu", "li", "yen", "isodata", "mean", "minimum", "triangle", "local", "niblack", "sauvola")


def _to_device(intensities, what: str, integer_histogram: bool = False, shifted: list | None = None):
    """-> (DeviceArray, was_numpy).  See the module docstring for the dtype rules.  ``integer_histogram``: the caller
    bins integer images by value (scikit-image's histogram), so integers beyond uint16 cannot be taken -- unless the
    caller passes ``shifted`` (a one-element list) and the image's RANGE fits 65,536 values: it then travels as
    ``x - min`` in uint16 and ``shifted[0]`` receives ``min`` (scikit-image bins such images from image_min to
    image_max, one bin per integer: SK/exposure/exposure.py:38-74)."""
    if isinstance(intensities, DeviceArray):
        d = intensities
        if d.dtype not in (np.uint16, np.float64):
            raise TypeError(f"{what}: device arrays must be uint16 or float64, got {d.dtype}")
        return d, False
    a = np.asarray(intensities)
    if a.dtype == np.bool_:
        a = a.astype(np.uint16)
    elif a.dtype == np.uint8:
        a = a.astype(np.uint16)
    elif np.issubdtype(a.dtype, np.integer) and a.dtype != np.uint16:
        lo, hi = (int(a.min()), int(a.max())) if a.size else (0, 0)
        if lo >= 0 and hi <= 65535:
            a = a.astype(np.uint16)  # exact: same values, same integer histogram
        elif integer_histogram and shifted is not None and hi - lo <= 65535:
            shifted[0] = lo
            # subtract in a type that holds the whole range: int8 [-128, 127] - (-128) overflows int8 itself
            wide = a if a.dtype == np.uint64 else a.astype(np.int64)
            a = (wide - wide.dtype.type(lo)).astype(np.uint16)
        elif integer_histogram and shifted is not None and hi - lo < _MAX_INTEGER_BINS:
            # one bin per value over a range beyond uint16: the image travels as float64 (exact below 2^53) and is
            # binned by amt_hist_range_f64; shifted[1] tells the caller the range
            shifted[0] = lo
            shifted.append(hi - lo + 1)
            a = a.astype(np.float64)
        elif integer_histogram:
            raise NotImplementedError(
                f"{what}: integer image with values in [{lo}, {hi}]: scikit-image bins integers one bin per value "
                f"({hi - lo + 1:,} bins here); the device path stops at {_MAX_INTEGER_BINS:,}"
            )
        else:
            a = a.astype(np.float64)
    elif a.dtype in (np.float32, np.float16):
        a = a.astype(np.float64)
    elif a.dtype not in (np.uint16, np.float64):
        raise TypeError(f"{what}: dtype {a.dtype} is not supported on the MI355X path")
    return get_context().asarray(np.ascontiguousarray(a)), True


def _img_as_float_plan(intensities):
    """How ``skimage.util.img_as_float`` (SK/util/dtype.py:280-330, called by ``filters.gaussian``) treats the dtype of a
    host array -> (array to upload, scale for the device Gaussian or None for its default).  uint16 and uint8 travel as
    uint16 and are multiplied by 1/65535 resp. 1/255 on the device, bool by 1; wider unsigned integers are multiplied by
    1/imax and signed integers mapped by (x + 0.5) * 2 / (imax - imin) on the host, in float64, exactly as scikit-image
    does, and travel as float64."""
    if isinstance(intensities, DeviceArray):
        return intensities, None
    a = np.asarray(intensities)
    if a.dtype == np.bool_:
        return a, 1.0
    if a.dtype == np.uint8:
        return a, 1.0 / 255
    if a.dtype.kind == "u" and a.dtype != np.uint16:
        return np.multiply(a, 1.0 / int(np.iinfo(a.dtype).max), dtype=np.float64), None
    if a.dtype.kind == "i":
        info = np.iinfo(a.dtype)
        f = np.add(a, 0.5, dtype=np.float64)
        f *= 2 / (int(info.max) - int(info.min))
        return f, None
    return a, None


def _sauvola_r(dtype) -> float:
    """threshold_sauvola's default ``r``: half the dtype's range, ``dtype_limits(image, clip_negative=False)``
    (SK/filters/thresholding.py:1079-1081; floats count as (-1, 1), bool as (False, True))."""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return 0.5
    if dt.kind in "ui":
        info = np.iinfo(dt)
        return 0.5 * (int(info.max) - int(info.min))
    return 1.0


def _flat(d: DeviceArray) -> DeviceArray:
    """The whole array as ONE plane (1, size): statistics over a stack are statistics over all its samples."""
    return d if d.ndim == 2 else d.reshape(1, d.size)


def _result(d: DeviceArray, was_numpy: bool):
    return d.numpy() if was_numpy else d


def _min_max(d: DeviceArray):
    mm = hipops.percentile(_flat(d), (0.0, 100.0)).numpy()[0]
    return mm[0], mm[1]


@device_operator
def rescale_by_percentile(
    intensities: ScalarArray,
    percentile_range: tuple[float, float] = (0, 100),
    out_range: tuple[float, float] = (0, 1),
) -> ScalarArray:
    """Percentile-based contrast stretching (R/operations.py:10-54): ``np.percentile`` then
    ``skimage.exposure.rescale_intensity(in_range=(p1, p2), out_range=out_range)``; float64 result."""
    if not (0 <= percentile_range[0] < percentile_range[1] <= 100):
        raise ValueError(
            f"Invalid percentile range: {percentile_range}. "
            f"Values must be in ascending order between 0 and 100."
        )
    if not isinstance(intensities, DeviceArray) and np.asarray(intensities).size == 0:
        return np.zeros_like(intensities, dtype=float)
    d, was_numpy = _to_device(intensities, "rescale_by_percentile")
    lo, hi = _min_max(d)
    if lo == hi:  # constant image (R/operations.py:43-44)
        const = np.full(d.shape, out_range[0], dtype=float)
        return const if was_numpy else d.ctx.asarray(const)
    f = _flat(d)
    p = hipops.percentile(f, percentile_range)
    return _result(hipops.rescale(f, p, out_range).reshape(d.shape), was_numpy)


@device_operator
def subtract_background_dog(
    intensities: ScalarArray,
    low_sigma: float = 0.6,
    high_sigma: float = 16.0,
    percentile: float = 0,
) -> Float64Array:
    """Difference-of-Gaussians background subtraction (R/operations.py:57-97):
    ``clip(dog - np.percentile(dog, percentile), 0, None)`` with ``dog = difference_of_gaussians(x, low, high)``."""
    if not (0 <= percentile <= 100):
        raise ValueError(f"Percentile must be between 0 and 100, got {percentile}")
    if low_sigma >= high_sigma:
        raise ValueError(f"low_sigma ({low_sigma}) must be smaller than high_sigma ({high_sigma})")
    intensities, scale = _img_as_float_plan(intensities)
    d, was_numpy = _to_device(intensities, "subtract_background_dog")
    dog = (hipops.difference_of_gaussians(d, low_sigma, high_sigma, scale=scale) if d.ndim == 2 else
           hipops.difference_of_gaussians_nd(d, low_sigma, high_sigma, scale=scale))
    f = _flat(dog)
    level = hipops.percentile(f, percentile)
    hipops.sub_clip0(f, level, out=f)
    return _result(dog, was_numpy)


@device_operator
def crop_to_center(intensities: ScalarArray, output_shape: tuple[int, int]) -> ScalarArray:
    """Centre crop on the last two axes, clamped to the image size (R/operations.py:100-132).
    numpy input -> a view, as in the reference; DeviceArray input -> a cropped device copy."""
    height, width = intensities.shape[-2:]
    crop_height, crop_width = output_shape
    crop_width = min(width, crop_width)
    crop_height = min(height, crop_height)
    left = (width - crop_width) // 2
    top = (height - crop_height) // 2
    if isinstance(intensities, DeviceArray):
        return hipops.crop(intensities, top, left, crop_height, crop_width)
    return intensities[..., top: top + crop_height, left: left + crop_width]


@device_operator
def expand_labels(label_image, distance: float = 1):
    """``skimage.segmentation.expand_labels(label_image, distance)`` on a 2-D label image
    (SK/segmentation/_expand_labels.py): every label grows by up to ``distance`` pixels into the background without
    overlapping its neighbours.  bool and integer dtypes; a numpy result has the input's dtype, as scikit-image's
    ``zeros_like`` gives it.  Labels must be non-negative and below 2**31 - 1.  A ``DeviceArray`` (int32, or the
    uint16 / uint8 a ``Pipeline`` uploads) stays on the device; its values are the caller's promise.

    Any float distance is exact (``hipops.expand_nmax``); ``distance < 0`` gives zeros.  Where pixels of several
    labels are equally near, the SMALLEST label is written: scipy's feature transform keeps whichever tied pixel its
    scan meets first, an artefact of its algorithm, while this rule is deterministic.  The support and every untied
    pixel equal scikit-image's.  Stacks are refused rather than treated as volumes (scikit-image would run a 3-D
    distance transform over them): map planes with ``Pipeline(parallel=True)`` or call ``hipops.expand_labels``."""
    if isinstance(label_image, DeviceArray):
        d = label_image
        if d.ndim != 2:
            raise ValueError("label_image must be a 2D array")
        if d.dtype == np.int32:
            return hipops.expand_labels(d, distance)
        if d.dtype not in (np.uint8, np.uint16):
            raise TypeError(f"expand_labels: device label images must be int32, uint16 or uint8, got {d.dtype}")
        grown = hipops.cast_labels(hipops.expand_labels(hipops.cast_labels(d, np.int32), distance), d.dtype)
        grown.is_bool = d.is_bool
        return grown
    a = np.asarray(label_image)
    if a.ndim != 2:
        raise ValueError("label_image must be a 2D array")
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"expand_labels: label_image must have a bool or integer dtype, got {a.dtype}")
    if a.size == 0:
        return np.zeros_like(a)
    if a.dtype.kind == "i" and int(a.min()) < 0:
        raise ValueError("label_image must have non-negative values")
    if int(a.max()) >= 2**31 - 1:
        raise ValueError("label values above 2**31 - 2 are not supported on the device path")
    d = get_context().asarray(a, dtype=np.int32)  # narrowed / widened while it moves into the staging buffer
    return hipops.expand_labels(d, distance).numpy(dtype=a.dtype)


@device_operator
def binary_fill_holes(mask, structure=None):
    """``scipy.ndimage.binary_fill_holes(mask, structure)`` on a 2-D mask: the holes of the foreground (``mask != 0``) are
    the background regions that cannot be reached from outside the image.  ``structure``: None or
    ``generate_binary_structure(2, 1)`` (the cross: holes are 4-connected background) or ``generate_binary_structure(2,
    2)`` (all-ones: 8-connected); other structures are refused.  A numpy bool / integer array gives a numpy bool array;
    a ``DeviceArray`` (a uint8 / bool mask, e.g. ``apply_threshold``'s result in a ``Pipeline``) stays on the device.
    Stacks are refused rather than treated as volumes (scipy would fill a 3-D volume): map planes with
    ``Pipeline(parallel=True)`` or call ``hipops.binary_fill_holes``."""
    st = hipops._fill_structure(structure)
    if isinstance(mask, DeviceArray):
        if mask.ndim != 2:
            raise ValueError("mask must be a 2D array")
        if mask.dtype != np.uint8:
            raise TypeError(f"binary_fill_holes: device masks must be uint8 / bool, got {mask.dtype}")
        return hipops.binary_fill_holes(mask, st)
    a = np.asarray(mask)
    if a.ndim != 2:
        raise ValueError("mask must be a 2D array")
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"binary_fill_holes: mask must have a bool or integer dtype, got {a.dtype}")
    if a.size == 0:
        return np.zeros(a.shape, dtype=bool)
    d = get_context().asarray(np.ascontiguousarray(a != 0))
    return hipops.binary_fill_holes(d, st).numpy()


def _area_filter_2d(which: str, mask, size, connectivity, integer_hint: str):
    """The 2-D front of both area filters: numpy bool in, numpy bool out; a ``DeviceArray`` stays on the device."""
    fn = getattr(hipops, which)
    if connectivity not in (1, 2):
        raise ValueError(f"{which}: connectivity must be 1 (4-connected) or 2 (8-connected), got {connectivity!r}")
    if isinstance(mask, DeviceArray):
        if mask.ndim != 2:
            raise ValueError("mask must be a 2D array")
        if mask.dtype != np.uint8:
            raise TypeError(f"{which}: device masks must be uint8 / bool, got {mask.dtype}")
        return fn(mask, size, connectivity)
    a = np.asarray(mask)
    if a.ndim != 2:
        raise ValueError("mask must be a 2D array")
    if a.dtype != np.bool_:
        if np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"{which}: scikit-image treats an integer array as a label image and filters it by label "
                            f"value, which this operator does not do; {integer_hint}")
        raise TypeError(f"{which}: mask must have a bool dtype, got {a.dtype}")
    if a.size == 0:
        return np.zeros(a.shape, dtype=bool)
    return fn(get_context().asarray(np.ascontiguousarray(a)), size, connectivity).numpy()


@device_operator
def remove_small_objects(mask, min_size: int = 64, connectivity: int = 1):
    """``skimage.morphology.remove_small_objects(mask, min_size, connectivity)`` on a 2-D bool mask: foreground
    components (``connectivity`` 1: 4-connected, 2: 8-connected) with fewer than ``min_size`` pixels are removed.  A
    numpy bool array gives a numpy bool array; a ``DeviceArray`` (a uint8 / bool mask, e.g. ``apply_threshold``'s result
    in a ``Pipeline``) stays on the device.  Integer numpy arrays are refused: scikit-image filters those by label
    value -- for label images use ``SegmentationMask.filter("area", ...)``.  Stacks are refused rather than treated as
    volumes: map planes with ``Pipeline(parallel=True)`` or call ``hipops.remove_small_objects``."""
    return _area_filter_2d("remove_small_objects", mask, min_size, connectivity,
                           'for label images use SegmentationMask.filter("area", ...), for masks pass a bool array')


@device_operator
def remove_small_holes(mask, area_threshold: int = 64, connectivity: int = 1):
    """``skimage.morphology.remove_small_holes(mask, area_threshold, connectivity)`` on a 2-D bool mask: background
    components with fewer than ``area_threshold`` pixels are filled, those on the image's frame included.  Types,
    connectivity and stacks as for ``remove_small_objects``; integer numpy arrays are refused, pass a bool array."""
    return _area_filter_2d("remove_small_holes", mask, area_threshold, connectivity, "pass a bool array (mask != 0)")


def _skeleton_2d(which: str, mask, call, result_dtype):
    """The 2-D front of ``skeletonize`` / ``skeleton_nodes``, with ``_area_filter_2d``'s rules for its input: a numpy bool
    array in, a numpy array of ``result_dtype`` out; a ``DeviceArray`` stays on the device."""
    if isinstance(mask, DeviceArray):
        if mask.ndim != 2:
            raise ValueError("mask must be a 2D array")
        if mask.dtype != np.uint8:
            raise TypeError(f"{which}: device masks must be uint8 / bool, got {mask.dtype}")
        return call(mask)
    a = np.asarray(mask)
    if a.ndim != 2:
        raise ValueError("mask must be a 2D array")
    if a.dtype != np.bool_:
        if np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"{which}: an integer array may be a label image, whose cells this operator would thin as one "
                            "mask; pass a bool array (mask != 0)")
        raise TypeError(f"{which}: mask must have a bool dtype, got {a.dtype}")
    if a.size == 0:
        return np.zeros(a.shape, dtype=result_dtype)
    return call(get_context().asarray(np.ascontiguousarray(a))).numpy(dtype=result_dtype)


@device_operator
def skeletonize(mask, max_iter: int | None = None):
    """Thinning of a 2-D bool mask to its centre lines by Zhang and Suen's rule, the one
    ``skimage.morphology.skeletonize`` cites for 2-D input (parity with scikit-image's 256-entry table is unpinned
    offline; ``hipops.skeletonize`` and include/amt_hip.h state the rule).  ``max_iter``: None runs to the fixed point, a
    positive integer stops after that many iterations.  A numpy bool array gives a numpy bool array; a ``DeviceArray``
    (a uint8 / bool mask, e.g. ``apply_threshold``'s result in a ``Pipeline``) stays on the device.  Integer numpy arrays
    and stacks are refused: map planes with ``Pipeline(parallel=True)`` or call ``hipops.skeletonize``."""
    if max_iter is None:
        k = 0
    else:
        if isinstance(max_iter, (bool, np.bool_)):
            raise TypeError("skeletonize: max_iter must be None or a positive integer, got a bool")
        try:
            k = int(max_iter.__index__())
        except AttributeError:
            raise TypeError(f"skeletonize: max_iter must be None or a positive integer, got {type(max_iter).__name__}") from None
        if k < 1:
            raise ValueError(f"skeletonize: max_iter must be None or a positive integer, got {k}")
    return _skeleton_2d("skeletonize", mask, lambda d: hipops.skeletonize(d, k), bool)


@device_operator
def skeleton_nodes(mask, connectivity: int = 2):
    """The neighbour class of every pixel of a 2-D bool mask, usually a skeleton: 0 off the mask, else 1 + the number of
    set neighbours (``connectivity`` 2: eight neighbours -- 1 an isolated pixel, 2 an end, 3 a path pixel, 4 and more a
    junction; 1: the four edge neighbours).  A numpy bool array gives a numpy uint8 array; a ``DeviceArray`` stays on the
    device.  Input rules as for ``skeletonize``."""
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (1, 2):
        raise ValueError(f"skeleton_nodes: connectivity must be 1 (four neighbours) or 2 (eight), got {connectivity!r}")
    return _skeleton_2d("skeleton_nodes", mask, lambda d: hipops.neighbor_classes(d, connectivity), np.uint8)


@device_operator
def skeletonize_labels(label_image, max_iter: int | None = None):
    """The skeleton of every cell of a 2-D label image, touching cells included: ``skeletonize``'s rule, but a neighbour
    counts only when it carries the same label as the pixel, which gives exactly the skeletons the cells would get one
    by one (``hipops.label_skeleton`` and include/amt_hip.h state the rule; parity with scikit-image per label is
    unpinned offline).  The result holds the label on the skeleton of its cell and 0 elsewhere.  Every non-zero value is
    a label.  A numpy integer label image gives an array of the same dtype (its values must fit int32); a
    ``DeviceArray`` (int32, or the uint16 / uint8 a ``Pipeline`` uploads) stays on the device.  bool arrays are masks:
    use ``skeletonize``.  ``max_iter`` as for ``skeletonize``.  Stacks are refused: map planes with
    ``Pipeline(parallel=True)`` or call ``hipops.label_skeleton``."""
    if max_iter is None:
        k = 0
    else:
        if isinstance(max_iter, (bool, np.bool_)):
            raise TypeError("skeletonize_labels: max_iter must be None or a positive integer, got a bool")
        try:
            k = int(max_iter.__index__())
        except AttributeError:
            raise TypeError("skeletonize_labels: max_iter must be None or a positive integer, got "
                            f"{type(max_iter).__name__}") from None
        if k < 1:
            raise ValueError(f"skeletonize_labels: max_iter must be None or a positive integer, got {k}")
    if isinstance(label_image, DeviceArray):
        d = label_image
        if d.ndim != 2:
            raise ValueError("label_image must be a 2D array")
        if d.is_bool:
            raise TypeError("skeletonize_labels: a bool array is a mask, not a label image; use skeletonize")
        if d.dtype == np.int32:
            return hipops.label_skeleton(d, k)
        if d.dtype not in (np.uint8, np.uint16):
            raise TypeError(f"skeletonize_labels: device label images must be int32, uint16 or uint8, got {d.dtype}")
        if d.size == 0:
            return d
        return hipops.cast_labels(hipops.label_skeleton(hipops.cast_labels(d, np.int32), k), d.dtype)
    a = np.asarray(label_image)
    if a.ndim != 2:
        raise ValueError("label_image must be a 2D array")
    if a.dtype == np.bool_:
        raise TypeError("skeletonize_labels: a bool array is a mask, not a label image; use skeletonize")
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"skeletonize_labels: label_image must have an integer dtype, got {a.dtype}")
    if a.size == 0:
        return np.zeros_like(a)
    if int(a.min()) < -2**31 or int(a.max()) > 2**31 - 1:
        raise ValueError("skeletonize_labels: label values must fit int32 on the device path")
    d = get_context().asarray(a, dtype=np.int32)
    return hipops.label_skeleton(d, k).numpy(dtype=a.dtype)


_RECON_DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float64))


def _recon_operand(op: str, x, what: str):
    """-> (host array or None, DeviceArray or None, caller's dtype) of a 2-D uint8 / uint16 / float64 image"""
    if isinstance(x, DeviceArray):
        if x.ndim != 2:
            raise ValueError(f"{what} must be a 2D array")
        if x.dtype not in (np.uint16, np.float64):
            raise TypeError(f"{op}: device arrays must be uint16 or float64, got {x.dtype}")
        return None, x, x.dtype
    a = np.asarray(x)
    if a.ndim != 2:
        raise ValueError(f"{what} must be a 2D array")
    if a.dtype not in _RECON_DTYPES:
        raise TypeError(f"{op}: {what} must be uint8, uint16 or float64, got {a.dtype}")
    return a, None, a.dtype


def _recon_upload(a: np.ndarray) -> DeviceArray:
    return get_context().asarray(np.ascontiguousarray(a.astype(np.uint16) if a.dtype == np.uint8 else a))


@device_operator
def reconstruction(seed, mask, method: str = "dilation", footprint=None, offset=None):
    """``skimage.morphology.reconstruction(seed, mask, method, footprint)`` on 2-D images: by dilation, ``seed`` spreads
    under ``mask`` until nothing changes (the least R >= seed with R = min(mask, max over the footprint of R)); by
    erosion the dual.  ``footprint``: None (3 x 3 all-ones, scikit-image's default), the 3 x 3 cross or all-ones;
    ``offset`` other than None is refused.  uint8 (numpy only), uint16 and float64 images of one dtype; numpy in gives
    numpy out in that dtype, a ``DeviceArray`` seed stays on the device (``mask`` may be either).  Stacks are refused:
    map planes with ``Pipeline(parallel=True)`` or call ``hipops.reconstruction``.  NaN is not supported."""
    dil = hipops._recon_method(method)
    fp = hipops._recon_footprint(footprint)
    if offset is not None:
        raise ValueError("reconstruction: offset is not supported (the footprint is anchored at its centre)")
    hs, ds, dts = _recon_operand("reconstruction", seed, "seed")
    hm, dm, dtm = _recon_operand("reconstruction", mask, "mask")
    if np.dtype(dts) != np.dtype(dtm):
        raise TypeError(f"reconstruction: seed ({dts}) and mask ({dtm}) must have the same dtype")
    shape_s = hs.shape if hs is not None else tuple(ds.shape)
    shape_m = hm.shape if hm is not None else tuple(dm.shape)
    if tuple(shape_s) != tuple(shape_m):
        raise ValueError(f"reconstruction: seed {tuple(shape_s)} and mask {tuple(shape_m)} must have the same shape")
    if hs is not None and hm is not None:
        if hs.size == 0:
            return np.zeros(hs.shape, dtype=hs.dtype)
        if dil and np.any(hs > hm):
            raise ValueError("Intensity of seed image must be less than that of the mask image for reconstruction by "
                             "dilation.")
        if not dil and np.any(hs < hm):
            raise ValueError("Intensity of seed image must be greater than that of the mask image for reconstruction by "
                             "erosion.")
    elif hs is not None and hs.size == 0:
        return np.zeros(hs.shape, dtype=hs.dtype)
    if ds is None:
        ds = _recon_upload(hs)
    if dm is None:
        dm = _recon_upload(hm).on(ds.ctx)
    if ds.dtype != dm.dtype:
        raise TypeError(f"reconstruction: seed ({ds.dtype}) and mask ({dm.dtype}) must have the same dtype on the device")
    r = hipops.reconstruction(ds, dm, method, fp)
    return r.numpy(dtype=hs.dtype) if hs is not None else r


def _h_extrema_2d(op: str, image, h, footprint, maxima: bool):
    fp = hipops._recon_footprint(footprint)
    ha, da, dt = _recon_operand(op, image, "image")
    if isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, float, np.integer, np.floating)) or not np.isfinite(h):
        raise ValueError(f"{op}: h must be a finite number, got {h!r}")
    if h == 0:
        raise ValueError("h = 0 is ambiguous, use local_maxima() or local_minima() instead")
    if h < 0:
        raise ValueError(f"{op}: h must be positive, got {h!r}")
    if np.dtype(dt) != np.float64 and float(h) != int(h):
        raise ValueError(f"{op}: h must be an integer for an integer image, got {h!r}")
    if ha is not None:
        if ha.size == 0:
            return np.zeros(ha.shape, dtype=np.uint8)
        lo, hi = ha.min(), ha.max()
    else:
        if da.size == 0:
            return da.ctx.zeros(da.shape, np.uint8)
        lo, hi = _min_max(da)
    if float(h) > float(hi) - float(lo):  # scikit-image's early exit: no extremum can stand that high
        return np.zeros(ha.shape, dtype=np.uint8) if ha is not None else da.ctx.zeros(da.shape, np.uint8)
    d = da if da is not None else _recon_upload(ha)
    m = (hipops.h_maxima if maxima else hipops.h_minima)(d, h, fp)
    return m.numpy(dtype=np.uint8) if ha is not None else m


@device_operator
def h_maxima(image, h, footprint=None):
    """``skimage.morphology.h_maxima(image, h, footprint)`` on a 2-D image: 1 where a maximum stands at least ``h`` above
    its surroundings, as ``np.uint8`` (a ``DeviceArray`` stays on the device as a uint8 / bool mask).  ``footprint`` and
    dtypes as for ``reconstruction``.  ``h`` must be positive, and an integer for an integer image (ValueError);
    ``h`` above the image's range gives all zeros.  Integer images follow scikit-image's rule (residue >= h); float64
    images mark the pixels where the reconstruction equals the seed ``image - h`` exactly (``hipops.h_maxima``)."""
    return _h_extrema_2d("h_maxima", image, h, footprint, True)


@device_operator
def h_minima(image, h, footprint=None):
    """``skimage.morphology.h_minima(image, h, footprint)``: the dual of ``h_maxima``."""
    return _h_extrema_2d("h_minima", image, h, footprint, False)


# ---- Z-stacks: (Z, Y, X) in, one (Y, X) plane out (hipops.z_project .. z_take; include/amt_hip.h states the rules) -----
_Z_DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float64))
FOCUS_METHODS = ("laplacian_variance", "normalized_variance", "brenner")
_EDF_SMOOTH = (0, 3, 5, 7, 9, 11, 13, 15)


def _z_batch(op: str, stack, integer_only: bool = False):
    """-> ((1, Z, Y, X) DeviceArray, was_numpy) of a (Z, Y, X) stack, refused before any device access"""
    if isinstance(stack, DeviceArray):
        d, was_numpy = stack, False
    else:
        d, was_numpy = np.asarray(stack), True
    if d.ndim != 3:
        raise ValueError(f"{op}: stack must be a (Z, Y, X) array, got shape {tuple(d.shape)}")
    if d.dtype not in _Z_DTYPES or (integer_only and d.dtype == np.float64):
        want = "uint8 or uint16 (focus is judged on raw data)" if integer_only else "uint8, uint16 or float64"
        raise TypeError(f"{op}: stack must be {want}, got {d.dtype}")
    if min(d.shape) < 1:
        raise ValueError(f"{op}: stack must not be empty, got shape {tuple(d.shape)}")
    if was_numpy:
        d = get_context().asarray(np.ascontiguousarray(d))
    return d.reshape((1,) + tuple(d.shape)), was_numpy


def _z_plane(d: DeviceArray, was_numpy: bool):
    """The (1, Y, X) result of a batch of one as a (Y, X) plane"""
    d = d.reshape(d.shape[1:])
    return d.numpy() if was_numpy else d


def _focus_method(op: str, method) -> str:
    if method not in FOCUS_METHODS:
        raise ValueError(f"{op}: method must be one of {FOCUS_METHODS}, got {method!r}")
    return method


def _scores_from_sums(sums, n: int, method: str) -> np.ndarray:
    """float64 scores of the planes whose integer sums are the rows of ``sums`` (hipops.focus_sums), n pixels a plane:
    exact rationals, rounded once"""
    from fractions import Fraction

    out = np.empty(len(sums), dtype=np.float64)
    for z, row in enumerate(sums):
        s, ss, lap, br = (int(v) for v in row)
        if method == "laplacian_variance":
            # the Laplacian sums to 0 under edge replication (the differences telescope): its mean square IS its variance
            out[z] = float(Fraction(lap, n))
        elif method == "normalized_variance":
            out[z] = float(Fraction(n * ss - s * s, n * s)) if s else 0.0
        else:
            out[z] = float(br)
    return out


@device_operator
def z_project(stack, method: str = "max"):
    """The maximum, minimum or mean projection of a (Z, Y, X) uint8 / uint16 / float64 stack along z: numpy's
    ``stack.max(axis=0)`` / ``min`` / ``mean`` bit for bit (the mean is float64).  numpy in gives numpy out; a
    ``DeviceArray`` stays on the device."""
    if method not in ("max", "min", "mean"):
        raise ValueError(f"z_project: method must be 'max', 'min' or 'mean', got {method!r}")
    d, was_numpy = _z_batch("z_project", stack)
    return _z_plane(hipops.z_project(d, method), was_numpy)


def focus_scores(stack, method: str = "laplacian_variance") -> Float64Array:
    """One focus score per plane of a (Z, Y, X) uint8 / uint16 stack -> float64 (Z,), larger = sharper.  The device makes
    four exact integer sums per plane (``hipops.focus_sums``); the score is formed from them on the host in exact
    rationals and rounded once.  With n = Y * X: ``"laplacian_variance"`` = sum(L^2) / n, the variance of the
    four-neighbour Laplacian L under edge replication (whose sum is identically 0); ``"normalized_variance"`` =
    (n sum(P^2) - sum(P)^2) / (n sum(P)), 0.0 for an all-zero plane; ``"brenner"`` = sum of (P(y, x+2) - P(y, x))^2."""
    _focus_method("focus_scores", method)
    d, _ = _z_batch("focus_scores", stack, integer_only=True)
    return _scores_from_sums(hipops.focus_sums(d).numpy()[0], d.shape[2] * d.shape[3], method)


@device_operator
def best_focus(stack, method: str = "laplacian_variance", return_index: bool = False):
    """The plane of a (Z, Y, X) uint8 / uint16 stack with the largest ``focus_scores``, the smallest z among equals; with
    ``return_index`` the pair (plane, z).  On the device the plane is a view of the stack, not a copy."""
    _focus_method("best_focus", method)
    d, was_numpy = _z_batch("best_focus", stack, integer_only=True)
    z = int(np.argmax(_scores_from_sums(hipops.focus_sums(d).numpy()[0], d.shape[2] * d.shape[3], method)))
    plane = np.asarray(stack)[z] if was_numpy else stack[z]
    return (plane, z) if return_index else plane


def _edf_args(radius, smooth):
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= 15:
        raise ValueError(f"extended_depth_of_field: radius must be an integer in 0..15, got {radius!r}")
    if isinstance(smooth, (bool, np.bool_)) or not isinstance(smooth, (int, np.integer)) or int(smooth) not in _EDF_SMOOTH:
        raise ValueError(f"extended_depth_of_field: smooth must be 0 or an odd integer in 3..15, got {smooth!r}")
    return int(radius), int(smooth)


def _edf_batch(d: DeviceArray, radius: int, smooth: int, need_index: bool):
    """-> (composite, index map or None) of an (N, Z, Y, X) batch"""
    if smooth == 0 and not need_index:
        return hipops.focus_stack(d, radius), None
    index = hipops.focus_index(d, radius)
    if smooth:
        index = hipops.median(index, np.ones((smooth, smooth), np.uint8), mode="nearest")
    return hipops.z_take(d, index), index


@device_operator
def extended_depth_of_field(stack, radius: int = 4, smooth: int = 0, return_index: bool = False):
    """The all-in-focus composite of a (Z, Y, X) uint8 / uint16 stack: every pixel comes from the plane where the squared
    Laplacian, summed over the (2 radius + 1)^2 window around it, is largest (the smallest z among equals;
    ``hipops.focus_index`` states the rule, which is this package's own).  ``smooth``: 0, or the odd side (3..15) of a
    median filter of the index map (``mode="nearest"``) before the pixels are taken.  With ``return_index`` the pair
    (composite, uint16 index map).  numpy in gives numpy out; a ``DeviceArray`` stays on the device."""
    radius, smooth = _edf_args(radius, smooth)
    d, was_numpy = _z_batch("extended_depth_of_field", stack, integer_only=True)
    plane, index = _edf_batch(d, radius, smooth, bool(return_index))
    if return_index:
        return _z_plane(plane, was_numpy), _z_plane(index, was_numpy)
    return _z_plane(plane, was_numpy)


def _global_threshold(d: DeviceArray, method: str, kwargs: dict) -> float:
    """Threshold VALUE for the histogram-based methods: histogram on the device, selection on <= 65,536 counts."""
    nbins = int(kwargs.pop("nbins", 256))
    if d.dtype == np.uint16:
        hist = hipops.histogram_u16(d).numpy()[0]
        counts, centers = _thresholds.counts_centers_u16(hist)
    else:
        h, mm = hipops.histogram_f64(d, nbins)
        mmv = mm.numpy()[0]
        counts, centers = _thresholds.counts_centers_f64(h.numpy()[0], mmv[0], mmv[1])
    if method == "yen":
        return _thresholds.yen(counts, centers)
    if method == "isodata":
        return _thresholds.isodata(counts, centers)
    if method == "triangle":
        return _thresholds.triangle(counts, centers)
    if method == "minimum":
        return _thresholds.minimum(counts, centers, **kwargs)
    raise AssertionError(method)


def _mean_threshold(d: DeviceArray) -> float:
    if d.dtype == np.uint16:
        hist = hipops.histogram_u16(d).numpy()[0]
        counts, centers = _thresholds.counts_centers_u16(hist)
        return _thresholds.mean_from_hist(counts, centers)
    inf = d.ctx.asarray(np.array([np.inf]))
    s = hipops.masked_sums(d, inf).numpy()[0]
    return s[0] / s[1]


def _li_threshold(d: DeviceArray, tolerance=None, initial_guess=None) -> float:
    """``skimage.filters.threshold_li`` (SK thresholding.py:642-707).  Integer images: exact, from the
    histogram.  Float images: every iteration's two class means come from one device reduction."""
    if d.dtype == np.uint16:
        hist = hipops.histogram_u16(d).numpy()[0]
        counts, centers = _thresholds.counts_centers_u16(hist)
        return _thresholds.li_from_hist(counts, centers, tolerance, initial_guess)
    ctx = d.ctx
    image_min, image_max = _min_max(d)
    if tolerance is None:
        # smallest gap between distinct values / 2: for float images take it from the data's own resolution
        # (scikit-image sorts the unique values; any tolerance below the true gap yields the same fixed point)
        tolerance = np.spacing(max(abs(image_min), abs(image_max))) / 2
    tot = hipops.masked_sums(d, ctx.asarray(np.array([np.inf]))).numpy()[0]
    t_next = (tot[0] / tot[1]) if initial_guess is None else float(initial_guess)
    t_curr = t_next - 2 * tolerance - 1.0
    # work in the original value space: means shift by image_min exactly as scikit-image's (image - min)
    for _ in range(10000):
        if abs(t_next - t_curr) <= tolerance:
            break
        t_curr = t_next
        s = hipops.masked_sums(d, ctx.asarray(np.array([t_curr]))).numpy()[0]
        mean_back = s[0] / s[1] - image_min
        mean_fore = s[2] / s[3] - image_min
        t_next = (mean_back - mean_fore) / (np.log(mean_back) - np.log(mean_fore)) + image_min
    return t_next


def _local_threshold(d: DeviceArray, block_size, method="gaussian", offset=0, mode="reflect", param=None, cval=0):
    """``skimage.filters.threshold_local`` (SK thresholding.py:206-236) -> float64 threshold image on the device."""
    if block_size % 2 == 0:
        raise ValueError(
            "The kwarg ``block_size`` must be odd! Given ``block_size`` {0} is even.".format(block_size)
        )
    if method == "gaussian":
        sigma = (block_size - 1) / 6.0 if param is None else param
        # scikit-image filters EVERY axis of an n-D image (ndi.gaussian_filter on the whole stack)
        t = hipops.gaussian_nd(d, sigma, mode=mode, cval=cval, scale=1.0)
    elif d.ndim != 2:
        raise NotImplementedError(
            f"threshold_local(method='{method}') filters every axis of an n-D image in scikit-image; the device path "
            "does that for method='gaussian' only -- map a stack over its first axis with Pipeline(parallel=True)"
        )
    elif method == "mean":
        t = hipops.uniform_filter(d, block_size, mode=mode, cval=cval)
    elif method == "median":
        t = hipops.median(d, np.ones((block_size, block_size), np.uint8), mode=mode, cval=cval)
        if t.dtype != np.float64:
            t = hipops.to_float64(t)
    else:
        raise ValueError(f"threshold_local method '{method}' is not supported on the device path")
    if offset:
        t = hipops.add_scalar(t, -float(offset))
    return t


def otsu_threshold_value(intensities, nbins: int = 256) -> float:
    """The value ``t`` behind ``apply_threshold(intensities, "otsu")``: that mask is ``intensities > t``, in the image's
    own value space.  The same device code picks it -- per dtype as ``apply_threshold`` does (module docstring):
    ``hipops.threshold_otsu`` for images that travel as uint16 or float64, the integer histograms for wider integers.
    A constant image gives its value (nothing lies above it, as ``apply_threshold`` answers all False); an empty one
    NaN."""
    if not isinstance(intensities, DeviceArray) and np.asarray(intensities).size == 0:
        return float("nan")
    shifted = [0]
    d, _ = _to_device(intensities, "apply_threshold", integer_histogram=True, shifted=shifted)
    offset = int(shifted[0])
    wide_bins = int(shifted[1]) if len(shifted) > 1 else 0
    d = _flat(d)
    lo, hi = _min_max(d)
    if lo == hi:
        return float(lo) + (0 if wide_bins else offset)
    if wide_bins:  # x > t on the float64 image
        counts = hipops.histogram_range(d, offset, wide_bins).numpy()[0].astype(np.int64)
        return float(_thresholds.otsu(counts, np.arange(offset, offset + wide_bins)))
    if offset:  # x - min > floor(t) - min  <=>  x > floor(t) for integers
        counts, centers = _thresholds.counts_centers_u16(hipops.histogram_u16(d).numpy()[0])
        t = _thresholds.otsu(counts, centers + offset)
        return float(t) if np.isnan(t) else float(np.floor(t))
    return float(hipops.threshold_otsu(d, nbins=int(nbins)).numpy()[0])


@device_operator
def apply_threshold(
    intensities: ScalarArray,
    method: Literal[
        "otsu", "li", "yen", "isodata", "mean", "minimum", "triangle", "local", "niblack", "sauvola"
    ] = "otsu",
    **kwargs,
) -> BoolArray:
    """``intensities > threshold_<method>(intensities, **kwargs)`` (R/operations.py:135-216); boolean result."""
    if not isinstance(intensities, DeviceArray) and np.asarray(intensities).size == 0:
        return np.zeros_like(intensities, dtype=bool)
    method_lower = method.lower()
    if method_lower not in _SUPPORTED_METHODS:
        raise ValueError(
            f"Unsupported thresholding method: '{method}'. "
            f"Supported methods: {', '.join(_SUPPORTED_METHODS)}"
        )
    src_dtype = intensities.dtype if isinstance(intensities, DeviceArray) else np.asarray(intensities).dtype
    shifted = [0]
    hist_method = method_lower in ("otsu", "yen", "isodata", "triangle", "minimum", "mean", "li")
    d, was_numpy = _to_device(intensities, "apply_threshold", integer_histogram=hist_method,
                              shifted=shifted if hist_method else None)
    offset = int(shifted[0])
    wide_bins = int(shifted[1]) if len(shifted) > 1 else 0  # integer image beyond a 65,536-value range
    shape = d.shape
    if d.ndim != 2 and method_lower not in ("local", "niblack", "sauvola"):
        d = _flat(d)  # global methods: ONE threshold from the histogram of the whole stack
    ctx = d.ctx
    lo, hi = _min_max(d)
    if lo == hi:  # constant image (R/operations.py:201-202)
        z = np.zeros(shape, dtype=bool)
        return z if was_numpy else ctx.asarray(z)
    kw = dict(kwargs)
    if wide_bins:
        # scikit-image's histogram of such an image has one bin per integer from min to max; the counts come from the
        # device, the selection runs on them with the same numpy expressions, and x > t is exact on the float64 image
        counts = hipops.histogram_range(_flat(d), offset, wide_bins).numpy()[0].astype(np.int64)
        centers = np.arange(offset, offset + wide_bins)
        if method_lower == "otsu":
            kw.pop("nbins", None)
            t = _thresholds.otsu(counts, centers)
        elif method_lower == "mean":
            t = _thresholds.mean_from_hist(counts, centers)
        elif method_lower == "li":
            t = _thresholds.li_from_hist(counts, centers, wrap_dtype=src_dtype, **kw)
        else:
            kw.pop("nbins", None)
            t = getattr(_thresholds, method_lower)(counts, centers, **kw)
        if np.isnan(t):
            z = np.zeros(shape, dtype=bool)
            return z if was_numpy else ctx.asarray(z)
        mask = hipops.greater_than(d, ctx.asarray(np.array([float(t)])))
    elif offset:
        # integer image beyond uint16 whose range fits: histogram of x - min on the device, the reference's threshold
        # from (counts, arange(min, max + 1)) on the host, and x > t  <=>  x - min > floor(t) - min for integers
        hist = hipops.histogram_u16(d).numpy()[0]
        counts, centers = _thresholds.counts_centers_u16(hist)
        centers = centers + offset
        if method_lower == "otsu":
            kw.pop("nbins", None)
            t = _thresholds.otsu(counts, centers)
        elif method_lower == "mean":
            t = _thresholds.mean_from_hist(counts, centers)
        elif method_lower == "li":
            t = _thresholds.li_from_hist(counts, centers, wrap_dtype=src_dtype, **kw)
        else:
            kw.pop("nbins", None)
            t = getattr(_thresholds, method_lower)(counts, centers, **kw)
        if np.isnan(t):  # x > nan is False everywhere (li on a signed image that wrapped in its own dtype)
            z = np.zeros(shape, dtype=bool)
            return z if was_numpy else ctx.asarray(z)
        mask = hipops.greater_than(d, ctx.asarray(np.array([float(int(np.floor(t)) - offset)])))
    elif method_lower == "otsu":
        thr = hipops.threshold_otsu(d, nbins=int(kw.pop("nbins", 256)))
        mask = hipops.greater_than(d, thr)
    elif method_lower in ("yen", "isodata", "triangle", "minimum"):
        t = _global_threshold(d, method_lower, kw)
        mask = hipops.greater_than(d, ctx.asarray(np.array([float(t)])))
    elif method_lower == "mean":
        mask = hipops.greater_than(d, ctx.asarray(np.array([float(_mean_threshold(d))])))
    elif method_lower == "li":
        mask = hipops.greater_than(d, ctx.asarray(np.array([float(_li_threshold(d, **kw))])))
    elif method_lower == "local":
        if "block_size" not in kw:
            raise TypeError("threshold_local() missing 1 required positional argument: 'block_size'")
        mask = hipops.greater_than_image(d, _local_threshold(d, **kw))
    else:  # niblack / sauvola (SK/filters/thresholding.py:967-1087)
        if method_lower == "sauvola" and kw.get("r") is None:
            kw["r"] = _sauvola_r(src_dtype)  # half the range of the CALLER's dtype, not of the uint16 it travels as
        # the window spans EVERY axis of a stack, as in scikit-image (window_size: one odd integer or one per axis)
        mask = hipops.greater_than_image(d, hipops.window_threshold(d, method=method_lower, nd=d.ndim > 2, **kw))
    if mask.shape != shape:
        is_bool = mask.is_bool
        mask = mask.reshape(shape)
        mask.is_bool = is_bool
    return _result(mask, was_numpy)


# ---- spot detection (hipops.local_maxima / mask_list / spot_measure / take_at) ----------------------------------------
def _spot_arg(what: str, name: str, value, lo: int, hi: int) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{what}: {name} must be an integer in {lo}..{hi}, got {value!r}")
    return int(value)


def _spot_number(what: str, name: str, value, finite: bool = False) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or np.isnan(float(value)) or (finite and not np.isfinite(float(value))):
        raise ValueError(f"{what}: {name} must be a {'finite ' if finite else ''}number, got {value!r}")
    return float(value)


def _spot_plane(what: str, image, name: str = "image"):
    """-> ((1, Y, X) uint16 / float64 DeviceArray, was_numpy) of one 2-D image; a numpy image with NaN is refused"""
    if not isinstance(image, DeviceArray):
        a = np.asarray(image)
        if a.ndim != 2:
            raise ValueError(f"{what}: {name} must be 2-D, got shape {a.shape}")
        if a.size == 0:
            raise ValueError(f"{what}: {name} is empty")
        if a.dtype.kind == "f" and np.isnan(a).any():
            raise ValueError(f"{what}: {name} contains NaN, which the local-maximum rule does not order")
        if a.dtype.kind not in "buif":
            raise TypeError(f"{what}: {name} has dtype {a.dtype}, which is not supported")
    elif image.ndim != 2:
        raise ValueError(f"{what}: {name} must be 2-D, got shape {image.shape}")
    d, was_numpy = _to_device(image, what)
    return d.reshape((1,) + tuple(d.shape)), was_numpy


def _spot_list_of(mask: DeviceArray, capacity: int):
    """-> ((1, K + 1) list of the K set pixels of a (1, Y, X) mask, K): one 4-byte look at the count, then a view"""
    spots = hipops.mask_list(mask, capacity)
    flat = spots.reshape(spots.size)
    count = int(flat[0:1].numpy()[0])
    if count > capacity:
        raise AssertionError(f"{count} marks in a plane that can hold {capacity}")
    keep = max(count, 1)  # a list has at least capacity 1; its one entry is -1 then
    return flat[0:keep + 1].reshape((1, keep + 1)), count


@device_operator
def peak_local_max(image, min_distance: int = 1, threshold_abs=None, threshold_rel=None, exclude_border=True,
                   num_peaks=np.inf, labels=None, footprint=None, p_norm=None, num_peaks_per_label=None):
    """The coordinates of the local maxima of a 2-D image -> (K, 2) int64 ``(row, col)``, sorted by descending value with
    raster order among equals (``skimage.feature.peak_local_max``'s signature and threshold rule).  A pixel is a peak iff
    it exceeds the threshold, is >= every pixel within ``min_distance`` (Chebyshev) and > those that precede it in raster
    order (``hipops.local_maxima`` states the rule, which is this package's own: a plateau yields ONE peak, at its first
    pixel, and peaks are more than ``min_distance`` apart; parity with scikit-image on plateaus is unpinned offline).
    The threshold is ``threshold_abs``, or the image minimum when it is None; with ``threshold_rel`` the larger of that
    and ``threshold_rel * image.max()``.  ``exclude_border``: True = ``min_distance``, False = 0, an int = that width.
    ``num_peaks`` keeps the first so many.  The maxima are found on the device; the short list is sorted on the host.
    ``labels=``, ``footprint=``, ``p_norm=`` and ``num_peaks_per_label=`` are not implemented: see ``detect_spots`` and
    ``SegmentationMask.cell_spots`` for spots per label."""
    for name, value in (("labels", labels), ("footprint", footprint), ("p_norm", p_norm),
                        ("num_peaks_per_label", num_peaks_per_label)):
        if value is not None:
            raise NotImplementedError(f"peak_local_max: {name}= is not implemented; use detect_spots(labels=) or "
                                      "SegmentationMask.cell_spots for spots per label")
    r = _spot_arg("peak_local_max", "min_distance", min_distance, 1, 15)
    if isinstance(exclude_border, (bool, np.bool_)):
        b = r if exclude_border else 0
    else:
        b = _spot_arg("peak_local_max", "exclude_border", exclude_border, 0, 2**31 - 1)
    if num_peaks != np.inf:
        num_peaks = _spot_arg("peak_local_max", "num_peaks", num_peaks, 0, 2**62)
    for name, value in (("threshold_abs", threshold_abs), ("threshold_rel", threshold_rel)):
        if value is not None:
            _spot_number("peak_local_max", name, value)
    d, _ = _spot_plane("peak_local_max", image)
    t = None if threshold_abs is None else float(threshold_abs)
    if t is None or threshold_rel is not None:
        mm = hipops.minmax(d if d.dtype == np.float64 else hipops.to_float64(d)).numpy()[0]
        if t is None:
            t = float(mm[0])
        if threshold_rel is not None:
            t = max(t, float(threshold_rel) * float(mm[1]))
    H, W = d.shape[1:]
    spots, count = _spot_list_of(hipops.local_maxima(d, r, t, b), hipops.spot_capacity(H, W, r))
    index = spots.numpy()[0, 1:1 + count].astype(np.int64)
    value = hipops.take_at(d, spots).numpy()[0, :count]
    order = np.argsort(-value.astype(np.float64), kind="stable")  # stable: raster order among equals
    index = index[order]
    if num_peaks != np.inf:
        index = index[:num_peaks]
    return np.stack([index // W, index % W], axis=1).reshape(-1, 2)


SPOT_KEYS = ("row", "col", "y", "x", "response", "intensity_sum", "background_mean", "intensity_net")


def _spot_table(response: DeviceArray, intensity: DeviceArray, r: int, t: float, b: int, k: int, labels: DeviceArray | None):
    """The table of ``detect_spots`` from (1, Y, X) planes on the device"""
    from . import _hip

    H, W = response.shape[1:]
    spots, count = _spot_list_of(hipops.local_maxima(response, r, t, b), hipops.spot_capacity(H, W, r))
    index = spots.numpy()[0, 1:1 + count].astype(np.int64)
    col = {name: i for i, name in enumerate(_hip.SPOT_COLS)}
    on_response = hipops.spot_measure(response, spots, k).numpy()[0, :count]
    on_intensity = on_response if intensity is response else hipops.spot_measure(intensity, spots, k).numpy()[0, :count]
    row, column = index // W, index % W
    with np.errstate(invalid="ignore", divide="ignore"):
        background = on_intensity[:, col["ring_sum"]] / on_intensity[:, col["ring_n"]]
    total = on_intensity[:, col["sum"]].copy()
    out = {"row": row, "col": column, "y": row + on_response[:, col["dy"]], "x": column + on_response[:, col["dx"]],
           "response": on_response[:, col["value"]].copy(), "intensity_sum": total, "background_mean": background,
           "intensity_net": total - on_intensity[:, col["n"]] * background}
    if labels is not None:
        out["label"] = hipops.take_at(labels, spots).numpy()[0, :count].astype(np.int64)
    return out


def _spot_labels(what: str, labels, shape, ctx):
    """``labels=`` of ``detect_spots`` as a (1, Y, X) int32 device plane: an integer label array, a DeviceArray or a
    ``SegmentationMask`` (whose device plane is used where it is)"""
    if labels is None:
        return None
    if hasattr(labels, "_label_plane"):
        plane = labels._label_plane()[0]
    elif isinstance(labels, DeviceArray):
        plane = labels
    else:
        a = np.asarray(labels)
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"{what}: labels must be an integer label array or a SegmentationMask, got dtype {a.dtype}")
        if a.size and (int(a.min()) < -2**31 or int(a.max()) >= 2**31):
            raise ValueError(f"{what}: labels must fit int32")
        plane = None if tuple(a.shape) != tuple(shape) else ctx.asarray(np.ascontiguousarray(a, dtype=np.int32))
    if plane is None or tuple(plane.shape[-2:]) != tuple(shape) or plane.size != shape[0] * shape[1]:
        raise ValueError(f"{what}: labels must have the image's shape {tuple(shape)}")
    if plane.dtype != np.int32:
        raise TypeError(f"{what}: device labels must be int32, got {plane.dtype}")
    return plane.reshape((1,) + tuple(shape))


@device_operator
def detect_spots(image, sigma=1.5, min_distance: int = 2, threshold=None, snr: float = 5.0, radius: int = 2,
                 exclude_border=None, labels=None, intensity=None):
    """Puncta (smFISH dots, foci, vesicles) of a 2-D image as a table: a dict of equal-length arrays in raster order --
    ``row``, ``col`` (int64), ``y``, ``x`` (float64: the pixel plus its sub-pixel offset), ``response``,
    ``intensity_sum``, ``background_mean``, ``intensity_net`` (float64) and, with ``labels=`` (an integer label array or
    a ``SegmentationMask``), ``label`` (int64, 0 on background).

    The response is ``difference_of_gaussians(image, sigma, 1.6 * sigma)``, with ``sigma=None`` the image itself.  Spots
    are the local maxima of the response within ``min_distance`` (``hipops.local_maxima``: this package's own rule, one
    mark per plateau) above ``threshold`` -- a number on the response, or with None
    ``p50 + snr * (p75 - p25) / 1.349`` of the response: a robust background level plus ``snr`` robust standard
    deviations, from three device percentiles and host float64 arithmetic -- and at least ``exclude_border`` pixels (None =
    ``min_distance``) from the edges.  The offsets are the vertex of the parabola through three samples of the response
    per axis (``hipops.spot_measure``).  ``intensity_sum`` is the sum of ``intensity`` (default: ``image``) over the
    (2 radius + 1)^2 window, ``background_mean`` its mean over the frame at distance radius + 1 .. radius + 2, and
    ``intensity_net`` the sum minus window pixels x background.  Everything pixel-sized runs on the device; what comes
    back is the short list."""
    what = "detect_spots"
    r = _spot_arg(what, "min_distance", min_distance, 1, 15)
    k = _spot_arg(what, "radius", radius, 0, 15)
    b = r if exclude_border is None else _spot_arg(what, "exclude_border", exclude_border, 0, 2**31 - 1)
    if sigma is not None and not _spot_number(what, "sigma", sigma, finite=True) > 0:
        raise ValueError(f"{what}: sigma must be a positive number or None, got {sigma!r}")
    if threshold is not None:
        _spot_number(what, "threshold", threshold)
    else:
        _spot_number(what, "snr", snr, finite=True)
    scaled, scale = (image, None) if sigma is None else _img_as_float_plan(image)
    d, _ = _spot_plane(what, scaled)
    shape = tuple(d.shape[1:])
    if intensity is None:
        # the plane that was uploaded holds the image's own values unless img_as_float rescaled it on the host
        source = d if scaled is image else _spot_plane(what, image)[0]
    else:
        source = _spot_plane(what, intensity, "intensity")[0]
        if tuple(source.shape[1:]) != shape:
            raise ValueError(f"{what}: intensity must have the image's shape {shape}, got {tuple(source.shape[1:])}")
    lab = _spot_labels(what, labels, shape, d.ctx)
    response = d if sigma is None else hipops.difference_of_gaussians(d, float(sigma), 1.6 * float(sigma), scale=scale)
    if threshold is None:
        p25, p50, p75 = (float(v) for v in hipops.percentile(response, [25, 50, 75]).numpy()[0])
        t = p50 + float(snr) * (p75 - p25) / 1.349
    else:
        t = float(threshold)
    return _spot_table(response, source, r, t, b, k, lab)
