"""``SegmentationMask``: label image -> per-cell feature table, on the GPU (reference: R/masks.py:15-467).

Same constructor, validation, error messages, immutability, property names, derived columns and key
order as the reference.  ``label_image`` (clear_border + label / relabel_sequential) and
``cell_properties`` (two ``regionprops_table`` passes in the reference, one per channel for intensity)
run as HIP kernels; only the (num_cells x columns) table crosses PCIe.
"""
from __future__ import annotations

import warnings
from collections.abc import Mapping
import numpy as np

from .typing import Float64Array, Int64Array, ScalarArray

class cached_property:  # noqa: N801 -- used like functools.cached_property
    """``functools.cached_property`` without its lock.  Up to Python 3.11 the standard descriptor holds ONE lock per
    property for ALL instances, so worker threads that each compute ``cell_properties`` of their OWN mask (one context
    per thread, R/pipeline.py:145-146) run one after the other (measured: 8 threads, 2.5 -> 31 ms per call).  Two
    threads racing on the SAME instance may both compute the value; the results are identical and one wins."""

    def __init__(self, func):
        self.func = func
        self.name = func.__name__
        self.__doc__ = func.__doc__

    def __set_name__(self, owner, name):
        self.name = name

    def __get__(self, obj, owner=None):
        if obj is None:
            return self
        d = obj.__dict__
        if self.name not in d:
            d[self.name] = self.func(obj)
        return d[self.name]


# columns of `cell_properties` when the caller names none (the reference's lists, R/masks.py:15-35)
DEFAULT_CELL_PROPERTY_NAMES = (
    "label centroid volume area area_convex perimeter eccentricity circularity solidity "
    "axis_major_length axis_minor_length orientation"
).split()
DEFAULT_INTENSITY_PROPERTY_NAMES = ["intensity_" + stat for stat in ("mean", "max", "min", "std")]


def _process_mask_device(mask_image, remove_edge_cells: bool, mx=None):
    """R/masks.py:38-65 on the device -> (int32 DeviceArray of sequential labels, count)."""
    from . import hipops
    from .device import get_context

    ctx = get_context()
    if mask_image.dtype == bool:
        lab, cnt = hipops.label(ctx.asarray(mask_image), connectivity=2)
        k = int(cnt.numpy()[0])
        if remove_edge_cells:
            # components of a label image are connected by construction: flag-and-renumber pass
            lab, cnt = hipops.clear_border_relabel(lab, max(k, 1))
            k = int(cnt.numpy()[0])
            if k == 0:
                raise ValueError(
                    "No cells remain after removing edge cells. Try setting remove_edge_cells=False."
                )
        return lab, k
    mx = int(mask_image.max() if mx is None else mx)
    if mx >= 2**31 - 1:
        raise ValueError("label values above 2**31 - 2 are not supported on the device path")
    lab = ctx.asarray(mask_image, dtype=np.int32)  # narrowed while it moves into the staging buffer
    if remove_edge_cells:
        # arbitrary label images: a label may have several pieces, only those touching the frame go
        lab = hipops.clear_border(lab)
        if int(hipops.max_per_plane(lab).numpy()[0]) == 0:
            raise ValueError(
                "No cells remain after removing edge cells. Try setting remove_edge_cells=False."
            )
    lab, cnt = hipops.relabel_sequential(lab, mx)
    return lab, int(cnt.numpy()[0])


def _hull_columns_of_fragmented_labels(lab, k: int, shape, morph, ext, want_feret: bool):
    """area_convex, solidity and feret_diameter_max of a label image whose labels' bounding-box heights add up to
    more than H * W -> (morph, ext).

    The hull kernels keep one row-extent entry per bounding-box row of every label in H * W entries per plane, which
    connected labels never exceed; the labels of an arbitrary integer image may have many pieces, and past that
    capacity the kernels give NaN for every label of the plane.  Such images are measured again in groups of labels
    whose heights fit, each group on a plane of its own (``hipops.keep_labels`` keeps the label values), and the
    columns are written back.  When the heights fit, nothing is done."""
    from . import _hip, hipops
    from .device import get_context

    c = {n: i for i, n in enumerate(_hip.RP_COLS)}
    H, W = shape
    heights = (morph[:, c["bbox-2"]] - morph[:, c["bbox-0"]]).astype(np.int64)
    if k == 0 or int(heights.sum()) <= H * W:
        return morph, ext
    morph = morph.copy()
    ext = None if ext is None else ext.copy()
    groups, cur, used = [], [], 0
    for i, h in enumerate(heights.tolist()):
        if used + h > H * W:
            groups.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += h
    groups.append(cur)
    ctx = get_context()
    ac, feret = c["area_convex"], _hip.RPX_COLS.index("feret_diameter_max")
    for g in groups:
        keep = np.zeros((1, k + 1), np.uint8)
        keep[0, np.asarray(g) + 1] = 1
        plane = hipops.keep_labels(lab.reshape((1,) + tuple(shape)), ctx.asarray(keep), k)
        morph[g, ac] = hipops.regionprops(plane, k).numpy()[0][g, ac]
        if want_feret and ext is not None:
            t, _ = hipops.regionprops_ext(plane, k, ["feret_diameter_max"])
            ext[g, feret] = t.numpy()[0][g, feret]
    area = morph[:, c["area"]]
    with np.errstate(divide="ignore", invalid="ignore"):
        morph[:, c["solidity"]] = np.where(area > 0, area / morph[:, ac], 0.0)
    return morph, ext


def _process_mask(mask_image, remove_edge_cells: bool):
    """The reference's module-level helper (R/masks.py:38-65): host array in, int64 label image out."""
    return _process_mask_device(np.asarray(mask_image), remove_edge_cells)[0].numpy_int64()


def _sequential_labels_on_device(label_image):
    """Arbitrary positive labels -> (int32 device plane numbered 1..k in ascending order of the labels, k)."""
    from . import hipops
    from .device import get_context

    a = np.asarray(label_image)
    if a.ndim != 2:
        raise ValueError("label_image must be a 2D array")
    mx = int(a.max()) if a.size else 0
    if mx <= 0:
        return None, 0
    if mx >= 2**31 - 1:
        raise ValueError("label values above 2**31 - 2 are not supported on the device path")
    lab, cnt = hipops.relabel_sequential(get_context().asarray(a, dtype=np.int32), mx)
    return lab, int(cnt.numpy()[0])


def _extract_outlines_skimage(label_image):
    """The reference's module-level helper (R/masks.py:82-115): one (n, 2) float64 (y, x) outline per label present
    in ``label_image``, in ascending label order -- marching squares on the device (``hipops.cell_outlines``)."""
    from . import hipops

    lab, k = _sequential_labels_on_device(label_image)
    return hipops.cell_outlines(lab, k) if k else []


def _extract_outlines_cellpose(label_image):
    """The reference's module-level helper (R/masks.py:68-79): ``cellpose.utils.outlines_list`` per label, (y, x)
    order -- border following on the device (``hipops.cell_outlines_borders``; parity unpinned)."""
    from . import hipops

    lab, k = _sequential_labels_on_device(label_image)
    return hipops.cell_outlines_borders(lab, k) if k else []


def _extrema(a: np.ndarray):
    """(min, max) of a 2-D array.  Planes of a megapixel and more are reduced band by band on the host-copy threads:
    integer images with one foreign call per band (``device.host_extrema``), other element types with numpy in pieces
    of 256 KB whose minimum AND maximum are taken while the piece is in cache.  The image crosses the memory bus once
    (a 2048^2 int64 label image is 33 MB, and with a worker thread per context the host's memory system and the
    interpreter lock are what bound the reference-level calls)."""
    from .device import _pool4, host_extrema

    if a.size < (1 << 20) or a.shape[0] < 8:
        return host_extrema(a) or (a.min(), a.max())
    rows = max(1, (256 << 10) // max(1, a.shape[1] * a.itemsize))

    def band(b):
        got = host_extrema(b)
        if got is not None:
            return got
        mn, mx = b[:1].min(), b[:1].max()
        for r in range(0, b.shape[0], rows):
            piece = b[r:r + rows]
            mn, mx = min(mn, piece.min()), max(mx, piece.max())
        return mn, mx

    step = -(-a.shape[0] // 4)
    futs = [_pool4().submit(band, a[r:r + step]) for r in range(0, a.shape[0], step)]
    parts = [f.result() for f in futs]
    return min(p[0] for p in parts), max(p[1] for p in parts)


def _as_one_block(planes):
    """The (C, Y, X) array whose channels ``planes`` are, when they lie back to back in memory (the usual case:
    ``{channel: fov[i]}`` of one acquisition); None otherwise."""
    p0 = planes[0]
    if len(planes) < 2 or any(p.dtype != p0.dtype or p.shape != p0.shape or not p.flags["C_CONTIGUOUS"] for p in planes):
        return None
    if any(p.ctypes.data != p0.ctypes.data + c * p0.nbytes for c, p in enumerate(planes)):
        return None
    base = p0.base
    while base is not None and not (isinstance(base, np.ndarray) and base.flags["C_CONTIGUOUS"]
                                    and base.ctypes.data <= p0.ctypes.data
                                    and base.ctypes.data + base.nbytes >= planes[-1].ctypes.data + p0.nbytes):
        base = getattr(base, "base", None)
    if base is None or any(p.base is None for p in planes):
        return None
    # a view of the owner that covers exactly the planes (no copy): the owner keeps the memory alive
    flat = base.reshape(-1).view(np.uint8)
    o = p0.ctypes.data - base.ctypes.data
    return flat[o:o + len(planes) * p0.nbytes].view(p0.dtype).reshape((len(planes),) + p0.shape)


def _check_label_plane(mask_image):
    """Constructor checks of the mask, in the reference's order and wording (R/masks.py:169-176) -> the image's
    largest value (kept for the device path's range check)."""
    if not isinstance(mask_image, np.ndarray):
        raise TypeError("mask_image must be a numpy array")
    if mask_image.ndim != 2:
        raise ValueError("mask_image must be a 2D array")
    # one pass for both extrema and no temporaries (the image is 33 MB at 2048^2 int64)
    mn, mx = _extrema(mask_image) if mask_image.size else (0, 0)
    if mask_image.dtype.kind not in "bu" and mn < 0:
        raise ValueError("mask_image must have non-negative values")
    if not mx:
        raise ValueError("mask_image contains no cells (all values are 0)")
    return mx


def _checked_intensities(images, shape):
    """None, or a NEW dict channel -> 2-D array of the mask's shape; the arrays themselves stay shared with the
    caller (R/masks.py:178-194)."""
    if images is None:
        return None
    if not isinstance(images, Mapping):
        raise TypeError("intensity_image_dict must be a Mapping of channels to 2D arrays")
    for channel, plane in images.items():
        label = f"Intensity image for '{channel.name}'"
        if not isinstance(plane, np.ndarray):
            raise TypeError(f"{label} must be a numpy array")
        if plane.ndim != 2:
            raise ValueError(f"{label} must be 2D")
        if plane.shape != shape:
            raise ValueError(f"{label} must have same shape as mask_image")
    return dict(images)


class SegmentationMask:
    """A label (or boolean) mask with the intensity images that belong to it, and the per-cell measurements derived
    from them (constructor contract: R/masks.py:118-208).

    mask_image                bool (foreground) or integer (labels) 2-D array with at least one cell
    intensity_image_dict      optional mapping Channel -> 2-D intensity image of the same shape
    remove_edge_cells         drop cells that touch the image frame before numbering (default True)
    outline_extractor         "cellpose" (pixel borders, the default) or "skimage" (sub-pixel contours)
    property_names            columns of `cell_properties` (default DEFAULT_CELL_PROPERTY_NAMES)
    intensity_property_names  per-channel intensity columns (default: all four when intensity images are given)

    The six constructor arguments cannot be reassigned afterwards; everything derived is computed on the GPU on
    first access and cached.
    """

    _CTOR_FIELDS = ("mask_image", "intensity_image_dict", "remove_edge_cells", "outline_extractor", "property_names",
                    "intensity_property_names")

    def __init__(self, mask_image, intensity_image_dict=None, remove_edge_cells=True, outline_extractor="cellpose",
                 property_names=None, intensity_property_names=None):
        mx = _check_label_plane(mask_image)
        channels = _checked_intensities(intensity_image_dict, mask_image.shape)
        if property_names is None:
            property_names = list(DEFAULT_CELL_PROPERTY_NAMES)
        if intensity_property_names is None:
            intensity_property_names = list(DEFAULT_INTENSITY_PROPERTY_NAMES) if channels else []
        given = (mask_image, channels, remove_edge_cells, outline_extractor, property_names, intensity_property_names)
        for name, value in zip(self._CTOR_FIELDS, given):
            object.__setattr__(self, name, value)
        object.__setattr__(self, "_mask_max", mx)
        object.__setattr__(self, "_sealed", True)

    @classmethod
    def _from_device(cls, labels, num_cells: int, morph: np.ndarray, inten, intensity_image_dict=None,
                     outline_extractor="cellpose", property_names=None, intensity_property_names=None):
        """A mask whose label plane was COMPUTED on the device (``SegmentationModel.batch_masks``): ``labels`` is the
        int32 plane after edge-cell removal and sequential numbering, ``morph`` / ``inten`` the feature rows of its
        ``num_cells`` cells.  Equal in every derived attribute to ``SegmentationMask(labels.numpy_int64(), ...)``;
        ``mask_image`` is that same label image, downloaded when it is first read."""
        if num_cells <= 0:
            raise ValueError("mask_image contains no cells (all values are 0)")
        self = object.__new__(cls)
        channels = _checked_intensities(intensity_image_dict, tuple(labels.shape[-2:]))
        if property_names is None:
            property_names = list(DEFAULT_CELL_PROPERTY_NAMES)
        if intensity_property_names is None:
            intensity_property_names = list(DEFAULT_INTENSITY_PROPERTY_NAMES) if channels else []
        given = (channels, True, outline_extractor, property_names, intensity_property_names)
        for name, value in zip(cls._CTOR_FIELDS[1:], given):
            object.__setattr__(self, name, value)
        d = self.__dict__
        d["_mask_max"] = int(num_cells)
        d["_labels_device"] = (labels, int(num_cells))
        d["_rows"] = (morph, inten)
        d["_sealed"] = True
        return self

    @classmethod
    def _derived(cls, parent: "SegmentationMask", labels, num_cells: int, parent_labels: np.ndarray):
        """A mask whose label plane was computed on the device FROM ``parent``'s (``expanded`` / ``ring``): ``labels``
        is an int32 (Y, X) plane numbered 1..``num_cells``, ``parent_labels[j]`` the label of ``parent.label_image``
        that label ``j + 1`` came from.  It shares the parent's intensity images, outline extractor and property
        lists, records ``remove_edge_cells=False`` (nothing is dropped), downloads ``mask_image`` / ``label_image``
        only when they are read and measures ``cell_properties`` on first access."""
        if num_cells <= 0:
            raise ValueError("mask_image contains no cells (all values are 0)")
        self = object.__new__(cls)
        channels = None if parent.intensity_image_dict is None else dict(parent.intensity_image_dict)
        given = (channels, False, parent.outline_extractor, list(parent.property_names),
                 list(parent.intensity_property_names))
        for name, value in zip(cls._CTOR_FIELDS[1:], given):
            object.__setattr__(self, name, value)
        d = self.__dict__
        d["_mask_max"] = int(num_cells)
        d["_labels_device"] = (labels, int(num_cells))
        d["parent_labels"] = parent_labels
        d["_sealed"] = True
        return self

    # row j of a derived mask (``expanded`` / ``ring``) came from label parent_labels[j] of the mask it was derived from
    parent_labels = None

    def __getattr__(self, name):
        # only reached for attributes that are not set: the lazily downloaded label image of a device-born mask
        if name == "mask_image" and "_labels_device" in self.__dict__:
            image = self.__dict__["_labels_device"][0].numpy_int64()
            self.__dict__["mask_image"] = image
            return image
        raise AttributeError(f"{type(self).__name__!s} object has no attribute {name!r}")

    def __setattr__(self, name, value):
        if name in self._CTOR_FIELDS and self.__dict__.get("_sealed", False):
            raise AttributeError(
                f"Cannot modify '{name}' after SegmentationMask is initialized. Create a new instance instead."
            )
        object.__setattr__(self, name, value)

    def __repr__(self):
        chans = [c.name for c in self.intensity_image_dict] if self.intensity_image_dict else []
        if "mask_image" not in self.__dict__:  # device-born: do not download the image for a repr
            shape = tuple(self.__dict__["_labels_device"][0].shape[-2:])
            return (f"SegmentationMask(shape={shape}, dtype=int64, channels={chans}, "
                    f"remove_edge_cells={self.remove_edge_cells}, outline_extractor={self.outline_extractor!r})")
        return (f"SegmentationMask(shape={self.mask_image.shape}, dtype={self.mask_image.dtype}, channels={chans}, "
                f"remove_edge_cells={self.remove_edge_cells}, outline_extractor={self.outline_extractor!r})")

    # ---------------------------------------------------------------------------------------------
    @cached_property
    def _labels_device(self):
        return _process_mask_device(self.mask_image, self.remove_edge_cells, self._mask_max)

    @cached_property
    def label_image(self) -> Int64Array:
        """Consecutive int64 labels 1..K, background 0, edge cells removed if requested (R/masks.py:210-218)."""
        lab, _ = self._labels_device
        return lab.numpy_int64()

    @cached_property
    def num_cells(self) -> int:
        return int(self._labels_device[1])

    @cached_property
    def cell_outlines(self) -> list[Float64Array]:
        """Per-cell outlines, one (n, 2) array of (y, x) vertices per cell (R/masks.py:229-245).

        Both extractors run on the device.  ``outline_extractor="skimage"``: marching squares at level 0.5 on each
        cell's padded bounding box, longest contour, in scikit-image's vertex order, float64 (R/masks.py:82-115;
        pinned by tests/golden/outlines_96.npz).  ``outline_extractor="cellpose"`` (the reference's default):
        ``cellpose.utils.outlines_list`` = OpenCV ``findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE)`` per cell, the
        border with the most points, int64 pixel coordinates, empty when it has fewer than five points
        (R/masks.py:68-79); restated from the published border-following algorithm, parity unpinned (neither
        package exists offline, the reference's tests hold no vector for it)."""
        from . import hipops

        lab, k = self._labels_device
        plane = lab[0] if lab.ndim == 3 else lab
        if self.outline_extractor == "cellpose":
            return hipops.cell_outlines_borders(plane, int(k))
        return hipops.cell_outlines(plane, int(k))

    def _intensity_stack(self, shape):
        """The intensity images as one device (C, Y, X) stack -> (stack, channel names, exact).  uint8 / uint16
        images are kept as uint16 and accumulated exactly (integer sums); any other dtype the reference accepts
        (R/masks.py:178-190: "any 2-D ndarray") is measured in float64, as regionprops does.  The planes go to the
        device one by one into their slot of the stack: no host-side stack."""
        from .device import get_context

        planes, names = [], []
        for channel, img in self.intensity_image_dict.items():
            planes.append(np.asarray(img))
            names.append(channel.name)
        exact = all(p.dtype in (np.uint8, np.uint16) for p in planes)
        ctx = get_context()
        stack = ctx.empty((len(planes),) + tuple(shape), np.uint16 if exact else np.float64)
        whole = _as_one_block(planes)
        if whole is not None:  # the planes are the channels of ONE (C, Y, X) array: one staged transfer
            ctx.asarray(whole, out=stack)
        else:
            for c, p in enumerate(planes):
                ctx.asarray(p, out=stack[c])  # converted to the stack's dtype on its way through staging
        return stack, names, exact

    @cached_property
    def cell_properties(self) -> dict[str, ScalarArray]:
        """Morphology + per-channel intensity features, one entry per cell ordered by label
        (R/masks.py:247-328; columns of scikit-image's ``regionprops_table``).  Besides the default columns, the
        extended names of ``segment.EXT_DEVICE_PROPERTIES`` / ``EXT_HOST_PROPERTIES`` (property_names) and
        ``WEIGHTED_PROPERTIES`` (intensity_property_names) are measured too.  Labels of several pieces whose
        bounding-box heights add up to more than the image's pixel count get area_convex, solidity and
        feret_diameter_max from a second pass in groups (``_hull_columns_of_fragmented_labels``), not NaN."""
        from . import hipops
        from .segment import WEIGHTED_PROPERTIES, assemble_cell_properties, ext_columns

        assert self.property_names is not None
        assert self.intensity_property_names is not None
        lab, k = self._labels_device
        k = int(k)
        shape = tuple(lab.shape[-2:])
        want_ext = ext_columns(self.property_names, self.intensity_property_names)
        want_w = bool(self.intensity_image_dict) and any(p in WEIGHTED_PROPERTIES for p in want_ext)
        if not want_w:  # weighted centroids without intensity images: the reference makes no intensity columns
            want_ext = [p for p in want_ext if p not in WEIGHTED_PROPERTIES]
        stack, names, exact = None, [], True
        if self.intensity_image_dict and self.intensity_property_names:
            names = [c.name for c in self.intensity_image_dict]
        if "_rows" in self.__dict__:  # measured by the chain that made the labels (SegmentationModel.batch_masks)
            morph, inten = self.__dict__["_rows"]
            inten = inten if (names and self.intensity_property_names) else None
            if want_w:
                stack, _, _ = self._intensity_stack(shape)
        else:
            inten = None
            if names:
                stack, names, exact = self._intensity_stack(shape)
                if exact and lab.size == stack.size // len(names):
                    # morphology + intensities share the bounding-box pass and the per-label scan
                    m, it = hipops.regionprops_full(lab.reshape((1,) + shape), stack.reshape((1,) + stack.shape),
                                                    max(k, 1))
                    morph, inten = m.numpy()[0][:k], it.numpy()[0][:k]
                else:
                    morph = hipops.regionprops(lab, max(k, 1)).numpy()[0][:k]
                    inten = hipops.regionprops_intensity(lab, stack, max(k, 1)).numpy()[0][:k]
            else:
                morph = hipops.regionprops(lab, max(k, 1)).numpy()[0][:k]
        ext = wext = None
        if want_ext:
            planes = lab.reshape((1,) + shape)
            t, w = hipops.regionprops_ext(planes, max(k, 1), want_ext,
                                          intensity=stack.reshape((1,) + stack.shape) if want_w else None)
            ext = None if t is None else t.numpy()[0][:k]
            wext = None if w is None else w.numpy()[0][:k]
        morph, ext = _hull_columns_of_fragmented_labels(lab, k, shape, morph, ext,
                                                        "feret_diameter_max" in want_ext)
        return assemble_cell_properties(morph, inten, names, list(self.property_names),
                                        list(self.intensity_property_names), ext=ext, wext=wext)

    def cell_colocalization(self, thresholds=None, pairs=None) -> dict[str, Float64Array]:
        """How pairs of channels relate inside every cell: ``pearson``, ``overlap`` (Manders' overlap coefficient),
        ``m1`` / ``m2`` (Manders' colocalisation coefficients) and ``intersection1`` / ``intersection2``, as
        ``skimage.measure`` (0.20 and later) defines them (include/amt_hip.h states the formulas), measured on the
        device.  Keys are ``f"{measure}_{a}_{b}"`` with the lower-cased channel names of ``intensity_image_dict`` in
        its order (``segment.colocalization_keys``), e.g. ``pearson_fitc_tritc``; each entry holds one value per cell,
        ordered by label like ``cell_properties`` (row j of a ring's table belongs to ``parent_labels[j]``).

        ``thresholds`` decides which pixels count as positive (value > threshold) for m1 / m2 and the intersection
        coefficients: None (0 for every channel), one number for all channels, or a mapping Channel -> number or
        ``"otsu"`` -- the Otsu threshold of that whole image, the value ``apply_threshold(image, "otsu")`` compares
        against; channels the mapping leaves out get 0.  ``pairs`` is a list of (Channel, Channel), default every pair
        in channel order; for (a, b), m1 is the share of a's intensity on b-positive pixels.  uint8 / uint16 images
        are summed exactly in integers, any other dtype in float64.  A channel that is constant over a cell gives a
        NaN ``pearson``."""
        from . import hipops
        from .device import get_context
        from .segment import colocalization_keys, colocalization_pairs

        channels = list(self.intensity_image_dict or {})
        if len(channels) < 2:
            raise ValueError("cell_colocalization needs at least two intensity images")
        index_pairs = colocalization_pairs(channels, pairs)
        values = [0.0] * len(channels)
        if isinstance(thresholds, Mapping):
            for channel, t in thresholds.items():
                if channel not in self.intensity_image_dict:
                    raise ValueError(f"thresholds names '{getattr(channel, 'name', channel)}', which has no intensity image")
                if isinstance(t, str):
                    if t.lower() != "otsu":
                        raise ValueError(f"threshold '{t}' is not supported: give a number or 'otsu'")
                elif isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)):
                    raise TypeError(f"a threshold must be a number or 'otsu', got {t!r}")
                values[channels.index(channel)] = t
        elif thresholds is not None:
            if isinstance(thresholds, (bool, str)) or not isinstance(thresholds, (int, float, np.integer, np.floating)):
                raise TypeError("thresholds must be None, a number or a mapping of channels to numbers or 'otsu'")
            values = [float(thresholds)] * len(channels)
        for c, t in enumerate(values):
            if isinstance(t, str):
                from .operations import otsu_threshold_value

                values[c] = otsu_threshold_value(self.intensity_image_dict[channels[c]])
        lab, k = self._labels_device
        k = int(k)
        shape = tuple(lab.shape[-2:])
        stack, _, _ = self._intensity_stack(shape)
        table = hipops.colocalization(lab.reshape((1,) + shape), stack.reshape((1,) + stack.shape), max(k, 1),
                                      thresholds=np.asarray(values, dtype=np.float64)[None, :],
                                      pairs=index_pairs).numpy()[0][:k]
        cols = table.reshape(k, -1)
        return {key: cols[:, i].copy() for i, key in enumerate(colocalization_keys(channels, index_pairs))}

    def cell_robust_intensity(self) -> dict[str, Float64Array]:
        """Robust intensity statistics of every channel inside every cell, measured on the device: the lower quartile,
        the median, the upper quartile (``np.percentile(values, 25 | 50 | 75)``, linear interpolation) and the raw
        median absolute deviation ``np.percentile(|values - median|, 50)`` (no 1.4826 factor) -- CellProfiler's
        LowerQuartile / Median / UpperQuartile / MAD.  Keys are ``intensity_q25_<channel>``,
        ``intensity_median_<channel>``, ``intensity_q75_<channel>``, ``intensity_mad_<channel>`` with the lower-cased
        channel names of ``intensity_image_dict``, channel by channel in its order
        (``segment.robust_intensity_keys``); each entry holds one float64 per cell, ordered by label like
        ``cell_properties`` (row j of an ``expanded`` / ``ring`` mask belongs to ``parent_labels[j]``).  uint8 / uint16
        images are selected exactly on integers, any other dtype in float64 (NaN and infinities are not supported);
        both equal numpy bit for bit.  Raises ``ValueError`` without intensity images."""
        from . import hipops
        from .segment import robust_intensity_keys

        channels = list(self.intensity_image_dict or {})
        if not channels:
            raise ValueError("cell_robust_intensity needs intensity images")
        lab, k = self._labels_device
        k = int(k)
        shape = tuple(lab.shape[-2:])
        stack, _, _ = self._intensity_stack(shape)
        table = hipops.robust_intensity(lab.reshape((1,) + shape), stack.reshape((1,) + stack.shape),
                                        max(k, 1)).numpy()[0][:k]
        cols = table.reshape(k, -1)
        return {key: cols[:, i].copy() for i, key in enumerate(robust_intensity_keys(channels))}

    def cell_texture(self, levels: int = 8, distance: int = 1, ranges=None, angles: str = "each") -> dict[str, Float64Array]:
        """Haralick texture of every channel inside every cell, measured on the device (CellProfiler's MeasureTexture):
        the thirteen features of ``_hip.TEX_COLS`` -- angular_second_moment, contrast, correlation, variance,
        inverse_difference_moment, sum_average, sum_variance, sum_entropy, entropy, difference_variance,
        difference_entropy, info_measure_1, info_measure_2, as ``mahotas.features.haralick`` defines them
        (include/amt_hip.h states the formulas) -- of the symmetric grey-level co-occurrence matrix of the cell's pixels
        at ``distance`` pixels in the directions 0, 45, 90 and 135 degrees, the image quantised to ``levels`` grey levels
        (2..64).  Keys are ``texture_<feature>_<channel>_<distance>_<angle>`` with the lower-cased channel names of
        ``intensity_image_dict``, channel by channel, angle by angle, feature by feature (``segment.texture_keys``), e.g.
        ``texture_contrast_dapi_1_45``; each entry holds one float64 per cell, ordered by label like ``cell_properties``
        (row j of an ``expanded`` / ``ring`` mask belongs to ``parent_labels[j]``).

        ``ranges`` says which intensities span the grey levels (values outside are clipped): None = each image's own
        minimum and maximum, found on the device; a (lo, hi) pair for every channel; or a mapping Channel -> (lo, hi),
        where channels the mapping leaves out keep their own minimum and maximum.  ``angles="mean"`` averages each
        feature over the directions in which the cell has a pair of pixels (keys
        ``texture_<feature>_<channel>_<distance>``).  A direction without a pair -- a cell narrower than ``distance`` --
        gives NaN.  uint8 / uint16 images are read as integers, any other dtype as float64 (NaN and infinities are not
        supported).  Raises ``ValueError`` without intensity images."""
        from . import hipops
        from .segment import texture_keys

        channels = list(self.intensity_image_dict or {})
        if not channels:
            raise ValueError("cell_texture needs intensity images")
        keys = texture_keys(channels, distance, angles)
        levels, distance = hipops.texture_parameters(levels, distance)

        def pair(r, what):
            try:
                lo, hi = (float(v) for v in r)
            except (TypeError, ValueError):
                raise TypeError(f"{what} must be a (lo, hi) pair of numbers, got {r!r}") from None
            return lo, hi

        if isinstance(ranges, Mapping):
            for channel in ranges:
                if channel not in self.intensity_image_dict:
                    raise ValueError(f"ranges names '{getattr(channel, 'name', channel)}', which has no intensity image")
            rows = []
            for channel in channels:
                if channel in ranges:
                    rows.append(pair(ranges[channel], f"the range of '{channel.name}'"))
                else:
                    image = self.intensity_image_dict[channel]
                    rows.append((float(image.min()), float(image.max())))
            ranges = np.asarray(rows, dtype=np.float64)[None]
        elif ranges is not None:
            ranges = np.asarray(pair(ranges, "ranges"), dtype=np.float64)
        lab, k = self._labels_device
        k = int(k)
        shape = tuple(lab.shape[-2:])
        stack, _, _ = self._intensity_stack(shape)
        table = hipops.texture(lab.reshape((1,) + shape), stack.reshape((1,) + stack.shape), max(k, 1), levels=levels,
                               distance=distance, ranges=ranges).numpy()[0][:k]
        if angles == "mean":  # over the directions that have pairs; all-NaN stays NaN
            valid = ~np.isnan(table)
            count = valid.sum(axis=2)
            total = np.where(valid, table, 0.0).sum(axis=2)
            table = np.where(count > 0, total / np.maximum(count, 1), np.nan)
        cols = table.reshape(k, -1)
        return {key: cols[:, i].copy() for i, key in enumerate(keys)}

    def cell_radial_distribution(self, bins: int = 4) -> dict[str, Float64Array]:
        """How every channel's signal is spread between the centre and the rim of every cell, and the two radii of the
        cell's shape, measured on the device (after CellProfiler's MeasureObjectIntensityDistribution and the
        MaximumRadius / MeanRadius of MeasureObjectSizeShape; include/amt_hip.h states the definitions).  Every pixel of
        a cell has its exact Euclidean distance d to the nearest pixel outside the cell -- background, a touching
        neighbour, or the frame around the image; ``maximum_radius`` is the largest d (the radius of the largest
        inscribed circle) and ``mean_radius`` the mean of d.  The cell is cut into ``bins`` rings (1..16) of equal width
        in ``d / maximum_radius``, ring 1 the innermost; per channel and ring, ``frac_at_d`` is the ring's share of the
        cell's total intensity, ``mean_frac`` that share divided by the ring's share of the cell's pixels, and
        ``radial_cv`` the coefficient of variation of the mean intensity over the (up to) eight wedges of the ring
        around the centroid.

        Keys are ``maximum_radius``, ``mean_radius``, then ``radial_<measure>_<channel>_<i>of<bins>`` with the
        lower-cased channel names of ``intensity_image_dict``, channel by channel, ring by ring
        (``segment.radial_keys``), e.g. ``radial_frac_at_d_fitc_1of4``; each entry holds one float64 per cell, ordered
        by label like ``cell_properties`` (row j of an ``expanded`` / ``ring`` mask belongs to ``parent_labels[j]``).
        Without intensity images the two radii alone are returned.  uint8 / uint16 images are read as integers, any
        other dtype as float64 (NaN and infinities are not supported).  A ring without a pixel, or a cell whose channel
        sums to zero, gives NaN."""
        from . import _hip, hipops
        from .segment import radial_keys

        channels = list(self.intensity_image_dict or {})
        keys = radial_keys(channels, bins)
        bins = hipops.radial_parameters(bins)
        lab, k = self._labels_device
        k = int(k)
        shape = tuple(lab.shape[-2:])
        stack = None
        if channels:
            stack, _, _ = self._intensity_stack(shape)
            stack = stack.reshape((1,) + stack.shape)
        geometry, table = hipops.radial_distribution(lab.reshape((1,) + shape), stack, max(k, 1), bins=bins)
        cols = geometry.numpy()[0][:k, :len(_hip.RAD_GEOM_COLS)]
        if table is not None:
            cols = np.concatenate([cols, table.numpy()[0][:k].reshape(k, -1)], axis=1)
        return {key: cols[:, i].copy() for i, key in enumerate(keys)}

    @cached_property
    def centroids_yx(self) -> Float64Array:
        """(num_cells, 2) array of [y, x] centroids (R/masks.py:330-353)."""
        if self.property_names is None:
            raise ValueError("property_names cannot be None.")
        if "centroid" not in self.property_names:
            message = ("Centroid property not available. Include 'centroid' in property_names to get centroid "
                       "coordinates. Returning empty array.")
            warnings.warn(message, UserWarning, stacklevel=2)
            return np.empty((0, 2), dtype=float)
        table = self.cell_properties
        return np.stack([table["centroid_y"], table["centroid_x"]], axis=1).astype(float)

    def filter(self, property_name: str, min_value: float | None = None,
               max_value: float | None = None) -> "SegmentationMask":
        """New mask keeping the cells with ``min_value <= property <= max_value`` (R/masks.py:355-418)."""
        from . import hipops
        from .device import get_context

        assert self.property_names is not None
        assert self.intensity_property_names is not None
        if min_value is None and max_value is None:
            raise ValueError("At least one of min_value or max_value must be provided.")
        if property_name not in self.cell_properties:
            raise ValueError(
                f"Property '{property_name}' not found. "
                f"Available properties: {list(self.cell_properties.keys())}"
            )
        values = self.cell_properties[property_name]
        keep = np.ones(self.num_cells, dtype=bool)
        if min_value is not None:
            keep &= values >= min_value
        if max_value is not None:
            keep &= values <= max_value
        flags = np.zeros((1, self.num_cells + 1), dtype=np.uint8)
        flags[0, 1:] = keep
        lab, _ = self._labels_device
        kept = hipops.keep_labels(lab, get_context().asarray(flags), self.num_cells)
        new_label_image = kept.numpy_int64()
        if not keep.any():
            raise ValueError(
                f"No cells remain after filtering '{property_name}' "
                f"with min={min_value}, max={max_value}."
            )
        # the survivors keep their pixels; numbering restarts at 1 and edge cells are NOT re-examined
        settings = {name: getattr(self, name) for name in self._CTOR_FIELDS[1:]}
        settings.update(mask_image=new_label_image, remove_edge_cells=False,
                        property_names=list(self.property_names),
                        intensity_property_names=list(self.intensity_property_names))
        return SegmentationMask(**settings)

    def _label_plane(self):
        """(int32 (Y, X) device plane of ``label_image``, num_cells)"""
        lab, k = self._labels_device
        return lab.reshape(tuple(lab.shape[-2:])), int(k)

    def expanded(self, distance: float) -> "SegmentationMask":
        """The same cells with the same numbering, each grown by up to ``distance`` pixels into the background without
        overlapping its neighbours: ``skimage.segmentation.expand_labels(self.label_image, distance)`` as a
        ``SegmentationMask`` (nuclei -> "cells").  Label ``i`` of the result is cell ``i`` of this mask, so row ``i`` of
        both ``cell_properties`` tables describes the same cell; ``parent_labels`` is ``arange(1, num_cells + 1)``.
        A background pixel equally near to several cells goes to the one with the SMALLEST label (scipy's choice
        among tied pixels is an artefact of its scan order; see ``hipops.expand_labels``).  The label plane is made
        on the device from this mask's and downloaded only if ``mask_image`` / ``label_image`` are read."""
        from . import hipops

        if not float(distance) >= 0:
            raise ValueError(f"distance must be non-negative, got {distance}")
        plane, k = self._label_plane()
        grown = hipops.expand_labels(plane, distance)
        return SegmentationMask._derived(self, grown, k, np.arange(1, k + 1, dtype=np.int64))

    def ring(self, distance: float) -> "SegmentationMask":
        """The annulus each cell gains by ``expanded(distance)`` -- the grown cell minus the cell itself ("cytoplasm"
        around a nucleus) -- as a ``SegmentationMask``.  Non-empty rings are numbered 1..K' in ascending order of
        their parent cell and ``parent_labels[j]`` is the label of this mask that ring ``j + 1`` surrounds; a cell
        enclosed by its neighbours gains no pixel and has no ring.  Raises the constructor's "contains no cells"
        ``ValueError`` when no ring pixel exists."""
        from . import hipops

        if not float(distance) >= 0:
            raise ValueError(f"distance must be non-negative, got {distance}")
        plane, k = self._label_plane()
        annulus = hipops.expand_labels(plane, distance, ring=True)
        boxes = hipops.label_bboxes(annulus, k)[0]
        parents = np.flatnonzero(boxes[:, 2] >= boxes[:, 0]).astype(np.int64) + 1
        if parents.size == 0:
            raise ValueError("mask_image contains no cells (all values are 0)")
        lab, _ = hipops.relabel_sequential(annulus, k)
        return SegmentationMask._derived(self, lab, int(parents.size), parents)

    def _companion_plane(self, other):
        """``other`` of ``relate`` as an int32 (Y, X) device plane of this mask's shape."""
        from .device import get_context

        plane, _ = self._label_plane()
        if isinstance(other, SegmentationMask):
            comp, _ = other._label_plane()
        else:
            if not isinstance(other, np.ndarray):
                raise TypeError("other must be a SegmentationMask or a numpy array")
            if other.dtype.kind not in "iu":
                raise TypeError("other must be an integer label array")
            if other.ndim != 2:
                raise ValueError("other must be a 2D array")
            mn, mx = _extrema(other) if other.size else (0, 0)
            if mn < 0:
                raise ValueError("other must have non-negative values")
            if mx >= 2**31 - 1:
                raise ValueError("label values above 2**31 - 2 are not supported on the device path")
            comp = get_context().asarray(other, dtype=np.int32)
        if tuple(comp.shape) != tuple(plane.shape):
            raise ValueError("other must have the same shape as this mask")
        return comp

    def relate(self, other) -> dict[str, ScalarArray]:
        """How every cell of this mask lies on another label image, one entry per cell ordered by label like
        ``cell_properties`` (CellProfiler's RelateObjects; a row of ``skimage.metrics.contingency_table``):

        parent            the label of ``other`` that covers most pixels of the cell; among labels covering equally
                          many the SMALLEST; 0 when the cell lies on ``other``'s background (int64)
        overlap           the number of pixels the cell shares with its parent (int64)
        partners          the number of different labels of ``other`` under the cell (int64)
        area              the cell's pixel count (int64)
        overlap_fraction  overlap / area (float64)

        ``other`` is a ``SegmentationMask`` of the same shape (its ``label_image`` numbering is what ``parent``
        holds; an ``expanded`` / ``ring`` mask works on either side) or a non-negative integer label array of the
        same shape with values up to 2**31 - 2, whose values are used as they are.  Both label planes are related on
        the device (``hipops.relate_labels``); a plane that is already there does not leave it, only the
        (num_cells x 4) table comes back."""
        from . import _hip, hipops

        plane, k = self._label_plane()
        comp = self._companion_plane(other)
        shape = tuple(plane.shape)
        table = hipops.relate_labels(plane.reshape((1,) + shape), max(k, 1), comp.reshape((1, 1) + shape)).numpy()
        cols = table[0, :k, 0, :]
        out = {name: cols[:, i].astype(np.int64) for i, name in enumerate(_hip.RPX_RCOLS)}
        out["overlap_fraction"] = out["overlap"].astype(np.float64) / out["area"].astype(np.float64)
        return out

    def child_counts(self, other: "SegmentationMask") -> Int64Array:
        """Per cell of this mask, the number of cells of ``other`` whose ``parent`` (``other.relate(self)``) it is:
        nuclei per cell, spots per nucleus.  A cell of ``other`` that lies on this mask's background counts for
        nobody."""
        if not isinstance(other, SegmentationMask):
            raise TypeError("other must be a SegmentationMask")
        parent = other.relate(self)["parent"]
        return np.bincount(parent, minlength=self.num_cells + 1)[1:self.num_cells + 1].astype(np.int64)

    def cell_neighbors(self, distance: float = 0, other=None) -> dict[str, ScalarArray]:
        """Every cell's surroundings, one entry per cell ordered by label like ``cell_properties`` (CellProfiler's
        MeasureObjectNeighbors), measured on the device:

        number_of_neighbors      how many different cells touch the cell (int64)
        touching_pixels          the pixels of the cell's ring that belong to another cell (int64)
        ring_pixels              the pixels of the ring: those outside the cell with one of its pixels among their
                                 eight neighbours; the image border clips it (int64)
        percent_touching         100 * touching_pixels / ring_pixels; NaN when the ring is empty, i.e. the cell fills
                                 the image (float64)
        main_neighbor            the cell holding most of the ring's pixels, the SMALLEST label among equals; 0 without
                                 a neighbour (int64)
        first_closest_label      the cell whose centroid is nearest, the SMALLEST label among equally near ones; 0 when
                                 the cell is alone (int64)
        first_closest_distance   the distance between the two centroids in pixels; NaN when the cell is alone (float64)
        second_closest_label / second_closest_distance   the same for the next nearest cell

        ``distance == 0``: cells are neighbours when they touch, diagonally included.  ``distance > 0``: the first five
        columns are taken on ``self.expanded(distance)`` -- two cells are neighbours when their GROWN versions touch,
        CellProfiler's "expand" flavour -- which bridges a gap of about ``2 * distance`` pixels between the cells
        themselves.  The four closest columns always come from this mask's own centroids.  ``other`` (a
        ``SegmentationMask`` or a non-negative integer label array of the same shape, as for ``relate``) replaces the
        label plane whose values are looked up on the rings -- "which cells touch the ring of this nucleus" -- and is
        used as it is, never grown; the closest columns ignore it.  Works on ``expanded`` / ``ring`` masks and on masks
        from ``batch_masks``; the label plane does not leave the device, only the two (num_cells x 4) tables come back
        (``hipops.neighbor_census``, ``hipops.nearest_labels``; keys: ``segment.neighbor_keys``)."""
        from . import _hip, hipops

        d = float(distance)
        if not (np.isfinite(d) and d >= 0):
            raise ValueError(f"distance must be non-negative and finite, got {distance}")
        plane, k = self._label_plane()
        comp = None if other is None else self._companion_plane(other)
        shape = tuple(plane.shape)
        grown = hipops.expand_labels(plane, d) if d > 0 else plane
        census = hipops.neighbor_census(grown.reshape((1,) + shape), max(k, 1),
                                        None if comp is None else comp.reshape((1, 1) + shape)).numpy()[0, :k, 0, :]
        near = hipops.nearest_labels(plane.reshape((1,) + shape), max(k, 1)).numpy()[0, :k, 0, :]
        cen = {name: census[:, i].astype(np.int64) for i, name in enumerate(_hip.RPX_NCOLS4)}
        with np.errstate(invalid="ignore", divide="ignore"):
            percent = 100.0 * cen["touching"].astype(np.float64) / cen["ring"].astype(np.float64)
        return {"number_of_neighbors": cen["count"], "touching_pixels": cen["touching"], "ring_pixels": cen["ring"],
                "percent_touching": percent, "main_neighbor": cen["main"],
                "first_closest_label": near[:, 0].astype(np.int64), "first_closest_distance": near[:, 1].copy(),
                "second_closest_label": near[:, 2].astype(np.int64), "second_closest_distance": near[:, 3].copy()}

    def _skeleton_plane(self):
        """(int32 (Y, X) device plane: the label on the skeleton of its cell, 0 elsewhere; num_cells)"""
        from . import hipops

        plane, k = self._label_plane()
        return hipops.label_skeleton(plane), k

    def skeleton_image(self):
        """The skeletons of all cells as one image of ``label_image``'s dtype: a pixel on the skeleton of cell ``i``
        holds ``i``, every other pixel 0.  Each cell is thinned as if it were alone in the image (Zhang and Suen's rule,
        ``hipops.label_skeleton``), so touching cells keep a skeleton each."""
        return self._skeleton_plane()[0].numpy_int64()

    def cell_skeleton(self) -> dict[str, ScalarArray]:
        """Every cell's skeleton, one entry per cell ordered by label like ``cell_properties`` (the per-object part of
        CellProfiler's MeasureObjectSkeleton that needs no traversal), thinned and counted on the device.  With the
        degree of a skeleton pixel = how many of its eight neighbours are skeleton pixels of the same cell:

        skeleton_pixels           the pixels of the cell's skeleton (int64)
        skeleton_isolated         of these, the ones of degree 0: a round cell thins to a single pixel (int64)
        skeleton_ends             degree 1 (int64)
        skeleton_path_pixels      degree 2 (int64)
        skeleton_junction_pixels  degree 3 and more -- a property of pixels, not of branch points: one crossing may
                                  hold several (int64)
        skeleton_length           orth + sqrt(2) * diag in pixels, with orth the horizontally or vertically adjacent
                                  pairs of skeleton pixels and diag the diagonal pairs that no such pair bridges
                                  (float64)

        The skeleton of a cell is the one it would get alone in the image, however its neighbours touch it
        (``skeleton_image`` shows it).  Works on ``expanded`` / ``ring`` masks and on masks from ``batch_masks``; the label
        plane and the skeleton do not leave the device, only the (num_cells x 7) table comes back
        (``hipops.label_skeleton``, ``hipops.label_census``; keys: ``segment.skeleton_keys``).  Parity with scikit-image or
        CellProfiler is unpinned offline."""
        from . import _hip, hipops

        skel, k = self._skeleton_plane()
        table = hipops.label_census(skel, max(k, 1)).numpy()[0, :k, :]
        col = {name: table[:, i].astype(np.int64) for i, name in enumerate(_hip.LCEN_COLS)}
        orth, diag = col["orth_links"].astype(np.float64), col["diag_links"].astype(np.float64)
        return {"skeleton_pixels": col["pixels"], "skeleton_isolated": col["isolated"], "skeleton_ends": col["ends"],
                "skeleton_path_pixels": col["path"], "skeleton_junction_pixels": col["junctions"],
                "skeleton_length": orth + np.sqrt(2.0) * diag}

    def _spot_channel(self, what: str, channel):
        if not self.intensity_image_dict:
            raise ValueError(f"{what} needs intensity images")
        if channel not in self.intensity_image_dict:
            raise ValueError(f"{what}: '{getattr(channel, 'name', channel)}' has no intensity image")
        return self.intensity_image_dict[channel]

    def spots(self, channel, **detect_kwargs) -> dict[str, ScalarArray]:
        """The puncta of ``channel``'s intensity image as ``operations.detect_spots`` finds them (its keyword arguments
        pass through, ``labels=`` excepted), with ``label`` = the cell under each spot, 0 on background: a dict of
        equal-length arrays in raster order.  Works on ``expanded`` / ``ring`` masks (``label`` then numbers their rows)
        and on masks from ``batch_masks``; the label plane does not leave the device, the labels under the spots are
        gathered there (``hipops.take_at``)."""
        from .operations import detect_spots

        if "labels" in detect_kwargs:
            raise TypeError("spots: labels= is this mask; it cannot be passed")
        return detect_spots(self._spot_channel("spots", channel), labels=self, **detect_kwargs)

    def cell_spots(self, channel, **detect_kwargs) -> dict[str, ScalarArray]:
        """Per-cell spot columns of ``channel``, one entry per cell ordered by label like ``cell_properties``
        (CellProfiler's per-object child count for puncta; keys: ``segment.spot_keys``): ``spot_count_<ch>`` (int64; spots
        on background are not counted), ``spot_intensity_sum_<ch>`` (the sum of the spots' ``intensity_net``) and
        ``spot_intensity_mean_<ch>`` (NaN at count 0), with the lower-cased channel name.  The spots are those of
        ``spots(channel, **detect_kwargs)``; the columns are a ``bincount`` over that short list."""
        from .segment import spot_keys

        table = self.spots(channel, **detect_kwargs)
        k = self.num_cells
        label = table["label"]
        inside = (label >= 1) & (label <= k)
        count = np.bincount(label[inside], minlength=k + 1)[1:k + 1].astype(np.int64)
        total = np.bincount(label[inside], weights=table["intensity_net"][inside], minlength=k + 1)[1:k + 1].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(count > 0, total / np.maximum(count, 1), np.nan)
        return dict(zip(spot_keys(channel), (count, total, mean)))

    def convert_properties_to_microns(self, pixel_size_um: float) -> dict[str, ScalarArray]:
        """Scale lengths / areas / volumes to microns with ``_um`` / ``_um2`` / ``_um3`` key suffixes
        (R/masks.py:420-467); dimensionless and intensity columns pass through."""
        linear = {"perimeter", "axis_major_length", "axis_minor_length"}
        area = {"area", "area_convex"}
        volume = {"volume"}
        tensor = {"inertia_tensor", "inertia_tensor_eigvals"}
        out = {}
        for name, vals in self.cell_properties.items():
            if name in linear:
                out[f"{name}_um"] = vals * pixel_size_um
            elif name in area or name in tensor:
                out[f"{name}_um2"] = vals * (pixel_size_um**2)
            elif name in volume:
                out[f"{name}_um3"] = vals * (pixel_size_um**3)
            else:
                out[name] = vals
        return out
