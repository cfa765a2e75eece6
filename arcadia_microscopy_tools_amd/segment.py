"""Batch segmentation + region-props drivers for the BASELINE.json configurations, fully on the device.

Stages (CPU restatement: oracle/chains.py):
  C2  Gaussian(sigma) -> Otsu -> '>' -> binary opening(disk r) -> binary closing(disk r) -> label (8-conn)
  C3  C2 mask on the DAPI channel [-> binary_fill_holes if fill_holes=True] [-> remove_small_objects if min_size > 1]
      -> EDT -> peak markers (min_distance) -> watershed (seeded relief)
      -> clear_border -> relabel_sequential -> morphology table + per-channel intensity table

``FovSegmenter`` preallocates every buffer for a batch of B fields of view, enqueues the whole chain
on one HIP stream without any host synchronisation, and only copies labels / tables back on request.
This is the classical backend behind ``SegmentationModel.segment`` (reference signature:
R/model.py:171-215) and what bench.py times.
"""
from __future__ import annotations

import numpy as np

from . import _hip, hipops
from .device import Context, DeviceArray, get_context

DEFAULT_CHANNELS = ("BRIGHTFIELD", "DAPI", "FITC", "TRITC")


class StageTimes:
    """HIP-event timers around each stage of one run (all on the segmenter's stream)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.timers: dict[str, object] = {}
        self.order: list[str] = []

    def begin(self, name):
        t = self.timers.get(name)
        if t is None:
            t = self.ctx.timer()
            self.timers[name] = t
            self.order.append(name)
        t.start()
        return t

    def ms(self) -> dict[str, float]:
        return {k: self.timers[k].elapsed_ms() for k in self.order}


class FovSegmenter:
    """Preallocated config-2 / config-3 chain for B fields of view of shape (C, H, W) uint16."""

    def __init__(self, batch: int, C: int, H: int, W: int, *, sigma: float = 2.0, radius: int = 2,
                 min_distance: int = 5, max_cells: int = 4096, dapi_index: int = 1, ctx: Context | None = None,
                 props: bool = True, profile: bool = False, fused: bool = True, low_traffic: bool = False, bin_plane: bool = True,
                 prefix_plane: bool = True, relief: str = "seeded", ties: str = "exact", fill_holes: bool = False,
                 min_size: int = 0):
        self.ctx = ctx or get_context()
        self.B, self.C, self.H, self.W = int(batch), int(C), int(H), int(W)
        self.sigma, self.radius, self.min_distance = float(sigma), int(radius), int(min_distance)
        self.max_cells, self.dapi_index, self.props = int(max_cells), int(dapi_index), bool(props)
        # fused = watershed + clear_border + relabel in one C-ABI call (self.ws is then only flood scratch: use
        # fused=False to inspect the watershed image itself)
        self.fused = bool(fused)
        # relief: "seeded" = the config-3 recipe (marker pixels spread first: oracle/skops.py:seeded_flood_image; cannot
        # tie); "plain" = SURVEY.md A.8 as written, watershed(-edt, markers, mask), whose equal-valued markers are
        # resolved by ``ties`` ('exact' = scikit-image's single heap, emulated for the planes that tie)
        if relief not in ("seeded", "plain"):
            raise ValueError(f"relief must be 'seeded' or 'plain', got {relief!r}")
        self.relief, self.ties = relief, ties
        if relief == "plain":
            self.fused = False
        self.tied = None  # per-plane tie flags of the last plain-relief run
        # low_traffic = Gaussian -> Otsu -> '>' through amt_gaussian_otsu_codes: the float64 smoothed planes are never
        # made (8 instead of 26 bytes of HBM traffic per pixel, 25 MB less memory per field of view; same masks, same
        # thresholds).  Off by default: the Gaussian is fp64-issue bound, so computing it twice costs more time than
        # the two reads of the float64 plane it saves (rocprofv3, 32 FOVs: 1.13 ms against 0.93 ms)
        self.low_traffic = bool(low_traffic)
        # bin_plane: the Otsu histogram pass leaves every sample's bin as a byte plane and '>' reads that plane
        # (amt_otsu_f64_bins / amt_threshold_open_close); False = compare the float64 plane (same masks)
        self.bin_plane = bool(bin_plane)
        # prefix_plane (the default where amt_gaussian_otsu_codes takes the batch and neither of the two switches above
        # asks for another path): ONE Gaussian pass stores the upper 32 bits of every float64 sample, the histogram pass
        # reads those and leaves 2-byte codes -- 6 instead of 9 bytes per pixel held and moved, same masks and
        # thresholds.  False = the float64 plane + byte bins
        self.prefix_plane = bool(prefix_plane)
        # fill_holes: scipy.ndimage.binary_fill_holes (cross structure) between the closing and the EDT, so that a
        # nucleus whose dim centre left a ring in the mask is one basin, not arcs; the filled mask lands in mask_b
        self.fill_holes = bool(fill_holes)
        # min_size > 1: skimage.morphology.remove_small_objects (4-connected, as the watershed's own mask labelling) after
        # the closing and the hole filling, before the EDT: debris that survived the opening gets no peak, no marker, no
        # basin and no feature row.  Written to the other of mask_a / mask_b; 0 (the default) launches nothing
        if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 0:
            raise ValueError(f"min_size must be a non-negative int, got {min_size!r}")
        self.min_size = int(min_size)
        self.footprint = hipops.disk(self.radius)
        c, B = self.ctx, self.B
        shp = (B, self.H, self.W)
        # Gaussian -> Otsu -> '>' without the float64 image when the fused path takes this shape (2-byte codes instead)
        self.codes_path = self.prefix_path = None  # decided on the first batch (needs the batch's alignment)
        self._gauss = None
        self.codes = self.thr_code = self.ghist = self._prefix = None
        self._bins = self._thr_code = None
        self.thr = c.empty((B,), np.float64)
        self.gmm = c.empty((B, 2), np.float64)  # [min, max] of the smoothed image, folded in by the Gaussian
        self.mask_a = c.empty(shp, np.uint8)
        self.mask_b = c.empty(shp, np.uint8)
        self.labels8 = None  # config 2 only, allocated on demand
        self.count8 = c.empty((B,), np.int32)
        self.d2 = c.empty(shp, np.int32)
        self.peaks = c.zeros(shp, np.uint8)  # zeroed once; see self._marker_keep
        # marker planes are zeroed ONCE: every run clears only the pixels the previous run wrote (peak_markers keep=)
        self.markers = c.zeros(shp, np.int32)
        self._marker_keep = (c.empty((B, hipops.label_sparse_capacity(self.H, self.W)), np.int32), c.zeros((B,), np.int32))
        self.nmarkers = c.zeros((B,), np.int32)
        self.ws = c.empty(shp, np.int32)
        self.labels = c.empty(shp, np.int32)
        self.ncells = c.empty((B,), np.int32)
        self.table = c.empty((B, self.max_cells, _hip.RP_NCOLS), np.float64)
        self.itable = c.empty((B, self.max_cells, self.C, 4), np.float64)
        self.times = StageTimes(self.ctx) if profile else None
        self._ran = None

    # ---------------------------------------------------------------------------------------------
    def _stage(self, name):
        if self.times is not None:
            if getattr(self, "_open", None) is not None:
                self._open.stop()
            self._open = self.times.begin(name)

    def _end(self):
        if self.times is not None and getattr(self, "_open", None) is not None:
            self._open.stop()
            self._open = None

    def _check_fovs(self, fovs: DeviceArray) -> DeviceArray:
        """Validate the batch and bind it to THIS segmenter's context: operators run on the stream of their
        input's context, and a batch part may have been uploaded by another context (bench.py's stream split, the
        feeder's buffers) -- every kernel of the chain must be on self.ctx's stream."""
        if fovs.dtype != np.uint16 or fovs.shape != (self.B, self.C, self.H, self.W):
            raise ValueError(f"expected uint16 FOV batch of shape {(self.B, self.C, self.H, self.W)}, got "
                             f"{fovs.dtype} {fovs.shape}")
        return fovs.on(self.ctx)

    def mask_chain(self, fovs: DeviceArray) -> DeviceArray:
        """Gaussian -> Otsu -> '>' -> opening -> closing on the DAPI channel of every FOV."""
        if self.codes_path is None:
            supported = hipops.gaussian_otsu_codes_supported(fovs, self.sigma, channel=self.dapi_index)
            self.codes_path = self.low_traffic and supported  # the two-pass form
            self.prefix_path = self.prefix_plane and self.bin_plane and not self.low_traffic and supported
            if self.codes_path or self.prefix_path:
                shp = (self.B, self.H, self.W)
                self.codes = self.ctx.empty(shp, np.uint16)
                self.thr_code = self.ctx.empty((self.B,), np.float64)
                self.ghist = self.ctx.empty((self.B, 256), np.uint32)
                if self.prefix_path:
                    self._prefix = self.ctx.empty(shp, np.uint32)
        if self.codes_path or self.prefix_path:
            # `gaussian > thr` is exactly `codes > thr_code`, and the float64 plane (8 B/px written, read twice) is never
            # made: one Gaussian pass + the prefix plane + a histogram pass, or (low_traffic) two Gaussian passes
            self._stage("gaussian_otsu")
            hipops.gaussian_otsu_codes(fovs, self.sigma, self.codes, self.thr, self.thr_code, self.gmm, self.ghist,
                                       channel=self.dapi_index, prefix=self._prefix)
            self._stage("threshold_open_close")
            hipops.threshold_open_close(self.codes, self.thr_code, self.footprint, out=self.mask_a)
            return self.mask_a
        self._stage("gaussian")
        hipops.gaussian(fovs, self.sigma, channel=self.dapi_index, out=self.gauss, minmax_out=self.gmm)
        if not self.bin_plane:
            self._stage("otsu")
            hipops.threshold_otsu(self.gauss, out=self.thr, minmax=self.gmm)
            self._stage("threshold_open_close")
            hipops.threshold_open_close(self.gauss, self.thr, self.footprint, out=self.mask_a)
            return self.mask_a
        if self._bins is None:
            # the histogram pass leaves every sample's bin as a byte plane, and the threshold comparison reads that
            # plane instead of the float64 one (8 -> 1 byte per pixel, identical masks)
            self._bins = self.ctx.empty((self.B, self.H, self.W), np.uint8)
            self._thr_code = self.ctx.empty((self.B,), np.float64)
        self._stage("otsu")
        hipops.threshold_otsu_bins(self.gauss, self.gmm, self.thr, self._thr_code, self._bins)
        # '>' + opening + closing as one bit-packed chain (identical to the three separate operators)
        self._stage("threshold_open_close")
        hipops.threshold_open_close(self.gauss, self.thr, self.footprint, out=self.mask_a, bins=self._bins,
                                    thr_code=self._thr_code)
        return self.mask_a

    def _mask(self, fovs: DeviceArray) -> DeviceArray:
        """``mask_chain``, with ``fill_holes`` its result filled into ``mask_b``, with ``min_size`` the small components
        removed into the other of the two mask buffers: what the stages downstream use."""
        mask = self.mask_chain(fovs)
        if self.fill_holes:
            self._stage("fill_holes")
            mask = hipops.binary_fill_holes(mask, out=self.mask_b)
        if self.min_size > 1:
            self._stage("remove_small")
            mask = hipops.remove_small_objects(mask, self.min_size, connectivity=1,
                                               out=self.mask_a if mask is self.mask_b else self.mask_b)
        return mask

    @property
    def gauss(self) -> DeviceArray:
        """The float64 smoothed DAPI planes of the separate-operator path (allocated on first use)."""
        if self._gauss is None:
            self._gauss = self.ctx.empty((self.B, self.H, self.W), np.float64)
        return self._gauss

    def run_c2(self, fovs: DeviceArray) -> DeviceArray:
        """BASELINE configs[1]: the mask chain + 8-connected labelling.  Returns int32 labels (B, H, W)."""
        fovs = self._check_fovs(fovs)
        if self.labels8 is None:
            self.labels8 = self.ctx.empty((self.B, self.H, self.W), np.int32)
        mask = self._mask(fovs)
        self._stage("label8")
        hipops.label(mask, 2, out=self.labels8, count=self.count8)
        self._end()
        self._ran = "c2"
        return self.labels8

    def run_c3(self, fovs: DeviceArray) -> DeviceArray:
        """BASELINE configs[2]: nuclei watershed + morphology / intensity tables.  Returns int32 labels."""
        fovs = self._check_fovs(fovs)
        mask = self._mask(fovs)
        self._stage("edt")
        hipops.edt(mask, want_edt=False, d2_out=self.d2)
        self._stage("peaks")
        # peak search + sparse labelling of the peaks it lists, one call: neither plane is scanned for its few peaks
        hipops.peak_markers(self.d2, mask, self.min_distance, 1, peaks=self.peaks, markers=self.markers,
                            count=self.nmarkers, keep=self._marker_keep)
        if self.fused:
            # watershed + clear_border + relabel_sequential in one call: the watershed image is never written out
            # (self.ws only receives the pixels of flooded components); the list of marker pixels peak_markers keeps
            # spares its statistics pass the marker plane
            self._stage("watershed_clear_relabel")
            hipops.watershed_edt_cleared(self.d2, self.markers, mask, self.nmarkers, self.max_cells, scratch=self.ws,
                                         out=self.labels, count=self.ncells, marker_list=self._marker_keep)
        else:
            self._stage("watershed")
            if self.relief == "plain":
                if self.tied is None:
                    self.tied = self.ctx.zeros((self.B,), np.int32)
                hipops.watershed_edt(self.d2, self.markers, mask, seeds_first=False, out=self.ws, ties=self.ties,
                                     ties_out=self.tied)
            else:
                hipops.watershed_edt(self.d2, self.markers, mask, seeds_first=True, out=self.ws)
            # every watershed label is one 4-connected region grown from one marker component, so
            # clear_border + relabel_sequential (R/masks.py:56,65) collapse into one flag-and-renumber pass; the
            # markers lie inside the mask, so exactly the labels 1..nmarkers occur in the result
            self._stage("clear_border")
            hipops.clear_border_relabel(self.ws, self.max_cells, out=self.labels, count=self.ncells,
                                        nlabels=self.nmarkers)
        if self.props:
            self._stage("regionprops")
            hipops.regionprops_full(self.labels, fovs, self.max_cells, out=self.table, iout=self.itable)
        self._end()
        self._ran = "c3"
        return self.labels

    # ---------------------------------------------------------------------------------------------
    def result(self, channel_names=DEFAULT_CHANNELS) -> "SegmentationResult":
        if self._ran != "c3":
            raise RuntimeError("run_c3() has not been called")
        nm = self.nmarkers.numpy()
        if (nm < 0).any():
            raise _hip.HipError("the peak mask of a field of view exceeded the sparse-labelling capacity")
        if (nm > self.max_cells).any():
            raise _hip.HipError(
                f"a field of view produced {int(nm.max())} markers but max_cells={self.max_cells}; "
                "raise max_cells")
        return SegmentationResult(self, channel_names)


class SegmentationResult:
    """Views onto a finished config-3 run; host copies are made lazily."""

    def __init__(self, seg: FovSegmenter, channel_names):
        self.seg = seg
        self.channel_names = tuple(channel_names)
        self.ncells = seg.ncells.numpy()

    def labels_device(self) -> DeviceArray:
        return self.seg.labels

    def labels_numpy(self) -> np.ndarray:
        """int64 label images (B, H, W), background 0 (dtype contract: R/model.py:215, R/masks.py:63-65)."""
        return self.seg.labels.numpy_int64()

    def feature_tables(self) -> list[dict[str, np.ndarray]]:
        """One dict per FOV with the keys of ``SegmentationMask.cell_properties`` (R/masks.py:247-328,
        default property lists R/masks.py:15-35)."""
        t = self.seg.table.numpy()
        it = self.seg.itable.numpy() if self.seg.props else None
        out = []
        for b in range(self.seg.B):
            k = int(self.ncells[b])
            out.append(assemble_cell_properties(t[b, :k], None if it is None else it[b, :k], self.channel_names))
        return out


# extended columns (scikit-image 0.25.2 names): from the device table of amt_regionprops_ext, or on the host from the
# area and the bounding box (area_bbox, extent, equivalent_diameter_area, as regionprops defines them)
EXT_DEVICE_PROPERTIES = ("euler_number", "perimeter_crofton", "area_filled", "feret_diameter_max", "centroid_local",
                         "inertia_tensor", "inertia_tensor_eigvals")
EXT_HOST_PROPERTIES = ("area_bbox", "extent", "equivalent_diameter_area")
WEIGHTED_PROPERTIES = ("centroid_weighted", "centroid_weighted_local")
_INTENSITY_STATS = {"intensity_mean": 0, "intensity_max": 1, "intensity_min": 2, "intensity_std": 3}


def ext_columns(property_names, intensity_property_names) -> list[str]:
    """The names ``hipops.regionprops_ext`` has to compute for these property lists (weighted centroids only count
    from the intensity list: in ``property_names`` they raise, as regionprops does without an intensity image)."""
    want = [p for p in property_names if p in EXT_DEVICE_PROPERTIES]
    want += [p for p in intensity_property_names if p in WEIGHTED_PROPERTIES]
    return list(dict.fromkeys(want))


def assemble_cell_properties(morph: np.ndarray, inten: np.ndarray | None, channel_names,
                             property_names=None, intensity_property_names=None, ext: np.ndarray | None = None,
                             wext: np.ndarray | None = None) -> dict[str, np.ndarray]:
    """Device tables -> the dict R/masks.py:247-328 builds (same keys, same order, derived columns on the
    host exactly as the reference derives them: circularity :292-297, volume :302-305, renames :311-314).
    ``ext`` (k, RPX_NCOLS) / ``wext`` (k, C, 4) are the tables of ``hipops.regionprops_ext`` for the extended names;
    array-valued properties are split with ``-`` as regionprops_table splits them."""
    from .masks import DEFAULT_CELL_PROPERTY_NAMES, DEFAULT_INTENSITY_PROPERTY_NAMES

    property_names = list(DEFAULT_CELL_PROPERTY_NAMES if property_names is None else property_names)
    if intensity_property_names is None:
        intensity_property_names = list(DEFAULT_INTENSITY_PROPERTY_NAMES) if inten is not None else []
    col = {c: morph[:, i] for i, c in enumerate(_hip.RP_COLS)}
    xcol = {} if ext is None else {c: ext[:, i] for i, c in enumerate(_hip.RPX_COLS)}
    k = morph.shape[0]
    needs_circ = "circularity" in property_names
    needs_vol = "volume" in property_names
    sk_props = [p for p in property_names if p not in ("circularity", "volume")]
    added = set()
    for dep in ["area", "perimeter"] if needs_circ else []:
        if dep not in sk_props:
            sk_props.append(dep)
            added.add(dep)
    for dep in ["axis_major_length", "axis_minor_length"] if needs_vol else []:
        if dep not in sk_props:
            sk_props.append(dep)
            added.add(dep)
    props: dict[str, np.ndarray] = {}
    for p in sk_props:
        if p == "label":
            props["label"] = np.arange(1, k + 1, dtype=np.int64)
        elif p == "centroid":
            props["centroid-0"] = col["centroid-0"].copy()
            props["centroid-1"] = col["centroid-1"].copy()
        elif p == "bbox":
            for i in range(4):
                props[f"bbox-{i}"] = col[f"bbox-{i}"].astype(np.int64)
        elif p in col:
            props[p] = col[p].copy()
        elif p in EXT_HOST_PROPERTIES:
            area_bbox = (col["bbox-2"] - col["bbox-0"]) * (col["bbox-3"] - col["bbox-1"])
            if p == "area_bbox":
                props[p] = area_bbox
            elif p == "extent":
                with np.errstate(divide="ignore", invalid="ignore"):
                    props[p] = col["area"] / area_bbox
            else:
                props[p] = (2 * 2 * col["area"] / np.pi) ** (1 / 2)
        elif p in EXT_DEVICE_PROPERTIES:
            if ext is None:
                raise ValueError(f"property '{p}' needs the extended region-property table")
            keys = [c for c in _hip.RPX_COLS if c == p or c.startswith(p + "-")]
            for c in keys:
                props[c] = xcol[c].astype(np.int64) if p == "euler_number" else xcol[c].copy()
        elif p in WEIGHTED_PROPERTIES:
            raise AttributeError(f"property '{p}' needs an intensity image (list it in intensity_property_names)")
        else:
            raise AttributeError(f"property '{p}' is not available on the device path")
    if needs_circ:
        area, per = props["area"], props["perimeter"]
        with np.errstate(divide="ignore", invalid="ignore"):
            props["circularity"] = np.where(per > 0, (4.0 * np.pi * area) / (per**2), 0.0)
    if needs_vol:
        a = props["axis_major_length"] / 2.0
        b = props["axis_minor_length"] / 2.0
        props["volume"] = np.where((a > 0) & (b > 0), (4.0 / 3.0) * np.pi * a * b * b, 0.0)
    for p in added:
        props.pop(p, None)
    if "centroid-0" in props:
        props["centroid_y"] = props.pop("centroid-0")
    if "centroid-1" in props:
        props["centroid_x"] = props.pop("centroid-1")
    if inten is not None and intensity_property_names:
        for ci, name in enumerate(channel_names):
            suffix = str(name).lower()
            for p in intensity_property_names:
                if p in _INTENSITY_STATS:
                    props[f"{p}_{suffix}"] = inten[:, ci, _INTENSITY_STATS[p]].copy()
                elif p in WEIGHTED_PROPERTIES:
                    if wext is None:
                        raise ValueError(f"intensity property '{p}' needs the weighted-centroid table")
                    for i, c in enumerate(_hip.RPX_WCOLS):
                        if c.rsplit("-", 1)[0] == p:
                            props[f"{c}_{suffix}"] = wext[:, ci, i].copy()
                else:
                    raise AttributeError(f"intensity property '{p}' is not available on the device path")
    return props


def cell_property_keys(channel_names, property_names=None, intensity_property_names=None) -> list[str]:
    """The keys ``assemble_cell_properties`` gives for these lists, in order (no device needed)."""
    C = len(channel_names)
    return list(assemble_cell_properties(np.zeros((0, _hip.RP_NCOLS)), np.zeros((0, C, 4)) if C else None,
                                         channel_names, property_names, intensity_property_names,
                                         ext=np.zeros((0, _hip.RPX_NCOLS)), wext=np.zeros((0, C, 4))))


def colocalization_pairs(channel_names, pairs=None) -> list[tuple[int, int]]:
    """Channel-index pairs for ``colocalization_keys`` / ``SegmentationMask.cell_colocalization``: every i < j in
    channel order for ``pairs=None``; else each (a, b) of ``pairs``, whose members are indices, names (any case) or
    objects with a ``name`` (a ``Channel``), must be two different channels of ``channel_names``."""
    names = [str(getattr(c, "name", c)).lower() for c in channel_names]
    if len(names) < 2:
        raise ValueError("colocalization needs at least two channels")
    if pairs is None:
        return [(i, j) for i in range(len(names)) for j in range(i + 1, len(names))]

    def index(member):
        if isinstance(member, (int, np.integer)) and not isinstance(member, bool):
            if not 0 <= int(member) < len(names):
                raise ValueError(f"pair member {member!r} is not a channel index below {len(names)}")
            return int(member)
        name = str(getattr(member, "name", member)).lower()
        if name not in names:
            raise ValueError(f"pair member {member!r} is not one of the channels {names}")
        return names.index(name)

    out = []
    for pair in pairs:
        if isinstance(pair, (str, bytes)) or len(pair) != 2:
            raise TypeError(f"pairs must be (channel, channel) tuples, got {pair!r}")
        i, j = index(pair[0]), index(pair[1])
        if i == j:
            raise ValueError(f"pair {pair!r} names the same channel twice")
        out.append((i, j))
    if not out:
        raise ValueError("pairs must name at least one pair of channels")
    return out


def colocalization_keys(channel_names, pairs=None) -> list[str]:
    """The keys of ``SegmentationMask.cell_colocalization`` for these channels, in order (no device needed): per pair
    (a, b), ``f"{measure}_{a}_{b}"`` for the measures of ``_hip.COLOC_COLS`` with the lower-cased channel names,
    e.g. ``pearson_fitc_tritc``."""
    names = [str(getattr(c, "name", c)).lower() for c in channel_names]
    return [f"{m}_{names[i]}_{names[j]}" for i, j in colocalization_pairs(channel_names, pairs) for m in _hip.COLOC_COLS]


def robust_intensity_keys(channel_names) -> list[str]:
    """The keys of ``SegmentationMask.cell_robust_intensity`` for these channels, in order (no device needed): channel
    by channel ``f"intensity_{stat}_{channel}"`` for the statistics of ``_hip.RPX_QCOLS`` with the lower-cased channel
    names, e.g. ``intensity_q25_dapi``, ``intensity_median_dapi``, ``intensity_q75_dapi``, ``intensity_mad_dapi``."""
    names = [str(getattr(c, "name", c)).lower() for c in channel_names]
    return [f"intensity_{stat}_{name}" for name in names for stat in _hip.RPX_QCOLS]


def texture_keys(channel_names, distance: int = 1, angles: str = "each") -> list[str]:
    """The keys of ``SegmentationMask.cell_texture`` for these channels, in order (no device needed): channel by
    channel, angle by angle (``_hip.TEX_ANGLES``), feature by feature (``_hip.TEX_COLS``),
    ``f"texture_{feature}_{channel}_{distance}_{angle}"`` with the lower-cased channel names, e.g.
    ``texture_contrast_dapi_1_45``; with ``angles="mean"`` one key per feature and channel,
    ``f"texture_{feature}_{channel}_{distance}"``."""
    if angles not in ("each", "mean"):
        raise ValueError(f"angles must be 'each' or 'mean', got {angles!r}")
    if isinstance(distance, bool) or not isinstance(distance, (int, np.integer)):
        raise TypeError(f"distance must be an integer, got {distance!r}")
    names = [str(getattr(c, "name", c)).lower() for c in channel_names]
    if angles == "mean":
        return [f"texture_{f}_{name}_{int(distance)}" for name in names for f in _hip.TEX_COLS]
    return [f"texture_{f}_{name}_{int(distance)}_{a}" for name in names for a in _hip.TEX_ANGLES for f in _hip.TEX_COLS]


def radial_keys(channel_names, bins: int = 4) -> list[str]:
    """The keys of ``SegmentationMask.cell_radial_distribution`` for these channels, in order (no device needed):
    ``maximum_radius`` and ``mean_radius``, then channel by channel, ring by ring (1 = the innermost), measure by
    measure (``_hip.RAD_COLS``) ``f"radial_{measure}_{channel}_{i}of{bins}"`` with the lower-cased channel names, e.g.
    ``radial_frac_at_d_fitc_1of4``."""
    bins = hipops.radial_parameters(bins)
    names = [str(getattr(c, "name", c)).lower() for c in channel_names]
    return list(_hip.RAD_GEOM_COLS) + [f"radial_{m}_{name}_{i}of{bins}" for name in names
                                        for i in range(1, bins + 1) for m in _hip.RAD_COLS]


def neighbor_keys() -> list[str]:
    """The keys of ``SegmentationMask.cell_neighbors``, in order (no device needed): the contact census of
    ``_hip.RPX_NCOLS4`` with ``percent_touching`` after the two pixel counts it is made of, then the two closest cells
    of ``_hip.RPX_DCOLS``."""
    return ["number_of_neighbors", "touching_pixels", "ring_pixels", "percent_touching", "main_neighbor",
            "first_closest_label", "first_closest_distance", "second_closest_label", "second_closest_distance"]


def skeleton_keys() -> list[str]:
    """The keys of ``SegmentationMask.cell_skeleton``, in order (no device needed): the five pixel counts of
    ``_hip.LCEN_COLS`` (int64), then ``skeleton_length`` (float64), made of the two link counts."""
    return ["skeleton_pixels", "skeleton_isolated", "skeleton_ends", "skeleton_path_pixels", "skeleton_junction_pixels",
            "skeleton_length"]


def spot_keys(channel) -> list[str]:
    """The keys of ``SegmentationMask.cell_spots`` for this channel, in order (no device needed):
    ``spot_count_<ch>`` (int64), ``spot_intensity_sum_<ch>`` and ``spot_intensity_mean_<ch>`` (float64) with the
    lower-cased channel name, e.g. ``spot_count_fitc``."""
    name = str(getattr(channel, "name", channel)).lower()
    return [f"spot_count_{name}", f"spot_intensity_sum_{name}", f"spot_intensity_mean_{name}"]


def segment_fovs(fovs, *, ctx: Context | None = None, channel_names=DEFAULT_CHANNELS, **kw) -> SegmentationResult:
    """Convenience: (B, C, H, W) uint16 (numpy or DeviceArray) -> config-3 ``SegmentationResult``."""
    ctx = ctx or get_context()
    d = fovs if isinstance(fovs, DeviceArray) else ctx.asarray(np.ascontiguousarray(fovs, dtype=np.uint16))
    B, C, H, W = d.shape
    seg = FovSegmenter(B, C, H, W, ctx=ctx, **kw)
    seg.run_c3(d)
    return seg.result(channel_names)
