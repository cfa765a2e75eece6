"""``MicroscopyImage`` and its metadata containers (reference: R/microscopy.py:17-308).

Same validation, properties, error messages and channel-slicing semantics as the reference.  Two
device-side additions: ``to_device()`` keeps the whole (..., C, Y, X) stack in HBM, where
``get_channel_intensities`` is a pointer offset (the reference returns a numpy view, R/microscopy.py:279-282),
and ``from_nd2_path`` reads the pixel block of uncompressed ND2 files with the built-in minimal reader
(``nd2lite``; the reference delegates to the ``nd2`` package, R/nikon.py:25-43).
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass, replace
from functools import cached_property
from pathlib import Path
from typing import Any

import numpy as np
from numpy import uint16

from .channels import Channel
from .exceptions import MetadataWarning
from .metadata_structures import ChannelMetadata, DimensionFlags
from .pipeline import Pipeline
from .typing import ScalarArray, UInt16Array


@dataclass
class InstrumentMetadata:
    """``sizes`` (e.g. {'C': 4, 'Y': 2048, 'X': 2048}) plus one ``ChannelMetadata`` per channel."""

    sizes: dict[str, int]
    channel_metadata_list: list[ChannelMetadata]

    def __post_init__(self) -> None:
        for key in ("X", "Y"):
            if key not in self.sizes:
                raise ValueError(
                    f"sizes must contain '{key}' dimension, got keys: {list(self.sizes.keys())}"
                )
        expected = self.sizes.get("C", 1)
        actual = len(self.channel_metadata_list)
        if actual != expected:
            raise ValueError(
                f"Number of channel metadata entries ({actual}) does not match "
                f"the channel dimension size ({expected}) in sizes"
            )

    @property
    def channel_axis(self) -> int | None:
        axes = list(self.sizes)
        return axes.index("C") if "C" in axes else None

    @cached_property
    def dimensions(self) -> DimensionFlags:
        flags = DimensionFlags(0)
        for cm in self.channel_metadata_list:
            flags |= cm.dimensions
        if len(self.channel_metadata_list) > 1:
            flags |= DimensionFlags.MULTICHANNEL
        return flags


@dataclass
class Metadata:
    """Instrument metadata plus optional sample metadata."""

    instrument: InstrumentMetadata
    sample: dict[str, Any] | None = None

    def __repr__(self) -> str:
        shown = [f"sizes={self.instrument.sizes}",
                 f"channels={[entry.channel.name for entry in self.instrument.channel_metadata_list]}"]
        if self.sample:
            shown.append(f"sample={self.sample}")
        return "<Metadata " + ", ".join(shown) + ">"


@dataclass
class MicroscopyImage:
    """Image intensities (canonically uint16) with metadata for all channels."""

    intensities: UInt16Array
    metadata: Metadata

    def __post_init__(self) -> None:
        sizes = self.metadata.instrument.sizes
        shape, wanted = self.intensities.shape, tuple(sizes.values())
        if shape != wanted:  # the axes of `sizes` ARE the axes of the array, in order (R/microscopy.py:117-123)
            raise ValueError(f"Intensities shape {shape} does not match metadata sizes {sizes} (expected shape {wanted})")
        dtype = self.intensities.dtype
        if dtype != uint16:  # uint16 is the canonical acquisition dtype (R/microscopy.py:125-131)
            note = f"Expected uint16 intensities, got {dtype}. Some operations may behave unexpectedly."
            warnings.warn(note, MetadataWarning, stacklevel=2)

    def __repr__(self) -> str:
        flat = self.intensities.reshape(-1)
        if flat.size <= 10:
            body = f"intensities={list(flat)}"
        else:
            head = ", ".join(map(str, flat[:3].tolist()))
            tail = ", ".join(map(str, flat[-3:].tolist()))
            body = f"intensities=[{head}, ..., {tail}]"
        names = [channel.name for channel in self.channels]
        return f"<MicroscopyImage sizes={self.sizes}, channels={names}, {body}, dtype={self.intensities.dtype}>"

    # -- constructors -----------------------------------------------------------------------------
    @classmethod
    def from_array(cls, intensities: np.ndarray, channels: list[Channel], axes: str | None = None,
                   sample_metadata: dict[str, Any] | None = None) -> "MicroscopyImage":
        """Build an image from a bare array: ``axes`` names the dimensions (default 'CYX' / 'YX')."""
        if axes is None:
            axes = "YX" if intensities.ndim == 2 else "CYX" if intensities.ndim == 3 else None
        if axes is None or len(axes) != intensities.ndim:
            raise ValueError("axes must name every dimension of intensities (e.g. 'TCYX')")
        sizes = {a: int(s) for a, s in zip(axes, intensities.shape)}
        meta = InstrumentMetadata(sizes, [ChannelMetadata(ch) for ch in channels])
        return cls(intensities, Metadata(meta, sample_metadata))

    @classmethod
    def from_nd2_path(cls, nd2_path: Path, channels: list[Channel] | None = None,
                      sample_metadata: dict[str, Any] | None = None) -> "MicroscopyImage":
        """Read an uncompressed ND2 file (reference: R/microscopy.py:154-176 -> R/nikon.py:25-43)."""
        from .nd2lite import load_nd2

        intensities, instrument = load_nd2(Path(nd2_path), channels)
        return cls(intensities, Metadata(instrument, sample_metadata))

    @classmethod
    def from_lif_path(cls, lif_path: Path, image_name: str, channels: list[Channel] | None = None,
                      sample_metadata: dict[str, Any] | None = None) -> "MicroscopyImage":
        """The reference reads Leica LIF files through the ``liffile`` package (R/microscopy.py:178-203,
        R/leica.py); file loaders other than uncompressed ND2 are outside this package: load the
        pixels with the reference's loader and hand them to ``from_array``."""
        raise NotImplementedError(
            "Leica LIF loading is not part of the MI355X hot path: read the image with the reference's "
            "arcadia_microscopy_tools.leica.load_lif_image and pass the array to MicroscopyImage.from_array"
        )

    # -- properties -------------------------------------------------------------------------------
    @property
    def shape(self) -> tuple[int, ...]:
        return self.intensities.shape

    @property
    def sizes(self) -> dict[str, int]:
        return self.metadata.instrument.sizes

    @property
    def dimensions(self) -> DimensionFlags:
        return self.metadata.instrument.dimensions

    @property
    def channels(self) -> list[Channel]:
        return [cm.channel for cm in self.metadata.instrument.channel_metadata_list]

    @property
    def channel_axis(self) -> int | None:
        return self.metadata.instrument.channel_axis

    @property
    def num_channels(self) -> int:
        return len(self.metadata.instrument.channel_metadata_list)

    @staticmethod
    def _resolve_channel_name(channel: str | Channel) -> str:
        return getattr(channel, "name", channel)

    # -- channel access (R/microscopy.py:241-282) ---------------------------------------------------
    def _channel_index(self, channel: str | Channel) -> int:
        name = self._resolve_channel_name(channel)
        names = [ch.name for ch in self.channels]
        if name not in names:
            raise ValueError(f"Channel '{name}' not found in image. Available channels: {names}")
        return names.index(name)

    def get_channel_intensities(self, channel: str | Channel) -> UInt16Array:
        """All data of one channel (T / Z axes preserved); a numpy VIEW, no copy."""
        index = self._channel_index(channel)
        if self.num_channels == 1:
            return self.intensities
        if self.channel_axis is None:
            raise ValueError("Channel axis not found in metadata")
        slices: list[slice | int] = [slice(None)] * self.intensities.ndim
        slices[self.channel_axis] = index
        return self.intensities[tuple(slices)]

    def apply_pipeline(self, pipeline: Pipeline, channel: str | Channel) -> ScalarArray:
        """``pipeline(self.get_channel_intensities(channel))`` (R/microscopy.py:284-308)."""
        return pipeline(self.get_channel_intensities(channel))

    # -- Z-stacks -----------------------------------------------------------------------------------
    def project_z(self, method: str = "max", reference_channel: str | Channel | None = None, **kwargs) -> "MicroscopyImage":
        """A new image without the ``Z`` axis: every combination of the other leading axes (T, P, C) is one stack of a
        batch that is uploaded once and collapsed by one call per operator.  ``method``: ``"max"`` / ``"min"`` (keep
        the dtype), ``"mean"`` (float64), ``"best_focus"`` (the plane with the largest ``operations.focus_scores``;
        kwargs: ``focus_method``, the ``method`` of ``operations.best_focus``, whose own name this call's ``method`` takes) or ``"edf"`` (``operations.extended_depth_of_field``; kwargs: ``radius``, ``smooth``).  With
        ``reference_channel`` the plane (``best_focus``) or the index map (``edf``) is chosen on that channel and applied
        to all channels of the same T / P; without it every channel chooses for itself.  ``sizes`` drops ``'Z'``, every
        channel loses ``DimensionFlags.Z_STACK`` and its resolution's z fields; everything else is kept."""
        plan = _ZPlan(self, method, reference_channel, kwargs)
        from .device import get_context

        lead = np.moveaxis(self.intensities, plan.z_axis, -3)
        batch = get_context().asarray(np.ascontiguousarray(lead).reshape(plan.batch_shape))
        out = plan.run(batch).numpy().reshape(plan.out_shape)
        return MicroscopyImage(out, plan.metadata)

    # -- device residency ---------------------------------------------------------------------------
    def to_device(self, ctx=None):
        """Upload the stack once; returns a ``DeviceImage`` whose channel access is a pointer offset."""
        from .device import get_context

        ctx = ctx or get_context()
        return DeviceImage(ctx.asarray(np.ascontiguousarray(self.intensities)), self)


_Z_METHODS = ("max", "min", "mean", "best_focus", "edf")
_Z_KWARGS = {"best_focus": ("focus_method",), "edf": ("radius", "smooth")}


class _ZPlan:
    """What ``project_z`` does to an image, settled from its metadata and arguments before any device access: the batch
    (N, Z, Y, X) with one stack per combination of the other leading axes in their order, the result's shape and
    metadata, and -- with a reference channel -- ``source[n]``, the stack whose choice stack n takes."""

    def __init__(self, image: MicroscopyImage, method: str, reference_channel, kwargs: dict):
        from . import operations

        sizes = image.sizes
        axes = list(sizes)
        if "Z" not in sizes:
            raise ValueError(f"project_z: the image has no 'Z' axis (sizes {sizes})")
        if axes[-2:] != ["Y", "X"]:
            raise ValueError(f"project_z: (Y, X) must be the last two axes, got {''.join(axes)}")
        if method not in _Z_METHODS:
            raise ValueError(f"project_z: method must be one of {_Z_METHODS}, got {method!r}")
        extra = sorted(set(kwargs) - set(_Z_KWARGS.get(method, ())))
        if extra:
            raise TypeError(f"project_z: method {method!r} takes no argument {extra[0]!r}")
        self.method = method
        self.focus_method = operations._focus_method("project_z", kwargs.get("focus_method", "laplacian_variance"))
        self.radius, self.smooth = operations._edf_args(kwargs.get("radius", 4), kwargs.get("smooth", 0))
        ref = None
        if reference_channel is not None:
            if method not in _Z_KWARGS:
                raise ValueError(f"project_z: reference_channel goes with 'best_focus' or 'edf', not {method!r}")
            ref = image._channel_index(reference_channel)
        self.z_axis = axes.index("Z")
        lead_axes = [a for a in axes[:-2] if a != "Z"]
        lead_shape = tuple(int(sizes[a]) for a in lead_axes)
        n = int(np.prod(lead_shape, dtype=np.int64))
        self.batch_shape = (n, int(sizes["Z"]), int(sizes["Y"]), int(sizes["X"]))
        self.out_shape = lead_shape + (int(sizes["Y"]), int(sizes["X"]))
        self.source = None
        if ref is not None and "C" in lead_axes and n:
            index = np.arange(n).reshape(lead_shape)
            chosen = np.take(index, [ref], axis=lead_axes.index("C"))
            self.source = np.broadcast_to(chosen, lead_shape).reshape(-1)
        instrument = image.metadata.instrument
        channel_metadata = []
        for cm in instrument.channel_metadata_list:
            res = cm.resolution
            if res is not None:
                res = replace(res, z_size_px=None, z_step_um=None)
            channel_metadata.append(replace(cm, dimensions=cm.dimensions & ~DimensionFlags.Z_STACK, resolution=res))
        new_sizes = {a: s for a, s in sizes.items() if a != "Z"}
        self.metadata = Metadata(InstrumentMetadata(new_sizes, channel_metadata), image.metadata.sample)

    def run(self, batch):
        """(N, Z, Y, X) on the device -> (N, Y, X) on the device"""
        from . import _hip, hipops, operations

        if self.method in ("max", "min", "mean"):
            return hipops.z_project(batch, self.method)
        N, _, H, W = batch.shape
        ctx = batch.ctx

        def copy_plane(dst, src):
            _hip.check(ctx._lib.amt_memcpy_d2d(ctx.handle, dst.ptr, src.ptr, src.nbytes), "amt_memcpy_d2d")

        if self.method == "best_focus":
            sums = hipops.focus_sums(batch).numpy()
            z = [int(np.argmax(operations._scores_from_sums(rows, H * W, self.focus_method))) for rows in sums]
            out = ctx.empty((N, H, W), batch.dtype)
            for n in range(N):
                copy_plane(out[n], batch[n][z[n] if self.source is None else z[int(self.source[n])]])
            return out
        if self.source is None:
            return operations._edf_batch(batch, self.radius, self.smooth, False)[0]
        # the index maps of the reference stacks alone where they lie back to back (C the first axis), else of all stacks
        refs = sorted(set(self.source.tolist()))
        contiguous = refs == list(range(refs[0], refs[-1] + 1))
        first = refs[0] if contiguous else 0
        chosen = hipops.focus_index(batch[refs[0]:refs[-1] + 1] if contiguous else batch, self.radius)
        if self.smooth:
            chosen = hipops.median(chosen, np.ones((self.smooth, self.smooth), np.uint8), mode="nearest")
        index = ctx.empty((N, H, W), np.uint16)
        for n in range(N):
            copy_plane(index[n], chosen[int(self.source[n]) - first])
        return hipops.z_take(batch, index)


class DeviceImage:
    """A ``MicroscopyImage`` whose intensities live in HBM."""

    def __init__(self, data, image: MicroscopyImage):
        self.data = data
        self.image = image

    def project_z(self, method: str = "max", reference_channel: str | Channel | None = None, **kwargs) -> "DeviceImage":
        """``MicroscopyImage.project_z`` without leaving the device.  The ``Z`` axis must stand right before (Y, X), as in
        the (C, Z, Y, X) block the ND2 reader returns, so that every stack is contiguous; the result's ``image`` carries
        the metadata only (its ``intensities`` is None)."""
        plan = _ZPlan(self.image, method, reference_channel, kwargs)
        if plan.z_axis != len(self.image.sizes) - 3:
            raise NotImplementedError("device Z projections need the Z axis right before (Y, X), e.g. (C, Z, Y, X); use the "
                                      "host image for other layouts")
        out = plan.run(self.data.reshape(plan.batch_shape))
        image = MicroscopyImage.__new__(MicroscopyImage)
        image.intensities, image.metadata = None, plan.metadata
        return DeviceImage(out.reshape(plan.out_shape), image)

    def get_channel_intensities(self, channel: str | Channel):
        """Device view of one channel.  Needs the channel axis to be the leading axis (or the one right
        before (Y, X) with all earlier axes of size 1) so that the channel is contiguous in memory."""
        img = self.image
        index = img._channel_index(channel)
        if img.num_channels == 1:
            return self.data
        axis = img.channel_axis
        if axis is None:
            raise ValueError("Channel axis not found in metadata")
        lead = int(np.prod(self.data.shape[:axis], dtype=np.int64))
        if lead != 1:
            raise NotImplementedError(
                "device channel views need the channel axis first (e.g. (C, Y, X) or (C, Z, Y, X)); "
                "use the host image for (T, C, Y, X) stacks"
            )
        flat = self.data.reshape(self.data.shape[axis:])
        return flat[index]
