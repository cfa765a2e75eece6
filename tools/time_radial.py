"""Time ``hipops.radial_distribution`` (per-cell radial intensity distribution and inscribed radii) on nuclei label planes
with four uint16 channels (device events), with ``hipops.robust_intensity`` and ``hipops.regionprops_intensity`` on the
same buffers as the yardsticks, and the host route it replaces.

    python tools/time_radial.py [--fovs 48] [--size 2048] [--distinct 8] [--reps 20] [--json profiles/radial.json]

The label planes are the config-3 nuclei of ``synth.synth_fov`` (what bench.py measures), made by ``FovSegmenter`` for
``--distinct`` fields of view and repeated to ``--fovs`` planes; the intensity stacks are the four channels of the same
fields of view.  The operators are timed in turns inside one loop, after two warm-up calls each, so all see the same
machine.  Prints one JSON line and writes it to ``--json``:

  radial_ms               median milliseconds per call of ``hipops.radial_distribution`` (all planes, four channels, 4 bins)
  radial_geometry_ms      the same without channels (the distances, the radii and the ring counts alone)
  radial_b16_ms           16 bins
  radial_expanded_ms      4 bins on the planes grown by ``expand_labels(12)`` (cells instead of nuclei)
  robust_ms, intensity_ms ``hipops.robust_intensity`` and ``hipops.regionprops_intensity`` on the same buffers
  radial_over_robust, radial_over_intensity   the ratios of the medians
  device_route_ms         ``cell_radial_distribution()`` of one field of view whose label plane is on the device (host
                          clock; the four channel images are uploaded inside it)
  host_route_ms           what it replaces: the label image downloaded, a distance transform per cell on the crop to its
                          box (scipy), rings, wedges and columns with numpy
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import radial_cases as rc  # noqa: E402
import radial_reference as rr  # noqa: E402
from arcadia_microscopy_tools_amd import _hip, channels, hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.masks import SegmentationMask  # noqa: E402
from arcadia_microscopy_tools_amd.segment import DEFAULT_CHANNELS, FovSegmenter, radial_keys  # noqa: E402


def _event_ms_in_turns(ctx, fns, reps):
    """Median / min / max milliseconds of each callable, timed one after the other inside every repetition."""
    for fn in fns:  # warm-up: arena growth, code load
        fn()
        fn()
    ctx.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t = ctx.timer()
            t.start()
            fn()
            t.stop()
            ms[i].append(t.elapsed_ms())
    return [(float(np.median(m)), float(np.min(m)), float(np.max(m))) for m in ms]


def host_route(label_image, images, k, bins):
    """(geometry (k, 2), table (k, C, bins, 3)): per cell on the crop to its bounding box, framed with one ring of
    zeros -- scipy's exact Euclidean distance transform, squared back to integers, then the definitions with numpy"""
    from scipy import ndimage as ndi

    C = len(images)
    geom = np.full((k, 2), np.nan)
    table = np.full((k, C, bins, len(rr.COLS)), np.nan)
    for l, box in enumerate(ndi.find_objects(label_image, max_label=k)):
        if box is None:
            continue
        member = np.pad(label_image[box] == l + 1, 1)
        d2 = np.rint(ndi.distance_transform_edt(member) ** 2).astype(np.int64)[1:-1, 1:-1]
        ys, xs = np.nonzero(member[1:-1, 1:-1])
        d2 = d2[ys, xs]
        n, dmax2 = len(ys), int(d2.max())
        b = sum((d2 * bins * bins <= dmax2 * (bins - j) * (bins - j)).astype(np.int64) for j in range(1, bins))
        w = rr.wedges(ys, xs)
        geom[l] = (np.sqrt(float(dmax2)), np.sqrt(d2.astype(np.float64)).sum() / n)
        n_bw = np.bincount(b * 8 + w, minlength=bins * 8).reshape(bins, 8)
        for c in range(C):
            v = images[c][box][ys, xs].astype(np.int64)
            S_bw = np.zeros(bins * 8, np.int64)
            np.add.at(S_bw, b * 8 + w, v)
            S_bw = S_bw.reshape(bins, 8)
            for j in range(bins):
                table[l, c, j] = rr.ring_columns(S_bw, n_bw, j, n)
    return geom, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fovs", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "radial.json"))
    a = ap.parse_args()
    ctx = get_context()
    lib = _hip.load_library()
    distinct = max(1, min(a.distinct, a.fovs))
    fovs = np.stack([synth.synth_fov(i, size=a.size) for i in range(distinct)])
    C = int(fovs.shape[1])
    seg = FovSegmenter(distinct, C, a.size, a.size, ctx=ctx, props=False)
    some_images = ctx.asarray(fovs)
    some = seg.run_c3(some_images)
    ncells = seg.ncells.numpy()
    k = int(ncells.max())
    labels = ctx.empty((a.fovs, a.size, a.size), np.int32)
    stacks = ctx.empty((a.fovs, C, a.size, a.size), np.uint16)
    for i in range(a.fovs):
        j = i % distinct
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, labels[i].ptr, some[j].ptr, some[j].nbytes), "amt_memcpy_d2d")
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, stacks[i].ptr, some_images[j].ptr, some_images[j].nbytes),
                   "amt_memcpy_d2d")
    expanded = hipops.expand_labels(labels, 12)
    ctx.synchronize()
    B = a.bins
    out = {"fovs": a.fovs, "size": a.size, "channels": C, "distinct": distinct, "reps": a.reps,
           "cells_per_fov": round(float(ncells.mean()), 1), "max_label": k, "bins": B}
    gtable = ctx.empty((a.fovs, k, _hip.RAD_GEOM_NCOLS), np.float64)
    rtable = ctx.empty((a.fovs, k, C, B, _hip.RAD_NCOLS), np.float64)
    rtable16 = ctx.empty((a.fovs, k, C, 16, _hip.RAD_NCOLS), np.float64)
    qtable = ctx.empty((a.fovs, k, C, 4), np.float64)
    itable = hipops.regionprops_intensity(labels, stacks, k)
    timed = _event_ms_in_turns(ctx, [
        lambda: hipops.radial_distribution(labels, stacks, k, bins=B, out=rtable, geometry_out=gtable),
        lambda: hipops.robust_intensity(labels, stacks, k, out=qtable),
        lambda: hipops.regionprops_intensity(labels, stacks, k, out=itable),
        lambda: hipops.radial_distribution(labels, None, k, bins=B, geometry_out=gtable),
        lambda: hipops.radial_distribution(labels, stacks, k, bins=16, out=rtable16, geometry_out=gtable),
        lambda: hipops.radial_distribution(expanded, stacks, k, bins=B, out=rtable, geometry_out=gtable)], a.reps)
    for name, t in zip(("radial", "robust", "intensity", "radial_geometry", "radial_b16", "radial_expanded"), timed):
        out[f"{name}_ms"] = round(t[0], 4)
        out[f"{name}_ms_min_max"] = [round(t[1], 4), round(t[2], 4)]
    out["radial_over_robust"] = round(timed[0][0] / timed[1][0], 3)
    out["radial_over_intensity"] = round(timed[0][0] / timed[2][0], 3)
    first = [x.numpy().tobytes() for x in hipops.radial_distribution(labels, stacks, k, bins=B)]
    again = [x.numpy().tobytes() for x in hipops.radial_distribution(labels, stacks, k, bins=B)]
    out["repeats_bit_for_bit"] = bool(first == again)

    # ---- one field of view, as a user sees it ----
    k0 = int(ncells[0])
    names = [channels.CHANNELS[n] for n in DEFAULT_CHANNELS[:C]]
    images = {ch: fovs[0][c] for c, ch in enumerate(names)}
    mask = SegmentationMask._from_device(labels[0], k0, None, None, intensity_image_dict=images)
    keys = radial_keys(names, B)
    device_ms, host_ms = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        mine = mask.cell_radial_distribution(bins=B)
        t1 = time.perf_counter()
        lab = mask._label_plane()[0].numpy_int64()
        other = host_route(lab, list(images.values()), k0, B)
        t2 = time.perf_counter()
        if rep:  # the first round warms both routes
            device_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
    out["device_route_ms"] = round(float(np.median(device_ms)), 3)
    out["host_route_ms"] = round(float(np.median(host_ms)), 3)
    out["host_over_device"] = round(out["host_route_ms"] / out["device_route_ms"], 2)
    cols = np.stack([mine[key] for key in keys], axis=1)
    # the host's mean radius is a plain float64 sum: close, not equal; everything else bit for bit
    out["routes_agree"] = bool(rc.same_bits(cols[:, 0], other[0][:, 0]) and rc.close(cols[:, 1], other[0][:, 1])
                               and rc.same_bits(cols[:, 2:].reshape(other[1].shape), other[1]))
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
