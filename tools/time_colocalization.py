"""Time ``hipops.colocalization`` on nuclei label planes with their four uint16 channels (device events), with
``hipops.regionprops_intensity`` on the same buffers as the yardstick, and the end-to-end figure a user sees.

    python tools/time_colocalization.py [--fovs 48] [--size 2048] [--distinct 8] [--reps 20]

The label planes are the config-3 nuclei of ``synth.synth_fov`` (what bench.py measures), made by ``FovSegmenter`` for
``--distinct`` fields of view and repeated, with their images, to ``--fovs`` planes.  The two operators are timed in
turns inside one loop, so both see the same machine.  Prints one JSON line:

  coloc_ms            median milliseconds per call: all 6 channel pairs of all planes (exact uint16 path)
  intensity_ms        ``hipops.regionprops_intensity`` (mean, max, min, std of the 4 channels), same buffers, same run
  coloc_over_intensity   the ratio of the two medians
  coloc_f64_ms        the float64 path on the same images converted to float64 (``--distinct`` planes only)
  device_route_ms     ``mask.cell_colocalization()`` on one four-channel field of view (host clock; upload of the
                      images, the kernels, download of the table)
  host_route_ms       what it replaces: the label image downloaded, then a numpy loop over the cells' bounding boxes
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arcadia_microscopy_tools_amd import _hip, hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.channels import BRIGHTFIELD, DAPI, FITC, TRITC  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.masks import SegmentationMask  # noqa: E402
from arcadia_microscopy_tools_amd.segment import FovSegmenter  # noqa: E402


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


def _host_colocalization(label_image, images, thresholds):
    """The six measures of every channel pair of every cell: numpy on the cells' bounding boxes."""
    from scipy import ndimage as ndi

    C = len(images)
    pairs = [(i, j) for i in range(C) for j in range(i + 1, C)]
    boxes = ndi.find_objects(label_image)
    out = np.zeros((len(boxes), len(pairs), 6))
    for lab, box in enumerate(boxes, start=1):
        if box is None:
            out[lab - 1, :, :2] = np.nan
            continue
        sel = label_image[box] == lab
        vals = [img[box][sel].astype(np.float64) for img in images]
        for p, (i, j) in enumerate(pairs):
            a, b = vals[i], vals[j]
            pa, pb = a > thresholds[i], b > thresholds[j]
            da, db = a - a.mean(), b - b.mean()
            den = np.sqrt((da * da).sum() * (db * db).sum())
            oden = np.sqrt((a * a).sum() * (b * b).sum())
            both = (pa & pb).sum()
            out[lab - 1, p] = (
                (da * db).sum() / den if den else np.nan, (a * b).sum() / oden if oden else np.nan,
                a[pb].sum() / a.sum() if a.sum() else 0.0, b[pa].sum() / b.sum() if b.sum() else 0.0,
                both / pa.sum() if pa.sum() else 0.0, both / pb.sum() if pb.sum() else 0.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fovs", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx = get_context()
    lib = _hip.load_library()
    distinct = max(1, min(a.distinct, a.fovs))
    fovs = np.stack([synth.synth_fov(i, size=a.size) for i in range(distinct)])
    seg = FovSegmenter(distinct, 4, a.size, a.size, ctx=ctx, props=False)
    some_images = ctx.asarray(fovs)
    some = seg.run_c3(some_images)
    ncells = seg.ncells.numpy()
    k = int(ncells.max())
    host_labels = some.numpy()
    labels = ctx.empty((a.fovs, a.size, a.size), np.int32)
    images = ctx.empty((a.fovs, 4, a.size, a.size), np.uint16)
    for i in range(a.fovs):
        j = i % distinct
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, labels[i].ptr, some[j].ptr, some[j].nbytes), "amt_memcpy_d2d")
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, images[i].ptr, some_images[j].ptr, some_images[j].nbytes),
                   "amt_memcpy_d2d")
    ctx.synchronize()
    out = {"fovs": a.fovs, "size": a.size, "distinct": distinct, "reps": a.reps,
           "cells_per_fov": round(float(ncells.mean()), 1), "max_label": k}
    thresholds = ctx.asarray(np.tile(np.percentile(fovs[0], 50, axis=(1, 2)), (a.fovs, 1)))
    table = ctx.empty((a.fovs, k, 6, _hip.COLOC_NCOLS), np.float64)
    itable = ctx.empty((a.fovs, k, 4, 4), np.float64)
    (coloc, intensity) = _event_ms_in_turns(ctx, [
        lambda: hipops.colocalization(labels, images, k, thresholds=thresholds, out=table),
        lambda: hipops.regionprops_intensity(labels, images, k, out=itable)], a.reps)
    out["coloc_ms"] = round(coloc[0], 4)
    out["coloc_ms_min_max"] = [round(coloc[1], 4), round(coloc[2], 4)]
    out["intensity_ms"] = round(intensity[0], 4)
    out["intensity_ms_min_max"] = [round(intensity[1], 4), round(intensity[2], 4)]
    out["coloc_over_intensity"] = round(coloc[0] / intensity[0], 3)
    again = ctx.empty(table.shape, np.float64)
    hipops.colocalization(labels, images, k, thresholds=thresholds, out=again)
    out["repeats_bit_for_bit"] = bool(table.numpy().tobytes() == again.numpy().tobytes())
    del again, itable
    fimages = ctx.asarray(fovs.astype(np.float64))
    ftable = ctx.empty((distinct, k, 6, _hip.COLOC_NCOLS), np.float64)
    (f64,) = _event_ms_in_turns(ctx, [lambda: hipops.colocalization(some, fimages, k, thresholds=thresholds[:distinct],
                                                                    out=ftable)], max(3, a.reps // 4))
    out["coloc_f64_ms"] = round(f64[0], 4)
    out["coloc_f64_planes"] = distinct
    same = np.abs(ftable.numpy() - table.numpy()[:distinct])
    out["f64_vs_exact_max_abs"] = float(np.nanmax(same))
    del fimages, ftable, table, labels, images

    # ---- one field of view, as a user sees it ----
    channels = {c: fovs[0][i] for i, c in enumerate((BRIGHTFIELD, DAPI, FITC, TRITC))}
    parent = SegmentationMask(host_labels[0].astype(np.int64), channels, remove_edge_cells=False)
    parent.num_cells
    device_ms, host_ms = [], []
    for rep in range(6):
        t0 = time.perf_counter()
        mine = parent.cell_colocalization()
        t1 = time.perf_counter()
        image = parent._labels_device[0].numpy_int64()
        image = image.reshape(image.shape[-2:])
        other = _host_colocalization(image, list(channels.values()), [0.0] * 4)
        t2 = time.perf_counter()
        if rep:  # the first round warms both routes
            device_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
    out["device_route_ms"] = round(float(np.median(device_ms)), 3)
    out["host_route_ms"] = round(float(np.median(host_ms)), 3)
    flat = np.stack(list(mine.values()), axis=1).reshape(other.shape)
    out["routes_max_abs_difference"] = float(np.nanmax(np.abs(flat - other)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
