"""Time ``hipops.expand_labels`` on nuclei label planes (device events), with ``hipops.edt`` of the same planes'
foreground masks as the yardstick, and the end-to-end figure a user sees.

    python tools/time_expand_labels.py [--fovs 48] [--size 2048] [--distinct 8] [--reps 20]

The label planes are the config-3 nuclei of ``synth.synth_fov`` (what bench.py measures), made by ``FovSegmenter`` for
``--distinct`` fields of view and repeated to ``--fovs`` planes.  Prints one JSON line:

  expand_d<distance>_ms      median milliseconds per call on all planes, for distances 3, 12 and 32
  expand_d<distance>_hbm     that time's share of the HBM peak (8.0 TB/s) at the algorithmic 8 bytes per pixel
                             (int32 in, int32 out)
  edt_ms                     ``hipops.edt`` (squared distances) on the same planes' masks, same run
  device_route_ms            ``mask.expanded(12).cell_properties`` on one field of view (host clock; ends in a download)
  host_route_ms              what it replaces: ``label_image`` download -> scipy feature transform -> a new
                             ``SegmentationMask`` -> ``cell_properties``
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

HBM_PEAK = 8.0e12  # bytes per second
DISTANCES = (3, 12, 32)


def _event_ms(ctx, fn, reps):
    fn()  # warm-up: arena growth, code load
    fn()
    ctx.synchronize()
    ms = []
    for _ in range(reps):
        t = ctx.timer()
        t.start()
        fn()
        t.stop()
        ms.append(t.elapsed_ms())
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _host_expand(label_image, distance):
    """scikit-image's expand_labels on scipy's feature transform (what a user runs without the device operator)."""
    from scipy import ndimage as ndi

    distances, nearest = ndi.distance_transform_edt(label_image == 0, return_indices=True)
    out = np.zeros_like(label_image)
    m = distances <= distance
    out[m] = label_image[tuple(ix[m] for ix in nearest)]
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
    some = seg.run_c3(ctx.asarray(fovs))
    ncells = seg.ncells.numpy()
    host_labels = some.numpy()
    some_masks = ctx.asarray((host_labels > 0).astype(np.uint8))
    labels = ctx.empty((a.fovs, a.size, a.size), np.int32)
    masks = ctx.empty((a.fovs, a.size, a.size), np.uint8)
    for i in range(a.fovs):
        j = i % distinct
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, labels[i].ptr, some[j].ptr, some[j].nbytes), "amt_memcpy_d2d")
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, masks[i].ptr, some_masks[j].ptr, some_masks[j].nbytes), "amt_memcpy_d2d")
    ctx.synchronize()
    out = {"fovs": a.fovs, "size": a.size, "distinct": distinct, "reps": a.reps,
           "cells_per_fov": round(float(ncells.mean()), 1), "coverage": round(float((host_labels > 0).mean()), 4)}
    grown = ctx.empty(labels.shape, np.int32)
    pixels = a.fovs * a.size * a.size
    for d in DISTANCES:
        med, lo, hi = _event_ms(ctx, lambda d=d: hipops.expand_labels(labels, d, out=grown), a.reps)
        out[f"expand_d{d}_ms"] = round(med, 4)
        out[f"expand_d{d}_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        out[f"expand_d{d}_hbm"] = round(8.0 * pixels / (med * 1e-3) / HBM_PEAK, 4)
        if d == 12:
            out["coverage_d12"] = round(float((grown[0].numpy() > 0).mean()), 4)
    d2 = ctx.empty(labels.shape, np.int32)
    med, lo, hi = _event_ms(ctx, lambda: hipops.edt(masks, want_d2=True, want_edt=False, d2_out=d2), a.reps)
    out["edt_ms"] = round(med, 4)
    out["edt_ms_min_max"] = [round(lo, 4), round(hi, 4)]
    out["expand_d12_over_edt"] = round(out["expand_d12_ms"] / med, 2)
    del grown, d2, labels, masks

    # ---- one field of view, as a user sees it ----
    channels = {c: fovs[0][i] for i, c in enumerate((BRIGHTFIELD, DAPI, FITC, TRITC))}
    parent = SegmentationMask(host_labels[0].astype(np.int64), channels, remove_edge_cells=False)
    parent.cell_properties
    device_ms, host_ms = [], []
    for rep in range(6):
        t0 = time.perf_counter()
        table = parent.expanded(12).cell_properties
        t1 = time.perf_counter()
        image = parent._labels_device[0].numpy_int64()
        other = SegmentationMask(_host_expand(image, 12), channels, remove_edge_cells=False).cell_properties
        t2 = time.perf_counter()
        if rep:  # the first round warms both routes
            device_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
    out["device_route_ms"] = round(float(np.median(device_ms)), 3)
    out["host_route_ms"] = round(float(np.median(host_ms)), 3)
    # the two routes may differ on tied pixels only, so the cell count is the same
    out["routes_same_cells"] = bool(len(table["label"]) == len(other["label"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
