"""Time ``hipops.relate_labels`` on nuclei label planes against their ``expanded(12)`` labels (device events), with the
two operators that traverse the same bounding boxes as yardsticks, and the host route it replaces.

    python tools/time_relate.py [--fovs 48] [--size 2048] [--distinct 8] [--reps 20] [--json profiles/relate.json]

The label planes are the config-3 nuclei of ``synth.synth_fov`` (what bench.py measures), made by ``FovSegmenter`` for
``--distinct`` fields of view and repeated to ``--fovs`` planes; the companion planes are ``hipops.expand_labels`` of
the same planes by 12 pixels.  The three operators are timed in turns inside one loop, after two warm-up calls each, so
all see the same machine.  Prints one JSON line and writes it to ``--json``:

  relate_ms               median milliseconds per call of ``hipops.relate_labels`` (all planes, one companion)
  weighted_ms             ``hipops.regionprops_ext(["centroid_weighted"])`` with one uint16 channel: the same box traversal,
                          a companion plane of half the bytes
  intensity_ms            ``hipops.regionprops_intensity`` with the same channel
  relate_over_weighted, relate_over_intensity   the ratios of the medians
  device_route_ms         ``nuclei.relate(cells)`` of one field of view whose planes are on the device (host clock)
  host_route_ms           what it replaces: both label images downloaded, then ``np.unique`` on the pair keys
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

import relate_reference as rr  # noqa: E402
from arcadia_microscopy_tools_amd import _hip, hipops, synth  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fovs", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "relate.json"))
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
    labels = ctx.empty((a.fovs, a.size, a.size), np.int32)
    channel = ctx.empty((a.fovs, 1, a.size, a.size), np.uint16)
    for i in range(a.fovs):
        j = i % distinct
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, labels[i].ptr, some[j].ptr, some[j].nbytes), "amt_memcpy_d2d")
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, channel[i].ptr, some_images[j][1].ptr, some_images[j][1].nbytes),
                   "amt_memcpy_d2d")
    cells = hipops.expand_labels(labels, 12)
    ctx.synchronize()
    out = {"fovs": a.fovs, "size": a.size, "distinct": distinct, "reps": a.reps,
           "cells_per_fov": round(float(ncells.mean()), 1), "max_label": k}
    table = ctx.empty((a.fovs, k, 1, 4), np.float64)
    wtable = ctx.empty((a.fovs, k, 1, 4), np.float64)
    itable = ctx.empty((a.fovs, k, 1, 4), np.float64)
    relate, weighted, intensity = _event_ms_in_turns(ctx, [
        lambda: hipops.relate_labels(labels, k, cells, out=table),
        lambda: hipops.regionprops_ext(labels, k, ["centroid_weighted"], intensity=channel, wout=wtable),
        lambda: hipops.regionprops_intensity(labels, channel, k, out=itable)], a.reps)
    for name, t in (("relate", relate), ("weighted", weighted), ("intensity", intensity)):
        out[f"{name}_ms"] = round(t[0], 4)
        out[f"{name}_ms_min_max"] = [round(t[1], 4), round(t[2], 4)]
    out["relate_over_weighted"] = round(relate[0] / weighted[0], 3)
    out["relate_over_intensity"] = round(relate[0] / intensity[0], 3)
    again = ctx.empty(table.shape, np.float64)
    hipops.relate_labels(labels, k, cells, out=again)
    first = table.numpy()
    out["repeats_bit_for_bit"] = bool(first.tobytes() == again.numpy().tobytes())
    out["parent_is_own_label"] = bool(np.array_equal(
        first[0, :, 0, 0], np.where(first[0, :, 0, 3] > 0, np.arange(1, k + 1), 0).astype(np.float64)))

    # ---- one field of view, as a user sees it ----
    k0 = int(ncells[0])
    nuclei = SegmentationMask._from_device(labels[0], k0, None, None)
    grown = nuclei.expanded(12)
    device_ms, host_ms = [], []
    for rep in range(6):
        t0 = time.perf_counter()
        mine = nuclei.relate(grown)
        t1 = time.perf_counter()
        la = nuclei._label_plane()[0].numpy_int64()
        lb = grown._label_plane()[0].numpy_int64()
        other = rr.relate_columns(la, lb, k0)
        t2 = time.perf_counter()
        if rep:  # the first round warms both routes
            device_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
    out["device_route_ms"] = round(float(np.median(device_ms)), 3)
    out["host_route_ms"] = round(float(np.median(host_ms)), 3)
    out["routes_equal"] = bool(all(np.array_equal(mine[n], other[:, i]) for i, n in enumerate(_hip.RPX_RCOLS)))
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
