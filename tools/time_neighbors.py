"""Time ``hipops.neighbor_census`` and ``hipops.nearest_labels`` on nuclei label planes (device events), with
``hipops.relate_labels`` of the planes on themselves as the yardstick, and the host route they replace.

    python tools/time_neighbors.py [--fovs 48] [--size 2048] [--distinct 8] [--reps 20] [--json profiles/neighbors.json]

The label planes are the config-3 nuclei of ``synth.synth_fov`` (what bench.py measures), made by ``FovSegmenter`` for
``--distinct`` fields of view and repeated to ``--fovs`` planes; the grown planes are ``hipops.expand_labels`` of the
same planes by 12 pixels.  The five operators are timed in turns inside one loop, after two warm-up calls each, so all
see the same machine.  Prints one JSON line and writes it to ``--json``:

  census_ms               median milliseconds per call of ``hipops.neighbor_census`` on the planes themselves
  census_expanded_ms      the same on the planes grown by 12 pixels (larger boxes, cells that touch)
  nearest_ms              ``hipops.nearest_labels`` on the planes
  relate_self_ms          ``hipops.relate_labels(labels, k, labels)`` on the same buffers: one pass over every box, two
                          planes read
  relate_self_expanded_ms the same yardstick on the grown planes
  census_over_relate, nearest_over_relate   the ratios of the medians to relate_self_ms
  census_expanded_over_relate               census_expanded_ms over relate_self_expanded_ms: both on the grown planes
  device_route_ms         ``mask.cell_neighbors()`` of one field of view whose plane is on the device (host clock)
  host_route_ms           what it replaces: the label image downloaded, then one numpy pass per cell over its grown box
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

import neighbors_reference as nr  # noqa: E402
from arcadia_microscopy_tools_amd import _hip, hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.masks import SegmentationMask  # noqa: E402
from arcadia_microscopy_tools_amd.segment import FovSegmenter, neighbor_keys  # noqa: E402


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


def host_route(lab: np.ndarray, k: int) -> dict:
    """The columns of ``cell_neighbors`` from a downloaded label image: the reference's ring and census on every cell's
    box grown by one pixel, and its closest-label search on the centroids."""
    H, W = lab.shape
    ys, xs = np.nonzero(lab)
    v = lab[ys, xs]
    y0, x0 = np.full(k + 1, H), np.full(k + 1, W)
    y1, x1 = np.full(k + 1, -1), np.full(k + 1, -1)
    np.minimum.at(y0, v, ys)
    np.minimum.at(x0, v, xs)
    np.maximum.at(y1, v, ys)
    np.maximum.at(x1, v, xs)
    census = np.zeros((k, 4), np.int64)
    for l in range(1, k + 1):
        if y1[l] < 0:
            continue
        crop = lab[max(y0[l] - 1, 0):y1[l] + 2, max(x0[l] - 1, 0):x1[l] + 2]
        vals = nr.neighbor_values(crop, crop, l)
        values, counts = np.unique(vals, return_counts=True)
        census[l - 1] = (len(values), len(vals), nr.ring_mask(crop, l).sum(),
                         values[np.argmax(counts)] if len(values) else 0)
    count = np.bincount(v, minlength=k + 1)[1:k + 1]
    with np.errstate(invalid="ignore", divide="ignore"):  # coordinate sums stay below 2^53: exact in float64
        cy = np.bincount(v, weights=ys, minlength=k + 1)[1:k + 1] / count
        cx = np.bincount(v, weights=xs, minlength=k + 1)[1:k + 1] / count
        who, d2 = nr.closest(cy, cx, count > 0)
        percent = 100.0 * census[:, 1].astype(np.float64) / census[:, 2].astype(np.float64)
    cols = [census[:, 0], census[:, 1], census[:, 2], percent, census[:, 3], who[:, 0], np.sqrt(d2[:, 0]), who[:, 1],
            np.sqrt(d2[:, 1])]
    return dict(zip(neighbor_keys(), cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fovs", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "neighbors.json"))
    a = ap.parse_args()
    ctx = get_context()
    lib = _hip.load_library()
    distinct = max(1, min(a.distinct, a.fovs))
    fovs = np.stack([synth.synth_fov(i, size=a.size) for i in range(distinct)])
    seg = FovSegmenter(distinct, 4, a.size, a.size, ctx=ctx, props=False)
    some = seg.run_c3(ctx.asarray(fovs))
    ncells = seg.ncells.numpy()
    k = int(ncells.max())
    labels = ctx.empty((a.fovs, a.size, a.size), np.int32)
    for i in range(a.fovs):
        j = i % distinct
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, labels[i].ptr, some[j].ptr, some[j].nbytes), "amt_memcpy_d2d")
    grown = hipops.expand_labels(labels, 12)
    ctx.synchronize()
    out = {"fovs": a.fovs, "size": a.size, "distinct": distinct, "reps": a.reps,
           "cells_per_fov": round(float(ncells.mean()), 1), "max_label": k}
    tables = [ctx.empty((a.fovs, k, 1, 4), np.float64) for _ in range(5)]
    names = ("census", "census_expanded", "nearest", "relate_self", "relate_self_expanded")
    times = _event_ms_in_turns(ctx, [
        lambda: hipops.neighbor_census(labels, k, out=tables[0]),
        lambda: hipops.neighbor_census(grown, k, out=tables[1]),
        lambda: hipops.nearest_labels(labels, k, out=tables[2]),
        lambda: hipops.relate_labels(labels, k, labels, out=tables[3]),
        lambda: hipops.relate_labels(grown, k, grown, out=tables[4])], a.reps)
    for name, t in zip(names, times):
        out[f"{name}_ms"] = round(t[0], 4)
        out[f"{name}_ms_min_max"] = [round(t[1], 4), round(t[2], 4)]
    out["census_over_relate"] = round(times[0][0] / times[3][0], 3)
    out["census_expanded_over_relate"] = round(times[1][0] / times[4][0], 3)
    out["nearest_over_relate"] = round(times[2][0] / times[3][0], 3)
    census = tables[0].numpy()
    touched = tables[1].numpy()
    out["mean_neighbors"] = round(float(census[0, :int(ncells[0]), 0, 0].mean()), 3)
    out["mean_neighbors_expanded"] = round(float(touched[0, :int(ncells[0]), 0, 0].mean()), 3)
    again = ctx.empty(tables[1].shape, np.float64)
    hipops.neighbor_census(grown, k, out=again)
    out["repeats_bit_for_bit"] = bool(touched.tobytes() == again.numpy().tobytes())

    # ---- one field of view, as a user sees it ----
    k0 = int(ncells[0])
    nuclei = SegmentationMask._from_device(labels[0], k0, None, None)
    device_ms, host_ms = [], []
    for rep in range(4):
        t0 = time.perf_counter()
        mine = nuclei.cell_neighbors()
        t1 = time.perf_counter()
        other = host_route(nuclei._label_plane()[0].numpy_int64(), k0)
        t2 = time.perf_counter()
        if rep:  # the first round warms both routes
            device_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
    out["device_route_ms"] = round(float(np.median(device_ms)), 3)
    out["host_route_ms"] = round(float(np.median(host_ms)), 3)
    out["routes_equal"] = bool(all(np.array_equal(mine[n], other[n], equal_nan=True) for n in neighbor_keys()))
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
