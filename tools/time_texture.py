"""Time ``hipops.texture`` (per-cell Haralick texture of every channel) on nuclei label planes with four uint16 channels
(device events), with ``hipops.robust_intensity`` on the same buffers as the yardstick, and the host route it replaces.

    python tools/time_texture.py [--fovs 48] [--size 2048] [--distinct 8] [--reps 20] [--json profiles/texture.json]

The label planes are the config-3 nuclei of ``synth.synth_fov`` (what bench.py measures), made by ``FovSegmenter`` for
``--distinct`` fields of view and repeated to ``--fovs`` planes; the intensity stacks are the four channels of the same
fields of view.  The operators are timed in turns inside one loop, after two warm-up calls each, so all see the same
machine.  Prints one JSON line and writes it to ``--json``:

  texture_ms              median milliseconds per call of ``hipops.texture`` (all planes, four channels, levels 8,
                          distance 1, default ranges: the extrema of every image are found inside the call)
  texture_given_ranges_ms the same with the ranges handed over on the device (the kernel and the box pass alone)
  robust_ms               ``hipops.robust_intensity`` on the same buffers
  texture_over_robust     the ratio of the medians (texture_ms / robust_ms)
  texture_l64_ms, texture_d3_ms   levels 64 and distance 3, default ranges
  device_route_ms         ``cell_texture()`` of one field of view whose label plane is on the device (host clock; the
                          four channel images are uploaded inside it)
  host_route_ms           what it replaces: the label image downloaded, the reference per cell on the crop to its box
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

import texture_cases as tc  # noqa: E402
import texture_reference as tr  # noqa: E402
from arcadia_microscopy_tools_amd import _hip, channels, hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.masks import SegmentationMask  # noqa: E402
from arcadia_microscopy_tools_amd.segment import DEFAULT_CHANNELS, FovSegmenter, texture_keys  # noqa: E402


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


def host_route(label_image, images, k):
    """(k, C, 4, 13): the reference per cell and channel on the crop to the cell's bounding box"""
    from scipy import ndimage as ndi

    stack = np.stack(images)
    rng = tr.default_ranges(stack)
    out = np.full((k, len(images), 4, len(tr.COLS)), np.nan)
    for l, box in enumerate(ndi.find_objects(label_image, max_label=k)):
        if box is None:
            continue
        member = label_image[box] == l + 1
        for c in range(len(images)):
            G = tr.glcm(member, tr.quantise(stack[c][box], rng[c, 0], rng[c, 1], 8), 8, 1)
            for a in range(4):
                out[l, c, a] = tr.features(G[a])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fovs", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "texture.json"))
    ap.add_argument("--trace", action="store_true",
                    help="only hipops.texture (levels 8, distance 1, default ranges) and hipops.robust_intensity on the batch: "
                         "under a kernel trace every texture_kernel dispatch is then that one configuration")
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
    ctx.synchronize()
    out = {"fovs": a.fovs, "size": a.size, "channels": C, "distinct": distinct, "reps": a.reps,
           "cells_per_fov": round(float(ncells.mean()), 1), "max_label": k, "levels": 8, "distance": 1}
    ttable = ctx.empty((a.fovs, k, C, 4, _hip.TEX_NCOLS), np.float64)
    qtable = ctx.empty((a.fovs, k, C, 4), np.float64)
    ranges = ctx.asarray(np.stack([tr.default_ranges(fovs[i % distinct]) for i in range(a.fovs)]))
    if a.trace:
        timed = _event_ms_in_turns(ctx, [lambda: hipops.texture(labels, stacks, k, out=ttable),
                                         lambda: hipops.robust_intensity(labels, stacks, k, out=qtable)], a.reps)
        out.update(texture_ms=round(timed[0][0], 4), robust_ms=round(timed[1][0], 4), trace=True)
        print(json.dumps(out))
        return
    timed = _event_ms_in_turns(ctx, [
        lambda: hipops.texture(labels, stacks, k, out=ttable),
        lambda: hipops.robust_intensity(labels, stacks, k, out=qtable),
        lambda: hipops.texture(labels, stacks, k, ranges=ranges, out=ttable),
        lambda: hipops.texture(labels, stacks, k, levels=64, out=ttable),
        lambda: hipops.texture(labels, stacks, k, distance=3, out=ttable)], a.reps)
    for name, t in zip(("texture", "robust", "texture_given_ranges", "texture_l64", "texture_d3"), timed):
        out[f"{name}_ms"] = round(t[0], 4)
        out[f"{name}_ms_min_max"] = [round(t[1], 4), round(t[2], 4)]
    out["texture_over_robust"] = round(timed[0][0] / timed[1][0], 3)
    out["goal_ratio"] = 1.5
    first = hipops.texture(labels, stacks, k).numpy()
    again = hipops.texture(labels, stacks, k, ranges=ranges).numpy()
    out["repeats_bit_for_bit"] = bool(first.tobytes() == again.tobytes())

    # ---- one field of view, as a user sees it ----
    k0 = int(ncells[0])
    names = [channels.CHANNELS[n] for n in DEFAULT_CHANNELS[:C]]
    images = {ch: fovs[0][c] for c, ch in enumerate(names)}
    mask = SegmentationMask._from_device(labels[0], k0, None, None, intensity_image_dict=images)
    keys = texture_keys(names)
    device_ms, host_ms = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        mine = mask.cell_texture()
        t1 = time.perf_counter()
        lab = mask._label_plane()[0].numpy_int64()
        other = host_route(lab, list(images.values()), k0)
        t2 = time.perf_counter()
        if rep:  # the first round warms both routes
            device_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
    out["device_route_ms"] = round(float(np.median(device_ms)), 3)
    out["host_route_ms"] = round(float(np.median(host_ms)), 3)
    table = np.stack([mine[key] for key in keys], axis=1).reshape(k0, C, 4, len(tr.COLS))
    none = np.zeros((0,), np.uint32)
    ok, err = tc.compare(table, none, other, none)
    out["routes_agree"] = bool(ok)
    out["largest_abs_error_per_column"] = {name: float(e) for name, e in zip(tr.COLS, err)}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
