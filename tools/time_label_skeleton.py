"""Time ``hipops.label_skeleton`` and ``hipops.label_census`` on nuclei label planes (device events), with the binary
``hipops.skeletonize(labels != 0)`` of the same planes as the yardstick, and the host route they replace.

    python tools/time_label_skeleton.py [--fovs 48] [--size 2048] [--distinct 8] [--reps 20] [--json profiles/label_skeleton.json]

The label planes are the config-3 nuclei of ``synth.synth_fov`` (what bench.py measures), made by ``FovSegmenter`` for
``--distinct`` fields of view and repeated to ``--fovs`` planes: watershed cells, which touch.  The four operators are
timed in turns inside one loop, after two warm-up calls each, so all see the same machine; every figure is the median
of ``--reps`` rounds.  Prints one JSON object and writes it to ``--json``:

  label_skeleton_ms        ``hipops.label_skeleton`` of the planes
  skeletonize_ms           the yardstick: ``hipops.skeletonize`` of the masks ``labels != 0`` of the same planes
  label_over_binary        the ratio of the two medians; the feature was written expecting at most about 3
  label_census_ms          ``hipops.label_census`` of the label skeletons
  neighbor_classes_ms      ``hipops.neighbor_classes`` of the binary skeletons, the per-pixel pass it is the per-cell form of
  iterations, launches, host_synchronisations   of both thinnings, from the library's line (AMT_DEBUG_SKELETONIZE=1)
  device_route_ms          ``mask.cell_skeleton()`` of one field of view whose plane is on the device (host clock)
  host_route_ms            what it replaces: the label image downloaded, then the numpy rule and the numpy census per
                           cell on its box
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import label_skeleton_reference as ref  # noqa: E402
from arcadia_microscopy_tools_amd import _hip, hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.masks import SegmentationMask  # noqa: E402
from arcadia_microscopy_tools_amd.segment import FovSegmenter, skeleton_keys  # noqa: E402


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


def counted(ctx, fn, name):
    """(iterations, launches, syncs) of one call of ``fn``: the library's line on stderr"""
    ctx.synchronize()
    sys.stderr.flush()
    os.environ["AMT_DEBUG_SKELETONIZE"] = "1"
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
            ctx.synchronize()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            del os.environ["AMT_DEBUG_SKELETONIZE"]
        tmp.seek(0)
        text = tmp.read().decode()
    m = re.search(rf"amt {name}: iterations=(\d+) launches=(\d+) syncs=(\d+)", text)
    return dict(zip(("iterations", "launches", "host_synchronisations"), (int(g) for g in m.groups())))


def host_route(lab: np.ndarray, k: int) -> dict:
    """The columns of ``cell_skeleton`` from a downloaded label image: every cell thinned alone on its box by the numpy
    rule, and the numpy census of that skeleton."""
    t = np.zeros((k, 7), np.int64)
    ys, xs = np.nonzero(lab)
    order = np.argsort(lab[ys, xs], kind="stable")
    ys, xs, ls = ys[order], xs[order], lab[ys, xs][order]
    starts = np.searchsorted(ls, np.arange(1, k + 2))
    for l in range(1, k + 1):
        a, b = starts[l - 1], starts[l]
        if a == b:
            continue
        box = (slice(ys[a:b].min(), ys[a:b].max() + 1), slice(xs[a:b].min(), xs[a:b].max() + 1))
        skel = ref.binary.skeletonize(lab[box] == l)[0]
        t[l - 1] = ref.census(skel.astype(np.int32), 1)[0]
    cols = [t[:, i] for i in range(5)] + [t[:, 5].astype(np.float64) + np.sqrt(2.0) * t[:, 6].astype(np.float64)]
    return dict(zip(skeleton_keys(), cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fovs", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "label_skeleton.json"))
    a = ap.parse_args()
    ctx = get_context()
    lib = _hip.load_library()
    distinct = max(1, min(a.distinct, a.fovs))
    fovs = np.stack([synth.synth_fov(i, size=a.size) for i in range(distinct)])
    seg = FovSegmenter(distinct, 4, a.size, a.size, ctx=ctx, props=False)
    some = seg.run_c3(ctx.asarray(fovs))
    ncells = seg.ncells.numpy()
    k = int(ncells.max())
    some_masks = ctx.asarray(some.numpy() != 0)
    labels = ctx.empty((a.fovs, a.size, a.size), np.int32)
    masks = ctx.empty((a.fovs, a.size, a.size), np.uint8)
    for i in range(a.fovs):
        j = i % distinct
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, labels[i].ptr, some[j].ptr, some[j].nbytes), "amt_memcpy_d2d")
        _hip.check(lib.amt_memcpy_d2d(ctx.handle, masks[i].ptr, some_masks[j].ptr, some_masks[j].nbytes), "amt_memcpy_d2d")
    ctx.synchronize()
    out = {"device": ctx.device_name(), "fovs": a.fovs, "size": a.size, "distinct": distinct, "reps": a.reps,
           "cells_per_fov": round(float(ncells.mean()), 1), "max_label": k,
           "label_skeleton_block": list(hipops.label_skeleton_block())}
    lskel = ctx.empty(labels.shape, np.int32)
    bskel = ctx.empty(masks.shape, np.uint8)
    table = ctx.empty((a.fovs, k, _hip.LCEN_NCOLS), np.int32)
    classes = ctx.empty(masks.shape, np.uint8)
    names = ("label_skeleton", "skeletonize", "label_census", "neighbor_classes")
    times = _event_ms_in_turns(ctx, [
        lambda: hipops.label_skeleton(labels, out=lskel),
        lambda: hipops.skeletonize(masks, out=bskel),
        lambda: hipops.label_census(lskel, k, out=table),
        lambda: hipops.neighbor_classes(bskel, 2, out=classes)], a.reps)
    for name, t in zip(names, times):
        out[f"{name}_ms"] = round(t[0], 4)
        out[f"{name}_ms_min_max"] = [round(t[1], 4), round(t[2], 4)]
    out["label_over_binary"] = round(times[0][0] / times[1][0], 3)
    out["expected_at_most"] = 3.0
    out["goal_met"] = bool(times[0][0] / times[1][0] <= 3.0)
    out["label_skeleton_counts"] = counted(ctx, lambda: hipops.label_skeleton(labels, out=lskel), "label_skeleton")
    out["skeletonize_counts"] = counted(ctx, lambda: hipops.skeletonize(masks, out=bskel), "skeletonize")
    first = table.numpy()
    again = ctx.empty(table.shape, np.int32)
    hipops.label_census(hipops.label_skeleton(labels), k, out=again)
    out["repeats_bit_for_bit"] = bool(first.tobytes() == again.numpy().tobytes())
    skel0 = lskel[0].numpy()
    out["plane0_pixels"] = {"labels": int(np.count_nonzero(some[0].numpy())), "label_skeleton": int(np.count_nonzero(skel0)),
                            "binary_skeleton": int(np.count_nonzero(bskel[0].numpy(dtype=np.uint8)))}

    # ---- one field of view, as a user sees it ----
    k0 = int(ncells[0])
    nuclei = SegmentationMask._from_device(labels[0], k0, None, None)
    device_ms = []
    for rep in range(4):
        t0 = time.perf_counter()
        mine = nuclei.cell_skeleton()
        device_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    other = host_route(nuclei._label_plane()[0].numpy_int64(), k0)
    host_ms = (time.perf_counter() - t0) * 1e3
    out["device_route_ms"] = round(float(np.median(device_ms[1:])), 3)
    out["host_route_ms"] = round(host_ms, 1)
    out["routes_agree"] = bool(all(mine[key].tobytes() == other[key].tobytes() for key in skeleton_keys()))
    out["mean_skeleton_length"] = round(float(mine["skeleton_length"].mean()), 3)
    out["mean_skeleton_ends"] = round(float(mine["skeleton_ends"].mean()), 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
