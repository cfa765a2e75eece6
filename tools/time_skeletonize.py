"""Time ``hipops.skeletonize`` (device events) against ONE 3 x 3 ``hipops.binary_erosion`` over the same planes, the cost of
one pass per launch: the quotient "skeletonize time / (sub-iterations x erosion time)" shows whether running the
sub-iterations in LDS pays against one launch per sub-iteration (below 1: it does).

    python tools/time_skeletonize.py [--planes 48] [--size 2048] [--json profiles/skeletonize.json]

Two workloads of ``--planes`` planes of ``--size`` squared: the nuclei masks (DAPI > Otsu) of ``synth.synth_fov``, and the
same masks after ``binary_fill_holes``.  In ONE run the operators take turns; each figure is the median of 20 rounds after
a warm-up.  Iterations (of the plane that needed most), launches and host synchronisations come from the library's
diagnostic line (AMT_DEBUG_SKELETONIZE=1).  Side figures: ``neighbor_classes`` of the skeletons alone, and the numpy rule
of tests/skeleton_reference.py on one plane, one host core.  Prints one JSON object; ``--json`` also writes it to a file.
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

from arcadia_microscopy_tools_amd import hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402

ROUNDS = 20
DISTINCT = 4


def alternate(ctx, fns):
    for fn in fns.values():
        fn()
        fn()
    ctx.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t = ctx.timer()
            t.start()
            fn()
            t.stop()
            ms[k].append(t.elapsed_ms())
    return ms


def counted(ctx, fn):
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
    m = re.search(r"amt skeletonize: iterations=(\d+) launches=(\d+) syncs=(\d+)", text)
    return tuple(int(g) for g in m.groups())


def figures(ctx, name, mask, plane0):
    import skeleton_reference as ref

    skel = ctx.empty(mask.shape, np.uint8)
    ero = ctx.empty(mask.shape, np.uint8)
    cls = ctx.empty(mask.shape, np.uint8)
    ones = np.ones((3, 3), np.uint8)
    ms = alternate(ctx, {"skeletonize": lambda: hipops.skeletonize(mask, out=skel),
                         "erosion": lambda: hipops.binary_erosion(mask, ones, out=ero),
                         "classes": lambda: hipops.neighbor_classes(skel, 2, out=cls)})
    s, e, c = (float(np.median(ms[k])) for k in ("skeletonize", "erosion", "classes"))
    iterations, launches, syncs = counted(ctx, lambda: hipops.skeletonize(mask, out=skel))
    t0 = time.perf_counter()
    want, host_iterations = ref.skeletonize(plane0)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = skel[0].numpy(dtype=np.uint8)
    out = {"skeletonize_ms": round(s, 3), "skeletonize_ms_min_max": [round(min(ms["skeletonize"]), 3), round(max(ms["skeletonize"]), 3)],
           "iterations": iterations, "sub_iterations": 2 * iterations, "launches": launches, "host_synchronisations": syncs,
           "erosion_3x3_ms": round(e, 4), "quotient_vs_one_pass_per_sub_iteration": round(s / (2 * iterations * e), 3),
           "neighbor_classes_ms": round(c, 4), "numpy_rule_one_plane_host_ms": round(host_ms, 1),
           "plane0_iterations": host_iterations, "plane0_equals_numpy_rule": bool(np.array_equal(got, want)),
           "plane0_pixels": [int(plane0.sum()), int(got.sum())]}
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = get_context()
    out = {"device": ctx.device_name(), "planes": a.planes, "size": a.size, "timed_rounds": ROUNDS,
           "skeleton_block": list(hipops.skeleton_block())}
    distinct = [synth.synth_fov(i, size=a.size)[1] for i in range(DISTINCT)]
    img = ctx.asarray(np.stack([distinct[i % DISTINCT] for i in range(a.planes)]))
    mask = hipops.greater_than(img, hipops.threshold_otsu(img))
    del img
    out["nuclei_masks"] = figures(ctx, "nuclei masks", mask, mask[0].numpy(dtype=np.uint8))
    filled = hipops.binary_fill_holes(mask)
    del mask
    out["filled_masks"] = figures(ctx, "filled masks", filled, filled[0].numpy(dtype=np.uint8))
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
