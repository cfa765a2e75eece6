"""Time ``hipops.remove_small_objects`` / ``remove_small_holes`` (device events, median of 10) for both connectivities,
next to ``hipops.binary_fill_holes`` on the same planes.

    python tools/time_area_filters.py [--planes 48] [--size 2048] [--min-size 64] [--json profiles/area_filters_bench.json]

The planes are the chain's synthetic nuclei mask: ``FovSegmenter.mask_chain`` (Gaussian -> Otsu -> opening -> closing) on
the DAPI channel of four ``synth.synth_fov`` fields of ``--size``, repeated to ``--planes`` planes.  The operators run in
turn, round by round, after a warm-up of two calls each.  ``fill_over_*`` in the output compares with this build's own
``binary_fill_holes``; for a comparison with the build before the area filters, time that build with
tools/time_fill_holes.py.  Prints one JSON object; ``--json`` also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from arcadia_microscopy_tools_amd import hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.segment import FovSegmenter  # noqa: E402

ROUNDS = 10
DISTINCT = 4


def nuclei_masks(ctx, size):
    """The mask chain's result for DISTINCT synthetic fields, as host uint8 planes."""
    fovs = ctx.asarray(np.stack([synth.synth_fov(i, size=size) for i in range(DISTINCT)]))
    seg = FovSegmenter(DISTINCT, 4, size, size, ctx=ctx, props=False)
    return seg.mask_chain(fovs).numpy(dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--min-size", type=int, default=64)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = get_context()
    distinct = nuclei_masks(ctx, a.size)
    m = ctx.asarray(np.stack([distinct[i % DISTINCT] for i in range(a.planes)]))
    out_d = ctx.empty(m.shape, np.uint8)
    fns = {"fill_holes": lambda: hipops.binary_fill_holes(m, out=out_d)}
    for conn in (1, 2):
        fns[f"remove_small_objects_c{conn}"] = lambda c=conn: hipops.remove_small_objects(m, a.min_size, c, out=out_d)
        fns[f"remove_small_holes_c{conn}"] = lambda c=conn: hipops.remove_small_holes(m, a.min_size, c, out=out_d)
    for fn in fns.values():  # warm-up: arena growth, code load
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
    res = {"device": ctx.device_name(), "planes": a.planes, "size": a.size, "min_size": a.min_size, "rounds": ROUNDS,
           "foreground_fraction": round(float(distinct.mean()), 4)}
    fill = float(np.median(ms["fill_holes"]))
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"ms": round(med, 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)],
                  "ns_per_pixel": round(med * 1e6 / (a.planes * a.size * a.size), 5),
                  "over_fill_holes_of_this_build": round(med / fill, 4)}
    # the result itself: plane 0 against scipy.ndimage.label + np.bincount
    from scipy import ndimage as ndi

    lab, _ = ndi.label(distinct[0] != 0)
    want = (distinct[0] != 0) & (np.bincount(lab.ravel())[lab] >= a.min_size)
    got = hipops.remove_small_objects(m, a.min_size, 1, out=out_d)[0].numpy(dtype=np.uint8)
    res["objects_equal_scipy"] = bool(np.array_equal(got != 0, want))
    res["objects_removed_pixels_plane0"] = int((distinct[0] != 0).sum()) - int(want.sum())
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
