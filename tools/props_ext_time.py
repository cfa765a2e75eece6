"""Time ``hipops.regionprops_ext`` against ``hipops.regionprops`` on the bench's label planes (device events).

    python tools/props_ext_time.py [--fovs 48] [--size 2048] [--reps 10]

The label planes are the config-3 nuclei of ``synth.synth_fov`` (what bench.py measures), made once by
``FovSegmenter``.  Prints one JSON line: milliseconds per call (median of --reps) for the existing morphology table,
the extended morphology set, and the weighted centroids of the 4 uint16 channels.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arcadia_microscopy_tools_amd import _hip, hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.segment import FovSegmenter  # noqa: E402

MORPH = [n for n in _hip.RPX_BITS if _hip.RPX_BITS[n] != _hip.RPX_WEIGHTED]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fovs", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    ctx = get_context()
    fovs = np.stack([synth.synth_fov(i, size=a.size) for i in range(a.fovs)])
    d = ctx.asarray(fovs)
    seg = FovSegmenter(a.fovs, 4, a.size, a.size, ctx=ctx, props=False)
    labels = seg.run_c3(d)
    K = seg.max_cells
    ncells = seg.ncells.numpy()
    table = ctx.empty((a.fovs, K, _hip.RP_NCOLS), np.float64)
    xt = ctx.empty((a.fovs, K, _hip.RPX_NCOLS), np.float64)
    wt = ctx.empty((a.fovs, K, 4, 4), np.float64)
    runs = {
        "regionprops": lambda: hipops.regionprops(labels, K, out=table),
        "regionprops_ext_morphology": lambda: hipops.regionprops_ext(labels, K, MORPH, out=xt),
        "regionprops_ext_weighted": lambda: hipops.regionprops_ext(labels, K, ["centroid_weighted"], intensity=d,
                                                                   wout=wt),
    }
    out = {"fovs": a.fovs, "size": a.size, "cells": int(ncells.sum()), "max_cells": K}
    for name, fn in runs.items():
        fn()  # warm-up: arena growth, code load
        ctx.synchronize()
        ms = []
        for _ in range(a.reps):
            t = ctx.timer()
            t.start()
            fn()
            t.stop()
            ms.append(t.elapsed_ms())
        out[name + "_ms"] = round(float(np.median(ms)), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
