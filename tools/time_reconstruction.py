"""Time the grey reconstruction operators (device events) against ONE 3 x 3 ``hipops.dilation`` over the same planes, the
unit step: the ratio reads as "equivalent full-plane passes".

    python tools/time_reconstruction.py [--planes 48] [--size 2048] [--json profiles/reconstruction.json]

Two workloads of ``--planes`` planes of ``--size`` squared:

  h-dome    uint16: ``h_reconstruction(a, h, minuend=a)`` (amt_rank_filter op 5 with its minuend) of the DAPI channel of
            ``synth.synth_fov``, h = 3 % of the plane's range;
  h_maxima  float64: ``h_maxima(edt, 2.0)`` of the Euclidean distance transform of the nuclei masks (DAPI > Otsu).

In ONE run the operator and the dilation take turns; each figure is the median of 20 rounds after a warm-up.  The number of
rounds and of host synchronisations comes from the library's diagnostic line (AMT_DEBUG_RECONSTRUCT=1, set here before the
library loads).  For the record: the heap flood of tests/reconstruction_reference.py on one plane, one host core.
Prints one JSON object; ``--json`` also writes it to a file.
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
os.environ["AMT_DEBUG_RECONSTRUCT"] = "1"

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
    """[(rounds, syncs), ...] of the reconstructions inside one call of ``fn``: the library's lines on stderr"""
    ctx.synchronize()
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
            ctx.synchronize()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode()
    return [(int(a), int(b)) for a, b in re.findall(r"amt reconstruct: rounds=(\d+) syncs=(\d+)", text)]


def figures(ctx, name, op, unit, one_plane_host):
    ms = alternate(ctx, {"op": op, "dilation": unit})
    a, d = float(np.median(ms["op"])), float(np.median(ms["dilation"]))
    calls = counted(ctx, op)
    t0 = time.perf_counter()
    one_plane_host()
    host_ms = (time.perf_counter() - t0) * 1e3
    out = {"ms": round(a, 3), "ms_min_max": [round(min(ms["op"]), 3), round(max(ms["op"]), 3)],
           "dilation_3x3_ms": round(d, 4), "equivalent_full_plane_passes": round(a / d, 1),
           "rounds": [c[0] for c in calls], "host_synchronisations": [c[1] for c in calls],
           "heap_reference_one_plane_host_ms": round(host_ms, 1)}
    print(name, json.dumps(out), flush=True)
    return out


def main():
    import reconstruction_reference as rr

    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = get_context()
    out = {"device": ctx.device_name(), "planes": a.planes, "size": a.size, "timed_rounds": ROUNDS,
           "tile_u16": list(hipops.reconstruct_tile(np.uint16)), "tile_f64": list(hipops.reconstruct_tile(np.float64))}
    distinct = [synth.synth_fov(i, size=a.size)[1] for i in range(DISTINCT)]
    host = np.stack([distinct[i % DISTINCT] for i in range(a.planes)])
    img = ctx.asarray(host)
    h = max(1, int(round(0.03 * (int(distinct[0].max()) - int(distinct[0].min())))))
    out["h_dome_h"] = h
    res = ctx.empty(img.shape, np.uint16)
    dil = ctx.empty(img.shape, np.uint16)
    ones = np.ones((3, 3), np.uint8)
    out["h_dome_u16"] = figures(
        ctx, "h-dome", lambda: hipops.h_reconstruction(img, h, "dilation", minuend=img, out=res),
        lambda: hipops.dilation(img, ones, out=dil),
        lambda: distinct[0] - rr.flood(rr.h_seed(distinct[0], h), distinct[0], rr.ONES))
    # the nuclei masks' distance transform
    mask = hipops.greater_than(img, hipops.threshold_otsu(img))
    _, edt = hipops.edt(mask, want_d2=False)
    edt0 = edt[0].numpy()
    del res, dil, mask
    marks = ctx.empty(edt.shape, np.uint8)
    dil64 = ctx.empty(edt.shape, np.float64)
    out["h_maxima_f64"] = figures(
        ctx, "h_maxima", lambda: hipops.h_maxima(edt, 2.0, out=marks), lambda: hipops.dilation(edt, ones, out=dil64),
        lambda: rr.h_extrema(edt0, 2.0, rr.ONES, True))
    out["h_maxima_marked_plane0"] = int(marks[0].numpy(dtype=np.uint8).sum())
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
