"""Time ``hipops.binary_fill_holes`` (device events) against ``hipops.label`` of the inverted mask, which does the same
component analysis plus the raster numbering and writes 4 bytes per pixel where the fill writes 1.

    python tools/time_fill_holes.py [--planes 48] [--size 2048] [--json profiles/fill_holes_bench.json]

Two batches of ``--planes`` planes:

  nuclei        ``tests/golden/props_ext.npz::nuc__labels > 0`` (256 x 256, 22 nuclei) tiled to ``--size``, with seeded
                holes punched into the nuclei (a disc of radius 2-5 at a random pixel of every nucleus copy);
  checkerboard  the complement's worst case for runs: 32 per 64-pixel row.

Per batch, in ONE run, alternating round by round: ``binary_fill_holes(m)`` and ``label(inverted m, connectivity=1)``
(the inverted mask is made beforehand and not timed).  Every figure rests on at least 0.5 s of timed work after the
warm-up.  For the record: scipy on one host core for one plane, and the stage times of ``FovSegmenter.run_c3`` with and
without ``fill_holes``.  Prints one JSON object; ``--json`` also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from arcadia_microscopy_tools_amd import hipops, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.segment import FovSegmenter  # noqa: E402

MIN_TIMED_S = 0.5


def nuclei_plane(size, seed):
    tile = np.load(os.path.join(ROOT, "tests", "golden", "props_ext.npz"), allow_pickle=False)["nuc__labels"]
    reps = -(-size // tile.shape[0])
    labels = np.tile(tile, (reps, reps))[:size, :size]
    mask = (labels > 0).astype(np.uint8)
    rng = np.random.default_rng(seed)
    th, tw = tile.shape
    yy, xx = np.indices((11, 11)) - 5
    ys, xs = np.nonzero(tile > 0)
    by_label = {k: np.flatnonzero(tile[ys, xs] == k) for k in range(1, int(tile.max()) + 1)}
    for ty in range(reps):
        for tx in range(reps):
            for k, idx in by_label.items():
                i = idx[rng.integers(len(idx))]
                r = int(rng.integers(2, 6))
                cy, cx = ty * th + ys[i], tx * tw + xs[i]
                disc = yy * yy + xx * xx <= r * r
                py, px = cy + yy[disc], cx + xx[disc]
                ok = (py >= 0) & (py < size) & (px >= 0) & (px < size)
                mask[py[ok], px[ok]] = 0
    return mask


def checkerboard_plane(size):
    y, x = np.indices((size, size))
    return ((y + x) % 2 == 0).astype(np.uint8)


def alternate(ctx, fns):
    """{name: [ms per round]} of the callables run in turn, round by round, until each has MIN_TIMED_S of timed work."""
    for fn in fns.values():  # warm-up: arena growth, code load
        fn()
        fn()
    ctx.synchronize()
    ms = {k: [] for k in fns}
    while min(sum(v) for v in ms.values()) < MIN_TIMED_S * 1e3 or len(next(iter(ms.values()))) < 5:
        for k, fn in fns.items():
            t = ctx.timer()
            t.start()
            fn()
            t.stop()
            ms[k].append(t.elapsed_ms())
    return ms


def batch_figures(ctx, name, distinct, planes):
    n = len(distinct)
    host = np.stack([distinct[i % n] for i in range(planes)])
    m = ctx.asarray(host)
    inv = ctx.asarray(host == 0)  # a bool array: label takes its leanest route, the truth-value run tables
    del host
    filled = ctx.empty(m.shape, np.uint8)
    labels = ctx.empty(m.shape, np.int32)
    count = ctx.empty((planes,), np.int32)
    ms = alternate(ctx, {"fill": lambda: hipops.binary_fill_holes(m, out=filled),
                         "label": lambda: hipops.label(inv, 1, out=labels, count=count)})
    fill, label = float(np.median(ms["fill"])), float(np.median(ms["label"]))
    px = planes * distinct[0].size
    out = {"planes": planes, "rounds": len(ms["fill"]), "fill_ms": round(fill, 4),
           "fill_ms_min_max": [round(min(ms["fill"]), 4), round(max(ms["fill"]), 4)],
           "label_inverted_ms": round(label, 4),
           "label_inverted_ms_min_max": [round(min(ms["label"]), 4), round(max(ms["label"]), 4)],
           "fill_over_label": round(fill / label, 4), "fill_not_slower_than_label": bool(fill <= label),
           "fill_ns_per_pixel": round(fill * 1e6 / px, 5)}
    # the result itself: one plane against scipy (timed on one host core), and how much there was to fill
    from scipy import ndimage as ndi

    t0 = time.perf_counter()
    want = ndi.binary_fill_holes(distinct[0] != 0)
    out["scipy_one_plane_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    got = filled[0].numpy(dtype=np.uint8)
    out["equals_scipy"] = bool(np.array_equal(got != 0, want))
    out["filled_pixels_plane0"] = int(want.sum()) - int((distinct[0] != 0).sum())
    print(name, json.dumps(out), flush=True)
    return out


def chain_figures(ctx, fovs_n, size):
    fovs = ctx.asarray(np.stack([synth.synth_fov(i, size=size) for i in range(fovs_n)]))
    out = {}
    for fill in (False, True):
        seg = FovSegmenter(fovs_n, 4, size, size, ctx=ctx, props=False, profile=True, fill_holes=fill)
        for _ in range(3):
            seg.run_c3(fovs)
        ctx.synchronize()
        out["fill_holes" if fill else "default"] = {k: round(v, 4) for k, v in seg.times.ms().items()}
        del seg
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--chain-fovs", type=int, default=8)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = get_context()
    out = {"device": ctx.device_name(), "planes": a.planes, "size": a.size, "min_timed_s": MIN_TIMED_S}
    out["nuclei"] = batch_figures(ctx, "nuclei", [nuclei_plane(a.size, s) for s in range(4)], a.planes)
    out["checkerboard"] = batch_figures(ctx, "checkerboard", [checkerboard_plane(a.size)], a.planes)
    out["run_c3_stage_ms"] = chain_figures(ctx, a.chain_fovs, a.size)
    out["run_c3_fovs"] = a.chain_fovs
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
