"""Time the spot operators (device events): ``local_maxima`` at r = 2 on the float64 DoG response against ``hipops.dilation``
with the 5 x 5 all-ones footprint on the same planes, ``mask_list`` and ``spot_measure``.

    python tools/time_spots.py [--planes 48] [--size 2048] [--spots 2000] [--json profiles/spots.json]

``--planes`` planes of ``--size`` squared uint16: the nuclei plane of ``synth.synth_fov`` with ``--spots`` Gaussian spots
(sigma 1.3, amplitude 800) planted per plane.  In ONE run the operators take turns; each figure is the median of 20 rounds
after a warm-up.

What the figures are set against: the dilation is existing code that takes the same 5 x 5 window maximum and moves 16
bytes per pixel (float64 in, float64 out) where ``local_maxima`` moves 9 (float64 in, a byte out); the goal is that
``local_maxima`` is no slower.  Its bytes over its time stand beside the 6.29 TB/s of a streaming copy on an MI355X.  On
the host clock: the whole ``operations.detect_spots`` of one field (upload and download included) against the README's
earlier route to spots, h-dome -> threshold -> ``label``; and the case table of tests/spots_cases.py in process, which
sizes the time limit of the poisoned child in tests/test_gpu_spots.py.  Prints one JSON object; ``--json`` also writes it.
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

from arcadia_microscopy_tools_amd import _hip, hipops, operations, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402

ROUNDS = 20
DISTINCT = 4
COPY_TBS = 6.29  # streaming copy, MI355X


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


def synthetic_field(seed, size, spots):
    """(size, size) uint16: synthetic nuclei with Gaussian spots planted on them"""
    rng = np.random.default_rng(seed)
    field = synth.synth_fov(seed, size=size)[1].astype(np.float64)
    ys, xs = rng.uniform(6, size - 7, spots), rng.uniform(6, size - 7, spots)
    yy, xx = np.mgrid[-5:6, -5:6]
    for cy, cx in zip(ys, xs):
        iy, ix = int(round(cy)), int(round(cx))
        field[iy - 5:iy + 6, ix - 5:ix + 6] += 800.0 * np.exp(-((yy + iy - cy) ** 2 + (xx + ix - cx) ** 2) / (2 * 1.3 ** 2))
    return np.clip(rng.poisson(field), 0, 65535).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=48)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--spots", type=int, default=2000)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = get_context()
    N, S = a.planes, a.size
    out = {"device": ctx.device_name(), "planes": N, "size": S, "planted_spots_per_plane": a.spots, "timed_rounds": ROUNDS,
           "tile": list(hipops.spot_tile())}
    fields = [synthetic_field(i, S, a.spots) for i in range(min(DISTINCT, N))]
    batch = ctx.empty((N, S, S), np.uint16)
    for i, f in enumerate(fields):
        ctx.asarray(f, out=batch[i])
    for n in range(len(fields), N):
        src = batch[n % len(fields)]
        _hip.check(ctx._lib.amt_memcpy_d2d(ctx.handle, batch[n].ptr, src.ptr, src.nbytes), "amt_memcpy_d2d")
    response = hipops.difference_of_gaussians(batch, 1.0, 1.6)
    q = hipops.percentile(response, [25, 50, 75]).numpy()
    thr = ctx.asarray(np.ascontiguousarray(q[:, 1] + 8.0 * (q[:, 2] - q[:, 0]) / 1.349))
    mask = ctx.empty((N, S, S), np.uint8)
    dilated = ctx.empty((N, S, S), np.float64)
    cap = 4 * a.spots
    spots = ctx.empty((N, cap + 1), np.int32)
    table = ctx.empty((N, cap, _hip.SPOT_NCOLS), np.float64)
    hipops.local_maxima(response, 2, thr, 2, out=mask)
    hipops.mask_list(mask, cap, out=spots)
    five = np.ones((5, 5), np.uint8)
    ms = alternate(ctx, {
        "local_maxima_r2_f64": lambda: hipops.local_maxima(response, 2, thr, 2, out=mask),
        "dilation_5x5_f64": lambda: hipops.dilation(response, five, out=dilated),
        "local_maxima_r2_u16": lambda: hipops.local_maxima(batch, 2, 0.0, 2, out=mask),
        "local_maxima_r15_f64": lambda: hipops.local_maxima(response, 15, thr, 2, out=mask),
        "mask_list": lambda: hipops.mask_list(mask, cap, out=spots),
        "spot_measure_k2": lambda: hipops.spot_measure(response, spots, 2, out=table),
    })
    hipops.local_maxima(response, 2, thr, 2, out=mask)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out["ms"] = {k: round(v, 3) for k, v in med.items()}
    out["ms_min_max"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}
    out["spots_found_per_plane"] = [int(v) for v in hipops.mask_list(mask, cap).numpy()[:DISTINCT, 0]]
    moved = response.nbytes + mask.nbytes
    tbs = moved / (med["local_maxima_r2_f64"] * 1e-3) / 1e12
    out["local_maxima_r2_f64"] = {"bytes_moved": moved, "tb_per_s": round(tbs, 3), "share_of_streaming_copy": round(tbs / COPY_TBS, 3),
                                  "over_dilation_5x5_f64": round(med["local_maxima_r2_f64"] / med["dilation_5x5_f64"], 3)}
    # one field through the reference-level call, against the earlier route to spots, on the host clock
    field = fields[0]
    kw = {"sigma": 1.0, "min_distance": 2, "snr": 8.0}
    operations.detect_spots(field, **kw)
    t0 = time.perf_counter()
    found = operations.detect_spots(field, **kw)
    detect_ms = (time.perf_counter() - t0) * 1e3
    d = ctx.asarray(field[None])

    def hdome_route():
        dome = hipops.h_reconstruction(d, 200.0, "dilation", minuend=d)  # image - reconstruction(image - h, image)
        blobs = hipops.greater_than(dome, ctx.asarray(np.array([100.0])))
        _, count = hipops.label(blobs)
        return int(count.numpy()[0])

    hdome_route()
    t0 = time.perf_counter()
    blobs = hdome_route()
    hdome_ms = round((time.perf_counter() - t0) * 1e3, 2)
    out["one_field_host_clock"] = {"detect_spots_ms": round(detect_ms, 2), "spots": int(len(found["row"])),
                                   "hdome_threshold_label_ms": hdome_ms, "hdome_blobs": blobs}
    import spots_cases

    t0 = time.perf_counter()
    res = spots_cases.run(ctx)
    out["table_in_process_s"] = round(time.perf_counter() - t0, 2)
    out["table_all_equal"] = all(v["equal"] for v in res.values())
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
