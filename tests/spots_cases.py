"""The case table of the spot operators (local_maxima, mask_list, spot_measure, take_at): the smallest planes on which the
kernels can still go wrong.  The local-maximum kernel owns 64 x 64 tiles (``hipops.spot_tile()``): planes below, at and
past one tile, odd unaligned planes (65 x 129, 70 x 131), planes smaller than the window, every radius class (1, 2 -- the
unrolled instances --, 5 and 15), both dtypes, and content chosen to break the tie rule: values in 0..5, constant planes
and rows, 65535 plateaus, -0.0 beside +0.0, equal peaks exactly r and r + 1 apart across the tile seam, peaks in every
corner and on every edge under three border widths, per-plane thresholds, a threshold equal to a peak.

A case is a dict with "name" and "op" ("maxima", "list", "measure", "take") and the op's operands; ``reference(case)`` gives
what tests/spots_reference.py makes of it, computed once per process and left unchanged; ``mismatch(case, got, want)``
states how a result may differ (only the float64 sums of spot_measure may, by the bound the reference computes).

``python -m tests.spots_cases --json PATH`` runs the table and writes a digest per result, whether it matched the
reference, and -- with AMT_DEBUG_POISON=1 -- what ``Context.scratch_check()`` found after every call.  Not collected by
pytest (no test_ prefix)."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import poison_child  # noqa: E402
import spots_reference as ref  # noqa: E402
from arcadia_microscopy_tools_amd import hipops  # noqa: E402
from poison_child import digest  # noqa: E402

TH, TW = hipops.spot_tile()
SHAPES = ((1, 1), (1, 9), (5, 3), (37, 53), (64, 64), (65, 129), (70, 131))
RADII = (1, 2, 5, 15)
WIDTHS = (1, 63, 64, 65, 131)

_CACHE: dict = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def tied_plane(shape, dtype, seed):
    """values in 0..5: nearly everything ties"""
    return np.random.default_rng(seed).integers(0, 6, size=shape).astype(dtype)


def seam_pairs(r):
    """six planes of 80 x 81: two equal peaks, the first at (63, 63) -- the last pixel of the first tile --, the second
    d = r and d = r + 1 away horizontally, vertically and diagonally, i.e. across the seam at 64"""
    planes = np.zeros((6, 80, 81), np.uint16)
    for i, (d, (sy, sx)) in enumerate((d, s) for d in (r, r + 1) for s in ((0, 1), (1, 0), (1, 1))):
        planes[i, 63, 63] = 500
        planes[i, 63 + sy * d, 63 + sx * d] = 500
    return planes


def corner_plane(shape=(37, 53)):
    H, W = shape
    a = np.zeros(shape, np.uint16)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1),
                 (H // 2, W // 2)):
        a[y, x] = 5
    return a


def signed_zero_plane():
    """negative float64 values, and a 2 x 2 patch of +-0.0 above them all: one plateau, not four peaks"""
    a = -1.0 - np.random.default_rng(7).random((37, 53))
    a[10:12, 20:22] = [[0.0, -0.0], [-0.0, 0.0]]
    a[30, 40] = -0.0
    return a


def plateau_plane():
    a = np.random.default_rng(8).integers(0, 60000, size=(70, 131)).astype(np.uint16)
    for y, x, h, w in ((0, 0, 3, 4), (60, 60, 8, 8), (30, 120, 5, 11), (67, 10, 3, 30)):
        a[y:y + h, x:x + w] = 65535
    return a


def blob_plane(shape, dtype, seed, n=12):
    """smooth bumps on noise: true maxima with concave neighbourhoods, for the sub-pixel fit"""
    rng = np.random.default_rng(seed)
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    a = rng.random(shape) * 20 + 100
    for _ in range(n):
        cy, cx = rng.random() * (H - 1), rng.random() * (W - 1)
        a += 900 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 1.4 ** 2))
    return np.round(a).astype(np.uint16) if np.dtype(dtype) == np.uint16 else (a - 500.0)


def hand_list(shape, points, capacity, count=None):
    W = shape[1]
    lst = np.full(capacity + 1, -1, np.int32)
    idx = sorted(y * W + x for y, x in points)
    lst[0] = len(idx) if count is None else count
    lst[1:1 + len(idx)] = idx
    return lst


def cases():
    def make():
        out = []
        seed = 0
        for shape in SHAPES:
            for r in RADII:
                for dtype in (np.uint16, np.float64):
                    seed += 1
                    out.append({"name": f"maxima ties {shape[0]} x {shape[1]} r {r} {np.dtype(dtype).name}", "op": "maxima",
                                "a": tied_plane((1,) + shape, dtype, seed), "r": r, "b": 0, "t": 0.0})
        for b in (0, 1):
            out.append({"name": f"maxima constant b {b}", "op": "maxima", "a": np.full((1, 37, 53), 7, np.uint16), "r": 2,
                        "b": b, "t": 0.0})
        row = np.zeros((1, 37, 53), np.uint16)
        row[0, 3] = 9
        for r in (2, 5):
            out.append({"name": f"maxima constant row r {r}", "op": "maxima", "a": row, "r": r, "b": 0, "t": 0.0})
        out.append({"name": "maxima 65535 plateaus", "op": "maxima", "a": plateau_plane()[None], "r": 2, "b": 0, "t": 65534.0})
        out.append({"name": "maxima signed zeros", "op": "maxima", "a": signed_zero_plane()[None], "r": 2, "b": 0, "t": -10.0})
        for r in RADII:
            out.append({"name": f"maxima seam pairs r {r}", "op": "maxima", "a": seam_pairs(r), "r": r, "b": 0, "t": 0.0})
        for b in (0, 1, 2):
            out.append({"name": f"maxima corners b {b}", "op": "maxima", "a": corner_plane()[None], "r": 2, "b": b, "t": 0.0})
        batch = np.random.default_rng(50).integers(0, 1001, size=(3, 70, 131)).astype(np.uint16)
        out.append({"name": "maxima per-plane thresholds", "op": "maxima", "a": batch, "r": 2, "b": 0,
                    "t": np.array([100.0, 990.0, 999.5])})
        out.append({"name": "maxima per-plane thresholds float64", "op": "maxima", "a": batch / 7.0, "r": 1, "b": 3,
                    "t": np.array([100.0, 142.0, -1.0])})
        strict = np.zeros((1, 37, 53), np.uint16)
        strict[0, 5, 5], strict[0, 20, 30] = 10, 20
        out.append({"name": "maxima threshold equals a peak", "op": "maxima", "a": strict, "r": 2, "b": 0, "t": 10.0})
        out.append({"name": "maxima threshold equals a peak float64", "op": "maxima", "a": strict * 0.1, "r": 2, "b": 0,
                    "t": float(np.float64(10) * 0.1)})
        # mask lists
        for W in WIDTHS:
            mask = (np.random.default_rng(60 + W).random((1, 7, W)) < 0.3).astype(np.uint8) * 3
            n = int(np.count_nonzero(mask))
            for cap in sorted({max(n, 1), max(n - 1, 1), n + 50}):
                out.append({"name": f"list 7 x {W} capacity {cap} of {n}", "op": "list", "mask": mask, "capacity": cap})
        for fill in (0, 1):
            out.append({"name": f"list {'full' if fill else 'empty'} 70 x 131", "op": "list",
                        "mask": np.full((1, 70, 131), fill, np.uint8), "capacity": None})
        masks = (np.random.default_rng(61).random((3, 70, 131)) < np.array([0.01, 0.5, 0.0003])[:, None, None]).astype(np.uint8)
        out.append({"name": "list batch of three", "op": "list", "mask": masks, "capacity": 600})
        tall = (np.random.default_rng(62).random((1, 5000, 3)) < 0.2).astype(np.uint8)  # rows past the scan's first chunk
        out.append({"name": "list 5000 x 3", "op": "list", "mask": tall, "capacity": None})
        # spot measure
        for dtype in (np.uint16, np.float64):
            a = blob_plane((70, 131), dtype, 70)
            H, W = a.shape
            name = np.dtype(dtype).name
            peaks = np.flatnonzero(ref.local_maxima(a, 2, float(np.median(a)), 0))
            lst = np.full(len(peaks) + 4, -1, np.int32)
            lst[0] = len(peaks)
            lst[1:1 + len(peaks)] = peaks
            for k in (0, 2, 15):
                out.append({"name": f"measure maxima {name} k {k}", "op": "measure", "a": a[None], "spots": lst[None], "k": k})
            edge = hand_list(a.shape, ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 60), (H - 1, 61), (33, 0), (34, W - 1),
                                       (1, 1), (35, 64), (63, 63), (64, 64)), 20)
            for k in (0, 2, 15):
                out.append({"name": f"measure corners and edges {name} k {k}", "op": "measure", "a": a[None], "spots": edge[None],
                            "k": k})
            valley = int(np.argmin(a[1:-1, 1:-1])) // (W - 2) + 1, int(np.argmin(a[1:-1, 1:-1])) % (W - 2) + 1
            out.append({"name": f"measure a minimum {name}", "op": "measure", "a": a[None],
                        "spots": hand_list(a.shape, (valley,), 3)[None], "k": 1})
            # a count past the capacity, a -1 entry in the middle, an index outside the plane
            odd = hand_list(a.shape, ((5, 5), (6, 9), (40, 100)), 3, count=9)
            holes = hand_list(a.shape, ((5, 5), (6, 9), (40, 100)), 5)
            holes[2] = -1
            holes[3] = H * W
            out.append({"name": f"measure overfull and holes {name}", "op": "measure", "a": np.stack([a, a]),
                        "spots": np.stack([np.pad(odd, (0, 2), constant_values=-1), holes]), "k": 2})
        small = tied_plane((1, 5, 3), np.uint16, 71)
        out.append({"name": "measure 5 x 3 k 15", "op": "measure", "a": small, "spots": ref.mask_list(np.ones((5, 3)), 15)[None],
                    "k": 15})
        one = np.full((1, 1, 1), 9, np.uint16)
        out.append({"name": "measure 1 x 1", "op": "measure", "a": one, "spots": np.array([[1, 0]], np.int32), "k": 0})
        # take at
        labels = np.random.default_rng(80).integers(-5, 2**31 - 1, size=(2, 37, 53)).astype(np.int32)
        pts = np.stack([ref.mask_list(np.random.default_rng(81 + i).random((37, 53)) < 0.02, 60) for i in range(2)])
        out.append({"name": "take int32 labels", "op": "take", "a": labels, "spots": pts})
        for dtype in (np.uint16, np.uint8, np.float64):
            out.append({"name": f"take {np.dtype(dtype).name}", "op": "take", "a": (labels % 251).astype(dtype), "spots": pts})
        return out
    return _memo("cases", make)


def case(name):
    return [c for c in cases() if c["name"] == name][0]


def _threshold_of(c, n):
    return float(c["t"][n]) if isinstance(c["t"], np.ndarray) else float(c["t"])


def reference(c):
    """{result name: array} of a case ("bound" of a measure case is the tolerance, not a result of the device)"""
    def make():
        if c["op"] == "maxima":
            return {"mask": np.stack([ref.local_maxima(p, c["r"], _threshold_of(c, n), c["b"]) for n, p in enumerate(c["a"])])}
        if c["op"] == "list":
            return {"list": np.stack([ref.mask_list(m, c["capacity"]) for m in c["mask"]])}
        if c["op"] == "measure":
            both = [ref.spot_measure(p, s, c["k"], bounds=True) for p, s in zip(c["a"], c["spots"])]
            return {"table": np.stack([t for t, _ in both]), "bound": np.stack([b for _, b in both])}
        return {"taken": np.stack([ref.take_at(p, s) for p, s in zip(c["a"], c["spots"])])}
    return _memo(("reference", c["name"]), make)


def run_case(ctx, c, check=None):
    """{result name: array} of a case on the device"""
    check = check or (lambda: None)
    if c["op"] == "maxima":
        t = ctx.asarray(c["t"]) if isinstance(c["t"], np.ndarray) else c["t"]
        out = {"mask": hipops.local_maxima(ctx.asarray(c["a"]), c["r"], t, c["b"]).numpy().astype(np.uint8)}
    elif c["op"] == "list":
        out = {"list": hipops.mask_list(ctx.asarray(c["mask"]), c["capacity"]).numpy()}
    elif c["op"] == "measure":
        out = {"table": hipops.spot_measure(ctx.asarray(c["a"]), ctx.asarray(c["spots"]), c["k"]).numpy()}
    else:
        out = {"taken": hipops.take_at(ctx.asarray(c["a"]), ctx.asarray(c["spots"])).numpy()}
    check()
    return out


def mismatch(c, got, want):
    """None, or what is wrong.  Everything is compared byte for byte but the two float64 sums of a spot_measure table on
    float64 planes, which may differ from the reference's by at most its "bound" (two sums of the same n terms in
    different fixed orders: twice n * 2^-52 * sum|v|, computed per row)."""
    for key, w in want.items():
        if key == "bound":
            continue
        g = got[key]
        if g.dtype != w.dtype or g.shape != w.shape:
            return f"{key}: {g.dtype} {g.shape}, expected {w.dtype} {w.shape}"
        if key == "table" and c["a"].dtype == np.float64:
            sums = [ref.COLS.index("sum"), ref.COLS.index("ring_sum")]
            rest = [i for i in range(ref.NCOLS) if i not in sums]
            if g[..., rest].tobytes() != w[..., rest].tobytes():
                return f"{key}: the exact columns differ"
            if not np.array_equal(np.isnan(g[..., sums]), np.isnan(w[..., sums])):
                return f"{key}: NaN rows differ"
            off = np.abs(np.nan_to_num(g[..., sums]) - np.nan_to_num(w[..., sums]))
            if (off > want["bound"]).any():
                return f"{key}: a float64 sum is off by {float(off.max())}, bound {float(want['bound'].max())}"
        elif g.tobytes() != w.tobytes():
            differ = g != w
            return f"{key}: {int(differ.sum())} entries differ, the first at {tuple(np.argwhere(differ)[0]) if differ.any() else None}"
    return None


def run(ctx, scratch_check=False):
    """Every case once: {"case / result": {"sha256", "equal", "dirty"}}"""
    out = {}
    for c in cases():
        dirty = []

        def check():
            if scratch_check:
                found = ctx.scratch_check()
                if found is not None:
                    dirty.append(list(found))
        got = run_case(ctx, c, check)
        bad = mismatch(c, got, reference(c))
        for key, arr in got.items():
            out[f"{c['name']} / {key}"] = {"sha256": digest(arr), "equal": bad is None, "dirty": dirty[:1] or None}
    return out


# ---- the planted fixture ------------------------------------------------------------------------------------------------
PLANTED = {"shape": (128, 128), "n": 40, "sigma": 1.3, "amplitude": 800.0, "background": 100.0, "apart": 6.0, "seed": 2024}
PLANTED_ARGS = {"sigma": 1.0, "min_distance": 2, "snr": 8.0}


def planted_plane():
    """-> (uint16 plane, (n, 2) float64 true centres (y, x)): Gaussian spots on a flat background with Poisson noise, at
    least ``apart`` pixels from one another and from the edges"""
    def make():
        rng = np.random.default_rng(PLANTED["seed"])
        H, W = PLANTED["shape"]
        centres = []
        while len(centres) < PLANTED["n"]:
            c = np.array([rng.uniform(PLANTED["apart"], H - 1 - PLANTED["apart"]), rng.uniform(PLANTED["apart"], W - 1 - PLANTED["apart"])])
            if all(np.hypot(*(c - o)) >= PLANTED["apart"] for o in centres):
                centres.append(c)
        centres = np.array(centres)
        yy, xx = np.mgrid[0:H, 0:W]
        clean = np.full((H, W), PLANTED["background"])
        for cy, cx in centres:
            clean += PLANTED["amplitude"] * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * PLANTED["sigma"] ** 2))
        return rng.poisson(clean).astype(np.uint16), centres
    return _memo("planted", make)


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="the spot case table on the device")
    ap.add_argument("--json", required=True)
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison_child.write(args.json, {"cases": run(get_context(), scratch_check=poison_child.poisoned())})
    return 0


if __name__ == "__main__":
    sys.exit(main())
