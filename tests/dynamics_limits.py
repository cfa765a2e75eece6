"""The Cellpose flow -> mask kernels (csrc/amt_dynamics.hip) on both sides of every switch they contain: the case table,
the census that says where each case sits, and the runner.

The kernels switch on counts and sizes that smooth synthetic flows never place exactly: a histogram bin is a seed above 10
pixels and is grown into above 2; growth runs five rounds in an 11 x 11 patch; tied seeds are ordered by raster index and
overlaps go to the later one; ``max_seeds`` seeds fit and one more does not; the size floor and ceiling; three diffusion
classes by the box with its ring; launch strides of 2048 labels and 512 seeds; the 48 KiB box map of the parallel hole
kernel and its ``nested`` flag; the rules ``|dY / 5| > 1e-3`` and ``cellprob > threshold`` at equality.  ``limits()`` reads
those numbers from the source and pins the text of the rules the census restates.

The seed and size cases use a PROGRAMMABLE HISTOGRAM: cell pixels of column x with dY = -1e6 and ``niter = 1`` all end in row
0 of their column, so bin (CP_RPAD, CP_RPAD + x) holds exactly as many pixels as the column has cells; every other bin holds
1 or 0.  The mirror images pile onto the bottom row and (with a small dY that makes the pixels "move") the left and right
columns.  The census does not trust the construction: it computes the histogram from ``cd.follow_flows``.

``run(ctx, groups, scratch_check)`` runs the cases on the device and returns one record per case in the form of
tests/operator_sweep.py (whose Recorder, rules and digest it uses): labels and counts bit for bit against
``cd.compute_masks`` / ``cd.fill_holes_and_remove_small_masks``, flow errors within rtol 1e-9 / atol 1e-12 of
``cd.flow_error``; every case once alone and once as plane 1 of a two-plane call beside a different case.

``python -m tests.dynamics_limits --json PATH`` runs everything and writes the records and the scratch findings.  Not
collected by pytest (tests/test_host_dynamics_limits.py and tests/test_gpu_dynamics_limits.py are)."""
from __future__ import annotations

import contextlib
import hashlib
import json
import os
import re
import sys
import time

import numpy as np
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import operator_sweep as sw  # noqa: E402
import poison_child  # noqa: E402
from oracle import cellpose_dynamics as cd  # noqa: E402

_I32, _F32, _F64 = np.int32, np.float32, np.float64
CSRC = os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc")
GROUPS = ["seeds and growth", "size filters", "diffusion classes", "holes"]
# cases that do not run, each with its reason: none
EXCLUDED: dict = {}
ERR_RTOL, ERR_ATOL = 1e-9, 1e-12  # the project's bar for the flow errors (tests/test_gpu_cellpose.py, the sweep)
BIG_FLOW = 1e6  # dP of a piled pixel: one Euler step of 2e5 pixels, clamped to the frame


# ---------------------------------------------------------------------------------------------------------------------
# the limits, read from the kernel source
# ---------------------------------------------------------------------------------------------------------------------
def limits():
    """The numbers the switches of amt_dynamics.hip compare with, by pattern from the source: a retune changes what this
    returns, and tests/test_host_dynamics_limits.py then says which case no longer sits where it claims."""
    src = open(os.path.join(CSRC, "amt_dynamics.hip")).read()

    def one(pattern, what, cast=int):
        m = re.findall(pattern, src)
        assert len(m) == 1, f"{what}: {len(m)} matches of {pattern!r}"
        return cast(m[0])

    out = {"CP_RPAD": one(r"constexpr int CP_RPAD = (\d+);", "CP_RPAD"),
           "CP_HOLE_TILE": one(r"constexpr int CP_HOLE_TILE = (\d+) \* 1024;", "CP_HOLE_TILE") * 1024}
    assert out["CP_RPAD"] == cd.RPAD, "the oracle pads its histogram like the kernels"
    # the three diffusion launches: <TILE_MAX, TILE_MIN> and the cap of their grids
    classes = re.findall(r"cp_diffuse_kernel<(\d+), (\d+)>, dim3\((glab(?: < (\d+) \? glab : \4)?), nplanes\)", src)
    assert len(classes) == 3, "the three cp_diffuse_kernel launches"
    out["DIFFUSE_CLASSES"] = [[int(c[0]), int(c[1])] for c in classes]
    out["LABEL_STRIDE"] = one(r"const int glab = cap < (\d+) \? cap : \1;", "the label stride of the flow-error launches")
    out["DIFFUSE_STRIDES"] = [int(c[3]) if c[3] else out["LABEL_STRIDE"] for c in classes]
    out["HOLES_STRIDE"] = one(r"const int gl = cap < (\d+) \? cap : \1;", "the label stride of cp_holes_kernel")
    out["GROW_STRIDE"] = one(r"hipLaunchKernelGGL\(cp_grow_kernel, dim3\((\d+), nplanes\)", "the seed stride of cp_grow_kernel")
    out["SEED_FLOOR"] = one(r"if \(v <= (\d+)\) continue;", "a bin is a seed above")
    out["GROW_FLOOR"] = one(r"h\[\(size_t\)y \* Wp \+ x\] > (\d+)\) \? 1 : 0;", "a bin is grown into above")
    out["GROW_ROUNDS"] = one(r"for \(int it = 0; it < (\d+); \+\+it\) \{\n\s+unsigned char nv\[2\]", "the growth rounds")
    patch = one(r"__shared__ unsigned char cur\[(\d+)\], good\[\1\];", "the growth patch")
    out["GROW_PATCH"] = int(round(patch ** 0.5))
    assert out["GROW_PATCH"] ** 2 == patch and out["GROW_PATCH"] == 2 * out["GROW_ROUNDS"] + 1
    assert f"cy + t / {out['GROW_PATCH']} - {out['GROW_ROUNDS']}" in src and f"t == {patch // 2} ? 1 : 0" in src
    moves = set(re.findall(r"fabsf\(dY\[i\] / 5\.0f\) > (\d+e-\d+)f", src))
    assert len(moves) == 1, "the moves rule of cp_follow_prep_kernel and cp_follow_kernel"
    out["MOVES"] = float(moves.pop())
    # the rules the census restates, pinned as text
    for text in (
            "const bool cell = pr[i] > thr;",                                              # a cell: strictly above
            "mv[u] = cell && fabsf(dY[i] / 5.0f) > 1e-3f;",                                 # it moves: strictly above
            "if (k < cap) seeds[",                                                         # max_seeds seeds fit
            "if (nseeds[plane] > cap) nout[plane] = -1;",                                  # one more: count -1
            "rank += s[j] > me;",                                                          # count, then raster index, descending
            "atomicMax(&M[",                                                               # overlaps: the later seed
            "return c[l] >= min_size && c[l] > 0 && (long long)c[l] <= big;",              # floor and ceiling, plain path
            "cnt[k] > 0 && cnt[k] >= min_size) v =",                                       # the floor, post path (parallel)
            "if (min_size > 0 && npix < min_size) {",                                      # the floor, post path (sequential)
            "const int th = b.y1 - b.y0 + 3, tw = b.x1 - b.x0 + 3;",                       # the box with its ring
            "if (npx <= TILE_MIN || (TILE_MAX > 0 && npx > TILE_MAX)) continue;",          # the class of a label
            "if (h < 3 || w < 3) continue;",                                               # no interior
            "if ((long long)h * w > CP_HOLE_TILE) {",                                      # the box map does not fit LDS
            "if (other > 0 && other <= K && kp[other]) nested[plane] = 1;",                # a kept label inside a hole
            "if (d < best) {",                                                             # centre ties: the first in raster order
    ):
        assert text in src, f"amt_dynamics.hip no longer holds: {text}"
    return out


def diffuse_class(lim, h, w):
    """Which of the three cp_diffuse_kernel launches takes a label with an h x w box: 0, 1 or 2."""
    npx = (h + 2) * (w + 2)
    took = [i for i, (tmax, tmin) in enumerate(lim["DIFFUSE_CLASSES"]) if not (npx <= tmin or (tmax > 0 and npx > tmax))]
    assert len(took) == 1, (h, w, took)
    return took[0]


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
def moves_pair():
    """(d_eq, d_above): float32 dY with dY / 5 == float32(1e-3) exactly, and the next float32, whose quotient is one ulp above."""
    t = _F32(limits()["MOVES"])
    d = _F32(5) * t
    while _F32(d) / _F32(5) > t:
        d = np.nextafter(d, _F32(0))
    while _F32(np.nextafter(d, _F32(1))) / _F32(5) <= t:
        d = np.nextafter(d, _F32(1))
    return _F32(d), _F32(np.nextafter(d, _F32(1)))


def piles(H, W, spec, side="top", small=0.01, prob=None):
    """The programmable histogram.  ``spec`` = {index: count or (first, count)}: of column (side top / bottom) or row (left /
    right) ``index``, ``count`` pixels counted from the side (or from pixel ``first``) are cells with a flow of BIG_FLOW
    towards the side.  ``small`` = the dY of the rows' pixels (left / right), which must make them move.  -> (dP, cellprob)."""
    dP, pr = np.zeros((2, H, W), _F32), np.full((H, W), -1.0, _F32)
    for i, c in spec.items():
        first, c = c if isinstance(c, tuple) else (0, c)
        if side == "top":
            sl = (slice(first, first + c), i)
        elif side == "bottom":
            sl = (slice(H - first - c, H - first), i)
        elif side == "left":
            sl = (i, slice(first, first + c))
        else:
            sl = (i, slice(W - first - c, W - first))
        pr[sl] = 1.0 if prob is None else prob.get(i, 1.0)
        if side in ("top", "bottom"):
            dP[0][sl] = -BIG_FLOW if side == "top" else BIG_FLOW
        else:
            dP[1][sl] = -BIG_FLOW if side == "left" else BIG_FLOW
            dP[0][sl] = small.get(i, 0.01) if isinstance(small, dict) else small
    return dP, pr


def boxes_plane(shape, boxes):
    """int32 labels of solid boxes [(y0, x0, h, w)], numbered in raster order of first appearance (as get_masks numbers)."""
    lab = np.zeros(shape, _I32)
    for k, (y0, x0, h, w) in enumerate(sorted(boxes), start=1):
        assert y0 >= 0 and x0 >= 0 and y0 + h <= shape[0] and x0 + w <= shape[1] and not lab[y0:y0 + h, x0:x0 + w].any()
        lab[y0:y0 + h, x0:x0 + w] = k
    return lab


def contraction_flows(labels, k=0.5):
    """Flows under which every label's pixels converge to one point inside the bin of the label's box centre:
    dP / 5 = k (c - position) with c chosen so that the fixed point of the sampled field, (c + 0.5) (size - 1) / size, is
    the middle of that bin.  -> (dP, cellprob)."""
    H, W = labels.shape
    dP, pr = np.zeros((2, H, W), _F64), np.where(labels > 0, 1.0, -1.0).astype(_F32)
    yy, xx = np.mgrid[0:H, 0:W].astype(_F64)
    for i, sl in enumerate(ndi.find_objects(labels)):
        if sl is None:
            continue
        m = labels == i + 1
        by, bx = (sl[0].start + sl[0].stop - 1) // 2, (sl[1].start + sl[1].stop - 1) // 2
        cy, cx = (by + 0.5) * H / (H - 1) - 0.5, (bx + 0.5) * W / (W - 1) - 0.5
        dP[0][m] = (5 * k * (cy - yy))[m]
        dP[1][m] = (5 * k * (cx - xx))[m]
    return dP.astype(_F32), pr


def normal_flows(shape, seed):
    return np.random.default_rng(seed).normal(0, 1, (2,) + tuple(shape)).astype(_F32)


def frame(h, w, t=1):
    m = np.ones((h, w), bool)
    m[t:h - t, t:w - t] = False
    return m


def spiral(n, closed):
    """A one-pixel square spiral from the top-left corner inwards with one pixel of background between its turns: the
    background corridor opens at (1, 0) on the box's border -- nothing is a hole -- unless ``closed`` stops the mouth."""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx
        if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
            y, x = ny, nx
            m[y, x] = True
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    if closed:
        m[1, 0] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
MASKS_DEFAULTS = {"thr": 0.0, "niter": 1, "min_size": 0, "frac": 0.4, "max_seeds": 16384, "flow_threshold": 0.0,
                  "fill_holes": False}
DIFFUSE_SHAPE = (100, 470)
DIFFUSE_NITER = 40  # Euler steps of the contraction flows: the distance to the fixed point halves with every step
# (y0, x0, h, w): ringed tiles of 2304, 2305, 6400 and 6401 pixels
DIFFUSE_BOXES = {
    "apart": [(1, 1, 3, 459), (6, 1, 78, 78), (6, 81, 46, 46), (6, 129, 35, 171)],
    "touching": [(0, 0, 3, 459), (3, 0, 78, 78), (3, 78, 46, 46), (3, 124, 35, 171)],
    "frame": [(97, 11, 3, 459), (0, 0, 78, 78), (0, 424, 46, 46), (0, 100, 35, 171)],
}
TILE_SHAPE = (260, 270)
HOLE_PARAMS = [(0, True), (15, True), (0, False), (15, False)]  # (min_size, fill_holes)
_CASES: list = []


def _masks_case(group, name, planes, **params):
    bad = set(params) - set(MASKS_DEFAULTS)
    assert not bad, bad
    return {"group": group, "name": name, "kind": "masks", "planes": planes, "params": dict(MASKS_DEFAULTS, **params)}


def _seed_cases():
    g = "seeds and growth"
    H, W = 40, 50
    out = [
        _masks_case(g, "bins of 10, 11 and 20", [piles(H, W, {10: 20, 30: 11, 40: 10})]),
        _masks_case(g, "neighbours of 2 and 3", [piles(H, W, {10: 20, 11: 3, 9: 2, 30: 20, 31: 2, 29: 3})]),
        _masks_case(g, "a run of 7 bins above 2", [piles(H, W, {10: 20, **{x: 3 for x in range(11, 18)}})]),
        _masks_case(g, "plateau of 520 tied seeds", [piles(24, 520, {x: 24 for x in range(520)})]),
        _masks_case(g, "plateau of 512 tied seeds", [piles(24, 512, {x: 24 for x in range(512)})]),
        _masks_case(g, "two tied seeds 4 bins apart",
                    [piles(H, W, {10: 20, 14: 20, **{x: 3 for x in (11, 12, 13, 15, 16, 17, 18, 19)}})]),
        _masks_case(g, "niter 0", [piles(H, W, {10: 20, 30: 11, 40: 10})], niter=0),
        _masks_case(g, "two rows", [piles(2, 50, {0: 20, 1: 11}, "left")]),
        _masks_case(g, "two columns", [piles(50, 2, {0: 20, 1: 11})]),
    ]
    for side in ("top", "bottom", "left", "right"):
        last = (W if side in ("top", "bottom") else H) - 1
        out.append(_masks_case(g, f"piles in the corners and on the edge: {side}",
                               [piles(H, W, {0: 20, 1: 3, last // 2: 11, last - 1: 3, last: 20}, side)]))
    # cellprob == threshold is no cell: column 20 has 11 pixels of which one sits ON the threshold, column 30 one ulp above
    thr = 0.5
    dP, pr = piles(H, W, {10: 11, 20: 11, 30: 11})
    pr[10, 20] = _F32(thr)
    pr[:11, 30] = np.nextafter(_F32(thr), _F32(1))
    out.append(_masks_case(g, "cellprob on the threshold", [(dP, pr)], thr=thr))
    # |dY / 5| == 1e-3 does not move: row 5 holds 11 such pixels, row 15 eleven one ulp above, row 25 a plain pile
    d_eq, d_above = moves_pair()
    out.append(_masks_case(g, "dY / 5 on 1e-3 and one ulp above",
                           [piles(H, W, {5: 11, 15: 11, 25: 20}, "left", small={5: d_eq, 15: d_above})]))
    three = piles(H, W, {10: 20, 25: 15, 40: 12})
    four = piles(H, W, {10: 20, 25: 15, 40: 12, 45: 13})
    out += [
        _masks_case(g, "max_seeds equal to the seed count", [three], max_seeds=3),
        _masks_case(g, "max_seeds one below the seed count", [three], max_seeds=2),
        _masks_case(g, "batch: fitting plane, overflowing plane", [three, four], max_seeds=3),
        _masks_case(g, "batch: overflowing plane, fitting plane", [four, three], max_seeds=3),
    ]
    return out


def _ceiling_plane(total):
    """20 x 10, one label of ``total`` pixels: the seed column of 20 with neighbours of 19, 19, 18 and a last one of 3 to 5."""
    return piles(20, 10, {2: 20, 1: 19, 3: 19, 4: 18, 0: total - 76})


def _size_cases():
    g = "size filters"
    floor = piles(40, 50, {10: 14, 25: 15, 40: 16})
    out = [
        _masks_case(g, "floor 14 15 16, plain path", [floor], min_size=15),
        _masks_case(g, "floor 14 15 16, fill_holes alone", [floor], min_size=15, fill_holes=True),
        _masks_case(g, "floor 14 15 16, flow_threshold alone", [floor], min_size=15, flow_threshold=1e30),
        # float32(0.01) lies below 0.01: 2,000 pixels give 19.9999995 there, 20 in float64
        _masks_case(g, "ceiling 19 20 21 of 2000 x 0.01", [piles(40, 50, {10: 19, 25: 20, 40: 21})], frac=0.01),
        _masks_case(g, "ceiling 19 20 21 of 2000 x 0.01, post path", [piles(40, 50, {10: 19, 25: 20, 40: 21})], frac=0.01,
                    fill_holes=True),
    ]
    # float32(0.4) lies above 0.4: 200 pixels give 80 either way
    for total in (79, 80, 81):
        out.append(_masks_case(g, f"ceiling {total} of 200 x 0.4", [_ceiling_plane(total)], frac=0.4))
    return out


def _thresholds_between(err):
    """float32 thresholds between consecutive reference errors (pairs closer than 1e-6 relative skipped), one below all of
    them and one above."""
    e = np.sort(np.asarray(err, _F64))
    out = [float(_F32(e[0] / 2))]
    for a, b in zip(e[:-1], e[1:]):
        t = float(_F32((a + b) / 2))
        if b - a > 1e-6 * b and a < t < b:
            out.append(t)
    out.append(float(_F32(e[-1] * 2)))
    assert all(t > 0 and not np.any(e == t) for t in out)
    return out


def _diffusion_cases():
    g = "diffusion classes"
    out = []
    for name, boxes in DIFFUSE_BOXES.items():
        lab = boxes_plane(DIFFUSE_SHAPE, boxes)
        out.append({"group": g, "name": f"four boxes {name}", "kind": "flow_error", "planes": [(lab, normal_flows(lab.shape, 11))],
                    "params": {"max_label": 4, "nlabels": 4}})
        # through cellpose_masks: where the boxes stand apart, get_masks gives them back; where they touch, a border pixel
        # samples its neighbour's flow and some change sides (the census shows the labels the oracle really makes)
        dP, pr = contraction_flows(lab)
        pre = cd.get_masks(cd.follow_flows(dP, pr > 0, DIFFUSE_NITER), MASKS_DEFAULTS["frac"], 0).astype(_I32)
        with _memo():
            err = cd.flow_error(pre, dP)
        for t in _thresholds_between(err):
            out.append(_masks_case(g, f"four boxes {name}, flow_threshold {t:.9g}", [(dP, pr)], niter=DIFFUSE_NITER, flow_threshold=t))
    # labels missing from the numbering; nlabels below and equal to max_label
    gaps = np.zeros((30, 40), _I32)
    gaps[2:9, 3:12], gaps[12:20, 20:26], gaps[22:28, 5:30] = 1, 3, 6
    for nl, mx in ((6, 6), (6, 9), (7, 9)):
        out.append({"group": g, "name": f"labels 1 3 6, nlabels {nl}, max_label {mx}", "kind": "flow_error",
                    "planes": [(gaps, normal_flows(gaps.shape, 12))], "params": {"max_label": mx, "nlabels": nl}})
    # a centre tie: the 2 x 2 block (four pixels at the same distance) and a transpose-symmetric mask with mean 4 / 3
    tie = np.zeros((12, 12), _I32)
    tie[1:3, 1:3] = 1
    tie[5, 6] = tie[6, 5] = tie[8, 8] = 2
    out.append({"group": g, "name": "centre ties", "kind": "flow_error", "planes": [(tie, normal_flows(tie.shape, 13))],
                "params": {"max_label": 2, "nlabels": 2}})
    for many in (many_labels(False), many_labels(False, 32, 64)):
        k = int(many.max())
        out.append({"group": g, "name": f"{k} labels of 3 x 3", "kind": "flow_error", "planes": [(many, normal_flows(many.shape, 14))],
                    "params": {"max_label": k, "nlabels": k}})
    return out


def many_labels(rings, rows=46, cols=46):
    """rows x cols labels of 3 x 3 pixels (``rings``: without their centre), one pixel apart: 2,116 on 184 x 184, or the
    2,048 of 32 x 64 on 128 x 256."""
    y, x = np.mgrid[0:4 * rows, 0:4 * cols]
    lab = np.where((y % 4 < 3) & (x % 4 < 3), (y // 4) * cols + x // 4 + 1, 0).astype(_I32)
    if rings:
        lab[(y % 4 == 1) & (x % 4 == 1)] = 0
    return lab


def _tile_frames(lim):
    """Closed one-pixel frames whose box is exactly CP_HOLE_TILE bytes and one byte more, each with a small ring elsewhere."""
    tile = lim["CP_HOLE_TILE"]
    assert tile == 192 * 256 and tile + 1 == 247 * 199
    planes = {}
    for key, (h, w) in (("on the tile", (192, 256)), ("one byte past the tile", (247, 199))):
        lab = np.zeros(TILE_SHAPE, _I32)
        lab[1:1 + h, 1:1 + w][frame(h, w)] = 1
        lab[252:257, 262:267][frame(5, 5)] = 2
        planes[key] = lab
    return planes


def _nested_plane(ring_first, inner_px):
    """A 9 x 9 ring and a second label with a 3 x 3 (or 2 x 2) fragment inside the ring's hole and 8 pixels outside."""
    lab = np.zeros((16, 30), _I32)
    a, b = (1, 2) if ring_first else (2, 1)
    lab[2:11, 2:11][frame(9, 9)] = a
    lab[5:5 + inner_px, 5:5 + inner_px] = b
    lab[4:6, 20:24] = b
    return lab


def _holes_inputs(lim):
    """{name: [label planes]} of the holes group."""
    frames = _tile_frames(lim)
    small = np.zeros((14, 24), _I32)
    small[1:3, 1:11], small[3:13, 20:22] = 1, 2
    small[5:8, 2:5][frame(3, 3)] = 3
    small[5:8, 8:11] = 4
    inside = {}
    for first in (True, False):
        lab = np.zeros((16, 30), _I32)
        a, b = (1, 2) if first else (2, 1)
        lab[2:11, 2:11][frame(9, 9)] = a
        lab[5:8, 5:8] = b  # 9 pixels: dropped at min_size 15, kept at 0
        inside[first] = lab
    above = _nested_plane(True, 3).copy()
    above[13, 25:29] = 7  # a value above max_label = 2: background
    sp = {c: np.pad(spiral(41, c), 2).astype(_I32) for c in (False, True)}
    return {
        "frame on the tile": [frames["on the tile"]], "frame one byte past the tile": [frames["one byte past the tile"]],
        "batch: unflagged frame, flagged frame": [frames["on the tile"], frames["one byte past the tile"]],
        "batch: flagged frame, unflagged frame": [frames["one byte past the tile"], frames["on the tile"]],
        "boxes of 2 x N, N x 2 and 3 x 3": [small],
        "open spiral": [sp[False]], "closed spiral": [sp[True]],
        "fragment in a hole, ring first": [_nested_plane(True, 3)], "fragment in a hole, ring later": [_nested_plane(False, 3)],
        "small label in a hole, ring first": [inside[True]], "small label in a hole, ring later": [inside[False]],
        "a value above max_label": [above],
        "2116 rings of 3 x 3": [many_labels(True)], "2048 rings of 3 x 3": [many_labels(True, 32, 64)],
    }


def _holes_cases():
    g = "holes"
    lim = limits()
    out = []
    for name, planes in _holes_inputs(lim).items():
        mx = 2 if name == "a value above max_label" else max(int(p.max()) for p in planes)
        for min_size, fill in HOLE_PARAMS:
            out.append({"group": g, "name": f"{name}, min_size {min_size}, fill {int(fill)}", "kind": "holes", "planes": planes,
                        "params": {"max_label": mx, "nlabels": mx, "min_size": min_size, "fill_holes": fill}})
    # through cellpose_masks(fill_holes=True): a frame two pixels thick at top and bottom piles onto row 0 (one label with a
    # hole of 17 x 3), the 13 cell pixels inside the hole pile onto the bottom row (a label of its own, inside the hole)
    H, W = 40, 50
    dP, pr = piles(H, W, {8: 21, 12: 21, 9: 2, 10: 2, 11: 2})
    for x in (9, 10, 11):
        pr[19:21, x], dP[0, 19:21, x] = 1.0, -BIG_FLOW
    pr[4:17, 10], dP[0, 4:17, 10] = 1.0, BIG_FLOW
    dP2, pr2 = piles(H, W, {30: 14, 40: 16})
    for a, b in ((dP, dP2), (pr, pr2)):
        a[..., 25:] = b[..., 25:]
    for min_size in (0, 15):
        out.append(_masks_case(g, f"a frame with a label in its hole, min_size {min_size}", [(dP, pr)], min_size=min_size,
                               fill_holes=True))
        out.append(_masks_case(g, f"a frame with a label in its hole, min_size {min_size}, not filled", [(dP, pr)],
                               min_size=min_size, flow_threshold=1e30))
    return out


def cases():
    """The table (made once; every array read-only)."""
    if not _CASES:
        for c in _seed_cases() + _size_cases() + _diffusion_cases() + _holes_cases():
            for pl in c["planes"]:
                for a in pl if isinstance(pl, tuple) else (pl,):
                    a.setflags(write=False)
            _CASES.append(c)
        names = [(c["group"], c["name"]) for c in _CASES]
        assert len(set(names)) == len(names)
    return _CASES


# ---------------------------------------------------------------------------------------------------------------------
# references (computed once, shared, read-only)
# ---------------------------------------------------------------------------------------------------------------------
_FLOWS_MEMO: dict = {}
_REF: dict = {}
_MASKS_TO_FLOWS = cd.masks_to_flows
_SPARED = [0.0]  # seconds of diffusion that remembered results spared since the last reset


@contextlib.contextmanager
def _memo():
    """While open, ``cd.masks_to_flows`` -- a pure function of the masks, and the whole cost of ``cd.flow_error`` -- remembers
    its results: the label planes of the diffusion group go through it once, not once per threshold."""
    def remembered(masks, n_iter=None):
        key = (masks.shape, str(masks.dtype), n_iter, hashlib.sha256(np.ascontiguousarray(masks).tobytes()).hexdigest())
        if key not in _FLOWS_MEMO:
            t0 = time.perf_counter()
            mu, T = _MASKS_TO_FLOWS(masks, n_iter)
            mu.setflags(write=False)
            T.setflags(write=False)
            _FLOWS_MEMO[key] = (mu, T, time.perf_counter() - t0)
        else:
            _SPARED[0] += _FLOWS_MEMO[key][2]  # what the caller would have spent
        return _FLOWS_MEMO[key][:2]

    cd.masks_to_flows = remembered
    try:
        yield
    finally:
        cd.masks_to_flows = _MASKS_TO_FLOWS


def _key(c):
    return (c["group"], c["name"])


def seeds_of(c, plane=0, lim=None):
    """(histogram, flat seed indices in the kernels' order) of a masks case, from ``cd.follow_flows``."""
    lim = lim or limits()
    dP, pr = c["planes"][plane]
    p = c["params"]
    cell = pr > _F32(p["thr"])
    pos = cd.follow_flows(dP, cell, p["niter"])
    H, W = pr.shape
    R = lim["CP_RPAD"]
    h = np.zeros((H + 2 * R, W + 2 * R), np.int64)
    np.add.at(h, (pos[0].astype(_I32).ravel() + R, pos[1].astype(_I32).ravel() + R), 1)
    s = np.flatnonzero((h == ndi.maximum_filter(h, 5, mode="reflect")) & (h > lim["SEED_FLOOR"]))
    s = s[np.lexsort((s, h.ravel()[s]))[::-1]]
    return h, s, pos


def reference(c):
    """Per plane what the case must give -> ([per-plane tuples], seconds it takes from nothing).  masks: (labels, count) of
    ``cd.compute_masks``, or (None, -1) for a plane with more seeds than max_seeds; flow_error: (errors padded with zeros to
    max_label,); holes: (labels, count) of ``cd.fill_holes_and_remove_small_masks`` (values above max_label background)."""
    if _key(c) in _REF:
        return _REF[_key(c)]
    p = c["params"]
    t0 = time.perf_counter()
    _SPARED[0] = 0.0
    wants = []
    with _memo(), np.errstate(invalid="ignore", divide="ignore"):  # ndimage.mean of an absent label: 0 / 0, then nan_to_num
        for i, pl in enumerate(c["planes"]):
            if c["kind"] == "masks":
                if len(seeds_of(c, i)[1]) > p["max_seeds"]:
                    wants.append((None, np.asarray(-1, _I32)))
                    continue
                m = cd.compute_masks(pl[0], pl[1], p["thr"], p["niter"], p["min_size"], p["frac"], p["flow_threshold"] or None,
                                     p["fill_holes"]).astype(_I32)
                wants.append((m, np.asarray(m.max(), _I32)))
            elif c["kind"] == "flow_error":
                e = np.zeros(p["max_label"], _F64)
                if pl[0].any():
                    r = cd.flow_error(pl[0], pl[1])
                    e[:r.size] = r
                wants.append((e,))
            else:
                m = cd.fill_holes_and_remove_small_masks(np.where(pl <= p["max_label"], pl, 0), p["min_size"],
                                                         p["fill_holes"]).astype(_I32)
                wants.append((m, np.asarray(m.max(), _I32)))
    for w in wants:
        for a in w:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _REF[_key(c)] = (wants, time.perf_counter() - t0 + _SPARED[0])  # the time of the reference computed from nothing
    return _REF[_key(c)]


# ---------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------
def canon(lab):
    """The labels renumbered in raster order of first appearance: equal for equal partitions."""
    ids, first = np.unique(lab.ravel(), return_index=True)
    order = [i for i in ids[np.argsort(first)] if i > 0]
    lut = np.zeros(int(lab.max()) + 1, _I32)
    lut[order] = np.arange(1, len(order) + 1)
    return lut[lab]


def _flipped(pl):
    dP, pr = pl
    return np.ascontiguousarray(dP[:, :, ::-1]) * np.array([1, -1], _F32)[:, None, None], np.ascontiguousarray(pr[:, ::-1])


def hole_flags(lim, lab, max_label, nlabels, min_size):
    """What cp_holes_kernel decides for a plane: {"flagged": the sequential kernel redoes it, "large": labels whose box map
    exceeds CP_HOLE_TILE, "nested": kept labels with another kept label's pixel in a hole, "flat": kept labels skipped for
    h < 3 or w < 3, "boxes": [h * w of every kept label]}."""
    lab = np.where(lab <= max_label, lab, 0)
    cnt = np.bincount(lab.ravel(), minlength=max_label + 1)
    kept = [l for l in range(1, nlabels + 1) if cnt[l] > 0 and cnt[l] >= min_size]
    out = {"large": [], "nested": [], "flat": [], "boxes": [], "kept": kept}
    objs = ndi.find_objects(lab, max_label)
    for l in kept:
        sl = objs[l - 1]
        h, w = sl[0].stop - sl[0].start, sl[1].stop - sl[1].start
        out["boxes"].append(h * w)
        if h < 3 or w < 3:
            out["flat"].append(l)
        elif h * w > lim["CP_HOLE_TILE"]:
            out["large"].append(l)
        else:
            m = lab[sl] == l
            inside = lab[sl][ndi.binary_fill_holes(m) & ~m]
            if np.isin(inside[inside > 0], kept).any():
                out["nested"].append(l)
    out["flagged"] = bool(out["large"] or out["nested"])
    return out


def census(c, lim=None):
    """Where a case sits.  masks: per plane the seeds' counts in the kernels' order, the bins around them, the pixel counts
    of the oracle's labels before any size filter, the ceiling in float64 and as the float32 fraction gave it, whether the
    tie order matters; flow_error: per label the box, the ringed tile and the class; holes: ``hole_flags``."""
    lim = lim or limits()
    p = c["params"]
    out = {"kind": c["kind"], "shape": list(np.shape(c["planes"][0][-1] if c["kind"] != "holes" else c["planes"][0]))}
    rows = []
    for i, pl in enumerate(c["planes"]):
        if c["kind"] == "masks":
            h, s, pos = seeds_of(c, i, lim)
            n = pl[1].size
            pre = cd.get_masks(pos, 1.0, 0)
            cell = pl[1] > _F32(p["thr"])
            f0 = np.abs(pl[0][0].astype(_F32) * cell.astype(_F32) / _F32(5))
            row = {"nseeds": int(s.size), "seed_counts": h.ravel()[s].tolist(), "seed_bins": [list(divmod(int(v), h.shape[1])) for v in s],
                   "hist_max_elsewhere": int(np.delete(h.ravel(), s).max()), "hist": h,
                   "sizes": sorted(np.bincount(pre.ravel())[1:].tolist()), "pre": pre,
                   "big": int(n * p["frac"]), "big_f32": int(n * float(_F32(p["frac"]))),
                   "overflow": bool(s.size > p["max_seeds"]), "cells": int(cell.sum()),
                   "movers": int((cell & (f0 > _F32(lim["MOVES"]))).sum()),
                   "on_moves": int((cell & (f0 == _F32(lim["MOVES"]))).sum()),
                   "on_threshold": int((pl[1] == _F32(p["thr"])).sum())}
            if p["flow_threshold"] and not row["overflow"] and pre.any():
                with _memo():
                    row["errors"] = cd.flow_error(cd.get_masks(pos, p["frac"], 0).astype(_I32), pl[0]).tolist()
        elif c["kind"] == "flow_error":
            lab = pl[0]
            labels = []
            for l, sl in enumerate(ndi.find_objects(lab), start=1):
                if sl is None:
                    continue
                bh, bw = sl[0].stop - sl[0].start, sl[1].stop - sl[1].start
                yi, xi = np.nonzero(lab[sl] == l)
                d = (xi - xi.mean()) ** 2 + (yi - yi.mean()) ** 2
                labels.append({"label": l, "box": [bh, bw], "tile": (bh + 2) * (bw + 2), "class": diffuse_class(lim, bh, bw),
                               "centre_ties": int((d == d.min()).sum()),
                               "frame": bool(sl[0].start == 0 or sl[1].start == 0 or sl[0].stop == lab.shape[0]
                                             or sl[1].stop == lab.shape[1])})
            row = {"labels": labels, "present": int(len(labels)), "max": int(lab.max()), "touching": _touch(lab)}
        else:
            row = hole_flags(lim, pl, p["max_label"], p["nlabels"], p["min_size"])
            row["max_value"] = int(pl.max())
        rows.append(row)
    out["planes"] = rows
    return out


def _touch(lab):
    """Two different labels 4-adjacent somewhere."""
    a = (lab[1:] > 0) & (lab[:-1] > 0) & (lab[1:] != lab[:-1])
    b = (lab[:, 1:] > 0) & (lab[:, :-1] > 0) & (lab[:, 1:] != lab[:, :-1])
    return bool(a.any() or b.any())


def tie_order_matters(c):
    """Does the oracle give another partition once the seeds of equal count are taken in the opposite order?  (The plane
    mirrored left to right, run, and mirrored back: seeds on one row swap their raster order.)"""
    p = c["params"]
    dP, pr = c["planes"][0]
    a = cd.compute_masks(dP, pr, p["thr"], p["niter"], p["min_size"], p["frac"])
    fd, fp = _flipped((dP, pr))
    b = cd.compute_masks(fd, fp, p["thr"], p["niter"], p["min_size"], p["frac"])[:, ::-1]
    return not np.array_equal(canon(a), canon(b))


def census_summary():
    """The census of every case without its arrays: what profiles/dynamics_limits.json records."""
    lim = limits()
    out = {}
    for c in cases():
        cen = census(c, lim)
        for row in cen["planes"]:
            row.pop("hist", None)
            row.pop("pre", None)
            for k in ("seed_counts", "seed_bins", "sizes"):
                if len(row.get(k, ())) > 8:
                    row[k] = row[k][:4] + [f"... {len(row[k]) - 4} more"]
            if "labels" in row and len(row["labels"]) > 8:
                row["labels"] = row["labels"][:2] + [f"... {len(row['labels']) - 2} more of the same box"]
            if "boxes" in row and len(row["boxes"]) > 8:
                row["boxes"], row["kept"] = row["boxes"][:2] + ["..."], len(row["kept"])
        out[f"{c['group']}: {c['name']}"] = cen
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
def _h():
    from arcadia_microscopy_tools_amd import hipops

    return hipops


def _call(ctx, c, planes):
    """The case's operator on a stack of planes -> tuple of numpy arrays, planes on axis 0."""
    h, p = _h(), c["params"]
    if c["kind"] == "masks":
        dP, pr = ctx.asarray(np.stack([pl[0] for pl in planes])), ctx.asarray(np.stack([pl[1] for pl in planes]))
        return sw._np(*h.cellpose_masks(dP, pr, p["thr"], p["niter"], p["min_size"], p["frac"], p["max_seeds"],
                                        flow_threshold=p["flow_threshold"], fill_holes=p["fill_holes"]))
    if c["kind"] == "flow_error":
        lab, dP = ctx.asarray(np.stack([pl[0] for pl in planes])), ctx.asarray(np.stack([pl[1] for pl in planes]))
        nl = ctx.asarray(np.full(len(planes), p["nlabels"], _I32))
        return sw._np(h.cellpose_flow_error(lab, dP, p["max_label"], nlabels=nl))
    nl = ctx.asarray(np.full(len(planes), p["nlabels"], _I32))
    return sw._np(*h.fill_holes_remove_small(ctx.asarray(np.stack(planes)), p["max_label"], p["min_size"], p["fill_holes"],
                                             nlabels=nl))


def _plane_result(c, outs, i, want):
    """(the arrays of plane i that are compared, their references): a plane with more seeds than max_seeds answers with
    its count alone."""
    got = tuple(o[i] for o in outs)
    if want[0] is None:
        return got[1:], want[1:]
    return got, want


def _shape_of(c):
    pl = c["planes"][0]
    return tuple((pl if c["kind"] == "holes" else pl[-1]).shape[-2:])


def companion(c, table):
    """The plane that stands in front of the case in its two-plane call: the first plane of another case of the same kind,
    shape and group whose input differs; a case with no such neighbour stands beside its own mirror image."""
    mine = c["planes"][0]
    for o in table:
        if o is c or o["kind"] != c["kind"] or o["group"] != c["group"] or _shape_of(o) != _shape_of(c):
            continue
        theirs = o["planes"][0]
        same = all(np.array_equal(a, b) for a, b in zip(mine, theirs)) if isinstance(mine, tuple) else np.array_equal(mine, theirs)
        if not same:
            return theirs
    if c["kind"] == "masks":
        return _flipped(mine)
    if c["kind"] == "flow_error":
        return np.ascontiguousarray(mine[0][:, ::-1]), np.ascontiguousarray(mine[1][:, :, ::-1])
    return np.ascontiguousarray(mine[:, ::-1])


def _run_case(ctx, rec, c, table):
    rules = (sw.close(ERR_RTOL, ERR_ATOL),) if c["kind"] == "flow_error" else (sw.exact, sw.exact)
    wants, _ = reference(c)
    shape = _shape_of(c)
    records = []

    def record(variant, pairs):
        status, index = "pass", None
        for k, (g, w, rule) in enumerate(pairs):
            ok, idx = rule(g, w)
            if not ok:
                status, index = "mismatch", repr((k, idx))
                break
        r = {"group": c["group"], "op": c["kind"], "param": c["name"], "shape": list(shape), "variant": variant,
             "status": status, "index": index, "sha256": sw._digest([np.asarray(g) for g, _, _ in pairs])}
        records.append(r)
        return r

    def pairs_of(outs, i, want):
        got, want = _plane_result(c, outs, i, want)
        return [(g, w, rule) for g, w, rule in zip(got, want, rules[len(rules) - len(got):])]

    t = time.perf_counter()
    rec.where = [c["kind"], c["name"], list(shape), "single"]
    outs = _call(ctx, c, c["planes"])
    pairs = [pr for i, w in enumerate(wants) for pr in pairs_of(outs, i, w)]
    single = record("single", pairs)
    if len(c["planes"]) == 1:
        rec.where[3] = "batch"
        outs = _call(ctx, c, [companion(c, table), c["planes"][0]])
        r = record("batch", pairs_of(outs, 1, wants[0]))
        if r["sha256"] != single["sha256"] and r["status"] == "pass":
            r.update(status="mismatch", index="plane 1 of the two-plane call differs from the single-plane result")
    else:  # a case of several planes: each plane alone must give what it gave in the batch
        for i, pl in enumerate(c["planes"]):
            rec.where[3] = f"plane {i} alone"
            alone = _call(ctx, c, [pl])
            r = record(f"plane {i} alone", pairs_of(alone, 0, wants[i]))
            if sw._digest([np.asarray(g) for g, _, _ in pairs_of(outs, i, wants[i])]) != r["sha256"] and r["status"] == "pass":
                r.update(status="mismatch", index=f"plane {i} of the batch differs from the plane alone")
    ms = round((time.perf_counter() - t) * 1e3 / len(records), 1)
    for r in records:
        r["ms"] = ms
    return records


def run(ctx, groups=None, scratch_check=False):
    """The cases of the groups (default: all): {"records": [...], "dirty": [...], "seconds": s}.  A mismatch is recorded
    and the run goes on; an exception from the library ends it at once."""
    records = []
    table = cases()
    t0 = time.perf_counter()
    with sw.Recorder(ctx, scratch_check) as rec:
        for group in (GROUPS if groups is None else groups):
            assert group in GROUPS, group
            for c in table:
                if c["group"] == group and _key(c) not in EXCLUDED:
                    records += _run_case(ctx, rec, c, table)
    return {"records": records, "dirty": rec.dirty, "seconds": time.perf_counter() - t0}


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", required=True, help="where to write the records and the scratch findings")
    ap.add_argument("--group", action="append", help="only this group (repeatable)")
    ap.add_argument("--profile", help="also write the run's time, its case counts, the limits and the census here")
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison = poison_child.poisoned()
    res = run(get_context(), args.group, scratch_check=poison)
    poison_child.write(args.json, res)
    bad = [r for r in res["records"] if r["status"] != "pass"]
    if args.profile:
        head = {"device": get_context().device_name(), "poison": poison, "seconds": round(res["seconds"], 2),
                "cases": len(res["records"]), "mismatches": len(bad), "dirty": len(res["dirty"]),
                "cases_per_group": {g: sum(r["group"] == g for r in res["records"]) for g in GROUPS}, "limits": limits()}
        with open(args.profile, "w") as f:  # one line per head entry and per case of the census
            lines = [f" {json.dumps(k)}: {json.dumps(v)}" for k, v in head.items()]
            cen = [f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in census_summary().items()]
            f.write("{\n" + ",\n".join(lines) + ',\n "census": {\n' + ",\n".join(cen) + "\n }\n}\n")
    for r in bad[:20]:
        print("MISMATCH", r["op"], r["param"], r["shape"], r["variant"], r["index"], flush=True)
    for d in res["dirty"][:20]:
        print("DIRTY SCRATCH", d, flush=True)
    print(f"{len(res['records'])} cases, {len(bad)} mismatches, {len(res['dirty'])} dirty scratch checks, "
          f"{res['seconds']:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
