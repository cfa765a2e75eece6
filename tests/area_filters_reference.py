"""Test-side reference for ``remove_small_objects`` / ``remove_small_holes`` (not collected): ``scipy.ndimage.label`` plus
``np.bincount``, written as the two rules, and the generators of tests/fill_holes_reference.py.

The rules (s = the size, connectivity of the structure: cross = 4-connected, all-ones = 8-connected):
  objects  ``out[p] = in[p] != 0`` and the foreground component of p has at least s pixels;
  holes    ``out[p] = in[p] != 0``, or the background component of p has fewer than s pixels -- frame-touching background
           components included (``~remove_small_objects(~ar, s, connectivity)``, what scikit-image computes).
tests/golden/area_filters.npz (tools/make_golden_area_filters.py, scikit-image 0.18.3) holds scikit-image's own answers
for a few planes; tests/test_host_area_filters.py compares this reference with them.

Nothing here is shared with the library.
"""
from __future__ import annotations

import os

import numpy as np
from scipy import ndimage as ndi

import fill_holes_reference as fh
from fill_holes_reference import (CROSS, FULL, SHAPES, SPIRAL_SHAPES, STRUCTURES, all_one, all_zero,  # noqa: F401
                                  checkerboard, nested, random, seam_holes, spiral, truth_bytes)

OPERATORS = ("objects", "holes")
CONNECTIVITY = {"cross": 1, "full": 2}
SEEDS = (0, 1, 2)
DENSITIES = (0.5, 0.65, 0.8)  # of the random planes, one per seed
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "area_filters.npz")
GOLDEN_SHAPES = [(70, 131), (33, 40), (64, 64)]
GOLDEN_SIZES = (2, 5, 17, 64)


def component_areas(truth, structure) -> np.ndarray:
    """Per pixel: the pixel count of its component of ``truth`` (a bool plane), 0 where ``truth`` is False."""
    truth = np.asarray(truth, bool)
    if truth.size == 0:
        return np.zeros(truth.shape, np.int64)
    lab, _ = ndi.label(truth, structure=np.asarray(structure) != 0)
    return np.bincount(lab.ravel())[lab] * truth


def objects_from_areas(mask, areas, size) -> np.ndarray:
    return ((np.asarray(mask) != 0) & (areas >= size)).astype(np.uint8)


def holes_from_areas(mask, bg_areas, size) -> np.ndarray:
    m = np.asarray(mask) != 0
    return (m | (~m & (bg_areas < size))).astype(np.uint8)


def remove_small_objects(mask, size, structure) -> np.ndarray:
    """Rule "objects" as uint8 0 / 1."""
    m = np.asarray(mask) != 0
    return objects_from_areas(m, component_areas(m, structure), size)


def remove_small_holes(mask, size, structure) -> np.ndarray:
    """Rule "holes" as uint8 0 / 1."""
    m = np.asarray(mask) != 0
    return holes_from_areas(m, component_areas(~m, structure), size)


def apply(op, mask, size, structure) -> np.ndarray:
    return remove_small_objects(mask, size, structure) if op == "objects" else remove_small_holes(mask, size, structure)


class Plane:
    """One plane with its per-pixel component areas of both polarities and both structures, computed once: the answer
    for any size is then two comparisons."""

    def __init__(self, plane):
        self.plane = np.ascontiguousarray(plane, np.uint8)
        m = self.plane != 0
        self.fg = {s: component_areas(m, st) for s, st in STRUCTURES}
        self.bg = {s: component_areas(~m, st) for s, st in STRUCTURES}

    def want(self, op, sname, size) -> np.ndarray:
        if op == "objects":
            return objects_from_areas(self.plane, self.fg[sname], size)
        return holes_from_areas(self.plane, self.bg[sname], size)


def frame_bays(shape):
    """Solid, with small background regions ON the frame (1, 3 and 6 pixels, and a pair that only a diagonal joins) and
    one 4-pixel hole inside: remove_small_holes fills frame-touching regions too, binary_fill_holes never does."""
    H, W = shape
    if H < 12 or W < 12:
        return None
    m = np.ones(shape, np.uint8)
    m[0, 2] = 0                    # 1 pixel on row 0
    m[0:3, 6] = 0                  # 3 pixels from row 0
    m[H - 2:H, W - 4:W - 1] = 0    # 6 pixels on the last row
    m[5, 0] = m[6, 1] = 0          # two pixels joined by a diagonal, the first on column 0
    m[H // 2:H // 2 + 2, W // 2:W // 2 + 2] = 0  # a 4-pixel hole
    return m


def planes(shape):
    """[(name, plane)] for the sweep: the named generators of tests/fill_holes_reference.py that fit ``shape``, and
    ``frame_bays``."""
    out = [(f"random-{s}", random(shape, DENSITIES[i], s)) for i, s in enumerate(SEEDS)]
    out += [("all_zero", all_zero(shape)), ("all_one", all_one(shape)), ("checkerboard", checkerboard(shape))]
    if shape in SPIRAL_SHAPES:
        out.append(("spiral-open", spiral(shape, True)))
    out += [("nested", nested(shape)), ("seam_holes", seam_holes(shape)), ("frame_bays", frame_bays(shape))]
    return [(n, p) for n, p in out if p is not None]


def sweep_sizes(shape):
    return (1, 2, 5, 17, shape[0] * shape[1], shape[0] * shape[1] + 1)


def golden_planes():
    """{name: plane} of the golden file's inputs: a random plane of (70, 131) and of (64, 64), a sparse one of (33, 40),
    and planes with small background regions on the frame."""
    return {"random-70x131": random((70, 131), 0.65, 1), "random-64x64": random((64, 64), 0.5, 0),
            "sparse-33x40": random((33, 40), 0.35, 2), "frame_bays-33x40": frame_bays((33, 40)),
            "frame_bays-64x64": frame_bays((64, 64))}


def blobs_field(size=256, count=10, nblobs=14, seed=5):
    """A four-channel uint16 field whose DAPI channel (index 1) holds ``count`` solid discs (radius 14-18) and ``nblobs``
    small 7 x 7 squares, all well apart: the squares survive an opening with disk(2) but stay far below a disc's area.
    -> (fov, disc centres [(y, x, r)], blob corners [(y, x)])"""
    rng = np.random.default_rng(seed)
    y, x = np.indices((size, size))
    dapi = np.full((size, size), 300.0)
    centres, blobs = [], []
    tries = 0
    while len(centres) < count and tries < 10000:
        tries += 1
        r = int(rng.integers(14, 19))
        cy, cx = rng.integers(r + 4, size - r - 4, 2)
        if all((cy - a) ** 2 + (cx - b) ** 2 > (r + c + 6) ** 2 for a, b, c in centres):
            centres.append((int(cy), int(cx), r))
    while len(blobs) < nblobs and tries < 20000:
        tries += 1
        by, bx = rng.integers(6, size - 13, 2)
        cy, cx = by + 3, bx + 3
        if (all((cy - a) ** 2 + (cx - b) ** 2 > (c + 14) ** 2 for a, b, c in centres)
                and all(abs(by - a) > 16 or abs(bx - b) > 16 for a, b in blobs)):
            blobs.append((int(by), int(bx)))
    for cy, cx, r in centres:
        dapi[np.hypot(y - cy, x - cx) <= r] = 9000.0
    for by, bx in blobs:
        dapi[by:by + 7, bx:bx + 7] = 9000.0
    dapi += rng.normal(0, 40, dapi.shape)
    fov = np.empty((4, size, size), np.uint16)
    for c in range(4):
        fov[c] = np.clip(rng.normal(500, 50, (size, size)), 0, 65535).astype(np.uint16)
    fov[1] = np.clip(dapi, 0, 65535).astype(np.uint16)
    return fov, centres, blobs


assert fh.SEEDS == SEEDS and fh.DENSITIES == DENSITIES
