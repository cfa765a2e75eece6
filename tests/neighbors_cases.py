"""The case list of tests/test_gpu_neighbors.py: label planes (and companion label planes) on the small shapes of the
relate tests, each run three ways through ``hipops.neighbor_census`` and ``hipops.nearest_labels`` and compared bit for
bit with tests/neighbors_reference.py.

``python -m tests.neighbors_cases --json FILE`` runs the whole list in a process of its own (the test starts it with
AMT_DEBUG_POISON=1), calls ``Context.scratch_check()`` after every call and writes digests, mismatches and dirty checks.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import neighbors_reference as nr  # noqa: E402
import poison_child  # noqa: E402
from relate_cases import BIG, SHAPES, _partners, blobs, overflow_shape  # noqa: E402,F401

LATTICE_SHAPE = (16, 16)


def voronoi(shape, seed: int, count: int) -> np.ndarray:
    """Every pixel to its nearest of ``count`` random centres: no background."""
    rng = np.random.RandomState(seed)
    H, W = shape
    cy, cx = rng.uniform(0, H, count), rng.uniform(0, W, count)
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.argmin((yy[..., None] - cy) ** 2 + (xx[..., None] - cx) ** 2, axis=-1) + 1).astype(np.int32)


def checkerboard(shape) -> np.ndarray:
    """Label 1 on the pixels with even y + x: every other pixel is on its ring."""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return ((yy + xx) % 2 == 0).astype(np.int32)


def capacity_values(kind: str, d: int, rng) -> np.ndarray:
    P = _partners()
    if kind == "random":  # d distinct values over the whole range, its upper end among them
        vals = np.unique(rng.randint(3, BIG, 4 * d).astype(np.int64))[:d]
        vals[0], vals[-1] = 3, BIG
    else:  # every value has the same home slot
        vals = 5 + P * np.arange(d, dtype=np.int64) * 3
    assert len(np.unique(vals)) == d and vals.min() >= 3
    return vals


_CASES: dict = {}


def cases(shape):
    """name -> (labels, companion or None, max_label) int32 planes of ``shape``; None: the labels are their own
    companion, handed over as the same buffer.  Built once per shape."""
    if shape in _CASES:
        return _CASES[shape]
    H, W = shape
    n = H * W
    P = _partners()
    seed = 1000 * H + W
    rng = np.random.RandomState(seed)
    count = max(1, min(12, n // 8))
    out = {}
    a = blobs(shape, seed, count, 2.0 + min(H, W) / 5.0)
    out["blobs"] = (a, None, count)
    out["voronoi"] = (voronoi(shape, seed + 2, count), None, count)
    out["gaps"] = (a * 3, None, 3 * count + 2)  # only every third number is present, the last two absent as well
    out["pieces"] = (rng.randint(0, 4, shape).astype(np.int32), None, 3)  # every label in many pieces
    # labels outside 1..4 are never measured; the positive ones are neighbours
    out["out_of_range_labels"] = (rng.randint(-2, 9, shape).astype(np.int32), None, 4)
    lab = np.zeros(shape, np.int32)
    lab[:, 0] = 1  # a box one column wide
    lab[0, 1:] = 2  # a box one row high, wider than 64 columns on the two widest shapes
    lab[H // 2:, W // 2:] = 3
    out["column_and_row"] = (lab, None, 3)
    out["full_plane"] = (np.ones(shape, np.int32), None, 2)  # no ring; label 2 is absent
    out["zero_companion"] = (a, np.zeros(shape, np.int32), count)
    board = checkerboard(shape)
    special = np.array([1, 2, BIG, P, 2 * P, 3 * P, P + 1, 2 * P + 1, BIG - P, BIG - 2 * P, 1 + 5 * P, 0, -7], np.int64)
    out["special_values"] = (board, special[rng.randint(0, len(special), shape)].astype(np.int32), 1)
    ring = int((board == 0).sum())
    if ring >= 2:  # 9 and 3 on equally many ring pixels, 7 on the odd one left: 3 wins
        vals = np.concatenate([np.tile([9, 3], ring // 2), [7] * (ring % 2)])
        comp = np.full(shape, 11, np.int32)  # under the label itself: never looked at
        comp[board == 0] = vals
        out["main_ties"] = (board, comp, 1)
    if shape == LATTICE_SHAPE:
        lab = np.zeros(shape, np.int32)
        for i in range(3):
            for j in range(3):
                lab[5 * i + 1:5 * i + 3, 5 * j + 1:5 * j + 3] = 3 * i + j + 1  # equal squares, centroids 5 apart
        out["lattice"] = (lab, None, 9)
        lab = np.zeros(shape, np.int32)
        lab[3:6, 4:9] = 2
        out["one_label"] = (lab, None, 3)
        lab = lab.copy()
        lab[10:12, 1:3] = 3
        out["two_labels"] = (lab, None, 3)
    if shape == overflow_shape():
        for d in (P - 1, P, P + 1, 4 * P):
            for kind in ("random", "congruent"):
                vals = capacity_values(kind, d, rng)
                # label 1 holds the even rows: the odd rows are its ring and carry exactly the d values.  Label 2 is two
                # pixels of row 1 with three of the values beside them in that row: both paths in one launch
                lab = np.zeros(shape, np.int32)
                lab[0::2] = 1
                lab[1, 1] = lab[1, 4] = 2
                slots = (H // 2) * W
                rest = np.concatenate([vals[3:], vals[rng.randint(0, d, slots - 4 - (d - 3))]])
                rng.shuffle(rest)
                odd = np.zeros((H // 2, W), np.int64)
                free = np.ones((H // 2, W), bool)
                for x, v in ((0, vals[0]), (2, vals[1]), (3, vals[2]), (5, vals[0])):
                    odd[0, x] = v
                    free[0, x] = False
                odd[free] = rest
                comp = np.zeros(shape, np.int32)
                comp[1::2] = odd
                out[f"{kind}_{d}_neighbors"] = (lab, comp, 2)
    _CASES[shape] = out
    return out


_REF: dict = {}


def reference(shape, name, max_label=None):
    """((max_label, 4) int64 census columns, (max_label, 4) float64 nearest columns) of the case; computed once and
    shared."""
    a, b, k = cases(shape)[name]
    k = k if max_label is None else max_label
    key = (shape, name, k)
    if key not in _REF:
        _REF[key] = (nr.census_columns(a, a if b is None else b, k), nr.nearest_columns(a, k))
    return _REF[key]


BATCH = ("blobs", "voronoi", "zero_companion")  # typical / no background / all-zero companion


def run(ctx, shapes=None, check=False):
    """Every case of ``shapes`` three ways, census and nearest -> {"records": [{"key", "sha256", "ok"}], "dirty":
    [...]}.  ``check``: call ``ctx.scratch_check()`` after every operator call."""
    from arcadia_microscopy_tools_amd import hipops

    records, dirty = [], []

    def call(key, what, labels, k, comp=None):
        if what == "census":
            t = hipops.neighbor_census(labels, k, comp).numpy()
        else:
            t = hipops.nearest_labels(labels, k).numpy()
        if check:
            bad = ctx.scratch_check()
            if bad is not None:
                dirty.append([list(key), list(bad)])
        return t

    def record(key, got, want):
        ok = (got.shape == want.shape and got.dtype == np.float64
              and np.array_equal(got, want.astype(np.float64), equal_nan=True))
        records.append({"key": list(key), "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest(),
                        "ok": bool(ok)})

    for shape in shapes or SHAPES:
        for name, (a, b, k) in cases(shape).items():
            census, nearest = reference(shape, name)
            la = ctx.asarray(a)
            lb = None if b is None else ctx.asarray(b)
            record((shape, name, "census", "single"), call((shape, name, "census"), "census", la, k, lb)[0, :, 0, :], census)
            record((shape, name, "nearest", "single"), call((shape, name, "nearest"), "nearest", la, k)[0, :, 0, :], nearest)
            # plane 1 of a two-plane stack: the base pointers are H * W * 4 bytes past an allocation's
            la = ctx.asarray(np.stack([np.roll(a, 1, axis=1), a]))
            lb = None if b is None else ctx.asarray(np.stack([np.roll(b, 1, axis=0), b]))[1]
            record((shape, name, "census", "plane1"),
                   call((shape, name, "census", "plane1"), "census", la[1], k, lb)[0, :, 0, :], census)
            record((shape, name, "nearest", "plane1"),
                   call((shape, name, "nearest", "plane1"), "nearest", la[1], k)[0, :, 0, :], nearest)
        k = max(cases(shape)[name][2] for name in BATCH)
        planes = [cases(shape)[name] for name in BATCH]
        la = ctx.asarray(np.stack([c[0] for c in planes]))
        lb = ctx.asarray(np.stack([c[0] if c[1] is None else c[1] for c in planes]))
        census = call((shape, "batch", "census"), "census", la, k, lb)
        nearest = call((shape, "batch", "nearest"), "nearest", la, k)
        for i, name in enumerate(BATCH):
            want = reference(shape, name, k)
            record((shape, name, "census", "batch"), census[i, :, 0, :], want[0])
            record((shape, name, "nearest", "batch"), nearest[i, :, 0, :], want[1])
    return {"records": records, "dirty": dirty}


def main(argv):
    from arcadia_microscopy_tools_amd.device import get_context

    out = argv[argv.index("--json") + 1]
    poison_child.write(out, run(get_context(), check=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
