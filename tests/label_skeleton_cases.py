"""The case table of label_skeleton / label_census: the smallest label planes on which the label-aware thinning and the
census can still go wrong.  Sizes come from the kernel's geometry (AMT_LABEL_SKELETON_TILE_ROWS, _TILE_WORDS and the blocking
depth T = AMT_LABEL_SKELETON_BLOCK_SUBITERS) and reuse tests/skeleton_cases.py's shapes for the seams: widths round the
64-pixel word seams and the tile's last word, heights round the tile-row seams.  The contents put the borders BETWEEN
labels on those seams, where a link bit of one word decides about a pixel of the next.

A case is a stack of int32 planes of one shape that goes through the device in ONE call; ``skeleton_reference(case)``
gives the planes and iteration counts rule (a) of tests/label_skeleton_reference.py makes of them, computed once per process.

``python -m tests.label_skeleton_cases --json PATH`` runs the table and writes a digest per case, whether it equalled the
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

import label_skeleton_reference as ref  # noqa: E402
import poison_child  # noqa: E402
import skeleton_cases as binary_cases  # noqa: E402
from arcadia_microscopy_tools_amd import _hip  # noqa: E402
from poison_child import digest  # noqa: E402

ROWS, WORDS, T = _hip.LABEL_SKELETON_TILE_ROWS, _hip.LABEL_SKELETON_TILE_WORDS, _hip.LABEL_SKELETON_BLOCK_SUBITERS
TILE_W = 64 * WORDS

# the binary table's shapes are made of the binary geometry; they are the label kernel's seams while the two agree
assert (ROWS, WORDS, T) == (binary_cases.ROWS, binary_cases.WORDS, binary_cases.T)
SHAPES = binary_cases.SHAPES
assert {s[1] for s in SHAPES} == {1, 2, 63, 64, 65, 127, 128, 129, TILE_W - 1, TILE_W + 1}
assert {s[0] for s in SHAPES} == {1, 2, 3, ROWS - 1, ROWS + 1, 2 * ROWS + 1}

HALF_THICK = 2 * T + 6          # one label of the bar: deeper than one launch of T sub-iterations reaches
BAR_THICK = 2 * HALF_THICK
BAR_WIDE = 2 * TILE_W + 6       # wider than two tiles
FRAME = 3
BAR_SHAPE = (BAR_THICK + 2 * FRAME, BAR_WIDE + 2 * FRAME)
EXOTIC = (2**31 - 1, -5, 1 << 20)  # label values that show that equality alone decides


def voronoi(shape, seeds, seed, holes=0.02):
    """`seeds` touching cells with labels 1..seeds (nearest seed point), `holes` of the pixels cleared"""
    rng = np.random.default_rng(seed)
    H, W = shape
    sy, sx = rng.integers(0, H, seeds), rng.integers(0, W, seeds)
    y, x = np.mgrid[0:H, 0:W]
    d = (y[None] - sy[:, None, None]) ** 2 + (x[None] - sx[:, None, None]) ** 2
    lab = (np.argmin(d, axis=0) + 1).astype(np.int32)
    lab[rng.random(shape) < holes] = 0
    return lab


def noise(shape, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, 4, shape), 0).astype(np.int32)


def _stripes(n):
    """labels 1, 2, 3 along an axis of n pixels, 1, 2 and 3 pixels wide"""
    return np.array([1, 2, 2, 3, 3, 3], np.int32)[np.arange(n) % 6]


def contents(shape):
    """(name, int32 plane) of every content of the table on one shape."""
    H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    vor = voronoi(shape, 12, 100 * H + W)
    exotic = vor.copy()
    for k, value in enumerate(EXOTIC):
        exotic[vor == k + 1] = value
    return [
        ("one label 7", np.full(shape, 7, np.int32)),
        ("zeros", np.zeros(shape, np.int32)),
        ("split on x = 64", np.where(x < 64, 1, 2).astype(np.int32)),
        ("split on the tile's last word", np.where(x < TILE_W - 64, 1, 2).astype(np.int32)),
        ("split on y = ROWS", np.where(y < ROWS, 1, 2).astype(np.int32)),
        ("stripe rows", np.broadcast_to(_stripes(H)[:, None], shape).astype(np.int32)),
        ("stripe columns", np.broadcast_to(_stripes(W)[None, :], shape).astype(np.int32)),
        ("checkerboard", (((y + x) & 1) + 1).astype(np.int32)),
        ("voronoi", vor),
        ("voronoi, exotic values", exotic),
        ("noise 0..3", noise(shape, 0.65, 1000 * H + W)),
    ]


def seam_disks():
    """Three planes: a disk of radius T + 3 cut into two labels along a tile corner (by the diagonal through it), along a
    tile-row seam and along a word seam."""
    r = T + 3
    shape = (ROWS + r + 5, TILE_W + r + 5)
    y, x = np.mgrid[0:shape[0], 0:shape[1]]

    def cut(cy, cx, second):
        return np.where(binary_cases.disk(shape, cy, cx, r) != 0, np.where(second, 2, 1), 0).astype(np.int32)

    return [("disk cut on a tile corner", cut(ROWS, TILE_W, (y - ROWS) > (x - TILE_W))),
            ("disk cut on a tile-row seam", cut(ROWS, TILE_W // 2 + 20, y >= ROWS)),
            ("disk cut on a word seam", cut(r + 2, 64 * (WORDS // 2), x >= 64 * (WORDS // 2)))]


def bar_on_border():
    p = np.ones((BAR_THICK, BAR_WIDE), np.int32)
    p[HALF_THICK:] = 2
    return p


def bar_framed():
    p = np.zeros(BAR_SHAPE, np.int32)
    p[FRAME:FRAME + BAR_THICK, FRAME:FRAME + BAR_WIDE] = bar_on_border()
    return p


_CACHE: dict = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bar_history():
    """The framed bar after 0, 1, 2, ... hand-run iterations of rule (a), up to and including the one that clears nothing."""
    def make():
        planes = [bar_framed()]
        while True:
            nxt, cleared = ref.iteration(planes[-1])
            planes.append(nxt.astype(np.int32))
            if cleared == 0:
                return planes
    return _memo("bar history", make)


def bar_iterations():
    return len(bar_history()) - 1


def max_iter_values():
    n = bar_iterations()
    return sorted(set(range(1, T // 2 + 3)) | {n - 1, n, n + 1})


def batch_of_three():
    return np.stack([np.zeros(BAR_SHAPE, np.int32), noise(BAR_SHAPE, 0.65, 77), bar_framed()])


def skeleton_cases():
    """-> [(name, max_iter, (N, H, W) int32 stack, content names)]"""
    def make():
        out = []
        for shape in SHAPES:
            names, planes = zip(*contents(shape))
            out.append((f"contents {shape[0]} x {shape[1]}", 0, np.stack(planes), names))
        names, planes = zip(*seam_disks())
        out.append(("seam disks", 0, np.stack(planes), names))
        out.append(("bar in a frame", 0, bar_framed()[None], ("bar",)))
        out.append(("bar on the border", 0, bar_on_border()[None], ("bar",)))
        for k in max_iter_values():
            out.append((f"bar max_iter {k}", k, bar_framed()[None], ("bar",)))
        out.append(("batch of three", 0, batch_of_three(), ("zeros", "noise 0..3", "bar")))
        for k in (1, 3, T // 2 + 1):
            out.append((f"batch of three max_iter {k}", k, batch_of_three(), ("zeros", "noise 0..3", "bar")))
        return out
    return _memo("skeleton cases", make)


def skeleton_reference(case):
    """(planes, iteration counts) of a skeleton case by rule (a)"""
    name, k, stack, _ = case

    def make():
        if name.startswith("bar max_iter"):
            hist = bar_history()
            return hist[min(k, len(hist) - 1)][None], [min(k, len(hist) - 1)]
        res = [ref.skeletonize(p, k) for p in stack]
        return np.stack([r[0] for r in res]), [r[1] for r in res]
    return _memo(("skeleton", name), make)


def l_and_staircase():
    """Three pixels each, label 1 the L, label 2 the pure diagonal, label 3 the staircase of an L on a diagonal"""
    p = np.zeros((9, 12), np.int32)
    p[1, 1] = p[2, 1] = p[2, 2] = 1  # two orthogonal links; the diagonal (1, 1) - (2, 2) is bridged: not counted
    p[5, 5] = p[6, 6] = p[7, 7] = 2  # two diagonal links
    p[1, 8] = p[1, 9] = p[2, 10] = 3  # one orthogonal, one diagonal
    return p


# pixels, isolated, ends, path, junctions, orth_links, diag_links -- worked out by hand: every pixel of the L has two
# neighbours of its label
HAND_TABLE = np.array([[3, 0, 0, 3, 0, 2, 0], [3, 0, 2, 1, 0, 0, 2], [3, 0, 2, 1, 0, 1, 1]], np.int32)


def census_cases():
    """-> [(name, max_label, (N, H, W) int32 stack, content names)]: the reference skeletons of the skeleton cases with
    max_label below, at and above the largest small label; a plane of one label (deg = 8); the hand cases"""
    def make():
        out = []
        for case in skeleton_cases():
            if case[1] != 0 or case[0] == "bar on the border":
                continue
            stack = skeleton_reference(case)[0]
            largest = int(stack[(stack > 0) & (stack < 100)].max(initial=1))
            for m in sorted({largest - 1, largest, largest + 2}):
                out.append((f"census of {case[0]}, max_label {m}", m, stack, case[3]))
        one = np.stack([np.ones((5, 70), np.int32), np.full((5, 70), 2, np.int32)])
        out.append(("census of one label everywhere", 2, one, ("label 1", "label 2")))
        out.append(("census of the L and the staircases", 3, l_and_staircase()[None], ("hand",)))
        out.append(("census of raw voronoi cells", 12, np.stack([voronoi((ROWS + 1, 129), 12, 5)]), ("voronoi",)))
        return out
    return _memo("census cases", make)


def census_reference(case):
    name, m, stack, _ = case
    return _memo(("census", name), lambda: np.stack([ref.census(p, m) for p in stack]).reshape(len(stack), m, 7))


def run_skeleton(ctx, case):
    from arcadia_microscopy_tools_amd import hipops

    return hipops.label_skeleton(ctx.asarray(case[2]), case[1]).numpy()


def run_census(ctx, case):
    from arcadia_microscopy_tools_amd import hipops

    return hipops.label_census(ctx.asarray(case[2]), case[1]).numpy()


def run(ctx, scratch_check=False):
    """Every case once: {name: {"sha256", "equal", "dirty"}}"""
    out = {}
    for cases, runner, reference in ((skeleton_cases(), run_skeleton, lambda c: skeleton_reference(c)[0]),
                                     (census_cases(), run_census, census_reference)):
        for case in cases:
            got = runner(ctx, case)
            dirty = ctx.scratch_check() if scratch_check else None
            out[case[0]] = {"sha256": digest(got), "equal": bool(np.array_equal(got, reference(case))),
                            "dirty": None if dirty is None else list(dirty)}
    return out


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="the label skeleton case table on the device")
    ap.add_argument("--json", required=True)
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison_child.write(args.json, {"cases": run(get_context(), scratch_check=poison_child.poisoned())})
    return 0


if __name__ == "__main__":
    sys.exit(main())
