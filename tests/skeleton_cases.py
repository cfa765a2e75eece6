"""The case table of skeletonize / neighbor_classes: the smallest planes on which the thinning kernel can still go wrong.
Its sizes come from the kernel's geometry (AMT_SKELETON_TILE_ROWS, AMT_SKELETON_TILE_WORDS and the blocking depth T =
AMT_SKELETON_BLOCK_SUBITERS): widths round the 64-pixel word seams and the tile's last word, heights round the tile-row
seams, disks of radius T + 3 on the seams, and a bar 2 T + 6 thick that needs more than one launch.

A case is a stack of planes of one shape that goes through the device in ONE call (every plane has its own iteration
count); ``reference(case)`` gives the planes tests/skeleton_reference.py makes of them, computed once per process.

``python -m tests.skeleton_cases --json PATH`` runs the table and writes a digest per case, whether it equalled the
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
import skeleton_reference as ref  # noqa: E402
from arcadia_microscopy_tools_amd import _hip  # noqa: E402
from poison_child import digest  # noqa: E402

ROWS, WORDS, T = _hip.SKELETON_TILE_ROWS, _hip.SKELETON_TILE_WORDS, _hip.SKELETON_BLOCK_SUBITERS
TILE_W = 64 * WORDS

WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, TILE_W - 1, TILE_W + 1)
HEIGHTS = (1, 2, 3, ROWS - 1, ROWS + 1, 2 * ROWS + 1)
# every width and every height at least once; single-row, single-word and single-pixel planes among them
SHAPES = (
    (1, 1), (2, 2), (3, 63), (1, 64), (2, 65), (3, 127), (ROWS - 1, 128), (ROWS + 1, 129), (2 * ROWS + 1, 65),
    (ROWS - 1, TILE_W - 1), (ROWS + 1, TILE_W + 1), (2 * ROWS + 1, 1), (2 * ROWS + 1, 2), (2, TILE_W + 1), (ROWS - 1, 64),
    (1, TILE_W - 1),
)
assert {s[1] for s in SHAPES} == set(WIDTHS) and {s[0] for s in SHAPES} == set(HEIGHTS)

BAR_THICK = 2 * T + 6
BAR_WIDE = 2 * TILE_W + 6  # wider than two tiles
FRAME = 3
BAR_SHAPE = (BAR_THICK + 2 * FRAME, BAR_WIDE + 2 * FRAME)


def random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _thick_line(shape, thick, dy, dx):
    """The pixels within `thick` steps (along x) of the line through the centre with direction (dy, dx)."""
    H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = H // 2, W // 2
    if dx == 0:  # a column
        d = x - cx
    elif dy == 0:  # a row
        d = y - cy
    else:  # a diagonal: x - cx = +-(y - cy)
        d = (x - cx) - (dx * dy) * (y - cy)
    return ((d >= 0) & (d < thick)).astype(np.uint8)


def contents(shape):
    """(name, plane) of every content of the table on one shape."""
    H, W = shape
    one = np.zeros(shape, np.uint8)
    one[H // 2, W // 2] = 1
    block = np.zeros(shape, np.uint8)
    block[H // 2:H // 2 + 2, W // 2:W // 2 + 2] = 1
    y, x = np.mgrid[0:H, 0:W]
    out = [("ones", np.ones(shape, np.uint8)), ("zeros", np.zeros(shape, np.uint8)), ("one pixel", one), ("2 x 2 block", block)]
    for thick in (1, 2):
        out.append((f"row x{thick}", _thick_line(shape, thick, 0, 1)))
        out.append((f"column x{thick}", _thick_line(shape, thick, 1, 0)))
        out.append((f"diagonal x{thick}", _thick_line(shape, thick, 1, 1)))
        out.append((f"antidiagonal x{thick}", _thick_line(shape, thick, 1, -1)))
    out.append(("checkerboard", ((y + x) & 1).astype(np.uint8)))
    for i, density in enumerate((0.35, 0.65, 0.9)):
        out.append((f"random {density}", random(shape, density, 1000 * H + W + i)))
    return out


def disk(shape, cy, cx, radius):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return ((y - cy) ** 2 + (x - cx) ** 2 <= radius ** 2).astype(np.uint8)


def seam_disks():
    """Three planes: a disk of radius T + 3 on a tile corner, on a tile-row seam and on a word seam."""
    r = T + 3
    shape = (ROWS + r + 5, TILE_W + r + 5)
    return [("disk on a tile corner", disk(shape, ROWS, TILE_W, r)),
            ("disk on a tile-row seam", disk(shape, ROWS, TILE_W // 2 + 20, r)),
            ("disk on a word seam", disk(shape, r + 2, 64 * (WORDS // 2), r))]


def bar_framed():
    p = np.zeros(BAR_SHAPE, np.uint8)
    p[FRAME:FRAME + BAR_THICK, FRAME:FRAME + BAR_WIDE] = 1
    return p


def bar_on_border():
    return np.ones((BAR_THICK, BAR_WIDE), np.uint8)


_CACHE: dict = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bar_history():
    """The framed bar after 0, 1, 2, ... hand-run iterations, up to and including the one that clears nothing."""
    def make():
        planes = [bar_framed()]
        while True:
            nxt, cleared = ref.iteration(planes[-1])
            planes.append(nxt)
            if cleared == 0:
                return planes
    return _memo("bar history", make)


def bar_iterations():
    return len(bar_history()) - 1


def max_iter_values():
    n = bar_iterations()
    return sorted(set(range(1, T // 2 + 3)) | {n - 1, n, n + 1})


def skeleton_cases():
    """-> [(name, max_iter, (N, H, W) uint8 stack, content names)]"""
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
        batch = np.stack([np.zeros(BAR_SHAPE, np.uint8), random(BAR_SHAPE, 0.65, 77), bar_framed()])
        out.append(("batch of three", 0, batch, ("zeros", "random 0.65", "bar")))
        for k in (1, 3, T // 2 + 1):
            out.append((f"batch of three max_iter {k}", k, batch, ("zeros", "random 0.65", "bar")))
        return out
    return _memo("skeleton cases", make)


def class_cases():
    """-> [(name, connectivity, stack, content names)]: random 0.5, a skeleton and all ones (eight set neighbours)"""
    def make():
        out = []
        for shape in SHAPES:
            rnd = random(shape, 0.5, 31 * shape[0] + shape[1])
            skel = ref.skeletonize(random(shape, 0.65, 17 * shape[0] + shape[1]))[0]
            stack = np.stack([rnd, skel, np.ones(shape, np.uint8)])
            for conn in (1, 2):
                out.append((f"classes {shape[0]} x {shape[1]} connectivity {conn}", conn, stack, ("random 0.5", "skeleton", "ones")))
        return out
    return _memo("class cases", make)


def skeleton_reference(case):
    """(planes, iteration counts) of a skeleton case"""
    name, k, stack, _ = case

    def make():
        if name.startswith("bar max_iter"):
            hist = bar_history()
            return hist[min(k, len(hist) - 1)][None], [min(k, len(hist) - 1)]
        res = [ref.skeletonize(p, k) for p in stack]
        return np.stack([r[0] for r in res]), [r[1] for r in res]
    return _memo(("skeleton", name), make)


def class_reference(case):
    name, conn, stack, _ = case
    return _memo(("classes", name), lambda: np.stack([ref.neighbor_classes(p, conn) for p in stack]))


def run_skeleton(ctx, case):
    from arcadia_microscopy_tools_amd import hipops

    return hipops.skeletonize(ctx.asarray(case[2]), case[1]).numpy(dtype=np.uint8)


def run_classes(ctx, case):
    from arcadia_microscopy_tools_amd import hipops

    return hipops.neighbor_classes(ctx.asarray(case[2]), case[1]).numpy(dtype=np.uint8)


def run(ctx, scratch_check=False):
    """Every case once: {name: {"sha256", "equal", "dirty"}}"""
    out = {}
    for cases, runner, reference in ((skeleton_cases(), run_skeleton, lambda c: skeleton_reference(c)[0]),
                                     (class_cases(), run_classes, class_reference)):
        for case in cases:
            got = runner(ctx, case)
            dirty = ctx.scratch_check() if scratch_check else None
            out[case[0]] = {"sha256": digest(got), "equal": bool(np.array_equal(got, reference(case))),
                            "dirty": None if dirty is None else list(dirty)}
    return out


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="the skeleton case table on the device")
    ap.add_argument("--json", required=True)
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison_child.write(args.json, {"cases": run(get_context(), scratch_check=poison_child.poisoned())})
    return 0


if __name__ == "__main__":
    sys.exit(main())
