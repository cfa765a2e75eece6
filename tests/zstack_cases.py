"""The case table of the Z-stack operators (z_project, focus_sums, focus_index, focus_stack, z_take): the smallest stacks on
which the kernels can still go wrong.  The seams come from the focus kernel's tile, ``hipops.zstack_tile()``: planes of
tile - 1, tile and tile + 1 in each direction; beside them an odd, unaligned plane (70 x 131), planes smaller than every
window, single rows and columns, every radius class (0, 1, 4, 15), Z = 1, 2, 5 and 257 (an 8-bit index would fail), both
integer dtypes, float64 for the projections and the gather, a batch of three different stacks, and content chosen to
break narrow arithmetic (a 0 / 65535 checkerboard: L^2 needs 37 bits), the tie rule (equal planes, values in 0..3) and
the point of it all (a planted depth map).

A case is (name, (N, Z, H, W) stack, radius or None); ``reference(case)`` gives what tests/zstack_reference.py makes of it,
computed once per process and left unchanged.

``python -m tests.zstack_cases --json PATH`` runs the table and writes a digest per result, whether it equalled the
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
import zstack_reference as ref  # noqa: E402
from arcadia_microscopy_tools_amd import hipops  # noqa: E402
from poison_child import digest  # noqa: E402

TH, TW = hipops.zstack_tile()
RADII = (0, 1, 4, 15)
ODD = (70, 131)
SEAM_SHAPES = ((TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (TH - 1, TW + 1), (TH + 1, TW - 1))
PLANTED_Z0 = (1, 3, 0)  # the focal plane of the three bands of the planted case


def random_stack(shape, dtype, seed):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(0, int(info.max) + 1, size=shape, dtype=dtype)


def checkerboard_stack(shape, z, where):
    """flat planes of 1000 but plane `where`, a 0 / 65535 checkerboard: |L| reaches 262140 and L^2 2^36"""
    H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    s = np.full((z, H, W), 1000, np.uint16)
    s[where] = (((y + x) & 1) * 65535).astype(np.uint16)
    return s


def box_blur(plane):
    """one pass of the 3 x 3 box mean in integers, edge replication"""
    p = np.pad(plane.astype(np.int64), 1, mode="edge")
    H, W = plane.shape
    return sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) // 9


def planted_z0(shape):
    """the planted focal plane per pixel: piecewise constant in three bands of columns"""
    H, W = shape
    z0 = np.empty(shape, np.int64)
    for b, v in enumerate(PLANTED_Z0):
        z0[:, b * W // 3:(b + 1) * W // 3] = v
    return z0


def planted_stack(shape, z, seed):
    """one sharp texture, blurred per plane by |z - z0(y, x)| passes of the box mean"""
    sharp = random_stack(shape, np.uint16, seed).astype(np.int64)
    levels = [sharp]
    for _ in range(z):
        levels.append(box_blur(levels[-1]))
    levels = np.stack(levels)
    z0 = planted_z0(shape)
    planes = [np.take_along_axis(levels, np.abs(k - z0)[None], axis=0)[0] for k in range(z)]
    return np.stack(planes).astype(np.uint16)


_CACHE: dict = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def cases():
    """-> [(name, (N, Z, H, W) stack, radius or None for float64 stacks)]"""
    def make():
        out = []
        seed = 100
        for shape in SEAM_SHAPES:
            seed += 1
            out.append((f"seam {shape[0]} x {shape[1]} r 4", random_stack((1, 2) + shape, np.uint16, seed), 4))
        out.append((f"seam {TH + 1} x {TW + 1} r 15", random_stack((1, 2, TH + 1, TW + 1), np.uint16, 120), 15))
        out.append((f"seam {TH} x {TW} uint8 r 1", random_stack((1, 2, TH, TW), np.uint8, 121), 1))
        for r in RADII:
            out.append((f"odd 70 x 131 Z 5 r {r}", random_stack((1, 5) + ODD, np.uint16, 130 + r), r))
            out.append((f"small 3 x 5 r {r}", random_stack((1, 2, 3, 5), np.uint16, 140 + r), r))
            out.append((f"pixel 1 x 1 r {r}", random_stack((1, 2, 1, 1), np.uint16, 150 + r), r))
        out.append(("odd 70 x 131 uint8 r 4", random_stack((1, 5) + ODD, np.uint8, 160), 4))
        for r in (1, 4):
            out.append((f"row 1 x 131 r {r}", random_stack((1, 2, 1, 131), np.uint16, 170 + r), r))
            out.append((f"column 70 x 1 r {r}", random_stack((1, 2, 70, 1), np.uint16, 180 + r), r))
        out.append(("Z 1 9 x 11", random_stack((1, 1, 9, 11), np.uint16, 190), 1))
        out.append(("Z 257 9 x 11", deep_stack(np.uint16, 191)[None], 1))
        out.append(("Z 257 9 x 11 uint8", deep_stack(np.uint8, 192)[None], 1))
        out.append(("batch of three", random_stack((3, 3) + ODD, np.uint16, 193), 4))
        for r in (4, 15):
            out.append((f"checkerboard r {r}", checkerboard_stack(ODD, 3, 1)[None], r))
        out.append(("equal planes", np.repeat(random_stack((1, 1, 40, 40), np.uint16, 194), 4, axis=1), 1))
        out.append(("ties 0..3", tie_stack()[None], 1))
        out.append(("planted depth map", planted_stack(ODD, 5, 195)[None], 4))
        rng = np.random.default_rng(196)
        out.append(("float64 70 x 131", rng.standard_normal((2, 5) + ODD) * 1e3, None))
        out.append((f"float64 {TH} x {TW}", rng.random((1, 3, TH, TW)), None))
        out.append(("float64 3 x 5", rng.random((1, 2, 3, 5)), None))
        return out
    return _memo("cases", make)


def deep_stack(dtype, seed):
    """257 planes of 9 x 11 with the top bits cleared, but the right part of the last plane: index 256 wins there"""
    s = random_stack((257, 9, 11), dtype, seed) >> 4
    s[256, :, 4:] = random_stack((9, 7), dtype, seed + 1000)
    return s


def tie_stack():
    """values in 0..3 on 40 x 40, Z = 4: E is small enough for tied maxima"""
    return (random_stack((4, 40, 40), np.uint16, 197) & 3).astype(np.uint16)


def take_index(case):
    """the index map of the case's z_take: random, reaching two planes past the stack (clamped)"""
    name, stack, _ = case
    N, Z, H, W = stack.shape
    return _memo(("take index", name), lambda: np.random.default_rng(len(name)).integers(0, Z + 2, size=(N, H, W)).astype(np.uint16))


def reference(case):
    """{result name: array} of a case: "max", "min", "mean", "take" and, for integer stacks, "sums", "index", "stack\""""
    name, stack, r = case

    def make():
        out = {m: np.stack([ref.z_project(s, m) for s in stack]) for m in ("max", "min", "mean")}
        out["take"] = np.stack([ref.z_take(s, i) for s, i in zip(stack, take_index(case))])
        if r is not None:
            out["sums"] = np.stack([ref.focus_sums(s) for s in stack])
            out["index"] = np.stack([ref.focus_index(s, r) for s in stack])
            out["stack"] = np.stack([ref.z_take(s, i) for s, i in zip(stack, out["index"])])
        return out
    return _memo(("reference", name), make)


def run_case(ctx, case, check=None):
    """{result name: array} of a case on the device; ``check`` is called after every operator"""
    name, stack, r = case
    d = ctx.asarray(stack)
    check = check or (lambda: None)
    out = {}
    for m in ("max", "min", "mean"):
        out[m] = hipops.z_project(d, m).numpy()
        check()
    out["take"] = hipops.z_take(d, ctx.asarray(take_index(case))).numpy()
    check()
    if r is not None:
        out["sums"] = hipops.focus_sums(d).numpy()
        check()
        out["index"] = hipops.focus_index(d, r).numpy()
        check()
        out["stack"] = hipops.focus_stack(d, r).numpy()
        check()
    return out


def run(ctx, scratch_check=False):
    """Every case once: {"case / result": {"sha256", "equal", "dirty"}}; the last entry is the smoothed composite of the
    planted case through ``operations`` (its median reserves scratch)"""
    from arcadia_microscopy_tools_amd import operations

    out = {}
    for case in cases():
        dirty = []

        def check():
            if scratch_check:
                found = ctx.scratch_check()
                if found is not None:
                    dirty.append(list(found))
        got = run_case(ctx, case, check)
        want = reference(case)
        assert set(got) == set(want)
        for key, arr in got.items():
            out[f"{case[0]} / {key}"] = {"sha256": digest(arr), "equal": bool(arr.dtype == want[key].dtype
                                                                              and np.array_equal(arr, want[key])),
                                         "dirty": dirty[:1] or None}
    planted = [c for c in cases() if c[0] == "planted depth map"][0][1][0]
    got = operations.extended_depth_of_field(planted, radius=4, smooth=3)
    found = ctx.scratch_check() if scratch_check else None
    out["planted depth map / edf smooth 3"] = {
        "sha256": digest(got), "equal": bool(np.array_equal(got, ref.extended_depth_of_field(planted, 4, 3)[0])),
        "dirty": None if found is None else [list(found)]}
    return out


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="the Z-stack case table on the device")
    ap.add_argument("--json", required=True)
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison_child.write(args.json, {"cases": run(get_context(), scratch_check=poison_child.poisoned())})
    return 0


if __name__ == "__main__":
    sys.exit(main())
