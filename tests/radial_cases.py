"""The case table of the radial distribution (AMT_RPX_RADIAL), shared by tests/test_host_radial.py and
tests/test_gpu_radial.py: the smallest label planes at which the kernel can still go wrong, each with its uint16
(C, Y, X) stack (None for C = 0), its max_label and its bins.  The float64 stack of a case is its uint16 stack divided
by 7 (zero stays zero).  The reference of a case (tests/radial_reference.py) is computed once and shared."""
from __future__ import annotations

import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import poison_child  # noqa: E402
import radial_reference as rr  # noqa: E402

KINDS = ("u16", "f64")
WIDTHS = (8, 9, 16, 17, 32, 33, 64, 65)  # the four lane layouts of amt_box_layout and the first second tile
RTOL, ATOL = 1e-9, 1e-12  # the project's bound for float64 per-label sums


def lds_tile() -> int:
    """RD_LDS_TILE of amt_radial.hip: the cells of a bounding box that is kept in LDS; a larger box goes through scratch"""
    src = open(os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc", "amt_radial.hip")).read()
    found = re.findall(r"constexpr int (RD_\w*TILE\w*) = (\d+);", src)
    assert [name for name, _ in found] == ["RD_LDS_TILE"], found  # the one box-size tier constant of the kernel
    return int(found[0][1])


def tier_radii():
    """(r_in, r_out): the largest disk whose (2 r + 1)^2 box is kept in LDS, and the next one"""
    r_in = (math.isqrt(lds_tile()) - 1) // 2
    assert (2 * r_in + 1) ** 2 <= lds_tile() < (2 * r_in + 3) ** 2
    return r_in, r_in + 1


def disk(shape, cy, cx, r2, label=1):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return np.where((yy - cy) ** 2 + (xx - cx) ** 2 <= r2, label, 0).astype(np.int32)


def _images(shape, C, seed):
    """C uint16 channels: a smooth one, a radial one, noise over the whole range (both ends present)"""
    if C == 0:
        return None
    rng = np.random.RandomState(seed)
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = ((0.5 + 0.3 * np.sin(yy / 3.1) * np.cos(xx / 4.3) + 0.2 * rng.uniform(-1, 1, shape)) * 40000).astype(np.uint16)
    radial = (np.hypot(yy - H / 2.0, xx - W / 2.0) * 300 + 50).astype(np.uint16)
    noise = rng.randint(0, 65536, shape).astype(np.uint16)
    noise.flat[0], noise.flat[-1] = 0, 65535
    return np.ascontiguousarray(np.stack([smooth, radial, noise][:C]))


def _case(lab, k, bins=4, C=1, stack=None, seed=0):
    lab = np.ascontiguousarray(lab, np.int32)
    if stack is None:
        stack = _images(lab.shape, C, seed + 31 * lab.shape[0] + lab.shape[1])
    return {"lab": lab, "k": int(k), "bins": int(bins), "stack": stack}


_CASES: dict = {}


def cases() -> dict:
    """name -> {"lab": (Y, X) int32, "k": max_label, "bins", "stack": (C, Y, X) uint16 or None}"""
    if _CASES:
        return _CASES
    out = _CASES
    z = lambda H, W: np.zeros((H, W), np.int32)  # noqa: E731
    lab = z(7, 5)
    lab[3, 2] = 1
    out["single_pixel"] = _case(lab, 1)
    out["fills_plane"] = _case(np.ones((7, 5)), 1, C=3)
    lab = z(9, 11)
    lab[0:4, 0:5] = 1
    lab[5:9, 7:11] = 2
    out["corners"] = _case(lab, 2)
    lab = z(9, 11)
    lab[2:7, 0:4] = 1      # the left border
    lab[0:3, 5:10] = 2     # the top border
    lab[6:9, 6:9] = 3      # the bottom border
    out["one_border"] = _case(lab, 3, C=3)
    lab = z(9, 12)
    lab[2:7, 1:6] = 1
    alone = lab.copy()
    lab[2:7, 6:11] = 2     # shares the edge x = 5 | 6
    out["shared_edge"] = _case(lab, 2)
    out["shared_edge_alone"] = _case(alone, 1, stack=out["shared_edge"]["stack"])
    lab = z(9, 14)
    lab[2:7, 1:5] = 1
    lab[2:7, 7:12] = 1     # two pieces, two pixels apart
    out["two_pieces"] = _case(lab, 1)
    lab = z(9, 9)
    lab[1:8, 1:8] = 1
    lab[4, 4] = 0          # a one-pixel hole
    out["hole"] = _case(lab, 1)
    out["annulus"] = _case(disk((21, 21), 10, 10, 81) - disk((21, 21), 10, 10, 16), 1, C=3)
    lab = z(12, 13)        # a U: the nearest outside pixel of (8, 4) lies diagonally, at (6, 6)
    lab[1:11, 1:12] = 1
    lab[1:7, 6] = 0
    out["u_shape"] = _case(lab, 1)
    for w in WIDTHS:
        lab = z(7, 70)
        lab[2:5, 3:3 + w] = 1
        out[f"width_{w}"] = _case(lab, 1)
    lab = z(70, 7)
    lab[2:67, 2:5] = 1
    out["tall_65x3"] = _case(lab, 1)
    # ---- one disk on either side of the box-size tier
    r_in, r_out = tier_radii()
    side = 2 * r_out + 5
    for name, r in (("tier_in", r_in), ("tier_out", r_out)):
        out[f"disk_{name}"] = _case(disk((side, side + 3), r_out + 2, r_out + 3, r * r), 1, C=3)
    lab = z(side, 2 * side)  # two labels past the tier that share an edge, each cut by three borders
    lab[:, :side] = 1
    lab[:, side:] = 2
    out["tier_out_touching"] = _case(lab, 2, C=2)
    # ---- ring ties a float rule gets wrong
    out["tie_disk17_bins3"] = _case(disk((11, 11), 5, 5, 17), 1, bins=3)
    out["tie_disk20_bins5"] = _case(disk((11, 11), 5, 5, 20), 1, bins=5)
    lab = z(11, 11)
    lab[1:10, 1:10] = 1
    out["tie_square9_bins5"] = _case(lab, 1, bins=5)
    # ---- wedge ties: odd symmetric shapes have pixels on the centroid's row, column and diagonals
    out["wedge_ties_disk"] = _case(disk((15, 15), 7, 7, 36), 1, bins=2, C=3)
    lab = z(9, 9)
    lab[2:7, 2:7] = 1
    out["wedge_ties_square"] = _case(lab, 1, bins=1)
    # ---- channel values
    lab = z(8, 9)
    lab[1:7, 1:8] = 1
    stack = _images((8, 9), 3, 5)
    stack[1] = 0
    out["zero_channel"] = _case(lab, 1, stack=stack)
    rect = int(math.isqrt(lds_tile()))
    lab = z(rect + 2, rect + 6)
    lab[1:rect + 1, 2:rect + 2] = 1
    out["full_scale_square"] = _case(lab, 1, stack=np.full((1,) + lab.shape, 65535, np.uint16))
    lab = z(rect + 2, rect + 6)
    lab[1:rect + 1, 2:rect + 3] = 1   # one column more: past the tier
    out["full_scale_square_plus"] = _case(lab, 1, stack=np.full((1,) + lab.shape, 65535, np.uint16))
    # ---- bins, channels, absent rows
    blob = disk((24, 30), 8, 9, 49) + disk((24, 30), 15, 20, 36, label=3) * (disk((24, 30), 8, 9, 49) == 0)
    for bins in (1, 4, 16):
        for C in (0, 1, 3):
            out[f"bins_{bins}_channels_{C}"] = _case(blob, 5, bins=bins, C=C)  # labels 2, 4 and 5 are absent
    # ---- twenty random planes with touching cells
    from arcadia_microscopy_tools_amd.synth import synthetic_flows

    for seed in range(20):
        truth = synthetic_flows((48, 64), 10, seed=seed)[2]
        out[f"random_{seed:02d}"] = _case(truth, 11, bins=(4, 3, 7)[seed % 3], C=(1, 2, 3)[seed % 3], seed=seed)
    return out


def stack_of(case, kind):
    s = case["stack"]
    if s is None or kind == "u16":
        return s
    return s.astype(np.float64) / 7.0


_REF: dict = {}


def reference(name, kind="u16"):
    """(geometry (k, GEOM_NCOLS), table (k, C, bins, 3) or None) of a case, computed once"""
    if (name, kind) not in _REF:
        c = cases()[name]
        _REF[(name, kind)] = rr.radial_stack(c["lab"], stack_of(c, kind), c["k"], c["bins"])
    return _REF[(name, kind)]


def run(ctx, names=None, check_scratch=False):
    """Every case (both element types) through ``hipops.radial_distribution`` on ``ctx`` -> {"records": [{"key", "ok",
    "sha256"}], "dirty": [...]}: ok = equal to the reference as tests/test_gpu_radial.py asks, sha256 of the two outputs'
    bytes; with ``check_scratch`` ``Context.scratch_check()`` runs after every call (AMT_DEBUG_POISON=1)."""
    import hashlib

    from arcadia_microscopy_tools_amd import hipops

    records, dirty = [], []
    for name, c in cases().items():
        if names is not None and name not in names:
            continue
        for kind in KINDS:
            stack = stack_of(c, kind)
            if stack is None and kind == "f64":
                continue
            geom, table = hipops.radial_distribution(ctx.asarray(c["lab"][None]),
                                                     None if stack is None else ctx.asarray(stack[None]), c["k"],
                                                     bins=c["bins"])
            if check_scratch:
                bad = ctx.scratch_check()
                if bad is not None:
                    dirty.append([name, kind, list(bad)])
            g = geom.numpy()[0]
            t = None if table is None else table.numpy()[0]
            want_g, want_t = reference(name, kind)
            ok = same_bits(g, want_g) and (t is None or (same_bits if kind == "u16" else close)(t, want_t))
            digest = hashlib.sha256(g.tobytes() + (b"" if t is None else t.tobytes())).hexdigest()
            records.append({"key": [name, kind], "ok": bool(ok), "sha256": digest})
    return {"records": records, "dirty": dirty}


def main(argv=None):
    """``python -m tests.radial_cases --json FILE``: the whole table in a process of its own (the GPU test starts it
    with AMT_DEBUG_POISON=1), a scratch check after every call"""
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--json", required=True)
    a = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison_child.write(a.json, run(get_context(), check_scratch=True))
    return 0


def same_bits(a, b) -> bool:
    """equal float64 bits, any NaN for any NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return a[keep].tobytes() == b[keep].tobytes()


def close(a, b) -> bool:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return bool(np.all(np.abs(a[keep] - b[keep]) <= ATOL + RTOL * np.abs(b[keep])))


if __name__ == "__main__":
    sys.exit(main())
