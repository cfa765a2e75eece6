"""The case table of grey reconstruction on the device (ops 3 .. 6 of amt_rank_filter), sized from the kernel's tile
(``hipops.reconstruct_tile``) so that every seam is crossed at the smallest planes that can still go wrong.

A case is (name, footprint name, seeds (N, H, W), masks (N, H, W)) for reconstruction BY DILATION; the erosion case is
its dual (``reconstruction_reference.dual`` of both images), and its expected result the dual of the expected result.
``expected(kind)`` computes every reference once (the heap flood) and keeps it.

``python -m tests.reconstruction_cases --json FILE`` runs the whole table, both methods and the h-operators, in a process
of its own with a scratch check after every call (the GPU test starts it with AMT_DEBUG_POISON=1).
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import poison_child  # noqa: E402
import reconstruction_reference as rr  # noqa: E402

KINDS = {"u16": np.uint16, "f64": np.float64}
SMALL = ((1, 1), (1, 9), (9, 1), (7, 5))


def tile(kind):
    from arcadia_microscopy_tools_amd import hipops

    return hipops.reconstruct_tile(KINDS[kind])


def seam_shape(kind):
    th, tw = tile(kind)
    return 2 * th + 3, 2 * tw + 5


def _values(kind, rng, shape, alphabet):
    v = rng.choice(np.asarray(alphabet), size=shape)
    return v.astype(KINDS[kind])


def _floor(kind):
    return 0 if kind == "u16" else -np.inf


def serpentine(kind, shape, high, level):
    """corridor rows 0, 2, 4, ... joined alternately at the right and the left end; a one-pixel seed at its start"""
    H, W = shape
    mask = np.zeros(shape, KINDS[kind])
    mask[0::2, :] = high
    for k, y in enumerate(range(1, H, 2)):
        mask[y, W - 1 if k % 2 == 0 else 0] = high
    seed = np.zeros(shape, KINDS[kind])
    seed[0, 0] = level
    return seed, mask


def staircase(kind, shape, high, level):
    """two diagonal corridors: from (0, 0), and one through the corner shared by four tiles; they pass under all-ones
    and stop at their first pixel under the cross"""
    H, W = shape
    th, tw = tile(kind)
    mask = np.zeros(shape, KINDS[kind])
    seed = np.zeros(shape, KINDS[kind])
    for y0, x0, lv in ((0, 0, level), (0, tw - th, level - 1)):
        n = min(H - y0, W - x0)
        idx = np.arange(n)
        mask[y0 + idx, x0 + idx] = high
        seed[y0, x0] = lv
    return seed, mask


@functools.lru_cache(maxsize=None)
def cases(kind):
    dt = KINDS[kind]
    rng = np.random.default_rng(20240 + len(kind) + (kind == "f64"))
    out = []
    alphabet = (3, 40, 41, 900) if kind == "u16" else (-7.5, -0.25, 1.0, 1e300)
    for shape in SMALL:  # below a tile
        mask = _values(kind, rng, shape, alphabet)
        seed = np.where(rng.random(shape) < 0.3, mask, np.asarray(min(alphabet), dt)).astype(dt)
        for fpn in rr.FOOTPRINTS:
            out.append((f"small {shape[0]}x{shape[1]}", fpn, seed[None], mask[None]))
    H, W = shape = seam_shape(kind)
    # a one-pixel seed in each corner under a constant mask: the fill crosses every seam in every direction
    seeds = np.zeros((4,) + shape, dt)
    for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        seeds[i, y, x] = 17 + i
    masks = np.full((4,) + shape, 50, dt)
    out.append(("corners", "cross", seeds, masks))
    out.append(("corners", "ones", seeds[1:3], masks[1:3]))
    s, m = serpentine(kind, shape, 1000, 700)
    out.append(("serpentine", "cross", s[None], m[None]))
    st, mt = serpentine(kind, (W, H), 1000, 700)
    out.append(("serpentine transposed", "cross", np.ascontiguousarray(st.T)[None], np.ascontiguousarray(mt.T)[None]))
    s2, m2 = staircase(kind, shape, 1000, 700)
    for fpn in rr.FOOTPRINTS:
        out.append(("staircase", fpn, s2[None], m2[None]))
    # plateaus: a four-value alphabet, seeds on a tenth of the pixels
    mask = _values(kind, rng, shape, alphabet)
    seed = np.where(rng.random(shape) < 0.1, mask, np.asarray(min(alphabet), dt)).astype(dt)
    for fpn in rr.FOOTPRINTS:
        out.append(("plateaus", fpn, seed[None], mask[None]))
    if kind == "u16":  # the full range, 0 and 65535 included
        mask = rng.integers(0, 65536, shape).astype(dt)
        mask[5, 7], mask[H - 2, W - 3] = 0, 65535
        seed = np.where(rng.random(shape) < 0.02, mask, 0).astype(dt)
        seed[H - 2, W - 3] = 65535
    else:  # negative values, -inf where there is no seed, a +inf seed under a +inf mask
        mask = rng.normal(0.0, 3.0, shape)
        mask[H // 2, W // 2] = np.inf
        seed = np.where(rng.random(shape) < 0.02, mask, -np.inf)
        seed[H // 2, W // 2] = np.inf
    for fpn in rr.FOOTPRINTS:
        out.append(("full range", fpn, seed[None], mask[None]))
    # three planes: one converges at once, one needs the serpentine's rounds, one is random -- planes are independent
    seeds = np.stack([m, s, seed])
    masks = np.stack([m, m, mask])
    out.append(("batch", "cross", seeds, masks))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(kind):
    """the dilation results of ``cases(kind)``, by the heap flood, computed once"""
    res = []
    for _, fpn, seeds, masks in cases(kind):
        res.append(np.stack([rr.flood(s, m, rr.FOOTPRINTS[fpn]) for s, m in zip(seeds, masks)]))
    return tuple(res)


H_CASES = {"u16": (1, 65535, 300), "f64": (0.75, 2.0)}


@functools.lru_cache(maxsize=None)
def h_image(kind):
    """a plane for ops 5 / 6: smooth bumps plus noise; uint16 reaches 0 and 65535 and holds values below h = 300"""
    H, W = seam_shape(kind)
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.zeros((H, W))
    for _ in range(12):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(4, 18)
        a += rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    a += 0.02 * rng.random((H, W))
    if kind == "f64":
        return (a * 10.0 - 3.0)[None]
    u = np.clip(a / a.max() * 70000.0 - 2000.0, 0, 65535).astype(np.uint16)
    assert u.min() == 0 and u.max() == 65535 and ((u > 0) & (u < 300)).any()
    return u[None]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def run(ctx, check_scratch=False):
    """every case x method and every h-operator on the device -> {"records": [...], "dirty": [...]}"""
    import hashlib

    from arcadia_microscopy_tools_amd import hipops

    records, dirty = [], []

    def note(key, arr):
        if check_scratch:
            bad = ctx.scratch_check()
            if bad is not None:
                dirty.append([list(key), list(bad)])
        records.append({"key": list(key), "sha256": hashlib.sha256(arr.tobytes()).hexdigest()})

    for kind in KINDS:
        for (name, fpn, seeds, masks) in cases(kind):
            for method in ("dilation", "erosion"):
                s, m = (seeds, masks) if method == "dilation" else (rr.dual(seeds), rr.dual(masks))
                r = hipops.reconstruction(ctx.asarray(s), ctx.asarray(m), method, rr.FOOTPRINTS[fpn])
                note((kind, name, fpn, method), r.numpy())
        a = ctx.asarray(h_image(kind))
        for h in H_CASES[kind]:
            for method in ("dilation", "erosion"):
                note((kind, "h", h, method), hipops.h_reconstruction(a, h, method).numpy())
            note((kind, "h-dome", h), hipops.h_reconstruction(a, h, "dilation", minuend=a).numpy())
            note((kind, "h_maxima", h), hipops.h_maxima(a, h).numpy())
            note((kind, "h_minima", h), hipops.h_minima(a, h).numpy())
    return {"records": records, "dirty": dirty}


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--json", required=True)
    a = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison_child.write(a.json, run(get_context(), check_scratch=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
