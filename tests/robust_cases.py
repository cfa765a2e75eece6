"""The case list of tests/test_gpu_robust_intensity.py: label planes and (C, Y, X) intensity stacks, uint16 and float64,
each run alone and as plane 1 of a stack (plus one batch of three different planes) through ``hipops.robust_intensity``
and compared bit for bit with tests/robust_reference.py.

``python -m tests.robust_cases --json FILE`` runs the whole list in a process of its own (the test starts it with
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

import poison_child  # noqa: E402
import robust_reference as qr  # noqa: E402

SHAPES = [(7, 5), (33, 40), (64, 64), (70, 131)]
BIG = (260, 260)  # one label of 67,600 pixels: counts beyond 16 bits
KINDS = ("u16", "f64")
DTYPE = {"u16": np.uint16, "f64": np.float64}


def _bins():
    from arcadia_microscopy_tools_amd import _hip

    return int(_hip.ROBUST_LDS_BINS)


def blobs(shape, seed: int, count: int, radius: float) -> np.ndarray:
    """Discs around ``count`` random centres, a pixel to its nearest centre; labels 1..count, some possibly empty."""
    rng = np.random.RandomState(seed)
    H, W = shape
    cy, cx = rng.uniform(0, H, count), rng.uniform(0, W, count)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (yy[..., None] - cy) ** 2 + (xx[..., None] - cx) ** 2
    near = np.argmin(d2, axis=-1)
    return np.where(np.min(d2, axis=-1) <= radius * radius, near + 1, 0).astype(np.int32)


def _runs(shape, counts):
    """labels 1, 2, ... in consecutive runs of ``counts`` pixels in raster order; the rest is background"""
    lab = np.zeros(shape[0] * shape[1], np.int32)
    at = 0
    for i, c in enumerate(counts):
        lab[at:at + c] = i + 1
        at += c
    assert at <= lab.size
    return lab.reshape(shape)


def _noise(rng, shape, kind):
    if kind == "u16":
        return rng.randint(0, 65536, shape).astype(np.uint16)
    return rng.normal(100.0, 30.0, shape)


def _window(rng, size, lo, levels):
    """``size`` uint16 values from lo .. lo + levels - 1 with both ends present"""
    v = rng.randint(lo, lo + levels, size)
    v[0], v[-1] = lo, lo + levels - 1
    rng.shuffle(v)
    return v.astype(np.uint16)


LEVELS = ("Bm1", "B", "Bp1", "2B", "65536")


def _levels(B):
    return dict(zip(LEVELS, (B - 1, B, B + 1, 2 * B, 65536)))


_CASES: dict = {}


def cases(shape, kind):
    """name -> (labels (Y, X) int32, stack (C, Y, X) uint16 / float64, max_label); built once per shape and kind."""
    if (shape, kind) in _CASES:
        return _CASES[(shape, kind)]
    H, W = shape
    n = H * W
    B = _bins()
    seed = 1000 * H + W + (0 if kind == "u16" else 7)
    rng = np.random.RandomState(seed)
    dt = DTYPE[kind]
    out = {}
    if shape == BIG:
        lab = np.ones(shape, np.int32)
        img = _noise(rng, shape, kind)
        if kind == "u16":
            img[0, 0], img[-1, -1] = 0, 65535
        out["one_label"] = (lab, img[None], 1)
        _CASES[(shape, kind)] = out
        return out
    count = max(1, min(12, n // 8))
    a = blobs(shape, seed, count, 2.0 + min(H, W) / 5.0)
    out["blobs"] = (a, _noise(rng, shape, kind)[None], count)
    out["gaps"] = (a * 3, _noise(rng, shape, kind)[None], 3 * count + 2)  # every third number present, the last two absent
    # label 1 in scattered pieces of modest values; its box holds the other labels' extreme values
    lab = rng.randint(0, 4, shape).astype(np.int32)
    img = np.where(lab == 1, rng.randint(1000, 1200, shape), np.where(rng.randint(0, 2, shape) == 1, 65535, 0))
    if kind == "f64":
        img = np.where(lab == 1, img * 0.37, np.where(img == 0, -1e300, 1e300))
    out["pieces"] = (lab, img.astype(dt)[None], 3)
    # labels of 1, 2, ... 8 pixels: every n mod 4, both parities ((7, 5) holds 1..7)
    small = [c for c in range(1, 9) if c * (c + 1) // 2 <= n]
    out["small_counts"] = (_runs(shape, small), _noise(rng, shape, kind)[None], len(small))
    lab = np.zeros(shape, np.int32)
    lab[:, 0] = 1  # a box one column wide
    lab[0, 1:] = 2  # a box one row high, wider than 64 columns on the widest shape
    lab[H // 2:, W // 2:] = 3
    out["column_and_row"] = (lab, _noise(rng, shape, kind)[None], 3)
    # five labels of m pixels (the last one even): constant, all lowest, all highest, all equal but one, half / half
    m = n // 5
    m5 = m - m % 2
    lab = _runs(shape, [m, m, m, m, m5])
    lo, hi, mid = (0, 65535, 1234) if kind == "u16" else (-1e300, 1e300, 0.1)
    flat = np.zeros(n, dt)
    flat[0:m] = mid
    flat[m:2 * m] = lo if kind == "u16" else 0.0
    flat[2 * m:3 * m] = hi
    flat[3 * m:4 * m] = mid
    flat[3 * m + m // 2] = hi
    flat[4 * m:4 * m + m5] = np.tile([lo, hi], m5 // 2)
    out["constants"] = (lab, flat.reshape(shape)[None], 5)
    for C in (2, 3, 5):
        out[f"channels_{C}"] = (a, np.stack([_noise(rng, shape, kind) for _ in range(C)]), count)
    if kind == "u16":
        whole = np.ones(shape, np.int32)
        whole[0] = 2  # label 2: the first row, label 1: the rest
        body = n - W
        for name, levels in _levels(B).items():
            img = np.concatenate([_noise(rng, (W,), kind), _window(rng, body, 0 if levels == 65536 else 321, levels)])
            out[f"levels_{name}"] = (whole, img.reshape(shape)[None], 2)
        step = 65536 // B  # values per coarse counter when the window is all of uint16
        # the window is all of uint16 (one pixel at each end), every other value inside ONE coarse counter
        v = (468 * step + rng.randint(0, step, body)).astype(np.uint16)
        v[0], v[1] = 0, 65535
        rng.shuffle(v)
        out["ranks_one_bin"] = (whole, np.concatenate([_noise(rng, (W,), kind), v]).reshape(shape)[None], 2)
        # uniform over all of uint16: the three quantiles lie in three counters far apart
        out["ranks_three_bins"] = (whole, _noise(rng, shape, kind)[None], 2)
        # an even count, one half low and one half high: the median's two ranks lie in two counters
        half = (body - body % 2) // 2
        v = np.concatenate([100 * step + rng.randint(0, step, half), 700 * step + rng.randint(0, step, half)])
        v[0], v[-1] = 0, 65535
        rng.shuffle(v)
        lab = whole.copy().ravel()
        lab[W + 2 * half:] = 0
        img = np.concatenate([_noise(rng, (W,), kind), v.astype(np.uint16), np.zeros(body - 2 * half, np.uint16)])
        out["rank_straddle"] = (lab.reshape(shape), img.reshape(shape)[None], 2)
        # values span B - 24 levels (one sweep places them), most of them at the low end: 2 median lies there and the
        # keys |2 v - 2 median| reach about twice the span, beyond the table
        v = np.concatenate([500 + rng.randint(0, 8, body - body // 8), 500 + rng.randint(0, B - 24, body // 8)])
        v[0], v[-1] = 500, 500 + B - 25
        rng.shuffle(v)
        out["mad_keys_wide"] = (whole, np.concatenate([_noise(rng, (W,), kind), v.astype(np.uint16)]).reshape(shape)[None], 2)
    else:
        # negative values and zeros of ONE sign per label (numpy's own order among -0.0 and +0.0 is not defined),
        # both zeros below every rank, subnormals, 600 orders of magnitude, heavy ties
        m = n // 6
        lab = _runs(shape, [m] * 6)
        flat = np.zeros(n, np.float64)
        flat[0:m] = np.array([-2.5, -0.0, 3.0])[rng.randint(0, 3, m)]
        flat[m:2 * m] = np.array([-1.0, 0.0, 2.0])[rng.randint(0, 3, m)]
        flat[2 * m:3 * m] = rng.normal(10.0, 1.0, m)
        if m >= 9:
            flat[2 * m], flat[2 * m + 1] = -0.0, 0.0
        flat[3 * m:4 * m] = 5e-324 * rng.randint(-50, 50, m)
        flat[3 * m:4 * m][flat[3 * m:4 * m] == 0] = 5e-324  # no zero of either sign among the subnormals
        flat[4 * m:5 * m] = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-300, 300, m)
        flat[5 * m:6 * m] = np.array([-7.25, 0.1, 0.1 + 2.0 ** -52, 1e10])[rng.randint(0, 4, m)]
        out["float_specials"] = (lab, flat.reshape(shape)[None], 6)
    _CASES[(shape, kind)] = out
    return out


_REF: dict = {}


def reference(shape, kind, name, max_label=None):
    """(max_label, C, 4) float64 of the case; computed once and shared."""
    lab, stack, k = cases(shape, kind)[name]
    k = k if max_label is None else max_label
    key = (shape, kind, name, k)
    if key not in _REF:
        _REF[key] = qr.robust_stack(lab, stack, k)
    return _REF[key]


BATCH = ("blobs", "constants", "pieces")  # three different planes with different stacks


def run(ctx, shapes=None, kinds=KINDS, check=False):
    """Every case of ``shapes`` alone and as plane 1, and the batch -> {"records": [{"key", "sha256", "ok"}],
    "dirty": [...]}.  ``check``: call ``ctx.scratch_check()`` after every operator call."""
    from arcadia_microscopy_tools_amd import hipops

    records, dirty = [], []

    def call(key, labels, stack, k):
        t = hipops.robust_intensity(labels, stack, k).numpy()
        if check:
            bad = ctx.scratch_check()
            if bad is not None:
                dirty.append([list(key), list(bad)])
        return t

    def record(key, got, want):
        got = np.ascontiguousarray(got)
        ok = got.shape == want.shape and got.dtype == np.float64 and got.tobytes() == np.ascontiguousarray(want).tobytes()
        records.append({"key": list(key), "sha256": hashlib.sha256(got.tobytes()).hexdigest(), "ok": bool(ok)})

    for shape in shapes or SHAPES + [BIG]:
        for kind in kinds:
            for name, (lab, stack, k) in cases(shape, kind).items():
                want = reference(shape, kind, name)
                got = call((shape, kind, name, "single"), ctx.asarray(lab[None]), ctx.asarray(stack[None]), k)
                record((shape, kind, name, "single"), got[0], want)
                # plane 1 of a two-plane stack: the base pointers lie inside an allocation
                la = ctx.asarray(np.stack([np.roll(lab, 1, axis=1), lab]))
                st = ctx.asarray(np.stack([np.roll(stack, 1, axis=1), stack]))
                got = call((shape, kind, name, "plane1"), la[1], st[1], k)
                record((shape, kind, name, "plane1"), got[0], want)
            if shape == BIG:
                continue
            k = max(cases(shape, kind)[name][2] for name in BATCH)
            la = ctx.asarray(np.stack([cases(shape, kind)[name][0] for name in BATCH]))
            st = ctx.asarray(np.stack([cases(shape, kind)[name][1] for name in BATCH]))
            got = call((shape, kind, "batch", "batch"), la, st, k)
            for i, name in enumerate(BATCH):
                record((shape, kind, name, "batch"), got[i], reference(shape, kind, name, k))
    return {"records": records, "dirty": dirty}


def main(argv):
    from arcadia_microscopy_tools_amd.device import get_context

    out = argv[argv.index("--json") + 1]
    poison_child.write(out, run(get_context(), check=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
