"""The case list of tests/test_gpu_texture.py: label planes and (C, Y, X) intensity stacks, uint16 and float64, each run
alone and as plane 1 of a stack (plus one batch of three different planes with different ranges) through
``hipops.texture`` and compared with tests/texture_reference.py: the counts byte for byte, the features within
RTOL / ATOL with NaNs in the same places, info_measure_2 on its square.

``python -m tests.texture_cases --json FILE`` runs the whole list in a process of its own (the test starts it with
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
import texture_reference as tr  # noqa: E402

SHAPES = [(7, 5), (33, 40), (64, 64), (70, 131)]
BIG = (260, 260)  # one constant label: 2 * 260 * 259 = 134,680 in one diagonal counter, beyond 16 bits
KINDS = ("u16", "f64")
DTYPE = {"u16": np.uint16, "f64": np.float64}
WIDTHS = (7, 8, 9, 16, 17, 32, 33, 64, 65)  # one box on each side of every switch of amt_box_layout
# the project's parity for float region properties, and an absolute term for the columns that are exactly 0 in the
# reference (two float64 summation orders of the reference differ by up to 3.5e-13 there)
RTOL, ATOL = 1e-9, 1e-12


def blobs(shape, seed: int, count: int, radius: float) -> np.ndarray:
    """Discs around ``count`` random centres, a pixel to its nearest centre; labels 1..count, some possibly empty."""
    rng = np.random.RandomState(seed)
    H, W = shape
    cy, cx = rng.uniform(0, H, count), rng.uniform(0, W, count)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (yy[..., None] - cy) ** 2 + (xx[..., None] - cx) ** 2
    near = np.argmin(d2, axis=-1)
    return np.where(np.min(d2, axis=-1) <= radius * radius, near + 1, 0).astype(np.int32)


def _noise(rng, shape, kind):
    """uint16 over all of 0..65535 (both ends present); float64 with negative values"""
    if kind == "u16":
        img = rng.randint(0, 65536, shape).astype(np.uint16)
        img.flat[0], img.flat[-1] = 0, 65535
        return img
    return rng.normal(0.0, 50.0, shape)


def _smooth(rng, shape, kind):
    """neighbouring pixels of similar value, as in an image: the matrices are not uniform"""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    v = 0.5 + 0.3 * np.sin(yy / 3.1) * np.cos(xx / 4.3) + 0.2 * rng.uniform(-1, 1, shape)
    return (v * 40000).astype(np.uint16) if kind == "u16" else (v - 0.5) * 200.0


def _case(lab, stack, k, levels=8, distance=1, ranges=None):
    return (np.ascontiguousarray(lab, np.int32), np.ascontiguousarray(stack), int(k),
            {"levels": levels, "distance": distance, "ranges": None if ranges is None else np.asarray(ranges, np.float64)})


def _corner_boxes(shape, w, hh):
    """four labels ``w`` columns wide and ``hh`` rows high in row bands of their own: the top-left corner, the right
    border, the left border and the bottom-right corner"""
    H, W = shape
    lab = np.zeros(shape, np.int32)
    lab[0:hh, 0:w] = 1
    lab[hh:2 * hh, W - w:W] = 2
    lab[H - 2 * hh:H - hh, 0:w] = 3
    lab[H - hh:H, W - w:W] = 4
    return lab


_CASES: dict = {}


def cases(shape, kind):
    """name -> (labels (Y, X) int32, stack (C, Y, X), max_label, {levels, distance, ranges}); built once per shape and kind."""
    if (shape, kind) in _CASES:
        return _CASES[(shape, kind)]
    H, W = shape
    n = H * W
    seed = 1000 * H + W + (0 if kind == "u16" else 7)
    rng = np.random.RandomState(seed)
    dt = DTYPE[kind]
    out = {}
    if shape == BIG:
        v = 1000 if kind == "u16" else -2.5
        out["one_constant_label"] = _case(np.ones(shape), np.full((1,) + shape, v, dt), 1, ranges=(v - 3, v + 1))
        _CASES[(shape, kind)] = out
        return out
    count = max(1, min(12, n // 8))
    a = blobs(shape, seed, count, 2.0 + min(H, W) / 5.0)
    noise, smooth = _noise(rng, shape, kind), _smooth(rng, shape, kind)
    out["blobs"] = _case(a, smooth[None], count + 1)  # the last label is absent
    out["blobs_noise"] = _case(a, noise[None], count + 1)
    # ---- box widths on both sides of every layout switch, at the plane's borders and corners; mirrored at d = 2
    hh = max(1, min(5, H // 4))
    for w in (w for w in WIDTHS if w <= W):
        lab = _corner_boxes(shape, w, hh)
        out[f"width_{w}"] = _case(lab, smooth[None], 4)
        out[f"width_{w}_mirrored"] = _case(lab[:, ::-1], noise[None], 4, distance=2)
    # ---- directions without a pair
    lab = np.zeros(shape, np.int32)
    lab[0, 0] = 1           # a single pixel
    lab[2, 0:3] = 2         # a row: nothing in 45 / 90 / 135
    lab[4:7, 4] = 3         # a column: only 90
    lab[4:6, 0:2] = 4       # 2 x 2: one pair on each diagonal
    out["no_pairs"] = _case(lab, noise[None], 4)
    lab = np.zeros(shape, np.int32)
    lab[0:5, 0:5] = 1
    out["distance_beyond_box"] = _case(lab, noise[None], 1, distance=7)
    # ---- labels in contact
    lab = np.ones(shape, np.int32)
    lab[:, W // 2:] = 2
    out["shared_edge"] = _case(lab, smooth[None], 2)
    yy, xx = np.mgrid[0:H, 0:W]
    out["checkerboard"] = _case(1 + (yy + xx) % 2, noise[None], 2)  # diagonal pairs only at d = 1
    lab = np.zeros(shape, np.int32)
    lab[:, 0:2] = 1
    lab[:, 2:4] = 2         # another label in the gap: it pairs with neither piece
    lab[:, 4:5] = 1         # column 1 + 3 = 4: the two pieces pair across the gap at d = 3
    out["two_pieces"] = _case(lab, noise[None], 2, distance=3)
    # ---- degenerate grey levels
    v = 1234 if kind == "u16" else -0.75
    whole = np.ones(shape, np.int32)
    out["constant_default_ranges"] = _case(whole, np.full((1,) + shape, v, dt), 1)  # hi == lo: level 0
    out["constant_level_5"] = _case(whole, np.full((1,) + shape, v, dt), 1, ranges=(v - 5.5, v + 2.5))
    two = np.where(xx % 2 == 0, 10, 900).astype(dt) if kind == "u16" else np.where(xx % 2 == 0, -3.5, 8.25)
    out["two_levels"] = _case(whole, two[None], 1)
    # ---- parameters
    for L in (2, 5, 32, 64):
        out[f"levels_{L}"] = _case(a, (noise if L == 64 else smooth)[None], count, levels=L)
    for d in (2, 3, 7):
        out[f"distance_{d}"] = _case(a, smooth[None], count, distance=d)
    lo, hi = np.percentile(smooth, [25, 75])
    out["ranges_narrow"] = _case(a, smooth[None], count, ranges=(float(lo), float(hi)))  # clipped at both ends
    mid = float(smooth[H // 2, W // 2])
    out["ranges_equal"] = _case(a, smooth[None], count, ranges=(mid, mid))
    out["ranges_value_at_hi"] = _case(a, smooth[None], count, ranges=(float(smooth.min()), mid))  # a value exactly at hi
    # ---- channels, each with a range of its own
    for C in (2, 5):
        stack = np.stack([_smooth(rng, shape, kind) if c % 2 else _noise(rng, shape, kind) for c in range(C)])
        out[f"channels_{C}"] = _case(a, stack, count)
    stack = out["channels_5"][1]
    r5 = tr.default_ranges(stack)
    r5[1] = r5[1, 0] + (r5[1, 1] - r5[1, 0]) * np.array([0.25, 0.5])
    out["channels_5_ranges"] = _case(a, stack, count, levels=5, distance=2, ranges=r5)
    _CASES[(shape, kind)] = out
    return out


_REF: dict = {}


def reference(shape, kind, name, max_label=None):
    """(table (max_label, C, 4, 13), counts (max_label, C, 4, L, L)) of the case; computed once and shared."""
    lab, stack, k, p = cases(shape, kind)[name]
    k = k if max_label is None else max_label
    key = (shape, kind, name, k)
    if key not in _REF:
        table, counts = tr.texture_stack(lab, stack, k, p["levels"], p["distance"], p["ranges"])
        table.setflags(write=False)
        counts.setflags(write=False)
        _REF[key] = (table, counts)
    return _REF[key]


def compare(got_table, got_counts, want_table, want_counts):
    """(ok, largest absolute error per column): counts byte for byte; NaNs in the same places; the features within
    RTOL / ATOL, info_measure_2 on its square (the root turns a 1e-16 rounding of HXY2 - HXY at exact independence into
    about 1e-8)."""
    err = np.zeros(len(tr.COLS))
    got_table, got_counts = np.ascontiguousarray(got_table), np.ascontiguousarray(got_counts)
    if got_counts.shape != want_counts.shape or got_counts.dtype != np.uint32 or \
            got_counts.tobytes() != np.ascontiguousarray(want_counts).tobytes():
        return False, err
    if got_table.shape != want_table.shape or got_table.dtype != np.float64 or \
            not np.array_equal(np.isnan(got_table), np.isnan(want_table)):
        return False, err
    g, w = got_table.copy(), want_table.copy()
    g[..., 12], w[..., 12] = g[..., 12] ** 2, w[..., 12] ** 2
    diff = np.where(np.isnan(w), 0.0, np.abs(g - w))
    err = diff.reshape(-1, len(tr.COLS)).max(axis=0) if diff.size else err
    ok = bool(np.all(diff <= ATOL + RTOL * np.abs(np.where(np.isnan(w), 0.0, w))))
    return ok, err


BATCH = ("blobs", "shared_edge", "two_levels")  # three different planes, each with a range of its own


def run(ctx, shapes=None, kinds=KINDS, check=False):
    """Every case of ``shapes`` alone and as plane 1, and the batch -> {"records": [{"key", "sha256", "ok", "err"}],
    "dirty": [...]}.  ``check``: call ``ctx.scratch_check()`` after every operator call."""
    from arcadia_microscopy_tools_amd import hipops

    records, dirty = [], []

    def call(key, labels, stack, k, p, ranges):
        t, g = hipops.texture(labels, stack, k, levels=p["levels"], distance=p["distance"], ranges=ranges, glcm=True)
        t, g = t.numpy(), g.numpy()
        if check:
            bad = ctx.scratch_check()
            if bad is not None:
                dirty.append([list(key), list(bad)])
        return t, g

    def record(key, table, counts, want):
        ok, err = compare(table, counts, *want)
        digest = hashlib.sha256(np.ascontiguousarray(table).tobytes() + np.ascontiguousarray(counts).tobytes()).hexdigest()
        records.append({"key": list(key), "sha256": digest, "ok": bool(ok), "err": [float(e) for e in err]})

    for shape in shapes or SHAPES + [BIG]:
        for kind in kinds:
            for name, (lab, stack, k, p) in cases(shape, kind).items():
                want = reference(shape, kind, name)
                r = None if p["ranges"] is None else np.broadcast_to(p["ranges"], (1, stack.shape[0], 2))
                t, g = call((shape, kind, name, "single"), ctx.asarray(lab[None]), ctx.asarray(stack[None]), k, p, r)
                record((shape, kind, name, "single"), t[0], g[0], want)
                # plane 1 of a two-plane stack: the base pointers lie inside an allocation
                la = ctx.asarray(np.stack([np.roll(lab, 1, axis=1), lab]))
                st = ctx.asarray(np.stack([np.roll(stack, 1, axis=2), stack]))
                t, g = call((shape, kind, name, "plane1"), la[1], st[1], k, p, r)
                record((shape, kind, name, "plane1"), t[0], g[0], want)
            if shape == BIG:
                continue
            members = [cases(shape, kind)[name] for name in BATCH]
            k = max(m[2] for m in members)
            p = members[0][3]
            assert all(m[3]["levels"] == p["levels"] and m[3]["distance"] == p["distance"] for m in members)
            # the ranges the planes would get by default, handed over explicitly: they differ from plane to plane
            ranges = np.stack([tr.default_ranges(m[1]) if m[3]["ranges"] is None
                               else np.broadcast_to(m[3]["ranges"], (m[1].shape[0], 2)) for m in members])
            la = ctx.asarray(np.stack([m[0] for m in members]))
            st = ctx.asarray(np.stack([m[1] for m in members]))
            t, g = call((shape, kind, "batch", "batch"), la, st, k, p, ranges)
            for i, name in enumerate(BATCH):
                record((shape, kind, name, "batch"), t[i], g[i], reference(shape, kind, name, k))
    return {"records": records, "dirty": dirty}


def main(argv):
    from arcadia_microscopy_tools_amd.device import get_context

    out = argv[argv.index("--json") + 1]
    poison_child.write(out, run(get_context(), check=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
