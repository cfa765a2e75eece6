"""The case list of tests/test_gpu_relate.py: label planes and companion label planes on the small shapes of the other
operator tests, each run three ways through ``hipops.relate_labels`` and compared bit for bit with
tests/relate_reference.py.

``python -m tests.relate_cases --json FILE`` runs the whole list in a process of its own (the test starts it with
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
import relate_reference as rr  # noqa: E402

SHAPES = [(1, 1), (1, 17), (19, 1), (7, 5), (16, 16), (33, 40), (64, 64), (65, 128), (70, 131)]
BIG = 2**31 - 2  # the largest companion value of the C ABI


def _partners():
    from arcadia_microscopy_tools_amd import _hip

    return int(_hip.RELATE_LDS_PARTNERS)


def overflow_shape():
    """The shape that carries the cases around the LDS table's capacity: 33 x 40 = 1320 pixels hold up to 4 x 256
    distinct partners, a larger table needs (70, 131)."""
    return (33, 40) if _partners() <= 256 else (70, 131)


def blobs(shape, seed: int, count: int, radius: float) -> np.ndarray:
    """Discs around ``count`` random centres, a pixel to its nearest centre; labels 1..count, some possibly empty."""
    rng = np.random.RandomState(seed)
    H, W = shape
    cy, cx = rng.uniform(0, H, count), rng.uniform(0, W, count)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (yy[..., None] - cy) ** 2 + (xx[..., None] - cx) ** 2
    near = np.argmin(d2, axis=-1)
    return np.where(np.min(d2, axis=-1) <= radius * radius, near + 1, 0).astype(np.int32)


def _flat(shape, fill):
    a = np.zeros(shape[0] * shape[1], np.int32)
    fill(a)
    return a.reshape(shape)


# the pairs whose contingency tables tests/golden/relate.npz records (tools/make_golden_relate.py): small values only,
# the tables are dense
GOLDEN = [((7, 5), "pieces"), ((16, 16), "blobs"), ((33, 40), "gaps"), ((33, 40), "dense"), ((64, 64), "blobs"),
          ((65, 128), "column_and_row"), ((70, 131), "zero_companion")]

_CASES: dict = {}


def cases(shape):
    """name -> (labels, companion, max_label) int32 planes of ``shape``; built once per shape."""
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
    b = blobs(shape, seed + 1, count + 2, 2.5 + min(H, W) / 4.0)
    out["blobs"] = (a, b, count)
    out["zero_companion"] = (a, np.zeros(shape, np.int32), count)
    out["gaps"] = (a * 3, b, 3 * count + 2)  # only every third number is present, the last two absent as well
    out["pieces"] = (rng.randint(0, 4, shape).astype(np.int32), b, 3)  # every label in many pieces
    out["dense"] = (rng.randint(1, 6, shape).astype(np.int32), rng.randint(1, 40, shape).astype(np.int32), 5)
    out["out_of_range_labels"] = (rng.randint(-2, 9, shape).astype(np.int32), b, 4)  # labels outside 1..4 are ignored
    if n >= 5:
        m = n // 5

        def ties(f):
            f[:2 * m] = 1
            f[2 * m:5 * m] = 2

        def tie_values(f):
            f[:2 * m] = np.tile([9, 3], m)  # two partners, m pixels each: 3 wins
            f[2 * m:5 * m] = np.tile([BIG, 7, 8], m)  # three partners: 7 wins
        out["ties"] = (_flat(shape, ties), _flat(shape, tie_values), 2)
    special = np.array([1, BIG, P, 2 * P, 3 * P, P + 1, 2 * P + 1, BIG - P, BIG - 2 * P, 1 + 5 * P], np.int64)
    out["special_values"] = (np.ones(shape, np.int32), special[rng.randint(0, len(special), shape)].astype(np.int32), 1)
    lab = np.zeros(shape, np.int32)
    lab[:, 0] = 1  # a box one column wide
    lab[0, 1:] = 2  # a box one row high, wider than 64 columns on the two widest shapes
    lab[H // 2:, W // 2:] = 3
    out["column_and_row"] = (lab, rng.randint(0, 5, shape).astype(np.int32), 3)
    if shape == overflow_shape():
        for d in (P - 1, P, P + 1, 4 * P):
            for kind in ("random", "congruent"):
                if kind == "random":  # d distinct values over the whole range, its two ends among them
                    vals = np.unique(rng.randint(2, BIG, 4 * d).astype(np.int64))[:d]
                    vals[0], vals[-1] = 1, BIG
                else:  # every value has the same home slot
                    vals = 5 + P * np.arange(d, dtype=np.int64) * 3
                assert len(np.unique(vals)) == d
                # label 1 (all rows but the first) carries exactly the d partners, label 2 (the first row) three of
                # them: both paths in one launch
                body = np.concatenate([vals, vals[rng.randint(0, d, n - W - d)]])
                rng.shuffle(body)
                comp = np.concatenate([vals[np.arange(W) % 3], body])
                lab = np.ones(shape, np.int32)
                lab[0] = 2
                out[f"{kind}_{d}_partners"] = (lab, comp.reshape(shape).astype(np.int32), 2)
    _CASES[shape] = out
    return out


_REF: dict = {}


def reference(shape, name, max_label=None):
    """(max_label, 4) int64 columns of the case; computed once and shared."""
    a, b, k = cases(shape)[name]
    k = k if max_label is None else max_label
    key = (shape, name, k)
    if key not in _REF:
        _REF[key] = rr.relate_columns(a, b, k)
    return _REF[key]


BATCH = ("blobs", "zero_companion", "dense")  # typical / all-zero companion / dense


def run(ctx, shapes=None, check=False):
    """Every case of ``shapes`` three ways -> {"records": [{"key", "sha256", "ok"}], "dirty": [...]}.  ``check``:
    call ``ctx.scratch_check()`` after every operator call."""
    from arcadia_microscopy_tools_amd import hipops

    records, dirty = [], []

    def call(key, labels, k, comp):
        t = hipops.relate_labels(labels, k, comp).numpy()
        if check:
            bad = ctx.scratch_check()
            if bad is not None:
                dirty.append([list(key), list(bad)])
        return t

    def record(key, got, want):
        ok = got.shape == want.shape and got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))
        records.append({"key": list(key), "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest(),
                        "ok": bool(ok)})

    for shape in shapes or SHAPES:
        H, W = shape
        for name, (a, b, k) in cases(shape).items():
            want = reference(shape, name)
            got = call((shape, name, "single"), ctx.asarray(a), k, ctx.asarray(b))
            record((shape, name, "single"), got[0, :, 0, :], want)
            # plane 1 of a two-plane stack: the base pointers are H * W * 4 bytes past an allocation's
            la = ctx.asarray(np.stack([np.roll(a, 1, axis=1), a]))
            lb = ctx.asarray(np.stack([np.roll(b, 1, axis=0), b]))
            got = call((shape, name, "plane1"), la[1], k, lb[1])
            record((shape, name, "plane1"), got[0, :, 0, :], want)
        k = max(cases(shape)[name][2] for name in BATCH)
        la = ctx.asarray(np.stack([cases(shape)[name][0] for name in BATCH]))
        lb = ctx.asarray(np.stack([cases(shape)[name][1] for name in BATCH]))
        got = call((shape, "batch", "batch"), la, k, lb)
        for i, name in enumerate(BATCH):
            record((shape, name, "batch"), got[i, :, 0, :], reference(shape, name, k))
    return {"records": records, "dirty": dirty}


def main(argv):
    from arcadia_microscopy_tools_amd.device import get_context

    out = argv[argv.index("--json") + 1]
    poison_child.write(out, run(get_context(), check=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
