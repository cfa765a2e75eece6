"""Test-side reference for per-cell channel colocalisation: plain numpy / Python, written from the definitions in
include/amt_hip.h (which restate skimage.measure's colocalisation functions), sharing nothing with the library.

For one label with pixel set P (n pixels), channels A and B, thresholds tA and tB:
    pearson        (n Sab - Sa Sb) / sqrt((n Saa - Sa^2)(n Sbb - Sb^2))   NaN when a channel is constant over P
    overlap        Sab / sqrt(Saa Sbb)                                      NaN when the denominator is 0
    m1             sum a[b > tB] / Sa                                       0 when Sa = 0
    m2             sum b[a > tA] / Sb                                       0 when Sb = 0
    intersection1  |{a > tA and b > tB}| / |{a > tA}|                       0 when the denominator is 0
    intersection2  |{a > tA and b > tB}| / |{b > tB}|                       0 when the denominator is 0
An empty P follows the same rules: NaN, NaN, 0, 0, 0, 0.

Integer images are evaluated in exact integer arithmetic: the sums are Python ints (gathered with uint64 numpy sums,
which are exact below 2^64 and checked to be), the quotients are single correctly rounded divisions of integers, and
the square roots are taken with math.isqrt at 128 extra bits, so every value is the correctly rounded float64 of the
true one.  Float images use numpy's two-pass form (means first, then centred sums).
"""
import math
from fractions import Fraction

import numpy as np

COLS = ("pearson", "overlap", "m1", "m2", "intersection1", "intersection2")
NAN = float("nan")
_EXTRA = 128  # bits of the integer square roots below the unit


def _ratio_over_root(num: int, radicand: int) -> float:
    """num / sqrt(radicand) for integers, radicand > 0, rounded once."""
    root = math.isqrt(radicand << (2 * _EXTRA))  # floor(sqrt(radicand) * 2^_EXTRA): relative error below 2^-128
    return float(Fraction(num << _EXTRA, root))


def _quotient(num: int, den: int) -> float:
    return num / den if den else 0.0  # int / int is correctly rounded in Python


def exact_pair(a, b, ta, tb):
    """The six columns for integer samples a, b (1-D arrays of equal length) -> tuple of floats."""
    a = np.asarray(a).astype(np.uint64).ravel()
    b = np.asarray(b).astype(np.uint64).ravel()
    n = int(a.size)
    assert n < 2 ** 32 and (n == 0 or (int(a.max()) < 2 ** 16 and int(b.max()) < 2 ** 16)), "sums must fit uint64"
    pa, pb = a.astype(np.float64) > ta, b.astype(np.float64) > tb  # values below 2^16 are exact in float64
    total = lambda x: int(x.sum(dtype=np.uint64))  # noqa: E731
    sa, sb, saa, sbb, sab = total(a), total(b), total(a * a), total(b * b), total(a * b)
    da, db = n * saa - sa * sa, n * sbb - sb * sb
    pearson = NAN if da == 0 or db == 0 else _ratio_over_root(n * sab - sa * sb, da * db)
    overlap = NAN if saa == 0 or sbb == 0 else _ratio_over_root(sab, saa * sbb)
    na, nb, nab = int(pa.sum()), int(pb.sum()), int((pa & pb).sum())
    return (pearson, overlap, _quotient(total(a[pb]), sa), _quotient(total(b[pa]), sb), _quotient(nab, na),
            _quotient(nab, nb))


def float_pair(a, b, ta, tb):
    """The six columns for float samples, two-pass."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    if a.size == 0:
        return (NAN, NAN, 0.0, 0.0, 0.0, 0.0)
    pa, pb = a > ta, b > tb
    if a.min() == a.max() or b.min() == b.max():
        pearson = NAN
    else:
        da, db = a - a.mean(), b - b.mean()
        pearson = float((da * db).sum() / np.sqrt((da * da).sum() * (db * db).sum()))
    oden = np.sqrt((a * a).sum() * (b * b).sum())
    overlap = NAN if oden == 0 else float((a * b).sum() / oden)
    sa, sb = a.sum(), b.sum()
    na, nb, nab = int(pa.sum()), int(pb.sum()), int((pa & pb).sum())
    return (pearson, overlap, float(a[pb].sum() / sa) if sa != 0 else 0.0, float(b[pa].sum() / sb) if sb != 0 else 0.0,
            nab / na if na else 0.0, nab / nb if nb else 0.0)


def all_pairs(C):
    return [(i, j) for i in range(C) for j in range(i + 1, C)]


def table(labels, stack, max_label, thresholds=None, pairs=None):
    """(max_label, npairs, 6) float64 for one label plane (Y, X) and its (C, Y, X) stack; integer stacks take the exact
    form, float stacks the two-pass one.  ``thresholds``: None, a number or C numbers."""
    stack = np.asarray(stack)
    C = stack.shape[0]
    thr = np.broadcast_to(np.asarray(0.0 if thresholds is None else thresholds, dtype=np.float64), (C,))
    pairs = all_pairs(C) if pairs is None else [tuple(p) for p in pairs]
    one = exact_pair if stack.dtype.kind in "ui" else float_pair
    flat = np.asarray(labels).ravel()
    order = np.argsort(flat, kind="stable")
    sorted_labels = flat[order]
    starts = np.searchsorted(sorted_labels, np.arange(1, max_label + 2))
    chans = stack.reshape(C, -1)
    out = np.empty((max_label, len(pairs), len(COLS)), np.float64)
    for lab in range(max_label):
        idx = order[starts[lab]:starts[lab + 1]]
        vals = chans[:, idx]
        for p, (i, j) in enumerate(pairs):
            out[lab, p] = one(vals[i], vals[j], float(thr[i]), float(thr[j]))
    return out


def degenerate_scene():
    """(labels (64, 96) int64, stack (4, 64, 96) uint16, what each label is): the rows of the definition table's
    right-hand column.  Channel 0 is random everywhere; the other channels are shaped per cell."""
    rng = np.random.default_rng(11)
    labels = np.zeros((64, 96), np.int64)
    stack = rng.integers(1, 60000, (4, 64, 96)).astype(np.uint16)
    what = {}
    labels[2:12, 3:20] = 1
    stack[1][labels == 1] = 777
    what[1] = "channel 1 constant"
    labels[14:30, 5:15] = 2
    stack[2][labels == 2] = 0
    what[2] = "channel 2 all zero"
    labels[40, 50] = 3
    what[3] = "one pixel"
    labels[33:60, 60:90] = 4
    stack[:, 33:60, 60:90] = rng.integers(0, 100, (4, 27, 30)).astype(np.uint16)
    what[4] = "no positives at threshold 100"
    labels[5:25, 30:55] = 5
    stack[:, 5:25, 30:55] = 0
    what[5] = "every channel zero"
    labels[45:62, 2:40] = 7  # label 6 is absent
    what[6] = "absent"
    what[7] = "ordinary"
    return labels, stack, what


def full_range_plane(size, seed=3):
    """One cell as large as the plane, values 0 and 65535 only (a quarter zeros) plus a second channel pair that is
    all 65535: with size = 2048 the product sums reach 2^22 * 65535^2, just below 2^54."""
    rng = np.random.default_rng(seed)
    labels = np.ones((size, size), np.int64)
    stack = np.full((4, size, size), 65535, np.uint16)
    stack[1][rng.random((size, size)) < 0.25] = 0
    stack[2][rng.random((size, size)) < 0.5] = 0
    return labels, stack
