"""Naive numpy reference of the per-label Haralick texture (include/amt_hip.h, ``AMT_RPX_TEXTURE``): quantisation, the symmetric
grey-level co-occurrence matrices of the four directions and the thirteen features of each, written from the definitions
(Haralick 1973; the columns of ``mahotas.features.haralick``).  ``glcm_loops`` counts pair by pair; ``glcm`` does the same
with shifted views and ``np.bincount`` (the large cases), and tests/test_host_texture.py holds the two together."""
from __future__ import annotations

import numpy as np

COLS = ("angular_second_moment", "contrast", "correlation", "variance", "inverse_difference_moment", "sum_average",
        "sum_variance", "sum_entropy", "entropy", "difference_variance", "difference_entropy", "info_measure_1",
        "info_measure_2")
ANGLES = ("0", "45", "90", "135")
NAN = np.float64("nan")


def offsets(d: int):
    """(dy, dx) of the directions 0, 45, 90, 135 degrees at distance d"""
    return [(0, d), (d, -d), (d, 0), (d, d)]


def quantise(values, lo, hi, L: int) -> np.ndarray:
    """min(L - 1, floor((clip(v, lo, hi) - lo) / (hi - lo) * L)) in float64, in that order; all 0 when hi <= lo"""
    v = np.asarray(values).astype(np.float64)
    lo, hi = float(lo), float(hi)
    if not hi > lo:
        return np.zeros(v.shape, np.int64)
    q = np.floor((np.minimum(np.maximum(v, lo), hi) - lo) / (hi - lo) * float(L))
    return np.minimum(q.astype(np.int64), L - 1)


def glcm_loops(member: np.ndarray, q: np.ndarray, L: int, d: int) -> np.ndarray:
    """(4, L, L) uint32: every unordered pair {p, p + offset} with both ends in ``member`` adds 1 to G[q(p)][q(p + offset)]
    and 1 to the transposed entry.  One pair at a time."""
    H, W = member.shape
    G = np.zeros((4, L, L), np.int64)
    for a, (dy, dx) in enumerate(offsets(d)):
        for y in range(H):
            for x in range(W):
                yy, xx = y + dy, x + dx
                if member[y, x] and 0 <= yy < H and 0 <= xx < W and member[yy, xx]:
                    G[a, q[y, x], q[yy, xx]] += 1
                    G[a, q[yy, xx], q[y, x]] += 1
    return G.astype(np.uint32)


def glcm(member: np.ndarray, q: np.ndarray, L: int, d: int) -> np.ndarray:
    """``glcm_loops`` with shifted views"""
    H, W = member.shape
    G = np.zeros((4, L, L), np.int64)
    for a, (dy, dx) in enumerate(offsets(d)):
        if H - dy <= 0 or W - abs(dx) <= 0:
            continue
        ys, yt = slice(0, H - dy), slice(dy, H)
        xs, xt = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        both = member[ys, xs] & member[yt, xt]
        one = np.bincount(q[ys, xs][both] * L + q[yt, xt][both], minlength=L * L).reshape(L, L)
        G[a] = one + one.T
    return G.astype(np.uint32)


def _entropy(p):
    p = p[p > 0]
    return -(p * np.log2(p)).sum()


def features(G: np.ndarray) -> np.ndarray:
    """The thirteen columns of one (L, L) matrix of counts; NaN when it holds no pair."""
    G = np.asarray(G).astype(np.int64)
    total = int(G.sum())
    if total == 0:
        return np.full(len(COLS), NAN)
    L = G.shape[0]
    N = float(total)
    p = G / N
    i, j = np.mgrid[0:L, 0:L]
    k = np.arange(L, dtype=np.float64)
    ks = np.arange(2 * L - 1, dtype=np.float64)
    rows = G.sum(axis=1)
    px = rows / N
    psum = np.bincount((i + j).ravel(), weights=G.ravel(), minlength=2 * L - 1) / N   # exact integers below 2^53
    pdiff = np.bincount(np.abs(i - j).ravel(), weights=G.ravel(), minlength=L) / N
    mu = (k * px).sum()
    var = ((k - mu) ** 2 * px).sum()
    corr = 1.0 if np.count_nonzero(rows) == 1 else ((i - mu) * (j - mu) * p).sum() / var
    sum_avg = (ks * psum).sum()
    dmean = (k * pdiff).sum()
    hxy = _entropy(p)
    hx = _entropy(px)
    pxpy = np.outer(px, px)
    nz = p > 0
    hxy1 = -(p[nz] * np.log2(pxpy[nz])).sum()
    hxy2 = _entropy(pxpy)
    out = np.empty(len(COLS))
    out[0] = (p * p).sum()
    out[1] = (k * k * pdiff).sum()
    out[2] = corr
    out[3] = var
    out[4] = (p / (1.0 + (i - j) ** 2)).sum()
    out[5] = sum_avg
    out[6] = ((ks - sum_avg) ** 2 * psum).sum()
    out[7] = _entropy(psum)
    out[8] = hxy
    out[9] = ((k - dmean) ** 2 * pdiff).sum()
    out[10] = _entropy(pdiff)
    out[11] = 0.0 if hx == 0 else (hxy - hxy1) / hx
    out[12] = np.sqrt(max(0.0, 1.0 - np.exp(-2.0 * (hxy2 - hxy))))
    return out


def default_ranges(stack: np.ndarray) -> np.ndarray:
    """(C, 2): every channel image's own minimum and maximum"""
    return np.array([[float(ch.min()), float(ch.max())] for ch in stack], dtype=np.float64).reshape(len(stack), 2)


def texture_stack(labels: np.ndarray, stack: np.ndarray, max_label: int, levels: int = 8, distance: int = 1, ranges=None):
    """(table (max_label, C, 4, 13) float64, counts (max_label, C, 4, L, L) uint32) of one label plane and its (C, Y, X)
    stack; ``ranges``: None (each channel's own min and max) or broadcastable to (C, 2).  A label is measured on the crop
    to its bounding box: a partner outside the box cannot carry the label."""
    labels = np.asarray(labels)
    C, L = stack.shape[0], int(levels)
    rng = default_ranges(stack) if ranges is None else np.broadcast_to(np.asarray(ranges, np.float64), (C, 2))
    table = np.full((max_label, C, 4, len(COLS)), NAN)
    counts = np.zeros((max_label, C, 4, L, L), np.uint32)
    for label in range(1, max_label + 1):
        ys, xs = np.nonzero(labels == label)
        if ys.size == 0:
            continue
        box = (slice(ys.min(), ys.max() + 1), slice(xs.min(), xs.max() + 1))
        member = labels[box] == label
        for c in range(C):
            q = quantise(stack[c][box], rng[c, 0], rng[c, 1], L)
            counts[label - 1, c] = glcm(member, q, L, int(distance))
            for a in range(4):
                table[label - 1, c, a] = features(counts[label - 1, c, a])
    return table, counts


def nanmean_angles(table: np.ndarray) -> np.ndarray:
    """(..., 4, 13) -> (..., 13): the mean over the directions that are not NaN; NaN where all four are"""
    valid = ~np.isnan(table)
    count = valid.sum(axis=-2)
    total = np.where(valid, table, 0.0).sum(axis=-2)
    return np.where(count > 0, total / np.maximum(count, 1), NAN)
