"""A numpy reference of the per-label radial distribution as include/amt_hip.h defines it (AMT_RPX_RADIAL): no scipy, no
device code.  d2 is a brute-force integer minimum over every pixel of the zero-framed plane that does not carry the
label; rings and wedges are decided on Python / int64 integers; every column is a scalar float64 loop in the stated
order, so for uint16 images the device must reproduce the bits."""
from __future__ import annotations

import math

import numpy as np

COLS = ("frac_at_d", "mean_frac", "radial_cv")
GEOM_COLS = ("maximum_radius", "mean_radius")
MAX_BINS = 16
GEOM_NCOLS = len(GEOM_COLS) + MAX_BINS
NWEDGES = 8


def distances(lab: np.ndarray, label: int):
    """(ys, xs, d2) of the pixels of ``label`` in raster order: d2 = the smallest squared distance to a pixel of the
    plane framed with one ring of zeros that does not carry the label (int64, exact)."""
    H, W = lab.shape
    framed = np.zeros((H + 2, W + 2), np.int64)
    framed[1:-1, 1:-1] = lab
    own = np.argwhere(framed == label).astype(np.int64)
    other = np.argwhere(framed != label).astype(np.int64)
    d2 = np.empty(len(own), np.int64)
    for at in range(0, len(own), 128):
        diff = own[at:at + 128, None, :] - other[None, :, :]
        d2[at:at + 128] = (diff * diff).sum(axis=-1).min(axis=1)
    return own[:, 0] - 1, own[:, 1] - 1, d2


def rings(d2, bins: int):
    """b(p) = the largest k in 0..bins-1 with d2 B^2 <= dmax2 (B - k)^2, on Python integers"""
    dmax2 = int(max(d2))
    out = []
    for d in (int(v) for v in d2):
        k = bins - 1
        while d * bins * bins > dmax2 * (bins - k) * (bins - k):
            k -= 1
        out.append(k)
    return np.asarray(out, np.int64)


def wedges(ys, xs):
    n, sy, sx = len(ys), int(ys.sum()), int(xs.sum())
    ey, ex = n * ys.astype(np.int64) - sy, n * xs.astype(np.int64) - sx
    return (ey > 0).astype(np.int64) + 2 * (ex > 0) + 4 * (np.abs(ey) > np.abs(ex))


def float_rings(d2, bins: int):
    """the rule a float implementation would use, for the tie cases: floor(B (1 - sqrt(d2) / sqrt(dmax2))), clipped"""
    d = np.sqrt(np.asarray(d2, np.float64))
    return np.clip(np.floor(bins * (1.0 - d / d.max())), 0, bins - 1).astype(np.int64)


def ring_columns(S_bw, n_bw, b: int, n: int):
    """the three columns of ring ``b`` from the float64 (rings, 8) sums -- for uint16 the exact integers converted once,
    with S_b and S summed as integers before -- and the integer (rings, 8) counts"""
    nan = float("nan")
    if S_bw.dtype.kind in "iu":
        Sb, S = float(int(S_bw[b].sum())), float(int(S_bw.sum()))
    else:
        Sb = S = 0.0
        for k in range(S_bw.shape[0]):
            Sk = 0.0
            for w in range(NWEDGES):
                Sk = Sk + float(S_bw[k, w])
            S = S + Sk
            if k == b:
                Sb = Sk
    nb = int(n_bw[b].sum())
    frac = nan if S == 0.0 else Sb / S
    mean_frac = nan if (nb == 0 or S == 0.0) else frac / (float(nb) / float(n))
    means = [float(S_bw[b, w]) / float(int(n_bw[b, w])) for w in range(NWEDGES) if n_bw[b, w]]
    if not means:
        return frac, mean_frac, nan
    total = 0.0
    for m in means:
        total = total + m
    mu = total / float(len(means))
    var = 0.0
    for m in means:
        var = var + (m - mu) * (m - mu)
    var = var / float(len(means))
    return frac, mean_frac, (nan if mu == 0.0 else math.sqrt(var) / mu)


def radial_label(lab, stack, label: int, bins: int):
    """(geometry row (GEOM_NCOLS,), table (C, bins, 3) or None) of one label; ``stack`` is (C, Y, X) or None"""
    C = 0 if stack is None else stack.shape[0]
    geom = np.zeros(GEOM_NCOLS)
    table = None if stack is None else np.full((C, bins, len(COLS)), np.nan)
    ys, xs, d2 = distances(lab, label)
    n = len(ys)
    if n == 0:
        geom[:2] = np.nan
        return geom, table
    b, w = rings(d2, bins), wedges(ys, xs)
    geom[0] = math.sqrt(float(int(d2.max())))
    geom[1] = math.fsum(math.sqrt(float(int(d))) for d in d2) / float(n)  # the exact sum, rounded once
    n_bw = np.zeros((bins, NWEDGES), np.int64)
    np.add.at(n_bw, (b, w), 1)
    geom[2:2 + bins] = n_bw.sum(axis=1)
    for c in range(C):
        v = stack[c][ys, xs]
        if v.dtype.kind in "iu":
            S_bw = np.zeros((bins, NWEDGES), np.int64)
            np.add.at(S_bw, (b, w), v.astype(np.int64))
        else:
            S_bw = np.zeros((bins, NWEDGES), np.float64)
            np.add.at(S_bw, (b, w), v.astype(np.float64))
        for k in range(bins):
            table[c, k] = ring_columns(S_bw, n_bw, k, n)
    return geom, table


def radial_stack(lab, stack, max_label: int, bins: int = 4):
    """(geometry (max_label, GEOM_NCOLS), table (max_label, C, bins, 3) or None) of one label plane"""
    rows = [radial_label(lab, stack, l, bins) for l in range(1, max_label + 1)]
    geom = np.stack([g for g, _ in rows]) if rows else np.zeros((0, GEOM_NCOLS))
    if stack is None:
        return geom, None
    table = np.stack([t for _, t in rows]) if rows else np.zeros((0, stack.shape[0], bins, len(COLS)))
    return geom, table
