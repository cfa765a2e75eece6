"""Plain numpy statements of the four spot rules of include/amt_hip.h (amt_rank_filter ops 15 .. 18) and of the functions
composed from them (``operations.peak_local_max`` / ``detect_spots``, ``SegmentationMask.cell_spots``).  Slow, obvious, and
independent of the package: the only import from the repository is the oracle's Gaussian for the response.  Not collected
by pytest (no test_ prefix)."""
from __future__ import annotations

import numpy as np

COLS = ("value", "dy", "dx", "sum", "n", "ring_sum", "ring_n")
NCOLS = len(COLS)
MAX_RADIUS = 15


def spot_capacity(H, W, r):
    return -(-H // (r + 1)) * -(-W // (r + 1))


def local_maxima(a, r, t=0.0, b=0):
    """(H, W) uint8: p is marked iff a(p) > t, a(p) >= a(q) for every q within Chebyshev distance r inside the image,
    a(p) > a(q) for those q that precede p in raster order, and p lies at least b pixels from every edge.  A loop over the
    (2 r + 1)^2 - 1 offsets; positions outside the image are -inf (less than everything)."""
    a = np.asarray(a)
    H, W = a.shape
    v = a.astype(np.float64)  # uint16 -> float64 is exact
    p = np.full((H + 2 * r, W + 2 * r), -np.inf)
    p[r:r + H, r:r + W] = v
    ok = v > t
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0:
                continue
            q = p[r + dy:r + dy + H, r + dx:r + dx + W]
            earlier = dy < 0 or (dy == 0 and dx < 0)
            ok &= (v > q) if earlier else (v >= q)
    yy, xx = np.mgrid[0:H, 0:W]
    ok &= (yy >= b) & (yy < H - b) & (xx >= b) & (xx < W - b)  # the border test comes last
    return ok.astype(np.uint8)


def mask_list(mask, capacity=None):
    """(capacity + 1,) int32: the true count, the first min(count, capacity) of np.flatnonzero, then -1"""
    mask = np.asarray(mask)
    capacity = mask.size if capacity is None else capacity
    idx = np.flatnonzero(mask)
    out = np.full(capacity + 1, -1, np.int32)
    out[0] = len(idx)
    n = min(len(idx), capacity)
    out[1:1 + n] = idx[:n]
    return out


def _entries(lst, HW):
    """the list's entries with -1 past min(count, capacity), for -1 entries and for indices outside the plane"""
    lst = np.asarray(lst)
    cap = len(lst) - 1
    kept = min(max(int(lst[0]), 0), cap)
    out = np.full(cap, -1, np.int64)
    out[:kept] = lst[1:1 + kept]
    out[(out < 0) | (out >= HW)] = -1
    return out


def parabola_offset(am, a0, ap):
    """the vertex of the parabola through (-1, am), (0, a0), (1, ap): each operation rounded once, in this order"""
    am, a0, ap = np.float64(am), np.float64(a0), np.float64(ap)
    den = (am - a0) + (ap - a0)
    if den >= 0:
        return np.float64(0.0)
    return np.float64(min(max((np.float64(0.5) * (am - ap)) / den, -0.5), 0.5))


def spot_measure(a, lst, k, bounds=False):
    """(capacity, 7) float64, NaN rows for absent entries.  With ``bounds`` also (capacity, 2): twice n * 2^-52 * sum|v|
    for the spot's and the ring's sum -- what two float64 sums of the same n terms in different fixed orders may differ
    by (0 for uint16, whose sums are exact integers)."""
    a = np.asarray(a)
    H, W = a.shape
    ent = _entries(lst, H * W)
    out = np.full((len(ent), NCOLS), np.nan)
    bound = np.zeros((len(ent), 2))
    exact = a.dtype.kind in "ui"
    for j, p in enumerate(ent):
        if p < 0:
            continue
        y, x = divmod(int(p), W)
        dy = parabola_offset(a[y - 1, x], a[y, x], a[y + 1, x]) if 0 < y < H - 1 else 0.0
        dx = parabola_offset(a[y, x - 1], a[y, x], a[y, x + 1]) if 0 < x < W - 1 else 0.0
        y0, y1, x0, x1 = max(y - k - 2, 0), min(y + k + 3, H), max(x - k - 2, 0), min(x + k + 3, W)
        big = a[y0:y1, x0:x1]
        yy, xx = np.mgrid[y0:y1, x0:x1]
        inner = (np.abs(yy - y) <= k) & (np.abs(xx - x) <= k)
        parts = []
        for sel in (inner, ~inner):
            vals = big[sel]
            if exact:
                parts += [float(int(vals.astype(np.int64).sum())), float(vals.size), 0.0]
            else:
                parts += [float(np.sum(vals.astype(np.float64))) if vals.size else 0.0, float(vals.size),
                          2.0 * vals.size * 2.0 ** -52 * float(np.abs(vals).sum())]
        out[j] = (float(a[y, x]), dy, dx, parts[0], parts[1], parts[3], parts[4])
        bound[j] = (parts[2], parts[5])
    return (out, bound) if bounds else out


def take_at(a, lst):
    """(capacity,) of a's dtype: a at the list's entries, 0 for absent ones"""
    a = np.asarray(a)
    ent = _entries(lst, a.size)
    out = np.zeros(len(ent), a.dtype)
    out[ent >= 0] = a.reshape(-1)[ent[ent >= 0]]
    return out


# ---- the composed functions ---------------------------------------------------------------------------------------------
def peak_local_max(image, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=True, num_peaks=np.inf):
    image = np.asarray(image)
    r = min_distance
    b = (r if exclude_border else 0) if isinstance(exclude_border, bool) else exclude_border
    t = float(image.min()) if threshold_abs is None else float(threshold_abs)
    if threshold_rel is not None:
        t = max(t, float(threshold_rel) * float(image.max()))
    idx = np.flatnonzero(local_maxima(image, r, t, b))
    order = np.argsort(-image.reshape(-1)[idx].astype(np.float64), kind="stable")
    idx = idx[order]
    if num_peaks != np.inf:
        idx = idx[:num_peaks]
    return np.stack([idx // image.shape[1], idx % image.shape[1]], axis=1).astype(np.int64).reshape(-1, 2)


def response_of(image, sigma):
    """difference_of_gaussians(image, sigma, 1.6 sigma) by the oracle's Gaussian; the image itself for sigma None"""
    if sigma is None:
        return np.asarray(image)
    from oracle import skops

    return skops.difference_of_gaussians(np.asarray(image), sigma, 1.6 * sigma)


def detect_spots(image, sigma=1.5, min_distance=2, threshold=None, snr=5.0, radius=2, exclude_border=None, labels=None,
                 intensity=None):
    image = np.asarray(image)
    resp = response_of(image, sigma)
    if threshold is None:
        p25, p50, p75 = (float(v) for v in np.percentile(resp, [25, 50, 75]))
        threshold = p50 + float(snr) * (p75 - p25) / 1.349
    b = min_distance if exclude_border is None else exclude_border
    lst = mask_list(local_maxima(resp, min_distance, float(threshold), b))
    n = int(lst[0])
    lst = lst[:max(n, 1) + 1]
    idx = lst[1:1 + n].astype(np.int64)
    W = image.shape[1]
    on_resp = spot_measure(resp, lst, radius)[:n]
    on_int = spot_measure(image if intensity is None else np.asarray(intensity), lst, radius)[:n]
    row, col = idx // W, idx % W
    with np.errstate(invalid="ignore", divide="ignore"):
        background = on_int[:, 5] / on_int[:, 6]
    out = {"row": row, "col": col, "y": row + on_resp[:, 1], "x": col + on_resp[:, 2], "response": on_resp[:, 0].copy(),
           "intensity_sum": on_int[:, 3].copy(), "background_mean": background,
           "intensity_net": on_int[:, 3] - on_int[:, 4] * background}
    if labels is not None:
        out["label"] = take_at(np.asarray(labels), lst)[:n].astype(np.int64)
    return out


def cell_spots(table, num_cells, name):
    label = table["label"]
    inside = (label >= 1) & (label <= num_cells)
    count = np.zeros(num_cells, np.int64)
    total = np.zeros(num_cells, np.float64)
    for lab, net in zip(label[inside], table["intensity_net"][inside]):  # in list order, as np.bincount adds
        count[lab - 1] += 1
        total[lab - 1] += net
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count > 0, total / np.maximum(count, 1), np.nan)
    return {f"spot_count_{name}": count, f"spot_intensity_sum_{name}": total, f"spot_intensity_mean_{name}": mean}
