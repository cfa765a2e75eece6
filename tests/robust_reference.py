"""numpy statement of AMT_RPX_ROBUST (include/amt_hip.h): per label the 25th / 50th / 75th percentile of a channel and
the raw median absolute deviation, each by ``np.percentile`` with linear interpolation.  MAD is the 50th PERCENTILE of
the absolute differences in float64, not ``np.median``: for an even count those differ in the last bit on float data.
"""
from __future__ import annotations

import numpy as np

COLS = ("q25", "median", "q75", "mad")


def robust_row(values) -> np.ndarray:
    """(4,) float64 of a 1-D multiset of pixel values; four NaNs for an empty one."""
    v = np.asarray(values)
    if v.size == 0:
        return np.full(4, np.nan)
    q25, med, q75 = (np.percentile(v, q) for q in (25, 50, 75))
    mad = np.percentile(np.abs(v.astype(np.float64) - np.float64(med)), 50)
    return np.array([q25, med, q75, mad], dtype=np.float64)


def robust_columns(labels, image, k: int) -> np.ndarray:
    """(k, 4) float64: row l - 1 describes the pixels of ``image`` where ``labels == l``; NaN rows for absent labels."""
    labels = np.asarray(labels)
    image = np.asarray(image)
    out = np.empty((k, 4), np.float64)
    for l in range(1, k + 1):
        out[l - 1] = robust_row(image[labels == l])
    return out


def robust_stack(labels, stack, k: int) -> np.ndarray:
    """(k, C, 4) of a (C, Y, X) stack"""
    return np.stack([robust_columns(labels, ch, k) for ch in stack], axis=1)


def sort_and_index_row(values) -> np.ndarray:
    """The same four numbers from a full sort and the rank rule written out: virtual index (n - 1) q / 100, and
    numpy's lerp a + (b - a) t, taken from the other end for t >= 0.5."""
    v = np.sort(np.asarray(values).astype(np.float64))
    if v.size == 0:
        return np.full(4, np.nan)

    def pct(s, q):
        n = len(s)
        virt = (n - 1) * (q / 100.0)
        lo = int(np.floor(virt))
        hi = min(lo + 1, n - 1)
        t = virt - lo
        a, b = s[lo], s[hi]
        d = b - a
        return b - d * (1.0 - t) if t >= 0.5 else a + d * t

    med = pct(v, 50)
    return np.array([pct(v, 25), med, pct(v, 75), pct(np.sort(np.abs(v - med)), 50)], dtype=np.float64)
