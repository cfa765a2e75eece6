"""Plain numpy reference of the neighbour columns (AMT_RPX_NEIGHBORS, AMT_RPX_NEAREST): one label at a time and
deliberately naive -- the ring from eight shifted copies of ``labels == l``, ``np.unique`` for the census, centroids as
``ys.sum() / count``, ``np.lexsort`` and ``np.sqrt`` for the closest labels."""
from __future__ import annotations

import numpy as np

NCOLS = ("count", "touching", "ring", "main")
DCOLS = ("first", "first_distance", "second", "second_distance")
KEYS = ("number_of_neighbors", "touching_pixels", "ring_pixels", "percent_touching", "main_neighbor",
        "first_closest_label", "first_closest_distance", "second_closest_label", "second_closest_distance")


def ring_mask(labels: np.ndarray, l: int) -> np.ndarray:
    """The in-image pixels that do not carry ``l`` and have an 8-neighbour that does."""
    m = labels == l
    H, W = m.shape
    padded = np.zeros((H + 2, W + 2), bool)
    padded[1:-1, 1:-1] = m
    grown = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                grown |= padded[dy:dy + H, dx:dx + W]
    return grown & ~m


def neighbor_values(labels: np.ndarray, comp: np.ndarray, l: int) -> np.ndarray:
    """The multiset N of label ``l``: the positive companion values other than ``l`` on its ring."""
    vals = np.asarray(comp)[ring_mask(labels, l)].astype(np.int64)
    return vals[(vals > 0) & (vals != l)]


def census_columns(labels: np.ndarray, comp: np.ndarray, max_label: int) -> np.ndarray:
    """(max_label, 4) int64 in NCOLS order."""
    out = np.zeros((max_label, 4), np.int64)
    for l in range(1, max_label + 1):
        if not (labels == l).any():
            continue
        vals = neighbor_values(labels, comp, l)
        values, counts = np.unique(vals, return_counts=True)
        main = int(values[np.argmax(counts)]) if len(values) else 0  # argmax: the first, i.e. the smallest value
        out[l - 1] = (len(values), len(vals), int(ring_mask(labels, l).sum()), main)
    return out


def neighbor_sets(labels: np.ndarray, comp: np.ndarray, max_label: int) -> list[set]:
    return [set(neighbor_values(labels, comp, l).tolist()) if (labels == l).any() else set()
            for l in range(1, max_label + 1)]


def centroids(labels: np.ndarray, max_label: int):
    """(cy, cx, present) of the labels 1..max_label; an absent label has NaN centroids."""
    cy = np.full(max_label, np.nan)
    cx = np.full(max_label, np.nan)
    for l in range(1, max_label + 1):
        ys, xs = np.nonzero(labels == l)
        if len(ys):
            cy[l - 1] = ys.sum() / len(ys)
            cx[l - 1] = xs.sum() / len(xs)
    return cy, cx, ~np.isnan(cy)


def nearest_d2(labels: np.ndarray, max_label: int):
    """((max_label, 2) int64 labels, (max_label, 2) float64 squared distances) of the two nearest present labels by
    centroid, ordered by (d2, label); 0 / NaN where there is none."""
    return closest(*centroids(labels, max_label))


def closest(cy: np.ndarray, cx: np.ndarray, present: np.ndarray):
    """``nearest_d2`` from the centroids of the labels 1..len(cy)."""
    max_label = len(cy)
    who = np.zeros((max_label, 2), np.int64)
    d2s = np.full((max_label, 2), np.nan)
    for l in range(1, max_label + 1):
        if not present[l - 1]:
            continue
        m = np.flatnonzero(present) + 1
        m = m[m != l]
        dy = cy[m - 1] - cy[l - 1]
        dx = cx[m - 1] - cx[l - 1]
        d2 = dy * dy + dx * dx
        order = np.lexsort((m, d2))[:2]
        who[l - 1, :len(order)] = m[order]
        d2s[l - 1, :len(order)] = d2[order]
    return who, d2s


def nearest_columns(labels: np.ndarray, max_label: int) -> np.ndarray:
    """(max_label, 4) float64 in DCOLS order."""
    who, d2 = nearest_d2(labels, max_label)
    out = np.empty((max_label, 4), np.float64)
    out[:, 0::2] = who
    out[:, 1::2] = np.sqrt(d2)
    return out


def cell_neighbors(label_image: np.ndarray, k: int, census_labels=None, other=None) -> dict:
    """``SegmentationMask.cell_neighbors`` restated: the census on ``census_labels`` (the grown label image; default
    the label image itself) against ``other`` (default ``census_labels``), the closest columns on ``label_image``."""
    grown = label_image if census_labels is None else census_labels
    cen = census_columns(grown, grown if other is None else other, k)
    near = nearest_columns(label_image, k)
    touching, ring = cen[:, 1], cen[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        percent = 100.0 * touching.astype(np.float64) / ring.astype(np.float64)
    return {"number_of_neighbors": cen[:, 0], "touching_pixels": touching, "ring_pixels": ring,
            "percent_touching": percent, "main_neighbor": cen[:, 3],
            "first_closest_label": near[:, 0].astype(np.int64), "first_closest_distance": near[:, 1],
            "second_closest_label": near[:, 2].astype(np.int64), "second_closest_distance": near[:, 3]}
