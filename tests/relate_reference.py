"""numpy reference for relating two label images (AMT_RPX_RELATE, SegmentationMask.relate, metrics).

``relate_columns(a, b, max_label)`` counts the pairs (label of a, value of b) with ``np.unique`` on int64 keys and
reads the four columns off the counts with the C ABI's tie rule (the smallest value among equal counts);
``columns_from_table`` reads the same columns off a dense contingency table such as
``skimage.metrics.contingency_table`` makes (tests/golden/relate.npz).  ``average_precision_assignment`` restates
``cellpose.metrics.average_precision`` with ``scipy.optimize.linear_sum_assignment`` for the matching.
"""
from __future__ import annotations

import numpy as np

RCOLS = ("parent", "overlap", "partners", "area")


def relate_columns(a, b, max_label: int) -> np.ndarray:
    """(max_label, 4) int64 {parent, overlap, partners, area} of labels 1..max_label of ``a`` on ``b``; labels of
    ``a`` outside 1..max_label are ignored, labels absent from ``a`` give four zeros."""
    a = np.asarray(a).astype(np.int64).ravel()
    b = np.asarray(b).astype(np.int64).ravel()
    out = np.zeros((max_label, 4), np.int64)
    inside = (a >= 1) & (a <= max_label)
    a, b = a[inside], b[inside]
    if a.size == 0:
        return out
    base = int(b.max()) + 1
    keys, counts = np.unique(a * base + b, return_counts=True)
    la, vb = keys // base, keys % base
    np.add.at(out[:, 3], la - 1, counts)
    pos = vb > 0
    la, vb, counts = la[pos], vb[pos], counts[pos]
    np.add.at(out[:, 2], la - 1, 1)
    # most pixels first, then the smallest value: the first row of every label in that order is its parent
    order = np.lexsort((vb, -counts, la))
    la, vb, counts = la[order], vb[order], counts[order]
    first = np.ones(la.size, bool)
    first[1:] = la[1:] != la[:-1]
    out[la[first] - 1, 0] = vb[first]
    out[la[first] - 1, 1] = counts[first]
    return out


def contingency(a, b) -> np.ndarray:
    """Dense (max(a) + 1, max(b) + 1) int64 table of pixel counts, row = value of a, column = value of b."""
    a = np.asarray(a).astype(np.int64).ravel()
    b = np.asarray(b).astype(np.int64).ravel()
    t = np.zeros((int(a.max()) + 1, int(b.max()) + 1), np.int64)
    np.add.at(t, (a, b), 1)
    return t


def columns_from_table(table, max_label: int) -> np.ndarray:
    """The four columns of rows 1..max_label of a dense contingency table (row = label, column = companion value)."""
    t = np.asarray(table).astype(np.int64)
    out = np.zeros((max_label, 4), np.int64)
    for l in range(1, min(max_label, t.shape[0] - 1) + 1):
        row = t[l]
        out[l - 1, 3] = row.sum()
        rest = row[1:]
        out[l - 1, 2] = np.count_nonzero(rest)
        if rest.size and rest.max() > 0:
            out[l - 1, 0] = int(np.argmax(rest)) + 1  # argmax returns the first = smallest value
            out[l - 1, 1] = rest.max()
    return out


def relation(a, b, max_label: int) -> dict:
    """``relate_columns`` as the dict ``SegmentationMask.relate`` returns."""
    t = relate_columns(a, b, max_label)
    d = {name: t[:, i].copy() for i, name in enumerate(RCOLS)}
    with np.errstate(divide="ignore", invalid="ignore"):
        d["overlap_fraction"] = d["overlap"].astype(np.float64) / d["area"].astype(np.float64)
    return d


def iou_matrix(true, pred) -> np.ndarray:
    """(n_true, n_pred) float64 IoU of labels 1..max of both images (cellpose.metrics._intersection_over_union
    without the background row and column)."""
    t = contingency(true, pred)
    n_true = t.sum(axis=1, keepdims=True)
    n_pred = t.sum(axis=0, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = t / (n_true + n_pred - t)
    iou[np.isnan(iou)] = 0.0
    return iou[1:, 1:]


def average_precision_assignment(true, pred, thresholds=(0.5, 0.75, 0.9)):
    """cellpose.metrics.average_precision for one image pair numbered 1..n: matches at IoU >= t, tp by optimal
    one-to-one assignment, fp = n_pred - tp, fn = n_true - tp, ap = tp / (tp + fp + fn)."""
    from scipy.optimize import linear_sum_assignment

    true, pred = np.asarray(true), np.asarray(pred)
    n_true, n_pred = int(true.max()), int(pred.max())
    tp = np.zeros(len(thresholds), np.int64)
    if n_true > 0 and n_pred > 0:
        iou = iou_matrix(true, pred)
        n_min = min(iou.shape)
        for k, th in enumerate(thresholds):
            costs = -(iou >= th).astype(float) - iou / (2 * n_min)
            ti, pi = linear_sum_assignment(costs)
            tp[k] = int((iou[ti, pi] >= th).sum())
    fp, fn = n_pred - tp, n_true - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        ap = tp.astype(np.float64) / (tp + fp + fn).astype(np.float64)
    return ap, tp, fp, fn
