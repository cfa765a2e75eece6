"""Scores of one segmentation against another, from the two directions of ``SegmentationMask.relate``.

The label images stay on the device: each direction is one ``hipops.relate_labels`` call whose per-label table
(parent, overlap, partners, area) is all that comes back.  ``average_precision`` restates
``cellpose.metrics.average_precision``; cellpose does not exist offline, so parity with it is unpinned, like the other
cellpose restatements of this package.  The matching rule works on the tables alone
(``average_precision_from_relations``) and is pinned against an optimal assignment in the host tests.
"""
from __future__ import annotations

import numpy as np

from .masks import SegmentationMask


def _as_mask(x):
    """A SegmentationMask as it is; a label array as a mask numbered 1..n in ascending order of its values, nothing
    dropped; None for an array without a label."""
    if isinstance(x, SegmentationMask):
        return x
    if not isinstance(x, np.ndarray):
        raise TypeError("expected a SegmentationMask or a numpy label array")
    if x.dtype.kind not in "iu":
        raise TypeError("a label array must have an integer dtype")
    if x.ndim != 2:
        raise ValueError("a label array must be 2D")
    if not x.any():
        return None
    return SegmentationMask(x, remove_edge_cells=False)


def _checked_thresholds(thresholds):
    thresholds = [float(t) for t in np.atleast_1d(thresholds)]
    if any(not t >= 0.5 for t in thresholds):
        raise ValueError("thresholds below 0.5 are not supported: the best-overlap partners only hold every "
                         "candidate pair from IoU 0.5 upwards")
    return thresholds


def _shape(m: SegmentationMask):
    return tuple(m._label_plane()[0].shape)


def iou_from_relations(a_on_b, b_on_a):
    """``intersection_over_union`` from the two relation tables (dicts with ``parent``, ``overlap`` and ``area``;
    the parents of one side number the rows of the other from 1)."""
    out = {}
    for side, mine, theirs in (("a", a_on_b, b_on_a), ("b", b_on_a, a_on_b)):
        parent = np.asarray(mine["parent"], dtype=np.int64)
        overlap = np.asarray(mine["overlap"], dtype=np.int64)
        area = np.asarray(mine["area"], dtype=np.int64)
        other_area = np.concatenate([np.zeros(1, np.int64), np.asarray(theirs["area"], dtype=np.int64)])[parent]
        union = area + other_area - overlap
        iou = np.zeros(parent.shape, np.float64)
        has = parent > 0
        iou[has] = overlap[has].astype(np.float64) / union[has].astype(np.float64)
        out[f"parent_{side}"] = parent
        out[f"iou_{side}"] = iou
    return out


def intersection_over_union(a, b) -> dict:
    """For every label of ``a`` its best-overlap partner in ``b`` and their IoU, and the same for ``b`` in ``a``:
    ``{"parent_a", "iou_a", "parent_b", "iou_b"}``, rows ordered like ``cell_properties``.

    ``a`` and ``b`` are ``SegmentationMask`` objects or non-negative integer label arrays of one shape with at least
    one label each (an array is numbered 1..n in ascending order of its values, as ``SegmentationMask(...,
    remove_edge_cells=False).label_image``; parents use that numbering).  ``parent`` is the label of the other image
    that covers most pixels of this one (the smallest among equal counts), 0 when it lies on background;
    ``iou`` = overlap / (area + area_other[parent] - overlap), 0 without a parent."""
    ma, mb = _as_mask(a), _as_mask(b)
    if ma is None or mb is None:
        raise ValueError("intersection_over_union needs at least one label in both images")
    return iou_from_relations(ma.relate(mb), mb.relate(ma))


def average_precision_from_relations(true_on_pred, pred_on_true, thresholds=(0.5, 0.75, 0.9)):
    """``average_precision`` from the two relation tables -> (ap, tp, fp, fn), one entry per threshold.

    A pair with IoU >= 0.5 shares at least half of either label's pixels and more than half of the smaller one's, so
    it is that label's best-overlap partner: the parents of the two tables hold every candidate pair.  Above 0.5 a
    label has at most one such partner and the pairs are the matching.  At exactly 0.5 a label cut into two exact
    halves by two labels of the other image has two candidates, each of which has no other; it counts once."""
    thresholds = _checked_thresholds(thresholds)
    n_true, n_pred = len(true_on_pred["parent"]), len(pred_on_true["parent"])
    tp = np.zeros(len(thresholds), np.int64)
    if n_true and n_pred:
        pairs = []
        for rel, other, flip in ((true_on_pred, pred_on_true, False), (pred_on_true, true_on_pred, True)):
            parent = np.asarray(rel["parent"], dtype=np.int64)
            rows = np.flatnonzero(parent > 0)
            overlap = np.asarray(rel["overlap"], dtype=np.int64)[rows]
            union = (np.asarray(rel["area"], dtype=np.int64)[rows]
                     + np.asarray(other["area"], dtype=np.int64)[parent[rows] - 1] - overlap)
            mine, theirs = rows + 1, parent[rows]
            pairs.append(np.stack([theirs if flip else mine, mine if flip else theirs, overlap, union], axis=1))
        cand = np.concatenate(pairs)  # (true label, pred label, overlap, union)
        if len(cand):
            cand = np.unique(cand, axis=0)  # each pair once
        for k, t in enumerate(thresholds):
            ok = cand[:, 2].astype(np.float64) / cand[:, 3].astype(np.float64) >= t
            edges = cand[ok]
            shared = sum(int((np.unique(edges[:, c], return_counts=True)[1] == 2).sum()) for c in (0, 1))
            tp[k] = len(edges) - shared
    fp, fn = n_pred - tp, n_true - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        ap = tp.astype(np.float64) / (tp + fp + fn).astype(np.float64)
    return ap, tp, fp, fn


def average_precision(true, pred, thresholds=(0.5, 0.75, 0.9)):
    """Average precision of ``pred`` against ``true`` at IoU thresholds >= 0.5 -> (ap, tp, fp, fn), one entry per
    threshold, with the definitions of ``cellpose.metrics.average_precision``: a true and a predicted label match at
    IoU >= t, tp is the size of the best one-to-one matching, fp = n_pred - tp, fn = n_true - tp and
    ap = tp / (tp + fp + fn) (NaN when both images are empty).  Parity with cellpose is unpinned offline.

    ``true`` and ``pred`` are ``SegmentationMask`` objects or non-negative integer label arrays of one shape; an
    all-zero array is an image without labels.  Both label images are related on the device
    (``SegmentationMask.relate`` in both directions) and no assignment solver runs: see
    ``average_precision_from_relations``.  Thresholds below 0.5 raise ``ValueError``."""
    thresholds = _checked_thresholds(thresholds)
    mt, mp = _as_mask(true), _as_mask(pred)
    empty = {"parent": np.zeros(0, np.int64), "overlap": np.zeros(0, np.int64), "area": np.zeros(0, np.int64)}
    if mt is None or mp is None:
        shapes = [np.shape(x) if isinstance(x, np.ndarray) else _shape(x) for x in (true, pred)]
        if shapes[0] != shapes[1]:
            raise ValueError("true and pred must have the same shape")
        count = lambda m: {k: np.zeros(m.num_cells, np.int64) for k in empty}  # noqa: E731 -- no partner anywhere
        return average_precision_from_relations(empty if mt is None else count(mt), empty if mp is None else count(mp),
                                                thresholds)
    return average_precision_from_relations(mt.relate(mp), mp.relate(mt), thresholds)
