"""The per-cell skeleton in plain numpy, as include/amt_hip.h states it, twice over and sharing nothing with the kernel:

(a) ``skeletonize`` -- Zhang and Suen's rule on a label plane with "a neighbour is set iff it lies inside the image and
    carries the centre's label": eight shifted views of the padded plane compared with the centre;
(b) ``skeletonize_isolated`` -- tests/skeleton_reference.py's binary rule on ``labels == l`` for every label l, merged, the
    iteration count the maximum over the labels.

And the census of the same-label pixel graph with explicit loops over the offsets.  Not collected by pytest."""
import numpy as np

import skeleton_reference as binary

RING = binary.RING  # (dy, dx) of P2 .. P9
LCEN_COLS = ("pixels", "isolated", "ends", "path", "junctions", "orth_links", "diag_links")


def _same(labels, dy, dx):
    """1 where the pixel carries a label and its neighbour at (dy, dx) lies inside the image and carries the same."""
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    pad = np.full((H + 2, W + 2), np.int64(1) << 40)
    pad[1:-1, 1:-1] = lab
    return ((pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == lab) & (lab != 0)).astype(np.int64)


def sub_iteration(labels, second):
    """-> (the label plane after one sub-iteration, the number of pixels it cleared)"""
    lab = np.asarray(labels).astype(np.int64)
    P2, P3, P4, P5, P6, P7, P8, P9 = ring = [_same(lab, dy, dx) for dy, dx in RING]
    B = sum(ring)
    A = sum(((ring[i] == 0) & (ring[(i + 1) % 8] == 1)).astype(np.int64) for i in range(8))
    if second:
        products = (P2 * P4 * P8 == 0) & (P2 * P6 * P8 == 0)
    else:
        products = (P2 * P4 * P6 == 0) & (P4 * P6 * P8 == 0)
    clear = (lab != 0) & (B >= 2) & (B <= 6) & (A == 1) & products
    out = lab.copy()
    out[clear] = 0
    return out, int(clear.sum())


def iteration(labels):
    a, n1 = sub_iteration(labels, False)
    b, n2 = sub_iteration(a, True)
    return b, n1 + n2


def skeletonize(labels, max_iter=0):
    """(a) -> (plane of the input's dtype: labels[p] on the skeleton of its label, else 0; iterations run, the one that
    cleared nothing included, or max_iter if that came first)"""
    src = np.asarray(labels)
    lab = src.astype(np.int64)
    count = 0
    while max_iter == 0 or count < max_iter:
        lab, cleared = iteration(lab)
        count += 1
        if cleared == 0:
            break
    return lab.astype(src.dtype), count


def skeletonize_isolated(labels, max_iter=0):
    """(b) -> (plane, iterations): every label thinned alone in its plane by the binary rule, the results merged; a plane
    without labels takes the one iteration that clears nothing, as an empty mask does"""
    src = np.asarray(labels)
    out = np.zeros_like(src)
    most = binary.skeletonize(np.zeros(src.shape, np.uint8), max_iter)[1]
    for l in np.unique(src):
        if l == 0:
            continue
        # alone in its plane: thinned on its bounding box, the plane's other pixels are background either way
        ys, xs = np.nonzero(src == l)
        box = (slice(ys.min(), ys.max() + 1), slice(xs.min(), xs.max() + 1))
        skel, n = binary.skeletonize(src[box] == l, max_iter)
        out[box][skel != 0] = l
        most = max(most, n)
    return out, most


def census(labels, max_label):
    """(max_label, 7) int32 in LCEN_COLS order, row l - 1 for label l; values outside 1..max_label own no row"""
    lab = np.asarray(labels).astype(np.int64)
    owns = (lab >= 1) & (lab <= max_label)
    deg = np.zeros(lab.shape, np.int64)
    for dy, dx in RING:
        deg += _same(lab, dy, dx)
    orth = np.zeros(lab.shape, np.int64)
    for dy, dx in ((0, 1), (1, 0)):  # every pair at its left / upper pixel
        orth += _same(lab, dy, dx)
    diag = np.zeros(lab.shape, np.int64)
    for dx in (1, -1):  # p and p + (1, dx), unless p + (0, dx) or p + (1, 0) carries the label too
        diag += _same(lab, 1, dx) * (1 - _same(lab, 0, dx)) * (1 - _same(lab, 1, 0))
    table = np.zeros((max_label, 7), np.int64)
    rows = lab[owns] - 1
    columns = (np.ones(lab.shape, np.int64), deg == 0, deg == 1, deg == 2, deg >= 3, orth, diag)
    for k, plane in enumerate(columns):
        table[:, k] = np.bincount(rows, weights=plane[owns].astype(np.float64), minlength=max_label)[:max_label]
    return table.astype(np.int32)


def cell_skeleton(label_image, num_cells):
    """What SegmentationMask.cell_skeleton returns for labels 1..num_cells, and the skeleton image"""
    skel, _ = skeletonize(label_image)
    t = census(skel, max(num_cells, 1))[:num_cells].astype(np.int64)
    out = {"skeleton_pixels": t[:, 0], "skeleton_isolated": t[:, 1], "skeleton_ends": t[:, 2],
           "skeleton_path_pixels": t[:, 3], "skeleton_junction_pixels": t[:, 4],
           "skeleton_length": t[:, 5].astype(np.float64) + np.sqrt(2.0) * t[:, 6].astype(np.float64)}
    return out, skel
