"""Zhang and Suen's thinning rule and the neighbour classes in plain numpy, as include/amt_hip.h states them: integer B and
A from eight shifted views of the zero-padded plane, no word tricks.  Shares nothing with the kernel.  Not collected by
pytest (no test_ prefix)."""
import numpy as np

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
FULL = np.ones((3, 3), np.uint8)
# (dy, dx) of P2 .. P9
RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def neighbours(plane):
    """P2 .. P9 of every pixel as eight int arrays (outside the image: 0)."""
    p = np.asarray(plane) != 0
    H, W = p.shape
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = p
    return [pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in RING]


def sub_iteration(plane, second):
    """-> (the plane after one sub-iteration, the number of pixels it cleared)"""
    p = (np.asarray(plane) != 0).astype(np.uint8)
    P2, P3, P4, P5, P6, P7, P8, P9 = ring = neighbours(p)
    B = sum(ring)
    A = sum(((ring[i] == 0) & (ring[(i + 1) % 8] == 1)).astype(np.int64) for i in range(8))
    if second:
        products = (P2 * P4 * P8 == 0) & (P2 * P6 * P8 == 0)
    else:
        products = (P2 * P4 * P6 == 0) & (P4 * P6 * P8 == 0)
    clear = (p == 1) & (B >= 2) & (B <= 6) & (A == 1) & products
    out = p.copy()
    out[clear] = 0
    return out, int(clear.sum())


def iteration(plane):
    a, n1 = sub_iteration(plane, False)
    b, n2 = sub_iteration(a, True)
    return b, n1 + n2


def skeletonize(plane, max_iter=0):
    """-> (uint8 0 / 1 plane, iterations run: the one that cleared nothing included, or max_iter if that came first)"""
    p = (np.asarray(plane) != 0).astype(np.uint8)
    count = 0
    while max_iter == 0 or count < max_iter:
        p, cleared = iteration(p)
        count += 1
        if cleared == 0:
            break
    return p, count


def neighbor_classes(plane, connectivity=2):
    """0 off the mask, else 1 + the set neighbours (2: eight of them, 1: the four edge neighbours)."""
    p = np.asarray(plane) != 0
    ring = neighbours(p)
    if connectivity == 1:
        ring = ring[0::2]  # P2, P4, P6, P8
    return np.where(p, 1 + sum(ring), 0).astype(np.uint8)
