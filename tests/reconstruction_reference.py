"""Two independent numpy statements of grey reconstruction as include/amt_hip.h defines it (ops 3 .. 6 of
amt_rank_filter), sharing nothing with the library:

(a) ``naive``  the fixed point itself: iterate R <- min(mask, grey_dilation(R)) from R = seed with scipy until nothing
               changes (by erosion: max(mask, grey_erosion(R))); the padding is the neutral value, so nothing comes from
               outside the image.  ~H + W sweeps on benign planes, ~10^4 on a serpentine: small planes only.
(b) ``flood``  a max-heap flood: pop the largest pixel, push min(R[p], mask[q]) into every neighbour q it raises.  One
               pass over the plane; this is the one used on the larger planes.  Erosion runs on the negated images.

``path_formula`` is the closed form R(p) = max_q min(seed(q), w(p, q)), w = the widest path under the mask, by brute
force (Floyd-Warshall on the pixel graph): planes up to 6 x 6.  ``WORKED`` is a 5 x 7 example worked by hand.
"""
import heapq

import numpy as np
from scipy import ndimage as ndi

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
ONES = np.ones((3, 3), np.uint8)
FOOTPRINTS = {"cross": CROSS, "ones": ONES}


def _offsets(fp):
    return [(dy - 1, dx - 1) for dy in range(3) for dx in range(3) if fp[dy, dx] and (dy, dx) != (1, 1)]


def naive(seed, mask, fp, method="dilation"):
    dt = seed.dtype
    r, m = seed.astype(np.float64), mask.astype(np.float64)
    while True:
        if method == "dilation":
            n = np.minimum(m, ndi.grey_dilation(r, footprint=fp, mode="constant", cval=-np.inf))
        else:
            n = np.maximum(m, ndi.grey_erosion(r, footprint=fp, mode="constant", cval=np.inf))
        if np.array_equal(n, r):
            return r.astype(dt)
        r = n


def flood(seed, mask, fp, method="dilation"):
    dt = seed.dtype
    sign = 1.0 if method == "dilation" else -1.0
    r = (sign * seed.astype(np.float64)).tolist()
    m = (sign * mask.astype(np.float64)).tolist()
    H, W = seed.shape
    offs = _offsets(fp)
    heap = [(-r[y][x], y, x) for y in range(H) for x in range(W)]
    heapq.heapify(heap)
    while heap:
        v, y, x = heapq.heappop(heap)
        v = -v
        if v != r[y][x]:
            continue  # a stale entry: the pixel was raised after this one was pushed
        for dy, dx in offs:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W:
                c = v if v < m[yy][xx] else m[yy][xx]
                if c > r[yy][xx]:
                    r[yy][xx] = c
                    heapq.heappush(heap, (-c, yy, xx))
    return (sign * np.array(r, np.float64).reshape(H, W)).astype(dt)


def path_formula(seed, mask, fp):
    """reconstruction by dilation from the path formula, brute force"""
    H, W = seed.shape
    n = H * W
    m = mask.astype(np.float64).reshape(-1)
    w = np.full((n, n), -np.inf)
    for y in range(H):
        for x in range(W):
            p = y * W + x
            w[p, p] = m[p]
            for dy, dx in _offsets(fp):
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W:
                    w[p, yy * W + xx] = min(m[p], m[yy * W + xx])
    for k in range(n):
        w = np.maximum(w, np.minimum(w[:, k:k + 1], w[k:k + 1, :]))
    s = seed.astype(np.float64).reshape(-1)
    return np.max(np.minimum(s[None, :], w), axis=1).reshape(H, W).astype(seed.dtype)


def dual(a):
    """the image whose reconstruction by erosion mirrors the reconstruction by dilation of ``a``"""
    return (65535 - a).astype(np.uint16) if a.dtype == np.uint16 else 0.0 - a  # 0.0 - 0.0 is +0.0: no -0.0 appears


def h_seed(a, h, method="dilation"):
    """the seed of ops 5 / 6: saturating for uint16, one rounding for float64"""
    if a.dtype == np.uint16:
        w = a.astype(np.int64) + (-int(h) if method == "dilation" else int(h))
        return np.clip(w, 0, 65535).astype(np.uint16)
    return a - h if method == "dilation" else a + h


def h_extrema(a, h, fp, maxima=True):
    """the mask rule of include/amt_hip.h: uint16 residue >= h, float64 R == seed"""
    method = "dilation" if maxima else "erosion"
    s = h_seed(a, h, method)
    r = flood(s, a, fp, method)
    if a.dtype == np.uint16:
        res = a.astype(np.int64) - r if maxima else r.astype(np.int64) - a
        return (res >= int(h)).astype(np.uint8)
    return (r == s).astype(np.uint8)


# ---- a 5 x 7 example worked by hand ------------------------------------------------------------------------------
# Two plateaus (5 and 7) in a floor of 1, a pixel of 9 below the 7s, and a pixel of 8 that touches both plateaus only
# diagonally.  The seed 4 fills the 5-plateau to 4 and the floor to 1; the seed 6 fills the 7-plateau and the 9 below it
# to 6.  Under the cross the 8 sees only floor (1).  Under all-ones it takes max(4, 6) = 6 from the plateaus' corners and
# hands min(5, 6) = 5 back to the 5-plateau.
WORKED_MASK = np.array([[1, 1, 1, 1, 1, 1, 1],
                        [1, 5, 5, 1, 7, 7, 1],
                        [1, 5, 5, 1, 7, 7, 1],
                        [1, 1, 1, 8, 1, 9, 1],
                        [1, 1, 1, 1, 1, 1, 1]], np.uint16)
WORKED_SEED = np.zeros((5, 7), np.uint16)
WORKED_SEED[1, 1] = 4
WORKED_SEED[2, 5] = 6
WORKED = {
    "cross": np.array([[1, 1, 1, 1, 1, 1, 1],
                       [1, 4, 4, 1, 6, 6, 1],
                       [1, 4, 4, 1, 6, 6, 1],
                       [1, 1, 1, 1, 1, 6, 1],
                       [1, 1, 1, 1, 1, 1, 1]], np.uint16),
    "ones": np.array([[1, 1, 1, 1, 1, 1, 1],
                      [1, 5, 5, 1, 6, 6, 1],
                      [1, 5, 5, 1, 6, 6, 1],
                      [1, 1, 1, 6, 1, 6, 1],
                      [1, 1, 1, 1, 1, 1, 1]], np.uint16),
}
