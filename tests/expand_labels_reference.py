"""Test-side reference of ``expand_labels`` (not a test module): the distance bound, the rule evaluated separably and
by brute force, and scikit-image's expression restated on scipy.

The rule: a background pixel p is labelled iff ``sqrt(float64(D2(p))) <= distance`` with D2 the exact integer squared
Euclidean distance to the nearest labelled pixel; it receives the label of that pixel, and the SMALLEST label among
the labelled pixels at distance D2(p) when several labels tie.  Labelled pixels keep their label for ``distance >= 0``;
``distance < 0`` gives zeros."""
import numpy as np

_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)  # key of "no labelled pixel": above every (d2 << 32 | label)


def nmax_of(distance):
    """Largest n with ``np.sqrt(np.float64(n)) <= distance`` from ``floor(distance**2)`` corrected by +-1 against that
    very test; -1 when no n qualifies."""
    d = float(distance)
    if not d >= 0:
        return -1
    n = int(np.floor(d * d))
    while n > 0 and not np.sqrt(np.float64(n)) <= d:
        n -= 1
    while np.sqrt(np.float64(n + 1)) <= d:
        n += 1
    return n


def nmax_by_enumeration(distance, limit):
    """max{n in 0..limit : sqrt(n) <= distance}, -1 when empty."""
    n = np.arange(limit + 1, dtype=np.float64)
    ok = np.flatnonzero(np.sqrt(n) <= distance)
    return int(ok[-1]) if ok.size else -1


def _column_pass(lab):
    """Per pixel the nearest labelled pixel of its COLUMN -> (g, label, tied); the smaller label on an up / down tie,
    g = -1 where the column holds no label."""
    H, W = lab.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    has = lab != 0
    up = np.maximum.accumulate(np.where(has, rows, -1), axis=0)
    dn = np.minimum.accumulate(np.where(has, rows, 4 * H)[::-1], axis=0)[::-1]
    big = np.int64(1) << 40
    gu = np.where(up >= 0, rows - up, big)
    gd = np.where(dn < 4 * H, dn - rows, big)
    lu = np.take_along_axis(lab, np.clip(up, 0, H - 1), axis=0)
    ld = np.take_along_axis(lab, np.clip(dn, 0, H - 1), axis=0)
    g = np.minimum(gu, gd)
    both = (gu == gd) & (g < big)
    label = np.where(gu < gd, lu, np.where(gd < gu, ld, np.minimum(lu, ld)))
    tied = both & (lu != ld)
    none = g >= big
    return np.where(none, -1, g), np.where(none, 0, label), tied


def nearest_two_pass(labels):
    """-> (d2, label, tied) per pixel: exact squared distance to the nearest labelled pixel (-1 on a plane without
    labels), the smallest label at that distance, and whether several labels lie at it.  Columns first (nearest
    labelled pixel of the column), then rows: minimum of dx^2 + g^2, the smaller label on equal totals."""
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    if not lab.any():
        return np.full((H, W), -1, np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    g, cl, ctied = _column_pass(lab)
    ckey = np.where(g >= 0, (g * g).astype(np.uint64) << np.uint64(32) | cl.astype(np.uint64), _NONE)
    best, tied = ckey.copy(), ctied.copy()
    shift32 = np.uint64(32)
    for dx in range(1, W):
        finite = best != _NONE
        if finite.all() and dx * dx > int((best >> shift32).max()):
            break
        add = np.uint64(dx * dx) << shift32
        for src, dst in ((slice(dx, W), slice(0, W - dx)), (slice(0, W - dx), slice(dx, W))):
            ck = ckey[:, src]
            cand = np.where(ck != _NONE, ck + add, _NONE)
            b, t = best[:, dst], tied[:, dst]
            same_d = (cand >> shift32 == b >> shift32) & (cand != _NONE)
            less_d = cand >> shift32 < b >> shift32
            t_new = np.where(less_d, ctied[:, src], t | (same_d & ((cand != b) | ctied[:, src])))
            best[:, dst] = np.minimum(b, cand)
            tied[:, dst] = t_new
    d2 = (best >> shift32).astype(np.int64)
    return d2, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), tied


def nearest_brute_force(labels):
    """The same three planes by a search over all labelled pixels (small planes only)."""
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    ys, xs = np.nonzero(lab)
    if ys.size == 0:
        return np.full((H, W), -1, np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    vals = lab[ys, xs]
    py, px = np.mgrid[0:H, 0:W]
    d = (py.reshape(-1, 1) - ys[None, :]) ** 2 + (px.reshape(-1, 1) - xs[None, :]) ** 2
    dmin = d.min(axis=1)
    at_min = d == dmin[:, None]
    lo = np.where(at_min, vals[None, :], np.iinfo(np.int64).max).min(axis=1)
    hi = np.where(at_min, vals[None, :], -1).max(axis=1)
    return dmin.reshape(H, W), lo.reshape(H, W), (lo != hi).reshape(H, W)


def apply_bound(labels, d2, nearest, distance):
    """The expanded label image from (d2, nearest label), in the dtype of ``labels``."""
    labels = np.asarray(labels)
    nmax = nmax_of(distance)
    keep = (d2 >= 0) & (d2 <= nmax)
    return np.where(keep, nearest, 0).astype(labels.dtype)


def expand_two_pass(labels, distance):
    d2, nearest, _ = nearest_two_pass(labels)
    return apply_bound(labels, d2, nearest, distance)


def expand_scipy(labels, distance):
    """scikit-image's ``expand_labels`` restated (SK/segmentation/_expand_labels.py) on scipy's feature transform."""
    from scipy import ndimage as ndi

    labels = np.asarray(labels)
    distances, nearest = ndi.distance_transform_edt(labels == 0, return_indices=True)
    out = np.zeros_like(labels)
    mask = distances <= distance
    out[mask] = labels[tuple(ix[mask] for ix in nearest)]
    return out


def disc_scene(shape, n_discs, seed, max_label=None, radii=(2, 7)):
    """Random discs with labels 1..n_discs (or random distinct labels up to ``max_label``), later discs on top."""
    rng = np.random.default_rng(seed)
    H, W = shape
    lab = np.zeros(shape, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    values = np.arange(1, n_discs + 1) if max_label is None else rng.choice(max_label, n_discs, replace=False) + 1
    for v in values:
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(radii[0], radii[1] + 1)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v
    return lab


DISTANCES = (-1, 0, 0.5, 1, 1.5, 2 ** 0.5, 2, 5 ** 0.5, 2.9999, 3, 4.2, 7, 12, 40)
