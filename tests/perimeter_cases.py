"""The case list of tests/test_gpu_perimeter_scan.py and tests/test_host_perimeter_cases.py: small label planes around
every switch of the perimeter count in ``rp_label_kernel`` (lane layouts, 32-column words, 64-column blocks, bands of
the row-word ring, the wide-box path) and of the box pass ``rp_boxes_kernel`` (16-byte and scalar loads, strips of 256
columns and 30 rows), with the expected values from oracle/regionprops.py.

The perimeter of a label is a function of its own binary image: ``class_counts`` returns the numbers of border pixels
in skimage's three weight classes (weights 1, sqrt 2, (1 + sqrt 2) / 2) the way ``oracle.regionprops.perimeter`` finds
them, and ``expected`` evaluates the perimeter from them in the order of ``rp_final_kernel``.
"""
from __future__ import annotations

import functools
import os
import re
import sys

import numpy as np
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import regionprops as orp  # noqa: E402

C1_CODES, C2_CODES, C3_CODES = (5, 7, 15, 17, 25, 27), (21, 33), (13, 23)
SQ2 = 1.4142135623730951


def _constants():
    """RP_PW (32-bit words of the ring) and RP_LBMAX as amt_props.hip states them."""
    with open(os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc", "amt_props.hip")) as f:
        src = f.read()
    m = re.search(r"constexpr int RP_PW = (\d+), RP_LBMAX = (\d+), RP_WIDE = 32 << RP_LBMAX;", src)
    assert m, "amt_props.hip no longer states RP_PW / RP_LBMAX / RP_WIDE in one line"
    return int(m.group(1)), int(m.group(2))


RP_PW, RP_LBMAX = _constants()
RP_WIDE = 32 << RP_LBMAX  # boxes wider than this take the wide-box path


def band_rows(width: int) -> int:
    """Rows per band of a box of ``width`` columns (rp_band_rows of amt_props.hip): one word per row up to 32 columns,
    two per 64-column block beyond, a row's words padded to a power of two, four rows of the ring kept back."""
    words = 1 if width <= 32 else 2 * ((width + 63) // 64)
    lb = (words - 1).bit_length()
    assert lb <= RP_LBMAX, width
    return (RP_PW >> lb) - 4


# ---- expected values ---------------------------------------------------------------------------------------------------
def code_histogram(image: np.ndarray) -> np.ndarray:
    """Counts of the 3 x 3 codes 1 + 2 a + 10 d over the border pixels of one binary image (50 bins), by the steps of
    ``oracle.regionprops.perimeter``."""
    image = image.astype(np.uint8)
    border = image - ndi.binary_erosion(image, orp.STREL_4, border_value=0)
    pim = ndi.convolve(border, np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode="constant", cval=0)
    return np.bincount(pim[border > 0].ravel(), minlength=50)


def class_counts(image: np.ndarray) -> tuple[int, int, int]:
    h = code_histogram(image)
    return tuple(int(h[list(c)].sum()) for c in (C1_CODES, C2_CODES, C3_CODES))


def perimeter_of_counts(c1, c2, c3):
    """float64, in the order of rp_final_kernel (no fused multiply-add there)."""
    return np.float64(c1) + np.float64(c2) * np.float64(SQ2) + np.float64(c3) * ((1.0 + np.float64(SQ2)) / 2.0)


def clean(plane: np.ndarray, max_label: int) -> np.ndarray:
    """Values outside 1 .. max_label are background for the boxes and "not my label" for the border."""
    p = np.asarray(plane, np.int64)
    return np.where((p >= 1) & (p <= max_label), p, 0)


def expected(plane: np.ndarray, max_label: int) -> dict:
    """Per label 1 .. max_label of one plane: ``present``, inclusive ``bbox`` (max < min where absent), ``area``,
    ``centroid``, the three class ``counts``, ``perimeter`` and the oracle's own ``oracle_perimeter``."""
    lab = clean(plane, max_label)
    out = dict(present=np.zeros(max_label, bool), bbox=np.tile(np.array([2**31 - 1, 2**31 - 1, -1, -1]), (max_label, 1)),
               area=np.zeros(max_label), centroid=np.zeros((max_label, 2)), counts=np.zeros((max_label, 3), np.int64),
               perimeter=np.zeros(max_label), oracle_perimeter=np.zeros(max_label), hist=np.zeros(50, np.int64))
    if not lab.any():
        return out
    ref = orp.regionprops_table(lab, properties=["label", "area", "centroid", "bbox", "perimeter"])
    for k, label in enumerate(ref["label"].astype(np.int64)):
        i = label - 1
        y0, x0, y1, x1 = (int(ref[f"bbox-{j}"][k]) for j in range(4))  # max exclusive
        img = lab[y0:y1, x0:x1] == label
        out["present"][i] = True
        out["bbox"][i] = (y0, x0, y1 - 1, x1 - 1)
        out["area"][i] = ref["area"][k]
        out["centroid"][i] = (ref["centroid-0"][k], ref["centroid-1"][k])
        out["counts"][i] = class_counts(img)
        out["perimeter"][i] = perimeter_of_counts(*out["counts"][i])
        out["oracle_perimeter"][i] = ref["perimeter"][k]
        out["hist"] += code_histogram(img)
    return out


# ---- shapes --------------------------------------------------------------------------------------------------------------
def _noise(rng, h, w, closed=True, p=0.6):
    box = rng.random((h, w)) < p
    if closed:
        box[0, :] = box[-1, :] = box[:, 0] = box[:, -1] = True
    else:
        box[0, 0] = box[-1, -1] = True
    return box


def _shapes(h, w):
    """Five shapes whose bounding box is exactly h x w."""
    yy, xx = np.mgrid[0:h, 0:w]
    solid = np.ones((h, w), bool)
    holes = solid.copy()
    holes[2:h - 1:4, 2:w - 1:5] = False
    lo = yy * max(w - 3, 0) // max(h - 1, 1)
    stairs = (xx >= lo) & (xx < lo + 3)
    checker = (yy + xx) % 2 == 0
    outline = np.zeros((h, w), bool)
    outline[0, :] = outline[-1, :] = outline[:, 0] = outline[:, -1] = True
    c = min(63, w // 2 - 1) if w > 1 else 0  # an outline that crosses the columns 63 / 64 (or the middle of a narrow box)
    outline[0:h:2, c] = True
    outline[1:h:2, min(c + 1, w - 1)] = True
    d = np.minimum(yy + max(c - h // 2, 0), w - 1)
    outline[yy[:, 0], d[:, 0]] = True
    return dict(solid=solid, holes=holes, stairs=stairs, checker=checker, outline=outline)


def _place(H, W, items):
    plane = np.zeros((H, W), np.int32)
    for (y, x, label, img) in items:
        h, w = img.shape
        assert y + h <= H and x + w <= W
        plane[y:y + h, x:x + w][img] = label
    return plane


# ---- the cases: name -> (planes (n, H, W) int32, max_label) -------------------------------------------------------------
THIN = (1, 2, 3, 5, 63, 64, 65, 129)
LAYOUT_WIDTHS = (16, 17, 32, 33, 64, 65, 128, 129)
BAND_WIDTHS = (8, 70, 1100)
MAX_LABELS = (1, 5, 65)
BOX_WIDTHS = (1, 2, 3, 5, 255, 256, 257)


def _band_heights(width):
    b = band_rows(width)
    return (b - 1, b, b + 1, 2 * b + 1, 3 * b + 7)


@functools.lru_cache(maxsize=None)
def perimeter_cases() -> dict:
    rng = np.random.default_rng(20260)
    cases = {}
    # 1. thin shapes: one label that fills the plane
    for n in THIN:
        cases[f"thin_1x{n}"] = (np.ones((1, 1, n), np.int32), 1)
        cases[f"thin_{n}x1"] = (np.ones((1, n, 1), np.int32), 1)
    # 2. the three scan layouts, the 32-column words and the block boundary: one label per plane
    for w in LAYOUT_WIDTHS:
        h = 21
        planes = [_place(h + 4, w + 7, [(2, 3, 1, img)]) for img in _shapes(h, w).values()]
        cases[f"layout_w{w}"] = (np.stack(planes), 1)
    # 3. band heights: one below, at and one above the band, two bands plus one row, more than three bands
    for w in BAND_WIDTHS:
        hs = _band_heights(w)
        planes = [_place(max(hs) + 1, w + 2, [(1, 1, 1, _noise(rng, h, w))]) for h in hs]
        cases[f"bands_w{w}"] = (np.stack(planes), 1)
    # 4. image frame and shared edges
    H, W = 40, 70
    frame = _place(H, W, [(0, 0, 1, _noise(rng, 6, 9)), (0, W - 12, 2, _noise(rng, 7, 12)), (H - 5, 0, 3, _noise(rng, 5, 34)),
                          (H - 9, W - 17, 4, _noise(rng, 9, 17)), (0, 20, 5, _noise(rng, 3, 16)), (H - 2, 40, 6, _noise(rng, 2, 9)),
                          (12, 0, 7, _noise(rng, 12, 1)), (9, W - 1, 8, _noise(rng, 14, 1)), (15, 10, 9, _noise(rng, 6, 40))])
    full = np.ones((H, W), np.int32)
    full[3:H - 2:5, 2:W - 1:7] = 0
    full[10:13, 30:33] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    shared = np.where(xx < np.where(yy < 20, 35, 15 + yy), 1, 2).astype(np.int32)  # a straight and a diagonal edge
    cases["frame"] = (np.stack([frame, full, shared]), 9)
    # 5. ignored values next to a label: above max_label and negative
    ign = np.zeros((12, 40), np.int32)
    ign[2:9, 3:20] = 1
    ign[4:7, 20:30] = 2
    ign[1, 3:20] = 3            # above max_label = 2
    ign[9, 5:15] = 2**31 - 1
    ign[2:9, 2] = -3
    ign[5, 8:12] = -1           # a "hole" of a negative value inside label 1
    ign[0, 39] = 7
    cases["ignored"] = (ign[None], 2)
    # 6. fragmented and nested
    frag = np.zeros((70, 200), np.int32)
    frag[0, 0] = frag[69, 199] = 1
    frag[10:30, 20:50][_noise(rng, 20, 30)] = 2
    frag[35:60, 100:170][_noise(rng, 25, 70, closed=False)] = 3
    ring = np.zeros((30, 40), bool)
    ring[0:3, :] = ring[-3:, :] = ring[:, 0:3] = ring[:, -3:] = True
    frag[32:62, 5:45][ring] = 4
    frag[40:52, 15:33][_noise(rng, 12, 18)] = 5  # its box lies wholly inside the box of label 4
    cases["fragmented"] = (frag[None], 5)
    # 7. batch and numbering: three planes of different content, gaps in the numbering, an all-background plane
    numbers = [1, 2, 5, 9, 33, 64, 65]
    a = _place(50, 90, [(2 + 11 * (i // 3), 1 + 29 * (i % 3), v, _noise(rng, 9, 11 + 8 * (i % 3)))
                        for i, v in enumerate(numbers)])
    b = _place(50, 90, [(5, 7, 5, _noise(rng, 30, 40, closed=False)), (40, 50, 1, _noise(rng, 8, 35))])
    for mx in MAX_LABELS:
        cases[f"batch_max{mx}"] = (np.stack([a, np.zeros_like(a), b]), mx)
    # 8. the wide-box path: one label across a 5-row plane with notches, just over and just under the limit
    for name, w in (("wide_over", RP_WIDE + 37), ("wide_under", RP_WIDE)):
        img = np.ones((5, w), bool)
        img[0, 5:w - 1:97] = img[4, 11:w - 1:61] = img[2, 7:w - 1:113] = False
        img[0:2, 63:66] = False
        img[1, 200:w - 200] = rng.random(w - 400) < 0.7
        cases[name] = (_place(5, w + 3, [(0, 2, 1, img)])[None], 1)
    for planes, _ in cases.values():
        planes.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def expected_of(name: str) -> tuple:
    planes, mx = perimeter_cases()[name]
    return tuple(expected(p, mx) for p in planes)


@functools.lru_cache(maxsize=None)
def box_cases() -> dict:
    """name -> (planes, max_label, misalign): the box pass on its own.  ``misalign`` int32 elements are put in front of
    the planes on the device, so the plane pointer is not 16-byte aligned."""
    rng = np.random.default_rng(20261)
    cases = {}
    for w in BOX_WIDTHS:
        H = 130  # five strips of 30 rows
        p = np.zeros((H, w), np.int32)
        p[rng.random((H, w)) < 0.08] = 1
        p[58:62, :] = 2                     # runs across every lane group and strip of the row, and across two row strips
        p[H - 1, w // 2:] = 3               # only in the last row
        p[5:9, w - 1] = 4                   # only in the last column
        p[100, 0] = 5
        p[20:23, max(w - 7, 0):max(w - 2, 1)] = 6
        cases[f"box_w{w}"] = (p[None], 7, 0)
    H, W = 70, 520
    p = np.zeros((H, W), np.int32)
    p[3, 2:7] = 1           # crosses a four-pixel lane group
    p[5, 250:262] = 2       # crosses the 64-lane boundary (256 columns)
    p[6:9, 255] = 3
    p[6:9, 256] = 4
    p[59:61, 100:300] = 5   # crosses the row strips
    p[H - 1, 511:] = 6
    p[10:40, 300:330][_noise(rng, 30, 30, closed=False)] = 7
    p[30, 0] = p[31, 1] = p[32, 0] = 8
    p[0, 519] = 2**31 - 1
    p[1, 519] = -5
    for mis in (0, 1, 2, 3):
        cases[f"runs_misalign{mis}"] = (np.stack([p, p[::-1, ::-1].copy()]), 8, mis)
    for planes, _, _ in cases.values():
        planes.setflags(write=False)
    return cases


def expected_boxes(planes, max_label) -> np.ndarray:
    return np.stack([expected(p, max_label)["bbox"] for p in planes]).astype(np.int32)
