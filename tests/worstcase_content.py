"""Worst-case CONTENT for the labelling, EDT, peak, expand and watershed kernels, the census that says which side of each
content switch an input is on, and the runner of the cases.

The kernels of amt_label.hip / amt_watershed.hip (and the run tables of amt_internal.h) switch on what a plane holds, not
only on its shape: runs per 64 x 64 tile (XR_CAP / SR_CAP: LDS table or per-pixel gather; RT_CAP and 32 runs per row: the
tables' own capacity), components per plane (row_stride = n / 2 + 1), a component's box and largest d2 (flood classes
S / M / M2 / L / X / G), marker label values (16-bit labels in LDS), heap occupancy (GH_LDS_N slots in LDS, the rest in
HBM).  ``PATTERNS`` are deterministic boolean planes for any (H, W) that sit on the far side of those switches;
``census(plane)`` measures the facts on the host; ``limits()`` reads the constants from the kernel sources.

``run(ctx, groups, scratch_check)`` runs the cases on the device and returns one record per case, in the form of
tests/operator_sweep.py (whose Recorder, rules and digest it uses): every result is compared bit for bit with the
reference of the operator's own test (oracle.skops, oracle.watershed, expand_labels_reference).

``python -m tests.worstcase_content --json PATH`` runs everything and writes the records and the scratch findings.  Not
collected by pytest (tests/test_host_worstcase_content.py and tests/test_gpu_worstcase_content.py are)."""
from __future__ import annotations

import heapq
import json
import os
import re
import sys
import time

import numpy as np
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import expand_labels_reference as expand_ref  # noqa: E402
import operator_sweep as sw  # noqa: E402
import poison_child  # noqa: E402
from oracle import skops  # noqa: E402

_I32, _U8, _F64 = np.int32, np.uint8, np.float64

# (192, 192): 3 x 3 whole tiles (one has all eight neighbours); a one-component pattern's box is above X_PX: class G
# (130, 144): W % 16 == 0 and n % 16 == 0, the run-table paths; tiles cut by both edges; the whole-plane box is class L
# (129, 131): the parent-plane paths; the checkerboard has exactly n / 2 + 1 components
SHAPES = [(192, 192), (130, 144), (129, 131)]
CSRC = os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------
# the limits, read from the kernel sources
# ---------------------------------------------------------------------------------------------------------------------
def limits():
    """The constants the content switches compare with, by pattern from the sources: a retune changes what this
    returns, and tests/test_host_worstcase_content.py then says which inputs no longer straddle it."""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("amt_label.hip", "amt_watershed.hip", "amt_internal.h")}

    def const(f, name):
        m = re.search(r"constexpr int (?:\w+ = \d+, )*" + name + r" = (\d+)[,;]", src[f])
        assert m, f"{name} not found in {f}"
        return int(m.group(1))

    out = {"XR_CAP": const("amt_label.hip", "XR_CAP"), "SR_CAP": const("amt_watershed.hip", "SR_CAP"),
           "RT_CAP": const("amt_internal.h", "RT_CAP"), "GH_LDS_N": const("amt_watershed.hip", "GH_LDS_N")}
    for c in ("S", "M", "M2", "L", "X"):
        out[c + "_PX"], out[c + "_NB"] = const("amt_watershed.hip", c + "_PX"), const("amt_watershed.hip", c + "_NB")
    out["PF_SLOT"], out["PF_SLOTS"] = const("amt_watershed.hip", "PF_SLOT"), const("amt_watershed.hip", "PF_SLOTS")
    assert "(npx2 * 4 + nq2 * 2 + nb2 * 6 + PF_SLOT - 1) / PF_SLOT" in src["amt_watershed.hip"]  # pf_slots_needed restates it
    m = re.search(r"S\[64 \* (\d+)\]", src["amt_label.hip"])
    assert m and "row << 5" in src["amt_label.hip"], "the run union-find's S[64 * 32] / row << 5 packing"
    out["ROW_RUNS"] = int(m.group(1))
    m = re.search(r"c\.labmax >= (0x[0-9A-Fa-f]+)\) cls = CLS_G", src["amt_watershed.hip"])
    assert m, "the 16-bit label rule of ws_classify_kernel"
    out["LAB16"] = int(m.group(1), 16)
    assert re.search(r"row_stride = n / 2 \+ 1;", src["amt_watershed.hip"]), "row_stride = n / 2 + 1"
    # the classify rule itself: the census restates it (flood_class), so its text is pinned here
    for c in ("S", "M", "M2", "L", "X"):
        assert f"area <= {c}_PX && c.cmax < {c}_NB) cls = CLS_{c};" in src["amt_watershed.hip"], c
    assert "(c.x1 - c.x0 + 3) * (c.y1 - c.y0 + 3)" in src["amt_watershed.hip"]
    return out


def flood_class(lim, area, cmax, labmin, labmax, mcnt):
    """ws_classify_kernel's rule for the d2 relief: '-' no marker, 'U' one label, else S / M / M2 / L / X / G."""
    if mcnt == 0:
        return "-"
    if labmin == labmax:
        return "U"
    if labmax >= lim["LAB16"]:
        return "G"
    for c in ("S", "M", "M2", "L", "X"):
        if area <= lim[c + "_PX"] and cmax < lim[c + "_NB"]:
            return c
    return "G"


def pf_slots_needed(lim, area, cmax, npix):
    """LDS slots ws_flood_persist_kernel reserves for a component of class S / M / M2 / L (npix = 0: not counted, the
    parent-plane statistics).  A component that needed more than PF_SLOTS would leave its wave spinning for ever."""
    even = lambda v: (v + 1) & ~1  # noqa: E731
    return (even(area) * 4 + even(npix if npix > 0 else area) * 2 + even(cmax + 1) * 6 + lim["PF_SLOT"] - 1) // lim["PF_SLOT"]


# ---------------------------------------------------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------------------------------------------------
def _grid(H, W):
    return np.mgrid[0:H, 0:W]


def _checker(phase):
    return lambda H, W: (lambda g: (g[0] + g[1]) % 2 == phase)(_grid(H, W))


def _cols(phase):
    return lambda H, W: np.broadcast_to(np.arange(W) % 2 == phase, (H, W)).copy()


def _rows(H, W):
    return np.broadcast_to((np.arange(H) % 2 == 0)[:, None], (H, W)).copy()


def _comb(top):
    def f(H, W):
        m = _cols(0)(H, W)
        m[0 if top else H - 1] = True
        return m
    return f


def _serpentine(H, W):
    """Alternate rows joined at alternating ends: one one-pixel-wide component whose box is the whole plane."""
    m = _rows(H, W)
    for y in range(1, H, 2):
        if y + 1 < H:
            m[y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    return m


def _rings(H, W):
    y, x = _grid(H, W)
    return np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x)) % 2 == 0


def _spiral(H, W):
    """A one-pixel square spiral from the top-left corner inwards, one pixel of background between its turns."""
    m = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx  # the pixel after the next one: stop one short of an earlier turn
        if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
            y, x = ny, nx
            m[y, x] = True
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return m


def _diag(kind):
    def f(H, W):
        y, x = _grid(H, W)
        if kind == "diag":
            return (y - x) % 4 == 0
        if kind == "anti":
            return (y + x) % 4 == 0
        return ((y - x) % 8 == 0) | ((y + x) % 8 == 0)
    return f


def _frame(H, W):
    m = np.zeros((H, W), bool)
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    return m


def _corners(anti):
    """Pixels only where four 64 x 64 tiles meet: the diagonal pair (63, 63), (64, 64) or the pair (63, 64), (64, 63)."""
    def f(H, W):
        m = np.zeros((H, W), bool)
        for cy in range(64, H, 64):
            for cx in range(64, W, 64):
                if anti:
                    m[cy - 1, cx] = m[cy, cx - 1] = True
                else:
                    m[cy - 1, cx - 1] = m[cy, cx] = True
        return m
    return f


def _seam_zip(H, W):
    """Column 63 on even rows and column 64 on odd rows at every tile seam: a component that crosses the seam on every row."""
    m = np.zeros((H, W), bool)
    for c in range(64, W, 64):
        m[0::2, c - 1] = True
        m[1::2, c] = True
    return m


def _noise(H, W):
    return np.random.default_rng([H, W, 50]).random((H, W)) < 0.5


THIN = {
    "checker0": _checker(0), "checker1": _checker(1), "cols0": _cols(0), "cols1": _cols(1), "rows": _rows,
    "comb_bottom": _comb(False), "comb_top": _comb(True), "serpentine": _serpentine, "rings": _rings, "spiral": _spiral,
    "diag4": _diag("diag"), "anti4": _diag("anti"), "crossed8": _diag("crossed"), "full": lambda H, W: np.ones((H, W), bool),
    "frame": _frame, "corners": _corners(False), "corners_anti": _corners(True), "seam_zip": _seam_zip, "noise50": _noise,
}


def _thick(fn):
    """The pattern of a third of the shape, every pixel a 3 x 3 block, cropped: distances, peak plateaus and floods exist."""
    return lambda H, W: np.kron(fn(-(-H // 3), -(-W // 3)), np.ones((3, 3), bool))[:H, :W].astype(bool)


def _thick_in_place(fn):
    """For the patterns tied to the tile seams (a third of the shape has its seams elsewhere, or none): every pixel grows
    to the 3 x 3 block around it, so the thick pattern still straddles the seams of the full plane."""
    return lambda H, W: ndi.binary_dilation(fn(H, W), np.ones((3, 3), bool))


SEAM_PATTERNS = ("corners", "corners_anti", "seam_zip")
PATTERNS = dict(THIN)
PATTERNS.update({name + "_x3": (_thick_in_place if name in SEAM_PATTERNS else _thick)(fn) for name, fn in THIN.items()})
_PLANES: dict = {}


def plane(name, shape):
    """The boolean plane of a pattern (made once, read-only)."""
    key = (name, tuple(shape))
    if key not in _PLANES:
        m = np.ascontiguousarray(PATTERNS[name](*shape), bool)
        assert m.shape == tuple(shape), key
        m.setflags(write=False)
        _PLANES[key] = m
    return _PLANES[key]


def values_plane(mask):
    """An int32 image on the mask's support in which neighbouring runs of a row hold different values."""
    left = np.zeros_like(mask)
    left[:, 1:] = mask[:, :-1]
    ordinal = np.cumsum((mask & ~left).ravel()).reshape(mask.shape)
    return np.where(mask, 1 + ordinal % 3, 0).astype(_I32)


# ---- the class-limit planes -----------------------------------------------------------------------------------------
# (width, height) of rectangles whose box with the sentinel ring, (w + 2) (h + 2), sits on an area limit or just past it,
# and of squares whose largest d2, (side / 2)^2, is the last below / the first at or above a bucket limit
LIMIT_BOXES = {
    "area S": ((62, 30), (62, 31)), "area M": ((126, 30), (126, 31)), "area M2": ((126, 62), (126, 63)),
    "area L": ((382, 62), (382, 63)), "area X": ((506, 62), (506, 63)),
    "cmax 512": ((44, 44), (46, 46)), "cmax 1024": ((62, 62), (64, 64)), "cmax 2048": ((90, 90), (92, 92)),
}
# NB - 1 = 511, 1023, 2047 are no sums of two squares, so no plane has such a largest d2; 1024 = 32^2 is the 64 x 64 square's.
# 512 = 16^2 + 16^2 and 2048 = 32^2 + 32^2 are the centre's d2 in a diamond |dy| + |dx| <= r of radius 31 / 63.  The small
# one is cut to a 62 x 62 box (area 4096 = M_PX: only its d2 keeps it out of class M), the large one's 127 x 127 box is
# inside L_PX and X_PX (only its d2 sends it to class G).
DIAMONDS = {"cmax 512": (31, 62), "cmax 2048": (63, 127)}  # limit -> (radius, side of the box)
_LAYOUT = [  # (plane shape, [(box, top row, left column)]): one pixel of background around every rectangle
    ((128, 528), [((506, 62), 1, 1), ((506, 63), 64, 1)]),
    ((128, 528), [((382, 62), 1, 1), ((382, 63), 64, 1), ((126, 62), 1, 385), ((126, 63), 64, 385)]),
    ((162, 528), [((62, 62), 1, 1), ((64, 64), 1, 65), ((44, 44), 1, 131), ((46, 46), 1, 177), ((62, 30), 1, 225),
                  ((62, 31), 33, 225), ((126, 30), 1, 289), ((126, 31), 33, 289), ((90, 90), 67, 1), ((92, 92), 67, 93)]),
    ((130, 528), [((127, 127), 1, 1), ((62, 62), 1, 145)]),  # the diamonds of DIAMONDS
]


def class_limit_planes():
    """[(mask, markers)]: the rectangles of LIMIT_BOXES, two markers of different labels in each (on its long axis)."""
    out = []
    for shape, boxes in _LAYOUT:
        m, mk = np.zeros(shape, bool), np.zeros(shape, _I32)
        pts = []
        for (w, h), y0, x0 in boxes:
            assert not m[y0 - 1:y0 + h + 1, x0 - 1:x0 + w + 1].any() and y0 + h < shape[0] and x0 + w < shape[1]
            if shape == (130, 528):
                r = {side: r for r, side in DIAMONDS.values()}[w]
                cy, cx = y0 + min(r, h // 2), x0 + min(r, w // 2)
                yy, xx = _grid(*shape)
                m[y0:y0 + h, x0:x0 + w] = (abs(yy - cy) + abs(xx - cx) <= r)[y0:y0 + h, x0:x0 + w]
            else:
                m[y0:y0 + h, x0:x0 + w] = True
            pts += [(y0 + h // 2, x0 + w // 4), (y0 + h // 2, x0 + 3 * w // 4)]
        for k, (y, x) in enumerate(sorted(pts)):
            mk[y, x] = k + 1
        out.append((m, mk))
    return out


def labels16_case():
    """A small plane of two blobs with three markers each, and the three offsets that bring its largest label to
    LAB16 - 1, LAB16 and 70000."""
    H, W = 40, 56
    y, x = _grid(H, W)
    m = ((y - 12) ** 2 + (x - 12) ** 2 <= 81) | ((y - 14) ** 2 + (x - 24) ** 2 <= 64) | ((y - 28) ** 2 + (x - 42) ** 2 <= 100)
    m |= (abs(y - 30) <= 3) & (abs(x - 14) <= 10)
    mk = np.zeros((H, W), _I32)
    for k, (py, px) in enumerate([(12, 10), (14, 26), (13, 18), (28, 42), (30, 8), (30, 20), (22, 46)]):
        assert m[py, px]
        mk[py, px] = k + 1
    return m, mk


def heap_case(lattice, tie_pair):
    """(d2, markers, mask) of a (192, 192) plane whose relief -sqrt(d2) is one plateau (d2 = 1), with a bar cut out of the
    mask and markers on a lattice -- period 4, period 2 or the checkerboard -- each with its own d2 > 1 (a fixed
    permutation of 2 .. M + 1), so every (value, age) key of the flood is unique.  ``tie_pair``: plus one two-pixel mask
    component of two markers with different labels and EQUAL d2 -- a tie (it sends a connectivity-1 plane to the
    single-heap emulation) whose pop order cannot change any pixel."""
    H = W = 192
    y, x = _grid(H, W)
    mask = np.ones((H, W), bool)
    mask[61:64, 20:150] = False  # the bar
    mask[99:102, 99:103] = False  # a hole for the tied pair
    sel = {"p4": (y % 4 == 1) & (x % 4 == 1), "p2": (y % 2 == 1) & (x % 2 == 1), "checker": (y + x) % 2 == 0}[lattice] & mask
    idx = np.flatnonzero(sel.ravel())
    M = idx.size
    d2 = np.ones((H, W), _I32)
    mk = np.zeros((H, W), _I32)
    d2.ravel()[idx] = 2 + np.random.default_rng(M).permutation(M)
    mk.ravel()[idx] = np.arange(1, M + 1)
    if tie_pair:
        mask[100, 100:102] = True
        d2[100, 100:102] = M + 10
        mk[100, 100], mk[100, 101] = M + 1, M + 2
    return d2, mk, mask


HEAP_CASES = [(lat, entry, conn) for lat in ("p4", "p2", "checker") for entry in ("f64", "edt") for conn in (2, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------
def run_counts(mask):
    """(most runs in one 64 x 64 tile, most runs in one tile row): a run is cut at a tile's left edge."""
    H, W = mask.shape
    left = np.zeros_like(mask)
    left[:, 1:] = mask[:, :-1]
    left[:, 0::64] = False
    heads = mask & ~left
    Hp, Wp = -(-H // 64) * 64, -(-W // 64) * 64
    hp = np.zeros((Hp, Wp), np.int64)
    hp[:H, :W] = heads
    per_row = hp.reshape(Hp, Wp // 64, 64).sum(2)  # (row, segment)
    per_tile = per_row.reshape(Hp // 64, 64, Wp // 64).sum(1)
    return int(per_tile.max()), int(per_row.max())


def component_rows(mask, d2, markers, lim):
    """Per 4-connected component of the mask what ws_classify_kernel sees: box area with the ring, largest d2, marker
    count and label range, and the class."""
    lab, n = ndi.label(mask)
    rows = []
    if n == 0:
        return rows
    idx = np.arange(1, n + 1)
    cmax = ndi.maximum(d2, lab, idx).astype(np.int64)
    npix = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    mm = markers != 0
    mcnt = np.bincount(lab[mm], minlength=n + 1)[1:]
    big = np.iinfo(np.int64).max
    labmin = np.full(n + 1, big)
    labmax = np.zeros(n + 1, np.int64)
    np.minimum.at(labmin, lab[mm], markers[mm])
    np.maximum.at(labmax, lab[mm], markers[mm])
    for i, sl in enumerate(ndi.find_objects(lab)):
        area = (sl[1].stop - sl[1].start + 2) * (sl[0].stop - sl[0].start + 2)
        rows.append({"area": int(area), "cmax": int(cmax[i]), "mcnt": int(mcnt[i]), "labmax": int(labmax[i + 1]),
                     "npix": int(npix[i]),
                     "cls": flood_class(lim, area, int(cmax[i]), int(labmin[i + 1]), int(labmax[i + 1]), int(mcnt[i]))})
    return rows


def chain_inputs(mask):
    """The chain's host side: (edt, d2, markers, count) by the marker recipe with min_distance 1."""
    e = skops.distance_transform_edt(mask)
    mk, n = skops.peak_markers(e, mask, 1)
    return e, np.rint(e * e).astype(_I32), mk.astype(_I32), int(n)


def census(mask, markers=None, d2=None, lim=None):
    """Which side of each content switch a plane is on.  Without ``markers`` / ``d2`` those of the chain are taken (the EDT of
    the mask, its peak markers)."""
    lim = lim or limits()
    mask = np.asarray(mask, bool)
    if markers is None:
        _, d2, markers, _ = chain_inputs(mask)
    per_tile, per_row = run_counts(mask)
    rows = component_rows(mask, d2, markers, lim)
    flooded = [r for r in rows if r["cls"] not in "-U"]
    return {"runs_per_tile": per_tile, "runs_per_row": per_row,
            "components_c1": int(ndi.label(mask)[1]), "components_c2": int(ndi.label(mask, structure=np.ones((3, 3)))[1]),
            "markers": int(np.count_nonzero(markers)), "labmax": int(markers.max()) if markers.size else 0,
            "classes": {c: sum(r["cls"] == c for r in rows) for c in ("-", "U", "S", "M", "M2", "L", "X", "G")},
            "flooded_area_max": max((r["area"] for r in flooded), default=0),
            "flooded_cmax_max": max((r["cmax"] for r in flooded), default=0), "rows": rows}


def census_summary():
    """The census of every input of the run, without the per-component rows: what profiles/worstcase_content.json records."""
    lim = limits()

    def brief(c):
        return {k: v for k, v in c.items() if k != "rows"}

    out = {f"{n} {s[0]}x{s[1]}": brief(census(plane(n, s), lim=lim)) for s in SHAPES for n in PATTERNS}
    for i, (mask, mk) in enumerate(class_limit_planes()):
        c = census(mask, mk, chain_inputs(mask)[1], lim)
        out[f"class limits plane {i}"] = dict(brief(c), boxes=[[r["area"], r["cmax"], r["cls"]] for r in c["rows"]])
    mask, mk = labels16_case()
    for off in [0] + labels16_offsets(lim, mk):
        out[f"labels at 16 bits +{off}"] = brief(census(mask, np.where(mk > 0, mk + off, 0), chain_inputs(mask)[1], lim))
    for lat in ("p4", "p2", "checker"):
        for conn in (2, 1):
            d2, mk, mask = heap_case(lat, conn == 1)
            out[f"heap {lat} c{conn}"] = {"markers": int(np.count_nonzero(mk)), "heap_peak":
                                          flood_heapq(-np.sqrt(d2.astype(_F64)), mk, mask, conn)[1]}
    return out


_NB = {1: ((-1, 0), (0, -1), (0, 1), (1, 0)),
       2: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def flood_heapq(value, markers, mask, connectivity=1):
    """scikit-image's flood restated on heapq -> (labels, peak number of heap entries): pop the smallest (value, age); every
    unlabelled masked neighbour, in raster order of the offsets, takes the popped pixel's label and is queued with the
    next age.  Marker pixels enter with age 0 in raster order (equal-valued markers then pop in raster order: the one
    thing scikit-image's own heap does otherwise)."""
    H, W = value.shape
    out = np.where(mask, markers, 0).astype(_I32)
    val = value.tolist()
    msk = np.asarray(mask, bool).tolist()
    lab = out.tolist()
    heap = [(val[y][x], 0, y, x) for y, x in zip(*np.nonzero(out))]
    heapq.heapify(heap)
    age, peak = 1, len(heap)
    nb = _NB[connectivity]
    while heap:
        _, _, y, x = heapq.heappop(heap)
        l = lab[y][x]
        for dy, dx in nb:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and msk[yy][xx] and lab[yy][xx] == 0:
                lab[yy][xx] = l
                heapq.heappush(heap, (val[yy][xx], age, yy, xx))
                age += 1
        if len(heap) > peak:
            peak = len(heap)
    return np.array(lab, _I32), peak


# ---------------------------------------------------------------------------------------------------------------------
# references (computed once, shared, read-only)
# ---------------------------------------------------------------------------------------------------------------------
_REF: dict = {}


def _once(key, fn):
    if key not in _REF:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def label_ref(name, shape, conn):
    """skops.label of the bool plane (scipy.ndimage.label)."""
    return _once(("label", name, shape, conn), lambda: skops.label(plane(name, shape), conn).astype(_I32))


def label_ref_int(name, shape, conn):
    """The second, independent reference: the raster pass of oracle/clabel.c on the plane as an integer image."""
    return _once(("label int", name, shape, conn), lambda: skops.label(plane(name, shape).astype(_I32), conn).astype(_I32))


def values_ref(name, shape, conn):
    return _once(("values", name, shape, conn), lambda: skops.label(values_plane(plane(name, shape)), conn).astype(_I32))


def cbr_ref(name, shape, conn):
    return _once(("cbr", name, shape, conn), lambda: sw._cbr_ref(label_ref(name, shape, conn)))


def ws_refs(mask, markers, e):
    """(watershed of the seeded relief, clear_border + relabel_sequential of it, its count)."""
    from oracle.watershed import watershed

    ws = watershed(skops.seeded_flood_image(e, markers), markers, mask=mask) if markers.any() else np.zeros(mask.shape, _I32)
    ws = ws.astype(_I32)
    cleared, cnt = sw._cbr_ref(ws)
    return ws, cleared, cnt


def chain_ref(name, shape):
    """(d2, edt, peaks, markers, count, watershed, cleared labels, cleared count)."""
    def make():
        mask = plane(name, shape)
        e, d2, mk, n = chain_inputs(mask)
        ws, cleared, cnt = ws_refs(mask, mk, e)
        return d2, e, mk != 0, mk, np.asarray(n, _I32), ws, cleared, cnt
    return _once(("chain", name, shape), make)


def heap_ref(lattice, conn):
    from oracle.watershed import watershed

    def make():
        d2, mk, mask = heap_case(lattice, conn == 1)
        return watershed(-np.sqrt(d2.astype(_F64)), mk, mask=mask, connectivity=conn).astype(_I32)
    return _once(("heap", lattice, conn), make)


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
EXPAND_PATTERNS = ("checker0", "comb_bottom", "comb_top")
EXPAND_DISTANCES = (1, 2 ** 0.5, 4.2)
LABEL_OPS = ("label", "label_sparse", "clear_border_relabel")
WATERSHED_OPS = ("edt", "peak_markers", "watershed_edt", "watershed_edt_cleared", "watershed_edt_cleared list")
# (operator, pattern, shape) triples that do not run, each with its reason: none
EXCLUDED: dict = {}

GROUPS = [f"labels {h}x{w}" for h, w in SHAPES] + [f"chain {h}x{w}" for h, w in SHAPES] + \
         ["expand_labels", "class limits", "labels at 16 bits", "heap beyond LDS"]


def _h():
    from arcadia_microscopy_tools_amd import hipops

    return hipops


class _Log:
    def __init__(self, group, rec):
        self.group, self.rec, self.records = group, rec, []
        self.t = time.perf_counter()

    def where(self, op, case, shape, variant):
        self.rec.where = [op, case, list(shape), variant]

    def add(self, op, case, shape, variant, outs, wants):
        """One record: outs against wants (tuples of arrays), bit for bit."""
        status, index = "pass", None
        for k, (g, w) in enumerate(zip(outs, wants)):
            ok, idx = sw.exact(g, w)
            if not ok:
                status, index = "mismatch", repr((k, idx))
                break
        r = {"group": self.group, "op": op, "param": case, "shape": list(shape), "variant": variant, "status": status,
             "index": index, "sha256": sw._digest([np.asarray(o) for o in outs]),
             "ms": round((time.perf_counter() - self.t) * 1e3, 1)}  # since the previous record: call, copies and reference
        self.t = time.perf_counter()
        self.records.append(r)
        return r

    def fail(self, r, why):
        if r["status"] == "pass":
            r.update(status="mismatch", index=why)


def _label_calls(ctx, masks, values, cbr_in, conn):
    """Every label operator of one connectivity on a stack of planes -> {operator / input kind: (labels, counts)}."""
    h = _h()
    mx = max(int(cbr_in.max()), 1)
    return {
        "label mask": sw._np(*h.label(ctx.asarray(masks), connectivity=conn)),
        "label bytes": sw._np(*h.label(ctx.asarray(masks.astype(_U8) * 3), connectivity=conn)),
        "label int32": sw._np(*h.label(ctx.asarray(values), connectivity=conn)),
        "label_sparse": sw._np(*h.label_sparse(ctx.asarray(masks), connectivity=conn)),
        "clear_border_relabel": sw._np(*h.clear_border_relabel(ctx.asarray(cbr_in), mx)),
    }


def _labels_wants(name, shape, conn):
    lab = label_ref(name, shape, conn)
    cnt = np.asarray(lab.max(), _I32)
    val = values_ref(name, shape, conn)
    return {"label mask": (lab, cnt), "label bytes": (lab, cnt), "label int32": (val, np.asarray(val.max(), _I32)),
            "label_sparse": (lab, cnt), "clear_border_relabel": cbr_ref(name, shape, conn)}


def _g_labels(ctx, log, shape):
    names = list(PATTERNS)
    for conn in (1, 2):
        single = {}
        for name in names:
            m = plane(name, shape)
            log.where("labels", f"{name} c{conn}", shape, "single")
            got = _label_calls(ctx, m[None], values_plane(m)[None], label_ref(name, shape, conn)[None], conn)
            wants = _labels_wants(name, shape, conn)
            for op, (lab, cnt) in got.items():
                r = log.add(op, f"{name} c{conn}", shape, "single", (lab[0], cnt[0]), wants[op])
                if op == "label mask" and not np.array_equal(lab[0], label_ref_int(name, shape, conn)):
                    log.fail(r, "differs from the second reference")
                single[(op, name)] = sw._digest([lab[0], cnt[0]])
        # all patterns of the shape as ONE batch: every plane equal to its reference and to the single-plane result
        log.where("labels", f"all patterns c{conn}", shape, "batch")
        masks = np.stack([plane(n, shape) for n in names])
        got = _label_calls(ctx, masks, np.stack([values_plane(m) for m in masks]),
                           np.stack([label_ref(n, shape, conn) for n in names]), conn)
        for op, (lab, cnt) in got.items():
            r = log.add(op, f"all patterns c{conn}", shape, "batch", (lab, cnt),
                        tuple(np.stack([np.asarray(_labels_wants(n, shape, conn)[op][k]) for n in names]) for k in (0, 1)))
            for i, n in enumerate(names):
                if sw._digest([lab[i], cnt[i]]) != single[(op, n)]:
                    log.fail(r, f"plane {i} ({n}) of the batch differs from the single-plane result")


def _watershed_three_ways(ctx, log, case, shape, d2, mk, dm, cnt, keep, want, variant="single"):
    """watershed_edt(seeds_first), watershed_edt_cleared without and with the marker list, against (ws, cleared, count).
    Returns the three results."""
    h = _h()
    ws, cleared, ccount = want
    mx = max(int(np.max(cnt.numpy())), 1)
    log.where("watershed_edt", case, shape, variant)
    w = sw._np(h.watershed_edt(d2, mk, dm, seeds_first=True))
    log.add("watershed_edt", case, shape, variant, w, (ws,))
    log.where("watershed_edt_cleared", case, shape, variant)
    a = sw._np(*h.watershed_edt_cleared(d2, mk, dm, cnt, mx, ctx.empty(d2.shape, _I32)))
    log.add("watershed_edt_cleared", case, shape, variant, a, (cleared, ccount))
    log.where("watershed_edt_cleared list", case, shape, variant)
    b = sw._np(*h.watershed_edt_cleared(d2, mk, dm, cnt, mx, ctx.empty(d2.shape, _I32), marker_list=keep))
    r = log.add("watershed_edt_cleared list", case, shape, variant, b, (cleared, ccount))
    if sw._digest(a) != sw._digest(b):
        log.fail(r, "the marker-list route differs from the dense one")
    return w, a, b


def _host_keep(ctx, markers):
    """The marker list as label_sparse(keep=) leaves it, from host markers (n, H, W)."""
    n = markers.shape[0]
    cap = max(int(np.count_nonzero(m)) for m in markers) + 8
    klist, kcount = np.zeros((n, cap), _I32), np.zeros(n, _I32)
    for i, m in enumerate(markers):
        idx = np.flatnonzero(m)
        klist[i, :idx.size], kcount[i] = idx, idx.size
    return ctx.asarray(klist), ctx.asarray(kcount)


def _chain(ctx, log, names, shape, variant):
    """edt -> peak_markers(min_distance 1, keep=) -> the three watershed routes on the planes of `names` in one call each;
    returns the digests of every plane's results, stage by stage."""
    h = _h()
    case = names[0] if variant == "single" else "all patterns"
    n = len(names)
    d2r, er, pkr, mkr, nr, wsr, clr, ccr = (np.stack([np.asarray(chain_ref(nm, shape)[k]) for nm in names]) for k in range(8))
    dm = ctx.asarray(np.stack([plane(nm, shape) for nm in names]))
    log.where("edt", case, shape, variant)
    d2, e = h.edt(dm)
    stages = [sw._np(d2, e)]
    log.add("edt", case, shape, variant, stages[0], (d2r, er))
    log.where("peak_markers", case, shape, variant)
    keep = (ctx.empty((n, h.label_sparse_capacity(*shape)), _I32), ctx.zeros((n,), _I32))
    pk, mk, cnt = h.peak_markers(d2, dm, 1, 1, peaks=ctx.zeros(dm.shape, _U8), markers=ctx.zeros(dm.shape, _I32),
                                 count=ctx.zeros((n,), _I32), keep=keep)
    stages.append(sw._np(pk, mk, cnt))
    r = log.add("peak_markers", case, shape, variant, stages[1], (pkr, mkr, nr))
    # the lists the chain hands on: every marker pixel of a plane once, in any order
    lists, counts = keep[0].numpy(), keep[1].numpy()
    for i in range(n):
        if sorted(lists[i, :int(counts[i])].tolist()) != np.flatnonzero(mkr[i]).tolist():
            log.fail(r, f"the kept list of plane {i} is not the set of its marker pixels")
    stages += _watershed_three_ways(ctx, log, case, shape, d2, mk, dm, cnt, keep, (wsr, clr, ccr), variant)
    return [[sw._digest([o[i] for o in st]) for st in stages] for i in range(n)]


def _g_chain(ctx, log, shape):
    names = list(PATTERNS)
    single = [_chain(ctx, log, [name], shape, "single")[0] for name in names]
    # all patterns of the shape as ONE batch: every plane equal to its reference and to the single-plane result
    batch = _chain(ctx, log, names, shape, "batch")
    for i, name in enumerate(names):
        if batch[i] != single[i]:
            log.fail(log.records[-1], f"plane {i} ({name}) of the batch differs from the single-plane results "
                                      f"(stages {[k for k in range(5) if batch[i][k] != single[i][k]]})")


def _g_expand(ctx, log):
    h = _h()
    for shape in SHAPES:
        for name in EXPAND_PATTERNS:
            lab = label_ref(name, shape, 1)
            d = ctx.asarray(lab[None])
            for dist in EXPAND_DISTANCES:
                case = f"{name} d={dist:.4g}"
                log.where("expand_labels", case, shape, "single")
                want = _once(("expand", name, shape, dist), lambda: expand_ref.expand_two_pass(lab, dist))
                log.add("expand_labels", case, shape, "single", sw._np(h.expand_labels(d, dist)), (want[None],))


def _given_markers(ctx, log, case, mask, mk, want=None):
    """The three watershed routes on (mask, hand-placed markers numbered 1..k)."""
    h = _h()
    e = skops.distance_transform_edt(mask)
    want = want or _once(("given", case), lambda: ws_refs(mask, mk, e))
    dm, dmk = ctx.asarray(mask[None]), ctx.asarray(mk[None])
    d2, _ = h.edt(dm)
    cnt = ctx.asarray(np.array([mk.max()], _I32))
    _watershed_three_ways(ctx, log, case, mask.shape, d2, dmk, dm, cnt, _host_keep(ctx, mk[None]),
                          tuple(np.asarray(w)[None] for w in want))


def _g_classes(ctx, log):
    for i, (mask, mk) in enumerate(class_limit_planes()):
        _given_markers(ctx, log, f"plane {i}", mask, mk)


def labels16_offsets(lim, mk):
    return [t - int(mk.max()) for t in (lim["LAB16"] - 1, lim["LAB16"], 70000)]


def _g_labels16(ctx, log):
    from oracle.watershed import watershed

    h = _h()
    mask, mk = labels16_case()
    e = skops.distance_transform_edt(mask)
    dm = ctx.asarray(mask[None])
    d2, _ = h.edt(dm)
    base = None
    for off in [0] + labels16_offsets(limits(), mk):
        mo = np.where(mk > 0, mk + off, 0).astype(_I32)
        case = f"labmax {int(mo.max())}"
        want = _once(("labels16", off), lambda: watershed(skops.seeded_flood_image(e, mo), mo, mask=mask).astype(_I32))
        log.where("watershed_edt", case, mask.shape, "single")
        got = h.watershed_edt(d2, ctx.asarray(mo[None]), dm, seeds_first=True).numpy()
        r = log.add("watershed_edt", case, mask.shape, "single", (got,), (want[None],))
        plain = np.where(got > 0, got - off, 0)
        if base is None:
            base = plain
        elif not np.array_equal(plain, base):
            log.fail(r, "differs from the result with small labels once the offset is removed")


def _g_heap(ctx, log):
    h = _h()
    for lattice, entry, conn in HEAP_CASES:
        d2, mk, mask = heap_case(lattice, conn == 1)
        case = f"{lattice} {entry} c{conn}"
        log.where("watershed", case, mask.shape, "single")
        dm, dmk = ctx.asarray(mask[None]), ctx.asarray(mk[None])
        if entry == "f64":
            got = h.watershed(ctx.asarray(-np.sqrt(d2.astype(_F64))[None]), dmk, dm, connectivity=conn)
        else:
            got = h.watershed_edt(ctx.asarray(d2[None]), dmk, dm, seeds_first=False, connectivity=conn)
        log.add("watershed " + entry, case, mask.shape, "single", sw._np(got), (heap_ref(lattice, conn)[None],))


def _dispatch(ctx, log, group):
    kind, _, arg = group.partition(" ")
    if kind in ("labels", "chain") and "x" in arg and arg.replace("x", "").isdigit():
        shape = tuple(int(v) for v in arg.split("x"))
        return (_g_labels if kind == "labels" else _g_chain)(ctx, log, shape)
    return {"expand_labels": _g_expand, "class limits": _g_classes, "labels at 16 bits": _g_labels16,
            "heap beyond LDS": _g_heap}[group](ctx, log)


def run(ctx, groups=None, scratch_check=False):
    """The cases of the groups (default: all): {"records": [...], "dirty": [...], "seconds": s}.  A mismatch is recorded
    and the run goes on; an exception from the library ends it at once."""
    records = []
    t0 = time.perf_counter()
    with sw.Recorder(ctx, scratch_check) as rec:
        for group in (GROUPS if groups is None else groups):
            log = _Log(group, rec)
            _dispatch(ctx, log, group)
            records += log.records
    return {"records": records, "dirty": rec.dirty, "seconds": time.perf_counter() - t0}


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", required=True, help="where to write the records and the scratch findings")
    ap.add_argument("--group", action="append", help="only this group (repeatable)")
    ap.add_argument("--profile", help="also write the run's time, its case count and the census of every input here")
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison = poison_child.poisoned()
    res = run(get_context(), args.group, scratch_check=poison)
    poison_child.write(args.json, res)
    bad = [r for r in res["records"] if r["status"] != "pass"]
    if args.profile:
        with open(args.profile, "w") as f:
            json.dump({"device": get_context().device_name(), "poison": poison, "seconds": round(res["seconds"], 2),
                       "cases": len(res["records"]), "mismatches": len(bad),
                       "cases_per_group": {g: sum(r["group"] == g for r in res["records"]) for g in GROUPS},
                       "limits": limits(), "census": census_summary()}, f, indent=1)
            f.write("\n")
    for r in bad[:20]:
        print("MISMATCH", r["op"], r["param"], r["shape"], r["variant"], r["index"], flush=True)
    for d in res["dirty"][:20]:
        print("DIRTY SCRATCH", d, flush=True)
    print(f"{len(res['records'])} cases, {len(bad)} mismatches, {len(res['dirty'])} dirty scratch checks, "
          f"{res['seconds']:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
