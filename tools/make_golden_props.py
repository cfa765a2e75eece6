"""Generate tests/golden/props_ext.npz and props_frag.npz: the extended regionprops columns of
``SegmentationMask.cell_properties``.

Run with the conda interpreter that has scikit-image 0.18.3:

    /opt/conda/bin/python3.9 tools/make_golden_props.py

The reference (R/masks.py:247-328) hands ``property_names`` and ``intensity_property_names`` to
``regionprops_table`` unchanged; this tool restates that function with the 0.18.3 property names and renames the
columns to the 0.25.2 names the reference pins (``OLD``).  Three cases, inputs stored next to the expected columns:

  nuc   the 22-nucleus label plane of c2c3_256.npz with its 4 uint16 channels (exact integer path)
  syn   a synthetic plane of topological corner cases with one uint16 and one float64 channel (float64 path)
  frag  (props_frag.npz) the kernels' boundary cases: 444 labels of two single pixels each, whose bounding-box
        heights add up to more than H * W; boxes of 63 / 64 / 65 / 128 / 129 rows or columns with holes on both
        sides of the 64-bit word seams; background that reaches the box frame only through a diagonal step across
        a seam; spiral corridors in 81 x 81 boxes, open and closed; the hull classes' 48 / 49 rows and 250 / 251
        columns; labels on the right and bottom frame; one uint16 channel near 65535 and one float64 channel with
        negative values

A file whose arrays are already what this tool computes is left as it is (the zip entries carry a time stamp).

For every case ``<case>__keys`` is the key order of the table and ``<case>__<key>`` a column; ``euler_number`` is
int64 (0.25.2's COL_DTYPES), ``label`` / ``bbox-*`` int64, every other column float64.

numpy 1.26's AVX-512 ``power`` loop is not correctly rounded (``102.0 ** 1`` gives 101.99999999999999), and
scikit-image's raw moments take ``delta ** arange(order + 1)``; the tool turns that loop off before numpy loads, so
the moments of a box are exact integers on every machine.
"""
import os
import warnings

os.environ.setdefault("NPY_DISABLE_CPU_FEATURES", "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL "
                                                  "AVX512_SPR")
import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")
import scipy  # noqa: E402
import skimage  # noqa: E402
from skimage import measure  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
VERSIONS = np.array([skimage.__version__, scipy.__version__, np.__version__])

# 0.25.2 name -> 0.18.3 name
OLD = {
    "area_convex": "convex_area",
    "axis_major_length": "major_axis_length",
    "axis_minor_length": "minor_axis_length",
    "intensity_mean": "mean_intensity",
    "intensity_max": "max_intensity",
    "intensity_min": "min_intensity",
    "area_filled": "filled_area",
    "area_bbox": "bbox_area",
    "equivalent_diameter_area": "equivalent_diameter",
    "centroid_local": "local_centroid",
    "centroid_weighted": "weighted_centroid",
    "centroid_weighted_local": "weighted_local_centroid",
}

DEFAULT = ("label centroid volume area area_convex perimeter eccentricity circularity solidity "
           "axis_major_length axis_minor_length orientation").split()
EXTENDED = ("euler_number perimeter_crofton area_filled feret_diameter_max area_bbox extent equivalent_diameter_area "
            "centroid_local inertia_tensor inertia_tensor_eigvals").split()
PROPS = DEFAULT + EXTENDED
IPROPS = ["intensity_mean", "intensity_max", "intensity_min", "intensity_std", "centroid_weighted",
          "centroid_weighted_local"]


# computed here with numpy: intensity_std does not exist in 0.18.3, and its regionprops_table casts max / min to int
# (its COL_DTYPES), which truncates float images; 0.25.2 keeps the image's values
BY_HAND = {"intensity_std": np.std, "intensity_max": np.max, "intensity_min": np.min}


def table(labels, names, intensity=None):
    """regionprops_table with 0.25.2 names in and out."""
    sk = [OLD.get(p, p) for p in names if p not in BY_HAND]
    t = measure.regionprops_table(labels, intensity_image=intensity, properties=sk)
    out = {}
    for p in names:
        if p in BY_HAND:
            out[p] = np.asarray([BY_HAND[p](intensity[labels == lab]) for lab in range(1, labels.max() + 1)])
            continue
        old = OLD.get(p, p)
        for k, v in t.items():
            if k == old or k.startswith(old + "-"):
                out[p + k[len(old):]] = np.asarray(v)
    return out


def cell_properties(labels, channels, property_names, intensity_property_names):
    """R/masks.py:247-328 restated."""
    needs_circ = "circularity" in property_names
    needs_vol = "volume" in property_names
    sk = [p for p in property_names if p not in ("circularity", "volume")]
    added = set()
    for dep in ["area", "perimeter"] if needs_circ else []:
        if dep not in sk:
            sk.append(dep)
            added.add(dep)
    for dep in ["axis_major_length", "axis_minor_length"] if needs_vol else []:
        if dep not in sk:
            sk.append(dep)
            added.add(dep)
    props = table(labels, sk)
    if needs_circ:
        area, per = props["area"], props["perimeter"]
        with np.errstate(divide="ignore", invalid="ignore"):
            props["circularity"] = np.where(per > 0, (4.0 * np.pi * area) / (per**2), 0.0)
    if needs_vol:
        a = props["axis_major_length"] / 2.0
        b = props["axis_minor_length"] / 2.0
        props["volume"] = np.where((a > 0) & (b > 0), (4.0 / 3.0) * np.pi * a * b * b, 0.0)
    for p in added:
        props.pop(p, None)
    if "centroid-0" in props:
        props["centroid_y"] = props.pop("centroid-0")
    if "centroid-1" in props:
        props["centroid_x"] = props.pop("centroid-1")
    for name, img in channels.items():
        for k, v in table(labels, intensity_property_names, img).items():
            props[f"{k}_{name.lower()}"] = v
    for k, v in props.items():
        if k == "label" or k.startswith("bbox-") or k == "euler_number":
            props[k] = np.asarray(v, dtype=np.int64)
        else:
            props[k] = np.asarray(v, dtype=np.float64)
    return props


def disk(shape, cy, cx, r):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def synthetic():
    shape = (110, 300)
    lab = np.zeros(shape, np.int64)
    lab[disk(shape, 12, 14, 8) & ~disk(shape, 12, 14, 4)] = 1  # ring
    lab[disk(shape, 14, 40, 9) & ~disk(shape, 14, 40, 5)] = 2  # ring with label 3 inside its hole
    lab[disk(shape, 14, 40, 2)] = 3
    lab[2:11, 60:65] = 4  # figure-8: two holes, Euler -1
    lab[4:6, 62] = 0
    lab[7:9, 62] = 0
    lab[2:5, 75:78] = 5  # two blobs touching at one corner
    lab[5:8, 78:81] = 5
    lab[2:5, 90:94] = 6  # one label, two disjoint pieces
    lab[8:11, 96:100] = 6
    lab[3, 110] = 7  # one pixel
    lab[8, 106:119] = 8  # one row
    lab[2:15, 124] = 9  # one column
    lab[0:5, 132:141] = 10  # touches the frame
    lab[4:9, 141:146] = 10
    # larger than the hull kernels' LDS class (48 x 250): an ellipse with a hole that holds label 12, and an empty hole
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    big = ((yy - 62) / 31.0) ** 2 + ((xx - 150) / 136.0) ** 2 <= 1.0
    lab[big] = 11
    lab[disk(shape, 62, 100, 6)] = 0
    lab[disk(shape, 62, 200, 7)] = 0
    lab[disk(shape, 62, 200, 3)] = 12
    lab[100:104, 20:26] = 13  # zero total intensity
    lab[96:108, 280:300] = 14  # touches the right frame, with a notch
    lab[100:104, 290:300] = 0
    lab[99:106, 50:57] = 15  # a square ring whose hole is one pixel wide on a diagonal
    lab[101:104, 52:55] = 0
    lab[102, 53] = 15

    rng = np.random.default_rng(7)
    dapi = rng.integers(0, 65536, shape, dtype=np.uint16)
    fitc = rng.random(shape) * 1000.0
    dapi[lab == 13] = 0
    fitc[lab == 13] = 0.0
    return lab, {"DAPI": dapi, "FITC": fitc}


def fragmented():
    """The frag case (see the module docstring) -> (labels, channels)."""
    H, W = 300, 320
    lab = np.zeros((H, W), np.int64)
    nxt = [1]

    def new():
        v = nxt[0]
        nxt[0] += 1
        return v

    def rect(y0, x0, h, w):
        v = new()
        lab[y0:y0 + h, x0:x0 + w] = v
        return v

    # hull classes: 48 x 250 (LDS kernel), 49 rows and 251 columns (global-memory kernel); slanted so the hull matters
    for (y0, x0, h, w) in ((8, 2, 48, 250), (8, 258, 49, 56), (60, 2, 30, 251)):
        v = new()
        for k in range(h):
            s = (k * (w // 3)) // h
            lab[y0 + k, x0 + s:x0 + s + w - w // 3] = v
        lab[y0, x0 + w - 1] = v  # the far corners fix the box
        lab[y0 + h - 1, x0] = v
        lab[y0 + h // 2, x0 + w // 3: x0 + w // 3 + 3] = 0  # a hole
    # frames of 63 / 64 / 65 columns with holes on both sides of box column 63 | 64
    for (y0, x0, h, w) in ((94, 2, 63, 63), (94, 68, 64, 64), (94, 135, 65, 65)):
        v = rect(y0, x0, h, w)
        for c in (61, 62, 63, 64):
            if c < w - 1:
                lab[y0 + 5 + 6 * (c - 61), x0 + c] = 0  # one-pixel holes at box columns 62, 63, 64
        if w > 64:
            lab[y0 + 30:y0 + 33, x0 + 63:x0 + 65] = 0  # a hole across the seam
            lab[y0 + 40, x0 + 63] = 0  # reaches the label's outside only through a diagonal step across the seam:
            lab[y0 + 41, x0 + 64:x0 + w] = 0  # (40, 63) - (41, 64) - the corridor to the right frame of the box
            lab[y0 + 50, x0 + 64] = 0  # and the mirror image: (50, 64) - (51, 63) - the corridor to the left frame
            lab[y0 + 51, x0:x0 + 64] = 0
    # 128 and 129 rows, 128 and 129 columns: holes next to box rows / columns 63 | 64 and 127 | 128
    for (y0, x0, h, w) in ((94, 203, 128, 12), (94, 218, 129, 13), (245, 2, 23, 128), (270, 2, 23, 129)):
        v = rect(y0, x0, h, w)
        for k in (62, 63, 64, 126, 127):
            if h > 64 and k < h - 1:
                lab[y0 + k, x0 + 3 + (k % 3) * 2] = 0
            if w > 64 and k < w - 1:
                lab[y0 + 2 + (k % 4) * 2, x0 + k] = 0
        if w > 64:
            lab[y0 + 11:y0 + 13, x0 + 63:x0 + 65] = 0  # a hole across the word seam
            lab[y0 + 15, x0 + 63] = 0  # reaches the outside only through (15, 63) - (16, 64), across the seam
            lab[y0 + 16, x0 + 64:x0 + w] = 0
            lab[y0 + 19, x0 + 64] = 0  # and the mirror image: (19, 64) - (20, 63) - the left frame of the box
            lab[y0 + 20, x0:x0 + 64] = 0
    # spiral corridors in 81 x 81 boxes: one open to the box frame, one closed
    for (y0, x0, closed) in ((94, 236, False), (162, 120, True)):
        v = new()
        n = 81
        box = np.ones((n, n), bool)
        # walls every other ring: the corridor between them winds inwards
        lo, hi, d = 1, n - 2, 0
        y, x = 1, 1
        path = []
        while lo <= hi:
            for xx in range(lo, hi + 1):
                path.append((lo, xx))
            for yy in range(lo + 1, hi + 1):
                path.append((yy, hi))
            for xx in range(hi - 1, lo - 1, -1):
                path.append((hi, xx))
            for yy in range(hi - 1, lo + 1, -1):
                path.append((yy, lo + 0))
            path.append((lo + 2, lo + 1))
            lo, hi = lo + 2, hi - 2
        for (py, px) in path:
            if 0 <= py < n and 0 <= px < n:
                box[py, px] = False
        if not closed:
            box[1, 0] = False  # the corridor starts at the box frame
        sub = lab[y0:y0 + n, x0:x0 + n]
        sub[box] = v
        sub[~box] = 0
    # frame contact: right and bottom frame, and the corner
    v = rect(H - 12, W - 20, 12, 20)
    lab[H - 6:H - 3, W - 20:W - 10] = 0
    v = rect(180, W - 4, 30, 4)
    # single pixels: every label below has one pixel in a band under the top frame and one above the bottom frame,
    # so the bounding-box heights add up to more than H * W
    rng = np.random.default_rng(11)
    top = [(y, x) for y in (1, 3, 5) for x in range(1, W - 24, 2) if lab[y, x] == 0]
    bot = [(y, x) for y in (H - 2, H - 4, H - 6) for x in range(1, W - 24, 2) if lab[y, x] == 0]
    nfrag = min(len(top), len(bot))
    ti, bi = rng.permutation(len(top))[:nfrag], rng.permutation(len(bot))[:nfrag]
    for a, b in zip(ti, bi):
        v = new()
        lab[top[a]] = v
        lab[bot[b]] = v
    rng = np.random.default_rng(5)
    # 2 x 2 blocks keep the file small
    dapi = np.kron(65535 - rng.integers(0, 4096, (H // 2, W // 2)), np.ones((2, 2), np.int64)).astype(np.uint16)
    fitc = np.kron(rng.integers(-512, 512, (H // 2, W // 2)), np.ones((2, 2))) / 8.0
    dapi[lab == 13] = 0
    fitc[lab == 14] = 0.0
    return lab, {"DAPI": dapi, "FITC": fitc}


def save(path, out):
    if os.path.exists(path):
        with np.load(path, allow_pickle=False) as old:
            if set(old.files) == set(out) and all(
                    old[k].dtype == np.asarray(out[k]).dtype and np.array_equal(old[k], out[k],
                                                                     equal_nan=old[k].dtype.kind == "f")
                    for k in out):
                print(path, "unchanged")
                return
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def main():
    c2c3 = np.load(os.path.join(OUT, "c2c3_256.npz"))
    nuc_lab = c2c3["labels"].astype(np.int64)
    fov = c2c3["fov"]
    nuc_ch = {n: fov[i] for i, n in enumerate(("BRIGHTFIELD", "DAPI", "FITC", "TRITC"))}
    syn_lab, syn_ch = synthetic()
    frag_lab, frag_ch = fragmented()
    out = {"versions": VERSIONS, "props": np.array(PROPS), "iprops": np.array(IPROPS),
           "nuc__labels": nuc_lab, "nuc__fov": fov, "syn__labels": syn_lab, "syn__dapi": syn_ch["DAPI"],
           "syn__fitc": syn_ch["FITC"]}
    frag = {"versions": VERSIONS, "props": np.array(PROPS), "iprops": np.array(IPROPS), "frag__labels": frag_lab,
            "frag__dapi": frag_ch["DAPI"], "frag__fitc": frag_ch["FITC"]}
    for case, lab, ch, dst in (("nuc", nuc_lab, nuc_ch, out), ("syn", syn_lab, syn_ch, out),
                               ("frag", frag_lab, frag_ch, frag)):
        assert lab.max() == len(np.unique(lab)) - 1, "labels must be sequential"
        t = cell_properties(lab, ch, list(PROPS), list(IPROPS))
        dst[f"{case}__keys"] = np.array(list(t))
        for k, v in t.items():
            dst[f"{case}__{k}"] = v
    save(os.path.join(OUT, "props_ext.npz"), out)
    save(os.path.join(OUT, "props_frag.npz"), frag)


if __name__ == "__main__":
    main()
