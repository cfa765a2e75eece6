"""Generate tests/golden/props_ext.npz: the extended regionprops columns of ``SegmentationMask.cell_properties``.

Run with the conda interpreter that has scikit-image 0.18.3:

    /opt/conda/bin/python3.9 tools/make_golden_props.py

The reference (R/masks.py:247-328) hands ``property_names`` and ``intensity_property_names`` to
``regionprops_table`` unchanged; this tool restates that function with the 0.18.3 property names and renames the
columns to the 0.25.2 names the reference pins (``OLD``).  Two cases, inputs stored next to the expected columns:

  nuc  the 22-nucleus label plane of c2c3_256.npz with its 4 uint16 channels (exact integer path)
  syn  a synthetic plane of topological corner cases with one uint16 and one float64 channel (float64 path)

For every case ``<case>__keys`` is the key order of the table and ``<case>__<key>`` a column; ``euler_number`` is
int64 (0.25.2's COL_DTYPES), ``label`` / ``bbox-*`` int64, every other column float64.
"""
import os
import warnings

import numpy as np

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


def main():
    c2c3 = np.load(os.path.join(OUT, "c2c3_256.npz"))
    nuc_lab = c2c3["labels"].astype(np.int64)
    fov = c2c3["fov"]
    nuc_ch = {n: fov[i] for i, n in enumerate(("BRIGHTFIELD", "DAPI", "FITC", "TRITC"))}
    syn_lab, syn_ch = synthetic()
    out = {"versions": VERSIONS, "props": np.array(PROPS), "iprops": np.array(IPROPS),
           "nuc__labels": nuc_lab, "nuc__fov": fov, "syn__labels": syn_lab, "syn__dapi": syn_ch["DAPI"],
           "syn__fitc": syn_ch["FITC"]}
    for case, lab, ch in (("nuc", nuc_lab, nuc_ch), ("syn", syn_lab, syn_ch)):
        assert lab.max() == len(np.unique(lab)) - 1, "labels must be sequential"
        t = cell_properties(lab, ch, list(PROPS), list(IPROPS))
        out[f"{case}__keys"] = np.array(list(t))
        for k, v in t.items():
            out[f"{case}__{k}"] = v
    path = os.path.join(OUT, "props_ext.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
