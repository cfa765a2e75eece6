"""Writes tests/golden/relate.npz: ``skimage.metrics.contingency_table`` of a handful of (label plane, companion plane)
pairs from tests/relate_cases.py, as dense int64 tables (row = label value, column = companion value).

Run with an interpreter that has scikit-image 0.18.3 (the pinned reference version), numpy and scipy:

    python3.9 tools/make_golden_relate.py

Keys: ``labels/<case>`` and ``companion/<case>`` (int16 planes), ``table/<case>``, ``max_label/<case>``,
``skimage_version`` / ``numpy_version`` / ``scipy_version``.  ``<case>`` is ``<H>x<W>_<name>``.
"""
import os
import sys

import numpy as np
import scipy
import skimage
from skimage.metrics import contingency_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import relate_cases as rc  # noqa: E402


def main():
    out = {"skimage_version": np.array(skimage.__version__), "numpy_version": np.array(np.__version__),
           "scipy_version": np.array(scipy.__version__)}
    for shape, name in rc.GOLDEN:
        a, b, k = rc.cases(shape)[name]
        assert 0 <= a.min() and a.max() < 2**15 and 0 <= b.min() and b.max() < 2**15
        case = f"{shape[0]}x{shape[1]}_{name}"
        table = np.asarray(contingency_table(a, b).todense()).astype(np.int64)
        assert table.shape == (a.max() + 1, b.max() + 1) and table.sum() == a.size
        out[f"labels/{case}"] = a.astype(np.int16)
        out[f"companion/{case}"] = b.astype(np.int16)
        out[f"table/{case}"] = table
        out[f"max_label/{case}"] = np.array(k, np.int64)
    path = os.path.join(ROOT, "tests", "golden", "relate.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes, scikit-image {skimage.__version__}")


if __name__ == "__main__":
    main()
