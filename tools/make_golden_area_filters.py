"""Writes tests/golden/area_filters.npz: scikit-image's own ``remove_small_objects`` / ``remove_small_holes`` on the planes
of ``tests/area_filters_reference.golden_planes()``, both connectivities, sizes 2 / 5 / 17 / 64.

Run with an interpreter that has scikit-image 0.18.3 (the pinned reference version), numpy and scipy:

    python3.9 tools/make_golden_area_filters.py

Keys: ``in/<plane>`` (uint8 0 / 1), ``<objects|holes>/<plane>/c<connectivity>/s<size>`` (bit-packed rows of the bool
result, ``np.packbits(out, axis=1)``), ``skimage_version``.
"""
import os
import sys

import numpy as np
import skimage
from skimage import morphology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import area_filters_reference as ref  # noqa: E402


def main():
    out = {"skimage_version": np.array(skimage.__version__)}
    for name, plane in ref.golden_planes().items():
        out[f"in/{name}"] = plane
        m = plane.astype(bool)
        for conn in (1, 2):
            for size in ref.GOLDEN_SIZES:
                out[f"objects/{name}/c{conn}/s{size}"] = np.packbits(
                    morphology.remove_small_objects(m, min_size=size, connectivity=conn), axis=1)
                out[f"holes/{name}/c{conn}/s{size}"] = np.packbits(
                    morphology.remove_small_holes(m, area_threshold=size, connectivity=conn), axis=1)
    path = os.path.join(ROOT, "tests", "golden", "area_filters.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes, scikit-image {skimage.__version__}")


if __name__ == "__main__":
    main()
