"""Inputs and helpers of tests/test_gpu_label_box_handoff.py: the fused watershed tail (``watershed_edt_cleared`` with a
marker list) leaves the boxes of its final labels with the context, and the per-label call that directly follows takes
them instead of reading the label planes.

``python -m tests.label_box_handoff_cases --json FILE`` runs the chain comparison in a process of its own: the test
starts it with AMT_DEBUG_POISON=1, in which mode the library runs the plane pass beside every hand-off and fails the
call when the two box tables differ.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import poison_child  # noqa: E402

EMPTY = (0x7FFFFFFF, 0x7FFFFFFF, -1, -1)


def numpy_boxes(labels: np.ndarray, max_label: int) -> np.ndarray:
    """(n, max_label, 4) int32 {ymin, xmin, ymax, xmax}, inclusive; EMPTY for a label that does not occur."""
    from scipy import ndimage as ndi

    out = np.empty((labels.shape[0], max_label, 4), np.int32)
    out[:] = EMPTY
    for b, plane in enumerate(labels):
        for l, sl in enumerate(ndi.find_objects(plane, max_label)):
            if sl is not None:
                out[b, l] = (sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1)
    return out


def blob_planes() -> np.ndarray:
    """The two 640 x 1200 planes of test_watershed_every_flood_class: components of every LDS flood class and of the
    HBM queue path, each with several markers."""
    H, W = 640, 1200
    yy, xx = np.mgrid[0:H, 0:W]

    def blobs(seed):
        rng = np.random.default_rng(seed)
        m = np.zeros((H, W), bool)
        for cy, cx, hy, hx in ((40, 40, 16, 22), (40, 140, 25, 33), (60, 300, 35, 48), (150, 120, 65, 75),
                               (150, 420, 80, 92), (330, 150, 100, 110), (420, 600, 140, 160)):
            for _ in range(6):
                oy, ox = rng.integers(-hy // 2, hy // 2 + 1), rng.integers(-hx // 2, hx // 2 + 1)
                ry, rx = rng.integers(hy // 3, hy // 2 + 1), rng.integers(hx // 3, hx // 2 + 1)
                m |= ((yy - cy - oy) / ry) ** 2 + ((xx - cx - ox) / rx) ** 2 <= 1.0
        m[200:330, 700:880] = True
        for cy, cx in ((50, 960), (50, 990 + seed)):
            m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= 30 ** 2
        for cy in (250, 330):
            for cx in (980, 1060):
                m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= 44 ** 2
        m[0] = m[-1] = False
        m[:, 0] = m[:, -1] = False
        return m

    return np.stack([blobs(5), blobs(6)])


def peak_markers_of(masks: np.ndarray) -> np.ndarray:
    from oracle import skops

    return np.stack([skops.peak_markers(skops.distance_transform_edt(m), m, 5)[0].astype(np.int32) for m in masks])


def fused_watershed(ctx, masks: np.ndarray, markers: np.ndarray, max_label: int):
    """``watershed_edt_cleared`` with the marker list on (n, H, W) masks and int32 markers.  Everything the call needs is
    on the device before it starts, so that it is the context's last image operation when it returns.  Returns the
    device labels."""
    from arcadia_microscopy_tools_amd import hipops

    n = masks.shape[0]
    cap = int(max(np.count_nonzero(m) for m in markers)) + 8
    klist, kcount = np.zeros((n, cap), np.int32), np.zeros(n, np.int32)
    for b in range(n):
        idx = np.flatnonzero(markers[b])
        klist[b, :idx.size], kcount[b] = idx, idx.size
    dm, dmk = ctx.asarray(masks), ctx.asarray(markers.astype(np.int32))
    d2, _ = hipops.edt(dm)
    nl = ctx.asarray(np.array([m.max() for m in markers], np.int32))
    dlist, dcount = ctx.asarray(klist), ctx.asarray(kcount)
    scratch, out, cnt = ctx.empty(masks.shape, np.int32), ctx.empty(masks.shape, np.int32), ctx.empty((n,), np.int32)
    lab, _ = hipops.watershed_edt_cleared(d2, dmk, dm, nl, max_label, scratch, out=out, count=cnt,
                                          marker_list=(dlist, dcount))
    return lab


def framed_windows(h: int, w: int, n: int = 3) -> np.ndarray:
    """(n, 4, h, w) uint16 windows cut out of larger synthetic fields of view, so that nuclei touch the frame; the last
    one with a constant DAPI plane: no mask, no markers, no cells."""
    from arcadia_microscopy_tools_amd import synth

    size = max(h, w) + 60
    big = np.stack([synth.synth_fov(40 + i, size=size) for i in range(n)])
    fovs = np.ascontiguousarray(big[:, :, 25:25 + h, 31:31 + w])
    fovs[n - 1, 1] = 300
    return fovs


def chain_tables(ctx, fovs: np.ndarray, fused: bool, profile: bool) -> dict:
    from arcadia_microscopy_tools_amd.segment import FovSegmenter

    seg = FovSegmenter(fovs.shape[0], 4, fovs.shape[2], fovs.shape[3], ctx=ctx, max_cells=256, fused=fused, profile=profile)
    seg.run_c3(ctx.asarray(fovs))
    return {"labels": seg.labels.numpy(), "ncells": seg.ncells.numpy(), "table": seg.table.numpy(),
            "itable": seg.itable.numpy()}


def chain_windows():
    """Two 4 x 208 x 208 windows with frame-touching nuclei (a width the run-table path takes)."""
    return framed_windows(208, 208, n=3)[:2]


def chain_digests(ctx) -> dict:
    res = {}
    fovs = chain_windows()
    for fused in (True, False):
        for profile in (False, True):
            for k, v in chain_tables(ctx, fovs, fused, profile).items():
                res[f"fused={fused} profile={profile} {k}"] = poison_child.digest(v)
    return res


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--json", required=True)
    a = ap.parse_args()
    from arcadia_microscopy_tools_amd.device import get_context

    poison_child.write(a.json, {"digests": chain_digests(get_context())})
