"""Time FovSegmenter.mask_chain on 48 resident copies of one 2048 x 2048 field of view, default path and low_traffic:
a synthetic field and the degenerate `1000 + {0,1}` plane (range of one grey level: a third of its samples are left
undecided by the prefix plane, so every plane is redone by the exact second Gaussian pass).

    python tools/mask_chain_batch_probe.py OUT.json

Host clock around mask_chain + a device synchronise, 5 warm-up and 10 timed repetitions; the masks of the two paths are
compared.  The figures `mask_chain_48_planes_*` of profiles/prefix_bench.json come from this script, run in the parent
commit's tree and in this one during the same visit."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arcadia_microscopy_tools_amd import synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402
from arcadia_microscopy_tools_amd.segment import FovSegmenter  # noqa: E402


def main():
    ctx = get_context()
    B, S = 48, 2048
    rng = np.random.default_rng(5)
    grey = np.zeros((4, S, S), np.uint16)
    grey[1] = (1000 + rng.integers(0, 2, (S, S))).astype(np.uint16)
    out = {}
    for label, src in (("degenerate", grey), ("synthetic", synth.synth_fov(0))):
        d = ctx.asarray(np.broadcast_to(src, (B,) + src.shape).copy())
        masks = {}
        for name, kw in (("default", {}), ("low_traffic", {"low_traffic": True})):
            seg = FovSegmenter(B, 4, S, S, ctx=ctx, props=False, **kw)
            dd = seg._check_fovs(d)
            for _ in range(5):
                seg.mask_chain(dd)
            ctx.synchronize()
            ts = []
            for _ in range(10):
                t0 = time.perf_counter()
                seg.mask_chain(dd)
                ctx.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            masks[name] = seg.mask_a.numpy()[:2].copy()
            out[f"{label}_{name}_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
                                         "max": round(max(ts), 3)}
            del seg
        out[f"{label}_masks_equal"] = bool(np.array_equal(masks["default"], masks["low_traffic"]))
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
