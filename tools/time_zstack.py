"""Time the Z-stack operators (device events): ``z_project`` (max, mean), ``focus_sums``, ``focus_index`` and ``focus_stack``
at r = 4 and r = 15, and ``z_take``, on the same buffers.

    python tools/time_zstack.py [--stacks 48] [--planes 9] [--size 2048] [--json profiles/zstack.json]

``--stacks`` stacks of ``--planes`` planes of ``--size`` squared uint16: the nuclei plane of ``synth.synth_fov``, blurred
per plane by a box of side 2 |z - z0| + 1 with the focal plane z0 constant on each cell of a 4 x 4 grid of regions.  In ONE
run the operators take turns; each figure is the median of 20 rounds after a warm-up.

What the figures are set against: ``z_project("max")`` is pure streaming, so its bytes (stacks in, one plane per stack out)
over its time is compared with the 6.29 TB/s of a streaming copy on an MI355X; ``focus_stack`` / ``focus_index`` have the
same mandatory traffic, so their time over ``z_project("max")``'s stands beside the halo factor their tile implies,
(tile + 2 r + 2)^2 / tile^2.  On the host clock: ``operations.extended_depth_of_field`` of one stack (upload and download
included) against the numpy rule of tests/zstack_reference.py.  Prints one JSON object; ``--json`` also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from arcadia_microscopy_tools_amd import _hip, hipops, operations, synth  # noqa: E402
from arcadia_microscopy_tools_amd.device import get_context  # noqa: E402

ROUNDS = 20
DISTINCT = 4
COPY_TBS = 6.29  # streaming copy, MI355X


def alternate(ctx, fns):
    for fn in fns.values():
        fn()
        fn()
    ctx.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t = ctx.timer()
            t.start()
            fn()
            t.stop()
            ms[k].append(t.elapsed_ms())
    return ms


def synthetic_stack(seed, planes, size):
    """(planes, size, size) uint16 and its planted focal planes"""
    from scipy import ndimage as ndi

    sharp = synth.synth_fov(seed, size=size)[1].astype(np.float64)
    levels = [sharp] + [ndi.uniform_filter(sharp, 2 * k + 1, mode="nearest") for k in range(1, planes)]
    levels = np.stack(levels)
    rng = np.random.default_rng(seed)
    z0 = np.kron(rng.integers(0, planes, size=(4, 4)), np.ones((size // 4, size // 4), np.int64))
    z0 = np.pad(z0, ((0, size - z0.shape[0]), (0, size - z0.shape[1])), mode="edge")
    stack = np.stack([np.take_along_axis(levels, np.abs(z - z0)[None], axis=0)[0] for z in range(planes)])
    return np.clip(np.rint(stack), 0, 65535).astype(np.uint16), z0


def main():
    import zstack_reference as ref

    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, default=48)
    ap.add_argument("--planes", type=int, default=9)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = get_context()
    N, Z, S = a.stacks, a.planes, a.size
    tile = hipops.zstack_tile()
    out = {"device": ctx.device_name(), "stacks": N, "planes": Z, "size": S, "timed_rounds": ROUNDS, "tile": list(tile)}
    made = [synthetic_stack(i, Z, S) for i in range(DISTINCT)]
    batch = ctx.empty((N, Z, S, S), np.uint16)
    for i, (stack, _) in enumerate(made):
        ctx.asarray(stack, out=batch[i])
    for n in range(DISTINCT, N):
        src = batch[n % DISTINCT]
        _hip.check(ctx._lib.amt_memcpy_d2d(ctx.handle, batch[n].ptr, src.ptr, src.nbytes), "amt_memcpy_d2d")
    plane16 = ctx.empty((N, S, S), np.uint16)
    plane64 = ctx.empty((N, S, S), np.float64)
    sums = ctx.empty((N, Z, 4), np.int64)
    index = hipops.focus_index(batch, 4)
    ms = alternate(ctx, {
        "z_project_max": lambda: hipops.z_project(batch, "max", out=plane16),
        "z_project_mean": lambda: hipops.z_project(batch, "mean", out=plane64),
        "focus_sums": lambda: hipops.focus_sums(batch, out=sums),
        "focus_index_r4": lambda: hipops.focus_index(batch, 4, out=plane16),
        "focus_stack_r4": lambda: hipops.focus_stack(batch, 4, out=plane16),
        "focus_index_r15": lambda: hipops.focus_index(batch, 15, out=plane16),
        "focus_stack_r15": lambda: hipops.focus_stack(batch, 15, out=plane16),
        "z_take": lambda: hipops.z_take(batch, index, out=plane16),
    })
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out["ms"] = {k: round(v, 3) for k, v in med.items()}
    out["ms_min_max"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}
    moved = batch.nbytes + plane16.nbytes
    tbs = moved / (med["z_project_max"] * 1e-3) / 1e12
    out["z_project_max"] = {"bytes_moved": moved, "tb_per_s": round(tbs, 3), "share_of_streaming_copy": round(tbs / COPY_TBS, 3)}
    for r in (4, 15):
        halo = (tile[0] + 2 * r + 2) * (tile[1] + 2 * r + 2) / (tile[0] * tile[1])
        out[f"r{r}"] = {"halo_factor": round(halo, 3),
                        "focus_stack_over_z_project_max": round(med[f"focus_stack_r{r}"] / med["z_project_max"], 2),
                        "focus_index_over_z_project_max": round(med[f"focus_index_r{r}"] / med["z_project_max"], 2)}
    # one stack through the reference-level call, against the numpy rule, on the host clock
    stack, z0 = made[0]
    operations.extended_depth_of_field(stack)
    t0 = time.perf_counter()
    got = operations.extended_depth_of_field(stack)
    device_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want, windex = ref.extended_depth_of_field(stack, 4, 0)
    host_ms = (time.perf_counter() - t0) * 1e3
    out["extended_depth_of_field_one_stack"] = {
        "device_call_host_clock_ms": round(device_ms, 1), "numpy_rule_host_ms": round(host_ms, 1),
        "equal": bool(np.array_equal(got, want)), "planted_focal_plane_recovered": round(float((windex == z0).mean()), 4)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
