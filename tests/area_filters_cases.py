"""Every sweep case of tests/test_gpu_area_filters.py as a function, and as a program:
``python -m tests.area_filters_cases --json OUT`` runs them in a process of its own (under ``AMT_DEBUG_POISON=1`` with a
scratch check after every call) and writes the digests of all outputs.

A case = (shape, generator, structure, operator, size), run three ways: the plane alone, as plane 1 of a two-plane stack
(an address that is no multiple of 16 for shapes such as (70, 131) and (15, 24)), and inside a batch of three different
planes in one call.  Every output is compared with the reference (scipy.ndimage.label + np.bincount), byte for byte, and
with scikit-image's own answer where tests/golden/area_filters.npz has the case.  Each plane is uploaded once and its
component areas are computed once; the sizes only change a comparison.
"""
from __future__ import annotations

import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import area_filters_reference as ref  # noqa: E402
import poison_child  # noqa: E402


def _sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def golden_cases():
    """{(plane bytes digest, op, connectivity, size): unpacked uint8 result} of the golden file."""
    out = {}
    with np.load(ref.GOLDEN) as z:
        for key in z.files:
            if not key.startswith(("objects/", "holes/")):
                continue
            op, name, conn, size = key.split("/")
            plane = z[f"in/{name}"]
            bits = np.unpackbits(z[key], axis=1)[:, :plane.shape[1]]
            out[(_sha(plane), op, int(conn[1:]), int(size[1:]))] = bits.astype(np.uint8)
    return out


def device_fn(op):
    from arcadia_microscopy_tools_amd import hipops

    return hipops.remove_small_objects if op == "objects" else hipops.remove_small_holes


def run_shape(ctx, shape, scratch_check=False, golden=None):
    """-> {"digests": {key: sha256}, "mismatches": [key], "dirty": [(key, finding)], "calls": n, "golden": n} for one
    shape."""
    digests, bad, dirty = {}, [], []
    calls = hits = 0
    golden = golden_cases() if golden is None else golden

    def call(op, d, size, conn, key):
        nonlocal calls
        out = device_fn(op)(d, size, conn)
        calls += 1
        if scratch_check:
            found = ctx.scratch_check()
            if found is not None:
                dirty.append((key, list(found)))
        return out.numpy(dtype=np.uint8)

    shape = tuple(shape)
    named = [(n, ref.Plane(p)) for n, p in ref.planes(shape)]
    sizes = ref.sweep_sizes(shape)
    singles = {n: ctx.asarray(P.plane) for n, P in named}
    stacks = {n: ctx.asarray(np.stack([1 - P.plane, P.plane])) for n, P in named}
    trios = []
    for i in range(0, len(named), 3):  # batches of three different planes in one call (the last batch wraps round)
        trio = [named[(i + j) % len(named)] for j in range(3)]
        trios.append((i // 3, trio, ctx.asarray(np.stack([P.plane for _, P in trio]))))
    for sname, _ in ref.STRUCTURES:
        conn = ref.CONNECTIVITY[sname]
        for op in ref.OPERATORS:
            for size in sizes:
                tag = f"{sname}/{op}/s{size}"
                for n, P in named:
                    key = f"{shape[0]}x{shape[1]}/{n}/{tag}"
                    want = P.want(op, sname, size)
                    g = golden.get((_sha(P.plane), op, conn, size))
                    hits += g is not None
                    for how, d in (("single", singles[n]), ("plane1", stacks[n][1])):
                        got = call(op, d, size, conn, f"{key}/{how}")
                        digests[f"{key}/{how}"] = _sha(got)
                        if not np.array_equal(got, want):
                            bad.append(f"{key}/{how}")
                        if g is not None and not np.array_equal(got, g):
                            bad.append(f"{key}/{how}/golden")
                for b, trio, d3 in trios:
                    key = f"{shape[0]}x{shape[1]}/batch{b}/{tag}"
                    got3 = call(op, d3, size, conn, key)
                    digests[key] = _sha(got3)
                    for j, (n, P) in enumerate(trio):
                        if not np.array_equal(got3[j], P.want(op, sname, size)):
                            bad.append(f"{key}/{n}")
    return {"digests": digests, "mismatches": bad, "dirty": dirty, "calls": calls, "golden": hits}


def run(ctx, scratch_check=False, shapes=None):
    t0 = time.perf_counter()
    res = {"digests": {}, "mismatches": [], "dirty": [], "calls": 0, "golden": 0}
    golden = golden_cases()
    for shape in shapes or ref.SHAPES:
        r = run_shape(ctx, shape, scratch_check, golden)
        res["digests"].update(r["digests"])
        res["mismatches"] += r["mismatches"]
        res["dirty"] += r["dirty"]
        res["calls"] += r["calls"]
        res["golden"] += r["golden"]
    res["seconds"] = time.perf_counter() - t0
    return res


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", required=True, help="where to write the digests, the mismatches and the scratch findings")
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    res = run(get_context(), scratch_check=poison_child.poisoned())
    poison_child.write(args.json, res)
    for k in res["mismatches"][:20]:
        print("MISMATCH", k, flush=True)
    for d in res["dirty"][:20]:
        print("DIRTY SCRATCH", d, flush=True)
    print(f"{res['calls']} calls, {len(res['mismatches'])} mismatches, {len(res['dirty'])} dirty scratch checks, "
          f"{res['seconds']:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
