"""Every ``hipops.binary_fill_holes`` case of tests/test_gpu_fill_holes.py as a function, and as a program:
``python -m tests.fill_holes_cases --json OUT`` runs them in a process of its own (under ``AMT_DEBUG_POISON=1`` with a
scratch check after every call) and writes the digests of all outputs.

A case = (shape, generator, structure), run three ways: the plane alone, as plane 1 of a two-plane stack (an address
that is no multiple of 16 for shapes such as (70, 131) and (15, 24)), and inside a batch of three different planes in
one call.  Every output is compared with scipy, byte for byte.
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

import fill_holes_reference as ref  # noqa: E402
import poison_child  # noqa: E402


def _sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_shape(ctx, shape, scratch_check=False):
    """-> {"digests": {key: sha256}, "mismatches": [key], "dirty": [(key, finding)], "calls": n} for one shape."""
    from arcadia_microscopy_tools_amd import hipops

    digests, bad, dirty = {}, [], []
    calls = 0

    def fill(d, st, key):
        nonlocal calls
        out = hipops.binary_fill_holes(d, st)
        calls += 1
        if scratch_check:
            found = ctx.scratch_check()
            if found is not None:
                dirty.append((key, list(found)))
        return out.numpy(dtype=np.uint8)

    named = ref.planes(tuple(shape))
    for sname, st in ref.STRUCTURES:
        want = {n: ref.scipy_fill(p, st) for n, p in named}
        single = {}
        for n, p in named:
            key = f"{shape[0]}x{shape[1]}/{n}/{sname}"
            got = fill(ctx.asarray(p), st, key + "/single")
            single[n] = got
            digests[key + "/single"] = _sha(got)
            if not np.array_equal(got, want[n]):
                bad.append(key + "/single")
            # plane 1 of a two-plane stack whose plane 0 is something else
            stack = ctx.asarray(np.stack([1 - p, p]))
            got1 = fill(stack[1], st, key + "/plane1")
            digests[key + "/plane1"] = _sha(got1)
            if not np.array_equal(got1, want[n]):
                bad.append(key + "/plane1")
        # batches of three different planes in one call (the last batch wraps round)
        for i in range(0, len(named), 3):
            trio = [named[(i + j) % len(named)] for j in range(3)]
            key = f"{shape[0]}x{shape[1]}/batch{i // 3}/{sname}"
            got3 = fill(ctx.asarray(np.stack([p for _, p in trio])), st, key)
            digests[key] = _sha(got3)
            for j, (n, _) in enumerate(trio):
                if not np.array_equal(got3[j], single[n]) or not np.array_equal(got3[j], want[n]):
                    bad.append(f"{key}/{n}")
    return {"digests": digests, "mismatches": bad, "dirty": dirty, "calls": calls}


def run(ctx, scratch_check=False, shapes=None):
    t0 = time.perf_counter()
    res = {"digests": {}, "mismatches": [], "dirty": [], "calls": 0}
    for shape in shapes or ref.SHAPES:
        r = run_shape(ctx, shape, scratch_check)
        res["digests"].update(r["digests"])
        res["mismatches"] += r["mismatches"]
        res["dirty"] += r["dirty"]
        res["calls"] += r["calls"]
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
