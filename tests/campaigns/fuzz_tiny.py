"""Tiny and ragged shapes (1 x 1 up to ~70 x 90, every width residue, planes shorter than a filter's reach) through
every operator of the path, against the CPU oracle / scipy.  The fast kernels have minimum sizes and alignment rules;
this sweep lives in the fallbacks and at the switch-over points.  Usage: fuzz_tiny.py [cases] [seed]."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from scipy import ndimage as ndi
from arcadia_microscopy_tools_amd.device import get_context
from arcadia_microscopy_tools_amd.operations import rescale_by_percentile, subtract_background_dog
from oracle import skops
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/: the sweep's table and checks
import operator_sweep as sweep


def draw(op):
    """This case's parameter sets of one operator of the table: as before the campaign moved onto the table, one random
    draw per operator and case (a mode, a footprint, a window), not the suite's full lists."""
    P = list(op.params)
    one = lambda sel: (lambda c: [c[int(rng.integers(0, len(c)))]])([p for p in P if sel(p)])
    if op.name == "gaussian":
        mode = ("nearest", "reflect", "mirror", "constant")[int(rng.integers(0, 4))]
        return [("u16", sg, mode) for sg in (0.6, 2.0)]
    if op.name == "apply_threshold global":
        return [p for p in P if p[0] == "u16"]
    if op.name == "window_threshold":
        w = one(lambda p: p[0] == "u16")[0][2]
        return [("u16", m, w) for m in ("niblack", "sauvola")]
    if op.name in ("apply_threshold local", "median"):
        return one(lambda p: p[0] == "u16")
    if op.name == "grey morphology":
        f = one(lambda p: p[0] == "u16")[0][2]
        return [p for p in P if p[0] == "u16" and p[2] == f]
    if op.name == "binary morphology":
        f = one(lambda p: True)[0][1]
        return [p for p in P if p[1] == f]
    if op.name == "label":
        return [("mask", 1), ("mask", 2), ("int32", 2)]
    return [{"edt": "mask", "label operators": "clear_border", "regionprops": "u16"}[op.name]]


def name_of(op, p):
    """The check names this campaign has always printed."""
    if op == "apply_threshold global":
        return "threshold " + p[1]
    if op == "window_threshold":
        return "threshold " + p[1]
    if op == "apply_threshold local":
        return "threshold local"
    if op == "grey morphology":
        return p[1]
    if op == "binary morphology":
        return "binary_" + p[0]
    if op == "label":
        return "label int" if p[0] == "int32" else "label"
    if op == "label operators":
        return "clear_border"
    return op


SWEEP_OPS = {o.name: o for o in sweep.OPS if o.name in (
    "gaussian", "apply_threshold global", "window_threshold", "apply_threshold local", "grey morphology", "median",
    "binary morphology", "label", "edt", "label operators", "regionprops")}

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
ctx = get_context()
bad = 0
counts = {}


def check(name, ok, info):
    global bad
    counts[name] = counts.get(name, 0) + 1
    if not ok:
        bad += 1
        print("MISMATCH", name, info, flush=True)


for case in range(ncases):
    if rng.random() < 0.35:
        H, W = int(rng.integers(1, 12)), int(rng.integers(1, 12))
    else:
        H, W = int(rng.integers(1, 70)), int(rng.integers(1, 90))
    shp = (H, W)
    img = rng.integers(0, 65536, shp).astype(np.uint16)
    if rng.random() < 0.3:  # smooth content: ties and plateaus
        img = (ndi.uniform_filter(img.astype(np.float64), 3) // 257 * 257).astype(np.uint16)
    got = subtract_background_dog(img, low_sigma=0.6, high_sigma=float(rng.choice([1.5, 4.0, 16.0])))
    check("dog finite", got.shape == shp and np.isfinite(got).all() and (got >= 0).all(), shp)
    dog = skops.difference_of_gaussians(img, 0.6, 3.0)
    exp = np.clip(dog - np.percentile(dog, 0), 0, None)
    check("dog", np.array_equal(subtract_background_dog(img, low_sigma=0.6, high_sigma=3.0), exp), shp)
    # percentile rescale
    lo, hi = sorted(rng.uniform(0, 100, 2))
    if hi - lo > 1e-3:
        got = rescale_by_percentile(img, percentile_range=(lo, hi))
        if img.min() == img.max():
            exp = np.zeros(shp)
        else:
            p1, p2 = np.percentile(img, (lo, hi))
            exp = skops.rescale_intensity(img, (p1, p2), (0.0, 1.0)) if p1 != p2 else None
        if exp is not None:
            check("rescale", np.array_equal(got, exp), (shp, lo, hi))
    # Gaussians, thresholds, grey and binary morphology, median, labels, EDT, clear_border, region properties: the
    # checks of the suite's operator sweep (tests/operator_sweep.py), on this case's shape and with planes of its own
    sweep.set_seed(int(rng.integers(0, 2 ** 31)))
    drawn = {name: draw(op) for name, op in SWEEP_OPS.items()}
    for name, op in SWEEP_OPS.items():
        by_repr = {repr(p): p for p in op.params}
        for r in sweep.run(ctx, ops=[name], shapes=[shp], only=("single",), pick=lambda o, p: p in drawn[o.name])["records"]:
            check(name_of(name, by_repr[r["param"]]), r["status"] == "pass", (shp, r["param"], r["index"]))
    if case % 50 == 49:
        print(f"{case + 1}/{ncases} cases, bad {bad}", flush=True)
# config 3 end to end on small, non-square windows of synthetic FOVs (nuclei cut by the frame, a handful of cells)
from arcadia_microscopy_tools_amd import synth
from arcadia_microscopy_tools_amd.segment import segment_fovs
from oracle import chains
for case in range(max(10, ncases // 10)):
    H2, W2 = int(rng.integers(12, 160)), int(rng.integers(12, 160))
    big = synth.synth_fov(3000 + case, size=192)
    y0, x0 = int(rng.integers(0, 192 - H2 + 1)), int(rng.integers(0, 192 - W2 + 1))
    fovs = np.ascontiguousarray(np.stack([big[:, y0:y0 + H2, x0:x0 + W2], big[:, :H2, :W2]]))
    res = segment_fovs(fovs, max_cells=512)
    lab, tabs = res.labels_numpy(), res.feature_tables()
    for j in range(2):
        rl, rpp = chains.c3_chain(fovs[j])
        check("c3 labels", np.array_equal(lab[j], rl), ((H2, W2), j))
        check("c3 props", all(np.allclose(tabs[j][c], rpp[c], rtol=1e-5, atol=1e-8) for c in rpp if c != "orientation"),
              ((H2, W2), j, int(rl.max())))
print({k: v for k, v in sorted(counts.items())})
print("BAD", bad)
sys.exit(1 if bad else 0)
