"""Every operator at both ends of its documented PARAMETER ranges, at each switch inside them and one step beyond each
end: the table, the limits it is built from, and the runner.

tests/operator_sweep.py moves the shape and tests/worstcase_content.py the content; the parameters of both stay in the
middle of their ranges (256 bins, disk(7), windows up to 15, radius up to 16, three planes).  include/amt_hip.h and the
AMT_REQUIRE lines document much wider ranges, and the kernels switch code paths inside them: the float64 Otsu kernel's LDS
arrays grow with nbins, hist_u16_launch leaves the part kernel beyond HIST_MAX_PARTS parts, the Gaussian leaves the fused
kernels beyond FR_MAX, threshold_open_close leaves its fused kernel beyond a 16-row / 64-column halo, ...

``limits()`` reads the ends and the switches from the sources by pattern, ``ranges(lim)`` names every range with its ends,
switches and the first value refused on either side, and ``table()`` is the list of cases: each carries marks
(range, role, value) saying which end or switch it sits on.  Every reference is the one the operator's existing test
uses, with that test's rule (tests/operator_sweep.py: ``exact``, ``close``, ``same_bits``, ``props_rule``, ...).  A
refusal case makes ONE call just outside a range and expects the library's ValueError (AMT_EINVAL) or the wrapper's own
exception; tests/test_host_parameter_limits.py shows from the source text that the refusal comes before the entry
point's first launch.  ``amt_nn_affine_act_bf16`` (torch tensors) has a group of its own, against a float64 evaluation of
its definition rounded once to bf16.

``run(ctx, groups, scratch_check)`` returns one record per case in the form of tests/operator_sweep.py (whose Recorder,
rules and digest it uses).  ``python -m tests.parameter_limits --json PATH [--profile PATH]`` runs everything.  Not
collected by pytest (tests/test_host_parameter_limits.py and tests/test_gpu_parameter_limits.py are)."""
from __future__ import annotations

import json
import os
import re
import sys
import time

import numpy as np
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import colocalization_reference as coloc_ref  # noqa: E402
import expand_labels_reference as expand_ref  # noqa: E402
import operator_sweep as sw  # noqa: E402
import poison_child  # noqa: E402
from oracle import blending as oblend  # noqa: E402
from oracle import regionprops as orp  # noqa: E402
from oracle import skops  # noqa: E402

_F64, _F32, _U16, _I32, _U8, _U32 = np.float64, np.float32, np.uint16, np.int32, np.uint8, np.uint32
CSRC = os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc")
LDS_BYTES = 160 * 1024  # of one gfx950 workgroup


# ---------------------------------------------------------------------------------------------------------------------
# the limits, read from the sources
# ---------------------------------------------------------------------------------------------------------------------
def sources():
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
    src["amt_hip.h"] = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    src["operations.py"] = open(os.path.join(ROOT, "arcadia_microscopy_tools_amd", "operations.py")).read()
    return src


def limits():
    """The constants the switches compare with and the literal bounds of the AMT_REQUIRE lines, by pattern: a retune
    changes what this returns, and tests/test_host_parameter_limits.py then says which case no longer sits on its end."""
    src = sources()

    def const(f, name):
        m = re.search(r"constexpr (?:int|size_t) (?:\w+ = \d+, )*" + name + r" = (\d+)[,;]", src[f])
        assert m, f"{name} not found in {f}"
        return int(m.group(1))

    def bound(f, pattern, n=1):
        ms = re.findall(pattern, src[f])
        assert len(ms) >= n, f"{pattern!r} not found {n} times in {f}"
        assert len(set(ms)) == 1, f"{pattern!r} has different values in {f}: {ms}"
        m = ms[0]
        return tuple(int(v) for v in m) if isinstance(m, tuple) else int(m)

    out = {}
    for f, names in (("amt_stats.hip", ("HIST_PART_PX", "HIST_MAX_PARTS", "PQ_MIN_N")), ("amt_filters.hip", ("FR_MAX", "H8G_CP")),
                     ("amt_edt.hip", ("PK_MAXM",)), ("amt_morph.hip", ("MAX_OFFS", "TOC_MAX_OFFS")),
                     ("amt_rank.hip", ("RK_MAX_OFFS",)), ("amt_overlay.hip", ("OV_MAX_LAYERS",)),
                     ("amt_props.hip", ("RP_MAXC", "COLOC_MAXC"))):
        for name in names:
            out[name] = const(f, name)
    m = re.search(r"#define AMT_PEAK_MARKERS_LDS_TIER (\d+)", src["amt_hip.h"])
    assert m, "AMT_PEAK_MARKERS_LDS_TIER"
    out["AMT_PEAK_MARKERS_LDS_TIER"] = int(m.group(1))
    st = "amt_stats.hip"
    out["HIST_F64_NBINS"] = bound(st, r'AMT_REQUIRE\(nbins >= (\d+) && nbins <= (\d+), "hist_f64')
    out["OTSU_F64_NBINS"] = bound(st, r'\(nbins >= (\d+) && nbins <= (\d+)\), "threshold_value')
    out["PCT_U16_NQ"] = bound(st, r'AMT_REQUIRE\(nq >= (\d+) && nq <= (\d+), "percentile_u16')
    out["PCT_F64_NQ"] = bound(st, r'AMT_REQUIRE\(nq >= (\d+) && nq <= (\d+), "percentile_f64')
    out["HIST_RANGE_LOG2"] = bound(st, r"AMT_REQUIRE\(nbins <= \(1ll << (\d+)\), \"hist_range_f64")
    # the dynamic LDS of otsu_f64_kernel in arrays of nbins doubles, and its static part (s_val[4], s_idx[4])
    out["OTSU_LDS_ARRAYS"] = bound(st, r"otsu_f64_kernel, dim3\(nplanes\), dim3\(256\), \(size_t\)(\d+) \* nbins \* sizeof\(double\)")
    body = function_body(src[st], "otsu_f64_kernel")
    assert "__shared__ double s_val[4];" in body and "__shared__ int s_idx[4];" in body
    out["OTSU_LDS_STATIC"] = 4 * 8 + 4 * 4
    out["GAUSS_RADIUS"] = bound("amt_filters.hip", r'AMT_REQUIRE\(r >= (\d+) && r <= (\d+), "gaussian')
    out["WINDOW_MAX"] = bound("amt_window.hip", r"AMT_REQUIRE\(window_y <= (\d+) && window_x <= \1,", 2)
    assert bound("amt_window.hip", r"AMT_REQUIRE\(lead_window\[a\] <= (\d+),") == out["WINDOW_MAX"]
    out["NLEAD_MAX"] = bound("amt_window.hip", r"nlead >= 0 && nlead <= (\d+)")
    out["FOOTPRINT_SIDE"] = bound("amt_morph.hip", r'AMT_REQUIRE\(fh <= (\d+) && fw <= \1, "footprint larger')
    assert bound("amt_rank.hip", r"fh >= 1 && fw >= 1 && fh <= (\d+) && fw <= \1,") == out["FOOTPRINT_SIDE"]
    out["TOC_HALO"] = bound("amt_morph.hip", r"noffs <= TOC_MAX_OFFS && 4 \* ry <= (\d+) && 4 \* rx <= (\d+)\)")
    out["SIDE_MAX"] = bound("amt_edt.hip", r'AMT_REQUIRE\(H <= (\d+) && W <= \1, "edt')
    assert bound("amt_expand.hip", r'AMT_REQUIRE\(H <= (\d+) && W <= \1, "expand_labels') == out["SIDE_MAX"]
    out["PLANES_MAX"] = bound("amt_normalize.hip", r"nplanes >= 0 && nplanes <= (\d+), \"normalize_planes_f32")
    assert bound("amt_expand.hip", r'AMT_REQUIRE\(nplanes <= (\d+), "expand_labels') == out["PLANES_MAX"]
    out["NN_ROWS_PER_LAUNCH"] = bound("amt_nn.hip", r"row0 < rows; row0 \+= (\d+)\)")
    out["NN_MAX_BLOCKS_X"] = bound("amt_nn.hip", r"amt_grid_for\(\(size_t\)W \* C8, 256, (\d+)\)")
    out["MAX_INTEGER_BINS_LOG2"] = bound("operations.py", r"_MAX_INTEGER_BINS = 1 << (\d+)")
    # the dispatch rules the table restates: their text is pinned here
    assert "if (parts * (size_t)nplanes > (size_t)HIST_MAX_PARTS) return 0;" in src[st]
    assert "int bpp = (int)((n + 262143) / 262144);" in src[st] and "int cap = (2 * ctx->num_cus + nplanes - 1) / nplanes;" in src[st]
    assert "if (n < PQ_MIN_N) return percentile_f64_radix(" in src[st]
    fl = src["amt_filters.hip"]
    out["V8G_LDS_KIB"] = bound("amt_filters.hip", r"constexpr size_t V8G_LDS_MAX = (\d+) \* 1024;")
    assert "const int TH_G = sizeof(TIn) == 2 ? 128 : 64;" in fl
    assert ("const size_t smem_g = (size_t)((TH_G + 2 * r + 7) & ~7) * 64 * sizeof(TIn) + (size_t)(2 * r + 1) * 8 + "
            "(size_t)(TH_G + 2 * r);") in fl
    assert "if (aligned && W % 64 == 0 && H > 2 * r && smem_g <= V8G_LDS_MAX) {" in fl
    assert "if (radius == 0) {  // sigma too small: scipy's kernel is the single weight 1.0" in fl
    assert fl.count("if (r == 64)") == 2 and "conv_v8g_kernel<TIn, 64>" in fl and "conv_h8g_kernel<ROWS, 64>" in fl
    assert "const int tw_g = ((H8G_CP - 2 * r - 1) / 8) * 8;" in fl
    assert "aligned && W % 2 == 0 && tw_g >= 64 && W >= H8G_CP + 2 * r && mode != AMT_MODE_WRAP;" in fl
    assert "const bool aligned = (W % 8 == 0) && W >= 256 && (in_stride % 8 == 0)" in fl and "if (aligned && modeok && H > 2 * R) {" in fl
    assert "AMT_FUSED_CASE(%d)" % out["FR_MAX"] in fl and "AMT_FUSED_CASE(%d)" % (out["FR_MAX"] + 1) not in fl
    assert "const int w = c8_shift >= 0 ? i >> c8_shift : i / C8;" in src["amt_nn.hip"]
    return out


def function_body(text, name):
    """The text of the definition of ``name`` (a kernel, a static helper or an extern "C" entry point) up to its closing
    brace in column 0."""
    m = re.search(r"^[^\n/]*\b" + re.escape(name) + r"\([^;{]*\{\n", text, re.M)
    assert m, f"{name}: definition not found"
    end = text.find("\n}\n", m.end())
    assert end > 0, name
    return text[m.start():end]


_LAUNCH = re.compile(r"hipLaunchKernelGGL|hipMemsetAsync")


def refusal_precedes_launch(src, steps):
    """steps: ((file, function, fragment), ...): in each function's text the fragment (the AMT_REQUIRE's condition, or the
    call of the helper that holds it) stands before the first hipLaunchKernelGGL / hipMemsetAsync."""
    for f, fn, fragment in steps:
        body = function_body(src[f], fn)
        at = body.find(fragment)
        if at < 0:
            return False, f"{fn}: {fragment!r} not found"
        m = _LAUNCH.search(body)
        if m and m.start() < at:
            return False, f"{fn}: a launch stands before {fragment!r}"
    return True, None


def ranges(lim=None):
    """Every documented range: {"lo", "hi"} (None: that end belongs to another suite or does not exist), "switches"
    {role: value} inside it and "refuse" {role: value} just outside it.  The table carries a case per entry."""
    lim = lim or limits()
    hb, ob, qu, qf, gr = lim["HIST_F64_NBINS"], lim["OTSU_F64_NBINS"], lim["PCT_U16_NQ"], lim["PCT_F64_NQ"], lim["GAUSS_RADIUS"]
    fit = (LDS_BYTES - lim["OTSU_LDS_STATIC"]) // 40  # 40 bytes of LDS per bin would end here; the kernel takes 32
    v8 = v8g_f64_radius(lim)
    top = 1 << lim["HIST_RANGE_LOG2"]
    return {
        "hist_f64 nbins": dict(lo=hb[0], hi=hb[1], switches={}, refuse={"lo": hb[0] - 1, "hi": hb[1] + 1}),
        "otsu_f64 nbins": dict(lo=ob[0], hi=ob[1], switches={"40 bytes per bin would fit LDS": fit, "40 bytes per bin would not": fit + 1},
                               refuse={"lo": ob[0] - 1, "hi": ob[1] + 1}),
        "hist_range nbins": dict(lo=1, hi=top, switches={"what operations.py asks for": 1 << lim["MAX_INTEGER_BINS_LOG2"]},
                                 refuse={"lo": 0, "hi": top + 1}),
        "percentile_f64 nq": dict(lo=qf[0], hi=qf[1], switches={"samples below PQ_MIN_N": 256, "samples at PQ_MIN_N": lim["PQ_MIN_N"]},
                                  refuse={"lo": qf[0] - 1, "hi": qf[1] + 1}),
        "percentile_u16 nq": dict(lo=qu[0], hi=qu[1], switches={}, refuse={"lo": qu[0] - 1, "hi": qu[1] + 1}),
        "hist_u16 parts": dict(lo=None, hi=None, refuse={}, switches={
            "scalar loads, HIST_MAX_PARTS parts": lim["HIST_MAX_PARTS"], "scalar loads, one part more": lim["HIST_MAX_PARTS"] + 1,
            "vector loads, HIST_MAX_PARTS parts": lim["HIST_MAX_PARTS"], "vector loads, one part more": lim["HIST_MAX_PARTS"] + 1,
            "two workgroups per plane": 2}),
        "gaussian radius": dict(lo=gr[0], hi=gr[1], refuse={"hi": gr[1] + 1},
                                switches={"smallest fused": 1, "FR_MAX": lim["FR_MAX"], "FR_MAX + 1": lim["FR_MAX"] + 1}),
        "gaussian vertical pass": dict(lo=None, hi=None, refuse={}, switches={
            "conv_v8g at the largest radius": gr[1], "conv_v8 at the largest radius": gr[1],
            "float64 conv_v8g at its largest radius": v8, "float64 on conv_v8 where the staged tile passes LDS": v8 + 1,
            "the r == 64 instantiations": 64}),
        "window": dict(lo=1, hi=lim["WINDOW_MAX"], switches={}, refuse={"hi": lim["WINDOW_MAX"] + 2, "even": 4}),
        "window nlead": dict(lo=1, hi=lim["NLEAD_MAX"], switches={}, refuse={"hi": lim["NLEAD_MAX"] + 1}),
        "footprint side": dict(lo=1, hi=lim["FOOTPRINT_SIDE"], switches={}, refuse={"hi": lim["FOOTPRINT_SIDE"] + 2}),
        "binary footprint cells": dict(lo=1, hi=lim["MAX_OFFS"], switches={}, refuse={"hi": lim["MAX_OFFS"] + 1}),
        "rank footprint cells": dict(lo=1, hi=lim["RK_MAX_OFFS"], switches={}, refuse={"hi": lim["RK_MAX_OFFS"] + 1}),
        "threshold_open_close footprint": dict(lo=None, hi=None, refuse={}, switches={
            "ry at the fused halo": lim["TOC_HALO"][0] // 4, "ry beyond it": lim["TOC_HALO"][0] // 4 + 1,
            "rx at the fused halo": lim["TOC_HALO"][1] // 4, "rx beyond it": lim["TOC_HALO"][1] // 4 + 1,
            "TOC_MAX_OFFS cells": lim["TOC_MAX_OFFS"], "TOC_MAX_OFFS + 1 cells": lim["TOC_MAX_OFFS"] + 1}),
        "min_distance": dict(lo=0, hi=lim["PK_MAXM"], switches={}, refuse={"lo": -1, "hi": lim["PK_MAXM"] + 1}),
        "side": dict(lo=1, hi=lim["SIDE_MAX"], switches={}, refuse={"hi": lim["SIDE_MAX"] + 1}),
        "planes": dict(lo=None, hi=lim["PLANES_MAX"], switches={}, refuse={"hi": lim["PLANES_MAX"] + 1}),
        "overlay layers": dict(lo=0, hi=lim["OV_MAX_LAYERS"], switches={}, refuse={"hi": lim["OV_MAX_LAYERS"] + 1}),
        "regionprops channels": dict(lo=None, hi=None, refuse={}, switches={"two groups of RP_MAXC": 2 * lim["RP_MAXC"],
                                                                             "three groups": 2 * lim["RP_MAXC"] + 1}),
        "colocalization channels": dict(lo=2, hi=None, refuse={}, switches={"more than COLOC_MAXC": lim["COLOC_MAXC"] + 2}),
        "affine channels": dict(lo=8, hi=None, switches={"C / 8 not a power of two": 24, "C / 8 a power of two": 64},
                                refuse={"not a multiple of 8": 12}),
        "affine rows": dict(lo=None, hi=None, refuse={}, switches={"a second launch": lim["NN_ROWS_PER_LAUNCH"] + 1}),
        "affine groups per row": dict(lo=None, hi=None, refuse={}, switches={"the grid-stride loop": 2 * 256 * lim["NN_MAX_BLOCKS_X"]}),
    }


def hist_u16_kernel_of(lim, nplanes, n):
    """hist_u16_scratch_bytes' rule: which kernel hist_u16_launch takes, and with how many parts / workgroups per plane
    (``num_cus`` only caps the latter from above: 2 * 256 CUs / nplanes, rounded up)."""
    parts = (n + lim["HIST_PART_PX"] - 1) // lim["HIST_PART_PX"]
    if n == 0 or parts * nplanes <= lim["HIST_MAX_PARTS"]:
        return "hist_u16_part_kernel", parts
    return "hist_u16_kernel", max(1, (n + 262143) // 262144)


def v8g_smem(r, itemsize):
    """The dynamic LDS conv_v8g_kernel would be launched with (gaussian_typed's smem_g): the staged tile of
    TH + 2 r rows (rounded up to 8) of 64 raw samples, the weights and one byte per row."""
    th = 128 if itemsize == 2 else 64
    return ((th + 2 * r + 7) & ~7) * 64 * itemsize + (2 * r + 1) * 8 + th + 2 * r


def v8g_f64_radius(lim):
    """The largest radius at which a float64 plane still takes conv_v8g_kernel."""
    return max(r for r in range(lim["GAUSS_RADIUS"][1] + 1) if v8g_smem(r, 8) <= lim["V8G_LDS_KIB"] * 1024)


def gaussian_path(lim, dt, r, mode, shape):
    """amt_gaussian / gaussian_typed / launch_fused's dispatch for one aligned plane -> the kernels' names."""
    H, W = shape
    if r == 0:  # amt_gaussian answers itself: the single weight 1.0
        return "convert_u16_f64" if dt == "u16" else "copy_f64"
    if r <= lim["FR_MAX"]:
        lds = dt == "u16" and W % 8 == 0 and W >= 256 and mode in ("nearest", "reflect", "mirror") and H > 2 * r
        return "gauss_lds" if lds else "gauss_fused"
    t64 = "<64>" if r == 64 else ""  # the two LDS-DMA kernels have an instantiation of their own for this radius
    fits = v8g_smem(r, 2 if dt == "u16" else 8) <= lim["V8G_LDS_KIB"] * 1024
    v = "v8g" + t64 if W % 64 == 0 and H > 2 * r and fits else "v8"
    tw_g = ((lim["H8G_CP"] - 2 * r - 1) // 8) * 8
    h = "h8g" + t64 if W % 2 == 0 and tw_g >= 64 and W >= lim["H8G_CP"] + 2 * r and mode != "wrap" else "h8"
    return f"conv_{v} + conv_{h}"


def toc_path(lim, fp):
    ry, rx = fp.shape[0] // 2, fp.shape[1] // 2
    fused = int(np.count_nonzero(fp)) <= lim["TOC_MAX_OFFS"] and 4 * ry <= lim["TOC_HALO"][0] and 4 * rx <= lim["TOC_HALO"][1]
    return "toc_fused" if fused else "packed_prim x 4"


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
_ONCE: dict = {}


def _once(key, fn):
    """Inputs and references: made once, shared, read-only."""
    if key not in _ONCE:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray) and a.dtype != object:
                a.setflags(write=False)
        _ONCE[key] = v
    return _ONCE[key]


def forget(prefix):
    """Drops the large inputs and references of one group."""
    for k in [k for k in _ONCE if k[0] == prefix]:
        del _ONCE[k]


class Case:
    """run(ctx) -> tuple of host arrays; want() -> the same tuple from the reference; rules: one rule or one per output;
    marks: ((range, role, value), ...); expect: the exception classes of a refusal (run must raise one of them);
    source: the steps of ``refusal_precedes_launch``."""

    def __init__(self, group, op, name, shape, run, want=None, rules=sw.exact, marks=(), expect=None, source=None):
        self.group, self.op, self.name, self.shape, self.run, self.want = group, op, name, tuple(shape), run, want
        self.rules, self.marks, self.expect, self.source = rules, tuple(marks), expect, source

    def key(self):
        return (self.group, self.op, self.name, self.shape)


def _h():
    from arcadia_microscopy_tools_amd import hipops

    return hipops


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _mark(lim_ranges, rng_name, value):
    """The marks of a case whose parameter of range ``rng_name`` is ``value``."""
    r = lim_ranges[rng_name]
    out = [(rng_name, role, value) for role in ("lo", "hi") if r[role] is not None and r[role] == value]
    out += [(rng_name, "switch " + role, value) for role, v in r["switches"].items() if v == value]
    return out


# ---- histograms and thresholds (float64) ----------------------------------------------------------------------------
def _f64_planes():
    return {"random": sw.img_f64((33, 40), 0), "few values": sw.img_f64((66, 320), 2),
            "smooth": _once(("in", "smooth"), lambda: skops.gaussian(sw.img_u16((66, 320), 0), 2.0)),
            "one sample": sw.img_f64((1, 1), 0), "constant": np.full((7, 5), 0.25)}


def _g_hist_f64(lim, R):
    g, cases = "histograms and thresholds f64", []
    planes = _f64_planes()
    for nbins in (1, 2, 255, 257, 1024, 4096):
        for pn, x in planes.items():
            cases.append(Case(g, "histogram_f64", f"nbins {nbins} {pn}", x.shape,
                              lambda ctx, x=x, nbins=nbins: tuple(a[0] for a in sw._np(*_h().histogram_f64(ctx.asarray(x[None]), nbins))),
                              lambda x=x, nbins=nbins: (np.histogram(x, bins=nbins)[0].astype(_U32), np.array([x.min(), x.max()])),
                              marks=_mark(R, "hist_f64 nbins", nbins)))
    ob = R["otsu_f64 nbins"]
    def otsu_ref(x, nbins):  # a constant plane gives its value (the rule of the sweep's "otsu f64")
        return (np.asarray(float(x.flat[0]) if x.min() == x.max() else skops.threshold_otsu(x, nbins), _F64),)

    for nbins in (2, 3, 255, 257, 1024, *sorted(ob["switches"].values()), ob["hi"]):
        for pn, x in planes.items():
            cases.append(Case(g, "threshold_otsu", f"nbins {nbins} {pn}", x.shape,
                              lambda ctx, x=x, nbins=nbins: (_h().threshold_otsu(ctx.asarray(x[None]), nbins=nbins).numpy()[0],),
                              lambda x=x, nbins=nbins: otsu_ref(x, nbins), marks=_mark(R, "otsu_f64 nbins", nbins)))

    def value(ctx, x, nbins):
        from arcadia_microscopy_tools_amd.operations import otsu_threshold_value

        return (np.asarray(otsu_threshold_value(x, nbins=nbins), _F64),)

    sm = planes["smooth"]
    cases.append(Case(g, "otsu_threshold_value", f"nbins {ob['hi']} smooth", sm.shape, lambda ctx: value(ctx, sm, ob["hi"]),
                      lambda: (np.asarray(skops.threshold_otsu(sm, ob["hi"]), _F64),), marks=_mark(R, "otsu_f64 nbins", ob["hi"])))

    def mask(ctx, x, method, nbins):
        from arcadia_microscopy_tools_amd.operations import apply_threshold

        return sw._np(apply_threshold(ctx.asarray(x), method, nbins=nbins))

    for method in ("yen", "isodata", "triangle"):
        for nbins in (16, R["hist_f64 nbins"]["hi"]):
            for pn in ("random", "few values", "smooth"):
                x = planes[pn]
                cases.append(Case(g, "apply_threshold " + method, f"nbins {nbins} {pn}", x.shape,
                                  lambda ctx, x=x, method=method, nbins=nbins: mask(ctx, x, method, nbins),
                                  lambda x=x, method=method, nbins=nbins: (x > getattr(skops, "threshold_" + method)(x, nbins),),
                                  marks=_mark(R, "hist_f64 nbins", nbins)))
    return cases


def _range_samples(lo, nbins):
    """Samples at lo - 1, lo, lo + nbins - 1, lo + nbins and a few inside (some twice), as a (3, 4) float64 plane."""
    inside = [lo + (nbins * k) // 7 for k in (1, 2, 2, 3, 5, 5, 5)] if nbins > 1 else [lo] * 7
    v = [lo - 1, lo, lo + nbins - 1, lo + nbins] + inside + [lo + nbins - 1]
    return np.array(v, _F64).reshape(3, 4)


def _g_hist_range(lim, R):
    g, cases, lo = "histogram_range", [], -5
    r = R["hist_range nbins"]

    def dev(ctx, x, nbins):
        h = _h().histogram_range(ctx.asarray(x[None]), lo, nbins).numpy()[0]
        nz = np.flatnonzero(h)
        out = (nz.astype(np.int64), h[nz].astype(_U32), np.asarray(np.count_nonzero(h), np.int64))
        del h
        ctx.trim()  # a gibibyte of bins does not stay in the pool
        return out

    def ref(x, nbins):
        v = x.ravel()
        v = v[(v >= lo) & (v < lo + nbins)].astype(np.int64) - lo
        u, c = np.unique(v, return_counts=True)
        return u.astype(np.int64), c.astype(_U32), np.asarray(u.size, np.int64)

    for nbins in (r["lo"], r["switches"]["what operations.py asks for"], r["hi"]):
        x = _range_samples(lo, nbins)
        cases.append(Case(g, "histogram_range", f"nbins {nbins}", x.shape, lambda ctx, x=x, nbins=nbins: dev(ctx, x, nbins),
                          lambda x=x, nbins=nbins: ref(x, nbins), marks=_mark(R, "hist_range nbins", nbins)))
    return cases


# ---- percentiles ----------------------------------------------------------------------------------------------------
def _q_of(nq):
    """Unsorted, repeated, with several 0 and 100 where there is room."""
    base = [100, 0, 50, 0, 100, 12.5, 50, 99.9, 0.1, 37.123]
    if nq <= len(base):
        return tuple(base[:nq]) if nq > 1 else (37.5,)
    return tuple(base + list(np.round(_rng(nq).uniform(0, 100, nq - len(base)), 3)))


def _g_percentiles(lim, R):
    g, cases = "percentiles", []
    rf, ru = R["percentile_f64 nq"], R["percentile_u16 nq"]
    for shape in ((16, 16), (256, 256)):
        n = shape[0] * shape[1]
        for kind in (0, 2):
            x = sw.img_f64(shape, kind)
            for nq in (rf["lo"], rf["hi"] - 1, rf["hi"]):
                q = _q_of(nq)
                cases.append(Case(g, "percentile f64", f"nq {nq} kind {kind}", shape,
                                  lambda ctx, x=x, q=q: (_h().percentile(ctx.asarray(x[None]), q).numpy()[0],),
                                  lambda x=x, q=q: (np.atleast_1d(np.percentile(x, q)),),
                                  marks=_mark(R, "percentile_f64 nq", nq) + _mark(R, "percentile_f64 nq", n)))
    for shape in ((16, 16), (33, 40)):
        for kind in (0, 2):
            x = sw.img_u16(shape, kind)
            for nq in (ru["lo"], ru["hi"]):
                q = _q_of(nq)
                cases.append(Case(g, "percentile u16", f"nq {nq} kind {kind}", shape,
                                  lambda ctx, x=x, q=q: (_h().percentile(ctx.asarray(x[None]), q).numpy()[0],),
                                  lambda x=x, q=q: (np.atleast_1d(np.percentile(x, q)),), marks=_mark(R, "percentile_u16 nq", nq)))
    return cases


# ---- uint16 histogram regimes ---------------------------------------------------------------------------------------
def hist_regimes(lim):
    """(planes, plane shape, role of the case in the "hist_u16 parts" range): every call of histogram_u16, threshold_otsu
    and percentile on uint16 goes through hist_u16_launch."""
    mp = lim["HIST_MAX_PARTS"]
    return [(mp, (7, 5), "scalar loads, HIST_MAX_PARTS parts"), (mp + 1, (7, 5), "scalar loads, one part more"),
            (mp, (8, 8), "vector loads, HIST_MAX_PARTS parts"), (mp + 1, (8, 8), "vector loads, one part more"),
            (mp // 5 + 1, (512, 514), "two workgroups per plane")]


_REGIME_Q = (0, 1, 50, 99.9, 100)


def _regime_planes(nplanes, shape):
    """Values in both 32768-bin windows; plane 0 entirely below 32768 (the `win == 0 && !more` early exit), plane 1 entirely
    above."""
    def make():
        x = _rng(nplanes, shape[0], shape[1], 7).integers(0, 65536, (nplanes,) + shape, dtype=_U16)
        x[0] &= 0x7FFF
        x[1] |= 0x8000
        return x
    return _once(("regime", "in", nplanes, shape), make)


def _sparse(h):
    nz = np.flatnonzero(h)
    return nz.astype(np.int64), h.ravel()[nz].astype(_U32)


def _regime_hist_ref(nplanes, shape):
    def make():  # np.bincount per plane, kept in the sparse form of _sparse
        at, counts = [], []
        for i, p in enumerate(_regime_planes(nplanes, shape)):
            c = np.bincount(p.ravel(), minlength=65536)
            nz = np.flatnonzero(c)
            at.append(nz.astype(np.int64) + i * 65536)
            counts.append(c[nz].astype(_U32))
        return np.concatenate(at), np.concatenate(counts)
    return _once(("regime", "hist", nplanes, shape), make)


def _g_hist_regime(lim, R, nplanes, shape, role):
    g = f"hist_u16 {nplanes} x {shape}"
    kernel, per = hist_u16_kernel_of(lim, nplanes, shape[0] * shape[1])
    name = f"{nplanes} planes: {kernel}, {per} per plane"
    value = R["hist_u16 parts"]["switches"][role]
    marks = [("hist_u16 parts", "switch " + role, value)]
    dev_in = {}

    def d(ctx):  # one upload for the three operators
        if "x" not in dev_in:
            dev_in["x"] = ctx.asarray(_regime_planes(nplanes, shape))
        return dev_in["x"]

    def hist(ctx):
        out = _sparse(_h().histogram_u16(d(ctx)).numpy())
        ctx.trim()
        return out

    def last(ctx):
        out = (_h().percentile(d(ctx), _REGIME_Q).numpy(),)
        dev_in.clear()
        return out

    return [
        Case(g, "histogram_u16", name, shape, hist, lambda: _regime_hist_ref(nplanes, shape), marks=marks),
        Case(g, "threshold_otsu u16", name, shape, lambda ctx: (_h().threshold_otsu(d(ctx)).numpy(),),
             lambda: (np.array([skops.threshold_otsu(p) for p in _regime_planes(nplanes, shape)], _F64),), marks=marks),
        Case(g, "percentile u16", name, shape, last,
             lambda: (np.ascontiguousarray(np.percentile(_regime_planes(nplanes, shape).reshape(nplanes, -1), _REGIME_Q, axis=1).T),),
             marks=marks),
    ]


# ---- Gaussian -------------------------------------------------------------------------------------------------------
GAUSS_SHAPES = [(1, 1), (7, 5), (40, 256), (33, 512), (130, 576)]


def gauss_sigmas(lim):
    """sigma -> radius int(4 sigma + 0.5): both ends of the range, the smallest fused radius and the two sides of FR_MAX."""
    hi = lim["GAUSS_RADIUS"][1]
    return {0.1: 0, 0.25: 1, lim["FR_MAX"] / 4.0: lim["FR_MAX"], (lim["FR_MAX"] + 1) / 4.0 - 0.05: lim["FR_MAX"] + 1, hi / 4.0: hi}


# a plane tall enough for the LDS-DMA vertical pass at the largest radius (H > 2 * 128, W % 64 == 0)
GAUSS_TALL = (264, 576)


def gauss_grid(lim):
    """(shape, {sigma: radius}, modes): every shape at both ends, the smallest fused radius and the two sides of FR_MAX; the
    tall plane at the largest radius and on both sides of the radius where a float64 tile stops fitting the LDS-DMA
    vertical pass; the r == 64 instantiations of the two LDS-DMA kernels."""
    hi, v8 = lim["GAUSS_RADIUS"][1], v8g_f64_radius(lim)
    grid = [(shape, gauss_sigmas(lim), sw.MODES) for shape in GAUSS_SHAPES]
    grid.append((GAUSS_TALL, {v8 / 4.0: v8, (v8 + 1) / 4.0: v8 + 1, hi / 4.0: hi}, ("nearest", "reflect", "wrap")))
    grid.append(((130, 576), {16.0: 64}, sw.MODES))
    return grid


def _gauss_marks(lim, R, dt, r, path):
    marks = _mark(R, "gaussian radius", r)
    name = "gaussian vertical pass"
    roles = R[name]["switches"]
    hi, v8 = lim["GAUSS_RADIUS"][1], v8g_f64_radius(lim)
    took = {"conv_v8g at the largest radius": r == hi and path.startswith("conv_v8g "),
            "conv_v8 at the largest radius": r == hi and path.startswith("conv_v8 "),
            "float64 conv_v8g at its largest radius": dt == "f64" and r == v8 and path.startswith("conv_v8g "),
            "float64 on conv_v8 where the staged tile passes LDS": dt == "f64" and r == v8 + 1 and path.startswith("conv_v8 "),
            "the r == 64 instantiations": path == "conv_v8g<64> + conv_h8g<64>"}
    return marks + [(name, "switch " + role, roles[role]) for role, yes in took.items() if yes]


def _g_gaussian(lim, R):
    g, cases = "gaussian", []
    for shape, sigmas, modes in gauss_grid(lim):
        for dt in ("u16", "f64"):
            x = sw.img(dt, shape, 0)
            for sigma, r in sigmas.items():
                for mode in modes:
                    p = (dt, sigma, mode)
                    path = gaussian_path(lim, dt, r, mode, shape)
                    cases.append(Case(g, "gaussian", f"{dt} r {r} {mode}: {path}", shape,
                                      lambda ctx, x=x, p=p: (_h().gaussian(ctx.asarray(x[None]), p[1], mode=p[2], cval=0.25).numpy()[0],),
                                      lambda x=x, p=p: sw._gauss_ref((x,), p), marks=_gauss_marks(lim, R, dt, r, path)))
    codes = [o for o in sw.OPS if o.name == "gaussian_otsu_codes"][0]
    for shape in ((40, 256), (66, 320)):
        x = sw.img_u16(shape, 0)
        p = (0.25, "nearest")
        cases.append(Case(g, "gaussian_otsu_codes", "r 1 nearest", shape,
                          lambda ctx, x=x, p=p: tuple(o[0] for o in sw._codes_dev(ctx, [ctx.asarray(x[None])], [x[None]], p)),
                          lambda x=x, p=p: sw._codes_ref((x,), p),
                          rules=codes.rules_for(p), marks=_mark(R, "gaussian radius", 1)))
    for shape in ((7, 5), (33, 40)):
        for lead in (1, 2):  # a leading axis of length 1, and one shorter than the radius (4)
            for dt in ("u16", "f64"):
                vol = np.stack([sw.img(dt, shape, 0, 50 + i) for i in range(lead)])
                for mode in ("nearest", "reflect", "wrap"):
                    cases.append(Case(g, "gaussian_nd", f"{dt} leading axis {lead} {mode}", (lead,) + shape,
                                      lambda ctx, vol=vol, mode=mode: sw._np(_h().gaussian_nd(ctx.asarray(vol), 1.0, mode=mode)),
                                      lambda vol=vol, dt=dt, mode=mode: sw._nd_ref((vol,), (dt, mode, "gaussian"))))
    return cases


# ---- window thresholds ----------------------------------------------------------------------------------------------
def corner_mean_std(image, w):
    """skops._mean_std, bit for bit, in time that does not grow with the window: the oracle correlates the integral images
    with a dense (w + 1)^ndim kernel of which only the 2^ndim corners are not zero (half a minute per plane at w = 255, or for a
    window of 3 on eight axes).  scipy adds the kernel's products in raster order and a zero weight adds nothing, so the same
    sums come from the corner terms alone, in that order.  tests/test_host_parameter_limits.py compares the two on the
    windows the oracle can afford."""
    import itertools

    if not isinstance(w, (list, tuple, np.ndarray)):
        w = (w,) * image.ndim
    pad_width = tuple((k // 2 + 1, k // 2) for k in w)
    padded = np.pad(image.astype("float"), pad_width, mode="reflect")
    integral, integral_sq = padded.copy(), padded * padded
    for i in range(image.ndim):
        integral = np.cumsum(integral, axis=i)
        integral_sq = np.cumsum(integral_sq, axis=i)

    def correlate(a):  # ndi.correlate(a, kern, mode="constant"): out[i] = sum over j of kern[j] a[i + j - (k + 1) // 2]
        ap = np.pad(a, tuple(((k + 1) // 2, k - (k + 1) // 2) for k in w))
        out = np.zeros(a.shape)
        for indices in itertools.product(*([[0, -1]] * image.ndim)):
            sign = (-1) ** (image.ndim % 2 != np.sum(indices) % 2)
            out = out + sign * ap[tuple(slice(0 if j == 0 else k, (0 if j == 0 else k) + n) for j, k, n in zip(indices, w, a.shape))]
        return out

    total_window_size = np.prod(w)
    m = skops._crop(correlate(integral), pad_width) / total_window_size
    g2 = skops._crop(correlate(integral_sq), pad_width) / total_window_size
    return m, np.sqrt(np.clip(g2 - m * m, 0, None))


def window_ref(image, method, w, k=0.2, r=None):
    """skops.threshold_niblack / threshold_sauvola (their expressions) on corner_mean_std."""
    m, s = corner_mean_std(image, w)
    if method == "niblack":
        return m - k * s
    if r is None:
        r = 0.5 * 65535 if image.dtype == _U16 else 1.0  # skops.threshold_sauvola: half the dtype's range; floats (-1, 1)
    return m * (1 + k * ((s / r) - 1))


def _g_windows(lim, R):
    g, cases = "window thresholds", []
    wmax = R["window"]["hi"]
    for shape in ((7, 5), (66, 320)):
        for dt in ("u16", "f64"):
            for method in ("niblack", "sauvola"):
                for w in (1, wmax, (1, wmax), (wmax, 1)):
                    x = sw.img(dt, shape, 0)
                    if dt == "f64" and w == 1:
                        # the window is the sample itself and its deviation exactly 0; the oracle's integral images return
                        # the sample with a rounding error e and sqrt(e) ~ 1e-8 for the deviation, above the rule's 1e-7
                        # relative.  Multiples of 2^-10 keep every cumulative sum of the oracle exact (35 bits at most).
                        x = np.rint(x * 1024.0) / 1024.0
                    p = (dt, method, w)
                    marks = _mark(R, "window", 1 if w == 1 else wmax)
                    cases.append(Case(g, "window_threshold", f"{dt} {method} window {w}", shape,
                                      lambda ctx, x=x, p=p: (sw._window_dev(ctx, [ctx.asarray(x[None])], [x[None]], p)[0][0],),
                                      lambda x=x, p=p: ((x > window_ref(x, p[1], p[2])) if p[0] == "u16" else window_ref(x, p[1], p[2]),),
                                      rules=sw.exact if dt == "u16" else sw.close(1e-7, 1e-12), marks=marks))
    nl = R["window nlead"]
    lead6 = (1, 2, 1, 2, 2, 1)[:nl["hi"]]
    for lead, w in (((2,), 3), (lead6, 3), (lead6, (1, 3, 1, 3, 3, 1)[:len(lead6)] + (3, 5))):
        shape = tuple(lead) + (7, 5)
        vol = _rng(len(shape), 9).integers(0, 65536, shape).astype(_U16)
        # (a window of 3 on all eight axes has 256 corner terms on a 640,000-sample padded volume: one method there)
        for method in ("niblack", "sauvola") if isinstance(w, tuple) or len(lead) == 1 else ("niblack",):
            r = 32767.5 if method == "sauvola" else None
            cases.append(Case(g, "window_threshold nd", f"{method} window {w}", shape,
                              lambda ctx, vol=vol, w=w, method=method, r=r: sw._np(
                                  _h().window_threshold(ctx.asarray(vol), w, method, 0.2, r=r, nd=True)),
                              lambda vol=vol, w=w, method=method: (window_ref(vol, method, w),),
                              rules=sw.close(1e-9, 1e-9), marks=_mark(R, "window nlead", len(lead))))
    return cases


# ---- footprints -----------------------------------------------------------------------------------------------------
def footprints(lim, cells):
    """1 x 1, the longest column and row, a sparse asymmetric footprint of the largest side with exactly ``cells`` cells, the
    full 31 x 31 square, an L and one off-centre cell (a dilation that forgot to mirror the footprint moves the other way)."""
    side = lim["FOOTPRINT_SIDE"]
    sparse = np.zeros(side * side, _U8)
    sparse[_rng(side, cells).permutation(side * side)[:cells]] = 1
    ell = np.zeros((5, 5), _U8)
    ell[:, 0] = ell[4, :] = 1
    off = np.zeros((5, 5), _U8)
    off[0, 1] = 1
    return {"1 x 1": np.ones((1, 1), _U8), f"{side} x 1": np.ones((side, 1), _U8), f"1 x {side}": np.ones((1, side), _U8),
            f"sparse {side} x {side}, {cells} cells": sparse.reshape(side, side), "full 31 x 31": np.ones((31, 31), _U8),
            "L": ell, "one off-centre cell": off}


def _fp_marks(R, fp, cells_range):
    m = _mark(R, cells_range, int(np.count_nonzero(fp)))
    for s in set(fp.shape):
        m += _mark(R, "footprint side", s)
    return m


def specks(shape):
    """A few set pixels, one near each of two corners, one in the middle and a pair: a dilation stamps the mirrored footprint
    around each, and the erosion of the complement ("holes") cuts the footprint out, so neither result can be constant."""
    H, W = shape
    m = np.zeros(shape, bool)
    for y, x in ((5, 7), (H // 2, W // 2), (H - 6, W - 2), (40, 41), (40, 42)):
        m[y, x] = True
    return m


def _binary_mask(shape, kind):
    return sw.mask_of(shape, kind) if kind in (0, 2) else specks(shape) if kind == "specks" else ~specks(shape)


def _g_binary_footprints(lim, R):
    g, cases = "binary footprints", []
    for fn, fp in footprints(lim, lim["MAX_OFFS"]).items():
        for shape in ((7, 5), (33, 40), (66, 320)):
            for kind in (0, 2) + (("specks", "holes") if shape == (66, 320) else ()):
                x = _binary_mask(shape, kind)
                for op in ("erosion", "dilation", "opening", "closing"):
                    cases.append(Case(g, "binary_" + op, f"{fn} kind {kind}", shape,
                                      lambda ctx, x=x, fp=fp, op=op: (getattr(_h(), "binary_" + op)(ctx.asarray(x[None]), fp).numpy()[0],),
                                      lambda x=x, fp=fp, op=op: (getattr(skops, "binary_" + op)(x, fp),),
                                      marks=_fp_marks(R, fp, "binary footprint cells")))
    return cases


def grey_ref(fn, x, fp):
    """fn(x, fp) for the 'reflect' filters of scipy.  Where the footprint reaches four plane lengths or more beyond an edge,
    scipy's offset table for footprints with holes maps the sample at exactly -4 len (-6 len, ...) to index -1 and reads in
    front of the row (NI_InitFilterOffsets: the remainder 0 of the period goes through `-cc - 1`); there the plane is
    extended first by numpy's 'symmetric' padding, which is scipy's 'reflect', and the result cropped."""
    ry, rx = fp.shape[0] // 2, fp.shape[1] // 2
    if ry < 4 * x.shape[0] and rx < 4 * x.shape[1]:
        return fn(x, fp)
    out = fn(np.pad(x, ((ry, ry), (rx, rx)), mode="symmetric"), fp)
    return np.ascontiguousarray(out[ry:out.shape[0] - ry, rx:out.shape[1] - rx])


def _g_grey_footprints(lim, R):
    g, cases = "grey footprints", []
    refs = {"erosion": lambda x, fp: grey_ref(skops.erosion, x, fp), "dilation": lambda x, fp: grey_ref(skops.dilation, x, fp),
            "median": lambda x, fp: ndi.median_filter(x, footprint=fp, mode="nearest")}
    for fn, fp in footprints(lim, lim["RK_MAX_OFFS"]).items():
        for shape in ((7, 5), (33, 40), (66, 320)):
            for dt in ("u16", "f64"):
                x = sw.img(dt, shape, 0)
                for op in ("erosion", "dilation", "median"):
                    cases.append(Case(g, op, f"{dt} {fn}", shape,
                                      lambda ctx, x=x, fp=fp, op=op: (getattr(_h(), op)(ctx.asarray(x[None]), fp).numpy()[0],),
                                      lambda x=x, fp=fp, op=op: (refs[op](x, fp),), marks=_fp_marks(R, fp, "rank footprint cells")))
    return cases


def toc_footprints(lim):
    """{name: (footprint, role in the range)}: disk(4) / disk(5), flat rows with rx 16 / 17, and a 9 x 33 block with
    TOC_MAX_OFFS cells and one more -- the two sides of each term of `noffs <= TOC_MAX_OFFS && 4 ry <= 16 && 4 rx <= 64`."""
    ry, rx = lim["TOC_HALO"][0] // 4, lim["TOC_HALO"][1] // 4
    out = {f"disk({ry})": (skops.disk(ry), "ry at the fused halo"), f"disk({ry + 1})": (skops.disk(ry + 1), "ry beyond it"),
           f"flat rx {rx}": (np.ones((1, 2 * rx + 1), _U8), "rx at the fused halo"),
           f"flat rx {rx + 1}": (np.ones((1, 2 * rx + 3), _U8), "rx beyond it")}
    for cells, role in ((lim["TOC_MAX_OFFS"], "TOC_MAX_OFFS cells"), (lim["TOC_MAX_OFFS"] + 1, "TOC_MAX_OFFS + 1 cells")):
        # a solid block of full height, as many whole columns as the count allows, and the rest of the cells on the centre row
        # from both ends inwards: the box stays (2 ry + 1) x (2 rx + 1)
        fp = np.zeros((2 * ry + 1, 2 * rx + 1), _U8)
        cols = (cells - 2) // (2 * ry + 1)
        c0 = (2 * rx + 1 - cols) // 2
        fp[:, c0:c0 + cols] = 1
        free = sorted(set(range(2 * rx + 1)) - set(range(c0, c0 + cols)), key=lambda c: (min(c, 2 * rx - c), c))
        for c in free[:cells - int(fp.sum())]:
            fp[ry, c] = 1
        out[f"block of {cells} cells"] = (fp, role)
    return out


def _g_toc(lim, R):
    g, cases = "threshold_open_close", []
    for fn, (fp, role) in toc_footprints(lim).items():
        for shape in ((33, 40), (66, 320)):
            x, t = sw._toc_make(shape, 0, ("f64", 0))
            if fn.startswith("block"):  # nothing survives an opening by a block this large unless most of the plane is set
                t = np.asarray(np.quantile(x, 0.01), _F64)
            value = R["threshold_open_close footprint"]["switches"][role]
            cases.append(Case(g, "threshold_open_close", f"{fn}: {toc_path(lim, fp)}", shape,
                              lambda ctx, x=x, t=t, fp=fp: (_h().threshold_open_close(
                                  ctx.asarray(x[None]), ctx.asarray(np.array([t], _F64)), fp).numpy()[0],),
                              lambda x=x, t=t, fp=fp: (skops.binary_closing(skops.binary_opening(x > t, fp), fp),),
                              marks=[("threshold_open_close footprint", "switch " + role, value)]))
    return cases


# ---- peaks ----------------------------------------------------------------------------------------------------------
def _g_peaks(lim, R):
    g, cases = "peaks", []
    r = R["min_distance"]
    for shape in ((16, 16), (33, 40), (66, 320)):  # the first is cleared whole at min_distance 16
        for kind in (0, 2):
            d2, mask = sw._relief_make(shape, kind, None)
            for m in (r["lo"], r["hi"]):
                cases.append(Case(g, "peak_mask", f"min_distance {m} kind {kind}", shape,
                                  lambda ctx, d2=d2, mask=mask, m=m: (_h().peak_mask(
                                      ctx.asarray(d2[None]), ctx.asarray(mask[None]), m).numpy()[0],),
                                  lambda d2=d2, mask=mask, m=m: (sw._peaks_ref(d2, mask, m),), marks=_mark(R, "min_distance", m)))
                for conn in (1, 2):
                    cases.append(Case(g, "peak_markers", f"min_distance {m} c{conn} kind {kind}", shape,
                                      lambda ctx, d2=d2, mask=mask, m=m, conn=conn: tuple(
                                          a[0] for a in sw._np(*_h().peak_markers(ctx.asarray(d2[None]), ctx.asarray(mask[None]),
                                                                                  m, conn))),
                                      lambda d2=d2, mask=mask, m=m, conn=conn: sw._peak_markers_ref((d2, mask), (m, conn)),
                                      marks=_mark(R, "min_distance", m)))
    return cases


# ---- sides ----------------------------------------------------------------------------------------------------------
def side_shapes(lim):
    s = lim["SIDE_MAX"]
    return [(1, s), (s, 1), (2, s)]


def _side_masks(shape):
    """Zero pixels only at the two ends of the plane (first and last pixel), only at the first (the squared distance goes up
    to (side - 1)^2), and nowhere."""
    both = np.ones(shape, bool)
    both.flat[0] = both.flat[-1] = False
    one = np.ones(shape, bool)
    one.flat[0] = False
    return {"zeros at both ends": both, "a zero at one end": one, "no zero pixel": np.ones(shape, bool)}


def _expand_ref(lab, dist):
    """expand_two_pass, whose row pass steps through every dx in Python: a wide plane goes in transposed (the rule -- nearest
    labelled pixel, the smallest label among equally near ones -- has no preferred axis)."""
    if lab.shape[1] > lab.shape[0]:
        return np.ascontiguousarray(expand_ref.expand_two_pass(np.ascontiguousarray(lab.T), dist).T)
    return expand_ref.expand_two_pass(lab, dist)


def _g_sides(lim, R):
    g, cases = "sides", []
    for shape in side_shapes(lim):
        marks = _mark(R, "side", min(shape)) + _mark(R, "side", max(shape))
        for mn, mask in _side_masks(shape).items():
            cases.append(Case(g, "edt", mn, shape,
                              lambda ctx, mask=mask: tuple(a[0] for a in sw._np(*_h().edt(ctx.asarray(mask[None])))),
                              lambda mask=mask: sw._edt_ref((mask,), None), marks=marks))
        two = np.zeros(shape, _I32)
        two.flat[0], two.flat[-1] = 7, 3
        one = np.zeros(shape, _I32)
        one.flat[0] = 5
        for ln, lab, dist in (("labels at both ends", two, 3), ("labels at both ends", two, 40000.0), ("a label at one end", one, 40000.0),
                              ("a label at one end", one, 1000.5)):
            cases.append(Case(g, "expand_labels", f"{ln} d={dist:g}", shape,
                              lambda ctx, lab=lab, dist=dist: (_h().expand_labels(ctx.asarray(lab[None]), dist).numpy()[0],),
                              lambda lab=lab, dist=dist: (_expand_ref(lab, dist),), marks=marks))
    return cases


# ---- plane counts ---------------------------------------------------------------------------------------------------
def _g_planes(lim, R):
    g, n = "plane counts", lim["PLANES_MAX"]
    marks = _mark(R, "planes", n)
    p = ("u16", "f64", False)
    U = 61  # distinct planes, repeated to the count: the reference runs once per distinct plane

    def norm_in():
        xs = np.stack([sw.img_u16((2, 2), 0, 900 + u) for u in range(U)])
        lohi = np.stack([np.percentile(x.astype(_F32).astype(_F64), (1, 99)) for x in xs])
        idx = np.arange(n) % U
        return xs[idx], lohi[idx], xs, lohi

    def norm_dev(ctx):
        X, L, _, _ = _once(("planes", "norm"), norm_in)
        return sw._np(_h().normalize_planes(ctx.asarray(X), ctx.asarray(L), invert=False))

    def norm_ref():
        _, _, xs, lohi = _once(("planes", "norm"), norm_in)
        per = np.stack([sw._normalize_ref((xs[u], lohi[u]), p)[0] for u in range(U)])
        return (per[np.arange(n) % U],)

    def lab_in():
        r = _rng(2, 2, 5)
        labs = np.stack([np.where(r.random((2, 2)) < 0.45, r.integers(1, 5, (2, 2)), 0) for _ in range(U)]).astype(_I32)
        labs[0] = 0
        return labs[np.arange(n) % U], labs

    def exp_dev(ctx, dist):
        return sw._np(_h().expand_labels(ctx.asarray(_once(("planes", "lab"), lab_in)[0]), dist))

    def exp_ref(dist):
        labs = _once(("planes", "lab"), lab_in)[1]
        per = np.stack([expand_ref.expand_two_pass(labs[u], dist) for u in range(U)])
        return (per[np.arange(n) % U],)

    cases = [Case(g, "normalize_planes", f"{n} planes", (2, 2), norm_dev, norm_ref, rules=sw.same_bits, marks=marks)]
    for dist in (1, 1.5):
        cases.append(Case(g, "expand_labels", f"{n} planes d={dist:g}", (2, 2), lambda ctx, dist=dist: exp_dev(ctx, dist),
                          lambda dist=dist: exp_ref(dist), marks=marks))
    return cases


# ---- overlay --------------------------------------------------------------------------------------------------------
_COLORS = ("#00ff00", "#ff00ff", "#3366cc", "#ffaa00", "#00ffff", "#ff0000", "#8040c0", "#ffffff", "#123456")


def overlay_layers(n, modes):
    """(colour, opacity, zero_transparent, blend mode) of n layers; modes: "alpha", "additive" or "mixed"."""
    return tuple((_COLORS[i], (1.0, 0.6, 0.3, 0.85)[i % 4], i % 2 == 0,
                  modes if modes != "mixed" else ("alpha", "additive", "additive")[i % 3]) for i in range(n))


def _overlay_dev(ctx, planes, layers):
    import warnings

    from arcadia_microscopy_tools_amd import BlendMode, Channel, Layer, create_overlay

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # values outside [0, 1] are part of the case: clipped inside the kernel
        ls = [Layer(Channel(f"c{i}", color=c), ctx.asarray(x), o, z, BlendMode.ADDITIVE if m == "additive" else BlendMode.ALPHA)
              for i, ((c, o, z, m), x) in enumerate(zip(layers, planes[1:]))]
        return sw._np(create_overlay(ctx.asarray(planes[0]), ls))


def _g_overlay(lim, R):
    g, cases = "overlay", []
    r = R["overlay layers"]
    for shape in ((7, 5), (33, 40), (66, 320)):
        for n, modes in ((r["lo"], "alpha"), (r["hi"], "alpha"), (r["hi"], "additive"), (r["hi"], "mixed")):
            planes = tuple(sw.img_f64(shape, (0, 1, 2)[i % 3] if i else 0, 30 + i) * 1.2 - 0.1 for i in range(1 + n))
            layers = overlay_layers(n, modes)
            cases.append(Case(g, "overlay", f"{n} layers {modes}", shape,
                              lambda ctx, planes=planes, layers=layers: _overlay_dev(ctx, planes, layers),
                              lambda planes=planes, layers=layers: (oblend.create_overlay(
                                  planes[0], [(c, x, o, z, m) for (c, o, z, m), x in zip(layers, planes[1:])]),),
                              marks=_mark(R, "overlay layers", n)))
    return cases


# ---- channel groups -------------------------------------------------------------------------------------------------
_IPROPS = ["intensity_mean", "intensity_max", "intensity_min", "intensity_std"]


def _g_channels(lim, R):
    g, cases = "channel groups", []

    def props_dev(ctx, lab, stack):
        from arcadia_microscopy_tools_amd.masks import DEFAULT_CELL_PROPERTY_NAMES
        from arcadia_microscopy_tools_amd.segment import assemble_cell_properties

        k = int(lab.max())
        mt, it = _h().regionprops_full(ctx.asarray(lab[None]), ctx.asarray(stack[None]), max(k, 1))
        mt, it = mt.numpy()[0][:k], it.numpy()[0][:k]
        d = assemble_cell_properties(mt, it, [f"ch{c}" for c in range(stack.shape[0])], list(DEFAULT_CELL_PROPERTY_NAMES), _IPROPS)
        return ((list(d), [np.asarray(v) for v in d.values()]), np.concatenate([mt.ravel(), it.ravel()]))

    def props_ref(lab, stack):
        from arcadia_microscopy_tools_amd.masks import DEFAULT_CELL_PROPERTY_NAMES

        d = orp.cell_properties(lab.astype(np.int64), {f"ch{c}": stack[c] for c in range(stack.shape[0])},
                                list(DEFAULT_CELL_PROPERTY_NAMES), _IPROPS)
        return ((list(d), [np.asarray(v) for v in d.values()]), None)

    for shape in ((33, 40), (66, 320)):
        lab = sw.labels_of(shape, 0)
        for C in R["regionprops channels"]["switches"].values():
            stack = np.stack([sw.img_u16(shape, (0, 2)[c % 2], 60 + c) for c in range(C)])
            cases.append(Case(g, "regionprops_full", f"C {C}", shape,
                              lambda ctx, lab=lab, stack=stack: props_dev(ctx, lab, stack),
                              lambda lab=lab, stack=stack: props_ref(lab, stack), rules=(sw.props_rule, lambda got, want: (True, None)),
                              marks=_mark(R, "regionprops channels", C)))
        rc = R["colocalization channels"]
        for C, pairs in ((rc["lo"], None), (rc["switches"]["more than COLOC_MAXC"], "ordered")):
            pr = None if pairs is None else [(i, j) for i in range(C) for j in range(C) if i != j]
            for dt in ("u16", "f64"):
                st = np.stack([sw.img_u16(shape, (0, 2, 0)[c % 3], 80 + c) for c in range(C)])
                st = st if dt == "u16" else st.astype(_F64) / 65535.0
                thr = tuple((1000, 20000.0, 40000.25, 0, 65534, 5.5)[c] * (1 if dt == "u16" else 1 / 65535.0) for c in range(C))
                K = max(int(lab.max()), 1)
                cases.append(Case(g, "colocalization", f"{dt} C {C} pairs {'default' if pr is None else len(pr)}", shape,
                                  lambda ctx, lab=lab, st=st, thr=thr, pr=pr, K=K: (_h().colocalization(
                                      ctx.asarray(lab[None]), ctx.asarray(st[None]), K, thresholds=thr,
                                      pairs=pr).numpy()[0][:int(lab.max())],),
                                  lambda lab=lab, st=st, thr=thr, pr=pr: (
                                      coloc_ref.table(lab.astype(np.int64), st, int(lab.max()), thr, pr),),
                                  rules=sw._coloc_rule(dt), marks=_mark(R, "colocalization channels", C)))
    return cases


# ---- amt_nn_affine_act_bf16 against its definition ------------------------------------------------------------------
def bf16_round(v):
    """The bf16 value nearest to each float64 of ``v``, ties to the even 8-bit significand (normal range): v = m 2^e with
    0.5 <= |m| < 1, the significand m 2^8 rounded by np.rint (half to even)."""
    m, e = np.frexp(np.asarray(v, _F64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def bf16_neighbours(v):
    """(the largest bf16 <= v, the smallest bf16 >= v) as float64."""
    m, e = np.frexp(np.asarray(v, _F64))
    return np.ldexp(np.floor(m * 256.0), e - 8), np.ldexp(np.ceil(m * 256.0), e - 8)


def bf16_bits(v):
    """The 16 bits of values that ARE bf16 numbers."""
    f = np.asarray(v, _F64).astype(_F32)
    assert np.array_equal(f.astype(_F64), np.asarray(v, _F64)) and not (f.view(_U32) & 0xFFFF).any(), "not bf16 values"
    return (f.view(_U32) >> 16).astype(_U16)


def bf16_values(bits):
    return (np.asarray(bits, _U16).astype(_U32) << 16).view(_F32).astype(_F64)


def affine_configs(lim):
    """(name, N, H, W, C, upsample, relu, absent pointers, marks-values): H, W are the OUTPUT sides."""
    out = []
    for C in (8, 24, 64):
        for ups in (0, 1):
            for relu in (0, 1):
                out.append((f"C {C} upsample {ups} relu {relu}", 2, 6, 10, C, ups, relu, ()))
    for ups in (0, 1):
        for absent in (("y",), ("style",), ("pre_bias",), ("sum_out",), ("y", "style", "pre_bias", "sum_out")):
            out.append((f"C 24 upsample {ups} relu 1 without {' '.join(absent)}", 2, 6, 10, 24, ups, 1, absent))
    rows = lim["NN_ROWS_PER_LAUNCH"] + 1
    out.append((f"{rows} rows: the second launch", 2, rows // 2, 2, 8, 0, 1, ()))
    groups = 2 * 256 * lim["NN_MAX_BLOCKS_X"]
    out.append((f"{groups} groups per row: the grid-stride loop", 1, 2, groups // 32, 256, 1, 1, ()))
    return out


def affine_inputs(name, N, H, W, C, ups, exact=True):
    """Host arrays in NHWC order (channels-last), float32.  exact: multiples of 1/8 within +-16 for x, y, pre_bias and style,
    scale in {0.5, 1, 2, -1}, shift a multiple of 1/8: every float32 step of the kernel is then exact (all partial results
    are multiples of 1/16 below 2^8, twelve bits at most), contracted or not, and only the final rounding to bf16 is left."""
    def make():
        r = _rng(N, H, W, C, ups, len(name), int(exact))
        h, w = (H // 2, W // 2) if ups else (H, W)
        if exact:
            d = lambda shape: (r.integers(-128, 129, shape) / 8.0).astype(_F32)  # noqa: E731
            return dict(x=d((N, h, w, C)), y=d((N, H, W, C)), style=d((N, C)), pre_bias=d((C,)),
                        scale=r.choice(np.array([0.5, 1.0, 2.0, -1.0], _F32), C), shift=(r.integers(-64, 65, C) / 8.0).astype(_F32))
        # random values, every term of a channel's result of ONE sign (positive sums, scale and shift of a common sign per
        # channel): |V| is then the sum of the terms' magnitudes and nothing cancels -- see affine_random_rule
        pos = lambda shape: r.uniform(0.25, 2.0, shape)  # noqa: E731
        bf = lambda a: bf16_round(a).astype(_F32)  # noqa: E731
        sign = r.choice([-1.0, 1.0], C)
        return dict(x=bf(pos((N, h, w, C))), y=bf(pos((N, H, W, C))), style=pos((N, C)).astype(_F32), pre_bias=pos((C,)).astype(_F32),
                    scale=(pos((C,)) * sign).astype(_F32), shift=(pos((C,)) * sign).astype(_F32))
    return _once(("affine", name, N, H, W, C, ups, exact), make)


def affine_definition(ins, ups, relu, absent):
    """(x + y + pre_bias, the value before its rounding to bf16, sum of the magnitudes of the terms) in float64."""
    x = ins["x"].astype(_F64)
    if ups:
        x = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    y = 0.0 if "y" in absent else ins["y"].astype(_F64)
    pre = 0.0 if "pre_bias" in absent else ins["pre_bias"].astype(_F64)[None, None, None, :]
    st = 0.0 if "style" in absent else ins["style"].astype(_F64)[:, None, None, :]
    sc, sh = ins["scale"].astype(_F64), ins["shift"].astype(_F64)
    s = x + y + pre
    v = (s + st) * sc + sh
    mag_s = np.abs(x) + np.abs(y) + np.abs(pre)
    mag_v = (mag_s + np.abs(st)) * np.abs(sc) + np.abs(sh)
    return s, (np.maximum(v, 0.0) if relu else v), mag_s, mag_v


def affine_call(ctx, ins, N, H, W, C, ups, relu, absent=(), offset=None):
    """The kernel on torch tensors (bf16 activations channels-last, float32 vectors) -> (out bits, sum_out bits or None)."""
    import torch

    from arcadia_microscopy_tools_amd import _hip

    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in ins.items()}
    x, y = t["x"].to(torch.bfloat16).contiguous(), t["y"].to(torch.bfloat16).contiguous()
    out = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=dev)
    ssum = None if "sum_out" in absent else torch.empty_like(out)
    ptr = lambda k, v: None if k in absent else v.data_ptr() + (offset or {}).get(k, 0)  # noqa: E731
    torch.cuda.synchronize()  # the inputs are complete before the library's stream reads them
    _hip.check(_hip.load_library().amt_nn_affine_act_bf16(
        ctx.handle, ptr("x", x), ptr("y", y), ptr("style", t["style"]), ptr("pre_bias", t["pre_bias"]), t["scale"].data_ptr(),
        t["shift"].data_ptr(), out.data_ptr(), None if ssum is None else ssum.data_ptr(), N, H, W, C, relu, ups),
        "amt_nn_affine_act_bf16")
    ctx.synchronize()
    bits = lambda a: a.view(torch.int16).cpu().numpy().view(_U16)  # noqa: E731
    return bits(out), (np.zeros(0, _U16) if ssum is None else bits(ssum))


# The random-valued case.  The kernel evaluates r = fl(fl(fl(fl(fl(x + y) + pre) + style) * scale) + shift) in float32: five
# roundings, each of relative size u = 2^-24 at most.  Every term's path to r passes through at most five of them (x and y
# through all five, shift through one), so r = sum of the terms times (1 + theta) with |theta| <= gamma_5 = 5u / (1 - 5u)
# (Higham, Accuracy and Stability, lemma 3.1), and |r - V| <= gamma_5 * ((|x| + |y| + |pre| + |style|) |scale| + |shift|) for
# the exact value V; a contracted multiply-add only removes a rounding.  x + y + pre_bias passes through two: gamma_2.  The
# kernel then rounds r to bf16 ONCE, to nearest even.  Hence: the output is one of the two bf16 neighbours of V, and it is
# the one nearest to V unless V lies within that bound of the midpoint between them.  The first half needs the bound to stay
# below half the spacing of the bf16 numbers at V, 2^-9 |V| at least: |V| > 2^9 gamma_5 (sum of the magnitudes), 1.6e-4 of it.
# Where the terms cancel further than that, a float32 chain is entitled to miss V by several bf16 steps, so the case's inputs
# keep every term of a result on one side of zero (affine_inputs); the exact cases carry the mixed signs.
_U24 = 2.0 ** -24


def affine_random_rule(got_bits, want):
    v, mag, roundings = want
    got = bf16_values(got_bits)
    if got.shape != v.shape:
        return False, ("shape", got.shape, v.shape)
    bound = roundings * _U24 / (1 - roundings * _U24) * mag
    lo, hi = bf16_neighbours(v)
    bad = (got != lo) & (got != hi)
    bad |= (got != bf16_round(v)) & (np.abs(v - (lo + hi) / 2) > bound)
    if bad.any():
        return False, tuple(int(i) for i in np.argwhere(bad)[0])
    return True, None


def _g_affine(lim, R):
    g, cases = "affine bf16", []
    for name, N, H, W, C, ups, relu, absent in affine_configs(lim):
        def run(ctx, a=(name, N, H, W, C, ups, relu, absent)):
            name, N, H, W, C, ups, relu, absent = a
            return affine_call(ctx, affine_inputs(name, N, H, W, C, ups), N, H, W, C, ups, relu, absent)

        def want(a=(name, N, H, W, C, ups, relu, absent)):
            name, N, H, W, C, ups, relu, absent = a
            s, v, _, _ = affine_definition(affine_inputs(name, N, H, W, C, ups), ups, relu, absent)
            return bf16_bits(bf16_round(v)), (np.zeros(0, _U16) if "sum_out" in absent else bf16_bits(bf16_round(s)))

        marks = _mark(R, "affine channels", C) + _mark(R, "affine rows", N * H) + _mark(R, "affine groups per row", W * C // 8)
        cases.append(Case(g, "nn_affine_act exact", name, (N, H, W, C), run, want, marks=marks))
    N, H, W, C, ups = 2, 16, 24, 64, 1

    def rrun(ctx):
        return affine_call(ctx, affine_inputs("random", N, H, W, C, ups, exact=False), N, H, W, C, ups, 0)

    def rwant():
        s, v, mag_s, mag_v = affine_definition(affine_inputs("random", N, H, W, C, ups, exact=False), ups, 0, ())
        return (v, mag_v, 5), (s, mag_s, 2)

    cases.append(Case(g, "nn_affine_act random", "C 64 upsample 1 relu 0", (N, H, W, C), rrun, rwant, rules=affine_random_rule,
                      marks=_mark(R, "affine channels", C)))
    return cases


# ---- one step beyond each end: a refusal, never a launch ------------------------------------------------------------
def _g_refusals(lim, R):
    g, cases = "refusals", []
    f64 = sw.img_f64((7, 5), 0)
    u16 = sw.img_u16((7, 5), 0)
    msk = sw.mask_of((7, 5), 0)

    def add(op, name, rng_name, role, run, source, expect=(ValueError,), shape=(7, 5)):
        cases.append(Case(g, op, name, shape, run, None, marks=[(rng_name, "refuse " + role, R[rng_name]["refuse"][role])],
                          expect=expect, source=source))

    st = "amt_stats.hip"
    hb, ob = R["hist_f64 nbins"], R["otsu_f64 nbins"]
    for role in ("lo", "hi"):
        nb = hb["refuse"][role]
        add("histogram_f64", f"nbins {nb}", "hist_f64 nbins", role,
            lambda ctx, nb=nb: _h().histogram_f64(ctx.asarray(f64[None]), nb),
            ((st, "amt_hist_f64", f"nbins >= {hb['lo']} && nbins <= {hb['hi']}"),))
        nb = ob["refuse"][role]
        add("threshold_otsu", f"nbins {nb}", "otsu_f64 nbins", role,
            lambda ctx, nb=nb: _h().threshold_otsu(ctx.asarray(f64[None]), nbins=nb),
            ((st, "amt_threshold_value", f"nbins >= {ob['lo']} && nbins <= {ob['hi']}"),))
        nb = R["hist_range nbins"]["refuse"][role]
        frag = "nbins >= 1" if role == "lo" else f"nbins <= (1ll << {lim['HIST_RANGE_LOG2']})"

        def hist_range(ctx, nb=nb):
            try:
                return _h().histogram_range(ctx.asarray(f64[None]), 0, nb)
            finally:
                ctx.trim()
        add("histogram_range", f"nbins {nb}", "hist_range nbins", role, hist_range, ((st, "amt_hist_range_f64", frag),))
        for dt, x, rn, fn in (("f64", f64, "percentile_f64 nq", "amt_percentile_f64"),
                              ("u16", u16, "percentile_u16 nq", "amt_percentile_u16")):
            nq = R[rn]["refuse"][role]
            q = list(np.linspace(0, 100, nq))
            add("percentile " + dt, f"nq {nq}", rn, role, lambda ctx, x=x, q=q: _h().percentile(ctx.asarray(x[None]), q),
                ((st, fn, f"nq >= {R[rn]['lo']} && nq <= {R[rn]['hi']}"),))
        m = R["min_distance"]["refuse"][role]
        d2 = np.ones((7, 5), _I32)
        frag = "min_distance >= 0 && min_distance <= PK_MAXM"
        add("peak_mask", f"min_distance {m}", "min_distance", role,
            lambda ctx, m=m: _h().peak_mask(ctx.asarray(d2[None]), ctx.asarray(msk[None]), m), (("amt_edt.hip", "amt_peak_mask", frag),))
        add("peak_markers", f"min_distance {m}", "min_distance", role,
            lambda ctx, m=m: _h().peak_markers(ctx.asarray(d2[None]), ctx.asarray(msk[None]), m, 1),
            (("amt_edt.hip", "amt_peak_markers", frag),))
    gr = R["gaussian radius"]
    sigma = (gr["refuse"]["hi"] - 0.2) / 4.0  # 32.2 -> int(4 sigma + 0.5) = 129
    add("gaussian", f"sigma {sigma:g}", "gaussian radius", "hi", lambda ctx: _h().gaussian(ctx.asarray(f64[None]), sigma),
        (("amt_filters.hip", "amt_gaussian", "check_gauss_args("),
         ("amt_filters.hip", "check_gauss_args", f"r >= {gr['lo']} && r <= {gr['hi']}")))
    w = R["window"]
    for role, fragment in (("hi", f"window_y <= {w['hi']} && window_x <= {w['hi']}"), ("even", "window_y >= 1 && (window_y & 1)")):
        ws = w["refuse"][role]
        add("window_threshold", f"window {ws}", "window", role,
            lambda ctx, ws=ws: _h().window_threshold(ctx.asarray(u16[None]), ws),
            (("amt_window.hip", "amt_window_threshold", fragment),))
    nl = R["window nlead"]["refuse"]["hi"]
    vol = np.zeros((1,) * nl + (3, 3), _U16)
    add("window_threshold nd", f"{nl} leading axes", "window nlead", "hi",
        lambda ctx: _h().window_threshold(ctx.asarray(vol), 3, nd=True),
        (("amt_window.hip", "amt_window_threshold_nd", f"nlead >= 0 && nlead <= {R['window nlead']['hi']}"),), shape=vol.shape)
    side = R["footprint side"]
    big = np.ones((side["refuse"]["hi"],) * 2, _U8)
    sfrag = f"fh <= {side['hi']} && fw <= {side['hi']}"
    morph = (("amt_morph.hip", "amt_binary_morph", "build_offsets("), ("amt_morph.hip", "build_offsets", sfrag))
    rank = (("amt_rank.hip", "amt_rank_filter", "rank_filter_impl("), ("amt_rank.hip", "rank_filter_impl", sfrag))
    add("binary_erosion", f"{big.shape[0]} x {big.shape[1]} footprint", "footprint side", "hi",
        lambda ctx: _h().binary_erosion(ctx.asarray(msk[None]), big), morph)
    add("erosion", f"{big.shape[0]} x {big.shape[1]} footprint", "footprint side", "hi",
        lambda ctx: _h().erosion(ctx.asarray(u16[None]), big), rank)
    for op, rn, x, source in (
            ("binary_dilation", "binary footprint cells", msk, morph[:1] + (("amt_morph.hip", "build_offsets", "k < MAX_OFFS"),)),
            ("median", "rank footprint cells", u16, rank[:1] + (("amt_rank.hip", "rank_filter_impl", "noffs < RK_MAX_OFFS"),))):
        cells = R[rn]["refuse"]["hi"]
        fp = np.zeros(side["hi"] ** 2, _U8)
        fp[:cells] = 1
        fp = fp.reshape(side["hi"], side["hi"])
        add(op, f"{cells} cells", rn, "hi",
            lambda ctx, op=op, x=x, fp=fp: getattr(_h(), op)(ctx.asarray(x[None]), fp), source)
    s = R["side"]["refuse"]["hi"]
    sfrag = f"H <= {R['side']['hi']} && W <= {R['side']['hi']}"
    add("edt", f"a side of {s}", "side", "hi", lambda ctx: _h().edt(ctx.asarray(np.ones((1, 1, s), bool))),
        (("amt_edt.hip", "amt_edt", sfrag),), shape=(1, s))
    add("expand_labels", f"a side of {s}", "side", "hi",
        lambda ctx: _h().expand_labels(ctx.asarray(np.ones((1, s, 1), _I32)), 1.0),
        (("amt_expand.hip", "amt_expand_labels", sfrag),), shape=(s, 1))
    n = R["planes"]["refuse"]["hi"]
    pfrag = f"nplanes <= {R['planes']['hi']}"
    add("normalize_planes", f"{n} planes", "planes", "hi",
        lambda ctx: _h().normalize_planes(ctx.asarray(np.ones((n, 1, 1), _U16)), ctx.asarray(np.tile(np.array([0.0, 1.0]), (n, 1)))),
        (("amt_normalize.hip", "amt_normalize_planes_f32", pfrag),), shape=(1, 1))
    add("expand_labels", f"{n} planes", "planes", "hi",
        lambda ctx: _h().expand_labels(ctx.asarray(np.ones((n, 1, 1), _I32)), 1.0),
        (("amt_expand.hip", "amt_expand_labels", pfrag),), shape=(1, 1))
    nlay = R["overlay layers"]["refuse"]["hi"]
    planes = tuple(sw.img_f64((7, 5), 0, 30 + i) for i in range(1 + nlay))
    add("overlay", f"{nlay} layers", "overlay layers", "hi",
        lambda ctx: _overlay_dev(ctx, planes, overlay_layers(nlay, "alpha")),
        (("amt_overlay.hip", "amt_overlay", "nlayers >= 0 && nlayers <= OV_MAX_LAYERS"),), expect=(NotImplementedError, ValueError))
    # amt_nn_affine_act_bf16: C = 12, an odd side with upsampling, a pointer off its 16-byte alignment
    nn = "amt_nn.hip"
    ins = lambda C: affine_inputs("refusal", 1, 8, 8, C, 0)  # noqa: E731  (buffers larger than what any of the calls names)
    add("nn_affine_act", "C 12", "affine channels", "not a multiple of 8",
        lambda ctx: affine_call(ctx, ins(16), 1, 8, 8, 12, 0, 1),
        ((nn, "amt_nn_affine_act_bf16", "C % 8 == 0"),), shape=(1, 8, 8, 12))
    cases.append(Case(g, "nn_affine_act", "odd H with upsample", (1, 3, 4, 16),
                      lambda ctx: affine_call(ctx, ins(16), 1, 3, 4, 16, 1, 1),
                      expect=(ValueError,), source=((nn, "amt_nn_affine_act_bf16", "!upsample || (H % 2 == 0 && W % 2 == 0)"),)))
    cases.append(Case(g, "nn_affine_act", "x offset by 8 bytes", (1, 4, 4, 16),
                      lambda ctx: affine_call(ctx, ins(16), 1, 4, 4, 16, 0, 1, offset={"x": 8}),
                      expect=(ValueError,), source=((nn, "amt_nn_affine_act_bf16", "& 15) == 0"),)))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
# (range, role) pairs the table does not reach, each with its reason: none
EXCLUDED: dict = {}

_BUILDERS = {"histograms and thresholds f64": _g_hist_f64, "histogram_range": _g_hist_range, "percentiles": _g_percentiles,
             "gaussian": _g_gaussian, "window thresholds": _g_windows, "binary footprints": _g_binary_footprints,
             "grey footprints": _g_grey_footprints, "threshold_open_close": _g_toc, "peaks": _g_peaks, "sides": _g_sides,
             "plane counts": _g_planes, "overlay": _g_overlay, "channel groups": _g_channels, "affine bf16": _g_affine,
             "refusals": _g_refusals}
_TABLE: dict = {}


def _regime_groups(lim):
    return {f"hist_u16 {n} x {s}": (n, s, role) for n, s, role in hist_regimes(lim)}


def groups():
    lim = _limits()
    names = list(_BUILDERS)
    at = names.index("gaussian")
    return names[:at] + list(_regime_groups(lim)) + names[at:]


def _limits():
    if "lim" not in _TABLE:
        _TABLE["lim"] = limits()
        _TABLE["ranges"] = ranges(_TABLE["lim"])
    return _TABLE["lim"]


def table(group):
    """The cases of one group (built once)."""
    lim = _limits()
    if group not in _TABLE:
        R = _TABLE["ranges"]
        _TABLE[group] = _BUILDERS[group](lim, R) if group in _BUILDERS else _g_hist_regime(lim, R, *_regime_groups(lim)[group])
        keys = [c.key() for c in _TABLE[group]]
        assert len(set(keys)) == len(keys), f"{group}: two cases share a key"
    return _TABLE[group]


GROUPS = groups()


def wanted_marks(lim=None):
    """Every (range, role, value) the table has to carry: both ends, each switch, one refusal per side that has one."""
    out = []
    for name, r in ranges(lim).items():
        out += [(name, role, r[role]) for role in ("lo", "hi") if r[role] is not None]
        out += [(name, "switch " + role, v) for role, v in r["switches"].items()]
        out += [(name, "refuse " + role, v) for role, v in r["refuse"].items()]
    return [m for m in out if m[:2] not in EXCLUDED]


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
def compare(case, outs, wants):
    rules = case.rules if isinstance(case.rules, tuple) else (case.rules,) * len(wants)
    if len(outs) != len(wants):
        return False, ("outputs", len(outs), len(wants))
    for k, (rule, g, w) in enumerate(zip(rules, outs, wants)):
        ok, idx = rule(g, w)
        if not ok:
            return False, (k, idx)
    return True, None


def reference(case):
    """The expected outputs of one case: computed once and shared, read-only (the large ones of the histogram regimes are
    made per run and dropped with their inputs)."""
    if case.group.startswith("hist_u16"):
        return case.want()
    return _once(("ref",) + case.key(), case.want)


def _digest(outs):
    return sw._digest([o if isinstance(o, np.ndarray) else (np.asarray(o) if np.isscalar(o) else o) for o in outs])


def _run_case(ctx, case):
    t = time.perf_counter()
    record = {"group": case.group, "op": case.op, "param": case.name, "shape": list(case.shape), "variant": "single",
              "status": "pass", "index": None, "marks": [list(m) for m in case.marks]}
    if case.expect is not None:
        try:
            case.run(ctx)
            record.update(status="mismatch", index="the call was not refused", sha256=_digest([]))
        except case.expect as e:
            record["sha256"] = _digest([np.frombuffer(type(e).__name__.encode(), _U8)])
    else:
        outs = case.run(ctx)
        record["sha256"] = _digest(outs)
        ok, idx = compare(case, outs, reference(case))
        if not ok:
            record.update(status="mismatch", index=repr(idx))
    record["ms"] = round((time.perf_counter() - t) * 1e3, 1)  # call, copies and reference
    return record


def run(ctx, groups=None, scratch_check=False):
    """The cases of the groups (default: all): {"records", "called", "dirty", "seconds"}.  A mismatch is recorded and the run
    goes on; an exception from the library that is not an expected refusal ends it at once."""
    records = []
    t0 = time.perf_counter()
    with sw.Recorder(ctx, scratch_check) as rec:
        for group in (GROUPS if groups is None else groups):
            for case in table(group):
                rec.where = [case.op, case.name, list(case.shape), "single"]
                records.append(_run_case(ctx, case))
            if group.startswith("hist_u16"):
                forget("regime")
                ctx.trim()
    return {"records": records, "called": sorted(rec.called), "dirty": rec.dirty, "seconds": time.perf_counter() - t0}


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", required=True, help="where to write the records, the scratch findings and the entry points")
    ap.add_argument("--group", action="append", help="only this group (repeatable)")
    ap.add_argument("--profile", help="also write the run's time, its cases per group, the limits and the entry points reached here")
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison = poison_child.poisoned()
    res = run(get_context(), args.group, scratch_check=poison)
    poison_child.write(args.json, res)
    bad = [r for r in res["records"] if r["status"] != "pass"]
    if args.profile:
        per = {g: round(sum(r["ms"] for r in res["records"] if r["group"] == g) / 1e3, 2) for g in GROUPS}
        with open(args.profile, "w") as f:
            json.dump({"device": get_context().device_name(), "poison": poison, "seconds": round(res["seconds"], 2),
                       "cases": len(res["records"]), "mismatches": len(bad),
                       "cases_per_group": {g: sum(r["group"] == g for r in res["records"]) for g in GROUPS},
                       "seconds_per_group": per, "limits": limits(), "entry_points": res["called"]}, f, indent=1)
            f.write("\n")
    for r in bad[:20]:
        print("MISMATCH", r["group"], r["op"], r["param"], r["shape"], r["index"], flush=True)
    for d in res["dirty"][:20]:
        print("DIRTY SCRATCH", d, flush=True)
    print(f"{len(res['records'])} cases, {len(bad)} mismatches, {len(res['dirty'])} dirty scratch checks, "
          f"{res['seconds']:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
