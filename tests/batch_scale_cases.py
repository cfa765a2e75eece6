"""Every batched operator on the far side of its WORK-SIZE switches: the host model of the dispatch, the table and the runner.

tests/operator_sweep.py moves the shape, tests/worstcase_content.py the content and tests/parameter_limits.py the
parameters; none of them sends more than five planes.  Several host drivers pick a kernel variant, a tile height or the
blocks per plane from the total work of the call -- ``nplanes`` times tiles against the chip's compute units -- so those
suites only ever see the "too few tiles to fill the chip" side.  This table reaches the other side with planes of a few
thousand pixels by raising ``nplanes``:

  gaussian tile height   the TH loop of launch_fused (gauss_lds_kernel and gauss_fused_kernel) and of launch_codes
  edt tile variant       edt_bits_kernel<64, 16> against <32, 24>
  percentile             want / gparts of amt_percentile_f64's classify pass
  label-count loops      a second trip of the amt_grid_for(nlab, 256, 1024) loops of amt_props.hip
  many planes            every operator of the sweep, skeletonize, reconstruction and h_maxima at 130 planes: the 64-thread
                         bookkeeping kernels beyond block 0, the per-plane counters and round masks beyond plane 63

``limits()`` reads the constants and the rule text of every switch from the .hip sources by pattern; the model functions
(``gaussian_variant``, ``edt_variant``, ``percentile_parts``, ``label_trips``) restate the rules and ``first_far`` derives
the first batch size on the far side of a switch (B*) for a given number of compute units.  A retune changes what they
return, and tests/test_host_batch_scale.py then says which case no longer straddles its switch.

A batch is laid out from a few distinct planes (``layout``): the sweep's kinds 0, 1 and 2 under two seeds -- kind 1 is
constant by definition, so its two copies hold the same values -- plus the extra planes a group names, in a fixed, seeded,
aperiodic order in which every distinct plane sits at least once below index 64 and at least once at or above it
(batches of fewer than 64 + that many planes, which only the percentile group has, cannot and do not).  Every distinct
plane's reference is computed once; EVERY plane of the batch is compared with the reference of the plane it holds, by the
rule tests/operator_sweep.py has for the operator.  No tolerance of its own.

``run(ctx, groups, scratch_check)`` returns one record per call in the form of tests/operator_sweep.py, each with the
variant the model says the call took.  ``python -m tests.batch_scale_cases --json PATH [--profile PATH]`` runs everything.
Not collected by pytest (tests/test_host_batch_scale.py and tests/test_gpu_batch_scale.py are)."""
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

import operator_sweep as sw  # noqa: E402
import parameter_limits as pl  # noqa: E402
import poison_child  # noqa: E402
import reconstruction_reference as rr  # noqa: E402
import skeleton_reference as skref  # noqa: E402
from oracle import skops  # noqa: E402

_F64, _U16, _U8 = np.float64, np.uint16, np.uint8
MEMORY_CAP = 512 * 1024 * 1024  # bytes of the largest operand of any call of the table
CU_COUNTS = (256, 304)  # the chips the host test checks the table for
MANY = 130  # planes of the bookkeeping groups: 130, 260 and 130 * nq cross the 64- and 128-thread seams


# ---------------------------------------------------------------------------------------------------------------------
# the switches, read from the sources
# ---------------------------------------------------------------------------------------------------------------------
def limits():
    """The constants and the text of every work-size rule, by pattern."""
    src = pl.sources()
    fl, ed, st, pr, cm = (src[f] for f in ("amt_filters.hip", "amt_edt.hip", "amt_stats.hip", "amt_props.hip", "amt_common.h"))

    def const(text, name):
        m = re.search(r"constexpr (?:int|size_t|uint32_t) " + name + r" = (\d+);", text)
        assert m, f"{name} not found"
        return int(m.group(1))

    out = {"FR_MAX": const(fl, "FR_MAX"), "PFX_CAP": const(fl, "PFX_CAP"), "PFX_CNT_STRIDE": const(fl, "PFX_CNT_STRIDE"),
           "PKM_CNT_STRIDE": const(ed, "PKM_CNT_STRIDE"), "PQ_VPT": const(st, "PQ_VPT"), "PQ_MIN_N": const(st, "PQ_MIN_N")}
    # the TH loop: (start, floor, blocks per CU) of each of its three copies
    loop = (r"int (TH2?) = (\d+);\n\s*while \(\1 > (\d+) && \(long long\)(gx2?) \* \(\(H \+ \1 - 1\) / \1\) \* nplanes < "
            r"(\d+)LL \* ctx->num_cus\) \1 >>= 1;")
    fused, codes = pl.function_body(fl, "launch_fused"), pl.function_body(fl, "launch_codes")
    found = {"lds": re.findall(loop, fused[:fused.index("constexpr int OUTW = ")]),
             "fused": re.findall(loop, fused[fused.index("constexpr int OUTW = "):]), "codes": re.findall(loop, codes)}
    for name, ms in found.items():
        assert len(ms) == 1, f"the TH loop of {name}: found {len(ms)} times"
        th, start, floor, gx, per_cu = ms[0]
        assert (th, gx) == (("TH", "gx") if name == "fused" else ("TH2", "gx2")), (name, th, gx)
        out["TH_" + name] = (int(start), int(floor), int(per_cu))
    m = re.search(r"constexpr int OUTW = (\d+) - 2 \* R;\n\s*const int gx = \(W \+ OUTW - 1\) / OUTW;", fused)
    assert m, "gauss_fused_kernel's tile width"
    out["OUTW"] = int(m.group(1))
    for body in (fused, codes):
        m = re.search(r"constexpr int RP = \(R \+ 7\) & ~7;\n\s*constexpr int OUTW2 = (\d+) - 2 \* RP;\n\s*"
                      r"const int gx2 = \(W \+ OUTW2 - 1\) / OUTW2;", body)
        assert m and int(m.group(1)) == out["OUTW"], "gauss_lds_kernel's tile width"
    # what TH decides inside the kernels: the row map's length and the last partial row group
    assert "for (int k = t; k < TH + 2 * R + 4; k += 256) ymap[k] = amt_map_index(y0 - R + k, H, mode);" in fl
    assert "for (int k = t; k < TH + 2 * R + 8; k += 256) ymap[k] = amt_map_index(y0 - R + k, H, mode);" in fl
    assert "const bool aligned = (W % 8 == 0) && W >= 256 && (in_stride % 8 == 0)" in fl and "if (aligned && modeok && H > 2 * R) {" in fl
    # the EDT tile rule
    assert "const size_t tiles64 = (size_t)((W + 63) / 64) * ((H + 63) / 64) * nplanes;" in ed
    m = re.search(r"if \(tiles64 >= (\d+) && !edt_out\)[^\n]*\n\s*hipLaunchKernelGGL\(\(edt_bits_kernel<(\d+), (\d+)>\), "
                  r"dim3\(WW, \(H \+ \d+\) / \2, nplanes\)[^;]*;\n\s*else\n\s*hipLaunchKernelGGL\(\(edt_bits_kernel<(\d+), (\d+)>\), "
                  r"dim3\(WW, \(H \+ \d+\) / \4, nplanes\)", ed)
    assert m, "the EDT tile rule"
    out["EDT_TILES"] = int(m.group(1))
    out["EDT_FAR"], out["EDT_NEAR"] = (int(m.group(2)), int(m.group(3))), (int(m.group(4)), int(m.group(5)))
    # the classify pass of amt_percentile_f64
    m = re.search(r"int want = (\d+) / nplanes;\n\s*want = want < (\d+) \? \2 : \(want > (\d+) \? \3 : want\);\n\s*"
                  r"const unsigned gparts = amt_grid_for\(n, 256 \* PQ_VPT, \(unsigned\)want\);", st)
    assert m, "want / gparts of amt_percentile_f64"
    out["PQ_WANT"] = tuple(int(v) for v in m.groups())
    assert "if (n < PQ_MIN_N) return percentile_f64_radix(" in st
    # the label-count loops
    ms = re.findall(r"hipLaunchKernelGGL\((\w+), dim3\(amt_grid_for\(nlab, (\d+), (\d+)\)\), dim3\(\2\)", pr)
    assert sorted(m[0] for m in ms) == ["rp_final_kernel", "rp_init_kernel", "rpx_centroid_kernel", "rpx_moments_kernel"], ms
    assert len({m[1:] for m in ms}) == 1, ms
    out["NLAB_GRID"] = (int(ms[0][1]), int(ms[0][2]))
    assert pr.count("i < nlab; i += (size_t)gridDim.x * %d) {" % out["NLAB_GRID"][0]) == 4
    assert "const size_t nlab = (size_t)nplanes * max_label;" in pr
    assert ("size_t b = (work_items + block - 1) / block;\n    if (b < 1) b = 1;\n    if (b > max_blocks) b = max_blocks;"
            in cm), "amt_grid_for"
    # the per-plane bookkeeping kernels of 64 threads, by what their grid counts
    book = {}
    for f in ("amt_stats.hip", "amt_label.hip", "amt_dynamics.hip", "amt_watershed.hip"):
        for kernel, work in re.findall(r"hipLaunchKernelGGL\((\w+), dim3\(\(([\w* ]+) \+ 63\) / 64\), dim3\(64\)", src[f]):
            if "nplanes" in work:
                book.setdefault(kernel, set()).add(work)
    out["BOOKKEEPING"] = {k: sorted(v) for k, v in sorted(book.items())}
    return out


_LIM: dict = {}


def _limits():
    if not _LIM:
        _LIM.update(limits())
    return _LIM


def radius_of(sigma):
    return int(4.0 * sigma + 0.5)


def _th(rule, gx, H, nplanes, num_cus):
    th, floor, per_cu = rule
    while th > floor and gx * ((H + th - 1) // th) * nplanes < per_cu * num_cus:
        th >>= 1
    return th


def gaussian_variant(lim, shape, dtype, sigma, mode, nplanes, num_cus, aligned=True):
    """launch_fused's choice for a radius 1 .. FR_MAX -> (kernel, TH, gx, partial): ``partial`` the rows of the last row
    group's last four-row step when the plane ends inside it (0: it ends on a step)."""
    H, W = shape
    R = radius_of(sigma)
    assert 1 <= R <= lim["FR_MAX"], R
    lds = dtype == "u16" and aligned and W % 8 == 0 and W >= 256 and mode in ("nearest", "reflect", "mirror") and H > 2 * R
    if lds:
        gx = -(-W // (lim["OUTW"] - 2 * ((R + 7) & ~7)))
        th = _th(lim["TH_lds"], gx, H, nplanes, num_cus)
        return "gauss_lds_kernel", th, gx, H % th % 4
    gx = -(-W // (lim["OUTW"] - 2 * R))
    th = _th(lim["TH_fused"], gx, H, nplanes, num_cus)
    return "gauss_fused_kernel", th, gx, H % th % 4


def codes_variant(lim, shape, sigma, nplanes, num_cus):
    """launch_codes' tile height (the call is refused unless the plane takes gauss_lds_kernel)."""
    H, W = shape
    gx = -(-W // (lim["OUTW"] - 2 * ((radius_of(sigma) + 7) & ~7)))
    th = _th(lim["TH_codes"], gx, H, nplanes, num_cus)
    return "gauss_lds_kernel", th, gx, H % th % 4


def edt_tiles(shape, nplanes):
    return -(-shape[1] // 64) * -(-shape[0] // 64) * nplanes


def edt_variant(lim, shape, nplanes, want_edt):
    """amt_edt's tile rule -> (tile rows, halo rows) of the edt_bits_kernel instance."""
    return lim["EDT_FAR"] if edt_tiles(shape, nplanes) >= lim["EDT_TILES"] and not want_edt else lim["EDT_NEAR"]


def percentile_parts(lim, n, nplanes):
    """amt_percentile_f64's classify pass -> (want, gparts, whether the cap binds); None below PQ_MIN_N (the radix path)."""
    if n < lim["PQ_MIN_N"]:
        return None
    top, lo, hi = lim["PQ_WANT"]
    want = min(max(top // nplanes, lo), hi)
    uncapped = max(1, -(-n // (256 * lim["PQ_VPT"])))
    return want, min(uncapped, want), uncapped > want


def label_trips(lim, nplanes, max_label):
    """Trips of the grid-stride loops over nplanes * max_label rows."""
    block, blocks = lim["NLAB_GRID"]
    nlab = nplanes * max_label
    grid = min(max(1, -(-nlab // block)), blocks)
    return -(-nlab // (grid * block))


def first_far(far, top=1 << 20):
    """The smallest batch size for which ``far(nplanes)`` holds (``far`` is monotone); None when there is none up to top."""
    if not far(top):
        return None
    lo, hi = 0, top  # far(lo) false (or lo == 0), far(hi) true
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if far(mid) else (mid, hi)
    return hi


# ---------------------------------------------------------------------------------------------------------------------
# planes and their order
# ---------------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1)
SLOTS = tuple((kind, seed) for seed in SEEDS for kind in (0, 1, 2))  # the sweep's kinds under two seeds
_ONCE: dict = {}


def _once(key, fn):
    if key not in _ONCE:
        _ONCE[key] = fn()
    return _ONCE[key]


def _seeded(seed, fn):
    """``fn()`` with the sweep's planes drawn for another seed; the sweep's own caches are keyed without the seed and stay
    untouched (nothing here goes through them for seed != 0)."""
    old = sw.SEED
    sw.SEED = int(seed)
    try:
        return fn()
    finally:
        sw.SEED = old


def layout(nplanes, nslots, seed=0, pinned=None):
    """The slot of every plane of a batch: seeded, aperiodic, every slot at least once below index 64 and once at or above
    it where the batch has room (nplanes >= 64 + nslots); ``pinned`` {index: slot} overrides single places afterwards."""
    rng = np.random.default_rng([nplanes, nslots, seed, 4099])
    order = rng.integers(0, nslots, nplanes)
    head = rng.permutation(min(64, nplanes))[:nslots]
    order[head] = np.arange(len(head))
    if nplanes >= 64 + nslots:
        tail = 64 + rng.permutation(nplanes - 64)[:nslots]
        order[tail] = np.arange(nslots)
    for i, s in (pinned or {}).items():
        order[i] = s
    return order


def covers_both_sides(order, nslots):
    return all((order[:64] == s).any() and (order[64:] == s).any() for s in range(nslots))


def is_aperiodic(order):
    n = len(order)
    return n < 4 or not any((order[p:] == order[:-p]).all() for p in range(1, n // 2 + 1))


def compare_planes(outs, order, wants, rules):
    """Every plane i of every output against wants[order[i]] -> (True, None) or (False, (output, plane, where))."""
    for k, rule in enumerate(rules):
        out = outs[k]
        for s in np.unique(order):
            idx = np.flatnonzero(order == s)
            w = wants[s][k]
            if rule is sw.exact and isinstance(out, np.ndarray) and out.dtype != object and isinstance(w, np.ndarray):
                got = out[idx]  # the same rule on all the planes that hold this slot at once
                if got.shape[1:] != w.shape:
                    return False, (k, int(idx[0]), ("shape", got.shape[1:], w.shape))
                bad = got != w[None]
                if got.dtype.kind == "f" or w.dtype.kind == "f":
                    bad &= ~(np.isnan(got.astype(_F64)) & np.isnan(w.astype(_F64))[None])
                if bad.any():
                    at = np.argwhere(bad)[0]
                    return False, (k, int(idx[at[0]]), tuple(int(v) for v in at[1:]))
            else:
                for i in idx:
                    ok, at = rule(out[i], w)
                    if not ok:
                        return False, (k, int(i), at)
    return True, None


class Case:
    """One call.  ``nplanes(num_cus)``: the batch size; ``variant(num_cus)``: what the model says the call takes;
    ``bytes(num_cus)``: the largest operand; ``run(ctx, num_cus)`` -> (outs, ok, index); ``side``: far / near / None."""

    def __init__(self, group, op, name, shape, nplanes, variant, nbytes, run, side=None, switch=None):
        self.group, self.op, self.name, self.shape = group, op, name, tuple(shape)
        self.nplanes, self.variant, self.bytes, self.run, self.side, self.switch = nplanes, variant, nbytes, run, side, switch

    def key(self):
        return (self.group, self.op, self.name, self.shape)


def _batch_case(group, op, name, shape, nplanes, variant, nbytes, slots, ins_of, want_of, dev, rules, side=None, switch=None,
                order_of=None):
    """A call on ``nplanes`` planes laid out from ``slots``; ins_of(slot) / want_of(slot) -> tuples of host arrays."""
    order_of = order_of or (lambda n: layout(n, len(slots)))

    def run(ctx, num_cus):
        n = nplanes(num_cus)
        order = order_of(n)
        ins = [ins_of(s) for s in slots]
        Hs = [np.stack([ins[s][j] for s in order]) for j in range(len(ins[0]))]
        D = [ctx.asarray(h) for h in Hs]
        outs = dev(ctx, D, Hs)
        wants = [want_of(s) for s in slots]
        nout = len(wants[0])
        r = rules.of(nout) if isinstance(rules, _SweepRules) else (rules if isinstance(rules, tuple) else (rules,) * nout)
        ok, at = compare_planes(outs, order, wants, r)
        return outs, ok, at
    case = Case(group, op, name, shape, nplanes, variant, nbytes, run, side, switch)
    case.slots, case.order_of = tuple(slots), order_of
    return case


# ---------------------------------------------------------------------------------------------------------------------
# gaussian tile height
# ---------------------------------------------------------------------------------------------------------------------
TH_TARGETS = (64, 128, 256)
GAUSS_LDS_SHAPE, GAUSS_FUSED_SHAPE = (130, 264), (130, 131)
# (path group, dtype, shape, ((sigma, mode), ...)): radii 2, 8 and FR_MAX on every path
GAUSS_PATHS = (
    ("gaussian lds u16", "u16", GAUSS_LDS_SHAPE, ((0.6, "reflect"), (2.0, "nearest"), (3.0, "mirror"))),
    ("gaussian fused u16", "u16", GAUSS_FUSED_SHAPE, ((0.6, "constant"), (2.0, "wrap"), (3.0, "nearest"))),
    ("gaussian fused f64", "f64", GAUSS_LDS_SHAPE, ((0.6, "wrap"), (2.0, "constant"), (3.0, "reflect"))),
)
SALT = 7  # of the second seed's image planes


def image_slot(dt, shape, slot):
    kind, seed = slot
    return _once(("img", dt, shape, slot), lambda: sw.img(dt, shape, kind, SALT * seed))


def gauss_ref(dt, shape, slot, sigma, mode):
    return _once(("gauss", dt, shape, slot, sigma, mode),
                 lambda: sw._gauss_ref((image_slot(dt, shape, slot),), (dt, sigma, mode)))


def gauss_batch(lim, shape, dt, sigma, mode, target, num_cus):
    """B* of one tile height: the first batch size at which the model's TH reaches ``target``."""
    return first_far(lambda n: gaussian_variant(lim, shape, dt, sigma, mode, n, num_cus)[1] >= target)


def _gauss_variant_text(lim, shape, dt, sigma, mode, n, num_cus):
    kernel, th, gx, partial = gaussian_variant(lim, shape, dt, sigma, mode, n, num_cus)
    return f"{kernel} TH {th} gx {gx}" + (f", last step {partial} rows" if partial else "") + (", H < TH" if shape[0] < th else "")


def _g_gaussian(lim, group):
    _, dt, shape, params = next(g for g in GAUSS_PATHS if g[0] == group)
    itemsize = 2 if dt == "u16" else 8
    cases = []

    def add(sigma, mode, target, side, minmax):
        def nplanes(num_cus):
            b = gauss_batch(lim, shape, dt, sigma, mode, target, num_cus)
            return b if side == "far" else b - 1

        def dev(ctx, D, Hs):
            h = sw._hipops()
            if minmax:
                mm = ctx.empty((D[0].shape[0], 2), _F64)
                return sw._np(h.gaussian(D[0], sigma, mode=mode, cval=0.25, minmax_out=mm), mm)
            return sw._np(h.gaussian(D[0], sigma, mode=mode, cval=0.25))

        def want(slot):
            g = gauss_ref(dt, shape, slot, sigma, mode)[0]
            return (g, np.array([g.min(), g.max()])) if minmax else (g,)
        name = f"sigma {sigma} {mode}{' minmax_out' if minmax else ''}, TH {target} {side}"
        cases.append(_batch_case(
            group, "gaussian", name, shape, nplanes,
            lambda cus: _gauss_variant_text(lim, shape, dt, sigma, mode, nplanes(cus), cus),
            lambda cus: nplanes(cus) * shape[0] * shape[1] * max(itemsize, 8),
            SLOTS, lambda s: (image_slot(dt, shape, s),), want, dev, sw.exact, side, f"TH {target}"))
    for sigma, mode in params:
        for target in TH_TARGETS:
            for side in ("far", "near"):
                add(sigma, mode, target, side, False)
    # the largest radius (the row map at its full length) under every other mode the path takes, at the last switch
    modes = sw.MODES[:3] if group == "gaussian lds u16" else sw.MODES
    sigma_max = max(s for s, _ in params)
    for mode in modes:
        if (sigma_max, mode) not in params:
            for side in ("far", "near"):
                add(sigma_max, mode, TH_TARGETS[-1], side, False)
    sigma, mode = params[1]  # the min / max keys are folded per block: once per path, on both sides of the last switch
    for side in ("far", "near"):
        add(sigma, mode, TH_TARGETS[-1], side, True)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# gaussian + otsu codes
# ---------------------------------------------------------------------------------------------------------------------
CODES_PARAMS = ((2.0, "nearest"), (0.6, "reflect"), (3.0, "mirror"))
# beyond the six planes: a plane of 16 grey levels (a few hundred undecided samples: on the fix-up list) and one of two
# neighbouring grey levels (every other sample undecided: the list overflows and the plane is redone as a whole)
CODES_SLOTS = SLOTS + ("16 grey levels", "one grey level")


def codes_plane(slot):
    if isinstance(slot, tuple):
        return image_slot("u16", GAUSS_LDS_SHAPE, slot)
    span = 16 if slot == "16 grey levels" else 1
    rng = np.random.default_rng([span, 811])
    return _once(("codes plane", slot), lambda: (1000 + rng.integers(0, span + 1, GAUSS_LDS_SHAPE)).astype(_U16))


def codes_ref(slot, sigma, mode):
    return _once(("codes", slot, sigma, mode), lambda: sw._codes_ref((codes_plane(slot),), (sigma, mode)))


def codes_undecided(slot, sigma, mode):
    """How many samples of the plane prefix_codes_kernel cannot decide from the upper 32 bits (the host model of its rule,
    ``_thresholds.prefix_rule``, on the reference's float64 plane); 0 for a constant plane, which is answered before."""
    from arcadia_microscopy_tools_amd._thresholds import prefix_rule

    def count():
        g = ndi.gaussian_filter(skops.img_as_float(codes_plane(slot)), sigma, mode=mode)
        lo, hi = float(g.min()), float(g.max())
        return 0 if lo == hi else int(np.count_nonzero(prefix_rule(g.ravel(), lo, hi)[2]))
    return _once(("undecided", slot, sigma, mode), count)


def codes_roles(lim, sigma, mode):
    """{slot: "nothing listed" | "fix-up list" | "overflow"}"""
    out = {}
    for s in CODES_SLOTS:
        n = codes_undecided(s, sigma, mode)
        out[s] = "nothing listed" if n == 0 else ("fix-up list" if n <= lim["PFX_CAP"] else "overflow")
    return out


def _g_codes(lim, group):
    shape = GAUSS_LDS_SHAPE
    cases = []
    for sigma, mode in CODES_PARAMS:
        for side in ("far", "near"):
            def nplanes(num_cus, sigma=sigma, side=side):
                b = first_far(lambda n: codes_variant(lim, shape, sigma, n, num_cus)[1] >= TH_TARGETS[-1])
                return b if side == "far" else b - 1

            def variant(cus, sigma=sigma, mode=mode, nplanes=nplanes):
                kernel, th, gx, _ = codes_variant(lim, shape, sigma, nplanes(cus), cus)
                roles = list(codes_roles(lim, sigma, mode).values())
                held = ", ".join(f"{roles.count(r)} {r}" for r in ("nothing listed", "fix-up list", "overflow"))
                return f"{kernel} EPI 1 / 2 / 3 TH {th} gx {gx}" + (", H < TH" if shape[0] < th else "") + f"; planes: {held}"
            cases.append(_batch_case(
                group, "gaussian_otsu_codes", f"sigma {sigma} {mode}, both forms, TH {TH_TARGETS[-1]} {side}", shape, nplanes,
                variant, lambda cus, nplanes=nplanes: nplanes(cus) * shape[0] * shape[1] * 4,
                CODES_SLOTS, lambda s: (codes_plane(s),), lambda s, sigma=sigma, mode=mode: codes_ref(s, sigma, mode),
                lambda ctx, D, Hs, sigma=sigma, mode=mode: sw._codes_dev(ctx, D, Hs, (sigma, mode)),
                (sw.exact, sw.exact, sw.exact, sw.exact, sw._hist_or_const, sw.exact), side, f"TH {TH_TARGETS[-1]}"))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# edt tile variant
# ---------------------------------------------------------------------------------------------------------------------
EDT_SHAPES = ((130, 144), (70, 131))
EDT_SLOTS = SLOTS + ("ones", "corner zero", "disk on a seam")


def edt_plane(shape, slot):
    def make():
        if isinstance(slot, tuple):
            return sw.mask_of(shape, slot[0], SALT * slot[1])
        m = np.ones(shape, bool)
        if slot == "corner zero":  # searches as deep and as wide as the plane, across every 64-pixel word
            m[0, 0] = False
        if slot == "disk on a seam":  # radius 30 round the corner four 64 x 64 tiles share (two, where H < 94)
            yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
            m = (yy - 64) ** 2 + (xx - 64) ** 2 <= 30 * 30
        return m
    return _once(("edt plane", shape, slot), make)


def edt_ref(shape, slot):
    return _once(("edt", shape, slot), lambda: sw._edt_ref((edt_plane(shape, slot),), None))


def edt_depths(shape, slot):
    """The row distance from every foreground pixel to the zero scipy names as its nearest (no zero: an empty array)."""
    m = edt_plane(shape, slot)
    if m.all() or not m.any():
        return np.zeros(0, np.int64)
    iy = ndi.distance_transform_edt(m, return_distances=False, return_indices=True)[0]
    return np.abs(iy - np.arange(shape[0])[:, None])[m]


def _g_edt(lim, group):
    cases = []
    for shape in EDT_SHAPES:
        far = lambda cus, shape=shape: first_far(lambda n: edt_tiles(shape, n) >= lim["EDT_TILES"])  # noqa: E731
        for side, want_edt in (("far", False), ("near", False), ("far", True)):
            def nplanes(cus, side=side, far=far):
                return far(cus) - (side == "near")

            def dev(ctx, D, Hs, want_edt=want_edt):
                d2, e = sw._hipops().edt(D[0], want_edt=want_edt)
                return sw._np(d2, e) if want_edt else sw._np(d2)

            def variant(cus, shape=shape, nplanes=nplanes, want_edt=want_edt):
                n = nplanes(cus)
                rows, halo = edt_variant(lim, shape, n, want_edt)
                return f"edt_bits_kernel<{rows}, {halo}> at {edt_tiles(shape, n)} tiles"
            cases.append(_batch_case(
                group, "edt", f"{'d2 and edt' if want_edt else 'd2 alone'}, {lim['EDT_TILES']} tiles {side}", shape, nplanes,
                variant, lambda cus, shape=shape, nplanes=nplanes, want_edt=want_edt:
                nplanes(cus) * shape[0] * shape[1] * (8 if want_edt else 4),
                EDT_SLOTS, lambda s, shape=shape: (edt_plane(shape, s),),
                lambda s, shape=shape, want_edt=want_edt: edt_ref(shape, s)[:2 if want_edt else 1], dev, sw.exact,
                None if want_edt else side, None if want_edt else "EDT tiles"))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# percentile
# ---------------------------------------------------------------------------------------------------------------------
PCT_SHAPE = (256, 1024)
PCT_PLANES = (1, 32, 33, 64)


def _g_percentile(lim, group):
    n = PCT_SHAPE[0] * PCT_SHAPE[1]
    cases = []
    for q in sw._QS:
        for nplanes in PCT_PLANES:
            def variant(cus, nplanes=nplanes):
                want, gparts, binds = percentile_parts(lim, n, nplanes)
                return f"pq_classify_kernel want {want} gparts {gparts}" + (" (capped)" if binds else "")
            binds = percentile_parts(lim, n, nplanes)[2]
            cases.append(_batch_case(
                group, "percentile", f"q {q}, {nplanes} planes", PCT_SHAPE, lambda cus, nplanes=nplanes: nplanes, variant,
                lambda cus, nplanes=nplanes: nplanes * n * 8, SLOTS, lambda s: (image_slot("f64", PCT_SHAPE, s),),
                lambda s, q=q: _once(("pct", s, q), lambda: (np.atleast_1d(np.percentile(image_slot("f64", PCT_SHAPE, s), q)),)),
                lambda ctx, D, Hs, q=q: sw._np(sw._hipops().percentile(D[0], q)), sw.exact,
                "far" if binds else "near", "gparts cap"))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# label-count loops
# ---------------------------------------------------------------------------------------------------------------------
LABEL_SHAPE = (33, 40)
LABEL_MAX = (2048, 2016)  # 130 planes: 266,240 rows (a second trip) and 262,080 (one)


def _props_op():
    return next(o for o in sw.OPS if o.name == "regionprops")


def props_ins(slot, p):
    kind, seed = slot
    return _once(("props in", slot), lambda: _seeded(seed, lambda: tuple(np.array(a) for a in _props_op().make(LABEL_SHAPE, kind, p))))


def props_want(slot, p):
    return _once(("props", slot, p), lambda: _props_op().ref(props_ins(slot, p), p))


def _props_dev_k(ctx, D, Hs, p, K):
    """tests/operator_sweep.py's _props_dev with the tables sized for ``K`` labels per plane, and a third output: whether
    the rows of the labels a plane does not hold follow include/amt_hip.h (area 0; 0 in every extended column)."""
    from arcadia_microscopy_tools_amd.masks import DEFAULT_CELL_PROPERTY_NAMES
    from arcadia_microscopy_tools_amd.segment import assemble_cell_properties, ext_columns

    h = sw._hipops()
    n = Hs[0].shape[0]
    inten = D[1] if p == "u16" else ctx.asarray(Hs[1].astype(_F64) / 7.0)
    names = list(DEFAULT_CELL_PROPERTY_NAMES) + sw.EXT_NAMES
    if p == "u16":
        mt, it = h.regionprops_full(D[0], inten, K)
    else:
        mt, it = h.regionprops(D[0], K), h.regionprops_intensity(D[0], inten, K)
    xt, wt = h.regionprops_ext(D[0], K, ext_columns(names, sw.IPROPS), intensity=inten)
    mt, it, xt, wt = mt.numpy(), it.numpy(), xt.numpy(), wt.numpy()
    out, raw, absent = [], [], np.zeros(n, bool)
    for i in range(n):
        k = int(Hs[0][i].max())
        d = assemble_cell_properties(mt[i][:k], it[i][:k], ("A", "B"), names, sw.IPROPS, ext=xt[i][:k], wext=wt[i][:k])
        out.append((list(d), [np.asarray(v) for v in d.values()]))
        raw.append(np.concatenate([t[i][:k].ravel() for t in (mt, it, xt, wt)]))
        absent[i] = bool((mt[i][k:, 0] == 0).all() and (xt[i][k:] == 0).all() and (wt[i][k:] == 0).all())
    return sw._ragged(out), sw._ragged(raw), absent


def _g_labels(lim, group):
    cases = []
    # the rows of the second trip are those of planes 128 and 129: they hold the planes of several labels (kind 0)
    order_of = lambda n: layout(n, len(SLOTS), pinned={n - 2: 0, n - 1: 3})  # noqa: E731
    for K in LABEL_MAX:
        for p in ("u16", "f64"):
            trips = label_trips(lim, MANY, K)
            cases.append(_batch_case(
                group, "regionprops", f"{p}, max_label {K}", LABEL_SHAPE, lambda cus: MANY,
                lambda cus, K=K, trips=trips: f"{MANY * K} rows: {trips} trip{'s' if trips > 1 else ''} of the nlab loops",
                lambda cus, K=K: MANY * K * 14 * 8, SLOTS, lambda s, p=p: props_ins(s, p),
                lambda s, p=p: props_want(s, p) + (np.asarray(True),),
                lambda ctx, D, Hs, p=p, K=K: _props_dev_k(ctx, D, Hs, p, K),
                (sw.props_rule, lambda g, w: (True, None), sw.exact), "far" if trips > 1 else "near", "nlab trips", order_of))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# many planes through the bookkeeping kernels
# ---------------------------------------------------------------------------------------------------------------------
MANY_SHAPES = ((7, 5), (70, 131))


def sweep_ins(op, pi, shape, slot):
    kind, seed = slot
    if seed == 0:
        return sw.inputs(op, pi, shape, kind)
    return _once(("sweep in", op.name, pi, shape, slot),
                 lambda: _seeded(seed, lambda: tuple(np.array(a, order="C") for a in op.make(shape, kind, op.params[pi]))))


def sweep_want(op, pi, shape, slot):
    kind, seed = slot
    if seed == 0:
        return sw.reference(op, pi, shape, kind)
    return _once(("sweep ref", op.name, pi, shape, slot), lambda: _seeded(seed, lambda: op.ref(sweep_ins(op, pi, shape, slot), op.params[pi])))


def _g_many_sweep(lim, group):
    family = group[len("many planes: "):]
    cases = []
    for op in sw.OPS:
        if op.family != family or not op.planes:
            continue
        for shape in MANY_SHAPES:
            for pi, p in enumerate(op.params):
                cases.append(_batch_case(
                    group, op.name, repr(p), shape, lambda cus: MANY, lambda cus: f"{MANY} planes",
                    lambda cus, shape=shape: MANY * shape[0] * shape[1] * 8 * 3, SLOTS,
                    lambda s, op=op, pi=pi, shape=shape: sweep_ins(op, pi, shape, s),
                    lambda s, op=op, pi=pi, shape=shape: sweep_want(op, pi, shape, s),
                    lambda ctx, D, Hs, op=op, p=p: op.dev(ctx, D, Hs, p), _SweepRules(op, p)))
    return cases


class _SweepRules:
    """The rules of one parameter set of a sweep operator, as many as it has outputs (known once a reference exists)."""

    def __init__(self, op, p):
        self.op, self.p = op, p

    def of(self, nout):
        return sw._rules(self.op, self.p, nout)


def skeleton_planes():
    """zeros and a finished skeleton need no work (one iteration that clears nothing); the random plane a few iterations;
    the three-launch bar of tests/skeleton_cases.py the most its table has."""
    import skeleton_cases as sc

    def make():
        zeros, rnd, bar = next(c for c in sc.skeleton_cases() if c[0] == "batch of three")[2]
        done = skref.skeletonize(rnd)[0]
        return {"zeros": zeros, "finished": done, "random 0.65": rnd, "bar": bar}
    return _once("skeleton planes", make)


def skeleton_want(name):
    return _once(("skeleton", name), lambda: skref.skeletonize(skeleton_planes()[name]))  # (plane, iterations)


# most planes need no work; the ones that do sit on both sides of index 64, the last plane among them
MANY_ORDER = {"work": (5, 63, 64, 129), "some": (40, 100)}


def many_order(n, idle, some, work):
    """Slots ``idle`` (a tuple) alternating aperiodically, ``some`` and ``work`` at the places of MANY_ORDER."""
    order = np.asarray(idle)[np.random.default_rng([n, 977]).integers(0, len(idle), n)]
    order[[0, 70]] = idle[0]
    order[[1, 71]] = idle[-1]
    order[list(MANY_ORDER["some"])] = some
    order[list(MANY_ORDER["work"])] = work
    return order


def recon_planes():
    """The planes of the "batch" case of tests/reconstruction_cases.py (uint16): seed == mask converges at once, the
    serpentine needs the most rounds of the table, the full-range plane a few."""
    import reconstruction_cases as rc

    def make():
        _, fpn, seeds, masks = next(c for c in rc.cases("u16") if c[0] == "batch")
        return {"converged": (seeds[0], masks[0]), "serpentine": (seeds[1], masks[1]), "full range": (seeds[2], masks[2])}, fpn
    return _once("recon planes", make)


def recon_want(name):
    planes, fpn = recon_planes()
    return _once(("recon", name), lambda: rr.flood(*planes[name], rr.FOOTPRINTS[fpn]))


def hmax_planes(kind):
    """A flat plane (one round) and the plane of smooth bumps of tests/reconstruction_cases.py, whose h-domes take many."""
    import reconstruction_cases as rc

    def make():
        bumps = rc.h_image(kind)[0]
        flat = np.full(bumps.shape, bumps.flat[0], bumps.dtype)
        return {"flat": flat, "bumps": bumps, "bumps reversed": np.ascontiguousarray(bumps[::-1, ::-1])}
    return _once(("hmax planes", kind), make)


def hmax_h(kind):
    import reconstruction_cases as rc

    return rc.H_CASES[kind][-1] if kind == "u16" else rc.H_CASES[kind][0]


def hmax_want(kind, name):
    return _once(("hmax", kind, name), lambda: rr.h_extrema(hmax_planes(kind)[name], hmax_h(kind), rr.ONES, True))


def _g_many_rounds(lim, group):
    cases = []
    names = ("zeros", "finished", "random 0.65", "bar")
    planes = skeleton_planes()
    shape = planes["bar"].shape
    cases.append(_batch_case(
        group, "skeletonize", "idle planes and three-launch bars", shape, lambda cus: MANY, lambda cus: f"{MANY} planes",
        lambda cus: MANY * shape[0] * shape[1], names, lambda s: (planes[s],), lambda s: (skeleton_want(s)[0],),
        lambda ctx, D, Hs: (sw._hipops().skeletonize(D[0]).numpy(dtype=_U8),), sw.exact,
        order_of=lambda n: many_order(n, (0, 1), 2, 3)))
    rnames = ("converged", "full range", "serpentine")
    rplanes, fpn = recon_planes()
    rshape = rplanes["serpentine"][0].shape
    cases.append(_batch_case(
        group, "reconstruction", f"uint16 {fpn}: converged planes and serpentines", rshape, lambda cus: MANY,
        lambda cus: f"{MANY} planes", lambda cus: MANY * rshape[0] * rshape[1] * 2, rnames, lambda s: rplanes[s],
        lambda s: (recon_want(s),),
        lambda ctx, D, Hs: sw._np(sw._hipops().reconstruction(D[0], D[1], "dilation", rr.FOOTPRINTS[fpn])), sw.exact,
        order_of=lambda n: many_order(n, (0,), 1, 2)))
    for kind in ("u16", "f64"):
        hp = hmax_planes(kind)
        hshape = hp["bumps"].shape
        cases.append(_batch_case(
            group, "h_maxima", f"{kind} h {hmax_h(kind)}: flat planes and h-domes", hshape, lambda cus: MANY,
            lambda cus: f"{MANY} planes", lambda cus, hshape=hshape: MANY * hshape[0] * hshape[1] * 8,
            ("flat", "bumps reversed", "bumps"), lambda s, hp=hp: (hp[s],), lambda s, kind=kind: (hmax_want(kind, s),),
            lambda ctx, D, Hs, kind=kind: (sw._hipops().h_maxima(D[0], hmax_h(kind)).numpy(dtype=_U8),), sw.exact,
            order_of=lambda n: many_order(n, (0,), 1, 2)))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
_BUILDERS = {**{g[0]: _g_gaussian for g in GAUSS_PATHS}, "gaussian otsu codes": _g_codes, "edt tile variant": _g_edt,
             "percentile": _g_percentile, "label-count loops": _g_labels,
             **{"many planes: " + f: _g_many_sweep for f in sw.FAMILIES}, "many planes: rounds": _g_many_rounds}
GROUPS = list(_BUILDERS)
_TABLE: dict = {}


def table(group):
    """The cases of one group (built once)."""
    if group not in _TABLE:
        _TABLE[group] = _BUILDERS[group](_limits(), group)
        keys = [c.key() for c in _TABLE[group]]
        assert len(set(keys)) == len(keys), f"{group}: two cases share a key"
    return _TABLE[group]


def num_cus_of(device_name):
    m = re.search(r"(\d+) CUs\)", device_name)
    assert m, f"no compute-unit count in {device_name!r}"
    return int(m.group(1))


def check_reach(case, num_cus):
    """A clear message when a case cannot sit on its side on this chip within the memory cap."""
    n = case.nplanes(num_cus)
    assert n is not None and n >= 1, f"{case.key()}: no batch size reaches its side with {num_cus} CUs"
    assert case.bytes(num_cus) < MEMORY_CAP, (f"{case.key()}: {n} planes need an operand of {case.bytes(num_cus)} bytes with "
                                              f"{num_cus} CUs, beyond the cap of {MEMORY_CAP}")


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
def _run_case(ctx, case, num_cus):
    t = time.perf_counter()
    check_reach(case, num_cus)
    outs, ok, at = case.run(ctx, num_cus)
    return {"group": case.group, "op": case.op, "param": case.name, "shape": list(case.shape), "nplanes": case.nplanes(num_cus),
            "variant": case.variant(num_cus), "status": "pass" if ok else "mismatch", "index": None if ok else repr(at),
            "sha256": sw._digest(outs), "ms": round((time.perf_counter() - t) * 1e3, 1)}


def run(ctx, groups=None, scratch_check=False):
    """The cases of the groups (default: all): {"records", "called", "dirty", "seconds", "num_cus"}.  A mismatch is
    recorded and the run goes on; an exception from the library ends it at once."""
    num_cus = num_cus_of(ctx.device_name())
    records = []
    t0 = time.perf_counter()
    with sw.Recorder(ctx, scratch_check) as rec:
        for group in (GROUPS if groups is None else groups):
            for case in table(group):
                rec.where = [case.op, case.name, list(case.shape), case.group]
                records.append(_run_case(ctx, case, num_cus))
            ctx.trim()
    return {"records": records, "called": sorted(rec.called), "dirty": rec.dirty, "seconds": time.perf_counter() - t0,
            "num_cus": num_cus}


def variants_of(records):
    """{group: {variant: calls}}: the report of which side every call sat on."""
    out: dict = {}
    for r in records:
        g = out.setdefault(r["group"], {})
        g[r["variant"]] = g.get(r["variant"], 0) + 1
    return out


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", required=True, help="where to write the records and the scratch findings")
    ap.add_argument("--group", action="append", help="only this group (repeatable)")
    ap.add_argument("--profile", help="also write the run's time, its calls and seconds per group and the variants reached")
    args = ap.parse_args(argv)
    from arcadia_microscopy_tools_amd.device import get_context

    poison = poison_child.poisoned()
    ctx = get_context()
    res = run(ctx, args.group, scratch_check=poison)
    poison_child.write(args.json, res)
    bad = [r for r in res["records"] if r["status"] != "pass"]
    if args.profile:
        groups = GROUPS if args.group is None else args.group
        with open(args.profile, "w") as f:
            json.dump({"device": ctx.device_name(), "poison": poison, "seconds": round(res["seconds"], 2),
                       "calls": len(res["records"]), "mismatches": len(bad),
                       "calls_per_group": {g: sum(r["group"] == g for r in res["records"]) for g in groups},
                       "seconds_per_group": {g: round(sum(r["ms"] for r in res["records"] if r["group"] == g) / 1e3, 2)
                                             for g in groups},
                       "variants": variants_of(res["records"])}, f, indent=1)
            f.write("\n")
    for r in bad[:20]:
        print("MISMATCH", r["group"], r["op"], r["param"], r["shape"], r["nplanes"], r["variant"], r["index"], flush=True)
    for d in res["dirty"][:20]:
        print("DIRTY SCRATCH", d, flush=True)
    print(f"{len(res['records'])} calls, {len(bad)} mismatches, {len(res['dirty'])} dirty scratch checks, "
          f"{res['seconds']:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
