"""The parameter-limit table (tests/parameter_limits.py) without a GPU: every documented range has its lower end, its upper
end, each internal switch and one refusal per side in the table, each at the value ``limits()`` reads from the sources
today; the dispatch each case names is the one the sources take; every refusal stands before the first launch of its entry
point; and every reference runs (once: the device tests share them) and is not degenerate."""
import numpy as np

import operator_sweep as sw
import parameter_limits as pl
from oracle import skops


def _all_cases():
    return [c for g in pl.GROUPS for c in pl.table(g)]


def test_limits_are_read_from_the_sources():
    lim = pl.limits()
    R = pl.ranges(lim)
    # what the issue's table was written against; a retune moves these, and the tests below say which case then left its end
    assert lim["HIST_F64_NBINS"] == (1, 4096) and lim["OTSU_F64_NBINS"] == (2, 4096)
    assert lim["PCT_U16_NQ"] == (1, 64) and lim["PCT_F64_NQ"] == (1, 8) and lim["GAUSS_RADIUS"] == (0, 128)
    assert lim["WINDOW_MAX"] == 255 and lim["FOOTPRINT_SIDE"] == 63 and lim["SIDE_MAX"] == 32768 and lim["PLANES_MAX"] == 65535
    assert lim["NLEAD_MAX"] == 6 and lim["HIST_RANGE_LOG2"] == 28
    # otsu_f64_kernel's LDS at the top of its range fits a workgroup: 32 bytes per bin (40 would end at 4094 bins)
    need = lim["OTSU_LDS_ARRAYS"] * lim["OTSU_F64_NBINS"][1] * 8 + lim["OTSU_LDS_STATIC"]
    assert need <= pl.LDS_BYTES, f"otsu_f64_kernel asks for {need} bytes of LDS at nbins {lim['OTSU_F64_NBINS'][1]}"
    sw_ = R["otsu_f64 nbins"]["switches"]
    assert 40 * sw_["40 bytes per bin would fit LDS"] + 48 <= pl.LDS_BYTES < 40 * sw_["40 bytes per bin would not"] + 48
    assert sorted(sw_.values()) == [4094, 4095]
    # hist_f64_kernel: nbins + 1 edges and four private histograms
    assert (lim["HIST_F64_NBINS"][1] + 1) * 8 + 4 * lim["HIST_F64_NBINS"][1] * 4 <= pl.LDS_BYTES
    assert 256 < lim["PQ_MIN_N"] == 256 * 256
    for _, sigmas, _ in pl.gauss_grid(lim):
        for sigma, r in sigmas.items():
            assert (len(skops.gaussian_weights(sigma)) - 1) // 2 == r == int(4.0 * sigma + 0.5), (sigma, r)
    # conv_v8g_kernel's staged tile: uint16 fits at every radius, float64 up to 124 (320 rows of 64 doubles fill a workgroup)
    assert lim["V8G_LDS_KIB"] * 1024 == pl.LDS_BYTES and pl.v8g_smem(128, 2) <= pl.LDS_BYTES
    assert pl.v8g_f64_radius(lim) == 124 and pl.v8g_smem(124, 8) == 162048 and pl.v8g_smem(125, 8) > pl.LDS_BYTES
    assert pl.v8g_smem(128, 8) == 166216
    assert int(4.0 * ((R["gaussian radius"]["refuse"]["hi"] - 0.2) / 4.0) + 0.5) == lim["GAUSS_RADIUS"][1] + 1


def test_every_range_has_both_ends_each_switch_and_its_refusals():
    lim = pl.limits()
    cases = _all_cases()
    keys = [c.key() for c in cases]
    assert len(set(keys)) == len(keys)
    have = {}
    for c in cases:
        for m in c.marks:
            have.setdefault(tuple(m[:2]), set()).add(m[2])
            assert (m[1].startswith("refuse ")) == (c.expect is not None), c.key()
    assert not pl.EXCLUDED
    R = pl.ranges(lim)
    for name, role, value in pl.wanted_marks(lim):
        assert (name, role) in have, f"no case at {role} of {name}"
        assert have[(name, role)] == {value}, f"{name} {role}: the table's {have[(name, role)]} is not the sources' {value}"
    assert set(n for n, _ in have) == set(R)
    # the issue's list, spelled out where the table derives a value
    assert {m[2] for c in cases for m in c.marks if m[0] == "hist_range nbins"} == {0, 1, 2 ** 26, 2 ** 28, 2 ** 28 + 1}
    assert {c.name for c in pl.table("refusals") if c.op == "gaussian"} == {"sigma 32.2"}
    assert {m[2] for c in pl.table("refusals") for m in c.marks if m[0] == "window"} == {257, 4}
    assert R["min_distance"]["refuse"] == {"lo": -1, "hi": 17} and R["window nlead"]["refuse"]["hi"] == 7
    assert R["overlay layers"]["refuse"]["hi"] == 9 and R["side"]["refuse"]["hi"] == 32769 and R["planes"]["refuse"]["hi"] == 65536
    nbins = {int(c.name.split()[1]) for c in pl.table("histograms and thresholds f64") if c.op == "threshold_otsu"}
    assert nbins == {2, 3, 255, 257, 1024, 4094, 4095, 4096}
    nbins = {int(c.name.split()[1]) for c in pl.table("histograms and thresholds f64") if c.op == "histogram_f64"}
    assert nbins == {1, 2, 255, 257, 1024, 4096}


def test_histogram_regimes_take_the_kernel_the_table_names():
    lim = pl.limits()
    want = {(1024, (7, 5)): ("hist_u16_part_kernel", 1, False), (1025, (7, 5)): ("hist_u16_kernel", 1, False),
            (1024, (8, 8)): ("hist_u16_part_kernel", 1, True), (1025, (8, 8)): ("hist_u16_kernel", 1, True),
            (205, (512, 514)): ("hist_u16_kernel", 2, True)}
    got = {}
    for nplanes, shape, role in pl.hist_regimes(lim):
        n = shape[0] * shape[1]
        kernel, per = pl.hist_u16_kernel_of(lim, nplanes, n)
        got[(nplanes, shape)] = (kernel, per, (n * 2) % 16 == 0)  # every plane of the stack 16-byte aligned: the vector loads
        cases = pl.table(f"hist_u16 {nplanes} x {shape}")
        assert {c.op for c in cases} == {"histogram_u16", "threshold_otsu u16", "percentile u16"}
        assert all(kernel + "," in c.name for c in cases)
    assert got == want
    # 205 planes of (512, 514): five parts each, 1,025 in all, and two workgroups per plane whatever the CU count above 102
    assert -(-512 * 514 // lim["HIST_PART_PX"]) == 5 and 205 * 5 == lim["HIST_MAX_PARTS"] + 1
    assert (512 * 514 + 262143) // 262144 == 2 <= (2 * 103 + 204) // 205
    # the benchmark's batch (32 planes of 2048 x 2048) is on the same side
    assert pl.hist_u16_kernel_of(lim, 32, 2048 * 2048)[0] == "hist_u16_kernel"
    # what every other collected test calls (one to three small planes) is not
    assert pl.hist_u16_kernel_of(lim, 3, 2048 * 2048)[0] == "hist_u16_part_kernel"
    x = pl._regime_planes(1025, (7, 5))
    assert x[0].max() < 32768 <= x[1].min() and (x[2:] < 32768).any() and (x[2:] >= 32768).any()
    pl.forget("regime")


def test_gaussian_and_open_close_paths():
    lim = pl.limits()
    path = lambda dt, r, mode, shape: pl.gaussian_path(lim, dt, r, mode, shape)  # noqa: E731
    assert path("u16", 12, "nearest", (40, 256)) == "gauss_lds" and path("f64", 12, "nearest", (40, 256)) == "gauss_fused"
    assert path("u16", 12, "wrap", (40, 256)) == "gauss_fused" and path("u16", 1, "reflect", (7, 5)) == "gauss_fused"
    assert path("u16", 13, "nearest", (40, 256)) == "conv_v8g + conv_h8"
    assert path("u16", 13, "nearest", (33, 512)) == path("f64", 13, "mirror", (130, 576)) == "conv_v8g + conv_h8g"
    assert path("u16", 13, "wrap", (33, 512)) == "conv_v8g + conv_h8"
    assert path("u16", 128, "nearest", (130, 576)) == path("f64", 128, "reflect", (130, 576)) == "conv_v8 + conv_h8"
    # radius 0 never reaches the filters: amt_gaussian converts or copies
    assert path("u16", 0, "nearest", (7, 5)) == path("u16", 0, "wrap", (33, 512)) == "convert_u16_f64"
    assert path("f64", 0, "reflect", (33, 512)) == path("f64", 0, "constant", (1, 1)) == "copy_f64"
    # the largest radius on a plane tall enough for the LDS-DMA vertical pass: uint16 takes it, float64's tile passes LDS
    assert path("u16", 128, "nearest", pl.GAUSS_TALL) == path("f64", 124, "wrap", pl.GAUSS_TALL) == "conv_v8g + conv_h8"
    assert path("f64", 125, "nearest", pl.GAUSS_TALL) == path("f64", 128, "reflect", pl.GAUSS_TALL) == "conv_v8 + conv_h8"
    assert pl.GAUSS_TALL[0] > 2 * lim["GAUSS_RADIUS"][1] and pl.GAUSS_TALL[1] % 64 == 0
    assert path("u16", 64, "mirror", (130, 576)) == path("f64", 64, "constant", (130, 576)) == "conv_v8g<64> + conv_h8g<64>"
    assert path("f64", 64, "wrap", (130, 576)) == "conv_v8g<64> + conv_h8"
    names = {c.name.split(": ")[1] for c in pl.table("gaussian") if c.op == "gaussian"}
    assert names == {"convert_u16_f64", "copy_f64", "gauss_lds", "gauss_fused", "conv_v8 + conv_h8", "conv_v8g + conv_h8",
                     "conv_v8g + conv_h8g", "conv_v8g<64> + conv_h8g<64>", "conv_v8g<64> + conv_h8"}
    r0 = [c for c in pl.table("gaussian") if c.op == "gaussian" and " r 0 " in c.name]
    assert len(r0) == 50 and all(c.name.endswith(("convert_u16_f64", "copy_f64")) for c in r0)
    for shape in ((33, 512), (130, 576)):  # W % 64 == 0 && W >= 256 + 2 r at the first two-pass radius
        assert shape[1] % 64 == 0 and shape[1] >= 256 + 2 * (lim["FR_MAX"] + 1)
    fps = pl.toc_footprints(lim)
    fused = {n: pl.toc_path(lim, fp) == "toc_fused" for n, (fp, _) in fps.items()}
    assert fused == {"disk(4)": True, "disk(5)": False, "flat rx 16": True, "flat rx 17": False, "block of 256 cells": True,
                     "block of 257 cells": False}
    for n in ("block of 256 cells", "block of 257 cells"):
        fp = fps[n][0]
        assert fp.shape == (9, 33) and np.count_nonzero(fp) == int(n.split()[2]) and fp[0].any() and fp[-1].any() \
            and fp[:, 0].any() and fp[:, -1].any()
    for cells in (lim["MAX_OFFS"], lim["RK_MAX_OFFS"]):
        f = pl.footprints(lim, cells)
        sparse = f[f"sparse 63 x 63, {cells} cells"]
        assert np.count_nonzero(sparse) == cells and not np.array_equal(sparse, sparse[::-1, ::-1])
        assert not np.array_equal(f["L"], f["L"][::-1, ::-1]) and f["one off-centre cell"].sum() == 1 and not f["one off-centre cell"][2, 2]


def test_every_refusal_stands_before_the_first_launch():
    src = pl.sources()
    cases = pl.table("refusals")
    assert len(cases) >= 30
    for c in cases:
        assert c.expect and c.source, c.key()
        ok, why = pl.refusal_precedes_launch(src, c.source)
        assert ok, (c.key(), why)
    # the check sees a launch that comes first: amt_threshold_value once cleared status_dev before it looked at nbins
    body = pl.function_body(src["amt_stats.hip"], "amt_threshold_value")
    assert body.find("nbins >= 2 && nbins <= 4096") < body.find("hipMemsetAsync(status_dev")
    moved = {"amt_stats.hip": src["amt_stats.hip"].replace("hipMemsetAsync(status_dev", "hipMemsetAsync(nothing")
             .replace("AMT_TRY(amt_set_device(ctx));\n    AMT_REQUIRE(in && thr_dev",
                      "AMT_HIP_CHECK(hipMemsetAsync(status_dev, 0, 4, ctx->stream));\n    AMT_REQUIRE(in && thr_dev")}
    assert not pl.refusal_precedes_launch(moved, (("amt_stats.hip", "amt_threshold_value", "nbins >= 2 && nbins <= 4096"),))[0]


def test_the_fast_window_reference_is_the_oracle():
    for shape in ((7, 5), (33, 40)):
        for dt in ("u16", "f64"):
            x = sw.img(dt, shape, 0)
            for w in (1, 3, 15, (5, 9), (1, 15), (15, 1)):
                for method in ("niblack", "sauvola"):
                    want = getattr(skops, "threshold_" + method)(x, window_size=w, k=0.2)
                    assert np.array_equal(pl.window_ref(x, method, w), want), (shape, dt, w, method)
    vol = np.random.default_rng(0).integers(0, 65536, (2, 2, 1, 7, 5)).astype(np.uint16)
    for w in (3, (1, 3, 1, 3, 5)):
        assert np.array_equal(pl.window_ref(vol, "niblack", w), skops.threshold_niblack(vol, window_size=w))
        assert np.array_equal(pl.window_ref(vol, "sauvola", w, r=32767.5), skops.threshold_sauvola(vol, window_size=w, r=32767.5))


def test_the_padded_grey_reference_is_the_oracle_where_scipy_stays_inside_the_plane():
    lim = pl.limits()
    fp = pl.footprints(lim, lim["RK_MAX_OFFS"])["sparse 63 x 63, 1024 cells"]
    x = sw.img_u16((33, 40), 0)
    for fn in (skops.erosion, skops.dilation):
        direct = fn(x, fp)
        padded = fn(np.pad(x, ((31, 31), (31, 31)), mode="symmetric"), fp)[31:-31, 31:-31]
        assert np.array_equal(direct, padded) and np.array_equal(pl.grey_ref(fn, x, fp), direct)
    # on (7, 5) the footprint reaches 4 x 7 rows and 4 x 5 columns beyond the edges: the erosion of a plane is never below its
    # minimum, which scipy's own call is there
    small = sw.img_u16((7, 5), 0)
    assert pl.grey_ref(skops.erosion, small, fp).min() == small.min() and pl.grey_ref(skops.dilation, small, fp).max() == small.max()


def test_bf16_rounding_and_the_rule_of_the_random_case():
    # ties go to the even significand, on both parities of the kept bit
    assert pl.bf16_round(1 + 2.0 ** -8) == 1.0 and pl.bf16_round(1 + 3 * 2.0 ** -8) == 1 + 2.0 ** -6
    assert pl.bf16_round(-(1 + 2.0 ** -8)) == -1.0 and pl.bf16_round(255.5) == 256.0 and pl.bf16_round(0.0) == 0.0
    # against the integer form of round-to-nearest-even on the float32 bits
    f = np.random.default_rng(1).normal(size=4096).astype(np.float32) * np.float32(37.0)
    f[:64] = (np.arange(64, dtype=np.float32) + np.float32(0.5)) * np.float32(2.0 ** -7) + np.float32(1.0)  # exact ties
    u = f.view(np.uint32)
    bits = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    assert np.array_equal(pl.bf16_bits(pl.bf16_round(f.astype(np.float64))), bits)
    lo, hi = pl.bf16_neighbours(f.astype(np.float64))
    assert (lo <= f).all() and (f <= hi).all() and np.array_equal(pl.bf16_values(pl.bf16_bits(lo)), lo)
    # the rule: the nearer neighbour always passes; the farther one only within the bound of the midpoint; anything else never
    v = np.array([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.3])
    mag = np.array([4.0, 4.0])
    near, far = pl.bf16_bits(pl.bf16_round(v)), pl.bf16_bits(np.array([1.0, 1.3046875]))
    assert pl.affine_random_rule(near, (v, mag, 5))[0]
    assert pl.affine_random_rule(np.array([far[0], near[1]]), (v, mag, 5))[0]
    assert pl.affine_random_rule(np.array([near[0], far[1]]), (v, mag, 5)) == (False, (1,))
    assert not pl.affine_random_rule(pl.bf16_bits(np.array([1.0 + 2.0 ** -6, 1.296875])), (v, mag, 5))[0]


def test_affine_cases_hold_what_the_issue_asks():
    lim = pl.limits()
    cfg = pl.affine_configs(lim)
    assert {c[4] for c in cfg} == {8, 24, 64, 256} and {(c[5], c[6]) for c in cfg} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c[7] for c in cfg} == {(), ("y",), ("style",), ("pre_bias",), ("sum_out",), ("y", "style", "pre_bias", "sum_out")}
    assert any(c[1] * c[2] == 65536 and c[3] == 2 and c[4] == 8 for c in cfg), "N = 2, H = 32768: the second launch"
    assert any(c[3] * c[4] // 8 == 32768 > 256 * lim["NN_MAX_BLOCKS_X"] and c[3] == 1024 and c[4] == 256 for c in cfg)
    ties = {"out": set(), "sum": set()}
    for name, N, H, W, C, ups, relu, absent in cfg:
        ins = pl.affine_inputs(name, N, H, W, C, ups)
        for k in ("x", "y", "style", "pre_bias", "shift"):
            assert np.array_equal(ins[k] * 8, np.rint(ins[k] * 8)) and np.abs(ins[k]).max() <= 16
        assert set(np.unique(ins["scale"])) <= {0.5, 1.0, 2.0, -1.0}
        s, v, _, _ = pl.affine_definition(ins, ups, relu, absent)
        assert np.abs(v).max() < 256 and np.array_equal(v * 16, np.rint(v * 16)), "every float32 step is exact"
        for key, val in (("out", v), ("sum", s)):
            m, _ = np.frexp(val)
            q = np.abs(m) * 256.0
            tie = (q - np.floor(q)) == 0.5
            ties[key] |= set(np.unique(np.floor(q[tie]).astype(np.int64) % 2).tolist())
    assert ties == {"out": {0, 1}, "sum": {0, 1}}, "exact ties on both parities of the kept bit"
    assert any(relu == 0 and (pl.affine_definition(pl.affine_inputs(n, N, H, W, C, u), u, 0, a)[1] < 0).any()
               for n, N, H, W, C, u, relu, a in cfg[:12])
    assert any(relu == 1 and (pl.affine_definition(pl.affine_inputs(n, N, H, W, C, u), u, 0, a)[1] < 0).any()
               for n, N, H, W, C, u, relu, a in cfg[:12])
    # the random case: the bound excuses a value only within ~3e-7 x (the terms' magnitudes) of a midpoint, the midpoints lie
    # 2^-8 |v| apart, so only results hundreds of times smaller than their terms are excused: the rule bites on the rest
    c = [c for c in pl.table("affine bf16") if c.op == "nn_affine_act random"][0]
    (v, mag, k), _ = pl.reference(c)
    lo, hi = pl.bf16_neighbours(v)
    bound = k * 2.0 ** -24 / (1 - k * 2.0 ** -24) * mag
    assert (bound < (hi - lo)[hi > lo].min() / 2).all() and np.array_equal(np.abs(v), mag) and (v < 0).any() and (v > 0).any()
    excused = np.abs(v - (lo + hi) / 2) <= bound
    assert excused.mean() < 1e-2 and v.size > 40000


def test_every_reference_runs_once_and_is_not_degenerate():
    n = 0
    varied = {}
    for g in pl.GROUPS:
        for c in pl.table(g):
            if c.expect is not None:
                assert c.want is None
                continue
            want = pl.reference(c)
            assert isinstance(want, tuple) and len(want) >= 1, c.key()
            n += 1
            if c.op in ("threshold_otsu", "otsu_threshold_value", "threshold_otsu u16", "percentile f64", "percentile u16",
                        "percentile u16"):
                assert np.isfinite(np.asarray(want[0], np.float64)).all(), c.key()
            if c.op.startswith("apply_threshold"):
                assert want[0].any() and not want[0].all(), c.key()
            if g in ("binary footprints", "grey footprints", "threshold_open_close", "peaks"):
                w = np.asarray(want[0])
                fp_name = c.name.rsplit(" kind ", 1)[0] if g != "peaks" else c.name
                varied[(g, c.op, fp_name)] = varied.get((g, c.op, fp_name), False) or bool(w.min() != w.max())
        if g.startswith("hist_u16"):
            pl.forget("regime")
    assert n > 800
    # no footprint, and no min_distance, whose result is constant on every plane of the table (empty by construction)
    flat = [k for k, v in varied.items() if not v]
    assert not flat, flat[:10]
    # and case by case where the input is made for it: a dilation / closing of the specks and an erosion / opening of the holes
    # show the footprint itself, and a grey filter of a random (66, 320) plane is never constant
    for c in pl.table("binary footprints"):
        if c.name.endswith(("kind specks", "kind holes")) and \
                (c.op in ("binary_dilation", "binary_closing")) == c.name.endswith("specks"):
            w = pl.reference(c)[0]
            assert w.any() and not w.all(), c.key()
    specks = [c for c in pl.table("binary footprints") if c.name.endswith("kind specks") and c.op == "binary_dilation"]
    assert len(specks) == 7 and len({pl.reference(c)[0].tobytes() for c in specks}) == 7
    for c in pl.table("grey footprints"):
        if c.shape == (66, 320):
            w = pl.reference(c)[0]
            assert w.min() != w.max(), c.key()
    # min_distance 16 clears (16, 16) whole and leaves peaks on (66, 320)
    pk = [c for c in pl.table("peaks") if c.op == "peak_mask" and "min_distance 16" in c.name]
    assert not any(pl.reference(c)[0].any() for c in pk if c.shape == (16, 16))
    assert any(pl.reference(c)[0].any() for c in pk if c.shape == (66, 320))
    one_end = [c for c in pl.table("sides") if c.op == "edt" and c.name == "a zero at one end" and min(c.shape) == 1]
    assert [int(pl.reference(c)[0].max()) for c in one_end] == [32767 ** 2, 32767 ** 2]
    # a reference is made once and shared read-only
    a = pl._side_masks((1, 8))
    assert a["no zero pixel"].all()
    assert not pl._once(("in", "smooth"), lambda: None).flags.writeable
