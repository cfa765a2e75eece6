"""The census of tests/dynamics_limits.py without a GPU: every switch of csrc/amt_dynamics.hip has a case strictly on each
side and, where the switch is a number, one exactly on it.  The numbers come from the kernel source
(dynamics_limits.limits), so a retune that unhooks a case fails here.  Each test names, for one row of switches, the cases
on either side.  All facts are taken from the oracle (``cd.follow_flows`` -> histogram, ``cd.get_masks`` without its size
filters), never from how the inputs were built."""
import numpy as np
import pytest

import dynamics_limits as dl
from oracle import cellpose_dynamics as cd

LIM = dl.limits()
R = LIM["CP_RPAD"]


@pytest.fixture(scope="module")
def cen():
    """(group, name) -> (case, census), made once."""
    return {(c["group"], c["name"]): (c, dl.census(c, LIM)) for c in dl.cases()}


def _masks(cen, name, group="seeds and growth", plane=0):
    c, ce = cen[(group, name)]
    return c, ce["planes"][plane]


def test_limits_are_those_of_the_source():
    assert LIM["DIFFUSE_CLASSES"][0][1] == 0 and LIM["DIFFUSE_CLASSES"][2][0] == 0
    assert LIM["DIFFUSE_CLASSES"][0][0] == LIM["DIFFUSE_CLASSES"][1][1] < LIM["DIFFUSE_CLASSES"][1][0] == LIM["DIFFUSE_CLASSES"][2][1]
    assert LIM["DIFFUSE_STRIDES"][0] == LIM["LABEL_STRIDE"] == LIM["HOLES_STRIDE"] > LIM["DIFFUSE_STRIDES"][1] > LIM["DIFFUSE_STRIDES"][2]
    assert LIM["GROW_FLOOR"] < LIM["SEED_FLOOR"] and LIM["GROW_PATCH"] == 2 * LIM["GROW_ROUNDS"] + 1
    assert np.float32(LIM["MOVES"]) == np.float32(1e-3)
    assert dl.EXCLUDED == {} and dl.GROUPS == ["seeds and growth", "size filters", "diffusion classes", "holes"]
    assert {c["group"] for c in dl.cases()} == set(dl.GROUPS)
    assert all(c["kind"] in ("masks", "flow_error", "holes") for c in dl.cases())


def test_the_histogram_is_what_the_cases_say(cen):
    """The programmable histogram, from the oracle's own end positions: the piles hold the named counts at row 0 / the last
    row / column 0 / the last column (corners included), every other bin holds at most what a neighbour pile holds."""
    _, row = _masks(cen, "bins of 10, 11 and 20")
    h = row["hist"]
    assert [int(h[R, R + x]) for x in (10, 30, 40)] == [2 * LIM["SEED_FLOOR"], LIM["SEED_FLOOR"] + 1, LIM["SEED_FLOOR"]]
    h = h.copy()
    h[R, [R + 10, R + 30, R + 40]] = 0
    assert h.max() == 1
    H, W = 40, 50
    where = {"top": lambda i: (R, R + i), "bottom": lambda i: (R + H - 1, R + i), "left": lambda i: (R + i, R),
             "right": lambda i: (R + i, R + W - 1)}
    for side, at in where.items():
        _, row = _masks(cen, f"piles in the corners and on the edge: {side}")
        last = (W if side in ("top", "bottom") else H) - 1
        assert [int(row["hist"][at(i)]) for i in (0, 1, last // 2, last - 1, last)] == [20, 3, 11, 3, 20], side
        assert sorted(row["seed_bins"]) == sorted([list(at(0)), list(at(last // 2)), list(at(last))]), side
        assert row["sizes"] == [11, 23, 23] and row["hist_max_elsewhere"] == 3
    corners = set()
    for side in where:
        corners |= {tuple(b) for b in _masks(cen, f"piles in the corners and on the edge: {side}")[1]["seed_bins"]}
    assert {(R, R), (R, R + W - 1), (R + H - 1, R), (R + H - 1, R + W - 1)} <= corners


def test_seed_floor(cen):
    """`v <= 10` in cp_seeds_kernel.  On it: the bin of 10 in "bins of 10, 11 and 20" (no seed).  Above: the bins of 11 and 20
    (seeds).  Below: the bins of 1 everywhere."""
    _, row = _masks(cen, "bins of 10, 11 and 20")
    f = LIM["SEED_FLOOR"]
    assert row["seed_counts"] == [2 * f, f + 1] and row["hist_max_elsewhere"] == f and row["sizes"] == [f + 1, 2 * f]
    assert int((row["hist"] == 1).sum()) > 1000


def test_grow_floor_and_rounds(cen):
    """`> 2` in cp_grow_kernel: neighbours of 2 (on it: not grown), 3 (above: grown) and 1 (below) on either side of a seed;
    five rounds in an 11 x 11 patch: of a run of seven bins of 3 beside a seed, five join the region."""
    g, rounds = LIM["GROW_FLOOR"], LIM["GROW_ROUNDS"]
    _, row = _masks(cen, "neighbours of 2 and 3")
    h, pre = row["hist"], row["pre"]
    assert [int(h[R, R + x]) for x in (9, 10, 11, 29, 30, 31)] == [g, 20, g + 1, g + 1, 20, g]
    assert row["sizes"] == [20 + g + 1] * 2
    assert (pre[:g, 9] == 0).all() and (pre[:g, 31] == 0).all() and (pre[:g + 1, 11] > 0).all() and (pre[:g + 1, 29] > 0).all()
    _, row = _masks(cen, "a run of 7 bins above 2")
    h, pre = row["hist"], row["pre"]
    assert all(int(h[R, R + x]) == g + 1 for x in range(11, 11 + rounds + 2))
    assert row["nseeds"] == 1 and row["sizes"] == [20 + (g + 1) * rounds]
    assert (pre[0, 10:11 + rounds] > 0).all() and (pre[0, 11 + rounds:13 + rounds] == 0).all()


def test_tie_order_and_the_later_seed(cen):
    """cp_rank_kernel orders equal counts by raster index, descending; cp_grow_kernel gives overlaps to the later seed.  Two
    tied seeds 4 bins apart with different reaches: in the other order the oracle makes one label, in this one two.  The
    plateaus: 520 (above the 512 workgroups of cp_grow_kernel) and 512 (on it) tied seeds whose regions all overlap."""
    c, row = _masks(cen, "two tied seeds 4 bins apart")
    assert row["seed_counts"] == [20, 20] and abs(row["seed_bins"][0][1] - row["seed_bins"][1][1]) == 4
    assert row["seed_bins"][0][1] > row["seed_bins"][1][1]  # descending raster index: the left seed is the later one
    assert row["sizes"] == [12, 52] and dl.tie_order_matters(c)
    stride = LIM["GROW_STRIDE"]
    for n, above in ((520, True), (512, False)):
        c, row = _masks(cen, f"plateau of {n} tied seeds")
        assert row["nseeds"] == n and set(row["seed_counts"]) == {24} and (n > stride) == above and (n == stride) != above
        assert int(dl.reference(c)[0][0][1]) == n - LIM["GROW_ROUNDS"]  # every region's owner is decided by the order
        assert dl.tie_order_matters(c)  # in the other order the label of six columns stands at the other end
    assert max(r["nseeds"] for (g, _), (_, ce) in cen.items() for r in ce["planes"] if "nseeds" in r and ce["shape"][1] < 500) < stride


def test_max_seeds(cen):
    """`k < cap` in cp_seeds_kernel, `nseeds > cap` in cp_map_kernel.  On it: three seeds, max_seeds 3 (valid).  Above: three
    seeds with max_seeds 2, four with 3 (count -1).  Below: every other case (16,384).  The two batch cases hold a fitting and
    an overflowing plane in either order."""
    c, row = _masks(cen, "max_seeds equal to the seed count")
    assert row["nseeds"] == c["params"]["max_seeds"] and not row["overflow"] and int(dl.reference(c)[0][0][1]) == 3
    c, row = _masks(cen, "max_seeds one below the seed count")
    assert row["nseeds"] == c["params"]["max_seeds"] + 1 and row["overflow"] and int(dl.reference(c)[0][0][1]) == -1
    for name, order in (("batch: fitting plane, overflowing plane", [False, True]),
                        ("batch: overflowing plane, fitting plane", [True, False])):
        c, ce = cen[("seeds and growth", name)]
        assert [r["overflow"] for r in ce["planes"]] == order
        assert [r["nseeds"] - c["params"]["max_seeds"] for r in ce["planes"]] == [int(o) for o in order]
        assert [w[0] is None for w in dl.reference(c)[0]] == order
    _, row = _masks(cen, "bins of 10, 11 and 20")
    assert row["nseeds"] < 16384 and not row["overflow"]


def test_moves_and_threshold_at_equality(cen):
    """`cellprob > thr`: one pixel ON the threshold is no cell (its column then holds 10: no seed), a column one ulp above is.
    `|dY / 5| > 1e-3`: a row whose dY / 5 is float32(1e-3) exactly stays, the row one ulp above piles up."""
    c, row = _masks(cen, "cellprob on the threshold")
    h = row["hist"]
    assert row["on_threshold"] == 1 and [int(h[R, R + x]) for x in (10, 20, 30)] == [11, LIM["SEED_FLOOR"], 11]
    assert row["seed_counts"] == [11, 11] and sorted(b[1] - R for b in row["seed_bins"]) == [10, 30]
    assert c["planes"][0][1][0, 30] == np.nextafter(np.float32(c["params"]["thr"]), np.float32(1))
    d_eq, d_above = dl.moves_pair()
    t = np.float32(LIM["MOVES"])
    assert d_eq / np.float32(5) == t and d_above / np.float32(5) == np.nextafter(t, np.float32(1)) and d_above == np.nextafter(d_eq, np.float32(1))
    c, row = _masks(cen, "dY / 5 on 1e-3 and one ulp above")
    h = row["hist"]
    assert row["on_moves"] == 11 and row["movers"] == 31 and row["cells"] == 42
    assert [int(h[R + y, R]) for y in (5, 15, 25)] == [1, 11, 20] and row["seed_counts"] == [20, 11]
    assert (c["planes"][0][0][0, 5, :11] == d_eq).all() and (c["planes"][0][0][0, 15, :11] == d_above).all()
    # niter 0 and the planes of two rows / two columns
    assert _masks(cen, "niter 0")[1]["nseeds"] == 0 and _masks(cen, "niter 0")[1]["movers"] > 0
    assert cen[("seeds and growth", "two rows")][1]["shape"] == [2, 50] and cen[("seeds and growth", "two columns")][1]["shape"] == [50, 2]
    assert _masks(cen, "two rows")[1]["sizes"] == [31] == _masks(cen, "two columns")[1]["sizes"]


def test_size_floor_on_every_path(cen):
    """min_size in cp_map_kernel (plain path), cp_keep_kernel (post path) and cp_holes_seq_kernel (flagged planes): labels of
    min_size - 1, min_size and min_size + 1 pixels through compute_masks alone, with fill_holes alone, and with a
    flow_threshold above every error alone; the sequential kernel's floor is met by "fragment in a hole, ring first"."""
    for name, post in (("plain path", False), ("fill_holes alone", True), ("flow_threshold alone", True)):
        c, row = _masks(cen, f"floor 14 15 16, {name}", "size filters")
        m, p = c["params"]["min_size"], c["params"]
        assert row["sizes"] == [m - 1, m, m + 1] and bool(p["flow_threshold"] or p["fill_holes"]) == post
        assert (p["flow_threshold"] > 0) != p["fill_holes"] or not post
        if p["flow_threshold"]:
            assert max(row["errors"]) < p["flow_threshold"] and len(row["errors"]) == 3
        want = dl.reference(c)[0][0]
        assert int(want[1]) == 2 and sorted(np.bincount(want[0].ravel())[1:].tolist()) == [m, m + 1]
    c, ce = cen[("holes", "fragment in a hole, ring first, min_size 15, fill 1")]
    lab = c["planes"][0]
    assert ce["planes"][0]["flagged"] and (lab == 2).sum() >= 15 > (lab[4:6, 20:24] == 2).sum() == 8
    assert int(dl.reference(c)[0][0][1]) == 1  # the package's loop drops label 2: what remains of it is below the floor


def test_size_ceiling_in_float64(cen):
    """big = int(H * W * max_size_fraction) in cp_map_kernel: labels of big - 1, big, big + 1.  2,000 pixels x 0.01: float64
    gives 20, the float32 fraction 19 (a float32 interface would drop the label of 20).  200 pixels x 0.4: 80 both ways."""
    for name in ("ceiling 19 20 21 of 2000 x 0.01", "ceiling 19 20 21 of 2000 x 0.01, post path"):
        c, row = _masks(cen, name, "size filters")
        n, f = c["planes"][0][1].size, c["params"]["frac"]
        assert n % 100 == 0 and row["big"] == int(n * f) == 20 and row["big_f32"] == int(n * float(np.float32(f))) == 19
        assert row["sizes"] == [row["big"] - 1, row["big"], row["big"] + 1]
        want = dl.reference(c)[0][0]
        assert sorted(np.bincount(want[0].ravel())[1:].tolist()) == [row["big"] - 1, row["big"]]
    for k, total in enumerate((79, 80, 81)):
        c, row = _masks(cen, f"ceiling {total} of 200 x 0.4", "size filters")
        n, f = c["planes"][0][1].size, c["params"]["frac"]
        assert n % 100 == 0 and row["big"] == int(n * f) == int(n * float(np.float32(f))) == row["big_f32"] == 80
        assert row["sizes"] == [row["big"] - 1 + k] and int(dl.reference(c)[0][0][1]) == (1 if total <= row["big"] else 0)
    assert float(np.float32(0.4)) > 0.4 and float(np.float32(0.01)) < 0.01


def test_diffusion_classes(cen):
    """`npx <= TILE_MIN || (TILE_MAX > 0 && npx > TILE_MAX)` with the ringed tile (h + 2)(w + 2): boxes of exactly 2304
    (class 0), 2305 and 6400 (class 1) and 6401 pixels (class 2), apart, touching pairwise, and against the frame; far below:
    every small label.  Through cellpose_masks the oracle makes the same boxes where they stand apart or on the frame."""
    (a, _), (b, _) = LIM["DIFFUSE_CLASSES"][:2]
    for name in dl.DIFFUSE_BOXES:
        c, ce = cen[("diffusion classes", f"four boxes {name}")]
        rows = ce["planes"][0]["labels"]
        assert sorted((r["tile"], r["class"]) for r in rows) == [(a, 0), (a + 1, 1), (b, 1), (b + 1, 2)], name
        assert ce["planes"][0]["touching"] == (name == "touching")
        assert all(r["frame"] for r in rows) == (name == "frame")
        lab = c["planes"][0][0]
        through = [(c2, ce2) for (g, n), (c2, ce2) in cen.items() if n.startswith(f"four boxes {name}, flow_threshold")]
        assert len(through) == 5
        for c2, ce2 in through:
            row = ce2["planes"][0]
            pre = row["pre"]
            if name == "touching":  # border pixels change sides: still four touching labels, in more than one class
                assert row["nseeds"] == 4 and dl._touch(pre) and not np.array_equal(pre, lab)
                assert len({dl.diffuse_class(LIM, *[s.stop - s.start for s in sl]) for sl in dl.ndi.find_objects(pre)}) >= 2
            else:
                assert np.array_equal(pre, lab), name
            e = np.sort(row["errors"])
            t = c2["params"]["flow_threshold"]
            assert t == float(np.float32(t)) and not (e == t).any()
        # the thresholds separate every pair of errors: 0, 1, 2, 3 and 4 labels survive
        assert sorted(int(dl.reference(c2)[0][0][1]) for c2, _ in through) == [0, 1, 2, 3, 4]
    small = cen[("diffusion classes", "centre ties")][1]["planes"][0]["labels"]
    assert all(r["tile"] < a and r["class"] == 0 for r in small)


def test_label_numbering_and_centre_ties(cen):
    """Labels missing from the numbering (1, 3, 6) with nlabels equal to max_label, and below it with and without an empty
    slot of its own; centres: the 2 x 2 block (four equidistant pixels) and the transpose-symmetric mask (0,1), (1,0), (3,3),
    whose mean 4 / 3 is no dyadic number (two equidistant pixels)."""
    for nl, mx in ((6, 6), (6, 9), (7, 9)):
        c, ce = cen[("diffusion classes", f"labels 1 3 6, nlabels {nl}, max_label {mx}")]
        assert [r["label"] for r in ce["planes"][0]["labels"]] == [1, 3, 6] and c["params"] == {"max_label": mx, "nlabels": nl}
        e = dl.reference(c)[0][0][0]
        assert e.shape == (mx,) and (e[[0, 2, 5]] > 0).all() and (np.delete(e, [0, 2, 5]) == 0).all()
    ties = cen[("diffusion classes", "centre ties")][1]["planes"][0]["labels"]
    assert [r["centre_ties"] for r in ties] == [4, 2]


def test_strides(cen):
    """The label loops stride by 2048 workgroups (cp_centers_kernel, cp_diffuse_kernel, cp_flow_error_kernel,
    cp_holes_kernel), the seed loop by 512.  Above: 2,116 labels / rings, 520 seeds.  On: 2,048 labels / rings, 512 seeds.
    Below: every other case.  The 512 and 256 of the two larger diffusion classes are not crossed."""
    for k in (2116, 2048):
        ce = cen[("diffusion classes", f"{k} labels of 3 x 3")][1]
        assert ce["planes"][0]["present"] == ce["planes"][0]["max"] == k and {r["class"] for r in ce["planes"][0]["labels"]} == {0}
        ce = cen[("holes", f"{k} rings of 3 x 3, min_size 0, fill 1")][1]
        assert len(ce["planes"][0]["kept"]) == k and not ce["planes"][0]["flagged"]
    assert 2048 == LIM["LABEL_STRIDE"] == LIM["HOLES_STRIDE"] < 2116
    per_class = {0: 0, 1: 0, 2: 0}
    for (g, n), (c, ce) in cen.items():
        if c["kind"] == "flow_error":
            for cl in per_class:
                per_class[cl] = max(per_class[cl], sum(r["class"] == cl for r in ce["planes"][0]["labels"]))
    assert per_class[1] < LIM["DIFFUSE_STRIDES"][1] and per_class[2] < LIM["DIFFUSE_STRIDES"][2]  # not crossed: stated, not hidden


def test_hole_tile_and_flags(cen):
    """`h * w > CP_HOLE_TILE`: a frame whose box is exactly CP_HOLE_TILE bytes (parallel kernel) and one byte more (the plane
    is flagged); `h < 3 || w < 3`: boxes of 2 x 10 and 10 x 2 (skipped), 3 x 3 (on the limit: handled), larger ones; the
    `nested` flag: a kept label in another's hole in either label order (flagged), a dropped one (not flagged), none."""
    tile = LIM["CP_HOLE_TILE"]
    on = cen[("holes", "frame on the tile, min_size 0, fill 1")][1]["planes"][0]
    past = cen[("holes", "frame one byte past the tile, min_size 0, fill 1")][1]["planes"][0]
    assert max(on["boxes"]) == tile and not on["flagged"] and max(past["boxes"]) == tile + 1 and past["large"] == [1] and past["flagged"]
    for name, want in (("batch: unflagged frame, flagged frame", [False, True]), ("batch: flagged frame, unflagged frame", [True, False])):
        for m in (0, 15):
            assert [r["flagged"] for r in cen[("holes", f"{name}, min_size {m}, fill 1")][1]["planes"]] == want
    flat = cen[("holes", "boxes of 2 x N, N x 2 and 3 x 3, min_size 0, fill 1")][1]["planes"][0]
    assert flat["flat"] == [1, 2] and flat["boxes"] == [20, 20, 9, 9] and not flat["flagged"]
    c = cen[("holes", "boxes of 2 x N, N x 2 and 3 x 3, min_size 0, fill 1")][0]
    assert int((dl.reference(c)[0][0][0] == 3).sum()) == 9 > int((c["planes"][0] == 3).sum())  # the 3 x 3 ring is filled
    for order in ("ring first", "ring later"):
        for m in (0, 15):
            assert cen[("holes", f"fragment in a hole, {order}, min_size {m}, fill 1")][1]["planes"][0]["nested"]
            small = cen[("holes", f"small label in a hole, {order}, min_size {m}, fill 1")][1]["planes"][0]
            assert bool(small["nested"]) == small["flagged"] == (m == 0)
    # the two label orders of the fragment case give different results under the package's loop: 1 and 2 labels
    got = [int(dl.reference(cen[("holes", f"fragment in a hole, {o}, min_size 15, fill 1")][0])[0][0][1]) for o in ("ring first", "ring later")]
    assert got == [1, 2]
    # spirals: nothing is a hole / everything is
    for closed, name in ((False, "open spiral"), (True, "closed spiral")):
        c = cen[("holes", f"{name}, min_size 0, fill 1")][0]
        want = dl.reference(c)[0][0][0]
        assert (int((want > 0).sum()) == 41 * 41) == closed and (np.array_equal(want, c["planes"][0])) != closed
    # a value above max_label is background
    c = cen[("holes", "a value above max_label, min_size 0, fill 1")][0]
    assert c["planes"][0].max() == 7 > c["params"]["max_label"] and dl.reference(c)[0][0][0].max() == 2
    # every input runs with min_size 0 and 15, filled and not
    names = {n.rsplit(", min_size", 1)[0] for (g, n), (c, _) in cen.items() if c["kind"] == "holes"}
    assert all(("holes", f"{n}, min_size {m}, fill {int(f)}") in cen for n in names for m, f in dl.HOLE_PARAMS) and len(names) == 14
    # through cellpose_masks: the frame's hole holds a label of 14 pixels: flagged at min_size 0, not at 15
    c, row = _masks(cen, "a frame with a label in its hole, min_size 0", "holes")
    assert row["sizes"] == [14, 14, 16, 54]
    for m, flagged in ((0, True), (15, False)):
        flags = dl.hole_flags(LIM, row["pre"], int(row["pre"].max()), int(row["pre"].max()), m)
        assert flags["flagged"] == flagged and bool(flags["nested"]) == flagged


def test_references_are_quick_and_are_the_oracle(cen):
    """No reference takes longer than 3 s from nothing (remembered diffusion results counted at their cost); the
    remembered ``masks_to_flows`` leaves ``cd.compute_masks`` what it is."""
    slow = {k: round(dl.reference(c)[1], 2) for k, (c, _) in cen.items() if dl.reference(c)[1] > 3.0}
    assert not slow, slow
    assert cd.masks_to_flows is dl._MASKS_TO_FLOWS
    c = cen[("diffusion classes", "centre ties")][0]
    assert np.array_equal(dl.reference(c)[0][0][0], cd.flow_error(*c["planes"][0]))
    c = cen[("size filters", "floor 14 15 16, flow_threshold alone")][0]
    p = c["params"]
    m = cd.compute_masks(*c["planes"][0], p["thr"], p["niter"], p["min_size"], p["frac"], p["flow_threshold"], p["fill_holes"])
    assert np.array_equal(dl.reference(c)[0][0][0], m)
