"""The census of tests/worstcase_content.py without a GPU: every content switch of the labelling and watershed kernels
has an input strictly on each side and, where the kernels name a limit, one exactly on it.  The limits come from the kernel
sources (worstcase_content.limits), so a retune that unhooks an input fails here.  Each test names, for one row of
switches, the inputs on either side."""
import os

import numpy as np
import pytest

import operator_sweep as sw
import worstcase_content as wc

LIM = wc.limits()
RUNS_OK = [s for s in wc.SHAPES if s[1] % 16 == 0 and (s[0] * s[1]) % 16 == 0]  # amt_i_ccl_runs_ok


@pytest.fixture(scope="module")
def cen():
    """census of every pattern on every shape, made once."""
    return {(n, s): wc.census(wc.plane(n, s), lim=LIM) for s in wc.SHAPES for n in wc.PATTERNS}


def test_limits_are_those_of_the_sources():
    assert LIM["XR_CAP"] == LIM["SR_CAP"] <= LIM["RT_CAP"] == 64 * LIM["ROW_RUNS"]
    assert LIM["S_PX"] < LIM["M_PX"] < LIM["M2_PX"] < LIM["L_PX"] < LIM["X_PX"] and LIM["LAB16"] == 0xFFFF
    assert RUNS_OK == wc.SHAPES[:2]  # two shapes take the run-table paths, (129, 131) the parent plane
    assert len(wc.PATTERNS) == 2 * len(wc.THIN) and not wc.EXCLUDED  # no label or watershed case is left out
    for name in wc.PATTERNS:
        for shape in wc.SHAPES:
            assert wc.plane(name, shape).shape == shape and wc.plane(name, shape).dtype == bool


def test_runs_per_tile_and_per_row(cen):
    """XR_CAP (ccl_expand_runs_kernel) on every shape with W % 16 == 0; SR_CAP (ws_stats_runs_kernel,
    ws_final_runs_kernel) on the same shapes through the marker-list route.
    Below: full, frame, rows, serpentine, corners, seam_zip and every thick pattern but the thick checkerboards / columns.
    Above: noise50 (~1,050), diag4 / anti4 (1,024), crossed8, the thick checkerboards (704).
    On RT_CAP and 32 runs per row: checker0/1, cols0/1, comb_bottom / comb_top.
    On SR_CAP itself: the 16 columns the right edge of (130, 144) cuts from a checkerboard tile."""
    for shape in RUNS_OK:
        tiles = {n: cen[(n, shape)]["runs_per_tile"] for n in wc.PATTERNS}
        rows = {n: cen[(n, shape)]["runs_per_row"] for n in wc.PATTERNS}
        for n in ("full", "frame", "rows", "serpentine", "corners", "seam_zip", "noise50_x3", "serpentine_x3"):
            assert 0 < tiles[n] < LIM["SR_CAP"], (n, shape)
        for n in ("noise50", "diag4", "anti4", "crossed8", "checker0_x3", "cols1_x3"):
            assert LIM["SR_CAP"] < tiles[n] < LIM["RT_CAP"], (n, shape)
        for n in ("checker0", "checker1", "cols0", "cols1", "comb_bottom", "comb_top"):
            assert tiles[n] == LIM["RT_CAP"] and rows[n] == LIM["ROW_RUNS"], (n, shape)
        assert max(tiles.values()) == LIM["RT_CAP"] and max(rows.values()) == LIM["ROW_RUNS"]
        assert 1 <= rows["noise50"] < LIM["ROW_RUNS"]
        # the tiles above the cap hold markers: the statistics and the final mapping have work there
        for n in ("noise50", "checker0", "comb_bottom"):
            assert cen[(n, shape)]["markers"] > 1000
    # a tile cut by the right edge, exactly on the cap
    m = wc.plane("checker0", (130, 144))[:64, 128:]
    assert m.shape == (64, 16) and wc.run_counts(m)[0] == LIM["SR_CAP"]
    # what the operator sweep's own masks reach: below the cap on every shape (its gather branches stay cold)
    most = [wc.run_counts(sw.mask_of(s, k)) for s in sw.SHAPES for k in (0, 1, 2)]
    assert max(t for t, _ in most) < LIM["XR_CAP"] and max(r for _, r in most) < LIM["ROW_RUNS"]


def test_run_table_path_of_the_watershed(cen):
    """`runs` in watershed_components needs the d2 relief, the fused tail, a marker list and W % 16 == 0: the chain's
    marker-list route on (192, 192) and (130, 144).  There it meets noise (noise50), thin structures (serpentine, spiral,
    rings, combs: floods of one-pixel-wide components), tiles cut by both edges with RT_CAP runs (checker0 on (130, 144)),
    and tiles with no run at all (corners), whose rcomp entries stay untouched under poison."""
    assert "watershed_edt_cleared list" in wc.WATERSHED_OPS
    for shape in RUNS_OK:
        for n in ("noise50", "noise50_x3", "serpentine", "comb_bottom", "comb_top_x3", "spiral_x3", "corners_x3"):
            c = cen[(n, shape)]["classes"]
            assert sum(c[k] for k in ("S", "M", "M2", "L", "X", "G")) >= 1, (n, shape)  # a flood, not only fills
    edge = wc.plane("checker0", (130, 144))
    assert wc.run_counts(edge[:64, :64])[0] == LIM["RT_CAP"] and wc.run_counts(edge[128:, 128:])[0] == 16
    assert wc.run_counts(wc.plane("corners", (192, 192))[:63, :63])[0] == 0


def test_components_per_plane(cen):
    """row_stride = n / 2 + 1 component rows per plane.  On it: checker0 on (129, 131), ceil(n / 2) components at
    connectivity 1 (one component at connectivity 2).  One below: checker0/1 on (192, 192), n / 2.  Far below: the rest."""
    n = 129 * 131
    c = cen[("checker0", (129, 131))]
    assert c["components_c1"] == n // 2 + 1 == -(-n // 2) and c["components_c2"] == 1
    assert cen[("checker1", (129, 131))]["components_c1"] == n // 2
    assert cen[("checker0", (192, 192))]["components_c1"] == 192 * 192 // 2
    assert cen[("full", (129, 131))]["components_c1"] == 1
    assert max(v["components_c1"] for (_, s), v in cen.items() if s == (129, 131)) == n // 2 + 1


def _class_rows():
    rows = []
    for mask, mk in wc.class_limit_planes():
        rows += wc.census(mask, mk, wc.chain_inputs(mask)[1], LIM)["rows"]
    return rows


def test_flood_class_limits():
    """Area (x1 - x0 + 3) (y1 - y0 + 3) against S_PX / M_PX / M2_PX / L_PX / X_PX: the first box of every LIMIT_BOXES pair is
    ON the limit, the second the next larger box.  Largest d2 against S_NB = M_NB / M2_NB / L_NB: the squares of
    LIMIT_BOXES on either side, the diamonds of DIAMONDS (512, 2048) and the 64 x 64 square (1024) exactly on the first
    value that no longer fits.  Every component holds two markers of different labels, so its class is a flood class."""
    rows = _class_rows()
    assert all(r["mcnt"] == 2 and r["cls"] in ("S", "M", "M2", "L", "X", "G") for r in rows)
    by = {}
    for r in rows:
        by.setdefault((r["area"], r["cmax"]), r["cls"])

    def cls_of(box):
        w, h = box
        return by[((w + 2) * (h + 2), ((min(w, h) + 1) // 2) ** 2)]

    order = ["S", "M", "M2", "L", "X", "G"]
    for c in ("S", "M", "M2", "L", "X"):
        on, past = wc.LIMIT_BOXES["area " + c]
        assert (on[0] + 2) * (on[1] + 2) == LIM[c + "_PX"] < (past[0] + 2) * (past[1] + 2), c
        assert cls_of(on) == c and cls_of(past) == order[order.index(c) + 1], c
    for nb, below, above in ((LIM["M_NB"], "M", "M2"), (LIM["M2_NB"], "M2", "L"), (LIM["L_NB"], "L", "G")):
        lo, hi = wc.LIMIT_BOXES[f"cmax {nb}"]
        assert (lo[0] // 2) ** 2 < nb <= (hi[0] // 2) ** 2
        assert cls_of(lo) == below and cls_of(hi) == above, nb
    # exactly on the limit: d2 = NB is the first value that no longer fits
    assert by[(64 * 64, LIM["M_NB"])] == "M2" and LIM["M_PX"] == 64 * 64       # the cut diamond: area fits M, d2 does not
    assert by[(66 * 66, LIM["M2_NB"])] == "L"                                  # the 64 x 64 square
    assert by[(129 * 129, LIM["L_NB"])] == "G" and 129 * 129 <= LIM["L_PX"]    # the diamond: area fits L, d2 fits nothing
    assert {r["cls"] for r in rows} == set(order)
    # NB - 1 is not reachable: no sum of two squares
    squares = {a * a + b * b for a in range(50) for b in range(50)}
    assert not {LIM["M_NB"] - 1, LIM["M2_NB"] - 1, LIM["L_NB"] - 1} & squares


def test_persistent_flood_never_waits_for_slots_it_cannot_get(cen):
    """ws_flood_persist_kernel spins until `need` contiguous LDS slots are free: every component of class S / M / M2 / L
    among the inputs -- the boxes on the area limits included -- needs at most PF_SLOTS, with the pixel count of the
    run-table statistics and without it; the 382 x 62 box on L_PX needs the most."""
    rows = _class_rows() + [r for c in cen.values() for r in c["rows"]]
    need = [max(wc.pf_slots_needed(LIM, r["area"], r["cmax"], r["npix"]), wc.pf_slots_needed(LIM, r["area"], r["cmax"], 0))
            for r in rows if r["cls"] in ("S", "M", "M2", "L")]
    assert len(need) > 500 and 56 <= max(need) <= LIM["PF_SLOTS"], max(need)
    assert wc.pf_slots_needed(LIM, LIM["L_PX"], LIM["L_NB"] - 1, 0) <= LIM["PF_SLOTS"]  # the largest class-L component


def test_boxes_of_thin_components(cen):
    """One-pixel-wide components whose BOX picks the class, not their pixel count: the serpentine, the combs and (thick)
    the spiral span the plane -- class G on (192, 192), where the box is above X_PX, class L on the two smaller shapes;
    staircases (diag4 at connectivity 1: single pixels; crossed8 at connectivity 2) and rings for the box filters."""
    for n in ("serpentine", "comb_bottom", "comb_top", "serpentine_x3", "comb_bottom_x3", "spiral_x3"):
        assert cen[(n, (192, 192))]["classes"]["G"] == 1 and cen[(n, (192, 192))]["flooded_area_max"] > LIM["X_PX"], n
        for shape in wc.SHAPES[1:2] if n == "spiral_x3" else wc.SHAPES[1:]:  # on (129, 131) that spiral's peaks are one marker
            c = cen[(n, shape)]
            assert c["classes"]["L"] == 1 and LIM["M2_PX"] < c["flooded_area_max"] <= LIM["L_PX"], (n, shape)
            assert c["components_c1"] == 1
    m = wc.plane("serpentine", (130, 144))
    assert np.count_nonzero(m) < m.size * 0.52  # half the plane's pixels, the whole plane's box
    assert cen[("spiral", (192, 192))]["components_c1"] == 1 and cen[("rings", (192, 192))]["components_c1"] == 48


def test_marker_labels_at_16_bits():
    """labmax >= 0xFFFF sends a component to class G.  Below: 65534 (and every pattern's own labels: at most 18,050).  On
    it: 65535.  Above: 70000."""
    mask, mk = wc.labels16_case()
    offs = wc.labels16_offsets(LIM, mk)
    d2 = wc.chain_inputs(mask)[1]
    got = []
    for off in [0] + offs:
        c = wc.census(mask, np.where(mk > 0, mk + off, 0), d2, LIM)
        got.append((c["labmax"], c["classes"]["G"], c["classes"]["S"] + c["classes"]["M"]))
    assert [g[0] for g in got] == [int(mk.max()), LIM["LAB16"] - 1, LIM["LAB16"], 70000]
    assert got[0][1] == got[1][1] == 0 and got[0][2] == got[1][2] == 3  # three flooded components, all in LDS
    assert got[2][1] >= 1 and got[3][1] == 3                            # the component that holds label 65535; all of them


@pytest.mark.parametrize("lattice,conn", [(lat, c) for lat in ("p4", "p2", "checker") for c in (2, 1)])
def test_heap_beyond_lds(lattice, conn):
    """GH_LDS_N heap slots live in LDS, the rest in HBM.  Above: every heap case (13,622 to 28,447 entries at the peak).
    The reference of these cases does not rest on one restatement: the C oracle and the heapq emulation agree."""
    d2, mk, mask = wc.heap_case(lattice, conn == 1)
    flat = d2[mk > 0]
    if conn == 1:  # the tied pair, and nothing else, repeats a value
        assert flat.size - np.unique(flat).size == 1 and d2[100, 100] == d2[100, 101] and mk[100, 100] != mk[100, 101]
        assert not mask[99:102, [99, 102]].any() and not mask[[99, 101], 99:103].any()
    else:
        assert np.unique(flat).size == flat.size
    assert (d2[mask & (mk == 0)] == 1).all() and flat.min() > 1
    lab, peak = wc.flood_heapq(-np.sqrt(d2.astype(np.float64)), mk, mask, conn)
    assert peak > LIM["GH_LDS_N"], peak
    assert np.array_equal(lab, wc.heap_ref(lattice, conn))


def test_heap_of_the_existing_cases_stays_in_lds():
    """Below GH_LDS_N: the plain relief of tests/golden/c2c3_256.npz peaks at 1,012 / 1,366 entries."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2c3_256.npz"))
    e = wc.skops.distance_transform_edt(g["mask"])
    peaks = [wc.flood_heapq(-e, g["markers"], g["mask"], c)[1] for c in (1, 2)]
    assert peaks == [1012, 1366] and max(peaks) < LIM["GH_LDS_N"]


def test_references_agree_on_the_label_cases():
    """scipy.ndimage.label and the raster pass of oracle/clabel.c are independent; both number every pattern alike."""
    for shape in wc.SHAPES:
        for name in wc.PATTERNS:
            for conn in (1, 2):
                assert np.array_equal(wc.label_ref(name, shape, conn), wc.label_ref_int(name, shape, conn)), (name, shape, conn)
