"""The work-size table (tests/batch_scale_cases.py) without a GPU: the model against the source patterns, the batch sizes
it derives for 256 compute units, the memory cap for 256 and 304, and the conditions on the content of the batches --
EDT search depths, planes on and off the fix-up list, planes that need very different numbers of rounds, every distinct
plane on both sides of index 64 -- from the references alone."""
import numpy as np
import pytest

import batch_scale_cases as bs
import operator_sweep as sw


@pytest.fixture(scope="module")
def lim():
    return bs.limits()


def test_model_reads_the_rules_from_the_sources(lim):
    # today's values: a retune changes them here first, and the tests below say which case left its switch
    for name in ("TH_lds", "TH_fused", "TH_codes"):
        assert lim[name] == (256, 32, 4), name
    assert lim["OUTW"] == 256 and lim["FR_MAX"] == 12
    assert lim["EDT_TILES"] == 4096 and lim["EDT_FAR"] == (64, 16) and lim["EDT_NEAR"] == (32, 24)
    assert lim["PQ_WANT"] == (4096, 64, 256) and lim["PQ_VPT"] == 8 and lim["PQ_MIN_N"] == 65536
    assert lim["NLAB_GRID"] == (256, 1024)
    assert lim["PFX_CNT_STRIDE"] == 32 and lim["PKM_CNT_STRIDE"] == 32 and lim["PFX_CAP"] == 8192
    # the 64-thread bookkeeping kernels and what their grids count
    assert lim["BOOKKEEPING"] == {
        "cp_seq_count_kernel": ["nplanes"], "fill_i32_kernel": ["nplanes"], "minmax_finish_kernel": ["2 * nplanes"],
        "minmax_init_kernel": ["nplanes"], "sel_finish_kernel": ["nplanes * nq"], "sel_overflow_kernel": ["nplanes"],
        "sp_clamp_kernel": ["nplanes"], "ws_set_flags_kernel": ["nplanes"]}
    # 130 planes put work in a second and a third block of each of them
    nq = max(len(q) for q in sw._QS)
    assert bs.MANY > 128 and 2 * bs.MANY > 256 and bs.MANY * nq > 64 * 12


def test_tile_height_model(lim):
    # single planes and the suite's widest batch stay at the floor or below the last switch
    assert bs.gaussian_variant(lim, (130, 264), "u16", 2.0, "nearest", 1, 256) == ("gauss_lds_kernel", 32, 2, 2)
    assert bs.gaussian_variant(lim, (2048, 2048), "u16", 2.0, "nearest", 5, 256)[1] == 64
    assert bs.gaussian_variant(lim, (2048, 2048), "u16", 2.0, "nearest", 14, 256)[1] == 128
    assert bs.gaussian_variant(lim, (2048, 2048), "u16", 2.0, "nearest", 15, 256)[1] == 256  # the headline run's side
    # the paths: uint16 with an aligned width and a reflecting mode takes the LDS kernel, everything else the fused one
    assert bs.gaussian_variant(lim, (130, 264), "u16", 2.0, "wrap", 1, 256)[0] == "gauss_fused_kernel"
    assert bs.gaussian_variant(lim, (130, 264), "f64", 2.0, "nearest", 1, 256)[0] == "gauss_fused_kernel"
    assert bs.gaussian_variant(lim, (130, 131), "u16", 2.0, "nearest", 1, 256)[0] == "gauss_fused_kernel"
    assert bs.gaussian_variant(lim, (16, 264), "u16", 2.0, "nearest", 1, 256)[0] == "gauss_fused_kernel"  # H <= 2 R
    # H = 130: every TH of the table ends in a partial step of 2 rows; TH = 256 also has H < TH
    for th in bs.TH_TARGETS:
        assert 130 % th % 4 == 2
    assert 130 < 256


def test_batch_sizes_for_256_compute_units(lim):
    for group, dt, shape, params in bs.GAUSS_PATHS:
        want = [342, 512, 1024] if shape == (130, 131) else [171, 256, 512]
        for sigma, mode in params:
            got = [bs.gauss_batch(lim, shape, dt, sigma, mode, t, 256) for t in bs.TH_TARGETS]
            assert got == want, (group, sigma, mode, got)
            kernel, _, gx, _ = bs.gaussian_variant(lim, shape, dt, sigma, mode, 1, 256)
            assert kernel == ("gauss_lds_kernel" if group == "gaussian lds u16" else "gauss_fused_kernel")
            assert gx == (1 if shape == (130, 131) else 2)
            for t, b in zip(bs.TH_TARGETS, got):  # B* sits on the switch: one plane fewer halves the tile
                assert bs.gaussian_variant(lim, shape, dt, sigma, mode, b, 256)[1] == t
                assert bs.gaussian_variant(lim, shape, dt, sigma, mode, b - 1, 256)[1] == t // 2
    assert {radius for _, _, _, params in bs.GAUSS_PATHS for radius in (bs.radius_of(s) for s, _ in params)} == {2, 8, lim["FR_MAX"]}
    modes = {g: {m for _, m in params} for g, _, _, params in bs.GAUSS_PATHS}
    assert modes["gaussian lds u16"] == {"nearest", "reflect", "mirror"}
    assert {"constant", "wrap"} <= modes["gaussian fused u16"] and {"constant", "wrap"} <= modes["gaussian fused f64"]
    # at the last switch the largest radius meets every mode its path takes
    for group, want in (("gaussian lds u16", sw.MODES[:3]), ("gaussian fused u16", sw.MODES), ("gaussian fused f64", sw.MODES)):
        for side in ("far", "near"):
            assert {c.name.split()[2].rstrip(",") for c in bs.table(group)
                    if c.name.startswith("sigma 3.0 ") and c.name.endswith(f"TH 256 {side}")} == set(want), group
    for sigma, _ in bs.CODES_PARAMS:
        assert bs.first_far(lambda n: bs.codes_variant(lim, (130, 264), sigma, n, 256)[1] >= 256) == 512
    # the EDT rule: (130, 144) has 9 tiles, (70, 131) has 6
    assert [bs.first_far(lambda n: bs.edt_tiles(s, n) >= lim["EDT_TILES"]) for s in bs.EDT_SHAPES] == [456, 683]
    assert bs.edt_tiles((130, 144), 456) == 4104 and bs.edt_tiles((130, 144), 455) == 4095
    assert bs.edt_variant(lim, (130, 144), 456, False) == (64, 16) and bs.edt_variant(lim, (130, 144), 455, False) == (32, 24)
    assert bs.edt_variant(lim, (130, 144), 456, True) == (32, 24)
    # percentile: 262,144 samples make 128 parts; the cap starts to bind at 33 planes
    n = bs.PCT_SHAPE[0] * bs.PCT_SHAPE[1]
    assert n == 262144 and [bs.percentile_parts(lim, n, k) for k in bs.PCT_PLANES] == [
        (256, 128, False), (128, 128, False), (124, 124, True), (64, 64, True)]
    assert bs.percentile_parts(lim, 65536, 5) == (256, 32, False) and bs.percentile_parts(lim, 65535, 5) is None
    # the label loops: a second trip from 262,145 rows
    assert [bs.label_trips(lim, bs.MANY, k) for k in bs.LABEL_MAX] == [2, 1]
    assert bs.MANY * 2048 == 266240 and bs.MANY * 2016 == 262080 and bs.label_trips(lim, 5, 2048) == 1


@pytest.mark.parametrize("group", bs.GROUPS)
def test_every_case_reaches_its_side_within_the_cap(group):
    cases = bs.table(group)
    assert cases, group
    for num_cus in bs.CU_COUNTS:
        for c in cases:
            bs.check_reach(c, num_cus)
            assert isinstance(c.variant(num_cus), str)
    # both sides of every switch the group names
    sides = {}
    for c in cases:
        if c.switch is not None:
            sides.setdefault((c.switch, c.name.rsplit(",", 1)[0], c.shape), set()).add(c.side)
    if group.startswith(("gaussian", "edt")):
        assert sides and all(v == {"far", "near"} for v in sides.values()), sides
    if group in ("percentile", "label-count loops"):
        assert {c.side for c in cases} == {"far", "near"}


@pytest.mark.parametrize("group", bs.GROUPS)
def test_every_distinct_plane_sits_on_both_sides_of_index_64(group):
    for c in bs.table(group):
        for num_cus in bs.CU_COUNTS:
            n = c.nplanes(num_cus)
            order = c.order_of(n)
            assert len(order) == n and order.min() >= 0 and order.max() < len(c.slots)
            assert bs.is_aperiodic(order), c.key()
            if n >= 64 + len(c.slots):
                assert bs.covers_both_sides(order, len(c.slots)), c.key()
            else:
                assert group == "percentile" and n in bs.PCT_PLANES
            assert np.array_equal(order, c.order_of(n))  # fixed: the child process lays out the same batch


def test_batches_hold_at_least_six_planes():
    assert len(bs.SLOTS) == 6 and {k for k, _ in bs.SLOTS} == {0, 1, 2} and {s for _, s in bs.SLOTS} == {0, 1}
    for dt, shape in (("u16", (130, 264)), ("u16", (130, 131)), ("f64", (130, 264)), ("f64", bs.PCT_SHAPE)):
        planes = [bs.image_slot(dt, shape, s) for s in bs.SLOTS]
        distinct = {p.tobytes() for p in planes}
        assert len(distinct) == 5  # kind 1 is the sweep's constant plane under either seed
    for shape in bs.EDT_SHAPES:
        assert len({bs.edt_plane(shape, s).tobytes() for s in bs.EDT_SLOTS}) == 8


def test_edt_batches_hold_the_depths_that_separate_the_instances(lim):
    far_halo, near_halo = lim["EDT_FAR"][1], lim["EDT_NEAR"][1]
    assert (far_halo, near_halo) == (16, 24)
    for shape in bs.EDT_SHAPES:
        depths = np.concatenate([bs.edt_depths(shape, s) for s in bs.EDT_SLOTS])
        between = int(np.count_nonzero((depths > far_halo) & (depths <= near_halo)))
        beyond = int(np.count_nonzero(depths > near_halo))
        assert between > 100 and beyond > 100, (shape, between, beyond)
        assert bs.edt_plane(shape, "ones").all() and np.count_nonzero(~bs.edt_plane(shape, "corner zero")) == 1
        # the disk crosses the seam of the 64-row tiles (and of the 32-row ones) and of the 64-pixel words
        disk = bs.edt_plane(shape, "disk on a seam")
        assert disk[63, 63] and disk[64, 64] and disk[63, 64] and disk[64, 63] and not disk[0, 0]
    # (130, 144): an interior 64-row tile and a last tile of 2 rows
    assert 130 // 64 == 2 and 130 % 64 == 2 and -(-144 // 64) == 3


def test_codes_batches_hold_planes_on_and_off_the_fixup_list(lim):
    for sigma, mode in bs.CODES_PARAMS:
        assert sw._codes_supported(bs.GAUSS_LDS_SHAPE, sigma, mode)
        roles = bs.codes_roles(lim, sigma, mode)
        # the constant planes list nothing; the sweep's random and tied planes and the plane of 16 grey levels put a few
        # to a few thousand samples on the list; the plane of two neighbouring grey levels overflows it
        assert roles[(1, 0)] == roles[(1, 1)] == "nothing listed"
        assert roles[(0, 0)] == roles["16 grey levels"] == "fix-up list"
        assert roles["one grey level"] == "overflow"
        assert bs.codes_undecided("16 grey levels", sigma, mode) > 64  # more than one trip of the fix-up blocks' loop


def test_round_counts_differ_within_a_batch():
    counts = {name: bs.skeleton_want(name)[1] for name in bs.skeleton_planes()}
    assert counts["zeros"] == counts["finished"] == 1 and 1 < counts["random 0.65"] < counts["bar"], counts
    import skeleton_cases as sc

    assert counts["bar"] > sc.T  # more sub-iterations than one launch runs: several launches
    planes, fpn = bs.recon_planes()
    changed = {name: int(np.count_nonzero(bs.recon_want(name) != planes[name][0])) for name in planes}
    H, W = planes["serpentine"][0].shape
    # a converged plane is its own result; the serpentine's fill walks a corridor of about half the plane, pixel by pixel
    assert changed["converged"] == 0 and changed["full range"] > 0 and changed["serpentine"] > H * W // 3, changed
    for kind in ("u16", "f64"):
        hp = bs.hmax_planes(kind)
        assert hp["flat"].min() == hp["flat"].max() and not np.array_equal(hp["bumps"], hp["bumps reversed"])
        marks = bs.hmax_want(kind, "bumps")
        assert 0 < marks.sum() < marks.size
    # the planes that need work sit on both sides of index 64, the last plane among them
    order = bs.many_order(bs.MANY, (0, 1), 2, 3)
    for slot in range(4):
        assert (order[:64] == slot).any() and (order[64:] == slot).any()
    assert order[63] == order[64] == order[bs.MANY - 1] == 3 and np.count_nonzero(order >= 2) == 6


def test_label_loop_case_measures_rows_of_the_second_trip(lim):
    case = bs.table("label-count loops")[0]
    order = case.order_of(bs.MANY)
    block, blocks = lim["NLAB_GRID"]
    first_plane = block * blocks // 2048  # the plane that holds the first row of the second trip
    assert first_plane == 128
    for i in range(first_plane, bs.MANY):
        labels = bs.props_ins(bs.SLOTS[order[i]], "u16")[0]
        assert labels.max() >= 2, i
    assert max(int(bs.props_ins(s, "u16")[0].max()) for s in bs.SLOTS) < 2016


def test_many_planes_groups_cover_every_batched_operator():
    names = {c.op for g in bs.GROUPS if g.startswith("many planes: ") for c in bs.table(g)}
    assert {o.name for o in sw.OPS if o.planes} <= names
    assert {"skeletonize", "reconstruction", "h_maxima"} <= names
    for g in bs.GROUPS:
        if g.startswith("many planes: ") and g != "many planes: rounds":
            cases = bs.table(g)
            assert {c.shape for c in cases} == set(bs.MANY_SHAPES)
            per_op = {o.name: len(o.params) for o in sw.OPS if o.planes and "many planes: " + o.family == g}
            for name, nparams in per_op.items():
                assert sum(c.op == name for c in cases) == nparams * len(bs.MANY_SHAPES), name


def test_compare_planes_names_the_plane():
    order = np.array([0, 1, 0, 1])
    wants = [(np.zeros((2, 2)),), (np.ones((2, 2)),)]
    out = np.stack([wants[s][0] for s in order])
    assert bs.compare_planes((out,), order, wants, (sw.exact,)) == (True, None)
    out[2, 1, 0] = np.nan
    assert bs.compare_planes((out,), order, wants, (sw.exact,)) == (False, (0, 2, (1, 0)))
    assert bs.compare_planes((out,), order, wants, (sw.close(0, 0),)) == (False, (0, 2, (1, 0)))
    assert bs.first_far(lambda n: n >= 7) == 7 and bs.first_far(lambda n: False) is None and bs.first_far(lambda n: True) == 1
    assert bs.num_cus_of("AMD Instinct MI355X (gfx950:sramecc+:xnack-, 256 CUs)") == 256
