"""Relating two label images, the parts that need no device: the numpy reference against contingency tables recorded from
scikit-image (tests/golden/relate.npz), the header's and the binding's constants, and the best-partner rule of
``metrics.average_precision`` against an optimal assignment."""
import os
import re

import numpy as np
import pytest

import relate_cases as rc
import relate_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "amt_hip.h")) as f:
        return f.read()


def _define(header, name):
    m = re.search(r"#define\s+" + name + r"\s+(\S+.*)", header)
    assert m, name
    return m.group(1).strip()


def test_reference_equals_the_recorded_contingency_tables(golden):
    g = golden("relate")
    assert str(g["skimage_version"]) == "0.18.3"
    assert str(g["numpy_version"]) and str(g["scipy_version"])
    cases = [k[len("table/"):] for k in g.files if k.startswith("table/")]
    assert sorted(cases) == sorted(f"{s[0]}x{s[1]}_{n}" for s, n in rc.GOLDEN)
    for (shape, name), case in zip(rc.GOLDEN, (f"{s[0]}x{s[1]}_{n}" for s, n in rc.GOLDEN)):
        a, b, k = g[f"labels/{case}"], g[f"companion/{case}"], int(g[f"max_label/{case}"])
        mine = rc.cases(shape)[name]
        assert np.array_equal(a, mine[0]) and np.array_equal(b, mine[1]) and k == mine[2], case  # the same planes
        table = g[f"table/{case}"]
        want = rr.columns_from_table(table, k)
        assert np.array_equal(rr.relate_columns(a, b, k), want), case
        assert np.array_equal(rc.reference(shape, name), want), case
        assert np.array_equal(rr.contingency(a, b), table), case
    # what the recorded cases cover
    gaps = rr.columns_from_table(g["table/33x40_gaps"], int(g["max_label/33x40_gaps"]))
    assert (gaps[1::3] == 0).all() and gaps[:, 3].sum() > 0
    assert (rr.columns_from_table(g["table/33x40_dense"], 5)[:, 2] > 8).all()
    assert not rr.columns_from_table(g["table/70x131_zero_companion"], 12)[:, :3].any()


def test_reference_tie_rule_and_special_values():
    ties = rc.reference((7, 5), "ties")
    assert ties.tolist() == [[3, 7, 2, 14], [7, 7, 3, 21]]
    a = np.array([[1, 1, 1, 1, 2, 0]])
    b = np.array([[rc.BIG, rc.BIG, 4, 4, 0, 9]])
    assert rr.relate_columns(a, b, 3).tolist() == [[4, 2, 2, 4], [0, 0, 0, 1], [0, 0, 0, 0]]
    assert rr.columns_from_table(rr.contingency(a, np.minimum(b, 50)), 3).tolist() == [[4, 2, 2, 4], [0, 0, 0, 1],
                                                                                        [0, 0, 0, 0]]


def test_header_defines_and_documents_the_relation():
    h = _header()
    assert eval(_define(h, "AMT_RPX_RELATE").replace("u", "")) == 256
    assert _define(h, "AMT_RPX_ALL") == "0xffu"
    assert [int(_define(h, "AMT_RPX_RCOL_" + n)) for n in ("PARENT", "OVERLAP", "PARTNERS", "AREA")] == [0, 1, 2, 3]
    assert int(_define(h, "AMT_RELATE_LDS_PARTNERS")) >= 64
    block = h[h.index("AMT_RPX_RELATE ----"):h.index("#define AMT_RPX_EULER_NUMBER")]
    for word in ("smallest", "distinct", "AMT_I32", "AMT_EINVAL", "AMT_RPX_CENTROID_WEIGHTED", "AMT_RELATE_LDS_PARTNERS",
                 "AMT_RPX_RCOL_PARENT", "AMT_RPX_RCOL_OVERLAP", "AMT_RPX_RCOL_PARTNERS", "AMT_RPX_RCOL_AREA"):
        assert word in block, word


def test_binding_constants_equal_the_header():
    from arcadia_microscopy_tools_amd import _hip

    h = _header()
    assert _hip.RPX_RELATE == 256 == 1 << 8
    assert _hip.RELATE_LDS_PARTNERS == int(_define(h, "AMT_RELATE_LDS_PARTNERS"))
    assert _hip.RPX_RCOLS == ("parent", "overlap", "partners", "area")
    for i, n in enumerate(_hip.RPX_RCOLS):
        assert int(_define(h, "AMT_RPX_RCOL_" + n.upper())) == i
    assert _hip.I32 == int(_define(h, "AMT_I32"))
    src = open(os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc", "amt_relate.hip")).read()
    assert "RL_SLOTS = AMT_RELATE_LDS_PARTNERS" in src  # the kernel's table is sized by the header's constant


def test_existing_column_tables_are_unchanged():
    from arcadia_microscopy_tools_amd import _hip

    assert _hip.RPX_BITS == {
        "euler_number": 1, "perimeter_crofton": 2, "area_filled": 4, "feret_diameter_max": 8, "centroid_local": 16,
        "inertia_tensor": 32, "inertia_tensor_eigvals": 64, "centroid_weighted": 128, "centroid_weighted_local": 128}
    assert _hip.RPX_COLS == (
        "euler_number", "perimeter_crofton", "area_filled", "feret_diameter_max", "centroid_local-0", "centroid_local-1",
        "inertia_tensor-0-0", "inertia_tensor-0-1", "inertia_tensor-1-0", "inertia_tensor-1-1", "inertia_tensor_eigvals-0",
        "inertia_tensor_eigvals-1")
    assert _hip.RPX_WCOLS == ("centroid_weighted-0", "centroid_weighted-1", "centroid_weighted_local-0",
                              "centroid_weighted_local-1")
    assert all(not bits & _hip.RPX_RELATE for bits in _hip.RPX_BITS.values())
    assert "amt_regionprops_ext" in _hip._SIGS and not any("relate" in name for name in _hip._SIGS)


# ---- the best-partner rule of metrics.average_precision --------------------------------------------------------------
THRESHOLDS = (0.5, 0.55, 2.0 / 3.0, 0.75, 0.9, 1.0)


def _rule(true, pred, thresholds=THRESHOLDS):
    from arcadia_microscopy_tools_amd import metrics

    n_true, n_pred = int(true.max()), int(pred.max())
    return metrics.average_precision_from_relations(rr.relation(true, pred, n_true), rr.relation(pred, true, n_pred),
                                                    thresholds)


def _assert_same(true, pred, what):
    got, want = _rule(true, pred), rr.average_precision_assignment(true, pred, THRESHOLDS)
    for g, w, name in zip(got, want, ("ap", "tp", "fp", "fn")):
        assert np.array_equal(g, w, equal_nan=True), (what, name, g, w)
    return got


def _random_pair(seed):
    """Two sequentially numbered label images that share most of their borders: blocks of a coarse grid, some merged,
    some split in exact halves, some shifted by a pixel, some dropped -- IoU values of exactly 0.5 included."""
    rng = np.random.RandomState(seed)
    H, W = 4 * rng.randint(2, 6), 4 * rng.randint(2, 6)
    yy, xx = np.mgrid[0:H, 0:W]
    true = ((yy // 4) * (W // 4) + xx // 4 + 1).astype(np.int64)
    pred = true.copy()
    nb = int(true.max())
    for l in range(1, nb + 1):
        r = rng.randint(0, 8)
        m = true == l
        if r == 0:
            pred[m & (xx % 4 >= 2)] = nb + l  # split in two exact halves
        elif r == 1:
            pred[m] = 0
        elif r == 2 and l > 1:
            pred[m] = l - 1  # merged with the block before
        elif r == 3:
            pred[m & (yy % 4 == 0)] = 0  # loses a row: IoU 0.75
        elif r == 4:
            pred[m & (yy % 4 >= 2)] = 0  # loses half: IoU 0.5
        elif r == 5:
            true[m & (xx % 4 == 3)] = 0
    if rng.randint(0, 3) == 0:
        pred = np.roll(pred, 1, axis=1)

    def sequential(a):
        vals, inv = np.unique(a, return_inverse=True)
        inv = inv.reshape(a.shape)
        return inv if vals[0] == 0 else inv + 1

    return sequential(true), sequential(pred)


def test_rule_equals_assignment_on_random_pairs():
    pytest.importorskip("scipy.optimize")
    halves = 0
    for seed in range(240):
        true, pred = _random_pair(seed)
        ap, tp, fp, fn = _assert_same(true, pred, seed)
        if true.max() and pred.max():
            iou = rr.iou_matrix(true, pred)
            halves += int(((iou == 0.5).sum(axis=1) == 2).any() or ((iou == 0.5).sum(axis=0) == 2).any())
    assert halves >= 20  # labels with two candidates at exactly 0.5 do occur


def test_rule_on_constructed_cases():
    pytest.importorskip("scipy.optimize")
    true = np.zeros((4, 8), np.int64)
    true[:, :4] = 1
    true[:, 4:] = 2
    split = true.copy()
    split[:2, :4] = 3  # label 1 in two exact halves: two candidates at IoU 0.5, one match
    ap, tp, fp, fn = _assert_same(true, split, "half split")
    assert tp.tolist() == [2, 1, 1, 1, 1, 1] and fp[0] == 1 and fn[0] == 0
    ap, tp, fp, fn = _assert_same(split, true, "half split, the other way round")
    assert tp[0] == 2 and fp[0] == 0 and fn[0] == 1
    ap, tp, fp, fn = _assert_same(true, true, "identical")
    assert ap.tolist() == [1.0] * 6 and tp.tolist() == [2] * 6
    other = np.zeros_like(true)
    other[0, 0] = 1
    disjoint_true = true.copy()
    disjoint_true[0, 0] = 0
    ap, tp, fp, fn = _assert_same(disjoint_true, other, "disjoint")
    assert not tp.any() and fp.tolist() == [1] * 6 and fn.tolist() == [2] * 6 and not ap.any()
    ap, tp, fp, fn = _assert_same(true, np.zeros_like(true), "empty pred")
    assert not tp.any() and not fp.any() and fn.tolist() == [2] * 6 and not ap.any()
    ap, tp, fp, fn = _assert_same(np.zeros_like(true), true, "empty true")
    assert fp.tolist() == [2] * 6
    dots = np.arange(1, 33, dtype=np.int64).reshape(4, 8)  # one-pixel labels
    ap, tp, fp, fn = _assert_same(dots, dots, "one-pixel labels")
    assert tp.tolist() == [32] * 6
    ap, tp, fp, fn = _assert_same(dots, np.roll(dots, 1, axis=1), "one-pixel labels, renumbered")
    assert tp.tolist() == [32] * 6
    pairs = np.repeat(np.arange(1, 17, dtype=np.int64), 2).reshape(4, 8)  # two-pixel labels over one-pixel labels
    ap, tp, fp, fn = _assert_same(pairs, dots, "one-pixel halves")
    assert tp.tolist() == [16, 0, 0, 0, 0, 0]


def test_thresholds_below_one_half_are_refused():
    from arcadia_microscopy_tools_amd import metrics

    true = np.ones((2, 2), np.int64)
    rel = rr.relation(true, true, 1)
    for bad in ((0.49,), (0.5, 0.25), 0.0, (float("nan"),)):
        with pytest.raises(ValueError, match="below 0.5"):
            metrics.average_precision_from_relations(rel, rel, bad)
        with pytest.raises(ValueError, match="below 0.5"):
            metrics.average_precision(true, true, bad)  # refused before anything touches a device
    ap, tp, fp, fn = metrics.average_precision_from_relations(rel, rel, 0.5)
    assert ap.tolist() == [1.0] and tp.tolist() == [1]
