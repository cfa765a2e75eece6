"""Per-cell channel colocalisation, the parts that need no device: the test-side reference itself (against numpy and
scipy where they define the same number), the degenerate rules of the definition table, the key list and the argument
checks of ``SegmentationMask.cell_colocalization``."""
import math

import numpy as np
import pytest

import colocalization_reference as ref
from arcadia_microscopy_tools_amd import _hip, hipops, segment
from arcadia_microscopy_tools_amd.channels import BRIGHTFIELD, DAPI, FITC, TRITC
from arcadia_microscopy_tools_amd.masks import SegmentationMask

NUC_CHANNELS = (BRIGHTFIELD, DAPI, FITC, TRITC)


def test_columns_are_exported_in_the_contract_order():
    assert _hip.COLOC_COLS == ("pearson", "overlap", "m1", "m2", "intersection1", "intersection2") == ref.COLS
    assert _hip.COLOC_NCOLS == 6
    assert "amt_colocalization" in _hip.exported_names()


def test_exact_reference_against_numpy_and_scipy_on_the_nuclei(golden):
    from scipy import stats

    g = golden("props_ext")
    labels, fov = g["nuc__labels"], g["nuc__fov"]
    k = int(labels.max())
    assert k == 22 and fov.shape[0] == 4 and fov.dtype == np.uint16
    pairs = ref.all_pairs(4)
    table = ref.table(labels, fov, k)
    assert table.shape == (22, 6, 6) and not np.isnan(table).any()  # no degenerate cell in this fixture
    worst = 0.0
    for lab in range(1, k + 1):
        sel = labels == lab
        for p, (i, j) in enumerate(pairs):
            a, b = fov[i][sel].astype(np.float64), fov[j][sel].astype(np.float64)
            for other in (np.corrcoef(a, b)[0, 1], stats.pearsonr(a, b)[0]):
                worst = max(worst, abs(table[lab - 1, p, 0] - other))
            # the remaining columns in plain float64 (sums of integers below 2^53 are exact there)
            assert table[lab - 1, p, 1] == pytest.approx((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()), rel=1e-14)
            assert table[lab - 1, p, 2] == a[b > 0].sum() / a.sum()
            assert table[lab - 1, p, 3] == b[a > 0].sum() / b.sum()
    print(f"exact pearson vs np.corrcoef / scipy.stats.pearsonr: largest difference {worst:.3g}")
    assert worst <= 1e-12
    # float samples through the two-pass form agree with the exact form too
    ftable = ref.table(labels, fov.astype(np.float64), k)
    assert np.abs(ftable - table).max() <= 1e-12


def test_degenerate_rules_of_the_definition_table():
    nan = float("nan")
    same = lambda got, want: all((math.isnan(g) and math.isnan(w)) or g == w for g, w in zip(got, want))  # noqa: E731
    rng = np.random.default_rng(0)
    a = rng.integers(1, 5000, 50)
    for one in (ref.exact_pair, ref.float_pair):
        # a constant channel: Pearson NaN, the others defined
        got = one(a, np.full(50, 9), 0, 0)
        assert math.isnan(got[0]) and got[1] > 0 and got[2:] == (1.0, 1.0, 1.0, 1.0)
        # an all-zero channel: constant, so Pearson NaN; overlap 0 / 0 = NaN; its own sums are 0 -> m2 = 0
        assert same(one(a, np.zeros(50, np.int64), 0, 0), (nan, nan, 0.0, 0.0, 0.0, 0.0))
        # one pixel: both channels constant
        assert same(one([7], [9], 0, 0), (nan, 7 * 9 / math.sqrt(49 * 81), 1.0, 1.0, 1.0, 1.0))
        # no positives: thresholds above every value
        got = one(a, a[::-1], 5000, 5000)
        assert not math.isnan(got[0]) and got[2:] == (0.0, 0.0, 0.0, 0.0)
        # "positive" is strictly greater than the threshold
        assert one([1, 2, 3], [3, 2, 1], 2, 1)[2:] == (3 / 6, 1 / 6, 0.0, 0.0)
        assert one([1, 2, 3], [3, 2, 5], 1, 2)[2:] == (4 / 6, 7 / 10, 1 / 2, 1 / 2)
        # no pixel at all
        assert same(one([], [], 0, 0), (nan, nan, 0.0, 0.0, 0.0, 0.0))
    # perfectly (anti)correlated integers give exactly +-1 in the exact form
    assert ref.exact_pair([1, 2, 3, 4], [2, 4, 6, 8], 0, 0)[0] == 1.0
    assert ref.exact_pair([1, 2, 3, 4], [8, 6, 4, 2], 0, 0)[0] == -1.0
    # the scene the device tests use holds each of these cells
    labels, stack, what = ref.degenerate_scene()
    table = ref.table(labels, stack, 7, thresholds=100)
    assert np.isnan(table[0, 0, 0]) and not np.isnan(table[0, 1, 0])  # label 1: pairs with channel 1 only
    assert np.isnan(table[1, 1, 1]) and table[1, 1, 3] == 0.0  # label 2, pair (0, 2)
    assert np.isnan(table[2, :, 0]).all() and not np.isnan(table[2, :, 1]).any()  # one pixel
    assert (table[3, :, 2:] == 0).all() and not np.isnan(table[3, :, :2]).any()  # no positives
    for row in (table[4], table[5]):  # every channel zero; absent
        assert np.isnan(row[:, :2]).all() and (row[:, 2:] == 0).all()
    assert not np.isnan(table[6]).any()


def test_colocalization_keys():
    names = ["BRIGHTFIELD", "DAPI", "FITC", "TRITC"]
    keys = segment.colocalization_keys(names)
    assert len(keys) == 36 and len(set(keys)) == 36
    assert keys[:6] == [f"{m}_brightfield_dapi" for m in _hip.COLOC_COLS]
    assert keys[-6:] == [f"{m}_fitc_tritc" for m in _hip.COLOC_COLS]
    assert "pearson_fitc_tritc" in keys and "pearson_tritc_fitc" not in keys
    # channel objects, and pairs by object, name or index, in the order given
    assert segment.colocalization_keys(NUC_CHANNELS) == keys
    assert segment.colocalization_keys(NUC_CHANNELS, [(TRITC, FITC), ("dapi", 3)]) == (
        [f"{m}_tritc_fitc" for m in _hip.COLOC_COLS] + [f"{m}_dapi_tritc" for m in _hip.COLOC_COLS])
    assert segment.colocalization_pairs(NUC_CHANNELS, [(TRITC, FITC)]) == [(3, 2)]
    with pytest.raises(ValueError):
        segment.colocalization_keys(["DAPI"])
    with pytest.raises(ValueError):
        segment.colocalization_keys(names, [("DAPI", "DAPI")])
    with pytest.raises(ValueError):
        segment.colocalization_keys(names, [("DAPI", "CY5")])
    with pytest.raises(ValueError):
        segment.colocalization_keys(names, [(0, 4)])
    with pytest.raises(ValueError):
        segment.colocalization_keys(names, [])
    with pytest.raises(TypeError):
        segment.colocalization_keys(names, ["DAPI"])


def test_hipops_pair_lists():
    assert hipops.colocalization_pairs(3).tolist() == [[0, 1], [0, 2], [1, 2]]
    got = hipops.colocalization_pairs(5, [(4, 0), (1, 2)])
    assert got.dtype == np.int32 and got.tolist() == [[4, 0], [1, 2]]
    for bad in ([(0, 0)], [(0, 5)], [(-1, 2)], []):
        with pytest.raises(ValueError):
            hipops.colocalization_pairs(5, bad)
    for bad in ([(0, 1, 2)], [(0.5, 1)], [("a", 1)]):
        with pytest.raises(TypeError):
            hipops.colocalization_pairs(5, bad)


def test_cell_colocalization_argument_errors_need_no_device(golden):
    g = golden("props_ext")
    labels, fov = g["nuc__labels"], g["nuc__fov"]
    with pytest.raises(ValueError, match="at least two intensity images"):
        SegmentationMask(labels, remove_edge_cells=False).cell_colocalization()
    with pytest.raises(ValueError, match="at least two intensity images"):
        SegmentationMask(labels, {DAPI: fov[1]}, remove_edge_cells=False).cell_colocalization()
    mask = SegmentationMask(labels, {DAPI: fov[1], FITC: fov[2]}, remove_edge_cells=False)
    with pytest.raises(ValueError):
        mask.cell_colocalization(pairs=[(DAPI, TRITC)])  # no image for TRITC
    with pytest.raises(ValueError):
        mask.cell_colocalization(pairs=[(DAPI, DAPI)])
    with pytest.raises(ValueError):
        mask.cell_colocalization(pairs=[])
    with pytest.raises(TypeError):
        mask.cell_colocalization(pairs=[DAPI])
    with pytest.raises(ValueError):
        mask.cell_colocalization(thresholds={TRITC: 5})
    with pytest.raises(ValueError):
        mask.cell_colocalization(thresholds={DAPI: "li"})
    with pytest.raises(TypeError):
        mask.cell_colocalization(thresholds={DAPI: [1, 2]})
    with pytest.raises(TypeError):
        mask.cell_colocalization(thresholds="otsu")
    with pytest.raises(TypeError):
        mask.cell_colocalization(thresholds=[1, 2])
    assert "_labels_device" not in mask.__dict__  # every check came before the first device call
