"""The perimeter count of ``rp_label_kernel`` and the box pass ``rp_boxes_kernel`` on the cases of
tests/perimeter_cases.py: boxes and perimeter exactly as the oracle (oracle/regionprops.py) gives them, area and centroid
as before."""
import numpy as np
import pytest

import perimeter_cases as pc
from arcadia_microscopy_tools_amd import _hip, hipops

pytestmark = pytest.mark.gpu

COL = {k: i for i, k in enumerate(_hip.RP_COLS)}


def _ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


@pytest.mark.parametrize("name", sorted(pc.perimeter_cases()))
def test_regionprops_boxes_and_perimeter_equal_the_oracle(name):
    planes, mx = pc.perimeter_cases()[name]
    table = hipops.regionprops(_ctx().asarray(np.ascontiguousarray(planes, np.int32)), mx).numpy()
    assert table.shape == (len(planes), mx, _hip.RP_NCOLS)
    for t, exp in zip(table, pc.expected_of(name)):
        here = exp["present"]
        assert not t[~here][:, [COL["area"], COL["perimeter"], COL["bbox-0"], COL["bbox-2"]]].any()
        if not here.any():
            continue
        box = exp["bbox"][here]
        for j, off in enumerate((0, 0, 1, 1)):  # the table's maxima are exclusive
            assert np.array_equal(t[here, COL[f"bbox-{j}"]], box[:, j] + off), (name, j)
        got = t[here, COL["perimeter"]]
        assert np.array_equal(got, exp["perimeter"][here]), (name, got - exp["perimeter"][here])
        assert np.array_equal(t[here, COL["area"]], exp["area"][here]), name
        for j in range(2):
            np.testing.assert_allclose(t[here, COL[f"centroid-{j}"]], exp["centroid"][here, j], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", sorted(pc.box_cases()))
def test_box_pass_equals_the_oracle(name):
    planes, mx, mis = pc.box_cases()[name]
    ctx = _ctx()
    flat = np.concatenate([np.zeros(mis, np.int32), np.ascontiguousarray(planes, np.int32).ravel()])
    dev = ctx.asarray(flat)[mis:].reshape(planes.shape)
    assert dev.ptr % 16 == 4 * mis
    want = pc.expected_boxes(planes, mx)
    assert np.array_equal(hipops.label_bboxes(dev, mx), want), name
    # the same boxes through the morphology table, which takes them from the same pass
    t = hipops.regionprops(dev, mx).numpy()
    here = want[..., 2] >= want[..., 0]
    got = np.stack([t[..., COL["bbox-0"]], t[..., COL["bbox-1"]], t[..., COL["bbox-2"]] - 1, t[..., COL["bbox-3"]] - 1], -1)
    assert np.array_equal(got[here], want[here]), name
