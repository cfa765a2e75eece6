"""``cellpose_hip.resolve_normalize``: CellposeModel.eval's ``normalize=`` / ``invert=`` options resolved on the host
(no GPU, no native library)."""
import numpy as np
import pytest

from arcadia_microscopy_tools_amd import cellpose_hip as ch


def test_options_are_eval_kwargs_of_the_route():
    assert "normalize" in ch._EVAL_KWARGS and "invert" in ch._EVAL_KWARGS


def test_off_by_default_and_when_asked():
    for off in (False, None, {"normalize": False}, {"normalize": False, "percentile": (2, 98)}):
        assert ch.resolve_normalize(off, False, 2) is None


def test_true_is_the_default_percentiles():
    plan = ch.resolve_normalize(True, False, 3)
    assert plan.percentile == (1.0, 99.0) and plan.lowhigh is None and plan.invert is False
    assert ch.resolve_normalize({}, False, 1) == plan
    assert ch.resolve_normalize({"normalize": True, "percentile": None, "lowhigh": None}, False, 1) == plan


def test_every_dict_key_is_recognised():
    plan = ch.resolve_normalize({"normalize": True, "lowhigh": None, "percentile": (0.5, 99.5), "invert": False,
                                 "norm3D": False, "sharpen_radius": 0, "smooth_radius": 0, "tile_norm_blocksize": 0,
                                 "tile_norm_smooth3D": 3}, False, 2)
    assert plan.percentile == (0.5, 99.5) and plan.lowhigh is None and plan.invert is False
    # norm3D / tile_norm_smooth3D are accepted and change nothing on a 2-D image
    assert ch.resolve_normalize({"norm3D": True, "tile_norm_smooth3D": 1, "percentile": (0.5, 99.5)}, False, 2) == plan
    assert ch.resolve_normalize({"percentile": [0, 100]}, False, 1).percentile == (0.0, 100.0)


def test_invert_is_ored():
    assert ch.resolve_normalize(True, True, 1).invert is True
    assert ch.resolve_normalize({"invert": True}, False, 1).invert is True
    assert ch.resolve_normalize({"invert": True}, True, 1).invert is True
    assert ch.resolve_normalize({"invert": False}, True, 1).invert is True
    assert ch.resolve_normalize({"invert": False}, False, 1).invert is False


def test_lowhigh_shared_and_per_channel():
    plan = ch.resolve_normalize({"lowhigh": (100, 4000.5)}, False, 3)
    assert plan.percentile is None and plan.lowhigh.dtype == np.float32 and plan.lowhigh.shape == (3, 2)
    assert plan.lowhigh.flags["C_CONTIGUOUS"]
    assert np.array_equal(plan.lowhigh, np.array([[100, 4000.5]] * 3, np.float32))
    per = [[0, 1], [10.25, 5000], [-3, 0.1]]
    plan = ch.resolve_normalize({"lowhigh": per, "invert": True}, False, 3)
    assert np.array_equal(plan.lowhigh, np.array(per, np.float32)) and plan.invert is True
    # one channel: a single pair in either spelling
    for one in ((5, 6), [(5, 6)]):
        assert np.array_equal(ch.resolve_normalize({"lowhigh": one}, False, 1).lowhigh, np.array([[5, 6]], np.float32))
    # values are rounded to float32 once, here
    plan = ch.resolve_normalize({"lowhigh": (0.1, 1 / 3)}, False, 1)
    assert np.array_equal(plan.lowhigh, np.array([[np.float32(0.1), np.float32(1 / 3)]], np.float32))


def test_unknown_key_is_a_value_error_naming_it():
    with pytest.raises(ValueError, match="tile_norm"):
        ch.resolve_normalize({"tile_norm": 64}, False, 1)
    with pytest.raises(ValueError, match="percentiles"):
        ch.resolve_normalize({"percentiles": (1, 99), "invert": True}, False, 1)


@pytest.mark.parametrize("key", ["sharpen_radius", "smooth_radius", "tile_norm_blocksize"])
def test_unimplemented_stage_is_a_type_error_naming_it(key):
    with pytest.raises(TypeError, match=key):
        ch.resolve_normalize({key: 4}, False, 1)
    with pytest.raises(TypeError, match=key):  # refused even when normalisation itself is off: never ignored
        ch.resolve_normalize({key: 1.5, "normalize": False}, False, 1)
    assert ch.resolve_normalize({key: 0}, False, 1) == ch.resolve_normalize(True, False, 1)


def test_lowhigh_with_percentile_is_refused():
    with pytest.raises(ValueError, match="lowhigh.*percentile"):
        ch.resolve_normalize({"lowhigh": (0, 1), "percentile": (1, 99)}, False, 1)


@pytest.mark.parametrize("bad", [(-1, 99), (1, 100.5), (50, 50), (99, 1), (1,), (1, 50, 99), "ab", 5])
def test_percentile_range(bad):
    with pytest.raises(ValueError, match="percentile"):
        ch.resolve_normalize({"percentile": bad}, False, 1)


@pytest.mark.parametrize("bad,channels", [((1, 1), 1), ((2, 1), 2), ((0, 1e-3), 1), ([[0, 1], [5, 5.0005]], 2),
                                          ([[0, 1], [0, 1], [0, 1]], 2), ((0, 1, 2), 3), ([[0, 1]], 2),
                                          ((0, float("nan")), 1), ("lo", 1)])
def test_lowhigh_shape_and_range(bad, channels):
    with pytest.raises(ValueError, match="lowhigh"):
        ch.resolve_normalize({"lowhigh": bad}, False, channels)


def test_invert_without_normalisation_is_refused():
    for off in (False, None, {"normalize": False}):
        with pytest.raises(ValueError, match="invert"):
            ch.resolve_normalize(off, True, 1)
    with pytest.raises(ValueError, match="invert"):
        ch.resolve_normalize({"normalize": False, "invert": True}, False, 1)


@pytest.mark.parametrize("bad", ["yes", 1, 0.5, (1, 99)])
def test_normalize_must_be_bool_or_dict(bad):
    with pytest.raises(ValueError, match="bool or a dict"):
        ch.resolve_normalize(bad, False, 1)


def test_classical_backend_refuses_the_option_without_a_gpu():
    """backend='classical' refuses every eval option before it touches the device, ``normalize`` included."""
    from arcadia_microscopy_tools_amd.model import SegmentationModel

    img = np.zeros((32, 32), np.uint16)
    with pytest.raises(RuntimeError, match="takes no CellposeModel.eval options"):
        SegmentationModel(backend="classical").segment(img, normalize=True)
