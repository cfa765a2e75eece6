"""The rule ``expand_labels`` implements, checked on the host: the separable evaluation against a brute-force search
and against scikit-image's expression on scipy's feature transform, the integer distance bound, and the validation
of ``operations.expand_labels`` (which needs no device)."""
import numpy as np
import pytest

import expand_labels_reference as ref
from arcadia_microscopy_tools_amd import hipops, operations

DISTANCES = ref.DISTANCES + (200,)  # the last one is larger than the scenes
SCENES = [((72, 90), 40, seed) for seed in range(8)] + [((1, 1), 1, 8), ((1, 70), 3, 9), ((70, 1), 3, 10), ((33, 65), 12, 11)]


@pytest.mark.parametrize("shape,n_discs,seed", SCENES)
def test_two_pass_equals_brute_force_and_scipy(shape, n_discs, seed):
    labels = ref.disc_scene(shape, n_discs, seed, max_label=None if seed % 2 else 5000)
    d2, nearest, tied = ref.nearest_two_pass(labels)
    bd2, bnearest, btied = ref.nearest_brute_force(labels)
    assert np.array_equal(d2, bd2) and np.array_equal(nearest, bnearest) and np.array_equal(tied, btied)
    assert np.array_equal(nearest[labels != 0], labels[labels != 0]) and not tied[labels != 0].any()
    for distance in DISTANCES:
        ours = ref.apply_bound(labels, d2, nearest, distance)
        assert np.array_equal(ours, ref.apply_bound(labels, bd2, bnearest, distance)), distance
        theirs = ref.expand_scipy(labels, distance)
        assert ours.dtype == theirs.dtype
        assert np.array_equal(ours != 0, theirs != 0), distance           # support: every pixel
        assert np.array_equal(ours[~tied], theirs[~tied]), distance        # label: every untied pixel
        grown_ties = tied & (ours != 0)                                    # tied pixels: the smallest label rule
        assert np.array_equal(ours[grown_ties], bnearest[grown_ties]), distance


def test_scenes_hold_ties_where_scipy_differs():
    """The comparison above is not vacuous: the scenes contain tied pixels, and scipy labels some of them otherwise."""
    n_tied = n_other = 0
    for shape, n_discs, seed in SCENES[:8]:
        labels = ref.disc_scene(shape, n_discs, seed, max_label=None if seed % 2 else 5000)
        d2, nearest, tied = ref.nearest_two_pass(labels)
        ours = ref.apply_bound(labels, d2, nearest, 12)
        theirs = ref.expand_scipy(labels, 12)
        n_tied += int((tied & (ours != 0)).sum())
        n_other += int((ours != theirs).sum())
    assert n_tied > 100 and n_other > 0


@pytest.mark.parametrize("distance", DISTANCES + (0.999999, 1.0000001, 10 ** 0.5, np.nextafter(3.0, 0), 31.99))
def test_nmax_is_the_largest_n_whose_root_is_within_the_distance(distance):
    want = ref.nmax_by_enumeration(distance, 50000)
    assert ref.nmax_of(distance) == want
    assert hipops.expand_nmax(distance) == want


def test_nmax_of_huge_and_odd_distances():
    assert hipops.expand_nmax(float("nan")) == -1 and hipops.expand_nmax(-0.0) == 0
    assert hipops.expand_nmax(1e300) >= 2 ** 31 and hipops.expand_nmax(float("inf")) >= 2 ** 31
    assert hipops.expand_nmax(46341) == 46341 ** 2


def test_validation_needs_no_device(monkeypatch):
    def no_device():
        raise AssertionError("the device was touched")

    monkeypatch.setattr(operations, "get_context", no_device)
    with pytest.raises(ValueError, match="2D"):
        operations.expand_labels(np.zeros((2, 8, 8), np.int64), 3)
    with pytest.raises(ValueError, match="2D"):
        operations.expand_labels(np.zeros(8, np.int32), 3)
    with pytest.raises(ValueError, match="non-negative"):
        operations.expand_labels(np.array([[0, -1], [2, 0]], np.int32), 1)
    with pytest.raises(ValueError, match="2\\*\\*31 - 2"):
        operations.expand_labels(np.array([[0, 2 ** 31 - 1]], np.int64), 1)
    with pytest.raises(TypeError, match="bool or integer"):
        operations.expand_labels(np.zeros((4, 4), np.float64), 1)
    empty = operations.expand_labels(np.zeros((0, 5), np.uint16), 2)
    assert empty.shape == (0, 5) and empty.dtype == np.uint16


def test_expand_labels_is_a_device_operator():
    from arcadia_microscopy_tools_amd.pipeline import ImageOperation, is_device_operator

    assert is_device_operator(operations.expand_labels)
    assert ImageOperation(operations.expand_labels, distance=3).on_device
