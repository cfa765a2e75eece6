"""The case list of tests/perimeter_cases.py on the CPU: a numpy restatement of the bit formulas of ``rp_perimeter_rows``
(amt_props.hip) -- row words of 32 columns, carries from the words left and right, bit-sliced neighbour sums -- gives the
oracle's three class counts on every case, and the cases together hold every 3 x 3 code that skimage weights and some
that it does not: the GPU test cannot pass on trivial content."""
import numpy as np
import pytest

import perimeter_cases as pc

M32 = 0xFFFFFFFF


def _row_words(img):
    """words[y][k] = the columns 32 k .. 32 k + 31 of row y as an integer, bit j = column 32 k + j."""
    h, w = img.shape
    nw = (w + 31) // 32
    padded = np.zeros((h, nw * 32), np.uint64)
    padded[:, :w] = img
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    return (padded.reshape(h, nw, 32) * weights).sum(axis=2).astype(np.uint64).tolist(), nw


def _sum4(p, q, r, t):
    x1, c1, x2, c2 = p ^ q, p & q, r ^ t, r & t
    return x1 ^ x2, c1 ^ c2 ^ (x1 & x2), c1 & c2


def bit_formula_counts(img):
    """(C1, C2, C3) of one binary image by the formulas of the device: m zero outside the box, B = m & ~(up & down &
    west & east), a / d = bit-sliced sums of the border neighbours across an edge / a corner."""
    words, nw = _row_words(np.asarray(img, bool))
    h = len(words)

    def m(y, k):
        return words[y][k] if 0 <= y < h and 0 <= k < nw else 0

    def west(f, y, k):  # the value of the column to the left, with the carry from the word to the left
        return ((f(y, k) << 1) & M32) | (f(y, k - 1) >> 31)

    def east(f, y, k):
        return (f(y, k) >> 1) | ((f(y, k + 1) & 1) << 31)

    def B(y, k):
        return m(y, k) & ~(m(y - 1, k) & m(y + 1, k) & west(m, y, k) & east(m, y, k)) & M32

    counts = [0, 0, 0]
    for y in range(h):
        for k in range(nw):
            a0, a1, a2 = _sum4(B(y - 1, k), B(y + 1, k), west(B, y, k), east(B, y, k))
            d0, d1, d2 = _sum4(west(B, y - 1, k), east(B, y - 1, k), west(B, y + 1, k), east(B, y + 1, k))
            ctr = B(y, k)
            a_is1, d_is2 = a0 & ~a1 & ~a2, d1 & ~d0 & ~d2
            counts[0] += bin(ctr & a1 & ~a2 & ~d2 & ~(d1 & d0) & M32).count("1")
            counts[1] += bin(ctr & ((~(a0 | a1 | a2) & d_is2) | (a_is1 & d1 & d0)) & M32).count("1")
            counts[2] += bin(ctr & a_is1 & ((d0 & ~d1 & ~d2) | d_is2) & M32).count("1")
    return tuple(counts)


@pytest.mark.parametrize("name", sorted(pc.perimeter_cases()))
def test_bit_formulas_give_the_oracles_class_counts(name):
    planes, mx = pc.perimeter_cases()[name]
    for plane, exp in zip(planes, pc.expected_of(name)):
        lab = pc.clean(plane, mx)
        for i in np.nonzero(exp["present"])[0]:
            y0, x0, y1, x1 = exp["bbox"][i]
            got = bit_formula_counts(lab[y0:y1 + 1, x0:x1 + 1] == i + 1)
            assert got == tuple(exp["counts"][i]), (name, i + 1)
        # the class weights applied to the counts are the oracle's perimeter (up to the order of its float sum)
        np.testing.assert_allclose(exp["perimeter"], exp["oracle_perimeter"], rtol=1e-13, atol=0)


def test_cases_hold_every_weighted_code_and_some_unweighted_ones():
    hist = np.zeros(50, np.int64)
    for name in pc.perimeter_cases():
        for exp in pc.expected_of(name):
            hist += exp["hist"]
    weighted = pc.C1_CODES + pc.C2_CODES + pc.C3_CODES
    assert all(hist[c] > 0 for c in weighted), {c: int(hist[c]) for c in weighted}
    unweighted = [c for c in np.nonzero(hist)[0] if c not in weighted]
    assert len(unweighted) >= 3, unweighted


def test_band_and_wide_cases_stand_on_the_documented_constants():
    assert pc.RP_WIDE <= 16384
    for w in pc.BAND_WIDTHS:
        b = pc.band_rows(w)
        planes, _ = pc.perimeter_cases()[f"bands_w{w}"]
        heights = sorted(int(np.ptp(np.nonzero(p.any(axis=1))[0])) + 1 for p in planes)
        assert heights == sorted((b - 1, b, b + 1, 2 * b + 1, 3 * b + 7)) and heights[-1] > 3 * b
    over, _ = pc.perimeter_cases()["wide_over"]
    under, _ = pc.perimeter_cases()["wide_under"]
    assert int(np.ptp(np.nonzero(over[0].any(axis=0))[0])) + 1 > pc.RP_WIDE
    assert int(np.ptp(np.nonzero(under[0].any(axis=0))[0])) + 1 == pc.RP_WIDE


def test_box_cases_reach_their_switches():
    cases = pc.box_cases()
    assert {planes.shape[2] for planes, _, _ in cases.values()} >= set(pc.BOX_WIDTHS)
    assert {mis for _, _, mis in cases.values()} == {0, 1, 2, 3}
    for name, (planes, mx, _) in cases.items():
        boxes = pc.expected_boxes(planes, mx)
        H, W = planes.shape[1:]
        assert (boxes[..., 2] == H - 1).any() and (boxes[..., 3] == W - 1).any(), name
