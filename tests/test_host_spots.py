"""Spot detection without a GPU: the numpy reference against a hand-worked example and its own invariants (spacing,
capacity, the lattice that reaches the capacity), the planted-spot fixture on the reference alone, the header's statement
of the four codes, every refusal of the C ABI that needs no device (null context), the bindings' refusals before any
device access, and the argument checks of ``peak_local_max`` / ``detect_spots``.  The local-maximum rule is this project's
own: nothing here claims parity with scikit-image on plateaus."""
import os
import re

import numpy as np
import pytest

import spots_cases as cases
import spots_reference as ref
from arcadia_microscopy_tools_amd import _hip, hipops, operations, segment
from arcadia_microscopy_tools_amd.device import DeviceArray
from arcadia_microscopy_tools_amd.pipeline import is_device_operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "amt_hip.h")).read()

# the hand-worked plane: a 2 x 2 plateau of 5, a ridge of three 7s, single peaks on the border and inside
HAND = np.array([[0, 0, 0, 0, 0, 0, 0],
                 [0, 5, 5, 0, 0, 0, 3],
                 [0, 5, 5, 0, 2, 0, 0],
                 [0, 0, 0, 0, 0, 0, 0],
                 [4, 0, 0, 7, 7, 7, 0],
                 [0, 0, 0, 0, 0, 0, 0],
                 [0, 0, 9, 0, 0, 0, 9]], np.uint16)


def _marks(a, r, t=0.0, b=0):
    return [tuple(int(v) for v in p) for p in np.argwhere(ref.local_maxima(a, r, t, b))]


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_reference_gives_the_hand_results():
    # r = 1.  The plateau yields its first pixel (1, 1): (1, 2) ties with its left neighbour, (2, 1) and (2, 2) with a pixel
    # of the row above -- all three fail a STRICT test.  The ridge yields (4, 3); (4, 4) and (4, 5) tie to the left.
    assert _marks(HAND, 1) == [(1, 1), (1, 6), (2, 4), (4, 0), (4, 3), (6, 2), (6, 6)]
    # r = 2: the 2 at (2, 4) sees the 5s, the 4 at (4, 0) the 5 at (2, 1), every 7 one of the 9s
    assert _marks(HAND, 2) == [(1, 1), (1, 6), (6, 2), (6, 6)]
    # the border comes last; the threshold is strict: 4 is not above 4
    assert _marks(HAND, 1, b=1) == [(1, 1), (2, 4), (4, 3)]
    assert _marks(HAND, 1, t=4.0) == [(1, 1), (4, 3), (6, 2), (6, 6)]
    assert _marks(HAND, 1, t=9.0) == []
    # a plateau whose first pixel lies in the border yields nothing there
    edge = np.zeros((5, 5), np.uint16)
    edge[0:2, 0:2] = 3
    assert _marks(edge, 1) == [(0, 0)] and _marks(edge, 1, b=1) == []
    # -0.0 equals +0.0: one plateau
    z = np.full((3, 3), -1.0)
    z[1, 0:2] = [-0.0, 0.0]
    assert _marks(z, 1, t=-0.5) == [(1, 0)]
    # the float64 plane gives what the uint16 plane gives
    assert _marks(HAND.astype(np.float64), 1) == _marks(HAND, 1)
    # the list: count, raster indices, -1; truncated it keeps the true count
    assert ref.mask_list(ref.local_maxima(HAND, 2), 6).tolist() == [4, 8, 13, 44, 48, -1, -1]
    assert ref.mask_list(ref.local_maxima(HAND, 2), 3).tolist() == [4, 8, 13, 44]
    # the parabola: (1, 3, 1) is centred; (1, 3, 2) leans towards the 2: den = -3, 0.5 * (1 - 2) / -3 = 1 / 6;
    # not concave: 0; a vertex past half a pixel is clamped
    assert ref.parabola_offset(1, 3, 1) == 0.0 and ref.parabola_offset(1, 3, 2) == (0.5 * -1.0) / -3.0
    assert ref.parabola_offset(3, 1, 3) == 0.0 and ref.parabola_offset(2, 2, 2) == 0.0
    assert ref.parabola_offset(0, 10, 9.9) == 0.5 * (0 - 9.9) / ((0 - 10.0) + (9.9 - 10))
    assert ref.parabola_offset(0, 1, 2) == 0.0 and ref.parabola_offset(5, 5.5, 0) == (0.5 * 5.0) / -6.0
    assert ref.parabola_offset(0, 1, 1.9) == 0.5
    # the measure row of the 9 at (6, 2), k = 1: the window is clipped to two rows; the frame reaches rows 3 .. 6
    row = ref.spot_measure(HAND, np.array([1, 44], np.int32), 1)[0]
    assert row.tolist() == [9.0, 0.0, 0.0, 9.0, 6.0, 4.0 + 7.0 + 7.0 + 7.0, 4.0 * 6 - 6.0]
    assert np.isnan(ref.spot_measure(HAND, np.array([0, 44], np.int32), 1)).all()
    assert ref.take_at(HAND, np.array([2, 44, 8, -1], np.int32)).tolist() == [9, 5, 0]


@pytest.mark.parametrize("shape", [(1, 9), (5, 3), (37, 53), (64, 64), (70, 130)])
@pytest.mark.parametrize("r", [1, 2, 5])
def test_reference_spacing_and_capacity_on_tied_planes(shape, r):
    for seed, top in ((1, 2), (2, 6), (3, 1)):
        a = np.random.default_rng(seed).integers(0, top, size=shape).astype(np.uint16)
        pts = np.argwhere(ref.local_maxima(a, r, -1.0, 0))
        assert len(pts) >= 1  # the first pixel holding the maximum is always marked
        assert len(pts) <= ref.spot_capacity(shape[0], shape[1], r) == hipops.spot_capacity(shape[0], shape[1], r)
        if len(pts) > 1:
            d = np.abs(pts[:, None, :] - pts[None, :, :]).max(axis=2)
            assert d[np.triu_indices(len(pts), 1)].min() > r
        # every marked pixel is a maximum of its window
        for y, x in pts[:50]:
            assert a[y, x] == a[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].max()


@pytest.mark.parametrize("r", [1, 2, 5, 15])
def test_a_lattice_reaches_the_capacity_exactly(r):
    for shape in ((37, 53), (64, 64), (1, 9), (16 * (r + 1), 3 * (r + 1) + 1)):
        a = np.zeros(shape, np.uint16)
        a[::r + 1, ::r + 1] = 100
        assert int(ref.local_maxima(a, r).sum()) == hipops.spot_capacity(shape[0], shape[1], r)
    for bad in (0, 16, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="min_distance"):
            hipops.spot_capacity(10, 10, bad)


def test_the_reference_alone_finds_the_planted_spots():
    """The fixture of tests/test_gpu_spots.py, on the CPU: exactly the planted spots, each within 0.25 px."""
    image, truth = cases.planted_plane()
    assert image.shape == (128, 128) and image.dtype == np.uint16 and len(truth) == 40
    d = np.hypot(*(truth[:, None, :] - truth[None, :, :]).transpose(2, 0, 1))
    assert d[np.triu_indices(40, 1)].min() >= 6 and truth.min() >= 6 and truth.max() <= 127 - 6
    table = ref.detect_spots(image, **cases.PLANTED_ARGS)
    assert len(table["row"]) == 40
    found = np.stack([table["y"], table["x"]], axis=1)
    nearest = np.hypot(*(found[:, None, :] - truth[None, :, :]).transpose(2, 0, 1))
    assert sorted(nearest.argmin(axis=1).tolist()) == list(range(40))  # one spot per planted centre, no extras
    print("planted spots: largest error", float(nearest.min(axis=1).max()), "median", float(np.median(nearest.min(axis=1))))
    assert nearest.min(axis=1).max() <= 0.25
    # the frame at distance 3 .. 4 still sees the spot's tail: 800 exp(-9 / 3.38) = 56 at its nearest pixels
    assert (table["intensity_net"] > 0).all() and (table["background_mean"] > 90).all() and (table["background_mean"] < 156).all()


def test_the_table_is_not_vacuous():
    table = {c["name"]: c for c in cases.cases()}
    assert len(table) == len(cases.cases())
    maxima = [c for c in table.values() if c["op"] == "maxima"]
    assert {c["a"].shape[1:] for c in maxima} >= set(cases.SHAPES) and {c["r"] for c in maxima} == {1, 2, 5, 15}
    assert {c["a"].dtype for c in maxima} == {np.dtype(np.uint16), np.dtype(np.float64)}
    for r in cases.RADII:  # at distance r only the first of two equal peaks survives, at r + 1 both do
        got = cases.reference(table[f"maxima seam pairs r {r}"])["mask"].sum(axis=(1, 2)).tolist()
        assert got == [1, 1, 1, 2, 2, 2], (r, got)
    assert cases.reference(table["maxima constant b 0"])["mask"].sum() == 1
    assert cases.reference(table["maxima constant b 1"])["mask"].sum() == 0
    assert [int(cases.reference(table[f"maxima corners b {b}"])["mask"].sum()) for b in (0, 1, 2)] == [9, 1, 1]
    # the 2 x 2 patch of +-0.0 is one plateau; the lone -0.0 is a peak of its own
    zeros = cases.reference(table["maxima signed zeros"])["mask"][0]
    assert zeros[10:12, 20:22].tolist() == [[1, 0], [0, 0]] and zeros[30, 40] == 1
    assert zeros.sum() > 20 and (table["maxima signed zeros"]["a"][0][zeros == 1] < 0).sum() == zeros.sum() - 2
    assert np.argwhere(cases.reference(table["maxima threshold equals a peak"])["mask"]).tolist() == [[0, 20, 30]]
    assert np.argwhere(cases.reference(table["maxima threshold equals a peak float64"])["mask"]).tolist() == [[0, 20, 30]]
    per_plane = cases.reference(table["maxima per-plane thresholds"])["mask"].sum(axis=(1, 2))
    assert per_plane[0] > per_plane[1] > per_plane[2] >= 0 and per_plane[1] > 0
    lists = [c for c in table.values() if c["op"] == "list"]
    assert {c["mask"].shape[2] for c in lists} >= set(cases.WIDTHS)
    kinds = set()
    for c in lists:
        for row in cases.reference(c)["list"]:
            cap = len(row) - 1
            kinds.add("equal" if row[0] == cap else "truncated" if row[0] > cap else "tail")
            assert (row[1 + min(row[0], cap):] == -1).all() and (row[1:1 + min(row[0], cap)] >= 0).all()
    assert kinds == {"equal", "truncated", "tail"}
    measured = [c for c in table.values() if c["op"] == "measure"]
    assert {c["k"] for c in measured} >= {0, 2, 15}
    valley = cases.reference(table["measure a minimum uint16"])["table"][0, 0]
    assert valley[1] == 0.0 and valley[2] == 0.0  # not concave: no offset
    peaks = cases.reference(table["measure maxima float64 k 2"])["table"][0]
    assert np.isnan(peaks[-3:]).all() and (np.abs(peaks[:-3, 1:3]) <= 0.5).all() and (peaks[:-3, 1:3] != 0).any()
    assert (cases.reference(table["measure maxima float64 k 2"])["bound"][0, :-3] > 0).all()
    assert cases.reference(table["measure 1 x 1"])["table"].tolist() == [[[9.0, 0.0, 0.0, 9.0, 1.0, 0.0, 0.0]]]


# ---- the header and the codes ---------------------------------------------------------------------------------------------
def test_header_defines_and_documents_the_codes():
    for name, value in (("AMT_RANK_LOCAL_MAXIMA", 15), ("AMT_RANK_MASK_LIST", 16), ("AMT_RANK_SPOT_MEASURE", 17),
                        ("AMT_RANK_TAKE_AT", 18), ("AMT_SPOT_NCOLS", 7), ("AMT_SPOT_MAX_RADIUS", 15),
                        ("AMT_SPOT_TILE_H", _hip.SPOT_TILE[0]), ("AMT_SPOT_TILE_W", _hip.SPOT_TILE[1])):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", HEADER, re.M), name
    for i, col in enumerate(_hip.SPOT_COLS):
        assert re.search(rf"^#define\s+AMT_SPOT_{col.upper()}\s+{i}\s*$", HEADER, re.M), col
    block = HEADER[:HEADER.index("int amt_rank_filter(")]
    block = block[block.rindex("/* grey erosion"):]
    for word in ("AMT_RANK_LOCAL_MAXIMA", "AMT_RANK_MASK_LIST", "AMT_RANK_SPOT_MEASURE", "AMT_RANK_TAKE_AT", "Chebyshev",
                 "raster order", "applied last", "ceil(H / (r+1)) * ceil(W / (r+1))", "first pixel in raster order",
                 "-0.0 equals +0.0", "unpinned offline", "np.flatnonzero", "true number", "clamped to [-0.5, 0.5]",
                 "den >= 0", "NaN throughout", "0 past the count", "no global float atomics", "nplanes == 0"):
        assert word in block, word


def test_python_constants_agree_with_the_header_and_the_reference():
    assert (_hip.RANK_LOCAL_MAXIMA, _hip.RANK_MASK_LIST, _hip.RANK_SPOT_MEASURE, _hip.RANK_TAKE_AT) == (15, 16, 17, 18)
    assert _hip.SPOT_COLS == ref.COLS and _hip.SPOT_NCOLS == 7 and _hip.SPOT_MAX_RADIUS == ref.MAX_RADIUS
    assert hipops.spot_tile() == _hip.SPOT_TILE
    for name in ("peak_local_max", "detect_spots"):
        assert is_device_operator(getattr(operations, name))
    assert segment.spot_keys("FITC") == ["spot_count_fitc", "spot_intensity_sum_fitc", "spot_intensity_mean_fitc"]
    assert "package's own" in hipops.local_maxima.__doc__ and "unpinned offline" in operations.peak_local_max.__doc__


def test_no_new_prototype():
    bare = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    names = re.findall(r"^(?:int|const char\s*\*)\s*(amt_\w+)\s*\(", bare, flags=re.M)
    assert len(names) == len(set(names)) == len(_hip._SIGS) and set(names) == set(_hip._SIGS)
    assert not [n for n in names if "spot" in n or "maxima" in n or "mask_list" in n or "take_at" in n]
    lib = _hip.load_library()
    for hidden in ("amt_local_maxima", "amt_mask_list", "amt_spot_measure", "amt_take_at", "amt_i_spots", "amt_i_spots_spans"):
        assert not hasattr(lib, hidden)


# ---- the C ABI with a null context ------------------------------------------------------------------------------------------
_BUF = np.zeros(1 << 16, np.uint8)
_A = (_BUF.ctypes.data + 255) & ~255   # in
_B = _A + (1 << 15)                    # out
_M = _A + (1 << 14)                    # minuend
THREE = np.ones((3, 3), np.uint8)
OPS = (15, 16, 17, 18)
DTYPES = {15: (_hip.U16, _hip.F64), 16: (_hip.U8,), 17: (_hip.U16, _hip.F64), 18: (_hip.U8, _hip.U16, _hip.I32, _hip.F64)}
ESIZE = {_hip.U8: 1, _hip.U16: 2, _hip.I32: 4, _hip.F64: 8}


def _call(op, *, dtype=None, fp=THREE, mode=3, cval=0.0, inp=None, out=None, minuend="default", H=4, W=4, nplanes=1):
    lib = _hip.load_library()
    fp = np.ascontiguousarray(fp, np.uint8)
    if dtype is None:
        dtype = DTYPES[op][0]
    if minuend == "default":
        minuend = _M if op in (17, 18) else None
    rc = lib.amt_rank_filter(None, _A if inp is None else inp, _B if out is None else out, dtype, nplanes, H, W,
                             fp.ctypes.data, fp.shape[0], fp.shape[1], op, mode, float(cval), minuend)
    return rc, lib.amt_last_error().decode()


def test_complete_calls_reach_the_context():
    for op in OPS:
        for dtype in DTYPES[op]:
            assert _call(op, dtype=dtype) == (-1, "null context"), (op, dtype)
        assert _call(op, nplanes=0) == (-1, "null context")
        assert _call(op, mode=1) == (-1, "null context")
        far = {"inp": 1 << 40, "out": 3 << 40, "minuend": (5 << 40) if op in (17, 18) else None}
        assert _call(op, mode=2**31 - 2, **far) == (-1, "null context")
        assert _call(op, H=46340, W=46340, **far) == (-1, "null context")  # just below 2^31 pixels
    for r in (1, 2, 5, 15):
        assert _call(15, fp=np.full((2 * r + 1, 2 * r + 1), r)) == (-1, "null context")
    for k in (0, 1, 15):
        assert _call(17, fp=np.full((2 * k + 1, 2 * k + 1), 7)) == (-1, "null context")
    assert _call(15, mode=0) == (-1, "null context")  # no border
    assert _call(15, minuend=_M) == (-1, "null context")  # per-plane thresholds
    for cval in (0.0, -5.5, 1e300, float("inf")):
        assert _call(15, cval=cval) == (-1, "null context")
    for op in (16, 18):  # the footprint is ignored
        assert _call(op, fp=np.zeros((2, 5))) == (-1, "null context")


@pytest.mark.parametrize("op", OPS)
def test_refusals_need_no_device(op):
    def refused(word, **kw):
        code, msg = _call(op, **kw)
        assert code == -1 and word in msg and msg.startswith("amt_rank_filter: ") and "null context" not in msg, (kw, msg)

    for dtype in {_hip.U8, _hip.U16, _hip.I32, _hip.F64, _hip.F32, _hip.I64, 17} - set(DTYPES[op]):
        refused("dtype", dtype=dtype)
    refused("plane too large", H=65536, W=32768, inp=1 << 40, out=3 << 40, minuend=(5 << 40) if op in (17, 18) else None)
    if op == 15:
        for fp in (np.ones((1, 1)), np.ones((33, 33)), np.ones((3, 5)), np.eye(3), np.ones((2, 2)), np.zeros((3, 3)),
                   [[1, 1, 1], [1, 0, 1], [1, 1, 1]]):  # r = 0, r = 16, not square, a zero cell, even
            refused("footprint", fp=fp)
        for b in (-1, -2**31):
            refused("border", mode=b)
    else:
        for cap in (0, -1, -2**31):
            refused("capacity", mode=cap, minuend=None if op == 16 else (5 << 40), inp=1 << 40, out=3 << 40)
    if op == 16:
        refused("minuend", minuend=_M)
    if op in (17, 18):
        refused("minuend", minuend=None)
    if op == 17:
        for fp in (np.ones((33, 33)), np.ones((3, 5)), np.eye(3), np.ones((2, 2)), np.zeros((1, 1))):
            refused("footprint", fp=fp)


def test_overlaps_are_refused_by_one_byte_and_touching_buffers_pass():
    n, H, W, cap = 2, 4, 4, 3
    for op in OPS:
        for dtype in DTYPES[op]:
            in_bytes = n * H * W * ESIZE[dtype]
            out_bytes = {15: n * H * W, 16: n * (cap + 1) * 4, 17: n * cap * 7 * 8, 18: n * cap * ESIZE[dtype]}[op]
            kw = {"dtype": dtype, "nplanes": n, "mode": cap}
            # `out` against `in`: its first byte on the last byte of `in`, its last byte on the first
            for out in (_A + in_bytes - 1, _A - out_bytes + 1, _A):
                code, msg = _call(op, out=out, **kw)
                assert code == -1 and "alias" in msg and msg.startswith("amt_rank_filter: "), (op, dtype, msg)
            for out in (_A + in_bytes, _A - out_bytes):  # they only touch
                assert _call(op, out=out, **kw) == (-1, "null context"), (op, dtype)
            if op == 16:
                continue
            m_bytes = n * 8 if op == 15 else n * (cap + 1) * 4
            for out in (_M + m_bytes - 1, _M - out_bytes + 1):
                code, msg = _call(op, out=out, minuend=_M, **kw)
                assert code == -1 and "alias" in msg and "minuend" in msg, (op, dtype, msg)
            code, msg = _call(op, out=_M, minuend=_M, **kw)
            assert code == -1 and ("alias" in msg or "differ from out" in msg)
            for out in (_M + m_bytes, _M - out_bytes):
                assert _call(op, out=out, minuend=_M, **kw) == (-1, "null context"), (op, dtype)
            assert _call(op, inp=_M, minuend=_M, **kw) == (-1, "null context")  # inputs may overlap inputs


# ---- the Python layers' argument errors -------------------------------------------------------------------------------------
class _NoDevice:
    """Stands where a DeviceArray would: any attribute access means validation did not come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the array was touched ({name}) before the arguments were validated")


class _NoContext:
    """Stands where a Context would: an operator that reaches for it (allocation, handle, stream) fails."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}): a device call before the refusal")


_CTX = _NoContext()


def _HostOnly(shape, dtype, ptr=4096):
    return DeviceArray(_CTX, ptr, shape, dtype)


def test_hipops_scalar_errors_come_before_any_device_access():
    for bad in (0, 16, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="min_distance"):
            hipops.local_maxima(_NoDevice(), bad)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="exclude_border"):
            hipops.local_maxima(_NoDevice(), 1, 0.0, bad)
    for bad in ("high", None, float("nan"), [1.0]):
        with pytest.raises(ValueError, match="threshold"):
            hipops.local_maxima(_NoDevice(), 1, bad)
    for bad in (0, -3, 1.5, True, 2**31 - 1):
        with pytest.raises(ValueError, match="capacity"):
            hipops.mask_list(_NoDevice(), bad)
    for bad in (-1, 16, 1.5, None, True):
        with pytest.raises(ValueError, match="radius"):
            hipops.spot_measure(_NoDevice(), _NoDevice(), bad)
    for fn in (hipops.local_maxima, hipops.mask_list, lambda a: hipops.spot_measure(a, _NoDevice()),
               lambda a: hipops.take_at(a, _NoDevice())):
        with pytest.raises(ValueError, match="DeviceArray"):
            fn(np.zeros((1, 4, 4), np.uint16))


def test_hipops_array_errors_and_overlaps_come_before_any_device_access():
    far = 1 << 20
    spots = _HostOnly((2, 4), np.int32, ptr=far)
    every = ((hipops.local_maxima, np.uint16, np.float32), (hipops.mask_list, np.uint8, np.uint16),
             (lambda a, **kw: hipops.spot_measure(a, spots, **kw), np.float64, np.int32),
             (lambda a, **kw: hipops.take_at(a, spots, **kw), np.int32, np.float32))
    for fn, good, bad in every:
        for shape in ((4, 4), (1, 2, 4, 4)):
            with pytest.raises(ValueError, match=r"\(N, H, W\)"):
                fn(_HostOnly(shape, good))
        with pytest.raises(ValueError, match="must be"):
            fn(_HostOnly((2, 4, 4), bad))
        with pytest.raises(ValueError, match="H \\* W"):
            fn(_HostOnly((2, 0, 4), good))
    a = _HostOnly((2, 4, 4), np.uint16)
    for bad in (_HostOnly((3, 4), np.int32, ptr=far), _HostOnly((2, 4), np.int64, ptr=far), _HostOnly((2, 1), np.int32, ptr=far),
                _HostOnly((8,), np.int32, ptr=far), np.zeros((2, 4), np.int32), None):
        for fn in (hipops.spot_measure, hipops.take_at):
            with pytest.raises(ValueError, match="spots must be"):
                fn(a, bad)
    for bad in (_HostOnly((3,), np.float64, ptr=far), _HostOnly((2,), np.float32, ptr=far), _HostOnly((2, 1), np.float64, ptr=far)):
        with pytest.raises(ValueError, match="per-plane thresholds"):
            hipops.local_maxima(a, 1, bad)
    # out= of the wrong shape or dtype, then overlaps by one element, then neighbours that only touch
    m = _HostOnly((2, 4, 4), np.uint8)
    calls = ((lambda **kw: hipops.local_maxima(a, **kw), a, (2, 4, 4), np.uint8),
             (lambda **kw: hipops.mask_list(m, 3, **kw), m, (2, 4), np.int32),
             (lambda **kw: hipops.spot_measure(a, spots, **kw), a, (2, 3, 7), np.float64),
             (lambda **kw: hipops.take_at(a, spots, **kw), a, (2, 3), np.uint16))
    for fn, src, shape, dtype in calls:
        with pytest.raises(ValueError, match="out has shape"):
            fn(out=_HostOnly(shape + (1,), dtype, ptr=2 * far))
        with pytest.raises(ValueError, match="out has shape"):
            fn(out=_HostOnly(shape, np.float32, ptr=2 * far))
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        for ptr in (4096, 4096 + src.nbytes - 1, 4096 - nbytes + 1):
            with pytest.raises(ValueError, match="alias"):
                fn(out=_HostOnly(shape, dtype, ptr=ptr))
        for ptr in (4096 + src.nbytes, 4096 - nbytes):
            with pytest.raises(AssertionError, match="the context was used"):  # as far as the call
                fn(out=_HostOnly(shape, dtype, ptr=ptr))
    for fn, shape, dtype in ((hipops.spot_measure, (2, 3, 7), np.float64), (hipops.take_at, (2, 3), np.uint16)):
        for ptr in (far, far + spots.nbytes - 1):
            with pytest.raises(ValueError, match="alias"):
                fn(a, spots, out=_HostOnly(shape, dtype, ptr=ptr))
    thr = _HostOnly((2,), np.float64, ptr=far)
    with pytest.raises(ValueError, match="alias"):
        hipops.local_maxima(a, 1, thr, out=_HostOnly((2, 4, 4), np.uint8, ptr=far + 15))
    with pytest.raises(AssertionError, match="the context was used"):
        hipops.local_maxima(a, 1, thr, out=_HostOnly((2, 4, 4), np.uint8, ptr=far + 16))


def test_operations_argument_checking():
    img = np.zeros((8, 8), np.uint16)
    for name, value in (("labels", img), ("footprint", np.ones((3, 3))), ("p_norm", 2), ("num_peaks_per_label", 3)):
        with pytest.raises(NotImplementedError, match="detect_spots") as e:
            operations.peak_local_max(img, **{name: value})
        assert "cell_spots" in str(e.value) and name in str(e.value)
    for bad in (0, 16, 1.5, True, None):
        with pytest.raises(ValueError, match="min_distance"):
            operations.peak_local_max(img, bad)
        with pytest.raises(ValueError, match="min_distance"):
            operations.detect_spots(img, min_distance=bad)
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError, match="exclude_border"):
            operations.peak_local_max(img, exclude_border=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="exclude_border"):
            operations.detect_spots(img, exclude_border=bad)
        with pytest.raises(ValueError, match="num_peaks"):
            operations.peak_local_max(img, num_peaks=bad)
    for bad in ("x", float("nan"), [1], True):
        with pytest.raises(ValueError, match="threshold_abs"):
            operations.peak_local_max(img, threshold_abs=bad)
        with pytest.raises(ValueError, match="threshold_rel"):
            operations.peak_local_max(img, threshold_rel=bad)
        with pytest.raises(ValueError, match="threshold"):
            operations.detect_spots(img, threshold=bad)
    for bad in (0, -1.0, "1", True, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            operations.detect_spots(img, sigma=bad)
    for bad in (-1, 16, 1.5, None, True):
        with pytest.raises(ValueError, match="radius"):
            operations.detect_spots(img, radius=bad)
    for bad in (float("inf"), float("nan"), "5", None):
        with pytest.raises(ValueError, match="snr"):
            operations.detect_spots(img, snr=bad)
    nan = np.zeros((8, 8))
    nan[3, 3] = np.nan
    for fn in (operations.peak_local_max, operations.detect_spots):
        with pytest.raises(ValueError, match="NaN"):
            fn(nan)
        for shape in ((8,), (2, 8, 8)):
            with pytest.raises(ValueError, match="2-D"):
                fn(np.zeros(shape, np.uint16))
        with pytest.raises(ValueError, match="empty"):
            fn(np.zeros((0, 8), np.uint16))
