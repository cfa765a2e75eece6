"""Grey reconstruction without a GPU: the two numpy references agree with each other, with a hand-worked example and
with the path formula; the header defines and documents the four new ``op`` codes of amt_rank_filter and no new
prototype; every refusal that needs no device arrives with a null context; the Python layers refuse bad arguments before
any device access."""
import ctypes
import os
import re

import numpy as np
import pytest

import reconstruction_cases as rc
import reconstruction_reference as rr
from arcadia_microscopy_tools_amd import _hip, hipops, operations
from arcadia_microscopy_tools_amd.pipeline import is_device_operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "amt_hip.h")).read()


# ---- the references ---------------------------------------------------------------------------------------------------
def test_worked_example():
    for fpn, fp in rr.FOOTPRINTS.items():
        for fn in (rr.naive, rr.flood, rr.path_formula):
            assert np.array_equal(fn(rr.WORKED_SEED, rr.WORKED_MASK, fp), rr.WORKED[fpn]), (fpn, fn.__name__)
        want = rr.dual(rr.WORKED[fpn])
        for fn in (rr.naive, rr.flood):
            got = fn(rr.dual(rr.WORKED_SEED), rr.dual(rr.WORKED_MASK), fp, "erosion")
            assert np.array_equal(got, want), (fpn, fn.__name__)
    assert not np.array_equal(rr.WORKED["cross"], rr.WORKED["ones"])


def test_references_agree_with_the_path_formula():
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (1, 6), (6, 1), (2, 3), (4, 5), (6, 6)):
        for dt in (np.uint16, np.float64):
            for _ in range(4):
                mask = rng.integers(0, 6, shape).astype(dt)
                seed = np.minimum(mask, rng.integers(0, 6, shape).astype(dt))
                if dt == np.float64:
                    mask, seed = mask - 2.5, seed - 2.5
                for fp in rr.FOOTPRINTS.values():
                    want = rr.path_formula(seed, mask, fp)
                    assert np.array_equal(rr.naive(seed, mask, fp), want)
                    assert np.array_equal(rr.flood(seed, mask, fp), want)
                    for fn in (rr.naive, rr.flood):
                        assert np.array_equal(fn(rr.dual(seed), rr.dual(mask), fp, "erosion"), rr.dual(want))


@pytest.mark.parametrize("kind", list(rc.KINDS))
def test_references_agree_on_the_small_cases(kind):
    table, want = rc.cases(kind), rc.expected(kind)
    assert len(table) == len(want)
    checked = 0
    for (name, fpn, seeds, masks), exp in zip(table, want):
        assert seeds.shape == masks.shape == exp.shape and seeds.dtype == masks.dtype == rc.KINDS[kind]
        assert (seeds <= masks).all(), name
        if not name.startswith("small"):
            continue
        for s, m, e in zip(seeds, masks, exp):
            assert np.array_equal(rr.naive(s, m, rr.FOOTPRINTS[fpn]), e), name
            checked += 1
    assert checked == 2 * len(rc.SMALL)


@pytest.mark.parametrize("kind", list(rc.KINDS))
def test_case_table_holds_what_it_promises(kind):
    th, tw = hipops.reconstruct_tile(rc.KINDS[kind])
    H, W = rc.seam_shape(kind)
    assert (H, W) == (2 * th + 3, 2 * tw + 5)
    by_name = {}
    for (name, fpn, seeds, masks), exp in zip(rc.cases(kind), rc.expected(kind)):
        by_name[(name, fpn)] = (seeds, masks, exp)
        assert not np.signbit(seeds.astype(np.float64)[seeds == 0]).any()  # no -0.0
    for shape in rc.SMALL:
        assert by_name[(f"small {shape[0]}x{shape[1]}", "cross")][0].shape == (1,) + shape
    s, m, e = by_name[("corners", "cross")]
    assert s.shape == (4, H, W) and all(np.all(e[i] == 17 + i) for i in range(4))  # each corner fills its whole plane
    s, m, e = by_name[("serpentine", "cross")]
    assert np.array_equal(e[0] == 700, m[0] == 1000) and int((s != 0).sum()) == 1  # the whole corridor from one pixel
    s, m, e = by_name[("serpentine transposed", "cross")]
    assert np.array_equal(e[0] == 700, m[0] == 1000) and (m[0][:, 0] == 1000).all()
    assert int((by_name[("staircase", "cross")][2] != 0).sum()) == 2  # stops at both first pixels
    e8 = by_name[("staircase", "ones")][2][0]
    assert e8[th - 1, tw - 1] == 699 and e8[th, tw] == 699 and e8[H - 1, H - 1] == 700  # through the tiles' common corner
    s, m, e = by_name[("full range", "ones")]
    if kind == "u16":
        assert m.min() == 0 and m.max() == 65535 and e.max() == 65535
    else:
        assert np.isinf(e).any() and (e < 0).any() and np.isneginf(s).any() and not np.isnan(e).any()
    s, m, e = by_name[("batch", "cross")]
    assert s.shape[0] == 3 and np.array_equal(s[0], m[0]) and np.array_equal(e[0], m[0])
    a = rc.h_image(kind)
    assert a.shape == (1, H, W) and a.dtype == rc.KINDS[kind]


def test_h_seed_saturates_at_both_ends():
    a = np.array([[0, 1, 299, 300, 65534, 65535]], np.uint16)
    assert rr.h_seed(a, 300).tolist() == [[0, 0, 0, 0, 65234, 65235]]
    assert rr.h_seed(a, 300, "erosion").tolist() == [[300, 301, 599, 600, 65535, 65535]]
    assert rr.h_seed(a, 65535).max() == 0 and rr.h_seed(a, 65535, "erosion").min() == 65535


# ---- the header and the binding ---------------------------------------------------------------------------------------
def test_header_defines_and_documents_the_codes():
    for name, value in (("AMT_RANK_RECONSTRUCT_DILATION", 3), ("AMT_RANK_RECONSTRUCT_EROSION", 4),
                        ("AMT_RANK_HMAX_RECONSTRUCT", 5), ("AMT_RANK_HMIN_RECONSTRUCT", 6)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", HEADER, re.M), name
    block = HEADER[:HEADER.index("int amt_rank_filter(")]
    block = block[block.rindex("/* grey erosion"):]
    for word in ("AMT_RANK_RECONSTRUCT_DILATION", "AMT_RANK_RECONSTRUCT_EROSION", "AMT_RANK_HMAX_RECONSTRUCT",
                 "AMT_RANK_HMIN_RECONSTRUCT", "WAIT FOR THE DEVICE", "seed <= mask", "4-connected", "8-connected", "NaN",
                 "h-dome", "residue >= h", "R(p) == seed(p)", "2^31", "nplanes == 0"):
        assert word in block, word


def test_binding_constants():
    assert (_hip.RANK_RECONSTRUCT_DILATION, _hip.RANK_RECONSTRUCT_EROSION, _hip.RANK_HMAX_RECONSTRUCT,
            _hip.RANK_HMIN_RECONSTRUCT) == (3, 4, 5, 6)
    tiles = {k: tuple(int(re.search(rf"^#define\s+AMT_RECONSTRUCT_TILE_{d}_{k}\s+(\d+)\s*$", HEADER, re.M).group(1))
                      for d in "HW") for k in ("U16", "F64")}
    assert hipops.reconstruct_tile(np.uint16) == _hip.RECONSTRUCT_TILE_U16 == tiles["U16"]
    assert hipops.reconstruct_tile(np.float64) == _hip.RECONSTRUCT_TILE_F64 == tiles["F64"]
    with pytest.raises(TypeError):
        hipops.reconstruct_tile(np.float32)
    for fn in (operations.reconstruction, operations.h_maxima, operations.h_minima):
        assert is_device_operator(fn)


def test_prototypes_are_unchanged():
    """The capability rides on amt_rank_filter: the C ABI has the names and the count it had."""
    bare = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    names = re.findall(r"^(?:int|const char\s*\*)\s*(amt_\w+)\s*\(", bare, flags=re.M)
    assert len(names) == len(set(names)) == len(_hip._SIGS) and set(names) == set(_hip._SIGS)
    assert not [n for n in names if "reconstruct" in n or "maxima" in n or "minima" in n]
    lib = _hip.load_library()
    assert not hasattr(lib, "amt_reconstruct") and not hasattr(lib, "amt_i_reconstruct")


# ---- refusals of the C ABI with a null context ---------------------------------------------------------------------------
def _call(op, *, dtype=_hip.U16, fp=rr.ONES, cval=0.0, minuend="own", inp="own", out="own", H=4, W=4, nplanes=1):
    lib = _hip.load_library()
    buf = np.zeros(3 * 512, np.float64)
    a, b, c = (buf[k * 512:].ctypes.data for k in range(3))
    fp = np.ascontiguousarray(fp, np.uint8)
    args = [None, a if inp == "own" else inp, b if out == "own" else out, dtype, nplanes, H, W, fp.ctypes.data, fp.shape[0],
            fp.shape[1], op, 0, float(cval), c if minuend == "own" else minuend]
    rc_ = lib.amt_rank_filter(*args)
    return rc_, lib.amt_last_error().decode()


@pytest.mark.parametrize("op", [3, 4, 5, 6])
def test_refusals_need_no_device(op):
    h = dict(cval=2.0, minuend=None) if op >= 5 else {}
    bad_fps = (np.ones((3, 5)), np.ones((5, 5)), np.eye(3), np.zeros((3, 3)), np.ones((1, 1)),
               [[0, 1, 0], [1, 1, 1], [0, 1, 1]], [[1, 1, 1], [1, 0, 1], [1, 1, 1]])
    for fp in bad_fps:
        code, msg = _call(op, fp=fp, **h)
        assert code == -1 and "footprint" in msg and "null context" not in msg, msg
    for dtype in (_hip.U8, _hip.I32, _hip.F32, _hip.I64):
        code, msg = _call(op, dtype=dtype, **h)
        assert code == -1 and "dtype" in msg and "null context" not in msg, msg
    if op <= 4:
        code, msg = _call(op, minuend=None)
        assert code == -1 and "mask" in msg and "NULL" in msg, msg
    else:
        for bad in (0.0, -1.0, 0.5, 65536.0, float("nan"), float("inf")):
            code, msg = _call(op, cval=bad, minuend=None)
            assert code == -1 and "h (cval)" in msg and "null context" not in msg, (bad, msg)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            code, msg = _call(op, dtype=_hip.F64, cval=bad, minuend=None)
            assert code == -1 and "h (cval)" in msg and "null context" not in msg, (bad, msg)
        assert _call(op, dtype=_hip.F64, cval=0.5, minuend=None)[1] == "null context"
    if op == 6:
        code, msg = _call(op, cval=2.0)
        assert code == -1 and "minuend" in msg and "null context" not in msg, msg
    # the existing aliasing check stays: out against either input
    buf = np.zeros(64, np.float64)
    code, msg = _call(op, inp=buf.ctypes.data, out=buf.ctypes.data, **h)
    assert code == -1 and "must not alias" in msg, msg
    if op != 6:
        code, msg = _call(op, out=buf.ctypes.data, **{**h, "minuend": buf.ctypes.data})
        assert code == -1 and "differ from out" in msg, msg
    # 4 GiB operands that never overlap (and are never touched: the refusal comes first)
    far = dict(inp=1 << 40, out=2 << 40)
    code, msg = _call(op, H=65536, W=32768, **far, **{**h, "minuend": None if op >= 5 else 3 << 40})
    assert code == -1 and "2^31" in msg, msg


@pytest.mark.parametrize("op", [3, 4, 5, 6])
@pytest.mark.parametrize("fp", list(rr.FOOTPRINTS))
def test_a_complete_call_reaches_the_context(op, fp):
    h = dict(cval=2.0, minuend=None) if op >= 5 else {}
    for dtype in (_hip.U16, _hip.F64):
        assert _call(op, dtype=dtype, fp=rr.FOOTPRINTS[fp], **h) == (-1, "null context")
    if op == 5:  # the h-dome's minuend; seed and mask may be one buffer
        assert _call(op, cval=65535.0) == (-1, "null context")
    if op <= 4:
        buf = np.zeros(64, np.float64)
        assert _call(op, inp=buf.ctypes.data, minuend=buf.ctypes.data) == (-1, "null context")


def test_the_filter_ops_keep_their_messages():
    for op in (0, 1, 2, 7, -1):
        assert _call(op) == (-1, "null context")


# ---- the Python layers: refusals before any device access -------------------------------------------------------------
class _NoDevice:
    """Stands where a DeviceArray would: any attribute access means validation did not come first."""

    def __getattr__(self, name):
        raise AssertionError(f"the array was touched ({name}) before the arguments were validated")


class _Fake:
    """A DeviceArray's description without a device: enough for the checks that come before the first call."""

    def __init__(self, shape, dtype, ptr=4096):
        self.shape, self.dtype, self.ptr, self.ndim = tuple(shape), np.dtype(dtype), ptr, len(shape)
        self.size = int(np.prod(shape))
        self.nbytes = self.size * self.dtype.itemsize

    @property
    def ctx(self):
        raise AssertionError("the context was asked for before the arguments were validated")

    @property
    def nplanes(self):
        return int(np.prod(self.shape[:-2]))


def test_hipops_refusals():
    nd = _NoDevice()
    for fp in (np.ones((5, 5)), np.eye(3), np.ones(3)):
        for call in (lambda: hipops.reconstruction(nd, nd, "dilation", fp), lambda: hipops.h_reconstruction(nd, 1, footprint=fp),
                     lambda: hipops.h_maxima(nd, 1, fp), lambda: hipops.h_minima(nd, 1, fp)):
            with pytest.raises(ValueError, match="footprint"):
                call()
    with pytest.raises(ValueError, match="method"):
        hipops.reconstruction(nd, nd, "opening")
    with pytest.raises(ValueError, match="method"):
        hipops.h_reconstruction(nd, 1, "closing")
    u, f = _Fake((2, 8, 8), np.uint16), _Fake((2, 8, 8), np.float64)
    with pytest.raises(TypeError):
        hipops.reconstruction(_Fake((8, 8), np.float32), _Fake((8, 8), np.float32))
    with pytest.raises(ValueError, match="same shape and dtype"):
        hipops.reconstruction(u, f)
    with pytest.raises(ValueError, match="same shape and dtype"):
        hipops.reconstruction(u, _Fake((2, 8, 9), np.uint16))
    with pytest.raises(ValueError, match=r"\(H, W\) or \(N, H, W\)"):
        hipops.reconstruction(_Fake((2, 2, 8, 8), np.uint16), _Fake((2, 2, 8, 8), np.uint16))
    for img, bad in ((u, 0), (u, -3), (u, 2.5), (u, 65536), (u, float("nan")), (f, 0.0), (f, -1.0), (f, float("inf")),
                     (u, "2"), (u, True), (u, None)):
        for fn in (hipops.h_reconstruction, hipops.h_maxima, hipops.h_minima):
            with pytest.raises(ValueError, match="h "):
                fn(img, bad)
    with pytest.raises(ValueError, match="minuend"):
        hipops.h_reconstruction(u, 2, "erosion", minuend=u)
    with pytest.raises(TypeError):
        hipops.h_maxima(_Fake((8, 8), np.uint8), 2)


def test_operations_refusals_and_empty_results():
    img = np.arange(48, dtype=np.uint16).reshape(6, 8)
    with pytest.raises(ValueError, match="offset"):
        operations.reconstruction(img, img, offset=np.array([1, 1]))
    with pytest.raises(ValueError, match="footprint"):
        operations.reconstruction(img, img, footprint=np.ones((5, 5)))
    with pytest.raises(ValueError, match="method"):
        operations.reconstruction(img, img, method="both")
    with pytest.raises(ValueError, match="2D"):
        operations.reconstruction(img[None], img[None])
    with pytest.raises(ValueError, match="same shape"):
        operations.reconstruction(img, img[:, :4])
    for bad in (np.float32, np.int16, np.int64, np.bool_):
        with pytest.raises(TypeError):
            operations.reconstruction(img.astype(bad), img.astype(bad))
        with pytest.raises(TypeError):
            operations.h_maxima(img.astype(bad), 2)
    with pytest.raises(TypeError, match="same dtype"):
        operations.reconstruction(img, img.astype(np.float64))
    with pytest.raises(ValueError, match="Intensity of seed image must be less than that of the mask image for "
                                         "reconstruction by dilation"):
        operations.reconstruction(img + 1, img)
    with pytest.raises(ValueError, match="Intensity of seed image must be greater than that of the mask image for "
                                         "reconstruction by erosion"):
        operations.reconstruction(img, img + 1, method="erosion")
    for fn in (operations.h_maxima, operations.h_minima):
        for bad in (0, -2, 1.5, float("nan")):
            with pytest.raises(ValueError):
                fn(img, bad)
        with pytest.raises(ValueError):
            fn(img.astype(np.float64), 0.0)
        with pytest.raises(ValueError, match="2D"):
            fn(img[None], 2)
        # h above the image's range: scikit-image's early exit, no device involved
        z = fn(img, 48)
        assert z.dtype == np.uint8 and z.shape == img.shape and not z.any()
        assert not fn(img.astype(np.uint8), 200).any() and not fn(img.astype(np.float64), 47.5).any()
        for shape in ((0, 5), (3, 0)):
            e = fn(np.zeros(shape, np.uint16), 2)
            assert e.shape == shape and e.dtype == np.uint8
    for dt in (np.uint8, np.uint16, np.float64):
        e = operations.reconstruction(np.zeros((0, 4), dt), np.zeros((0, 4), dt))
        assert e.shape == (0, 4) and e.dtype == dt
