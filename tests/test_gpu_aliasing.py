"""Overlapping operands on the device (tests/aliasing_cases.py holds the verdicts, tests/test_host_aliasing.py the table's
completeness and the refusals at made-up addresses).  Inputs, references and comparison rules are operator_sweep's.

In place: the result written over the input equals the out-of-place result bit for bit, and the reference by the
operator's own rule.  Refused: on real overlapping views of one allocation the call is refused and every byte of the
allocation is what it was; the neighbouring view that does not overlap succeeds and equals the reference."""
import numpy as np
import pytest

import operator_sweep as sw
from arcadia_microscopy_tools_amd import _hip, hipops
from arcadia_microscopy_tools_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

OPS = {o.name: o for o in sw.OPS}
SHAPES = [(1, 1), (7, 5), (16, 16), (70, 131), (66, 320)]
CASES = [(s, v) for s in SHAPES for v in ("single", "batch")] + [((70, 131), "view")]  # view: plane 1 of a stack, unaligned
KINDS = {"single": (0,), "batch": (0, 1, 2), "view": (2, 0)}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _host(opname, p, shape, variant):
    """The host arrays of the case (planes on axis 0) and the reference of every plane, from operator_sweep."""
    op = OPS[opname]
    pi = op.params.index(p)
    kinds = KINDS[variant]
    Hs = [np.stack([sw.inputs(op, pi, shape, k)[j] for k in kinds]) for j in range(len(sw.inputs(op, pi, shape, kinds[0])))]
    checked = kinds[1:] if variant == "view" else kinds
    return op, Hs, [sw.reference(op, pi, shape, k) for k in checked]


def _upload(ctx, Hs, variant):
    D = [ctx.asarray(h) for h in Hs]
    return [d[1:] for d in D] if variant == "view" else D


def _check(op, p, got, refs, k=0):
    rule = sw._rules(op, p, len(refs[0]))[k]
    for i, want in enumerate(refs):
        ok, idx = rule(got[i], want[k])
        assert ok, (op.name, p, i, idx)


def _max_label(Hs):
    return max(int(Hs[0].max()), 1)


def _keep(ctx, Hs):
    keep = np.zeros((Hs[0].shape[0], _max_label(Hs) + 1), np.uint8)
    keep[:, 1::2] = 1
    return ctx.asarray(keep)


# name: (operator of the sweep, its parameter set, call(ctx, D, Hs, out) -> the device array that holds output 0)
IN_PLACE = {
    # the form of operations.subtract_background_dog: hipops.sub_clip0(f, level, out=f)
    "sub_clip0 as subtract_background_dog calls it": ("elementwise", "sub_clip0", lambda c, D, Hs, o: hipops.sub_clip0(D[0], D[1], out=o)),
    "rescale float64": ("elementwise", "rescale f64", lambda c, D, Hs, o: hipops.rescale(D[0], D[1], (0.0, 1.0), out=o)),
    "add_scalar": ("elementwise", "add_scalar", lambda c, D, Hs, o: hipops.add_scalar(D[0], -3.5, out=o)),
    "clear_border": ("label operators", "clear_border", lambda c, D, Hs, o: hipops.clear_border(D[0], out=o)),
    "relabel_sequential": ("label operators", "relabel_sequential",
                           lambda c, D, Hs, o: hipops.relabel_sequential(D[0], _max_label(Hs), out=o)[0]),
    "clear_border_relabel": ("label operators", "clear_border_relabel",
                             lambda c, D, Hs, o: hipops.clear_border_relabel(D[0], _max_label(Hs), out=o)[0]),
    "clear_border_relabel nlabels": ("label operators", "clear_border_relabel nlabels",
                                     lambda c, D, Hs, o: hipops.clear_border_relabel(D[0], _max_label(Hs), out=o, nlabels=D[1])[0]),
    "keep_labels": ("label operators", "keep_labels", lambda c, D, Hs, o: hipops.keep_labels(D[0], _keep(c, Hs), _max_label(Hs), out=o)),
}


@pytest.mark.parametrize("shape,variant", CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("name", sorted(IN_PLACE))
def test_in_place_equals_out_of_place_and_the_reference(ctx, name, shape, variant):
    opname, p, call = IN_PLACE[name]
    op, Hs, refs = _host(opname, p, shape, variant)
    D = _upload(ctx, Hs, variant)
    hs = [h[1:] for h in Hs] if variant == "view" else Hs
    apart = call(ctx, D, hs, None).numpy()
    assert np.array_equal(D[0].numpy(), hs[0])  # out of place leaves the input alone
    D2 = _upload(ctx, Hs, variant)
    res = call(ctx, D2, hs, D2[0])
    assert res.ptr == D2[0].ptr
    over = res.numpy()
    assert over.dtype == apart.dtype and over.tobytes() == apart.tobytes()
    _check(op, p, over, refs)


@pytest.mark.parametrize("shape,variant", CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("which", ("a", "b", "both"))
def test_subtract_in_place(ctx, which, shape, variant):
    """amt_subtract has no operator of its own in the sweep (difference_of_gaussians_nd and white_tophat end in it): the
    sweep's float64 planes, out = a, out = b, and a - a onto itself."""
    lib = _hip.load_library()
    kinds = KINDS[variant]
    a = np.stack([sw.img_f64(shape, k, 50) for k in kinds])
    b = np.stack([sw.img_f64(shape, k, 51) for k in kinds])
    da, db = ctx.asarray(a), ctx.asarray(b)
    if variant == "view":
        a, b, da, db = a[1:], b[1:], da[1:], db[1:]
    if which == "both":
        b, db = a, da
    out = da if which != "b" else db
    _hip.check(lib.amt_subtract(ctx.handle, da.ptr, db.ptr, out.ptr, _hip.F64, a.size), "amt_subtract")
    assert out.numpy().tobytes() == (a - b).tobytes()


def _same(h):
    return lambda c, D, Hs, o: h(D, o)


# name: (operator, parameter set, index of the input that the output overlaps, call(ctx, D, Hs, out) -> output 0,
#        dtype of the output).  Input and output planes have the same byte size in every case.
REFUSED = {
    "gaussian sigma 2.0 (radius 8, fused)": ("gaussian", ("f64", 2.0, "nearest"), 0, _same(lambda D, o: hipops.gaussian(D[0], 2.0, out=o))),
    "gaussian sigma 4.0 (radius 16, two passes)": ("gaussian", ("f64", 4.0, "nearest"), 0,
                                                   _same(lambda D, o: hipops.gaussian(D[0], 4.0, out=o))),
    "difference_of_gaussians": ("difference_of_gaussians", "f64", 0,
                                _same(lambda D, o: hipops.difference_of_gaussians(D[0], 0.6, 3.0, out=o))),
    "window_threshold float64": ("window_threshold", ("f64", "niblack", 3), 0,
                                 _same(lambda D, o: hipops.window_threshold(D[0], 3, "niblack", 0.2, out=o))),
    "label int32": ("label", ("int32", 2), 0, _same(lambda D, o: hipops.label(D[0], connectivity=2, out=o)[0])),
    "watershed_edt out=d2": ("watershed", ("edt", 1), 0,
                             _same(lambda D, o: hipops.watershed_edt(D[0], D[1], D[2], seeds_first=True, out=o))),
    "watershed_edt out=markers": ("watershed", ("edt", 1), 1,
                                  _same(lambda D, o: hipops.watershed_edt(D[0], D[1], D[2], seeds_first=True, out=o))),
    "peak_mask out=mask": ("peak_mask", 1, 1, _same(lambda D, o: hipops.peak_mask(D[0], D[1], 1, out=o))),
    "binary_erosion": ("binary morphology", ("erosion", "cross"), 0, _same(lambda D, o: hipops.binary_erosion(D[0], None, out=o))),
    "median uint16": ("median", ("u16", "sq3", "nearest"), 0,
                      _same(lambda D, o: hipops.median(D[0], np.ones((3, 3), np.uint8), mode="nearest", out=o))),
    "expand_labels": ("expand_labels", (1, False), 0, _same(lambda D, o: hipops.expand_labels(D[0], 1, out=o))),
}


@pytest.mark.parametrize("shape,variant", [c for c in CASES if c[1] != "view"], ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_overlaps_leave_every_byte_alone(ctx, name, shape, variant):
    opname, p, k, call = REFUSED[name]
    op, Hs, refs = _host(opname, p, shape, variant)
    n = Hs[0].shape[0]
    # the aliased input in the first n planes of ONE allocation of 2 n + 1 planes; the rest is filler the call must not touch
    filler = np.full((n + 1,) + Hs[k].shape[1:], 7, Hs[k].dtype)
    whole_h = np.concatenate([Hs[k], filler])
    whole = ctx.asarray(whole_h)
    if Hs[k].dtype == bool:
        whole_h = whole_h.view(np.uint8)
    others = [None if j == k else ctx.asarray(h) for j, h in enumerate(Hs)]
    probe = call(ctx, [ctx.asarray(h) for h in Hs], Hs, None)  # the output's dtype, from an ordinary call
    assert probe.dtype.itemsize == whole.dtype.itemsize, "the case needs planes of one byte size"

    plane = whole[0:1].nbytes

    def view(lo, nbytes=0):
        return DeviceArray(ctx, whole.ptr + lo * plane + nbytes, (n,) + tuple(Hs[k].shape[1:]), probe.dtype)

    def ins(lo):
        src = whole[lo:lo + n]
        return [src if j == k else d for j, d in enumerate(others)]

    placements = [("exact", 0, 0, 0)]
    if n > 1:  # one plane of a single-plane call is its neighbour, not an overlap
        placements += [("plane forward", 0, 1, 0), ("plane backward", 1, 0, 0)]
    if n * plane > 8:
        placements.append(("8 bytes", 0, 0, 8))
    for what, src_lo, dst_lo, off in placements:
        with pytest.raises(ValueError, match="alias"):
            call(ctx, ins(src_lo), Hs, view(dst_lo, off))
        assert whole.numpy().view(np.uint8).tobytes() == whole_h.view(np.uint8).tobytes(), (name, what)
        for j, d in enumerate(others):
            if d is not None:
                assert np.array_equal(d.numpy(), Hs[j]), (name, what, j)
    # the C ABI itself, past the binding: one plane forward (a single plane: exact)
    rc = _raw(ctx, name, ins(0), Hs, view(1) if n > 1 else view(0))
    if rc is not None:
        assert rc == -1 and "alias" in _hip.load_library().amt_last_error().decode(), name
        assert whole.numpy().view(np.uint8).tobytes() == whole_h.view(np.uint8).tobytes(), name
    # neighbours that touch: planes n .. 2 n written from planes 0 .. n
    got = call(ctx, ins(0), Hs, view(n)).numpy()
    _check(op, p, got, refs)
    assert np.array_equal(whole[0:n].numpy().view(np.uint8), whole_h[0:n].view(np.uint8))


def _raw(ctx, name, D, Hs, out):
    """The library call of the pinned cases without the binding's check in front (None: covered through the binding only)."""
    lib = _hip.load_library()
    n, H, W = D[0].shape
    if name.startswith("gaussian"):
        w = hipops.gaussian_weights(2.0 if "2.0" in name else 4.0)
        return lib.amt_gaussian(ctx.handle, D[0].ptr, _hip.F64, 1.0, out.ptr, n, H, W, w.ctypes.data, (len(w) - 1) // 2,
                                _hip.MODES["nearest"], 0.0, 0, None)
    if name == "watershed_edt out=d2" or name == "watershed_edt out=markers":
        return lib.amt_watershed_edt(ctx.handle, D[0].ptr, D[1].ptr, D[2].ptr, out.ptr, n, H, W, 1, 1, 0, None)
    if name == "label int32":
        cnt = ctx.empty((n,), np.int32)
        return lib.amt_label(ctx.handle, D[0].ptr, _hip.I32, out.ptr, cnt.ptr, n, H, W, 2)
    if name == "peak_mask out=mask":
        return lib.amt_peak_mask(ctx.handle, D[0].ptr, D[1].ptr, out.ptr, n, H, W, 1, None, None, 0, None)
    return None


def test_label_of_two_planes_onto_the_next_two(ctx):
    """label(stack[0:2], out=stack[1:3]): equal pointers were the only thing the library compared."""
    op = OPS["label"]
    pi = op.params.index(("int32", 2))
    planes = np.stack([sw.inputs(op, pi, (70, 131), k)[0] for k in (0, 2, 0)])
    stack = ctx.asarray(planes)
    with pytest.raises(ValueError, match="alias"):
        hipops.label(stack[0:2], out=stack[1:3])
    cnt = ctx.empty((2,), np.int32)
    lib = _hip.load_library()
    assert lib.amt_label(ctx.handle, stack[0:2].ptr, _hip.I32, stack[1:3].ptr, cnt.ptr, 2, 70, 131, 2) == -1
    assert "amt_label: out must not alias in" in lib.amt_last_error().decode()
    assert np.array_equal(stack.numpy(), planes)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_deinterleave_and_crop_onto_their_source(ctx, shape):
    op = OPS["deinterleave"]
    pi = op.params.index(3)
    frames = np.stack([sw.inputs(op, pi, shape, k)[0] for k in (0, 1, 2)])  # (3, H, W, 3)
    H, W = shape
    d = ctx.asarray(np.concatenate([frames, frames]))  # six frames: the last three are room for a neighbouring output
    src = d[0:3]
    for off in (0, 8 if src.nbytes > 8 else 2):
        with pytest.raises(ValueError, match="alias"):
            hipops.deinterleave(src, 3, out=DeviceArray(ctx, d.ptr + off, (3, 3, H, W), np.uint16))
    assert np.array_equal(d.numpy(), np.concatenate([frames, frames]))
    got = hipops.deinterleave(src, 3, out=DeviceArray(ctx, d.ptr + src.nbytes, (3, 3, H, W), np.uint16)).numpy()
    for i, k in enumerate((0, 1, 2)):
        assert np.array_equal(got[i], sw.reference(op, pi, shape, k)[0])
    # crop onto its source
    cop = OPS["crop and pad_edge"]
    cpi = cop.params.index(("crop", "u16"))
    planes = np.stack([sw.inputs(cop, cpi, shape, k)[0] for k in (0, 1, 2)])
    h, w = H - H // 3 - H // 5, W - W // 4 - W // 5
    if h == 0 or w == 0:
        return  # (1, 1) crops to nothing: an empty output overlaps nothing
    s = ctx.asarray(np.concatenate([planes, planes]))
    with pytest.raises(ValueError, match="alias"):
        hipops.crop(s[0:3], H // 3, W // 4, h, w, out=DeviceArray(ctx, s.ptr, (3, h, w), np.uint16))
    assert np.array_equal(s.numpy(), np.concatenate([planes, planes]))
    got = hipops.crop(s[0:3], H // 3, W // 4, h, w, out=DeviceArray(ctx, s.ptr + s[0:3].nbytes, (3, h, w), np.uint16)).numpy()
    for i, k in enumerate((0, 1, 2)):
        assert np.array_equal(got[i], sw.reference(cop, cpi, shape, k)[0])
