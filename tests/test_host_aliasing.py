"""The aliasing rule of include/amt_hip.h without a GPU: the table of tests/aliasing_cases.py is complete, the library
refuses every refused pair before it touches the context (made-up addresses, null context), accepts the in-place pairs only
when they coincide exactly, and the Python binding refuses first, before any device access."""
import os
import re

import numpy as np
import pytest

import aliasing_cases as ac
from arcadia_microscopy_tools_amd import _hip, hipops
from arcadia_microscopy_tools_amd.device import DeviceArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototypes():
    header = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    header = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    decls = re.findall(r"^(int|const char\s*\*)\s*(amt_\w+)\s*\(([^)]*)\)\s*;", header, flags=re.M)
    out = {}
    for _, name, params in decls:
        ps = []
        for p in params.split(","):
            p = " ".join(p.split())
            if p in ("", "void"):
                continue
            ps.append((p.rsplit("*", 1)[-1].strip() if "*" in p else p.rsplit(None, 1)[-1], "*" in p, p.startswith("const ")))
        out[name] = ps  # (parameter name, is a pointer, points to const)
    return out


def test_every_entry_point_that_writes_device_memory_has_a_verdict():
    protos = _prototypes()
    assert set(ac.EXEMPT) <= set(protos) and not set(ac.EXEMPT) & set(ac.BY_NAME)
    for name, params in protos.items():
        if name in ac.EXEMPT:
            continue
        writes = [p for p, ptr, const in params if ptr and not const and p not in ac.HANDLES]
        if not writes:
            assert name not in ac.BY_NAME, name  # nothing to write: no row
            continue
        assert name in ac.BY_NAME, f"{name} writes device memory and has no row in tests/aliasing_cases.py"
        r = ac.BY_NAME[name]
        ops = {o[0]: o for o in r.operands}
        listed = {n.split("[")[0] for n in ops}  # "layers_host[0]": a device operand inside the host table layers_host
        for p, ptr, const in params:
            if not ptr:
                continue
            kinds = [p in ac.HANDLES, p in r.host, p in ops]
            assert sum(kinds) == 1 or (p in r.host and p in listed and not kinds[2]), (name, p, "unclassified pointer")
            if p in ops:  # an output is a non-const pointer, an input a const one
                assert (ops[p][1] == "out") == (not const), (name, p)
        assert set(r.host) | {n for n in ops if "[" not in n} | set(ac.HANDLES) >= {p for p, ptr, _ in params if ptr}, name
        assert {n for n in ops if "[" not in n} <= {p for p, ptr, _ in params if ptr}, (name, "operand that is no parameter")
        assert set(r.inout) <= {o[0] for o in r.outputs()}, name
    assert set(ac.BY_NAME) <= set(protos)
    n_in_place, n_refused = ac.verdict_counts()
    assert n_in_place == 9 and n_refused > 100  # the figures of DESIGN.md


def _call(lib, r, addr):
    rc = getattr(lib, r.fn)(*r.args(addr))
    return rc, lib.amt_last_error().decode()


@pytest.mark.parametrize("fn", sorted(ac.BY_NAME))
def test_library_refuses_overlaps_before_it_touches_the_context(fn):
    lib = _hip.load_library()
    r = ac.BY_NAME[fn]
    rc, msg = _call(lib, r, ac.addresses(r))
    assert rc == -1 and msg == "null context", (fn, msg)  # apart, every operand: as far as the context
    for o, x, verdict in r.pairs():
        placements = ac.shifts(o, x)
        assert placements and placements[0] == ("exact", 0), (fn, o[0], x[0])
        for what, s in placements:
            addr = ac.addresses(r)
            addr[o[0]] = addr[x[0]] + s
            rc, msg = _call(lib, r, addr)
            if verdict == "in place" and s == 0:
                assert rc == -1 and msg == "null context", (fn, o[0], x[0], what, msg)
                continue
            assert rc == -1 and ("alias" in msg or "overlap" in msg), (fn, o[0], x[0], what, msg)
            assert msg.startswith(fn + ": ") and o[0] in msg and x[0] in msg, (fn, o[0], x[0], what, msg)
        for s in (x[2], -o[2]):  # neighbours that touch: not an overlap
            addr = ac.addresses(r)
            addr[o[0]] = addr[x[0]] + s
            rc, msg = _call(lib, r, addr)
            assert rc == -1 and msg == "null context", (fn, o[0], x[0], s, msg)


def test_in_place_needs_the_same_element_size():
    """amt_rescale on uint16 input: same start, other length and element size -- not the in-place pair."""
    lib = _hip.load_library()
    n = ac.N * ac.PX
    assert lib.amt_rescale(None, 1 << 24, ac.U16, 1 << 26, 0.0, 1.0, 1 << 24, ac.N, ac.PX) == -1
    assert "only in place" in lib.amt_last_error().decode()
    assert lib.amt_rescale(None, 1 << 24, ac.U16, 1 << 26, 0.0, 1.0, (1 << 24) + 2 * n, ac.N, ac.PX) == -1
    assert lib.amt_last_error() == b"null context"
    # absent operands (null pointers, empty batches) overlap nothing
    assert lib.amt_gaussian(None, 1 << 24, ac.F64, 1.0, 1 << 24, 0, 4, 6, None, 1, 0, 0.0, 0, None) == -1
    assert lib.amt_last_error() == b"null context"


# ---- the binding ------------------------------------------------------------------------------------------------------------
class _NoContext:
    """Stands where a Context would: an operator that reaches for it (allocation, handle, stream) fails."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}): a device call before the refusal")


_CTX = _NoContext()
_N, _H, _W = 3, 8, 8
_PL = {np.dtype(t): _H * _W * np.dtype(t).itemsize for t in (np.uint8, np.uint16, np.int32, np.float32, np.float64, np.int64)}


def _arr(shape, dtype, ptr):
    return DeviceArray(_CTX, ptr, shape, dtype)


def _stack(dtype, ptr=1 << 20):
    return _arr((_N, _H, _W), dtype, ptr)


def _small(shape, dtype, k):
    return _arr(shape, dtype, (1 << 28) + k * 4096)


# name -> (input dtype, output dtype, call(a, o), in place allowed)
_f64, _u8, _i32, _u16, _f32 = np.float64, np.uint8, np.int32, np.uint16, np.float32
BINDING = {
    "gaussian sigma 2": (_f64, _f64, lambda a, o: hipops.gaussian(a, 2.0, out=o), False),
    "gaussian sigma 4": (_f64, _f64, lambda a, o: hipops.gaussian(a, 4.0, out=o), False),
    "uniform_filter": (_f64, _f64, lambda a, o: hipops.uniform_filter(a, 3, out=o), False),
    "difference_of_gaussians": (_f64, _f64, lambda a, o: hipops.difference_of_gaussians(a, 0.6, 3.0, out=o), False),
    "window_threshold": (_f64, _f64, lambda a, o: hipops.window_threshold(a, 3, out=o), False),
    "sub_clip0": (_f64, _f64, lambda a, o: hipops.sub_clip0(a, _small((_N,), _f64, 1), out=o), True),
    "rescale": (_f64, _f64, lambda a, o: hipops.rescale(a, _small((_N, 2), _f64, 1), out=o), True),
    "add_scalar": (_f64, _f64, lambda a, o: hipops.add_scalar(a, 1.0, out=o), True),
    "clear_border": (_i32, _i32, lambda a, o: hipops.clear_border(a, out=o), True),
    "relabel_sequential": (_i32, _i32, lambda a, o: hipops.relabel_sequential(a, 5, out=o, count=_small((_N,), _i32, 1)), True),
    "clear_border_relabel": (_i32, _i32, lambda a, o: hipops.clear_border_relabel(a, 5, out=o, count=_small((_N,), _i32, 1)), True),
    "keep_labels": (_i32, _i32, lambda a, o: hipops.keep_labels(a, _small((_N, 6), _u8, 1), 5, out=o), True),
    "label int32": (_i32, _i32, lambda a, o: hipops.label(a, out=o, count=_small((_N,), _i32, 1)), False),
    "expand_labels": (_i32, _i32, lambda a, o: hipops.expand_labels(a, 2.0, out=o), False),
    "binary_erosion": (_u8, _u8, lambda a, o: hipops.binary_erosion(a, out=o), False),
    "binary_closing": (_u8, _u8, lambda a, o: hipops.binary_closing(a, out=o), False),
    "binary_fill_holes": (_u8, _u8, lambda a, o: hipops.binary_fill_holes(a, out=o), False),
    "remove_small_objects": (_u8, _u8, lambda a, o: hipops.remove_small_objects(a, 4, out=o), False),
    "median": (_u16, _u16, lambda a, o: hipops.median(a, out=o), False),
    "erosion": (_u16, _u16, lambda a, o: hipops.erosion(a, out=o), False),
    "watershed_edt out=d2": (_i32, _i32, lambda a, o: hipops.watershed_edt(a, _small((_N, _H, _W), _i32, 8),
                                                                            _small((_N, _H, _W), _u8, 4), out=o), False),
    "watershed_edt out=markers": (_i32, _i32, lambda a, o: hipops.watershed_edt(_small((_N, _H, _W), _i32, 8), a,
                                                                                 _small((_N, _H, _W), _u8, 4), out=o), False),
    "peak_mask out=mask": (_u8, _u8, lambda a, o: hipops.peak_mask(_small((_N, _H, _W), _i32, 8), a, 1, out=o), False),
    "cellpose_masks out=cellprob": (_f32, _i32, lambda a, o: hipops.cellpose_masks(_small((_N, 2, _H, _W), _f32, 16), a, out=o,
                                                                                   count=_small((_N,), _i32, 1)), False),
    "normalize_planes": (_f32, _f32, lambda a, o: hipops.normalize_planes(a, _small((_N, 2), _f64, 1), out=o), False),
    "greater_than": (_f64, _u8, lambda a, o: hipops.greater_than(a, _small((_N,), _f64, 1), out=o), False),
    "to_float64": (_u16, _f64, lambda a, o: hipops.to_float64(a, out=o), False),
    "to_int64": (_i32, np.int64, lambda a, o: hipops.to_int64(a, out=o), False),
    "edt d2_out": (_u8, _i32, lambda a, o: hipops.edt(a, want_edt=False, d2_out=o), False),
}


@pytest.mark.parametrize("name", sorted(BINDING))
def test_binding_refuses_before_any_device_access(name):
    tin, tout, call, in_place = BINDING[name]
    base = 1 << 20
    a = _stack(tin, base)
    plane = _PL[np.dtype(tout)]
    for what, s in (("exact", 0), ("plane forward", plane), ("plane backward", -plane), ("8 bytes", 8)):
        o = _stack(tout, base + s)
        if not -o.nbytes < s < a.nbytes:  # an output plane longer than the whole input batch: a neighbour, below
            continue
        if in_place and s == 0:
            with pytest.raises(AssertionError, match="the context was used"):  # accepted: as far as the device call
                call(a, o)
            continue
        with pytest.raises(ValueError, match="alias"):
            call(a, o)
    for s in (a.nbytes, -_N * plane):  # neighbours that touch
        with pytest.raises(AssertionError, match="the context was used"):
            call(a, _stack(tout, base + s))


def test_binding_named_views():
    """label(stack[0:2], out=stack[1:3]), deinterleave onto its input, crop onto its source, a channel of a (C, Y, X) stack
    filtered onto its neighbour channel."""
    stack = _arr((3, _H, _W), _i32, 1 << 20)
    with pytest.raises(ValueError, match="alias"):
        hipops.label(stack[0:2], out=stack[1:3], count=_small((2,), _i32, 1))
    yxc = _arr((_N, _H, _W, 2), _u16, 1 << 20)
    with pytest.raises(ValueError, match="alias"):
        hipops.deinterleave(yxc, 2, out=_arr((_N, 2, _H, _W), _u16, 1 << 20))
    src = _arr((_N, _H, _W), _u16, 1 << 20)
    with pytest.raises(ValueError, match="alias"):
        hipops.crop(src, 1, 1, 4, 4, out=_arr((_N, 4, 4), _u16, (1 << 20) + 16))
    cyx = _arr((2, 2, _H, _W), _f64, 1 << 20)  # channel 0 of both stacks spans the first three planes of four
    with pytest.raises(ValueError, match="alias"):
        hipops.gaussian(cyx, 2.0, channel=0, out=_arr((2, _H, _W), _f64, (1 << 20) + _PL[np.dtype(_f64)]))
    with pytest.raises(AssertionError, match="the context was used"):
        hipops.gaussian(cyx, 2.0, channel=0, out=_arr((2, _H, _W), _f64, (1 << 20) + 4 * _PL[np.dtype(_f64)]))
