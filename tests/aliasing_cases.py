"""One verdict per operand pair, for every entry point of include/amt_hip.h that writes device memory.

The rule (include/amt_hip.h, Conventions): inputs may overlap inputs; an output -- caller-owned scratch and in/out planes
included -- must not overlap any other operand, not even in part, unless the pair is marked ``in place`` here, and then only
exactly (same start, same byte length, same element size).  ``in place`` is given where every kernel before the last only
reads the input and the last maps element i to element i within one thread; everything else is ``refused``, also where a
scratch copy happens to sit in between today.

A row lists the device operands of one entry point in the header's parameter names, with their role and how their byte
length follows from the arguments (written out for the small geometry below), the host pointers, and a builder of the C
arguments from made-up addresses -- with a null context nothing is dereferenced on the device side.  Not collected by
pytest (tests/test_host_aliasing.py and tests/test_gpu_aliasing.py are)."""
from __future__ import annotations

import ctypes

import numpy as np

N, H, W, C = 3, 4, 6, 2          # planes, rows, columns, channels of every made-up call
PX = H * W                       # pixels of a plane
K, NLAB, CAP, NQ, NBINS, NPAIRS = 5, 4, 7, 3, 16, 1
U8, U16, I32, F64, I64, F32 = 0, 1, 2, 3, 4, 5

# ---- host tables the calls read before (or without) touching the device ---------------------------------------------------
_W3 = np.array([0.25, 0.5, 0.25])
_FP = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
_Q = np.array([1.0, 50.0, 99.0])
_PAIRS = np.array([[0, 1]], np.int32)
_LUTS = np.zeros((2, 256, 4))
_OPAC = np.array([1.0, 0.5])
_MODE = np.zeros(2, np.int32)
_LEAD = np.array([N], np.int32)
_LWIN = np.array([3], np.int32)


def _p(a):
    return a.ctypes.data


EXEMPT = (  # plumbing: context, memory, stream, events, timers, host helpers -- no image operands to relate
    "amt_ctx_create", "amt_ctx_create_on_stream", "amt_ctx_destroy", "amt_ctx_set_fork", "amt_ctx_stream", "amt_device_name",
    "amt_malloc", "amt_free", "amt_memcpy_h2d", "amt_memcpy_d2h", "amt_memcpy_d2d", "amt_memset", "amt_sync",
    "amt_debug_scratch_check", "amt_stream_wait", "amt_event_create", "amt_event_record", "amt_event_wait", "amt_event_sync",
    "amt_event_destroy", "amt_host_alloc", "amt_host_free", "amt_host_copy", "amt_host_minmax_int", "amt_host_narrow_i64_i32",
    "amt_timer_create", "amt_timer_start", "amt_timer_stop", "amt_timer_elapsed_ms", "amt_timer_destroy")
HANDLES = ("ctx",)


class Row:
    def __init__(self, fn, operands, args, inplace=(), host=(), inout=(), note=""):
        self.fn, self.args, self.host, self.note = fn, args, tuple(host), note
        self.operands = [(n, r, int(b), int(e)) for n, r, b, e in operands]  # name, "in" / "out", bytes, element size
        self.inplace = set(inplace)   # (output, input) pairs accepted when exact
        self.inout = tuple(inout)     # outputs that are in/out by design (listed, and refused against everything else)
        names = [o[0] for o in self.operands]
        assert len(set(names)) == len(names) and all(o in names and i in names for o, i in self.inplace), fn

    def outputs(self):
        return [o for o in self.operands if o[1] == "out"]

    def pairs(self):
        """(output, other operand, verdict) for every pair the rule speaks about."""
        out = []
        for i, a in enumerate(self.operands):
            for b in self.operands[i + 1:]:
                if a[1] == "out" or b[1] == "out":
                    o, x = (a, b) if a[1] == "out" else (b, a)
                    out.append((o, x, "in place" if (o[0], x[0]) in self.inplace else "refused"))
        return out


ROWS: list[Row] = []


def row(*a, **kw):
    ROWS.append(Row(*a, **kw))


def _i(n, b, e=1):
    return (n, "in", b, e)


def _o(n, b, e=1):
    return (n, "out", b, e)


# ---- filters ----------------------------------------------------------------------------------------------------------------
row("amt_deinterleave_u16", [_i("yxc", N * PX * C * 2, 2), _o("cyx", N * PX * C * 2, 2)],
    lambda a: [None, a["yxc"], a["cyx"], N, H, W, C])
# in_plane_stride = 2 planes: the input spans (N - 1) * stride + H * W elements
row("amt_gaussian", [_i("in", ((N - 1) * 2 * PX + PX) * 8, 8), _o("out", N * PX * 8, 8), _o("minmax_dev", N * 2 * 8, 8)],
    lambda a: [None, a["in"], F64, 1.0, a["out"], N, H, W, _p(_W3), 1, 0, 0.0, 2 * PX, a["minmax_dev"]], host=("weights",),
    note="fused kernel (radius <= 12) reads a halo that neighbour tiles overwrite; two-pass form is right only through scratch")
row("amt_gaussian_otsu_codes",
    [_i("in", N * PX * 2, 2), _o("minmax_dev", N * 16, 8), _o("hist_dev", N * 256 * 4, 4), _o("thr_dev", N * 8, 8),
     _o("thr_code_dev", N * 8, 8), _o("codes", N * PX * 2, 2), _o("prefix", N * PX * 4, 4)],
    lambda a: [None, a["in"], 1.0, N, H, W, _p(_W3), 1, 0, 0, a["minmax_dev"], a["hist_dev"], a["thr_dev"], a["thr_code_dev"],
               a["codes"], a["prefix"]], host=("weights",))
row("amt_convolve_axis0", [_i("in", N * PX * 8, 8), _o("out", N * PX * 8, 8)],
    lambda a: [None, a["in"], F64, 1.0, a["out"], N, H, W, _p(_W3), 1, 0, 0.0], host=("weights",))
row("amt_dog", [_i("in", N * PX * 8, 8), _o("out", N * PX * 8, 8)],
    lambda a: [None, a["in"], F64, 1.0, a["out"], N, H, W, _p(_W3), 1, _p(_W3), 1, 0, 0.0], host=("w_lo", "w_hi"),
    note="the first Gaussian is written to out before the second reads in")
row("amt_sub_clip0_f64", [_i("in", N * PX * 8, 8), _i("level_dev", N * 8, 8), _o("out", N * PX * 8, 8)],
    lambda a: [None, a["in"], a["level_dev"], a["out"], N, PX], inplace=[("out", "in")])
row("amt_rescale", [_i("in", N * PX * 8, 8), _i("range_dev", N * 16, 8), _o("out", N * PX * 8, 8)],
    lambda a: [None, a["in"], F64, a["range_dev"], 0.0, 1.0, a["out"], N, PX], inplace=[("out", "in")],
    note="float64 input only: uint16 input has another element size")
row("amt_convert_u16_f64", [_i("in", N * PX * 2, 2), _o("out", N * PX * 8, 8)], lambda a: [None, a["in"], 1.0, a["out"], N * PX])
row("amt_add_scalar_f64", [_i("in", N * PX * 8, 8), _o("out", N * PX * 8, 8)], lambda a: [None, a["in"], 1.0, a["out"], N * PX],
    inplace=[("out", "in")])
row("amt_pad_edge", [_i("src", N * PX * 2, 2), _o("dst", N * (H + 4) * (W + 2) * 2, 2)],
    lambda a: [None, a["src"], a["dst"], 2, N, H, W, 2, 1])
row("amt_copy_rect", [_i("src", N * PX * 2, 2), _o("dst", N * 2 * 3 * 2, 2)],
    lambda a: [None, a["src"], a["dst"], 2, N, H, W, 1, 1, 2, 3])
row("amt_subtract", [_i("a", N * PX * 8, 8), _i("b", N * PX * 8, 8), _o("out", N * PX * 8, 8)],
    lambda a: [None, a["a"], a["b"], a["out"], F64, N * PX], inplace=[("out", "a"), ("out", "b")])
# ---- statistics and thresholds ---------------------------------------------------------------------------------------------
row("amt_hist_u16", [_i("in", N * PX * 2, 2), _o("hist", N * 65536 * 4, 4)], lambda a: [None, a["in"], a["hist"], N, PX])
row("amt_hist_range_f64", [_i("in", N * PX * 8, 8), _o("hist", N * NBINS * 4, 4)],
    lambda a: [None, a["in"], 0.0, NBINS, a["hist"], N, PX])
row("amt_minmax_f64", [_i("in", N * PX * 8, 8), _o("minmax_dev", N * 16, 8)], lambda a: [None, a["in"], a["minmax_dev"], N, PX])
row("amt_hist_f64", [_i("in", N * PX * 8, 8), _i("minmax_dev", N * 16, 8), _o("hist", N * NBINS * 4, 4)],
    lambda a: [None, a["in"], a["minmax_dev"], a["hist"], NBINS, N, PX])
row("amt_percentile_u16", [_i("in", N * PX * 2, 2), _o("out_dev", N * NQ * 8, 8)],
    lambda a: [None, a["in"], _p(_Q), NQ, a["out_dev"], N, PX], host=("q_host",))
row("amt_percentile_f64", [_i("in", N * PX * 8, 8), _o("out_dev", N * NQ * 8, 8)],
    lambda a: [None, a["in"], _p(_Q), NQ, a["out_dev"], N, PX], host=("q_host",))
row("amt_masked_sums_f64", [_i("in", N * PX * 8, 8), _i("thr_dev", N * 8, 8), _o("out_dev", N * 32, 8)],
    lambda a: [None, a["in"], a["thr_dev"], a["out_dev"], N, PX])
row("amt_threshold_value", [_i("in", N * PX * 8, 8), _o("thr_dev", N * 8, 8), _o("status_dev", N * 4, 4), _i("minmax_dev", N * 16, 8)],
    lambda a: [None, a["in"], F64, 0, 256, a["thr_dev"], a["status_dev"], N, PX, a["minmax_dev"]])
row("amt_threshold_gt", [_i("in", N * PX * 8, 8), _i("thr_dev", N * 8, 8), _o("out", N * PX, 1)],
    lambda a: [None, a["in"], F64, a["thr_dev"], a["out"], N, PX])
row("amt_window_threshold", [_i("in", N * PX * 8, 8), _o("thr_image", N * PX * 8, 8)],
    lambda a: [None, a["in"], F64, a["thr_image"], N, H, W, 3, 3, 0, 0.2, 1.0],
    note="the window sums of a pixel read what a neighbour's thread wrote")
# nplanes = the product of lead_shape
row("amt_window_threshold_nd", [_i("in", N * PX * 8, 8), _o("thr_image", N * PX * 8, 8)],
    lambda a: [None, a["in"], F64, a["thr_image"], 1, _p(_LEAD), _p(_LWIN), H, W, 3, 3, 0, 0.2, 1.0],
    host=("lead_shape", "lead_window"))
row("amt_threshold_gt_image", [_i("in", N * PX * 8, 8), _i("thr_image", N * PX * 8, 8), _o("out", N * PX, 1)],
    lambda a: [None, a["in"], F64, a["thr_image"], a["out"], N * PX])
# ---- morphology and rank filters ---------------------------------------------------------------------------------------------
row("amt_binary_morph", [_i("in", N * PX, 1), _o("out", N * PX, 1)],
    lambda a: [None, a["in"], a["out"], N, H, W, _p(_FP), 3, 3, 0, 1], host=("footprint",),
    note="codes 0-3 are right in place only because the packed words sit in scratch; codes 4-6 read planes they overwrite")
row("amt_otsu_f64_bins", [_i("in", N * PX * 8, 8), _i("minmax_dev", N * 16, 8), _o("thr_dev", N * 8, 8),
                          _o("thr_code_dev", N * 8, 8), _o("bins", N * PX, 1)],
    lambda a: [None, a["in"], a["minmax_dev"], a["thr_dev"], a["thr_code_dev"], a["bins"], N, PX])
row("amt_threshold_open_close", [_i("in", N * PX * 8, 8), _i("thr_dev", N * 8, 8), _o("out", N * PX, 1), _i("bins", N * PX, 1),
                                 _i("thr_code_dev", N * 8, 8)],
    lambda a: [None, a["in"], F64, a["thr_dev"], a["out"], N, H, W, _p(_FP), 3, 3, a["bins"], a["thr_code_dev"]],
    host=("footprint",))
row("amt_rank_filter", [_i("in", N * PX * 2, 2), _o("out", N * PX * 2, 2), _i("minuend", N * PX * 2, 2)],
    lambda a: [None, a["in"], a["out"], U16, N, H, W, _p(_FP), 3, 3, 0, 0, 0.0, a["minuend"]], host=("footprint",))
# ---- labelling --------------------------------------------------------------------------------------------------------------
row("amt_label", [_i("in", N * PX * 4, 4), _o("out", N * PX * 4, 4), _o("count_dev", N * 4, 4)],
    lambda a: [None, a["in"], I32, a["out"], a["count_dev"], N, H, W, 2])
row("amt_label_mask", [_i("mask", N * PX, 1), _o("out", N * PX * 4, 4), _o("count_dev", N * 4, 4)],
    lambda a: [None, a["mask"], a["out"], a["count_dev"], N, H, W, 2])
row("amt_label_sparse", [_i("in", N * PX, 1), _o("out", N * PX * 4, 4), _o("count_dev", N * 4, 4), _o("keep_list", N * CAP * 4, 4),
                         _o("keep_count", N * 4, 4)],
    lambda a: [None, a["in"], a["out"], a["count_dev"], N, H, W, 2, CAP, a["keep_list"], a["keep_count"]],
    inout=("out", "keep_list", "keep_count"))
row("amt_clear_border", [_i("in", N * PX * 4, 4), _o("out", N * PX * 4, 4)], lambda a: [None, a["in"], a["out"], N, H, W],
    inplace=[("out", "in")])
row("amt_relabel_sequential", [_i("in", N * PX * 4, 4), _o("out", N * PX * 4, 4), _o("count_dev", N * 4, 4)],
    lambda a: [None, a["in"], a["out"], a["count_dev"], N, PX, K], inplace=[("out", "in")])
row("amt_clear_border_relabel", [_i("in", N * PX * 4, 4), _o("out", N * PX * 4, 4), _o("count_dev", N * 4, 4),
                                 _i("nlabels_dev", N * 4, 4)],
    lambda a: [None, a["in"], a["out"], a["count_dev"], N, H, W, K, a["nlabels_dev"]], inplace=[("out", "in")])
row("amt_keep_labels", [_i("in", N * PX * 4, 4), _i("keep_dev", N * (K + 1), 1), _o("out", N * PX * 4, 4)],
    lambda a: [None, a["in"], a["keep_dev"], a["out"], N, PX, K], inplace=[("out", "in")])
row("amt_cast_i32_i64", [_i("in", N * PX * 4, 4), _o("out", N * PX * 8, 8)], lambda a: [None, a["in"], a["out"], N * PX])
row("amt_cast_labels", [_i("in", N * PX * 2, 2), _o("out", N * PX * 4, 4)], lambda a: [None, a["in"], U16, a["out"], I32, N * PX])
row("amt_expand_labels", [_i("labels", N * PX * 4, 4), _o("out", N * PX * 4, 4)],
    lambda a: [None, a["labels"], a["out"], N, H, W, 4, 0])
# ---- distance transform, markers, watershed -------------------------------------------------------------------------------------
row("amt_edt", [_i("mask", N * PX, 1), _o("d2_out", N * PX * 4, 4), _o("edt_out", N * PX * 8, 8)],
    lambda a: [None, a["mask"], a["d2_out"], a["edt_out"], N, H, W])
row("amt_peak_mask", [_i("d2", N * PX * 4, 4), _i("mask", N * PX, 1), _o("peaks", N * PX, 1), _i("prev_list", N * CAP * 4, 4),
                      _i("prev_count", N * 4, 4), _i("prev_status", N * 4, 4)],
    lambda a: [None, a["d2"], a["mask"], a["peaks"], N, H, W, 1, a["prev_list"], a["prev_count"], CAP, a["prev_status"]],
    inout=("peaks",))
row("amt_peak_markers", [_i("d2", N * PX * 4, 4), _i("mask", N * PX, 1), _o("peaks", N * PX, 1), _o("markers", N * PX * 4, 4),
                         _o("count_dev", N * 4, 4), _o("keep_list", N * CAP * 4, 4), _o("keep_count", N * 4, 4)],
    lambda a: [None, a["d2"], a["mask"], a["peaks"], a["markers"], a["count_dev"], N, H, W, 1, 1, CAP, a["keep_list"],
               a["keep_count"]], inout=("peaks", "markers", "count_dev", "keep_list", "keep_count"))
row("amt_watershed_edt", [_i("d2", N * PX * 4, 4), _i("markers", N * PX * 4, 4), _i("mask", N * PX, 1), _o("out", N * PX * 4, 4),
                          _o("ties_dev", N * 4, 4)],
    lambda a: [None, a["d2"], a["markers"], a["mask"], a["out"], N, H, W, 1, 1, 0, a["ties_dev"]])
row("amt_watershed_f64", [_i("relief", N * PX * 8, 8), _i("markers", N * PX * 4, 4), _i("mask", N * PX, 1),
                          _o("out", N * PX * 4, 4), _o("ties_dev", N * 4, 4)],
    lambda a: [None, a["relief"], a["markers"], a["mask"], a["out"], N, H, W, 1, 0, a["ties_dev"]])
row("amt_watershed_edt_cleared",
    [_i("d2", N * PX * 4, 4), _i("markers", N * PX * 4, 4), _i("mask", N * PX, 1), _o("ws_scratch", N * PX * 4, 4),
     _o("labels_out", N * PX * 4, 4), _o("count_dev", N * 4, 4), _i("nlabels_dev", N * 4, 4), _i("marker_list", N * CAP * 4, 4),
     _i("marker_count", N * 4, 4)],
    lambda a: [None, a["d2"], a["markers"], a["mask"], a["ws_scratch"], a["labels_out"], a["count_dev"], N, H, W, K,
               a["nlabels_dev"], a["marker_list"], a["marker_count"], CAP])
# ---- region properties, colocalisation, plate rows, outlines ----------------------------------------------------------------------
row("amt_regionprops", [_i("labels", N * PX * 4, 4), _i("intensity", N * C * PX * 2, 2), _o("table_dev", N * K * 14 * 8, 8),
                        _o("itable_dev", N * K * C * 4 * 8, 8)],
    lambda a: [None, a["labels"], a["intensity"], C, a["table_dev"], a["itable_dev"], N, H, W, K])
row("amt_regionprops_intensity_f64", [_i("labels", N * PX * 4, 4), _i("intensity", N * C * PX * 8, 8),
                                      _o("table_dev", N * K * C * 4 * 8, 8)],
    lambda a: [None, a["labels"], a["intensity"], C, a["table_dev"], N, H, W, K])
# columns = euler number | weighted centroids: both tables
row("amt_regionprops_ext", [_i("labels", N * PX * 4, 4), _i("intensity", N * C * PX * 2, 2), _o("table_dev", N * K * 12 * 8, 8),
                            _o("wtable_dev", N * K * C * 4 * 8, 8)],
    lambda a: [None, a["labels"], a["intensity"], U16, C, 1 | 128, a["table_dev"], a["wtable_dev"], N, H, W, K],
    note="labels and the companion planes are both inputs: the RELATE companion may be labels itself")
row("amt_max_i32", [_i("in", N * PX * 4, 4), _o("max_dev", N * 4, 4)], lambda a: [None, a["in"], a["max_dev"], N, PX])
row("amt_colocalization", [_i("labels", N * PX * 4, 4), _i("intensity", N * C * PX * 2, 2), _i("thresholds_dev", N * C * 8, 8),
                           _o("table_dev", N * K * NPAIRS * 6 * 8, 8)],
    lambda a: [None, a["labels"], a["intensity"], U16, C, a["thresholds_dev"], _p(_PAIRS), NPAIRS, a["table_dev"], N, H, W, K],
    host=("pairs_host",))
row("amt_pack_plate_rows", [_i("table_dev", N * K * 14 * 8, 8), _i("itable_dev", N * K * C * 32, 8), _i("ncells_dev", N * 4, 4),
                            _i("fov_index_dev", N * 4, 4), _o("rows_dev", N * K * (16 + 4 * C) * 8, 8), _o("nrows_dev", 8, 8)],
    lambda a: [None, a["table_dev"], a["itable_dev"], a["ncells_dev"], N, K, C, a["fov_index_dev"], 0, a["rows_dev"], N * K,
               a["nrows_dev"]])
row("amt_label_bboxes", [_i("labels", N * PX * 4, 4), _o("bbox_dev", N * K * 16, 4)],
    lambda a: [None, a["labels"], a["bbox_dev"], N, H, W, K])
row("amt_contours_find", [_i("labels", PX * 4, 4), _i("boxes_dev", NLAB * 20, 4), _i("voff_dev", (NLAB + 1) * 8, 8),
                          _o("visited_dev", 40, 1), _o("info_dev", NLAB * 16, 4)],
    lambda a: [None, a["labels"], H, W, NLAB, a["boxes_dev"], a["voff_dev"], a["visited_dev"], 40, a["info_dev"]])
# the length of points_dev is poff_dev[nlab], known on the device only: the library sees its first point
row("amt_contours_emit", [_i("labels", PX * 4, 4), _i("boxes_dev", NLAB * 20, 4), _i("info_dev", NLAB * 16, 4),
                          _i("poff_dev", (NLAB + 1) * 8, 8), _o("points_dev", 16, 8)],
    lambda a: [None, a["labels"], H, W, NLAB, a["boxes_dev"], a["info_dev"], a["poff_dev"], a["points_dev"]],
    note="points_dev: only its first 16 bytes can be checked on the host")
row("amt_borders_find", [_i("labels", PX * 4, 4), _i("boxes_dev", NLAB * 20, 4), _o("marks_dev", PX, 1), _o("info_dev", NLAB * 12, 4)],
    lambda a: [None, a["labels"], H, W, NLAB, a["boxes_dev"], a["marks_dev"], a["info_dev"]])
row("amt_borders_emit", [_i("labels", PX * 4, 4), _i("boxes_dev", NLAB * 20, 4), _i("info_dev", NLAB * 12, 4),
                         _i("poff_dev", (NLAB + 1) * 8, 8), _o("points_dev", 8, 4)],
    lambda a: [None, a["labels"], H, W, NLAB, a["boxes_dev"], a["info_dev"], a["poff_dev"], a["points_dev"]],
    note="points_dev: only its first 8 bytes can be checked on the host")
# ---- cellpose ------------------------------------------------------------------------------------------------------------------
row("amt_cellpose_masks_ex", [_i("dP", N * 2 * PX * 4, 4), _i("cellprob", N * PX * 4, 4), _o("labels_out", N * PX * 4, 4),
                              _o("count_dev", N * 4, 4)],
    lambda a: [None, a["dP"], a["cellprob"], a["labels_out"], a["count_dev"], N, H, W, 0.0, 10, 0, 0.4, 16, 0.0, 0])
row("amt_fill_holes_remove_small", [_o("labels_io", N * PX * 4, 4), _i("nlabels_dev", N * 4, 4), _o("count_dev", N * 4, 4)],
    lambda a: [None, a["labels_io"], a["nlabels_dev"], a["count_dev"], N, H, W, K, 0, 1], inout=("labels_io",))
row("amt_cellpose_flow_error", [_i("labels", N * PX * 4, 4), _i("dP", N * 2 * PX * 4, 4), _i("nlabels_dev", N * 4, 4),
                                _o("err_out", N * K * 8, 8)],
    lambda a: [None, a["labels"], a["dP"], a["nlabels_dev"], a["err_out"], N, H, W, K])


# ---- overlay: the layers' device pointers travel inside the host table layers_host -----------------------------------------------
def _overlay_args(a):
    table = (ctypes.c_void_p * 2)(a["layers_host[0]"], a["layers_host[1]"])
    _overlay_args.keep = table  # alive until the call returns
    return [None, a["background"], ctypes.addressof(table), 2, _p(_LUTS), _p(_OPAC), _p(_MODE), a["out_rgb"], H, W]


row("amt_overlay", [_i("background", PX * 8, 8), _o("out_rgb", PX * 24, 8), _i("layers_host[0]", PX * 8, 8),
                    _i("layers_host[1]", PX * 8, 8)], _overlay_args,
    host=("layers_host", "luts_host", "opacity_host", "mode_host"))
# ---- network glue, normalisation ------------------------------------------------------------------------------------------------
_NC = 8
row("amt_nn_affine_act_bf16",
    [_i("x", N * PX * _NC * 2, 2), _i("y", N * PX * _NC * 2, 2), _i("style", N * _NC * 4, 4), _i("pre_bias", _NC * 4, 4),
     _i("scale", _NC * 4, 4), _i("shift", _NC * 4, 4), _o("out", N * PX * _NC * 2, 2), _o("sum_out", N * PX * _NC * 2, 2)],
    lambda a: [None, a["x"], a["y"], a["style"], a["pre_bias"], a["scale"], a["shift"], a["out"], a["sum_out"], N, H, W, _NC, 1, 0])
row("amt_normalize_planes_f32", [_i("in", N * PX * 4, 4), _i("lohi_dev", N * 2 * 8, 8), _o("out", N * PX * 4, 4)],
    lambda a: [None, a["in"], F32, a["lohi_dev"], F64, 0, a["out"], N, PX],
    note="float32 in and out have the same size, but the 16-byte path and the scalar tail of neighbouring threads interleave")
row("amt_convert_f32_f64", [_i("in", N * PX * 4, 4), _o("out", N * PX * 8, 8)], lambda a: [None, a["in"], a["out"], N * PX])

BY_NAME = {r.fn: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


def verdict_counts():
    """(pairs judged in place, pairs refused) over the whole table."""
    v = [p[2] for r in ROWS for p in r.pairs()]
    return v.count("in place"), v.count("refused")


# ---- made-up addresses ---------------------------------------------------------------------------------------------------------
BASE, GAP = 1 << 24, 1 << 22  # operands 4 MiB apart: far more than the longest of them


def addresses(r):
    """Every operand of the row at an address of its own."""
    return {o[0]: BASE + k * GAP for k, o in enumerate(r.operands)}


def shifts(o, x):
    """The overlapping placements of output ``o`` against operand ``x`` (offsets of o's start from x's): exact alias, one
    plane forward and backward (a third of a batch operand; none for operands of a single plane), 8 bytes forward."""
    cand = [("exact", 0), ("8 bytes", 8)]
    for arr in (o, x):
        if arr[2] % N == 0 and arr[2] // N >= arr[3]:
            plane = arr[2] // N
            cand += [("plane forward", plane), ("plane backward", -plane)]
    seen, out = set(), []
    for name, s in cand:
        if -o[2] < s < x[2] and s not in seen:  # the spans really intersect
            seen.add(s)
            out.append((name, s))
    return out
