"""The label boxes that the fused watershed tail hands to the per-label call that directly follows it on its context
("Label boxes from the watershed's tail"): they equal the plane pass integer for integer, the note reaches
only the next image operation, and the chain's tables do not move."""
import numpy as np
import pytest

import label_box_handoff_cases as hc
import poison_child

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _both_box_calls(ctx, make_labels, shape, max_label):
    """Boxes of the call that directly follows the watershed (the hand-off, where the watershed left a note) and of the
    one after it (the plane pass), each against numpy's boxes of the label planes."""
    from arcadia_microscopy_tools_amd import hipops

    # the output array of label_bboxes comes from the context's pool: after this call a block of its size lies there, and
    # the first call below allocates nothing between the watershed and the box pass
    hipops.label_bboxes(ctx.zeros(shape, np.int32), max_label)
    lab = make_labels()
    first = hipops.label_bboxes(lab, max_label)
    second = hipops.label_bboxes(lab, max_label)
    want = hc.numpy_boxes(lab.numpy(), max_label)
    assert np.array_equal(first, want), np.argwhere(first != want)[:8]
    assert np.array_equal(second, want), np.argwhere(second != want)[:8]
    return lab.numpy()


@pytest.fixture(scope="module")
def blob_case():
    masks = hc.blob_planes()
    return masks, hc.peak_markers_of(masks)


def test_boxes_every_flood_class(ctx, blob_case):
    masks, markers = blob_case
    ml = int(markers.max())
    lab = _both_box_calls(ctx, lambda: hc.fused_watershed(ctx, masks, markers, ml), masks.shape, ml)
    assert lab.max() >= 12


@pytest.mark.parametrize("h,w", [(208, 208), (300, 464), (129, 208), (200, 80), (200, 200), (333, 333)])
def test_boxes_windows_with_nuclei_on_the_frame(ctx, h, w):
    """Widths that are a multiple of 16 take the run-table path and leave boxes; 200 and 333 take the parent-plane path and
    leave none.  The last plane is constant: no mask, no markers."""
    from arcadia_microscopy_tools_amd.segment import FovSegmenter

    fovs = hc.framed_windows(h, w)
    seg = FovSegmenter(3, 4, h, w, ctx=ctx, max_cells=256, props=False)
    d = ctx.asarray(fovs)
    lab = _both_box_calls(ctx, lambda: seg.run_c3(d), (3, h, w), 256)
    assert lab[0].max() > 0 and lab[2].max() == 0


def _two_disks(h=96, w=128):
    yy, xx = np.mgrid[0:h, 0:w]
    a = (yy - 40) ** 2 + (xx - 30) ** 2 <= 15 ** 2
    b = (yy - 50) ** 2 + (xx - 90) ** 2 <= 20 ** 2
    return a, b


def test_boxes_plane_without_markers_and_component_without_marker(ctx):
    a, b = _two_disks()
    masks = np.stack([a | b, a | b])
    markers = np.zeros(masks.shape, np.int32)
    markers[1, 40, 30] = 1  # plane 0: no marker at all; plane 1: the second disk has none
    lab = _both_box_calls(ctx, lambda: hc.fused_watershed(ctx, masks, markers, 4), masks.shape, 4)
    assert lab[0].max() == 0 and lab[1].max() == 1


def test_boxes_constant_planes(ctx):
    masks = np.stack([np.zeros((64, 80), bool), np.ones((64, 80), bool)])
    masks[1, 0, 0] = False  # one background pixel, so that the distance transform is defined
    markers = np.zeros(masks.shape, np.int32)
    markers[1, 30, 40] = 1  # the full plane touches the frame: its one label is cleared
    lab = _both_box_calls(ctx, lambda: hc.fused_watershed(ctx, masks, markers, 3), masks.shape, 3)
    assert lab.max() == 0


def test_boxes_more_labels_than_max_label(ctx):
    a, b = _two_disks()
    masks = (a | b)[None]
    markers = np.zeros(masks.shape, np.int32)
    for k, (y, x) in enumerate(((32, 30), (48, 30), (40, 22), (42, 96), (58, 84)), 1):
        markers[0, y, x] = k
    lab = _both_box_calls(ctx, lambda: hc.fused_watershed(ctx, masks, markers, 3), masks.shape, 3)
    assert lab.max() >= 1


def _square_case():
    m = np.zeros((336, 352), bool)
    m[20:320, 30:330] = True  # 300 x 300: more than one wave walks
    mk = np.zeros(m.shape, np.int32)
    mk[100, 100], mk[230, 250] = 1, 2
    return m, mk


def test_boxes_component_above_the_walk_cap(ctx, blob_case):
    m, mk = _square_case()
    lab = _both_box_calls(ctx, lambda: hc.fused_watershed(ctx, m[None], mk[None], 8), (1,) + m.shape, 8)
    assert lab.max() == 2
    # ... and as the middle plane of a batch of three whose other planes are ordinary
    a, b = _two_disks(*m.shape)
    ordinary = a | b
    omk = np.zeros(m.shape, np.int32)
    omk[32, 30], omk[48, 30], omk[50, 90] = 1, 2, 3
    masks, markers = np.stack([ordinary, m, ordinary]), np.stack([omk, mk, omk])
    lab = _both_box_calls(ctx, lambda: hc.fused_watershed(ctx, masks, markers, 8), masks.shape, 8)
    assert lab[0].max() == 3 and lab[1].max() == 2


def test_boxes_one_label_in_two_components(ctx):
    """Markers are the caller's: label 1 seeds two single-label components, and label 2 a single-label component and,
    beside label 3, a flooded one.  The box of such a label is the union, which plain stores per component would miss."""
    yy, xx = np.mgrid[0:96, 0:160]
    disks = [(yy - cy) ** 2 + (xx - cx) ** 2 <= 12 ** 2 for cy, cx in ((20, 20), (70, 60), (25, 100), (70, 130))]
    masks = (disks[0] | disks[1] | disks[2] | disks[3])[None]
    markers = np.zeros(masks.shape, np.int32)
    markers[0, 20, 20] = markers[0, 70, 60] = 1
    markers[0, 25, 100] = 2
    markers[0, 70, 124], markers[0, 70, 136] = 2, 3
    lab = _both_box_calls(ctx, lambda: hc.fused_watershed(ctx, masks, markers, 4), masks.shape, 4)
    assert lab.max() == 3 and lab[0, 20, 20] == lab[0, 70, 60] and lab[0, 25, 100] == lab[0, 70, 124] != lab[0, 70, 136]


def _clear_behind_the_library(arr):
    """Waits for the device and zeroes a device array through the HIP runtime itself: no call of the library, so nothing
    voids a note.  This breaks the hand-off's contract on purpose and is a probe for tests only -- and not for a process
    with AMT_DEBUG_POISON=1, where the library checks every hand-off against the plane pass and rightly fails the call."""
    import ctypes

    assert not poison_child.poisoned(), "this probe breaks the hand-off's contract; run it without AMT_DEBUG_POISON"
    # the HIP runtime the library is bound to, by the path it is mapped from (a second runtime in the process would not
    # see the device)
    with open("/proc/self/maps") as f:
        mapped = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(mapped) == 1, mapped
    hip = ctypes.CDLL(mapped[0])
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemset(ctypes.c_void_p(arr.ptr), 0, arr.nbytes) == 0 and hip.hipDeviceSynchronize() == 0


def test_first_call_takes_the_handoff(ctx):
    """The label planes are cleared behind the library's back.  The call that directly follows the watershed must still
    return the watershed's boxes -- it did not read the planes -- and the one after it the empty boxes of what the planes
    now hold.  Without this, every comparison above would also pass with two plane passes."""
    from arcadia_microscopy_tools_amd import hipops

    a, b = _two_disks()
    masks = (a | b)[None]
    markers = np.zeros(masks.shape, np.int32)
    markers[0, 32, 30], markers[0, 48, 30], markers[0, 50, 90] = 1, 2, 3
    hipops.label_bboxes(ctx.zeros(masks.shape, np.int32), 4)  # primes the pool, see _both_box_calls
    lab = hc.fused_watershed(ctx, masks, markers, 4)
    want = hc.numpy_boxes(np.where(masks, np.where(a, 0, 3), 0).astype(np.int32), 4)  # label 3: the second disk
    _clear_behind_the_library(lab)
    first = hipops.label_bboxes(lab, 4)
    second = hipops.label_bboxes(lab, 4)
    assert np.array_equal(first[0, 2], want[0, 2]) and (first[0, :3, 2] >= first[0, :3, 0]).all()
    assert np.array_equal(second, hc.numpy_boxes(np.zeros(masks.shape, np.int32), 4))


@pytest.mark.parametrize("profile", [False, True])
def test_segmenter_takes_the_handoff(ctx, monkeypatch, profile):
    """Between the two stages of FovSegmenter.run_c3 lie at most a timer's stop and start (profile=True), which void
    nothing: in place of the region-property call the same probe asks for the boxes of the cleared planes and must get
    the watershed's."""
    from arcadia_microscopy_tools_amd import hipops, segment

    fovs = hc.chain_windows()
    seg = segment.FovSegmenter(2, 4, 208, 208, ctx=ctx, max_cells=256, profile=profile)
    d = ctx.asarray(fovs)
    want = hc.numpy_boxes(seg.run_c3(d).numpy(), 256)
    hipops.label_bboxes(seg.labels, 256)  # primes the pool, see _both_box_calls
    got = {}

    def probe(labels, intensity, max_label, out=None, iout=None):
        _clear_behind_the_library(labels)
        got["boxes"] = hipops.label_bboxes(labels, max_label)
        return out, iout

    monkeypatch.setattr(segment.hipops, "regionprops_full", probe)
    seg.run_c3(d)
    assert want[..., 2].max() > 0 and np.array_equal(got["boxes"], want)
    assert seg.labels.numpy().max() == 0


# ---- the note reaches only the next call ----------------------------------------------------------------------------
class _Chain:
    """A segmenter without the region-property stage on the chain windows, and what regionprops_full needs."""

    def __init__(self, ctx):
        from arcadia_microscopy_tools_amd import _hip
        from arcadia_microscopy_tools_amd.segment import FovSegmenter

        self.ctx = ctx
        self.fovs = hc.chain_windows()
        self.d = ctx.asarray(self.fovs)
        self.K = 256
        self.seg = FovSegmenter(2, 4, 208, 208, ctx=ctx, max_cells=self.K, props=False)
        self.tabs = {k: (ctx.empty((2, k, _hip.RP_NCOLS), np.float64), ctx.empty((2, k, 4, 4), np.float64))
                     for k in (self.K, 200)}

    def watershed(self):
        return self.seg.run_c3(self.d)

    def props(self, labels, K=None):
        from arcadia_microscopy_tools_amd import hipops

        K = K or self.K
        o, io = self.tabs[K]
        t, it = hipops.regionprops_full(labels, self.d, K, out=o, iout=io)
        return t.numpy().tobytes(), it.numpy().tobytes()

    def fresh(self, labels, K=None):
        """regionprops_full on a fresh copy of what the label buffer holds: the plane pass."""
        return self.props(self.ctx.asarray(labels.numpy()), K=K)


@pytest.fixture(scope="module")
def chain(ctx):
    return _Chain(ctx)


def test_note_upload_into_the_label_buffer(ctx, chain):
    lab = chain.watershed()
    other = np.roll(lab.numpy(), (7, 11), (1, 2))
    lab = chain.watershed()
    ctx.asarray(other, out=lab)
    assert chain.props(lab) == chain.fresh(lab)
    assert np.array_equal(lab.numpy(), other)


def test_note_keep_labels_in_place(ctx, chain):
    from arcadia_microscopy_tools_amd import hipops

    keep = np.ones((2, chain.K + 1), np.uint8)
    keep[:, 1::2] = 0
    dkeep = ctx.asarray(keep)
    lab = chain.watershed()
    before = lab.numpy()
    hipops.keep_labels(lab, dkeep, chain.K, out=lab)
    assert chain.props(lab) == chain.fresh(lab)
    assert before.max() > 1 and set(np.unique(lab.numpy())) == set(np.unique(before)[::2])


def test_note_sync(ctx, chain):
    lab = chain.watershed()
    ctx.synchronize()
    assert chain.props(lab) == chain.fresh(lab)


def test_note_other_max_label(ctx, chain):
    lab = chain.watershed()
    assert chain.props(lab, K=200) == chain.fresh(lab, K=200)


def test_note_copy_at_another_address(ctx, chain):
    lab = chain.watershed()
    copy = ctx.asarray(lab.numpy())
    lab = chain.watershed()
    assert chain.props(copy) == chain.fresh(lab)


def test_note_second_context(ctx, chain):
    from arcadia_microscopy_tools_amd.device import Context

    other = Context(ctx.device)
    o, io = chain.tabs[chain.K]
    lab = chain.watershed()
    ctx.synchronize()
    from arcadia_microscopy_tools_amd import hipops

    t, it = hipops.regionprops_full(lab.on(other), chain.d.on(other), chain.K, out=o.on(other), iout=io.on(other))
    other.synchronize()
    got = (t.numpy().tobytes(), it.numpy().tobytes())
    assert got == chain.fresh(lab)


@pytest.mark.parametrize("how", ["stream_wait", "event", "event_sync", "timer"])
def test_note_labels_changed_by_a_second_context(ctx, chain, how):
    """Library calls only, no race: the watershed's work is published to a second context (or to the host), which
    changes the labels in place and is waited for; the first context's region properties must see the change."""
    from arcadia_microscopy_tools_amd import hipops
    from arcadia_microscopy_tools_amd.device import Context, Timer

    other = Context(ctx.device)
    keep = np.ones((2, chain.K + 1), np.uint8)
    keep[:, 1::2] = 0
    dkeep = other.asarray(keep)
    ev, t = ctx.event(), Timer(ctx)
    other.synchronize()
    if how == "timer":
        t.start()
    lab = chain.watershed()
    if how == "stream_wait":
        other.wait_for(ctx)
    elif how == "event":
        ev.record(ctx)
        ev.wait(other)
    elif how == "event_sync":
        ev.record(ctx)
        ev.synchronize()
    else:
        t.stop()
        t.elapsed_ms()
    hipops.keep_labels(lab.on(other), dkeep, chain.K, out=lab.on(other))
    other.synchronize()
    got = chain.props(lab)
    assert got == chain.fresh(lab)
    vals = np.unique(lab.numpy())
    assert vals.size > 1 and not (vals % 2).any()


def test_note_two_regionprops(ctx, chain):
    lab = chain.watershed()
    first = chain.props(lab)
    second = chain.props(lab)
    assert first == second == chain.fresh(lab)


# ---- the chain ------------------------------------------------------------------------------------------------------
def test_chain_fused_equals_separate_calls(ctx, tmp_path):
    """Every column of table and itable bit for bit, fused against separate calls, with the stage timers and without;
    then the same in a process whose scratch is poisoned, where the library checks every hand-off against the plane pass."""
    here = hc.chain_digests(ctx)
    for k in ("labels", "ncells", "table", "itable"):
        vals = {here[f"fused={f} profile={p} {k}"] for f in (True, False) for p in (False, True)}
        assert len(vals) == 1, k
    there = poison_child.run_module("tests.label_box_handoff_cases", tmp_path / "handoff.json", 120.0,
                                    "the poisoned chain of the label-box hand-off")
    poison_child.assert_unmoved(here, there["digests"])
