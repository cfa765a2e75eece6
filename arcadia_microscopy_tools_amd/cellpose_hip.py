"""The Cellpose path on MI355X (BASELINE configs[4]): network forward through PyTorch-ROCm (bf16, MFMA) and the
flow -> mask post-processing in HIP (``amt_cellpose_masks_ex``).

The reference wraps ``cellpose.models.CellposeModel`` (R/model.py:160-169, :206-215, :270-290), whose weights are
fetched from the network by name -- unobtainable offline, as is the package itself.  What can be built and measured
here is (a) the post-processing, restated from the published algorithm (csrc/amt_dynamics.hip; oracle:
oracle/cellpose_dynamics.py; **parity unpinned**), and (b) the forward pass of a network of Cellpose's published
U-Net architecture (``CPnetStandIn``, RANDOM weights) to size the MFMA work: its output is meaningless as a
segmentation and is never presented as one.  A real checkpoint is used by passing any ``torch.nn.Module`` that maps
``(N, C, H, W)`` images to ``(N, 3, H, W)`` = (dY, dX, cellprob) as ``SegmentationModel(network=...)``.

PyTorch is plumbing here (device memory, the conv stack on MFMA); the post-processing never touches torch kernels.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _hip, hipops
from .device import Context, DeviceArray, get_context


def _torch():
    import torch

    return torch


def make_standin(in_channels: int = 2, nbase=(32, 64, 128, 256), seed: int = 0):
    """Cellpose's residual U-Net ("CPnet", Stringer et al. 2021, Fig. 1 / Methods): four scales of two residual
    blocks (each two 3x3 convolutions with batch norm + ReLU in front), max-pool downsampling, a 256-d style vector
    (global average of the deepest features, L2-normalised) added into every upsampling block, additive skips, and
    a 1x1 output convolution to 3 maps.  RANDOM weights: an architectural stand-in to measure the forward pass."""
    torch = _torch()
    nn = torch.nn

    def bconv(cin, cout, k):
        return nn.Sequential(nn.BatchNorm2d(cin, eps=1e-5), nn.ReLU(inplace=True), nn.Conv2d(cin, cout, k, padding=k // 2))

    class ResDown(nn.Module):
        def __init__(self, cin, cout):
            super().__init__()
            self.proj = nn.Sequential(nn.BatchNorm2d(cin, eps=1e-5), nn.Conv2d(cin, cout, 1))
            self.conv = nn.ModuleList([bconv(cin, cout, 3), bconv(cout, cout, 3), bconv(cout, cout, 3), bconv(cout, cout, 3)])

        def forward(self, x):
            x = self.proj(x) + self.conv[1](self.conv[0](x))
            return x + self.conv[3](self.conv[2](x))

    class ConvStyle(nn.Module):
        def __init__(self, cin, cout, nstyle):
            super().__init__()
            self.conv = bconv(cin, cout, 3)
            self.full = nn.Linear(nstyle, cout)

        def forward(self, style, x, y=None):
            if y is not None:
                x = x + y
            return self.conv(x + self.full(style)[:, :, None, None])

    class ResUp(nn.Module):
        def __init__(self, cin, cout, nstyle):
            super().__init__()
            self.conv0 = bconv(cin, cout, 3)
            self.c1 = ConvStyle(cout, cout, nstyle)
            self.c2 = ConvStyle(cout, cout, nstyle)
            self.c3 = ConvStyle(cout, cout, nstyle)
            self.proj = nn.Sequential(nn.BatchNorm2d(cin, eps=1e-5), nn.Conv2d(cin, cout, 1))

        def forward(self, x, y, style):
            x = self.proj(x) + self.c1(style, self.conv0(x), y=y)
            return x + self.c3(style, self.c2(style, x))

    class CPnetStandIn(nn.Module):
        def __init__(self):
            super().__init__()
            chans = (in_channels,) + tuple(nbase)
            self.down = nn.ModuleList([ResDown(chans[i], chans[i + 1]) for i in range(len(nbase))])
            self.pool = nn.MaxPool2d(2, 2)
            ups = []
            for i in range(len(nbase) - 1, -1, -1):
                cin = nbase[min(i + 1, len(nbase) - 1)]
                ups.append(ResUp(cin, nbase[i], nbase[-1]))
            self.up = nn.ModuleList(ups)
            self.upsample = nn.Upsample(scale_factor=2, mode="nearest")
            self.out = nn.Sequential(nn.BatchNorm2d(nbase[0], eps=1e-5), nn.ReLU(inplace=True), nn.Conv2d(nbase[0], 3, 1))

        def forward(self, x):
            feats = []
            for i, blk in enumerate(self.down):
                x = blk(self.pool(x) if i > 0 else x)
                feats.append(x)
            style = feats[-1].mean(dim=(2, 3))
            style = style / (style.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-6)
            x = self.up[0](feats[-1], feats[-1], style)
            for j, blk in enumerate(self.up[1:], start=1):
                x = blk(self.upsample(x), feats[-1 - j], style)
            return self.out(x)

    g = torch.Generator().manual_seed(seed)
    net = CPnetStandIn()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) / float(np.sqrt(p[0].numel())))  # fan-in scaling
    return net.eval()


def prepare_network(net, device, dtype="bf16"):
    """Move a flow network to the GPU in the compute dtype (bf16 unless told otherwise), channels-last."""
    torch = _torch()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype]
    return net.to(device=device, dtype=dt, memory_format=torch.channels_last).eval(), dt


def forward_flops(net, x) -> int:
    """FLOPs of one forward pass on ``x`` (torch.utils.flop_counter: 2 x multiply-accumulates of the convolutions and
    linear layers -- the MFMA work; SURVEY.md 8(d) prescribes this counter)."""
    torch = _torch()
    from torch.utils.flop_counter import FlopCounterMode

    with torch.no_grad(), FlopCounterMode(display=False) as fc:
        net(x)
    return int(fc.get_total_flops())


def tensor_as_device_array(t, ctx: Context) -> DeviceArray:
    """A contiguous CUDA tensor's memory as a DeviceArray of ``ctx`` (no copy; the tensor must outlive the view and
    the caller orders the streams)."""
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    torch = _torch()
    np_dtype = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8, torch.float64: np.float64}[t.dtype]
    return DeviceArray(ctx, t.data_ptr(), tuple(t.shape), np_dtype, base=t)


def flows_to_masks(flows, cellprob_threshold: float = 0.0, niter: int | None = None, min_size: int = 15,
                   ctx: Context | None = None, max_seeds: int = 16384, flow_threshold: float = 0.0,
                   fill_holes: bool = False, max_size_fraction: float = 0.4):
    """``(N, 3, H, W)`` float32 network output (dY, dX, cellprob) -- a CUDA tensor or a numpy array -- -> (int32
    labels (N, H, W) DeviceArray, counts (N,) DeviceArray).  ``niter`` defaults to Cellpose's 200; ``flow_threshold``
    > 0 runs the flow-error filter, ``fill_holes`` the hole filling (``hipops.cellpose_masks``)."""
    ctx = ctx or get_context()
    niter = 200 if niter is None or niter == 0 else int(niter)
    keep = None
    if isinstance(flows, np.ndarray):
        f = np.ascontiguousarray(flows, dtype=np.float32)
        d = ctx.asarray(f)
        N, _, H, W = f.shape
    else:
        torch = _torch()
        t = flows.detach().to(torch.float32).contiguous()
        torch.cuda.current_stream(t.device).synchronize()  # the network ran on torch's stream, the kernels run on ctx's
        d = tensor_as_device_array(t, ctx)
        keep = t  # a temporary made here must outlive the kernels that read it (they run on ctx's stream)
        N, _, H, W = t.shape
    if d.shape[1] != 3:
        raise ValueError(f"expected (N, 3, H, W) flows, got {d.shape}")
    # (N, 3, H, W): planes 0..1 of every image are the flows, plane 2 the probability -- two strided views cannot be
    # expressed as DeviceArrays, so the three maps of each image are addressed per image
    labels = ctx.empty((N, H, W), np.int32)
    counts = ctx.empty((N,), np.int32)
    for i in range(N):
        img = d[i]
        hipops.cellpose_masks(img[0:2], img[2], cellprob_threshold, niter, min_size, max_size_fraction,
                              out=labels[i:i + 1].reshape(H, W), count=counts[i:i + 1], max_seeds=max_seeds,
                              flow_threshold=flow_threshold or 0.0, fill_holes=fill_holes)
    if keep is not None:
        ctx.synchronize()  # torch's allocator may hand the block to the next torch op once `keep` dies
    return labels, counts


def tile_starts(L: int, bsize: int, tile_overlap: float = 0.1):
    """Tile origins along one axis as ``cellpose.transforms.make_tiles`` places them: tiles of min(bsize, L) pixels,
    ceil((1 + 2 * overlap) * L / bsize) of them, evenly spaced from 0 to L - tile."""
    tile_overlap = min(0.5, max(0.05, tile_overlap))
    b = min(bsize, L)
    n = 1 if L <= bsize else int(np.ceil((1.0 + 2 * tile_overlap) * L / bsize))
    return np.linspace(0, L - b, n).astype(int), b


def taper_mask(ly: int, lx: int, sig: float = 7.5) -> np.ndarray:
    """``cellpose.transforms._taper_mask``: sigmoid roll-off towards the tile edges (float64, host: a 256 x 256 table)."""
    bsize = max(224, max(ly, lx))
    xm = np.arange(bsize)
    xm = np.abs(xm - xm.mean())
    m = 1 / (1 + np.exp((xm - (bsize / 2 - 20)) / sig))
    m = m * m[:, np.newaxis]
    return m[bsize // 2 - ly // 2: bsize // 2 + ly // 2 + ly % 2, bsize // 2 - lx // 2: bsize // 2 + lx // 2 + lx % 2]


def tiled_forward(net, x, batch_size: int = 8, bsize: int = 256, tile_overlap: float = 0.1):
    """``cellpose``'s ``run_net``: the (C, H, W) image tensor ``x`` is cut into overlapping ``bsize`` tiles, the network
    runs on ``batch_size`` tiles at a time, and the outputs are blended with the taper mask (``average_tiles``).
    Returns (3, H, W) float32.  ``bsize`` <= 0 runs the whole image in one pass."""
    torch = _torch()
    C, H, W = x.shape
    if bsize <= 0:
        with torch.no_grad():
            return net(x[None])[0].to(torch.float32)
    ys, by = tile_starts(H, bsize, tile_overlap)
    xs, bx = tile_starts(W, bsize, tile_overlap)
    origins = [(int(y), int(xx)) for y in ys for xx in xs]
    mask = torch.from_numpy(taper_mask(by, bx).astype(np.float32)).to(x.device)
    out = torch.zeros((3, H, W), dtype=torch.float32, device=x.device)
    navg = torch.zeros((H, W), dtype=torch.float32, device=x.device)
    bs = max(1, int(batch_size))
    for k0 in range(0, len(origins), bs):
        chunk = origins[k0:k0 + bs]
        tiles = torch.stack([x[:, y:y + by, xx:xx + bx] for y, xx in chunk])
        if x.dim() == 3 and tiles.shape[1] > 1:
            tiles = tiles.contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            y_t = net(tiles).to(torch.float32)
        for (y, xx), o in zip(chunk, y_t):
            out[:, y:y + by, xx:xx + bx] += o * mask
            navg[y:y + by, xx:xx + bx] += mask
    return out / navg


_EVAL_KWARGS = ("min_size", "max_size_fraction", "bsize", "tile_overlap", "fill_holes", "max_seeds", "normalize",
                "invert")

# the keys of CellposeModel.eval's ``normalize=`` dict with cellpose 4.0.x's defaults (models.normalize_default;
# ``percentile`` None = (1.0, 99.0))
_NORMALIZE_DEFAULTS = {"normalize": True, "lowhigh": None, "percentile": None, "invert": False, "norm3D": True,
                       "sharpen_radius": 0, "smooth_radius": 0, "tile_norm_blocksize": 0, "tile_norm_smooth3D": 1}
_NORMALIZE_REFUSED = ("sharpen_radius", "smooth_radius", "tile_norm_blocksize")  # implemented nowhere on this route
NORMALIZE_MIN_RANGE = np.float32(1e-3)  # normalize99 leaves a channel at zero unless hi - lo exceeds this


class NormalizePlan(NamedTuple):
    """What ``resolve_normalize`` makes of ``normalize=`` / ``invert=``: exactly one of ``percentile`` (lower, upper)
    and ``lowhigh`` ((channels, 2) float32) is set."""

    percentile: tuple[float, float] | None
    lowhigh: np.ndarray | None
    invert: bool


def resolve_normalize(normalize, invert, channels: int) -> NormalizePlan | None:
    """The ``normalize=`` / ``invert=`` options of ``CellposeModel.eval`` for an image of ``channels`` channels -> a
    ``NormalizePlan``, or None when the image goes to the network as it is (pure host code).

    Restated from cellpose 4.0.x (``models.CellposeModel.eval`` / ``transforms.normalize_img``; the package is not
    importable here: **parity unpinned**).  ``normalize`` is False / None, True (= the defaults) or a dict with the keys
    ``normalize``, ``lowhigh``, ``percentile``, ``invert``, ``norm3D``, ``sharpen_radius``, ``smooth_radius``,
    ``tile_norm_blocksize``, ``tile_norm_smooth3D``; ``invert`` is ORed with the dict's.  An option is implemented or
    refused, never ignored: an unknown key raises ``ValueError``, a non-zero ``sharpen_radius`` / ``smooth_radius`` /
    ``tile_norm_blocksize`` ``TypeError``; ``norm3D`` and ``tile_norm_smooth3D`` have no effect on a 2-D image."""
    inv = bool(invert)
    if normalize is None:
        normalize = False
    if isinstance(normalize, (bool, np.bool_)):
        params = dict(_NORMALIZE_DEFAULTS, normalize=bool(normalize))
    elif isinstance(normalize, dict):
        unknown = sorted(set(normalize) - set(_NORMALIZE_DEFAULTS), key=str)
        if unknown:
            raise ValueError(f"normalize: unknown key(s) {unknown}; recognised: {list(_NORMALIZE_DEFAULTS)}")
        params = {**_NORMALIZE_DEFAULTS, **normalize}
    else:
        raise ValueError(f"normalize must be a bool or a dict, got {type(normalize).__name__}")
    for key in _NORMALIZE_REFUSED:
        if params[key]:
            raise TypeError(f"normalize: '{key}' = {params[key]!r} is not implemented on the network + HIP route "
                            "(only 0 is accepted)")
    inv = inv or bool(params["invert"])
    if not params["normalize"]:
        if inv:
            raise ValueError("invert needs normalize: 1 - x of un-normalised intensities is meaningless")
        return None
    lowhigh, percentile = params["lowhigh"], params["percentile"]
    if lowhigh is not None and percentile is not None:
        raise ValueError("normalize: 'lowhigh' and 'percentile' exclude each other")
    if lowhigh is not None:
        try:
            lh = np.asarray(lowhigh, dtype=np.float32)
        except (TypeError, ValueError) as e:
            raise ValueError(f"normalize: 'lowhigh' must hold numbers ({e})") from e
        if lh.shape == (2,):
            lh = np.broadcast_to(lh, (int(channels), 2))
        if lh.shape != (int(channels), 2):
            raise ValueError(f"normalize: 'lowhigh' must be one (low, high) pair or one pair per channel, shape "
                             f"({channels}, 2); got shape {np.shape(lowhigh)}")
        lh = np.ascontiguousarray(lh)
        if not np.all(lh[:, 1] - lh[:, 0] > NORMALIZE_MIN_RANGE):
            raise ValueError(f"normalize: 'lowhigh' needs high - low > 1e-3 for every channel, got {lh.tolist()}")
        return NormalizePlan(None, lh, inv)
    if percentile is None:
        percentile = (1.0, 99.0)
    try:
        lower, upper = (float(v) for v in percentile)
    except (TypeError, ValueError) as e:
        raise ValueError(f"normalize: 'percentile' must be a (lower, upper) pair, got {percentile!r}") from e
    if not (0 <= lower < upper <= 100):
        raise ValueError(f"normalize: 'percentile' must satisfy 0 <= lower < upper <= 100, got {percentile!r}")
    return NormalizePlan((lower, upper), None, inv)


def normalize_image(image: np.ndarray, plan: NormalizePlan, ctx: Context | None = None, device=None):
    """``([C], H, W)`` image -> the float32 ``(C, H, W)`` CUDA tensor ``CellposeModel.eval`` would hand its network
    (cellpose 4.0.x ``normalize_img`` / ``normalize99``, restated; **parity unpinned**), computed on the device from the
    image in the dtype the caller holds.  Per channel, independently:

    1. ``x32`` = the samples as float32 (uint8 / uint16 / float32 exact; float64 and other integers rounded once);
    2. ``lo, hi`` = the plan's ``lowhigh`` pair, or ``np.percentile(x32.astype(np.float64), p)`` for the plan's two
       percentiles (exact order statistics, linear interpolation in float64), each rounded once to float32;
    3. ``y = (x32 - lo) / (hi - lo)`` (float32: a subtraction, then a division by the float32 difference) if
       ``hi - lo > 1e-3``, else 0 for the whole channel;
    4. ``invert``: ``y = 1 - y``.

    The image is uploaded once (uint16 travels as 2 bytes per sample; uint8 is widened to it on the host, float64 and
    other integers are rounded to float32 there), the percentiles of all channels come from one launch of the
    order-statistics kernels and stay on the device, ``hipops.normalize_planes`` rounds them and writes the tensor.
    Everything runs on ``ctx``'s stream, which is ordered behind torch's current stream before the tensor is written
    and in front of it afterwards (the stream rule); the host waits only for its own upload."""
    torch = _torch()
    ctx = ctx or get_context()
    a = np.asarray(image)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"expected an image of shape ([channel], height, width), got {np.shape(image)}")
    if a.dtype == np.uint8:
        a = a.astype(np.uint16)  # exact; the order-statistics kernels take uint16
    elif a.dtype not in (np.uint16, np.float32):
        a = a.astype(np.float32)
    C, H, W = a.shape
    if plan.lowhigh is not None and plan.lowhigh.shape != (C, 2):
        raise ValueError(f"the plan holds {len(plan.lowhigh)} (low, high) pairs, the image has {C} channel(s)")
    device = torch.device("cuda", ctx.device) if device is None else torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    if device.type != "cuda" or index != ctx.device:
        raise ValueError(f"the context runs on GPU {ctx.device}, the tensor was asked for on {device}")
    d = ctx.asarray(np.ascontiguousarray(a))
    if plan.lowhigh is not None:
        lohi = ctx.asarray(plan.lowhigh)
    else:
        lohi = hipops.percentile(d if d.dtype == np.uint16 else hipops.to_float64(d), plan.percentile)
    y = torch.empty((C, H, W), dtype=torch.float32, device=device)
    cur = torch.cuda.current_stream(y.device)
    side = torch.cuda.ExternalStream(ctx.stream_ptr, device=y.device)
    side.wait_stream(cur)  # torch may have handed out a block that work queued on its stream still uses
    hipops.normalize_planes(d, lohi, invert=plan.invert, out=tensor_as_device_array(y, ctx))
    cur.wait_stream(side)  # the network reads y on torch's stream
    return y


def segment_image(net, image: np.ndarray, device, compute_dtype, *, cellprob_threshold=0.0, niter=None, batch_size=8,
                  flow_threshold=0.4, diameter=30.0, ctx: Context | None = None, min_size: int = 15,
                  max_size_fraction: float = 0.4, bsize: int = 256, tile_overlap: float = 0.1, fill_holes: bool = True,
                  max_seeds: int = 16384, normalize=False, invert: bool = False) -> np.ndarray:
    """One ``([C], H, W)`` image -> int64 labels through ``net`` + the HIP post-processing.  The parameters the
    reference hands to ``CellposeModel.eval`` (R/model.py:206-215) act as they do there:

    * ``diameter``: the image is resized by 30 / diameter (bilinear) before the network and the flows are resized back
      to the image's size before the masks are computed (30 = no resizing);
    * ``batch_size``: tiles per forward pass of the tiled network run (``bsize`` pixels per tile, ``tile_overlap``);
    * ``flow_threshold``: the flow-error filter (0 / None switches it off), ``cellprob_threshold``, ``niter`` (None / 0 =
      200), ``min_size`` (with the hole filling of ``fill_holes_and_remove_small_masks``), ``max_size_fraction``.

    **One difference from ``eval``: the image is NOT normalised unless asked.**  ``eval`` defaults to
    ``normalize=True`` (every channel mapped so that its 1st percentile is 0 and its 99th is 1); this route defaults to
    ``normalize=False`` and gives the network the caller's intensities as float32, because callers and tests of the
    route's earlier versions feed it networks that decode raw values.  A network trained by Cellpose expects
    normalised input: pass ``normalize=True`` with such a checkpoint.  ``normalize=`` (True, or eval's dict:
    ``lowhigh``, ``percentile``, ``invert``, ...) and ``invert=`` are resolved by ``resolve_normalize`` and computed on
    the device by ``normalize_image``, at full resolution before the resize, as Cellpose does; tile normalisation,
    sharpening and smoothing are refused, as is every ``eval`` option not named in ``_EVAL_KWARGS`` (restated from
    cellpose 4.0.x, parity unpinned).

    Tiles smaller than 16 pixels per side cannot pass the four poolings of a U-Net; the (resized) image is padded to a
    multiple of 16 by edge replication and the flows cropped back."""
    torch = _torch()
    shape = np.shape(image)
    if len(shape) not in (2, 3):
        raise ValueError(f"expected an image of shape ([channel], height, width), got {shape}")
    plan = resolve_normalize(normalize, invert, 1 if len(shape) == 2 else shape[0])
    if plan is None:
        a = np.asarray(image, dtype=np.float32)
        if a.ndim == 2:
            a = a[None]
        x = torch.from_numpy(np.ascontiguousarray(a)).to(device=device)
    else:
        x = normalize_image(image, plan, ctx, device)
    C, H, W = x.shape
    rescale = 30.0 / float(diameter)
    Hr, Wr = (H, W) if rescale == 1.0 else (max(1, int(H * rescale)), max(1, int(W * rescale)))
    F = torch.nn.functional
    if (Hr, Wr) != (H, W):
        x = F.interpolate(x[None], size=(Hr, Wr), mode="bilinear", align_corners=False, antialias=False)[0]
    ph, pw = (-Hr) % 16, (-Wr) % 16
    if ph or pw:
        x = F.pad(x[None], (0, pw, 0, ph), mode="replicate")[0]
    y = tiled_forward(net, x.to(compute_dtype), batch_size=batch_size, bsize=bsize, tile_overlap=tile_overlap)
    y = y[:, :Hr, :Wr]
    if (Hr, Wr) != (H, W):
        y = F.interpolate(y[None], size=(H, W), mode="bilinear", align_corners=False, antialias=False)[0]
    y = y[None].contiguous()
    labels, counts = flows_to_masks(y, cellprob_threshold, niter, min_size=min_size, ctx=ctx, max_seeds=max_seeds,
                                    flow_threshold=flow_threshold or 0.0, fill_holes=fill_holes,
                                    max_size_fraction=max_size_fraction)
    c = int(counts.numpy()[0])
    if c < 0:
        raise RuntimeError("the flow field produced more seeds than the post-processing's capacity")
    return labels[0].numpy_int64()


class FusedStandIn:
    """The forward pass of ``make_standin``'s network with its elementwise glue fused (``amt_nn_affine_act_bf16``).

    Eager PyTorch runs one kernel per operation: per convolution a batch norm, a ReLU and up to two additions, each a full
    pass over the activations, and three nearest-neighbour upsamplings -- 27.6 of the forward's 38.6 ms per 8 tiles of
    2 x 1024^2 (rocprofv3), against 10.8 ms of convolutions.  Every convolution of the architecture is "batch norm ->
    [ReLU] -> conv" on a sum of up to three terms (input or its upsampling, skip / residual partner, style vector), so
    one HIP pass prepares each convolution's input; the convolutions themselves stay with MIOpen.  Same weights, same
    graph; fewer bf16 roundings than the eager pass (one per fused group).  ``net`` must come from ``make_standin`` +
    ``prepare_network`` (bf16, channels-last); the torch operations are issued on ``ctx``'s stream."""

    def __init__(self, net, ctx: Context):
        torch = _torch()
        self.net, self.ctx = net, ctx
        p = next(net.parameters())
        if p.dtype != torch.bfloat16:
            raise ValueError("FusedStandIn needs the network in bf16 (prepare_network(..., 'bf16'))")
        self.device = p.device
        self.stream = torch.cuda.ExternalStream(ctx.stream_ptr, device=self.device)
        self._folded = {}
        self._lib = _hip.load_library()

    def _affine(self, bn):
        f = self._folded.get(id(bn))
        if f is None:
            torch = _torch()
            with torch.no_grad():
                scale = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
                shift = bn.bias.float() - bn.running_mean.float() * scale
            f = self._folded[id(bn)] = (scale.contiguous(), shift.contiguous())
        return f

    # An activation travels as (tensor, bias): a convolution is run WITHOUT its bias (the framework would add it in an
    # elementwise pass of its own) and the bias is added by whichever fused pass reads the tensor next.
    def _conv(self, conv, x):
        torch = _torch()
        y = torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding)
        return y, (self._bias(conv) if conv.bias is not None else None)

    def _bias(self, conv):
        f = self._folded.get(id(conv))
        if f is None:
            f = self._folded[id(conv)] = conv.bias.detach().float().contiguous()
        return f

    def _pre(self, bx, by):
        if bx is None or by is None:
            return bx if by is None else by
        key = (id(bx), id(by))
        f = self._folded.get(key)
        if f is None:
            f = self._folded[key] = (bx + by).contiguous()
        return f

    def _glue(self, xb, bn, relu, yb=None, style=None, upsample=False, want_sum=False):
        """One fused pass; ``bn`` = a BatchNorm2d, or None for the identity map (a plain sum)."""
        torch = _torch()
        x, bx = xb
        y, by = yb if yb is not None else (None, None)
        N, C, H, W = x.shape
        if upsample:
            H, W = 2 * H, 2 * W
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        if y is not None and not y.is_contiguous(memory_format=torch.channels_last):
            y = y.contiguous(memory_format=torch.channels_last)
        scale, shift = self._affine(bn) if bn is not None else self._identity(C)
        pre = self._pre(bx, by)
        out = torch.empty((N, C, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        s = torch.empty_like(out) if want_sum else None
        _hip.check(self._lib.amt_nn_affine_act_bf16(self.ctx.handle, x.data_ptr(), y.data_ptr() if y is not None else None,
                                                    style.data_ptr() if style is not None else None,
                                                    pre.data_ptr() if pre is not None else None, scale.data_ptr(),
                                                    shift.data_ptr(), out.data_ptr(), s.data_ptr() if s is not None else None,
                                                    N, H, W, C, 1 if relu else 0, 1 if upsample else 0),
                   "amt_nn_affine_act_bf16")
        return (out, s) if want_sum else out

    def _identity(self, C):
        f = self._folded.get(("id", C))
        if f is None:
            torch = _torch()
            f = self._folded[("id", C)] = (torch.ones(C, device=self.device), torch.zeros(C, device=self.device))
        return f

    def _bconv(self, seq, xb, **kw):
        """nn.Sequential(BatchNorm2d, ReLU, Conv2d) on the fused sum -> (tensor, pending bias)."""
        if xb[0].shape[1] % 8:
            if kw or xb[1] is not None:
                raise ValueError("unfused fallback only for a plain input")
            return seq(xb[0]), None  # the 2-channel input layer
        return self._conv(seq[2], self._glue(xb, seq[0], True, **kw))

    def _proj(self, seq, xb, upsample=False):
        """nn.Sequential(BatchNorm2d, Conv2d 1x1) -> (tensor, pending bias)."""
        if xb[0].shape[1] % 8:
            return seq(xb[0]), None
        return self._conv(seq[1], self._glue(xb, seq[0], False, upsample=upsample))

    def _res_down(self, blk, x):
        xb = (x, None)
        p = self._proj(blk.proj, xb)
        b = self._bconv(blk.conv[1], self._bconv(blk.conv[0], xb))
        g, x1 = self._glue(p, blk.conv[2][0], True, yb=b, want_sum=True)  # x1 = proj + conv path, g = relu(bn(x1))
        d = self._bconv(blk.conv[3], self._conv(blk.conv[2][2], g))
        return self._glue((x1, None), None, False, yb=d)  # x1 + d (+ d's bias)

    def _style(self, cs, style):
        return cs.full(style).float().contiguous()  # (N, cout) float32

    def _res_up(self, blk, x, y, style, upsample):
        xb = (x, None)
        a = self._conv(blk.conv0[2], self._glue(xb, blk.conv0[0], True, upsample=upsample))
        p = self._proj(blk.proj, xb, upsample=upsample)
        b = self._conv(blk.c1.conv[2], self._glue(a, blk.c1.conv[0], True, yb=(y, None), style=self._style(blk.c1, style)))
        g, x1 = self._glue(p, blk.c2.conv[0], True, yb=b, style=self._style(blk.c2, style), want_sum=True)
        c = self._conv(blk.c2.conv[2], g)
        d = self._conv(blk.c3.conv[2], self._glue(c, blk.c3.conv[0], True, style=self._style(blk.c3, style)))
        return self._glue((x1, None), None, False, yb=d)

    def __call__(self, x):
        torch = _torch()
        net = self.net
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.no_grad(), torch.cuda.stream(self.stream):
            feats = []
            for i, blk in enumerate(net.down):
                x = self._res_down(blk, net.pool(x) if i > 0 else x)
                feats.append(x)
            style = feats[-1].mean(dim=(2, 3))
            style = style / (style.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-6)
            x = self._res_up(net.up[0], feats[-1], feats[-1], style, False)
            for j, blk in enumerate(net.up[1:], start=1):
                x = self._res_up(blk, x, feats[-1 - j], style, True)  # the upsampling is read, not made
            y = net.out[2](self._glue((x, None), net.out[0], True))
        cur.wait_stream(self.stream)
        y.record_stream(cur)  # allocated on self.stream, used by the caller on its own: the allocator must know
        return y
