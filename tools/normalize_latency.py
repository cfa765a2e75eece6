"""Preparation of the network input on the Cellpose route: ``cellpose_hip.normalize_image`` (upload in the image's own
dtype + device percentiles + the normalisation kernel) beside (a) the un-normalised preparation (host float32 conversion
+ torch upload) and (b) the host restatement of the normalisation followed by (a) -- what a caller had to do before
``normalize=`` existed.  Warm, median of ``--repeats`` runs; wall-clock times end in a device synchronise, stage times
are HIP events on the context's stream (they include the host's enqueue gaps between launches; the kernel's own time
comes from ``rocprofv3 --kernel-trace --stats -- python tools/normalize_latency.py --kernels-only --sizes 3x2048``,
which only launches the kernel over rotating buffers).  Prints one JSON line per image size."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (bench.py uses the same figure)


def host_restatement(img, percentile=(1.0, 99.0)):
    out = np.empty(img.shape, np.float32)
    for c in range(img.shape[0]):
        x32 = img[c].astype(np.float32)
        lo, hi = (np.float32(np.percentile(x32.astype(np.float64), p)) for p in percentile)
        d = hi - lo
        out[c] = (x32 - lo) / d if d > np.float32(1e-3) else 0.0
    return out


def median_ms(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def event_ms(ctx, fns, repeats, warmup=1):
    """Median over ``repeats`` of the mean time of one call when every function of ``fns`` is launched once between
    two events (the functions work on different buffers, together larger than the 256 MiB Infinity Cache, so that a
    launch finds its operands in HBM)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    timer, ts = ctx.timer(), []
    for _ in range(repeats):
        timer.start()
        for fn in fns:
            fn()
        timer.stop()
        ts.append(timer.elapsed_ms() / len(fns))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--sizes", default="2x1024,3x2048")
    ap.add_argument("--kernels-only", action="store_true", help="launch the normalisation kernel only (for a kernel trace)")
    args = ap.parse_args()
    import torch

    from arcadia_microscopy_tools_amd import cellpose_hip as ch, hipops, synth
    from arcadia_microscopy_tools_amd.device import get_context

    ctx = get_context()
    dev = torch.device("cuda", ctx.device)
    for spec in args.sizes.split(","):
        C, size = (int(v) for v in spec.split("x"))
        img = np.ascontiguousarray(synth.synth_fov(5, size=size)[1:1 + C])
        plan = ch.resolve_normalize(True, False, C)

        def new():
            y = ch.normalize_image(img, plan, ctx, dev)
            torch.cuda.synchronize(dev)
            return y

        def parent(a=img):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(device=dev)
            torch.cuda.synchronize(dev)
            return x

        def host_then_parent():
            return parent(host_restatement(img))

        n = img.size
        nsets = max(2, min(48, -(-(512 << 20) // (n * 6))))  # 2 bytes read + 4 written per sample and set
        sets = [(ctx.asarray(img), ctx.empty(img.shape, np.float32)) for _ in range(nsets)]
        d = sets[0][0]
        lohi = hipops.percentile(d, plan.percentile)
        if args.kernels_only:
            for _ in range(args.repeats):
                for d, o in sets:
                    hipops.normalize_planes(d, lohi, out=o)
            ctx.synchronize()
            print(json.dumps({"image": f"{C}x{size}x{size} uint16", "launches": args.repeats * nsets,
                              "algorithmic_bytes_per_launch": n * 6}), flush=True)
            continue
        same = bool(torch.equal(new(), host_then_parent()))
        t_kernel = event_ms(ctx, [lambda d=d, o=o: hipops.normalize_planes(d, lohi, out=o) for d, o in sets], args.repeats)
        t_pct = event_ms(ctx, [lambda d=d: hipops.percentile(d, plan.percentile, out=lohi) for d, _ in sets], args.repeats)
        t_upload = median_ms(lambda: ctx.asarray(img, out=d), args.repeats)
        row = {
            "image": f"{C}x{size}x{size} uint16", "repeats": args.repeats, "bit_identical_to_host": same,
            "new_prepare_wall_ms": round(median_ms(new, args.repeats), 3),
            "a_unnormalised_prepare_wall_ms": round(median_ms(parent, args.repeats), 3),
            "b_host_normalise_then_a_wall_ms": round(median_ms(host_then_parent, max(20, args.repeats // 2)), 3),
            "upload_u16_wall_ms": round(t_upload, 3), "percentiles_event_ms": round(t_pct, 4),
            "kernel_event_ms": round(t_kernel, 4),
            "kernel_gbs": round(n * 6 / (t_kernel * 1e-3) / 1e9, 1),
            "kernel_fraction_of_hbm_peak": round(n * 6 / (t_kernel * 1e-3) / 1e9 / HBM_PEAK_GBS, 3),
        }
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
