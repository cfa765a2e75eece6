// The census of the same-label pixel graph of a label plane (AMT_RANK_LABEL_CENSUS of amt_rank_filter; the columns
// AMT_LCEN_* are defined in include/amt_hip.h).  On the label skeleton of AMT_RANK_LABEL_SKELETON it gives every cell's
// skeleton pixels, ends, path and junction pixels and the links a length is made of.
//
// One wave per (label, plane) over the label's box, as every per-label kernel (amt_perlabel.h): the centre values of four
// row slots are loaded together, and only a lane whose pixel carries the label looks at its eight neighbours -- on a
// skeleton that is one lane in dozens, and the neighbours' cache lines are the ones the centres came from.  A neighbour
// counts when it lies inside the image and carries the label.  Every count is an integer summed over the wave by the
// butterfly: no atomics, so two runs give identical bytes.
#include "amt_internal.h"
#include "amt_perlabel.h"

__global__ void __launch_bounds__(64) lcen_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                  int* __restrict__ table, int H, int W, int max_label) {
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    int* out = table + li * AMT_LCEN_NCOLS;
    const amt_box box = amt_load_box(bbox, li);
    if (box.absent()) {
        if (lane < AMT_LCEN_NCOLS) out[lane] = 0;
        return;
    }
    const int* L = labels + (size_t)plane * H * W;
    const int want = l + 1;
    const int lc = amt_box_layout(box.x0, box.x1);
    int cnt[AMT_LCEN_NCOLS] = {};
    amt_box_for_loaded_cells(
        box, lc, lane, [&](int y, int x) { return L[(size_t)y * W + x]; },
        [&](int x, int y, int v) {
            if (x > box.x1 || y > box.y1 || v != want) return;
            const bool up = y > 0, down = y + 1 < H, left = x > 0, right = x + 1 < W;
            const int* c = L + (size_t)y * W + x;
            const bool n = up && c[-W] == want, s = down && c[W] == want;
            const bool w = left && c[-1] == want, e = right && c[1] == want;
            const bool nw = up && left && c[-W - 1] == want, ne = up && right && c[-W + 1] == want;
            const bool sw = down && left && c[W - 1] == want, se = down && right && c[W + 1] == want;
            const int deg = (int)n + (int)s + (int)w + (int)e + (int)nw + (int)ne + (int)sw + (int)se;
            cnt[AMT_LCEN_PIXELS] += 1;
            cnt[AMT_LCEN_ISOLATED] += deg == 0;
            cnt[AMT_LCEN_ENDS] += deg == 1;
            cnt[AMT_LCEN_PATH] += deg == 2;
            cnt[AMT_LCEN_JUNCTIONS] += deg >= 3;
            // every pair is counted at its upper (or, in a row, its left) pixel
            cnt[AMT_LCEN_ORTH_LINKS] += (int)e + (int)s;
            cnt[AMT_LCEN_DIAG_LINKS] += (int)(se && !e && !s) + (int)(sw && !w && !s);
        });
#pragma unroll
    for (int k = 0; k < AMT_LCEN_NCOLS; ++k) {
        const int total = amt_wave_sum(cnt[k]);  // a plane has fewer than 2^31 - 1 pixels, and twice as many links at most
        if (lane == k) out[k] = total;
    }
}

// AMT_RANK_LABEL_CENSUS: amt_rank_filter has checked the operands' aliasing; everything else is checked here.  Boxes, then
// the census; asynchronous.
int amt_i_label_census(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W,
                       const uint8_t* footprint, int fh, int fw, int max_label, const void* minuend) {
    AMT_TRY(amt_i_label_op_refusals("label_census", "max_label", in, out, dtype, nplanes, H, W, footprint, fh, fw, max_label,
                                    minuend));
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0 || max_label == 0) return AMT_OK;
    amt_scratch s(ctx);
    amt_buf<int> bbox(s, (size_t)nplanes * max_label * 4);
    AMT_TRY(s.commit());
    AMT_TRY(amt_i_label_boxes(ctx, (const int*)in, bbox, nullptr, nplanes, H, W, max_label));
    hipLaunchKernelGGL(lcen_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, (const int*)in, (const int*)bbox,
                       (int*)out, H, W, max_label);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
