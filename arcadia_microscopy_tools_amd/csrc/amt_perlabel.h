// Device helpers of the per-label kernels: one wave per (label, plane) over the label's bounding box (amt_props.hip,
// amt_relate.hip, amt_robust.hip).  The box and the row of a label that is absent from its plane, the
// lane layouts and the walk over a box in two planes, and the wave reductions.
#pragma once
#include "amt_common.h"

#ifdef __HIPCC__
// bbox ints per (plane, label): miny, minx, maxy, maxx, all inclusive; amt_i_label_boxes (amt_internal.h) makes them
struct amt_box {
    int y0, x0, y1, x1;
    __device__ __forceinline__ bool absent() const { return y1 < y0; }  // the label has no pixel in its plane
    __device__ __forceinline__ int w() const { return x1 - x0 + 1; }
    __device__ __forceinline__ int h() const { return y1 - y0 + 1; }
};
__device__ __forceinline__ amt_box amt_load_box(const int* __restrict__ bbox, size_t li) {
    return {bbox[li * 4 + 0], bbox[li * 4 + 1], bbox[li * 4 + 2], bbox[li * 4 + 3]};
}

// the table row of an absent label: `count` doubles of `value`, written by the wave
__device__ __forceinline__ void amt_fill_row(double* __restrict__ out, int count, double value, int lane) {
    for (int i = lane; i < count; i += 64) out[i] = value;
}
__device__ __forceinline__ double amt_quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// lc for the columns x0 .. x1: the wave covers 2^lc columns x (64 >> lc) rows per row slot, 8 x 8, 16 x 4 and 32 x 2 for
// boxes of at most 8 / 16 / 32 columns (a nucleus: ~28 of 64 lanes of a 64 x 1 slot hold a pixel of the box), 64 x 1
// otherwise.  Takes the two columns, not the width: "x1 - x0 + 1 <= 8" inside a callee is no longer folded to
// "x1 - x0 < 8" once it is inlined, which costs every kernel an instruction.
__device__ __forceinline__ int amt_box_layout(int x0, int x1) {
    const int d = x1 - x0;
    return d < 8 ? 3 : (d < 16 ? 4 : (d < 32 ? 5 : 6));
}

// f(v) for the value v of plane I under every pixel of the label `want` of plane L, each pixel once.  Two row slots per
// step, their four loads issued together from coordinates clamped into the box; what lies outside the box or the label
// is discarded where it is used.
template <typename T, typename F>
__device__ __forceinline__ void amt_box_for_pixels(const int* __restrict__ L, const T* __restrict__ I, int W,
                                                   const amt_box& box, int want, int lc, int lane, F&& f) {
    const int x0 = box.x0, y0 = box.y0, x1 = box.x1, y1 = box.y1;
    const int cols = 1 << lc, rw = 64 >> lc;
    const int col = lane & (cols - 1), sub = lane >> lc;
    for (int yb = y0 + sub; yb - sub <= y1; yb += 2 * rw) {
        const int ya = yb, yc = yb + rw;
        const size_t ra = (size_t)(ya <= y1 ? ya : y1) * W, rc = (size_t)(yc <= y1 ? yc : y1) * W;
        for (int xb = x0; xb <= x1; xb += cols) {
            const int x = xb + col, xc = x <= x1 ? x : x1;
            const int la = L[ra + xc], lb = L[rc + xc];
            const T va = I[ra + xc], vb = I[rc + xc];
            if (x <= x1 && ya <= y1 && la == want) f(va);
            if (x <= x1 && yc <= y1 && lb == want) f(vb);
        }
    }
}

// f(x, y) for the cell of every lane in every row slot and column tile of the box, in the lane layout above, one row slot
// per step: for kernels that need a pixel's coordinates (its partners at an offset) rather than its value.  Cells beyond
// x1 / y1 are handed over too (a lane of the last tile): the callee drops them, or clamps them for loads it issues.
template <typename F>
__device__ __forceinline__ void amt_box_for_cells(const amt_box& box, int lc, int lane, F&& f) {
    const int cols = 1 << lc, rw = 64 >> lc;
    const int col = lane & (cols - 1), sub = lane >> lc;
    for (int yb = box.y0; yb <= box.y1; yb += rw)
        for (int xb = box.x0; xb <= box.x1; xb += cols) f(xb + col, yb + sub);
}

// The same walk with a value per cell, f(x, y, v) with v = load(yc, xc) from the coordinates clamped into the box: four
// row slots per step, their four loads issued together before the first f runs (f may wait on LDS, which would
// otherwise put every load's latency into the loop one after the other).
template <typename Ld, typename F>
__device__ __forceinline__ void amt_box_for_loaded_cells(const amt_box& box, int lc, int lane, Ld&& load, F&& f) {
    const int cols = 1 << lc, rw = 64 >> lc;
    const int col = lane & (cols - 1), sub = lane >> lc;
    const int x1 = box.x1, y1 = box.y1;
    for (int yb = box.y0 + sub; yb - sub <= y1; yb += 4 * rw)
        for (int xb = box.x0; xb <= x1; xb += cols) {
            const int x = xb + col, xc = x <= x1 ? x : x1;
            const int ya = yb, yc = yb + rw, yd = yb + 2 * rw, ye = yb + 3 * rw;
            const auto va = load(ya <= y1 ? ya : y1, xc), vc = load(yc <= y1 ? yc : y1, xc);
            const auto vd = load(yd <= y1 ? yd : y1, xc), ve = load(ye <= y1 ? ye : y1, xc);
            f(x, ya, va);
            f(x, yc, vc);
            f(x, yd, vd);
            f(x, ye, ve);
        }
}

// ---- wave reductions: the butterfly over the lanes 32, 16, .. 1 away; every lane gets the result -----------------------
// float64 sums depend on this order: the tables of the float64 kernels keep their bits only while it stands.
struct amt_op_sum {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct amt_op_min {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};
struct amt_op_max {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};
template <typename Op, typename T>
__device__ __forceinline__ T amt_wave_reduce(T v, int from = 32) {
#pragma unroll
    for (int off = from; off >= 1; off >>= 1) v = Op()(v, __shfl_xor(v, off));
    return v;
}
template <typename T>
__device__ __forceinline__ T amt_wave_sum(T v) { return amt_wave_reduce<amt_op_sum>(v); }
template <typename T>
__device__ __forceinline__ T amt_wave_min(T v) { return amt_wave_reduce<amt_op_min>(v); }
template <typename T>
__device__ __forceinline__ T amt_wave_max(T v) { return amt_wave_reduce<amt_op_max>(v); }

// N values per lane reduced over the wave for N - 1 + log2(64 / N) exchanges (one all-reduce each takes 6 N): every step
// halves what a lane still carries -- it keeps one half of its values, hands the other half to the lane 64 / N * HALF away
// and folds in what that lane hands over; the last levels are an all-reduce.  On return lane L holds the wave's result
// of value (L / (64 / N)) % N.  For integer sums and minima: any order gives the same bits.
template <int N, int HALF, typename Op, typename T>
__device__ __forceinline__ void amt_wave_scatter_step(T (&t)[N], int lane) {
    constexpr int STRIDE = 64 / N * HALF;
    const bool up = (lane & STRIDE) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const T keep = up ? t[i + HALF] : t[i];
        const T send = up ? t[i] : t[i + HALF];
        t[i] = Op()(keep, __shfl_xor(send, STRIDE));
    }
    if constexpr (HALF > 1) amt_wave_scatter_step<N, HALF / 2, Op>(t, lane);
}
template <int N, typename Op, typename T>
__device__ __forceinline__ T amt_wave_reduce_scatter(T (&t)[N], int lane) {
    static_assert(N == 8 || N == 16 || N == 32, "a power of two below the wave's 64 lanes");
    amt_wave_scatter_step<N, N / 2, Op>(t, lane);
    return amt_wave_reduce<Op>(t[0], 64 / N / 2);
}
#endif
