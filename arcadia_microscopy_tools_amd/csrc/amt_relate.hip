// What lies under and around a label (amt_regionprops_ext's AMT_RPX_RELATE, AMT_RPX_NEIGHBORS and AMT_RPX_NEAREST,
// which checks the arguments, makes the bounding boxes and calls the launchers at the end of this file): the census of
// the companion values under a label's pixels and on its ring, and the two nearest labels by centroid.  The columns are
// defined in include/amt_hip.h.
#include "amt_internal.h"
#include "amt_perlabel.h"

typedef unsigned long long u64;

// ---- relate two label images (AMT_RPX_RELATE) -----------------------------------------------------------------------
// One wave per (label, plane) over the label's box, one companion label plane after the other: which companion values
// lie under the label's pixels, and how often.  The (value, count) pairs live in an open-addressed LDS table of
// RL_SLOTS slots (key 0 = empty: a partner is never 0), home slot = value mod RL_SLOTS, linear probing, claimed with a
// compare-and-swap and counted with an add.  A probe sequence visits every slot once and then gives up, so the table
// holds up to RL_SLOTS distinct partners however their values collide, and no lane ever waits for another.  Counts are
// integer sums: the order in which the lanes arrive changes which slot a value gets, never a count.
// A lane keeps the run of equal values it is reading down its column in registers and goes to the table when the value
// changes: a nucleus inside one cell costs a lane one table update, not one per pixel.
// LDS: 2 x 4 x RL_SLOTS = 1 KiB per workgroup of one wave, so the 32-wave cap of a CU binds (8 waves per SIMD), not
// the LDS (160 workgroups' worth).
// More than RL_SLOTS distinct partners (a lane found no slot): the table is dropped and the partners are selected one
// by one in ascending order, one pass over the box each -- the pass that counts partner v also finds the smallest
// value above v.  Every pass raises v, so there are (partners + 1) passes and then it ends.
constexpr int RL_SLOTS = AMT_RELATE_LDS_PARTNERS;
static_assert((RL_SLOTS & (RL_SLOTS - 1)) == 0 && RL_SLOTS >= 64, "slot index by mask; a lane reduces RL_SLOTS / 64 slots");

// add `c` pixels of partner `v` (> 0) to the table; false when all RL_SLOTS slots belong to other values
__device__ __forceinline__ bool rl_table_add(int* keys, unsigned* cnts, int v, unsigned c) {
    unsigned s = (unsigned)v & (RL_SLOTS - 1);
    for (int probe = 0; probe < RL_SLOTS; ++probe) {
        int k = ((volatile int*)keys)[s];  // a key never changes once set: only an empty slot needs the exchange
        if (k == 0) k = atomicCAS(&keys[s], 0, v);  // the value found there, 0 when this lane claimed the slot
        if (k == 0 || k == v) {
            atomicAdd(&cnts[s], c);
            return true;
        }
        s = (s + 1) & (RL_SLOTS - 1);
    }
    return false;
}

// The census of the values one wave is handed: `each(f)` calls f(v) once for every pixel that counts, every call of
// `each` in the same order.  Values <= 0 and the value `skip` are seen and not counted.  total = all values seen,
// counted = those that count, partners = the distinct ones among them, best / bestv = the maximal count of one value and
// the smallest value that has it (0, 0 without any).  keys / cnts: the wave's table of RL_SLOTS slots.
struct rl_census_t {
    unsigned total, counted, partners, best, bestv;
};
template <typename Each>
__device__ __forceinline__ rl_census_t rl_census(int* keys, unsigned* cnts, int lane, int skip, Each&& each) {
    for (int i = lane; i < RL_SLOTS; i += 64) {
        keys[i] = 0;
        cnts[i] = 0;
    }
    __syncthreads();
    rl_census_t r = {0, 0, 0, 0, 0};
    unsigned runc = 0;
    int runv = 0;
    bool full = false;
    each([&](int v) {
        r.total += 1u;
        if (v > 0 && v != skip) r.counted += 1u;
        if (v == runv) {
            runc += 1u;
        } else {
            if (runv > 0 && runv != skip && !full) full = !rl_table_add(keys, cnts, runv, runc);
            runv = v;
            runc = 1u;
        }
    });
    if (runv > 0 && runv != skip && !full) full = !rl_table_add(keys, cnts, runv, runc);
    __syncthreads();
    r.total = (unsigned)amt_wave_sum((u64)r.total);  // a plane has fewer than 2^32 pixels
    r.counted = (unsigned)amt_wave_sum((u64)r.counted);
    if (!__any(full)) {
        for (int i = lane; i < RL_SLOTS; i += 64) {
            const unsigned k = (unsigned)keys[i], cn = cnts[i];
            if (k != 0) {
                r.partners += 1u;
                if (cn > r.best || (cn == r.best && k < r.bestv)) r.best = cn, r.bestv = k;
            }
        }
        r.partners = (unsigned)amt_wave_sum((u64)r.partners);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned ob = __shfl_xor(r.best, o), ov = __shfl_xor(r.bestv, o);
            if (ob > r.best || (ob == r.best && ob != 0 && ov < r.bestv)) r.best = ob, r.bestv = ov;
        }
    } else {
        // smallest value first
        unsigned cur = 0x7fffffffu;
        each([&](int v) {
            if (v > 0 && v != skip && (unsigned)v < cur) cur = (unsigned)v;
        });
        cur = amt_wave_min(cur);
        while (cur != 0x7fffffffu) {
            unsigned cn = 0, next = 0x7fffffffu;
            each([&](int v) {
                if ((unsigned)v == cur) cn += 1u;
                else if (v > 0 && v != skip && (unsigned)v > cur && (unsigned)v < next) next = (unsigned)v;
            });
            cn = (unsigned)amt_wave_sum((u64)cn);
            next = amt_wave_min(next);
            r.partners += 1u;
            if (cn > r.best) r.best = cn, r.bestv = cur;  // ascending values: an equal count keeps the smaller one
            cur = next;  // > the value just counted, or the end mark
        }
    }
    __syncthreads();  // the table may be cleared for the next census
    return r;
}

__global__ void __launch_bounds__(64) rpx_relate_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                        const int* __restrict__ comp, int C, double* __restrict__ wtable,
                                                        int H, int W, int max_label) {
    __shared__ int keys[RL_SLOTS];
    __shared__ unsigned cnts[RL_SLOTS];
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    double* out = wtable + li * (size_t)C * 4;
    const amt_box box = amt_load_box(bbox, li);
    if (box.absent()) {
        amt_fill_row(out, C * 4, 0.0, lane);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* L = labels + (size_t)plane * n;
    const int lc = amt_box_layout(box.x0, box.x1);
    for (int c = 0; c < C; ++c) {
        const int* B = comp + ((size_t)plane * C + c) * n;
        const rl_census_t r = rl_census(keys, cnts, lane, 0, [&](auto&& f) {
            amt_box_for_pixels(L, B, W, box, l + 1, lc, lane, f);
        });
        if (lane == 0) {
            out[c * 4 + AMT_RPX_RCOL_PARENT] = (double)r.bestv;
            out[c * 4 + AMT_RPX_RCOL_OVERLAP] = (double)r.best;
            out[c * 4 + AMT_RPX_RCOL_PARTNERS] = (double)r.partners;
            out[c * 4 + AMT_RPX_RCOL_AREA] = (double)r.total;
        }
    }
}

// ---- a label's neighbours (AMT_RPX_NEIGHBORS) -----------------------------------------------------------------------
// The same census, taken on the label's RING: the pixels that do not carry the label and have an 8-neighbour that does.
// One wave per (label, plane) over the label's box grown by one pixel and clamped to the plane (outside it no pixel has
// such a neighbour).  The wave covers 2^lc columns; its 64 >> lc lane groups share the rows of the grown box in bands of
// consecutive rows, and a lane walks down its column of its band.  With m = (labels == label) and h = m of the pixel
// and its two neighbours in the row, a pixel is on the ring when it is not m and h of its row, the row above or the row
// below is set: a lane carries h of the rows y - 1 and y, gets m of x - 1 / x + 1 in row y + 1 from the lanes beside it
// and, in the first and last column of the tile, from one halo load -- two loads per lane and row instead of nine.
// Rows go four at a time, their loads issued together from coordinates clamped into the grown box; the companion is read
// only where a row of the four has a ring pixel in the wave, and not at all when it is the label plane itself.
constexpr int NB_ROWS = 4;
template <typename F>
__device__ __forceinline__ void nb_for_ring(const int* __restrict__ L, const int* __restrict__ B, int W, int gx0, int gy0,
                                            int gx1, int gy1, int want, int lc, int lane, F&& f) {
    const int cols = 1 << lc, rw = 64 >> lc;
    const int col = lane & (cols - 1), sub = lane >> lc;
    const int bh = (gy1 - gy0 + rw) / rw;  // rows per band, rounded up
    const int ya = gy0 + sub * bh;         // this lane's band: rows ya .. yz (none when yz < ya)
    const int yz = ya + bh - 1 <= gy1 ? ya + bh - 1 : gy1;
    const bool self = L == B;
    const bool first = col == 0, last = col == cols - 1;
    for (int xb = gx0; xb <= gx1; xb += cols) {
        const int x = xb + col;
        const bool inx = x <= gx1;
        const int xc = inx ? x : gx1;
        const int hx = first ? x - 1 : x + 1;  // the halo column of the tile's first / last lane
        const bool halo = (first || last) && hx >= gx0 && hx <= gx1;
        bool hprev = false, hcur = false;  // h of the rows y - 1 and y
        int lcur = want;                   // labels[y][x]; rows before the band are never emitted
        // the row in hand is y = ya - 2 + k: two steps fill the window before the band's first row
        for (int k0 = 0; k0 < bh + 2; k0 += NB_ROWS) {
            int ln[NB_ROWS], lh[NB_ROWS];
#pragma unroll
            for (int j = 0; j < NB_ROWS; ++j) {  // the rows below the rows in hand
                const int yn = ya - 1 + k0 + j;
                const size_t row = (size_t)(yn < gy0 ? gy0 : (yn > gy1 ? gy1 : yn)) * W;
                ln[j] = L[row + xc];
                lh[j] = halo ? L[row + hx] : 0;
            }
            bool ring[NB_ROWS];
            int lab[NB_ROWS];
            bool any = false;
#pragma unroll
            for (int j = 0; j < NB_ROWS; ++j) {
                const int y = ya - 2 + k0 + j, yn = y + 1;
                const bool rown = yn >= gy0 && yn <= gy1;
                const bool m = rown && inx && ln[j] == want;
                const bool mh = rown && halo && lh[j] == want;
                const bool left = __shfl_up((int)m, 1) != 0, right = __shfl_down((int)m, 1) != 0;
                const bool hnext = m || (first ? mh : left) || (last ? mh : right);
                ring[j] = y >= ya && y <= yz && inx && lcur != want && (hprev || hcur || hnext);
                lab[j] = lcur;
                any = any || ring[j];
                hprev = hcur;
                hcur = hnext;
                lcur = ln[j];
            }
            if (!__any(any)) continue;
            int v[NB_ROWS];
#pragma unroll
            for (int j = 0; j < NB_ROWS; ++j) {
                const int y = ya - 2 + k0 + j;
                v[j] = self ? lab[j] : B[(size_t)(y < gy0 ? gy0 : (y > gy1 ? gy1 : y)) * W + xc];
            }
#pragma unroll
            for (int j = 0; j < NB_ROWS; ++j)
                if (ring[j]) f(v[j]);
        }
    }
}

__global__ void __launch_bounds__(64) rpx_neighbors_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                           const int* __restrict__ comp, int C,
                                                           double* __restrict__ wtable, int H, int W, int max_label) {
    __shared__ int keys[RL_SLOTS];
    __shared__ unsigned cnts[RL_SLOTS];
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    double* out = wtable + li * (size_t)C * 4;
    const amt_box box = amt_load_box(bbox, li);
    if (box.absent()) {
        amt_fill_row(out, C * 4, 0.0, lane);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* L = labels + (size_t)plane * n;
    const int gy0 = box.y0 > 0 ? box.y0 - 1 : 0, gx0 = box.x0 > 0 ? box.x0 - 1 : 0;
    const int gy1 = box.y1 < H - 1 ? box.y1 + 1 : H - 1, gx1 = box.x1 < W - 1 ? box.x1 + 1 : W - 1;
    const int lc = amt_box_layout(gx0, gx1);
    for (int c = 0; c < C; ++c) {
        const int* B = comp + ((size_t)plane * C + c) * n;
        const rl_census_t r = rl_census(keys, cnts, lane, l + 1, [&](auto&& f) {
            nb_for_ring(L, B, W, gx0, gy0, gx1, gy1, l + 1, lc, lane, f);
        });
        if (lane == 0) {
            out[c * 4 + AMT_RPX_NCOL_COUNT] = (double)r.partners;
            out[c * 4 + AMT_RPX_NCOL_TOUCHING] = (double)r.counted;
            out[c * 4 + AMT_RPX_NCOL_RING] = (double)r.total;
            out[c * 4 + AMT_RPX_NCOL_MAIN] = (double)r.bestv;
        }
    }
}

// ---- the two nearest labels by centroid (AMT_RPX_NEAREST) -----------------------------------------------------------
// The centroid table (rpx_centroid_kernel of amt_props.hip): (cy, cx) of every (plane, label); cy = NaN marks a label that
// is absent from its plane.
// One lane per query label; the labels of the plane pass through LDS in chunks of the workgroup's size (every lane reads
// the same entry: a broadcast).  Candidates arrive in ascending label order, so "strictly nearer" keeps the smallest
// label among equal distances.  max_label^2 distances per plane: a plane of a thousand cells is a million of them.
constexpr int NN_CHUNK = 256;
__global__ void __launch_bounds__(NN_CHUNK) rpx_nearest_kernel(const double2* __restrict__ cen, double* __restrict__ wtable,
                                                               int max_label) {
    __shared__ double2 chunk[NN_CHUNK];
    const int plane = blockIdx.y, tid = threadIdx.x;
    const int l = blockIdx.x * NN_CHUNK + tid;
    const double2* P = cen + (size_t)plane * max_label;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double2 me = l < max_label ? P[l] : make_double2(nan, nan);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double d1 = inf, d2 = inf;  // centroids lie inside the plane: every distance is finite
    int m1 = 0, m2 = 0;
    for (int base = 0; base < max_label; base += NN_CHUNK) {
        __syncthreads();  // the chunk before has been read
        if (base + tid < max_label) chunk[tid] = P[base + tid];
        __syncthreads();
        const int cnt = max_label - base < NN_CHUNK ? max_label - base : NN_CHUNK;
        for (int i = 0; i < cnt; ++i) {
            const double2 o = chunk[i];
            const double dy = o.x - me.x, dx = o.y - me.y;
            const double d = dy * dy + dx * dx;  // NaN when either label is absent: no comparison below holds
            if (base + i == l) continue;
            if (d < d1) {
                d2 = d1, m2 = m1;
                d1 = d, m1 = base + i + 1;
            } else if (d < d2) {
                d2 = d, m2 = base + i + 1;
            }
        }
    }
    if (l < max_label) {
        double* out = wtable + ((size_t)plane * max_label + l) * 4;
        out[AMT_RPX_DCOL_FIRST] = (double)m1;
        out[AMT_RPX_DCOL_FIRST_DISTANCE] = m1 ? sqrt(d1) : nan;
        out[AMT_RPX_DCOL_SECOND] = (double)m2;
        out[AMT_RPX_DCOL_SECOND_DISTANCE] = m2 ? sqrt(d2) : nan;
    }
}

int amt_i_relate_labels(amt_ctx* ctx, const int* labels, const int* bbox, const int* comp, int C, double* wtable,
                        int nplanes, int H, int W, int max_label) {
    hipLaunchKernelGGL(rpx_relate_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox, comp, C,
                       wtable, H, W, max_label);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_i_neighbor_census(amt_ctx* ctx, const int* labels, const int* bbox, const int* comp, int C, double* wtable,
                          int nplanes, int H, int W, int max_label) {
    hipLaunchKernelGGL(rpx_neighbors_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox, comp, C,
                       wtable, H, W, max_label);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_i_nearest_labels(amt_ctx* ctx, const double2* cen, double* wtable, int nplanes, int max_label) {
    hipLaunchKernelGGL(rpx_nearest_kernel, dim3((max_label + NN_CHUNK - 1) / NN_CHUNK, nplanes), dim3(NN_CHUNK), 0,
                       ctx->stream, cen, wtable, max_label);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
