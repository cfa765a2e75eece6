// Region properties as segmented integer reductions keyed by label.
//
// Reference call site: R/masks.py:286-326 (ski.measure.regionprops_table, once for morphology and once
// per channel for intensity).  Property definitions: SK/measure/_regionprops.py:277-468,
// SK/measure/_regionprops_utils.py:186-249 (perimeter), SK/measure/_moments.py:379-445 (inertia tensor),
// SK/morphology/convex_hull.py (area_convex) -- SURVEY.md section 8a row A12, A.7, A.12.
//
// All accumulation is integer (counts, coordinate sums, intensity sums) and therefore independent of
// the order in which pixels arrive; floating point only enters in the final per-label kernel.
// Two passes: rp_boxes_kernel streams the label planes once for the bounding boxes (atomics only from runs that can
// be an extreme of their label); rp_label_kernel, one wave per label over its box, makes everything else privately
// per lane -- moment sums, row extents, intensities, and the perimeter from the row words of the scan -- no atomics.
#include "amt_internal.h"
#include "amt_perlabel.h"

#include <vector>

typedef unsigned long long u64;

// accumulator slots per (plane, label)
enum { A_N = 0, A_SY, A_SX, A_SYY, A_SXX, A_SXY, A_C1, A_C2, A_C3, A_NACC };

// empty boxes (amt_box of amt_perlabel.h) -- or, with `src`, the boxes the watershed's tail left with the context -- and,
// with `acc`, cleared accumulators
__global__ void __launch_bounds__(256) rp_init_kernel(u64* __restrict__ acc, int* __restrict__ bbox, size_t nlab,
                                                      const int* __restrict__ src) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nlab; i += (size_t)gridDim.x * 256) {
        if (acc)
            for (int k = 0; k < A_NACC; ++k) acc[i * A_NACC + k] = 0;
        bbox[i * 4 + 0] = src ? src[i * 4 + 0] : 0x7fffffff;
        bbox[i * 4 + 1] = src ? src[i * 4 + 1] : 0x7fffffff;
        bbox[i * 4 + 2] = src ? src[i * 4 + 2] : -1;
        bbox[i * 4 + 3] = src ? src[i * 4 + 3] : -1;
    }
}

// AMT_DEBUG_POISON=1: the boxes that were handed over against those of the plane pass; *first = the smallest index of an
// int that differs
__global__ void __launch_bounds__(256) rp_boxes_differ_kernel(const int* __restrict__ a, const int* __restrict__ b, size_t n,
                                                              u64* __restrict__ first) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        if (a[i] != b[i]) atomicMin(first, (u64)i);
}

// exact a*b - c*d for 64-bit operands, as a double (the difference itself must fit in 127 bits)
__device__ __forceinline__ double diff_of_products(u64 a, u64 b, u64 c, u64 d) {
    u64 lo1 = a * b, hi1 = __umul64hi(a, b);
    u64 lo2 = c * d, hi2 = __umul64hi(c, d);
    // (hi1:lo1) - (hi2:lo2), signed
    bool neg = (hi1 < hi2) || (hi1 == hi2 && lo1 < lo2);
    u64 hi, lo;
    if (!neg) {
        lo = lo1 - lo2;
        hi = hi1 - hi2 - (lo1 < lo2 ? 1 : 0);
    } else {
        lo = lo2 - lo1;
        hi = hi2 - hi1 - (lo2 < lo1 ? 1 : 0);
    }
    double v = (double)hi * 18446744073709551616.0 + (double)lo;
    return neg ? -v : v;
}

// bounding boxes, a pure streaming read of the label planes: a wave owns a strip of BX_COLS columns (four per lane, one
// 16-byte load per row) and slides down BX_ROWS rows (+ 1 halo row above / below) with a three-row window in registers;
// loads are issued BX_BATCH rows ahead of their use.  Rows that are all background skip everything.  Atomics come only
// from runs that can be an extreme of their label: a run asks for y0 / y1 only if the pixel above / below its head is
// not its label, for x0 only from a head with no pixel of the label above-left or below-left, for x1 from a tail
// likewise -- interior rows of a blob ask for nothing.  The four requests of the lane's four pixels are flat per-lane
// conditions behind ONE uniform test.  What lies left of a strip's first column and right of its last one is not
// loaded and counts as another label: a request too many there, never one too few.
// VEC: the plane pointer is 16-byte aligned and W % 4 == 0 (every row, of every plane, then starts on 16 bytes);
// otherwise four scalar loads per lane (odd widths, sliced planes).
// only_planes (nullable): planes whose flag is 0 are skipped (the watershed's tail, which has the boxes of all but the
// planes it flags: amt_i_label_boxes_flagged).
constexpr int BX_ROWS = 30, BX_COLS = 256, BX_BATCH = 4, BX_NBATCH = (BX_ROWS + 2) / BX_BATCH;
static_assert(BX_BATCH * BX_NBATCH == BX_ROWS + 2, "row batches must tile the strip");

template <bool VEC>
__global__ void __launch_bounds__(256) rp_boxes_kernel(const int* __restrict__ labels, int* __restrict__ bbox, int H,
                                                       int W, int max_label, const int* __restrict__ only_planes) {
    const int lane = threadIdx.x & 63;
    const int strip = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (strip > (W - 1) / BX_COLS) return;  // whole wave; the kernel has no barrier
    const int plane = blockIdx.z;
    if (only_planes && !only_planes[plane]) return;
    const int* L = labels + (size_t)plane * H * W;
    int* bbp = bbox + (size_t)plane * max_label * 4;
    const unsigned x = (unsigned)strip * BX_COLS + 4u * lane;  // the first of the lane's four columns
    const unsigned uw = (unsigned)W, ml = (unsigned)max_label;
    const int ya = blockIdx.y * BX_ROWS, yend = ya + BX_ROWS < H ? ya + BX_ROWS : H;

    // UNCONDITIONAL loads from clamped coordinates; what lies outside the image or outside 1..max_label is zeroed
    // where the value is used
    unsigned xc[4], mlx[4];  // mlx: the largest label of the column, none outside the image
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xc[k] = x + k < uw ? x + k : uw - 1u;
        mlx[k] = x + k < uw ? ml : 0u;
    }
    const unsigned xv = x < uw ? x : uw - 4u;  // VEC: W >= 4
    auto load_row = [&](int y) -> int4 {
        const int yc = y < 0 ? 0 : (y < H ? y : H - 1);
        const int* row = L + (size_t)yc * W;
        if constexpr (VEC) return *(const int4*)(row + xv);
        else return make_int4(row[xc[0]], row[xc[1]], row[xc[2]], row[xc[3]]);
    };
    int4 cur[BX_BATCH], nxt[BX_BATCH];
#pragma unroll
    for (int j = 0; j < BX_BATCH; ++j) cur[j] = load_row(ya - 1 + j);
    // window: c = row r-1 (the row whose runs ask), u = row r-2; index 0 / 5 = the pixel left / right of the lane's four
    int c[6] = {}, u[6] = {};
    for (int b = 0; b < BX_NBATCH; ++b) {
        if (ya - 1 + b * BX_BATCH > yend) break;  // uniform: row yend is the last one a row of this strip looks at
        if (b + 1 < BX_NBATCH) {
#pragma unroll
            for (int j = 0; j < BX_BATCH; ++j) nxt[j] = load_row(ya - 1 + (b + 1) * BX_BATCH + j);
        }
#pragma unroll
        for (int j = 0; j < BX_BATCH; ++j) {
            const int r = ya - 1 + b * BX_BATCH + j;  // row of d
            const bool rin = r >= 0 && r < H;
            const int raw[4] = {cur[j].x, cur[j].y, cur[j].z, cur[j].w};
            int d[6];
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // as unsigned a negative value is above every max_label
                const unsigned top = rin ? mlx[VEC ? 0 : k] : 0u;  // VEC: the lane's four columns lie inside or outside together
                d[k + 1] = (unsigned)raw[k] <= top ? raw[k] : 0;
            }
            d[0] = amt_lane_left(d[4]);
            d[5] = amt_lane_right(d[1]);
            const int yc = r - 1;
            if (yc >= ya && yc < yend && __ballot((c[1] | c[2] | c[3] | c[4]) != 0) != 0ull) {  // uniform
                // a request is a minimum of differences: nonzero if the label is one and differs from every pixel named
                // (vector instructions; as compares the same logic is twice as many scalar ones)
                unsigned q0[4], q1[4], q2[4], q3[4], qk[4], any = 0u;
#pragma unroll
                for (int k = 1; k <= 4; ++k) {
                    const unsigned v = (unsigned)c[k];
                    const unsigned cl = c[k - 1] ^ v, cr = c[k + 1] ^ v, uu = u[k] ^ v, dd = d[k] ^ v;
                    const unsigned ul = u[k - 1] ^ v, dl = d[k - 1] ^ v, ur = u[k + 1] ^ v, dr = d[k + 1] ^ v;
                    q0[k - 1] = min(min(v, cl), uu);               // head of a run, not the label above it
                    q2[k - 1] = min(min(v, cl), dd);               //                              below it
                    q1[k - 1] = min(min(min(cl, ul), dl), v);      // head, not the label above-left or below-left
                    q3[k - 1] = min(min(min(cr, ur), dr), v);      // tail likewise
                    qk[k - 1] = q0[k - 1] | q1[k - 1] | q2[k - 1] | q3[k - 1];
                    any |= qk[k - 1];
                }
                if (__ballot(any != 0u)) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (!qk[k]) continue;  // one skipped block per pixel, not four
                        int* B = bbp + (size_t)(c[k + 1] - 1) * 4;
                        if (q0[k]) atomicMin(&B[0], yc);
                        if (q2[k]) atomicMax(&B[2], yc);
                        if (q1[k]) atomicMin(&B[1], (int)(x + k));
                        if (q3[k]) atomicMax(&B[3], (int)(x + k));
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                u[k] = c[k];
                c[k] = d[k];
            }
        }
#pragma unroll
        for (int j = 0; j < BX_BATCH; ++j) cur[j] = nxt[j];
    }
}

// the plane pass: boxes folded into `bbox` (whose entries are empty boxes or parts of the true ones) by atomics
static int rp_boxes_pass(amt_ctx* ctx, const int* labels, int* bbox, int nplanes, int H, int W, int max_label,
                         const int* only_planes) {
    const int nstrips = (W - 1) / BX_COLS + 1;
    const dim3 grid((nstrips + 3) / 4, (H - 1) / BX_ROWS + 1, nplanes);
    if ((uintptr_t)labels % 16 == 0 && W % 4 == 0)
        hipLaunchKernelGGL(rp_boxes_kernel<true>, grid, dim3(256), 0, ctx->stream, labels, bbox, H, W, max_label, only_planes);
    else
        hipLaunchKernelGGL(rp_boxes_kernel<false>, grid, dim3(256), 0, ctx->stream, labels, bbox, H, W, max_label, only_planes);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

int amt_i_label_boxes_flagged(amt_ctx* ctx, const int* labels, int* bbox, const int* only_planes, int nplanes, int H, int W,
                              int max_label) {
    return rp_boxes_pass(ctx, labels, bbox, nplanes, H, W, max_label, only_planes);
}

// The box pass of every per-label operation: bbox[plane][label] = the label's box, empty for an absent label; `acc`
// (nullable) = the A_NACC accumulators per (plane, label), cleared by the same launch.
// The hand-off ("Label boxes from the watershed's tail"): when the image operation directly before this one on
// the context was the amt_watershed_edt_cleared that wrote exactly these planes, the boxes it left with the context are
// copied by the clearing launch and the label planes are not read.  With AMT_DEBUG_POISON=1 the plane pass runs all the
// same and the call fails unless the two tables agree.
int amt_i_label_boxes(amt_ctx* ctx, const int* labels, int* bbox, unsigned long long* acc, int nplanes, int H, int W,
                      int max_label) {
    const size_t nlab = (size_t)nplanes * max_label;
    const int* handed = amt_box_note_take(ctx, labels, nplanes, H, W, max_label);
    const bool check = handed && amt_poison_enabled();
    hipLaunchKernelGGL(rp_init_kernel, dim3(amt_grid_for(nlab, 256, 1024)), dim3(256), 0, ctx->stream, acc, bbox, nlab,
                       check ? (const int*)nullptr : handed);
    AMT_LAUNCH_CHECK();
    if (handed && !check) return AMT_OK;
    AMT_TRY(rp_boxes_pass(ctx, labels, bbox, nplanes, H, W, max_label, nullptr));
    if (check) {
        if (!ctx->dbg_first) AMT_HIP_CHECK(hipMalloc((void**)&ctx->dbg_first, sizeof(unsigned long long)));
        AMT_HIP_CHECK(hipMemsetAsync(ctx->dbg_first, 0xFF, sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(rp_boxes_differ_kernel, dim3(amt_grid_for(nlab * 4, 256, 1024)), dim3(256), 0, ctx->stream, handed,
                           (const int*)bbox, nlab * 4, ctx->dbg_first);
        AMT_LAUNCH_CHECK();
        unsigned long long first = 0;
        AMT_HIP_CHECK(hipMemcpyAsync(&first, ctx->dbg_first, sizeof(first), hipMemcpyDeviceToHost, ctx->stream));
        AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (first != ~0ull) {
            amt_set_error("label boxes: the boxes handed over by amt_watershed_edt_cleared differ from the plane pass at "
                          "plane %llu, label %llu, field %llu",
                          first / 4 / (unsigned long long)max_label, first / 4 % (unsigned long long)max_label + 1, first % 4);
            return AMT_EHIP;
        }
    }
    return AMT_OK;
}

// One wave per label scans the label's bounding box (and nothing else): exact integer moment sums,
// per-row extents for the convex hull, and {sum, sum of squares, min, max} of up to 4 intensity channels
// per call, all accumulated privately per lane and reduced once -- no atomics, run-to-run identical.
constexpr int RP_MAXC = 4;
constexpr int RPS = 3;  // row slots per step: their label and intensity loads are issued together
// The perimeter's row words: an LDS ring of RP_PW 32-bit words per wave, 4 KB (the kernel's registers allow 24 single-wave
// workgroups per CU, which leaves 6.6 KB each).  A box of nw 32-column words per row keeps RP_PW >> lb rows in it, lb =
// ceil(log2(nw)) (a row's words start at a power of two); it is scanned in bands of rp_band_rows(lb) rows, the four
// rows less are the rows the next band's count still looks at.  Boxes wider than RP_WIDE columns (lb > RP_LBMAX: fewer
// than 8 rows would fit) take rp_perimeter_plain.
constexpr int RP_PW = 1024, RP_LBMAX = 7, RP_WIDE = 32 << RP_LBMAX;
__host__ __device__ constexpr int rp_band_rows(int lb) { return (RP_PW >> lb) - 4; }
__device__ __forceinline__ size_t rp_uniform(size_t v) {  // a wave-uniform value, kept in scalar registers
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((size_t)hi << 32) | lo;
}
struct RpSums {
    u64 cnt, sy, sx, syy, sxx, sxy;
    u64 s[RP_MAXC], q[RP_MAXC];
    unsigned mn[RP_MAXC], mx[RP_MAXC];
};

// The scan of one box.  The wave covers 2^LC columns x (64 >> LC) rows per row slot: 16 x 4 and 32 x 2 for boxes of at
// most 16 / 32 columns (a nucleus: ~28 of 64 lanes of a 64 x 1 slot hold a pixel of the box), 64 x 1 with a loop over
// 64-column blocks otherwise.  A lane owns ONE column of a block, so sx, sxx and sxy follow from the lane's pixel count
// and row sum (x * count, x^2 * count, x * sum of y); per row a lane only counts and adds y.
// ONE round trip per step: the labels and the intensities of the step's RPS row slots are requested together,
// unconditionally, from coordinates clamped into the box; what lies outside the box or the label is discarded where it is
// used (a select next to a load is turned back into a branch around it, and its wait serialises the loads).
// The kernel is bound by instruction issue, not by the round trips ("What the numbers say"): a second register
// set that kept the loads of step s + 1 in flight while step s was consumed cost a fifth of the waves per SIMD and ran
// 20-90 us slower per 48 planes.  What pays is fewer instructions per pixel and per wave.
// The scan takes the rows ya .. y1 of the box that starts at (y0, x0): the whole box, or one band of it (rp_label_kernel).
// `pw` (nullable): every row's words of "label == want" go to the LDS ring of rp_perimeter_rows, the columns 32 k ..
// 32 k + 31 of row y to pw[((y - y0) & (RP_PW - 1 >> lb)) << lb | k].
template <int LC>
__device__ __forceinline__ void rp_label_scan(const int* __restrict__ L, const uint16_t* __restrict__ I, size_t n, int W,
                                              int x0, int y0, int x1, int ya, int y1, int want, int nc, bool rows_ok,
                                              int2* __restrict__ myrows, unsigned* __restrict__ pw, int lb, int lane,
                                              RpSums& a, unsigned& tcnt, u64& tsy) {
    constexpr int COLS = 1 << LC, RW = 64 >> LC;
    const int col = lane & (COLS - 1), sub = lane >> LC;
    // addresses: a wave-uniform base per row slot (scalar registers) and one small byte offset per lane, which the label
    // and every channel share -- not 15 64-bit addresses per step in vector registers
    size_t cofs[RP_MAXC];  // the channels past nc re-read channel 0 (and are not used)
#pragma unroll
    for (int c = 0; c < RP_MAXC; ++c) cofs[c] = rp_uniform((size_t)(c < nc ? c : 0) * n);
    int lv[RPS];
    unsigned iv[RPS][RP_MAXC] = {};
    auto load_step = [&](int yb, int xb) {
        const int xr = x1 - xb;
        const unsigned cx = (unsigned)(col <= xr ? col : xr);
#pragma unroll
        for (int j = 0; j < RPS; ++j) {
            const int yt = yb + j * RW, ys = yt <= y1 ? yt : y1;  // the slot's first row, uniform
            const int y = yt + sub, yc = y <= y1 ? y : y1;
            const unsigned off = (unsigned)(yc - ys) * (unsigned)W + cx;  // < RW * W + 64: see the dispatch
            const size_t base = (size_t)ys * W + xb;
            lv[j] = *(const int*)((const char*)(L + base) + off * 4u);
            if (I) {
#pragma unroll
                for (int c = 0; c < RP_MAXC; ++c)
                    iv[j][c] = *(const uint16_t*)((const char*)(I + cofs[c] + base) + off * 2u);
            }
        }
    };
    int nyb = ya, nxb = x0;
    int rmin[RPS], rmax[RPS];     // LC == 6: a row's extent over the blocks of its row group
    // tcnt, tsy: LC < 6: the lane's column is the same in every step, so the closed forms are taken once at the end
    do {
        const int yb = nyb, xb = nxb;
        load_step(yb, xb);
        nxb = xb + 64;
        if (LC < 6 || nxb > x1) {
            nxb = x0;
            nyb = yb + RPS * RW;
        }
        const int x = xb + col;
        if (LC == 6 && xb == x0) {
#pragma unroll
            for (int j = 0; j < RPS; ++j) {
                rmin[j] = 0x7fffffff;
                rmax[j] = -1;
            }
        }
        // a lane holds one pixel per row slot whatever the layout: RPS pixels per step, bsy <= RPS * (H - 1), no overflow
        unsigned bcnt = 0, bsy = 0;
        int2* steprows = myrows + (yb - y0 + sub);  // LC < 6: this lane's row of slot 0; the slots lie RW rows apart
#pragma unroll
        for (int j = 0; j < RPS; ++j) {
            const int y = yb + j * RW + sub;
            const bool m = x <= x1 && y <= y1 && lv[j] == want;
            if (m) {
                bcnt += 1u;
                bsy += (unsigned)y;
                a.syy += (u64)(unsigned)y * (unsigned)y;
                if (I) {  // all RP_MAXC channels: a uniform branch per channel costs more than the sums of an unused one
#pragma unroll
                    for (int c = 0; c < RP_MAXC; ++c) {
                        const unsigned v = iv[j][c];
                        a.s[c] += v;
                        a.q[c] += (u64)v * v;
                        a.mn[c] = v < a.mn[c] ? v : a.mn[c];
                        a.mx[c] = v > a.mx[c] ? v : a.mx[c];
                    }
                }
            }
            const u64 bal = __ballot(m);
            if constexpr (LC == 6) {
                if (pw && lane == 0 && y <= y1)  // lb >= 1: two words, 8-byte aligned
                    *(u64*)(pw + (((y - y0) & ((RP_PW - 1) >> lb)) << lb) + ((xb - x0) >> 5)) = bal;
                if (bal) {
                    const int first = xb + __ffsll((long long)bal) - 1;
                    const int last = xb + 63 - __clzll((long long)bal);
                    rmin[j] = first < rmin[j] ? first : rmin[j];
                    rmax[j] = last > rmax[j] ? last : rmax[j];
                }
            } else {  // the box is one block wide: row y is bits [sub * COLS, (sub + 1) * COLS) of the ballot
                const unsigned sm = (unsigned)(bal >> (sub * COLS)) & (0xffffffffu >> (32 - COLS));
                if (rows_ok && col == 0 && y <= y1)
                    steprows[j * RW] = sm ? make_int2(x0 + __ffs((int)sm) - 1, x0 + 31 - __clz((int)sm))
                                          : make_int2(0x7fffffff, -1);
                if (pw && col == 0 && y <= y1) pw[(y - y0) & (RP_PW - 1)] = sm;
            }
        }
        if constexpr (LC == 6) {
            a.cnt += bcnt;
            a.sy += bsy;
            a.sx += (u64)(unsigned)x * bcnt;
            a.sxx += (u64)(unsigned)x * (unsigned)x * bcnt;
            a.sxy += (u64)(unsigned)x * bsy;
            if (rows_ok && lane == 0 && nxb == x0) {  // last block of the row group
#pragma unroll
                for (int j = 0; j < RPS; ++j)
                    if (yb + j <= y1) myrows[yb + j - y0] = make_int2(rmin[j], rmax[j]);
            }
        } else {
            tcnt += bcnt;
            tsy += bsy;
        }
    } while (nyb <= y1);
}

// perimeter (SK/measure/_regionprops_utils.py:186-249) of the label whose row words m[y] the scan has left in the ring:
// border pixels B[y] = m[y] & ~(m[y-1] & m[y+1] & west(m[y]) & east(m[y])) (4-neighbourhood, outside = background), and
// for every border pixel the 3 x 3 code 1 + 2 a + 10 d, a / d = its border neighbours across an edge / a corner, as
// bit-sliced sums over all 64 columns of a word at once.  skimage weights the codes {5, 7, 15, 17, 25, 27} (C1: a in
// {2, 3}, d <= 2), {21, 33} (C2: (a, d) = (0, 2), (1, 3)) and {13, 23} (C3: a = 1, d in {1, 2}).
// One lane per (row, word of 32 columns) counts the rows ya .. yb; rows outside y0 .. ylast and words outside 0 .. nw - 1
// are zero.  Of the words left and right only the carry bits matter: column 31 / 0 of m and of B, and columns 30 / 1 of
// m for those.
__device__ __forceinline__ void rp_sum4(unsigned p, unsigned q, unsigned r, unsigned t, unsigned& s0, unsigned& s1,
                                        unsigned& s2) {
    const unsigned x1 = p ^ q, c1 = p & q, x2 = r ^ t, c2 = r & t, k = x1 & x2;
    s0 = x1 ^ x2;
    s1 = c1 ^ c2 ^ k;
    s2 = c1 & c2;
}
template <bool MULTI>  // more than one word per row
__device__ __forceinline__ void rp_perimeter_rows(const unsigned* __restrict__ pw, int lb, int nw, int y0, int ylast,
                                                  int ya, int yb, int lane, unsigned (&cls)[3]) {
    const int rmask = (RP_PW - 1) >> lb;
    for (int i = lane; i < (yb - ya + 1) << lb; i += 64) {
        const int y = ya + (i >> lb), b = MULTI ? i & ((1 << lb) - 1) : 0;
        if (MULTI && b >= nw) continue;
        unsigned m[5];
        unsigned lf[5], rt[5];  // MULTI: the columns 31 (bit 1), 30 (bit 0) of word b - 1 and 0, 1 of word b + 1
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int yy = y - 2 + r;
            const bool ok = yy >= y0 && yy <= ylast;
            const int base = (((yy - y0) & rmask) << lb) + b;  // inside the ring whatever yy is
            const unsigned mc = pw[base];
            m[r] = ok ? mc : 0u;
            lf[r] = rt[r] = 0u;
            if constexpr (MULTI) {
                const unsigned ml = pw[base - (b > 0 ? 1 : 0)], mr = pw[base + (b + 1 < nw ? 1 : 0)];
                lf[r] = (ok && b > 0) ? ml >> 30 : 0u;
                rt[r] = (ok && b + 1 < nw) ? mr & 3u : 0u;
            }
        }
        unsigned B[3], wst[3], est[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const unsigned c = m[r + 1];
            const unsigned cin_w = lf[r + 1] >> 1, cin_e = (rt[r + 1] & 1u) << 31;
            B[r] = c & ~(m[r] & m[r + 2] & ((c << 1) | cin_w) & ((c >> 1) | cin_e));
            // B of column 31 of word b - 1 and of column 0 of word b + 1 (bit 0 of each expression)
            const unsigned bl = (lf[r + 1] >> 1) & ~((lf[r] >> 1) & (lf[r + 2] >> 1) & lf[r + 1] & c) & 1u;
            const unsigned br = rt[r + 1] & ~(rt[r] & rt[r + 2] & (c >> 31) & (rt[r + 1] >> 1)) & 1u;
            wst[r] = (B[r] << 1) | bl;
            est[r] = (B[r] >> 1) | (br << 31);
        }
        unsigned a0, a1, a2, d0, d1, d2;
        rp_sum4(B[0], B[2], wst[1], est[1], a0, a1, a2);
        rp_sum4(wst[0], est[0], wst[2], est[2], d0, d1, d2);
        const unsigned ctr = B[1];
        const unsigned a_is1 = a0 & ~a1 & ~a2, d_is2 = d1 & ~d0 & ~d2;
        cls[0] += (unsigned)__popc(ctr & a1 & ~a2 & ~d2 & ~(d1 & d0));
        cls[1] += (unsigned)__popc(ctr & ((~(a0 | a1 | a2) & d_is2) | (a_is1 & d1 & d0)));
        cls[2] += (unsigned)__popc(ctr & a_is1 & ((d0 & ~d1 & ~d2) | d_is2));
    }
}

// The same counts for a box wider than RP_WIDE columns, pixel by pixel from the label plane: speed does not matter here.
__device__ __forceinline__ void rp_perimeter_plain(const int* __restrict__ L, int H, int W, int x0, int y0, int x1, int y1,
                                                   int want, int lane, unsigned (&cls)[3]) {
    auto on = [&](int y, int x) {
        return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && L[(size_t)y * W + x] == want;
    };
    auto border = [&](int y, int x) {
        return on(y, x) && !(on(y - 1, x) && on(y + 1, x) && on(y, x - 1) && on(y, x + 1));
    };
    for (int y = y0; y <= y1; ++y)
        for (int xb = x0; xb <= x1; xb += 64) {
            const int x = xb + lane;
            if (x > x1 || !border(y, x)) continue;
            const int a = border(y - 1, x) + border(y + 1, x) + border(y, x - 1) + border(y, x + 1);
            const int d = border(y - 1, x - 1) + border(y - 1, x + 1) + border(y + 1, x - 1) + border(y + 1, x + 1);
            cls[0] += (a == 2 || a == 3) && d <= 2;
            cls[1] += (a == 0 && d == 2) || (a == 1 && d == 3);
            cls[2] += a == 1 && (d == 1 || d == 2);
        }
}

// The scan of a box and, with `pw`, its perimeter counts: band by band if the box is taller than the ring.
template <int LC>
__device__ __forceinline__ void rp_label_bands(const int* __restrict__ L, const uint16_t* __restrict__ I, size_t n, int W,
                                               int x0, int y0, int x1, int y1, int want, int nc, bool rows_ok,
                                               int2* __restrict__ myrows, unsigned* __restrict__ pw, int lb, int nw, int lane,
                                               RpSums& a, unsigned (&cls)[3]) {
    const int band = rp_band_rows(lb);
    unsigned tcnt = 0;
    u64 tsy = 0;
    int ya = y0, ycount = y0;
    do {
        const int yb = (pw && y1 - ya >= band) ? ya + band - 1 : y1;
        rp_label_scan<LC>(L, I, n, W, x0, y0, x1, ya, yb, want, nc, rows_ok, myrows, pw, lb, lane, a, tcnt, tsy);
        if (pw) {
            __syncthreads();  // one wave: orders the row words before the lanes that read them
            const int yc = yb == y1 ? y1 : yb - 2;  // row yc + 2 is the last one in the ring
            rp_perimeter_rows<LC == 6>(pw, lb, nw, y0, yb, ycount, yc, lane, cls);
            ycount = yc + 1;
            __syncthreads();
        }
        ya = yb + 1;
    } while (ya <= y1);
    if constexpr (LC < 6) {
        const unsigned x = (unsigned)(x0 + (lane & ((1 << LC) - 1)));
        a.cnt = tcnt;
        a.sy = tsy;
        a.sx = (u64)x * tcnt;
        a.sxx = (u64)x * x * tcnt;
        a.sxy = (u64)x * tsy;
    }
}

// want_morph: bit 0 = the moment sums go to `acc` and the row extents to `rows`, bit 1 = the perimeter's three class
// counts go to acc[A_C1 .. A_C3] too
__global__ void __launch_bounds__(64) rp_label_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                      const int* __restrict__ hoff, const int* __restrict__ htot,
                                                      int2* __restrict__ rows, size_t cap, u64* __restrict__ acc,
                                                      const uint16_t* __restrict__ inten, int C, int c0, int nc,
                                                      double* __restrict__ itable, int H, int W, int max_label,
                                                      int want_morph) {
    const int plane = blockIdx.y;
    const int l = blockIdx.x;
    const int lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    const amt_box box = amt_load_box(bbox, li);
    const int y0 = box.y0, x0 = box.x0, y1 = box.y1, x1 = box.x1;
    if (box.absent()) {
        if (itable) amt_fill_row(itable + (li * C + c0) * 4, 4 * nc, 0.0, lane);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* L = labels + (size_t)plane * n;
    const uint16_t* I = inten ? inten + ((size_t)plane * C + c0) * n : nullptr;
    const bool rows_ok = want_morph && (size_t)htot[plane] <= cap;
    int2* myrows = rows + (size_t)plane * cap + (size_t)hoff[li];
    RpSums a;
    a.cnt = a.sy = a.sx = a.syy = a.sxx = a.sxy = 0;
#pragma unroll
    for (int c = 0; c < RP_MAXC; ++c) {
        a.s[c] = 0;
        a.q[c] = 0;
        a.mn[c] = 0xffffffffu;
        a.mx[c] = 0;
    }
    // wave-uniform; the 2- and 4-row slots keep their per-lane byte offsets (< 4 * (3 * W + 64)) in 32 bits
    const int w = W < (1 << 28) ? x1 - x0 + 1 : 64;
    // the perimeter: the scan leaves the row words in the ring, band by band if the box is taller than the ring
    __shared__ __attribute__((aligned(8))) unsigned s_pw[RP_PW];
    const bool per = (want_morph & 2) != 0;
    // 64 x 1: whole 64-column blocks, so an even number (>= 2) of words per row
    const int nw = w <= 32 ? 1 : (((x1 - x0) >> 6) + 1) * 2, lb = 32 - __clz(nw - 1);
    const bool ring = per && x1 - x0 < RP_WIDE;  // lb <= RP_LBMAX
    unsigned cls[3] = {0u, 0u, 0u};
    unsigned* pw = ring ? s_pw : nullptr;
    if (w <= 16) rp_label_bands<4>(L, I, n, W, x0, y0, x1, y1, l + 1, nc, rows_ok, myrows, pw, 0, 1, lane, a, cls);
    else if (w <= 32) rp_label_bands<5>(L, I, n, W, x0, y0, x1, y1, l + 1, nc, rows_ok, myrows, pw, 0, 1, lane, a, cls);
    else rp_label_bands<6>(L, I, n, W, x0, y0, x1, y1, l + 1, nc, rows_ok, myrows, pw, lb, nw, lane, a, cls);
    if (per && !ring) rp_perimeter_plain(L, H, W, x0, y0, x1, y1, l + 1, lane, cls);
    // ONE reduction of everything: the six moment sums in the order of the accumulator slots, then sum and sum of
    // squares per channel; the extrema as minima (max v = ~min ~v)
    static_assert(A_N == 0 && A_SXY == 5, "the moment sums are the first six accumulator slots");
    u64 t[16];
    t[A_N] = a.cnt, t[A_SY] = a.sy, t[A_SX] = a.sx, t[A_SYY] = a.syy, t[A_SXX] = a.sxx, t[A_SXY] = a.sxy;
    unsigned e[2 * RP_MAXC];
#pragma unroll
    for (int c = 0; c < RP_MAXC; ++c) {
        t[6 + c] = a.s[c];
        t[6 + RP_MAXC + c] = a.q[c];
        e[c] = a.mn[c];
        e[RP_MAXC + c] = ~a.mx[c];
    }
    t[14] = t[15] = 0;
    const u64 red = amt_wave_reduce_scatter<16, amt_op_sum>(t, lane);  // value k in the lanes 4 k .. 4 k + 3
    if (want_morph && (lane & 3) == 0 && lane < 4 * 6) acc[li * A_NACC + (lane >> 2)] = red;
    if (per) {
        static_assert(A_C2 == A_C1 + 1 && A_C3 == A_C1 + 2, "the class counts are three consecutive accumulator slots");
        u64 pc[8] = {cls[0], cls[1], cls[2], 0, 0, 0, 0, 0};
        const u64 pr = amt_wave_reduce_scatter<8, amt_op_sum>(pc, lane);  // value k in the lanes 8 k .. 8 k + 7
        if ((lane & 7) == 0 && lane < 8 * 3) acc[li * A_NACC + A_C1 + (lane >> 3)] = pr;
    }
    if (itable) {
        const unsigned ext = amt_wave_reduce_scatter<8, amt_op_min>(e, lane);  // value k in the lanes 8 k .. 8 k + 7
        // lane c finalises channel c
        const u64 cnt = __shfl(red, 0), S = __shfl(red, 4 * (6 + lane)), Q = __shfl(red, 4 * (6 + RP_MAXC + lane));
        const unsigned lo = __shfl(ext, 8 * lane), hi = ~__shfl(ext, 8 * (RP_MAXC + lane));
        if (lane < nc) {
            double* o = itable + (li * C + c0 + lane) * 4;
            if (cnt == 0) {
                o[0] = o[1] = o[2] = o[3] = 0.0;
            } else {
                const double dn = (double)cnt;
                o[0] = (double)S / dn;
                o[1] = (double)hi;
                o[2] = (double)lo;
                const double nv = diff_of_products(cnt, Q, S, S);  // n*Sxx - Sx^2 = n^2 * var
                const double var = nv / (dn * dn);
                o[3] = sqrt(var < 0.0 ? 0.0 : var);
            }
        }
    }
}

// ---- convex area (exact integer hull of the pixel diamonds) -------------------------------------
// rows[plane][off(label) + (y - miny)] = {min x, max x} of the label in that row
__global__ void __launch_bounds__(256) rp_heights_kernel(const int* __restrict__ bbox, int* __restrict__ hoff,
                                                         int max_label) {
    const int plane = blockIdx.y;
    for (int l = blockIdx.x * 256 + threadIdx.x; l < max_label; l += gridDim.x * 256) {
        const int* B = bbox + ((size_t)plane * max_label + l) * 4;
        hoff[(size_t)plane * max_label + l] = B[2] >= B[0] ? B[2] - B[0] + 1 : 0;
    }
}

// labels of at most HULL_HMAX rows and HULL_WMAX columns go to rp_hull_lds_kernel, the rest to rp_hull_kernel
constexpr int HULL_HMAX = 48, HULL_WMAX = 250;

// area_convex and, with it, solidity = area / area_convex: rp_final_kernel has written the row's area (and a zero
// solidity for an absent label) earlier on the stream, and a label's row is written by exactly one lane of one hull kernel
__device__ __forceinline__ void rp_write_convex(double* __restrict__ trow, double convex) {
    const double area = trow[AMT_RP_AREA];
    trow[AMT_RP_AREA_CONVEX] = convex;
    trow[AMT_RP_SOLIDITY] = area > 0.0 ? area / convex : 0.0;
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {  // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ long long ceil_div(long long a, long long b) {  // b > 0
    long long q = a / b;
    return (a % b != 0 && a > 0) ? q + 1 : q;
}

// One lane per label.  Work in doubled coordinates (Y = 2y, X = 2x): row y with extent [a, b]
// contributes the diamond points (2y-1, 2a), (2y+1, 2a), (2y, 2a-1) on the left and
// (2y-1, 2b), (2y+1, 2b), (2y, 2b+1) on the right (the inner diamond points can never be extreme).
// Left chain = lower-left convex boundary of {(Y, minX(Y))}, right chain of {(Y, maxX(Y))}, built by a
// monotone scan in Y; then pixel centres (2y, 2x) with XL(2y) <= 2x <= XR(2y) are counted exactly.
// CROWS (amt_regionprops_ext): instead of the count, every row's {min x, max x} of the convex image goes to
// crows[plane][off(label) + (y - miny)] (the layout of `rows`); `table` is not touched.
template <bool CROWS>
__global__ void __launch_bounds__(64) rp_hull_kernel(const int* __restrict__ bbox, const int* __restrict__ hoff,
                                                     const int* __restrict__ htot, const int2* __restrict__ rows,
                                                     int2* __restrict__ chainL, int2* __restrict__ chainR, size_t cap,
                                                     double* __restrict__ table, int max_label, int skip_h,
                                                     int2* __restrict__ crows) {
    const int plane = blockIdx.y;
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= max_label) return;
    const size_t li = (size_t)plane * max_label + l;
    double* trow = CROWS ? nullptr : table + li * AMT_RP_NCOLS;
    const int miny = bbox[li * 4 + 0], maxy = bbox[li * 4 + 2];
    if (maxy < miny) {
        if (!CROWS && skip_h == 0) trow[AMT_RP_AREA_CONVEX] = 0.0;
        return;
    }
    const int h = maxy - miny + 1;
    if (h <= skip_h && bbox[li * 4 + 3] - bbox[li * 4 + 1] + 1 <= HULL_WMAX) return;  // done by rp_hull_lds_kernel
    const size_t off = (size_t)hoff[li];
    if ((size_t)htot[plane] > cap || off + (size_t)h > cap) {  // capacity exceeded (fragmented labels)
        if (!CROWS) rp_write_convex(trow, __longlong_as_double(0x7ff8000000000000ll));
        return;
    }
    const int2* r = rows + (size_t)plane * cap + off;
    // chains hold up to 2h+1 vertices each; scratch capacity per plane is 3*cap: offset 3*off, len 3*h
    int2* CL = chainL + (size_t)plane * 3 * cap + 3 * off;
    int2* CR = chainR + (size_t)plane * 3 * cap + 3 * off;
    int nl = 0, nr = 0;
    // iterate Y = 2*miny-1 .. 2*maxy+1
    for (int Y = 2 * miny - 1; Y <= 2 * maxy + 1; ++Y) {
        int mn = 0x7fffffff, mx = -0x7fffffff;
        if (Y & 1) {  // odd: shared by rows (Y-1)/2 and (Y+1)/2
            int ya = (Y - 1) / 2, yb = (Y + 1) / 2;
            if (Y < 0) {  // only for miny == 0: Y = -1 -> rows -1 (none) and 0
                ya = -1;
                yb = 0;
            }
            if (ya >= miny && ya <= maxy) {
                int2 e = r[ya - miny];
                if (e.y >= e.x) {
                    mn = min(mn, 2 * e.x);
                    mx = max(mx, 2 * e.y);
                }
            }
            if (yb >= miny && yb <= maxy) {
                int2 e = r[yb - miny];
                if (e.y >= e.x) {
                    mn = min(mn, 2 * e.x);
                    mx = max(mx, 2 * e.y);
                }
            }
        } else {
            int2 e = r[Y / 2 - miny];
            if (e.y >= e.x) {
                mn = 2 * e.x - 1;
                mx = 2 * e.y + 1;
            }
        }
        if (mx < mn) continue;  // no pixel of this label contributes at this Y
        // left chain: keep it convex towards -X: pop while the last vertex is not strictly left of the
        // segment (prev -> new)
        while (nl >= 2) {
            int2 p0 = CL[nl - 2], p1 = CL[nl - 1];
            long long cr = (long long)(p1.x - p0.x) * (mn - p0.y) - (long long)(p1.y - p0.y) * (Y - p0.x);
            // points are (Y, X) stored as (x=Y, y=X); cr = dY1*dX2 - dX1*dY2 ; left chain needs cr > 0 to keep p1
            if (cr <= 0) --nl; else break;
        }
        CL[nl++] = make_int2(Y, mn);
        while (nr >= 2) {
            int2 p0 = CR[nr - 2], p1 = CR[nr - 1];
            long long cr = (long long)(p1.x - p0.x) * (mx - p0.y) - (long long)(p1.y - p0.y) * (Y - p0.x);
            if (cr >= 0) --nr; else break;
        }
        CR[nr++] = make_int2(Y, mx);
    }
    // count pixel centres
    long long count = 0;
    int il = 0, ir = 0;
    for (int y = miny; y <= maxy; ++y) {
        const int Y = 2 * y;
        while (il + 1 < nl && CL[il + 1].x <= Y) ++il;
        while (ir + 1 < nr && CR[ir + 1].x <= Y) ++ir;
        // left bound XL(Y) on segment il -> il+1 (or vertex if exactly at / past the end)
        long long xmin, xmax;
        {
            int2 p0 = CL[il];
            if (p0.x == Y || il + 1 >= nl) {
                xmin = ceil_div(p0.y, 2);
            } else {
                int2 p1 = CL[il + 1];
                long long dY = p1.x - p0.x;  // > 0
                long long num = (long long)p0.y * dY + (long long)(p1.y - p0.y) * (Y - p0.x);  // XL * dY
                xmin = ceil_div(num, 2 * dY);
            }
        }
        {
            int2 p0 = CR[ir];
            if (p0.x == Y || ir + 1 >= nr) {
                xmax = floor_div(p0.y, 2);
            } else {
                int2 p1 = CR[ir + 1];
                long long dY = p1.x - p0.x;
                long long num = (long long)p0.y * dY + (long long)(p1.y - p0.y) * (Y - p0.x);
                xmax = floor_div(num, 2 * dY);
            }
        }
        if (CROWS) crows[(size_t)plane * cap + off + (y - miny)] = make_int2((int)xmin, (int)xmax);
        else if (xmax >= xmin) count += xmax - xmin + 1;
    }
    if (!CROWS) rp_write_convex(trow, (double)count);
}

// The same hull for labels that fit a small box (at most HULL_HMAX rows and HULL_WMAX columns: every nucleus-sized
// label): two lanes per label, row extents and chains in LDS, interleaved over the wave ([word][lane]), all arithmetic in
// 32 bits.  Coordinates are taken relative to the box (x - x0, Y - Y0), so a row is one 16-bit word (min | max << 8) and
// a chain vertex one 16-bit word ((Y - Y0) << 9 | (X - X0)); every product stays below 2^20.  The HBM-scratch kernel above
// takes the labels that do not fit.
// Round 3: with one lane per label the kernel is a chain of dependent instructions per lane -- ~100 steps in Y with two
// monotone stacks each -- on ~1,000 waves per 48 planes, one per SIMD, nothing to hide a latency behind (222 us; that
// variant was measured and removed).  The left and the right chain are independent: lane 2 i builds the left one, lane
// 2 i + 1 the right one (a pop is "cr <= 0" on the left, "cr >= 0" on the right), each interpolates its own bound per
// row, the pair exchanges bounds by a lane swap; half the LDS per wave, twice the waves.
constexpr int HULL_CH = 2 * HULL_HMAX + 1;
__device__ __forceinline__ int floor_div32(int a, int b) {  // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ int ceil_div32(int a, int b) {  // b > 0
    const int q = a / b;
    return (a % b != 0 && a > 0) ? q + 1 : q;
}
template <bool CROWS>  // as rp_hull_kernel
__global__ void __launch_bounds__(64) rp_hull_lds_kernel(const int* __restrict__ bbox, const int* __restrict__ hoff,
                                                         const int* __restrict__ htot, const int2* __restrict__ rows,
                                                         size_t cap, double* __restrict__ table, int max_label,
                                                         int2* __restrict__ crows) {
    __shared__ unsigned short s_rows[HULL_HMAX * 32];
    __shared__ unsigned short s_ch[HULL_CH * 64];
    const int plane = blockIdx.y;
    const int lane = threadIdx.x, side = lane & 1, pr = lane >> 1;
    const int l = blockIdx.x * 32 + pr;
    if (l >= max_label) return;
    const size_t li = (size_t)plane * max_label + l;
    double* trow = CROWS ? nullptr : table + li * AMT_RP_NCOLS;
    const int miny = bbox[li * 4 + 0], x0 = bbox[li * 4 + 1], maxy = bbox[li * 4 + 2], x1 = bbox[li * 4 + 3];
    if (maxy < miny) {
        if (!CROWS && side == 0) trow[AMT_RP_AREA_CONVEX] = 0.0;
        return;
    }
    const int h = maxy - miny + 1;
    if (h > HULL_HMAX || x1 - x0 + 1 > HULL_WMAX) return;  // rp_hull_kernel takes it
    const size_t off = (size_t)hoff[li];
    if ((size_t)htot[plane] > cap || off + (size_t)h > cap) {  // capacity exceeded (fragmented labels)
        if (!CROWS && side == 0) rp_write_convex(trow, __longlong_as_double(0x7ff8000000000000ll));
        return;
    }
    const int2* r = rows + (size_t)plane * cap + off;
    // the pair shares the loading: lane `side` takes the rows k = side (mod 2), eight per round trip
    for (int k0 = side; k0 < h; k0 += 16) {
        int2 e[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) e[u] = r[min(k0 + 2 * u, h - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + 2 * u < h)  // an empty row (max < min) keeps that property: 255 | 0 << 8
                s_rows[(k0 + 2 * u) * 32 + pr] =
                    e[u].y >= e[u].x ? (unsigned short)((e[u].x - x0) | ((e[u].y - x0) << 8)) : (unsigned short)255;
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // doubled, box-relative coordinates: Yr = Y - (2 miny - 1) in [0, 2h], Xr = X - (2 x0 - 1) in [0, 2w]
    int nc = 0;
    for (int Yr = 0; Yr <= 2 * h; ++Yr) {
        int mn = 0x7fffffff, mx = -1;
        if (!(Yr & 1)) {  // odd Y: shared by the rows above and below
            const int ka = (Yr >> 1) - 1, kb = Yr >> 1;
            if (ka >= 0) {
                const unsigned e = s_rows[ka * 32 + pr];
                if ((e >> 8) >= (e & 255)) {
                    mn = min(mn, 2 * (int)(e & 255) + 1);
                    mx = max(mx, 2 * (int)(e >> 8) + 1);
                }
            }
            if (kb < h) {
                const unsigned e = s_rows[kb * 32 + pr];
                if ((e >> 8) >= (e & 255)) {
                    mn = min(mn, 2 * (int)(e & 255) + 1);
                    mx = max(mx, 2 * (int)(e >> 8) + 1);
                }
            }
        } else {
            const unsigned e = s_rows[(Yr >> 1) * 32 + pr];
            if ((e >> 8) >= (e & 255)) {
                mn = 2 * (int)(e & 255);
                mx = 2 * (int)(e >> 8) + 2;
            }
        }
        if (mx < mn) continue;  // no pixel of this label contributes at this Y
        const int val = side ? mx : mn;
        while (nc >= 2) {
            const int v0 = s_ch[(nc - 2) * 64 + lane], v1 = s_ch[(nc - 1) * 64 + lane];
            const int cr = ((v1 >> 9) - (v0 >> 9)) * (val - (v0 & 511)) - ((v1 & 511) - (v0 & 511)) * (Yr - (v0 >> 9));
            if (side ? cr >= 0 : cr <= 0) --nc; else break;
        }
        s_ch[(nc++) * 64 + lane] = (unsigned short)((Yr << 9) | val);
    }
    // count pixel centres: row k sits at Yr = 2k + 1; pixel x at Xr = 2 (x - x0) + 1
    int count = 0;
    int ic = 0;
    for (int k = 0; k < h; ++k) {
        const int Yr = 2 * k + 1;
        while (ic + 1 < nc && (int)(s_ch[(ic + 1) * 64 + lane] >> 9) <= Yr) ++ic;
        int b;  // this lane's bound of the pixel index: XL <= 2 x + 1 (left, rounded up) or 2 x + 1 <= XR (right, down)
        const int v0 = s_ch[ic * 64 + lane];
        if ((v0 >> 9) == Yr || ic + 1 >= nc) {
            b = side ? floor_div32((v0 & 511) - 1, 2) : ceil_div32((v0 & 511) - 1, 2);
        } else {
            const int v1 = s_ch[(ic + 1) * 64 + lane];
            const int dY = (v1 >> 9) - (v0 >> 9);  // > 0
            const int num = ((v0 & 511) - 1) * dY + ((v1 & 511) - (v0 & 511)) * (Yr - (v0 >> 9));  // (X - 1) * dY
            b = side ? floor_div32(num, 2 * dY) : ceil_div32(num, 2 * dY);
        }
        const int other = __shfl_xor(b, 1);
        const int xmin = side ? other : b, xmax = side ? b : other;
        if (CROWS) {
            if (side == 0) crows[(size_t)plane * cap + off + k] = make_int2(xmin + x0, xmax + x0);
        } else if (xmax >= xmin) {
            count += xmax - xmin + 1;
        }
    }
    if (!CROWS && side == 0) rp_write_convex(trow, (double)count);
}

// ---- final per-label columns ------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rp_final_kernel(const u64* __restrict__ acc, const int* __restrict__ bbox,
                                                       double* __restrict__ table, size_t nlab) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nlab; i += (size_t)gridDim.x * 256) {
        const u64* A = acc + i * A_NACC;
        const int* B = bbox + i * 4;
        double* t = table + i * AMT_RP_NCOLS;
        const u64 n = A[A_N];
        if (n == 0) {
            for (int k = 0; k < AMT_RP_NCOLS; ++k)
                if (k != AMT_RP_AREA_CONVEX) t[k] = 0.0;
            continue;
        }
        const double dn = (double)n;
        t[AMT_RP_AREA] = dn;
        t[AMT_RP_CENTROID_Y] = (double)A[A_SY] / dn;
        t[AMT_RP_CENTROID_X] = (double)A[A_SX] / dn;
        t[AMT_RP_BBOX_Y0] = (double)B[0];
        t[AMT_RP_BBOX_X0] = (double)B[1];
        t[AMT_RP_BBOX_Y1] = (double)(B[2] + 1);
        t[AMT_RP_BBOX_X1] = (double)(B[3] + 1);
        const double SQ2 = 1.4142135623730951;
        t[AMT_RP_PERIMETER] = (double)A[A_C1] + (double)A[A_C2] * SQ2 + (double)A[A_C3] * ((1.0 + SQ2) / 2.0);
        // n * mu20 etc. as exact integers (translation invariant)
        const double Nyy = diff_of_products(n, A[A_SYY], A[A_SY], A[A_SY]);  // n*Syy - Sy^2 = n * mu20
        const double Nxx = diff_of_products(n, A[A_SXX], A[A_SX], A[A_SX]);  // n * mu02
        const double Nxy = diff_of_products(n, A[A_SXY], A[A_SX], A[A_SY]);  // n * mu11
        const double n2 = dn * dn;
        const double a = Nxx / n2;   // T[0,0] = mu02 / mu00
        const double c = Nyy / n2;   // T[1,1] = mu20 / mu00
        const double b = -Nxy / n2;  // T[0,1] = -mu11 / mu00
        const double tr = (a + c) * 0.5;
        const double hd = (a - c) * 0.5;
        const double rad = sqrt(hd * hd + b * b);
        double l1 = tr + rad, l2 = tr - rad;
        l1 = l1 < 0.0 ? 0.0 : l1;
        l2 = l2 < 0.0 ? 0.0 : l2;
        t[AMT_RP_AXIS_MAJOR] = 4.0 * sqrt(l1);
        t[AMT_RP_AXIS_MINOR] = 4.0 * sqrt(l2);
        t[AMT_RP_ECCENTRICITY] = l1 == 0.0 ? 0.0 : sqrt(1.0 - l2 / l1);
        double orient;
        if (Nxx == Nyy) {  // a - c == 0, decided on the exact integer numerators
            orient = (Nxy > 0.0) ? -0.78539816339744828 : 0.78539816339744828;  // b < 0 <=> mu11 > 0
        } else {
            orient = 0.5 * atan2(-2.0 * b, c - a);
        }
        t[AMT_RP_ORIENTATION] = orient;
    }
}

// table_dev != NULL: fill the AMT_RP_* table; itable_dev != NULL: fill {mean, max, min, std} per label and channel
extern "C" int amt_regionprops(amt_ctx* ctx, const int32_t* labels, const uint16_t* intensity, int C, double* table_dev,
                               double* itable_dev, int nplanes, int H, int W, int max_label) {
    AMT_REQUIRE(labels && (table_dev || itable_dev) && nplanes >= 0 && H > 0 && W > 0 && max_label >= 0,
                "regionprops: bad arguments");
    AMT_REQUIRE(!intensity == !itable_dev && (!itable_dev || C >= 1),
                "regionprops: the intensity planes (C >= 1) and the intensity table go together");
    AMT_CHECK_OPERANDS("amt_regionprops", amt_in("labels", labels, amt_span(4, nplanes, H, W)),
                       amt_in("intensity", intensity, amt_span(2, nplanes, C, H, W)),
                       amt_out("table_dev", table_dev, amt_span(8, nplanes, max_label, AMT_RP_NCOLS)),
                       amt_out("itable_dev", itable_dev, amt_span(8, nplanes, max_label, C, 4)));
    AMT_TRY(amt_set_device(ctx));
    const bool want_morph = table_dev != nullptr;
    if (nplanes == 0 || max_label == 0) return AMT_OK;
    const size_t n = (size_t)H * W;
    const size_t nlab = (size_t)nplanes * max_label;
    const size_t cap = want_morph ? n : 1;  // row-extent entries per plane (sum of bbox heights)
    amt_scratch s(ctx);
    amt_buf<u64> acc(s, nlab * A_NACC);
    amt_buf<int> bbox(s, nlab * 4);
    amt_buf<int> hoff(s, nlab);
    amt_buf<int> htot(s, nplanes);
    amt_buf<int2> rows(s, (size_t)nplanes * cap);
    amt_buf<int2> chainL(s, (size_t)nplanes * 3 * cap);
    amt_buf<int2> chainR(s, (size_t)nplanes * 3 * cap);
    AMT_TRY(s.commit());
    AMT_TRY(amt_i_label_boxes(ctx, labels, bbox, acc, nplanes, H, W, max_label));
    hipLaunchKernelGGL(rp_heights_kernel, dim3(amt_grid_for(max_label, 256, 256), nplanes), dim3(256), 0, ctx->stream,
                       bbox, hoff, max_label);
    AMT_LAUNCH_CHECK();
    AMT_TRY(amt_scan_excl(ctx, hoff, max_label, (size_t)max_label, htot, nplanes));
    // per-label scan: moments, row extents and perimeter on the first call, intensity channels in groups of RP_MAXC
    const int groups = intensity ? (C + RP_MAXC - 1) / RP_MAXC : 1;
    for (int g = 0; g < groups; ++g) {
        const int c0 = g * RP_MAXC;
        const int nc = intensity ? ((C - c0) < RP_MAXC ? (C - c0) : RP_MAXC) : 0;
        hipLaunchKernelGGL(rp_label_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox, hoff, htot,
                           rows, cap, acc, intensity, C, c0, nc, intensity ? itable_dev : (double*)nullptr, H, W,
                           max_label, (want_morph && g == 0) ? 3 : 0);
        AMT_LAUNCH_CHECK();
    }
    if (want_morph) {
        hipLaunchKernelGGL(rp_final_kernel, dim3(amt_grid_for(nlab, 256, 1024)), dim3(256), 0, ctx->stream, acc, bbox,
                           table_dev, nlab);
        AMT_LAUNCH_CHECK();
        // the hull kernels read the area that rp_final_kernel has just written: they write area_convex AND solidity
        const int skip_h = HULL_HMAX;
        hipLaunchKernelGGL(rp_hull_lds_kernel<false>, dim3((max_label + 31) / 32, nplanes), dim3(64), 0, ctx->stream, bbox,
                           hoff, htot, rows, cap, table_dev, max_label, (int2*)nullptr);
        AMT_LAUNCH_CHECK();
        // labels taller than HULL_HMAX rows or wider than HULL_WMAX columns: chains in HBM scratch
        hipLaunchKernelGGL(rp_hull_kernel<false>, dim3((max_label + 63) / 64, nplanes), dim3(64), 0, ctx->stream, bbox,
                           hoff, htot, rows, chainL, chainR, cap, table_dev, max_label, skip_h, (int2*)nullptr);
        AMT_LAUNCH_CHECK();
    }
    return AMT_OK;
}

// ---- intensity statistics of float64 images (R/masks.py:319-323 accepts any 2-D ndarray as intensity image) -------
// One wave per label over its bounding box, two sweeps as np.mean / np.std make them: the mean first, then the mean
// of the squared deviations (population std).  float64 sums depend on the order of addition: results
// agree with numpy's pairwise sums to ~1e-15 relative, not bit for bit (the uint16 entry point is exact).
__global__ void __launch_bounds__(64) rp_intensity_f64_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                              const double* __restrict__ inten, int C,
                                                              double* __restrict__ itable, int H, int W, int max_label) {
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    const amt_box box = amt_load_box(bbox, li);
    const int y0 = box.y0, x0 = box.x0, y1 = box.y1, x1 = box.x1;
    double* out = itable + li * (size_t)C * 4;
    if (box.absent()) {
        amt_fill_row(out, C * 4, 0.0, lane);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* lab = labels + (size_t)plane * n;
    for (int c = 0; c < C; ++c) {
        const double* img = inten + ((size_t)plane * C + c) * n;
        double s = 0.0, cnt = 0.0, mn = __longlong_as_double(0x7ff0000000000000ll), mx = -mn;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0 + lane; x <= x1; x += 64)
                if (lab[(size_t)y * W + x] == l + 1) {
                    const double v = img[(size_t)y * W + x];
                    s += v;
                    cnt += 1.0;
                    mn = v < mn ? v : mn;
                    mx = v > mx ? v : mx;
                }
        s = amt_wave_sum(s);
        cnt = amt_wave_sum(cnt);
        mn = amt_wave_min(mn);
        mx = amt_wave_max(mx);
        const double mean = s / cnt;
        double q = 0.0;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0 + lane; x <= x1; x += 64)
                if (lab[(size_t)y * W + x] == l + 1) {
                    const double d = img[(size_t)y * W + x] - mean;
                    q += d * d;
                }
        q = amt_wave_sum(q);
        if (lane == 0) {
            out[c * 4 + 0] = mean;
            out[c * 4 + 1] = mx;
            out[c * 4 + 2] = mn;
            out[c * 4 + 3] = sqrt(q / cnt);
        }
    }
}

extern "C" int amt_regionprops_intensity_f64(amt_ctx* ctx, const int32_t* labels, const double* intensity, int C,
                                             double* table_dev, int nplanes, int H, int W, int max_label) {
    AMT_CHECK_OPERANDS("amt_regionprops_intensity_f64", amt_in("labels", labels, amt_span(4, nplanes, H, W)),
                       amt_in("intensity", intensity, amt_span(8, nplanes, C, H, W)),
                       amt_out("table_dev", table_dev, amt_span(8, nplanes, max_label, C, 4)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(labels && intensity && table_dev && nplanes >= 0 && H > 0 && W > 0 && max_label >= 0 && C >= 1,
                "regionprops_intensity_f64: bad arguments");
    if (nplanes == 0 || max_label == 0) return AMT_OK;
    amt_scratch s(ctx);
    amt_buf<int> bbox(s, (size_t)nplanes * max_label * 4);
    AMT_TRY(s.commit());
    AMT_TRY(amt_i_label_boxes(ctx, labels, bbox, nullptr, nplanes, H, W, max_label));
    hipLaunchKernelGGL(rp_intensity_f64_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox, intensity, C,
                       table_dev, H, W, max_label);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- bounding boxes only (what the outline extractor needs, R/masks.py:99) ---------------------------
extern "C" int amt_label_bboxes(amt_ctx* ctx, const int32_t* labels, int32_t* bbox_dev, int nplanes, int H, int W,
                                int max_label) {
    AMT_CHECK_OPERANDS("amt_label_bboxes", amt_in("labels", labels, amt_span(4, nplanes, H, W)),
                       amt_out("bbox_dev", bbox_dev, amt_span(4, nplanes, max_label, 4)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(labels && bbox_dev && nplanes >= 0 && H > 0 && W > 0 && max_label >= 1, "label_bboxes: bad arguments");
    if (nplanes == 0) return AMT_OK;
    return amt_i_label_boxes(ctx, labels, bbox_dev, nullptr, nplanes, H, W, max_label);
}

// ---- extended region properties (amt_regionprops_ext) ---------------------------------------------------------------
// SK/measure/_regionprops_utils.py:58-184 (euler_number), :252-328 (perimeter_crofton), SK/measure/_regionprops.py
// filled_image (ndi.binary_fill_holes with a 3x3 structure), feret_diameter_max (find_contours of the padded convex
// image), local_centroid / weighted_*centroid, SK/measure/_moments.py inertia_tensor(_eigvals).

// 2x2 configurations: window (y, x) over the zero-padded box holds the pixels (y-1, x-1) (8), (y-1, x) (2), (y, x-1) (4)
// and (y, x) (1) -- the codes ndi.convolve(image, [[0,0,0],[0,1,4],[0,2,8]]) gives.  Windows cover y in [y0, y1 + 1],
// x in [x0, x1 + 1]: the (h+1) x (w+1) grid including the padding (the other windows are code 0).  One wave per
// label; a lane keeps its column's previous row in registers.  Codes 0 and 15 (every window outside and inside the
// label) have coefficient 0 for both properties and are not counted; the rest go to an LDS histogram with integer
// atomics (exact, so run-to-run identical).
__global__ void __launch_bounds__(64) rpx_quad_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                      double* __restrict__ table, int H, int W, int max_label,
                                                      int want_euler, int want_crofton) {
    __shared__ unsigned hist[16];
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    if (lane < 16) hist[lane] = 0;
    __syncthreads();
    const amt_box box = amt_load_box(bbox, li);
    const int y0 = box.y0, x0 = box.x0, y1 = box.y1, x1 = box.x1;
    const int* L = labels + (size_t)plane * H * W;
    const int want = l + 1;
    if (!box.absent()) {
        for (int xb = x0; xb <= x1 + 1; xb += 64) {
            const int x = xb + lane;
            const bool col = x <= x1 + 1;
            // p(y, x) and p(y, x - 1) of the previous row
            unsigned up = 0, upl = 0;
            for (int y = y0; y <= y1 + 1; ++y) {
                unsigned c = 0, cl = 0;
                if (col && y <= y1) {
                    if (x <= x1) c = L[(size_t)y * W + x] == want;
                    if (x - 1 >= x0) cl = L[(size_t)y * W + x - 1] == want;
                }
                const unsigned code = c | (up << 1) | (cl << 2) | (upl << 3);
                if (col && code != 0 && code != 15) atomicAdd(&hist[code], 1u);
                up = c;
                upl = cl;
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        double* t = table + li * AMT_RPX_NCOLS;
        long long h[16];
        for (int k = 0; k < 16; ++k) h[k] = hist[k];
        if (want_euler) t[AMT_RPX_COL_EULER_NUMBER] = (double)(h[8] - h[6] - h[14]);  // EULER_COEFS2D_8
        if (want_crofton) {
            const double pi = 3.141592653589793, s2 = sqrt(2.0);
            const double coefs[16] = {0, pi / 4 * (1 + 1 / s2), pi / (4 * s2), pi / (2 * s2), 0, pi / 4 * (1 + 1 / s2),
                                      0, pi / (4 * s2), pi / 4, pi / 2, pi / (4 * s2), pi / (4 * s2), pi / 4, pi / 2, 0, 0};
            double p = 0.0;
            for (int k = 0; k < 16; ++k) p += coefs[k] * (double)h[k];
            t[AMT_RPX_COL_PERIMETER_CROFTON] = box.absent() ? 0.0 : p;
        }
    }
}

// ---- area_filled ------------------------------------------------------------------------------------------------------
// Background = "not this label" inside the box; what is reachable from the box edge through 8-connected background
// is outside, the rest of the background is holes.  Boxes of at most 64 x 64: one wave per label, lane k holds row k as
// one 64-bit word (bit j = column x0 + j) in a register; rows above / below come from lane shifts.
constexpr int HOLE_SMALL = 64;
__device__ __forceinline__ u64 row_fill(u64 r, u64 b) {  // grow r along the row inside b until it stops
    for (;;) {
        const u64 t = (r | (r << 1) | (r >> 1)) & b;
        if (t == r) return r;
        r = t;
    }
}
__global__ void __launch_bounds__(64) rpx_holes_small_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                             const u64* __restrict__ acc, double* __restrict__ table,
                                                             int H, int W, int max_label) {
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    const amt_box box = amt_load_box(bbox, li);
    const int y0 = box.y0, x0 = box.x0;
    double* t = table + li * AMT_RPX_NCOLS;
    if (box.absent()) {
        if (lane == 0) t[AMT_RPX_COL_AREA_FILLED] = 0.0;
        return;
    }
    const int h = box.h(), w = box.w();
    if (h > HOLE_SMALL || w > HOLE_SMALL) return;  // rpx_holes_large_kernel
    const int* L = labels + (size_t)plane * H * W;
    const u64 wmask = w == 64 ? ~0ull : (1ull << w) - 1ull;
    u64 fg = 0;
    for (int k = 0; k < h; ++k) {  // row k: lane j reads column x0 + j, the ballot is the row's word
        const bool m = lane < w && L[(size_t)(y0 + k) * W + x0 + lane] == l + 1;
        const u64 word = __ballot(m);
        if (lane == k) fg = word;
    }
    const u64 b = lane < h ? ~fg & wmask : 0ull;
    u64 r = (lane == 0 || lane == h - 1) ? b : b & (1ull | (1ull << (w - 1)));
    for (;;) {
        r = row_fill(r, b);
        u64 up = __shfl_up(r, 1), dn = __shfl_down(r, 1);
        up = lane > 0 ? up : 0ull;
        dn = lane < 63 ? dn : 0ull;
        const u64 v = up | dn;
        const u64 rn = r | ((v | (v << 1) | (v >> 1)) & b);
        const u64 changed = __ballot(rn != r);
        r = rn;
        if (!changed) break;
    }
    u64 holes = (u64)__popcll(b & ~r);
    holes = amt_wave_sum(holes);
    if (lane == 0) t[AMT_RPX_COL_AREA_FILLED] = (double)(acc[li * A_NACC + A_N] + holes);
}

// Larger boxes: one workgroup per plane takes its large labels one after the other, with the box's background and
// reached bits in global scratch (rows of wpr 64-bit words); the fill sweeps the words in place until a sweep changes
// nothing.  Bits only ever get set and never leave the background, so words read while a neighbour updates them are
// still a subset of the final set, and a sweep without a change means the fill is complete.
__global__ void __launch_bounds__(256) rpx_holes_large_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                              const u64* __restrict__ acc, double* __restrict__ table,
                                                              u64* __restrict__ scratch, size_t scratch_words, int H,
                                                              int W, int max_label) {
    __shared__ u64 red[4];
    __shared__ int list[256];
    __shared__ int nlist;
    const int plane = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int* L = labels + (size_t)plane * H * W;
    u64* Bw = scratch + (size_t)plane * 2 * scratch_words;
    u64* Rw = Bw + scratch_words;
    for (int base = 0; base < max_label; base += 256) {
        // the large labels of the next 256, found in parallel (their order in the list does not matter)
        if (tid == 0) nlist = 0;
        __syncthreads();
        {
            const int l = base + tid;
            if (l < max_label) {
                const int* B = bbox + ((size_t)plane * max_label + l) * 4;
                if (B[2] >= B[0] && (B[2] - B[0] + 1 > HOLE_SMALL || B[3] - B[1] + 1 > HOLE_SMALL))
                    list[atomicAdd(&nlist, 1)] = l;
            }
        }
        __syncthreads();
        const int nl = nlist;
        for (int il = 0; il < nl; ++il) {
            const int l = list[il];
            const size_t li = (size_t)plane * max_label + l;
            const int y0 = bbox[li * 4 + 0], x0 = bbox[li * 4 + 1], y1 = bbox[li * 4 + 2], x1 = bbox[li * 4 + 3];
            const int h = y1 - y0 + 1, w = x1 - x0 + 1;
            const int wpr = (w + 63) / 64;
            const int nw = h * wpr;
            const int lastbits = w - (wpr - 1) * 64;
            const u64 lastmask = lastbits == 64 ? ~0ull : (1ull << lastbits) - 1ull;
            // background words (one wave per word: lane j reads column 64 q + j) and the seeds on the box edge
            for (int i = wv; i < nw; i += 4) {
                const int k = i / wpr, q = i - k * wpr;
                const int x = x0 + 64 * q + lane;
                const bool m = x <= x1 && L[(size_t)(y0 + k) * W + x] == l + 1;
                const u64 fg = __ballot(m);
                const u64 b = ~fg & (q == wpr - 1 ? lastmask : ~0ull);
                u64 seed = (k == 0 || k == h - 1) ? b : 0ull;
                if (q == 0) seed |= b & 1ull;
                if (q == wpr - 1) seed |= b & (1ull << (lastbits - 1));
                if (lane == 0) {
                    Bw[i] = b;
                    Rw[i] = seed;
                }
            }
            __syncthreads();
            for (;;) {
                int changed = 0;
                for (int i = tid; i < nw; i += 256) {
                    const int k = i / wpr, q = i - k * wpr;
                    const u64 b = Bw[i], r = Rw[i];
                    if (b == r) continue;  // nothing left to reach in this word
                    // the 3 x 3 neighbourhood: words of the rows above / below and the edge bits of the words beside
                    u64 v = 0, side = 0;
                    for (int dk = -1; dk <= 1; ++dk) {
                        const int kk = k + dk;
                        if (kk < 0 || kk >= h) continue;
                        const u64* row = Rw + (size_t)kk * wpr;
                        if (dk != 0) v |= row[q];
                        if (q > 0) side |= row[q - 1] >> 63;
                        if (q + 1 < wpr) side |= (row[q + 1] & 1ull) << 63;
                    }
                    u64 rn = r | ((v | (v << 1) | (v >> 1) | side) & b);
                    rn = row_fill(rn, b);
                    if (rn != r) {
                        Rw[i] = rn;
                        changed = 1;
                    }
                }
                if (!__syncthreads_or(changed)) break;
            }
            u64 holes = 0;
            for (int i = tid; i < nw; i += 256) holes += (u64)__popcll(Bw[i] & ~Rw[i]);
            holes = amt_wave_sum(holes);
            if (lane == 0) red[wv] = holes;
            __syncthreads();
            if (tid == 0)
                table[li * AMT_RPX_NCOLS + AMT_RPX_COL_AREA_FILLED] =
                    (double)(acc[li * A_NACC + A_N] + red[0] + red[1] + red[2] + red[3]);
            __syncthreads();
        }
        __syncthreads();  // every thread has read nlist and the list before they are rewritten
    }
}

// ---- feret_diameter_max ---------------------------------------------------------------------------------------------
// The contour of the convex image at level 0.5 passes through the midpoint of every edge between a pixel of the image
// and one outside it; the farthest pair of those midpoints is the diameter.  In doubled coordinates the midpoints of
// row y with convex extent [a, b] are (2y, 2a - 1) and (2y, 2b + 1), and the columns of the row that have no pixel
// above (below) give midpoints on the line 2y - 1 (2y + 1).  Those lie on at most two segments per side, and the
// farthest point of a segment from any point is one of its ends: up to 10 candidates per row, all exact integers.
struct FeretRow {
    int Y[10], X[10];
};
__device__ __forceinline__ int2 crow_at(const int2* cr, int k, int h) {
    return (k < 0 || k >= h) ? make_int2(1, 0) : cr[k];  // outside the box: empty
}
__device__ __forceinline__ void feret_row(const int2* cr, int k, int h, int y0, int2 fallback, FeretRow& p) {
    const int2 e = crow_at(cr, k, h);
    const int Y = 2 * (y0 + k);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        p.Y[i] = fallback.x;
        p.X[i] = fallback.y;
    }
    if (e.y < e.x) return;
    p.Y[0] = Y, p.X[0] = 2 * e.x - 1;
    p.Y[1] = Y, p.X[1] = 2 * e.y + 1;
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // s = 0: the neighbour above (edge line Y - 1), s = 1: below (Y + 1)
        const int2 o = crow_at(cr, s ? k + 1 : k - 1, h);
        const int Ye = s ? Y + 1 : Y - 1;
        int a0 = e.x, b0 = e.y, a1 = 1, b1 = 0;  // [a, b] minus [o.x, o.y]: up to two intervals
        if (o.y >= o.x && o.x <= e.y && o.y >= e.x) {
            a0 = e.x, b0 = min(e.y, o.x - 1);
            a1 = max(e.x, o.y + 1), b1 = e.y;
        }
        const int base = 2 + 4 * s;
        if (b0 >= a0) {
            p.Y[base] = Ye, p.X[base] = 2 * a0;
            p.Y[base + 1] = Ye, p.X[base + 1] = 2 * b0;
        } else {
            p.Y[base] = p.Y[0], p.X[base] = p.X[0];
            p.Y[base + 1] = p.Y[0], p.X[base + 1] = p.X[0];
        }
        if (b1 >= a1) {
            p.Y[base + 2] = Ye, p.X[base + 2] = 2 * a1;
            p.Y[base + 3] = Ye, p.X[base + 3] = 2 * b1;
        } else {
            p.Y[base + 2] = p.Y[0], p.X[base + 2] = p.X[0];
            p.Y[base + 3] = p.Y[0], p.X[base + 3] = p.X[0];
        }
    }
}
__global__ void __launch_bounds__(64) rpx_feret_kernel(const int* __restrict__ bbox, const int* __restrict__ hoff,
                                                       const int* __restrict__ htot, const int2* __restrict__ crows,
                                                       size_t cap, double* __restrict__ table, int max_label) {
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    double* t = table + li * AMT_RPX_NCOLS;
    const int y0 = bbox[li * 4 + 0], y1 = bbox[li * 4 + 2];
    if (y1 < y0) {
        if (lane == 0) t[AMT_RPX_COL_FERET_DIAMETER_MAX] = 0.0;
        return;
    }
    const int h = y1 - y0 + 1;
    const size_t off = (size_t)hoff[li];
    if ((size_t)htot[plane] > cap || off + (size_t)h > cap) {  // the hull kernels skipped it too
        if (lane == 0) t[AMT_RPX_COL_FERET_DIAMETER_MAX] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const int2* cr = crows + (size_t)plane * cap + off;
    const int2 e0 = cr[0];  // the top row holds a pixel of the label, so its convex extent is not empty
    const int2 fallback = make_int2(2 * y0, 2 * e0.x - 1);
    // the lanes share the row pairs (ka <= kb) of the box evenly, not one row each
    long long best = 0;
    for (int p = lane; p < h * h; p += 64) {
        const int ka = p / h, kb = p - ka * h;
        if (kb < ka) continue;
        FeretRow a, b;
        feret_row(cr, ka, h, y0, fallback, a);
        feret_row(cr, kb, h, y0, fallback, b);
#pragma unroll
        for (int i = 0; i < 10; ++i)
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const long long dy = a.Y[i] - b.Y[j], dx = a.X[i] - b.X[j];
                const long long d = dy * dy + dx * dx;
                best = d > best ? d : best;
            }
    }
    best = amt_wave_max(best);
    if (lane == 0) t[AMT_RPX_COL_FERET_DIAMETER_MAX] = sqrt((double)best) * 0.5;  // = sqrt(best / 4), exactly
}

// ---- centroid_local, inertia_tensor, inertia_tensor_eigvals from the exact moment sums of rp_label_kernel -------------
__global__ void __launch_bounds__(256) rpx_moments_kernel(const u64* __restrict__ acc, const int* __restrict__ bbox,
                                                          double* __restrict__ table, size_t nlab, int columns) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nlab; i += (size_t)gridDim.x * 256) {
        const u64* A = acc + i * A_NACC;
        double* t = table + i * AMT_RPX_NCOLS;
        const u64 n = A[A_N];
        double cy = 0, cx = 0, a = 0, b = 0, c = 0, l1 = 0, l2 = 0;
        if (n != 0) {
            const double dn = (double)n;
            // sum of (y - y0): exact integers, so M10 / M00 rounds once, as the float64 moments of the box do
            cy = (double)(A[A_SY] - n * (u64)bbox[i * 4 + 0]) / dn;
            cx = (double)(A[A_SX] - n * (u64)bbox[i * 4 + 1]) / dn;
            const double Nyy = diff_of_products(n, A[A_SYY], A[A_SY], A[A_SY]);  // n * mu20
            const double Nxx = diff_of_products(n, A[A_SXX], A[A_SX], A[A_SX]);  // n * mu02
            const double Nxy = diff_of_products(n, A[A_SXY], A[A_SX], A[A_SY]);  // n * mu11
            const double n2 = dn * dn;
            a = Nxx / n2;   // T[0,0] = mu02 / mu00
            c = Nyy / n2;   // T[1,1] = mu20 / mu00
            b = -Nxy / n2;  // T[0,1] = T[1,0] = -mu11 / mu00
            const double tr = (a + c) * 0.5, hd = (a - c) * 0.5;
            const double rad = sqrt(hd * hd + b * b);
            l1 = tr + rad;
            l2 = tr - rad;
            l1 = l1 < 0.0 ? 0.0 : l1;
            l2 = l2 < 0.0 ? 0.0 : l2;
        }
        if (columns & AMT_RPX_CENTROID_LOCAL) {
            t[AMT_RPX_COL_CENTROID_LOCAL_Y] = cy;
            t[AMT_RPX_COL_CENTROID_LOCAL_X] = cx;
        }
        if (columns & AMT_RPX_INERTIA_TENSOR) {
            t[AMT_RPX_COL_INERTIA_00] = a;
            t[AMT_RPX_COL_INERTIA_01] = b;
            t[AMT_RPX_COL_INERTIA_10] = b;
            t[AMT_RPX_COL_INERTIA_11] = c;
        }
        if (columns & AMT_RPX_INERTIA_EIGVALS) {
            t[AMT_RPX_COL_EIGVAL_0] = l1;
            t[AMT_RPX_COL_EIGVAL_1] = l2;
        }
    }
}

// ---- centroid_weighted(_local) --------------------------------------------------------------------------------------
// One wave per label over its box: sum I, sum I (y - y0), sum I (x - x0) per channel.  uint16 images sum in 64-bit
// integers (exact: the float64 moments of the box are exact integers too); float64 images sum in float64.
template <typename T, typename S>
__global__ void __launch_bounds__(64) rpx_weighted_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                          const T* __restrict__ inten, int C, double* __restrict__ wtable,
                                                          int H, int W, int max_label) {
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    double* out = wtable + li * (size_t)C * 4;
    const amt_box box = amt_load_box(bbox, li);
    const int y0 = box.y0, x0 = box.x0, y1 = box.y1, x1 = box.x1;
    if (box.absent()) {
        amt_fill_row(out, C * 4, 0.0, lane);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* lab = labels + (size_t)plane * n;
    for (int c = 0; c < C; ++c) {
        const T* img = inten + ((size_t)plane * C + c) * n;
        S s = 0, sy = 0, sx = 0;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0 + lane; x <= x1; x += 64)
                if (lab[(size_t)y * W + x] == l + 1) {
                    const S v = (S)img[(size_t)y * W + x];
                    s += v;
                    sy += v * (S)(y - y0);
                    sx += v * (S)(x - x0);
                }
        s = amt_wave_sum(s), sy = amt_wave_sum(sy), sx = amt_wave_sum(sx);
        if (lane == 0) {
            const double ly = (double)sy / (double)s, lx = (double)sx / (double)s;  // 0 / 0 = NaN, as scikit-image
            out[c * 4 + 0] = ly + (double)y0;
            out[c * 4 + 1] = lx + (double)x0;
            out[c * 4 + 2] = ly;
            out[c * 4 + 3] = lx;
        }
    }
}

// ---- the centroid table of AMT_RPX_NEAREST (amt_relate.hip searches it) ------------------------------------------------
// (cy, cx) of every (plane, label) from the integer sums of rp_label_kernel; cy = NaN marks a label that
// is absent from its plane
__global__ void __launch_bounds__(256) rpx_centroid_kernel(const u64* __restrict__ acc, double2* __restrict__ cen,
                                                           size_t nlab) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nlab; i += (size_t)gridDim.x * 256) {
        const u64* A = acc + i * A_NACC;
        const u64 n = A[A_N];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        cen[i] = n != 0 ? make_double2((double)A[A_SY] / (double)n, (double)A[A_SX] / (double)n) : make_double2(nan, nan);
    }
}

extern "C" int amt_regionprops_ext(amt_ctx* ctx, const int32_t* labels, const void* intensity, int in_code, int C,
                                   int columns, double* table_dev, double* wtable_dev, int nplanes, int H, int W,
                                   int max_label) {
    const unsigned cols = (unsigned)columns;
    if (cols & AMT_RPX_RADIAL) {
        // radial distribution: the bins ride in the field of the texture levels, table_dev takes the geometry rows
        const unsigned bins = 0x7fu << AMT_RPX_TEXTURE_LEVELS_SHIFT;
        AMT_REQUIRE((cols & ~(AMT_RPX_RADIAL | bins)) == 0, "regionprops_ext: no other column bit goes with AMT_RPX_RADIAL");
        return amt_i_radial(ctx, labels, intensity, in_code, C, (int)(cols >> AMT_RPX_TEXTURE_LEVELS_SHIFT & 0x7fu), table_dev,
                            wtable_dev, nplanes, H, W, max_label);
    }
    if (cols & (AMT_RPX_TEXTURE | AMT_RPX_TEXTURE_COUNTS)) {
        // Haralick texture: levels and distance ride in the upper bits, table_dev holds the ranges
        const unsigned params = 0x7fu << AMT_RPX_TEXTURE_LEVELS_SHIFT | 0x3ffu << AMT_RPX_TEXTURE_DISTANCE_SHIFT;
        const bool counts = (cols & AMT_RPX_TEXTURE_COUNTS) != 0;
        AMT_REQUIRE((cols & ~(AMT_RPX_TEXTURE | AMT_RPX_TEXTURE_COUNTS | params)) == 0 && counts != ((cols & AMT_RPX_TEXTURE) != 0),
                    "regionprops_ext: one of AMT_RPX_TEXTURE and AMT_RPX_TEXTURE_COUNTS, and no other column bit with it");
        return amt_i_texture(ctx, labels, intensity, in_code, C, table_dev, (int)(cols >> AMT_RPX_TEXTURE_LEVELS_SHIFT & 0x7fu),
                             (int)(cols >> AMT_RPX_TEXTURE_DISTANCE_SHIFT & 0x3ffu), counts, wtable_dev, nplanes, H, W,
                             max_label);
    }
    const bool want_w = (cols & AMT_RPX_CENTROID_WEIGHTED) != 0;
    const bool want_r = (cols & AMT_RPX_RELATE) != 0;
    const bool want_q = (cols & AMT_RPX_ROBUST) != 0;
    const bool want_n = (cols & AMT_RPX_NEIGHBORS) != 0;
    const bool want_d = (cols & AMT_RPX_NEAREST) != 0;
    const bool want_c = want_w || want_r || want_q || want_n;  // the call has companion planes
    const bool want_t = want_c || want_d;                      // ... and the table of four columns per companion
    const unsigned table_bits =
        AMT_RPX_CENTROID_WEIGHTED | AMT_RPX_RELATE | AMT_RPX_ROBUST | AMT_RPX_NEIGHBORS | AMT_RPX_NEAREST;
    const bool want_m = (cols & ~table_bits) != 0;
    AMT_REQUIRE(labels && nplanes >= 0 && H > 0 && W > 0 && max_label >= 0 && cols != 0 &&
                    (cols & ~(AMT_RPX_ALL | AMT_RPX_RELATE | AMT_RPX_ROBUST | AMT_RPX_NEIGHBORS | AMT_RPX_NEAREST)) == 0,
                "regionprops_ext: bad arguments");
    AMT_REQUIRE((int)want_w + (int)want_r + (int)want_q + (int)want_n + (int)want_d <= 1,
                "regionprops_ext: AMT_RPX_CENTROID_WEIGHTED, AMT_RPX_RELATE, AMT_RPX_ROBUST, AMT_RPX_NEIGHBORS and "
                "AMT_RPX_NEAREST share the table of four columns per companion: one call, one of them");
    AMT_REQUIRE(!table_dev == !want_m, "regionprops_ext: the morphology table and its column bits go together");
    AMT_REQUIRE(want_c == !!intensity && want_t == !!wtable_dev && (!want_c || C >= 1),
                "regionprops_ext: the intensity planes (C >= 1), the weighted table and AMT_RPX_CENTROID_WEIGHTED or "
                "AMT_RPX_ROBUST (or the companion label planes, the relation table and AMT_RPX_RELATE or "
                "AMT_RPX_NEIGHBORS) go together; AMT_RPX_NEAREST takes the table alone");
    AMT_REQUIRE(!want_d || (in_code == 0 && C == 1), "regionprops_ext: AMT_RPX_NEAREST takes in_code 0 and C == 1");
    AMT_REQUIRE(!(want_w || want_q) || in_code == AMT_U16 || in_code == AMT_F64,
                "regionprops_ext: intensity must be AMT_U16 or AMT_F64");
    AMT_REQUIRE((want_r || want_n) == (in_code == AMT_I32),
                "regionprops_ext: AMT_I32 companion label planes and AMT_RPX_RELATE or AMT_RPX_NEIGHBORS go together");
    // labels and intensity are both inputs: a companion may be the very buffer `labels` points to
    AMT_CHECK_OPERANDS("amt_regionprops_ext", amt_in("labels", labels, amt_span(4, nplanes, H, W)),
                       amt_in("intensity", intensity, amt_span(amt_esize(in_code), nplanes, C, H, W)),
                       amt_out("table_dev", table_dev, amt_span(8, nplanes, max_label, AMT_RPX_NCOLS)),
                       amt_out("wtable_dev", wtable_dev, amt_span(8, nplanes, max_label, C, 4)));
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0 || max_label == 0) return AMT_OK;
    const bool euler = cols & (AMT_RPX_EULER_NUMBER | AMT_RPX_PERIMETER_CROFTON);
    const bool filled = cols & AMT_RPX_AREA_FILLED, feret = cols & AMT_RPX_FERET_DIAMETER_MAX;
    const bool moments = cols & (AMT_RPX_CENTROID_LOCAL | AMT_RPX_INERTIA_TENSOR | AMT_RPX_INERTIA_EIGVALS);
    const bool scan = filled || feret || moments || want_d;  // rp_label_kernel: pixel counts, moment sums, row extents
    const size_t n = (size_t)H * W;
    const size_t nlab = (size_t)nplanes * max_label;
    const size_t cap = feret ? n : 1;
    const size_t hwords = filled ? (size_t)H * ((W + 63) / 64) : 0;
    amt_scratch s(ctx);
    amt_buf<u64> acc(s, nlab * A_NACC);
    amt_buf<int> bbox(s, nlab * 4);
    amt_buf<int> hoff(s, nlab);
    amt_buf<int> htot(s, nplanes);
    amt_buf<int2> rows(s, (size_t)nplanes * cap);
    amt_buf<int2> crows(s, (size_t)nplanes * cap);
    amt_buf<int2> chainL(s, (size_t)nplanes * 3 * cap);
    amt_buf<int2> chainR(s, (size_t)nplanes * 3 * cap);
    amt_buf<u64> hscratch(s, (size_t)nplanes * 2 * hwords);
    amt_buf<double2> cen(s, nlab, want_d);
    AMT_TRY(s.commit());
    AMT_TRY(amt_i_label_boxes(ctx, labels, bbox, acc, nplanes, H, W, max_label));
    if (scan) {
        hipLaunchKernelGGL(rp_heights_kernel, dim3(amt_grid_for(max_label, 256, 256), nplanes), dim3(256), 0, ctx->stream,
                           bbox, hoff, max_label);
        AMT_LAUNCH_CHECK();
        AMT_TRY(amt_scan_excl(ctx, hoff, max_label, (size_t)max_label, htot, nplanes));
        hipLaunchKernelGGL(rp_label_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox, hoff, htot,
                           rows, cap, acc, (const uint16_t*)nullptr, 1, 0, 0, (double*)nullptr, H, W, max_label, 1);
        AMT_LAUNCH_CHECK();
    }
    if (euler) {
        hipLaunchKernelGGL(rpx_quad_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox, table_dev, H,
                           W, max_label, (cols & AMT_RPX_EULER_NUMBER) ? 1 : 0, (cols & AMT_RPX_PERIMETER_CROFTON) ? 1 : 0);
        AMT_LAUNCH_CHECK();
    }
    if (filled) {
        hipLaunchKernelGGL(rpx_holes_small_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox, acc,
                           table_dev, H, W, max_label);
        AMT_LAUNCH_CHECK();
        hipLaunchKernelGGL(rpx_holes_large_kernel, dim3(nplanes), dim3(256), 0, ctx->stream, labels, bbox, acc, table_dev,
                           hscratch, hwords, H, W, max_label);
        AMT_LAUNCH_CHECK();
    }
    if (feret) {
        hipLaunchKernelGGL(rp_hull_lds_kernel<true>, dim3((max_label + 31) / 32, nplanes), dim3(64), 0, ctx->stream, bbox,
                           hoff, htot, rows, cap, (double*)nullptr, max_label, crows);
        AMT_LAUNCH_CHECK();
        hipLaunchKernelGGL(rp_hull_kernel<true>, dim3((max_label + 63) / 64, nplanes), dim3(64), 0, ctx->stream, bbox, hoff,
                           htot, rows, chainL, chainR, cap, (double*)nullptr, max_label, HULL_HMAX, crows);
        AMT_LAUNCH_CHECK();
        hipLaunchKernelGGL(rpx_feret_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, bbox, hoff, htot, crows,
                           cap, table_dev, max_label);
        AMT_LAUNCH_CHECK();
    }
    if (moments) {
        hipLaunchKernelGGL(rpx_moments_kernel, dim3(amt_grid_for(nlab, 256, 1024)), dim3(256), 0, ctx->stream, acc, bbox,
                           table_dev, nlab, columns);
        AMT_LAUNCH_CHECK();
    }
    if (want_w) {
        if (in_code == AMT_U16)
            hipLaunchKernelGGL((rpx_weighted_kernel<uint16_t, u64>), dim3(max_label, nplanes), dim3(64), 0, ctx->stream,
                               labels, bbox, (const uint16_t*)intensity, C, wtable_dev, H, W, max_label);
        else
            hipLaunchKernelGGL((rpx_weighted_kernel<double, double>), dim3(max_label, nplanes), dim3(64), 0, ctx->stream,
                               labels, bbox, (const double*)intensity, C, wtable_dev, H, W, max_label);
        AMT_LAUNCH_CHECK();
    }
    if (want_r)
        AMT_TRY(amt_i_relate_labels(ctx, labels, bbox, (const int*)intensity, C, wtable_dev, nplanes, H, W, max_label));
    if (want_n)
        AMT_TRY(amt_i_neighbor_census(ctx, labels, bbox, (const int*)intensity, C, wtable_dev, nplanes, H, W, max_label));
    if (want_d) {
        hipLaunchKernelGGL(rpx_centroid_kernel, dim3(amt_grid_for(nlab, 256, 1024)), dim3(256), 0, ctx->stream, acc, cen,
                           nlab);
        AMT_LAUNCH_CHECK();
        AMT_TRY(amt_i_nearest_labels(ctx, cen, wtable_dev, nplanes, max_label));
    }
    if (want_q) AMT_TRY(amt_i_robust_intensity(ctx, labels, bbox, intensity, in_code, C, wtable_dev, nplanes, H, W, max_label));
    return AMT_OK;
}

// ---- per-label channel colocalisation (amt_colocalization) ----------------------------------------------------------
// Pearson, Manders' overlap / M1 / M2 and the intersection coefficients of channel pairs inside every label (the
// definitions stand in include/amt_hip.h).  Same traffic as the intensity pass of rp_label_kernel: the label's bounding
// box in the label plane and in the channels of the launch.

// One launch measures up to COLOC_MAXC channels and every pair of them: slot pair k = (a, b), a < b, in the order
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  out[k] = index of the requested pair that slot pair answers, -1 for none;
// swap[k]: the request names the channels the other way round (m1 / m2 and intersection1 / 2 change places).
constexpr int COLOC_MAXC = 4, COLOC_MAXP = 6;
struct coloc_launch {
    int chan[COLOC_MAXC];
    int nch;
    int out[COLOC_MAXP];
    int swap[COLOC_MAXP];
};
__host__ __device__ __forceinline__ int coloc_slot_a(int k) { return k < 3 ? 0 : (k < 5 ? 1 : 2); }
__host__ __device__ __forceinline__ int coloc_slot_b(int k) { return k < 3 ? k + 1 : (k < 5 ? k - 1 : 3); }

// layout of the 32 reduced words: per channel slot sum v, sum v^2; per slot pair sum a b, sum a[b > tB], sum b[a > tA];
// then the counts, two to a word (each stays below 2^32): n, positives per slot, both-positive per pair
enum { CO_S = 0, CO_Q = 4, CO_AB = 8, CO_AIF = 14, CO_BIF = 20, CO_CNT = 26 };
__device__ __forceinline__ u64 coloc_count(const u64* red, int i) {
    return (red[CO_CNT + (i >> 1)] >> (32 * (i & 1))) & 0xffffffffull;
}

__device__ __forceinline__ void coloc_write_empty(double* t) {
    const double nan = amt_quiet_nan();
    t[0] = nan;
    t[1] = nan;
    t[2] = t[3] = t[4] = t[5] = 0.0;
}

// uint16 images: one wave per (label, plane) over the label's bounding box, rows in steps of RPS with the label and the
// intensity loads of a step issued together from clamped coordinates, lanes own columns (rp_label_kernel's scan).  All
// sums are exact integers, private per lane, reduced once; lanes 0..5 finalise one slot pair each in float64.
// "v > t" for an integer v and a float64 t is "v > floor(t)", so the comparison runs on integers.
__global__ void __launch_bounds__(64) coloc_u16_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                       const uint16_t* __restrict__ inten, int C,
                                                       const double* __restrict__ thr, const coloc_launch P,
                                                       double* __restrict__ table, int npairs, int H, int W,
                                                       int max_label) {
    __shared__ u64 red[32];
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    const amt_box box = amt_load_box(bbox, li);
    const int y0 = box.y0, x0 = box.x0, y1 = box.y1, x1 = box.x1;
    double* rows = table + li * (size_t)npairs * AMT_COLOC_NCOLS;
    if (box.absent()) {
        if (lane < COLOC_MAXP && P.out[lane] >= 0) coloc_write_empty(rows + (size_t)P.out[lane] * AMT_COLOC_NCOLS);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* L = labels + (size_t)plane * n;
    const uint16_t* I = inten + (size_t)plane * C * n;
    const int want = l + 1;
    size_t coff[COLOC_MAXC];
    int ti[COLOC_MAXC];  // v is positive when v > ti: -1 = every value, 65535 = none (a NaN threshold too)
#pragma unroll
    for (int c = 0; c < COLOC_MAXC; ++c) {
        const int ch = P.chan[c < P.nch ? c : 0];
        coff[c] = (size_t)ch * n;
        const double t = thr[(size_t)plane * C + ch];
        ti[c] = !(t < 65535.0) ? 65535 : (t < 0.0 ? -1 : (int)floor(t));
    }
    u64 s[COLOC_MAXC], q[COLOC_MAXC], ab[COLOC_MAXP], aif[COLOC_MAXP], bif[COLOC_MAXP];
    unsigned cnt = 0, np[COLOC_MAXC], both[COLOC_MAXP];
#pragma unroll
    for (int c = 0; c < COLOC_MAXC; ++c) s[c] = q[c] = 0, np[c] = 0;
#pragma unroll
    for (int k = 0; k < COLOC_MAXP; ++k) ab[k] = aif[k] = bif[k] = 0, both[k] = 0;
    constexpr int RPS = 3;
    for (int yb = y0; yb <= y1; yb += RPS) {
        for (int xb = x0; xb <= x1; xb += 64) {
            const int x = xb + lane;
            const int xc = x <= x1 ? x : x1;
            int lv[RPS];
            unsigned iv[RPS][COLOC_MAXC];
#pragma unroll
            for (int j = 0; j < RPS; ++j) {
                const int yc = yb + j <= y1 ? yb + j : y1;
                lv[j] = L[(size_t)yc * W + xc];
            }
#pragma unroll
            for (int j = 0; j < RPS; ++j) {
                const int yc = yb + j <= y1 ? yb + j : y1;
#pragma unroll
                for (int c = 0; c < COLOC_MAXC; ++c) iv[j][c] = I[coff[c] + (size_t)yc * W + xc];
            }
#pragma unroll
            for (int j = 0; j < RPS; ++j) {
                const bool m = x <= x1 && yb + j <= y1 && lv[j] == want;
                unsigned v[COLOC_MAXC];
                bool pos[COLOC_MAXC];
                cnt += m ? 1u : 0u;
#pragma unroll
                for (int c = 0; c < COLOC_MAXC; ++c) {
                    v[c] = m ? iv[j][c] : 0u;
                    pos[c] = m && (int)iv[j][c] > ti[c];
                    if (c < P.nch) {
                        s[c] += v[c];
                        q[c] += (u64)v[c] * v[c];
                        np[c] += pos[c] ? 1u : 0u;
                    }
                }
#pragma unroll
                for (int k = 0; k < COLOC_MAXP; ++k)
                    if (P.out[k] >= 0) {
                        const int a = coloc_slot_a(k), b = coloc_slot_b(k);
                        ab[k] += (u64)v[a] * v[b];
                        aif[k] += pos[b] ? v[a] : 0u;
                        bif[k] += pos[a] ? v[b] : 0u;
                        both[k] += (pos[a] && pos[b]) ? 1u : 0u;
                    }
            }
        }
    }
    u64 t[32];
#pragma unroll
    for (int c = 0; c < COLOC_MAXC; ++c) t[CO_S + c] = s[c], t[CO_Q + c] = q[c];
#pragma unroll
    for (int k = 0; k < COLOC_MAXP; ++k) t[CO_AB + k] = ab[k], t[CO_AIF + k] = aif[k], t[CO_BIF + k] = bif[k];
    t[CO_CNT + 0] = (u64)cnt | ((u64)np[0] << 32);
    t[CO_CNT + 1] = (u64)np[1] | ((u64)np[2] << 32);
    t[CO_CNT + 2] = (u64)np[3] | ((u64)both[0] << 32);
    t[CO_CNT + 3] = (u64)both[1] | ((u64)both[2] << 32);
    t[CO_CNT + 4] = (u64)both[3] | ((u64)both[4] << 32);
    t[CO_CNT + 5] = (u64)both[5];
    const u64 mine = amt_wave_reduce_scatter<32, amt_op_sum>(t, lane);  // value k in the lanes 2 k, 2 k + 1
    if (!(lane & 1)) red[lane >> 1] = mine;
    __syncthreads();
    if (lane < COLOC_MAXP && P.out[lane] >= 0) {
        const int k = lane, a = coloc_slot_a(k), b = coloc_slot_b(k);
        const u64 N = coloc_count(red, 0), na = coloc_count(red, 1 + a), nb = coloc_count(red, 1 + b);
        const u64 nab = coloc_count(red, 5 + k);
        const u64 Sa = red[CO_S + a], Sb = red[CO_S + b], Qa = red[CO_Q + a], Qb = red[CO_Q + b];
        const u64 AB = red[CO_AB + k], AIF = red[CO_AIF + k], BIF = red[CO_BIF + k];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        // exact 128-bit differences, rounded only once they are formed: nothing cancels in float64
        const double da = diff_of_products(N, Qa, Sa, Sa), db = diff_of_products(N, Qb, Sb, Sb);
        const double num = diff_of_products(N, AB, Sa, Sb);
        double m1 = Sa ? (double)AIF / (double)Sa : 0.0, m2 = Sb ? (double)BIF / (double)Sb : 0.0;
        double i1 = na ? (double)nab / (double)na : 0.0, i2 = nb ? (double)nab / (double)nb : 0.0;
        if (P.swap[k]) {
            double tmp = m1;
            m1 = m2, m2 = tmp;
            tmp = i1;
            i1 = i2, i2 = tmp;
        }
        double* o = rows + (size_t)P.out[k] * AMT_COLOC_NCOLS;
        o[AMT_COLOC_PEARSON] = (da == 0.0 || db == 0.0) ? nan : num / sqrt(da * db);  // da == 0: n Saa == Sa^2, exactly
        o[AMT_COLOC_OVERLAP] = (Qa == 0 || Qb == 0) ? nan : (double)AB / sqrt((double)Qa * (double)Qb);
        o[AMT_COLOC_M1] = m1;
        o[AMT_COLOC_M2] = m2;
        o[AMT_COLOC_INTERSECTION1] = i1;
        o[AMT_COLOC_INTERSECTION2] = i2;
    }
}

// float64 images: one wave per label and requested pair, two sweeps as rp_intensity_f64_kernel makes them -- raw sums,
// extrema and the thresholded sums first, then the sums centred on the means.  Plain and untuned.
__global__ void __launch_bounds__(64) coloc_f64_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                       const double* __restrict__ inten, int C,
                                                       const double* __restrict__ thr, int ca, int cb, int pair,
                                                       double* __restrict__ table, int npairs, int H, int W,
                                                       int max_label) {
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    const amt_box box = amt_load_box(bbox, li);
    const int y0 = box.y0, x0 = box.x0, y1 = box.y1, x1 = box.x1;
    double* o = table + (li * (size_t)npairs + pair) * AMT_COLOC_NCOLS;
    if (box.absent()) {
        if (lane == 0) coloc_write_empty(o);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* lab = labels + (size_t)plane * n;
    const double* A = inten + ((size_t)plane * C + ca) * n;
    const double* B = inten + ((size_t)plane * C + cb) * n;
    const double ta = thr[(size_t)plane * C + ca], tb = thr[(size_t)plane * C + cb];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double cnt = 0, sa = 0, sb = 0, qa = 0, qb = 0, pab = 0, aif = 0, bif = 0, na = 0, nb = 0, nab = 0;
    double mna = inf, mxa = -inf, mnb = inf, mxb = -inf;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0 + lane; x <= x1; x += 64)
            if (lab[(size_t)y * W + x] == l + 1) {
                const double a = A[(size_t)y * W + x], b = B[(size_t)y * W + x];
                const bool pa = a > ta, pb = b > tb;
                cnt += 1.0;
                sa += a;
                sb += b;
                qa += a * a;
                qb += b * b;
                pab += a * b;
                if (pb) aif += a;
                if (pa) bif += b;
                na += pa ? 1.0 : 0.0;
                nb += pb ? 1.0 : 0.0;
                nab += (pa && pb) ? 1.0 : 0.0;
                mna = a < mna ? a : mna;
                mxa = a > mxa ? a : mxa;
                mnb = b < mnb ? b : mnb;
                mxb = b > mxb ? b : mxb;
            }
    cnt = amt_wave_sum(cnt), sa = amt_wave_sum(sa), sb = amt_wave_sum(sb), qa = amt_wave_sum(qa), qb = amt_wave_sum(qb);
    pab = amt_wave_sum(pab), aif = amt_wave_sum(aif), bif = amt_wave_sum(bif);
    na = amt_wave_sum(na), nb = amt_wave_sum(nb), nab = amt_wave_sum(nab);
    mna = amt_wave_min(mna), mxa = amt_wave_max(mxa), mnb = amt_wave_min(mnb), mxb = amt_wave_max(mxb);
    const double ma = sa / cnt, mb = sb / cnt;
    double cab = 0, caa = 0, cbb = 0;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0 + lane; x <= x1; x += 64)
            if (lab[(size_t)y * W + x] == l + 1) {
                const double da = A[(size_t)y * W + x] - ma, db = B[(size_t)y * W + x] - mb;
                cab += da * db;
                caa += da * da;
                cbb += db * db;
            }
    cab = amt_wave_sum(cab), caa = amt_wave_sum(caa), cbb = amt_wave_sum(cbb);
    if (lane == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const bool constant = !(mna < mxa) || !(mnb < mxb);  // min == max over the label (an empty label too)
        const double den = sqrt(caa * cbb), oden = sqrt(qa * qb);
        o[AMT_COLOC_PEARSON] = (constant || den == 0.0) ? nan : cab / den;
        o[AMT_COLOC_OVERLAP] = oden == 0.0 ? nan : pab / oden;
        o[AMT_COLOC_M1] = sa != 0.0 ? aif / sa : 0.0;
        o[AMT_COLOC_M2] = sb != 0.0 ? bif / sb : 0.0;
        o[AMT_COLOC_INTERSECTION1] = na != 0.0 ? nab / na : 0.0;
        o[AMT_COLOC_INTERSECTION2] = nb != 0.0 ? nab / nb : 0.0;
    }
}

extern "C" int amt_colocalization(amt_ctx* ctx, const int32_t* labels, const void* intensity, int in_code, int C,
                                  const double* thresholds_dev, const int32_t* pairs_host, int npairs,
                                  double* table_dev, int nplanes, int H, int W, int max_label) {
    AMT_REQUIRE(labels && intensity && thresholds_dev && pairs_host && table_dev && nplanes >= 0 && H > 0 && W > 0 &&
                    max_label >= 0 && C >= 2 && npairs >= 1,
                "colocalization: bad arguments");
    AMT_REQUIRE(in_code == AMT_U16 || in_code == AMT_F64, "colocalization: intensity must be AMT_U16 or AMT_F64");
    AMT_REQUIRE((size_t)H * W <= 0xffffffffull, "colocalization: planes of more than 2^32 - 1 pixels are not supported");
    for (int p = 0; p < npairs; ++p) {
        const int i = pairs_host[2 * p], j = pairs_host[2 * p + 1];
        AMT_REQUIRE(i >= 0 && i < C && j >= 0 && j < C && i != j,
                    "colocalization: pair %d = (%d, %d) must name two different channels below %d", p, i, j, C);
    }
    AMT_CHECK_OPERANDS("amt_colocalization", amt_in("labels", labels, amt_span(4, nplanes, H, W)),
                       amt_in("intensity", intensity, amt_span(amt_esize(in_code), nplanes, C, H, W)),
                       amt_in("thresholds_dev", thresholds_dev, amt_span(8, nplanes, C)),
                       amt_out("table_dev", table_dev, amt_span(8, nplanes, max_label, npairs, AMT_COLOC_NCOLS)));
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0 || max_label == 0) return AMT_OK;
    amt_scratch s(ctx);
    amt_buf<int> bbox(s, (size_t)nplanes * max_label * 4);
    AMT_TRY(s.commit());
    AMT_TRY(amt_i_label_boxes(ctx, labels, bbox, nullptr, nplanes, H, W, max_label));
    if (in_code == AMT_F64) {
        for (int p = 0; p < npairs; ++p) {
            hipLaunchKernelGGL(coloc_f64_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox,
                               (const double*)intensity, C, thresholds_dev, pairs_host[2 * p], pairs_host[2 * p + 1], p,
                               table_dev, npairs, H, W, max_label);
            AMT_LAUNCH_CHECK();
        }
        return AMT_OK;
    }
    // Cover the requested pairs with channel lists of at most COLOC_MAXC: a list starts from the first pair that is
    // still open and takes the channels of further open pairs while they fit; every open pair inside the list whose
    // slot pair is free is answered by that launch (a pair asked for twice, or both ways round, waits for the next).
    std::vector<char> done((size_t)npairs, 0);
    for (int first = 0; first < npairs; ++first) {
        if (done[first]) continue;
        coloc_launch P;
        P.nch = 0;
        for (int c = 0; c < COLOC_MAXC; ++c) P.chan[c] = 0;
        for (int k = 0; k < COLOC_MAXP; ++k) P.out[k] = -1, P.swap[k] = 0;
        auto slot_of = [&](int ch) {
            for (int c = 0; c < P.nch; ++c)
                if (P.chan[c] == ch) return c;
            return -1;
        };
        for (int p = first; p < npairs; ++p) {
            if (done[p]) continue;
            const int i = pairs_host[2 * p], j = pairs_host[2 * p + 1];
            const int missing = (slot_of(i) < 0 ? 1 : 0) + (slot_of(j) < 0 ? 1 : 0);
            if (P.nch + missing > COLOC_MAXC) continue;
            if (slot_of(i) < 0) P.chan[P.nch++] = i;
            if (slot_of(j) < 0) P.chan[P.nch++] = j;
        }
        for (int p = first; p < npairs; ++p) {
            if (done[p]) continue;
            const int si = slot_of(pairs_host[2 * p]), sj = slot_of(pairs_host[2 * p + 1]);
            if (si < 0 || sj < 0) continue;
            const int a = si < sj ? si : sj, b = si < sj ? sj : si;
            int k = 0;
            while (coloc_slot_a(k) != a || coloc_slot_b(k) != b) ++k;
            if (P.out[k] >= 0) continue;
            P.out[k] = p;
            P.swap[k] = si > sj ? 1 : 0;
            done[p] = 1;
        }
        hipLaunchKernelGGL(coloc_u16_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox,
                           (const uint16_t*)intensity, C, thresholds_dev, P, table_dev, npairs, H, W, max_label);
        AMT_LAUNCH_CHECK();
    }
    return AMT_OK;
}
