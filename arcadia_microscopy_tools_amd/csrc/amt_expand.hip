// skimage.segmentation.expand_labels(label_image, distance) on 2-D planes (SK/segmentation/_expand_labels.py:
//   distances, nearest = distance_transform_edt(label_image == 0, return_indices=True)
//   out[distances <= distance] = label_image[nearest][distances <= distance]).
//
// A background pixel p receives a label iff D2(p) <= nmax, with D2 the exact integer squared Euclidean distance to the
// nearest labelled pixel and nmax = max{n : sqrt(float64(n)) <= distance} computed by the caller: the device compares
// integers only.  The label is that of the nearest labelled pixel; when pixels of SEVERAL labels lie at distance D2(p)
// the SMALLEST of those labels wins (scipy's feature transform keeps whichever tied pixel its scan meets first, an
// artefact of its algorithm; this rule does not depend on tiling, plane size or batch position).
//
// Evaluation, separable like the EDT's (amt_edt.hip), every pass carrying (distance, label) and comparing
// lexicographically:
//   rows   : (g, l)(y,x) = distance to and label of the nearest labelled pixel of row y within r = floor(sqrt(nmax))
//            columns, the smaller label when the left and the right one are equally far.  "Labelled" flags are packed
//            into 64-pixel words; the nearest flag on either side is a clz / ffs, its label one gathered read.
//   columns: min over k of (k^2 + g(y+-k,x)^2, l(y+-k,x)), scanning k outward while k^2 <= min(best, nmax) -- "<=", so
//            that an equally distant candidate with a smaller label is still seen.  A block stages (g, l) of 64 columns
//            x (32 + 2 * min(r, 32)) rows in LDS; searches deeper than 32 rows (r > 32 only) evaluate (g, l) from the
//            words and the label plane.  They are exact and degrade, never fail.
#include "amt_internal.h"

constexpr unsigned XL_INF = 0xFFFFu;  // no labelled pixel of this row within reach
constexpr unsigned XL_NONE = 0xFFFFFFFFu;
constexpr int XL_ROWS = 32, XL_HALO = 32, XL_TROWS = XL_ROWS + 2 * XL_HALO;
constexpr int XL_WORDS_PER_WAVE = 8;
constexpr int XL_CHUNK = 6;  // window rows a lane stages together

// word i = "labelled" flags of 64 consecutive pixels of a row (bit b = column 64 * wi + b; beyond W: not labelled).
// A wave reads the 64 labels of a word in one coalesced load and votes.
__global__ void __launch_bounds__(256) expand_label_words_kernel(const int* __restrict__ lab, unsigned long long* __restrict__ lw,
                                                                 int W, int WW, size_t nwords) {
    const int lane = threadIdx.x & 63;
    const size_t i0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * XL_WORDS_PER_WAVE;
    if (i0 >= nwords) return;  // whole wave
    int v[XL_WORDS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < XL_WORDS_PER_WAVE; ++j) {
        const size_t i = i0 + j;
        v[j] = 0;
        if (i < nwords) {
            const size_t row = i / WW;  // plane * H + y
            const int x = (int)(i - row * WW) * 64 + lane;
            if (x < W) v[j] = lab[row * W + x];
        }
    }
#pragma unroll
    for (int j = 0; j < XL_WORDS_PER_WAVE; ++j) {
        const unsigned long long b = __ballot(v[j] != 0);
        if (lane == 0 && i0 + j < nwords) lw[i0 + j] = b;
    }
}

// (g, l) of pixel x of a row: distance to the nearest labelled pixel of the row and its label (the smaller label when
// both sides are equally far); XL_INF / 0 when none lies within gmax (<= 32767) columns
__device__ __forceinline__ void xl_row_nearest(const unsigned long long* __restrict__ zr, const int* __restrict__ Lrow, int WW,
                                               int x, unsigned gmax, unsigned& g, int& l) {
    const int wi = x >> 6, bit = x & 63;
    const unsigned long long own = zr[wi];
    if ((own >> bit) & 1ull) {
        g = 0u;
        l = Lrow[x];
        return;
    }
    unsigned dl = XL_NONE, dr = XL_NONE;
    unsigned long long m = own & ((1ull << bit) - 1ull);
    int w = wi;
    const int wlo = (unsigned)x > gmax ? (int)((unsigned)x - gmax) >> 6 : 0;
    while (m == 0 && w > wlo) m = zr[--w];
    if (m) dl = (unsigned)(x - (w * 64 + 63 - __clzll((long long)m)));
    m = bit == 63 ? 0ull : (own >> (bit + 1)) << (bit + 1);
    w = wi;
    const int whi = (int)(((unsigned)x + gmax) >> 6) < WW - 1 ? (int)(((unsigned)x + gmax) >> 6) : WW - 1;
    while (m == 0 && w < whi) m = zr[++w];
    if (m) dr = (unsigned)(w * 64 + __ffsll((long long)m) - 1 - x);
    const unsigned d = dl < dr ? dl : dr;
    g = XL_INF;
    l = 0;
    if (d > gmax) return;
    g = d;
    const int a = dl == d ? Lrow[x - (int)d] : 0x7fffffff;
    const int b = dr == d ? Lrow[x + (int)d] : 0x7fffffff;
    l = a < b ? a : b;
}

// candidate (c, lc) replaces (best, bl) when it is nearer, or equally near with a smaller label
__device__ __forceinline__ void xl_take(unsigned c, int lc, unsigned& best, int& bl) {
    const bool t = c < best || (c == best && lc < bl);
    best = t ? c : best;
    bl = t ? lc : bl;
}

__global__ void __launch_bounds__(256) expand_labels_kernel(const unsigned long long* __restrict__ lw, const int* __restrict__ lab,
                                                            int* __restrict__ out, int H, int W, int WW, unsigned nmax, int r,
                                                            int ring) {
    __shared__ __attribute__((aligned(16))) unsigned short gt[XL_TROWS][64];
    __shared__ __attribute__((aligned(16))) int lt[XL_TROWS][64];
    __shared__ unsigned long long zs[XL_TROWS][3];  // flag words of the window rows: left neighbour, own, right neighbour
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = blockIdx.x;  // the tile's word column
    const int y0 = blockIdx.y * XL_ROWS;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const unsigned long long* zp = lw + (size_t)blockIdx.z * H * WW;
    const int* L = lab + plane;
    const int halo = r < XL_HALO ? r : XL_HALO;  // rows above / below the tile that the LDS search can reach
    const unsigned gcap = r < 32767 ? (unsigned)r : 32767u;
    // ---- (g, l) of the window: a wave per row, a lane per column ----
    const int lo = XL_HALO - halo, hi = XL_HALO + XL_ROWS + halo;  // the window rows the search can reach
    const int x = wi * 64 + lane;
    if (r <= 64) {
        // The nearest flag within 64 columns lies in the pixel's own word or a neighbouring one: the three words of
        // every row go to LDS with all loads in flight at once, (g, source columns) are arithmetic on them, and the
        // labels of a chunk of rows are gathered together (a row loop of load word -> clz -> load label -> store
        // waits for memory twice per row).
        for (int i = threadIdx.x; i < (hi - lo) * 3; i += 256) {
            const int rr = lo + i / 3, c = i % 3;
            const int y = y0 - XL_HALO + rr, w = wi - 1 + c;
            zs[rr][c] = (y >= 0 && y < H && w >= 0 && w < WW) ? zp[(size_t)y * WW + w] : 0ull;
        }
        __syncthreads();
        const int xc = x < W ? x : W - 1;
        for (int base = lo + wave; base < hi; base += 4 * XL_CHUNK) {
            unsigned g[XL_CHUNK];
            int pa[XL_CHUNK], pb[XL_CHUNK], la[XL_CHUNK], lb[XL_CHUNK];
#pragma unroll
            for (int i = 0; i < XL_CHUNK; ++i) {
                const int rr = base + 4 * i < hi ? base + 4 * i : base;  // past the window: the chunk's first row again
                const unsigned long long own = zs[rr][1];
                const bool self = (own >> lane) & 1ull;
                unsigned long long m = own & ((1ull << lane) - 1ull);
                int w = wi;
                if (m == 0) m = zs[rr][0], w = wi - 1;
                const unsigned dl = m ? (unsigned)(x - (w * 64 + 63 - __clzll((long long)m))) : XL_NONE;
                m = lane == 63 ? 0ull : (own >> (lane + 1)) << (lane + 1);
                w = wi;
                if (m == 0) m = zs[rr][2], w = wi + 1;
                const unsigned dr = m ? (unsigned)(w * 64 + __ffsll((long long)m) - 1 - x) : XL_NONE;
                const unsigned d = self ? 0u : (dl < dr ? dl : dr);
                const bool none = d > gcap;
                g[i] = none ? XL_INF : d;
                pa[i] = none ? xc : (dl == d ? x - (int)d : x + (int)d);  // self: d = 0, both are x
                pb[i] = none ? xc : (dr == d ? x + (int)d : x - (int)d);
            }
#pragma unroll
            for (int i = 0; i < XL_CHUNK; ++i) {  // unconditional loads from clamped rows: all in flight together
                const int rr = base + 4 * i < hi ? base + 4 * i : base;
                const int y = y0 - XL_HALO + rr;
                const int* Lrow = L + (size_t)(y < 0 ? 0 : (y < H ? y : H - 1)) * W;
                la[i] = Lrow[pa[i]];
                lb[i] = Lrow[pb[i]];
            }
#pragma unroll
            for (int i = 0; i < XL_CHUNK; ++i) {
                const int rr = base + 4 * i < hi ? base + 4 * i : base;
                gt[rr][lane] = (unsigned short)g[i];
                lt[rr][lane] = g[i] == XL_INF ? 0 : (la[i] < lb[i] ? la[i] : lb[i]);
            }
        }
    } else {
        for (int rr = lo + wave; rr < hi; rr += 4) {
            const int y = y0 - XL_HALO + rr;
            unsigned g = XL_INF;
            int l = 0;
            if (y >= 0 && y < H && x < W) xl_row_nearest(zp + (size_t)y * WW, L + (size_t)y * W, WW, x, gcap, g, l);
            gt[rr][lane] = (unsigned short)g;
            lt[rr][lane] = l;
        }
    }
    __syncthreads();
    // ---- the column search: a lane owns four consecutive pixels of a row (one 8-byte read brings the four g of a row
    // above / below; the labels are read only when one of the eight candidates can win) ----
    const int c4 = (lane & 15) * 4, rsub = lane >> 4;
    const int xg = wi * 64 + c4;
    if (xg >= W) return;
    const bool vec = xg + 3 < W && (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
#pragma unroll 1
    for (int j = 0; j < XL_ROWS / 16; ++j) {
        const int ly = XL_HALO + wave * (XL_ROWS / 4) + rsub + 4 * j;
        const int y = y0 - XL_HALO + ly;
        if (y >= H) continue;
        unsigned best[4];
        int bl[4];
        bool own[4];
        {
            const uint2 gq = *reinterpret_cast<const uint2*>(&gt[ly][c4]);
            const int4 lq = *reinterpret_cast<const int4*>(&lt[ly][c4]);
            const unsigned g0[4] = {gq.x & 0xFFFFu, gq.x >> 16, gq.y & 0xFFFFu, gq.y >> 16};
            const int l0[4] = {lq.x, lq.y, lq.z, lq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                own[i] = g0[i] == 0u;
                best[i] = g0[i] == XL_INF ? XL_NONE : g0[i] * g0[i];
                bl[i] = l0[i];
            }
        }
        for (unsigned k = 1; k <= (unsigned)halo; ++k) {
            const unsigned kk = k * k;
            bool go = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) go |= kk <= (best[i] < nmax ? best[i] : nmax);
            if (!go) break;
            const uint2 uq = *reinterpret_cast<const uint2*>(&gt[ly - (int)k][c4]);
            const uint2 dq = *reinterpret_cast<const uint2*>(&gt[ly + (int)k][c4]);
            const unsigned gu[4] = {uq.x & 0xFFFFu, uq.x >> 16, uq.y & 0xFFFFu, uq.y >> 16};
            const unsigned gd[4] = {dq.x & 0xFFFFu, dq.x >> 16, dq.y & 0xFFFFu, dq.y >> 16};
            unsigned cu[4], cd[4];
            bool need = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                cu[i] = gu[i] == XL_INF ? XL_NONE : kk + gu[i] * gu[i];  // < 2^31: k, g <= 32767
                cd[i] = gd[i] == XL_INF ? XL_NONE : kk + gd[i] * gd[i];
                need |= (cu[i] != XL_NONE && cu[i] <= best[i]) || (cd[i] != XL_NONE && cd[i] <= best[i]);
            }
            if (need) {
                const int4 ul = *reinterpret_cast<const int4*>(&lt[ly - (int)k][c4]);
                const int4 dl = *reinterpret_cast<const int4*>(&lt[ly + (int)k][c4]);
                const int lu[4] = {ul.x, ul.y, ul.z, ul.w};
                const int ld[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (cu[i] != XL_NONE) xl_take(cu[i], lu[i], best[i], bl[i]);
                    if (cd[i] != XL_NONE) xl_take(cd[i], ld[i], best[i], bl[i]);
                }
            }
        }
        int res[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned b = best[i];
            int l = bl[i];
            const int x = xg + i;
            if (!own[i] && x < W && r > XL_HALO) {  // beyond the LDS halo
                for (unsigned k = XL_HALO + 1; k <= (unsigned)r; ++k) {
                    const unsigned kk = k * k;  // <= nmax < 2^31
                    const unsigned bound = b < nmax ? b : nmax;
                    if (kk > bound) break;
                    const int yu = y - (int)k, yd = y + (int)k;
                    if (yu < 0 && yd >= H) break;
                    // only g with kk + g^2 <= bound matter; the float square root is off by far less than the + 1
                    unsigned gmax = (unsigned)sqrtf((float)(bound - kk)) + 1u;
                    gmax = gmax < gcap ? gmax : gcap;
                    unsigned g;
                    int lc;
                    if (yu >= 0) {
                        xl_row_nearest(zp + (size_t)yu * WW, L + (size_t)yu * W, WW, x, gmax, g, lc);
                        if (g != XL_INF) xl_take(kk + g * g, lc, b, l);
                    }
                    if (yd < H) {
                        xl_row_nearest(zp + (size_t)yd * WW, L + (size_t)yd * W, WW, x, gmax, g, lc);
                        if (g != XL_INF) xl_take(kk + g * g, lc, b, l);
                    }
                }
            }
            res[i] = own[i] ? (ring ? 0 : l) : (b <= nmax ? l : 0);
        }
        const size_t i0 = plane + (size_t)y * W + xg;
        if (vec) {
            *reinterpret_cast<int4*>(out + i0) = make_int4(res[0], res[1], res[2], res[3]);
        } else {
            for (int i = 0; i < 4 && xg + i < W; ++i) out[i0 + i] = res[i];
        }
    }
}

extern "C" int amt_expand_labels(amt_ctx* ctx, const int32_t* labels, int32_t* out, int nplanes, int H, int W, int64_t nmax,
                                 int ring) {
    AMT_CHECK_OPERANDS("amt_expand_labels", amt_in("labels", labels, amt_span(4, nplanes, H, W)),
                       amt_out("out", out, amt_span(4, nplanes, H, W)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(labels && out && nplanes >= 0 && H > 0 && W > 0, "expand_labels: bad arguments");
    AMT_REQUIRE(H <= 32768 && W <= 32768, "expand_labels: image larger than 32768 pixels per side");
    AMT_REQUIRE(nplanes <= 65535, "expand_labels: more than 65535 planes in one call");
    if (nplanes == 0) return AMT_OK;
    if (nmax < 0) {  // distance < 0: `distances <= distance` holds nowhere, not even inside the labels
        AMT_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)nplanes * H * W * sizeof(int32_t), ctx->stream));
        return AMT_OK;
    }
    const unsigned nm = nmax > 0x7fffffffll ? 0x7fffffffu : (unsigned)nmax;  // D2 < 2^31 on planes of this size
    int r = (int)sqrt((double)nm);
    while ((long long)r * r > (long long)nm) --r;
    while ((long long)(r + 1) * (r + 1) <= (long long)nm) ++r;
    const int WW = (W + 63) / 64;
    const size_t nwords = (size_t)nplanes * H * WW;
    amt_scratch s(ctx);
    amt_buf<unsigned long long> lw(s, nwords);
    AMT_TRY(s.commit());
    const size_t nwaves = (nwords + XL_WORDS_PER_WAVE - 1) / XL_WORDS_PER_WAVE;
    hipLaunchKernelGGL(expand_label_words_kernel, dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, ctx->stream, labels, lw, W,
                       WW, nwords);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(expand_labels_kernel, dim3(WW, (H + XL_ROWS - 1) / XL_ROWS, nplanes), dim3(256), 0, ctx->stream, lw,
                       labels, out, H, W, WW, nm, r, ring);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- label planes of other element types -------------------------------------------------------------------------
// uint8 / uint16 label planes (a Pipeline uploads uint16 images as they are) widen to the int32 the kernels take, and an
// int32 result narrows back; values are copied, the caller vouches that they fit
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) cast_labels_kernel(const TI* __restrict__ in, TO* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (TO)in[i];
}

extern "C" int amt_cast_labels(amt_ctx* ctx, const void* in, int in_dtype, void* out, int out_dtype, size_t n) {
    // the two element sizes differ for every pair the cast accepts: never in place
    AMT_CHECK_OPERANDS("amt_cast_labels", amt_in("in", in, amt_span(amt_esize(in_dtype), (long long)n)),
                       amt_out("out", out, amt_span(amt_esize(out_dtype), (long long)n)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(in && out, "cast_labels: bad arguments");
    if (n == 0) return AMT_OK;
    const dim3 grid(amt_grid_for(n, 256)), block(256);
#define XL_CAST(TI, TO) \
    hipLaunchKernelGGL((cast_labels_kernel<TI, TO>), grid, block, 0, ctx->stream, (const TI*)in, (TO*)out, n)
    if (in_dtype == AMT_U8 && out_dtype == AMT_I32) XL_CAST(uint8_t, int32_t);
    else if (in_dtype == AMT_U16 && out_dtype == AMT_I32) XL_CAST(uint16_t, int32_t);
    else if (in_dtype == AMT_I32 && out_dtype == AMT_U8) XL_CAST(int32_t, uint8_t);
    else if (in_dtype == AMT_I32 && out_dtype == AMT_U16) XL_CAST(int32_t, uint16_t);
    else AMT_REQUIRE(false, "cast_labels: unsupported conversion %d -> %d", in_dtype, out_dtype);
#undef XL_CAST
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
