// Per-label Haralick texture (AMT_RPX_TEXTURE of amt_regionprops_ext): the symmetric grey-level co-occurrence matrices
// of every label in the four directions 0 / 45 / 90 / 135 degrees and the thirteen features of each.  The definitions
// stand in include/amt_hip.h.
//
// One single-wave workgroup per (label, plane) sweeps the label's bounding box, one channel after the other, and counts
// the four directions in that one sweep.  A box of at most TX_TILE pixels (a nucleus) is read ONCE per channel: every
// pixel is quantised once into a byte of LDS (its level, or TX_OUTSIDE for a pixel of another label), and the pairs are
// formed from those bytes.  A larger box is swept in memory: a lane loads its pixel and the four partners at (0, d),
// (d, -d), (d, 0), (d, d) in the label plane and in the channel, all from coordinates clamped into the box.  Either way
// nothing outside the box -- and with it nothing outside the plane -- is ever read: a partner that would lie outside the
// box cannot carry the label and is dropped before it is looked at.
//
// Counters: four tables of L x L 32-bit integers in dynamic LDS (4 L^2 x 4 bytes: 1 KiB at L = 8, 64 KiB at L = 64).  A
// pair {p, p + offset} adds ONE to the one-sided table A[q(p)][q(p + offset)] (half the LDS atomics of a table that is
// kept symmetric); the matrix of the definition is G = A + A^T, formed where it is read.  Integer LDS atomics are sums:
// no arrival order changes a table.  The marginals (row totals, sums over i + j and over |i - j|) are integer LDS
// atomics too, so everything up to "divide by the total" is exact.  The float64 sums of the features run lane-strided
// over the table in ascending order and are reduced eight at a time (amt_wave_reduce_scatter): one fixed order, two
// runs give identical bytes.  Nothing is written to global memory but the feature rows or, in a counts call, the matrices G.
#include "amt_internal.h"
#include "amt_perlabel.h"

namespace {

constexpr int TX_MAXL = 64;      // levels: one row total per lane
constexpr int TX_TILE = 4096;    // pixels of a box that is kept quantised in LDS (64 x 64; a nucleus has ~800)
constexpr unsigned TX_OUTSIDE = 255u;

// q = min(L - 1, floor((clip(v, lo, hi) - lo) / (hi - lo) * L)), in float64 in exactly that order; den = hi - lo
__device__ __forceinline__ int tx_quantise(double v, double lo, double hi, double den, int L) {
    if (!(hi > lo)) return 0;
    double c = v < lo ? lo : v;
    c = c > hi ? hi : c;
    const int q = (int)floor((c - lo) / den * (double)L);
    return q > L - 1 ? L - 1 : (q < 0 ? 0 : q);  // q < 0: only from the unsupported NaN; the counters stay in bounds
}

__device__ __forceinline__ double tx_plogp(double p) { return p > 0.0 ? p * log2(p) : 0.0; }

// One sweep of the box in memory: the pairs of the four directions into the one-sided tables tab[a][q(p)][q(partner)].
template <typename T>
__device__ __forceinline__ void tx_count(const int* __restrict__ Lp, const T* __restrict__ I, int W, const amt_box& box,
                                         int want, int lc, int lane, int d, double lo, double hi, int L, unsigned* tab) {
    const int x0 = box.x0, x1 = box.x1, y1 = box.y1;
    const double den = hi - lo;
    const int LL = L * L;
    amt_box_for_cells(box, lc, lane, [&](int x, int y) {
        const int xc = x <= x1 ? x : x1, yc = y <= y1 ? y : y1;
        const int yd = yc + d <= y1 ? yc + d : y1;  // the partners' row and columns, clamped into the box
        const int xr = xc + d <= x1 ? xc + d : x1, xl = xc - d >= x0 ? xc - d : x0;
        const size_t r0 = (size_t)yc * W, rd = (size_t)yd * W;
        const int l0 = Lp[r0 + xc], l1 = Lp[r0 + xr], l2 = Lp[rd + xl], l3 = Lp[rd + xc], l4 = Lp[rd + xr];
        const T v0 = I[r0 + xc], v1 = I[r0 + xr], v2 = I[rd + xl], v3 = I[rd + xc], v4 = I[rd + xr];
        if (!(x <= x1 && y <= y1 && l0 == want)) return;
        const bool right = x + d <= x1, left = x - d >= x0, down = y + d <= y1;
        unsigned* row = tab + tx_quantise((double)v0, lo, hi, den, L) * L;
        if (right && l1 == want) atomicAdd(&row[tx_quantise((double)v1, lo, hi, den, L)], 1u);
        if (down && left && l2 == want) atomicAdd(&row[LL + tx_quantise((double)v2, lo, hi, den, L)], 1u);
        if (down && l3 == want) atomicAdd(&row[2 * LL + tx_quantise((double)v3, lo, hi, den, L)], 1u);
        if (down && right && l4 == want) atomicAdd(&row[3 * LL + tx_quantise((double)v4, lo, hi, den, L)], 1u);
    });
}

// The same for a box of at most TX_TILE pixels: tile[(y - y0) w + (x - x0)] = the pixel's level, TX_OUTSIDE where it
// does not carry the label.  The fill keeps amt_box_for_pixels' own form -- two row slots per step, their four loads
// issued together -- because it stores every cell of the box, not only the label's; the pairs then come from the tile.
template <typename T>
__device__ __forceinline__ void tx_count_tile(const int* __restrict__ Lp, const T* __restrict__ I, int W,
                                              const amt_box& box, int want, int lc, int lane, int d, double lo, double hi,
                                              int L, unsigned* tab, unsigned char* tile) {
    const int x0 = box.x0, y0 = box.y0, x1 = box.x1, y1 = box.y1, w = x1 - x0 + 1;
    const int cols = 1 << lc, rw = 64 >> lc;
    const int col = lane & (cols - 1), sub = lane >> lc;
    const double den = hi - lo;
    const int LL = L * L;
    for (int yb = y0 + sub; yb - sub <= y1; yb += 2 * rw) {
        const int ya = yb, yc = yb + rw;
        const size_t ra = (size_t)(ya <= y1 ? ya : y1) * W, rc = (size_t)(yc <= y1 ? yc : y1) * W;
        for (int xb = x0; xb <= x1; xb += cols) {
            const int x = xb + col, xc = x <= x1 ? x : x1;
            const int la = Lp[ra + xc], lb = Lp[rc + xc];
            const T va = I[ra + xc], vb = I[rc + xc];
            if (x <= x1 && ya <= y1)
                tile[(ya - y0) * w + (x - x0)] =
                    (unsigned char)(la == want ? (unsigned)tx_quantise((double)va, lo, hi, den, L) : TX_OUTSIDE);
            if (x <= x1 && yc <= y1)
                tile[(yc - y0) * w + (x - x0)] =
                    (unsigned char)(lb == want ? (unsigned)tx_quantise((double)vb, lo, hi, den, L) : TX_OUTSIDE);
        }
    }
    __syncthreads();
    const int dw = d * w;
    amt_box_for_cells(box, lc, lane, [&](int x, int y) {
        if (!(x <= x1 && y <= y1)) return;
        const int at = (y - y0) * w + (x - x0);
        const unsigned q0 = tile[at];
        if (q0 == TX_OUTSIDE) return;
        const bool right = x + d <= x1, left = x - d >= x0, down = y + d <= y1;
        unsigned* row = tab + q0 * L;
        const unsigned q1 = right ? tile[at + d] : TX_OUTSIDE;
        const unsigned q2 = down && left ? tile[at + dw - d] : TX_OUTSIDE;
        const unsigned q3 = down ? tile[at + dw] : TX_OUTSIDE;
        const unsigned q4 = down && right ? tile[at + dw + d] : TX_OUTSIDE;
        if (q1 != TX_OUTSIDE) atomicAdd(&row[q1], 1u);
        if (q2 != TX_OUTSIDE) atomicAdd(&row[LL + q2], 1u);
        if (q3 != TX_OUTSIDE) atomicAdd(&row[2 * LL + q3], 1u);
        if (q4 != TX_OUTSIDE) atomicAdd(&row[3 * LL + q4], 1u);
    });
}

// LDS of the feature pass: integer marginals of G and what the float64 sums read per level
struct tx_marginals {
    unsigned rowsum[TX_MAXL];       // R(i) = sum_j G(i, j)
    unsigned sum[2 * TX_MAXL];      // S(k) = sum_{i + j = k} G, k = 0 .. 2 L - 2
    unsigned diff[TX_MAXL];         // D(k) = sum_{|i - j| = k} G
    double px[TX_MAXL];             // R(i) / total
    double lpx[TX_MAXL];            // log2 px(i), 0 where px(i) = 0
};

// eight per-lane partial sums -> the eight totals in every lane: one reduce-scatter (10 exchanges) and a broadcast each
__device__ __forceinline__ void tx_sum8(double (&t)[8], int lane) {
    const double mine = amt_wave_reduce_scatter<8, amt_op_sum>(t, lane);  // total i in the lanes 8 i .. 8 i + 7
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = __shfl(mine, 8 * i);
}

// G = A + A^T of one direction from its one-sided table A, as it is: the counts output.
__device__ __forceinline__ void tx_write_counts(const unsigned* A, int L, int lane, uint32_t* __restrict__ glcm) {
    for (int e = lane; e < L * L; e += 64) {
        const int i = e / L, j = e - i * L;
        glcm[e] = A[e] + A[j * L + i];
    }
}

// The thirteen features of one direction from its one-sided table A (G = A + A^T), written by lane 0.  Every lane
// returns with the table read: the caller may clear it.
__device__ __forceinline__ void tx_features(const unsigned* A, int L, int lane, tx_marginals& m, double* __restrict__ out) {
    const int LL = L * L;
    for (int i = lane; i < TX_MAXL; i += 64) m.rowsum[i] = 0u, m.diff[i] = 0u;
    for (int i = lane; i < 2 * TX_MAXL; i += 64) m.sum[i] = 0u;
    __syncthreads();
    unsigned long long tot = 0;
    for (int e = lane; e < LL; e += 64) {
        const int i = e / L, j = e - i * L;
        const unsigned g = A[e] + A[j * L + i];
        if (g) {
            atomicAdd(&m.rowsum[i], g);
            atomicAdd(&m.sum[i + j], g);
            atomicAdd(&m.diff[i > j ? i - j : j - i], g);
            tot += g;
        }
    }
    tot = amt_wave_sum(tot);
    __syncthreads();
    if (tot == 0) {  // no pair in this direction
        amt_fill_row(out, AMT_TEX_NCOLS, amt_quiet_nan(), lane);
        return;
    }
    const double N = (double)tot;
    // ---- what needs the total alone.  Lane k owns px(k), p-(k) and p+(k), p+(k + 64); the matrix goes lane-strided
    const unsigned rk = lane < L ? m.rowsum[lane] : 0u;
    const double pxk = (double)rk / N;
    const double lpxk = pxk > 0.0 ? log2(pxk) : 0.0;
    const double pdk = lane < L ? (double)m.diff[lane] / N : 0.0;
    const double psa = lane < 2 * L - 1 ? (double)m.sum[lane] / N : 0.0;
    const double psb = lane + 64 < 2 * L - 1 ? (double)m.sum[lane + 64] / N : 0.0;
    const double k = (double)lane, kb = (double)(lane + 64);
    m.px[lane] = pxk;
    m.lpx[lane] = lpxk;
    const int nlevels = __popcll(__ballot(rk != 0u));
    double asm_ = 0.0, idm = 0.0, ent = 0.0;
    for (int e = lane; e < LL; e += 64) {
        const int i = e / L, j = e - i * L;
        const unsigned g = A[e] + A[j * L + i];
        if (g) {
            const double p = (double)g / N, dij = (double)(i - j);
            asm_ += p * p;
            idm += p / (1.0 + dij * dij);
            ent += p * log2(p);
        }
    }
    double s[8];
    s[0] = k * pxk;                                            // mu
    s[1] = pxk * lpxk;                                         // -HX
    s[2] = k * psa + kb * psb;                                 // sum_average
    s[3] = tx_plogp(psa) + (2 * L - 1 > 64 ? tx_plogp(psb) : 0.0);  // -sum_entropy
    s[4] = k * pdk;                                            // m of the differences
    s[5] = k * k * pdk;                                        // contrast
    s[6] = tx_plogp(pdk);                                      // -difference_entropy
    s[7] = ent;                                                // -HXY
    tx_sum8(s, lane);
    const double mu = s[0], hx = 0.0 - s[1], sum_avg = s[2], sum_ent = 0.0 - s[3], dmean = s[4], contrast = s[5];
    const double diff_ent = 0.0 - s[6], hxy = 0.0 - s[7];
    __syncthreads();  // px, lpx are written
    // ---- the centred sums and what needs px of both levels
    double cnum = 0.0, hxy1 = 0.0, hxy2 = 0.0;
    for (int e = lane; e < LL; e += 64) {
        const int i = e / L, j = e - i * L;
        const unsigned g = A[e] + A[j * L + i];
        const double pi = m.px[i], pj = m.px[j], ll = m.lpx[i] + m.lpx[j];
        hxy2 += pi * pj * ll;
        if (g) {
            const double p = (double)g / N;
            cnum += ((double)i - mu) * ((double)j - mu) * p;
            hxy1 += p * ll;
        }
    }
    double c[8];
    c[0] = (k - mu) * (k - mu) * pxk;                                                          // variance
    c[1] = (k - sum_avg) * (k - sum_avg) * psa + (kb - sum_avg) * (kb - sum_avg) * psb;        // sum_variance
    c[2] = (k - dmean) * (k - dmean) * pdk;                                                    // difference_variance
    c[3] = cnum;
    c[4] = hxy1;
    c[5] = hxy2;
    c[6] = asm_;
    c[7] = idm;
    tx_sum8(c, lane);
    __syncthreads();  // the table and the marginals are read
    if (lane == 0) {
        const double var = c[0], arg = 1.0 - exp(-2.0 * ((0.0 - c[5]) - hxy));
        out[AMT_TEX_ANGULAR_SECOND_MOMENT] = c[6];
        out[AMT_TEX_CONTRAST] = contrast;
        out[AMT_TEX_CORRELATION] = nlevels == 1 ? 1.0 : c[3] / var;
        out[AMT_TEX_VARIANCE] = var;
        out[AMT_TEX_INVERSE_DIFFERENCE_MOMENT] = c[7];
        out[AMT_TEX_SUM_AVERAGE] = sum_avg;
        out[AMT_TEX_SUM_VARIANCE] = c[1];
        out[AMT_TEX_SUM_ENTROPY] = sum_ent;
        out[AMT_TEX_ENTROPY] = hxy;
        out[AMT_TEX_DIFFERENCE_VARIANCE] = c[2];
        out[AMT_TEX_DIFFERENCE_ENTROPY] = diff_ent;
        out[AMT_TEX_INFO_MEASURE_1] = hx == 0.0 ? 0.0 : (hxy - (0.0 - c[4])) / hx;
        out[AMT_TEX_INFO_MEASURE_2] = sqrt(arg > 0.0 ? arg : 0.0);
    }
}

template <typename T>
__global__ void __launch_bounds__(64) texture_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                     const T* __restrict__ inten, int C,
                                                     const double* __restrict__ ranges, int L, int d,
                                                     double* __restrict__ table, uint32_t* __restrict__ glcm, int H, int W,
                                                     int max_label) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ tx_marginals marg;
    __shared__ unsigned char tile[TX_TILE];
    unsigned* tab = reinterpret_cast<unsigned*>(smem_raw);  // [4][L][L]
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    const int LL = L * L;
    // a launch writes one of the two: the feature rows (table) or the counts (glcm)
    double* out = table ? table + li * (size_t)C * 4 * AMT_TEX_NCOLS : nullptr;
    uint32_t* gout = table ? nullptr : glcm + li * (size_t)C * 4 * LL;
    const amt_box box = amt_load_box(bbox, li);
    if (box.absent()) {
        if (out) amt_fill_row(out, C * 4 * AMT_TEX_NCOLS, amt_quiet_nan(), lane);
        if (gout)
            for (size_t i = lane; i < (size_t)C * 4 * LL; i += 64) gout[i] = 0u;
        return;
    }
    const size_t n = (size_t)H * W;
    const int* Lp = labels + (size_t)plane * n;
    const int want = l + 1, lc = amt_box_layout(box.x0, box.x1);
    const bool kept = (long long)box.w() * box.h() <= TX_TILE;
    for (int c = 0; c < C; ++c) {
        const T* I = inten + ((size_t)plane * C + c) * n;
        const double lo = ranges[((size_t)plane * C + c) * 2], hi = ranges[((size_t)plane * C + c) * 2 + 1];
        for (int i = lane; i < 4 * LL; i += 64) tab[i] = 0u;
        __syncthreads();  // the counters are clear; the last direction of the channel before has left the tile
        if (kept)
            tx_count_tile(Lp, I, W, box, want, lc, lane, d, lo, hi, L, tab, tile);
        else
            tx_count(Lp, I, W, box, want, lc, lane, d, lo, hi, L, tab);
        __syncthreads();
        if (out) {
            for (int a = 0; a < 4; ++a)
                tx_features(tab + a * LL, L, lane, marg, out + ((size_t)c * 4 + a) * AMT_TEX_NCOLS);
        } else {
            for (int a = 0; a < 4; ++a) tx_write_counts(tab + a * LL, L, lane, gout + ((size_t)c * 4 + a) * LL);
            __syncthreads();  // the tables are read: the next channel may clear them
        }
    }
}

template <typename T>
int tx_launch(amt_ctx* ctx, const int* labels, const int* bbox, const void* intensity, int C, const double* ranges,
              int L, int d, double* table, uint32_t* glcm, int nplanes, int H, int W, int max_label) {
    const size_t lds = (size_t)4 * L * L * sizeof(unsigned);
    // 64 KiB of counters at L = 64 plus the marginals and the tile: more than the 64 KiB a launch gets without asking.
    // Always the largest size any call needs, so that calls from several host threads cannot undercut one another.
    AMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&texture_kernel<T>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      4 * TX_MAXL * TX_MAXL * (int)sizeof(unsigned)));
    hipLaunchKernelGGL(texture_kernel<T>, dim3(max_label, nplanes), dim3(64), lds, ctx->stream, labels, bbox,
                       (const T*)intensity, C, ranges, L, d, table, glcm, H, W, max_label);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // namespace

// AMT_RPX_TEXTURE / AMT_RPX_TEXTURE_COUNTS of amt_regionprops_ext, which has taken `columns` apart: levels, distance, and
// whether the call writes the counts instead of the features.  ranges = its table_dev (an input here), out = its wtable_dev.
int amt_i_texture(amt_ctx* ctx, const int32_t* labels, const void* intensity, int in_code, int C, const double* ranges,
                  int levels, int distance, bool counts, double* out, int nplanes, int H, int W, int max_label) {
    AMT_REQUIRE(labels && intensity && ranges && out && nplanes >= 0 && H > 0 && W > 0 && max_label >= 0 && C >= 1,
                "regionprops_ext: AMT_RPX_TEXTURE takes labels, intensity planes (C >= 1), the ranges in table_dev and "
                "wtable_dev");
    AMT_REQUIRE(in_code == AMT_U16 || in_code == AMT_F64, "regionprops_ext: intensity must be AMT_U16 or AMT_F64");
    AMT_REQUIRE(levels >= 2 && levels <= TX_MAXL, "regionprops_ext: texture levels %d out of range 2..%d", levels, TX_MAXL);
    AMT_REQUIRE(distance >= 1 && distance <= 255, "regionprops_ext: texture distance %d out of range 1..255", distance);
    // a counter holds up to twice the pairs of a direction, fewer than the plane's pixels
    AMT_REQUIRE((size_t)H * W <= 0x7fffffffull, "regionprops_ext: texture on planes of more than 2^31 - 1 pixels is not supported");
    const size_t rows = amt_span(1, nplanes, max_label, (long long)C * 4);  // (plane, label, channel, direction)
    const size_t obytes = counts ? rows * (size_t)levels * levels * 4 : rows * AMT_TEX_NCOLS * 8;
    AMT_CHECK_OPERANDS("amt_regionprops_ext", amt_in("labels", labels, amt_span(4, nplanes, H, W)),
                       amt_in("intensity", intensity, amt_span(amt_esize(in_code), nplanes, C, H, W)),
                       amt_in("table_dev", ranges, amt_span(8, nplanes, C, 2)),
                       amt_out("wtable_dev", out, obytes));
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0 || max_label == 0) return AMT_OK;
    uint32_t* glcm = counts ? reinterpret_cast<uint32_t*>(out) : nullptr;
    double* table = counts ? nullptr : out;
    amt_scratch s(ctx);
    amt_buf<int> bbox(s, (size_t)nplanes * max_label * 4);
    AMT_TRY(s.commit());
    AMT_TRY(amt_i_label_boxes(ctx, labels, bbox, nullptr, nplanes, H, W, max_label));
    if (in_code == AMT_U16)
        return tx_launch<uint16_t>(ctx, labels, bbox, intensity, C, ranges, levels, distance, table, glcm, nplanes, H, W,
                                   max_label);
    return tx_launch<double>(ctx, labels, bbox, intensity, C, ranges, levels, distance, table, glcm, nplanes, H, W,
                             max_label);
}
