// Robust per-label intensity statistics (AMT_RPX_ROBUST of amt_regionprops_ext): the 25th / 50th / 75th percentile and
// the median absolute deviation of every channel over every label, as np.percentile (method 'linear') gives them.
// The definitions stand in include/amt_hip.h, the rank rule in amt_rank_rule.h.
//
// One single-wave workgroup per (label, plane) sweeps the label's bounding box, one channel after the other.  A sweep
// reads the box in the label plane and in the channel: lanes own columns, two row slots per step with their four loads
// issued together from coordinates clamped into the box (amt_box_for_pixels of amt_perlabel.h); a uint16 box of at
// most 32 row slots is read once per channel and kept in LDS for the later sweeps (rb_kept_pixels).  Nothing is written
// to global memory but the four results: the selection state lives in LDS and registers, so no scratch grows with a
// label's area and no global atomic is used.  Counters are 32 bits wide: exact up to the plane's 2^31 - 2 pixels.
#include "amt_internal.h"
#include "amt_perlabel.h"
#include "amt_rank_rule.h"

namespace {

// A table of `count` counters, lane l owning the `per` consecutive ones from l * per (per * 64 >= count).
// lsum = the lane's total, lexc = the total of the lanes before it.
__device__ __forceinline__ void rb_lane_totals(const unsigned* tab, int per, int count, int lane, unsigned& lexc,
                                               unsigned& lsum) {
    unsigned s = 0;
    for (int i = 0; i < per; ++i) {
        const int b = lane * per + i;
        s += b < count ? tab[b] : 0u;
    }
    unsigned inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    lsum = s;
    lexc = inc - s;
}

// the counter that holds the element of 0-based rank r (< the table's total), and how many elements lie before it
__device__ __forceinline__ void rb_locate(const unsigned* tab, int per, int count, int lane, unsigned lexc, unsigned lsum,
                                          unsigned r, unsigned& bin, unsigned& before) {
    const bool mine = r >= lexc && r - lexc < lsum;  // true in exactly one lane
    unsigned b = 0, c = 0;
    if (mine) {
        unsigned run = lexc;
        for (int i = 0; i < per; ++i) {
            const int k = lane * per + i;
            const unsigned cn = k < count ? tab[k] : 0u;
            if (r - run < cn) {
                b = (unsigned)k;
                c = run;
                break;
            }
            run += cn;
        }
    }
    const unsigned long long m = __ballot(mine);
    const int src = m ? __ffsll((long long)m) - 1 : 0;
    bin = __shfl(b, src);
    before = __shfl(c, src);
}

// ---- uint16: counting selection in LDS --------------------------------------------------------------------------
// The keys of a selection lie in 0..kmax and are mapped onto the RB_BINS counters by key >> s, with the smallest s that
// fits.  One sweep counts them (LDS integer atomics: sums, so any arrival order gives the same table), a prefix sum over
// the table places all NR ranks at once.  With s > 0 a second sweep counts the low s bits of the keys that fell into
// the at most NR coarse bins the ranks lie in: rank i's fine counters are the 2^s from (j << s), j being the first rank
// that lies in the same coarse bin.  A selection costs one or two sweeps whatever the label's area and values.
constexpr int RB_BINS = AMT_ROBUST_LDS_BINS;
static_assert((RB_BINS & (RB_BINS - 1)) == 0 && RB_BINS >= 1024, "counter index by shift; a lane scans up to RB_BINS / 64 counters");
// the fine counters share the table: six coarse bins of 65536 / RB_BINS values each for the quartiles, two of
// 131072 / RB_BINS keys each for MAD
static_assert(6 * (65536 / RB_BINS) <= RB_BINS && 2 * (131072 / RB_BINS) <= RB_BINS, "fine counters must fit the table");


// Where a sweep gets the label's pixels of one channel from.  rb_box_pixels: the memory sweep over the bounding box.
struct rb_box_pixels {
    const int* __restrict__ L;
    const uint16_t* __restrict__ I;
    int W;
    amt_box box;
    int want, lc, lane;
    template <typename F>
    __device__ __forceinline__ void for_each(F&& f) const {
        amt_box_for_pixels(L, I, W, box, want, lc, lane, f);
    }
};

// rb_kept_pixels: a box of at most 64 columns and RB_KEEP row slots (32 rows of 33..64 columns, 64 rows of 17..32,
// ...: a nucleus) is read from memory ONCE per channel: a lane puts the value of its pixel of row slot j into its own
// LDS cell kept[j * 64 + lane] and bit j of a register says whether that pixel belongs to the label; every sweep of the
// channel's selections then reads the lane's own cells (no exchange between lanes, so no barrier).  Same pixels, same
// sums: the results do not depend on the source.  The loads of four row slots are issued together from clamped
// coordinates.  LDS: 4 KiB of counters + 4 KiB of kept values per workgroup of one wave, 20 workgroups per CU, which is
// also what the registers admit (5 waves per SIMD).
constexpr int RB_KEEP = 32;
struct rb_kept_pixels {
    const uint16_t* kept;
    unsigned mask;
    int nslots, lane;
    __device__ __forceinline__ static bool fits(int w, int h, int lc) { return w <= 64 && h <= RB_KEEP * (64 >> lc); }
    __device__ __forceinline__ void load(uint16_t* cells, const int* __restrict__ L, const uint16_t* __restrict__ I, int W,
                                         const amt_box& box, int want, int lc, int lane_) {
        const int x0 = box.x0, y0 = box.y0, x1 = box.x1, y1 = box.y1;
        const int cols = 1 << lc, rw = 64 >> lc;  // the box is at most `cols` wide
        const int x = x0 + (lane_ & (cols - 1)), sub = lane_ >> lc;
        const int xc = x <= x1 ? x : x1;
        kept = cells;
        lane = lane_;
        nslots = (y1 - y0) / rw + 1;  // <= RB_KEEP
        mask = 0u;
        for (int j = 0; j < nslots; j += 4) {  // j + 3 <= RB_KEEP - 1
            int lv[4];
            uint16_t iv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int y = y0 + (j + k) * rw + sub;
                lv[k] = L[(size_t)(y <= y1 ? y : y1) * W + xc];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int y = y0 + (j + k) * rw + sub;
                iv[k] = I[(size_t)(y <= y1 ? y : y1) * W + xc];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int y = y0 + (j + k) * rw + sub;
                mask |= (x <= x1 && y <= y1 && lv[k] == want) ? 1u << (j + k) : 0u;
                cells[(j + k) * 64 + lane_] = iv[k];
            }
        }
    }
    template <typename F>
    __device__ __forceinline__ void for_each(F&& f) const {
        for (int j = 0; j < nslots; ++j)
            if ((mask >> j) & 1u) f(kept[j * 64 + lane]);
    }
};

template <int NR, typename P, typename K>
__device__ __forceinline__ void rb_select_u16(const P& px, int lane, unsigned* tab, unsigned kmax,
                                              const unsigned (&rk)[NR], unsigned (&key_out)[NR], K&& key) {
    int s = 0;
    while ((kmax >> s) >= (unsigned)RB_BINS) ++s;
    // only the counters the window reaches are cleared and scanned: a nucleus spans a few hundred levels
    const int used = (int)(kmax >> s) + 1, used_per = (used + 63) / 64;
    for (int i = lane; i < used; i += 64) tab[i] = 0u;
    __syncthreads();
    px.for_each([&](uint16_t v) { atomicAdd(&tab[key(v) >> s], 1u); });
    __syncthreads();
    unsigned lexc, lsum, bin[NR], before[NR];
    rb_lane_totals(tab, used_per, used, lane, lexc, lsum);
#pragma unroll
    for (int i = 0; i < NR; ++i) rb_locate(tab, used_per, used, lane, lexc, lsum, rk[i], bin[i], before[i]);
    if (s == 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) key_out[i] = bin[i];
        __syncthreads();  // the table is read: the next selection may clear it
        return;
    }
    __syncthreads();
    for (int i = lane; i < (NR << s); i += 64) tab[i] = 0u;
    __syncthreads();
    const unsigned low = (1u << s) - 1u;
    px.for_each([&](uint16_t v) {
        const unsigned k = key(v), b = k >> s;
        int slot = -1;
#pragma unroll
        for (int i = NR - 1; i >= 0; --i) slot = b == bin[i] ? i : slot;  // the first rank of that coarse bin
        if (slot >= 0) atomicAdd(&tab[((unsigned)slot << s) + (k & low)], 1u);
    });
    __syncthreads();
    const int fine = 1 << s, per = fine >= 64 ? fine / 64 : 1;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        int slot = i;
#pragma unroll
        for (int j = i - 1; j >= 0; --j) slot = bin[j] == bin[i] ? j : slot;
        unsigned fbin, fbefore;
        rb_lane_totals(tab + (slot << s), per, fine, lane, lexc, lsum);
        rb_locate(tab + (slot << s), per, fine, lane, lexc, lsum, rk[i] - before[i], fbin, fbefore);
        key_out[i] = (bin[i] << s) + fbin;
    }
    __syncthreads();
}

// the four results of one channel over the label's pixels `px` (at least one), written by lane 0
template <typename P>
__device__ __forceinline__ void rb_channel_u16(const P& px, int lane, unsigned* tab, double* __restrict__ out) {
    unsigned cnt = 0, mn = 65535u, mx = 0u;
    px.for_each([&](uint16_t v) {
        cnt += 1u;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    });
    cnt = amt_wave_sum(cnt);
    mn = amt_wave_min(mn);
    mx = amt_wave_max(mx);
    double res[4];
    if (mn == mx) {  // a constant label: every quantile is the value, every distance 0
        res[AMT_RPX_QCOL_Q25] = res[AMT_RPX_QCOL_MEDIAN] = res[AMT_RPX_QCOL_Q75] = (double)mn;
        res[AMT_RPX_QCOL_MAD] = 0.0;
    } else {
        unsigned rk[6], val[6];
        int t4[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const amt_rank r = amt_rank_of(cnt, 0.25 * (q + 1));
            rk[2 * q] = (unsigned)r.lo;
            rk[2 * q + 1] = (unsigned)r.hi;
            t4[q] = amt_rank_quarters(r.t);
        }
        rb_select_u16<6>(px, lane, tab, mx - mn, rk, val, [&](uint16_t v) { return (unsigned)v - mn; });
#pragma unroll
        for (int q = 0; q < 3; ++q) res[q] = amt_quartile_u16(mn + val[2 * q], mn + val[2 * q + 1], t4[q]);
        // MAD: the median's ranks among the keys |2 v - 2 median|, which lie in 0..kmax
        const bool odd = (cnt & 1u) != 0;
        const unsigned m2 = amt_median2_u16(mn + val[2], mn + val[3], odd);
        const unsigned below = m2 - 2u * mn, above = 2u * mx - m2;
        const unsigned mrk[2] = {rk[2], rk[3]};
        unsigned mkey[2];
        rb_select_u16<2>(px, lane, tab, below > above ? below : above, mrk, mkey, [&](uint16_t v) {
            const unsigned v2 = 2u * (unsigned)v;
            return v2 > m2 ? v2 - m2 : m2 - v2;
        });
        res[AMT_RPX_QCOL_MAD] = amt_mad_u16(mkey[0], mkey[1], odd);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = res[k];
    }
}

__global__ void __launch_bounds__(64) robust_u16_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                        const uint16_t* __restrict__ inten, int C,
                                                        double* __restrict__ wtable, int H, int W, int max_label) {
    __shared__ unsigned tab[RB_BINS];
    __shared__ uint16_t cells[RB_KEEP * 64];
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    double* out = wtable + li * (size_t)C * 4;
    const amt_box box = amt_load_box(bbox, li);
    if (box.absent()) {  // numpy on an empty array
        amt_fill_row(out, C * 4, amt_quiet_nan(), lane);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* L = labels + (size_t)plane * n;
    const int want = l + 1, w = box.w(), h = box.h(), lc = amt_box_layout(box.x0, box.x1);
    const bool keep = rb_kept_pixels::fits(w, h, lc);
    for (int c = 0; c < C; ++c) {
        const uint16_t* I = inten + ((size_t)plane * C + c) * n;
        if (keep) {
            rb_kept_pixels px;
            px.load(cells, L, I, W, box, want, lc, lane);
            rb_channel_u16(px, lane, tab, out + c * 4);
        } else {
            const rb_box_pixels px{L, I, W, box, want, lc, lane};
            rb_channel_u16(px, lane, tab, out + c * 4);
        }
    }
}

// ---- float64: plain and untuned, like coloc_f64_kernel ------------------------------------------------------------
// Order-preserving 64-bit keys (amt_f64_key), MSB-first radix select with a 256-counter LDS histogram: 8 sweeps of 8
// bits per rank, one rank after the other (a rank that repeats an earlier one is copied).  MAD is a second selection
// on |v - median|, the difference taken in float64.
template <typename K>
__device__ __forceinline__ unsigned long long rb_select_f64(const int* __restrict__ L, const double* __restrict__ I,
                                                            int W, const amt_box& box, int want, int lc, int lane,
                                                            unsigned* hist, unsigned r, K&& key) {
    unsigned long long prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);  // the bits already decided
        for (int i = lane; i < 256; i += 64) hist[i] = 0u;
        __syncthreads();
        amt_box_for_pixels(L, I, W, box, want, lc, lane, [&](double v) {
            const unsigned long long k = key(v);
            if (((k ^ prefix) & himask) == 0) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
        });
        __syncthreads();
        unsigned lexc, lsum, bin, before;
        rb_lane_totals(hist, 4, 256, lane, lexc, lsum);
        rb_locate(hist, 4, 256, lane, lexc, lsum, r, bin, before);
        prefix |= (unsigned long long)bin << shift;
        r -= before;
        __syncthreads();
    }
    return prefix;
}

__global__ void __launch_bounds__(64) robust_f64_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                        const double* __restrict__ inten, int C,
                                                        double* __restrict__ wtable, int H, int W, int max_label) {
    __shared__ unsigned hist[256];
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    double* out = wtable + li * (size_t)C * 4;
    const amt_box box = amt_load_box(bbox, li);
    if (box.absent()) {
        amt_fill_row(out, C * 4, amt_quiet_nan(), lane);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* L = labels + (size_t)plane * n;
    const int want = l + 1, lc = amt_box_layout(box.x0, box.x1);
    for (int c = 0; c < C; ++c) {
        const double* I = inten + ((size_t)plane * C + c) * n;
        unsigned cnt = 0;
        amt_box_for_pixels(L, I, W, box, want, lc, lane, [&](double) { cnt += 1u; });
        cnt = amt_wave_sum(cnt);
        unsigned rk[6];
        double t[3], val[6], res[4];
        for (int q = 0; q < 3; ++q) {
            const amt_rank r = amt_rank_of(cnt, 0.25 * (q + 1));
            rk[2 * q] = (unsigned)r.lo;
            rk[2 * q + 1] = (unsigned)r.hi;
            t[q] = r.t;
        }
        for (int i = 0; i < 6; ++i) {
            int same = -1;
            for (int j = 0; j < i; ++j) same = rk[j] == rk[i] ? j : same;
            val[i] = same >= 0 ? val[same]
                               : amt_key_f64(rb_select_f64(L, I, W, box, want, lc, lane, hist, rk[i],
                                                           [](double v) { return amt_f64_key(v); }));
        }
        for (int q = 0; q < 3; ++q) res[q] = amt_np_lerp(val[2 * q], val[2 * q + 1], t[q]);
        const double med = res[AMT_RPX_QCOL_MEDIAN];
        auto dist = [med](double v) { return amt_f64_key(fabs(v - med)); };
        const double da = amt_key_f64(rb_select_f64(L, I, W, box, want, lc, lane, hist, rk[2], dist));
        const double db = rk[3] == rk[2]
                              ? da
                              : amt_key_f64(rb_select_f64(L, I, W, box, want, lc, lane, hist, rk[3], dist));
        res[AMT_RPX_QCOL_MAD] = amt_np_lerp(da, db, t[1]);
        if (lane == 0) {
            for (int k = 0; k < 4; ++k) out[c * 4 + k] = res[k];
        }
    }
}

}  // namespace

int amt_i_robust_intensity(amt_ctx* ctx, const int* labels, const int* bbox, const void* intensity, int in_code, int C,
                           double* wtable, int nplanes, int H, int W, int max_label) {
    if (in_code == AMT_U16)
        hipLaunchKernelGGL(robust_u16_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox,
                           (const uint16_t*)intensity, C, wtable, H, W, max_label);
    else
        hipLaunchKernelGGL(robust_f64_kernel, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox,
                           (const double*)intensity, C, wtable, H, W, max_label);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
