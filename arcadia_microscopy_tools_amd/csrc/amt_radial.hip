// Per-label radial intensity distribution and inscribed radii (AMT_RPX_RADIAL of amt_regionprops_ext): the exact squared
// Euclidean distance of every pixel of a label to the label's own edge, the ring and the wedge of every pixel, and per
// (channel, ring) the three columns AMT_RAD_*.  The definitions stand in include/amt_hip.h.
//
// One single-wave workgroup per (label, plane) works inside the label's bounding box; nothing outside the box -- and with
// it nothing outside the plane -- is ever read: the rows above and below the box and the columns left and right of it
// hold no pixel of the label, which is all the distance needs to know of them.
//   column phase  g(y, x) = the vertical distance from a pixel of the label to the nearest pixel of its column that does
//                 not carry the label: one scan down and one scan up per column, a lane per column;
//   row phase     d2(y, x) = min over x' of (x - x')^2 + g(y, x')^2 with g = 0 where (y, x') does not carry the label
//                 (the two columns beside the box included), widened from x' = x until (x - x')^2 reaches the best value;
//                 the same sweep gives n, Sum y, Sum x, max d2 and the exact sum of the roots;
//   code pass     ring and wedge of every pixel from integers, kept as one code per pixel; ring x wedge pixel counts;
//   channel pass  one sweep per channel (AMT_F64: per channel and occupied ring) for the ring x wedge sums.
// g is kept SATURATED: a value g >= sat only ever offers candidates >= sat^2, and sat^2 is larger than any d2 of its
// tier (below), so the minimum never comes from a saturated value and stays exact.
//
// Two tiers by the box's cell count.  Up to RD_LDS_TILE cells (a nucleus has ~800, an expanded(12) cell ~3000) g, d2
// and the code share one 16-bit word per cell in LDS: a box of that size is at most 64 cells across its narrower side,
// so d <= 32 and d2 <= 1024 < 63^2.  A larger box keeps them in two planes of arena scratch (16-bit g / code, 32-bit d2)
// at the label's OWN pixels, which no other workgroup touches: a plane has at most 2^31 - 1 pixels, so its narrower side
// is at most 46340, d <= 23171 and d2 < 32767^2.  What one phase stores there the next phase reads through other lanes:
// stores are fenced at agent scope and the loads bypass the vector L1 (a line may have been read before, for a
// neighbouring label's pixels, by another wave of the same CU).
//
// Counting is integer (LDS atomics on 32- and 64-bit integers are sums: no arrival order changes them).  The sum of the
// roots is exact: every root is an integer multiple of 2^-52 below 2^15, summed in 128 bits and rounded once.  AMT_F64
// sums run per lane in the order of the box walk and through amt_wave_reduce_scatter: one fixed order.  No global atomics.
#include "amt_internal.h"
#include "amt_perlabel.h"

namespace {

constexpr int RD_MAXB = 16;             // rings
constexpr int RD_NW = 8;                // wedges
constexpr int RD_LDS_TILE = 4096;       // cells of a box that is kept in LDS
constexpr unsigned RD_OUTSIDE = 255u;   // the code of a cell that does not carry the label (a code is ring * 8 + wedge < 128)

typedef unsigned long long rd_u64;
typedef unsigned __int128 rd_u128;

// ---- where g, d2 and the code of a box live: LDS or the label's own pixels of two scratch planes ------------------------
// get_* give 0 (g, d2) or RD_OUTSIDE (code) for a cell that does not carry the label; set_* take whether it does.
// LDS: one 16-bit word per cell.  Membership (0 / 1), then g in the low 6 bits (0 = the cell does not carry the label),
// then d2 - 1 in the 10 bits above it (d2 is 1..1024), at last the code in the whole word.  The row phase writes the
// d2 field of a lane's own cell while other lanes read that cell's g field: either word they see holds the same g.
struct rd_lds {
    static constexpr unsigned SAT = 63u;
    unsigned short* t;  // [h][w]
    int y0, x0, w;
    __device__ __forceinline__ int at(int y, int x) const { return (y - y0) * w + (x - x0); }
    __device__ __forceinline__ bool member(int y, int x) const { return t[at(y, x)] != 0; }
    __device__ __forceinline__ unsigned get_g(int y, int x) const { return t[at(y, x)] & 63u; }
    __device__ __forceinline__ void set_g(int y, int x, bool own, unsigned v) const { t[at(y, x)] = (unsigned short)(own ? v : 0u); }
    __device__ __forceinline__ unsigned get_d2(int y, int x) const {
        const unsigned v = t[at(y, x)];
        return (v & 63u) ? (v >> 6) + 1u : 0u;
    }
    __device__ __forceinline__ void set_d2(int y, int x, bool own, unsigned v) const {
        if (own) t[at(y, x)] = (unsigned short)((t[at(y, x)] & 63u) | ((v - 1u) << 6));
    }
    __device__ __forceinline__ unsigned get_code(int y, int x) const { return t[at(y, x)]; }
    __device__ __forceinline__ void set_code(int y, int x, bool own, unsigned v) const { t[at(y, x)] = (unsigned short)(own ? v : RD_OUTSIDE); }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
};
static_assert(RD_LDS_TILE <= 4096 && rd_lds::SAT * rd_lds::SAT > 1024u, "d2 - 1 of the LDS tier must fit ten bits, below the saturated g squared");
struct rd_mem {
    static constexpr unsigned SAT = 32767u;
    const int* L;        // the label plane
    unsigned short* g;   // plane: g, then the code, at the label's own pixels
    unsigned* d2;        // plane
    int W, want;
    __device__ __forceinline__ size_t at(int y, int x) const { return (size_t)y * W + x; }
    __device__ __forceinline__ bool member(int y, int x) const { return L[at(y, x)] == want; }
    __device__ __forceinline__ unsigned get_g(int y, int x) const {
        return member(y, x) ? (unsigned)__hip_atomic_load(&g[at(y, x)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    }
    __device__ __forceinline__ void set_g(int y, int x, bool own, unsigned v) const {
        if (own) g[at(y, x)] = (unsigned short)v;
    }
    __device__ __forceinline__ unsigned get_d2(int y, int x) const {
        return member(y, x) ? __hip_atomic_load(&d2[at(y, x)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    }
    __device__ __forceinline__ void set_d2(int y, int x, bool own, unsigned v) const {
        if (own) d2[at(y, x)] = v;
    }
    __device__ __forceinline__ unsigned get_code(int y, int x) const {
        return member(y, x) ? (unsigned)__hip_atomic_load(&g[at(y, x)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : RD_OUTSIDE;
    }
    __device__ __forceinline__ void set_code(int y, int x, bool own, unsigned v) const { set_g(y, x, own, v); }
    __device__ __forceinline__ void barrier() const {
        __threadfence();
        __syncthreads();
    }
};

// LDS of a workgroup besides the tile
struct rd_counters {
    unsigned nbw[RD_MAXB * RD_NW];  // pixels per (ring, wedge)
    rd_u64 sbw[RD_MAXB * RD_NW];    // AMT_U16: the sums per (ring, wedge); AMT_F64: the same as float64 bits
};

// what the row phase leaves in every lane
struct rd_geom {
    unsigned n, dmax2;
    long long sy, sx;
    double root_sum;  // Sum sqrt(d2), correctly rounded
};

// a 128-bit integer to the nearest float64, ties to even
__device__ __forceinline__ double rd_round_u128(rd_u128 t) {
    const rd_u64 hi = (rd_u64)(t >> 64), lo = (rd_u64)t;
    if (hi == 0 && lo < (1ull << 53)) return (double)lo;
    const int top = hi ? 127 - __clzll((long long)hi) : 63 - __clzll((long long)lo);  // the highest set bit, >= 53
    const int shift = top - 52;
    rd_u64 mant = (rd_u64)(t >> shift);
    const rd_u128 rem = t & (((rd_u128)1 << shift) - 1), half = (rd_u128)1 << (shift - 1);
    if (rem > half || (rem == half && (mant & 1ull))) ++mant;  // 2^53 is still exact as a float64
    return (double)mant * __longlong_as_double((long long)(1023 + shift) << 52);
}

// the tile's membership words from the label plane: every cell of the box once
__device__ __forceinline__ void rd_fill_members(const int* __restrict__ Lp, int W, const amt_box& box, int want, int lc,
                                                int lane, const rd_lds& st) {
    const int x1 = box.x1, y1 = box.y1;
    amt_box_for_loaded_cells(
        box, lc, lane, [&](int yc, int xc) { return Lp[(size_t)yc * W + xc]; },
        [&](int x, int y, int l) {
            if (x <= x1 && y <= y1) st.t[st.at(y, x)] = (unsigned short)(l == want);
        });
}

// column phase: a lane per column, down then up
template <typename S>
__device__ __forceinline__ void rd_columns(const amt_box& box, int lane, const S& st) {
    for (int xb = box.x0; xb <= box.x1; xb += 64) {
        const int x = xb + lane;
        if (x > box.x1) continue;
        unsigned run = 0;
        for (int y = box.y0; y <= box.y1; ++y) {
            const bool m = st.member(y, x);
            run = m ? run + 1 : 0u;
            st.set_g(y, x, m, run < S::SAT ? run : S::SAT);
        }
    }
    st.barrier();
    for (int xb = box.x0; xb <= box.x1; xb += 64) {
        const int x = xb + lane;
        if (x > box.x1) continue;
        unsigned run = 0;
        for (int y = box.y1; y >= box.y0; --y) {
            const unsigned cur = st.get_g(y, x);
            run = cur ? run + 1 : 0u;
            if (run < cur) st.set_g(y, x, true, run);
        }
    }
    st.barrier();
}

// row phase and first sweep
template <typename S>
__device__ __forceinline__ rd_geom rd_distances(const amt_box& box, int lc, int lane, const S& st) {
    const int x0 = box.x0, x1 = box.x1, y1 = box.y1;
    unsigned n = 0, dmax2 = 0;
    long long sy = 0, sx = 0;
    rd_u128 roots = 0;  // in units of 2^-52
    amt_box_for_cells(box, lc, lane, [&](int x, int y) {
        if (x > x1 || y > y1) return;
        const unsigned g0 = st.get_g(y, x);
        if (g0 == 0u) {
            st.set_d2(y, x, false, 0u);
            return;
        }
        unsigned best = g0 * g0;
        for (unsigned dx = 1; dx * dx < best; ++dx) {
            const int xl = x - (int)dx, xr = x + (int)dx;
            const unsigned gl = xl >= x0 ? st.get_g(y, xl) : 0u, gr = xr <= x1 ? st.get_g(y, xr) : 0u;
            const unsigned cl = dx * dx + gl * gl, cr = dx * dx + gr * gr;
            best = cl < best ? cl : best;
            best = cr < best ? cr : best;
        }
        st.set_d2(y, x, true, best);
        ++n;
        sy += y;
        sx += x;
        dmax2 = best > dmax2 ? best : dmax2;
        const long long bits = __double_as_longlong(sqrt((double)best));  // 1 <= root < 2^15
        roots += (rd_u128)((rd_u64)(bits & 0xfffffffffffffll) | (1ull << 52)) << (int)((bits >> 52) - 1023);
    });
    st.barrier();
    rd_geom r;
    r.n = amt_wave_sum(n);
    r.dmax2 = amt_wave_max(dmax2);
    r.sy = amt_wave_sum(sy);
    r.sx = amt_wave_sum(sx);
    // four 32-bit limbs of a lane's sum: each wave sum stays below 2^38
    rd_u128 total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) total += (rd_u128)amt_wave_sum((rd_u64)(unsigned)(roots >> (32 * i))) << (32 * i);
    r.root_sum = rd_round_u128(total) * __longlong_as_double((long long)(1023 - 52) << 52);
    return r;
}

// ring and wedge of every pixel, and the pixel counts per (ring, wedge); nbw is clear on entry
template <typename S>
__device__ __forceinline__ void rd_codes(const amt_box& box, int lc, int lane, const S& st, const rd_geom& gm, int B,
                                         unsigned* nbw) {
    const int x1 = box.x1, y1 = box.y1;
    const long long n = gm.n, BB = (long long)B * B, dmax2 = gm.dmax2;
    amt_box_for_cells(box, lc, lane, [&](int x, int y) {
        if (x > x1 || y > y1) return;
        const long long d2 = st.get_d2(y, x);
        if (d2 == 0) {
            st.set_code(y, x, false, 0u);
            return;
        }
        int b = B - 1;  // the largest k with d2 B^2 <= dmax2 (B - k)^2; k = 0 always holds
        while (b > 0 && d2 * BB > dmax2 * (B - b) * (B - b)) --b;
        const long long ey = n * y - gm.sy, ex = n * x - gm.sx;
        const long long ay = ey < 0 ? -ey : ey, ax = ex < 0 ? -ex : ex;
        const unsigned code = (unsigned)b * RD_NW + (unsigned)(ey > 0) + 2u * (unsigned)(ex > 0) + 4u * (unsigned)(ay > ax);
        st.set_code(y, x, true, code);
        atomicAdd(&nbw[code], 1u);
    });
    st.barrier();
}

// AMT_U16: the sums per (ring, wedge) of one channel into sbw (clear on entry), exact
template <typename S>
__device__ __forceinline__ void rd_channel(const uint16_t* __restrict__ I, int W, const amt_box& box, int lc, int lane,
                                           const S& st, int B, rd_counters& cn) {
    const int x1 = box.x1, y1 = box.y1;
    amt_box_for_loaded_cells(
        box, lc, lane, [&](int yc, int xc) { return I[(size_t)yc * W + xc]; },
        [&](int x, int y, uint16_t v) {
            if (x > x1 || y > y1) return;
            const unsigned code = st.get_code(y, x);
            if (code >= (unsigned)(RD_MAXB * RD_NW)) return;  // RD_OUTSIDE
            atomicAdd(&cn.sbw[code], (rd_u64)v);
        });
    __syncthreads();
}

// AMT_F64: one sweep per occupied ring, eight wedge sums per lane, reduced in one fixed order
template <typename S>
__device__ __forceinline__ void rd_channel(const double* __restrict__ I, int W, const amt_box& box, int lc, int lane,
                                           const S& st, int B, rd_counters& cn) {
    const int x1 = box.x1, y1 = box.y1;
    for (int b = 0; b < B; ++b) {
        unsigned nb = 0;
        for (int w = 0; w < RD_NW; ++w) nb += cn.nbw[b * RD_NW + w];
        if (nb == 0u) continue;  // the same for every lane
        double acc[RD_NW];
#pragma unroll
        for (int w = 0; w < RD_NW; ++w) acc[w] = 0.0;
        amt_box_for_loaded_cells(
            box, lc, lane, [&](int yc, int xc) { return I[(size_t)yc * W + xc]; },
            [&](int x, int y, double v) {
                if (x > x1 || y > y1) return;
                const unsigned code = st.get_code(y, x);
                if (code >= (unsigned)(RD_MAXB * RD_NW) || (int)(code >> 3) != b) return;  // RD_OUTSIDE, or another ring
                const unsigned wedge = code & 7u;
#pragma unroll
                for (int w = 0; w < RD_NW; ++w) acc[w] += wedge == (unsigned)w ? v : 0.0;
            });
        const double mine = amt_wave_reduce_scatter<RD_NW, amt_op_sum>(acc, lane);  // wedge w in the lanes 8 w .. 8 w + 7
        if ((lane & 7) == 0) cn.sbw[b * RD_NW + (lane >> 3)] = (rd_u64)__double_as_longlong(mine);
    }
    __syncthreads();
}

// S_bw as a float64: the exact integer converted once, or the float64 sum as it is
template <typename T>
__device__ __forceinline__ double rd_sum_value(rd_u64 s) {
    if constexpr (std::is_same<T, double>::value) return __longlong_as_double((long long)s);
    else return (double)s;
}

// the three columns of ring `b` of one channel, in the order the header states
template <typename T>
__device__ __forceinline__ void rd_ring_columns(const rd_counters& cn, int B, int b, unsigned n, double* __restrict__ out) {
    const double nan = amt_quiet_nan();
    double Sb = 0.0, S = 0.0;
    unsigned nb = 0;
    if constexpr (std::is_same<T, double>::value) {
        for (int k = 0; k < B; ++k) {
            double Sk = 0.0;
            for (int w = 0; w < RD_NW; ++w) Sk += rd_sum_value<T>(cn.sbw[k * RD_NW + w]);
            S += Sk;
            if (k == b) Sb = Sk;
        }
    } else {
        rd_u64 ib = 0, is = 0;
        for (int k = 0; k < B; ++k)
            for (int w = 0; w < RD_NW; ++w) {
                is += cn.sbw[k * RD_NW + w];
                if (k == b) ib += cn.sbw[k * RD_NW + w];
            }
        Sb = (double)ib;
        S = (double)is;
    }
    for (int w = 0; w < RD_NW; ++w) nb += cn.nbw[b * RD_NW + w];
    const double frac = S == 0.0 ? nan : Sb / S;
    out[AMT_RAD_FRAC_AT_D] = frac;
    out[AMT_RAD_MEAN_FRAC] = (nb == 0u || S == 0.0) ? nan : frac / ((double)nb / (double)n);
    double sum = 0.0, var = 0.0;
    int cnt = 0;
    for (int w = 0; w < RD_NW; ++w) {
        const unsigned c = cn.nbw[b * RD_NW + w];
        if (c) {
            sum += rd_sum_value<T>(cn.sbw[b * RD_NW + w]) / (double)c;
            ++cnt;
        }
    }
    if (cnt == 0) {
        out[AMT_RAD_RADIAL_CV] = nan;
        return;
    }
    const double mu = sum / (double)cnt;
    for (int w = 0; w < RD_NW; ++w) {
        const unsigned c = cn.nbw[b * RD_NW + w];
        if (c) {
            const double d = rd_sum_value<T>(cn.sbw[b * RD_NW + w]) / (double)c - mu;
            var += d * d;
        }
    }
    var = var / (double)cnt;
    out[AMT_RAD_RADIAL_CV] = mu == 0.0 ? nan : sqrt(var) / mu;
}

// everything after the tier is chosen
template <typename T, typename S>
__device__ __forceinline__ void rd_measure(const S& st, const T* __restrict__ inten, int C, size_t plane_px, int W,
                                           const amt_box& box, int lc, int lane, int B, rd_counters& cn,
                                           double* __restrict__ geom, double* __restrict__ out) {
    rd_columns(box, lane, st);
    const rd_geom gm = rd_distances(box, lc, lane, st);
    for (int i = lane; i < RD_MAXB * RD_NW; i += 64) cn.nbw[i] = 0u;
    __syncthreads();
    rd_codes(box, lc, lane, st, gm, B, cn.nbw);
    if (lane == 0) {
        geom[AMT_RAD_GEOM_MAXIMUM_RADIUS] = sqrt((double)gm.dmax2);
        geom[AMT_RAD_GEOM_MEAN_RADIUS] = gm.root_sum / (double)gm.n;
    }
    if (lane < RD_MAXB) {
        unsigned nb = 0;
        if (lane < B)
            for (int w = 0; w < RD_NW; ++w) nb += cn.nbw[lane * RD_NW + w];
        geom[AMT_RAD_GEOM_RING_COUNT0 + lane] = (double)nb;
    }
    for (int c = 0; c < C; ++c) {
        for (int i = lane; i < RD_MAXB * RD_NW; i += 64) cn.sbw[i] = 0ull;  // +0.0 as float64 bits too
        __syncthreads();
        rd_channel(inten + (size_t)c * plane_px, W, box, lc, lane, st, B, cn);
        if (lane < B) rd_ring_columns<T>(cn, B, lane, gm.n, out + ((size_t)c * B + lane) * AMT_RAD_NCOLS);
        __syncthreads();  // the sums are read: the next channel may clear them
    }
}

template <typename T>
__global__ void __launch_bounds__(64) radial_kernel(const int* __restrict__ labels, const int* __restrict__ bbox,
                                                    const T* __restrict__ inten, int C, int B,
                                                    double* __restrict__ gtable, double* __restrict__ table,
                                                    unsigned short* __restrict__ gplane, unsigned* __restrict__ dplane,
                                                    int H, int W, int max_label) {
    __shared__ unsigned short tile[RD_LDS_TILE];
    __shared__ rd_counters cn;
    const int plane = blockIdx.y, l = blockIdx.x, lane = threadIdx.x;
    const size_t li = (size_t)plane * max_label + l;
    double* geom = gtable + li * AMT_RAD_GEOM_NCOLS;
    double* out = C ? table + li * (size_t)C * B * AMT_RAD_NCOLS : nullptr;
    const amt_box box = amt_load_box(bbox, li);
    if (box.absent()) {
        if (lane < AMT_RAD_GEOM_NCOLS) geom[lane] = lane < AMT_RAD_GEOM_RING_COUNT0 ? amt_quiet_nan() : 0.0;
        if (out) amt_fill_row(out, C * B * AMT_RAD_NCOLS, amt_quiet_nan(), lane);
        return;
    }
    const size_t n = (size_t)H * W;
    const int* Lp = labels + (size_t)plane * n;
    const T* I = inten ? inten + (size_t)plane * C * n : nullptr;
    const int want = l + 1, lc = amt_box_layout(box.x0, box.x1);
    if ((long long)box.w() * box.h() <= RD_LDS_TILE) {
        const rd_lds st{tile, box.y0, box.x0, box.w()};
        rd_fill_members(Lp, W, box, want, lc, lane, st);
        __syncthreads();
        rd_measure<T>(st, I, C, n, W, box, lc, lane, B, cn, geom, out);
    } else {
        const rd_mem st{Lp, gplane + (size_t)plane * n, dplane + (size_t)plane * n, W, want};
        rd_measure<T>(st, I, C, n, W, box, lc, lane, B, cn, geom, out);
    }
}

template <typename T>
int rd_launch(amt_ctx* ctx, const int* labels, const int* bbox, const void* intensity, int C, int B, double* gtable,
              double* table, unsigned short* gplane, unsigned* dplane, int nplanes, int H, int W, int max_label) {
    hipLaunchKernelGGL(radial_kernel<T>, dim3(max_label, nplanes), dim3(64), 0, ctx->stream, labels, bbox,
                       (const T*)intensity, C, B, gtable, table, gplane, dplane, H, W, max_label);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // namespace

// AMT_RPX_RADIAL of amt_regionprops_ext, which has taken `columns` apart: geom = its table_dev, out = its wtable_dev.
int amt_i_radial(amt_ctx* ctx, const int32_t* labels, const void* intensity, int in_code, int C, int bins, double* geom,
                 double* out, int nplanes, int H, int W, int max_label) {
    AMT_REQUIRE(labels && geom && nplanes >= 0 && H > 0 && W > 0 && max_label >= 0 && C >= 0,
                "regionprops_ext: AMT_RPX_RADIAL takes labels and the geometry rows in table_dev");
    AMT_REQUIRE(bins >= 1 && bins <= RD_MAXB, "regionprops_ext: radial bins %d out of range 1..%d", bins, RD_MAXB);
    AMT_REQUIRE((C >= 1) == !!intensity && (C >= 1) == !!out,
                "regionprops_ext: AMT_RPX_RADIAL takes intensity planes (C >= 1) and wtable_dev together, or C == 0 and "
                "neither");
    AMT_REQUIRE(C == 0 || in_code == AMT_U16 || in_code == AMT_F64, "regionprops_ext: intensity must be AMT_U16 or AMT_F64");
    // the saturation of g in the scratch tier, and 32-bit pixel counts
    AMT_REQUIRE((size_t)H * W <= 0x7fffffffull, "regionprops_ext: radial on planes of more than 2^31 - 1 pixels is not supported");
    AMT_CHECK_OPERANDS("amt_regionprops_ext", amt_in("labels", labels, amt_span(4, nplanes, H, W)),
                       amt_in("intensity", intensity, amt_span(amt_esize(in_code), nplanes, C, H, W)),
                       amt_out("table_dev", geom, amt_span(8, nplanes, max_label, AMT_RAD_GEOM_NCOLS)),
                       amt_out("wtable_dev", out, amt_span(8, nplanes, max_label, (long long)C * bins, AMT_RAD_NCOLS)));
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0 || max_label == 0) return AMT_OK;
    // the two planes of the scratch tier are always reserved: which boxes need them is known on the device only
    const size_t px = (size_t)nplanes * H * W;
    amt_scratch s(ctx);
    amt_buf<int> bbox(s, (size_t)nplanes * max_label * 4);
    amt_buf<unsigned short> gplane(s, px);
    amt_buf<unsigned> dplane(s, px);
    AMT_TRY(s.commit());
    AMT_TRY(amt_i_label_boxes(ctx, labels, bbox, nullptr, nplanes, H, W, max_label));
    if (C >= 1 && in_code == AMT_F64)
        return rd_launch<double>(ctx, labels, bbox, intensity, C, bins, geom, out, gplane, dplane, nplanes, H, W, max_label);
    return rd_launch<uint16_t>(ctx, labels, bbox, intensity, C, bins, geom, out, gplane, dplane, nplanes, H, W, max_label);
}
