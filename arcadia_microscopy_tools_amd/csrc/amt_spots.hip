// Spot detection: ops AMT_RANK_LOCAL_MAXIMA .. AMT_RANK_TAKE_AT of amt_rank_filter (include/amt_hip.h states the rules).
// All four are asynchronous, use no float atomics and give identical bytes on every run.
//
// Local maxima (op 15): a workgroup owns one AMT_SPOT_TILE_H x AMT_SPOT_TILE_W output tile and stages it with a halo of
// r in LDS; a position outside the image is staged as "less than everything" (-1 under uint16 values held as int, -inf
// under float64).  The window maximum is separable: per staged row the maximum of the r pixels to the left, of the r
// pixels to the right and of the whole row window (R); per column the maximum of R over the r rows above and the r rows
// below.  A pixel is marked iff v > above, v > left, v >= right, v >= below, v > t and it lies inside the border: the
// strict comparisons are the ones towards pixels that precede it in raster order.  2 r + 2 r LDS reads per pixel, not
// (2 r + 1)^2, and no branch depends on the data.
//
// Mask list (op 16): per-row counts (a wave per row, ballots and popcounts: integer adds only), one exclusive scan per
// plane, then a wave per row again that places the raster indices of its set pixels behind its row's offset.  The order
// of the list is the raster order, whatever the schedule.
//
// Spot measure / take at (ops 17 / 18): a wave / a lane per list entry.
#include "amt_internal.h"

namespace {

constexpr int SP_H = AMT_SPOT_TILE_H, SP_W = AMT_SPOT_TILE_W;
constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_OWN = SP_H / SP_WAVES;  // rows of a column one thread decides: wave q owns rows q * SP_OWN ...
static_assert(SP_W == 64 && SP_H % SP_WAVES == 0, "a wave's lanes are the tile's columns");

// the type a value is staged as, and what stands for a position outside the image
template <typename T> struct lm_key;
template <> struct lm_key<uint16_t> {
    typedef int type;
    static __device__ __forceinline__ int lowest() { return -1; }
};
template <> struct lm_key<double> {
    typedef double type;
    static __device__ __forceinline__ double lowest() { return -__builtin_huge_val(); }
};
template <typename K> __device__ __forceinline__ K lm_max(K a, K b) { return a > b ? a : b; }

static size_t lm_lds_bytes(size_t ksize, int r) {
    const size_t sh = SP_H + 2 * r, sw = SP_W + 2 * r;
    return sh * sw * ksize + sh * SP_W * ksize + (size_t)SP_H * SP_W;  // staged tile, row maxima, row flags
}

// RC: the radius when it is known at compile time (the loops unroll), 0 = `r_arg`
template <typename T, int RC>
__global__ void __launch_bounds__(SP_THREADS) lmax_kernel(const T* __restrict__ in, uint8_t* __restrict__ out,
                                                          const double* __restrict__ thr, double cval, int nplanes, int H,
                                                          int W, int r_arg, int b, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lm_lds[];
    typedef typename lm_key<T>::type K;
    const int r = RC ? RC : r_arg;
    const int sh = SP_H + 2 * r, sw = SP_W + 2 * r;
    K* S = reinterpret_cast<K*>(lm_lds);       // sh x sw: the tile plus halo
    K* R = S + sh * sw;                        // sh x SP_W: the maximum of the row window 2 r + 1 wide
    uint8_t* F = reinterpret_cast<uint8_t*>(R + sh * SP_W);  // SP_H x SP_W: v > left and v >= right
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)(blockIdx.x % tiles_x) * SP_W, y0 = (int)(blockIdx.x / tiles_x) * SP_H;
    const size_t HW = (size_t)H * W;
    const K low = lm_key<T>::lowest();
    for (int s = blockIdx.y; s < nplanes; s += gridDim.y) {
        const T* P = in + (size_t)s * HW;
        for (int e = tid; e < sh * sw; e += SP_THREADS) {
            const int sy = e / sw, sx = e - sy * sw;
            const int gy = y0 - r + sy, gx = x0 - r + sx;
            S[e] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? (K)P[(size_t)gy * W + gx] : low;
        }
        __syncthreads();
        for (int e = tid; e < sh * SP_W; e += SP_THREADS) {
            const int row = e >> 6, x = e & 63;
            const K* c = S + row * sw + x + r;
            K left = low, right = low;
            for (int j = 1; j <= r; ++j) {  // RC != 0: a constant trip count, unrolled
                left = lm_max(left, c[-j]);
                right = lm_max(right, c[j]);
            }
            const K v = c[0];
            R[e] = lm_max(lm_max(left, v), right);
            if (row >= r && row < r + SP_H) F[(row - r) * SP_W + x] = (uint8_t)((v > left) & (v >= right));
        }
        __syncthreads();
        const double t = thr ? thr[s] : cval;
        const int gx = x0 + lane;
        const bool xin = gx >= b && gx < W - b;
        for (int i = 0; i < SP_OWN; ++i) {
            const int y = wave * SP_OWN + i, gy = y0 + y;
            const K* c = R + (y + r) * SP_W + lane;
            K above = low, below = low;
            for (int j = 1; j <= r; ++j) {  // RC != 0: a constant trip count, unrolled
                above = lm_max(above, c[-j * SP_W]);
                below = lm_max(below, c[j * SP_W]);
            }
            const K v = S[(y + r) * sw + lane + r];
            const bool mark = F[y * SP_W + lane] && v > above && v >= below && (double)v > t && xin && gy >= b && gy < H - b;
            if (gy < H && gx < W) out[(size_t)s * HW + (size_t)gy * W + gx] = mark ? 1 : 0;
        }
        __syncthreads();  // the next plane stages into the same LDS
    }
}

template <typename T, int RC>
int lmax_launch(amt_ctx* ctx, const void* in, void* out, const void* thr, double cval, int nplanes, int H, int W, int r, int b) {
    typedef typename lm_key<T>::type K;
    // float64 tiles pass the 64 KiB a launch gets without asking (121 KiB at r = 15); always the largest size of the
    // instance, so that calls from several host threads cannot undercut one another
    AMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&lmax_kernel<T, RC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lm_lds_bytes(sizeof(K), RC ? RC : AMT_SPOT_MAX_RADIUS)));
    const int tiles_x = (W + SP_W - 1) / SP_W, tiles_y = (H + SP_H - 1) / SP_H;
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, nplanes < 65535 ? nplanes : 65535);
    hipLaunchKernelGGL((lmax_kernel<T, RC>), grid, dim3(SP_THREADS), lm_lds_bytes(sizeof(K), r), ctx->stream, (const T*)in,
                       (uint8_t*)out, (const double*)thr, cval, nplanes, H, W, r, b, tiles_x);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

template <typename T>
int lmax_go(amt_ctx* ctx, const void* in, void* out, const void* thr, double cval, int nplanes, int H, int W, int r, int b) {
    if (r == 1) return lmax_launch<T, 1>(ctx, in, out, thr, cval, nplanes, H, W, r, b);
    if (r == 2) return lmax_launch<T, 2>(ctx, in, out, thr, cval, nplanes, H, W, r, b);
    return lmax_launch<T, 0>(ctx, in, out, thr, cval, nplanes, H, W, r, b);
}

// ---- mask list: a wave per image row, SP_WAVES rows per workgroup ------------------------------------------------------
// PLACE = false: counts[plane * H + y] = set pixels of row y.  PLACE = true: counts holds the exclusive scan of that, and
// the row's set pixels go to list[1 + offset ...] as raster indices, as far as `capacity` reaches.
template <bool PLACE>
__global__ void __launch_bounds__(SP_THREADS) mlist_rows_kernel(const uint8_t* __restrict__ in, int* __restrict__ counts,
                                                                int* __restrict__ list, int nplanes, int H, int W, int capacity) {
    const int lane = threadIdx.x & 63;
    const int y = (int)(blockIdx.x * SP_WAVES + (threadIdx.x >> 6));
    if (y >= H) return;  // the whole wave
    const size_t HW = (size_t)H * W;
    for (int s = blockIdx.y; s < nplanes; s += gridDim.y) {
        const uint8_t* row = in + (size_t)s * HW + (size_t)y * W;
        int* dst = PLACE ? list + (size_t)s * ((size_t)capacity + 1) + 1 : nullptr;
        int n = PLACE ? counts[(size_t)s * H + y] : 0;
        for (int xb = 0; xb < W; xb += 64) {  // wave-uniform trip count: every lane votes
            const int x = xb + lane;
            const bool set = x < W && row[x] != 0;
            const unsigned long long votes = __ballot(set);
            if (PLACE) {
                const int pos = n + __popcll(votes & ((1ull << lane) - 1ull));
                if (set && pos < capacity) dst[pos] = y * W + x;
            }
            n += __popcll(votes);
        }
        if (!PLACE && lane == 0) counts[(size_t)s * H + y] = n;
    }
}

// list[plane][0] = the true count; the entries past min(count, capacity) = -1
__global__ void __launch_bounds__(256) mlist_finish_kernel(const int* __restrict__ totals, int* __restrict__ list, int nplanes,
                                                           int capacity) {
    const size_t pitch = (size_t)capacity + 1;
    for (int s = blockIdx.y; s < nplanes; s += gridDim.y) {
        const int total = totals[s];
        const size_t kept = (size_t)(total < capacity ? total : capacity);
        int* row = list + (size_t)s * pitch;
        for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < pitch; j += (size_t)gridDim.x * 256) {
            if (j == 0) row[0] = total;
            else if (j > kept) row[j] = -1;
        }
    }
}

int mlist_go(amt_ctx* ctx, const void* in, void* out, int nplanes, int H, int W, int capacity) {
    amt_scratch s(ctx);
    amt_buf<int> counts(s, (size_t)nplanes * H);
    amt_buf<int> totals(s, (size_t)nplanes);
    AMT_TRY(s.commit());
    const dim3 grid((unsigned)((H + SP_WAVES - 1) / SP_WAVES), nplanes < 65535 ? nplanes : 65535);
    hipLaunchKernelGGL((mlist_rows_kernel<false>), grid, dim3(SP_THREADS), 0, ctx->stream, (const uint8_t*)in, (int*)counts,
                       (int*)nullptr, nplanes, H, W, capacity);
    AMT_LAUNCH_CHECK();
    AMT_TRY(amt_scan_excl(ctx, counts, H, (size_t)H, totals, nplanes));
    hipLaunchKernelGGL((mlist_rows_kernel<true>), grid, dim3(SP_THREADS), 0, ctx->stream, (const uint8_t*)in, (int*)counts,
                       (int*)out, nplanes, H, W, capacity);
    AMT_LAUNCH_CHECK();
    const dim3 gfin(amt_grid_for((size_t)capacity + 1, 256, 4096), nplanes < 65535 ? nplanes : 65535);
    hipLaunchKernelGGL(mlist_finish_kernel, gfin, dim3(256), 0, ctx->stream, (const int*)totals, (int*)out, nplanes, capacity);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- a list entry: its raster index, or -1 past min(count, capacity), for a -1 entry and for an index outside the plane
__device__ __forceinline__ int spot_at(const int* __restrict__ list, int j, int capacity, size_t HW) {
    const int count = list[0];
    const int kept = count < capacity ? count : capacity;
    if (j >= kept) return -1;
    const int p = list[1 + j];
    return (p >= 0 && (size_t)p < HW) ? p : -1;
}

template <typename A> __device__ __forceinline__ A spot_wave_sum(A v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);  // a + b = b + a: every lane ends with the same bits
    return v;
}
template <typename T> struct sm_acc { typedef unsigned long long type; };  // 1225 values of 65535: exact
template <> struct sm_acc<double> { typedef double type; };

// a wave per list entry.  The window (2 k + 5)^2 is walked once: lane l takes its elements l, l + 64, ... in that order
// (row by row), the ones within k go to the spot's sum, the frame k + 1 .. k + 2 to the ring's; then one butterfly.
template <typename T>
__global__ void __launch_bounds__(SP_THREADS) smeasure_kernel(const T* __restrict__ in, const int* __restrict__ lists,
                                                              double* __restrict__ out, int nplanes, int H, int W, int k,
                                                              int capacity) {
    typedef typename sm_acc<T>::type A;
    const int lane = threadIdx.x & 63;
    const size_t j = (size_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (j >= (size_t)capacity) return;  // the whole wave
    const size_t HW = (size_t)H * W;
    const double nan = __builtin_nan("");
    for (int s = blockIdx.y; s < nplanes; s += gridDim.y) {
        const T* P = in + (size_t)s * HW;
        double* row = out + ((size_t)s * capacity + j) * AMT_SPOT_NCOLS;
        const int p = spot_at(lists + (size_t)s * ((size_t)capacity + 1), (int)j, capacity, HW);
        if (p < 0) {  // wave-uniform
            if (lane < AMT_SPOT_NCOLS) row[lane] = nan;
            continue;
        }
        const int y = p / W, x = p - y * W;
        const int side = 2 * k + 5, reach = k + 2;
        A sum = 0, ring = 0;
        int n = 0, nring = 0;
        for (int e = lane; e < side * side; e += 64) {
            const int ey = e / side;
            const int dy = ey - reach, dx = e - ey * side - reach;
            const int gy = y + dy, gx = x + dx;
            if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
            const A v = (A)P[(size_t)gy * W + gx];
            if (dy >= -k && dy <= k && dx >= -k && dx <= k) {
                sum += v;
                ++n;
            } else {
                ring += v;
                ++nring;
            }
        }
        sum = spot_wave_sum(sum);
        ring = spot_wave_sum(ring);
        n = spot_wave_sum(n);
        nring = spot_wave_sum(nring);
        if (lane == 0) {
            const double a0 = (double)P[p];
            double off[2];
#pragma unroll
            for (int axis = 0; axis < 2; ++axis) {
                const int at = axis ? x : y, last = axis ? W - 1 : H - 1;
                const size_t step = axis ? (size_t)1 : (size_t)W;
                double o = 0.0;
                if (at > 0 && at < last) {
                    const double am = (double)P[p - step], ap = (double)P[p + step];
                    const double den = (am - a0) + (ap - a0);
                    if (!(den >= 0.0)) {
                        o = (0.5 * (am - ap)) / den;
                        o = o < -0.5 ? -0.5 : (o > 0.5 ? 0.5 : o);
                    }
                }
                off[axis] = o;
            }
            row[AMT_SPOT_VALUE] = a0;
            row[AMT_SPOT_DY] = off[0];
            row[AMT_SPOT_DX] = off[1];
            row[AMT_SPOT_SUM] = (double)sum;
            row[AMT_SPOT_N] = (double)n;
            row[AMT_SPOT_RING_SUM] = (double)ring;
            row[AMT_SPOT_RING_N] = (double)nring;
        }
    }
}

template <typename T>
int smeasure_go(amt_ctx* ctx, const void* in, const void* lists, void* out, int nplanes, int H, int W, int k, int capacity) {
    const dim3 grid((unsigned)(((size_t)capacity + SP_WAVES - 1) / SP_WAVES), nplanes < 65535 ? nplanes : 65535);
    hipLaunchKernelGGL(smeasure_kernel<T>, grid, dim3(SP_THREADS), 0, ctx->stream, (const T*)in, (const int*)lists, (double*)out,
                       nplanes, H, W, k, capacity);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// a lane per list entry
template <typename T>
__global__ void __launch_bounds__(256) takeat_kernel(const T* __restrict__ in, const int* __restrict__ lists, T* __restrict__ out,
                                                     int nplanes, size_t HW, int capacity) {
    for (int s = blockIdx.y; s < nplanes; s += gridDim.y) {
        const T* P = in + (size_t)s * HW;
        const int* list = lists + (size_t)s * ((size_t)capacity + 1);
        T* row = out + (size_t)s * capacity;
        for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < (size_t)capacity; j += (size_t)gridDim.x * 256) {
            const int p = spot_at(list, (int)j, capacity, HW);
            row[j] = p >= 0 ? P[p] : (T)0;
        }
    }
}

template <typename T>
int takeat_go(amt_ctx* ctx, const void* in, const void* lists, void* out, int nplanes, size_t HW, int capacity) {
    const dim3 grid(amt_grid_for((size_t)capacity, 256, 4096), nplanes < 65535 ? nplanes : 65535);
    hipLaunchKernelGGL(takeat_kernel<T>, grid, dim3(256), 0, ctx->stream, (const T*)in, (const int*)lists, (T*)out, nplanes, HW,
                       capacity);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // namespace

// Byte lengths of the operands of ops 15 .. 18, for amt_rank_filter's aliasing check (0 = absent or not yet refusable)
void amt_i_spots_spans(int op, int dtype, int nplanes, int H, int W, int mode, size_t* in_bytes, size_t* out_bytes,
                       size_t* minuend_bytes) {
    const size_t e = amt_esize(dtype);
    const long long list = mode >= 1 ? (long long)mode + 1 : 0;  // a list of capacity `mode`
    *in_bytes = amt_span(e, nplanes, H, W);
    switch (op) {
        case AMT_RANK_LOCAL_MAXIMA:
            *out_bytes = amt_span(1, nplanes, H, W);
            *minuend_bytes = amt_span(8, nplanes);  // the per-plane thresholds
            break;
        case AMT_RANK_MASK_LIST:
            *out_bytes = amt_span(4, nplanes, list);
            *minuend_bytes = 0;
            break;
        case AMT_RANK_SPOT_MEASURE:
            *out_bytes = amt_span(8, nplanes, mode, AMT_SPOT_NCOLS);
            *minuend_bytes = amt_span(4, nplanes, list);
            break;
        default:
            *out_bytes = amt_span(e, nplanes, mode);
            *minuend_bytes = amt_span(4, nplanes, list);
            break;
    }
}

// (2 r + 1) x (2 r + 1), every cell non-zero, lo <= r <= hi: r, else -1
static int spots_square_radius(const uint8_t* footprint, int fh, int fw, int lo, int hi) {
    if (!footprint || fh != fw || !(fh & 1) || fh < 2 * lo + 1 || fh > 2 * hi + 1) return -1;
    for (int i = 0; i < fh * fw; ++i)
        if (!footprint[i]) return -1;
    return fh / 2;
}

// Ops 15 .. 18 of amt_rank_filter, which has checked the operands' aliasing.  The refusals that need no device come before
// the context is looked at.
int amt_i_spots(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W, const uint8_t* footprint, int fh,
                int fw, int op, int mode, double cval, const void* minuend) {
    const char* what = op == AMT_RANK_LOCAL_MAXIMA   ? "local_maxima"
                       : op == AMT_RANK_MASK_LIST    ? "mask_list"
                       : op == AMT_RANK_SPOT_MEASURE ? "spot_measure"
                                                     : "take_at";
    AMT_REQUIRE(in && out && nplanes >= 0 && H > 0 && W > 0, "amt_rank_filter: %s: bad arguments", what);
    int r = 0;
    switch (op) {
        case AMT_RANK_LOCAL_MAXIMA:
            AMT_REQUIRE(dtype == AMT_U16 || dtype == AMT_F64, "amt_rank_filter: local_maxima: dtype must be AMT_U16 or AMT_F64, got %d",
                        dtype);
            r = spots_square_radius(footprint, fh, fw, 1, AMT_SPOT_MAX_RADIUS);
            AMT_REQUIRE(r >= 1, "amt_rank_filter: local_maxima: the footprint must be (2 r + 1) x (2 r + 1) all non-zero with r in 1..%d",
                        AMT_SPOT_MAX_RADIUS);
            AMT_REQUIRE(mode >= 0, "amt_rank_filter: local_maxima: the border width (mode) must not be negative, got %d", mode);
            break;
        case AMT_RANK_MASK_LIST:
            AMT_REQUIRE(dtype == AMT_U8, "amt_rank_filter: mask_list: dtype must be AMT_U8, got %d", dtype);
            break;
        case AMT_RANK_SPOT_MEASURE:
            AMT_REQUIRE(dtype == AMT_U16 || dtype == AMT_F64, "amt_rank_filter: spot_measure: dtype must be AMT_U16 or AMT_F64, got %d",
                        dtype);
            r = spots_square_radius(footprint, fh, fw, 0, AMT_SPOT_MAX_RADIUS);
            AMT_REQUIRE(r >= 0, "amt_rank_filter: spot_measure: the footprint must be (2 k + 1) x (2 k + 1) all non-zero with k in 0..%d",
                        AMT_SPOT_MAX_RADIUS);
            break;
        default:
            AMT_REQUIRE(dtype == AMT_U8 || dtype == AMT_U16 || dtype == AMT_I32 || dtype == AMT_F64,
                        "amt_rank_filter: take_at: dtype must be AMT_U8, AMT_U16, AMT_I32 or AMT_F64, got %d", dtype);
            break;
    }
    if (op != AMT_RANK_LOCAL_MAXIMA) {
        AMT_REQUIRE(mode >= 1, "amt_rank_filter: %s: capacity (mode) must be at least 1, got %d", what, mode);
        if (op == AMT_RANK_MASK_LIST)
            AMT_REQUIRE(minuend == nullptr, "amt_rank_filter: mask_list takes no minuend");
        else
            AMT_REQUIRE(minuend != nullptr, "amt_rank_filter: %s: minuend (the list of spots) is required", what);
    }
    AMT_REQUIRE((size_t)H * W < 0x80000000ull, "amt_rank_filter: %s: plane too large (H * W must be below 2^31)", what);
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0) return AMT_OK;
    const size_t HW = (size_t)H * W;
    switch (op) {
        case AMT_RANK_LOCAL_MAXIMA:
            return dtype == AMT_U16 ? lmax_go<uint16_t>(ctx, in, out, minuend, cval, nplanes, H, W, r, mode)
                                    : lmax_go<double>(ctx, in, out, minuend, cval, nplanes, H, W, r, mode);
        case AMT_RANK_MASK_LIST: return mlist_go(ctx, in, out, nplanes, H, W, mode);
        case AMT_RANK_SPOT_MEASURE:
            return dtype == AMT_U16 ? smeasure_go<uint16_t>(ctx, in, minuend, out, nplanes, H, W, r, mode)
                                    : smeasure_go<double>(ctx, in, minuend, out, nplanes, H, W, r, mode);
        default:
            if (dtype == AMT_U8) return takeat_go<uint8_t>(ctx, in, minuend, out, nplanes, HW, mode);
            if (dtype == AMT_U16) return takeat_go<uint16_t>(ctx, in, minuend, out, nplanes, HW, mode);
            if (dtype == AMT_I32) return takeat_go<int32_t>(ctx, in, minuend, out, nplanes, HW, mode);
            return takeat_go<double>(ctx, in, minuend, out, nplanes, HW, mode);
    }
}
