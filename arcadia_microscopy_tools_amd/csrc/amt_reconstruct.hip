// Grey reconstruction (skimage.morphology.reconstruction) and the h-maxima / h-minima reconstructions built on it: ops
// AMT_RANK_RECONSTRUCT_DILATION .. AMT_RANK_HMIN_RECONSTRUCT of amt_rank_filter (include/amt_hip.h states the
// definitions).  By dilation, R is the least image with R >= seed and R = min(mask, max over the footprint of R); by
// erosion the dual.  Nothing propagates from outside the image.
//
// The state lives in `out`.  A 256-thread workgroup owns one tile of RC_TH x RC_TW pixels: it loads the tile and a
// one-pixel halo of state and mask into LDS, brings the tile to its LOCAL fixed point there (the halo stays as loaded),
// and stores its interior only if something changed; it then bumps the round's counter.  Inside LDS every phase gives each
// cell one owner and reads no cell that another thread writes in the same phase:
//   rows      lane r walks row r left to right and back, carrying the running value in a register;
//   columns   lane c walks column c down and up;
//   diagonals (all-ones footprint) every lane relaxes cells of the even rows against their four diagonal neighbours, which
//             lie in odd rows; then the odd rows against the even ones.
// Before each turn of these phases all lanes test, read-only, whether a neighbour can still raise any cell; the turns
// repeat until none can.  Every change raises (by erosion: lowers) a cell to another value
// of the tile, so the loop ends; comparisons are written so that a NaN changes nothing rather than everything.
//
// Rounds.  Round 0 reads the seed (ops 5 / 6 compute it from the image while loading) for interior and halo alike, clamps
// it under the mask, counts seed-over-mask violations per plane and stores every tile: it reads nothing that it writes,
// one launch.  A later round updates `out` in place in four launches, one per colour (tile-row parity x tile-column
// parity): the eight neighbours of a tile all have another colour, so no load of a cell can race with a store to it, and
// what a neighbour stored is handed over by the kernel boundary alone.  No workgroup waits for another.  The fixed point
// is unique, so the bytes of `out` do not depend on the order in which tiles ran.
// The host enqueues RC_BATCH rounds, reads their counters (one small copy, one synchronise) and stops after a round in
// which no workgroup stored anything; the launches of a round whose predecessor was clean return at once.
#include "amt_internal.h"

#include <cmath>
#include <cstdlib>

// tile interiors (include/amt_hip.h restates them as AMT_RECONSTRUCT_TILE_*); LDS rows are padded so that the lanes of a
// row walk (stride = one LDS row) fall on distinct banks: 130 uint16 = 65 dwords, 67 doubles = 134 dwords
constexpr int RC_BATCH = 8;
template <typename T>
struct rc_tile;
template <>
struct rc_tile<uint16_t> {
    static constexpr int TH = AMT_RECONSTRUCT_TILE_H_U16, TW = AMT_RECONSTRUCT_TILE_W_U16, PITCH = TW + 2;
};
template <>
struct rc_tile<double> {
    static constexpr int TH = AMT_RECONSTRUCT_TILE_H_F64, TW = AMT_RECONSTRUCT_TILE_W_F64, PITCH = TW + 3;
};
static_assert((rc_tile<uint16_t>::PITCH * 2 / 4) % 2 == 1 && rc_tile<uint16_t>::PITCH % 2 == 0, "uint16 rows: odd dwords");
static_assert(rc_tile<double>::PITCH % 2 == 1, "float64 rows: an odd number of 8-byte words");

// DIL: "better" is greater; erosion: smaller.  All three keep the first operand when a NaN is involved.
template <bool DIL, typename T>
__device__ __forceinline__ bool rc_better(T a, T b) {
    return DIL ? a > b : a < b;
}
template <bool DIL, typename T>
__device__ __forceinline__ T rc_up(T v, T n) {  // max (dilation) / min (erosion)
    return rc_better<DIL>(n, v) ? n : v;
}
template <bool DIL, typename T>
__device__ __forceinline__ T rc_cap(T v, T m) {  // hold v under (over) the mask
    return rc_better<DIL>(v, m) ? m : v;
}
template <bool DIL>
__device__ __forceinline__ uint16_t rc_neutral(uint16_t) {
    return DIL ? (uint16_t)0 : (uint16_t)65535;
}
template <bool DIL>
__device__ __forceinline__ double rc_neutral(double) {
    return DIL ? -HUGE_VAL : HUGE_VAL;
}
// seed of ops 5 / 6 from the image value: saturating for uint16, one rounding for float64
template <bool DIL>
__device__ __forceinline__ uint16_t rc_hseed(uint16_t v, uint16_t h) {
    return DIL ? (uint16_t)(v > h ? v - h : 0) : (uint16_t)(65535 - v > h ? v + h : 65535);
}
template <bool DIL>
__device__ __forceinline__ double rc_hseed(double v, double h) {
    return DIL ? v - h : v + h;
}

// hdr: word 0 = ~(first plane with a violation), 0 for none; viol[plane] = violations of the plane
// FIRST: round 0 (every tile, reads `seed`, or the mask with HSEED); else the tiles of colour (cy, cx), in place
template <typename T, bool DIL, bool FIRST>
__global__ void __launch_bounds__(256) rc_round_kernel(const T* __restrict__ seed, const T* __restrict__ mask, T* out, int H,
                                                       int W, int ntx, int nty, int cy, int cx, int c8, int hseed, T h,
                                                       const unsigned* prev, unsigned* changed, unsigned* hdr,
                                                       unsigned* viol) {
    constexpr int TH = rc_tile<T>::TH, TW = rc_tile<T>::TW, PITCH = rc_tile<T>::PITCH;
    constexpr int ROWS = TH + 2, COLS = TW + 2;
    __shared__ T S[ROWS * PITCH];
    __shared__ T M[ROWS * PITCH];
    __shared__ int flag;
    if (!FIRST && prev && *prev == 0u) return;  // the round before this one stored nothing: neither will this one
    const int tid = threadIdx.x;
    // this launch's tiles: sx x sy of them per plane, every second tile from (cy, cx) on (FIRST: all of them)
    const int step = FIRST ? 1 : 2;
    const int sx = (ntx - cx + step - 1) / step, sy = (nty - cy + step - 1) / step;
    unsigned b = blockIdx.x;
    const int tx = cx + step * (int)(b % (unsigned)sx);
    b /= (unsigned)sx;
    const int ty = cy + step * (int)(b % (unsigned)sy);
    const int plane_i = (int)(b / (unsigned)sy);
    const size_t plane = (size_t)plane_i * H * W;
    const int x0 = tx * TW - 1, y0 = ty * TH - 1;  // image coordinates of LDS cell (0, 0)
    const T neutral = rc_neutral<DIL>(T());
    int nviol = 0;
    for (int i = tid; i < ROWS * COLS; i += 256) {
        const int ky = i / COLS, kx = i - ky * COLS;
        const int y = y0 + ky, x = x0 + kx;
        T s = neutral, m = neutral;  // outside the image: nothing comes from there, and nothing changes there
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t p = plane + (size_t)y * W + x;
            m = mask[p];
            if (FIRST) {
                s = hseed ? rc_hseed<DIL>(m, h) : seed[p];
                if (rc_better<DIL>(s, m)) {
                    if (ky >= 1 && ky <= TH && kx >= 1 && kx <= TW) ++nviol;  // counted by the tile that owns the pixel
                    s = m;
                }
            } else {
                s = out[p];
            }
        }
        S[ky * PITCH + kx] = s;
        M[ky * PITCH + kx] = m;
    }
    if (FIRST && nviol) {
        atomicAdd(&viol[plane_i], (unsigned)nviol);
        atomicMax(&hdr[0], ~(unsigned)plane_i);
    }
    bool dirty = FIRST;
    while (true) {
        __syncthreads();  // the loads or the last turn's writes, and the last reads of `flag`
        if (tid == 0) flag = 0;
        __syncthreads();
        // can a neighbour still raise any cell?  Read-only and every lane busy: a tile that is at its fixed point
        // already -- most tiles of most rounds -- ends here, without the serial walks
        bool need = false;
        for (int i = tid; i < TH * TW; i += 256) {
            const int ky = 1 + i / TW, kx = 1 + i % TW;
            const T* c = S + ky * PITCH + kx;
            const T v = *c;
            T nb = rc_up<DIL>(rc_up<DIL>(c[-1], c[1]), rc_up<DIL>(c[-PITCH], c[PITCH]));
            if (c8) {
                nb = rc_up<DIL>(nb, rc_up<DIL>(c[-PITCH - 1], c[-PITCH + 1]));
                nb = rc_up<DIL>(nb, rc_up<DIL>(c[PITCH - 1], c[PITCH + 1]));
            }
            need |= rc_better<DIL>(rc_cap<DIL>(rc_up<DIL>(v, nb), M[ky * PITCH + kx]), v);
        }
        if (need) flag = 1;
        __syncthreads();
        if (!flag) break;  // uniform: every thread reads the same word between two barriers
        dirty = true;
        // one turn: every neighbour relation is applied at least once, so the cell found above is raised
        if (tid < TH) {  // rows
            T* s = S + (tid + 1) * PITCH;
            const T* m = M + (tid + 1) * PITCH;
            T run = s[0];
            for (int x = 1; x <= TW; ++x) {
                const T v = s[x];
                const T n = rc_cap<DIL>(rc_up<DIL>(v, run), m[x]);
                if (rc_better<DIL>(n, v)) {
                    s[x] = n;
                    run = n;
                } else {
                    run = v;
                }
            }
            run = s[TW + 1];
            for (int x = TW; x >= 1; --x) {
                const T v = s[x];
                const T n = rc_cap<DIL>(rc_up<DIL>(v, run), m[x]);
                if (rc_better<DIL>(n, v)) {
                    s[x] = n;
                    run = n;
                } else {
                    run = v;
                }
            }
        }
        __syncthreads();
        if (tid < TW) {  // columns
            T* s = S + tid + 1;
            const T* m = M + tid + 1;
            T run = s[0];
            for (int y = 1; y <= TH; ++y) {
                const T v = s[y * PITCH];
                const T n = rc_cap<DIL>(rc_up<DIL>(v, run), m[y * PITCH]);
                if (rc_better<DIL>(n, v)) {
                    s[y * PITCH] = n;
                    run = n;
                } else {
                    run = v;
                }
            }
            run = s[(TH + 1) * PITCH];
            for (int y = TH; y >= 1; --y) {
                const T v = s[y * PITCH];
                const T n = rc_cap<DIL>(rc_up<DIL>(v, run), m[y * PITCH]);
                if (rc_better<DIL>(n, v)) {
                    s[y * PITCH] = n;
                    run = n;
                } else {
                    run = v;
                }
            }
        }
        if (c8) {  // diagonals: the rows of one parity against the rows of the other
            for (int par = 0; par < 2; ++par) {
                __syncthreads();
                for (int i = tid; i < (TH / 2) * TW; i += 256) {
                    const int ky = 1 + par + 2 * (i / TW), kx = 1 + i % TW;
                    T* c = S + ky * PITCH + kx;
                    const T v = *c;
                    T nb = rc_up<DIL>(c[-PITCH - 1], c[-PITCH + 1]);
                    nb = rc_up<DIL>(nb, rc_up<DIL>(c[PITCH - 1], c[PITCH + 1]));
                    const T n = rc_cap<DIL>(rc_up<DIL>(v, nb), M[ky * PITCH + kx]);
                    if (rc_better<DIL>(n, v)) {
                        *c = n;
                        }
                }
            }
        }
    }
    if (!dirty) return;
    for (int i = tid; i < TH * TW; i += 256) {
        const int ky = 1 + i / TW, kx = 1 + i % TW;
        const int y = y0 + ky, x = x0 + kx;
        if (y < H && x < W) out[plane + (size_t)y * W + x] = S[ky * PITCH + kx];
    }
    if (tid == 0) atomicAdd(changed, 1u);
}

template <typename T, bool DIL>
static int rc_run(amt_ctx* ctx, const T* seed, const T* mask, T* out, int nplanes, int H, int W, int c8, int hseed, T h) {
    constexpr int TH = rc_tile<T>::TH, TW = rc_tile<T>::TW;
    static_assert(TH % 2 == 0, "the diagonal phase splits the tile's rows by parity");
    const int ntx = (W + TW - 1) / TW, nty = (H + TH - 1) / TH;
    AMT_REQUIRE((unsigned long long)ntx * nty * nplanes < 0x7fffffffull, "rank_filter: too many tiles for one launch");
    amt_scratch s(ctx);
    amt_buf<unsigned> hdr(s, 1 + RC_BATCH);  // word 0: first plane with a violation; then one counter per round of a batch
    amt_buf<unsigned> viol(s, (size_t)nplanes);
    AMT_TRY(s.commit());
    unsigned* const cnt = hdr;
    AMT_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned) * (1 + RC_BATCH), ctx->stream));
    AMT_HIP_CHECK(hipMemsetAsync(viol, 0, sizeof(unsigned) * (size_t)nplanes, ctx->stream));
    hipLaunchKernelGGL((rc_round_kernel<T, DIL, true>), dim3((unsigned)(ntx * nty * nplanes)), dim3(256), 0, ctx->stream,
                       seed, mask, out, H, W, ntx, nty, 0, 0, c8, hseed, h, (const unsigned*)nullptr, cnt + 1, cnt,
                       (unsigned*)viol);
    AMT_LAUNCH_CHECK();
    const unsigned long long limit = (unsigned long long)H * W + 1;  // a round that stores raises at least one pixel
    unsigned long long rounds = 0, syncs = 0;
    while (true) {
        AMT_HIP_CHECK(hipMemsetAsync(cnt + 1, 0, sizeof(unsigned) * RC_BATCH, ctx->stream));
        for (int k = 1; k <= RC_BATCH; ++k)
            for (int col = 0; col < 4; ++col) {
                const int cy = col >> 1, cx = col & 1;
                const int sx = (ntx - cx + 1) / 2, sy = (nty - cy + 1) / 2;
                if (sx == 0 || sy == 0) continue;
                hipLaunchKernelGGL((rc_round_kernel<T, DIL, false>), dim3((unsigned)(sx * sy * nplanes)), dim3(256), 0,
                                   ctx->stream, seed, mask, out, H, W, ntx, nty, cy, cx, c8, hseed, h,
                                   k == 1 ? (const unsigned*)nullptr : (const unsigned*)(cnt + k - 1), cnt + k, cnt,
                                   (unsigned*)viol);
            }
        AMT_LAUNCH_CHECK();
        unsigned host[1 + RC_BATCH];
        AMT_HIP_CHECK(hipMemcpyAsync(host, cnt, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
        AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (host[0] != 0u) {
            const int bad = (int)~host[0];
            unsigned n = 0;
            AMT_HIP_CHECK(hipMemcpyAsync(&n, (unsigned*)viol + bad, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
            AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            if (DIL)
                amt_set_error("rank_filter: Intensity of seed image must be less than that of the mask image for "
                              "reconstruction by dilation (plane %d: %u pixels of the seed are above the mask)", bad, n);
            else
                amt_set_error("rank_filter: Intensity of seed image must be greater than that of the mask image for "
                              "reconstruction by erosion (plane %d: %u pixels of the seed are below the mask)", bad, n);
            return AMT_EINVAL;
        }
        ++syncs;
        for (int k = 1; k <= RC_BATCH; ++k)
            if (host[k] == 0u) {
                // AMT_DEBUG_RECONSTRUCT=1 (tools/time_reconstruction.py): how long the data made the call -- the rounds
                // up to and including the clean one (round 0 counted) and the host's synchronisations
                static const bool report = [] {
                    const char* e = getenv("AMT_DEBUG_RECONSTRUCT");
                    return e && e[0] == '1';
                }();
                if (report)
                    fprintf(stderr, "amt reconstruct: rounds=%llu syncs=%llu\n", rounds + (unsigned long long)k + 1, syncs);
                return AMT_OK;
            }
        rounds += RC_BATCH;
        if (rounds > limit) {
            amt_set_error("rank_filter: reconstruction did not converge in %llu rounds", rounds);
            return AMT_EHIP;
        }
    }
}

// Ops 3 .. 6 of amt_rank_filter, which has checked the operands' aliasing.  `mask` is the call's `minuend` for ops 3 / 4;
// ops 5 / 6 take the image itself as the mask.  Every refusal that needs no device comes before the context is looked at.
int amt_i_reconstruct(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W,
                      const uint8_t* footprint, int fh, int fw, int op, double cval, const void* minuend) {
    AMT_REQUIRE(in && out && footprint && nplanes >= 0 && H > 0 && W > 0, "rank_filter: bad arguments");
    AMT_REQUIRE(dtype == AMT_U16 || dtype == AMT_F64, "rank_filter: dtype must be AMT_U16 or AMT_F64");
    bool cross = fh == 3 && fw == 3, ones = cross;
    if (cross)
        for (int i = 0; i < 9; ++i) {
            const bool on = footprint[i] != 0, arm = (i & 1) || i == 4;
            if (on != arm) cross = false;
            if (!on) ones = false;
        }
    AMT_REQUIRE(cross || ones,
                "rank_filter: reconstruction takes the 3 x 3 cross (4-connected) or the 3 x 3 all-ones footprint "
                "(8-connected), got another %d x %d footprint", fh, fw);
    const bool by_dilation = op == AMT_RANK_RECONSTRUCT_DILATION || op == AMT_RANK_HMAX_RECONSTRUCT;
    const bool hop = op == AMT_RANK_HMAX_RECONSTRUCT || op == AMT_RANK_HMIN_RECONSTRUCT;
    if (!hop) {
        AMT_REQUIRE(minuend != nullptr, "rank_filter: reconstruction takes its mask image in `minuend`, which is NULL");
    } else {
        if (dtype == AMT_U16)
            AMT_REQUIRE(cval >= 1.0 && cval <= 65535.0 && cval == std::floor(cval),
                        "rank_filter: h (cval) of an AMT_U16 image must be an integer in 1..65535, got %g", cval);
        else
            AMT_REQUIRE(std::isfinite(cval) && cval > 0.0, "rank_filter: h (cval) must be finite and > 0, got %g", cval);
        AMT_REQUIRE(op != AMT_RANK_HMIN_RECONSTRUCT || minuend == nullptr,
                    "rank_filter: AMT_RANK_HMIN_RECONSTRUCT takes no minuend");
    }
    AMT_REQUIRE((unsigned long long)H * W < 0x80000000ull, "rank_filter: reconstruction needs H * W < 2^31 (got %d x %d)", H, W);
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0) return AMT_OK;
    const void* mask = hop ? in : minuend;
    const int c8 = ones ? 1 : 0, hseed = hop ? 1 : 0;
    if (dtype == AMT_U16) {
        const uint16_t h = hop ? (uint16_t)cval : (uint16_t)0;
        return by_dilation ? rc_run<uint16_t, true>(ctx, (const uint16_t*)in, (const uint16_t*)mask, (uint16_t*)out, nplanes,
                                                    H, W, c8, hseed, h)
                           : rc_run<uint16_t, false>(ctx, (const uint16_t*)in, (const uint16_t*)mask, (uint16_t*)out, nplanes,
                                                     H, W, c8, hseed, h);
    }
    const double h = hop ? cval : 0.0;
    return by_dilation
               ? rc_run<double, true>(ctx, (const double*)in, (const double*)mask, (double*)out, nplanes, H, W, c8, hseed, h)
               : rc_run<double, false>(ctx, (const double*)in, (const double*)mask, (double*)out, nplanes, H, W, c8, hseed, h);
}
