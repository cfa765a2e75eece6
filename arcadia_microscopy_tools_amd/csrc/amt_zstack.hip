// Z-stacks: ops AMT_RANK_Z_PROJECT .. AMT_RANK_Z_TAKE of amt_rank_filter (include/amt_hip.h states the definitions).  `in`
// is nplanes x Z x H x W, `mode` carries Z.  Everything is integer arithmetic but the two means, which divide once; no op
// reserves scratch, none waits for the device.
//
// Focus index / focus stack (ops 12 / 13): a workgroup owns one AMT_ZSTACK_TILE_H x AMT_ZSTACK_TILE_W output tile and loops
// over z.  Per plane it stages the tile plus a halo of r + 1 pixels in LDS (edge replication by clamped addresses), forms
// the Laplacian L on the tile plus r (0 outside the image), sums L^2 along rows with a sliding window, then along columns,
// and keeps the best E, its z and (op 13) its pixel value in registers.  The loads of plane z + 1 are issued into registers
// before plane z is summed.  Every stack is read once plus halo, and only `out` is written.
//
// Focus sums (op 11): every workgroup sums a chunk of a plane and adds its four totals to the row with 64-bit integer
// atomics (integers: the bytes depend on no order); the rows are cleared by a memset on the stream first.
#include "amt_internal.h"

namespace {

constexpr int ZT_H = AMT_ZSTACK_TILE_H, ZT_W = AMT_ZSTACK_TILE_W;
constexpr int ZT_THREADS = 256;
constexpr int ZT_WAVES = ZT_THREADS / 64;
constexpr int ZT_OWN = ZT_H / ZT_WAVES;  // rows of a column one thread owns: wave q owns rows q * ZT_OWN ...
constexpr int ZT_SEG = ZT_W / ZT_WAVES;  // columns of a row one thread sums: wave s sums columns s * ZT_SEG ...
constexpr int ZT_RP = ZT_W + 1;          // pitch of the row sums
static_assert(ZT_W == 64 && ZT_H % ZT_WAVES == 0, "a wave's lanes are the tile's columns");

// elements of the staged tile (halo rb + 1) per thread
constexpr int zf_nload(int rb) { return ((ZT_H + 2 * rb + 2) * (ZT_W + 2 * rb + 2) + ZT_THREADS - 1) / ZT_THREADS; }
static size_t zf_lds_bytes(int r) {
    const size_t lh = ZT_H + 2 * r, lp = (ZT_W + 2 * r) | 1;
    return lh * ZT_RP * 8 + lh * lp * 4 + (size_t)(ZT_H + 2 * r + 2) * (ZT_W + 2 * r + 2) * 2;
}

__device__ __forceinline__ int zclamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned long long zsq(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);  // |L| < 2^19: one widening multiply
    return (unsigned long long)a * a;
}

// RB: the largest radius this instance stages (its register prefetch is sized for it).  STACK: op 13, else op 12.
template <typename T, int RB, bool STACK>
__global__ void __launch_bounds__(ZT_THREADS) zfocus_kernel(const T* __restrict__ in, void* __restrict__ outv, int nplanes,
                                                            int Z, int H, int W, int r, int tiles_x) {
    extern __shared__ unsigned long long zf_lds[];
    constexpr int NLOAD = zf_nload(RB);
    const int rh = ZT_H + 2 * r + 2, rw = ZT_W + 2 * r + 2;  // the staged tile
    const int lh = ZT_H + 2 * r, lw = ZT_W + 2 * r, lp = lw | 1;  // the Laplacian's
    unsigned long long* R = zf_lds;                              // lh x ZT_RP row sums
    int* L = reinterpret_cast<int*>(R + (size_t)lh * ZT_RP);     // lh x lp
    uint16_t* raw = reinterpret_cast<uint16_t*>(L + (size_t)lh * lp);  // rh x rw
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)(blockIdx.x % tiles_x) * ZT_W, y0 = (int)(blockIdx.x / tiles_x) * ZT_H;
    const size_t HW = (size_t)H * W;
    const int nraw = rh * rw;

    int off[NLOAD];  // offset inside its plane of the pixel a staged element shows, -1 past the staged tile
#pragma unroll
    for (int k = 0; k < NLOAD; ++k) {
        const int e = tid + k * ZT_THREADS;
        const int ry = e / rw, rx = e - ry * rw;
        off[k] = e < nraw ? zclamp(y0 - r - 1 + ry, H - 1) * W + zclamp(x0 - r - 1 + rx, W - 1) : -1;
    }
    for (int s = blockIdx.y; s < nplanes; s += gridDim.y) {
        const T* stack = in + (size_t)s * Z * HW;
        long long best[ZT_OWN];
        int bz[ZT_OWN];
        T bv[ZT_OWN];
#pragma unroll
        for (int i = 0; i < ZT_OWN; ++i) {
            best[i] = -1;
            bz[i] = 0;
            bv[i] = 0;
        }
        T pre[NLOAD];
#pragma unroll
        for (int k = 0; k < NLOAD; ++k) pre[k] = off[k] >= 0 ? stack[off[k]] : (T)0;
        for (int z = 0; z < Z; ++z) {
#pragma unroll
            for (int k = 0; k < NLOAD; ++k)
                if (off[k] >= 0) raw[tid + k * ZT_THREADS] = pre[k];
            __syncthreads();
            if (z + 1 < Z) {  // in flight while this plane is summed
                const T* next = stack + (size_t)(z + 1) * HW;
#pragma unroll
                for (int k = 0; k < NLOAD; ++k) pre[k] = off[k] >= 0 ? next[off[k]] : (T)0;
            }
            // L on the tile plus r; a position outside the image counts 0
            for (int ly = wave; ly < lh; ly += ZT_WAVES) {
                const int gy = y0 - r + ly;
                for (int lx = lane; lx < lw; lx += 64) {
                    const int gx = x0 - r + lx;
                    const uint16_t* c = raw + (ly + 1) * rw + lx + 1;
                    const int v = 4 * (int)c[0] - (int)c[-rw] - (int)c[rw] - (int)c[-1] - (int)c[1];
                    L[ly * lp + lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? v : 0;
                }
            }
            __syncthreads();
            // rows: R[row][x] = sum of L^2 over columns x .. x + 2 r of L (the tile's column x - r .. x + r)
            for (int row = lane; row < lh; row += 64) {
                const int* lr = L + row * lp + wave * ZT_SEG;
                unsigned long long* rr = R + (size_t)row * ZT_RP + wave * ZT_SEG;
                unsigned long long sum = 0;
                for (int j = 0; j <= 2 * r; ++j) sum += zsq(lr[j]);
                rr[0] = sum;
#pragma unroll
                for (int i = 1; i < ZT_SEG; ++i) {
                    sum += zsq(lr[i + 2 * r]) - zsq(lr[i - 1]);
                    rr[i] = sum;
                }
            }
            __syncthreads();
            // columns: E of output row y = sum of R over rows y .. y + 2 r
            {
                const unsigned long long* rc = R + (size_t)(wave * ZT_OWN) * ZT_RP + lane;
                unsigned long long e = 0;
                for (int j = 0; j <= 2 * r; ++j) e += rc[(size_t)j * ZT_RP];
#pragma unroll
                for (int i = 0; i < ZT_OWN; ++i) {
                    if (i > 0) e += rc[(size_t)(i + 2 * r) * ZT_RP] - rc[(size_t)(i - 1) * ZT_RP];
                    if ((long long)e > best[i]) {  // strictly larger: the smallest z among equals stays
                        best[i] = (long long)e;
                        bz[i] = z;
                        if (STACK) bv[i] = (T)raw[(wave * ZT_OWN + i + r + 1) * rw + lane + r + 1];
                    }
                }
            }
            __syncthreads();
        }
        const int gx = x0 + lane;
        if (gx < W) {
#pragma unroll
            for (int i = 0; i < ZT_OWN; ++i) {
                const int gy = y0 + wave * ZT_OWN + i;
                if (gy < H) {
                    const size_t o = (size_t)s * HW + (size_t)gy * W + gx;
                    if (STACK) reinterpret_cast<T*>(outv)[o] = bv[i];
                    else reinterpret_cast<uint16_t*>(outv)[o] = (uint16_t)bz[i];
                }
            }
        }
    }
}

template <typename T, int RB, bool STACK>
int zfocus_launch(amt_ctx* ctx, const void* in, void* out, int nplanes, int Z, int H, int W, int r) {
    // up to 101 KiB at r = 15, more than the 64 KiB a launch gets without asking; always the largest size, so that calls
    // from several host threads cannot undercut one another
    AMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&zfocus_kernel<T, RB, STACK>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)zf_lds_bytes(RB)));
    const int tiles_x = (W + ZT_W - 1) / ZT_W, tiles_y = (H + ZT_H - 1) / ZT_H;
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, nplanes < 65535 ? nplanes : 65535);
    hipLaunchKernelGGL((zfocus_kernel<T, RB, STACK>), grid, dim3(ZT_THREADS), zf_lds_bytes(r), ctx->stream, (const T*)in, out,
                       nplanes, Z, H, W, r, tiles_x);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

template <typename T>
int zfocus_go(amt_ctx* ctx, const void* in, void* out, int nplanes, int Z, int H, int W, int r, bool stack) {
    if (r <= 4) return stack ? zfocus_launch<T, 4, true>(ctx, in, out, nplanes, Z, H, W, r)
                             : zfocus_launch<T, 4, false>(ctx, in, out, nplanes, Z, H, W, r);
    return stack ? zfocus_launch<T, 15, true>(ctx, in, out, nplanes, Z, H, W, r)
                 : zfocus_launch<T, 15, false>(ctx, in, out, nplanes, Z, H, W, r);
}

// ---- projections: VEC pixels per lane and step, one 16-byte load per plane -------------------------------------------
template <typename E, int N>
struct alignas(sizeof(E) * N > 16 ? 16 : sizeof(E) * N) zvec {
    E v[N];
};
template <typename T> struct zacc { typedef unsigned type; };  // 65535 planes of 65535 stay below 2^32
template <> struct zacc<double> { typedef double type; };

// METHOD: 0 max, 1 min, 2 mean (O = double)
template <typename T, typename O, int METHOD, int VEC>
__global__ void __launch_bounds__(256) zproject_kernel(const T* __restrict__ in, O* __restrict__ out, int nplanes, int Z,
                                                       size_t HW) {
    typedef zvec<T, VEC> vin;
    typedef zvec<O, VEC> vout;
    typedef typename zacc<T>::type A;
    const size_t groups = HW / VEC;
    for (int s = blockIdx.y; s < nplanes; s += gridDim.y) {
        const vin* src = reinterpret_cast<const vin*>(in + (size_t)s * Z * HW);
        vout* dst = reinterpret_cast<vout*>(out + (size_t)s * HW);
        for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
            vin first = src[g];
            A acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = (A)first.v[k];
#pragma unroll 4
            for (int z = 1; z < Z; ++z) {
                const vin p = src[(size_t)z * groups + g];
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const A v = (A)p.v[k];
                    if (METHOD == 0) acc[k] = v > acc[k] ? v : acc[k];
                    else if (METHOD == 1) acc[k] = v < acc[k] ? v : acc[k];
                    else acc[k] += v;  // z = 0, 1, ... in order
                }
            }
            vout o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = METHOD == 2 ? (O)((double)acc[k] / (double)Z) : (O)acc[k];
            dst[g] = o;
        }
    }
}

template <typename T, int VEC>
int zproject_launch(amt_ctx* ctx, const void* in, void* out, int nplanes, int Z, size_t HW, int method) {
    const dim3 grid(amt_grid_for(HW / VEC, 256, 4096), nplanes < 65535 ? nplanes : 65535);
    if (method == 0)
        hipLaunchKernelGGL((zproject_kernel<T, T, 0, VEC>), grid, dim3(256), 0, ctx->stream, (const T*)in, (T*)out, nplanes, Z, HW);
    else if (method == 1)
        hipLaunchKernelGGL((zproject_kernel<T, T, 1, VEC>), grid, dim3(256), 0, ctx->stream, (const T*)in, (T*)out, nplanes, Z, HW);
    else
        hipLaunchKernelGGL((zproject_kernel<T, double, 2, VEC>), grid, dim3(256), 0, ctx->stream, (const T*)in, (double*)out,
                           nplanes, Z, HW);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

template <typename T>
int zproject_go(amt_ctx* ctx, const void* in, void* out, int nplanes, int Z, size_t HW, int method) {
    constexpr int VEC = 16 / (int)sizeof(T);
    // whole 16-byte groups per plane, read and written aligned; anything else goes pixel by pixel
    const bool wide = HW % VEC == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    return wide ? zproject_launch<T, VEC>(ctx, in, out, nplanes, Z, HW, method)
                : zproject_launch<T, 1>(ctx, in, out, nplanes, Z, HW, method);
}

// ---- gather along z: four pixels per lane --------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) ztake_kernel(const T* __restrict__ in, const uint16_t* __restrict__ index,
                                                    T* __restrict__ out, int nplanes, int Z, size_t HW) {
    for (int s = blockIdx.y; s < nplanes; s += gridDim.y) {
        const T* stack = in + (size_t)s * Z * HW;
        const uint16_t* idx = index + (size_t)s * HW;
        T* dst = out + (size_t)s * HW;
        for (size_t base = (size_t)blockIdx.x * 1024; base < HW; base += (size_t)gridDim.x * 1024) {
            int zi[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t p = base + k * 256 + threadIdx.x;
                zi[k] = p < HW ? (int)idx[p] : 0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t p = base + k * 256 + threadIdx.x;
                const int z = zi[k] < Z - 1 ? zi[k] : Z - 1;  // an index past the stack is clamped
                if (p < HW) dst[p] = stack[(size_t)z * HW + p];
            }
        }
    }
}

template <typename T>
int ztake_go(amt_ctx* ctx, const void* in, const void* index, void* out, int nplanes, int Z, size_t HW) {
    const dim3 grid(amt_grid_for(HW, 1024, 4096), nplanes < 65535 ? nplanes : 65535);
    hipLaunchKernelGGL(ztake_kernel<T>, grid, dim3(256), 0, ctx->stream, (const T*)in, (const uint16_t*)index, (T*)out, nplanes,
                       Z, HW);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- focus sums ------------------------------------------------------------------------------------------------------
constexpr int ZS_CHUNK = 256 * 16;  // pixels of a plane per workgroup

__device__ __forceinline__ unsigned long long zwave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// WIDE: W is a multiple of 8 and the planes are aligned to 8 pixels -- a lane takes 8 pixels of a row with one load each
// for the row, the row above and the row below, one pixel to the left and two to the right
template <typename T, bool WIDE>
__global__ void __launch_bounds__(256) zsums_kernel(const T* __restrict__ in, unsigned long long* __restrict__ out,
                                                    size_t nrows, int H, int W) {
    __shared__ unsigned long long part[ZT_WAVES][AMT_ZF_NCOLS];
    const int HWi = H * W;  // <= 2^27
    for (size_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const T* P = in + row * (size_t)HWi;
        unsigned long long acc[AMT_ZF_NCOLS] = {0, 0, 0, 0};
        const int base = blockIdx.x * ZS_CHUNK;
        if (WIDE) {
            typedef zvec<T, 8> v8;
            typedef zvec<T, 2> v2;
            for (int k = 0; k < ZS_CHUNK / (256 * 8); ++k) {
                const int p0 = base + (k * 256 + (int)threadIdx.x) * 8;
                if (p0 >= HWi) break;
                const int y0 = p0 / W, x0 = p0 - y0 * W;
                const v8 c = *reinterpret_cast<const v8*>(P + p0);
                const v8 up = *reinterpret_cast<const v8*>(P + (y0 > 0 ? p0 - W : p0));
                const v8 dn = *reinterpret_cast<const v8*>(P + (y0 + 1 < H ? p0 + W : p0));
                const bool more = x0 + 8 < W;  // then x0 + 9 < W as well: W is a multiple of 8
                const int left = x0 > 0 ? (int)P[p0 - 1] : (int)c.v[0];
                v2 rt;
                rt.v[0] = rt.v[1] = c.v[7];
                if (more) rt = *reinterpret_cast<const v2*>(P + p0 + 8);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int ci = (int)c.v[i];
                    const int l = i > 0 ? (int)c.v[i > 0 ? i - 1 : 0] : left;
                    const int r1 = i < 7 ? (int)c.v[i < 7 ? i + 1 : 7] : (int)rt.v[0];
                    acc[AMT_ZF_SUM] += (unsigned)ci;
                    acc[AMT_ZF_SUMSQ] += zsq(ci);
                    acc[AMT_ZF_LAP_SUMSQ] += zsq(4 * ci - (int)up.v[i] - (int)dn.v[i] - l - r1);
                    if (i < 6) acc[AMT_ZF_BRENNER] += zsq((int)c.v[i < 6 ? i + 2 : 7] - ci);
                    else if (more) acc[AMT_ZF_BRENNER] += zsq((int)rt.v[i - 6] - ci);
                }
            }
        } else {
        int y = (base + (int)threadIdx.x) / W, x = base + (int)threadIdx.x - y * W;
        for (int k = 0; k < ZS_CHUNK / 256; ++k, x += 256) {
            const int p = base + k * 256 + (int)threadIdx.x;
            if (p >= HWi) break;
            if (W >= 256) {  // a step of 256 pixels crosses one row end at most
                if (x >= W) {
                    x -= W;
                    ++y;
                }
            } else {
                y = p / W;
                x = p - y * W;
            }
            const int c = (int)P[p];
            const int up = (int)P[y > 0 ? p - W : p], down = (int)P[y + 1 < H ? p + W : p];
            const int left = (int)P[x > 0 ? p - 1 : p], right = (int)P[x + 1 < W ? p + 1 : p];
            acc[AMT_ZF_SUM] += (unsigned)c;
            acc[AMT_ZF_SUMSQ] += zsq(c);
            acc[AMT_ZF_LAP_SUMSQ] += zsq(4 * c - up - down - left - right);
            if (x + 2 < W) acc[AMT_ZF_BRENNER] += zsq((int)P[p + 2] - c);
        }
        }
#pragma unroll
        for (int j = 0; j < AMT_ZF_NCOLS; ++j) {
            const unsigned long long t = zwave_sum(acc[j]);
            if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][j] = t;
        }
        __syncthreads();
        if (threadIdx.x < AMT_ZF_NCOLS) {
            unsigned long long t = 0;
            for (int w = 0; w < ZT_WAVES; ++w) t += part[w][threadIdx.x];
            if (t) atomicAdd(&out[row * AMT_ZF_NCOLS + threadIdx.x], t);
        }
        __syncthreads();
    }
}

template <typename T>
int zsums_go(amt_ctx* ctx, const void* in, void* out, int nplanes, int Z, int H, int W) {
    const size_t nrows = (size_t)nplanes * Z;
    AMT_HIP_CHECK(hipMemsetAsync(out, 0, nrows * AMT_ZF_NCOLS * sizeof(unsigned long long), ctx->stream));
    const size_t HW = (size_t)H * W;
    const dim3 grid((unsigned)((HW + ZS_CHUNK - 1) / ZS_CHUNK), (unsigned)(nrows < 65535 ? nrows : 65535));
    // whole groups of 8 pixels per row, read aligned; anything else goes pixel by pixel
    if (W % 8 == 0 && (reinterpret_cast<uintptr_t>(in) % (8 * sizeof(T))) == 0)
        hipLaunchKernelGGL((zsums_kernel<T, true>), grid, dim3(256), 0, ctx->stream, (const T*)in, (unsigned long long*)out, nrows,
                           H, W);
    else
        hipLaunchKernelGGL((zsums_kernel<T, false>), grid, dim3(256), 0, ctx->stream, (const T*)in, (unsigned long long*)out, nrows,
                           H, W);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

}  // namespace

// Byte lengths of the operands of ops 10 .. 14, for amt_rank_filter's aliasing check (0 = absent or not yet refusable)
void amt_i_zstack_spans(int op, int dtype, int nplanes, int H, int W, int Z, double cval, size_t* in_bytes, size_t* out_bytes,
                        size_t* minuend_bytes) {
    const size_t e = amt_esize(dtype);
    *in_bytes = amt_span(e, nplanes, Z, H, W);
    *minuend_bytes = op == AMT_RANK_Z_TAKE ? amt_span(2, nplanes, H, W) : 0;
    switch (op) {
        case AMT_RANK_Z_PROJECT: *out_bytes = amt_span(cval == 2.0 ? 8 : e, nplanes, H, W); break;
        case AMT_RANK_Z_FOCUS_SUMS: *out_bytes = amt_span(8, nplanes, Z, AMT_ZF_NCOLS); break;
        case AMT_RANK_Z_FOCUS_INDEX: *out_bytes = amt_span(2, nplanes, H, W); break;
        default: *out_bytes = amt_span(e, nplanes, H, W); break;
    }
}

// Ops 10 .. 14 of amt_rank_filter, which has checked the operands' aliasing.  The refusals that need no device come before
// the context is looked at.
int amt_i_zstack(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W, const uint8_t* footprint,
                 int fh, int fw, int op, int Z, double cval, const void* minuend) {
    const char* what = op == AMT_RANK_Z_PROJECT        ? "z_project"
                       : op == AMT_RANK_Z_FOCUS_SUMS   ? "z_focus_sums"
                       : op == AMT_RANK_Z_FOCUS_INDEX  ? "z_focus_index"
                       : op == AMT_RANK_Z_FOCUS_STACK  ? "z_focus_stack"
                                                       : "z_take";
    const bool focus = op == AMT_RANK_Z_FOCUS_SUMS || op == AMT_RANK_Z_FOCUS_INDEX || op == AMT_RANK_Z_FOCUS_STACK;
    AMT_REQUIRE(in && out && nplanes >= 0 && H > 0 && W > 0, "rank_filter: %s: bad arguments", what);
    if (focus)
        AMT_REQUIRE(dtype == AMT_U8 || dtype == AMT_U16,
                    "rank_filter: %s: dtype must be AMT_U8 or AMT_U16 (focus is judged on raw data), got %d", what, dtype);
    else
        AMT_REQUIRE(dtype == AMT_U8 || dtype == AMT_U16 || dtype == AMT_F64,
                    "rank_filter: %s: dtype must be AMT_U8, AMT_U16 or AMT_F64, got %d", what, dtype);
    AMT_REQUIRE(Z >= 1 && Z <= 65535, "rank_filter: %s: Z (mode) must be in 1..65535, got %d", what, Z);
    int r = 0;
    if (op == AMT_RANK_Z_FOCUS_INDEX || op == AMT_RANK_Z_FOCUS_STACK) {
        bool ones = footprint && fh == fw && (fh & 1) && fh >= 1 && fh <= 2 * AMT_ZSTACK_MAX_RADIUS + 1;
        for (int i = 0; ones && i < fh * fw; ++i) ones = footprint[i] != 0;
        AMT_REQUIRE(ones, "rank_filter: %s: the footprint must be (2 r + 1) x (2 r + 1) all non-zero with r in 0..%d", what,
                    AMT_ZSTACK_MAX_RADIUS);
        r = fh / 2;
    }
    if (op == AMT_RANK_Z_PROJECT)
        AMT_REQUIRE(cval == 0.0 || cval == 1.0 || cval == 2.0, "rank_filter: z_project: cval must be 0 (max), 1 (min) or 2 (mean)");
    if (op == AMT_RANK_Z_TAKE)
        AMT_REQUIRE(minuend != nullptr, "rank_filter: z_take: minuend (the uint16 index map) is required");
    else
        AMT_REQUIRE(minuend == nullptr, "rank_filter: %s takes no minuend", what);
    AMT_REQUIRE((size_t)H * W < 0x80000000ull, "rank_filter: %s: plane too large (H * W must be below 2^31)", what);
    if (op == AMT_RANK_Z_FOCUS_SUMS)
        AMT_REQUIRE((size_t)H * W <= (1ull << 27), "rank_filter: z_focus_sums: H * W must not exceed 2^27 (the sums are 64-bit)");
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0) return AMT_OK;
    const size_t HW = (size_t)H * W;
    switch (op) {
        case AMT_RANK_Z_PROJECT: {
            const int method = (int)cval;
            if (dtype == AMT_U8) return zproject_go<uint8_t>(ctx, in, out, nplanes, Z, HW, method);
            if (dtype == AMT_U16) return zproject_go<uint16_t>(ctx, in, out, nplanes, Z, HW, method);
            return zproject_go<double>(ctx, in, out, nplanes, Z, HW, method);
        }
        case AMT_RANK_Z_FOCUS_SUMS:
            return dtype == AMT_U8 ? zsums_go<uint8_t>(ctx, in, out, nplanes, Z, H, W)
                                   : zsums_go<uint16_t>(ctx, in, out, nplanes, Z, H, W);
        case AMT_RANK_Z_FOCUS_INDEX:
        case AMT_RANK_Z_FOCUS_STACK:
            return dtype == AMT_U8 ? zfocus_go<uint8_t>(ctx, in, out, nplanes, Z, H, W, r, op == AMT_RANK_Z_FOCUS_STACK)
                                   : zfocus_go<uint16_t>(ctx, in, out, nplanes, Z, H, W, r, op == AMT_RANK_Z_FOCUS_STACK);
        default:
            if (dtype == AMT_U8) return ztake_go<uint8_t>(ctx, in, minuend, out, nplanes, Z, HW);
            if (dtype == AMT_U16) return ztake_go<uint16_t>(ctx, in, minuend, out, nplanes, Z, HW);
            return ztake_go<double>(ctx, in, minuend, out, nplanes, Z, HW);
    }
}
