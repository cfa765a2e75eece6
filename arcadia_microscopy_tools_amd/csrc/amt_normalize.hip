// Image normalisation of CellposeModel.eval on the network + HIP route (R/model.py:206-215 calls eval, which maps every
// channel so that its 1st percentile becomes 0 and its 99th becomes 1 before the network sees it; restated from cellpose
// 4.0.x transforms.normalize_img / normalize99, PARITY UNPINNED; caller: cellpose_hip.normalize_image).
//
// Per plane, all in float32, one operation each and in this order (no reciprocal, no fused multiply-add; the library is
// built with -ffp-contract=off and HIP's float division is correctly rounded, so the result equals numpy's bit for bit):
//     lo, hi = the plane's pair rounded to float32;  d = hi - lo
//     y = d > 1e-3f ? (x - lo) / d : 0;  invert: y = 1 - y
// An HBM-bound pass: 2 / 4 / 8 bytes read and 4 written per sample.  A lane owns 8 consecutive samples (one, two or four
// 16-byte loads, two 16-byte stores) and four such groups per trip, all requested before the first is used; the
// plane's pair, its difference and the degenerate-plane decision are wave-uniform (scalar registers), and a degenerate
// plane is filled without being read.  Planes follow each other without padding, so a plane whose first sample is not
// on a 16-byte boundary (n % 8 != 0) peels up to 7 leading samples; they and the tail after the last whole group go
// one sample per lane.
#include "amt_internal.h"

namespace {

constexpr int NRM_V = 8;       // samples per lane and group
constexpr int NRM_GROUPS = 4;  // groups per lane and trip, all loaded before the first use
constexpr int NRM_BLOCK = 256;

typedef unsigned nrm_u4 __attribute__((ext_vector_type(4)));  // 16 bytes in four consecutive registers

template <typename T>
struct nrm_raw {  // the 8 samples of a group as they come from memory
    nrm_u4 q[sizeof(T) * NRM_V / 16];
};

template <typename T>
__device__ __forceinline__ nrm_raw<T> nrm_load(const T* p) {
    nrm_raw<T> r;
    const nrm_u4* v = reinterpret_cast<const nrm_u4*>(p);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) * NRM_V / 16); ++k) r.q[k] = v[k];
    return r;
}

__device__ __forceinline__ void nrm_unpack(const nrm_raw<uint16_t>& r, float (&x)[NRM_V]) {
    const unsigned w[4] = {r.q[0].x, r.q[0].y, r.q[0].z, r.q[0].w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x[2 * k] = (float)(w[k] & 0xFFFFu);
        x[2 * k + 1] = (float)(w[k] >> 16);
    }
}

__device__ __forceinline__ void nrm_unpack(const nrm_raw<float>& r, float (&x)[NRM_V]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        x[4 * k] = __uint_as_float(r.q[k].x);
        x[4 * k + 1] = __uint_as_float(r.q[k].y);
        x[4 * k + 2] = __uint_as_float(r.q[k].z);
        x[4 * k + 3] = __uint_as_float(r.q[k].w);
    }
}

__device__ __forceinline__ void nrm_unpack(const nrm_raw<double>& r, float (&x)[NRM_V]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // float64 samples are rounded once, to nearest even, as numpy's astype does
        x[2 * k] = (float)__hiloint2double((int)r.q[k].y, (int)r.q[k].x);
        x[2 * k + 1] = (float)__hiloint2double((int)r.q[k].w, (int)r.q[k].z);
    }
}

__device__ __forceinline__ float nrm_one(float x, float lo, float d, int invert) {
    const float y = (x - lo) / d;
    return invert ? 1.0f - y : y;
}

__device__ __forceinline__ void nrm_store(float* p, const float (&y)[NRM_V]) {
    float4* o = reinterpret_cast<float4*>(p);
    o[0] = make_float4(y[0], y[1], y[2], y[3]);
    o[1] = make_float4(y[4], y[5], y[6], y[7]);
}

// grid = (blocks per plane, planes).  `vec` = both base pointers are 16-byte aligned (otherwise every sample takes the
// one-sample path).
template <typename T>
__global__ void __launch_bounds__(NRM_BLOCK) normalize_planes_kernel(const T* __restrict__ in,
                                                                     const void* __restrict__ lohi, int lohi_f64,
                                                                     int invert, float* __restrict__ out, size_t n,
                                                                     int vec) {
    const size_t p = blockIdx.y;
    float lo, hi;
    if (lohi_f64) {  // percentiles straight from the order-statistics kernels: rounded to float32 here, once
        lo = (float)static_cast<const double*>(lohi)[2 * p];
        hi = (float)static_cast<const double*>(lohi)[2 * p + 1];
    } else {
        lo = static_cast<const float*>(lohi)[2 * p];
        hi = static_cast<const float*>(lohi)[2 * p + 1];
    }
    const float d = hi - lo;
    const bool live = d > 1e-3f;  // once per plane; false for NaN too
    const float dead = invert ? 1.0f : 0.0f;
    const size_t base = p * n;
    const T* ip = in + base;
    float* op = out + base;
    size_t head = n;
    if (vec) {
        head = (size_t)((NRM_V - (int)(base & (NRM_V - 1))) & (NRM_V - 1));
        if (head > n) head = n;
    }
    const size_t ngroups = (n - head) / NRM_V;
    const size_t tail0 = head + ngroups * NRM_V;
    const size_t nloose = head + (n - tail0);
    const size_t tid = (size_t)blockIdx.x * NRM_BLOCK + threadIdx.x, nthreads = (size_t)gridDim.x * NRM_BLOCK;

    for (size_t i = tid; i < nloose; i += nthreads) {  // head and tail: < 16 samples of an aligned call
        const size_t j = i < head ? i : tail0 + (i - head);
        op[j] = live ? nrm_one((float)ip[j], lo, d, invert) : dead;
    }

    const T* vp = ip + head;
    float* vo = op + head;
    const size_t trip = nthreads * NRM_GROUPS;
    for (size_t g0 = (size_t)blockIdx.x * NRM_BLOCK * NRM_GROUPS; g0 < ngroups; g0 += trip) {
        size_t g[NRM_GROUPS];
#pragma unroll
        for (int k = 0; k < NRM_GROUPS; ++k) g[k] = g0 + (size_t)k * NRM_BLOCK + threadIdx.x;
        float y[NRM_GROUPS][NRM_V];
        if (live) {
            nrm_raw<T> raw[NRM_GROUPS];
            // unconditional loads from clamped group numbers (g0 < ngroups, so ngroups - 1 is a group of this plane);
            // validity is applied at the store
#pragma unroll
            for (int k = 0; k < NRM_GROUPS; ++k)
                raw[k] = nrm_load<T>(vp + (g[k] < ngroups ? g[k] : ngroups - 1) * NRM_V);
            // nothing crosses this line: the scheduler otherwise sinks the later groups' loads below the first groups'
            // divisions (two loads in flight instead of all); the waits that follow are counted, one group at a time
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < NRM_GROUPS; ++k) {
                float x[NRM_V];
                nrm_unpack(raw[k], x);
#pragma unroll
                for (int s = 0; s < NRM_V; ++s) y[k][s] = nrm_one(x[s], lo, d, invert);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NRM_GROUPS; ++k)
#pragma unroll
                for (int s = 0; s < NRM_V; ++s) y[k][s] = dead;
        }
#pragma unroll
        for (int k = 0; k < NRM_GROUPS; ++k)
            if (g[k] < ngroups) nrm_store(vo + g[k] * NRM_V, y[k]);
    }
}

// float32 -> float64, exact: four samples per lane (one 16-byte load, two 16-byte stores), the rest one per lane
__global__ void __launch_bounds__(NRM_BLOCK) convert_f32_f64_kernel(const float* __restrict__ in,
                                                                    double* __restrict__ out, size_t n, int vec) {
    const size_t tid = (size_t)blockIdx.x * NRM_BLOCK + threadIdx.x, nthreads = (size_t)gridDim.x * NRM_BLOCK;
    const size_t nquads = vec ? n / 4 : 0;
    for (size_t q = tid; q < nquads; q += nthreads) {
        const float4 v = reinterpret_cast<const float4*>(in)[q];
        double2* o = reinterpret_cast<double2*>(out) + 2 * q;
        o[0] = make_double2((double)v.x, (double)v.y);
        o[1] = make_double2((double)v.z, (double)v.w);
    }
    for (size_t i = nquads * 4 + tid; i < n; i += nthreads) out[i] = (double)in[i];
}

bool aligned16(const void* a, const void* b) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

}  // namespace

extern "C" int amt_convert_f32_f64(amt_ctx* ctx, const float* in, double* out, size_t n) {
    AMT_CHECK_OPERANDS("amt_convert_f32_f64", amt_in("in", in, amt_span(4, (long long)n)), amt_out("out", out, amt_span(8, (long long)n)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(in && out, "convert_f32_f64: null pointer");
    if (n == 0) return AMT_OK;
    hipLaunchKernelGGL(convert_f32_f64_kernel, dim3(amt_grid_for((n + 3) / 4, NRM_BLOCK)), dim3(NRM_BLOCK), 0,
                       ctx->stream, in, out, n, aligned16(in, out) ? 1 : 0);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

extern "C" int amt_normalize_planes_f32(amt_ctx* ctx, const void* in, int in_dtype, const void* lohi_dev, int lohi_dtype,
                                        int invert, float* out, int nplanes, size_t n) {
    AMT_CHECK_OPERANDS("amt_normalize_planes_f32", amt_in("in", in, amt_span(amt_esize(in_dtype), nplanes, (long long)n)),
                       amt_in("lohi_dev", lohi_dev, amt_span(amt_esize(lohi_dtype), nplanes, 2)),
                       amt_out("out", out, amt_span(4, nplanes, (long long)n)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(in && lohi_dev && out, "normalize_planes_f32: null pointer");
    AMT_REQUIRE(in_dtype == AMT_U16 || in_dtype == AMT_F32 || in_dtype == AMT_F64,
                "normalize_planes_f32: in_dtype must be AMT_U16, AMT_F32 or AMT_F64");
    AMT_REQUIRE(lohi_dtype == AMT_F32 || lohi_dtype == AMT_F64,
                "normalize_planes_f32: lohi_dtype must be AMT_F32 or AMT_F64");
    AMT_REQUIRE(nplanes >= 0 && nplanes <= 65535, "normalize_planes_f32: %d planes (0..65535 per call)", nplanes);
    if (nplanes == 0 || n == 0) return AMT_OK;
    const int vec = aligned16(in, out) ? 1 : 0;
    const size_t per_trip = (size_t)NRM_V * NRM_GROUPS;
    dim3 grid(amt_grid_for((n + per_trip - 1) / per_trip, NRM_BLOCK, 2048), nplanes);
    const int f64 = lohi_dtype == AMT_F64, inv = invert ? 1 : 0;
    switch (in_dtype) {
        case AMT_U16:
            hipLaunchKernelGGL((normalize_planes_kernel<uint16_t>), grid, dim3(NRM_BLOCK), 0, ctx->stream,
                               (const uint16_t*)in, lohi_dev, f64, inv, out, n, vec);
            break;
        case AMT_F32:
            hipLaunchKernelGGL((normalize_planes_kernel<float>), grid, dim3(NRM_BLOCK), 0, ctx->stream,
                               (const float*)in, lohi_dev, f64, inv, out, n, vec);
            break;
        default:
            hipLaunchKernelGGL((normalize_planes_kernel<double>), grid, dim3(NRM_BLOCK), 0, ctx->stream,
                               (const double*)in, lohi_dev, f64, inv, out, n, vec);
            break;
    }
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
