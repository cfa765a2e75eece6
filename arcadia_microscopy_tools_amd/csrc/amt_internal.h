// Cross-translation-unit internals of libamt_hip.so (not part of the C ABI).
#pragma once
#include "amt_common.h"

#include <type_traits>

// ---- exclusive prefix sum over int32 arrays: one 1024-thread workgroup per plane ---------------
// data[plane][0..len) is replaced by its exclusive scan; total[plane] (optional) receives the sum.
template <int ITEMS>
__global__ void __launch_bounds__(1024) amt_scan_excl_kernel(int* __restrict__ data, int len, size_t plane_stride,
                                                             int* __restrict__ total,
                                                             const int* __restrict__ len_dev = nullptr) {
    __shared__ int s[1024];
    __shared__ int carry;
    int* d = data + (size_t)blockIdx.x * plane_stride;
    if (len_dev) len = len_dev[blockIdx.x];  // per-plane length that only the device knows
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int start = 0; start < len; start += 1024 * ITEMS) {
        const int b = start + threadIdx.x * ITEMS;
        int v[ITEMS];
        int sum = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            v[k] = (b + k < len) ? d[b + k] : 0;
            sum += v[k];
        }
        s[threadIdx.x] = sum;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            int t = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        const int c = carry;
        int run = c + s[threadIdx.x] - sum;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (b + k < len) d[b + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0 && total) total[blockIdx.x] = carry;
}

static inline int amt_scan_excl(amt_ctx* ctx, int* data, int len, size_t plane_stride, int* total, int nplanes) {
    if (len <= 4096)
        hipLaunchKernelGGL((amt_scan_excl_kernel<4>), dim3(nplanes), dim3(1024), 0, ctx->stream, data, len,
                           plane_stride, total, (const int*)nullptr);
    else
        hipLaunchKernelGGL((amt_scan_excl_kernel<16>), dim3(nplanes), dim3(1024), 0, ctx->stream, data, len,
                           plane_stride, total, (const int*)nullptr);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// same, with the per-plane length read from device memory (len_dev[plane] <= plane_stride)
static inline int amt_scan_excl_dev(amt_ctx* ctx, int* data, const int* len_dev, size_t plane_stride, int* total,
                                    int nplanes) {
    hipLaunchKernelGGL((amt_scan_excl_kernel<8>), dim3(nplanes), dim3(1024), 0, ctx->stream, data, 0, plane_stride,
                       total, len_dev);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- float64 min / max per plane on ordered 64-bit keys (amt_stats.hip) ---------------------------
// keys = 2 * nplanes scratch words; init -> (producers fold with atomicMin / atomicMax on amt_f64_key) -> finish
// zero_a / zero_b (nullable): na / nb 32-bit words cleared by the same launch
int amt_i_minmax_init(amt_ctx* ctx, unsigned long long* keys, int nplanes, uint32_t* zero_a = nullptr, size_t na = 0,
                      uint32_t* zero_b = nullptr, size_t nb = 0);
int amt_i_minmax_finish(amt_ctx* ctx, const unsigned long long* keys, double* out, int nplanes);
int amt_i_minmax_f64(amt_ctx* ctx, const double* in, unsigned long long* keys, double* out, int nplanes, size_t n);
// Otsu threshold of float64 histograms (np.histogram edges from minmax); thr_code (nullable) = 2 * bin index
int amt_i_otsu_from_hist(amt_ctx* ctx, const uint32_t* hist, const double* minmax, int nbins, double* thr,
                         double* thr_code, int nplanes);

// ---- connected components (amt_label.hip) -------------------------------------------------------
// Tile geometry of a labelling of nplanes planes of H x W pixels, derived once (amt_i_ccl_geom) for every launch of
// amt_label.hip and amt_watershed.hip.  Tiles are 64 x 64 pixels: `segs` per tile row, `trows` tile rows per plane.
struct ccl_geom {
    int nplanes, H, W;
    size_t n;          // pixels of a plane
    int segs, trows;   // 64-pixel column segments / 64-row tile rows of a plane
    size_t ntiles;     // nplanes * trows * segs: an int in the kernels, which only paths that bound it may launch
    size_t cap, nlist; // root lists (one per tile row): entries per list, number of lists = nplanes * trows
    int nblk;          // chunks of a plane in the raster renumbering's root counts
    int nrow_blocks;   // of gb.y, the blocks that stitch tile-row boundaries (the others: segment boundaries)
    int jobs;          // seams between the run-table tiles of a plane
    dim3 gs;           // a block per tile
    dim3 gb;           // ccl_border_kernel (gb.y == 0: a single tile, nothing to stitch)
    dim3 gseams;       // ccl_seams_runs_kernel: four jobs per block
    dim3 glists;       // the kernels that walk the root lists
    size_t multi_ints() const { return 16 + ntiles * 4; }  // scratch behind `multi`: the flag + two column words per tile
};
ccl_geom amt_i_ccl_geom(int nplanes, int H, int W);
// 4-connected components of a uint8 mask without the per-pixel compression pass: pixels point at their tile-local
// root; tile-local roots are appended to one list per TILE ROW, rootlist[(plane * trows + tile_row) * cap ...], counted
// in nroots[plane * trows + tile_row] (zero on entry).  Callers compress the listed roots themselves and resolve a pixel
// as L[L[p]].
// multi (nullable): ccl_geom::multi_ints() of scratch; with it a 0 / 1 mask takes the bit-parallel tile kernel (other
// byte values are detected and redone by the pixel kernel)
int amt_i_ccl_tileroots_u8(amt_ctx* ctx, const ccl_geom& g, const uint8_t* in, int* L, int* rootlist, int* nroots,
                           int* multi = nullptr);
// Run tables of a 0 / 1 (or truth-value) mask, per 64 x 64 tile t = (plane * tile_rows + tile_row) * segments + segment:
//   tbits[t * 64 + row]   the row's 64 pixels as a word (bit i = column i)
//   rtab[t * RT_CAP + k]  for the tile's k-th run in raster order: (row << 6 | column) of the first pixel of its TILE ROOT
//   nruns[t]              number of runs
// A pixel's run: runs of the rows above (prefix sum of the rows' head counts) + heads at or before it in its own row.
//   roff[t * 64 + row]    runs of the tile's rows above `row` (optional: random look-ups need it, tile-wide passes scan)
constexpr int RT_CAP = 2048;  // 64 rows x at most 32 runs
// What every run-table path asks of its mask: whole 16-byte groups of pixels per row and per plane, read aligned.  Each
// caller adds the alignment of its own planes and the limit of the int index it forms from ntiles.
static inline bool amt_i_ccl_runs_ok(const void* in, const ccl_geom& g) {
    return g.W % 16 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && g.n % 16 == 0;
}
// ... and of an operation that expands the tables into planes at `out`, 16 bytes per lane (amt_label, the component
// filters).  The limit keeps the row-word index t * 64 + row of tbits, and with it the tile count the expansion takes,
// inside an int
static inline bool amt_i_ccl_runs_out_ok(const void* in, const void* out, const ccl_geom& g) {
    return amt_i_ccl_runs_ok(in, g) && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && g.ntiles * 64 < 0x7fffffffull;
}
// The watershed's labelling of its mask from run tables alone: 4-connected components of the NON-ZERO bytes; L is written
// at the tile roots only (L[root] = root, then the seams' unions), the tile roots are listed as amt_i_ccl_tileroots_u8
// lists them
int amt_i_ccl_tileroots_runs_u8(amt_ctx* ctx, const ccl_geom& g, const uint8_t* in, int* L, int* rootlist, int* nroots,
                                unsigned long long* tbits, unsigned short* rtab, int* nruns, unsigned short* roff);
// what a kernel needs for random look-ups "pixel -> run -> component" (rcomp[t * RT_CAP + k] = the 1-based component id of
// run k, written by the watershed's statistics pass); tbits == nullptr: no run tables, the caller reads its parent plane
struct amt_runtabs {
    const unsigned long long* tbits;
    const unsigned short* roff;
    const unsigned short* rtab;
    const int* rcomp;
    int segs, trows;
};
// A[t] = A[L[t]] for every listed tile root t (lists compressed): a pixel then reaches its component's entry of A
// with one hop through its tile root
int amt_i_propagate_roots(amt_ctx* ctx, const ccl_geom& g, int* A, const int* L, const int* rootlist, const int* nroots);

// The component filters of nplanes truth-value masks (amt_binary_morph's AMT_MORPH_FILL_HOLES and
// AMT_MORPH_REMOVE_SMALL_OBJECTS / _HOLES, which checks the arguments).  With "component" the pixel's 4-connected (c8:
// 8-connected) component of its own polarity:
//   objects by area   out = in != 0 and the component has at least `size` pixels (size >= 1);
//   holes by area     out = in != 0, or the background component has fewer than `size` pixels (size >= 1);
//   holes by frame    scipy.ndimage.binary_fill_holes: out = in != 0, or the background component holds no pixel of the
//                     1-pixel frame (size must be 1).
// out must not alias in.
enum amt_comp_what { AMT_COMP_OBJECTS_BY_AREA, AMT_COMP_HOLES_BY_AREA, AMT_COMP_HOLES_BY_FRAME };
int amt_i_component_filter(amt_ctx* ctx, const uint8_t* in, uint8_t* out, int nplanes, int H, int W, bool c8,
                           amt_comp_what what, int size);

// ---- per-label operations: one wave per (label, plane) over the label's bounding box (amt_perlabel.h) ---------------
// The box pass (amt_props.hip): bbox[plane][label] = {miny, minx, maxy, maxx} of every label 1..max_label, maxy < miny
// for a label absent from its plane; acc (nullable) = the moment accumulators of amt_props.hip per (plane, label),
// cleared by the same launch
int amt_i_label_boxes(amt_ctx* ctx, const int* labels, int* bbox, unsigned long long* acc, int nplanes, int H, int W,
                      int max_label);
// the plane pass alone, over the planes whose flag in only_planes[] (device) is non-zero: their labels' extremes are
// folded into bbox by atomics, so bbox must hold empty boxes or parts of the true ones (amt_watershed.hip's fused tail)
int amt_i_label_boxes_flagged(amt_ctx* ctx, const int* labels, int* bbox, const int* only_planes, int nplanes, int H, int W,
                              int max_label);
// The table bits of amt_regionprops_ext, which checks the arguments and makes the bounding boxes; wtable[plane][label]
// [channel] holds four columns.  AMT_RPX_ROBUST (amt_robust.hip): {q25, median, q75, MAD} of the AMT_U16 / AMT_F64
// channel over the label
int amt_i_robust_intensity(amt_ctx* ctx, const int* labels, const int* bbox, const void* intensity, int in_code, int C,
                           double* wtable, int nplanes, int H, int W, int max_label);
// AMT_RPX_RELATE / AMT_RPX_NEIGHBORS (amt_relate.hip): the census of companion plane `comp[plane][channel]` under the
// label's pixels / on its ring; AMT_RPX_NEAREST: the two nearest labels by the centroids cen[plane][label] = (cy, cx),
// NaN for an absent label
int amt_i_relate_labels(amt_ctx* ctx, const int* labels, const int* bbox, const int* comp, int C, double* wtable,
                        int nplanes, int H, int W, int max_label);
int amt_i_neighbor_census(amt_ctx* ctx, const int* labels, const int* bbox, const int* comp, int C, double* wtable,
                          int nplanes, int H, int W, int max_label);
int amt_i_nearest_labels(amt_ctx* ctx, const double2* cen, double* wtable, int nplanes, int max_label);
// AMT_RPX_TEXTURE / AMT_RPX_TEXTURE_COUNTS (amt_texture.hip): a call of its own -- it checks its arguments and operands,
// makes the bounding boxes and fills out = the feature rows [plane][label][channel][direction][AMT_TEX_NCOLS] or, with
// `counts`, the uint32 matrices [plane][label][channel][direction][levels][levels] instead
int amt_i_texture(amt_ctx* ctx, const int32_t* labels, const void* intensity, int in_code, int C, const double* ranges,
                  int levels, int distance, bool counts, double* out, int nplanes, int H, int W, int max_label);
// AMT_RPX_RADIAL (amt_radial.hip): a call of its own, like texture -- geom = the rows [plane][label][AMT_RAD_GEOM_NCOLS]
// (radii and ring counts), out = [plane][label][channel][ring][AMT_RAD_NCOLS], absent (with intensity) when C == 0
int amt_i_radial(amt_ctx* ctx, const int32_t* labels, const void* intensity, int in_code, int C, int bins, double* geom,
                 double* out, int nplanes, int H, int W, int max_label);

// ---- grey reconstruction (amt_reconstruct.hip): ops AMT_RANK_RECONSTRUCT_DILATION .. AMT_RANK_HMIN_RECONSTRUCT of
// amt_rank_filter, which has checked the operands' aliasing; it checks everything else, refusing what needs no device
// before it looks at the context, and returns once `out` holds the reconstruction (it waits for the device)
int amt_i_reconstruct(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W,
                      const uint8_t* footprint, int fh, int fw, int op, double cval, const void* minuend);

// ---- per-cell skeletons: ops AMT_RANK_LABEL_SKELETON (amt_morph.hip, beside the binary thinning it shares its kernel
// with) and AMT_RANK_LABEL_CENSUS (amt_skelcensus.hip) of amt_rank_filter, which has checked the operands' aliasing; they
// check everything else, the refusals that need no device (amt_i_label_op_refusals: dtype, footprint, a negative `mode`,
// a minuend, the plane size) before they look at the context.  The skeleton waits for the device, the census does not.
int amt_i_label_op_refusals(const char* what, const char* mode_name, const void* in, void* out, int dtype, int nplanes,
                            int H, int W, const uint8_t* footprint, int fh, int fw, int mode, const void* minuend);
int amt_i_label_skeleton(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W,
                         const uint8_t* footprint, int fh, int fw, int max_iter, const void* minuend);
int amt_i_label_census(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W,
                       const uint8_t* footprint, int fh, int fw, int max_label, const void* minuend);

// ---- Z-stacks (amt_zstack.hip): ops AMT_RANK_Z_PROJECT .. AMT_RANK_Z_TAKE of amt_rank_filter, whose `mode` carries Z.
// amt_i_zstack_spans gives the byte lengths of the three operands for the aliasing check amt_rank_filter makes;
// amt_i_zstack checks everything else, the refusals that need no device (dtype, Z, footprint, minuend, sizes) before it
// looks at the context.  Asynchronous, no scratch.
void amt_i_zstack_spans(int op, int dtype, int nplanes, int H, int W, int Z, double cval, size_t* in_bytes, size_t* out_bytes,
                        size_t* minuend_bytes);
int amt_i_zstack(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W, const uint8_t* footprint,
                 int fh, int fw, int op, int Z, double cval, const void* minuend);

// ---- spot detection (amt_spots.hip): ops AMT_RANK_LOCAL_MAXIMA .. AMT_RANK_TAKE_AT of amt_rank_filter, whose `mode`
// carries the border width (op 15) or the capacity of a list of spots (ops 16 .. 18).  amt_i_spots_spans gives the byte
// lengths of the three operands for the aliasing check amt_rank_filter makes; amt_i_spots checks everything else, the
// refusals that need no device (dtype, footprint, mode, minuend, sizes) before it looks at the context.  Asynchronous;
// only the mask list reserves scratch (its per-row counts).
void amt_i_spots_spans(int op, int dtype, int nplanes, int H, int W, int mode, size_t* in_bytes, size_t* out_bytes,
                       size_t* minuend_bytes);
int amt_i_spots(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W, const uint8_t* footprint,
                int fh, int fw, int op, int mode, double cval, const void* minuend);

// runtime bool -> template argument: f(std::true_type) or f(std::false_type), for launches of <bool> kernel templates
template <typename F>
static inline void amt_with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

#ifdef __HIPCC__
// Lock-free union-find on an int array of parents (amt_label.hip's labelling, amt_edt.hip's peak markers): uf_* on a
// plane or list in HBM, lds_* on one in LDS.  The root of a set is its smallest index.
__device__ __forceinline__ int uf_find_volatile(int* L, int a) {
    int p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != a) {
        a = p;
        p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return a;
}

// union by minimum index (Komura-style): the larger root is redirected to the smaller one.
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
    while (true) {
        a = uf_find_volatile(L, a);
        b = uf_find_volatile(L, b);
        if (a == b) return;
        if (a < b) {
            int t = a;
            a = b;
            b = t;
        }
        // a > b: try to hang a below b
        int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;  // someone else moved a meanwhile; retry from there
    }
}

__device__ __forceinline__ int lds_find(int* S, int a) {
    int p = __hip_atomic_load(&S[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (p != a) {
        a = p;
        p = __hip_atomic_load(&S[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return a;
}

__device__ __forceinline__ void lds_union(int* S, int a, int b) {
    while (true) {
        a = lds_find(S, a);
        b = lds_find(S, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&S[a], b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ int ccl_wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}
// flat index (inside its plane) of the tile root of run k of tile (ty, bx)
__device__ __forceinline__ int ccl_rt_root(const unsigned short* __restrict__ rtab, size_t tile, int k, int ty, int bx,
                                           int W) {
    const int e = rtab[tile * RT_CAP + k];
    return (ty * 64 + (e >> 6)) * W + bx * 64 + (e & 63);
}
// run of pixel (y, x) of `plane`: its index into rtab / rcomp (tile * RT_CAP + ordinal), or -1 for a background pixel
__device__ __forceinline__ long long amt_rt_px_run(const amt_runtabs& rt, int plane, int y, int x) {
    const size_t t = ((size_t)plane * rt.trows + (y >> 6)) * rt.segs + (x >> 6);
    const int row = y & 63, col = x & 63;
    const unsigned long long w = rt.tbits[t * 64 + row];
    const int ro = rt.roff[t * 64 + row];
    if (!((w >> col) & 1ull)) return -1;
    return (long long)(t * RT_CAP) + ro + __popcll((w & ~(w << 1)) & ((2ull << col) - 1ull)) - 1;
}
// flat index (inside its plane) of the tile root of the run with table index ri (as amt_rt_px_run returns it)
__device__ __forceinline__ int amt_rt_run_root(const amt_runtabs& rt, long long ri, int W) {
    const size_t t = (size_t)ri / RT_CAP;
    const int e = rt.rtab[ri];
    const int bx = (int)(t % rt.segs), ty = (int)((t / rt.segs) % rt.trows);
    return (ty * 64 + (e >> 6)) * W + bx * 64 + (e & 63);
}
// Value of the neighbouring lane by DPP wave shift (a VALU move, no LDS crossbar as ds_bpermute needs): lane 0 of
// amt_lane_left / lane 63 of amt_lane_right receive 0, every caller masks those lanes itself.  All 64 lanes must be
// active (call from wave-uniform control flow only).
__device__ __forceinline__ int amt_lane_left(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int amt_lane_right(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false); }
__device__ __forceinline__ long long amt_lane_left(long long v) {
    const unsigned lo = (unsigned)amt_lane_left((int)(unsigned)v), hi = (unsigned)amt_lane_left((int)(v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long amt_lane_right(long long v) {
    const unsigned lo = (unsigned)amt_lane_right((int)(unsigned)v), hi = (unsigned)amt_lane_right((int)(v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
#endif
