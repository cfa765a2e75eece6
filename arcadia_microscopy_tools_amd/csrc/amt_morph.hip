// Binary morphology on uint8 0/1 masks: erode, dilate, and fused open / close; thinning to centre lines (skeletonize) and
// the neighbour classes of a skeleton's pixels further down.
//
// Semantics = skimage.morphology.binary_* (SK/morphology/binary.py:42,77,82-147), which call
// scipy.ndimage.binary_erosion(structure, border_value=True) and binary_dilation(structure):
//   erosion : out[p] = AND_{s in S} in[p + s]   (outside the image counts as `border_value`)
//   dilation: out[p] = OR_{s in S}  in[p - s]   (outside counts as `border_value`, 0 in skimage)
// S = the non-zero footprint cells as offsets from the centre.
//
// Layout: the mask is packed to one BIT per pixel (a wave ballot turns 64 consecutive pixels into one
// 64-bit word), the primitives run on the packed rows -- a footprint offset (dy, dx) is one funnel shift
// of (previous | current | next) word of row y + dy followed by an AND / OR, i.e. |S| word operations
// per 64 pixels -- and the result is unpacked to bytes.  The packed plane (H * ceil(W / 64) words; 512 KB
// at 2048^2) lives in L2, so an opening or closing costs one HBM read and one HBM write of the byte mask.
#include "amt_internal.h"

#include <cstdlib>
#include <vector>

typedef unsigned long long u64;
constexpr int MAX_OFFS = 1024;

constexpr int PACK_WORDS_PER_WAVE = 16;

// A wave packs PACK_WORDS_PER_WAVE consecutive words of the (row-major) packed plane: lane i tests pixel
// word * 64 + i of the word's row.  The word coordinates are wave-uniform and advance incrementally (no division per
// word); every load is UNCONDITIONAL from clamped coordinates and nothing is computed from a value next to its load,
// so all PACK_WORDS_PER_WAVE loads of a wave are in flight together (a test inside the bounds check would put a
// wait behind each load).  TEST(value) decides the bit.
template <typename T, typename TEST>
__device__ __forceinline__ void pack_words(const T* __restrict__ src, u64* __restrict__ dst, int H, int W, int WW,
                                           TEST test) {
    const int lane = threadIdx.x & 63;
    const unsigned nwords = (unsigned)H * (unsigned)WW;  // < 2^31: H, W <= 32768
    const unsigned w0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4u + (threadIdx.x >> 6)) * PACK_WORDS_PER_WAVE);
    if (w0 >= nwords) return;
    const int y0 = (int)(w0 / (unsigned)WW), wx0 = (int)(w0 - (unsigned)y0 * (unsigned)WW);
    T val[PACK_WORDS_PER_WAVE];
    {
        int y = y0, wx = wx0;
#pragma unroll
        for (int k = 0; k < PACK_WORDS_PER_WAVE; ++k) {
            const int yc = y < H ? y : H - 1;
            const int x = wx * 64 + lane;
            val[k] = src[(size_t)yc * W + (x < W ? x : W - 1)];
            if (++wx == WW) {
                wx = 0;
                ++y;
            }
        }
    }
    int y = y0, wx = wx0;
#pragma unroll
    for (int k = 0; k < PACK_WORDS_PER_WAVE; ++k) {
        const bool inside = y < H && wx * 64 + lane < W;  // beyond W: bit 0
        const u64 m = __ballot(inside && test(val[k]));
        if (lane == 0 && y < H) dst[w0 + k] = m;
        if (++wx == WW) {
            wx = 0;
            ++y;
        }
    }
}

__global__ void __launch_bounds__(256) pack_kernel(const uint8_t* __restrict__ in, u64* __restrict__ packed, int H,
                                                   int W, int WW) {
    const size_t plane = blockIdx.y;
    pack_words(in + plane * (size_t)H * W, packed + plane * (size_t)H * WW, H, W, WW,
               [](uint8_t v) { return v != 0; });
}

// same packing, fused with the comparison `in > thr[plane]` (R/operations.py:216): the byte mask of the
// threshold never exists
template <typename T>
__global__ void __launch_bounds__(256) pack_gt_kernel(const T* __restrict__ in, const double* __restrict__ thr,
                                                      u64* __restrict__ packed, int H, int W, int WW) {
    const size_t plane = blockIdx.y;
    const double t = thr[plane];
    pack_words(in + plane * (size_t)H * W, packed + plane * (size_t)H * WW, H, W, WW,
               [t](T v) { return (double)v > t; });
}

// `vals > thr[plane]` from the byte plane of 256-bin indices (amt_otsu_f64_bins): thr is the centre of bin k, so a sample
// of a higher bin is above it (>= that bin's lower edge > centre_k), one of a lower bin below it, and only a sample of
// bin k itself has to be looked at -- 1 byte per pixel instead of 8, plus the float64 values along the objects' rims.
// A thread owns 16 consecutive pixels (one 16-byte load), four threads make a 64-pixel word.  W % 64 == 0.
__global__ void __launch_bounds__(256) pack_bins_kernel(const uint8_t* __restrict__ bins, const double* __restrict__ vals,
                                                        const double* __restrict__ thr,
                                                        const double* __restrict__ thr_code, u64* __restrict__ packed,
                                                        size_t n) {
    const size_t plane = blockIdx.y;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;  // 16-pixel group of the plane
    if (q * 16 >= n) return;                                  // whole quads leave together (n % 64 == 0)
    const double t = thr[plane];
    const unsigned k = (unsigned)(thr_code[plane] * 0.5);
    const uint4 b16 = *reinterpret_cast<const uint4*>(bins + plane * n + q * 16);
    const unsigned wv[4] = {b16.x, b16.y, b16.z, b16.w};
    const double* v = vals + plane * n + q * 16;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const unsigned b = (wv[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        bool bit = b > k;
        if (b == k) bit = v[j] > t;
        m |= (bit ? 1u : 0u) << j;
    }
    const u64 m1 = (u64)(unsigned)__shfl_down((int)m, 1), m2 = (u64)(unsigned)__shfl_down((int)m, 2),
              m3 = (u64)(unsigned)__shfl_down((int)m, 3);
    if ((threadIdx.x & 3) == 0) packed[plane * (n / 64) + q / 4] = (u64)m | (m1 << 16) | (m2 << 32) | (m3 << 48);
}

// `in > thr[plane]` for uint16 planes (the 2-byte codes of amt_gaussian_otsu_codes) in the layout of pack_bins_kernel: a
// thread owns 16 consecutive pixels (two 16-byte loads), four threads make a 64-pixel word.  W % 64 == 0.  For an integer
// v the comparison (double)v > t is v > floor(t) (t >= 0), always true for t < 0, never for NaN.
__global__ void __launch_bounds__(256) pack_gt_u16x16_kernel(const uint16_t* __restrict__ in, const double* __restrict__ thr,
                                                             u64* __restrict__ packed, size_t n) {
    const size_t plane = blockIdx.y;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;  // 16-pixel group of the plane
    if (q * 16 >= n) return;                                  // whole quads leave together (n % 64 == 0)
    const double t = thr[plane];
    const int it = t < 0.0 ? -1 : (t < 65535.0 ? (int)t : 65535);  // NaN -> 65535: no uint16 is above it
    const uint4* src = reinterpret_cast<const uint4*>(in + plane * n + q * 16);
    const uint4 a = src[0], b = src[1];
    const unsigned wv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int v = (int)((wv[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
        m |= (v > it ? 1u : 0u) << j;
    }
    const u64 m1 = (u64)(unsigned)__shfl_down((int)m, 1), m2 = (u64)(unsigned)__shfl_down((int)m, 2),
              m3 = (u64)(unsigned)__shfl_down((int)m, 3);
    if ((threadIdx.x & 3) == 0) packed[plane * (n / 64) + q / 4] = (u64)m | (m1 << 16) | (m2 << 32) | (m3 << 48);
}

__device__ __forceinline__ unsigned spread4(unsigned nib) {
    return (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
}

__global__ void __launch_bounds__(256) unpack_kernel(const u64* __restrict__ packed, uint8_t* __restrict__ out, int H,
                                                     int W, int WW) {
    // one thread per 16 pixels of a row (one 16-byte store when W % 16 == 0)
    const size_t plane = blockIdx.y;
    const int per_row = (W + 15) / 16;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)H * per_row) return;
    const int y = (int)(q / per_row);
    const int x = (int)(q - (size_t)y * per_row) * 16;
    const u64 w = packed[(plane * H + y) * WW + (x >> 6)];
    const unsigned bits = (unsigned)(w >> (x & 63)) & 0xFFFFu;
    uint8_t* o = out + (plane * H + y) * W + x;
    if ((W & 15) == 0) {
        uint4 r;
        r.x = spread4(bits & 0xFu);
        r.y = spread4((bits >> 4) & 0xFu);
        r.z = spread4((bits >> 8) & 0xFu);
        r.w = spread4((bits >> 12) & 0xFu);
        *reinterpret_cast<uint4*>(o) = r;
    } else {
        for (int k = 0; k < 16 && x + k < W; ++k) o[k] = (bits >> k) & 1u;
    }
}

// bits of word `wx` of row y as the primitive sees them: outside the image = border (all ones / zeros),
// and the bits of the last word beyond W also read as border
__device__ __forceinline__ u64 row_word(const u64* __restrict__ rows, int y, int wx, int H, int WW, int W,
                                        u64 border) {
    if (y < 0 || y >= H || wx < 0 || wx >= WW) return border;
    u64 v = rows[(size_t)y * WW + wx];
    if (wx == WW - 1 && (W & 63)) {
        const u64 valid = (1ull << (W & 63)) - 1ull;
        v = (v & valid) | (border & ~valid);
    }
    return v;
}

// offsets are sorted by dy (row-major footprint scan), so the three words of a source row are loaded once
template <bool ERODE>
__global__ void __launch_bounds__(256) packed_prim_kernel(const u64* __restrict__ in, u64* __restrict__ out, int H,
                                                          int W, int WW, const int2* __restrict__ offs_g, int noffs,
                                                          int border_value) {
    __shared__ int2 offs[MAX_OFFS];
    for (int i = threadIdx.x; i < noffs; i += 256) offs[i] = offs_g[i];
    __syncthreads();
    const int wx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (wx >= WW || y >= H) return;
    const u64* rows = in + (size_t)blockIdx.z * H * WW;
    const u64 border = border_value ? ~0ull : 0ull;
    u64 acc = ERODE ? ~0ull : 0ull;
    int cur_dy = 0x7fffffff;
    u64 p = 0, c = 0, nx = 0;
    for (int k = 0; k < noffs; ++k) {
        // erosion reads in[p + s]; dilation reads in[p - s]
        const int dy = ERODE ? offs[k].y : -offs[k].y;
        const int dx = ERODE ? offs[k].x : -offs[k].x;
        if (dy != cur_dy) {
            cur_dy = dy;
            p = row_word(rows, y + dy, wx - 1, H, WW, W, border);
            c = row_word(rows, y + dy, wx, H, WW, W, border);
            nx = row_word(rows, y + dy, wx + 1, H, WW, W, border);
        }
        u64 v;
        if (dx == 0)
            v = c;
        else if (dx > 0)
            v = (c >> dx) | (nx << (64 - dx));  // pixel x + dx
        else
            v = (c << (-dx)) | (p >> (64 + dx));  // pixel x - |dx|
        acc = ERODE ? (acc & v) : (acc | v);
    }
    out[((size_t)blockIdx.z * H + y) * WW + wx] = acc;
}

static int build_offsets(const uint8_t* fp, int fh, int fw, int2* host, int* n) {
    AMT_REQUIRE(fp && fh >= 1 && fw >= 1 && (fh & 1) && (fw & 1),
                "footprint must have odd height and width (got %d x %d)", fh, fw);
    AMT_REQUIRE(fh <= 63 && fw <= 63, "footprint larger than 63 x 63 is not supported");
    int k = 0;
    for (int y = 0; y < fh; ++y)
        for (int x = 0; x < fw; ++x)
            if (fp[y * fw + x]) {
                AMT_REQUIRE(k < MAX_OFFS, "footprint has more than %d cells", MAX_OFFS);
                host[k].x = x - fw / 2;
                host[k].y = y - fh / 2;
                ++k;
            }
    AMT_REQUIRE(k > 0, "footprint is empty");
    *n = k;
    return AMT_OK;
}

// ---- skeletonize (AMT_MORPH_SKELETONIZE) and neighbour classes (AMT_MORPH_NEIGHBOR_CLASSES) ----------------------------
// Zhang and Suen's thinning, as include/amt_hip.h states it, on the packed plane.  A sub-iteration is a pure 3 x 3 boolean
// function of the plane before it: the eight neighbour words of a word come from the rows above and below and from funnel
// shifts with the adjacent words, B (set neighbours) from a bit-sliced adder, A (0 -> 1 transitions round the ring) from
// "at least one" / "at least two" of the eight transitions, the two products from ANDs -- a few dozen word operations per
// 64 pixels, no per-pixel branch.
//
// sk_block_kernel: a 256-thread workgroup owns a tile of SK_ROWS rows x SK_WORDS words.  It loads the tile with a halo of
// SK_T rows above and below and one word left and right into LDS and runs up to SK_T sub-iterations LDS -> LDS (two
// buffers).  After t sub-iterations only positions at least t pixels from the loaded edge are right, so sub-iteration t
// computes rows [t + 1, rows - t - 1) only and the tile itself is exact after SK_T.  Positions outside the image and the
// bits beyond W are loaded as 0, and a sub-iteration only clears bits, so they stay 0 without a fix-up per step; the
// physical padding of the LDS tile (one row / word on every side) is zeroed once and never written.
// Two packed planes in scratch are read and written in turns (a launch reads the halos its neighbours own, so it cannot
// update in place); every tile therefore stores its interior, changed or not.  What a launch changed is recorded per
// plane as a 64-bit mask: bit t is set when sub-iteration t cleared a pixel of some tile's interior.  The host finds the
// first iteration (bit pair) that cleared nothing in it -- the plane's iteration count -- and a plane whose mask came out
// 0 has both packed planes equal, so its tiles return at once in every later launch.
constexpr int SK_ROWS = AMT_SKELETON_TILE_ROWS, SK_WORDS = AMT_SKELETON_TILE_WORDS, SK_T = AMT_SKELETON_BLOCK_SUBITERS;
constexpr int SK_TR = SK_ROWS + 2 * SK_T;          // loaded rows
constexpr int SK_PW = SK_WORDS + 4;                // physical words per LDS row: tile, two halo words, two padding words
constexpr int SK_PHYS = (SK_TR + 2) * SK_PW;       // one LDS buffer
constexpr int SK_BATCH = 3;                        // most launches between two looks at the masks
static_assert(SK_T >= 2 && SK_T <= 64 && SK_T % 2 == 0, "the halo word holds 64 pixels, an iteration is two sub-iterations");
static_assert(SK_TR * (SK_WORDS + 2) < 2048 && SK_WORDS + 2 <= 34, "the row / column split by multiplication");
// The label variant (AMT_RANK_LABEL_SKELETON of amt_rank_filter) runs the same kernel on the mask labels != 0 with four
// constant LINK planes beside it, one bit per pixel: E / S / SE / SW(p) = "p carries a label and the pixel at (0, 1) /
// (1, 0) / (1, 1) / (1, -1) from p carries the same one".  A neighbour counts as set when its mask bit is set AND the link
// between the two pixels is: towards E, S, SE, SW that is the centre's own link word, towards W, N, NW, NE the
// neighbour's, shifted as the neighbour's mask word is.  Its LDS holds the two mask buffers and the four link tiles.
static_assert(AMT_LABEL_SKELETON_TILE_ROWS == SK_ROWS && AMT_LABEL_SKELETON_TILE_WORDS == SK_WORDS &&
              AMT_LABEL_SKELETON_BLOCK_SUBITERS == SK_T, "one kernel, one geometry: the label variant shares the binary one's");
constexpr int SK_NLINKS = 4;  // E, S, SE, SW, in this order in scratch and in LDS
static_assert((2 + SK_NLINKS) * SK_PHYS * 8 + 64 <= 160 * 1024 / 2, "two workgroups of the label variant per CU");

#define SK_L(c, p) (((c) << 1) | ((p) >> 63)) /* pixel x - 1 */
#define SK_R(c, n) (((c) >> 1) | ((n) << 63)) /* pixel x + 1 */

// the eight neighbour words P2 .. P9 of a word, in the header's order
struct sk_ring {
    u64 p2, p3, p4, p5, p6, p7, p8, p9;
};

// s = the word in an LDS mask buffer; the rows above / below are SK_PW words away
__device__ __forceinline__ sk_ring sk_ring_plain(const u64* s) {
    const u64 up = s[-SK_PW - 1], uc = s[-SK_PW], un = s[-SK_PW + 1], cp = s[-1], c = s[0], cn = s[1];
    const u64 dp = s[SK_PW - 1], dc = s[SK_PW], dn = s[SK_PW + 1];
    return {uc, SK_R(uc, un), SK_R(c, cn), SK_R(dc, dn), dc, SK_L(dc, dp), SK_L(c, cp), SK_L(uc, up)};
}

// the same with the links: k = the word's link tile E; S, SE, SW follow SK_PHYS words apart, laid out as the mask
__device__ __forceinline__ sk_ring sk_ring_linked(const u64* s, const u64* k) {
    const u64 *S = k + SK_PHYS, *SE = S + SK_PHYS, *SW = SE + SK_PHYS;
    const u64 c = s[0], cn = s[1], dp = s[SK_PW - 1], dc = s[SK_PW], dn = s[SK_PW + 1];
    const u64 uc = s[-SK_PW];
    sk_ring r;
    r.p4 = SK_R(c, cn) & k[0];
    r.p6 = dc & S[0];
    r.p5 = SK_R(dc, dn) & SE[0];
    r.p7 = SK_L(dc, dp) & SW[0];
    r.p8 = SK_L(c & k[0], s[-1] & k[-1]);
    r.p2 = uc & S[-SK_PW];
    r.p3 = SK_R(uc & SW[-SK_PW], s[-SK_PW + 1] & SW[-SK_PW + 1]);
    r.p9 = SK_L(uc & SE[-SK_PW], s[-SK_PW - 1] & SE[-SK_PW - 1]);
    return r;
}

// the pixels of word c that sub-iteration `second` clears, given its neighbour words
__device__ __forceinline__ u64 sk_cleared(const sk_ring& r, u64 c, bool second) {
    const u64 p2 = r.p2, p3 = r.p3, p4 = r.p4, p5 = r.p5, p6 = r.p6, p7 = r.p7, p8 = r.p8, p9 = r.p9;
    // B = p2 + .. + p9 as four bit planes b0..b3
    const u64 x1 = p2 ^ p3, s1 = x1 ^ p4, c1 = (p2 & p3) | (p4 & x1);
    const u64 x2 = p5 ^ p6, s2 = x2 ^ p7, c2 = (p5 & p6) | (p7 & x2);
    const u64 s3 = p8 ^ p9, c3 = p8 & p9;
    const u64 x4 = s1 ^ s2, b0 = x4 ^ s3, c4 = (s1 & s2) | (s3 & x4);
    const u64 x5 = c1 ^ c2, t = x5 ^ c3, d1 = (c1 & c2) | (c3 & x5);
    const u64 b1 = t ^ c4, d2 = t & c4;
    const u64 b2 = d1 ^ d2, b3 = d1 & d2;
    const u64 b_ok = (b1 | b2) & ~b3 & ~(b0 & b1 & b2);  // 2 <= B <= 6
    // A == 1: exactly one of the eight transitions ~P_i & P_{i+1}
    u64 one = ~p2 & p3, two = 0ull, tr;
    tr = ~p3 & p4, two |= one & tr, one |= tr;
    tr = ~p4 & p5, two |= one & tr, one |= tr;
    tr = ~p5 & p6, two |= one & tr, one |= tr;
    tr = ~p6 & p7, two |= one & tr, one |= tr;
    tr = ~p7 & p8, two |= one & tr, one |= tr;
    tr = ~p8 & p9, two |= one & tr, one |= tr;
    tr = ~p9 & p2, two |= one & tr, one |= tr;
    const u64 prod = second ? ((p2 & p4 & p8) | (p2 & p6 & p8)) : ((p2 & p4 & p6) | (p4 & p6 & p8));
    return c & b_ok & one & ~two & ~prod;
}

// prev / cur: this launch's and the one before's change masks, one word per plane.  LINKED: links = the four link planes
// of the whole batch, link_stride words apart (nullptr otherwise)
template <bool LINKED>
__global__ void __launch_bounds__(256) sk_block_kernel(const u64* __restrict__ src, u64* __restrict__ dst,
                                                       const u64* __restrict__ links, size_t link_stride, int H, int W,
                                                       int WW, int nsub, const u64* __restrict__ prev, u64* cur) {
    constexpr int NBUF = LINKED ? 2 + SK_NLINKS : 2;
    __shared__ u64 lds[NBUF * SK_PHYS];
    __shared__ u64 s_chg;
    const int plane = blockIdx.z;
    if (prev[plane] == 0ull) return;  // the launch before this one changed nothing in the plane: dst already equals src
    const int tid = threadIdx.x;
    const int wx0 = (int)blockIdx.x * SK_WORDS, y0 = (int)blockIdx.y * SK_ROWS;  // the tile's first word / row
    const int tww = (WW - wx0) < SK_WORDS ? (WW - wx0) : SK_WORDS;
    const int TW = tww + 2;
    const int y_top = y0 - SK_T, wx_left = wx0 - 1;
    const unsigned inv = ((1u << 20) + (unsigned)TW - 1u) / (unsigned)TW;  // idx / TW as a multiply
    for (int i = tid; i < NBUF * SK_PHYS; i += 256) lds[i] = 0ull;
    if (tid == 0) s_chg = 0ull;
    __syncthreads();
    u64* a = lds + SK_PW + 1;  // logical (row 0, word 0)
    u64* b = a + SK_PHYS;
    const u64* rows = src + (size_t)plane * H * WW;
    const u64 last_valid = (W & 63) ? (1ull << (W & 63)) - 1ull : ~0ull;
    int any = 0;
    for (int idx = tid; idx < SK_TR * TW; idx += 256) {
        const int r = (int)(((unsigned)idx * inv) >> 20), wc = idx - r * TW;
        const int y = y_top + r, wx = wx_left + wc;
        u64 v = 0ull;
        if (y >= 0 && y < H && wx >= 0 && wx < WW) {
            v = rows[(size_t)y * WW + wx];
            if (wx == WW - 1) v &= last_valid;
        }
        a[r * SK_PW + wc] = v;
        any |= v != 0ull;
    }
    u64 chg = 0ull;
    if (__syncthreads_or(any)) {
        if constexpr (LINKED) {
            // the links of the loaded region: constant through the launch; outside the image 0, and a link word is only
            // read ANDed with mask bits of its own plane position, which are 0 there too
            const u64* lrows = links + (size_t)plane * H * WW;
            for (int idx = tid; idx < SK_TR * TW; idx += 256) {
                const int r = (int)(((unsigned)idx * inv) >> 20), wc = idx - r * TW;
                const int y = y_top + r, wx = wx_left + wc;
                if (y >= 0 && y < H && wx >= 0 && wx < WW) {
                    const size_t at = (size_t)y * WW + wx;
#pragma unroll
                    for (int k = 0; k < SK_NLINKS; ++k) a[(2 + k) * SK_PHYS + r * SK_PW + wc] = lrows[k * link_stride + at];
                }
            }
            __syncthreads();
        }
        int clean = 0;
        for (int t = 0; t < nsub; ++t) {
            const int r_lo = t + 1, count = (SK_TR - 2 * (t + 1)) * TW;
            int step = 0;
            for (int idx = tid; idx < count; idx += 256) {
                const int rr = (int)(((unsigned)idx * inv) >> 20);
                const int r = r_lo + rr, wc = idx - rr * TW;
                const u64* s = a + r * SK_PW + wc;
                const u64 c = s[0];
                u64 v = c;
                if (c) {
                    if constexpr (LINKED) {
                        // a and b take turns: the link tiles lie 2 or 1 buffers behind the word
                        const u64* k = s + (a < b ? 2 * SK_PHYS : SK_PHYS);
                        v = c & ~sk_cleared(sk_ring_linked(s, k), c, t & 1);
                    } else {
                        v = c & ~sk_cleared(sk_ring_plain(s), c, t & 1);
                    }
                    if (v != c) {
                        step = 1;
                        if (r >= SK_T && r < SK_T + SK_ROWS && wc >= 1 && wc <= tww) chg |= 1ull << t;
                    }
                }
                b[r * SK_PW + wc] = v;
            }
            u64* sw = a;
            a = b;
            b = sw;
            // two sub-iterations in a row that cleared nothing: the next reads what the one before last read
            clean = __syncthreads_or(step) ? 0 : clean + 1;
            if (clean == 2) break;
        }
        if (chg) atomicOr(&s_chg, chg);
        __syncthreads();
    }
    u64* o = dst + (size_t)plane * H * WW;
    for (int idx = tid; idx < SK_ROWS * tww; idx += 256) {
        const int r = idx / tww, wc = idx - r * tww;
        const int y = y0 + r;
        if (y < H) o[(size_t)y * WW + wx0 + wc] = a[(SK_T + r) * SK_PW + 1 + wc];
    }
    if (tid == 0 && s_chg) atomicOr(cur + plane, s_chg);
}

// The label variant's way in: the mask labels != 0 and the four link planes (E, S, SE, SW, link_stride words apart) of an
// int32 label plane in one pass.  A wave makes LK_WORDS_PER_WAVE consecutive words of the packed plane, lane i the bit of
// pixel word * 64 + i: the pixel and its four partners are loaded UNCONDITIONALLY from clamped coordinates, all loads of
// the wave's words issued before the first ballot, and a partner outside the image is dropped where the bit is made.  Bits
// beyond W are 0 in all five planes.
constexpr int LK_WORDS_PER_WAVE = 4;
__global__ void __launch_bounds__(256) sk_pack_links_kernel(const int* __restrict__ labels, u64* __restrict__ mask,
                                                            u64* __restrict__ links, size_t link_stride, int H, int W,
                                                            int WW) {
    const size_t plane = blockIdx.y;
    const int* L = labels + plane * (size_t)H * W;
    u64* m = mask + plane * (size_t)H * WW;
    u64* k = links + plane * (size_t)H * WW;
    const int lane = threadIdx.x & 63;
    const unsigned nwords = (unsigned)H * (unsigned)WW;
    const unsigned w0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4u + (threadIdx.x >> 6)) * LK_WORDS_PER_WAVE);
    if (w0 >= nwords) return;
    const int y0 = (int)(w0 / (unsigned)WW), wx0 = (int)(w0 - (unsigned)y0 * (unsigned)WW);
    int v[LK_WORDS_PER_WAVE], e[LK_WORDS_PER_WAVE], s[LK_WORDS_PER_WAVE], se[LK_WORDS_PER_WAVE], sw[LK_WORDS_PER_WAVE];
    {
        int y = y0, wx = wx0;
#pragma unroll
        for (int j = 0; j < LK_WORDS_PER_WAVE; ++j) {
            const int yc = y < H ? y : H - 1, yd = yc + 1 < H ? yc + 1 : H - 1;
            const int x = wx * 64 + lane;
            const int xc = x < W ? x : W - 1, xr = xc + 1 < W ? xc + 1 : W - 1, xl = xc > 0 ? xc - 1 : 0;
            const int *rc = L + (size_t)yc * W, *rd = L + (size_t)yd * W;
            v[j] = rc[xc];
            e[j] = rc[xr];
            s[j] = rd[xc];
            se[j] = rd[xr];
            sw[j] = rd[xl];
            if (++wx == WW) {
                wx = 0;
                ++y;
            }
        }
    }
    int y = y0, wx = wx0;
#pragma unroll
    for (int j = 0; j < LK_WORDS_PER_WAVE; ++j) {
        const int x = wx * 64 + lane;
        const bool on = y < H && x < W && v[j] != 0;
        const bool below = y + 1 < H, right = x + 1 < W, left = x >= 1;
        const u64 bm = __ballot(on);
        const u64 be = __ballot(on && right && e[j] == v[j]);
        const u64 bs = __ballot(on && below && s[j] == v[j]);
        const u64 bse = __ballot(on && below && right && se[j] == v[j]);
        const u64 bsw = __ballot(on && below && left && sw[j] == v[j]);
        if (lane == 0 && y < H) {
            m[w0 + j] = bm;
            k[w0 + j] = be;
            k[link_stride + w0 + j] = bs;
            k[2 * link_stride + w0 + j] = bse;
            k[3 * link_stride + w0 + j] = bsw;
        }
        if (++wx == WW) {
            wx = 0;
            ++y;
        }
    }
}

// ... and its way out: out = labels where the bit is set, 0 elsewhere; one thread per four pixels of a row, a 16-byte
// load and store per lane where VEC (both planes 16-byte aligned and W % 4 == 0)
template <bool VEC>
__global__ void __launch_bounds__(256) sk_unpack_labels_kernel(const u64* __restrict__ packed, const int* __restrict__ labels,
                                                               int* __restrict__ out, int H, int W, int WW) {
    const size_t plane = blockIdx.y;
    const int per_row = (W + 3) / 4;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)H * per_row) return;
    const int y = (int)(q / per_row);
    const int x = (int)(q - (size_t)y * per_row) * 4;
    const u64 w = packed[(plane * H + y) * WW + (x >> 6)];
    const unsigned bits = (unsigned)(w >> (x & 63)) & 0xFu;  // x % 4 == 0: the four bits lie in one word
    const size_t at = (plane * H + y) * W + x;
    if constexpr (VEC) {
        const int4 l = *reinterpret_cast<const int4*>(labels + at);
        *reinterpret_cast<int4*>(out + at) = make_int4(l.x & -(int)(bits & 1u), l.y & -(int)((bits >> 1) & 1u),
                                                       l.z & -(int)((bits >> 2) & 1u), l.w & -(int)((bits >> 3) & 1u));
    } else {
        for (int j = 0; j < 4 && x + j < W; ++j) out[at + j] = labels[at + j] & -(int)((bits >> j) & 1u);
    }
}

// The driver of both variants.  LINKED: in / out are int32 label planes (amt_i_label_skeleton), otherwise uint8 masks.
template <bool LINKED>
static int sk_run(amt_ctx* ctx, const void* in, void* out, int nplanes, int H, int W, int max_iter) {
    const char* const name = LINKED ? "label_skeleton" : "skeletonize";
    const int WW = (W + 63) / 64;
    const size_t words = (size_t)nplanes * H * WW;
    const int ntx = (WW + SK_WORDS - 1) / SK_WORDS, nty = (H + SK_ROWS - 1) / SK_ROWS;
    AMT_REQUIRE(nplanes <= 65535, "%s: at most 65535 planes per call (got %d)", name, nplanes);
    amt_scratch s(ctx);
    amt_buf<u64> pa(s, words);
    amt_buf<u64> pb(s, words);
    amt_buf<u64> masks(s, (size_t)(SK_BATCH + 1) * nplanes);  // row 0: the launch before the batch; then one row per launch
    amt_buf<u64> links(s, SK_NLINKS * words, LINKED);
    AMT_TRY(s.commit());
    const size_t nwords = (size_t)H * WW;
    if constexpr (LINKED) {
        const unsigned gpack = (unsigned)((nwords + 4 * LK_WORDS_PER_WAVE - 1) / (4 * LK_WORDS_PER_WAVE));
        hipLaunchKernelGGL(sk_pack_links_kernel, dim3(gpack, nplanes), dim3(256), 0, ctx->stream, (const int*)in, (u64*)pa,
                           (u64*)links, words, H, W, WW);
    } else {
        const unsigned gpack = (unsigned)((nwords + 4 * PACK_WORDS_PER_WAVE - 1) / (4 * PACK_WORDS_PER_WAVE));
        hipLaunchKernelGGL(pack_kernel, dim3(gpack, nplanes), dim3(256), 0, ctx->stream, (const uint8_t*)in, pa, H, W, WW);
    }
    AMT_LAUNCH_CHECK();
    u64* const m = masks;
    const size_t row = sizeof(u64) * (size_t)nplanes;
    AMT_HIP_CHECK(hipMemsetAsync(m, 0xFF, row, ctx->stream));
    u64 *src = pa, *dst = pb;
    std::vector<u64> host((size_t)SK_BATCH * nplanes);
    std::vector<long long> iters((size_t)nplanes, -1);
    // a launch that is not clean clears at least one pixel
    const unsigned long long limit = (unsigned long long)H * W + 2;
    const long long budget = max_iter > 0 ? 2ll * max_iter : -1;  // sub-iterations; -1: to the fixed point
    long long done_sub = 0;
    unsigned long long launches = 0, syncs = 0;
    int open = nplanes;
    while (open > 0 && (budget < 0 || done_sub < budget)) {
        AMT_HIP_CHECK(hipMemsetAsync(m + nplanes, 0, row * SK_BATCH, ctx->stream));
        int n = 0, nsub[SK_BATCH];
        long long sub = done_sub;
        // 1, 2, then SK_BATCH launches between looks: most masks are done after one launch, deep ones after many
        const int batch = syncs + 1 < (unsigned long long)SK_BATCH ? (int)syncs + 1 : SK_BATCH;
        while (n < batch && (budget < 0 || sub < budget)) {
            nsub[n] = budget < 0 || budget - sub >= SK_T ? SK_T : (int)(budget - sub);
            hipLaunchKernelGGL(sk_block_kernel<LINKED>, dim3(ntx, nty, nplanes), dim3(256), 0, ctx->stream, src, dst,
                               (const u64*)links, words, H, W, WW, nsub[n], m + (size_t)n * nplanes,
                               m + (size_t)(n + 1) * nplanes);
            AMT_LAUNCH_CHECK();
            u64* sw = src;
            src = dst;
            dst = sw;
            sub += nsub[n++];
        }
        AMT_HIP_CHECK(hipMemcpyAsync(host.data(), m + nplanes, row * n, hipMemcpyDeviceToHost, ctx->stream));
        AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ++syncs;
        launches += n;
        for (int k = 0; k < n; ++k) {
            for (int p = 0; p < nplanes; ++p) {
                if (iters[p] >= 0) continue;
                const u64 bits = host[(size_t)k * nplanes + p];
                for (int i = 0; i < nsub[k] / 2; ++i)
                    if (((bits >> (2 * i)) & 3ull) == 0ull) {
                        iters[p] = done_sub / 2 + i + 1;
                        --open;
                        break;
                    }
            }
            done_sub += nsub[k];
        }
        if (launches > limit) {
            amt_set_error("%s did not converge in %llu launches", name, launches);
            return AMT_EHIP;
        }
        if (open > 0 && (budget < 0 || done_sub < budget))
            AMT_HIP_CHECK(hipMemcpyAsync(m, m + (size_t)n * nplanes, row, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if constexpr (LINKED) {
        const size_t nq = (size_t)H * ((W + 3) / 4);
        const dim3 grid((unsigned)((nq + 255) / 256), nplanes);
        if (W % 4 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0)
            hipLaunchKernelGGL(sk_unpack_labels_kernel<true>, grid, dim3(256), 0, ctx->stream, src, (const int*)in, (int*)out,
                               H, W, WW);
        else
            hipLaunchKernelGGL(sk_unpack_labels_kernel<false>, grid, dim3(256), 0, ctx->stream, src, (const int*)in,
                               (int*)out, H, W, WW);
    } else {
        const size_t nq = (size_t)H * ((W + 15) / 16);
        hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((nq + 255) / 256), nplanes), dim3(256), 0, ctx->stream, src,
                           (uint8_t*)out, H, W, WW);
    }
    AMT_LAUNCH_CHECK();
    AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ++syncs;
    // AMT_DEBUG_SKELETONIZE=1 (tools/time_skeletonize.py): how long the data made the call -- the iterations of the plane
    // that needed most (the one that cleared nothing included; max_iter where that came first), launches and host waits
    const char* report = getenv("AMT_DEBUG_SKELETONIZE");  // read per call: the op waits for the device anyway
    if (report && report[0] == '1') {
        long long most = 0;
        for (int p = 0; p < nplanes; ++p) {
            const long long it = iters[p] >= 0 ? iters[p] : (long long)max_iter;
            most = it > most ? it : most;
        }
        fprintf(stderr, "amt %s: iterations=%lld launches=%llu syncs=%llu\n", name, most, launches, syncs);
    }
    return AMT_OK;
}

// out = 0 where the pixel is clear, else 1 + its set neighbours (eight with `full`, the four edge neighbours otherwise).
// One thread per 16 pixels of a row, as unpack_kernel: the three rows' bits x - 1 .. x + 16 as 18-bit windows, the count
// as bit planes over the 16 pixels, spread to bytes.
__device__ __forceinline__ unsigned nc_window(const u64* __restrict__ rows, int y, int wx, int xs, int H, int WW, int W) {
    const u64 c = row_word(rows, y, wx, H, WW, W, 0ull);
    u64 v = xs ? c >> (xs - 1) : (c << 1) | (row_word(rows, y, wx - 1, H, WW, W, 0ull) >> 63);
    if (xs == 48) v = (v & 0x1FFFFull) | ((row_word(rows, y, wx + 1, H, WW, W, 0ull) & 1ull) << 17);
    return (unsigned)v & 0x3FFFFu;
}

__global__ void __launch_bounds__(256) neighbor_classes_kernel(const u64* __restrict__ packed, uint8_t* __restrict__ out,
                                                               int H, int W, int WW, int full) {
    const size_t plane = blockIdx.y;
    const int per_row = (W + 15) / 16;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)H * per_row) return;
    const int y = (int)(q / per_row);
    const int x = (int)(q - (size_t)y * per_row) * 16;
    const u64* rows = packed + plane * (size_t)H * WW;
    const unsigned wu = nc_window(rows, y - 1, x >> 6, x & 63, H, WW, W);
    const unsigned wc = nc_window(rows, y, x >> 6, x & 63, H, WW, W);
    const unsigned wd = nc_window(rows, y + 1, x >> 6, x & 63, H, WW, W);
    const unsigned corner = full ? 0xFFFFu : 0u;
    const unsigned p2 = (wu >> 1) & 0xFFFFu, p3 = (wu >> 2) & corner, p4 = (wc >> 2) & 0xFFFFu, p5 = (wd >> 2) & corner;
    const unsigned p6 = (wd >> 1) & 0xFFFFu, p7 = wd & corner, p8 = wc & 0xFFFFu, p9 = wu & corner;
    const unsigned centre = (wc >> 1) & 0xFFFFu;
    const unsigned x1 = p2 ^ p3, s1 = x1 ^ p4, c1 = (p2 & p3) | (p4 & x1);
    const unsigned x2 = p5 ^ p6, s2 = x2 ^ p7, c2 = (p5 & p6) | (p7 & x2);
    const unsigned s3 = p8 ^ p9, c3 = p8 & p9;
    const unsigned x4 = s1 ^ s2, b0 = x4 ^ s3, c4 = (s1 & s2) | (s3 & x4);
    const unsigned x5 = c1 ^ c2, t = x5 ^ c3, d1 = (c1 & c2) | (c3 & x5);
    const unsigned b1 = t ^ c4, d2 = t & c4;
    const unsigned b2 = d1 ^ d2, b3 = d1 & d2;
    unsigned r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sh = 4 * k;
        const unsigned on = spread4((centre >> sh) & 0xFu);  // 0 / 1 per byte
        const unsigned n = spread4((b0 >> sh) & 0xFu) | (spread4((b1 >> sh) & 0xFu) << 1) |
                           (spread4((b2 >> sh) & 0xFu) << 2) | (spread4((b3 >> sh) & 0xFu) << 3);
        r[k] = (n + on) & (on * 0xFFu);  // bytes of at most 9: no carry between them
    }
    uint8_t* o = out + (plane * H + y) * W + x;
    if ((W & 15) == 0) {
        *reinterpret_cast<uint4*>(o) = make_uint4(r[0], r[1], r[2], r[3]);
    } else {
        for (int k = 0; k < 16 && x + k < W; ++k) o[k] = (uint8_t)((r[k >> 2] >> (8 * (k & 3))) & 0xFFu);
    }
}

// pack, count: asynchronous
static int nc_run(amt_ctx* ctx, const uint8_t* in, uint8_t* out, int nplanes, int H, int W, int full) {
    AMT_REQUIRE(nplanes <= 65535, "neighbor_classes: at most 65535 planes per call (got %d)", nplanes);
    const int WW = (W + 63) / 64;
    amt_scratch s(ctx);
    amt_buf<u64> pa(s, (size_t)nplanes * H * WW);
    AMT_TRY(s.commit());
    const size_t nwords = (size_t)H * WW;
    const unsigned gpack = (unsigned)((nwords + 4 * PACK_WORDS_PER_WAVE - 1) / (4 * PACK_WORDS_PER_WAVE));
    hipLaunchKernelGGL(pack_kernel, dim3(gpack, nplanes), dim3(256), 0, ctx->stream, in, pa, H, W, WW);
    AMT_LAUNCH_CHECK();
    const size_t nq = (size_t)H * ((W + 15) / 16);
    hipLaunchKernelGGL(neighbor_classes_kernel, dim3((unsigned)((nq + 255) / 256), nplanes), dim3(256), 0, ctx->stream,
                       (const u64*)pa, out, H, W, WW, full);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// 0: neither, 1: the 3 x 3 cross, 2: 3 x 3 all-ones
static int structure3(const uint8_t* footprint, int fh, int fw) {
    if (!footprint || fh != 3 || fw != 3) return 0;
    bool cross = true, ones = true;
    for (int i = 0; i < 9; ++i) {
        const bool on = footprint[i] != 0, arm = (i & 1) || i == 4;
        if (on != arm) cross = false;
        if (!on) ones = false;
    }
    return ones ? 2 : cross ? 1 : 0;
}

// The refusals ops AMT_RANK_LABEL_SKELETON / AMT_RANK_LABEL_CENSUS of amt_rank_filter share, none of which needs a device:
// `what` = the op's name, `mode` = max_iter / max_label
int amt_i_label_op_refusals(const char* what, const char* mode_name, const void* in, void* out, int dtype, int nplanes,
                            int H, int W, const uint8_t* footprint, int fh, int fw, int mode, const void* minuend) {
    AMT_REQUIRE(in && out && nplanes >= 0 && H > 0 && W > 0, "rank_filter: %s: bad arguments", what);
    AMT_REQUIRE(dtype == AMT_I32, "rank_filter: %s: dtype must be AMT_I32 (a label plane), got %d", what, dtype);
    AMT_REQUIRE(structure3(footprint, fh, fw) == 2,
                "rank_filter: %s: the footprint must be 3 x 3 all-ones, the eight-neighbourhood the rule reads", what);
    AMT_REQUIRE(mode >= 0, "rank_filter: %s: %s (mode) must not be negative, got %d", what, mode_name, mode);
    AMT_REQUIRE(minuend == nullptr, "rank_filter: %s takes no minuend", what);
    AMT_REQUIRE((size_t)H * W < 0x7fffffffull, "rank_filter: %s: plane too large (H * W must be below 2^31 - 1)", what);
    AMT_REQUIRE(nplanes <= 65535, "rank_filter: %s: at most 65535 planes per call (got %d)", what, nplanes);
    return AMT_OK;
}

// AMT_RANK_LABEL_SKELETON: amt_rank_filter has checked the operands' aliasing; everything else is checked here
int amt_i_label_skeleton(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W,
                         const uint8_t* footprint, int fh, int fw, int max_iter, const void* minuend) {
    AMT_TRY(amt_i_label_op_refusals("label_skeleton", "max_iter", in, out, dtype, nplanes, H, W, footprint, fh, fw, max_iter,
                                    minuend));
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0) return AMT_OK;
    return sk_run<true>(ctx, in, out, nplanes, H, W, max_iter);
}

// op: AMT_MORPH_ERODE, AMT_MORPH_DILATE, AMT_MORPH_OPEN (erode then dilate), AMT_MORPH_CLOSE (dilate then erode),
// AMT_MORPH_FILL_HOLES, AMT_MORPH_REMOVE_SMALL_OBJECTS / _HOLES (amt_label.hip: amt_i_component_filter, the area
// filters' size in border_value), AMT_MORPH_SKELETONIZE (max_iter in border_value), AMT_MORPH_NEIGHBOR_CLASSES
extern "C" int amt_binary_morph(amt_ctx* ctx, const uint8_t* in, uint8_t* out, int nplanes, int H, int W,
                                const uint8_t* footprint, int fh, int fw, int op, int border_value) {
    // every op: a component filter's write-out of one plane would land in input still to be read, and erosion / dilation /
    // opening / closing are right in place only because the packed words happen to sit in scratch in between
    AMT_CHECK_OPERANDS("amt_binary_morph", amt_in("in", in, amt_span(1, nplanes, H, W)), amt_out("out", out, amt_span(1, nplanes, H, W)));
    // the refusals that need no device
    AMT_REQUIRE(op >= AMT_MORPH_ERODE && op <= AMT_MORPH_NEIGHBOR_CLASSES, "binary morphology: op must be 0..8, got %d", op);
    if (op == AMT_MORPH_SKELETONIZE) {
        AMT_REQUIRE(structure3(footprint, fh, fw) == 2,
                    "skeletonize: the footprint must be 3 x 3 all-ones, the eight-neighbourhood the rule reads");
        AMT_REQUIRE(border_value >= 0, "skeletonize: max_iter (border_value) must be 0 (no limit) or positive, got %d",
                    border_value);
    }
    if (op == AMT_MORPH_NEIGHBOR_CLASSES)
        AMT_REQUIRE(structure3(footprint, fh, fw) != 0,
                    "neighbor_classes: the footprint must be the 3 x 3 cross (four neighbours) or 3 x 3 all-ones (eight)");
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(in && out && nplanes >= 0 && H > 0 && W > 0, "binary morphology: bad arguments");
    if (op >= AMT_MORPH_SKELETONIZE) {
        AMT_REQUIRE((size_t)H * W < 0x7fffffffull, "%s: plane too large", op == AMT_MORPH_SKELETONIZE ? "skeletonize" : "neighbor_classes");
        if (nplanes == 0) return AMT_OK;
        if (op == AMT_MORPH_SKELETONIZE) return sk_run<false>(ctx, in, out, nplanes, H, W, border_value);
        return nc_run(ctx, in, out, nplanes, H, W, structure3(footprint, fh, fw) == 2 ? 1 : 0);
    }
    if (op >= AMT_MORPH_FILL_HOLES) {
        const bool fill = op == AMT_MORPH_FILL_HOLES;
        const char* name = fill ? "fill_holes" : op == AMT_MORPH_REMOVE_SMALL_OBJECTS ? "remove_small_objects" : "remove_small_holes";
        // the two structures for which scipy's propagation from outside the image is "background components that hold
        // no frame pixel": the 3 x 3 cross (4-connected background) and 3 x 3 all-ones (8-connected); the area filters
        // take their connectivity from the same two
        int cells = 0;
        bool cross = footprint && fh == 3 && fw == 3;
        if (cross)
            for (int k = 0; k < 9; ++k) {
                cells += footprint[k] != 0;
                if ((k & 1) == 0 && k != 4 && footprint[k]) cross = false;  // a corner
            }
        const bool full = footprint && fh == 3 && fw == 3 && cells == 9;
        cross = cross && cells == 5;
        AMT_REQUIRE(cross || full,
                    "%s: the structure must be the 3 x 3 cross (4-connected %s) or 3 x 3 all-ones "
                    "(8-connected %s)", name, fill ? "background" : "components", fill ? "background" : "components");
        AMT_REQUIRE(fill || border_value >= 1, "%s: the size (border_value) must be at least 1, got %d", name, border_value);
        if (nplanes == 0) return AMT_OK;
        const bool holes = op == AMT_MORPH_REMOVE_SMALL_HOLES;
        const amt_comp_what what = fill ? AMT_COMP_HOLES_BY_FRAME : holes ? AMT_COMP_HOLES_BY_AREA : AMT_COMP_OBJECTS_BY_AREA;
        return amt_i_component_filter(ctx, in, out, nplanes, H, W, full, what, fill ? 1 : border_value);
    }
    static thread_local int2 host[MAX_OFFS];
    int noffs = 0;
    AMT_TRY(build_offsets(footprint, fh, fw, host, &noffs));
    if (nplanes == 0) return AMT_OK;
    const int WW = (W + 63) / 64;
    const size_t words = (size_t)nplanes * H * WW;
    amt_scratch s(ctx);
    amt_buf<int2> offs(s, noffs);
    amt_buf<u64> pa(s, words);
    amt_buf<u64> pb(s, words);
    AMT_TRY(s.commit());
    AMT_TRY(amt_param_upload(ctx, offs, host, sizeof(int2) * noffs));
    const size_t nwords = (size_t)H * WW;
    const unsigned gpack = (unsigned)((nwords + 4 * PACK_WORDS_PER_WAVE - 1) / (4 * PACK_WORDS_PER_WAVE));
    hipLaunchKernelGGL(pack_kernel, dim3(gpack, nplanes), dim3(256), 0, ctx->stream, in, pa, H, W, WW);
    AMT_LAUNCH_CHECK();
    dim3 gp((WW + 63) / 64, (H + 3) / 4, nplanes);
    u64* result = pb;
    switch (op) {
        case AMT_MORPH_ERODE:
            hipLaunchKernelGGL((packed_prim_kernel<true>), gp, dim3(256), 0, ctx->stream, pa, pb, H, W, WW, offs, noffs,
                               border_value);
            break;
        case AMT_MORPH_DILATE:
            hipLaunchKernelGGL((packed_prim_kernel<false>), gp, dim3(256), 0, ctx->stream, pa, pb, H, W, WW, offs, noffs,
                               border_value);
            break;
        case AMT_MORPH_OPEN:  // skimage: erosion sees outside = 1, dilation sees outside = 0
            hipLaunchKernelGGL((packed_prim_kernel<true>), gp, dim3(256), 0, ctx->stream, pa, pb, H, W, WW, offs, noffs, 1);
            AMT_LAUNCH_CHECK();
            hipLaunchKernelGGL((packed_prim_kernel<false>), gp, dim3(256), 0, ctx->stream, pb, pa, H, W, WW, offs, noffs,
                               0);
            result = pa;
            break;
        default:  // AMT_MORPH_CLOSE
            hipLaunchKernelGGL((packed_prim_kernel<false>), gp, dim3(256), 0, ctx->stream, pa, pb, H, W, WW, offs, noffs,
                               0);
            AMT_LAUNCH_CHECK();
            hipLaunchKernelGGL((packed_prim_kernel<true>), gp, dim3(256), 0, ctx->stream, pb, pa, H, W, WW, offs, noffs, 1);
            result = pa;
            break;
    }
    AMT_LAUNCH_CHECK();
    const size_t nq = (size_t)H * ((W + 15) / 16);
    hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((nq + 255) / 256), nplanes), dim3(256), 0, ctx->stream, result, out,
                       H, W, WW);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- fused threshold -> opening -> closing ---------------------------------------------------------
// `binary_closing(binary_opening(in > thr))` (the Gaussian -> Otsu -> '>' -> open -> close mask chain of
// BASELINE configs[1]/[2]) in two kernels:
//   pack_gt_kernel      streams the image once and leaves one BIT per pixel (high occupancy, HBM-bound);
//   toc_fused_kernel    a block owns a band of TOC_BR rows x up to TOC_TWW words (64 px each): it copies the band
//                       plus a halo of 4 * ry rows (and one halo word left / right) of the packed plane (L2-resident,
//                       1/64 of the image) into LDS, runs erosion, dilation, dilation, erosion LDS -> LDS, and
//                       unpacks the band to bytes -- the only other HBM traffic of the chain.
// Positions outside the IMAGE read as each primitive's own border value (scipy's border_value: 1 for erosion,
// 0 for dilation); positions outside the TILE also read as border, which only corrupts halo words that the band
// never uses.
constexpr int TOC_BR = 32, TOC_TWW = 32, TOC_MAX_OFFS = 256;

// The LDS tile is physically padded by PADR rows above / below and one word left / right that are never
// written, so the primitives need no tile-bound checks; the border substitution for positions outside the
// image (and for the bits of the last word beyond W) is done when a word is WRITTEN, with the border value
// of the primitive that will read it next.
struct toc_tile {
    int TR, TW;          // tile rows / words per tile row (logical)
    int PW;              // physical words per row = TW + 2
    int y_top, wx_left;  // image row of tile row 0, image word of tile column 0
    int H, W, WW;
};
constexpr int TOC_PADR = 4;  // >= ry of the fused path (4 * ry <= 16)

__device__ __forceinline__ u64 toc_fix(const toc_tile& t, int r, int wc, u64 v, u64 next_border) {
    const int y = t.y_top + r, wx = t.wx_left + wc;
    if (y < 0 || y >= t.H || wx < 0 || wx >= t.WW) return next_border;
    if (wx == t.WW - 1 && (t.W & 63)) {
        const u64 valid = (1ull << (t.W & 63)) - 1ull;
        v = (v & valid) | (next_border & ~valid);
    }
    return v;
}

// buf points at logical (row 0, word 0); rows are PW words apart.  Only tile rows [r_lo, r_hi) are produced: each
// primitive of the chain needs ry fewer rows on either side than the one before it.  `inv` = ceil(2^20 / TW) turns
// the row / column split of the flat index into a multiply (exact for idx < 2^11, TW <= 34).
// DISK2: the footprint is disk(2) (the 13 cells |dy| + |dx| <= 2), unrolled with constant shifts; otherwise the
// generic offset list is walked.
template <bool ERODE, bool DISK2>
__device__ __forceinline__ void toc_prim(const u64* src, u64* dst, const toc_tile& t, const int2* offs, int noffs,
                                         u64 next_border, int r_lo, int r_hi, unsigned inv) {
    const int count = (r_hi - r_lo) * t.TW;
    for (int idx = threadIdx.x; idx < count; idx += 256) {
        const int rr = (int)(((unsigned)idx * inv) >> 20);
        const int r = r_lo + rr, wc = idx - rr * t.TW;
        u64 acc;
        if (DISK2) {
            const u64* s0 = src + r * t.PW + wc;
            const u64 a2 = s0[-2 * t.PW], b2 = s0[2 * t.PW];
            const u64 ap = s0[-t.PW - 1], ac = s0[-t.PW], an = s0[-t.PW + 1];
            const u64 cp = s0[-1], cc = s0[0], cn = s0[1];
            const u64 bp = s0[t.PW - 1], bc = s0[t.PW], bn = s0[t.PW + 1];
#define TOC_L(c, p, d) (((c) << (d)) | ((p) >> (64 - (d))))  /* pixel x - d */
#define TOC_R(c, n, d) (((c) >> (d)) | ((n) << (64 - (d))))  /* pixel x + d */
            if (ERODE) {
                acc = a2 & b2 & ac & TOC_L(ac, ap, 1) & TOC_R(ac, an, 1) & bc & TOC_L(bc, bp, 1) & TOC_R(bc, bn, 1) &
                      cc & TOC_L(cc, cp, 1) & TOC_R(cc, cn, 1) & TOC_L(cc, cp, 2) & TOC_R(cc, cn, 2);
            } else {
                acc = a2 | b2 | ac | TOC_L(ac, ap, 1) | TOC_R(ac, an, 1) | bc | TOC_L(bc, bp, 1) | TOC_R(bc, bn, 1) |
                      cc | TOC_L(cc, cp, 1) | TOC_R(cc, cn, 1) | TOC_L(cc, cp, 2) | TOC_R(cc, cn, 2);
            }
#undef TOC_L
#undef TOC_R
        } else {
            acc = ERODE ? ~0ull : 0ull;
            int cur_dy = 0x7fffffff;
            u64 p = 0, c = 0, nx = 0;
            for (int k = 0; k < noffs; ++k) {
                const int dy = ERODE ? offs[k].y : -offs[k].y;
                const int dx = ERODE ? offs[k].x : -offs[k].x;
                if (dy != cur_dy) {
                    cur_dy = dy;
                    const u64* row = src + (r + dy) * t.PW + wc;
                    p = row[-1];
                    c = row[0];
                    nx = row[1];
                }
                u64 v;
                if (dx == 0)
                    v = c;
                else if (dx > 0)
                    v = (c >> dx) | (nx << (64 - dx));
                else
                    v = (c << (-dx)) | (p >> (64 + dx));
                acc = ERODE ? (acc & v) : (acc | v);
            }
        }
        dst[r * t.PW + wc] = toc_fix(t, r, wc, acc, next_border);
    }
}

template <bool DISK2>
__global__ void __launch_bounds__(256) toc_fused_kernel(const u64* __restrict__ packed, uint8_t* __restrict__ out,
                                                        int H, int W, int WW, const int2* __restrict__ offs_g,
                                                        int noffs, int HY) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int2 offs[TOC_MAX_OFFS];
    const int tww = (WW - (int)blockIdx.x * TOC_TWW) < TOC_TWW ? (WW - (int)blockIdx.x * TOC_TWW) : TOC_TWW;
    toc_tile t;
    t.TR = TOC_BR + 2 * HY;
    t.TW = tww + 2;
    t.PW = t.TW + 2;
    t.y_top = (int)blockIdx.y * TOC_BR - HY;
    t.wx_left = (int)blockIdx.x * TOC_TWW - 1;
    t.H = H;
    t.W = W;
    t.WW = WW;
    const int phys = (t.TR + 2 * TOC_PADR) * t.PW;
    u64* physA = reinterpret_cast<u64*>(smem_raw);
    u64* physB = physA + phys;
    u64* bufA = physA + TOC_PADR * t.PW + 1;
    u64* bufB = physB + TOC_PADR * t.PW + 1;
    for (int i = threadIdx.x; i < noffs; i += 256) offs[i] = offs_g[i];
    for (int i = threadIdx.x; i < 2 * phys; i += 256) physA[i] = 0ull;  // padding is never written again
    __syncthreads();
    const size_t plane = blockIdx.z;
    const u64* src = packed + plane * (size_t)H * WW;
    // ---- 1. copy the packed band + halo (outside the image: erosion's border, all ones) ----
    const unsigned inv_tw = ((1u << 20) + (unsigned)t.TW - 1u) / (unsigned)t.TW;  // idx / TW as a multiply (idx < 2^11)
    for (int idx = threadIdx.x; idx < t.TR * t.TW; idx += 256) {
        const int r = (int)(((unsigned)idx * inv_tw) >> 20), wc = idx - r * t.TW;
        const int y = t.y_top + r, wx = t.wx_left + wc;
        const u64 v = (y >= 0 && y < H && wx >= 0 && wx < WW) ? src[(size_t)y * WW + wx] : 0ull;
        bufA[r * t.PW + wc] = toc_fix(t, r, wc, v, ~0ull);
    }
    __syncthreads();
    // ---- 2. opening = erosion, dilation; closing = dilation, erosion (skimage: erosion sees outside = 1,
    //         dilation sees outside = 0) ----
    const int ry = HY / 4;
    const unsigned inv = inv_tw;
    toc_prim<true, DISK2>(bufA, bufB, t, offs, noffs, 0ull, ry, t.TR - ry, inv);
    __syncthreads();
    toc_prim<false, DISK2>(bufB, bufA, t, offs, noffs, 0ull, 2 * ry, t.TR - 2 * ry, inv);
    __syncthreads();
    toc_prim<false, DISK2>(bufA, bufB, t, offs, noffs, ~0ull, 3 * ry, t.TR - 3 * ry, inv);
    __syncthreads();
    toc_prim<true, DISK2>(bufB, bufA, t, offs, noffs, 0ull, 4 * ry, t.TR - 4 * ry, inv);
    __syncthreads();
    // ---- 3. unpack the band: 16 pixels per thread and step ----
    const int per_row = tww * 4;
    const unsigned inv_pr = ((1u << 20) + (unsigned)per_row - 1u) / (unsigned)per_row;  // q < 2^12, per_row <= 128
    for (int q = threadIdx.x; q < TOC_BR * per_row; q += 256) {
        const int r = (int)(((unsigned)q * inv_pr) >> 20), rem = q - r * per_row;
        const int wc = rem >> 2, part = rem & 3;
        const int y = (int)blockIdx.y * TOC_BR + r;
        const int x = ((int)blockIdx.x * TOC_TWW + wc) * 64 + part * 16;
        if (y >= H || x >= W) continue;
        const u64 w = bufA[(HY + r) * t.PW + 1 + wc];
        const unsigned bits = (unsigned)(w >> (part * 16)) & 0xFFFFu;
        uint8_t* o = out + (plane * H + y) * W + x;
        if (x + 15 < W && ((reinterpret_cast<uintptr_t>(o) & 15) == 0)) {
            uint4 rr;
            rr.x = spread4(bits & 0xFu);
            rr.y = spread4((bits >> 4) & 0xFu);
            rr.z = spread4((bits >> 8) & 0xFu);
            rr.w = spread4((bits >> 12) & 0xFu);
            *reinterpret_cast<uint4*>(o) = rr;
        } else {
            for (int k = 0; k < 16 && x + k < W; ++k) o[k] = (bits >> k) & 1u;
        }
    }
}

// `binary_closing(binary_opening(in > thr))` in one packed chain: compare -> 4 word-level primitives ->
// unpack (the Gaussian -> Otsu -> '>' -> open -> close mask chain of BASELINE configs[1]/[2]).
// bins / thr_code_dev (both or neither, float64 input only): the byte plane of bin indices and the threshold's bin that
// amt_otsu_f64_bins made -- the comparison reads the float64 value only inside that bin.
extern "C" int amt_threshold_open_close(amt_ctx* ctx, const void* in, int in_dtype, const double* thr_dev, uint8_t* out,
                                        int nplanes, int H, int W, const uint8_t* footprint, int fh, int fw,
                                        const uint8_t* bins, const double* thr_code_dev) {
    AMT_REQUIRE(!bins == !thr_code_dev, "threshold_open_close: the bin plane and the threshold's bin go together");
    AMT_REQUIRE(!bins || in_dtype == AMT_F64, "threshold_open_close: a bin plane requires AMT_F64 input");
    AMT_CHECK_OPERANDS("amt_threshold_open_close", amt_in("in", in, amt_span(amt_esize(in_dtype), nplanes, H, W)),
                       amt_in("thr_dev", thr_dev, amt_span(8, nplanes)), amt_out("out", out, amt_span(1, nplanes, H, W)),
                       amt_in("bins", bins, amt_span(1, nplanes, H, W)), amt_in("thr_code_dev", thr_code_dev, amt_span(8, nplanes)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(in && thr_dev && out && nplanes >= 0 && H > 0 && W > 0, "threshold_open_close: bad arguments");
    AMT_REQUIRE(in_dtype == AMT_U16 || in_dtype == AMT_F64, "threshold_open_close: dtype must be AMT_U16 or AMT_F64");
    static thread_local int2 host[MAX_OFFS];
    int noffs = 0;
    AMT_TRY(build_offsets(footprint, fh, fw, host, &noffs));
    if (nplanes == 0) return AMT_OK;
    const int WW = (W + 63) / 64;
    const size_t words = (size_t)nplanes * H * WW;
    const int ry = fh / 2, rx = fw / 2;
    if (noffs <= TOC_MAX_OFFS && 4 * ry <= 16 && 4 * rx <= 64) {
        // single fused kernel: halo of 4 * ry rows and one 64-pixel word per side covers the four primitives
        amt_scratch s(ctx);
        amt_buf<int2> offs(s, noffs);
        amt_buf<u64> pa(s, words);
        AMT_TRY(s.commit());
        AMT_TRY(amt_param_upload(ctx, offs, host, sizeof(int2) * noffs));
        const size_t nwords = (size_t)H * WW;
        const unsigned gpack = (unsigned)((nwords + 4 * PACK_WORDS_PER_WAVE - 1) / (4 * PACK_WORDS_PER_WAVE));
        const size_t npx = (size_t)H * W;
        if (bins && (W & 63) == 0 && ((reinterpret_cast<uintptr_t>(bins) | npx) & 15) == 0)
            hipLaunchKernelGGL(pack_bins_kernel, dim3((unsigned)((npx / 16 + 255) / 256), nplanes), dim3(256), 0, ctx->stream,
                               bins, (const double*)in, thr_dev, thr_code_dev, pa, npx);
        else if (in_dtype == AMT_F64)
            hipLaunchKernelGGL((pack_gt_kernel<double>), dim3(gpack, nplanes), dim3(256), 0, ctx->stream,
                               (const double*)in, thr_dev, pa, H, W, WW);
        else if ((W & 63) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0)
            hipLaunchKernelGGL(pack_gt_u16x16_kernel, dim3((unsigned)((npx / 16 + 255) / 256), nplanes), dim3(256), 0,
                               ctx->stream, (const uint16_t*)in, thr_dev, pa, npx);
        else
            hipLaunchKernelGGL((pack_gt_kernel<uint16_t>), dim3(gpack, nplanes), dim3(256), 0, ctx->stream,
                               (const uint16_t*)in, thr_dev, pa, H, W, WW);
        AMT_LAUNCH_CHECK();
        const int HY = 4 * ry;
        const int tww = WW < TOC_TWW ? WW : TOC_TWW;
        const size_t smem = (size_t)2 * (TOC_BR + 2 * HY + 2 * TOC_PADR) * (tww + 4) * sizeof(u64);
        dim3 grid((WW + TOC_TWW - 1) / TOC_TWW, (H + TOC_BR - 1) / TOC_BR, nplanes);
        bool disk2 = fh == 5 && fw == 5 && noffs == 13;  // disk(2): the 13 cells with |dy| + |dx| <= 2
        for (int k = 0; k < noffs && disk2; ++k)
            disk2 = (host[k].x < 0 ? -host[k].x : host[k].x) + (host[k].y < 0 ? -host[k].y : host[k].y) <= 2;
        if (disk2)
            hipLaunchKernelGGL(toc_fused_kernel<true>, grid, dim3(256), smem, ctx->stream, pa, out, H, W, WW, offs,
                               noffs, HY);
        else
            hipLaunchKernelGGL(toc_fused_kernel<false>, grid, dim3(256), smem, ctx->stream, pa, out, H, W, WW, offs,
                               noffs, HY);
        AMT_LAUNCH_CHECK();
        return AMT_OK;
    }
    amt_scratch s(ctx);
    amt_buf<int2> offs(s, noffs);
    amt_buf<u64> pa(s, words);
    amt_buf<u64> pb(s, words);
    AMT_TRY(s.commit());
    AMT_TRY(amt_param_upload(ctx, offs, host, sizeof(int2) * noffs));
    const size_t nwords = (size_t)H * WW;
    const unsigned gpack = (unsigned)((nwords + 4 * PACK_WORDS_PER_WAVE - 1) / (4 * PACK_WORDS_PER_WAVE));
    if (in_dtype == AMT_F64)
        hipLaunchKernelGGL((pack_gt_kernel<double>), dim3(gpack, nplanes), dim3(256), 0, ctx->stream, (const double*)in,
                           thr_dev, pa, H, W, WW);
    else
        hipLaunchKernelGGL((pack_gt_kernel<uint16_t>), dim3(gpack, nplanes), dim3(256), 0, ctx->stream,
                           (const uint16_t*)in, thr_dev, pa, H, W, WW);
    AMT_LAUNCH_CHECK();
    dim3 gp((WW + 63) / 64, (H + 3) / 4, nplanes);
    // opening: erosion (outside = 1) then dilation (outside = 0); closing: dilation then erosion
    hipLaunchKernelGGL((packed_prim_kernel<true>), gp, dim3(256), 0, ctx->stream, pa, pb, H, W, WW, offs, noffs, 1);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL((packed_prim_kernel<false>), gp, dim3(256), 0, ctx->stream, pb, pa, H, W, WW, offs, noffs, 0);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL((packed_prim_kernel<false>), gp, dim3(256), 0, ctx->stream, pa, pb, H, W, WW, offs, noffs, 0);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL((packed_prim_kernel<true>), gp, dim3(256), 0, ctx->stream, pb, pa, H, W, WW, offs, noffs, 1);
    AMT_LAUNCH_CHECK();
    const size_t nq = (size_t)H * ((W + 15) / 16);
    hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((nq + 255) / 256), nplanes), dim3(256), 0, ctx->stream, pa, out, H,
                       W, WW);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
