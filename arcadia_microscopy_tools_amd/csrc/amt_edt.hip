// Exact Euclidean distance transform, the peak mask of the config-3 marker recipe, and the markers labelled from the list of
// the peaks that the search found (amt_peak_markers, at the end of the file).
//
// scipy.ndimage.distance_transform_edt(mask) == sqrt(float64(d2)) bitwise, with d2 the exact integer
// squared distance to the nearest zero pixel.  d2 is computed separably:
//   rows   : g(y,x) = distance to the nearest zero pixel in row y (G_INF if none).  The mask is packed into
//            64-pixel bit words of "zero" flags; the nearest zero on either side of a pixel is a clz / ffs on its
//            own word, walking to further words only across solid 64-pixel stretches.  g fits uint16 (sides are
//            <= 32768).
//   columns: d2(y,x) = min_k (k^2 + g(y+-k,x)^2), scanning k outward while k^2 < best.  A block computes the g
//            of 64 columns x (64 + 2*16) or (32 + 2*24) rows into LDS; only searches deeper than the halo continue,
//            with g evaluated from the words.
// Both searches are exact and cost O(distance) per pixel, which is what nuclei-sized objects need; they
// degrade (never fail) on very large solid regions.
#include "amt_internal.h"

constexpr unsigned G_INF = 0xFFFFu;  // no zero pixel in this row
// column tiles: 64 rows + 2 x 16 halo rows for batches (least staging per output row), 32 + 2 x 24 when a call
// has too few tiles to fill the chip (single planes)

// ---- both passes in one kernel, from a packed plane of zero flags (round 3) -------------------------------------------
// A separate row pass would write g as uint16 (2 bytes per pixel) and the column pass read it back with its halo (3): more
// traffic than the mask (1) and the result (4) together; that two-pass variant was measured and removed.  g is a function
// of the row's ZERO FLAGS alone, and those are one bit per pixel: edt_zero_words_kernel packs them (64 pixels per word,
// 1/8 byte per pixel), and a column tile computes the g of its 64 x (ROWS + 2 HALO) window itself -- three words per row
// (its own segment and the ones left / right of it) sit in LDS, a thread owns 8 consecutive pixels of a row, and only a
// row without a zero pixel within 64 columns walks further words in global memory.  Searches deeper than the halo
// evaluate g(y +- k, x) from the words too.
__global__ void __launch_bounds__(256) edt_zero_words_kernel(const uint8_t* __restrict__ mask, unsigned long long* __restrict__ zw,
                                                             int H, int W, int WW, size_t nwords, int fast) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nwords) return;
    const int wi = (int)(i % WW);
    const size_t row = i / WW;  // plane * H + y
    const uint8_t* p = mask + row * W + (size_t)wi * 64;
    const int valid = W - wi * 64 < 64 ? W - wi * 64 : 64;
    unsigned long long z = 0;
    if (fast) {  // W % 16 == 0 and a 16-byte aligned plane: 16-byte loads
        uint4 q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = *reinterpret_cast<const uint4*>(p + (16 * j < valid ? 16 * j : 0));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned v[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
            unsigned sixteen = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned nz = ((((v[k] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v[k]) >> 7) & 0x01010101u;  // byte != 0
                sixteen |= (((nz ^ 0x01010101u) * 0x01020408u) >> 24) << (4 * k);                          // byte i == 0 -> bit i
            }
            if (16 * j < valid) z |= (unsigned long long)(sixteen & 0xFFFFu) << (16 * j);
        }
    } else {
        for (int k = 0; k < valid; ++k) z |= (unsigned long long)(p[k] == 0) << k;
    }
    zw[i] = z;  // pixels beyond W: "not zero"
}

// distance of (y, x) to the nearest zero pixel of row y (G_INF if the row has none), from the row's zero-flag words
__device__ __forceinline__ unsigned edt_g_at(const unsigned long long* __restrict__ zr, int WW, int x) {
    const int wi = x >> 6, bit = x & 63;
    const unsigned long long own = zr[wi];
    if ((own >> bit) & 1ull) return 0u;
    unsigned dl = G_INF, dr = G_INF;
    unsigned long long m = own & ((1ull << bit) - 1ull);
    int w = wi;
    while (m == 0 && w > 0) m = zr[--w];
    if (m) dl = (unsigned)(x - (w * 64 + 63 - __clzll((long long)m)));
    m = bit == 63 ? 0ull : (own >> (bit + 1)) << (bit + 1);
    w = wi;
    while (m == 0 && w + 1 < WW) m = zr[++w];
    if (m) dr = (unsigned)(w * 64 + __ffsll((long long)m) - 1 - x);
    const unsigned d = dl < dr ? dl : dr;
    return d >= G_INF ? G_INF : d;
}

template <int EC_ROWS, int EC_HALO>
__global__ void __launch_bounds__(256) edt_bits_kernel(const unsigned long long* __restrict__ zw, int* __restrict__ d2_out,
                                                       double* __restrict__ edt_out, int H, int W, int WW) {
    constexpr int EC_TROWS = EC_ROWS + 2 * EC_HALO;
    __shared__ __attribute__((aligned(16))) unsigned short tile[EC_TROWS][64];
    __shared__ unsigned long long zs[EC_TROWS][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = blockIdx.x;  // the tile's word column
    const int y0 = blockIdx.y * EC_ROWS;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const unsigned long long* zp = zw + (size_t)blockIdx.z * H * WW;
    // ---- the zero flags of the window: own word, left and right neighbour (outside the image: no zero) ----
    for (int i = threadIdx.x; i < EC_TROWS * 3; i += 256) {
        const int r = i / 3, c = i - r * 3;
        const int y = y0 - EC_HALO + r, w = wi - 1 + c;
        zs[r][c] = (y >= 0 && y < H && w >= 0 && w < WW) ? zp[(size_t)y * WW + w] : 0ull;
    }
    __syncthreads();
    // ---- g of the window: a thread owns 8 consecutive pixels of a row.  The nearest zero left of the group (clz) and
    // right of it (ffs) seed a forward and a backward sweep over the 8 pixels, and the 8 distances leave in one 16-byte
    // store ----
    constexpr unsigned BIG = 0x20000u;  // > any distance inside a row (sides are <= 32768)
    for (int task = threadIdx.x; task < EC_TROWS * 8; task += 256) {
        const int r = task >> 3, b = task & 7;
        const int y = y0 - EC_HALO + r;
        uint4 out = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);  // rows outside the image: G_INF
        if (y >= 0 && y < H) {
            const int bit0 = b * 8, x0 = wi * 64 + bit0;
            const unsigned long long own = zs[r][1];
            const unsigned z8 = (unsigned)(own >> bit0) & 0xffu;
            out = make_uint4(0u, 0u, 0u, 0u);
            if (z8 != 0xffu) {
                unsigned dl = BIG, dr = BIG;  // distance of pixel x0 to the nearest zero left of the group / of x0+7 right
                unsigned long long m = own & ((1ull << bit0) - 1ull);
                int w = wi;
                if (m == 0 && w > 0) {
                    m = zs[r][0];
                    --w;
                    const unsigned long long* zr = zp + (size_t)y * WW;
                    while (m == 0 && w > 0) m = zr[--w];
                }
                if (m) dl = (unsigned)(x0 - (w * 64 + 63 - __clzll((long long)m)));
                const int sh = bit0 + 8;
                m = sh == 64 ? 0ull : (own >> sh) << sh;
                w = wi;
                if (m == 0 && w + 1 < WW) {
                    m = zs[r][2];
                    ++w;
                    const unsigned long long* zr = zp + (size_t)y * WW;
                    while (m == 0 && w + 1 < WW) m = zr[++w];
                }
                if (m) dr = (unsigned)(w * 64 + __ffsll((long long)m) - 1 - (x0 + 7));
                unsigned L[8], R[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned prev = i == 0 ? dl : L[i - 1] + 1u;
                    L[i] = ((z8 >> i) & 1u) ? 0u : (prev < BIG ? prev : BIG);
                }
#pragma unroll
                for (int i = 7; i >= 0; --i) {
                    const unsigned nxt = i == 7 ? dr : R[i + 1] + 1u;
                    R[i] = ((z8 >> i) & 1u) ? 0u : (nxt < BIG ? nxt : BIG);
                }
                unsigned d[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned mn = L[i] < R[i] ? L[i] : R[i];
                    d[i] = mn >= G_INF ? G_INF : mn;
                }
                out.x = d[0] | (d[1] << 16);
                out.y = d[2] | (d[3] << 16);
                out.z = d[4] | (d[5] << 16);
                out.w = d[6] | (d[7] << 16);
            }
        }
        *reinterpret_cast<uint4*>(&tile[r][b * 8]) = out;
    }
    __syncthreads();
    // ---- the column search (g beyond the halo evaluated from the words).  A lane owns FOUR
    // consecutive pixels of a row: one 8-byte LDS read brings the four g of a row above / below, the four searches are
    // independent chains that share every LDS wait, and the results leave in one 16-byte store (a wave writes 4 rows x
    // 256 bytes; with a pixel per lane the stores alone took 223 us per 48 planes, 3.6 TB/s) ----
    const int c4 = (lane & 15) * 4, rsub = lane >> 4;
    const int xg = wi * 64 + c4;
    if (xg >= W) return;
    const bool vec = xg + 3 < W && (W & 3) == 0 && (!d2_out || (reinterpret_cast<uintptr_t>(d2_out) & 15) == 0) &&
                     (!edt_out || (reinterpret_cast<uintptr_t>(edt_out) & 15) == 0);
#pragma unroll 1
    for (int j = 0; j < EC_ROWS / 16; ++j) {
        const int ly = EC_HALO + wave * (EC_ROWS / 4) + rsub + 4 * j;
        const int y = y0 - EC_HALO + ly;
        if (y >= H) continue;
        unsigned best[4];
        {
            const uint2 gq = *reinterpret_cast<const uint2*>(&tile[ly][c4]);
            const unsigned g0[4] = {gq.x & 0xFFFFu, gq.x >> 16, gq.y & 0xFFFFu, gq.y >> 16};
#pragma unroll
            for (int i = 0; i < 4; ++i) best[i] = g0[i] == G_INF ? 0xFFFFFFFFu : g0[i] * g0[i];
        }
        for (unsigned k = 1; k <= (unsigned)EC_HALO; ++k) {
            const unsigned kk = k * k;
            if (!(kk < best[0] || kk < best[1] || kk < best[2] || kk < best[3])) break;
            const uint2 uq = *reinterpret_cast<const uint2*>(&tile[ly - (int)k][c4]);
            const uint2 dq = *reinterpret_cast<const uint2*>(&tile[ly + (int)k][c4]);
            const unsigned gu[4] = {uq.x & 0xFFFFu, uq.x >> 16, uq.y & 0xFFFFu, uq.y >> 16};
            const unsigned gd[4] = {dq.x & 0xFFFFu, dq.x >> 16, dq.y & 0xFFFFu, dq.y >> 16};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned gm = gu[i] < gd[i] ? gu[i] : gd[i];
                // gm == G_INF: 65535^2 + k^2 < 2^32 stays above every finite candidate and below the "no zero" mark
                const unsigned c = gm == G_INF ? 0xFFFFFFFFu : kk + gm * gm;
                best[i] = c < best[i] ? c : best[i];  // a candidate at distance k cannot beat best <= k^2: no need to mask
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned bq = best[i];
            const int x = xg + i;
            if (bq != 0 && x < W) {
                for (unsigned kk = EC_HALO + 1; kk < 65536u && (unsigned long long)kk * kk < bq; ++kk) {  // beyond the LDS halo
                    const int yu = y - (int)kk, yd = y + (int)kk;
                    if (yu < 0 && yd >= H) break;
                    unsigned gm = G_INF;
                    if (yu >= 0) gm = edt_g_at(zp + (size_t)yu * WW, WW, x);
                    if (yd < H) {
                        const unsigned gd = edt_g_at(zp + (size_t)yd * WW, WW, x);
                        gm = gd < gm ? gd : gm;
                    }
                    if (gm != G_INF) {
                        const unsigned c = kk * kk + gm * gm;  // < 2^31: both terms < 2^30
                        bq = c < bq ? c : bq;
                    }
                }
                // no zero pixel in the whole plane (a column sees none only then): scipy's feature transform then
                // measures from index (-1, 0) -- distance_transform_edt(np.ones((2, 2))) == [[1, sqrt 2], [2, sqrt 5]]
                if (bq > 0x7fffffffu) bq = (unsigned)(y + 1) * (unsigned)(y + 1) + (unsigned)x * (unsigned)x;
            }
            best[i] = bq;
        }
        const size_t i0 = plane + (size_t)y * W + xg;
        if (vec) {
            if (d2_out) *reinterpret_cast<int4*>(d2_out + i0) = make_int4((int)best[0], (int)best[1], (int)best[2], (int)best[3]);
            if (edt_out) {
                *reinterpret_cast<double2*>(edt_out + i0) = make_double2(sqrt((double)best[0]), sqrt((double)best[1]));
                *reinterpret_cast<double2*>(edt_out + i0 + 2) = make_double2(sqrt((double)best[2]), sqrt((double)best[3]));
            }
        } else {
            for (int i = 0; i < 4 && xg + i < W; ++i) {
                if (d2_out) d2_out[i0 + i] = (int)best[i];
                if (edt_out) edt_out[i0 + i] = sqrt((double)best[i]);
            }
        }
    }
}

extern "C" int amt_edt(amt_ctx* ctx, const uint8_t* mask, int32_t* d2_out, double* edt_out, int nplanes, int H,
                       int W) {
    AMT_CHECK_OPERANDS("amt_edt", amt_in("mask", mask, amt_span(1, nplanes, H, W)), amt_out("d2_out", d2_out, amt_span(4, nplanes, H, W)),
                       amt_out("edt_out", edt_out, amt_span(8, nplanes, H, W)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(mask && (d2_out || edt_out) && nplanes >= 0 && H > 0 && W > 0, "edt: bad arguments");
    AMT_REQUIRE(H <= 32768 && W <= 32768, "edt: image larger than 32768 pixels per side");
    if (nplanes == 0) return AMT_OK;
    const size_t tiles64 = (size_t)((W + 63) / 64) * ((H + 63) / 64) * nplanes;
    const int WW = (W + 63) / 64;
    const size_t nwords = (size_t)nplanes * H * WW;
    amt_scratch s(ctx);
    amt_buf<unsigned long long> zw(s, nwords);
    AMT_TRY(s.commit());
    const int fast = W % 16 == 0 && (reinterpret_cast<uintptr_t>(mask) & 15) == 0;
    hipLaunchKernelGGL(edt_zero_words_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, ctx->stream, mask, zw, H,
                       W, WW, nwords, fast);
    AMT_LAUNCH_CHECK();
    if (tiles64 >= 4096 && !edt_out)  // with the float64 output (sqrt + 8-byte stores) the shorter tiles measured faster
        hipLaunchKernelGGL((edt_bits_kernel<64, 16>), dim3(WW, (H + 63) / 64, nplanes), dim3(256), 0, ctx->stream, zw, d2_out,
                           edt_out, H, W, WW);
    else
        hipLaunchKernelGGL((edt_bits_kernel<32, 24>), dim3(WW, (H + 31) / 32, nplanes), dim3(256), 0, ctx->stream, zw, d2_out,
                           edt_out, H, W, WW);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- peak mask ---------------------------------------------------------------------------------
// peaks = (d2 == maximum_filter(d2, size=2m+1, mode='constant' (0))) & mask & (d2 > 0), border m cleared
// (comparing the integer d2 is equivalent to comparing sqrt(d2)).
// "d2 equals the window maximum" == "nothing in the window exceeds d2", so no maximum image is built: a pixel
// is first compared with its 8 neighbours (which rejects all but a few per nucleus), and only the survivors look
// at the full (2m+1)^2 window.
constexpr int PK_MAXM = 16;
// No LDS: a wave slides a three-row register window down a strip of PKR_IN columns (+ one halo
// column on either side); the 8-neighbour pre-test uses DPP wave shifts, and the few survivors (a handful per
// nucleus) are checked one at a time by the WHOLE wave: 64 lanes read the (2m+1)^2 window straight from global
// memory (L2 hits: the strip has just streamed those rows) and vote.  The host clears `peaks` first; only peak
// pixels are written.
constexpr int PKR_ROWS = 64, PKR_IN = 62, PKR_BATCH = 22, PKR_NBATCH = (PKR_ROWS + 2) / PKR_BATCH;
static_assert(PKR_BATCH * PKR_NBATCH == PKR_ROWS + 2, "row batches must tile the strip");
// LIST (amt_peak_markers): every peak is also appended to its plane's "found" list, found[plane * cap ...], a wave's
// peaks together with one returning atomic on the plane's counter fcount[plane * PKM_CNT_STRIDE]; the order is whatever
// the waves' timing makes it, and the counter keeps counting past `cap` (the entries beyond are dropped: that plane has
// overflowed).
constexpr int PKM_CNT_STRIDE = 32;  // words between the planes' counters: one 128-byte line each (PFX_CNT_STRIDE's reason)

template <bool LIST>
__global__ void __launch_bounds__(256) peaks_rows_kernel(const int* __restrict__ d2, const uint8_t* __restrict__ mask,
                                                         uint8_t* __restrict__ peaks, int H, int W, int m,
                                                         int* __restrict__ found, int* __restrict__ fcount, int cap) {
    const int lane = threadIdx.x & 63;
    const int strip = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (strip * PKR_IN >= W) return;  // whole wave; the kernel has no barrier
    const size_t base = (size_t)blockIdx.z * H * W;
    const int* D = d2 + base;
    const int x = strip * PKR_IN - 1 + lane;
    const int y0 = blockIdx.y * PKR_ROWS;
    const bool xin = x >= 0 && x < W;
    const bool xok = xin && lane >= 1 && lane <= PKR_IN && x >= m && x < W - m;  // output lane inside the cleared frame
    const int side = 2 * m + 1, wsize = side * side;

    // UNCONDITIONAL loads from clamped coordinates; positions outside the image become the constant 0 where the
    // value is used (a select next to the load would be turned back into a branch around it, and the wait that
    // comes with it serialises the loads)
    const int xc = x < 0 ? 0 : (x < W ? x : W - 1);
    auto load_row = [&](int y) -> int {
        const int yc = y < 0 ? 0 : (y < H ? y : H - 1);
        return D[(size_t)yc * W + xc];
    };
    // LIST: the wave collects its peaks in registers and appends them with ONE returning atomic when it ends (or holds 64)
    int npk = 0, mypk = 0;
    auto flush = [&]() {
        int at = 0;
        if (lane == 0) at = atomicAdd(&fcount[(size_t)blockIdx.z * PKM_CNT_STRIDE], npk);
        at = __shfl(at, 0) + lane;
        if (lane < npk && at < cap) found[(size_t)blockIdx.z * cap + at] = mypk;
        npk = 0;
    };
    int cur[PKR_BATCH], nxt[PKR_BATCH];
#pragma unroll
    for (int j = 0; j < PKR_BATCH; ++j) cur[j] = load_row(y0 - 1 + j);
    // window: v1 = row r-1 (the centre row of this step) with its neighbours, h2 = 3-wide maximum of row r-2
    int v1 = 0, v1l = 0, v1r = 0, h1 = 0, h2 = 0;
    for (int b = 0; b < PKR_NBATCH; ++b) {
        if (b + 1 < PKR_NBATCH) {
#pragma unroll
            for (int j = 0; j < PKR_BATCH; ++j) nxt[j] = load_row(y0 - 1 + (b + 1) * PKR_BATCH + j);
        }
#pragma unroll
        for (int j = 0; j < PKR_BATCH; ++j) {
            const int r = y0 - 1 + b * PKR_BATCH + j;  // row of v0
            const int v0 = (xin && r >= 0 && r < H) ? cur[j] : 0;
            if (__ballot(v0 > 0 || v1 > 0) == 0ull) {  // uniform: no candidate in row r-1, nothing to carry from row r
                h2 = h1, h1 = 0, v1 = 0, v1l = 0, v1r = 0;  // (non-positive values never beat a candidate)
                continue;
            }
            const int v0l = amt_lane_left(v0), v0r = amt_lane_right(v0);
            int h0 = v0 > v0l ? v0 : v0l;
            h0 = h0 > v0r ? h0 : v0r;
            const int yc = r - 1;  // centre row
            bool cand = xok && v1 > 0 && yc >= y0 && yc < y0 + PKR_ROWS && yc >= m && yc < H - m;
            if (m >= 1) {
                int nb = h0 > h2 ? h0 : h2;
                nb = nb > v1l ? nb : v1l;
                nb = nb > v1r ? nb : v1r;
                cand = cand && !(nb > v1);
            }
            unsigned long long todo = __ballot(cand);
            while (todo) {  // uniform: one survivor at a time, the whole wave reads its window
                const int sl = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const int sv = __shfl(v1, sl);
                const int sx = strip * PKR_IN - 1 + sl;
                bool gt = false;
                for (int k = lane; k < wsize; k += 64) {
                    const int dy = k / side, dx = k - dy * side;
                    gt |= D[(size_t)(yc - m + dy) * W + (sx - m + dx)] > sv;  // inside the image: the frame is cleared
                }
                const bool hit = __ballot(gt) == 0ull && lane == sl && mask[base + (size_t)yc * W + sx];
                if (hit) peaks[base + (size_t)yc * W + sx] = 1;
                if (LIST && __ballot(hit) != 0ull) {  // uniform: the wave's npk-th peak waits in lane npk
                    if (lane == npk) mypk = yc * W + sx;
                    if (++npk == 64) flush();
                }
            }
            h2 = h1, h1 = h0;
            v1 = v0, v1l = v0l, v1r = v0r;
        }
#pragma unroll
        for (int j = 0; j < PKR_BATCH; ++j) cur[j] = nxt[j];
    }
    if (LIST && npk) flush();
}

// peaks[list[k]] = 0 for the listed pixels of every plane
// (status[plane] < 0: that run's list overflowed and does not hold every peak -- the whole plane is cleared)
__global__ void __launch_bounds__(256) peaks_unwrite_kernel(const int* __restrict__ list, const int* __restrict__ count,
                                                            const int* __restrict__ status, uint8_t* __restrict__ peaks,
                                                            size_t n, int cap) {
    uint8_t* o = peaks + (size_t)blockIdx.y * n;
    if (status[blockIdx.y] < 0) {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) o[i] = 0;
        return;
    }
    const int K = count[blockIdx.y] < cap ? count[blockIdx.y] : cap;
    const int* lst = list + (size_t)blockIdx.y * cap;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) o[lst[k]] = 0;
}

// prev_list / prev_count / prev_status (all or none): the previous run's peak lists and label counts (amt_hip.h)
extern "C" int amt_peak_mask(amt_ctx* ctx, const int32_t* d2, const uint8_t* mask, uint8_t* peaks, int nplanes, int H,
                             int W, int min_distance, const int32_t* prev_list, const int32_t* prev_count, int capacity,
                             const int32_t* prev_status) {
    AMT_REQUIRE(!prev_list == !prev_count && !prev_list == !prev_status,
                "peak_mask: the previous run's peak lists, counts and label counts go together");
    AMT_REQUIRE(!prev_list || capacity >= 1, "peak_mask: the previous run's list capacity must be positive");
    // mask and peaks are both byte planes: peaks onto the mask would pass every type check
    AMT_CHECK_OPERANDS("amt_peak_mask", amt_in("d2", d2, amt_span(4, nplanes, H, W)), amt_in("mask", mask, amt_span(1, nplanes, H, W)),
                       amt_out("peaks", peaks, amt_span(1, nplanes, H, W)),
                       amt_in("prev_list", prev_list, amt_span(4, nplanes, capacity)),
                       amt_in("prev_count", prev_count, amt_span(4, nplanes)),
                       amt_in("prev_status", prev_status, amt_span(4, nplanes)));
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(d2 && mask && peaks && nplanes >= 0 && H > 0 && W > 0, "peak_mask: bad arguments");
    AMT_REQUIRE(min_distance >= 0 && min_distance <= PK_MAXM, "peak_mask: min_distance %d out of range 0..%d",
                min_distance, PK_MAXM);
    if (nplanes == 0) return AMT_OK;
    const int m = min_distance;
    if (prev_list) {
        // the plane is zero except at the previous run's peaks, which amt_label_sparse kept as a list
        hipLaunchKernelGGL(peaks_unwrite_kernel, dim3(amt_grid_for((size_t)capacity, 256, 64), nplanes), dim3(256), 0,
                           ctx->stream, prev_list, prev_count, prev_status, peaks, (size_t)H * W, capacity);
        AMT_LAUNCH_CHECK();
    } else {
        AMT_HIP_CHECK(hipMemsetAsync(peaks, 0, (size_t)nplanes * H * W, ctx->stream));
    }
    const int nstrips = (W + PKR_IN - 1) / PKR_IN;
    dim3 grid((nstrips + 3) / 4, (H + PKR_ROWS - 1) / PKR_ROWS, nplanes);
    hipLaunchKernelGGL(peaks_rows_kernel<false>, grid, dim3(256), 0, ctx->stream, d2, mask, peaks, H, W, m, (int*)nullptr,
                       (int*)nullptr, 0);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// ---- peak markers: amt_peak_mask + amt_label_sparse from the list of the peaks the search found ------------------------
// The search knows every peak when it writes it, so nothing scans a plane for them: peaks_clear_kernel undoes the previous
// run's writes in both planes, peaks_rows_kernel<true> lists what it finds, and ONE workgroup per plane
// (sp_markers_kernel) sorts that list into raster order -- which makes it amt_label_sparse's compacted list --, joins
// neighbours, ranks the roots and scatters the labels.  Same numbering as amt_label_sparse by construction: the root of a
// component is its smallest list index, roots are numbered in list order.
constexpr int PKM_TIER = AMT_PEAK_MARKERS_LDS_TIER;  // longer lists are labelled in the arena's global scratch
constexpr int PKM_THREADS = 1024;
static_assert(2 * PKM_TIER * sizeof(int) <= 36 * 1024 - 256, "list + parents of the LDS tier stay below 36 KB");

// peaks[p] = 0 and markers[p] = 0 for the pixels the previous run listed (status[plane] < 0: that run overflowed its
// list and both planes are cleared whole); the plane's counter of found peaks starts at zero
__global__ void __launch_bounds__(256) peaks_clear_kernel(const int* __restrict__ list, const int* __restrict__ count,
                                                          const int* __restrict__ status, uint8_t* __restrict__ peaks,
                                                          int* __restrict__ markers, int* __restrict__ fcount, size_t n,
                                                          int cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) fcount[(size_t)blockIdx.y * PKM_CNT_STRIDE] = 0;
    uint8_t* pk = peaks + (size_t)blockIdx.y * n;
    int* mk = markers + (size_t)blockIdx.y * n;
    if (status[blockIdx.y] < 0) {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) pk[i] = 0, mk[i] = 0;
        return;
    }
    const int K = count[blockIdx.y] < cap ? count[blockIdx.y] : cap;
    const int* lst = list + (size_t)blockIdx.y * cap;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
        const int p = lst[k];
        pk[p] = 0;
        mk[p] = 0;
    }
}

// Ascending sort of a[0 .. n) by the whole workgroup, any n: bitonic merges whose first step mirrors its block, so every
// compare-exchange moves the smaller value to the lower index and the elements past n -- which stand for +infinity --
// would never move; pairs that reach past n are skipped.  Ends behind a barrier.
__device__ __forceinline__ void pkm_exchange(int* a, int i, int l, int n) {
    if (l < n) {
        const int u = a[i], v = a[l];
        if (u > v) a[i] = v, a[l] = u;
    }
}
__device__ __forceinline__ void pkm_sort(int* a, int n) {
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    const int pairs = n2 >> 1;
    for (int k = 2; k <= n2; k <<= 1) {
        const int hk = k >> 1;
        for (int t = threadIdx.x; t < pairs; t += PKM_THREADS) {
            const int i = ((t & ~(hk - 1)) << 1) | (t & (hk - 1));
            pkm_exchange(a, i, i ^ (k - 1), n);
        }
        __syncthreads();
        for (int j = hk >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < pairs; t += PKM_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                pkm_exchange(a, i, i | j, n);
            }
            __syncthreads();
        }
    }
}

// The found list lst[0 .. K) of one plane -> sorted (and stored as the keep list kl), labelled, scattered into mk.
// lst / par live in LDS (LDS) or in global scratch; returns the number of components.  wsum = one int per wave.
template <bool LDS>
__device__ __forceinline__ int pkm_label(int* lst, int* par, int K, int W, int conn8, int* __restrict__ mk,
                                         int* __restrict__ kl, int* wsum) {
    const int tid = threadIdx.x;
    pkm_sort(lst, K);
    for (int k = tid; k < K; k += PKM_THREADS) {
        par[k] = k;
        if (kl) kl[k] = lst[k];
    }
    __syncthreads();
    // unions with the west, north and (8-connectivity) north-west / north-east neighbours: the west one is the previous
    // entry, the others sit around the lower bound of p - W among the entries before k
    for (int k = tid; k < K; k += PKM_THREADS) {
        const int p = lst[k];
        const int y = p / W, x = p - y * W;
        if (x > 0 && k > 0 && lst[k - 1] == p - 1) {
            if (LDS) lds_union(par, k, k - 1); else uf_union(par, k, k - 1);
        }
        if (y == 0) continue;
        const int north = p - W;
        int lo = 0, hi = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (lst[mid] < north) lo = mid + 1; else hi = mid;
        }
        // lo <= k and lst[lo] >= north (lst[k] = p itself ends the search)
        const bool up = lst[lo] == north;
        if (up) {
            if (LDS) lds_union(par, k, lo); else uf_union(par, k, lo);
        }
        if (conn8) {
            if (x > 0 && lo > 0 && lst[lo - 1] == north - 1) {
                if (LDS) lds_union(par, k, lo - 1); else uf_union(par, k, lo - 1);
            }
            const int ne = lo + (up ? 1 : 0);
            if (x + 1 < W && ne < k && lst[ne] == north + 1) {
                if (LDS) lds_union(par, k, ne); else uf_union(par, k, ne);
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < K; k += PKM_THREADS) par[k] = LDS ? lds_find(par, k) : uf_find_volatile(par, k);
    __syncthreads();
    // rank the roots in list order: every thread owns a stretch of consecutive entries
    const int per = (K + PKM_THREADS - 1) / PKM_THREADS;
    const int b = tid * per < K ? tid * per : K, e = b + per < K ? b + per : K;
    int mine = 0;
    for (int k = b; k < e; ++k) mine += par[k] == k ? 1 : 0;
    const int lane = tid & 63, wave = tid >> 6;
    const int incl = ccl_wave_incl_scan(mine, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int rank = incl - mine, total = 0;
    for (int w = 0; w < PKM_THREADS / 64; ++w) {
        if (w < wave) rank += wsum[w];
        total += wsum[w];
    }
    for (int k = b; k < e; ++k)
        if (par[k] == k) par[k] = ~(rank++);  // a root carries its rank, complemented: negative, so no parent index
    __syncthreads();
    for (int k = tid; k < K; k += PKM_THREADS) {
        int v = par[k];
        if (v >= 0) v = par[v];
        mk[lst[k]] = -v;  // rank + 1
    }
    return total;
}

__global__ void __launch_bounds__(PKM_THREADS) sp_markers_kernel(int* found, const int* __restrict__ fcount, int* gpar,
                                                                 int* __restrict__ markers, int* __restrict__ count_dev,
                                                                 int* __restrict__ keep_list, int* __restrict__ keep_count,
                                                                 size_t n, int W, int cap, int conn8) {
    __shared__ int s_lst[PKM_TIER], s_par[PKM_TIER];
    __shared__ int s_wsum[PKM_THREADS / 64];
    const int plane = blockIdx.x;
    const int K = fcount[(size_t)plane * PKM_CNT_STRIDE];
    if (K > cap) {  // block-uniform: the list does not hold every peak -- no markers, and the next run clears whole planes
        if (threadIdx.x == 0) {
            count_dev[plane] = -1;
            if (keep_count) keep_count[plane] = 0;
        }
        return;
    }
    int* fl = found + (size_t)plane * cap;
    int* mk = markers + (size_t)plane * n;
    int* kl = keep_list ? keep_list + (size_t)plane * cap : nullptr;
    int nroots;
    if (K <= PKM_TIER) {
        for (int k = threadIdx.x; k < K; k += PKM_THREADS) s_lst[k] = fl[k];
        __syncthreads();
        nroots = pkm_label<true>(s_lst, s_par, K, W, conn8, mk, kl, s_wsum);
    } else {
        nroots = pkm_label<false>(fl, gpar + (size_t)plane * cap, K, W, conn8, mk, kl, s_wsum);
    }
    if (threadIdx.x == 0) {
        count_dev[plane] = nroots;
        if (keep_count) keep_count[plane] = K;
    }
}

extern "C" int amt_peak_markers(amt_ctx* ctx, const int32_t* d2, const uint8_t* mask, uint8_t* peaks, int32_t* markers,
                                int32_t* count_dev, int nplanes, int H, int W, int min_distance, int connectivity,
                                int capacity, int32_t* keep_list, int32_t* keep_count) {
    AMT_REQUIRE(!keep_list == !keep_count, "peak_markers: keep_list and keep_count go together");
    AMT_CHECK_OPERANDS("amt_peak_markers", amt_in("d2", d2, amt_span(4, nplanes, H, W)), amt_in("mask", mask, amt_span(1, nplanes, H, W)),
                       amt_out("peaks", peaks, amt_span(1, nplanes, H, W)), amt_out("markers", markers, amt_span(4, nplanes, H, W)),
                       amt_out("count_dev", count_dev, amt_span(4, nplanes)),
                       amt_out("keep_list", keep_list, amt_span(4, nplanes, capacity)),
                       amt_out("keep_count", keep_count, amt_span(4, nplanes)));
    AMT_REQUIRE(d2 && mask && peaks && markers && count_dev && nplanes >= 0 && H > 0 && W > 0,
                "peak_markers: bad arguments");
    AMT_REQUIRE(min_distance >= 0 && min_distance <= PK_MAXM, "peak_markers: min_distance %d out of range 0..%d",
                min_distance, PK_MAXM);
    AMT_REQUIRE(connectivity == 1 || connectivity == 2, "peak_markers: connectivity must be 1 or 2");
    AMT_REQUIRE(capacity >= 1, "peak_markers: capacity must be positive");
    AMT_REQUIRE((size_t)H * W < 0x7fffffffull, "peak_markers: plane too large");
    AMT_TRY(amt_set_device(ctx));
    if (nplanes == 0) return AMT_OK;
    const size_t n = (size_t)H * W;
    const size_t capn = (size_t)nplanes * capacity;
    amt_scratch s(ctx);
    amt_buf<int> found(s, capn);   // a buffer of its own: the keep list holds the previous run's pixels until the clear has run
    amt_buf<int> parent(s, capn);  // lists beyond the LDS tier only
    amt_buf<int> fcount(s, (size_t)nplanes * PKM_CNT_STRIDE);
    AMT_TRY(s.commit());
    if (keep_list) {
        hipLaunchKernelGGL(peaks_clear_kernel, dim3(amt_grid_for((size_t)capacity, 256, 64), nplanes), dim3(256), 0,
                           ctx->stream, (const int*)keep_list, (const int*)keep_count, (const int*)count_dev, peaks, markers,
                           (int*)fcount, n, capacity);
        AMT_LAUNCH_CHECK();
    } else {
        AMT_HIP_CHECK(hipMemsetAsync(peaks, 0, (size_t)nplanes * n, ctx->stream));
        AMT_HIP_CHECK(hipMemsetAsync(markers, 0, (size_t)nplanes * n * sizeof(int32_t), ctx->stream));
        AMT_HIP_CHECK(hipMemsetAsync(fcount, 0, (size_t)nplanes * PKM_CNT_STRIDE * sizeof(int), ctx->stream));
    }
    const int nstrips = (W + PKR_IN - 1) / PKR_IN;
    dim3 grid((nstrips + 3) / 4, (H + PKR_ROWS - 1) / PKR_ROWS, nplanes);
    hipLaunchKernelGGL(peaks_rows_kernel<true>, grid, dim3(256), 0, ctx->stream, d2, mask, peaks, H, W, min_distance,
                       (int*)found, (int*)fcount, capacity);
    AMT_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_markers_kernel, dim3(nplanes), dim3(PKM_THREADS), 0, ctx->stream, (int*)found,
                       (const int*)fcount, (int*)parent, markers, count_dev, keep_list, keep_count, n, W, capacity,
                       connectivity == 2 ? 1 : 0);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}
