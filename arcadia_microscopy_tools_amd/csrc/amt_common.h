// Internal helpers shared by the HIP translation units of libamt_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/amt_hip.h"
#include "amt_scratch_plan.h"

struct amt_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    // grow-only scratch arena; handed out whole by amt_scratch::commit at the start of every public op
    char* arena;
    size_t arena_cap;
    // pinned host ring for small parameter tables (weights, footprint offsets, rank requests): the
    // caller's pointer is consumed before the public function returns, the DMA reads the pinned copy.
    char* mailbox;
    size_t mailbox_cap;
    size_t mailbox_off;
    int num_cus;
    // auxiliary streams + events for fork/join of independent latency-bound kernels inside one op
    hipStream_t aux[3];      // the streams an op's independent kernels are launched on (auxiliary ones, or `stream`)
    hipStream_t aux_own[3];  // the auxiliary streams this context created
    hipEvent_t ev[4];
    bool aux_ready;
    int fork;  // amt_ctx_set_fork: how many auxiliary streams the ops of this context use (0..3)
    // the last committed plan (offsets, exact lengths, total): what amt_debug_scratch_check scans the padding of
    size_t plan_off[AMT_SCRATCH_SLOTS];
    size_t plan_len[AMT_SCRATCH_SLOTS];
    int plan_count;
    size_t plan_total;
    bool plan_valid;
    unsigned long long* dbg_first;  // device word of amt_debug_scratch_check (allocated on its first use)
    // ---- label boxes handed from amt_watershed_edt_cleared to the per-label call that directly follows it ----
    // op_serial counts the image operations of this context: every entry point that checks operands
    // (amt_check_operands counts), every copy, fill, allocation, release and synchronisation, and every call that makes
    // the context's work visible to another stream or to the host (amt_stream_wait on either side, event record / wait /
    // sync, amt_timer_elapsed_ms) advances it.  The note names the label planes whose boxes box_buf holds (grow-only,
    // outside the arena, which the next op reuses) and the serial of the call that enqueued them; amt_box_note_take
    // (below) is the one look at it.
    unsigned long long op_serial;
    int* box_buf;
    size_t box_cap;  // ints
    struct {
        bool valid;
        const void* labels;
        int nplanes, H, W, max_label, device;
        unsigned long long serial;
    } box_note;
};
static inline void amt_note_op(amt_ctx* ctx) {
    if (ctx) ++ctx->op_serial;
}
// amt_ctx.hip.  amt_box_buffer: box_buf with room for `ints` ints (drops the note; may synchronise to grow).
// amt_box_note_leave: the producer has ENQUEUED the boxes {ymin, xmin, ymax, xmax} of labels 1..max_label of these planes.
// amt_box_note_take: the consumer's one look -- the boxes if the note was left by the image operation directly before
// the current one on this context and names exactly these planes, else nullptr; the note is gone either way.
int amt_box_buffer(amt_ctx* ctx, size_t ints, int** buf);
void amt_box_note_leave(amt_ctx* ctx, const void* labels, int nplanes, int H, int W, int max_label);
const int* amt_box_note_take(amt_ctx* ctx, const void* labels, int nplanes, int H, int W, int max_label);
bool amt_poison_enabled();  // AMT_DEBUG_POISON=1

// fork: aux streams wait for everything enqueued so far on the main stream; join: main waits for them
int amt_fork(amt_ctx* ctx);
int amt_join(amt_ctx* ctx);

void amt_set_error(const char* fmt, ...);

#define AMT_HIP_CHECK(expr)                                                                      \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            amt_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return AMT_EHIP;                                                                     \
        }                                                                                        \
    } while (0)

#define AMT_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            amt_set_error(__VA_ARGS__); \
            return AMT_EINVAL;          \
        }                               \
    } while (0)

#define AMT_LAUNCH_CHECK()                                                                        \
    do {                                                                                          \
        hipError_t _e = hipGetLastError();                                                        \
        if (_e != hipSuccess) {                                                                   \
            amt_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return AMT_EHIP;                                                                      \
        }                                                                                         \
    } while (0)

#define AMT_TRY(expr)             \
    do {                          \
        int _rc = (expr);         \
        if (_rc != AMT_OK) return _rc; \
    } while (0)

// ---- operand aliasing (include/amt_hip.h, Conventions) ---------------------------------------------------------
// Every entry point that writes device memory hands its device operands to amt_check_operands FIRST: before the context
// is touched -- but for its count of image operations, which amt_check_operands advances (amt_note_op) -- and before
// anything is reserved or launched (a refusal needs no device; a few pointer comparisons on the host, no launch, no
// synchronisation).  Inputs may overlap inputs.  An output -- caller-owned scratch and in/out planes included -- must
// not overlap any other operand, except that it may COINCIDE with the inputs named in `inplace` (a mask over the
// indices of the operand list): same start, same byte length, same element size.  A null pointer or a length of zero is
// an absent operand.
struct amt_operand {
    const char* name;
    const void* ptr;
    size_t bytes;
    bool output;
    unsigned inplace;  // outputs: bit i set = may coincide exactly with operand i of the list
    size_t elem;       // element size, compared for an in-place pair
};
static inline amt_operand amt_in(const char* name, const void* p, size_t bytes, size_t elem = 1) {
    return amt_operand{name, p, bytes, false, 0u, elem};
}
static inline amt_operand amt_out(const char* name, const void* p, size_t bytes, unsigned inplace = 0u, size_t elem = 1) {
    return amt_operand{name, p, bytes, true, inplace, elem};
}
// elem * a * b * c * d bytes; 0 when a factor is not positive (the entry point's own argument checks refuse those)
static inline size_t amt_span(size_t elem, long long a, long long b = 1, long long c = 1, long long d = 1) {
    if (a <= 0 || b <= 0 || c <= 0 || d <= 0 || elem == 0) return 0;
    const long long f[4] = {a, b, c, d};
    size_t n = elem;
    for (long long v : f) {
        if (n > (SIZE_MAX >> 1) / (size_t)v) return SIZE_MAX >> 1;
        n *= (size_t)v;
    }
    return n;
}
static inline size_t amt_esize(int dtype) {
    switch (dtype) {
        case AMT_U8: return 1;
        case AMT_U16: return 2;
        case AMT_I32: case AMT_F32: return 4;
        case AMT_F64: case AMT_I64: return 8;
        default: return 0;  // an unknown code: the operand counts as absent, the entry point refuses the code
    }
}
// counts an image operation of `ctx` (nullable), refused or not, then checks
int amt_check_operands(amt_ctx* ctx, const char* op, const amt_operand* ops, int n);
// needs the entry point's context in scope under the name `ctx`
#define AMT_CHECK_OPERANDS(op, ...)                                                              \
    do {                                                                                         \
        const amt_operand _ops[] = {__VA_ARGS__};                                                \
        AMT_TRY(amt_check_operands(ctx, op, _ops, (int)(sizeof(_ops) / sizeof(_ops[0]))));       \
    } while (0)

// ---- scratch ----------------------------------------------------------------------------------
// An op declares its buffers into an amt_scratch (amt_scratch_plan.h: the layout rule), then commits once: commit()
// reserves exactly the declared total in the context's arena (may reallocate: synchronises the stream first) and only
// then fills the pointers.  Memory is only valid until the next op on the same context, which is safe because all
// work of one context is ordered on one stream.
struct amt_scratch : amt_scratch_plan {
    amt_ctx* ctx;
    explicit amt_scratch(amt_ctx* c) : ctx(c) {}
    int commit();
};
// copy `bytes` from caller-owned host memory to device memory via the pinned ring (stream ordered)
int amt_param_upload(amt_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);

__host__ __device__ static inline size_t amt_align(size_t n, size_t a = 256) { return (n + a - 1) / a * a; }

static inline int amt_set_device(amt_ctx* ctx) {
    if (!ctx) {
        amt_set_error("null context");
        return AMT_EINVAL;
    }
    AMT_HIP_CHECK(hipSetDevice(ctx->device));
    return AMT_OK;
}

static inline unsigned amt_grid_for(size_t work_items, unsigned block, unsigned max_blocks = 8192) {
    size_t b = (work_items + block - 1) / block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (unsigned)b;
}

// ---- device helpers ----------------------------------------------------------------------------
// scipy.ndimage index extension.  Returns -1 for AMT_MODE_CONSTANT out of range.
__device__ __forceinline__ int amt_map_index(int i, int n, int mode) {
    if (i >= 0 && i < n) return i;
    switch (mode) {
        case AMT_MODE_NEAREST:
            return i < 0 ? 0 : n - 1;
        case AMT_MODE_REFLECT: {
            int p = 2 * n;
            int m = i % p;
            if (m < 0) m += p;
            return m < n ? m : p - 1 - m;
        }
        case AMT_MODE_MIRROR: {
            if (n == 1) return 0;
            int p = 2 * n - 2;
            int m = i % p;
            if (m < 0) m += p;
            return m < n ? m : p - m;
        }
        case AMT_MODE_WRAP: {
            int m = i % n;
            if (m < 0) m += n;
            return m;
        }
        default:
            return -1;
    }
}

// order-preserving map float64 <-> uint64 (for atomic min/max and radix select)
__device__ __forceinline__ unsigned long long amt_f64_key(double v) {
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double amt_key_f64(unsigned long long k) {
    unsigned long long u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}
