// Context, memory, timers and error plumbing of libamt_hip.so.
#include "amt_common.h"

#include <cstdlib>

static thread_local char g_err[1024] = "";

void amt_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int amt_check_operands(amt_ctx* ctx, const char* op, const amt_operand* ops, int n) {
    amt_note_op(ctx);
    for (int i = 0; i < n; ++i) {
        const amt_operand& a = ops[i];
        if (!a.ptr || !a.bytes) continue;
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.ptr);
        const uintptr_t a1 = a.bytes > UINTPTR_MAX - a0 ? UINTPTR_MAX : a0 + a.bytes;
        for (int j = i + 1; j < n; ++j) {
            const amt_operand& b = ops[j];
            if (!b.ptr || !b.bytes || !(a.output || b.output)) continue;
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(b.ptr);
            const uintptr_t b1 = b.bytes > UINTPTR_MAX - b0 ? UINTPTR_MAX : b0 + b.bytes;
            if (a1 <= b0 || b1 <= a0) continue;
            const amt_operand& o = a.output ? a : b;   // the output of the pair names it first
            const amt_operand& x = a.output ? b : a;
            const bool allowed = (a.output && !b.output && ((a.inplace >> j) & 1u)) ||
                                 (b.output && !a.output && ((b.inplace >> i) & 1u));
            if (!allowed) {
                amt_set_error("%s: %s must not alias %s, nor overlap it in part", op, o.name, x.name);
                return AMT_EINVAL;
            }
            if (a0 != b0 || a.bytes != b.bytes || a.elem != b.elem) {
                amt_set_error("%s: %s may alias %s only in place (same start, same length, same element size); this "
                              "overlap is partial",
                              op, o.name, x.name);
                return AMT_EINVAL;
            }
        }
    }
    return AMT_OK;
}

extern "C" const char* amt_last_error(void) { return g_err; }
extern "C" const char* amt_version(void) { return "amt_hip 0.1 (gfx950)"; }

extern "C" int amt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int fork_default();

static int ctx_create_common(int device, hipStream_t stream, bool own, amt_ctx** out) {
    AMT_REQUIRE(out != nullptr, "amt_ctx_create: out is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        amt_set_error("no HIP device available (%s); libamt_hip requires an MI355X (gfx950)",
                      e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return AMT_ENODEV;
    }
    AMT_REQUIRE(device >= 0 && device < n, "amt_ctx_create: device %d out of range (have %d)", device, n);
    AMT_HIP_CHECK(hipSetDevice(device));
    amt_ctx* c = new amt_ctx();
    c->device = device;
    c->own_stream = own;
    c->stream = stream;
    if (own) {
        hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (se != hipSuccess) {
            delete c;
            amt_set_error("hipStreamCreate failed: %s", hipGetErrorString(se));
            return AMT_EHIP;
        }
    }
    c->arena = nullptr;
    c->arena_cap = 0;
    c->mailbox = nullptr;
    c->mailbox_cap = 0;
    c->mailbox_off = 0;
    c->aux_ready = false;
    c->fork = fork_default();
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess)
        c->num_cus = prop.multiProcessorCount;
    else
        c->num_cus = 256;
    c->mailbox_cap = 1u << 20;
    if (hipHostMalloc((void**)&c->mailbox, c->mailbox_cap, hipHostMallocDefault) != hipSuccess) {
        c->mailbox = nullptr;
        c->mailbox_cap = 0;
    }
    *out = c;
    return AMT_OK;
}

extern "C" int amt_ctx_create(int device, amt_ctx** out) { return ctx_create_common(device, nullptr, true, out); }

extern "C" int amt_ctx_create_on_stream(int device, void* hip_stream, amt_ctx** out) {
    return ctx_create_common(device, (hipStream_t)hip_stream, false, out);
}

extern "C" int amt_ctx_destroy(amt_ctx* ctx) {
    if (!ctx) return AMT_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->dbg_first) (void)hipFree(ctx->dbg_first);
    if (ctx->box_buf) (void)hipFree(ctx->box_buf);
    if (ctx->mailbox) (void)hipHostFree(ctx->mailbox);
    if (ctx->aux_ready) {
        for (int i = 0; i < 3; ++i) (void)hipStreamDestroy(ctx->aux_own[i]);
        for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ctx->ev[i]);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return AMT_OK;
}

extern "C" int amt_device_name(amt_ctx* ctx, char* buf, int buflen) {
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(buf && buflen > 0, "amt_device_name: bad buffer");
    hipDeviceProp_t prop;
    AMT_HIP_CHECK(hipGetDeviceProperties(&prop, ctx->device));
    snprintf(buf, (size_t)buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return AMT_OK;
}

// AMT_DEBUG_POISON=1 (diagnostic): every allocation and, at the start of every op, the whole scratch arena are filled
// with 0xCD bytes, so a kernel that relies on "fresh memory is zero" fails deterministically instead of once in a while.
static bool poison_enabled() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("AMT_DEBUG_POISON");
        v = (e && e[0] == '1') ? 1 : 0;
    }
    return v == 1;
}
bool amt_poison_enabled() { return poison_enabled(); }

// ---- the hand-off of label boxes (amt_common.h: amt_ctx::box_note) ----
int amt_box_buffer(amt_ctx* ctx, size_t ints, int** buf) {
    ctx->box_note.valid = false;  // whatever the buffer held is about to be replaced
    if (ints > ctx->box_cap) {
        // an earlier hand-off's copy may still be reading the buffer: drain the stream before freeing
        AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (ctx->box_buf) AMT_HIP_CHECK(hipFree(ctx->box_buf));
        ctx->box_buf = nullptr;
        ctx->box_cap = 0;
        const size_t cap = ints + ints / 4;
        hipError_t e = hipMalloc((void**)&ctx->box_buf, cap * sizeof(int));
        if (e != hipSuccess) {
            amt_set_error("label box buffer allocation of %zu bytes failed: %s", cap * sizeof(int), hipGetErrorString(e));
            return AMT_ENOMEM;
        }
        ctx->box_cap = cap;
    }
    *buf = ctx->box_buf;
    return AMT_OK;
}

void amt_box_note_leave(amt_ctx* ctx, const void* labels, int nplanes, int H, int W, int max_label) {
    // a borrowed stream (amt_ctx_create_on_stream) carries its owner's work between two calls of the library, ordered
    // and unseen: no note there
    if (!ctx->own_stream) return;
    ctx->box_note = {true, labels, nplanes, H, W, max_label, ctx->device, ctx->op_serial};
}

const int* amt_box_note_take(amt_ctx* ctx, const void* labels, int nplanes, int H, int W, int max_label) {
    const auto n = ctx->box_note;
    ctx->box_note.valid = false;  // one look, used or not
    const bool hit = n.valid && n.serial + 1 == ctx->op_serial && n.labels == labels && n.nplanes == nplanes && n.H == H &&
                     n.W == W && n.max_label == max_label && n.device == ctx->device && ctx->box_buf;
    return hit ? ctx->box_buf : nullptr;
}

int amt_scratch::commit() {
    AMT_REQUIRE(!overflow, "scratch plan: more than %d buffers declared", AMT_SCRATCH_SLOTS);
    ctx->plan_valid = false;
    const size_t total_bytes = total + 4096;  // total is a multiple of 256
    if (total_bytes > ctx->arena_cap) {
        // previous users of the arena are ordered before us on the stream; drain it before freeing
        AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (ctx->arena) AMT_HIP_CHECK(hipFree(ctx->arena));
        ctx->arena = nullptr;
        ctx->arena_cap = 0;
        size_t cap = total_bytes + total_bytes / 4;
        hipError_t e = hipMalloc((void**)&ctx->arena, cap);
        if (e != hipSuccess) {
            amt_set_error("scratch arena allocation of %zu bytes failed: %s", cap, hipGetErrorString(e));
            return AMT_ENOMEM;
        }
        ctx->arena_cap = cap;
    }
    if (poison_enabled()) AMT_HIP_CHECK(hipMemsetAsync(ctx->arena, 0xCD, ctx->arena_cap, ctx->stream));
    fill(ctx->arena);
    memcpy(ctx->plan_off, off, sizeof(size_t) * count);
    memcpy(ctx->plan_len, len, sizeof(size_t) * count);
    ctx->plan_count = count;
    ctx->plan_total = total;
    ctx->plan_valid = true;
    return AMT_OK;
}

// ---- AMT_DEBUG_POISON=1: the padding behind every buffer of the last plan and the arena beyond its total are red zones
// What a clean answer does NOT say: only the LAST committed plan is known, so an entry point that commits scratch more than
// once (a sub-op with a plan of its own) is checked for its final plan alone; a write that lands inside a neighbouring
// buffer (a take whose length is a multiple of 256 has no padding) is not seen; and the caller looks after the entry point
// has returned, not between its kernels.
// (commit() left 0xCD there and no kernel owns them).  ranges: [beg, end) byte offsets into the arena, the last one the tail.
struct scratch_ranges {
    unsigned long long beg[AMT_SCRATCH_SLOTS + 1], end[AMT_SCRATCH_SLOTS + 1];
    int n;
};

__global__ void __launch_bounds__(256) scratch_check_kernel(const unsigned char* __restrict__ arena, scratch_ranges r,
                                                            unsigned long long* __restrict__ first) {
    const size_t gt = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    // paddings: shorter than 256 bytes each; a grid-stride loop over 256 byte positions per buffer, so that every
    // buffer's padding is looked at however small the grid is
    for (size_t k = gt; k < (size_t)(r.n - 1) * 256; k += nthreads) {
        const unsigned long long o = r.beg[k / 256] + k % 256;
        if (o < r.end[k / 256] && arena[o] != 0xCD) atomicMin(first, o);
    }
    // the tail starts on a 256-byte boundary: 4-byte words, then the odd bytes
    const unsigned long long tb = r.beg[r.n - 1], te = r.end[r.n - 1];
    const size_t words = (size_t)(te - tb) / 4;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(arena + tb);
    for (size_t i = gt; i < words; i += nthreads) {
        const uint32_t v = w[i] ^ 0xCDCDCDCDu;
        if (v) atomicMin(first, tb + i * 4 + (unsigned)(__ffs((int)v) - 1) / 8);
    }
    for (unsigned long long o = tb + words * 4 + gt; o < te; o += nthreads)
        if (arena[o] != 0xCD) atomicMin(first, o);
}

extern "C" int amt_debug_scratch_check(amt_ctx* ctx, int* slot, uint64_t* offset) {
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(slot && offset, "amt_debug_scratch_check: null argument");
    *slot = -1;
    *offset = 0;
    AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (!poison_enabled() || !ctx->plan_valid || !ctx->arena) return AMT_OK;
    scratch_ranges r;
    const int count = ctx->plan_count;
    for (int i = 0; i < count; ++i) {
        r.beg[i] = ctx->plan_off[i] + ctx->plan_len[i];
        r.end[i] = i + 1 < count ? ctx->plan_off[i + 1] : ctx->plan_total;
    }
    r.beg[count] = ctx->plan_total;
    r.end[count] = ctx->arena_cap;
    r.n = count + 1;
    if (!ctx->dbg_first) AMT_HIP_CHECK(hipMalloc((void**)&ctx->dbg_first, sizeof(unsigned long long)));
    AMT_HIP_CHECK(hipMemsetAsync(ctx->dbg_first, 0xFF, sizeof(unsigned long long), ctx->stream));
    const size_t work = (size_t)(r.end[count] - r.beg[count]) / 4 + (size_t)r.n * 256;
    hipLaunchKernelGGL(scratch_check_kernel, dim3(amt_grid_for(work, 256 * 16, 4096)), dim3(256), 0, ctx->stream,
                       (const unsigned char*)ctx->arena, r, ctx->dbg_first);
    AMT_LAUNCH_CHECK();
    unsigned long long first = 0;
    AMT_HIP_CHECK(hipMemcpyAsync(&first, ctx->dbg_first, sizeof(first), hipMemcpyDeviceToHost, ctx->stream));
    AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (first == ~0ull) return AMT_OK;
    for (int i = 0; i <= count; ++i)
        if (first >= r.beg[i] && first < r.end[i]) *slot = i;
    *offset = first;
    return AMT_OK;
}

// AMT_FORK=0 keeps every kernel of an op on the context's single stream (no auxiliary streams); 1..3 = that many
static int fork_default() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("AMT_FORK");
        v = (e && e[0] >= '0' && e[0] <= '3') ? e[0] - '0' : 3;
    }
    return v;
}

// Per context: a process that already runs several contexts side by side (one per HIP stream) gains nothing from the
// auxiliary streams -- their events and the extra hardware queues cost more than the overlap inside one op brings
// (bench.py, 4 contexts: 11.1 k FOV/s without, 10.2 k with) -- while a single context needs them (watershed stage
// 1.80 ms against 2.32 ms per 32 FOVs).
extern "C" int amt_ctx_set_fork(amt_ctx* ctx, int enable) {
    AMT_REQUIRE(ctx != nullptr, "ctx_set_fork: null context");
    ctx->fork = enable < 0 ? 0 : (enable > 3 ? 3 : enable);  // 1 ("on") .. 3 = that many auxiliary streams
    return AMT_OK;
}

int amt_fork(amt_ctx* ctx) {
    const int n = ctx->fork;
    if (n == 0) {
        ctx->aux[0] = ctx->aux[1] = ctx->aux[2] = ctx->stream;
        return AMT_OK;
    }
    if (!ctx->aux_ready) {
        for (int i = 0; i < 3; ++i) AMT_HIP_CHECK(hipStreamCreateWithFlags(&ctx->aux_own[i], hipStreamNonBlocking));
        for (int i = 0; i < 4; ++i) AMT_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev[i], hipEventDisableTiming));
        ctx->aux_ready = true;
    }
    for (int i = 0; i < 3; ++i) ctx->aux[i] = ctx->aux_own[i % n];
    AMT_HIP_CHECK(hipEventRecord(ctx->ev[0], ctx->stream));
    for (int i = 0; i < n; ++i) AMT_HIP_CHECK(hipStreamWaitEvent(ctx->aux_own[i], ctx->ev[0], 0));
    return AMT_OK;
}

int amt_join(amt_ctx* ctx) {
    const int n = ctx->fork;
    if (n == 0) return AMT_OK;
    for (int i = 0; i < n; ++i) {
        AMT_HIP_CHECK(hipEventRecord(ctx->ev[1 + i], ctx->aux_own[i]));
        AMT_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev[1 + i], 0));
    }
    return AMT_OK;
}

int amt_param_upload(amt_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes) {
    if (bytes == 0) return AMT_OK;
    size_t need = amt_align(bytes, 256);
    if (!ctx->mailbox || need > ctx->mailbox_cap) {
        // too large for the ring: synchronous copy (the caller's buffer is consumed before returning)
        AMT_HIP_CHECK(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
        AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return AMT_OK;
    }
    if (ctx->mailbox_off + need > ctx->mailbox_cap) {
        // wrap: older slots may still be in flight
        AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->mailbox_off = 0;
    }
    char* slot = ctx->mailbox + ctx->mailbox_off;
    ctx->mailbox_off += need;
    memcpy(slot, host_src, bytes);
    AMT_HIP_CHECK(hipMemcpyAsync(dev_dst, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
    return AMT_OK;
}

extern "C" int amt_malloc(amt_ctx* ctx, size_t bytes, void** dptr) {
    amt_note_op(ctx);
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(dptr != nullptr, "amt_malloc: dptr is null");
    if (bytes == 0) bytes = 256;
    hipError_t e = hipMalloc(dptr, bytes);
    if (e != hipSuccess) {
        amt_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return AMT_ENOMEM;
    }
    if (poison_enabled()) {
        AMT_HIP_CHECK(hipMemsetAsync(*dptr, 0xCD, bytes, ctx->stream));
        AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return AMT_OK;
}

extern "C" int amt_free(amt_ctx* ctx, void* dptr) {
    amt_note_op(ctx);
    AMT_TRY(amt_set_device(ctx));
    if (dptr) AMT_HIP_CHECK(hipFree(dptr));
    return AMT_OK;
}

extern "C" int amt_memcpy_h2d(amt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    amt_note_op(ctx);
    AMT_TRY(amt_set_device(ctx));
    if (bytes) AMT_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return AMT_OK;
}
extern "C" int amt_memcpy_d2h(amt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    amt_note_op(ctx);
    AMT_TRY(amt_set_device(ctx));
    if (bytes) AMT_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return AMT_OK;
}
extern "C" int amt_memcpy_d2d(amt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    amt_note_op(ctx);
    AMT_TRY(amt_set_device(ctx));
    if (bytes) AMT_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return AMT_OK;
}
extern "C" int amt_memset(amt_ctx* ctx, void* dst, int value, size_t bytes) {
    amt_note_op(ctx);
    AMT_TRY(amt_set_device(ctx));
    if (bytes) AMT_HIP_CHECK(hipMemsetAsync(dst, value, bytes, ctx->stream));
    return AMT_OK;
}
extern "C" int amt_sync(amt_ctx* ctx) {
    amt_note_op(ctx);
    AMT_TRY(amt_set_device(ctx));
    AMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return AMT_OK;
}

extern "C" int amt_ctx_stream(amt_ctx* ctx, void** hip_stream) {
    AMT_REQUIRE(ctx && hip_stream, "amt_ctx_stream: null argument");
    *hip_stream = (void*)ctx->stream;
    return AMT_OK;
}

extern "C" int amt_stream_wait(amt_ctx* ctx, amt_ctx* other) {
    amt_note_op(ctx);
    // everything enqueued so far on `other`'s stream happens-before what is enqueued next on `ctx`'s stream
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(other != nullptr, "amt_stream_wait: other is null");
    amt_note_op(other);  // its work so far is published: `ctx` may change what it wrote
    AMT_REQUIRE(other->device == ctx->device, "amt_stream_wait: contexts on different devices");
    hipEvent_t ev;
    AMT_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    AMT_HIP_CHECK(hipEventRecord(ev, other->stream));
    AMT_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ev, 0));
    AMT_HIP_CHECK(hipEventDestroy(ev));  // destruction is deferred until the event has completed
    return AMT_OK;
}

// ---- events: ordering between contexts at a RECORDED point (amt_stream_wait orders after everything so far) ----
extern "C" int amt_event_create(amt_ctx* ctx, void** event) {
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(event != nullptr, "amt_event_create: event is null");
    hipEvent_t ev;
    AMT_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    *event = (void*)ev;
    return AMT_OK;
}
extern "C" int amt_event_record(amt_ctx* ctx, void* event) {
    amt_note_op(ctx);  // publishes the context's work so far to whoever waits for the event
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(event != nullptr, "amt_event_record: event is null");
    AMT_HIP_CHECK(hipEventRecord((hipEvent_t)event, ctx->stream));
    return AMT_OK;
}
extern "C" int amt_event_wait(amt_ctx* ctx, void* event) {
    amt_note_op(ctx);
    // what is enqueued next on ctx's stream happens after the event's last record (no-op if never recorded)
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(event != nullptr, "amt_event_wait: event is null");
    AMT_HIP_CHECK(hipStreamWaitEvent(ctx->stream, (hipEvent_t)event, 0));
    return AMT_OK;
}
extern "C" int amt_event_sync(amt_ctx* ctx, void* event) {
    amt_note_op(ctx);  // the host has seen the context's work: it may start anything
    // the HOST waits for the event's last record: a chunked download hands finished chunks to host threads
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(event != nullptr, "amt_event_sync: event is null");
    AMT_HIP_CHECK(hipEventSynchronize((hipEvent_t)event));
    return AMT_OK;
}
extern "C" int amt_event_destroy(amt_ctx* ctx, void* event) {
    AMT_TRY(amt_set_device(ctx));
    if (event) AMT_HIP_CHECK(hipEventDestroy((hipEvent_t)event));
    return AMT_OK;
}

extern "C" int amt_host_alloc(size_t bytes, void** hptr) {
    AMT_REQUIRE(hptr != nullptr, "amt_host_alloc: hptr is null");
    hipError_t e = hipHostMalloc(hptr, bytes ? bytes : 64, hipHostMallocDefault);
    if (e != hipSuccess) {
        amt_set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return AMT_ENOMEM;
    }
    return AMT_OK;
}
extern "C" int amt_host_free(void* hptr) {
    if (hptr) AMT_HIP_CHECK(hipHostFree(hptr));
    return AMT_OK;
}

// Host memcpy with streaming stores: a staging block is written once and next read by the DMA engine, so pulling its
// lines into the cache first (what an ordinary store does) only doubles the destination's traffic.  Plain host code.
extern "C" int amt_host_copy(void* dst, const void* src, size_t bytes) {
    AMT_REQUIRE((dst && src) || bytes == 0, "amt_host_copy: null pointer");
    typedef long long v2di __attribute__((vector_size(16)));
    unsigned char* d = (unsigned char*)dst;
    const unsigned char* s = (const unsigned char*)src;
    size_t head = ((uintptr_t)d & 15) ? 16 - ((uintptr_t)d & 15) : 0;
    if (head > bytes) head = bytes;
    memcpy(d, s, head);
    d += head, s += head, bytes -= head;
    size_t i = 0;
    for (; i + 64 <= bytes; i += 64) {
        v2di a, b, c, e;
        memcpy(&a, s + i, 16);
        memcpy(&b, s + i + 16, 16);
        memcpy(&c, s + i + 32, 16);
        memcpy(&e, s + i + 48, 16);
        __builtin_nontemporal_store(a, (v2di*)(d + i));
        __builtin_nontemporal_store(b, (v2di*)(d + i + 16));
        __builtin_nontemporal_store(c, (v2di*)(d + i + 32));
        __builtin_nontemporal_store(e, (v2di*)(d + i + 48));
    }
    __atomic_thread_fence(__ATOMIC_SEQ_CST);  // streaming stores are weakly ordered: drain them before returning
    memcpy(d + i, s + i, bytes - i);
    return AMT_OK;
}

// Extrema of an integer host array in ONE foreign call (the Python layer's worker threads otherwise make dozens of
// short numpy calls per label image and queue for the interpreter lock between them).  itemsize 1 / 2 / 4 / 8.
template <typename T>
static void host_minmax(const T* p, size_t n, int64_t out[2]) {
    T lo[4] = {p[0], p[0], p[0], p[0]}, hi[4] = {p[0], p[0], p[0], p[0]};
    size_t i = 0;
    for (; i + 4 <= n; i += 4)
        for (int k = 0; k < 4; ++k) {
            const T v = p[i + k];
            lo[k] = v < lo[k] ? v : lo[k];
            hi[k] = v > hi[k] ? v : hi[k];
        }
    for (; i < n; ++i) {
        lo[0] = p[i] < lo[0] ? p[i] : lo[0];
        hi[0] = p[i] > hi[0] ? p[i] : hi[0];
    }
    for (int k = 1; k < 4; ++k) {
        lo[0] = lo[k] < lo[0] ? lo[k] : lo[0];
        hi[0] = hi[k] > hi[0] ? hi[k] : hi[0];
    }
    out[0] = (int64_t)lo[0];
    out[1] = (int64_t)hi[0];
}

extern "C" int amt_host_minmax_int(const void* src, int itemsize, int is_signed, size_t n, int64_t* out) {
    AMT_REQUIRE(src && out && n > 0, "amt_host_minmax_int: empty input");
    switch (itemsize * 2 + (is_signed ? 1 : 0)) {
        case 2: host_minmax((const uint8_t*)src, n, out); break;
        case 3: host_minmax((const int8_t*)src, n, out); break;
        case 4: host_minmax((const uint16_t*)src, n, out); break;
        case 5: host_minmax((const int16_t*)src, n, out); break;
        case 8: host_minmax((const uint32_t*)src, n, out); break;
        case 9: host_minmax((const int32_t*)src, n, out); break;
        case 17: host_minmax((const int64_t*)src, n, out); break;
        default: AMT_REQUIRE(false, "amt_host_minmax_int: unsupported element type (itemsize %d, signed %d)", itemsize, is_signed);
    }
    return AMT_OK;
}

// int64 -> int32 (label images travel as int32) with streaming stores, and the extrema of the SOURCE values in the
// same pass when `minmax` is given.  Values are truncated like a C cast; callers check the range from the extrema.
extern "C" int amt_host_narrow_i64_i32(int32_t* dst, const int64_t* src, size_t n, int64_t* minmax) {
    AMT_REQUIRE((dst && src) || n == 0, "amt_host_narrow_i64_i32: null pointer");
    int64_t lo = n ? src[0] : 0, hi = lo;
    size_t i = 0;
    typedef int v4si __attribute__((vector_size(16)));
    if (((uintptr_t)dst & 15) == 0) {
        for (; i + 4 <= n; i += 4) {
            const int64_t a = src[i], b = src[i + 1], c = src[i + 2], d = src[i + 3];
            if (minmax) {
                const int64_t l1 = a < b ? a : b, l2 = c < d ? c : d, h1 = a > b ? a : b, h2 = c > d ? c : d;
                const int64_t l = l1 < l2 ? l1 : l2, h = h1 > h2 ? h1 : h2;
                lo = l < lo ? l : lo;
                hi = h > hi ? h : hi;
            }
            const v4si v = {(int)a, (int)b, (int)c, (int)d};
            __builtin_nontemporal_store(v, (v4si*)(dst + i));
        }
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
    }
    for (; i < n; ++i) {
        const int64_t a = src[i];
        if (minmax) {
            lo = a < lo ? a : lo;
            hi = a > hi ? a : hi;
        }
        dst[i] = (int32_t)a;
    }
    if (minmax) {
        minmax[0] = lo;
        minmax[1] = hi;
    }
    return AMT_OK;
}

struct amt_timer {
    hipEvent_t start, stop;
};

extern "C" int amt_timer_create(amt_ctx* ctx, void** timer) {
    AMT_TRY(amt_set_device(ctx));
    AMT_REQUIRE(timer != nullptr, "amt_timer_create: null");
    amt_timer* t = new amt_timer();
    AMT_HIP_CHECK(hipEventCreate(&t->start));
    AMT_HIP_CHECK(hipEventCreate(&t->stop));
    *timer = t;
    return AMT_OK;
}
extern "C" int amt_timer_start(amt_ctx* ctx, void* timer) {
    AMT_TRY(amt_set_device(ctx));
    AMT_HIP_CHECK(hipEventRecord(((amt_timer*)timer)->start, ctx->stream));
    return AMT_OK;
}
extern "C" int amt_timer_stop(amt_ctx* ctx, void* timer) {
    AMT_TRY(amt_set_device(ctx));
    AMT_HIP_CHECK(hipEventRecord(((amt_timer*)timer)->stop, ctx->stream));
    return AMT_OK;
}
extern "C" int amt_timer_elapsed_ms(amt_ctx* ctx, void* timer, float* ms) {
    amt_note_op(ctx);  // a host synchronisation on the stop event
    AMT_TRY(amt_set_device(ctx));
    amt_timer* t = (amt_timer*)timer;
    AMT_HIP_CHECK(hipEventSynchronize(t->stop));
    AMT_HIP_CHECK(hipEventElapsedTime(ms, t->start, t->stop));
    return AMT_OK;
}
extern "C" int amt_timer_destroy(amt_ctx* ctx, void* timer) {
    AMT_TRY(amt_set_device(ctx));
    amt_timer* t = (amt_timer*)timer;
    if (t) {
        (void)hipEventDestroy(t->start);
        (void)hipEventDestroy(t->stop);
        delete t;
    }
    return AMT_OK;
}
