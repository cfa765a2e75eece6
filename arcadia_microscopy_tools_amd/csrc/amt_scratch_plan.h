// Layout rule of an op's device scratch (no HIP here: a host compiler can test it).
// An op declares every buffer once with take(); each take is rounded up to 256 bytes, offsets follow the order of the
// declarations, and the reservation is the end of the last take.  The pointers are written by fill(), i.e. only once
// the reservation of exactly that total exists; a pointer whose take was skipped by a condition stays nullptr.
// len[] keeps every take's exact byte length: what lies between off[i] + len[i] and the next offset is padding no kernel
// may write (amt_debug_scratch_check).
#pragma once
#include <cstddef>
#include <cstring>

// the largest op (amt_cellpose_masks_ex with its later stages) declares 30 buffers
constexpr int AMT_SCRATCH_SLOTS = 48;

struct amt_scratch_plan {
    void* slot[AMT_SCRATCH_SLOTS];  // address of the caller's pointer variable
    size_t off[AMT_SCRATCH_SLOTS];
    size_t len[AMT_SCRATCH_SLOTS];  // exact bytes of the take (off[i] + len[i] <= the next offset)
    int count = 0;
    size_t total = 0;
    bool overflow = false;  // one take too many for the table: the plan must not be committed

    template <typename T>
    void take(T*& p, size_t n) {
        p = nullptr;
        if (count == AMT_SCRATCH_SLOTS) {
            overflow = true;
            return;
        }
        slot[count] = &p;
        off[count] = total;
        len[count++] = n * sizeof(T);
        total += (n * sizeof(T) + 255) / 256 * 256;
    }

    void fill(char* base) const {
        for (int i = 0; i < count; ++i) {
            char* p = base + off[i];
            memcpy(slot[i], &p, sizeof(p));  // every T* has the representation of a char*
        }
    }
};

// A buffer declared into a plan in one statement: converts to its T* (nullptr before the commit, and for good when
// `wanted` was false).  It must live until the plan is committed, and does not move: the plan holds the address of p.
// Where the ADDRESS of the pointer is needed (a kernel argument array), &buf is refused: write &buf.p.
template <typename T>
struct amt_buf {
    T* p = nullptr;
    amt_buf(amt_scratch_plan& s, size_t n, bool wanted = true) {
        if (wanted) s.take(p, n);
    }
    amt_buf(const amt_buf&) = delete;
    void operator&() const = delete;
    operator T*() const { return p; }
};
