"""The layout rule of the ops' device scratch (csrc/amt_scratch_plan.h), checked on the CPU: the header has no HIP
include, so a few lines of C++ built with the system compiler exercise exactly the code the library compiles."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include "amt_scratch_plan.h"

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    char* const base = reinterpret_cast<char*>(uintptr_t(1) << 40);  // a fake arena: never dereferenced
    amt_scratch_plan s;
    int *a, *skipped = nullptr;
    double* b;
    unsigned char *empty, *c;
    const bool runs = false;
    s.take(a, 3);        // 12 bytes -> one 256-byte slot
    s.take(b, 33);       // 264 bytes -> two
    s.take(empty, 0);    // a zero-count take is legal and occupies nothing
    if (runs) s.take(skipped, 100);
    amt_buf<short> h(s, 1), h_skipped(s, 1000, runs);
    s.take(c, 257);
    CHECK(a == nullptr && b == nullptr && (short*)h == nullptr);  // no pointer before the fill
    CHECK(!s.overflow && s.count == 5);
    const size_t want[5] = {0, 256, 768, 768, 1024};  // offsets follow the order of the declarations
    for (int i = 0; i < 5; ++i) CHECK(s.off[i] == want[i] && s.off[i] % 256 == 0);
    CHECK(s.total == 1024 + 512);  // the end of the last take
    // every take's exact byte length is kept beside its offset: what follows it up to the next offset is padding
    const size_t want_len[5] = {3 * sizeof(int), 33 * sizeof(double), 0, sizeof(short), 257};
    for (int i = 0; i < 5; ++i) {
        CHECK(s.len[i] == want_len[i]);
        CHECK(s.off[i] + s.len[i] <= (i + 1 < 5 ? s.off[i + 1] : s.total));
        CHECK((i + 1 < 5 ? s.off[i + 1] : s.total) - (s.off[i] + s.len[i]) < 256);  // less than one rounding unit
    }
    s.fill(base);
    CHECK((char*)a == base && (char*)b == base + 256 && (char*)empty == base + 768 && (char*)(short*)h == base + 768);
    CHECK((char*)c == base + 1024);
    CHECK(skipped == nullptr && (short*)h_skipped == nullptr);  // a take skipped by its condition stays null

    amt_scratch_plan t;
    int* p[AMT_SCRATCH_SLOTS + 1];
    for (int i = 0; i < AMT_SCRATCH_SLOTS; ++i) t.take(p[i], 1);
    CHECK(!t.overflow && t.count == AMT_SCRATCH_SLOTS && t.total == (size_t)256 * AMT_SCRATCH_SLOTS);
    CHECK(t.len[0] == sizeof(int) && t.len[AMT_SCRATCH_SLOTS - 1] == sizeof(int));
    t.take(p[AMT_SCRATCH_SLOTS], 1);  // one take too many for the table is reported, not dropped silently
    CHECK(t.overflow && t.count == AMT_SCRATCH_SLOTS && p[AMT_SCRATCH_SLOTS] == nullptr);
    std::printf("ok\n");
    return 0;
}
"""


def test_scratch_plan_layout(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found (g++ / c++ / clang++)")
    src = tmp_path / "plan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "plan"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_no_op_sizes_its_scratch_by_hand():
    """Arena memory is reachable only through a committed plan: the old begin / take pair is gone from every op."""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(".hip"):
            text = open(os.path.join(CSRC, name)).read()
            for word in ("amt_arena_begin", "amt_arena_take", "arena_take_t"):
                assert word not in text, f"{name} still uses {word}"
