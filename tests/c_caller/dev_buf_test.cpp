// Host test of csrc/dev_buf.h (the owning types of every device and pinned buffer of a handle) against an allocator
// defined HERE: the four HIP entry points the header calls are malloc / free with a count of live allocations, a record
// of every pointer freed and a switch that makes the n-th allocation fail.  No HIP library is linked, no GPU touched.
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__
//       -I/opt/rocm/include -I narrow_band_least_squares_amd/csrc tests/c_caller/dev_buf_test.cpp -o dev_buf_test
// Prints "ok <checks>"; exit code 1 at the first failed check.
#include "dev_buf.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct Alloc { void* p; size_t bytes; bool pinned; };
std::vector<Alloc> g_live;
std::vector<void*> g_freed;        // every pointer handed to hipFree / hipHostFree, in order
long g_allocs = 0;                 // successful allocations
long g_fail_at = 0;                // > 0: that many allocator calls from now, the last of them fails
long g_bad = 0;                    // frees of something that is no live allocation of the right kind
long g_checks = 0;

hipError_t fake_alloc(void** out, size_t bytes, bool pinned) {
    if (g_fail_at > 0 && --g_fail_at == 0) { *out = (void*)(uintptr_t)0xdead; return hipErrorOutOfMemory; }   // (garbage, as a failed call may leave)
    *out = malloc(bytes);
    g_live.push_back({*out, bytes, pinned});
    ++g_allocs;
    return hipSuccess;
}

hipError_t fake_free(void* p, bool pinned) {
    g_freed.push_back(p);
    for (size_t i = 0; i < g_live.size(); ++i)
        if (g_live[i].p == p && g_live[i].pinned == pinned) {
            free(p);
            g_live.erase(g_live.begin() + (long)i);
            return hipSuccess;
        }
    ++g_bad;
    return hipErrorInvalidValue;
}

size_t live_bytes(const void* p) {
    for (const Alloc& a : g_live) if (a.p == p) return a.bytes;
    return 0;
}

bool was_freed(const void* p) {
    for (const void* f : g_freed) if (f == p) return true;
    return false;
}

#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }   \
    } while (0)

// grow / release / destructor, the same for both types
template <typename B>
void grow_and_release() {
    const size_t live0 = g_live.size();
    {
        B b;
        CHECK(b.p == nullptr && b.cap == 0 && !b);
        long a0 = g_allocs; size_t f0 = g_freed.size();
        CHECK(b.grow(100) == hipSuccess);
        CHECK(b.p && b.cap == 100 && live_bytes(b.p) == 100 && g_allocs == a0 + 1 && g_freed.size() == f0);
        // smaller or equal: no allocator call, the pointer stays
        auto* const p100 = b.p;
        a0 = g_allocs; f0 = g_freed.size();
        CHECK(b.grow(100) == hipSuccess && b.grow(40) == hipSuccess && b.grow(0) == hipSuccess);
        CHECK(b.p == p100 && b.cap == 100 && g_allocs == a0 && g_freed.size() == f0);
        // larger: one free (of the old block), one allocation
        CHECK(b.grow(101) == hipSuccess);
        CHECK(g_allocs == a0 + 1 && g_freed.size() == f0 + 1 && g_freed.back() == (void*)p100);
        CHECK(b.cap == 101 && live_bytes(b.p) == 101 && g_live.size() == live0 + 1);
        // a failed grow leaves nothing (the old block is gone, the garbage the allocator left is not kept); the next one works
        auto* const p101 = b.p;
        g_fail_at = 1;
        CHECK(b.grow(500) == hipErrorOutOfMemory);
        CHECK(b.p == nullptr && b.cap == 0 && was_freed(p101) && g_live.size() == live0);
        CHECK(b.grow(500) == hipSuccess && b.p && b.cap == 500 && live_bytes(b.p) == 500);
        // release: one free, empty afterwards, and again is no call at all
        auto* const p500 = b.p;
        f0 = g_freed.size();
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && g_freed.size() == f0 + 1 && g_freed.back() == (void*)p500);
        b.release();
        CHECK(g_freed.size() == f0 + 1);
        // grow(0) on an empty buffer: 8 bytes
        CHECK(b.grow(0) == hipSuccess && b.cap == 8 && live_bytes(b.p) == 8);
        // the failing allocation may be the n-th: the first of these two succeeds
        B c;
        g_fail_at = 2;
        CHECK(b.grow(64) == hipSuccess && c.grow(64) == hipErrorOutOfMemory && c.p == nullptr && c.cap == 0);
        CHECK(g_live.size() == live0 + 1);
    }   // the destructors: b's block goes, the empty c calls nothing
    CHECK(g_live.size() == live0 && g_bad == 0);
    {   // a buffer that never held anything (a handle whose creation failed half-way) is destroyed without a call
        const size_t f0 = g_freed.size();
        { B never; (void)never; }
        CHECK(g_freed.size() == f0);
    }
}

void arena_places() {
    const size_t live0 = g_live.size();
    const size_t f_begin = g_freed.size();
    unsigned char* slot[3];
    {
        dev_buf<unsigned char> arena;
        CHECK(arena.grow(4096) == hipSuccess && !arena.in_arena);
        for (int i = 0; i < 3; ++i) slot[i] = arena.p + 64 * i;
        dev_buf<double> a, b;
        dev_buf<int32_t> c;
        // place on an empty buffer: no call
        size_t f0 = g_freed.size(); long a0 = g_allocs;
        a.place((double*)slot[0]);
        CHECK((void*)a.p == (void*)slot[0] && a.in_arena && a.cap == 0 && g_freed.size() == f0 && g_allocs == a0);
        // place on a buffer with an allocation of its own: that is freed, once
        CHECK(b.grow(256) == hipSuccess);
        double* const own = b.p;
        f0 = g_freed.size();
        b.place((double*)slot[1]);
        CHECK(g_freed.size() == f0 + 1 && g_freed.back() == (void*)own && b.in_arena && (void*)b.p == (void*)slot[1]);
        // place on an arena place (the next plan): frees nothing
        f0 = g_freed.size();
        b.place((double*)slot[2]);
        b.place((double*)slot[1]);
        c.place((int32_t*)slot[2]);
        CHECK(g_freed.size() == f0 && (void*)b.p == (void*)slot[1] && c.in_arena);
        // the conversions the launchers rely on: pointer value, arithmetic, null test
        double* raw = a;
        CHECK(raw == (double*)slot[0] && a + 2 == raw + 2 && a && (const double*)a == raw);
        // leave_arena, then grow: an allocation of its own, the interior pointer is never freed
        a0 = g_allocs; f0 = g_freed.size();
        a.leave_arena();
        CHECK(a.p == nullptr && a.cap == 0 && !a.in_arena && g_freed.size() == f0);
        CHECK(a.grow(48) == hipSuccess && !a.in_arena && a.cap == 48 && live_bytes(a.p) == 48 && g_allocs == a0 + 1 && g_freed.size() == f0);
        // leave_arena on an allocation of its own keeps it
        double* const a48 = a.p;
        a.leave_arena();
        CHECK(a.p == a48 && a.cap == 48 && g_freed.size() == f0);
        // back into the arena and out again through grow alone: still no free of a place
        a.place((double*)slot[0]);
        CHECK(g_freed.size() == f0 + 1 && g_freed.back() == (void*)a48);
        CHECK(a.grow(0) == hipSuccess && !a.in_arena && a.cap == 8 && live_bytes(a.p) == 8);    // (a place has no capacity to keep)
        a.place((double*)slot[0]);
        // release of a place: no call
        f0 = g_freed.size();
        b.release();
        CHECK(b.p == nullptr && !b.in_arena && b.cap == 0 && g_freed.size() == f0);
        b.place((double*)slot[1]);
    }   // destructors in reverse order: c, b, a are places (no call), the arena's block is freed once
    // no interior place was ever handed to hipFree; slot[0] IS the arena's base address: freed once, by the arena
    long frees[3] = {0, 0, 0};
    for (size_t k = f_begin; k < g_freed.size(); ++k)
        for (int i = 0; i < 3; ++i) frees[i] += g_freed[k] == (void*)slot[i];
    CHECK(frees[0] == 1 && frees[1] == 0 && frees[2] == 0);
    CHECK(g_live.size() == live0 && g_bad == 0);
}

void adopt_block() {
    const size_t live0 = g_live.size();
    unsigned char* fresh = nullptr;
    {
        dev_buf<unsigned char> res;
        CHECK(res.grow(72) == hipSuccess);
        unsigned char* const old = res.p;
        CHECK(hipMalloc((void**)&fresh, 4096) == hipSuccess);
        const size_t f0 = g_freed.size();
        res.adopt(fresh, 4096);
        CHECK(res.p == fresh && res.cap == 4096 && !res.in_arena && g_freed.size() == f0 + 1 && g_freed.back() == (void*)old);
        // what it adopted is its own: kept by a smaller grow, freed by the destructor
        CHECK(res.grow(4096) == hipSuccess && res.p == fresh && g_freed.size() == f0 + 1);
    }
    CHECK(g_freed.back() == (void*)fresh && g_live.size() == live0 && g_bad == 0);
}

}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) { return fake_alloc(ptr, size, false); }
hipError_t hipFree(void* ptr) { return fake_free(ptr, false); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int flags) { return flags == hipHostMallocDefault ? fake_alloc(ptr, size, true) : hipErrorInvalidValue; }
hipError_t hipHostFree(void* ptr) { return fake_free(ptr, true); }
}

int main() {
    grow_and_release<dev_buf<double>>();
    grow_and_release<dev_buf<unsigned char>>();
    grow_and_release<pinned_buf>();
    arena_places();
    adopt_block();
    CHECK(g_live.empty() && g_bad == 0);
    printf("ok %ld\n", g_checks);
    return 0;
}
