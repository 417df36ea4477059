// How libnbls_hip.so owns memory: one value type per HBM allocation (dev_buf) and per pinned one (pinned_buf).  Each
// carries its pointer, its capacity and — for the plan tables — whether it is a place inside the plan arena, which is
// never freed on its own.  Neither type knows the handle, its error text or its streams; the destructor frees, so a
// struct of these needs no free list.  Nothing here synchronises: hipFree waits for the device, the callers know when.
#pragma once
#include <hip/hip_runtime_api.h>

template <typename T>
struct dev_buf {
    T* p = nullptr;
    size_t cap = 0;          // bytes of an allocation of its own (0 for a place in the arena)
    bool in_arena = false;   // p points into another buffer's allocation

    dev_buf() = default;
    dev_buf(const dev_buf&) = delete;              // a copy would free twice
    dev_buf& operator=(const dev_buf&) = delete;
    ~dev_buf() { release(); }
    operator T*() const { return p; }

    // At least `bytes` (0: 8 bytes), contents NOT kept: an allocation that is big enough stays, anything else is freed
    // and made anew.  After a failure the buffer is empty.
    hipError_t grow(size_t bytes) {
        if (p && !in_arena && cap >= bytes) return hipSuccess;
        release();
        if (bytes == 0) bytes = 8;
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) p = nullptr;
        else cap = bytes;
        return e;
    }
    void release() {
        if (p && !in_arena) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        in_arena = false;
    }
    // Become the place `at` of the arena (an allocation of its own goes first).
    void place(T* at) {
        release();
        p = at;
        in_arena = true;
    }
    // A place in the arena is forgotten: nothing allocated.  An allocation of its own stays.
    void leave_arena() {
        if (in_arena) release();
    }
    // Take over the fresh allocation q of `bytes` (hipMalloc) in place of the present one.
    void adopt(T* q, size_t bytes) {
        release();
        p = q;
        cap = bytes;
    }
};

struct pinned_buf {
    unsigned char* p = nullptr;
    size_t cap = 0;

    pinned_buf() = default;
    pinned_buf(const pinned_buf&) = delete;
    pinned_buf& operator=(const pinned_buf&) = delete;
    ~pinned_buf() { release(); }
    operator unsigned char*() const { return p; }

    hipError_t grow(size_t bytes) {                // as dev_buf::grow
        if (p && cap >= bytes) return hipSuccess;
        release();
        if (bytes == 0) bytes = 8;
        const hipError_t e = hipHostMalloc((void**)&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) p = nullptr;
        else cap = bytes;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};
