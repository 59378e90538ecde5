// prt_devmem.h — the owners of a context's device memory, pinned host words and events (DESIGN.md "Ownership").
//
// Every allocation of prt_api.cpp is a member or a local of one of the three types below and is freed by destruction (or by
// assignment of a fresh value) and nowhere else.  The owners reach the runtime through the plain functions declared first:
// one link-time seam.  prt_api.cpp defines them over HIP and keeps the process-wide counters of prt_device_memory_info there;
// tests/devmem_owner.cpp defines them over malloc and a counter, which makes this header testable without a GPU.
// Included by the .cpp units only.
#pragma once

#include <cstddef>

// ---- the seam: 0 = success, anything else is the runtime's own error code ----
int prt_dev_alloc(void** p, size_t bytes);
void prt_dev_free(void* p, size_t bytes);
int prt_dev_copy_in(void* dst, const void* src, size_t bytes);  // host -> device, blocking
void prt_dev_adopted(size_t bytes);  // an array allocated elsewhere (bvh_gpu.hip) enters the books ...
void prt_dev_taken(size_t bytes);    // ... or one of ours leaves them unfreed
int prt_pinned_alloc(void** p, size_t bytes);
void prt_pinned_free(void* p);
int prt_event_create(void** ev, bool timing);
void prt_event_destroy(void* ev);

// A device allocation.  ensure() only grows it; a failed ensure leaves it empty.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, bytes = o.bytes;
            o.p = nullptr, o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    void release() {
        if (p) prt_dev_free(p, bytes);
        p = nullptr, bytes = 0;
    }
    // Release first, then allocate: the old and the new block never exist together.
    int ensure(size_t need) {
        if (need <= bytes) return 0;
        release();
        const int e = prt_dev_alloc(&p, need);
        if (e) p = nullptr;
        else bytes = need;
        return e;
    }
    // A fresh block of max(n, min_bytes) bytes holding the n bytes at src.
    int alloc_copy(const void* src, size_t n, size_t min_bytes = 16) {
        release();
        const int e = ensure(n > min_bytes ? n : min_bytes);
        return (e || !n) ? e : prt_dev_copy_in(p, src, n);
    }
    // Hand-over of an array another unit allocated, and back.
    void adopt(void* ptr, size_t n) {
        release();
        if (!ptr) return;
        p = ptr, bytes = n;
        prt_dev_adopted(n);
    }
    void* take() {
        void* q = p;
        if (q) prt_dev_taken(bytes);
        p = nullptr, bytes = 0;
        return q;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// Pinned host words the device writes and the host reads after a wait.
struct PinnedBuf {
    void* p = nullptr;

    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~PinnedBuf() { release(); }

    void release() {
        if (p) prt_pinned_free(p);
        p = nullptr;
    }
    int alloc(size_t n) {
        release();
        const int e = prt_pinned_alloc(&p, n);
        if (e) p = nullptr;
        return e;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// One event; h is the runtime's handle (a hipEvent_t).
struct DevEvent {
    void* h = nullptr;

    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    DevEvent(DevEvent&& o) noexcept : h(o.h) { o.h = nullptr; }
    DevEvent& operator=(DevEvent&& o) noexcept {
        if (this != &o) {
            release();
            h = o.h;
            o.h = nullptr;
        }
        return *this;
    }
    ~DevEvent() { release(); }

    void release() {
        if (h) prt_event_destroy(h);
        h = nullptr;
    }
    int create(bool timing) {
        release();
        const int e = prt_event_create(&h, timing);
        if (e) h = nullptr;
        return e;
    }
};
