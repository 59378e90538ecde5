// The owners of prt_devmem.h over a fake runtime (malloc and counters) under AddressSanitizer + UBSan: every case of
// tests/test_devmem_owner.py's docstring.  A failed check prints UNEXPECTED and the program returns 1; a double free or a
// leak is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>

#include "prt_devmem.h"

namespace {

struct Fake {
    std::map<void*, size_t> dev, pinned, events;  // live blocks and their sizes; dev_bytes: live bytes as the seam counts them
    size_t dev_bytes = 0, allocs = 0, frees = 0, copies = 0, copied_bytes = 0, max_dev_blocks = 0;
    long fail_at = -1;  // the k-th device allocation from now (0 = the next) fails
    int bad = 0;
} F;

int checks = 0;
#define CHECK(x)                                                         \
    do {                                                                 \
        ++checks;                                                        \
        if (!(x)) {                                                      \
            printf("UNEXPECTED line %d: %s\n", __LINE__, #x);            \
            ++F.bad;                                                     \
        }                                                                \
    } while (0)

bool balanced() { return F.dev.empty() && F.dev_bytes == 0 && F.pinned.empty() && F.events.empty(); }

}  // namespace

// ---- the seam over malloc ----
int prt_dev_alloc(void** p, size_t bytes) {
    if (F.fail_at == 0) {
        F.fail_at = -1;
        *p = (void*)(uintptr_t)0xDEAD0;  // (a failed allocation may leave anything behind: the owner must not keep it)
        return 2;
    }
    if (F.fail_at > 0) --F.fail_at;
    *p = malloc(bytes ? bytes : 1);
    F.dev[*p] = bytes;
    F.dev_bytes += bytes;
    ++F.allocs;
    if (F.dev.size() > F.max_dev_blocks) F.max_dev_blocks = F.dev.size();
    return 0;
}
void prt_dev_free(void* p, size_t bytes) {
    auto it = F.dev.find(p);
    if (it == F.dev.end() || it->second != bytes) {
        printf("UNEXPECTED free of %p (%zu bytes): not a live block of that size\n", p, bytes);
        ++F.bad;
        return;
    }
    F.dev_bytes -= bytes;
    F.dev.erase(it);
    ++F.frees;
    free(p);
}
int prt_dev_copy_in(void* dst, const void* src, size_t bytes) {
    memcpy(dst, src, bytes);
    ++F.copies;
    F.copied_bytes += bytes;
    return 0;
}
void prt_dev_adopted(size_t bytes) { F.dev_bytes += bytes; }
void prt_dev_taken(size_t bytes) { F.dev_bytes -= bytes; }
int prt_pinned_alloc(void** p, size_t bytes) {
    *p = malloc(bytes);
    F.pinned[*p] = bytes;
    return 0;
}
void prt_pinned_free(void* p) {
    if (!F.pinned.erase(p)) {
        printf("UNEXPECTED pinned free of %p\n", p);
        ++F.bad;
        return;
    }
    free(p);
}
int prt_event_create(void** ev, bool timing) {
    *ev = malloc(1);
    F.events[*ev] = timing ? 1 : 0;
    return 0;
}
void prt_event_destroy(void* ev) {
    if (!F.events.erase(ev)) {
        printf("UNEXPECTED destroy of event %p\n", ev);
        ++F.bad;
        return;
    }
    free(ev);
}

namespace {

// An array "allocated elsewhere", as bvh_gpu.hip's are: a live block the books do not count until it is adopted
void* foreign(size_t bytes) {
    void* p = malloc(bytes);
    F.dev[p] = bytes;
    return p;
}

struct Five {  // the shape of ensure_path_state: five arrays, allocated in order until one fails
    DevBuf a, b, c, d, e;
    int alloc(size_t n) {
        int rc = a.ensure(n);
        if (!rc) rc = b.ensure(2 * n);
        if (!rc) rc = c.ensure(3 * n);
        if (!rc) rc = d.ensure(4 * n);
        if (!rc) rc = e.ensure(5 * n);
        return rc;
    }
};

void device_cases() {
    {  // a default-constructed owner frees nothing
        DevBuf b;
        CHECK(b.p == nullptr && b.bytes == 0);
    }
    CHECK(F.allocs == 0 && F.frees == 0 && balanced());
    {  // one alloc, one destruction
        DevBuf b;
        CHECK(b.ensure(100) == 0 && b.p && b.bytes == 100);
        CHECK(F.dev.size() == 1 && F.dev_bytes == 100);
        memset(b.p, 1, 100);
    }
    CHECK(F.allocs == 1 && F.frees == 1 && balanced());
    {  // need <= bytes: the pointer stays, no call; growing frees before it allocates
        DevBuf b;
        CHECK(b.ensure(64) == 0);
        void* p0 = b.p;
        const size_t a0 = F.allocs, f0 = F.frees;
        CHECK(b.ensure(64) == 0 && b.ensure(1) == 0 && b.ensure(0) == 0);
        CHECK(b.p == p0 && b.bytes == 64 && F.allocs == a0 && F.frees == f0);
        F.max_dev_blocks = 0;
        CHECK(b.ensure(65) == 0 && b.bytes == 65);
        CHECK(F.allocs == a0 + 1 && F.frees == f0 + 1 && F.max_dev_blocks == 1 && F.dev_bytes == 65);
    }
    CHECK(balanced());
    {  // a failed ensure leaves the owner empty, with nothing to free
        DevBuf b;
        CHECK(b.ensure(32) == 0);
        const size_t f0 = F.frees;
        F.fail_at = 0;
        CHECK(b.ensure(33) != 0);
        CHECK(b.p == nullptr && b.bytes == 0 && F.frees == f0 + 1 && F.dev.empty() && F.dev_bytes == 0);
        CHECK(b.ensure(8) == 0 && b.bytes == 8);  // (and it can be used again)
    }
    CHECK(balanced());
    {  // alloc_copy: the minimum, nothing copied for 0 bytes; the bytes for more; the old block goes first
        DevBuf b;
        const size_t c0 = F.copies;
        CHECK(b.alloc_copy(nullptr, 0) == 0 && b.p && b.bytes == 16 && F.copies == c0);
        const char src[40] = "thirty-nine characters and a terminator";
        F.max_dev_blocks = 0;
        CHECK(b.alloc_copy(src, sizeof(src)) == 0 && b.bytes == 40 && F.copies == c0 + 1 && F.max_dev_blocks == 1);
        CHECK(memcmp(b.p, src, sizeof(src)) == 0);
        CHECK(b.alloc_copy(src, 3) == 0 && b.bytes == 16 && memcmp(b.p, src, 3) == 0);  // (never reuses: upload_* free first)
        CHECK(b.alloc_copy(src, 8, 64) == 0 && b.bytes == 64);
        CHECK(b.as<char>() == (char*)b.p);
        F.fail_at = 0;
        CHECK(b.alloc_copy(src, 8) != 0 && b.p == nullptr && b.bytes == 0);
    }
    CHECK(balanced());
    {  // moves transfer ownership; assignment frees the target's old block exactly once; self-move is harmless
        DevBuf a;
        CHECK(a.ensure(10) == 0);
        void* pa = a.p;
        DevBuf b(std::move(a));
        CHECK(a.p == nullptr && a.bytes == 0 && b.p == pa && b.bytes == 10 && F.dev.size() == 1);
        DevBuf c;
        CHECK(c.ensure(20) == 0);
        const size_t f0 = F.frees;
        c = std::move(b);
        CHECK(F.frees == f0 + 1 && c.p == pa && c.bytes == 10 && b.p == nullptr && F.dev.size() == 1 && F.dev_bytes == 10);
        DevBuf& self = c;
        c = std::move(self);
        CHECK(c.p == pa && c.bytes == 10 && F.frees == f0 + 1);
        c = DevBuf();  // reset by assignment of a fresh value
        CHECK(c.p == nullptr && F.frees == f0 + 2 && F.dev.empty());
    }
    CHECK(balanced());
    {  // adopt then destruction frees once and the books balance; take then destruction frees nothing
        const size_t f0 = F.frees;
        {
            DevBuf b;
            b.adopt(foreign(48), 48);
            CHECK(b.bytes == 48 && F.dev_bytes == 48);
            b.adopt(nullptr, 7);  // (a builder that produced nothing)
            CHECK(b.p == nullptr && b.bytes == 0 && F.frees == f0 + 1 && F.dev_bytes == 0);
            b.adopt(foreign(24), 24);
        }
        CHECK(F.frees == f0 + 2 && balanced());
        void* out;
        {
            DevBuf b;
            CHECK(b.ensure(12) == 0);
            out = b.take();
            CHECK(out && b.p == nullptr && b.bytes == 0 && F.dev_bytes == 0);
            CHECK(b.take() == nullptr);
        }
        CHECK(F.frees == f0 + 2 && F.dev.size() == 1);
        F.dev.erase(out);
        free(out);
    }
    CHECK(balanced());
    for (long k = 0; k < 5; ++k) {  // five owners, the k-th allocation fails (k = 2: the third)
        const size_t a0 = F.allocs, f0 = F.frees;
        {
            Five s;
            F.fail_at = k;
            CHECK(s.alloc(8) != 0);
            CHECK(F.allocs == a0 + (size_t)k && F.dev.size() == (size_t)k);
            CHECK(s.e.p == nullptr && (k > 2 || s.c.p == nullptr));
            s = Five();  // (what ensure_path_state does before it tries again)
            CHECK(F.dev.empty());
            CHECK(s.alloc(8) == 0 && F.dev.size() == 5);
        }
        CHECK(F.frees - f0 == F.allocs - a0 && balanced());
    }
}

void pinned_and_event_cases() {
    { PinnedBuf p; CHECK(p.p == nullptr); }
    CHECK(balanced());
    {
        PinnedBuf p;
        CHECK(p.alloc(64) == 0 && p.p && F.pinned.size() == 1);
        *p.as<uint32_t>() = 7u;
        PinnedBuf q(std::move(p));
        CHECK(p.p == nullptr && *q.as<uint32_t>() == 7u && F.pinned.size() == 1);
        PinnedBuf r;
        CHECK(r.alloc(8) == 0 && F.pinned.size() == 2);
        r = std::move(q);
        CHECK(F.pinned.size() == 1 && *r.as<uint32_t>() == 7u);
        PinnedBuf& self = r;
        r = std::move(self);
        CHECK(r.p && F.pinned.size() == 1);
        CHECK(r.alloc(16) == 0 && F.pinned.size() == 1);  // (a second alloc frees the first)
    }
    CHECK(balanced());
    { DevEvent e; CHECK(e.h == nullptr); }
    CHECK(balanced());
    {
        DevEvent e[4];  // (an array of them, as the context holds per bounce)
        for (DevEvent& x : e) CHECK(x.create(false) == 0 && x.h);
        CHECK(F.events.size() == 4);
        DevEvent a(std::move(e[0]));
        CHECK(e[0].h == nullptr && a.h && F.events.size() == 4);
        e[1] = std::move(a);
        CHECK(a.h == nullptr && F.events.size() == 3);
        DevEvent& self = e[1];
        e[1] = std::move(self);
        CHECK(e[1].h && F.events.size() == 3);
        CHECK(e[1].create(true) == 0 && F.events.size() == 3 && F.events[e[1].h] == 1);
    }
    CHECK(balanced());
}

}  // namespace

int main() {
    device_cases();
    pinned_and_event_cases();
    printf("%d checks, %zu allocations, %zu frees, %d unexpected; no sanitizer report\n", checks, F.allocs, F.frees, F.bad);
    return F.bad ? 1 : 0;
}
