// The path numbering of a batch (csrc/prt_path_id.h) and the kept primary stage's key for it (csrc/prt_primary_cache.h), on
// their own: decode(encode(pixel, sample)) == (pixel, sample) in both orders; the pixel-major decode (a magic multiply-high)
// equals id / S and id % S on ids 0 .. 2^20, around every multiple of S inside sixteen windows of 2^16 ids spread evenly up to
// 2^32 - 1, and on the last 2^20 ids below n_pix_local * S, for every listed S and pixel count whose product fits 32 bits; two
// stage keys that differ only in the id order, or only in the S the ids were built for, are not reusable for each other.
// Built with g++ -fsanitize=address,undefined; includes nothing but the headers under test.
#include "prt_path_id.h"
#include "prt_primary_cache.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures < 20) {                          \
                std::printf("UNEXPECTED: " __VA_ARGS__);  \
                std::printf(" (line %d)\n", __LINE__);    \
            }                                             \
            ++failures;                                   \
        }                                                 \
    } while (0)

static unsigned long long checked = 0;

static void check_decode(const PrtPathIdOrder& o, uint32_t S, uint32_t id) {
    uint32_t p = 0, s = 0;
    prt_path_id_decode(o, id, p, s);
    CHECK(p == id / S && s == id % S, "S %u id %u: decoded (%u, %u), want (%u, %u)", S, id, p, s, id / S, id % S);
    ++checked;
}

static void check_round_trip(const PrtPathIdOrder& o, uint32_t pixel, uint32_t sample) {
    uint32_t p = 0, s = 0;
    prt_path_id_decode(o, prt_path_id_encode(o, pixel, sample), p, s);
    CHECK(p == pixel && s == sample, "order S %u n %u: (%u, %u) came back as (%u, %u)", o.S, o.n_pix_local, pixel, sample, p, s);
    ++checked;
}

int main() {
    const uint32_t Ss[] = {8, 9, 63, 64, 65, 70, 130, 255, 256, 257, 1000, 4096};
    const uint32_t Ns[] = {1, 37 * 29, 2073600, 8294400};
    unsigned pairs = 0;
    for (const uint32_t S : Ss) {
        const PrtPathIdOrder pm = prt_path_id_order(1u, S, true);
        CHECK(pm.S == S, "S %u: no pixel-major order", S);
        // ids 0 .. 2^20
        for (uint32_t id = 0; id <= (1u << 20); ++id) check_decode(pm, S, id);
        // sixteen windows of 2^16 ids, evenly spaced, the last one ending at 2^32 - 1: every multiple of S in it, and +- 1
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint64_t lo = (uint64_t)w * ((0xFFFFFFFFull - 0xFFFFull) / 15ull), hi = lo + 0xFFFFull;  // w = 15: hi = 2^32 - 1
            if (w == 15u) CHECK(hi == 0xFFFFFFFFull, "the last window ends at %llu", (unsigned long long)hi);
            for (uint64_t m = (lo + S - 1) / S * S; m <= hi; m += S) {
                if (m >= 1) check_decode(pm, S, (uint32_t)(m - 1));
                check_decode(pm, S, (uint32_t)m);
                if (m + 1 <= 0xFFFFFFFFull) check_decode(pm, S, (uint32_t)(m + 1));
            }
            check_decode(pm, S, (uint32_t)lo);
            check_decode(pm, S, (uint32_t)hi);
        }
        for (const uint32_t n : Ns) {
            const uint64_t n_paths = (uint64_t)n * S;
            if (n_paths > (1ull << 32)) continue;
            ++pairs;
            const PrtPathIdOrder o = prt_path_id_order(n, S, true), sm = prt_path_id_order(n, S, false);
            CHECK(o.S == S && o.magic == pm.magic && o.shift == pm.shift && sm.S == 0u, "S %u n %u: the order's fields", S, n);
            // the last 2^20 ids below n * S
            const uint64_t first = n_paths > (1ull << 20) ? n_paths - (1ull << 20) : 0ull;
            for (uint64_t id = first; id < n_paths; ++id) check_decode(o, S, (uint32_t)id);
            // round trips in both orders: the first and last pixels and a stride through the rest, every sample of each
            for (uint32_t k = 0; k < 64u; ++k) {
                const uint32_t pixel = k == 0u ? 0u : k == 1u ? n - 1u : k == 2u ? n / 2u : (uint32_t)(((uint64_t)k * 2654435761ull) % n);
                for (uint32_t s = 0; s < S; ++s) {
                    check_round_trip(o, pixel, s);
                    check_round_trip(sm, pixel, s);
                }
            }
            CHECK(prt_path_id_encode(o, n - 1u, S - 1u) == (uint32_t)(n_paths - 1ull), "S %u n %u: the last pixel-major id", S, n);
            CHECK(prt_path_id_encode(sm, n - 1u, S - 1u) == (uint32_t)(n_paths - 1ull), "S %u n %u: the last sample-major id", S, n);
            CHECK(prt_path_id_encode(o, 1u % n, 0u) == (1u % n) * S && prt_path_id_encode(sm, 0u, 1u) == n, "S %u n %u: the strides", S, n);
        }
    }
    CHECK(pairs == 12u + 12u + 11u + 10u, "pairs with a product of at most 2^32: %u", pairs);  // 1 and 37 x 29: all; 2,073,600: S <= 1000; 8,294,400: S <= 257

    // which batches are pixel-major: the compact route, from 8 samples on, the tunable at 1
    CHECK(prt_path_id_pixel_major(true, 8u, 1) && prt_path_id_pixel_major(true, 256u, 1), "eligible batches");
    CHECK(!prt_path_id_pixel_major(true, 7u, 1) && !prt_path_id_pixel_major(true, 1u, 1), "fewer than 8 samples");
    CHECK(!prt_path_id_pixel_major(false, 256u, 1) && !prt_path_id_pixel_major(true, 256u, 0), "off the compact route, or switched off");

    // the kept primary stage: equal keys are reusable; the order alone, or the S alone, is enough to rebuild
    {
        PrtPrimaryStageKey k{};
        k.batch.valid = true, k.batch.compact = true, k.batch.plan.compact = true;
        k.batch.n_pix_local = 2073600, k.batch.S_cur = 256, k.batch.max_depth = 5;
        k.id_order = 1, k.id_S = 256;
        CHECK(prt_primary_stage_reusable(k, k), "equal stage keys are reusable");
        PrtPrimaryStageKey other_order = k, other_S = k, other_batch = k;
        other_order.id_order = 0;
        other_S.id_S = 255;
        other_batch.batch.S_cur = 255;
        CHECK(!prt_primary_stage_reusable(k, other_order) && !prt_primary_stage_reusable(other_order, k), "keys that differ in the id order");
        CHECK(!prt_primary_stage_reusable(k, other_S) && !prt_primary_stage_reusable(other_S, k), "keys that differ in the ids' S");
        CHECK(!prt_primary_stage_reusable(k, other_batch) && !prt_primary_stage_reusable(other_batch, k), "keys that differ in the batch size");
        PrtPrimaryStageKey cleared = k;
        cleared.batch.valid = false;
        CHECK(!prt_primary_stage_reusable(cleared, k) && !prt_primary_stage_reusable(k, cleared), "a cleared stage key");
    }
    if (failures) {
        std::printf("%d path-id checks failed\n", failures);
        return 1;
    }
    std::printf("path-id host checks passed (%llu ids, %u pairs)\n", checked, pairs);
    return 0;
}
