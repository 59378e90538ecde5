// The key of the persistent primary stage (csrc/prt_primary_cache.h) on its own: prt_primary_reusable is true for equal keys of
// an eligible batch, false as soon as ANY single field differs (on either side), false from or for a cleared key, and false
// whenever the batch at hand is jittered, uses a lens, renders a tile list or is instrumented, even against an equal key.
// The structured bindings below name every field of PrtPrimaryKey and of PrtRoutePlan: a field added to either without a case
// here no longer compiles.  Built with g++ -fsanitize=address,undefined; includes nothing but the header under test.
#include "prt_primary_cache.h"

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond, what)                                             \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("UNEXPECTED: %s (line %d)\n", what, __LINE__); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static PrtPrimaryKey eligible_key() {
    PrtPrimaryKey k{};
    k.valid = true;
    k.camera_gen = 3, k.scene_gen = 7;
    k.W = 1920, k.H = 1080, k.rank = 0, k.world = 1, k.n_pix_local = 1920 * 1080;
    k.S_cur = 256, k.max_depth = 5;
    k.plan.path = false, k.plan.compact = true, k.plan.walk = true, k.plan.primary_hit = true, k.plan.walk8 = true, k.plan.fuse = 0;
    k.plan.raygen = PRT_INST(k_raygen, ffft), k.plan.shade0 = PRT_INST(k_shade, 0ffft), k.plan.shade = PRT_INST(k_shade, 0ffff);
    k.plan.accumulate = PRT_I_k_accumulate, k.plan.last_segment = 2;
    k.walk_row = (uint32_t)PRT_W8_lean8_5waves, k.walk_prim = true;
    k.compact = true, k.walk = true, k.primary_hit = true, k.lens = false, k.jitter = false;
    k.rr_depth = 0, k.clamp = 0.0f;
    k.listed = false, k.instrumented = false, k.exact = true;
    return k;
}

struct Case {
    const char* name;
    std::function<void(PrtPrimaryKey&)> flip;
};

int main() {
    // every field, by name: the counts below are what the cases must add up to
    {
        PrtPrimaryKey k = eligible_key();
        auto& [valid, camera_gen, scene_gen, W, H, rank, world, n_pix_local, S_cur, max_depth, plan, walk_row, walk_prim, compact, walk, primary_hit,
               lens, jitter, rr_depth, clamp, listed, instrumented, exact] = k;
        auto& [path, p_compact, p_walk, p_primary_hit, walk8, fuse, raygen, shade0, shade, accumulate, last_segment] = plan;
        (void)valid, (void)camera_gen, (void)scene_gen, (void)W, (void)H, (void)rank, (void)world, (void)n_pix_local, (void)S_cur, (void)max_depth;
        (void)walk_row, (void)walk_prim, (void)compact, (void)walk, (void)primary_hit, (void)lens, (void)jitter, (void)rr_depth, (void)clamp;
        (void)listed, (void)instrumented, (void)exact;
        (void)path, (void)p_compact, (void)p_walk, (void)p_primary_hit, (void)walk8, (void)fuse, (void)raygen, (void)shade0, (void)shade;
        (void)accumulate, (void)last_segment;
    }
    constexpr size_t kKeyFields = 23, kPlanFields = 11;
    const std::vector<Case> cases = {
        {"camera_gen", [](PrtPrimaryKey& k) { ++k.camera_gen; }},
        {"scene_gen", [](PrtPrimaryKey& k) { ++k.scene_gen; }},
        {"W", [](PrtPrimaryKey& k) { k.W = 1280; }},
        {"H", [](PrtPrimaryKey& k) { k.H = 720; }},
        {"rank", [](PrtPrimaryKey& k) { k.rank = 1; }},
        {"world", [](PrtPrimaryKey& k) { k.world = 3; }},
        {"n_pix_local", [](PrtPrimaryKey& k) { k.n_pix_local -= 64; }},
        {"S_cur", [](PrtPrimaryKey& k) { k.S_cur = 255; }},
        {"max_depth", [](PrtPrimaryKey& k) { k.max_depth = 4; }},
        {"plan.path", [](PrtPrimaryKey& k) { k.plan.path = true; }},
        {"plan.compact", [](PrtPrimaryKey& k) { k.plan.compact = false; }},
        {"plan.walk", [](PrtPrimaryKey& k) { k.plan.walk = false; }},
        {"plan.primary_hit", [](PrtPrimaryKey& k) { k.plan.primary_hit = false; }},
        {"plan.walk8", [](PrtPrimaryKey& k) { k.plan.walk8 = false; }},
        {"plan.fuse", [](PrtPrimaryKey& k) { k.plan.fuse = 1; }},
        {"plan.raygen", [](PrtPrimaryKey& k) { k.plan.raygen = PRT_INST(k_raygen, ffff); }},
        {"plan.shade0", [](PrtPrimaryKey& k) { k.plan.shade0 = PRT_INST(k_shade, 0ffff); }},
        {"plan.shade", [](PrtPrimaryKey& k) { k.plan.shade = PRT_INST(k_shade, 0tfff); }},
        {"plan.accumulate", [](PrtPrimaryKey& k) { k.plan.accumulate = PRT_I_k_accumulate_lit; }},
        {"plan.last_segment", [](PrtPrimaryKey& k) { k.plan.last_segment = 1; }},
        {"walk_row", [](PrtPrimaryKey& k) { k.walk_row = (uint32_t)PRT_W8_deep15_4waves; }},
        {"walk_prim", [](PrtPrimaryKey& k) { k.walk_prim = false; }},
        {"compact", [](PrtPrimaryKey& k) { k.compact = false; }},
        {"walk", [](PrtPrimaryKey& k) { k.walk = false; }},
        {"primary_hit", [](PrtPrimaryKey& k) { k.primary_hit = false; }},
        {"lens", [](PrtPrimaryKey& k) { k.lens = true; }},
        {"jitter", [](PrtPrimaryKey& k) { k.jitter = true; }},
        {"rr_depth", [](PrtPrimaryKey& k) { k.rr_depth = 3; }},
        {"clamp", [](PrtPrimaryKey& k) { k.clamp = 10.0f; }},
        {"listed", [](PrtPrimaryKey& k) { k.listed = true; }},
        {"instrumented", [](PrtPrimaryKey& k) { k.instrumented = true; }},
        {"exact", [](PrtPrimaryKey& k) { k.exact = false; }},
    };
    // (`valid` has its own checks below; `plan` is covered field by field)
    CHECK(cases.size() == (kKeyFields - 2) + kPlanFields, "one case per field of the key and of the plan");

    const PrtPrimaryKey base = eligible_key();
    CHECK(prt_primary_reusable(base, base), "equal keys of an eligible batch are reusable");
    CHECK(prt_primary_reusable(base, eligible_key()), "equal keys built apart are reusable");
    for (const Case& cs : cases) {
        PrtPrimaryKey other = eligible_key();
        cs.flip(other);
        CHECK(!prt_primary_reusable(base, other), cs.name);  // the batch at hand differs
        CHECK(!prt_primary_reusable(other, base), cs.name);  // the held stage differs
    }
    // a cleared key: on either side, on both, and the zero-initialised key a context starts with
    {
        PrtPrimaryKey cleared = eligible_key();
        cleared.valid = false;
        CHECK(!prt_primary_reusable(cleared, base), "a cleared key holds nothing");
        CHECK(!prt_primary_reusable(base, cleared), "a batch that is not eligible has no valid key");
        CHECK(!prt_primary_reusable(cleared, cleared), "two cleared keys");
        CHECK(!prt_primary_reusable(PrtPrimaryKey{}, PrtPrimaryKey{}), "two zero keys");
        CHECK(!prt_primary_reusable(PrtPrimaryKey{}, base), "a zero key holds nothing");
    }
    // never for a jittered, lens, listed or instrumented batch, nor off the compact route, even against the very same key
    for (const char* name : {"jitter", "lens", "listed", "instrumented", "compact"}) {
        PrtPrimaryKey k = eligible_key();
        for (const Case& cs : cases)
            if (std::string(cs.name) == name) cs.flip(k);
        CHECK(!prt_primary_reusable(k, k), name);
    }
    if (failures) {
        std::printf("%d primary-cache checks failed\n", failures);
        return 1;
    }
    std::printf("primary-cache host checks passed (%zu single-field cases)\n", cases.size());
    return 0;
}
