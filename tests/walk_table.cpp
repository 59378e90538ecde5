// Every combination of the walk facts (prt_walk.h) through prt_plan_walk.  The outcome of a combination is the launches of the
// walk (kernel with all template arguments, grid, resolved exit_max / tri_min / stack_cap / steal, perm kept or dropped;
// "overflow": count and rays from the overflow list, not the caller's; "reset": k_reset_cursors precedes it), what the library
// reports for the scene (public name, occupancy instance, resident grid) and the three route predicates.  The output is one line
// per distinct value of each component of the outcome (text_of below), with the number of combinations that have it and an
// order-independent 64-bit hash of their indices (the sum of splitmix64(index) mod 2^64).
// tests/test_walk_table.py compares the output with tests/golden/walk_table.txt, which was recorded from the hand-written
// launchers of the commit before prt_walk.h existed: that commit's launcher text compiled with stub types and
// hipLaunchKernelGGL as a macro that notes kernel, grid and arguments, put in outcome_of's place through
// WALK_TABLE_OUTCOME_FROM over this file's enumeration.  (The recorder is not in the repository.)
// Plain g++, no HIP:  g++ -std=c++17 -O2 -I parallelraytracing_amd/csrc tests/walk_table.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>

#include "prt_walk.h"

// The domain: every value on either side of a threshold of the choice.
static const bool TREES[][3] = {{true, true, true}, {false, true, true}, {true, false, false}};  // has8, has4, has2: see possible()
static const uint32_t DEPTH8[] = {9, 10, 12, 13, 16, 17};     // stack entries + 1 of the lean, wide and deep rows
static const uint32_t STACK4[] = {22, 23, 27, 28, 35, 36};    // the 4-wide rows' LDS stacks
static const uint32_t DEPTH2[] = {25, 31, 32, 33};            // binary pushes (depth - 1) around 24 and 31; k_intersect's stack around 31
static const uint32_t STACK_LDS[] = {0, 1, 2, 3, 4, 5, 6, 24, 39};  // what prt_set_param accepts
static const uint32_t STRIDE[] = {5, 8};
static const uint32_t EXIT_MAX[] = {0xFFFFFFFFu, 8}, TRI_MIN[] = {0, 16}, STACK_CAP[] = {0, 1}, STEAL[] = {0, 4};
static const uint32_t GRID_BLOCKS = 1280;
static const uint32_t MAX_RAYS[] = {256 * GRID_BLOCKS - 256, 256 * GRID_BLOCKS, 256 * GRID_BLOCKS + 1};  // fewer, as many, more blocks
// REQUESTS: closest hit x instrumented x primary offered (0 .. 3), then any-hit, seeded any-hit, path

// index -> facts, mixed radix, the digits in this order from the lowest.  (The facts that fewest choices read come first, so that
// neighbouring indices mostly share an outcome: main() looks an outcome up only when it changes.)
template <class T, size_t N>
static T take(uint64_t& idx, uint64_t& radix, const T (&v)[N]) {
    const T x = v[idx % N];
    idx /= N, radix *= N;
    return x;
}
static const uint32_t TWO[] = {0, 1}, THREE[] = {0, 1, 2}, REQUESTS[] = {0, 1, 2, 3, 4, 5, 6};
static PrtWalkFacts facts_of(uint64_t idx, uint64_t* n_index = nullptr) {
    PrtWalkFacts f{};
    uint64_t radix = 1;
    f.abvh = take(idx, radix, TWO);
    f.depth2 = take(idx, radix, DEPTH2), f.max_stack4 = take(idx, radix, STACK4);
    f.max_rays = take(idx, radix, MAX_RAYS);
    f.steal = take(idx, radix, STEAL), f.stack_cap = take(idx, radix, STACK_CAP);
    f.tri_min = take(idx, radix, TRI_MIN), f.exit_max = take(idx, radix, EXIT_MAX);
    const uint32_t r = take(idx, radix, REQUESTS);
    f.request = r < 4u ? PRT_WALK_CLOSEST : PrtWalkRequest(r - 3u);
    f.stats = r < 4u && (r & 1u);
    f.primary = r < 4u && (r & 2u);
    f.variant = (int)take(idx, radix, THREE);
    f.wide = take(idx, radix, THREE);
    f.node_stride = take(idx, radix, STRIDE);
    f.stack_lds = take(idx, radix, STACK_LDS);
    f.depth8 = take(idx, radix, DEPTH8);
    f.insts = take(idx, radix, TWO);
    const bool* t = TREES[idx % 3];
    radix *= 3;
    f.has8 = t[0], f.has4 = t[1], f.has2 = t[2];
    f.grid_blocks = GRID_BLOCKS;
    if (n_index) *n_index = radix;
    return f;
}
// Combinations no context can produce:
static bool possible(const PrtWalkFacts& f) {
    // the binary and the 4-wide tree are uploaded together (host-built scenes) and dropped together (device build, refit);
    // a scene has at least one tree, so no 4-wide or binary walk without its tree (TREES lists the three cases that remain)
    if (f.has2 != f.has4 || !(f.has8 || f.has4)) return false;
    if (f.insts && !f.has8) return false;  // placed copies: the 8-wide array starts with the top-level tree
    // without a 4-wide tree and without copies: the device builders stop at 15 levels, prt_refit_meshes refuses more than 16
    if (!f.has4 && !f.insts && f.depth8 > 16u) return false;
    // run_batch offers compact primary rays on the compact route only: variant 0 and prt_traverse_takes_primary
    if (f.primary && !(f.variant == 0 && prt_traverse_takes_primary(f))) return false;
    // the any-hit callers (shadow rays, prt_occluded, the last segment) pass no statistics; the last segment needs walk8
    if ((f.request == PRT_WALK_ANY || f.request == PRT_WALK_SEEDED) && f.stats) return false;
    if (f.request == PRT_WALK_SEEDED && !prt_route_walk8(f)) return false;
    // the PATH route: variant 0, the gate (no statistics, prt_path_kernel_applies)
    if (f.request == PRT_WALK_PATH && !(f.variant == 0 && !f.stats && prt_path_kernel_applies(f))) return false;
    return true;
}

// kernels: 0 k_traverse8_persistent, 1 k_occluded8_persistent, 2 k_occluded8_seeded, 3 k_traverse4_persistent,
// 4 k_traverse_persistent, 5 k_intersect
static const char* const KERNEL[] = {"k_traverse8_persistent", "k_occluded8_persistent", "k_occluded8_seeded", "k_traverse4_persistent",
                                     "k_traverse_persistent", "k_intersect"};
static const char KERNEL_ARGS[][8] = {"iibbbbb", "iibb", "iibb", "iiib", "iiib", "ibi"};  // int / bool template arguments
struct Instance {
    uint32_t kernel;
    int32_t arg[7];
};
struct Launch {
    Instance inst;
    uint32_t grid, tuned, exit_max, tri_min, stack_cap, steal, keep_perm, overflow, reset;  // tuned 0: the kernel takes no tunables
};
struct Outcome {  // (uint32_t only: compared and hashed as bytes)
    uint32_t name;  // 0 .. 5: inst12_4waves, wide11_5waves, lean8_5waves, deep15_4waves, bvh4, bvh2
    uint32_t resident_grid, takes_primary, path_applies, walk8, n;
    Instance occupancy;
    Launch launch[2];
};
static const char* const NAME[] = {"inst12_4waves", "wide11_5waves", "lean8_5waves", "deep15_4waves", "bvh4", "bvh2"};
static uint32_t name_code(const char* s) {
    for (uint32_t i = 0; i < 6; ++i)
        if (!strcmp(s, NAME[i])) return i;
    return 6;
}

#ifdef WALK_TABLE_OUTCOME_FROM  // (the golden file's recorder: outcome_of from another source)
#include WALK_TABLE_OUTCOME_FROM
#else
static Instance instance_of(PrtWalkRow row, PrtWalkRequest form, bool stats, bool prim) {
    const PrtWalkRowInfo& ri = prt_walk_row(row);
    const int* a = ri.arg;
    if (ri.family == 8u && (form == PRT_WALK_ANY || form == PRT_WALK_SEEDED)) return Instance{form == PRT_WALK_ANY ? 1u : 2u, {a[0], a[1], a[2], a[3]}};
    if (ri.family == 8u) return Instance{0u, {a[0], a[1], stats, a[2], a[3], prim, form == PRT_WALK_PATH}};
    if (ri.family == 0u) return Instance{5u, {a[0], stats, a[1]}};
    return Instance{ri.family == 4u ? 3u : 4u, {a[0], a[1], a[2], stats}};
}
static Outcome outcome_of(const PrtWalkFacts& f) {
    const PrtWalkPlan p = prt_plan_walk(f);
    Outcome o{};
    o.name = name_code(p.name);
    o.resident_grid = p.resident_grid;
    o.takes_primary = prt_traverse_takes_primary(f), o.path_applies = prt_path_kernel_applies(f), o.walk8 = prt_route_walk8(f);
    o.n = p.n;
    o.occupancy = instance_of(p.occupancy, PRT_WALK_CLOSEST, false, false);
    for (uint32_t i = 0; i < p.n; ++i) {
        const PrtWalkLaunch& l = p.launch[i];
        Launch& t = o.launch[i];
        t.inst = instance_of(l.row, l.form, l.stats, l.prim);
        t.grid = l.grid;
        t.tuned = t.inst.kernel != 5u;
        if (t.tuned) t.exit_max = l.exit_max, t.tri_min = l.tri_min, t.stack_cap = l.stack_cap, t.steal = l.steal, t.keep_perm = l.keep_perm;
        t.overflow = l.overflow, t.reset = l.reset;
    }
    return o;
}
#endif

static std::string text_of(const Instance& k) {
    std::string s = std::string(KERNEL[k.kernel]) + "<";
    for (size_t i = 0; KERNEL_ARGS[k.kernel][i]; ++i)
        s += (i ? ", " : "") + (KERNEL_ARGS[k.kernel][i] == 'b' ? std::string(k.arg[i] ? "true" : "false") : std::to_string(k.arg[i]));
    return s + ">";
}
// The table has one section per COMPONENT of the outcome, each aggregated on its own: the line says which indices have that value
// of the component.  Two sources of outcomes that agree on every section agree on every component of every index, that is on
// every outcome; printing the components jointly would say the same in the product of the sections' line counts (2928 lines).
//   walk: what is launched and what the library reports, without the numbers below
//   grid, exit_max, tri_min, stack_cap, steal: that number of each launch, beside the first launch's kernel and leading arguments
static const char* const SECTION[] = {"walk", "grid", "exit_max", "tri_min", "stack_cap", "steal"};
static std::string text_of(const Outcome& o, uint32_t section) {
    std::string s = SECTION[section];
    if (section == 0u) {
        char buf[256];
        snprintf(buf, sizeof buf, " name=%s occupancy=%s resident=%u takes_primary=%u path_applies=%u walk8=%u |", o.name < 6 ? NAME[o.name] : "?",
                 text_of(o.occupancy).c_str(), o.resident_grid, o.takes_primary, o.path_applies, o.walk8);
        s += buf;
        for (uint32_t i = 0; i < o.n; ++i) {
            const Launch& t = o.launch[i];
            s += (i ? " + " : " ") + text_of(t.inst);
            if (t.tuned) s += t.keep_perm ? " perm=kept" : " perm=dropped";
            if (t.overflow || t.reset) s += std::string(t.overflow ? " overflow" : "") + (t.reset ? " reset" : "");
        }
        return s;
    }
    const Instance& k = o.launch[0].inst;
    s += std::string(" ") + KERNEL[k.kernel] + "<" + std::to_string(k.arg[0]) + (k.kernel == 5u ? "" : ", " + std::to_string(k.arg[1])) + ", ...>";
    for (uint32_t i = 0; i < o.n; ++i) {
        const Launch& t = o.launch[i];
        const uint32_t v[] = {t.grid, t.exit_max, t.tri_min, t.stack_cap, t.steal};
        s += (i ? " + " : " ") + ((section == 1u || t.tuned) ? std::to_string(v[section - 1u]) : std::string("-"));
    }
    return s;
}

static uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
struct Sum {
    uint64_t n = 0, h = 0;
};

int main() {
    std::unordered_map<std::string, Sum> rows;  // key: the outcome's bytes
    std::string last_key;
    Sum* last = nullptr;
    uint64_t n = 0;
    facts_of(0, &n);
    for (uint64_t idx = 0; idx < n; ++idx) {
        const PrtWalkFacts f = facts_of(idx);
        if (!possible(f)) continue;
        const Outcome o = outcome_of(f);
        if (!last || memcmp(last_key.data(), &o, sizeof o)) {
            last_key.assign((const char*)&o, sizeof o);
            last = &rows[last_key];  // (references into an unordered_map survive rehashing)
        }
        ++last->n;
        last->h += splitmix64(idx);
    }
    for (uint32_t section = 0; section < sizeof SECTION / sizeof *SECTION; ++section) {
        std::map<std::string, Sum> lines;
        for (const auto& [k, s] : rows) {
            Outcome o;
            memcpy(&o, k.data(), sizeof o);
            Sum& t = lines[text_of(o, section)];
            t.n += s.n;
            t.h += s.h;
        }
        for (const auto& [l, s] : lines) printf("%s count=%llu hash=%016llx\n", l.c_str(), (unsigned long long)s.n, (unsigned long long)s.h);
    }
    return 0;
}
