// Every combination of the batch facts (prt_route.h) through prt_plan_route, aggregated to one line per distinct plan: the
// plan, the number of combinations that map to it, and an order-independent 64-bit hash of their indices (the sum of
// splitmix64(index) mod 2^64).  tests/test_route_table.py compares the output with tests/golden/route_table.txt, which was
// recorded from the hand-written launchers and route expressions of the commit before prt_route.h existed.
// With the argument "clusters" it runs a second pass instead: every combination twice, light_clusters false and true, one line
// per distinct (lit && mesh_lights, plan without clusters, plan with clusters) and the number of combinations behind it;
// tests/test_route_table.py states in its own words how the two plans of a line may differ.
// Plain g++, no HIP:  g++ -std=c++17 -O2 -I parallelraytracing_amd/csrc tests/route_table.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>

#include "prt_route.h"

// index -> facts: bit i of the index is fact i of this order; the two values above the bits are path_kernel (0, 1, 2)
static const uint32_t N_BITS = 22u, N_INDEX = 3u << N_BITS;
static PrtRouteFacts facts_of(uint32_t idx) {
    PrtRouteFacts f{};
    uint32_t b = 0;
    auto bit = [&]() { return ((idx >> b++) & 1u) != 0u; };
    f.lit = bit(), f.mesh_lights = bit(), f.env = bit(), f.tex = bit(), f.lens = bit(), f.listed = bit(), f.film_stats = bit();
    f.has_nodes = bit(), f.has_bvh2 = bit(), f.insts = bit(), f.abvh = bit(), f.few_prims = bit();
    f.jitter = bit(), f.sa = bit(), f.multi_sample = bit();
    f.variant0 = bit(), f.compact_primary = bit(), f.primary_walk = bit(), f.takes_primary = bit(), f.primary_hit = bit();
    f.path_gate = bit();
    f.fuse = bit() ? 1u : 0u;
    f.path_kernel = idx >> N_BITS;
    return f;
}
// Combinations no context can produce, by the definitions of the two functions behind the combined facts:
// prt_traverse_takes_primary requires !n_insts, prt_path_kernel_applies requires !n_insts && !abvh_nodes.
static bool possible(const PrtRouteFacts& f) { return !(f.takes_primary && f.insts) && !(f.path_gate && (f.insts || f.abvh)); }

struct Row {
    uint32_t path, compact, walk, fuse, primary_hit, walk8;
    const char *raygen, *shade0, *shade, *accumulate;
    bool operator<(const Row& o) const {
        return std::tie(path, compact, walk, fuse, primary_hit, walk8, raygen, shade0, shade, accumulate) <
               std::tie(o.path, o.compact, o.walk, o.fuse, o.primary_hit, o.walk8, o.raygen, o.shade0, o.shade, o.accumulate);
    }
};

static Row row_of(const PrtRouteFacts& f) {
    const PrtRoutePlan p = prt_plan_route(f);
    return Row{p.path, p.compact, p.walk, p.fuse, p.primary_hit, p.walk8, prt_raygen_name(p.raygen), prt_shade_name(p.shade0),
               prt_shade_name(p.shade), prt_accumulate_name(p.accumulate)};
}

static uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static std::string text_of(const Row& r) {
    char buf[512];
    snprintf(buf, sizeof buf, "path=%u compact=%u walk=%u fuse=%u primary_hit=%u walk8=%u raygen=%s shade0=%s shade=%s accumulate=%s",
             r.path, r.compact, r.walk, r.fuse, r.primary_hit, r.walk8, *r.raygen ? r.raygen : "-", *r.shade0 ? r.shade0 : "-",
             *r.shade ? r.shade : "-", r.accumulate);
    return buf;
}

struct Sum {
    uint64_t n = 0, h = 0;
};

// The second pass: "mesh_lit=<lit && mesh_lights> | <plan, light_clusters false> | <plan, light_clusters true> count=<n>"
static int clusters_pass() {
    std::map<std::tuple<bool, Row, Row>, uint64_t> pairs;
    for (uint32_t idx = 0; idx < N_INDEX; ++idx) {
        PrtRouteFacts f = facts_of(idx);
        if (!possible(f)) continue;
        const Row off = row_of(f);
        f.light_clusters = true;
        ++pairs[{f.lit && f.mesh_lights, off, row_of(f)}];
    }
    std::map<std::string, uint64_t> lines;
    for (const auto& [k, n] : pairs)
        lines[std::string("mesh_lit=") + (std::get<0>(k) ? "1" : "0") + " | " + text_of(std::get<1>(k)) + " | " + text_of(std::get<2>(k))] += n;
    for (const auto& [l, n] : lines) printf("%s count=%llu\n", l.c_str(), (unsigned long long)n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return strcmp(argv[1], "clusters") ? 2 : clusters_pass();
    std::map<Row, Sum> rows;  // (names compare by address here; equal texts are merged below)
    for (uint32_t idx = 0; idx < N_INDEX; ++idx) {
        const PrtRouteFacts f = facts_of(idx);
        if (!possible(f)) continue;
        Sum& s = rows[row_of(f)];
        ++s.n;
        s.h += splitmix64(idx);
    }
    std::map<std::string, Sum> lines;
    for (const auto& [r, s] : rows) {
        Sum& t = lines[text_of(r)];
        t.n += s.n;
        t.h += s.h;
    }
    for (const auto& [l, s] : lines) printf("%s count=%llu hash=%016llx\n", l.c_str(), (unsigned long long)s.n, (unsigned long long)s.h);
    return 0;
}
