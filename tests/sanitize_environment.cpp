// sanitize_environment.cpp — the host half of the environment light under AddressSanitizer + UBSan on the CPU: the table
// builder (prt_scene.cpp prt_build_environment) and the PFM reader (prt_host.cpp prt_read_pfm).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I parallelraytracing_amd/csrc \
//       tests/sanitize_environment.cpp parallelraytracing_amd/csrc/prt_host.cpp parallelraytracing_amd/csrc/bvh.cpp \
//       parallelraytracing_amd/csrc/prt_scene.cpp -pthread -o /tmp/sanitize_environment
//   /tmp/sanitize_environment <scratch directory> [n_mutations]
// Tables: maps from 1 x 1 to 257 x 129 (constant, seeded log-normal, black rows and row ends, one huge texel, denormals,
// FLT_MAX, all black); the widths must add up to 2^32 per table and the search tables must return, for thresholds either
// side of every boundary, the interval that holds the draw.  Every invalid description must be refused with
// PRT_ERR_INVALID and leave the output untouched.  Reader: a valid file in both byte orders reads back bit for bit; then
// n seeded mutations of header and body (bytes flipped, inserted, removed, the file cut short, sizes inflated) must each
// end in PRT_OK or PRT_ERR_IO, never in a report.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "prt.h"
#include "prt_scene.h"

static int n_fail = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        printf("  ^^^ UNEXPECTED: %s\n", what);
        ++n_fail;
    }
}

// the interval the device-side search returns for draw r: smallest i in [0, last] with r < thr[i], else last
static uint32_t search(const uint32_t* thr, uint32_t last, uint32_t r) {
    uint32_t lo = 0, hi = last;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r < thr[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}

static void check_search(const uint64_t* width, const uint32_t* thr, uint32_t n, uint32_t last, const char* what) {
    uint64_t T = 0, sum = 0;
    for (uint32_t i = 0; i < n; ++i) sum += width[i];
    expect(sum == 4294967296ull, what);
    for (uint32_t i = 0; i < n; ++i) {
        if (width[i]) {
            expect(search(thr, last, (uint32_t)T) == i, what);                      // first draw of the interval
            expect(search(thr, last, (uint32_t)(T + width[i] - 1)) == i, what);     // its last
        }
        T += width[i];
    }
}

static void check_tables(const std::vector<float>& rgb, uint32_t W, uint32_t H, bool black, const char* what) {
    PrtEnvironment e{rgb.data(), W, H, 0.5f};
    PrtEnvTables t;
    std::string err;
    const int rc = prt_build_environment(&e, &t, &err);
    expect(rc == PRT_OK, what);
    if (rc) return;
    expect(t.W == W && t.H == H && t.texels.size() == 4 * (size_t)W * H, what);
    expect(t.row_width.empty() == black, what);
    expect(prt_environment_threshold(t, 3) == (black ? 0u : 2147483648ull), what);
    expect(prt_environment_threshold(t, 0) == (black ? 0u : 4294967296ull), what);
    if (black) return;
    check_search(t.row_width.data(), t.row_thr.data(), H, t.row_last, what);
    uint32_t n_sampled = 0;
    for (uint32_t i = 0; i < H; ++i) {
        if (!t.row_width[i]) continue;
        check_search(&t.col_width[(size_t)i * W], &t.col_thr[(size_t)i * W], W, t.col_last[i], what);
        for (uint32_t j = 0; j < W; ++j) {
            const bool sampled = t.col_width[(size_t)i * W + j] != 0;
            n_sampled += sampled;
            expect((t.texels[4 * ((size_t)i * W + j) + 3] > 0.0f) == sampled, "pdf entry positive exactly where the interval is not empty");
        }
    }
    expect(n_sampled == t.n_sampled, what);
}

static void refuse(const PrtEnvironment& e, const char* what) {
    PrtEnvTables t;
    t.W = 77;  // must stay
    std::string err;
    expect(prt_build_environment(&e, &t, &err) == PRT_ERR_INVALID && t.W == 77 && !err.empty(), what);
}

static std::vector<unsigned char> slurp(const std::string& p) {
    std::vector<unsigned char> b;
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return b;
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

static void spit(const std::string& p, const std::vector<unsigned char>& b) {
    FILE* f = fopen(p.c_str(), "wb");
    if (!f) return;
    if (!b.empty()) fwrite(b.data(), 1, b.size(), f);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const int n_mut = argc > 2 ? atoi(argv[2]) : 300;
    std::mt19937 rng(2024);
    std::lognormal_distribution<float> ln(0.0f, 1.5f);

    // ---- tables ----
    const uint32_t sizes[][2] = {{1, 1}, {5, 3}, {16, 8}, {64, 32}, {257, 129}, {1, 7}, {9, 1}};
    for (const auto& sz : sizes) {
        const uint32_t W = sz[0], H = sz[1];
        std::vector<float> a(3 * (size_t)W * H);
        for (float& v : a) v = 0.25f;
        check_tables(a, W, H, false, "constant map");
        for (float& v : a) v = ln(rng);
        check_tables(a, W, H, false, "log-normal map");
        std::vector<float> b = a;
        for (uint32_t j = 0; j < 3 * W; ++j) b[j] = b[3 * (size_t)W * (H - 1) + j] = 0.0f;   // first and last row black
        if (H > 2) {
            for (int ch = 0; ch < 3; ++ch) b[3 * (size_t)W * 1 + ch] = b[3 * ((size_t)W * 2 - 1) + ch] = 0.0f;  // both ends of row 1
            check_tables(b, W, H, false, "black rows and row ends");
        }
        b = a;
        b[3 * ((size_t)W * (H / 2) + W / 2)] = 1.0e30f;   // every other interval may round to nothing
        check_tables(b, W, H, false, "one huge texel");
        b[0] = FLT_MAX;
        b[1] = FLT_MAX;
        b[2] = FLT_MAX;
        check_tables(b, W, H, false, "FLT_MAX texel");
        for (float& v : b) v = 1.0e-44f;
        check_tables(b, W, H, false, "denormal map");
        for (float& v : b) v = 0.0f;
        check_tables(b, W, H, true, "all-black map");
    }
    {
        std::vector<float> a(3 * 4 * 2, 1.0f);
        refuse(PrtEnvironment{nullptr, 4, 2, 0.5f}, "null image");
        refuse(PrtEnvironment{a.data(), 0, 2, 0.5f}, "width 0");
        refuse(PrtEnvironment{a.data(), 4, 0, 0.5f}, "height 0");
        refuse(PrtEnvironment{a.data(), PRT_ENV_MAX_WIDTH + 1, 1, 0.5f}, "too wide");
        refuse(PrtEnvironment{a.data(), 1, PRT_ENV_MAX_HEIGHT + 1, 0.5f}, "too high");
        refuse(PrtEnvironment{a.data(), 4, 2, -0.1f}, "negative share");
        refuse(PrtEnvironment{a.data(), 4, 2, 1.5f}, "share above 1");
        refuse(PrtEnvironment{a.data(), 4, 2, NAN}, "NaN share");
        std::vector<float> b = a;
        b[5] = -1.0e-30f;
        refuse(PrtEnvironment{b.data(), 4, 2, 0.5f}, "negative texel");
        b[5] = INFINITY;
        refuse(PrtEnvironment{b.data(), 4, 2, 0.5f}, "infinite texel");
        b[5] = NAN;
        refuse(PrtEnvironment{b.data(), 4, 2, 0.5f}, "NaN texel");
    }
    printf("tables done\n");

    // ---- PFM reader ----
    const uint32_t W = 7, H = 5;
    std::vector<float> img(3 * W * H);
    for (float& v : img) v = ln(rng);
    const std::string good = dir + "/good.pfm", mut = dir + "/mut.pfm";
    expect(prt_write_pfm(good.c_str(), img.data(), W, H) == PRT_OK, "write");
    float* back = nullptr;
    uint32_t w = 0, h = 0;
    expect(prt_read_pfm(good.c_str(), &back, &w, &h) == PRT_OK && w == W && h == H && back &&
               memcmp(back, img.data(), img.size() * sizeof(float)) == 0,
           "round trip, little-endian");
    prt_image_free(back);
    const std::vector<unsigned char> file = slurp(good);
    size_t header = 0;
    for (int nl = 0; header < file.size() && nl < 3; ++header) nl += file[header] == '\n';
    {   // the same image big-endian: "1.0" and every float's bytes reversed
        std::vector<unsigned char> be(file.begin(), file.begin() + (long)header);
        const std::string hd(be.begin(), be.end());
        const size_t at = hd.find("-1.0");
        expect(at != std::string::npos, "the writer's scale");
        be.erase(be.begin() + (long)at);
        for (size_t k = header; k + 3 < file.size(); k += 4)
            for (int q = 3; q >= 0; --q) be.push_back(file[k + (size_t)q]);
        spit(mut, be);
        back = nullptr;
        expect(prt_read_pfm(mut.c_str(), &back, &w, &h) == PRT_OK && w == W && h == H && back &&
                   memcmp(back, img.data(), img.size() * sizeof(float)) == 0,
               "round trip, big-endian");
        prt_image_free(back);
    }
    expect(prt_read_pfm((dir + "/missing.pfm").c_str(), &back, &w, &h) == PRT_ERR_IO, "missing file");
    int n_ok = 0, n_io = 0;
    const char* headers[] = {"Pf\n7 5\n-1.0\n", "PF\n7 5\n0\n", "PF\n7 5\nnan\n", "PF\n-7 5\n-1.0\n", "PF\n7 5 -1.0", "PF\n99999 99999\n-1.0\n",
                             "PF\n4294967297 1\n-1.0\n", "PF 268435456 1 -1\n", "PF\n7\n", "", "PF", "PF\n7 5\n-1.0e999999\n",
                             "PF\n00000000000000000000007 5\n-1.0\n", "P6\n7 5\n255\n"};
    for (int k = 0; k < n_mut + (int)(sizeof(headers) / sizeof(headers[0])); ++k) {
        std::vector<unsigned char> b = file;
        if (k >= n_mut) {  // a hand-written header in front of the valid body
            const char* hd = headers[k - n_mut];
            b.assign(file.begin() + (long)header, file.end());
            b.insert(b.begin(), hd, hd + strlen(hd));
        } else {
            const int edits = 1 + (int)(rng() % 4);
            for (int e = 0; e < edits && !b.empty(); ++e) {
                const bool in_header = rng() % 3 != 0;
                const size_t at = in_header ? rng() % std::min(b.size(), header + 2) : rng() % b.size();
                switch (rng() % 5) {
                    case 0: b[at] = (unsigned char)rng(); break;
                    case 1: b.insert(b.begin() + (long)at, (unsigned char)("0123456789 \n-.eE+PF"[rng() % 19])); break;
                    case 2: b.erase(b.begin() + (long)at); break;
                    case 3: b.resize(at); break;
                    default: b.insert(b.begin() + (long)at, 9, (unsigned char)('0' + rng() % 10)); break;
                }
            }
        }
        spit(mut, b);
        back = nullptr;
        const int rc = prt_read_pfm(mut.c_str(), &back, &w, &h);
        expect(rc == PRT_OK || rc == PRT_ERR_IO, "a mutated file is read or refused as PRT_ERR_IO");
        if (rc == PRT_OK) {
            expect(back && w > 0 && h > 0, "a read image has a size");
            volatile float sink = 0.0f;
            for (size_t q = 0; q < 3 * (size_t)w * h; ++q) sink = sink + (back[q] == back[q] ? 0.0f : 1.0f);   // touch every float
            prt_image_free(back);
            ++n_ok;
        } else {
            expect(back == nullptr && w == 0 && h == 0, "a refused file leaves no image");
            ++n_io;
        }
    }
    remove(mut.c_str());
    remove(good.c_str());
    printf("pfm: %d mutations read, %d refused\n", n_ok, n_io);
    if (n_fail) {
        printf("%d UNEXPECTED\n", n_fail);
        return 1;
    }
    printf("no sanitizer report\n");
    return 0;
}
