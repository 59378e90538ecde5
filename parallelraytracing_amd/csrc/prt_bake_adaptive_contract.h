// prt_bake_adaptive_contract.h — the HIP-free pieces of the bake's statistics and adaptive sampling (include/prt.h "Bake
// statistics and adaptive sampling"): the refusals of the settings in the header's order, the block count and the noise
// formula.  Plain C++: prt_api.cpp and tests/sanitize_bake_adaptive.cpp compile these same lines.  The stopping rule itself
// is prt_adaptive.h's.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#include "../../include/prt.h"
#include "prt_adaptive.h"

// The aligned 8 x 8 blocks of a W x H map.
inline uint32_t prt_bake_block_count(uint32_t W, uint32_t H) { return ((W + 7u) >> 3) * ((H + 7u) >> 3); }

// What is wrong with a threshold / noise_floor pair, or null.
inline const char* prt_bake_rule_refusal(float threshold, float noise_floor) {
    if (!(threshold >= 0.0f) || !(noise_floor >= 0.0f)) return "threshold and noise_floor must be >= 0 (and not NaN)";
    if (threshold == 0.0f && noise_floor == 0.0f) return "threshold and noise_floor are both 0";
    return nullptr;
}

// The first refusal of prt_bake_irradiance_adaptive's settings for a W x H map, in the header's order, or null.
inline const char* prt_bake_adaptive_refusal(const PrtBakeAdaptive* cfg, uint32_t W, uint32_t H) {
    if (!cfg) return "null settings";
    if (cfg->reserved[0] != 0u || cfg->reserved[1] != 0u || cfg->reserved[2] != 0u) return "settings.reserved must be 0";
    if (cfg->min_spp == 0u) return "min_spp = 0: the call keeps no moments from an earlier one";
    if (const char* why = prt_bake_rule_refusal(cfg->threshold, cfg->noise_floor)) return why;
    if (cfg->max_spp < cfg->min_spp) return "max_spp < min_spp";
    if (cfg->step_spp == 0u && cfg->max_spp > cfg->min_spp) return "step_spp is 0 with max_spp > min_spp";
    if (cfg->max_spp > PRT_RADIANCE_MAX_SAMPLES) return "max_spp above PRT_RADIANCE_MAX_SAMPLES";
    if ((uint64_t)W * H * cfg->max_spp > 0xFFFFFFFFull) return "width x height x max_spp exceeds 2^32 - 1 paths";
    return nullptr;
}

// prt_bake_noise.  False: refused.
inline bool prt_bake_noise_rule(uint64_t n, const float* count, const float* sum_y, const float* sum_y2, float noise_floor, float* rel_err) {
    if (!(noise_floor >= 0.0f)) return false;
    if (n != 0u && (!count || !sum_y || !sum_y2 || !rel_err)) return false;
    for (uint64_t t = 0; t < n; ++t) {
        const float cnt = count[t];
        if (cnt == 0.0f) {
            rel_err[t] = 0.0f;
        } else if (!(cnt >= 2.0f)) {
            rel_err[t] = std::numeric_limits<float>::infinity();
        } else {
            const double dn = (double)cnt, m = (double)sum_y[t] / dn;
            const double d = (double)sum_y2[t] / dn - m * m;
            const double V = d > 0.0 ? d : 0.0;
            rel_err[t] = (float)(std::sqrt(V / (dn - 1.0)) / (m + (double)noise_floor));
        }
    }
    return true;
}
