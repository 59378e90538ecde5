// prt_path_id.h — how a batch numbers its paths, in both directions: (local pixel, sample) -> path id (k_raygen, k_accumulate)
// and path id -> (local pixel, sample) (primary_ray: the first k_shade and the bounce-0 walk of compact primary rays).  Plain C++
// with no HIP header: hipcc compiles it for the device, g++ compiles it alone (tests/path_id.cpp holds the decode to id / S and
// id % S).  DESIGN.md section 2 "Path ids" says which batches take which order.
//
//   sample-major (S = 0 below):  id = sample * n_pix_local + pixel.  The ids of one SAMPLE are adjacent: a wave that holds 64
//                                pixels stores its path results (rad[id], 16 B each) coalesced.  Every route but the one below.
//   pixel-major  (S = samples of the batch):  id = pixel * S + sample.  The ids of one PIXEL are adjacent.  For batches whose
//                                ray slots are pixel-major (compact primary rays, at least PRT_PATH_ID_MIN_SAMPLES samples): a
//                                wave of the first k_shade holds 64 samples of one pixel, later launches runs of them.
// Path ids are below 2^32 (run_batch refuses more paths); rad[] and every per-path array are indexed by them.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PRT_PATH_ID_FN __host__ __device__ inline
#else
#define PRT_PATH_ID_FN inline
#endif

// k_raygen stores pixel-major ray slots for a group of at least this many samples (raygen_step); a batch takes pixel-major ids
// from the same count on (a partial last group keeps its sample-major slots and takes the batch's ids)
#define PRT_PATH_ID_MIN_SAMPLES 8u

struct PrtPathIdOrder {
    uint32_t n_pix_local;  // local pixels of the batch (PrtTileMap)
    float inv_n;           // sample-major decode: 1 / n_pix_local, the first guess of id / n_pix_local (corrected exactly)
    uint32_t S;            // 0: sample-major.  Otherwise pixel-major ids of a batch of S samples, 2 <= S <= 2^31, and
    uint32_t magic, shift; // floor(id / S) = (((id - h) >> 1) + h) >> shift with h = high word of id * magic, for EVERY id < 2^32
                           // (Granlund & Montgomery 1994, fig. 4.1: L = ceil(log2 S), magic = floor(2^32 (2^L - S) / S) + 1,
                           // shift = L - 1; a power of two gives magic = 1, h = 0: the plain shift)
};

// The order of a batch of S samples over n_pix_local pixels (host: the magic number needs a 64-bit division).
inline PrtPathIdOrder prt_path_id_order(uint32_t n_pix_local, uint32_t S, bool pixel_major) {
    PrtPathIdOrder o{};
    o.n_pix_local = n_pix_local;
    o.inv_n = n_pix_local ? 1.0f / (float)n_pix_local : 0.0f;
    if (pixel_major && S >= 2u && S <= 0x80000000u) {
        uint32_t L = 1u;
        while (L < 32u && (1ull << L) < S) ++L;
        o.S = S;
        o.magic = (uint32_t)(((1ull << 32) * ((1ull << L) - S)) / S + 1ull);
        o.shift = L - 1u;
    }
    return o;
}

// Which batches number their paths pixel-major: compact primary rays (PrtRoutePlan.compact), enough samples for pixel-major
// slots, and the path_id_order tunable.
inline bool prt_path_id_pixel_major(bool compact, uint32_t S, int path_id_order) {
    return compact && S >= PRT_PATH_ID_MIN_SAMPLES && path_id_order != 0;
}

PRT_PATH_ID_FN uint32_t prt_path_id_encode(const PrtPathIdOrder& o, uint32_t pixel_local, uint32_t sample) {
    return o.S ? pixel_local * o.S + sample : sample * o.n_pix_local + pixel_local;
}

PRT_PATH_ID_FN void prt_path_id_decode(const PrtPathIdOrder& o, uint32_t id, uint32_t& pixel_local, uint32_t& sample) {
    if (o.S) {  // exact integer arithmetic: with S as the divisor a float guess is off by more than one (one ulp of id = 5e8 is 32)
        const uint32_t h = (uint32_t)(((uint64_t)id * o.magic) >> 32);
        const uint32_t q = (((id - h) >> 1) + h) >> o.shift;
        pixel_local = q;
        sample = id - q * o.S;
        return;
    }
    // the divisor is the pixel count: the quotient is a sample index, small enough for the float guess to be within one of it
    uint32_t q = (uint32_t)((float)id * o.inv_n);
    uint32_t r = id - q * o.n_pix_local;
    if ((int32_t)r < 0) {
        --q;
        r += o.n_pix_local;
    }
    if (r >= o.n_pix_local) {
        ++q;
        r -= o.n_pix_local;
    }
    sample = q;
    pixel_local = r;
}
