// prt_scene_pod.h — the two device-visible POD records the host-side scene compiler (prt_scene.cpp) fills: DevPrim and
// DevInstance.  No HIP type in here, so the compiler builds with a plain C++ compiler (and runs under the host
// sanitizers); prt_kernels.h includes this file, the kernels read the same structs.
//
// This file is OUTSIDE the kernel fingerprint (tools/kernel_sha.py hashes prt_kernels.hip, prt_device.h and
// prt_kernels.h only): the static_asserts below pin both layouts instead, so that a change of either cannot go
// unnoticed on the host or on the device side.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct DevPrim {  // 28 dwords; mat/inv keep rows 0..2 of glm's column-major mat4 (cols 0..3)
    uint32_t shape_type;
    float p0, p1;
    uint32_t material;
    float mat[12];  // mat[c*3 + r]
    float inv[12];
};

// One placed mesh copy (PrtInstance) as the kernels see it: 128 B.  mat / inv: rows 0..2 of the column-major mat4
// (like DevPrim).  root: its mesh's root in nodes8; slot_base: first triangle slot of its mesh in tris / tri_normals;
// prim_base: global primitive index of its first triangle (tie-break order); virt_base: first hit id of this copy
// minus n_prims (hit id = n_prims + virt_base + slot - slot_base).
struct DevInstance {
    float mat[12];
    float inv[12];
    uint32_t root, slot_base, prim_base, virt_base;
    uint32_t material, n_tris;
    float inv_scale;  // 1 / uniform scale of mat
    float extent;     // max |coordinate| of the mesh in its own space (culling pad)
};

// float4s per record of the light table (layout: prt_kernels.h, DevLights); prt_scene.cpp fills it, the lighting kernels read it
#define PRT_LIGHT_F4 5u

static_assert(sizeof(DevPrim) == 112 && offsetof(DevPrim, inv) == 64, "DevPrim: 28 dwords, inv last (prt_device.h reads this layout)");
static_assert(sizeof(DevInstance) == 128 && offsetof(DevInstance, extent) == 124, "DevInstance: 128 B, extent last (prt_device.h reads this layout)");
