// hrt_aov.h -- the per-sample rule of the feature buffers (hrt_render_aov_* in include/hrt.h), used by k_aov / k_aov_st.
//
// The sample's ray is the beauty path's camera ray (path_begin under the same rng_ctx) and `wh` its first hit, found by
// world_hit<false>(sc, o, d, pr.t_min, +inf, ...) under that context: a ConstantMedium's free-path draw is then the beauty path's own.
// Eight floats per sample, as two float4:
//   A = albedo.rgb, alpha     hit: the material's albedo (below), 1          miss: clamp01(background_value(sc, d)), 0
//   B = normal.xyz, depth     hit: rec.normal as hit_record leaves it (0, 0, 0 for a ConstantMedium), rec.t * length(d)      miss: 0, 0, 0, 0
// Albedo of a hit = the material's `albedo` hrt_matvec3 at (rec.u, rec.v, rec.p), i.e. what its scatter multiplies the path by:
//   LAMBERTIAN, METAL, ISOTROPIC, PBR   that value, un-clamped (PBR: whichever lobe its mix would choose, the attenuation is this one)
//   UVTEST                              rec.normal (material.h:116-129: its attenuation)
//   DIELECTRIC                          1, 1, 1
//   DIFFUSE_LIGHT                       clamp01(nee_emitted(sc, rec)): emit x strength, as its `emitted`
// clamp01: each channel to [0, 1], NaN -> 0.  No specular follow-through: a mirror or a glass reports itself.
#pragma once
#include "hrt_device.h"

namespace hrt {

struct AovSample { float4 A, B; };

// fminf(fmaxf(x, 0), 1): fmaxf returns its other operand for a NaN, so NaN -> 0
__device__ inline float aov_clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ inline vec3 aov_clamp01(vec3 c) { return vec3(aov_clamp01(c.x), aov_clamp01(c.y), aov_clamp01(c.z)); }

// sqrtf(d.x*d.x + d.y*d.y + d.z*d.z), the products summed in that order
__device__ inline float aov_length(vec3 d) { return sqrtf(d.x * d.x + d.y * d.y + d.z * d.z); }

__device__ inline vec3 aov_albedo(const DScene& sc, const DRec& rec) {
    int mat_i = rec.mat;
    HRT_BOUNDS(2, mat_i, sc.n_mats);
    const hrt_material& m = sc.lmats[mat_i];
    const int kind = m.kind;
    if (kind == HRT_MAT_DIELECTRIC) return vec3(1.0f, 1.0f, 1.0f);
    if (kind == HRT_MAT_UVTEST) return rec.normal;
    if (kind == HRT_MAT_DIFFUSE_LIGHT) return aov_clamp01(nee_emitted(sc, rec));   // (nee_emitted asks for a valid rec.mat only)
    return matvec3_value(sc, m.albedo, rec.u, rec.v, rec.p);
}

__device__ inline AovSample aov_sample(const DScene& sc, const hrt_params& pr, vec3 o, vec3 d, const WorldHit& wh) {
    AovSample s;
    if (wh.prim < 0) {
        const vec3 bg = aov_clamp01(background_value(sc, d));
        s.A = make_float4(bg.x, bg.y, bg.z, 0.0f);
        s.B = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return s;
    }
    DRec rec;
    hit_record(sc, wh, o, d, pr.quirks, pr.t_min, rec);
    const vec3 a = aov_albedo(sc, rec);
    const bool medium = sc.lprims[wh.prim].kind == HRT_PRIM_MEDIUM;    // constantMedium.cpp:34 gives it an arbitrary (1, 0, 0)
    const vec3 n = medium ? vec3(0.0f) : rec.normal;
    s.A = make_float4(a.x, a.y, a.z, 1.0f);
    s.B = make_float4(n.x, n.y, n.z, rec.t * aov_length(d));
    return s;
}

}  // namespace hrt
