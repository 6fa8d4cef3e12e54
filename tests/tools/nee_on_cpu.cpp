// nee_on_cpu.cpp — TEST TOOL ONLY (compiled by tests/test_nee_cpu.py into a temporary directory).
//
// Compiles the product's next-event-estimation device functions (hobbyraytracer_amd/csrc/hrt_device.h nee_*) for the HOST, so
// that the CPU-only test run can check the estimator's densities and samplers against numpy: p_b of material_scatter's own
// scatter, the root choice, the light samplers and their densities, the MIS weights.  Not part of the product.
#include <cmath>
#include <cstdlib>
#include <cstring>

#define __device__
struct float4 { float x, y, z, w; };
struct uint4 { unsigned x, y, z, w; };
static inline int __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
static inline float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }

#include "../../hobbyraytracer_amd/csrc/hrt_device.h"

using namespace hrt;

namespace {
float4 f4(const float* p) { float4 r; r.x = p[0]; r.y = p[1]; r.z = p[2]; r.w = p[3]; return r; }
}

extern "C" {

// out[3 * i] = p_b, t0, t1 of direction w[3 i .. 3 i + 2] for the normal n
void nee_bsdf_pdf_batch(const float* n, int64_t count, const float* w, float* out) {
    const vec3 nn(n[0], n[1], n[2]);
    for (int64_t i = 0; i < count; ++i) {
        float t0, t1;
        out[3 * i] = nee_bsdf_pdf(nn, vec3(w[3 * i], w[3 * i + 1], w[3 * i + 2]), t0, t1);
        out[3 * i + 1] = t0; out[3 * i + 2] = t1;
    }
}

// normalize(sd) of material_scatter's Lambertian branch (sd = n + sphericalRand, near_zero -> n) for `count` paths keyed by
// (pixel = i, sample 0, bounce 0) with the product's RNG: the directions whose density nee_bsdf_pdf claims to be
void scatter_dirs(const float* n, uint32_t seed, int64_t count, float* out) {
    const vec3 nn(n[0], n[1], n[2]);
    for (int64_t i = 0; i < count; ++i) {
        rng_ctx ctx; ctx.seed_lo = seed; ctx.seed_hi = 0; ctx.pixel = (uint32_t)i; ctx.sample = 0; ctx.bounce = 0;
        const u32x4 dr = rng_draw(ctx, RNG_SCATTER, 0);
        vec3 sd = nn + spherical_rand(dr.x, dr.y);
        if (near_zero(sd)) sd = nn;
        const vec3 w = normalize(sd);
        out[3 * i] = w.x; out[3 * i + 1] = w.y; out[3 * i + 2] = w.z;
    }
}

float nee_pick_root_c(float t0, float t1, uint32_t u) { return nee_pick_root(t0, t1, u); }
float nee_mis_bsdf_c(float pb, float q) { return nee_mis_bsdf(pb, q); }
float nee_mis_shadow_c(float pb, float q) { return nee_mis_shadow(pb, q); }

// L = 12 floats (one light record).  For each (uy[i], uz[i]): ok[i], w (3), pl, reach -> out[5 i ..]
void nee_sample_batch(const float* L, const float* x, int64_t count, const uint32_t* uy, const uint32_t* uz, int32_t* ok, float* out) {
    const float4 L0 = f4(L), L1 = f4(L + 4), L2 = f4(L + 8);
    const vec3 xx(x[0], x[1], x[2]);
    for (int64_t i = 0; i < count; ++i) {
        vec3 w; float pl = 0.0f, reach = 0.0f;
        ok[i] = nee_sample(L0, L1, L2, xx, uy[i], uz[i], w, pl, reach) ? 1 : 0;
        out[5 * i] = w.x; out[5 * i + 1] = w.y; out[5 * i + 2] = w.z; out[5 * i + 3] = pl; out[5 * i + 4] = reach;
    }
}

// nee_pdf of unit direction w from x, y = where it meets the light
void nee_pdf_batch(const float* L, const float* x, int64_t count, const float* w, const float* y, float* out) {
    const float4 L0 = f4(L), L1 = f4(L + 4), L2 = f4(L + 8);
    const vec3 xx(x[0], x[1], x[2]);
    for (int64_t i = 0; i < count; ++i)
        out[i] = nee_pdf(L0, L1, L2, xx, vec3(w[3 * i], w[3 * i + 1], w[3 * i + 2]), vec3(y[3 * i], y[3 * i + 1], y[3 * i + 2]));
}

int nee_choose_c(const float* table, int n_lights, uint32_t u) { return nee_choose((const float4*)table, n_lights, u); }

}
