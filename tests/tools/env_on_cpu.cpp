// env_on_cpu.cpp — TEST TOOL ONLY (compiled by tests/test_env_nee_cpu.py into a temporary directory).
//
// Compiles the product's environment-map sampling functions (hobbyraytracer_amd/csrc/hrt_device.h env_*) for the HOST, so that the
// CPU-only test run can check the cells, the sampler and the density against numpy float64 tables.  Not part of the product.
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

extern "C" {

// out[4 (j W + i) ..] = phi0, dphi, c0, dc of every cell (fp32, as the sampler uses them; out may be NULL); omega[j W + i] = the fp32
// solid angle
void env_cells(int W, int H, float* out, float* omega) {
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) {
            const size_t k = (size_t)j * W + i;
            if (out) env_cell_bounds<float>(i, j, W, H, out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
            omega[k] = env_cell_solid_angle<float>(i, j, W, H);
        }
}

// the cell background_value reads for each direction d[3 n ..] -> ij[2 n ..] = i, j
void env_cell_of_batch(int W, int H, int64_t count, const float* d, int32_t* ij) {
    for (int64_t n = 0; n < count; ++n) {
        int i, j;
        env_cell_of(vec3(d[3 * n], d[3 * n + 1], d[3 * n + 2]), W, H, i, j);
        ij[2 * n] = i; ij[2 * n + 1] = j;
    }
}

// env_sample with the RNG_ENV draws of (pixel = n, sample 0, bounce 0, seed): ok[n], ij[2 n ..], w[3 n ..], pdf[n]
void env_sample_batch(const float* marg, const float* cond, int W, int H, uint32_t seed, int64_t count, int32_t* ok, int32_t* ij, float* w,
                      float* pdf) {
    for (int64_t n = 0; n < count; ++n) {
        rng_ctx ctx; ctx.seed_lo = seed; ctx.seed_hi = 0; ctx.pixel = (uint32_t)n; ctx.sample = 0; ctx.bounce = 0;
        vec3 d; float p = 0.0f; int i = -1, j = -1;
        ok[n] = env_sample(marg, cond, W, H, rng_draw(ctx, RNG_ENV, 0), d, p, i, j) ? 1 : 0;
        ij[2 * n] = i; ij[2 * n + 1] = j;
        w[3 * n] = d.x; w[3 * n + 1] = d.y; w[3 * n + 2] = d.z;
        pdf[n] = p;
    }
}

// env_pdf of each direction d[3 n ..]
void env_pdf_batch(const float* marg, const float* cond, int W, int H, int64_t count, const float* d, float* out) {
    for (int64_t n = 0; n < count; ++n) out[n] = env_pdf(marg, cond, W, H, vec3(d[3 * n], d[3 * n + 1], d[3 * n + 2]));
}

// the table's float64 weight of every texel (env_texel_weight, as k_env_rows computes it): tex = H x W x channels
void env_weights(const float* tex, int W, int H, int channels, double* out) {
    for (int j = 0; j < H; ++j) {
        double phi0, dphi, c0, dc;
        env_cell_bounds<double>(0, j, W, H, phi0, dphi, c0, dc);
        for (int i = 0; i < W; ++i) out[(size_t)j * W + i] = env_texel_weight(tex + ((size_t)j * W + i) * channels, i, W, dc);
    }
}

float env_mis_bsdf_c(float pb, float q) { return nee_mis_bsdf(pb, q); }
float env_mis_shadow_c(float pb, float q) { return nee_mis_shadow(pb, q); }

}
