// hrt_rng.h — counter-based RNG shared by the HIP kernels, the host plumbing
// and the CPU oracle, plus the restatement of glm's gtc/random distributions.
//
// The reference draws every random number from glm::linearRand /
// sphericalRand / ballRand, i.e. from the unseeded global std::rand()
// (call sites: main.cpp:120-121, material.h:81,118,139,173,218,227,
// constantMedium.cpp:25, bvh.cpp:10).  That
// stream is not reproducible even between two runs of the reference, so
// "seeds pinned" is defined here: Philox4x32-10 (Salmon et al., SC'11) with
//   key     = (seed_lo, seed_hi)
//   counter = (pixel_index, sample_index, bounce, purpose | aux << 8)
// One call yields 4 x u32, enough for any single event of Appendix B.  The key
// contains nothing about tiles, ranks or lanes, so every tiling / GPU count /
// thread schedule produces the identical image.
//
// Documented deviation (Q-11): uniform float = (u32 >> 8) * 2^-24 in [0,1)
// instead of glm's float(u32 built from rand()%255 bytes) / float(UINT32_MAX).
#pragma once
#include "hrt_glm.h"

namespace hrt {

struct u32x4 { uint32_t x, y, z, w; };

enum rng_purpose : uint32_t {
    RNG_JITTER = 0,   // main.cpp:120-121 (bounce field = 0)
    RNG_SCATTER = 1,  // Material::scatter draws of one bounce
    RNG_MEDIUM = 2,   // constantMedium.cpp:25, aux = prim index
    RNG_BALL = 3,     // glm::ballRand rejection loop, aux = attempt
    RNG_BUILD = 4,    // bvh.cpp:10 axis choice (oracle tree build only)
    RNG_LENS = 5,     // camera.h:34 glm::circularRand(lensRadius), HRT_FLAG_THIN_LENS only (bounce field = 0)
    RNG_LIGHT = 6,    // HRT_FLAG_NEE only: one draw per eligible vertex (bounce field = the vertex's bounce, aux = 0):
                      //   x = light choice, y / z = the point on the light, w = the root choice (hrt_device.h nee_*)
                      //   HRT_FLAG_NEE_EMITTERS (hrt_device.h emit_*): aux 0 keeps these words, x = the alias slot
                      //   ((uint64)x n >> 32); aux 1 word x = the alias coin (its y, z, w are unused)
    RNG_ENV = 7,      // HRT_FLAG_NEE_ENV only: per eligible vertex (bounce field = the vertex's bounce) aux = 0: x = row, y = column,
                      //   z = phi in the cell, w = cos theta in the cell; aux = 1: x = the root choice (hrt_device.h env_*)
    RNG_ROULETTE = 8  // HRT_FLAG_ROULETTE only: per vertex that plays (bounce field = the vertex's bounce, aux = 0): x = the survival coin
                      //   (hrt_roulette.h)
};
// Final counter layout: (pixel, sample, bounce, purpose | aux << 8).  The path's own draws (JITTER, LENS, SCATTER, BALL, MEDIUM)
// use bounce = the segment's index; HRT_FLAG_NEE's shadow ray of the vertex at bounce b draws its ConstantMedium free paths
// with bounce = b | HRT_RNG_SHADOW (bit 31), so they never share numbers with a path segment's, and RNG_LIGHT is a purpose
// of its own: every draw of the BSDF path is the one of the default render.
#define HRT_RNG_SHADOW 0x80000000u
// HRT_FLAG_NEE_ENV's environment shadow ray of the same vertex: bounce = b | HRT_RNG_SHADOW | HRT_RNG_SHADOW_ENV (bit 30)
#define HRT_RNG_SHADOW_ENV 0x40000000u

HRT_HD void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    uint32_t n0 = hi1 ^ c1 ^ k0;
    uint32_t n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
}

HRT_HD u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 10; ++i) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    u32x4 r; r.x = c0; r.y = c1; r.z = c2; r.w = c3;
    return r;
}

// Per-path RNG context: which pixel / sample / bounce is being evaluated.
struct rng_ctx {
    uint32_t seed_lo, seed_hi;
    uint32_t pixel, sample, bounce;
};

HRT_HD u32x4 rng_draw(const rng_ctx& c, uint32_t purpose, uint32_t aux) {
    return philox4x32_10(c.pixel, c.sample, c.bounce, purpose | (aux << 8), c.seed_lo, c.seed_hi);
}

// ------------------------------------------------------------------ the stratified sampler (HRT_FLAG_STRATIFIED)
// A draw SITE is one (seed, pixel, bounce, purpose, aux).  With the flag, the samples s = 0, 1, 2, ... of a pixel take, at every site,
// the points of an Owen-scrambled, index-shuffled Sobol' (0,2)-sequence (Burley, "Practical Hash-based Owen Scrambling", JCGT 2020)
// instead of independent Philox words; sites are padded: each has a shuffle and scrambles of its own.
//   seeds   = philox4x32_10 with the counter (pixel, HRT_RNG_SEEDS, bounce, purpose | aux << 8 | HRT_RNG_SEEDS_BIT): the sample field
//             holds a value no sample index takes (they are ints) and bit 31 of the fourth word is one no aux reaches (prim indexes and
//             attempts stay below 2^23), so no draw of the default render makes this call, and it does not depend on `sample`.
//             Net A takes the words x, y, z as (shuffle, scramble 0, scramble 1); net B takes strat_mix of w + 1, 2, 3 times the golden ratio.
//   nus(v, seed) = brev(lk(brev(v), seed)), lk = the Laine-Karras permutation with Burley's constants: every step lets a bit depend on
//             lower bits only, so between two bit reversals it is a nested (Owen) permutation and keeps every elementary interval intact.
//   a net   : j = nus(s, shuffle); coordinate 0 = nus(brev(j), scramble 0) = brev(lk(j, scramble 0)), the van der Corput point;
//             coordinate 1 = nus(sobol2(j), scramble 1) with Sobol's second dimension (v_0 = 1 << 31, v_k = v_{k-1} ^ (v_{k-1} >> 1)).
//             Bit-reversed, that matrix is the substitution z -> 1 + z in the polynomial sum_k j_k z^k over GF(2), which splits in halves
//             ((1 + z)^16 = 1 + z^16): five masked shifts, strat_pascal, give brev(sobol2(j)) from j without a table.
//   words   : a draw returns rng_draw's u32x4.  (A0, A1) = net A, (B0, B1) = net B; a single coordinate of a net is a scrambled
//             (0,1)-sequence, so every word is stratified on its own, and the two words of one 2-D choice are the two coordinates of one net:
//               RNG_JITTER         x, y = A0, A1: the point in the pixel
//               RNG_LENS           x = A0: the angle on the lens' circle
//               RNG_SCATTER        x, y = A0, A1: sphericalRand;  z, w = B0, B1: the dielectric's Fresnel coin u01d(z, w) (z leads)
//               RNG_LIGHT aux 0    y, z = A0, A1: the point on the light;  x = B0: the light / alias slot;  w = B1: the root choice
//               RNG_LIGHT aux 1    x = A0: the alias coin
//               RNG_ENV aux 0      x, y = A0, A1: row, column;  z, w = B0, B1: phi, cos theta in the cell
//               RNG_ENV aux 1      x = A0: the root choice
//               RNG_ROULETTE       x = A0: the survival coin (HRT_FLAG_ROULETTE)
//   not stratified: RNG_MEDIUM (drawn inside the traversal), RNG_BALL (a rejection loop) and RNG_BUILD keep rng_draw.
#define HRT_RNG_SEEDS 0xFFFFFFFFu
#define HRT_RNG_SEEDS_BIT 0x80000000u

HRT_HD uint32_t strat_brev(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v);
#else
    v = (v >> 16) | (v << 16);
    v = ((v & 0xFF00FF00u) >> 8) | ((v & 0x00FF00FFu) << 8);
    v = ((v & 0xF0F0F0F0u) >> 4) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v & 0xCCCCCCCCu) >> 2) | ((v & 0x33333333u) << 2);
    return ((v & 0xAAAAAAAAu) >> 1) | ((v & 0x55555555u) << 1);
#endif
}
// Laine-Karras permutation (on bit-reversed values)
HRT_HD uint32_t strat_lk(uint32_t x, uint32_t seed) {
    x += seed;
    x ^= x * 0x6c50b47cu;
    x ^= x * 0xb82f1e52u;
    x ^= x * 0xc7afe638u;
    x ^= x * 0x8d22f6e6u;
    return x;
}
// brev(sobol2(j)): the coefficients of J(1 + z) for J(z) = sum_k j_k z^k over GF(2)
HRT_HD uint32_t strat_pascal(uint32_t j) {
    j ^= j >> 16;
    j ^= (j & 0xFF00FF00u) >> 8;
    j ^= (j & 0xF0F0F0F0u) >> 4;
    j ^= (j & 0xCCCCCCCCu) >> 2;
    j ^= (j & 0xAAAAAAAAu) >> 1;
    return j;
}
// a full-avalanche integer mix (the seeds of net B from one Philox word)
HRT_HD uint32_t strat_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// point `rs` = brev(sample) of the net seeded by (shuffle, scramble 0, scramble 1)
HRT_HD void strat_net(uint32_t rs, uint32_t sa, uint32_t sb, uint32_t sc, uint32_t& c0, uint32_t& c1) {
    const uint32_t j = strat_brev(strat_lk(rs, sa));
    c0 = strat_brev(strat_lk(j, sb));
    c1 = strat_brev(strat_lk(strat_pascal(j), sc));
}
// the seed words of a draw site (they do not depend on c.sample)
HRT_HD u32x4 strat_seeds(const rng_ctx& c, uint32_t purpose, uint32_t aux) {
    return philox4x32_10(c.pixel, HRT_RNG_SEEDS, c.bounce, purpose | (aux << 8) | HRT_RNG_SEEDS_BIT, c.seed_lo, c.seed_hi);
}
// rng_draw's stratified twin (the word layout per purpose: the table above)
HRT_HD u32x4 strat_draw(const rng_ctx& c, uint32_t purpose, uint32_t aux) {
    const u32x4 k = strat_seeds(c, purpose, aux);
    const uint32_t rs = strat_brev(c.sample);
    uint32_t a0, a1, b0, b1;
    strat_net(rs, k.x, k.y, k.z, a0, a1);
    strat_net(rs, strat_mix(k.w + 0x9E3779B9u), strat_mix(k.w + 0x3C6EF372u), strat_mix(k.w + 0xDAA66D2Bu), b0, b1);
    u32x4 r;
    if (purpose == RNG_LIGHT && aux == 0) { r.x = b0; r.y = a0; r.z = a1; r.w = b1; }
    else { r.x = a0; r.y = a1; r.z = b0; r.w = b1; }
    return r;
}
// the draw of a site by the sampler chosen at compile time: STRAT = false is rng_draw itself
template <bool STRAT>
HRT_HD u32x4 rng_draw_as(const rng_ctx& c, uint32_t purpose, uint32_t aux) {
    if (STRAT) return strat_draw(c, purpose, aux);
    return rng_draw(c, purpose, aux);
}

HRT_HD float u01(uint32_t u) { return (float)(u >> 8) * 5.9604644775390625e-8f; }  // 2^-24
HRT_HD double u01d(uint32_t hi, uint32_t lo) {
    uint64_t v = ((uint64_t)hi << 32) | lo;
    return (double)(v >> 11) * 1.1102230246251565404e-16;  // 2^-53
}
// glm::linearRand(Min, Max) = u * (Max - Min) + Min
HRT_HD float linear_rand(uint32_t u, float mn, float mx) { return u01(u) * (mx - mn) + mn; }

// glm::sphericalRand(1): theta = linearRand(0, 2pi); phi = acos(linearRand(-1, 1));
// (sin(phi) cos(theta), sin(phi) sin(theta), cos(phi))
HRT_HD vec3 spherical_rand(uint32_t u_theta, uint32_t u_z) {
    float theta = linear_rand(u_theta, 0.0f, 6.283185307179586476925286766559f);
    float phi = gacos(linear_rand(u_z, -1.0f, 1.0f));
    float sp, cp, st, ct;
    gsincos(phi, sp, cp);
    gsincos(theta, st, ct);
    float x = sp * ct;
    float y = sp * st;
    float z = cp;
    return vec3(x, y, z);
}

// glm::circularRand(R): a = linearRand(0, 2 pi); (cos a, sin a) * R   -- a point ON the circle (gtc/random.inl)
HRT_HD void circular_rand(uint32_t u_a, float radius, float& x, float& y) {
    float a = linear_rand(u_a, 0.0f, 6.283185307179586476925286766559f);
    float s, c;
    gsincos(a, s, c);
    x = c * radius; y = s * radius;
}

// glm::ballRand(1): rejection on linearRand(vec3(-1), vec3(1)) until length <= 1.
// One Philox call per attempt (purpose RNG_BALL, aux = attempt).  The loop is
// bounded (P[reject] = 1 - pi/6 per attempt; 64 attempts fail with p ~ 1e-21).
HRT_HD vec3 ball_rand(const rng_ctx& c) {
    vec3 r(0.0f);
    for (uint32_t attempt = 0; attempt < 64; ++attempt) {
        u32x4 u = rng_draw(c, RNG_BALL, attempt);
        r = vec3(linear_rand(u.x, -1.0f, 1.0f), linear_rand(u.y, -1.0f, 1.0f), linear_rand(u.z, -1.0f, 1.0f));
        if (!(length(r) > 1.0f)) break;
    }
    return r;
}

}  // namespace hrt
