// sampler_on_cpu.cpp — TEST TOOL ONLY (compiled by tests/test_stratified_cpu.py into a temporary directory).
//
// Compiles the samplers of hobbyraytracer_amd/csrc/hrt_rng.h (rng_draw and HRT_FLAG_STRATIFIED's strat_draw) for the
// HOST, keyed the way hrt_sampler_probe keys them on the device.  Not part of the product.
#include <cstdint>

#include "../../hobbyraytracer_amd/csrc/hrt_rng.h"

using namespace hrt;

namespace {
rng_ctx ctx_of(uint32_t seed_lo, uint32_t seed_hi, const uint32_t* key) {
    rng_ctx c; c.seed_lo = seed_lo; c.seed_hi = seed_hi; c.pixel = key[0]; c.sample = key[1]; c.bounce = key[2];
    return c;
}
void put(uint32_t* out, const u32x4& u) { out[0] = u.x; out[1] = u.y; out[2] = u.z; out[3] = u.w; }
}

extern "C" {

// keys[4 i ..] = pixel, sample, bounce, purpose | aux << 8  ->  out[4 i ..] = the draw's words x, y, z, w
// which: 0 = rng_draw, 1 = strat_draw, 2 = strat_seeds
void sampler_draw(uint32_t seed_lo, uint32_t seed_hi, int64_t n, const uint32_t* keys, uint32_t* out, int which) {
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t* k = keys + 4 * i;
        const rng_ctx c = ctx_of(seed_lo, seed_hi, k);
        const uint32_t purpose = k[3] & 0xFFu, aux = k[3] >> 8;
        put(out + 4 * i, which == 0 ? rng_draw_as<false>(c, purpose, aux) : which == 1 ? rng_draw_as<true>(c, purpose, aux) : strat_seeds(c, purpose, aux));
    }
}

// the sampler's parts, for the restatement in numpy
uint32_t strat_brev_c(uint32_t v) { return strat_brev(v); }
uint32_t strat_lk_c(uint32_t v, uint32_t seed) { return strat_lk(v, seed); }
uint32_t strat_pascal_c(uint32_t v) { return strat_pascal(v); }
uint32_t strat_mix_c(uint32_t v) { return strat_mix(v); }

}
