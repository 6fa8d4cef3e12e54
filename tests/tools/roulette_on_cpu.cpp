// roulette_on_cpu.cpp — TEST TOOL ONLY (compiled by tests/test_roulette_cpu.py into a temporary directory).
//
// Compiles HRT_FLAG_ROULETTE's rule (hobbyraytracer_amd/csrc/hrt_roulette.h) for the HOST: the statements the kernels
// k_wf_shade_rr / k_wf_shade_st_rr run.  Not part of the product.
#include <cstdint>
#include <cstring>

#include "../../hobbyraytracer_amd/csrc/hrt_roulette.h"

using namespace hrt;

extern "C" {

// the survival probability of an attenuation (1: no roulette)
float roulette_q_c(const float* atten, float q_floor) { return roulette_q(vec3(atten[0], atten[1], atten[2]), q_floor); }

// The decision for every one of the 2^24 values u01 takes (the low 8 bits of the word, which u01 drops, vary too): *survivors = how
// many go on; atten_out = the attenuation the survivors go on with (the input when none survives); returns 1 when every survivor got
// the same bits and every killed path kept its attenuation untouched, else 0.
int roulette_sweep(const float* atten, float q_floor, int64_t* survivors, float* atten_out) {
    const vec3 in(atten[0], atten[1], atten[2]);
    const float q = roulette_q(in, q_floor);
    int64_t n = 0;
    int same = 1;
    float first[3] = {atten[0], atten[1], atten[2]};
    for (uint32_t k = 0; k < (1u << 24); ++k) {
        vec3 a = in;
        const bool killed = roulette_decide(q, (k << 8) | (k * 0x9Du & 0xFFu), a);
        const float now[3] = {a.x, a.y, a.z};
        if (killed) { if (std::memcmp(now, atten, sizeof(now)) != 0) same = 0; continue; }
        if (n++ == 0) std::memcpy(first, now, sizeof(first));
        else if (std::memcmp(first, now, sizeof(first)) != 0) same = 0;
    }
    *survivors = n;
    std::memcpy(atten_out, first, sizeof(first));
    return same;
}

// the whole rule at the vertex of round `round` of (pixel, sample), with its own draw: returns 1 when the path ends; atten in / out
int roulette_rule(uint32_t seed_lo, uint32_t seed_hi, uint32_t pixel, uint32_t sample, int32_t round, int32_t first_bounce, float q_floor,
                  float* atten, int strat) {
    rng_ctx c; c.seed_lo = seed_lo; c.seed_hi = seed_hi; c.pixel = pixel; c.sample = sample; c.bounce = (uint32_t)round;
    vec3 a(atten[0], atten[1], atten[2]);
    const bool killed = strat ? roulette<true>(c, round, first_bounce, q_floor, a) : roulette<false>(c, round, first_bounce, q_floor, a);
    atten[0] = a.x; atten[1] = a.y; atten[2] = a.z;
    return killed ? 1 : 0;
}

// hrt_rng.h's purposes, in the order JITTER, SCATTER, MEDIUM, BALL, BUILD, LENS, LIGHT, ENV, ROULETTE; and the defaults
void roulette_constants(uint32_t* purposes9, int32_t* first_bounce, float* q_floor) {
    const uint32_t p[9] = {RNG_JITTER, RNG_SCATTER, RNG_MEDIUM, RNG_BALL, RNG_BUILD, RNG_LENS, RNG_LIGHT, RNG_ENV, RNG_ROULETTE};
    std::memcpy(purposes9, p, sizeof(p));
    *first_bounce = HRT_ROULETTE_FIRST_BOUNCE; *q_floor = HRT_ROULETTE_Q_FLOOR;
}

}
