// hrt_roulette.h -- HRT_FLAG_ROULETTE's rule, shared by the kernels k_wf_shade_rr / k_wf_shade_st_rr and the host tests
// (tests/tools/roulette_on_cpu.cpp).
//
// Where: wf_shade_task, directly after the vertex's path_shade* call has returned "not ended" -- the scatter has multiplied the
// attenuation -- and only when round + 1 >= first_bounce (round + 1 = the number of scatters the path has made, this one included).
//   q = min(1, max(atten.x, atten.y, atten.z)), then q = max(q, q_floor)
//   !(q < 1), or an attenuation that is not finite: nothing happens (the NaN / inf convention of the state record stays as it is)
//   u = u01(word x of the RNG_ROULETTE draw of (pixel, sample, bounce = round)); under HRT_FLAG_STRATIFIED word A0 of that site
//   u >= q : the path ends; its slot's radiance is what an ended path's is, it is not compacted, not enqueued, takes no light sample
//   u <  q : atten = atten / q, one IEEE division per component; the path goes on
// u takes the 2^24 values k 2^-24, so a path survives with probability ceil(q 2^24) 2^-24: within 2^-24 of q.
// Everything downstream of the decision -- the vertex's own light sample, which k_wf_shadow weights by the attenuation of the state
// record, and every later vertex -- happens with probability q and carries 1 / q: the estimator stays unbiased.
#pragma once
#include "hrt_rng.h"

namespace hrt {

#define HRT_ROULETTE_FIRST_BOUNCE 3
#define HRT_ROULETTE_Q_FLOOR 0.05f

// the survival probability of a path with this attenuation; 1: no roulette at this vertex
HRT_HD float roulette_q(const vec3& atten, float q_floor) {
    const float s = atten.x + atten.y + atten.z;
    if (!(fabsf(s) < __builtin_huge_valf())) return 1.0f;      // a NaN or inf component (a finite sum that overflows has a component >= 1)
    const float q = fmaxf(fminf(1.0f, fmaxf(atten.x, fmaxf(atten.y, atten.z))), q_floor);
    return q < 1.0f ? q : 1.0f;
}
// the decision for one random word: true = the path ends here; false = it goes on, re-weighted
HRT_HD bool roulette_decide(float q, uint32_t word, vec3& atten) {
    if (!(q < 1.0f)) return false;
    if (u01(word) >= q) return true;
    atten = vec3(atten.x / q, atten.y / q, atten.z / q);
    return false;
}
// the rule at the vertex of round `round` (ctx.bounce == round): draws only where a decision is made
template <bool STRAT>
HRT_HD bool roulette(const rng_ctx& ctx, int round, int first_bounce, float q_floor, vec3& atten) {
    if (round + 1 < first_bounce) return false;
    const float q = roulette_q(atten, q_floor);
    if (!(q < 1.0f)) return false;
    return roulette_decide(q, rng_draw_as<STRAT>(ctx, RNG_ROULETTE, 0).x, atten);
}

}  // namespace hrt
