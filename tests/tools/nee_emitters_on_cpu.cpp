// nee_emitters_on_cpu.cpp — TEST TOOL ONLY (compiled by tests/test_nee_emitters_cpu.py into a temporary directory).
//
// Compiles the emitter table builder (hobbyraytracer_amd/csrc/hrt_emitters.h) and the emitter sampling device functions
// (hrt_device.h emit_*) for the HOST, so that the CPU-only test run can check the table, the alias choice, the samplers and their
// densities against numpy.  Not part of the product.
#include <cmath>
#include <cstdlib>
#include <cstring>

#define __device__
struct float4 { float x, y, z, w; };
struct uint4 { unsigned x, y, z, w; };
struct float2 { float x, y; };
static inline int __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
static inline float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }

#include "../../hobbyraytracer_amd/csrc/hrt_device.h"

using namespace hrt;

namespace {
float4 f4(const float* p) { float4 r; r.x = p[0]; r.y = p[1]; r.z = p[2]; r.w = p[3]; return r; }
}

extern "C" {

// the table of `f`: size query with rec == NULL, else every output filled (sizes as hrt_emitter_table_build's)
int64_t emit_build(const hrt_flat_scene* f, float* rec, float* shade, float* thresh, int32_t* alias, int32_t* base) {
    hrt_emitter_table t;
    const int64_t n = hrt_build_emitter_table(f, t);
    if (rec) {
        std::memcpy(rec, t.rec.data(), t.rec.size() * sizeof(float));
        std::memcpy(shade, t.shade.data(), t.shade.size() * sizeof(float));
        std::memcpy(thresh, t.thresh.data(), t.thresh.size() * sizeof(float));
        std::memcpy(alias, t.alias.data(), t.alias.size() * sizeof(int32_t));
        std::memcpy(base, t.base.data(), t.base.size() * sizeof(int32_t));
    }
    return n;
}

// emit_choose for count (ux, coin) pairs; tab = n (thresh, alias bits) pairs
void emit_choose_batch(const float* tab, int n, int64_t count, const uint32_t* ux, const uint32_t* coin, int32_t* out) {
    const float2* t = (const float2*)tab;
    for (int64_t i = 0; i < count; ++i) out[i] = emit_choose(t, n, ux[i], coin[i]);
}

// one record (16 floats): for each (uy[i], uz[i]) ok[i], w (3), pl, reach -> out[5 i ..] (planar and sphere entries)
void emit_sample_batch(const float* rec, const float* x, int64_t count, const uint32_t* uy, const uint32_t* uz, int32_t* ok, float* out) {
    const float4 E0 = f4(rec), E1 = f4(rec + 4), E2 = f4(rec + 8), E3 = f4(rec + 12);
    const vec3 xx(x[0], x[1], x[2]);
    const int kind = __float_as_int(E0.y);
    for (int64_t i = 0; i < count; ++i) {
        vec3 w; float pl = 0.0f, reach = 0.0f;
        const bool r = kind == HRT_PRIM_SPHERE ? nee_sample(E0, E1, E2, xx, uy[i], uz[i], w, pl, reach)
                                               : emit_sample_planar(kind == HRT_EMIT_TRI, E1, E2, E3, xx, uy[i], uz[i], w, pl, reach);
        ok[i] = r ? 1 : 0;
        out[5 * i] = w.x; out[5 * i + 1] = w.y; out[5 * i + 2] = w.z; out[5 * i + 3] = pl; out[5 * i + 4] = reach;
    }
}

// q = P_sel p_l of unit direction w from x meeting the planar entry of shade record S at y
void emit_q_batch(const float* S, const float* x, int64_t count, const float* w, const float* y, float* out) {
    const float4 s = f4(S);
    const vec3 xx(x[0], x[1], x[2]);
    for (int64_t i = 0; i < count; ++i)
        out[i] = emit_q_planar(s, xx, vec3(w[3 * i], w[3 * i + 1], w[3 * i + 2]), vec3(y[3 * i], y[3 * i + 1], y[3 * i + 2]));
}

}
