// hrt_emitters.h — HRT_FLAG_NEE_EMITTERS' emitter table, built on the host in float64.  Host code only (no HIP):
// hrt_hip.hip builds it at hrt_scene_create and in hrt_emitter_table_build, and the CPU tests compile it with g++.
//
// Entries, in prim order (a prim's entries are contiguous; base[prim] = its first, -1 for a prim without entries):
//   XY / XZ / YZ_RECT   one parallelogram            (sub = -1)
//   BOX                 six parallelograms, one per WorldHit::sub side (box_side's order)
//   MESH                one triangle per mesh triangle (sub = the mesh-local triangle index)
//   SPHERE, unwrapped   the sphere of the HRT_FLAG_NEE table (cone / area sampler of hrt_device.h nee_sample)
// of every prim with a DiffuseLight material whose constant emission luminance x strength (a texture factor counts as 1) is positive
// and finite.  Planar entries may sit under any wrapper chain: their corners are mapped to world space by the wrappers' forward maps
// (the maps xf_unapply applies to rec.p, innermost first) in float64.  Left out (they keep weight 1): wrapped spheres (ellipsoids
// under a non-uniform scale) and free TRIANGLE prims -- Triangle::hit as written (hrt_device.h triangle_eval) normalises its vectors, so
// neither the directions it accepts nor its hit point rec.p = o + t d are those of the geometric triangle a light sample would draw.  An entry whose geometry is
// degenerate or not finite keeps its slot with weight 0: it is never drawn and its q is 0.
//
// Record of entry i (HRT_EMIT_REC float4 = 64 B):
//   E0 = prim (bits), kind (bits: HRT_EMIT_PARA / HRT_EMIT_TRI / HRT_PRIM_SPHERE), P_sel, sub (bits)
//   E1 = planar: origin.xyz, world area        sphere: centre.xyz, r
//   E2 = planar: edge1.xyz, 1 if wrapped else 0 sphere: 0, area, 0, 0   (E0..E2 of a sphere are a HRT_NEE_REC record)
//   E3 = planar: edge2.xyz, 0                  sphere: 0
// shade[i] = planar: unit geometric normal.xyz, P_sel / area; sphere: centre.xyz, -r (the shade kernel then reads P_sel from E0).
// Alias table (Vose), one slot per entry: slot = (uint64)x n >> 32 of RNG_LIGHT aux 0 word x; the entry is the slot itself when
// u01(coin) < thresh[slot] (coin = RNG_LIGHT aux 1 word x), else alias[slot].  P_sel is the probability that the stored fp32 table
// realises, recomputed from the stored thresholds and aliases (hrt_emit::realised).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/hrt.h"

#define HRT_EMIT_REC 4
#define HRT_EMIT_PARA 16
#define HRT_EMIT_TRI 17

struct hrt_emitter_table {
    int64_t n = 0;
    std::vector<float> rec;      // 4 * HRT_EMIT_REC floats per entry
    std::vector<float> shade;    // 4 floats per entry
    std::vector<float> thresh;   // per slot
    std::vector<int32_t> alias;  // per slot
    std::vector<int32_t> base;   // per prim
};

namespace hrt_emit {

struct D3 { double x, y, z; };
inline D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 mul(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double norm(D3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
inline bool finite(D3 a) { return std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z); }
inline bool finite_f(D3 a) { return std::isfinite((float)a.x) && std::isfinite((float)a.y) && std::isfinite((float)a.z); }

// One wrapper's forward map of a point: xf_unapply's map of rec.p (translate.cpp:15, scale.cpp:23, rotateQuat.cpp:60 = glm's q * v,
// rotateY.cpp:61-66), in float64
inline D3 xf_forward(const hrt_xform& x, D3 p) {
    const double v0 = x.v[0], v1 = x.v[1], v2 = x.v[2], v3 = x.v[3];
    if (x.kind == HRT_XF_TRANSLATE) return {p.x + v0, p.y + v1, p.z + v2};
    if (x.kind == HRT_XF_SCALE) return {p.x * v0, p.y * v1, p.z * v2};
    if (x.kind == HRT_XF_ROTATE_QUAT) {
        const D3 q = {v0, v1, v2};
        const D3 uv = cross(q, p), uuv = cross(q, uv);
        return add(p, mul(add(mul(uv, v3), uuv), 2.0));
    }
    return {v1 * p.x + v0 * p.z, p.y, -v0 * p.x + v1 * p.z};   // rotate_y: v = sin, cos
}
inline D3 to_world(const hrt_prim& pr, D3 p) {
    for (int k = pr.n_xforms - 1; k >= 0; --k) p = xf_forward(pr.xf[k], p);
    return p;
}
// the rect of axis `axis` (0: x const = YZ, 1: y = XZ, 2: z = XY), p = a0, a1, b0, b1, k: origin and the two edge end points
inline void rect_corners(int axis, const double* p, D3& o, D3& a, D3& b) {
    auto pt = [&](double u, double v) -> D3 {
        if (axis == 0) return {p[4], u, v};
        if (axis == 1) return {u, p[4], v};
        return {u, v, p[4]};
    };
    o = pt(p[0], p[2]); a = pt(p[1], p[2]); b = pt(p[0], p[3]);
}

struct Entry {
    int32_t prim, kind, sub;
    D3 o, e1, e2;           // world space (sphere: o = centre, e1.x = r)
    double area, weight;    // weight 0: never drawn
    bool wrapped;
};

// Appends one planar entry: local origin and edge end points mapped through the prim's wrappers.
inline void planar(std::vector<Entry>& out, const hrt_prim& pr, int32_t prim, int32_t kind, int32_t s, D3 o, D3 a, D3 b, bool ok, double power) {
    Entry e;
    e.prim = prim; e.kind = kind; e.sub = s; e.wrapped = pr.n_xforms > 0;
    e.o = to_world(pr, o);
    e.e1 = sub(to_world(pr, a), e.o);
    e.e2 = sub(to_world(pr, b), e.o);
    const double c = norm(cross(e.e1, e.e2));
    e.area = kind == HRT_EMIT_TRI ? 0.5 * c : c;
    e.weight = e.area * power;
    const bool good = ok && finite(e.o) && finite(e.e1) && finite(e.e2) && finite_f(e.o) && finite_f(e.e1) && finite_f(e.e2) &&
                      e.area > 0.0 && std::isfinite(e.area) && std::isfinite((float)e.area) && (float)e.area > 0.0f &&
                      e.weight > 0.0 && std::isfinite(e.weight);
    if (!good) { e.weight = 0.0; if (!(std::isfinite(e.area) && e.area > 0.0)) e.area = 0.0; }
    out.push_back(e);
}

// Probability of each entry under the fp32 alias table (thresh, alias) of n slots, in float64: slot s is drawn by the words x with
// floor(x n / 2^32) = s, the coin keeps it when u01(coin) = (coin >> 8) 2^-24 < thresh[s]
inline void realised(int64_t n, const float* thresh, const int32_t* alias, std::vector<double>& p) {
    p.assign((size_t)n, 0.0);
    const uint64_t N = (uint64_t)n;
    for (uint64_t s = 0; s < N; ++s) {
        const uint64_t lo = ((s << 32) + N - 1) / N, hi = (((s + 1) << 32) + N - 1) / N;
        const double ps = (double)(hi - lo) * (1.0 / 4294967296.0);
        const double t = (double)thresh[s];
        double k = t <= 0.0 ? 0.0 : std::ceil(t * 16777216.0);
        if (k > 16777216.0) k = 16777216.0;
        const double keep = k * (1.0 / 16777216.0);
        p[s] += ps * keep;
        if (keep < 1.0) p[(size_t)alias[s]] += ps * (1.0 - keep);
    }
}

}  // namespace hrt_emit

// Builds the table of `f` into t (t.n = 0: no emitter table).  Deterministic: one fixed order of float64 operations.
inline int64_t hrt_build_emitter_table(const hrt_flat_scene* f, hrt_emitter_table& t) {
    using namespace hrt_emit;
    t = hrt_emitter_table();
    t.base.assign(f->n_prims, -1);
    std::vector<Entry> ent;
    for (uint32_t i = 0; i < f->n_prims; ++i) {
        const hrt_prim& pr = f->prims[i];
        if (pr.material < 0 || (uint32_t)pr.material >= f->n_materials) continue;
        const hrt_material& m = f->materials[pr.material];
        if (m.kind != HRT_MAT_DIFFUSE_LIGHT) continue;
        const double lum = m.albedo.tex < 0 ? 0.2126 * m.albedo.c[0] + 0.7152 * m.albedo.c[1] + 0.0722 * m.albedo.c[2] : 1.0;
        const double strength = m.s0.tex < 0 ? (double)m.s0.c : 1.0;
        const double power = lum * strength;
        if (!(power > 0.0) || !std::isfinite(power)) continue;
        const size_t first = ent.size();
        double p[9];
        for (int k = 0; k < 9; ++k) p[k] = pr.p[k];
        if (pr.kind == HRT_PRIM_SPHERE) {
            if (pr.n_xforms != 0) continue;   // an ellipsoid under a non-uniform scale: not sampled
            bool ok = true;
            for (int k = 0; k < 4; ++k) ok = ok && std::isfinite(pr.p[k]);
            if (!ok || !(pr.p[3] > 0.0f)) continue;
            Entry e;
            e.prim = (int32_t)i; e.kind = HRT_PRIM_SPHERE; e.sub = -1; e.wrapped = false;
            e.o = {p[0], p[1], p[2]}; e.e1 = {p[3], 0.0, 0.0}; e.e2 = {0.0, 0.0, 0.0};
            e.area = 4.0 * 3.14159265358979323846 * p[3] * p[3];
            e.weight = e.area * power;
            if (!(e.weight > 0.0) || !std::isfinite(e.weight) || !std::isfinite((float)e.area)) continue;
            ent.push_back(e);
        } else if (pr.kind == HRT_PRIM_XY_RECT || pr.kind == HRT_PRIM_XZ_RECT || pr.kind == HRT_PRIM_YZ_RECT) {
            const int axis = pr.kind == HRT_PRIM_YZ_RECT ? 0 : (pr.kind == HRT_PRIM_XZ_RECT ? 1 : 2);
            D3 o, a, b;
            rect_corners(axis, p, o, a, b);
            planar(ent, pr, (int32_t)i, HRT_EMIT_PARA, -1, o, a, b, p[1] > p[0] && p[3] > p[2], power);
        } else if (pr.kind == HRT_PRIM_BOX) {
            for (int s = 0; s < 6; ++s) {   // hrt_device.h box_side
                double rp[5];
                int axis;
                if (s < 2) { axis = 2; rp[0] = p[0]; rp[1] = p[3]; rp[2] = p[1]; rp[3] = p[4]; rp[4] = s == 0 ? p[5] : p[2]; }
                else if (s < 4) { axis = 1; rp[0] = p[0]; rp[1] = p[3]; rp[2] = p[2]; rp[3] = p[5]; rp[4] = s == 2 ? p[4] : p[1]; }
                else { axis = 0; rp[0] = p[1]; rp[1] = p[4]; rp[2] = p[2]; rp[3] = p[5]; rp[4] = s == 4 ? p[3] : p[0]; }
                D3 o, a, b;
                rect_corners(axis, rp, o, a, b);
                planar(ent, pr, (int32_t)i, HRT_EMIT_PARA, s, o, a, b, rp[1] > rp[0] && rp[3] > rp[2], power);
            }
        } else if (pr.kind == HRT_PRIM_MESH) {
            if (pr.mesh < 0 || (uint32_t)pr.mesh >= f->n_meshes) continue;
            const hrt_mesh& mh = f->meshes[pr.mesh];
            if ((uint64_t)mh.tri_first + mh.tri_count > f->n_tris) continue;
            for (uint32_t k = 0; k < mh.tri_count; ++k) {
                const float* v = f->tri_pos + 9ull * ((uint64_t)mh.tri_first + k);
                planar(ent, pr, (int32_t)i, HRT_EMIT_TRI, (int32_t)k, {v[0], v[1], v[2]}, {v[3], v[4], v[5]}, {v[6], v[7], v[8]}, true, power);
            }
        } else continue;
        bool any = false;
        for (size_t k = first; k < ent.size(); ++k) any = any || ent[k].weight > 0.0;
        if (!any) { ent.resize(first); continue; }
        t.base[i] = (int32_t)first;
    }
    double total = 0.0;
    for (const Entry& e : ent) total += e.weight;
    if (ent.empty() || !(total > 0.0) || !std::isfinite(total) || ent.size() >= ((size_t)1 << 30)) {
        t.base.assign(f->n_prims, -1);
        return 0;
    }
    const int64_t n = (int64_t)ent.size();
    // Vose's alias method in float64, in a fixed order (both work lists are stacks filled in entry order)
    std::vector<double> scaled((size_t)n), th((size_t)n, 1.0);
    std::vector<int32_t> al((size_t)n);
    std::vector<int32_t> small, large;
    int32_t any_pos = -1;
    for (int64_t i = 0; i < n; ++i) {
        scaled[(size_t)i] = ent[(size_t)i].weight / total * (double)n;
        al[(size_t)i] = (int32_t)i;
        if (any_pos < 0 && ent[(size_t)i].weight > 0.0) any_pos = (int32_t)i;
        (scaled[(size_t)i] < 1.0 ? small : large).push_back((int32_t)i);
    }
    while (!small.empty() && !large.empty()) {
        const int32_t l = small.back(); small.pop_back();
        const int32_t g = large.back(); large.pop_back();
        th[(size_t)l] = scaled[(size_t)l];
        al[(size_t)l] = g;
        scaled[(size_t)g] = (scaled[(size_t)g] + scaled[(size_t)l]) - 1.0;
        (scaled[(size_t)g] < 1.0 ? small : large).push_back(g);
    }
    for (int32_t g : large) { th[(size_t)g] = 1.0; al[(size_t)g] = g; }
    for (int32_t l : small) { th[(size_t)l] = 1.0; al[(size_t)l] = l; }      // rounding leftovers: keep themselves
    for (int64_t i = 0; i < n; ++i)      // an entry of weight 0 is never drawn: its slot always goes to a drawable entry
        if (!(ent[(size_t)i].weight > 0.0)) {
            th[(size_t)i] = 0.0;
            if (!(ent[(size_t)al[(size_t)i]].weight > 0.0)) al[(size_t)i] = any_pos;
        }
    t.n = n;
    t.thresh.resize((size_t)n);
    t.alias = al;
    for (int64_t i = 0; i < n; ++i) t.thresh[(size_t)i] = (float)th[(size_t)i];
    std::vector<double> pr;
    realised(n, t.thresh.data(), t.alias.data(), pr);
    t.rec.assign((size_t)n * 4 * HRT_EMIT_REC, 0.0f);
    t.shade.assign((size_t)n * 4, 0.0f);
    for (int64_t i = 0; i < n; ++i) {
        const Entry& e = ent[(size_t)i];
        float* r = t.rec.data() + (size_t)i * 4 * HRT_EMIT_REC;
        float* s = t.shade.data() + (size_t)i * 4;
        const float psel = (float)pr[(size_t)i];
        memcpy(&r[0], &e.prim, 4); memcpy(&r[1], &e.kind, 4); r[2] = psel; memcpy(&r[3], &e.sub, 4);
        if (e.kind == HRT_PRIM_SPHERE) {
            r[4] = (float)e.o.x; r[5] = (float)e.o.y; r[6] = (float)e.o.z; r[7] = (float)e.e1.x;
            r[9] = (float)e.area;
            s[0] = r[4]; s[1] = r[5]; s[2] = r[6]; s[3] = -r[7];
            continue;
        }
        const float af = (float)e.area;
        r[4] = (float)e.o.x; r[5] = (float)e.o.y; r[6] = (float)e.o.z; r[7] = af;
        r[8] = (float)e.e1.x; r[9] = (float)e.e1.y; r[10] = (float)e.e1.z; r[11] = e.wrapped ? 1.0f : 0.0f;
        r[12] = (float)e.e2.x; r[13] = (float)e.e2.y; r[14] = (float)e.e2.z;
        if (e.weight > 0.0) {
            const D3 c = cross(e.e1, e.e2);
            const double cn = norm(c);
            s[0] = (float)(c.x / cn); s[1] = (float)(c.y / cn); s[2] = (float)(c.z / cn);
            s[3] = (float)((double)psel / (double)af);
        }
    }
    return n;
}
