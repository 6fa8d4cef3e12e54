// hrt_aov_ids.hip -- k_aov_ids<STRAT>: id mattes and the position buffer of the feature-buffer pass (hrt_render_aov_ids_* in
// include/hrt.h).  A unit of its own so that no kernel of hrt_hip.hip changes by its presence; the entry points, which
// share check_aov and the maps with hrt_render_aov_*, are in hrt_hip.hip and reach the kernel through hrt_aov_ids_launch below.
//
// The sample's ray is k_aov's: path_begin<STRAT> under (seed, pixel, sample, bounce 0), then world_hit<false>(..., pr.t_min, +inf, ...)
// under that context.  Per sample:  object id = wh.prim, material id = rec.mat as hit_record leaves it, position = rec.p;  a miss is
// -1, -1 and 0, 0, 0.  The matte rule -- the two 8-slot tables, their order, the four reported ranks -- is stated in include/hrt.h
// and restated in tests/aov_ids_np.py; the code below follows the header's words.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hrt_device.h"
#include "hrt_map.h"

using namespace hrt;

namespace {

static_assert(HRT_AOV_ID_SLOTS == 8 && HRT_AOV_ID_RANKS == 4, "the table code below is written out for 8 slots and 4 ranks");

// One (id, count) table, HRT_AOV_ID_SLOTS slots in registers: every index below is a compile-time constant after unrolling, so the
// arrays never become private memory.  n == 0 marks an empty slot; slots fill from 0 upwards and are never released, so the used
// slots are always a prefix and "the first slot that is empty or holds the id" is the header's rule.
struct IdTable { int id[HRT_AOV_ID_SLOTS]; int n[HRT_AOV_ID_SLOTS]; };

__device__ inline void ids_clear(IdTable& t) {
#pragma unroll
    for (int k = 0; k < HRT_AOV_ID_SLOTS; ++k) { t.id[k] = INT32_MIN; t.n[k] = 0; }
}
__device__ inline void ids_add(IdTable& t, int id) {
    bool placed = false;      // (a full table without the id: nothing is taken, the sample is dropped)
#pragma unroll
    for (int k = 0; k < HRT_AOV_ID_SLOTS; ++k) {
        const bool take = !placed && (t.n[k] == 0 || t.id[k] == id);
        t.id[k] = take ? id : t.id[k];
        t.n[k] += take ? 1 : 0;
        placed = placed || take;
    }
}
// slot a stays in front of slot b: count descending, then id ascending (signed).  Empty slots (count 0) are equal among themselves.
__device__ inline void ids_cmpswap(IdTable& t, int a, int b) {
    const bool swap = t.n[b] > t.n[a] || (t.n[b] == t.n[a] && t.id[b] < t.id[a]);
    const int ia = t.id[a], na = t.n[a];
    t.id[a] = swap ? t.id[b] : ia; t.n[a] = swap ? t.n[b] : na;
    t.id[b] = swap ? ia : t.id[b]; t.n[b] = swap ? na : t.n[b];
}
// the 19-comparator sorting network for 8 elements (six layers; Knuth, TAOCP 3, 5.3.4)
__device__ inline void ids_sort(IdTable& t) {
    ids_cmpswap(t, 0, 2); ids_cmpswap(t, 1, 3); ids_cmpswap(t, 4, 6); ids_cmpswap(t, 5, 7);
    ids_cmpswap(t, 0, 4); ids_cmpswap(t, 1, 5); ids_cmpswap(t, 2, 6); ids_cmpswap(t, 3, 7);
    ids_cmpswap(t, 0, 1); ids_cmpswap(t, 2, 3); ids_cmpswap(t, 4, 5); ids_cmpswap(t, 6, 7);
    ids_cmpswap(t, 2, 4); ids_cmpswap(t, 3, 5);
    ids_cmpswap(t, 1, 4); ids_cmpswap(t, 3, 6);
    ids_cmpswap(t, 1, 2); ids_cmpswap(t, 3, 4); ids_cmpswap(t, 5, 6);
}
// the first four ranks of a sorted table: ids, and coverage = (float)count / n, one IEEE division each; an unused rank is INT32_MIN, +0
__device__ inline void ids_report(const IdTable& t, float n, uint4& ids, uint4& cov) {
    ids = make_uint4((unsigned)(t.n[0] ? t.id[0] : INT32_MIN), (unsigned)(t.n[1] ? t.id[1] : INT32_MIN),
                     (unsigned)(t.n[2] ? t.id[2] : INT32_MIN), (unsigned)(t.n[3] ? t.id[3] : INT32_MIN));
    cov = make_uint4(__float_as_uint((float)t.n[0] / n), __float_as_uint((float)t.n[1] / n), __float_as_uint((float)t.n[2] / n),
                     __float_as_uint((float)t.n[3] / n));
}

// One thread owns local pixel lp of `map` and walks samples [s0, s0 + n_s) in ascending order, as k_aov does, with k_aov's LDS (the
// per-lane traversal stack and the staged tables) and its launch bound: the 32 registers of the two tables fit beside the traversal's
// under the 168 VGPRs of three waves per SIMD without scratch (DESIGN.md 4.14 has hipcc's figures).  Five 16-byte stores per pixel.
#define HRT_AOV_IDS_WAVES 3
template <bool STRAT>
__global__ __launch_bounds__(HRT_BLOCK, HRT_AOV_IDS_WAVES) void k_aov_ids(DScene sc, hrt_camera cam, hrt_params pr, RenderMap map, unsigned n_local, int s0, int n_s,
                                                                          uint4* __restrict__ out) {
    __shared__ int s_stack[HRT_STACK_DEPTH * HRT_BLOCK];
    __shared__ __attribute__((aligned(16))) uint32_t s_tables[HRT_TABLE_LDS_BYTES / 4];
    int* stack = s_stack + threadIdx.x;
    stage_tables(sc, s_tables);
    const unsigned lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= n_local) return;
    sc.stale_ff = 0;      // as in k_aov: only rec.frontFace depends on it, and nothing written here does
    int px, py;
    slot_pixel(map, lp, px, py);
    IdTable obj, mat;
    ids_clear(obj); ids_clear(mat);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    rng_ctx ctx; ctx.seed_lo = pr.seed_lo; ctx.seed_hi = pr.seed_hi; ctx.pixel = (uint32_t)(py * pr.width + px);
    for (int s = s0; s < s0 + n_s; ++s) {
        ctx.sample = (uint32_t)s; ctx.bounce = 0;
        PathState ps;
        path_begin<STRAT>(cam, pr, px, py, ctx, ps);
        DCounters cnt; cnt.box_tests = 0; cnt.tri_tests = 0;
        const WorldHit wh = world_hit<false>(sc, ps.o, ps.d, pr.t_min, __builtin_huge_valf(), pr.quirks, ctx, stack, cnt);
        int oid = -1, mid = -1;
        vec3 p(0.0f);
        if (wh.prim >= 0) {
            DRec rec;
            hit_record(sc, wh, ps.o, ps.d, pr.quirks, pr.t_min, rec);
            oid = wh.prim; mid = rec.mat; p = rec.p;
        }
        ids_add(obj, oid);
        ids_add(mat, mid);
        sx = sx + p.x; sy = sy + p.y; sz = sz + p.z;
    }
    const float n = (float)n_s;
    ids_sort(obj); ids_sort(mat);
    uint4 oi, oc, mi, mc;
    ids_report(obj, n, oi, oc);
    ids_report(mat, n, mi, mc);
    uint4* o = out + 5ull * lp;
    o[0] = make_uint4(__float_as_uint(sx / n), __float_as_uint(sy / n), __float_as_uint(sz / n), 0u);
    o[1] = oi; o[2] = oc; o[3] = mi; o[4] = mc;
}

}  // namespace

// (for hrt_hip.hip, not part of the ABI)  `map` is that unit's RenderMap -- the same text, hrt_map.h -- and n_local = map_pixels(map)
// > 0 pixels of 80 bytes each follow d_out, which the caller has checked for alignment; the caller has made the device current.
extern "C" __attribute__((visibility("hidden"))) hipError_t hrt_aov_ids_launch(const DScene* ds, const hrt_camera* cam, const hrt_params* pr, const void* map,
                                                                               unsigned n_local, int first, int count, void* d_out, hipStream_t stream) {
    const RenderMap& m = *static_cast<const RenderMap*>(map);
    const unsigned blocks = (n_local + HRT_BLOCK - 1) / HRT_BLOCK;
    if (pr->flags & HRT_FLAG_STRATIFIED)
        hipLaunchKernelGGL(k_aov_ids<true>, dim3(blocks), dim3(HRT_BLOCK), 0, stream, *ds, *cam, *pr, m, n_local, first, count, (uint4*)d_out);
    else
        hipLaunchKernelGGL(k_aov_ids<false>, dim3(blocks), dim3(HRT_BLOCK), 0, stream, *ds, *cam, *pr, m, n_local, first, count, (uint4*)d_out);
    return hipGetLastError();
}
