// hrt_wf_kernels.h -- the three kernels of the wavefront pipeline that draw random numbers outside the traversal: k_wf_gen (jitter, lens),
// k_wf_shade (the scatter) and k_wf_shadow (the light and environment samples).  NOT a header in the usual sense: hrt_hip.hip includes
// it TWICE, once per sampler, with
//   HRT_K(name) = name,      HRT_STRAT = false : the default kernels (Philox words per sample, hrt_rng.h rng_draw), and
//   HRT_K(name) = name##_st, HRT_STRAT = true  : the kernels of HRT_FLAG_STRATIFIED (hrt_rng.h strat_draw).
// The stratified kernels have names of their own because tests/test_*_resources.py find the default ones by their mangled names; and
// the text is shared by inclusion, not through a __device__ body both kernels call, because that body, although always inlined, changed
// the default kernels' code (kernel arguments reached through references: 1 % more instructions in k_wf_shade<false, false>, +0.2 ms on
// the headline frame).  This way the default kernels are compiled from the statements they always were.
// HRT_FLAG_ROULETTE includes it twice more, with HRT_RR defined, for k_wf_shade alone:
//   HRT_K(name) = name##_rr,    HRT_STRAT = false : k_wf_shade_rr, and
//   HRT_K(name) = name##_st_rr, HRT_STRAT = true  : k_wf_shade_st_rr,
// which take the rule's two parameters as kernel arguments of their own (hrt_params does not grow) and hand them to wf_shade_task<...,
// RR = true>.  k_wf_gen and k_wf_shadow play no roulette and are not compiled again.
#if !defined(HRT_K) || !defined(HRT_STRAT)
#error "include from hrt_hip.hip with HRT_K and HRT_STRAT defined"
#endif
#ifdef HRT_RR
#define HRT_RR_ON true
#define HRT_RR_PARAMS , int rr_first, float rr_floor
#define HRT_RR_ARGS , rr_first, rr_floor
#else
#define HRT_RR_ON false
#define HRT_RR_PARAMS
#define HRT_RR_ARGS
#endif

#ifndef HRT_RR
// Camera rays (main.cpp:115-123) of every slot of the batch + the preparation of their first segment.
template <bool STATS>
__global__ __launch_bounds__(256) void HRT_K(k_wf_gen)(DScene sc, hrt_camera cam, hrt_params pr, RenderMap map, WfScene ws, unsigned n_local, int s0,
                                                       unsigned n_slots, WfBuf w, DeviceCounters* counters) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned n_culled = 0;
    HRT_FOR_MY_TASKS(task, w, wave, lane) {
        const unsigned base = task * w.T;
        const unsigned n = base < n_slots ? min(w.T, n_slots - base) : 0u;
        unsigned qpos = base, rcount = 0;
        for (unsigned j0 = 0; j0 < n; j0 += 64) {
            const unsigned j = j0 + lane;
            int enq = HRT_ENQ_NONE;
            MeshRay mr;
            float closest = __builtin_huge_valf();
            const unsigned slot = base + j;
            if (j < n) {
                int px, py;
                const unsigned sl = fastdiv(slot, n_local, map.m_nl);
                slot_pixel(map, slot - sl * n_local, px, py);
                rng_ctx ctx; ctx.seed_lo = pr.seed_lo; ctx.seed_hi = pr.seed_hi;
                ctx.pixel = (uint32_t)(py * pr.width + px); ctx.sample = (uint32_t)(s0 + (int)sl); ctx.bounce = 0;
                PathState ps;
                path_begin<HRT_STRAT>(cam, pr, px, py, ctx, ps);
                int prim = -1, sub = -1;
                enq = wf_prepare<STATS>(sc, pr, 0, ws.first_mesh, ws.has_mesh ? ws.first_mesh : -1, ps.o, ps.d, ctx, closest, prim, sub, mr, n_culled);
                wf_store_state(w, 0, slot, ps, closest, slot, prim, sub);
            }
            wf_enqueue(w, enq, mr, closest, slot, lt, qpos, base + w.T - 1, rcount);
        }
        if (lane == 0) { w.live[task] = n; w.qn[task] = qpos - base; w.rn[task] = rcount; if (rcount) wf_ref_publish(w, task, rcount); }
    }
    if (STATS) {
        const unsigned c = wave_sum(n_culled);
        if (lane == 0 && c) atomicAdd(&counters->box_tests, 2ull * c);   // the root's two boxes were tested
    }
}
#endif   // !HRT_RR

// One round's shading of every task (wf_shade_task).
// ENV (HRT_FLAG_NEE_ENV, with NEE only): the environment map's MIS weight on escapes from eligible vertices
// EMIT (HRT_FLAG_NEE_EMITTERS, with NEE only): the MIS weight of emission found on any entry of the emitter table
// LOBES (HRT_FLAG_NEE_LOBES, with NEE only): rough Metal and Isotropic vertices are eligible too
template <bool STATS, bool NEE, bool ENV = false, bool EMIT = false, bool LOBES = false>
__global__ __launch_bounds__(256, HRT_SHADE_WAVES) void HRT_K(k_wf_shade)(DScene sc, hrt_params pr, RenderMap map, WfScene ws, unsigned n_local, int s0, int round,
                                                         WfBuf w, DeviceCounters* counters HRT_RR_PARAMS) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    __shared__ __attribute__((aligned(16))) uint32_t s_tables[HRT_TABLE_LDS_BYTES / 4];
    __shared__ float s_missq[4][(ENV ? 8 : 7) * HRT_MISSQ_CAP];
#ifdef HRT_SHADE_PROFILE
    g_prof_counters = counters;
#endif
    stage_tables(sc, s_tables);
    MissQueue mq;
    mq.f = s_missq[threadIdx.x >> 6]; mq.slot = (unsigned*)(mq.f + (ENV ? 7 : 6) * HRT_MISSQ_CAP); mq.count = 0;
    unsigned n_seg = 0, n_culled = 0;
    PathCounters pc; pc.rays = 0; pc.samples = 0; pc.mesh_hits = 0; pc.env_lookups = 0; pc.bvh.box_tests = 0; pc.bvh.tri_tests = 0;
    HRT_FOR_MY_TASKS(task, w, wave, lane) {
        unsigned live, qn, rn;
        wf_shade_task<STATS, NEE, ENV, EMIT, LOBES, HRT_STRAT, HRT_RR_ON>(sc, pr, map, ws, n_local, s0, round, w, task, HRT_UNIFORM(w.live[task]), lane, lt, mq, pc, n_seg, n_culled, live, qn, rn HRT_RR_ARGS);
        if (lane == 0) { w.live[task] = live; w.qn[task] = qn; w.rn[task] = rn; if (rn) wf_ref_publish(w, task, rn); }
    }
    if (mq.count) missq_flush<STATS, ENV>(sc, w, mq, lane, mq.count, pc);
    wf_shade_counters<STATS>(w, counters, wave, lane, n_seg, n_culled, pc);
}

#ifndef HRT_RR
// The light samples of one round's survivors (the comment at the place of inclusion in hrt_hip.hip says what they are).  With HRT_STRAT
// the RNG_LIGHT and RNG_ENV draws are the stratified sampler's; the shadow rays' ConstantMedium draws inside world_hit keep rng_draw.
template <bool ENV, bool EMIT = false, bool LOBES = false>
__global__ __launch_bounds__(HRT_BLOCK) void HRT_K(k_wf_shadow)(DScene sc, hrt_params pr, RenderMap map, unsigned n_local, int s0, int round, WfBuf w) {
    __shared__ int s_stack[HRT_STACK_DEPTH * HRT_BLOCK];
    __shared__ __attribute__((aligned(16))) uint32_t s_tables[HRT_TABLE_LDS_BYTES / 4];
    __shared__ unsigned s_queue[HRT_BLOCK / 64][HRT_SHADOWQ_CAP];
    int* stack = s_stack + threadIdx.x;
    stage_tables(sc, s_tables);
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    unsigned* const q = s_queue[threadIdx.x >> 6];
    const int nxt = (round + 1) & 1;
    unsigned n_shadow = 0;
    unsigned qn = 0;                          // wave-uniform queue length
    TaskPuller puller = HRT_TASK_PULLER(wave, w.n_groups);
    unsigned task = 0, j0 = 0, n = 0;
    bool have = wf_next_task(w, puller, lane, task);
    if (have) n = HRT_UNIFORM(w.live[task]);
    for (;;) {
        // fill: whole 64-position chunks of this wave's tasks until 64 eligible positions wait (or the tasks are done)
        while (have && qn < 64) {
            if (j0 >= n) {
                have = wf_next_task(w, puller, lane, task);
                j0 = 0;
                n = have ? HRT_UNIFORM(w.live[task]) : 0u;
                continue;
            }
            const unsigned pos = task * w.T + j0 + lane;
            const bool elig = j0 + lane < n && w.N[nxt][HRT_NREC(pos)].w >= 0.0f;
            const unsigned long long m = __ballot(elig);
            if (elig) q[qn + lanes_below(m)] = pos;
            qn += (unsigned)__popcll(m);          // < 64 + 64 <= HRT_SHADOWQ_CAP
            j0 += 64;
        }
        const unsigned k = qn < 64 ? qn : 64u;
        if (k == 0) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const unsigned pos = lane < k ? q[qn - k + lane] : 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        qn -= k;
        if (lane >= k) continue;
        const float4 nr = w.N[nxt][HRT_NREC(pos)];
        const float4 mr = LOBES ? w.N[nxt][HRT_NREC(pos) + 1] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#ifdef HRT_LOBES_NO_ACC   // experiment only: no correction for the bounce's survival -- the biased estimator
        const float inv_acc = 1.0f;
#else
        const float inv_acc = LOBES ? nee_vertex_inv_acc(nr, mr) : 1.0f;
#endif     // a Metal vertex samples only when its bounce survived
        const float4 a = w.S0[nxt][pos], b = w.S1[nxt][pos];
        const float az = w.S3[nxt][pos];
        const unsigned slot = __float_as_uint(w.S2[nxt][pos].w);
        const vec3 x(a.x, a.y, a.z);
        [&]() {   // the table-light sample (a lambda: `return` ends it, and the environment sample below still runs)
            if (ENV && (EMIT ? w.n_emit : w.n_lights) == 0) return;
            rng_ctx ctx = slot_ctx(pr, map, slot, n_local, s0, round);
            const u32x4 u = rng_draw_as<HRT_STRAT>(ctx, RNG_LIGHT, 0);
            if (EMIT) {
                const int li = emit_choose(w.emit_alias, w.n_emit, u.x, rng_draw_as<HRT_STRAT>(ctx, RNG_LIGHT, 1).x);
                const float4 E0 = w.emit_rec[HRT_EMIT_REC * li], E1 = w.emit_rec[HRT_EMIT_REC * li + 1], E2 = w.emit_rec[HRT_EMIT_REC * li + 2];
                vec3 wd;
                float pl, reach;
                const int kind = __float_as_int(E0.y);
                const bool ok = kind == HRT_PRIM_SPHERE ? nee_sample(E0, E1, E2, x, u.y, u.z, wd, pl, reach)
                                                        : emit_sample_planar(kind == HRT_EMIT_TRI, E1, E2, w.emit_rec[HRT_EMIT_REC * li + 3], x, u.y, u.z, wd, pl, reach);
                if (!ok) return;
                float t0, t1;
                const float pb = LOBES ? nee_vertex_pdf(nr, mr, wd, t0, t1) : nee_bsdf_pdf(vec3(nr.x, nr.y, nr.z), wd, t0, t1);
                if (!(pb > 0.0f)) return;
                const float tk = LOBES ? nee_vertex_len(mr.w, nee_pick_root(t0, t1, u.w), u.w) : nee_pick_root(t0, t1, u.w);
                if (LOBES && !(tk > 0.0f)) return;
                const vec3 d = tk * wd;
#ifdef HRT_EMIT_EUCLID_TMAX
                const float t_max = reach / tk * 1.001f;
#else
                const float t_max = E2.w != 0.0f ? __builtin_huge_valf() : reach / tk * 1.001f;   // E2.w: wrapped
#endif
                ctx.bounce = (uint32_t)round | HRT_RNG_SHADOW;
                ++n_shadow;
                DCounters cnt; cnt.box_tests = 0; cnt.tri_tests = 0;
                const WorldHit wh = world_hit<false>(sc, x, d, pr.t_min, t_max, pr.quirks, ctx, stack, cnt);
                const int esub = __float_as_int(E0.w);
                if (wh.prim != __float_as_int(E0.x) || (esub >= 0 && sub_tri(wh.sub) != esub)) return;
                DRec rec;
                hit_record(sc, wh, x, d, pr.quirks, pr.t_min, rec);
                const vec3 term = vec3(b.z, b.w, az) * nee_emitted(sc, rec) * (LOBES ? nee_mis_shadow(pb, E0.z * pl) * inv_acc : nee_mis_shadow(pb, E0.z * pl));
                const float4 acc = w.direct[slot];
                w.direct[slot] = make_float4(acc.x + term.x, acc.y + term.y, acc.z + term.z, 0.0f);
                return;
            }
            const int li = nee_choose(w.lights, w.n_lights, u.x);
            const float4 L0 = w.lights[HRT_NEE_REC * li], L1 = w.lights[HRT_NEE_REC * li + 1], L2 = w.lights[HRT_NEE_REC * li + 2];
            vec3 wd;
            float pl, reach;
            if (!nee_sample(L0, L1, L2, x, u.y, u.z, wd, pl, reach)) return;
            float t0, t1;
            const float pb = LOBES ? nee_vertex_pdf(nr, mr, wd, t0, t1) : nee_bsdf_pdf(vec3(nr.x, nr.y, nr.z), wd, t0, t1);
            if (!(pb > 0.0f)) return;
#ifdef HRT_NEE_UNIT_SHADOW
            const float tk = 1.0f;
#else
            const float tk = LOBES ? nee_vertex_len(mr.w, nee_pick_root(t0, t1, u.w), u.w) : nee_pick_root(t0, t1, u.w);
            if (LOBES && !(tk > 0.0f)) return;
#endif
            const vec3 d = tk * wd;
            ctx.bounce = (uint32_t)round | HRT_RNG_SHADOW;
            ++n_shadow;
            DCounters cnt; cnt.box_tests = 0; cnt.tri_tests = 0;
            const WorldHit wh = world_hit<false>(sc, x, d, pr.t_min, reach / tk * 1.001f, pr.quirks, ctx, stack, cnt);
            if (wh.prim != __float_as_int(L0.x)) return;
            DRec rec;
            hit_record(sc, wh, x, d, pr.quirks, pr.t_min, rec);
            const vec3 term = vec3(b.z, b.w, az) * nee_emitted(sc, rec) * (LOBES ? nee_mis_shadow(pb, L0.z * pl) * inv_acc : nee_mis_shadow(pb, L0.z * pl));
            const float4 acc = w.direct[slot];
            w.direct[slot] = make_float4(acc.x + term.x, acc.y + term.y, acc.z + term.z, 0.0f);
        }();
        if (ENV) {   // the environment sample of the same vertex
            rng_ctx ctx = slot_ctx(pr, map, slot, n_local, s0, round);
            vec3 we;
            float pe, t0, t1;
            int ci, cj;
            if (!env_sample(w.env_marg, w.env_cond, w.env_w, w.env_h, rng_draw_as<HRT_STRAT>(ctx, RNG_ENV, 0), we, pe, ci, cj)) continue;
            const float pb = LOBES ? nee_vertex_pdf(nr, mr, we, t0, t1) : nee_bsdf_pdf(vec3(nr.x, nr.y, nr.z), we, t0, t1);
            if (!(pb > 0.0f)) continue;
            const uint32_t ur = rng_draw_as<HRT_STRAT>(ctx, RNG_ENV, 1).x;
            const float te = LOBES ? nee_vertex_len(mr.w, nee_pick_root(t0, t1, ur), ur) : nee_pick_root(t0, t1, ur);
            if (LOBES && !(te > 0.0f)) continue;
            const vec3 d = te * we;
            pe = env_pdf(w.env_marg, w.env_cond, w.env_w, w.env_h, d);   // the density of the texel background_value reads for d
            if (!(pe > 0.0f)) continue;
            ctx.bounce = (uint32_t)round | HRT_RNG_SHADOW | HRT_RNG_SHADOW_ENV;
            ++n_shadow;
            DCounters cnt; cnt.box_tests = 0; cnt.tri_tests = 0;
            const WorldHit wh = world_hit<false>(sc, x, d, pr.t_min, __builtin_huge_valf(), pr.quirks, ctx, stack, cnt);
            if (wh.prim >= 0) continue;
            const vec3 term = vec3(b.z, b.w, az) * background_value(sc, d) * (LOBES ? nee_mis_shadow(pb, pe) * inv_acc : nee_mis_shadow(pb, pe));
            const float4 acc = w.direct[slot];
            w.direct[slot] = make_float4(acc.x + term.x, acc.y + term.y, acc.z + term.z, 0.0f);
        }
    }
    const unsigned c = wave_sum(n_shadow);
    if (lane == 0 && c) w.wave_shadow[wave] += (unsigned long long)c;      // this wave's own cell
}
#endif   // !HRT_RR
#undef HRT_RR_ON
#undef HRT_RR_PARAMS
#undef HRT_RR_ARGS
