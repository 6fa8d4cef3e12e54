// hrt_filter.hip -- the film reconstruction filters of include/hrt.h ("reconstruction filter"): tent, cubic B-spline
// and Mitchell-Netravali.
//
// Under HRT_FLAG_FILTER a pixel is no longer the plain mean of the samples whose jitter fell inside it (k_wf_reduce) but the weighted
// mean of the samples of its neighbourhood, each weighted by the filter's value at the sample's distance from the pixel's centre.  The
// pass is a GATHER over what a wavefront batch already holds -- the per-sample radiances WfBuf::rad (+ direct under NEE) and the samples'
// jitters, which are a pure function of (seed, pixel, sample) -- so no path carries a signed weight and nothing upstream changes.  The
// definition -- every operation and its order -- is in include/hrt.h; tests/filter_np.py restates those words in numpy float32 and the
// kernels must give its bits, which is why the arithmetic below is plain + - * / , fabsf and comparisons, written in the header's order,
// under -ffp-contract=off.
//
//   k_flt_gather<N, STRAT>   once per batch, in place of k_wf_reduce's film write: acc += w * v over the batch's samples; a batch that
//                            holds all the samples of the render also sums the weights and finishes its pixels
//   k_flt_finish<N, STRAT>   once per render that took several batches, by the call that reaches params->samples: Wsum over all
//                            samples, acc / Wsum, clamp at 0
//
// Both run 16 x 16-pixel blocks.  Per sample a block stages the (16 + 2 N)^2 cells of its pixels and their halo in LDS -- the jitter
// (one Philox or stratified draw per cell, not one per tap) and, in the gather, the radiance --, then, after a barrier, the cells' 1-D
// weights k(tx) and k(ty) for each of the 2 N + 1 offsets (flt_stage_weights: the divisions and polynomials once per cell and offset,
// not once per tap), and after a second barrier every thread walks its (2 N + 1)^2 taps in the header's order, a product of two staged
// weights each; a third barrier frees the tile for the next sample.  N is the window's half-width: 0 for R = 0.5, 1 for R <= 1.5, 2 for
// R <= 2.5; the header's support test decides which taps count, the window only has to hold them.  A cell outside the call's rectangle
// gets a NaN jitter: it fails the support test like any tap that is too far, so the tap loop has no bounds test.  Every pixel is
// written by its own thread only: no atomics, and the result does not depend on scheduling.  LDS per block: 24 + 8 (2 N + 1) bytes per
// cell for the gather, 25 600 at N = 2 (6 blocks per CU's 160 KB), 16 less per cell for the finishing kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/hrt.h"
#include "hrt_rng.h"

extern "C" __attribute__((visibility("hidden"))) void hrt_set_last_error(const char* msg);   // hrt_hip.hip
// defined at the end of this file; hrt_hip.hip declares the same three
extern "C" __attribute__((visibility("hidden"))) hrt_status hrt_filter_resolve(int32_t kind, float radius, float* resolved);
extern "C" __attribute__((visibility("hidden"))) hipError_t hrt_filter_gather_launch(int32_t kind, float radius, int32_t W, hrt_rect rect, uint32_t seed_lo, uint32_t seed_hi,
                                                                                     int strat, const float4* rad, const float4* direct, unsigned n_local, int s0,
                                                                                     int chunk, int first, int finish, float* acc, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t hrt_filter_finish_launch(int32_t kind, float radius, int32_t W, hrt_rect rect, uint32_t seed_lo, uint32_t seed_hi,
                                                                                     int strat, int samples, float* acc, hipStream_t stream);

namespace {

using namespace hrt;

#define HRT_FLT_TILE 16

struct FltArgs {
    int32_t W;                   // the film's width: a sample's RNG key holds the pixel's index in the FILM
    int32_t x0, y0, rw, rh;      // the call's rectangle; local pixel lp = ly * rw + lx
    uint32_t seed_lo, seed_hi;
    int32_t kind;
    float R;
};

// the 1-D kernels of include/hrt.h for t in [0, 1); 16/3, -7/3 and 32/3 are the nearest floats
__device__ inline float flt_k(int kind, float t) {
    if (kind == HRT_FILTER_TENT) return 1.0f - t;
    const float x = t + t;
    float a;
    if (kind == HRT_FILTER_BSPLINE) {
        if (x < 1.0f) { a = 3.0f * x - 6.0f; a = a * x; a = a * x; a = a + 4.0f; }
        else { const float u = 2.0f - x; a = (u * u) * u; }
    } else {
        if (x < 1.0f) { a = 7.0f * x - 12.0f; a = a * x; a = a * x; a = a + 0x1.555556p+2f; }
        else { a = -0x1.2aaaaap+1f * x + 12.0f; a = a * x - 20.0f; a = a * x + 0x1.555556p+3f; }
    }
    return a / 6.0f;
}

// the jitter of sample s of the rectangle's pixel (lx, ly): words x, y of the RNG_JITTER site at bounce 0, as path_begin draws them
template <bool STRAT>
__device__ inline float2 flt_jitter(const FltArgs& a, int lx, int ly, int s) {
    rng_ctx ctx;
    ctx.seed_lo = a.seed_lo; ctx.seed_hi = a.seed_hi;
    ctx.pixel = (uint32_t)((a.y0 + ly) * a.W + (a.x0 + lx)); ctx.sample = (uint32_t)s; ctx.bounce = 0;
    const u32x4 u = rng_draw_as<STRAT>(ctx, RNG_JITTER, 0);
    return make_float2(u01(u.x), u01(u.y));
}

// Stages one sample's 1-D weights: for every cell c of the tile and every offset o in -N .. N the weight the cell's sample has for the
// output pixel o columns (wgt[(o + N) * CELLS + c]) or o rows ((T + o + N) * CELLS + c) away from the pixel that owns it, or a NaN
// where the header's support test fails.  A tap (ox, oy) at cell c then is wgt_x[ox][c] * wgt_y[oy][c]: the header's k(tx) * k(ty), each
// factor computed once per cell and offset instead of once per tap -- 2 (2N + 1) divisions-and-polynomials per cell where the taps of the
// threads around it would make 2 (2N + 1)^2.
template <int N>
__device__ inline void flt_stage_weights(const FltArgs& a, const float2* jit, float* wgt, int tid) {
    constexpr int S = HRT_FLT_TILE + 2 * N, CELLS = S * S, T = 2 * N + 1;
    for (int i = tid; i < 2 * T * CELLS; i += HRT_FLT_TILE * HRT_FLT_TILE) {
        const int ao = i / CELLS, c = i - ao * CELLS;
        const int axis = ao / T, o = ao - axis * T - N;
        const float2 j = jit[c];
        // x: dx = ((float)(qx - px) + jx) - 0.5f with qx - px = o;  y: dy = ((float)(py - qy) + jy) - 0.5f with py - qy = -o
        const float d = ((float)(axis ? -o : o) + (axis ? j.y : j.x)) - 0.5f;
        const float t = fabsf(d) / a.R;
        wgt[i] = t < 1.0f ? flt_k(a.kind, t) : __builtin_nanf("");
    }
}

// the jitters of sample s of the tile's cells; a cell outside the rectangle gets NaNs
template <int N, bool STRAT>
__device__ inline float2 flt_cell_jitter(const FltArgs& a, int qx, int qy, int s) {
    if (qx >= 0 && qx < a.rw && qy >= 0 && qy < a.rh) return flt_jitter<STRAT>(a, qx, qy, s);
    return make_float2(__builtin_nanf(""), __builtin_nanf(""));
}

// rad / direct: [chunk][n_local] float4, sample s0 + k in slab k (WfBuf::rad's layout); direct may be NULL.  first: acc starts from +0.
// finish: the batch holds ALL the samples of the render (first, and s0 + chunk == samples), so the weight sum this kernel adds up beside
// acc -- the same taps in the same order, from +0 -- is the header's Wsum and the pixel is finished here; k_flt_finish is not launched.
template <int N, bool STRAT>
__global__ __launch_bounds__(256) void k_flt_gather(FltArgs a, const float4* __restrict__ rad, const float4* __restrict__ direct, unsigned n_local,
                                                    int s0, int chunk, int first, int finish, float* __restrict__ acc) {
    constexpr int S = HRT_FLT_TILE + 2 * N, CELLS = S * S, T = 2 * N + 1;
    __shared__ float4 val[CELLS];
    __shared__ float2 jit[CELLS];
    __shared__ float wgt[2 * T * CELLS];
    const int tid = threadIdx.y * HRT_FLT_TILE + threadIdx.x;
    const int bx0 = blockIdx.x * HRT_FLT_TILE - N, by0 = blockIdx.y * HRT_FLT_TILE - N;
    const int lx = blockIdx.x * HRT_FLT_TILE + threadIdx.x, ly = blockIdx.y * HRT_FLT_TILE + threadIdx.y;
    const bool mine = lx < a.rw && ly < a.rh;
    const size_t lp = mine ? (size_t)ly * a.rw + lx : 0;
    float r = 0.0f, g = 0.0f, b = 0.0f, wsum = 0.0f;
    if (mine && !first) { r = acc[3 * lp]; g = acc[3 * lp + 1]; b = acc[3 * lp + 2]; }
    for (int k = 0; k < chunk; ++k) {
        for (int c = tid; c < CELLS; c += HRT_FLT_TILE * HRT_FLT_TILE) {
            const int cy = c / S, cx = c - cy * S;
            const int qx = bx0 + cx, qy = by0 + cy;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (qx >= 0 && qx < a.rw && qy >= 0 && qy < a.rh) {
                const size_t i = (size_t)k * n_local + ((size_t)qy * a.rw + qx);
                v = rad[i];
                if (direct) { const float4 d = direct[i]; v.x = v.x + d.x; v.y = v.y + d.y; v.z = v.z + d.z; }   // wf_sample_value
            }
            val[c] = v; jit[c] = flt_cell_jitter<N, STRAT>(a, qx, qy, s0 + k);
        }
        __syncthreads();
        flt_stage_weights<N>(a, jit, wgt, tid);
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int oy = -N; oy <= N; ++oy)
#pragma unroll
                for (int ox = -N; ox <= N; ++ox) {
                    const int c = (threadIdx.y + N + oy) * S + threadIdx.x + N + ox;
                    const float kx = wgt[(ox + N) * CELLS + c], ky = wgt[(T + oy + N) * CELLS + c];
                    if (kx == kx && ky == ky) {       // both inside the support: the tap counts
                        const float w = kx * ky;
                        const float4 v = val[c];
                        r = r + w * v.x; g = g + w * v.y; b = b + w * v.z;
                        wsum = wsum + w;
                    }
                }
        }
        __syncthreads();
    }
    if (!mine) return;
    if (finish) {
        r = wsum > 0.0f ? r / wsum : 0.0f; g = wsum > 0.0f ? g / wsum : 0.0f; b = wsum > 0.0f ? b / wsum : 0.0f;
        r = r < 0.0f ? 0.0f : r; g = g < 0.0f ? 0.0f : g; b = b < 0.0f ? 0.0f : b;          // a NaN stays a NaN
    }
    acc[3 * lp] = r; acc[3 * lp + 1] = g; acc[3 * lp + 2] = b;
}

template <int N, bool STRAT>
__global__ __launch_bounds__(256) void k_flt_finish(FltArgs a, int samples, float* __restrict__ acc) {
    constexpr int S = HRT_FLT_TILE + 2 * N, CELLS = S * S, T = 2 * N + 1;
    __shared__ float2 jit[CELLS];
    __shared__ float wgt[2 * T * CELLS];
    const int tid = threadIdx.y * HRT_FLT_TILE + threadIdx.x;
    const int bx0 = blockIdx.x * HRT_FLT_TILE - N, by0 = blockIdx.y * HRT_FLT_TILE - N;
    const int lx = blockIdx.x * HRT_FLT_TILE + threadIdx.x, ly = blockIdx.y * HRT_FLT_TILE + threadIdx.y;
    const bool mine = lx < a.rw && ly < a.rh;
    float wsum = 0.0f;
    for (int s = 0; s < samples; ++s) {
        for (int c = tid; c < CELLS; c += HRT_FLT_TILE * HRT_FLT_TILE) {
            const int cy = c / S, cx = c - cy * S;
            jit[c] = flt_cell_jitter<N, STRAT>(a, bx0 + cx, by0 + cy, s);
        }
        __syncthreads();
        flt_stage_weights<N>(a, jit, wgt, tid);
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int oy = -N; oy <= N; ++oy)
#pragma unroll
                for (int ox = -N; ox <= N; ++ox) {
                    const int c = (threadIdx.y + N + oy) * S + threadIdx.x + N + ox;
                    const float kx = wgt[(ox + N) * CELLS + c], ky = wgt[(T + oy + N) * CELLS + c];
                    if (kx == kx && ky == ky) wsum = wsum + kx * ky;
                }
        }
        __syncthreads();
    }
    if (!mine) return;
    const size_t lp = (size_t)ly * a.rw + lx;
    for (int k = 0; k < 3; ++k) {
        const float v = acc[3 * lp + k];
        float o = wsum > 0.0f ? v / wsum : 0.0f;
        o = o < 0.0f ? 0.0f : o;          // a NaN stays a NaN
        acc[3 * lp + k] = o;
    }
}

int flt_half_width(float R) { return R <= 0.5f ? 0 : (R <= 1.5f ? 1 : 2); }

dim3 flt_grid(const FltArgs& a) { return dim3((a.rw + HRT_FLT_TILE - 1) / HRT_FLT_TILE, (a.rh + HRT_FLT_TILE - 1) / HRT_FLT_TILE); }

template <typename F>
void with_window(int n, bool strat, F&& f) {
    auto by_sampler = [&](auto NN) {
        if (strat) f(NN, std::true_type{});
        else f(NN, std::false_type{});
    };
    switch (n) {
        case 0: by_sampler(std::integral_constant<int, 0>{}); break;
        case 1: by_sampler(std::integral_constant<int, 1>{}); break;
        default: by_sampler(std::integral_constant<int, 2>{}); break;
    }
}

FltArgs flt_args(int32_t kind, float radius, int32_t W, hrt_rect rect, uint32_t seed_lo, uint32_t seed_hi) {
    FltArgs a;
    a.W = W; a.x0 = rect.x0; a.y0 = rect.y0; a.rw = rect.w; a.rh = rect.h;
    a.seed_lo = seed_lo; a.seed_hi = seed_hi; a.kind = kind; a.R = radius;
    return a;
}

struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
struct DevMem {
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
};
hrt_status ffail(hrt_status st, const std::string& msg) { hrt_set_last_error(msg.c_str()); return st; }
#define FCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return ffail(e_ == hipErrorOutOfMemory ? HRT_ERR_OOM : HRT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

hrt_status filter_samples_impl(int device, int32_t kind, float radius, int32_t W, int32_t H, hrt_rect rect, uint32_t seed_lo, uint32_t seed_hi,
                               int32_t stratified, int32_t samples, const float* rad, float* out) {
    const std::string who = "hrt_filter_samples";
    float R = 0.0f;
    const hrt_status sf = hrt_filter_resolve(kind, radius, &R);
    if (sf != HRT_OK) return sf;
    if (!rad || !out) return ffail(HRT_ERR_INVALID, who + ": NULL argument");
    if (W < 1 || H < 1 || (int64_t)W * H > (int64_t)1 << 30) return ffail(HRT_ERR_INVALID, who + ": the film must hold 1 .. 2^30 pixels");
    if (rect.w <= 0 || rect.h <= 0 || rect.x0 < 0 || rect.y0 < 0 || rect.x0 > W - rect.w || rect.y0 > H - rect.h)
        return ffail(HRT_ERR_INVALID, who + ": rectangle empty or outside the film");
    if (samples < 1) return ffail(HRT_ERR_INVALID, who + ": samples must be >= 1");
    if (stratified != 0 && stratified != 1) return ffail(HRT_ERR_INVALID, who + ": stratified must be 0 or 1");
    DeviceGuard guard;
    int n_dev = 0;
    FCHK(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return ffail(HRT_ERR_NO_DEVICE, who + ": no such device");
    FCHK(hipSetDevice(device));
    // the samples go up in batches of at most 64 MiB of float4 slots, each gathered as a render's batch is
    const size_t n = (size_t)rect.w * rect.h;
    const int chunk = (int)std::min<size_t>((size_t)samples, std::max<size_t>(1, ((size_t)4 << 20) / n));
    DevMem d_rad, d_acc;
    FCHK(hipMalloc(&d_rad.p, (size_t)chunk * n * sizeof(float4)));
    FCHK(hipMalloc(&d_acc.p, n * 3 * sizeof(float)));
    std::vector<float> staged((size_t)chunk * n * 4);
    for (int s0 = 0; s0 < samples; s0 += chunk) {
        const int c = std::min(chunk, samples - s0);
        const float* src = rad + (size_t)s0 * n * 3;
        for (size_t i = 0; i < (size_t)c * n; ++i) { staged[4 * i] = src[3 * i]; staged[4 * i + 1] = src[3 * i + 1]; staged[4 * i + 2] = src[3 * i + 2]; staged[4 * i + 3] = 0.0f; }
        FCHK(hipMemcpy(d_rad.p, staged.data(), (size_t)c * n * sizeof(float4), hipMemcpyHostToDevice));
        FCHK(hrt_filter_gather_launch(kind, R, W, rect, seed_lo, seed_hi, stratified, (const float4*)d_rad.p, nullptr, (unsigned)n, s0, c, s0 == 0 ? 1 : 0,
                                      c == samples ? 1 : 0, (float*)d_acc.p, nullptr));
        FCHK(hipDeviceSynchronize());     // `staged` is reused
    }
    if (chunk < samples) FCHK(hrt_filter_finish_launch(kind, R, W, rect, seed_lo, seed_hi, stratified, samples, (float*)d_acc.p, nullptr));
    FCHK(hipMemcpy(out, d_acc.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return HRT_OK;
}

}  // namespace

// ---- what launch_wavefront (hrt_hip.hip) reaches the kernels through; `radius` is a resolved one (hrt_filter_resolve)
extern "C" __attribute__((visibility("hidden"))) hipError_t hrt_filter_gather_launch(int32_t kind, float radius, int32_t W, hrt_rect rect, uint32_t seed_lo, uint32_t seed_hi,
                                                                                     int strat, const float4* rad, const float4* direct, unsigned n_local, int s0,
                                                                                     int chunk, int first, int finish, float* acc, hipStream_t stream) {
    const FltArgs a = flt_args(kind, radius, W, rect, seed_lo, seed_hi);
    with_window(flt_half_width(radius), strat != 0, [&](auto NN, auto ST) {
        hipLaunchKernelGGL((k_flt_gather<decltype(NN)::value, decltype(ST)::value>), flt_grid(a), dim3(HRT_FLT_TILE, HRT_FLT_TILE), 0, stream, a, rad, direct, n_local, s0,
                           chunk, first, finish, acc);
    });
    return hipGetLastError();
}
extern "C" __attribute__((visibility("hidden"))) hipError_t hrt_filter_finish_launch(int32_t kind, float radius, int32_t W, hrt_rect rect, uint32_t seed_lo, uint32_t seed_hi,
                                                                                     int strat, int samples, float* acc, hipStream_t stream) {
    const FltArgs a = flt_args(kind, radius, W, rect, seed_lo, seed_hi);
    with_window(flt_half_width(radius), strat != 0, [&](auto NN, auto ST) {
        hipLaunchKernelGGL((k_flt_finish<decltype(NN)::value, decltype(ST)::value>), flt_grid(a), dim3(HRT_FLT_TILE, HRT_FLT_TILE), 0, stream, a, samples, acc);
    });
    return hipGetLastError();
}

// kind and radius as the setters and hrt_filter_samples judge them: *resolved = the radius in use (the kind's default for radius <= 0)
extern "C" __attribute__((visibility("hidden"))) hrt_status hrt_filter_resolve(int32_t kind, float radius, float* resolved) {
    if (kind != HRT_FILTER_TENT && kind != HRT_FILTER_BSPLINE && kind != HRT_FILTER_MITCHELL) return ffail(HRT_ERR_INVALID, "filter: unknown kind");
    if (radius != radius) return ffail(HRT_ERR_INVALID, "filter: the radius is NaN");
    const float R = radius <= 0.0f ? (kind == HRT_FILTER_TENT ? 1.0f : 2.0f) : radius;
    if (!(R >= 0.5f && R <= 2.5f)) return ffail(HRT_ERR_INVALID, "filter: the radius must lie in [0.5, 2.5] pixels");
    *resolved = R;
    return HRT_OK;
}

extern "C" hrt_status hrt_filter_samples(int device, int32_t kind, float radius, int32_t W, int32_t H, hrt_rect rect, uint32_t seed_lo, uint32_t seed_hi,
                                         int32_t stratified, int32_t samples, const float* rad, float* out) {
    try {
        return filter_samples_impl(device, kind, radius, W, H, rect, seed_lo, seed_hi, stratified, samples, rad, out);
    } catch (const std::bad_alloc&) { return ffail(HRT_ERR_OOM, "hrt_filter_samples: out of host memory"); }
    catch (const std::exception& e) { return ffail(HRT_ERR_INVALID, std::string("hrt_filter_samples: ") + e.what()); }
    catch (...) { return ffail(HRT_ERR_INVALID, "hrt_filter_samples: unknown C++ exception"); }
}
