// hrt_develop.hip -- hrt_develop*: the develop stage of include/hrt.h ("develop"): pyramid bloom and metered exposure.
//
// The film is blurred by a pyramid of up to 8 half-size levels (a 4 x 4 binomial tap down, a bilinear tap up, every level added on the
// way up), mixed back into the film, metered through an exact 2048-bin histogram of its luminance and scaled.  The definition -- every
// operation and its order -- is in include/hrt.h; tests/develop_np.py restates those words in numpy float32 (float64 where the header
// says so) and the kernels must give its bits, which is why the arithmetic below is plain + - * / and comparisons, written in the
// header's order, under -ffp-contract=off.
//
//   k_dv_down_film  thread per pixel of level 1: rgb (the validity rule applied) -> D_1
//   k_dv_down       thread per pixel of level k + 1: D_k -> D_{k+1}
//   k_dv_up_add     thread per pixel of level k: E_k = D_k + U(E_{k+1}), in place
//   k_dv_meter_film grid-stride over the film: m = mix(rgb, U(E_1) / L) -> the block's histogram in LDS -> the counters
//   k_dv_meter      one block: the counters -> N, mean_ev and scale (float64), the info record and the optional histogram
//   k_dv_write      thread per pixel: m again, times the scale -> out
//
// A level is one float4 per pixel (rgb and a pad), so every tap is one 16-byte load; a level is written once and read by a few
// neighbouring threads, out of the L2 it was just written to, and there is no LDS tile (DESIGN.md 4.17 has the argument).  The workspace
// is the 2048 counters, the info record, and levels 1 .. L.  E_k overwrites D_k: a thread of k_dv_up_add reads its own pixel of level k
// only.  The metered film m is never stored: k_dv_write forms it again from rgb and E_1 with the same operations, reading its own pixel
// of rgb only, which is what makes d_out == d_rgb legal.  The histogram is integer adds on LDS words and one integer global add per
// non-zero bin: integer adds commute, so the counts are exact whatever the schedule.  There are no float atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/hrt.h"

extern "C" __attribute__((visibility("hidden"))) void hrt_set_last_error(const char* msg);   // hrt_hip.hip

namespace {

#define HRT_DV_BLOCK 256
#define HRT_DV_WAVES 4                              // __launch_bounds__(256, 4): at least 4 waves per SIMD
#define HRT_DV_MAX_LEVELS 8
#define HRT_DV_METER_BLOCKS 512                     // the most blocks of k_dv_meter_film, each of which merges a whole histogram (measured)
#define HRT_DV_HIST_BYTES (HRT_DEVELOP_BINS * 4)    // 8192
#define HRT_DV_INFO_BYTES 32                        // the info record's slot (24 bytes used): keeps the pyramid 16-byte aligned

__device__ inline float dv_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ inline bool dv_finite(float x) { return fabsf(x) <= 3.402823466e38f; }
__device__ inline int dv_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
__device__ inline float dv_w(int k) { return (k == 0 || k == 3) ? 0.125f : 0.375f; }

struct DvFilm {                                     // level 0: the film, with the validity rule
    const float* rgb;
    __device__ float4 at(int x, int y, int w) const {
        const size_t i = (size_t)y * w + x;
        const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        const bool valid = dv_finite(r) && dv_finite(g) && dv_finite(b);
        return valid ? make_float4(r, g, b, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
};
struct DvLevel {                                    // a level of the pyramid
    const float4* d;
    __device__ float4 at(int x, int y, int w) const { return d[(size_t)y * w + x]; }
};

// hrt.h step 2: a w x h level -> its (w + 1) / 2 x (h + 1) / 2 successor
template <class Src>
__device__ inline void dv_down(const Src src, float4* __restrict__ dst, int w, int h) {
    const int w2 = (w + 1) / 2, h2 = (h + 1) / 2;
    const unsigned i = blockIdx.x * HRT_DV_BLOCK + threadIdx.x;
    if (i >= (unsigned)w2 * (unsigned)h2) return;
    const int x = (int)(i % (unsigned)w2), y = (int)(i / (unsigned)w2);
    float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int sy = dv_clamp(2 * y - 1 + j, h - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int sx = dv_clamp(2 * x - 1 + k, w - 1);
            const float wt = dv_w(j) * dv_w(k);
            const float4 v = src.at(sx, sy, w);
            r = r + v.x * wt; g = g + v.y * wt; b = b + v.z * wt;
        }
    }
    dst[i] = make_float4(r, g, b, 0.0f);
}

__global__ __launch_bounds__(HRT_DV_BLOCK, HRT_DV_WAVES) void k_dv_down_film(const float* __restrict__ rgb, float4* __restrict__ dst, int w, int h) {
    dv_down(DvFilm{rgb}, dst, w, h);
}
__global__ __launch_bounds__(HRT_DV_BLOCK, HRT_DV_WAVES) void k_dv_down(const float4* __restrict__ src, float4* __restrict__ dst, int w, int h) {
    dv_down(DvLevel{src}, dst, w, h);
}

// hrt.h step 3: U(C)(x, y) of the cw x ch level C
__device__ inline float4 dv_up(const float4* __restrict__ C, int cw, int ch, int x, int y) {
    const int cx = x >> 1, cy = y >> 1;
    const int nx = dv_clamp(cx + ((x & 1) ? 1 : -1), cw - 1), ny = dv_clamp(cy + ((y & 1) ? 1 : -1), ch - 1);
    const float4 a = C[(size_t)cy * cw + cx], b = C[(size_t)cy * cw + nx], c = C[(size_t)ny * cw + cx], d = C[(size_t)ny * cw + nx];
    float4 u;
    u.x = a.x * 0.5625f + b.x * 0.1875f + c.x * 0.1875f + d.x * 0.0625f;
    u.y = a.y * 0.5625f + b.y * 0.1875f + c.y * 0.1875f + d.y * 0.0625f;
    u.z = a.z * 0.5625f + b.z * 0.1875f + c.z * 0.1875f + d.z * 0.0625f;
    u.w = 0.0f;
    return u;
}

// hrt.h step 4: E_k = D_k + U(E_{k+1}), in place on the w x h level `fine`; `coarse` is (w + 1) / 2 x (h + 1) / 2
__global__ __launch_bounds__(HRT_DV_BLOCK, HRT_DV_WAVES) void k_dv_up_add(const float4* __restrict__ coarse, float4* fine, int w, int h) {
    const unsigned i = blockIdx.x * HRT_DV_BLOCK + threadIdx.x;
    if (i >= (unsigned)w * (unsigned)h) return;
    const int x = (int)(i % (unsigned)w), y = (int)(i / (unsigned)w);
    const float4 u = dv_up(coarse, (w + 1) / 2, (h + 1) / 2, x, y);
    const float4 d = fine[i];
    fine[i] = make_float4(d.x + u.x, d.y + u.y, d.z + u.z, 0.0f);
}

struct DvMix {                                      // what steps 4 (its last line) and 5 need; E1 == nullptr: no bloom, m = c
    const float4* E1;
    int W, H;
    float levels;                                   // (float)L
    float s, one_minus_s;
};

// m of pixel i, whose channels are r, g, b; false for an invalid pixel (whose bits stay)
__device__ inline bool dv_mix(const DvMix& mx, unsigned i, float& r, float& g, float& b) {
    if (!(dv_finite(r) && dv_finite(g) && dv_finite(b))) return false;
    if (mx.E1) {
        const int x = (int)(i % (unsigned)mx.W), y = (int)(i / (unsigned)mx.W);
        const float4 u = dv_up(mx.E1, (mx.W + 1) / 2, (mx.H + 1) / 2, x, y);
        const float br = u.x / mx.levels, bg = u.y / mx.levels, bb = u.z / mx.levels;
        r = r * mx.one_minus_s + br * mx.s;
        g = g * mx.one_minus_s + bg * mx.s;
        b = b * mx.one_minus_s + bb * mx.s;
    }
    return true;
}

// the histogram of Y(m): the block's own 2048 counters in LDS, then one global add per non-zero bin
__global__ __launch_bounds__(HRT_DV_BLOCK, HRT_DV_WAVES) void k_dv_meter_film(const float* __restrict__ rgb, DvMix mx, float meter_floor,
                                                                               uint32_t* __restrict__ counters) {
    __shared__ uint32_t bins[HRT_DEVELOP_BINS];
    for (int k = threadIdx.x; k < HRT_DEVELOP_BINS; k += HRT_DV_BLOCK) bins[k] = 0u;
    __syncthreads();
    const unsigned n = (unsigned)mx.W * (unsigned)mx.H;
    for (unsigned i = blockIdx.x * HRT_DV_BLOCK + threadIdx.x; i < n; i += gridDim.x * HRT_DV_BLOCK) {
        float r = rgb[3 * (size_t)i], g = rgb[3 * (size_t)i + 1], b = rgb[3 * (size_t)i + 2];
        if (!dv_mix(mx, i, r, g, b)) continue;
        const float l = dv_lum(r, g, b);
        if (dv_finite(l) && l >= meter_floor) atomicAdd(&bins[(__float_as_uint(l) >> 20) & (HRT_DEVELOP_BINS - 1)], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < HRT_DEVELOP_BINS; k += HRT_DV_BLOCK) {
        const uint32_t c = bins[k];
        if (c) atomicAdd(&counters[k], c);
    }
}

struct DvMeter {
    int mode;                                       // 2: read the counters; 0, 1: the record of a call that does not meter
    float manual_scale;
    uint32_t levels;
    double key, low, high, ev_min, ev_max;
};

// One block, thread t owns bins 8 t .. 8 t + 7 (one stop): the integer prefix of the counts through LDS, then the float64 window sums.
__global__ __launch_bounds__(HRT_DV_BLOCK, HRT_DV_WAVES) void k_dv_meter(const uint32_t* __restrict__ counters, DvMeter mt, hrt_develop_info* __restrict__ ws_info,
                                                                          hrt_develop_info* __restrict__ d_info, uint32_t* __restrict__ d_hist) {
    __shared__ uint32_t before[HRT_DV_BLOCK];       // the counts of the threads below
    __shared__ double part_num[HRT_DV_BLOCK], part_den[HRT_DV_BLOCK];
    const int t = threadIdx.x;
    uint32_t nb[8];
    uint32_t mine = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        nb[k] = mt.mode == 2 ? counters[8 * t + k] : 0u;
        if (d_hist) d_hist[8 * t + k] = nb[k];
        mine += nb[k];
    }
    before[t] = mine;
    __syncthreads();
    for (int step = 1; step < HRT_DV_BLOCK; step <<= 1) {          // an inclusive scan of 256 integers
        const uint32_t add = t >= step ? before[t - step] : 0u;
        __syncthreads();
        before[t] += add;
        __syncthreads();
    }
    const uint32_t N = before[HRT_DV_BLOCK - 1];
    uint32_t C = before[t] - mine;
    const double lo = mt.low * (double)N, hi = mt.high * (double)N;
    const double cmid[8] = {0.0874628412503394, 0.2479275134435855, 0.3923174227787603, 0.5235619560570128,
                            0.6438561897747247, 0.7548875021634686, 0.8579809951275721, 0.9541963103868752};
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double c0 = (double)C, c1 = (double)(C + nb[k]);
        const double top = c1 < hi ? c1 : hi, bottom = c0 > lo ? c0 : lo;
        const double o = top - bottom > 0.0 ? top - bottom : 0.0;
        const double ev = (double)(t - 127) + cmid[k];
        num = num + o * ev;
        den = den + o;
        C += nb[k];
    }
    part_num[t] = num;
    part_den[t] = den;
    __syncthreads();
    if (t != 0) return;
    hrt_develop_info info;
    info.mean_ev = 0.0;
    info.scale = mt.mode == 1 ? mt.manual_scale : 1.0f;
    info.metered = N;
    info.levels = mt.levels;
    info.pad = 0u;
    if (N > 0u) {
        num = 0.0; den = 0.0;
        for (int k = 0; k < HRT_DV_BLOCK; ++k) { num = num + part_num[k]; den = den + part_den[k]; }
        double ev = num / den;
        ev = ev < mt.ev_min ? mt.ev_min : ev > mt.ev_max ? mt.ev_max : ev;
        info.mean_ev = ev;
        info.scale = (float)(mt.key * exp2(-ev));
    }
    *ws_info = info;
    if (d_info) *d_info = info;
}

// out = m * scale for a valid pixel (scale_from: the record k_dv_meter left; NULL: `scale`; apply == 0: out = m), its bits for an invalid one
__global__ __launch_bounds__(HRT_DV_BLOCK, HRT_DV_WAVES) void k_dv_write(const float* rgb, DvMix mx, int apply, float scale,
                                                                          const hrt_develop_info* __restrict__ scale_from, float* out) {
    const unsigned i = blockIdx.x * HRT_DV_BLOCK + threadIdx.x;
    if (i >= (unsigned)mx.W * (unsigned)mx.H) return;
    float r = rgb[3 * (size_t)i], g = rgb[3 * (size_t)i + 1], b = rgb[3 * (size_t)i + 2];
    if (dv_mix(mx, i, r, g, b) && apply) {
        if (scale_from) scale = scale_from->scale;
        r = r * scale; g = g * scale; b = b * scale;
    }
    out[3 * (size_t)i] = r; out[3 * (size_t)i + 1] = g; out[3 * (size_t)i + 2] = b;
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
hrt_status dfail(hrt_status st, const std::string& msg) { hrt_set_last_error(msg.c_str()); return st; }
#define DCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return dfail(e_ == hipErrorOutOfMemory ? HRT_ERR_OOM : HRT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define DLAUNCH(name) do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return dfail(HRT_ERR_HIP, std::string(name " launch: ") + hipGetErrorString(e_)); } while (0)

const size_t kMaxPixels = (size_t)1 << 30;
bool finite(float x) { return std::fabs(x) <= 3.402823466e38f; }
bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// the sizes of levels 1 .. L of a W x H film under bloom_levels = levels; returns L
int pyramid(int32_t W, int32_t H, int32_t levels, int32_t* w, int32_t* h) {
    int L = 0;
    int32_t cw = W, ch = H;
    while (L < levels && (cw > 1 || ch > 1)) {
        cw = (cw + 1) / 2; ch = (ch + 1) / 2;
        w[L] = cw; h[L] = ch;
        ++L;
    }
    return L;
}

// everything that can be refused without a device; `who` prefixes the message
hrt_status check_film(const char* who, int32_t W, int32_t H, const hrt_develop_params* p) {
    const std::string w(who);
    if (!p) return dfail(HRT_ERR_INVALID, w + ": NULL argument");
    if (W < 1 || H < 1) return dfail(HRT_ERR_INVALID, w + ": width and height must be >= 1");
    if ((size_t)W * (size_t)H > kMaxPixels) return dfail(HRT_ERR_INVALID, w + ": more than 2^30 pixels");
    if (p->bloom_levels < 0 || p->bloom_levels > HRT_DV_MAX_LEVELS) return dfail(HRT_ERR_INVALID, w + ": bloom_levels must be 0..8");
    if (!(p->bloom_strength >= 0.0f && p->bloom_strength <= 1.0f)) return dfail(HRT_ERR_INVALID, w + ": bloom_strength must be in [0, 1]");
    if (p->exposure_mode < 0 || p->exposure_mode > 2) return dfail(HRT_ERR_INVALID, w + ": exposure_mode must be 0, 1 or 2");
    if (!finite(p->exposure_ev) || !(std::fabs(p->exposure_ev) <= 64.0f)) return dfail(HRT_ERR_INVALID, w + ": exposure_ev must be finite and within +-64");
    if (!finite(p->key) || !(p->key > 0.0f)) return dfail(HRT_ERR_INVALID, w + ": key must be finite and above 0");
    if (!(p->meter_low >= 0.0f && p->meter_low < p->meter_high && p->meter_high <= 1.0f)) return dfail(HRT_ERR_INVALID, w + ": meter_low and meter_high must satisfy 0 <= meter_low < meter_high <= 1");
    if (!finite(p->meter_floor) || !(p->meter_floor >= 1.17549435e-38f)) return dfail(HRT_ERR_INVALID, w + ": meter_floor must be finite and at least 2^-126");
    if (!finite(p->ev_min) || !finite(p->ev_max) || !(p->ev_min <= p->ev_max)) return dfail(HRT_ERR_INVALID, w + ": ev_min and ev_max must be finite with ev_min <= ev_max");
    return HRT_OK;
}
hrt_status set_device(const char* who, int device) {
    int n_dev = 0;
    DCHK(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return dfail(HRT_ERR_NO_DEVICE, std::string(who) + ": no such device");
    DCHK(hipSetDevice(device));
    return HRT_OK;
}
unsigned blocks(size_t n) { return (unsigned)((n + HRT_DV_BLOCK - 1) / HRT_DV_BLOCK); }

// the launches, on the current device
hrt_status enqueue(int32_t W, int32_t H, const hrt_develop_params& p, const float* d_rgb, float* d_out, hrt_develop_info* d_info, uint32_t* d_hist,
                   void* d_ws, hipStream_t stream) {
    const size_t n = (size_t)W * H;
    uint32_t* counters = (uint32_t*)d_ws;
    hrt_develop_info* ws_info = (hrt_develop_info*)((char*)d_ws + HRT_DV_HIST_BYTES);
    float4* level[HRT_DV_MAX_LEVELS];
    int32_t lw[HRT_DV_MAX_LEVELS], lh[HRT_DV_MAX_LEVELS];
    const int L = pyramid(W, H, p.bloom_levels, lw, lh);
    float4* next = (float4*)((char*)d_ws + HRT_DV_HIST_BYTES + HRT_DV_INFO_BYTES);
    for (int k = 0; k < L; ++k) { level[k] = next; next += (size_t)lw[k] * lh[k]; }
    const bool bloom = L > 0 && p.bloom_strength != 0.0f;
    const bool meter = p.exposure_mode == 2;

    if (meter) DCHK(hipMemsetAsync(counters, 0, HRT_DV_HIST_BYTES, stream));
    if (bloom) {
        hipLaunchKernelGGL(k_dv_down_film, dim3(blocks((size_t)lw[0] * lh[0])), dim3(HRT_DV_BLOCK), 0, stream, d_rgb, level[0], W, H);
        DLAUNCH("k_dv_down_film");
        for (int k = 1; k < L; ++k) {
            hipLaunchKernelGGL(k_dv_down, dim3(blocks((size_t)lw[k] * lh[k])), dim3(HRT_DV_BLOCK), 0, stream, (const float4*)level[k - 1], level[k], lw[k - 1], lh[k - 1]);
            DLAUNCH("k_dv_down");
        }
        for (int k = L - 2; k >= 0; --k) {
            hipLaunchKernelGGL(k_dv_up_add, dim3(blocks((size_t)lw[k] * lh[k])), dim3(HRT_DV_BLOCK), 0, stream, (const float4*)level[k + 1], level[k], lw[k], lh[k]);
            DLAUNCH("k_dv_up_add");
        }
    }
    DvMix mx;
    mx.E1 = bloom ? level[0] : nullptr;
    mx.W = W; mx.H = H;
    mx.levels = (float)(L > 0 ? L : 1);
    mx.s = p.bloom_strength;
    mx.one_minus_s = 1.0f - p.bloom_strength;
    const float manual = (float)std::exp2((double)p.exposure_ev);
    if (meter) {
        const unsigned g = blocks(n) < HRT_DV_METER_BLOCKS ? blocks(n) : HRT_DV_METER_BLOCKS;
        hipLaunchKernelGGL(k_dv_meter_film, dim3(g), dim3(HRT_DV_BLOCK), 0, stream, d_rgb, mx, p.meter_floor, counters);
        DLAUNCH("k_dv_meter_film");
    }
    if (meter || d_info || d_hist) {
        DvMeter mt;
        mt.mode = p.exposure_mode;
        mt.manual_scale = manual;
        mt.levels = (uint32_t)L;
        mt.key = (double)p.key; mt.low = (double)p.meter_low; mt.high = (double)p.meter_high;
        mt.ev_min = (double)p.ev_min; mt.ev_max = (double)p.ev_max;
        hipLaunchKernelGGL(k_dv_meter, dim3(1), dim3(HRT_DV_BLOCK), 0, stream, (const uint32_t*)counters, mt, ws_info, d_info, d_hist);
        DLAUNCH("k_dv_meter");
    }
    hipLaunchKernelGGL(k_dv_write, dim3(blocks(n)), dim3(HRT_DV_BLOCK), 0, stream, d_rgb, mx, p.exposure_mode != 0 ? 1 : 0, manual,
                       meter ? (const hrt_develop_info*)ws_info : nullptr, d_out);
    DLAUNCH("k_dv_write");
    return HRT_OK;
}

uint64_t workspace_bytes(int32_t W, int32_t H, int32_t levels) {
    int32_t lw[HRT_DV_MAX_LEVELS], lh[HRT_DV_MAX_LEVELS];
    const int L = pyramid(W, H, levels, lw, lh);
    uint64_t bytes = HRT_DV_HIST_BYTES + HRT_DV_INFO_BYTES;
    for (int k = 0; k < L; ++k) bytes += 16ull * (uint64_t)lw[k] * (uint64_t)lh[k];
    return bytes;
}

hrt_status develop_device_impl(int device, int32_t W, int32_t H, const hrt_develop_params* p, const float* d_rgb, float* d_out,
                               hrt_develop_info* d_info, uint32_t* d_hist, void* d_ws, void* stream) {
    const char* who = "hrt_develop_device";
    const hrt_status st = check_film(who, W, H, p);
    if (st != HRT_OK) return st;
    if (!d_rgb || !d_out || !d_ws) return dfail(HRT_ERR_INVALID, std::string(who) + ": NULL argument");
    if (misaligned(d_ws, 16)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: the workspace must be 16-byte aligned");
    if (misaligned(d_rgb, 4) || misaligned(d_out, 4) || misaligned(d_hist, 4)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: float and counter buffers must be 4-byte aligned");
    if (misaligned(d_info, 8)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: the info record must be 8-byte aligned");
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    return enqueue(W, H, *p, d_rgb, d_out, d_info, d_hist, d_ws, (hipStream_t)stream);
}

hrt_status develop_host_impl(int device, int32_t W, int32_t H, const hrt_develop_params* p, const float* rgb, float* out, hrt_develop_info* info,
                             uint32_t* hist) {
    const char* who = "hrt_develop";
    const hrt_status st = check_film(who, W, H, p);
    if (st != HRT_OK) return st;
    if (!rgb || !out) return dfail(HRT_ERR_INVALID, std::string(who) + ": NULL argument");
    if (misaligned(rgb, 4) || misaligned(out, 4) || misaligned(hist, 4)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: float and counter buffers must be 4-byte aligned");
    if (misaligned(info, 8)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: the info record must be 8-byte aligned");
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    // one allocation: workspace | info | histogram | rgb | out -- the first three multiples of 16 bytes
    const size_t n = (size_t)W * H;
    const size_t ws = (size_t)((workspace_bytes(W, H, p->bloom_levels) + 15) & ~(uint64_t)15);
    const size_t o_info = ws, o_hist = o_info + HRT_DV_INFO_BYTES, o_rgb = o_hist + HRT_DV_HIST_BYTES, o_out = o_rgb + 12 * n, total = o_out + 12 * n;
    DevMem mem;
    DCHK(hipMalloc(&mem.p, total));
    char* base = (char*)mem.p;
    DCHK(hipMemcpy(base + o_rgb, rgb, 12 * n, hipMemcpyHostToDevice));
    const hrt_status se = enqueue(W, H, *p, (const float*)(base + o_rgb), (float*)(base + o_out), info ? (hrt_develop_info*)(base + o_info) : nullptr,
                                  hist ? (uint32_t*)(base + o_hist) : nullptr, base, nullptr);
    if (se != HRT_OK) return se;
    // (the null stream: the copies wait for the kernels; nothing is handed out unless every copy succeeded up to it)
    hrt_develop_info got;
    if (info) DCHK(hipMemcpy(&got, base + o_info, sizeof(got), hipMemcpyDeviceToHost));
    if (hist) DCHK(hipMemcpy(hist, base + o_hist, HRT_DV_HIST_BYTES, hipMemcpyDeviceToHost));
    DCHK(hipMemcpy(out, base + o_out, 12 * n, hipMemcpyDeviceToHost));
    if (info) *info = got;
    return HRT_OK;
}

#define DV_TRY try {
#define DV_CATCH(who) } catch (const std::bad_alloc&) { return dfail(HRT_ERR_OOM, who ": out of host memory"); } \
    catch (const std::exception& e) { return dfail(HRT_ERR_INVALID, std::string(who ": ") + e.what()); } \
    catch (...) { return dfail(HRT_ERR_INVALID, who ": unknown C++ exception"); }

}  // namespace

extern "C" void hrt_develop_defaults(hrt_develop_params* p) {
    if (!p) return;
    p->bloom_levels = 0;
    p->bloom_strength = 0.05f;
    p->exposure_mode = 0;
    p->exposure_ev = 0.0f;
    p->key = 0.18f;
    p->meter_low = 0.10f;
    p->meter_high = 0.90f;
    p->meter_floor = 1.52587890625e-05f;   // 2^-16
    p->ev_min = -16.0f;
    p->ev_max = 16.0f;
}

extern "C" uint64_t hrt_develop_workspace_bytes(int32_t W, int32_t H, int32_t levels) {
    if (W < 1 || H < 1 || (size_t)W * (size_t)H > kMaxPixels || levels < 0 || levels > HRT_DV_MAX_LEVELS) return 0;
    return workspace_bytes(W, H, levels);
}

extern "C" hrt_status hrt_develop_device(int device, int32_t W, int32_t H, const hrt_develop_params* params, const float* d_rgb, float* d_out,
                                         hrt_develop_info* d_info, uint32_t* d_hist, void* d_workspace, void* stream) {
    DV_TRY
    return develop_device_impl(device, W, H, params, d_rgb, d_out, d_info, d_hist, d_workspace, stream);
    DV_CATCH("hrt_develop_device")
}

extern "C" hrt_status hrt_develop(int device, int32_t W, int32_t H, const hrt_develop_params* params, const float* rgb, float* out,
                                  hrt_develop_info* info, uint32_t* hist) {
    DV_TRY
    return develop_host_impl(device, W, H, params, rgb, out, info, hist);
    DV_CATCH("hrt_develop")
}
