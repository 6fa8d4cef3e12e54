// hrt_denoise.hip -- hrt_denoise*: the guided denoiser of include/hrt.h ("guided denoiser").
//
// An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) whose luminance weight is scaled by the pixel's own standard
// deviation (the spatial part of SVGF, Schied et al. 2017), over albedo-demodulated radiance, guided by the feature buffers of
// hrt_render_aov_* (first-hit albedo, alpha, normal, depth).  The definition -- every operation and its order -- is in
// include/hrt.h; tests/denoise_np.py restates those words in numpy float32 and the kernels must give its bits, which is why the
// arithmetic below is plain + - * /, sqrtf, fabsf and comparisons, written in the header's order, under -ffp-contract=off.
//
//   k_dn_prepare    thread per pixel: rgb, aov, var -> S = (e.rgb, v) and G = (unit normal, z); an invalid pixel gets G.x = +inf
//   k_dn_variance   thread per pixel, only when no variance is given: the 7 x 7 spatial estimate of v
//   k_dn_atrous     thread per pixel, once per iteration: 3 x 3 mean of v, then the 25 taps at spacing 1 << j; S -> S'
//   k_dn_finish     thread per pixel: e * albedo (an invalid pixel: its input bits) -> out
//   k_dn_resolve    the film's resolve (hrt_device.h film_resolve) for a caller without an hrt_scene
//
// The working state is two float4 per pixel, so a tap costs two 16-byte loads.  A valid pixel's unit normal is never infinite
// (hrt.h: it is n * (1 / sqrtf(n.n)) or 0), so G.x = +inf marks a pixel that no tap may read and that passes through unchanged:
// there is no separate mask.  Blocks are 16 x 16 pixels: a wave covers four rows of 16 pixels, i.e. four runs of 256 contiguous
// bytes per load.  No LDS: the three images of the headline film are 19 MB and every tap after the first touch is a cache hit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>

#include "hrt_device.h"          // film_resolve, read-only (and include/hrt.h)

extern "C" __attribute__((visibility("hidden"))) void hrt_set_last_error(const char* msg);   // hrt_hip.hip

namespace {

#define HRT_DN_TILE 16
#define HRT_DN_WAVES 4           // __launch_bounds__(256, 4): four blocks of four waves per CU, i.e. at least 4 waves per SIMD

__device__ inline float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ inline float dn_pos(float x) { return x > 0.0f ? x : 0.0f; }                       // hrt.h: max(0, x); NaN -> 0
__device__ inline float dn_falloff(float x) { const float u = dn_pos(1.0f - x); return u * u; }   // hrt.h: r(x)
__device__ inline bool dn_finite(float x) { return fabsf(x) <= 3.402823466e38f; }
__device__ inline bool dn_invalid(const float4& g) { return g.x == __builtin_huge_valf(); }
__device__ inline float dn_floor(float a, float floor_) { return a > floor_ ? a : floor_; }

__global__ __launch_bounds__(256, HRT_DN_WAVES) void k_dn_prepare(const float* __restrict__ rgb, const float4* __restrict__ aov,
                                                                   const float* __restrict__ var, float4* __restrict__ S,
                                                                   float4* __restrict__ G, int W, int H, float albedo_floor) {
    const int x = blockIdx.x * HRT_DN_TILE + threadIdx.x, y = blockIdx.y * HRT_DN_TILE + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const float4 A = aov[2 * i], B = aov[2 * i + 1];
    const float cr = rgb[3 * i], cg = rgb[3 * i + 1], cb = rgb[3 * i + 2];
    const float ar = dn_floor(A.x, albedo_floor), ag = dn_floor(A.y, albedo_floor), ab = dn_floor(A.z, albedo_floor);
    float4 s, g;
    s.x = cr / ar; s.y = cg / ag; s.z = cb / ab; s.w = 0.0f;
    if (var) {
        const float v = var[i], ya = dn_lum(ar, ag, ab);
        s.w = (v > 0.0f ? v : 0.0f) / (ya * ya);
    }
    const float d = B.x * B.x + B.y * B.y + B.z * B.z;
    if (d > 0.0f) { const float inv = 1.0f / sqrtf(d); g.x = B.x * inv; g.y = B.y * inv; g.z = B.z * inv; }
    else { g.x = 0.0f; g.y = 0.0f; g.z = 0.0f; }
    g.w = A.w > 0.0f ? B.w / A.w : 0.0f;
    if (!(dn_finite(cr) && dn_finite(cg) && dn_finite(cb))) g.x = __builtin_huge_valf();
    S[i] = s; G[i] = g;
}

// v of a pixel without a given variance: the 7 x 7 window at spacing 1, in-film valid taps in row-major order (the centre included)
__global__ __launch_bounds__(256, HRT_DN_WAVES) void k_dn_variance(const float4* __restrict__ Sin, const float4* __restrict__ G,
                                                                    float4* __restrict__ Sout, int W, int H) {
    const int x = blockIdx.x * HRT_DN_TILE + threadIdx.x, y = blockIdx.y * HRT_DN_TILE + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    float4 s = Sin[i];
    if (!dn_invalid(G[i])) {
        float s1 = 0.0f, s2 = 0.0f, n = 0.0f;
        for (int dy = -3; dy <= 3; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
            for (int dx = -3; dx <= 3; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * W + qx;
                if (dn_invalid(G[q])) continue;
                const float4 t = Sin[q];
                const float l = dn_lum(t.x, t.y, t.z);
                s1 += l; s2 += l * l; n += 1.0f;
            }
        }
        const float m = s1 / n;
        s.w = dn_pos(s2 / n - m * m);
    }
    Sout[i] = s;
}

__global__ __launch_bounds__(256, HRT_DN_WAVES) void k_dn_atrous(const float4* __restrict__ Sin, const float4* __restrict__ G,
                                                                  float4* __restrict__ Sout, int W, int H, int step, float sigma_l,
                                                                  float sigma_z, int normal_squarings) {
    const int x = blockIdx.x * HRT_DN_TILE + threadIdx.x, y = blockIdx.y * HRT_DN_TILE + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const float4 sp = Sin[i], gp = G[i];
    if (dn_invalid(gp)) { Sout[i] = sp; return; }

    // the (1/4, 1/2, 1/4)^2 mean of v over the valid 3 x 3 neighbourhood, normalised by the weights used
    float vs = 0.0f, gs = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * W + qx;
            if (dn_invalid(G[q])) continue;
            const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            vs += g * Sin[q].w; gs += g;
        }
    }
    const float sd = sqrtf(vs / gs);
    const float den_l = sigma_l * sd + 1e-6f;
    const float lp = dn_lum(sp.x, sp.y, sp.z);
    const bool p_zero = gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f;

    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= H) continue;
        const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * W + qx;
            const float4 gq = G[q];
            if (dn_invalid(gq)) continue;
            const float4 sq = Sin[q];
            const float kx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
            float w = kx * ky;
            if (dx != 0 || dy != 0) {
                const bool q_zero = gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f;
                float wn;
                if (p_zero && q_zero) wn = 1.0f;
                else if (p_zero || q_zero) wn = 0.0f;
                else {
                    wn = dn_pos(gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
                    for (int k = 0; k < normal_squarings; ++k) wn = wn * wn;
                }
                const float wz = dn_falloff(fabsf(gp.w - gq.w) / (sigma_z * (gp.w > gq.w ? gp.w : gq.w) + 1e-6f));
                const float wl = dn_falloff(fabsf(lp - dn_lum(sq.x, sq.y, sq.z)) / den_l);
                w = w * wn * wz * wl;
            }
            sr += w * sq.x; sg += w * sq.y; sb += w * sq.z;
            sw += w;
            sv += (w * w) * sq.w;
        }
    }
    float4 o;
    o.x = sr / sw; o.y = sg / sw; o.z = sb / sw; o.w = sv / (sw * sw);
    Sout[i] = o;
}

// out may be rgb itself: a thread reads its own pixel before it writes it, and no other
__global__ __launch_bounds__(256, HRT_DN_WAVES) void k_dn_finish(const float4* __restrict__ S, const float4* __restrict__ G,
                                                                  const float4* __restrict__ aov, const float* rgb, float* out,
                                                                  int W, int H, float albedo_floor) {
    const int x = blockIdx.x * HRT_DN_TILE + threadIdx.x, y = blockIdx.y * HRT_DN_TILE + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    if (!dn_invalid(G[i])) {
        const float4 s = S[i], A = aov[2 * i];
        r = s.x * dn_floor(A.x, albedo_floor); g = s.y * dn_floor(A.y, albedo_floor); b = s.z * dn_floor(A.z, albedo_floor);
    }
    out[3 * i] = r; out[3 * i + 1] = g; out[3 * i + 2] = b;
}

__global__ __launch_bounds__(256) void k_dn_resolve(const float* __restrict__ rgb, long long n_pixels, uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    uint8_t q[3];
    hrt::film_resolve(hrt::vec3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]), q);
    out[3 * i] = q[0]; out[3 * i + 1] = q[1]; out[3 * i + 2] = q[2];
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
bool positive_finite(float x) { return x > 0.0f && x <= 3.402823466e38f; }
bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// everything that can be refused without a device; `who` prefixes the message
hrt_status check_film(const char* who, int32_t W, int32_t H, const hrt_denoise_params* p) {
    const std::string w(who);
    if (!p) return dfail(HRT_ERR_INVALID, w + ": NULL argument");
    if (W < 1 || H < 1) return dfail(HRT_ERR_INVALID, w + ": width and height must be >= 1");
    if ((size_t)W * (size_t)H > kMaxPixels) return dfail(HRT_ERR_INVALID, w + ": more than 2^30 pixels");
    if (p->iterations < 1 || p->iterations > 8) return dfail(HRT_ERR_INVALID, w + ": iterations must be 1..8");
    if (p->normal_squarings < 0 || p->normal_squarings > 10) return dfail(HRT_ERR_INVALID, w + ": normal_squarings must be 0..10");
    if (!positive_finite(p->sigma_l)) return dfail(HRT_ERR_INVALID, w + ": sigma_l must be finite and positive");
    if (!positive_finite(p->sigma_z)) return dfail(HRT_ERR_INVALID, w + ": sigma_z must be finite and positive");
    if (!positive_finite(p->albedo_floor)) return dfail(HRT_ERR_INVALID, w + ": albedo_floor must be finite and positive");
    return HRT_OK;
}
hrt_status set_device(const char* who, int device) {
    int n_dev = 0;
    DCHK(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return dfail(HRT_ERR_NO_DEVICE, std::string(who) + ": no such device");
    DCHK(hipSetDevice(device));
    return HRT_OK;
}

// the launches, on the current device
hrt_status enqueue(int32_t W, int32_t H, const hrt_denoise_params& p, const float* d_rgb, const float* d_aov, const float* d_var,
                   float* d_out, void* d_ws, hipStream_t stream) {
    const size_t n = (size_t)W * H;
    float4* S[2] = {(float4*)d_ws, (float4*)d_ws + n};
    float4* G = (float4*)d_ws + 2 * n;
    const dim3 block(HRT_DN_TILE, HRT_DN_TILE), grid((W + HRT_DN_TILE - 1) / HRT_DN_TILE, (H + HRT_DN_TILE - 1) / HRT_DN_TILE);
    int cur = 0;
    if (d_var) {
        hipLaunchKernelGGL(k_dn_prepare, grid, block, 0, stream, d_rgb, (const float4*)d_aov, d_var, S[0], G, W, H, p.albedo_floor);
        DLAUNCH("k_dn_prepare");
    } else {
        hipLaunchKernelGGL(k_dn_prepare, grid, block, 0, stream, d_rgb, (const float4*)d_aov, d_var, S[1], G, W, H, p.albedo_floor);
        DLAUNCH("k_dn_prepare");
        hipLaunchKernelGGL(k_dn_variance, grid, block, 0, stream, S[1], G, S[0], W, H);
        DLAUNCH("k_dn_variance");
    }
    for (int j = 0; j < p.iterations; ++j) {
        hipLaunchKernelGGL(k_dn_atrous, grid, block, 0, stream, S[cur], G, S[cur ^ 1], W, H, 1 << j, p.sigma_l, p.sigma_z, p.normal_squarings);
        DLAUNCH("k_dn_atrous");
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_dn_finish, grid, block, 0, stream, S[cur], G, (const float4*)d_aov, d_rgb, d_out, W, H, p.albedo_floor);
    DLAUNCH("k_dn_finish");
    return HRT_OK;
}

hrt_status denoise_device_impl(int device, int32_t W, int32_t H, const hrt_denoise_params* p, const float* d_rgb, const float* d_aov,
                               const float* d_var, float* d_out, void* d_ws, void* stream) {
    const char* who = "hrt_denoise_device";
    const hrt_status st = check_film(who, W, H, p);
    if (st != HRT_OK) return st;
    if (!d_rgb || !d_aov || !d_out || !d_ws) return dfail(HRT_ERR_INVALID, std::string(who) + ": NULL argument");
    if (misaligned(d_aov, 16) || misaligned(d_ws, 16)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: the feature buffer and the workspace must be 16-byte aligned");
    if (misaligned(d_rgb, 4) || misaligned(d_out, 4) || misaligned(d_var, 4)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: float buffers must be 4-byte aligned");
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    return enqueue(W, H, *p, d_rgb, d_aov, d_var, d_out, d_ws, (hipStream_t)stream);
}

hrt_status denoise_host_impl(int device, int32_t W, int32_t H, const hrt_denoise_params* p, const float* rgb, const float* aov,
                             const float* var, float* out) {
    const char* who = "hrt_denoise";
    const hrt_status st = check_film(who, W, H, p);
    if (st != HRT_OK) return st;
    if (!rgb || !aov || !out) return dfail(HRT_ERR_INVALID, std::string(who) + ": NULL argument");
    if (misaligned(rgb, 4) || misaligned(aov, 4) || misaligned(out, 4) || misaligned(var, 4)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: float buffers must be 4-byte aligned");
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    // one allocation: aov | workspace | rgb (filtered in place) | var -- every part a multiple of 4 n bytes, the first two of 16
    const size_t n = (size_t)W * H;
    const size_t o_aov = 0, o_ws = 32 * n, o_rgb = o_ws + 48 * n, o_var = o_rgb + 12 * n, total = o_var + (var ? 4 * n : 0);
    DevMem mem;
    DCHK(hipMalloc(&mem.p, total));
    char* base = (char*)mem.p;
    DCHK(hipMemcpy(base + o_aov, aov, 32 * n, hipMemcpyHostToDevice));
    DCHK(hipMemcpy(base + o_rgb, rgb, 12 * n, hipMemcpyHostToDevice));
    if (var) DCHK(hipMemcpy(base + o_var, var, 4 * n, hipMemcpyHostToDevice));
    const hrt_status se = enqueue(W, H, *p, (const float*)(base + o_rgb), (const float*)(base + o_aov), var ? (const float*)(base + o_var) : nullptr,
                                  (float*)(base + o_rgb), base + o_ws, nullptr);
    if (se != HRT_OK) return se;
    DCHK(hipMemcpy(out, base + o_rgb, 12 * n, hipMemcpyDeviceToHost));      // (the null stream: the copy waits for the kernels)
    return HRT_OK;
}

hrt_status resolve_impl(int device, const float* rgb, int64_t n_pixels, uint8_t* out) {
    const char* who = "hrt_denoise_resolve_u8";
    if (!rgb || !out || n_pixels < 0 || (uint64_t)n_pixels > kMaxPixels) return dfail(HRT_ERR_INVALID, std::string(who) + ": bad argument");
    if (n_pixels == 0) return HRT_OK;
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    const size_t n = (size_t)n_pixels;
    DevMem mem;
    DCHK(hipMalloc(&mem.p, 16 * n));
    float* d_in = (float*)mem.p;
    uint8_t* d_out = (uint8_t*)mem.p + 12 * n;
    DCHK(hipMemcpy(d_in, rgb, 12 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_dn_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d_in, (long long)n_pixels, d_out);
    DLAUNCH("k_dn_resolve");
    DCHK(hipMemcpy(out, d_out, 3 * n, hipMemcpyDeviceToHost));
    return HRT_OK;
}

#define DN_TRY try {
#define DN_CATCH(who) } catch (const std::bad_alloc&) { return dfail(HRT_ERR_OOM, who ": out of host memory"); } \
    catch (const std::exception& e) { return dfail(HRT_ERR_INVALID, std::string(who ": ") + e.what()); } \
    catch (...) { return dfail(HRT_ERR_INVALID, who ": unknown C++ exception"); }

}  // namespace

extern "C" void hrt_denoise_defaults(hrt_denoise_params* p) {
    if (!p) return;
    p->iterations = 5;
    p->normal_squarings = 7;
    p->sigma_l = 2.5f;
    p->sigma_z = 0.5f;
    p->albedo_floor = 0.01f;
}

extern "C" uint64_t hrt_denoise_workspace_bytes(int32_t W, int32_t H) {
    if (W < 1 || H < 1 || (size_t)W * (size_t)H > kMaxPixels) return 0;
    return 48ull * (uint64_t)W * (uint64_t)H;
}

extern "C" hrt_status hrt_denoise_device(int device, int32_t W, int32_t H, const hrt_denoise_params* params, const float* d_rgb,
                                         const float* d_aov, const float* d_var, float* d_out, void* d_workspace, void* stream) {
    DN_TRY
    return denoise_device_impl(device, W, H, params, d_rgb, d_aov, d_var, d_out, d_workspace, stream);
    DN_CATCH("hrt_denoise_device")
}

extern "C" hrt_status hrt_denoise(int device, int32_t W, int32_t H, const hrt_denoise_params* params, const float* rgb, const float* aov,
                                  const float* var, float* out) {
    DN_TRY
    return denoise_host_impl(device, W, H, params, rgb, aov, var, out);
    DN_CATCH("hrt_denoise")
}

extern "C" hrt_status hrt_denoise_resolve_u8(int device, const float* rgb_linear, int64_t n_pixels, uint8_t* out_rgb8) {
    DN_TRY
    return resolve_impl(device, rgb_linear, n_pixels, out_rgb8);
    DN_CATCH("hrt_denoise_resolve_u8")
}
