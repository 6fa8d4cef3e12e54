// hrt_despeckle.hip -- hrt_despeckle*: the energy-preserving outlier filter of include/hrt.h ("despeckle").
//
// A pixel whose luminance is more than `ratio` times the rank-th largest luminance of its small window is an outlier (a "firefly").
// It is brought down to that yardstick and what it held above it is dealt out in equal shares over the valid pixels of its own
// window, itself included, so the film's sum stays what it was; a pixel with a non-finite channel becomes the mean of its valid
// neighbours.  The definition -- every operation and its order -- is in include/hrt.h; tests/despeckle_np.py restates those words
// in numpy float32 and the kernels must give its bits, which is why the arithmetic below is plain + - * /, sqrtf and comparisons,
// written in the header's order, under -ffp-contract=off.
//
//   k_ds_luma     thread per pixel: rgb -> L, the luminance; an invalid pixel gets a NaN
//   k_ds_detect   thread per pixel: L (a 16 x 16 tile and its halo, staged in LDS), rgb, var -> D = (share.rgb, s or a marker)
//   k_ds_apply    thread per pixel: rgb, D over the window -> out and the optional map
//
// The workspace is D (one float4 per pixel) followed by L (one float per pixel): 20 bytes per pixel.  A valid pixel's luminance is
// finite by definition, so a NaN in L marks a pixel that no window may count, and the cells of the LDS tile that lie outside the
// film hold the same NaN: there is no separate mask and no bounds test in the window loop of k_ds_detect.  D.w is s = ref / l for
// an outlier (0 <= s < 1), kDsPlain for any other valid pixel and kDsInvalid for an invalid one.  Every pixel is written by its own
// thread only -- the shares are gathered, not scattered -- so there are no atomics and the result does not depend on scheduling.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/hrt.h"

extern "C" __attribute__((visibility("hidden"))) void hrt_set_last_error(const char* msg);   // hrt_hip.hip

namespace {

#define HRT_DS_TILE 16
#define HRT_DS_HALO 2                               // the largest radius
#define HRT_DS_LDS (HRT_DS_TILE + 2 * HRT_DS_HALO)  // 20: the staged tile is 20 x 20 floats, 1600 bytes
#define HRT_DS_WAVES 4                              // __launch_bounds__(256, 4): at least 4 waves per SIMD

constexpr float kDsPlain = 2.0f;                    // D.w of a valid pixel that is no outlier
constexpr float kDsInvalid = -1.0f;                 // D.w of an invalid pixel

__device__ inline float ds_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ inline bool ds_finite(float x) { return fabsf(x) <= 3.402823466e38f; }
__device__ inline float ds_pos(float x) { return x > 0.0f ? x : 0.0f; }                       // hrt.h: max(0, x); NaN -> 0

__global__ __launch_bounds__(256, HRT_DS_WAVES) void k_ds_luma(const float* __restrict__ rgb, float* __restrict__ L, int W, int H) {
    const int x = blockIdx.x * HRT_DS_TILE + threadIdx.x, y = blockIdx.y * HRT_DS_TILE + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    const float l = ds_lum(r, g, b);
    const bool valid = ds_finite(r) && ds_finite(g) && ds_finite(b) && ds_finite(l);
    L[i] = valid ? l : __builtin_nanf("");
}

__global__ __launch_bounds__(256, HRT_DS_WAVES) void k_ds_detect(const float* __restrict__ rgb, const float* __restrict__ L,
                                                                  const float* __restrict__ var, float4* __restrict__ D, int W, int H,
                                                                  int radius, int rank, float ratio, float gate_z) {
    __shared__ float tile[HRT_DS_LDS * HRT_DS_LDS];
    const int x0 = blockIdx.x * HRT_DS_TILE - HRT_DS_HALO, y0 = blockIdx.y * HRT_DS_TILE - HRT_DS_HALO;
    // the cells within `radius` of the block's 16 x 16 pixels; the others, and those outside the film, are never counted
    const int lo = HRT_DS_HALO - radius, hi = HRT_DS_HALO + HRT_DS_TILE + radius;
    for (int c = threadIdx.y * HRT_DS_TILE + threadIdx.x; c < HRT_DS_LDS * HRT_DS_LDS; c += HRT_DS_TILE * HRT_DS_TILE) {
        const int cx = c % HRT_DS_LDS, cy = c / HRT_DS_LDS;
        const int gx = x0 + cx, gy = y0 + cy;
        float v = __builtin_nanf("");
        if (cx >= lo && cx < hi && cy >= lo && cy < hi && gx >= 0 && gx < W && gy >= 0 && gy < H) v = L[(size_t)gy * W + gx];
        tile[c] = v;
    }
    __syncthreads();
    const int x = blockIdx.x * HRT_DS_TILE + threadIdx.x, y = blockIdx.y * HRT_DS_TILE + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const int cx = threadIdx.x + HRT_DS_HALO, cy = threadIdx.y + HRT_DS_HALO;
    const float l = tile[cy * HRT_DS_LDS + cx];
    float4 d;
    d.x = 0.0f; d.y = 0.0f; d.z = 0.0f; d.w = kDsPlain;
    if (!ds_finite(l)) { d.w = kDsInvalid; D[i] = d; return; }

    // the four largest luminances of the valid neighbours, t0 >= t1 >= t2 >= t3, and how many valid neighbours there are
    float t0 = -__builtin_huge_valf(), t1 = t0, t2 = t0, t3 = t0;
    int others = 0;
    for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
            if (dx == 0 && dy == 0) continue;
            float v = tile[(cy + dy) * HRT_DS_LDS + cx + dx];
            if (!ds_finite(v)) continue;
            ++others;
            float u;
            if (v > t0) { u = t0; t0 = v; v = u; }
            if (v > t1) { u = t1; t1 = v; v = u; }
            if (v > t2) { u = t2; t2 = v; v = u; }
            if (v > t3) t3 = v;
        }
    const float ref = rank == 1 ? t0 : rank == 2 ? t1 : rank == 3 ? t2 : t3;
    bool outlier = others >= rank && l > 0.0f && ref >= 0.0f && l > ratio * ref;
    if (outlier && var && gate_z > 0.0f) outlier = gate_z * sqrtf(ds_pos(var[i])) >= l - ref;
    if (outlier) {
        const float s = ref / l;
        const float n = (float)(others + 1);
        const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        d.x = (r - r * s) / n; d.y = (g - g * s) / n; d.z = (b - b * s) / n;
        d.w = s;
    }
    D[i] = d;
}

// out must not be rgb: a repaired pixel reads its neighbours' input values
__global__ __launch_bounds__(256, HRT_DS_WAVES) void k_ds_apply(const float* __restrict__ rgb, const float4* __restrict__ D,
                                                                 float* __restrict__ out, float* __restrict__ map, int W, int H,
                                                                 int radius, int repair_invalid) {
    const int x = blockIdx.x * HRT_DS_TILE + threadIdx.x, y = blockIdx.y * HRT_DS_TILE + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const float4 dp = D[i];
    float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    float m = 0.0f;
    const int ya = y - radius < 0 ? 0 : y - radius, yb = y + radius >= H ? H - 1 : y + radius;
    const int xa = x - radius < 0 ? 0 : x - radius, xb = x + radius >= W ? W - 1 : x + radius;
    if (dp.w != kDsInvalid) {
        if (dp.w != kDsPlain) { r = r * dp.w; g = g * dp.w; b = b * dp.w; m = 1.0f - dp.w; }
        for (int qy = ya; qy <= yb; ++qy)
            for (int qx = xa; qx <= xb; ++qx) {
                const float4 dq = D[(size_t)qy * W + qx];
                if (dq.w == kDsInvalid) continue;
                r = r + dq.x; g = g + dq.y; b = b + dq.z;
            }
    } else if (repair_invalid) {
        float sr = 0.0f, sg = 0.0f, sb = 0.0f;
        int count = 0;
        for (int qy = ya; qy <= yb; ++qy)
            for (int qx = xa; qx <= xb; ++qx) {
                const size_t q = (size_t)qy * W + qx;
                if (D[q].w == kDsInvalid) continue;
                sr = sr + rgb[3 * q]; sg = sg + rgb[3 * q + 1]; sb = sb + rgb[3 * q + 2];
                ++count;
            }
        if (count > 0) { const float n = (float)count; r = sr / n; g = sg / n; b = sb / n; m = -1.0f; }
    }
    out[3 * i] = r; out[3 * i + 1] = g; out[3 * i + 2] = b;
    if (map) map[i] = m;
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

// everything that can be refused without a device; `who` prefixes the message
hrt_status check_film(const char* who, int32_t W, int32_t H, const hrt_despeckle_params* p) {
    const std::string w(who);
    if (!p) return dfail(HRT_ERR_INVALID, w + ": NULL argument");
    if (W < 1 || H < 1) return dfail(HRT_ERR_INVALID, w + ": width and height must be >= 1");
    if ((size_t)W * (size_t)H > kMaxPixels) return dfail(HRT_ERR_INVALID, w + ": more than 2^30 pixels");
    if (p->radius < 1 || p->radius > HRT_DS_HALO) return dfail(HRT_ERR_INVALID, w + ": radius must be 1 or 2");
    if (p->rank < 1 || p->rank > 4) return dfail(HRT_ERR_INVALID, w + ": rank must be 1..4");
    if (!finite(p->ratio) || !(p->ratio > 1.0f)) return dfail(HRT_ERR_INVALID, w + ": ratio must be finite and above 1");
    if (!finite(p->gate_z) || !(p->gate_z >= 0.0f)) return dfail(HRT_ERR_INVALID, w + ": gate_z must be finite and not negative");
    if (p->repair_invalid != 0 && p->repair_invalid != 1) return dfail(HRT_ERR_INVALID, w + ": repair_invalid must be 0 or 1");
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
hrt_status enqueue(int32_t W, int32_t H, const hrt_despeckle_params& p, const float* d_rgb, const float* d_var, float* d_out, float* d_map,
                   void* d_ws, hipStream_t stream) {
    const size_t n = (size_t)W * H;
    float4* D = (float4*)d_ws;
    float* L = (float*)(D + n);
    const dim3 block(HRT_DS_TILE, HRT_DS_TILE), grid((W + HRT_DS_TILE - 1) / HRT_DS_TILE, (H + HRT_DS_TILE - 1) / HRT_DS_TILE);
    hipLaunchKernelGGL(k_ds_luma, grid, block, 0, stream, d_rgb, L, W, H);
    DLAUNCH("k_ds_luma");
    hipLaunchKernelGGL(k_ds_detect, grid, block, 0, stream, d_rgb, (const float*)L, d_var, D, W, H, p.radius, p.rank, p.ratio, p.gate_z);
    DLAUNCH("k_ds_detect");
    hipLaunchKernelGGL(k_ds_apply, grid, block, 0, stream, d_rgb, (const float4*)D, d_out, d_map, W, H, p.radius, p.repair_invalid);
    DLAUNCH("k_ds_apply");
    return HRT_OK;
}

hrt_status despeckle_device_impl(int device, int32_t W, int32_t H, const hrt_despeckle_params* p, const float* d_rgb, const float* d_var,
                                 float* d_out, float* d_map, void* d_ws, void* stream) {
    const char* who = "hrt_despeckle_device";
    const hrt_status st = check_film(who, W, H, p);
    if (st != HRT_OK) return st;
    if (!d_rgb || !d_out || !d_ws) return dfail(HRT_ERR_INVALID, std::string(who) + ": NULL argument");
    if (d_out == d_rgb) return dfail(HRT_ERR_INVALID, std::string(who) + ": the output must not be the input (out == rgb)");
    if (misaligned(d_ws, 16)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: the workspace must be 16-byte aligned");
    if (misaligned(d_rgb, 4) || misaligned(d_out, 4) || misaligned(d_var, 4) || misaligned(d_map, 4)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: float buffers must be 4-byte aligned");
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    return enqueue(W, H, *p, d_rgb, d_var, d_out, d_map, d_ws, (hipStream_t)stream);
}

hrt_status despeckle_host_impl(int device, int32_t W, int32_t H, const hrt_despeckle_params* p, const float* rgb, const float* var,
                               float* out, float* map) {
    const char* who = "hrt_despeckle";
    const hrt_status st = check_film(who, W, H, p);
    if (st != HRT_OK) return st;
    if (!rgb || !out) return dfail(HRT_ERR_INVALID, std::string(who) + ": NULL argument");
    if (out == rgb) return dfail(HRT_ERR_INVALID, std::string(who) + ": the output must not be the input (out == rgb)");
    if (misaligned(rgb, 4) || misaligned(out, 4) || misaligned(var, 4) || misaligned(map, 4)) return dfail(HRT_ERR_INVALID, std::string(who) + ": misaligned pointer: float buffers must be 4-byte aligned");
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    // one allocation: workspace | rgb | out | var | map -- every part a multiple of 4 n bytes, the first of 16
    const size_t n = (size_t)W * H;
    const size_t o_ws = 0, o_rgb = 20 * n, o_out = o_rgb + 12 * n, o_var = o_out + 12 * n, o_map = o_var + (var ? 4 * n : 0), total = o_map + (map ? 4 * n : 0);
    DevMem mem;
    DCHK(hipMalloc(&mem.p, total));
    char* base = (char*)mem.p;
    DCHK(hipMemcpy(base + o_rgb, rgb, 12 * n, hipMemcpyHostToDevice));
    if (var) DCHK(hipMemcpy(base + o_var, var, 4 * n, hipMemcpyHostToDevice));
    const hrt_status se = enqueue(W, H, *p, (const float*)(base + o_rgb), var ? (const float*)(base + o_var) : nullptr, (float*)(base + o_out),
                                  map ? (float*)(base + o_map) : nullptr, base + o_ws, nullptr);
    if (se != HRT_OK) return se;
    DCHK(hipMemcpy(out, base + o_out, 12 * n, hipMemcpyDeviceToHost));      // (the null stream: the copy waits for the kernels)
    if (map) DCHK(hipMemcpy(map, base + o_map, 4 * n, hipMemcpyDeviceToHost));
    return HRT_OK;
}

#define DS_TRY try {
#define DS_CATCH(who) } catch (const std::bad_alloc&) { return dfail(HRT_ERR_OOM, who ": out of host memory"); } \
    catch (const std::exception& e) { return dfail(HRT_ERR_INVALID, std::string(who ": ") + e.what()); } \
    catch (...) { return dfail(HRT_ERR_INVALID, who ": unknown C++ exception"); }

}  // namespace

extern "C" void hrt_despeckle_defaults(hrt_despeckle_params* p) {
    if (!p) return;
    p->radius = 1;
    p->rank = 2;
    p->ratio = 2.0f;
    p->gate_z = 2.0f;
    p->repair_invalid = 1;
}

extern "C" uint64_t hrt_despeckle_workspace_bytes(int32_t W, int32_t H) {
    if (W < 1 || H < 1 || (size_t)W * (size_t)H > kMaxPixels) return 0;
    return 20ull * (uint64_t)W * (uint64_t)H;
}

extern "C" hrt_status hrt_despeckle_device(int device, int32_t W, int32_t H, const hrt_despeckle_params* params, const float* d_rgb,
                                           const float* d_var, float* d_out, float* d_map, void* d_workspace, void* stream) {
    DS_TRY
    return despeckle_device_impl(device, W, H, params, d_rgb, d_var, d_out, d_map, d_workspace, stream);
    DS_CATCH("hrt_despeckle_device")
}

extern "C" hrt_status hrt_despeckle(int device, int32_t W, int32_t H, const hrt_despeckle_params* params, const float* rgb, const float* var,
                                    float* out, float* map) {
    DS_TRY
    return despeckle_host_impl(device, W, H, params, rgb, var, out, map);
    DS_CATCH("hrt_despeckle")
}
