// hrt_variance.hip -- hrt_variance_* and hrt_adaptive_variance*: the measured variance of include/hrt.h ("measured variance",
// DESIGN.md 4.13), the `var` input of the guided denoiser.
//
// The variance of every pixel's mean luminance from the batch means of a render taken in passes (Chan et al.'s pairwise update of the
// sum of squared deviations, folded in after every pass) or from the buffers of an adaptive render.  The definition -- every operation
// and its order -- is in include/hrt.h; tests/variance_np.py restates those words in numpy float32 and the kernels must give its bits,
// which is why the arithmetic below is plain + - * / and comparisons, written in the header's order, under -ffp-contract=off.
//
//   k_var_fold      thread per pixel: rgb (12 B), state (8 B) -> state (8 B)
//   k_var_finish    thread per pixel: state (8 B) -> var (4 B)
//   k_var_adaptive  thread per pixel: sums (12 B), sq (4 B), count (4 B) -> var (4 B)
//
// Streaming kernels: every byte is touched once, a wave reads whole contiguous runs (768 B of rgb, 512 B of state), there is nothing to
// share between pixels, so no LDS, no atomics, and a handful of registers.  Like the denoiser the unit needs no scene.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/hrt.h"

extern "C" __attribute__((visibility("hidden"))) void hrt_set_last_error(const char* msg);   // hrt_hip.hip

namespace {

__device__ inline float var_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }   // hrt.h: Y
__device__ inline float var_pos(float x) { return x > 0.0f ? x : 0.0f; }                                         // hrt.h: max(0, x); NaN -> 0

__global__ __launch_bounds__(256) void k_var_fold(const float* __restrict__ rgb, float2* __restrict__ state, long long n_pixels,
                                                  float scale, int done, int c) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const float y = var_lum(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]) * scale;
    float2 s;
    s.x = y;
    s.y = 0.0f;
    if (done > 0) {
        const float2 old = state[i];
        const float mb = (y - old.x) / (float)c;
        const float mp = old.x / (float)done;
        const float d = mb - mp;
        const float w = ((float)done * (float)c) / (float)(done + c);
        s.y = old.y + (d * d) * w;
    }
    state[i] = s;
}

__global__ __launch_bounds__(256) void k_var_finish(const float2* __restrict__ state, float* __restrict__ var, long long n_pixels,
                                                    int samples, int batches) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    var[i] = var_pos(state[i].y / (float)(batches - 1)) / (float)samples;
}

__global__ __launch_bounds__(256) void k_var_adaptive(const float* __restrict__ sums, const float* __restrict__ sq,
                                                      const int* __restrict__ count, float* __restrict__ var, long long n_pixels) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const int cnt = count[i];
    float v = 0.0f;
    if (cnt >= 2) {
        const float n = (float)cnt;
        const float m = var_lum(sums[3 * i], sums[3 * i + 1], sums[3 * i + 2]) / n;
        v = var_pos((sq[i] - n * m * m) / (n - 1.0f)) / n;
    }
    var[i] = v;
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
hrt_status vfail(hrt_status st, const std::string& msg) { hrt_set_last_error(msg.c_str()); return st; }
#define VCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return vfail(e_ == hipErrorOutOfMemory ? HRT_ERR_OOM : HRT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define VLAUNCH(name) do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return vfail(HRT_ERR_HIP, std::string(name " launch: ") + hipGetErrorString(e_)); } while (0)

const int64_t kMaxPixels = (int64_t)1 << 30;
bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// everything that can be refused without a device; `who` prefixes the message
hrt_status check_pixels(const std::string& who, int64_t n) {
    if (n < 1) return vfail(HRT_ERR_INVALID, who + ": n_pixels must be >= 1");
    if (n > kMaxPixels) return vfail(HRT_ERR_INVALID, who + ": more than 2^30 pixels");
    return HRT_OK;
}
hrt_status check_fold(const char* who_, int64_t n, const float* rgb, float scale, int32_t done, int32_t c, const float* state) {
    const std::string who(who_);
    if (!rgb || !state) return vfail(HRT_ERR_INVALID, who + ": NULL argument");
    const hrt_status st = check_pixels(who, n);
    if (st != HRT_OK) return st;
    if (done < 0) return vfail(HRT_ERR_INVALID, who + ": samples_before must be >= 0");
    if (c < 1) return vfail(HRT_ERR_INVALID, who + ": samples_batch must be >= 1");
    if ((int64_t)done + (int64_t)c > 0x7fffffffll) return vfail(HRT_ERR_INVALID, who + ": samples_before + samples_batch must be below 2^31");
    if (!(scale > 0.0f && scale <= 3.402823466e38f)) return vfail(HRT_ERR_INVALID, who + ": scale must be finite and positive");
    if (misaligned(rgb, 4) || misaligned(state, 8)) return vfail(HRT_ERR_INVALID, who + ": misaligned pointer: the state must be 8-byte aligned, float buffers 4-byte aligned");
    return HRT_OK;
}
hrt_status check_finish(const char* who_, int64_t n, const float* state, int32_t samples, int32_t batches, const float* var) {
    const std::string who(who_);
    if (!state || !var) return vfail(HRT_ERR_INVALID, who + ": NULL argument");
    const hrt_status st = check_pixels(who, n);
    if (st != HRT_OK) return st;
    if (batches < 2) return vfail(HRT_ERR_INVALID, who + ": batches must be >= 2");
    if (samples < batches) return vfail(HRT_ERR_INVALID, who + ": samples must be >= batches");
    if (misaligned(state, 8) || misaligned(var, 4)) return vfail(HRT_ERR_INVALID, who + ": misaligned pointer: the state must be 8-byte aligned, float buffers 4-byte aligned");
    return HRT_OK;
}
hrt_status check_adaptive(const char* who_, int64_t n, const float* sums, const float* sq, const int32_t* count, const float* var) {
    const std::string who(who_);
    if (!sums || !sq || !count || !var) return vfail(HRT_ERR_INVALID, who + ": NULL argument");
    const hrt_status st = check_pixels(who, n);
    if (st != HRT_OK) return st;
    if (misaligned(sums, 4) || misaligned(sq, 4) || misaligned(count, 4) || misaligned(var, 4)) return vfail(HRT_ERR_INVALID, who + ": misaligned pointer: the buffers must be 4-byte aligned");
    return HRT_OK;
}
hrt_status set_device(const char* who, int device) {
    int n_dev = 0;
    VCHK(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return vfail(HRT_ERR_NO_DEVICE, std::string(who) + ": no such device");
    VCHK(hipSetDevice(device));
    return HRT_OK;
}

// the launches, on the current device
hrt_status enqueue_fold(int64_t n, const float* d_rgb, float scale, int32_t done, int32_t c, float* d_state, hipStream_t stream) {
    hipLaunchKernelGGL(k_var_fold, grid_of(n), dim3(256), 0, stream, d_rgb, (float2*)d_state, (long long)n, scale, (int)done, (int)c);
    VLAUNCH("k_var_fold");
    return HRT_OK;
}
hrt_status enqueue_finish(int64_t n, const float* d_state, int32_t samples, int32_t batches, float* d_var, hipStream_t stream) {
    hipLaunchKernelGGL(k_var_finish, grid_of(n), dim3(256), 0, stream, (const float2*)d_state, d_var, (long long)n, (int)samples, (int)batches);
    VLAUNCH("k_var_finish");
    return HRT_OK;
}
hrt_status enqueue_adaptive(int64_t n, const float* d_sums, const float* d_sq, const int32_t* d_count, float* d_var, hipStream_t stream) {
    hipLaunchKernelGGL(k_var_adaptive, grid_of(n), dim3(256), 0, stream, d_sums, d_sq, (const int*)d_count, d_var, (long long)n);
    VLAUNCH("k_var_adaptive");
    return HRT_OK;
}

hrt_status fold_host_impl(int device, int64_t n_pixels, const float* rgb, float scale, int32_t done, int32_t c, float* state) {
    const char* who = "hrt_variance_fold";
    const hrt_status st = check_fold(who, n_pixels, rgb, scale, done, c, state);
    if (st != HRT_OK) return st;
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    const size_t n = (size_t)n_pixels;       // one allocation: state | rgb
    DevMem mem;
    VCHK(hipMalloc(&mem.p, 20 * n));
    char* base = (char*)mem.p;
    VCHK(hipMemcpy(base + 8 * n, rgb, 12 * n, hipMemcpyHostToDevice));
    if (done > 0) VCHK(hipMemcpy(base, state, 8 * n, hipMemcpyHostToDevice));
    const hrt_status se = enqueue_fold(n_pixels, (const float*)(base + 8 * n), scale, done, c, (float*)base, nullptr);
    if (se != HRT_OK) return se;
    VCHK(hipMemcpy(state, base, 8 * n, hipMemcpyDeviceToHost));      // (the null stream: the copy waits for the kernel)
    return HRT_OK;
}

hrt_status finish_host_impl(int device, int64_t n_pixels, const float* state, int32_t samples, int32_t batches, float* var) {
    const char* who = "hrt_variance_finish";
    const hrt_status st = check_finish(who, n_pixels, state, samples, batches, var);
    if (st != HRT_OK) return st;
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    const size_t n = (size_t)n_pixels;       // state | var
    DevMem mem;
    VCHK(hipMalloc(&mem.p, 12 * n));
    char* base = (char*)mem.p;
    VCHK(hipMemcpy(base, state, 8 * n, hipMemcpyHostToDevice));
    const hrt_status se = enqueue_finish(n_pixels, (const float*)base, samples, batches, (float*)(base + 8 * n), nullptr);
    if (se != HRT_OK) return se;
    VCHK(hipMemcpy(var, base + 8 * n, 4 * n, hipMemcpyDeviceToHost));
    return HRT_OK;
}

hrt_status adaptive_host_impl(int device, int64_t n_pixels, const float* sums, const float* sq, const int32_t* count, float* var) {
    const char* who = "hrt_adaptive_variance";
    const hrt_status st = check_adaptive(who, n_pixels, sums, sq, count, var);
    if (st != HRT_OK) return st;
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    const size_t n = (size_t)n_pixels;       // sums | sq | count | var
    DevMem mem;
    VCHK(hipMalloc(&mem.p, 24 * n));
    char* base = (char*)mem.p;
    VCHK(hipMemcpy(base, sums, 12 * n, hipMemcpyHostToDevice));
    VCHK(hipMemcpy(base + 12 * n, sq, 4 * n, hipMemcpyHostToDevice));
    VCHK(hipMemcpy(base + 16 * n, count, 4 * n, hipMemcpyHostToDevice));
    const hrt_status se = enqueue_adaptive(n_pixels, (const float*)base, (const float*)(base + 12 * n), (const int32_t*)(base + 16 * n),
                                           (float*)(base + 20 * n), nullptr);
    if (se != HRT_OK) return se;
    VCHK(hipMemcpy(var, base + 20 * n, 4 * n, hipMemcpyDeviceToHost));
    return HRT_OK;
}

#define VAR_TRY try {
#define VAR_CATCH(who) } catch (const std::bad_alloc&) { return vfail(HRT_ERR_OOM, who ": out of host memory"); } \
    catch (const std::exception& e) { return vfail(HRT_ERR_INVALID, std::string(who ": ") + e.what()); } \
    catch (...) { return vfail(HRT_ERR_INVALID, who ": unknown C++ exception"); }

}  // namespace

extern "C" uint64_t hrt_variance_state_bytes(int64_t n_pixels) {
    if (n_pixels < 1 || n_pixels > kMaxPixels) return 0;
    return 8ull * (uint64_t)n_pixels;
}

extern "C" hrt_status hrt_variance_fold_device(int device, int64_t n_pixels, const float* d_rgb, float scale, int32_t samples_before,
                                               int32_t samples_batch, float* d_state, void* stream) {
    VAR_TRY
    const char* who = "hrt_variance_fold_device";
    const hrt_status st = check_fold(who, n_pixels, d_rgb, scale, samples_before, samples_batch, d_state);
    if (st != HRT_OK) return st;
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    return enqueue_fold(n_pixels, d_rgb, scale, samples_before, samples_batch, d_state, (hipStream_t)stream);
    VAR_CATCH("hrt_variance_fold_device")
}

extern "C" hrt_status hrt_variance_finish_device(int device, int64_t n_pixels, const float* d_state, int32_t samples, int32_t batches,
                                                 float* d_var, void* stream) {
    VAR_TRY
    const char* who = "hrt_variance_finish_device";
    const hrt_status st = check_finish(who, n_pixels, d_state, samples, batches, d_var);
    if (st != HRT_OK) return st;
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    return enqueue_finish(n_pixels, d_state, samples, batches, d_var, (hipStream_t)stream);
    VAR_CATCH("hrt_variance_finish_device")
}

extern "C" hrt_status hrt_adaptive_variance_device(int device, int64_t n_pixels, const float* d_sums, const float* d_sq,
                                                   const int32_t* d_count, float* d_var, void* stream) {
    VAR_TRY
    const char* who = "hrt_adaptive_variance_device";
    const hrt_status st = check_adaptive(who, n_pixels, d_sums, d_sq, d_count, d_var);
    if (st != HRT_OK) return st;
    DeviceGuard guard;
    const hrt_status sd = set_device(who, device);
    if (sd != HRT_OK) return sd;
    return enqueue_adaptive(n_pixels, d_sums, d_sq, d_count, d_var, (hipStream_t)stream);
    VAR_CATCH("hrt_adaptive_variance_device")
}

extern "C" hrt_status hrt_variance_fold(int device, int64_t n_pixels, const float* rgb, float scale, int32_t samples_before,
                                        int32_t samples_batch, float* state) {
    VAR_TRY
    return fold_host_impl(device, n_pixels, rgb, scale, samples_before, samples_batch, state);
    VAR_CATCH("hrt_variance_fold")
}

extern "C" hrt_status hrt_variance_finish(int device, int64_t n_pixels, const float* state, int32_t samples, int32_t batches, float* var) {
    VAR_TRY
    return finish_host_impl(device, n_pixels, state, samples, batches, var);
    VAR_CATCH("hrt_variance_finish")
}

extern "C" hrt_status hrt_adaptive_variance(int device, int64_t n_pixels, const float* sums, const float* sq, const int32_t* count,
                                            float* var) {
    VAR_TRY
    return adaptive_host_impl(device, n_pixels, sums, sq, count, var);
    VAR_CATCH("hrt_adaptive_variance")
}
