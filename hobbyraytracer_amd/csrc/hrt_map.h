// hrt_map.h -- which pixel of the film a render call's local pixel is: the kernel argument RenderMap and slot_pixel, shared by
// hrt_hip.hip (which builds the maps: rect_map, stripe_map, list_map) and hrt_aov_ids.hip.
//
// The unnamed namespace is deliberate: RenderMap is a parameter type of the kernels of hrt_hip.hip, which stand in that unit's own
// unnamed namespace, and their names -- what hipcc's resource report and the tests that read it go by -- must stay what they were
// when the struct was defined there.  Each unit that includes this header gets its own, identical, copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

struct RenderMap {
    int32_t mode;            // 0 = rect tile, 1 = interleaved row blocks, 2 = list of row-block pixels (adaptive passes)
    int32_t x0, y0;          // rect origin
    int32_t rw, rh;          // local region size
    int32_t R, rank, G;      // stripes
    int32_t tiles_x;         // ceil(rw / 8)
    int32_t total_items;     // tiles_x * ceil(rh / 8) * 64
    // exact division of 32-bit numbers by rw and by rw*rh as multiply-high + shift (host-computed magic
    // numbers, fastdiv below): the wavefront kernels turn slot ids into (sample, pixel) for every path
    uint64_t m_rw, m_nl;
    // mode 2: local pixel lp of the batch is pixel pix[lp] of the row-block layout (an index in [0, rw * rh), the stripe
    // order of mode 1); n_list entries, every one of them at the same sample count
    const int32_t* pix;
    uint32_t n_list;
};
// pixels one render call of `map` covers
inline uint32_t map_pixels(const RenderMap& map) { return map.mode == 2 ? map.n_list : (uint32_t)map.rw * (uint32_t)map.rh; }

// floor(x / d) for any 32-bit x: with m = floor(2^64 / d) + 1 the product's high half is exact for every
// x < 2^32 (the error term x / 2^64 * d stays below 1 / d).  d = 1 needs no magic.
__host__ __device__ inline uint32_t fastdiv(uint32_t x, uint32_t d, uint64_t m) {
    if (d == 1) return x;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__umul64hi(m, (uint64_t)x);
#else
    return (uint32_t)(((unsigned __int128)m * x) >> 64);
#endif
}
inline uint64_t fastdiv_magic(uint32_t d) { return d <= 1 ? 0 : (uint64_t)(~0ull / d) + 1; }

__device__ inline void slot_pixel(const RenderMap& map, unsigned lp, int& px, int& py) {
    if (map.mode == 2) lp = (unsigned)map.pix[lp];   // (uniform branch) the list holds indices of the mode-1 layout
    const int ly = (int)fastdiv(lp, (unsigned)map.rw, map.m_rw);
    const int lx = (int)(lp - (unsigned)ly * (unsigned)map.rw);
    if (map.mode == 0) { px = map.x0 + lx; py = map.y0 + ly; }
    else { const int b = ly / map.R; px = lx; py = (b * map.G + map.rank) * map.R + (ly - b * map.R); }
}

}  // namespace
