// render.h — the seam of the reference (main.cpp:81-82): same call shape, the
// body is the MI355X path (flatten -> libhrt_hip.so) instead of the PSTL loop.
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "classes.h"

namespace hrthost {

struct RenderOptions {
    int gpus = 1;                       // image row blocks are interleaved over this many devices
    int rows_per_block = 8;
    bool thin_lens = false;             // sample the lens as camera.h:34's commented-out circularRand(lensRadius) would (--lens)
    bool nee = false;                   // next-event estimation with MIS for the rect and sphere lights (--nee, hrt.h HRT_FLAG_NEE)
    bool nee_env = false;               // ... and environment-map importance sampling (--nee-env, HRT_FLAG_NEE_ENV; needs nee)
    bool nee_emitters = false;          // ... over the emitter table (--nee-emitters, HRT_FLAG_NEE_EMITTERS; needs nee)
    bool stratified = false;            // the stratified sampler (--stratified, HRT_FLAG_STRATIFIED)
    bool nee_lobes = false;             // ... at rough metal and medium vertices too (--nee-lobes, HRT_FLAG_NEE_LOBES; needs nee)
    bool roulette = false;              // Russian roulette (--roulette, HRT_FLAG_ROULETTE) ...
    int roulette_start = 3;             // ... from a path's N-th scatter on (--roulette-start N)
    float roulette_floor = 0.05f;       // ... with no survival probability below Q (--roulette-floor Q)
    int filter_kind = -1;               // the film's reconstruction filter (--filter, HRT_FLAG_FILTER): HRT_FILTER_*, -1 = the box filter ...
    float filter_radius = 0.0f;         // ... at this radius in pixels (--filter-radius; <= 0: the kind's default).  One device, no adaptive passes
    double* filter_seconds = nullptr;   // ... (optional) gets the time of the filter's own kernels, from HIP events
    bool force_rccl = false;            // gather through an RCCL communicator even with one device (--rccl; tests)
    uint32_t quirks = HRT_QUIRKS_REFERENCE;
    uint64_t seed = 0;
    int max_depth = 50;                 // MAX_DEPTH (main.cpp:32)
    bool stats = false;                 // count box / triangle tests too
    bool progress = true;               // the reporter thread of main.cpp:97-109: "Pixels rendered: x/N" every 500 ms (--no-progress)
    int progress_interval_ms = 500;     // main.cpp:107
    // Progressive rendering: samples are taken in passes of `pass_samples` (0 = all at once);
    // after every pass but the last the film holds the preview (mean of the samples so far) and `on_pass`
    // is called (the CLI rewrites the output image there).  With `checkpoint` set, the accumulation sums and
    // the next sample index are stored after every pass; `resume` continues a render from such a file (any
    // GPU count: the file holds whole-film rows).  The finished film is bit-identical however it was batched.
    int pass_samples = 0;
    int max_passes = 0;                 // > 0: stop after this many passes (the checkpoint continues the render later)
    std::string checkpoint;
    bool resume = false;
    std::function<void(int samples_done)> on_pass;
    // Adaptive sampling (hrt.h hrt_render_stripes_adaptive): adaptive >= 0 is the stopping threshold (the relative standard
    // error of a pixel's mean luminance); every pixel takes min_samples, then passes of pass_samples (16 when 0) go to the
    // pixels still above it.  One GPU, no checkpoints.  The film gets sums / count; sample_counts (optional) the counts.
    float adaptive = -1.0f;
    int min_samples = 16;
    float adaptive_floor = 0.01f;       // luminance floor of the relative error's denominator (dark pixels)
    std::vector<int32_t>* sample_counts = nullptr;
    // Feature buffers (--aov, hrt.h hrt_render_aov_tile): aov_samples > 0 runs the pass over samples [0, aov_samples)
    // of every pixel on the first device, whatever `gpus` is, before the film's render and independent of it (of the estimator, the
    // batching, a resume, adaptive sampling); *aov_out gets width * height * 8 floats in film order, *aov_seconds (optional) the
    // wall time of the pass, the upload and release of its own copy of the scene included.  Checkpoints do not hold them.
    int aov_samples = 0;
    std::vector<float>* aov_out = nullptr;
    double* aov_seconds = nullptr;
    // Id mattes and position (--aov-ids, hrt.h hrt_render_aov_ids_tile): with aov_ids_out set (and aov_samples > 0) the
    // feature-buffer pass is followed, on its own temporary scene, by the id pass over the same samples; *aov_ids_out gets width *
    // height * 80 bytes in film order, *aov_ids_seconds (optional) the wall time of that call alone.  *aov_ids_manifest (optional) gets
    // the text of PREFIX.ids.txt: one line per object id (primitive kind, material id) and one per material id (kind, and the name
    // `material_names` has for it, when it has one).  Ids of 2^24 or more would not survive the float of the PFM files: refused.
    std::vector<uint8_t>* aov_ids_out = nullptr;
    double* aov_ids_seconds = nullptr;
    std::string* aov_ids_manifest = nullptr;
    const std::map<std::string, std::shared_ptr<Material>>* material_names = nullptr;
    // Measured variance (--denoise-variance measured, hrt.h hrt_variance_*): with variance_out set the render measures
    // the variance of every pixel's mean luminance -- an adaptive render from its own buffers (hrt_adaptive_variance), any other from
    // the batch means of its passes: the passes of pass_samples or, without them, variance_batches passes (range j starts at
    // j * ceil(samples / variance_batches)) taken for this purpose only, without previews; resumed sums count as the first batch.  The
    // gathered whole-film sums are folded on the first device after every pass, whatever `gpus` is; the film's bits do not depend on
    // any of it.  *variance_out gets width * height floats in film order, or stays empty when fewer than two batches existed;
    // *variance_seconds (optional) the wall time of the folds, copies included.  Checkpoints do not hold the state.
    int variance_batches = 0;
    std::vector<float>* variance_out = nullptr;
    double* variance_seconds = nullptr;
};

// render() of main.cpp:81-140.  nThreads is accepted and unused, exactly as in
// the reference (main.cpp:81 never reads it).  Returns HRT_OK or the failing
// status (message on stderr); fills film->getPixels() and film->linear().
hrt_status render(int nThreads, const std::shared_ptr<Texture> background, const std::shared_ptr<Hittable> world,
                  const Camera& camera, std::shared_ptr<Film>& film, const RenderOptions& opt, hrt_stats* stats,
                  double* render_seconds);

}  // namespace hrthost
