// main.cpp — the CLI, drop-in for the reference's executable (main.cpp:142-195):
//     hobbyraytracer [scene.yaml]
// Default scene "teapot_scene.yaml" in the cwd, same console lines, same exit
// code convention (Q-12: the process returns Film::outputFilm()'s int, 1 on
// success; -1 when the scene fails to load).  Additive flags:
//     --gpus N   --seed S   --spp N   --size WxH   --quirks reference|fixed
//     --assets DIR (search dir for meshes / textures)   --stats   --out FILE
//     --make-assets DIR (write the procedural teapot.obj / marble_bust_01.obj / old_hall_4k.hdr and exit)
//     --progressive N (take the samples in passes of N and rewrite the output image after every pass)
//     --checkpoint FILE (store the accumulation buffer after every pass)   --resume (continue from that file)
//     --max-passes K (stop after K passes; with --checkpoint the render can be resumed later)
//     --dump-linear FILE.pfm (the fp32 linear film, bit for bit, next to the tonemapped image)
//     --obj-indices reference|rebased (multi-object OBJ files: the reference's un-rebased face indices, mesh.cpp:111-114, or correct ones)
//     --lens (thin-lens sampling with the scene's `aperture`: camera.h:34's commented-out circularRand(lensRadius); off = the reference)
//     --nee (next-event estimation with MIS for the scene's rect and sphere lights; off = the reference's estimator)
//     --nee-env (--nee and environment-map importance sampling; implies --nee)
//     --nee-emitters (--nee over every rect, box and mesh emitter, wrapped or not; implies --nee)
//     --nee-lobes (--nee at rough metal and medium vertices too; implies --nee)
//     --stratified (the samples of a pixel from Owen-scrambled (0,2)-sequences instead of independent numbers; combines
//         with every flag above and below.  With --adaptive the samples of a pixel are negatively correlated, so the estimated standard
//         error over-states the real one: a pixel stops no earlier than it should, and may take more samples than it needs)
//     --roulette (Russian roulette, DESIGN.md 4.10: from a path's third scatter on it survives with probability q = max(0.05, min(1, its
//         largest attenuation component)) and survivors are re-weighted by 1 / q; unbiased, fewer segments, slightly more noise per sample;
//         combines with the --nee flags and --stratified; with it --stats prints its line without box_tests / tri_tests)
//     --roulette-start N (the scatter from which roulette is played, 3; implies --roulette)
//     --roulette-floor Q (the smallest survival probability, in (0, 1], 0.05; implies --roulette)
//     --no-progress (no reporter thread and no progress counter on the device: main.cpp:97-109), --progress-ms N (its interval, 500)
//     --rccl (gather the film through an RCCL communicator even on one GPU; with --gpus N > 1 it always is)
//     --adaptive T (adaptive sampling: a pixel stops once the relative standard error of its mean luminance is below T;
//         one GPU, no --checkpoint / --resume)   --min-samples N (what every pixel takes first, 16)   --progressive N (the
//         samples a pass adds to the pixels still active, 16)   --adaptive-floor F (luminance floor of the relative error, 0.01)
//     --sample-map FILE.pfm (with --adaptive: the samples each pixel took, as floats in all three channels)
//     --aov PREFIX (feature buffers, DESIGN.md 4.11: PREFIX.albedo.pfm, PREFIX.normal.pfm, PREFIX.depth.pfm and PREFIX.alpha.pfm, the
//         first-hit albedo, normal, depth and coverage of the film's camera rays, for a denoiser or a compositor; depth and alpha in all
//         three channels.  First device only; depends on --lens, --stratified, --quirks, --seed and --size, on nothing else)
//     --aov-spp N (the samples per pixel of that pass, samples 0 .. N - 1; min(spp, 16) by default; 1 <= N <= spp; needs --aov or --denoise)
//     --aov-ids (needs --aov PREFIX; id mattes and position, DESIGN.md 4.14, over the samples of the --aov pass: PREFIX.position.pfm;
//         PREFIX.object0.pfm .. PREFIX.object3.pfm and PREFIX.material0.pfm .. PREFIX.material3.pfm, the four largest shares of each pixel
//         with R = the id as a float (-1: no hit; -2147483648: rank unused), G = its coverage, B = 0; PREFIX.ids.txt, what the ids stand for)
//     --matte object:ID[,ID...] FILE.pfm | --matte material:ID[,ID...] FILE.pfm (the summed coverage of those ids, in all three channels;
//         may be repeated; implies --aov-ids)
//     --denoise (the guided denoiser, DESIGN.md 4.12: runs the feature-buffer pass as --aov would -- its files only with --aov PREFIX --
//         and filters the finished film on the first device with hrt_denoise, spatial variance estimate; the image file and
//         --dump-linear then hold the filtered film.  Previews and checkpoints stay unfiltered)
//     --denoise-iterations N (1 .. 8)   --denoise-sigma-l X   --denoise-sigma-z X (finite, > 0; each implies --denoise)
//     --dump-noisy FILE.pfm (with --denoise or --despeckle: the unfiltered linear film)
//     --denoise-variance spatial|measured (implies --denoise; DESIGN.md 4.13.  spatial, the default: the filter estimates the variance
//         from a 7 x 7 window.  measured: it is given the variance of every pixel's mean luminance -- with --adaptive from the adaptive
//         render's buffers, otherwise from the batch means of the render's passes: the passes of --progressive N or, without it,
//         --denoise-batches K passes (--max-passes counts them).  The film is the same bits however it is batched.  After --resume the
//         resumed sums are the first batch; with fewer than two batches (--spp 1, nothing left to render) the filter falls back to the
//         spatial estimate and says so.  Without --denoise-sigma-l the filter then takes sigma_l = 6 instead of 2.5.  With --stratified
//         the batches are not independent and the measured variance is too large: the filter smooths more)
//     --denoise-batches K (2 .. 64, default 4, reduced to the samples per pixel; implies --denoise-variance measured)
//     --dump-variance FILE.pfm (with --denoise-variance measured: the variance in all three channels)
//     --despeckle (the energy-preserving outlier filter, DESIGN.md 4.15: the finished film goes through hrt_despeckle on the first device
//         before --denoise, or on its own; the image file and --dump-linear hold the result, --dump-noisy the film before both stages.
//         It is given the measured variance when the run has one (--denoise-variance measured, --adaptive); without one its variance gate is off and
//         the program says so.  The denoiser receives the variance unchanged.  Previews and checkpoints stay unfiltered)
//     --despeckle-ratio X (finite, > 1; 2)   --despeckle-rank K (1 .. 4; 2)   --despeckle-radius R (1 or 2; 1)
//     --despeckle-gate Z (finite, >= 0; 2; 0 switches the gate off)   (each implies --despeckle)
//     --despeckle-map FILE.pfm (needs --despeckle: 1 - s where a pixel was brought down to a share s of itself, -1 where a non-finite
//         pixel was repaired, 0 elsewhere; in all three channels)
//     --filter tent|bspline|mitchell (the film's reconstruction filter, DESIGN.md 4.16: a pixel is the weighted mean of the samples of
//         its neighbourhood instead of the mean of its own, the box filter; the same paths, the same rays.  One GPU; not with --adaptive,
//         --checkpoint / --resume, --denoise-variance measured or --denoise-batches.  Combines with the --nee flags, --stratified, --roulette,
//         --lens, --progressive, --aov*, --despeckle and --denoise; the previews of --progressive show the unnormalised sums over the
//         samples done, and the feature buffers of --aov stay box-filtered)
//     --filter-radius X (the filter's radius in pixels, 0.5 .. 2.5; tent 1, bspline 2, mitchell 2 by default; needs --filter)
//     --bloom (the develop stage, DESIGN.md 4.17: the finished film -- after --despeckle and --denoise -- goes through hrt_develop on the
//         first device before it is resolved; an energy-conserving pyramid bloom of 5 levels, mixed in at strength 0.05.  The image file and
//         --dump-linear hold the developed film; previews, checkpoints and every --aov file stay undeveloped)
//     --bloom-strength S (0 .. 1; 0.05)   --bloom-levels N (1 .. 8; 5)   (each implies --bloom)
//     --exposure EV|auto (the same stage: EV, a number of stops from -64 to 64, multiplies the film by 2^EV; auto meters the film after
//         the bloom -- the mean of its log luminance between the 10th and the 90th percentile -- and brings that level to 0.18)
//     --exposure-key K (finite, > 0; 0.18)   --exposure-window LO,HI (0 <= LO < HI <= 1; 0.1,0.9)   (each implies --exposure auto and is
//         a usage error with a numeric --exposure)
//     --dump-undeveloped FILE.pfm (needs one of the develop flags: the linear film the stage received)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <cmath>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/hrt_host.h"
#include "assets.h"
#include "classes.h"
#include "image_io.h"
#include "render.h"

using namespace hrthost;

// sigma_l under --denoise-variance measured when --denoise-sigma-l is not given: the lowest worse-of-two error ratio of the sweep of
// DESIGN.md 4.13 at K = 4 (hrt_denoise_defaults keeps 2.5, the best value for the spatial estimate)
constexpr float kMeasuredSigmaL = 6.0f;

constexpr int NUM_THREADS = 12;  // main.cpp:34 (unused by render, as in the reference)

static void printElapsed(const char* what, std::chrono::high_resolution_clock::time_point start) {
    auto eMS = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::high_resolution_clock::now() - start);
    unsigned int iH = (unsigned)std::chrono::duration_cast<std::chrono::hours>(eMS).count();
    unsigned int iM = (unsigned)std::chrono::duration_cast<std::chrono::minutes>(eMS).count() - (iH * 60);
    long double fS = (eMS.count() / 1000.0) - (double)((iM * 60) + (iH * 3600));
    std::cout << std::endl << std::setprecision(6) << what << " (completed in " << iH << ":" << iM << ":" << fS << ")" << std::endl;
}

int main(int argc, char** argv) {
    auto start = std::chrono::high_resolution_clock::now();
    std::string file = "teapot_scene.yaml";  // main.cpp:146
    std::string assets, out, makeAssets, dumpLinear, dumpNoisy, sampleMap, aovPrefix, dumpVariance, despeckleMap;
    std::string filterName;
    bool haveFilterRadius = false;
    double filter_s = 0.0;
    bool develop = false, exposureNumeric = false, exposureAutoOnly = false;
    std::string dumpUndeveloped;
    hrt_develop_params dvp;
    hrt_develop_defaults(&dvp);
    bool despeckle = false;
    hrt_despeckle_params dsp;
    hrt_despeckle_defaults(&dsp);
    bool denoise = false, measured = false, haveVarianceMode = false, haveSigmaL = false;
    long denoiseBatches = 4;
    hrt_denoise_params dnp;
    hrt_denoise_defaults(&dnp);
    long aovSpp = -1;
    bool aovIds = false;
    struct Matte { bool material; std::vector<int32_t> ids; std::string file; };
    std::vector<Matte> mattes;
    bool haveAovSpp = false;
    RenderOptions opt;
    int spp = -1, sw = -1, sh = -1;
    bool haveFile = false;
    // a non-negative finite number, or exit 2 (before anything has touched a device)
    auto number = [](const char* flag, const char* v) -> float {
        char* end = nullptr;
        const double x = std::strtod(v, &end);
        if (end == v || *end != '\0' || !std::isfinite(x) || x < 0.0) { std::cerr << flag << " takes a number >= 0" << std::endl; std::exit(2); }
        return (float)x;
    };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&](const char* flag) -> const char* {
            if (i + 1 >= argc) { std::cerr << flag << " needs a value" << std::endl; std::exit(2); }
            return argv[++i];
        };
        if (a == "--gpus") opt.gpus = std::atoi(next("--gpus"));
        else if (a == "--seed") opt.seed = std::strtoull(next("--seed"), nullptr, 0);
        else if (a == "--spp") spp = std::atoi(next("--spp"));
        else if (a == "--size") { if (std::sscanf(next("--size"), "%dx%d", &sw, &sh) != 2) { std::cerr << "--size WxH" << std::endl; return 2; } }
        else if (a == "--quirks") { std::string q = next("--quirks"); opt.quirks = (q == "fixed") ? HRT_QUIRKS_FIXED : HRT_QUIRKS_REFERENCE; }
        else if (a == "--assets") assets = next("--assets");
        else if (a == "--out") out = next("--out");
        else if (a == "--stats") opt.stats = true;
        else if (a == "--no-progress") opt.progress = false;
        else if (a == "--progress-ms") opt.progress_interval_ms = std::max(1, std::atoi(next("--progress-ms")));
        else if (a == "--rccl") opt.force_rccl = true;
        else if (a == "--lens") opt.thin_lens = true;
        else if (a == "--nee") opt.nee = true;
        else if (a == "--nee-env") { opt.nee = true; opt.nee_env = true; }
        else if (a == "--nee-emitters") { opt.nee = true; opt.nee_emitters = true; }
        else if (a == "--nee-lobes") { opt.nee = true; opt.nee_lobes = true; }
        else if (a == "--stratified") opt.stratified = true;
        else if (a == "--roulette") opt.roulette = true;
        else if (a == "--roulette-start") {
            const char* v = next("--roulette-start");
            char* end = nullptr;
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 0 || n > 0x7fffffffl) { std::cerr << "--roulette-start takes an integer >= 0" << std::endl; return 2; }
            opt.roulette = true; opt.roulette_start = (int)n;
        }
        else if (a == "--roulette-floor") {
            opt.roulette_floor = number("--roulette-floor", next("--roulette-floor"));
            if (!(opt.roulette_floor > 0.0f && opt.roulette_floor <= 1.0f)) { std::cerr << "--roulette-floor takes a number in (0, 1]" << std::endl; return 2; }
            opt.roulette = true;
        }
        else if (a == "--obj-indices") { std::string v = next("--obj-indices"); setenv("HRT_OBJ_INDICES", v == "rebased" ? "rebased" : "reference", 1); }
        else if (a == "--bvh") {     // who builds the meshes' culling trees: the host (binned SAH, default) or the GPU (gpu-sah: the same tree; lbvh: fastest to build, +16 % box tests)
            const std::string v = next("--bvh");
            if (v == "lbvh") hrt_host_set_bvh_builder(hrt_bvh_build_device, 0);
            else if (v == "gpu-sah") hrt_host_set_bvh_builder(hrt_bvh_build_sah, 0);
            else if (v != "sah") { std::cerr << "--bvh takes sah, gpu-sah or lbvh" << std::endl; return -1; }
        }
        else if (a == "--make-assets") makeAssets = next("--make-assets");
        else if (a == "--progressive") opt.pass_samples = std::atoi(next("--progressive"));
        else if (a == "--checkpoint") opt.checkpoint = next("--checkpoint");
        else if (a == "--resume") opt.resume = true;
        else if (a == "--max-passes") opt.max_passes = std::atoi(next("--max-passes"));
        else if (a == "--dump-linear") dumpLinear = next("--dump-linear");
        else if (a == "--adaptive") opt.adaptive = number("--adaptive", next("--adaptive"));
        else if (a == "--adaptive-floor") opt.adaptive_floor = number("--adaptive-floor", next("--adaptive-floor"));
        else if (a == "--min-samples") opt.min_samples = std::atoi(next("--min-samples"));
        else if (a == "--sample-map") sampleMap = next("--sample-map");
        else if (a == "--aov") aovPrefix = next("--aov");
        else if (a == "--aov-spp") {
            const char* v = next("--aov-spp");
            char* end = nullptr;
            aovSpp = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || aovSpp < 1 || aovSpp > 0x7fffffffl) { std::cerr << "--aov-spp takes an integer >= 1" << std::endl; return 2; }
            haveAovSpp = true;
        }
        else if (a == "--aov-ids") aovIds = true;
        else if (a == "--matte") {     // object:ID[,ID...] or material:ID[,ID...], then the file
            const std::string spec = next("--matte");
            Matte m;
            const size_t colon = spec.find(':');
            const std::string kind = spec.substr(0, colon);
            bool ok = colon != std::string::npos && (kind == "object" || kind == "material");
            m.material = kind == "material";
            const char* v = ok ? spec.c_str() + colon + 1 : "";
            while (ok) {
                char* end = nullptr;
                const long id = std::strtol(v, &end, 10);
                ok = end != v && id >= -1 && id < (1l << 24) && (*end == ',' || *end == '\0');
                if (!ok) break;
                m.ids.push_back((int32_t)id);
                if (*end == '\0') break;
                v = end + 1;
            }
            if (!ok || m.ids.empty()) { std::cerr << "--matte takes object:ID[,ID...] or material:ID[,ID...] (ids from -1, the miss, to 2^24 - 1) and a file" << std::endl; return 2; }
            m.file = next("--matte");
            mattes.push_back(m);
            aovIds = true;
        }
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-iterations") {
            const char* v = next("--denoise-iterations");
            char* end = nullptr;
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > 8) { std::cerr << "--denoise-iterations takes an integer from 1 to 8" << std::endl; return 2; }
            denoise = true; dnp.iterations = (int32_t)n;
        }
        else if (a == "--denoise-sigma-l" || a == "--denoise-sigma-z") {
            const float x = number(a.c_str(), next(a.c_str()));
            if (!(x > 0.0f) || !std::isfinite(x)) { std::cerr << a << " takes a finite number > 0" << std::endl; return 2; }
            denoise = true; (a == "--denoise-sigma-l" ? dnp.sigma_l : dnp.sigma_z) = x;
            if (a == "--denoise-sigma-l") haveSigmaL = true;
        }
        else if (a == "--denoise-variance") {
            const std::string v = next("--denoise-variance");
            if (v != "spatial" && v != "measured") { std::cerr << "--denoise-variance takes spatial or measured" << std::endl; return 2; }
            denoise = true; measured = v == "measured"; haveVarianceMode = true;
        }
        else if (a == "--denoise-batches") {
            const char* v = next("--denoise-batches");
            char* end = nullptr;
            denoiseBatches = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || denoiseBatches < 2 || denoiseBatches > 64) { std::cerr << "--denoise-batches takes an integer from 2 to 64" << std::endl; return 2; }
            denoise = true;
            if (!haveVarianceMode) measured = true;
        }
        else if (a == "--filter") {
            filterName = next("--filter");
            opt.filter_kind = filterName == "tent" ? HRT_FILTER_TENT : filterName == "bspline" ? HRT_FILTER_BSPLINE : filterName == "mitchell" ? HRT_FILTER_MITCHELL : -1;
            if (opt.filter_kind < 0) { std::cerr << "--filter takes tent, bspline or mitchell" << std::endl; return 2; }
        }
        else if (a == "--filter-radius") {
            opt.filter_radius = number("--filter-radius", next("--filter-radius"));
            if (!(opt.filter_radius >= 0.5f && opt.filter_radius <= 2.5f)) { std::cerr << "--filter-radius takes a number from 0.5 to 2.5" << std::endl; return 2; }
            haveFilterRadius = true;
        }
        else if (a == "--despeckle") despeckle = true;
        else if (a == "--despeckle-rank" || a == "--despeckle-radius") {
            const bool isRank = a == "--despeckle-rank";
            const char* v = next(a.c_str());
            char* end = nullptr;
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > (isRank ? 4 : 2)) { std::cerr << a << " takes an integer from 1 to " << (isRank ? 4 : 2) << std::endl; return 2; }
            despeckle = true; (isRank ? dsp.rank : dsp.radius) = (int32_t)n;
        }
        else if (a == "--despeckle-ratio") {
            const float x = number("--despeckle-ratio", next("--despeckle-ratio"));
            if (!(x > 1.0f) || !std::isfinite(x)) { std::cerr << "--despeckle-ratio takes a finite number > 1" << std::endl; return 2; }
            despeckle = true; dsp.ratio = x;
        }
        else if (a == "--despeckle-gate") {
            const float x = number("--despeckle-gate", next("--despeckle-gate"));
            if (!std::isfinite(x)) { std::cerr << "--despeckle-gate takes a finite number >= 0" << std::endl; return 2; }
            despeckle = true; dsp.gate_z = x;
        }
        else if (a == "--despeckle-map") despeckleMap = next("--despeckle-map");
        else if (a == "--bloom") { develop = true; if (dvp.bloom_levels == 0) dvp.bloom_levels = 5; }
        else if (a == "--bloom-strength") {
            const float x = number("--bloom-strength", next("--bloom-strength"));
            if (!(x <= 1.0f)) { std::cerr << "--bloom-strength takes a number from 0 to 1" << std::endl; return 2; }
            develop = true; dvp.bloom_strength = x;
            if (dvp.bloom_levels == 0) dvp.bloom_levels = 5;
        }
        else if (a == "--bloom-levels") {
            const char* v = next("--bloom-levels");
            char* end = nullptr;
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > 8) { std::cerr << "--bloom-levels takes an integer from 1 to 8" << std::endl; return 2; }
            develop = true; dvp.bloom_levels = (int32_t)n;
        }
        else if (a == "--exposure") {
            const std::string v = next("--exposure");
            develop = true;
            if (v == "auto") dvp.exposure_mode = 2;
            else {
                char* end = nullptr;
                const double x = std::strtod(v.c_str(), &end);
                if (end == v.c_str() || *end != '\0' || !std::isfinite(x) || std::fabs(x) > 64.0) { std::cerr << "--exposure takes auto or a number of stops from -64 to 64" << std::endl; return 2; }
                dvp.exposure_mode = 1; dvp.exposure_ev = (float)x; exposureNumeric = true;
            }
        }
        else if (a == "--exposure-key") {
            const float x = number("--exposure-key", next("--exposure-key"));
            if (!(x > 0.0f) || !std::isfinite(x)) { std::cerr << "--exposure-key takes a finite number > 0" << std::endl; return 2; }
            develop = true; exposureAutoOnly = true; dvp.key = x;
        }
        else if (a == "--exposure-window") {
            const char* v = next("--exposure-window");
            char* end = nullptr;
            const double lo = std::strtod(v, &end);
            bool ok = end != v && *end == ',';
            double hi = 0.0;
            if (ok) { const char* v2 = end + 1; hi = std::strtod(v2, &end); ok = end != v2 && *end == '\0'; }
            if (!ok || !(lo >= 0.0 && (float)lo < (float)hi && hi <= 1.0)) { std::cerr << "--exposure-window takes LO,HI with 0 <= LO < HI <= 1" << std::endl; return 2; }
            develop = true; exposureAutoOnly = true; dvp.meter_low = (float)lo; dvp.meter_high = (float)hi;
        }
        else if (a == "--dump-undeveloped") dumpUndeveloped = next("--dump-undeveloped");
        else if (a == "--dump-variance") dumpVariance = next("--dump-variance");
        else if (a == "--dump-noisy") dumpNoisy = next("--dump-noisy");
        else if (!haveFile) { file = a; haveFile = true; }
    }
    if (opt.adaptive >= 0.0f) {
        const char* why = opt.gpus > 1 ? "--gpus N > 1" : !opt.checkpoint.empty() ? "--checkpoint" : opt.resume ? "--resume" : nullptr;
        if (why) { std::cerr << "--adaptive cannot be combined with " << why << std::endl; return 2; }
        if (opt.min_samples < 2) { std::cerr << "--min-samples must be >= 2" << std::endl; return 2; }
        if (opt.pass_samples <= 0) opt.pass_samples = 16;
    } else if (!sampleMap.empty()) { std::cerr << "--sample-map needs --adaptive" << std::endl; return 2; }
    if (haveFilterRadius && opt.filter_kind < 0) { std::cerr << "--filter-radius needs --filter tent|bspline|mitchell" << std::endl; return 2; }
    if (opt.filter_kind >= 0) {
        const char* why = opt.adaptive >= 0.0f ? "--adaptive" : opt.gpus > 1 ? "--gpus N > 1" : !opt.checkpoint.empty() ? "--checkpoint" : opt.resume ? "--resume" :
                          measured ? "--denoise-variance measured / --denoise-batches" : nullptr;
        if (why) { std::cerr << "--filter cannot be combined with " << why << std::endl; return 2; }
        opt.filter_seconds = &filter_s;
    }
    if (haveAovSpp && aovPrefix.empty() && !denoise) { std::cerr << "--aov-spp needs --aov PREFIX" << std::endl; return 2; }
    if (aovIds && aovPrefix.empty()) { std::cerr << (mattes.empty() ? "--aov-ids" : "--matte") << " needs --aov PREFIX" << std::endl; return 2; }
    if (!dumpNoisy.empty() && !denoise && !despeckle) { std::cerr << "--dump-noisy needs --denoise or --despeckle" << std::endl; return 2; }
    if (!despeckleMap.empty() && !despeckle) { std::cerr << "--despeckle-map needs --despeckle" << std::endl; return 2; }
    if (exposureAutoOnly && exposureNumeric) { std::cerr << "--exposure-key and --exposure-window meter the film: they cannot be combined with a numeric --exposure" << std::endl; return 2; }
    if (exposureAutoOnly) dvp.exposure_mode = 2;
    if (!dumpUndeveloped.empty() && !develop) { std::cerr << "--dump-undeveloped needs --bloom or --exposure" << std::endl; return 2; }
    if (!dumpVariance.empty() && !measured) { std::cerr << "--dump-variance needs --denoise-variance measured" << std::endl; return 2; }
    if (!makeAssets.empty()) {
        long t = writeTeapotObj(makeAssets + "/teapot.obj", 1.0);
        long b = writeBustObj(makeAssets + "/marble_bust_01.obj", 1.0);
        bool h = writeHallHdr(makeAssets + "/old_hall_4k.hdr", 4096, 2048);
        std::cout << "teapot.obj: " << t << " triangles, marble_bust_01.obj: " << b << " triangles, old_hall_4k.hdr: " << (h ? "ok" : "FAILED") << std::endl;
        return (t > 0 && b > 0 && h) ? 0 : 1;
    }

    Scene scene;
    if (scene.loadScene(file, assets) < 1) return -1;  // main.cpp:155-156

    std::shared_ptr<Film> film = scene.getFilm();
    if (sw > 0 || spp > 0) {
        film_desc f = film->getFilm();
        if (sw > 0 && (sw < 2 || sh < 2 || (long long)sw * sh > (1ll << 30))) { std::cerr << "--size: 2x2 up to 2^30 pixels" << std::endl; return 2; }
        scene.setFilmSize(sw > 0 ? sw : f.width, sh > 0 ? sh : f.height, spp > 0 ? spp : f.samples);
    }
    if (!out.empty()) film->setOutput(out);
    Camera camera = scene.getCamera();
    std::shared_ptr<Texture> background = scene.getBackground();
    std::shared_ptr<HittableList> world = scene.getScene();

    printElapsed(("Loaded scene: " + file + "!").c_str(), start);
    const double load_s = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - start).count();

    if (opt.resume && opt.checkpoint.empty()) { std::cerr << "--resume needs --checkpoint FILE" << std::endl; return 2; }
    if (opt.adaptive >= 0.0f && film->getFilm().samples < 2) { std::cerr << "--adaptive needs at least 2 samples per pixel" << std::endl; return 2; }
    if (haveAovSpp && aovSpp > film->getFilm().samples) { std::cerr << "--aov-spp must not exceed the samples per pixel (" << film->getFilm().samples << ")" << std::endl; return 2; }
    std::vector<float> aov;
    double aov_s = 0.0, denoise_s = 0.0, variance_s = 0.0, despeckle_s = 0.0, develop_s = 0.0;
    hrt_develop_info developInfo{};
    unsigned long long despecklePixels = 0, despeckleRepaired = 0;
    std::vector<float> variance;
    if (measured || (despeckle && opt.adaptive >= 0.0f)) {   // (an adaptive render's buffers hold a variance: the outlier filter takes it)
        opt.variance_out = &variance;
        opt.variance_seconds = &variance_s;
        opt.variance_batches = (int)denoiseBatches;
    }
    if (!aovPrefix.empty() || denoise) {
        opt.aov_samples = haveAovSpp ? (int)aovSpp : std::min(film->getFilm().samples, 16);
        opt.aov_out = &aov;
        opt.aov_seconds = &aov_s;
    }
    std::vector<uint8_t> aovIdsBuf;
    std::string idManifest;
    double aov_ids_s = 0.0;
    if (aovIds) {
        opt.aov_ids_out = &aovIdsBuf;
        opt.aov_ids_seconds = &aov_ids_s;
        opt.aov_ids_manifest = &idManifest;
        opt.material_names = &scene.getMaterials();
    }
    std::vector<int32_t> counts;
    if (opt.adaptive >= 0.0f) opt.sample_counts = &counts;
    if (opt.pass_samples > 0) opt.on_pass = [&film](int) { film->outputFilm(); };   // preview image after every pass
    hrt_stats stats{};
    double seconds = 0.0;
    hrt_status st = render(NUM_THREADS, background, world, camera, film, opt, &stats, &seconds);
    if (st != HRT_OK) return -1;

    std::vector<float> unfiltered;   // the film before both stages, for --dump-noisy
    if (despeckle || denoise) unfiltered = film->linear();
    if (despeckle) {   // the finished film through the outlier filter on the first device, ahead of the denoiser; resolved below unless --denoise does
        const int w = film->getFilm().width, h = film->getFilm().height;
        const auto t0 = std::chrono::high_resolution_clock::now();
        const bool haveVariance = variance.size() == (size_t)w * h;
        if (!haveVariance && dsp.gate_z > 0.0f) std::cerr << "despeckle: no measured variance (--denoise-variance measured, --adaptive): the variance gate is off" << std::endl;
        std::vector<float> map((size_t)w * h);
        st = hrt_despeckle(0, w, h, &dsp, unfiltered.data(), haveVariance ? variance.data() : nullptr, film->linear().data(), map.data());
        if (st == HRT_OK && !denoise) st = hrt_denoise_resolve_u8(0, film->linear().data(), (int64_t)w * h, film->getPixels());
        if (st != HRT_OK) { std::cerr << "despeckle: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl; return -1; }
        despeckle_s = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        for (const float m : map) { despecklePixels += m > 0.0f; despeckleRepaired += m < 0.0f; }
        if (!despeckleMap.empty()) {
            std::vector<float> img((size_t)w * h * 3);
            for (size_t i = 0; i < (size_t)w * h; ++i) img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = map[i];
            if (!writePFM(despeckleMap, img.data(), w, h)) { std::cerr << "cannot write " << despeckleMap << std::endl; return -1; }
        }
        if (!denoise && !dumpNoisy.empty() && !writePFM(dumpNoisy, unfiltered.data(), w, h)) { std::cerr << "cannot write " << dumpNoisy << std::endl; return -1; }
    }
    if (denoise) {   // the finished film, filtered on the first device and resolved as the film resolves itself; the noisy one is kept for --dump-noisy
        const int w = film->getFilm().width, h = film->getFilm().height;
        const auto t0 = std::chrono::high_resolution_clock::now();
        std::vector<float> noisy = film->linear();
        const bool haveVariance = measured && variance.size() == (size_t)w * h;
        if (measured && !haveVariance) std::cerr << "denoise: fewer than two batches of samples to measure the variance from: using the spatial estimate" << std::endl;
        if (haveVariance && !haveSigmaL) dnp.sigma_l = kMeasuredSigmaL;
        st = hrt_denoise(0, w, h, &dnp, noisy.data(), aov.data(), haveVariance ? variance.data() : nullptr, film->linear().data());
        if (st == HRT_OK) st = hrt_denoise_resolve_u8(0, film->linear().data(), (int64_t)w * h, film->getPixels());
        if (st != HRT_OK) { std::cerr << "denoise: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl; return -1; }
        denoise_s = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        if (!dumpNoisy.empty() && !writePFM(dumpNoisy, unfiltered.data(), w, h)) { std::cerr << "cannot write " << dumpNoisy << std::endl; return -1; }
        if (!dumpVariance.empty() && !haveVariance) std::cerr << "--dump-variance: no variance was measured, " << dumpVariance << " is not written" << std::endl;
        if (!dumpVariance.empty() && haveVariance) {
            std::vector<float> img((size_t)w * h * 3);
            for (size_t i = 0; i < (size_t)w * h; ++i) img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = variance[i];
            if (!writePFM(dumpVariance, img.data(), w, h)) { std::cerr << "cannot write " << dumpVariance << std::endl; return -1; }
        }
    }
    if (develop) {   // the clean film through the develop stage on the first device, and resolved as the film resolves itself
        const int w = film->getFilm().width, h = film->getFilm().height;
        const auto t0 = std::chrono::high_resolution_clock::now();
        const std::vector<float> undeveloped = film->linear();
        st = hrt_develop(0, w, h, &dvp, undeveloped.data(), film->linear().data(), &developInfo, nullptr);
        if (st == HRT_OK) st = hrt_denoise_resolve_u8(0, film->linear().data(), (int64_t)w * h, film->getPixels());
        if (st != HRT_OK) { std::cerr << "develop: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl; return -1; }
        develop_s = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        if (!dumpUndeveloped.empty() && !writePFM(dumpUndeveloped, undeveloped.data(), w, h)) { std::cerr << "cannot write " << dumpUndeveloped << std::endl; return -1; }
    }
    int r = film->outputFilm();
    if (!dumpLinear.empty() && !writePFM(dumpLinear, film->linear().data(), film->getFilm().width, film->getFilm().height)) {
        std::cerr << "cannot write " << dumpLinear << std::endl;
        return -1;
    }
    if (!aovPrefix.empty()) {   // the four feature images, through the film's own PFM writer; the scalars in all three channels
        const int w = film->getFilm().width, h = film->getFilm().height;
        const size_t n = (size_t)w * h;
        std::vector<float> img(n * 3);
        const struct { const char* name; int first; bool scalar; } parts[4] = {{"albedo", 0, false}, {"normal", 4, false}, {"depth", 7, true}, {"alpha", 3, true}};
        for (const auto& part : parts) {
            for (size_t i = 0; i < n; ++i)
                for (int k = 0; k < 3; ++k) img[3 * i + k] = aov[8 * i + part.first + (part.scalar ? 0 : k)];
            const std::string path = aovPrefix + "." + part.name + ".pfm";
            if (!writePFM(path, img.data(), w, h)) { std::cerr << "cannot write " << path << std::endl; return -1; }
        }
    }
    if (aovIds) {   // hrt.h's 80 bytes per pixel: position | object ids | object coverages | material ids | material coverages
        const int w = film->getFilm().width, h = film->getFilm().height;
        const size_t n = (size_t)w * h;
        std::vector<float> img(n * 3);
        auto f32 = [&](size_t i, int word) { float x; std::memcpy(&x, aovIdsBuf.data() + 80 * i + 4 * word, 4); return x; };
        auto i32 = [&](size_t i, int word) { int32_t x; std::memcpy(&x, aovIdsBuf.data() + 80 * i + 4 * word, 4); return x; };
        auto write = [&](const std::string& path) {
            if (writePFM(path, img.data(), w, h)) return true;
            std::cerr << "cannot write " << path << std::endl;
            return false;
        };
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) img[3 * i + k] = f32(i, k);
        if (!write(aovPrefix + ".position.pfm")) return -1;
        for (int kind = 0; kind < 2; ++kind)
            for (int rank = 0; rank < HRT_AOV_ID_RANKS; ++rank) {
                for (size_t i = 0; i < n; ++i) {
                    img[3 * i] = (float)i32(i, 4 + 8 * kind + rank);
                    img[3 * i + 1] = f32(i, 8 + 8 * kind + rank);
                    img[3 * i + 2] = 0.0f;
                }
                if (!write(aovPrefix + (kind ? ".material" : ".object") + std::to_string(rank) + ".pfm")) return -1;
            }
        for (const Matte& m : mattes) {   // the coverages of the wanted ids, added in rank order
            for (size_t i = 0; i < n; ++i) {
                float sum = 0.0f;
                for (int rank = 0; rank < HRT_AOV_ID_RANKS; ++rank)
                    if (std::find(m.ids.begin(), m.ids.end(), i32(i, 4 + 8 * (m.material ? 1 : 0) + rank)) != m.ids.end())
                        sum = sum + f32(i, 8 + 8 * (m.material ? 1 : 0) + rank);
                img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = sum;
            }
            if (!write(m.file)) return -1;
        }
        FILE* mf = std::fopen((aovPrefix + ".ids.txt").c_str(), "w");
        if (!mf || std::fputs(idManifest.c_str(), mf) < 0 || std::fclose(mf) != 0) { std::cerr << "cannot write " << aovPrefix << ".ids.txt" << std::endl; return -1; }
    }
    if (!sampleMap.empty()) {
        std::vector<float> m(counts.size() * 3);
        for (size_t i = 0; i < counts.size(); ++i) m[3 * i] = m[3 * i + 1] = m[3 * i + 2] = (float)counts[i];
        if (!writePFM(sampleMap, m.data(), film->getFilm().width, film->getFilm().height)) {
            std::cerr << "cannot write " << sampleMap << std::endl;
            return -1;
        }
    }

    if (opt.stats || std::getenv("HRT_STATS")) {
        const double bytes = 32.0 * stats.box_tests + 36.0 * stats.tri_tests + 60.0 * stats.mesh_hits + 12.0 * stats.env_lookups +
                             12.0 * film->getFilm().width * film->getFilm().height;
        // wall_s: the reference's own stopwatch (main.cpp:144,184): process start to after the image file is written
        const double wall_s = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - start).count();
        char extra[1024] = "";
        if (opt.adaptive >= 0.0f) {   // the samples adaptive sampling took, and their share of the uniform render's
            const double uniform = (double)film->getFilm().width * film->getFilm().height * film->getFilm().samples;
            std::snprintf(extra, sizeof(extra), ", \"adaptive_threshold\": %g, \"samples_taken\": %llu, \"sample_fraction\": %.6f",
                          opt.adaptive, (unsigned long long)stats.samples, (double)stats.samples / uniform);
        }
        if (opt.nee) {                // the shadow rays of next-event estimation (not part of `rays`)
            const size_t k = std::strlen(extra);
            std::snprintf(extra + k, sizeof(extra) - k, ", \"shadow_rays\": %llu", (unsigned long long)stats.shadow_rays);
        }
        if (opt.aov_samples > 0) {    // the feature-buffer pass: its samples per pixel and the wall time of the call
            const size_t k = std::strlen(extra);
            std::snprintf(extra + k, sizeof(extra) - k, ", \"aov_spp\": %d, \"aov_s\": %.6f", opt.aov_samples, aov_s);
        }
        if (aovIds) {                 // the id pass: the wall time of its call on the feature pass's scene
            const size_t k = std::strlen(extra);
            std::snprintf(extra + k, sizeof(extra) - k, ", \"aov_ids_s\": %.6f", aov_ids_s);
        }
        if (denoise) {                // the filter and the resolve of the filtered film: the wall time of the two calls, copies included
            const size_t k = std::strlen(extra);
            std::snprintf(extra + k, sizeof(extra) - k, ", \"denoise_s\": %.6f", denoise_s);
        }
        if (despeckle) {              // the outlier filter (and, without --denoise, the resolve): the wall time, copies included; the counts from its map
            const size_t k = std::strlen(extra);
            std::snprintf(extra + k, sizeof(extra) - k, ", \"despeckle_s\": %.6f, \"despeckle_pixels\": %llu, \"despeckle_repaired\": %llu", despeckle_s, despecklePixels, despeckleRepaired);
        }
        if (opt.filter_kind >= 0) {   // the reconstruction filter: its kind and the time of its own kernels, from HIP events
            const size_t k = std::strlen(extra);
            std::snprintf(extra + k, sizeof(extra) - k, ", \"filter\": \"%s\", \"filter_s\": %.6f", filterName.c_str(), filter_s);
        }
        if (develop) {                // the develop stage and its resolve: the wall time, copies included; the levels used, the factor applied and,
            const size_t k = std::strlen(extra);   // under --exposure auto, the metered level in stops (otherwise the stops given)
            std::snprintf(extra + k, sizeof(extra) - k, ", \"develop_s\": %.6f, \"bloom_levels\": %u, \"exposure_scale\": %.9g, \"exposure_ev\": %.17g", develop_s,
                          dvp.bloom_strength != 0.0f ? developInfo.levels : 0u, (double)developInfo.scale, dvp.exposure_mode == 2 ? developInfo.mean_ev : (double)dvp.exposure_ev);
        }
        if (measured) {               // the measured variance: the wall time of its folds on the first device, copies included
            const size_t k = std::strlen(extra);
            std::snprintf(extra + k, sizeof(extra) - k, ", \"variance_s\": %.6f", variance_s);
        }
        std::printf("{\"rays\": %llu, \"samples\": %llu, \"box_tests\": %llu, \"tri_tests\": %llu, \"render_s\": %.6f, "
                    "\"kernel_ms\": %.3f, \"mrays_per_s\": %.3f, \"msamples_per_s\": %.3f, \"algorithmic_gb_per_s\": %.3f, "
                    "\"load_s\": %.6f, \"wall_s\": %.6f, \"gpus\": %d%s}\n",
                    (unsigned long long)stats.rays, (unsigned long long)stats.samples, (unsigned long long)stats.box_tests,
                    (unsigned long long)stats.tri_tests, seconds, stats.kernel_ms, stats.rays / seconds / 1e6,
                    stats.samples / seconds / 1e6, stats.kernel_ms > 0 ? bytes / (stats.kernel_ms * 1e-3) / 1e9 : 0.0, load_s, wall_s, opt.gpus, extra);
    }
    printElapsed("Done!", start);
    return r;  // main.cpp:194 (1 = success)
}
