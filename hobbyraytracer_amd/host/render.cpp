// render.cpp — render() (main.cpp:81-140) on the GPU path.
//
// The scene is replicated on every device; image rows are dealt
// to devices in interleaved blocks of `rows_per_block` rows so that sky rows
// and geometry rows are shared out evenly; the RNG is keyed by the absolute
// pixel index, so the result is bit-identical for every device count.  The
// devices keep their stripes in their own memory; libhrt_hip.so's multi-GPU
// session (hrt_multi_*) gathers them on the first device over RCCL / xGMI,
// which also resolves the film to u8 (Film::tonemap + writeColour).
#include "render.h"

#include <atomic>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace hrthost {

namespace {
// Checkpoint of a progressive render: header + width*height*3 fp32 sums in absolute row order.
struct Checkpoint {
    int32_t width, height, samples, next_sample;
    uint64_t seed;
    uint32_t quirks;
    int32_t max_depth;
    uint64_t scene_hash;   // of the flattened scene and the camera: sums of another scene must not be continued
};
const char kMagic[8] = {'H', 'R', 'T', 'C', 'K', 'P', 'T', '2'};

// A render with --nee folds this constant into its checkpoint's scene_hash: its sums are not the default estimator's, and a
// checkpoint of the one cannot be continued by the other (the file format stays as it is).
constexpr uint64_t kNeeHashSalt = 0x4e45452d4d495321ull;   // "NEE-MIS!"
// ... and one with --nee-env folds its own, so that neither --nee nor the default estimator can continue it, nor it them
constexpr uint64_t kNeeEnvHashSalt = 0x4e45452d454e5621ull;   // "NEE-ENV!"
// ... and one with --nee-emitters its own again, on top of the --nee-env salt when both are on
constexpr uint64_t kNeeEmittersHashSalt = 0x4e45452d454d4954ull;   // "NEE-EMIT"
// ... and one with --nee-lobes its own, on top of whichever of the above applies
constexpr uint64_t kNeeLobesHashSalt = 0x4e45452d4c4f4245ull;   // "NEE-LOBE"
// ... and one with --stratified its own, whatever the estimator: its sums continue a sequence, not a stream of independent samples
constexpr uint64_t kStratifiedHashSalt = 0x535452415449464cull;   // "STRATIFL"
// ... and one with --roulette its own, with the rule's two parameters folded in: survivors are re-weighted by them, so only a render
// with the same settings continues its sums
constexpr uint64_t kRouletteHashSalt = 0x524f554c45545445ull;   // "ROULETTE"
// FNV-1a over everything the kernels read of the scene (hrt_flat_scene's arrays) and the camera constants.
uint64_t sceneHash(const hrt_flat_scene& f, const hrt_camera& cam) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t bytes) {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    };
    mix(&cam, sizeof(cam));
    mix(f.prims, sizeof(hrt_prim) * f.n_prims); mix(f.materials, sizeof(hrt_material) * f.n_materials);
    mix(f.textures, sizeof(hrt_texture) * f.n_textures); mix(f.meshes, sizeof(hrt_mesh) * f.n_meshes);
    mix(f.tri_pos, sizeof(float) * 9 * f.n_tris); mix(f.tri_nrm, sizeof(float) * 9 * f.n_tris); mix(f.tri_uv, sizeof(float) * 6 * f.n_tris);
    if (f.tri_ref_order) mix(f.tri_ref_order, sizeof(uint32_t) * f.n_tris);
    mix(f.texels_u8, (size_t)f.n_texels_u8);
    // (a 4096 x 2048 fp32 environment map is 100 MB: sample it -- every 61st float and the size)
    mix(&f.n_texels_f32, sizeof(f.n_texels_f32));
    for (uint64_t i = 0; i < f.n_texels_f32; i += 61) mix(f.texels_f32 + i, sizeof(float));
    mix(&f.background_tex, sizeof(f.background_tex));
    return h;
}

// what a checkpoint's scene_hash holds: the scene and camera, and whether the render estimates with next-event estimation
uint64_t renderHash(const hrt_flat_scene& f, const hrt_camera& cam, const RenderOptions& opt) {
    uint64_t h = sceneHash(f, cam) ^ (opt.nee && opt.nee_lobes ? kNeeLobesHashSalt : 0) ^ (opt.stratified ? kStratifiedHashSalt : 0);
    if (opt.roulette) {
        uint32_t floor_bits;
        std::memcpy(&floor_bits, &opt.roulette_floor, sizeof(floor_bits));
        h ^= (kRouletteHashSalt ^ (uint64_t)(uint32_t)opt.roulette_start ^ ((uint64_t)floor_bits << 32)) * 1099511628211ull;
    }
    if (opt.nee && opt.nee_emitters) return h ^ kNeeEmittersHashSalt ^ (opt.nee_env ? kNeeEnvHashSalt : 0);
    if (opt.nee && opt.nee_env) return h ^ kNeeEnvHashSalt;
    return opt.nee ? h ^ kNeeHashSalt : h;
}

bool writeCheckpoint(const std::string& path, const Checkpoint& ck, const std::vector<float>& sums) {
    const std::string tmp = path + ".tmp";   // never leave a torn file under the real name
    FILE* fp = std::fopen(tmp.c_str(), "wb");
    if (!fp) return false;
    bool ok = std::fwrite(kMagic, 1, 8, fp) == 8 && std::fwrite(&ck, sizeof(ck), 1, fp) == 1 &&
              std::fwrite(sums.data(), sizeof(float), sums.size(), fp) == sums.size();
    ok = (std::fclose(fp) == 0) && ok;
    if (ok) ok = std::rename(tmp.c_str(), path.c_str()) == 0;
    if (!ok) std::remove(tmp.c_str());
    return ok;
}
bool readCheckpoint(const std::string& path, Checkpoint& ck, std::vector<float>& sums, std::string& why) {
    FILE* fp = std::fopen(path.c_str(), "rb");
    if (!fp) { why = "cannot open " + path; return false; }
    char magic[8];
    bool ok = std::fread(magic, 1, 8, fp) == 8 && std::memcmp(magic, kMagic, 8) == 0 && std::fread(&ck, sizeof(ck), 1, fp) == 1;
    if (ok && (ck.width < 2 || ck.height < 2 || (size_t)ck.width * ck.height * 3 != sums.size())) ok = false;
    if (ok) ok = std::fread(sums.data(), sizeof(float), sums.size(), fp) == sums.size();
    std::fclose(fp);
    if (!ok) why = path + " is not a checkpoint of this film";
    return ok;
}
// Adds one pass's counters to a render's running total (the traversal_launches / traversal_ms pair is not summed).
void addPassStats(hrt_stats& total, const hrt_stats& ps) {
    total.rays += ps.rays; total.samples += ps.samples; total.box_tests += ps.box_tests; total.tri_tests += ps.tri_tests;
    total.mesh_hits += ps.mesh_hits; total.env_lookups += ps.env_lookups; total.launches += ps.launches;
    total.traversal_box_tests += ps.traversal_box_tests; total.traversal_tri_tests += ps.traversal_tri_tests;
    total.shadow_rays += ps.shadow_rays;
    total.kernel_ms += ps.kernel_ms;
}
// The adaptive render on the first device (hrt.h hrt_render_stripes_adaptive): passes until no pixel is active, the film is
// sums / count.  Host buffers: one stripe partition (G = 1) is the film in row order.
hrt_status renderAdaptive(const hrt_flat_scene& flat, const hrt_camera& cam, hrt_params pr, std::shared_ptr<Film>& film,
                          const RenderOptions& opt, hrt_stats* stats, double* render_seconds) {
    const film_desc f = film->getFilm();
    const int numPixels = f.width * f.height;
    hrt_adaptive ad{};
    ad.min_samples = std::min(opt.min_samples, f.samples);
    ad.pass_samples = opt.pass_samples > 0 ? opt.pass_samples : 16;
    ad.threshold = opt.adaptive;
    ad.floor = opt.adaptive_floor;
    hrt_scene* sc = nullptr;
    hrt_status st = hrt_scene_create(&flat, 0, &sc);
    if (st != HRT_OK) { std::cerr << "hrt_scene_create: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl; return st; }
    if (opt.roulette && (st = hrt_scene_set_roulette(sc, opt.roulette_start, opt.roulette_floor)) != HRT_OK) {
        std::cerr << "hrt_scene_set_roulette: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
        hrt_scene_destroy(sc);
        return st;
    }
    std::vector<float> sums((size_t)numPixels * 3), sq((size_t)numPixels);
    std::vector<int32_t> count((size_t)numPixels, 0);
    std::vector<float>& lin = film->linear();
    auto mean = [&]() {
        for (size_t i = 0; i < (size_t)numPixels; ++i) {
            const float c = static_cast<float>(count[i]);
            for (int k = 0; k < 3; ++k) lin[3 * i + k] = sums[3 * i + k] / c;
        }
    };
    const auto t0 = std::chrono::high_resolution_clock::now();
    hrt_stats total{};
    for (int pass = 0;; ++pass) {
        int64_t active = 0;
        hrt_stats ps{};
        st = hrt_render_stripes_adaptive(sc, &cam, &pr, opt.rows_per_block, 0, 1, &ad, sums.data(), sq.data(), count.data(), pass, &active, &ps);
        if (st != HRT_OK) break;
        addPassStats(total, ps);
        if (active == 0) break;
        if (opt.progress) std::cout << "\rPass " << pass << ": " << active << "/" << numPixels << " pixels active" << std::flush;
        if (opt.on_pass) {   // preview: the mean of every pixel's samples so far
            mean();
            st = hrt_resolve_u8(sc, lin.data(), numPixels, film->getPixels());
            if (st != HRT_OK) break;
            opt.on_pass((int)(total.samples / (uint64_t)numPixels));
        }
    }
    if (st == HRT_OK) {
        mean();
        st = hrt_resolve_u8(sc, lin.data(), numPixels, film->getPixels());
    }
    if (st == HRT_OK && opt.variance_out) {   // the measured variance, from the buffers the stopping rule itself reads
        const auto v0 = std::chrono::high_resolution_clock::now();
        opt.variance_out->assign((size_t)numPixels, 0.0f);
        st = hrt_adaptive_variance(0, numPixels, sums.data(), sq.data(), count.data(), opt.variance_out->data());
        if (opt.variance_seconds) *opt.variance_seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - v0).count();
    }
    if (st != HRT_OK) std::cerr << "\nadaptive render failed: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (render_seconds) *render_seconds = std::chrono::duration<double>(t1 - t0).count();
    if (opt.progress) std::cout << "\rPixels rendered: " << numPixels << "/" << numPixels << std::flush << "\n";
    hrt_scene_destroy(sc);
    if (opt.sample_counts) *opt.sample_counts = count;
    if (stats) *stats = total;
    return st;
}
// The feature-buffer pass (hrt.h hrt_render_aov_tile) on the first device: a scene of its own, gone again before the film's render
// takes its memory.  Its params are the film's with samples = opt.aov_samples; of the flags only the lens and the sampler are read.
// The film's session (hrt_multi) does not hand out its scenes, so the pass uploads the scene a second time: *opt.aov_seconds is the
// wall time of all of it -- upload, pass and release --, none of which is inside render_seconds.
hrt_status renderAov(const hrt_flat_scene& flat, const hrt_camera& cam, hrt_params pr, const RenderOptions& opt) {
    pr.samples = opt.aov_samples;
    pr.flags &= HRT_FLAG_THIN_LENS | HRT_FLAG_STRATIFIED;
    opt.aov_out->assign((size_t)pr.width * pr.height * 8, 0.0f);
    const auto t0 = std::chrono::high_resolution_clock::now();
    hrt_scene* sc = nullptr;
    hrt_status st = hrt_scene_create(&flat, 0, &sc);
    if (st != HRT_OK) { std::cerr << "hrt_scene_create: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl; return st; }
    st = hrt_render_aov_tile(sc, &cam, &pr, hrt_rect{0, 0, pr.width, pr.height}, opt.aov_out->data());
    if (st != HRT_OK) std::cerr << "feature buffers: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
    double ids_s = 0.0;
    if (st == HRT_OK && opt.aov_ids_out) {   // the id pass: the same samples, the same scene
        const auto t1 = std::chrono::high_resolution_clock::now();
        opt.aov_ids_out->assign((size_t)hrt_aov_ids_bytes((int64_t)pr.width * pr.height), 0);
        st = hrt_render_aov_ids_tile(sc, &cam, &pr, hrt_rect{0, 0, pr.width, pr.height}, opt.aov_ids_out->data());
        if (st != HRT_OK) std::cerr << "id mattes: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
        ids_s = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t1).count();
        if (opt.aov_ids_seconds) *opt.aov_ids_seconds = ids_s;
    }
    hrt_scene_destroy(sc);
    if (opt.aov_seconds) *opt.aov_seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count() - ids_s;
    return st;
}
// PREFIX.ids.txt (--aov-ids): what the ids of the mattes stand for, from the flattened scene the pass renders
std::string idManifest(const FlatBuilder& fb, const std::map<std::string, std::shared_ptr<Material>>* names) {
    static const char* const primKinds[] = {"sphere", "xy_rect", "xz_rect", "yz_rect", "box", "mesh", "medium", "triangle"};
    static const char* const matKinds[] = {"lambertian", "metal", "dielectric", "diffuse_light", "isotropic", "pbr", "uv_test"};
    std::vector<std::string> name(fb.materials.size());
    if (names)
        for (const auto& kv : *names) {
            const int id = fb.materialId(kv.second.get());
            if (id >= 0 && name[(size_t)id].empty()) name[(size_t)id] = kv.first;
        }
    std::ostringstream os;
    os << "# object ID KIND material MATERIAL_ID | material ID KIND [NAME] | a miss is id -1\n";
    for (size_t i = 0; i < fb.prims.size(); ++i) {
        const int k = fb.prims[i].kind;
        os << "object " << i << " " << (k >= 0 && k < 8 ? primKinds[k] : "unknown") << " material " << fb.prims[i].material << "\n";
    }
    for (size_t i = 0; i < fb.materials.size(); ++i) {
        const int k = fb.materials[i].kind;
        os << "material " << i << " " << (k >= 0 && k < 7 ? matKinds[k] : "unknown");
        if (!name[i].empty()) os << " " << name[i];
        os << "\n";
    }
    return os.str();
}
}  // namespace

hrt_status render(int /*nThreads*/, const std::shared_ptr<Texture> background, const std::shared_ptr<Hittable> world,
                  const Camera& camera, std::shared_ptr<Film>& film, const RenderOptions& opt, hrt_stats* stats,
                  double* render_seconds) {
    const film_desc f = film->getFilm();
    const int numPixels = f.width * f.height;

    FlatBuilder fb;
    try {
        flattenWorld(fb, world, background);
    } catch (const FlattenError& e) {
        std::cerr << "flatten: " << e.what() << std::endl;
        return e.status;
    }
    const hrt_flat_scene flat = fb.flat();
    const hrt_camera cam = camera.flatten();

    int ndev = 0;
    hrt_status st = hrt_device_count(&ndev);
    if (st != HRT_OK || ndev < 1) {
        std::cerr << "no MI355X device available: " << hrt_last_error() << " (there is no CPU fallback)" << std::endl;
        return st != HRT_OK ? st : HRT_ERR_NO_DEVICE;
    }
    const int G = opt.gpus < 1 ? 1 : (opt.gpus > ndev ? ndev : opt.gpus);

    hrt_params pr{};
    pr.width = f.width; pr.height = f.height; pr.samples = f.samples;
    pr.max_depth = opt.max_depth; pr.t_min = 0.001f; pr.quirks = opt.quirks;
    pr.seed_lo = (uint32_t)opt.seed; pr.seed_hi = (uint32_t)(opt.seed >> 32);
    // (--roulette has no counting kernels, and the library refuses the two flags together: --stats then prints its line from the
    //  counters that are always kept, and says so)
    if (opt.stats && opt.roulette)
        std::cerr << "--stats with --roulette: box_tests, tri_tests, mesh_hits and env_lookups are not counted (0 in the line); rays, samples and shadow_rays are" << std::endl;
    pr.flags = (opt.stats && !opt.roulette ? HRT_FLAG_STATS : 0) | (opt.thin_lens ? HRT_FLAG_THIN_LENS : 0) | (opt.progress ? HRT_FLAG_PROGRESS : 0) |
               (opt.nee ? HRT_FLAG_NEE : 0) | (opt.nee && opt.nee_env ? HRT_FLAG_NEE_ENV : 0) |
               (opt.nee && opt.nee_emitters ? HRT_FLAG_NEE_EMITTERS : 0) | (opt.nee && opt.nee_lobes ? HRT_FLAG_NEE_LOBES : 0) |
               (opt.stratified ? HRT_FLAG_STRATIFIED : 0) | (opt.roulette ? HRT_FLAG_ROULETTE : 0) | (opt.filter_kind >= 0 ? HRT_FLAG_FILTER : 0);

    if (opt.aov_samples > 0 && opt.aov_out && opt.aov_ids_out) {
        if (fb.prims.size() >= (1u << 24) || fb.materials.size() >= (1u << 24)) {
            std::cerr << "--aov-ids: the scene has 2^24 or more objects or materials; their ids do not fit the float of a PFM file" << std::endl;
            return HRT_ERR_UNSUPPORTED;
        }
        if (opt.aov_ids_manifest) *opt.aov_ids_manifest = idManifest(fb, opt.material_names);
    }
    if (opt.aov_samples > 0 && opt.aov_out && (st = renderAov(flat, cam, pr, opt)) != HRT_OK) return st;

    if (opt.adaptive >= 0.0f) return renderAdaptive(flat, cam, pr, film, opt, stats, render_seconds);

    // The multi-GPU session: scene on every device, stripes accumulated in device memory, RCCL gather (hrt.h hrt_multi_*).
    hrt_multi* multi = nullptr;
    st = hrt_multi_create(&flat, G, nullptr, opt.force_rccl ? 1 : 0, &multi);
    if (st != HRT_OK) {
        std::cerr << "hrt_multi_create(" << G << " devices): " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
        return st;
    }
    if (opt.roulette && (st = hrt_multi_set_roulette(multi, opt.roulette_start, opt.roulette_floor)) != HRT_OK) {
        std::cerr << "hrt_multi_set_roulette: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
        hrt_multi_destroy(multi);
        return st;
    }
    if (opt.filter_kind >= 0 && (st = hrt_multi_set_filter(multi, opt.filter_kind, opt.filter_radius)) != HRT_OK) {
        std::cerr << "hrt_multi_set_filter: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
        hrt_multi_destroy(multi);
        return st;
    }

    std::cout << "\rPixels rendered: 0/" << numPixels << std::flush;  // main.cpp:100
    const auto t0 = std::chrono::high_resolution_clock::now();

    // The reporter thread (main.cpp:97-109).  The reference counts finished pixels; here all pixels finish together, so the
    // figure is the pixel-equivalent of the camera paths that have ended: numPixels x paths ended / all paths, read from the
    // devices' host-mapped progress counters (hrt_multi_progress: no HIP call) every 500 ms.  It is woken when the render is
    // over instead of sleeping its interval out (the reference's join can cost its run up to 500 ms).
    std::atomic<long long> pathsBefore{0};          // paths of the passes already finished
    std::mutex rm;
    std::condition_variable rcv;
    bool reporterStop = false;
    std::thread reporter;
    if (opt.progress) {
        reporter = std::thread([&]() {
            const double allPaths = (double)numPixels * (double)f.samples;
            std::unique_lock<std::mutex> lk(rm);
            while (!reporterStop) {
                if (rcv.wait_for(lk, std::chrono::milliseconds(opt.progress_interval_ms), [&] { return reporterStop; })) break;
                uint64_t done = 0, total = 0;
                if (hrt_multi_progress(multi, &done, &total) != HRT_OK) continue;
                if (done > total) done = total;
                long long px = (long long)((double)numPixels * ((double)pathsBefore.load() + (double)done) / allPaths);
                if (px > numPixels) px = numPixels;
                std::cout << "\rPixels rendered: " << px << "/" << numPixels << std::flush;
            }
        });
    }
    auto stopReporter = [&]() {
        if (!reporter.joinable()) return;
        { std::lock_guard<std::mutex> g(rm); reporterStop = true; }
        rcv.notify_all();
        reporter.join();
    };

    const int R = opt.rows_per_block;
    std::vector<float>& lin = film->linear();     // what the film shows: the preview mean, at the end the final mean
    std::vector<float> sums(lin.size(), 0.0f);     // whole-film accumulation buffer (film order), as gathered on the first device
    auto cleanup = [&]() { stopReporter(); hrt_multi_destroy(multi); };

    int s_done = 0;
    bool have_resume = false;
    if (opt.resume) {
        Checkpoint ck;
        std::string why;
        if (!readCheckpoint(opt.checkpoint, ck, sums, why)) { std::cerr << "\nresume: " << why << std::endl; cleanup(); return HRT_ERR_IO; }
        if (ck.width != f.width || ck.height != f.height || ck.samples != f.samples || ck.seed != opt.seed || ck.quirks != opt.quirks ||
            ck.max_depth != opt.max_depth || ck.next_sample < 0 || ck.next_sample > f.samples || ck.scene_hash != renderHash(flat, cam, opt)) {
            std::cerr << "\nresume: " << opt.checkpoint << " belongs to a different render (scene, camera, film, samples, seed, quirks or depth differ)" << std::endl;
            cleanup();
            return HRT_ERR_INVALID;
        }
        s_done = ck.next_sample;
        pathsBefore.store((long long)numPixels * (long long)s_done);
        have_resume = true;
        std::cout << "\rResumed at sample " << s_done << "/" << f.samples << std::endl;
    }
    // The measured variance (hrt.h hrt_variance_*): the gathered sums are folded on the first device after every pass; without
    // --progressive the render is split into variance_batches passes for it.  Resumed sums are the first batch.
    const bool measure = opt.variance_out != nullptr;
    std::vector<float> vstate;
    int vbatches = 0;
    double vseconds = 0.0;
    auto fold = [&](float scale, int before, int count) -> hrt_status {
        const auto v0 = std::chrono::high_resolution_clock::now();
        if (vstate.empty()) vstate.assign((size_t)numPixels * 2, 0.0f);
        const hrt_status fs = hrt_variance_fold(0, numPixels, sums.data(), scale, before, count, vstate.data());
        vseconds += std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - v0).count();
        if (fs == HRT_OK) ++vbatches;
        else std::cerr << "\nvariance: " << hrt_status_str(fs) << ": " << hrt_last_error() << std::endl;
        return fs;
    };
    if (measure) opt.variance_out->clear();
    if (measure && s_done > 0 && s_done < f.samples && (st = fold(1.0f, 0, s_done)) != HRT_OK) { cleanup(); return st; }
    int pass = opt.pass_samples > 0 ? opt.pass_samples : f.samples;
    if (measure && opt.pass_samples <= 0 && opt.variance_batches > 1) {
        const int K = std::min(opt.variance_batches, f.samples);
        pass = (f.samples + K - 1) / K;
    }
    hrt_stats total{};
    int passes = 0;
    bool resolved = false;
    while (s_done < f.samples && (opt.max_passes <= 0 || passes < opt.max_passes)) {
        ++passes;
        const int n = std::min(pass, f.samples - s_done);
        hrt_stats ps{};
        st = hrt_multi_render(multi, &cam, &pr, R, s_done, n, have_resume ? sums.data() : nullptr, sums.data(), film->getPixels(), &ps);
        have_resume = false;
        if (st != HRT_OK) {
            std::cerr << "\nrender failed: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
            cleanup();
            return st;
        }
        resolved = true;
        addPassStats(total, ps);
        if (measure && (st = fold(s_done + n == f.samples ? static_cast<float>(f.samples) : 1.0f, s_done, n)) != HRT_OK) { cleanup(); return st; }
        s_done += n;
        pathsBefore.store((long long)numPixels * (long long)s_done);
        if (!opt.checkpoint.empty()) {
            Checkpoint ck{f.width, f.height, f.samples, s_done, opt.seed, opt.quirks, opt.max_depth, renderHash(flat, cam, opt)};
            if (!writeCheckpoint(opt.checkpoint, ck, sums)) { std::cerr << "\ncannot write checkpoint " << opt.checkpoint << std::endl; cleanup(); return HRT_ERR_IO; }
        }
        if (s_done < f.samples) {   // preview: mean of the samples so far (the u8 film was resolved on the device)
            const float k = static_cast<float>(s_done);
            for (size_t i = 0; i < lin.size(); ++i) lin[i] = sums[i] / k;
            std::cout << "\rSamples rendered: " << s_done << "/" << f.samples << std::flush;
            if (opt.on_pass) opt.on_pass(s_done);
        }
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    if (render_seconds) *render_seconds = std::chrono::duration<double>(t1 - t0).count() - vseconds;   // (the folds are variance_seconds')
    st = HRT_OK;
    if (s_done >= f.samples && resolved) lin = sums;   // the last pass divided (main.cpp:126): the sums are the means now
    else if (!resolved) {                              // nothing rendered in this call (resume of a stopped render with --max-passes 0 ...)
        hrt_stats none{};
        st = hrt_multi_render(multi, &cam, &pr, R, s_done, 0, have_resume ? sums.data() : nullptr, nullptr, film->getPixels(), &none);
        if (st != HRT_OK) std::cerr << "\nresolve failed: " << hrt_last_error() << std::endl;
        const float k = static_cast<float>(s_done > 0 && s_done < f.samples ? s_done : 1);
        for (size_t i = 0; i < lin.size(); ++i) lin[i] = sums[i] / k;
    }
    if (st == HRT_OK && measure && vbatches >= 2) {   // fewer than two batches: *variance_out stays empty and the caller falls back
        const auto v0 = std::chrono::high_resolution_clock::now();
        opt.variance_out->assign((size_t)numPixels, 0.0f);
        st = hrt_variance_finish(0, numPixels, vstate.data(), s_done, vbatches, opt.variance_out->data());
        vseconds += std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - v0).count();
        if (st != HRT_OK) std::cerr << "\nvariance: " << hrt_status_str(st) << ": " << hrt_last_error() << std::endl;
    }
    if (opt.variance_seconds) *opt.variance_seconds = vseconds;
    if (opt.filter_seconds) {
        double ms = 0.0;
        if (hrt_multi_filter_ms(multi, &ms) == HRT_OK) *opt.filter_seconds = ms * 1e-3;
    }
    stopReporter();
    std::cout << "\rPixels rendered: " << numPixels << "/" << numPixels << std::flush << "\n";
    hrt_multi_destroy(multi);
    if (stats) *stats = total;
    return st;
}

}  // namespace hrthost
