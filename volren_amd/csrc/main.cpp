// main.cpp -- `volren`: the offline (--render) driver of the reference's src/main.cpp on the HIP renderer.
//
// Same command line, same order semantics (src/main.cpp:311-347 for -w/-h, :360-435 for everything else: arguments are
// processed left to right, paths load immediately, later flags override what a loader set), same per-frame loop
// (:524-557): reset -> sppx samples -> tonemap -> "<stem>_%06d.png" in the current directory.
// Not provided: the interactive window/GUI, Python scripts (.py arguments: `python -m volren_amd.run_script` runs them) and the tinycolormap presets.
// Addition: --gpus N [--devices a,b,...] renders every frame on N devices (sharded.h: scene replicated, 16x16 tiles dealt diagonally, one
// grouped ncclAllGather per frame; a device named more than once = logical shards of one GPU, exchanged by device-to-device copies).
// Addition: --denoise keeps the per-pixel variance, runs the feature pass (min(spp, 16) samples) and the a-trous denoiser (vr_denoise.h) after every
// frame and writes the tonemapped denoised frame instead of the raw one (one device only).  --denoise-temporal does the same through
// denoise_temporal (vr_temporal.h): the history is kept across the frames of the run, so every frame after the first is blended with the ones before it.
// --denoise-reject T with it: a pixel whose history disagrees with its frame beyond the noise of the two starts afresh (vr_temporal.h 2a, 3a; refused alone).
// --denoise-moments with it: the filter's variance comes from luminance moments kept in the history (vr_moments.h), for runs of 1 to a few spp per
// frame (refused alone and with --denoise-reject above 0).
// --expected-features N with any of them: the guide is the noise-free expected-value pass of N x N rays per pixel (vr_expected.h; N in 1..4) instead of
// the sampled feature pass (refused without a denoise flag).
// --resolve with --expected-features N, N >= 2: the frame's hit/miss noise is replaced by the expected coverage of that pass (vr_resolve.h).  Alone it writes the
// tonemapped resolved frame; with --denoise / --denoise-temporal the filter starts from the resolved frame ("denoise_resolve" = 1).  One device only.
// --denoise-layers with --denoise / --denoise-temporal and --expected-features N, N >= 2: the filter runs on the scattered layer alone and the analytic
// background is put back afterwards ("denoise_layers" = 1, vr_layers.h); refused without them.
// --denoise-filter 0|1 and --denoise-ridge X with --denoise-layers: 1 runs one pass of local regression on the scattered layer in the place of the a-trous
// iterations ("denoise_filter" = 1, vr_regress.h), X is the ridge on its slopes ("denoise_ridge": 0 = zero order, or in [2^-20, 2^20]); refused without it.
// --denoise-demodulate with --denoise-layers: the scattered layer is divided by the guide's albedo in front of the filter and multiplied back behind it
// ("denoise_demodulate" = 1, vr_demod.h), and so is the layer --upsample rebuilds; refused without it.
// --upsample F (2..4) with --denoise-layers (and so with a denoise flag and --expected-features N): the frame is rendered and filtered at -w x -h, its layer is
// rebuilt at F times that size per axis under an expected-value guide of N rays at the large size (vr_upsample.h), and the tonemapped F w x F h frame is
// written; refused alone.
// --expected-skip 0|1 with --expected-features: whether that pass skips empty space by the clear-distance table (default 1; the frame is the same either
// way; refused without --expected-features).
// --expected-field 0|1 with --expected-features: which field that pass marches -- 0 the trilinear one (default), 1 the tracker's (without a LUT the cubic
// B-spline field of vr_cubic.h; with one the trilinear field, the same frame); refused without --expected-features.
// Addition: --adaptive T renders every frame with adaptive sampling per 16x16 tile (render_adaptive(min(16, spp), spp, T): vr_adaptive.h) and logs
// the mean samples per pixel; combines with --denoise (one device only).
//
//   volren data/smoke.brick data/table_mountain_2_puresky_1k.hdr -w 1024 -h 1024 --render --spp 4096 --bounces 128 \
//          --albedo 0.8 --phase 0.3 --density 100 --env_strength 3 --env_rot 270 --exposure 3 --gamma 2.0 --cam_fov 40
#include <sys/wait.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <filesystem>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "imageio.h"
#include "renderer.h"
#include "sharded.h"

namespace fs = std::filesystem;
using namespace vr;

static std::shared_ptr<RendererHIP> renderer;
static std::string out_filename = "output.png";

// A path on the command line is loaded the moment it is seen (src/main.cpp:37-81, 428-432): ".hdr" replaces the environment, ".txt" binds a
// transfer function and hides the environment, anything else is a volume file or a folder of animation frames -- which also resets the density
// scale, fits the volume into the unit cube and commits it.  Every kind restarts the accumulation; a loader that throws is reported on stderr
// with the reference's wording and the render goes on with what was loaded before (the reference's catch blocks).
struct PathKind {
    const char* ext;       // file extension, or nullptr for "everything else"
    const char* what;      // the noun of the reference's message: "Unable to load <what> from <path>: ..."
    void (*load)(const std::string& path);
};
static const PathKind kPathKinds[] = {
    { ".hdr", "envmap", [](const std::string& path) { renderer->environment = std::make_shared<Environment>(path); } },
    { ".txt", "transferfunc", [](const std::string& path) {
          renderer->transferfunc = std::make_shared<TransferFunction>(path);
          renderer->show_environment = false;
      } },
    { nullptr, "volume", [](const std::string& path) {
          std::cout << "load volume: " << path << std::endl;
          renderer->volume = fs::is_directory(path) ? Volume::load_folder(path) : std::make_shared<Volume>(path);
          renderer->density_scale = 1.f;
          renderer->scale_and_move_to_unit_cube();
          renderer->commit();
      } },
};
static void handle_path(const std::string& path) {
    const std::string ext = fs::path(path).extension().string();
    if (ext == ".py") return;                               // main() hands the whole command line to python -m volren_amd.run_script before anything else
    for (const PathKind& kind : kPathKinds) {
        if (kind.ext && ext != kind.ext) continue;
        try {
            kind.load(path);
            renderer->sample = 0;
        } catch (const std::exception& e) {
            std::cerr << "Unable to load " << kind.what << " from " << path << ": " << e.what() << std::endl;
        }
        return;
    }
}

struct Args {
    int argc; char** argv; int i;
    bool has(int n) const { return i + n < argc; }
    std::string next() { if (i + 1 >= argc) throw std::runtime_error(std::string("missing value after ") + argv[i]); return argv[++i]; }
    float nextf() { return std::stof(next()); }
    int nexti() { return std::stoi(next()); }
};

static void parse_cmd(int argc, char** argv) {
    Args a{ argc, argv, 0 };
    for (a.i = 1; a.i < argc; ++a.i) {
        const std::string arg = argv[a.i];
        if (arg == "--render" || arg == "--denoise" || arg == "--denoise-temporal" || arg == "--denoise-moments" || arg == "--denoise-layers" || arg == "--denoise-demodulate" || arg == "--resolve") {      // --denoise*, --adaptive: main()
        } else if (arg == "-w" || arg == "-h" || arg == "--title" || arg == "--major" || arg == "--minor" || arg == "--swap" || arg == "--font" || arg == "--fontsize") {
            a.next();                                           // consumed by the context set-up pass
        } else if (arg == "--upsample" || arg == "--denoise-filter" || arg == "--denoise-ridge") {
            a.next();                                           // main()
        } else if (arg == "--no-resize" || arg == "--hidden" || arg == "--no-decoration" || arg == "--floating" || arg == "--maximised" || arg == "---debug") {
        } else if (arg == "--output") out_filename = a.next();
        else if (arg == "--samples" || arg == "--spp" || arg == "--sppx") renderer->sppx = a.nexti();
        else if (arg == "--bounces") renderer->bounces = a.nexti();
        else if (arg == "--albedo") renderer->albedo = vec3(a.nextf());
        else if (arg == "--density") renderer->density_scale = a.nextf();       // SETS (after load_volume multiplied it)
        else if (arg == "--emission") renderer->emission_scale = a.nextf();
        else if (arg == "--phase") renderer->phase = a.nextf();
        else if (arg == "--env_strength") renderer->environment->strength = a.nextf();
        else if (arg == "--env_rot") renderer->environment->transform = rotation_axis(a.nextf(), 1);
        else if (arg == "--env_hide") renderer->show_environment = false;
        else if (arg == "--fau") {
            renderer->transferfunc = std::make_shared<TransferFunction>(std::vector<vec4>({ vec4(0, 0, 0, 0), vec4(4 / 255.f, 49 / 255.f, 106 / 255.f, 0.33f),
                                                                                          vec4(38 / 255.f, 97 / 255.f, 65 / 255.f, 0.66f), vec4(151 / 255.f, 27 / 255.f, 47 / 255.f, 1.f) }));
        } else if (arg == "--turbo" || arg == "--viridis") {
            std::cerr << arg << ": tinycolormap presets are not part of this build" << std::endl;
        // src/main.cpp:397-402: the value is only consumed when a transfer function exists; without one it stays behind as an argument of its own
        // (not a flag, not a file: ignored)
        } else if (arg == "--tf_left") { if (renderer->transferfunc) renderer->transferfunc->window_left = a.nextf(); }
        else if (arg == "--tf_width") { if (renderer->transferfunc) renderer->transferfunc->window_width = a.nextf(); }
        else if (arg == "--cam_pos") { renderer->camera.pos.x = a.nextf(); renderer->camera.pos.y = a.nextf(); renderer->camera.pos.z = a.nextf(); }
        else if (arg == "--cam_dir") { renderer->camera.dir.x = a.nextf(); renderer->camera.dir.y = a.nextf(); renderer->camera.dir.z = a.nextf(); }
        else if (arg == "--cam_fov") renderer->camera.fov_degree = a.nextf();
        else if (arg == "--exposure") renderer->tonemap_exposure = a.nextf();
        else if (arg == "--gamma") renderer->tonemap_gamma = a.nextf();
        else if (arg == "--vol_rot_x" || arg == "--vol_rot_y" || arg == "--vol_rot_z") {
            // glm::mat3(glm::rotate(mat4(volume->transform), angle, axis)): the translation is dropped (reference quirk, main.cpp:417-422)
            const int axis = arg.back() - 'x';
            const mat4 r = from3(rotation_axis(a.nextf(), axis));
            renderer->volume->transform = from3(upper3(renderer->volume->transform * r));
        } else if (arg == "--vol_crop_min") { renderer->vol_clip_min.x = a.nextf(); renderer->vol_clip_min.y = a.nextf(); renderer->vol_clip_min.z = a.nextf(); }
        else if (arg == "--vol_crop_max") { renderer->vol_clip_max.x = a.nextf(); renderer->vol_clip_max.y = a.nextf(); renderer->vol_clip_max.z = a.nextf(); }
        else if (arg == "--seed") renderer->seed = a.nexti();                        // addition
        else if (arg == "--device" || arg == "--gpus" || arg == "--devices" || arg == "--adaptive" || arg == "--denoise-reject" || arg == "--expected-features" || arg == "--expected-skip" || arg == "--expected-field") a.next();  // consumed earlier
        else if (fs::is_regular_file(arg) || fs::is_directory(arg)) handle_path(arg);
    }
}

static std::vector<int> parse_int_list(const std::string& s) {
    std::vector<int> v;
    size_t pos = 0;
    while (pos <= s.size()) {
        const size_t c = s.find(',', pos);
        const std::string tok = s.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
        if (!tok.empty()) v.push_back(std::stoi(tok));
        if (c == std::string::npos) break;
        pos = c + 1;
    }
    return v;
}

// `volren script.py --render -w W -h H` (src/main.cpp:83-91 embeds CPython and evaluates the file): this build starts an ordinary interpreter on
// volren_amd.run_script, which makes `import volpy` resolve to the HIP-backed module and gives `volpy.Renderer()` the -w / -h resolution.  Done before
// this process has touched the GPU; the interpreter is a child, its exit status is ours.
static int run_python_script(int argc, char** argv) {
    std::error_code ec;
    const fs::path exe = fs::read_symlink("/proc/self/exe", ec);
    const std::string root = ec ? std::string(".") : exe.parent_path().parent_path().string();      // <root>/volren_amd/volren
    std::string cmd = "PYTHONPATH='" + root + "'${PYTHONPATH:+:$PYTHONPATH} python3 -m volren_amd.run_script";
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i], q = "'";
        for (char c : a) { if (c == '\'') q += "'\\''"; else q += c; }
        cmd += " " + q + "'";
    }
    const int rc = std::system(cmd.c_str());
    return rc == -1 ? 1 : (WIFEXITED(rc) ? WEXITSTATUS(rc) : 1);
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg.size() > 3 && arg.compare(arg.size() - 3, 3, ".py") == 0 && fs::is_regular_file(arg)) return run_python_script(argc, argv);
    }
    int width = 1280, height = 720, device = 0, gpus = 0;        // cppgl ContextParameters defaults (unverified): always pass -w/-h
    bool denoise = false, temporal = false, adaptive = false;      // temporal: --denoise with the history kept across the frames of the run
    float threshold = 0.f, reject = 0.f;      // reject: --denoise-reject, the history rejection threshold of --denoise-temporal (0 = off)
    int expected_rays = 0;      // --expected-features N: the denoise flags take their guide from render_features_expected(N) instead of render_features(min(spp, 16))
    int expected_skip = -1;     // --expected-skip 0|1 (with --expected-features): whether that pass drops the steps of empty space (same frame either way); -1: the renderer's default
    int expected_field = -1;    // --expected-field 0|1 (with --expected-features): the field that pass marches, 1 = the tracker's; -1: the renderer's default
    bool resolve = false;       // --resolve (with --expected-features N >= 2): the control variate on the expected coverage, alone or in front of the filter
    bool layers = false;        // --denoise-layers (with a denoise flag and --expected-features N >= 2): the filter runs on the scattered layer alone ("denoise_layers" = 1, vr_layers.h)
    bool demodulate = false;    // --denoise-demodulate (with --denoise-layers): the layer is filtered divided by the guide's albedo ("denoise_demodulate" = 1, vr_demod.h)
    int filter = -1;            // --denoise-filter 0|1 (with --denoise-layers): one pass of local regression in the iterations' place (vr_regress.h); -1: not given
    float ridge = -1.f;         // --denoise-ridge X (with --denoise-layers): the ridge of that regression; -1: not given, the renderer's default
    int upsample = 0;           // --upsample F (with --denoise-layers): the frame written is F times -w x -h, rebuilt from the filtered layer (vr_upsample.h); 0: off
    bool reject_given = false, moments = false;      // moments: --denoise-moments, the filter's variance from the history's luminance moments (low-spp sequences)
    std::vector<int> devices;
    try {
        for (int i = 1; i < argc; ++i) {
            const std::string arg = argv[i];
            if (arg == "-w" && i + 1 < argc) width = std::stoi(argv[++i]);
            else if (arg == "-h" && i + 1 < argc) height = std::stoi(argv[++i]);
            else if (arg == "--device" && i + 1 < argc) device = std::stoi(argv[++i]);
            else if (arg == "--gpus" && i + 1 < argc) gpus = std::stoi(argv[++i]);
            else if (arg == "--devices" && i + 1 < argc) devices = parse_int_list(argv[++i]);
            else if (arg == "--denoise") denoise = true;
            else if (arg == "--denoise-temporal") denoise = temporal = true;
            else if (arg == "--denoise-moments") moments = true;
            else if (arg == "--denoise-layers") layers = true;
            else if (arg == "--denoise-demodulate") demodulate = true;
            else if (arg == "--resolve") resolve = true;
            else if (arg == "--denoise-reject") {
                if (i + 1 >= argc) throw std::runtime_error("missing value after --denoise-reject");
                reject_given = true;
                reject = std::stof(argv[++i]);
                if (!(reject == 0.f || (reject >= kTemporalRejectMin && reject <= kTemporalRejectMax)))
                    throw std::runtime_error("--denoise-reject: the threshold must be 0 (off) or in [2^-10, 2^20]");
            } else if (arg == "--expected-features") {
                if (i + 1 >= argc) throw std::runtime_error("missing value after --expected-features");
                expected_rays = std::stoi(argv[++i]);
                if (expected_rays < 1 || expected_rays > kExpectedMaxRays) throw std::runtime_error("--expected-features: the rays per pixel axis must be 1..4");
            } else if (arg == "--denoise-filter") {
                if (i + 1 >= argc) throw std::runtime_error("missing value after --denoise-filter");
                const std::string v = argv[++i];
                if (v != "0" && v != "1") throw std::runtime_error("--denoise-filter: 0 (the a-trous iterations) or 1 (one pass of local regression)");
                filter = v == "1" ? 1 : 0;
            } else if (arg == "--denoise-ridge") {
                if (i + 1 >= argc) throw std::runtime_error("missing value after --denoise-ridge");
                ridge = std::stof(argv[++i]);
                if (!regress_ridge_ok(ridge)) throw std::runtime_error("--denoise-ridge: the ridge must be 0 (zero order) or in [2^-20, 2^20]");
            } else if (arg == "--upsample") {
                if (i + 1 >= argc) throw std::runtime_error("missing value after --upsample");
                upsample = std::stoi(argv[++i]);
                if (upsample < 2 || upsample > 4) throw std::runtime_error("--upsample: the factor per axis must be 2..4");
            } else if (arg == "--expected-skip") {
                if (i + 1 >= argc) throw std::runtime_error("missing value after --expected-skip");
                const std::string v = argv[++i];
                if (v != "0" && v != "1") throw std::runtime_error("--expected-skip: 0 (march every step) or 1 (skip empty space)");
                expected_skip = v == "1" ? 1 : 0;
            } else if (arg == "--expected-field") {
                if (i + 1 >= argc) throw std::runtime_error("missing value after --expected-field");
                const std::string v = argv[++i];
                if (v != "0" && v != "1") throw std::runtime_error("--expected-field: 0 (the trilinear field) or 1 (the tracker's field)");
                expected_field = v == "1" ? 1 : 0;
            } else if (arg == "--adaptive") {
                if (i + 1 >= argc) throw std::runtime_error("missing value after --adaptive");
                adaptive = true;
                threshold = std::stof(argv[++i]);
                if (!(threshold >= 0.f) || !std::isfinite(threshold)) throw std::runtime_error("--adaptive: the threshold must be finite and >= 0");
            }
        }
        if (reject_given && !temporal) throw std::runtime_error("--denoise-reject needs --denoise-temporal: it rejects the history that only that call keeps");
        if (resolve && expected_rays == 0) throw std::runtime_error("--resolve needs --expected-features N with N >= 2: the expected coverage of that pass is what replaces the frame's");
        if (resolve && expected_rays < 2) throw std::runtime_error("--resolve needs --expected-features N with N >= 2: one ray gives the coverage of the pixel's centre, not of its area");
        if (layers && !denoise) throw std::runtime_error("--denoise-layers needs --denoise or --denoise-temporal: it is a setting of their filter");
        if (layers && expected_rays < 2) throw std::runtime_error("--denoise-layers needs --expected-features N with N >= 2: the expected coverage of that pass splits the frame into background and scattered layer");
        if (demodulate && !layers) throw std::runtime_error("--denoise-demodulate needs --denoise-layers: the albedo divides the scattered layer");
        if (filter >= 0 && !layers) throw std::runtime_error("--denoise-filter needs --denoise-layers: the regression is defined on the scattered layer");
        if (ridge >= 0.f && !layers) throw std::runtime_error("--denoise-ridge needs --denoise-layers: it is a setting of the regression on the scattered layer");
        if (upsample > 0 && !layers) throw std::runtime_error("--upsample needs --denoise-layers: the filtered scattered layer is what it upsamples");
        if (expected_rays > 0 && !denoise && !resolve) throw std::runtime_error("--expected-features needs --denoise, --denoise-temporal or --resolve: it chooses the guide of their filter");
        if (expected_skip >= 0 && expected_rays == 0) throw std::runtime_error("--expected-skip needs --expected-features: it is a setting of that pass");
        if (expected_field >= 0 && expected_rays == 0) throw std::runtime_error("--expected-field needs --expected-features: it is a setting of that pass");
        if (moments && !temporal) throw std::runtime_error("--denoise-moments needs --denoise-temporal: the moments live in the history that only that call keeps");
        if (moments && reject > 0.f) throw std::runtime_error("--denoise-moments and --denoise-reject do not go together: the rejection statistic needs the frames' sample variance");
        if (adaptive && (gpus > 0 || devices.size() > 1))
            throw std::runtime_error("--adaptive renders on one device only: drop --gpus / --devices (the sharded renderer has no adaptive sampling)");
        if (resolve && (gpus > 0 || devices.size() > 1)) throw std::runtime_error("--resolve renders on one device only: drop --gpus / --devices");
        if (denoise && (gpus > 0 || devices.size() > 1))
            throw std::runtime_error(std::string(temporal ? "--denoise-temporal" : "--denoise") + " renders on one device only: drop --gpus / --devices (the sharded renderer has no denoiser)");
        // one renderer per part; without --gpus / --devices: one part on --device, the reference's single-context loop
        if (devices.empty()) {
            if (gpus <= 1) devices = { device };
            else for (int d = 0; d < gpus; ++d) devices.push_back(d);
        } else if (gpus > 0 && (size_t)gpus != devices.size()) throw std::runtime_error("--gpus and --devices disagree");
        const bool sharded = devices.size() > 1 || gpus > 0;
        std::vector<std::shared_ptr<RendererHIP>> parts;
        for (size_t k = 0; k < devices.size(); ++k) {
            // the scene is replicated by running the command line once per part (paths load onto the part's device)
            VR_HIP(hipSetDevice(devices[k]));
            renderer = std::make_shared<RendererHIP>();
            renderer->resolution = { width, height };
            renderer->init();
            parse_cmd(argc, argv);
            if (renderer->volume->grids.empty()) {
                // debug box of the reference (main.cpp:465-474): a 1x1x4 dense grid in front of the camera
                const float values[4] = { 1.f, 2.5f, 5.f, 10.f };
                auto box = std::make_shared<DenseGrid>(1, 1, 4, values);
                const vec3 d = renderer->camera.dir;
                box->transform = scale_then_translate(1.f, vec3(2.f * d.x + 0.f, 2.f * d.y - 0.5f, 2.f * d.z - 2.f));
                renderer->volume = std::make_shared<Volume>(box);
                renderer->commit();
            }
            renderer->reset();
            if (denoise) renderer->variance = 1;        // the denoiser's variance input: kept from sample 1 of every frame
            renderer->denoise_reject = reject;
            renderer->denoise_moments = moments ? 1 : 0;
            renderer->denoise_resolve = resolve && denoise ? 1 : 0;
            renderer->denoise_layers = layers ? 1 : 0;
            renderer->denoise_demodulate = demodulate ? 1 : 0;
            if (filter >= 0) renderer->set_denoise_filter(filter);
            if (ridge >= 0.f) renderer->set_denoise_ridge(ridge);
            if (expected_skip >= 0) renderer->expected_skip = expected_skip;
            if (expected_field >= 0) renderer->expected_field = expected_field;
            parts.push_back(renderer);
        }
        renderer = parts[0];                            // holds the whole frame after the gather
        std::unique_ptr<ShardedRenderer> shards;
        if (sharded) {
            std::vector<RendererHIP*> raw;
            for (auto& p : parts) raw.push_back(p.get());
            shards = std::make_unique<ShardedRenderer>(raw, devices);
            std::cout << "rendering on " << devices.size() << " part(s), devices";
            for (int d : devices) std::cout << " " << d;
            std::cout << ", tile exchange: " << shards->transport() << std::endl;
        }
        std::cout << "rendering..." << std::endl;
        for (size_t i = 0; i < renderer->volume->n_grid_frames(); ++i) {
            for (auto& p : parts) { p->reset(); p->volume->grid_frame_counter = i; }
            const auto t0 = std::chrono::steady_clock::now();
            if (shards) {
                shards->render(renderer->sppx);
                shards->synchronize();
            } else if (adaptive) {
                renderer->render_adaptive(std::min(16, renderer->sppx), renderer->sppx, threshold);
                renderer->synchronize();
                if (renderer->watchdog_status()) throw std::runtime_error("path-tracing kernel watchdog tripped");
            } else {
                renderer->render(renderer->sppx);          // == while (sample < sppx) trace();
                renderer->synchronize();
                if (renderer->watchdog_status()) throw std::runtime_error("path-tracing kernel watchdog tripped");
            }
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (adaptive) {
                const std::vector<int32_t> n = renderer->tile_samples();
                double px_samples = 0.0;                   // partial edge tiles count their pixels inside the frame
                const int tiles_x = vr::tiles_x(width);
                for (size_t t = 0; t < n.size(); ++t) {
                    const int tx = (int)(t % tiles_x), ty = (int)(t / tiles_x);
                    px_samples += (double)n[t] * std::min(16, width - 16 * tx) * std::min(16, height - 16 * ty);
                }
                std::cout << "adaptive: " << px_samples / ((double)width * height) << " spp mean, " << renderer->sample << " max / " << renderer->sppx
                          << ", " << renderer->adaptive_rounds << " rounds  (" << sec << " s, " << px_samples / sec / 1e6 << " Msamples/s)" << std::endl;
            } else {
                std::cout << renderer->sample << " / " << renderer->sppx << "  (" << sec << " s, "
                          << (double)width * height * renderer->sppx / sec / 1e6 << " Msamples/s)" << std::endl;
            }
            VR_HIP(hipSetDevice(devices[0]));
            renderer->tonemapping = true;               // the offline loop always tonemaps (main.cpp:540-550)
            if (denoise) {
                if (expected_rays > 0) renderer->render_features_expected(expected_rays);
                else renderer->render_features(std::min(renderer->sppx, 16));
                if (temporal) renderer->denoise_temporal();      // the first frame: what denoise() gives
                else renderer->denoise();
                renderer->synchronize();
                if (renderer->watchdog_status()) throw std::runtime_error("feature pass: a camera segment exceeded its step budget");
                if (upsample > 0) {
                    renderer->upsample(upsample, expected_rays);
                    renderer->synchronize();
                }
                renderer->draw_from(upsample > 0 ? *renderer->upsampled() : *renderer->denoised());
            } else if (resolve) {
                renderer->render_features_expected(expected_rays);
                renderer->resolve();
                renderer->synchronize();
                renderer->draw_from(*renderer->resolved());
            } else {
                renderer->draw();
            }
            const int out_w = upsample > 0 ? upsample * width : width, out_h = upsample > 0 ? upsample * height : height;
            std::vector<float> fb((size_t)out_w * out_h * 4);
            renderer->download_display(fb.data());
            std::vector<uint8_t> rgba;
            framebuffer_to_rgba8(fb.data(), out_w, out_h, rgba);
            char num[16];
            snprintf(num, sizeof num, "%06zu", i);
            const std::string out_fn = fs::path(out_filename).stem().string() + "_" + num + ".png";   // directory of --output is dropped (reference quirk)
            save_png_rgba8(out_fn, rgba.data(), out_w, out_h);
            std::cout << out_fn << " written." << std::endl;
        }
        shards.reset();                                 // before the parts it points at
    } catch (std::exception& e) {
        std::cerr << "volren: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
