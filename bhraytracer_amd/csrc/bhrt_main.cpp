// bhrt_main.cpp — C++ host program above the C ABI: the headless equivalent of the reference's main()
// (Main.cpp:418-431: LoadScene -> ShowViewport -> BeginRender -> SaveImages; the seam viewport.cpp:425-449 calls BeginRender
// synchronously), with the reference's compile-time constants (scene path Main.cpp:423, output path Main.cpp:416, PT_SampleCount
// :141, GIBounceCount :130, INTERNAL_REFLECTION_BOUNCE :41) as command-line options.
//
//   bhrt render <scene.xml> [-o out.png] [--spp N] [--gi N] [--bounces N] [--seed S] [--no-jitter] [--no-gamma]
//               [--device D | --gpus N [--rehearse]] [--rank R --world N] [--tile T] [--radiance out.f32] [--leaf-skip] [--photon-exact]
//               [--photons N] [--photon-file map.dat] [--photon-out map.dat]     (USE_PhotonMap, Main.cpp:51,53,194,383)
//               [--denoise [--denoise-iters K] [--guide-spp N [--coverage-filter [--sigma-coverage X]]]]  (DenoiseImage of the x64 build, Main.cpp:57-96,236-238)
//               [--adaptive [--spp-min N] [--adaptive-threshold X] [--samples-png path]]  (RenderImage::sampleCount, scene.h:534,603-630)
//               [--lens [--dof R] [--focaldist D]]                               (the viewport's depth of field, viewport.cpp:236-243, rendered)
//               [--emission]                                                     (the <emission> of the materials, xmlload.cpp:344-348, shaded)
//               [--face-materials]                                               (the .mtl sub-material of each mesh face, viewport.cpp:581-607, rendered)
//               [--global-map N [--global-radius R]]                             (BuildPhotonMap, Main.cpp:196,251-317, gathered where the GI recursion ends)
//               [--progressive N [--time-limit SECONDS] [--live-png path]]       (BeginRender .. StopRender, Main.cpp:178,243: the frame in steps)
//               [--camera-pos X,Y,Z] [--camera-target X,Y,Z] [--camera-up X,Y,Z] [--fov F]   (the <camera> tags, xmlload.cpp:109-127, replaced)
//               [--shutter-pos X,Y,Z] [--shutter-target X,Y,Z] [--shutter-up X,Y,Z]           (camera motion blur: the camera at the end of the exposure)
//               [--temporal N [--to-pos X,Y,Z] [--to-target X,Y,Z] [--to-up X,Y,Z] [--node-to-translate NAME:X,Y,Z] [--light-to-pos NAME:X,Y,Z] [--frames-png PREFIX]   (N frames along a camera, object or light move, each carried into the next)
//                   [--denoise [--denoise-iters K]   (each frame written denoised with its carried variance)
//                       [--spatial-variance [--variance-radius R] [--variance-min-length X]]   (the variance of a short history estimated from its neighbourhood)
//                       [--reject-change [--change-radius R] [--change-sigma LO,HI]]]]   (history dropped where a surface's light changed)
//               [--node-translate NAME:X,Y,Z]   (repeatable: one translate op on that node before anything is rendered)
//               [--light-pos NAME:X,Y,Z] [--light-dir NAME:X,Y,Z] [--light-intensity NAME:R,G,B] [--light-size NAME:S]   (repeatable: that <light> edited before anything is rendered)
//   bhrt info   <scene.xml>
//
// --gpus N: ONE process drives N GPUs of the node (the reference's one process drives 16 OpenMP threads, Main.cpp:422): the
// image is cut into interleaved tile x tile squares (tile t -> GPU t mod N), one host thread per GPU calls
// bhrt_render_dev for its tiles, packs them (bhrt_tiles_pack_dev), ONE ncclAllGather over the RCCL communicator of the N devices
// (xGMI) moves every GPU's block to all of them, bhrt_tiles_unpack_dev rebuilds the frame, GPU 0's copy is saved.  The caustic
// photon map is emitted in disjoint emission-index ranges on the N GPUs (bhrt_photon_emit_range) and installed on every one
// (bhrt_photon_install): the same map as on one GPU.  --gpus 1 runs the same code over a one-device communicator.
// --gpus N --rehearse: the same N threads, rendezvous points, per-rank renders, packs and unpacks with every rank on device 0 and the
// ncclAllGather replaced by N device-to-device copies — what a one-GPU box can run of the N > 1 control flow (tests/test_cli.py).
// Without --gpus: one device, no RCCL involved (--rank / --world then render that rank's tiles only, for process-per-GPU launchers).
// --denoise: the PNG is the denoised frame (bhrt_denoise, as the reference's 64-bit build saves it); --radiance stays the render's own
// radiance.  With --gpus N the ranks' variance tiles travel in a second block beside the first and GPU 0 denoises the gathered frame; a
// partial frame (--world > 1) cannot be denoised.
// --guide-spp N (needs --denoise; without it a usage error): the filter's guides (depth, normal, albedo) are bhrt_guides' at N samples per pixel with
// the render's seed, jitter and lens: averaged over the pixel footprint the colour image is averaged over.  0, the default: the
// guides the denoiser computes itself, the pinhole ray through the pixel corner.  With --gpus N the guides are computed where the denoiser runs,
// on GPU 0 for the whole frame.
// --coverage-filter (needs --denoise and --guide-spp N > 0; without them a usage error): the filter is bhrt_denoise_sampled, which
// also takes bhrt_guides' coverage image: demodulation by albedo + (1 - coverage), normals compared by direction, coverage as a weight of its own.
// --sigma-coverage X (finite, >= 0; needs --coverage-filter): its coverage tolerance, default BHRT_DENOISE_SIGMA_COVERAGE.  With --gpus N on GPU 0,
// as --guide-spp.  Without the flag --guide-spp hands its three images to bhrt_denoise as before.
// --adaptive: bhrt_render_adaptive; --spp is the per-pixel maximum, --spp-min round 0's samples.  --samples-png writes the
// sample-count image as SaveSampleCountImage does (scene.h:630); its normalisation needs the whole frame, so --world > 1 refuses it.  With
// --gpus N the counts travel as the float section of a further block (exact below 2^24); with --denoise the adaptive variance is the filter's.
// --lens: bhrt_opts.lens = 1, a thin-lens camera with the scene's <dof> as aperture radius, focused at <focaldist>.  --dof R and
// --focaldist D replace the scene's values (bhrt_scene_set_lens, before the upload) and imply --lens.  The option travels in bhrt_opts, so it
// works with --gpus, --adaptive and --denoise; the denoiser's guides stay those of the pinhole ray unless --guide-spp asks for sampled ones.
// --emission: bhrt_scene_set_emissive(scene, 1) before the upload and before --gpus N clones the scene: every Shade() frame of a Blinn
// material adds its <emission> last.  Scene state, so it reaches every render the other options choose (--gpus, --rehearse, --denoise, --adaptive,
// --lens); the denoiser's albedo guide stays the diffuse colour.  Without the flag the frame is the reference's, which never shades <emission>.
// --face-materials: bhrt_scene_set_face_materials(scene, 1) before the upload and before --gpus N clones the scene: a mesh with a .mtl
// shades every face with its own sub-material.  Scene state, so it reaches every render the other options choose (--gpus, --rehearse, --denoise,
// --adaptive, --lens, --emission), the denoiser's albedo guide included.  Without the flag the frame is the reference's: sub-material 0 everywhere.
// --global-map N: bhrt_scene_set_global_gather(scene, 1, R) before --gpus N clones the scene, and bhrt_global_map_build with the render's seed on every
// device once its scene is uploaded: a Shade() frame whose GI term is cut by the bounce budget gathers it from the global photon
// map (radius R, default the reference's 0.5).  With --gpus K every rank builds the whole map itself: the emission is keyed, so the bytes are
// the same on every rank.  Independent of --photons; --photon-exact selects the heavy-query path of both gathers.
// --progressive N: the frame as a session (bhrt_progressive_*): steps of N samples per pixel up to --spp, one line per step
// (step, samples per pixel min / max, active pixels, seconds since the first step began).  --live-png is written whole after each step (a
// temporary file beside it, renamed over it): what a viewport would show.  --time-limit stops after the first step that ends beyond the
// limit; at least one step always runs; the final PNG is the frame at that moment.  --adaptive becomes the session's retirement test
// (--samples-png works), --denoise filters the final frame once, and the scene options (--lens, --emission, --face-materials, --global-map,
// --photons) apply as they do to a blocking render.  One device: with --gpus N > 1 a usage error (no tile exchange per step yet).
// --camera-pos / --camera-target / --camera-up / --fov: bhrt_scene_set_camera before the upload and before --gpus N clones the scene.
// Each is optional; a missing one is read from the scene: its position, the point it looks at on the plane of focus (pos + dir * focaldist), its
// up vector, its fov.  --shutter-pos / --shutter-target / --shutter-up: any of them turns the camera shutter on (bhrt_scene_set_shutter): the
// camera moves from the scene's pose (after the camera flags) to this one during the exposure, every sample at a time of its own; a missing one
// is taken from pose 0.  Scene state, so it reaches every render the other options choose, --guide-spp's guides included.  A malformed value is a
// usage error before the scene is loaded; poses the library refuses (a quarter turn or more apart, up along the view) fail with its message.
// Off unless asked for: without the flags the frame is the scene file's pinhole or lens frame.
// --temporal N (N >= 2): temporal reprojection.  N frames of --spp samples each, frame k with seed --seed + k and the camera
//     X_k = X0 + (X1 - X0) * ((float)k / (float)(N - 1))      per component, in float32, for X = position, target, up
// set through bhrt_scene_set_camera; pose 0 is the scene's camera (after the camera flags; a missing value as --camera-* reads it), pose 1 the
// --to-* values, a missing one taken from pose 0.  Frame 0 is its render; frame k + 1 is its render blended (bhrt_temporal_accumulate) into
// frame k's accumulated output and length reprojected into its view (bhrt_reproject with both views' first hits, albedo included), with the
// library's default options.  -o gets the last frame, --frames-png PREFIX every frame as PREFIX000.png, PREFIX001.png, ...; --radiance the last
// frame's accumulated radiance.  One device, whole frames: with --progressive, --adaptive, --gpus or --world > 1,
// with N < 2, or --to-* / --frames-png without --temporal: a usage error.  The loop is a temporal session (bhrt_temporal_begin / _frame / _end,
// DESIGN.md 23): the setters, then one call per frame; the stages named here and below are the session's, on images that stay on the device.
// --temporal N --denoise [--denoise-iters K]: every frame is rendered with bhrt_render_var, reprojected with bhrt_reproject_var
// (with the node snapshot and id images under --node-to-translate) and accumulated with bhrt_temporal_accumulate_var, and what is written is
// bhrt_denoise(accumulated frame, its carried variance, this view's first hit).  The next frame gets the un-denoised accumulated frame and its
// variance: the denoised image is for display and is never fed back.  Needs --spp >= 2 (a 1-spp frame has no variance); --guide-spp and
// --coverage-filter beside it are usage errors (sampled guides are not carried).  Without --denoise the calls are those named above.
// --spatial-variance [--variance-radius R] [--variance-min-length X] (needs --temporal N --denoise; anywhere else, and R or X without the flag, a
// usage error): --spp 1 becomes legal, and there the current frame's variance, for every pixel, is bhrt_variance_spatial's estimate
// of the rendered frame (no variance or length image) in the place of bhrt_render_var's zeros.  At every --spp the variance bhrt_denoise gets is
// bhrt_variance_spatial(accumulated frame, its carried variance, its length): a pixel with fewer than X samples behind it (default 4 x spp: four
// frames) is filtered with the estimate from its (2R + 1)^2 neighbourhood (R in 1..4, default 3), the others with their carried variance.  The
// next frame gets the un-denoised accumulated frame and its carried variance, unmodified.  Without the flag every command line behaves as before.
// --reject-change [--change-radius R] [--change-sigma LO,HI] (needs --temporal N --denoise; anywhere else, and R or LO,HI without the flag, a usage
// error): bhrt_temporal_set_change on the session with the library's defaults, R (1..4) and the two thresholds (finite, 0 <= LO <= HI)
// replacing theirs: from frame 1 on bhrt_temporal_change shortens the reprojected length where history and current frame differ by more than
// their noise, before bhrt_temporal_accumulate_var reads it.  Without the flag every command line behaves as before.
// --node-translate NAME:X,Y,Z (repeatable, any mode): one translate op appended to the node of that <object name=> through
// bhrt_scene_set_node_transform, before anything is rendered.  --node-to-translate NAME:X,Y,Z (repeatable, needs --temporal N): frame k sets the
// node to the record it had before frame 0 plus a translate of delta * ((float)k / (float)(N - 1)) per component in float32, and frames are
// reprojected with bhrt_reproject_moving from the previous frame's node snapshot, id image (bhrt_first_hit_node) and accumulated output; without
// --to-* the camera stays.  An unknown name, a malformed value, or --node-to-translate without --temporal: a usage error before any device is touched.
// --light-pos NAME:X,Y,Z (a point light's <position>), --light-dir NAME:X,Y,Z (a direct light's <direction>, normalised by the library),
// --light-intensity NAME:R,G,B and --light-size NAME:S (a point light's <size>) (each repeatable, any mode): bhrt_scene_set_light on
// the light of that <light name=>, in command-line order, before anything is rendered and before --gpus N clones the scene.  --light-to-pos
// NAME:X,Y,Z (repeatable, needs --temporal N): frame k sets the point light to p0 + (p1 - p0) * ((float)k / (float)(N - 1)) per component in
// float32, p0 its position before frame 0, between the session's frames; the session notices it only through --reject-change.  An unknown name,
// a light of another kind than the option's, a malformed value, or --light-to-pos without --temporal: a usage error before any device is
// touched; values the library refuses (a negative intensity, a direction of length 0) fail with its message, before the upload too.
// --width W / --height H (any mode): bhrt_scene_set_resolution on the loaded scene, before every other setter; either flag alone
// keeps the other value.  A value below 1 is a usage error; a size the library refuses fails with its message.
// --upsample S [--upsample-depth-tolerance X] [--upsample-normal-threshold X] [--upsample-fallback albedo|light]: the frame is rendered at 1/S of the size and rebuilt
// at full size by bhrt_upsample: a clone of the scene, with every setter above applied, is set to W/S x H/S and rendered with bhrt_render_var
// (with --spp 1 with bhrt_render: no variance), photon maps are built on that clone, both scenes' bhrt_first_hit images are taken, and
// bhrt_upsample with the library's defaults (X replacing a stop; bhrt_upsample_opts.fallback as --upsample-fallback says; gamma as --no-gamma says) writes the full-size frame; with --denoise
// bhrt_denoise then filters that frame with the upsampled variance and the full-size guides.  S outside 1..8 or not a divisor of both sides,
// X or --upsample-fallback without --upsample, another word than albedo or light, and --upsample beside --temporal, --progressive, --adaptive, --guide-spp, --world or --gpus N > 1: a usage error before
// any device is touched.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "bhrt.h"
#include "bhrt_flat.h"

static int fail(const char *what)
{
    fprintf(stderr, "bhrt: %s: %s\n", what, bhrt_last_error());
    return 1;
}
#define HOST_CHECK(expr, what)                                                                  \
    do {                                                                                        \
        if ((expr) != 0) { fprintf(stderr, "bhrt: GPU %d: %s failed (%s)\n", r, what, #expr); \
            failed.store(true); return; }                                                       \
    } while (0)

struct Args {
    std::string scene, out = "out.png", radiance_out, photon_file, photon_out;
    uint32_t photons = 0;
    bhrt_opts o;
    int device = 0, gpus = 0;
    bool rehearse = false; // --rehearse: the N ranks of --gpus N all on device 0, the all-gather as N device-to-device copies (no RCCL)
    bool denoise = false;
    bhrt_denoise_opts dn;
    int guide_spp = 0;                 // --guide-spp N: the denoiser's guides from bhrt_guides at N samples per pixel; 0 = the denoiser's own first hit
    bool guide_spp_given = false;
    bool coverage_filter = false;      // --coverage-filter: bhrt_denoise_sampled with bhrt_guides' four images instead of bhrt_denoise with three
    float sigma_coverage = BHRT_DENOISE_SIGMA_COVERAGE; // --sigma-coverage X
    bool sigma_coverage_given = false;
    bool adaptive = false;
    bhrt_adaptive_opts ad;
    std::string samples_png;
    float dof = -1.f, focaldist = 0.f; // --dof / --focaldist: values for bhrt_scene_set_lens; dof < 0: not given
    bool emission = false;             // --emission: bhrt_scene_set_emissive
    bool face_materials = false;       // --face-materials: bhrt_scene_set_face_materials
    uint32_t global_map = 0;           // --global-map N: photons of the global map (bhrt_global_map_build); switches the global gather on
    float global_radius = 0.f;         // --global-radius R; 0 = the reference's 0.5
    int progressive = 0;               // --progressive N: samples per pixel and step of a bhrt_progressive_* session; 0 = one blocking render
    bool progressive_given = false;
    double time_limit = -1.0;          // --time-limit SECONDS; < 0: not given
    std::string live_png;              // --live-png PATH
    // --camera-pos / -target / -up, --fov and --shutter-pos / -target / -up: values for bhrt_scene_set_camera and bhrt_scene_set_shutter
    struct Vec { bool given = false; float v[3] = {0, 0, 0}; };
    Vec cam_pos, cam_target, cam_up, sh_pos, sh_target, sh_up;
    float fov = 0.f;                   // 0: not given
    int temporal = 0;                  // --temporal N: frames of the camera move; 0 = one frame
    bool temporal_given = false;
    Vec to_pos, to_target, to_up;      // --to-pos / -target / -up: the pose of the last frame
    std::string frames_png;            // --frames-png PREFIX
    bool spatial_variance = false;     // --spatial-variance (with --temporal N --denoise): bhrt_variance_spatial where a pixel's history is short
    int variance_radius = 0;           // --variance-radius R; 0: not given (the library's default)
    bool variance_radius_given = false;
    float variance_min_length = -1.f;  // --variance-min-length X; < 0: not given (4 x spp: four frames)
    bool reject_change = false;        // --reject-change (with --temporal N --denoise): bhrt_temporal_set_change, the change test of DESIGN.md 24
    int change_radius = 0;             // --change-radius R
    bool change_radius_given = false;
    float change_sigma[2] = {0, 0};    // --change-sigma LO,HI
    bool change_sigma_given = false;
    // --node-translate NAME:X,Y,Z (any mode: one translate op before anything is rendered) and --node-to-translate NAME:X,Y,Z (--temporal: the
    // node's translation at the last frame); `node` is resolved once the scene is loaded
    struct NodeMove { std::string name; float v[3] = {0, 0, 0}; int32_t node = -1; };
    std::vector<NodeMove> node_translate, node_to_translate;
    // --light-pos / --light-dir / --light-intensity NAME:X,Y,Z and --light-size NAME:S (any mode: bhrt_scene_set_light before anything is rendered, in
    // command-line order) and --light-to-pos NAME:X,Y,Z (--temporal: the point light's position at the last frame); `light` is resolved once the
    // scene is loaded
    struct LightEdit { const char *opt = ""; std::string name; float v[3] = {0, 0, 0}; int32_t light = -1; };
    std::vector<LightEdit> light_edits, light_to_pos;
    int width = 0, height = 0;         // --width W / --height H: bhrt_scene_set_resolution; 0: not given
    bool width_given = false, height_given = false;
    int upsample = 0;                  // --upsample S: render at 1/S of the size, bhrt_upsample to the full one
    bool upsample_given = false;
    float up_depth_tolerance = -1.f, up_normal_threshold = 0.f; // --upsample-depth-tolerance X (< 0: not given) / --upsample-normal-threshold X
    bool up_normal_threshold_given = false;
    int up_fallback = BHRT_UPSAMPLE_FALLBACK_ALBEDO; // --upsample-fallback albedo|light: bhrt_upsample_opts.fallback
    bool up_fallback_given = false;
    bool Camera() const { return cam_pos.given || cam_target.given || cam_up.given || fov > 0.f; }
    bool Shutter() const { return sh_pos.given || sh_target.given || sh_up.given; }
};

// three finite numbers "X,Y,Z" (--camera-*, --shutter-*), else a usage error
static Args::Vec vector_value(const char *opt, const char *text)
{
    Args::Vec r;
    const char *p = text;
    for (int k = 0; k < 3; k++) {
        char *end = nullptr;
        r.v[k] = strtof(p, &end);
        const bool last = k == 2;
        if (end == p || !(r.v[k] >= -3.402823466e38f && r.v[k] <= 3.402823466e38f) || (last ? *end != 0 : *end != ',')) {
            fprintf(stderr, "bhrt: usage: %s needs three finite numbers X,Y,Z, got \"%s\"\n", opt, text);
            exit(2);
        }
        p = end + 1;
    }
    r.given = true;
    return r;
}

// "NAME:X,Y,Z" (--node-translate, --node-to-translate): a node's name and three finite numbers, else a usage error
static Args::NodeMove node_move_value(const char *opt, const char *text)
{
    Args::NodeMove m;
    const char *colon = strrchr(text, ':');
    if (!colon || colon == text) {
        fprintf(stderr, "bhrt: usage: %s needs NAME:X,Y,Z, got \"%s\"\n", opt, text);
        exit(2);
    }
    m.name.assign(text, colon);
    const Args::Vec v = vector_value(opt, colon + 1);
    for (int k = 0; k < 3; k++) m.v[k] = v.v[k];
    return m;
}

// "NAME:X,Y,Z" (--light-pos, --light-dir, --light-intensity, --light-to-pos) or, with scalar, "NAME:S" (--light-size): a light's name and three
// finite numbers or one, else a usage error
static Args::LightEdit light_edit_value(const char *opt, const char *text, bool scalar = false)
{
    Args::LightEdit e;
    e.opt = opt;
    const char *colon = strrchr(text, ':');
    if (!colon || colon == text) {
        fprintf(stderr, "bhrt: usage: %s needs %s, got \"%s\"\n", opt, scalar ? "NAME:S" : "NAME:X,Y,Z", text);
        exit(2);
    }
    e.name.assign(text, colon);
    if (scalar) {
        char *end = nullptr;
        e.v[0] = strtof(colon + 1, &end);
        if (end == colon + 1 || *end || !(e.v[0] >= 0.f && e.v[0] <= 3.402823466e38f)) {
            fprintf(stderr, "bhrt: usage: %s needs NAME:S with a finite number S >= 0, got \"%s\"\n", opt, text);
            exit(2);
        }
    } else {
        const Args::Vec v = vector_value(opt, colon + 1);
        for (int k = 0; k < 3; k++) e.v[k] = v.v[k];
    }
    return e;
}

// a finite number >= 0 (--dof, --time-limit) or > 0 (--focaldist, --global-radius), else a usage error
static float number_value(const char *opt, const char *text, bool positive)
{
    char *end = nullptr;
    const float v = strtof(text, &end);
    if (end == text || *end || !(v >= 0.f && v <= 3.402823466e38f) || (positive && !(v > 0.f))) {
        fprintf(stderr, "bhrt: usage: %s needs a finite number %s, got \"%s\"\n", opt, positive ? "> 0" : ">= 0", text);
        exit(2);
    }
    return v;
}

// the adaptive frame's round count (doubling from min_spp up to the largest count) and the spp statistics of its rendered pixels (count > 0);
// rounds = false (--progressive: the steps are the caller's, and their lines say what ran): the statistics alone
static void print_adaptive(const std::vector<uint32_t> &cnt, const bhrt_opts &o, const bhrt_adaptive_opts &ad, bool rounds_known = true)
{
    uint64_t total = 0, px = 0;
    uint32_t cmin = 0xffffffffu, cmax = 0;
    for (uint32_t c : cnt)
        if (c) { total += c; px++; cmin = std::min(cmin, c); cmax = std::max(cmax, c); }
    int rounds = px ? 1 : 0;
    for (uint32_t n = (uint32_t)ad.min_spp; px && n < cmax; rounds++) n = std::min<uint32_t>((uint32_t)o.spp, 2 * n);
    if (!rounds_known) {
        printf("adaptive: spp mean %.3f min %u max %u, %llu samples\n", px ? (double)total / (double)px : 0.0, px ? cmin : 0, cmax, (unsigned long long)total);
        return;
    }
    printf("adaptive: %d round(s), spp mean %.3f min %u max %u, %llu samples\n", rounds, px ? (double)total / (double)px : 0.0, px ? cmin : 0, cmax,
           (unsigned long long)total);
}

// --progressive: BeginRender as a session stepped until every pixel has retired or the time limit has passed, then StopRender.  rgb / rad / var /
// cnt: the frame at that moment (rad, var and cnt may be empty); st: the sums over the steps.
static int render_progressive(bhrt_scene *scene, const Args &A, const bhrt_info &info, std::vector<uint8_t> &rgb, std::vector<float> &rad, std::vector<float> &var,
                              std::vector<uint32_t> &cnt, bhrt_stats &st)
{
    if (bhrt_progressive_begin(scene, &A.o, A.adaptive ? &A.ad : nullptr)) return fail("BeginRender (progressive)");
    const std::string tmp = A.live_png.empty() ? std::string() : A.live_png + ".tmp";
    const auto t0 = std::chrono::steady_clock::now();
    bhrt_progress pg;
    memset(&pg, 0, sizeof pg);
    for (;;) {
        bhrt_stats one;
        if (bhrt_progressive_step(scene, A.progressive, &one)) return fail("progressive step");
        st.closest_rays += one.closest_rays; st.shadow_rays += one.shadow_rays; st.shade_calls += one.shade_calls; st.camera_samples += one.camera_samples;
        st.passes += one.passes; st.wave_iterations += one.wave_iterations; st.seconds_total += one.seconds_total;
        if (bhrt_progressive_status(scene, &pg)) return fail("progressive status");
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("step %u: spp min %u max %u, %llu active pixel(s), %.3f s\n", pg.steps, pg.spp_min, pg.spp_max, (unsigned long long)pg.active_pixels, secs);
        fflush(stdout);
        if (!A.live_png.empty()) { // the viewport's refresh: a whole file at every moment
            if (bhrt_progressive_frame(scene, rgb.data(), nullptr, nullptr, nullptr)) return fail("progressive frame");
            if (bhrt_save_png(tmp.c_str(), rgb.data(), info.width, info.height)) return fail("SaveImage (live)");
            if (rename(tmp.c_str(), A.live_png.c_str())) { fprintf(stderr, "bhrt: cannot rename %s to %s\n", tmp.c_str(), A.live_png.c_str()); return 1; }
        }
        if (pg.finished || (A.time_limit >= 0.0 && secs > A.time_limit)) break;
    }
    if (bhrt_progressive_frame(scene, rgb.data(), rad.empty() ? nullptr : rad.data(), var.empty() ? nullptr : var.data(), cnt.empty() ? nullptr : cnt.data()))
        return fail("progressive frame");
    if (bhrt_progressive_end(scene)) return fail("StopRender");
    printf("progressive: %u step(s) of %d, %s\n", pg.steps, A.progressive, pg.finished ? "finished" : "stopped by --time-limit");
    return 0;
}

// The options of the guide images --guide-spp asks for: the render's seed, jitter and lens, the whole frame
static bhrt_opts guide_opts(const Args &A)
{
    bhrt_opts g = A.o;
    g.spp = A.guide_spp; g.rank = 0; g.world_size = 1;
    return g;
}

// DenoiseImage on host images (Main.cpp:236-238), with sampled guides when --guide-spp asks for them; rgb receives the filter's bytes
static int denoise_frame(bhrt_scene *scene, const Args &A, const bhrt_info &info, const float *rad, const float *var, uint8_t *rgb)
{
    if (A.guide_spp <= 0) return bhrt_denoise(scene, &A.dn, rad, var, nullptr, nullptr, nullptr, nullptr, rgb) ? fail("DenoiseImage") : 0;
    const size_t npx = (size_t)info.width * info.height;
    std::vector<float> z(npx), nrm(npx * 3), alb(npx * 3);
    const bhrt_opts g = guide_opts(A);
    if (A.coverage_filter) {
        std::vector<float> cov(npx);
        if (bhrt_guides(scene, &g, z.data(), nrm.data(), alb.data(), cov.data())) return fail("guide images");
        return bhrt_denoise_sampled(scene, &A.dn, A.sigma_coverage, rad, var, z.data(), nrm.data(), alb.data(), cov.data(), nullptr, rgb) ? fail("DenoiseImage (sampled guides)") : 0;
    }
    if (bhrt_guides(scene, &g, z.data(), nrm.data(), alb.data(), nullptr)) return fail("guide images");
    return bhrt_denoise(scene, &A.dn, rad, var, z.data(), nrm.data(), alb.data(), nullptr, rgb) ? fail("DenoiseImage") : 0;
}

// --upsample S: `low` (the clone at W/S x H/S, uploaded, photon maps built) is rendered, `full` gives the full-size first hit; bhrt_upsample
// writes the W x H frame, and with --denoise bhrt_denoise filters it with the upsampled variance and the same full-size guides.
// rgb / rad: the full-size frame (rad may be empty); st: the low render's.
static int render_upsampled(bhrt_scene *full, bhrt_scene *low, const Args &A, const bhrt_info &info, std::vector<uint8_t> &rgb, std::vector<float> &rad, bhrt_stats &st)
{
    const int w = info.width / A.upsample, h = info.height / A.upsample;
    const size_t n = (size_t)w * h, N = (size_t)info.width * info.height;
    const bool var = A.o.spp > 1; // at 1 sample per pixel a frame's variance is 0 by definition: none is carried
    std::vector<float> lrad(n * 3), lvar(var ? n * 3 : 0), lz(n), ln(n * 3), la(n * 3), z(N), nrm(N * 3), alb(N * 3), ovar(var && A.denoise ? N * 3 : 0);
    if (var ? bhrt_render_var(low, &A.o, nullptr, lrad.data(), lvar.data(), &st) : bhrt_render(low, &A.o, nullptr, lrad.data(), &st)) return fail("BeginRender (low frame)");
    if (bhrt_first_hit(low, lz.data(), ln.data(), la.data()) || bhrt_first_hit(full, z.data(), nrm.data(), alb.data())) return fail("first hit");
    bhrt_upsample_opts uo;
    bhrt_default_upsample_opts(&uo);
    uo.gamma = A.o.gamma;
    if (A.up_depth_tolerance >= 0.f) uo.depth_tolerance = A.up_depth_tolerance;
    if (A.up_normal_threshold_given) uo.normal_threshold = A.up_normal_threshold;
    uo.fallback = A.up_fallback;
    if (bhrt_upsample(full, &uo, w, h, lrad.data(), var ? lvar.data() : nullptr, lz.data(), ln.data(), la.data(), z.data(), nrm.data(), alb.data(),
                      rad.empty() ? nullptr : rad.data(), ovar.empty() ? nullptr : ovar.data(), nullptr, rgb.data()))
        return fail("upsample");
    printf("upsample: %d x %d at %d spp -> %d x %d (factor %d, depth tolerance %g, normal threshold %g, fallback %s)\n", w, h, A.o.spp, info.width, info.height,
           A.upsample, uo.depth_tolerance, uo.normal_threshold, uo.fallback == BHRT_UPSAMPLE_FALLBACK_LIGHT ? "light" : "albedo");
    if (A.denoise && bhrt_denoise(full, &A.dn, rad.data(), ovar.empty() ? nullptr : ovar.data(), z.data(), nrm.data(), alb.data(), nullptr, rgb.data())) return fail("DenoiseImage");
    return 0;
}

// --temporal N: N frames along the camera move p0 -> p1 (position, target, up), each reprojected into the next view and accumulated there.
// rgb / rad: the last frame (rad may be empty); st: the sums over the frames' renders.
static int render_temporal(bhrt_scene *scene, const Args &A, const bhrt_info &info, const float p0[9], const float p1[9], std::vector<uint8_t> &rgb, std::vector<float> &rad,
                           bhrt_stats &st)
{
    // the library's default stage options; --denoise carries the variance, --spatial-variance estimates it where the history is short
    // (DESIGN.md 22), --node-to-translate follows the nodes.  The session keeps every image on the device
    bhrt_temporal_session_opts ts;
    bhrt_default_temporal_session_opts(&ts);
    ts.temporal.gamma = A.o.gamma;
    ts.denoise_opts = A.dn;
    if (A.variance_radius_given) ts.spatial.radius = A.variance_radius;
    ts.spatial.min_length = A.variance_min_length >= 0.f ? A.variance_min_length : 4.f * (float)A.o.spp;
    ts.carry_variance = A.denoise; ts.denoise = A.denoise;
    ts.spatial_variance = A.spatial_variance;
    ts.follow_nodes = !A.node_to_translate.empty();
    // --node-to-translate: the moved nodes' records as they stand before frame 0
    std::vector<bhrt_xform> saved(A.node_to_translate.size());
    for (size_t m = 0; m < saved.size(); m++)
        if (bhrt_scene_get_node_transform(scene, A.node_to_translate[m].node, &saved[m])) return fail("node transform");
    // --light-to-pos: the moved point lights' positions as they stand before frame 0
    std::vector<bhrt_light_info> lights0(A.light_to_pos.size());
    for (size_t m = 0; m < lights0.size(); m++)
        if (bhrt_scene_get_light(scene, A.light_to_pos[m].light, &lights0[m])) return fail("get light");
    if (bhrt_temporal_begin(scene, &A.o, &ts)) return fail("temporal session");
    if (A.reject_change) { // the change test between reprojection and accumulation
        bhrt_change_opts ch;
        bhrt_default_change_opts(&ch);
        if (A.change_radius_given) ch.radius = A.change_radius;
        if (A.change_sigma_given) { ch.sigma_lo = A.change_sigma[0]; ch.sigma_hi = A.change_sigma[1]; }
        if (bhrt_temporal_set_change(scene, &ch)) return fail("temporal change test");
    }
    for (int k = 0; k < A.temporal; k++) {
        const float s = (float)k / (float)(A.temporal - 1);
        float p[9];
        for (int c = 0; c < 9; c++) p[c] = p0[c] + (p1[c] - p0[c]) * s;
        if (bhrt_scene_set_camera(scene, p, p + 3, p + 6, 0.f)) return fail("set camera");
        for (size_t m = 0; m < saved.size(); m++) { // the saved record plus a translate of delta * s
            const Args::NodeMove &mv = A.node_to_translate[m];
            bhrt_xform_op op = {BHRT_XFORM_TRANSLATE, {mv.v[0] * s, mv.v[1] * s, mv.v[2] * s, 0.f}};
            if (bhrt_scene_set_node_transform(scene, mv.node, saved[m].tm, saved[m].pos, &op, 1)) return fail("set node transform");
        }
        for (size_t m = 0; m < lights0.size(); m++) { // the point light in equal steps from its position to --light-to-pos
            const Args::LightEdit &e = A.light_to_pos[m];
            float q[3];
            for (int c = 0; c < 3; c++) q[c] = lights0[m].vec[c] + (e.v[c] - lights0[m].vec[c]) * s;
            if (bhrt_scene_set_light(scene, e.light, nullptr, q, -1.f)) return fail("set light");
        }
        bhrt_stats one;
        if (bhrt_temporal_frame(scene, rgb.data(), nullptr, &one)) return fail("temporal frame");
        st.closest_rays += one.closest_rays; st.shadow_rays += one.shadow_rays; st.shade_calls += one.shade_calls; st.camera_samples += one.camera_samples;
        st.passes += one.passes; st.wave_iterations += one.wave_iterations; st.seconds_total += one.seconds_total;
        bhrt_temporal_progress pg;
        if (bhrt_temporal_status(scene, &pg)) return fail("temporal status");
        printf("frame %d: camera %g,%g,%g, history on %.1f%% of the pixels\n", k, p[0], p[1], p[2], 100.0 * (double)pg.history_pixels / (double)pg.pixels);
        if (!A.frames_png.empty()) {
            char name[16];
            snprintf(name, sizeof name, "%03d.png", k);
            if (bhrt_save_png((A.frames_png + name).c_str(), rgb.data(), info.width, info.height)) return fail("SaveImage (frame)");
        }
    }
    if (!rad.empty() && bhrt_temporal_image(scene, BHRT_TEMPORAL_IMG_ACCUMULATED, rad.data())) return fail("temporal image");
    if (bhrt_temporal_end(scene)) return fail("temporal end");
    return 0;
}

// Everything render_multi owns besides the caller's scene: released on every way out (the early returns included).
struct MultiGuard {
    std::vector<ncclComm_t> comms;
    std::vector<bhrt_scene *> clones; // scenes[1..N-1]
    bool aborted = false;
    ~MultiGuard()
    {
        for (ncclComm_t c : comms)
            if (c) { if (aborted) ncclCommAbort(c); else ncclCommDestroy(c); }
        for (bhrt_scene *s : clones)
            if (s) bhrt_scene_free(s);
    }
};

// BeginRender over N GPUs of this node; rgb / rad: the whole frame on the host (rad may be empty)
static int render_multi(bhrt_scene *first, const Args &A, const bhrt_info &info, std::vector<uint8_t> &rgb, std::vector<float> &rad, std::vector<uint32_t> &cnt,
                        std::vector<bhrt_stats> &stats, double &gather_seconds)
{
    const int N = A.gpus, W = info.width, H = info.height, tile = A.o.tile_size > 0 ? A.o.tile_size : 32;
    int have = 0;
    if (bhrt_device_count(&have) || have < (A.rehearse ? 1 : N)) { fprintf(stderr, "bhrt: --gpus %d but %d device(s) visible\n", N, have); return 1; }
    std::vector<int> devs(N);
    for (int r = 0; r < N; r++) devs[r] = A.rehearse ? 0 : r;
    MultiGuard G;
    if (!A.rehearse) {
        G.comms.assign(N, nullptr);
        if (ncclCommInitAll(G.comms.data(), N, devs.data()) != ncclSuccess) { fprintf(stderr, "bhrt: ncclCommInitAll over %d devices failed\n", N); return 1; }
    }
    std::vector<bhrt_scene *> scenes(N, nullptr);
    scenes[0] = first;
    G.clones.assign(N, nullptr);
    for (int r = 1; r < N; r++) {
        if (bhrt_scene_clone(first, &scenes[r])) return fail("scene clone");
        G.clones[r] = scenes[r];
    }
    const size_t bb = bhrt_tiles_block_bytes(W, H, tile, N), npx = (size_t)W * H;
    stats.assign(N, bhrt_stats());
    std::atomic<bool> failed(false);

    // ---- caustic photon map over the N GPUs (BuildCausticPhotonMap, Main.cpp:342-386): batches of 2^20 emissions — the batch of the
    // single-GPU build, cut like bhraytracer_amd/dist.py::photon_build_sharded cuts it (slice r = blocks [256 B r / N, 256 B (r + 1) / N) of
    // the batch's B = 4096 blocks of 256), so that every N stops after the same number of emissions when a scene runs out of its emission
    // budget —, GPU r emits the r-th slice of every batch, the host strings the slices together in emission order and every GPU installs the
    // first `photons` records.
    if (!A.photon_file.empty()) {
        for (int r = 0; r < N; r++)
            if (bhrt_scene_upload(scenes[r], devs[r]) || bhrt_photon_import(scenes[r], A.photon_file.c_str(), 0)) return fail("photon import");
    } else if (A.photons) {
        const uint32_t batch = 1u << 20, blocks = batch / 256;
        if ((uint32_t)N > blocks) { fprintf(stderr, "bhrt: --gpus %d: more ranks than emission blocks per batch\n", N); return 1; }
        std::vector<uint8_t> kept;
        uint64_t e0 = 0, total = 0;
        const uint64_t budget = (uint64_t)A.photons * 4096ull + (1ull << 24);
        while (total < A.photons && e0 < budget) {
            std::vector<std::vector<uint8_t>> part(N);
            std::vector<uint32_t> cnt(N, 0);
            std::vector<std::thread> th;
            for (int r = 0; r < N; r++)
                th.emplace_back([&, r]() {
                    HOST_CHECK(bhrt_scene_upload(scenes[r], devs[r]), "upload");
                    const uint32_t lo = 256u * (uint32_t)((uint64_t)blocks * (uint64_t)r / (uint64_t)N), hi = 256u * (uint32_t)((uint64_t)blocks * (uint64_t)(r + 1) / (uint64_t)N);
                    uint32_t cap = std::max(4 * (hi - lo), 4096u);
                    for (int attempt = 0; attempt < 2; attempt++) { // "photons_out too small" reports the size it needs
                        part[r].resize((size_t)cap * 24);
                        if (bhrt_photon_emit_range(scenes[r], &A.o, 0, e0 + lo, hi - lo, part[r].data(), cap, &cnt[r]) == 0) return;
                        if (cnt[r] <= cap) break;
                        cap = cnt[r];
                    }
                    fprintf(stderr, "bhrt: GPU %d: photon emission: %s\n", r, bhrt_last_error());
                    failed.store(true);
                });
            for (auto &t : th) t.join();
            if (failed.load()) return 1;
            for (int r = 0; r < N; r++) { kept.insert(kept.end(), part[r].begin(), part[r].begin() + (size_t)cnt[r] * 24); total += cnt[r]; }
            e0 += batch;
        }
        if (total == 0) { fprintf(stderr, "bhrt: photon map: no photon reached a photon surface\n"); return 1; }
        const uint32_t n = (uint32_t)std::min<uint64_t>(total, A.photons);
        for (int r = 0; r < N; r++)
            if (bhrt_photon_install(scenes[r], kept.data(), n)) return fail("photon install");
        printf("caustic photon map: %u photons from %llu emissions on %d GPU(s)\n", n, (unsigned long long)e0, N);
    }
    if ((A.o.photon_map || A.photons || !A.photon_file.empty()) && !A.photon_out.empty() && bhrt_photon_export(scenes[0], A.photon_out.c_str())) return fail("photon export");

    // ---- the frame: one host thread per GPU.  The threads agree on failure at three rendezvous points — after set-up, after the render, after
    // the pack — so either all of them enter the collective or none does: a rank missing from an all-gather would hang the others.  Inside the
    // collective a thread never blocks in a stream synchronise: it polls its stream and the failure flag, and when a peer has failed it
    // aborts its communicator (ncclCommAbort) and leaves.
    std::vector<double> gather_s(N, 0.0);
    std::vector<uint8_t *> mine_of(N, nullptr), mine_v_of(N, nullptr), mine_c_of(N, nullptr); // --rehearse: where every rank's packed blocks lie (all on device 0)
    std::atomic<int> ready(0), rendered(0), packed(0), exchanged(0);
    auto rendezvous = [&](std::atomic<int> &c) { c.fetch_add(1); while (c.load() < N) std::this_thread::yield(); return !failed.load(); };
    std::vector<std::thread> th;
    for (int r = 0; r < N; r++)
        th.emplace_back([&, r]() {
            uint8_t *d_rgb = nullptr, *d_mine = nullptr, *d_all = nullptr, *d_mine_v = nullptr, *d_all_v = nullptr, *d_mine_c = nullptr, *d_all_c = nullptr;
            float *d_rad = nullptr, *d_var = nullptr, *d_cntf = nullptr, *d_guide = nullptr;
            uint32_t *d_cnt = nullptr;
            hipStream_t s = nullptr;
            auto setup = [&]() {
                HOST_CHECK(bhrt_scene_upload(scenes[r], devs[r]), "upload");
                if (A.global_map) HOST_CHECK(bhrt_global_map_build(scenes[r], &A.o, A.global_map, nullptr), "global map build"); // the whole map on every rank: keyed emission, identical bytes
                HOST_CHECK(hipSetDevice(devs[r]), "hipSetDevice");
                HOST_CHECK(hipStreamCreate(&s), "stream");
                HOST_CHECK(hipMalloc(&d_rgb, npx * 3), "hipMalloc");
                HOST_CHECK(hipMalloc(&d_rad, npx * 3 * sizeof(float)), "hipMalloc");
                HOST_CHECK(hipMalloc(&d_mine, bb), "hipMalloc");
                HOST_CHECK(hipMalloc(&d_all, bb * N), "hipMalloc");
                HOST_CHECK(hipMemsetAsync(d_rgb, 0, npx * 3, s), "memset");
                HOST_CHECK(hipMemsetAsync(d_rad, 0, npx * 3 * sizeof(float), s), "memset");
                if (A.denoise) { // the variance tiles: a second block of the same shape (its RGB8 section repeats the first block's)
                    HOST_CHECK(hipMalloc(&d_var, npx * 3 * sizeof(float)), "hipMalloc");
                    HOST_CHECK(hipMalloc(&d_mine_v, bb), "hipMalloc");
                    HOST_CHECK(hipMalloc(&d_all_v, bb * N), "hipMalloc");
                    HOST_CHECK(hipMemsetAsync(d_var, 0, npx * 3 * sizeof(float), s), "memset");
                    if (r == 0 && A.guide_spp > 0) HOST_CHECK(hipMalloc(&d_guide, npx * 8 * sizeof(float)), "hipMalloc"); // z, normal, albedo, coverage
                }
                if (A.adaptive) { // the counts: a further block whose float section holds them (channel 0 of a W x H x 3 float image)
                    HOST_CHECK(hipMalloc(&d_cnt, npx * sizeof(uint32_t)), "hipMalloc");
                    HOST_CHECK(hipMalloc(&d_cntf, npx * 3 * sizeof(float)), "hipMalloc");
                    HOST_CHECK(hipMalloc(&d_mine_c, bb), "hipMalloc");
                    HOST_CHECK(hipMalloc(&d_all_c, bb * N), "hipMalloc");
                    HOST_CHECK(hipMemsetAsync(d_cnt, 0, npx * sizeof(uint32_t), s), "memset");
                }
                HOST_CHECK(hipStreamSynchronize(s), "sync");
            };
            setup();
            auto release = [&]() {
                (void)hipFree(d_rgb); (void)hipFree(d_rad); (void)hipFree(d_mine); (void)hipFree(d_all);
                (void)hipFree(d_var); (void)hipFree(d_mine_v); (void)hipFree(d_all_v); (void)hipFree(d_guide);
                (void)hipFree(d_cnt); (void)hipFree(d_cntf); (void)hipFree(d_mine_c); (void)hipFree(d_all_c);
                if (s) (void)hipStreamDestroy(s);
            };
            if (!rendezvous(ready)) { release(); return; }
            bhrt_opts o = A.o;
            o.rank = r; o.world_size = N; o.tile_size = tile;
            if (A.photons || !A.photon_file.empty()) o.photon_map = 1;
            const int rc = A.adaptive ? bhrt_render_adaptive_dev(scenes[r], &o, &A.ad, d_rgb, d_rad, d_var, d_cnt, &stats[r], nullptr)
                                      : bhrt_render_var_dev(scenes[r], &o, d_rgb, d_rad, d_var, &stats[r], nullptr);
            if (rc) { fprintf(stderr, "bhrt: GPU %d: BeginRender: %s\n", r, bhrt_last_error()); failed.store(true); }
            if (!rc && A.adaptive) { // counts -> floats (exact below 2^24): through the host, W x H words
                std::vector<uint32_t> hc(npx);
                std::vector<float> hf(npx * 3, 0.f);
                if (hipMemcpy(hc.data(), d_cnt, npx * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) failed.store(true);
                for (size_t k = 0; k < npx; k++) hf[3 * k] = (float)hc[k];
                if (hipMemcpy(d_cntf, hf.data(), npx * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) failed.store(true);
            }
            if (!rendezvous(rendered)) { release(); return; }
            const auto t0 = std::chrono::steady_clock::now();
            auto pack = [&]() {
                HOST_CHECK(bhrt_tiles_pack_dev(d_rgb, d_rad, W, H, tile, r, N, d_mine, s), "pack");
                if (A.denoise) HOST_CHECK(bhrt_tiles_pack_dev(d_rgb, d_var, W, H, tile, r, N, d_mine_v, s), "pack");
                if (A.adaptive) HOST_CHECK(bhrt_tiles_pack_dev(d_rgb, d_cntf, W, H, tile, r, N, d_mine_c, s), "pack");
                HOST_CHECK(hipStreamSynchronize(s), "sync");
                mine_of[r] = d_mine;
                mine_v_of[r] = d_mine_v;
                mine_c_of[r] = d_mine_c;
            };
            pack();
            if (getenv("BHRT_TEST_FAIL_PACK") && atoi(getenv("BHRT_TEST_FAIL_PACK")) == r) { fprintf(stderr, "bhrt: GPU %d: pack failed (test knob)\n", r); failed.store(true); }
            if (!rendezvous(packed)) { release(); return; } // a rank whose pack failed keeps everybody out of the collective
            // waits for the stream without blocking in it: a peer's failure is seen within a poll
            auto wait_stream = [&]() -> bool {
                for (;;) {
                    const hipError_t q = hipStreamQuery(s);
                    if (q == hipSuccess) return true;
                    if (q != hipErrorNotReady) { fprintf(stderr, "bhrt: GPU %d: stream: %s\n", r, hipGetErrorString(q)); failed.store(true); }
                    if (failed.load()) {
                        if (!A.rehearse) { ncclCommAbort(G.comms[r]); G.comms[r] = nullptr; }
                        return false;
                    }
                    std::this_thread::yield();
                }
            };
            auto exchange = [&]() {
                if (A.rehearse) { // the all-gather of N ranks on ONE device: every rank copies every block into its own receive buffer
                    for (int k = 0; k < N; k++) HOST_CHECK(hipMemcpyAsync(d_all + (size_t)k * bb, mine_of[k], bb, hipMemcpyDeviceToDevice, s), "copy of a peer's block");
                    if (A.denoise)
                        for (int k = 0; k < N; k++) HOST_CHECK(hipMemcpyAsync(d_all_v + (size_t)k * bb, mine_v_of[k], bb, hipMemcpyDeviceToDevice, s), "copy of a peer's block");
                    if (A.adaptive)
                        for (int k = 0; k < N; k++) HOST_CHECK(hipMemcpyAsync(d_all_c + (size_t)k * bb, mine_c_of[k], bb, hipMemcpyDeviceToDevice, s), "copy of a peer's block");
                } else if (ncclAllGather(d_mine, d_all, bb, ncclUint8, G.comms[r], s) != ncclSuccess ||
                           (A.denoise && ncclAllGather(d_mine_v, d_all_v, bb, ncclUint8, G.comms[r], s) != ncclSuccess) ||
                           (A.adaptive && ncclAllGather(d_mine_c, d_all_c, bb, ncclUint8, G.comms[r], s) != ncclSuccess)) {
                    fprintf(stderr, "bhrt: GPU %d: ncclAllGather failed\n", r);
                    failed.store(true);
                }
                if (!wait_stream()) return;
                HOST_CHECK(bhrt_tiles_unpack_dev(d_all, W, H, tile, N, d_rgb, d_rad, s), "unpack");
                if (A.denoise) HOST_CHECK(bhrt_tiles_unpack_dev(d_all_v, W, H, tile, N, d_rgb, d_var, s), "unpack"); // the same RGB8 bytes again
                if (A.adaptive) HOST_CHECK(bhrt_tiles_unpack_dev(d_all_c, W, H, tile, N, d_rgb, d_cntf, s), "unpack");
                HOST_CHECK(hipStreamSynchronize(s), "sync");
                gather_s[r] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (r == 0 && A.denoise) { // DenoiseImage on the gathered frame (Main.cpp:236-238): the PNG bytes become the filter's
                    if (d_guide) { // --guide-spp: the whole frame's guides, here where the filter runs
                        const bhrt_opts g = guide_opts(A);
                        HOST_CHECK(bhrt_guides_dev(scenes[0], &g, d_guide, d_guide + npx, d_guide + 4 * npx, A.coverage_filter ? d_guide + 7 * npx : nullptr, s), "guide images");
                    }
                    if (A.coverage_filter)
                        HOST_CHECK(bhrt_denoise_sampled_dev(scenes[0], &A.dn, A.sigma_coverage, d_rad, d_var, d_guide, d_guide + npx, d_guide + 4 * npx, d_guide + 7 * npx, nullptr, d_rgb, s),
                                   "denoise (sampled guides)");
                    else
                        HOST_CHECK(bhrt_denoise_dev(scenes[0], &A.dn, d_rad, d_var, d_guide, d_guide ? d_guide + npx : nullptr, d_guide ? d_guide + 4 * npx : nullptr, nullptr, d_rgb, s),
                                   "denoise");
                    HOST_CHECK(hipStreamSynchronize(s), "sync");
                }
                if (r == 0) {
                    HOST_CHECK(hipMemcpy(rgb.data(), d_rgb, npx * 3, hipMemcpyDeviceToHost), "copy");
                    if (!rad.empty()) HOST_CHECK(hipMemcpy(rad.data(), d_rad, npx * 3 * sizeof(float), hipMemcpyDeviceToHost), "copy");
                    if (A.adaptive) {
                        std::vector<float> hf(npx * 3);
                        HOST_CHECK(hipMemcpy(hf.data(), d_cntf, npx * 3 * sizeof(float), hipMemcpyDeviceToHost), "copy");
                        cnt.assign(npx, 0);
                        for (size_t k = 0; k < npx; k++) cnt[k] = (uint32_t)hf[3 * k];
                    }
                }
            };
            exchange();
            rendezvous(exchanged); // --rehearse: nobody frees a block a peer may still be copying
            release();
        });
    for (auto &t : th) t.join();
    gather_seconds = *std::max_element(gather_s.begin(), gather_s.end());
    G.aborted = failed.load();
    return failed.load() ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || (strcmp(argv[1], "render") && strcmp(argv[1], "info"))) {
        fprintf(stderr, "usage: bhrt render|info <scene.xml> [options]\n");
        return 2;
    }
    const bool render = !strcmp(argv[1], "render");
    Args A;
    A.scene = argv[2];
    bhrt_opts &o = A.o;
    bhrt_default_opts(&o);
    bhrt_default_denoise_opts(&A.dn);
    bhrt_default_adaptive_opts(&A.ad);
    for (int a = 3; a < argc; a++) {
        std::string s = argv[a];
        auto next = [&]() -> const char * { if (a + 1 >= argc) { fprintf(stderr, "bhrt: %s needs a value\n", s.c_str()); exit(2); } return argv[++a]; };
        if (s == "-o") A.out = next();
        else if (s == "--spp") o.spp = atoi(next());
        else if (s == "--gi") o.gi_bounces = atoi(next());
        else if (s == "--bounces") o.internal_bounces = atoi(next());
        else if (s == "--seed") o.seed = (uint32_t)strtoul(next(), nullptr, 10);
        else if (s == "--no-jitter") o.jitter = 0;
        else if (s == "--no-gamma") o.gamma = 0;
        else if (s == "--leaf-skip") o.leaf_skip = 1;
        else if (s == "--photon-exact") o.photon_exact = 1;
        else if (s == "--device") A.device = atoi(next());
        else if (s == "--gpus") A.gpus = atoi(next());
        else if (s == "--rehearse") A.rehearse = true;
        else if (s == "--rank") o.rank = atoi(next());
        else if (s == "--world") o.world_size = atoi(next());
        else if (s == "--tile") o.tile_size = atoi(next());
        else if (s == "--radiance") A.radiance_out = next();
        else if (s == "--photons") A.photons = (uint32_t)strtoul(next(), nullptr, 10);
        else if (s == "--photon-file") A.photon_file = next();
        else if (s == "--photon-out") A.photon_out = next();
        else if (s == "--denoise") A.denoise = true;
        else if (s == "--denoise-iters") A.dn.iterations = atoi(next());
        else if (s == "--guide-spp") { A.guide_spp = atoi(next()); A.guide_spp_given = true; }
        else if (s == "--coverage-filter") A.coverage_filter = true;
        else if (s == "--sigma-coverage") { A.sigma_coverage = number_value("--sigma-coverage", next(), false); A.sigma_coverage_given = true; }
        else if (s == "--adaptive") A.adaptive = true;
        else if (s == "--spp-min") A.ad.min_spp = atoi(next());
        else if (s == "--adaptive-threshold") A.ad.threshold = (float)atof(next());
        else if (s == "--samples-png") A.samples_png = next();
        else if (s == "--lens") o.lens = 1;
        else if (s == "--emission") A.emission = true;
        else if (s == "--face-materials") A.face_materials = true;
        else if (s == "--global-map") A.global_map = (uint32_t)strtoul(next(), nullptr, 10);
        else if (s == "--global-radius") A.global_radius = number_value("--global-radius", next(), true);
        else if (s == "--progressive") { A.progressive = atoi(next()); A.progressive_given = true; }
        else if (s == "--time-limit") A.time_limit = number_value("--time-limit", next(), false);
        else if (s == "--live-png") A.live_png = next();
        else if (s == "--dof") { A.dof = number_value("--dof", next(), false); o.lens = 1; }
        else if (s == "--focaldist") { A.focaldist = number_value("--focaldist", next(), true); o.lens = 1; }
        else if (s == "--camera-pos") A.cam_pos = vector_value("--camera-pos", next());
        else if (s == "--camera-target") A.cam_target = vector_value("--camera-target", next());
        else if (s == "--camera-up") A.cam_up = vector_value("--camera-up", next());
        else if (s == "--shutter-pos") A.sh_pos = vector_value("--shutter-pos", next());
        else if (s == "--shutter-target") A.sh_target = vector_value("--shutter-target", next());
        else if (s == "--shutter-up") A.sh_up = vector_value("--shutter-up", next());
        else if (s == "--temporal") { A.temporal = atoi(next()); A.temporal_given = true; }
        else if (s == "--to-pos") A.to_pos = vector_value("--to-pos", next());
        else if (s == "--to-target") A.to_target = vector_value("--to-target", next());
        else if (s == "--to-up") A.to_up = vector_value("--to-up", next());
        else if (s == "--frames-png") A.frames_png = next();
        else if (s == "--spatial-variance") A.spatial_variance = true;
        else if (s == "--variance-radius") { A.variance_radius = atoi(next()); A.variance_radius_given = true; }
        else if (s == "--variance-min-length") A.variance_min_length = number_value("--variance-min-length", next(), false);
        else if (s == "--reject-change") A.reject_change = true;
        else if (s == "--change-radius") { A.change_radius = atoi(next()); A.change_radius_given = true; }
        else if (s == "--change-sigma") {
            const char *text = next();
            char *end = nullptr, *end2 = nullptr;
            const float lo = strtof(text, &end);
            const float hi = end != text && *end == ',' ? strtof(end + 1, &end2) : 0.f;
            if (end == text || *end != ',' || end2 == end + 1 || *end2 || !(lo >= 0.f && lo <= hi && hi <= 3.402823466e38f)) {
                fprintf(stderr, "bhrt: usage: --change-sigma needs two finite numbers LO,HI with 0 <= LO <= HI, got \"%s\"\n", text);
                return 2;
            }
            A.change_sigma[0] = lo; A.change_sigma[1] = hi; A.change_sigma_given = true;
        }
        else if (s == "--node-translate") A.node_translate.push_back(node_move_value("--node-translate", next()));
        else if (s == "--node-to-translate") A.node_to_translate.push_back(node_move_value("--node-to-translate", next()));
        else if (s == "--light-pos") A.light_edits.push_back(light_edit_value("--light-pos", next()));
        else if (s == "--light-dir") A.light_edits.push_back(light_edit_value("--light-dir", next()));
        else if (s == "--light-intensity") A.light_edits.push_back(light_edit_value("--light-intensity", next()));
        else if (s == "--light-size") A.light_edits.push_back(light_edit_value("--light-size", next(), true));
        else if (s == "--light-to-pos") A.light_to_pos.push_back(light_edit_value("--light-to-pos", next()));
        else if (s == "--width") { A.width = atoi(next()); A.width_given = true; }
        else if (s == "--height") { A.height = atoi(next()); A.height_given = true; }
        else if (s == "--upsample") { A.upsample = atoi(next()); A.upsample_given = true; }
        else if (s == "--upsample-depth-tolerance") A.up_depth_tolerance = number_value("--upsample-depth-tolerance", next(), false);
        else if (s == "--upsample-normal-threshold") {
            const char *text = next();
            char *end = nullptr;
            A.up_normal_threshold = strtof(text, &end);
            if (end == text || *end || A.up_normal_threshold != A.up_normal_threshold) { fprintf(stderr, "bhrt: usage: --upsample-normal-threshold needs a number, got \"%s\"\n", text); return 2; }
            A.up_normal_threshold_given = true;
        }
        else if (s == "--upsample-fallback") {
            const std::string word = next();
            if (word == "albedo") A.up_fallback = BHRT_UPSAMPLE_FALLBACK_ALBEDO;
            else if (word == "light") A.up_fallback = BHRT_UPSAMPLE_FALLBACK_LIGHT;
            else { fprintf(stderr, "bhrt: usage: --upsample-fallback needs albedo or light, got \"%s\"\n", word.c_str()); return 2; }
            A.up_fallback_given = true;
        }
        else if (s == "--fov") {
            A.fov = number_value("--fov", next(), true);
            if (!(A.fov < 180.f)) { fprintf(stderr, "bhrt: usage: --fov needs a number of degrees below 180\n"); return 2; }
        }
        else { fprintf(stderr, "bhrt: unknown option %s\n", s.c_str()); return 2; }
    }
    if (A.gpus < 0 || A.gpus > 64 || (A.gpus > 0 && (o.rank != 0 || o.world_size != 1))) { fprintf(stderr, "bhrt: --gpus N drives all N ranks itself (no --rank / --world)\n"); return 2; }
    if (A.denoise && o.world_size > 1) { // before any device is touched
        fprintf(stderr, "bhrt: usage: --denoise filters the whole frame; a rank of --world %d renders part of it (use --gpus N)\n", o.world_size);
        return 2;
    }
    if (A.denoise && (A.dn.iterations < 0 || A.dn.iterations > 16)) { fprintf(stderr, "bhrt: usage: --denoise-iters must be in 0..16\n"); return 2; }
    if (A.guide_spp_given && !A.denoise) { fprintf(stderr, "bhrt: usage: --guide-spp needs --denoise (the guide images steer the denoiser)\n"); return 2; }
    if (A.guide_spp < 0 || A.guide_spp > 65535) { fprintf(stderr, "bhrt: usage: --guide-spp must be in 0..65535 (0 = the denoiser's own first-hit guides)\n"); return 2; }
    if (A.coverage_filter && (!A.denoise || A.guide_spp <= 0)) {
        fprintf(stderr, "bhrt: usage: --coverage-filter needs --denoise and --guide-spp N with N > 0 (the filter reads the sampled guides' coverage)\n");
        return 2;
    }
    if (A.sigma_coverage_given && !A.coverage_filter) { fprintf(stderr, "bhrt: usage: --sigma-coverage needs --coverage-filter\n"); return 2; }
    if (!A.adaptive && !A.samples_png.empty()) { fprintf(stderr, "bhrt: usage: --samples-png needs --adaptive\n"); return 2; }
    if (A.adaptive && !A.samples_png.empty() && o.world_size > 1) { // before any device is touched
        fprintf(stderr, "bhrt: usage: --samples-png normalises over the whole frame; a rank of --world %d renders part of it (use --gpus N)\n", o.world_size);
        return 2;
    }
    if (A.adaptive && (A.ad.min_spp < 2 || A.ad.min_spp > o.spp || o.spp > 65535 || A.ad.threshold != A.ad.threshold)) {
        fprintf(stderr, "bhrt: usage: --adaptive needs 2 <= --spp-min <= --spp <= 65535 and a number for --adaptive-threshold\n");
        return 2;
    }
    if (A.global_radius > 0.f && !A.global_map) { fprintf(stderr, "bhrt: usage: --global-radius needs --global-map N\n"); return 2; }
    if (!A.progressive_given && (A.time_limit >= 0.0 || !A.live_png.empty())) { fprintf(stderr, "bhrt: usage: --time-limit and --live-png need --progressive N\n"); return 2; }
    if (A.progressive_given && A.progressive < 1) { fprintf(stderr, "bhrt: usage: --progressive needs a step of at least 1 sample per pixel\n"); return 2; }
    if (A.progressive_given && A.gpus > 1) { // before any device is touched
        fprintf(stderr, "bhrt: usage: --progressive runs on one device; --gpus %d would need a tile exchange per step\n", A.gpus);
        return 2;
    }
    if (!A.temporal_given && (A.to_pos.given || A.to_target.given || A.to_up.given || !A.frames_png.empty())) {
        fprintf(stderr, "bhrt: usage: --to-pos, --to-target, --to-up and --frames-png need --temporal N\n");
        return 2;
    }
    if (!A.temporal_given && !A.node_to_translate.empty()) { fprintf(stderr, "bhrt: usage: --node-to-translate needs --temporal N\n"); return 2; }
    if (!A.temporal_given && !A.light_to_pos.empty()) { fprintf(stderr, "bhrt: usage: --light-to-pos needs --temporal N\n"); return 2; }
    if (A.temporal_given && (A.temporal < 2 || A.progressive_given || A.adaptive || A.gpus > 0 || o.world_size > 1)) { // before any device is touched
        fprintf(stderr, "bhrt: usage: --temporal needs N >= 2 frames and renders whole frames on one device (no --progressive, --adaptive, --gpus, --world)\n");
        return 2;
    }
    if ((A.spatial_variance || A.variance_radius_given || A.variance_min_length >= 0.f) && !(A.spatial_variance && A.temporal_given && A.denoise)) {
        fprintf(stderr, "bhrt: usage: --spatial-variance needs --temporal N --denoise, and --variance-radius / --variance-min-length need --spatial-variance\n");
        return 2;
    }
    if (A.variance_radius_given && (A.variance_radius < 1 || A.variance_radius > 4)) { fprintf(stderr, "bhrt: usage: --variance-radius must be in 1..4\n"); return 2; }
    if ((A.reject_change || A.change_radius_given || A.change_sigma_given) && !(A.reject_change && A.temporal_given && A.denoise)) {
        fprintf(stderr, "bhrt: usage: --reject-change needs --temporal N --denoise, and --change-radius / --change-sigma need --reject-change\n");
        return 2;
    }
    if (A.change_radius_given && (A.change_radius < 1 || A.change_radius > 4)) { fprintf(stderr, "bhrt: usage: --change-radius must be in 1..4\n"); return 2; }
    if (A.temporal_given && A.denoise && o.spp < (A.spatial_variance ? 1 : 2)) {
        fprintf(stderr, "bhrt: usage: --temporal with --denoise needs --spp >= 2 (at 1 sample per pixel a frame's variance is 0 by definition; --spatial-variance estimates one)\n");
        return 2;
    }
    if (A.temporal_given && A.denoise && (A.guide_spp_given || A.coverage_filter)) {
        fprintf(stderr, "bhrt: usage: --temporal with --denoise filters with the first-hit guides (no --guide-spp, --coverage-filter)\n");
        return 2;
    }
    if ((A.width_given && A.width < 1) || (A.height_given && A.height < 1)) { fprintf(stderr, "bhrt: usage: --width and --height need a size of at least 1\n"); return 2; }
    if ((A.up_depth_tolerance >= 0.f || A.up_normal_threshold_given || A.up_fallback_given) && !A.upsample_given) {
        fprintf(stderr, "bhrt: usage: --upsample-depth-tolerance, --upsample-normal-threshold and --upsample-fallback need --upsample S\n");
        return 2;
    }
    if (A.upsample_given && (A.upsample < 1 || A.upsample > 8)) { fprintf(stderr, "bhrt: usage: --upsample needs a factor S in 1..8\n"); return 2; }
    if (A.upsample_given && (A.temporal_given || A.progressive_given || A.adaptive || A.guide_spp_given || A.gpus > 1 || o.world_size > 1)) { // before any device is touched
        fprintf(stderr, "bhrt: usage: --upsample renders one whole frame on one device (no --temporal, --progressive, --adaptive, --guide-spp, --world, --gpus N > 1)\n");
        return 2;
    }
    if ((A.progressive_given || A.upsample_given) && A.gpus == 1) A.gpus = 0; // one device: no communicator is needed
    A.dn.gamma = o.gamma;
    bhrt_scene *scene = nullptr;
    if (bhrt_scene_load_xml(A.scene.c_str(), &scene)) return fail("LoadScene");
    bhrt_info info;
    bhrt_scene_info(scene, &info);
    for (uint32_t i = 0; i < info.n_warnings; i++) {
        const char *w = nullptr;
        if (!bhrt_scene_warning(scene, i, &w)) fprintf(stderr, "bhrt: warning: %s\n", w);
    }
    if (A.width_given || A.height_given) { // before everything else: every later setter and message sees the new size
        if (bhrt_scene_set_resolution(scene, A.width_given ? A.width : info.width, A.height_given ? A.height : info.height)) return fail("set resolution");
        bhrt_scene_info(scene, &info);
    }
    if (A.upsample_given && (info.width % A.upsample || info.height % A.upsample)) { // before any device is touched
        fprintf(stderr, "bhrt: usage: --upsample %d does not divide the image size %d x %d\n", A.upsample, info.width, info.height);
        bhrt_scene_free(scene);
        return 2;
    }
    printf("Render image width: %d\nRender image height: %d\n", info.width, info.height); // Main.cpp:426-427
    printf("nodes %u, meshes %u (%u triangles, %u BVH nodes), materials %u, lights %u, textures %u, scene blob %llu bytes\n", info.n_nodes,
           info.n_meshes, info.n_triangles, info.n_bvh_nodes, info.n_materials, info.n_lights, info.n_textures, (unsigned long long)info.flat_bytes);
    for (std::vector<Args::NodeMove> *moves : {&A.node_translate, &A.node_to_translate}) // before any device is touched
        for (Args::NodeMove &m : *moves)
            if (bhrt_scene_node_index(scene, m.name.c_str(), &m.node)) {
                fprintf(stderr, "bhrt: usage: %s: the scene has no node named \"%s\"\n", moves == &A.node_translate ? "--node-translate" : "--node-to-translate", m.name.c_str());
                bhrt_scene_free(scene);
                return 2;
            }
    for (std::vector<Args::LightEdit> *edits : {&A.light_edits, &A.light_to_pos}) // before any device is touched: the name, and the kind the option needs
        for (Args::LightEdit &e : *edits) {
            if (bhrt_scene_light_index(scene, e.name.c_str(), &e.light)) {
                fprintf(stderr, "bhrt: usage: %s: the scene has no light named \"%s\"\n", e.opt, e.name.c_str());
                bhrt_scene_free(scene);
                return 2;
            }
            bhrt_light_info li;
            if (bhrt_scene_get_light(scene, e.light, &li)) return fail("get light");
            const bool dir = !strcmp(e.opt, "--light-dir"), any = !strcmp(e.opt, "--light-intensity");
            if (!any && li.type != (dir ? BHRT_LIGHT_DIRECT : BHRT_LIGHT_POINT)) {
                fprintf(stderr, "bhrt: usage: %s: the light \"%s\" is not a %s light\n", e.opt, e.name.c_str(), dir ? "direct" : "point");
                bhrt_scene_free(scene);
                return 2;
            }
        }
    if (!render) { bhrt_scene_free(scene); return 0; }
    for (const Args::LightEdit &e : A.light_edits) { // in command-line order, before the upload and before --gpus N clones the scene
        const bool size = !strcmp(e.opt, "--light-size"), intensity = !strcmp(e.opt, "--light-intensity");
        if (bhrt_scene_set_light(scene, e.light, intensity ? e.v : nullptr, size || intensity ? nullptr : e.v, size ? e.v[0] : -1.f)) return fail(e.opt);
        if (size) printf("light %s (%d): %s %g\n", e.name.c_str(), e.light, e.opt + 8, e.v[0]);
        else printf("light %s (%d): %s %g,%g,%g\n", e.name.c_str(), e.light, e.opt + 8, e.v[0], e.v[1], e.v[2]);
    }
    for (const Args::NodeMove &m : A.node_translate) { // one translate op appended to the node, before the upload and before --gpus N clones the scene
        bhrt_xform xf;
        bhrt_xform_op op = {BHRT_XFORM_TRANSLATE, {m.v[0], m.v[1], m.v[2], 0.f}};
        if (bhrt_scene_get_node_transform(scene, m.node, &xf) || bhrt_scene_set_node_transform(scene, m.node, xf.tm, xf.pos, &op, 1)) return fail("node translate");
        printf("node %s (%d): translated by %g,%g,%g\n", m.name.c_str(), m.node, m.v[0], m.v[1], m.v[2]);
    }
    if (A.emission && bhrt_scene_set_emissive(scene, 1)) return fail("set emissive"); // before the upload and before --gpus N clones the scene
    if (A.face_materials && bhrt_scene_set_face_materials(scene, 1)) return fail("set face materials"); // likewise
    if (A.global_map && bhrt_scene_set_global_gather(scene, 1, A.global_radius)) return fail("set global gather"); // likewise; the map is built after the upload
    if (o.lens) { // before the upload and before --gpus N clones the scene
        const bhrt_flat_header *fh = nullptr;
        uint64_t fb = 0;
        if (bhrt_scene_flat(scene, (const void **)&fh, &fb)) return fail("scene blob");
        if ((A.dof >= 0.f || A.focaldist > 0.f) && bhrt_scene_set_lens(scene, A.focaldist, A.dof >= 0.f ? A.dof : fh->camera.dof)) return fail("set lens");
        if (!(fh->camera.dof >= 0.f && fh->camera.dof <= 3.402823466e38f)) { fprintf(stderr, "bhrt: usage: --lens: the scene's <dof> must be a finite number >= 0 (or give --dof)\n"); return 2; }
        printf("lens: focal distance %g, aperture radius %g%s\n", fh->camera.focaldist, fh->camera.dof, fh->camera.dof > 0.f ? "" : " (pinhole)");
        if (A.denoise && A.guide_spp <= 0) printf("note: --denoise guides (depth, normal, albedo) are those of the pinhole ray; --guide-spp N forms them from the lens rays\n");
    }
    float pose0[9] = {0}, pose1[9] = {0}; // --temporal: the first and the last frame's position, target, up
    if (A.Camera() || A.Shutter() || A.temporal_given) { // before the upload and before --gpus N clones the scene; after --focaldist, which places the default target
        const bhrt_flat_header *fh = nullptr;
        uint64_t fb = 0;
        if (bhrt_scene_flat(scene, (const void **)&fh, &fb)) return fail("scene blob");
        auto pose = [&](const Args::Vec &gp, const Args::Vec &gt, const Args::Vec &gu, float *pos, float *target, float *up) {
            const bhrt_camera &c = fh->camera; // the scene's pose now: the missing values
            for (int k = 0; k < 3; k++) {
                pos[k] = gp.given ? gp.v[k] : c.pos[k];
                target[k] = gt.given ? gt.v[k] : c.pos[k] + c.dir[k] * c.focaldist;
                up[k] = gu.given ? gu.v[k] : c.up[k];
            }
        };
        float p[3], t[3], u[3];
        if (A.Camera()) {
            pose(A.cam_pos, A.cam_target, A.cam_up, p, t, u);
            if (bhrt_scene_set_camera(scene, p, t, u, A.fov)) return fail("set camera");
        }
        pose(A.cam_pos, A.cam_target, A.cam_up, p, t, u); // pose 0 as it stands
        printf("camera: position %g,%g,%g target %g,%g,%g up %g,%g,%g fov %g\n", p[0], p[1], p[2], t[0], t[1], t[2], u[0], u[1], u[2], fh->camera.fov);
        if (A.Shutter()) {
            float p1[3], t1[3], u1[3];
            pose(A.sh_pos, A.sh_target, A.sh_up, p1, t1, u1);
            if (!A.sh_target.given) for (int k = 0; k < 3; k++) t1[k] = t[k]; // pose 0's target as given, not recomputed
            if (!A.sh_pos.given) for (int k = 0; k < 3; k++) p1[k] = p[k];
            if (!A.sh_up.given) for (int k = 0; k < 3; k++) u1[k] = u[k];
            if (bhrt_scene_set_shutter(scene, 1, p1, t1, u1)) return fail("set shutter");
            printf("shutter: to position %g,%g,%g target %g,%g,%g up %g,%g,%g during the exposure\n", p1[0], p1[1], p1[2], t1[0], t1[1], t1[2], u1[0], u1[1], u1[2]);
        }
        for (int k = 0; k < 3; k++) {
            pose0[k] = p[k]; pose0[3 + k] = t[k]; pose0[6 + k] = u[k];
            pose1[k] = A.to_pos.given ? A.to_pos.v[k] : p[k]; pose1[3 + k] = A.to_target.given ? A.to_target.v[k] : t[k]; pose1[6 + k] = A.to_up.given ? A.to_up.v[k] : u[k];
        }
    }
    if (A.denoise && A.guide_spp > 0) printf("denoise guides: %d sample(s) per pixel%s\n", A.guide_spp, o.lens ? ", through the lens" : "");
    if (A.coverage_filter) printf("denoise filter: for sampled guides, coverage tolerance %g\n", A.sigma_coverage);
    std::vector<uint8_t> rgb((size_t)info.width * info.height * 3, 0);
    std::vector<float> rad(A.radiance_out.empty() && !A.denoise ? 0 : (size_t)info.width * info.height * 3, 0.f);
    std::vector<uint32_t> cnt(A.adaptive ? (size_t)info.width * info.height : 0, 0u);
    bhrt_stats st;
    memset(&st, 0, sizeof st);
    if (A.gpus > 0) {
        std::vector<bhrt_stats> per;
        double gather_s = 0;
        const auto t0 = std::chrono::steady_clock::now();
        if (render_multi(scene, A, info, rgb, rad, cnt, per, gather_s)) return 1;
        const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        double slowest = 0;
        for (int r = 0; r < A.gpus; r++) {
            st.closest_rays += per[r].closest_rays; st.shadow_rays += per[r].shadow_rays; st.camera_samples += per[r].camera_samples;
            st.wave_iterations = std::max(st.wave_iterations, per[r].wave_iterations); st.passes = std::max(st.passes, per[r].passes);
            slowest = std::max(slowest, per[r].seconds_total);
            printf("GPU %d: %llu camera samples, %llu rays, %.3f s\n", r, (unsigned long long)per[r].camera_samples,
                   (unsigned long long)(per[r].closest_rays + per[r].shadow_rays), per[r].seconds_total);
        }
        st.seconds_total = slowest;
        printf("%d GPU(s): frame %.3f s on the slowest GPU, %s tile gather %.4f s, %.3f s wall incl. set-up\n", A.gpus, slowest, A.rehearse ? "rehearsed (device-to-device)" : "RCCL", gather_s, wall);
    } else {
        bhrt_scene *full = scene; // --upsample: `scene` becomes the low-size clone that is rendered (every setter above is in it), `full` keeps the frame's size
        if (A.upsample_given) {
            if (bhrt_scene_clone(full, &scene)) return fail("clone");
            if (bhrt_scene_set_resolution(scene, info.width / A.upsample, info.height / A.upsample)) return fail("set resolution (low frame)");
            if (bhrt_scene_upload(full, A.device)) return fail("upload");
        }
        if (bhrt_scene_upload(scene, A.device)) return fail("upload");
        if (A.global_map) { // BuildPhotonMap, Main.cpp:196
            uint32_t stored = 0;
            if (bhrt_global_map_build(scene, &o, A.global_map, &stored)) return fail("BuildPhotonMap");
            printf("global photon map: %u photons, gather radius %g\n", stored, A.global_radius > 0.f ? A.global_radius : 0.5f);
        }
        if (!A.photon_file.empty()) { // a cached photon pass
            if (bhrt_photon_import(scene, A.photon_file.c_str(), 0)) return fail("photon import");
            o.photon_map = 1;
        } else if (A.photons) { // BuildCausticPhotonMap, Main.cpp:194
            uint32_t stored = 0;
            if (bhrt_photon_build(scene, &o, A.photons, &stored)) return fail("BuildCausticPhotonMap");
            printf("caustic photon map: %u photons\n", stored);
            o.photon_map = 1;
        }
        if (o.photon_map && !A.photon_out.empty() && bhrt_photon_export(scene, A.photon_out.c_str())) return fail("photon export");
        if (A.upsample_given) {
            if (render_upsampled(full, scene, A, info, rgb, rad, st)) return 1;
            bhrt_scene_free(scene);
            scene = full;
        } else if (A.temporal_given) {
            if (render_temporal(scene, A, info, pose0, pose1, rgb, rad, st)) return 1;
        } else if (A.progressive_given) {
            std::vector<float> var(A.denoise ? rad.size() : 0, 0.f);
            if (render_progressive(scene, A, info, rgb, rad, var, cnt, st)) return 1;
            if (A.denoise && denoise_frame(scene, A, info, rad.data(), var.data(), rgb.data())) return 1;
        } else if (A.adaptive) {
            std::vector<float> var(A.denoise ? rad.size() : 0, 0.f);
            if (bhrt_render_adaptive(scene, &o, &A.ad, rgb.data(), rad.empty() ? nullptr : rad.data(), var.empty() ? nullptr : var.data(), cnt.data(), &st))
                return fail("BeginRender (adaptive)");
            if (A.denoise && denoise_frame(scene, A, info, rad.data(), var.data(), rgb.data())) return 1;
        } else if (A.denoise) {
            std::vector<float> var(rad.size(), 0.f);
            if (bhrt_render_var(scene, &o, rgb.data(), rad.data(), var.data(), &st)) return fail("BeginRender");
            if (denoise_frame(scene, A, info, rad.data(), var.data(), rgb.data())) return 1;
        } else if (bhrt_render(scene, &o, rgb.data(), rad.empty() ? nullptr : rad.data(), &st)) return fail("BeginRender");
    }
    const double rays = (double)st.closest_rays + (double)st.shadow_rays;
    printf("rendered %llu camera samples, %.0f rays (%llu closest + %llu shadow), %u wave steps in %u pass(es): %.3f s, %.1f Mrays/s\n",
           (unsigned long long)st.camera_samples, rays, (unsigned long long)st.closest_rays, (unsigned long long)st.shadow_rays, st.wave_iterations,
           st.passes, st.seconds_total, rays / st.seconds_total / 1e6);
    if (A.adaptive) print_adaptive(cnt, o, A.ad, !A.progressive_given);
    if (bhrt_save_png(A.out.c_str(), rgb.data(), info.width, info.height)) return fail("SaveImage");
    if (!A.samples_png.empty()) { // ComputeSampleCountImage + SaveSampleCountImage (scene.h:603-630)
        std::vector<uint8_t> img(cnt.size());
        uint32_t smax = 0;
        if (bhrt_sample_count_image(scene, cnt.data(), cnt.size(), img.data(), &smax)) return fail("ComputeSampleCountImage");
        if (bhrt_save_png_gray(A.samples_png.c_str(), img.data(), info.width, info.height)) return fail("SaveSampleCountImage");
    }
    if (!A.radiance_out.empty()) {
        FILE *fp = fopen(A.radiance_out.c_str(), "wb");
        if (!fp) { fprintf(stderr, "bhrt: cannot write %s\n", A.radiance_out.c_str()); return 1; }
        fwrite(rad.data(), sizeof(float), rad.size(), fp);
        fclose(fp);
    }
    printf("wrote %s\n", A.out.c_str());
    bhrt_scene_free(scene);
    return 0;
}
