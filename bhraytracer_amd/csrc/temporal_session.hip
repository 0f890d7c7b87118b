// temporal_session.hip — the temporal session (bhrt_temporal_*): reproject -> accumulate -> estimate -> denoise as one call per
// frame on images that stay in HBM.  A translation unit above the library's own public _dev entry points: every stage is the call a host would
// make (include/bhrt.h states the sequence), so a frame is what the chained wrappers give byte for byte; this file owns the images, the order,
// the "previous" view and the failure state, and launches nothing itself but the count of the pixels with history (k_history_count, temporal.hip).
// The change test (bhrt_temporal_set_change) is one more such call, bhrt_temporal_change_dev, between reprojection and accumulation.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "bhrt.h"
#include "bhrt_flat.h"
#include "denoise.h"
#include "dev_buf.h"
#include "scene_internal.h"
#include "temporal.h"

namespace bhrt {

// One view's first hit: what reprojection compares two frames by
struct TemporalView {
    DevBuf<float> z, normal, albedo;
    DevBuf<int32_t> node; // follow_nodes
};

struct TemporalSession {
    bhrt_opts o = {};
    bhrt_temporal_session_opts t = {};
    int device = -1;   // where the images live; -1 = none allocated yet
    size_t npx = 0;    // the pixels they are sized for
    uint32_t k = 0;    // complete frames since begin or reset: the next frame's index
    bool failed = false;
    uint64_t history_pixels = 0;
    // the previous view (after a frame: that frame's) and the one a frame fills; the accumulated frame the next frame reprojects and the one a
    // frame writes.  A frame ends by swapping each pair
    TemporalView prev, cur;
    DevBuf<float> acc, acc_len, out, out_len;
    DevBuf<float> acc_var, out_var;              // carry_variance
    DevBuf<float> radiance, history, history_len; // the frame's render, the reprojected light and its length
    DevBuf<float> variance, history_var;         // carry_variance
    DevBuf<float> filter_var;                    // spatial_variance
    bool change_on = false;                      // bhrt_temporal_set_change: stage 2C between reprojection and accumulation
    bhrt_change_opts change = {};
    DevBuf<float> change_img, used_len;          // the change test: lambda and the length stage 5 received
    DevBuf<float> display;                       // denoise, host variant: the radiance bhrt_temporal_frame copies out
    DevBuf<uint8_t> rgb;                         // host variant
    DevBuf<unsigned long long> d_count;
    float prev_frame[12] = {0};
    std::vector<bhrt_xform> prev_xf;             // follow_nodes
};

void DestroyTemporalSession(TemporalSession *t)
{
    if (!t) return;
    if (t->device >= 0) (void)hipSetDevice(t->device);
    delete t; // hipFree waits for the device
}

bool TemporalSessionHoldsBuffers(const TemporalSession *t) { return t && t->device >= 0; }

static const char *SessionOptsError(bhrt_scene *scene, const bhrt_opts *o, const bhrt_temporal_session_opts *t)
{
    if (t->spatial_variance && !t->carry_variance) return "bhrt_temporal_begin: spatial_variance needs carry_variance";
    if (t->denoise && !t->carry_variance) return "bhrt_temporal_begin: denoise needs carry_variance";
    if (t->carry_variance && o->spp < 2 && !t->spatial_variance) return "bhrt_temporal_begin: carry_variance at spp < 2 needs spatial_variance (a 1-spp frame has no variance)";
    if (o->world_size > 1) return "bhrt_temporal_begin: a session renders whole frames (world_size must be 1)";
    float frame[12];
    if (bhrt_scene_get_camera_frame(scene, frame)) return "bhrt_temporal_begin: the scene has no camera frame";
    static const float image = 0.f; // stands for a given image: the checks read no pixel
    const char *bad = ReprojectArgsError(&t->reproject, frame, &image, &image);
    if (*bad) return bad;
    bad = TemporalArgsError(&t->temporal, (float)o->spp);
    if (*bad) return bad;
    if (t->spatial_variance) {
        bad = SpatialVarianceArgsError(&t->spatial, &image, &image, &image, &image);
        if (*bad) return bad;
    }
    if (t->denoise) {
        bad = DenoiseOptsError(t->denoise_opts);
        if (*bad) return bad;
    }
    return "";
}

// The images of the session's mode, sized for the scene's frame.  A size that changed (it cannot through the public setters) starts over.
static int ReserveImages(bhrt_scene *scene, TemporalSession &T, bool host_rgb, bool host_display)
{
    const bhrt_flat_header *H = scene->flat.hdr();
    const size_t n = (size_t)H->camera.width * H->camera.height;
    if (n == 0 || n > 0x7fffffffull) { SetError("bhrt_temporal_frame: frame size out of range"); return BHRT_ERR_ARG; }
    if (T.npx != n) { T.k = 0; T.npx = n; }
    T.device = SceneDevice(scene);
    const bool var = T.t.carry_variance != 0;
    for (TemporalView *v : {&T.prev, &T.cur}) {
        BHRT_TRY(v->z.Reserve(n));
        BHRT_TRY(v->normal.Reserve(n * 3));
        BHRT_TRY(v->albedo.Reserve(n * 3));
        if (T.t.follow_nodes) BHRT_TRY(v->node.Reserve(n));
    }
    for (DevBuf<float> *b : {&T.acc, &T.out, &T.radiance, &T.history}) BHRT_TRY(b->Reserve(n * 3));
    for (DevBuf<float> *b : {&T.acc_len, &T.out_len, &T.history_len}) BHRT_TRY(b->Reserve(n));
    if (var)
        for (DevBuf<float> *b : {&T.acc_var, &T.out_var, &T.variance, &T.history_var}) BHRT_TRY(b->Reserve(n * 3));
    if (T.t.spatial_variance) BHRT_TRY(T.filter_var.Reserve(n * 3));
    if (T.change_on)
        for (DevBuf<float> *b : {&T.change_img, &T.used_len}) BHRT_TRY(b->Reserve(n));
    if (host_display) BHRT_TRY(T.display.Reserve(n * 3));
    if (host_rgb) BHRT_TRY(T.rgb.Reserve(n * 3));
    BHRT_TRY(T.d_count.Reserve(1));
    if (T.t.follow_nodes) T.prev_xf.resize(std::max<uint32_t>(H->n_nodes, 1));
    return BHRT_OK;
}

// The stages of frame T.k.  d_rgb8 / d_display: where the displayed frame's bytes and (with denoise) radiance go, device memory, may be NULL
static int RunFrame(bhrt_scene *scene, TemporalSession &T, uint8_t *d_rgb8, float *d_display, bhrt_stats *stats, hipStream_t st)
{
    const bhrt_temporal_session_opts &t = T.t;
    const bool var = t.carry_variance != 0, moving = t.follow_nodes != 0, first = T.k == 0;
    bhrt_opts o = T.o;
    o.seed = T.o.seed + T.k;
    TemporalView &P = T.prev, &C = T.cur;
    BHRT_TRY(bhrt_first_hit_ex_dev(scene, C.z, C.normal, C.albedo, moving ? C.node.p : nullptr, st));
    BHRT_TRY(var ? bhrt_render_var_dev(scene, &o, nullptr, T.radiance, T.variance, stats, st) : bhrt_render_dev(scene, &o, nullptr, T.radiance, stats, st));
    if (var) { // the calls that carry the variance
        if (t.spatial_variance && o.spp < 2) BHRT_TRY(bhrt_variance_spatial_dev(scene, &t.spatial, T.radiance, nullptr, nullptr, C.z, C.normal, C.albedo, T.variance, st));
        if (!first)
            BHRT_TRY(bhrt_reproject_var_dev(scene, &t.reproject, T.prev_frame, moving ? T.prev_xf.data() : nullptr, P.z, P.normal, T.acc, T.acc_var, T.acc_len, P.albedo,
                                            moving ? P.node.p : nullptr, C.z, C.normal, C.albedo, moving ? C.node.p : nullptr, T.history, T.history_var, T.history_len, nullptr,
                                            st));
        const bool change = T.change_on && !first; // step 4b: the length stage 5 receives
        if (change)
            BHRT_TRY(bhrt_temporal_change_dev(scene, &T.change, T.radiance, T.variance, T.history, T.history_var, T.history_len, C.z, C.normal, T.used_len, T.change_img, st));
        BHRT_TRY(bhrt_temporal_accumulate_var_dev(scene, &t.temporal, T.radiance, T.variance, (float)o.spp, first ? nullptr : T.history.p, first ? nullptr : T.history_var.p,
                                                  first ? nullptr : (change ? T.used_len.p : T.history_len.p), T.out, T.out_var, T.out_len, t.denoise ? nullptr : d_rgb8, st));
        if (t.spatial_variance) BHRT_TRY(bhrt_variance_spatial_dev(scene, &t.spatial, T.out, T.out_var, T.out_len, C.z, C.normal, C.albedo, T.filter_var, st));
        if (t.denoise)
            BHRT_TRY(bhrt_denoise_dev(scene, &t.denoise_opts, T.out, t.spatial_variance ? T.filter_var.p : T.out_var.p, C.z, C.normal, C.albedo, d_display, d_rgb8, st));
    } else {
        if (!first && moving)
            BHRT_TRY(bhrt_reproject_moving_dev(scene, &t.reproject, T.prev_frame, T.prev_xf.data(), P.z, P.normal, T.acc, T.acc_len, P.albedo, P.node, C.z, C.normal, C.albedo, C.node,
                                               T.history, T.history_len, nullptr, st));
        else if (!first)
            BHRT_TRY(bhrt_reproject_dev(scene, &t.reproject, T.prev_frame, P.z, P.normal, T.acc, T.acc_len, P.albedo, C.z, C.normal, C.albedo, T.history, T.history_len, nullptr, st));
        BHRT_TRY(bhrt_temporal_accumulate_dev(scene, &t.temporal, T.radiance, (float)o.spp, first ? nullptr : T.history.p, first ? nullptr : T.history_len.p, T.out, T.out_len,
                                              d_rgb8, st));
    }
    if (first) HIP_CHECK(hipMemsetAsync(T.history_len, 0, T.npx * sizeof(float), st)); // frame 0 has no history: the kept image says so
    if (first && T.change_on)
        for (DevBuf<float> *b : {&T.change_img, &T.used_len}) HIP_CHECK(hipMemsetAsync(b->p, 0, T.npx * sizeof(float), st));
    HIP_CHECK(HistoryCountLaunch(T.history_len, T.npx, T.d_count, st));
    return BHRT_OK;
}

// A frame for either variant.  Host pointers (rgb8, radiance) are served through the session's own device images; device pointers are written
// by the stages themselves, the accumulated radiance of a session without denoise by one device copy.
static int Frame(bhrt_scene *scene, bool dev, uint8_t *rgb8, float *radiance, bhrt_stats *stats)
{
    const char *what = dev ? "bhrt_temporal_frame_dev" : "bhrt_temporal_frame";
    if (!scene) { SetError(std::string(what) + ": null scene"); return BHRT_ERR_ARG; }
    TemporalSession *Tp = scene->temporal;
    if (!Tp) { SetError(std::string(what) + ": no temporal session is open on this scene (bhrt_temporal_begin)"); return BHRT_ERR_ARG; }
    TemporalSession &T = *Tp;
    if (T.failed) { SetError(std::string(what) + ": a frame of this session failed; bhrt_temporal_reset or bhrt_temporal_end"); return BHRT_ERR_ARG; }
    BHRT_TRY(RenderArgsCheck(scene, &T.o)); // the setters may have run since begin
    if (!scene->dev) BHRT_TRY(bhrt_scene_upload(scene, 0));
    HIP_CHECK(hipSetDevice(SceneDevice(scene)));
    const bool denoise = T.t.denoise != 0;
    BHRT_TRY(ReserveImages(scene, T, !dev && rgb8, !dev && radiance && denoise));
    hipStream_t st = (hipStream_t)SceneStream(scene);
    const size_t n = T.npx;
    uint8_t *d_rgb8 = dev ? rgb8 : (rgb8 ? T.rgb.p : nullptr);
    float *d_display = !denoise ? nullptr : dev ? radiance : (radiance ? T.display.p : nullptr);
    int rc = RunFrame(scene, T, d_rgb8, d_display, stats, st);
    unsigned long long count = 0;
    if (!rc) rc = [&]() -> int {
        HIP_CHECK(hipMemcpyAsync(&count, T.d_count, sizeof count, hipMemcpyDeviceToHost, st));
        const float *shown = denoise ? d_display : T.out.p; // the displayed radiance on the device
        if (dev && radiance && !denoise) HIP_CHECK(hipMemcpyAsync(radiance, shown, n * 12, hipMemcpyDeviceToDevice, st));
        if (!dev && radiance) HIP_CHECK(hipMemcpyAsync(radiance, shown, n * 12, hipMemcpyDeviceToHost, st));
        if (!dev && rgb8) HIP_CHECK(hipMemcpyAsync(rgb8, d_rgb8, n * 3, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        BHRT_TRY(bhrt_scene_get_camera_frame(scene, T.prev_frame));
        if (T.t.follow_nodes) BHRT_TRY(bhrt_scene_get_node_transforms(scene, T.prev_xf.data(), (uint32_t)T.prev_xf.size(), nullptr));
        return BHRT_OK;
    }();
    if (rc) { // work of this frame may have run: the images no longer describe frame k - 1
        (void)hipStreamSynchronize(st);
        T.failed = true;
        return rc;
    }
    std::swap(T.prev, T.cur);
    std::swap(T.acc, T.out); std::swap(T.acc_len, T.out_len); std::swap(T.acc_var, T.out_var);
    T.history_pixels = count;
    T.k++;
    return BHRT_OK;
}

// the kept image `which` of the last complete frame: its device address and its bytes; nullptr where the session's mode does not keep it
static const void *KeptImage(const TemporalSession &T, int which, size_t &bytes)
{
    const size_t n = T.npx;
    const bool var = T.t.carry_variance != 0;
    bytes = n * 12;
    switch (which) {
    case BHRT_TEMPORAL_IMG_ACCUMULATED: return T.acc.p;
    case BHRT_TEMPORAL_IMG_VARIANCE: return var ? T.acc_var.p : nullptr;
    case BHRT_TEMPORAL_IMG_LENGTH: bytes = n * 4; return T.acc_len.p;
    case BHRT_TEMPORAL_IMG_HISTORY_LENGTH: bytes = n * 4; return T.history_len.p;
    case BHRT_TEMPORAL_IMG_FILTER_VARIANCE: return T.t.spatial_variance ? T.filter_var.p : nullptr;
    case BHRT_TEMPORAL_IMG_Z: bytes = n * 4; return T.prev.z.p;
    case BHRT_TEMPORAL_IMG_NORMAL: return T.prev.normal.p;
    case BHRT_TEMPORAL_IMG_ALBEDO: return T.prev.albedo.p;
    case BHRT_TEMPORAL_IMG_NODE: bytes = n * 4; return T.t.follow_nodes ? (const void *)T.prev.node.p : nullptr;
    case BHRT_TEMPORAL_IMG_CURRENT: return T.radiance.p;
    case BHRT_TEMPORAL_IMG_CURRENT_VARIANCE: return var ? T.variance.p : nullptr;
    case BHRT_TEMPORAL_IMG_CHANGE: bytes = n * 4; return T.change_on ? T.change_img.p : nullptr;
    case BHRT_TEMPORAL_IMG_USED_LENGTH: bytes = n * 4; return T.change_on ? T.used_len.p : nullptr;
    }
    return nullptr;
}

static int FindImage(bhrt_scene *scene, int which, const char *what, const void *&d, size_t &bytes)
{
    if (!scene) { SetError(std::string(what) + ": null scene"); return BHRT_ERR_ARG; }
    const TemporalSession *T = scene->temporal;
    if (!T) { SetError(std::string(what) + ": no temporal session is open on this scene (bhrt_temporal_begin)"); return BHRT_ERR_ARG; }
    if (T->failed) { SetError(std::string(what) + ": a frame of this session failed; bhrt_temporal_reset or bhrt_temporal_end"); return BHRT_ERR_ARG; }
    if (T->k == 0 || T->device < 0) { SetError(std::string(what) + ": no frame since bhrt_temporal_begin or _reset"); return BHRT_ERR_ARG; }
    d = KeptImage(*T, which, bytes);
    if (!d) { SetError(std::string(what) + ": image " + std::to_string(which) + " is not kept by this session's mode"); return BHRT_ERR_ARG; }
    return BHRT_OK;
}

} // namespace bhrt

using namespace bhrt;

extern "C" {

int bhrt_temporal_begin(bhrt_scene *scene, const bhrt_opts *opts, const bhrt_temporal_session_opts *topts)
try {
    if (!scene || !opts || !topts) { SetError("bhrt_temporal_begin: null argument"); return BHRT_ERR_ARG; }
    if (scene->temporal) { SetError("bhrt_temporal_begin: a session is already open on this scene (bhrt_temporal_end first)"); return BHRT_ERR_ARG; }
    BHRT_TRY(RenderArgsCheck(scene, opts)); // first: the stages' checks below read spp
    const char *bad = SessionOptsError(scene, opts, topts);
    if (*bad) { SetError(bad); return BHRT_ERR_ARG; }
    TemporalSession *T = new TemporalSession;
    T->o = *opts;
    T->t = *topts;
    scene->temporal = T;
    scene->temporal_release = DestroyTemporalSession; // for bhrt_scene_free
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_frame(bhrt_scene *scene, uint8_t *rgb8, float *radiance, bhrt_stats *stats)
try {
    return Frame(scene, false, rgb8, radiance, stats);
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_frame_dev(bhrt_scene *scene, uint8_t *d_rgb8, float *d_radiance, bhrt_stats *stats)
try {
    return Frame(scene, true, d_rgb8, d_radiance, stats);
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_reset(bhrt_scene *scene)
try {
    if (!scene) { SetError("bhrt_temporal_reset: null scene"); return BHRT_ERR_ARG; }
    if (!scene->temporal) { SetError("bhrt_temporal_reset: no temporal session is open on this scene (bhrt_temporal_begin)"); return BHRT_ERR_ARG; }
    scene->temporal->k = 0;
    scene->temporal->failed = false;
    scene->temporal->history_pixels = 0;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_set_change(bhrt_scene *scene, const bhrt_change_opts *opts)
try {
    if (!scene) { SetError("bhrt_temporal_set_change: null scene"); return BHRT_ERR_ARG; }
    TemporalSession *T = scene->temporal;
    if (!T) { SetError("bhrt_temporal_set_change: no temporal session is open on this scene (bhrt_temporal_begin)"); return BHRT_ERR_ARG; }
    if (T->k > 0) { SetError("bhrt_temporal_set_change: a frame has completed since bhrt_temporal_begin or _reset"); return BHRT_ERR_ARG; }
    if (!T->t.carry_variance) { SetError("bhrt_temporal_set_change: the change test needs carry_variance (it reads both variances)"); return BHRT_ERR_ARG; }
    if (opts) {
        const char *bad = TemporalChangeOptsError(opts);
        if (*bad) { SetError(bad); return BHRT_ERR_ARG; }
        T->change = *opts;
    }
    T->change_on = opts != nullptr;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_status(const bhrt_scene *scene, bhrt_temporal_progress *progress)
try {
    if (!scene || !progress) { SetError("bhrt_temporal_status: null argument"); return BHRT_ERR_ARG; }
    const TemporalSession *T = scene->temporal;
    if (!T) { SetError("bhrt_temporal_status: no temporal session is open on this scene (bhrt_temporal_begin)"); return BHRT_ERR_ARG; }
    memset(progress, 0, sizeof *progress);
    progress->frames = T->k;
    progress->failed = T->failed ? 1 : 0;
    progress->history_pixels = T->history_pixels;
    progress->pixels = (uint64_t)scene->flat.hdr()->camera.width * (uint64_t)scene->flat.hdr()->camera.height;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_image_dev(bhrt_scene *scene, int which, const void **d_ptr)
try {
    if (!d_ptr) { SetError("bhrt_temporal_image_dev: null argument"); return BHRT_ERR_ARG; }
    size_t bytes = 0;
    return FindImage(scene, which, "bhrt_temporal_image_dev", *d_ptr, bytes);
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_image(bhrt_scene *scene, int which, void *host)
try {
    if (!host) { SetError("bhrt_temporal_image: null argument"); return BHRT_ERR_ARG; }
    const void *d = nullptr;
    size_t bytes = 0;
    BHRT_TRY(FindImage(scene, which, "bhrt_temporal_image", d, bytes));
    HIP_CHECK(hipSetDevice(scene->temporal->device));
    hipStream_t st = (hipStream_t)SceneStream(scene);
    HIP_CHECK(hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_end(bhrt_scene *scene)
try {
    if (!scene) { SetError("bhrt_temporal_end: null scene"); return BHRT_ERR_ARG; }
    DestroyTemporalSession(scene->temporal);
    scene->temporal = nullptr;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

} // extern "C"
