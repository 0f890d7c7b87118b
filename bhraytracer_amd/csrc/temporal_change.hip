// temporal_change.hip — the entry points of the temporal change test (bhrt_temporal_change*; stage 2C of temporal.hip, which holds
// the kernel and its launcher).  A translation unit above the library's public _dev entry points, like temporal_session.hip: guides the caller
// leaves out are bhrt_first_hit_dev's, into scratch the scene owns through a pointer (scene_internal.h).
#include <hip/hip_runtime.h>

#include <string>

#include "bhrt.h"
#include "bhrt_flat.h"
#include "dev_buf.h"
#include "scene_internal.h"
#include "temporal.h"

namespace bhrt {

// z (n floats) then normal (3n floats) of guides computed here, on the device the scene was uploaded to when they were allocated
struct ChangeScratch {
    int device = -1;
    DevBuf<float> g;
};

static void DestroyChangeScratch(ChangeScratch *c)
{
    if (!c) return;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    delete c; // hipFree waits for the device
}

// the scene's guide scratch, n pixels, on the scene's device (a scene uploaded to another device since gets new memory there)
static int ReserveChangeScratch(bhrt_scene *scene, size_t n, float *&g)
{
    const int dev = SceneDevice(scene);
    if (scene->change_scratch && scene->change_scratch->device != dev) {
        DestroyChangeScratch(scene->change_scratch);
        scene->change_scratch = nullptr;
        HIP_CHECK(hipSetDevice(dev));
    }
    if (!scene->change_scratch) {
        scene->change_scratch = new ChangeScratch;
        scene->change_scratch_release = DestroyChangeScratch;
        scene->change_scratch->device = dev;
    }
    BHRT_TRY(scene->change_scratch->g.Reserve(n * 4));
    g = scene->change_scratch->g.p;
    return BHRT_OK;
}

// the arguments of both entry points, checked alike and before any device is touched
static int TemporalChangeArgs(const bhrt_scene *scene, const bhrt_change_opts *opts, const float *radiance, const float *variance, const float *history,
                              const float *history_variance, const float *length, const float *out_length)
{
    if (!scene) { SetError("temporal change: null scene"); return BHRT_ERR_ARG; }
    const char *bad = TemporalChangeArgsError(opts, radiance, variance, history, history_variance, length, out_length);
    if (*bad) { SetError(bad); return BHRT_ERR_ARG; }
    return BHRT_OK;
}

} // namespace bhrt

using namespace bhrt;

extern "C" {

int bhrt_temporal_change_dev(bhrt_scene *scene, const bhrt_change_opts *opts, const float *d_radiance, const float *d_variance, const float *d_history,
                             const float *d_history_variance, const float *d_length, const float *d_z, const float *d_normal, float *d_out_length, float *d_change,
                             void *stream)
try {
    BHRT_TRY(TemporalChangeArgs(scene, opts, d_radiance, d_variance, d_history, d_history_variance, d_length, d_out_length));
    if (!scene->dev) BHRT_TRY(bhrt_scene_upload(scene, 0));
    HIP_CHECK(hipSetDevice(SceneDevice(scene)));
    const bhrt_flat_header *H = scene->flat.hdr();
    const int W = H->camera.width, Hh = H->camera.height;
    const size_t n = (size_t)W * Hh;
    if (n == 0 || n > 0x7fffffffull) { SetError("temporal change: frame size out of range"); return BHRT_ERR_ARG; }
    hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)SceneStream(scene);
    TemporalChangeJob J;
    J.W = W; J.H = Hh; J.o = *opts;
    J.radiance = d_radiance; J.variance = d_variance; J.history = d_history; J.history_variance = d_history_variance; J.length = d_length;
    J.z = d_z; J.normal = d_normal; J.out_length = d_out_length; J.change = d_change;
    if (!d_z || !d_normal) { // the guides the caller left out, by the kernel of bhrt_first_hit* on the call's stream
        float *g = nullptr;
        BHRT_TRY(ReserveChangeScratch(scene, n, g));
        float *gz = d_z ? nullptr : g, *gn = d_normal ? nullptr : g + n;
        BHRT_TRY(bhrt_first_hit_dev(scene, gz, gn, nullptr, st));
        if (gz) J.z = gz;
        if (gn) J.normal = gn;
    }
    HIP_CHECK(TemporalChangeLaunch(J, st));
    if (!stream) HIP_CHECK(hipStreamSynchronize(st));
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_temporal_change(bhrt_scene *scene, const bhrt_change_opts *opts, const float *radiance, const float *variance, const float *history,
                         const float *history_variance, const float *length, const float *z, const float *normal, float *out_length, float *change)
try {
    BHRT_TRY(TemporalChangeArgs(scene, opts, radiance, variance, history, history_variance, length, out_length));
    if (!scene->dev) BHRT_TRY(bhrt_scene_upload(scene, 0));
    HIP_CHECK(hipSetDevice(SceneDevice(scene)));
    const bhrt_flat_header *H = scene->flat.hdr();
    const size_t n = (size_t)H->camera.width * H->camera.height;
    hipStream_t st = (hipStream_t)SceneStream(scene);
    // device copies, back to back, in floats per pixel: radiance 3, variance 3, history 3, its variance 3, length 1, z 1, normal 3, then out_length 1, change 1
    const float *const in[7] = {radiance, variance, history, history_variance, length, z, normal};
    const size_t width[9] = {3, 3, 3, 3, 1, 1, 3, 1, 1};
    DevBuf<float> d;
    BHRT_TRY(d.Reserve(n * 19));
    float *at[9];
    for (size_t k = 0, off = 0; k < 9; off += width[k] * n, k++) at[k] = d.p + off;
    for (int k = 0; k < 7; k++)
        if (in[k]) HIP_CHECK(hipMemcpyAsync(at[k], in[k], width[k] * n * sizeof(float), hipMemcpyHostToDevice, st));
    auto gin = [&](int k) -> float * { return in[k] ? at[k] : nullptr; };
    BHRT_TRY(bhrt_temporal_change_dev(scene, opts, gin(0), gin(1), gin(2), gin(3), gin(4), gin(5), gin(6), at[7], change ? at[8] : nullptr, nullptr));
    HIP_CHECK(hipMemcpy(out_length, at[7], n * sizeof(float), hipMemcpyDeviceToHost));
    if (change) HIP_CHECK(hipMemcpy(change, at[8], n * sizeof(float), hipMemcpyDeviceToHost));
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

} // extern "C"
