// capi_host.cpp — host-only entry points of include/bhrt.h: scene loading (the LoadScene seam,
// xmlload.cpp:65), scene introspection and PNG output (RenderImage::SaveImage, scene.h:628).
#include <string.h>

#include <exception>
#include <new>

#include "png_io.h"
#include "scene_internal.h"

namespace bhrt {
static thread_local std::string g_error;
void SetError(const std::string &msg) { g_error = msg; }
int AbiException()
{
    try { throw; }
    catch (const std::bad_alloc &) { SetError("out of host memory"); return BHRT_ERR_IO; }
    catch (const std::exception &e) { SetError(std::string("internal error: ") + e.what()); return BHRT_ERR_UNSUPPORTED; }
    catch (...) { SetError("internal error"); return BHRT_ERR_UNSUPPORTED; }
}
} // namespace bhrt

extern "C" {

const char *bhrt_last_error(void) { return bhrt::g_error.c_str(); }

void bhrt_default_opts(bhrt_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->spp = 32;              // Main.cpp:141
    o->gi_bounces = 3;        // Main.cpp:130
    o->internal_bounces = 16; // Main.cpp:41
    o->seed = 0;
    o->jitter = 1;
    o->gamma = 1; // Main.cpp:128
    o->photon_map = 0; // Main.cpp:51 (commented out in the reference)
    o->rank = 0;
    o->world_size = 1;
    o->tile_size = 32;
    o->samples_per_pass = 0;
}

void bhrt_default_denoise_opts(bhrt_denoise_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->iterations = 4;
    o->sigma_normal = 32.f;
    o->sigma_depth = 0.01f;
    o->sigma_luminance = 4.f; // K, sigma_*: the lowest MSE of a grid over 4-spp frames of c3_mesh_small, c3_room_small, c2_glass_small
    o->gamma = 1; // as bhrt_opts.gamma (Main.cpp:128)
}

void bhrt_default_adaptive_opts(bhrt_adaptive_opts *a)
{
    if (!a) return;
    memset(a, 0, sizeof *a);
    a->min_spp = 16;
    a->threshold = 0.01f;
    a->floor = 0.1f; // threshold, floor: the quality grid of tools/adaptive_quality.py over c3_room, c2_glass, c3_mesh
}

void bhrt_default_reproject_opts(bhrt_reproject_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->depth_tolerance = BHRT_REPROJECT_DEPTH_TOLERANCE;
    o->normal_threshold = BHRT_REPROJECT_NORMAL_THRESHOLD; // both: the MSE grid of tools/temporal_defaults.py over c3_mesh_small and c4_textured
}

void bhrt_default_temporal_opts(bhrt_temporal_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->clamp_k = BHRT_TEMPORAL_CLAMP_K;
    o->max_length = BHRT_TEMPORAL_MAX_LENGTH; // both: the same grid
    o->gamma = 1; // as bhrt_opts.gamma (Main.cpp:128)
}

void bhrt_default_spatial_variance_opts(bhrt_spatial_variance_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->radius = 3; // SVGF's 7 x 7
    o->depth_tolerance = 0.01f; // bhrt_default_denoise_opts' sigma_depth
    o->normal_threshold = BHRT_REPROJECT_NORMAL_THRESHOLD;
    o->min_length = 4.f; // the project's own numbers, not new measurements
    o->demodulate = 1;
}

void bhrt_default_change_opts(bhrt_change_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->radius = 3; // stage 3S's window
    o->sigma_lo = BHRT_CHANGE_SIGMA_LO;
    o->sigma_hi = BHRT_CHANGE_SIGMA_HI; // both: the grid of tools/temporal_change_quality.py over c3_mesh_small
    o->depth_tolerance = 0.01f; // bhrt_default_spatial_variance_opts'
    o->normal_threshold = BHRT_REPROJECT_NORMAL_THRESHOLD;
}

void bhrt_default_upsample_opts(bhrt_upsample_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->depth_tolerance = 0.01f; // bhrt_default_spatial_variance_opts'
    o->normal_threshold = BHRT_REPROJECT_NORMAL_THRESHOLD;
    o->demodulate = 1;
    o->gamma = 1; // as bhrt_opts.gamma (Main.cpp:128)
    o->fallback = BHRT_UPSAMPLE_FALLBACK_ALBEDO; // 0: the rule as it was before the switch existed
}

void bhrt_default_temporal_session_opts(bhrt_temporal_session_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o); // the four switches off: bhrt_reproject* + bhrt_temporal_accumulate*, the camera alone
    bhrt_default_reproject_opts(&o->reproject);
    bhrt_default_temporal_opts(&o->temporal);
    bhrt_default_spatial_variance_opts(&o->spatial);
    bhrt_default_denoise_opts(&o->denoise_opts);
}

int bhrt_scene_load_xml(const char *path, bhrt_scene **out) { return bhrt_scene_load_xml_ex(path, -1, out); }

int bhrt_scene_load_xml_ex(const char *path, int bvh_device, bhrt_scene **out)
try {
    if (!path || !out) { bhrt::SetError("bhrt_scene_load_xml: null argument"); return BHRT_ERR_ARG; }
    *out = nullptr;
    bhrt_scene *s = new bhrt_scene;
    std::string err;
    int rc = bhrt::LoadSceneXml(path, s->flat, err, bvh_device);
    if (rc) {
        bhrt::SetError(err);
        delete s;
        return rc == 1 ? BHRT_ERR_IO : (rc == 7 ? BHRT_ERR_HIP : BHRT_ERR_PARSE);
    }
    const bhrt_flat_header *H = s->flat.hdr();
    const bhrt_mesh *m = (const bhrt_mesh *)(s->flat.blob.data() + H->off_meshes);
    for (uint32_t i = 0; i < H->n_meshes; i++) {
        s->n_triangles += m[i].nf;
        s->n_bvh_nodes += m[i].n_bvh_nodes;
        if (m[i].bvh_depth > s->max_bvh_depth) s->max_bvh_depth = m[i].bvh_depth;
    }
    *out = s;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_clone(const bhrt_scene *src, bhrt_scene **out)
try {
    if (!src || !out) { bhrt::SetError("bhrt_scene_clone: null argument"); return BHRT_ERR_ARG; }
    bhrt_scene *s = new bhrt_scene;
    s->flat = src->flat; // the host copy only, node names and edited node transforms included: the clone is uploaded to a device of its own (one handle per GPU)
    s->n_triangles = src->n_triangles; s->n_bvh_nodes = src->n_bvh_nodes; s->max_bvh_depth = src->max_bvh_depth;
    *out = s;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

void bhrt_scene_free(bhrt_scene *s)
{
    if (!s) return;
    if (s->temporal && s->temporal_release) s->temporal_release(s->temporal); // an open temporal session's images, before the streams of the device state go
    if (s->change_scratch && s->change_scratch_release) s->change_scratch_release(s->change_scratch); // likewise: the guides bhrt_temporal_change* computed itself
    if (s->upsample_scratch && s->upsample_scratch_release) s->upsample_scratch_release(s->upsample_scratch); // likewise: the guides bhrt_upsample* computed itself
    if (s->dev) bhrt::DestroyDeviceState(s->dev);
    delete s;
}

int bhrt_scene_info(const bhrt_scene *s, bhrt_info *info)
try {
    if (!s || !info) { bhrt::SetError("bhrt_scene_info: null argument"); return BHRT_ERR_ARG; }
    const bhrt_flat_header *H = s->flat.hdr();
    memset(info, 0, sizeof *info);
    info->width = H->camera.width; info->height = H->camera.height;
    info->n_nodes = H->n_nodes; info->n_meshes = H->n_meshes; info->n_triangles = s->n_triangles;
    info->n_bvh_nodes = s->n_bvh_nodes; info->n_materials = H->n_materials; info->n_lights = H->n_lights;
    info->n_textures = H->n_textures; info->max_node_depth = H->max_node_depth; info->max_bvh_depth = s->max_bvh_depth;
    info->flat_bytes = H->total_bytes; info->n_warnings = (uint32_t)s->flat.warnings.size();
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_warning(const bhrt_scene *s, uint32_t i, const char **text)
try {
    if (!s || !text || i >= s->flat.warnings.size()) { bhrt::SetError("bhrt_scene_warning: bad index"); return BHRT_ERR_ARG; }
    *text = s->flat.warnings[i].c_str();
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_flat(const bhrt_scene *s, const void **blob, uint64_t *bytes)
try {
    if (!s || !blob || !bytes) { bhrt::SetError("bhrt_scene_flat: null argument"); return BHRT_ERR_ARG; }
    *blob = s->flat.blob.data();
    *bytes = s->flat.blob.size();
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_save_png(const char *path, const uint8_t *rgb8, int w, int h)
try {
    if (!path || !rgb8) { bhrt::SetError("bhrt_save_png: null argument"); return BHRT_ERR_ARG; }
    if (!bhrt::SavePng(path, rgb8, w, h, 3)) { bhrt::SetError(std::string("cannot write ") + path); return BHRT_ERR_IO; }
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_save_png_gray(const char *path, const uint8_t *gray, int w, int h)
try {
    if (!path || !gray) { bhrt::SetError("bhrt_save_png_gray: null argument"); return BHRT_ERR_ARG; }
    if (!bhrt::SavePng(path, gray, w, h, 1)) { bhrt::SetError(std::string("cannot write ") + path); return BHRT_ERR_IO; }
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

} // extern "C"
