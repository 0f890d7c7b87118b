// scene_edit.cpp — the entry points of include/bhrt.h that read or edit a loaded scene (bhrt::FlatScene): lens, image size, camera and shutter, node
// transforms, lights, emission, face materials.  Host code; a setter ends in the hooks of scene_internal.h, which bring an uploaded scene's device
// copy up to date and do nothing for a scene that is not uploaded.
#include <stddef.h>
#include <string.h>

#include <cmath>

#include "scene_internal.h"

using namespace bhrt;

extern "C" {

int bhrt_scene_set_lens(bhrt_scene *scene, float focaldist, float dof)
try {
    if (!scene) { SetError("bhrt_scene_set_lens: null scene"); return BHRT_ERR_ARG; }
    if (!(dof >= 0.f && dof <= 3.402823466e38f)) { SetError("bhrt_scene_set_lens: dof must be finite and >= 0"); return BHRT_ERR_ARG; }
    if (!(focaldist >= -3.402823466e38f && focaldist <= 3.402823466e38f)) { SetError("bhrt_scene_set_lens: focaldist is not finite"); return BHRT_ERR_ARG; }
    bhrt_flat_header *H = reinterpret_cast<bhrt_flat_header *>(scene->flat.blob.data());
    if (focaldist > 0.f) H->camera.focaldist = focaldist;
    H->camera.dof = dof;
    DeriveCameraFrame(H->camera);
    if (scene->flat.shutter) { // pose 1 takes the scene's focaldist and dof: its frame follows
        bhrt_camera &c1 = scene->flat.shutter_cam;
        c1.focaldist = H->camera.focaldist; c1.dof = H->camera.dof;
        DeriveCameraFrame(c1);
    }
    RefreshCamera(scene);
    RefreshShutter(scene);
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

// The image size.  The loader takes any positive int; the limits are the render's and the image-space entry points': a pixel
// index is 31 bits everywhere, and a side of at most 2^24 keeps every pixel coordinate exact as a float32 and the tile arithmetic inside an int.
int bhrt_scene_set_resolution(bhrt_scene *scene, int32_t width, int32_t height)
try {
    if (!scene) { SetError("bhrt_scene_set_resolution: null scene"); return BHRT_ERR_ARG; }
    if (width < 1 || height < 1) { SetError("bhrt_scene_set_resolution: width and height must be >= 1"); return BHRT_ERR_ARG; }
    if (width > BHRT_MAX_IMAGE_SIDE || height > BHRT_MAX_IMAGE_SIDE || (int64_t)width * height > (int64_t)BHRT_MAX_IMAGE_PIXELS) {
        SetError("bhrt_scene_set_resolution: at most 2^24 pixels a side and 2^31 - 1 pixels in all");
        return BHRT_ERR_ARG;
    }
    if (scene->prog.open) { SetError("bhrt_scene_set_resolution: a progressive session is open on this scene (bhrt_progressive_end first)"); return BHRT_ERR_ARG; }
    if (scene->temporal) { SetError("bhrt_scene_set_resolution: a temporal session is open on this scene (bhrt_temporal_end first)"); return BHRT_ERR_ARG; }
    bhrt_flat_header *H = reinterpret_cast<bhrt_flat_header *>(scene->flat.blob.data());
    H->camera.width = width; H->camera.height = height;
    DeriveCameraFrame(H->camera);
    if (scene->flat.shutter) { // pose 1 takes the scene's size: its frame follows
        bhrt_camera &c1 = scene->flat.shutter_cam;
        c1.width = width; c1.height = height;
        DeriveCameraFrame(c1);
    }
    // the kernels' camera and shutter are arguments; every per-pixel device buffer is sized by the call that uses it
    RefreshCamera(scene);
    RefreshShutter(scene);
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

// ---- the camera and its shutter
static bool Finite3(const float *v) { return v && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
// Pose 1 of a shutter: the camera `base` (fov, focaldist, dof, size) at (pos, target, up); "" = a valid pose, else what is wrong
static const char *PoseCamera(const bhrt_camera &base, const float pos[3], const float target[3], const float up[3], bhrt_camera &out)
{
    if (!pos || !target || !up) return "a NULL pointer";
    if (!Finite3(pos) || !Finite3(target) || !Finite3(up)) return "a component that is not finite";
    out = base;
    if (!SetCameraPose(out, pos, target, up, base.fov)) return "target == pos, or up parallel to target - pos";
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(out.dir[k]) || !std::isfinite(out.up[k]) || !std::isfinite(out.top_left[k]) || !std::isfinite(out.dd_x[k]) || !std::isfinite(out.dd_y[k]))
            return "a camera frame that is not finite";
    return "";
}

int bhrt_scene_set_camera(bhrt_scene *scene, const float pos[3], const float target[3], const float up[3], float fov)
try {
    if (!scene) { SetError("bhrt_scene_set_camera: null scene"); return BHRT_ERR_ARG; }
    if (!std::isfinite(fov) || fov >= 180.f) { SetError("bhrt_scene_set_camera: fov must be finite and below 180 (<= 0 keeps the current one)"); return BHRT_ERR_ARG; }
    bhrt_flat_header *H = reinterpret_cast<bhrt_flat_header *>(scene->flat.blob.data());
    bhrt_camera base = H->camera, cam, cam1 = scene->flat.shutter_cam;
    if (fov > 0.f) base.fov = fov;
    const char *bad = PoseCamera(base, pos, target, up, cam);
    if (*bad) { SetError(std::string("bhrt_scene_set_camera: ") + bad); return BHRT_ERR_ARG; }
    if (scene->flat.shutter) { // pose 1 takes the new fov; the pair that results must still be less than a quarter turn apart
        bad = PoseCamera(base, scene->flat.shutter_pos, scene->flat.shutter_target, scene->flat.shutter_up, cam1);
        if (!*bad) bad = ShutterPairError(cam, cam1);
        if (*bad) { SetError(std::string("bhrt_scene_set_camera: with the shutter's pose 1: ") + bad); return BHRT_ERR_ARG; }
    }
    H->camera = cam; // nothing above changed the scene
    scene->flat.shutter_cam = cam1;
    // the camera position through every node's chain and the kernels' camera; nothing else is uploaded again
    const int rc = RefreshCamChain(scene);
    if (rc) return rc;
    RefreshCamera(scene);
    RefreshShutter(scene);
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_set_shutter(bhrt_scene *scene, int on, const float pos1[3], const float target1[3], const float up1[3])
try {
    if (!scene) { SetError("bhrt_scene_set_shutter: null scene"); return BHRT_ERR_ARG; }
    bhrt::FlatScene &F = scene->flat;
    if (!on) {
        F.shutter = 0;
        memset(F.shutter_pos, 0, sizeof F.shutter_pos); memset(F.shutter_target, 0, sizeof F.shutter_target); memset(F.shutter_up, 0, sizeof F.shutter_up);
        memset(&F.shutter_cam, 0, sizeof F.shutter_cam);
        RefreshShutter(scene);
        return BHRT_OK;
    }
    bhrt_camera cam1;
    const char *bad = PoseCamera(F.hdr()->camera, pos1, target1, up1, cam1);
    if (!*bad) bad = ShutterPairError(F.hdr()->camera, cam1);
    if (*bad) { SetError(std::string("bhrt_scene_set_shutter: ") + bad); return BHRT_ERR_ARG; }
    F.shutter = 1;
    for (int k = 0; k < 3; k++) { F.shutter_pos[k] = pos1[k]; F.shutter_target[k] = target1[k]; F.shutter_up[k] = up1[k]; }
    F.shutter_cam = cam1;
    RefreshShutter(scene);
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_get_shutter(const bhrt_scene *scene, int *on, float pose1[9], float frame1[12])
try {
    if (!scene) { SetError("bhrt_scene_get_shutter: null scene"); return BHRT_ERR_ARG; }
    const bhrt::FlatScene &F = scene->flat;
    const bhrt_camera &c = F.shutter_cam;
    if (on) *on = F.shutter;
    if (pose1) for (int k = 0; k < 3; k++) { pose1[k] = F.shutter_pos[k]; pose1[3 + k] = F.shutter_target[k]; pose1[6 + k] = F.shutter_up[k]; }
    if (frame1) for (int k = 0; k < 3; k++) { frame1[k] = c.pos[k]; frame1[3 + k] = c.top_left[k]; frame1[6 + k] = c.dd_x[k]; frame1[9 + k] = c.dd_y[k]; }
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_get_camera_frame(const bhrt_scene *scene, float frame[12])
try {
    if (!scene || !frame) { SetError("bhrt_scene_get_camera_frame: null argument"); return BHRT_ERR_ARG; }
    const bhrt_camera &c = scene->flat.hdr()->camera;
    for (int k = 0; k < 3; k++) { frame[k] = c.pos[k]; frame[3 + k] = c.top_left[k]; frame[6 + k] = c.dd_x[k]; frame[9 + k] = c.dd_y[k]; }
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

// ---- moving objects: node names and transforms
int bhrt_scene_node_index(const bhrt_scene *scene, const char *name, int32_t *index)
try {
    if (!scene || !name || !index) { SetError("bhrt_scene_node_index: null argument"); return BHRT_ERR_ARG; }
    const std::vector<std::string> &names = scene->flat.node_names;
    for (size_t i = 0; i < names.size(); i++) // the first of that name in the blob's pre-order
        if (names[i] == name) { *index = (int32_t)i; return BHRT_OK; }
    SetError(std::string("bhrt_scene_node_index: no node named \"") + name + "\"");
    return BHRT_ERR_ARG;
} catch (...) { return bhrt::AbiException(); }

static const bhrt_node *HostNodes(const bhrt_scene *scene) { return (const bhrt_node *)(scene->flat.blob.data() + scene->flat.hdr()->off_nodes); }

int bhrt_scene_get_node_transform(const bhrt_scene *scene, int32_t node, bhrt_xform *out)
try {
    if (!scene || !out) { SetError("bhrt_scene_get_node_transform: null argument"); return BHRT_ERR_ARG; }
    if (node < 0 || (uint32_t)node >= scene->flat.hdr()->n_nodes) { SetError("bhrt_scene_get_node_transform: node index out of range"); return BHRT_ERR_ARG; }
    *out = HostNodes(scene)[node].xf;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_get_node_transforms(const bhrt_scene *scene, bhrt_xform *out, uint32_t capacity, uint32_t *n)
try {
    if (!scene) { SetError("bhrt_scene_get_node_transforms: null scene"); return BHRT_ERR_ARG; }
    const uint32_t n_nodes = scene->flat.hdr()->n_nodes;
    if (n) *n = n_nodes;
    if (capacity < n_nodes || (n_nodes > 0 && !out)) { SetError("bhrt_scene_get_node_transforms: room for " + std::to_string(n_nodes) + " records is needed"); return BHRT_ERR_ARG; }
    for (uint32_t k = 0; k < n_nodes; k++) out[k] = HostNodes(scene)[k].xf;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_set_node_transform(bhrt_scene *scene, int32_t node, const float tm[9], const float pos[3], const bhrt_xform_op *ops, uint32_t n_ops)
try {
    if (!scene) { SetError("bhrt_scene_set_node_transform: null scene"); return BHRT_ERR_ARG; }
    const bhrt_flat_header *H = scene->flat.hdr();
    if (node < 0 || (uint32_t)node >= H->n_nodes) { SetError("bhrt_scene_set_node_transform: node index out of range"); return BHRT_ERR_ARG; }
    bhrt_xform xf;
    const char *bad = bhrt::BuildNodeXform(tm, pos, ops, n_ops, xf);
    if (*bad) { SetError(std::string("bhrt_scene_set_node_transform: ") + bad); return BHRT_ERR_ARG; }
    const size_t off = (size_t)H->off_nodes + (size_t)node * sizeof(bhrt_node) + offsetof(bhrt_node, xf);
    memcpy(scene->flat.blob.data() + off, &xf, sizeof xf); // nothing above changed the scene
    return RefreshNodeXform(scene, off, xf); // the node's 84 bytes and the camera position through every node's chain; nothing else is uploaded again
} catch (...) { return bhrt::AbiException(); }

// ---- lights: named by their index in document order (FlatScene::lights); the blob holds them sorted
int bhrt_scene_light_count(const bhrt_scene *scene, int32_t *n)
try {
    if (!scene || !n) { SetError("bhrt_scene_light_count: null argument"); return BHRT_ERR_ARG; }
    *n = (int32_t)scene->flat.lights.size();
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_light_index(const bhrt_scene *scene, const char *name, int32_t *index)
try {
    if (!scene || !name || !index) { SetError("bhrt_scene_light_index: null argument"); return BHRT_ERR_ARG; }
    const std::vector<bhrt::FlatScene::Light> &lights = scene->flat.lights;
    for (size_t i = 0; i < lights.size(); i++) // the first of that name in document order
        if (lights[i].name == name) { *index = (int32_t)i; return BHRT_OK; }
    SetError(std::string("bhrt_scene_light_index: no light named \"") + name + "\"");
    return BHRT_ERR_ARG;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_get_light(const bhrt_scene *scene, int32_t light, bhrt_light_info *out)
try {
    if (!scene || !out) { SetError("bhrt_scene_get_light: null argument"); return BHRT_ERR_ARG; }
    if (light < 0 || (size_t)light >= scene->flat.lights.size()) { SetError("bhrt_scene_get_light: light index out of range"); return BHRT_ERR_ARG; }
    const bhrt::FlatScene::Light &l = scene->flat.lights[(size_t)light];
    memset(out, 0, sizeof *out);
    out->type = l.type;
    for (int k = 0; k < 3; k++) { out->intensity[k] = l.intensity[k]; out->vec[k] = l.vec[k]; }
    out->size = l.size;
    out->blob_index = l.blob_index;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_set_light(bhrt_scene *scene, int32_t light, const float intensity[3], const float vec[3], float size)
try {
    if (!scene) { SetError("bhrt_scene_set_light: null scene"); return BHRT_ERR_ARG; }
    const char *bad = bhrt::SetLight(scene->flat, light, intensity, vec, size);
    if (*bad) { SetError(std::string("bhrt_scene_set_light: ") + bad); return BHRT_ERR_ARG; }
    return RefreshLights(scene); // the lights block, the pick table and the kernels' all_light_intensity; nothing else is uploaded again
} catch (...) { return bhrt::AbiException(); }

// ---- the emission term: scene state beside the blob
int bhrt_scene_set_emissive(bhrt_scene *scene, int on)
try {
    if (!scene) { SetError("bhrt_scene_set_emissive: null scene"); return BHRT_ERR_ARG; }
    scene->flat.emissive = on ? 1 : 0;
    return RefreshEmission(scene);
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_material_index(const bhrt_scene *scene, const char *name, int32_t *index)
try {
    if (!scene || !name || !index) { SetError("bhrt_scene_material_index: null argument"); return BHRT_ERR_ARG; }
    const std::vector<std::string> &names = scene->flat.material_names;
    for (size_t i = 0; i < names.size(); i++) // the first of that name, as the loader's own lookup (xmlload.cpp:101-107)
        if (names[i] == name) { *index = (int32_t)i; return BHRT_OK; }
    SetError(std::string("bhrt_scene_material_index: no material named \"") + name + "\"");
    return BHRT_ERR_ARG;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_set_material_emission(bhrt_scene *scene, int32_t material, const float rgb[3])
try {
    if (!scene || !rgb) { SetError("bhrt_scene_set_material_emission: null argument"); return BHRT_ERR_ARG; }
    if (material < 0 || (size_t)material >= scene->flat.emission.size()) { SetError("bhrt_scene_set_material_emission: material index out of range"); return BHRT_ERR_ARG; }
    bhrt_texcolor &e = scene->flat.emission[(size_t)material];
    e.color[0] = rgb[0]; e.color[1] = rgb[1]; e.color[2] = rgb[2];
    e.map = -1;
    return RefreshEmission(scene);
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_get_material_emission(const bhrt_scene *scene, int32_t material, float rgb[3], int32_t *texmap)
try {
    if (!scene) { SetError("bhrt_scene_get_material_emission: null scene"); return BHRT_ERR_ARG; }
    if (material < 0 || (size_t)material >= scene->flat.emission.size()) { SetError("bhrt_scene_get_material_emission: material index out of range"); return BHRT_ERR_ARG; }
    const bhrt_texcolor &e = scene->flat.emission[(size_t)material];
    if (rgb) { rgb[0] = e.color[0]; rgb[1] = e.color[1]; rgb[2] = e.color[2]; }
    if (texmap) *texmap = e.map;
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

// ---- face materials: scene state beside the blob
int bhrt_scene_set_face_materials(bhrt_scene *scene, int on)
try {
    if (!scene) { SetError("bhrt_scene_set_face_materials: null scene"); return BHRT_ERR_ARG; }
    scene->flat.face_materials = on ? 1 : 0;
    return RefreshFaceMaterials(scene);
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_submaterial_count(const bhrt_scene *scene, int32_t material, int32_t *n)
try {
    if (!scene || !n) { SetError("bhrt_scene_submaterial_count: null argument"); return BHRT_ERR_ARG; }
    const std::vector<int32_t> &first = scene->flat.sub_first;
    if (material < 0 || (size_t)material + 1 >= first.size()) { SetError("bhrt_scene_submaterial_count: material index out of range"); return BHRT_ERR_ARG; }
    *n = first[(size_t)material + 1] - first[(size_t)material];
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_scene_get_submaterial(const bhrt_scene *scene, int32_t material, int32_t sub, struct bhrt_material *out, uint32_t *face_end)
try {
    if (!scene) { SetError("bhrt_scene_get_submaterial: null scene"); return BHRT_ERR_ARG; }
    const std::vector<int32_t> &first = scene->flat.sub_first;
    if (material < 0 || (size_t)material + 1 >= first.size()) { SetError("bhrt_scene_get_submaterial: material index out of range"); return BHRT_ERR_ARG; }
    if (sub < 0 || sub >= first[(size_t)material + 1] - first[(size_t)material]) { SetError("bhrt_scene_get_submaterial: sub-material index out of range"); return BHRT_ERR_ARG; }
    const size_t k = (size_t)(first[(size_t)material] + sub);
    if (out) *out = scene->flat.sub_materials[k];
    if (face_end) *face_end = scene->flat.sub_face_end[k];
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

} // extern "C"
