// scene_host.h — host front-end: XML scene -> flattened scene blob (include/bhrt_flat.h).
// Mirrors the reference's xmlload surface (xmlload.cpp:65-582) with its own reader.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "bhrt_flat.h"

struct bhrt_xform_op; // include/bhrt.h

namespace bhrt {

struct FlatScene {
    std::vector<uint8_t> blob;
    std::vector<std::string> warnings; // the reference printf()s and carries on (xmlload.cpp:212-214,570-573)
    // Scene state beside the blob: the <emission> of every material (xmlload.cpp:344-348; its map is an index into the blob's
    // texmaps[]), the materials' XML names, and the switch of the emission term (bhrt_scene_set_emissive).  The blob holds none of it: its
    // bytes are what they were before the term existed.
    std::vector<bhrt_texcolor> emission;      // [n_materials]
    std::vector<std::string> material_names;  // [n_materials]
    std::vector<std::string> node_names;      // [n_nodes]: the <object name=> of every node in the blob's pre-order, "" where there is none
    int emissive = 0;
    // Face materials, beside the blob too: the sub-materials of every MultiMtl (one per `newmtl` of the mesh's .mtl, converted as
    // the blob's record is from the first; xmlload.cpp:219-250) and the cumulative face counts that group the mesh's faces by them
    // (cyTriMesh.h:461-487).  Material m owns entries [sub_first[m], sub_first[m + 1]) of the two arrays; none for a Blinn material or an empty
    // MultiMtl.  Entry sub_first[m] repeats the blob's record of m byte for byte.  face_materials: the switch (bhrt_scene_set_face_materials).
    std::vector<int32_t> sub_first;           // [n_materials + 1]
    std::vector<bhrt_material> sub_materials; // [sub_first[n_materials]]
    std::vector<uint32_t> sub_face_end;       // likewise: faces [sub_face_end[i - 1], sub_face_end[i]) of the mesh shade with sub-material i
    int face_materials = 0;
    // The global gather, beside the blob too: the switch and the gather radius (bhrt_scene_set_global_gather).  The map itself
    // is device state (DeviceState::gmap): a clone carries these two and no map.
    int global_gather = 0;
    float global_radius = 0.5f; // MAX_Area, MtlBlinn.cpp:29
    // The camera shutter, beside the blob too: the switch, pose 1 as the caller gave it (position, target, up: the camera at the
    // end of the exposure; pose 0 is the blob's camera) and the camera derived from it with the blob camera's fov, focaldist, dof and size
    // (SetCameraPose).  shutter_cam is derived again whenever bhrt_scene_set_lens or bhrt_scene_set_camera changes what it depends on.
    int shutter = 0;
    float shutter_pos[3] = {0, 0, 0}, shutter_target[3] = {0, 0, 0}, shutter_up[3] = {0, 0, 0};
    bhrt_camera shutter_cam = {};
    // The lights, beside the blob too: every <light> the loader accepted, in document order, as LoadLight read it (a direct
    // light's vec normalised), with its name= ("" when absent).  The blob's lights[] is this list sorted by Gray() (CalculateLightsIntensity);
    // blob_index says where each light stands there now.  SetLight edits a record and derives the blob's lights[] and all_light_intensity again.
    struct Light {
        std::string name;
        int32_t type = 0; // BHRT_LIGHT_*
        float intensity[3] = {0, 0, 0}, vec[3] = {0, 0, 0}, size = 0;
        int32_t blob_index = 0;
    };
    std::vector<Light> lights; // [n_lights]
    const bhrt_flat_header *hdr() const { return reinterpret_cast<const bhrt_flat_header *>(blob.data()); }
};

// Returns 0 on success (like LoadScene returning 1), non-zero + err on failure.
// bvh_device >= 0: the mesh BVHs are built on that HIP device (bvh_build.hip) instead of by BuildBvh below; same result.
int LoadSceneXml(const char *path, FlatScene &out, std::string &err, int bvh_device = -1);

// top_left, dd_x, dd_y of a camera whose other fields are set (the loader's own derivation; bhrt_scene_set_lens runs it again)
void DeriveCameraFrame(bhrt_camera &C);
// pos, dir, up and fov of C from a position, a target and an up vector, as the loader treats the <camera> tags, then DeriveCameraFrame;
// false: target == pos, or up parallel to target - pos
bool SetCameraPose(bhrt_camera &C, const float pos[3], const float target[3], const float up[3], float fov);
// The pair of poses of a shutter: "" when dir, dd_x and dd_y of the two cameras each have a positive dot product and every value of
// b's frame is finite (no interpolated axis can then be zero), else what is wrong
const char *ShutterPairError(const bhrt_camera &a, const bhrt_camera &b);

// The record bhrt_scene_set_node_transform stores: (tm, pos) — both NULL = the identity — with itm = MatInverse(tm), then the ops in
// order through LoadTransform's own Scale / Rotate / Translate, stored as the loader stores a node's.  "" and `out` written when every input
// and every value of the result is finite, else what is wrong and `out` untouched.
const char *BuildNodeXform(const float tm[9], const float pos[3], const bhrt_xform_op *ops, uint32_t n_ops, bhrt_xform &out);

// What bhrt_scene_set_light does to the host scene: the values given (intensity / vec NULL, size < 0: kept; a direct light's vec
// through the loader's normalized()) go into F.lights[light], then the loader's own sort-and-sum and store run on the document-order list and
// rewrite the blob's lights[] and all_light_intensity in place.  "" when done, else what is wrong and F untouched.
const char *SetLight(FlatScene &F, int32_t light, const float intensity[3], const float vec[3], float size);

// OBJ mesh -> arrays, same face/index rules as cyTriMesh::LoadFromFileObj (cyTriMesh.h:263-547)
struct HostMesh {
    std::vector<float> v, vn, vt;       // xyz triples
    std::vector<uint32_t> f, fn, ft;    // index triples
    struct Mtl {
        std::string name;
        float Ka[3] = {0, 0, 0}, Kd[3] = {1, 1, 1}, Ks[3] = {0, 0, 0}, Tf[3] = {0, 0, 0};
        float Ns = 0, Ni = 1;
        int illum = 2;
        std::string map_Kd, map_Ks;
    };
    std::vector<Mtl> mtls;
    std::vector<int> mcfc; // material cumulative face count
    float bound_min[3] = {1, 1, 1}, bound_max[3] = {0, 0, 0};
    // BVH (cyBVH.h:122-142), node 0 unused, root = 1
    std::vector<bhrt_bvh_node> bvh;
    std::vector<uint32_t> elems;
    uint32_t bvh_depth = 0;
    bool had_vt = true;
};
bool LoadObj(const char *path, bool load_mtl, HostMesh &m, std::string &err);
void ComputeNormals(HostMesh &m);     // cyTriMesh.h:248-261
void ComputeBoundingBox(HostMesh &m); // cyTriMesh.h:229-246
void BuildBvh(HostMesh &m, unsigned max_elems_per_node = 4); // cyBVH.h:122-142, objects.h:59
int BuildBvhDevice(HostMesh &m, unsigned max_elems_per_node, int device); // the same tree from the device build (bvh_build.hip); 0 = ok

} // namespace bhrt
