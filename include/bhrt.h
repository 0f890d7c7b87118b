/* bhrt.h — C ABI of the MI355X-native render path (libbhrt.so).
 *
 * Drop-in boundary for the per-pixel render path of BosonHBC/BHRayTracer.  The reference has
 * no FFI: its seam is three free functions plus `extern` globals shared between the UI and the
 * renderer (all paths relative to /root/reference/BHRayTracer):
 *     int  LoadScene(char const *filename);   Main.cpp:43, xmlload.cpp:65
 *     void BeginRender();                     Main.cpp:178   (called from viewport.cpp:425-449)
 *     void StopRender();                      Main.cpp:243   (here: bhrt_progressive_end, the end of a resumable frame)
 *     globals rootNode, camera, renderImage, lights, materials, ...   Main.cpp:17-37
 * and, one level down, the plugin virtuals of Scenes/scene.h (Object::IntersectRay :256,
 * Light::Illuminate :268, Material::Shade :291, Texture::Sample :314) reached through
 * recursive() (Main.cpp:389) and GenLight::Shadow (Lights/GenLight.cpp:10).
 * This header exports the same units with explicit ownership (an opaque scene handle instead of
 * globals) and runtime options instead of the reference's compile-time #defines.
 *
 * Threading: calls on one bhrt_scene must not overlap; different scenes are independent.
 * Errors: every function returns 0 on success, non-zero otherwise; bhrt_last_error() gives the
 * message for the calling thread.  Compute entry points fail (never fall back to the CPU) when
 * no gfx950 device is usable.
 */
#ifndef BHRT_H
#define BHRT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bhrt_scene bhrt_scene;

/* BHRT_HIT_* as in Scenes/scene.h:57-60 */
#define BHRT_SIDE_FRONT 1
#define BHRT_SIDE_BACK 2
#define BHRT_SIDE_BOTH 3

enum {
    BHRT_OK = 0,
    BHRT_ERR_IO = 1,
    BHRT_ERR_PARSE = 2,
    BHRT_ERR_ARG = 3,
    BHRT_ERR_NO_DEVICE = 4,
    BHRT_ERR_HIP = 5,
    BHRT_ERR_UNSUPPORTED = 6,
    BHRT_ERR_OVERFLOW = 7
};

typedef struct bhrt_info { /* replaces reading the globals camera / rootNode / lights (Main.cpp:17-30) */
    int32_t width, height;
    uint32_t n_nodes, n_meshes, n_triangles, n_bvh_nodes, n_materials, n_lights, n_textures;
    uint32_t max_node_depth, max_bvh_depth;
    uint64_t flat_bytes;
    uint32_t n_warnings;
} bhrt_info;

/* Runtime form of the reference's compile-time knobs (SURVEY.md §5 "Config / flags"). */
typedef struct bhrt_opts {
    int32_t spp;              /* PT_SampleCount (Main.cpp:141), default 32 */
    int32_t gi_bounces;       /* GIBounceCount (Main.cpp:130), default 3 */
    int32_t internal_bounces; /* INTERNAL_REFLECTION_BOUNCE (Main.cpp:41), default 16 */
    uint32_t seed;            /* stream seed of include/bhrt_rng.h (the reference never calls srand) */
    int32_t jitter;           /* 1 = RandomPositionInPixel (Main.cpp:132-139); 0 = ray through the pixel corner */
    int32_t gamma;            /* USE_GamaCorrection (Main.cpp:128): 1 = pow(c, 1/2.2f) before Color24 */
    int32_t photon_map;       /* USE_PhotonMap (Main.cpp:51): 1 = gather from the caustic map built by bhrt_photon_build */
    /* tile partition: this process renders tiles t with t % world_size == rank */
    int32_t rank, world_size;
    int32_t tile_size;        /* square tile edge in pixels, default 32 */
    int32_t samples_per_pass; /* upper bound on camera samples in flight per wavefront pass.  Device memory per sample: ~1 KB (1.4 KB with the photon map or the global gather)
                                 when six Shade() frames are provided per sample slot.  0 = choose: what the frame needs, at most 2^28 slots, halved until
                                 the workspace fits into 85 % of the free memory — with six frames per slot that is 2^27 (~138 GB / 186 GB); a frame too
                                 large for one such pass (config 4: 2.65e8 samples per GPU) provides the frames per slot its earlier passes needed + 30 %
                                 instead (1.7 for config 4: 2^28 slots in 180 GB) and is one pass from its second render on */
    int32_t timers;           /* HIP-event kernel timers of bhrt_stats: 0 = seconds_shade only (default; an event between two kernels
                               * idles the GPU ~6 us), 1 = all kernel groups, -1 = none */
    int32_t photon_exact;     /* caustic gather of queries with >= 1000 photons inside the radius: 0 (default) = the same photon SET as
                               * LocatePhotons (cyPhotonMap.h:421-498) found by a wave-cooperative selection, sums in a fixed order (irradiance
                               * equal to a few ulp); 1 = the reference's candidate-heap history replayed lane by lane, identical bits, ~5x slower */
    int32_t leaf_skip;        /* 1 = the mesh walks leave out a box-missed LEAF sibling (TriObj.cpp:245-248,263-266,286-300) when its visit provably
                               * accepts nothing (bhrt_flat.h: bhrt_mesh::skip_*; proof in scene_host.cpp::ComputeLeafSkip).  Same hit records either
                               * way; 0 (default): on the scenes measured the test costs more instructions than the visits it saves */
    float photon_radius;      /* gather radius of the caustic term, MAX_Area (MtlBlinn.cpp:29); 0 = the reference's 0.5.  The photon count of an estimate,
                               * MAX_PhotonCountInArea = 1000 (MtlBlinn.cpp:28), is a TEMPLATE argument in the reference too (EstimateIrradiance<1000>,
                               * MtlBlinn.cpp:333) and sizes the candidate lists of the kernels: compile-time here as there (device_photon.h: BHRT_PHOTON_K) */
    int32_t lens;             /* thin-lens camera: 0 (default) = pinhole, BeginRender's frame whatever the scene's <dof>; 1 = when camera.dof > 0 the
                               * ray of a sample starts on the disc of radius dof around the eye, in the camera's x/y plane, and goes through the sample's point on
                               * the image plane, which lies at <focaldist> (Main.cpp:181-189): the viewport's preview (viewport.cpp:236-243) as a render.  With
                               * dof == 0 the render is the pinhole one, bit for bit.  Any other value, or 1 with a negative / non-finite dof: BHRT_ERR_ARG,
                               * before a device is touched.  The images beside the colour image (bhrt_first_hit*) and the guides the denoiser computes itself stay the pinhole ray's;
                               * bhrt_guides* forms guide images from the lens rays */
} bhrt_opts;

typedef struct bhrt_stats {
    uint64_t closest_rays;  /* top-level recursive() equivalents traced (Main.cpp:389) */
    uint64_t shadow_rays;   /* GenLight::Shadow equivalents traced (GenLight.cpp:10) */
    uint64_t shade_calls;   /* MtlBlinn::Shade equivalents evaluated */
    uint64_t camera_samples;
    uint32_t passes, wave_iterations;
    double seconds_total;    /* wall clock of the call, scene already resident */
    double seconds_trace_closest, seconds_trace_shadow, seconds_shade, seconds_other; /* HIP-event kernel time */
    uint64_t launches_trace_closest, launches_trace_shadow;
    /* caustic gather (EstimateIrradiance<1000>, DataStructure/cyPhotonMap.h:332-382; called at MtlBlinn.cpp:334) */
    double seconds_photon_gather;  /* wall clock of the gather of every pass, HIP events */
    double seconds_photon_heavy;   /* ... of which in the pass for queries with >= 1000 photons inside the radius */
    uint64_t photon_queries;       /* Shade() frames that asked for the caustic term */
    uint64_t photon_heavy_queries; /* queries that met 1000 photons */
    uint64_t photon_wave_queries;  /* queries whose walk was handed to a whole wave */
    uint64_t photon_exact_queries; /* heavy queries answered by the exact replay of the reference's candidate heap */
    uint64_t photon_nodes_visited; /* kd-tree nodes whose photon was examined (24 B each: SURVEY.md 8d) */
    uint64_t deferred_rays;        /* rays parallel to a coordinate axis of the mesh they enter (Box.cpp:13-28 ignores that axis: a walk of
                                    * nearly the whole BVH): traced in wave steps of their own at the end of their pass */
    /* the lane pass of the gather (k_photon_gather_fast) alone: queries it answered, kd nodes it examined, and — only with the knob "gather_stats"
     * (bhrt_scene_knob: a statistics instantiation of the kernel, 7 % slower) — the photons those answers were made of */
    uint64_t photon_lane_queries, photon_lane_nodes, photon_found;
    uint64_t launches_resolve_fused; /* passes whose root frames were resolved straight into the image (k_resolve_frames, knob "fused_resolve") */
    /* the global gather (bhrt_scene_set_global_gather): EstimateIrradiance<1000> on the global map where gi < 0 cuts the GI term */
    uint64_t global_gather_queries;       /* Shade() frames that asked for the global term */
    uint64_t global_gather_heavy_queries; /* queries that met 1000 photons */
    double seconds_global_gather;         /* wall clock of the gather of every pass, HIP events */
} bhrt_stats;

/* compact hit record written by the trace kernel (SoA on the device: one array per field) */
typedef struct bhrt_hits {
    float *t;         /* HitInfo::z = ray parameter, BIGFLOAT on a miss */
    int32_t *node;    /* flattened node index (DFS pre-order of the Node tree), -1 on a miss */
    int32_t *prim;    /* triangle id for mesh hits, -1 otherwise */
    int32_t *front;   /* HitInfo::front */
} bhrt_hits;

const char *bhrt_last_error(void);
void bhrt_default_opts(bhrt_opts *opts);

/* ---- scene (= LoadScene + the globals it fills) ------------------------------------------------ */
int bhrt_scene_load_xml(const char *path, bhrt_scene **out);            /* xmlload.cpp:65 */
/* same, with the mesh BVHs (TriObj::Load -> cyBVHTriMesh::SetMesh(this, 4), objects.h:59) built on HIP device `bvh_device`
 * instead of by the host front-end; -1 = host.  The flattened scene is byte-identical either way. */
int bhrt_scene_load_xml_ex(const char *path, int bvh_device, bhrt_scene **out);
/* cyBVH::Build (DataStructure/cyBVH.h:122-142; SplitTempNode :242-278, ConvertTempData :281-291, MeanSplit :295-328) on the
 * device, node for node: ids, boxes, leaf ranges and element order equal the reference's recursive build.  Host pointers.
 * vertices: n_vertices xyz triples; faces: n_faces index triples; nodes_out (bhrt_bvh_node of include/bhrt_flat.h): capacity
 * >= 2 * n_faces + 1 is always enough (node 0 unused, root = 1; *n_nodes = nodes without slot 0); elems_out: n_faces. */
struct bhrt_bvh_node;
int bhrt_bvh_build(const float *vertices, uint32_t n_vertices, const uint32_t *faces, uint32_t n_faces, uint32_t max_per_leaf, int device,
                   struct bhrt_bvh_node *nodes_out, uint32_t node_capacity, uint32_t *n_nodes, uint32_t *elems_out, uint32_t *depth);
/* A second handle on the same loaded scene (host copy of the flattened scene, no device state): the reference's globals are
 * one per process; a host that drives several GPUs keeps one handle per device (bhrt_scene_upload) — see csrc/bhrt_main.cpp. */
int bhrt_scene_clone(const bhrt_scene *scene, bhrt_scene **out);
void bhrt_scene_free(bhrt_scene *scene);
int bhrt_scene_info(const bhrt_scene *scene, bhrt_info *info);
int bhrt_scene_warning(const bhrt_scene *scene, uint32_t i, const char **text); /* the reference printf()s these */
int bhrt_scene_flat(const bhrt_scene *scene, const void **blob, uint64_t *bytes); /* host copy of the HBM image (include/bhrt_flat.h) */
/* The camera's <focaldist> and <dof> of a loaded scene (xmlload.cpp:119-120): focaldist <= 0 keeps the current one; dof < 0 or not finite, a NaN
 * or infinite focaldist: BHRT_ERR_ARG.  The camera frame (top_left, dd_x, dd_y) is derived again by the loader's own code, so bhrt_scene_flat is
 * afterwards byte-identical to the blob of the same XML with the two values written into its <camera>.  Needs no device; on an uploaded scene
 * the device's copy of the camera is refreshed (nothing else is uploaded again).  The pointer bhrt_scene_flat returned stays valid. */
int bhrt_scene_set_lens(bhrt_scene *scene, float focaldist, float dof);
/* The camera's <width> and <height> of a loaded scene (xmlload.cpp:121-122): the image size of every later render and image-space call.  The
 * camera frame is derived again by the loader's own code, and so is pose 1 of an active shutter, so bhrt_scene_flat is afterwards byte-identical
 * to the blob of the same XML with the two values written into its <camera>, bhrt_scene_info reports the new size and bhrt_scene_clone carries
 * it.  The pointer bhrt_scene_flat returned stays valid.  Needs no device; on an uploaded scene only the device's copy of the camera, and of the
 * shutter if one is on, is refreshed: every per-pixel device buffer of a scene is sized by the call that uses it (DESIGN.md 25 lists them).
 * BHRT_ERR_ARG, with nothing changed and before any device is touched: a NULL scene; a width or height < 1; a width or height above
 * BHRT_MAX_IMAGE_SIDE, or width * height above BHRT_MAX_IMAGE_PIXELS (the loader itself takes any positive int; these are what the render and
 * the image-space entry points accept: a pixel index is 31 bits everywhere, and a pixel coordinate must be exact as a float32); an open
 * progressive or temporal session on the scene, whose per-pixel state has the old size (end it first). */
#define BHRT_MAX_IMAGE_SIDE 16777216      /* 2^24 */
#define BHRT_MAX_IMAGE_PIXELS 2147483647  /* 2^31 - 1 */
int bhrt_scene_set_resolution(bhrt_scene *scene, int32_t width, int32_t height);
/* The camera's <position>, <target>, <up> and <fov> of a loaded scene (xmlload.cpp:109-127), through the loader's own operations:
 * dir = normalized(target - pos), x = dir ^ up, up = normalized(x ^ dir), then the camera frame.  fov <= 0 keeps the current fov; focaldist, dof,
 * width and height are kept.  bhrt_scene_flat is afterwards byte-identical to the blob of the same XML with the four values written into its
 * <camera>, and the pointer it returned stays valid.  Needs no device; on an uploaded scene the device's copy of the camera and the camera
 * position carried through every node's chain are refreshed (nothing else is uploaded again), so the call is cheap enough for a viewport: between
 * two steps of a progressive session later samples use the new camera, as with the other setters.  BHRT_ERR_ARG, with nothing changed and before
 * any device is touched: a NULL pointer; a component that is not finite; a fov that is NaN, infinite or >= 180; target == pos; up parallel to
 * target - pos; and, while a shutter is on, a camera that is a quarter turn or more from the shutter's pose 1 (see below). */
int bhrt_scene_set_camera(bhrt_scene *scene, const float pos[3], const float target[3], const float up[3], float fov);
/* The camera shutter: camera motion blur.  Pose 0 is the scene's camera, pose 1 = (pos1, target1, up1) the camera at the end of the
 * exposure, with the scene's fov, focaldist, dof and size and a frame derived by the loader's own operations (it is derived again whenever
 * bhrt_scene_set_lens or bhrt_scene_set_camera changes what it depends on).  With the shutter on every camera sample (pixel i, j, sample s) draws
 * a time t, uniform on [0, 1): rand_to_unit of draw 0 of the stream keyed by section BHRT_SEC_SHUTTER of path code 0 under the sample's key
 * (include/bhrt_rng.h: sample key of seed, j * W + i, s), a stream of its own, and its ray is the camera ray — jitter and lens as without a shutter — of the frame
 *     X_t = X0 + (X1 - X0) * t      per component, in float32, for X = pos, top_left, dd_x, dd_y
 * with the jitter's and the lens's axes normalized(dd_x_t), normalized(dd_y_t) and pixel length |dd_x_t|.  Equal poses give the render without a
 * shutter bit for bit.  All later bhrt_render*, _samples, _var*, _adaptive*, bhrt_progressive_*, bhrt_guides* and bhrt_camera_rays of the scene
 * follow the shutter.  bhrt_first_hit* and the guides bhrt_denoise* computes itself stay those of pose 0's pinhole ray.  One stated limit: the
 * texture footprint of a plane hit reads the camera's dd_x, dd_y (Plane.cpp:51-70) and keeps reading pose 0's at every bounce, as under the lens:
 * exact under a translation; under a rotation a textured plane is filtered with pose 0's footprint.
 * The state lives beside the flat blob: bhrt_scene_flat's bytes do not change, bhrt_scene_clone carries it, bhrt_opts has no field for it.  Needs
 * no device; on an uploaded scene the device's copy is refreshed.  Default: off.
 *   on == 0   clears the state; the three pointers may be NULL
 *   on != 0   BHRT_ERR_ARG with nothing changed, before any device is touched, for a NULL pointer, a component that is not finite,
 *             target1 == pos1, up1 parallel to target1 - pos1, and for poses a quarter turn or more apart: dir0 . dir1 <= 0, dd_x0 . dd_x1 <= 0 or
 *             dd_y0 . dd_y1 <= 0 (with positive products no interpolated axis can be zero, so no ray is ever NaN)
 * get_shutter: the switch, pose 1 as given (pos1, target1, up1) and its derived frame (pos1, top_left1, dd_x1, dd_y1); any pointer may be NULL. */
int bhrt_scene_set_shutter(bhrt_scene *scene, int on, const float pos1[3], const float target1[3], const float up1[3]);
int bhrt_scene_get_shutter(const bhrt_scene *scene, int *on, float pose1[9], float frame1[12]);
/* The camera frame of the scene's camera: pos, top_left, dd_x, dd_y, in the layout of bhrt_scene_get_shutter's frame1; the blob's bhrt_camera,
 * before and after bhrt_scene_set_camera / bhrt_scene_set_lens.  Needs no device.  A host that reprojects (bhrt_reproject*) calls it before it
 * moves the camera. */
int bhrt_scene_get_camera_frame(const bhrt_scene *scene, float frame[12]);
/* Moving objects: the names and transforms of the nodes of a loaded scene.  A node is named by its index in the blob's nodes[]
 * (DFS pre-order of the XML's <object> elements, include/bhrt_flat.h), which is also what bhrt_hits::node and bhrt_first_hit_node* report.
 *   node_index           the first node whose <object name=> is `name`, in that order; an unknown name or a NULL argument: BHRT_ERR_ARG
 *   get_node_transform   the blob's record (tm, pos, itm) of that node
 *   get_node_transforms  all n_nodes records; capacity < n_nodes: BHRT_ERR_ARG.  *n (may be NULL) = n_nodes.  The snapshot a host takes before it
 *                        moves something (bhrt_reproject_moving* reads it), as bhrt_scene_get_camera_frame is for the camera
 *   set_node_transform   starts from (tm, pos) — both NULL: the identity; exactly one NULL: BHRT_ERR_ARG — applies the ops in order with the
 *                        loader's own Transformation operations (xmlload.cpp:275-303: a rotate's axis is normalised, its angle is in degrees) and
 *                        stores tm, pos and itm as the loader stores them.  Called with the node's current tm / pos and ops o_1 .. o_n,
 *                        bhrt_scene_flat is afterwards byte-identical to the blob of the same XML with <scale> / <rotate> / <translate> elements
 *                        for o_1 .. o_n appended to that <object>; called with NULL / NULL, to the blob with the node's transform children
 *                        replaced by them.  Restoring a saved record is (tm, pos, no ops).  The pointer bhrt_scene_flat returned stays valid.
 * BHRT_ERR_ARG, with nothing changed and before any device is touched: a NULL scene; a node outside [0, n_nodes); ops == NULL with n_ops > 0; an
 * unknown kind; a component that is not finite; a rotate axis of length 0; a result whose tm, pos or itm holds a value that is not finite (a
 * singular matrix).  ("Nothing changed" covers BHRT_ERR_ARG: after a BHRT_ERR_HIP from an uploaded scene's refresh the host blob holds the new
 * record and the device may not.)  None of the calls needs a device.  The refresh writes into the device's live blob with blocking copies, as
 * the other setters do: the host calls it when the scene's renders and image calls on its own streams have finished.  On an uploaded scene the node's 84 bytes in the device's blob and the camera position
 * carried through every node's chain are refreshed, and nothing else is uploaded again: between two steps of a progressive session later
 * samples see the new transform, as with the other setters.  Stated limits: an installed caustic or global photon map is the old scene's (the
 * host builds it again); the shutter does not interpolate nodes, so there is no object motion blur; lights are moved by
 * bhrt_scene_set_light, not by this call.  bhrt_scene_clone
 * carries the names and the edits. */
enum { BHRT_XFORM_SCALE = 0, BHRT_XFORM_ROTATE = 1, BHRT_XFORM_TRANSLATE = 2 };
typedef struct bhrt_xform_op {
    int32_t kind; /* BHRT_XFORM_* */
    float v[4];   /* scale: x, y, z; rotate: axis x, y, z and the angle in degrees; translate: x, y, z */
} bhrt_xform_op;
struct bhrt_xform; /* include/bhrt_flat.h: tm[9], pos[3], itm[9], 84 bytes */
int bhrt_scene_node_index(const bhrt_scene *scene, const char *name, int32_t *index);
int bhrt_scene_get_node_transform(const bhrt_scene *scene, int32_t node, struct bhrt_xform *out);
int bhrt_scene_get_node_transforms(const bhrt_scene *scene, struct bhrt_xform *out, uint32_t capacity, uint32_t *n);
int bhrt_scene_set_node_transform(bhrt_scene *scene, int32_t node, const float tm[9], const float pos[3], const bhrt_xform_op *ops, uint32_t n_ops);
/* Lights: the <light> elements of a loaded scene, found, read and set without a reload.  A light is named by its index in document
 * order: the order of the XML's accepted <light> elements (type ambient, direct or point; xmlload.cpp:394-474).  The blob's lights[] is that list
 * sorted ascending by Gray() (CalculateLightsIntensity, Main.cpp:116-123), so an intensity edit can permute the blob; the index does not change.
 *   light_count   the number of lights (bhrt_info.n_lights)
 *   light_index   the first light whose <light name=> is `name`, in document order; an unknown name or a NULL argument: BHRT_ERR_ARG
 *   get_light     the light as the loader read it (a direct light's vec normalised) and blob_index, where it stands in the blob's lights[] now
 *   set_light     intensity == NULL keeps the intensity, vec == NULL the position (point) or direction (direct), size < 0 the size.  A direct
 *                 light's vec goes through the loader's own normalized(); kind and count never change; a light is switched off by a zero
 *                 intensity.  The loader's own sort and float sum then run again on the document-order list and the blob's lights[] and
 *                 all_light_intensity are rewritten in place: bhrt_scene_flat is afterwards byte-identical, ties in Gray() included, to the blob
 *                 of the same XML with <intensity r g b> (no value=), <position x y z> / <direction x y z> (the caller's un-normalised vector) and
 *                 <size value> written into that <light>.  The pointer bhrt_scene_flat returned stays valid and total_bytes is unchanged.
 * BHRT_ERR_ARG, with nothing changed and before any device is touched: a NULL scene; an index outside [0, n); a component that is not finite; a
 * negative intensity component; a vec for an ambient light; a size >= 0 for a light that is not a point light; a direct vec of length 0, or one
 * whose normalisation is not finite; a size that is NaN or +inf; an edit after which all_light_intensity is not finite and > 0 (the light-pick
 * table divides by it: a stated limit, although the loader itself takes such a file).  None of the calls needs a device.  On an uploaded scene
 * the lights block of the device's blob, the n_lights entries of the light-pick table and the kernels' copy of all_light_intensity are
 * refreshed, and nothing else is uploaded again, with blocking copies, as the other setters do: the host calls it when the scene's renders and
 * image calls on its own streams have finished.  Between two steps of a progressive session or two frames of a temporal session later samples
 * see the new light, as with the other setters.  Stated limits: an installed caustic or global photon map is the old light's (the host builds it
 * again); the shutter does not interpolate lights, so there is no light motion blur; a temporal session notices the change only through the
 * change test, which is off unless bhrt_temporal_set_change switched it on.  bhrt_scene_clone carries the names and the edits. */
typedef struct bhrt_light_info {
    int32_t type;        /* BHRT_LIGHT_* of include/bhrt_flat.h */
    float intensity[3];
    float vec[3];        /* point: position; direct: the normalised direction; ambient: 0 */
    float size;          /* point: the radius; else 0 */
    int32_t blob_index;  /* where the light stands in the blob's lights[] now */
    int32_t reserved[5]; /* 0 */
} bhrt_light_info; /* 56 B */
int bhrt_scene_light_count(const bhrt_scene *scene, int32_t *n);
int bhrt_scene_light_index(const bhrt_scene *scene, const char *name, int32_t *index);
int bhrt_scene_get_light(const bhrt_scene *scene, int32_t light, bhrt_light_info *out);
int bhrt_scene_set_light(bhrt_scene *scene, int32_t light, const float intensity[3], const float vec[3], float size);
/* The emission term.  Every Blinn material carries the <emission> of its XML (xmlload.cpp:344-348: a colour, optionally a texture
 * map); the reference parses it and never shades it, and so does a scene here until it is switched on.  With the term on, every Shade() frame of
 * a Blinn material evaluates to  Shade(hit) + emission.Sample(uvw, duvw)  — one float addition per channel, behind everything Shade() does, on
 * front and back hits, at every bounce (a GI or refraction ray that lands on an emitter brings its light back).  Frames of a node without
 * material or with an empty MultiMtl get nothing.  The state lives beside the flat blob: bhrt_scene_flat's bytes do not change, bhrt_scene_clone
 * carries it, and bhrt_opts has no field for it.  None of these calls needs a device; on an uploaded scene they refresh the device's copy.
 *   set_emissive           on != 0: the term is part of all later renders of this scene (bhrt_render*, _samples, _var*, _adaptive*); default 0
 *   material_index         the index of the XML material of that name (the first, as the loader resolves node materials); unknown: BHRT_ERR_ARG
 *   set_material_emission  a plain colour for that material, any map dropped; index out of range: BHRT_ERR_ARG
 *   get_material_emission  the colour and the index into the blob's texmaps[] (-1 = plain colour); rgb / texmap may be NULL */
int bhrt_scene_set_emissive(bhrt_scene *scene, int on);
int bhrt_scene_material_index(const bhrt_scene *scene, const char *name, int32_t *index);
int bhrt_scene_set_material_emission(bhrt_scene *scene, int32_t material, const float rgb[3]);
int bhrt_scene_get_material_emission(const bhrt_scene *scene, int32_t material, float rgb[3], int32_t *texmap);
/* Face materials.  An OBJ's .mtl becomes a MultiMtl with one Blinn sub-material per `newmtl` (xmlload.cpp:219-250) and the mesh
 * keeps its faces grouped by them (cyTriMesh.h:461-487), but the reference's triangle hits never set the material id, so a render shades the whole
 * mesh with sub-material 0 — and so does a scene here until it is switched on.  With the switch on, every Shade() frame opened on a hit of a node
 * whose material is a MultiMtl uses the sub-material of the face that was hit: the first i with face < face_end[i]
 * (TriMesh::GetMaterialIndex), and sub-material 0 where there is none (faces in front of any usemtl, a hit that is no triangle, a face id beyond
 * the material's own mesh).  Everything behind the choice follows it at every bounce: Fresnel, the refraction chain and its absorption, the GI
 * lobe, the caustic gather, textures; bhrt_first_hit's albedo too.  Photon emission does not (MultiMtl has no photon bounce).  The state lives
 * beside the flat blob: bhrt_scene_flat's bytes do not change, bhrt_info.n_materials and the material indices stay the blob's, bhrt_scene_clone
 * carries it, and bhrt_opts has no field for it.  None of these calls needs a device; on an uploaded scene the setter refreshes the device's copy.
 * Materials plus sub-materials beyond 4095 with the switch on: the renders return BHRT_ERR_UNSUPPORTED.
 *   set_face_materials   on != 0: all later bhrt_render*, _samples, _var*, _adaptive*, bhrt_first_hit* and the denoiser's guides; default 0
 *   submaterial_count    the number of sub-materials of that material, 0 for one that is not a MultiMtl (or an empty one); index out of range:
 *                        BHRT_ERR_ARG
 *   get_submaterial      sub-material `sub` as the blob's materials are laid out (bhrt_flat.h; sub-material 0 is the blob's own record, byte for
 *                        byte) and the end of its face range; out / face_end may be NULL; material or sub out of range: BHRT_ERR_ARG */
struct bhrt_material;
int bhrt_scene_set_face_materials(bhrt_scene *scene, int on);
/* The global gather: indirect light from the global photon map where the GI recursion ends.  PathTracing_GlobalIllumination returns
 * black when its bounce budget is spent (i_GIbounceCount < 0, MtlBlinn.cpp:386); with the switch on and a global map installed it returns there
 *     (E, vL) = EstimateIrradiance<1000>(radius, hInfo.p, &hInfo.N) on the global map          (cyPhotonMap.h:332-382)
 *     G       = -vL . vN > 0 ? clamp(Color::Black() + diffuse.Sample(uvw, duvw) * E) : black;   black where G.r is NaN or no photon is found
 * and Shade() goes on as it does behind any GI term: outColor += G, the early return at white, the direct and caustic terms, the clamp, the NaN
 * replacement, Le.  Frames that open a GI child (gi >= 0) are unchanged, so gi_bounces = 0 adds multi-bounce indirect light behind one GI ray per
 * sample, and gi_bounces = -1 shows the map at the first hit.  Frames of a node without material or with an empty MultiMtl get nothing; with face
 * materials on, diffuse is the hit face's sub-material.  The caustic map (bhrt_opts.photon_map) is independent; bhrt_opts.photon_exact selects the
 * heavy-query path of both gathers.  The switch and radius live beside the flat blob: bhrt_scene_flat's bytes do not change, bhrt_scene_clone
 * carries them (not the map, which is device state), and bhrt_opts has no field for them.  Needs no device.
 *   on != 0: all later bhrt_render*, _samples, _var*, _adaptive* of this scene; they return BHRT_ERR_ARG, before any kernel is launched, while no
 *   global map is installed.  radius: 0 = the reference's MAX_Area, 0.5 (MtlBlinn.cpp:29); negative or not finite: BHRT_ERR_ARG.  Default: off */
int bhrt_scene_set_global_gather(bhrt_scene *scene, int on, float radius);
int bhrt_scene_submaterial_count(const bhrt_scene *scene, int32_t material, int32_t *n);
int bhrt_scene_get_submaterial(const bhrt_scene *scene, int32_t material, int32_t sub, struct bhrt_material *out, uint32_t *face_end);

/* ---- device residency ---------------------------------------------------------------------------- */
int bhrt_scene_upload(bhrt_scene *scene, int device); /* copies the flat scene into HBM of `device`; idempotent.  To another device: the device state of the
                                                        * old one is dropped; BHRT_ERR_ARG while a progressive session holds state there */
/* knobs of an uploaded scene: they steer which internal path a render takes, never its result.  Test knobs "frame_cap", "gather_lane_budget" (0 = off) and
 * "gather_stats"; "shadow_overlap" (default 1; 0 = the any-hit kernels of a wave step run in front of the next step on the pass's own stream instead of
 * beside it on a second one: the kernel groups timed alone, bench.py's `frac_alone`); "fused_resolve" (default 1; 0 = a render that asks for the image
 * alone ends in the root level of k_combine and k_resolve, through the per-sample buffer, like every other render, instead of k_resolve_frames);
 * "finish_misses" (default 1; 0 = the closest-hit kernel files the rays that left the scene for the shading kernel, like every other ray, instead of
 * storing their value itself).
 * The library reads its development switches (BHRT_STREAM_WAVES, BHRT_FUSED_CAMERA, BHRT_NO_SLOW_QUEUE, BHRT_DEBUG_*, BHRT_PHOTON_BALANCE_HOST,
 * BHRT_GATHER_COUNTING_SORT, BHRT_SHADOW_OVERLAP, BHRT_FUSED_RESOLVE, BHRT_FINISH_MISSES) from the environment once, at upload; the test knobs are not reachable from the environment at
 * all.  tests/test_switch_paths.py holds every switch to "never its result" (DESIGN.md 5). */
int bhrt_scene_knob(bhrt_scene *scene, const char *name, int value);
int bhrt_device_count(int *n);

/* ---- the hot path --------------------------------------------------------------------------------- */
/* recursive(&rootNode, ray, hit, bHit, hitSide) for n rays (Main.cpp:389-413).
 * rays_soa: 6 arrays of n floats back to back (ox[n], oy[n], oz[n], dx[n], dy[n], dz[n]).
 * *_host variants take host pointers (copies included); *_dev take device pointers + a hipStream_t. */
int bhrt_trace_closest_host(bhrt_scene *scene, const float *rays_soa, int hit_side, size_t n, bhrt_hits out);
int bhrt_trace_closest_dev(bhrt_scene *scene, const float *d_rays_soa, int hit_side, size_t n, bhrt_hits d_out, void *stream);
/* GenLight::Shadow(ray, t_max) (Lights/GenLight.cpp:10-13): vis = 0 occluded / 1 visible */
int bhrt_trace_shadow_host(bhrt_scene *scene, const float *rays_soa, const float *tmax, size_t n, float *vis);
int bhrt_trace_shadow_dev(bhrt_scene *scene, const float *d_rays_soa, const float *d_tmax, size_t n, float *d_vis, void *stream);

/* BeginRender() (Main.cpp:178-242) without the UI and without the PNG write: renders this rank's tiles.
 * rgb8: W*H*3 bytes, row-major j*W+i like RenderImage::GetPixels (may be NULL);
 * radiance: W*H*3 floats, the per-pixel average BEFORE gamma (may be NULL).
 * Pixels of tiles owned by other ranks are left untouched.  Host pointers. */
int bhrt_render(bhrt_scene *scene, const bhrt_opts *opts, uint8_t *rgb8, float *radiance, bhrt_stats *stats);
/* Pinned (page-locked) host memory for the frame buffers handed to bhrt_render: the device-to-host copy then runs at the full PCIe
 * rate (a pageable destination: about half).  Any host pointer works; this is only faster. */
int bhrt_host_alloc(void **ptr, size_t bytes);
void bhrt_host_free(void *ptr);
/* same, but the outputs stay in HBM (device pointers; for timing and for the RCCL gather) */
int bhrt_render_dev(bhrt_scene *scene, const bhrt_opts *opts, uint8_t *d_rgb8, float *d_radiance, bhrt_stats *stats, void *stream);
/* per-sample radiance for a pixel region, keyed RNG (parity tests): out = region_pixels*spp*3 floats, host */
int bhrt_render_samples(bhrt_scene *scene, const bhrt_opts *opts, int x0, int y0, int x1, int y1, float *samples, bhrt_stats *stats);

/* test hook: the camera rays of a pixel region as the render's first wave step forms them (bhrt_opts.lens 0: the device function the camera
 * kernels inline; 1: the lens kernel's body), on the device.  rays: region_pixels * spp * 6 floats (ox, oy, oz, dx, dy, dz per sample), host,
 * in the order of bhrt_render_samples.  Uses spp, seed, jitter and lens of the options, and the scene's shutter (the shutter kernels' body). */
int bhrt_camera_rays(bhrt_scene *scene, const bhrt_opts *opts, int x0, int y0, int x1, int y1, float *rays);

/* ---- caustic photon map (Main.cpp:342-386, DataStructure/cyPhotonMap.h) -------------------------- */
int bhrt_photon_build(bhrt_scene *scene, const bhrt_opts *opts, uint32_t max_photons, uint32_t *n_stored);
/* Multi-GPU build of the caustic map: the emission loop of BuildCausticPhotonMap (Main.cpp:342-386) draws from
 * a stream keyed by the emission index, so ranks can run disjoint index ranges.  bhrt_photon_emit_range runs emissions
 * [e0, e0 + count) (count a multiple of 256) and returns the photons they store, in emission order, with unscaled power
 * (24-byte records; photons_out may be a host or a device pointer — the records of a multi-GPU build never need to touch the host;
 * *n_photons = how many, also when that is more than capacity: BHRT_ERR_ARG then, call again with room for them).  bhrt_photon_install takes records in
 * emission order (after the exchange: the first MAX_CausticPhotonCount of all ranks' records), applies ScalePhotonPowers(1/n)
 * (Main.cpp:380), balances and installs the map for bhrt_render* — the same map bhrt_photon_build makes alone. */
int bhrt_photon_emit_range(bhrt_scene *scene, const bhrt_opts *opts, int global_map, uint64_t e0, uint32_t count, void *photons_out, uint32_t capacity,
                           uint32_t *n_photons);
int bhrt_photon_install(bhrt_scene *scene, const void *records_emission_order /* host or device pointer */, uint32_t n);
/* The reference's second map, BuildPhotonMap (Main.cpp:251-295; TracePhotonRay Main.cpp:296-317, RandomPhotonBounce
 * MtlBlinn.cpp:140-202): photons that survive diffuse and specular bounces, stored from the second hit on (indirect light only).
 * Its only call is commented out in the reference (Main.cpp:196) and the reference never gathers from it.  This call builds it
 * on request and hands it back, installing nothing: balanced 24-byte records into photons_out (capacity records; may be NULL)
 * and / or written like Resource/photonmap.dat (dat_path, may be NULL).  The global gather (bhrt_scene_set_global_gather) reads
 * the map that bhrt_global_map_build / _set install. */
int bhrt_photon_build_global(bhrt_scene *scene, const bhrt_opts *opts, uint32_t max_photons, void *photons_out, uint32_t capacity, uint32_t *n_stored,
                             const char *dat_path);
/* The global map's own device slot; the caustic map of bhrt_photon_build / _install / _import is not touched by any of these.
 *   build        BuildPhotonMap as bhrt_photon_build_global runs it (same records), balanced and left installed; *n_stored may be NULL
 *   set          installs n balanced 24-byte records as they are (what bhrt_photon_build_global or bhrt_global_map_get returned); host or device
 *                pointer; n = 0 removes the map
 *   get          mirrors bhrt_photon_get
 *   gather_host  bhrt_photon_gather_host_ex on this slot: the estimate alone (test hook) */
int bhrt_global_map_build(bhrt_scene *scene, const bhrt_opts *opts, uint32_t max_photons, uint32_t *n_stored);
int bhrt_global_map_set(bhrt_scene *scene, const void *balanced_records, uint32_t n);
int bhrt_global_map_get(const bhrt_scene *scene, void *photons_out /* 24 B records, balanced order */, uint32_t capacity, uint32_t *n);
int bhrt_global_gather_host(bhrt_scene *scene, const float *p, const float *n, size_t cnt, float radius, int photon_exact, float *irrad, float *dir);
int bhrt_photon_gather_host(bhrt_scene *scene, const float *p, const float *n, size_t cnt, float radius, float *irrad, float *dir);
/* same with the choice of bhrt_opts.photon_exact, and (test hook, any pointer may be NULL) the photons the estimate used: knn = cnt x 1000
 * indices into the balanced map (1-based, unsorted, unused slots 0), knn_count = how many, d2max = np.dist2[0] at the end of LocatePhotons.
 * Filled for the queries the selection pass answers (>= 1000 photons in the radius, photon_exact = 0); knn_count = 0 otherwise. */
int bhrt_photon_gather_host_ex(bhrt_scene *scene, const float *p, const float *n, size_t cnt, float radius, int photon_exact, float *irrad, float *dir,
                               uint32_t *knn, uint32_t *knn_count, float *d2max);
int bhrt_photon_get(const bhrt_scene *scene, void *photons_out /* 24 B records, balanced order */, uint32_t capacity, uint32_t *n);
int bhrt_photon_export(const bhrt_scene *scene, const char *dat_path); /* 24-byte records, Main.cpp:383-385 */
/* Loads a map written by bhrt_photon_export or by the reference (Resource/causticPhotonMap.dat) instead of building it.
 * rebalance = 1: PhotonMap::InitializePhotonMapByFile (cyPhotonMap.h:409-417), which balances the records again;
 * rebalance = 0: the records are used in the order of the file (a balanced map as exported: the cached photon pass). */
int bhrt_photon_import(bhrt_scene *scene, const char *dat_path, int rebalance);

/* ---- multi-GPU framebuffer exchange (no counterpart in the single-process reference) ------------------
 * Tile t (row-major over ceil(W/tile) x ceil(H/tile) tiles) belongs to rank t mod world, the same rule bhrt_render*
 * applies through bhrt_opts.rank / world_size / tile_size.  A rank packs the tiles it rendered into ONE block
 * (float radiance section, then RGB8 section); one all-gather of the blocks (RCCL) and one unpack give every rank
 * the whole image.  Device pointers; `stream` is a hipStream_t (NULL = the default stream), the calls do not synchronise. */
size_t bhrt_tiles_block_bytes(int width, int height, int tile, int world); /* bytes of one rank's block */
int bhrt_tiles_pack_dev(const uint8_t *d_rgb8, const float *d_radiance, int width, int height, int tile, int rank, int world, void *d_block, void *stream);
int bhrt_tiles_unpack_dev(const void *d_blocks /* world blocks, rank-major */, int width, int height, int tile, int world, uint8_t *d_rgb8, float *d_radiance,
                          void *stream);

/* ---- images beside the colour image ------------------------------------------
 * First hit of the un-jittered camera ray of every pixel (the pixel corner: `1 / 2 == 0`, Main.cpp:145), row-major:
 *   z       W*H floats      HitInfo::z, BIGFLOAT where nothing is hit = RenderImage::GetZBuffer() (scene.h:532; its store is
 *                           commented out at Main.cpp:231)
 *   normal  W*H*3 floats    HitInfo::N in world space (zero on a miss)   \ the optional "normal" / "albedo" images of
 *   albedo  W*H*3 floats    diffuse.Sample(uvw, duvw) of the hit material / DenoiseImage (Main.cpp:70-71, commented out there)
 * Any pointer may be NULL. */
int bhrt_first_hit_dev(bhrt_scene *scene, float *d_z, float *d_normal, float *d_albedo, void *stream);
int bhrt_first_hit(bhrt_scene *scene, float *z, float *normal, float *albedo);
/* The node-id image: W*H int32, row-major, the index into the blob's nodes[] of the first hit of the same un-jittered camera
 * ray, -1 where nothing is hit: bhrt_hits::node of bhrt_trace_closest* for that ray with BHRT_SIDE_FRONT.  It tells a host which object a
 * pixel shows.  A kernel of its own beside bhrt_first_hit*'s, whose three images and code are unchanged.  _dev: a device pointer; with a
 * stream the call does not synchronise.  A NULL image: BHRT_ERR_ARG. */
int bhrt_first_hit_node_dev(bhrt_scene *scene, int32_t *d_node, void *stream);
int bhrt_first_hit_node(bhrt_scene *scene, int32_t *node);
/* All four images from ONE trace per pixel: z, normal and albedo are bhrt_first_hit*'s bytes and node is bhrt_first_hit_node*'s,
 * face materials included.  A third kernel beside the two, whose code is unchanged.  Any pointer may be NULL; all four NULL: BHRT_ERR_ARG,
 * before any device is touched.  _dev: device pointers; with a stream the call does not synchronise. */
int bhrt_first_hit_ex_dev(bhrt_scene *scene, float *d_z, float *d_normal, float *d_albedo, int32_t *d_node, void *stream);
int bhrt_first_hit_ex(bhrt_scene *scene, float *z, float *normal, float *albedo, int32_t *node);
/* Sampled guide images: the same three images, and the coverage, formed by the render's own camera samples, so that they are
 * averaged over the pixel footprint the colour image is averaged over: jitter and, with bhrt_opts.lens, the aperture.  For an owned pixel inside
 * the image and n = spp, sample s = 0 .. n-1 has the camera ray the render forms for (seed, pixel, s) (what bhrt_camera_rays returns), its first
 * hit with BHRT_SIDE_FRONT, and on a hit the values of the first-hit images for that ray: t_s, N_s (HitInfo::N, world space) and kd_s (a Blinn material:
 * diffuse.Sample(uvw, duvw); white: (1, 1, 1); else 0).  With k the number of samples that hit and every sum taken over those samples alone, in
 * float32, in ascending sample order, starting from the first one's value:
 *   coverage  W*H floats    (float)k / (float)n
 *   z         W*H floats    k ? (sum t_s) / (float)k : BIGFLOAT
 *   normal    W*H*3 floats  (sum N_s) / (float)n        not renormalised: a pixel on an edge, or one that partly misses, carries a shorter normal
 *   albedo    W*H*3 floats  (sum kd_s) / (float)n
 * With spp = 1, jitter = 0 and lens = 0 (or dof = 0) z, normal and albedo are the first-hit images bit for bit.  Row-major; any pointer may be NULL.
 * Uses spp (1 .. 65535), seed, jitter, lens, rank, world_size, tile_size and samples_per_pass (the most samples in flight; 0 = no bound) of the
 * options; the result depends on neither the pass size nor the partition, and pixels of other ranks' tiles are left untouched.  Bad options
 * (spp, lens, lens = 1 with a bad dof, rank outside world_size): BHRT_ERR_ARG, before any device is touched.  The face-material switch of the
 * scene applies to the albedo as it does to the first-hit images.  _dev: device pointers; with a stream the call does not synchronise.  The running
 * sums of a call whose spp exceeds one workgroup's 256 samples (or samples_per_pass) are scratch of the scene, 32 B per pixel of a pass: calls on
 * one scene must not overlap. */
int bhrt_guides_dev(bhrt_scene *scene, const bhrt_opts *opts, float *d_z, float *d_normal, float *d_albedo, float *d_coverage, void *stream);
int bhrt_guides(bhrt_scene *scene, const bhrt_opts *opts, float *z, float *normal, float *albedo, float *coverage);
/* RenderImage::ComputeZBufferImage (scene.h:578-600): 8-bit depth image, 0 where nothing is hit.  Device pointers. */
int bhrt_zbuffer_image_dev(bhrt_scene *scene, const float *d_z, size_t n, uint8_t *d_img, void *stream);
/* colorArray of BeginRender (Main.cpp:202,219-229): pow(colour, 1/2.2f) as floats — the "color" image DenoiseImage is given
 * (Main.cpp:60-69).  d_radiance = the radiance image of bhrt_render_dev. */
int bhrt_color_image_dev(bhrt_scene *scene, const float *d_radiance, size_t n_pixels, int gamma, float *d_color, void *stream);

/* ---- denoiser: the DenoiseImage step of the reference's 64-bit build (Main.cpp:57-96, applied at Main.cpp:236-238) --------------
 * An edge-avoiding a-trous wavelet filter guided by the first hit (z, normal, albedo) and, when given, the per-pixel variance of the
 * render; the filter is stated exactly in csrc/denoise.hip.  Not OIDN (a neural network): the same step, not its bits. */
typedef struct bhrt_denoise_opts {
    int32_t iterations;    /* K: a-trous levels, step 2^k for k < K (0 = the identity: out = radiance, rgb8 = the render's bytes); default 4 */
    float sigma_normal;    /* exponent of the normal weight, default 32 */
    float sigma_depth;     /* relative depth tolerance per pixel of distance, default 0.01 */
    float sigma_luminance; /* luminance tolerance in standard deviations of the noise (used with a variance image), default 4 */
    int32_t gamma;         /* rgb8: 1 = pow(c, 1/2.2f) before Color24, as bhrt_opts.gamma; default 1 */
    int32_t reserved[3];
} bhrt_denoise_opts;
void bhrt_default_denoise_opts(bhrt_denoise_opts *opts);
/* bhrt_render_dev / bhrt_render plus the denoiser's noise estimate: variance = W*H*3 floats, the per-channel variance of each pixel's
 * mean, sum_s (x_s - m)^2 / (spp - 1) / spp (0 at spp = 1), laid out like radiance (pixels of other ranks' tiles untouched, so it travels
 * through bhrt_tiles_pack_dev / _unpack_dev as the radiance section of a second block).  variance = NULL: exactly bhrt_render_dev / bhrt_render. */
int bhrt_render_var_dev(bhrt_scene *scene, const bhrt_opts *opts, uint8_t *d_rgb8, float *d_radiance, float *d_variance, bhrt_stats *stats, void *stream);
int bhrt_render_var(bhrt_scene *scene, const bhrt_opts *opts, uint8_t *rgb8, float *radiance, float *variance, bhrt_stats *stats);
/* DenoiseImage(colorArray, renderImage) (Main.cpp:236-238) on the whole W x H frame of the scene's camera.
 * radiance: W*H*3 linear floats (bhrt_render*'s radiance, before gamma).  variance: bhrt_render_var*'s, or NULL (no luminance weight).
 * z (W*H), normal, albedo (W*H*3 each): the first-hit images of bhrt_first_hit*; each may be NULL = computed here by the same kernel.
 * out: W*H*3 linear floats, rgb8: W*H*3 bytes (gamma + Color24 as in bhrt_render); either may be NULL.
 * _dev: device pointers; with a stream the call does not synchronise.  Scratch (48 B per pixel, + 28 B when guides are computed) belongs
 * to the scene: calls on one scene must not overlap, a call on another stream included. */
int bhrt_denoise_dev(bhrt_scene *scene, const bhrt_denoise_opts *opts, const float *d_radiance, const float *d_variance, const float *d_z, const float *d_normal,
                     const float *d_albedo, float *d_out, uint8_t *d_rgb8, void *stream);
int bhrt_denoise(bhrt_scene *scene, const bhrt_denoise_opts *opts, const float *radiance, const float *variance, const float *z, const float *normal,
                 const float *albedo, float *out, uint8_t *rgb8);
/* The denoiser for sampled guides: the same filter with a demodulation, a normal weight and a further weight that read the
 * coverage image, stated exactly in csrc/denoise.hip beside the other.  z, normal, albedo and coverage are the four images of one
 * bhrt_guides* call with the render's seed, jitter and lens: a partly covered pixel is divided by albedo + (1 - coverage), the share of the
 * background included, its shortened normal is compared by direction, and pixels of unlike coverage mix less
 * (exp(-|coverage difference| / sigma_coverage)).  Fed one un-jittered pinhole sample's guides it is bhrt_denoise* to rounding.
 * radiance, variance (may be NULL), out, rgb8 and the options: as for bhrt_denoise*.  sigma_coverage: finite and >= 0, else BHRT_ERR_ARG;
 * BHRT_DENOISE_SIGMA_COVERAGE is the measured default.  With iterations > 0 all four guide images are required (a NULL one: BHRT_ERR_ARG);
 * iterations = 0 reads none.  _dev: device pointers; with a stream the call does not synchronise.  Scratch (48 B per pixel; the coverage is read
 * in place) is the scene's, shared with bhrt_denoise*: calls on one scene must not overlap, a call on another stream included. */
#define BHRT_DENOISE_SIGMA_COVERAGE 0.5f
int bhrt_denoise_sampled_dev(bhrt_scene *scene, const bhrt_denoise_opts *opts, float sigma_coverage, const float *d_radiance, const float *d_variance, const float *d_z,
                             const float *d_normal, const float *d_albedo, const float *d_coverage, float *d_out, uint8_t *d_rgb8, void *stream);
int bhrt_denoise_sampled(bhrt_scene *scene, const bhrt_denoise_opts *opts, float sigma_coverage, const float *radiance, const float *variance, const float *z,
                         const float *normal, const float *albedo, const float *coverage, float *out, uint8_t *rgb8);

/* ---- temporal reprojection: carry a frame's light across a camera move ---------------------------------------------
 * When the camera moves between two frames, bhrt_reproject* finds for every pixel of the new view where its surface point was in the previous
 * view and fetches the light gathered there if it is still the same surface; bhrt_temporal_accumulate* blends the new frame's samples into it.
 * Both stages are stated exactly in csrc/temporal.hip (float32, a fixed order: the same inputs give the same bytes).  They run beside the
 * render path and change no render.  Moving objects: bhrt_reproject_moving* below.  Not covered: lens and shutter (the guides stay the pinhole ray's, as
 * for bhrt_denoise*); reflections and refractions are reprojected as if they were surface light; a progressive session's state is not seeded.
 *
 * bhrt_reproject*: the current view is the scene's camera, W x H.  prev_frame: the previous view's bhrt_scene_get_camera_frame, a HOST pointer
 * in both variants.  prev_z (W*H), prev_normal (W*H*3): the previous view's first hit (bhrt_first_hit*), required.  prev_radiance (W*H*3):
 * the light to carry (a render's radiance or an accumulated frame), required when history is asked for.  prev_length (W*H floats): the
 * samples behind each previous pixel; NULL = 1 everywhere.  prev_albedo (W*H*3, optional): with it the history is carried as irradiance,
 * prev_radiance / divisor(prev_albedo) * divisor(albedo); without it no albedo is read or computed.  z, normal, albedo: the current view's
 * first hit; each may be NULL = computed here by the same kernel.  Outputs, each may be NULL: history (W*H*3), length (W*H; 0 = the pixel has
 * no history), motion (W*H*2: where the pixel was, in pixels, minus where it is).
 * BHRT_ERR_ARG before any device is touched: a NULL scene, options, prev_frame, prev_z or prev_normal; a prev_frame component that is not
 * finite; a depth_tolerance that is negative or not finite; a NaN normal_threshold; a prev_frame whose image plane holds its eye
 * (dot(top_left - pos, dd_x ^ dd_y) == 0); prev_albedo without prev_radiance; history without prev_radiance.
 * _dev: device pointers; with a stream the call does not synchronise.  Scratch for guides computed here (28 B per pixel) is the scene's,
 * shared with bhrt_denoise*: calls on one scene must not overlap, a call on another stream included. */
#define BHRT_REPROJECT_DEPTH_TOLERANCE 0.01f
#define BHRT_REPROJECT_NORMAL_THRESHOLD 0.99f
#define BHRT_TEMPORAL_CLAMP_K 1.0f
#define BHRT_TEMPORAL_MAX_LENGTH 16.0f
typedef struct bhrt_reproject_opts {
    float depth_tolerance;  /* a tap is the same surface when |z' - t| <= depth_tolerance * t; default BHRT_REPROJECT_DEPTH_TOLERANCE */
    float normal_threshold; /* ... and dot(unit(n), unit(n')) >= normal_threshold; default BHRT_REPROJECT_NORMAL_THRESHOLD */
    int32_t reserved[6];
} bhrt_reproject_opts;
void bhrt_default_reproject_opts(bhrt_reproject_opts *opts);
int bhrt_reproject_dev(bhrt_scene *scene, const bhrt_reproject_opts *opts, const float prev_frame[12], const float *d_prev_z, const float *d_prev_normal,
                       const float *d_prev_radiance, const float *d_prev_length, const float *d_prev_albedo, const float *d_z, const float *d_normal,
                       const float *d_albedo, float *d_history, float *d_length, float *d_motion, void *stream);
int bhrt_reproject(bhrt_scene *scene, const bhrt_reproject_opts *opts, const float prev_frame[12], const float *prev_z, const float *prev_normal,
                   const float *prev_radiance, const float *prev_length, const float *prev_albedo, const float *z, const float *normal, const float *albedo,
                   float *history, float *length, float *motion);
/* Reprojection through object motion (stated exactly in csrc/temporal.hip beside stage 1).  bhrt_reproject* with three more
 * arguments: prev_xforms, the bhrt_scene_get_node_transforms snapshot of the previous frame (n_nodes records, a HOST pointer in both variants);
 * prev_id (W*H int32, optional), the previous view's bhrt_first_hit_node*; id (W*H int32), the current view's, NULL = computed here.  A hit
 * pixel whose node, or an ancestor of it, has other bhrt_xform bytes in prev_xforms than in the scene is carried to where its surface point was
 * before the move — through the node's chain with the current records, back out with the previous ones — and its normal takes the same path;
 * with prev_id a tap is valid only if the previous view showed the same node there.  A hit pixel whose id is outside [0, n_nodes) is invalid
 * (the kernel does not index with it).  With nothing moved every output is bhrt_reproject*'s bit for bit.  motion contains the object's motion.
 * BHRT_ERR_ARG before any device is touched: everything bhrt_reproject* refuses, a NULL prev_xforms, a prev_xforms value that is not finite.
 * Scratch is the scene's, as for bhrt_reproject*: 28 B per pixel for guides computed here, 4 B per pixel for an id computed here; calls on one
 * scene must not overlap.  The previous records (88 B per node) reach the device on the call's own stream from pinned memory of the scene, two
 * buffers used in turn: calls issued one after the other on one stream are ordered by it and each keeps its own records, and with a stream
 * the call does not wait for the device, except that the third call in a row waits until the stream has passed the first. */
int bhrt_reproject_moving_dev(bhrt_scene *scene, const bhrt_reproject_opts *opts, const float prev_frame[12], const struct bhrt_xform *prev_xforms,
                              const float *d_prev_z, const float *d_prev_normal, const float *d_prev_radiance, const float *d_prev_length, const float *d_prev_albedo,
                              const int32_t *d_prev_id, const float *d_z, const float *d_normal, const float *d_albedo, const int32_t *d_id, float *d_history,
                              float *d_length, float *d_motion, void *stream);
int bhrt_reproject_moving(bhrt_scene *scene, const bhrt_reproject_opts *opts, const float prev_frame[12], const struct bhrt_xform *prev_xforms, const float *prev_z,
                          const float *prev_normal, const float *prev_radiance, const float *prev_length, const float *prev_albedo, const int32_t *prev_id,
                          const float *z, const float *normal, const float *albedo, const int32_t *id, float *history, float *length, float *motion);
/* bhrt_temporal_accumulate*: radiance (W*H*3, required): the current frame; cur_samples: the samples behind it (> 0); history, length:
 * bhrt_reproject*'s (either NULL: no pixel has a history, out = radiance).  A pixel with length > 0 blends: out = h + (c - h) * a with
 * a = cur_samples / (l + cur_samples), l = min(length, max_length), after h has been clamped to mean +- clamp_k standard deviations of the
 * current frame's 3 x 3 block (clamp_k < 0: no clamp).  Outputs, each may be NULL: out (W*H*3), out_length (W*H: min(l + cur_samples,
 * max_length), the length to hand to the next bhrt_reproject*), rgb8 (gamma + Color24 of out, as in bhrt_render).
 * BHRT_ERR_ARG before any device is touched: a NULL scene, options or radiance; cur_samples or max_length that is not > 0 (a NaN included;
 * max_length = +inf is allowed).  _dev: device pointers; with a stream the call does not synchronise.  No scratch. */
typedef struct bhrt_temporal_opts {
    float clamp_k;    /* the history is clamped to mean +- clamp_k sigma of the 3 x 3 block; < 0 = off; default BHRT_TEMPORAL_CLAMP_K */
    float max_length; /* the most samples a history counts for (a floor under the blend weight of new samples); default BHRT_TEMPORAL_MAX_LENGTH */
    int32_t gamma;    /* rgb8: 1 = pow(c, 1/2.2f) before Color24, as bhrt_opts.gamma; default 1 */
    int32_t reserved[5];
} bhrt_temporal_opts;
void bhrt_default_temporal_opts(bhrt_temporal_opts *opts);
int bhrt_temporal_accumulate_dev(bhrt_scene *scene, const bhrt_temporal_opts *opts, const float *d_radiance, float cur_samples, const float *d_history,
                                 const float *d_length, float *d_out, float *d_out_length, uint8_t *d_rgb8, void *stream);
int bhrt_temporal_accumulate(bhrt_scene *scene, const bhrt_temporal_opts *opts, const float *radiance, float cur_samples, const float *history, const float *length,
                             float *out, float *out_length, uint8_t *rgb8);

/* ---- the variance of a temporally accumulated frame: SVGF's temporal half -----------------------------------------------
 * bhrt_render_var* gives bhrt_denoise* the per-channel variance of a pixel's mean; once a frame has been blended with reprojected history that
 * variance no longer describes it.  The two calls below are bhrt_reproject* / bhrt_reproject_moving* and bhrt_temporal_accumulate* with the
 * variance carried beside the light, stated exactly in csrc/temporal.hip as stages 1V and 2V (new kernels beside the existing ones, which
 * do not change): reproject -> accumulate -> denoise then works end to end.  The limits are those of the stages above: lens and shutter are not
 * covered, reflections are carried as surface light, a progressive session is not seeded; and a frame needs >= 2 samples per pixel for a
 * variance (bhrt_render_var's is 0 at 1 spp).
 *
 * bhrt_reproject_var*: prev_xforms == NULL: camera only, the arguments and outputs of bhrt_reproject* (prev_id and id must then be NULL too);
 * else those of bhrt_reproject_moving*.  Two more images: prev_variance (W*H*3), the variance of prev_radiance (bhrt_render_var*'s of a rendered
 * frame, out_variance of an accumulated one), and history_variance (W*H*3, may be NULL), the variance of history: the previous variance
 * interpolated with the history's own bilinear weights over the same valid taps (w, not w^2: never below the variance of the interpolated
 * value for independent taps, and exact for the single tap of a pixel that did not move); with albedo images divided by divisor(prev_albedo)^2
 * and multiplied by divisor(albedo)^2, the square of what the light is rescaled by; 0 where the pixel has no history.  history, length and
 * motion are bhrt_reproject*'s (bhrt_reproject_moving*'s) bytes for the same inputs, with or without the variance pair.  With prev_albedo
 * given, the albedo takes part when history or history_variance is asked for.
 * BHRT_ERR_ARG before any device is touched: everything bhrt_reproject* refuses; with prev_xforms everything bhrt_reproject_moving* refuses;
 * without prev_xforms a prev_id or id that is not NULL; history_variance without prev_variance; prev_variance without prev_radiance.
 * _dev: device pointers (prev_frame and prev_xforms stay HOST pointers); with a stream the call does not synchronise.  Scratch is the scene's
 * and shared with bhrt_reproject* / bhrt_reproject_moving* under their rules: 28 B per pixel for guides computed here, 4 B per pixel for an id
 * computed here, and with prev_xforms the pinned double buffer of the previous records (the third call in a row waits until the stream has
 * passed the first, whichever of the two entry points issued them).  Calls on one scene must not overlap. */
int bhrt_reproject_var_dev(bhrt_scene *scene, const bhrt_reproject_opts *opts, const float prev_frame[12], const struct bhrt_xform *prev_xforms, const float *d_prev_z,
                           const float *d_prev_normal, const float *d_prev_radiance, const float *d_prev_variance, const float *d_prev_length, const float *d_prev_albedo,
                           const int32_t *d_prev_id, const float *d_z, const float *d_normal, const float *d_albedo, const int32_t *d_id, float *d_history,
                           float *d_history_variance, float *d_length, float *d_motion, void *stream);
int bhrt_reproject_var(bhrt_scene *scene, const bhrt_reproject_opts *opts, const float prev_frame[12], const struct bhrt_xform *prev_xforms, const float *prev_z,
                       const float *prev_normal, const float *prev_radiance, const float *prev_variance, const float *prev_length, const float *prev_albedo,
                       const int32_t *prev_id, const float *z, const float *normal, const float *albedo, const int32_t *id, float *history, float *history_variance,
                       float *length, float *motion);
/* bhrt_temporal_accumulate_var*: bhrt_temporal_accumulate* with variance (W*H*3, required): the current frame's, bhrt_render_var*'s;
 * history_variance: bhrt_reproject_var*'s; out_variance (W*H*3, may be NULL): the variance of out.  A pixel without history: out_variance =
 * variance.  A pixel that blends, per channel: out_variance = (1 - a)^2 hv + a^2 variance with the blend's own weight a, where hv =
 * history_variance, raised to max(hv, variance) in a channel whose history the clamp changed (a clamped value comes from the current frame's
 * neighbourhood: it is not trusted more than the current pixel).  With the clamp off and max_length = +inf, frames of n1 and n2 samples
 * pool to (n1^2 v1 + n2^2 v2) / (n1 + n2)^2.  out, out_length and rgb8 are bhrt_temporal_accumulate*'s bytes for the same inputs.
 * out_variance is what bhrt_denoise* takes as variance and what the next bhrt_reproject_var* takes as prev_variance (with out as
 * prev_radiance: the denoised image is for display and is not fed back).
 * BHRT_ERR_ARG before any device is touched: everything bhrt_temporal_accumulate* refuses; a NULL variance; history and length given while
 * history_variance is NULL.  With history or length NULL no pixel has a history: out = radiance, out_variance = variance.
 * _dev: device pointers; with a stream the call does not synchronise.  No scratch. */
int bhrt_temporal_accumulate_var_dev(bhrt_scene *scene, const bhrt_temporal_opts *opts, const float *d_radiance, const float *d_variance, float cur_samples,
                                     const float *d_history, const float *d_history_variance, const float *d_length, float *d_out, float *d_out_variance,
                                     float *d_out_length, uint8_t *d_rgb8, void *stream);
int bhrt_temporal_accumulate_var(bhrt_scene *scene, const bhrt_temporal_opts *opts, const float *radiance, const float *variance, float cur_samples, const float *history,
                                 const float *history_variance, const float *length, float *out, float *out_variance, float *out_length, uint8_t *rgb8);

/* ---- spatial variance estimate: SVGF's variance for a short history ---------------------------------------------------------
 * bhrt_render_var*'s variance is 0 at 1 spp and comes from 2-4 samples at 2-4 spp; a pixel that bhrt_reproject* reports with length 0, every
 * pixel of a sequence's first frame and an imported radiance image have none they can trust.  bhrt_variance_spatial* estimates the variance of
 * such a pixel's mean from the pixel's neighbourhood on its own surface: the unbiased sample variance of the (demodulated) radiance over the
 * taps of a (2 radius + 1)^2 window that pass hard depth and normal stops, in two passes (the mean, then the squared deviations), stated
 * exactly in csrc/temporal.hip as stage 3S and equal to its numpy restatement bit for bit.  The estimate contains the signal's own gradient
 * over the window beside the noise, as SVGF's does.  The limits of bhrt_reproject* stand (pinhole guides: no lens, no shutter).
 *
 * The frame is the scene's camera, W x H.  radiance (W*H*3, required).  variance (W*H*3, may be NULL): the frame's present variance.  length
 * (W*H, may be NULL; needs variance): the samples behind each pixel, bhrt_temporal_accumulate*'s out_length or bhrt_reproject*'s length: a pixel
 * with length >= min_length keeps its variance's bits; a NaN length, and every pixel without a length image, is estimated.  z, normal, albedo:
 * the first hit; each may be NULL = computed here by the kernel of bhrt_first_hit*; albedo is read or computed only with opts.demodulate.
 * out_variance (W*H*3, required): must not alias any input (a pixel's taps are its neighbours' inputs).  A pixel with fewer than two valid
 * taps gets its variance's value, 0 without a variance image.
 * BHRT_ERR_ARG before any device is touched: a NULL scene, options, radiance or out_variance; a radius outside 1..4; a depth_tolerance that is
 * negative or not finite; a NaN normal_threshold; a NaN min_length; a length without a variance.
 * _dev: device pointers; with a stream the call does not synchronise.  Scratch for guides computed here (28 B per pixel) is the scene's,
 * shared with bhrt_denoise* and bhrt_reproject*: calls on one scene must not overlap, a call on another stream included. */
typedef struct bhrt_spatial_variance_opts {
    int32_t radius;         /* R: the window is (2R + 1)^2 taps, 1..4; default 3 (SVGF's 7 x 7) */
    float depth_tolerance;  /* a tap at distance r pixels is the same surface when |z_q - z_p| <= (depth_tolerance * z_p) * r; default 0.01f, bhrt_denoise_opts.sigma_depth's */
    float normal_threshold; /* ... and dot(n_p, n_q) >= normal_threshold; default BHRT_REPROJECT_NORMAL_THRESHOLD */
    float min_length;       /* pixels with length >= min_length keep their variance; default 4 (SVGF: four frames at one sample) */
    int32_t demodulate;     /* 1 (default): estimate on radiance / divisor(albedo); 0: on the radiance, no albedo read or computed */
    int32_t reserved[3];
} bhrt_spatial_variance_opts;
void bhrt_default_spatial_variance_opts(bhrt_spatial_variance_opts *opts);
int bhrt_variance_spatial_dev(bhrt_scene *scene, const bhrt_spatial_variance_opts *opts, const float *d_radiance, const float *d_variance, const float *d_length,
                              const float *d_z, const float *d_normal, const float *d_albedo, float *d_out_variance, void *stream);
int bhrt_variance_spatial(bhrt_scene *scene, const bhrt_spatial_variance_opts *opts, const float *radiance, const float *variance, const float *length, const float *z,
                          const float *normal, const float *albedo, float *out_variance);

/* ---- temporal change test: drop history where a surface's light changed --------------------------------------------------------
 * bhrt_reproject* notices that a pixel shows another surface; it does not notice that the same surface is lit differently: under the shadow, the
 * reflection and the indirect light of an object that moved the history is accepted at full length and the old light fades out over
 * max_length frames.  bhrt_temporal_change* sits between bhrt_reproject_var* and bhrt_temporal_accumulate_var*: over the taps of a
 * (2 radius + 1)^2 window that have history and lie on the pixel's own surface (bhrt_variance_spatial*'s depth and normal stops) it sums the
 * luminance difference d = L(radiance) - L(history) and the luminance variance w = vL(variance) + vL(history_variance), forms
 * x = |sum d| / sqrt(sum w), the difference of the window's mean in standard deviations of its predicted noise, and writes
 * out_length = length * (1 - lambda), lambda = 0 up to sigma_lo, 1 from sigma_hi, linear between.  Stated exactly in csrc/temporal.hip as stage
 * 2C and equal to its numpy restatement bit for bit.  out_length is what bhrt_temporal_accumulate_var* takes as length: it blends more of the
 * new samples, bhrt_variance_spatial* re-estimates the variance of the shortened pixels and the denoiser filters them harder.  A pixel without
 * history keeps its length's bits; a NaN anywhere keeps the history (lambda = 0); history == radiance gives out_length == length bit for bit.
 *
 * The frame is the scene's camera, W x H.  radiance, variance (W*H*3 each): the current frame and the variance of its mean (bhrt_render_var*'s,
 * bhrt_variance_spatial*'s at 1 spp).  history, history_variance (W*H*3 each), length (W*H): bhrt_reproject_var*'s.  z (W*H), normal (W*H*3):
 * the current first hit; each may be NULL = computed here by the kernel of bhrt_first_hit*.  out_length (W*H, required, not the length image: a
 * pixel's taps read their neighbours' lengths).  change (W*H, may be NULL): lambda.
 * BHRT_ERR_ARG before any device is touched: a NULL scene, options or required image; a radius outside 1..4; a sigma that is negative or not
 * finite, sigma_hi < sigma_lo; a depth_tolerance that is negative or not finite; a NaN normal_threshold; out_length == length.
 * _dev: device pointers; with a stream the call does not synchronise.  Scratch for guides computed here (16 B per pixel) is the scene's: calls
 * on one scene must not overlap, a call on another stream included. */
#define BHRT_CHANGE_SIGMA_LO 3.0f /* the measured defaults: DESIGN.md 24 */
#define BHRT_CHANGE_SIGMA_HI 6.0f
typedef struct bhrt_change_opts {
    int32_t radius;         /* R: the window is (2R + 1)^2 taps, 1..4; default 3 */
    float sigma_lo;         /* finite, >= 0: up to here the difference counts as noise (lambda = 0); default BHRT_CHANGE_SIGMA_LO */
    float sigma_hi;         /* finite, >= sigma_lo: from here the history is dropped (lambda = 1); default BHRT_CHANGE_SIGMA_HI */
    float depth_tolerance;  /* bhrt_spatial_variance_opts' meaning and default */
    float normal_threshold; /* bhrt_spatial_variance_opts' meaning and default */
    int32_t reserved[3];
} bhrt_change_opts;
void bhrt_default_change_opts(bhrt_change_opts *opts);
int bhrt_temporal_change_dev(bhrt_scene *scene, const bhrt_change_opts *opts, const float *d_radiance, const float *d_variance, const float *d_history,
                             const float *d_history_variance, const float *d_length, const float *d_z, const float *d_normal, float *d_out_length, float *d_change,
                             void *stream);
int bhrt_temporal_change(bhrt_scene *scene, const bhrt_change_opts *opts, const float *radiance, const float *variance, const float *history,
                         const float *history_variance, const float *length, const float *z, const float *normal, float *out_length, float *change);

/* ---- guided upsampling: render at 1/s of the size, restore full-size edges ----------------------------------------------------
 * The cost of a frame is samples x pixels.  bhrt_upsample* rebuilds a W x H frame from a frame rendered at w x h, W = s w and H = s h, along
 * the full-size first hit, which costs one trace per pixel: a joint bilateral upsampling of the demodulated light.  A full pixel takes the four
 * low pixels around it (the low pixel's colour sits at its centre) with their bilinear weights, drops those that bhrt_variance_spatial*'s
 * hard depth and normal stops say lie on another surface, and multiplies the full-size albedo back in, which carries the texture detail.
 * Stated exactly in csrc/upsample.hip as stage 4U and equal to its numpy restatement on the bytes of every output.
 *
 * The scene is the full-size one, W x H; the low frame's size is given: an integer s in 1..8 with W == s * low_width and H == s * low_height.
 * The low frame is that of the same scene at the low size (bhrt_scene_clone + bhrt_scene_set_resolution), so that low pixel (I, J) covers the
 * full pixels [s I, s I + s) x [s J, s J + s) and its first-hit ray is that of the full pixel (s I, s J).
 * low_radiance (w*h*3, required).  low_variance (w*h*3, may be NULL): the variance of each low pixel's mean.  low_z (w*h), low_normal (w*h*3),
 * required: the low scene's bhrt_first_hit* or bhrt_guides* images, or a low-size session's BHRT_TEMPORAL_IMG_Z / _NORMAL.  low_albedo
 * (w*h*3): required with opts.demodulate, else not read.  z (W*H), normal (W*H*3), albedo (W*H*3): the full-size first hit; each may be NULL =
 * computed here by bhrt_first_hit_dev on the call's stream; albedo is read or computed only with opts.demodulate.
 * Outputs, each may be NULL but not all: out (W*H*3); out_variance (W*H*3; needs low_variance); confidence (W*H): the sum of the bilinear
 * weights of the taps that passed, 0 where no tap passed and opts.fallback decided the pixel (below); rgb8 (W*H*3 bytes: gamma and Color24 of
 * out, as the other stages').  A NaN guide fails the stops; a NaN radiance propagates into the pixels that weigh it.  With s == 1, the same guides on both
 * sides, demodulate == 0 and a radiance without -0, out is the radiance bit for bit.
 * out_variance is each pixel's own variance: sum k^2 v / (sum k)^2 over its taps.  Neighbouring full pixels share taps, so their values are
 * correlated and the frame's noise is NOT independent across pixels: a filter that reads out_variance as independent per-pixel noise
 * (bhrt_denoise*) understates the noise of an average over neighbours by up to s^2.
 * A pixel no tap passes (confidence == 0) takes the taps of its own kind (hit or miss) with their bilinear weights, or all four if there is none.
 * opts.fallback says what it takes from them.  BHRT_UPSAMPLE_FALLBACK_ALBEDO (0, the default): the same sums as every other pixel, so with
 * demodulate the taps' demodulated light times the pixel's own divisor(albedo): light of a surface with another albedo comes out scaled by the
 * ratio of the two.  BHRT_UPSAMPLE_FALLBACK_LIGHT (1): the taps' light as rendered, out = sum k c / S and out_variance =
 * sum k^2 v / S^2 over the raw low_radiance and low_variance, and no albedo is multiplied in: that light was never divided by an albedo the
 * pixel shares.  Pixels with confidence > 0 are the same bytes in both modes, and so is every pixel with demodulate == 0.
 * BHRT_ERR_ARG before any device is touched: a NULL scene, options or required image; low_width or low_height < 1, or no s in 1..8 with
 * W == s * low_width and H == s * low_height; a depth_tolerance that is negative or not finite; a NaN normal_threshold; a fallback that is neither
 * of the two values; all outputs NULL; out_variance without low_variance; an output that is also an input (or another output).
 * _dev: device pointers; with a stream the call does not synchronise.  Scratch for guides computed here (up to 28 B per pixel) is the
 * scene's: calls on one scene must not overlap, a call on another stream included. */
enum { BHRT_UPSAMPLE_FALLBACK_ALBEDO = 0,   /* a pixel no tap passes is summed like every other pixel: the default */
       BHRT_UPSAMPLE_FALLBACK_LIGHT = 1 }; /* a pixel no tap passes takes the taps' modulated light */
typedef struct bhrt_upsample_opts {
    float depth_tolerance;  /* bhrt_spatial_variance_opts' meaning and default (0.01f), with the distance to the tap's guide pixel, at least 1 */
    float normal_threshold; /* bhrt_spatial_variance_opts' meaning and default */
    int32_t demodulate;     /* 1 (default): interpolate radiance / divisor(albedo) and multiply divisor(full albedo) back; 0: the radiance, no albedo read or computed */
    int32_t gamma;          /* of rgb8; default 1, as bhrt_opts.gamma */
    int32_t fallback;       /* BHRT_UPSAMPLE_FALLBACK_*: what a pixel with confidence == 0 takes; default BHRT_UPSAMPLE_FALLBACK_ALBEDO */
    int32_t reserved[3];
} bhrt_upsample_opts;
void bhrt_default_upsample_opts(bhrt_upsample_opts *opts);
int bhrt_upsample_dev(bhrt_scene *scene, const bhrt_upsample_opts *opts, int32_t low_width, int32_t low_height, const float *d_low_radiance,
                      const float *d_low_variance, const float *d_low_z, const float *d_low_normal, const float *d_low_albedo, const float *d_z,
                      const float *d_normal, const float *d_albedo, float *d_out, float *d_out_variance, float *d_confidence, uint8_t *d_rgb8, void *stream);
int bhrt_upsample(bhrt_scene *scene, const bhrt_upsample_opts *opts, int32_t low_width, int32_t low_height, const float *low_radiance,
                  const float *low_variance, const float *low_z, const float *low_normal, const float *low_albedo, const float *z, const float *normal,
                  const float *albedo, float *out, float *out_variance, float *confidence, uint8_t *rgb8);

/* ---- temporal session: the chain above as one device-resident call per frame ---------------------------------------------------
 * A viewport's loop while the camera or an object moves:  bhrt_temporal_begin(scene, &opts, &topts);  then per frame the scene setters
 * (bhrt_scene_set_camera, bhrt_scene_set_node_transform, ...) and bhrt_temporal_frame(scene, rgb8, NULL, NULL);  bhrt_temporal_end(scene).
 * A session belongs to a scene; at most one is open per scene, beside at most one progressive session.  Frame k (0-based since begin or the
 * last reset) runs, on the scene's own stream and on images that stay in HBM:
 *   1. bhrt_first_hit_ex_dev: z, normal, albedo of this view, and the node ids with follow_nodes (one trace per pixel)
 *   2. bhrt_render_var_dev with carry_variance, else bhrt_render_dev, with the session's bhrt_opts and seed + k: the current frame, radiance alone
 *   3. at spp < 2 with spatial_variance: bhrt_variance_spatial_dev(current frame, no variance, no length) is the current frame's variance
 *   4. for k > 0: the reprojection of the kept accumulated frame, its variance and its length out of the kept view (camera frame, first hit,
 *      albedo, and with follow_nodes the node snapshot and the ids) into this one: bhrt_reproject_dev, with follow_nodes
 *      bhrt_reproject_moving_dev, with carry_variance bhrt_reproject_var_dev
 *  4b. for k > 0 with the change test on (bhrt_temporal_set_change): bhrt_temporal_change_dev(current frame, its variance as stage 5 will read
 *      it, history, history variance, history length, this view's z and normal): the used length and the change image; stage 5 then receives
 *      the used length in the place of the history length
 *   5. bhrt_temporal_accumulate_dev / _var_dev with cur_samples = spp (frame 0: no history)
 *   6. with spatial_variance: bhrt_variance_spatial_dev(accumulated frame, its variance, its length): the filter's variance
 *   7. with denoise: bhrt_denoise_dev(accumulated frame, the filter's variance, this view's first hit): the displayed frame
 *   8. the count of the pixels with history (bhrt_temporal_status)
 *   9. bhrt_scene_get_camera_frame, and with follow_nodes bhrt_scene_get_node_transforms: the next frame's "previous"
 *  10. previous and current images change places (pointers)
 * and is, byte for byte, what the same host wrappers give when a host chains them that way (bhrt render --temporal is this loop).  The caller
 * gets the displayed frame: the denoised one with denoise, else the accumulated one; rgb8 with the gamma of the stage that wrote it
 * (denoise_opts.gamma, else temporal.gamma).  The un-denoised accumulated frame and its unmodified variance go on to the next frame.  Between two
 * frames the host's only job is the scene setters; bhrt_render*, bhrt_denoise*, bhrt_first_hit* and the other image calls on the scene between
 * two frames do not disturb the session (the denoiser's and the guides' scratch stays the scene's, the session's images are its own).
 * Streams: everything runs on the scene's own stream, and every call below that touches the device synchronises that stream before it
 * returns (the render does so anyway); calls on one scene must not overlap.
 * Memory: all images are device memory, allocated by the first frame for the session's mode on the device the scene is uploaded to, kept over
 * bhrt_temporal_reset, freed by bhrt_temporal_end and bhrt_scene_free.  Bytes per pixel: light only 116 (two views' first hit 56, current 12,
 * history 12 + 4, two accumulated frames 24 + their lengths 8); carry_variance + 48 (current, history and two accumulated variances);
 * spatial_variance + 12; follow_nodes + 8; the change test + 8 (change, used length); the host variant of bhrt_temporal_frame + 3 for rgb8, and with denoise + 12 for the radiance
 * it copies out.  While a session holds images, bhrt_scene_upload to another device returns BHRT_ERR_ARG and changes nothing.
 * Limits, those of the stages: the guides are the pinhole ray's (no lens, no shutter in them), reflections and refractions are carried as
 * surface light, a light edited between two frames (bhrt_scene_set_light) is noticed only by the change test, one rank (world_size 1), every pixel the same spp. */
typedef struct bhrt_temporal_session_opts {
    bhrt_reproject_opts reproject;
    bhrt_temporal_opts temporal;
    bhrt_spatial_variance_opts spatial;
    bhrt_denoise_opts denoise_opts;
    int32_t carry_variance;   /* 0: bhrt_reproject* + bhrt_temporal_accumulate*; 1: the _var chain on bhrt_render_var* */
    int32_t spatial_variance; /* needs carry_variance: stage 3S where the stages above name it (at spp < 2 on the rendered frame, always on the accumulated one) */
    int32_t denoise;          /* needs carry_variance: the displayed frame is bhrt_denoise*'s */
    int32_t follow_nodes;     /* 1: node-id images and the node snapshot; reprojection through bhrt_reproject_moving* / _var with prev_xforms */
    int32_t reserved[4];
} bhrt_temporal_session_opts;
typedef struct bhrt_temporal_progress {
    uint32_t frames;         /* complete frames since begin or the last reset */
    int32_t failed;          /* 1: a frame failed part-way; only bhrt_temporal_reset and bhrt_temporal_end are served */
    uint64_t history_pixels; /* pixels of the last complete frame whose reprojected length is > 0; 0 after frame 0 */
    uint64_t pixels;         /* W * H */
    int32_t reserved[4];
} bhrt_temporal_progress;
enum {
    BHRT_TEMPORAL_IMG_ACCUMULATED = 0,      /* W*H*3 float: the un-denoised accumulated frame, what the next frame reprojects */
    BHRT_TEMPORAL_IMG_VARIANCE = 1,         /* W*H*3 float: its carried variance (carry_variance) */
    BHRT_TEMPORAL_IMG_LENGTH = 2,           /* W*H float: its length */
    BHRT_TEMPORAL_IMG_HISTORY_LENGTH = 3,   /* W*H float: the reprojected length of the last frame, 0 = the pixel had no history (all 0 after frame 0) */
    BHRT_TEMPORAL_IMG_FILTER_VARIANCE = 4,  /* W*H*3 float: the variance the denoiser was given (spatial_variance) */
    BHRT_TEMPORAL_IMG_Z = 5,                /* W*H float    \                                                    */
    BHRT_TEMPORAL_IMG_NORMAL = 6,           /* W*H*3 float   | the last frame's view: bhrt_first_hit_ex*'s images */
    BHRT_TEMPORAL_IMG_ALBEDO = 7,           /* W*H*3 float   |                                                    */
    BHRT_TEMPORAL_IMG_NODE = 8,             /* W*H int32    /  (follow_nodes)                                     */
    BHRT_TEMPORAL_IMG_CURRENT = 9,          /* W*H*3 float: the last frame's own render */
    BHRT_TEMPORAL_IMG_CURRENT_VARIANCE = 10, /* W*H*3 float: its variance as stage 5 read it (carry_variance) */
    BHRT_TEMPORAL_IMG_CHANGE = 11,          /* W*H float: lambda of the change test (bhrt_temporal_set_change); all 0 after frame 0 */
    BHRT_TEMPORAL_IMG_USED_LENGTH = 12      /* W*H float: the history length stage 5 received, the change test's out_length; all 0 after frame 0 */
};
void bhrt_default_temporal_session_opts(bhrt_temporal_session_opts *opts); /* the four stages' defaults, the four switches 0 */
/* begin: copies the options; needs no device.  BHRT_ERR_ARG, before any device is touched and with nothing changed: a NULL argument; a session
 * already open on the scene; spatial_variance or denoise without carry_variance; carry_variance with spp < 2 and no spatial_variance (a 1-spp
 * frame has no variance); what the stages refuse of their options (bhrt_reproject*, bhrt_temporal_accumulate* with cur_samples = spp,
 * bhrt_variance_spatial*, bhrt_denoise*); what bhrt_render* refuses of its options: spp outside 1..65535, rank, bounce counts, lens, the global
 * gather or photon_map without a map; world_size > 1.
 * frame: rgb8 (W*H*3 bytes) and radiance (W*H*3 floats, linear) receive the displayed frame; either may be NULL.  bhrt_temporal_frame: host
 * pointers; _dev: device pointers, written by the stages themselves (no staging copy).  *stats (may be NULL) is the frame's render's.  A frame
 * that fails once it has launched work marks the session failed: frame, image and image_dev then return BHRT_ERR_ARG, status reports the last
 * complete frame, and bhrt_temporal_reset or bhrt_temporal_end is the way out.
 * reset: a cut.  The next frame is frame 0 again (no history, seed + 0); the images stay allocated; clears a failure.
 * status: frames, the pixels with history in the last complete frame (counted on the device: k_history_count), W * H, failed.
 * image: a copy of one kept image of the last complete frame into host memory; image_dev: its device address, borrowed: valid until the next
 * frame, reset or end.  BHRT_ERR_ARG: an unknown `which`, an image the session's mode does not keep, no complete frame since begin or reset.
 * Without an open session frame, reset, status, image and image_dev return BHRT_ERR_ARG; end returns BHRT_OK. */
int bhrt_temporal_begin(bhrt_scene *scene, const bhrt_opts *opts, const bhrt_temporal_session_opts *topts);
int bhrt_temporal_frame(bhrt_scene *scene, uint8_t *rgb8, float *radiance, bhrt_stats *stats);
int bhrt_temporal_frame_dev(bhrt_scene *scene, uint8_t *d_rgb8, float *d_radiance, bhrt_stats *stats);
int bhrt_temporal_reset(bhrt_scene *scene);
int bhrt_temporal_status(const bhrt_scene *scene, bhrt_temporal_progress *progress);
int bhrt_temporal_image(bhrt_scene *scene, int which, void *host);
int bhrt_temporal_image_dev(bhrt_scene *scene, int which, const void **d_ptr);
int bhrt_temporal_end(bhrt_scene *scene);
/* The change test of a session: bhrt_temporal_session_opts keeps its bytes, so the switch is a call.  opts: copied; NULL = off,
 * the state after begin.  Legal while a session is open and no frame has completed since begin or the last reset.  With the test on, frame
 * k > 0 runs step 4b above; the two images it writes are kept (BHRT_TEMPORAL_IMG_CHANGE, _USED_LENGTH; with the test off the session's mode
 * does not keep them).  BHRT_TEMPORAL_IMG_HISTORY_LENGTH and bhrt_temporal_progress.history_pixels stay the reprojected length's: they answer
 * "did this pixel find its surface", which the change test does not alter.  bhrt_temporal_reset keeps the setting, bhrt_temporal_end drops it.
 * Without this call every frame is byte for byte what it is without the stage.
 * BHRT_ERR_ARG with nothing changed: a NULL scene; no open session; a complete frame already exists; a session without carry_variance (the
 * test reads both variances); what bhrt_temporal_change* refuses of the options. */
int bhrt_temporal_set_change(bhrt_scene *scene, const bhrt_change_opts *opts /* NULL = off */);

/* ---- adaptive sampling: RenderImage's per-pixel sample counts (Scenes/scene.h:534,570), which BeginRender only ever sets to 0
 * (Main.cpp:214), filled by a render that stops sampling a pixel once its mean is good enough ------------------------
 * Rounds: round 0 gives every owned pixel samples [0, min_spp); round r >= 1 gives every pixel still active samples [n_{r-1}, n_r),
 * n_r = min(max_spp, 2 n_{r-1}), max_spp = bhrt_opts.spp: ceil(log2(max / min)) + 1 rounds at most.  Every sample has the RNG key of
 * bhrt_render's (seed, pixel, sample index), so a pixel's outputs are bit-identical to bhrt_render_var's at that pixel's count.
 * A pixel keeps, in float32 and in sample order, the running sum S (mean = S / (float)n, bhrt_render's operations) and a Welford
 * recurrence per channel (d = x - mu; mu += d / k; M2 += d (x - mu), k = 1..n).  After each round it takes part in:
 *   v_c = (M2_c / (n - 1)) / n      (variance of the mean, per channel)
 *   L   = (0.2126 m_r + 0.7152 m_g) + 0.0722 m_b,   vL = (0.2126^2 v_r + 0.7152^2 v_g) + 0.0722^2 v_b
 *   the pixel retires when n == max_spp or sqrt(vL) <= threshold * max(L, floor).
 * The test reads the pixel's own samples only: results do not depend on rank, world size, tile size or pass size.  After the last
 * round every owned pixel's radiance, RGB8 bytes (bhrt_opts.gamma as bhrt_render), variance (laid out like bhrt_render_var's) and count n are
 * written, once; pixels of other ranks' tiles are left untouched.  What the images hold after a call that returned an error is unspecified.  Ranks may finish unevenly: adaptive work is not rebalanced between them. */
typedef struct bhrt_adaptive_opts {
    int32_t min_spp;  /* samples of round 0, >= 2; bhrt_opts.spp is the per-pixel maximum (<= 65535); default 16 */
    float threshold;  /* relative standard error of the mean's luminance; < 0 = never retire early (every pixel reaches spp), +inf = every
                       * pixel retires at min_spp; default: DESIGN.md 10 */
    float floor;      /* luminance below which the error is taken relative to `floor` (> 0); default: DESIGN.md 10 */
    int32_t reserved[5];
} bhrt_adaptive_opts;
void bhrt_default_adaptive_opts(bhrt_adaptive_opts *a);
/* The arguments are checked before any device is touched: 2 <= min_spp <= spp <= 65535, floor > 0, threshold not NaN, else BHRT_ERR_ARG.
 * rgb8 / radiance / variance: as bhrt_render_var's (each may be NULL); count: W*H uint32 samples per pixel (may be NULL).
 * stats->camera_samples = the sum of the counts of the owned pixels inside the image.  _dev: device pointers (the render synchronises its
 * own stream); the state of the rounds (48 B per owned pixel) belongs to the scene. */
int bhrt_render_adaptive_dev(bhrt_scene *scene, const bhrt_opts *opts, const bhrt_adaptive_opts *aopts, uint8_t *d_rgb8, float *d_radiance, float *d_variance,
                             uint32_t *d_count, bhrt_stats *stats, void *stream);
int bhrt_render_adaptive(bhrt_scene *scene, const bhrt_opts *opts, const bhrt_adaptive_opts *aopts, uint8_t *rgb8, float *radiance, float *variance,
                         uint32_t *count, bhrt_stats *stats);
/* RenderImage::ComputeSampleCountImage (scene.h:603-626): smin / smax over the n counts, img = (255 (s - smin)) / (smax - smin) in integers,
 * clamped to 0..255, 0 everywhere when smax == smin; *smax (a host pointer, may be NULL) = smax, the function's return value there.
 * _dev: device count and image, synchronises (the range scratch is shared with the other API calls); the other: host pointers. */
int bhrt_sample_count_image_dev(bhrt_scene *scene, const uint32_t *d_count, size_t n, uint8_t *d_img, uint32_t *smax, void *stream);
int bhrt_sample_count_image(bhrt_scene *scene, const uint32_t *count, size_t n, uint8_t *img, uint32_t *smax);
/* RenderImage::SaveSampleCountImage (scene.h:630): an 8-bit one-channel PNG of w x h bytes */
int bhrt_save_png_gray(const char *path, const uint8_t *gray, int width, int height);

/* ---- progressive rendering: the frame as a state that a call advances by a few samples per pixel and that can be read at any point
 * (DESIGN.md 15).  BeginRender() starts a frame the viewport shows filling in, and StopRender() (Main.cpp:243) ends it whenever the user
 * likes: begin / step / frame / end.  A session belongs to a scene; at most one is open per scene.
 * Every active pixel of the session stands at the same count c.  bhrt_progressive_step(n) renders samples [c, min(spp, c + n)) of every
 * active pixel, each with the RNG key of bhrt_render's (seed, pixel, sample index), and folds them into the pixel's state in float32 and in
 * sample order with the operations of the adaptive rounds above (S += x; d = x - mu; mu += d / k; M2 += d * (x - mu)).  A pixel at its new
 * count c' then retires when c' == spp, or, with adaptive options, when c' >= min_spp and sqrt(vL) <= threshold * max(L, floor) (L, vL as
 * above).  Without adaptive options only the maximum retires a pixel.  So a uniform session's frame at count c is bhrt_render's at spp = c bit
 * for bit, and a session stepped min_spp, min_spp, 2 min_spp, ... is bhrt_render_adaptive's.  A retired pixel keeps its state: the frame keeps
 * returning the value it retired with.
 * The state (40 B per owned pixel: S, mu, M2, count; plus two lists of 4 B) lives in a buffer of its own that belongs to the scene; it is
 * allocated by the first step or frame, on the device the scene is uploaded to, and freed by bhrt_progressive_end and bhrt_scene_free.  While a
 * session holds state there, bhrt_scene_upload to another device returns BHRT_ERR_ARG and changes nothing (end the session first); to the same
 * device it stays the no-op it is.  bhrt_render*, bhrt_render_adaptive*,
 * bhrt_first_hit* and bhrt_denoise* on the same scene between two steps do not disturb the session.  The scene setters (bhrt_scene_set_lens,
 * _set_camera, _set_shutter, _set_emissive, _set_material_emission, _set_face_materials, _set_global_gather, the photon and global maps) between two steps apply to
 * the samples rendered afterwards: the frame then mixes samples of both states. */
typedef struct bhrt_progress {
    uint32_t steps;            /* bhrt_progressive_step calls that rendered something */
    uint32_t spp_min, spp_max; /* smallest / largest count over this rank's pixels inside the image */
    uint64_t active_pixels;    /* pixels that the next step would still sample */
    uint64_t camera_samples;   /* sum of the counts */
    int32_t finished;          /* 1 = no active pixel is left */
    int32_t reserved[3];
} bhrt_progress;
/* begin: copies the options.  bhrt_opts.spp is the per-pixel maximum, 1 <= spp <= 65535; rank, world_size, tile_size and samples_per_pass mean
 * what they mean for bhrt_render; aopts = NULL: a uniform session.  Checked before any device is touched, BHRT_ERR_ARG otherwise: the options as
 * bhrt_render_adaptive checks its own (lens, the global gather without a map, photon_map without a map), with aopts 2 <= min_spp <= spp,
 * floor > 0 and threshold not NaN, and that no session is open on the scene.  Needs no device.
 * step: n_samples <= 0 or no open session: BHRT_ERR_ARG.  *stats (may be NULL) is that step's alone.  A step on a finished session returns
 * BHRT_OK, renders nothing and does not count in bhrt_progress.steps.  A step that fails once it has started rendering (BHRT_ERR_HIP,
 * BHRT_ERR_OVERFLOW, ...) may have folded some of its passes: the session is marked failed, bhrt_progressive_step and _frame* return BHRT_ERR_ARG
 * from then on, bhrt_progressive_status reports the last complete step, and bhrt_progressive_end is the way out.
 * frame: resolves the state into the caller's images for this rank's pixels inside the image, at any time in an open session, any number of
 * times: radiance = S / (float)c, rgb8 = gamma + Color24 of it (the session's bhrt_opts.gamma), variance = (M2 / (float)(c - 1)) / (float)c
 * (0 at c == 1), count = c; pixels at count 0 (before the first step) are written as zeros, pixels of other ranks' tiles are left untouched.
 * Layouts as bhrt_render_adaptive's; any pointer may be NULL.  _dev: device pointers; with a stream the kernel is enqueued there and the call
 * does not synchronise (the caller does, before the next call on this scene); stream = NULL: the scene's own stream, synchronised.
 * end: the StopRender of the seam: closes the session and frees its state; BHRT_OK when no session is open. */
int bhrt_progressive_begin(bhrt_scene *scene, const bhrt_opts *opts, const bhrt_adaptive_opts *aopts /* NULL = uniform */);
int bhrt_progressive_step(bhrt_scene *scene, int32_t n_samples, bhrt_stats *stats);
int bhrt_progressive_frame(bhrt_scene *scene, uint8_t *rgb8, float *radiance, float *variance, uint32_t *count);
int bhrt_progressive_frame_dev(bhrt_scene *scene, uint8_t *d_rgb8, float *d_radiance, float *d_variance, uint32_t *d_count, void *stream);
int bhrt_progressive_status(const bhrt_scene *scene, bhrt_progress *progress);
int bhrt_progressive_end(bhrt_scene *scene);

/* ---- test hook: csrc/bhrt_detmath.h evaluated on the device, to prove host and device produce the same bits.
 * fn: 0 sin 1 cos 2 tan 3 acos 4 asin 5 atan2(a,b) 6 pow(a,b) 7 rand_to_unit(bits of a) 8 a/b 9 sqrt(a); host pointers */
int bhrt_math_eval_dev(int fn, const float *a, const float *b, size_t n, float *out);

/* ---- image output (RenderImage::SaveImage, Scenes/scene.h:628-644) ------------------------------- */
int bhrt_save_png(const char *path, const uint8_t *rgb8, int width, int height);

#ifdef __cplusplus
}
#endif
#endif /* BHRT_H */
