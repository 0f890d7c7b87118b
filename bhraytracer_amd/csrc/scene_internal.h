// scene_internal.h — the opaque bhrt_scene handle behind include/bhrt.h
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "bhrt.h"
#include "scene_host.h"

namespace bhrt {
struct DeviceState; // device_state.h (part of the kernels.hip translation unit)
void SetError(const std::string &msg);
// No C++ exception crosses the C ABI: every `int bhrt_*` entry point is a function-try-block that ends in this handler
// (std::bad_alloc from a file-sized allocation, std::length_error, ...): sets bhrt_last_error() and returns an error code.
int AbiException();
void DestroyDeviceState(DeviceState *d); // defined in the HIP TU

// What the setters of scene_edit.cpp call after they have changed scene->flat; defined in the HIP TU.  Each brings one part of an uploaded
// scene's device copy up to date, and returns (BHRT_OK) at once when the scene is not uploaded.  The two that cannot fail return nothing.
void RefreshCamera(bhrt_scene *scene);       // the kernels' camera (DevScene::cam) from the header's
void RefreshShutter(bhrt_scene *scene);      // the kernels' shutter (DeviceState::shutter) from FlatScene::shutter*
int RefreshCamChain(bhrt_scene *scene);      // DevScene::cam_chain, filled and uploaded again: the camera has moved
int RefreshNodeXform(bhrt_scene *scene, size_t off, const bhrt_xform &xf); // a node's record, at byte off of the blob, then cam_chain: the node is on some chain
int RefreshLights(bhrt_scene *scene);        // the blob's lights[], DevScene::light_pick and ::all_light_intensity: a light was edited
int RefreshEmission(bhrt_scene *scene);      // FlatScene::emission / emissive
int RefreshFaceMaterials(bhrt_scene *scene); // FlatScene::face_materials

// The host side of a progressive session (bhrt_progressive_*): the options it was begun with and what the steps so far have left.
// Everything bhrt_progressive_status reports is kept here: a step reads back one word (the next list's length), and every pixel that left
// the list in a step retired at that step's count.  The per-pixel state is device memory (DeviceState::d_prog), allocated by the first step or frame.
struct ProgressiveSession {
    bool open = false, adaptive = false;
    bool failed = false;         // a step failed part-way: passes may be folded that c and the lists do not know of; only end is left
    uint64_t id = 0;             // names the session; DeviceState::prog_session says whose state d_prog holds, so the state's validity lives with the buffer
    bhrt_opts o = {};
    bhrt_adaptive_opts a = {};
    uint32_t c = 0;              // the count every active pixel stands at
    uint32_t steps = 0;
    uint32_t first_retired = 0;  // the count of the first pixels that retired; 0 = none has
    uint64_t owned = 0;          // owned-pixel indices of this rank (edge-tile pixels outside the image included)
    uint64_t active = 0;         // active pixels inside the image
    uint64_t retired_samples = 0; // sum of the counts of the retired pixels
    int cur = 0;                 // which of the two device lists holds the active pixels (c > 0; the first step takes the range [0, owned))
};

// The temporal session (bhrt_temporal_*) lives in temporal_session.hip, a translation unit above the public _dev entry points; the
// scene owns it through a pointer.  What that unit needs from the scene's device state is defined in the kernels.hip unit.
struct TemporalSession;
void DestroyTemporalSession(TemporalSession *t);            // frees its images on their device; nullptr: nothing
bool TemporalSessionHoldsBuffers(const TemporalSession *t); // bhrt_scene_upload to another device is refused while it does
void *SceneStream(const bhrt_scene *scene);                 // the scene's own hipStream_t; nullptr before the upload
int SceneDevice(const bhrt_scene *scene);                   // the device the scene is uploaded to; -1 before the upload
int RenderArgsCheck(bhrt_scene *scene, const bhrt_opts *opts); // what bhrt_render* refuses of its options, host arithmetic only

// The guides bhrt_temporal_change* computes itself (z, normal: 16 B per pixel) live in temporal_change.hip, above the public _dev entry points
// like the session; the scene owns them through a pointer.
struct ChangeScratch;
// Likewise the full-size guides bhrt_upsample* computes itself (z, normal, albedo: up to 28 B per pixel), in upsample.hip.
struct UpsampleScratch;
} // namespace bhrt

struct bhrt_scene {
    bhrt::FlatScene flat;
    uint32_t n_triangles = 0, n_bvh_nodes = 0, max_bvh_depth = 0;
    bhrt::DeviceState *dev = nullptr;
    bhrt::ProgressiveSession prog; // not carried by bhrt_scene_clone
    bhrt::TemporalSession *temporal = nullptr; // bhrt_temporal_begin .. _end; not carried by bhrt_scene_clone
    // how bhrt_scene_free (capi_host.cpp, which also links into host-only programs without the HIP units) releases it: set with `temporal`
    void (*temporal_release)(bhrt::TemporalSession *) = nullptr;
    bhrt::ChangeScratch *change_scratch = nullptr; // allocated by the first bhrt_temporal_change* call that is given no guides; not carried by bhrt_scene_clone
    void (*change_scratch_release)(bhrt::ChangeScratch *) = nullptr; // set with `change_scratch`, for bhrt_scene_free
    bhrt::UpsampleScratch *upsample_scratch = nullptr; // allocated by the first bhrt_upsample* call that is given no full-size guides; not carried by bhrt_scene_clone
    void (*upsample_scratch_release)(bhrt::UpsampleScratch *) = nullptr; // set with `upsample_scratch`, for bhrt_scene_free
};
