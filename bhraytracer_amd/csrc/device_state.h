// device_state.h — what a scene owns on its device: memory, streams, events, the installed photon map.
// Part of the kernels.hip translation unit, included there behind the kernels (it uses their argument types and HIP_CHECK); not a header for
// other files: they see `struct DeviceState;`, DestroyDeviceState and the Refresh* hooks of the scene setters (scene_internal.h).
#pragma once
#include "dev_buf.h" // DevBuf, PinnedBuf

namespace bhrt {

// Streams and events of a DeviceState.  A base class, so that it is destroyed AFTER the members of DeviceState: device memory is released
// (hipFree waits for the device) before the streams go.
struct DeviceQueues {
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t stream2 = nullptr;             // k_trace_slow runs here, beside the pass
    std::vector<hipEvent_t> slow_events;       // one per k_trace_slow launch of a pass (its hits are in place)
    hipStream_t stream3 = nullptr;             // any-hit work of a wave step beside the next step's closest-hit work (WavePass::sh_overlap, knobs.shadow_overlap)
    hipEvent_t ev_shade = nullptr, ev_shadow[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> ev_pool;           // Timer
    DeviceQueues() = default;
    DeviceQueues(const DeviceQueues &) = delete;
    DeviceQueues &operator=(const DeviceQueues &) = delete;
    ~DeviceQueues()
    {
        if (ev_shade) (void)hipEventDestroy(ev_shade);
        for (int k = 0; k < 2; k++) if (ev_shadow[k]) (void)hipEventDestroy(ev_shadow[k]);
        if (stream3) (void)hipStreamDestroy(stream3);
        for (int k = 0; k < 2; k++) if (ev[k]) (void)hipEventDestroy(ev[k]);
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
        for (hipEvent_t e : slow_events) (void)hipEventDestroy(e);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Scratch of the photon gather (GatherPass), kept from call to call.
struct GatherWorkspace {
    uint32_t cap = 0;             // queries the next six have room for, and what d_sort_temp is sized for (Reserve)
    DevBuf<uint32_t> d_heavy, d_long; // queries that met 1000 photons in the lane pass; queries whose walk outlasted its lane budget
    DevBuf<uint32_t> d_cell_of, d_gorder, d_rank_of, d_keys_out; // gather order (cell sort)
    DevBuf<uint8_t> d_sort_temp; size_t sort_temp_bytes = 0;
    DevBuf<uint32_t> d_cells, d_tile_sums; // the counting sort: a count per cell and one entry more, and its scan's tile sums
    DevBuf<uint32_t> d_sel;       // candidate scratch of the selection pass's waves (grown by the pass)
    DevBuf<unsigned long long> d_scr; uint32_t scr_lanes = 0; // candidate heaps of the exact replay: BHRT_HEAP_COLUMN x scr_lanes, element-major (grown by the replay)
    DevBuf<GatherCounters> d_cnt;    // what the kernels count, one group per pass
    PinnedBuf<GatherCounters> h_cnt; // its host copy: a pass reads back the group it cleared
    // Room for a gather of cnt queries.  A failed regrow leaves cap 0, so the next call tries again.
    int Reserve(uint32_t cnt, hipStream_t stream)
    {
        if (cap < cnt) {
            cap = 0;
            DevBuf<uint32_t> *const lists[] = {&d_heavy, &d_long, &d_cell_of, &d_gorder, &d_rank_of, &d_keys_out};
            for (DevBuf<uint32_t> *buf : lists) buf->Free();
            d_sort_temp.Free();
            for (DevBuf<uint32_t> *buf : lists) BHRT_TRY(buf->Reserve(cnt));
            if (GatherSortPairs(nullptr, nullptr, nullptr, nullptr, cnt, nullptr, &sort_temp_bytes, 28, stream) != 0) { SetError("gather sort: temp size"); return BHRT_ERR_HIP; }
            BHRT_TRY(d_sort_temp.Reserve(std::max<size_t>(sort_temp_bytes, 16)));
            cap = cnt;
        }
        BHRT_TRY(d_cnt.Reserve(1));
        BHRT_TRY(d_cells.Reserve((size_t)BHRT_GATHER_CELLS + 1));
        BHRT_TRY(d_tile_sums.Reserve((size_t)(BHRT_GATHER_CELLS / kScanTile + kScanBlock)));
        return h_cnt ? BHRT_OK : h_cnt.Alloc(1);
    }
};

// An installed photon map: the balanced 24-byte records (heap order, slot 0 unused), the decoded copy the gather walks, and the host copy a
// getter fetches on demand.  InstallPhotonMapDev fills one.
struct PhotonSlot {
    DevBuf<DPhoton> d_photons;
    uint32_t n_photons = 0;
    std::vector<HostPhoton> h_photons; // balanced copy for bhrt_photon_get / _export, bhrt_global_map_get
    DevBuf<float4> d_ph_hot, d_ph_cold, d_ph_dbox; // decoded copy the gather walks (PhotonMapDev)
    PhotonMapDev pm = {};
    void Clear() { d_photons.Free(); d_ph_hot.Free(); d_ph_cold.Free(); d_ph_dbox.Free(); n_photons = 0; h_photons.clear(); pm = PhotonMapDev{}; }
};

struct DeviceState : DeviceQueues {
    int device = -1;
    uint32_t n_cus = 256; // compute units of the device (hipDeviceProp_t::multiProcessorCount): sizes the grids of the resident-wave kernels
    DevBuf<uint8_t> d_blob;
    DevBuf<int32_t> d_chain;
    DevBuf<float> d_aux; // mat_r0 + light_pick (DevScene)
    DevBuf<bhrt_texcolor> d_emission;  // FlatScene::emission, uploaded with the scene; Frames::emission points here while the term is on
    bool emission_on = false;          // bhrt_scene_set_emissive
    bool emission_textured = false;    // some material's emission has a map
    bool le_on = false;                // the running render keeps Le per frame (Frames::le): term on and emission_textured
    DevBuf<float> d_le;                // 3 * cap_frames floats, only then
    // face materials, built at upload for a scene that has sub-materials: the extended material table (the blob's materials, then
    // FlatScene::sub_materials), its Schlick R0s, and FaceMtlTable's array.  S.materials / S.mat_r0 point at them only while the switch is on
    DevBuf<bhrt_material> d_mtl_ext;
    DevBuf<float> d_r0_ext;
    DevBuf<int32_t> d_fm_tab;
    FaceMtlTable fm = {nullptr, 0}; // fm.tab != null: bhrt_scene_set_face_materials is on and the scene has sub-materials
    DevScene S;
    ShutterInfo shutter = {};                  // the kernels' copy of the scene's shutter (RefreshShutter): pose 1's frame; on = 0: no shutter kernel runs
    // wavefront workspace (EnsureWorkspace)
    uint32_t cap_samples = 0, cap_rays = 0, cap_frames = 0;
    DevBuf<float> d_rayf[2];                   // 6 * cap_rays floats each
    DevBuf<uint32_t> d_rayu[2];                // 3 * cap_rays
    DevBuf<float> d_hitf;                      // cap_rays
    DevBuf<int32_t> d_hiti;                    // 3 * cap_rays
    DevBuf<float> d_shf;                       // 7 * cap_rays
    DevBuf<uint32_t> d_shu;                    // cap_rays
    DevBuf<uint32_t> d_fu;                     // 4 * cap_frames
    DevBuf<uint64_t> d_fcode;                  // cap_frames
    DevBuf<float> d_ff;                        // (3*7 + 2) * cap_frames
    DevBuf<float> d_samples;                   // 3 * cap_samples
    DevBuf<uint32_t> d_root;                   // cap_samples: sample slot -> its root Shade() frame, or kNoRootFrame (k_shade -> k_resolve_frames)
    DevBuf<uint32_t> d_order;                  // 4 * BHRT_ORDER_SHARDS * order_shard_cap (shading order, device_types.h::RayOrder)
    uint32_t order_shard_cap = 0;
    DevBuf<uint32_t> d_seg;                    // seg_start[97] + seg_count[96] + mesh_start[33] + mesh_count[33] + frame_base[96]
    DevBuf<uint32_t> d_park;                   // park_key[cap_rays] + park_sorted[cap_rays] + park_rank[cap_rays] + buckets + tile sums (RayOrder)
    DevBuf<float> d_slowf;                     // slow queue (SlowQueue): 6 * kSlowCap floats, then kSlowCap hit distances
    DevBuf<uint32_t> d_slowu;                  // 3 * kSlowCap, then 3 * kSlowCap hit words (node, prim, front)
    // the any-hit work beside the pass (stream3): the second shadow queue, its own parked list (the RC_MESH part of a RayOrder), segment table
    // and counters
    DevBuf<float> d_shf2;                      // 7 * cap_rays
    DevBuf<uint32_t> d_shu2;                   // cap_rays
    DevBuf<uint32_t> d_order_sh;               // BHRT_ORDER_SHARDS * order_shard_cap
    DevBuf<uint32_t> d_seg_sh;                 // mesh_start[33] + mesh_count[33]
    DevBuf<Counters> d_cnt_sh;
    DevBuf<Counters> d_cnt;
    PinnedBuf<HostCounters> h_pub; // device-visible: written by publish_counters
    HostCounters *d_pub = nullptr; // the device's address of h_pub
    uint32_t pub_seq = 0;
    int timers = 0;                // bhrt_opts.timers of the running call
    struct PendingTimer { int e0, e1; double *acc; };
    std::vector<PendingTimer> ev_pending;
    std::vector<int> ev_free;                  // indices of ev_pool not in use
    // the caustic photon map (bhrt_photon_build / _install / _import) and the global one (bhrt_global_map_build / _set): independent slots
    PhotonSlot cmap, gmap;
    DevBuf<float> d_ph_frames;         // 15 * cap_frames floats (p, N, V, kd, ks per frame), only with photon_map or the global gather
    GatherWorkspace gw;
    // Development switches, read from the environment ONCE, when the scene is uploaded (none changes a result), and the two test knobs, which
    // no environment variable reaches: only bhrt_scene_knob sets them.
    struct Knobs {
        int stream_waves = -1;          // BHRT_STREAM_WAVES: resident waves of k_trace_mesh_stream; 0 = the launch-per-64-rays kernel; -1 = default
        bool fused_camera = true;       // BHRT_FUSED_CAMERA=0: two-kernel camera step in mesh-free scenes
        bool no_slow_queue = false;     // BHRT_NO_SLOW_QUEUE: axis-parallel rays stay in their wave steps
        bool debug_slow = false, debug_gather = false, debug_drain = false; // BHRT_DEBUG_*: statistics on stderr
        bool balance_host = false;      // BHRT_PHOTON_BALANCE_HOST: photon_host.cpp instead of k_pb_level (the tests' second opinion)
        int frame_cap = 0;              // knob "frame_cap": a frame pool that overflows (the retry path under test); 0 = off
        int gather_lane_budget = 0;     // knob "gather_lane_budget": photons a lane may visit before its query goes to the one-wave pass; 0 = default
        bool gather_counting_sort = false; // BHRT_GATHER_COUNTING_SORT=1: the cell order by the counting sort instead of the radix sort of pairs
        bool shadow_overlap = true;     // BHRT_SHADOW_OVERLAP=0: the any-hit kernels of a wave step on the pass's own stream, in front of the next step
        bool fused_resolve = true;      // BHRT_FUSED_RESOLVE=0, knob "fused_resolve": a plain render resolves through the sample buffer (k_combine's root level + k_resolve)
        bool finish_misses = true;      // BHRT_FINISH_MISSES=0, knob "finish_misses": k_trace_closest files the rays that left the scene for k_shade like every other ray
        int gather_stats = 0;           // knob "gather_stats": the lane pass counts the photons its answers are made of (bhrt_stats.photon_found), 7 % slower
        void FromEnv()
        {
            if (const char *e = getenv("BHRT_STREAM_WAVES")) stream_waves = atoi(e);
            if (const char *e = getenv("BHRT_FUSED_CAMERA")) fused_camera = atoi(e) != 0;
            no_slow_queue = getenv("BHRT_NO_SLOW_QUEUE") != nullptr;
            debug_slow = getenv("BHRT_DEBUG_SLOW") != nullptr; debug_gather = getenv("BHRT_DEBUG_GATHER") != nullptr; debug_drain = getenv("BHRT_DEBUG_DRAIN") != nullptr;
            if (const char *e = getenv("BHRT_PHOTON_BALANCE_HOST")) balance_host = atoi(e) != 0;
            if (const char *e = getenv("BHRT_GATHER_COUNTING_SORT")) gather_counting_sort = atoi(e) != 0;
            if (const char *e = getenv("BHRT_SHADOW_OVERLAP")) shadow_overlap = atoi(e) != 0;
            if (const char *e = getenv("BHRT_FUSED_RESOLVE")) fused_resolve = atoi(e) != 0;
            if (const char *e = getenv("BHRT_FINISH_MISSES")) finish_misses = atoi(e) != 0;
        }
    } knobs;
    // a capacity overflow halves the pass (RenderPixels); later frames of the same scene and options start from the reduced size
    uint64_t pass_hint_key = 0;
    uint32_t pass_hint = 0;
    uint64_t frames_seen_key = 0; // Shade() frames per sample slot the passes of a render (scene, options: the key) have needed so far (max)
    double frames_seen = 0;
    // bhrt_render / _var / _adaptive: the device copy of the frame, kept between calls (FrameStage); the variance and count images on first use
    size_t frame_px = 0; // pixels of d_frame_rgb and d_frame_rad
    DevBuf<uint8_t> d_frame_rgb;
    DevBuf<float> d_frame_rad, d_frame_var;
    DevBuf<uint32_t> d_frame_cnt;
    // The estimator's state (FoldViews, kernels.hip): FoldState, 40 B per owned pixel, two lists of owned-pixel indices (4 B each) and the next
    // list's length: 48 B per owned pixel + 16.  Two buffers of that layout:
    // bhrt_render_adaptive_dev: the state of the rounds; grown on demand, never zeroed (round 0 writes what the frame kernel reads)
    DevBuf<uint8_t> d_ad;
    // bhrt_progressive_*: the session's state.  No render entry point touches it; freed by bhrt_progressive_end
    DevBuf<uint8_t> d_prog;
    uint64_t prog_session = 0; // ProgressiveSession::id of the session whose state d_prog holds (allocated and zeroed for it); 0 = none
    // bhrt_denoise_dev: the filter's planes (DenoisePlaneBytes), then the first-hit guides it computes itself; grown on demand
    DevBuf<uint8_t> d_dn;
    // bhrt_guides_dev: the running sums between the sample chunks of a call (k_guides), 32 B per pixel of a pass; only when spp exceeds one chunk
    DevBuf<float4> d_guides;
    // bhrt_reproject_moving_dev: the previous node records with moved[] (88 B per node), and the node-id image it computes itself (4 B per pixel).
    // The records travel on the call's stream from pinned memory.  Two slots used in turn, each with an event recorded behind the call's kernel:
    // a slot's pinned words are written again only after the stream has passed the call that used them last.
    struct MovingNodeSlot {
        PinnedBuf<uint32_t> h;
        DevBuf<uint32_t> d;
        hipEvent_t done = nullptr;
        bool used = false;
        MovingNodeSlot() = default;
        MovingNodeSlot(const MovingNodeSlot &) = delete;
        MovingNodeSlot &operator=(const MovingNodeSlot &) = delete;
        ~MovingNodeSlot() { if (done) (void)hipEventDestroy(done); }
    } moving_nodes[2];
    uint32_t moving_turn = 0;
    DevBuf<int32_t> d_moving_id;
    // scratch for the public trace API (EnsureApiScratch)
    size_t api_cap = 0; // rays
    DevBuf<float> d_api_f;   // 9 * api_cap
    DevBuf<int32_t> d_api_i; // 3 * api_cap
};

void DestroyDeviceState(DeviceState *d)
{
    if (!d) return;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    delete d; // the buffers, then (DeviceQueues) the events and streams
}

} // namespace bhrt
