// temporal.h — launchers of the image-space stages of temporal.hip (bhrt_reproject*, bhrt_temporal_accumulate* and their variance-carrying
// forms bhrt_reproject_var*, bhrt_temporal_accumulate_var*, and bhrt_variance_spatial*; kernels.hip owns the scene state and the first-hit kernel that fills in the guides
// a caller leaves out).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "bhrt.h"
#include "bhrt_flat.h"

namespace bhrt {

struct ReprojectJob {
    int W, H;
    bhrt_reproject_opts o;
    float cur[12];              // pos, top_left, dd_x, dd_y of the scene's camera now
    float prev[12];             // the same of the previous view
    const float *prev_z;        // W*H
    const float *prev_normal;   // W*H*3
    const float *prev_radiance; // W*H*3, or NULL when no history image is asked for
    const float *prev_length;   // W*H, or NULL = 1 everywhere
    const float *prev_albedo;   // W*H*3, or NULL: no albedo takes part
    const float *z, *normal;    // the current view's first hit
    const float *albedo;        // read only with prev_albedo
    float *history;             // W*H*3, or NULL
    float *length;              // W*H, or NULL
    float *motion;              // W*H*2, or NULL
};

// "" when the arguments are usable, else what is wrong with them (host arithmetic only)
const char *ReprojectArgsError(const bhrt_reproject_opts *o, const float *prev_frame, const float *prev_radiance, const float *prev_albedo);
hipError_t ReprojectLaunch(const ReprojectJob &J, hipStream_t s);

// stage 1 through object motion (k_reproject_moving): the job above and what says where every node was
constexpr int kPrevNodeWords = 22; // a node's previous record in the scene's scratch: tm'[9], pos'[3], itm'[9], then moved (int32): 88 B
struct ReprojectMovingJob : ReprojectJob {
    const bhrt_node *nodes;    // device: the scene's nodes, the current records
    const int32_t *chain;      // device: n_nodes x BHRT_MAX_NODE_DEPTH, the depth-1 ancestor first (DeviceState::d_chain)
    const uint32_t *prev_nodes; // device: n_nodes x kPrevNodeWords
    int n_nodes;
    const int32_t *prev_id;    // W*H, or NULL: the previous view's node ids take no part
    const int32_t *id;         // W*H: the current view's
};
// "" when the snapshot is usable (non-NULL, every value finite; n_nodes == 0 reads nothing)
const char *ReprojectMovingArgsError(const bhrt_xform *prev_xforms, uint32_t n_nodes);
// fills n_nodes x kPrevNodeWords words from the snapshot and the scene's nodes: moved = the bytes of the node's record or of an ancestor's differ
void FillPrevNodes(const bhrt_node *nodes, const bhrt_xform *prev_xforms, uint32_t n_nodes, uint32_t *out);
hipError_t ReprojectMovingLaunch(const ReprojectMovingJob &J, hipStream_t s);

// stage 1V (k_reproject_var): the moving job and the variance pair; prev_nodes == NULL = camera only (stage 1: nodes, chain, the ids unread)
struct ReprojectVarJob : ReprojectMovingJob {
    const float *prev_variance; // W*H*3, or NULL when no history variance is asked for
    float *history_variance;    // W*H*3, or NULL
};
hipError_t ReprojectVarLaunch(const ReprojectVarJob &J, hipStream_t s);

struct TemporalJob {
    int W, H;
    bhrt_temporal_opts o;
    float cur_samples;
    const float *radiance; // W*H*3
    const float *history;  // W*H*3, or NULL (then no pixel has a history)
    const float *length;   // W*H, or NULL (likewise)
    float *out;            // W*H*3, or NULL
    float *out_length;     // W*H, or NULL
    uint8_t *rgb8;         // W*H*3 bytes, or NULL
};

const char *TemporalArgsError(const bhrt_temporal_opts *o, float cur_samples);
hipError_t TemporalLaunch(const TemporalJob &J, hipStream_t s);

// stage 2V (k_temporal_accumulate_var)
struct TemporalVarJob : TemporalJob {
    const float *variance;         // W*H*3: the current frame's
    const float *history_variance; // W*H*3: stage 1V's; NULL only when history or length is
    float *out_variance;           // W*H*3, or NULL
};
hipError_t TemporalVarLaunch(const TemporalVarJob &J, hipStream_t s);

// stage 3S (k_spatial_variance)
struct SpatialVarianceJob {
    int W, H;
    bhrt_spatial_variance_opts o;
    const float *radiance; // W*H*3
    const float *variance; // W*H*3, or NULL
    const float *length;   // W*H, or NULL (then every pixel is estimated); needs variance
    const float *z;        // W*H
    const float *normal;   // W*H*3
    const float *albedo;   // W*H*3; read only with o.demodulate
    float *out_variance;   // W*H*3; aliases no input
};
// "" when the arguments are usable, else what is wrong with them (host arithmetic only)
const char *SpatialVarianceArgsError(const bhrt_spatial_variance_opts *o, const float *radiance, const float *variance, const float *length, const float *out_variance);
hipError_t SpatialVarianceLaunch(const SpatialVarianceJob &J, hipStream_t s);

// stage 2C (k_temporal_change)
struct TemporalChangeJob {
    int W, H;
    bhrt_change_opts o;
    const float *radiance, *variance;         // W*H*3 each: the current frame and the variance of its mean
    const float *history, *history_variance;  // W*H*3 each: stage 1V's
    const float *length;                      // W*H: stage 1V's
    const float *z;                           // W*H
    const float *normal;                      // W*H*3
    float *out_length;                        // W*H; not `length`
    float *change;                            // W*H, or NULL
};
// "" when the options (the arguments) are usable, else what is wrong with them (host arithmetic only); the session checks the options alone
const char *TemporalChangeOptsError(const bhrt_change_opts *o);
const char *TemporalChangeArgsError(const bhrt_change_opts *o, const float *radiance, const float *variance, const float *history, const float *history_variance,
                                    const float *length, const float *out_length);
hipError_t TemporalChangeLaunch(const TemporalChangeJob &J, hipStream_t s);

// the temporal session's count of the pixels with history (k_history_count): zeroes *count (device) on `s`, then adds the number of
// the n (< 2^32) device lengths that are > 0
hipError_t HistoryCountLaunch(const float *length, size_t n, unsigned long long *count, hipStream_t s);

} // namespace bhrt
