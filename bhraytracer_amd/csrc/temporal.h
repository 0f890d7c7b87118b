// temporal.h — launchers of the two image-space stages of temporal.hip (bhrt_reproject*, bhrt_temporal_accumulate*; kernels.hip owns the
// scene state and the first-hit kernel that fills in the guides a caller leaves out).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "bhrt.h"

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

} // namespace bhrt
