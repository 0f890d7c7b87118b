// denoise.h — launcher of the edge-avoiding a-trous filter of denoise.hip (bhrt_denoise*, kernels.hip owns the scene state).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "bhrt.h"

namespace bhrt {

struct DenoiseJob {
    int W, H;
    bhrt_denoise_opts o;
    const float *radiance; // W*H*3, linear
    const float *variance; // W*H*3 per-channel variance of the mean, or NULL
    const float *z;        // W*H first-hit ray parameter, BHRT_BIGFLOAT on a miss
    const float *normal;   // W*H*3, zero on a miss
    const float *albedo;   // W*H*3, zero on a miss
    float *out;            // W*H*3 linear, or NULL
    uint8_t *rgb8;         // W*H*3 bytes, or NULL
    float4 *planes;        // scratch: 3 * W*H float4 (two ping-pong planes of (e.rgb, v_L), one of (n.xyz, z))
};

// bytes of DenoiseJob::planes for a W x H frame
inline size_t DenoisePlaneBytes(int W, int H) { return (size_t)W * (size_t)H * 3 * sizeof(float4); }
// "" when the options are usable, else what is wrong with them
const char *DenoiseOptsError(const bhrt_denoise_opts &o);
// enqueues the whole filter on `s`; returns the launch status
hipError_t DenoiseLaunch(const DenoiseJob &J, hipStream_t s);

// The filter for sampled guides (bhrt_denoise_sampled*): J's z, normal and albedo are bhrt_guides' images and `coverage` (W*H) its coverage
// image; all four are read when J.o.iterations > 0.  The planes are DenoiseJob::planes as above: the coverage is read in place.
// "" when sigma_coverage is usable (finite, >= 0), else what is wrong with it
const char *DenoiseSigmaCoverageError(float sigma_coverage);
hipError_t DenoiseSampledLaunch(const DenoiseJob &J, const float *coverage, float sigma_coverage, hipStream_t s);

} // namespace bhrt
