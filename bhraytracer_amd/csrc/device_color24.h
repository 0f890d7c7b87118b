// device_color24.h — the tail of every 8-bit image of the render path: gamma (USE_GamaCorrection, Main.cpp:220-226) and Color24
// (cyColor.h:271-272).  k_resolve, k_resolve_frames, k_fold_frame (kernels.hip) and the denoiser's last iteration (denoise.hip) all call it, so a frame that
// the denoiser leaves alone (K = 0) gets the render's own bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bhrt_detmath.h"
#include "vecmath.h"

namespace bhrt {

// one channel: the channels do not meet (k_resolve_frames holds one channel per lane).
// int(t) is undefined in C++ for NaN and for |t| >= 2^31.  The compiled reference converts with x86's cvttss2si, whose answer for all of
// those is INT_MIN, so NaN, +-inf and any v * 255 + 0.5 from 2^31 up give byte 0 (the GPU's own conversion saturates: +inf would give 255).
// The same rule as k_z_image's (kernels.hip) and the oracle's FloatToByte; in range it truncates toward zero and clamps, as before.
__device__ inline uint8_t color24_channel(float v, int gamma)
{
    if (gamma) v = dm::powf_(v, 1 / 2.2f);
    const float t = v * 255 + 0.5f;
    const int b = t != t ? (int)0x80000000 : (t >= 2147483648.f ? (int)0x80000000 : (t <= -2147483649.f ? (int)0x80000000 : int(t)));
    return (uint8_t)(b < 0 ? 0 : (b > 255 ? 255 : b));
}
__device__ inline void store_color24(uint8_t *rgb8, size_t pix, V3 out, int gamma)
{
    rgb8[pix * 3] = color24_channel(out.x, gamma);
    rgb8[pix * 3 + 1] = color24_channel(out.y, gamma);
    rgb8[pix * 3 + 2] = color24_channel(out.z, gamma);
}

} // namespace bhrt
