// device_color24.h — the tail of every 8-bit image of the render path: gamma (USE_GamaCorrection, Main.cpp:220-226) and Color24
// (cyColor.h:271-272).  k_resolve (kernels.hip) and the denoiser's last iteration (denoise.hip) both call it, so a frame that
// the denoiser leaves alone (K = 0) gets the render's own bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bhrt_detmath.h"
#include "vecmath.h"

namespace bhrt {

__device__ inline void store_color24(uint8_t *rgb8, size_t pix, V3 out, int gamma)
{
    if (gamma) {
        const float inv = 1 / 2.2f;
        out = v3(dm::powf_(out.x, inv), dm::powf_(out.y, inv), dm::powf_(out.z, inv));
    }
    int r = int(out.x * 255 + 0.5f), g = int(out.y * 255 + 0.5f), b = int(out.z * 255 + 0.5f);
    rgb8[pix * 3] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    rgb8[pix * 3 + 1] = (uint8_t)(g < 0 ? 0 : (g > 255 ? 255 : g));
    rgb8[pix * 3 + 2] = (uint8_t)(b < 0 ? 0 : (b > 255 ? 255 : b));
}

} // namespace bhrt
