// upsample.hip — guided upsampling (bhrt_upsample*): a frame rendered at 1/s of the size, rebuilt at full size along the full-size
// first hit.  A translation unit above the library's public _dev entry points, like temporal_change.hip: full-size guides the caller leaves out
// are bhrt_first_hit_dev's, into scratch the scene owns through a pointer (scene_internal.h).
//
// 4U. GUIDED UPSAMPLING (k_upsample<kVar, kLight>).  All arithmetic is IEEE float32, evaluated left to right as written, IEEE division, no contraction, the
// correctly rounded square root dm::sqrt_f; positions are integers (tests/test_upsample.py restates the stage in numpy with the same order).
//   divisor(a) = dn_divisor of denoise.hip, as in temporal.hip: max(a', 1e-3) per channel, a' = a if max(a.r, a.g, a.b) >= 1e-3, else (1, 1, 1)
//   The scene's frame is W x H; the low frame is w x h, W = s w, H = s h, s an integer in 1..8.  c, v = the low radiance and the variance of its
//   mean (optional); zl, nl, al = the low first hit; z, n, a = the full-size first hit.  Per full pixel p = (x, y):
//   position tx = 2 x + 1 - s,  I0 = floor(tx / 2s) (integers; -1 at the left border),  fx = (float)(tx - 2s I0) / (float)(2s);  ty, J0, fy likewise.
//            (The centre of low pixel I lies at full coordinate s I + (s - 1) / 2: the low pixel's colour sits at its centre.)
//   taps     t = 0..3: (I0, J0), (I0 + 1, J0), (I0, J0 + 1), (I0 + 1, J0 + 1), each index clamped into the low image: (I_t, J_t), q = J_t w + I_t;
//            b_0 = (1 - fx)(1 - fy),  b_1 = fx (1 - fy),  b_2 = (1 - fx) fy,  b_3 = fx fy
//   per low pixel q (once, when it is staged):  with demodulate d_q = divisor(al_q), e_q = c_q / d_q per channel and vv_q = v_q / (d_q d_q), the
//            product first, then one division;  without, e_q = c_q, vv_q = v_q and no albedo is read
//   test     stage 3S's, with the distance from p to the tap's guide pixel (s I_t, s J_t), the full pixel whose un-jittered ray the low guide traced:
//            dx = s I_t - x, dy = s J_t - y (integers), r = max(1, sqrt((float)(dx dx + dy dy)))
//            p a miss (z_p >= BHRT_BIGFLOAT):  the tap passes iff zl_q >= BHRT_BIGFLOAT
//            p a hit:  iff zl_q < BHRT_BIGFLOAT and |zl_q - z_p| <= (depth_tolerance z_p) r
//                      and (n_p.x nl_q.x + n_p.y nl_q.y) + n_p.z nl_q.z >= normal_threshold      (the normals as they are: no unit(); a zero normal
//                      passes only a threshold <= 0, as in 3S)
//            a comparison with a NaN is false: a NaN guide fails the test
//   weights  k_t = b_t where tap t passes, else 0;  S = sum k_t in tap order, from 0;  confidence_p = S
//            S == 0:  k_t = b_t for the taps of the pixel's own kind (kind = z >= BHRT_BIGFLOAT, of zl_q and z_p; a NaN depth is a hit), S again
//            still 0: k_t = b_t for all four taps, S again
//   result   over the taps with k_t > 0, in tap order, per channel, from 0:  m = m + k_t e_q,  u = u + (k_t k_t) vv_q
//            out_p = m / S;  out_variance_p = u / (S S);  with demodulate g = divisor(a_p):  out_p = out_p g,  out_variance_p = out_variance_p (g g)
//            rgb8_p = store_color24(out_p) (device_color24.h: the gamma and Color24 of k_resolve)
//   fallback = BHRT_UPSAMPLE_FALLBACK_LIGHT (opts.fallback; the rule above is BHRT_UPSAMPLE_FALLBACK_ALBEDO, the default).  Position, taps, b_t, the
//            test, k_t, the first S and confidence_p = S are the same, and a pixel whose first S is not 0 is the same in every byte of every
//            output.  A pixel whose first S == 0 chooses its weights as above (its own kind, then all four) and sums the raw low images, in tap
//            order from 0, over the taps with k_t > 0:  m = m + k_t c_q,  u = u + (k_t k_t) v_q;  out_p = m / S;  out_variance_p = u / (S S);
//            NO multiplication by divisor(a_p);  rgb8_p = store_color24(out_p).  A pixel none of whose taps lies on its surface would otherwise
//            get light that was divided by another surface's albedo times its own: a floor of albedo 0.9 under taps on glass of albedo 0.02
//            comes out 45 times too bright.  That light was never divided by an albedo the pixel shares, so it is taken as it
//            was rendered.  With demodulate == 0 e_q = c_q and vv_q = v_q: the two rules are the same arithmetic and the same kernel runs.
//   A tap of weight 0 takes no part: a NaN radiance propagates into exactly the pixels that weigh it.  With s = 1 every tx is even, fx = fy = 0,
//   tap 0 is the pixel itself with b_0 = 1: with the same guides on both sides and demodulate = 0, out = (0 + 1 c) / 1 = c bit for bit for a c
//   that is not -0 (where the pixel fails its own test — a zero normal, a NaN depth — the first fallback gives the same tap).
//   out_variance is the variance of out_p alone, for independent low pixels.  Neighbouring full pixels share taps: their values are correlated,
//   the frame's noise is not independent across pixels, and out_variance says nothing about that (include/bhrt.h).
//
// THE KERNEL.  16 x 16 workgroups of full pixels.  The taps of a workgroup span at most ceil(15 / s) + 2 <= 17 low pixels a side (I0 grows by at
// most ceil(30 / 2s) over 16 pixels, and each pixel reads I0 and I0 + 1), so the workgroup first stages that low tile in LDS, clamped indices
// resolved while staging, as planes e.r, e.g, e.b, z, n.x, n.y, n.z and with a variance vv.r, vv.g, vv.b: the demodulating divisions happen once
// per staged low pixel, not once per tap.  The kind of a tap is one comparison on its staged z; a plane of its own would cost a load to save it.
// Every thread of the workgroup stages, also one outside the image, in two trips of a fixed count.  Rows are 18 words apart: for s >= 2 the 16
// lanes of a row read at most 9 distinct consecutive words (pairs of lanes share one and broadcast), and the next row of the 32-lane half
// starts 18 banks on: no two lanes of a half share a bank; at s = 1 (nothing is upsampled) the 17th word of a row meets the next row's first
// two banks.  The roots of dx dx + dy dy <= 2 * 11^2 (|dx| < 3s / 2) sit in LDS as well, one correctly rounded square root each.  Four taps
// with fixed trip counts, no dynamically indexed array, no atomics, no scratch memory.  kVar removes the variance planes, their loads and the
// store; the other outputs are uniform branches.  kLight (fallback = LIGHT with demodulate) adds one divergent branch for the pixels whose first
// S == 0, about 1 % of a frame: the staged e_q d_q is not c_q bit for bit, so the branch reads its up to four clamped low pixels again from
// global memory (they were read while staging: L2 hits) instead of staging three to six more planes for every workgroup; LDS stays as it is.
// The instantiations without kLight are the kernel as it was.  Per full pixel 16 B read (28 B with albedo) and up to 12 + 12 + 4 + 3 B written; per low pixel
// 28 B (40 B with albedo, 12 B more with a variance), 1 / s^2 of that per full pixel plus the tile's overlap.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "bhrt.h"
#include "bhrt_flat.h"
#include "dev_buf.h"
#include "device_color24.h"
#include "scene_internal.h"

namespace bhrt {

constexpr int kUpTx = 16, kUpTy = 16;       // the workgroup: full pixels
constexpr int kUpTileMax = 17;              // ceil(15 / s) + 2 at s = 1
constexpr int kUpStride = 18;               // words between the rows of a plane
constexpr int kUpPlane = kUpStride * kUpTileMax;
constexpr int kUpRoots = 2 * 11 * 11 + 1;   // |dx|, |dy| <= 11 at s = 8
constexpr int kUpMaxScale = 8;

// the images and constants of one k_upsample call
struct UpsampleJob {
    int W, H, w, h, s;
    float depth_tolerance, normal_threshold;
    int demodulate, gamma;
    const float *c, *v;         // low radiance; its variance, or NULL
    const float *zl, *nl, *al;  // the low first hit; al is read only with demodulate
    const float *z, *n, *a;     // the full-size first hit; a is read only with demodulate
    float *out, *out_variance, *confidence; // each may be NULL
    uint8_t *rgb8;                          // likewise
};

// divisor(a): dn_divisor of denoise.hip
__device__ inline V3 up_divisor(const float *albedo, size_t p)
{
    V3 a = v3(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]);
    const float m = fmaxf(fmaxf(a.x, a.y), a.z);
    if (!(m >= 1e-3f)) a = v3(1, 1, 1);
    return v3(fmaxf(a.x, 1e-3f), fmaxf(a.y, 1e-3f), fmaxf(a.z, 1e-3f));
}

// floor(t / d) for t >= -d, d > 0
__device__ inline int up_floor_div(int t, int d) { return (int)((unsigned)(t + d) / (unsigned)d) - 1; }

// Stage 4U.  Every thread of the workgroup, also one outside the image, takes part in staging the tile.
template <bool kVar, bool kLight>
__global__ void __launch_bounds__(kUpTx *kUpTy) k_upsample(UpsampleJob J)
{
    __shared__ float tile[kVar ? 10 : 7][kUpPlane]; // e.r, e.g, e.b, z, n.x, n.y, n.z, then vv.r, vv.g, vv.b of the low tile
    __shared__ float root[kUpRoots];                // sqrt((float)k), k = dx dx + dy dy
    const int tid = (int)(threadIdx.y * kUpTx + threadIdx.x);
    const int s = J.s, s2 = 2 * s;
    const int x0 = (int)(blockIdx.x * kUpTx), y0 = (int)(blockIdx.y * kUpTy);
    const int li0 = up_floor_div(2 * x0 + 1 - s, s2), lj0 = up_floor_div(2 * y0 + 1 - s, s2); // the tile's first low pixel, before the clamp
    const int tw = (15 + s - 1) / s + 2;                                                       // its side
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int i = tid + k * (kUpTx * kUpTy);
        const int ly = i / kUpStride, lx = i - ly * kUpStride;
        if (lx < tw && ly < tw) {
            const int gi = min(max(li0 + lx, 0), J.w - 1), gj = min(max(lj0 + ly, 0), J.h - 1);
            const size_t q = (size_t)gj * J.w + gi;
            V3 e = v3(J.c[3 * q], J.c[3 * q + 1], J.c[3 * q + 2]);
            V3 vv = v3(0, 0, 0);
            if (kVar) vv = v3(J.v[3 * q], J.v[3 * q + 1], J.v[3 * q + 2]);
            if (J.demodulate) {
                const V3 dq = up_divisor(J.al, q);
                e = v3(e.x / dq.x, e.y / dq.y, e.z / dq.z);
                if (kVar) vv = v3(vv.x / (dq.x * dq.x), vv.y / (dq.y * dq.y), vv.z / (dq.z * dq.z));
            }
            tile[0][i] = e.x; tile[1][i] = e.y; tile[2][i] = e.z;
            tile[3][i] = J.zl[q];
            tile[4][i] = J.nl[3 * q]; tile[5][i] = J.nl[3 * q + 1]; tile[6][i] = J.nl[3 * q + 2];
            if constexpr (kVar) { tile[7][i] = vv.x; tile[8][i] = vv.y; tile[9][i] = vv.z; }
        }
    }
    if (tid < kUpRoots) root[tid] = dm::sqrt_f((float)tid);
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= J.W || y >= J.H) return;
    const size_t p = (size_t)y * J.W + x;
    const int tx = 2 * x + 1 - s, ty = 2 * y + 1 - s;
    const int I0 = up_floor_div(tx, s2), J0 = up_floor_div(ty, s2);
    const float fx = (float)(tx - s2 * I0) / (float)s2, fy = (float)(ty - s2 * J0) / (float)s2;
    const float gx = 1.f - fx, gy = 1.f - fy;
    const float zp = J.z[p];
    const V3 np = v3(J.n[3 * p], J.n[3 * p + 1], J.n[3 * p + 2]);
    const bool miss = zp >= BHRT_BIGFLOAT;
    const float tz = J.depth_tolerance * zp;
    const int base = (J0 - lj0) * kUpStride + (I0 - li0);
    int q[4];
    float b[4], zq[4], k[4];
    bool pass[4];
    float S = 0.f;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int di = t & 1, dj = t >> 1;
        q[t] = base + dj * kUpStride + di;
        b[t] = (di ? fx : gx) * (dj ? fy : gy);
        const int dx = s * min(max(I0 + di, 0), J.w - 1) - x, dy = s * min(max(J0 + dj, 0), J.h - 1) - y;
        const float r = fmaxf(1.f, root[dx * dx + dy * dy]);
        zq[t] = tile[3][q[t]];
        if (miss) pass[t] = zq[t] >= BHRT_BIGFLOAT;
        else
            pass[t] = zq[t] < BHRT_BIGFLOAT && fabsf(zq[t] - zp) <= tz * r &&
                      (np.x * tile[4][q[t]] + np.y * tile[5][q[t]]) + np.z * tile[6][q[t]] >= J.normal_threshold;
        k[t] = pass[t] ? b[t] : 0.f;
        S = S + k[t];
    }
    if (J.confidence) J.confidence[p] = S;
    const bool lost = S == 0.f; // no tap passed: the pixel falls back
    if (lost) { // no tap on the pixel's surface: the taps of its own kind
#pragma unroll
        for (int t = 0; t < 4; t++) {
            k[t] = (zq[t] >= BHRT_BIGFLOAT) == miss ? b[t] : 0.f;
            S = S + k[t];
        }
        if (S == 0.f) { // none of weight: all four
#pragma unroll
            for (int t = 0; t < 4; t++) {
                k[t] = b[t];
                S = S + k[t];
            }
        }
    }
    V3 m = v3(0, 0, 0), u = v3(0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (!(k[t] > 0.f)) continue;
        m = m + v3(tile[0][q[t]], tile[1][q[t]], tile[2][q[t]]) * k[t];
        if constexpr (kVar) u = u + v3(tile[7][q[t]], tile[8][q[t]], tile[9][q[t]]) * (k[t] * k[t]);
    }
    V3 o = m / S, ov = v3(0, 0, 0);
    if (kVar) ov = u / (S * S);
    if (kLight && lost) { // the taps' light as it was rendered, and no albedo of the pixel's own
        m = v3(0, 0, 0);
        u = v3(0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (!(k[t] > 0.f)) continue;
            const int gi = min(max(I0 + (t & 1), 0), J.w - 1), gj = min(max(J0 + (t >> 1), 0), J.h - 1); // as staged: inside the low image
            const size_t g = (size_t)gj * J.w + gi;
            m = m + v3(J.c[3 * g], J.c[3 * g + 1], J.c[3 * g + 2]) * k[t];
            if constexpr (kVar) u = u + v3(J.v[3 * g], J.v[3 * g + 1], J.v[3 * g + 2]) * (k[t] * k[t]);
        }
        o = m / S;
        if (kVar) ov = u / (S * S);
    } else if (J.demodulate) {
        const V3 g = up_divisor(J.a, p);
        o = v3(o.x * g.x, o.y * g.y, o.z * g.z);
        if (kVar) ov = v3(ov.x * (g.x * g.x), ov.y * (g.y * g.y), ov.z * (g.z * g.z));
    }
    if (J.out) { J.out[3 * p] = o.x; J.out[3 * p + 1] = o.y; J.out[3 * p + 2] = o.z; }
    if constexpr (kVar) { J.out_variance[3 * p] = ov.x; J.out_variance[3 * p + 1] = ov.y; J.out_variance[3 * p + 2] = ov.z; }
    if (J.rgb8) store_color24(J.rgb8, p, o, J.gamma);
}

// light: fallback = BHRT_UPSAMPLE_FALLBACK_LIGHT
static hipError_t UpsampleLaunch(const UpsampleJob &J, bool light, hipStream_t st)
{
    const dim3 grid((unsigned)((J.W + kUpTx - 1) / kUpTx), (unsigned)((J.H + kUpTy - 1) / kUpTy)), block(kUpTx, kUpTy);
    if (light && J.demodulate) { // without demodulate the two fallbacks are the same arithmetic: the kernel without kLight serves both
        if (J.out_variance) hipLaunchKernelGGL((k_upsample<true, true>), grid, block, 0, st, J);
        else hipLaunchKernelGGL((k_upsample<false, true>), grid, block, 0, st, J);
    } else if (J.out_variance) hipLaunchKernelGGL((k_upsample<true, false>), grid, block, 0, st, J);
    else hipLaunchKernelGGL((k_upsample<false, false>), grid, block, 0, st, J);
    return hipGetLastError();
}

// z (N floats), normal (3N), albedo (3N) of full-size guides computed here, on the device the scene was uploaded to when they were allocated
struct UpsampleScratch {
    int device = -1;
    DevBuf<float> g;
};

static void DestroyUpsampleScratch(UpsampleScratch *c)
{
    if (!c) return;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    delete c; // hipFree waits for the device
}

// the scene's guide scratch, `floats` floats, on the scene's device (a scene uploaded to another device since gets new memory there)
static int ReserveUpsampleScratch(bhrt_scene *scene, size_t floats, float *&g)
{
    const int dev = SceneDevice(scene);
    if (scene->upsample_scratch && scene->upsample_scratch->device != dev) {
        DestroyUpsampleScratch(scene->upsample_scratch);
        scene->upsample_scratch = nullptr;
        HIP_CHECK(hipSetDevice(dev));
    }
    if (!scene->upsample_scratch) {
        scene->upsample_scratch = new UpsampleScratch;
        scene->upsample_scratch_release = DestroyUpsampleScratch;
        scene->upsample_scratch->device = dev;
    }
    BHRT_TRY(scene->upsample_scratch->g.Reserve(floats));
    g = scene->upsample_scratch->g.p;
    return BHRT_OK;
}

static inline bool UpFinite(float x) { return x >= -3.402823466e38f && x <= 3.402823466e38f; }

// The arguments of both entry points, checked alike and before any device is touched (host arithmetic only); s: the factor
static int UpsampleArgs(const bhrt_scene *scene, const bhrt_upsample_opts *o, int32_t lw, int32_t lh, const float *low_radiance, const float *low_variance,
                        const float *low_z, const float *low_normal, const float *low_albedo, const float *z, const float *normal, const float *albedo,
                        const float *out, const float *out_variance, const float *confidence, const uint8_t *rgb8, int &s)
{
    auto bad = [](const char *what) { SetError(std::string("upsample: ") + what); return BHRT_ERR_ARG; };
    if (!scene) return bad("null scene");
    if (!o) return bad("null options");
    if (!low_radiance || !low_z || !low_normal) return bad("low_radiance, low_z and low_normal are required");
    if (o->demodulate && !low_albedo) return bad("demodulate needs low_albedo");
    const bhrt_flat_header *H = scene->flat.hdr();
    const int W = H->camera.width, Hh = H->camera.height;
    if (lw < 1 || lh < 1) return bad("low_width and low_height must be >= 1");
    s = W / lw;
    if (s < 1 || s > kUpMaxScale || (int64_t)s * lw != W || (int64_t)s * lh != Hh)
        return bad("the scene's size must be s times the low frame's, in both directions, for an integer s in 1..8");
    if ((uint64_t)W * (uint64_t)Hh > 0x7fffffffull) return bad("frame size out of range");
    if (!(o->depth_tolerance >= 0.f) || !UpFinite(o->depth_tolerance)) return bad("depth_tolerance must be finite and >= 0");
    if (o->normal_threshold != o->normal_threshold) return bad("normal_threshold is NaN");
    if (o->fallback != BHRT_UPSAMPLE_FALLBACK_ALBEDO && o->fallback != BHRT_UPSAMPLE_FALLBACK_LIGHT)
        return bad("fallback must be BHRT_UPSAMPLE_FALLBACK_ALBEDO or BHRT_UPSAMPLE_FALLBACK_LIGHT");
    if (!out && !out_variance && !confidence && !rgb8) return bad("no output is asked for");
    if (out_variance && !low_variance) return bad("out_variance needs low_variance");
    // an output may be neither an input nor another output: a pixel's taps are other pixels' inputs
    const size_t n = (size_t)lw * lh, N = (size_t)W * Hh;
    struct Range { const void *p; size_t bytes; };
    const Range in[8] = {{low_radiance, 12 * n}, {low_variance, 12 * n}, {low_z, 4 * n}, {low_normal, 12 * n}, {o->demodulate ? low_albedo : nullptr, 12 * n},
                         {z, 4 * N}, {normal, 12 * N}, {o->demodulate ? albedo : nullptr, 12 * N}};
    const Range outs[4] = {{out, 12 * N}, {out_variance, 12 * N}, {confidence, 4 * N}, {rgb8, 3 * N}};
    auto overlap = [](const Range &a, const Range &b) {
        if (!a.p || !b.p) return false;
        const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
        return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
    };
    for (int i = 0; i < 4; i++) {
        for (int k = 0; k < 8; k++)
            if (overlap(outs[i], in[k])) return bad("an output aliases an input");
        for (int k = i + 1; k < 4; k++)
            if (overlap(outs[i], outs[k])) return bad("two outputs alias");
    }
    return BHRT_OK;
}

} // namespace bhrt

using namespace bhrt;

extern "C" {

int bhrt_upsample_dev(bhrt_scene *scene, const bhrt_upsample_opts *opts, int32_t low_width, int32_t low_height, const float *d_low_radiance,
                      const float *d_low_variance, const float *d_low_z, const float *d_low_normal, const float *d_low_albedo, const float *d_z,
                      const float *d_normal, const float *d_albedo, float *d_out, float *d_out_variance, float *d_confidence, uint8_t *d_rgb8, void *stream)
try {
    int s = 0;
    BHRT_TRY(UpsampleArgs(scene, opts, low_width, low_height, d_low_radiance, d_low_variance, d_low_z, d_low_normal, d_low_albedo, d_z, d_normal, d_albedo, d_out,
                          d_out_variance, d_confidence, d_rgb8, s));
    if (!scene->dev) BHRT_TRY(bhrt_scene_upload(scene, 0));
    HIP_CHECK(hipSetDevice(SceneDevice(scene)));
    const bhrt_flat_header *H = scene->flat.hdr();
    hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)SceneStream(scene);
    UpsampleJob J;
    J.W = H->camera.width; J.H = H->camera.height; J.w = low_width; J.h = low_height; J.s = s;
    J.depth_tolerance = opts->depth_tolerance; J.normal_threshold = opts->normal_threshold;
    J.demodulate = opts->demodulate ? 1 : 0; J.gamma = opts->gamma;
    J.c = d_low_radiance; J.v = d_out_variance ? d_low_variance : nullptr; // a variance nobody asks for is not read
    J.zl = d_low_z; J.nl = d_low_normal; J.al = J.demodulate ? d_low_albedo : nullptr;
    J.z = d_z; J.n = d_normal; J.a = J.demodulate ? d_albedo : nullptr;
    J.out = d_out; J.out_variance = d_out_variance; J.confidence = d_confidence; J.rgb8 = d_rgb8;
    const bool need_a = J.demodulate && !d_albedo;
    if (!d_z || !d_normal || need_a) { // the full-size guides the caller left out, by the kernel of bhrt_first_hit* on the call's stream
        const size_t N = (size_t)J.W * J.H;
        float *g = nullptr;
        BHRT_TRY(ReserveUpsampleScratch(scene, N * (need_a ? 7 : 4), g));
        float *gz = d_z ? nullptr : g, *gn = d_normal ? nullptr : g + N, *ga = need_a ? g + 4 * N : nullptr;
        BHRT_TRY(bhrt_first_hit_dev(scene, gz, gn, ga, st));
        if (gz) J.z = gz;
        if (gn) J.n = gn;
        if (ga) J.a = ga;
    }
    HIP_CHECK(UpsampleLaunch(J, opts->fallback == BHRT_UPSAMPLE_FALLBACK_LIGHT, st));
    if (!stream) HIP_CHECK(hipStreamSynchronize(st));
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

int bhrt_upsample(bhrt_scene *scene, const bhrt_upsample_opts *opts, int32_t low_width, int32_t low_height, const float *low_radiance,
                  const float *low_variance, const float *low_z, const float *low_normal, const float *low_albedo, const float *z, const float *normal,
                  const float *albedo, float *out, float *out_variance, float *confidence, uint8_t *rgb8)
try {
    int s = 0;
    BHRT_TRY(UpsampleArgs(scene, opts, low_width, low_height, low_radiance, low_variance, low_z, low_normal, low_albedo, z, normal, albedo, out, out_variance,
                          confidence, rgb8, s));
    if (!scene->dev) BHRT_TRY(bhrt_scene_upload(scene, 0));
    HIP_CHECK(hipSetDevice(SceneDevice(scene)));
    const bhrt_flat_header *H = scene->flat.hdr();
    const size_t n = (size_t)low_width * low_height, N = (size_t)H->camera.width * H->camera.height;
    hipStream_t st = (hipStream_t)SceneStream(scene);
    // device copies, back to back, in floats: the low radiance, variance, z, normal, albedo (3, 3, 1, 3, 3 per low pixel), the full z, normal, albedo
    // (1, 3, 3 per pixel), then out, out_variance, confidence (3, 3, 1) and the bytes of rgb8 (3 per pixel, rounded up to floats)
    const float *const in[8] = {low_radiance, low_variance, low_z, low_normal, opts->demodulate ? low_albedo : nullptr, z, normal, opts->demodulate ? albedo : nullptr};
    const size_t size[12] = {3 * n, 3 * n, n, 3 * n, 3 * n, N, 3 * N, 3 * N, 3 * N, 3 * N, N, (3 * N + 3) / 4};
    DevBuf<float> d;
    size_t total = 0;
    for (int k = 0; k < 12; k++) total += size[k];
    BHRT_TRY(d.Reserve(total));
    float *at[12];
    for (size_t k = 0, off = 0; k < 12; off += size[k], k++) at[k] = d.p + off;
    for (int k = 0; k < 8; k++)
        if (in[k]) HIP_CHECK(hipMemcpyAsync(at[k], in[k], size[k] * sizeof(float), hipMemcpyHostToDevice, st));
    auto gin = [&](int k) -> float * { return in[k] ? at[k] : nullptr; };
    BHRT_TRY(bhrt_upsample_dev(scene, opts, low_width, low_height, gin(0), gin(1), gin(2), gin(3), gin(4), gin(5), gin(6), gin(7), out ? at[8] : nullptr,
                               out_variance ? at[9] : nullptr, confidence ? at[10] : nullptr, rgb8 ? (uint8_t *)at[11] : nullptr, nullptr));
    if (out) HIP_CHECK(hipMemcpy(out, at[8], 3 * N * sizeof(float), hipMemcpyDeviceToHost));
    if (out_variance) HIP_CHECK(hipMemcpy(out_variance, at[9], 3 * N * sizeof(float), hipMemcpyDeviceToHost));
    if (confidence) HIP_CHECK(hipMemcpy(confidence, at[10], N * sizeof(float), hipMemcpyDeviceToHost));
    if (rgb8) HIP_CHECK(hipMemcpy(rgb8, at[11], 3 * N, hipMemcpyDeviceToHost));
    return BHRT_OK;
} catch (...) { return bhrt::AbiException(); }

} // extern "C"
