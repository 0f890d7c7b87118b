// denoise.hip — the DenoiseImage step of the reference's 64-bit build (Main.cpp:57-96, applied to every frame at Main.cpp:236-238) as
// an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with the variance-guided luminance term of SVGF's spatial filter
// (Schied et al. 2017), guided by the first hit of k_first_hit (z, normal, albedo).  OIDN itself (a neural network shipped as a binary)
// is not reproduced; this is the capability, not its bits.
//
// THE FILTER.  All arithmetic is IEEE float32, evaluated left to right as written, no contraction (tests/test_denoise.py restates it in
// numpy with the same tap and sum order).  Per pixel p of a W x H frame:
//   inputs   c = radiance (linear, before gamma); v = per-channel variance of the mean (optional); z, n, a = first-hit ray parameter,
//            normal, albedo (a miss: z >= BHRT_BIGFLOAT, n = 0, a = 0)
//   demodulation
//            a' = a if max(a.r, a.g, a.b) >= 1e-3, else (1, 1, 1)        (misses, black diffuse, non-Blinn materials)
//            d  = max(a', 1e-3) per channel
//            e  = c / d;   v_e = v / (d * d)                               (per channel)
//            L(x) = (0.2126 x.r + 0.7152 x.g) + 0.0722 x.b
//            v_L = ((0.2126 * 0.2126) v_e.r + (0.7152 * 0.7152) v_e.g) + (0.0722 * 0.0722) v_e.b     (0 without a variance image)
//   iterations k = 0 .. K-1, step s = 2^k, taps (dx, dy) in {-2..2}^2 row-major (dy outer), tap q = p + s (dx, dy); taps outside the
//   image are skipped.  h[-2..2] = (1/16, 1/4, 3/8, 1/4, 1/16).
//            centre tap (0, 0): w = h[0] h[0] = 9/64 (every guide weight of a pixel with itself is 1)
//            other taps:        w = (((h[dx] h[dy]) w_n) w_z) w_l
//            w_n = 1 if n_p = n_q = 0;  0 if exactly one of them is 0;  else pow(max(0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z), sigma_n)
//            w_z = 1 if both are misses;  0 if exactly one is;  else exp(-|z_p - z_q| / ((sigma_z z_p) (s r) + 1e-6)), r = sqrt(dx^2 + dy^2)
//                  (z is a ray parameter along un-normalised camera directions: the relative form keeps the weight scale-free)
//            w_l = exp(-|L(e_p) - L(e_q)| / (sigma_l sqrt(g_p) + 1e-4)) with a variance image, else 1; g_p = the 3x3 binomial blur of
//                  the current v_L: taps (dx, dy) in {-1..1}^2 row-major with weight b[dx] b[dy], b[-1..1] = (1/4, 1/2, 1/4), skipped taps
//                  renormalised: g_p = (sum b b v_L,q) / (sum b b)
//            e_p <- (sum w e_q) / (sum w)   per channel;   v_L,p <- (sum (w w) v_L,q) / ((sum w) (sum w))   with a variance image
//            (sums over the taps in tap order, starting from 0)
//   output   out = e d (per channel, the divisor of the demodulation: a channel the albedo has no share of keeps its light);
//            rgb8 = store_color24(out) (device_color24.h: the gamma and Color24 of k_resolve)
//            K = 0: out = c exactly, rgb8 = store_color24(c) = the render's own bytes.
//
// KERNELS.  k_dn_prepare demodulates and packs two float4 planes, (e.rgb, v_L) and (n.xyz, z): a tap is two 16-byte loads.  One
// k_dn_step per iteration on 16 x 16 pixel workgroups (a wave = 16 x 4 pixels: its taps share cache lines), ping-ponging between two
// (e, v_L) planes; the last one remodulates and writes out / rgb8 instead of a plane.  Fixed tap order, no atomics: the same inputs give
// the same bytes.  Bytes per pixel and iteration: 32 read + 16 written (the taps' re-reads hit L2 / MALL); DESIGN.md 9 has the times.
//
// THE FILTER FOR SAMPLED GUIDES (bhrt_denoise_sampled*).  z, n, a are bhrt_guides' images, averaged over the camera samples of a
// pixel, and cov = its coverage image, W x H floats in [0, 1]: a partly covered pixel carries n and a scaled by its coverage and a colour that
// holds (1 - cov) x background.  The filter is THE FILTER above with three changes; everything not named here (float32, left to right, no
// contraction, the taps, h, the tap order, the miss rule, w_z, w_l, the variance carry, K = 0) is as written there.
//   A. demodulation
//            t   = 1 - cov
//            a_c = a + t                                                    (per channel)
//            a'  = a_c if max(a_c.r, a_c.g, a_c.b) >= 1e-3, else (1, 1, 1)
//            d   = max(a', 1e-3) per channel;  e = c / d, v_e = v / (d * d) and out = e d use this d
//            (c ~ sum_hits kd_s L_s / n + (1 - cov) B, and a + (1 - cov) is that sum with L_s = B = 1: e is a weighted mean of the
//            irradiances and the background)
//   B. normal weight on the direction
//            l  = sqrt((n.x n.x + n.y n.y) + n.z n.z);   nh = n / l per component where l > 0, else 0        (once per pixel)
//            w_n and its zero-normal rule are those above with nh in the place of n
//   C. coverage as a feature
//            w_c = exp(-|cov_p - cov_q| / (sigma_c + 1e-6))
//            other taps:  w = ((((h[dx] h[dy]) w_n) w_z) w_l) w_c;   the centre tap stays 9/64
// With cov = 1 on hits and 0 on misses and unit normals (one un-jittered pinhole sample) A is the divisor above exactly (a + 0 on a hit,
// 0 + 1 = (1, 1, 1) = a' on a miss), w_c = 1 wherever w_z != 0, and nh = n up to the rounding of l: THE FILTER to rounding.
//
// ITS KERNELS.  k_dns_prepare applies A and B and packs the same two planes, (e.rgb, v_L) and (nh.xyz, z), with IEEE divisions: the planes
// are the definition's bits.  k_dns_step reads the caller's coverage image (no plane of its own: the scratch stays 48 B per pixel): a tap is
// two 16-byte loads and one 4-byte load, a level reads 36 B and writes 16 B per pixel (the last one reads 12 B more of albedo and writes
// 15 B instead).  DESIGN.md 9 found a level of k_dn_step bound by one powf, two expf and two IEEE divisions per tap; this definition is new
// text, so its step evaluates the tap's guide weights as ONE exponential on the hardware log2 / exp2:
//            w = (h[dx] h[dy]) exp2(((x_n + x_z) + x_l) + x_c)
//            x_n = sigma_n log2(max(0, nh_p . nh_q))   (0 when sigma_n = 0: pow(x, 0) = 1 also at x = 0; the zero-normal rule gives 0 or -inf)
//            x_z = |z_p - z_q| k_z[r],   k_z[r] = -log2(e) rcp((sigma_z z_p) (s r) + 1e-6) for the five r of a level, once per pixel
//                  (the miss rule gives 0 or -inf)
//            x_l = |L(e_p) - L(e_q)| k_l,   k_l = -log2(e) / (sigma_l sqrt(g_p) + 1e-4), once per pixel (0 without a variance image)
//            x_c = |cov_p - cov_q| k_c,     k_c = -log2(e) / (sigma_c + 1e-6), once per call on the host
// and the sums are divided by one reciprocal of sum w per pixel.  That is the definition to rounding, not to the bit: the tests hold it to
// the numpy restatement (np.power, np.exp, the product of the four weights) within the bound they hold k_dn_step to.  Same 16 x 16
// workgroups, fixed tap order, no atomics: the same inputs give the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>

#include "bhrt_flat.h"
#include "denoise.h"
#include "device_color24.h"

namespace bhrt {

constexpr int kDnTx = 16, kDnTy = 16;

__device__ inline float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// d = max(a', 1e-3) of the demodulation
__device__ inline V3 dn_divisor(const float *albedo, size_t p)
{
    V3 a = v3(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]);
    const float m = fmaxf(fmaxf(a.x, a.y), a.z);
    if (!(m >= 1e-3f)) a = v3(1, 1, 1);
    return v3(fmaxf(a.x, 1e-3f), fmaxf(a.y, 1e-3f), fmaxf(a.z, 1e-3f));
}

template <bool kVar>
__global__ void __launch_bounds__(256) k_dn_prepare(uint32_t n_px, const float *c, const float *v, const float *z, const float *n, const float *albedo,
                                                    float4 *A, float4 *G)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_px) return;
    const V3 d = dn_divisor(albedo, p);
    const size_t k = 3 * (size_t)p;
    float vl = 0.f;
    if (kVar) {
        const float er = v[k] / (d.x * d.x), eg = v[k + 1] / (d.y * d.y), eb = v[k + 2] / (d.z * d.z);
        vl = ((0.2126f * 0.2126f) * er + (0.7152f * 0.7152f) * eg) + (0.0722f * 0.0722f) * eb;
    }
    A[p] = make_float4(c[k] / d.x, c[k + 1] / d.y, c[k + 2] / d.z, vl);
    G[p] = make_float4(n[k], n[k + 1], n[k + 2], z[p]);
}

__device__ inline float dn_h(int k) { return k == 0 ? 0.375f : (k == 1 || k == -1 ? 0.25f : 0.0625f); }
__device__ inline float dn_b(int k) { return k == 0 ? 0.5f : 0.25f; }

template <bool kVar, bool kLast>
__global__ void __launch_bounds__(kDnTx *kDnTy) k_dn_step(int W, int H, int s, float sigma_n, float sigma_z, float sigma_l, const float4 *__restrict__ Ain,
                                                          const float4 *__restrict__ G, float4 *__restrict__ Aout, const float *__restrict__ albedo,
                                                          float *__restrict__ out, uint8_t *__restrict__ rgb8, int gamma)
{
    const int x = (int)(blockIdx.x * kDnTx + threadIdx.x), y = (int)(blockIdx.y * kDnTy + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 ap = Ain[p], gp = G[p];
    const bool p_zero = gp.x == 0.f && gp.y == 0.f && gp.z == 0.f, p_miss = gp.w >= BHRT_BIGFLOAT;
    const float lp = dn_lum(ap.x, ap.y, ap.z);
    float den_l = 1.f;
    if (kVar) {
        float gs = 0.f, gw = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const float w = dn_b(dx) * dn_b(dy);
                gs = gs + w * Ain[(size_t)qy * W + qx].w;
                gw = gw + w;
            }
        }
        den_l = sigma_l * sqrtf(gs / gw) + 1e-4f;
    }
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * W + qx;
            const float4 aq = Ain[q];
            float w;
            if (dx == 0 && dy == 0) {
                w = 0.375f * 0.375f;
            } else {
                const float4 gq = G[q];
                const bool q_zero = gq.x == 0.f && gq.y == 0.f && gq.z == 0.f, q_miss = gq.w >= BHRT_BIGFLOAT;
                float wn, wz, wl = 1.f;
                if (p_zero || q_zero) wn = p_zero == q_zero ? 1.f : 0.f;
                else wn = powf(fmaxf(0.f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z), sigma_n);
                if (p_miss || q_miss) wz = p_miss == q_miss ? 1.f : 0.f;
                else {
                    const float r = (float)s * sqrtf((float)(dx * dx + dy * dy));
                    wz = expf(-fabsf(gp.w - gq.w) / ((sigma_z * gp.w) * r + 1e-6f));
                }
                if (kVar) wl = expf(-fabsf(lp - dn_lum(aq.x, aq.y, aq.z)) / den_l);
                w = ((dn_h(dx) * dn_h(dy)) * wn) * wz * wl;
            }
            sw = sw + w;
            sr = sr + w * aq.x;
            sg = sg + w * aq.y;
            sb = sb + w * aq.z;
            if (kVar) sv = sv + (w * w) * aq.w;
        }
    }
    const float er = sr / sw, eg = sg / sw, eb = sb / sw;
    if (kLast) {
        const V3 d = dn_divisor(albedo, p);
        const V3 o = v3(er * d.x, eg * d.y, eb * d.z);
        if (out) { out[3 * p] = o.x; out[3 * p + 1] = o.y; out[3 * p + 2] = o.z; }
        if (rgb8) store_color24(rgb8, p, o, gamma);
    } else {
        Aout[p] = make_float4(er, eg, eb, kVar ? sv / (sw * sw) : 0.f);
    }
}

// K = 0: the filter is the identity
__global__ void __launch_bounds__(256) k_dn_identity(uint32_t n_px, const float *c, int gamma, float *out, uint8_t *rgb8)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_px) return;
    const V3 o = v3(c[3 * (size_t)p], c[3 * (size_t)p + 1], c[3 * (size_t)p + 2]);
    if (out) { out[3 * (size_t)p] = o.x; out[3 * (size_t)p + 1] = o.y; out[3 * (size_t)p + 2] = o.z; }
    if (rgb8) store_color24(rgb8, p, o, gamma);
}

// ---- the filter for sampled guides -------------------------------------------------------------------------------------------------
// d = max(a', 1e-3) of demodulation A: the albedo plus the background's share
__device__ inline V3 dns_divisor(const float *albedo, const float *cov, size_t p)
{
    const float t = 1.f - cov[p];
    V3 a = v3(albedo[3 * p] + t, albedo[3 * p + 1] + t, albedo[3 * p + 2] + t);
    const float m = fmaxf(fmaxf(a.x, a.y), a.z);
    if (!(m >= 1e-3f)) a = v3(1, 1, 1);
    return v3(fmaxf(a.x, 1e-3f), fmaxf(a.y, 1e-3f), fmaxf(a.z, 1e-3f));
}

template <bool kVar>
__global__ void __launch_bounds__(256) k_dns_prepare(uint32_t n_px, const float *c, const float *v, const float *z, const float *n, const float *albedo,
                                                     const float *cov, float4 *A, float4 *G)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_px) return;
    const V3 d = dns_divisor(albedo, cov, p);
    const size_t k = 3 * (size_t)p;
    float vl = 0.f;
    if (kVar) {
        const float er = v[k] / (d.x * d.x), eg = v[k + 1] / (d.y * d.y), eb = v[k + 2] / (d.z * d.z);
        vl = ((0.2126f * 0.2126f) * er + (0.7152f * 0.7152f) * eg) + (0.0722f * 0.0722f) * eb;
    }
    A[p] = make_float4(c[k] / d.x, c[k + 1] / d.y, c[k + 2] / d.z, vl);
    const float nx = n[k], ny = n[k + 1], nz = n[k + 2];
    const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
    G[p] = l > 0.f ? make_float4(nx / l, ny / l, nz / l, z[p]) : make_float4(0.f, 0.f, 0.f, z[p]);
}

constexpr float kLog2e = 1.44269504088896340736f;
// index of r^2 = dx^2 + dy^2 in {1, 2, 4, 5, 8} among the five distances of a level's taps
__device__ constexpr int dns_ridx(int r2) { return r2 == 1 ? 0 : r2 == 2 ? 1 : r2 == 4 ? 2 : r2 == 5 ? 3 : 4; }

// kc = -log2(e) / (sigma_c + 1e-6); sn0: sigma_n == 0
template <bool kVar, bool kLast>
__global__ void __launch_bounds__(kDnTx *kDnTy) k_dns_step(int W, int H, int s, float sigma_n, int sn0, float sigma_z, float sigma_l, float kc,
                                                           const float4 *__restrict__ Ain, const float4 *__restrict__ G, const float *__restrict__ cov,
                                                           float4 *__restrict__ Aout, const float *__restrict__ albedo, float *__restrict__ out,
                                                           uint8_t *__restrict__ rgb8, int gamma)
{
    const int x = (int)(blockIdx.x * kDnTx + threadIdx.x), y = (int)(blockIdx.y * kDnTy + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 ap = Ain[p], gp = G[p];
    const float cp = cov[p];
    const bool p_zero = gp.x == 0.f && gp.y == 0.f && gp.z == 0.f, p_miss = gp.w >= BHRT_BIGFLOAT;
    const float lp = dn_lum(ap.x, ap.y, ap.z);
    float kl = 0.f;
    if (kVar) {
        float gs = 0.f, gw = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const float w = dn_b(dx) * dn_b(dy);
                gs = gs + w * Ain[(size_t)qy * W + qx].w;
                gw = gw + w;
            }
        }
        kl = -kLog2e / (sigma_l * sqrtf(gs / gw) + 1e-4f);
    }
    float kz[5];
    {
        const float zs = sigma_z * gp.w, fs = (float)s;
        const float r[5] = {1.f, 1.41421356237309504880f, 2.f, 2.23606797749978969641f, 2.82842712474619009760f}; // sqrtf of 1, 2, 4, 5, 8
#pragma unroll
        for (int k = 0; k < 5; k++) kz[k] = -kLog2e * __builtin_amdgcn_rcpf(zs * (fs * r[k]) + 1e-6f);
    }
    const float ninf = -__builtin_huge_valf();
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * W + qx;
            const float4 aq = Ain[q];
            float w;
            if (dx == 0 && dy == 0) {
                w = 0.375f * 0.375f;
            } else {
                const float4 gq = G[q];
                const float cq = cov[q];
                const bool q_zero = gq.x == 0.f && gq.y == 0.f && gq.z == 0.f, q_miss = gq.w >= BHRT_BIGFLOAT;
                float xn, xz;
                if (p_zero || q_zero) xn = p_zero == q_zero ? 0.f : ninf;
                else if (sn0) xn = 0.f;
                else xn = sigma_n * __builtin_amdgcn_logf(fmaxf(0.f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z));
                if (p_miss || q_miss) xz = p_miss == q_miss ? 0.f : ninf;
                else xz = fabsf(gp.w - gq.w) * kz[dns_ridx(dx * dx + dy * dy)];
                float e = xn + xz;
                if (kVar) e = e + fabsf(lp - dn_lum(aq.x, aq.y, aq.z)) * kl;
                e = e + fabsf(cp - cq) * kc;
                w = (dn_h(dx) * dn_h(dy)) * __builtin_amdgcn_exp2f(e);
            }
            sw = sw + w;
            sr = sr + w * aq.x;
            sg = sg + w * aq.y;
            sb = sb + w * aq.z;
            if (kVar) sv = sv + (w * w) * aq.w;
        }
    }
    const float inv = 1.f / sw;
    const float er = sr * inv, eg = sg * inv, eb = sb * inv;
    if (kLast) {
        const V3 d = dns_divisor(albedo, cov, p);
        const V3 o = v3(er * d.x, eg * d.y, eb * d.z);
        if (out) { out[3 * p] = o.x; out[3 * p + 1] = o.y; out[3 * p + 2] = o.z; }
        if (rgb8) store_color24(rgb8, p, o, gamma);
    } else {
        Aout[p] = make_float4(er, eg, eb, kVar ? sv * (inv * inv) : 0.f);
    }
}

const char *DenoiseOptsError(const bhrt_denoise_opts &o)
{
    if (o.iterations < 0 || o.iterations > 16) return "denoise: iterations must be in 0..16";
    if (!(o.sigma_normal >= 0.f && o.sigma_normal < 1e30f) || !(o.sigma_depth >= 0.f && o.sigma_depth < 1e30f) ||
        !(o.sigma_luminance >= 0.f && o.sigma_luminance < 1e30f))
        return "denoise: sigmas must be finite and >= 0";
    return "";
}

template <bool kVar>
static void LaunchSteps(const DenoiseJob &J, hipStream_t s)
{
    const uint32_t n_px = (uint32_t)((size_t)J.W * J.H);
    const size_t px = n_px;
    float4 *A[2] = {J.planes, J.planes + px}, *G = J.planes + 2 * px;
    hipLaunchKernelGGL(k_dn_prepare<kVar>, dim3((n_px + 255) / 256), dim3(256), 0, s, n_px, J.radiance, J.variance, J.z, J.normal, J.albedo, A[0], G);
    const dim3 grid((unsigned)((J.W + kDnTx - 1) / kDnTx), (unsigned)((J.H + kDnTy - 1) / kDnTy)), block(kDnTx, kDnTy);
    const int K = J.o.iterations;
    for (int k = 0; k < K; k++) {
        const float4 *in = A[k & 1];
        float4 *nxt = A[(k + 1) & 1];
        if (k + 1 < K)
            hipLaunchKernelGGL((k_dn_step<kVar, false>), grid, block, 0, s, J.W, J.H, 1 << k, J.o.sigma_normal, J.o.sigma_depth, J.o.sigma_luminance, in, G, nxt,
                               J.albedo, (float *)nullptr, (uint8_t *)nullptr, 0);
        else
            hipLaunchKernelGGL((k_dn_step<kVar, true>), grid, block, 0, s, J.W, J.H, 1 << k, J.o.sigma_normal, J.o.sigma_depth, J.o.sigma_luminance, in, G,
                               (float4 *)nullptr, J.albedo, J.out, J.rgb8, J.o.gamma ? 1 : 0);
    }
}

hipError_t DenoiseLaunch(const DenoiseJob &J, hipStream_t s)
{
    const uint32_t n_px = (uint32_t)((size_t)J.W * J.H);
    if (!J.out && !J.rgb8) return hipSuccess;
    if (J.o.iterations == 0)
        hipLaunchKernelGGL(k_dn_identity, dim3((n_px + 255) / 256), dim3(256), 0, s, n_px, J.radiance, J.o.gamma ? 1 : 0, J.out, J.rgb8);
    else if (J.variance)
        LaunchSteps<true>(J, s);
    else
        LaunchSteps<false>(J, s);
    return hipGetLastError();
}

const char *DenoiseSigmaCoverageError(float sigma_coverage)
{
    return sigma_coverage >= 0.f && sigma_coverage <= 3.402823466e38f ? "" : "denoise: sigma_coverage must be finite and >= 0";
}

template <bool kVar>
static void LaunchSampledSteps(const DenoiseJob &J, const float *cov, float sigma_coverage, hipStream_t s)
{
    const uint32_t n_px = (uint32_t)((size_t)J.W * J.H);
    const size_t px = n_px;
    float4 *A[2] = {J.planes, J.planes + px}, *G = J.planes + 2 * px;
    hipLaunchKernelGGL(k_dns_prepare<kVar>, dim3((n_px + 255) / 256), dim3(256), 0, s, n_px, J.radiance, J.variance, J.z, J.normal, J.albedo, cov, A[0], G);
    const dim3 grid((unsigned)((J.W + kDnTx - 1) / kDnTx), (unsigned)((J.H + kDnTy - 1) / kDnTy)), block(kDnTx, kDnTy);
    const int K = J.o.iterations, sn0 = J.o.sigma_normal == 0.f ? 1 : 0;
    const float kc = -kLog2e / (sigma_coverage + 1e-6f);
    for (int k = 0; k < K; k++) {
        const float4 *in = A[k & 1];
        float4 *nxt = A[(k + 1) & 1];
        if (k + 1 < K)
            hipLaunchKernelGGL((k_dns_step<kVar, false>), grid, block, 0, s, J.W, J.H, 1 << k, J.o.sigma_normal, sn0, J.o.sigma_depth, J.o.sigma_luminance, kc, in, G,
                               cov, nxt, J.albedo, (float *)nullptr, (uint8_t *)nullptr, 0);
        else
            hipLaunchKernelGGL((k_dns_step<kVar, true>), grid, block, 0, s, J.W, J.H, 1 << k, J.o.sigma_normal, sn0, J.o.sigma_depth, J.o.sigma_luminance, kc, in, G,
                               cov, (float4 *)nullptr, J.albedo, J.out, J.rgb8, J.o.gamma ? 1 : 0);
    }
}

hipError_t DenoiseSampledLaunch(const DenoiseJob &J, const float *coverage, float sigma_coverage, hipStream_t s)
{
    const uint32_t n_px = (uint32_t)((size_t)J.W * J.H);
    if (!J.out && !J.rgb8) return hipSuccess;
    if (J.o.iterations == 0)
        hipLaunchKernelGGL(k_dn_identity, dim3((n_px + 255) / 256), dim3(256), 0, s, n_px, J.radiance, J.o.gamma ? 1 : 0, J.out, J.rgb8);
    else if (J.variance)
        LaunchSampledSteps<true>(J, coverage, sigma_coverage, s);
    else
        LaunchSampledSteps<false>(J, coverage, sigma_coverage, s);
    return hipGetLastError();
}

} // namespace bhrt
