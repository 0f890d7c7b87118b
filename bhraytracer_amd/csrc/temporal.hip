// temporal.hip — temporal reprojection: what interactive path tracers do when the camera moves.  For every pixel of the new view,
// find where its surface point was in the previous view, fetch the light gathered there if it is still the same surface (k_reproject), and
// blend the new samples into it (k_temporal_accumulate).  Two image-space stages beside the render path, guided by the first hit of
// k_first_hit (z, normal, albedo) of both views.
//
// THE DEFINITION.  All arithmetic is IEEE float32, evaluated left to right as written, IEEE division, no contraction, the correctly rounded
// square root dm::sqrt_f (tests/test_reproject.py restates both stages in numpy with the same order).
//   dot(a, b)  = (a.x b.x + a.y b.y) + a.z b.z
//   a ^ b      = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
//   unit(n)    = rule B of denoise.hip: l = sqrt((n.x n.x + n.y n.y) + n.z n.z); n / l per component where l > 0, else 0
//   divisor(a) = dn_divisor of denoise.hip: max(a', 1e-3) per channel, a' = a if max(a.r, a.g, a.b) >= 1e-3, else (1, 1, 1)
//
// 1. REPROJECTION, pixel (i, j) of the W x H frame of the current camera C = (pos, top_left, dd_x, dd_y); primed symbols are the previous view's:
//   its frame (pos', top_left', dd_x', dd_y'), first hit z', n', albedo a' (optional), radiance c' and length l' (the samples behind each pixel;
//   without a length image 1 everywhere).  z, n, a: the current view's first hit.
//   miss (z >= BHRT_BIGFLOAT)
//            u = i, v = j: one tap of weight 1, valid when it is a miss too (z' >= BHRT_BIGFLOAT) and l' > 0.  (The reference's background is
//            sampled in screen space, Main.cpp:159-168: a background pixel's history is its own pixel.)
//   hit      d = ((top_left + (float)i dd_x) - (float)j dd_y) - pos            (k_first_hit's expression)
//            x = pos + d * z                                                   (z is a parameter along the un-normalised d: no square root)
//            q = x - pos',  A = top_left' - pos',  m = dd_x' ^ dd_y'
//            t = dot(q, m) / dot(A, m)                                         (the ray parameter the previous view must have stored for x)
//            the pixel is invalid unless t > 0 and t is finite
//            r = q / t - A
//            u = dot(r, dd_x') / dot(dd_x', dd_x'),   v = -(dot(r, dd_y') / dot(dd_y', dd_y'))
//   snap     where |u - rintf(u)| <= 2^-7: u = rintf(u); likewise v.  A design rule: a bilinear weight below 1/128 is dropped, so that a camera
//            that did not move gives the previous frame's bits.
//   bounds   the pixel is invalid unless u >= -1 && u < W && v >= -1 && v < H  (a NaN fails)
//   taps     i0 = floorf(u), fx = u - i0, j0 = floorf(v), fy = v - j0;  taps (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1) in that order with
//            weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy;  a tap of weight 0 is skipped
//            a hit pixel's tap is valid when it lies inside the image, l' > 0, z' < BHRT_BIGFLOAT, |z' - t| <= depth_tolerance * t and
//            dot(unit(n), unit(n')) >= normal_threshold
//   result   sw = the sum of the valid weights, in tap order, from 0; the pixel is invalid unless sw > 0
//            history = (sum w e') / sw * g per channel:  e' = c' / divisor(a'), g = divisor(a) when albedo images take part, else e' = c' and
//            there is no multiplication;  length = (sum w l') / sw;  motion = (u - i, v - j)
//   invalid  history = 0, length = 0, motion = 0
//
// 1M. REPROJECTION THROUGH OBJECT MOTION (k_reproject_moving): stage 1 with these changes for a hit pixel.  k = id (the node of the
//   pixel's first hit, bhrt_first_hit_node), xf_c = (tm, pos, itm) the scene's record of node c now, xf'_c the previous one (prev_xforms);
//   mat_mul(M, p) = (p.x M0 + p.y M3 + p.z M6, p.x M1 + p.y M4 + p.z M7, p.x M2 + p.y M5 + p.z M8), mat_tmul(M, d) = (M0 d.x + M1 d.y + M2 d.z,
//   M3 d.x + M4 d.y + M5 d.z, M6 d.x + M7 d.y + M8 d.z), each sum left to right (vecmath.h).
//   id       k < 0 or k >= n_nodes: the pixel is invalid (nothing is indexed with such a k)
//   moved[k] formed on the host: 1 when the 84 bytes of xf_c and xf'_c differ for c = k or any ancestor of k
//   moved    with the chain c_1 .. c_m of k (the depth-1 ancestor first, k last; m = min(depth, BHRT_MAX_NODE_DEPTH)):
//            p = x;       for a = 1 .. m: p = mat_mul(itm_a, p - pos_a)         (into the node's space with the current records: FillCamChain's expression)
//                         for a = m .. 1: p = mat_mul(tm'_a, p) + pos'_a        (back out with the previous ones)
//            x' = p replaces x in q = x - pos'
//            nl = n;      for a = 1 .. m: nl = mat_tmul(tm_a, nl);  for a = m .. 1: nl = mat_tmul(itm'_a, nl);  no normalisation on the way;
//            unit(nl) replaces unit(n) in the normal test
//   unmoved  x' = x and n is untouched: with nothing moved every output is stage 1's bit for bit
//   taps     with a prev_id image, a hit pixel's tap is valid only if prev_id[tap] == k as well
//   Misses, snap, bounds, taps, result and motion are stage 1's; motion now contains the object's motion.
//
// 1V. REPROJECTION THAT ALSO CARRIES A VARIANCE (k_reproject_var<kAlbedo, kMoving>): everything stage 1 computes (stage 1M when
//   kMoving), in the same operations and order, so history, length and motion are those stages' bits.  In addition, with v' the previous view's
//   variance image (W*H*3, laid out like c': the per-channel variance of each pixel's mean, bhrt_render_var's or stage 2V's):
//   taps     per valid tap, in tap order, per channel, from 0:  sv = sv + w * ve'
//            ve' = v' without albedo images;  with them ve' = v' / (dq * dq), dq = divisor(a'(q)): the product first, then one IEEE division
//            (e' = c' / dq is the carried light, so its variance is v' / dq^2)
//   result   hv = sv / sw;  with albedo images hv = hv * (g * g), g = divisor(a): the product first, then one multiplication
//   invalid  hv = 0
//   The weights are the bilinear w, not w^2: the variance is interpolated linearly, as SVGF interpolates its moments.  A design rule.  With
//   the normalised weights w / sw <= 1, sum (w / sw) v >= sum (w / sw)^2 v: for independent taps the linear interpolation never understates
//   the variance of the interpolated value (it overstates it by up to 4 x at the centre of four taps, where neighbouring pixels then share
//   taps and are no longer independent: the squared weights would understate their common noise).  And it is exact for the single tap of
//   a snapped or static pixel: a camera that did not move carries the previous variance's bits.
//
// 2. ACCUMULATION, per pixel: c = the current radiance, n_c = cur_samples (the samples behind it), h, l = history and length of stage 1.
//   no history (not l > 0):  out = c, out_length = min(n_c, max_length)
//   else, with clamp_k >= 0:  the taps of the 3 x 3 block of the current radiance that lie inside the image, row-major, m of them; per channel
//            mu = (sum c) / m,  sigma = sqrt((sum (c - mu)(c - mu)) / m),  h = min(max(h, mu - clamp_k sigma), mu + clamp_k sigma)
//   then     l = min(l, max_length),  a = n_c / (l + n_c),  out = h + (c - h) * a,  out_length = min(l + n_c, max_length)
//   rgb8 = store_color24(out) (device_color24.h: the gamma and Color24 of k_resolve)
//
// 2V. ACCUMULATION THAT ALSO BLENDS THE VARIANCE (k_temporal_accumulate_var): out, out_length and rgb8 are stage 2's operations
//   exactly.  v = the current frame's variance (bhrt_render_var's), hv = the history's of stage 1V.
//   no history (not l > 0):  out_variance = v
//   else, per channel, with h0 the history before the clamp and h after it (h = h0 with the clamp off):
//            hv = (h != h0) ? fmaxf(hv, v) : hv       a clamped history channel is a value taken from the current frame's neighbourhood: it
//                                                     cannot be trusted more than the current pixel.  A design rule.
//            out_variance = ((1 - a) * (1 - a)) * hv + (a * a) * v      with stage 2's a: out = (1 - a) h + a c, h and c independent
//   With the clamp off and max_length = +inf, two frames of n1 and n2 samples pool to (n1^2 vA + n2^2 vB) / (n1 + n2)^2.
//
// 2C. TEMPORAL CHANGE TEST (k_temporal_change<R>): between stage 1V and stage 2V.  Stage 1 notices that a pixel shows another
//   surface; it does not notice that the same surface is lit differently (a shadow, a reflection or the indirect light of an object that moved).
//   This stage compares history and current frame over a window on the pixel's own surface, in units of the noise both variances predict, and
//   shortens the pixel's history length where the difference is more than noise; stages 2V, 3S and the denoiser then act on the short length
//   untouched.  c, v = the current radiance and the variance of its mean (bhrt_render_var*'s, or stage 3S's at 1 spp); h, hv, l = history,
//   history variance and length of stage 1V; z, n = the current first hit; R = radius (1..4).
//   per pixel q   L(x)  = (0.2126 x.r + 0.7152 x.g) + 0.0722 x.b
//            vL(x) = ((0.2126 * 0.2126) x.r + (0.7152 * 0.7152) x.g) + (0.0722 * 0.0722) x.b        (the denoiser's two expressions)
//            d_q = L(c_q) - L(h_q),   w_q = vL(v_q) + vL(hv_q),   has_q = l_q > 0  (a NaN is false)
//   no history (not l_p > 0):  out_length_p = l_p, the same bits, and change_p = 0
//   window   taps (dx, dy) in {-R..R}^2 row-major (dy outer), q = p + (dx, dy); taps outside the image are skipped; the centre tap is always valid
//            another tap is valid iff has_q and it passes stage 3S's surface test:
//            p a miss (z_p >= BHRT_BIGFLOAT):  z_q >= BHRT_BIGFLOAT
//            p a hit:  z_q < BHRT_BIGFLOAT and |z_q - z_p| <= (depth_tolerance z_p) r, r = sqrt((float)(dx dx + dy dy)),
//                      and (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= normal_threshold      (the normals as they are: no unit())
//            a comparison with a NaN is false: the tap is invalid
//   statistic over the valid taps in tap order, from 0:  s = s + d_q,  sw = sw + w_q;  then
//            x = fabsf(s) / sqrt(sw) where sw > 0;  where sw <= 0:  x = +inf if fabsf(s) > 0, else 0;  where sw is a NaN:  x = 0
//   result   lambda = !(x > sigma_lo) ? 0 : (x >= sigma_hi ? 1 : (x - sigma_lo) / (sigma_hi - sigma_lo))
//            out_length_p = l_p * (1 - lambda),   change_p = lambda
//   For independent taps x is the difference of the window's mean in standard deviations of its noise: |s / k| / sqrt(sw / k^2), and k cancels.
//   A NaN anywhere (a radiance, a variance, a sum) gives lambda = 0: the history is kept.  A design rule: NaN radiance is the business of the
//   render's own replacement rule, not this stage's.  Properties: lambda = 1 gives out_length = 0, so stage 2 treats the pixel as one without
//   history (out = c, out_variance = v).  h == c bit for bit over a window gives s = 0, x = 0 and out_length == l bit for bit (l * 1).  The
//   statistic is conservative where hv is overstated: the w-not-w^2 interpolation of stage 1V overstates it by up to 4 x, and so does the
//   clamp's raise of stage 2V in the frames before.  It is optimistic where neighbouring histories share bilinear taps: their noise is then
//   correlated and sw, which adds the taps' variances as if they were independent, understates the variance of s.  That is why the
//   thresholds sigma_lo and sigma_hi are measured, not derived.
//
// 3S. SPATIAL VARIANCE ESTIMATE (k_spatial_variance<R>): the variance of a frame that has none it can trust — a 1-spp frame, a
//   pixel whose history is short, an imported radiance image — estimated from the pixel's neighbourhood on its own surface, as SVGF does while
//   a history is shorter than four frames.  Divisions and square roots are correctly rounded.  c = the radiance, v = the frame's present
//   variance (optional), l = the samples behind each pixel (optional; needs v), z, n, a = the first hit; R = radius (1..4).
//   pass     with l: where l_p >= min_length, out_p = v_p, the same bits (a NaN l_p fails the comparison: the pixel is estimated)
//   demod    with demodulate: d_q = divisor(a_q), else d_q = (1, 1, 1) and no albedo is read;  e_q = c_q / d_q per channel
//   window   taps (dx, dy) in {-R..R}^2 row-major (dy outer), q = p + (dx, dy); taps outside the image are skipped; the centre tap is always valid
//            p a miss (z_p >= BHRT_BIGFLOAT):  another tap is valid iff z_q >= BHRT_BIGFLOAT
//            p a hit:  another tap is valid iff z_q < BHRT_BIGFLOAT and |z_q - z_p| <= (depth_tolerance z_p) r, r = sqrt((float)(dx dx + dy dy)),
//                      and (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= normal_threshold      (the normals as they are: no unit())
//            a comparison with a NaN is false: the tap is invalid
//   estimate k = the number of valid taps;  per channel, over the valid taps in tap order, from 0:
//            s = s + e_q,  m = s / (float)k;   then  t = t + (e_q - m)(e_q - m),  ve = t / (float)(k - 1);   out_p = ve (d_p d_p)
//   k < 2    out_p = v_p with a variance image, else 0
//   Hard stops as stage 1's, no exp or pow: the restatement is equal bit for bit.  Two passes: a sum of squares is >= 0 by construction and
//   has none of the cancellation of m2 - m1^2.  k - 1: the unbiased sample variance.  Every c_q is already a pixel's mean at the frame's sample
//   count, so the spread of neighbouring means over one surface estimates the variance of a pixel's mean, the quantity bhrt_denoise* and
//   stage 2V take.  It also contains the signal's own gradient over the window (texture left after demodulation, shading, shadow edges), as
//   SVGF's estimate does: it overstates the noise where the image itself varies.
//
// KERNELS.  k_reproject: one lane per pixel of the current camera, 256 in a row; the call's constants (A, m, the three dots) come from the host,
// in the same float32 operations.  It reads 28 B per pixel of the current view (40 B with albedo) and, per tap, 32 B of the previous one (44 B
// with albedo); it writes 24 B.  k_temporal_accumulate: the denoiser's 16 x 16 workgroups; the 3 x 3 block is read through the cache (a wave
// is 16 x 4 pixels: its taps share cache lines; a tile staged through LDS measured no better).  Fixed tap order, no atomics:
// the same inputs give the same bytes.  k_reproject_moving: k_reproject's lane layout and taps (its body is repeated rather than shared, so
// that k_reproject keeps its code); 4 B more per pixel (8 B with prev_id per tap), and for a pixel of a moved node 84 B of the current and
// 88 B of the previous record per chain level, from the scene's nodes and from a scratch buffer of 88 B per node.  The chain loop is bounded
// by BHRT_MAX_NODE_DEPTH; no array is indexed dynamically (no scratch memory).  k_reproject_var: the same lane layout and taps, one body for
// the camera-only and the moving case (it is new: no existing kernel's code depends on it); per tap 12 B more (v'), 12 B more written (hv).
// k_temporal_accumulate_var: k_temporal_accumulate's workgroups and 3 x 3 block; 24 B more read (v, hv), 12 B more written.
// k_spatial_variance<R>: the 16 x 16 workgroups again.  A pixel reads up to 2 (2R + 1)^2 taps, so the workgroup first stages its (16 + 2R)^2
// halo tile in LDS, demodulated once per tile pixel, as seven planes (e.r, e.g, e.b, z, n.x, n.y, n.z): 13.6 KB at R = 3, and a wave's 16 x 4
// lanes read 16 consecutive words of a plane per row, rows 16 + 2R >= 18 words apart: no two lanes of a 32-lane half share a bank.  The r of
// the up to 33 distances dx dx + dy dy sit in LDS as well, one correctly rounded square root each.  Pass 1 keeps each tap's verdict in an 81-bit
// mask in registers; pass 2 reads e alone.  demodulate, "variance given" and "length given" are uniform branches, R a template parameter (fixed
// trip counts, no dynamically indexed array: no scratch memory).  Per pixel 28 B read (40 B with albedo; 12 B and 4 B more with v and l), times
// ((16 + 2R) / 16)^2 for the halo (1.89 at R = 3, from the cache), 12 B written.  Fixed tap order, no atomics.
// k_temporal_change<R>: k_spatial_variance's scheme.  16 x 16 workgroups; the (16 + 2R)^2 halo tile is staged once in LDS as seven planes
// (d, w, z, n.x, n.y, n.z and the has-history verdict as a word), d and w evaluated once per tile pixel, rows 16 + 2R >= 18 words apart as in
// 3S; the correctly rounded roots of dx dx + dy dy in LDS as well.  Every thread of the workgroup stages, also one outside the image.  One pass
// over the window with fixed trip counts (R a template parameter), no dynamically indexed array, no atomics, no scratch memory.  Per pixel
// 68 B read (c, v, h, hv 12 B each, l, z 4 B each, n 12 B), times ((16 + 2R) / 16)^2 for the halo, 4 B written (8 B with the change image).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "bhrt_flat.h"
#include "device_color24.h"
#include "temporal.h"

namespace bhrt {

constexpr int kTaTx = 16, kTaTy = 16;

// divisor(a): dn_divisor of denoise.hip
__device__ inline V3 tp_divisor(const float *albedo, size_t p)
{
    V3 a = v3(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]);
    const float m = fmaxf(fmaxf(a.x, a.y), a.z);
    if (!(m >= 1e-3f)) a = v3(1, 1, 1);
    return v3(fmaxf(a.x, 1e-3f), fmaxf(a.y, 1e-3f), fmaxf(a.z, 1e-3f));
}

// unit(n): rule B of denoise.hip
__device__ inline V3 tp_unit(const float *normal, size_t p)
{
    const V3 n = v3(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]);
    const float l = dm::sqrt_f((n.x * n.x + n.y * n.y) + n.z * n.z);
    return l > 0.f ? v3(n.x / l, n.y / l, n.z / l) : v3(0, 0, 0);
}

// the constants of one call, in the definition's operations (ReprojectConsts, on the host)
struct ReprojectFrame {
    V3 pos, top_left, dd_x, dd_y; // C
    V3 ppos, pdd_x, pdd_y;        // pos', dd_x', dd_y'
    V3 A, m;                      // top_left' - pos', dd_x' ^ dd_y'
    float Am, xx, yy;             // dot(A, m), dot(dd_x', dd_x'), dot(dd_y', dd_y')
};

template <bool kAlbedo>
__global__ void __launch_bounds__(256) k_reproject(int W, int H, ReprojectFrame F, float depth_tolerance, float normal_threshold, const float *__restrict__ pz,
                                                   const float *__restrict__ pn, const float *__restrict__ pc, const float *__restrict__ pl,
                                                   const float *__restrict__ pa, const float *__restrict__ z, const float *__restrict__ n,
                                                   const float *__restrict__ a, float *__restrict__ history, float *__restrict__ length,
                                                   float *__restrict__ motion)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (uint32_t)(W * H)) return;
    const int j = (int)(p / (uint32_t)W), i = (int)(p - (uint32_t)j * (uint32_t)W);
    const float fi = (float)i, fj = (float)j, zp = z[p];
    const bool miss = zp >= BHRT_BIGFLOAT;
    float u = fi, v = fj, t = 0.f;
    bool ok = true;
    V3 nu = v3(0, 0, 0);
    if (!miss) {
        const V3 d = ((F.top_left + fi * F.dd_x) - fj * F.dd_y) - F.pos;
        const V3 x = F.pos + d * zp;
        const V3 q = x - F.ppos;
        t = dot(q, F.m) / F.Am;
        ok = t > 0.f && t <= 3.402823466e38f;
        const V3 r = q / t - F.A;
        u = dot(r, F.pdd_x) / F.xx;
        v = -(dot(r, F.pdd_y) / F.yy);
        const float ru = rintf(u), rv = rintf(v);
        if (fabsf(u - ru) <= 0.0078125f) u = ru;
        if (fabsf(v - rv) <= 0.0078125f) v = rv;
        nu = tp_unit(n, p);
    }
    ok = ok && u >= -1.f && u < (float)W && v >= -1.f && v < (float)H;
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f;
    if (ok) {
        const float f0 = floorf(u), g0 = floorf(v);
        const float fx = u - f0, fy = v - g0, ax = 1.f - fx, ay = 1.f - fy;
        const int i0 = (int)f0, j0 = (int)g0;
        const float w4[4] = {ax * ay, fx * ay, ax * fy, fx * fy};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float w = w4[k];
            const int qi = i0 + (k & 1), qj = j0 + (k >> 1);
            if (w == 0.f || qi < 0 || qi >= W || qj < 0 || qj >= H) continue;
            const size_t q = (size_t)qj * W + qi;
            const float lq = pl ? pl[q] : 1.f, zq = pz[q];
            if (!(lq > 0.f)) continue;
            if (miss) {
                if (!(zq >= BHRT_BIGFLOAT)) continue;
            } else {
                if (!(zq < BHRT_BIGFLOAT) || !(fabsf(zq - t) <= depth_tolerance * t)) continue;
                if (!(dot(nu, tp_unit(pn, q)) >= normal_threshold)) continue;
            }
            sw = sw + w;
            sl = sl + w * lq;
            if (history) {
                V3 e = v3(pc[3 * q], pc[3 * q + 1], pc[3 * q + 2]);
                if (kAlbedo) {
                    const V3 dq = tp_divisor(pa, q);
                    e = v3(e.x / dq.x, e.y / dq.y, e.z / dq.z);
                }
                sr = sr + w * e.x;
                sg = sg + w * e.y;
                sb = sb + w * e.z;
            }
        }
        ok = sw > 0.f;
    }
    V3 h = v3(0, 0, 0);
    float l = 0.f, mu = 0.f, mv = 0.f;
    if (ok) {
        h = v3(sr / sw, sg / sw, sb / sw);
        if (kAlbedo && history) {
            const V3 g = tp_divisor(a, p);
            h = v3(h.x * g.x, h.y * g.y, h.z * g.z);
        }
        l = sl / sw;
        mu = u - fi;
        mv = v - fj;
    }
    if (history) { history[3 * (size_t)p] = h.x; history[3 * (size_t)p + 1] = h.y; history[3 * (size_t)p + 2] = h.z; }
    if (length) length[p] = l;
    if (motion) { motion[2 * (size_t)p] = mu; motion[2 * (size_t)p + 1] = mv; }
}

// the nodes of one k_reproject_moving call (ReprojectMovingJob)
struct MovingNodes {
    const bhrt_node *nodes;
    const int32_t *chain;
    const uint32_t *prev; // kPrevNodeWords per node
    int n_nodes;
};

// Stage 1M.  k_reproject's body with the id check, the chain walk of a moved node and the prev_id test added.
template <bool kAlbedo>
__global__ void __launch_bounds__(256) k_reproject_moving(int W, int H, ReprojectFrame F, float depth_tolerance, float normal_threshold, MovingNodes M,
                                                          const float *__restrict__ pz, const float *__restrict__ pn, const float *__restrict__ pc,
                                                          const float *__restrict__ pl, const float *__restrict__ pa, const int32_t *__restrict__ pid,
                                                          const float *__restrict__ z, const float *__restrict__ n, const float *__restrict__ a,
                                                          const int32_t *__restrict__ id, float *__restrict__ history, float *__restrict__ length,
                                                          float *__restrict__ motion)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (uint32_t)(W * H)) return;
    const int j = (int)(p / (uint32_t)W), i = (int)(p - (uint32_t)j * (uint32_t)W);
    const float fi = (float)i, fj = (float)j, zp = z[p];
    const bool miss = zp >= BHRT_BIGFLOAT;
    float u = fi, v = fj, t = 0.f;
    bool ok = true;
    V3 nu = v3(0, 0, 0);
    int32_t k = -1;
    if (!miss) {
        const V3 d = ((F.top_left + fi * F.dd_x) - fj * F.dd_y) - F.pos;
        V3 x = F.pos + d * zp;
        V3 nl = v3(n[3 * (size_t)p], n[3 * (size_t)p + 1], n[3 * (size_t)p + 2]);
        k = id[p];
        const bool known = (uint32_t)k < (uint32_t)M.n_nodes; // a negative k wraps above every n_nodes
        if (known && M.prev[(size_t)k * kPrevNodeWords + 21] != 0u) {
            const int32_t *c = M.chain + (size_t)k * BHRT_MAX_NODE_DEPTH;
            const int m = min(M.nodes[k].depth, BHRT_MAX_NODE_DEPTH);
            for (int l = 0; l < m; l++) {
                const bhrt_xform &xf = M.nodes[c[l]].xf;
                x = mat_mul(xf.itm, x - v3(xf.pos[0], xf.pos[1], xf.pos[2]));
                nl = mat_tmul(xf.tm, nl);
            }
            for (int l = m - 1; l >= 0; l--) {
                const float *r = (const float *)(M.prev + (size_t)c[l] * kPrevNodeWords);
                x = mat_mul(r, x) + v3(r[9], r[10], r[11]);
                nl = mat_tmul(r + 12, nl);
            }
        }
        const V3 q = x - F.ppos;
        t = dot(q, F.m) / F.Am;
        ok = known && t > 0.f && t <= 3.402823466e38f;
        const V3 r = q / t - F.A;
        u = dot(r, F.pdd_x) / F.xx;
        v = -(dot(r, F.pdd_y) / F.yy);
        const float ru = rintf(u), rv = rintf(v);
        if (fabsf(u - ru) <= 0.0078125f) u = ru;
        if (fabsf(v - rv) <= 0.0078125f) v = rv;
        const float ln = dm::sqrt_f((nl.x * nl.x + nl.y * nl.y) + nl.z * nl.z); // unit(nl)
        nu = ln > 0.f ? v3(nl.x / ln, nl.y / ln, nl.z / ln) : v3(0, 0, 0);
    }
    ok = ok && u >= -1.f && u < (float)W && v >= -1.f && v < (float)H;
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f;
    if (ok) {
        const float f0 = floorf(u), g0 = floorf(v);
        const float fx = u - f0, fy = v - g0, ax = 1.f - fx, ay = 1.f - fy;
        const int i0 = (int)f0, j0 = (int)g0;
        const float w4[4] = {ax * ay, fx * ay, ax * fy, fx * fy};
#pragma unroll
        for (int e4 = 0; e4 < 4; e4++) {
            const float w = w4[e4];
            const int qi = i0 + (e4 & 1), qj = j0 + (e4 >> 1);
            if (w == 0.f || qi < 0 || qi >= W || qj < 0 || qj >= H) continue;
            const size_t q = (size_t)qj * W + qi;
            const float lq = pl ? pl[q] : 1.f, zq = pz[q];
            if (!(lq > 0.f)) continue;
            if (miss) {
                if (!(zq >= BHRT_BIGFLOAT)) continue;
            } else {
                if (!(zq < BHRT_BIGFLOAT) || !(fabsf(zq - t) <= depth_tolerance * t)) continue;
                if (pid && pid[q] != k) continue;
                if (!(dot(nu, tp_unit(pn, q)) >= normal_threshold)) continue;
            }
            sw = sw + w;
            sl = sl + w * lq;
            if (history) {
                V3 e = v3(pc[3 * q], pc[3 * q + 1], pc[3 * q + 2]);
                if (kAlbedo) {
                    const V3 dq = tp_divisor(pa, q);
                    e = v3(e.x / dq.x, e.y / dq.y, e.z / dq.z);
                }
                sr = sr + w * e.x;
                sg = sg + w * e.y;
                sb = sb + w * e.z;
            }
        }
        ok = sw > 0.f;
    }
    V3 h = v3(0, 0, 0);
    float l = 0.f, mu = 0.f, mv = 0.f;
    if (ok) {
        h = v3(sr / sw, sg / sw, sb / sw);
        if (kAlbedo && history) {
            const V3 g = tp_divisor(a, p);
            h = v3(h.x * g.x, h.y * g.y, h.z * g.z);
        }
        l = sl / sw;
        mu = u - fi;
        mv = v - fj;
    }
    if (history) { history[3 * (size_t)p] = h.x; history[3 * (size_t)p + 1] = h.y; history[3 * (size_t)p + 2] = h.z; }
    if (length) length[p] = l;
    if (motion) { motion[2 * (size_t)p] = mu; motion[2 * (size_t)p + 1] = mv; }
}

// the images of one k_reproject_var call (the parameter list of k_reproject_moving plus v' and hv)
struct ReprojectVarImages {
    const float *pz, *pn, *pc, *pv, *pl, *pa; // the previous view: z', n', c', v', l', a'
    const int32_t *pid;                       // id' (kMoving only)
    const float *z, *n, *a;                   // the current view
    const int32_t *id;                        // kMoving only
    float *history, *history_variance, *length, *motion;
};

// Stage 1V.  Stage 1's body (stage 1M's with kMoving), statement for statement, with the variance sums beside the radiance sums.
template <bool kAlbedo, bool kMoving>
__global__ void __launch_bounds__(256) k_reproject_var(int W, int H, ReprojectFrame F, float depth_tolerance, float normal_threshold, MovingNodes M, ReprojectVarImages I)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (uint32_t)(W * H)) return;
    const int j = (int)(p / (uint32_t)W), i = (int)(p - (uint32_t)j * (uint32_t)W);
    const float fi = (float)i, fj = (float)j, zp = I.z[p];
    const bool miss = zp >= BHRT_BIGFLOAT;
    float u = fi, v = fj, t = 0.f;
    bool ok = true;
    V3 nu = v3(0, 0, 0);
    int32_t k = -1;
    if (!miss) {
        const V3 d = ((F.top_left + fi * F.dd_x) - fj * F.dd_y) - F.pos;
        V3 x = F.pos + d * zp;
        V3 nl = v3(I.n[3 * (size_t)p], I.n[3 * (size_t)p + 1], I.n[3 * (size_t)p + 2]);
        bool known = true;
        if (kMoving) {
            k = I.id[p];
            known = (uint32_t)k < (uint32_t)M.n_nodes; // a negative k wraps above every n_nodes
            if (known && M.prev[(size_t)k * kPrevNodeWords + 21] != 0u) {
                const int32_t *c = M.chain + (size_t)k * BHRT_MAX_NODE_DEPTH;
                const int m = min(M.nodes[k].depth, BHRT_MAX_NODE_DEPTH);
                for (int l = 0; l < m; l++) {
                    const bhrt_xform &xf = M.nodes[c[l]].xf;
                    x = mat_mul(xf.itm, x - v3(xf.pos[0], xf.pos[1], xf.pos[2]));
                    nl = mat_tmul(xf.tm, nl);
                }
                for (int l = m - 1; l >= 0; l--) {
                    const float *r = (const float *)(M.prev + (size_t)c[l] * kPrevNodeWords);
                    x = mat_mul(r, x) + v3(r[9], r[10], r[11]);
                    nl = mat_tmul(r + 12, nl);
                }
            }
        }
        const V3 q = x - F.ppos;
        t = dot(q, F.m) / F.Am;
        ok = known && t > 0.f && t <= 3.402823466e38f;
        const V3 r = q / t - F.A;
        u = dot(r, F.pdd_x) / F.xx;
        v = -(dot(r, F.pdd_y) / F.yy);
        const float ru = rintf(u), rv = rintf(v);
        if (fabsf(u - ru) <= 0.0078125f) u = ru;
        if (fabsf(v - rv) <= 0.0078125f) v = rv;
        const float ln = dm::sqrt_f((nl.x * nl.x + nl.y * nl.y) + nl.z * nl.z); // unit(nl)
        nu = ln > 0.f ? v3(nl.x / ln, nl.y / ln, nl.z / ln) : v3(0, 0, 0);
    }
    ok = ok && u >= -1.f && u < (float)W && v >= -1.f && v < (float)H;
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f, vr = 0.f, vg = 0.f, vb = 0.f;
    if (ok) {
        const float f0 = floorf(u), g0 = floorf(v);
        const float fx = u - f0, fy = v - g0, ax = 1.f - fx, ay = 1.f - fy;
        const int i0 = (int)f0, j0 = (int)g0;
        const float w4[4] = {ax * ay, fx * ay, ax * fy, fx * fy};
#pragma unroll
        for (int e4 = 0; e4 < 4; e4++) {
            const float w = w4[e4];
            const int qi = i0 + (e4 & 1), qj = j0 + (e4 >> 1);
            if (w == 0.f || qi < 0 || qi >= W || qj < 0 || qj >= H) continue;
            const size_t q = (size_t)qj * W + qi;
            const float lq = I.pl ? I.pl[q] : 1.f, zq = I.pz[q];
            if (!(lq > 0.f)) continue;
            if (miss) {
                if (!(zq >= BHRT_BIGFLOAT)) continue;
            } else {
                if (!(zq < BHRT_BIGFLOAT) || !(fabsf(zq - t) <= depth_tolerance * t)) continue;
                if (kMoving && I.pid && I.pid[q] != k) continue;
                if (!(dot(nu, tp_unit(I.pn, q)) >= normal_threshold)) continue;
            }
            sw = sw + w;
            sl = sl + w * lq;
            V3 dq = v3(1, 1, 1);
            if (kAlbedo) dq = tp_divisor(I.pa, q);
            if (I.history) {
                V3 e = v3(I.pc[3 * q], I.pc[3 * q + 1], I.pc[3 * q + 2]);
                if (kAlbedo) e = v3(e.x / dq.x, e.y / dq.y, e.z / dq.z);
                sr = sr + w * e.x;
                sg = sg + w * e.y;
                sb = sb + w * e.z;
            }
            if (I.history_variance) {
                V3 e = v3(I.pv[3 * q], I.pv[3 * q + 1], I.pv[3 * q + 2]);
                if (kAlbedo) e = v3(e.x / (dq.x * dq.x), e.y / (dq.y * dq.y), e.z / (dq.z * dq.z));
                vr = vr + w * e.x;
                vg = vg + w * e.y;
                vb = vb + w * e.z;
            }
        }
        ok = sw > 0.f;
    }
    V3 h = v3(0, 0, 0), hv = v3(0, 0, 0);
    float l = 0.f, mu = 0.f, mv = 0.f;
    if (ok) {
        h = v3(sr / sw, sg / sw, sb / sw);
        hv = v3(vr / sw, vg / sw, vb / sw);
        if (kAlbedo) {
            const V3 g = tp_divisor(I.a, p);
            h = v3(h.x * g.x, h.y * g.y, h.z * g.z);
            hv = v3(hv.x * (g.x * g.x), hv.y * (g.y * g.y), hv.z * (g.z * g.z));
        }
        l = sl / sw;
        mu = u - fi;
        mv = v - fj;
    }
    if (I.history) { I.history[3 * (size_t)p] = h.x; I.history[3 * (size_t)p + 1] = h.y; I.history[3 * (size_t)p + 2] = h.z; }
    if (I.history_variance) { I.history_variance[3 * (size_t)p] = hv.x; I.history_variance[3 * (size_t)p + 1] = hv.y; I.history_variance[3 * (size_t)p + 2] = hv.z; }
    if (I.length) I.length[p] = l;
    if (I.motion) { I.motion[2 * (size_t)p] = mu; I.motion[2 * (size_t)p + 1] = mv; }
}

// Stage 2V.  k_temporal_accumulate's body, statement for statement, with the variance blended beside the radiance.
__global__ void __launch_bounds__(kTaTx *kTaTy) k_temporal_accumulate_var(int W, int H, float clamp_k, float max_length, float cur_samples, const float *__restrict__ c,
                                                                          const float *__restrict__ var, const float *__restrict__ history,
                                                                          const float *__restrict__ history_variance, const float *__restrict__ length,
                                                                          float *__restrict__ out, float *__restrict__ out_variance, float *__restrict__ out_length,
                                                                          uint8_t *__restrict__ rgb8, int gamma)
{
    const int x = (int)(blockIdx.x * kTaTx + threadIdx.x), y = (int)(blockIdx.y * kTaTy + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const V3 cp = v3(c[3 * p], c[3 * p + 1], c[3 * p + 2]);
    const V3 vp = v3(var[3 * p], var[3 * p + 1], var[3 * p + 2]);
    const float lp = history && length ? length[p] : 0.f;
    V3 o = cp, ov = vp;
    float ol = fminf(cur_samples, max_length);
    if (lp > 0.f) {
        const V3 h0 = v3(history[3 * p], history[3 * p + 1], history[3 * p + 2]);
        V3 h = h0;
        if (clamp_k >= 0.f) {
            V3 q[9]; // statically indexed: registers
            bool in[9];
            int m = 0;
            V3 s = v3(0, 0, 0);
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const int dy = k / 3 - 1, dx = k % 3 - 1, qy = y + dy, qx = x + dx;
                in[k] = qy >= 0 && qy < H && qx >= 0 && qx < W;
                q[k] = v3(0, 0, 0);
                if (!in[k]) continue;
                const size_t g = ((size_t)qy * W + qx) * 3;
                q[k] = v3(c[g], c[g + 1], c[g + 2]);
                s = s + q[k];
                m++;
            }
            const float fm = (float)m;
            const V3 mu = s / fm;
            V3 s2 = v3(0, 0, 0);
#pragma unroll
            for (int k = 0; k < 9; k++) {
                if (!in[k]) continue;
                const V3 e = q[k] - mu;
                s2 = s2 + e * e;
            }
            const V3 sd = v3(dm::sqrt_f(s2.x / fm), dm::sqrt_f(s2.y / fm), dm::sqrt_f(s2.z / fm));
            const V3 ks = clamp_k * sd;
            h = v3(fminf(fmaxf(h.x, mu.x - ks.x), mu.x + ks.x), fminf(fmaxf(h.y, mu.y - ks.y), mu.y + ks.y), fminf(fmaxf(h.z, mu.z - ks.z), mu.z + ks.z));
        }
        V3 hv = v3(history_variance[3 * p], history_variance[3 * p + 1], history_variance[3 * p + 2]);
        if (h.x != h0.x) hv.x = fmaxf(hv.x, vp.x);
        if (h.y != h0.y) hv.y = fmaxf(hv.y, vp.y);
        if (h.z != h0.z) hv.z = fmaxf(hv.z, vp.z);
        const float l = fminf(lp, max_length);
        const float a = cur_samples / (l + cur_samples);
        o = h + (cp - h) * a;
        const float b = 1.f - a, bb = b * b, aa = a * a;
        ov = v3(bb * hv.x + aa * vp.x, bb * hv.y + aa * vp.y, bb * hv.z + aa * vp.z);
        ol = fminf(l + cur_samples, max_length);
    }
    if (out) { out[3 * p] = o.x; out[3 * p + 1] = o.y; out[3 * p + 2] = o.z; }
    if (out_variance) { out_variance[3 * p] = ov.x; out_variance[3 * p + 1] = ov.y; out_variance[3 * p + 2] = ov.z; }
    if (out_length) out_length[p] = ol;
    if (rgb8) store_color24(rgb8, p, o, gamma);
}

__global__ void __launch_bounds__(kTaTx *kTaTy) k_temporal_accumulate(int W, int H, float clamp_k, float max_length, float cur_samples, const float *__restrict__ c,
                                                                      const float *__restrict__ history, const float *__restrict__ length, float *__restrict__ out,
                                                                      float *__restrict__ out_length, uint8_t *__restrict__ rgb8, int gamma)
{
    const int x = (int)(blockIdx.x * kTaTx + threadIdx.x), y = (int)(blockIdx.y * kTaTy + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const V3 cp = v3(c[3 * p], c[3 * p + 1], c[3 * p + 2]);
    const float lp = history && length ? length[p] : 0.f;
    V3 o = cp;
    float ol = fminf(cur_samples, max_length);
    if (lp > 0.f) {
        V3 h = v3(history[3 * p], history[3 * p + 1], history[3 * p + 2]);
        if (clamp_k >= 0.f) {
            V3 q[9]; // statically indexed: registers
            bool in[9];
            int m = 0;
            V3 s = v3(0, 0, 0);
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const int dy = k / 3 - 1, dx = k % 3 - 1, qy = y + dy, qx = x + dx;
                in[k] = qy >= 0 && qy < H && qx >= 0 && qx < W;
                q[k] = v3(0, 0, 0);
                if (!in[k]) continue;
                const size_t g = ((size_t)qy * W + qx) * 3;
                q[k] = v3(c[g], c[g + 1], c[g + 2]);
                s = s + q[k];
                m++;
            }
            const float fm = (float)m;
            const V3 mu = s / fm;
            V3 s2 = v3(0, 0, 0);
#pragma unroll
            for (int k = 0; k < 9; k++) {
                if (!in[k]) continue;
                const V3 e = q[k] - mu;
                s2 = s2 + e * e;
            }
            const V3 sd = v3(dm::sqrt_f(s2.x / fm), dm::sqrt_f(s2.y / fm), dm::sqrt_f(s2.z / fm));
            const V3 ks = clamp_k * sd;
            h = v3(fminf(fmaxf(h.x, mu.x - ks.x), mu.x + ks.x), fminf(fmaxf(h.y, mu.y - ks.y), mu.y + ks.y), fminf(fmaxf(h.z, mu.z - ks.z), mu.z + ks.z));
        }
        const float l = fminf(lp, max_length);
        const float a = cur_samples / (l + cur_samples);
        o = h + (cp - h) * a;
        ol = fminf(l + cur_samples, max_length);
    }
    if (out) { out[3 * p] = o.x; out[3 * p + 1] = o.y; out[3 * p + 2] = o.z; }
    if (out_length) out_length[p] = ol;
    if (rgb8) store_color24(rgb8, p, o, gamma);
}

// the images of one k_spatial_variance call
struct SpatialVarianceImages {
    const float *c, *v, *l; // radiance; variance and length, or NULL
    const float *z, *n, *a; // the first hit; a is read only with demodulate
    float *out;
};

// Stage 3S.  Every thread of the workgroup, also one outside the image, takes part in staging the tile.
template <int R>
__global__ void __launch_bounds__(kTaTx *kTaTy) k_spatial_variance(int W, int H, float depth_tolerance, float normal_threshold, float min_length, int demodulate,
                                                                   SpatialVarianceImages I)
{
    constexpr int TW = kTaTx + 2 * R, TH = kTaTy + 2 * R, NT = TW * TH, D = 2 * R + 1;
    __shared__ float tile[7][NT];         // e.r, e.g, e.b, z, n.x, n.y, n.z of the halo tile
    __shared__ float root[2 * R * R + 1]; // sqrt((float)k), k = dx dx + dy dy
    const int tid = (int)(threadIdx.y * kTaTx + threadIdx.x);
    const int x0 = (int)(blockIdx.x * kTaTx) - R, y0 = (int)(blockIdx.y * kTaTy) - R;
    for (int i = tid; i < NT; i += kTaTx * kTaTy) {
        const int ly = i / TW, lx = i - ly * TW, gx = x0 + lx, gy = y0 + ly;
        V3 e = v3(0, 0, 0), nq = v3(0, 0, 0);
        float zq = 0.f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) { // a tile pixel outside the image is never read as a tap
            const size_t q = (size_t)gy * W + gx;
            e = v3(I.c[3 * q], I.c[3 * q + 1], I.c[3 * q + 2]);
            if (demodulate) {
                const V3 dq = tp_divisor(I.a, q);
                e = v3(e.x / dq.x, e.y / dq.y, e.z / dq.z);
            }
            zq = I.z[q];
            nq = v3(I.n[3 * q], I.n[3 * q + 1], I.n[3 * q + 2]);
        }
        tile[0][i] = e.x; tile[1][i] = e.y; tile[2][i] = e.z;
        tile[3][i] = zq;
        tile[4][i] = nq.x; tile[5][i] = nq.y; tile[6][i] = nq.z;
    }
    if (tid <= 2 * R * R) root[tid] = dm::sqrt_f((float)tid);
    __syncthreads();
    const int x = x0 + R + (int)threadIdx.x, y = y0 + R + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    V3 vp = v3(0, 0, 0);
    if (I.v) vp = v3(I.v[3 * p], I.v[3 * p + 1], I.v[3 * p + 2]);
    V3 o = vp; // pass-through, and fewer than two valid taps
    const bool keep = I.l && I.l[p] >= min_length;
    if (!keep) {
        const int cp = ((int)threadIdx.y + R) * TW + (int)threadIdx.x + R;
        const float zp = tile[3][cp];
        const V3 np = v3(tile[4][cp], tile[5][cp], tile[6][cp]);
        const bool miss = zp >= BHRT_BIGFLOAT;
        const float tz = depth_tolerance * zp;
        uint64_t lo = 0, hi = 0; // the verdict of tap (dy + R) D + (dx + R): bits 0..63 and 64..80
        int k = 0;
        V3 s = v3(0, 0, 0);
        for (int dy = -R; dy <= R; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int dx = -R; dx <= R; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const int q = cp + dy * TW + dx;
                bool ok = true;
                if (dx != 0 || dy != 0) {
                    const float zq = tile[3][q];
                    if (miss) ok = zq >= BHRT_BIGFLOAT;
                    else
                        ok = zq < BHRT_BIGFLOAT && fabsf(zq - zp) <= tz * root[dx * dx + dy * dy] &&
                             (np.x * tile[4][q] + np.y * tile[5][q]) + np.z * tile[6][q] >= normal_threshold;
                }
                if (!ok) continue;
                const int bit = (dy + R) * D + (dx + R);
                if (bit < 64) lo |= 1ull << bit;
                else hi |= 1ull << (bit - 64);
                k++;
                s = s + v3(tile[0][q], tile[1][q], tile[2][q]);
            }
        }
        if (k >= 2) {
            const V3 m = s / (float)k;
            V3 t = v3(0, 0, 0);
            for (int dy = -R; dy <= R; dy++) {
#pragma unroll
                for (int dx = -R; dx <= R; dx++) {
                    const int bit = (dy + R) * D + (dx + R);
                    if (!(((bit < 64 ? lo >> bit : hi >> (bit - 64)) & 1ull))) continue;
                    const int q = cp + dy * TW + dx;
                    const V3 e = v3(tile[0][q], tile[1][q], tile[2][q]) - m;
                    t = t + e * e;
                }
            }
            o = t / (float)(k - 1);
            if (demodulate) {
                const V3 d = tp_divisor(I.a, p);
                o = v3(o.x * (d.x * d.x), o.y * (d.y * d.y), o.z * (d.z * d.z));
            }
        }
    }
    I.out[3 * p] = o.x; I.out[3 * p + 1] = o.y; I.out[3 * p + 2] = o.z;
}

// the images of one k_temporal_change call
struct TemporalChangeImages {
    const float *c, *v, *h, *hv, *l; // the current frame and its variance; history, its variance and its length
    const float *z, *n;              // the current first hit
    float *out_length, *change;      // change may be NULL
};

__device__ inline float tc_lum(const float *x, size_t q) { return (0.2126f * x[3 * q] + 0.7152f * x[3 * q + 1]) + 0.0722f * x[3 * q + 2]; }
__device__ inline float tc_vlum(const float *x, size_t q)
{
    return ((0.2126f * 0.2126f) * x[3 * q] + (0.7152f * 0.7152f) * x[3 * q + 1]) + (0.0722f * 0.0722f) * x[3 * q + 2];
}

// Stage 2C.  Every thread of the workgroup, also one outside the image, takes part in staging the tile.
template <int R>
__global__ void __launch_bounds__(kTaTx *kTaTy) k_temporal_change(int W, int H, float sigma_lo, float sigma_hi, float depth_tolerance, float normal_threshold,
                                                                  TemporalChangeImages I)
{
    constexpr int TW = kTaTx + 2 * R, TH = kTaTy + 2 * R, NT = TW * TH;
    __shared__ float tile[6][NT];         // d, w, z, n.x, n.y, n.z of the halo tile
    __shared__ uint32_t has[NT];          // 1: the tile pixel has history (l > 0)
    __shared__ float root[2 * R * R + 1]; // sqrt((float)k), k = dx dx + dy dy
    const int tid = (int)(threadIdx.y * kTaTx + threadIdx.x);
    const int x0 = (int)(blockIdx.x * kTaTx) - R, y0 = (int)(blockIdx.y * kTaTy) - R;
    for (int i = tid; i < NT; i += kTaTx * kTaTy) {
        const int ly = i / TW, lx = i - ly * TW, gx = x0 + lx, gy = y0 + ly;
        float dq = 0.f, wq = 0.f, zq = 0.f;
        V3 nq = v3(0, 0, 0);
        uint32_t hq = 0u;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) { // a tile pixel outside the image is never read as a tap
            const size_t q = (size_t)gy * W + gx;
            dq = tc_lum(I.c, q) - tc_lum(I.h, q);
            wq = tc_vlum(I.v, q) + tc_vlum(I.hv, q);
            hq = I.l[q] > 0.f ? 1u : 0u;
            zq = I.z[q];
            nq = v3(I.n[3 * q], I.n[3 * q + 1], I.n[3 * q + 2]);
        }
        tile[0][i] = dq; tile[1][i] = wq;
        tile[2][i] = zq;
        tile[3][i] = nq.x; tile[4][i] = nq.y; tile[5][i] = nq.z;
        has[i] = hq;
    }
    if (tid <= 2 * R * R) root[tid] = dm::sqrt_f((float)tid);
    __syncthreads();
    const int x = x0 + R + (int)threadIdx.x, y = y0 + R + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float lp = I.l[p];
    float ol = lp, lambda = 0.f; // no history: the length's own bits
    if (lp > 0.f) {
        const int cp = ((int)threadIdx.y + R) * TW + (int)threadIdx.x + R;
        const float zp = tile[2][cp];
        const V3 np = v3(tile[3][cp], tile[4][cp], tile[5][cp]);
        const bool miss = zp >= BHRT_BIGFLOAT;
        const float tz = depth_tolerance * zp;
        float s = 0.f, sw = 0.f;
        for (int dy = -R; dy <= R; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int dx = -R; dx <= R; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const int q = cp + dy * TW + dx;
                bool ok = true;
                if (dx != 0 || dy != 0) {
                    const float zq = tile[2][q];
                    ok = has[q] != 0u;
                    if (miss) ok = ok && zq >= BHRT_BIGFLOAT;
                    else
                        ok = ok && zq < BHRT_BIGFLOAT && fabsf(zq - zp) <= tz * root[dx * dx + dy * dy] &&
                             (np.x * tile[3][q] + np.y * tile[4][q]) + np.z * tile[5][q] >= normal_threshold;
                }
                if (!ok) continue;
                s = s + tile[0][q];
                sw = sw + tile[1][q];
            }
        }
        const float as = fabsf(s);
        float xs = 0.f; // a NaN sw
        if (sw > 0.f) xs = as / dm::sqrt_f(sw);
        else if (sw <= 0.f && as > 0.f) xs = __builtin_huge_valf();
        lambda = !(xs > sigma_lo) ? 0.f : (xs >= sigma_hi ? 1.f : (xs - sigma_lo) / (sigma_hi - sigma_lo));
        ol = lp * (1.f - lambda);
    }
    I.out_length[p] = ol;
    if (I.change) I.change[p] = lambda;
}

// The pixels with history (bhrt_temporal_status): how many of the n lengths are > 0 (a NaN is not).  Every wave counts its 64
// lanes with one ballot and one popcount per round of the grid-stride loop, the workgroup's four wave sums meet in LDS, and one 64-bit
// integer atomicAdd per workgroup reaches *count, which the caller has zeroed on the same stream.  Integer and order-free: exact.
constexpr int kHcBlock = 256, kHcMaxBlocks = 2048;
__global__ void __launch_bounds__(kHcBlock) k_history_count(const float *__restrict__ length, uint32_t n, unsigned long long *count)
{
    __shared__ uint32_t s_wave[kHcBlock / 64];
    uint32_t mine = 0; // the same in every lane of a wave
    for (uint64_t base = (uint64_t)blockIdx.x * kHcBlock; base < n; base += (uint64_t)gridDim.x * kHcBlock) { // uniform: every lane takes part in the ballot
        const uint64_t q = base + threadIdx.x;
        const bool has = q < n && length[q] > 0.f;
        mine += (uint32_t)__popcll(__ballot(has));
    }
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < kHcBlock / 64; w++) sum += s_wave[w];
        if (sum) atomicAdd(count, (unsigned long long)sum);
    }
}

hipError_t HistoryCountLaunch(const float *length, size_t n, unsigned long long *count, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(count, 0, sizeof *count, s);
    if (e != hipSuccess || n == 0) return e;
    const size_t blocks = (n + kHcBlock - 1) / kHcBlock;
    hipLaunchKernelGGL(k_history_count, dim3((unsigned)(blocks < (size_t)kHcMaxBlocks ? blocks : (size_t)kHcMaxBlocks)), dim3(kHcBlock), 0, s, length, (uint32_t)n, count);
    return hipGetLastError();
}

static inline bool Finite(float x) { return x >= -3.402823466e38f && x <= 3.402823466e38f; }
static inline V3 H3(const float *p) { return v3(p[0], p[1], p[2]); }

static ReprojectFrame ReprojectConsts(const float *cur, const float *prev)
{
    ReprojectFrame F;
    F.pos = H3(cur); F.top_left = H3(cur + 3); F.dd_x = H3(cur + 6); F.dd_y = H3(cur + 9);
    F.ppos = H3(prev); F.pdd_x = H3(prev + 6); F.pdd_y = H3(prev + 9);
    F.A = H3(prev + 3) - F.ppos;
    F.m = cross(F.pdd_x, F.pdd_y);
    F.Am = dot(F.A, F.m);
    F.xx = dot(F.pdd_x, F.pdd_x);
    F.yy = dot(F.pdd_y, F.pdd_y);
    return F;
}

const char *ReprojectArgsError(const bhrt_reproject_opts *o, const float *prev_frame, const float *prev_radiance, const float *prev_albedo)
{
    if (!o) return "reproject: null options";
    if (!prev_frame) return "reproject: null previous camera frame";
    for (int k = 0; k < 12; k++)
        if (!Finite(prev_frame[k])) return "reproject: the previous camera frame must be finite";
    if (!(o->depth_tolerance >= 0.f) || !Finite(o->depth_tolerance)) return "reproject: depth_tolerance must be finite and >= 0";
    if (o->normal_threshold != o->normal_threshold) return "reproject: normal_threshold is not a number";
    const float zero[12] = {0};
    if (ReprojectConsts(zero, prev_frame).Am == 0.f) return "reproject: the previous camera frame is degenerate (its image plane holds its eye)";
    if (prev_albedo && !prev_radiance) return "reproject: a previous albedo without a previous radiance";
    return "";
}

hipError_t ReprojectLaunch(const ReprojectJob &J, hipStream_t s)
{
    if (!J.history && !J.length && !J.motion) return hipSuccess;
    const uint32_t n_px = (uint32_t)((size_t)J.W * J.H);
    const ReprojectFrame F = ReprojectConsts(J.cur, J.prev);
    const bool alb = J.prev_albedo && J.history;
    hipLaunchKernelGGL(alb ? k_reproject<true> : k_reproject<false>, dim3((n_px + 255) / 256), dim3(256), 0, s, J.W, J.H, F, J.o.depth_tolerance, J.o.normal_threshold,
                       J.prev_z, J.prev_normal, J.prev_radiance, J.prev_length, J.prev_albedo, J.z, J.normal, J.albedo, J.history, J.length, J.motion);
    return hipGetLastError();
}

const char *ReprojectMovingArgsError(const bhrt_xform *prev_xforms, uint32_t n_nodes)
{
    if (!prev_xforms) return "reproject moving: null previous node transforms";
    auto finite = [](const float *f, int n) { for (int e = 0; e < n; e++) if (!Finite(f[e])) return false; return true; };
    for (uint32_t k = 0; k < n_nodes; k++) {
        const bhrt_xform &x = prev_xforms[k];
        if (!finite(x.tm, 9) || !finite(x.pos, 3) || !finite(x.itm, 9)) return "reproject moving: the previous node transforms must be finite";
    }
    return "";
}

void FillPrevNodes(const bhrt_node *nodes, const bhrt_xform *prev_xforms, uint32_t n_nodes, uint32_t *out)
{
    static_assert(sizeof(bhrt_xform) == 84 && kPrevNodeWords * 4 == 88, "a previous record and its flag");
    static_assert(offsetof(bhrt_xform, tm) == 0 && offsetof(bhrt_xform, pos) == 36 && offsetof(bhrt_xform, itm) == 48, "the kernel reads tm', pos', itm' at words 0, 9, 12");
    for (uint32_t k = 0; k < n_nodes; k++) { // pre-order: a parent comes before its children
        uint32_t *o = out + (size_t)k * kPrevNodeWords;
        memcpy(o, &prev_xforms[k], sizeof(bhrt_xform));
        const int32_t parent = nodes[k].parent;
        const bool up = parent >= 0 && (uint32_t)parent < k && out[(size_t)parent * kPrevNodeWords + 21] != 0u;
        o[21] = up || memcmp(&prev_xforms[k], &nodes[k].xf, sizeof(bhrt_xform)) != 0 ? 1u : 0u;
    }
}

hipError_t ReprojectMovingLaunch(const ReprojectMovingJob &J, hipStream_t s)
{
    if (!J.history && !J.length && !J.motion) return hipSuccess;
    const uint32_t n_px = (uint32_t)((size_t)J.W * J.H);
    const ReprojectFrame F = ReprojectConsts(J.cur, J.prev);
    const bool alb = J.prev_albedo && J.history;
    const MovingNodes M = {J.nodes, J.chain, J.prev_nodes, J.n_nodes};
    hipLaunchKernelGGL(alb ? k_reproject_moving<true> : k_reproject_moving<false>, dim3((n_px + 255) / 256), dim3(256), 0, s, J.W, J.H, F, J.o.depth_tolerance,
                       J.o.normal_threshold, M, J.prev_z, J.prev_normal, J.prev_radiance, J.prev_length, J.prev_albedo, J.prev_id, J.z, J.normal, J.albedo, J.id, J.history,
                       J.length, J.motion);
    return hipGetLastError();
}

hipError_t ReprojectVarLaunch(const ReprojectVarJob &J, hipStream_t s)
{
    if (!J.history && !J.history_variance && !J.length && !J.motion) return hipSuccess;
    const uint32_t n_px = (uint32_t)((size_t)J.W * J.H);
    const ReprojectFrame F = ReprojectConsts(J.cur, J.prev);
    const bool alb = J.prev_albedo && (J.history || J.history_variance);
    const bool moving = J.prev_nodes != nullptr;
    const MovingNodes M = {J.nodes, J.chain, J.prev_nodes, J.n_nodes};
    const ReprojectVarImages I = {J.prev_z, J.prev_normal, J.prev_radiance, J.prev_variance, J.prev_length, J.prev_albedo, J.prev_id, J.z, J.normal, J.albedo, J.id,
                                  J.history, J.history_variance, J.length, J.motion};
    auto kernel = moving ? (alb ? k_reproject_var<true, true> : k_reproject_var<false, true>) : (alb ? k_reproject_var<true, false> : k_reproject_var<false, false>);
    hipLaunchKernelGGL(kernel, dim3((n_px + 255) / 256), dim3(256), 0, s, J.W, J.H, F, J.o.depth_tolerance, J.o.normal_threshold, M, I);
    return hipGetLastError();
}

const char *TemporalArgsError(const bhrt_temporal_opts *o, float cur_samples)
{
    if (!o) return "temporal accumulate: null options";
    if (!(cur_samples > 0.f)) return "temporal accumulate: cur_samples must be > 0";
    if (!(o->max_length > 0.f)) return "temporal accumulate: max_length must be > 0";
    return "";
}

hipError_t TemporalLaunch(const TemporalJob &J, hipStream_t s)
{
    if (!J.out && !J.out_length && !J.rgb8) return hipSuccess;
    const dim3 grid((unsigned)((J.W + kTaTx - 1) / kTaTx), (unsigned)((J.H + kTaTy - 1) / kTaTy)), block(kTaTx, kTaTy);
    hipLaunchKernelGGL(k_temporal_accumulate, grid, block, 0, s, J.W, J.H, J.o.clamp_k, J.o.max_length, J.cur_samples, J.radiance, J.history, J.length,
                       J.out, J.out_length, J.rgb8, J.o.gamma ? 1 : 0);
    return hipGetLastError();
}

hipError_t TemporalVarLaunch(const TemporalVarJob &J, hipStream_t s)
{
    if (!J.out && !J.out_variance && !J.out_length && !J.rgb8) return hipSuccess;
    const dim3 grid((unsigned)((J.W + kTaTx - 1) / kTaTx), (unsigned)((J.H + kTaTy - 1) / kTaTy)), block(kTaTx, kTaTy);
    hipLaunchKernelGGL(k_temporal_accumulate_var, grid, block, 0, s, J.W, J.H, J.o.clamp_k, J.o.max_length, J.cur_samples, J.radiance, J.variance, J.history,
                       J.history_variance, J.length, J.out, J.out_variance, J.out_length, J.rgb8, J.o.gamma ? 1 : 0);
    return hipGetLastError();
}

const char *SpatialVarianceArgsError(const bhrt_spatial_variance_opts *o, const float *radiance, const float *variance, const float *length, const float *out_variance)
{
    if (!o) return "spatial variance: null options";
    if (!radiance || !out_variance) return "spatial variance: null radiance or out_variance";
    if (o->radius < 1 || o->radius > 4) return "spatial variance: radius must be in 1..4";
    if (!(o->depth_tolerance >= 0.f) || !Finite(o->depth_tolerance)) return "spatial variance: depth_tolerance must be finite and >= 0";
    if (o->normal_threshold != o->normal_threshold) return "spatial variance: normal_threshold is not a number";
    if (o->min_length != o->min_length) return "spatial variance: min_length is not a number";
    if (length && !variance) return "spatial variance: a length image needs the variance it lets through";
    return "";
}

hipError_t SpatialVarianceLaunch(const SpatialVarianceJob &J, hipStream_t s)
{
    const dim3 grid((unsigned)((J.W + kTaTx - 1) / kTaTx), (unsigned)((J.H + kTaTy - 1) / kTaTy)), block(kTaTx, kTaTy);
    const SpatialVarianceImages I = {J.radiance, J.variance, J.length, J.z, J.normal, J.albedo, J.out_variance};
    auto kernel = J.o.radius == 1 ? k_spatial_variance<1> : J.o.radius == 2 ? k_spatial_variance<2> : J.o.radius == 3 ? k_spatial_variance<3> : k_spatial_variance<4>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, J.W, J.H, J.o.depth_tolerance, J.o.normal_threshold, J.o.min_length, J.o.demodulate ? 1 : 0, I);
    return hipGetLastError();
}

const char *TemporalChangeOptsError(const bhrt_change_opts *o)
{
    if (!o) return "temporal change: null options";
    if (o->radius < 1 || o->radius > 4) return "temporal change: radius must be in 1..4";
    if (!(o->sigma_lo >= 0.f) || !Finite(o->sigma_lo)) return "temporal change: sigma_lo must be finite and >= 0";
    if (!(o->sigma_hi >= o->sigma_lo) || !Finite(o->sigma_hi)) return "temporal change: sigma_hi must be finite and >= sigma_lo";
    if (!(o->depth_tolerance >= 0.f) || !Finite(o->depth_tolerance)) return "temporal change: depth_tolerance must be finite and >= 0";
    if (o->normal_threshold != o->normal_threshold) return "temporal change: normal_threshold is not a number";
    return "";
}

const char *TemporalChangeArgsError(const bhrt_change_opts *o, const float *radiance, const float *variance, const float *history, const float *history_variance,
                                    const float *length, const float *out_length)
{
    const char *bad = TemporalChangeOptsError(o);
    if (*bad) return bad;
    if (!radiance || !variance || !history || !history_variance || !length || !out_length) return "temporal change: null radiance, variance, history, history_variance, length or out_length";
    if (out_length == length) return "temporal change: out_length must not be the length image (a pixel's taps read their neighbours' lengths)";
    return "";
}

hipError_t TemporalChangeLaunch(const TemporalChangeJob &J, hipStream_t s)
{
    const dim3 grid((unsigned)((J.W + kTaTx - 1) / kTaTx), (unsigned)((J.H + kTaTy - 1) / kTaTy)), block(kTaTx, kTaTy);
    const TemporalChangeImages I = {J.radiance, J.variance, J.history, J.history_variance, J.length, J.z, J.normal, J.out_length, J.change};
    auto kernel = J.o.radius == 1 ? k_temporal_change<1> : J.o.radius == 2 ? k_temporal_change<2> : J.o.radius == 3 ? k_temporal_change<3> : k_temporal_change<4>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, J.W, J.H, J.o.sigma_lo, J.o.sigma_hi, J.o.depth_tolerance, J.o.normal_threshold, I);
    return hipGetLastError();
}

} // namespace bhrt
