"""The spatial variance estimate: bhrt_variance_spatial gives a frame that has no variance it can trust — a 1-spp frame, a pixel
whose history is short, an imported radiance image — the sample variance of its (demodulated) radiance over the pixel's neighbourhood on its
own surface (csrc/temporal.hip states it as stage 3S).

spatial_variance_ref restates the stage in numpy, float32, in the kernel's tap and sum order, vectorised over pixels: one tap of every pixel at
a time.  A tap that is invalid enters both sums as + 0, which is what skipping it does (a sum that starts at +0 never becomes -0)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, have_gpu, same_bits
from test_denoise import _synthetic_xml, _tap, divisor
from test_reproject import BIG, scene  # noqa: F401
from test_temporal_variance import _rho

f32 = np.float32
NAN, INF = float("nan"), float("inf")


def spatial_variance_ref(c, v=None, l=None, z=None, n=None, a=None, radius=3, depth_tolerance=0.01, normal_threshold=0.99, min_length=4.0, demodulate=1):
    """Stage 3S of csrc/temporal.hip on (H, W[, 3]) arrays; v, l may be None, a is read only with demodulate.  Returns out_variance."""
    c, z, n = (np.asarray(k, f32) for k in (c, z, n))
    H, W = z.shape
    R, tol, thr, ml = int(radius), f32(depth_tolerance), f32(normal_threshold), f32(min_length)
    zero = np.zeros((H, W, 3), f32)
    with np.errstate(all="ignore"):
        d = divisor(np.asarray(a, f32)) if demodulate else np.ones((H, W, 3), f32)
        e = (c / d).astype(f32)
        miss = z >= BIG
        tz = (tol * z).astype(f32)
        k = np.zeros((H, W), np.int32)
        s = zero.copy()
        taps = []
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                eq, inside = _tap(e, dx, dy)
                if dx == 0 and dy == 0:
                    ok = np.ones((H, W), bool)
                else:
                    zq, _ = _tap(z, dx, dy)
                    nq, _ = _tap(n, dx, dy)
                    r = np.sqrt(f32(dx * dx + dy * dy))
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    same = (zq < BIG) & (np.abs(zq - z) <= tz * r) & (dot >= thr)
                    ok = inside & np.where(miss, zq >= BIG, same)
                k = k + ok
                s = s + np.where(ok[..., None], eq, f32(0))
                taps.append((ok, eq))
        m = (s / k.astype(f32)[..., None]).astype(f32)
        t = zero.copy()
        for ok, eq in taps:
            dev = eq - m
            t = t + np.where(ok[..., None], dev * dev, f32(0))
        ve = (t / (k - 1).astype(f32)[..., None]).astype(f32)
        est = (ve * (d * d).astype(f32)).astype(f32) if demodulate else ve            # the product first, then one multiplication
        keep = zero if v is None else np.asarray(v, f32)
        out = np.where((k >= 2)[..., None], est, keep)
        if l is not None:
            out = np.where((np.asarray(l, f32) >= ml)[..., None], keep, out)
    return out.astype(f32)


def flat_guides(H, W, depth=3.0):
    """A fronto-parallel plane: every tap of every window is valid."""
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    return np.full((H, W), depth, f32), n


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("bhrt_variance_spatial", "bhrt_variance_spatial_dev")


def test_symbols_exported_declared_and_wrapped(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in SYMBOLS:
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr), s
    assert hasattr(B.lib(), "bhrt_default_spatial_variance_opts") and "bhrt_default_spatial_variance_opts" in B.EXPORTS
    assert re.search(r"\bvoid bhrt_default_spatial_variance_opts\(", hdr) and "DESIGN.md 22" in hdr
    for w in ("variance_spatial", "variance_spatial_dev"):
        assert callable(getattr(B.Scene, w))
    head = open(os.path.join(ROOT, "bhraytracer_amd", "csrc", "temporal.hip")).read().split("#include")[0]
    assert "3S. SPATIAL VARIANCE ESTIMATE" in head


def test_defaults(B):
    import ctypes as C
    o = B.default_spatial_variance_opts()
    assert (o.radius, o.demodulate) == (3, 1) and o.min_length == 4.0
    assert f32(o.depth_tolerance) == f32(0.01) == f32(B.default_denoise_opts().sigma_depth)
    assert f32(o.normal_threshold) == f32(B.REPROJECT_NORMAL_THRESHOLD)
    assert C.sizeof(B.SpatialVarianceOpts) == 32 and not any(o.reserved)
    assert B.default_spatial_variance_opts(radius=2, demodulate=0).radius == 2


def test_bad_arguments_are_refused_before_the_device(B, scene):
    """Every BHRT_ERR_ARG case (error 3) on a loaded scene that was never uploaded: the checks come before any device is touched."""
    sc = scene("c1_sphere_plane")
    W, H = sc.width, sc.height
    z, n3 = np.ones((H, W), f32), np.ones((H, W, 3), f32)
    ok = B.default_spatial_variance_opts()
    D = B.default_spatial_variance_opts
    cases = [(None, n3, n3, z), (ok, None, n3, z),                                                   # NULL options, NULL radiance
             (D(radius=0), n3, n3, z), (D(radius=5), n3, n3, z), (D(radius=-1), n3, n3, z),
             (D(depth_tolerance=-0.01), n3, n3, z), (D(depth_tolerance=INF), n3, n3, z), (D(depth_tolerance=NAN), n3, n3, z),
             (D(normal_threshold=NAN), n3, n3, z), (D(min_length=NAN), n3, n3, z),
             (ok, n3, None, z)]                                                                      # a length without a variance
    for o, c, v, l in cases:
        with pytest.raises(B.BhrtError, match="bhrt error 3"):
            sc.variance_spatial(o, c, v, l, z, n3, n3)
    with pytest.raises(B.BhrtError, match="bhrt error 3"):                                           # NULL out_variance (the pointers are never read)
        sc.variance_spatial_dev(ok, 4096, d_out_variance=0)
    with pytest.raises(B.BhrtError, match="bhrt error 3"):
        sc.variance_spatial_dev(ok, 0, d_out_variance=4096)
    import ctypes as C
    out = np.zeros((H, W, 3), f32)
    assert B.lib().bhrt_variance_spatial(None, C.byref(ok), n3.ctypes.data_as(C.c_void_p), None, None, None, None, None, out.ctypes.data_as(C.c_void_p)) == 3   # NULL scene
    # what is allowed gets past the checks (without a device: "no device", not error 3)
    allowed = (lambda: sc.variance_spatial(ok, n3), lambda: sc.variance_spatial(ok, n3, n3), lambda: sc.variance_spatial(ok, n3, n3, z, z, n3, n3),
               lambda: sc.variance_spatial(D(radius=1, depth_tolerance=0.0, normal_threshold=-INF, min_length=INF, demodulate=0), n3),
               lambda: sc.variance_spatial(D(radius=4, min_length=-INF), n3, n3, z))
    for call in allowed:
        try:
            call()
        except B.BhrtError as e:
            assert "bhrt error 3" not in str(e) and not have_gpu()


def test_restatement_constant_image_and_pass_through():
    """A constant image gives exactly 0 (the mean of k equal values v is fl(k v) / k = v wherever k v is a float: v = 0.75 has two mantissa
    bits, k <= 81 seven), with and without demodulation by a constant albedo.  Where l >= min_length the output is v's bits, a negative value,
    an infinity and a NaN included; below it, and at a NaN l, the estimate."""
    H, W = 9, 11
    z, n = flat_guides(H, W)
    c = np.full((H, W, 3), 0.75, f32)
    a = np.full((H, W, 3), 0.5, f32)
    for R in (1, 2, 3, 4):
        for dm in (0, 1):
            out = spatial_variance_ref(c, None, None, z, n, a, radius=R, demodulate=dm)
            assert same_bits(out, np.zeros_like(c))
    rng = np.random.RandomState(1)
    v = rng.gamma(2.0, 0.01, (H, W, 3)).astype(f32)
    v[0, 0], v[0, 1], v[0, 2] = -1.0, INF, NAN
    l = np.full((H, W), 4, f32)
    l[3], l[4, :5], l[4, 5:], l[5, 0] = 3.999, NAN, INF, 5
    noisy = rng.uniform(0, 1, (H, W, 3)).astype(f32)
    out = spatial_variance_ref(noisy, v, l, z, n, a)
    est = spatial_variance_ref(noisy, v, None, z, n, a)
    kept = l >= 4
    assert same_bits(out[kept], v[kept]) and kept[0, :3].all() and kept[4, 5:].all()
    assert same_bits(out[~kept], est[~kept]) and not kept[3].any() and not kept[4, :5].any() and (est > 0).all()


def test_restatement_equals_the_sample_variance():
    """R = 1 on a 3 x 3 plane: the centre's window holds all nine values, and the estimate is np.var(ddof = 1) of them.  Rounding: with the
    computed mean m' in the place of the mean m, sum (e - m')^2 = sum (e - m)^2 + 9 (m - m')^2 exactly, so the mean's rounding enters in the
    second order only (below 1e-13 relative here).  What is left: the subtraction (u = 2^-24 on a deviation, 2 u on its square), the square (u),
    eight additions of positive terms (8 u) and the division (u): 12 u relative, plus the float32 rounding of the inputs' own exact values,
    which the float64 side shares.  The corner pixels have 4 taps, the edge pixels 6: the same identity."""
    rng = np.random.RandomState(2)
    z, n = flat_guides(3, 3)
    for trial in range(20):
        c = rng.uniform(0, 2, (3, 3, 3)).astype(f32)
        out = spatial_variance_ref(c, None, None, z, n, None, radius=1, demodulate=0)
        want = np.var(c.astype(np.float64).reshape(9, 3), axis=0, ddof=1)
        assert np.allclose(out[1, 1], want, rtol=12 * 2.0 ** -24, atol=0), (out[1, 1], want)
        assert np.allclose(out[0, 0], np.var(c[:2, :2].astype(np.float64).reshape(4, 3), axis=0, ddof=1), rtol=12 * 2.0 ** -24, atol=0)
        assert np.allclose(out[1, 2], np.var(c[:, 1:].astype(np.float64).reshape(6, 3), axis=0, ddof=1), rtol=12 * 2.0 ** -24, atol=0)
    assert (out >= 0).all()


def test_restatement_keeps_edges_apart():
    """Two half-planes of different depth and brightness: 0 on both sides of the edge (nothing mixes across); with the depth stop opened wide
    the pixels within R of the edge mix and are not 0.  The same for a normal flip at equal depth.  A miss pixel uses miss taps only and a hit
    pixel no miss tap: a constant sky beside a constant surface gives 0 everywhere."""
    H, W = 12, 20
    z, n = flat_guides(H, W)
    c = np.full((H, W, 3), 0.25, f32)
    c[:, W // 2:] = 0.75
    zs = z.copy()
    zs[:, W // 2:] = 7
    for R in (1, 3, 4):
        assert same_bits(spatial_variance_ref(c, None, None, zs, n, None, radius=R, demodulate=0), np.zeros_like(c))
        mixed = spatial_variance_ref(c, None, None, zs, n, None, radius=R, demodulate=0, depth_tolerance=10.0)
        assert (mixed[:, W // 2 - R:W // 2 + R] > 0).all() and not mixed[:, :W // 2 - R].any() and not mixed[:, W // 2 + R:].any()
        ns = n.copy()
        ns[:, W // 2:] = np.float32([0.6, 0, 0.8])                                  # a unit normal 0.8 off the other: below 0.99
        assert same_bits(spatial_variance_ref(c, None, None, z, ns, None, radius=R, demodulate=0), np.zeros_like(c))
        assert spatial_variance_ref(c, None, None, z, ns, None, radius=R, demodulate=0, normal_threshold=0.5).any()
        zm, nm = z.copy(), n.copy()
        zm[:, W // 2:], nm[:, W // 2:] = BIG, 0
        zm[0, W - 1] = INF                                                           # an infinite z is a miss as well
        assert same_bits(spatial_variance_ref(c, None, None, zm, nm, None, radius=R, demodulate=0), np.zeros_like(c))
    # the misses see each other whatever their "depth" and normal: a noisy sky has a variance, and it is the sky's own
    rng = np.random.RandomState(3)
    sky = c.copy()
    sky[:, W // 2:] = rng.uniform(0, 1, (H, W - W // 2, 3)).astype(f32)
    out = spatial_variance_ref(sky, None, None, zm, nm, None, radius=1, demodulate=0)
    assert not out[:, :W // 2].any() and (out[:, W // 2:] > 0).all()
    assert np.allclose(out[5, W - 3], np.var(sky[4:7, W - 4:W - 1].astype(np.float64).reshape(9, 3), axis=0, ddof=1), rtol=12 * 2.0 ** -24, atol=0)


def test_restatement_fewer_than_two_taps_and_nan():
    """A pixel no neighbour shares a surface with (its own depth; a NaN z, which fails every comparison) has k = 1: it gets v_p, 0 without a
    variance image.  Its neighbours do not use it: its radiance of 1000 leaves their variance at 0.  A 1 x 1 frame is such a pixel."""
    H, W = 9, 9
    z, n = flat_guides(H, W)
    c = np.full((H, W, 3), 0.5, f32)
    v = np.full((H, W, 3), 0.125, f32)
    z[2, 2], z[6, 6] = 100.0, NAN
    c[2, 2] = c[6, 6] = 1000.0
    for R in (1, 3):
        out = spatial_variance_ref(c, None, None, z, n, None, radius=R, demodulate=0)
        assert same_bits(out, np.zeros_like(c))
        out = spatial_variance_ref(c, v, None, z, n, None, radius=R, demodulate=0)
        only = np.zeros((H, W), bool)
        only[2, 2] = only[6, 6] = True
        assert same_bits(out[only], v[only]) and not out[~only].any()
    one = spatial_variance_ref(np.ones((1, 1, 3), f32), None, None, np.ones((1, 1), f32), np.ones((1, 1, 3), f32), None, demodulate=0)
    assert same_bits(one, np.zeros((1, 1, 3), f32))
    # a NaN normal component fails the normal test: the pixel is alone as well
    nn = n.copy()
    nn[4, 4, 0] = NAN
    out = spatial_variance_ref(c, v, None, flat_guides(H, W)[0], nn, None, radius=1, demodulate=0)
    assert same_bits(out[4, 4], v[4, 4])


def test_restatement_demodulation_removes_the_texture():
    """c = fl(a K) over a textured albedo (every channel in [0.2, 1): d = a exactly) is constant light on a textured surface.  Demodulated,
    e = fl(c / a) = K (1 + e1)(1 + e2), |e| <= u = 2^-24: within 2 u K (1 + u) of K.  R = 1: the sum of k <= 9 such values carries at most 8 u,
    the division u: |e_q - m| <= (2 + 2 + 8 + 1) u K = 13 u K to first order, and the sample variance is at most 9/8 of the largest squared
    deviation.  u K <= ulp(K), so sqrt(out) / a <= 13 sqrt(9/8) ulp(K) < 14 ulp(K) (the remodulation's two roundings are inside the margin).
    Without demodulation the texture is the variance: orders of magnitude above."""
    rng = np.random.RandomState(4)
    H, W = 13, 17
    z, n = flat_guides(H, W)
    a = rng.uniform(0.2, 1, (H, W, 3)).astype(f32)
    for K in (f32(0.7), f32(1.0), f32(3.3)):
        c = (a * K).astype(f32)
        out = spatial_variance_ref(c, None, None, z, n, a, radius=1, demodulate=1)
        sd_in_ulps = np.sqrt(out.astype(np.float64)) / a / float(np.spacing(K))
        assert (out >= 0).all() and sd_in_ulps.max() < 14, sd_in_ulps.max()
        raw = spatial_variance_ref(c, None, None, z, n, a, radius=1, demodulate=0)
        assert raw.min() > 1e6 * out.max()
    # an albedo below the floor: divisor() replaces it, per channel or as a whole, and the estimate is remodulated by the same divisor
    a[5, 5] = (0.5, 1e-5, 0.5)
    a[7, 7] = 0
    assert same_bits(divisor(a)[5, 5], np.float32([0.5, 1e-3, 0.5])) and same_bits(divisor(a)[7, 7], np.ones(3, f32))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def crafted(rng, W, H):
    """A frame of W x H with depth steps, normal flips and normals near the threshold, misses (1e30 and inf), albedo below 1e-3 in one channel
    and in all, NaN and +-inf in z, and a length image on both sides of 4, equal to it included, with NaN and inf: (c, v, l, z, n, a)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(f32)
    z = (f32(3) + f32(0.01) * xx + f32(0.02) * yy).astype(f32)
    z[:, W // 2:] += f32(2)                                                     # a depth step
    z[yy > f32(0.7) * H] *= f32(1.03)                                           # a step near the tolerance: some taps pass at a distance, none beside
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    n[(xx + yy) > f32(0.6) * (W + H)] = np.float32([0.6, 0, 0.8])               # a normal flip
    n = (n + rng.normal(0, 0.05, (H, W, 3))).astype(f32)                        # raw dots on both sides of 0.99
    u = rng.uniform(size=(H, W))
    miss = (u < 0.08) | ((yy < 3) & (xx > W // 3))
    z[miss] = BIG
    z[miss & (u < 0.02)] = INF
    n[miss] = 0
    z[(u > 0.10) & (u < 0.12)] = NAN
    z[(u > 0.12) & (u < 0.13)] = -INF
    a = rng.uniform(0.2, 1, (H, W, 3)).astype(f32)
    a[(u > 0.2) & (u < 0.25)] = np.float32([0.5, 1e-5, 0.5])
    a[(u > 0.25) & (u < 0.3)] = np.float32([5e-4, 1e-5, 0])
    a[miss] = 0
    c = (np.maximum(a, f32(0.1)) * rng.gamma(4.0, 0.25, (H, W, 3))).astype(f32)
    v = rng.gamma(2.0, 0.01, (H, W, 3)).astype(f32)
    l = rng.randint(0, 9, (H, W)).astype(f32)
    w = rng.uniform(size=(H, W))
    l[w < 0.05], l[(w > 0.05) & (w < 0.1)], l[(w > 0.1) & (w < 0.15)] = NAN, INF, 3.9999998
    return c, v, l, z, n, a


def _mismatch(got, ref):
    return int((~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref)))).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (16, 16), (17, 33), (37, 19)])
def test_kernel_equals_restatement_on_crafted_frames(B, scene, tmp_path, size):
    """k_spatial_variance<R> against spatial_variance_ref bit for bit: a frame of one pixel, one smaller than every window, one workgroup
    exactly, and two with workgroup and halo edges on both axes; every R, with and without demodulation, the variance and the length image."""
    W, H = size
    sc = scene(_synthetic_xml(tmp_path, W, H))
    c, v, l, z, n, a = crafted(np.random.RandomState(10 + W), W, H)
    if W * H > 100:
        assert (z >= BIG).any() and np.isnan(z).any() and (l == 4).any() and np.isnan(l).any()
    for R in (1, 2, 3, 4):
        for dm in (0, 1):
            for vv, ll in ((None, None), (v, None), (v, l)):
                o = B.default_spatial_variance_opts(radius=R, demodulate=dm, depth_tolerance=0.02)
                got = sc.variance_spatial(o, c, vv, ll, z, n, a if dm else None)
                ref = spatial_variance_ref(c, vv, ll, z, n, a, radius=R, demodulate=dm, depth_tolerance=0.02)
                assert same_bits(got, ref), (R, dm, vv is not None, ll is not None, _mismatch(got, ref))
            with pytest.raises(B.BhrtError, match="bhrt error 3"):
                sc.variance_spatial(o, c, None, l, z, n, a)
    if W * H > 100:
        assert (ref > 0).any() and same_bits(ref[l >= 4], v[l >= 4])
    # other thresholds: the depth stop shut (only equal depths pass), the normal stop wide open, min_length at its ends
    for kw in (dict(depth_tolerance=0.0), dict(normal_threshold=-INF), dict(min_length=-INF), dict(min_length=INF), dict(min_length=0.0)):
        got = sc.variance_spatial(B.default_spatial_variance_opts(**kw), c, v, l, z, n, a)
        assert same_bits(got, spatial_variance_ref(c, v, l, z, n, a, **kw)), kw


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3_mesh_small", "c4_textured"])
def test_kernel_equals_restatement_on_renders(B, scene, name):
    """The first-hit images and a 2-spp render of a mesh scene and a textured one: the kernel's bytes are the restatement's, with guides
    passed in and with guides computed here (the same bytes), for the default window and the smallest and largest."""
    sc = scene(name)
    z, n, a = sc.first_hit()
    _, rad, var = sc.render_var(B.default_opts(spp=2, seed=9))
    rng = np.random.RandomState(11)
    l = rng.randint(0, 9, z.shape).astype(f32)
    for R, dm, vv, ll in ((3, 1, None, None), (3, 1, var, l), (3, 0, var, None), (1, 1, None, None), (4, 0, var, l)):
        o = B.default_spatial_variance_opts(radius=R, demodulate=dm)
        ref = spatial_variance_ref(rad, vv, ll, z, n, a, radius=R, demodulate=dm)
        got = sc.variance_spatial(o, rad, vv, ll, z, n, a)
        assert same_bits(got, ref), (R, dm, _mismatch(got, ref))
        assert same_bits(sc.variance_spatial(o, rad, vv, ll), ref)                                   # every guide computed here
        assert same_bits(sc.variance_spatial(o, rad, vv, ll, z, None, a if dm else None), ref)       # only the normal
    assert (ref >= 0).all() and (ref > 0).mean() > 0.5


@pytest.mark.gpu
def test_call_variants_and_shared_scratch(B, scene):
    """bhrt_variance_spatial_dev on a stream gives the host call's bytes, with guides given and computed; a bhrt_denoise call in between, which
    uses the same scratch of the scene, does not disturb a later result."""
    import torch
    sc = scene("c3_mesh_small")
    W, H = sc.width, sc.height
    z, n, a = sc.first_hit()
    _, rad, var = sc.render_var(B.default_opts(spp=2, seed=3))
    l = np.random.RandomState(12).randint(0, 9, z.shape).astype(f32)
    o = B.default_spatial_variance_opts()
    want = sc.variance_spatial(o, rad, var, l, z, n, a)
    assert same_bits(want, spatial_variance_ref(rad, var, l, z, n, a))
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t = {k: up(x) for k, x in (("c", rad), ("v", var), ("l", l), ("z", z), ("n", n), ("a", a))}
    out = torch.full((H, W, 3), -1.0, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    sc.variance_spatial_dev(o, t["c"].data_ptr(), t["v"].data_ptr(), t["l"].data_ptr(), t["z"].data_ptr(), t["n"].data_ptr(), t["a"].data_ptr(), out.data_ptr(),
                            stream=s.cuda_stream)
    s.synchronize()
    assert same_bits(out.cpu().numpy(), want)
    out.fill_(-1.0)
    torch.cuda.synchronize()
    sc.variance_spatial_dev(o, t["c"].data_ptr(), t["v"].data_ptr(), t["l"].data_ptr(), d_out_variance=out.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert same_bits(out.cpu().numpy(), want)
    out.fill_(-1.0)
    sc.variance_spatial_dev(o, t["c"].data_ptr(), t["v"].data_ptr(), t["l"].data_ptr(), d_out_variance=out.data_ptr())                 # no stream: synchronous
    assert same_bits(out.cpu().numpy(), want)
    den = sc.denoise(B.default_denoise_opts(), rad, want)[0]                    # its planes and guides overwrite the scratch
    assert same_bits(sc.variance_spatial(o, rad, var, l), want)
    assert same_bits(sc.denoise(B.default_denoise_opts(), rad, want)[0], den)


@pytest.mark.gpu
def test_it_closes_the_gap_at_one_sample(B, scene):
    """c3_mesh_small, a static camera, 8 frames of 1 spp (seeds s .. s + 7).  Each frame's variance is this stage's estimate of the rendered
    frame, every pixel; the frames are chained through bhrt_reproject_var and bhrt_temporal_accumulate_var with the library's defaults, and the
    result is denoised with this stage's estimate of the accumulated frame (its carried variance and length handed in, library defaults, as the
    host program does).  R = 256 spp with another seed.  The denoised frame is closer to R than the accumulated one.  The MSEs are printed.
    Measured: accumulated 4.070e-4, denoised with the estimate 1.558e-4, with variance = NULL 8.651e-4, with the all-zero variance
    that was the only one to be had at 1 spp 4.065e-4 (a zero variance all but shuts the luminance stop: next to nothing is filtered); with the
    estimate taken for every pixel, no carried variance handed in, 1.653e-4."""
    sc = scene("c3_mesh_small")
    s0 = 200
    ro, to, dn, sv = B.default_reproject_opts(), B.default_temporal_opts(), B.default_denoise_opts(), B.default_spatial_variance_opts()
    fr = sc.camera_frame()
    z, n, a = sc.first_hit()
    acc = accv = ln = None
    for k in range(8):
        rad = sc.render(B.default_opts(spp=1, seed=s0 + k))[1]
        var = sc.variance_spatial(sv, rad, None, None, z, n, a)
        if k == 0:
            acc, accv, ln, _ = sc.temporal_accumulate_var(to, rad, var, 1.0)
        else:
            h, hv, l, _ = sc.reproject_var(ro, fr, z, n, acc, accv, ln, a, z, n, a, want=("history", "history_variance", "length"))
            acc, accv, ln, _ = sc.temporal_accumulate_var(to, rad, var, 1.0, h, hv, l)
    assert (ln == 8).all()
    R = sc.render(B.default_opts(spp=256, seed=s0 + 77))[1]
    mse = lambda x: float(np.mean((x - R) ** 2))  # noqa: E731
    est = sc.variance_spatial(sv, acc, accv, ln, z, n, a)
    fresh = sc.variance_spatial(sv, acc, None, None, z, n, a)
    with_est = sc.denoise(dn, acc, est, z, n, a)[0]
    print(f"MSE accumulated {mse(acc):.4g}, denoised with the estimate {mse(with_est):.4g}, with variance = NULL {mse(sc.denoise(dn, acc, None, z, n, a)[0]):.4g}, "
          f"with the all-zero variance {mse(sc.denoise(dn, acc, np.zeros_like(acc), z, n, a)[0]):.4g}; with the estimate of every pixel "
          f"{mse(sc.denoise(dn, acc, fresh, z, n, a)[0]):.4g}")
    assert mse(with_est) < mse(acc)


@pytest.mark.gpu
def test_calibration_is_recorded(B, scene):
    """One 4-spp frame of c3_mesh_small: DESIGN.md 21's rho = sum (L(x) - L(R))^2 / sum v_L over the hit pixels, for bhrt_render_var's own
    variance and for this stage's estimate (every pixel), against R = 256 spp.  Both estimate sigma^2 / 4: expectation 1 + 4 / 256.  Recorded,
    not asserted: the estimate contains the signal's gradient (rho below the expectation means it overstates the noise).  Measured
    (DESIGN.md 22): rho_own 1.6856, rho_spatial 0.9037 over 43531 hit pixels (a few bright pixels dominate both sums)."""
    sc = scene("c3_mesh_small")
    z, n, a = sc.first_hit()
    _, rad, var = sc.render_var(B.default_opts(spp=4, seed=300))
    R = sc.render(B.default_opts(spp=256, seed=377))[1]
    est = sc.variance_spatial(B.default_spatial_variance_opts(), rad, None, None, z, n, a)
    hit = z < BIG
    print(f"calibration over {hit.sum()} hit pixels: rho_own {_rho(rad, var, R, hit):.4f}, rho_spatial {_rho(rad, est, R, hit):.4f}, expectation {1 + 4 / 256:.4f}")
    assert np.isfinite(est).all() and (est >= 0).all()
