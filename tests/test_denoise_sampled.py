"""The denoiser for sampled guides (bhrt_denoise_sampled): bhrt_denoise's filter with a demodulation that knows the background's
share of a partly covered pixel, a normal weight on the direction of the averaged normal, and the coverage as a weight of its own
(csrc/denoise.hip states it beside the other filter).

denoise_sampled_ref below restates it in numpy, float32, with the tap and sum order of tests/test_denoise.py's denoise_ref, the precise
np.power and np.exp and the product of the four weights as the definition writes them; the kernel, which folds a tap's weights into one
hardware exp2, is held to it within the bound the other kernel is held to its restatement (_check_vs_ref)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENES, have_gpu, same_bits
from test_denoise import BIG, BT, HT, LUM, _check_vs_ref, _edges, _synthetic_xml, _tap, color24, denoise_ref, divisor, lum, synthetic

f32 = np.float32
OPTION_SETS = ((5, 128.0, 0.02, 4.0), (3, 16.0, 0.5, 1.0), (1, 0.0, 0.0, 0.0))


def unit(n):
    """B: l = sqrt((n.x n.x + n.y n.y) + n.z n.z); n / l per component where l > 0, else 0"""
    n = np.asarray(n, f32)
    l = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).astype(f32)
    with np.errstate(all="ignore"):
        return np.where((l > 0)[..., None], n / l[..., None], f32(0)).astype(f32)


def sampled_divisor(a, cov):
    """A: d = max(a', 1e-3), a' = a + (1 - cov) where its largest channel is >= 1e-3, else 1"""
    t = (f32(1) - np.asarray(cov, f32)).astype(f32)
    return divisor((np.asarray(a, f32) + t[..., None]).astype(f32))


def denoise_sampled_ref(c, v, z, n, a, cov, iterations=4, sigma_normal=32.0, sigma_depth=0.01, sigma_luminance=4.0, sigma_coverage=None):
    """The filter for sampled guides of csrc/denoise.hip on (H, W, 3) / (H, W) float32 arrays; v may be None.  Returns the linear output."""
    c, z, n, a, cov = (np.asarray(t, f32) for t in (c, z, n, a, cov))
    if iterations == 0:
        return c.copy()
    sn, sz, sl, sc = f32(sigma_normal), f32(sigma_depth), f32(sigma_luminance), f32(sigma_coverage)
    d = sampled_divisor(a, cov)
    e = (c / d).astype(f32)
    var = v is not None
    vl = None
    if var:
        ve = (np.asarray(v, f32) / (d * d)).astype(f32)
        vl = ((LUM[0] * LUM[0]) * ve[..., 0] + (LUM[1] * LUM[1]) * ve[..., 1]) + (LUM[2] * LUM[2]) * ve[..., 2]
    n = unit(n)
    zero = (n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0)
    miss = z >= BIG
    den_c = sc + f32(1e-6)
    for k in range(iterations):
        s = 1 << k
        lp = lum(e)
        if var:
            gs, gw = np.zeros_like(vl), np.zeros_like(vl)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    vq, ok = _tap(vl, dx, dy)
                    w = np.where(ok, BT[dx] * BT[dy], f32(0))
                    gs = gs + w * vq
                    gw = gw + w
            den_l = sl * np.sqrt(gs / gw) + f32(1e-4)
        sw = np.zeros(c.shape[:2], f32)
        se = np.zeros(c.shape, f32)
        sv = np.zeros(c.shape[:2], f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                eq, ok = _tap(e, s * dx, s * dy)
                if dx == 0 and dy == 0:
                    w = np.full(c.shape[:2], f32(0.375) * f32(0.375), f32)
                else:
                    w = np.full(c.shape[:2], HT[dx] * HT[dy], f32)
                    nq, _ = _tap(n, s * dx, s * dy)
                    zq, _ = _tap(z, s * dx, s * dy)
                    zq_zero, _ = _tap(zero, s * dx, s * dy)
                    q_miss, _ = _tap(miss, s * dx, s * dy)
                    cq, _ = _tap(cov, s * dx, s * dy)
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    with np.errstate(all="ignore"):
                        wn = np.power(np.maximum(f32(0), dot), sn)
                        r = f32(s) * np.sqrt(f32(dx * dx + dy * dy))
                        wz = np.exp(-np.abs(z - zq) / ((sz * z) * r + f32(1e-6)))
                    wn = np.where(zero | zq_zero, np.where(zero == zq_zero, f32(1), f32(0)), wn)
                    wz = np.where(miss | q_miss, np.where(miss == q_miss, f32(1), f32(0)), wz)
                    w = (w * wn) * wz
                    if var:
                        w = w * np.exp(-np.abs(lp - lum(eq)) / den_l)
                    w = w * np.exp(-np.abs(cov - cq) / den_c)
                w = np.where(ok, w, f32(0)).astype(f32)
                sw = sw + w
                se = se + w[..., None] * eq
                if var:
                    vq, _ = _tap(vl, s * dx, s * dy)
                    sv = sv + (w * w) * vq
        e = (se / sw[..., None]).astype(f32)
        if var:
            vl = (sv / (sw * sw)).astype(f32)
    return (e * d).astype(f32)


def pinhole_coverage(z):
    return np.where(z >= BIG, f32(0), f32(1)).astype(f32)


def banded(W=97, H=61, lo=43, width=10):
    """synthetic() with the coverage of one pinhole sample and, across the depth step, a band of partial coverage: cov ramps 0 .. 1 over
    columns lo .. lo + width, n and a scaled by it, a miss where it is 0.  Returns (c, v, z, n, a, cov)."""
    c, v, z, n, a = synthetic(W, H)
    cov = pinhole_coverage(z)
    ramp = np.clip((np.arange(W, dtype=f32) - f32(lo)) / f32(width), 0, 1).astype(f32)
    band = (np.arange(W) >= lo) & (np.arange(W) <= lo + width)
    cov[:, band] = cov[:, band] * ramp[band][None, :]
    n = (n * cov[..., None]).astype(f32)
    a = (a * cov[..., None]).astype(f32)
    z = np.where(cov > 0, z, BIG).astype(f32)
    assert ((cov > 0) & (cov < 1)).sum() >= 8 * (H - 8) and (cov == 0).any() and (cov == 1).any()
    return c, v, z, n, a, cov


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_sampled_denoiser_symbols_exported_and_declared(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in ("bhrt_denoise_sampled", "bhrt_denoise_sampled_dev"):
        assert hasattr(B.lib(), s) and s in B.EXPORTS
        assert re.search(r"\bint " + s + r"\(", hdr)


def test_python_wrappers_exist(B):
    assert callable(B.Scene.denoise_sampled) and callable(B.Scene.denoise_sampled_dev)


def test_default_sigma_coverage(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    m = re.search(r"#define\s+BHRT_DENOISE_SIGMA_COVERAGE\s+([0-9.eE+-]+)f\b", hdr)
    assert m, "include/bhrt.h names no default"
    assert float(m.group(1)) == B.DENOISE_SIGMA_COVERAGE
    assert np.isfinite(B.DENOISE_SIGMA_COVERAGE) and B.DENOISE_SIGMA_COVERAGE > 0


@pytest.mark.skipif(have_gpu(), reason="checks the no-device behaviour")
def test_sampled_denoiser_refuses_without_a_device(load_scene, B):
    sc = load_scene("c1_sphere_plane")
    img = np.zeros((sc.height, sc.width, 3), f32)
    one = np.ones((sc.height, sc.width), f32)
    with pytest.raises(B.BhrtError, match="(?i)device"):
        sc.denoise_sampled(B.default_denoise_opts(), img, None, one, img, img, one)
    with pytest.raises(B.BhrtError, match="(?i)device"):
        sc.denoise_sampled_dev(B.default_denoise_opts(), B.DENOISE_SIGMA_COVERAGE, 0)


def test_restatement_with_pinhole_guides_is_the_other_restatement():
    """cov = 0 on misses and 1 elsewhere, the frame's unit normals: A is the old divisor, w_c = 1 wherever w_z != 0, B differs by rounding."""
    c, v, z, n, a = synthetic()
    cov = pinhole_coverage(z)
    assert same_bits(sampled_divisor(a, cov), divisor(a))
    for vv in (v, None):
        for K, sn, sz, sl in OPTION_SETS + ((4, 32.0, 0.01, 4.0),):
            for sc in (0.25, 0.0):
                new = denoise_sampled_ref(c, vv, z, n, a, cov, K, sn, sz, sl, sc)
                old = denoise_ref(c, vv, z, n, a, K, sn, sz, sl)
                _check_vs_ref(new, color24(new), old)


def test_restatement_keeps_a_frame_of_constant_irradiance():
    """A fixed point: c = E (a + (1 - cov)) for a constant E, so that e = E everywhere and every weighted mean returns E, whatever the guide
    weights are: the output is c to 1e-5 relative for K = 1, 3, 5.  (The frame's albedo is floored at 0.05 on hits first: where a channel of
    a + (1 - cov) is 0 the colour E x 0 is 0, which is not E d for the clamped d, and no filter that demodulates could return it.)
    denoise_ref fed the same images does not return c: in the band it divides by cov x kd alone."""
    E = f32(0.7)
    c, v, z, n, a, cov = banded()
    hit = z < BIG
    a = np.where(hit[..., None], np.maximum(a, f32(0.05) * cov[..., None]), a).astype(f32)
    c = (E * (a + (f32(1) - cov)[..., None])).astype(f32)
    band = (cov > 0) & (cov < 1)
    for K in (1, 3, 5):
        for vv, sn, sz, sl, sc in ((None, 32.0, 0.01, 4.0, 0.25), (v, 128.0, 0.02, 4.0, 0.0), (v, 0.0, 0.5, 1.0, 10.0)):
            out = denoise_sampled_ref(c, vv, z, n, a, cov, K, sn, sz, sl, sc)
            rel = np.abs(out - c) / np.abs(c)
            assert rel.max() <= 1e-5, (K, float(rel.max()))
        old = denoise_ref(c, None, z, n, a, K)
        rel_old = np.abs(old - c) / np.abs(c)
        print(f"K = {K}: the filter without coverage is off by up to {rel_old[band].max():.3g} relative in the band")
        assert rel_old[band].max() > 1e-2


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lens_frame(B, load_scene):
    """lens_spheres, 4 spp through the lens, with bhrt_guides at 8 spp of the same seed and lens: shared, read-only."""
    sc = load_scene("lens_spheres")
    rgb, rad, var = sc.render_var(B.default_opts(spp=4, seed=5, lens=1))
    g = sc.guides(B.default_opts(spp=8, seed=5, lens=1))
    for x in (rgb, rad, var, *g.values()):
        x.setflags(write=False)
    return sc, rgb, rad, var, g


@pytest.mark.gpu
@pytest.mark.parametrize("with_var", [True, False])
def test_sampled_kernel_matches_restatement_synthetic(B, tmp_path, with_var):
    W, H = 97, 61
    sc = B.Scene(_synthetic_xml(tmp_path, W, H))
    try:
        c, v, z, n, a, cov = banded(W, H)
        vv = v if with_var else None
        for K, sn, sz, sl in OPTION_SETS:
            o = B.default_denoise_opts(iterations=K, sigma_normal=sn, sigma_depth=sz, sigma_luminance=sl)
            for sigc in (B.DENOISE_SIGMA_COVERAGE, 0.0, 10.0):
                out, rgb = sc.denoise_sampled(o, c, vv, z, n, a, cov, sigc)
                ref = denoise_sampled_ref(c, vv, z, n, a, cov, K, sn, sz, sl, sigc)
                print(f"K {K} sigma_n {sn} sigma_c {sigc}: max relative difference {float((np.abs(out - ref) / np.maximum(np.abs(ref), 1e-6)).max()):.3g}")
                _check_vs_ref(out, rgb, ref)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_var", [True, False])
def test_sampled_kernel_matches_restatement_render(B, lens_frame, with_var):
    sc, _, rad, var, g = lens_frame
    vv = var if with_var else None
    assert ((g["coverage"] > 0) & (g["coverage"] < 1)).mean() > 0.01
    out, rgb = sc.denoise_sampled(B.default_denoise_opts(), rad, vv, g["z"], g["normal"], g["albedo"], g["coverage"])
    ref = denoise_sampled_ref(rad, vv, g["z"], g["normal"], g["albedo"], g["coverage"], sigma_coverage=B.DENOISE_SIGMA_COVERAGE)
    print(f"max relative difference {float((np.abs(out - ref) / np.maximum(np.abs(ref), 1e-6)).max()):.3g}")
    _check_vs_ref(out, rgb, ref)


@pytest.mark.gpu
def test_sampled_denoise_identities(B, lens_frame):
    import torch
    sc, rgb, rad, var, g = lens_frame
    W, H = sc.width, sc.height
    G = (g["z"], g["normal"], g["albedo"], g["coverage"])
    sig = B.DENOISE_SIGMA_COVERAGE
    o = B.default_denoise_opts()
    before = sc.denoise(o, rad, var)
    # K = 0: the radiance bit for bit and the render's bytes; no guide is read
    out0, rgb0 = sc.denoise_sampled(B.default_denoise_opts(iterations=0), rad, var, *G)
    assert same_bits(out0, rad) and np.array_equal(rgb0, rgb)
    out0, rgb0 = sc.denoise_sampled(B.default_denoise_opts(iterations=0), rad, None, None, None, None, None)
    assert same_bits(out0, rad) and np.array_equal(rgb0, rgb)
    # two calls: the same bytes
    a1, b1 = sc.denoise_sampled(o, rad, var, *G)
    a2, b2 = sc.denoise_sampled(o, rad, var, *G)
    assert same_bits(a1, a2) and np.array_equal(b1, b2) and not same_bits(a1, rad)
    # bhrt_denoise before and after: identical bits
    after = sc.denoise(o, rad, var)
    assert same_bits(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the device entry point on a stream
    dev = _dev()
    t = {k: torch.from_numpy(np.array(x, np.float32)).to(dev) for k, x in (("c", rad), ("v", var), ("z", G[0]), ("n", G[1]), ("a", G[2]), ("cov", G[3]))}
    d_out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    d_rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    ptrs = [t[k].data_ptr() for k in ("c", "v", "z", "n", "a", "cov")]
    sc.denoise_sampled_dev(o, sig, *ptrs, d_out.data_ptr(), d_rgb.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert same_bits(d_out.cpu().numpy(), a1) and np.array_equal(d_rgb.cpu().numpy(), b1)
    # rgb8 alone and out alone
    d_out.zero_()
    d_rgb.zero_()
    sc.denoise_sampled_dev(o, sig, *ptrs, d_rgb8=d_rgb.data_ptr())
    assert np.array_equal(d_rgb.cpu().numpy(), b1) and not d_out.any()
    d_rgb.zero_()
    sc.denoise_sampled_dev(o, sig, *ptrs, d_out=d_out.data_ptr())
    assert same_bits(d_out.cpu().numpy(), a1) and not d_rgb.any()
    # bad arguments
    for k in range(4):
        part = list(G)
        part[k] = None
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: "):
            sc.denoise_sampled(o, rad, var, *part)
        dp = list(ptrs)
        dp[2 + k] = 0
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: "):
            sc.denoise_sampled_dev(o, sig, *dp, d_out.data_ptr(), d_rgb.data_ptr())
    for bad in (float("nan"), -0.5, float("inf")):
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*sigma_coverage"):
            sc.denoise_sampled(o, rad, var, *G, bad)
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*sigma_coverage"):
            sc.denoise_sampled_dev(o, bad, *ptrs, d_out.data_ptr(), d_rgb.data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lens_spheres", "c3_mesh_small"])
def test_one_pinhole_sample_gives_the_other_denoiser(B, load_scene, name):
    """Guides from bhrt_guides(spp = 1, jitter = 0): 0 / 1 coverage that matches the misses and unit normals, so the filter is bhrt_denoise's
    to rounding."""
    sc = load_scene(name)
    _, rad, var = sc.render_var(B.default_opts(spp=4, seed=5))
    g = sc.guides(B.default_opts(spp=1, jitter=0))
    assert set(np.unique(g["coverage"]).tolist()) <= {0.0, 1.0}
    o = B.default_denoise_opts()
    for vv in (var, None):
        old, _ = sc.denoise(o, rad, vv)
        new, rgb = sc.denoise_sampled(o, rad, vv, g["z"], g["normal"], g["albedo"], g["coverage"])
        _check_vs_ref(new, rgb, old)


@pytest.mark.gpu
def test_coverage_filter_quality_on_a_lens_frame(B, load_scene):
    """The point of the filter.  The setup of tests/test_guides.py::test_sampled_guides_against_the_denoisers_own_on_a_lens_frame: lens_spheres
    at 8 spp (seed 1) through the lens, guides at 8 spp, mean squared error on linear radiance against a 2048-spp frame of seed 77.  With the
    sampled guides the new filter must beat both the noisy frame and bhrt_denoise, over the frame and over the blurred pixels (0 < coverage
    < 1, dilated by one pixel).  Measured on an MI355X (the figures this test prints):
        frame:    noisy 0.003329, bhrt_denoise with its own pinhole guides 0.000944, bhrt_denoise with sampled guides 0.003055, new 0.002424
        blurred:  noisy 0.002539, own 0.001885, sampled 0.002478, new 0.002375
    The new filter does NOT beat bhrt_denoise with its own pinhole guides, on the frame or on the blurred pixels: at 8 guide samples the averaged
    z is noisy against sigma_depth, and the mirror and glass spheres carry light that the albedo guide has no share of.  That
    comparison is printed, not asserted."""
    sc = load_scene("lens_spheres")
    own = B.Scene(os.path.join(SCENES, "lens_spheres.xml"))  # the reference frame's workspace goes with its handle
    try:
        _, ref, _ = own.render(B.default_opts(spp=2048, seed=77, lens=1))
    finally:
        own.close()
    opts = B.default_opts(spp=8, seed=1, lens=1)
    _, noisy, var = sc.render_var(opts)
    o = B.default_denoise_opts()
    old_own, _ = sc.denoise(o, noisy, var)
    g = sc.guides(opts)
    old_sampled, _ = sc.denoise(o, noisy, var, g["z"], g["normal"], g["albedo"])
    new, _ = sc.denoise_sampled(o, noisy, var, g["z"], g["normal"], g["albedo"], g["coverage"])
    mse = lambda x, m=None: float(np.mean(((x.astype(np.float64) - ref) ** 2)[m] if m is not None else (x.astype(np.float64) - ref) ** 2))  # noqa: E731
    partial = (g["coverage"] > 0) & (g["coverage"] < 1)
    blurred = partial.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            blurred |= np.roll(np.roll(partial, dy, 0), dx, 1)
    for what, m in (("frame", None), (f"blurred pixels ({blurred.mean():.1%})", blurred)):
        print(f"MSE against 2048 spp, {what}: noisy {mse(noisy, m):.4g}, own guides {mse(old_own, m):.4g}, sampled guides {mse(old_sampled, m):.4g}, "
              f"coverage filter {mse(new, m):.4g}")
    assert np.isfinite(new).all()
    for m in (None, blurred):
        assert mse(new, m) < mse(old_sampled, m)
        assert mse(new, m) < mse(noisy, m)


@pytest.mark.gpu
def test_coverage_filter_on_a_jittered_frame_without_the_lens(B, O, load_scene):
    """c3_mesh_small at 4 spp, jittered, lens off, guides at 16 spp, against a 1024-spp frame of another seed: the figures of the new filter
    beside bhrt_denoise's (its own pinhole guides), whole frame and edge pixels, are printed and recorded in DESIGN.md 17; asserted is only
    that the new filter does not raise the error of the noisy frame.  Measured on an MI355X:
        frame: noisy 0.000961, bhrt_denoise 0.0001858, new 0.0001781;   edges (5.2 %): noisy 0.003418, bhrt_denoise 0.00143, new 0.001185"""
    sc = load_scene("c3_mesh_small")
    own = B.Scene(os.path.join(SCENES, "c3_mesh_small.xml"))
    try:
        _, ref, _ = own.render(B.default_opts(spp=1024, seed=77))
    finally:
        own.close()
    _, noisy, var = sc.render_var(B.default_opts(spp=4, seed=1))
    g = sc.guides(B.default_opts(spp=16, seed=1))
    o = B.default_denoise_opts()
    old, _ = sc.denoise(o, noisy, var)
    new, _ = sc.denoise_sampled(o, noisy, var, g["z"], g["normal"], g["albedo"], g["coverage"])
    mse = lambda x, m=None: float(np.mean(((x.astype(np.float64) - ref) ** 2)[m] if m is not None else (x.astype(np.float64) - ref) ** 2))  # noqa: E731
    edge = _edges(sc, B, O)
    print(f"c3_mesh_small 4 spp, guides 16 spp: MSE noisy {mse(noisy):.4g}, bhrt_denoise {mse(old):.4g}, coverage filter {mse(new):.4g}; "
          f"edges ({edge.mean():.1%}): noisy {mse(noisy, edge):.4g}, bhrt_denoise {mse(old, edge):.4g}, coverage filter {mse(new, edge):.4g}")
    assert mse(new) <= mse(noisy)
