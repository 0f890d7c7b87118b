"""The denoiser (DenoiseImage of the reference's 64-bit build, Main.cpp:57-96,236-238): bhrt_render_var's per-pixel variance and
bhrt_denoise's edge-avoiding a-trous filter (csrc/denoise.hip states it).

denoise_ref below restates that filter in numpy, float32, with the kernel's tap order and sum order, vectorised over pixels: one tap of
every pixel at a time.  A tap outside the image enters with weight 0 — it adds +0 to every sum, which is what skipping it does."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import SCENES, have_gpu, same_bits

f32 = np.float32
BIG = f32(1e30)
LUM = (f32(0.2126), f32(0.7152), f32(0.0722))
HT = {-2: f32(1 / 16), -1: f32(1 / 4), 0: f32(3 / 8), 1: f32(1 / 4), 2: f32(1 / 16)}
BT = {-1: f32(0.25), 0: f32(0.5), 1: f32(0.25)}
DEFAULTS = dict(iterations=4, sigma_normal=32.0, sigma_depth=0.01, sigma_luminance=4.0, gamma=1)


def lum(e):
    return (LUM[0] * e[..., 0] + LUM[1] * e[..., 1]) + LUM[2] * e[..., 2]


def divisor(a):
    """d = max(a', 1e-3), a' = a where max(a) >= 1e-3 else 1"""
    m = np.maximum(np.maximum(a[..., 0], a[..., 1]), a[..., 2])
    ap = np.where((m >= f32(1e-3))[..., None], a, f32(1))
    return np.maximum(ap, f32(1e-3)).astype(f32)


def _tap(img, dx, dy):
    """img shifted so that [y, x] holds img[y + dy, x + dx] (clamped index) and the mask of taps inside the image."""
    H, W = img.shape[:2]
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return img[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)], ok


def denoise_ref(c, v, z, n, a, iterations=4, sigma_normal=32.0, sigma_depth=0.01, sigma_luminance=4.0, guides=True):
    """The filter of csrc/denoise.hip on (H, W, 3) / (H, W) float32 arrays; v may be None.  guides=False: w_n = w_z = 1 (the same filter
    without its edge stops; with v None also w_l = 1).  Returns the linear output image."""
    c, z, n, a = (np.asarray(t, f32) for t in (c, z, n, a))
    if iterations == 0:
        return c.copy()
    sn, sz, sl = f32(sigma_normal), f32(sigma_depth), f32(sigma_luminance)
    d = divisor(a)
    e = (c / d).astype(f32)
    var = v is not None
    vl = None
    if var:
        ve = (np.asarray(v, f32) / (d * d)).astype(f32)
        vl = ((LUM[0] * LUM[0]) * ve[..., 0] + (LUM[1] * LUM[1]) * ve[..., 1]) + (LUM[2] * LUM[2]) * ve[..., 2]
    zero = (n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0)
    miss = z >= BIG
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
                    if guides:
                        nq, _ = _tap(n, s * dx, s * dy)
                        zq, _ = _tap(z, s * dx, s * dy)
                        zq_zero, _ = _tap(zero, s * dx, s * dy)
                        q_miss, _ = _tap(miss, s * dx, s * dy)
                        dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                        with np.errstate(all="ignore"):
                            wn = np.power(np.maximum(f32(0), dot), sn)
                            r = f32(s) * np.sqrt(f32(dx * dx + dy * dy))
                            wz = np.exp(-np.abs(z - zq) / ((sz * z) * r + f32(1e-6)))
                        wn = np.where(zero | zq_zero, np.where(zero == zq_zero, f32(1), f32(0)), wn)
                        wz = np.where(miss | q_miss, np.where(miss == q_miss, f32(1), f32(0)), wz)
                        w = (w * wn) * wz
                    if var:
                        wl = np.exp(-np.abs(lp - lum(eq)) / den_l)
                        w = w * wl
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


def color24(out, gamma=1):
    """store_color24 (device_color24.h) with numpy's pow: for comparisons that allow 1 step of 255"""
    x = np.power(out.astype(np.float64), 1 / 2.2).astype(f32) if gamma else out
    return np.clip((x * f32(255) + f32(0.5)).astype(np.int64), 0, 255).astype(np.uint8)


def synthetic(W=97, H=61, seed=0):
    """A frame with depth and normal steps, misses, zero and coloured albedo, and noise: (c, v, z, n, a)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(f32)
    z = (f32(3) + f32(0.01) * xx).astype(f32)
    z[:, W // 2:] = f32(7) + f32(0.02) * yy[:, W // 2:]            # a depth step
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    tilt = xx + yy > (W + H) // 3                                     # a normal step
    n[tilt] = np.float32([0.6, 0, 0.8])
    miss = (yy < 8) & (xx > W // 3)                                   # sky
    z[miss] = BIG
    n[miss] = 0
    a = np.broadcast_to(np.float32([0.6, 0.4, 0.2]), (H, W, 3)).copy()
    a[(xx < 20) & (yy > 30)] = 0                                      # black / non-Blinn
    a[miss] = 0
    a[(xx > 70) & (yy > 40)] = np.float32([0.9, 0.0, 0.3])            # a channel without albedo
    base = np.where(tilt[..., None], f32(0.3), f32(0.8)) * np.where(xx[..., None] < W // 2, f32(1), f32(0.5))
    c = (base * np.maximum(a, f32(0.1)) * rng.gamma(4.0, 0.25, (H, W, 3)).astype(f32)).astype(f32)
    c[miss] = np.float32([0.4, 0.5, 0.7])
    v = (c * c * f32(0.25) * rng.uniform(0.5, 1.5, (H, W, 3)).astype(f32)).astype(f32)
    return c, v, z, n, a


def _synthetic_xml(tmp_path, W, H):
    p = tmp_path / f"frame_{W}x{H}.xml"
    p.write_text(f"""<xml><scene><object type="sphere" name="s" material="m"/><material type="blinn" name="m"><diffuse value="0.5"/></material>
      <light type="point" name="l"><intensity value="10"/><position z="10"/></light></scene>
      <camera><position z="10"/><target z="0"/><up y="1"/><width value="{W}"/><height value="{H}"/></camera></xml>""")
    return str(p)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_denoise_symbols_exported(B):
    L = B.lib()
    for s in ("bhrt_default_denoise_opts", "bhrt_render_var", "bhrt_render_var_dev", "bhrt_denoise", "bhrt_denoise_dev"):
        assert hasattr(L, s) and s in B.EXPORTS


def test_default_denoise_opts(B):
    o = B.default_denoise_opts()
    assert C.sizeof(B.DenoiseOpts) == 32
    got = {k: getattr(o, k) for k in DEFAULTS}
    assert got == pytest.approx(DEFAULTS) and list(o.reserved) == [0, 0, 0]
    assert B.default_denoise_opts(iterations=2, gamma=0).iterations == 2


@pytest.mark.skipif(have_gpu(), reason="checks the no-device behaviour")
def test_denoise_and_render_var_refuse_without_a_device(load_scene, B):
    sc = load_scene("c1_sphere_plane")
    img = np.zeros((sc.height, sc.width, 3), np.float32)
    with pytest.raises(B.BhrtError, match="(?i)device"):
        sc.denoise(B.default_denoise_opts(), img)
    with pytest.raises(B.BhrtError, match="(?i)device"):
        sc.render_var(B.default_opts(spp=1))


def test_reference_identities():
    c, v, z, n, a = synthetic(23, 17)
    assert same_bits(denoise_ref(c, v, z, n, a, iterations=0), c)
    # a constant image stays constant: 0.5 is exact through every weighted mean, 0.3 within rounding
    for val, exact in ((0.5, True), (0.3, False)):
        cc = np.full_like(c, f32(val))
        for vv in (v, None):
            got = denoise_ref(cc, vv, z, n, np.ones_like(a))
            assert same_bits(got, cc) if exact else np.allclose(got, cc, rtol=1e-6, atol=0)


def test_reference_keeps_a_depth_edge():
    """The guides do work in the restatement: a hard depth / normal step is not blurred across, the unguided filter blurs it."""
    c, v, z, n, a = synthetic(40, 24)
    c = np.broadcast_to(np.where((np.arange(40) < 20)[None, :, None], f32(0.2), f32(0.8)), (24, 40, 3)).astype(f32)
    z = np.where(np.arange(40) < 20, f32(3), f32(9))[None, :].repeat(24, 0).astype(f32)
    n = np.zeros_like(c)
    n[..., 2] = 1
    a = np.ones_like(c)
    g = denoise_ref(c, None, z, n, a)
    u = denoise_ref(c, None, z, n, a, guides=False)
    assert np.abs(g - c).mean() < 0.2 * np.abs(u - c).mean() and np.abs(u - c).max() > 0.1


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.gpu
def test_render_var_plumbing(B, load_scene):
    sc = load_scene("c2_glass_small")
    W, H = sc.width, sc.height
    o = B.default_opts(spp=8, gi_bounces=3, seed=3)
    rgb, rad, st = sc.render(o)
    rgb_v, rad_v, var = sc.render_var(o)
    assert np.array_equal(rgb, rgb_v) and same_bits(rad, rad_v)
    smp, _ = sc.render_samples(o, 0, 0, W, H)                       # (W*H, spp, 3)
    m = np.zeros((W * H, 3), f32)
    for s in range(o.spp):
        m = m + smp[:, s]
    m = m / f32(o.spp)
    acc = np.zeros_like(m)
    for s in range(o.spp):
        dd = smp[:, s] - m
        acc = acc + dd * dd
    ref = ((acc / f32(o.spp - 1)) / f32(o.spp)).reshape(H, W, 3)
    assert same_bits(m.reshape(H, W, 3), rad)
    err = np.abs(var - ref) / np.maximum(np.abs(ref), 1e-9)
    assert (np.abs(var - ref) <= np.maximum(1e-6 * np.abs(ref), 1e-9)).all(), float(err.max())
    assert (var > 0).mean() > 0.1
    # the same variance when the frame takes several passes
    o3 = B.default_opts(spp=8, gi_bounces=3, seed=3, samples_per_pass=W * H * 8 // 3)
    assert sc.render(o3)[2].passes >= 3
    rgb3, rad3, var3 = sc.render_var(o3)
    assert np.array_equal(rgb3, rgb) and same_bits(rad3, rad) and same_bits(var3, var)
    # one sample: zero variance
    _, _, var1 = sc.render_var(B.default_opts(spp=1, seed=3))
    assert not var1.any()


@pytest.mark.gpu
def test_render_var_leaves_other_ranks_tiles_alone(B, load_scene):
    import torch
    sc = load_scene("c1_sphere_plane")
    W, H = sc.width, sc.height
    var = torch.full((H, W, 3), -1.0, dtype=torch.float32, device=_dev())
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device=_dev())
    sc.render_var_dev(B.default_opts(spp=4, rank=1, world_size=2, tile_size=16), 0, rad.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    v = var.cpu().numpy()
    t = (np.arange(H)[:, None] // 16) * ((W + 15) // 16) + np.arange(W)[None, :] // 16
    assert (v[t % 2 == 0] == -1).all() and (v[t % 2 == 1] >= 0).all()


def _check_vs_ref(out, rgb, ref, gamma=1):
    rel = np.abs(out - ref) / np.maximum(np.abs(ref), 1e-6)
    assert (np.abs(out - ref) <= np.maximum(1e-4 * np.abs(ref), 1e-6)).all(), float(rel.max())
    diff = np.abs(rgb.astype(int) - color24(ref, gamma).astype(int))
    assert diff.max() <= 1 and (diff > 0).any(axis=-1).mean() <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("with_var", [True, False])
def test_kernel_matches_restatement_synthetic(B, tmp_path, with_var):
    W, H = 97, 61
    sc = B.Scene(_synthetic_xml(tmp_path, W, H))
    c, v, z, n, a = synthetic(W, H)
    for K, sn, sz, sl in ((5, 128.0, 0.02, 4.0), (3, 16.0, 0.5, 1.0), (1, 0.0, 0.0, 0.0)):
        o = B.default_denoise_opts(iterations=K, sigma_normal=sn, sigma_depth=sz, sigma_luminance=sl)
        out, rgb = sc.denoise(o, c, v if with_var else None, z, n, a)
        ref = denoise_ref(c, v if with_var else None, z, n, a, K, sn, sz, sl)
        _check_vs_ref(out, rgb, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("with_var", [True, False])
def test_kernel_matches_restatement_render(B, load_scene, with_var):
    sc = load_scene("c3_mesh_small")
    _, rad, var = sc.render_var(B.default_opts(spp=4, seed=11))
    z, n, a = sc.first_hit()
    o = B.default_denoise_opts()
    out, rgb = sc.denoise(o, rad, var if with_var else None, z, n, a)
    _check_vs_ref(out, rgb, denoise_ref(rad, var if with_var else None, z, n, a))


@pytest.mark.gpu
def test_denoise_identities(B, load_scene):
    import torch
    sc = load_scene("c3_mesh_small")
    W, H = sc.width, sc.height
    ro = B.default_opts(spp=4, seed=5)
    rgb, rad, var = sc.render_var(ro)
    out0, rgb0 = sc.denoise(B.default_denoise_opts(iterations=0), rad, var)
    assert same_bits(out0, rad) and np.array_equal(rgb0, rgb)
    rgb_ng = sc.render_var(B.default_opts(spp=4, seed=5, gamma=0))[0]
    assert np.array_equal(sc.denoise(B.default_denoise_opts(iterations=0, gamma=0), rad)[1], rgb_ng)
    o = B.default_denoise_opts()
    a1, b1 = sc.denoise(o, rad, var)
    a2, b2 = sc.denoise(o, rad, var)
    assert same_bits(a1, a2) and np.array_equal(b1, b2)
    z, n, al = sc.first_hit()
    a3, b3 = sc.denoise(o, rad, var, z, n, al)
    assert same_bits(a1, a3) and np.array_equal(b1, b3)
    # the device entry point on a stream, guides partly given: the same bytes
    dev = _dev()
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in (("c", rad), ("v", var), ("n", n))}
    d_out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    d_rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    sc.denoise_dev(o, t["c"].data_ptr(), t["v"].data_ptr(), 0, t["n"].data_ptr(), 0, d_out.data_ptr(), d_rgb.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert same_bits(d_out.cpu().numpy(), a1) and np.array_equal(d_rgb.cpu().numpy(), b1)
    # rgb8 alone
    d_rgb.zero_()
    sc.denoise_dev(o, t["c"].data_ptr(), t["v"].data_ptr(), d_rgb8=d_rgb.data_ptr())
    assert np.array_equal(d_rgb.cpu().numpy(), b1)


def _edges(sc, B, O):
    o, d = O.primary_rays(sc.flat_view())
    h = sc.trace_closest(o, d, B.SIDE_FRONT)
    key = (h["node"].astype(np.int64) << 32) + h["prim"].astype(np.int64) + 1
    key = key.reshape(sc.height, sc.width)
    edge = np.zeros(key.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            kq, ok = _tap(key, dx, dy)
            edge |= ok & (kq != key)
    return edge


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3_mesh_small", "c3_room_small", "c2_glass_small"])
def test_denoise_quality(B, O, load_scene, name):
    """4 spp against a 1024 spp frame of another seed, in linear radiance: the denoiser at least halves the MSE, and on edge pixels (a 3x3
    neighbourhood with more than one first-hit node / triangle) the guided filter does no worse than the same filter without its guides."""
    sc = load_scene(name)
    # the reference frame on a handle of its own, closed at once: a 1024-spp frame sizes a workspace of tens of GB, which the session's
    # cached scene would otherwise keep for the rest of the suite
    own = B.Scene(os.path.join(SCENES, name + ".xml"))
    try:
        _, ref, _ = own.render(B.default_opts(spp=1024, seed=77))
    finally:
        own.close()
    _, rad, var = sc.render_var(B.default_opts(spp=4, seed=1))
    z, n, a = sc.first_hit()
    o = B.default_denoise_opts()
    out, _ = sc.denoise(o, rad, var)
    flat_z, flat_n = np.ones_like(z), np.zeros_like(n)
    flat_n[..., 2] = 1
    plain, _ = sc.denoise(o, rad, None, flat_z, flat_n, a)            # w_n = w_z = w_l = 1: the same filter, no guides
    mse = lambda x, m=None: float(np.mean(((x - ref) ** 2)[m] if m is not None else (x - ref) ** 2))  # noqa: E731
    edge = _edges(sc, B, O)
    print(f"{name}: MSE noisy {mse(rad):.4g} denoised {mse(out):.4g} unguided {mse(plain):.4g}; edges ({edge.mean():.1%}): "
          f"noisy {mse(rad, edge):.4g} denoised {mse(out, edge):.4g} unguided {mse(plain, edge):.4g}")
    assert mse(out) <= 0.5 * mse(rad)
    assert mse(out, edge) <= mse(plain, edge)
