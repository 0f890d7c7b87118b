"""Adaptive sampling (bhrt_render_adaptive) and the sample-count image (RenderImage::ComputeSampleCountImage, scene.h:603-626).

The guarantee under test: every pixel of an adaptive frame is bit-identical to the same pixel of a uniform render at that pixel's sample
count, and each count is what the rounds and the retirement test of include/bhrt.h give, restated below in numpy float32 from the
per-sample radiance of bhrt_render_samples."""
import math
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits

f32 = np.float32
LUM = (f32(0.2126), f32(0.7152), f32(0.0722))
SCENES3 = ["c3_room_small", "c2_glass_small", "c3_mesh_small"]


@pytest.fixture
def scene(B):
    """Private scene handles, freed with their device state when the test ends: the workspaces these tests grow stay out of the
    session's shared scene cache."""
    opened = []

    def _load(name):
        opened.append(B.Scene(os.path.join(SCENES, name + ".xml")))
        return opened[-1]
    yield _load
    for sc in opened:
        sc.close()


def schedule(n_min, n_max):
    out, n = [n_min], n_min
    while n < n_max:
        n = min(n_max, 2 * n)
        out.append(n)
    return out


def counts_ref(samples, n_min, n_max, threshold, floor):
    """The rounds and the retirement test on samples (pixels, >= n_max, 3) float32, in the kernel's operations and order."""
    P = samples.shape[0]
    S, mu, M2 = (np.zeros((P, 3), f32) for _ in range(3))
    cnt = np.zeros(P, np.uint32)
    active = np.ones(P, bool)
    stops = set(schedule(n_min, n_max))
    thr, fl = f32(threshold), f32(floor)
    for k in range(1, n_max + 1):
        x = samples[:, k - 1].astype(f32)
        S = S + x
        d = x - mu
        mu = mu + d / f32(k)
        M2 = M2 + d * (x - mu)
        if k in stops:
            m = S / f32(k)
            v = (M2 / f32(k - 1)) / f32(k)
            L = (LUM[0] * m[:, 0] + LUM[1] * m[:, 1]) + LUM[2] * m[:, 2]
            vL = ((LUM[0] * LUM[0]) * v[:, 0] + (LUM[1] * LUM[1]) * v[:, 1]) + (LUM[2] * LUM[2]) * v[:, 2]
            retire = active & ((k >= n_max) | (np.sqrt(vL) <= thr * np.fmax(L, fl)))
            cnt[retire] = k
            active &= ~retire
    assert not active.any()
    return cnt


def count_image_ref(cnt):
    """ComputeSampleCountImage (scene.h:603-626) in integers."""
    c = np.asarray(cnt, np.int64)
    smin, smax = int(c.min()), int(c.max())
    if smax == smin:
        return np.zeros(c.shape, np.uint8), smax
    return np.clip((255 * (c - smin)) // (smax - smin), 0, 255).astype(np.uint8), smax


# ---- CPU: options and argument checks (before any device is touched) -----------------------------------------------------------------
def test_default_adaptive_opts(B):
    a = B.default_adaptive_opts()
    assert (a.min_spp, round(a.threshold, 6), round(a.floor, 6)) == (16, 0.01, 0.1)
    assert list(a.reserved) == [0] * 5
    assert B.default_adaptive_opts(min_spp=4, threshold=-1.0).min_spp == 4


@pytest.mark.parametrize("spp,kw,msg", [
    (32, dict(min_spp=1), "min_spp"),
    (8, dict(min_spp=16), "min_spp"),
    (65536, dict(min_spp=16), "spp"),
    (32, dict(floor=0.0), "floor"),
    (32, dict(threshold=float("nan")), "NaN"),
])
def test_invalid_arguments_are_refused_before_the_device(B, scene, spp, kw, msg):
    sc = scene("c1_sphere_plane")
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*" + msg):
        sc.render_adaptive(B.default_opts(spp=spp), B.default_adaptive_opts(**kw))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES3)
def test_never_retiring_equals_the_uniform_render(B, scene, name):
    sc = scene(name)
    o = B.default_opts(spp=8, gi_bounces=3, seed=5)
    rgb, rad, var, cnt, st = sc.render_adaptive(o, B.default_adaptive_opts(min_spp=2, threshold=-1.0))
    assert (cnt == 8).all()
    urgb, urad, uvar = sc.render_var(o)
    assert np.array_equal(rgb, urgb) and same_bits(rad, urad)
    assert np.all(np.abs(var - uvar) <= 1e-4 * np.abs(uvar) + 1e-12)
    assert st.camera_samples == int(cnt.sum()) == sc.width * sc.height * 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES3)
def test_infinite_threshold_stops_at_min_spp(B, scene, name):
    sc = scene(name)
    rgb, rad, var, cnt, st = sc.render_adaptive(B.default_opts(spp=32, seed=3), B.default_adaptive_opts(min_spp=4, threshold=math.inf))
    assert (cnt == 4).all()
    urgb, urad, _ = sc.render(B.default_opts(spp=4, seed=3))
    assert np.array_equal(rgb, urgb) and same_bits(rad, urad)
    assert st.camera_samples == int(cnt.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES3)
def test_each_pixel_equals_the_uniform_render_at_its_count(B, scene, name):
    sc = scene(name)
    H, W = sc.height, sc.width
    o = B.default_opts(spp=64, gi_bounces=3, seed=11)
    a = B.default_adaptive_opts(min_spp=4, threshold=0.05, floor=0.05)
    rgb, rad, var, cnt, st = sc.render_adaptive(o, a)
    levels = schedule(4, 64)
    assert set(np.unique(cnt).tolist()) <= set(levels)
    assert (cnt == 4).any() and (cnt == 64).any()
    assert st.camera_samples == int(cnt.sum())
    for n in levels:
        sel = cnt == n
        if not sel.any():
            continue
        urgb, urad, uvar = sc.render_var(B.default_opts(spp=n, gi_bounces=3, seed=11))
        assert np.array_equal(rgb[sel], urgb[sel]) and same_bits(rad[sel], urad[sel]), n
        assert np.all(np.abs(var[sel] - uvar[sel]) <= 1e-4 * np.abs(uvar[sel]) + 1e-12), n
    samples, _ = sc.render_samples(o, 0, 0, W, H)
    ref = counts_ref(samples, 4, 64, 0.05, 0.05).reshape(H, W)
    assert np.array_equal(cnt, ref), f"{int((cnt != ref).sum())} pixels differ"


@pytest.mark.gpu
def test_partition_invariance(B, scene):
    sc = scene("c3_mesh_small")
    a = B.default_adaptive_opts(min_spp=4, threshold=0.05, floor=0.05)
    ref = sc.render_adaptive(B.default_opts(spp=32, seed=4), a)
    parts = [sc.render_adaptive(B.default_opts(spp=32, seed=4, rank=r, world_size=3, tile_size=16), a) for r in range(3)]
    owned = [p[3] > 0 for p in parts]
    assert (sum(m.astype(int) for m in owned) == 1).all()  # every pixel rendered by exactly one rank
    for k in range(4):
        comp = np.zeros_like(ref[k])
        for p, m in zip(parts, owned):
            comp[m] = p[k][m]
        assert same_bits(comp, ref[k]) if comp.dtype == np.float32 else np.array_equal(comp, ref[k]), k
    assert sum(p[4].camera_samples for p in parts) == ref[4].camera_samples


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2_glass_small", "c3_mesh_small"])
def test_overflowing_passes_inside_rounds(B, scene, name):
    sc = scene(name)
    o = B.default_opts(spp=16, gi_bounces=3, seed=9)
    a = B.default_adaptive_opts(min_spp=4, threshold=0.05, floor=0.05)
    base = sc.render_adaptive(o, a)
    sc.knob("frame_cap", max(1, int(base[4].shade_calls) // 8))
    try:
        got = sc.render_adaptive(o, a)
    finally:
        sc.knob("frame_cap", 0)
    assert got[4].passes > base[4].passes
    assert np.array_equal(got[0], base[0]) and same_bits(got[1], base[1]) and same_bits(got[2], base[2]) and np.array_equal(got[3], base[3])


@pytest.mark.gpu
def test_photon_map_never_retiring_equals_uniform(B, scene):
    sc = scene("c5_caustics")
    o = B.default_opts(spp=4, gi_bounces=2, seed=3, photon_map=1)
    assert sc.photon_build(B.default_opts(), 20000) > 0
    rgb, rad, _, cnt, _ = sc.render_adaptive(o, B.default_adaptive_opts(min_spp=2, threshold=-1.0))
    urgb, urad, _ = sc.render(o)
    assert (cnt == 4).all() and np.array_equal(rgb, urgb) and same_bits(rad, urad)


@pytest.mark.gpu
def test_sample_count_image_and_repeatability(B, scene):
    sc = scene("c3_room_small")
    o, a = B.default_opts(spp=32, seed=7), B.default_adaptive_opts(min_spp=4, threshold=0.05, floor=0.05)
    first = sc.render_adaptive(o, a)
    second = sc.render_adaptive(o, a)
    for x, y in zip(first[:4], second[:4]):
        assert x.tobytes() == y.tobytes()
    cnt = first[3]
    img, smax = sc.sample_count_image(cnt)
    rimg, rmax = count_image_ref(cnt)
    assert np.array_equal(img, rimg) and smax == rmax and len(np.unique(img)) > 1
    z = np.zeros_like(cnt)
    img0, smax0 = sc.sample_count_image(z)
    assert not img0.any() and smax0 == 0
    img7, smax7 = sc.sample_count_image(z + 7)
    assert not img7.any() and smax7 == 7
