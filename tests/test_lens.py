"""Thin-lens camera (bhrt_opts.lens, bhrt_scene_set_lens): depth of field from the scene's <dof> and <focaldist>.

The lens model is restated below in numpy float32 (lens_rays_ref), with sqrt, sin, cos and rand_to_unit taken from the oracle's device-math
evaluator, so the restatement needs no GPU.  The GPU tests hold bhrt_camera_rays equal to it bit for bit, and the per-sample radiance of a
lens render equal to the oracle's for a camera whose `pos` is the lens origin of that sample: the oracle forms `ray.dir = target - cam.pos`
from the blob it is handed, with the jitter of the same sample key, so its sample s is the lens render's sample s."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import SCENES, same_bits

f32 = np.float32
RAND_MAX = 2147483647
SEC_LENS = 3
LENS_SCENES = ["lens_spheres", "lens_mesh_small"]
FOCUS_NODE = 1  # both scenes: node 0 is the ground, node 1 the object on the plane of focus


@pytest.fixture
def scene(B):
    """Private scene handles, freed with their device state when the test ends (set_lens changes a scene: nothing shared)."""
    opened = []

    def _load(name):
        path = name if os.path.isabs(name) else os.path.join(SCENES, name + ".xml")
        opened.append(B.Scene(path))
        return opened[-1]
    yield _load
    for sc in opened:
        sc.close()


# ---- include/bhrt_rng.h in numpy (uint32 arithmetic carried in uint64) ---------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x, np.uint64) & M32


def mix32(x):
    x = _u(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def sample_key(seed, pixel, sample):
    return mix32(mix32(_u(seed) * np.uint64(0x9E3779B9) + _u(pixel)) + _u(sample) * np.uint64(0x85EBCA6B) + np.uint64(0x1B873593))


def section_key(key, path_code, section):
    lo, hi = _u(path_code & 0xFFFFFFFF), _u(path_code >> 32)
    k = mix32(_u(key) ^ mix32(lo + np.uint64(0x68E31DA4)))
    k = mix32(k ^ mix32(hi + np.uint64(0xB5297A4D)))
    return mix32(k + _u(section) * np.uint64(0x1B56C4E9) + np.uint64(0x7F4A7C15))


def rand31(key, counter):
    return (mix32(_u(key) ^ mix32(_u(counter) + np.uint64(0x632BE5AB))) >> np.uint64(1)).astype(np.int32)


# ---- the lens model of DESIGN.md 11, float32 in the kernel's order ---------------------------------------------------------------------
def rand_to_unit(O, r):
    return O.math_eval(7, O.MATH_DEVICE, np.ascontiguousarray(r, np.int32).view(f32))


def lens_disc(O, key, R):
    """The aperture point of the samples with keys `key` in the lens plane: (r cos a, r sin a), float32."""
    lkey = section_key(key, 0, SEC_LENS)
    u1, u2 = rand_to_unit(O, rand31(lkey, 0)), rand_to_unit(O, rand31(lkey, 1))
    r = O.math_eval(9, O.MATH_DEVICE, u1) * f32(R)
    a = (f32(np.pi) * f32(2.0)) * u2
    sn, cs = O.math_eval(0, O.MATH_DEVICE, a), O.math_eval(1, O.MATH_DEVICE, a)
    return r * cs, r * sn


def _vec(v):
    return np.array(list(v), f32)


def unit(v):
    n = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])  # vecmath.h: length, normalized
    return (v / n).astype(f32), f32(n)


def lens_rays_ref(O, cam, spp, seed=0, jitter=1, lens_r=0.0, pixels=None):
    """Camera rays of `pixels` ((n, 2) int i, j; default the whole frame, row-major) x spp samples: (o, d, target), each (n, spp, 3) float32.
    lens_r = 0: the pinhole ray of kernels.hip::camera_ray; > 0: the thin-lens ray."""
    W, H = cam.width, cam.height
    if pixels is None:
        jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pixels = np.stack([ii.ravel(), jj.ravel()], axis=1)
    pixels = np.asarray(pixels, np.int64)
    n = len(pixels)
    i = np.repeat(pixels[:, 0], spp)
    j = np.repeat(pixels[:, 1], spp)
    s = np.tile(np.arange(spp), n)
    tl, ddx, ddy, pos = _vec(cam.top_left), _vec(cam.dd_x), _vec(cam.dd_y), _vec(cam.pos)
    target = (tl[None, :] + i.astype(f32)[:, None] * ddx[None, :]) - j.astype(f32)[:, None] * ddy[None, :]
    ux, pixel_len = unit(ddx)
    uy, _ = unit(ddy)
    key = sample_key(seed, j * W + i, s)
    if jitter:
        fx = ((rand31(key, 0).astype(np.float64) / RAND_MAX) * 2 - 1).astype(f32)
        target = target + ((ux[None, :] * fx[:, None]) * pixel_len) / f32(2)
        fy = ((rand31(key, 1).astype(np.float64) / RAND_MAX) * 2 - 1).astype(f32)
        target = target + ((uy[None, :] * fy[:, None]) * pixel_len) / f32(2)
    o = np.broadcast_to(pos, target.shape).astype(f32)
    if lens_r > 0:
        lx, ly = lens_disc(O, key, lens_r)
        off = (ux[None, :] * lx[:, None]) + (uy[None, :] * ly[:, None])
        o = pos[None, :] + off
    d = target - o
    assert o.dtype == f32 and d.dtype == f32 and target.dtype == f32
    return o.reshape(n, spp, 3), d.reshape(n, spp, 3), target.reshape(n, spp, 3)


def with_camera(xml_text, **values):
    """The scene text with <focaldist> / <dof> of its <camera> replaced (or added)."""
    head, cam = xml_text.split("<camera>")
    for tag, v in values.items():
        cam = re.sub(r"\s*<%s [^>]*/>" % tag, "", cam)
        cam = cam.replace("</camera>", '  <%s value="%s"/>\n  </camera>' % (tag, v))
    return head + "<camera>" + cam


def patched_pos(B, blob, pos):
    """The blob with header.camera.pos overwritten: nothing else changes."""
    from bhraytracer_amd.flat import Camera, Header
    off = Header.camera.offset + Camera.pos.offset
    b = bytearray(blob)
    b[off:off + 12] = np.asarray(pos, f32).tobytes()
    return bytes(b)


def pair_grid(W, H):
    """The (pixel, sample) pairs of the radiance test: every fourth pixel of the frame in both directions, samples 0..3 in turn."""
    px = [(i, j, (i // 4 + 2 * (j // 4)) % 4) for j in range(2, H, 4) for i in range(1, W, 4)]
    return np.array(px, np.int64)


def chosen_pairs(O, sc, seed):
    """Pairs, their lens and pinhole rays, and the conditions that keep the radiance test from passing on a lens that does nothing."""
    cam = sc.flat_view().header.camera
    pairs = pair_grid(cam.width, cam.height)
    o, d, _ = lens_rays_ref(O, cam, 4, seed=seed, jitter=1, lens_r=cam.dof, pixels=pairs[:, :2])
    po, pd, _ = lens_rays_ref(O, cam, 4, seed=seed, jitter=1, lens_r=0.0, pixels=pairs[:, :2])
    k = np.arange(len(pairs))
    o, d, po, pd = o[k, pairs[:, 2]], d[k, pairs[:, 2]], po[k, pairs[:, 2]], pd[k, pairs[:, 2]]
    blob = sc.flat_bytes()
    hl, hp = O.trace_closest(blob, o, d, 1), O.trace_closest(blob, po, pd, 1)
    n = len(pairs)
    differs = int(np.sum((hl["node"] != hp["node"]) | (hl["prim"] != hp["prim"])))
    misses = int(np.sum(hl["node"] < 0))
    in_focus = int(np.sum(hl["node"] == FOCUS_NODE))
    print(f"{n} pairs: first hit differs from the pinhole ray's {differs}, miss {misses}, in-focus object {in_focus}")
    assert n >= 256 and (pairs[:, 2] > 0).sum() >= n // 2
    assert differs >= 0.1 * n and misses >= 0.1 * n and in_focus >= 0.1 * n
    return pairs, o, d


# ---- CPU: options, argument checks, set_lens, the restated model ------------------------------------------------------------------------
def test_default_opts_have_the_lens_off(B):
    o = B.default_opts()
    assert o.lens == 0 and C.sizeof(B.Opts) == 64
    assert B.default_opts(lens=1).lens == 1


def test_lens_values_other_than_0_and_1_are_refused_before_the_device(B, scene):
    sc = scene("lens_spheres")
    for call in (lambda o: sc.render(o), lambda o: sc.render_var(o), lambda o: sc.render_samples(o, 0, 0, 4, 4),
                 lambda o: sc.render_adaptive(o, B.default_adaptive_opts(min_spp=2)), lambda o: sc.camera_rays(o)):
        for bad in (2, -1):
            with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*lens"):
                call(B.default_opts(spp=4, lens=bad))


@pytest.mark.parametrize("dof", [-1.0, float("nan"), float("inf")])
def test_set_lens_refuses_a_bad_aperture(B, scene, dof):
    sc = scene("lens_spheres")
    before = sc.flat_bytes()
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*dof"):
        sc.set_lens(dof=dof)
    for fd in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*focaldist"):
            sc.set_lens(focaldist=fd, dof=1.0)
    sc._flat = None
    assert sc.flat_bytes() == before


@pytest.mark.parametrize("dof", ["-1", "nan", "inf"])
def test_lens_on_a_scene_with_a_bad_dof_is_refused_before_the_device(B, scene, dof):
    """set_lens refuses such a value, so the scene gets it from its file."""
    path = os.path.join(SCENES, "_tmp_lens_baddof_%s.xml" % dof.replace("-", "m"))
    try:
        with open(path, "w") as f:
            f.write(with_camera(open(os.path.join(SCENES, "lens_spheres.xml")).read(), dof=dof))
        sc = scene(path)
        got = sc.flat_view().header.camera.dof
        assert not (0 <= got < np.inf), "the loader did not take the value %s" % dof
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*dof"):
            sc.render(B.default_opts(spp=1, lens=1))
    finally:
        if os.path.exists(path):
            os.remove(path)


def test_camera_rays_needs_a_device(B, scene):
    sc = scene("lens_spheres")
    if B.device_count() > 0:
        o, d = sc.camera_rays(B.default_opts(spp=2, lens=1), (0, 0, 8, 4))
        assert o.shape == d.shape == (32, 2, 3)
    else:
        with pytest.raises(B.BhrtError, match=r"bhrt error 4"):
            sc.camera_rays(B.default_opts(spp=2, lens=1))


@pytest.mark.parametrize("name,fd,dof", [
    ("lens_spheres", 25.0, 0.75), ("lens_spheres", 0.0, 2.0), ("lens_spheres", -3.0, 0.0), ("lens_spheres", 41.5, 0.0),
    ("lens_mesh_small", 18.25, 3.0), ("c3_mesh_small", 31.0, 1.0), ("c2_glass_small", 0.0, 0.5),
])
def test_set_lens_gives_the_blob_of_the_edited_scene_file(B, scene, name, fd, dof):
    text = open(os.path.join(SCENES, name + ".xml")).read()
    sc = scene(name)
    current = sc.flat_view().header.camera.focaldist
    sc.set_lens(focaldist=fd, dof=dof)
    path = os.path.join(SCENES, "_tmp_lens_%s_%s_%s.xml" % (name, fd, dof))  # beside the scene: it refers to its mesh by a relative path
    try:
        with open(path, "w") as f:
            f.write(with_camera(text, focaldist=repr(fd if fd > 0 else float(current)), dof=repr(dof)))
        ref = scene(path)
        cam = ref.flat_view().header.camera
        assert cam.dof == f32(dof) and cam.focaldist == (f32(fd) if fd > 0 else current)
        assert sc.flat_bytes() == ref.flat_bytes()
    finally:
        if os.path.exists(path):
            os.remove(path)


def test_set_lens_on_an_authored_scene_with_the_shipped_values(B, scene, tmp_path):
    """proj9.xml's focal distance 70 and aperture 1.5 on a copy of proj1.xml (no file beside it is needed), against the edited text."""
    from conftest import GOLDEN
    data = os.path.join(GOLDEN, "shipped", "Resource", "Data")
    p9 = scene(os.path.join(data, "proj9.xml")).flat_view().header.camera
    assert (p9.focaldist, p9.dof) == (70.0, 1.5)
    text = open(os.path.join(data, "proj1.xml")).read()
    a, b = str(tmp_path / "a.xml"), str(tmp_path / "b.xml")
    open(a, "w").write(text)
    open(b, "w").write(with_camera(text, focaldist="70", dof="1.5"))
    sa, sb = scene(a), scene(b)
    assert sa.flat_bytes() != sb.flat_bytes()
    sa.set_lens(focaldist=70.0, dof=1.5)
    assert sa.flat_bytes() == sb.flat_bytes()


def test_the_restated_lens_samples_the_disc_uniformly(O):
    """65 536 slots.  r^2 / R^2 is uniform on [0, 1]: its mean has the standard error 0.29 / 256 = 0.0011, the bound is five of those.  A
    component of a uniform point of the disc has the standard deviation R / 2: five standard errors of its mean are 5 R / (2 * 256)."""
    R = 1.5
    pixel = np.repeat(np.arange(16384), 4)
    s = np.tile(np.arange(4), 16384)
    lx, ly = lens_disc(O, sample_key(7, pixel, s), R)
    assert lx.dtype == f32 and len(lx) == 65536
    r2 = lx.astype(np.float64) ** 2 + ly.astype(np.float64) ** 2
    print("max r / R", np.sqrt(r2.max()) / R, "mean r^2 / R^2", r2.mean() / R ** 2, "means", lx.mean(dtype=np.float64), ly.mean(dtype=np.float64))
    assert np.sqrt(r2.max()) <= R * (1 + 1e-6)
    assert abs(r2.mean() / R ** 2 - 0.5) <= 0.006
    assert abs(lx.mean(dtype=np.float64)) <= 5 * R / (2 * 256) and abs(ly.mean(dtype=np.float64)) <= 5 * R / (2 * 256)
    # the lens draws are a stream of their own: not the jitter draws of the sample key
    key = sample_key(7, pixel, s)
    assert not np.array_equal(rand31(section_key(key, 0, SEC_LENS), 0), rand31(key, 0))


@pytest.mark.parametrize("name", LENS_SCENES)
def test_the_chosen_pairs_exercise_the_lens(B, O, scene, name):
    """The conditions of the radiance test hold for the oracle alone (no GPU)."""
    chosen_pairs(O, scene(name), seed=9)


def test_oracle_takes_the_camera_position_from_the_blob(B, O, scene):
    """The patched-`pos` recipe on the CPU.  A scene file with another <position> also moves the image plane, so it cannot serve as the
    second opinion; the tracer can: the rays formed by hand from the unpatched frame and the new position (origin P, direction target - P)
    miss the scene exactly where the oracle's render of the patched blob returns the background colour, sample by sample."""
    sc = scene("lens_spheres")
    blob = sc.flat_bytes()
    hdr = sc.flat_view().header
    cam = hdr.camera
    new_pos = _vec(cam.pos) + _vec(cam.up) * f32(4.0)
    region = (8, 20, 88, 50)
    W, H = cam.width, cam.height
    base = O.render(blob, W, H, 2, gi=3, seed=4, region=region)["samples"]
    assert same_bits(O.render(patched_pos(B, blob, _vec(cam.pos)), W, H, 2, gi=3, seed=4, region=region)["samples"], base)
    moved = O.render(patched_pos(B, blob, new_pos), W, H, 2, gi=3, seed=4, region=region)["samples"]
    assert not same_bits(moved, base)
    px = np.array([(i, j) for j in range(region[1], region[3]) for i in range(region[0], region[2])])
    _, _, target = lens_rays_ref(O, cam, 2, seed=4, jitter=1, pixels=px)
    d = (target - new_pos[None, None, :]).reshape(-1, 3)
    hit = O.trace_closest(blob, np.broadcast_to(new_pos, d.shape).astype(f32), d, 1)
    miss = (hit["node"] < 0).reshape(-1, 2)
    is_bg = np.all(moved.view(np.uint32) == _vec(hdr.background.color).view(np.uint32)[None, None, :], axis=2)
    old_miss = np.all(base.view(np.uint32) == _vec(hdr.background.color).view(np.uint32)[None, None, :], axis=2)
    print("misses from the new position", int(miss.sum()), "of", miss.size, "; from the old one", int(old_miss.sum()))
    assert miss.sum() >= 50 and (~miss).sum() >= 50 and (miss != old_miss).sum() >= 50
    assert np.array_equal(is_bg, miss)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("jitter", [1, 0])
@pytest.mark.parametrize("name", LENS_SCENES)
def test_camera_rays_equal_the_restated_model(B, O, scene, name, jitter):
    sc = scene(name)
    sc.upload(0)
    cam = sc.flat_view().header.camera
    assert cam.dof > 0
    o, d = sc.camera_rays(B.default_opts(spp=4, seed=9, jitter=jitter, lens=1))
    ro, rd, _ = lens_rays_ref(O, cam, 4, seed=9, jitter=jitter, lens_r=cam.dof)
    assert same_bits(o, ro) and same_bits(d, rd)
    assert not same_bits(o, np.broadcast_to(_vec(cam.pos), o.shape))
    po, pd = sc.camera_rays(B.default_opts(spp=4, seed=9, jitter=jitter, lens=0))
    qo, qd, _ = lens_rays_ref(O, cam, 4, seed=9, jitter=jitter, lens_r=0.0)
    assert same_bits(po, qo) and same_bits(pd, qd)
    if not jitter:
        oo, od = O.primary_rays(sc.flat_view())
        assert same_bits(po[:, 0], oo) and same_bits(pd[:, 0], od) and same_bits(pd[:, 3], od)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENS_SCENES)
def test_lens_with_a_closed_aperture_is_the_pinhole_render(B, scene, name):
    sc = scene(name)
    sc.set_lens(dof=0.0)
    o0, o1 = B.default_opts(spp=4, seed=3, lens=0), B.default_opts(spp=4, seed=3, lens=1)
    rgb0, rad0, _ = sc.render(o0)
    rgb1, rad1, _ = sc.render(o1)
    assert np.array_equal(rgb0, rgb1) and same_bits(rad0, rad1)
    s0, _ = sc.render_samples(o0, 0, 0, sc.width, sc.height)
    s1, _ = sc.render_samples(o1, 0, 0, sc.width, sc.height)
    assert same_bits(s0, s1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENS_SCENES)
def test_lens_off_renders_the_oracles_pinhole_frame(B, O, scene, name):
    sc = scene(name)
    assert sc.flat_view().header.camera.dof > 0
    gs, _ = sc.render_samples(B.default_opts(spp=2, gi_bounces=3, seed=5, lens=0), 0, 0, sc.width, sc.height)
    ro = O.render(sc.flat_bytes(), sc.width, sc.height, 2, gi=3, seed=5)
    assert same_bits(gs, ro["samples"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENS_SCENES)
def test_lens_radiance_equals_the_oracle_with_the_lens_origin_as_camera_position(B, O, scene, name):
    sc = scene(name)
    W, H = sc.width, sc.height
    pairs, o, d = chosen_pairs(O, sc, seed=9)
    blob = sc.flat_bytes()
    gs, _ = sc.render_samples(B.default_opts(spp=4, gi_bounces=3, seed=9, lens=1), 0, 0, W, H)
    pin, _ = sc.render_samples(B.default_opts(spp=4, gi_bounces=3, seed=9, lens=0), 0, 0, W, H)
    bad, moved = [], 0
    for (i, j, s), org in zip(pairs, o):
        ref = O.render(patched_pos(B, blob, org), W, H, int(s) + 1, gi=3, seed=9, region=(int(i), int(j), int(i) + 1, int(j) + 1), threads=1)["samples"][0, s]
        got = gs[j * W + i, s]
        moved += not same_bits(got, pin[j * W + i, s])
        if not same_bits(got, ref):
            bad.append((int(i), int(j), int(s), got.tolist(), ref.tolist()))
    print(f"{len(pairs)} pairs, {moved} differ from the pinhole render, {len(bad)} differ from the oracle")
    assert not bad, bad[:5]
    assert moved >= len(pairs) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENS_SCENES)
def test_first_hits_of_the_hooks_lens_rays(B, O, scene, name):
    sc = scene(name)
    cam = sc.flat_view().header.camera
    o, d = sc.camera_rays(B.default_opts(spp=4, seed=9, lens=1))
    ro, rd, _ = lens_rays_ref(O, cam, 4, seed=9, lens_r=cam.dof)
    g = sc.trace_closest(o.reshape(-1, 3), d.reshape(-1, 3), B.SIDE_FRONT)
    r = O.trace_closest(sc.flat_bytes(), ro.reshape(-1, 3), rd.reshape(-1, 3), 1)
    assert np.array_equal(g["node"], r["node"]) and np.array_equal(g["prim"], r["prim"]) and same_bits(g["t"], r["t"])


@pytest.mark.gpu
def test_lens_rays_meet_on_the_plane_of_focus(B, scene):
    """Jitter off, 64 spp: the lens rays of a pixel all go through its point on the plane at the focal distance, and fan out behind it."""
    sc = scene("lens_spheres")
    cam = sc.flat_view().header.camera
    fd, R = float(cam.focaldist), float(cam.dof)
    o, d = sc.camera_rays(B.default_opts(spp=64, jitter=0, lens=1))
    o, d = o.astype(np.float64), d.astype(np.float64)
    pos, fwd = _vec(cam.pos).astype(np.float64), _vec(cam.dir).astype(np.float64)
    po, pd = sc.camera_rays(B.default_opts(spp=1, jitter=0, lens=0))
    assert np.all(pd[:, 0].astype(np.float64) @ fwd > 0)  # every pinhole ray hits a plane in front of the camera that faces it
    for dist, check in ((fd, lambda spread: spread.max() <= 1e-4 * fd), (2 * fd, lambda spread: spread.min() > R / 4)):
        t = (dist - (o - pos) @ fwd) / (d @ fwd)  # plane: (p - pos) . fwd = dist
        p = o + t[..., None] * d
        spread = np.linalg.norm(p.max(axis=1) - p.min(axis=1), axis=1)
        print("plane at", dist, "spread of the hit points: min", spread.min(), "max", spread.max())
        assert check(spread)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENS_SCENES)
def test_lens_render_does_not_depend_on_tiles_ranks_or_pass_size(B, scene, name):
    sc = scene(name)
    o = B.default_opts(spp=4, gi_bounces=3, seed=2, lens=1)
    rgb, rad, st = sc.render(o)
    pin, _, _ = sc.render(B.default_opts(spp=4, gi_bounces=3, seed=2, lens=0))
    assert not np.array_equal(rgb, pin)
    assert st.camera_samples == sc.width * sc.height * 4
    # world 3 / tile 16: the union of the ranks' tiles
    urgb, urad = np.zeros_like(rgb), np.zeros_like(rad)
    for r in range(3):
        orr = B.default_opts(spp=4, gi_bounces=3, seed=2, lens=1, rank=r, world_size=3, tile_size=16)
        _check = B.lib().bhrt_render(sc._h, C.byref(orr), urgb.ctypes.data_as(C.c_void_p), urad.ctypes.data_as(C.c_void_p), None)
        assert _check == 0
    assert np.array_equal(urgb, rgb) and same_bits(urad, rad)
    # render_var's radiance is render's
    vrgb, vrad, _ = sc.render_var(o)
    assert np.array_equal(vrgb, rgb) and same_bits(vrad, rad)
    # small passes
    prgb, prad, pst = sc.render(B.default_opts(spp=4, gi_bounces=3, seed=2, lens=1, samples_per_pass=4096))
    assert pst.passes > 1 and np.array_equal(prgb, rgb) and same_bits(prad, rad)
    # a pass that overflows its frame pool and is redone in halves
    sc.knob("frame_cap", 6000)
    try:
        hrgb, hrad, hst = sc.render(o)
    finally:
        sc.knob("frame_cap", 0)
    assert hst.passes > st.passes
    assert np.array_equal(hrgb, rgb) and same_bits(hrad, rad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENS_SCENES)
def test_adaptive_lens_render(B, scene, name):
    sc = scene(name)
    o = B.default_opts(spp=8, gi_bounces=3, seed=5, lens=1)
    rgb, rad, var, cnt, st = sc.render_adaptive(o, B.default_adaptive_opts(min_spp=2, threshold=-1.0))
    urgb, urad, uvar = sc.render_var(o)
    assert (cnt == 8).all() and np.array_equal(rgb, urgb) and same_bits(rad, urad)
    o = B.default_opts(spp=64, gi_bounces=3, seed=11, lens=1)
    rgb, rad, var, cnt, st = sc.render_adaptive(o, B.default_adaptive_opts(min_spp=4, threshold=0.05, floor=0.05))
    levels = sorted(set(np.unique(cnt).tolist()))
    print("counts", {n: int((cnt == n).sum()) for n in levels})
    assert len(levels) > 1 and st.camera_samples == int(cnt.sum())
    for n in levels:
        sel = cnt == n
        urgb, urad, _ = sc.render_var(B.default_opts(spp=n, gi_bounces=3, seed=11, lens=1))
        assert np.array_equal(rgb[sel], urgb[sel]) and same_bits(rad[sel], urad[sel]), n


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENS_SCENES)
def test_set_lens_after_upload_renders_like_a_fresh_scene(B, scene, name):
    text = open(os.path.join(SCENES, name + ".xml")).read()
    sc = scene(name)
    sc.upload(0)
    o = B.default_opts(spp=4, gi_bounces=3, seed=8, lens=1)
    before, _, _ = sc.render(o)
    sc.set_lens(focaldist=24.0, dof=0.6)
    rgb, rad, _ = sc.render(o)
    assert not np.array_equal(rgb, before)
    path = os.path.join(SCENES, "_tmp_lens_fresh_%s.xml" % name)
    try:
        with open(path, "w") as f:
            f.write(with_camera(text, focaldist="24.0", dof="0.6"))
        fresh = scene(path)
        assert fresh.flat_bytes() == sc.flat_bytes()
        frgb, frad, _ = fresh.render(o)
    finally:
        if os.path.exists(path):
            os.remove(path)
    assert np.array_equal(rgb, frgb) and same_bits(rad, frad)
