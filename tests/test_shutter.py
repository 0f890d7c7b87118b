"""The camera shutter (bhrt_scene_set_shutter): camera motion blur between the scene's camera (pose 0) and a second pose.

The model is restated below in numpy float32 (shutter_rays_ref), on top of tests/test_lens.py's restatement of the keys, the jitter and the
lens.  The GPU tests hold bhrt_camera_rays equal to it bit for bit, and the per-sample radiance of a shutter render equal to the unmodified
oracle's for a blob whose camera is the frame at that sample's time (pos, top_left, dd_x, dd_y patched; with the lens on, pos is the lens
origin): the oracle renders whatever camera the blob holds, with the jitter of the same sample key."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits
from test_camera import edited_scene
from test_guides import crop, z_and_coverage
from test_lens import _vec, lens_disc, pair_grid, rand31, rand_to_unit, sample_key, section_key, RAND_MAX

f32 = np.float32
SEC_SHUTTER = 4
SEED = 9
NAN, INF = float("nan"), float("inf")

# name -> (pos1, target1, up1).  Every scene's camera is at (0, -30, 10) with up (0, 0, 1); a pixel at the focal distance is 0.17 units wide.
# "translate": position and target move by the same vector, whose components and sums are exact in float32, so dir, up and with them
# dd_x, dd_y are pose 0's bit for bit (asserted): about ten pixels sideways and four up.  "rotate": a move plus a turn and a roll.
TRANSLATE = (1.75, 0.5, 0.75)
TARGET0 = {"lens_spheres": (0.0, 0.0, 4.5), "lens_mesh_small": (0.0, 0.0, 5.0), "shutter_plain": (0.0, 0.0, 4.0)}


def pose1(name, kind):
    t0 = TARGET0[name]
    if kind == "translate":
        return (tuple(a + b for a, b in zip((0.0, -30.0, 10.0), TRANSLATE)), tuple(a + b for a, b in zip(t0, TRANSLATE)), (0.0, 0.0, 1.0))
    if kind == "same":
        return ((0.0, -30.0, 10.0), t0, (0.0, 0.0, 1.0))
    return ((2.0, -29.0, 11.0), (t0[0] - 1.5, t0[1], t0[2] + 0.5), (0.06, 0.0, 1.0))


CASES = [("lens_spheres", "translate"), ("lens_mesh_small", "translate"), ("shutter_plain", "rotate")]


@pytest.fixture
def scene(B):
    """Private scene handles, freed with their device state when the test ends (the setters change a scene: nothing shared)."""
    opened = []

    def _load(name, kind=None):
        path = name if os.path.isabs(name) else os.path.join(SCENES, name + ".xml")
        opened.append(B.Scene(path))
        if kind is not None:
            opened[-1].set_shutter(True, *pose1(name, kind))
        return opened[-1]
    yield _load
    for sc in opened:
        sc.close()


# ---- the model of DESIGN.md 18, float32 in the kernel's order -----------------------------------------------------------------------------
def shutter_time(O, key):
    return rand_to_unit(O, rand31(section_key(key, 0, SEC_SHUTTER), 0))


def units(v):
    """vecmath.h's length and normalized of the rows of v (n, 3) float32."""
    n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    assert n.dtype == f32
    return (v / n[:, None]).astype(f32), n


def shutter_rays_ref(O, cam, frame1, spp, seed=0, jitter=1, lens_r=0.0, pixels=None):
    """Camera rays of `pixels` ((n, 2) int i, j; default the whole frame, row-major) x spp samples with the shutter between cam (pose 0) and
    frame1 ((4, 3): pos1, top_left1, dd_x1, dd_y1).  Returns (o, d, t, frame): (n, spp, 3) twice, (n, spp) and (n, spp, 4, 3) float32, frame =
    the interpolated pos, top_left, dd_x, dd_y of every sample."""
    W, H = cam.width, cam.height
    if pixels is None:
        jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pixels = np.stack([ii.ravel(), jj.ravel()], axis=1)
    pixels = np.asarray(pixels, np.int64)
    n = len(pixels)
    i = np.repeat(pixels[:, 0], spp)
    j = np.repeat(pixels[:, 1], spp)
    s = np.tile(np.arange(spp), n)
    key = sample_key(seed, j * W + i, s)
    t = shutter_time(O, key)
    assert t.dtype == f32
    X0 = np.stack([_vec(cam.pos), _vec(cam.top_left), _vec(cam.dd_x), _vec(cam.dd_y)])
    X1 = np.ascontiguousarray(frame1, f32).reshape(4, 3)
    Xt = X0[None] + (X1 - X0)[None] * t[:, None, None]
    assert Xt.dtype == f32
    pos, tl, ddx, ddy = Xt[:, 0], Xt[:, 1], Xt[:, 2], Xt[:, 3]
    ux, pixel_len = units(ddx)
    uy, _ = units(ddy)
    target = (tl + i.astype(f32)[:, None] * ddx) - j.astype(f32)[:, None] * ddy
    if jitter:
        fx = ((rand31(key, 0).astype(np.float64) / RAND_MAX) * 2 - 1).astype(f32)
        target = target + ((ux * fx[:, None]) * pixel_len[:, None]) / f32(2)
        fy = ((rand31(key, 1).astype(np.float64) / RAND_MAX) * 2 - 1).astype(f32)
        target = target + ((uy * fy[:, None]) * pixel_len[:, None]) / f32(2)
    o = pos
    if lens_r > 0:
        lx, ly = lens_disc(O, key, lens_r)
        o = pos + ((ux * lx[:, None]) + (uy * ly[:, None]))
    d = target - o
    assert o.dtype == f32 and d.dtype == f32
    return o.reshape(n, spp, 3), d.reshape(n, spp, 3), t.reshape(n, spp), Xt.reshape(n, spp, 4, 3)


def frame_of(cam):
    return np.stack([_vec(cam.pos), _vec(cam.top_left), _vec(cam.dd_x), _vec(cam.dd_y)])


def patched_frame(blob, pos, frame):
    """The blob with header.camera.pos, top_left, dd_x, dd_y overwritten (pos on its own: the lens origin where the lens is on)."""
    from bhraytracer_amd.flat import Camera, Header
    b = bytearray(blob)
    base = Header.camera.offset
    for field, v in ((Camera.pos, pos), (Camera.top_left, frame[1]), (Camera.dd_x, frame[2]), (Camera.dd_y, frame[3])):
        b[base + field.offset:base + field.offset + 12] = np.asarray(v, f32).tobytes()
    return bytes(b)


def chosen_pairs(O, sc, lens):
    """Pairs, their shutter rays and frames, and the conditions that keep the radiance test from passing on a shutter that does nothing."""
    cam = sc.flat_view().header.camera
    on, _, frame1 = sc.shutter()
    assert on
    pairs = pair_grid(cam.width, cam.height)
    lens_r = float(cam.dof) if lens else 0.0
    o, d, t, fr = shutter_rays_ref(O, cam, frame1, 4, seed=SEED, jitter=1, lens_r=lens_r, pixels=pairs[:, :2])
    po, pd, _, _ = shutter_rays_ref(O, cam, frame_of(cam), 4, seed=SEED, jitter=1, lens_r=lens_r, pixels=pairs[:, :2])
    k = np.arange(len(pairs))
    o, d, fr, po, pd = o[k, pairs[:, 2]], d[k, pairs[:, 2]], fr[k, pairs[:, 2]], po[k, pairs[:, 2]], pd[k, pairs[:, 2]]
    blob = sc.flat_bytes()
    hs, hp = O.trace_closest(blob, o, d, 1), O.trace_closest(blob, po, pd, 1)
    n = len(pairs)
    differs = int(np.sum((hs["node"] != hp["node"]) | (hs["prim"] != hp["prim"])))
    misses = int(np.sum(hs["node"] < 0))
    objects = int(np.sum(hs["node"] > 0))  # node 0 is the ground in every scene
    print(f"{n} pairs: first hit differs from the pose-0 ray's {differs}, miss {misses}, hit an object {objects}")
    assert n >= 256 and (pairs[:, 2] > 0).sum() >= n // 2
    assert differs >= 0.1 * n and misses >= 0.1 * n and objects >= 0.1 * n
    return pairs, o, d, fr


# ---- CPU: the state, the argument checks, the restated model ------------------------------------------------------------------------------
def test_the_shutter_is_off_by_default_and_leaves_the_blob_alone(B, scene):
    sc = scene("lens_mesh_small")
    before = sc.flat_bytes()
    on, pose, frame = sc.shutter()
    assert not on and not pose.any() and not frame.any()
    sc.set_shutter(True, *pose1("lens_mesh_small", "rotate"))
    on, pose, frame = sc.shutter()
    assert on and same_bits(pose, np.array(pose1("lens_mesh_small", "rotate"), f32))
    sc._flat = None
    assert sc.flat_bytes() == before
    sc.set_shutter(False)  # the pointers may be NULL
    on, pose, frame = sc.shutter()
    assert not on and not pose.any() and not frame.any()
    sc._flat = None
    assert sc.flat_bytes() == before


@pytest.mark.parametrize("name,kind", CASES + [("shutter_plain", "translate")])
def test_pose_1_is_the_frame_of_the_edited_scene_file(B, scene, name, kind):
    """... with the scene's fov, focaldist and size; a translation keeps dd_x, dd_y bit for bit, the rotation does not."""
    sc = scene(name, kind)
    p1 = pose1(name, kind)
    with edited_scene(name, "pose1" + kind, position=p1[0], target=p1[1], up=p1[2]) as path:
        cam1 = scene(path).flat_view().header.camera
    _, _, frame1 = sc.shutter()
    assert same_bits(frame1, frame_of(cam1))
    cam0 = sc.flat_view().header.camera
    same_axes = same_bits(frame1[2:], frame_of(cam0)[2:])
    assert same_axes == (kind == "translate")
    assert not same_bits(frame1[:2], frame_of(cam0)[:2])
    if kind == "rotate":
        assert sc.info.n_textures == 0
    else:
        assert sc.info.n_textures >= 1 or name == "shutter_plain"


def test_pose_1_follows_set_lens_and_set_camera(B, scene):
    sc = scene("lens_spheres", "rotate")
    p1 = pose1("lens_spheres", "rotate")
    _, _, before = sc.shutter()
    sc.set_lens(focaldist=24.0, dof=0.5)
    _, pose, after = sc.shutter()
    assert same_bits(pose, np.array(p1, f32)) and not same_bits(after[1:], before[1:]) and same_bits(after[0], before[0])
    with edited_scene("lens_spheres", "follow", position=p1[0], target=p1[1], up=p1[2]) as path:
        ref = scene(path)
        ref.set_lens(focaldist=24.0, dof=0.5)
        assert same_bits(after, frame_of(ref.flat_view().header.camera))
    sc.set_camera((0.5, -29.0, 10.0), (0.0, 0.0, 4.0), (0.0, 0.0, 1.0), 41.0)  # a new fov: pose 1 takes it
    _, pose, wide = sc.shutter()
    with edited_scene("lens_spheres", "follow2", position=p1[0], target=p1[1], up=p1[2], fov=41.0) as path:
        ref = scene(path)
        ref.set_lens(focaldist=24.0, dof=0.5)
        assert same_bits(wide, frame_of(ref.flat_view().header.camera))
    assert same_bits(pose, np.array(p1, f32))


def test_a_clone_carries_the_shutter(B, scene):
    sc = scene("shutter_plain", "rotate")
    other = sc.clone()
    try:
        a, b = sc.shutter(), other.shutter()
        assert b[0] and same_bits(a[1], b[1]) and same_bits(a[2], b[2])
        assert other.flat_bytes() == sc.flat_bytes()
    finally:
        other.close()


P0, T0, U0 = (0.0, -30.0, 10.0), (0.0, 0.0, 4.0), (0.0, 0.0, 1.0)
BAD_POSES = [
    ((NAN, 0, 0), T0, U0, "finite"), (P0, (0, 0, INF), U0, "finite"), (P0, T0, (0, -INF, 0), "finite"),
    ((1, 2, 3), (1, 2, 3), U0, "target == pos"), ((0, -30, 0), (0, 0, 0), (0, 3, 0), "parallel"),
    (None, T0, U0, "NULL"), (P0, None, U0, "NULL"), (P0, T0, None, "NULL"),
    ((0.0, 30.0, 10.0), T0, U0, "quarter turn"),          # looks the other way: dir0 . dir1 <= 0
    ((30.0, 0.0, 4.0), T0, U0, "quarter turn"),           # a quarter turn about the vertical: dir0 . dir1 = 0 or dd_x0 . dd_x1 <= 0
    (P0, T0, (0.0, 0.0, -1.0), "quarter turn"),           # upside down: dd_x and dd_y flip
    (P0, T0, (1.0, 0.0, 0.0), "quarter turn"),            # rolled a quarter turn: dd_y0 . dd_y1 = 0
]


@pytest.mark.parametrize("pos,target,up,what", BAD_POSES)
def test_set_shutter_refuses_bad_poses_and_changes_nothing(B, scene, pos, target, up, what):
    import re
    sc = scene("shutter_plain")  # never uploaded
    before = sc.flat_bytes()
    for armed in (False, True):
        if armed:
            sc.set_shutter(True, *pose1("shutter_plain", "translate"))
        state = sc.shutter()
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: bhrt_scene_set_shutter: .*" + re.escape(what)):
            sc.set_shutter(True, pos, target, up)
        now = sc.shutter()
        assert now[0] == state[0] and same_bits(now[1], state[1]) and same_bits(now[2], state[2])
        sc._flat = None
        assert sc.flat_bytes() == before


def test_set_camera_checks_the_pair_while_a_shutter_is_on(B, scene):
    sc = scene("shutter_plain", "translate")
    before, state = sc.flat_bytes(), sc.shutter()
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: bhrt_scene_set_camera: .*quarter turn"):
        sc.set_camera((0.0, 30.0, 10.0), T0, U0, 0.0)
    now = sc.shutter()
    sc._flat = None
    assert sc.flat_bytes() == before and now[0] and same_bits(now[1], state[1]) and same_bits(now[2], state[2])
    sc.set_shutter(False)
    sc.set_camera((0.0, 30.0, 10.0), T0, U0, 0.0)  # fine without a shutter
    sc._flat = None
    assert sc.flat_bytes() != before


def test_the_restated_time_is_uniform_on_the_unit_interval(O):
    """8192 keys.  A uniform t has mean 1 / 2 with standard error 0.2887 / sqrt(8192) = 0.0032 and variance 1 / 12 whose estimate has the standard
    error sqrt(1 / 180 / 8192) = 0.00082: the bounds are five of each."""
    pixel = np.repeat(np.arange(2048), 4)
    s = np.tile(np.arange(4), 2048)
    key = sample_key(7, pixel, s)
    t = shutter_time(O, key).astype(np.float64)
    print("t: min", t.min(), "max", t.max(), "mean", t.mean(), "variance", t.var())
    assert len(t) == 8192 and t.min() >= 0.0 and t.max() < 1.0
    assert abs(t.mean() - 0.5) <= 5 * 0.0032 and abs(t.var() - 1 / 12) <= 5 * 0.00082
    # a stream of its own: neither the jitter's draws nor the lens's
    assert not np.array_equal(rand31(section_key(key, 0, SEC_SHUTTER), 0), rand31(key, 0))
    assert not np.array_equal(rand31(section_key(key, 0, SEC_SHUTTER), 0), rand31(section_key(key, 0, 3), 0))


def test_equal_poses_restate_the_lens_model(B, O, scene):
    from test_lens import lens_rays_ref
    cam = scene("lens_spheres").flat_view().header.camera
    for lens_r in (0.0, float(cam.dof)):
        o, d, _, _ = shutter_rays_ref(O, cam, frame_of(cam), 2, seed=3, lens_r=lens_r)
        lo, ld, _ = lens_rays_ref(O, cam, 2, seed=3, lens_r=lens_r)
        assert same_bits(o, lo) and same_bits(d, ld)


def test_oracle_takes_the_camera_frame_from_the_blob(B, O, scene):
    """1 x 1 regions of the blob with pos, top_left, dd_x, dd_y patched to pose 1's differ from the unpatched ones and equal those of the scene
    file that yields that frame."""
    name = "shutter_plain"
    sc = scene(name, "rotate")
    p1 = pose1(name, "rotate")
    _, _, frame1 = sc.shutter()
    blob = sc.flat_bytes()
    with edited_scene(name, "oracle", position=p1[0], target=p1[1], up=p1[2]) as path:
        ref_blob = scene(path).flat_bytes()
    patched = patched_frame(blob, frame1[0], frame1)
    W, H = sc.width, sc.height
    differ = 0
    for (i, j) in [(10, 30), (40, 36), (48, 50), (70, 40), (30, 60), (60, 20), (85, 65), (20, 44)]:
        region = (i, j, i + 1, j + 1)
        a = O.render(patched, W, H, 3, gi=3, seed=4, region=region, threads=1)["samples"]
        b = O.render(ref_blob, W, H, 3, gi=3, seed=4, region=region, threads=1)["samples"]
        c = O.render(blob, W, H, 3, gi=3, seed=4, region=region, threads=1)["samples"]
        assert same_bits(a, b)
        differ += not same_bits(a, c)
    assert differ >= 6


@pytest.mark.parametrize("lens", [0, 1])
@pytest.mark.parametrize("name,kind", CASES)
def test_the_chosen_pairs_exercise_the_shutter(B, O, scene, name, kind, lens):
    """The conditions of the radiance test hold for the oracle alone (no GPU)."""
    chosen_pairs(O, scene(name, kind), lens)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lens", [0, 1])
@pytest.mark.parametrize("jitter", [1, 0])
@pytest.mark.parametrize("name,kind", CASES)
def test_camera_rays_equal_the_restated_model(B, O, scene, name, kind, jitter, lens):
    sc = scene(name, kind)
    sc.upload(0)
    cam = sc.flat_view().header.camera
    assert cam.dof > 0
    _, _, frame1 = sc.shutter()
    o, d = sc.camera_rays(B.default_opts(spp=4, seed=SEED, jitter=jitter, lens=lens))
    ro, rd, _, _ = shutter_rays_ref(O, cam, frame1, 4, seed=SEED, jitter=jitter, lens_r=float(cam.dof) if lens else 0.0)
    assert same_bits(o, ro) and same_bits(d, rd)
    assert not same_bits(o, np.broadcast_to(_vec(cam.pos), o.shape))
    sc.set_shutter(False)  # an uploaded scene: the device's copy follows
    po, pd = sc.camera_rays(B.default_opts(spp=4, seed=SEED, jitter=jitter, lens=lens))
    qo, qd, _, _ = shutter_rays_ref(O, cam, frame_of(cam), 4, seed=SEED, jitter=jitter, lens_r=float(cam.dof) if lens else 0.0)
    assert same_bits(po, qo) and same_bits(pd, qd) and not same_bits(pd, d)


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [0, 1])
@pytest.mark.parametrize("name", ["lens_spheres", "lens_mesh_small", "shutter_plain"])
def test_equal_poses_render_the_frame_without_a_shutter(B, scene, name, lens):
    off, on = scene(name), scene(name, "same")
    cam = off.flat_view().header.camera
    assert same_bits(on.shutter()[2], frame_of(cam))
    o = B.default_opts(spp=4, gi_bounces=3, seed=3, lens=lens)
    rgb0, rad0, _ = off.render(o)
    rgb1, rad1, _ = on.render(o)
    assert np.array_equal(rgb0, rgb1) and same_bits(rad0, rad1)
    s0, _ = off.render_samples(o, 0, 0, off.width, off.height)
    s1, _ = on.render_samples(o, 0, 0, on.width, on.height)
    assert same_bits(s0, s1)
    g0, g1 = off.guides(o), on.guides(o)
    for k in g0:
        assert same_bits(g0[k], g1[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [0, 1])
@pytest.mark.parametrize("name,kind", CASES)
def test_shutter_radiance_equals_the_oracle_with_the_frame_at_the_samples_time(B, O, scene, name, kind, lens):
    sc = scene(name, kind)
    W, H = sc.width, sc.height
    cam = sc.flat_view().header.camera
    same_axes = same_bits(sc.shutter()[2][2:], frame_of(cam)[2:])
    assert same_axes if kind == "translate" else sc.info.n_textures == 0  # a plane's texture footprint reads pose 0's dd_x, dd_y
    pairs, o, d, fr = chosen_pairs(O, sc, lens)
    blob = sc.flat_bytes()
    opts = B.default_opts(spp=4, gi_bounces=3, seed=SEED, lens=lens)
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    sc.set_shutter(False)
    still, _ = sc.render_samples(opts, 0, 0, W, H)
    bad, moved = [], 0
    for (i, j, s), org, f in zip(pairs, o, fr):
        ref = O.render(patched_frame(blob, org, f), W, H, int(s) + 1, gi=3, seed=SEED, region=(int(i), int(j), int(i) + 1, int(j) + 1), threads=1)["samples"][0, s]
        got = gs[j * W + i, s]
        moved += not same_bits(got, still[j * W + i, s])
        if not same_bits(got, ref):
            bad.append((int(i), int(j), int(s), got.tolist(), ref.tolist()))
    print(f"{len(pairs)} pairs, {moved} differ from the render without a shutter, {len(bad)} differ from the oracle")
    assert not bad, bad[:5]
    assert moved >= len(pairs) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [0, 1])
@pytest.mark.parametrize("name,kind", CASES)
def test_first_hits_and_guides_of_the_shutter_rays(B, O, scene, name, kind, lens):
    """First hits of the hook's rays equal the oracle's; bhrt_guides' z and coverage are tests/test_guides.py's fold of the oracle's hits of the
    restated rays."""
    sc = scene(name, kind)
    cam = sc.flat_view().header.camera
    opts = B.default_opts(spp=5, seed=SEED, lens=lens)
    o, d = sc.camera_rays(opts)
    ro, rd, _, _ = shutter_rays_ref(O, cam, sc.shutter()[2], 5, seed=SEED, lens_r=float(cam.dof) if lens else 0.0)
    g = sc.trace_closest(o.reshape(-1, 3), d.reshape(-1, 3), B.SIDE_FRONT)
    r = O.trace_closest(sc.flat_bytes(), ro.reshape(-1, 3), rd.reshape(-1, 3), 1)
    assert np.array_equal(g["node"], r["node"]) and np.array_equal(g["prim"], r["prim"]) and same_bits(g["t"], r["t"])
    z, cov, k = z_and_coverage(O, sc.flat_bytes(), ro, rd)
    partial = int(((k > 0) & (k < 5)).sum())
    print(f"{partial} pixels hit partly, {int((k == 0).sum())} miss, {int((k == 5).sum())} hit with every sample")
    assert partial >= 10 and (k == 0).sum() >= 10 and (k == 5).sum() >= 10
    whole = (0, 0, sc.width, sc.height)
    gd = sc.guides(opts)
    assert same_bits(crop(gd["coverage"], whole)[:, 0], cov) and same_bits(crop(gd["z"], whole)[:, 0], z)
    sc.set_shutter(False)
    assert not same_bits(sc.guides(opts, want=("z",))["z"], gd["z"])


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [0, 1])
@pytest.mark.parametrize("name,kind", [("lens_mesh_small", "translate"), ("shutter_plain", "rotate")])
def test_shutter_render_does_not_depend_on_tiles_ranks_or_pass_size(B, scene, name, kind, lens):
    sc = scene(name, kind)
    kw = dict(spp=4, gi_bounces=3, seed=2, lens=lens)
    o = B.default_opts(**kw)
    rgb, rad, st = sc.render(o)
    assert st.camera_samples == sc.width * sc.height * 4
    urgb, urad = np.zeros_like(rgb), np.zeros_like(rad)
    for r in range(3):  # world 3 / tile 16: the union of the ranks' tiles
        orr = B.default_opts(rank=r, world_size=3, tile_size=16, **kw)
        assert B.lib().bhrt_render(sc._h, C.byref(orr), urgb.ctypes.data_as(C.c_void_p), urad.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(urgb, rgb) and same_bits(urad, rad)
    trgb, trad, _ = sc.render(B.default_opts(tile_size=8, **kw))
    assert np.array_equal(trgb, rgb) and same_bits(trad, rad)
    vrgb, vrad, _ = sc.render_var(o)
    assert np.array_equal(vrgb, rgb) and same_bits(vrad, rad)
    prgb, prad, pst = sc.render(B.default_opts(samples_per_pass=4096, **kw))
    assert pst.passes > 1 and np.array_equal(prgb, rgb) and same_bits(prad, rad)
    sc.knob("frame_cap", 6000)  # a pass that overflows its frame pool and is redone in halves: its rays are formed again
    try:
        hrgb, hrad, hst = sc.render(o)
    finally:
        sc.knob("frame_cap", 0)
    assert hst.passes > st.passes
    assert np.array_equal(hrgb, rgb) and same_bits(hrad, rad)
    sc.set_shutter(False)
    assert not np.array_equal(sc.render(o)[0], rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,lens", [("lens_mesh_small", "translate", 1), ("shutter_plain", "rotate", 0)])
def test_adaptive_shutter_render_is_the_uniform_render_at_each_pixels_count(B, scene, name, kind, lens):
    sc = scene(name, kind)
    o = B.default_opts(spp=64, gi_bounces=3, seed=11, lens=lens)
    rgb, rad, var, cnt, st = sc.render_adaptive(o, B.default_adaptive_opts(min_spp=4, threshold=0.05, floor=0.05))
    levels = sorted(set(np.unique(cnt).tolist()))
    print("counts", {n: int((cnt == n).sum()) for n in levels})
    assert len(levels) > 1 and st.camera_samples == int(cnt.sum())
    for n in levels:
        sel = cnt == n
        urgb, urad, _ = sc.render_var(B.default_opts(spp=n, gi_bounces=3, seed=11, lens=lens))
        assert np.array_equal(rgb[sel], urgb[sel]) and same_bits(rad[sel], urad[sel]), n


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,lens", [("lens_mesh_small", "translate", 0), ("shutter_plain", "rotate", 1)])
def test_a_progressive_session_is_the_render_at_its_count(B, scene, name, kind, lens):
    sc = scene(name, kind)
    o = B.default_opts(spp=4, gi_bounces=3, seed=6, lens=lens)
    sc.progressive_begin(o)
    try:
        for c, step in ((1, 1), (3, 2), (4, 1)):
            sc.progressive_step(step)
            prgb, prad, _, pcnt = sc.progressive_frame()
            rgb, rad, _ = sc.render(B.default_opts(spp=c, gi_bounces=3, seed=6, lens=lens))
            assert (pcnt == c).all() and np.array_equal(prgb, rgb) and same_bits(prad, rad), c
    finally:
        sc.progressive_end()
