"""Temporal reprojection: bhrt_reproject carries a frame's light across a camera move, bhrt_temporal_accumulate blends the new
frame's samples into it (csrc/temporal.hip states both stages).

reproject_ref and accumulate_ref below restate the two stages in numpy, float32, in the kernel's operation, tap and sum order, vectorised over
pixels.  A tap that is skipped enters with weight 0 and value 0: it adds +0 to every sum, which is what skipping it does (the sums start at +0
and can never be -0)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENES, have_gpu, same_bits
from test_denoise import _synthetic_xml, _tap, divisor
from test_denoise_sampled import unit

f32 = np.float32
BIG = f32(1e30)
NAN, INF = float("nan"), float("inf")
SNAP = f32(2.0 ** -7)
TOL, THR = 0.02, 0.9                       # the tests' own options: they do not depend on the defaults
MOVE = (1.5, 0.0, 0.5)                     # the translation of the moved-camera cases, same target
TURN = (4.0, 0.0, 0.0)                     # the rotation: the target moved by 4 units
CPU_SCENES = ["c1_sphere_plane", "c2_glass_small", "c3_mesh_small", "c4_textured"]


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(f32)


def project(cur, prev, z):
    """The geometry of stage 1 for every pixel: (x, t, u, v before the snap), NaN / inf where the definition produces them."""
    H, W = z.shape
    pos, tl, ddx, ddy = (np.asarray(cur, f32).reshape(4, 3)[k] for k in range(4))
    ppos, ptl, pddx, pddy = (np.asarray(prev, f32).reshape(4, 3)[k] for k in range(4))
    jj, ii = np.mgrid[0:H, 0:W]
    fi, fj = ii.astype(f32), jj.astype(f32)
    with np.errstate(all="ignore"):
        d = ((tl + fi[..., None] * ddx) - fj[..., None] * ddy) - pos
        x = (pos + d * z[..., None]).astype(f32)
        q = x - ppos
        A = ptl - ppos
        m = cross3(pddx, pddy)
        t = (dot3(q, m) / dot3(A, m)).astype(f32)
        r = q / t[..., None] - A
        u = (dot3(r, pddx) / dot3(pddx, pddx)).astype(f32)
        v = (-(dot3(r, pddy) / dot3(pddy, pddy))).astype(f32)
    return x, t, u, v


def reproject_ref(cur, prev, z, n, pz, pn, pc=None, pl=None, a=None, pa=None, tol=TOL, thr=THR):
    """Stage 1 of csrc/temporal.hip on (H, W[, 3]) float32 arrays.  Returns (history, length, motion, valid, hit-pixel t, u, v)."""
    z, n, pz, pn = (np.asarray(k, f32) for k in (z, n, pz, pn))
    H, W = z.shape
    tol, thr = f32(tol), f32(thr)
    jj, ii = np.mgrid[0:H, 0:W]
    fi, fj = ii.astype(f32), jj.astype(f32)
    miss = z >= BIG
    _, t, u, v = project(cur, prev, z)
    with np.errstate(all="ignore"):
        ok = miss | ((t > 0) & np.isfinite(t))
        ru, rv = np.rint(u), np.rint(v)
        u = np.where(np.abs(u - ru) <= SNAP, ru, u)
        v = np.where(np.abs(v - rv) <= SNAP, rv, v)
        u, v = np.where(miss, fi, u).astype(f32), np.where(miss, fj, v).astype(f32)
        ok = ok & (u >= -1) & (u < W) & (v >= -1) & (v < H)
        us, vs = np.where(ok, u, f32(0)), np.where(ok, v, f32(0))
        f0, g0 = np.floor(us), np.floor(vs)
        fx, fy = us - f0, vs - g0
        ax, ay = f32(1) - fx, f32(1) - fy
        i0, j0 = f0.astype(np.int64), g0.astype(np.int64)
        weights = (ax * ay, fx * ay, ax * fy, fx * fy)
        nu, pnu = unit(n), unit(pn)
        sw, sl, se = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
        e_all = None
        if pc is not None:
            e_all = np.asarray(pc, f32)
            if pa is not None:
                e_all = (e_all / divisor(np.asarray(pa, f32))).astype(f32)
        for k in range(4):
            qi, qj = i0 + (k & 1), j0 + (k >> 1)
            inside = (qi >= 0) & (qi < W) & (qj >= 0) & (qj < H)
            ci, cj = np.clip(qi, 0, W - 1), np.clip(qj, 0, H - 1)
            w = weights[k]
            lq = np.asarray(pl, f32)[cj, ci] if pl is not None else np.ones((H, W), f32)
            zq = pz[cj, ci]
            same = (zq < BIG) & (np.abs(zq - t) <= tol * t) & (dot3(nu, pnu[cj, ci]) >= thr)
            val = ok & (w != 0) & inside & (lq > 0) & np.where(miss, zq >= BIG, same)
            w = np.where(val, w, f32(0)).astype(f32)
            sw = sw + w
            sl = sl + w * np.where(val, lq, f32(0))
            if e_all is not None:
                se = se + w[..., None] * np.where(val[..., None], e_all[cj, ci], f32(0))
        valid = ok & (sw > 0)
        h = (se / sw[..., None]).astype(f32)
        if pa is not None:
            h = (h * divisor(np.asarray(a, f32))).astype(f32)
        history = np.where(valid[..., None], h, f32(0)).astype(f32)
        length = np.where(valid, sl / sw, f32(0)).astype(f32)
        motion = np.where(valid[..., None], np.stack([u - fi, v - fj], -1), f32(0)).astype(f32)
    return history, length, motion, valid, t, u, v


def accumulate_ref(c, cur_samples, h, l, clamp_k=-1.0, max_length=INF):
    """Stage 2 of csrc/temporal.hip.  Returns (out, out_length)."""
    c, h, l = np.asarray(c, f32), np.asarray(h, f32), np.asarray(l, f32)
    nc, ml, ck = f32(cur_samples), f32(max_length), f32(clamp_k)
    has = l > 0
    with np.errstate(all="ignore"):
        if clamp_k >= 0:
            s, m = np.zeros(c.shape, f32), np.zeros(c.shape[:2], f32)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    cq, ok = _tap(c, dx, dy)
                    s = s + np.where(ok[..., None], cq, f32(0))
                    m = m + ok.astype(f32)
            mu = (s / m[..., None]).astype(f32)
            s2 = np.zeros(c.shape, f32)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    cq, ok = _tap(c, dx, dy)
                    e = cq - mu
                    s2 = s2 + np.where(ok[..., None], e * e, f32(0))
            ks = ck * np.sqrt(s2 / m[..., None]).astype(f32)
            h = np.minimum(np.maximum(h, mu - ks), mu + ks).astype(f32)
        lc = np.minimum(l, ml)
        a = nc / (lc + nc)
        out = np.where(has[..., None], h + (c - h) * a[..., None], c).astype(f32)
        ol = np.where(has, np.minimum(lc + nc, ml), np.minimum(nc, ml)).astype(f32)
    return out, ol


def xml_pose(name):
    """(position, target, up) of the <camera> of tests/scenes/<name>.xml"""
    cam = open(os.path.join(SCENES, name + ".xml")).read().split("<camera>")[1]
    out = []
    for tag in ("position", "target", "up"):
        m = re.search(r"<%s ([^>]*)/>" % tag, cam).group(1)
        out.append(tuple(float((re.search(r'%s="([^"]*)"' % k, m) or [0, 0])[1]) for k in "xyz"))
    return out


def moved(pose, dpos=(0, 0, 0), dtarget=(0, 0, 0)):
    pos, target, up = pose
    return tuple(p + d for p, d in zip(pos, dpos)), tuple(p + d for p, d in zip(target, dtarget)), up


def frame_of(cam):
    return np.float32([list(cam.pos), list(cam.top_left), list(cam.dd_x), list(cam.dd_y)])


@pytest.fixture
def scene(B):
    """Private scene handles, freed with their device state when the test ends (set_camera changes a scene: nothing shared)."""
    opened = []

    def _load(name):
        path = name if os.path.isabs(name) else os.path.join(SCENES, name + ".xml")
        opened.append(B.Scene(path))
        return opened[-1]
    yield _load
    for sc in opened:
        sc.close()


_views = {}


def oracle_views(B, O, name):
    """The oracle's first-hit images of the scene's camera and of the camera moved by MOVE: computed once, shared, never written to."""
    if name not in _views:
        sc = B.Scene(os.path.join(SCENES, name + ".xml"))
        try:
            W, H = sc.width, sc.height
            out = []
            for dpos in ((0, 0, 0), MOVE):
                sc.set_camera(*moved(xml_pose(name), dpos))
                z, n, a = O.first_hit(sc.flat_bytes(), W, H)
                out.append((sc.camera_frame(), z.reshape(H, W), n.reshape(H, W, 3), a.reshape(H, W, 3)))
            for view in out:
                for img in view:
                    img.setflags(write=False)
            _views[name] = out
        finally:
            sc.close()
    return _views[name]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("bhrt_scene_get_camera_frame", "bhrt_default_reproject_opts", "bhrt_default_temporal_opts", "bhrt_reproject", "bhrt_reproject_dev",
           "bhrt_temporal_accumulate", "bhrt_temporal_accumulate_dev")


def test_symbols_exported_and_declared(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in SYMBOLS:
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\b(int|void) %s\(" % s, hdr), s


def test_python_wrappers_exist(B):
    for w in ("camera_frame", "reproject", "reproject_dev", "temporal_accumulate", "temporal_accumulate_dev"):
        assert callable(getattr(B.Scene, w))
    assert callable(B.default_reproject_opts) and callable(B.default_temporal_opts)


def test_defaults_are_the_headers_macros(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    macro = lambda k: float(re.search(r"#define %s ([-0-9.e]+)f" % k, hdr).group(1))  # noqa: E731
    r, t = B.default_reproject_opts(), B.default_temporal_opts()
    assert C.sizeof(B.ReprojectOpts) == 32 and C.sizeof(B.TemporalOpts) == 32
    assert f32(r.depth_tolerance) == f32(macro("BHRT_REPROJECT_DEPTH_TOLERANCE")) == f32(B.REPROJECT_DEPTH_TOLERANCE)
    assert f32(r.normal_threshold) == f32(macro("BHRT_REPROJECT_NORMAL_THRESHOLD")) == f32(B.REPROJECT_NORMAL_THRESHOLD)
    assert f32(t.clamp_k) == f32(macro("BHRT_TEMPORAL_CLAMP_K")) == f32(B.TEMPORAL_CLAMP_K)
    assert f32(t.max_length) == f32(macro("BHRT_TEMPORAL_MAX_LENGTH")) == f32(B.TEMPORAL_MAX_LENGTH)
    assert t.gamma == 1 and list(r.reserved) == [0] * 6 and list(t.reserved) == [0] * 5
    assert B.default_reproject_opts(depth_tolerance=0.5).depth_tolerance == 0.5 and B.default_temporal_opts(gamma=0).gamma == 0


def _bad_frame(frame, k, value):
    f = frame.copy()
    f.reshape(-1)[k] = value
    return f


def test_bad_arguments_are_refused_before_the_device(B, load_scene):
    """Every BHRT_ERR_ARG case (error 3) is returned with or without a device: the checks come first."""
    sc = load_scene("c2_glass_small")
    W, H = sc.width, sc.height
    fr = sc.camera_frame()
    z, n3 = np.ones((H, W), f32), np.ones((H, W, 3), f32)
    ok = B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR)
    flat = fr.copy()
    flat[1] = flat[0]                                     # top_left' == pos': A = 0, dot(A, m) == 0
    cases = [
        (ok, None, dict(prev_radiance=n3)),
        (ok, _bad_frame(fr, 0, NAN), dict(prev_radiance=n3)),
        (ok, _bad_frame(fr, 7, INF), dict(prev_radiance=n3)),
        (ok, _bad_frame(fr, 11, -INF), dict(prev_radiance=n3)),
        (B.default_reproject_opts(depth_tolerance=-0.01), fr, dict(prev_radiance=n3)),
        (B.default_reproject_opts(depth_tolerance=INF), fr, dict(prev_radiance=n3)),
        (B.default_reproject_opts(depth_tolerance=NAN), fr, dict(prev_radiance=n3)),
        (B.default_reproject_opts(normal_threshold=NAN), fr, dict(prev_radiance=n3)),
        (ok, flat, dict(prev_radiance=n3)),
        (ok, fr, dict(prev_albedo=n3, want=("length",))),   # albedo' without radiance'
        (ok, fr, dict()),                                   # a history without radiance'
    ]
    for o, f, kw in cases:
        with pytest.raises(B.BhrtError, match="bhrt error 3"):
            sc.reproject(o, f, z, n3, **kw)
    for kw in (dict(cur_samples=0.0), dict(cur_samples=-1.0), dict(cur_samples=NAN), dict(max_length=0.0), dict(max_length=-2.0), dict(max_length=NAN)):
        o = B.default_temporal_opts(clamp_k=-1.0, max_length=kw.get("max_length", INF))
        with pytest.raises(B.BhrtError, match="bhrt error 3"):
            sc.temporal_accumulate(o, n3, kw.get("cur_samples", 4.0), n3, z)
    # what is allowed gets past the checks: a negative or infinite threshold, clamp off, max_length = +inf (without a device: "no device", not error 3)
    for call in (lambda: sc.reproject(B.default_reproject_opts(depth_tolerance=0.0, normal_threshold=-INF), fr, z, n3, n3),
                 lambda: sc.temporal_accumulate(B.default_temporal_opts(clamp_k=-1.0, max_length=INF), n3, 4.0, n3, z)):
        try:
            call()
        except B.BhrtError as e:
            assert "bhrt error 3" not in str(e) and not have_gpu()


def test_camera_frame_is_the_blobs_camera(B, scene):
    sc = scene("c3_mesh_small")
    assert same_bits(sc.camera_frame(), frame_of(sc.flat_view().header.camera))
    before = sc.camera_frame()
    sc.set_camera(*moved(xml_pose("c3_mesh_small"), MOVE))
    assert same_bits(sc.camera_frame(), frame_of(sc.flat_view().header.camera)) and not same_bits(sc.camera_frame(), before)
    sc.set_lens(12.0, 0.25)
    assert same_bits(sc.camera_frame(), frame_of(sc.flat_view().header.camera))


@pytest.mark.parametrize("name", CPU_SCENES)
def test_restatement_static_camera_returns_the_previous_frame(B, O, name):
    (fr, z, n, a), _ = oracle_views(B, O, name)
    rad = np.random.RandomState(1).uniform(0, 2, n.shape).astype(f32)
    h, l, mo, valid, _, _, _ = reproject_ref(fr, fr, z, n, z, n, rad)
    assert valid.all() and same_bits(h, rad) and (l == 1).all() and not mo.any()


@pytest.mark.parametrize("name", CPU_SCENES)
def test_restatement_moved_camera(B, O, name):
    """The camera moved by MOVE with the same target: at least 90 % of the hit pixels find their surface in the previous view, and for each
    of them pos' + t (A + u dd_x' - v dd_y') is the pixel's own surface point x within 1e-4 |x|."""
    (fr0, z0, n0, a0), (fr1, z1, n1, a1) = oracle_views(B, O, name)
    rad = np.random.RandomState(2).uniform(0, 2, n0.shape).astype(f32)
    h, l, mo, valid, t, u, v = reproject_ref(fr1, fr0, z1, n1, z0, n0, rad)
    hit = z1 < BIG
    share = valid[hit].mean()
    print(f"{name}: {share:.1%} of {hit.sum()} hit pixels valid")
    assert share >= 0.9
    x, _, u_hit, v_hit = project(fr1, fr0, z1)
    ppos, ptl, pddx, pddy = (fr0[k].astype(np.float64) for k in range(4))
    m = valid & hit
    x, t64 = x[m].astype(np.float64), t[m, None].astype(np.float64)
    back = lambda uu, vv: ppos + t64 * ((ptl - ppos) + uu[m, None].astype(np.float64) * pddx - vv[m, None].astype(np.float64) * pddy)  # noqa: E731
    # the hit formulas' own u, v: the geometry.  The snap is a design rule on top of it: it moves a tap by up to 2^-7 pixel on purpose, which at
    # the depth t is up to t 2^-7 (|dd_x'| + |dd_y'|) in the world (2.7e-4 on c1's points beside the origin, 30 units from the eye)
    err = np.linalg.norm(back(u_hit, v_hit) - x, axis=-1)
    assert (err <= 1e-4 * np.linalg.norm(x, axis=-1)).all(), float((err / np.linalg.norm(x, axis=-1)).max())
    err = np.linalg.norm(back(u, v) - x, axis=-1)
    snap = t64[:, 0] * 2.0 ** -7 * (np.linalg.norm(pddx) + np.linalg.norm(pddy))
    assert (err <= 1e-4 * np.linalg.norm(x, axis=-1) + snap).all()
    assert (l[valid] == 1).all() and not l[~valid].any() and not h[~valid].any()


def test_restatement_of_the_accumulation():
    rng = np.random.RandomState(3)
    c, h = rng.uniform(0, 1, (9, 11, 3)).astype(f32), rng.uniform(0, 1, (9, 11, 3)).astype(f32)
    l = np.full((9, 11), 12, f32)
    l[2:4] = 0
    out, ol = accumulate_ref(c, 4, h, l)
    assert same_bits(out[2:4], c[2:4]) and (ol[2:4] == 4).all() and (ol[5:] == 16).all()
    assert same_bits(out[5:], (h + (c - h) * f32(0.25))[5:])
    out0, _ = accumulate_ref(c, 4, h, l, clamp_k=0.0)                  # clamp to the mean itself
    mean = np.mean([_tap(c, dx, dy)[0][4, 5] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    assert np.allclose(out0[4, 5], mean + (c[4, 5] - mean) * 0.25, rtol=1e-5)
    assert (accumulate_ref(c, 4, h, l, max_length=8.0)[1] == np.where(l > 0, 8, 4)).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


class Views:
    """Two views of one scene on the GPU: the scene's camera (0) and a moved one (1), with first hits and a 2-spp render of view 0."""

    def __init__(self, B, sc, pose, dpos, dtarget):
        self.sc = sc
        sc.set_camera(*pose)
        self.fr0 = sc.camera_frame()
        self.g0 = sc.first_hit()
        self.rad0 = sc.render(B.default_opts(spp=2, seed=1))[1]
        sc.set_camera(*moved(pose, dpos, dtarget))
        self.fr1 = sc.camera_frame()
        self.g1 = sc.first_hit()


def _check_reproject(B, V, with_albedo, pass_guides, pl):
    (z0, n0, a0), (z1, n1, a1) = V.g0, V.g1
    o = B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR)
    got = V.sc.reproject(o, V.fr0, z0, n0, V.rad0, pl, a0 if with_albedo else None, *((z1, n1, a1 if with_albedo else None) if pass_guides else ()))
    ref = reproject_ref(V.fr1, V.fr0, z1, n1, z0, n0, V.rad0, pl, a1 if with_albedo else None, a0 if with_albedo else None)
    for k, what in enumerate(("history", "length", "motion")):
        assert same_bits(got[k], ref[k]), (what, int((got[k].view(np.uint32) != ref[k].view(np.uint32)).sum()))
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("move", ["static", "translate", "rotate"])
@pytest.mark.parametrize("name", ["c3_mesh_small", "c4_textured", "synthetic"])
def test_kernel_equals_restatement(B, scene, tmp_path, name, move):
    """k_reproject against reproject_ref, bit for bit: with and without albedo images, guides passed in and computed by the call, a random
    length' image with zeros and NULL length'.  The synthetic frame is 97 x 61: neither edge is a multiple of 16, 5917 pixels are no
    multiple of 256."""
    if name == "synthetic":
        sc, pose = scene(_synthetic_xml(tmp_path, 97, 61)), ((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        dpos, dtarget = {"static": ((0, 0, 0), (0, 0, 0)), "translate": ((0.4, 0.1, 0.3), (0, 0, 0)), "rotate": ((0, 0, 0), (0.5, 0.2, 0))}[move]
    else:
        sc, pose = scene(name), xml_pose(name)
        dpos, dtarget = {"static": ((0, 0, 0), (0, 0, 0)), "translate": (MOVE, (0, 0, 0)), "rotate": ((0, 0, 0), TURN)}[move]
    V = Views(B, sc, pose, dpos, dtarget)
    H, W = V.g0[0].shape
    rng = np.random.RandomState(4)
    pl = rng.randint(0, 9, (H, W)).astype(f32)          # zeros included
    assert (pl == 0).any()
    ref = _check_reproject(B, V, False, True, None)
    hit = V.g1[0] < BIG
    print(f"{name} {move}: {ref[3][hit].mean():.1%} of the hit pixels valid, {(np.abs(ref[2]) > 0).any(-1).mean():.1%} moved")
    if move == "static":
        assert ref[3].all() and same_bits(ref[0], V.rad0)
    else:
        assert ref[3][hit].mean() > 0.5 and (ref[2] != np.rint(ref[2])).any()   # bilinear taps take part
    _check_reproject(B, V, True, False, pl)
    _check_reproject(B, V, True, True, None)
    _check_reproject(B, V, False, False, pl)


@pytest.mark.gpu
def test_kernel_on_crafted_inputs(B, scene, tmp_path):
    """z and normals handed in, so that no scene has to produce them: a previous camera behind the points (t <= 0), u in [-1, 0) and
    [W - 1, W), a NaN and a miss in z, a zero normal on either side, tolerance 0."""
    W, H = 97, 61
    sc = scene(_synthetic_xml(tmp_path, W, H))
    cur = sc.camera_frame()
    rng = np.random.RandomState(5)
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    z = np.full((H, W), 1.0, f32)                        # the plane through the camera's target, facing it
    rad = rng.uniform(0, 2, (H, W, 3)).astype(f32)
    pl = rng.randint(1, 9, (H, W)).astype(f32)
    a, pa = rng.uniform(0, 1, (H, W, 3)).astype(f32), rng.uniform(0, 1, (H, W, 3)).astype(f32)

    def check(prev, z, n, pz, pn, tol=TOL, thr=THR):
        o = B.default_reproject_opts(depth_tolerance=tol, normal_threshold=thr)
        got = sc.reproject(o, prev, pz, pn, rad, pl, pa, z, n, a)
        ref = reproject_ref(cur, prev, z, n, pz, pn, rad, pl, a, pa, tol, thr)
        for k in range(3):
            assert same_bits(got[k], ref[k]), k
        return ref

    # the previous camera half a pixel and 0.3 pixel aside: u - i = 0.5 puts u in [-1, 0) at i = 0 and in [W - 1, W) at i = W - 1
    for shift in (0.5, -0.5, 0.3):
        prev = cur.copy()
        prev[0] += f32(shift) * cur[2]
        prev[1] += f32(shift) * cur[2]
        ref = check(prev, z, n, z, n)
        u = ref[5]
        assert ((u >= -1) & (u < 0)).any() or ((u >= W - 1) & (u < W)).any()
        assert ref[3][:, 1:-1].all()
    # a previous camera that looks the same way from beyond the plane: the points lie behind it, t = -1 everywhere
    D = (cur[1] + f32(48) * cur[2] - f32(30) * cur[3]) - cur[0]
    prev = cur.copy()
    prev[0] += f32(2) * D
    prev[1] += f32(2) * D
    ref = check(prev, z, n, z, n)
    assert (ref[4] <= 0).all() and not ref[3].any()
    # a NaN and a miss in z and z', zero normals on either side: exact and half-pixel taps
    for shift in (0.0, 0.5):
        prev = cur.copy()
        prev[0] += f32(shift) * cur[2]
        prev[1] += f32(shift) * cur[2]
        zz, pz, nn, pn = z.copy(), z.copy(), n.copy(), n.copy()
        zz[5, 7], zz[6, 9], zz[7, 11] = NAN, BIG, INF
        pz[20, 30], pz[21, 33], pz[6, 9], pz[8, 40] = NAN, BIG, BIG, f32(2e30)
        zz[30:34, 50:60] = BIG                               # a patch of sky in both views, and one in the current view alone
        pz[30:34, 50:60] = BIG
        zz[40:44, 20:30] = BIG
        nn[10, 10:20] = 0
        pn[12, 10:20] = 0
        nn[14, 10:20] = pn[14, 10:20] = 0
        ref = check(prev, zz, nn, pz, pn)
        assert not ref[3][5, 7] and not ref[3][7, 11] and not ref[3][10, 12] and not ref[3][14, 12] and not ref[3][41, 25]
        assert ref[3][31, 55] and (shift != 0.0 or ref[3][6, 9])
    # tolerance 0: only a previous depth that equals t to the bit passes, and the columns' depths alternate by one ulp
    pz = z.copy()
    pz[:, ::2] = np.nextafter(f32(1), f32(2))
    ref = check(cur, z, n, pz, n, tol=0.0)
    assert not ref[3].all()
    # threshold above 1 refuses everything, -inf accepts any pair of non-NaN normals
    assert not check(cur, z, n, z, n, thr=1.5)[3].any()
    assert check(cur, z, n, z, -n, thr=-INF)[3].all()


@pytest.mark.gpu
@pytest.mark.parametrize("max_length", [8.0, INF])
@pytest.mark.parametrize("clamp_k", [-1.0, 0.0, 1.0, 3.0])
def test_accumulate_kernel_equals_restatement(B, O, scene, tmp_path, clamp_k, max_length):
    """k_temporal_accumulate against accumulate_ref bit for bit, rgb8 included, on a 97 x 61 frame: every edge and corner pixel has a history."""
    W, H = 97, 61
    sc = scene(_synthetic_xml(tmp_path, W, H))
    rng = np.random.RandomState(6)
    c = rng.gamma(2.0, 0.3, (H, W, 3)).astype(f32)
    h = rng.gamma(2.0, 0.3, (H, W, 3)).astype(f32)
    l = rng.uniform(0.5, 20, (H, W)).astype(f32)
    l[rng.uniform(size=(H, W)) < 0.2] = 0
    l[0, :], l[-1, :], l[:, 0], l[:, -1] = 3, 5, 7, 9
    for gamma in (1, 0):
        out, ol, rgb = sc.temporal_accumulate(B.default_temporal_opts(clamp_k=clamp_k, max_length=max_length, gamma=gamma), c, 4.0, h, l)
        ro, rl = accumulate_ref(c, 4.0, h, l, clamp_k, max_length)
        assert same_bits(out, ro) and same_bits(ol, rl)
        assert np.array_equal(rgb, O.color24(ro, gamma))
    assert same_bits(out[l == 0], c[l == 0])
    # no history at all: the frame itself
    out, ol, _ = sc.temporal_accumulate(B.default_temporal_opts(clamp_k=clamp_k, max_length=max_length), c, 4.0)
    assert same_bits(out, c) and (ol == min(4.0, max_length)).all()


@pytest.mark.gpu
def test_static_camera_chain(B, load_scene):
    """Two renders of one view, reprojected and accumulated: the mean of the two frames, every length 2 spp.  On device pointers and a stream."""
    import torch
    sc = load_scene("c3_mesh_small")
    W, H, spp = sc.width, sc.height, 4
    r1 = sc.render(B.default_opts(spp=spp, seed=1))[1]
    r2 = sc.render(B.default_opts(spp=spp, seed=2))[1]
    z, n, _ = sc.first_hit()
    dev = _dev()
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in (("z", z), ("n", n), ("r1", r1), ("r2", r2))}
    t["l"] = torch.full((H, W), float(spp), dtype=torch.float32, device=dev)
    hist, out = (torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
    ln, oln = (torch.zeros((H, W), dtype=torch.float32, device=dev) for _ in range(2))
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    sc.reproject_dev(B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR), sc.camera_frame(), t["z"].data_ptr(), t["n"].data_ptr(), t["r1"].data_ptr(),
                     t["l"].data_ptr(), d_history=hist.data_ptr(), d_length=ln.data_ptr(), stream=s.cuda_stream)
    sc.temporal_accumulate_dev(B.default_temporal_opts(clamp_k=-1.0, max_length=INF), t["r2"].data_ptr(), float(spp), hist.data_ptr(), ln.data_ptr(), out.data_ptr(),
                               oln.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert same_bits(hist.cpu().numpy(), r1) and (ln.cpu().numpy() == spp).all()
    assert same_bits(out.cpu().numpy(), r1 + (r2 - r1) * f32(0.5)) and (oln.cpu().numpy() == 2 * spp).all()


@pytest.mark.gpu
def test_reprojection_quality(B, scene):
    """c3_mesh_small, the camera moved by MOVE: a 64-spp frame of the old view carried into a 4-spp frame of the new one is closer to the new
    view's 256-spp frame than the 4-spp frame alone, over the pixels reprojection marks valid; the others are the 4-spp frame's own bits."""
    sc = scene("c3_mesh_small")
    pose = xml_pose("c3_mesh_small")
    fr0 = sc.camera_frame()
    z0, n0, a0 = sc.first_hit()
    old = sc.render(B.default_opts(spp=64, seed=3))[1]
    sc.set_camera(*moved(pose, MOVE))
    R = sc.render(B.default_opts(spp=256, seed=77))[1]
    A = sc.render(B.default_opts(spp=4, seed=1))[1]
    h, l, _ = sc.reproject(B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR), fr0, z0, n0, old, np.full(z0.shape, 64, f32), a0)
    Bm, ol, _ = sc.temporal_accumulate(B.default_temporal_opts(clamp_k=-1.0, max_length=INF), A, 4.0, h, l)
    valid = l > 0
    mse = lambda x, m: float(np.mean(((x - R) ** 2)[m]))  # noqa: E731
    print(f"valid {valid.mean():.1%}: MSE(A, R) {mse(A, valid):.4g}, MSE(B, R) {mse(Bm, valid):.4g}")
    assert same_bits(Bm[~valid], A[~valid]) and (ol[~valid] == 4).all()
    assert valid.mean() > 0.5
    assert mse(Bm, valid) < mse(A, valid)
