"""Reprojection through object motion: bhrt_reproject_moving carries a frame's light across a move of the scene's nodes as well
as of its camera (csrc/temporal.hip states stage 1M beside stage 1).

reproject_moving_ref restates the stage in numpy, float32, in the kernel's operation, tap and sum order, with the helpers of test_reproject's
restatement of stage 1; with nothing moved it must equal that restatement bit for bit, which ties the two together."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENES, have_gpu, same_bits
from test_denoise import divisor
from test_denoise_sampled import unit
from test_reproject import BIG, SNAP, THR, TOL, cross3, dot3, moved as moved_pose, reproject_ref, xml_pose

f32 = np.float32
NAN, INF = float("nan"), float("inf")
INT32_MAX = 2 ** 31 - 1
# The moves of the two authored cases.  The ball of c1_sphere_plane is 6 units wide; its translation is 1.25 units long, under a quarter of that.
BALL_MOVE = (1.0, 0.0, 0.75)
PARENT_TURN = (0.0, 0.0, 1.0, 6.0)          # the parent of moving_nested rotated by 6 degrees about the world's z axis: its children follow
CAMERA_MOVE = (0.75, 0.0, 0.5)              # the camera's translation of the "camera and object both moved" cases
BALL_FLOOR = 0.9                            # the issue's condition on c1's ball
NESTED_FLOOR = 0.9829                       # what the restatement gives on the oracle's images of moving_nested: 461 of 469 pixels


def mat_mul(m, p):
    return np.stack([(p[..., 0] * m[0] + p[..., 1] * m[3]) + p[..., 2] * m[6], (p[..., 0] * m[1] + p[..., 1] * m[4]) + p[..., 2] * m[7],
                     (p[..., 0] * m[2] + p[..., 1] * m[5]) + p[..., 2] * m[8]], -1).astype(f32)


def mat_tmul(m, d):
    return np.stack([(m[0] * d[..., 0] + m[1] * d[..., 1]) + m[2] * d[..., 2], (m[3] * d[..., 0] + m[4] * d[..., 1]) + m[5] * d[..., 2],
                     (m[6] * d[..., 0] + m[7] * d[..., 1]) + m[8] * d[..., 2]], -1).astype(f32)


def moved_nodes(parents, xf, pxf):
    """moved[k]: the 84 bytes of node k's record, or of an ancestor's, differ between the snapshot and the scene."""
    out = np.zeros(len(parents), bool)
    for k, p in enumerate(parents):                 # pre-order: a parent comes first
        out[k] = (p >= 0 and out[p]) or xf[k].tobytes() != pxf[k].tobytes()
    return out


def chain_of(parents, k):
    c = []
    while k >= 0:
        c.insert(0, k)
        k = parents[k]
    return c                                        # the depth-1 ancestor first, k last


def reproject_moving_ref(cur, prev, parents, xf, pxf, z, n, ids, pz, pn, pc=None, pl=None, a=None, pa=None, pid=None, tol=TOL, thr=THR):
    """Stage 1M of csrc/temporal.hip on (H, W[, 3]) arrays.  parents: the nodes' parent indices; xf, pxf: the scene's and the previous records
    (XFORM_DTYPE).  Returns (history, length, motion, valid, t, u, v) as reproject_ref does."""
    z, n, pz, pn = (np.asarray(k, f32) for k in (z, n, pz, pn))
    ids = np.asarray(ids, np.int32)
    H, W = z.shape
    tol, thr = f32(tol), f32(thr)
    n_nodes = len(parents)
    jj, ii = np.mgrid[0:H, 0:W]
    fi, fj = ii.astype(f32), jj.astype(f32)
    miss = z >= BIG
    pos, tl, ddx, ddy = (np.asarray(cur, f32).reshape(4, 3)[k] for k in range(4))
    ppos, ptl, pddx, pddy = (np.asarray(prev, f32).reshape(4, 3)[k] for k in range(4))
    mv = moved_nodes(parents, xf, pxf)
    with np.errstate(all="ignore"):
        d = ((tl + fi[..., None] * ddx) - fj[..., None] * ddy) - pos
        x = (pos + d * z[..., None]).astype(f32)
        nl = n.copy()
        known = (ids >= 0) & (ids < n_nodes)
        for k in range(n_nodes):
            m = ~miss & known & (ids == k)
            if not mv[k] or not m.any():
                continue
            p, q = x[m], nl[m]
            chain = chain_of(parents, k)
            for c in chain:
                p = mat_mul(xf[c]["itm"], p - xf[c]["pos"])
                q = mat_tmul(xf[c]["tm"], q)
            for c in reversed(chain):
                p = (mat_mul(pxf[c]["tm"], p) + pxf[c]["pos"]).astype(f32)
                q = mat_tmul(pxf[c]["itm"], q)
            x[m], nl[m] = p, q
        q = x - ppos
        A = ptl - ppos
        mm = cross3(pddx, pddy)
        t = (dot3(q, mm) / dot3(A, mm)).astype(f32)
        r = q / t[..., None] - A
        u = (dot3(r, pddx) / dot3(pddx, pddx)).astype(f32)
        v = (-(dot3(r, pddy) / dot3(pddy, pddy))).astype(f32)
        ok = miss | (known & (t > 0) & np.isfinite(t))
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
        nu, pnu = unit(nl), unit(pn)
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
            if pid is not None:
                same = same & (np.asarray(pid, np.int32)[cj, ci] == ids)
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


@pytest.fixture
def scene(B):
    """Private scene handles, freed with their device state when the test ends (the setters change a scene: nothing shared)."""
    opened = []

    def _load(name):
        path = name if os.path.isabs(name) else os.path.join(SCENES, name + ".xml")
        opened.append(B.Scene(path))
        return opened[-1]
    yield _load
    for sc in opened:
        sc.close()


def parents_of(sc):
    return [n.parent for n in sc.flat_view().nodes]


def apply_move(B, sc, move):
    """The named moves of the tests on a scene handle: 'ball' translates c1's ball, 'parent' turns moving_nested's parent (and so its children)."""
    if move == "ball":
        k, ops = sc.node_index("ball"), [B.translate(*BALL_MOVE)]
    else:
        k, ops = sc.node_index("parent"), [B.rotate(*PARENT_TURN)]
    cur = sc.node_transform(k)
    sc.set_node_transform(k, cur["tm"], cur["pos"], ops)
    return k


def oracle_state(O, sc):
    """(camera frame, z, normal, albedo, ids, node records) of the scene as it stands, by the oracle."""
    W, H = sc.width, sc.height
    z, n, a = O.first_hit(sc.flat_bytes(), W, H)
    o, d = O.primary_rays(sc.flat_view())
    ids = O.trace_closest(sc.flat_bytes(), o, d, 1)["node"].reshape(H, W)
    return sc.camera_frame(), z.reshape(H, W), n.reshape(H, W, 3), a.reshape(H, W, 3), ids, sc.node_transforms()


_pairs = {}


def oracle_pair(B, O, name, move):
    """The oracle's images before and after the move, computed once, shared, never written to."""
    if (name, move) not in _pairs:
        sc = B.Scene(os.path.join(SCENES, name + ".xml"))
        try:
            s0 = oracle_state(O, sc)
            k = apply_move(B, sc, move)
            s1 = oracle_state(O, sc)
            for st in (s0, s1):
                for img in st:
                    img.setflags(write=False)
            _pairs[(name, move)] = (s0, s1, parents_of(sc), list(range(k, sc.flat_view().nodes[k].subtree_end)))
        finally:
            sc.close()
    return _pairs[(name, move)]


def one_hot(ids, n_nodes):
    """A radiance that names what a pixel shows: channel 0 = the ground (node 0), 1 = any other node, 2 = the sky."""
    return np.stack([ids == 0, ids > 0, ids < 0], -1).astype(f32)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("bhrt_reproject_moving", "bhrt_reproject_moving_dev")


def test_symbols_exported_declared_and_wrapped(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in SYMBOLS:
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr), s
    assert callable(B.Scene.reproject_moving) and callable(B.Scene.reproject_moving_dev)
    assert "moving objects (the scene has none)" not in hdr and "DESIGN.md 20" in hdr


def test_bad_arguments_are_refused_before_the_device(B, scene):
    """Everything bhrt_reproject refuses, a NULL snapshot and a snapshot value that is not finite: error 3 with or without a device."""
    sc = scene("moving_nested")
    W, H = sc.width, sc.height
    fr, xf = sc.camera_frame(), sc.node_transforms()
    z, n3 = np.ones((H, W), f32), np.ones((H, W, 3), f32)
    ok = B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR)
    bad_frame = fr.copy()
    bad_frame[2, 1] = NAN
    cases = [(ok, fr, None, dict(prev_radiance=n3)), (ok, None, xf, dict(prev_radiance=n3)), (ok, bad_frame, xf, dict(prev_radiance=n3)),
             (B.default_reproject_opts(depth_tolerance=-1.0), fr, xf, dict(prev_radiance=n3)), (ok, fr, xf, dict()),
             (ok, fr, xf, dict(prev_albedo=n3, want=("length",)))]
    for field, k, value in (("tm", 0, NAN), ("pos", 2, INF), ("itm", 8, -INF)):
        bad = xf.copy()
        bad[3][field][k] = value
        cases.append((ok, fr, bad, dict(prev_radiance=n3)))
    for o, f, x, kw in cases:
        with pytest.raises(B.BhrtError, match="bhrt error 3"):
            sc.reproject_moving(o, f, x, z, n3, **kw)
    with pytest.raises(ValueError):
        sc.reproject_moving(ok, fr, xf[:3], z, n3, n3)
    try:                                                   # what is allowed gets past the checks (without a device: "no device", not error 3)
        sc.reproject_moving(ok, fr, xf, z, n3, n3)
    except B.BhrtError as e:
        assert "bhrt error 3" not in str(e) and not have_gpu()


@pytest.mark.parametrize("name,move", [("c1_sphere_plane", "ball"), ("moving_nested", "parent")])
def test_restatement_with_nothing_moved_is_stage_1(B, O, name, move):
    """Bit for bit reproject_ref, with a camera move, with and without albedo, with and without prev_id (of the same scene state)."""
    s0, _, parents, _ = oracle_pair(B, O, name, move)
    fr0, z0, n0, a0, id0, xf0 = s0
    sc = B.Scene(os.path.join(SCENES, name + ".xml"))
    try:
        sc.set_camera(*moved_pose(xml_pose(name), CAMERA_MOVE))
        fr1, z1, n1, a1, id1, xf1 = oracle_state(O, sc)
    finally:
        sc.close()
    assert xf1.tobytes() == xf0.tobytes()
    rng = np.random.RandomState(1)
    rad = rng.uniform(0, 2, n0.shape).astype(f32)
    pl = rng.randint(0, 5, z0.shape).astype(f32)
    for cur, z, n, a, ids in ((fr0, z0, n0, a0, id0), (fr1, z1, n1, a1, id1)):
        for alb in (False, True):
            want = reproject_ref(cur, fr0, z, n, z0, n0, rad, pl, a if alb else None, a0 if alb else None)
            got = reproject_moving_ref(cur, fr0, parents, xf0, xf0, z, n, ids, z0, n0, rad, pl, a if alb else None, a0 if alb else None)
            assert all(same_bits(g, w) for g, w in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3])
    # a static camera and the previous ids: still the previous frame
    got = reproject_moving_ref(fr0, fr0, parents, xf0, xf0, z0, n0, id0, z0, n0, rad, None, pid=id0)
    assert got[3].all() and same_bits(got[0], rad)


def _moved_case(B, O, name, move):
    s0, s1, parents, mine = oracle_pair(B, O, name, move)
    fr0, z0, n0, a0, id0, xf0 = s0
    fr1, z1, n1, a1, id1, xf1 = s1
    rad = one_hot(id0, len(parents))
    h, l, mo, valid, t, u, v = reproject_moving_ref(fr1, fr0, parents, xf1, xf0, z1, n1, id1, z0, n0, rad, None, pid=id0)
    return id0, id1, mine, h, valid, u, v, mo


@pytest.mark.parametrize("name,move,floor", [("c1_sphere_plane", "ball", BALL_FLOOR), ("moving_nested", "parent", NESTED_FLOOR)])
def test_restatement_follows_the_object(B, O, name, move, floor):
    """The oracle's images, a static camera, prev_id given, the previous radiance naming what each pixel showed (ground, object, sky).
    Every pixel that the move uncovered or covered is invalid or carries the light of its own kind alone; at least `floor` of the moved
    object's pixels are valid; and where they are, the previous bilinear position holds the pixel's own node."""
    id0, id1, mine, h, valid, u, v, mo = _moved_case(B, O, name, move)
    H, W = id0.shape
    was, now = np.isin(id0, mine), np.isin(id1, mine)
    changed = was ^ now
    assert changed.sum() > 10
    ground, obj = changed & (id1 == 0), changed & now
    assert ground.any() and obj.any()
    assert not h[ground & valid][:, 1:].any()        # an uncovered ground pixel: no light of an object or of the sky
    assert not h[obj & valid][:, [0, 2]].any()       # a covered pixel now shows the object: no light of the ground or of the sky
    assert not h[(id1 == 0) & valid][:, 1:].any() and not h[now & valid][:, [0, 2]].any()   # and so everywhere
    share = valid[now].mean()
    print(f"{name}: {share:.4f} of the {now.sum()} pixels of the moved nodes are valid; {valid[ground].mean():.3f} of {ground.sum()} uncovered ground pixels")
    assert share >= floor
    sel = now & valid
    i0, j0 = np.floor(u[sel]).astype(int), np.floor(v[sel]).astype(int)
    k = id1[sel]
    held = np.zeros(k.shape, bool)
    for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
        qi, qj = i0 + di, j0 + dj
        inside = (qi >= 0) & (qi < W) & (qj >= 0) & (qj < H)
        held |= inside & (id0[np.clip(qj, 0, H - 1), np.clip(qi, 0, W - 1)] == k)
    assert held.all()
    assert (np.abs(mo[sel]).max(-1) > 0).mean() > 0.9           # the motion image contains the object's motion
    assert not mo[(id1 == 0) & valid].any()                     # and the ground, under a static camera, did not move


def test_the_ball_move_is_under_a_quarter_of_its_width(B):
    sc = B.Scene(os.path.join(SCENES, "c1_sphere_plane.xml"))
    try:
        width = 2 * float(sc.node_transform(sc.node_index("ball"))["tm"][0])      # a sphere of radius 1, scaled
    finally:
        sc.close()
    assert float(np.linalg.norm(BALL_MOVE)) < width / 4


def test_camera_only_reprojection_loses_the_moved_ball(B, O):
    """What the new stage is for: on the same images stage 1 (reproject_ref, which knows of no nodes) finds far fewer of the ball's pixels."""
    s0, s1, parents, mine = oracle_pair(B, O, "c1_sphere_plane", "ball")
    fr0, z0, n0, a0, id0, xf0 = s0
    fr1, z1, n1, a1, id1, xf1 = s1
    now = np.isin(id1, mine)
    plain = reproject_ref(fr1, fr0, z1, n1, z0, n0, one_hot(id0, 2))
    _, _, _, _, valid, _, _, _ = _moved_case(B, O, "c1_sphere_plane", "ball")
    print(f"valid share of the ball: stage 1 {plain[3][now].mean():.3f}, stage 1M {valid[now].mean():.3f}")
    assert plain[3][now].mean() < valid[now].mean()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
class States:
    """Two states of one scene on the GPU: as loaded (0), with guides, ids, records and a 2-spp render, and after `move` (1)."""

    def __init__(self, B, sc, pose, move, camera):
        self.sc = sc
        self.parents = parents_of(sc)
        sc.set_camera(*pose)
        self.fr0, self.g0, self.id0, self.xf0 = sc.camera_frame(), sc.first_hit(), sc.first_hit_node(), sc.node_transforms()
        self.rad0 = sc.render(B.default_opts(spp=2, seed=1))[1]
        if move is not None:
            move(sc)
        if camera:
            sc.set_camera(*moved_pose(pose, CAMERA_MOVE))
        self.fr1, self.g1, self.id1, self.xf1 = sc.camera_frame(), sc.first_hit(), sc.first_hit_node(), sc.node_transforms()


def _check(B, S, with_albedo, pass_guides, pass_id, with_pid, pl, refs=None):
    """One call against the restatement, bit for bit.  refs: a dict that keeps the restatement per (albedo, prev_id, length'): what the call
    computes itself (guides, id) does not change what it must return."""
    (z0, n0, a0), (z1, n1, a1) = S.g0, S.g1
    o = B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR)
    kw = dict(z=z1, normal=n1, albedo=a1 if with_albedo else None) if pass_guides else {}
    got = S.sc.reproject_moving(o, S.fr0, S.xf0, z0, n0, S.rad0, pl, a0 if with_albedo else None, S.id0 if with_pid else None,
                                id=S.id1 if pass_id else None, **kw)
    key = (with_albedo, with_pid, pl is not None)
    if refs is None or key not in refs:
        ref = reproject_moving_ref(S.fr1, S.fr0, S.parents, S.xf1, S.xf0, z1, n1, S.id1, z0, n0, S.rad0, pl, a1 if with_albedo else None,
                                   a0 if with_albedo else None, S.id0 if with_pid else None)
        if refs is not None:
            refs[key] = ref
    else:
        ref = refs[key]
    for k, what in enumerate(("history", "length", "motion")):
        assert same_bits(got[k], ref[k]), (what, key, pass_guides, pass_id, int((got[k].view(np.uint32) != ref[k].view(np.uint32)).sum()))
    return ref


def _nested_97x61(tmp_path):
    """moving_nested at 97 x 61: neither edge is a multiple of 16, 5917 pixels are no multiple of 256 (the ragged last workgroup)."""
    import shutil
    text = open(os.path.join(SCENES, "moving_nested.xml")).read().replace('<width value="96"/>', '<width value="97"/>').replace('<height value="64"/>', '<height value="61"/>')
    assert 'value="97"' in text and 'value="61"' in text
    path = os.path.join(str(tmp_path), "moving_nested_97x61.xml")
    open(path, "w").write(text)
    shutil.copy(os.path.join(SCENES, "mesh_small.obj"), str(tmp_path))
    return path


def _load_case(B, scene, tmp_path, name):
    if name == "ragged":
        return scene(_nested_97x61(tmp_path)), xml_pose("moving_nested"), "parent"
    return scene(name), xml_pose(name), "ball" if name == "c1_sphere_plane" else "parent"


@pytest.mark.gpu
@pytest.mark.parametrize("move", ["nothing", "object", "camera_and_object"])
@pytest.mark.parametrize("name", ["c1_sphere_plane", "moving_nested", "ragged"])
def test_kernel_equals_restatement(B, scene, tmp_path, name, move):
    """k_reproject_moving against reproject_moving_ref bit for bit over the whole product of: with and without albedo, id given and computed,
    prev_id given and NULL, a random length' image with zeros and NULL (16 calls; the guides are given with the id and computed with it, and
    two more calls split them); with nothing moved also bhrt_reproject's bytes."""
    sc, pose, what = _load_case(B, scene, tmp_path, name)
    S = States(B, sc, pose, None if move == "nothing" else (lambda s: apply_move(B, s, what)), move == "camera_and_object")
    H, W = S.id0.shape
    pl = np.random.RandomState(4).randint(0, 9, (H, W)).astype(f32)
    assert (pl == 0).any()
    refs = {}
    ref = _check(B, S, False, True, True, True, None, refs)
    hit = S.g1[0] < BIG
    mv = moved_nodes(S.parents, S.xf1, S.xf0)
    on_moved = hit & np.isin(S.id1, np.nonzero(mv)[0])
    print(f"{name} {move}: {ref[3][hit].mean():.1%} of the hit pixels valid, {ref[3][on_moved].mean() if on_moved.any() else 1:.1%} of {on_moved.sum()} on moved nodes")
    if move == "nothing":
        assert not mv.any() and ref[3].all() and same_bits(ref[0], S.rad0)
        o = B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR)
        for alb in (False, True):
            plain = sc.reproject(o, S.fr0, S.g0[0], S.g0[1], S.rad0, pl, S.g0[2] if alb else None)
            moving = sc.reproject_moving(o, S.fr0, S.xf0, S.g0[0], S.g0[1], S.rad0, pl, S.g0[2] if alb else None)
            assert all(same_bits(a, b) for a, b in zip(plain, moving))
    else:
        assert mv.any() and on_moved.sum() > 50 and ref[3][on_moved].mean() > 0.5 and (ref[2][on_moved] != 0).any()
    for with_albedo, pass_id, with_pid, random_pl in itertools.product((False, True), repeat=4):
        _check(B, S, with_albedo, pass_id, pass_id, with_pid, pl if random_pl else None, refs)
    _check(B, S, True, False, True, True, pl, refs)       # guides computed, id given
    _check(B, S, True, True, False, False, None, refs)    # guides given, id computed
    assert len(refs) == 8


@pytest.mark.gpu
def test_ids_outside_the_scene_are_invalid_pixels(B, scene):
    """Crafted id images: -1 on a hit pixel, n_nodes and INT32_MAX.  The kernel compares (uint32_t)k < n_nodes before anything is indexed with
    k, so these pixels are invalid by construction; the restatement says the same, and every other pixel is untouched by them."""
    sc = scene("moving_nested")
    S = States(B, sc, xml_pose("moving_nested"), lambda s: apply_move(B, s, "parent"), False)
    ids = S.id1.copy()
    hit = S.g1[0] < BIG
    jj, ii = np.nonzero(hit & (S.id1 > 0))
    assert len(jj) > 30
    bad = [(-1, slice(0, 10)), (sc.info.n_nodes, slice(10, 20)), (INT32_MAX, slice(20, 30)), (-(2 ** 31), slice(30, 31))]
    for value, sl in bad:
        ids[jj[sl], ii[sl]] = value
    o = B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR)
    for pid in (S.id0, None):
        got = sc.reproject_moving(o, S.fr0, S.xf0, S.g0[0], S.g0[1], S.rad0, None, None, pid, S.g1[0], S.g1[1], None, ids)
        ref = reproject_moving_ref(S.fr1, S.fr0, S.parents, S.xf1, S.xf0, S.g1[0], S.g1[1], ids, S.g0[0], S.g0[1], S.rad0, pid=pid)
        assert all(same_bits(g, r) for g, r in zip(got, ref[:3]))
        assert not got[1][jj[:31], ii[:31]].any() and not got[0][jj[:31], ii[:31]].any() and not got[2][jj[:31], ii[:31]].any()
        clean = reproject_moving_ref(S.fr1, S.fr0, S.parents, S.xf1, S.xf0, S.g1[0], S.g1[1], S.id1, S.g0[0], S.g0[1], S.rad0, pid=pid)
        rest = np.ones(hit.shape, bool)
        rest[jj[:31], ii[:31]] = False
        assert same_bits(got[0][rest], clean[0][rest]) and same_bits(got[1][rest], clean[1][rest])


@pytest.mark.gpu
def test_dev_variant_on_a_stream(B, scene):
    """Four calls issued back to back on one non-blocking stream, with no wait between them, alternating between two snapshots (the state
    before the move; the state after it, against which nothing moved): each call must see its own records, the two behind it notwithstanding."""
    import torch
    sc = scene("moving_nested")
    S = States(B, sc, xml_pose("moving_nested"), lambda s: apply_move(B, s, "parent"), True)
    H, W = S.id0.shape
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t = {k: up(x) for k, x in (("z0", S.g0[0]), ("n0", S.g0[1]), ("a0", S.g0[2]), ("rad", S.rad0), ("id0", S.id0))}
    outs = [tuple(torch.zeros((H, W, c), dtype=torch.float32, device=dev) for c in (3, 1, 2)) for _ in range(4)]
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    o = B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR)
    for k, (hist, ln, mo) in enumerate(outs):
        sc.reproject_moving_dev(o, S.fr0, S.xf0 if k % 2 == 0 else S.xf1, t["z0"].data_ptr(), t["n0"].data_ptr(), t["rad"].data_ptr(), 0, t["a0"].data_ptr(),
                                t["id0"].data_ptr(), d_history=hist.data_ptr(), d_length=ln.data_ptr(), d_motion=mo.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    refs = [reproject_moving_ref(S.fr1, S.fr0, S.parents, S.xf1, x, S.g1[0], S.g1[1], S.id1, S.g0[0], S.g0[1], S.rad0, None, S.g1[2], S.g0[2], S.id0)
            for x in (S.xf0, S.xf1)]
    assert not same_bits(refs[0][0], refs[1][0])
    for k, (hist, ln, mo) in enumerate(outs):
        ref = refs[k % 2]
        assert same_bits(hist.cpu().numpy(), ref[0]) and same_bits(ln.cpu().numpy()[..., 0], ref[1]) and same_bits(mo.cpu().numpy(), ref[2]), k


@pytest.mark.gpu
def test_quality_of_a_carried_ball(B, scene):
    """c1_sphere_plane, the ball translated by BALL_MOVE: a 64-spp history carried into a 4-spp frame is closer to the new state's 256-spp frame
    than the 4-spp frame alone AND than what camera-only bhrt_reproject + accumulate gives, over the ball's valid pixels.  The three
    MSEs are printed; measured: carried 1.93e-3, 4 spp alone 6.28e-3, camera-only 1.76e-2 over 13239 pixels."""
    sc = scene("c1_sphere_plane")
    ro, to = B.default_reproject_opts(depth_tolerance=TOL, normal_threshold=THR), B.default_temporal_opts(clamp_k=-1.0, max_length=INF)
    fr0, xf0 = sc.camera_frame(), sc.node_transforms()
    z0, n0, a0 = sc.first_hit()
    id0 = sc.first_hit_node()
    old = sc.render(B.default_opts(spp=64, seed=3))[1]
    ball = apply_move(B, sc, "ball")
    R = sc.render(B.default_opts(spp=256, seed=77))[1]
    A = sc.render(B.default_opts(spp=4, seed=1))[1]
    l0 = np.full(z0.shape, 64, f32)
    h, l, _ = sc.reproject_moving(ro, fr0, xf0, z0, n0, old, l0, a0, id0)
    carried = sc.temporal_accumulate(to, A, 4.0, h, l)[0]
    hc, lc, _ = sc.reproject(ro, fr0, z0, n0, old, l0, a0)
    camera_only = sc.temporal_accumulate(to, A, 4.0, hc, lc)[0]
    m = (sc.first_hit_node() == ball) & (l > 0)
    mse = lambda x: float(np.mean(((x - R) ** 2)[m]))  # noqa: E731
    print(f"ball pixels valid {m.sum()}: MSE carried {mse(carried):.4g}, 4 spp alone {mse(A):.4g}, camera-only reprojection {mse(camera_only):.4g}")
    assert m.sum() > 1000
    assert mse(carried) < mse(A) and mse(carried) < mse(camera_only)
