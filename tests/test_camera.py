"""bhrt_scene_set_camera: position, target, up and fov of a loaded scene, through the loader's own operations.

On the CPU the blob after the call is held to the blob of the edited scene file, byte for byte, and every refused argument to BHRT_ERR_ARG
with the blob unchanged.  On the GPU a camera set after the upload renders like the freshly loaded edited scene, frame and first hit, on a
scene with nested nodes and a mesh: the camera position carried through every node's chain (DevScene::cam_chain) has to follow."""
import os
import re

import numpy as np
import pytest

from conftest import SCENES, same_bits

f32 = np.float32
NAN, INF = float("nan"), float("inf")


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


def with_camera_pose(xml_text, position=None, target=None, up=None, fov=None):
    """The scene text with <position>, <target>, <up> (x, y, z) and <fov> of its <camera> replaced (or added); None keeps a tag."""
    head, cam = xml_text.split("<camera>")
    for tag, v in (("position", position), ("target", target), ("up", up)):
        if v is None:
            continue
        cam = re.sub(r"\s*<%s [^>]*/>" % tag, "", cam)
        cam = cam.replace("</camera>", '  <%s x="%r" y="%r" z="%r"/>\n  </camera>' % (tag, float(v[0]), float(v[1]), float(v[2])))
    if fov is not None:
        cam = re.sub(r"\s*<fov [^>]*/>", "", cam)
        cam = cam.replace("</camera>", '  <fov value="%r"/>\n  </camera>' % float(fov))
    return head + "<camera>" + cam


class edited_scene:
    """A temporary scene file beside tests/scenes/<name>.xml (it refers to its mesh by a relative path) with the camera tags replaced."""

    def __init__(self, name, tag, **pose):
        self.path = os.path.join(SCENES, "_tmp_camera_%s_%s.xml" % (name, tag))
        self.text = with_camera_pose(open(os.path.join(SCENES, name + ".xml")).read(), **pose)

    def __enter__(self):
        with open(self.path, "w") as f:
            f.write(self.text)
        return self.path

    def __exit__(self, *exc):
        if os.path.exists(self.path):
            os.remove(self.path)


# pos, target, up, fov: an up that is not orthogonal to the view direction in every case but the last; fov <= 0 keeps the scene's
POSES = [
    ((3.0, -28.0, 12.5), (1.0, 0.5, 4.0), (0.0, 0.0, 1.0), 35.0),
    ((-12.25, -20.0, 6.0), (0.0, 2.0, 3.0), (0.1, 0.2, 1.0), 0.0),
    ((10.0, 14.0, 21.0), (-1.0, -2.0, 0.5), (0.3, -0.4, 0.8), -5.0),
    ((0.0, -40.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 2.0), 52.5),
]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_the_camera_calls_are_exported(B):
    assert {"bhrt_scene_set_camera", "bhrt_scene_set_shutter", "bhrt_scene_get_shutter"} <= set(B.EXPORTS)
    for name in ("bhrt_scene_set_camera", "bhrt_scene_set_shutter", "bhrt_scene_get_shutter"):
        assert hasattr(B.lib(), name)
    hdr = open(os.path.join(os.path.dirname(SCENES), "..", "include", "bhrt.h")).read()
    assert "int bhrt_scene_set_camera(bhrt_scene *scene, const float pos[3], const float target[3], const float up[3], float fov);" in hdr
    assert "int bhrt_scene_set_shutter(bhrt_scene *scene, int on, const float pos1[3], const float target1[3], const float up1[3]);" in hdr
    rng = open(os.path.join(os.path.dirname(SCENES), "..", "include", "bhrt_rng.h")).read()
    assert "#define BHRT_SEC_SHUTTER 4u" in rng


@pytest.mark.parametrize("k", range(len(POSES)))
@pytest.mark.parametrize("name", ["lens_spheres", "shutter_plain", "c3_mesh_small"])
def test_set_camera_gives_the_blob_of_the_edited_scene_file(B, scene, name, k):
    pos, target, up, fov = POSES[k]
    sc = scene(name)
    before = sc.flat_bytes()
    cam0 = sc.flat_view().header.camera
    old = (cam0.fov, cam0.focaldist, cam0.dof, cam0.width, cam0.height)
    sc.set_camera(pos, target, up, fov)
    with edited_scene(name, "blob%d" % k, position=pos, target=target, up=up, fov=fov if fov > 0 else None) as path:
        ref = scene(path)
        cam = ref.flat_view().header.camera
        assert tuple(cam.pos) == tuple(f32(x) for x in pos)
        assert cam.fov == (f32(fov) if fov > 0 else old[0]) and (cam.focaldist, cam.dof, cam.width, cam.height) == old[1:]
        assert ref.flat_bytes() != before
        assert sc.flat_bytes() == ref.flat_bytes()
    d, u = np.array(list(cam.dir), np.float64), np.array(list(cam.up), np.float64)
    assert abs(d @ u) < 1e-6 and abs(np.linalg.norm(d) - 1) < 1e-6 and abs(np.linalg.norm(u) - 1) < 1e-6


def test_set_camera_keeps_the_blob_pointer_and_needs_no_device(B, scene):
    import ctypes as C
    sc = scene("shutter_plain")
    p0, n0, p1, n1 = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    assert B.lib().bhrt_scene_flat(sc._h, C.byref(p0), C.byref(n0)) == 0
    sc.set_camera(*POSES[0])
    assert B.lib().bhrt_scene_flat(sc._h, C.byref(p1), C.byref(n1)) == 0
    assert p0.value == p1.value and n0.value == n1.value
    assert C.string_at(p0, n0.value) == sc.flat_bytes()


BAD_CAMERAS = [
    ((NAN, 0, 0), (0, 0, 0), (0, 0, 1), 30.0, "finite"),
    ((0, -30, 10), (0, INF, 0), (0, 0, 1), 30.0, "finite"),
    ((0, -30, 10), (0, 0, 0), (0, -INF, 1), 30.0, "finite"),
    ((0, -30, 10), (0, 0, 0), (0, 0, 1), NAN, "fov"),
    ((0, -30, 10), (0, 0, 0), (0, 0, 1), INF, "fov"),
    ((0, -30, 10), (0, 0, 0), (0, 0, 1), -INF, "fov"),
    ((0, -30, 10), (0, 0, 0), (0, 0, 1), 180.0, "fov"),
    ((0, -30, 10), (0, 0, 0), (0, 0, 1), 270.0, "fov"),
    ((1, 2, 3), (1, 2, 3), (0, 0, 1), 30.0, "target == pos"),
    ((0, -30, 0), (0, 0, 0), (0, 2, 0), 30.0, "parallel"),
    ((0, -30, 0), (0, 0, 0), (0, 0, 0), 30.0, "parallel"),
    (None, (0, 0, 0), (0, 0, 1), 30.0, "NULL"),
    ((0, -30, 10), None, (0, 0, 1), 30.0, "NULL"),
    ((0, -30, 10), (0, 0, 0), None, 30.0, "NULL"),
]


@pytest.mark.parametrize("pos,target,up,fov,what", BAD_CAMERAS)
def test_set_camera_refuses_bad_arguments_and_changes_nothing(B, scene, pos, target, up, fov, what):
    sc = scene("shutter_plain")  # never uploaded
    before = sc.flat_bytes()
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: bhrt_scene_set_camera: .*" + re.escape(what)):
        sc.set_camera(pos, target, up, fov)
    sc._flat = None
    assert sc.flat_bytes() == before


def test_set_camera_refuses_a_null_scene(B):
    import ctypes as C
    v = (C.c_float * 3)(0, 0, 1)
    assert B.lib().bhrt_scene_set_camera(None, v, v, v, C.c_float(30)) == 3
    assert B.lib().bhrt_scene_set_shutter(None, 0, None, None, None) == 3


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
NEW_POSE = ((14.0, -24.0, 13.5), (1.0, 1.5, 3.0), (0.1, 0.0, 1.0), 36.0)


@pytest.mark.gpu
def test_set_camera_after_upload_renders_like_a_fresh_scene(B, O, scene):
    """Nested nodes and a mesh: the frame and bhrt_first_hit both read the camera position through the nodes' chains."""
    sc = scene("shutter_plain")
    assert sc.info.max_node_depth >= 3 and sc.info.n_meshes >= 1
    sc.upload(0)
    o = B.default_opts(spp=2, gi_bounces=3, seed=8)
    before, _, _ = sc.render(o)
    z0, _, _ = sc.first_hit()
    sc.set_camera(*NEW_POSE)
    rgb, rad, _ = sc.render(o)
    z, nrm, alb = sc.first_hit()
    assert not np.array_equal(rgb, before) and not same_bits(z, z0)
    with edited_scene("shutter_plain", "fresh", position=NEW_POSE[0], target=NEW_POSE[1], up=NEW_POSE[2], fov=NEW_POSE[3]) as path:
        fresh = scene(path)
        assert fresh.flat_bytes() == sc.flat_bytes()
        frgb, frad, _ = fresh.render(o)
        fz, fn, fa = fresh.first_hit()
    assert np.array_equal(rgb, frgb) and same_bits(rad, frad)
    assert same_bits(z, fz) and same_bits(nrm, fn) and same_bits(alb, fa)
    oz, on, oa = O.first_hit(sc.flat_bytes(), sc.width, sc.height)
    assert same_bits(z.ravel(), oz) and same_bits(nrm.reshape(-1, 3), on)
    hit = z < 1e29
    print("first hit: %d of %d pixels hit" % (int(hit.sum()), hit.size))
    assert hit.sum() >= hit.size // 4 and (~hit).sum() >= 10


@pytest.mark.gpu
def test_set_camera_between_two_progressive_sessions(B, scene):
    """End a session, set the camera, begin again: the second session's frame is the new camera's.  Between two steps of one session later
    samples use the new camera, as with the other setters: the frame then mixes both."""
    sc = scene("shutter_plain")
    o = B.default_opts(spp=4, gi_bounces=3, seed=5)
    sc.progressive_begin(o)
    sc.progressive_step(4)
    first = sc.progressive_frame()
    sc.progressive_end()
    old_rgb, old_rad, _ = sc.render(o)
    assert np.array_equal(first[0], old_rgb) and same_bits(first[1], old_rad)
    sc.set_camera(*NEW_POSE)
    sc.progressive_begin(o)
    sc.progressive_step(2)
    sc.progressive_step(2)
    second = sc.progressive_frame()
    sc.progressive_end()
    with edited_scene("shutter_plain", "prog", position=NEW_POSE[0], target=NEW_POSE[1], up=NEW_POSE[2], fov=NEW_POSE[3]) as path:
        frgb, frad, _ = scene(path).render(o)
    assert np.array_equal(second[0], frgb) and same_bits(second[1], frad)
    assert not np.array_equal(second[0], old_rgb)
    # inside one session: two samples of the new camera, then two of the old pose again
    back = scene("shutter_plain").flat_view().header.camera
    sc.progressive_begin(o)
    sc.progressive_step(2)
    sc.set_camera((0.0, -30.0, 10.0), (0.0, 0.0, 4.0), (0.0, 0.0, 1.0), float(back.fov))
    sc.progressive_step(2)
    mixed = sc.progressive_frame()
    sc.progressive_end()
    assert not same_bits(mixed[1], frad) and not same_bits(mixed[1], old_rad)
    s_orig, _ = scene(path_of("shutter_plain")).render_samples(o, 0, 0, sc.width, sc.height)
    with edited_scene("shutter_plain", "prog2", position=NEW_POSE[0], target=NEW_POSE[1], up=NEW_POSE[2], fov=NEW_POSE[3]) as path:
        s_moved, _ = scene(path).render_samples(o, 0, 0, sc.width, sc.height)
    # samples 0, 1 of the moved camera and 2, 3 of the original one.  The session folds in float32 in an order of its own: four terms of one
    # sign, so the two means agree to a few ulp (2^-23 each); 1e-5 relative is 80 ulp
    expect = (((s_moved[:, 0] + s_moved[:, 1]) + s_orig[:, 2]) + s_orig[:, 3]) / f32(4)
    assert np.allclose(mixed[1].reshape(-1, 3), expect, rtol=1e-5, atol=1e-7)


def path_of(name):
    return os.path.join(SCENES, name + ".xml")
