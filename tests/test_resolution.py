"""bhrt_scene_set_resolution: the <camera>'s width and height of a loaded scene through the loader's own code.  The blob becomes
that of the scene file with the two values edited, pose 1 of an active shutter follows, the clone carries the edit, and an uploaded scene needs
nothing but its camera refreshed: every per-pixel device buffer is sized by the call that uses it."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, SCENES

f32 = np.float32
ERR_ARG = 3
MAX_SIDE, MAX_PIXELS = 1 << 24, (1 << 31) - 1
POSE1 = ((0.4, 0.1, 0.2), None, None)  # the shutter's pose 1: the camera moved a little, its target and up kept (filled in from the scene)


def edited_xml(tmp_path, name, W, H):
    """A copy of tests/scenes/<name>.xml with <width> and <height> edited, beside copies of the mesh files it names."""
    text = open(os.path.join(SCENES, name + ".xml")).read()
    text, k1 = re.subn(r'<width value="\d+"/>', '<width value="%d"/>' % W, text)
    text, k2 = re.subn(r'<height value="\d+"/>', '<height value="%d"/>' % H, text)
    assert k1 == 1 and k2 == 1
    for obj in set(re.findall(r'name="([^"]+\.obj)"', text)):
        shutil.copy(os.path.join(SCENES, obj), tmp_path / obj)
    path = tmp_path / ("%s_%dx%d.xml" % (name, W, H))
    path.write_text(text)
    return str(path)


def _pose1(sc):
    cam = sc.flat_view().header.camera
    pos = np.float32(list(cam.pos))
    target = pos + np.float32(list(cam.dir)) * f32(cam.focaldist)
    return pos + np.float32(POSE1[0]), target, np.float32(list(cam.up))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_symbol_exported_declared_and_wrapped(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    s = "bhrt_scene_set_resolution"
    assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr) and callable(B.Scene.set_resolution)
    assert int(re.search(r"#define BHRT_MAX_IMAGE_SIDE (\d+)", hdr).group(1)) == MAX_SIDE
    assert int(re.search(r"#define BHRT_MAX_IMAGE_PIXELS (\d+)", hdr).group(1)) == MAX_PIXELS


def test_refusals_change_nothing_and_need_no_device(B):
    """A NULL scene, a side below 1, a side above 2^24, more than 2^31 - 1 pixels, and an open progressive or temporal session: BHRT_ERR_ARG on a
    scene that was never uploaded, the blob and the reported size untouched.  The largest sizes are taken (nothing per pixel lives on the host)."""
    L = B.lib()
    assert L.bhrt_scene_set_resolution(None, 4, 4) == ERR_ARG
    sc = B.Scene(os.path.join(SCENES, "c1_sphere_plane.xml"))
    try:
        before, size = sc.flat_bytes(), (sc.width, sc.height)
        for w, h in ((0, 4), (4, 0), (-1, 4), (4, -7), (0, 0), (MAX_SIDE + 1, 1), (1, MAX_SIDE + 1), (46341, 46341), (1 << 16, 1 << 15), (MAX_SIDE, 128),
                     (2147483647, 2147483647)):
            with pytest.raises(B.BhrtError, match="bhrt error 3.*bhrt_scene_set_resolution"):
                sc.set_resolution(w, h)
            assert sc.flat_bytes() == before and (sc.width, sc.height) == size
        for open_, close in ((lambda: sc.progressive_begin(B.default_opts(spp=2)), sc.progressive_end),
                             (lambda: sc.temporal_begin(B.default_opts(spp=2), B.default_temporal_session_opts()), sc.temporal_end)):
            open_()
            with pytest.raises(B.BhrtError, match="bhrt error 3.*session is open"):
                sc.set_resolution(32, 24)
            sc._flat = None
            assert sc.flat_bytes() == before and (sc.width, sc.height) == size
            close()
            sc.set_resolution(32, 24)                                             # the session ended: allowed again
            sc.set_resolution(*size)
            assert sc.flat_bytes() == before
        for w, h in ((46340, 46340), (MAX_SIDE, 127), (1, MAX_SIDE), (1 << 16, (1 << 15) - 1)):
            sc.set_resolution(w, h)
            assert (sc.width, sc.height) == (w, h)
    finally:
        sc.close()


@pytest.mark.parametrize("name", ["c1_sphere_plane", "c3_mesh_small"])
@pytest.mark.parametrize("size", [(1000, 700), (75, 57), (1, 1), (3, 200)])
def test_blob_equals_the_edited_scene_file(B, tmp_path, name, size):
    """After the setter bhrt_scene_flat is byte-identical to the blob of the scene file with the two values edited, at the same address;
    bhrt_scene_info reports the size; pose 1 of a shutter that is on has the frame the edited file's scene derives; the clone carries all of it."""
    W, H = size
    sc, want = B.Scene(os.path.join(SCENES, name + ".xml")), B.Scene(edited_xml(tmp_path, name, W, H))
    try:
        p0, p1, nbytes = C.c_void_p(), C.c_void_p(), C.c_uint64()
        assert B.lib().bhrt_scene_flat(sc._h, C.byref(p0), C.byref(nbytes)) == 0
        assert sc.flat_bytes() != want.flat_bytes()
        for shutter in (False, True):
            if shutter:
                sc.set_resolution(*want_size)                                     # back, with the shutter switched on at the old size
                sc.set_shutter(True, *_pose1(sc))
                want.set_shutter(True, *_pose1(want))
            want_size = (sc.width, sc.height)
            sc.set_resolution(W, H)
            assert (sc.width, sc.height) == (W, H) == (want.width, want.height)
            assert sc.flat_bytes() == want.flat_bytes()
            assert B.lib().bhrt_scene_flat(sc._h, C.byref(p1), C.byref(nbytes)) == 0 and p1.value == p0.value and nbytes.value == len(want.flat_bytes())
            on, pose, frame = sc.shutter()
            on_w, pose_w, frame_w = want.shutter()
            assert on == on_w == shutter and pose.tobytes() == pose_w.tobytes() and frame.tobytes() == frame_w.tobytes()
            assert sc.camera_frame().tobytes() == want.camera_frame().tobytes()
            cl = sc.clone()
            try:
                assert (cl.width, cl.height) == (W, H) and cl.flat_bytes() == want.flat_bytes() and cl.shutter()[2].tobytes() == frame_w.tobytes()
                cl.set_resolution(8, 8)                                           # the clone's own size from here on
                assert (sc.width, sc.height) == (W, H) and sc.flat_bytes() == want.flat_bytes()
            finally:
                cl.close()
        assert frame.any()
    finally:
        sc.close()
        want.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_an_uploaded_scene_is_resized_down_then_up(B, tmp_path):
    """c3_mesh_small, uploaded and rendered at its own size, then set to 75 x 57 and to 333 x 251: each time bhrt_render at 2 spp, bhrt_render_var,
    bhrt_first_hit, and a bhrt_denoise and a bhrt_temporal_change call that compute their own guides equal those of a freshly loaded scene file
    with the size edited, byte for byte.  Every per-pixel device buffer is sized by the call that uses it."""
    name = "c3_mesh_small"
    sc = B.Scene(os.path.join(SCENES, name + ".xml"))
    o = B.default_opts(spp=2, seed=4)

    def everything(s):
        rgb, rad, _ = s.render(o)
        _, rad2, var = s.render_var(o)
        z, n, a = s.first_hit()
        dn = s.denoise(B.default_denoise_opts(), rad, var)                         # its own guides
        l = np.full((s.height, s.width), 4, f32)
        ch = s.temporal_change(B.default_change_opts(), rad, var, rad[::-1].copy(), var, l)   # its own guides; the history is the frame upside down
        sv = s.variance_spatial(B.default_spatial_variance_opts(), rad)            # its own guides, from the denoiser's scratch
        return [rgb, rad, rad2, var, z, n, a, dn[0], dn[1], ch[0], ch[1], sv]
    try:
        sc.upload(0)
        first = everything(sc)
        assert first[0].shape == (240, 320, 3)
        for W, H in ((75, 57), (333, 251)):
            sc.set_resolution(W, H)
            got = everything(sc)
            fresh = B.Scene(edited_xml(tmp_path, name, W, H))
            try:
                want = everything(fresh)
            finally:
                fresh.close()
            assert got[0].shape == (H, W, 3) and got[9].shape == (H, W)
            for k, (g, w) in enumerate(zip(got, want)):
                assert g.tobytes() == w.tobytes(), (W, H, k)
            assert (got[10] > 0).any()                                            # the change test found the flipped history
    finally:
        sc.close()
