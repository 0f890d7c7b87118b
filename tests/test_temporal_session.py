"""The temporal session (bhrt_temporal_*): reproject -> accumulate -> estimate -> denoise as one device-resident call per frame.
Every kept image of every frame equals, byte for byte, what the existing host wrappers give when they are chained as bhrt render --temporal
chained them; the loop is restated here once (_chain).  c3_mesh_small, 320 x 240, three frames along a camera move."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENES
from test_cli import _png, _run

f32 = np.float32
ERR_ARG = 3
XML = os.path.join(SCENES, "c3_mesh_small.xml")
POSE0 = np.float32([0, -30, 10, 0, 0, 3, 0, 0, 1])          # the scene's own camera: position, target, up
POSE1 = np.float32([1.5, -30, 10.5, 0, 0, 3, 0, 0, 1])
SEED, FRAMES = 5, 3
# mode -> (spp, carry_variance, spatial_variance, denoise, follow_nodes)
MODES = {"light": (2, 0, 0, 0, 0), "denoise": (2, 1, 0, 1, 0), "spatial": (1, 1, 1, 1, 0), "nodes": (1, 1, 1, 1, 1), "light_nodes": (2, 0, 0, 0, 1)}
BALL_MOVE = (-1.5, 0.5, 0.75)                               # the translation of the node "ball" at the last frame (mode "nodes")
SYMBOLS = ["bhrt_temporal_begin", "bhrt_temporal_frame", "bhrt_temporal_frame_dev", "bhrt_temporal_reset", "bhrt_temporal_status", "bhrt_temporal_image",
           "bhrt_temporal_image_dev", "bhrt_temporal_end"]


def _opts(B, mode):
    spp, carry, spatial, denoise, nodes = MODES[mode]
    return B.default_opts(spp=spp, seed=SEED), B.default_temporal_session_opts(carry_variance=carry, spatial_variance=spatial, denoise=denoise, follow_nodes=nodes)


# ---- without a device -----------------------------------------------------------------------------------------------------------------------

def test_exports(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in SYMBOLS:
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr), s
    s = "bhrt_default_temporal_session_opts"
    assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bvoid %s\(" % s, hdr)
    for k, name in enumerate(["ACCUMULATED", "VARIANCE", "LENGTH", "HISTORY_LENGTH", "FILTER_VARIANCE", "Z", "NORMAL", "ALBEDO", "NODE", "CURRENT", "CURRENT_VARIANCE"]):
        assert re.search(r"\bBHRT_TEMPORAL_IMG_%s = %d\b" % (name, k), hdr) and getattr(B, "TEMPORAL_IMG_" + name) == k


def test_struct_sizes_and_defaults(B):
    """The C side writes exactly sizeof(struct) bytes (both calls memset their struct): the Python structs have the C sizes."""
    assert C.sizeof(B.TemporalSessionOpts) == 4 * 32 + 8 * 4 and C.sizeof(B.TemporalProgress) == 40
    buf = (C.c_uint8 * 256)(*([0xAB] * 256))
    B.lib().bhrt_default_temporal_session_opts(C.byref(buf))
    n = C.sizeof(B.TemporalSessionOpts)
    assert bytes(buf[n - 16:n]) == bytes(16) and bytes(buf[n:]) == b"\xab" * (256 - n)      # reserved[4] is the struct's tail
    o = B.default_temporal_session_opts()
    assert bytes(o) == bytes(buf[:n])
    for got, want in ((o.reproject, B.default_reproject_opts()), (o.temporal, B.default_temporal_opts()), (o.spatial, B.default_spatial_variance_opts()),
                      (o.denoise_opts, B.default_denoise_opts())):
        assert bytes(got) == bytes(want)
    assert (o.carry_variance, o.spatial_variance, o.denoise, o.follow_nodes) == (0, 0, 0, 0)
    sc = B.Scene(XML)
    try:
        sc.temporal_begin(*_opts(B, "light"))
        buf = (C.c_uint8 * 256)(*([0xAB] * 256))
        assert B.lib().bhrt_temporal_status(sc._h, C.byref(buf)) == 0
        n = C.sizeof(B.TemporalProgress)
        assert bytes(buf[n:]) == b"\xab" * (256 - n)
        p = B.TemporalProgress.from_buffer_copy(bytes(buf[:n]))
        assert (p.frames, p.failed, p.history_pixels, p.pixels) == (0, 0, 0, 320 * 240)
    finally:
        sc.close()


def _refused(B, sc, opts, topts, match):
    with pytest.raises(B.BhrtError, match="bhrt error 3.*" + match):
        sc.temporal_begin(opts, topts)
    assert B.lib().bhrt_temporal_status(sc._h, C.byref(B.TemporalProgress())) == ERR_ARG    # nothing changed: no session is open


def test_refusals_on_a_scene_that_was_never_uploaded(B):
    sc = B.Scene(XML)
    try:
        L, o2, T = B.lib(), B.default_opts(spp=2), B.default_temporal_session_opts
        t = T()
        assert L.bhrt_temporal_begin(None, C.byref(o2), C.byref(t)) == ERR_ARG
        _refused(B, sc, None, t, "null")
        _refused(B, sc, o2, None, "null")
        _refused(B, sc, o2, T(spatial_variance=1), "spatial_variance needs carry_variance")
        _refused(B, sc, o2, T(denoise=1), "denoise needs carry_variance")
        _refused(B, sc, B.default_opts(spp=1), T(carry_variance=1), "spp < 2")
        _refused(B, sc, B.default_opts(spp=1), T(carry_variance=1, denoise=1), "spp < 2")
        # what the stages refuse of their own options
        t = T()
        t.reproject.depth_tolerance = -1.0
        _refused(B, sc, o2, t, "depth_tolerance")
        t = T()
        t.reproject.normal_threshold = float("nan")
        _refused(B, sc, o2, t, "normal_threshold")
        t = T()
        t.temporal.max_length = 0.0
        _refused(B, sc, o2, t, "max_length")
        t = T(carry_variance=1, spatial_variance=1)
        t.spatial.radius = 5
        _refused(B, sc, o2, t, "radius")
        t = T(carry_variance=1, spatial_variance=1)
        t.spatial.min_length = float("nan")
        _refused(B, sc, o2, t, "min_length")
        t = T(carry_variance=1, denoise=1)
        t.denoise_opts.iterations = 17
        _refused(B, sc, o2, t, "iterations")
        t = T(carry_variance=1, denoise=1)
        t.denoise_opts.sigma_depth = -1.0
        _refused(B, sc, o2, t, "sigmas")
        # what bhrt_render* refuses of bhrt_opts
        _refused(B, sc, B.default_opts(spp=0), T(), "spp")
        _refused(B, sc, B.default_opts(spp=65536), T(), "spp")
        _refused(B, sc, B.default_opts(spp=2, lens=2), T(), "lens")
        _refused(B, sc, B.default_opts(spp=2, gi_bounces=61), T(), "bounce")
        _refused(B, sc, B.default_opts(spp=2, rank=1), T(), "rank")
        _refused(B, sc, B.default_opts(spp=2, photon_map=1), T(), "photon_map")
        _refused(B, sc, B.default_opts(spp=2, world_size=2), T(), "world_size")
        sc.set_global_gather(True)
        _refused(B, sc, o2, T(), "global")
        sc.set_global_gather(False)
        # a second session
        sc.temporal_begin(o2, T())
        with pytest.raises(B.BhrtError, match="bhrt error 3.*already open"):
            sc.temporal_begin(o2, T())
        assert sc.temporal_status().frames == 0                                            # the first one stands
        # before the first frame no image can be asked for; one outside 0..10 never
        for which in (B.TEMPORAL_IMG_ACCUMULATED, B.TEMPORAL_IMG_Z, 11, -1):
            assert L.bhrt_temporal_image(sc._h, which, C.byref((C.c_uint8 * 16)())) == ERR_ARG
            assert L.bhrt_temporal_image_dev(sc._h, which, C.byref(C.c_void_p())) == ERR_ARG
        assert L.bhrt_temporal_image(sc._h, 0, None) == ERR_ARG and L.bhrt_temporal_image_dev(sc._h, 0, None) == ERR_ARG
        assert L.bhrt_temporal_status(sc._h, None) == ERR_ARG
        sc.temporal_end()
    finally:
        sc.close()


def test_calls_without_a_session(B):
    sc = B.Scene(XML)
    try:
        L = B.lib()
        assert L.bhrt_temporal_frame(sc._h, None, None, None) == ERR_ARG and L.bhrt_temporal_frame_dev(sc._h, None, None, None) == ERR_ARG
        assert L.bhrt_temporal_image(sc._h, 0, C.byref((C.c_uint8 * 16)())) == ERR_ARG
        assert L.bhrt_temporal_image_dev(sc._h, 0, C.byref(C.c_void_p())) == ERR_ARG
        assert L.bhrt_temporal_reset(sc._h) == ERR_ARG
        assert L.bhrt_temporal_status(sc._h, C.byref(B.TemporalProgress())) == ERR_ARG
        assert L.bhrt_temporal_end(sc._h) == 0
        for fn in (L.bhrt_temporal_reset, L.bhrt_temporal_end):
            assert fn(None) == ERR_ARG
        assert L.bhrt_temporal_reset(sc._h) == ERR_ARG and b"no temporal session" in L.bhrt_last_error()
    finally:
        sc.close()


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------------

KEPT = {"accumulated": "ACCUMULATED", "variance": "VARIANCE", "length": "LENGTH", "history_length": "HISTORY_LENGTH", "filter_variance": "FILTER_VARIANCE",
        "z": "Z", "normal": "NORMAL", "albedo": "ALBEDO", "node": "NODE", "current": "CURRENT", "current_variance": "CURRENT_VARIANCE"}


def _pose(k, frames=FRAMES):
    return (POSE0 + (POSE1 - POSE0) * (f32(k) / f32(frames - 1))).astype(f32)


def _set_frame(B, sc, mode, k, saved):
    """The host's whole job between two frames: the camera, and in mode "nodes" the node "ball" at its saved record plus a part of the move."""
    p = _pose(k)
    sc.set_camera(p[0:3], p[3:6], p[6:9])
    if MODES[mode][4]:
        s = f32(k) / f32(FRAMES - 1)
        sc.set_node_transform(sc.node_index("ball"), saved["tm"], saved["pos"], [B.translate(*[float(f32(v) * s) for v in BALL_MOVE])])


def _chain(B, mode):
    """What bhrt render --temporal did frame by frame before the session existed, through the host wrappers: one dict of images per frame."""
    spp, carry, spatial, denoise, nodes = MODES[mode]
    ro, to, sv, dn = B.default_reproject_opts(), B.default_temporal_opts(), B.default_spatial_variance_opts(), B.default_denoise_opts()
    sc = B.Scene(XML)
    out, prev = [], None
    try:
        saved = sc.node_transform(sc.node_index("ball")) if nodes else None
        for k in range(FRAMES):
            _set_frame(B, sc, mode, k, saved)
            o = B.default_opts(spp=spp, seed=SEED + k)
            f = {}
            f["z"], f["normal"], f["albedo"] = z, n, a = sc.first_hit()
            if nodes:
                f["node"] = sc.first_hit_node()
            h = hv = hl = None
            if carry:
                _, cur, cv = sc.render_var(o)
                if spatial and spp < 2:
                    cv = sc.variance_spatial(sv, cur, None, None, z, n, a)
                if prev is not None:
                    h, hv, hl = sc.reproject_var(ro, prev["frame"], prev["z"], prev["normal"], prev["accumulated"], prev["variance"], prev["length"], prev["albedo"], z, n, a,
                                                 prev_xforms=prev["xf"] if nodes else None, prev_id=prev["node"] if nodes else None, id=f["node"] if nodes else None,
                                                 want=("history", "history_variance", "length"))[:3]
                acc, accv, ln, rgb = sc.temporal_accumulate_var(to, cur, cv, float(spp), h, hv, hl)
                f["variance"], f["current_variance"] = accv, cv
                est = accv
                if spatial:
                    est = f["filter_variance"] = sc.variance_spatial(sv, acc, accv, ln, z, n, a)
                shown = acc
                if denoise:
                    shown, rgb = sc.denoise(dn, acc, est, z, n, a)
            else:
                cur = sc.render(o)[1]
                if prev is not None and nodes:
                    h, hl = sc.reproject_moving(ro, prev["frame"], prev["xf"], prev["z"], prev["normal"], prev["accumulated"], prev["length"], prev["albedo"], prev["node"],
                                                z, n, a, f["node"], want=("history", "length"))[:2]
                elif prev is not None:
                    h, hl = sc.reproject(ro, prev["frame"], prev["z"], prev["normal"], prev["accumulated"], prev["length"], prev["albedo"], z, n, a, want=("history", "length"))[:2]
                acc, ln, rgb = sc.temporal_accumulate(to, cur, float(spp), h, hl)
                shown = acc
            f.update(accumulated=acc, length=ln, current=cur, history_length=np.zeros_like(ln) if hl is None else hl, shown=shown, rgb8=rgb)
            out.append(f)
            prev = dict(f, frame=sc.camera_frame(), xf=sc.node_transforms() if nodes else None)
    finally:
        sc.close()
    return out


_chains = {}


@pytest.fixture(scope="module")
def chain(B):
    """The reference frames of a mode, computed once and shared; nobody writes to them."""
    def get(mode):
        if mode not in _chains:
            _chains[mode] = _chain(B, mode)
            for f in _chains[mode]:
                for a in f.values():
                    a.flags.writeable = False
        return _chains[mode]
    return get


def _kept(B, sc):
    f = {}
    for key, name in KEPT.items():
        which = getattr(B, "TEMPORAL_IMG_" + name)
        p = C.c_void_p()
        if B.lib().bhrt_temporal_image_dev(sc._h, which, C.byref(p)) == ERR_ARG:           # not kept by this mode: the host copy is refused alike
            with pytest.raises(B.BhrtError, match="not kept"):
                sc.temporal_image(which)
            continue
        assert p.value
        f[key] = sc.temporal_image(which)
    return f


def _same(got, want, where):
    assert set(got) == set(want), (where, sorted(set(got) ^ set(want)))
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), (where, key)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_every_kept_image_of_every_frame_equals_the_chained_wrappers(B, chain, mode):
    ref = chain(mode)
    sc = B.Scene(XML)
    try:
        saved = sc.node_transform(sc.node_index("ball")) if MODES[mode][4] else None
        sc.temporal_begin(*_opts(B, mode))
        for k in range(FRAMES):
            _set_frame(B, sc, mode, k, saved)
            rgb, rad, st = sc.temporal_frame()
            f = dict(_kept(B, sc), shown=rad, rgb8=rgb)
            _same(f, ref[k], (mode, k))
            pg = sc.temporal_status()
            with_history = int((ref[k]["history_length"] > 0).sum())
            assert (pg.frames, pg.failed, pg.pixels, pg.history_pixels) == (k + 1, 0, 320 * 240, with_history), k
            assert (with_history == 0) == (k == 0)                                         # frame 0 has none; the move leaves most pixels theirs
            assert st.camera_samples == 320 * 240 * MODES[mode][0]
        assert with_history > 320 * 240 // 4                                              # about half the view is ground and mesh, and the move is small
        if MODES[mode][4]:                                                                 # the moved node is seen, and its motion changed the frame
            assert (ref[2]["node"] == sc.node_index("ball")).any() and ref[2]["node"].tobytes() != ref[0]["node"].tobytes()
        sc.temporal_end()
    finally:
        sc.close()


@pytest.mark.gpu
def test_reset_end_begin_and_free_with_an_open_session(B, chain):
    ref = chain("spatial")
    sc = B.Scene(XML)
    try:
        sc.temporal_begin(*_opts(B, "spatial"))
        for k in range(2):
            _set_frame(B, sc, "spatial", k, None)
            sc.temporal_frame()
        before = sc.temporal_image_dev(B.TEMPORAL_IMG_ACCUMULATED)
        sc.temporal_reset()                                                                # a cut: frame 0 again, seed + 0, no history
        assert sc.temporal_status().frames == 0
        with pytest.raises(B.BhrtError, match="no frame since"):
            sc.temporal_image(B.TEMPORAL_IMG_ACCUMULATED)
        _set_frame(B, sc, "spatial", 0, None)
        rgb, rad, _ = sc.temporal_frame()
        _same(dict(_kept(B, sc), shown=rad, rgb8=rgb), ref[0], "after reset")
        assert before and sc.temporal_image_dev(B.TEMPORAL_IMG_ACCUMULATED)
        sc.temporal_end()
        sc.temporal_end()                                                                  # fine when none is open
        sc.temporal_begin(*_opts(B, "spatial"))                                            # end, then begin: a fresh session
        rgb, rad, _ = sc.temporal_frame()
        _same(dict(_kept(B, sc), shown=rad, rgb8=rgb), ref[0], "after end and begin")
    finally:
        sc.close()                                                                         # bhrt_scene_free with the session open
    # the freed session's images are gone with it: sessions opened and freed over and over do not run the device out of memory
    for _ in range(3):
        sc = B.Scene(XML)
        try:
            sc.temporal_begin(*_opts(B, "spatial"))
            _set_frame(B, sc, "spatial", 0, None)
            rgb, rad, _ = sc.temporal_frame()
            assert rgb.tobytes() == ref[0]["rgb8"].tobytes()
        finally:
            sc.close()
    sc = B.Scene(XML)
    try:                                                                                   # an allocation-heavy call afterwards still gets its memory
        assert sc.render(B.default_opts(spp=8, seed=1))[2].camera_samples == 320 * 240 * 8
    finally:
        sc.close()


@pytest.mark.gpu
def test_other_calls_between_two_frames_do_not_disturb_the_session(B, chain):
    ref = chain("spatial")
    sc = B.Scene(XML)
    try:
        sc.temporal_begin(*_opts(B, "spatial"))
        for k in range(FRAMES):
            if k == 2:                                                                     # between frames 1 and 2, at frame 1's camera
                _, rad, var = sc.render_var(B.default_opts(spp=3, seed=99))
                sc.denoise(B.default_denoise_opts(iterations=2), rad, var)                 # computes its own guides in the scene's scratch
                sc.first_hit()
                sc.first_hit_node()
            _set_frame(B, sc, "spatial", k, None)                                          # the camera is all the host sets
            rgb, rad, _ = sc.temporal_frame()
        _same(dict(_kept(B, sc), shown=rad, rgb8=rgb), ref[2], "frame 2")
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["light", "denoise"])
def test_the_device_variant_equals_the_host_variant(B, chain, mode):
    import torch
    ref = chain(mode)
    sc = B.Scene(XML)
    try:
        sc.temporal_begin(*_opts(B, mode))
        rgb = torch.full((240, 320, 3), 7, dtype=torch.uint8, device="cuda")
        rad = torch.full((240, 320, 3), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(FRAMES):
            _set_frame(B, sc, mode, k, None)
            if k == 1:                                                                     # either pointer may be NULL
                sc.temporal_frame_dev(0, 0)
                continue
            sc.temporal_frame_dev(rgb.data_ptr(), rad.data_ptr())                          # synchronised when it returns
            assert rgb.cpu().numpy().tobytes() == ref[k]["rgb8"].tobytes() and rad.cpu().numpy().tobytes() == ref[k]["shown"].tobytes(), k
        _same(_kept(B, sc), {k: v for k, v in ref[2].items() if k not in ("shown", "rgb8")}, "kept")
    finally:
        sc.close()


@pytest.mark.gpu
def test_a_one_frame_session_is_render_var_and_denoise(B):
    sc, ref = B.Scene(XML), B.Scene(XML)
    try:
        o, t = _opts(B, "denoise")
        sc.temporal_begin(o, t)
        rgb, rad, _ = sc.temporal_frame()
        _, cur, var = ref.render_var(o)
        out, out_rgb = ref.denoise(B.default_denoise_opts(), cur, var)
        assert rad.tobytes() == out.tobytes() and rgb.tobytes() == out_rgb.tobytes()
        assert sc.temporal_image(B.TEMPORAL_IMG_ACCUMULATED).tobytes() == cur.tobytes() and sc.temporal_image(B.TEMPORAL_IMG_VARIANCE).tobytes() == var.tobytes()
        sc.temporal_end()
        sc.temporal_begin(B.default_opts(spp=2, seed=SEED), B.default_temporal_session_opts())   # light only: the frame is bhrt_render's
        rgb, rad, _ = sc.temporal_frame()
        ref_rgb, ref_rad, _ = ref.render(o)
        assert rad.tobytes() == ref_rad.tobytes() and rgb.tobytes() == ref_rgb.tobytes()
    finally:
        sc.close()
        ref.close()


@pytest.mark.gpu
def test_cli_frames_equal_the_python_session(B, tmp_path):
    """bhrt render --temporal 3 --denoise --spatial-variance --spp 1 --frames-png writes the frames of the Python session."""
    from test_cli_temporal import POSE0 as CLI_POSE0, POSE_FLAGS, TO_POS, XML as CLI_XML
    png, prefix = str(tmp_path / "last.png"), str(tmp_path / "frame_")
    out = _run(["render", CLI_XML, "-o", png, "--spp", "1", "--seed", "5", "--frames-png", prefix, "--temporal", "3", "--denoise", "--spatial-variance"] + POSE_FLAGS, SCENES)
    frames = [_png(prefix + "%03d.png" % k) for k in range(3)]
    p0, p1 = np.float32(CLI_POSE0).reshape(-1), np.float32((TO_POS,) + CLI_POSE0[1:]).reshape(-1)
    sc = B.Scene(CLI_XML)
    try:
        sc.temporal_begin(B.default_opts(spp=1, seed=5), B.default_temporal_session_opts(carry_variance=1, spatial_variance=1, denoise=1))
        for k in range(3):
            p = (p0 + (p1 - p0) * (f32(k) / f32(2))).astype(f32)
            sc.set_camera(p[0:3], p[3:6], p[6:9])
            rgb = sc.temporal_frame(want_radiance=False)[0]
            assert np.array_equal(rgb, frames[k]), k
            pg = sc.temporal_status()
            assert "frame %d: camera %g,%g,%g, history on %.1f%% of the pixels" % (k, p[0], p[1], p[2], 100.0 * pg.history_pixels / pg.pixels) in out
    finally:
        sc.close()
