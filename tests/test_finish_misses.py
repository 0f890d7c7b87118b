"""Rays that miss, finished where they are traced (DESIGN.md 4 "Finish misses in the closest-hit kernel", knob "finish_misses" = 1, the default):
k_trace_closest stores the value of an unparked GI miss into its owner frame and the no-root-frame mark of an unparked camera miss into the
slot -> root frame map, and files neither for k_shade.  Knob 0 files every ray, as before.  The two owe each other the same bits: one copy of
the miss arithmetic (gi_miss), the same frames in the same order, the same queue lengths.

Every case renders with the knob at 1 and at 0 and compares the radiance, the RGB8 image and every field of bhrt_stats except the seconds_*
ones; the first two cases also against the oracle's keyed-mode render.  Nothing in bhrt_stats tells the two paths apart (that is the point:
the host's bookkeeping comes from queue lengths and frame counts), so every case asserts the premise that puts the rays it is named after
into the frame."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES, same_bits

pytestmark = pytest.mark.gpu

SWITCHES = ("BHRT_STREAM_WAVES", "BHRT_SHADOW_OVERLAP", "BHRT_FINISH_MISSES")

# three meshes of two kinds, one of them glass, in front of two walls (the scene of tests/test_switch_paths.py, restated)
THREE_MESHES_XML = """<xml><scene><background r="0.1" g="0.1" b="0.2"/><environment value="0.4"/>
  <object type="plane" name="floor" material="wall"><scale value="14"/></object>
  <object type="plane" name="back" material="wall"><scale value="14"/><rotate angle="90" x="1"/><translate y="9" z="6"/></object>
  <object type="obj" name="mesh_small.obj" material="glass"><scale value="2.2"/><translate x="-3" y="1" z="2.4"/></object>
  <object type="obj" name="mesh_b.obj" material="red"><scale x="2.5" y="2" z="2.8"/><rotate angle="35" z="1"/><translate x="2.5" y="3" z="2.9"/></object>
  <object name="grp"><rotate angle="-20" z="1"/><translate x="0.5" y="-2.5" z="0"/>
    <object type="obj" name="mesh_small.obj" material="red"><scale value="1.3"/><translate z="1.4"/></object>
    <object type="sphere" name="s" material="mirror"><scale value="0.9"/><translate x="2.6" z="0.9"/></object>
  </object>
  <material type="blinn" name="wall"><diffuse r="0.7" g="0.7" b="0.65"/><specular value="0.1"/><glossiness value="20"/></material>
  <material type="blinn" name="red"><diffuse r="0.8" g="0.25" b="0.2"/><specular value="0.5"/><glossiness value="60"/></material>
  <material type="blinn" name="mirror"><diffuse value="0.05"/><specular value="0.9"/><glossiness value="2000"/></material>
  <material type="blinn" name="glass"><diffuse value="0.05"/><specular value="0.8"/><glossiness value="80"/><refraction value="0.85" index="1.5"/><absorption r="0.05" g="0.02" b="0.1"/></material>
  <light type="point" name="p"><intensity value="260"/><position x="-2" y="-9" z="14"/><size value="1.5"/></light>
  <light type="ambient" name="a"><intensity value="0.1"/></light>
  </scene><camera><position x="0.5" y="-17" z="6.5"/><target x="0" y="1" z="2.2"/><up z="1"/><fov value="38"/><width value="125"/><height value="93"/></camera></xml>"""

# the camera straight above an unrotated mesh: without jitter the rays of the image's middle column and middle row are parallel to a coordinate
# plane of the mesh's space, which is what the render path sets aside (the scene of test_axis_parallel_rays_take_wave_steps_of_their_own)
ABOVE_XML = """<xml><scene><background r="0.1" g="0.1" b="0.2"/><environment r="0.4" g="0.4" b="0.5"/>
  <object type="plane" name="floor" material="w"><scale value="20"/></object>
  <object type="obj" name="mesh_small.obj" material="g"><scale value="3"/><translate z="4"/></object>
  <object type="sphere" name="s" material="r"><scale value="1.5"/><translate x="6" y="2" z="1.5"/></object>
  <material type="blinn" name="w"><diffuse value="0.8"/><specular value="0.1"/></material>
  <material type="blinn" name="r"><diffuse r="0.8" g="0.2" b="0.2"/><specular value="0.4"/><glossiness value="20"/></material>
  <material type="blinn" name="g"><diffuse value="0.05"/><specular value="0.5"/><glossiness value="60"/><refraction value="0.9" index="1.5"/></material>
  <light type="point" name="p"><intensity value="300"/><position x="3" y="-4" z="18"/><size value="1"/></light></scene>
  <camera><position x="0" y="0" z="30"/><target x="0" y="0" z="0"/><up x="0" y="1" z="0"/><fov value="40"/><width value="64"/><height value="48"/></camera></xml>"""


@pytest.fixture(scope="module")
def gpu(B):
    if B.device_count() < 1:
        pytest.fail("no HIP device: the render path has no CPU fallback, GPU tests cannot run here")
    return B


def _resized(name, w, h):
    txt = open(os.path.join(SCENES, name + ".xml")).read()
    txt, n1 = re.subn(r'<width value="\d+"/>', f'<width value="{w}"/>', txt)
    txt, n2 = re.subn(r'<height value="\d+"/>', f'<height value="{h}"/>', txt)
    assert n1 == 1 and n2 == 1
    return txt


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    """The module's scene files beside the assets they name: key -> path of the XML."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_mesh
    d = tmp_path_factory.mktemp("finish_misses")
    for asset in ("mesh_small.obj", "tex_small.png", "tex_small.ppm"):
        shutil.copy(os.path.join(SCENES, asset), d / asset)
    gen_mesh.generate(str(d / "mesh_b.obj"), 20)  # 800 triangles; mesh_small.obj has 288
    texts = {
        "three_meshes": THREE_MESHES_XML,
        "above": ABOVE_XML,
        "c4_textured_144": _resized("c4_textured", 144, 108),
        "c3_mesh_77": _resized("c3_mesh_small", 77, 45),
        "c3_mesh_96": _resized("c3_mesh_small", 96, 72),
    }
    out = {}
    for key, txt in texts.items():
        (d / (key + ".xml")).write_text(txt)
        out[key] = str(d / (key + ".xml"))
    for name in ("c3_mesh_small", "c2_glass_small", "lens_mesh_small"):
        out[name] = os.path.join(SCENES, name + ".xml")
    return out


@pytest.fixture
def fresh(gpu, monkeypatch, scene_dir):
    """fresh(key, env) -> a private scene handle (the knob is state of a handle: none of conftest's shared ones), uploaded with exactly the
    switches of `env` in the environment (they are read once, at upload); closed when the test is done."""
    made = []

    def _get(key, env=None):
        env = env or {}
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for k, v in env.items():
            assert k in SWITCHES
            monkeypatch.setenv(k, str(v))
        try:
            sc = gpu.Scene(scene_dir[key])
            sc.upload(0)
        finally:
            for k in env:
                monkeypatch.delenv(k)
        made.append(sc)
        return sc
    yield _get
    for sc in made:
        sc.close()


def _both(sc, render):
    """render(sc) with the knob at 1 and at 0 -> (result with the misses finished in the trace kernel, result with every ray filed)."""
    try:
        sc.knob("finish_misses", 1)
        a = render(sc)
        sc.knob("finish_misses", 0)
        b = render(sc)
    finally:
        sc.knob("finish_misses", 1)
    return a, b


def _diff(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    return f"{int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:8].tolist()}"


def _counters(st):
    return {k: v for k, v in st.as_dict().items() if not k.startswith("seconds_")}


def _same_frame(a, b):
    """(rgb8, radiance, stats) of two renders: the same bytes, the same floats, the same counters."""
    (rgb, rad, st), (rgb0, rad0, st0) = a, b
    assert same_bits(rad, rad0), "radiance: " + _diff(rad, rad0)
    assert np.array_equal(rgb, rgb0)
    assert _counters(st) == _counters(st0)


def _check_ab(sc, opts):
    a, b = _both(sc, lambda s: s.render(opts))
    _same_frame(a, b)
    assert a[2].passes >= 1 and a[2].launches_resolve_fused == a[2].passes  # the plain render: camera misses go through the slot -> root frame map
    return a


def _primary_nodes(gpu, O, sc):
    o, d = O.primary_rays(sc.flat_view())
    h = sc.trace_closest(o, d, gpu.SIDE_FRONT)
    return h["node"], h["prim"]


def _check_oracle(O, sc, rgb, rad, spp, gi, seed):
    ro = O.render(sc.flat_bytes(), sc.width, sc.height, spp, gi=gi, seed=seed, threads=16, want_samples=False)
    assert same_bits(rad, ro["radiance"]), "against the oracle: " + _diff(rad, ro["radiance"])
    assert np.array_equal(rgb, ro["rgb8"])
    return ro


def test_mesh_scene_parked_and_unparked_misses(gpu, O, fresh):
    """Case 1.  The open mesh scene: camera rays and GI rays that pass the mesh's root box are parked and miss later (filed, as before), those that
    pass beside it miss in k_trace_closest<park> (finished there), in one and the same wave step."""
    sc = fresh("c3_mesh_small")
    node, prim = _primary_nodes(gpu, O, sc)
    assert sc.info.n_meshes > 0 and (node < 0).sum() > 1000 and (prim >= 0).sum() > 1000  # camera misses, and a mesh in view
    assert sc.flat_view().header.environment.map < 0                                      # a plain colour: the switch is on
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=4, gi_bounces=3, seed=12))
    assert st.closest_rays > 2 * st.shade_calls  # most GI rays open no frame: they leave the scene
    _check_oracle(O, sc, rgb, rad, 4, 3, 12)


def test_scene_without_meshes_gi_branch_only(gpu, O, fresh):
    """Case 2.  No mesh: the camera step is k_shade's fused form (no trace kernel in front of it), so only GI misses are finished, in
    k_trace_closest<false, false, false>; the refraction rays that leave the glass and miss stay filed for k_shade."""
    sc = fresh("c2_glass_small")
    fv = sc.flat_view()
    assert sc.info.n_meshes == 0 and any(m.refraction.color[0] > 0 for m in fv.materials)
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=4, gi_bounces=3, seed=12))
    assert st.launches_trace_closest == st.wave_iterations - 1  # the fused camera step launches none
    _check_oracle(O, sc, rgb, rad, 4, 3, 12)


@pytest.mark.parametrize("env", [{}, {"BHRT_SHADOW_OVERLAP": 0, "BHRT_STREAM_WAVES": 0}], ids=["default", "no_overlap_no_stream"])
def test_three_mesh_instances(gpu, fresh, env):
    """Case 3.  Several mesh nodes: a ray parks at the first root box it enters, whatever lies behind; only a ray that enters none is finished.
    Also with the any-hit kernels on the pass's own stream and the launch-per-64-rays walk kernels."""
    sc = fresh("three_meshes", env)
    assert sc.info.n_meshes >= 2 and (sc.width, sc.height) == (125, 93)
    _check_ab(sc, gpu.default_opts(spp=4, gi_bounces=3, seed=21))


def test_lens_rays_from_the_queue(gpu, O, fresh):
    """Case 4.  lens = 1: the camera rays come from the queue (k_lens_rays) and go through k_trace_closest<park, false> as rays of kind
    RK_CAMERA; the slot of a miss is the ray's frame word."""
    sc = fresh("lens_mesh_small")
    node, _ = _primary_nodes(gpu, O, sc)
    assert (node < 0).sum() > 100 and sc.info.n_meshes > 0
    opts = gpu.default_opts(spp=4, gi_bounces=3, seed=4, lens=1)
    rgb, rad, st = _check_ab(sc, opts)
    pin = sc.render(gpu.default_opts(spp=4, gi_bounces=3, seed=4))
    assert not same_bits(rad, pin[1])  # the aperture is open


def test_textured_environment_takes_the_old_path(gpu, O, fresh):
    """Case 5.  c4_textured's environment is a texture: the value of a GI miss needs texture code, so the host leaves finishing off for the whole
    render, camera misses included; knob 1 and knob 0 launch the same kernels with the same arguments."""
    sc = fresh("c4_textured_144")
    fv = sc.flat_view()
    node, _ = _primary_nodes(gpu, O, sc)
    assert fv.header.environment.map >= 0 and fv.header.n_texmaps > 0 and (node < 0).sum() > 100
    _check_ab(sc, gpu.default_opts(spp=3, gi_bounces=2, seed=2))


def test_renders_that_keep_the_sample_buffer(gpu, O, fresh):
    """Case 6.  Region samples and the variance image read the per-sample buffer: there is no slot -> root frame map, a camera miss stays filed
    and k_shade stores its background sample; GI misses are finished all the same."""
    sc = fresh("lens_mesh_small")
    node, _ = _primary_nodes(gpu, O, sc)
    miss = (node < 0).reshape(sc.height, sc.width)
    opts = gpu.default_opts(spp=4, gi_bounces=3, seed=7)
    region = (10, 8, 90, 66)
    x0, y0, x1, y1 = region
    assert miss[y0:y1, x0:x1].sum() > 100
    (gs, st), (gs0, st0) = _both(sc, lambda s: s.render_samples(opts, *region))
    assert st.launches_resolve_fused == 0 and st0.launches_resolve_fused == 0
    assert gs.shape == ((x1 - x0) * (y1 - y0), 4, 3) and same_bits(gs, gs0), _diff(gs, gs0)
    assert _counters(st) == _counters(st0)
    bg = np.asarray(list(sc.flat_view().header.background.color), np.float32)
    assert int(np.all(gs.view(np.uint32) == bg.view(np.uint32), axis=-1).sum()) > 100  # k_shade stored the background sample of the camera misses
    v, v0 = _both(sc, lambda s: s.render_var(opts))
    assert np.array_equal(v[0], v0[0]) and same_bits(v[1], v0[1]) and same_bits(v[2], v0[2]) and v[2].any()
    rgb, rad, _ = _check_ab(sc, opts)  # and the plain render of the same frame agrees with both
    assert np.array_equal(rgb, v[0]) and same_bits(rad, v[1])


def test_edge_tiles_as_rank_1_of_3(gpu, fresh):
    """Case 7.  77 x 45 pixels in 32-pixel tiles, rank 1 of 3: the rank's tiles on the right and bottom edge stick out of the image; their slots
    are dead, and a dead slot is neither a miss to finish nor a ray to file."""
    sc = fresh("c3_mesh_77")
    w, h, spp = sc.width, sc.height, 4
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=spp, gi_bounces=3, seed=3, rank=1, world_size=3, tile_size=32))
    tiles_x, tiles_y = (w + 31) // 32, (h + 31) // 32
    mine = np.zeros((h, w), bool)
    n_slots = 0
    for t in range(1, tiles_x * tiles_y, 3):
        ty, tx = divmod(t, tiles_x)
        mine[ty * 32:(ty + 1) * 32, tx * 32:(tx + 1) * 32] = True
        n_slots += 32 * 32
    assert 0 < st.camera_samples == int(mine.sum()) * spp < n_slots * spp  # the premise: dead slots
    assert not rad[~mine].any() and not rgb[~mine].any()


def test_pass_that_overflows_and_is_redone_in_halves(gpu, fresh):
    """Case 8.  The frame pool at a third of what the frame needs: the pass overflows part-way, after its trace kernels have written GI values
    and map entries, and is redone in halves, which writes them again.  A scene remembers the pass size that fitted, so each side gets a
    handle of its own and meets the overflow itself."""
    opts = gpu.default_opts(spp=4, gi_bounces=3, seed=9)
    out = []
    for knob in (1, 0):
        sc = fresh("c3_mesh_96")
        sc.knob("finish_misses", knob)
        base = sc.render(opts)
        assert base[2].passes == 1
        sc.knob("frame_cap", max(1, int(base[2].shade_calls) // 3))
        try:
            capped = sc.render(opts)
        finally:
            sc.knob("frame_cap", 0)
        assert capped[2].passes >= 3
        assert np.array_equal(capped[0], base[0]) and same_bits(capped[1], base[1])
        out.append((base, capped))
    _same_frame(out[0][0], out[1][0])
    _same_frame(out[0][1], out[1][1])


def test_axis_parallel_rays_are_neither_finished_nor_lost(gpu, O, fresh):
    """Case 9.  The camera straight above an unrotated mesh, no jitter: the middle row and column are set aside to the slow queue by the camera
    step's trace kernel, with whatever hit they had so far — often none.  They are not rays of that step any more: not finished there, not
    filed, and shaded once, in the step that moves them back in."""
    sc = fresh("above")
    o, d = O.primary_rays(sc.flat_view())
    assert ((d == 0).sum(axis=1) >= 1).sum() >= 64 + 48 - 1  # the premise: the middle column and row are axis-parallel rays
    opts = gpu.default_opts(spp=2, gi_bounces=2, seed=6, jitter=0)
    rgb, rad, st = _check_ab(sc, opts)
    assert st.deferred_rays >= 30 * 2  # those that enter the mesh's root box were set aside
    (gs, s1), (gs0, s0) = _both(sc, lambda s: s.render_samples(opts, 0, 0, s.width, s.height))
    assert same_bits(gs, gs0) and _counters(s1) == _counters(s0)
    ro = O.render(sc.flat_bytes(), sc.width, sc.height, 2, gi=2, seed=6, jitter=0)
    assert same_bits(gs, ro["samples"])
