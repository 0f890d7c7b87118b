"""The wavefront's switchable paths and queue edges against the oracle (DESIGN.md 5 maps every instantiation and switch to its test here).

device_state.h says of the development switches "none changes a result".  They are read from the environment ONCE, when a scene is
uploaded (Knobs::FromEnv), so every case below sets the variable, loads a FRESH scene (not conftest's cached load_scene), uploads it, and
removes the variable again; the default path renders a second fresh scene of the same XML.  Every comparison is on bits: per-sample
radiance of the switched path against the oracle's and against the default path's, and closest_rays / shadow_rays / shade_calls against
the default path's.  Every test asserts the premise that makes it reach the path it is named after, so a case that silently takes the
default path fails instead of passing.

The scene texts are the ones of test_gpu_parity.py (three meshes in a closed box, two refractive meshes, the camera above a mesh, the
48-level chain), restated here with frame sizes that make the wave steps ragged.

What this module found when it was added: k_file_all filed a ride-along's rays from an unaligned first slot, so a wave could straddle a 1024-slot
shard boundary with a shard that was not wave-uniform (file_ray's contract); the 1080p slow-queue test below differed from the oracle in ~160 pixels,
differently from run to run.  Fixed in kernels.hip (waves cover aligned runs of 64 slots).

The constants below restate the library's and only serve to assert premises, never to compute an expected value."""
import os
import re
import shutil

import numpy as np
import pytest

from conftest import SCENES, ensure_mesh, same_bits

pytestmark = pytest.mark.gpu

K_SLOW_CAP = 1 << 16        # kernels.hip kSlowCap: rays set aside per pass
INJECT_MIN_RAYS = 1 << 20   # kernels.hip kInjectMinRays (BHRT_INJECT_MIN_LOG2 20): a batch rides along only with a step of at least this many rays
GATHER_SORT_MIN = 1 << 16   # kernels.hip GatherPass::OrderByCell: the gather sorts its queries by cell only from this many queries on
PATH16_MAX_NODES = 1 << 17  # kernels.hip PathMode: 16-bit path entries up to this many BVH nodes, 32-bit above
PATH_MAX_DEPTH = 32         # kernels.hip PathMode: deeper trees walk parent links (no path in LDS, leaf_skip not compiled in)

SWITCHES = ("BHRT_STREAM_WAVES", "BHRT_FUSED_CAMERA", "BHRT_NO_SLOW_QUEUE", "BHRT_DEBUG_SLOW", "BHRT_GATHER_COUNTING_SORT", "BHRT_SHADOW_OVERLAP")

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

TWO_MESHES_XML = """<xml><scene>
  <background r="0.1" g="0.1" b="0.2"/><environment r="0.5" g="0.5" b="0.6"/>
  <object type="sphere" name="s0" material="red"><scale value="1.2"/><translate x="-5" y="1" z="1.2"/></object>
  <object type="obj" name="mesh_small.obj" material="glass"><scale value="2.5"/><translate x="-1.5" y="0" z="3"/></object>
  <object type="plane" name="ground" material="white"><scale value="25"/></object>
  <object name="grp"><rotate angle="35" z="1"/><translate x="3" y="2" z="0"/>
    <object type="obj" name="mesh_small.obj" material="blue"><scale x="2" y="1.5" z="2.2"/><rotate angle="20" x="1"/><translate z="2.6"/></object>
    <object type="sphere" name="s1" material="red"><scale value="0.8"/><translate x="2.5" z="0.8"/></object>
  </object>
  <material type="blinn" name="white"><diffuse value="0.8"/><specular value="0.1"/></material>
  <material type="blinn" name="red"><diffuse r="0.8" g="0.2" b="0.2"/><specular value="0.5"/><glossiness value="20"/></material>
  <material type="blinn" name="blue"><diffuse r="0.2" g="0.3" b="0.8"/><specular value="0.6"/><glossiness value="40"/></material>
  <material type="blinn" name="glass"><diffuse value="0.05"/><specular value="0.6"/><glossiness value="60"/>
    <refraction value="0.9" index="1.5"/><absorption r="0.02" g="0.05" b="0.02"/></material>
  <light type="ambient" name="a"><intensity value="0.1"/></light>
  <light type="point" name="p"><intensity value="250"/><position x="2" y="-8" z="16"/><size value="1.5"/></light>
  </scene><camera><position x="1" y="-22" z="9"/><target x="0" y="0" z="2.5"/><up z="1"/><fov value="35"/>
  <width value="149"/><height value="111"/></camera></xml>"""

# the camera straight above an unrotated mesh: without jitter the rays of the image's middle column and middle row are parallel to a coordinate
# plane of the mesh's space (a zero direction component), which is what the render path sets aside (device_trace.h::trace_closest, park_slow)
ABOVE_XML = """<xml><scene><background r="0.1" g="0.1" b="0.2"/><environment r="0.4" g="0.4" b="0.5"/>
  <object type="plane" name="floor" material="w"><scale value="20"/></object>
  <object type="obj" name="mesh_small.obj" material="g"><scale value="@SCALE@"/><translate z="@Z@"/></object>
  <object type="sphere" name="s" material="r"><scale value="1.5"/><translate x="6" y="2" z="1.5"/></object>
  <material type="blinn" name="w"><diffuse value="0.8"/><specular value="0.1"/></material>
  <material type="blinn" name="r"><diffuse r="0.8" g="0.2" b="0.2"/><specular value="0.4"/><glossiness value="20"/></material>
  <material type="blinn" name="g"><diffuse value="0.05"/><specular value="0.5"/><glossiness value="60"/><refraction value="0.9" index="1.5"/></material>
  <light type="point" name="p"><intensity value="300"/><position x="3" y="-4" z="18"/><size value="1"/></light></scene>
  <camera><position x="0" y="0" z="30"/><target x="0" y="0" z="0"/><up x="0" y="1" z="0"/><fov value="40"/><width value="@W@"/><height value="@H@"/></camera></xml>"""

CHAIN_XML = """<xml><scene><background r="0.1" g="0.1" b="0.2"/><environment r="0.5" g="0.5" b="0.5"/>
  <object type="plane" name="g" material="g"><scale value="50"/></object>
  <object type="obj" name="chain.obj" material="m"><scale x="0.00002" y="8" z="8"/><translate x="-6"/></object>
  <object type="sphere" name="s" material="m"><translate x="3" z="1"/></object>
  <material type="blinn" name="g"><diffuse r="0.7" g="0.7" b="0.7"/><specular value="0"/></material>
  <material type="blinn" name="m"><diffuse r="0.8" g="0.3" b="0.2"/><specular value="0.4"/><glossiness value="30"/></material>
  <light type="point" name="l"><intensity value="200"/><position x="2" y="-8" z="12"/><size value="1"/></light></scene>
  <camera><position x="0" y="-22" z="6"/><target x="0" y="0" z="2"/><up z="1"/><fov value="50"/><width value="127"/><height value="71"/></camera></xml>"""


def _above_xml(w, h, scale=3, z=4):
    return ABOVE_XML.replace("@W@", str(w)).replace("@H@", str(h)).replace("@SCALE@", str(scale)).replace("@Z@", str(z))


def _resized(name, w, h):
    """A committed scene's text with another frame size."""
    txt = open(os.path.join(SCENES, name + ".xml")).read()
    txt, n1 = re.subn(r'<width value="\d+"/>', f'<width value="{w}"/>', txt)
    txt, n2 = re.subn(r'<height value="\d+"/>', f'<height value="{h}"/>', txt)
    assert n1 == 1 and n2 == 1
    return txt


@pytest.fixture(scope="module")
def gpu(B):
    if B.device_count() < 1:
        pytest.fail("no HIP device: the render path has no CPU fallback, GPU tests cannot run here")
    return B


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """The module's scene files, written once: name -> path of the XML."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_mesh
    d = tmp_path_factory.mktemp("switch_paths")
    for asset in ("mesh_small.obj", "tex_small.png", "tex_small.ppm"):
        shutil.copy(os.path.join(SCENES, asset), d / asset)
    gen_mesh.generate(str(d / "mesh_b.obj"), 20)  # 800 triangles; mesh_small.obj has 288
    with open(d / "chain.obj", "w") as fp:  # triangles at exponentially spaced positions: MeanSplit peels off two at a time, 48 levels
        n = 100
        for k in range(n):
            x = 1.6 ** k * 1e-6
            fp.write(f"v {x!r} -0.3 {0.2 + 0.001 * k!r}\nv {x * 1.05!r} 0.3 {0.2!r}\nv {x!r} 0.0 {0.6 + 0.002 * k!r}\n")
        fp.write("vt 0 0 0\nvn 0 -1 0\n")
        for k in range(n):
            fp.write(f"f {3 * k + 1}/1/1 {3 * k + 2}/1/1 {3 * k + 3}/1/1\n")
    ensure_mesh(400)  # 320,000 triangles, > 2^17 BVH nodes (tests/scenes/gen, git-ignored)
    os.symlink(os.path.join(SCENES, "gen"), d / "gen")
    c4 = _resized("c4_textured", 288, 216)
    # c4_textured holds one mesh node; the two-kernel camera step only exists in scenes without meshes, so this variant leaves the node out
    c4, n_cut = re.subn(r'<object type="obj".*?</object>\s*', "", c4, flags=re.S)
    assert n_cut == 1
    texts = {
        "three_meshes": THREE_MESHES_XML,
        "two_meshes": TWO_MESHES_XML,
        "c3_mesh_small": _resized("c3_mesh_small", 159, 119),
        "c3_room_small": _resized("c3_room_small", 141, 107),
        "big_mesh": open(os.path.join(SCENES, "c3_mesh.xml")).read().replace("gen/mesh_224.obj", "gen/mesh_400.obj")
                    .replace('<width value="1920"/>', '<width value="480"/>').replace('<height value="1080"/>', '<height value="270"/>'),
        "chain": CHAIN_XML,
        "c1_sphere_plane": _resized("c1_sphere_plane", 317, 239),
        "c2_glass_small": _resized("c2_glass_small", 320, 180),
        "c4_textured_no_mesh": c4,
        "above_small": _above_xml(64, 48),
        "above_full": _above_xml(1920, 1080, scale=6, z=10),
        "c5_caustics": _resized("c5_caustics", 320, 240),
    }
    out = {}
    for name, txt in texts.items():
        (d / (name + ".xml")).write_text(txt)
        out[name] = str(d / (name + ".xml"))
    return out


def _fresh_scene(B, monkeypatch, xml, env):
    """A new scene uploaded with exactly the switches of `env` in the environment (Knobs::FromEnv runs at upload), which is clean again on return."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        assert k in SWITCHES
        monkeypatch.setenv(k, str(v))
    try:
        sc = B.Scene(xml)
        sc.upload(0)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return sc


def _diff(a, b):
    """For assertion messages: how many float32 values of two arrays differ in their bits, and where the first ones are."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    return f"{int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:8].tolist()}"


def _counts(st):
    return (st.camera_samples, st.closest_rays, st.shadow_rays, st.shade_calls)


_default_scenes = {}  # xml -> the default path's scene (fresh: never one of conftest's cached scenes, never uploaded with a switch set)
_bases = {}           # (xml, region, options) -> (default path's samples, its counts, its stats, the oracle's samples)


def _default_scene(B, monkeypatch, xml):
    if xml not in _default_scenes:
        _default_scenes[xml] = _fresh_scene(B, monkeypatch, xml, {})
    return _default_scenes[xml]


def _base(B, O, monkeypatch, xml, region=None, **kw):
    """The default path's render of `xml` with options kw (leaf_skip = 0) and the oracle's render of the same samples; the two are compared here."""
    key = (xml, region, tuple(sorted(kw.items())))
    if key not in _bases:
        sc = _default_scene(B, monkeypatch, xml)
        reg = region or (0, 0, sc.width, sc.height)
        gs, st = sc.render_samples(B.default_opts(**kw), *reg)
        ro = O.render(sc.flat_bytes(), sc.width, sc.height, kw["spp"], gi=kw["gi_bounces"], seed=kw["seed"], jitter=kw.get("jitter", 1), region=reg, threads=16)["samples"]
        assert gs.shape == ro.shape and same_bits(gs, ro), f"the DEFAULT path differs from the oracle: {_diff(gs, ro)}"
        _bases[key] = (gs, _counts(st), st, ro)
    return _bases[key]


def _check_switched(B, O, monkeypatch, xml, env, region=None, sc=None, leaf_skip=0, **kw):
    """Renders `xml` on a fresh scene uploaded under `env` (or on `sc`) and holds samples and ray counts to the oracle and to the default path.
    Returns (stats of the switched render, stats of the default render, the switched scene)."""
    d_gs, d_counts, d_st, ro = _base(B, O, monkeypatch, xml, region, **kw)
    if sc is None:
        sc = _fresh_scene(B, monkeypatch, xml, env)
    reg = region or (0, 0, sc.width, sc.height)
    gs, st = sc.render_samples(B.default_opts(leaf_skip=leaf_skip, **kw), *reg)
    assert gs.shape == ro.shape
    assert same_bits(gs, ro), f"{env} leaf_skip={leaf_skip}: differs from the oracle: {_diff(gs, ro)}"
    assert same_bits(gs, d_gs), f"{env} leaf_skip={leaf_skip}: differs from the default path: {_diff(gs, d_gs)}"
    assert _counts(st) == d_counts, (env, leaf_skip, _counts(st), d_counts)
    return st, d_st, sc


MESH_SCENES = ["three_meshes", "two_meshes", "c3_mesh_small", "c3_room_small"]
MESH_OPTS = dict(spp=3, gi_bounces=3, seed=21)  # 125 x 93, 149 x 111, 159 x 119, 141 x 107 pixels x 3 samples: no step is a multiple of 64 rays by construction


# ---------------------------------------------------------------------------------------------------- the streamed mesh walk
@pytest.mark.parametrize("name", MESH_SCENES)
@pytest.mark.parametrize("waves", [1, 2, 7])
def test_streamed_mesh_walk_refills_its_waves_from_the_cursor(gpu, O, monkeypatch, scenes, name, waves):
    """k_trace_mesh_stream<1> with 1, 2 and 7 resident waves (BHRT_STREAM_WAVES): every wave takes batch after batch from the cursor, refills when
    32 of its lanes are free, meets the ragged last batch, and — three meshes of two kinds, one of them glass, in a closed box; two refractive
    meshes; the closed room — holds lanes that wait at one mesh node while the wave walks another mesh, across refills.  With the default of several
    thousand waves each wave of these frames takes one batch and leaves.  Every sample of the frame."""
    st, d_st, sc = _check_switched(gpu, O, monkeypatch, scenes[name], {"BHRT_STREAM_WAVES": waves}, **MESH_OPTS)
    assert sc.info.n_meshes >= 1 and sc.info.max_bvh_depth <= PATH_MAX_DEPTH and sc.info.n_bvh_nodes <= PATH16_MAX_NODES
    assert st.closest_rays - st.camera_samples > 64 * waves * 20  # the premise: many times what the resident waves hold at once
    assert (sc.width * sc.height * MESH_OPTS["spp"]) % 64 != 0
    sc.close()


@pytest.mark.parametrize("name", MESH_SCENES)
def test_launch_per_64_rays_mesh_kernels(gpu, O, monkeypatch, scenes, name):
    """BHRT_STREAM_WAVES=0: the later wave steps' parked rays go through k_trace_mesh<false, 1> (one workgroup per 64 key-sorted rays) instead of the
    streamed kernel.  Every sample of the frame; with leaf_skip = 1 as well (the camera step's k_trace_mesh<true, 1, true> and k_shadow_mesh<1, true>
    beside the later steps' walk, which has no leaf-skip form)."""
    st, d_st, sc = _check_switched(gpu, O, monkeypatch, scenes[name], {"BHRT_STREAM_WAVES": 0}, **MESH_OPTS)
    assert sc.info.n_meshes >= 1 and st.closest_rays > st.camera_samples
    _check_switched(gpu, O, monkeypatch, scenes[name], {"BHRT_STREAM_WAVES": 0}, sc=sc, leaf_skip=1, **MESH_OPTS)
    sc.close()


BIG_REGION = (180, 90, 300, 170)
BIG_OPTS = dict(spp=2, gi_bounces=3, seed=3)


def _primary_hits_equal(sc, O):
    blob = sc.flat_bytes()
    o, d = O.primary_rays(sc.flat_view())
    h, r = sc.trace_closest(o, d, 1), O.trace_closest(blob, o, d, 1)
    assert np.array_equal(h["node"], r["node"]) and np.array_equal(h["prim"], r["prim"]) and same_bits(h["t"], r["t"])
    return r


@pytest.mark.parametrize("waves", [0, 2])
def test_mesh_above_2_17_nodes_with_32_bit_path_entries(gpu, O, monkeypatch, scenes, waves):
    """The 320 k-triangle mesh (210 k BVH nodes: 32-bit path entries).  BHRT_STREAM_WAVES=0 -> k_trace_mesh<false, 2>; =2 -> k_trace_mesh_stream<2> with
    two waves that refill thousands of times.  Radiance of a region (the whole 480 x 270 frame is rendered), primary hits of every pixel, and the same
    with leaf_skip = 1: k_trace_mesh<true, 2, true>, k_shadow_mesh<2, true> and (waves = 2) k_trace_mesh_stream<2, true>."""
    st, d_st, sc = _check_switched(gpu, O, monkeypatch, scenes["big_mesh"], {"BHRT_STREAM_WAVES": waves}, region=BIG_REGION, **BIG_OPTS)
    assert sc.info.n_bvh_nodes > PATH16_MAX_NODES and sc.info.max_bvh_depth <= PATH_MAX_DEPTH
    assert st.closest_rays - st.camera_samples > 64 * max(waves, 1) * 20
    r = _primary_hits_equal(sc, O)
    assert (r["prim"] >= 0).sum() > 1000  # the mesh is in view
    assert sc.flat_view().meshes[0].skip_omax > 0  # leaves of this mesh qualify for the skip
    _check_switched(gpu, O, monkeypatch, scenes["big_mesh"], {"BHRT_STREAM_WAVES": waves}, region=BIG_REGION, sc=sc, leaf_skip=1, **BIG_OPTS)
    sc.close()


# ---------------------------------------------------------------------------------------------------- leaf skip x path entries
@pytest.mark.parametrize("name,path", [("c3_mesh_small", 16), ("big_mesh", 32), ("chain", 0)])
def test_leaf_skip_with_16_bit_32_bit_and_no_path_entries(gpu, O, monkeypatch, scenes, name, path):
    """bhrt_opts.leaf_skip = 1 on the default path for the three forms of the walk: 16-bit path entries (k_trace_mesh<true, 1, true>,
    k_trace_mesh_stream<1, true>, k_shadow_mesh<1, true>), 32-bit ones (<.., 2, true>) and the parent-link walk of a tree deeper than 32 levels, where
    the option is ignored (k_trace_mesh<.., 0>, k_shadow_mesh<0>) and the frame must be right all the same.  The same with BHRT_STREAM_WAVES=0 on the two
    small scenes (the big mesh has it in test_mesh_above_2_17_nodes_with_32_bit_path_entries)."""
    region, kw = (BIG_REGION, BIG_OPTS) if name == "big_mesh" else (None, dict(spp=3, gi_bounces=2, seed=4))
    sc = _default_scene(gpu, monkeypatch, scenes[name])
    m = sc.flat_view().meshes[0]
    if path == 16:
        assert m.skip_omax > 0 and sc.info.n_bvh_nodes <= PATH16_MAX_NODES and sc.info.max_bvh_depth <= PATH_MAX_DEPTH
    elif path == 32:
        assert m.skip_omax > 0 and sc.info.n_bvh_nodes > PATH16_MAX_NODES and sc.info.max_bvh_depth <= PATH_MAX_DEPTH
    else:
        assert sc.info.max_bvh_depth > PATH_MAX_DEPTH
    st, d_st, _ = _check_switched(gpu, O, monkeypatch, scenes[name], {}, region=region, sc=sc, leaf_skip=1, **kw)
    assert st.closest_rays > st.camera_samples and st.shadow_rays > 0
    if name != "big_mesh":
        _, _, sw = _check_switched(gpu, O, monkeypatch, scenes[name], {"BHRT_STREAM_WAVES": 0}, leaf_skip=1, **kw)
        sw.close()


# ---------------------------------------------------------------------------------------------------- the two-kernel camera step
@pytest.mark.parametrize("name,jitter,gi", [("c1_sphere_plane", 1, 2), ("c1_sphere_plane", 0, -1), ("c2_glass_small", 1, 3), ("c2_glass_small", 0, 2),
                                            ("c4_textured_no_mesh", 1, 2), ("c4_textured_no_mesh", 0, 2)])
def test_two_kernel_camera_step_of_scenes_without_meshes(gpu, O, monkeypatch, scenes, name, jitter, gi):
    """BHRT_FUSED_CAMERA=0: the camera step of a scene without meshes as k_trace_closest<false, true, false> + k_shade<true, tex> instead of k_shade's
    fused form (kFused), without (c1, c2) and with texture maps (c4_textured without its one mesh node: the two-kernel step only exists where
    n_meshes == 0), with and without jitter, and with gi_bounces = -1.  Every sample of the frame."""
    kw = dict(spp=2, gi_bounces=gi, seed=11, jitter=jitter)
    st, d_st, sc = _check_switched(gpu, O, monkeypatch, scenes[name], {"BHRT_FUSED_CAMERA": 0}, **kw)
    assert sc.info.n_meshes == 0
    assert (sc.flat_view().header.n_texmaps > 0) == (name == "c4_textured_no_mesh")
    assert st.camera_samples == sc.width * sc.height * 2
    sc.close()


# ---------------------------------------------------------------------------------------------------- the slow queue, small frame
def _axis_parallel(d):
    return (d == 0).any(axis=1)


def test_without_the_slow_queue_axis_parallel_rays_stay_in_their_wave_steps(gpu, O, monkeypatch, scenes):
    """BHRT_NO_SLOW_QUEUE=1 on the camera-above-mesh scene: nothing is set aside, the axis-parallel rays walk the BVH in the wave step they belong to.
    "Nothing depends on WHEN a ray is traced" in the other direction."""
    kw = dict(spp=2, gi_bounces=2, seed=6, jitter=0)
    st, d_st, sc = _check_switched(gpu, O, monkeypatch, scenes["above_small"], {"BHRT_NO_SLOW_QUEUE": 1}, **kw)
    o, d = O.primary_rays(sc.flat_view())
    assert _axis_parallel(d).sum() >= 64 + 48 - 1
    assert st.deferred_rays == 0 and d_st.deferred_rays > 0
    sc.close()


def test_shadow_overlap_switch_through_the_environment(gpu, O, monkeypatch, scenes):
    """BHRT_SHADOW_OVERLAP=0 read at upload: the same bits as the knob set to 0 and to 1 on a default scene."""
    xml = scenes["c3_mesh_small"]
    st, d_st, sc = _check_switched(gpu, O, monkeypatch, xml, {"BHRT_SHADOW_OVERLAP": 0}, **MESH_OPTS)
    assert st.shadow_rays > 0
    sc.close()
    kn = _fresh_scene(gpu, monkeypatch, xml, {})
    for v in (0, 1):
        kn.knob("shadow_overlap", v)
        _check_switched(gpu, O, monkeypatch, xml, {}, sc=kn, **MESH_OPTS)
    kn.close()


# ---------------------------------------------------------------------------------------------------- the gather's counting sort
def test_gather_counting_sort_gives_the_radix_sorts_frames(gpu, O, monkeypatch, scenes):
    """BHRT_GATHER_COUNTING_SORT=1 ("A/B and second opinion"): the gather's queries ordered by the counting sort (atomics: the order inside a cell
    varies) instead of the stable radix sort.  c5_caustics with 20,000 photons, the whole frame: radiance bits equal the default sort's with
    photon_exact 0 and 1, and the photon_exact = 1 frame equals the oracle's bits, as test_photon.py checks for the default sort."""
    xml, n_photons = scenes["c5_caustics"], 20000
    dsc = _fresh_scene(gpu, monkeypatch, xml, {})
    csc = _fresh_scene(gpu, monkeypatch, xml, {"BHRT_GATHER_COUNTING_SORT": 1})
    bal, _, _ = O.photon_build(dsc.flat_bytes(), n_photons, seed=3)  # stays attached for O.render(photon=1)
    for sc in (dsc, csc):
        assert sc.photon_build(gpu.default_opts(seed=3), n_photons) == n_photons
        assert np.array_equal(sc.photon_get(), bal)
    W, H = dsc.width, dsc.height
    ro = O.render(dsc.flat_bytes(), W, H, 2, gi=2, seed=3, region=(0, 0, W, H), photon=1, threads=16)["samples"]
    for exact in (0, 1):
        opts = gpu.default_opts(spp=2, gi_bounces=2, seed=3, photon_map=1, photon_exact=exact)
        gd, std = dsc.render_samples(opts, 0, 0, W, H)
        gc, stc = csc.render_samples(opts, 0, 0, W, H)
        assert stc.passes == 1 and stc.photon_queries >= GATHER_SORT_MIN  # the premise: one gather of enough queries to be sorted at all
        assert same_bits(gc, gd)
        assert _counts(stc) == _counts(std) and stc.photon_queries == std.photon_queries and stc.photon_heavy_queries == std.photon_heavy_queries
        if exact:
            assert same_bits(gd, ro) and same_bits(gc, ro)
            assert stc.photon_exact_queries >= stc.photon_heavy_queries
    off, _ = csc.render_samples(gpu.default_opts(spp=2, gi_bounces=2, seed=3), 0, 0, W, H)
    assert not same_bits(off, gc)  # the caustic term is in these frames
    dsc.close()
    csc.close()


# ---------------------------------------------------------------------------------------------------- the slow queue at full size
def _rays_entering_root_box(fv, o, d):
    """Rays (world space) that enter the root box of the scene's one mesh node, by the slab test in float64 with the margin of a few float32 ulp kept
    clear on both sides: a lower bound of what the device's float32 test lets in."""
    node = next(n for n in fv.nodes if n.obj_type == 3)
    mesh = fv.meshes[node.mesh]
    itm = np.array(list(node.xf.itm), np.float64).reshape(3, 3)
    assert np.count_nonzero(itm - np.diag(np.diag(itm))) == 0  # unrotated: a zero component stays one in the mesh's space
    lp = (o.astype(np.float64) - np.array(list(node.xf.pos), np.float64)) * np.diag(itm)
    ld = d.astype(np.float64) * np.diag(itm)
    lo, hi = np.array(list(mesh.bound_min), np.float64), np.array(list(mesh.bound_max), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - lp) / ld, (hi - lp) / ld
    par = ld == 0  # Box::IntersectRay leaves such an axis out
    tn = np.where(par, -np.inf, np.minimum(t0, t1)).max(axis=1)
    tf = np.where(par, np.inf, np.maximum(t0, t1)).min(axis=1)
    return (tn * (1 + 1e-5) < tf * (1 - 1e-5)) & (tf > 0)


def test_slow_queue_at_full_size_cap_ride_along_and_move_in(gpu, O, monkeypatch, scenes, capfd):
    """The camera-above-mesh scene at 1920 x 1080 without jitter (the mesh scaled to reach across the frame's height, so that enough rays of the
    middle column and row enter its root box at an spp that one pass holds): more axis-parallel camera rays than kSlowCap in ONE pass.

    * the cap: the camera step sets aside kSlowCap rays and leaves the rest in their wave step (deferred_rays == kSlowCap);
    * the ride-along branch: the batch set aside by step 0 is moved in behind the rays of step 2 (k_inject_slow at offset n_cur, k_file_all(first = n_cur));
      step 2 holds far more than 2^20 rays — the diagnostic line of BHRT_DEBUG_SLOW says so and is asserted;
    * the same frame, bit for bit and ray for ray, with BHRT_NO_SLOW_QUEUE=1 and with passes too small to reach the cap (everything is set aside there);
    * against the oracle on a 4-pixel strip around the middle column, one around the middle row, and a block away from both.

    The BHRT_DEBUG_SLOW render is cut into two passes (tile_size 16, the second pass = the last 60 tiles: the bottom of the middle column, 8 rows of
    960 pixels): its first pass rides along, its second is too small for that (at most two rays follow from one, so step 2 holds < 4 x 230,400 < 2^20
    rays) and moves its rays in when the queue has run empty.  Both lines are asserted, as is that this frame equals the others."""
    xml = scenes["above_full"]
    dsc = _fresh_scene(gpu, monkeypatch, xml, {})
    W, H = dsc.width, dsc.height
    assert (W, H) == (1920, 1080)
    fv, blob = dsc.flat_view(), dsc.flat_bytes()
    o, d = O.primary_rays(fv)
    slow = (_axis_parallel(d) & _rays_entering_root_box(fv, o, d)).reshape(H, W)
    n_slow_px = int(slow.sum())
    assert slow[:, W // 2].sum() > 900 and slow[H // 2, :].sum() > 900 and n_slow_px == slow[:, W // 2].sum() + slow[H // 2, :].sum() - 1
    spp = K_SLOW_CAP // n_slow_px + 2
    assert n_slow_px * spp > K_SLOW_CAP and W * H * spp < (1 << 26)
    kw = dict(spp=spp, gi_bounces=2, seed=6, jitter=0)

    rgb, rad, st = dsc.render(gpu.default_opts(**kw))
    assert st.passes == 1 and st.camera_samples == W * H * spp
    assert st.deferred_rays == K_SLOW_CAP                       # the cap branch: more were eligible, the host clamps
    assert st.closest_rays - st.camera_samples > 4 * INJECT_MIN_RAYS

    nsc = _fresh_scene(gpu, monkeypatch, xml, {"BHRT_NO_SLOW_QUEUE": 1})
    rgb_n, rad_n, st_n = nsc.render(gpu.default_opts(**kw))
    assert st_n.passes == 1 and st_n.deferred_rays == 0
    assert _counts(st_n) == _counts(st)
    assert same_bits(rad_n, rad), _diff(rad_n, rad)
    assert np.array_equal(rgb_n, rgb)
    nsc.close()

    # passes of 2^20 samples hold T tiles of 32 x 32 pixels (one more when a pass starts inside a tile): at most T tiles' width of the middle row and three
    # tile rows' height of the middle column — fewer axis-parallel camera rays than the cap, so every one of them is set aside
    per_pass = 1 << 20
    tiles_per_pass = -(-per_pass // (spp * 32 * 32)) + 1
    assert (tiles_per_pass * 32 + 3 * 32) * spp < K_SLOW_CAP and tiles_per_pass < W // 32
    rgb_p, rad_p, st_p = dsc.render(gpu.default_opts(samples_per_pass=per_pass, **kw))
    assert st_p.passes > 8 and st_p.deferred_rays >= n_slow_px * spp > K_SLOW_CAP
    assert _counts(st_p) == _counts(st)
    assert same_bits(rad_p, rad), _diff(rad_p, rad)
    assert np.array_equal(rgb_p, rgb)

    # the oracle on the strips (default path) ...
    regions = [(W // 2 - 2, 0, W // 2 + 2, H), (0, H // 2 - 2, W, H // 2 + 2), (300, 200, 364, 232)]
    for reg in regions[:2]:
        gs, st_r = dsc.render_samples(gpu.default_opts(**kw), *reg)
        ro = O.render(blob, W, H, spp, gi=2, seed=6, jitter=0, region=reg, threads=16)
        assert same_bits(gs, ro["samples"]), _diff(gs, ro["samples"])
        assert _counts(st_r) == _counts(st) and st_r.deferred_rays == K_SLOW_CAP
        assert same_bits(rad[reg[1]:reg[3], reg[0]:reg[2]], ro["radiance"])  # the resolved frame of the first render, too
    dsc.close()

    # ... and on the block with BHRT_DEBUG_SLOW=1 in two passes: ride along in the first, move in after the second
    tile = 16
    tiles_x, tiles_y = W // tile, (H + tile - 1) // tile
    last_tiles = tiles_x // 2                                    # tile columns 60..119 of the last tile row: x >= 960, y >= 1072
    assert (W // 2) % tile == 0 and slow[(tiles_y - 1) * tile:, W // 2].sum() == H - (tiles_y - 1) * tile == 8
    first_pass = (tiles_x * tiles_y - last_tiles) * tile * tile * spp
    assert 4 * last_tiles * tile * 8 * spp < INJECT_MIN_RAYS     # step 2 of the second pass cannot reach a ride-along's size
    assert (n_slow_px - 8) * spp > K_SLOW_CAP                    # the first pass alone still exceeds the cap
    bsc = _fresh_scene(gpu, monkeypatch, xml, {"BHRT_DEBUG_SLOW": 1})
    capfd.readouterr()
    reg = regions[2]
    gs, st_b = bsc.render_samples(gpu.default_opts(tile_size=tile, samples_per_pass=first_pass, **kw), *reg)
    err = capfd.readouterr().err
    ro = O.render(blob, W, H, spp, gi=2, seed=6, jitter=0, region=reg, threads=16)
    assert same_bits(gs, ro["samples"]) and same_bits(rad[reg[1]:reg[3], reg[0]:reg[2]], ro["radiance"])
    assert st_b.passes == 2 and _counts(st_b) == _counts(st)
    assert st_b.deferred_rays >= K_SLOW_CAP + 8 * spp            # the first pass at its cap, every slow ray of the second
    rides = [ln for ln in err.splitlines() if "ride along with wave step" in ln]
    moves = [ln for ln in err.splitlines() if "moved in after wave step" in ln]
    assert rides and moves, err[-2000:]
    m = re.search(r"slow rays: (\d+) ride along with wave step (\d+) \((\d+) rays\)", rides[0])
    assert m and int(m.group(1)) == K_SLOW_CAP and int(m.group(2)) >= 1 and int(m.group(3)) >= INJECT_MIN_RAYS
    bsc.close()
