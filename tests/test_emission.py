"""Emissive materials: with bhrt_scene_set_emissive on, every Shade() frame of a Blinn material evaluates to
Shade(hit) + emission.Sample(uvw, duvw), one float addition per channel, last.

The oracle knows nothing of emission and still pins the term bit for bit, two ways:
  1. white body  a black-bodied emitter with Le = (1, 1, 1) has the Shade() value of an empty MultiMtl (constant white, materials.h:71): the oracle
                 renders the flat blob with the emitter's material kind patched to BHRT_MTL_WHITE, the GPU the unpatched scene with the term on;
  2. one add     without child frames (gi_bounces = -1, internal_bounces = 0) a sample is the oracle's sample + Le of the material of its first hit.
tests/scenes/emission_room.xml: a closed room without any light, the emitter "lamp" a fifth of the frame.  33 x 17 pixels, spp 3."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, SCENES, ensure_mesh, same_bits

XML = os.path.join(SCENES, "emission_room.xml")
W, H, SPP = 33, 17, 3
MTL_WHITE = 1  # include/bhrt_flat.h: BHRT_MTL_WHITE
ERR_ARG = "bhrt error 3"  # BHRT_ERR_ARG
COMBOS = [(gi, ib, seed) for gi in (-1, 0, 3) for ib in (0, 16) for seed in (0, 9)]


# ---------------------------------------------------------------------------------------------------- scenes
def _text():
    return open(XML).read()


def _sub(txt, old, new):
    assert txt.count(old) == 1, old
    return txt.replace(old, new)


LIGHT = '    <light type="point" name="pointLight">\n      <intensity value="60"/>\n      <position x="0" y="-10" z="20"/>\n      <size value="1"/>\n    </light>\n  </scene>'


def _variant_plain():
    """Test 2: coloured emitters and one light, so that Shade_ref != 0."""
    t = _sub(_text(), '<emission r="1" g="1" b="1"/>', '<emission r="0.25" g="0.5" b="2.0"/>')
    t = _sub(t, '<diffuse r="0.8" g="0.3" b="0.3"/>', '<diffuse r="0.6" g="0.5" b="0.4"/>\n      <emission r="0.125" g="0" b="0.0625"/>')
    return _sub(t, "  </scene>", LIGHT)


def _variant_textured():
    """Test 2: the lamp's emission through a checkerboard, the ball's through the image file."""
    t = _sub(_text(), '<emission r="1" g="1" b="1"/>',
             '<emission r="1" g="0.5" b="2" texture="checkerboard">\n        <color1 r="0.25" g="1" b="0.5"/>\n        <color2 r="1" g="0.125" b="0.75"/>\n'
             '        <scale x="0.3" y="0.2"/>\n      </emission>')
    t = _sub(t, '<diffuse r="0.8" g="0.3" b="0.3"/>', '<diffuse r="0.6" g="0.5" b="0.4"/>\n      <emission r="0.5" g="1" b="0.75" texture="tex_small.png"/>')
    return _sub(t, "  </scene>", LIGHT)


def _variant_no_emission_element():
    return _sub(_text(), '      <emission r="1" g="1" b="1"/>\n', "")


def _variant_no_mesh():
    """The same room without the mesh: the camera step is k_shade's fused form (it traces its camera rays itself)."""
    t, n = re.subn(r'    <object type="obj" name="mesh_small.obj".*?</object>\n', "", _text(), flags=re.S)
    assert n == 1
    return t


@pytest.fixture(scope="module")
def make_scene(B, tmp_path_factory):
    """Private scene handles (the switch is state of a handle), freed when the module is done.  make_scene() = the committed scene,
    make_scene(text, tag) = a variant of it written beside copies of its assets."""
    d = tmp_path_factory.mktemp("emission")
    for asset in ("mesh_small.obj", "tex_small.png"):
        shutil.copy(os.path.join(SCENES, asset), d / asset)
    opened = []

    def _make(text=None, tag=None):
        path = XML
        if text is not None:
            path = str(d / f"{tag}.xml")
            with open(path, "w") as fp:
                fp.write(text)
        opened.append(B.Scene(path))
        return opened[-1]
    yield _make
    for sc in opened:
        sc.close()


@pytest.fixture(scope="module")
def gpu(B):
    if B.device_count() < 1:
        pytest.fail("no HIP device: the render path has no CPU fallback, GPU tests cannot run here")
    return B


@pytest.fixture(scope="module")
def room(gpu, make_scene):
    """emission_room.xml, uploaded, the term on."""
    sc = make_scene()
    sc.upload(0)
    sc.set_emissive(True)
    return sc


def _material_offset(fv, mi):
    from bhraytracer_amd import flat
    return fv.header.off_materials + mi * C.sizeof(flat.Material)


def _white_blob(sc, name="lamp"):
    """The scene's flat blob with the kind of material `name` set to BHRT_MTL_WHITE."""
    off = _material_offset(sc.flat_view(), sc.material_index(name))
    b = bytearray(sc.flat_bytes())
    b[off:off + 4] = np.int32(MTL_WHITE).tobytes()
    return bytes(b)


_expected = {}


def _white_expected(O, sc, gi, ib, seed):
    """The oracle's render of the white-patched blob, once per parameter set (shared by the tests, never written to)."""
    key = (gi, ib, seed)
    if key not in _expected:
        r = O.render(_white_blob(sc), W, H, SPP, gi=gi, bounces=ib, seed=seed, threads=16)
        for a in (r["samples"], r["radiance"], r["rgb8"]):
            a.setflags(write=False)
        _expected[key] = r
    return _expected[key]


def _first_hit_material(gpu, O, sc, opts):
    """Material index of the first hit of every camera sample (-1: a miss or a node without material), (pixels, spp)."""
    o, d = sc.camera_rays(opts)
    h = O.trace_closest(sc.flat_bytes(), o.reshape(-1, 3), d.reshape(-1, 3), gpu.SIDE_FRONT)
    node_mtl = np.array([n.material for n in sc.flat_view().nodes] + [-1], np.int32)  # [-1]: a miss
    return node_mtl[h["node"]].reshape(o.shape[0], o.shape[1])


def _diff(a, b):
    bad = np.argwhere(np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32))
    return f"{len(bad)} of {a.size} values differ, first at {bad[:6].tolist()}"


# ---------------------------------------------------------------------------------------------------- 1. white-body equivalence
@pytest.mark.gpu
@pytest.mark.parametrize("gi,ib,seed", COMBOS)
def test_white_body_equivalence(gpu, O, room, gi, ib, seed):
    opts = gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed)
    exp = _white_expected(O, room, gi, ib, seed)["samples"]
    # the comparison is not an empty one: the oracle ignores emission (exactly 0 where the camera ray hits the lamp first), the lamp is in view,
    # and light arrives
    lamp_first = _first_hit_material(gpu, O, room, opts) == room.material_index("lamp")
    plain = O.render(room.flat_bytes(), W, H, SPP, gi=gi, bounces=ib, seed=seed, threads=16)["samples"]
    assert np.all(plain[lamp_first].view(np.uint32) == 0)
    assert lamp_first.mean() >= 0.05, lamp_first.mean()
    assert (exp != 0).any(axis=2).mean() >= 0.20, (exp != 0).any(axis=2).mean()
    gs, st = room.render_samples(opts, 0, 0, W, H)
    assert st.camera_samples == W * H * SPP
    assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("gi,ib,seed", [(3, 16, 0), (0, 0, 9)])
def test_white_body_resolved_frame_both_ways(gpu, O, room, fused, gi, ib, seed):
    """radiance and rgb8 of a plain render: the root frames resolved straight into the image (k_resolve_frames) and through the sample buffer."""
    exp = _white_expected(O, room, gi, ib, seed)
    try:
        room.knob("fused_resolve", fused)
        rgb, rad, st = room.render(gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed))
    finally:
        room.knob("fused_resolve", 1)
    assert st.launches_resolve_fused == (st.passes if fused else 0)
    assert same_bits(rad, exp["radiance"]), _diff(rad, exp["radiance"])
    assert np.array_equal(rgb, exp["rgb8"])


@pytest.mark.gpu
def test_white_body_over_frame_batches_and_passes(gpu, O, room):
    gi, ib, seed = 3, 16, 9
    exp = _white_expected(O, room, gi, ib, seed)["samples"]
    opts = gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed)
    _, st = room.render_samples(opts, 0, 0, W, H)
    assert st.passes == 1
    try:  # a frame pool of a third of what the frame needs: passes overflow and are redone in halves
        room.knob("frame_cap", max(1, int(st.shade_calls) // 3))
        gs, st2 = room.render_samples(opts, 0, 0, W, H)
    finally:
        room.knob("frame_cap", 0)
    assert st2.passes >= 3
    assert same_bits(gs, exp), _diff(gs, exp)
    gs, st3 = room.render_samples(gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed, samples_per_pass=W * H * SPP // 2), 0, 0, W, H)
    assert st3.passes >= 2
    assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
def test_white_body_as_rank_1_of_2(gpu, O, room):
    from bhraytracer_amd import dist
    gi, ib, seed, tile = 3, 16, 0, 8
    exp = _white_expected(O, room, gi, ib, seed)["samples"]
    own = dist.owned_mask(W, H, tile, 1, 2).numpy().reshape(-1)
    assert 0 < own.sum() < W * H
    gs, _ = room.render_samples(gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed, rank=1, world_size=2, tile_size=tile), 0, 0, W, H)
    assert same_bits(gs[own], exp[own]), _diff(gs[own], exp[own])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
def test_white_body_without_meshes_fused_camera_step(gpu, O, make_scene, seed):
    sc = make_scene(_variant_no_mesh(), "no_mesh")
    assert sc.info.n_meshes == 0
    sc.set_emissive(True)  # before the upload: the upload carries the switch
    sc.upload(0)
    exp = O.render(_white_blob(sc), W, H, SPP, gi=3, bounces=16, seed=seed, threads=16)
    assert (exp["samples"] != 0).any(axis=2).mean() >= 0.20
    opts = gpu.default_opts(spp=SPP, gi_bounces=3, internal_bounces=16, seed=seed)
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(gs, exp["samples"]), _diff(gs, exp["samples"])
    rgb, rad, _ = sc.render(opts)
    assert same_bits(rad, exp["radiance"]) and np.array_equal(rgb, exp["rgb8"])


# ---------------------------------------------------------------------------------------------------- 2. one-add exactness
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
def test_one_add_plain_colours(gpu, O, make_scene, seed):
    sc = make_scene(_variant_plain(), f"plain_{seed}")
    sc.upload(0)
    sc.set_emissive(True)
    opts = gpu.default_opts(spp=SPP, gi_bounces=-1, internal_bounces=0, seed=seed)
    le = np.array([sc.material_emission(m)[0] for m in range(sc.info.n_materials)] + [(0, 0, 0)], np.float32)  # [-1]: no material, no emission
    assert le[sc.material_index("lamp")].tolist() == [0.25, 0.5, 2.0] and le[sc.material_index("ball")].tolist() == [0.125, 0, 0.0625]
    mtl = _first_hit_material(gpu, O, sc, opts)
    assert (mtl == sc.material_index("lamp")).mean() >= 0.05 and (mtl == sc.material_index("ball")).sum() > 0
    base = O.render(sc.flat_bytes(), W, H, SPP, gi=-1, bounces=0, seed=seed, threads=16)["samples"]
    assert (base != 0).any(axis=2).mean() >= 0.20  # the light: Shade_ref != 0
    exp = base + le[mtl]  # float32 + float32: the one addition
    assert exp.dtype == np.float32
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
def test_one_add_textured_emission(gpu, O, make_scene):
    from bhraytracer_amd import flat
    sc = make_scene(_variant_textured(), "textured")
    sc.upload(0)
    sc.set_emissive(True)
    fv = sc.flat_view()
    lamp, ball = sc.material_index("lamp"), sc.material_index("ball")
    assert fv.textures[fv.texmaps[sc.material_emission(lamp)[1]].texture].type == 0  # BHRT_TEX_CHECKER
    assert fv.textures[fv.texmaps[sc.material_emission(ball)[1]].texture].width > 0                        # the image file
    opts = gpu.default_opts(spp=1, gi_bounces=-1, internal_bounces=0, seed=0, jitter=0)
    # expected Le per pixel: the oracle's albedo image (diffuse.Sample(uvw, duvw) of the first hit) of a blob whose diffuse TexturedColor is the emission one
    b = bytearray(sc.flat_bytes())
    for m in range(sc.info.n_materials):
        (r, g, bl), tm = sc.material_emission(m)
        off = _material_offset(fv, m) + flat.Material.diffuse.offset
        b[off:off + 16] = bytes(flat.TexColor((r, g, bl), tm))
    _, _, le = O.first_hit(bytes(b), W, H)
    o, d = sc.camera_rays(opts)
    po, pd = O.primary_rays(fv)
    agree = np.all(o.reshape(-1, 3).view(np.uint32) == po.view(np.uint32), axis=1) & np.all(d.reshape(-1, 3).view(np.uint32) == pd.view(np.uint32), axis=1)
    assert agree.all(), f"camera_rays with jitter 0 differ from oracle_lib.primary_rays at {int((~agree).sum())} pixels"
    base = O.render(sc.flat_bytes(), W, H, 1, gi=-1, bounces=0, seed=0, jitter=0, threads=16)["samples"]
    exp = base[:, 0, :] + le
    mtl = _first_hit_material(gpu, O, sc, opts)[:, 0]
    assert len(np.unique(le[mtl == lamp], axis=0)) >= 2 and len(np.unique(le[mtl == ball], axis=0)) >= 2  # the textures vary over the emitters
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(gs[:, 0, :], exp), _diff(gs[:, 0, :], exp)
    rgb, rad, _ = sc.render(opts)  # the resolved frame: spp 1, so the pixel is the sample
    assert same_bits(rad.reshape(-1, 3), exp), _diff(rad.reshape(-1, 3), exp)


# ---------------------------------------------------------------------------------------------------- 3. off is off
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
def test_off_is_the_oracle_frame(gpu, O, make_scene, seed):
    """The switch at its default: the <emission> of the XML does nothing, as in the reference.  The room (black: it has no light) and the
    variant with a light."""
    for text, tag in ((None, None), (_variant_plain(), f"off_{seed}")):
        sc = make_scene(text, tag)
        sc.upload(0)
        gs, _ = sc.render_samples(gpu.default_opts(spp=SPP, gi_bounces=3, internal_bounces=16, seed=seed), 0, 0, W, H)
        exp = O.render(sc.flat_bytes(), W, H, SPP, gi=3, bounces=16, seed=seed, threads=16)["samples"]
        assert same_bits(gs, exp), _diff(gs, exp)
        assert (exp != 0).any() == (text is not None)
        sc.set_emissive(True)
        sc.set_emissive(False)  # on and off again: off
        gs, _ = sc.render_samples(gpu.default_opts(spp=SPP, gi_bounces=3, internal_bounces=16, seed=seed), 0, 0, W, H)
        assert same_bits(gs, exp), _diff(gs, exp)


def test_default_opts_unchanged_and_64_bytes(B):
    assert C.sizeof(B.Opts) == 64
    o = B.default_opts()
    got = {n: getattr(o, n) for n, _ in B.Opts._fields_}
    assert got == dict(spp=32, gi_bounces=3, internal_bounces=16, seed=0, jitter=1, gamma=1, photon_map=0, rank=0, world_size=1, tile_size=32,
                       samples_per_pass=0, timers=0, photon_exact=0, leaf_skip=0, photon_radius=0.0, lens=0)
    canary = (C.c_uint8 * 128)(*([0xA5] * 128))  # bhrt_default_opts writes 64 bytes, no more
    B.lib().bhrt_default_opts(C.byref(canary))
    assert bytes(canary)[:64] == bytes(o) and set(bytes(canary)[64:]) == {0xA5}


def _scene_xmls():
    return sorted(f for f in os.listdir(SCENES) if f.endswith(".xml"))


@pytest.mark.parametrize("name", _scene_xmls())
def test_flat_blob_keeps_its_bytes(B, name):
    """The emission state lives beside the blob: switching it on, or setting a material's emission, changes no byte of it."""
    path = os.path.join(SCENES, name)
    if "gen/mesh_224.obj" in open(path).read():
        ensure_mesh(224)
    sc = B.Scene(path)
    try:
        before = sc.flat_bytes()
        sc.set_emissive(True)
        sc._flat = None
        assert sc.flat_bytes() == before
        if sc.info.n_materials:
            sc.set_material_emission(0, (1, 2, 3))
            sc._flat = None
            assert sc.flat_bytes() == before
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------- 4. riding along
@pytest.mark.gpu
def test_adaptive_pixels_equal_uniform_renders_at_their_count(gpu, room):
    opts = gpu.default_opts(spp=8, gi_bounces=3, seed=9)
    rgb, rad, var, cnt, st = room.render_adaptive(opts, gpu.default_adaptive_opts(min_spp=2, threshold=0.05))
    assert st.camera_samples == int(cnt.sum()) and set(np.unique(cnt).tolist()) <= {2, 4, 8} and len(np.unique(cnt)) >= 2
    assert (rad != 0).any(axis=2).mean() >= 0.20  # the emission term is in the frame
    for n in np.unique(cnt).tolist():
        urgb, urad, uvar = room.render_var(gpu.default_opts(spp=int(n), gi_bounces=3, seed=9))
        m = cnt == n
        assert same_bits(rad[m], urad[m]) and np.array_equal(rgb[m], urgb[m]), n
        # the variance is a Welford recurrence there and two passes here: tests/test_adaptive.py's tolerance for the same property
        assert np.all(np.abs(var[m] - uvar[m]) <= 1e-4 * np.abs(uvar[m]) + 1e-12), n


@pytest.mark.gpu
def test_render_var_radiance_is_renders(gpu, O, room):
    opts = gpu.default_opts(spp=SPP, gi_bounces=3, seed=0)
    rgb, rad, _ = room.render(opts)
    vrgb, vrad, var = room.render_var(opts)
    assert same_bits(rad, vrad) and np.array_equal(rgb, vrgb) and (var > 0).any()
    assert same_bits(rad, _white_expected(O, room, 3, 16, 0)["radiance"])


@pytest.mark.gpu
def test_lens_with_emission_from_the_setter(gpu, B):
    sc = B.Scene(os.path.join(SCENES, "lens_spheres.xml"))  # no mesh, <dof> 1.5
    try:
        sc.upload(0)
        opts = gpu.default_opts(spp=SPP, gi_bounces=2, seed=3, lens=1)
        _, off, _ = sc.render(opts)
        sc.set_material_emission(sc.material_index("ball"), (0.5, 0.25, 0.125))  # refreshes the uploaded scene
        _, still_off, _ = sc.render(opts)
        assert same_bits(off, still_off)  # the switch is off
        sc.set_emissive(True)
        _, on, _ = sc.render(opts)
        assert np.isfinite(on).all() and not same_bits(on, off)  # (not monotone: a brighter child can take a parent through an early return of Shade())
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------- 5. API
@pytest.mark.gpu
def test_setter_renders_like_the_xml(gpu, room, make_scene):
    opts = gpu.default_opts(spp=SPP, gi_bounces=3, seed=9)
    ref, _ = room.render_samples(opts, 0, 0, W, H)
    sc = make_scene(_variant_no_emission_element(), "no_element")
    lamp = sc.material_index("lamp")
    assert sc.material_emission(lamp) == ((0.0, 0.0, 0.0), -1)
    sc.upload(0)
    sc.set_emissive(True)
    dark, _ = sc.render_samples(opts, 0, 0, W, H)
    assert not dark.any()  # no light and no emitter
    sc.set_material_emission(lamp, (1, 1, 1))  # on the uploaded scene
    assert sc.material_emission(lamp) == ((1.0, 1.0, 1.0), -1)
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(gs, ref), _diff(gs, ref)


@pytest.mark.gpu
def test_clone_carries_switch_and_emission(gpu, room, make_scene):
    opts = gpu.default_opts(spp=SPP, gi_bounces=3, seed=0)
    src = make_scene()
    src.set_emissive(True)
    src.set_material_emission(src.material_index("ball"), (0.5, 0.25, 2.0))
    cl = src.clone()
    try:
        assert cl.material_emission(cl.material_index("ball")) == ((0.5, 0.25, 2.0), -1) and cl.flat_bytes() == src.flat_bytes()
        a, _ = src.render_samples(opts, 0, 0, W, H)
        b, _ = cl.render_samples(opts, 0, 0, W, H)
        base, _ = room.render_samples(opts, 0, 0, W, H)
        assert same_bits(a, b) and not same_bits(a, base)
    finally:
        cl.close()


def test_api_errors_and_getters(B):
    sc = B.Scene(XML)
    try:
        assert sc.info.n_materials == 7
        for i, name in enumerate(["wall", "wallRed", "wallBlue", "lamp", "ball", "glass", "meshmtl"]):
            assert sc.material_index(name) == i
        with pytest.raises(B.BhrtError, match=ERR_ARG):
            sc.material_index("no such material")
        for bad in (-1, 7, 1 << 20):
            with pytest.raises(B.BhrtError, match=ERR_ARG):
                sc.set_material_emission(bad, (1, 1, 1))
            with pytest.raises(B.BhrtError, match=ERR_ARG):
                sc.material_emission(bad)
        sc.set_material_emission(2, (0.5, 0.25, 4.0))
        assert sc.material_emission(2) == ((0.5, 0.25, 4.0), -1)
        assert B.lib().bhrt_scene_get_material_emission(sc._h, 2, None, None) == 0  # either output may be NULL
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------- 7. the loader (no GPU)
def test_loader_keeps_colour_and_map(B, tmp_path):
    sc = B.Scene(XML)
    try:
        lamp = sc.material_index("lamp")
        for m in range(sc.info.n_materials):
            assert sc.material_emission(m) == (((1.0, 1.0, 1.0) if m == lamp else (0.0, 0.0, 0.0)), -1)
    finally:
        sc.close()
    for asset in ("mesh_small.obj", "tex_small.png"):
        shutil.copy(os.path.join(SCENES, asset), tmp_path / asset)
    (tmp_path / "t.xml").write_text(_variant_textured())
    sc = B.Scene(str(tmp_path / "t.xml"))
    try:
        assert sc.warnings() == []
        fv = sc.flat_view()
        assert fv.header.n_texmaps == 2  # the two <emission> maps: pushed to texmaps[] as before, only now their index is kept
        rgb, tm = sc.material_emission(sc.material_index("lamp"))
        assert rgb == (1.0, 0.5, 2.0) and tm == 0
        tex = fv.textures[fv.texmaps[tm].texture]
        assert tex.type == 0 and list(tex.color1) == [0.25, 1.0, 0.5] and list(tex.color2) == [1.0, 0.125, 0.75]
        rgb, tm = sc.material_emission(sc.material_index("ball"))
        assert rgb == (0.5, 1.0, 0.75) and tm == 1
        tex = fv.textures[fv.texmaps[tm].texture]
        assert tex.type == 1 and tex.width > 0 and tex.height > 0
        sc.set_material_emission(sc.material_index("lamp"), (3, 2, 1))  # a plain colour drops the map
        assert sc.material_emission(sc.material_index("lamp")) == ((3.0, 2.0, 1.0), -1)
    finally:
        sc.close()


def test_shipped_proj12_reports_its_emission(B):
    cwd = os.getcwd()
    os.chdir(os.path.join(GOLDEN, "shipped"))  # the reference resolves asset paths against its working directory
    try:
        sc = B.Scene(os.path.join("Resource", "Data", "proj12.xml"))
    finally:
        os.chdir(cwd)
    try:
        assert sc.material_emission(sc.material_index("light")) == ((20.0, 20.0, 20.0), -1)  # <emission value="20"/>
        assert sc.material_emission(sc.material_index("wallBlue")) == ((0.0, 0.0, 0.0), -1)
    finally:
        sc.close()
