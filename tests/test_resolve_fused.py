"""The end of a pass, both ways (DESIGN.md 4 "Resolve from the frames"): a render that asks for the image alone resolves its root frames straight
into it (k_resolve_frames, knob "fused_resolve" = 1, the default); every other render, and knob 0, folds them into the per-sample buffer
(k_combine's root level) and sums that (k_resolve).  The two owe each other the same bits: the same frame arithmetic per sample, the same
additions from zero in sample order, the same division, the same Color24.

Every case renders with the knob at 1 and at 0 on one scene handle and compares rgb8 and radiance bit for bit; the first two also against the
oracle's keyed-mode render.  Every render asserts which path it took (bhrt_stats.launches_resolve_fused: one per pass, or none), so a case that
silently takes the other path fails instead of passing."""
import os
import re
import shutil

import numpy as np
import pytest

from conftest import SCENES, same_bits

pytestmark = pytest.mark.gpu


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
def scene(gpu, tmp_path_factory):
    """Private scene handles (the knob is state of a handle: none of conftest's shared ones), freed when the module is done.  name -> the committed
    scene; (name, w, h) -> the same scene text with another frame size."""
    d = tmp_path_factory.mktemp("resolve_fused")
    for asset in ("mesh_small.obj", "tex_small.png", "tex_small.ppm"):
        shutil.copy(os.path.join(SCENES, asset), d / asset)
    made = {}

    def _get(name, w=None, h=None):
        key = (name, w, h)
        if key not in made:
            path = os.path.join(SCENES, name + ".xml")
            if w is not None:
                path = str(d / f"{name}_{w}x{h}.xml")
                with open(path, "w") as fp:
                    fp.write(_resized(name, w, h))
            made[key] = gpu.Scene(path)
            made[key].upload(0)
        return made[key]
    yield _get
    for sc in made.values():
        sc.close()


def _both(sc, opts, render=None):
    """`render(sc, opts)` (default: sc.render) with the knob at 1 and at 0 -> (result fused, result through the sample buffer)."""
    render = render or (lambda s, o: s.render(o))
    try:
        sc.knob("fused_resolve", 1)
        a = render(sc, opts)
        sc.knob("fused_resolve", 0)
        b = render(sc, opts)
    finally:
        sc.knob("fused_resolve", 1)
    return a, b


def _check_ab(sc, opts):
    """The A/B of a plain render: same bytes, same floats, same ray counts, and each took the path it was asked to take."""
    (rgb, rad, st), (rgb0, rad0, st0) = _both(sc, opts)
    assert st.passes >= 1 and st.launches_resolve_fused == st.passes, (st.passes, st.launches_resolve_fused)
    assert st0.launches_resolve_fused == 0
    bad = np.argwhere(rad.view(np.uint32) != rad0.view(np.uint32))
    assert same_bits(rad, rad0), f"radiance: {len(bad)} of {rad.size} values differ, first at {bad[:8].tolist()}"
    assert np.array_equal(rgb, rgb0)
    assert (st.camera_samples, st.closest_rays, st.shadow_rays, st.shade_calls) == (st0.camera_samples, st0.closest_rays, st0.shadow_rays, st0.shade_calls)
    return rgb, rad, st


def _primary_nodes(gpu, O, sc):
    o, d = O.primary_rays(sc.flat_view())
    h = sc.trace_closest(o, d, gpu.SIDE_FRONT)
    return h["node"], h["prim"]


def _check_oracle(O, sc, rgb, rad, spp, gi, seed):
    ro = O.render(sc.flat_bytes(), sc.width, sc.height, spp, gi=gi, seed=seed, threads=16, want_samples=False)
    assert same_bits(rad, ro["radiance"]) and np.array_equal(rgb, ro["rgb8"])


# lanes over samples: fewer than a wave, one lane short of it, exactly one wave, one over, more than two chunks
@pytest.mark.parametrize("spp", [1, 3, 63, 64, 65, 130])
def test_mesh_scene_with_camera_misses(gpu, O, scene, spp):
    """The mesh scene of the lens tests through the pinhole camera: the camera step parks rays into the mesh walk, k_shade<true, tex> fills the
    map from the shading order, and the rays that leave over the horizon take the background value in k_resolve_frames."""
    sc = scene("lens_mesh_small")
    node, prim = _primary_nodes(gpu, O, sc)
    assert (node < 0).sum() > 100 and (prim >= 0).sum() > 100 and sc.info.n_meshes > 0  # camera misses, and a mesh in view
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=spp, gi_bounces=2, seed=5))
    assert st.camera_samples == sc.width * sc.height * spp
    _check_oracle(O, sc, rgb, rad, spp, 2, 5)


@pytest.mark.parametrize("spp", [3, 65])
def test_scene_without_meshes(gpu, O, scene, spp):
    """No mesh: the camera step is k_shade's fused form (it traces its camera rays itself, frame numbers from one atomic per workgroup), which
    fills the map and the sentinel as well."""
    sc = scene("lens_spheres")
    node, _ = _primary_nodes(gpu, O, sc)
    assert sc.info.n_meshes == 0 and (node < 0).sum() > 100 and (node >= 0).sum() > 100
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=spp, gi_bounces=3, seed=8))
    _check_oracle(O, sc, rgb, rad, spp, 3, 8)


@pytest.mark.parametrize("name,w,h", [("c1_sphere_plane", 75, 50), ("c3_mesh_small", 77, 45)])
def test_edge_tiles_as_rank_1_of_3(gpu, scene, name, w, h):
    """Neither side a multiple of the 32-pixel tile, rendered as rank 1 of 3: the rank's tiles on the right and bottom edge stick out of the image,
    their slots are dead — k_shade writes no map entry for them and k_resolve_frames must not read one.  Pixels of other ranks stay untouched."""
    sc = scene(name, w, h)
    spp = 5
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=spp, gi_bounces=2, seed=3, rank=1, world_size=3, tile_size=32))
    tiles_x, tiles_y = (w + 31) // 32, (h + 31) // 32
    mine = np.zeros((h, w), bool)
    n_slots = 0
    for t in range(1, tiles_x * tiles_y, 3):
        ty, tx = divmod(t, tiles_x)
        mine[ty * 32:(ty + 1) * 32, tx * 32:(tx + 1) * 32] = True
        n_slots += 32 * 32
    assert 0 < st.camera_samples == int(mine.sum()) * spp < n_slots * spp  # the premise: dead slots
    assert not rad[~mine].any() and not rgb[~mine].any()


def test_three_passes(gpu, scene):
    sc = scene("lens_mesh_small")
    kw = dict(spp=4, gi_bounces=2, seed=6)
    one = _check_ab(sc, gpu.default_opts(**kw))
    assert one[2].passes == 1
    rgb, rad, st = _check_ab(sc, gpu.default_opts(samples_per_pass=sc.width * sc.height * 4 // 3 - 1000, **kw))
    assert st.passes >= 3
    assert np.array_equal(rgb, one[0]) and same_bits(rad, one[1])


def test_pass_that_overflows_and_is_redone_in_halves(gpu, scene):
    """The frame pool at a third of what the frame needs: the pass overflows part-way, with the map half filled, and is redone in halves.  (The fused
    render goes first and meets the overflow; the scene remembers the pass size that fitted, so the render behind it may start from there.)"""
    sc = scene("c3_mesh_small", 96, 72)
    opts = gpu.default_opts(spp=4, gi_bounces=3, seed=9)
    base = _check_ab(sc, opts)
    assert base[2].passes == 1
    sc.knob("frame_cap", max(1, int(base[2].shade_calls) // 3))
    try:
        rgb, rad, st = _check_ab(sc, opts)
    finally:
        sc.knob("frame_cap", 0)
    assert st.passes >= 3
    assert np.array_equal(rgb, base[0]) and same_bits(rad, base[1])


@pytest.mark.parametrize("name", ["lens_spheres", "lens_mesh_small"])
def test_thin_lens(gpu, scene, name):
    """lens = 1: k_lens_rays writes the camera rays into the queue and the queue kernels shade them (k_shade<false, tex> on RK_CAMERA rays)."""
    sc = scene(name)
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=3, gi_bounces=2, seed=4, lens=1))
    pin = sc.render(gpu.default_opts(spp=3, gi_bounces=2, seed=4))
    assert not same_bits(rad, pin[1])  # the aperture is open


def test_textured_background(gpu, O, scene):
    """c4_textured's background is a texture: a sentinel lane samples it at (i / W, j / H, 0), as k_shade does on the other path."""
    sc = scene("c4_textured", 144, 108)
    fv = sc.flat_view()
    node, _ = _primary_nodes(gpu, O, sc)
    assert fv.header.n_texmaps > 0 and (node < 0).sum() > 100
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=3, gi_bounces=2, seed=2))
    miss = (node < 0).reshape(sc.height, sc.width)
    assert len(np.unique(rad[miss].view(np.uint32), axis=0)) > 8  # many background values: a texture, not one colour


def test_photon_map(gpu, scene):
    sc = scene("c5_caustics", 96, 72)
    assert sc.photon_build(gpu.default_opts(seed=3), 2000) > 0
    rgb, rad, st = _check_ab(sc, gpu.default_opts(spp=3, gi_bounces=2, seed=3, photon_map=1))
    off = sc.render(gpu.default_opts(spp=3, gi_bounces=2, seed=3))
    assert not same_bits(rad, off[1])  # the caustic term is in


def test_other_consumers_keep_the_sample_buffer(gpu, scene):
    """Region samples and the variance image read the per-sample buffer: whatever the knob says, the fused kernel is not used there, and they return
    what they returned before."""
    sc = scene("lens_mesh_small")
    opts = gpu.default_opts(spp=5, gi_bounces=2, seed=7)
    region = (10, 8, 90, 66)
    (gs, st), (gs0, st0) = _both(sc, opts, lambda s, o: s.render_samples(o, *region))
    assert st.launches_resolve_fused == 0 and st0.launches_resolve_fused == 0
    assert gs.shape == (80 * 58, 5, 3) and same_bits(gs, gs0)
    v, v0 = _both(sc, opts, lambda s, o: s.render_var(o))
    assert np.array_equal(v[0], v0[0]) and same_bits(v[1], v0[1]) and same_bits(v[2], v0[2]) and v[2].any()
    rgb, rad, _ = _check_ab(sc, opts)  # and the plain render of the same frame agrees with both
    assert np.array_equal(rgb, v[0]) and same_bits(rad, v[1])
    x0, y0, x1, y1 = region
    mean = np.zeros((gs.shape[0], 3), np.float32)
    for s in range(5):
        mean = mean + gs[:, s, :]
    assert same_bits((mean / np.float32(5)).reshape(y1 - y0, x1 - x0, 3), rad[y0:y1, x0:x1])
