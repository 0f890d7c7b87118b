"""The global gather: where gi < 0 cuts the GI term (MtlBlinn.cpp:386) a Shade() frame takes
    G = -vL . vN > 0 ? clamp(Color::Black() + diffuse.Sample(uvw, duvw) * E) : black,   (E, vL) = EstimateIrradiance<1000>(radius, p, &N)
from the global photon map (bhrt_scene_set_global_gather, bhrt_global_map_build / _set / _get, bhrt_global_gather_host).

Every scene handle here is this module's own: the switch is state of a handle, and the session's load_scene handles are shared with other files.
Regions are 32 x 32 pixels at 2 spp, maps 20 000 photons (the caustic map of section 3: 5 000).  The oracle builds the maps of sections 1-3 on the
CPU; the test_inputs_* cases (no GPU) hold the conditions on the chosen regions, map sizes and radii with the oracle alone.

  C5   c5_caustics.xml, region (40, 200)-(72, 232): floor, red wall and the lower part of the glass sphere; radius 0.25
  C4   c4_textured.xml, region (128, 92)-(160, 124), jitter 0 (every sample of a pixel is the ray through its corner, so diffuse.Sample is the
       albedo image of O.first_hit, the route of test_face_materials.py); radius 0.15
  H    c5_caustics.xml with the point light at intensity 0.5 / 0.03125 (maps) and without any light (renders); radius 1"""
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits
from test_lens import lens_rays_ref

f32 = np.float32
ERR_ARG = "bhrt error 3"  # BHRT_ERR_ARG
SPP, N_MAP, N_CAUSTIC, MAP_SEED = 2, 20000, 5000, 0
CASES = {  # name -> (scene, region, jitter, radius)
    "C5": ("c5_caustics", (40, 200, 72, 232), 1, 0.25),
    "C4": ("c4_textured", (128, 92, 160, 124), 0, 0.15),
}
H_BRIGHT, H_DIM, H_RADIUS = "0.5", "0.03125", 1.0  # intensities 2^-1 and 2^-5: a factor of exactly 2^4


def _diff(a, b):
    bad = np.argwhere(np.ascontiguousarray(a, f32).view(np.uint32) != np.ascontiguousarray(b, f32).view(np.uint32))
    return f"{len(bad)} of {a.size} values differ, first at {bad[:6].tolist()}"


def _differs(a, b):
    return (np.ascontiguousarray(a, f32).view(np.uint32) != np.ascontiguousarray(b, f32).view(np.uint32)).any(axis=-1)


def _pixels(region):
    x0, y0, x1, y1 = region
    jj, ii = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
    return np.stack([ii.ravel(), jj.ravel()], axis=1)  # the order of bhrt_render_samples


# ---------------------------------------------------------------------------------------------------- scenes and maps
@pytest.fixture(scope="module")
def scenes(B, tmp_path_factory):
    """tag -> this module's own handle of a scene (no device needed to make one); all closed when the module is done."""
    root = tmp_path_factory.mktemp("global_gather")
    made = {}

    def _h_text(intensity):
        t = open(os.path.join(SCENES, "c5_caustics.xml")).read()
        light = t[t.index('    <light type="point"'):t.index("  </scene>")]
        if intensity is None:
            return t.replace(light, "")
        assert t.count('<intensity value="100.5"/>') == 1
        return t.replace('<intensity value="100.5"/>', f'<intensity value="{intensity}"/>')

    def _get(tag):
        if tag not in made:
            if tag.startswith("H_"):
                path = root / (tag + ".xml")
                path.write_text(_h_text({"H_bright": H_BRIGHT, "H_dim": H_DIM, "H_dark": None}[tag]))
                made[tag] = B.Scene(str(path))
            else:
                made[tag] = B.Scene(os.path.join(SCENES, tag.split(":")[0] + ".xml"))  # "name:anything" = a further handle of the same file
            assert made[tag].warnings() == []
        return made[tag]
    yield _get
    for sc in made.values():
        sc.close()


@pytest.fixture(scope="module")
def gpu(B):
    if B.device_count() < 1:
        pytest.fail("no HIP device: the render path has no CPU fallback, GPU tests cannot run here")
    return B


_maps = {}


def _oracle_map(O, sc, name):
    """The oracle's global map of a scene file, built once; attached for O.photon_gather / O.photon_knn."""
    if name not in _maps:
        _maps[name] = O.photon_build_global(sc.flat_bytes(), N_MAP, seed=MAP_SEED)[0]
        _maps[name].setflags(write=False)
        assert len(_maps[name]) == N_MAP
    O.photon_attach(_maps[name])
    return _maps[name]


def _power(records):
    return np.ascontiguousarray(records[:, 12:16]).view(f32).ravel()


def _far_away(records):
    """The same records with every position translated by 10^4 along each axis: farther than any radius from every surface."""
    r = records.copy()
    pos = np.ascontiguousarray(r[:, :12]).view(f32) + f32(1e4)
    r[:, :12] = pos.view(np.uint8)
    return r


# ---------------------------------------------------------------------------------------------------- the expected frame at the cut-off
def _normalized(v):
    n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(f32)  # vecmath.h: length, normalized
    with np.errstate(invalid="ignore", divide="ignore"):
        return (v / n[:, None]).astype(f32)


def _g_term(kd, E, vL, N):
    """G in float32, in the order of the statement above.  kd, E, vL, N: (n, 3) float32."""
    vN = _normalized(N)
    cos = -((vL[:, 0] * vN[:, 0] + vL[:, 1] * vN[:, 1]) + vL[:, 2] * vN[:, 2]).astype(f32)
    g = np.minimum((f32(0) + (kd * E).astype(f32)).astype(f32), f32(1))  # Color::Black() + diffuse * E, ClampMax
    g = np.where((cos > 0)[:, None], g, f32(0)).astype(f32)
    g[np.isnan(g[:, 0])] = 0
    return g


def _cutoff_expected(O, sc, case, rays, seed):
    """(expected samples, G, the oracle's samples without the term) of a case at gi_bounces = -1, internal_bounces = 0, all (pixels, spp, 3).
    rays: the camera rays of the region's samples, (pixels, spp, 3) each.  The case's map is attached to the oracle."""
    name, region, jitter, radius = CASES[case]
    blob, fv = sc.flat_bytes(), sc.flat_view()
    o, d = rays
    h = O.trace_closest(blob, o.reshape(-1, 3), d.reshape(-1, 3), 1)
    p, N = np.ascontiguousarray(h["attrs"][:, 1:4]), np.ascontiguousarray(h["attrs"][:, 4:7])
    node_mtl = np.array([n.material for n in fv.nodes] + [-1], np.int32)  # [-1]: a miss
    mi = node_mtl[h["node"]]
    assert (mi[h["node"] >= 0] >= 0).all() and all(fv.materials[k].kind == 0 for k in np.unique(mi[mi >= 0]))  # first hits are Blinn materials (BHRT_MTL_BLINN)
    if jitter:  # plain colours: the blob's
        assert all(fv.materials[k].diffuse.map < 0 for k in np.unique(mi[mi >= 0]))
        kd = np.array([list(fv.materials[k].diffuse.color) if k >= 0 else [0, 0, 0] for k in mi], f32)
    else:  # diffuse.Sample(uvw, duvw) of the ray through the pixel corner: O.first_hit's albedo image
        assert any(fv.materials[k].diffuse.map >= 0 for k in np.unique(mi[mi >= 0]))
        px = _pixels(region)
        alb = O.first_hit(blob, sc.width, sc.height)[2][px[:, 1] * sc.width + px[:, 0]]
        kd = np.repeat(alb, SPP, axis=0).astype(f32)
    E, vL = O.photon_gather(p, N, radius)
    g = _g_term(kd, E, vL, N)
    g[h["node"] < 0] = 0  # a miss opens no frame
    g = g.reshape(o.shape)
    off = O.render(blob, sc.width, sc.height, SPP, gi=-1, bounces=0, seed=seed, jitter=jitter, region=region, threads=16)["samples"]
    white = (g >= 1).all(axis=-1, keepdims=True)  # Shade()'s early return behind the GI term
    return np.where(white, g, (g + off).astype(f32)).astype(f32), g, off


def _restated_rays(O, sc, case, seed):
    name, region, jitter, radius = CASES[case]
    o, d, _ = lens_rays_ref(O, sc.flat_view().header.camera, SPP, seed=seed, jitter=jitter, pixels=_pixels(region))
    return o, d


def _assert_cutoff_inputs(exp, g, off):
    assert (g != 0).any(axis=-1).mean() >= 0.25, (g != 0).any(axis=-1).mean()
    assert (g == 0).all(axis=-1).mean() >= 0.10, (g == 0).all(axis=-1).mean()
    assert _differs(exp, off).mean() >= 0.25, _differs(exp, off).mean()


@pytest.mark.parametrize("case", list(CASES))
def test_inputs_cutoff(B, O, scenes, case):
    """Region, map size and radius of section 2, held with the oracle alone."""
    sc = scenes(CASES[case][0])
    _oracle_map(O, sc, CASES[case][0])
    _assert_cutoff_inputs(*_cutoff_expected(O, sc, case, _restated_rays(O, sc, case, 0), 0))


def test_inputs_homogeneity(B, O, scenes):
    """Section 4: the two maps differ in the powers alone, by exactly 2^4; the dim map cannot reach the clamp; the dark scene is black."""
    bright = O.photon_build_global(scenes("H_bright").flat_bytes(), N_MAP, seed=MAP_SEED)[0]
    dim = O.photon_build_global(scenes("H_dim").flat_bytes(), N_MAP, seed=MAP_SEED)[0]
    assert len(bright) == len(dim) == N_MAP
    assert np.array_equal(_power(bright), f32(16) * _power(dim)) and (_power(dim) > 0).all()
    assert np.array_equal(np.delete(bright, slice(12, 16), axis=1), np.delete(dim, slice(12, 16), axis=1))
    assert float(_power(dim).astype(np.float64).sum()) / (np.pi * H_RADIUS ** 2) < 1 / 32
    dark = scenes("H_dark")
    assert dark.info.n_lights == 0
    hdr = dark.flat_view().header
    assert list(hdr.background.color) == [0, 0, 0] and list(hdr.environment.color) == [0, 0, 0] and hdr.background.map < 0 and hdr.environment.map < 0


# ---------------------------------------------------------------------------------------------------- 1. the estimate alone
@pytest.fixture(scope="module")
def c5(gpu, O, scenes):
    """c5_caustics uploaded, the oracle's global map installed with bhrt_global_map_set."""
    sc = scenes("c5_caustics")
    sc.upload(0)
    sc.global_map_set(_oracle_map(O, sc, "c5_caustics"))
    return sc


def _first_hit_points(O, sc, step=8):
    po, pd = O.primary_rays(sc.flat_view())
    W, H = sc.width, sc.height
    keep = ((np.arange(W * H) % W) % step == 0) & ((np.arange(W * H) // W) % step == 0)
    h = O.trace_closest(sc.flat_bytes(), po[keep], pd[keep], 1)
    hit = h["node"] >= 0
    return np.ascontiguousarray(h["attrs"][hit, 1:4]), np.ascontiguousarray(h["attrs"][hit, 4:7])


@pytest.mark.gpu
def test_estimate_is_the_oracles(gpu, O, c5):
    m = _oracle_map(O, c5, "c5_caustics")
    assert np.array_equal(c5.global_map_get(), m)  # installed as they are
    p, n = _first_hit_points(O, c5)
    assert len(p) >= 1000
    # photon_exact = 1 at a radius where part of the queries meet 1000 photons: the candidate heap's history
    _, cnt, _ = O.photon_knn(p, n, 10.0)
    assert (cnt == 1000).mean() >= 0.10 and ((cnt > 0) & (cnt < 1000)).mean() >= 0.10
    E, vL = O.photon_gather(p, n, 10.0)
    ge, gd = c5.global_gather(p, n, 10.0, exact=True)
    assert same_bits(ge, E) and same_bits(gd, vL), _diff(ge, E)
    # photon_exact = 0 where no query reaches 1000 photons: the walk-order sums
    _, cnt, _ = O.photon_knn(p, n, 0.5)
    assert cnt.max() < 1000 and (cnt > 0).mean() >= 0.5
    E, vL = O.photon_gather(p, n, 0.5)
    ge, gd = c5.global_gather(p, n, 0.5, exact=False)
    assert same_bits(ge, E) and same_bits(gd, vL), _diff(ge, E)
    assert (E != 0).any(axis=-1).mean() >= 0.5


# ---------------------------------------------------------------------------------------------------- 2. the pin at the cut-off
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
@pytest.mark.parametrize("case", list(CASES))
def test_cutoff_frame_is_g_plus_the_oracles_sample(gpu, O, scenes, case, seed):
    name, region, jitter, radius = CASES[case]
    sc = scenes(name)
    sc.upload(0)
    sc.global_map_set(_oracle_map(O, sc, name))
    opts = gpu.default_opts(spp=SPP, gi_bounces=-1, internal_bounces=0, seed=seed, jitter=jitter, photon_exact=1)
    rays = sc.camera_rays(opts, region)
    ro, rd = _restated_rays(O, sc, case, seed)
    assert same_bits(rays[0], ro) and same_bits(rays[1], rd)  # the premise of test_inputs_cutoff
    exp, g, off = _cutoff_expected(O, sc, case, rays, seed)
    _assert_cutoff_inputs(exp, g, off)
    try:
        sc.set_global_gather(False)
        gs_off, _ = sc.render_samples(opts, *region)
        sc.set_global_gather(True, radius)
        gs, st = sc.render_samples(opts, *region)
    finally:
        sc.set_global_gather(False)
    assert same_bits(gs_off, off), _diff(gs_off, off)
    # bhrt_render_samples renders the whole frame and hands back the region: every camera sample of the frame whose first hit is a Blinn material
    # opens a root frame with gi = -1, and with internal_bounces = 0 there are no other frames
    fo, fd, _ = lens_rays_ref(O, sc.flat_view().header.camera, SPP, seed=seed, jitter=jitter)
    fh = O.trace_closest(sc.flat_bytes(), fo.reshape(-1, 3), fd.reshape(-1, 3), 1)
    fv = sc.flat_view()
    blinn = np.array([n.material >= 0 and fv.materials[n.material].kind == 0 for n in fv.nodes] + [False])  # [False]: a miss
    assert st.camera_samples == sc.width * sc.height * SPP
    assert st.global_gather_queries == int(blinn[fh["node"]].sum())
    assert same_bits(gs, exp), _diff(gs, exp)


# ---------------------------------------------------------------------------------------------------- 3. nothing in reach, nothing changes
@pytest.mark.gpu
@pytest.mark.parametrize("photon_map", [0, 1])
@pytest.mark.parametrize("gi", [0, 1, 3])
def test_map_out_of_reach_changes_nothing(gpu, O, scenes, gi, photon_map):
    region = CASES["C5"][1]
    sc = scenes("c5_caustics:far")
    sc.upload(0)
    far = _far_away(_oracle_map(O, sc, "c5_caustics"))
    assert (np.ascontiguousarray(far[:, :12]).view(f32) > 9000).all()
    sc.global_map_set(far)
    if photon_map:
        assert sc.photon_build(gpu.default_opts(seed=MAP_SEED), N_CAUSTIC) == N_CAUSTIC
    opts = gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=16, seed=9, photon_map=photon_map)
    try:
        sc.set_global_gather(False)
        off, st0 = sc.render_samples(opts, *region)
        sc.set_global_gather(True, 0.5)
        on, st = sc.render_samples(opts, *region)
    finally:
        sc.set_global_gather(False)
    assert st0.global_gather_queries == 0 and st.global_gather_queries > 0 and st.global_gather_heavy_queries == 0
    assert st.photon_queries == st0.photon_queries and (st.photon_queries > 0) == bool(photon_map)
    assert same_bits(on, off), _diff(on, off)


# ---------------------------------------------------------------------------------------------------- 4. homogeneity at depth
@pytest.mark.gpu
def test_sixteen_times_the_power_is_sixteen_times_the_frame(gpu, O, scenes):
    region = CASES["C5"][1]
    built = {}
    for tag in ("H_bright", "H_dim"):  # the device's own builds
        s = scenes(tag)
        s.upload(0)
        built[tag] = s.photon_build_global(gpu.default_opts(seed=MAP_SEED), N_MAP)
    bright, dim = built["H_bright"], built["H_dim"]
    assert len(bright) == len(dim) == N_MAP
    assert np.array_equal(_power(bright), f32(16) * _power(dim)) and (_power(dim) > 0).all()
    assert np.array_equal(np.delete(bright, slice(12, 16), axis=1), np.delete(dim, slice(12, 16), axis=1))
    assert float(_power(dim).astype(np.float64).sum()) / (np.pi * H_RADIUS ** 2) < 1 / 32  # no clamp in either render
    dark = scenes("H_dark")
    dark.upload(0)
    for gi in (0, 2):
        opts = gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=0, seed=9)
        dark.set_global_gather(False)
        zero, _ = dark.render_samples(opts, *region)
        assert (zero == 0).all()  # the direct term is exactly zero: no light, black background and environment
        try:
            dark.set_global_gather(True, H_RADIUS)
            dark.global_map_set(bright)
            sb, _ = dark.render_samples(opts, *region)
            dark.global_map_set(dim)
            sd, _ = dark.render_samples(opts, *region)
        finally:
            dark.set_global_gather(False)
        assert (sd != 0).any(axis=-1).mean() >= 0.25
        assert same_bits(sb, (f32(16) * sd).astype(f32)), _diff(sb, f32(16) * sd)


# ---------------------------------------------------------------------------------------------------- 5. off is off
def test_switch_needs_no_device_and_keeps_the_blob(B, scenes):
    sc = scenes("c5_caustics:host")
    before = bytes(sc.flat_bytes())
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(B.BhrtError, match=ERR_ARG):
            sc.set_global_gather(True, bad)
    opts = B.default_opts(spp=1)
    sc.set_global_gather(True, 0.25)
    sc._flat = None
    assert bytes(sc.flat_bytes()) == before
    for call in (lambda s: s.render(opts), lambda s: s.render_samples(opts, 0, 0, 4, 4), lambda s: s.render_var(opts),
                 lambda s: s.render_adaptive(B.default_opts(spp=4), B.default_adaptive_opts(min_spp=2))):
        with pytest.raises(B.BhrtError, match=ERR_ARG + ".*global"):  # the switch is on and no map is installed: refused before a device is looked for
            call(sc)
        cl = sc.clone()  # carries the switch
        try:
            with pytest.raises(B.BhrtError, match=ERR_ARG + ".*global"):
                call(cl)
        finally:
            cl.close()
    with pytest.raises(B.BhrtError, match=ERR_ARG):
        sc.global_map_get()
    sc.global_map_set(None)  # removing a map that is not there needs no device either
    sc.set_global_gather(False)
    assert B.default_opts().photon_map == 0 and B.default_opts().gi_bounces == 3


@pytest.mark.gpu
def test_off_is_the_parents_frame_and_the_caustic_map_is_untouched(gpu, O, scenes):
    region = CASES["C5"][1]
    sc = scenes("c5_caustics:off")
    before = bytes(sc.flat_bytes())
    sc.upload(0)
    assert sc.photon_build(gpu.default_opts(seed=MAP_SEED), N_CAUSTIC) == N_CAUSTIC
    caustic = sc.photon_get()
    for photon_map in (0, 1):
        opts = gpu.default_opts(spp=SPP, gi_bounces=1, internal_bounces=16, seed=9, photon_map=photon_map, photon_exact=1)
        if photon_map:
            O.photon_attach(caustic)
        parent = O.render(sc.flat_bytes(), sc.width, sc.height, SPP, gi=1, bounces=16, seed=9, region=region, threads=16, photon=photon_map)["samples"]
        sc.global_map_set(None)
        sc.set_global_gather(False)
        a, _ = sc.render_samples(opts, *region)  # never switched on
        sc.global_map_set(_oracle_map(O, sc, "c5_caustics"))
        b, st_b = sc.render_samples(opts, *region)  # a map installed, the switch off
        sc.set_global_gather(True, 0.5)
        on, st_on = sc.render_samples(opts, *region)
        sc.set_global_gather(False)
        c, _ = sc.render_samples(opts, *region)  # on, then off
        for got in (a, b, c):
            assert same_bits(got, parent), _diff(got, parent)
        assert _differs(on, parent).mean() >= 0.25
        assert st_b.global_gather_queries == 0 and st_on.global_gather_queries > 0
        assert np.array_equal(sc.photon_get(), caustic)
    assert sc.global_map_build(gpu.default_opts(seed=MAP_SEED), N_MAP) == N_MAP  # the device's build into the slot: the oracle's map
    assert np.array_equal(sc.global_map_get(), _oracle_map(O, sc, "c5_caustics"))
    assert np.array_equal(sc.photon_get(), caustic)
    sc._flat = None
    assert bytes(sc.flat_bytes()) == before


@pytest.mark.gpu
def test_clone_carries_switch_and_radius_but_no_map(gpu, O, scenes):
    region = CASES["C5"][1]
    sc = scenes("c5_caustics:clone")
    sc.upload(0)
    m = _oracle_map(O, sc, "c5_caustics")
    sc.global_map_set(m)
    opts = gpu.default_opts(spp=SPP, gi_bounces=0, internal_bounces=0, seed=9)
    try:
        sc.set_global_gather(True, 0.25)
        want, _ = sc.render_samples(opts, *region)
        sc.set_global_gather(True, 0.0)  # 0 = the reference's 0.5
        other, _ = sc.render_samples(opts, *region)
        sc.set_global_gather(True, 0.5)
        half, _ = sc.render_samples(opts, *region)
        assert same_bits(other, half) and _differs(want, other).mean() >= 0.25
        sc.set_global_gather(True, 0.25)
        cl = sc.clone()
        try:
            cl.upload(0)
            with pytest.raises(gpu.BhrtError, match=ERR_ARG + ".*global"):  # the switch came along, the map did not
                cl.render_samples(opts, *region)
            cl.global_map_set(sc.global_map_get())
            got, _ = cl.render_samples(opts, *region)
            assert same_bits(got, want), _diff(got, want)
        finally:
            cl.close()
    finally:
        sc.set_global_gather(False)


# ---------------------------------------------------------------------------------------------------- 6. independence of path
@pytest.mark.gpu
@pytest.mark.parametrize("emission", [0, 1])
def test_on_frame_does_not_depend_on_the_path(gpu, O, B, scenes, tmp_path, emission):
    from bhraytracer_amd import dist
    if emission:  # emitters that are lit: the walls of c5_caustics, through the setter
        sc = scenes("c5_caustics:emit")
        sc.set_emissive(True)
        sc.set_material_emission(sc.material_index("wall"), (0.03125, 0.0625, 0.015625))
    else:
        sc = scenes("c5_caustics:path")
    sc.upload(0)
    sc.global_map_set(_oracle_map(O, sc, "c5_caustics"))
    W, H, tile = sc.width, sc.height, 8
    region = CASES["C5"][1]
    kw = dict(spp=SPP, gi_bounces=1, internal_bounces=16, seed=9)
    try:
        sc.set_global_gather(False)
        off, _ = sc.render_samples(gpu.default_opts(**kw), *region)
        sc.set_global_gather(True, 0.5)
        want, st = sc.render_samples(gpu.default_opts(**kw), *region)
        assert st.passes == 1 and st.global_gather_queries > 0 and _differs(want, off).mean() >= 0.25
        # small passes
        got, st2 = sc.render_samples(gpu.default_opts(samples_per_pass=W * H * SPP // 3, **kw), *region)
        assert st2.passes >= 3 and same_bits(got, want), _diff(got, want)
        assert st2.global_gather_queries == st.global_gather_queries
        # two rehearsed ranks, stitched
        px = _pixels(region)
        stitched = np.zeros_like(want)
        for rank in (0, 1):
            own = dist.owned_mask(W, H, tile, rank, 2).numpy().reshape(-1)[px[:, 1] * W + px[:, 0]]
            part, _ = sc.render_samples(gpu.default_opts(rank=rank, world_size=2, tile_size=tile, **kw), *region)
            assert 0 < own.sum() < len(px)
            stitched[own] = part[own]
        assert same_bits(stitched, want), _diff(stitched, want)
        # the resolve straight from the root frames and through the sample buffer
        frames = {}
        for fused in (1, 0):
            try:
                sc.knob("fused_resolve", fused)
                rgb, rad, stf = sc.render(gpu.default_opts(**kw))
            finally:
                sc.knob("fused_resolve", 1)
            assert stf.launches_resolve_fused == (stf.passes if fused else 0)
            frames[fused] = (rgb, rad)
        assert same_bits(frames[0][1], frames[1][1]) and np.array_equal(frames[0][0], frames[1][0])
        mean = (want[:, 0] + want[:, 1]) / f32(SPP)  # k_resolve: the samples added from zero in order, divided by (float)spp
        assert same_bits(frames[1][1][px[:, 1], px[:, 0]], mean.astype(f32))
    finally:
        sc.set_global_gather(False)
