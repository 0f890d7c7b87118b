"""The caustic photon map under the three scene switches: emission, face materials and the thin lens.
The feature files (test_emission.py, test_face_materials.py, test_lens.py) render with photon_map = 0; here every render has photon_map = 1, and the
oracle pins the frames bit for bit with the tricks of those files: the white body, the one add, the blob patched to sub-material k, the camera at
the sample's lens point.  Their helpers are imported from them.

The map: the GPU builds it from the scene as loaded (the patches exist for the oracle only, so they cannot change which photons there are), it is
read back with photon_get() and handed to the oracle with photon_attach; test_gpu_map_is_the_oracles_map holds it equal to the oracle's own build.
Every comparison with the oracle is on bits and runs with photon_exact = 1, except section 6.  33 x 17 pixels, spp 3.

Scenes (variants written to a temporary directory):
  E   emission_room.xml with the point light of test_emission.py (intensity 60) at (4, -26, 18) and the glass sphere, scale 3, at (6, -16, 12), between
      the light and the ball: the ball lies near the focus, where the caustic alone takes the direct term over white, and the photons the glass
      reflects reach the walls and the lamp.  Sections 1 and 2.
  F   facemtl_room.xml with the light at (0.3, -28, 22) and the glass sphere, scale 1.5, at (0.3, -23, 17.5): above the camera's line of sight, between
      the light and the mesh, whose camera side lies behind the focus in the widened beam: all three face groups receive photons.  Sections 3 and 5.
  L   c5_caustics.xml at 33 x 17, focal distance 54 (the floor under the glass sphere), aperture 1.  Section 4.

test_inputs_* (no GPU) hold the conditions on these inputs with the oracle alone: for every material a case is about, at least 20 compared samples
whose first hit is that material and whose oracle sample with the photon term differs from the one without.  The first hits come from the camera
rays restated in test_lens.py (lens_rays_ref), which the GPU tests hold equal to bhrt_camera_rays."""
import os
import re
import shutil

import numpy as np
import pytest

from conftest import SCENES, same_bits
from test_emission import LIGHT, _diff, _material_offset, _sub, _white_blob
from test_face_materials import _face_end, _multi, _obj_uniform, _patched_blob
from test_lens import lens_rays_ref, patched_pos

W, H, SPP = 33, 17, 3
N_EF, N_L = 20000, 5000  # photons of the maps of E / F and of L
MAP_SEED = 0
MIN_LIT = 20
COMBOS = [(gi, ib, seed) for gi in (-1, 0, 3) for ib in (0, 16) for seed in (0, 9)]
FM_COMBOS = [(-1, 0, 0), (-1, 0, 9), (0, 16, 0), (3, 0, 9), (3, 16, 0), (3, 16, 9)]
L_FOCALDIST, L_DOF, L_GI, L_SEED = 54.0, 1.0, 3, 9
L_FLOOR = 1  # c5_caustics: node 0 is the group "box", node 1 its first child, WallBottom (test_inputs_lens_floor checks that its hits have z = 0)
BAR = 1e-4  # README, "Parity bar": absolute, on radiance


# ---------------------------------------------------------------------------------------------------- scenes
def _text(name):
    return open(os.path.join(SCENES, name)).read()


def _e_text():
    t = _sub(_text("emission_room.xml"), '<scale value="4"/>\n      <translate x="-9" y="-6" z="4"/>', '<scale value="3"/>\n      <translate x="6" y="-16" z="12"/>')
    return _sub(t, "  </scene>", _sub(LIGHT, '<position x="0" y="-10" z="20"/>', '<position x="4" y="-26" z="18"/>'))


def _e_plain():
    """Section 2: coloured emitters on lit bodies that are not black (the lamp's body is black in the committed scene)."""
    t = _sub(_e_text(), '<diffuse value="0"/>\n      <specular value="0"/>\n      <emission r="1" g="1" b="1"/>',
             '<diffuse r="0.5" g="0.6" b="0.4"/>\n      <specular value="0"/>\n      <emission r="0.25" g="0.5" b="2.0"/>')
    return _sub(t, '<diffuse r="0.8" g="0.3" b="0.3"/>', '<diffuse r="0.6" g="0.5" b="0.4"/>\n      <emission r="0.125" g="0" b="0.0625"/>')


def _e_textured():
    """Section 2: the lamp's emission through a checkerboard, the ball's through the image file."""
    t = _sub(_e_text(), '<diffuse value="0"/>\n      <specular value="0"/>\n      <emission r="1" g="1" b="1"/>',
             '<diffuse r="0.5" g="0.6" b="0.4"/>\n      <specular value="0"/>\n      <emission r="1" g="0.5" b="2" texture="checkerboard">\n'
             '        <color1 r="0.25" g="1" b="0.5"/>\n        <color2 r="1" g="0.125" b="0.75"/>\n        <scale x="0.3" y="0.2"/>\n      </emission>')
    return _sub(t, '<diffuse r="0.8" g="0.3" b="0.3"/>', '<diffuse r="0.6" g="0.5" b="0.4"/>\n      <emission r="0.5" g="1" b="0.75" texture="tex_small.png"/>')


def _f_text():
    t = _sub(_text("facemtl_room.xml"), '<scale value="4"/>\n      <translate x="-9" y="-6" z="4"/>', '<scale value="1.5"/>\n      <translate x="0.3" y="-23" z="17.5"/>')
    return _sub(t, '<position x="4" y="-14" z="21"/>', '<position x="0.3" y="-28" z="22"/>')


def _l_text():
    t, n1 = re.subn(r'<width value="\d+"/>', f'<width value="{W}"/>', _text("c5_caustics.xml"))
    t, n2 = re.subn(r'<height value="\d+"/>', f'<height value="{H}"/>', t)
    assert n1 == 1 and n2 == 1
    return t


# role -> (scene text, text of facemtl.obj or None for the committed one, photons).  One handle per role: the switches are state of a handle.
ROLES = {
    "E": (_e_text, None, N_EF), "E_plain": (_e_plain, None, N_EF), "E_textured": (_e_textured, None, N_EF),
    "F": (_f_text, None, N_EF), "F_off": (_f_text, None, N_EF), "F_all": (_f_text, None, N_EF),
    "F_uniform1": (_f_text, lambda: _obj_uniform(1), N_EF), "F_uniform2": (_f_text, lambda: _obj_uniform(2), N_EF),
    "L": (_l_text, None, N_L), "L_closed": (_l_text, None, N_L),
}


def _prepare(role, sc):
    """The switches of a role, set before the upload (the upload carries them)."""
    if role.startswith("E"):
        sc.set_emissive(True)
    if role in ("F", "F_uniform1", "F_uniform2", "F_all"):
        sc.set_face_materials(True)
    if role == "F_all":
        sc.set_emissive(True)
        sc.set_material_emission(sc.material_index("lamp"), (0.25, 0.5, 2.0))
        sc.set_material_emission(sc.material_index("ball"), (0.125, 0, 0.0625))
        sc.set_material_emission(sc.material_index("wall"), (0.03125, 0.0625, 0.015625))
        sc.set_lens(dof=0.5)
    if role == "L":
        sc.set_lens(focaldist=L_FOCALDIST, dof=L_DOF)
    if role == "L_closed":
        sc.set_lens(focaldist=L_FOCALDIST, dof=0.0)


@pytest.fixture(scope="module")
def host(B, tmp_path_factory):
    """role -> its scene handle with the role's switches set, not uploaded (no device needed); freed when the module is done."""
    root = tmp_path_factory.mktemp("photon_switches")
    made = {}

    def _get(role):
        if role not in made:
            text, obj, _ = ROLES[role]
            d = root / role
            d.mkdir()
            for asset in ("mesh_small.obj", "tex_small.png", "facemtl.obj", "facemtl.mtl"):
                shutil.copy(os.path.join(SCENES, asset), d / asset)
            if obj is not None:
                (d / "facemtl.obj").write_text(obj())
            (d / "scene.xml").write_text(text())
            sc = B.Scene(str(d / "scene.xml"))
            assert sc.warnings() == []
            _prepare(role, sc)
            made[role] = sc
        return made[role]
    yield _get
    for sc in made.values():
        sc.close()


@pytest.fixture(scope="module")
def gpu(B):
    if B.device_count() < 1:
        pytest.fail("no HIP device: the render path has no CPU fallback, GPU tests cannot run here")
    return B


@pytest.fixture(scope="module")
def dev(gpu, host):
    """role -> (scene uploaded with its caustic map built on the GPU, that map as photon_get() returns it)."""
    ready = {}

    def _get(role):
        if role not in ready:
            sc = host(role)
            sc.upload(0)
            n = sc.photon_build(gpu.default_opts(seed=MAP_SEED), ROLES[role][2])
            assert n == ROLES[role][2]
            got = sc.photon_get()
            got.setflags(write=False)
            ready[role] = (sc, got)
        return ready[role]
    return _get


_maps = {}


def _oracle_map(O, sc, role):
    """The oracle's own build of the role's map from the blob as loaded, once; it stays attached."""
    key = (ROLES[role][0].__name__, role if ROLES[role][1] else None, ROLES[role][2])  # the switches and the camera do not reach the blob's scene
    if key not in _maps:
        _maps[key] = O.photon_build(sc.flat_bytes(), ROLES[role][2], seed=MAP_SEED)[0]
        _maps[key].setflags(write=False)
    O.photon_attach(_maps[key])
    return _maps[key]


def _opts(B, gi, ib, seed, **kw):
    kw.setdefault("photon_exact", 1)
    return B.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed, photon_map=1, **kw)


def _render(O, blob, gi, ib, seed, photon, jitter=1):
    r = O.render(blob, W, H, SPP, gi=gi, bounces=ib, seed=seed, jitter=jitter, threads=16, photon=photon)
    for a in (r["samples"], r["radiance"], r["rgb8"]):
        a.setflags(write=False)
    return r


def _lit(O, blob, gi, ib, seed, jitter=1):
    """(the oracle's samples with the photon term, the mask of those that differ from the samples without it) under the attached map."""
    on = _render(O, blob, gi, ib, seed, 1, jitter)["samples"]
    off = _render(O, blob, gi, ib, seed, 0, jitter)["samples"]
    return on, (on.view(np.uint32) != off.view(np.uint32)).any(axis=-1)


def _rays(O, sc, seed, jitter=1, lens=0):
    cam = sc.flat_view().header.camera
    o, d, _ = lens_rays_ref(O, cam, SPP, seed=seed, jitter=jitter, lens_r=cam.dof if lens else 0.0)
    return o, d


def _first_hits(O, sc, seed, jitter=1, lens=0):
    """(pixels, spp) arrays of the camera samples' first hits: node, face, material (-1: a miss or a node without material)."""
    o, d = _rays(O, sc, seed, jitter, lens)
    h = O.trace_closest(sc.flat_bytes(), o.reshape(-1, 3), d.reshape(-1, 3), 1)
    node_mtl = np.array([n.material for n in sc.flat_view().nodes] + [-1], np.int32)  # [-1]: a miss
    shape = o.shape[:2]
    return h["node"].reshape(shape), h["prim"].reshape(shape), node_mtl[h["node"]].reshape(shape), (o + h["t"].reshape(shape)[..., None] * d)


def _assert_rays(sc, O, opts):
    """The premise of every first-hit mask: the restated camera rays are the device's."""
    o, d = sc.camera_rays(opts)
    ro, rd = _rays(O, sc, opts.seed, opts.jitter, opts.lens)
    assert same_bits(o, ro) and same_bits(d, rd)


def _groups(O, sc, seed):
    """(pixels, spp): the face group of the first hit, -1 off the mesh (test_face_materials._first_hit_group, from the restated rays)."""
    _, prim, mtl, _ = _first_hits(O, sc, seed)
    fe = _face_end(sc)
    g = np.searchsorted(fe, prim, side="right")
    assert (g[mtl == _multi(sc)] < len(fe)).all()  # every face of the mesh has a group
    return np.where(mtl == _multi(sc), g, -1)


# ---------------------------------------------------------------------------------------------------- 0. the inputs (no GPU)
def _one_add_inputs(O, sc, role, seed):
    """Section 2's expectation and its conditions under the attached map: (expected samples, per material: lit count, count of lit samples whose direct term with the
    caustic is clamped at white in a channel where Le is not 0)."""
    jitter = 0 if role == "E_textured" else 1
    _, _, mtl, _ = _first_hits(O, sc, seed, jitter)
    base, lit = _lit(O, sc.flat_bytes(), -1, 0, seed, jitter)
    if role == "E_textured":
        le = np.repeat(_le_image(O, sc)[:, None, :], SPP, axis=1)
    else:
        table = np.array([sc.material_emission(m)[0] for m in range(sc.info.n_materials)] + [(0, 0, 0)], np.float32)  # [-1]: no material, no emission
        le = table[mtl]
    exp = base + le  # float32 + float32: the one addition
    assert exp.dtype == np.float32
    counts = {}
    for name in ("lamp", "ball"):
        m = mtl == sc.material_index(name)
        clamped = ((base == 1) & (le != 0)).any(axis=-1)
        counts[name] = (int((m & lit).sum()), int((m & lit & clamped).sum()))
    return exp, counts


def _le_image(O, sc):
    """Le of every pixel's un-jittered first hit: the oracle's albedo image of a blob whose diffuse TexturedColor is the emission one
    (test_emission.test_one_add_textured_emission)."""
    from bhraytracer_amd import flat
    fv = sc.flat_view()
    b = bytearray(sc.flat_bytes())
    for m in range(sc.info.n_materials):
        (r, g, bl), tm = sc.material_emission(m)
        off = _material_offset(fv, m) + flat.Material.diffuse.offset
        b[off:off + 16] = bytes(flat.TexColor((r, g, bl), tm))
    return O.first_hit(bytes(b), W, H)[2]


def _check_one_add_counts(counts):
    print(counts)
    for name, (lit, clamped) in counts.items():
        assert lit >= MIN_LIT, (name, lit)
    assert sum(c for _, c in counts.values()) > 0, counts  # + Le behind the clamp of the caustic-lit direct term: such samples are compared


@pytest.mark.parametrize("role,seed", [("E_plain", 0), ("E_plain", 9), ("E_textured", 0)])
def test_inputs_one_add_bodies_receive_photons(O, host, role, seed):
    sc = host(role)
    _oracle_map(O, sc, role)
    exp, counts = _one_add_inputs(O, sc, role, seed)
    _check_one_add_counts(counts)
    le_lamp, le_ball = sc.material_emission(sc.material_index("lamp")), sc.material_emission(sc.material_index("ball"))
    assert (le_lamp[1] >= 0) == (le_ball[1] >= 0) == (role == "E_textured")


def _fm_counts(O, sc, role, seed, groups_of):
    """Per group k of groups_of: the samples whose first hit is a face of group k and whose oracle sample of the blob patched to k, without child
    frames, has a caustic term (the term of that very hit)."""
    _oracle_map(O, sc, role)
    g = _groups(O, sc, seed)
    return {k: int((_lit(O, _patched_blob(sc, k), -1, 0, seed)[1] & (g == k)).sum()) for k in groups_of}


@pytest.mark.parametrize("seed", [0, 9])
def test_inputs_every_face_group_receives_photons(O, host, seed):
    counts = {"mixed": _fm_counts(O, host("F"), "F", seed, (0, 1, 2))}
    for k in (1, 2):
        counts[f"uniform{k}"] = _fm_counts(O, host(f"F_uniform{k}"), f"F_uniform{k}", seed, (k,))
    print(counts)
    for case, per_group in counts.items():
        for k, n in per_group.items():
            assert n >= MIN_LIT, (case, k, n)


def _with_glossiness_of(sc, blob_k, k0):
    """blob_k (the blob patched to a sub-material) with only the MultiMtl's glossiness replaced by sub-material k0's."""
    from bhraytracer_amd import flat
    off = _material_offset(sc.flat_view(), _multi(sc)) + flat.Material.glossiness.offset
    b = bytearray(blob_k)
    b[off:off + 4] = np.float32(sc.submaterial(_multi(sc), k0)[0].glossiness).tobytes()
    return bytes(b)


@pytest.mark.parametrize("role", ["F", "F_uniform1"])
def test_inputs_m1_glossiness_shows_in_the_photon_render(O, host, role):
    """What separates the extended material table from the blob's, and the face's index from the node's, in GatherToFrames: m1's Ns 80 against m0's
    Ns 8.  The oracle's photon render of the blob patched to m1 differs from the one with m0's glossiness in m1's record, on samples whose first
    hit is m1 and has a caustic term."""
    sc = host(role)
    mm = _multi(sc)
    assert sc.submaterial(mm, 1)[0].glossiness == 80 and sc.submaterial(mm, 0)[0].glossiness == 8
    _oracle_map(O, sc, role)
    g = _groups(O, sc, 0)
    m1 = _patched_blob(sc, 1)
    a, lit = _lit(O, m1, -1, 0, 0)
    b = _render(O, _with_glossiness_of(sc, m1, 0), -1, 0, 0, 1)["samples"]
    differ = (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1)
    print(role, "m1 first hits with a caustic term:", int((lit & (g == 1)).sum()), "of which differ under m0's glossiness:", int((differ & lit & (g == 1)).sum()))
    assert (differ & lit & (g == 1)).sum() >= MIN_LIT


def _lens_oracle(O, B, sc, seed, gi, photon, o=None):
    """Per-sample radiance of the lens render: the oracle with the camera position at each sample's lens point
    (test_lens.test_lens_radiance_equals_the_oracle_with_the_lens_origin_as_camera_position), every sample of the frame."""
    if o is None:
        o, _ = _rays(O, sc, seed, lens=1)
    blob = sc.flat_bytes()
    out = np.zeros((W * H, SPP, 3), np.float32)
    for p in range(W * H):
        i, j = p % W, p // W
        for s in range(SPP):
            out[p, s] = O.render(patched_pos(B, blob, o[p, s]), W, H, s + 1, gi=gi, seed=seed, region=(i, j, i + 1, j + 1), threads=1, photon=photon)["samples"][0, s]
    return out


def _lens_inputs(O, B, sc):
    node, _, _, p = _first_hits(O, sc, L_SEED, lens=1)
    floor = node == L_FLOOR
    assert floor.sum() > 0 and np.abs(p[floor][:, 2]).max() <= 1e-3  # node L_FLOOR is the floor, z = 0
    on = _lens_oracle(O, B, sc, L_SEED, L_GI, 1)
    off = _lens_oracle(O, B, sc, L_SEED, L_GI, 0)
    lit = (on.view(np.uint32) != off.view(np.uint32)).any(axis=-1)
    cam = sc.flat_view().header.camera
    depth = (p - np.array(list(cam.pos), np.float32)) @ np.array(list(cam.dir), np.float32)
    in_focus = floor & (np.abs(depth - L_FOCALDIST) <= 0.25 * L_FOCALDIST)
    return on, int((lit & in_focus).sum())


def test_inputs_lens_floor_receives_photons(B, O, host):
    sc = host("L")
    cam = sc.flat_view().header.camera
    assert cam.dof == L_DOF and cam.focaldist == L_FOCALDIST and (cam.width, cam.height) == (W, H)
    _oracle_map(O, sc, "L")
    _, n = _lens_inputs(O, B, sc)
    print("lit samples of the floor within a quarter of the focal distance of the plane of focus:", n)
    assert n >= MIN_LIT


# ---------------------------------------------------------------------------------------------------- the map
@pytest.mark.gpu
@pytest.mark.parametrize("role", ["E", "E_plain", "F", "F_uniform1", "F_uniform2", "L"])
def test_gpu_map_is_the_oracles_map(O, dev, role):
    """Emission with the switches of the role on: the map is the one of the blob as loaded (face materials: photon emission ignores the
    sub-materials), every byte."""
    sc, got = dev(role)
    assert np.array_equal(got, _oracle_map(O, sc, role))


def _attach(O, role, dev):
    sc, got = dev(role)
    O.photon_attach(got)
    return sc


# ---------------------------------------------------------------------------------------------------- 1. emission x photon, white body
_white = {}


def _white_expected(O, sc, gi, ib, seed):
    key = (gi, ib, seed)
    if key not in _white:
        _white[key] = _render(O, _white_blob(sc), gi, ib, seed, 1)
    return _white[key]


@pytest.mark.gpu
@pytest.mark.parametrize("gi,ib,seed", COMBOS)
def test_white_body_equivalence(gpu, O, dev, gi, ib, seed):
    sc = _attach(O, "E", dev)
    opts = _opts(gpu, gi, ib, seed)
    exp = _white_expected(O, sc, gi, ib, seed)["samples"]
    # not an empty comparison: the lamp is in view and black without the term, and the photon term is in the expected frame
    _assert_rays(sc, O, opts)
    lamp_first = _first_hits(O, sc, seed)[2] == sc.material_index("lamp")
    assert lamp_first.mean() >= 0.05
    assert np.all(_render(O, sc.flat_bytes(), gi, ib, seed, 1)["samples"][lamp_first].view(np.uint32) == 0)
    no_photon = _render(O, _white_blob(sc), gi, ib, seed, 0)["samples"]
    assert (exp.view(np.uint32) != no_photon.view(np.uint32)).any(axis=-1).sum() >= MIN_LIT
    gs, st = sc.render_samples(opts, 0, 0, W, H)
    assert st.camera_samples == W * H * SPP and st.photon_queries > 0
    assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("gi,ib,seed", [(3, 16, 0), (0, 0, 9)])
def test_white_body_resolved_frame_both_ways(gpu, O, dev, fused, gi, ib, seed):
    """radiance and rgb8: k_resolve_frames<kTex, true> and k_combine<true> + k_resolve, each with photon = 1."""
    sc = _attach(O, "E", dev)
    exp = _white_expected(O, sc, gi, ib, seed)
    try:
        sc.knob("fused_resolve", fused)
        rgb, rad, st = sc.render(_opts(gpu, gi, ib, seed))
    finally:
        sc.knob("fused_resolve", 1)
    assert st.launches_resolve_fused == (st.passes if fused else 0) and st.photon_queries > 0
    assert same_bits(rad, exp["radiance"]), _diff(rad, exp["radiance"])
    assert np.array_equal(rgb, exp["rgb8"])


# ---------------------------------------------------------------------------------------------------- 2. emission x photon, one add
@pytest.mark.gpu
@pytest.mark.parametrize("role,seed", [("E_plain", 0), ("E_plain", 9), ("E_textured", 0)])
def test_one_add_behind_the_caustic_clamp(gpu, O, dev, role, seed):
    """Without child frames a sample is the oracle's photon sample + Le of its first hit: Le is added behind the clamp of direct + caustic."""
    sc = _attach(O, role, dev)
    opts = _opts(gpu, -1, 0, seed, jitter=0 if role == "E_textured" else 1)
    _assert_rays(sc, O, opts)
    exp, counts = _one_add_inputs(O, sc, role, seed)
    _check_one_add_counts(counts)
    gs, st = sc.render_samples(opts, 0, 0, W, H)
    assert st.photon_queries > 0
    assert same_bits(gs, exp), _diff(gs, exp)


# ---------------------------------------------------------------------------------------------------- 3. face materials x photon
_fm = {}


def _fm_expected(O, sc, role, k, gi, ib, seed):
    """The oracle's photon render of the role's blob patched to sub-material k (None: as loaded) under the attached map, once per parameter set."""
    key = (role, k, gi, ib, seed)
    if key not in _fm:
        _fm[key] = _render(O, sc.flat_bytes() if k is None else _patched_blob(sc, k), gi, ib, seed, 1)
    return _fm[key]


@pytest.mark.gpu
@pytest.mark.parametrize("gi,ib,seed", FM_COMBOS)
@pytest.mark.parametrize("k", [1, 2])
def test_uniform_group_is_the_patched_blob(gpu, O, dev, k, gi, ib, seed):
    """Every face in group k: the caustic term of a mesh hit is shaded with sub-material k (kd, ks from shade_entry, the glossiness from the
    extended table in GatherToFrames), on photons that bounced off sub-material 0."""
    role = f"F_uniform{k}"
    sc = _attach(O, role, dev)
    fe = _face_end(sc)
    assert len(fe) == 3 and fe[k] == fe[2] == sc.info.n_triangles and fe[k - 1] == 0
    exp = _fm_expected(O, sc, role, k, gi, ib, seed)
    unpatched = _fm_expected(O, sc, role, None, gi, ib, seed)["samples"]
    assert (exp["samples"].view(np.uint32) != unpatched.view(np.uint32)).any(axis=-1).mean() >= 0.05
    opts = _opts(gpu, gi, ib, seed)
    _assert_rays(sc, O, opts)
    gs, st = sc.render_samples(opts, 0, 0, W, H)
    assert st.camera_samples == W * H * SPP and st.photon_queries > 0
    assert same_bits(gs, exp["samples"]), _diff(gs, exp["samples"])
    rgb, rad, _ = sc.render(opts)
    assert same_bits(rad, exp["radiance"]), _diff(rad, exp["radiance"])
    assert np.array_equal(rgb, exp["rgb8"])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
def test_mixed_groups_select_by_first_hit(gpu, O, dev, seed):
    sc = _attach(O, "F", dev)
    opts = _opts(gpu, -1, 0, seed)
    _assert_rays(sc, O, opts)
    g = _groups(O, sc, seed)
    rs = [_fm_expected(O, sc, "F", k, -1, 0, seed)["samples"] for k in range(3)]
    for k in range(3):
        assert (g == k).mean() >= 0.05
        assert same_bits(rs[k][g < 0], rs[0][g < 0])  # off the mesh the patch changes nothing
    exp = rs[0].copy()
    for k in (1, 2):
        exp[g == k] = rs[k][g == k]
    gs, st = sc.render_samples(opts, 0, 0, W, H)
    assert st.camera_samples == W * H * SPP and st.photon_queries > 0
    assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
def test_face_materials_off_is_the_oracles_photon_frame(gpu, O, dev, seed):
    sc = _attach(O, "F_off", dev)
    exp = _fm_expected(O, sc, "F_off", None, 3, 16, seed)["samples"]
    gs, _ = sc.render_samples(_opts(gpu, 3, 16, seed), 0, 0, W, H)
    assert same_bits(gs, exp), _diff(gs, exp)
    on, _ = dev("F")[0].render_samples(_opts(gpu, 3, 16, seed), 0, 0, W, H)  # the same scene and the same map, the switch on
    assert np.array_equal(dev("F")[1], dev("F_off")[1])
    assert (on.view(np.uint32) != exp.view(np.uint32)).any(axis=-1).mean() >= 0.05


# ---------------------------------------------------------------------------------------------------- 4. lens x photon
@pytest.mark.gpu
def test_lens_photon_radiance_equals_the_oracle_at_the_lens_point(gpu, O, dev):
    sc = _attach(O, "L", dev)
    opts = gpu.default_opts(spp=SPP, gi_bounces=L_GI, seed=L_SEED, photon_map=1, photon_exact=1, lens=1)
    _assert_rays(sc, O, opts)
    exp, n = _lens_inputs(O, gpu, sc)
    assert n >= MIN_LIT
    gs, st = sc.render_samples(opts, 0, 0, W, H)
    assert st.photon_queries > 0
    assert same_bits(gs, exp), _diff(gs, exp)
    pin, _ = sc.render_samples(gpu.default_opts(spp=SPP, gi_bounces=L_GI, seed=L_SEED, photon_map=1, photon_exact=1), 0, 0, W, H)
    assert (gs.view(np.uint32) != pin.view(np.uint32)).any(axis=-1).mean() >= 0.5  # the aperture is open


@pytest.mark.gpu
def test_lens_with_a_closed_aperture_is_the_pinhole_photon_render(gpu, O, dev):
    sc = _attach(O, "L_closed", dev)
    assert sc.flat_view().header.camera.dof == 0
    kw = dict(spp=SPP, gi_bounces=L_GI, seed=L_SEED, photon_map=1, photon_exact=1)
    exp = O.render(sc.flat_bytes(), W, H, SPP, gi=L_GI, seed=L_SEED, threads=16, photon=1)
    assert not same_bits(exp["samples"], O.render(sc.flat_bytes(), W, H, SPP, gi=L_GI, seed=L_SEED, threads=16, photon=0)["samples"])
    for lens in (1, 0):
        gs, _ = sc.render_samples(gpu.default_opts(lens=lens, **kw), 0, 0, W, H)
        assert same_bits(gs, exp["samples"]), (lens, _diff(gs, exp["samples"]))
        rgb, rad, _ = sc.render(gpu.default_opts(lens=lens, **kw))
        assert same_bits(rad, exp["radiance"]) and np.array_equal(rgb, exp["rgb8"]), lens


# ---------------------------------------------------------------------------------------------------- 5. all three at once
ALL = dict(spp=SPP, gi_bounces=3, internal_bounces=16, seed=9, photon_map=1, photon_exact=1, lens=1)


@pytest.fixture(scope="module")
def all_on(gpu, dev):
    """F with coloured emitters, face materials, the lens open and the photon map: (scene, samples, rgb8, radiance, stats) of the plain renders."""
    sc, _ = dev("F_all")
    gs, st = sc.render_samples(gpu.default_opts(**ALL), 0, 0, W, H)
    rgb, rad, rst = sc.render(gpu.default_opts(**ALL))
    assert st.passes == rst.passes == 1 and st.photon_queries > 0 and rst.launches_resolve_fused == 1
    for a in (gs, rgb, rad):
        a.setflags(write=False)
    return sc, gs, rgb, rad, st


@pytest.mark.gpu
def test_all_on_every_switch_shows(gpu, all_on):
    """Each of the four is in the frame: switching any one off changes it."""
    sc, gs, _, _, _ = all_on
    for off in (dict(photon_map=0), dict(lens=0)):
        other, _ = sc.render_samples(gpu.default_opts(**{**ALL, **off}), 0, 0, W, H)
        assert (other.view(np.uint32) != gs.view(np.uint32)).any(axis=-1).mean() >= 0.05, off
    for setter in (sc.set_emissive, sc.set_face_materials):
        try:
            setter(False)
            other, _ = sc.render_samples(gpu.default_opts(**ALL), 0, 0, W, H)
        finally:
            setter(True)
        assert (other.view(np.uint32) != gs.view(np.uint32)).any(axis=-1).mean() >= 0.05, setter.__name__
    again, _ = sc.render_samples(gpu.default_opts(**ALL), 0, 0, W, H)
    assert same_bits(again, gs)


@pytest.mark.gpu
def test_all_on_three_passes(gpu, all_on):
    sc, gs, rgb, rad, _ = all_on
    o = gpu.default_opts(samples_per_pass=W * H * SPP // 3 + SPP, **ALL)
    got, st = sc.render_samples(o, 0, 0, W, H)
    assert st.passes >= 3
    assert same_bits(got, gs), _diff(got, gs)
    prgb, prad, pst = sc.render(o)
    assert pst.passes >= 3 and same_bits(prad, rad) and np.array_equal(prgb, rgb)


@pytest.mark.gpu
def test_all_on_pass_that_overflows_and_is_redone_in_halves(gpu, all_on):
    sc, gs, _, _, st = all_on
    try:
        sc.knob("frame_cap", max(1, int(st.shade_calls) // 3))
        got, st2 = sc.render_samples(gpu.default_opts(**ALL), 0, 0, W, H)
    finally:
        sc.knob("frame_cap", 0)
    assert st2.passes >= 3
    assert same_bits(got, gs), _diff(got, gs)


@pytest.mark.gpu
def test_all_on_as_rank_1_of_2(gpu, all_on):
    from bhraytracer_amd import dist
    sc, gs, _, _, _ = all_on
    tile = 8
    own = dist.owned_mask(W, H, tile, 1, 2).numpy().reshape(-1)
    assert 0 < own.sum() < W * H
    got, _ = sc.render_samples(gpu.default_opts(rank=1, world_size=2, tile_size=tile, **ALL), 0, 0, W, H)
    assert same_bits(got[own], gs[own]), _diff(got[own], gs[own])


@pytest.mark.gpu
def test_all_on_resolved_both_ways_and_render_var(gpu, all_on):
    sc, gs, rgb, rad, _ = all_on
    try:
        sc.knob("fused_resolve", 0)
        rgb0, rad0, st0 = sc.render(gpu.default_opts(**ALL))
    finally:
        sc.knob("fused_resolve", 1)
    assert st0.launches_resolve_fused == 0
    assert same_bits(rad0, rad), _diff(rad0, rad)
    assert np.array_equal(rgb0, rgb)
    vrgb, vrad, var = sc.render_var(gpu.default_opts(**ALL))
    assert same_bits(vrad, rad), _diff(vrad, rad)
    assert np.array_equal(vrgb, rgb) and (var > 0).any()
    mean = np.zeros((W * H, 3), np.float32)  # and the frame is the mean of the samples: additions from zero in sample order, one division
    for s in range(SPP):
        mean = mean + gs[:, s, :]
    assert same_bits((mean / np.float32(SPP)).reshape(H, W, 3), rad)


@pytest.mark.gpu
def test_all_on_selection_pass_and_lane_pass(gpu, all_on):
    """gather_lane_budget 1 hands every query's walk to a whole wave; the default leaves them to the lanes: both feed GatherToFrames."""
    sc, gs, _, _, st = all_on
    try:
        sc.knob("gather_lane_budget", 1)
        got, st1 = sc.render_samples(gpu.default_opts(**ALL), 0, 0, W, H)
    finally:
        sc.knob("gather_lane_budget", 0)
    print("wave queries: budget 1", st1.photon_wave_queries, "default", st.photon_wave_queries, "of", st.photon_queries)
    assert st1.photon_queries == st.photon_queries and st1.photon_wave_queries > st.photon_wave_queries and st.photon_wave_queries < st.photon_queries
    assert same_bits(got, gs), _diff(got, gs)


# ---------------------------------------------------------------------------------------------------- 6. the default gather
def _check_default_gather(sc, opts, exp):
    gs, st = sc.render_samples(opts, 0, 0, W, H)
    err = float(np.nanmax(np.abs(gs - exp)))
    print("heavy queries", st.photon_heavy_queries, "of", st.photon_queries, "exact", st.photon_exact_queries, "max |difference|", err)
    assert st.photon_queries > 0
    assert err <= BAR
    assert np.array_equal(np.isnan(gs), np.isnan(exp))
    if st.photon_heavy_queries == 0:
        assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
def test_default_gather_white_body(gpu, O, dev):
    sc = _attach(O, "E", dev)
    gi, ib, seed = 3, 16, 0
    _check_default_gather(sc, _opts(gpu, gi, ib, seed, photon_exact=0), _white_expected(O, sc, gi, ib, seed)["samples"])


@pytest.mark.gpu
def test_default_gather_uniform_group_1(gpu, O, dev):
    sc = _attach(O, "F_uniform1", dev)
    gi, ib, seed = 3, 16, 9
    _check_default_gather(sc, _opts(gpu, gi, ib, seed, photon_exact=0), _fm_expected(O, sc, "F_uniform1", 1, gi, ib, seed)["samples"])
