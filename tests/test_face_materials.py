"""Face materials: with bhrt_scene_set_face_materials on, a hit of a node whose material is a MultiMtl (an OBJ with a .mtl) shades
with the sub-material of the face that was hit, s(prim) = the first i with prim < face_end[i], and sub-material 0 where there is none.

The oracle shades every MultiMtl with its record in the blob (the reference's sub-material 0) and still pins the switch bit for bit: the record is
overwritten, in Python, with the bytes of sub-material k (bhrt_scene_get_submaterial), and
  1. uniform k   an OBJ whose faces all belong to group k renders, at full depth, as the oracle renders the blob patched to k;
  2. mixed       without child frames (gi_bounces = -1, internal_bounces = 0) a sample depends on the material of its first hit only: it is the
                 sample of the oracle's render of the blob patched to the group of the face O.trace_closest finds for its camera ray.
tests/scenes/facemtl_room.xml: the room of the emission tests with one light and the mesh facemtl.obj, three groups.  33 x 17 pixels, spp 3."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import SCENES, same_bits

XML = os.path.join(SCENES, "facemtl_room.xml")
OBJ = os.path.join(SCENES, "facemtl.obj")
MTL = os.path.join(SCENES, "facemtl.mtl")
W, H, SPP = 33, 17, 3
ERR_ARG = "bhrt error 3"  # BHRT_ERR_ARG
COMBOS = [(gi, ib, seed) for gi in (-1, 0, 3) for ib in (0, 16) for seed in (0, 9)]
ONE = (3, 16, 9)  # the combination that also runs the resolves, frame batches, passes, ranks and the var / adaptive entry points


# ---------------------------------------------------------------------------------------------------- scenes
def _obj_uniform(k):
    """All three usemtl names appear, in order (the table has three entries), and every face belongs to group k."""
    lines = [l for l in open(OBJ).read().splitlines() if not l.startswith("usemtl")]
    at = next(i for i, l in enumerate(lines) if l.startswith("mtllib")) + 1
    return "\n".join(lines[:at] + ["usemtl m0", "usemtl m1", "usemtl m2", f"usemtl m{k}"] + lines[at:]) + "\n"


def _obj_m0_faces_first_without_usemtl():
    """The faces of group m0 in front of the first usemtl (no material: the loader files them behind the last group), then m1's, then m2's."""
    head, faces, cur = [], {"m0": [], "m1": [], "m2": []}, None
    for l in open(OBJ).read().splitlines():
        if l.startswith("usemtl"):
            cur = l.split()[1]
        elif l.startswith("f "):
            faces[cur].append(l)
        else:
            head.append(l)
    return "\n".join(head + faces["m0"] + ["usemtl m1"] + faces["m1"] + ["usemtl m2"] + faces["m2"]) + "\n"


def _mtl_identical():
    """Three entries of different names and the same parameters (m1's: a texture and a tight highlight)."""
    body = "Kd 0.9 0.9 0.6\nKs 0.7 0.6 0.5\nNs 80\nillum 2\nmap_Kd tex_small.png\n"
    return "".join(f"newmtl m{i}\n{body}" for i in range(3))


def _xml_with_sphere_of_the_mesh_material():
    """The ball names the mesh's MultiMtl: a hit that is no triangle."""
    t = open(XML).read()
    old = '<object type="sphere" name="ball" material="ball">'
    assert t.count(old) == 1
    return t.replace(old, '<object type="sphere" name="ball" material="facemtl.obj">')


@pytest.fixture(scope="module")
def make_scene(B, tmp_path_factory):
    """Private scene handles (the switch is state of a handle), freed when the module is done.  make_scene() = the committed scene;
    make_scene(tag, obj=..., mtl=..., xml=...) = a variant written to a temporary directory beside copies of the assets: the OBJ text replaces
    facemtl.obj there, the .mtl text facemtl.mtl."""
    root = tmp_path_factory.mktemp("facemtl")
    opened = []

    def _make(tag=None, obj=None, mtl=None, xml=None):
        path = XML
        if tag is not None:
            d = root / tag
            d.mkdir()
            shutil.copy(os.path.join(SCENES, "tex_small.png"), d / "tex_small.png")
            (d / "facemtl.obj").write_text(obj if obj is not None else open(OBJ).read())
            (d / "facemtl.mtl").write_text(mtl if mtl is not None else open(MTL).read())
            (d / "facemtl_room.xml").write_text(xml if xml is not None else open(XML).read())
            path = str(d / "facemtl_room.xml")
        opened.append(B.Scene(path))
        assert opened[-1].warnings() == []
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
    """facemtl_room.xml, uploaded, the switch on."""
    sc = make_scene()
    sc.upload(0)
    sc.set_face_materials(True)
    return sc


@pytest.fixture(scope="module")
def uniform(gpu, make_scene):
    """k -> the variant whose faces all belong to group k, uploaded, the switch on."""
    made = {}

    def _get(k):
        if k not in made:
            sc = make_scene(f"uniform{k}", obj=_obj_uniform(k))
            sc.set_face_materials(True)  # before the upload: the upload carries the switch
            sc.upload(0)
            made[k] = sc
        return made[k]
    return _get


def _multi(sc):
    """The index of the scene's MultiMtl."""
    (mm,) = [m for m in range(sc.info.n_materials) if sc.submaterial_count(m) > 0]
    return mm


def _face_end(sc):
    mm = _multi(sc)
    return np.array([sc.submaterial(mm, k)[1] for k in range(sc.submaterial_count(mm))], np.int64)


def _patched_blob(sc, k):
    """The scene's flat blob with the MultiMtl's record overwritten with the bytes of its sub-material k."""
    from bhraytracer_amd import flat
    mm = _multi(sc)
    off = sc.flat_view().header.off_materials + mm * C.sizeof(flat.Material)
    b = bytearray(sc.flat_bytes())
    b[off:off + C.sizeof(flat.Material)] = bytes(sc.submaterial(mm, k)[0])
    return bytes(b)


_renders = {}


def _oracle(O, sc, k, gi, ib, seed):
    """The oracle's render of sc's blob patched to sub-material k (None: unpatched), once per parameter set, shared and never written to."""
    key = (id(sc), k, gi, ib, seed)
    if key not in _renders:
        r = O.render(sc.flat_bytes() if k is None else _patched_blob(sc, k), W, H, SPP, gi=gi, bounces=ib, seed=seed, threads=16)
        for a in (r["samples"], r["radiance"], r["rgb8"]):
            a.setflags(write=False)
        _renders[key] = r
    return _renders[key]


def _differs(a, b):
    """The share of samples that differ in some bit."""
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).mean()


def _first_hit_group(gpu, O, sc, opts):
    """(pixels, spp): the group of the face of every camera sample's first hit — s(prim) with the fallback to 0 — and -1 where the first hit is
    not on a node of the MultiMtl; and the same array without the fallback (len(face_end) where GetMaterialIndex returns -1)."""
    o, d = sc.camera_rays(opts)
    h = O.trace_closest(sc.flat_bytes(), o.reshape(-1, 3), d.reshape(-1, 3), gpu.SIDE_FRONT)
    node_mtl = np.array([n.material for n in sc.flat_view().nodes] + [-1], np.int32)  # [-1]: a miss
    fe = _face_end(sc)
    raw = np.searchsorted(fe, h["prim"], side="right")  # the first i with prim < face_end[i]
    raw[h["prim"] < 0] = len(fe)
    g = np.where(raw < len(fe), raw, 0)
    on = node_mtl[h["node"]] == _multi(sc)
    shape = (o.shape[0], o.shape[1])
    return np.where(on, g, -1).reshape(shape), np.where(on, raw, -1).reshape(shape)


def _diff(a, b):
    bad = np.argwhere(np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32))
    return f"{len(bad)} of {a.size} values differ, first at {bad[:6].tolist()}"


def _assert_inputs(groups, n_groups=3):
    """The conditions on the inputs: a case cannot pass empty."""
    for k in range(n_groups):
        assert (groups == k).mean() >= 0.05, (k, (groups == k).mean())
    assert (groups < 0).mean() >= 0.20, (groups < 0).mean()


# ---------------------------------------------------------------------------------------------------- 1. uniform k, full depth
@pytest.mark.gpu
@pytest.mark.parametrize("gi,ib,seed", COMBOS)
@pytest.mark.parametrize("k", [1, 2])
def test_uniform_group_is_the_patched_blob(gpu, O, uniform, k, gi, ib, seed):
    sc = uniform(k)
    fe = _face_end(sc)
    assert len(fe) == 3 and fe[k] == fe[2] == sc.info.n_triangles and (k == 0 or fe[k - 1] == 0)  # three entries, every face in group k
    exp = _oracle(O, sc, k, gi, ib, seed)
    assert _differs(exp["samples"], _oracle(O, sc, None, gi, ib, seed)["samples"]) >= 0.05
    opts = gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed)
    gs, st = sc.render_samples(opts, 0, 0, W, H)
    assert st.camera_samples == W * H * SPP
    assert same_bits(gs, exp["samples"]), _diff(gs, exp["samples"])
    rgb, rad, _ = sc.render(opts)
    assert same_bits(rad, exp["radiance"]), _diff(rad, exp["radiance"])
    assert np.array_equal(rgb, exp["rgb8"])


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("k", [1, 2])
def test_uniform_group_resolved_frame_both_ways(gpu, O, uniform, k, fused):
    """The root frames resolved straight into the image (k_resolve_frames) and through the sample buffer."""
    gi, ib, seed = ONE
    sc = uniform(k)
    exp = _oracle(O, sc, k, gi, ib, seed)
    try:
        sc.knob("fused_resolve", fused)
        rgb, rad, st = sc.render(gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed))
    finally:
        sc.knob("fused_resolve", 1)
    assert st.launches_resolve_fused == (st.passes if fused else 0)
    assert same_bits(rad, exp["radiance"]), _diff(rad, exp["radiance"])
    assert np.array_equal(rgb, exp["rgb8"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_uniform_group_over_frame_batches_and_passes(gpu, O, uniform, k):
    gi, ib, seed = ONE
    sc = uniform(k)
    exp = _oracle(O, sc, k, gi, ib, seed)["samples"]
    opts = gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed)
    _, st = sc.render_samples(opts, 0, 0, W, H)
    assert st.passes == 1
    try:  # a frame pool of a third of what the frame needs: passes overflow and are redone in halves
        sc.knob("frame_cap", max(1, int(st.shade_calls) // 3))
        gs, st2 = sc.render_samples(opts, 0, 0, W, H)
    finally:
        sc.knob("frame_cap", 0)
    assert st2.passes >= 3
    assert same_bits(gs, exp), _diff(gs, exp)
    gs, st3 = sc.render_samples(gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed, samples_per_pass=W * H * SPP // 2), 0, 0, W, H)
    assert st3.passes >= 2
    assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_uniform_group_as_rank_1_of_2(gpu, O, uniform, k):
    from bhraytracer_amd import dist
    gi, ib, seed = ONE
    tile = 8
    sc = uniform(k)
    exp = _oracle(O, sc, k, gi, ib, seed)["samples"]
    own = dist.owned_mask(W, H, tile, 1, 2).numpy().reshape(-1)
    assert 0 < own.sum() < W * H
    gs, _ = sc.render_samples(gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed, rank=1, world_size=2, tile_size=tile), 0, 0, W, H)
    assert same_bits(gs[own], exp[own]), _diff(gs[own], exp[own])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_uniform_group_through_var_and_adaptive(gpu, O, uniform, k):
    """bhrt_render_var, and bhrt_render_adaptive with a threshold < 0 (no pixel retires: every pixel gets opts.spp samples)."""
    gi, ib, seed = ONE
    sc = uniform(k)
    exp = _oracle(O, sc, k, gi, ib, seed)
    opts = gpu.default_opts(spp=SPP, gi_bounces=gi, internal_bounces=ib, seed=seed)
    vrgb, vrad, var = sc.render_var(opts)
    assert same_bits(vrad, exp["radiance"]), _diff(vrad, exp["radiance"])
    assert np.array_equal(vrgb, exp["rgb8"]) and (var > 0).any()
    argb, arad, _, cnt, st = sc.render_adaptive(opts, gpu.default_adaptive_opts(min_spp=2, threshold=-1.0))
    assert (cnt == SPP).all() and st.camera_samples == W * H * SPP
    assert same_bits(arad, exp["radiance"]), _diff(arad, exp["radiance"])
    assert np.array_equal(argb, exp["rgb8"])


# ---------------------------------------------------------------------------------------------------- 2. mixed, first-hit selection
def _selected(O, sc, groups, seed, n_groups):
    """Every sample taken from the oracle's render of the blob patched to the group of its first hit; samples that do not hit the mesh first
    are the same in all of them."""
    rs = [_oracle(O, sc, k, -1, 0, seed)["samples"] for k in range(n_groups)]
    off_mesh = groups < 0
    for r in rs[1:]:
        assert same_bits(r[off_mesh], rs[0][off_mesh])
        assert _differs(r, _oracle(O, sc, None, -1, 0, seed)["samples"]) >= 0.05
    exp = rs[0].copy()
    for k in range(1, n_groups):
        exp[groups == k] = rs[k][groups == k]
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
def test_mixed_groups_select_by_first_hit(gpu, O, room, seed):
    opts = gpu.default_opts(spp=SPP, gi_bounces=-1, internal_bounces=0, seed=seed)
    groups, raw = _first_hit_group(gpu, O, room, opts)
    _assert_inputs(groups)
    assert (raw < 3).all()  # every face of the committed mesh has a group
    exp = _selected(O, room, groups, seed, 3)
    gs, st = room.render_samples(opts, 0, 0, W, H)
    assert st.camera_samples == W * H * SPP
    assert same_bits(gs, exp), _diff(gs, exp)  # every sample of the frame


# ---------------------------------------------------------------------------------------------------- 3. identical sub-materials
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
def test_identical_submaterials_change_nothing(gpu, O, make_scene, seed):
    sc = make_scene(f"identical{seed}", mtl=_mtl_identical())
    mm = _multi(sc)
    recs = [sc.submaterial(mm, k)[0] for k in range(3)]
    assert sc.submaterial_count(mm) == 3 and recs[0].diffuse.map == 0
    for r in recs[1:]:  # the same parameters; each its own texture map, of the same texture
        assert r.diffuse.map > 0 and bytes(r)[:16] == bytes(recs[0])[:16] and bytes(r)[20:] == bytes(recs[0])[20:]
    sc.upload(0)
    opts = gpu.default_opts(spp=SPP, gi_bounces=3, internal_bounces=16, seed=seed)
    exp = O.render(sc.flat_bytes(), W, H, SPP, gi=3, bounces=16, seed=seed, threads=16)["samples"]
    off, _ = sc.render_samples(opts, 0, 0, W, H)
    sc.set_face_materials(True)
    on, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(off, exp), _diff(off, exp)
    assert same_bits(on, exp), _diff(on, exp)


# ---------------------------------------------------------------------------------------------------- 4. off is off
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 9])
def test_off_is_the_oracle_frame(gpu, O, make_scene, room, seed):
    sc = make_scene()
    sc.upload(0)
    opts = gpu.default_opts(spp=SPP, gi_bounces=3, internal_bounces=16, seed=seed)
    exp = _oracle(O, room, None, 3, 16, seed)["samples"]  # the same XML: the same blob
    assert sc.flat_bytes() == room.flat_bytes()
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(gs, exp), _diff(gs, exp)
    sc.set_face_materials(True)
    on, _ = sc.render_samples(opts, 0, 0, W, H)
    assert _differs(on, exp) >= 0.05  # the switch does something here
    sc.set_face_materials(False)  # on and off again: off
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
def test_scene_without_multimtl_renders_the_same_bits(gpu, B):
    sc = B.Scene(os.path.join(SCENES, "c3_mesh_small.xml"))
    try:
        assert all(sc.submaterial_count(m) == 0 for m in range(sc.info.n_materials))
        sc.upload(0)
        opts = gpu.default_opts(spp=2, gi_bounces=3, seed=9)
        region = (96, 64, 160, 112)
        off, _ = sc.render_samples(opts, *region)
        z0, n0, a0 = sc.first_hit()
        sc.set_face_materials(True)
        on, _ = sc.render_samples(opts, *region)
        z1, n1, a1 = sc.first_hit()
        assert same_bits(on, off) and (off != 0).any()
        assert same_bits(z0, z1) and same_bits(n0, n1) and same_bits(a0, a1)
    finally:
        sc.close()


@pytest.mark.gpu
def test_clone_carries_switch_and_table(gpu, room, make_scene):
    opts = gpu.default_opts(spp=SPP, gi_bounces=3, seed=0)
    src = make_scene()
    src.set_face_materials(True)
    cl = src.clone()
    try:
        mm = _multi(src)
        assert cl.flat_bytes() == src.flat_bytes() and cl.submaterial_count(mm) == 3
        for k in range(3):
            a, b = src.submaterial(mm, k), cl.submaterial(mm, k)
            assert bytes(a[0]) == bytes(b[0]) and a[1] == b[1]
        got, _ = cl.render_samples(opts, 0, 0, W, H)  # uploads the clone: the switch came with it
        exp, _ = room.render_samples(opts, 0, 0, W, H)
        assert same_bits(got, exp), _diff(got, exp)
        src.set_face_materials(False)  # the clone has a state of its own
        off, _ = src.render_samples(opts, 0, 0, W, H)
        again, _ = cl.render_samples(opts, 0, 0, W, H)
        assert same_bits(again, exp) and not same_bits(off, exp)
    finally:
        cl.close()


# ---------------------------------------------------------------------------------------------------- 5. first-hit albedo
@pytest.mark.gpu
def test_first_hit_albedo_is_the_faces_submaterial(gpu, O, room, make_scene):
    fv = room.flat_view()
    po, pd = O.primary_rays(fv)
    h = O.trace_closest(room.flat_bytes(), po, pd, gpu.SIDE_FRONT)
    node_mtl = np.array([n.material for n in fv.nodes] + [-1], np.int32)
    fe = _face_end(room)
    g = np.searchsorted(fe, h["prim"], side="right")
    assert (g[node_mtl[h["node"]] == _multi(room)] < 3).all()
    g = np.where(node_mtl[h["node"]] == _multi(room), g, 0)  # off the mesh: the same in every patched blob
    for k in range(3):
        assert ((g == k) & (node_mtl[h["node"]] == _multi(room))).mean() >= 0.05
    per_k = [O.first_hit(_patched_blob(room, k), W, H) for k in range(3)]
    exp = per_k[0][2].copy()
    for k in (1, 2):
        exp[g == k] = per_k[k][2][g == k]
    assert len(np.unique(exp[g == 1], axis=0)) >= 2  # m1's texture varies over its faces
    z, nrm, alb = room.first_hit()
    assert same_bits(alb.reshape(-1, 3), exp), _diff(alb.reshape(-1, 3), exp)
    assert not same_bits(exp, per_k[0][2])
    off = make_scene()
    off.upload(0)
    z0, n0, a0 = off.first_hit()  # the switch off: sub-material 0 everywhere, z and normal the same either way
    assert same_bits(a0.reshape(-1, 3), per_k[0][2])
    assert same_bits(z, z0) and same_bits(nrm, n0)
    assert same_bits(z.reshape(-1), per_k[0][0]) and same_bits(nrm.reshape(-1, 3), per_k[0][1])


# ---------------------------------------------------------------------------------------------------- 6. the fallback rule
@pytest.mark.gpu
def test_faces_in_front_of_any_usemtl_shade_as_submaterial_0(gpu, O, make_scene):
    sc = make_scene("no_usemtl", obj=_obj_m0_faces_first_without_usemtl())
    fe = _face_end(sc)
    assert len(fe) == 2 and 0 < fe[0] < fe[1] < sc.info.n_triangles  # two groups (m1, m2); the faces behind them have none
    sc.set_face_materials(True)
    sc.upload(0)
    seed = 9
    opts = gpu.default_opts(spp=SPP, gi_bounces=-1, internal_bounces=0, seed=seed)
    groups, raw = _first_hit_group(gpu, O, sc, opts)
    assert (raw == 2).mean() >= 0.05 and (groups[raw == 2] == 0).all()  # hits of faces without a group: they shade as sub-material 0
    _assert_inputs(groups, 2)
    exp = _selected(O, sc, groups, seed, 2)
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(gs, exp), _diff(gs, exp)


@pytest.mark.gpu
def test_sphere_of_the_mesh_material_shades_as_submaterial_0(gpu, O, make_scene):
    sc = make_scene("sphere", xml=_xml_with_sphere_of_the_mesh_material())
    sc.set_face_materials(True)
    sc.upload(0)
    seed = 0
    opts = gpu.default_opts(spp=SPP, gi_bounces=-1, internal_bounces=0, seed=seed)
    o, d = sc.camera_rays(opts)
    h = O.trace_closest(sc.flat_bytes(), o.reshape(-1, 3), d.reshape(-1, 3), gpu.SIDE_FRONT)
    nodes = sc.flat_view().nodes
    (ball,) = [i for i, n in enumerate(nodes) if n.material == _multi(sc) and n.mesh < 0]
    on_ball = (h["node"] == ball).reshape(o.shape[0], o.shape[1])
    assert on_ball.sum() > 0 and (h["prim"][h["node"] == ball] < 0).all()
    groups, _ = _first_hit_group(gpu, O, sc, opts)
    assert (groups[on_ball] == 0).all()  # prim = -1: the fallback
    _assert_inputs(groups)
    exp = _selected(O, sc, groups, seed, 3)
    gs, _ = sc.render_samples(opts, 0, 0, W, H)
    assert same_bits(gs, exp), _diff(gs, exp)


# ---------------------------------------------------------------------------------------------------- 7. the loader and the API (no GPU)
def _mtl_entries(text):
    out, cur = [], None
    for l in text.splitlines():
        t = l.split()
        if not t or t[0].startswith("#"):
            continue
        if t[0] == "newmtl":
            cur = {"name": t[1]}
            out.append(cur)
        else:
            cur[t[0]] = t[1:]
    return out


def test_submaterials_are_the_mtl_file(B):
    sc = B.Scene(XML)
    try:
        assert sc.warnings() == []
        mm = sc.material_index("facemtl.obj")
        assert [sc.submaterial_count(m) for m in range(sc.info.n_materials)] == [3 if m == mm else 0 for m in range(sc.info.n_materials)]
        ent = _mtl_entries(open(MTL).read())
        assert [e["name"] for e in ent] == ["m0", "m1", "m2"]  # and the OBJ meets them in this order
        f32 = lambda v: [float(np.float32(x)) for x in v]
        ends = []
        for k, e in enumerate(ent):
            m, end = sc.submaterial(mm, k)
            ends.append(end)
            assert m.kind == 0  # BHRT_MTL_BLINN
            assert list(m.diffuse.color) == f32(e["Kd"]) and list(m.specular.color) == f32(e["Ks"])
            assert m.glossiness == float(np.float32(e["Ns"][0])) and m.ior == float(np.float32(e.get("Ni", ["1"])[0]))
            assert (m.diffuse.map >= 0) == ("map_Kd" in e) and m.specular.map == -1 and m.refraction.map == -1
            if int(e["illum"][0]) >= 6:  # refraction colour 1 - Tf; the glossiness is the reference's acos(pow(2, 1 / Ns)), not a number
                assert list(m.refraction.color) == [float(np.float32(1) - np.float32(x)) for x in e["Tf"]]
                assert np.isnan(m.refraction_glossiness)
            else:
                assert list(m.refraction.color) == [0, 0, 0] and m.refraction_glossiness == 0
            assert list(m.absorption) == [0, 0, 0]
        assert ends == sorted(ends) and ends[0] > 0 and ends[-1] <= sc.info.n_triangles
        assert ends == [96, 192, 288]
        fv = sc.flat_view()
        assert bytes(sc.submaterial(mm, 0)[0]) == bytes(fv.materials[mm])  # sub-material 0 is the blob's record
        tm = sc.submaterial(mm, 1)[0].diffuse.map
        assert fv.header.n_texmaps == 1 and tm == 0 and fv.textures[fv.texmaps[tm].texture].width > 0  # pushed as before, now its index is kept
    finally:
        sc.close()


def test_api_errors_and_null_outputs(B):
    from bhraytracer_amd import flat
    sc = B.Scene(XML)
    try:
        mm, n = sc.material_index("facemtl.obj"), sc.info.n_materials
        for bad in (-1, n, 1 << 20):
            with pytest.raises(B.BhrtError, match=ERR_ARG):
                sc.submaterial_count(bad)
            with pytest.raises(B.BhrtError, match=ERR_ARG):
                sc.submaterial(bad, 0)
        for bad in (-1, 3, 1 << 20):
            with pytest.raises(B.BhrtError, match=ERR_ARG):
                sc.submaterial(mm, bad)
        with pytest.raises(B.BhrtError, match=ERR_ARG):
            sc.submaterial(sc.material_index("wall"), 0)  # a Blinn material has none
        assert B.lib().bhrt_scene_get_submaterial(sc._h, mm, 1, None, None) == 0  # either output may be NULL
        m, e = flat.Material(), C.c_uint32(0)
        assert B.lib().bhrt_scene_get_submaterial(sc._h, mm, 1, C.byref(m), None) == 0 and m.glossiness == 80
        assert B.lib().bhrt_scene_get_submaterial(sc._h, mm, 1, None, C.byref(e)) == 0 and e.value == 192
        assert B.lib().bhrt_scene_submaterial_count(sc._h, mm, None) != 0
        assert B.lib().bhrt_scene_set_face_materials(None, 1) != 0
    finally:
        sc.close()


def test_flat_blob_and_info_keep_their_values_and_no_call_needs_a_device(B):
    """Every call of the feature on a scene that is never uploaded: this test runs where there is no device."""
    assert C.sizeof(B.Opts) == 64
    sc = B.Scene(XML)
    try:
        before, n = sc.flat_bytes(), sc.info.n_materials
        mm = sc.material_index("facemtl.obj")
        calls = [lambda: sc.set_face_materials(True), lambda: sc.submaterial_count(mm), lambda: sc.submaterial(mm, 2), lambda: sc.set_face_materials(False),
                 lambda: sc.set_face_materials(True)]
        for call in calls:
            call()
            sc._flat = None
            assert sc.flat_bytes() == before
        cl = sc.clone()
        try:
            assert cl.flat_bytes() == before and cl.info.n_materials == n and cl.submaterial(mm, 2)[1] == 288
        finally:
            cl.close()
    finally:
        sc.close()
