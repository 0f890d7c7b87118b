"""The oracle and the front-end against the unmodified reference (oracle/_ref/ref_harness[_pm]).  The reference's outputs were recorded
by tests/golden/make_ref_parity.py into tests/golden/ref_parity*.npz, on inputs that are committed as well (the scenes under tests/scenes,
the reference's shipped XMLs and their textures under tests/golden/shipped, the XML text of every random scene), so these tests need
nothing outside the repository."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, SCENES, same_bits

SHIPPED_ROOT = os.path.join(GOLDEN, "shipped")  # the reference resolves asset paths against its working directory: Resource/...


@pytest.fixture(scope="module")
def ref():
    """The reference's recorded outputs, by name (tests/golden/make_ref_parity.py)."""
    out = {}
    for name in ("ref_parity", "ref_parity_render"):
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _key(rel):
    return rel.replace("/", "__").replace(".xml", "")


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_scene_dump_matches_front_end(B, ref):
    # transforms, camera frame, light order, meshes and the BVH: bit for bit
    sc = B.Scene(os.path.join(SCENES, "c4_textured.xml"))
    fv = sc.flat_view()
    d = lambda ext: ref["dump_c4_textured_" + ext]
    nf = d("nodes_f32").reshape(-1, 21)
    mine = np.array([list(n.xf.tm) + list(n.xf.pos) + list(n.xf.itm) for n in fv.nodes], np.float32).view(np.uint32)
    assert np.array_equal(nf, mine)
    ni = d("nodes_i32").reshape(-1, 5)
    assert np.array_equal(ni, np.array([[n.parent, n.depth, n.obj_type, n.mesh, n.material] for n in fv.nodes], np.int32))
    m = fv.mesh_arrays(0)
    assert np.array_equal(d("mesh0_bvh_u32"), m["bvh_data"])
    assert np.array_equal(d("mesh0_bvh_f32").reshape(-1, 6)[1:], m["bvh_bounds"].view(np.uint32)[1:])
    assert np.array_equal(d("mesh0_elems_u32"), m["elems"])
    assert np.array_equal(d("mesh0_vn_f32"), m["vn"].view(np.uint32).ravel())
    lf = d("lights_f32")
    assert [int(t) for t in lf[:-1].reshape(-1, 8)[:, 0]] == [l.type for l in fv.lights]     # CalculateLightsIntensity sort
    assert lf[-1] == np.float32(fv.header.all_light_intensity)


def _shipped_xmls():
    return sorted(os.path.relpath(f, SHIPPED_ROOT) for f in glob.glob(os.path.join(SHIPPED_ROOT, "Resource", "**", "*.xml"), recursive=True))


def test_all_19_shipped_scenes_are_committed():
    assert len(_shipped_xmls()) == 19


@pytest.mark.parametrize("rel", _shipped_xmls())
def test_front_end_dump_of_every_shipped_scene(rel, B, ref):
    """xmlload's result on all 19 shipped XMLs (scene graph, transforms, camera frame, sorted lights,
    materials) equals the front-end's flat scene bit for bit.  Meshes are absent from the reference checkout, so their
    nodes are null objects on both sides."""
    d = lambda ext: ref[f"dump_{_key(rel)}_{ext}"]
    cwd = os.getcwd()
    os.chdir(SHIPPED_ROOT)
    try:
        fv = B.Scene(rel).flat_view()
    finally:
        os.chdir(cwd)
    u32 = lambda a: np.asarray(a, np.float32).view(np.uint32)
    nf = d("nodes_f32").reshape(-1, 21)
    assert np.array_equal(nf, u32([list(n.xf.tm) + list(n.xf.pos) + list(n.xf.itm) for n in fv.nodes]).reshape(-1, 21))
    ni = d("nodes_i32").reshape(-1, 5)
    assert np.array_equal(ni, np.array([[n.parent, n.depth, n.obj_type, n.mesh, n.material] for n in fv.nodes], np.int32).reshape(-1, 5))
    c = fv.header.camera
    cam = list(c.pos) + list(c.dir) + list(c.up) + [c.fov, c.focaldist, c.width, c.height] + list(c.top_left) + list(c.dd_x) + list(c.dd_y)
    assert np.array_equal(d("camera_f32"), u32(cam))
    lights = []
    for l in fv.lights:
        lights += [l.type] + list(l.intensity) + (list(l.vec) if l.type else [0, 0, 0]) + [l.size if l.type == 2 else 0]
    lights.append(fv.header.all_light_intensity)
    assert np.array_equal(d("lights_f32"), u32(lights))
    mf = d("materials_f32").reshape(-1, 26)
    assert len(mf) == len(fv.materials)
    for row, m in zip(mf, fv.materials):
        if m.kind != 0:
            assert (row == -1).all()            # MultiMtl
            continue
        mine = []
        for tc in (m.diffuse, m.specular, m.refraction):
            mine += list(tc.color) + [1.0 if tc.map >= 0 else 0.0]
        assert np.array_equal(u32(row[:12]), u32(mine))   # row[12:20]: reflection / emission, parsed but never used by Shade (Q8)
        assert np.array_equal(u32(row[20:]), u32([m.glossiness] + list(m.absorption) + [m.ior, m.refraction_glossiness]))


SHIPPED = ["proj12_backfaceTest", "proj3", "proj13", "proj7", "proj10", "proj2"]


@pytest.mark.parametrize("name", SHIPPED)
def test_integrator_on_shipped_scenes(name, B, O, ref):
    """MtlBlinn::Shade through GI depth 3 on the reference's own scene files (meshes absent -> null objects; its two textures at 256x256)."""
    xml = os.path.join("Resource", "Data", name + ".xml")
    region = (330, 260, 430, 330)
    spp = 2
    cwd = os.getcwd()
    os.chdir(SHIPPED_ROOT)
    try:
        sc = B.Scene(xml)
    finally:
        os.chdir(cwd)
    r = O.render(sc.flat_bytes(), sc.width, sc.height, spp, gi=3, rng=O.RNG_SEQUENTIAL, math=O.MATH_LIBM, region=region, threads=4)
    npx = (region[2] - region[0]) * (region[3] - region[1])
    assert same_bits(r["samples"], ref[f"render_{name}_samples"].reshape(npx, spp, 3))
    assert np.array_equal(r["rgb8"].reshape(-1, 3), ref[f"render_{name}_rgb8"].reshape(npx, 3))


def test_large_mesh_primary_hits(B, O, ref):
    """BASELINE config 3 geometry (100,352 triangles): BVH node-for-node and every primary hit bit-exact."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_mesh
    mesh = os.path.join(SCENES, "gen", "mesh_224.obj")
    if not os.path.exists(mesh):
        gen_mesh.generate(mesh, 224)
    txt = open(os.path.join(SCENES, "c3_mesh.xml")).read().replace('<width value="1920"/>', '<width value="480"/>').replace('<height value="1080"/>', '<height value="270"/>')
    xml = os.path.join(SCENES, "_tmp_c3_480.xml")
    open(xml, "w").write(txt)
    try:
        sc = B.Scene(xml)
    finally:
        os.remove(xml)
    m = sc.flat_view().mesh_arrays(0)
    assert m["f"].shape[0] == 100352
    assert _sha(np.ascontiguousarray(m["bvh_data"], np.uint32)) == str(ref["mesh480_bvh_u32_sha"])
    o, d = O.primary_rays(sc.flat_view())
    r = O.trace_closest(sc.flat_bytes(), o, d, 1)
    assert np.array_equal(ref["mesh480_primary_node"], r["node"])
    hit = r["node"] >= 0
    attrs = np.ascontiguousarray(r["attrs"][hit][:, :9], np.float32)
    assert not np.isnan(attrs).any() and _sha(attrs) == str(ref["mesh480_hit_attrs_sha"])   # the reference's hit attributes, bit for bit


def test_random_scenes_reference_vs_oracle(B, O, ref, tmp_path):
    """tools/fuzz_ref.py on fixed seeds: random scene graphs rendered by the unmodified reference (sequential stream
    through the interposed rand()) and by the oracle in sequential / libm mode, per-sample radiance and RGB8 bit for bit.
    (360 further seeds were run by hand when this was added: all identical.)  The XML of each seed is the one the reference rendered."""
    import shutil
    shutil.copy(os.path.join(SCENES, "mesh_small.obj"), tmp_path / "mesh_small.obj")
    for seed in range(301, 313):
        xml = f"fuzz_{seed}.xml"
        (tmp_path / xml).write_text(str(ref[f"fuzz_{seed}_xml"]))
        gi = int(ref[f"fuzz_{seed}_gi"])
        cwd = os.getcwd()
        os.chdir(tmp_path)
        try:
            sc = B.Scene(xml)
        finally:
            os.chdir(cwd)
        o = O.render(sc.flat_bytes(), sc.width, sc.height, 2, gi=gi, seed=seed, rng=O.RNG_SEQUENTIAL, math=O.MATH_LIBM, region=(0, 0, 96, 72), threads=4)
        samples = np.ascontiguousarray(o["samples"], np.float32)
        assert samples.shape == (96 * 72, 2, 3) and _sha(samples) == str(ref[f"fuzz_{seed}_samples_sha"]), seed   # bit for bit
        assert np.array_equal(o["rgb8"].reshape(-1, 3), ref[f"fuzz_{seed}_rgb8"].reshape(-1, 3)), seed


def test_random_scenes_photon_map_reference_vs_oracle(B, O, ref, tmp_path):
    """BuildCausticPhotonMap + PrepareForIrradianceEstimation of the unmodified reference (oracle/_ref/ref_harness_pm) on
    seeded random scenes that have a caustic path: emitted and balanced photon bytes and the emission count equal the
    oracle's (sequential / libm mode).  (34 such scenes were run by hand; scenes without a caustic path never leave the
    reference's emission loop.)"""
    import shutil
    shutil.copy(os.path.join(SCENES, "mesh_small.obj"), tmp_path / "mesh_small.obj")
    for seed in (11, 14, 31, 40):
        xml = f"f{seed}.xml"
        (tmp_path / xml).write_text(str(ref[f"pfuzz_{seed}_xml"]))
        p = lambda what: ref[f"pfuzz_{seed}_{what}"]
        cwd = os.getcwd()
        os.chdir(tmp_path)
        try:
            sc = B.Scene(xml)
        finally:
            os.chdir(cwd)
        bal, emitted, n_emit = O.photon_build(sc.flat_bytes(), 1500, seed=seed, rng=O.RNG_SEQUENTIAL, math=O.MATH_LIBM)
        meta = p("photons_meta")
        assert n_emit == int(meta[1]), seed
        ref_em, ref_bal = p("photons_emitted"), p("photons_balanced")
        m = np.ones(24, bool)
        m[19] = False   # byte 19 = planeAndDirZ: bit 3 always defined, the split-plane bits only for internal nodes (uninitialised elsewhere)
        assert np.array_equal(emitted[:, m], ref_em[:, m]) and np.array_equal(emitted[:, 19] & 8, ref_em[:, 19] & 8), seed
        assert np.array_equal(bal[:, m], ref_bal[:, m]) and np.array_equal(bal[:, 19] & 8, ref_bal[:, 19] & 8), seed
        internal = np.arange(1, len(ref_bal) + 1) < int(meta[3])
        assert np.array_equal(bal[internal, 19] & 3, ref_bal[internal, 19] & 3), seed
        # the global map (BuildPhotonMap) of the same scene
        bal, emitted, n_emit = O.photon_build_global(sc.flat_bytes(), 1200, seed=seed, rng=O.RNG_SEQUENTIAL, math=O.MATH_LIBM)
        meta = p("gphotons_meta")
        assert n_emit == int(meta[1]), seed
        ref_em, ref_bal = p("gphotons_emitted"), p("gphotons_balanced")
        assert np.array_equal(emitted[:, m], ref_em[:, m]) and np.array_equal(emitted[:, 19] & 8, ref_em[:, 19] & 8), seed
        assert np.array_equal(bal[:, m], ref_bal[:, m]) and np.array_equal(bal[:, 19] & 8, ref_bal[:, 19] & 8), seed
