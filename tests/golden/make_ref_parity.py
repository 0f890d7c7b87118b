#!/usr/bin/env python3
"""Records what tests/test_ref_parity.py, test_front_end.py and test_sanitize.py compare against, so that they run on a checkout alone.

Inputs (committed as fixtures):
  shipped/Resource/...   the reference's 19 shipped scene XMLs, unchanged, and the two textures they use (Data/bricks.png, Data/clouds.png)
                         scaled to 256x256 so that each stays a small file; the meshes are absent, as in the reference's own checkout
Expected outputs (ref_parity.npz), all from the UNMODIFIED reference (oracle/_ref/ref_harness[_pm], built by oracle/Makefile) run on
exactly those inputs:
  dump_c4_textured_*     `dump` of tests/scenes/c4_textured.xml: node transforms, node ints, mesh 0 BVH / elements / normals, lights
  dump_<scene>_*         `dump` of every shipped XML: nodes, camera frame, sorted lights, materials
  render_<scene>_*       (ref_parity_render.npz: each file stays under 1 MiB) `render` of six shipped scenes over the region (330, 260)-(430, 330), 2 spp, GI depth 3: samples and RGB8
  mesh480_*              `dump primary` of tests/scenes/c3_mesh.xml at 480x270 (100,352 triangles): SHA-256 of the BVH and of the hit
                         attributes, the node index of every primary hit
  fuzz_<seed>_*          tools/fuzz_parity.random_scene for seeds 301..312 (the XML text is stored): SHA-256 of the per-sample radiance, RGB8
  pfuzz_<seed>_*         the -DUSE_PhotonMap build on seeds 11, 14, 31, 40: caustic and global photon maps (meta, emitted, balanced)

Runs where a checkout of the reference and oracle/_ref exist:  python tests/golden/make_ref_parity.py <reference>/BHRayTracer
"""
import glob
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SCENES = os.path.join(ROOT, "tests", "scenes")
SHIPPED = os.path.join(HERE, "shipped")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
TEXTURES = ["Resource/Data/bricks.png", "Resource/Data/clouds.png"]
TEXTURE_SIZE = 256
INTEGRATOR_SCENES = ["proj12_backfaceTest", "proj3", "proj13", "proj7", "proj10", "proj2"]
INTEGRATOR_REGION = (330, 260, 430, 330)
FUZZ_SEEDS = range(301, 313)
PHOTON_SEEDS = (11, 14, 31, 40)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def key(rel):
    return rel.replace("/", "__").replace(".xml", "")


def run(harness, scene, prefix, *args, cwd):
    subprocess.run([harness, scene, prefix, *map(str, args)], cwd=cwd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                   timeout=600)


def shipped_inputs(reference):
    from PIL import Image
    shutil.rmtree(SHIPPED, ignore_errors=True)
    for src in sorted(glob.glob(os.path.join(reference, "Resource", "**", "*.xml"), recursive=True)):
        dst = os.path.join(SHIPPED, os.path.relpath(src, reference))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(src, dst)
    for rel in TEXTURES:
        im = Image.open(os.path.join(reference, rel)).convert("RGB").resize((TEXTURE_SIZE, TEXTURE_SIZE), Image.LANCZOS)
        im.save(os.path.join(SHIPPED, rel), optimize=True)


def main():
    reference = sys.argv[1] if len(sys.argv) > 1 else ""
    if not (os.path.exists(HARNESS) and os.path.isfile(os.path.join(reference, "Main.cpp"))):
        sys.exit("usage: make_ref_parity.py <reference>/BHRayTracer  (needs oracle/_ref/ref_harness: make -C oracle ref)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity
    shipped_inputs(reference)
    tmp = tempfile.mkdtemp(prefix="bhrt_refparity_")
    out, render = {}, {}

    pre = os.path.join(tmp, "c4")
    run(HARNESS, "c4_textured.xml", pre, "dump", cwd=SCENES)
    for ext, dt in (("nodes_f32", np.uint32), ("nodes_i32", np.int32), ("mesh0.bvh_u32", np.uint32), ("mesh0.bvh_f32", np.uint32),
                    ("mesh0.elems_u32", np.uint32), ("mesh0.vn_f32", np.uint32), ("lights_f32", np.float32)):
        out["dump_c4_textured_" + ext.replace(".", "_")] = np.fromfile(pre + "." + ext, dt)

    rels = sorted(os.path.relpath(f, SHIPPED) for f in glob.glob(os.path.join(SHIPPED, "Resource", "**", "*.xml"), recursive=True))
    for rel in rels:
        pre = os.path.join(tmp, "d_" + key(rel))
        run(HARNESS, rel, pre, "dump", cwd=SHIPPED)
        for ext, dt in (("nodes_f32", np.uint32), ("nodes_i32", np.int32), ("camera_f32", np.uint32), ("lights_f32", np.uint32),
                        ("materials_f32", np.float32)):
            out[f"dump_{key(rel)}_{ext}"] = np.fromfile(pre + "." + ext, dt)

    for name in INTEGRATOR_SCENES:
        rel = os.path.join("Resource", "Data", name + ".xml")
        pre = os.path.join(tmp, "r_" + name)
        run(HARNESS, rel, pre, "--spp", 2, "--gi", 3, "--region", *INTEGRATOR_REGION, "render", cwd=SHIPPED)
        render[f"render_{name}_samples"] = np.fromfile(pre + ".samples_f32", np.float32)
        render[f"render_{name}_rgb8"] = np.fromfile(pre + ".rgb8", np.uint8)

    txt = open(os.path.join(SCENES, "c3_mesh.xml")).read().replace('<width value="1920"/>', '<width value="480"/>').replace(
        '<height value="1080"/>', '<height value="270"/>')
    mesh = os.path.join(SCENES, "gen", "mesh_224.obj")
    if not os.path.exists(mesh):
        import gen_mesh
        gen_mesh.generate(mesh, 224)
    xml = os.path.join(SCENES, "_tmp_c3_480.xml")
    open(xml, "w").write(txt)
    try:
        pre = os.path.join(tmp, "c3")
        run(HARNESS, "_tmp_c3_480.xml", pre, "dump", "primary", cwd=SCENES)
    finally:
        os.remove(xml)
    ri = np.fromfile(pre + ".primary_i32", np.int32).reshape(-1, 2)
    rf = np.fromfile(pre + ".primary_f32", np.float32).reshape(-1, 16)
    out["mesh480_bvh_u32_sha"] = sha(np.fromfile(pre + ".mesh0.bvh_u32", np.uint32))
    out["mesh480_primary_node"] = ri[:, 0].copy()
    out["mesh480_hit_attrs_sha"] = sha(rf[ri[:, 0] >= 0][:, :9])

    fdir = os.path.join(tmp, "fuzz")
    os.makedirs(fdir)
    shutil.copy(os.path.join(SCENES, "mesh_small.obj"), os.path.join(fdir, "mesh_small.obj"))
    for seed in FUZZ_SEEDS:
        rng = np.random.default_rng(seed)
        xml = f"fuzz_{seed}.xml"
        fuzz_parity.random_scene(rng, os.path.join(fdir, xml))
        gi = int(rng.integers(0, 4))
        pre = os.path.join(fdir, f"r{seed}")
        run(HARNESS, xml, pre, "--spp", 2, "--gi", gi, "--seed", seed, "--region", 0, 0, 96, 72, "render", cwd=fdir)
        out[f"fuzz_{seed}_xml"] = np.array(open(os.path.join(fdir, xml)).read())
        out[f"fuzz_{seed}_gi"] = gi
        out[f"fuzz_{seed}_samples_sha"] = sha(np.fromfile(pre + ".samples_f32", np.float32))
        out[f"fuzz_{seed}_rgb8"] = np.fromfile(pre + ".rgb8", np.uint8)

    for seed in PHOTON_SEEDS:
        rng = np.random.default_rng(seed)
        xml = f"f{seed}.xml"
        fuzz_parity.random_scene(rng, os.path.join(fdir, xml))
        out[f"pfuzz_{seed}_xml"] = np.array(open(os.path.join(fdir, xml)).read())
        pre = os.path.join(fdir, f"p{seed}")
        for cmd, n in (("photons", 1500), ("gphotons", 1200)):
            run(HARNESS + "_pm", xml, pre, "--seed", seed, "--photons", n, cmd, cwd=fdir)
            out[f"pfuzz_{seed}_{cmd}_meta"] = np.fromfile(f"{pre}.{cmd}_meta", np.uint64)
            out[f"pfuzz_{seed}_{cmd}_emitted"] = np.fromfile(f"{pre}.{cmd}_emitted", np.uint8).reshape(-1, 24)
            out[f"pfuzz_{seed}_{cmd}_balanced"] = np.fromfile(f"{pre}.{cmd}_balanced", np.uint8).reshape(-1, 24)

    shutil.rmtree(tmp)
    for name, arrays in (("ref_parity", out), ("ref_parity_render", render)):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}.npz: {len(arrays)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")
    print(f"{len(rels)} shipped scenes")


if __name__ == "__main__":
    main()
