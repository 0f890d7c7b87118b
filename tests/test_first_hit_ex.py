"""bhrt_first_hit_ex* (DESIGN.md 23): the three images of bhrt_first_hit* and the node ids of bhrt_first_hit_node* from one trace per pixel, byte
for byte, on the committed scenes, with face materials, and on two scenes the test writes: a 1 x 1 image and a 37 x 19 one (one partial
256-lane workgroup after two full ones) that holds a sphere, a plane, a small mesh and pixels that miss."""
import itertools
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, SCENES

NAMES = ("z", "normal", "albedo", "node")

SMALL = """<xml><scene>
  <background r="0.05" g="0.07" b="0.12"/>
  <object type="plane" name="ground" material="ground"><scale value="12"/></object>
  <object type="obj" name="mesh_small.obj" material="blob">
    <scale value="3.5"/><rotate angle="25" x="1"/><rotate angle="40" z="1"/><translate x="-3" y="1" z="4.2"/>
  </object>
  <object type="sphere" name="ball" material="ball"><scale value="3"/><translate x="5" y="-6" z="3"/></object>
  <material type="blinn" name="ground">
    <diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.3" g="0.3" b="0.35"/><color2 r="0.8" g="0.8" b="0.75"/><scale x="0.1" y="0.1"/></diffuse>
    <specular value="0"/>
  </material>
  <material type="blinn" name="blob"><diffuse r="0.3" g="0.6" b="0.8"/><specular value="0.6"/><glossiness value="30"/></material>
  <material type="blinn" name="ball"><diffuse r="0.8" g="0.2" b="0.2"/><specular value="0.7"/><glossiness value="20"/></material>
  <light type="point" name="pointLight"><intensity value="300"/><position x="4" y="-10" z="20"/></light>
</scene>
<camera><position x="0" y="-30" z="10"/><target x="0" y="0" z="3"/><up x="0" y="0" z="1"/><fov value="40"/><width value="%d"/><height value="%d"/></camera></xml>
"""


def test_exports_and_null_images(B, load_scene):
    """The two symbols are in the library, the header and EXPORTS; four NULL images are BHRT_ERR_ARG on a scene that was never uploaded."""
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in ("bhrt_first_hit_ex", "bhrt_first_hit_ex_dev"):
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr), s
    sc = B.Scene(os.path.join(SCENES, "c1_sphere_plane.xml"))
    try:
        assert B.lib().bhrt_first_hit_ex(sc._h, None, None, None, None) == 3
        assert B.lib().bhrt_first_hit_ex_dev(sc._h, None, None, None, None, None) == 3
        assert B.lib().bhrt_first_hit_ex(None, None, None, None, None) == 3
        with pytest.raises(B.BhrtError, match="no image"):
            sc.first_hit_ex(want=())
    finally:
        sc.close()


def _pair(sc):
    z, n, a = sc.first_hit()
    return {"z": z, "normal": n, "albedo": a, "node": sc.first_hit_node()}


def _check_equal(sc):
    ref, got = _pair(sc), sc.first_hit_ex()
    for k in NAMES:
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), k
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,face_materials", [("c3_mesh_small", False), ("c3_mesh_small", True), ("c4_textured", False), ("c4_textured", True),
                                                 ("facemtl_room", False), ("facemtl_room", True)])
def test_equals_the_two_kernels(B, name, face_materials):
    """facemtl_room is the scene with sub-materials: with the switch on it runs the face-material instantiation of both kernels."""
    sc = B.Scene(os.path.join(SCENES, name + ".xml"))
    try:
        sc.set_face_materials(face_materials)
        ref = _check_equal(sc)
        assert (ref["node"] >= 0).any()
    finally:
        sc.close()


@pytest.fixture(scope="module")
def written(B, tmp_path_factory):
    d = tmp_path_factory.mktemp("first_hit_ex")
    shutil.copy(os.path.join(SCENES, "mesh_small.obj"), d / "mesh_small.obj")
    scenes = {}
    for w, h in ((1, 1), (37, 19)):
        p = d / ("s%dx%d.xml" % (w, h))
        p.write_text(SMALL % (w, h))
        scenes[(w, h)] = B.Scene(str(p))
    yield scenes
    for sc in scenes.values():
        sc.close()


@pytest.mark.gpu
def test_one_pixel_image(written):
    ref = _check_equal(written[(1, 1)])
    assert ref["node"].shape == (1, 1)


@pytest.mark.gpu
def test_partial_workgroup_with_every_kind_of_pixel(written):
    ref = _check_equal(written[(37, 19)])
    assert 37 * 19 % 256 != 0 and set(np.unique(ref["node"])) == {-1, 0, 1, 2}   # misses, the plane, the mesh, the sphere


@pytest.mark.gpu
def test_every_subset_of_null_pointers_and_the_device_variant(B, written):
    """Every non-empty subset of the four images, host call and _dev call: the images asked for hold the full call's bytes, and the others'
    memory is not written."""
    import torch
    sc = written[(37, 19)]
    full = sc.first_hit_ex()
    for r in range(1, 5):
        for want in itertools.combinations(NAMES, r):
            got = sc.first_hit_ex(want=want)
            assert set(got) == set(want)
            for k in want:
                assert got[k].tobytes() == full[k].tobytes(), (want, k)
            # the device variant into poisoned tensors: the ones left out keep the poison
            dev = {k: torch.full(full[k].shape, -7, dtype=torch.int32 if k == "node" else torch.float32, device="cuda") for k in NAMES}
            torch.cuda.synchronize()
            sc.first_hit_ex_dev(**{"d_" + k: dev[k].data_ptr() for k in want})
            torch.cuda.synchronize()
            for k in NAMES:
                host = dev[k].cpu().numpy()
                assert host.tobytes() == full[k].tobytes() if k in want else (host == -7).all(), (want, k)
