"""`bhrt render --camera-pos / --camera-target / --camera-up / --fov` and `--shutter-pos / --shutter-target / --shutter-up`: the flags
write the PNG that bhrt_scene_set_camera and bhrt_scene_set_shutter give through the library, and a malformed value is a usage error (exit 2)
before a scene is loaded."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

CLI = os.path.join(ROOT, "bhraytracer_amd", "bhrt")
f32 = np.float32
XML = os.path.join(SCENES, "shutter_plain.xml")


def _png(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "RGB"
    return np.asarray(im)


def _csv(v):
    return ",".join(repr(float(x)) for x in v)


@pytest.mark.parametrize("args", [
    ["--camera-pos", "1,2"], ["--camera-pos", "1,2,3,4"], ["--camera-target", "1;2;3"], ["--camera-up", "a,b,c"], ["--camera-pos", "1,nan,3"],
    ["--shutter-pos", "1,2,"], ["--shutter-target", "inf,0,0"], ["--shutter-up", ""], ["--shutter-pos"],
    ["--fov", "200"], ["--fov", "180"], ["--fov", "-1"], ["--fov", "0"], ["--fov", "wide"], ["--fov", "nan"],
])
def test_malformed_values_are_usage_errors_before_a_scene_is_loaded(args, tmp_path):
    missing = str(tmp_path / "no_such_scene.xml")  # loading it would fail with exit status 1
    r = subprocess.run([CLI, "render", missing] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "LoadScene" not in r.stderr and "Render image width" not in r.stdout
    assert ("usage" in r.stderr or "needs a value" in r.stderr) and args[0] in r.stderr


CAMERA = {"pos": (6.0, -27.0, 12.0), "target": (0.5, 0.0, 3.5), "up": (0.05, 0.0, 1.0), "fov": 33.0}
POSE1 = {"pos": (7.5, -26.5, 12.5), "target": (0.0, 0.5, 3.5), "up": (0.0, 0.0, 1.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all_flags", "shutter_pos_alone", "camera_alone_gpus_1"])
def test_the_flags_write_the_png_of_the_library_calls(B, mode, tmp_path):
    png = str(tmp_path / (mode + ".png"))
    args = ["render", XML, "-o", png, "--spp", "2", "--gi", "2", "--seed", "4"]
    sc = B.Scene(XML)
    try:
        cam = sc.flat_view().header.camera
        if mode in ("all_flags", "camera_alone_gpus_1"):
            args += ["--camera-pos", _csv(CAMERA["pos"]), "--camera-target", _csv(CAMERA["target"]), "--camera-up", _csv(CAMERA["up"]), "--fov", repr(CAMERA["fov"])]
            sc.set_camera(CAMERA["pos"], CAMERA["target"], CAMERA["up"], CAMERA["fov"])
        if mode == "all_flags":
            args += ["--shutter-pos", _csv(POSE1["pos"]), "--shutter-target", _csv(POSE1["target"]), "--shutter-up", _csv(POSE1["up"])]
            sc.set_shutter(True, POSE1["pos"], POSE1["target"], POSE1["up"])
        if mode == "shutter_pos_alone":  # target and up from pose 0: the point looked at on the plane of focus, the scene's up
            args += ["--shutter-pos", _csv(POSE1["pos"])]
            pos, d, up = np.array(list(cam.pos), f32), np.array(list(cam.dir), f32), np.array(list(cam.up), f32)
            sc.set_shutter(True, POSE1["pos"], pos + d * f32(cam.focaldist), up)
        if mode == "camera_alone_gpus_1":
            args += ["--gpus", "1"]
        r = subprocess.run([CLI] + args, cwd=SCENES, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "camera: position" in r.stdout and ("shutter: to position" in r.stdout) == (mode != "camera_alone_gpus_1")
        rgb, _, _ = sc.render(B.default_opts(spp=2, gi_bounces=2, seed=4))
        assert sc.shutter()[0] == (mode != "camera_alone_gpus_1")
        plain = B.Scene(XML)
        try:
            still, _, _ = plain.render(B.default_opts(spp=2, gi_bounces=2, seed=4))
        finally:
            plain.close()
    finally:
        sc.close()
    img = _png(png)
    assert np.array_equal(img, rgb) and not np.array_equal(img, still)


def test_poses_the_library_refuses_fail_with_its_message(tmp_path):
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png"), "--spp", "1", "--shutter-pos", "0,30,10"], cwd=SCENES, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 1 and "quarter turn" in r.stderr
