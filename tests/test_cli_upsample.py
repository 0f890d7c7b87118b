"""bhrt render --width W --height H and --upsample S: the size flags are bhrt_scene_set_resolution before everything else; --upsample
renders a clone of the scene at 1/S of the size with bhrt_render_var, takes both first hits, and bhrt_upsample writes the full-size frame,
which --denoise then filters with the upsampled variance."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from test_cli import CLI, _png, _run

XML = os.path.join(SCENES, "c1_sphere_plane.xml")
UP = ["--upsample", "2"]


@pytest.mark.parametrize("extra", [["--upsample", "0"], ["--upsample", "9"], ["--upsample", "-2"], ["--upsample", "7"], UP + ["--width", "201"],
                                   UP + ["--height", "151"], UP + ["--temporal", "3"], UP + ["--progressive", "2"], UP + ["--adaptive", "--spp", "8", "--spp-min", "2"],
                                   UP + ["--gpus", "2"], UP + ["--world", "2"], UP + ["--denoise", "--guide-spp", "4"], ["--upsample-depth-tolerance", "0.1"],
                                   ["--upsample-normal-threshold", "0.5"], UP + ["--upsample-depth-tolerance", "-1"], UP + ["--upsample-depth-tolerance", "inf"],
                                   UP + ["--upsample-normal-threshold", "nan"], UP + ["--upsample-normal-threshold", "x"], ["--width", "0"], ["--height", "-3"]])
def test_usage_errors(tmp_path, extra):
    """A factor outside 1..8 or one that does not divide both sides (7 does not divide the scene's 640; 2 not an odd side), --upsample beside a
    mode it does not combine with, a stop without the flag or without a usable value, a size below 1: exit 2 before any device is touched,
    nothing written."""
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png"), "--spp", "2"] + extra, cwd=SCENES, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and not os.listdir(tmp_path), r.stderr


def test_the_scene_the_usage_cases_assume(B):
    sc = B.Scene(XML)
    try:
        assert (sc.width, sc.height) == (640, 480)
    finally:
        sc.close()


def _python_chain(B, spp, seed, s, denoise, size=None, **stops):
    full = B.Scene(XML)
    try:
        if size:
            full.set_resolution(*size)
        low = full.clone()
        try:
            low.set_resolution(full.width // s, full.height // s)
            o = B.default_opts(spp=spp, seed=seed)
            if spp > 1:
                _, c, v = low.render_var(o)
            else:
                c, v = low.render(o)[1], None
            zl, nl, al = low.first_hit()
            z, n, a = full.first_hit()
            up = full.upsample(B.default_upsample_opts(**stops), c, zl, nl, al, v, z, n, a, want=("out", "variance", "rgb8"))
            if not denoise:
                return up["rgb8"]
            return full.denoise(B.default_denoise_opts(), up["out"], up.get("variance"), z, n, a)[1]
        finally:
            low.close()
    finally:
        full.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spp,denoise", [(4, False), (4, True), (1, False), (1, True)])
def test_upsample_equals_the_python_chain(B, tmp_path, spp, denoise):
    png = str(tmp_path / "up.png")
    out = _run(["render", XML, "-o", png, "--spp", str(spp), "--seed", "7"] + UP + (["--denoise"] if denoise else []), SCENES)
    assert "wrote " + png in out and "upsample: 320 x 240 at %d spp -> 640 x 480" % spp in out
    img = _png(png)
    assert img.shape == (480, 640, 3) and np.array_equal(img, _python_chain(B, spp, 7, 2, denoise))
    if spp == 4 and not denoise:                                           # the flag changes what is written
        _run(["render", XML, "-o", png, "--spp", "4", "--seed", "7"], SCENES)
        assert not np.array_equal(_png(png), img)


@pytest.mark.gpu
def test_size_flags_equal_the_setter_and_feed_the_upsampling(B, tmp_path):
    """--width / --height alone and together equal bhrt_scene_set_resolution + bhrt_render; with --upsample the factor divides the new size, and
    the two stops reach the stage."""
    png = str(tmp_path / "s.png")
    for flags, size in ((["--width", "96"], (96, 480)), (["--height", "40"], (640, 40)), (["--width", "33", "--height", "17"], (33, 17))):
        out = _run(["render", XML, "-o", png, "--spp", "2", "--seed", "3"] + flags, SCENES)
        assert "Render image width: %d\nRender image height: %d" % size in out
        sc = B.Scene(XML)
        try:
            sc.set_resolution(*size)
            want = sc.render(B.default_opts(spp=2, seed=3), want_radiance=False)[0]
        finally:
            sc.close()
        assert np.array_equal(_png(png), want), flags
    _run(["render", XML, "-o", png, "--spp", "2", "--seed", "3", "--width", "96", "--height", "64", "--upsample", "4", "--upsample-depth-tolerance", "0.05",
          "--upsample-normal-threshold", "0.5"], SCENES)
    assert np.array_equal(_png(png), _python_chain(B, 2, 3, 4, False, size=(96, 64), depth_tolerance=0.05, normal_threshold=0.5))
