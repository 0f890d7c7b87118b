"""bhrt render --temporal N: N frames along a camera move, each reprojected into the next view and accumulated there."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from test_cli import CLI, _png, _run

f32 = np.float32
XML = os.path.join(SCENES, "c1_sphere_plane.xml")
POSE0 = ((0.0, -30.0, 10.0), (0.0, 0.0, 3.0), (0.0, 0.0, 1.0))     # the scene's own camera, spelled out: position, target, up
TO_POS = (1.5, -30.0, 10.5)
POSE_FLAGS = ["--camera-pos", "0,-30,10", "--camera-target", "0,0,3", "--camera-up", "0,0,1", "--to-pos", "1.5,-30,10.5"]


@pytest.mark.parametrize("extra", [["--temporal", "1"], ["--temporal", "0"], ["--temporal", "3", "--progressive", "2"], ["--temporal", "3", "--adaptive"],
                                   ["--temporal", "3", "--gpus", "1"], ["--frames-png", "f"], []])
def test_usage_errors(tmp_path, extra):
    """N < 2, --temporal beside --progressive, --adaptive or --gpus, and the move's flags without --temporal: refused before any device is touched."""
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png"), "--to-pos", "1.5,-30,10.5"] + extra, cwd=SCENES, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and not os.path.exists(tmp_path / "x.png")


@pytest.mark.gpu
def test_three_frames_equal_the_python_sequence(B, tmp_path):
    png, prefix = str(tmp_path / "last.png"), str(tmp_path / "frame_")
    out = _run(["render", XML, "-o", png, "--temporal", "3", "--spp", "2", "--seed", "5", "--frames-png", prefix] + POSE_FLAGS, SCENES)
    assert "wrote " + png in out and "frame 2:" in out
    frames = [_png(prefix + "%03d.png" % k) for k in range(3)]
    assert np.array_equal(_png(png), frames[2])
    # the same sequence through the Python wrappers
    sc = B.Scene(XML)
    try:
        p0, p1 = np.float32(POSE0).reshape(-1), np.float32((TO_POS,) + POSE0[1:]).reshape(-1)
        ro, to = B.default_reproject_opts(), B.default_temporal_opts()
        prev = None
        for k in range(3):
            p = (p0 + (p1 - p0) * (f32(k) / f32(2))).astype(f32)
            sc.set_camera(p[0:3], p[3:6], p[6:9])
            z, n, a = sc.first_hit()
            rad = sc.render(B.default_opts(spp=2, seed=5 + k))[1]
            h, l = (None, None) if prev is None else sc.reproject(ro, *prev, z, n, a, want=("history", "length"))[:2]
            acc, ln, rgb = sc.temporal_accumulate(to, rad, 2.0, h, l)
            assert np.array_equal(rgb, frames[k]), k
            prev = (sc.camera_frame(), z, n, acc, ln, a)
        assert (ln > 2).mean() > 0.5                               # the last frame carries history on most of its pixels
    finally:
        sc.close()
