"""bhrt render --temporal N --denoise --reject-change: the session's change test from the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from test_cli import CLI, _png, _run
from test_cli_temporal import POSE0, POSE_FLAGS, TO_POS, XML

f32 = np.float32


@pytest.mark.parametrize("extra", [["--reject-change"], ["--temporal", "3", "--reject-change"], ["--denoise", "--reject-change"],
                                   ["--temporal", "3", "--denoise", "--change-radius", "2"], ["--temporal", "3", "--denoise", "--change-sigma", "1,2"],
                                   ["--temporal", "3", "--denoise", "--reject-change", "--change-radius", "0"],
                                   ["--temporal", "3", "--denoise", "--reject-change", "--change-radius", "5"],
                                   ["--temporal", "3", "--denoise", "--reject-change", "--change-sigma", "2,1"],
                                   ["--temporal", "3", "--denoise", "--reject-change", "--change-sigma", "1"],
                                   ["--temporal", "3", "--denoise", "--reject-change", "--change-sigma", "-1,2"],
                                   ["--temporal", "3", "--denoise", "--reject-change", "--change-sigma", "1,nan"]])
def test_cli_usage_errors(tmp_path, extra):
    """The flag outside --temporal N --denoise, R or LO,HI without the flag, R outside 1..4, a malformed pair: exit 2 before any device is touched."""
    xml = os.path.join(SCENES, "c1_sphere_plane.xml")
    r = subprocess.run([CLI, "render", xml, "-o", str(tmp_path / "x.png"), "--spp", "2"] + extra, cwd=SCENES, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and not os.path.exists(tmp_path / "x.png")


def _python_frames(B, change):
    p0, p1 = np.float32(POSE0).reshape(-1), np.float32((TO_POS,) + POSE0[1:]).reshape(-1)
    sc = B.Scene(XML)
    out = []
    try:
        sc.temporal_begin(B.default_opts(spp=1, seed=5), B.default_temporal_session_opts(carry_variance=1, spatial_variance=1, denoise=1))
        if change is not None:
            sc.temporal_set_change(change)
        for k in range(3):
            p = (p0 + (p1 - p0) * (f32(k) / f32(2))).astype(f32)
            sc.set_camera(p[0:3], p[3:6], p[6:9])
            out.append(sc.temporal_frame(want_radiance=False)[0])
    finally:
        sc.close()
    return out


@pytest.mark.gpu
def test_cli_frames_equal_the_python_session(B, tmp_path):
    """With the flag the frames are those of a Python session with bhrt_temporal_set_change (the defaults; R and LO,HI reach the options); without
    it they are those of a session without the stage, as before."""
    base = ["render", XML, "--spp", "1", "--seed", "5", "--temporal", "3", "--denoise", "--spatial-variance"] + POSE_FLAGS
    for name, flags, change in (("on", ["--reject-change"], B.default_change_opts()), ("off", [], None),
                                ("opts", ["--reject-change", "--change-radius", "2", "--change-sigma", "0.5,1"], B.default_change_opts(radius=2, sigma_lo=0.5, sigma_hi=1.0))):
        png, prefix = str(tmp_path / (name + ".png")), str(tmp_path / (name + "_"))
        out = _run(base + ["-o", png, "--frames-png", prefix] + flags, SCENES)
        want = _python_frames(B, change)
        for k in range(3):
            assert np.array_equal(_png(prefix + "%03d.png" % k), want[k]), (name, k)
        assert "frame 2:" in out and np.array_equal(_png(png), want[2])
