"""bhrt render --temporal N --denoise --spatial-variance: --spp 1 becomes legal, the rendered frame's variance at 1 spp and the
variance the denoiser gets at every spp come from bhrt_variance_spatial, and what goes on to the next frame is untouched."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from test_cli import CLI, _png, _run
from test_cli_temporal import POSE0, POSE_FLAGS, TO_POS, XML

f32 = np.float32
TEMPORAL = ["--temporal", "3", "--denoise"]


@pytest.mark.parametrize("extra", [["--spatial-variance"], ["--spatial-variance", "--denoise"], ["--spatial-variance", "--temporal", "3"],
                                   TEMPORAL + ["--variance-radius", "2"], TEMPORAL + ["--variance-min-length", "8"],
                                   TEMPORAL + ["--spatial-variance", "--variance-radius", "0"], TEMPORAL + ["--spatial-variance", "--variance-radius", "5"],
                                   TEMPORAL + ["--spatial-variance", "--variance-min-length", "nan"], TEMPORAL + ["--spatial-variance", "--spp", "0"],
                                   TEMPORAL + ["--spp", "1"]])
def test_usage_errors(tmp_path, extra):
    """The flag without --temporal N --denoise, its two values without the flag, a radius outside 1..4, a min-length that is no number, and
    still --spp 1 without the flag: exit 2 before any device is touched, nothing written."""
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png"), "--spp", "2"] + extra, cwd=SCENES, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and not os.listdir(tmp_path)


def _python_sequence(B, sc, frames, spp, radius=None, min_length=None):
    """The wrappers' sequence of render_temporal with --denoise --spatial-variance."""
    ro, to, dn = B.default_reproject_opts(), B.default_temporal_opts(), B.default_denoise_opts()
    sv = B.default_spatial_variance_opts(min_length=4.0 * spp if min_length is None else min_length)
    if radius is not None:
        sv.radius = radius
    p0, p1 = np.float32(POSE0).reshape(-1), np.float32((TO_POS,) + POSE0[1:]).reshape(-1)
    prev = None
    for k in range(3):
        p = (p0 + (p1 - p0) * (f32(k) / f32(2))).astype(f32)
        sc.set_camera(p[0:3], p[3:6], p[6:9])
        z, n, a = sc.first_hit()
        _, rad, var = sc.render_var(B.default_opts(spp=spp, seed=5 + k))
        if spp < 2:
            assert not var.any()
            var = sc.variance_spatial(sv, rad, None, None, z, n, a)
        h = hv = l = None
        if prev is not None:
            fr, pz, pn, acc, accv, ln, pa = prev
            h, hv, l = sc.reproject_var(ro, fr, pz, pn, acc, accv, ln, pa, z, n, a, want=("history", "history_variance", "length"))[:3]
        acc, accv, ln, _ = sc.temporal_accumulate_var(to, rad, var, float(spp), h, hv, l)
        est = sc.variance_spatial(sv, acc, accv, ln, z, n, a)
        rgb = sc.denoise(dn, acc, est, z, n, a)[1]
        assert np.array_equal(rgb, frames[k]), k
        prev = (sc.camera_frame(), z, n, acc, accv, ln, a)
    return ln, accv, est


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 2])
def test_three_frames_equal_the_python_sequence(B, tmp_path, spp):
    png, prefix = str(tmp_path / "last.png"), str(tmp_path / "frame_")
    out = _run(["render", XML, "-o", png, "--spp", str(spp), "--seed", "5", "--frames-png", prefix] + TEMPORAL + ["--spatial-variance"] + POSE_FLAGS, SCENES)
    assert "wrote " + png in out and "frame 2:" in out
    frames = [_png(prefix + "%03d.png" % k) for k in range(3)]
    assert np.array_equal(_png(png), frames[2])
    sc = B.Scene(XML)
    try:
        ln, accv, est = _python_sequence(B, sc, frames, spp)
        assert (ln < 4 * spp).all() and not np.array_equal(est, accv)      # three frames are a short history everywhere: every pixel is estimated
    finally:
        sc.close()
    if spp == 2:                                                           # the flag changes what is written
        plain = str(tmp_path / "plain_")
        _run(["render", XML, "-o", png, "--spp", "2", "--seed", "5", "--frames-png", plain] + TEMPORAL + POSE_FLAGS, SCENES)
        assert not np.array_equal(_png(plain + "000.png"), frames[0])


@pytest.mark.gpu
def test_radius_and_min_length_reach_the_stage(B, tmp_path):
    png, prefix = str(tmp_path / "last.png"), str(tmp_path / "frame_")
    _run(["render", XML, "-o", png, "--spp", "1", "--seed", "5", "--frames-png", prefix, "--variance-radius", "2", "--variance-min-length", "2.5"] + TEMPORAL +
         ["--spatial-variance"] + POSE_FLAGS, SCENES)
    frames = [_png(prefix + "%03d.png" % k) for k in range(3)]
    sc = B.Scene(XML)
    try:
        ln, accv, est = _python_sequence(B, sc, frames, 1, radius=2, min_length=2.5)
        short = ~(ln >= 2.5)
        assert short.any() and (~short).any()                              # both kinds of pixel: estimated and passed through
        assert np.array_equal(est[~short], accv[~short]) and not np.array_equal(est[short], accv[short])
    finally:
        sc.close()
