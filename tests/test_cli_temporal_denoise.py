"""bhrt render --temporal N --denoise: every frame accumulated with its variance carried along and written denoised; the
un-denoised accumulated frame and its variance go on to the next frame."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from test_cli import CLI, _png, _run
from test_cli_node_transform import DELTA, NESTED, NESTED_POSE, NESTED_POSE_FLAGS
from test_cli_temporal import POSE0, POSE_FLAGS, TO_POS, XML

f32 = np.float32


@pytest.mark.parametrize("extra", [["--spp", "1"], ["--spp", "2", "--guide-spp", "4"], ["--spp", "2", "--guide-spp", "4", "--coverage-filter"]])
def test_usage_errors(tmp_path, extra):
    """--temporal with --denoise at 1 spp (no variance), with --guide-spp and with --coverage-filter: exit 2 before any device is touched."""
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png"), "--temporal", "3", "--denoise", "--frames-png", str(tmp_path / "f_")] + POSE_FLAGS + extra,
                       cwd=SCENES, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and not os.listdir(tmp_path)


def _python_sequence(B, sc, frames, set_state, moving):
    """The wrappers' sequence of render_temporal with --denoise: frame k's bytes are denoise(accumulated frame, its carried variance)."""
    ro, to, dn = B.default_reproject_opts(), B.default_temporal_opts(), B.default_denoise_opts()
    prev = None
    for k in range(3):
        set_state(k)
        z, n, a = sc.first_hit()
        _, rad, var = sc.render_var(B.default_opts(spp=2, seed=5 + k))
        ids = sc.first_hit_node() if moving else None
        h = hv = l = None
        if prev is not None:
            fr, xf, pz, pn, acc, accv, ln, pa, pid = prev
            h, hv, l = sc.reproject_var(ro, fr, pz, pn, acc, accv, ln, pa, z, n, a, prev_xforms=xf, prev_id=pid, id=ids,
                                        want=("history", "history_variance", "length"))[:3]
        acc, accv, ln, plain = sc.temporal_accumulate_var(to, rad, var, 2.0, h, hv, l)
        rgb = sc.denoise(dn, acc, accv, z, n, a)[1]
        assert np.array_equal(rgb, frames[k]), k
        assert not np.array_equal(rgb, plain)                          # the file holds the denoised frame, not the accumulated one
        prev = (sc.camera_frame(), sc.node_transforms() if moving else None, z, n, acc, accv, ln, a, ids)
    return ln, ids


@pytest.mark.gpu
def test_three_denoised_frames_equal_the_python_sequence(B, tmp_path):
    png, prefix = str(tmp_path / "last.png"), str(tmp_path / "frame_")
    out = _run(["render", XML, "-o", png, "--temporal", "3", "--denoise", "--spp", "2", "--seed", "5", "--frames-png", prefix] + POSE_FLAGS, SCENES)
    assert "wrote " + png in out and "frame 2:" in out
    frames = [_png(prefix + "%03d.png" % k) for k in range(3)]
    assert np.array_equal(_png(png), frames[2])
    sc = B.Scene(XML)
    try:
        p0, p1 = np.float32(POSE0).reshape(-1), np.float32((TO_POS,) + POSE0[1:]).reshape(-1)

        def set_state(k):
            p = (p0 + (p1 - p0) * (f32(k) / f32(2))).astype(f32)
            sc.set_camera(p[0:3], p[3:6], p[6:9])
        ln, _ = _python_sequence(B, sc, frames, set_state, False)
        assert (ln > 2).mean() > 0.5
    finally:
        sc.close()


@pytest.mark.gpu
def test_three_denoised_frames_of_a_moving_node_equal_the_python_sequence(B, tmp_path):
    png, prefix = str(tmp_path / "last.png"), str(tmp_path / "frame_")
    out = _run(["render", NESTED, "-o", png, "--temporal", "3", "--denoise", "--spp", "2", "--seed", "5", "--frames-png", prefix, "--node-to-translate",
                "parent:%g,%g,%g" % DELTA] + NESTED_POSE_FLAGS, SCENES)
    assert "wrote " + png in out and "frame 2:" in out
    frames = [_png(prefix + "%03d.png" % k) for k in range(3)]
    assert np.array_equal(_png(png), frames[2]) and not np.array_equal(frames[0], frames[2])
    sc = B.Scene(NESTED)
    try:
        node = sc.node_index("parent")
        saved = sc.node_transform(node)

        def set_state(k):
            sc.set_camera(*NESTED_POSE)
            s = f32(k) / f32(2)
            sc.set_node_transform(node, saved["tm"], saved["pos"], [B.translate(*[float(f32(d) * s) for d in DELTA])])
        ln, ids = _python_sequence(B, sc, frames, set_state, True)
        assert (ln[np.isin(ids, [1, 2, 3])] > 2).mean() > 0.5
    finally:
        sc.close()
