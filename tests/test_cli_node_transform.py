"""bhrt render --node-translate / --node-to-translate: an object moved from the command line, before a render and along the
frames of --temporal."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from test_cli import CLI, _png, _run
from test_node_transform import edited_xml

f32 = np.float32
C1 = os.path.join(SCENES, "c1_sphere_plane.xml")
NESTED = os.path.join(SCENES, "moving_nested.xml")
NESTED_POSE = ((0.0, -18.0, 8.0), (0.0, 0.0, 2.5), (0.0, 0.0, 1.0))     # moving_nested's own camera, spelled out: position, target, up
NESTED_POSE_FLAGS = ["--camera-pos", "0,-18,8", "--camera-target", "0,0,2.5", "--camera-up", "0,0,1"]
DELTA = (1.5, -0.75, 0.5)                                                # the parent's translation at the last frame


@pytest.mark.parametrize("extra", [["--node-translate", "nobody:1,2,3"], ["--node-translate", "ball:1,2"], ["--node-translate", "ball"],
                                   ["--node-translate", ":1,2,3"], ["--node-translate", "ball:1,2,x"], ["--node-translate", "ball:1,2,inf"],
                                   ["--node-to-translate", "ball:1,0,0"], ["--temporal", "3", "--node-to-translate", "nobody:1,0,0"],
                                   ["--temporal", "3", "--node-to-translate", "ball:1,0"]])
def test_usage_errors(tmp_path, extra):
    """An unknown name, a malformed value, --node-to-translate without --temporal: exit 2 before any device is touched, nothing written."""
    r = subprocess.run([CLI, "render", C1, "-o", str(tmp_path / "x.png")] + extra, cwd=SCENES, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and not os.path.exists(tmp_path / "x.png")


@pytest.mark.gpu
def test_node_translate_renders_the_edited_scene_file(B, tmp_path):
    moved, edited = str(tmp_path / "moved.png"), str(tmp_path / "edited.png")
    out = _run(["render", C1, "-o", moved, "--spp", "2", "--seed", "3", "--node-translate", "ball:1.25,-0.5,0.75"], SCENES)
    assert "node ball (1): translated by 1.25,-0.5,0.75" in out
    xml = edited_xml(tmp_path, "c1_sphere_plane", "ball", [B.translate(1.25, -0.5, 0.75)], False)
    _run(["render", xml, "-o", edited, "--spp", "2", "--seed", "3"], str(tmp_path))
    plain = str(tmp_path / "plain.png")
    _run(["render", C1, "-o", plain, "--spp", "2", "--seed", "3"], SCENES)
    assert np.array_equal(_png(moved), _png(edited)) and not np.array_equal(_png(moved), _png(plain))


@pytest.mark.gpu
def test_three_frames_of_a_moving_node_equal_the_python_sequence(B, tmp_path):
    """--temporal 3 --node-to-translate on moving_nested, the camera staying: every frame's bytes are those of the Python wrappers for the same
    sequence (set_node_transform to the saved record plus delta * k / 2, first_hit, first_hit_node, render, reproject_moving, accumulate)."""
    png, prefix = str(tmp_path / "last.png"), str(tmp_path / "frame_")
    out = _run(["render", NESTED, "-o", png, "--temporal", "3", "--spp", "2", "--seed", "5", "--frames-png", prefix, "--node-to-translate",
                "parent:%g,%g,%g" % DELTA] + NESTED_POSE_FLAGS, SCENES)
    assert "wrote " + png in out and "frame 2:" in out
    frames = [_png(prefix + "%03d.png" % k) for k in range(3)]
    assert np.array_equal(_png(png), frames[2]) and not np.array_equal(frames[0], frames[2])
    sc = B.Scene(NESTED)
    try:
        ro, to = B.default_reproject_opts(), B.default_temporal_opts()
        node = sc.node_index("parent")
        saved = sc.node_transform(node)
        prev = None
        for k in range(3):
            sc.set_camera(*NESTED_POSE)
            s = f32(k) / f32(2)
            sc.set_node_transform(node, saved["tm"], saved["pos"], [B.translate(*[float(f32(d) * s) for d in DELTA])])
            z, n, a = sc.first_hit()
            rad = sc.render(B.default_opts(spp=2, seed=5 + k))[1]
            ids = sc.first_hit_node()
            h, l = (None, None) if prev is None else sc.reproject_moving(ro, prev[0], prev[1], prev[2], prev[3], prev[4], prev[5], prev[6], prev[7], z, n, a, ids,
                                                                         want=("history", "length"))[:2]
            acc, ln, rgb = sc.temporal_accumulate(to, rad, 2.0, h, l)
            assert np.array_equal(rgb, frames[k]), k
            prev = (sc.camera_frame(), sc.node_transforms(), z, n, acc, ln, a, ids)
        moved_px = np.isin(ids, [1, 2, 3])
        assert (ln[moved_px] > 2).mean() > 0.5                     # the moved nodes' pixels carry history in the last frame
    finally:
        sc.close()
