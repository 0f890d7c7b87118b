"""bhrt render --light-pos / --light-dir / --light-intensity / --light-size / --light-to-pos: a light edited from the command
line, before a render and along the frames of --temporal."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from test_cli import CLI, _png, _run
from test_lights import edited_xml

FOUR = os.path.join(SCENES, "lights_four.xml")

USAGE = [
    (["--light-pos", "nobody:1,2,3"], "--light-pos"),                    # an unknown name
    (["--light-dir", "nobody:1,2,3"], "--light-dir"),
    (["--light-intensity", "nobody:1,2,3"], "--light-intensity"),
    (["--light-size", "nobody:1"], "--light-size"),
    (["--light-pos", "Key:1,2,3"], "--light-pos"),                       # names compare exactly
    (["--light-pos", "key:1,2"], "--light-pos"),                         # malformed values
    (["--light-pos", "key"], "--light-pos"),
    (["--light-pos", ":1,2,3"], "--light-pos"),
    (["--light-dir", "sun:1,2,x"], "--light-dir"),
    (["--light-intensity", "amb:1,2,inf"], "--light-intensity"),
    (["--light-size", "fill:"], "--light-size"),
    (["--light-size", "fill:-1"], "--light-size"),
    (["--light-size", "fill:1,2,3"], "--light-size"),
    (["--light-size", "fill:nan"], "--light-size"),
    (["--light-pos", "sun:1,2,3"], "--light-pos"),                       # a light of another kind than the option's
    (["--light-dir", "key:1,2,3"], "--light-dir"),
    (["--light-size", "amb:1"], "--light-size"),
    (["--light-to-pos", "key:1,0,0"], "--light-to-pos"),                 # without --temporal
    (["--temporal", "3", "--light-to-pos", "nobody:1,0,0"], "--light-to-pos"),
    (["--temporal", "3", "--light-to-pos", "key:1,0"], "--light-to-pos"),
    (["--temporal", "3", "--light-to-pos", "sun:1,0,0"], "--light-to-pos"),
]


@pytest.mark.parametrize("extra,option", USAGE)
def test_usage_errors(tmp_path, extra, option):
    """An unknown name, a malformed value, --light-to-pos without --temporal: exit 2 with a message that names the option, before any device is
    touched, nothing written."""
    r = subprocess.run([CLI, "render", FOUR, "-o", str(tmp_path / "x.png")] + extra, cwd=SCENES, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and option in r.stderr and not os.path.exists(tmp_path / "x.png"), r.stderr


def test_a_value_the_library_refuses_fails_with_its_message(tmp_path):
    """A negative intensity passes the command line's parse and is refused by bhrt_scene_set_light, before the upload: non-zero, no image."""
    r = subprocess.run([CLI, "render", FOUR, "-o", str(tmp_path / "x.png"), "--light-intensity", "key:1,-2,3"], cwd=SCENES, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--light-intensity" in r.stderr and "bhrt_scene_set_light" in r.stderr and not os.path.exists(tmp_path / "x.png")


@pytest.mark.gpu
def test_light_flags_render_the_edited_scene_file(tmp_path):
    moved, edited, plain = str(tmp_path / "moved.png"), str(tmp_path / "edited.png"), str(tmp_path / "plain.png")
    common = ["--spp", "2", "--gi", "1", "--seed", "3"]
    out = _run(["render", FOUR, "-o", moved, "--light-pos", "key:1.25,-7.5,17.75", "--light-intensity", "key:0.03,0.01,0.05", "--light-dir", "sun:-0.3,1.7,-2.2",
                "--light-size", "fill:0.25"] + common, SCENES)
    assert "light key (0): pos 1.25,-7.5,17.75" in out and "light key (0): intensity 0.03,0.01,0.05" in out
    assert "light sun (1): dir -0.3,1.7,-2.2" in out and "light fill (3): size 0.25" in out
    xml = edited_xml(tmp_path, "lights_four", [("key", (0.03, 0.01, 0.05), (1.25, -7.5, 17.75), None), ("sun", None, (-0.3, 1.7, -2.2), None),
                                               ("fill", None, None, 0.25)])
    _run(["render", xml, "-o", edited] + common, str(tmp_path))
    _run(["render", FOUR, "-o", plain] + common, SCENES)
    assert np.array_equal(_png(moved), _png(edited)) and not np.array_equal(_png(moved), _png(plain))


@pytest.mark.gpu
def test_three_frames_of_a_moving_light(tmp_path):
    """--temporal 3 --light-to-pos: three frames written, exit 0; the light's move shows between the first and the last."""
    png, prefix = str(tmp_path / "last.png"), str(tmp_path / "frame_")
    out = _run(["render", FOUR, "-o", png, "--temporal", "3", "--spp", "2", "--gi", "1", "--seed", "5", "--frames-png", prefix, "--light-to-pos", "key:14,-10,12"],
               SCENES)
    assert "wrote " + png in out and "frame 2:" in out
    frames = [_png(prefix + "%03d.png" % k) for k in range(3)]
    assert frames[0].shape == (24, 32, 3) and np.array_equal(_png(png), frames[2]) and not np.array_equal(frames[0], frames[2])
