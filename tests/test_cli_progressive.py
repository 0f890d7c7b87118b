"""The host program's --progressive N [--time-limit SECONDS] [--live-png PATH] (csrc/bhrt_main.cpp): the frame rendered as a
bhrt_progressive_* session, one line per step, and the same bytes on disk as the blocking render."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

CLI = os.path.join(ROOT, "bhraytracer_amd", "bhrt")
XML = os.path.join(SCENES, "c3_room_small.xml")


def _run(args, cwd):
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _step_lines(out):
    return [[int(x) for x in m.groups()] for m in re.finditer(r"^step (\d+): spp min (\d+) max (\d+), (\d+) active pixel\(s\), [0-9.]+ s$", out, re.M)]


@pytest.mark.parametrize("args", [
    ["--time-limit", "1"],
    ["--live-png", "live.png"],
    ["--progressive", "0"],
    ["--progressive", "-2"],
    ["--progressive", "2", "--gpus", "2"],
    ["--progressive", "2", "--time-limit", "-1"],
])
def test_usage_errors_exit_with_2_before_a_device_is_touched(args, tmp_path):
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png")] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr, r.stderr
    assert not os.listdir(str(tmp_path))


@pytest.mark.gpu
def test_progressive_writes_the_blocking_render_s_bytes(tmp_path):
    a, b, live = str(tmp_path / "a.png"), str(tmp_path / "b.png"), str(tmp_path / "live.png")
    common = ["render", XML, "--spp", "8", "--gi", "3", "--seed", "9"]
    out = _run(common + ["--progressive", "3", "-o", a, "--live-png", live], SCENES)
    blocking = _run(common + ["-o", b], SCENES)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert _step_lines(out) == [[1, 3, 3, 320 * 240], [2, 6, 6, 320 * 240], [3, 8, 8, 0]]
    assert not _step_lines(blocking) and "progressive:" not in blocking
    from PIL import Image
    im = Image.open(live)
    assert im.mode == "RGB" and im.size == (320, 240)
    assert np.array_equal(np.asarray(im), np.asarray(Image.open(a)))  # the last refresh is the final frame
    assert not os.path.exists(live + ".tmp")


@pytest.mark.gpu
def test_time_limit_stops_after_the_first_step_beyond_it(tmp_path):
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    out = _run(["render", XML, "--spp", "8", "--seed", "9", "--progressive", "2", "--time-limit", "0", "-o", a], SCENES)
    assert _step_lines(out) == [[1, 2, 2, 320 * 240]] and "stopped by --time-limit" in out
    _run(["render", XML, "--spp", "2", "--seed", "9", "-o", b], SCENES)
    assert open(a, "rb").read() == open(b, "rb").read()  # the frame at that moment


@pytest.mark.gpu
def test_progressive_adaptive_on_the_schedule_is_the_adaptive_run(tmp_path):
    p = {k: str(tmp_path / k) for k in ("a.png", "a_cnt.png", "b.png", "b_cnt.png")}
    common = ["render", XML, "--seed", "9", "--adaptive", "--spp-min", "4", "--spp", "8", "--adaptive-threshold", "0.05"]
    out = _run(common + ["--progressive", "4", "-o", p["a.png"], "--samples-png", p["a_cnt.png"]], SCENES)
    _run(common + ["-o", p["b.png"], "--samples-png", p["b_cnt.png"]], SCENES)
    assert open(p["a_cnt.png"], "rb").read() == open(p["b_cnt.png"], "rb").read()
    assert open(p["a.png"], "rb").read() == open(p["b.png"], "rb").read()
    steps = _step_lines(out)
    assert [s[:3] for s in steps] == [[1, 4, 4], [2, 4, 8]] and 0 < steps[0][3] < 320 * 240 and steps[1][3] == 0
