"""`bhrt render --lens [--dof R] [--focaldist D]`: the thin-lens camera from the host program, alone and over rehearsed ranks."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

CLI = os.path.join(ROOT, "bhraytracer_amd", "bhrt")
XML = os.path.join(SCENES, "lens_spheres.xml")
ARGS = ["--spp", "4", "--seed", "6", "--gi", "3"]


@pytest.fixture
def scene(B):
    opened = []

    def _load(name):
        opened.append(B.Scene(os.path.join(SCENES, name + ".xml")))
        return opened[-1]
    yield _load
    for sc in opened:
        sc.close()


def _run(args, cwd):
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.mark.parametrize("extra", [["--dof", "-1"], ["--dof", "x"], ["--focaldist", "nan"], ["--focaldist", "0"], ["--dof", "inf"], ["--dof", "1.5x"]])
def test_cli_lens_usage_errors(tmp_path, extra):
    """Refused while the options are read: no scene is loaded and no device is touched (this runs without one)."""
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png")] + extra, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and r.stderr.startswith("bhrt: usage:"), (r.returncode, r.stderr)
    assert not (tmp_path / "x.png").exists()


@pytest.mark.gpu
def test_cli_lens_png_is_the_library_render(B, scene, tmp_path):
    sc = scene("lens_spheres")
    png, pin = str(tmp_path / "l.png"), str(tmp_path / "p.png")
    out = _run(["render", XML, "-o", png, "--lens"] + ARGS, SCENES)
    assert "lens: focal distance 30.5, aperture radius 1.5" in out
    rgb, _, _ = sc.render(B.default_opts(spp=4, seed=6, gi_bounces=3, lens=1))
    assert np.array_equal(_png(png), rgb)
    out = _run(["render", XML, "-o", pin] + ARGS, SCENES)  # without --lens: the pinhole frame, whatever the scene's <dof>
    assert "lens:" not in out
    prgb, _, _ = sc.render(B.default_opts(spp=4, seed=6, gi_bounces=3))
    assert np.array_equal(_png(pin), prgb) and not np.array_equal(prgb, rgb)


@pytest.mark.gpu
def test_cli_dof_and_focaldist_are_set_lens(B, scene, tmp_path):
    sc = scene("lens_spheres")
    png = str(tmp_path / "l.png")
    out = _run(["render", XML, "-o", png, "--dof", "0.75", "--focaldist", "22"] + ARGS, SCENES)
    assert "lens: focal distance 22, aperture radius 0.75" in out
    sc.set_lens(22.0, 0.75)
    rgb, _, _ = sc.render(B.default_opts(spp=4, seed=6, gi_bounces=3, lens=1))
    assert np.array_equal(_png(png), rgb)


@pytest.mark.gpu
def test_cli_lens_over_rehearsed_ranks(tmp_path):
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    out = _run(["render", XML, "-o", a, "--tile", "16", "--gpus", "3", "--rehearse", "--lens", "--dof", "1.0"] + ARGS, SCENES)
    assert "3 GPU(s)" in out and "rehearsed" in out and "aperture radius 1" in out
    _run(["render", XML, "-o", b, "--device", "0", "--lens", "--dof", "1.0"] + ARGS, SCENES)
    assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.gpu
def test_cli_lens_with_denoise_prints_the_note(tmp_path):
    out = _run(["render", XML, "-o", str(tmp_path / "d.png"), "--lens", "--denoise"] + ARGS, SCENES)
    assert "guides" in out and "pinhole" in out
