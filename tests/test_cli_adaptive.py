"""`bhrt render --adaptive`: adaptive sampling from the host program, the sample-count image (--samples-png, SaveSampleCountImage,
scene.h:630), the counts' block through the multi-GPU path and the adaptive variance as the denoiser's input."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES, same_bits

CLI = os.path.join(ROOT, "bhraytracer_amd", "bhrt")
ARGS = ["--spp", "32", "--spp-min", "4", "--adaptive-threshold", "0.05", "--seed", "6", "--gi", "3"]


@pytest.fixture
def scene(B):
    """Private scene handles, freed with their device state when the test ends: the workspaces these tests grow stay out of the
    session's shared scene cache."""
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


def _png(path, mode="RGB"):
    from PIL import Image
    return np.asarray(Image.open(path).convert(mode))


@pytest.mark.parametrize("extra", [["--samples-png", "s.png", "--rank", "0", "--world", "2"], ["--spp", "4", "--spp-min", "8"]])
def test_cli_adaptive_usage_errors(tmp_path, extra):
    """Refused before any device is touched (this runs without one)."""
    r = subprocess.run([CLI, "render", os.path.join(SCENES, "c3_mesh_small.xml"), "-o", str(tmp_path / "x.png"), "--adaptive"] + extra,
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and "usage" in r.stderr
    assert not (tmp_path / "x.png").exists() and not (tmp_path / "s.png").exists()


@pytest.mark.gpu
def test_cli_adaptive_png_and_samples_png_are_the_library_pipeline(B, scene, tmp_path):
    sc = scene("c3_room_small")
    png, spng = str(tmp_path / "a.png"), str(tmp_path / "s.png")
    out = _run(["render", os.path.join(SCENES, "c3_room_small.xml"), "-o", png, "--adaptive", "--samples-png", spng] + ARGS, SCENES)
    rgb, rad, var, cnt, st = sc.render_adaptive(B.default_opts(spp=32, seed=6, gi_bounces=3), B.default_adaptive_opts(min_spp=4, threshold=0.05))
    img, smax = sc.sample_count_image(cnt)
    assert np.array_equal(_png(png), rgb)
    assert np.array_equal(_png(spng, "L"), img) and smax == cnt.max()
    assert f"{int(cnt.sum())} samples" in out and "adaptive:" in out


@pytest.mark.gpu
def test_cli_adaptive_over_rehearsed_ranks(tmp_path):
    xml = os.path.join(SCENES, "c3_mesh_small.xml")
    a, b, sa, sb = (str(tmp_path / n) for n in ("a.png", "b.png", "sa.png", "sb.png"))
    out = _run(["render", xml, "-o", a, "--samples-png", sa, "--tile", "16", "--gpus", "3", "--rehearse", "--adaptive"] + ARGS, SCENES)
    assert "3 GPU(s)" in out and "rehearsed" in out
    _run(["render", xml, "-o", b, "--samples-png", sb, "--device", "0", "--adaptive"] + ARGS, SCENES)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert open(sa, "rb").read() == open(sb, "rb").read()


@pytest.mark.gpu
def test_cli_adaptive_denoise_uses_the_adaptive_variance(B, scene, tmp_path):
    sc = scene("c3_room_small")
    png, f32 = str(tmp_path / "d.png"), str(tmp_path / "d.f32")
    _run(["render", os.path.join(SCENES, "c3_room_small.xml"), "-o", png, "--radiance", f32, "--adaptive", "--denoise"] + ARGS, SCENES)
    rgb, rad, var, cnt, _ = sc.render_adaptive(B.default_opts(spp=32, seed=6, gi_bounces=3), B.default_adaptive_opts(min_spp=4, threshold=0.05))
    _, drgb = sc.denoise(B.default_denoise_opts(), rad, var)
    assert np.array_equal(_png(png), drgb) and not np.array_equal(drgb, rgb)
    assert same_bits(np.fromfile(f32, np.float32).reshape(rad.shape), rad)
