"""`bhrt render --denoise`: the PNG is the denoised frame (DenoiseImage of the reference's 64-bit build, Main.cpp:236-238) on one
device and through the multi-GPU path, where the variance tiles travel beside the radiance tiles and GPU 0 denoises the gathered frame."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES, same_bits

CLI = os.path.join(ROOT, "bhraytracer_amd", "bhrt")


def _run(args, cwd):
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_cli_denoise_refuses_a_partial_frame(tmp_path):
    """--world > 1 renders part of the frame: --denoise is a usage error, found before any device is touched (this runs without one)."""
    r = subprocess.run([CLI, "render", os.path.join(SCENES, "c3_mesh_small.xml"), "-o", str(tmp_path / "x.png"), "--denoise", "--rank", "0", "--world", "2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr and "--denoise" in r.stderr
    assert not (tmp_path / "x.png").exists()


@pytest.mark.gpu
def test_cli_denoise_png_is_the_library_pipeline(B, load_scene, tmp_path):
    sc = load_scene("c3_room_small")
    png, f32 = str(tmp_path / "d.png"), str(tmp_path / "d.f32")
    _run(["render", os.path.join(SCENES, "c3_room_small.xml"), "-o", png, "--radiance", f32, "--spp", "4", "--gi", "3", "--seed", "9", "--denoise"], SCENES)
    o = B.default_opts(spp=4, gi_bounces=3, seed=9)
    rgb, rad, var = sc.render_var(o)
    _, drgb = sc.denoise(B.default_denoise_opts(), rad, var)
    assert np.array_equal(_png(png), drgb) and not np.array_equal(drgb, rgb)
    assert same_bits(np.fromfile(f32, np.float32).reshape(rad.shape), rad)       # --radiance: the render's own, not denoised
    k2 = str(tmp_path / "k2.png")
    _run(["render", os.path.join(SCENES, "c3_room_small.xml"), "-o", k2, "--spp", "4", "--gi", "3", "--seed", "9", "--denoise", "--denoise-iters", "2"], SCENES)
    assert np.array_equal(_png(k2), sc.denoise(B.default_denoise_opts(iterations=2), rad, var)[1])


@pytest.mark.gpu
def test_cli_denoise_over_rehearsed_ranks(tmp_path):
    """--gpus 3 --rehearse --denoise: variance tiles packed, exchanged and unpacked beside the radiance; the same PNG as one device."""
    xml = os.path.join(SCENES, "c3_mesh_small.xml")
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    out = _run(["render", xml, "-o", a, "--spp", "4", "--seed", "2", "--tile", "16", "--gpus", "3", "--rehearse", "--denoise"], SCENES)
    assert "3 GPU(s)" in out and "rehearsed" in out
    _run(["render", xml, "-o", b, "--spp", "4", "--seed", "2", "--device", "0", "--denoise"], SCENES)
    assert open(a, "rb").read() == open(b, "rb").read()
