"""`bhrt render --denoise --guide-spp N --coverage-filter [--sigma-coverage X]`: the frame filtered by bhrt_denoise_sampled with bhrt_guides'
four images, on one device and where the multi-GPU path denoises the gathered frame; without the flag the bytes of before."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

CLI = os.path.join(ROOT, "bhraytracer_amd", "bhrt")
XML = os.path.join(SCENES, "lens_spheres.xml")
ARGS = ["--spp", "4", "--seed", "6", "--gi", "3"]


def _run(args, cwd):
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.mark.parametrize("extra", [["--guide-spp", "8", "--coverage-filter"], ["--denoise", "--coverage-filter"], ["--denoise", "--guide-spp", "0", "--coverage-filter"],
                                   ["--denoise", "--guide-spp", "8", "--sigma-coverage", "0.5"], ["--denoise", "--guide-spp", "8", "--coverage-filter", "--sigma-coverage", "-1"],
                                   ["--denoise", "--guide-spp", "8", "--coverage-filter", "--sigma-coverage", "nan"]])
def test_cli_coverage_filter_usage_errors(tmp_path, extra):
    """--coverage-filter without --denoise, without --guide-spp or with --guide-spp 0, --sigma-coverage without the filter or with a bad value:
    refused while the options are read, before a scene is loaded or a device touched."""
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png"), "--lens"] + extra, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and r.stderr.startswith("bhrt: usage:"), (r.returncode, r.stderr)
    assert not (tmp_path / "x.png").exists()


def test_cli_parses_coverage_filter(B, tmp_path):
    """Accepted with --denoise --guide-spp N: the program gets as far as the device (and, where there is none, fails there: no fallback)."""
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png"), "--denoise", "--guide-spp", "2", "--lens", "--spp", "1", "--coverage-filter",
                        "--sigma-coverage", "0.5"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert "usage" not in r.stderr and "unknown option" not in r.stderr
    assert "denoise filter: for sampled guides, coverage tolerance 0.5" in r.stdout
    if B.device_count() > 0:
        assert r.returncode == 0 and (tmp_path / "x.png").exists()
    else:
        assert r.returncode == 1 and "device" in r.stderr.lower() and not (tmp_path / "x.png").exists()


@pytest.fixture(scope="module")
def pipeline(B):
    """The library's frames for ARGS through the lens with guides at 8 spp: bhrt_denoise with the sampled guides, and the coverage filter at
    its default and at sigma_coverage = 0.05 (far from any default the grid of DESIGN.md 17 could choose)."""
    sc = B.Scene(XML)
    try:
        _, rad, var = sc.render_var(B.default_opts(spp=4, seed=6, gi_bounces=3, lens=1))
        g = sc.guides(B.default_opts(spp=8, seed=6, gi_bounces=3, lens=1))
        G = (g["z"], g["normal"], g["albedo"], g["coverage"])
        o = B.default_denoise_opts()
        return {"old": sc.denoise(o, rad, var, *G[:3])[1], "new": sc.denoise_sampled(o, rad, var, *G)[1], "new_0.05": sc.denoise_sampled(o, rad, var, *G, 0.05)[1]}
    finally:
        sc.close()


@pytest.mark.gpu
def test_cli_coverage_filter_png_is_the_library_pipeline(pipeline, tmp_path):
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    out = _run(["render", XML, "-o", a, "--lens", "--denoise", "--guide-spp", "8", "--coverage-filter"] + ARGS, SCENES)
    assert "denoise guides: 8 sample(s) per pixel, through the lens" in out and "denoise filter: for sampled guides" in out
    assert np.array_equal(_png(a), pipeline["new"]) and not np.array_equal(pipeline["new"], pipeline["old"])
    _run(["render", XML, "-o", b, "--lens", "--denoise", "--guide-spp", "8", "--coverage-filter", "--sigma-coverage", "0.05"] + ARGS, SCENES)
    assert np.array_equal(_png(b), pipeline["new_0.05"]) and not np.array_equal(pipeline["new_0.05"], pipeline["new"])


@pytest.mark.gpu
def test_cli_without_the_flag_writes_the_bytes_of_before(pipeline, tmp_path):
    a = str(tmp_path / "a.png")
    out = _run(["render", XML, "-o", a, "--lens", "--denoise", "--guide-spp", "8"] + ARGS, SCENES)
    assert "denoise filter:" not in out
    assert np.array_equal(_png(a), pipeline["old"])


@pytest.mark.gpu
def test_cli_coverage_filter_over_rehearsed_ranks(tmp_path):
    """--gpus 3 --rehearse: guides, coverage and the filter run for the whole frame where the gathered frame is denoised; the one-device PNG."""
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    out = _run(["render", XML, "-o", a, "--tile", "16", "--gpus", "3", "--rehearse", "--lens", "--denoise", "--guide-spp", "5", "--coverage-filter"] + ARGS, SCENES)
    assert "3 GPU(s)" in out and "rehearsed" in out
    _run(["render", XML, "-o", b, "--device", "0", "--lens", "--denoise", "--guide-spp", "5", "--coverage-filter"] + ARGS, SCENES)
    assert open(a, "rb").read() == open(b, "rb").read()
