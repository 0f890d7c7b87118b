"""`bhrt render --global-map N [--global-radius R]`: the global gather from the host program."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

CLI = os.path.join(ROOT, "bhraytracer_amd", "bhrt")
ARGS = ["--spp", "2", "--seed", "9", "--gi", "0", "--bounces", "0"]
N_MAP, RADIUS, SIZE = 5000, 0.3, 32

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_cli_global_map_png_is_the_library_render(B, tmp_path):
    text = open(os.path.join(SCENES, "c5_caustics.xml")).read()
    assert text.count('<width value="320"/>') == 1 and text.count('<height value="240"/>') == 1
    xml = str(tmp_path / "scene.xml")
    open(xml, "w").write(text.replace('<width value="320"/>', f'<width value="{SIZE}"/>').replace('<height value="240"/>', f'<height value="{SIZE}"/>'))
    sc = B.Scene(xml)
    try:
        opts = B.default_opts(spp=2, seed=9, gi_bounces=0, internal_bounces=0)
        off, _, _ = sc.render(opts)
        assert sc.global_map_build(opts, N_MAP) == N_MAP  # the render's seed
        sc.set_global_gather(True, RADIUS)
        on, _, st = sc.render(opts)
        assert st.global_gather_queries > 0
    finally:
        sc.close()
    assert (on != off).any(axis=2).mean() >= 0.05
    a, b, c = str(tmp_path / "a.png"), str(tmp_path / "b.png"), str(tmp_path / "c.png")
    out = _run(["render", xml, "-o", a, "--global-map", str(N_MAP), "--global-radius", str(RADIUS)] + ARGS, str(tmp_path))
    assert f"global photon map: {N_MAP} photons" in out
    assert np.array_equal(_png(a), on)
    out = _run(["render", xml, "-o", b, "--global-map", str(N_MAP), "--global-radius", str(RADIUS), "--tile", "8", "--gpus", "2", "--rehearse"] + ARGS, str(tmp_path))
    assert "2 GPU(s)" in out and "rehearsed" in out  # every rank builds the whole map; the clones carry the switch
    assert np.array_equal(_png(b), on) and open(a, "rb").read() == open(b, "rb").read()
    _run(["render", xml, "-o", c] + ARGS, str(tmp_path))  # without the flag: the frame as it was
    assert np.array_equal(_png(c), off) and not np.array_equal(_png(c), _png(a))
