"""`bhrt render --face-materials`: the face-material switch from the host program."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENES

CLI = os.path.join(ROOT, "bhraytracer_amd", "bhrt")
XML = os.path.join(SCENES, "facemtl_room.xml")
ARGS = ["--spp", "3", "--seed", "9", "--gi", "3"]

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_cli_face_materials_png_is_the_library_render(B, tmp_path):
    sc = B.Scene(XML)
    try:
        opts = B.default_opts(spp=3, seed=9, gi_bounces=3)
        off, _, _ = sc.render(opts)
        sc.set_face_materials(True)
        on, _, _ = sc.render(opts)
    finally:
        sc.close()
    assert (on != off).any(axis=2).mean() >= 0.05
    a, b, c = str(tmp_path / "a.png"), str(tmp_path / "b.png"), str(tmp_path / "c.png")
    _run(["render", XML, "-o", a, "--face-materials"] + ARGS, SCENES)
    assert np.array_equal(_png(a), on)
    out = _run(["render", XML, "-o", b, "--face-materials", "--tile", "8", "--gpus", "2", "--rehearse"] + ARGS, SCENES)  # the clones carry the switch
    assert "2 GPU(s)" in out and "rehearsed" in out
    assert np.array_equal(_png(b), on) and open(a, "rb").read() == open(b, "rb").read()
    _run(["render", XML, "-o", c] + ARGS, SCENES)  # without the flag: the frame the reference renders, sub-material 0 everywhere
    assert np.array_equal(_png(c), off) and not np.array_equal(_png(c), _png(a))
