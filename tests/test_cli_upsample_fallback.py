"""bhrt render --upsample S --upsample-fallback albedo|light: the word becomes bhrt_upsample_opts.fallback; without --upsample or
with another word it is a usage error before any device is touched."""
import os
import subprocess

import numpy as np
import pytest

from conftest import SCENES
from test_cli import CLI, _png, _run

XML = os.path.join(SCENES, "c2_glass_small.xml")     # a transparent object before a bright floor: the two rules write different frames
UP = ["--upsample", "2"]


@pytest.mark.parametrize("extra", [["--upsample-fallback", "light"], ["--upsample-fallback", "albedo"], UP + ["--upsample-fallback", "glass"],
                                   UP + ["--upsample-fallback", "1"], UP + ["--upsample-fallback", "Light"], UP + ["--upsample-fallback", ""]])
def test_usage_errors(tmp_path, extra):
    """The flag without --upsample, or with a word that is neither albedo nor light: exit 2 before any device is touched, nothing written."""
    r = subprocess.run([CLI, "render", XML, "-o", str(tmp_path / "x.png"), "--spp", "2"] + extra, cwd=SCENES, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and "--upsample-fallback" in r.stderr and not os.listdir(tmp_path), r.stderr


def _python_chain(B, spp, seed, s, **opts):
    full = B.Scene(XML)
    try:
        low = full.clone()
        try:
            low.set_resolution(full.width // s, full.height // s)
            _, c, v = low.render_var(B.default_opts(spp=spp, seed=seed))
            zl, nl, al = low.first_hit()
        finally:
            low.close()
        z, n, a = full.first_hit()
        return full.upsample(B.default_upsample_opts(**opts), c, zl, nl, al, v, z, n, a, want=("rgb8",))["rgb8"]
    finally:
        full.close()


@pytest.mark.gpu
def test_fallback_flag_equals_the_python_chain(B, tmp_path):
    """--upsample-fallback light writes the bytes of the Python chain with fallback = 1 and says so in the upsample: line; albedo writes the
    PNG of the command without the flag; the two words write different frames on a scene with glass in it."""
    png = {k: str(tmp_path / (k + ".png")) for k in ("light", "albedo", "none")}
    base = ["render", XML, "--spp", "4", "--seed", "7"] + UP
    out = _run(base + ["-o", png["light"], "--upsample-fallback", "light"], SCENES)
    assert "upsample: 160 x 90 at 4 spp -> 320 x 180" in out and "fallback light" in out
    out = _run(base + ["-o", png["albedo"], "--upsample-fallback", "albedo"], SCENES)
    assert "fallback albedo" in out
    _run(base + ["-o", png["none"]], SCENES)
    light, albedo, none = (_png(png[k]) for k in ("light", "albedo", "none"))
    assert light.shape == (180, 320, 3) and np.array_equal(light, _python_chain(B, 4, 7, 2, fallback=B.UPSAMPLE_FALLBACK_LIGHT))
    assert np.array_equal(albedo, none) and np.array_equal(none, _python_chain(B, 4, 7, 2))
    assert not np.array_equal(light, albedo)
