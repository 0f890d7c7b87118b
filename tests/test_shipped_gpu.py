"""The reference's own 19 scene files (tests/golden/shipped) on the GPU.

The chain reference -> oracle -> GPU, in one place: test_ref_parity.py pins the front-end's flat scene of all 19 files to the reference's xmlload
dump (CPU), and for the six scenes recorded in tests/golden/ref_parity_render.npz (proj12_backfaceTest, proj3, proj13, proj7, proj10, proj2) it
pins the oracle's sequential / libm render of the region (330, 260, 430, 330) at 2 spp, GI depth 3, to the unmodified reference's samples, bit
for bit (test_integrator_on_shipped_scenes).  Here the HIP path renders the same flat blobs and is held to the oracle in its default (keyed,
device-math) mode — the mode every other GPU test uses: primary hits of every pixel, per-sample radiance on that same region and on one that
holds the horizon of the scene's largest plane, and shadow rays towards every light that casts one.

These files hold what no authored scene has together: a plane scaled by 1000 under a checker scaled 0.003 (proj7, proj10), a transformed background
texture beside an untransformed environment texture, <reflection> / <refraction glossiness> attributes, three and four sized point lights, and
null-object nodes where a mesh file is absent (meshes do not ship with the reference)."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, same_bits

pytestmark = pytest.mark.gpu

SHIPPED_ROOT = os.path.join(GOLDEN, "shipped")  # the reference resolves asset paths against its working directory: Resource/...
REGION = (330, 260, 430, 330)                   # the region tests/golden/make_ref_parity.py recorded from the reference
LIGHT_AMBIENT, LIGHT_DIRECT, LIGHT_POINT = 0, 1, 2
OBJ_PLANE = 2


def _shipped_xmls():
    return sorted(os.path.relpath(f, SHIPPED_ROOT) for f in glob.glob(os.path.join(SHIPPED_ROOT, "Resource", "**", "*.xml"), recursive=True))


def test_all_19_shipped_scenes_are_rendered():
    assert len(_shipped_xmls()) == 19


def _horizon_region(fv, node, W, H):
    """A 100 x 24 region on the longest horizontal edge of the largest plane's pixels — its horizon, or where another object cuts it off.
    None when the scene has no plane, or its largest plane is out of view or fills the frame."""
    planes = [(float(np.linalg.norm(np.array(list(n.xf.tm), np.float64))), k) for k, n in enumerate(fv.nodes) if n.obj_type == OBJ_PLANE]
    if not planes:
        return None
    mask = node.reshape(H, W) == max(planes)[1]
    edge = mask[1:] != mask[:-1]  # edge[y, x]: rows y and y + 1 differ
    if not edge.any():
        return None
    y = int(np.argmax(edge.sum(axis=1)))
    x = int(np.median(np.where(edge[y])[0]))
    x0, y0 = min(max(x - 50, 0), W - 100), min(max(y + 1 - 12, 0), H - 24)
    reg = (x0, y0, x0 + 100, y0 + 24)
    inside = mask[reg[1]:reg[3], reg[0]:reg[2]]
    assert inside.any() and not inside.all()  # the edge runs through the region
    return reg


@pytest.mark.parametrize("rel", _shipped_xmls())
def test_shipped_scene_on_the_gpu(rel, B, O):
    if B.device_count() < 1:
        pytest.fail("no HIP device: the render path has no CPU fallback, GPU tests cannot run here")
    cwd = os.getcwd()
    os.chdir(SHIPPED_ROOT)
    try:
        sc = B.Scene(rel)
    finally:
        os.chdir(cwd)
    fv, blob = sc.flat_view(), sc.flat_bytes()
    W, H = sc.width, sc.height
    assert REGION[2] <= W and REGION[3] <= H
    # primary hits of every pixel, front side and both sides
    o, d = O.primary_rays(fv)
    for side in (1, 3):
        h, r = sc.trace_closest(o, d, side), O.trace_closest(blob, o, d, side)
        assert np.array_equal(h["node"], r["node"]) and np.array_equal(h["prim"], r["prim"]) and same_bits(h["t"], r["t"])
        hit = r["node"] >= 0
        assert np.array_equal(h["front"][hit], r["front"][hit])
        if side == 1:
            front = r
    # per-sample radiance: the region the reference was recorded on, and the largest plane's horizon (the frame's top-left block where there is none)
    horizon = _horizon_region(fv, front["node"], W, H)
    for region in (REGION, horizon or (0, 0, 100, 24)):
        gs, st = sc.render_samples(B.default_opts(spp=2, gi_bounces=3), *region)
        ro = O.render(blob, W, H, 2, gi=3, region=region, threads=16)
        assert same_bits(gs, ro["samples"])
        assert st.camera_samples == W * H * 2
    # shadow rays from the hit points towards each light that casts shadows (GenLight::Shadow: a point light's segment, a direct light's ray)
    hit = front["node"] >= 0
    P = front["attrs"][hit][::7, 1:4]
    for light in fv.lights:
        if light.type == LIGHT_AMBIENT or not len(P):
            continue
        L = np.array(list(light.vec), np.float32)
        sd, tmax = ((L[None] - P).astype(np.float32), 1.0) if light.type == LIGHT_POINT else (np.broadcast_to(-L, P.shape).astype(np.float32), 1e30)
        assert np.array_equal(sc.trace_shadow(P, sd, tmax), O.trace_shadow(blob, P, sd, tmax))
    sc.close()
