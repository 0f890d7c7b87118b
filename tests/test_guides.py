"""Sampled guide images (bhrt_guides): z, normal, albedo and coverage formed by the render's own camera samples and averaged
per pixel, so that the denoiser's guides follow the jitter and the lens as the colour image does.

What the images must hold is restated here in numpy float32 from per-sample values the code under test does not produce:
  * the rays are bhrt_camera_rays' (pinned to the restated camera model by tests/test_lens.py), or that model itself in the CPU tests;
  * the hits and their t are the oracle's (oracle_lib.trace_closest);
  * a sample's N and kd are the oracle's first-hit images of a 1 x 1 frame whose camera is that sample's ray: `pos` = the sample's origin and
    `top_left` = its point on the image plane, so the oracle's pixel (0, 0) forms ((T + 0 dd_x) - 0 dd_y) - pos = the sample's direction.
The sums run over the samples that hit, in sample order, starting from the first one's value (include/bhrt.h); equal bits are required."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits
from test_lens import lens_rays_ref

f32 = np.float32
BIG = f32(1.0e30)
SEED = 3
SCENE_NAMES = ["lens_spheres", "lens_mesh_small", "c4_textured", "facemtl_room"]
# sky, silhouettes of the objects and ground in both lens scenes (96 x 72): 48 x 32 pixels
REGION = (8, 16, 56, 48)
SMALL = (20, 24, 36, 32)  # 16 x 8 of it, for the counts beyond one workgroup's samples


@pytest.fixture(scope="module")
def scene(B):
    """Private scene handles (set_face_materials changes a scene), freed when the module is done."""
    opened = {}

    def _load(name, face_materials=False):
        key = (name, face_materials)
        if key not in opened:
            opened[key] = B.Scene(os.path.join(SCENES, name + ".xml"))
            if face_materials:
                opened[key].set_face_materials(True)
        return opened[key]
    yield _load
    for sc in opened.values():
        sc.close()


def region_pixels(region):
    x0, y0, x1, y1 = region
    return np.array([(i, j) for j in range(y0, y1) for i in range(x0, x1)], np.int64)


def fold(values, hit):
    """(pixels, n, c) float32 values, (pixels, n) bool -> the float32 sum over the samples that hit, in sample order, starting from the first
    one's value (0 where none hits)."""
    values = np.ascontiguousarray(values, f32)
    acc = np.zeros((values.shape[0], values.shape[2]), f32)
    seen = np.zeros(values.shape[0], bool)
    for s in range(values.shape[1]):
        h = hit[:, s]
        start = h & ~seen
        go_on = h & seen
        acc[start] = values[start, s]
        acc[go_on] = acc[go_on] + values[go_on, s]
        seen |= h
    assert acc.dtype == f32
    return acc


def z_and_coverage(O, blob, o, d):
    """The restated z and coverage of pixels with rays o, d (pixels, n, 3), and the hit counts."""
    n = o.shape[1]
    h = O.trace_closest(blob, o.reshape(-1, 3), d.reshape(-1, 3), 1)
    hit = (h["node"] >= 0).reshape(-1, n)
    k = hit.sum(axis=1)
    st = fold(h["t"].reshape(-1, n, 1), hit)[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(k > 0, st / k.astype(f32), BIG).astype(f32)
    cov = (k.astype(f32) / f32(n)).astype(f32)
    return z, cov, k


def assert_mixed(k, n):
    """The precondition of the z / coverage test: pixels that partly hit, that miss and that hit with every sample."""
    partial, none, full = int(((k > 0) & (k < n)).sum()), int((k == 0).sum()), int((k == n).sum())
    print(f"n = {n}: {partial} pixels hit partly, {none} miss, {full} hit with every sample")
    assert partial >= 1 and none >= 1 and full >= 1


def crop(img, region):
    x0, y0, x1, y1 = region
    return img[y0:y1, x0:x1].reshape((y1 - y0) * (x1 - x0), -1)


# ---- per-sample N and kd from the oracle: a 1 x 1 frame whose camera is the sample's ray ------------------------------------------------------
def sample_blob(blob, o, T):
    from bhraytracer_amd.flat import Camera, Header
    b = bytearray(blob)
    base = Header.camera.offset
    b[base + Camera.pos.offset:base + Camera.pos.offset + 12] = np.asarray(o, f32).tobytes()
    b[base + Camera.top_left.offset:base + Camera.top_left.offset + 12] = np.asarray(T, f32).tobytes()
    b[base + Camera.width.offset:base + Camera.width.offset + 8] = np.asarray([1, 1], np.int32).tobytes()
    return bytes(b)


def oracle_direction(cam, o, T):
    """What the oracle's first-hit image forms for pixel (0, 0) of the patched camera (bhrt_oracle.cpp: FirstHitT)."""
    ddx, ddy = np.array(list(cam.dd_x), f32), np.array(list(cam.dd_y), f32)
    return ((T + f32(0) * ddx) - f32(0) * ddy) - o


def submaterial_blobs(sc):
    """Face materials on: the blob patched to sub-material g for every g, and the face ranges (tests/test_face_materials.py's recipe)."""
    from bhraytracer_amd import flat
    (mm,) = [m for m in range(sc.info.n_materials) if sc.submaterial_count(m) > 0]
    off = sc.flat_view().header.off_materials + mm * C.sizeof(flat.Material)
    blobs, face_end = [], []
    for g in range(sc.submaterial_count(mm)):
        rec, end = sc.submaterial(mm, g)
        b = bytearray(sc.flat_bytes())
        b[off:off + C.sizeof(flat.Material)] = bytes(rec)
        blobs.append(bytes(b))
        face_end.append(end)
    return mm, blobs, np.array(face_end, np.int64)


class Pairs:
    """At most 40 (pixel, sample) pairs of a scene: whole pixels at 5 samples, chosen from the oracle's hits alone."""

    def __init__(self, O, sc, name, lens, face_materials):
        self.n = 5
        cam = sc.flat_view().header.camera
        self.cam = cam
        W, H = cam.width, cam.height
        blob = sc.flat_bytes()
        o, d, T = lens_rays_ref(O, cam, self.n, seed=SEED, jitter=1, lens_r=cam.dof if lens else 0.0)
        h = O.trace_closest(blob, o.reshape(-1, 3), d.reshape(-1, 3), 1)
        node, prim = h["node"].reshape(-1, self.n), h["prim"].reshape(-1, self.n)
        k = (node >= 0).sum(axis=1)
        mats = sc.flat_view().materials
        node_mtl = np.array([nd.material for nd in sc.flat_view().nodes] + [-1], np.int32)
        self.group = np.zeros_like(node)
        self.blobs = [blob]
        chosen = []

        def take(mask, count, what):
            found = [p for p in np.flatnonzero(mask) if p not in chosen][:count]
            assert len(found) == count, f"{name}: no pixel for: {what}"
            chosen.extend(int(p) for p in found)

        if name == "lens_spheres":
            take((k > 0) & (k < self.n), 3, "a silhouette against the sky")
            take(np.array([len(set(r.tolist())) > 1 for r in node]) & (k == self.n), 2, "an edge between two objects")
            take(k == self.n, 2, "an interior pixel")
            take(k == 0, 1, "a pixel of sky")
        elif name == "c4_textured":
            textured_plane = [i for i, nd in enumerate(sc.flat_view().nodes) if nd.obj_type == 2 and mats[nd.material].diffuse.map >= 0]
            assert textured_plane, "c4_textured has no textured plane"
            on_plane = np.isin(node, textured_plane)
            take(on_plane.all(axis=1), 3, "the textured plane")  # the duvw path
            take(on_plane.any(axis=1) & ~on_plane.all(axis=1), 2, "the textured plane's edge")
            take((node_mtl[node] >= 0).all(axis=1) & ~on_plane.any(axis=1) & np.array([len(set(r.tolist())) == 1 for r in node]), 3, "another textured object")
        else:
            assert face_materials
            mm, self.blobs, face_end = submaterial_blobs(sc)
            raw = np.searchsorted(face_end, prim, side="right")
            g = np.where((prim >= 0) & (raw < len(face_end)), raw, 0)
            self.group = np.where(node_mtl[node] == mm, g, 0)  # off the mesh every patched blob is the same
            on_mesh = node_mtl[node] == mm
            for grp in range(len(face_end)):
                take((on_mesh & (self.group == grp)).all(axis=1), 2, f"sub-material {grp}")
            take(np.array([on_mesh[p].all() and len(set(self.group[p].tolist())) > 1 for p in range(len(node))]), 1, "two sub-materials in one pixel")
            take(~on_mesh.any(axis=1), 1, "the room")
            self.groups_seen = sorted(set(self.group[chosen][on_mesh[chosen]].tolist()))
        assert len(chosen) * self.n <= 40
        self.pix = np.array(chosen, np.int64)
        self.ij = np.stack([self.pix % W, self.pix // W], axis=1)
        self.o, self.d, self.T = o[self.pix], d[self.pix], T[self.pix]
        self.group = self.group[self.pix]
        # a pair is usable when the oracle's pixel (0, 0) of the patched camera is exactly the sample's ray
        self.usable = np.array([[same_bits(oracle_direction(cam, self.o[p, s], self.T[p, s]), self.d[p, s]) for s in range(self.n)] for p in range(len(self.pix))])

    def expected(self, O, o=None, d=None):
        """(normal, albedo, keep): the restated images at the chosen pixels whose pairs are all usable.  o, d: the rays the device formed, which
        must be the restated model's."""
        if o is not None:
            assert same_bits(o, self.o) and same_bits(d, self.d)
        keep = self.usable.all(axis=1)
        P = len(self.pix)
        N, kd, hit = np.zeros((P, self.n, 3), f32), np.zeros((P, self.n, 3), f32), np.zeros((P, self.n), bool)
        for p in np.flatnonzero(keep):
            for s in range(self.n):
                z, nrm, alb = O.first_hit(sample_blob(self.blobs[self.group[p, s]], self.o[p, s], self.T[p, s]), 1, 1)
                hit[p, s] = z[0] != BIG
                N[p, s], kd[p, s] = nrm[0], alb[0]
        return (fold(N, hit) / f32(self.n)).astype(f32), (fold(kd, hit) / f32(self.n)).astype(f32), keep


PAIR_CASES = [("lens_spheres", 1, False), ("c4_textured", 0, False), ("facemtl_room", 0, True)]


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------------
def test_guides_are_declared_and_exported(B):
    assert hasattr(B.lib(), "bhrt_guides") and hasattr(B.lib(), "bhrt_guides_dev")
    assert "bhrt_guides" in B.EXPORTS and "bhrt_guides_dev" in B.EXPORTS


@pytest.mark.parametrize("bad,what", [(dict(spp=0), "spp"), (dict(spp=-3), "spp"), (dict(spp=65536), "spp"), (dict(lens=2), "lens"), (dict(lens=-1), "lens"),
                                      (dict(rank=1), "rank"), (dict(rank=3, world_size=3), "rank"), (dict(rank=-1, world_size=2), "rank")])
def test_bad_options_are_refused_before_the_device(B, scene, bad, what):
    """BHRT_ERR_ARG on a machine with a device and on one without: the options are checked first."""
    sc = scene("lens_spheres")
    opts = B.default_opts(**{**dict(spp=4), **bad})
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*" + what):
        sc.guides(opts)
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*" + what):
        sc.guides_dev(opts, d_z=0)


def test_lens_on_a_scene_with_a_bad_dof_is_refused_before_the_device(B, tmp_path):
    text = open(os.path.join(SCENES, "lens_spheres.xml")).read().replace('<dof value="1.5"/>', '<dof value="-1"/>')
    assert 'value="-1"' in text
    path = tmp_path / "baddof.xml"
    path.write_text(text)
    sc = B.Scene(str(path))
    try:
        assert sc.flat_view().header.camera.dof < 0
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*dof"):
            sc.guides(B.default_opts(spp=4, lens=1))
    finally:
        sc.close()


def test_guides_need_a_device_and_never_fall_back(B):
    sc = B.Scene(os.path.join(SCENES, "lens_spheres.xml"))
    try:
        if B.device_count() > 0:
            g = sc.guides(B.default_opts(spp=2, lens=1))
            assert sorted(g) == ["albedo", "coverage", "normal", "z"] and g["normal"].shape == (sc.height, sc.width, 3)
        else:
            with pytest.raises(B.BhrtError, match=r"bhrt error 4"):
                sc.guides(B.default_opts(spp=2, lens=1))
    finally:
        sc.close()


def test_fold_starts_from_the_first_hit_and_keeps_the_order():
    v = np.array([[[1e8], [1.0], [-1e8], [1.0]], [[-0.0], [5.0], [-0.0], [7.0]]], f32)
    hit = np.array([[True, True, True, True], [True, False, True, False]])
    out = fold(v, hit)
    assert out[0, 0] == f32(1.0)                      # ((1e8 + 1) - 1e8) + 1 in float32: the 1 in front is lost, the one behind is not
    assert np.signbit(out[1, 0]) and out[1, 0] == 0   # -0 + -0: no +0 in front of the sum
    assert fold(v, np.zeros((2, 4), bool)).tolist() == [[0.0], [0.0]]


@pytest.mark.parametrize("lens", [0, 1])
@pytest.mark.parametrize("name", ["lens_spheres", "lens_mesh_small"])
def test_the_region_mixes_hits_and_misses(B, O, scene, name, lens):
    """The precondition of the z / coverage test, with the oracle and the restated camera alone."""
    sc = scene(name)
    cam = sc.flat_view().header.camera
    for n in (5, 67):
        o, d, _ = lens_rays_ref(O, cam, n, seed=SEED, jitter=1, lens_r=cam.dof if lens else 0.0, pixels=region_pixels(REGION))
        assert_mixed(z_and_coverage(O, sc.flat_bytes(), o, d)[2], n)


@pytest.mark.parametrize("name,lens,fm", PAIR_CASES)
def test_the_chosen_pairs_are_the_oracles_rays(B, O, scene, name, lens, fm):
    """The precondition of the normal / albedo test, with the oracle alone: the pairs cover what they must, and for at least three quarters
    of them the oracle's patched 1 x 1 camera forms exactly the sample's direction."""
    P = Pairs(O, scene(name, fm), name, lens, fm)
    print(f"{name}: {P.usable.size} pairs at pixels {P.ij.tolist()}, {int((~P.usable).sum())} not usable")
    assert P.usable.size <= 40 and (~P.usable).sum() * 4 <= P.usable.size
    assert P.usable.all(axis=1).sum() * 4 >= 3 * len(P.pix)
    if fm:
        assert len(P.groups_seen) >= 2
    normal, albedo, keep = P.expected(O)
    assert np.isfinite(normal).all() and np.isfinite(albedo).all()
    if name == "lens_spheres":  # a silhouette pixel carries a shorter normal than an interior one
        length = np.sqrt((normal.astype(np.float64) ** 2).sum(axis=1))
        assert length[keep].min() < 0.9 * length[keep].max()
    if name == "c4_textured":   # the texture shows: the albedo varies over the plane's pixels
        assert len({tuple(a) for a in albedo[keep][:3].tolist()}) > 1


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fm", [False, True])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_one_unjittered_pinhole_sample_is_the_first_hit(B, scene, name, fm):
    sc = scene(name, fm)
    z, n, a = sc.first_hit()
    g = sc.guides(B.default_opts(spp=1, jitter=0, lens=0, seed=SEED))
    assert same_bits(g["z"], z) and same_bits(g["normal"], n) and same_bits(g["albedo"], a)
    assert np.array_equal(g["coverage"], (z != BIG).astype(f32))
    assert (z != BIG).any() and np.abs(a).sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 67])
@pytest.mark.parametrize("lens", [0, 1])
@pytest.mark.parametrize("name", ["lens_spheres", "lens_mesh_small"])
def test_z_and_coverage_are_the_oracles_hits_summed_in_order(B, O, scene, name, lens, n):
    sc = scene(name)
    opts = B.default_opts(spp=n, seed=SEED, jitter=1, lens=lens)
    o, d = sc.camera_rays(opts, REGION)
    z, cov, k = z_and_coverage(O, sc.flat_bytes(), o, d)
    assert_mixed(k, n)
    g = sc.guides(opts, want=("z", "coverage"))
    assert same_bits(crop(g["coverage"], REGION)[:, 0], cov)
    assert same_bits(crop(g["z"], REGION)[:, 0], z)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [256, 300])
def test_z_and_coverage_beyond_one_workgroups_samples(B, O, scene, n):
    """256 samples fill a workgroup, 300 take a second chunk and the running sums between them."""
    sc = scene("lens_mesh_small")
    opts = B.default_opts(spp=n, seed=SEED, jitter=1, lens=1)
    o, d = sc.camera_rays(opts, SMALL)
    z, cov, k = z_and_coverage(O, sc.flat_bytes(), o, d)
    assert_mixed(k, n)
    g = sc.guides(opts, want=("z", "coverage"))
    assert same_bits(crop(g["coverage"], SMALL)[:, 0], cov) and same_bits(crop(g["z"], SMALL)[:, 0], z)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lens,fm", PAIR_CASES)
def test_normal_and_albedo_are_the_oracles_per_sample_values_summed_in_order(B, O, scene, name, lens, fm):
    sc = scene(name, fm)
    P = Pairs(O, sc, name, lens, fm)
    opts = B.default_opts(spp=P.n, seed=SEED, jitter=1, lens=lens)
    o, d = sc.camera_rays(opts)
    normal, albedo, keep = P.expected(O, o[P.pix], d[P.pix])
    assert keep.sum() * 4 >= 3 * len(keep)
    g = sc.guides(opts)
    got_n, got_a = g["normal"][P.ij[:, 1], P.ij[:, 0]], g["albedo"][P.ij[:, 1], P.ij[:, 0]]
    print(f"{name}: normal {got_n[keep].tolist()} albedo {got_a[keep].tolist()}")
    assert same_bits(got_n[keep], normal[keep])
    assert same_bits(got_a[keep], albedo[keep])
    if fm:  # the switch off: the mesh's pixels show sub-material 0 alone
        off = B.Scene(os.path.join(SCENES, name + ".xml"))
        try:
            assert not same_bits(off.guides(opts, want=("albedo",))["albedo"], g["albedo"])
        finally:
            off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 67])
def test_guides_do_not_depend_on_ranks_tiles_or_pass_size(B, scene, n):
    sc = scene("lens_mesh_small")
    kw = dict(spp=n, seed=SEED, jitter=1, lens=1)
    base = sc.guides(B.default_opts(**kw))
    assert 0 < base["coverage"].mean() < 1
    # three logical ranks, tile 8: each leaves the others' tiles alone, the union is the frame
    H, W = sc.height, sc.width
    sentinel = f32(-7.5)
    union = {k: np.full_like(v, sentinel) for k, v in base.items()}
    ty, tx = np.arange(H)[:, None] // 8, np.arange(W)[None, :] // 8
    owner = (ty * ((W + 7) // 8) + tx) % 3
    for r in range(3):
        mine = {k: np.full_like(v, sentinel) for k, v in base.items()}
        sc.guides(B.default_opts(rank=r, world_size=3, tile_size=8, **kw), into=mine)
        for k in base:
            assert same_bits(mine[k][owner == r], base[k][owner == r]), (k, r)
            assert (mine[k][owner != r] == sentinel).all(), (k, r)
        sc.guides(B.default_opts(rank=r, world_size=3, tile_size=8, **kw), into=union)
    for k in base:
        assert same_bits(union[k], base[k]), k
    # few samples in flight: chunks of 3 samples and of 64, passes of a few pixels, running sums between the chunks
    for spp_pass in (3, 64, 1000):
        small = sc.guides(B.default_opts(samples_per_pass=spp_pass, **kw))
        for k in base:
            assert same_bits(small[k], base[k]), (k, spp_pass)
    # NULL for any subset of the outputs
    names = list(base)
    for mask in range(1, 15):
        want = tuple(k for b, k in enumerate(names) if mask >> b & 1)
        part = sc.guides(B.default_opts(**kw), want=want)
        assert sorted(part) == sorted(want)
        for k in want:
            assert same_bits(part[k], base[k]), (k, want)


@pytest.mark.gpu
def test_guides_dev_on_a_stream(B, scene):
    import torch
    sc = scene("lens_spheres")
    opts = B.default_opts(spp=67, seed=SEED, lens=1, samples_per_pass=4096)
    base = sc.guides(opts)
    dev = torch.device("cuda:0")
    H, W = sc.height, sc.width
    t = {"z": torch.zeros((H, W), device=dev), "normal": torch.zeros((H, W, 3), device=dev), "albedo": torch.zeros((H, W, 3), device=dev),
         "coverage": torch.zeros((H, W), device=dev)}
    s = torch.cuda.Stream(dev)
    sc.guides_dev(opts, t["z"].data_ptr(), t["normal"].data_ptr(), t["albedo"].data_ptr(), t["coverage"].data_ptr(), s.cuda_stream)
    s.synchronize()
    for k in base:
        assert same_bits(t[k].cpu().numpy(), base[k]), k


@pytest.mark.gpu
def test_denoiser_fed_one_pinhole_sample_is_the_denoiser_with_its_own_guides(B, scene):
    sc = scene("lens_spheres")
    _, rad, var = sc.render_var(B.default_opts(spp=4, seed=5, lens=1))
    o = B.default_denoise_opts()
    own, own_rgb = sc.denoise(o, rad, var)
    g = sc.guides(B.default_opts(spp=1, jitter=0))
    fed, fed_rgb = sc.denoise(o, rad, var, g["z"], g["normal"], g["albedo"])
    assert same_bits(fed, own) and np.array_equal(fed_rgb, own_rgb)
    s = sc.guides(B.default_opts(spp=8, seed=5, lens=1))
    out, _ = sc.denoise(o, rad, var, s["z"], s["normal"], s["albedo"])
    assert not same_bits(out, own)


@pytest.mark.gpu
def test_sampled_guides_against_the_denoisers_own_on_a_lens_frame(B, scene):
    """lens_spheres at 8 spp through the lens, denoised with the denoiser's own (pinhole) guides and with sampled guides at 8 spp, both against
    a 2048-spp frame of another seed, by mean squared error on linear radiance.  Measured on an MI355X (the figures this test prints):
        noisy 0.003329, the denoiser's own guides 0.000944, sampled guides 0.003055
    The sampled guides do NOT lower the error with the filter as it stands, so nothing is asserted about the order of the two: the filter divides
    the colour by the albedo guide, and a partly covered pixel's averaged albedo is small while its colour holds the background (DESIGN.md 16
    has the figures per guide image and per guide sample count).  The test keeps the comparison running and its figures in the log."""
    sc = scene("lens_spheres")
    own = B.Scene(os.path.join(SCENES, "lens_spheres.xml"))  # the reference frame's workspace goes with its handle
    try:
        _, ref, _ = own.render(B.default_opts(spp=2048, seed=77, lens=1))
    finally:
        own.close()
    opts = B.default_opts(spp=8, seed=1, lens=1)
    _, rad, var = sc.render_var(opts)
    o = B.default_denoise_opts()
    pin, _ = sc.denoise(o, rad, var)
    g = sc.guides(opts)
    smp, _ = sc.denoise(o, rad, var, g["z"], g["normal"], g["albedo"])
    mse = lambda x, m=None: float(np.mean(((x.astype(np.float64) - ref) ** 2)[m] if m is not None else (x.astype(np.float64) - ref) ** 2))  # noqa: E731
    blurred = (g["coverage"] > 0) & (g["coverage"] < 1)
    for dy in (-1, 0, 1):  # and their neighbours: where the two sets of guides differ most
        for dx in (-1, 0, 1):
            blurred |= np.roll(np.roll((g["coverage"] > 0) & (g["coverage"] < 1), dy, 0), dx, 1)
    print(f"MSE against 2048 spp: noisy {mse(rad):.4g}, own guides {mse(pin):.4g}, sampled guides {mse(smp):.4g}; "
          f"silhouette pixels ({blurred.mean():.1%}): noisy {mse(rad, blurred):.4g}, own {mse(pin, blurred):.4g}, sampled {mse(smp, blurred):.4g}")
    assert np.isfinite(smp).all() and np.isfinite(pin).all() and mse(pin) > 0 and mse(smp) > 0
    assert not same_bits(smp, pin)
