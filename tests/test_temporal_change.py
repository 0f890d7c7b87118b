"""The temporal change test: bhrt_temporal_change shortens a reprojected pixel's history length where history and current frame
differ, over a window on the pixel's own surface, by more than the noise both variances predict (csrc/temporal.hip states it as stage 2C), and
bhrt_temporal_set_change places it between reprojection and accumulation of a temporal session.

temporal_change_ref restates the stage in numpy, float32, in the kernel's tap and sum order, vectorised over pixels: one tap of every pixel at
a time.  A tap that is invalid enters both sums as + 0, which is what skipping it does (a sum that starts at +0 never becomes -0)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, have_gpu
from test_denoise import _synthetic_xml, _tap
from test_reproject import BIG, scene  # noqa: F401
from test_temporal_session import BALL_MOVE, FRAMES, SEED, XML, _kept, _pose, _same

f32 = np.float32
NAN, INF = float("nan"), float("inf")
ERR_ARG = 3
SYMBOLS = ("bhrt_temporal_change", "bhrt_temporal_change_dev", "bhrt_temporal_set_change")
KR, KG, KB = f32(0.2126), f32(0.7152), f32(0.0722)


def lum(x):
    return ((KR * x[..., 0] + KG * x[..., 1]) + KB * x[..., 2]).astype(f32)


def vlum(x):
    return (((KR * KR) * x[..., 0] + (KG * KG) * x[..., 1]) + (KB * KB) * x[..., 2]).astype(f32)


def temporal_change_ref(c, v, h, hv, l, z, n, radius=3, sigma_lo=1.5, sigma_hi=3.0, depth_tolerance=0.01, normal_threshold=0.99):
    """Stage 2C of csrc/temporal.hip on (H, W[, 3]) arrays.  Returns (out_length, change)."""
    c, v, h, hv, l, z, n = (np.asarray(k, f32) for k in (c, v, h, hv, l, z, n))
    H, W = z.shape
    R, lo, hi, tol, thr = int(radius), f32(sigma_lo), f32(sigma_hi), f32(depth_tolerance), f32(normal_threshold)
    with np.errstate(all="ignore"):
        d = (lum(c) - lum(h)).astype(f32)
        w = (vlum(v) + vlum(hv)).astype(f32)
        has = l > 0
        miss = z >= BIG
        tz = (tol * z).astype(f32)
        s, sw = np.zeros((H, W), f32), np.zeros((H, W), f32)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                dq, inside = _tap(d, dx, dy)
                wq, _ = _tap(w, dx, dy)
                if dx == 0 and dy == 0:
                    ok = np.ones((H, W), bool)
                else:
                    hq, _ = _tap(has, dx, dy)
                    zq, _ = _tap(z, dx, dy)
                    nq, _ = _tap(n, dx, dy)
                    r = np.sqrt(f32(dx * dx + dy * dy))
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    same = (zq < BIG) & (np.abs(zq - z) <= tz * r) & (dot >= thr)
                    ok = inside & hq & np.where(miss, zq >= BIG, same)
                s = (s + np.where(ok, dq, f32(0))).astype(f32)
                sw = (sw + np.where(ok, wq, f32(0))).astype(f32)
        a = np.abs(s)
        x = np.where(sw > 0, a / np.sqrt(sw), np.where((sw <= 0) & (a > 0), f32(INF), f32(0))).astype(f32)
        lam = np.where(~(x > lo), f32(0), np.where(x >= hi, f32(1), (x - lo) / (hi - lo))).astype(f32)
        lam = np.where(has, lam, f32(0)).astype(f32)
        out = np.where(has, l * (f32(1) - lam), l).astype(f32)
    return out, lam


def flat_guides(H, W, depth=3.0):
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    return np.full((H, W), depth, f32), n


# the constant block: d = 0.5 and w = 0.25 at every pixel, exactly.  L((g, g, g)) = g for g a power of two because (0.2126f + 0.7152f) + 0.0722f
# is 1 in float32; vL((0, 0, t)) = fl((0.0722f 0.0722f) t) is 0.25 for t = fl(0.25 / (0.0722f 0.0722f)).  Both are asserted below.
BLOCK_C = f32(0.5)
BLOCK_T = f32(0.25) / (KB * KB)


def block_bound(R):
    """x of a pixel whose whole (2R + 1)^2 window lies in the block: s = k / 2 and sw = k / 4 are exact (k <= 81), sqrt(k / 4) = (2R + 1) / 2, so
    x = (k / 2) / ((2R + 1) / 2) = 2R + 1, exactly."""
    return float(2 * R + 1)


def crafted(rng, W, H):
    """A frame of W x H: depth steps, a normal flip, normals near the threshold, misses beside hits, NaN in z; lengths 0, < 0 and NaN among
    positive ones; variances that put x on both sides of the thresholds; a region without any variance where h == c and one where h != c;
    a NaN radiance and a NaN variance; and, where it fits, the constant block.  Returns (c, v, h, hv, l, z, n, block) with block the slice pair
    of the constant block or None."""
    yy, xx = np.mgrid[0:H, 0:W].astype(f32)
    z = (f32(3) + f32(0.01) * xx + f32(0.02) * yy).astype(f32)
    z[:, W // 2:] += f32(2)                                                     # a depth step
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    n[(xx + yy) > f32(0.6) * (W + H)] = np.float32([0.6, 0, 0.8])               # a normal flip
    n = (n + rng.normal(0, 0.03, (H, W, 3))).astype(f32)                        # raw dots on both sides of 0.99
    u = rng.uniform(size=(H, W))
    miss = (u < 0.06) | ((yy < 3) & (xx > W // 3))                              # a band of misses beside hits, and single ones
    z[miss] = BIG
    z[miss & (u < 0.02)] = INF
    n[miss] = 0
    z[(u > 0.10) & (u < 0.12)] = NAN
    c = rng.gamma(4.0, 0.25, (H, W, 3)).astype(f32)
    h = (c + rng.normal(0, 0.05, (H, W, 3)) + f32(0.03)).astype(f32)            # history: the same light, a little noise and a small common offset
    v = rng.gamma(2.0, 0.002, (H, W, 3)).astype(f32)
    hv = rng.gamma(2.0, 0.001, (H, W, 3)).astype(f32)
    l = rng.randint(1, 17, (H, W)).astype(f32)
    w = rng.uniform(size=(H, W))
    l[w < 0.05], l[(w > 0.05) & (w < 0.1)], l[(w > 0.1) & (w < 0.15)] = 0, -1, NAN
    lower = yy >= f32(0.75) * H                                                 # no variance at all: x is 0 where h == c, +inf where it is not
    v[lower] = 0
    hv[lower] = 0
    h[lower & (xx < W // 2)] = c[lower & (xx < W // 2)]
    block = None
    if W >= 17 and H >= 17:
        block = (slice(4, 15), slice(3, 14))                                   # 11 x 11: at R = 4 the 3 x 3 pixels in its middle see nothing else
        z[block], n[block], l[block] = 50.0, np.float32([0, 0, 1]), 4.0
        c[block], h[block] = BLOCK_C, 0
        v[block], hv[block] = np.float32([0, 0, BLOCK_T]), 0
    if W * H > 100:
        c[H // 2, 1, 1] = NAN                                                   # a NaN radiance in one tap
        v[H // 2 + 2, W - 2, 0] = NAN                                           # and a NaN variance in another
        l[H // 2, 1] = l[H // 2 + 2, W - 2] = 3
    return c, v, h, hv, l, z, n, block


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_symbols_exported_declared_and_wrapped(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in SYMBOLS:
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr), s
    s = "bhrt_default_change_opts"
    assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bvoid %s\(" % s, hdr) and "DESIGN.md 24" in hdr
    for w in ("temporal_change", "temporal_change_dev", "temporal_set_change"):
        assert callable(getattr(B.Scene, w))
    for k, name in ((11, "CHANGE"), (12, "USED_LENGTH")):
        assert re.search(r"\bBHRT_TEMPORAL_IMG_%s = %d\b" % (name, k), hdr) and getattr(B, "TEMPORAL_IMG_" + name) == k
    head = open(os.path.join(ROOT, "bhraytracer_amd", "csrc", "temporal.hip")).read().split("#include")[0]
    assert "2C. TEMPORAL CHANGE TEST" in head
    lo, hi = (float(re.search(r"#define BHRT_CHANGE_SIGMA_%s ([0-9.]+)f" % k, hdr).group(1)) for k in ("LO", "HI"))
    assert (lo, hi) == (B.CHANGE_SIGMA_LO, B.CHANGE_SIGMA_HI) and 0 <= lo <= hi


def test_struct_sizes_and_defaults(B):
    assert C.sizeof(B.ChangeOpts) == 32
    assert C.sizeof(B.TemporalSessionOpts) == 4 * 32 + 8 * 4 and C.sizeof(B.TemporalProgress) == 40            # the session structs keep their sizes
    buf = (C.c_uint8 * 64)(*([0xAB] * 64))
    B.lib().bhrt_default_change_opts(C.byref(buf))
    assert bytes(buf[20:32]) == bytes(12) and bytes(buf[32:]) == b"\xab" * 32                                # exactly 32 bytes, reserved[3] the zero tail
    o = B.default_change_opts()
    assert bytes(o) == bytes(buf[:32])
    assert o.radius == 3 and f32(o.sigma_lo) == f32(B.CHANGE_SIGMA_LO) and f32(o.sigma_hi) == f32(B.CHANGE_SIGMA_HI)
    sv = B.default_spatial_variance_opts()
    assert f32(o.depth_tolerance) == f32(sv.depth_tolerance) and f32(o.normal_threshold) == f32(sv.normal_threshold)
    assert B.default_change_opts(radius=2, sigma_lo=0.0).radius == 2


def test_bad_arguments_are_refused_before_the_device(B, scene):
    """Every BHRT_ERR_ARG case (error 3) on a loaded scene that was never uploaded: the checks come before any device is touched."""
    sc = scene("c1_sphere_plane")
    W, H = sc.width, sc.height
    l, n3 = np.ones((H, W), f32), np.ones((H, W, 3), f32)
    ok, D = B.default_change_opts(), B.default_change_opts
    bad_opts = [None, D(radius=0), D(radius=5), D(radius=-1), D(sigma_lo=-0.5), D(sigma_lo=NAN), D(sigma_lo=INF, sigma_hi=INF), D(sigma_hi=NAN), D(sigma_hi=INF),
                D(sigma_lo=2.0, sigma_hi=1.0), D(depth_tolerance=-0.01), D(depth_tolerance=INF), D(depth_tolerance=NAN), D(normal_threshold=NAN)]
    for o in bad_opts:
        with pytest.raises(B.BhrtError, match="bhrt error 3"):
            sc.temporal_change(o, n3, n3, n3, n3, l, l, n3)
    for k in range(5):                                                                               # each required input image NULL
        a = [n3, n3, n3, n3, l]
        a[k] = None
        with pytest.raises(B.BhrtError, match="bhrt error 3"):
            sc.temporal_change(ok, *a, l, n3)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros((H, W), f32)
    L = B.lib()
    assert L.bhrt_temporal_change(None, C.byref(ok), p(n3), p(n3), p(n3), p(n3), p(l), None, None, p(out), None) == ERR_ARG                # NULL scene
    assert L.bhrt_temporal_change(sc._h, C.byref(ok), p(n3), p(n3), p(n3), p(n3), p(l), None, None, None, None) == ERR_ARG               # NULL out_length
    assert L.bhrt_temporal_change(sc._h, C.byref(ok), p(n3), p(n3), p(n3), p(n3), p(l), None, None, p(l), None) == ERR_ARG and b"out_length" in L.bhrt_last_error()
    with pytest.raises(B.BhrtError, match="bhrt error 3"):                                           # the alias, on the device variant (the pointers are never read)
        sc.temporal_change_dev(ok, 4096, 4096, 4096, 4096, 8192, d_out_length=8192)
    with pytest.raises(B.BhrtError, match="bhrt error 3"):
        sc.temporal_change_dev(ok, 4096, 4096, 4096, 4096, 8192, d_out_length=0)
    with pytest.raises(B.BhrtError, match="bhrt error 3"):
        sc.temporal_change_dev(ok, 0, 4096, 4096, 4096, 8192, d_out_length=4096)
    # what is allowed gets past the checks (without a device: "no device", not error 3)
    allowed = (lambda: sc.temporal_change(ok, n3, n3, n3, n3, l), lambda: sc.temporal_change(ok, n3, n3, n3, n3, l, l, n3, want_change=False),
               lambda: sc.temporal_change(D(radius=1, sigma_lo=0.0, sigma_hi=0.0, depth_tolerance=0.0, normal_threshold=-INF), n3, n3, n3, n3, l),
               lambda: sc.temporal_change(D(radius=4, sigma_lo=2.0, sigma_hi=2.0), n3, n3, n3, n3, l))
    for call in allowed:
        try:
            call()
        except B.BhrtError as e:
            assert "bhrt error 3" not in str(e) and not have_gpu()


def test_set_change_refusals_without_a_device(B):
    sc = B.Scene(XML)
    try:
        L, ok = B.lib(), B.default_change_opts()
        assert L.bhrt_temporal_set_change(None, C.byref(ok)) == ERR_ARG
        with pytest.raises(B.BhrtError, match="bhrt error 3.*no temporal session"):
            sc.temporal_set_change(ok)
        with pytest.raises(B.BhrtError, match="bhrt error 3.*no temporal session"):
            sc.temporal_set_change(None)
        sc.temporal_begin(B.default_opts(spp=2), B.default_temporal_session_opts())                  # light only: no variance to read
        with pytest.raises(B.BhrtError, match="bhrt error 3.*carry_variance"):
            sc.temporal_set_change(ok)
        sc.temporal_end()
        sc.temporal_begin(B.default_opts(spp=2), B.default_temporal_session_opts(carry_variance=1))
        for bad in (B.default_change_opts(radius=5), B.default_change_opts(sigma_lo=-1.0), B.default_change_opts(sigma_lo=3.0, sigma_hi=2.0),
                    B.default_change_opts(sigma_hi=INF), B.default_change_opts(depth_tolerance=NAN), B.default_change_opts(normal_threshold=NAN)):
            with pytest.raises(B.BhrtError, match="bhrt error 3.*temporal change"):
                sc.temporal_set_change(bad)
        sc.temporal_set_change(ok)
        sc.temporal_set_change(None)                                                                 # off again
        sc.temporal_set_change(B.default_change_opts(radius=1, sigma_lo=0.0, sigma_hi=0.0))
        assert sc.temporal_status().frames == 0
        sc.temporal_end()
        with pytest.raises(B.BhrtError, match="bhrt error 3.*no temporal session"):                  # end dropped it with the session
            sc.temporal_set_change(None)
    finally:
        sc.close()


def test_restatement_block_is_exact_and_sits_on_the_bounds():
    """The construction the GPU test relies on: d = 0.5 and w = 0.25 exactly at every block pixel, s and sw exact, x = 2R + 1 exactly; with
    sigma_lo = x the pixel keeps its history (x > sigma_lo fails), with sigma_hi = x it loses it (x >= sigma_hi), and sigma_lo == sigma_hi == x
    keeps it, while sigma_lo == sigma_hi just below x drops it."""
    assert (KR + KG) + KB == f32(1) and (KB * KB) * BLOCK_T == f32(0.25)
    H = W = 13
    z, n = flat_guides(H, W)
    c, h = np.full((H, W, 3), BLOCK_C, f32), np.zeros((H, W, 3), f32)
    v, hv = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
    v[..., 2] = BLOCK_T
    assert (lum(c) - lum(h) == f32(0.5)).all() and (vlum(v) + vlum(hv) == f32(0.25)).all()
    l = np.full((H, W), 4, f32)
    for R in (1, 2, 3, 4):
        X, k = block_bound(R), (2 * R + 1) ** 2
        assert f32(k * 0.5) / np.sqrt(f32(k * 0.25)) == f32(X)
        inner = (slice(R, H - R), slice(R, W - R))
        below = float(np.nextafter(f32(X), f32(0)))
        for lo, hi, lam in ((X, 2 * X, 0.0), (X / 2, X, 1.0), (X, X, 0.0), (below, below, 1.0), (below, float(np.nextafter(f32(X), f32(INF))), 0.5)):
            ol, ch = temporal_change_ref(c, v, h, hv, l, z, n, radius=R, sigma_lo=lo, sigma_hi=hi)
            assert (ch[inner] == f32(lam)).all() and (ol[inner] == f32(4) * (f32(1) - f32(lam))).all(), (R, lo, hi)


def test_restatement_properties():
    """history == radiance keeps every length's bits; a pixel without history keeps its length's bits and is no tap; nothing crosses a depth
    edge; a NaN keeps the history; no variance at all and any difference drops it."""
    rng = np.random.RandomState(5)
    H, W = 12, 20
    c, v, h, hv, l, z, n, _ = crafted(rng, W, H)
    ol, ch = temporal_change_ref(c, v, c, hv, l, z, n)
    assert ol.tobytes() == l.tobytes() and not ch.any()
    ol, ch = temporal_change_ref(c, v, h, hv, l, z, n, sigma_lo=0.5, sigma_hi=1.0)
    none = ~(l > 0)
    assert ol[none].tobytes() == l[none].tobytes() and not ch[none].any() and none.sum() > 10 and (ch > 0).any() and (ch == 0).any()
    zf, nf = flat_guides(H, W)
    zs = zf.copy()
    zs[:, W // 2:] = 7
    cc, hh = np.full((H, W, 3), 0.5, f32), np.full((H, W, 3), 0.5, f32)
    hh[:, W // 2:] = 0.25                                                       # the light changed on the right half only
    vv = np.full((H, W, 3), 1e-4, f32)
    ll = np.full((H, W), 8, f32)
    ol, ch = temporal_change_ref(cc, vv, hh, vv, ll, zs, nf)
    assert not ch[:, :W // 2].any() and (ch[:, W // 2:] == 1).all() and (ol[:, W // 2:] == 0).all() and (ol[:, :W // 2] == 8).all()
    ol, ch = temporal_change_ref(cc, vv, hh, vv, ll, zf, nf)                    # one surface: the pixels within R of the border see the change
    assert (ch[:, W // 2 - 3:W // 2] > 0).all() and not ch[:, :W // 2 - 3].any()
    ll2 = ll.copy()
    ll2[:, W // 2:] = 0                                                         # without history the changed half is no tap either
    assert not temporal_change_ref(cc, vv, hh, vv, ll2, zf, nf)[1].any()
    cn = cc.copy()
    cn[5, W // 2 + 4, 0] = NAN
    ch = temporal_change_ref(cn, vv, hh, vv, ll, zs, nf)[1]
    assert not ch[2:9, W // 2 + 1:W // 2 + 8].any() and (ch[:, W - 2:] == 1).all()
    vn = vv.copy()
    vn[5, W // 2 + 4, 1] = NAN
    assert not temporal_change_ref(cc, vn, hh, vv, ll, zs, nf)[1][2:9, W // 2 + 1:W // 2 + 8].any()
    zero = np.zeros_like(vv)
    ol, ch = temporal_change_ref(cc, zero, hh, zero, ll, zs, nf)
    assert not ch[:, :W // 2].any() and (ch[:, W // 2:] == 1).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 33), (37, 19)])
def test_kernel_equals_restatement_on_crafted_frames(B, scene, tmp_path, size):
    """k_temporal_change<R> against temporal_change_ref on the bytes of both outputs: one pixel, one workgroup exactly, and frames of more
    workgroups with the last partial on either axis; every R, with the change image and without, thresholds on both sides of the frame's x,
    equal thresholds, and the constant block's own bound as sigma_lo and as sigma_hi."""
    W, H = size
    sc = scene(_synthetic_xml(tmp_path, W, H))
    c, v, h, hv, l, z, n, block = crafted(np.random.RandomState(20 + W), W, H)
    if W * H > 100:
        assert (z >= BIG).any() and (z < BIG).any() and np.isnan(z).any() and (l == 0).any() and (l < 0).any() and np.isnan(l).any() and np.isnan(c).any()
    seen = set()
    for R in (1, 2, 3, 4):
        X = block_bound(R)
        for lo, hi in ((1.5, 3.0), (0.0, 0.5), (2.0, 2.0), (X, 2 * X), (X / 2, X), (X, X)):
            o = B.default_change_opts(radius=R, sigma_lo=lo, sigma_hi=hi, depth_tolerance=0.02)
            ref_l, ref_c = temporal_change_ref(c, v, h, hv, l, z, n, radius=R, sigma_lo=lo, sigma_hi=hi, depth_tolerance=0.02)
            got_l, got_c = sc.temporal_change(o, c, v, h, hv, l, z, n)
            assert got_l.tobytes() == ref_l.tobytes() and got_c.tobytes() == ref_c.tobytes(), (R, lo, hi, int((got_c != ref_c).sum()))
            only_l, none = sc.temporal_change(o, c, v, h, hv, l, z, n, want_change=False)
            assert none is None and only_l.tobytes() == ref_l.tobytes()
            if block is not None:                                               # the pixels whose whole window is the block sit on the bound
                mid = ref_c[block][R:11 - R, R:11 - R]
                assert mid.size and (mid == (1.0 if hi == X and lo < X else 0.0 if lo >= X else mid)).all(), (R, lo, hi)
                seen.add((lo >= X, hi == X and lo < X))
    if block is not None:
        assert seen >= {(True, False), (False, True)}
    if W * H > 100:                                                             # x = 0 and x = +inf where no tap has any variance
        lower = np.mgrid[0:H, 0:W][0] >= np.float32(0.75) * H + 1
        ref_c = temporal_change_ref(c, v, h, hv, l, z, n, radius=1, sigma_lo=1e30, sigma_hi=1e30, depth_tolerance=0.02)[1]
        assert ((ref_c == 0) & lower & (l > 0)).any() and ((ref_c == 1) & lower).any()
        got_c = sc.temporal_change(B.default_change_opts(radius=1, sigma_lo=1e30, sigma_hi=1e30, depth_tolerance=0.02), c, v, h, hv, l, z, n)[1]
        assert got_c.tobytes() == ref_c.tobytes()
    # other stops: the depth stop shut, the normal stop wide open
    for kw in (dict(depth_tolerance=0.0), dict(normal_threshold=-INF)):
        got = sc.temporal_change(B.default_change_opts(**kw), c, v, h, hv, l, z, n)
        ref = temporal_change_ref(c, v, h, hv, l, z, n, sigma_lo=B.CHANGE_SIGMA_LO, sigma_hi=B.CHANGE_SIGMA_HI, **kw)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), kw


@pytest.mark.gpu
def test_properties_call_variants_and_computed_guides(B, scene):
    """On c3_mesh_small: history == radiance keeps the bytes of the length and changes nothing; the host wrapper equals the device variant on
    device tensors, on a stream; z and normal left out equal the call fed bhrt_first_hit's images."""
    import torch
    sc = scene("c3_mesh_small")
    W, H = sc.width, sc.height
    z, n, _ = sc.first_hit()
    _, rad, var = sc.render_var(B.default_opts(spp=2, seed=3))
    _, old, ovar = sc.render_var(B.default_opts(spp=2, seed=4))
    rng = np.random.RandomState(21)
    l = rng.randint(0, 9, (H, W)).astype(f32)
    l[rng.uniform(size=(H, W)) < 0.05] = NAN
    o = B.default_change_opts()
    same_l, same_c = sc.temporal_change(o, rad, var, rad, ovar, l, z, n)
    assert same_l.tobytes() == l.tobytes() and not same_c.any()
    want_l, want_c = sc.temporal_change(o, rad, var, old, ovar, l, z, n)
    ref_l, ref_c = temporal_change_ref(rad, var, old, ovar, l, z, n, sigma_lo=B.CHANGE_SIGMA_LO, sigma_hi=B.CHANGE_SIGMA_HI)
    assert want_l.tobytes() == ref_l.tobytes() and want_c.tobytes() == ref_c.tobytes()
    for zz, nn in ((None, None), (z, None), (None, n)):                         # guides computed here
        got_l, got_c = sc.temporal_change(o, rad, var, old, ovar, l, zz, nn)
        assert got_l.tobytes() == want_l.tobytes() and got_c.tobytes() == want_c.tobytes()
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t = [up(x) for x in (rad, var, old, ovar, l, z, n)]
    out_l = torch.full((H, W), -1.0, dtype=torch.float32, device=dev)
    out_c = torch.full((H, W), -1.0, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    sc.temporal_change_dev(o, *[x.data_ptr() for x in t], out_l.data_ptr(), out_c.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert out_l.cpu().numpy().tobytes() == want_l.tobytes() and out_c.cpu().numpy().tobytes() == want_c.tobytes()
    out_l.fill_(-1.0)
    torch.cuda.synchronize()
    sc.temporal_change_dev(o, *[x.data_ptr() for x in t[:5]], d_out_length=out_l.data_ptr())                    # no guides, no change image, no stream: synchronous
    assert out_l.cpu().numpy().tobytes() == want_l.tobytes()


# the session: MODE -> (spp, spatial_variance); carry_variance, denoise and follow_nodes are on in both
SESSION_MODES = {"one_sample": (1, 1), "two_samples": (2, 0)}


def _session_opts(B, mode):
    spp, spatial = SESSION_MODES[mode]
    return B.default_opts(spp=spp, seed=SEED), B.default_temporal_session_opts(carry_variance=1, spatial_variance=spatial, denoise=1, follow_nodes=1)


def _set_frame(B, sc, k, saved):
    """The camera along test_temporal_session's move, and the ball translated at the last frame."""
    p = _pose(k)
    sc.set_camera(p[0:3], p[3:6], p[6:9])
    sc.set_node_transform(sc.node_index("ball"), saved["tm"], saved["pos"], [B.translate(*(BALL_MOVE if k == FRAMES - 1 else (0.0, 0.0, 0.0)))])


def _chain(B, mode, change):
    """The session's frames through the host wrappers, bhrt_temporal_change between bhrt_reproject_var and bhrt_temporal_accumulate_var when
    `change` (the options) is given: one dict of images per frame."""
    spp, spatial = SESSION_MODES[mode]
    ro, to, sv, dn = B.default_reproject_opts(), B.default_temporal_opts(), B.default_spatial_variance_opts(), B.default_denoise_opts()
    sc = B.Scene(XML)
    out, prev = [], None
    try:
        saved = sc.node_transform(sc.node_index("ball"))
        for k in range(FRAMES):
            _set_frame(B, sc, k, saved)
            f = {}
            f["z"], f["normal"], f["albedo"] = z, n, a = sc.first_hit()
            f["node"] = sc.first_hit_node()
            _, cur, cv = sc.render_var(B.default_opts(spp=spp, seed=SEED + k))
            if spatial and spp < 2:
                cv = sc.variance_spatial(sv, cur, None, None, z, n, a)
            h = hv = hl = used = None
            if prev is not None:
                h, hv, hl = sc.reproject_var(ro, prev["frame"], prev["z"], prev["normal"], prev["accumulated"], prev["variance"], prev["length"], prev["albedo"], z, n, a,
                                             prev_xforms=prev["xf"], prev_id=prev["node"], id=f["node"], want=("history", "history_variance", "length"))[:3]
                used = hl
                if change is not None:
                    used, lam = sc.temporal_change(change, cur, cv, h, hv, hl, z, n)
            acc, accv, ln, rgb = sc.temporal_accumulate_var(to, cur, cv, float(spp), h, hv, used)
            f["variance"], f["current_variance"] = accv, cv
            est = accv
            if spatial:
                est = f["filter_variance"] = sc.variance_spatial(sv, acc, accv, ln, z, n, a)
            shown, rgb = sc.denoise(dn, acc, est, z, n, a)
            f.update(accumulated=acc, length=ln, current=cur, history_length=np.zeros_like(ln) if hl is None else hl, shown=shown, rgb8=rgb)
            if change is not None:
                f.update(change=np.zeros_like(ln) if prev is None else lam, used_length=np.zeros_like(ln) if prev is None else used)
            out.append(f)
            prev = dict(f, frame=sc.camera_frame(), xf=sc.node_transforms())
    finally:
        sc.close()
    return out


_chains = {}


@pytest.fixture(scope="module")
def chain(B):
    """The reference frames of (mode, with the stage), computed once and shared; nobody writes to them."""
    def get(mode, on):
        if (mode, on) not in _chains:
            _chains[mode, on] = _chain(B, mode, B.default_change_opts() if on else None)
            for f in _chains[mode, on]:
                for a in f.values():
                    a.flags.writeable = False
        return _chains[mode, on]
    return get


def _kept_all(B, sc):
    f = _kept(B, sc)
    for key, which in (("change", B.TEMPORAL_IMG_CHANGE), ("used_length", B.TEMPORAL_IMG_USED_LENGTH)):
        if B.lib().bhrt_temporal_image_dev(sc._h, which, C.byref(C.c_void_p())) == ERR_ARG:
            with pytest.raises(B.BhrtError, match="not kept"):
                sc.temporal_image(which)
            continue
        f[key] = sc.temporal_image(which)
    return f


def _frames(B, mode, setup):
    """A session of FRAMES frames; setup(sc) runs after begin.  Returns one dict per frame and the history_pixels of each."""
    sc = B.Scene(XML)
    out, counts = [], []
    try:
        saved = sc.node_transform(sc.node_index("ball"))
        sc.temporal_begin(*_session_opts(B, mode))
        setup(sc)
        for k in range(FRAMES):
            _set_frame(B, sc, k, saved)
            rgb, rad, _ = sc.temporal_frame()
            out.append(dict(_kept_all(B, sc), shown=rad, rgb8=rgb))
            counts.append(sc.temporal_status().history_pixels)
        sc.temporal_end()
    finally:
        sc.close()
    return out, counts


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(SESSION_MODES))
def test_session_frames_equal_the_chained_wrappers(B, chain, mode):
    ref = chain(mode, True)
    got, counts = _frames(B, mode, lambda sc: sc.temporal_set_change(B.default_change_opts()))
    for k in range(FRAMES):
        _same(got[k], ref[k], (mode, k))
        assert counts[k] == int((ref[k]["history_length"] > 0).sum())
    assert not ref[0]["change"].any() and not ref[0]["used_length"].any()
    assert (ref[2]["change"] > 0).any() and (ref[2]["used_length"] < ref[2]["history_length"]).any()   # the stage did something to compare


@pytest.mark.gpu
def test_session_without_the_stage_is_unchanged_and_the_switch_follows_its_rules(B, chain):
    mode = "one_sample"
    off, on = chain(mode, False), chain(mode, True)
    never, counts_never = _frames(B, mode, lambda sc: None)

    def on_then_off(sc):
        sc.temporal_set_change(B.default_change_opts())
        sc.temporal_set_change(None)
    nulled, counts_nulled = _frames(B, mode, on_then_off)
    for k in range(FRAMES):
        _same(never[k], off[k], ("never", k))
        _same(nulled[k], off[k], ("set to NULL", k))
        assert "change" not in never[k] and "used_length" not in never[k]
        assert off[k]["history_length"].tobytes() == on[k]["history_length"].tobytes() or k == 2   # the stage changes what frame 2 reprojects, not who finds a surface
        assert counts_never[k] == counts_nulled[k] == int((on[k]["history_length"] > 0).sum())    # history_pixels is unchanged by the stage
    sc = B.Scene(XML)
    try:
        saved = sc.node_transform(sc.node_index("ball"))
        sc.temporal_begin(*_session_opts(B, mode))
        sc.temporal_set_change(B.default_change_opts())
        _set_frame(B, sc, 0, saved)
        sc.temporal_frame()
        for o in (None, B.default_change_opts()):
            with pytest.raises(B.BhrtError, match="bhrt error 3.*a frame has completed"):
                sc.temporal_set_change(o)
        _set_frame(B, sc, 1, saved)
        sc.temporal_frame()
        sc.temporal_reset()                                                     # a cut keeps the setting: the three frames are the chain's again
        for k in range(FRAMES):
            _set_frame(B, sc, k, saved)
            rgb, rad, _ = sc.temporal_frame()
        _same(dict(_kept_all(B, sc), shown=rad, rgb8=rgb), on[2], "after reset")
        sc.temporal_reset()
        sc.temporal_set_change(None)                                            # legal again after a reset
        _set_frame(B, sc, 0, saved)
        rgb, rad, _ = sc.temporal_frame()
        _same(dict(_kept_all(B, sc), shown=rad, rgb8=rgb), off[0], "off after reset")
    finally:
        sc.close()


@pytest.mark.gpu
def test_the_stage_lowers_the_error_where_the_light_changed(B):
    """c3_mesh_small, a static camera, 1 spp, carry + spatial + denoise + follow_nodes, six frames; the ball is translated by BALL_MOVE at frame
    3 and stays.  T0, T1: 256-spp renders (with their variance) of the scene before and after the move.  The changed region: the pixels whose
    truth luminance differs before and after by more than three standard deviations of that difference as the two renders' own variances give
    it, |L(T1) - L(T0)| > 3 sqrt(vL(var0) + vL(var1)).  Over it, the mean absolute error of the last displayed frame against T1 is lower with the
    stage (library defaults) than without.  The figures are printed."""
    def run(on):
        sc = B.Scene(XML)
        try:
            saved = sc.node_transform(sc.node_index("ball"))
            sc.temporal_begin(B.default_opts(spp=1, seed=40), B.default_temporal_session_opts(carry_variance=1, spatial_variance=1, denoise=1, follow_nodes=1))
            if on:
                sc.temporal_set_change(B.default_change_opts())
            for k in range(6):
                sc.set_node_transform(sc.node_index("ball"), saved["tm"], saved["pos"], [B.translate(*(BALL_MOVE if k >= 3 else (0.0, 0.0, 0.0)))])
                rad = sc.temporal_frame()[1]
            lam = sc.temporal_image(B.TEMPORAL_IMG_CHANGE) if on else None
            return rad, lam
        finally:
            sc.close()
    sc = B.Scene(XML)
    try:
        saved = sc.node_transform(sc.node_index("ball"))
        _, T0, V0 = sc.render_var(B.default_opts(spp=256, seed=977))
        sc.set_node_transform(sc.node_index("ball"), saved["tm"], saved["pos"], [B.translate(*BALL_MOVE)])
        _, T1, V1 = sc.render_var(B.default_opts(spp=256, seed=978))
    finally:
        sc.close()
    changed = np.abs(lum(T1) - lum(T0)) > f32(3) * np.sqrt(vlum(V0) + vlum(V1))
    with_stage, lam = run(True)
    without, _ = run(False)
    mae = lambda x, m: float(np.abs(x - T1)[m].mean())  # noqa: E731
    print(f"changed region {int(changed.sum())} pixels; MAE there without the stage {mae(without, changed):.5g}, with {mae(with_stage, changed):.5g}; "
          f"elsewhere without {mae(without, ~changed):.5g}, with {mae(with_stage, ~changed):.5g}; lambda > 0 on {float((lam > 0).mean()):.4f} of the last frame")
    assert changed.sum() > 200
    assert mae(with_stage, changed) < mae(without, changed)
