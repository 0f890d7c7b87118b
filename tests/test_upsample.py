"""Guided upsampling: bhrt_upsample rebuilds a W x H frame from one rendered at w x h, W = s w, H = s h, along the full-size first
hit (csrc/upsample.hip states it as stage 4U).

upsample_ref restates the stage in numpy, float32, in the kernel's tap and sum order, vectorised over full pixels: one tap of every pixel at a
time.  A tap of weight 0 enters the sums as + 0, which is what skipping it does (a sum that starts at +0 never becomes -0)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, have_gpu
from test_denoise import _synthetic_xml, divisor
from test_reproject import BIG, scene  # noqa: F401

f32 = np.float32
NAN, INF = float("nan"), float("inf")
ERR_ARG = 3
SYMBOLS = ("bhrt_upsample", "bhrt_upsample_dev")
# low (w, h) -> factor: the sizes the kernel is pinned at
CASES = [((1, 1), 2), ((8, 8), 4), ((17, 11), 3), ((19, 37), 2), ((5, 3), 8)]


def positions(W, s):
    """The integer position rule along one axis: (I0, f) per full coordinate.  tx = 2x + 1 - s, I0 = floor(tx / 2s), f = (tx - 2s I0) / 2s."""
    x = np.arange(W, dtype=np.int64)
    tx = 2 * x + 1 - s
    I0 = np.floor_divide(tx, 2 * s)
    return I0, ((tx - 2 * s * I0).astype(f32) / f32(2 * s)).astype(f32)


def upsample_ref(c, v, zl, nl, al, z, n, a, depth_tolerance=0.01, normal_threshold=0.99, demodulate=1):
    """Stage 4U of csrc/upsample.hip.  c, v (or None), zl, nl, al: the low frame (h, w[, 3]); z, n, a: the full-size first hit (H, W[, 3]); al
    and a are read only with demodulate.  Returns a dict: out, variance (None without v), confidence, and `fallback` (0 = a tap passed, 1 = the
    taps of the pixel's own kind, 2 = all four) and the bilinear weights `b` (4, H, W), which the kernel does not write."""
    c, zl, nl, z, n = (np.asarray(k, f32) for k in (c, zl, nl, z, n))
    H, W = z.shape
    h, w = zl.shape
    s = W // w
    assert 1 <= s <= 8 and W == s * w and H == s * h
    tol, thr = f32(depth_tolerance), f32(normal_threshold)
    with np.errstate(all="ignore"):
        e, vv = c, None if v is None else np.asarray(v, f32)
        if demodulate:
            d = divisor(np.asarray(al, f32))
            e = (c / d).astype(f32)
            if vv is not None:
                vv = (vv / (d * d).astype(f32)).astype(f32)
        I0, fx = positions(W, s)
        J0, fy = positions(H, s)
        gx, gy = (f32(1) - fx).astype(f32), (f32(1) - fy).astype(f32)
        xs, ys = np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64)
        miss = z >= BIG
        tz = (tol * z).astype(f32)
        b, ok, kind, idx = [], [], [], []
        for t in range(4):
            di, dj = t & 1, t >> 1
            I, J = np.clip(I0 + di, 0, w - 1), np.clip(J0 + dj, 0, h - 1)
            q = np.ix_(J, I)
            b.append(((fx if di else gx)[None, :] * (fy if dj else gy)[:, None]).astype(f32))
            dx, dy = (s * I - xs)[None, :], (s * J - ys)[:, None]
            r = np.maximum(f32(1), np.sqrt((dx * dx + dy * dy).astype(f32))).astype(f32)
            zq, nq = zl[q], nl[q]
            dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
            same = (zq < BIG) & (np.abs(zq - z) <= tz * r) & (dot >= thr)
            ok.append(np.where(miss, zq >= BIG, same))
            kind.append((zq >= BIG) == miss)
            idx.append(q)
        zero = np.zeros((H, W), f32)

        def weigh(masks):
            k = [np.where(m, bt, f32(0)).astype(f32) for m, bt in zip(masks, b)]
            S = zero
            for kt in k:
                S = (S + kt).astype(f32)
            return k, S
        k, S = weigh(ok)
        conf = S
        fallback = np.zeros((H, W), np.int32)
        k1, S1 = weigh(kind)
        k2, S2 = weigh([np.ones((H, W), bool)] * 4)
        first, second = S == 0, (S == 0) & (S1 == 0)
        fallback[first], fallback[second] = 1, 2
        k = [np.where(second, c2, np.where(first, c1, c0)).astype(f32) for c0, c1, c2 in zip(k, k1, k2)]
        S = np.where(second, S2, np.where(first, S1, S)).astype(f32)
        m = np.zeros((H, W, 3), f32)
        u = np.zeros((H, W, 3), f32)
        for t in range(4):
            on = (k[t] > 0)[..., None]
            m = (m + np.where(on, k[t][..., None] * e[idx[t]], f32(0))).astype(f32)
            if vv is not None:
                u = (u + np.where(on, (k[t] * k[t]).astype(f32)[..., None] * vv[idx[t]], f32(0))).astype(f32)
        out = (m / S[..., None]).astype(f32)
        var = None if vv is None else (u / (S * S).astype(f32)[..., None]).astype(f32)
        if demodulate:
            g = divisor(np.asarray(a, f32))
            out = (out * g).astype(f32)
            if var is not None:
                var = (var * (g * g).astype(f32)).astype(f32)
    return dict(out=out, variance=var, confidence=conf, fallback=fallback, b=np.stack(b))


def crafted(rng, w, h, s):
    """A low frame of w x h and full-size guides of s w x s h: the full guides hold a depth step, a normal flip, normals near the threshold, a band
    of misses and single ones, zero normals and a NaN depth; the low guides are the full ones at the guide pixels (s I, s J), then a NaN, a zero
    normal and a miss of their own.  Single full pixels are given a depth (a kind) none of their taps has: both fallbacks.  The low radiance holds
    a NaN, the albedo black and near-black pixels.  Returns (c, v, zl, nl, al, z, n, a)."""
    W, H = s * w, s * h
    yy, xx = np.mgrid[0:H, 0:W].astype(f32)
    z = (f32(3) + f32(0.004) * xx + f32(0.006) * yy).astype(f32)
    z[:, W // 2:] += f32(2)                                                     # a depth step
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    n[(xx + yy) > f32(0.6) * (W + H)] = np.float32([0.6, 0, 0.8])               # a normal flip
    n = (n + rng.normal(0, 0.03, (H, W, 3))).astype(f32)                        # raw dots on both sides of 0.99
    a = rng.uniform(0.05, 0.95, (H, W, 3)).astype(f32)                          # the texture detail demodulation gives back
    u = rng.uniform(size=(H, W))
    miss = (u < 0.04) | ((yy < H // 4) & (xx > W // 3))                         # a band of misses beside hits, and single ones
    z[miss] = BIG
    z[miss & (u < 0.015)] = INF
    n[miss] = 0
    a[miss] = 0
    n[(u > 0.20) & (u < 0.23)] = 0                                              # zero normals on hits
    a[(u > 0.30) & (u < 0.33)] = 0                                              # black: divisor 1
    a[(u > 0.33) & (u < 0.35)] = 5e-4                                           # below the floor on every channel
    a[(u > 0.35) & (u < 0.37), 1] = 0                                           # one channel below it
    zl, nl, al = z[::s, ::s].copy(), n[::s, ::s].copy(), a[::s, ::s].copy()
    ul = rng.uniform(size=(h, w))
    zl[ul < 0.03] = NAN                                                         # a NaN guide on the low side
    nl[(ul > 0.03) & (ul < 0.06)] = 0
    zl[(ul > 0.06) & (ul < 0.08)] = BIG
    z[(u > 0.10) & (u < 0.115)] = NAN                                           # and on the full side
    z[(u > 0.40) & (u < 0.43)] = 50.0                                           # a hit none of whose taps is near: its own kind counts
    flip = (u > 0.50) & (u < 0.54)                                              # a pixel of the other kind than its surroundings: often all four
    z[flip] = np.where(z[flip] >= BIG, f32(4), BIG)
    if w * h > 8:                                                               # the same by hand, for the frames too small for chance
        zl[h - 1, 1], nl[h - 1, 0] = NAN, 0
        z[H - 2, 1], z[H - 3, 2 * s], z[H - 1, 3 * s + 1], n[H - 2, s] = NAN, 50.0, BIG, 0
    c = rng.gamma(4.0, 0.25, (h, w, 3)).astype(f32)
    v = rng.gamma(2.0, 0.002, (h, w, 3)).astype(f32)
    if w * h > 8:
        c[h // 2, w // 2, 1] = NAN                                              # a NaN radiance
    return c, v, zl, nl, al, z, n, a


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_symbols_exported_declared_and_wrapped(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in SYMBOLS:
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr), s
    s = "bhrt_default_upsample_opts"
    assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bvoid %s\(" % s, hdr) and "DESIGN.md 25" in hdr
    for w in ("upsample", "upsample_dev", "set_resolution"):
        assert callable(getattr(B.Scene, w))
    head = open(os.path.join(ROOT, "bhraytracer_amd", "csrc", "upsample.hip")).read().split("#include")[0]
    assert "4U. GUIDED UPSAMPLING" in head and "not independent" in head


def test_struct_size_and_defaults(B):
    assert C.sizeof(B.UpsampleOpts) == 32
    buf = (C.c_uint8 * 64)(*([0xAB] * 64))
    B.lib().bhrt_default_upsample_opts(C.byref(buf))
    assert bytes(buf[16:32]) == bytes(16) and bytes(buf[32:]) == b"\xab" * 32                                # exactly 32 bytes, reserved[4] the zero tail
    o = B.default_upsample_opts()
    assert bytes(o) == bytes(buf[:32])
    sv = B.default_spatial_variance_opts()
    assert f32(o.depth_tolerance) == f32(sv.depth_tolerance) and f32(o.normal_threshold) == f32(sv.normal_threshold)      # stage 3S's
    assert o.demodulate == 1 and o.gamma == 1 and list(o.reserved) == [0, 0, 0, 0]
    assert B.default_upsample_opts(demodulate=0).demodulate == 0


def test_bad_arguments_are_refused_before_the_device(B, scene):
    """Every BHRT_ERR_ARG case (error 3) on a loaded scene that was never uploaded: the checks come before any device is touched."""
    sc = scene("c1_sphere_plane")
    W, H = sc.width, sc.height
    assert W % 2 == 0 and H % 2 == 0
    w, h = W // 2, H // 2
    l1, l3 = np.ones((h, w), f32), np.ones((h, w, 3), f32)
    ok, D = B.default_upsample_opts(), B.default_upsample_opts
    for o in (None, D(depth_tolerance=-0.01), D(depth_tolerance=INF), D(depth_tolerance=NAN), D(normal_threshold=NAN)):
        with pytest.raises(B.BhrtError, match="bhrt error 3"):
            sc.upsample(o, l3, l1, l3, l3)
    with pytest.raises(B.BhrtError, match="bhrt error 3.*low_albedo"):             # demodulate needs the low albedo
        sc.upsample(ok, l3, l1, l3, None)
    with pytest.raises(B.BhrtError, match="bhrt error 3"):                         # nothing asked for (a variance without low_variance is not allocated)
        sc.upsample(ok, l3, l1, l3, l3, want=("variance",))
    L = B.lib()
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros((H, W, 3), f32)
    a = lambda **kw: [kw.get("scene", sc._h), C.byref(ok), kw.get("w", w), kw.get("h", h), kw.get("c", p(l3)), kw.get("v"), kw.get("zl", p(l1)),  # noqa: E731
                      kw.get("nl", p(l3)), p(l3), None, None, None, kw.get("out", p(out)), kw.get("ov"), None, None]
    assert L.bhrt_upsample(*a()) != ERR_ARG or have_gpu() is False
    for kw in (dict(scene=None), dict(c=None), dict(zl=None), dict(nl=None), dict(out=None), dict(ov=p(out.copy()))):
        assert L.bhrt_upsample(*a(**kw)) == ERR_ARG, kw
    # the size rule: W = s w and H = s h for one integer s in 1..8
    for bw, bh in ((0, h), (w, 0), (-1, -1), (w, H), (W, h), (w + 1, h), (W * 2, H * 2), (w, h + 1)):
        assert L.bhrt_upsample(*a(w=bw, h=bh)) == ERR_ARG and b"upsample" in L.bhrt_last_error(), (bw, bh)
    if W % 16 == 0 and H % 16 == 0:                                                # s = 16 divides both and is refused
        assert L.bhrt_upsample(*a(w=W // 16, h=H // 16)) == ERR_ARG
    # an output that is an input, or another output, on the device variant (the pointers are never read)
    n3, N3 = 12 * w * h, 12 * W * H
    base = 1 << 20
    lo = dict(d_low_radiance=base, d_low_z=base + n3, d_low_normal=base + 2 * n3, d_low_albedo=base + 3 * n3, d_low_variance=base + 4 * n3)
    free = base + 8 * N3
    for kw in (dict(d_out=base), dict(d_out=base + n3 - 4), dict(d_out=base + 3 * n3), dict(d_out_variance=base + 4 * n3), dict(d_confidence=base + 2 * n3),
               dict(d_rgb8=base + n3), dict(d_out=free, d_z=free + N3 - 4), dict(d_out=free, d_normal=free), dict(d_out=free, d_albedo=free + 8),
               dict(d_out=free, d_out_variance=free + 4), dict(d_out=free, d_rgb8=free + N3 - 1), dict(d_confidence=free, d_out_variance=free)):
        with pytest.raises(B.BhrtError, match="bhrt error 3.*alias"):
            sc.upsample_dev(ok, w, h, **{**lo, **kw})
    with pytest.raises(B.BhrtError, match="bhrt error 3"):
        sc.upsample_dev(ok, w, h, **lo)                                            # no output
    with pytest.raises(B.BhrtError, match="bhrt error 3.*low_variance"):
        sc.upsample_dev(ok, w, h, **{**lo, "d_low_variance": 0}, d_out_variance=free)
    # what is allowed gets past the checks (without a device: "no device", not error 3)
    allowed = (lambda: sc.upsample(ok, l3, l1, l3, l3), lambda: sc.upsample(D(demodulate=0), l3, l1, l3), lambda: sc.upsample(ok, l3, l1, l3, l3, l3),
               lambda: sc.upsample(D(depth_tolerance=0.0, normal_threshold=-INF), l3, l1, l3, l3, want=("rgb8",)),
               lambda: sc.upsample(ok, np.ones((H, W, 3), f32), np.ones((H, W), f32), np.ones((H, W, 3), f32), np.ones((H, W, 3), f32)))      # s = 1
    for call in allowed:
        try:
            call()
        except B.BhrtError as e:
            assert "bhrt error 3" not in str(e) and not have_gpu()


@pytest.mark.parametrize("s", [1, 2, 3, 4, 5, 6, 7, 8])
def test_restatement_position_rule(s):
    """The integer position rule: the low pixel's colour sits at its centre, s I + (s - 1) / 2 in full coordinates; I0 is -1 left of the first
    centre and w - 1 right of the last; f is exact to one rounding of k / 2s; the four weights sum to 1 within their four roundings; the tap
    span of 16 pixels fits the kernel's tile and the guide distance its table of roots."""
    w = 9
    W = s * w
    I0, f = positions(W, s)
    x = np.arange(W)
    centre = s * I0 + (s - 1) / 2.0                                               # of low pixel I0, exact in double
    assert ((x - centre) / s == f.astype(np.float64)).all() or s in (3, 5, 6, 7)   # a power of two divides exactly
    assert (np.abs((x - centre) / s - f) <= 2.0 ** -25).all() and (f >= 0).all() and (f < 1).all()
    assert I0[0] == (-1 if s > 1 else 0) and I0[-1] == w - 1 and (np.diff(I0) >= 0).all() and (np.diff(I0) <= 1).all()
    first = (s - 1) // 2 if s % 2 else s // 2                                      # the first pixel at or right of centre 0
    assert (I0[:first] == -1).all() and I0[first] == 0
    if s in (2, 3, 4):                                                            # the borders, spelled out
        want = {2: ([-1, 0, 0, 1], [0.75, 0.25, 0.75, 0.25]), 3: ([-1, 0, 0, 0, 1], [2 / 3, 0, 1 / 3, 2 / 3, 0]),
                4: ([-1, -1, 0, 0, 0, 0, 1], [0.625, 0.875, 0.125, 0.375, 0.625, 0.875, 0.125])}[s]
        k = len(want[0])
        assert I0[:k].tolist() == want[0] and (f[:k] == (np.float32(want[1]) if s != 3 else (np.float32([4, 0, 2, 4, 0]) / f32(6)))).all()
        assert I0[-1] == w - 1 and f[-1] == f32((s - 1) / (2.0 * s)) or s == 3   # the last pixel lies (s - 1) / 2 right of the last centre
        assert I0[W - 1] + 1 == w                                                 # its right tap is clamped onto the same low pixel
    g = (f32(1) - f).astype(f32)
    bsum = ((g[None, :] * g[:, None] + f[None, :] * g[:, None]) + g[None, :] * f[:, None]) + f[None, :] * f[:, None]
    assert (np.abs(bsum.astype(np.float64) - 1) <= 4 * 2.0 ** -24).all()
    for x0 in range(0, W, 16):                                                    # the kernel's tile: ceil(15 / s) + 2 low pixels a side, at most 17
        blk = I0[x0:x0 + 16]
        assert blk.max() + 1 - blk.min() + 1 <= (15 + s - 1) // s + 2 <= 17
    I = np.clip(I0[:, None] + np.arange(2)[None, :], 0, w - 1)
    assert np.abs(s * I - x[:, None]).max() <= 11 and np.abs(s * I - x[:, None]).max() < 1.5 * s + (s == 1)


def test_restatement_identity_at_s_1():
    """s = 1, the same guides on both sides, demodulate = 0: out is the radiance bit for bit (no -0 in it), also where a pixel fails its own
    test (a zero normal, a NaN depth: the first fallback gives the same tap), the variance is the variance and a NaN stays where it is."""
    rng = np.random.RandomState(3)
    c, v, zl, nl, al, z, n, a = crafted(rng, 23, 19, 1)
    c[2, 3] = [INF, -INF, 0.0]
    r = upsample_ref(c, v, z, n, a, z, n, a, demodulate=0)
    assert r["out"].tobytes() == c.tobytes() and r["variance"].tobytes() == v.tobytes()
    assert (r["fallback"] == 1).any() and not (r["fallback"] == 2).any() and (r["confidence"][r["fallback"] == 0] == 1).all()
    assert (r["b"][0] == 1).all() and not r["b"][1:].any()
    rd = upsample_ref(c, v, z, n, a, z, n, a, demodulate=1)                         # c / d * d: within two roundings, not bits
    fin = np.isfinite(c)
    assert np.allclose(rd["out"][fin], c[fin], rtol=3e-7, atol=0) and np.isnan(rd["out"][~np.isfinite(c) & np.isnan(c)]).all()


def test_restatement_properties():
    """A constant low frame comes out constant; nothing crosses a depth edge; a NaN radiance reaches exactly the pixels that weigh it; a NaN guide
    fails the test; confidence is the weight that passed; the variance of a pixel between four equal taps is a quarter of theirs."""
    s, w, h = 4, 8, 6
    W, H = s * w, s * h
    z = np.full((H, W), 3, f32)
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    a = np.full((H, W, 3), 0.5, f32)
    zl, nl, al = z[::s, ::s].copy(), n[::s, ::s].copy(), a[::s, ::s].copy()
    c, v = np.full((h, w, 3), 0.375, f32), np.full((h, w, 3), 0.25, f32)
    r = upsample_ref(c, v, zl, nl, al, z, n, a, demodulate=0)
    assert (np.abs(r["out"] - f32(0.375)) <= 2.0 ** -24).all() and not r["fallback"].any()
    assert (np.abs(r["confidence"] - 1) <= 4 * 2.0 ** -24).all()
    assert r["variance"].max() <= 0.25 * (1 + 1e-6) and np.isclose(r["variance"][3, 3], 0.25 * (0.625 ** 4 + 2 * (0.625 * 0.375) ** 2 + 0.375 ** 4)).all()
    # a depth edge between low columns 3 and 4: left pixels take only left taps
    z2 = z.copy()
    z2[:, 4 * s:] = 7
    zl2 = z2[::s, ::s].copy()
    c2 = c.copy()
    c2[:, 4:] = 2.0
    r = upsample_ref(c2, None, zl2, nl, al, z2, n, a, demodulate=0)
    assert (r["out"][:, :4 * s] == f32(0.375)).all() and (r["out"][:, 4 * s:] == f32(2.0)).all() and r["variance"] is None
    assert (r["confidence"][:, 3 * s + 2:4 * s + 2] < 1 - 1e-3).all() and not r["fallback"].any()
    # a NaN radiance at low (2, 3) reaches the pixels whose passing taps hold it, no others
    c3 = c.copy()
    c3[2, 3, 0] = NAN
    r = upsample_ref(c3, None, zl, nl, al, z, n, a, demodulate=0)
    bad = np.isnan(r["out"][..., 0])
    ys, xs = np.nonzero(bad)
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (6, 13, 10, 17) and bad.sum() == 64      # s / 2 left of centre 1 (2) up to s / 2 right of centre 3 (4)
    assert not np.isnan(r["out"][..., 1:]).any()
    # a NaN low depth fails every test against it: its weight is gone from the confidence
    zl4 = zl.copy()
    zl4[2, 3] = NAN
    r = upsample_ref(c, None, zl4, nl, al, z, n, a, demodulate=0)
    assert (r["confidence"][bad] < 1).all() and (r["confidence"][~bad] > 1 - 1e-6).all() and (r["out"] == r["out"]).all()
    # a full pixel that is a miss among hits: no tap passes and none is of its kind
    z5 = z.copy()
    z5[9, 9] = BIG
    r = upsample_ref(c, None, zl, nl, al, z5, n, a, demodulate=0)
    assert r["fallback"][9, 9] == 2 and r["confidence"][9, 9] == 0 and r["fallback"].sum() == 2
    z5[9, 9] = 50.0
    r = upsample_ref(c, None, zl, nl, al, z5, n, a, demodulate=0)
    assert r["fallback"][9, 9] == 1 and r["confidence"][9, 9] == 0 and r["fallback"].sum() == 1


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

WANTS = (("out", "variance", "confidence", "rgb8"), ("out",), ("variance", "confidence"), ("rgb8",), ("confidence",))


@pytest.mark.gpu
@pytest.mark.parametrize("low,s", CASES)
def test_kernel_equals_restatement_on_crafted_frames(B, O, scene, tmp_path, low, s):
    """k_upsample against upsample_ref on the bytes of all four outputs, on frames whose size is set through bhrt_scene_set_resolution: one
    low pixel, one workgroup exactly and more, the last partial on either axis, every factor's own tile; each with and without the variance,
    the confidence, rgb8 and demodulate, with both gammas and with other stops."""
    w, h = low
    W, H = s * w, s * h
    sc = scene(_synthetic_xml(tmp_path, w, h))
    sc.set_resolution(W, H)
    assert (sc.width, sc.height) == (W, H)
    c, v, zl, nl, al, z, n, a = crafted(np.random.RandomState(40 + w), w, h, s)
    if W * H > 500:
        assert (z >= BIG).any() and (z < BIG).any() and np.isnan(z).any() and np.isnan(zl).any() and np.isnan(c).any()
        assert ((n == 0).all(-1) & (z < BIG)).any() and ((nl == 0).all(-1)).any()
    seen = set()
    for demod in (1, 0):
        for kw in (dict(), dict(depth_tolerance=0.0), dict(depth_tolerance=0.05, normal_threshold=-INF), dict(normal_threshold=0.9999, gamma=0)):
            o = B.default_upsample_opts(demodulate=demod, **kw)
            ref = upsample_ref(c, v, zl, nl, al, z, n, a, depth_tolerance=o.depth_tolerance, normal_threshold=o.normal_threshold, demodulate=demod)
            ref["rgb8"] = O.color24(ref["out"], o.gamma)
            seen |= set(np.unique(ref["fallback"]).tolist())
            for want in WANTS if not kw else WANTS[:1]:
                got = sc.upsample(o, c, zl, nl, al if demod else None, v if "variance" in want else None, z, n, a if demod else None, want=want)
                assert set(got) == set(want)
                for name in want:
                    assert got[name].tobytes() == ref[name].tobytes(), (demod, kw, want, name, int((got[name] != ref[name]).sum()))
            if demod == 0:                                                     # albedo images are not read without demodulate
                got = sc.upsample(o, c, zl, nl, None, v, z, n, None, want=("out", "variance"))
                assert got["out"].tobytes() == ref["out"].tobytes() and got["variance"].tobytes() == ref["variance"].tobytes()
    if W * H > 500:
        assert seen == {0, 1, 2}                                               # both fallbacks were taken
    # all four borders: the outermost ring takes clamped taps
    assert ref["out"].shape == (H, W, 3)


@pytest.mark.gpu
def test_identity_call_variants_and_computed_guides(B, O, scene):
    """On c1_sphere_plane at half size: s = 1 with the same guides and demodulate = 0 returns the radiance's bytes; the host wrapper equals the
    device variant on device tensors, on a stream; full-size guides left out equal the call fed bhrt_first_hit's images."""
    import torch
    full = scene("c1_sphere_plane")
    W, H = full.width, full.height
    low = full.clone()
    try:
        w, h = W // 2, H // 2
        low.set_resolution(w, h)
        _, c, v = low.render_var(B.default_opts(spp=2, seed=3))
        zl, nl, al = low.first_hit()
        z, n, a = full.first_hit()
        one = low.upsample(B.default_upsample_opts(demodulate=0), c, zl, nl, None, v, zl, nl, None)
        assert one["out"].tobytes() == (c + f32(0)).tobytes() and one["variance"].tobytes() == v.tobytes()
        for demod in (1, 0):
            o = B.default_upsample_opts(demodulate=demod)
            want = full.upsample(o, c, zl, nl, al, v, z, n, a)
            ref = upsample_ref(c, v, zl, nl, al, z, n, a, demodulate=demod)
            ref["rgb8"] = O.color24(ref["out"], 1)
            for name in ("out", "variance", "confidence", "rgb8"):
                assert want[name].tobytes() == ref[name].tobytes(), (demod, name)
            for zz, nn, aa in ((None, None, None), (z, None, a), (None, n, None), (z, n, None)):        # guides computed here
                got = full.upsample(o, c, zl, nl, al, v, zz, nn, aa)
                for name in want:
                    assert got[name].tobytes() == want[name].tobytes(), (demod, name)
            dev = torch.device("cuda", 0)
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
            t = [up(x) for x in (c, v, zl, nl, al, z, n, a)]
            outs = [torch.full(sh, -1.0, dtype=torch.float32, device=dev) for sh in ((H, W, 3), (H, W, 3), (H, W))]
            rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
            st = torch.cuda.Stream(dev)
            torch.cuda.synchronize()
            full.upsample_dev(o, w, h, *[x.data_ptr() for x in t], *[x.data_ptr() for x in outs], rgb.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            for name, x in zip(("out", "variance", "confidence", "rgb8"), outs + [rgb]):
                assert x.cpu().numpy().tobytes() == want[name].tobytes(), (demod, name)
            outs[0].fill_(-1.0)
            torch.cuda.synchronize()
            full.upsample_dev(o, w, h, t[0].data_ptr(), 0, *[x.data_ptr() for x in t[2:5]], d_out=outs[0].data_ptr())   # no guides, no stream: synchronous
            assert outs[0].cpu().numpy().tobytes() == want["out"].tobytes()
    finally:
        low.close()


def _mse(x, ref, mask=None):
    d = (x.astype(np.float64) - ref.astype(np.float64)) ** 2
    return float(d.mean() if mask is None else d[mask].mean())


def edge_pixels(node):
    """Pixels whose 3 x 3 block holds more than one first-hit node."""
    H, W = node.shape
    pad = np.pad(node, 1, mode="edge")
    blocks = np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return (blocks != node[None]).any(0)


@pytest.mark.gpu
def test_guided_beats_plain_bilinear_on_c3_mesh_small(B, scene):
    """c3_mesh_small, 160 x 120 at 16 spp upsampled with s = 2, against the 256-spp full-size frame: the guided frame's MSE is below that of the
    same low frame upsampled with every surface test passing and demodulate = 0 (plain bilinear), on the whole frame and on the edge pixels.
    A condition, not a ratio.  The figures are printed."""
    full = scene("c3_mesh_small")
    W, H = full.width, full.height
    assert (W, H) == (320, 240)
    low = full.clone()
    try:
        low.set_resolution(W // 2, H // 2)
        _, c, v = low.render_var(B.default_opts(spp=16, seed=11))
        zl, nl, al = low.first_hit()
        ref = full.render(B.default_opts(spp=256, seed=5))[1]
        guided = full.upsample(B.default_upsample_opts(), c, zl, nl, al, v, want=("out",))["out"]
        plain = full.upsample(B.default_upsample_opts(depth_tolerance=3e38, normal_threshold=-INF, demodulate=0), c, np.ones_like(zl), nl, None, None,
                              np.ones((H, W), f32), want=("out", "confidence"))
        assert (np.abs(plain["confidence"] - 1) <= 4 * 2.0 ** -24).all()         # every tap passed: plain bilinear
        edges = edge_pixels(full.first_hit_node())
        figures = dict(guided=_mse(guided, ref), plain=_mse(plain["out"], ref), guided_edges=_mse(guided, ref, edges), plain_edges=_mse(plain["out"], ref, edges),
                       edge_pixels=int(edges.sum()))
        print("upsample quality c3_mesh_small s=2:", figures)
        assert 0 < edges.sum() < edges.size
        assert figures["guided"] < figures["plain"], figures
        assert figures["guided_edges"] < figures["plain_edges"], figures
    finally:
        low.close()
