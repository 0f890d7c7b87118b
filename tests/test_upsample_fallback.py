"""The fallback switch of guided upsampling: bhrt_upsample_opts.fallback = BHRT_UPSAMPLE_FALLBACK_LIGHT gives a pixel no tap
passes the taps' light as it was rendered, with no albedo of its own (csrc/upsample.hip states it in stage 4U's head).

upsample_ref_fb restates the stage with both rules in numpy, float32, in the kernel's tap and sum order, in the style of
tests/test_upsample.py::upsample_ref (which stays the yardstick of rule 0: the two are compared on the bytes)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_denoise import _synthetic_xml, divisor
from test_reproject import BIG, scene  # noqa: F401
from test_upsample import _mse, edge_pixels, positions, upsample_ref

f32 = np.float32
NAN, INF = float("nan"), float("inf")
ERR_ARG = 3
ALBEDO, LIGHT = 0, 1
# low (w, h) -> factor: one workgroup, several, a ragged edge, s = 2, 4, 3 and 8, a tile that clamps on every side
CASES = [((1, 1), 2), ((8, 8), 4), ((17, 11), 3), ((5, 3), 8)]


def upsample_ref_fb(c, v, zl, nl, al, z, n, a, depth_tolerance=0.01, normal_threshold=0.99, demodulate=1, fallback=ALBEDO):
    """Stage 4U of csrc/upsample.hip with opts.fallback.  Arguments as upsample_ref's.  Returns its dict (out, variance, confidence, `fallback` =
    the level a pixel fell back to: 0 a tap passed, 1 its own kind, 2 all four; b) and, beside it, the weights `k` (4, H, W) the sums ran with,
    `tap_miss` (4, H, W): the kind of each tap, and `tap_nan` (4, H, W): a NaN in the tap's radiance."""
    c, zl, nl, z, n = (np.asarray(k, f32) for k in (c, zl, nl, z, n))
    H, W = z.shape
    h, w = zl.shape
    s = W // w
    assert 1 <= s <= 8 and W == s * w and H == s * h and fallback in (ALBEDO, LIGHT)
    tol, thr = f32(depth_tolerance), f32(normal_threshold)
    with np.errstate(all="ignore"):
        raw_v = None if v is None else np.asarray(v, f32)
        e, vv = c, raw_v
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
        b, ok, kind, idx, tap_miss = [], [], [], [], []
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
            tap_miss.append(zq >= BIG)
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
        level = np.zeros((H, W), np.int32)
        k1, S1 = weigh(kind)
        k2, S2 = weigh([np.ones((H, W), bool)] * 4)
        first, second = S == 0, (S == 0) & (S1 == 0)
        level[first], level[second] = 1, 2
        k = [np.where(second, c2, np.where(first, c1, c0)).astype(f32) for c0, c1, c2 in zip(k, k1, k2)]
        S = np.where(second, S2, np.where(first, S1, S)).astype(f32)

        def sums(img, img_v):
            m = np.zeros((H, W, 3), f32)
            u = np.zeros((H, W, 3), f32)
            for t in range(4):
                on = (k[t] > 0)[..., None]
                m = (m + np.where(on, k[t][..., None] * img[idx[t]], f32(0))).astype(f32)
                if img_v is not None:
                    u = (u + np.where(on, (k[t] * k[t]).astype(f32)[..., None] * img_v[idx[t]], f32(0))).astype(f32)
            return (m / S[..., None]).astype(f32), None if img_v is None else (u / (S * S).astype(f32)[..., None]).astype(f32)
        out, var = sums(e, vv)
        if demodulate:
            g = divisor(np.asarray(a, f32))
            out = (out * g).astype(f32)
            if var is not None:
                var = (var * (g * g).astype(f32)).astype(f32)
            if fallback == LIGHT:                                              # the raw low images, and no divisor(a_p)
                out1, var1 = sums(c, raw_v)
                out = np.where(first[..., None], out1, out)
                if var is not None:
                    var = np.where(first[..., None], var1, var)
    return dict(out=out, variance=var, confidence=conf, fallback=level, b=np.stack(b), k=np.stack(k), tap_miss=np.stack(tap_miss),
                tap_nan=np.stack([np.isnan(c[q]).any(-1) for q in idx]))


def classes(r, z, n):
    """Which kinds of pixel a frame holds, from the restatement's own record.  `own_mixed`: a hit that takes the taps of its own kind, hits that
    fail, beside taps that are misses (a miss never takes the first fallback: a tap of its kind passes its test).  `all_four_nan`: a NaN depth
    (a hit by the rule) over taps that are all misses.  `all_four_miss`: a miss over taps that are all hits."""
    weighed = r["b"] > 0
    tap_m, tap_h = (r["tap_miss"] & weighed).any(0), (~r["tap_miss"] & weighed).any(0)
    lvl = r["fallback"]
    hit = ~(z >= BIG)
    return dict(confident=(r["confidence"] > 0).any(),
                own_kind=(lvl == 1).any(),
                own_mixed=((lvl == 1) & hit & tap_m & tap_h).any(),
                all_four_nan=((lvl == 2) & np.isnan(z) & tap_m & ~tap_h).any(),
                all_four_miss=((lvl == 2) & (z >= BIG) & tap_h & ~tap_m).any(),
                nan_radiance=((lvl > 0) & ((r["k"] > 0) & r["tap_nan"]).any(0)).any(),
                zero_normal=((n == 0).all(-1) & hit & (lvl > 0)).any())


def crafted_fb(rng, w, h, s):
    """A low frame w x h (w, h >= 3) and full-size guides s w x s h in which every class of `classes` occurs by construction, chance adding more:
    the low frame's first column is a miss, the rest a sloped surface; the low albedo is dark (0.02 .. 0.1) where the full one is bright, so
    the two rules differ by factors.  Returns (c, v, zl, nl, al, z, n, a)."""
    W, H = s * w, s * h
    yy, xx = np.mgrid[0:H, 0:W].astype(f32)
    z = (f32(3) + f32(0.004) * xx + f32(0.006) * yy).astype(f32)
    n = np.zeros((H, W, 3), f32)
    n[..., 2] = 1
    n = (n + rng.normal(0, 0.02, (H, W, 3))).astype(f32)
    a = rng.uniform(0.3, 0.95, (H, W, 3)).astype(f32)
    z[:, :s], n[:, :s], a[:, :s] = BIG, 0, 0                                   # the full pixels of low column 0: misses
    zl, nl = z[::s, ::s].copy(), n[::s, ::s].copy()
    al = rng.uniform(0.02, 0.1, (h, w, 3)).astype(f32)
    al[:, 0] = 0
    al[h - 1, w - 1] = 5e-4                                                    # below the floor: divisor 1
    u = rng.uniform(size=(H, W))
    z[(u < 0.04) & (xx >= s)] = 50.0                                           # hits none of whose taps is near
    flip = (u > 0.05) & (u < 0.08)                                             # pixels of the other kind than their surroundings
    z[flip] = np.where(z[flip] >= BIG, f32(4), BIG)
    z[(u > 0.08) & (u < 0.10)] = NAN
    n[(u > 0.10) & (u < 0.12)] = 0
    ym = H // 2
    z[ym, 0] = NAN                                                             # both taps' columns clamp onto low column 0: all four, over misses
    z[ym, s] = 50.0                                                            # I0 = 0, 0 < fx < 1: misses on the left, hits that fail on the right
    z[ym, W - 2], n[ym, W - 2] = BIG, 0                                        # a miss over hits: all four
    z[1, W - 1], n[1, W - 1] = f32(3) + f32(0.004) * f32(W - 1) + f32(0.006), 0    # a zero normal on a hit
    nl[0, w - 1] = 0
    zl[h - 1, 2] = NAN
    c = rng.gamma(4.0, 0.25, (h, w, 3)).astype(f32)
    v = rng.gamma(2.0, 0.002, (h, w, 3)).astype(f32)
    J0 = positions(H, s)[0][ym]
    c[min(max(J0, 0), h - 1), 1, 1] = NAN                                      # a NaN radiance under the taps of (s, ym)
    return c, v, zl, nl, al, z, n, a


def one_low_pixel_frames(rng, s=2):
    """1 x 1 -> 2 x 2: one low pixel has one kind and one radiance, so no single frame holds every class; three frames do between them (a hit
    among misses needs two low pixels and is left to the larger shapes)."""
    frames = []
    for low_miss, nan_c in ((False, False), (True, False), (False, True)):
        z = np.float32([[3.0, 50.0], [BIG, 3.0]]) if not low_miss else np.float32([[BIG, NAN], [INF, 4.0]])
        n = np.zeros((2, 2, 3), f32)
        n[..., 2] = 1
        n[1, 1] = 0                                                            # a zero normal on a hit
        a = rng.uniform(0.3, 0.95, (2, 2, 3)).astype(f32)
        zl = np.full((1, 1), BIG if low_miss else 3.0, f32)
        nl = np.float32([[[0, 0, 0 if low_miss else 1]]])
        al = np.float32([[[0, 0, 0]]]) if low_miss else rng.uniform(0.02, 0.1, (1, 1, 3)).astype(f32)
        c = rng.gamma(4.0, 0.25, (1, 1, 3)).astype(f32)
        if nan_c:
            c[0, 0, 2] = NAN
        v = rng.gamma(2.0, 0.002, (1, 1, 3)).astype(f32)
        frames.append((c, v, zl, nl, al, z, n, a))
    return frames


def frames_of(low, s):
    w, h = low
    rng = np.random.RandomState(70 + w)
    return one_low_pixel_frames(rng, s) if (w, h) == (1, 1) else [crafted_fb(rng, w, h, s)]


def assert_classes(low, frames, **opts):
    """Every class occurs in every frame; for the one-low-pixel shape in the frames together, a hit among misses excepted (see there)."""
    seen = [classes(upsample_ref_fb(*f, fallback=LIGHT, **opts), f[5], f[6]) for f in frames]
    if low == (1, 1):
        union = {k: any(s[k] for s in seen) for k in seen[0]}
        union.pop("own_mixed")
        assert all(union.values()), union
    else:
        for s in seen:
            assert all(s.values()), s


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_struct_size_default_and_constants(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    assert "BHRT_UPSAMPLE_FALLBACK_ALBEDO = 0" in hdr and "BHRT_UPSAMPLE_FALLBACK_LIGHT = 1" in hdr and "int32_t fallback;" in hdr
    assert (B.UPSAMPLE_FALLBACK_ALBEDO, B.UPSAMPLE_FALLBACK_LIGHT) == (0, 1)
    assert C.sizeof(B.UpsampleOpts) == 32
    o = B.default_upsample_opts()
    assert o.fallback == 0 and bytes(o)[16:] == bytes(16)
    o = B.default_upsample_opts(fallback=B.UPSAMPLE_FALLBACK_LIGHT)
    assert o.fallback == 1 and list(o.reserved) == [1, 0, 0, 0] and bytes(o)[16:20] == (1).to_bytes(4, "little")      # the int32 after gamma
    head = open(os.path.join(ROOT, "bhraytracer_amd", "csrc", "upsample.hip")).read().split("#include")[0]
    assert "BHRT_UPSAMPLE_FALLBACK_LIGHT" in head


@pytest.mark.parametrize("value", [2, -1])
def test_a_fallback_that_is_neither_is_refused_before_the_device(B, scene, value):
    """BHRT_ERR_ARG (error 3) through both entry points on a scene that was never uploaded."""
    sc = scene("c1_sphere_plane")
    w, h = sc.width // 2, sc.height // 2
    l1, l3 = np.ones((h, w), f32), np.ones((h, w, 3), f32)
    bad = B.default_upsample_opts(fallback=value)
    with pytest.raises(B.BhrtError, match="bhrt error 3.*fallback"):
        sc.upsample(bad, l3, l1, l3, l3)
    n3, N3 = 12 * w * h, 12 * sc.width * sc.height
    base = 1 << 20
    with pytest.raises(B.BhrtError, match="bhrt error 3.*fallback"):           # the pointers are never read
        sc.upsample_dev(bad, w, h, d_low_radiance=base, d_low_z=base + n3, d_low_normal=base + 2 * n3, d_low_albedo=base + 3 * n3, d_out=base + 8 * N3)
    assert B.lib().bhrt_upsample(sc._h, C.byref(bad), w, h, *[x.ctypes.data_as(C.c_void_p) for x in (l3, l3, l1, l3, l3)], None, None, None,
                                 np.zeros((sc.height, sc.width, 3), f32).ctypes.data_as(C.c_void_p), None, None, None) == ERR_ARG
    assert b"fallback" in B.lib().bhrt_last_error()


@pytest.mark.parametrize("low,s", CASES)
def test_restatement_rule_0_is_the_yardstick_and_the_frames_hold_every_class(low, s):
    """upsample_ref_fb at fallback = 0 is tests/test_upsample.py::upsample_ref on the bytes, and the crafted frames hold every class of pixel."""
    frames = frames_of(low, s)
    assert_classes(low, frames)
    for f in frames:
        for demod in (1, 0):
            mine, theirs = upsample_ref_fb(*f, demodulate=demod, fallback=ALBEDO), upsample_ref(*f, demodulate=demod)
            for name in ("out", "variance", "confidence", "fallback"):
                assert mine[name].tobytes() == theirs[name].tobytes(), (demod, name)


@pytest.mark.parametrize("low,s", CASES[1:])
def test_restatement_properties_of_the_light_rule(low, s):
    """Rule 1 is rule 0 wherever confidence > 0, and everywhere with demodulate = 0; where no tap passed, out is the b-weighted mean of the raw
    radiance of the taps that count and does not depend on either albedo image, and rule 0 does depend on them."""
    c, v, zl, nl, al, z, n, a = frames_of(low, s)[0]
    r0, r1 = (upsample_ref_fb(c, v, zl, nl, al, z, n, a, fallback=fb) for fb in (ALBEDO, LIGHT))
    sure = r0["confidence"] > 0
    assert sure.any() and (~sure).any() and r0["confidence"].tobytes() == r1["confidence"].tobytes()
    for name in ("out", "variance"):
        assert r1[name][sure].tobytes() == r0[name][sure].tobytes()
        assert r1[name][~sure].tobytes() != r0[name][~sure].tobytes()
    d0, d1 = (upsample_ref_fb(c, v, zl, nl, al, z, n, a, demodulate=0, fallback=fb) for fb in (ALBEDO, LIGHT))
    assert d0["out"].tobytes() == d1["out"].tobytes() and d0["variance"].tobytes() == d1["variance"].tobytes()
    rng = np.random.RandomState(5)
    other = upsample_ref_fb(c, v, zl, nl, rng.uniform(0.2, 0.9, al.shape).astype(f32), z, n, rng.uniform(0.01, 0.5, a.shape).astype(f32), fallback=LIGHT)
    for name in ("out", "variance"):
        assert other[name][~sure].tobytes() == r1[name][~sure].tobytes()
    # by hand, pixel by pixel: the taps of the pixel's own kind with b, or all four, over the raw radiance
    I0, _ = positions(z.shape[1], s)
    J0, _ = positions(z.shape[0], s)
    h, w = zl.shape
    checked = 0
    for y, x in zip(*np.nonzero(~sure)):
        taps = [(min(max(J0[y] + (t >> 1), 0), h - 1), min(max(I0[x] + (t & 1), 0), w - 1)) for t in range(4)]
        bt = r1["b"][:, y, x]
        own = [bool(zl[q] >= BIG) == bool(z[y, x] >= BIG) for q in taps]
        k = [bt[t] if own[t] else f32(0) for t in range(4)]
        if sum(k) == 0:
            k = list(bt)
        S, m = f32(0), np.zeros(3, f32)
        for t in range(4):
            S = f32(S + k[t])
            if k[t] > 0:
                m = (m + k[t] * c[taps[t]]).astype(f32)
        with np.errstate(all="ignore"):
            want = (m / S).astype(f32)
        assert want.tobytes() == r1["out"][y, x].tobytes(), (y, x)
        checked += 1
    assert checked == (~sure).sum() > 0


def test_restatement_floor_pixel_over_glass_by_hand():
    """2 x 2 -> 4 x 4: the low frame is glass of albedo 0.02 and radiance 0.5; full pixel (1, 1) is floor of albedo 0.9 at a depth that fails the
    stop.  Rule 0 gives it the glass's light times 0.9 / 0.02, about 22.5; rule 1 gives it 0.5."""
    zl, nl = np.full((2, 2), 3, f32), np.zeros((2, 2, 3), f32)
    nl[..., 2] = 1
    al, c, v = np.full((2, 2, 3), 0.02, f32), np.full((2, 2, 3), 0.5, f32), np.full((2, 2, 3), 0.01, f32)
    z, n, a = np.full((4, 4), 3, f32), np.zeros((4, 4, 3), f32), np.full((4, 4, 3), 0.02, f32)
    n[..., 2] = 1
    z[1, 1], a[1, 1] = 50.0, 0.9
    r0, r1 = (upsample_ref_fb(c, v, zl, nl, al, z, n, a, fallback=fb) for fb in (ALBEDO, LIGHT))
    assert r0["confidence"][1, 1] == 0 and r0["fallback"][1, 1] == 1 and (r0["fallback"].sum(), (r0["confidence"] > 0).sum()) == (1, 15)
    bt = np.float32([0.5625, 0.1875, 0.1875, 0.0625])                          # fx = fy = 1 / 4 at s = 2
    assert (r0["b"][:, 1, 1] == bt).all()
    e = f32(0.5) / f32(0.02)
    m, S = f32(0), f32(0)
    for k in bt:
        S, m = f32(S + k), f32(m + f32(k * e))
    want0 = f32(f32(m / S) * f32(0.9))
    assert S == 1 and (r0["out"][1, 1] == want0).all() and abs(float(want0) - 22.5) < 1e-4
    assert (r1["out"][1, 1] == f32(0.5)).all()                                  # sum b 0.5 / 1: exact
    u0 = f32(0)
    for k in bt:
        u0 = f32(u0 + f32(f32(k * k) * f32(0.01)))
    assert (r1["variance"][1, 1] == u0).all()                                   # / (1 * 1)
    rest = np.ones((4, 4), bool)
    rest[1, 1] = False
    assert r0["out"][rest].tobytes() == r1["out"][rest].tobytes() and r0["variance"][rest].tobytes() == r1["variance"][rest].tobytes()
    assert np.allclose(r0["out"][rest], 0.5, rtol=1e-6)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

WANTS = (("out", "variance", "confidence", "rgb8"), ("out",), ("variance", "confidence"), ("rgb8",))


def _sized_scene(scene, tmp_path, low, s):
    sc = scene(_synthetic_xml(tmp_path, low[0], low[1]))
    sc.set_resolution(s * low[0], s * low[1])
    assert (sc.width, sc.height) == (s * low[0], s * low[1])
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("low,s", CASES)
def test_kernel_equals_restatement_with_the_light_rule(B, O, scene, tmp_path, low, s):
    """k_upsample at fallback = 1 against upsample_ref_fb on the bytes of all four outputs, with and without the variance, the confidence, rgb8
    and demodulate, under the default stops and under others; every frame holds every class of pixel (asserted)."""
    sc = _sized_scene(scene, tmp_path, low, s)
    frames = frames_of(low, s)
    assert_classes(low, frames)
    for c, v, zl, nl, al, z, n, a in frames:
        for demod in (1, 0):
            for kw in (dict(), dict(depth_tolerance=0.05, normal_threshold=-INF, gamma=0)):
                o = B.default_upsample_opts(demodulate=demod, fallback=LIGHT, **kw)
                ref = upsample_ref_fb(c, v, zl, nl, al, z, n, a, depth_tolerance=o.depth_tolerance, normal_threshold=o.normal_threshold, demodulate=demod, fallback=LIGHT)
                ref["rgb8"] = O.color24(ref["out"], o.gamma)
                assert (ref["fallback"] > 0).any()
                for want in WANTS if not kw else WANTS[:1]:
                    got = sc.upsample(o, c, zl, nl, al if demod else None, v if "variance" in want else None, z, n, a if demod else None, want=want)
                    assert set(got) == set(want)
                    for name in want:
                        assert got[name].tobytes() == ref[name].tobytes(), (demod, kw, want, name, int((got[name] != ref[name]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("low,s", CASES)
def test_default_rule_did_not_move_and_the_rules_agree_without_demodulate(B, O, scene, tmp_path, low, s):
    """The same frames at fallback = 0 (set, and left at the default): the bytes of tests/test_upsample.py::upsample_ref.  With demodulate = 0
    the device's bytes under rule 1 are those under rule 0, with the albedo images left out."""
    sc = _sized_scene(scene, tmp_path, low, s)
    for c, v, zl, nl, al, z, n, a in frames_of(low, s):
        ref = upsample_ref(c, v, zl, nl, al, z, n, a)
        ref["rgb8"] = O.color24(ref["out"], 1)
        for o in (B.default_upsample_opts(), B.default_upsample_opts(fallback=ALBEDO)):
            got = sc.upsample(o, c, zl, nl, al, v, z, n, a)
            for name in ("out", "variance", "confidence", "rgb8"):
                assert got[name].tobytes() == ref[name].tobytes(), name
        g0, g1 = (sc.upsample(B.default_upsample_opts(demodulate=0, fallback=fb), c, zl, nl, None, v, z, n, None) for fb in (ALBEDO, LIGHT))
        ref = upsample_ref(c, v, zl, nl, al, z, n, a, demodulate=0)
        for name in ("out", "variance", "confidence", "rgb8"):
            assert g1[name].tobytes() == g0[name].tobytes(), name
        assert g0["out"].tobytes() == ref["out"].tobytes()


@pytest.mark.gpu
def test_call_variants_and_computed_guides_with_the_light_rule(B, O, scene):
    """c1_sphere_plane from half size at fallback = 1: the host wrapper equals the restatement and the device variant on device tensors on a
    stream; full-size guides left out equal the call fed bhrt_first_hit's images."""
    import torch
    full = scene("c1_sphere_plane")
    W, H = full.width, full.height
    low = full.clone()
    try:
        w, h = W // 2, H // 2
        low.set_resolution(w, h)
        _, c, v = low.render_var(B.default_opts(spp=2, seed=3))
        zl, nl, al = low.first_hit()
    finally:
        low.close()
    z, n, a = full.first_hit()
    o = B.default_upsample_opts(fallback=LIGHT)
    want = full.upsample(o, c, zl, nl, al, v, z, n, a)
    ref = upsample_ref_fb(c, v, zl, nl, al, z, n, a, fallback=LIGHT)
    ref["rgb8"] = O.color24(ref["out"], 1)
    print("c1_sphere_plane s=2: pixels with confidence 0:", int((ref["confidence"] == 0).sum()))
    names = ("out", "variance", "confidence", "rgb8")
    for name in names:
        assert want[name].tobytes() == ref[name].tobytes(), name
    for zz, nn, aa in ((None, None, None), (z, None, a), (None, n, None), (z, n, None)):                # guides computed here
        got = full.upsample(o, c, zl, nl, al, v, zz, nn, aa)
        for name in names:
            assert got[name].tobytes() == want[name].tobytes(), name
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (c, v, zl, nl, al, z, n, a)]
    outs = [torch.full(sh, -1.0, dtype=torch.float32, device=dev) for sh in ((H, W, 3), (H, W, 3), (H, W))]
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    full.upsample_dev(o, w, h, *[x.data_ptr() for x in t], *[x.data_ptr() for x in outs], rgb.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    for name, x in zip(names, outs + [rgb]):
        assert x.cpu().numpy().tobytes() == want[name].tobytes(), name
    outs[0].fill_(-1.0)
    torch.cuda.synchronize()
    full.upsample_dev(o, w, h, t[0].data_ptr(), 0, *[x.data_ptr() for x in t[2:5]], d_out=outs[0].data_ptr())       # no guides, no stream: synchronous
    assert outs[0].cpu().numpy().tobytes() == want["out"].tobytes()


@pytest.mark.gpu
def test_light_rule_beats_plain_bilinear_and_the_albedo_rule_on_c2_glass_small(B, scene):
    """c2_glass_small, 160 x 90 at 16 spp (seed 11) upsampled with s = 2, against the 256-spp full-size frame (seed 5), as the condition on
    c3_mesh_small is set up: with fallback = 1 the guided frame's MSE is below plain bilinear's on the whole frame and on the edge pixels, and
    below the guided frame's with fallback = 0 on the whole frame; the pixels with confidence 0 exist and are under 5 % of the frame.
    Conditions, not ratios.  The figures are printed."""
    full = scene("c2_glass_small")
    W, H = full.width, full.height
    if W % 2 or H % 2:
        full.set_resolution(W - W % 2, H - H % 2)
        W, H = full.width, full.height
    low = full.clone()
    try:
        low.set_resolution(W // 2, H // 2)
        _, c, v = low.render_var(B.default_opts(spp=16, seed=11))
        zl, nl, al = low.first_hit()
    finally:
        low.close()
    ref = full.render(B.default_opts(spp=256, seed=5))[1]
    light = full.upsample(B.default_upsample_opts(fallback=LIGHT), c, zl, nl, al, v, want=("out", "confidence"))
    albedo = full.upsample(B.default_upsample_opts(), c, zl, nl, al, v, want=("out", "confidence"))
    plain = full.upsample(B.default_upsample_opts(depth_tolerance=3e38, normal_threshold=-INF, demodulate=0), c, np.ones_like(zl), nl, None, None,
                          np.ones((H, W), f32), want=("out", "confidence"))
    assert (np.abs(plain["confidence"] - 1) <= 4 * 2.0 ** -24).all()             # every tap passed: plain bilinear
    assert light["confidence"].tobytes() == albedo["confidence"].tobytes()
    lost = light["confidence"] == 0
    edges = edge_pixels(full.first_hit_node())
    figures = dict(light=_mse(light["out"], ref), albedo=_mse(albedo["out"], ref), plain=_mse(plain["out"], ref), light_edges=_mse(light["out"], ref, edges),
                   albedo_edges=_mse(albedo["out"], ref, edges), plain_edges=_mse(plain["out"], ref, edges), edge_pixels=int(edges.sum()),
                   confidence_zero=int(lost.sum()), confidence_zero_share=float(lost.mean()))
    print("upsample fallback quality c2_glass_small s=2:", figures)
    assert light["out"][~lost].tobytes() == albedo["out"][~lost].tobytes()
    assert 0 < edges.sum() < edges.size
    assert 0 < lost.sum() < 0.05 * lost.size, figures
    assert figures["light"] < figures["plain"], figures
    assert figures["light_edges"] < figures["plain_edges"], figures
    assert figures["light"] < figures["albedo"], figures
