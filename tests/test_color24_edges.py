"""The tail of every 8-bit image — gamma, then Color24::FloatToByte (cyColor.h:271-272) — where int(float) is undefined in C++.

The rule (csrc/device_color24.h color24_channel, the oracle's FloatToByte): with t = v * 255 + 0.5f in float arithmetic, NaN, t >= 2^31 and
t <= -2^31 convert to INT_MIN, what the compiled reference's cvttss2si gives on x86-64, hence to byte 0; anything else truncates toward zero
and clamps to [0, 255].  A GPU conversion left to itself saturates instead: +inf, 1e30 or 8421505 would come out 255, white where the
reference is black.

CPU: O.color24 against a numpy restatement of the rule on a crafted vector.  GPU: the same vector, tiled over a frame, through
bhrt_denoise and bhrt_denoise_sampled with no iterations (the identity kernel: out = the input's bits, rgb8 = store_color24 of it) and
through bhrt_color_image_dev, against the oracle byte for byte and bit for bit."""
import numpy as np
import pytest

from conftest import same_bits

f32 = np.float32
INF = f32(np.inf)
FLT_MAX = np.finfo(f32).max
BYTE_EDGES = (0, 1, 127, 128, 254, 255, 256)
INT_EDGE = f32(8421504.0)  # the largest float v with v * 255 + 0.5f < 2^31 (2147483520); its successor 8421505 gives exactly 2^31


def t_of(v):
    """v * 255 + 0.5f, each operation rounded to float."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(v, f32) * f32(255) + f32(0.5)
    assert t.dtype == f32
    return t


def rule_bytes(v):
    """The rule restated: v after gamma -> byte."""
    t = t_of(v)
    int_min = np.isnan(t) | (t >= f32(2147483648.0)) | (t <= f32(-2147483649.0))
    i = np.where(int_min, np.int64(-2 ** 31), np.trunc(np.where(int_min, f32(0), t)).astype(np.int64))
    return np.clip(i, 0, 255).astype(np.uint8)


def around(v, reach):
    out = [f32(v)]
    lo = hi = f32(v)
    for _ in range(reach):
        lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        out += [lo, hi]
    return np.array(out, f32)


# the classes of the crafted vector; every one must be present in what a test feeds
CLASSES = {
    "byte edge": np.concatenate([around((k - 0.5) / 255, 3) for k in BYTE_EDGES]),  # v * 255 + 0.5f just below, at and just above k
    "negative": np.array([-0.0, -1e-45, -1e-7, -1e-3, -0.5 / 255, -0.002, -1 / 255, -1, -1e10], f32),
    "int edge": np.concatenate([[f32(8.4e6)], around(INT_EDGE, 2)]),
    "huge": np.array([1e30, FLT_MAX], f32),
    "non-finite": np.array([np.inf, -np.inf, np.nan], f32),
    "plain": np.array([0.0, 0.25, 0.5, 0.75, 1.0, 2.0, 1e-45, 1e-10], f32),
}
VECTOR = np.concatenate(list(CLASSES.values()))


def holds_every_class(a):
    a = np.asarray(a, f32).reshape(-1)
    bits = set(a.view(np.uint32).tolist())
    return all(bits & set(v.view(np.uint32).tolist()) for v in CLASSES.values())


def test_vector_reaches_the_edges():
    """The byte-edge values straddle every k, the int-edge values straddle 2^31, and the rule answers them as the issue states."""
    for k in BYTE_EDGES:
        t = t_of(around((k - 0.5) / 255, 3))
        assert t.min() < k <= t.max() and np.all(np.abs(t - k) < 1e-4)
        assert (t == k).any() or k == 0  # the integer itself is hit (at 0 the sum's spacing is 2^-24: the straddle is what counts)
    t = t_of(around(INT_EDGE, 2))
    assert (t == f32(2147483520.0)).any() and (t == f32(2147483648.0)).any()
    assert list(rule_bytes(np.array([INT_EDGE, np.nextafter(INT_EDGE, INF), 8.4e6, 1e30, FLT_MAX, np.inf, -np.inf, np.nan, -1e10, -0.0, 1.0], f32))) \
        == [255, 0, 255, 0, 0, 0, 0, 0, 0, 0, 255]
    assert holds_every_class(VECTOR) and not holds_every_class(VECTOR[np.isfinite(VECTOR)])


@pytest.mark.parametrize("gamma", [0, 1])
def test_oracle_color24_follows_the_rule(gamma, O):
    v = VECTOR
    if gamma:  # negatives become NaN through powf_ (a non-integer exponent) and so byte 0
        v = O.math_eval(6, O.MATH_DEVICE, VECTOR, np.full_like(VECTOR, f32(1) / f32(2.2)))
        assert same_bits(v, O.color_image(VECTOR, 1))
        assert np.isnan(v[VECTOR < 0]).all() and v[np.signbit(VECTOR) & (VECTOR == 0)][0] == 0
    got = O.color24(VECTOR, gamma)
    want = rule_bytes(v)
    assert np.array_equal(got, want), f"gamma {gamma}: " + "; ".join(f"{VECTOR[k]!r}: {got[k]}, rule {want[k]}" for k in np.flatnonzero(got != want))
    assert set(want.tolist()) >= {0, 1, 126, 127, 128, 253, 254, 255} if not gamma else want.max() == 255
    # white is reached only by in-range values; everything the conversion cannot hold is black
    beyond = np.isnan(t_of(v)) | (np.abs(t_of(v)) >= f32(2147483648.0))
    assert beyond.sum() >= 6 and np.all(got[beyond] == 0)


def crafted_frame(W, H):
    frame = np.resize(VECTOR, H * W * 3).astype(f32).reshape(H * W, 3)
    frame[-1] = [np.inf, np.nan, 1e30]  # one pixel whose three channels leave the range in three ways
    frame[-2] = [1e30, np.inf, np.nan]
    return frame.reshape(H, W, 3)


@pytest.mark.gpu
def test_gpu_image_tail_on_the_crafted_frame(B, O, load_scene):
    import torch
    if B.device_count() < 1:
        pytest.fail("no HIP device")
    sc = load_scene("c1_sphere_plane")
    W, H = sc.width, sc.height
    frame = crafted_frame(W, H)
    assert holds_every_class(frame) and W * H * 3 >= 2 * VECTOR.size
    for gamma in (0, 1):
        want = O.color24(frame, gamma)
        assert (want == 255).any() and not want.reshape(-1, 3)[-2:].any()  # the two pixels of +inf, NaN and 1e30 are black
        o = B.default_denoise_opts(iterations=0, gamma=gamma)
        out, rgb = sc.denoise(o, frame)
        assert same_bits(out, frame), f"gamma {gamma}: bhrt_denoise changed the radiance"
        bad = np.flatnonzero(rgb.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, f"gamma {gamma}: bhrt_denoise, {bad.size} bytes differ, e.g. " + "; ".join(
            f"{frame.reshape(-1)[k]!r}: {rgb.reshape(-1)[k]}, oracle {want.reshape(-1)[k]}" for k in bad[:6])
        out, rgb = sc.denoise_sampled(o, frame, None, None, None, None, None)  # no iterations: no guide is read
        assert same_bits(out, frame) and np.array_equal(rgb, want), f"gamma {gamma}: bhrt_denoise_sampled"
        dev = torch.device("cuda", 0)
        rad = torch.from_numpy(frame).to(dev)
        col = torch.zeros_like(rad)
        sc.color_image_dev(rad.data_ptr(), H * W, gamma, col.data_ptr())
        torch.cuda.synchronize()
        assert same_bits(col.cpu().numpy().reshape(-1), O.color_image(frame.reshape(-1), gamma)), f"gamma {gamma}: bhrt_color_image_dev"
