"""bhrt_detmath.h at its edges: accuracy against float64, special values against libm, device bits against host bits.

tests/test_detmath.py holds the header to libm's *float* functions on comfortable ranges.  Here the oracle's device-math mode
(O.math_eval(fn, O.MATH_DEVICE, ...): the header compiled for the host) is measured against numpy float64 on the float32 inputs widened
to float64, in ulps of the float32-rounded reference (np.spacing), on seeded inputs (np.random.default_rng(0), 400,000 points per set).

Measured maxima (x86-64 host; the GPU test below is what makes them hold for gfx950).  "first" is the figure of the measurement that
motivated these tests, "here" the one these tests print (pytest -s); the bound asserted is ceil(here + 0.5) ulp.

    case                                                               first     here    bound
    sin   uniform(-8, 8)                                               1.46      1.457   2
    cos   uniform(-8, 8)                                               -         1.451   2
    sin   uniform(-100, 100)                                           1.49      1.467   2
    cos   uniform(-100, 100)                                           -         3.948   5     (x = 83.252205, beside the zero at 26.5 pi)
    tan   uniform(-1.5707, 1.5707)                                     2.77      2.835   4
    acos  [-1,1], 1-e^u, -1+e^u (u in [-30,0]), e^u (u in [-100,0])    1.22      1.249   2
    asin  the same four sets                                           2.34      2.350   3
    atan2 both arguments normal * e^u, u in [-40,40]                   2.75      2.717   4
    powf_ x = e^u (u in [-80,80]), y in [-40,40]: normal results       0.50      0.500   1
    powf_ the same, subnormal results, in units of 2^-149              -         0.500   1
    powf_ the same, overflowing results                                all +inf  all +inf

sin / cos by range (absolute error, the measure that matters near their zeros):

    |x| <= 1e4          7.5e-8 first; here sin 7.40e-8, cos 7.54e-8; asserted <= 1e-7
    1e4 < |x| <= 1e5    9.6e-7 at 1e5 first; here sin 9.58e-7, cos 7.39e-7    printed only: the result is asserted finite and in [-1, 1]
    1e5 <= |x| < 1e6    3e-2 at 1e6 first;   here sin 3.13e-2, cos 2.43e-2    printed only, as above
    |x| >= 1e6, +-inf, NaN                                    NaN, asserted

Every caller of sinf_, cosf_, tanf_ and sincos_f in csrc/ passes an angle within [0, 2 pi]: 2 pi * rnd01 (device_shade.h
sample_along_normal, sample_along_light_direction, sample_in_semi_sphere, draw_along_light_direction, sample_in_light; device_photon.h's
emission direction; kernels.hip's lens sample and its denoiser tap table), acos_safe(...) in [0, pi] and half or twice such an angle
(device_shade.h gi_direction, sample_in_light; device_photon.h).  test_callers_range_is_inside_the_accurate_domain states that as numbers.

Special values: the 20 values of SPECIALS, for the one-argument functions and as a 20 x 20 grid for atan2f_ and powf_, against libm
(O.MATH_LIBM): the NaN pattern, the infinities, the sign of zero, and the value to 4 ulp.  The deliberate differences from libm are
documented in the header and asserted here as documented: sinf_ / cosf_ / tanf_ of |x| >= 1e6 are NaN (libm reduces any finite
argument), at 999999.9 they are only finite (and sin / cos in [-1, 1]), sinf_(-0.0) = tanf_(-0.0) = +0.0 (libm: -0.0; the sign costs
an operation on the path every call takes), and 7 cells of powf_'s grid: powf_(-inf, y) = NaN for y in {+-0.5, 2.5, +-1e-45, 999999.9}
(libm: +inf for y > 0, +0 for y < 0) and powf_(-1, -inf) = +inf (libm: 1).  Handling the infinities before the negative-base test makes
all 400 cells agree, but changes the VGPR count of two k_shade instances (113 -> 112) and of k_photon_emit<true> (123 -> 121), which
inline powf_; so the order stayed and the 7 cells are documented.  sqrtf of a subnormal is never subnormal (sqrt(2^-149) = 2^-74.5), so the GPU edge set is
asked for subnormal inputs AND subnormal results of fn 0, 4, 6 and 8, and for subnormal inputs with normal results of fn 9.
"""
import math

import numpy as np
import pytest

from conftest import same_bits
from test_detmath import ulp_diff

f32 = np.float32
N = 400000
FLT_MAX = np.finfo(f32).max
FLT_MIN = np.finfo(f32).tiny
DENORM_MIN = f32(2.0 ** -149)
INF = f32(np.inf)
NAN = f32(np.nan)
SIN, COS, TAN, ACOS, ASIN, ATAN2, POW, RAND, DIV, SQRT = range(10)

# +-0, +-inf, NaN, +-1, +-0.5, +-2, 3, 2.5, -3, +-1e-45, 3.4e38, +-1e6, 999999.9
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1, -1, 0.5, -0.5, 2, -2, 3, 2.5, -3, 1e-45, -1e-45, 3.4e38, 1e6, -1e6, 999999.9], f32)


def ulp_err(dev, ref64):
    """|dev - ref| in ulps of the float32-rounded reference."""
    with np.errstate(over="ignore"):  # a float64 reference beyond FLT_MAX rounds to inf; the callers mask those
        sp = np.spacing(np.abs(ref64.astype(f32))).astype(np.float64)
    return np.abs(dev.astype(np.float64) - ref64) / sp


def is_subnormal(a):
    a = np.asarray(a, f32)
    return (a != 0) & (np.abs(a) < FLT_MIN)


def asin_sets(rng):
    return np.concatenate([rng.uniform(-1, 1, N), 1 - np.exp(rng.uniform(-30, 0, N)), -1 + np.exp(rng.uniform(-30, 0, N)),
                           np.exp(rng.uniform(-100, 0, N))])


def scaled_normals(rng):
    return rng.standard_normal(N) * np.exp(rng.uniform(-40, 40, N))


# (name, fn, float64 reference, first argument, second argument or None, measured maximum in ulp)
ACCURACY = [
    ("sin8", SIN, np.sin, lambda r: r.uniform(-8, 8, N), None, 1.457),
    ("cos8", COS, np.cos, lambda r: r.uniform(-8, 8, N), None, 1.451),
    ("sin100", SIN, np.sin, lambda r: r.uniform(-100, 100, N), None, 1.467),
    ("cos100", COS, np.cos, lambda r: r.uniform(-100, 100, N), None, 3.948),
    ("tan", TAN, np.tan, lambda r: r.uniform(-1.5707, 1.5707, N), None, 2.835),
    ("acos", ACOS, np.arccos, asin_sets, None, 1.249),
    ("asin", ASIN, np.arcsin, asin_sets, None, 2.350),
    ("atan2", ATAN2, np.arctan2, scaled_normals, scaled_normals, 2.717),
]


@pytest.mark.parametrize("name,fn,ref,ga,gb,measured", ACCURACY, ids=[c[0] for c in ACCURACY])
def test_accuracy_against_float64(name, fn, ref, ga, gb, measured, O):
    rng = np.random.default_rng(0)
    a = ga(rng).astype(f32)
    b = gb(rng).astype(f32) if gb else None
    dev = O.math_eval(fn, O.MATH_DEVICE, a, b)
    r64 = ref(a.astype(np.float64)) if b is None else ref(a.astype(np.float64), b.astype(np.float64))
    assert np.isfinite(dev).all() and np.isfinite(r64).all()
    e = ulp_err(dev, r64)
    k = int(np.argmax(e))
    print(f"\n{name}: max {e.max():.3f} ulp at a={a[k]!r}" + ("" if b is None else f" b={b[k]!r}") + f" ({a.size} points)")
    assert e.max() <= math.ceil(measured + 0.5), f"{name}: {e.max():.3f} ulp at a={a[k]!r}"


def test_powf_against_float64(O):
    """Normal results within 1 ulp, subnormal results within one unit of 2^-149, every overflowing result +inf."""
    rng = np.random.default_rng(0)
    x = np.exp(rng.uniform(-80, 80, N)).astype(f32)
    y = rng.uniform(-40, 40, N).astype(f32)
    dev = O.math_eval(POW, O.MATH_DEVICE, x, y)
    with np.errstate(over="ignore", under="ignore"):
        r64 = np.power(x.astype(np.float64), y.astype(np.float64))
        r32 = r64.astype(f32)
    over, sub = np.isinf(r32), r64 < float(FLT_MIN)
    normal = ~over & ~sub
    assert over.sum() > 1000 and sub.sum() > 1000 and normal.sum() > 1000
    e = ulp_err(dev[normal], r64[normal])
    es = np.abs(dev[sub].astype(np.float64) - r64[sub]) / float(DENORM_MIN)
    print(f"\npowf_: normal max {e.max():.3f} ulp ({normal.sum()}), subnormal max {es.max():.3f} units of 2^-149 ({sub.sum()}, "
          f"{np.count_nonzero(is_subnormal(dev[sub]))} of them nonzero), overflowing {over.sum()}")
    assert e.max() <= 1.0
    assert es.max() <= 1.0
    assert np.count_nonzero(is_subnormal(dev[sub])) > 100  # the subnormal class is not only zeros
    assert np.all(dev[over] == INF)


def test_sincos_domain(O):
    """Where 'sin and cos of x' holds: 1e-7 absolute up to 1e4, a bounded finite value up to 1e6, NaN from there on."""
    rng = np.random.default_rng(0)
    x = rng.uniform(-1e4, 1e4, N).astype(f32)
    for fn, ref in ((SIN, np.sin), (COS, np.cos)):
        err = np.abs(O.math_eval(fn, O.MATH_DEVICE, x).astype(np.float64) - ref(x.astype(np.float64)))
        print(f"\nfn {fn}: |x| <= 1e4 max abs error {err.max():.3e}")
        assert err.max() <= 1e-7
    below_1e6 = np.nextafter(f32(1e6), f32(0))
    for lo, hi in ((1e4, 1e5), (1e5, float(below_1e6))):
        x = (rng.uniform(lo, hi, N) * rng.choice([-1.0, 1.0], N)).astype(f32)
        x = np.concatenate([x, np.array([lo, -lo, hi, -hi], f32)])
        x = x[np.abs(x) > f32(1e4)]
        for fn, ref in ((SIN, np.sin), (COS, np.cos)):
            d = O.math_eval(fn, O.MATH_DEVICE, x)
            print(f"fn {fn}: {lo:g} <= |x| <= {hi:g} max abs error {np.abs(d.astype(np.float64) - ref(x.astype(np.float64))).max():.3e}")
            assert np.isfinite(d).all() and np.all(np.abs(d) <= 1)
    out = np.array([1e6, np.nextafter(f32(1e6), INF), 1e7, 2.0 ** 20, 2.0 ** 24, 1e30, FLT_MAX, np.inf], f32)
    out = np.concatenate([out, -out, [NAN]])
    for fn in (SIN, COS, TAN):
        assert np.isnan(O.math_eval(fn, O.MATH_DEVICE, out)).all()
    assert np.isfinite(O.math_eval(SIN, O.MATH_DEVICE, np.array([below_1e6, -below_1e6], f32))).all()


def test_callers_range_is_inside_the_accurate_domain(O):
    """The callers' angles (the module docstring lists them) lie in [0, 2 pi]: there sin and cos hold 1e-7 absolute and 2 ulp (the
    +-8 case above contains the range), and the largest such float is far below the 1e4 of the absolute bound."""
    two_pi = f32(2 * math.pi)  # what (float)(rnd01 * 2 * pi) and ((float)M_PI * 2) * u reach at most
    assert 0 <= two_pi < 8 < 1e4
    x = np.concatenate([np.linspace(0, float(two_pi), 100001).astype(f32), [two_pi]])
    for fn, ref in ((SIN, np.sin), (COS, np.cos)):
        err = np.abs(O.math_eval(fn, O.MATH_DEVICE, x).astype(np.float64) - ref(x.astype(np.float64)))
        assert err.max() <= 1e-7


def assert_like_libm(dev, ref, what):
    """NaN pattern, infinities, the sign of zero, and the value to 4 ulp."""
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), f"{what}: NaN pattern\n{dev}\n{ref}"
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isinf(dev[ok]), np.isinf(ref[ok])), f"{what}: infinities\n{dev}\n{ref}"
    assert np.array_equal(np.signbit(dev[ok]), np.signbit(ref[ok])), f"{what}: signs (of zero)\n{dev}\n{ref}"
    assert np.array_equal(dev[ok] == 0, ref[ok] == 0), f"{what}: zeros\n{dev}\n{ref}"
    assert ulp_diff(dev[ok], ref[ok]).max() <= 4, f"{what}: more than 4 ulp\n{dev}\n{ref}"


@pytest.mark.parametrize("fn", [SIN, COS, TAN, ACOS, ASIN])
def test_special_values_one_argument(fn, O):
    x = SPECIALS
    dev, ref = O.math_eval(fn, O.MATH_DEVICE, x), O.math_eval(fn, O.MATH_LIBM, x)
    if fn in (SIN, COS, TAN):  # the documented differences from libm: the domain ends at 1e6, and -0.0 gives +0.0
        outside = np.abs(x) >= f32(1e6)  # +-1e6, 3.4e38, +-inf (libm: NaN for the infinities as well)
        assert np.isnan(dev[outside]).all()
        edge = x == f32(999999.9)  # inside the domain, outside the accurate range: finite, sin and cos bounded
        assert np.isfinite(dev[edge]).all() and (fn == TAN or np.all(np.abs(dev[edge]) <= 1))
        rest = ~outside & ~edge
        minus_zero = (x == 0) & np.signbit(x)
        if fn != COS:
            assert same_bits(dev[minus_zero], np.array([0.0], f32)), "sinf_ / tanf_ of -0.0: the header documents +0.0"
            assert same_bits(ref[minus_zero], np.array([-0.0], f32))
            rest &= ~minus_zero
        dev, ref = dev[rest], ref[rest]
    assert_like_libm(dev, ref, f"fn {fn}")


@pytest.mark.parametrize("fn", [ATAN2, POW])
def test_special_values_grid(fn, O):
    """The 20 x 20 grid agrees with libm: atan2f_ in all 400 cells, powf_ in all but the 7 that fall under its two documented differences
    (powf_(-inf, finite non-integer y) = NaN, powf_(-1, -inf) = +inf), which hold the documented values."""
    a, b = [g.reshape(-1).copy() for g in np.meshgrid(SPECIALS, SPECIALS, indexing="ij")]
    dev, ref = O.math_eval(fn, O.MATH_DEVICE, a, b), O.math_eval(fn, O.MATH_LIBM, a, b)
    if fn == POW:
        nan_cells = (a == -INF) & np.isfinite(b) & (b != np.trunc(b))
        inf_cell = (a == -1) & (b == -INF)
        assert nan_cells.sum() == 6 and inf_cell.sum() == 1
        assert np.isnan(dev[nan_cells]).all() and np.all(dev[inf_cell] == INF)
        assert np.array_equal(ref[nan_cells], np.where(b[nan_cells] > 0, INF, f32(0))) and np.all(ref[inf_cell] == 1)  # what libm says there
        keep = ~(nan_cells | inf_cell)
        a, b, dev, ref = a[keep], b[keep], dev[keep], ref[keep]
    bad = ~((np.isnan(dev) & np.isnan(ref)) | (~np.isnan(dev) & ~np.isnan(ref) & (np.signbit(dev) == np.signbit(ref)) & (np.isinf(dev) == np.isinf(ref))
                                                & ((dev == 0) == (ref == 0)) & (ulp_diff(dev, ref) <= 4)))
    cells = [f"({a[k]!r}, {b[k]!r}): {dev[k]!r}, libm {ref[k]!r}" for k in np.flatnonzero(bad)]
    assert not cells, f"fn {fn}: {len(cells)} cells differ from libm: " + "; ".join(cells)
    assert_like_libm(dev, ref, f"fn {fn}")


# ---- the deterministic edge set of the GPU test ---------------------------------------------------------------------------------------
def neighbours(values, reach=2):
    """Every value with its +-1 .. +-reach ulp neighbours."""
    out = []
    for v in np.asarray(values, f32):
        lo = hi = v
        out.append(v)
        for _ in range(reach):
            lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
            out += [lo, hi]
    return np.array(out, f32)


def subnormals():
    s = np.concatenate([[FLT_MIN, FLT_MIN / 2, 1e-45], np.exp(np.linspace(np.log(1.5e-45), np.log(1.17e-38), 64))]).astype(f32)
    return np.concatenate([s, -s])


def one_argument_set():
    # the header's branch constants: asin / acos (0.5, 1), atan (tan(pi/8), tan(3pi/8)), sincos_f (1e6), exp_d (709, -745), log_pos_d (sqrt 2)
    branch = np.array([0.5, 1.0, 0.4142135623730950, 2.414213562373095, 1e6, 709.0, 745.0, 1.41421356237309504880], f32)
    branch = neighbours(np.concatenate([branch, -branch]))
    quarter_turns = neighbours((np.arange(65) * (np.pi / 2)).astype(f32), reach=1)
    points = np.array([999999.9, 1e6, 0.0, -0.0, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, -999999.9, -1e6], f32)
    return np.concatenate([branch, quarter_turns, -quarter_turns, points, subnormals()])


def grid():
    return [g.reshape(-1).copy() for g in np.meshgrid(SPECIALS, SPECIALS, indexing="ij")]


def pairs(a, b):
    """The cross product of two value lists as two flat arrays."""
    return [g.reshape(-1).copy() for g in np.meshgrid(np.asarray(a, f32), np.asarray(b, f32), indexing="ij")]


def division_set():
    sub = subnormals()
    normal = np.array([1, -3, 0.7, 1e-3, 1.5e10, 7e37], f32)
    huge = np.array([1e30, -3e35, FLT_MAX, 2.0 ** 100], f32)
    ga, gb = grid()
    s_a, s_b = pairs(sub, normal)  # subnormal / normal
    n_a, n_b = pairs(np.array([1e-10, -3e-8, 1.0, 7e-3, FLT_MIN, 5e-38], f32), huge)  # normal / huge: subnormal (or zero) quotients
    # (d * FLT_MIN - 1 ulp) / d = FLT_MIN - 2^-149 * 2^floor(log2 d) / d.  d a power of two: FLT_MIN - 2^-150, the tie that rounds (to even) UP to
    # FLT_MIN; any other d: past the tie (1000: 0.512 units), down to the largest subnormal.  The first eight of each sign are the ties.
    d = np.array([2, 4, 8, 16, 1024, 2.0 ** 20, 2.0 ** 60, 2.0 ** 100, 3, 5, 7, 1000], f32)
    r_a = np.nextafter((d * FLT_MIN).astype(f32), f32(0))
    return np.concatenate([ga, s_a, n_a, r_a, -r_a]), np.concatenate([gb, s_b, n_b, d, d])


def pow_set():
    e = f32(2.7182818)  # the absorption call's base (device_shade.h: powf_(e, -absorption * distance))
    ga, gb = grid()
    xs, ys = [ga], [gb]

    def add(x, y):
        x, y = pairs(x, y)
        xs.append(x)
        ys.append(y)
    steps = np.concatenate([np.arange(-151, -124.9, 0.25), np.arange(126, 129.1, 0.25)])
    add([2], steps)  # subnormal results and the overflow boundary
    add(subnormals()[:67], [0.5, -0.5, 1, -1, 2, -2, 0.25, 1 / 2.2, 3, 1e-3])
    add([e], [-745, -709, -104, -103.9, -87.4, -87.3])
    for x in (e, f32(2), f32(10), f32(0.5), f32(1e-3)):  # y * log x straddling exp_d's clamps at 709 and -745
        lx = math.log(float(x))
        add([x], neighbours(np.array([709 / lx, -709 / lx, -745 / lx, 745 / lx], f32)))
    neg = np.array([-0.5, -1, -2, -3, -1e-45, -1e6, -np.inf, -0.0, -FLT_MIN / 2, -FLT_MAX], f32)
    ints = np.concatenate([np.arange(-6, 6.1, 0.5), [8388607.5, 8388608, 16777215, 16777216, 2.0 ** 52, 2.0 ** 53, 2.0 ** 60, FLT_MAX,
                                                     -8388607.5, -16777215, -16777216, -(2.0 ** 53), -FLT_MAX]])
    add(neg, ints)  # integral and half-integral exponents of negative bases
    return np.concatenate(xs), np.concatenate(ys)


def edge_cases():
    """(fn, a, b) of the GPU test."""
    one = one_argument_set()
    cases = [(fn, one, None) for fn in (SIN, COS, TAN, ACOS, ASIN, SQRT)]
    ga, gb = grid()
    cases.append((ATAN2, np.concatenate([ga, pairs(subnormals(), [1, -1e-40, 1e30, 0])[0]]), np.concatenate([gb, pairs(subnormals(), [1, -1e-40, 1e30, 0])[1]])))
    cases.append((POW,) + pow_set())
    cases.append((RAND, np.array([0, 1, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1], np.uint32).view(f32), None))
    cases.append((DIV,) + division_set())
    return cases


def test_edge_set_is_not_vacuous(O):
    """The set reaches what it is for: subnormal operands and subnormal results, the FLT_MIN round-up, both sides of every clamp."""
    seen = {}
    for fn, a, b in edge_cases():
        assert a.dtype == f32 and (b is None or (b.dtype == f32 and b.shape == a.shape))
        host = O.math_eval(fn, O.MATH_DEVICE, a, b)
        sub_in = is_subnormal(a) | (is_subnormal(b) if b is not None else False)
        seen[fn] = (np.count_nonzero(sub_in), np.count_nonzero(is_subnormal(host)), a.size)
        if fn == SQRT:  # sqrt(2^-149) = 2^-74.5: a subnormal argument always has a normal root
            assert sub_in.any() and not is_subnormal(host[sub_in]).any() and np.all(host[sub_in & (a > 0)] >= f32(2.0 ** -75))
        if fn == DIV:
            q = np.abs(host[-24:]).reshape(2, 12)
            assert np.all(q[:, :8] == FLT_MIN) and np.all(q[:, 8:] == np.nextafter(FLT_MIN, f32(0)))  # the ties round up to FLT_MIN
        if fn == POW:
            assert np.count_nonzero(host == INF) > 10 and np.count_nonzero(host == 0) > 10 and np.count_nonzero(host == FLT_MAX) == 0
            two = a == 2
            assert host[two & (b == -149)][0] == DENORM_MIN and host[two & (b == 127.75)][0] < INF and host[two & (b == 128)][0] == INF
    for fn in (SIN, ASIN, POW, DIV):
        assert seen[fn][0] > 0 and seen[fn][1] > 0, f"fn {fn}: {seen[fn]}"
    assert max(v[2] for v in seen.values()) < 8000  # "a few thousand elements per function"


@pytest.mark.gpu
def test_device_bits_equal_host_bits_on_the_edges(B, O):
    """gfx950 and x86-64 give the same bits on branch points, subnormal operands and results, clamps and special values."""
    if B.device_count() < 1:
        pytest.fail("no HIP device")
    for fn, a, b in edge_cases():
        dev = B.math_eval_dev(fn, a, b)
        host = O.math_eval(fn, O.MATH_DEVICE, a, b)
        same = (dev.view(np.uint32) == host.view(np.uint32)) | (np.isnan(dev) & np.isnan(host))
        assert same.all(), (f"fn {fn}: {np.count_nonzero(~same)} of {a.size} differ, e.g. a={a[~same][:4]!r} b={None if b is None else b[~same][:4]!r} "
                            f"dev={dev[~same][:4]!r} host={host[~same][:4]!r}")
