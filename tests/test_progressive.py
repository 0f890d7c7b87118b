"""Progressive rendering (bhrt_progressive_*): the frame as a session that steps advance and that can be read at any point.

The guarantees under test: a uniform session's frame at count c is bhrt_render's at spp = c, bit for bit; a session stepped on the doubling
schedule is bhrt_render_adaptive's frame; off the schedule every count is what the fold and the retirement test of include/bhrt.h give,
restated below in numpy float32 from the per-sample radiance of bhrt_render_samples; and nothing else the library does on the scene between
two steps shows in the frame."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENES, same_bits

f32 = np.float32
LUM = (f32(0.2126), f32(0.7152), f32(0.0722))
SCENES3 = ["c3_room_small", "c2_glass_small", "c3_mesh_small"]
STEPS = (1, 2, 5)  # test 1's session: counts 1, 3, 8


def opts1(B, **kw):
    return B.default_opts(**dict(dict(spp=8, gi_bounces=3, seed=5), **kw))


@pytest.fixture
def scene(B):
    """Private scene handles, freed with their device state (an open session included) when the test ends."""
    opened = []

    def _load(name):
        opened.append(B.Scene(os.path.join(SCENES, name + ".xml")))
        return opened[-1]
    yield _load
    for sc in opened:
        sc.close()


@pytest.fixture(scope="module")
def uniform_ref(B):
    """What test 1's session must show, by the blocking entry points: name -> {1, 3, 8: (rgb8, radiance)} of bhrt_render and "var": the variance
    of bhrt_render_adaptive(min_spp = 2, threshold = -1) at 8.  Computed once per scene, on a handle of its own, and never written to."""
    cache = {}

    def _ref(name):
        if name not in cache:
            sc = B.Scene(os.path.join(SCENES, name + ".xml"))
            try:
                ref = {}
                for n in np.cumsum(STEPS).tolist():
                    rgb, rad, _ = sc.render(opts1(B, spp=n))
                    ref[n] = (rgb, rad)
                ref["var"] = sc.render_adaptive(opts1(B), B.default_adaptive_opts(min_spp=2, threshold=-1.0))[2]
                for a in list(ref[1]) + list(ref[3]) + list(ref[8]) + [ref["var"]]:
                    a.setflags(write=False)
                cache[name] = ref
            finally:
                sc.close()
        return cache[name]
    return _ref


def frames_equal(a, b):
    """(rgb8, radiance, variance, count) tuples: bytes and bits."""
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and np.array_equal(a[3], b[3])


def session_counts_ref(samples, steps, n_min, n_max, threshold, floor):
    """The fold and the retirement test of a session on samples (pixels, >= n_max, 3) float32, in the kernel's operations and order: the
    recurrence runs over every sample, the test where a step ends (at the running totals of `steps`, capped at n_max) once n >= n_min."""
    P = samples.shape[0]
    S, mu, M2 = (np.zeros((P, 3), f32) for _ in range(3))
    cnt = np.zeros(P, np.uint32)
    active = np.ones(P, bool)
    stops = set(min(n_max, int(t)) for t in np.cumsum(steps))
    thr, fl = f32(threshold), f32(floor)
    for k in range(1, n_max + 1):
        x = samples[:, k - 1].astype(f32)
        S = S + x
        d = x - mu
        mu = mu + d / f32(k)
        M2 = M2 + d * (x - mu)
        if k in stops:
            retire = np.full(P, k >= n_max)
            if n_min <= k < n_max:
                m = S / f32(k)
                v = (M2 / f32(k - 1)) / f32(k)
                L = (LUM[0] * m[:, 0] + LUM[1] * m[:, 1]) + LUM[2] * m[:, 2]
                vL = ((LUM[0] * LUM[0]) * v[:, 0] + (LUM[1] * LUM[1]) * v[:, 1]) + (LUM[2] * LUM[2]) * v[:, 2]
                with np.errstate(invalid="ignore"):
                    retire = np.sqrt(vL) <= thr * np.fmax(L, fl)
            retire &= active
            cnt[retire] = k
            active &= ~retire
    assert not active.any()
    return cnt


# ---- CPU: the struct and the argument checks (before any device is touched) -------------------------------------------------------------
def test_progress_struct_matches_header(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    body = re.search(r"typedef struct bhrt_progress \{(.*?)\} bhrt_progress;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size_of = {"uint32_t": 4, "int32_t": 4, "uint64_t": 8}
    names, off, align = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        typ, rest = decl.split(None, 1)
        for item in rest.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", item.strip())
            sz = size_of[typ]
            off = (off + sz - 1) // sz * sz
            assert getattr(B.Progress, m.group(1)).offset == off, m.group(1)
            names.append(m.group(1))
            off += sz * int(m.group(2) or 1)
            align = max(align, sz)
    assert names == [n for n, _ in B.Progress._fields_]
    assert C.sizeof(B.Progress) == (off + align - 1) // align * align == 48


def test_calls_without_a_session_are_refused(B, scene):
    sc = scene("c3_room_small")
    for call, name in ((lambda: sc.progressive_step(1), "step"), (sc.progressive_frame, "frame"), (sc.progressive_status, "status")):
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: bhrt_progressive_%s.*session" % name):
            call()
    sc.progressive_end()  # OK when none is open
    sc.progressive_begin(opts1(B))
    sc.progressive_end()
    sc.progressive_end()
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*session"):
        sc.progressive_status()


def test_begin_twice_and_bad_step_are_refused(B, scene):
    sc = scene("c3_room_small")
    sc.progressive_begin(opts1(B))
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*session is already open"):
        sc.progressive_begin(opts1(B))
    for n in (0, -3):
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*n_samples"):
            sc.progressive_step(n)
    p = sc.progressive_status()  # begin needs no device: the session stands at zero
    assert (p.steps, p.spp_min, p.spp_max, p.active_pixels, p.camera_samples, p.finished) == (0, 0, 0, sc.width * sc.height, 0, 0)
    sc.progressive_end()
    sc.progressive_begin(opts1(B, rank=1, world_size=2, tile_size=32))  # 320 x 240 in 32-pixel tiles: 10 x 8, the last row 16 high; odd tiles
    assert sc.progressive_status().active_pixels == 5 * 7 * 32 * 32 + 5 * 32 * 16


@pytest.mark.parametrize("okw,akw,msg", [
    (dict(spp=0), None, "spp"),
    (dict(spp=65536), None, "spp"),
    (dict(spp=65536), dict(min_spp=16), "spp"),
    (dict(spp=32), dict(min_spp=1), "min_spp"),
    (dict(spp=8), dict(min_spp=16), "min_spp"),
    (dict(spp=32), dict(floor=0.0), "floor"),
    (dict(spp=32), dict(threshold=float("nan")), "NaN"),
    (dict(spp=8, lens=2), None, "lens"),
])
def test_invalid_options_are_refused_before_the_device(B, scene, okw, akw, msg):
    sc = scene("c1_sphere_plane")
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*" + msg):
        sc.progressive_begin(B.default_opts(**okw), B.default_adaptive_opts(**akw) if akw is not None else None)
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*session"):  # and no session was opened
        sc.progressive_status()


def test_global_gather_without_a_map_is_refused(B, scene):
    sc = scene("c3_room_small")
    sc.set_global_gather(True)
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*global map"):
        sc.progressive_begin(opts1(B))
    sc.set_global_gather(False)
    sc.progressive_begin(opts1(B))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def run_session(B, sc, o, aopts=None, steps=STEPS, between=None):
    """Begins, steps and reads the frame after every step: [(frame, stats, status)]."""
    sc.progressive_begin(o, aopts)
    out = []
    for k, n in enumerate(steps):
        st = sc.progressive_step(n)
        out.append((sc.progressive_frame(), st, sc.progressive_status()))
        if between:
            between(k)
    return out


def check_against_uniform(sc, run, ref, o_spp=8):
    """Test 1's assertions on a run of the STEPS session."""
    W, H = sc.width, sc.height
    for (frame, st, p), n, k in zip(run, np.cumsum(STEPS).tolist(), range(3)):
        rgb, rad, var, cnt = frame
        assert np.array_equal(rgb, ref[n][0]) and same_bits(rad, ref[n][1]), n
        assert (cnt == n).all()
        assert (p.steps, p.spp_min, p.spp_max, p.camera_samples) == (k + 1, n, n, W * H * n)
        assert p.active_pixels == (W * H if n < o_spp else 0) and p.finished == (n == o_spp)
        if n == 1:
            assert not var.any()
    assert same_bits(run[-1][0][2], ref["var"])
    assert sum(st.camera_samples for _, st, _ in run) == W * H * o_spp


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES3)
def test_uniform_session_is_the_uniform_render(B, scene, uniform_ref, name):
    sc = scene(name)
    before_any_step = None
    sc.progressive_begin(opts1(B))
    before_any_step = sc.progressive_frame()
    assert not any(a.any() for a in before_any_step)  # count 0: zeros
    sc.progressive_end()
    run = run_session(B, sc, opts1(B))
    check_against_uniform(sc, run, uniform_ref(name))
    st = sc.progressive_step(4)  # finished: OK, renders nothing, does not count
    assert st.camera_samples == 0 and st.passes == 0
    p = sc.progressive_status()
    assert p.steps == 3 and p.finished == 1
    assert frames_equal(sc.progressive_frame(), run[-1][0])


@pytest.mark.gpu
def test_on_the_doubling_schedule_a_session_is_the_adaptive_render(B, scene):
    sc = scene("c1_sphere_plane")  # its background retires at once, its shaded pixels at every level
    o, a = B.default_opts(spp=32, gi_bounces=3, seed=7), B.default_adaptive_opts(min_spp=4)
    ad = sc.render_adaptive(o, a)
    levels, hist = np.unique(ad[3], return_counts=True)
    assert (hist >= 0.01 * ad[3].size).sum() >= 2, (levels, hist)  # the parent's own frame mixes counts
    run = run_session(B, sc, o, a, steps=(4, 4, 8, 16))
    frame, _, p = run[-1]
    assert frames_equal(frame, ad[:4])
    assert p.finished == 1 and (p.spp_min, p.spp_max) == (int(levels.min()), int(levels.max()))
    assert int(frame[3].sum(dtype=np.uint64)) == sum(st.camera_samples for _, st, _ in run) == p.camera_samples == ad[4].camera_samples
    # in between: the pixels that have retired show their final value, the others the running count
    for (f, _, pk), n in zip(run, (4, 8, 16, 32)):
        assert np.array_equal(f[3], np.minimum(ad[3], n)) and pk.active_pixels == int((ad[3] > n).sum())


@pytest.mark.gpu
def test_off_the_schedule(B, scene):
    sc = scene("c3_room_small")
    H, W = sc.height, sc.width
    o, a = B.default_opts(spp=16, gi_bounces=3, seed=11), B.default_adaptive_opts(min_spp=4, threshold=0.05, floor=0.05)
    run = run_session(B, sc, o, a, steps=(3,) * 6)
    rgb, rad, var, cnt = run[-1][0]
    assert run[-1][2].finished == 1 and run[-2][2].finished == 0
    samples, _ = sc.render_samples(o, 0, 0, W, H)
    ref = session_counts_ref(samples, (3,) * 6, 4, 16, 0.05, 0.05).reshape(H, W)
    assert np.array_equal(cnt, ref), f"{int((cnt != ref).sum())} pixels differ"
    levels = np.unique(cnt).tolist()
    assert set(levels) <= {6, 9, 12, 15, 16} and len(levels) >= 2
    for n in levels:
        sel = cnt == n
        urgb, urad, uvar = sc.render_var(B.default_opts(spp=n, gi_bounces=3, seed=11))
        assert np.array_equal(rgb[sel], urgb[sel]) and same_bits(rad[sel], urad[sel]), n
        assert np.all(np.abs(var[sel] - uvar[sel]) <= 1e-4 * np.abs(uvar[sel]) + 1e-12), n  # the two-pass variance: the session's anchor outside the fold
    assert int(cnt.sum(dtype=np.uint64)) == sum(st.camera_samples for _, st, _ in run)


@pytest.mark.gpu
def test_pass_size_and_overflow_do_not_show(B, scene, uniform_ref):
    name = "c3_mesh_small"
    sc = scene(name)
    run = run_session(B, sc, opts1(B, samples_per_pass=25000))  # 76800 pixels: a step of 1 takes 4 passes, a step of 5 sixteen
    assert all(st.passes >= 3 for _, st, _ in run)
    check_against_uniform(sc, run, uniform_ref(name))
    sc.progressive_end()
    whole = run_session(B, sc, opts1(B))
    sc.progressive_end()
    sc.knob("frame_cap", max(1, int(whole[0][1].shade_calls) // 3))  # the smallest step's frames do not fit: its pass overflows and is redone in halves
    try:
        over = run_session(B, sc, opts1(B))
    finally:
        sc.knob("frame_cap", 0)
    assert all(so.passes > sw.passes for (_, so, _), (_, sw, _) in zip(over, whole))
    check_against_uniform(sc, over, uniform_ref(name))


@pytest.mark.gpu
def test_a_rank_writes_its_own_tiles_only(B, scene, uniform_ref):
    name = "c3_room_small"
    sc, ref = scene(name), uniform_ref(name)
    H, W = sc.height, sc.width
    yy, xx = np.mgrid[0:H, 0:W]
    mine = ((yy // 32) * ((W + 31) // 32) + xx // 32) % 2 == 1
    sc.progressive_begin(opts1(B, rank=1, world_size=2, tile_size=32))
    total = 0
    for n in STEPS:
        total += sc.progressive_step(n).camera_samples
    rgb = np.full((H, W, 3), 0xAB, np.uint8)
    rad, var = np.full((H, W, 3), 123.5, f32), np.full((H, W, 3), 123.5, f32)
    cnt = np.full((H, W), 0xDEADBEEF, np.uint32)
    sc.progressive_frame_into(rgb, rad, var, cnt)
    assert (rgb[~mine] == 0xAB).all() and (rad[~mine] == 123.5).all() and (var[~mine] == 123.5).all() and (cnt[~mine] == 0xDEADBEEF).all()
    assert np.array_equal(rgb[mine], ref[8][0][mine]) and same_bits(rad[mine], ref[8][1][mine]) and same_bits(var[mine], ref["var"][mine])
    assert (cnt[mine] == 8).all()
    p = sc.progressive_status()
    assert total == p.camera_samples == int(mine.sum()) * 8 and p.finished == 1


@pytest.mark.gpu
def test_neighbours_do_not_disturb_it(B, scene, uniform_ref):
    name = "c2_glass_small"
    sc = scene(name)
    kept = {}

    def between(k):
        if k == 0:
            sc.render(B.default_opts(spp=2, gi_bounces=2, seed=99))
            sc.render_adaptive(B.default_opts(spp=16, seed=3), B.default_adaptive_opts(min_spp=4, threshold=0.05, floor=0.05))
        elif k == 1:
            kept["z"] = sc.first_hit()[0]
            _, rad, var = sc.render_var(B.default_opts(spp=2, seed=98))
            sc.denoise(B.default_denoise_opts(), rad, var)
    run = run_session(B, sc, opts1(B), between=between)
    assert kept["z"].shape == (sc.height, sc.width)
    check_against_uniform(sc, run, uniform_ref(name))


@pytest.mark.gpu
def test_lens_passes_through(B, scene):
    sc = scene("lens_spheres")  # <dof> 1.5
    o = B.default_opts(spp=4, gi_bounces=2, seed=3, lens=1)
    frame = run_session(B, sc, o, steps=(2, 2))[-1][0]
    rgb, rad, _ = sc.render(o)
    assert np.array_equal(frame[0], rgb) and same_bits(frame[1], rad)
    assert not same_bits(rad, sc.render(B.default_opts(spp=4, gi_bounces=2, seed=3))[1])  # the lens is in the frame


@pytest.mark.gpu
def test_emission_passes_through_and_setters_apply_to_later_samples(B, scene):
    sc = scene("lens_spheres")
    o = B.default_opts(spp=4, gi_bounces=2, seed=3)
    off = sc.render(o)[1]
    sc.set_material_emission(sc.material_index("ball"), (0.5, 0.25, 0.125))
    sc.set_emissive(True)
    frame = run_session(B, sc, o, steps=(2, 2))[-1][0]
    rgb, rad, _ = sc.render(o)
    assert np.array_equal(frame[0], rgb) and same_bits(frame[1], rad) and not same_bits(rad, off)
    sc.progressive_end()
    # the switch flipped between two steps: samples 0-1 without the term, 2-3 with it
    sc.set_emissive(False)
    sc.progressive_begin(o)
    sc.progressive_step(2)
    sc.set_emissive(True)
    sc.progressive_step(2)
    mixed = sc.progressive_frame()[1]
    s_on = sc.render_samples(o, 0, 0, sc.width, sc.height)[0]
    sc.set_emissive(False)
    s_off = sc.render_samples(o, 0, 0, sc.width, sc.height)[0]
    assert not same_bits(s_on, s_off)
    want = ((((np.zeros_like(s_off[:, 0]) + s_off[:, 0]) + s_off[:, 1]) + s_on[:, 2]) + s_on[:, 3]) / f32(4)
    assert same_bits(mixed.reshape(-1, 3), want)


@pytest.mark.gpu
def test_photon_map_passes_through(B, scene):
    sc = scene("c5_caustics")
    o = B.default_opts(spp=4, gi_bounces=2, seed=3, photon_map=1, photon_exact=1)
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*photon_map"):
        sc.progressive_begin(o)  # no map yet
    assert sc.photon_build(B.default_opts(), 20000) > 0
    run = run_session(B, sc, o, steps=(1, 3))
    rgb, rad, _ = sc.render(o)
    assert np.array_equal(run[-1][0][0], rgb) and same_bits(run[-1][0][1], rad)
    assert sum(st.photon_queries for _, st, _ in run) > 0


@pytest.mark.gpu
def test_resolve_on_demand(B, scene):
    import torch
    sc = scene("c3_mesh_small")
    H, W = sc.height, sc.width
    sc.progressive_begin(opts1(B))
    sc.progressive_step(3)
    first, second = sc.progressive_frame(), sc.progressive_frame()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second))
    dev = torch.device("cuda", 0)
    d_rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    d_rad, d_var = (torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
    d_cnt = torch.zeros((H, W), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    sc.progressive_frame_dev(d_rgb.data_ptr(), d_rad.data_ptr(), d_var.data_ptr(), d_cnt.data_ptr(), s.cuda_stream)
    s.synchronize()
    got = (d_rgb.cpu().numpy(), d_rad.cpu().numpy(), d_var.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32))
    assert frames_equal(got, first)
    d_rad.zero_()
    sc.progressive_frame_dev(d_radiance_ptr=d_rad.data_ptr())  # any pointer may be NULL; no stream: synchronised
    assert same_bits(d_rad.cpu().numpy(), first[1])


@pytest.mark.gpu
def test_upload_elsewhere_is_refused_while_the_session_holds_state(B, scene, uniform_ref):
    """The session's state is device memory of the device the scene is uploaded to: a move that would drop it is an argument error that changes
    nothing (refused before a device is looked for, so one device is enough to see it), and the session goes on."""
    name = "c3_mesh_small"
    sc = scene(name)
    sc.upload(0)
    sc.progressive_begin(opts1(B))
    sc.progressive_step(1)
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: bhrt_scene_upload.*session.*device 0"):
        sc.upload(1)
    sc.upload(0)  # the same device: the no-op it always was
    for n in STEPS[1:]:
        sc.progressive_step(n)
    ref = uniform_ref(name)
    rgb, rad, var, cnt = sc.progressive_frame()
    assert np.array_equal(rgb, ref[8][0]) and same_bits(rad, ref[8][1]) and same_bits(var, ref["var"]) and (cnt == 8).all()


@pytest.mark.gpu
def test_a_refused_step_leaves_the_session_usable_and_a_failed_one_does_not(B, scene, uniform_ref):
    name = "c3_room_small"
    sc, ref = scene(name), uniform_ref(name)
    sc.progressive_begin(opts1(B))
    sc.progressive_step(1)
    sc.set_global_gather(True)  # no global map: the step's argument checks refuse it, nothing is rendered
    with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*global map"):
        sc.progressive_step(2)
    sc.set_global_gather(False)
    assert sc.progressive_status().steps == 1
    sc.progressive_step(2)
    rgb, rad, _, _ = sc.progressive_frame()
    assert np.array_equal(rgb, ref[3][0]) and same_bits(rad, ref[3][1])
    sc.knob("frame_cap", 1)  # no pixel of the closed room fits one Shade() frame: the step's passes halve down to one pixel and give up
    try:
        with pytest.raises(B.BhrtError, match=r"bhrt error 7: .*overflow"):
            sc.progressive_step(5)
    finally:
        sc.knob("frame_cap", 0)
    for call in (lambda: sc.progressive_step(5), sc.progressive_frame):
        with pytest.raises(B.BhrtError, match=r"bhrt error 3: .*a step of this session failed"):
            call()
    p = sc.progressive_status()
    assert (p.steps, p.spp_max, p.finished) == (2, 3, 0)  # the last complete step
    sc.progressive_end()
    sc.progressive_begin(opts1(B))  # a new session on the same scene starts from nothing
    assert not sc.progressive_frame()[3].any()
