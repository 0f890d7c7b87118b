"""Lights of a loaded scene: bhrt_scene_light_count, _light_index, _get_light and _set_light.

The setter's stated property is checked against the loader itself: the blob after an edit is the blob of the edited scene file, written with
%.9g values (which round-trip a float32) — <intensity r g b> with no value=, <position> / <direction> with the caller's un-normalised vector,
<size value>.  Every comparison is bit for bit; the expected value is always a fresh load of the edited XML, never the code under test.  The
oracle and the kernels evaluate the blob and what the upload derives from it, so an edited scene needs no new oracle code."""
import ctypes as C
import os
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from conftest import ROOT, SCENES, same_bits

f32 = np.float32
NAN, INF = float("nan"), float("inf")
FOUR = "lights_four"
NAMES = ["key", "sun", "amb", "fill"]          # document order
KEY, SUN, AMB, FILL = range(4)
KINDS = [2, 1, 0, 2]                           # BHRT_LIGHT_POINT, _DIRECT, _AMBIENT, _POINT
BLOB_INDEX = [2, 1, 0, 3]                      # ascending Gray(): amb 0.1, sun 0.5, key 150, fill 150 (the tie keeps document order here)
# (name, intensity, vec, size): values no shorter decimal states exactly (%.9g must carry them)
MOVE_POINT = ("key", None, (4.0 / 3.0, -7.1, 17.3), None)
RESIZE = ("fill", None, None, 1.0 / 3.0)
TURN_DIRECT = ("sun", None, (-0.3, 1.7, -2.2), None)              # un-normalised
DIM_AMBIENT = ("amb", (0.07, 0.2 / 3.0, 0.11), None, None)
# the direct term picks light l where a draw is <= Gray_l / all_light_intensity (MtlBlinn.cpp:304-351): at Gray() 0.1 of 300.6 a small frame
# never picks amb, so the rendered ambient edit raises it to where a quarter of the draws do (it passes sun on the way: places 0 and 1 swap)
RAISE_AMBIENT = ("amb", (120.0, 90.5, 100.1), None, None)
REORDER = ("key", (0.03, 0.01, 0.05), None, None)                 # Gray() 0.03: key goes from place 2 to place 0, amb and sun move up
MAKE_TIE = ("sun", (0.1, 0.1, 0.1), None, None)                   # Gray() of amb, which stands later in the document
BREAK_TIE = ("fill", (150.0, 150.0, 149.0), None, None)           # below key now: the tied pair swaps
EDITS = {"move_point": MOVE_POINT, "resize": RESIZE, "turn_direct": TURN_DIRECT, "dim_ambient": DIM_AMBIENT, "raise_ambient": RAISE_AMBIENT,
         "reorder": REORDER, "make_tie": MAKE_TIE, "break_tie": BREAK_TIE}
RENDERED = ["move_point", "resize", "turn_direct", "raise_ambient", "reorder"]


def edited_xml(tmp_path, name, edits, tag="edit"):
    """tests/scenes/<name>.xml with the values of `edits` written into the first <light name=> of each, replacing the children of that tag:
    <intensity r g b> (no value=), <position x y z> (point) or <direction x y z> (direct), <size value>; written into tmp_path."""
    tree = ET.parse(os.path.join(SCENES, name + ".xml"))
    g = lambda x: "%.9g" % f32(x)  # noqa: E731
    for light, intensity, vec, size in edits:
        el = next(e for e in tree.getroot().iter("light") if e.get("name") == light)

        def put(tag_, **attrs):
            for c in [c for c in el if c.tag == tag_]:
                el.remove(c)
            ET.SubElement(el, tag_, **attrs)
        if intensity is not None:
            put("intensity", r=g(intensity[0]), g=g(intensity[1]), b=g(intensity[2]))
        if vec is not None:
            put({"point": "position", "direct": "direction"}[el.get("type")], x=g(vec[0]), y=g(vec[1]), z=g(vec[2]))
        if size is not None:
            put("size", value=g(size))
    path = os.path.join(str(tmp_path), f"{name}_{tag}.xml")
    tree.write(path)
    return path


def apply(sc, edit):
    name, intensity, vec, size = edit
    sc.set_light(sc.light_index(name), intensity, vec, -1.0 if size is None else size)


def record(sc, k):
    """get_light's record as a tuple of bytes and ints: what a refusal must leave unchanged."""
    i = sc.light(k)
    return (i.type, bytes(i.intensity), bytes(i.vec), bytes(C.c_float(i.size)), i.blob_index, tuple(i.reserved))


@pytest.fixture
def scene(B):
    """Private scene handles, freed with their device state when the test ends (the setter changes a scene: nothing shared)."""
    opened = []

    def _load(name):
        path = name if os.path.isabs(name) else os.path.join(SCENES, name + ".xml")
        opened.append(B.Scene(path))
        return opened[-1]
    yield _load
    for sc in opened:
        sc.close()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("bhrt_scene_light_count", "bhrt_scene_light_index", "bhrt_scene_get_light", "bhrt_scene_set_light")


def test_symbols_exported_declared_and_wrapped(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in SYMBOLS:
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr), s
    for w in ("light_count", "light_index", "light", "set_light"):
        assert callable(getattr(B.Scene, w))
    assert C.sizeof(B.LightInfo) == 56 and "DESIGN.md 26" in hdr and "} bhrt_light_info;" in hdr
    assert (B.LIGHT_AMBIENT, B.LIGHT_DIRECT, B.LIGHT_POINT) == (0, 1, 2)


def test_count_index_and_get_light(B, scene):
    sc = scene(FOUR)
    assert sc.light_count() == sc.info.n_lights == 4
    assert [sc.light_index(n) for n in NAMES] == [0, 1, 2, 3]
    for bad in ("nobody", "", "Key"):
        with pytest.raises(B.BhrtError, match="bhrt error 3: bhrt_scene_light_index"):
            sc.light_index(bad)
    L = B.lib()
    i, n = C.c_int32(7), C.c_int32(7)
    assert L.bhrt_scene_light_index(sc._h, None, C.byref(i)) == 3 and L.bhrt_scene_light_index(None, b"key", C.byref(i)) == 3
    assert L.bhrt_scene_light_index(sc._h, b"key", None) == 3 and i.value == 7
    assert L.bhrt_scene_light_count(None, C.byref(n)) == 3 and L.bhrt_scene_light_count(sc._h, None) == 3 and n.value == 7
    info = B.LightInfo()
    assert L.bhrt_scene_get_light(None, 0, C.byref(info)) == 3 and L.bhrt_scene_get_light(sc._h, 0, None) == 3
    for bad in (-1, 4):
        with pytest.raises(B.BhrtError, match="bhrt error 3: bhrt_scene_get_light"):
            sc.light(bad)
    got = [sc.light(k) for k in range(4)]
    assert [x.type for x in got] == KINDS and [x.blob_index for x in got] == BLOB_INDEX
    assert all(tuple(x.reserved) == (0,) * 5 for x in got)
    blob = sc.flat_view().lights
    for x in got:                                                # the record is the blob's, where blob_index says
        b = blob[x.blob_index]
        assert (x.type, bytes(x.intensity), bytes(x.vec), bytes(C.c_float(x.size))) == (b.type, bytes(b.intensity), bytes(b.vec), bytes(C.c_float(b.size)))
    # the values, as the loader reads them
    assert same_bits(list(got[KEY].intensity), [300, 150, 0]) and same_bits(list(got[KEY].vec), [0, -10, 20]) and got[KEY].size == 0
    d = np.float32([1, 2, -3])
    assert same_bits(list(got[SUN].vec), d / np.sqrt((d * d).sum(dtype=f32), dtype=f32)) and same_bits(list(got[SUN].intensity), [0.5] * 3)
    assert same_bits(list(got[AMB].intensity), [0.1] * 3) and same_bits(list(got[AMB].vec), [0, 0, 0]) and got[AMB].size == 0
    assert same_bits(list(got[FILL].vec), [12, -6, 9]) and got[FILL].size == 0.5
    # a scene with one light, and names are those of the <light> elements
    c1 = scene("c1_sphere_plane")
    assert c1.light_count() == 1 and c1.light_index("pointLight") == 0 and c1.light(0).blob_index == 0


@pytest.mark.parametrize("which", sorted(EDITS))
def test_set_light_gives_the_blob_of_the_edited_scene_file(B, scene, tmp_path, which):
    sc = scene(FOUR)
    original = sc.flat_bytes()
    p, n = C.c_void_p(), C.c_uint64()
    assert B.lib().bhrt_scene_flat(sc._h, C.byref(p), C.byref(n)) == 0
    where, size = p.value, n.value
    apply(sc, EDITS[which])
    want = scene(edited_xml(tmp_path, FOUR, [EDITS[which]], which))
    assert sc.flat_bytes() == want.flat_bytes() and want.flat_bytes() != original
    assert [record(sc, k) for k in range(4)] == [record(want, k) for k in range(4)]
    # the pointer bhrt_scene_flat returned stays valid and total_bytes is unchanged
    assert B.lib().bhrt_scene_flat(sc._h, C.byref(p), C.byref(n)) == 0 and (p.value, n.value) == (where, size)
    assert C.string_at(p, n.value) == want.flat_bytes() and sc.flat_view().header.total_bytes == size == len(original)
    now = [sc.light(k).blob_index for k in range(4)]
    if which == "reorder":
        assert now == [0, 2, 1, 3] and sum(a != b for a, b in zip(now, BLOB_INDEX)) >= 2
    elif which == "make_tie":                                    # sun and amb tie at 0.1: the loader's sort decides, the setter follows it
        assert sorted(now[:3]) == [0, 1, 2] and now[KEY] == 2
    elif which == "break_tie":
        assert now == [3, 1, 0, 2]
    elif which == "raise_ambient":
        assert now == [2, 0, 1, 3]
    else:
        assert now == BLOB_INDEX


def test_two_edits_in_a_row_and_the_inverse_edit(B, scene, tmp_path):
    sc = scene(FOUR)
    original = sc.flat_bytes()
    saved = [sc.light(k) for k in range(4)]
    for k, e in enumerate((REORDER, TURN_DIRECT, RESIZE, MAKE_TIE)):       # sun is edited twice: the direction, then the intensity beside it
        apply(sc, e)
        done = (REORDER, TURN_DIRECT, RESIZE, MAKE_TIE)[:k + 1]
        assert sc.flat_bytes() == scene(edited_xml(tmp_path, FOUR, done, "row%d" % k)).flat_bytes(), k
    # all three values of one light in one call
    one = scene(FOUR)
    one.set_light(FILL, (1.5, 2.5, 1.0 / 7.0), (0.1, 0.2, 0.3), 0.7)
    assert one.flat_bytes() == scene(edited_xml(tmp_path, FOUR, [("fill", (1.5, 2.5, 1.0 / 7.0), (0.1, 0.2, 0.3), 0.7)], "all")).flat_bytes()
    # the inverse edits, in any order, give the original blob: a direct light's saved vec is a unit vector, which normalized() may not return
    # bit for bit, so its direction goes back as the file states it
    sc.set_light(KEY, list(saved[KEY].intensity))
    sc.set_light(FILL, None, None, saved[FILL].size)
    sc.set_light(SUN, list(saved[SUN].intensity), (1, 2, -3))
    assert sc.flat_bytes() == original and [record(sc, k) for k in range(4)] == [record(scene(FOUR), k) for k in range(4)]


def test_clone_carries_names_and_edits(B, scene, tmp_path):
    sc = scene(FOUR)
    before = sc.clone()
    apply(sc, REORDER)
    after = sc.clone()
    try:
        assert before.flat_bytes() == scene(FOUR).flat_bytes() and after.flat_bytes() == sc.flat_bytes()
        for cl in (before, after):
            assert [cl.light_index(n) for n in NAMES] == [0, 1, 2, 3] and cl.light_count() == 4
        assert [record(after, k) for k in range(4)] == [record(sc, k) for k in range(4)]
        apply(before, REORDER)                                    # the clone taken before the edit takes the same edit
        assert before.flat_bytes() == sc.flat_bytes()
        apply(after, MOVE_POINT)                                  # a copy, not a view
        assert after.flat_bytes() != sc.flat_bytes()
        assert after.flat_bytes() == scene(edited_xml(tmp_path, FOUR, [REORDER, MOVE_POINT], "clone")).flat_bytes()
    finally:
        before.close()
        after.close()


def test_every_refusal_leaves_the_blob_and_the_records_unchanged(B, scene):
    sc = scene(FOUR)
    before, records = sc.flat_bytes(), [record(sc, k) for k in range(4)]
    cases = [
        ("light -1", lambda: sc.set_light(-1, (1, 1, 1))),
        ("light n", lambda: sc.set_light(4, (1, 1, 1))),
        ("NaN intensity", lambda: sc.set_light(KEY, (1, NAN, 1))),
        ("inf intensity", lambda: sc.set_light(AMB, (INF, 1, 1))),
        ("negative intensity", lambda: sc.set_light(SUN, (1, 1, -0.5))),
        ("NaN position", lambda: sc.set_light(KEY, None, (0, NAN, 0))),
        ("inf position", lambda: sc.set_light(FILL, None, (0, 0, -INF))),
        ("inf direction", lambda: sc.set_light(SUN, None, (INF, 0, 1))),
        ("vec for an ambient light", lambda: sc.set_light(AMB, None, (0, 0, 1))),
        ("size for a direct light", lambda: sc.set_light(SUN, None, None, 0.5)),
        ("size 0 for an ambient light", lambda: sc.set_light(AMB, None, None, 0.0)),
        ("direction of length 0", lambda: sc.set_light(SUN, None, (0, 0, 0))),
        ("direction whose length underflows to 0", lambda: sc.set_light(SUN, None, (1e-30, 0, 0))),
        ("NaN size", lambda: sc.set_light(FILL, None, None, NAN)),
        ("inf size", lambda: sc.set_light(FILL, None, None, INF)),
        ("a valid vec beside a bad size", lambda: sc.set_light(FILL, None, (1, 2, 3), NAN)),
        ("a valid intensity beside a bad vec", lambda: sc.set_light(KEY, (1, 2, 3), (NAN, 0, 0))),
        ("sum overflows", lambda: sc.set_light(KEY, (3.4e38, 3.4e38, 3.4e38))),
    ]
    for what, call in cases:
        with pytest.raises(B.BhrtError, match="bhrt error 3: bhrt_scene_set_light"):
            call()
        sc._flat = None
        assert sc.flat_bytes() == before and [record(sc, k) for k in range(4)] == records, what
    v3 = (C.c_float * 3)(1, 1, 1)
    assert B.lib().bhrt_scene_set_light(None, 0, v3, None, C.c_float(-1)) == 3
    # all lights off: all_light_intensity would be 0, which the pick table divides by
    c1 = scene("c1_sphere_plane")
    c1_before = c1.flat_bytes()
    with pytest.raises(B.BhrtError, match="bhrt error 3: bhrt_scene_set_light"):
        c1.set_light(0, (0, 0, 0))
    c1._flat = None
    assert c1.flat_bytes() == c1_before and same_bits(list(c1.light(0).intensity), [300] * 3)
    # one light of several switched off is fine, and is the edited file's blob; nothing with all NULL / size < 0 is a no-op that succeeds
    sc.set_light(KEY)
    sc.set_light(SUN, None, None, -INF)
    assert sc.flat_bytes() == before and [record(sc, k) for k in range(4)] == records
    sc.set_light(KEY, (0, 0, 0))
    assert sc.flat_bytes() != before and sc.light(KEY).blob_index == 0


def test_a_light_switched_off_is_the_edited_file(B, scene, tmp_path):
    sc = scene(FOUR)
    off = ("fill", (0.0, 0.0, 0.0), None, None)
    apply(sc, off)
    assert sc.flat_bytes() == scene(edited_xml(tmp_path, FOUR, [off], "off")).flat_bytes()
    # a direction whose length overflows: the loader's normalized() divides by inf and stores (0, 0, 0), which is finite; so does the setter
    far = ("sun", None, (3e38, 3e38, 0.0), None)
    apply(sc, far)
    assert sc.flat_bytes() == scene(edited_xml(tmp_path, FOUR, [off, far], "far")).flat_bytes() and same_bits(list(sc.light(SUN).vec), [0, 0, 0])


def test_the_oracle_on_the_edited_blob_is_the_oracle_on_the_fresh_load(B, O, scene, tmp_path):
    """Trivially true by byte identity; asserted once to show that the parity chain needs no new oracle code."""
    sc = scene(FOUR)
    before = O.render(sc.flat_bytes(), sc.width, sc.height, 2, gi=1)["samples"]
    apply(sc, MOVE_POINT)
    apply(sc, REORDER)
    fresh = scene(edited_xml(tmp_path, FOUR, [MOVE_POINT, REORDER], "oracle"))
    a = O.render(sc.flat_bytes(), sc.width, sc.height, 2, gi=1)["samples"]
    b = O.render(fresh.flat_bytes(), fresh.width, fresh.height, 2, gi=1)["samples"]
    assert same_bits(a, b) and not same_bits(a, before)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def opts_of(B, **kw):
    return B.default_opts(**dict(dict(spp=2, gi_bounces=1, seed=7), **kw))


@pytest.fixture(scope="module")
def original_frame(B):
    """The unedited scene's frame: what every edit must differ from.  Rendered once."""
    sc = B.Scene(os.path.join(SCENES, FOUR + ".xml"))
    try:
        rgb, rad, _ = sc.render(opts_of(B))
        return rgb, rad
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", RENDERED)
def test_an_edit_before_the_upload_renders_like_a_fresh_load(B, scene, tmp_path, original_frame, which):
    sc = scene(FOUR)
    apply(sc, EDITS[which])
    fresh = scene(edited_xml(tmp_path, FOUR, [EDITS[which]], which))
    assert sc.flat_bytes() == fresh.flat_bytes()
    o = opts_of(B)
    rgb, rad, _ = sc.render(o)
    frgb, frad, _ = fresh.render(o)
    assert same_bits(rad, frad) and np.array_equal(rgb, frgb)
    assert not same_bits(rad, original_frame[1])                  # the edit shows in the frame


@pytest.mark.gpu
@pytest.mark.parametrize("which", RENDERED)
def test_an_edit_of_an_uploaded_scene_renders_like_a_fresh_load_and_back(B, scene, tmp_path, original_frame, which):
    """The refresh path: the lights block, the pick table and the kernels' all_light_intensity of a scene that has rendered already."""
    sc = scene(FOUR)
    o = opts_of(B)
    rgb0, rad0, _ = sc.render(o)                                  # the device has seen the original scene
    assert same_bits(rad0, original_frame[1]) and np.array_equal(rgb0, original_frame[0])
    saved = [sc.light(k) for k in range(4)]
    apply(sc, EDITS[which])
    fresh = scene(edited_xml(tmp_path, FOUR, [EDITS[which]], which))
    rgb, rad, _ = sc.render(o)
    frgb, frad, _ = fresh.render(o)
    assert same_bits(rad, frad) and np.array_equal(rgb, frgb) and not same_bits(rad, rad0)
    k = sc.light_index(EDITS[which][0])                           # the inverse edit: the first render's bytes again
    if KINDS[k] == 1:
        sc.set_light(k, list(saved[k].intensity), (1, 2, -3))     # the direction as the file states it
    elif KINDS[k] == 2:
        sc.set_light(k, list(saved[k].intensity), list(saved[k].vec), saved[k].size)
    else:
        sc.set_light(k, list(saved[k].intensity))
    assert sc.flat_bytes() == scene(FOUR).flat_bytes()
    rgb1, rad1, _ = sc.render(o)
    assert same_bits(rad1, rad0) and np.array_equal(rgb1, rgb0)


@pytest.mark.gpu
def test_an_edit_between_two_progressive_steps(B, scene, tmp_path):
    """Sample 0 of the original scene, sample 1 of the edited one, folded in order: later samples see the new light."""
    sc = scene(FOUR)
    o = opts_of(B, spp=2, seed=3)
    s = sc.render_samples(o, 0, 0, sc.width, sc.height)[0]
    x0 = s[:, 0]
    fresh = scene(edited_xml(tmp_path, FOUR, [MOVE_POINT, REORDER], "prog"))
    x1 = fresh.render_samples(o, 0, 0, fresh.width, fresh.height)[0][:, 1]
    sc.progressive_begin(o)
    sc.progressive_step(1)
    apply(sc, MOVE_POINT)
    apply(sc, REORDER)
    sc.progressive_step(1)
    mixed = sc.progressive_frame()[1]
    sc.progressive_end()
    want = ((np.zeros_like(x0) + x0) + x1) / f32(2)
    assert same_bits(mixed.reshape(-1, 3), want)
    assert not same_bits(x1, s[:, 1])                             # sample 1 of the original scene is another one


@pytest.mark.gpu
def test_a_light_moved_between_two_frames_of_a_temporal_session(B, scene, tmp_path):
    """Frame 0, set_light, frame 1: the session's current frame is the edited file's render at seed + 1, the history is kept (the camera did not
    move, nothing was reset).  What the change test makes of the moved light is a quality figure, not asserted here."""
    sc = scene(FOUR)
    o = opts_of(B, spp=2, seed=11)
    sc.temporal_begin(o, B.default_temporal_session_opts(carry_variance=1))
    try:
        sc.temporal_frame()
        first = sc.temporal_image(B.TEMPORAL_IMG_CURRENT)
        apply(sc, MOVE_POINT)
        sc.temporal_frame()
        cur = sc.temporal_image(B.TEMPORAL_IMG_CURRENT)
        pg = sc.temporal_status()
    finally:
        sc.temporal_end()
    fresh = scene(edited_xml(tmp_path, FOUR, [MOVE_POINT], "temporal"))
    want = fresh.render_var(opts_of(B, spp=2, seed=12))[1]
    assert same_bits(cur, want) and not same_bits(cur, first)
    assert same_bits(cur, sc.render_var(opts_of(B, spp=2, seed=12))[1])
    assert (pg.frames, pg.failed) == (2, 0) and pg.history_pixels == pg.pixels == sc.width * sc.height


@pytest.mark.gpu
def test_an_installed_photon_map_is_the_old_light_s_until_it_is_built_again(B, scene, tmp_path):
    """The stated limit, pinned: set_light leaves an installed caustic map alone; bhrt_photon_build afterwards gives the records of a fresh load
    of the edited file, byte for byte (PhotonLights is formed from the host blob by every build)."""
    name, n = "c5_caustics", 2000
    move = ("pointLight", None, (1.5, -2.25, 20.0 + 1.0 / 3.0), None)
    sc = scene(name)
    o = B.default_opts(seed=3)
    assert sc.photon_build(o, n) == n
    old = sc.photon_get()
    sc.set_light(sc.light_index("pointLight"), None, move[2])
    assert np.array_equal(sc.photon_get(), old)                   # the installed map is still the old light's
    assert sc.photon_build(o, n) == n
    fresh = scene(edited_xml(tmp_path, name, [move], "photon"))
    assert fresh.flat_bytes() == sc.flat_bytes()
    assert fresh.photon_build(o, n) == n
    new = sc.photon_get()
    assert np.array_equal(new, fresh.photon_get()) and not np.array_equal(new, old)
