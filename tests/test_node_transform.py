"""Moving objects: the names and transforms of a loaded scene's nodes (bhrt_scene_node_index, _get_node_transform(s),
_set_node_transform) and the node-id image (bhrt_first_hit_node).

The setter's stated property is checked against the loader itself: the blob after an edit is the blob of the edited scene file, written with
%.9g values (which round-trip a float32).  The oracle evaluates the blob, so a moved scene is checked bit for bit with no new oracle code; it
has no lens, so the lens = 1 run is compared with a fresh load of the edited file alone."""
import ctypes as C
import os
import re
import shutil
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from conftest import ROOT, SCENES, same_bits

f32 = np.float32
NAN, INF = float("nan"), float("inf")
BOTH = ["c1_sphere_plane", "moving_nested"]
# (scene, node name): a root node of c1, and a parent (depth 1, two children) and a child (depth 2) of moving_nested
NODES = [("c1_sphere_plane", "ball"), ("moving_nested", "parent"), ("moving_nested", "moon"), ("moving_nested", "mesh_small.obj")]
MOVE = {"c1_sphere_plane": ("ball", (1.25, -0.5, 0.75)), "moving_nested": ("parent", (0.75, -0.5, 0.25))}


def ops_of(B):
    """One op of every kind, with values no shorter decimal states exactly (%.9g must carry them)."""
    return [B.scale(1.1, 0.9, 1.0 / 3.0), B.rotate(0.3, -1.0, 2.0, 33.3), B.translate(0.1, -2.0 / 3.0, 0.7)]


def edited_xml(tmp_path, name, node, ops, replace, tag="edit"):
    """tests/scenes/<name>.xml with <scale> / <rotate> / <translate> elements for `ops` appended to the first <object name=node> (replace: its own
    transform children dropped first), written into tmp_path beside a copy of the mesh the scene names."""
    tree = ET.parse(os.path.join(SCENES, name + ".xml"))
    obj = next(e for e in tree.getroot().iter("object") if e.get("name") == node)
    if replace:
        for c in [c for c in obj if c.tag in ("scale", "rotate", "translate")]:
            obj.remove(c)
    g = lambda x: "%.9g" % f32(x)  # noqa: E731
    for op in ops:
        e = ET.SubElement(obj, ("scale", "rotate", "translate")[op.kind], x=g(op.v[0]), y=g(op.v[1]), z=g(op.v[2]))
        if op.kind == 1:
            e.set("angle", g(op.v[3]))
    path = os.path.join(str(tmp_path), f"{name}_{tag}.xml")
    tree.write(path)
    for mesh in ("mesh_small.obj",):
        if mesh in open(path).read() and not os.path.exists(os.path.join(str(tmp_path), mesh)):
            shutil.copy(os.path.join(SCENES, mesh), str(tmp_path))
    return path


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


def oracle_ids(O, sc):
    o, d = O.primary_rays(sc.flat_view())
    return O.trace_closest(sc.flat_bytes(), o, d, 1)["node"].reshape(sc.height, sc.width)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("bhrt_scene_node_index", "bhrt_scene_get_node_transform", "bhrt_scene_get_node_transforms", "bhrt_scene_set_node_transform",
           "bhrt_first_hit_node", "bhrt_first_hit_node_dev")


def test_symbols_exported_declared_and_wrapped(B):
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    for s in SYMBOLS:
        assert hasattr(B.lib(), s) and s in B.EXPORTS and re.search(r"\bint %s\(" % s, hdr), s
    for w in ("node_index", "node_transform", "node_transforms", "set_node_transform", "first_hit_node", "first_hit_node_dev"):
        assert callable(getattr(B.Scene, w))
    assert C.sizeof(B.XformOp) == 20 and B.XFORM_DTYPE.itemsize == 84
    assert re.search(r"enum \{ BHRT_XFORM_SCALE = 0, BHRT_XFORM_ROTATE = 1, BHRT_XFORM_TRANSLATE = 2 \};", hdr)
    assert (B.XFORM_SCALE, B.XFORM_ROTATE, B.XFORM_TRANSLATE) == (0, 1, 2)


def test_node_index_and_the_getters(B, scene):
    sc = scene("moving_nested")
    assert [sc.node_index(n) for n in ("ground", "parent", "moon", "mesh_small.obj")] == [0, 1, 2, 3]
    for bad in ("nobody", "", "Parent"):
        with pytest.raises(B.BhrtError, match="bhrt error 3: bhrt_scene_node_index"):
            sc.node_index(bad)
    i = C.c_int32(7)
    assert B.lib().bhrt_scene_node_index(sc._h, None, C.byref(i)) == 3 and B.lib().bhrt_scene_node_index(None, b"moon", C.byref(i)) == 3
    assert B.lib().bhrt_scene_node_index(sc._h, b"moon", None) == 3 and i.value == 7
    nodes = sc.flat_view().nodes
    all_ = sc.node_transforms()
    assert all_.shape == (4,)
    for k, n in enumerate(nodes):
        for rec in (sc.node_transform(k), all_[k]):
            assert same_bits(rec["tm"], list(n.xf.tm)) and same_bits(rec["pos"], list(n.xf.pos)) and same_bits(rec["itm"], list(n.xf.itm))
    for bad in (-1, 4):
        with pytest.raises(B.BhrtError, match="bhrt error 3"):
            sc.node_transform(bad)
    buf, n = np.zeros(4, B.XFORM_DTYPE), C.c_uint32(0)
    assert B.lib().bhrt_scene_get_node_transforms(sc._h, buf.ctypes.data_as(C.c_void_p), C.c_uint32(3), C.byref(n)) == 3 and n.value == 4
    assert B.lib().bhrt_scene_get_node_transforms(None, buf.ctypes.data_as(C.c_void_p), C.c_uint32(4), C.byref(n)) == 3
    assert scene("c1_sphere_plane").node_index("ball") == 1


def test_every_refusal_leaves_the_blob_unchanged(B, scene):
    sc = scene("moving_nested")
    before = sc.flat_bytes()
    cur = sc.node_transform(1)
    tm, pos = cur["tm"], cur["pos"]
    singular = np.float32([1, 0, 0, 2, 0, 0, 0, 0, 1])
    bad_tm, bad_pos = tm.copy(), pos.copy()
    bad_tm[4], bad_pos[2] = NAN, INF
    cases = [
        ("node -1", lambda: sc.set_node_transform(-1, tm, pos)),
        ("node n_nodes", lambda: sc.set_node_transform(4, tm, pos)),
        ("tm without pos", lambda: sc.set_node_transform(1, tm, None)),
        ("pos without tm", lambda: sc.set_node_transform(1, None, pos)),
        ("unknown kind", lambda: sc.set_node_transform(1, tm, pos, [B.XformOp(3, (1, 1, 1, 0))])),
        ("negative kind", lambda: sc.set_node_transform(1, tm, pos, [B.translate(1, 0, 0), B.XformOp(-1, (1, 1, 1, 0))])),
        ("NaN tm", lambda: sc.set_node_transform(1, bad_tm, pos)),
        ("inf pos", lambda: sc.set_node_transform(1, tm, bad_pos)),
        ("NaN scale", lambda: sc.set_node_transform(1, tm, pos, [B.scale(1, NAN, 1)])),
        ("inf translate", lambda: sc.set_node_transform(1, None, None, [B.translate(0, 0, -INF)])),
        ("NaN angle", lambda: sc.set_node_transform(1, tm, pos, [B.rotate(0, 0, 1, NAN)])),
        ("inf axis", lambda: sc.set_node_transform(1, tm, pos, [B.rotate(INF, 0, 1, 10)])),
        ("zero axis", lambda: sc.set_node_transform(1, tm, pos, [B.rotate(0, 0, 0, 10)])),
        ("zero scale", lambda: sc.set_node_transform(1, tm, pos, [B.scale(1, 0, 1)])),
        ("singular tm", lambda: sc.set_node_transform(1, singular, pos)),
        ("overflow", lambda: sc.set_node_transform(1, tm, pos, [B.scale(3e38, 3e38, 3e38), B.scale(10, 10, 10)])),
    ]
    for what, call in cases:
        with pytest.raises(B.BhrtError, match="bhrt error 3: bhrt_scene_set_node_transform"):
            call()
        sc._flat = None
        assert sc.flat_bytes() == before, what
    L = B.lib()
    v9, v3 = (C.c_float * 9)(*tm), (C.c_float * 3)(*pos)
    assert L.bhrt_scene_set_node_transform(None, 1, v9, v3, None, C.c_uint32(0)) == 3
    assert L.bhrt_scene_set_node_transform(sc._h, 1, v9, v3, None, C.c_uint32(1)) == 3      # ops == NULL with n_ops > 0
    sc._flat = None
    assert sc.flat_bytes() == before


@pytest.mark.parametrize("name,node", NODES)
def test_set_node_transform_gives_the_blob_of_the_edited_scene_file(B, scene, tmp_path, name, node):
    """Both forms of the stated property: the node's current (tm, pos) and ops = the XML with the ops appended to that <object>; NULL / NULL and
    ops = the XML with the node's transform children replaced by them."""
    ops = ops_of(B)
    for replace in (False, True):
        sc = scene(name)
        k = sc.node_index(node)
        original = sc.flat_bytes()
        cur = sc.node_transform(k)
        if replace:
            sc.set_node_transform(k, None, None, ops)
        else:
            sc.set_node_transform(k, cur["tm"], cur["pos"], ops)
        want = scene(edited_xml(tmp_path, name, node, ops, replace, "r" if replace else "a")).flat_bytes()
        assert sc.flat_bytes() == want and want != original
        others = [j for j in range(sc.info.n_nodes) if j != k]
        assert all(sc.node_transform(j).tobytes() == scene(name).node_transform(j).tobytes() for j in others)
        # one op at a time is the same as all at once
        sc2 = scene(name)
        if replace:
            sc2.set_node_transform(k, None, None, [])
        for op in ops:
            c = sc2.node_transform(k)
            sc2.set_node_transform(k, c["tm"], c["pos"], [op])
        assert sc2.flat_bytes() == want


@pytest.mark.parametrize("name,node", NODES)
def test_restoring_a_saved_record_returns_the_original_blob(B, scene, name, node):
    sc = scene(name)
    k = sc.node_index(node)
    original = sc.flat_bytes()
    saved = sc.node_transforms()
    sc.set_node_transform(k, None, None, ops_of(B))
    assert sc.flat_bytes() != original
    sc.set_node_transform(k, saved[k]["tm"], saved[k]["pos"])
    assert sc.flat_bytes() == original


def test_the_blob_pointer_stays_valid_and_no_device_is_needed(B, scene):
    sc = scene("moving_nested")
    p, n = C.c_void_p(), C.c_uint64()
    assert B.lib().bhrt_scene_flat(sc._h, C.byref(p), C.byref(n)) == 0
    where = p.value
    sc.set_node_transform(2, None, None, [B.translate(1, 2, 3)])
    assert B.lib().bhrt_scene_flat(sc._h, C.byref(p), C.byref(n)) == 0 and p.value == where
    assert C.string_at(p, n.value) == sc.flat_bytes()
    assert same_bits(sc.node_transform(2)["pos"], [1, 2, 3])


def test_clone_carries_names_and_edits(B, scene):
    sc = scene("moving_nested")
    sc.set_node_transform(sc.node_index("moon"), None, None, ops_of(B))
    cl = sc.clone()
    try:
        assert cl.flat_bytes() == sc.flat_bytes()
        assert [cl.node_index(n) for n in ("ground", "parent", "moon", "mesh_small.obj")] == [0, 1, 2, 3]
        cl.set_node_transform(1, None, None, [B.translate(0, 0, 1)])
        assert cl.flat_bytes() != sc.flat_bytes()         # a copy, not a view
    finally:
        cl.close()


@pytest.mark.parametrize("name", BOTH)
def test_oracle_first_hit_changes_where_the_object_was_or_is_and_only_there(B, O, scene, name):
    sc = scene(name)
    W, H = sc.width, sc.height
    node, delta = MOVE[name]
    k = sc.node_index(node)
    mine = list(range(k, sc.flat_view().nodes[k].subtree_end))          # the node and its descendants
    z0, n0, a0 = O.first_hit(sc.flat_bytes(), W, H)
    id0 = oracle_ids(O, sc).reshape(-1)
    cur = sc.node_transform(k)
    sc.set_node_transform(k, cur["tm"], cur["pos"], [B.translate(*delta)])
    z1, n1, a1 = O.first_hit(sc.flat_bytes(), W, H)
    id1 = oracle_ids(O, sc).reshape(-1)
    was, now = np.isin(id0, mine), np.isin(id1, mine)
    changed = (z0.view(np.uint32) != z1.view(np.uint32)) | (n0.view(np.uint32) != n1.view(np.uint32)).any(-1) | (a0.view(np.uint32) != a1.view(np.uint32)).any(-1)
    assert changed.any() and not changed[~(was | now)].any()
    assert changed[was ^ now].all() and (was ^ now).any() and (was & now).any()
    assert (z0[was & now] != z1[was & now]).mean() > 0.9   # the surface under a pixel that stays on the object is another point of it


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def region_on(ids, mine):
    """A 16 x 8 region that straddles the moved object: centred on the right-most column of its pixels."""
    H, W = ids.shape
    jj, ii = np.nonzero(np.isin(ids, mine))
    i, j = int(ii.max()), int(jj[ii == ii.max()][0])
    x0, y0 = min(max(i - 8, 0), W - 16), min(max(j - 4, 0), H - 8)
    return x0, y0, x0 + 16, y0 + 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH)
def test_moved_scene_renders_like_the_oracle_and_like_a_fresh_load(B, O, scene, tmp_path, name):
    """After set_node_transform on an UPLOADED scene, bhrt_render_samples equals the oracle's render of the edited blob and a fresh load +
    upload of the edited XML bit for bit, and so do trace_closest's hit records; with lens = 1 (the oracle has no lens) the fresh load alone."""
    sc = scene(name)
    W, H = sc.width, sc.height
    node, delta = MOVE[name]
    k = sc.node_index(node)
    mine = list(range(k, sc.flat_view().nodes[k].subtree_end))
    o = B.default_opts(spp=2)
    sc.upload(0)
    sc.render_samples(o, 0, 0, 16, 8)                                     # the device has seen the original scene
    cur = sc.node_transform(k)
    ops = [B.translate(*delta)]
    sc.set_node_transform(k, cur["tm"], cur["pos"], ops)
    fresh = scene(edited_xml(tmp_path, name, node, ops, False))
    assert fresh.flat_bytes() == sc.flat_bytes()
    ids = oracle_ids(O, sc)
    region = region_on(ids, mine)
    inside = ids[region[1]:region[3], region[0]:region[2]]
    assert np.isin(inside, mine).any() and not np.isin(inside, mine).all()
    gs = sc.render_samples(o, *region)[0]
    ref = O.render(sc.flat_bytes(), W, H, 2, region=region)["samples"]
    assert same_bits(gs, ref) and same_bits(gs, fresh.render_samples(o, *region)[0])
    before = O.render(scene(name).flat_bytes(), W, H, 2, region=region)["samples"]
    assert not same_bits(ref, before)                                      # the move shows in the region
    # hit records of the whole frame's primary rays
    ro, rd = O.primary_rays(sc.flat_view())
    g, r = sc.trace_closest(ro, rd, B.SIDE_FRONT), O.trace_closest(sc.flat_bytes(), ro, rd, 1)
    assert np.array_equal(g["node"], r["node"]) and np.array_equal(g["prim"], r["prim"]) and np.array_equal(g["front"], r["front"]) and same_bits(g["t"], r["t"])
    # through the lens
    for s in (sc, fresh):
        s.set_lens(dof=0.4)
    ol = B.default_opts(spp=2, lens=1)
    gl = sc.render_samples(ol, *region)[0]
    assert same_bits(gl, fresh.render_samples(ol, *region)[0]) and not same_bits(gl, gs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH)
def test_first_hit_node_equals_the_oracle_before_and_after_a_move(B, O, scene, name):
    """The id image is the oracle's trace_closest(...).node over primary_rays, exactly; bhrt_first_hit's three images do not depend on whether
    the id image was asked for."""
    import torch
    sc = scene(name)
    node, delta = MOVE[name]
    k = sc.node_index(node)
    guides = sc.first_hit()
    ids0 = sc.first_hit_node()
    assert ids0.dtype == np.int32 and np.array_equal(ids0, oracle_ids(O, sc))
    assert (ids0 == -1).any() and set(np.unique(ids0)) == set(range(-1, sc.info.n_nodes))
    again = sc.first_hit()
    assert all(same_bits(a, b) for a, b in zip(guides, again))
    z, n, a = O.first_hit(sc.flat_bytes(), sc.width, sc.height)
    assert same_bits(guides[0].reshape(-1), z) and same_bits(guides[1].reshape(-1, 3), n) and same_bits(guides[2].reshape(-1, 3), a)
    cur = sc.node_transform(k)
    sc.set_node_transform(k, cur["tm"], cur["pos"], [B.translate(*delta)])
    ids1 = sc.first_hit_node()
    assert np.array_equal(ids1, oracle_ids(O, sc)) and not np.array_equal(ids1, ids0)
    # the _dev variant on a stream
    dev = torch.device("cuda", 0)
    t = torch.full((sc.height, sc.width), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    sc.first_hit_node_dev(t.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(t.cpu().numpy(), ids1)
    with pytest.raises(B.BhrtError, match="bhrt error 3"):
        sc.first_hit_node_dev(0)


@pytest.mark.gpu
def test_a_move_between_two_progressive_steps(B, scene):
    """Samples 0-1 of the original scene, 2-3 of the moved one, folded in order: later samples see the new transform."""
    sc = scene("moving_nested")
    o = B.default_opts(spp=4, gi_bounces=2, seed=3)
    k = sc.node_index("parent")
    saved = sc.node_transform(k)
    sc.progressive_begin(o)
    sc.progressive_step(2)
    sc.set_node_transform(k, saved["tm"], saved["pos"], [B.translate(*MOVE["moving_nested"][1])])
    sc.progressive_step(2)
    mixed = sc.progressive_frame()[1]
    sc.progressive_end()
    s_new = sc.render_samples(o, 0, 0, sc.width, sc.height)[0]
    sc.set_node_transform(k, saved["tm"], saved["pos"])
    s_old = sc.render_samples(o, 0, 0, sc.width, sc.height)[0]
    assert not same_bits(s_new, s_old)
    want = ((((np.zeros_like(s_old[:, 0]) + s_old[:, 0]) + s_old[:, 1]) + s_new[:, 2]) + s_new[:, 3]) / f32(4)
    assert same_bits(mixed.reshape(-1, 3), want)
