"""The device BVH build (bvh_build.hip) at its scan, leaf-size, depth and non-finite edges.

tests/test_bvh_build.py holds the device build to the oracle's cyBVH::Build (oracle/bhrt_oracle.cpp::oracle_bvh_build) on three
meshes and 24 soups, all at max_per_leaf = 4 and at sizes drawn from one list.  This file builds the inputs that reach what those
leave out, from numpy alone:

  strip(n)   a triangle strip along x: sizes on both sides of the scan's tile edges (kTile = 4096), in order and shuffled, and
             1024 * 4096 + 1, the first size at which the one-workgroup scan of the tile sums carries into a second chunk;
  comb(K)    triangle k at x = 2**k: every split peels one element off, so the tree is as deep as it is large;
  same(n)    n copies of one triangle: no axis separates anything, every node goes through all three partition rounds (each one
             permutes it) and ends as a forced halving or, up to 8 elements, as a leaf -- at every max_per_leaf incl. the clamps;
  zero ties  -0.0 and +0.0 as the touching extreme in different waves and workgroups: the first in list order supplies the bits;
  non-finite inf, 3e30 (beyond the box's 1e30 seed) and NaN coordinates: `if (b > v) b = v` never lets a NaN bound into a box.

The checker is everywhere O.bvh_build(v, f, max_per); all 8 words of every node, the element order, the node count and the depth
(taken from the oracle's parent links) must be equal.  Integer and compare work: no tolerance anywhere.  The compiled reference
builds at its own fixed setting (4), so the oracle at other settings is pinned by reading cyBVH.h:122-142,242-328, not by a dump."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_bvh_build import XML, soups, write_obj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096                      # kTile of bvh_build.hip
CHUNK_EDGE = 1024 * TILE + 1     # kTileThreads tiles per chunk of k_bvh_scan_sums: the first n with a second chunk
POS_NAN, NEG_NAN = 0x7FC00000, 0xFFC00000


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def strip(n, shuffle_seed=None):
    i = np.arange(n + 2)
    v = np.stack([i, i % 2, np.zeros_like(i)], axis=1).astype(np.float32)
    k = np.arange(n, dtype=np.uint32)
    f = np.stack([k, k + 1, k + 2], axis=1)
    if shuffle_seed is not None:
        f = f[np.random.default_rng(shuffle_seed).permutation(n)]
    return v, np.ascontiguousarray(f)


def comb(K):
    v = np.zeros((K, 3, 3), np.float32)
    v[:, :, 0] = (2.0 ** np.arange(K))[:, None]
    v[:, 1, 1] = 1e-3
    v[:, 2, 2] = 1e-3
    return v.reshape(-1, 3), np.arange(3 * K, dtype=np.uint32).reshape(K, 3)


def same(n):
    tri = np.random.default_rng(7).normal(size=(1, 3, 3))
    return np.repeat(tri, n, axis=0).reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def zero_ties(variant, mirrored):
    """600 small triangles strictly inside x < 0 but for the holders, which touch x = 0 with one vertex.  Three groups of holders:
    the first one (list position 300, i.e. workgroup 1 wave 0 of the 256-thread kernels; position 0 in variant C), the rest of
    its workgroup (301..511) and the next workgroup's (512..599).  A: the first holds -0.0, all others +0.0; B: the signs
    swapped; C: as A with the first holder at position 0.  mirrored: x -> -x, the same on the minimum side."""
    n = 600
    rng = np.random.default_rng(11)
    c = np.concatenate([rng.uniform(-5, -1, (n, 1, 1)), rng.uniform(-5, 5, (n, 1, 2))], axis=2)
    tri = (c + rng.normal(scale=0.1, size=(n, 3, 3))).astype(np.float32)
    assert tri[..., 0].max() < -0.25
    first = 0 if variant == "C" else 300
    z_first, z_rest = (np.float32(0.0), np.float32(-0.0)) if variant == "B" else (np.float32(-0.0), np.float32(0.0))
    tri[first, first % 3, 0] = z_first
    for e in range(301, n):
        tri[e, e % 3, 0] = z_rest
    if mirrored:
        tri[..., 0] = -tri[..., 0]
    return tri.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def non_finite(case):
    """A 10-triangle random mesh; triangle t's vertices are rows 3t, 3t+1, 3t+2."""
    v = np.random.default_rng(5).normal(size=(30, 3)).astype(np.float32)
    u = v.view(np.uint32)
    if case == "a":
        v[3 * 0, 0] = np.inf; v[3 * 3, 1] = -np.inf; v[3 * 6, 2] = 3e30
    elif case == "b":
        u[3 * 1, 0] = POS_NAN; u[3 * 4, 1] = NEG_NAN; u[3 * 7 + 1, 2] = POS_NAN     # two first vertices, one second vertex
    else:
        u[0::3, 0] = POS_NAN
    return v, np.arange(30, dtype=np.uint32).reshape(10, 3)


# ---- the checker's side ---------------------------------------------------------------------------------------------------
_oracle = {}


def oracle(O, key, v, f, max_per):
    """O.bvh_build, once per (input name, max_per)."""
    k = (key, max_per)
    if k not in _oracle:
        nodes, elems = O.bvh_build(v, f, max_per)
        nodes.setflags(write=False); elems.setflags(write=False)
        _oracle[k] = (nodes, elems)
    return _oracle[k]


def node_levels(nodes):
    """Level of every node from the parent links (word 7; the root is node 1 with parent 0, slot 0 is unused)."""
    parent = nodes[:, 7].astype(np.int64)
    level = np.zeros(len(nodes), np.int64)
    idx, p = np.arange(2, len(nodes)), parent[2:]
    while len(idx):                              # p walks up; a node leaves once it has reached the root
        level[idx] += 1
        keep = p != 1
        idx, p = idx[keep], parent[p[keep]]
    return level


def tree_depth(nodes):
    return int(node_levels(nodes).max())


def is_leaf(nodes):
    return (nodes[:, 6] >> 31) == 1


def leaf_counts(nodes):
    return ((nodes[:, 6] >> 28) & 7) + 1


def check(B, O, key, v, f, max_per):
    """The bare entry point against the oracle: every node word, the element order, the node count and the depth; and a second
    build of the same input gives the same bytes."""
    on, oe = oracle(O, key, v, f, max_per)
    dn, de, dd = B.bvh_build(v, f, max_per)
    dn2, de2, dd2 = B.bvh_build(v, f, max_per)
    assert dn.tobytes() == dn2.tobytes() and de.tobytes() == de2.tobytes() and dd == dd2, (key, max_per, "two builds differ")
    m = min(len(dn), len(on))
    bad = np.flatnonzero((dn[1:m] != on[1:m]).any(axis=1)) + 1
    words = lambda row: " ".join("%08x" % x for x in row)
    first = f"node {bad[0]}: device {words(dn[bad[0]])} oracle {words(on[bad[0]])}" if len(bad) else None
    assert len(dn) == len(on), f"{key} at {max_per}: {len(dn) - 1} nodes, the oracle {len(on) - 1}; first difference: {first}"
    assert first is None, f"{key} at {max_per}: {first}"
    assert np.array_equal(dn[1:], on[1:]) and np.array_equal(de, oe), (key, max_per)
    assert dd == tree_depth(on), (key, max_per, dd)
    return dn, de, dd


def need_device(B):
    if B.device_count() < 1:
        pytest.fail("no HIP device")


# ---- CPU: the inputs reach what they claim ----------------------------------------------------------------------------------
def test_the_inputs_reach_what_they_claim(O):
    for n, n_nodes, depth in ((4095, 2047, 10), (4096, 2047, 10), (4097, 2049, 11), (8193, 4097, 12)):
        on, oe = oracle(O, f"strip{n}", *strip(n), 4)
        assert (len(on) - 1, tree_depth(on)) == (n_nodes, depth), n
        assert np.array_equal(np.sort(oe), np.arange(n))
    v, f = comb(126)
    on, _ = oracle(O, "comb126", v, f, 1)
    assert (len(on) - 1, tree_depth(on)) == (251, 125)
    lv, leaf = node_levels(on)[1:], is_leaf(on)[1:]
    for l in range(1, 125):                       # a comb: one leaf and one inner node on every level below the root ...
        assert (int(np.sum(leaf[lv == l])), int(np.sum(~leaf[lv == l]))) == (1, 1), l
    assert int(np.sum(leaf[lv == 125])) == 2 and int(np.sum(lv == 125)) == 2   # ... and the last two elements at the bottom
    on, _ = oracle(O, "comb126", v, f, 4)
    assert (len(on) - 1, tree_depth(on)) == (245, 122)

    v, f = same(9)
    order = {mp: oracle(O, "same9", v, f, mp)[1] for mp in (0, 1, 2, 4, 8, 9, 100)}
    assert list(order[2]) == [4, 5, 2, 3, 8, 0, 1, 6, 7] and list(order[4]) == [2, 3, 4, 5, 8, 0, 1, 6, 7] and list(order[8]) == [2, 3, 4, 5, 6, 7, 8, 0, 1]
    for a, b in ((2, 4), (2, 8), (4, 8)):         # the leaf size decides how often a node is permuted: the case discriminates
        assert not np.array_equal(order[a], order[b])
    assert np.array_equal(order[0], order[1]) and np.array_equal(order[1], order[2])
    assert np.array_equal(order[8], order[9]) and np.array_equal(order[8], order[100])
    on = oracle(O, "same9", v, f, 2)[0]
    assert leaf_counts(on)[1:][is_leaf(on)[1:]].max() > 2      # no axis separates: leaves above max_per (the ST_ACTIVE -> ST_LEAF arm)

    for mirrored, word in ((False, 3), (True, 0)):
        sign = {var: int(oracle(O, f"zero{var}{mirrored}", *zero_ties(var, mirrored), 4)[0][1, word]) for var in "ABC"}
        assert {sign["A"], sign["B"]} == {0x00000000, 0x80000000} and sign["C"] == sign["A"], (mirrored, sign)

    root = oracle(O, "nonfinite_b", *non_finite("b"), 4)[0][1, :6].view(np.float32)
    assert np.all(np.isfinite(root)), root        # NaN bounds never enter a box (cyBVH.h's `if (b > v) b = v`)
    assert np.isnan(non_finite("b")[0]).sum() == 3 and np.signbit(non_finite("b")[0][12, 1])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shuffled", [False, True])
def test_strips_at_the_scan_tile_edges(B, O, shuffled):
    need_device(B)
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        v, f = strip(n, 1000 + n if shuffled else None)
        check(B, O, f"strip{n}{'s' if shuffled else ''}", v, f, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("max_per", [1, 4])
def test_comb_is_as_deep_as_it_is_large(B, O, max_per):
    need_device(B)
    v, f = comb(126)
    dn, _, depth = check(B, O, "comb126", v, f, max_per)
    assert depth == tree_depth(oracle(O, "comb126", v, f, max_per)[0]) >= 122


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 8, 9, 16, 17, 33])
def test_identical_triangles_at_every_leaf_size(B, O, n):
    need_device(B)
    v, f = same(n)
    got = {mp: check(B, O, f"same{n}", v, f, mp) for mp in (0, 1, 2, 4, 8, 9, 100)}
    for group in ((0, 1), (8, 9, 100)):           # the clamps 0 -> 1 and > 8 -> 8
        for mp in group[1:]:
            assert got[mp][0].tobytes() == got[group[0]][0].tobytes() and got[mp][1].tobytes() == got[group[0]][1].tobytes() and got[mp][2] == got[group[0]][2], (n, mp)
    if n == 9:
        oe = {mp: oracle(O, "same9", v, f, mp)[1] for mp in (2, 4, 8)}
        for a, b in ((2, 4), (2, 8), (4, 8)):
            assert not np.array_equal(oe[a], oe[b])


@pytest.mark.gpu
@pytest.mark.parametrize("max_per", [1, 8])
def test_soups_at_other_leaf_sizes(B, O, max_per):
    need_device(B)
    for name, v, f in soups():
        check(B, O, name, v, f, max_per)


@pytest.mark.gpu
@pytest.mark.parametrize("mirrored", [False, True])
def test_zero_ties_across_waves_and_workgroups(B, O, mirrored):
    need_device(B)
    word = 0 if mirrored else 3                   # root lo.x / hi.x
    sign = {}
    for var in "ABC":
        v, f = zero_ties(var, mirrored)
        dn, _, _ = check(B, O, f"zero{var}{mirrored}", v, f, 4)
        sign[var] = int(oracle(O, f"zero{var}{mirrored}", v, f, 4)[0][1, word])
        assert int(dn[1, word]) == sign[var]
    assert {sign["A"], sign["B"]} == {0x00000000, 0x80000000}     # the first holder decides: the case discriminates


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_non_finite_coordinates(B, O, tmp_path, case):
    """Measured on an MI355X with the library before the NaN rule of k_bvh_root_keys / k_bvh_assign: case b gave 7 nodes where the
    oracle has 5, with the root box lo.y = 0x7149f2ca (1e30) and hi.x = 0xf149f2ca (-1e30) where the oracle keeps the other
    elements' extremes, 0xbfa98498 (-1.3243589) and 0x3f778b7f (0.9669723).  Cases a and c were equal before and after."""
    need_device(B)
    v, f = non_finite(case)
    check(B, O, "nonfinite_" + case, v, f, 4)
    write_obj(tmp_path / "m.obj", v, f)           # repr(float) writes nan / inf, the loader's sscanf reads them
    xml = tmp_path / "m.xml"
    xml.write_text(XML.format(obj="m.obj"))
    host, dev = B.Scene(str(xml)), B.Scene(str(xml), bvh_device=0)   # load only: these scenes are never uploaded or rendered
    assert host.info.n_triangles == 10
    assert host.flat_bytes() == dev.flat_bytes()


@pytest.mark.gpu
def test_back_to_back_builds_leave_nothing_behind(B, O):
    need_device(B)
    sv, sf = strip(2 * TILE + 1, 1000 + 2 * TILE + 1)
    first = check(B, O, f"strip{2 * TILE + 1}s", sv, sf, 4)
    check(B, O, "same9", *same(9), 4)
    check(B, O, "comb126", *comb(126), 1)
    last = check(B, O, f"strip{2 * TILE + 1}s", sv, sf, 4)
    assert first[0].tobytes() == last[0].tobytes() and first[1].tobytes() == last[1].tobytes() and first[2] == last[2]


@pytest.mark.gpu
def test_scan_chunk_edge(B, O):
    """strip(1024 * 4096 + 1): the smallest input whose tile sums need a second chunk in k_bvh_scan_sums (the one exception to "a
    few seconds" in this file: no smaller n runs that carry).  Measured: the oracle's build of this strip took 2.3 s on one core of
    a machine without a GPU (the shuffled variant: 7.4 s); the whole test, oracle and both device builds, took 1.4 s on an MI355X
    machine with a faster CPU.  Device scratch is about 1.2 GB, the host arrays about as much."""
    need_device(B)
    v, f = strip(CHUNK_EDGE)
    check(B, O, "strip_chunk_edge", v, f, 4)
    _oracle.pop(("strip_chunk_edge", 4))          # 270 MB of nodes nobody else needs


def _raw(B, v, nv, f, nf, max_per, device, nodes, cap, elems):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    n, depth = C.c_uint32(0xdeadbeef), C.c_uint32(0xdeadbeef)
    rc = B.lib().bhrt_bvh_build(p(v), C.c_uint32(nv), p(f), C.c_uint32(nf), C.c_uint32(max_per), C.c_int(device), p(nodes), C.c_uint32(cap), C.byref(n), p(elems),
                                C.byref(depth))
    return rc, n.value, depth.value


@pytest.mark.gpu
def test_argument_errors(B, O):
    need_device(B)
    hdr = open(os.path.join(ROOT, "include", "bhrt.h")).read()
    ERR_ARG = int(re.search(r"BHRT_ERR_ARG\s*=\s*(\d+)", hdr).group(1))
    v, f = strip(100)
    on, oe = oracle(O, "strip100", v, f, 4)
    n_nodes = len(on) - 1
    nodes = np.full((2 * len(f) + 1, 8), 0xABABABAB, np.uint32)
    elems = np.zeros(len(f), np.uint32)
    bad = {
        "n_faces = 0": (v, len(v), f, 0, 0, nodes, len(nodes), elems),
        "n_vertices = 0": (v, 0, f, len(f), 0, nodes, len(nodes), elems),
        "null vertices": (None, len(v), f, len(f), 0, nodes, len(nodes), elems),
        "null faces": (v, len(v), None, len(f), 0, nodes, len(nodes), elems),
        "null nodes_out": (v, len(v), f, len(f), 0, None, len(nodes), elems),
        "null elems_out": (v, len(v), f, len(f), 0, nodes, len(nodes), None),
        "device = -1": (v, len(v), f, len(f), -1, nodes, len(nodes), elems),
        "device = count": (v, len(v), f, len(f), B.device_count(), nodes, len(nodes), elems),
        "node_capacity one too few": (v, len(v), f, len(f), 0, nodes, n_nodes, elems),   # n_nodes + 1 entries are written
    }
    for what, (av, nv, af, nf, device, an, cap, ae) in bad.items():
        rc, _, _ = _raw(B, av, nv, af, nf, 4, device, an, cap, ae)
        assert rc == ERR_ARG, (what, rc)
        assert B.lib().bhrt_last_error(), what
        assert np.all(nodes == 0xABABABAB), what + ": nodes_out written"
    rc, n, depth = _raw(B, v, len(v), f, len(f), 4, 0, nodes, n_nodes + 1, elems)
    assert (rc, n, depth) == (0, n_nodes, tree_depth(on))
    assert np.array_equal(nodes[1:n_nodes + 1], on[1:]) and np.array_equal(elems, oe)
    assert np.all(nodes[n_nodes + 1:] == 0xABABABAB)
    check(B, O, "strip100", v, f, 4)              # and a valid build after the refused ones
