"""Ray-primitive intersection at its decision thresholds: rays built to land ON the comparisons of
device_trace.h — triangle vertices and edges, coplanar equal-t ties, the grazing band of tri_plane_test, the shadow biases and
t_max, sphere tangents and on-surface origins, the plane's extent and d.z == 0, the slab tests' zero / tiny / huge components and
equal entry distances — instead of generic ones.  Three links:

  reference -> golden   tests/golden/make_intersect_edges.py ran the unmodified reference on exactly the rays `families()` builds
                        (the generator imports this module, so no input is stored) and recorded node, front and the bits of z per
                        closest ray and hit side, a SHA-256 of p and N over the hit rays, and the visibility of every shadow ray.
                        Of a hit's attributes uvw is left out: the reference never writes a sphere hit's uvw.z (Sphere.cpp:60).
  oracle -> golden      CPU, bit for bit (the oracle's trace calls use libm throughout).
  GPU -> oracle         node, prim, front and the bits of t; shadow visibility; in generated order and under a fixed permutation;
                        batch lengths that are no multiple of 64.  Plus the parked render-path walks on a flat grid whose every
                        primary ray meets the mesh at a grid vertex (test_render_walks_on_grid_vertices).

Every family asserts its own premise on the CPU (test_premise_*) with a restatement of the quantity it targets: float32 numpy in
vecmath.h's operation order where the kernel's own float is the target, float64 where a geometric fact is.  A premise is a
condition on the inputs, never an expected value.
"""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCENES, same_bits

f32 = np.float32
PERP, TRI_BIAS, SHADOW_BIAS = f32(0.001745), f32(0.0001), f32(0.00001)      # TriObj.cpp:12,9; GenLight.cpp:5
FAST_REL, FAST_ABS, FAST_BIG = f32(2.0 ** -19), f32(2.0 ** -100), f32(1.2676506e30)
N_ELL, N_UNIT, N_TOP, N_GRP, N_INNER, N_MESH, N_GRID = range(7)
SIDES = (1, 2, 3)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def A(x):
    return np.ascontiguousarray(x, f32)


def step(x, k):
    """x moved by k float32 steps (k an int array or scalar): nextafter applied |k| times, through the bit pattern."""
    x = A(x)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, np.int64(-2 ** 31) - i, i) + k          # monotone integer line
    i = np.where(i < 0, np.int64(-2 ** 31) - i, i)
    return i.astype(np.int32).view(f32)


def step1(x, k):
    return float(step(x, k)[0])


# ------------------------------------------------------------------------------------------------ assets
def write_grid_obj(path, nx, ny, pitch):
    """A flat grid of nx x ny quads in z = 0, centred, two triangles per quad with the same orientation (normal +z).  Every face
    corner has its own vn and vt, so every triangle shades differently: a wrong `prim` changes N and uvw of the hit."""
    with open(path, "w") as fp:
        fp.write(f"# flat grid, {nx} x {ny} quads, pitch {pitch!r}\n")
        for j in range(ny + 1):
            for i in range(nx + 1):
                fp.write(f"v {(i - nx / 2) * pitch!r} {(j - ny / 2) * pitch!r} 0.0\n")
        faces = []
        for j in range(ny):
            for i in range(nx):
                a = j * (nx + 1) + i + 1
                faces += [(a, a + 1, a + nx + 2), (a, a + nx + 2, a + nx + 1)]
        for k in range(3 * len(faces)):
            x, y = 0.3 * np.sin(0.7 * k + 0.1), 0.3 * np.cos(1.3 * k)
            n = np.array([x, y, 1.0]) / np.sqrt(x * x + y * y + 1.0)
            fp.write(f"vn {n[0]:.6f} {n[1]:.6f} {n[2]:.6f}\nvt {(k * 37 % 101) / 101:.6f} {(k * 53 % 97) / 97:.6f} 0\n")
        for k, f in enumerate(faces):
            fp.write("f " + " ".join(f"{v}/{3 * k + c + 1}/{3 * k + c + 1}" for c, v in enumerate(f)) + "\n")


# ------------------------------------------------------------------------------------------------ float32 restatements
def _mat_mul(m, p):          # vecmath.h mat_mul, m column-major
    m = [f32(x) for x in m]
    return np.stack([p[:, 0] * m[0] + p[:, 1] * m[3] + p[:, 2] * m[6], p[:, 0] * m[1] + p[:, 1] * m[4] + p[:, 2] * m[7],
                     p[:, 0] * m[2] + p[:, 1] * m[5] + p[:, 2] * m[8]], 1)


def _chain(fv, n):
    c = []
    while n >= 0:
        c.append(n)
        n = fv.nodes[n].parent
    return c[::-1]


def to_node(xf, p, d):       # Node::ToNodeCoords (scene.h:490-496) in float32
    pos = A(list(xf.pos))[None]
    q = _mat_mul(xf.itm, p - pos)
    return q, _mat_mul(xf.itm, (p + d) - pos) - q


def local_ray(fv, n, o, d, upto_parent=False):
    """The ray of node n's object space (device_trace.h::local_ray); upto_parent: of its parent's space."""
    p, q = A(o), A(d)
    ch = _chain(fv, n)
    for k in (ch[:-1] if upto_parent else ch):
        p, q = to_node(fv.nodes[k].xf, p, q)
    return p, q


def shadow_local_ray(fv, n, o, d, upto_parent=False):
    """The ray the any-hit tests see: GenLight's walk starts AT the root, whose identity ToNodeCoords re-forms d as (p + d) - p."""
    o, d = A(o), A(d)
    with np.errstate(all="ignore"):
        return local_ray(fv, n, o, (o + d) - o, upto_parent)


def plane_anyhit_terms(fv, n, o, d):
    """GenLight.cpp:50-57 in float32: t from the plane's own space, the hit point x from the PARENT-space ray."""
    p, q = shadow_local_ray(fv, n, o, d)
    pp, pq = shadow_local_ray(fv, n, o, d, upto_parent=True)
    with np.errstate(all="ignore"):
        t = -p[:, 2] / q[:, 2]
        return t, pp + t[:, None] * pq


def to_world(fv, n, p):
    """Object-space points of node n in world space, float64 (construction only: what counts is restated from the float32 result)."""
    p = np.asarray(p, np.float64)
    for k in _chain(fv, n)[::-1]:
        xf = fv.nodes[k].xf
        tm = np.array(list(xf.tm), np.float64).reshape(3, 3).T      # column-major
        p = p @ tm.T + np.array(list(xf.pos), np.float64)
    return p


def world_ray(fv, n, o, d):
    """Object-space rays carried to world space in float32."""
    ow = to_world(fv, n, o)
    return A(ow), A(to_world(fv, n, np.asarray(o, np.float64) + np.asarray(d, np.float64)) - ow)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def tri_table(v, f, p, d, chunk=2048):
    """TriObj::IntersectTriangle (TriObj.cpp:68-168) for every ray x triangle in float32, operation for operation: t, the grazing
    quotient `perp`, its approximate form aperp = |t_divisor * (1 / (|vN| |d|))|, and `inside` (the three-area rule)."""
    v, p, d = A(v), A(p), A(d)
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    a, b = v1 - v0, v2 - v0
    vN = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    nlen, nd0 = np.sqrt(_dot(vN, vN)), _dot(vN, v0)
    ax = np.abs(vN)
    axis = np.where((ax[:, 0] >= ax[:, 1]) & (ax[:, 0] >= ax[:, 2]), 0, np.where((ax[:, 1] >= ax[:, 0]) & (ax[:, 1] >= ax[:, 2]), 1, 2))
    iu, iv = np.where(axis == 0, 1, 0), np.where(axis == 2, 1, 2)
    T = np.arange(len(f))
    out = {k: [] for k in ("t", "perp", "aperp", "inside", "tdiv", "den")}
    with np.errstate(all="ignore"):
        for s in range(0, len(p), chunk):
            pp, dd = p[s:s + chunk, None, :], d[s:s + chunk, None, :]
            tdiv = _dot(vN[None], dd)
            den = nlen[None] * np.sqrt(_dot(dd, dd))
            t = (nd0[None] - _dot(vN[None], pp)) / tdiv
            vX = pp + t[..., None] * dd
            X, Y = vX[:, T, iu], vX[:, T, iv]
            e = [(vk[T, iu][None] - X, vk[T, iv][None] - Y) for vk in (v0, v1, v2)]
            cr = lambda q, r: ((-q[1]) * r[0] + q[0] * r[1]) / f32(2)
            a0, a1, a2 = cr(e[1], e[2]), cr(e[2], e[0]), cr(e[0], e[1])
            neg = [x < 0 for x in (a0, a1, a2)]
            out["inside"].append(~((neg[0] | neg[1] | neg[2]) & ~(neg[0] & neg[1] & neg[2])))
            out["t"].append(t); out["tdiv"].append(tdiv); out["den"].append(den + 0 * tdiv); out["perp"].append(tdiv / den)
            out["aperp"].append(np.abs(tdiv * (f32(1) / den)))
    return {k: np.concatenate(x) for k, x in out.items()}


def sphere_terms(p, d):      # Sphere.cpp:8-20 in float32
    with np.errstate(all="ignore"):
        Aq, Bq, Cq = _dot(d, d), f32(2) * _dot(d, p), _dot(p, p) - f32(1)
        DD = Bq * Bq - f32(4) * Aq * Cq
        sq = np.sqrt(np.maximum(DD, 0))
        return Aq, Bq, Cq, DD, (-Bq + sq) / (f32(2) * Aq), (-Bq - sq) / (f32(2) * Aq)


def plane_terms(p, d):       # Plane.cpp:8-20 in float32
    with np.errstate(all="ignore"):
        t = -p[:, 2] / d[:, 2]
        return t, p + t[:, None] * d


# ------------------------------------------------------------------------------------------------ the ray families
def _edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), 1)
    return np.unique(e, axis=0)


def _origins(centre, radius):
    """Twelve fixed origins around a point: the vertices of an icosahedron, so every surface is seen from both sides."""
    g = (1 + 5 ** 0.5) / 2
    ico = np.array([[0, 1, g], [0, -1, g], [0, 1, -g], [0, -1, -g], [1, g, 0], [-1, g, 0], [1, -g, 0], [-1, -g, 0],
                    [g, 0, 1], [-g, 0, 1], [g, 0, -1], [-g, 0, -1]]) / np.sqrt(1 + g * g)
    return centre[None] + radius * ico


def fam_vertices_edges(fv):
    """1: rays from a dozen origins at every vertex, and from four at the midpoint and third-point of every edge, of both meshes;
    targets carried to world space in float32.  Adjacent triangles compete for each hit."""
    o, d, meta = [], [], []
    for node in (N_MESH, N_GRID):
        m = fv.mesh_arrays(fv.nodes[node].mesh)
        v, e = np.asarray(m["v"], np.float64), _edges(m["f"])
        org = _origins(to_world(fv, node, v.mean(0)), 14.0)
        vt = A(to_world(fv, node, v))
        et = A(to_world(fv, node, np.concatenate([(v[e[:, 0]] + v[e[:, 1]]) / 2, v[e[:, 0]] + (v[e[:, 1]] - v[e[:, 0]]) / 3])))
        for k in range(12):
            o.append(np.broadcast_to(A(org[k]), vt.shape)); d.append(vt - A(org[k]))
            meta.append(np.stack([np.full(len(vt), node), np.arange(len(vt)), np.full(len(vt), -1), np.zeros(len(vt), int)], 1))
        ee = np.concatenate([e, e])
        for k in range(4):
            ok = A(org[(np.arange(len(et)) * 5 + 3 * k) % 12])
            o.append(ok); d.append(et - ok)
            meta.append(np.stack([np.full(len(et), node), ee[:, 0], ee[:, 1], np.repeat([1, 2], len(e))], 1))
    return {"o": A(np.concatenate(o)), "d": A(np.concatenate(d)), "meta": np.concatenate(meta)}


TIE_DIRS = np.array([[0, 0, -1], [0, 0, 1], [0.5, 0.25, -1], [-0.25, 0.5, -1], [0.5, 0, -1], [0, -0.5, -1], [0.25, -0.25, 1],
                     [1, 0, -0.5], [0, 1, -0.25], [-0.5, -0.5, -1]], np.float64)


def fam_coplanar_ties(fv):
    """2: on the flat grid, rays that arrive EXACTLY at a grid vertex: o = v - 4 d with dyadic d, so t = 4 and o + t d = v without
    rounding, in object space and (scale 4, offsets that are small integers) in world space.  Straight down / up (two zero
    components: the exact box path), oblique, and along grid lines (one zero component, origin on a box face).  Every triangle around
    the vertex reports the same t: prim is decided by leaf order and traversal order alone."""
    m = fv.mesh_arrays(fv.nodes[N_GRID].mesh)
    v = np.asarray(m["v"], np.float64)
    cnt = np.bincount(m["f"].ravel(), minlength=len(v))
    v = v[cnt >= 3]                                   # every vertex with at least three triangles around it (not the two lone corners)
    o = (v[:, None, :] - 4 * TIE_DIRS[None]).reshape(-1, 3)
    d = np.broadcast_to(TIE_DIRS[None], (len(v), len(TIE_DIRS), 3)).reshape(-1, 3)
    ow, dw = world_ray(fv, N_GRID, o, d)
    return {"o": ow, "d": dw}


def _grazing_scan(fv, node, tri, ow, dw, axis, window):
    """Steps dw[axis] float by float around the step at which the grazing quotient of triangle `tri` crosses 0.001745 (found by a
    secant on the float64 value) and restates aperp for every step.  Returns (rays o, d, aperp, perp)."""
    m = fv.mesh_arrays(fv.nodes[node].mesh)
    f = m["f"][tri:tri + 1]

    def at(k):
        dk = np.repeat(dw[None], len(k), 0)
        dk[:, axis] = step(np.full(len(k), dw[axis], f32), k)
        p, q = local_ray(fv, node, np.repeat(ow[None], len(k), 0), dk)
        tt = tri_table(m["v"], f, p, q)
        return dk, tt["aperp"][:, 0], tt["perp"][:, 0]
    k0 = 0
    for _ in range(6):                               # secant towards |perp| = PERP, in float steps of the component
        _, _, pr = at(np.array([k0, k0 + 4096]))
        a0, a1 = abs(float(pr[0])), abs(float(pr[1]))
        if a1 == a0:
            break
        k0 = int(round(k0 + (float(PERP) - a0) * 4096 / (a1 - a0)))
    k = k0 + np.arange(-window, window + 1)
    dk, ap, pr = at(k)
    return np.repeat(ow[None], len(k), 0), dk, ap, pr


def fam_grazing(fv):
    """3: for 24 triangles of mesh_small.obj and 12 of the grid, rays that meet the triangle's inside at the angle asin(0.001745) to
    its plane, one direction component stepped float by float.  Kept: the rays whose restated t_divisor * rcp(|vN| |d|) lies within
    0.001745 (1 +- 2^-19) — tri_plane_test's fallback band — and a ring of those within 4 x 2^-19 outside it on both sides."""
    o, d, band, tri_of = [], [], [], []
    for node, tris, dirs, window in ((N_MESH, range(5, 288, 12), 6, 24), (N_GRID, range(3, 128, 11), 2, 150)):
        m = fv.mesh_arrays(fv.nodes[node].mesh)
        v = np.asarray(m["v"], np.float64)
        for tri in tris:
            v0, v1, v2 = v[m["f"][tri]]
            n = np.cross(v1 - v0, v2 - v0); n /= np.linalg.norm(n)
            c = v0 + 0.5 * (v1 - v0) + 0.25 * (v2 - v0)          # inside, dyadic weights
            e1 = (v1 - v0) / np.linalg.norm(v1 - v0); e2 = np.cross(n, e1)
            for j in range(dirs):
                ang = 0.4 + j * np.pi / dirs * (1 if node == N_MESH else 0.5)
                u = np.cos(ang) * e1 + np.sin(ang) * e2
                if node == N_GRID:
                    u = np.array([1.0, 0.5, 0.0]) if j == 0 else np.array([-0.25, 1.0, 0.0])
                dd = 16 * (u - float(PERP) * np.linalg.norm(u) * n * (1 if (tri + j) % 2 else -1))
                k = 2.0 ** -6 if node == N_MESH else 2.0
                ow, dw = world_ray(fv, node, (c - k * dd)[None], dd[None])
                nw = to_world(fv, node, n[None]) - to_world(fv, node, np.zeros((1, 3)))
                axis = 2 if node == N_GRID else int(np.argmin(np.where(np.abs(nw[0]) > 0.15, np.abs(dw[0]), np.inf)))
                oo, dk, ap, pr = _grazing_scan(fv, node, tri, ow[0], dw[0], axis, window)
                rel = np.abs(ap.astype(np.float64) / float(PERP) - 1) * 2.0 ** 19
                keep = rel <= 4
                o.append(oo[keep]); d.append(dk[keep]); band.append(rel[keep] <= 1)
                tri_of.append(np.stack([np.full(keep.sum(), node), np.full(keep.sum(), tri)], 1))
    return {"o": A(np.concatenate(o)), "d": A(np.concatenate(d)), "in_band": np.concatenate(band), "meta": np.concatenate(tri_of)}


def fam_sphere(fv):
    """5: both spheres.  Tangent rays whose origin is stepped float by float so that DD crosses 0 (on the unit sphere, axis-parallel
    ones reach DD == 0 exactly); origins on the surface (C == 0), inside, at the centre; both roots positive, both negative, of
    opposite sign; every ray again with its direction scaled by 1e-18 and by 1e18."""
    rng = np.random.default_rng(51)
    o, d, node, grp = [], [], [], []
    ax = np.eye(3)
    for nd in (N_UNIT, N_ELL):
        P, D = [], []
        for a in range(3):                                            # axis-parallel tangents: o = e_b (1 + k ulp) - 3 e_a
            for b in range(3):
                if a != b:
                    for sgn in (1, -1):
                        for k in range(-6, 7):
                            x = step1(f32(1), 4 * k)             # steps of 4: stays representable after the unit sphere's translation
                            P.append(sgn * x * ax[b] - 3 * ax[a]); D.append(ax[a] * (1 if k % 2 else 2))
        for _ in range(24):                                           # generic tangents
            q = rng.normal(size=3); q /= np.linalg.norm(q)
            t = np.cross(q, rng.normal(size=3)); t /= np.linalg.norm(t)
            for k in range(-6, 7):
                P.append(q * (1 + k * 2.0 ** -22) - 2.5 * t); D.append(t * 1.5)
        surf = [ax[0], -ax[1], ax[2], -ax[0]]
        for q in surf:                                                # on the surface: outward, inward, tangent, oblique both ways
            t = np.roll(q, 1)
            for dd in (q, -q, t, -q + t, q + t, -0.5 * q - t, -2 * q):
                P.append(q); D.append(dd)
        for q in (np.zeros(3), 0.5 * ax[0], -0.25 * ax[2] + 0.5 * ax[1], 0.9375 * ax[1]):   # centre and inside: roots of opposite sign
            for dd in (ax[0], -ax[1], ax[2] + 0.5 * ax[0], np.array([0.25, -0.5, 1.0])):
                P.append(q); D.append(dd)
        for _ in range(40):                                           # outside: towards (both positive) and away (both negative)
            q = rng.normal(size=3); q *= 3 / np.linalg.norm(q)
            aim = rng.normal(size=3) * 0.5
            P.append(q); D.append(aim - q); P.append(q); D.append(q - aim)
        P, D = np.array(P), np.array(D)
        P, D = np.concatenate([P, P, P]), np.concatenate([D, D * 1e-18, D * 1e18])
        with np.errstate(over="ignore"):
            ow, dw = world_ray(fv, nd, P, D)
        o.append(ow); d.append(dw); node.append(np.full(len(ow), nd))
    return {"o": A(np.concatenate(o)), "d": A(np.concatenate(d)), "node": np.concatenate(node)}


def fam_plane(fv):
    """6: both planes.  Hit points on x = +-1, y = +-1 and at the four corners, the world origin stepped float by float so that the
    restated hit point crosses the bound (inward, on it, outward); d.z = +0.0 and -0.0; origins on the plane (p.z == 0).
    An object-space p.z of -0.0 cannot be reached: ToNodeCoords forms p.z from (p - pos).z, and a difference of equal floats is +0.0
    (it would take pos.z == 0 and all three products of the z row negative zeros; `top` has pos.z = 1.5, `inner` sits in a rotated
    group), so only +0.0 occurs; d.z = -0.0 is given in world space and becomes +0.0 the same way."""
    o, d, node = [], [], []
    pts = [(1, 0.3), (-1, -0.6), (0.2, 1), (-0.7, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]
    dirs = [(0.2, 0.1, -1), (-0.3, 0.25, 1), (0.5, -0.75, -0.5), (0, 0, -1)]
    for nd in (N_TOP, N_INNER):
        for (x, y) in pts:
            for dd in dirs:
                h, dd = np.array([x, y, 0.0]), np.array(dd)
                ow, dw = world_ray(fv, nd, (h - 2 * dd)[None], dd[None])
                for comp in range(3):
                    k = np.arange(-5, 6)
                    oo = np.repeat(ow, len(k), 0)
                    oo[:, comp] = step(oo[:, comp], k)
                    o.append(oo); d.append(np.repeat(dw, len(k), 0)); node.append(np.full(len(k), nd))
        ow, dw = world_ray(fv, nd, np.array([[0.2, -0.3, 0.5], [0.9, 0.9, -0.25], [0.0, 0.0, 0.0], [0.5, 0.5, 0.0]]),
                           np.array([[1, 0.5, 0.0], [-1, 0.25, 0.0], [0.3, 0.2, -1], [0.1, -0.2, 1]]))
        for z in (0.0, -0.0):                                        # world d.z = +-0: the top plane's z row is exact, so d'.z == 0 there
            dz = dw.copy(); dz[:2, 2] = z
            o.append(ow); d.append(dz); node.append(np.full(len(ow), nd))
    oz = A([[-12, -10, 1.5], [-11, -9.5, 1.5], [-13.5, -10.25, 1.5]])    # exactly on the top plane: p'.z == 0
    for dd in ([0.1, 0.2, -1], [0.1, 0.2, 1], [1, 0, 0]):
        o.append(oz); d.append(np.repeat(A([dd]), 3, 0)); node.append(np.full(3, N_TOP))
    return {"o": A(np.concatenate(o)), "d": A(np.concatenate(d)), "node": np.concatenate(node)}


def fam_slabs(fv):
    """7: the slab tests.  (a) mesh_small.obj: for every inner BVH node whose child boxes overlap, rays that start inside both and rays
    that enter both through a face plane the two boxes share (equal entry distances: order_fast cannot call it).  (b) the grid: rays
    lying in a box face — an origin coordinate equal to a bound, a zero direction component on that axis.  (c) the grid again, from
    x = 0 (the node's x offset is zero, so a tiny d.x survives ToNodeCoords): d.x subnormal, one step below / at / above
    BHRT_FAST_ABS = 2^-100, and below / at / above 2^100, both signs."""
    rng = np.random.default_rng(77)
    o, d, kind = [], [], []
    m = fv.mesh_arrays(fv.nodes[N_MESH].mesh)
    bb, data = np.asarray(m["bvh_bounds"], np.float64), m["bvh_data"]
    P, D = [], []
    for i in range(1, len(data)):
        if data[i] & 0x80000000:
            continue
        c1 = int(data[i] & 0x7fffffff)
        b1, b2 = bb[c1], bb[c1 + 1]
        lo, hi = np.maximum(b1[:3], b2[:3]), np.minimum(b1[3:], b2[3:])
        if (hi < lo).any():
            continue
        mid = (lo + hi) / 2
        for _ in range(6):
            P.append(mid); D.append(rng.normal(size=3))
        for a in range(3):
            for side in (0, 3):
                if b1[a + side] == b2[a + side]:
                    tgt = mid.copy(); tgt[a] = b1[a + side]
                    for _ in range(3):
                        dd = rng.normal(size=3); dd[a] = abs(dd[a]) * (1 if side == 0 else -1) + 0.2 * (1 if side == 0 else -1)
                        P.append(tgt - 3 * dd); D.append(dd)
    ow, dw = world_ray(fv, N_MESH, np.array(P), np.array(D))
    o.append(ow); d.append(dw); kind.append(np.zeros(len(ow), int))
    g = fv.mesh_arrays(fv.nodes[N_GRID].mesh)
    gb = np.asarray(g["bvh_bounds"], np.float64)[1:]
    P, D = [], []
    for b in gb[::2]:                                                # (b) in a box face
        for a in (0, 1):
            for side in (0, 3):
                c = np.array([(b[0] + b[3]) / 2, (b[1] + b[4]) / 2, 0.0]); c[a] = b[a + side]
                for dd in ([0.5, 0.5, -1.0], [-0.25, 1.0, -0.5], [1.0, -0.5, 1.0]):
                    dd = np.array(dd); dd[a] = 0.0
                    P.append(c - 2 * dd); D.append(dd)
    ow, dw = world_ray(fv, N_GRID, np.array(P), np.array(D))
    o.append(ow); d.append(dw); kind.append(np.ones(len(ow), int))
    ow, dw = [], []
    tiny = [1e-40, 1.4e-45, step1(FAST_ABS, -1), float(FAST_ABS), step1(FAST_ABS, 1), 1e-20]
    huge = [step1(f32(2.0 ** 100), -1), 2.0 ** 100, step1(f32(2.0 ** 100), 1), 2.0 ** 110]
    for y in (-0.875, -0.25, 0.0, 0.3125, 0.75):                     # object space; world = 4 x + (0, -12, 0), exact
        for dx in tiny + huge:
            for sg in (1, -1):
                for dyz in ((0.25, -1.0), (-0.5, -1.0), (0.125, 1.0)):
                    dd = np.array([sg * dx, dyz[0], dyz[1]])
                    p = np.array([0.0, y, 0.0]) - 2 * np.array([0.0, dyz[0], dyz[1]])
                    ow.append(4 * p + np.array([0, -12.0, 0])); dw.append(4 * dd)
    o.append(A(ow)); d.append(A(dw)); kind.append(np.full(len(ow), 2))
    return {"o": A(np.concatenate(o)), "d": A(np.concatenate(d)), "kind": np.concatenate(kind)}


def _restated_shadow_t(fv, blob_hit, o, d):
    """The t the any-hit test of the primitive each ray hit computes, in float32: plane -p.z / d.z, sphere min(t1, t2), triangle t."""
    node, prim = blob_hit
    t = np.full(len(o), np.nan, f32)
    for nd in np.unique(node):
        s = node == nd
        p, q = shadow_local_ray(fv, nd, o[s], d[s])
        ty = fv.nodes[nd].obj_type
        if ty == 1:
            _, _, _, _, t1, t2 = sphere_terms(p, q)
            t[s] = np.where(t1 <= t2, t1, t2)
        elif ty == 2:
            t[s] = plane_terms(p, q)[0]
        else:
            m = fv.mesh_arrays(fv.nodes[nd].mesh)
            tt = np.full(s.sum(), np.nan, f32)
            pr = prim[s]
            for k in range(0, s.sum(), 512):
                tab = tri_table(m["v"], m["f"][pr[k:k + 512]], p[k:k + 512], q[k:k + 512])["t"]
                tt[k:k + 512] = np.diagonal(tab)
            t[s] = tt
    return t


def fam_bias_range(fv, O, blob, fams):
    """4: front hits of triangles and spheres taken from families 1 and 5 (the oracle serves the construction only; the planes' any-hit
    test bounds the parent-space hit point, so its rays are built apart: fam_plane_shadow).  Shadow rays
    along the same line from a point a quarter of d short of the surface, the direction scaled so that the any-hit test's restated t
    is BHRT_SHADOW_BIAS or BHRT_TRI_BIAS, then the scale stepped through seven values a few floats apart (t moves through the bias);
    origins on the surface, onward and back out; and the original rays with t_max equal to the oracle's hit t and to its two
    neighbours.  `what`: 0 t_max, 1 / 2 the two bias scans, 3 on the surface; `node`, `prim`: the hit each row was made from."""
    pick = (("vertices_edges", 24), ("sphere", 6))
    o = np.concatenate([fams[k]["o"][::s] for k, s in pick])
    d = np.concatenate([fams[k]["d"][::s] for k, s in pick])
    r = O.trace_closest(blob, o, d, 1)
    ok = (r["node"] >= 0) & np.isfinite(r["t"]) & (np.abs(d).max(1) < 1e6) & (np.abs(d).max(1) > 1e-6)
    o, d, t, node, prim = o[ok], d[ok], r["t"][ok], r["node"][ok], r["prim"][ok]
    n = len(o)
    rows = [(o, d, t, 0, node, prim), (o, d, step(t, 1), 0, node, prim), (o, d, step(t, -1), 0, node, prim)]
    hitp = A(o + t[:, None] * d)
    far = np.full(n, 1e3, f32)
    for bias, tag in ((SHADOW_BIAS, 1), (TRI_BIAS, 2)):
        back = A(hitp - f32(0.25) * d)
        t0 = _restated_shadow_t(fv, (node, prim), back, d)
        with np.errstate(all="ignore"):
            c = (t0 / bias).astype(f32)
        g = np.isfinite(c) & (c > 0)
        for k in range(-3, 4):
            rows.append((back[g], A(d[g] * step(c[g], 3 * k)[:, None]), far[g], tag, node[g], prim[g]))
    rows.append((hitp, d, far, 3, node, prim))
    rows.append((hitp, -d, far, 3, node, prim))
    cat = lambda i: np.concatenate([np.broadcast_to(x[i], (len(x[0]),)) if np.ndim(x[i]) == 0 else x[i] for x in rows])
    return {"o": A(cat(0)), "d": A(cat(1)), "tmax": A(cat(2)), "what": cat(3), "node": cat(4), "prim": cat(5), "n_hits": n}


def fam_plane_shadow(fv):
    """4 and 6 for the any-hit plane test (GenLight.cpp:50-57), which takes t from the plane's own space but bounds the hit point of the
    PARENT-space ray: for `top` the world-space point, for `inner` the group-space one.  Targets are points of the
    (unbounded) plane whose parent-space x, y are prescribed.  what = 0: x, y on +-1 and at the corners, the world origin stepped float
    by float so that the restated parent-space hit point crosses the bound; 1: targets inside the bound, the direction scaled so that
    the restated t is BHRT_SHADOW_BIAS and the scale stepped; 2, 3, 4: t_max equal to the restated t, to the next float up, to the next
    float down."""
    rows = []
    dirs = np.array([(0.2, 0.1, -1), (-0.3, 0.25, 1), (0.5, -0.75, -0.5), (0, 0, -1), (0.1, 0.3, 0.8), (-0.4, 0.2, -0.7)]) * 0.125
    for nd in (N_TOP, N_INNER):
        xf, par = fv.nodes[nd].xf, fv.nodes[nd].parent
        tm, pos = np.array(list(xf.tm), np.float64).reshape(3, 3).T, np.array(list(xf.pos), np.float64)

        def on_plane(x, y):                                           # the point of the plane z' = 0 with parent-space x, y
            h = np.linalg.solve(tm[:2, :2], np.array([x, y]) - pos[:2])
            return tm @ np.array([h[0], h[1], 0.0]) + pos

        def world(P, D):
            if par < 0:
                return A(P), A(D)
            return world_ray(fv, par, P, D)
        for (x, y) in [(1, 0.3), (-1, -0.6), (0.2, 1), (-0.7, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]:
            for D in dirs[:4]:
                X = on_plane(x, y)
                ow, dw = world((X - 2 * D)[None], D[None])
                for comp in range(3):
                    k = np.arange(-5, 6)
                    oo = np.repeat(ow, len(k), 0)
                    oo[:, comp] = step(oo[:, comp], k)
                    rows.append((oo, np.repeat(dw, len(k), 0), np.full(len(k), 4, f32), nd, 0))
        for (x, y) in [(0.3, -0.4), (-0.6, 0.7), (0.0, 0.0), (0.875, 0.9), (-0.95, 0.1)]:
            X = on_plane(x, y)
            ow, dw = world(X[None] - 2 * dirs, dirs)
            t, _ = plane_anyhit_terms(fv, nd, ow, dw)
            for what, k in ((2, 0), (3, 1), (4, -1)):
                rows.append((ow, dw, step(t, k), nd, what))
            bo, bd = world(X[None] - 0.25 * dirs, dirs)
            t0, _ = plane_anyhit_terms(fv, nd, bo, bd)
            c = (t0 / SHADOW_BIAS).astype(f32)
            for k in range(-6, 7):
                rows.append((bo, A(bd * step(c, 2 * k)[:, None]), np.full(len(bo), 1e3, f32), nd, 1))
    cat = lambda i: np.concatenate([np.broadcast_to(x[i], (len(x[0]),)) if np.ndim(x[i]) == 0 else x[i] for x in rows])
    return {"o": A(cat(0)), "d": A(cat(1)), "tmax": A(cat(2)), "node": cat(3), "what": cat(4)}


def families(sc, O):
    """name -> {"o", "d"[, "tmax"], ...}: closest-hit families (no tmax) and shadow families, deterministic for a given scene."""
    fv, blob = sc.flat_view(), sc.flat_bytes()
    assert [fv.nodes[i].obj_type for i in range(7)] == [1, 1, 2, 0, 2, 3, 3] and fv.nodes[N_INNER].parent == N_GRP
    F = {"vertices_edges": fam_vertices_edges(fv), "coplanar_ties": fam_coplanar_ties(fv), "grazing": fam_grazing(fv),
         "sphere": fam_sphere(fv), "plane": fam_plane(fv), "slabs": fam_slabs(fv)}
    F["bias_range"] = fam_bias_range(fv, O, blob, F)
    F["plane_shadow"] = fam_plane_shadow(fv)
    # the closest families as any-hit rays too (GenLight::Shadow stops at t_max = 1: the part of the ray up to o + d, and beyond)
    for name, stride, tm in (("vertices_edges", 4, 1.25), ("coplanar_ties", 1, 8.0), ("grazing", 4, 1.0), ("sphere", 2, 1.5), ("plane", 1, 4.0), ("slabs", 1, 8.0)):
        F["shadow_" + name] = {"o": F[name]["o"][::stride], "d": F[name]["d"][::stride], "tmax": np.full(len(F[name]["o"][::stride]), tm, f32)}
    return F


def closest_names(F):
    return [k for k in F if "tmax" not in F[k]]


def shadow_names(F):
    return [k for k in F if "tmax" in F[k]]


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def scene(load_scene):
    return load_scene("intersect_edges")


@pytest.fixture(scope="module")
def fams(scene, O):
    return families(scene, O)


@pytest.fixture(scope="module")
def oracle(scene, fams, O):
    """The oracle's answers, computed once: (family, side) -> closest record, family -> visibility."""
    blob = scene.flat_bytes()
    out = {}
    for k in closest_names(fams):
        for side in SIDES:
            out[k, side] = O.trace_closest(blob, fams[k]["o"], fams[k]["d"], side)
    for k in shadow_names(fams):
        out[k] = O.trace_shadow(blob, fams[k]["o"], fams[k]["d"], fams[k]["tmax"])
    return out


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "intersect_edges.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gpu(B):
    if B.device_count() < 1:
        pytest.fail("no HIP device: the render path has no CPU fallback, GPU tests cannot run here")
    return B


# ------------------------------------------------------------------------------------------------ the committed assets
def test_grid_asset_is_what_the_writer_writes(tmp_path):
    write_grid_obj(str(tmp_path / "g.obj"), 8, 8, 0.25)
    assert (tmp_path / "g.obj").read_text() == open(os.path.join(SCENES, "grid_flat.obj")).read()


def test_budget(fams):
    nc = sum(len(fams[k]["o"]) for k in closest_names(fams))
    ns = sum(len(fams[k]["o"]) for k in shadow_names(fams))
    print("closest rays per family:", {k: len(fams[k]["o"]) for k in closest_names(fams)}, "shadow:", {k: len(fams[k]["o"]) for k in shadow_names(fams)})
    assert nc <= 40000 and ns <= 20000


# ------------------------------------------------------------------------------------------------ premises (CPU)
def test_premise_vertices_edges(scene, fams, oracle):
    """The targets are vertices / edge midpoints / third-points (float64: the restated object-space ray passes within 1e-5 of them
    at parameter 1; the meshes' size is about one, the world-space float32 target is good to 1e-6), and adjacent triangles compete: for most
    rays at least two triangles report a plane hit within 4 float steps of each other; the three-area rule both accepts and rejects
    among the triangles around the target; and the same vertex is owned by different triangles from different origins."""
    fv, F = scene.flat_view(), fams["vertices_edges"]
    for node in (N_MESH, N_GRID):
        s = F["meta"][:, 0] == node
        m = fv.mesh_arrays(fv.nodes[node].mesh)
        p, q = local_ray(fv, node, F["o"][s], F["d"][s])
        tt = tri_table(m["v"], m["f"], p, q)
        meta = F["meta"][s]
        adj = (m["f"][None, :, :] == meta[:, 1][:, None, None]).any(2)                       # triangles around the target's (first) vertex
        # float64: the ray passes the target vertex / edge point at parameter 1
        v = np.asarray(m["v"], np.float64)
        va, vb, kind = v[meta[:, 1]], v[np.maximum(meta[:, 2], 0)], meta[:, 3:4]
        tgt = np.where(kind == 0, va, np.where(kind == 1, (va + vb) / 2, va + (vb - va) / 3))
        isv = meta[:, 3] == 0
        x1 = p.astype(np.float64) + q.astype(np.float64)
        assert np.abs(x1 - tgt).max() < 1e-5 and (kind == 1).sum() > 100 and (kind == 2).sum() > 100
        near = np.abs(tt["t"].astype(np.float64) - 1) < 1e-5
        cand = adj & near & (np.abs(tt["perp"]) >= PERP)
        assert (cand.sum(1) >= 2).mean() > 0.6          # eight of the twelve origins lie off the flat grid's own plane
        acc, rej = (cand & tt["inside"]).sum(), (cand & ~tt["inside"]).sum()
        assert acc > 100 and rej > 100                                                          # both outcomes of the area rule
        assert (((cand & tt["inside"]).sum(1) >= 2)).sum() > 50                                  # equal-or-near t accepted twice: order decides
        r = oracle["vertices_edges", 3]
        prim, hit = r["prim"][s], r["node"][s] == node
        owners = {}
        for vi, pr, h in zip(meta[isv, 1], prim[isv], hit[isv]):
            if h:
                owners.setdefault(int(vi), set()).add(int(pr))
        assert sum(len(x) >= 2 for x in owners.values()) >= 10                  # the owner of a vertex changes with the origin


def test_premise_coplanar_ties(scene, fams, oracle):
    """Every ray has at least three triangles that accept the hit point with bit-equal t (restated in float32, object space), t == 4."""
    fv, F = scene.flat_view(), fams["coplanar_ties"]
    m = fv.mesh_arrays(fv.nodes[N_GRID].mesh)
    p, q = local_ray(fv, N_GRID, F["o"], F["d"])
    tt = tri_table(m["v"], m["f"], p, q)
    ok = tt["inside"] & (tt["t"] == f32(4))
    assert (ok.sum(1) >= 3).all() and (ok.sum(1) == 6).any()
    assert ((q == 0).sum(1) == 2).any() and ((q == 0).sum(1) == 1).any() and ((q == 0).sum(1) == 0).any()
    r = oracle["coplanar_ties", 3]
    g = r["node"] == N_GRID                                                # (a few oblique rays meet the plane `top` on their way)
    assert g.mean() > 0.9 and same_bits(r["t"][g], np.full(g.sum(), 4, f32))
    assert ok[np.flatnonzero(g), r["prim"][g]].all()                       # the oracle's owner is one of the tied candidates


def test_premise_grazing(scene, fams, oracle):
    """The in-band rays are in the band: restated in float32 (as kept) and in float64 (the exact quotient within 2^-19 + 2^-21, the
    reciprocal's own error).  Inside the band the exact float32 quotient decides both ways, and the oracle's answer shows it."""
    fv, F = scene.flat_view(), fams["grazing"]
    inb, n_lo, n_hi, shown = F["in_band"], 0, 0, [0, 0]
    r = oracle["grazing", 3]
    for node in (N_MESH, N_GRID):
        m = fv.mesh_arrays(fv.nodes[node].mesh)
        for tri in np.unique(F["meta"][F["meta"][:, 0] == node, 1]):
            s = (F["meta"][:, 0] == node) & (F["meta"][:, 1] == tri)
            p, q = local_ray(fv, node, F["o"][s], F["d"][s])
            tt = tri_table(m["v"], m["f"][tri:tri + 1], p, q)
            rel32 = np.abs(tt["aperp"][:, 0].astype(np.float64) / float(PERP) - 1)
            assert (rel32[inb[s]] <= 2.0 ** -19).all() and (rel32[~inb[s]] > 2.0 ** -19).all() and (rel32 <= 4 * 2.0 ** -19).all()
            perp64 = np.abs(tt["tdiv"][:, 0].astype(np.float64) / tt["den"][:, 0].astype(np.float64))   # the exact quotient of the kernel's two floats
            assert (np.abs(perp64[inb[s]] / float(PERP) - 1) <= 2.0 ** -19 + 2.0 ** -22).all()
            assert tt["inside"].all() and (tt["t"] > 0).all()               # nothing but the grazing test can reject this triangle
            graz = np.abs(tt["perp"][:, 0]) < PERP
            n_lo += int((graz & inb[s]).sum()); n_hi += int((~graz & inb[s]).sum())
            own = (r["node"][s] == node) & (r["prim"][s] == tri)
            shown[0] += int((own & inb[s]).sum()); shown[1] += int((~own & inb[s]).sum())
            assert not (own & graz).any()
    print(f"grazing band: {n_lo} rays below 0.001745 (rejected), {n_hi} at or above (tested); {int((~inb).sum())} in the ring outside")
    assert n_lo >= 100 and n_hi >= 100 and shown[0] >= 50 and shown[1] >= 50


def test_premise_sphere(scene, fams, oracle):
    fv, F = scene.flat_view(), fams["sphere"]
    for nd in (N_UNIT, N_ELL):
        s = F["node"] == nd
        p, q = local_ray(fv, nd, F["o"][s], F["d"][s])
        Aq, Bq, Cq, DD, t1, t2 = sphere_terms(p, q)
        assert (DD > 0).sum() > 50 and (DD < 0).sum() > 50                  # DD > 0 both ways ...
        if nd == N_UNIT:
            assert (DD[Aq > 0] == 0).sum() >= 12 and (Cq == 0).sum() >= 20     # ... and exactly on it; origins exactly on the surface
        h = DD > 0
        with np.errstate(all="ignore"):
            prod = t1 * t2
        assert (h & (t1 < 0) & (t2 < 0)).any() and (h & (prod < 0)).any() and (h & (t1 > 0) & (t2 > 0)).any()
        if nd == N_UNIT:
            assert (h & (prod == 0)).any()                                  # t1 * t2 <= 0 at equality
        r1, r3 = oracle["sphere", 1], oracle["sphere", 3]
        assert (r1["node"][s] == nd).any() and ((r3["node"][s] == nd) & (r3["front"][s] == 0)).any() and (r3["node"][s] != nd).any()


def test_premise_plane(scene, fams, oracle):
    fv, F = scene.flat_view(), fams["plane"]
    for nd in (N_TOP, N_INNER):
        s = F["node"] == nd
        p, q = local_ray(fv, nd, F["o"][s], F["d"][s])
        t, x = plane_terms(p, q)
        for c in (0, 1):
            for b in (1, -1):
                on, out, inn = x[:, c] == f32(b), b * x[:, c] > 1, (b * x[:, c] < 1) & (b * x[:, c] > 0.999)
                assert on.any() and out.any() and inn.any(), (nd, c, b)          # x > 1 / x < -1: inside, ON the bound, outside
        if nd == N_TOP:
            assert (q[:, 2] == 0).sum() >= 4 and (p[:, 2] == 0).sum() >= 9      # d.z == 0, p.z == 0 (t <= 0)
        r = oracle["plane", 3]
        assert (r["node"][s] == nd).any() and (r["node"][s] != nd).any()
        assert not np.signbit(p[p[:, 2] == 0, 2]).any()                        # -0.0 is unreachable (fam_plane)
    assert (np.signbit(F["d"][:, 2]) & (F["d"][:, 2] == 0)).any()


def _slab(b, p, d):
    """Box::IntersectRay's tMin / tMax in float64 (premise arithmetic), axes with d == 0 left out."""
    with np.errstate(all="ignore"):
        t1, t2 = (b[None, :3] - p) / d, (b[None, 3:] - p) / d
    lo, hi = np.where(d != 0, np.minimum(t1, t2), -np.inf), np.where(d != 0, np.maximum(t1, t2), np.inf)
    return lo.max(1), hi.min(1)


def test_premise_slabs(scene, fams):
    fv, F = scene.flat_view(), fams["slabs"]
    # (a) equal or nearly equal entry distances into overlapping sibling boxes
    s = F["kind"] == 0
    p, q = local_ray(fv, N_MESH, F["o"][s], F["d"][s])
    m = fv.mesh_arrays(fv.nodes[N_MESH].mesh)
    bb, data = np.asarray(m["bvh_bounds"], np.float64), m["bvh_data"]
    eq = near = inside = 0
    for i in range(1, len(data)):
        if not data[i] & 0x80000000:
            c1 = int(data[i] & 0x7fffffff)
            a0, a1 = _slab(bb[c1], p.astype(np.float64), q.astype(np.float64))
            b0, b1 = _slab(bb[c1 + 1], p.astype(np.float64), q.astype(np.float64))
            both = (a0 <= a1) & (b0 <= b1)
            eq += int((both & (a0 == b0)).sum())
            near += int((both & (np.abs(a0 - b0) <= 2.0 ** -19 * (np.abs(a0) + np.abs(b0)))).sum())
            inside += int((both & (a0 < 0) & (b0 < 0)).sum())
    assert eq > 200 and near >= eq and inside > 200
    # (b) rays in a box face
    s = F["kind"] == 1
    p, q = local_ray(fv, N_GRID, F["o"][s], F["d"][s])
    gb = fv.mesh_arrays(fv.nodes[N_GRID].mesh)["bvh_bounds"][1:]
    for a in (0, 1):
        z = q[:, a] == 0
        assert z.sum() > 50 and np.isin(p[z, a], np.concatenate([gb[:, a], gb[:, a + 3]])).all()
    # (c) tiny and huge components, restated in object space
    s = F["kind"] == 2
    p, q = local_ray(fv, N_GRID, F["o"][s], F["d"][s])
    ax = np.abs(q[:, 0])
    sub = (ax > 0) & (ax < 1.17549435e-38)
    assert sub.any() and (ax == step(FAST_ABS, -1)).any() and (ax == FAST_ABS).any() and (ax == step(FAST_ABS, 1)).any()
    assert (ax == step(FAST_BIG, -1)).any() and (ax == FAST_BIG).any() and (ax == step(FAST_BIG, 1)).any()
    assert (p[:, 0] == 0).all()


def test_premise_bias_range(scene, fams, oracle):
    """Per primitive type (sphere, triangle): t < t_max is strict — rays exist for which t_max at the oracle's hit t does not block, the
    next float up does and the next float down does not; the restated any-hit t of the scanned rays lies on both sides of each bias, a
    few float steps away; and the oracle's answers along the scans fall both ways."""
    fv, F, vis = scene.flat_view(), fams["bias_range"], oracle["bias_range"]
    w, n = F["what"], F["n_hits"]
    at, up, dn = vis[:n], vis[n:2 * n], vis[2 * n:3 * n]
    ty = np.array([fv.nodes[k].obj_type for k in F["node"]])
    for kind in (1, 3):
        k = ty[:n] == kind
        assert ((up == 0) & (at == 1) & (dn == 1) & k).sum() > 20, kind
    for tag, bias in ((1, SHADOW_BIAS), (2, TRI_BIAS)):
        s = w == tag
        t = _restated_shadow_t(fv, (F["node"][s], F["prim"][s]), F["o"][s], F["d"][s])
        close = np.abs(t.astype(np.float64) / float(bias) - 1) < 1e-5           # within ~100 float steps of the bias
        for kind in (1, 3):
            k = (ty[s] == kind) & close
            assert (t[k] > bias).sum() > 20 and (t[k] <= bias).sum() > 20, (tag, kind)
            assert (vis[s][k] == 0).sum() > 10 and (vis[s][k] == 1).sum() > 10, (tag, kind)


def test_premise_plane_shadow(scene, fams, oracle):
    """Per plane node and per comparison of the any-hit plane test, restated in float32 and seen in the oracle's answers: the parent-
    space hit point lies inside, exactly on and outside each of the four bounds, and visibility falls both ways along those scans; among
    rays that pass the extent, t lies on both sides of BHRT_SHADOW_BIAS within a few floats and visibility falls both ways; t_max at t
    does not block, the next float up does, the next float down does not."""
    fv, F, vis = scene.flat_view(), fams["plane_shadow"], oracle["plane_shadow"]
    for nd in (N_TOP, N_INNER):
        s = F["node"] == nd
        t, x = plane_anyhit_terms(fv, nd, F["o"][s], F["d"][s])
        w, v = F["what"][s], vis[s]
        inside = (np.abs(x[:, 0]) <= 1) & (np.abs(x[:, 1]) <= 1)
        e = w == 0
        for c in (0, 1):
            for b in (1, -1):
                near = e & (np.abs(x[:, c] - f32(b)) < 1e-5) & (np.abs(x[:, 1 - c]) <= 1)
                on, out, inn = near & (x[:, c] == f32(b)), near & (b * x[:, c] > 1), near & (b * x[:, c] < 1)
                assert on.any() and out.any() and inn.any(), (nd, c, b)
                assert (v[on] == 0).all() and (v[inn] == 0).all() and (v[out] == 1).all(), (nd, c, b)   # nothing else decides these rays
        bsc = (w == 1) & inside
        assert (np.abs(t[bsc].astype(np.float64) / float(SHADOW_BIAS) - 1) < 1e-5).all()
        assert (t[bsc] > SHADOW_BIAS).sum() > 20 and (t[bsc] <= SHADOW_BIAS).sum() > 20
        assert (v[bsc][t[bsc] > SHADOW_BIAS] == 0).all() and (v[bsc][t[bsc] <= SHADOW_BIAS] == 1).all()
        at, up, dn = (w == 2) & inside, (w == 3) & inside, (w == 4) & inside
        assert at.sum() >= 20 and (F["tmax"][s][at] == t[at]).all()
        assert (v[at] == 1).all() and (v[up] == 0).all() and (v[dn] == 1).all()


# ------------------------------------------------------------------------------------------------ oracle -> golden (CPU)
def test_oracle_equals_the_reference(fams, oracle, gold):
    for k in closest_names(fams):
        for side in SIDES:
            r = oracle[k, side]
            assert np.array_equal(r["node"], gold[f"{k}_node_{side}"]), (k, side)
            hit = r["node"] >= 0
            assert np.array_equal(r["front"][hit], gold[f"{k}_front_{side}"][hit]), (k, side)
            assert np.array_equal(r["t"].view(np.uint32)[hit], gold[f"{k}_zbits_{side}"][hit]), (k, side)
            assert sha(r["attrs"][hit][:, 1:7]) == str(gold[f"{k}_pN_sha_{side}"]), (k, side)     # p and N: a wrong triangle shows in N
    for k in shadow_names(fams):
        assert np.array_equal(oracle[k].astype(np.int8), gold[f"{k}_vis"]), k
        assert len(oracle[k]) == len(gold[f"{k}_vis"])


# ------------------------------------------------------------------------------------------------ GPU -> oracle
def _perm(n):
    return np.random.default_rng(1234).permutation(n)


@pytest.mark.gpu
@pytest.mark.parametrize("side", SIDES)
def test_gpu_closest_equals_the_oracle(side, gpu, scene, fams, oracle):
    for k in closest_names(fams):
        o, d, r = fams[k]["o"], fams[k]["d"], oracle[k, side]
        n = len(o)
        cut = n - (1 if n % 64 == 0 else 0)                                    # a batch length that is no multiple of 64
        p = _perm(n)[:cut]
        for idx in (np.arange(cut), p):
            h = scene.trace_closest(o[idx], d[idx], side)
            assert np.array_equal(h["node"], r["node"][idx]), (k, "node")
            assert np.array_equal(h["prim"], r["prim"][idx]), (k, "prim")
            hit = h["node"] >= 0
            assert np.array_equal(h["front"][hit], r["front"][idx][hit]), (k, "front")
            assert same_bits(h["t"], r["t"][idx]), (k, "t")
        if n % 64 == 0:
            h = scene.trace_closest(o[-1:], d[-1:], side)
            assert h["node"][0] == r["node"][-1] and h["prim"][0] == r["prim"][-1] and same_bits(h["t"], r["t"][-1:])


@pytest.mark.gpu
def test_gpu_shadow_equals_the_oracle(gpu, scene, fams, oracle):
    for k in shadow_names(fams):
        o, d, tm, r = fams[k]["o"], fams[k]["d"], fams[k]["tmax"], oracle[k]
        n = len(o)
        cut = n - (1 if n % 64 == 0 else 0)
        for idx in (np.arange(cut), _perm(n)[:cut]):
            assert np.array_equal(scene.trace_shadow(o[idx], d[idx], tm[idx]), r[idx]), k
        if n % 64 == 0:
            assert np.array_equal(scene.trace_shadow(o[-1:], d[-1:], tm[-1:]), r[-1:]), k


# ------------------------------------------------------------------------------------------------ the parked render-path walks
GRID_XML = """<xml><scene><background r="0.1" g="0.1" b="0.2"/><environment r="0.4" g="0.4" b="0.5"/>
  <object type="plane" name="floor" material="w"><scale value="60"/><translate z="-3"/></object>
  <object type="obj" name="grid.obj" material="g"/>
  <object type="sphere" name="s" material="r"><scale value="2"/><translate x="5" y="3" z="4"/></object>
  <material type="blinn" name="w"><diffuse value="0.8"/><specular value="0.1"/></material>
  <material type="blinn" name="r"><diffuse r="0.8" g="0.2" b="0.2"/><specular value="0.4"/><glossiness value="20"/></material>
  <material type="blinn" name="g"><diffuse r="0.3" g="0.7" b="0.4"/><specular value="0.5"/><glossiness value="40"/></material>
  <light type="point" name="p"><intensity value="400"/><position x="6" y="-8" z="20"/><size value="1"/></light></scene>
  <camera><position x="0" y="0" z="24"/><target x="0" y="0" z="0"/><up x="0" y="1" z="0"/><fov value="90"/><width value="64"/><height value="48"/></camera></xml>"""


@pytest.mark.gpu
def test_render_walks_on_grid_vertices(gpu, B, O, tmp_path):
    """k_trace_mesh's camera form, mesh_closest_vote, the slow queue's mesh_closest_coop and k_shadow_mesh cannot be fed rays; a scene
    feeds them.  A flat 64 x 48 grid of pitch 1 under a camera 24 above it with a 90 degree field of view: the pixel pitch on z = 0 is
    the grid pitch, so with jitter off every primary ray meets the mesh at a grid vertex to within rounding, where up to six coplanar
    triangles tie; column 32 and row 24 are axis-parallel rays (the slow queue).  Every triangle has its own corner normals and
    texture coordinates, so a wrong prim changes the radiance."""
    write_grid_obj(str(tmp_path / "grid.obj"), 64, 48, 1.0)
    (tmp_path / "g.xml").write_text(GRID_XML)
    sc = B.Scene(str(tmp_path / "g.xml"))
    blob, W, H = sc.flat_bytes(), sc.width, sc.height
    o, d = O.primary_rays(sc.flat_view())
    r = O.trace_closest(blob, o, d, 1)
    mesh = r["node"] == 1
    xy = r["attrs"][mesh][:, 1:3].astype(np.float64)
    off = np.abs(xy - np.round(xy)).min(1)                                       # distance to the nearest grid line, in pitches
    assert mesh.sum() > W * H // 2 and (off <= 1e-5).mean() >= 0.9
    assert (d[:, 0] == 0).sum() == H and (d[:, 1] == 0).sum() == W               # the axis-parallel column and row
    z, nrm, alb = sc.first_hit()
    oz, on, oa = O.first_hit(blob, W, H)
    assert same_bits(z.ravel(), oz) and same_bits(nrm.reshape(-1, 3), on) and same_bits(alb.reshape(-1, 3), oa)
    assert np.array_equal(sc.first_hit_node().ravel(), r["node"])
    for gi in (0, 2):
        ro = O.render(blob, W, H, 1, gi=gi, seed=5, jitter=0)["samples"]
        for ls in (0, 1):
            gs, _ = sc.render_samples(B.default_opts(spp=1, gi_bounces=gi, seed=5, jitter=0, leaf_skip=ls), 0, 0, W, H)
            assert same_bits(gs, ro), (gi, ls)
    sc.close()                                                                   # nothing of this scene stays on the device for the tests that follow
