"""Times the camera shutter (bhrt_scene_set_shutter) on the C3 headline frame (tests/scenes/c3_mesh.xml, 1920x1080, 64 spp), scene
resident, outputs left in HBM:
    a   lens = 0, no shutter                  the pinhole render
    b   lens = 1, aperture radius 1e-6        the stored-ray route alone (k_lens_rays + the camera step through the queue kernels)
    s0  shutter on, pose 1 = pose 0           the same route with k_shutter_rays: s0 - b is the per-sample frame arithmetic
    s1  shutter on, about --pixels of motion  a sideways move that shifts the mesh by that many pixels: s1 - s0 is what less coherent camera
                                              rays cost the walk, a property of the image
One warm-up render of every variant, then --reps rounds that alternate them.  Times are bhrt_stats.seconds_total.  Prints one JSON line with
each variant's times, mean and spread, and the bytes k_shutter_rays writes (36 B per sample slot); for the kernel's own time run this under
`rocprofv3 --kernel-trace --stats` (--reps 1 is enough)."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def xml_pose(path):
    """position, target, up of the scene file's <camera>."""
    cam = open(path).read().split("<camera>")[1]
    out = []
    for tag in ("position", "target", "up"):
        m = re.search(r"<%s ([^>]*)/>" % tag, cam)
        out.append(tuple(float(re.search(r'%s="([^"]*)"' % k, m.group(1)).group(1)) for k in "xyz"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--pixels", type=float, default=10.0, help="motion of variant s1, in pixels at the mesh's distance")
    ap.add_argument("--scene", default="c3_mesh")
    a = ap.parse_args()
    import torch
    import bhraytracer_amd as B
    from conftest import ensure_mesh
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda", 0)
    if a.scene in ("c3_mesh", "c3_room", "c4_mesh_4k"):
        ensure_mesh(224)
    path = os.path.join(ROOT, "tests", "scenes", a.scene + ".xml")
    sc = B.Scene(path)
    cam = sc.flat_view().header.camera
    pos, target, up = xml_pose(path)
    # the mesh of c3_mesh sits at (-1, 1, 4.2); a sideways move of v shifts a point at distance D by v / D * focaldist on the image plane
    dist = float(sum((p - q) ** 2 for p, q in zip(cam.pos, (-1.0, 1.0, 4.2))) ** 0.5) if a.scene == "c3_mesh" else float(cam.focaldist)
    ddx = np.array(list(cam.dd_x), np.float64)
    move = ddx * (a.pixels * dist / float(cam.focaldist))
    moved = (tuple(np.array(pos) + move), tuple(np.array(target) + move), up)
    sc.upload(0)
    W, H = sc.width, sc.height
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    variants = (("a_pinhole", 0, None), ("b_lens_closed", 1, None), ("s0_shutter_still", 0, (pos, target, up)), ("s1_shutter_moving", 0, moved))
    times = {n: [] for n, _, _ in variants}
    stats = {}

    def render(lens, pose1):
        sc.set_lens(0.0, 1e-6 if lens else 0.0)
        if pose1 is None:
            sc.set_shutter(False)
        else:
            sc.set_shutter(True, *pose1)
        return sc.render_dev(B.default_opts(spp=a.spp, gi_bounces=3, lens=lens), rgb.data_ptr(), rad.data_ptr())
    for name, lens, pose1 in variants:  # warm-up: code objects, workspace, the learned pass sizes
        render(lens, pose1)
    for _ in range(a.reps):
        for name, lens, pose1 in variants:
            st = render(lens, pose1)
            times[name].append(st.seconds_total * 1e3)
            stats[name] = {"closest_rays": st.closest_rays, "shadow_rays": st.shadow_rays, "wave_steps": st.wave_iterations, "passes": st.passes}
    res = {"scene": a.scene, "frame": f"{W}x{H} x {a.spp} spp", "pixels": a.pixels, "move": [float(x) for x in move], "reps": a.reps,
           "shutter_rays_bytes": W * H * a.spp * 36}
    for name, t in times.items():
        res[name] = {"ms": [round(x, 3) for x in t], "mean_ms": sum(t) / len(t), "spread_ms": max(t) - min(t), **stats[name]}
    res["b_minus_a_ms"] = res["b_lens_closed"]["mean_ms"] - res["a_pinhole"]["mean_ms"]
    res["s0_minus_b_ms"] = res["s0_shutter_still"]["mean_ms"] - res["b_lens_closed"]["mean_ms"]
    res["s0_minus_a_ms"] = res["s0_shutter_still"]["mean_ms"] - res["a_pinhole"]["mean_ms"]
    res["s1_minus_s0_ms"] = res["s1_shutter_moving"]["mean_ms"] - res["s0_shutter_still"]["mean_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
