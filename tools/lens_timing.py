"""Times the thin-lens camera (bhrt_opts.lens) on the C3 headline frame (tests/scenes/c3_mesh.xml, 1920x1080, 64 spp),
focused on the mesh (bhrt_scene_set_lens), scene resident, outputs left in HBM:
    a  lens = 0                               the pinhole render
    b  lens = 1, aperture radius 1e-6         the rays are the pinhole rays to within rounding: b - a is the cost of the mechanism
                                              (k_lens_rays + the camera step through the queue kernels and the key sort)
    c  lens = 1, aperture radius --dof        c - b is what less coherent camera rays cost the mesh walk: a property of the image
One warm-up render of every variant, then --reps rounds that alternate a, b, c.  Times are bhrt_stats.seconds_total (a host clock around
the render, which ends in a stream synchronise).  Prints one JSON line with each variant's times, mean and spread, and the bytes k_lens_rays
writes (36 B per sample slot); for the kernel's own time run this under `rocprofv3 --kernel-trace --stats` (--reps 1 is enough)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--dof", type=float, default=0.6, help="aperture radius of variant c")
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
    sc = B.Scene(os.path.join(ROOT, "tests", "scenes", a.scene + ".xml"))
    cam = sc.flat_view().header.camera
    # the mesh of c3_mesh sits at (-1, 1, 4.2): focus on its centre
    focus = float(sum((p - q) ** 2 for p, q in zip(cam.pos, (-1.0, 1.0, 4.2))) ** 0.5) if a.scene == "c3_mesh" else float(cam.focaldist)
    sc.upload(0)
    W, H = sc.width, sc.height
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    variants = (("a_pinhole", 0, 0.0), ("b_lens_closed", 1, 1e-6), ("c_lens_open", 1, a.dof))
    times = {n: [] for n, _, _ in variants}
    stats = {}

    def render(lens, dof):
        sc.set_lens(focus, dof)
        return sc.render_dev(B.default_opts(spp=a.spp, gi_bounces=3, lens=lens), rgb.data_ptr(), rad.data_ptr())
    for name, lens, dof in variants:  # warm-up: code objects, workspace, the learned pass sizes
        render(lens, dof)
    for _ in range(a.reps):
        for name, lens, dof in variants:
            st = render(lens, dof)
            times[name].append(st.seconds_total * 1e3)
            stats[name] = {"closest_rays": st.closest_rays, "shadow_rays": st.shadow_rays, "wave_steps": st.wave_iterations, "passes": st.passes}
    res = {"scene": a.scene, "frame": f"{W}x{H} x {a.spp} spp", "focaldist": focus, "dof_c": a.dof, "reps": a.reps,
           "lens_rays_bytes": W * H * a.spp * 36}
    for name, t in times.items():
        res[name] = {"ms": [round(x, 3) for x in t], "mean_ms": sum(t) / len(t), "spread_ms": max(t) - min(t), **stats[name]}
    res["b_minus_a_ms"] = res["b_lens_closed"]["mean_ms"] - res["a_pinhole"]["mean_ms"]
    res["c_minus_b_ms"] = res["c_lens_open"]["mean_ms"] - res["b_lens_closed"]["mean_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
