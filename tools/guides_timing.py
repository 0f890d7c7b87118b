"""Times the sampled guide images (bhrt_guides_dev) on the C3 headline frame (tests/scenes/c3_mesh.xml, 1920x1080), scene
resident, outputs left in HBM:
    first_hit   bhrt_first_hit_dev                                    one pinhole ray per pixel, the guides the denoiser computes itself
    guides      bhrt_guides_dev at --spp samples per pixel, jittered  lens = 0 and, focused on the mesh with aperture --dof, lens = 1
    frame       bhrt_render_dev at --frame-spp                        one frame of the scene, what the guides' cost is held against
One warm-up call of every variant, then --reps rounds that alternate them.  Times are a host clock around a call that ends in a stream
synchronise.  Prints one JSON line with each variant's times, median and spread; for the kernel's own time run this under
`rocprofv3 --kernel-trace --stats` (--reps 1 is enough)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16, help="guide samples per pixel")
    ap.add_argument("--frame-spp", type=int, default=64)
    ap.add_argument("--dof", type=float, default=0.6)
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
    focus = float(sum((p - q) ** 2 for p, q in zip(cam.pos, (-1.0, 1.0, 4.2))) ** 0.5) if a.scene == "c3_mesh" else float(cam.focaldist)
    sc.set_lens(focus, a.dof)
    sc.upload(0)
    W, H = sc.width, sc.height
    z = torch.zeros((H, W), dtype=torch.float32, device=dev)
    nrm = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    alb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    cov = torch.zeros((H, W), dtype=torch.float32, device=dev)
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    variants = {
        "first_hit": lambda: sc.first_hit_dev(z.data_ptr(), nrm.data_ptr(), alb.data_ptr()),
        "guides_pinhole": lambda: sc.guides_dev(B.default_opts(spp=a.spp, lens=0), z.data_ptr(), nrm.data_ptr(), alb.data_ptr(), cov.data_ptr()),
        "guides_lens": lambda: sc.guides_dev(B.default_opts(spp=a.spp, lens=1), z.data_ptr(), nrm.data_ptr(), alb.data_ptr(), cov.data_ptr()),
        "guides_1spp": lambda: sc.guides_dev(B.default_opts(spp=1, jitter=0), z.data_ptr(), nrm.data_ptr(), alb.data_ptr(), cov.data_ptr()),
        "frame": lambda: sc.render_dev(B.default_opts(spp=a.frame_spp, gi_bounces=3), rgb.data_ptr(), rad.data_ptr()),
    }
    times = {n: [] for n in variants}
    for f in variants.values():  # warm-up: code objects, workspace, the learned pass sizes
        f()
    for _ in range(a.reps):
        for n, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[n].append((time.perf_counter() - t0) * 1e3)
    res = {"scene": a.scene, "frame": f"{W}x{H}", "guide_spp": a.spp, "frame_spp": a.frame_spp, "focaldist": focus, "dof": a.dof, "reps": a.reps,
           "coverage_mean": float(cov.mean().item())}
    for n, t in times.items():
        res[n] = {"ms": [round(x, 3) for x in t], "median_ms": statistics.median(t), "spread_ms": max(t) - min(t)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
