"""Times the global gather (bhrt_scene_set_global_gather) on the closed Cornell room of the bench (tests/scenes/c3_room.xml,
1920x1080 as committed, --spp samples, default 16), scene resident, outputs left in HBM:
    off  gi_bounces = 3, the switch off: the frame as the reference renders it
    on   gi_bounces = 0, the switch on, a global map of --photons photons (default 10^6) at --radius (default the reference's 0.5)
The two are DIFFERENT ESTIMATORS of the frame: three GI bounces traced against one GI bounce whose end gathers from the map.  No image equality
is claimed or checked; `mean_radiance` of each is printed for orientation only.
One warm-up render of each, then --reps rounds that alternate them.  Times are bhrt_stats.seconds_total (a host clock around the render, which
ends in a stream synchronise); the map's build time is the host clock around bhrt_global_map_build.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--photons", type=int, default=1000000)
    ap.add_argument("--radius", type=float, default=0.5)
    a = ap.parse_args()
    import torch
    import bhraytracer_amd as B
    from conftest import ensure_mesh
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    ensure_mesh(224)  # the room's mesh, written on demand
    dev = torch.device("cuda", 0)
    sc = B.Scene(os.path.join(ROOT, "tests", "scenes", "c3_room.xml"))
    sc.upload(0)
    t0 = time.perf_counter()
    n = sc.global_map_build(B.default_opts(seed=0), a.photons)
    build_s = time.perf_counter() - t0
    W, H = sc.width, sc.height
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    variants = (("off_gi3", False, 3), ("on_gi0", True, 0))
    times = {v[0]: [] for v in variants}
    stats = {}

    def render(on, gi):
        sc.set_global_gather(on, a.radius)
        return sc.render_dev(B.default_opts(spp=a.spp, gi_bounces=gi), rgb.data_ptr(), rad.data_ptr())
    for _, on, gi in variants:  # warm-up: code objects, workspace, the learned pass sizes
        render(on, gi)
    for _ in range(a.reps):
        for name, on, gi in variants:
            st = render(on, gi)
            times[name].append(st.seconds_total * 1e3)
            stats[name] = {"closest_rays": st.closest_rays, "shadow_rays": st.shadow_rays, "shade_calls": st.shade_calls, "wave_steps": st.wave_iterations,
                           "passes": st.passes, "seconds_global_gather": st.seconds_global_gather, "global_gather_queries": st.global_gather_queries,
                           "global_gather_heavy_queries": st.global_gather_heavy_queries, "mean_radiance": float(rad.mean().item())}
    res = {"scene": "c3_room", "frame": f"{W}x{H} x {a.spp} spp", "reps": a.reps, "photons": n, "radius": a.radius, "map_build_s": build_s}
    for name, t in times.items():
        res[name] = {"ms": [round(x, 3) for x in t], "mean_ms": sum(t) / len(t), "spread_ms": max(t) - min(t), **stats[name]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
