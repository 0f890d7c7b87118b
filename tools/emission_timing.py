"""Times the emission term (bhrt_scene_set_emissive) on the closed-room frame (tests/scenes/c3_room.xml, 1920x1080, 64 spp),
scene resident, outputs left in HBM:
    a  term off                                   the frame as the reference renders it
    b  term on, every emission (0, 0, 0)          the emission-on kernels (k_combine<true>, k_resolve_frames<.., true>) adding zeros:
                                                  b - a is the cost of the mechanism, the image is a's
    c  term on, material --material emits --le         c - b is what the light does to the paths: a property of the image
--material names the emitter (default "wallRed": the left wall of the room).
One warm-up render of every variant, then --reps rounds that alternate a, b, c.  Times are bhrt_stats.seconds_total (a host clock around the
render, which ends in a stream synchronise).  Prints one JSON line with each variant's times, mean and spread."""
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
    ap.add_argument("--le", type=float, default=0.5, help="emission of variant c, all three channels")
    ap.add_argument("--scene", default="c3_room")
    ap.add_argument("--material", default="wallRed")
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
    mi = sc.material_index(a.material)
    sc.upload(0)
    W, H = sc.width, sc.height
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    variants = (("a_off", False, 0.0), ("b_on_black", True, 0.0), ("c_on_emitting", True, a.le))
    times = {n: [] for n, _, _ in variants}
    stats = {}

    def render(on, le):
        sc.set_material_emission(mi, (le, le, le))
        sc.set_emissive(on)
        return sc.render_dev(B.default_opts(spp=a.spp, gi_bounces=3), rgb.data_ptr(), rad.data_ptr())
    for name, on, le in variants:  # warm-up: code objects, workspace, the learned pass sizes
        render(on, le)
    for _ in range(a.reps):
        for name, on, le in variants:
            st = render(on, le)
            times[name].append(st.seconds_total * 1e3)
            stats[name] = {"closest_rays": st.closest_rays, "shadow_rays": st.shadow_rays, "shade_calls": st.shade_calls, "wave_steps": st.wave_iterations,
                           "passes": st.passes, "mean_radiance": float(rad.mean().item())}
    res = {"scene": a.scene, "frame": f"{W}x{H} x {a.spp} spp", "emitter": a.material, "le_c": a.le, "reps": a.reps}
    for name, t in times.items():
        res[name] = {"ms": [round(x, 3) for x in t], "mean_ms": sum(t) / len(t), "spread_ms": max(t) - min(t), **stats[name]}
    res["b_minus_a_ms"] = res["b_on_black"]["mean_ms"] - res["a_off"]["mean_ms"]
    res["c_minus_b_ms"] = res["c_on_emitting"]["mean_ms"] - res["b_on_black"]["mean_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
