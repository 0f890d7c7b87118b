"""Times the face-material switch (bhrt_scene_set_face_materials) on the three-group room (tests/scenes/facemtl_room.xml with the
camera's frame set to --width x --height, default 1920x1080, 16 spp), scene resident, outputs left in HBM:
    off  the frame as the reference renders it: the whole mesh in sub-material 0
    on   every face in its own sub-material: other kernels (k_shade<.., kFm>) AND another image (a third of the mesh refracts), so on - off is
         not the cost of the lookup alone
One warm-up render of each, then --reps rounds that alternate them.  Times are bhrt_stats.seconds_total (a host clock around the render, which
ends in a stream synchronise).  Prints one JSON line with each variant's times, mean and spread."""
import argparse
import json
import os
import re
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import torch
    import bhraytracer_amd as B
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda", 0)
    scenes = os.path.join(ROOT, "tests", "scenes")
    with tempfile.TemporaryDirectory() as d:
        for asset in ("facemtl.obj", "facemtl.mtl", "tex_small.png"):
            shutil.copy(os.path.join(scenes, asset), os.path.join(d, asset))
        text = open(os.path.join(scenes, "facemtl_room.xml")).read()
        text, n1 = re.subn(r'<width value="\d+"/>', f'<width value="{a.width}"/>', text)
        text, n2 = re.subn(r'<height value="\d+"/>', f'<height value="{a.height}"/>', text)
        assert n1 == 1 and n2 == 1
        with open(os.path.join(d, "room.xml"), "w") as fp:
            fp.write(text)
        sc = B.Scene(os.path.join(d, "room.xml"))
    sc.upload(0)
    W, H = sc.width, sc.height
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    variants = (("off", False), ("on", True))
    times = {n: [] for n, _ in variants}
    stats = {}

    def render(on):
        sc.set_face_materials(on)
        return sc.render_dev(B.default_opts(spp=a.spp, gi_bounces=3), rgb.data_ptr(), rad.data_ptr())
    for _, on in variants:  # warm-up: code objects, workspace, the learned pass sizes
        render(on)
    for _ in range(a.reps):
        for name, on in variants:
            st = render(on)
            times[name].append(st.seconds_total * 1e3)
            stats[name] = {"closest_rays": st.closest_rays, "shadow_rays": st.shadow_rays, "shade_calls": st.shade_calls, "wave_steps": st.wave_iterations,
                           "passes": st.passes, "mean_radiance": float(rad.mean().item())}
    res = {"scene": "facemtl_room", "frame": f"{W}x{H} x {a.spp} spp", "reps": a.reps}
    for name, t in times.items():
        res[name] = {"ms": [round(x, 3) for x in t], "mean_ms": sum(t) / len(t), "spread_ms": max(t) - min(t), **stats[name]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
