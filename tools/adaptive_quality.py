"""Time to quality of adaptive sampling (bhrt_render_adaptive) against uniform frames, at the scenes' full size (1920x1080).

For every scene: a reference frame of --ref-spp samples per pixel with a DIFFERENT seed, uniform frames of 32 / 64 / 128 spp and adaptive
frames (min 16, max 256) over a grid of thresholds and floors; each line gives the MSE of the linear radiance against the reference and the
render's wall time (bhrt_stats.seconds_total, scene resident, outputs in HBM; the best of --reps renders after a warm-up render).  Prints one
JSON line per frame, then a summary line per scene: the cheapest adaptive setting whose MSE is at most uniform-64's, and its time over
uniform-64's.  --once: one uniform (64 spp) and one adaptive frame (the defaults) of the first scene, for a profiler run
(`rocprofv3 --kernel-trace --stats -- python tools/adaptive_quality.py --once`).  --time-only: per scene, only the wall times of 1 + --reps adaptive
frames (min 16, max 256, the first threshold and floor), one JSON line; with BHRT_LIB set, of that build: run it in turns to compare two builds."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3_room,c2_glass,c3_mesh")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--thresholds", default="0.01,0.02,0.03,0.05")
    ap.add_argument("--floors", default="0.05,0.1")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--time-only", action="store_true")
    a = ap.parse_args()
    import torch
    import bhraytracer_amd as B
    from conftest import ensure_mesh
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    ensure_mesh(224)
    dev = torch.device("cuda", 0)
    for name in a.scenes.split(","):
        sc = B.Scene(os.path.join(ROOT, "tests", "scenes", name + ".xml"))
        sc.upload(0)
        W, H = sc.width, sc.height
        rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        cnt = torch.zeros((H, W), dtype=torch.int32, device=dev)

        def uniform(spp, seed=1, reps=a.reps):
            sts = [sc.render_dev(B.default_opts(spp=spp, seed=seed), rgb.data_ptr(), rad.data_ptr()) for _ in range(1 + reps)]
            return rad.cpu().numpy().copy(), min(s.seconds_total for s in sts[1:] or sts), sts[-1]

        def adaptive(ao, spp=256):
            sts = [sc.render_adaptive_dev(B.default_opts(spp=spp, seed=1), ao, rgb.data_ptr(), rad.data_ptr(), 0, cnt.data_ptr()) for _ in range(1 + a.reps)]
            return rad.cpu().numpy().copy(), min(s.seconds_total for s in sts[1:]), sts[-1]

        if a.once:
            uniform(64)
            adaptive(B.default_adaptive_opts())
            print(json.dumps({"scene": name, "once": True}))
            return
        if a.time_only:
            ao = B.default_adaptive_opts(min_spp=16, threshold=float(a.thresholds.split(",")[0]), floor=float(a.floors.split(",")[0]))
            sts = [sc.render_adaptive_dev(B.default_opts(spp=256, seed=1), ao, rgb.data_ptr(), rad.data_ptr(), 0, cnt.data_ptr()) for _ in range(1 + a.reps)]
            print(json.dumps({"scene": name, "lib": B.LIB_PATH, "warmup_s": sts[0].seconds_total, "seconds": [s.seconds_total for s in sts[1:]],
                              "samples": sts[-1].camera_samples, "passes": sts[-1].passes}), flush=True)
            continue
        ref, _, _ = uniform(a.ref_spp, seed=1000, reps=0)
        rows = []
        for spp in (32, 64, 128):
            img, t, st = uniform(spp)
            rows.append({"scene": name, "mode": "uniform", "spp": spp, "mse": float(np.mean((img - ref) ** 2)), "seconds": t, "samples": st.camera_samples})
            print(json.dumps(rows[-1]), flush=True)
        for fl in (float(x) for x in a.floors.split(",")):
            for th in (float(x) for x in a.thresholds.split(",")):
                img, t, st = adaptive(B.default_adaptive_opts(min_spp=16, threshold=th, floor=fl))
                c = cnt.cpu().numpy()
                rows.append({"scene": name, "mode": "adaptive", "min_spp": 16, "max_spp": 256, "threshold": th, "floor": fl, "mse": float(np.mean((img - ref) ** 2)),
                             "seconds": t, "samples": st.camera_samples, "mean_spp": float(c.mean()), "at_min": float((c == 16).mean()),
                             "at_max": float((c == 256).mean()), "passes": st.passes})
                print(json.dumps(rows[-1]), flush=True)
        u64 = next(r for r in rows if r["mode"] == "uniform" and r["spp"] == 64)
        ok = [r for r in rows if r["mode"] == "adaptive" and r["mse"] <= u64["mse"]]
        best = min(ok, key=lambda r: r["seconds"]) if ok else None
        print(json.dumps({"scene": name, "summary": True, "uniform64_mse": u64["mse"], "uniform64_s": u64["seconds"],
                          "best_adaptive": best, "time_ratio": best["seconds"] / u64["seconds"] if best else None}), flush=True)


if __name__ == "__main__":
    main()
