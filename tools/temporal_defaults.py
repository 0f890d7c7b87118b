"""Chooses the defaults of temporal reprojection (BHRT_REPROJECT_*, BHRT_TEMPORAL_* of include/bhrt.h) on the GPU, as
BHRT_DENOISE_SIGMA_COVERAGE was chosen.  On tests/scenes/c3_mesh_small and c4_textured: a 64-spp frame at the scene's camera is reprojected
into the view of the camera moved by (+1.5, 0, +0.5) with the same target (with albedo) and a 4-spp frame there is accumulated onto it; the
figure of merit is the MSE of the result against a 1024-spp frame at the moved camera, over the whole frame, summed over both scenes relative
to each scene's MSE of the 4-spp frame alone.  Two grids, the second at the winners of the first:
    depth_tolerance x normal_threshold   with the clamp off and max_length = +inf
    clamp_k x max_length                  at that pair
Prints one JSON line with both tables."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MOVE = (1.5, 0.0, 0.5)
TOLS = (0.005, 0.01, 0.02, 0.05, 0.1)
THRS = (0.5, 0.8, 0.9, 0.95, 0.99)
CLAMPS = (-1.0, 1.0, 2.0, 3.0, 5.0)
LENGTHS = (16.0, 64.0, 256.0, float("inf"))


def main():
    import bhraytracer_amd as B
    from test_reproject import xml_pose
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    f32 = np.float32
    data = {}
    for name in ("c3_mesh_small", "c4_textured"):
        sc = B.Scene(os.path.join(ROOT, "tests", "scenes", name + ".xml"))
        pos, target, up = xml_pose(name)
        fr0 = sc.camera_frame()
        g0 = sc.first_hit()
        old = sc.render(B.default_opts(spp=64, seed=3))[1]
        sc.set_camera(tuple(p + d for p, d in zip(pos, MOVE)), target, up)
        g1 = sc.first_hit()
        R = sc.render(B.default_opts(spp=1024, seed=77))[1]
        A = sc.render(B.default_opts(spp=4, seed=1))[1]
        data[name] = (sc, fr0, g0, old, g1, R, A)

    def run(name, tol, thr, ck, ml):
        sc, fr0, (z0, n0, a0), old, (z1, n1, a1), R, A = data[name]
        h, l, _ = sc.reproject(B.default_reproject_opts(depth_tolerance=tol, normal_threshold=thr), fr0, z0, n0, old, np.full(z0.shape, 64, f32), a0, z1, n1, a1)
        out = sc.temporal_accumulate(B.default_temporal_opts(clamp_k=ck, max_length=ml), A, 4.0, h, l)[0]
        return float(np.mean((out - R) ** 2)), float((l > 0).mean())

    res = {"noisy_mse": {k: float(np.mean((v[6] - v[5]) ** 2)) for k, v in data.items()}, "grid1": [], "grid2": []}
    score = lambda m: sum(m[k] / res["noisy_mse"][k] for k in data)  # noqa: E731
    best = None
    for tol in TOLS:
        for thr in THRS:
            r = {k: run(k, tol, thr, -1.0, float("inf")) for k in data}
            row = {"depth_tolerance": tol, "normal_threshold": thr, "mse": {k: r[k][0] for k in data}, "valid": {k: r[k][1] for k in data}}
            row["score"] = score(row["mse"])
            res["grid1"].append(row)
            if best is None or row["score"] < best["score"]:
                best = row
    res["best1"] = best
    best2 = None
    for ck in CLAMPS:
        for ml in LENGTHS:
            r = {k: run(k, best["depth_tolerance"], best["normal_threshold"], ck, ml) for k in data}
            row = {"clamp_k": ck, "max_length": ml, "mse": {k: r[k][0] for k in data}}
            row["score"] = score(row["mse"])
            res["grid2"].append(row)
            if best2 is None or row["score"] < best2["score"]:
                best2 = row
    res["best2"] = best2
    print(json.dumps(res).replace("Infinity", '"inf"'))


if __name__ == "__main__":
    main()
