"""Times the spatial variance estimate (csrc/temporal.hip stage 3S) with the method of tools/temporal_var_timing.py:
tests/scenes/c3_mesh.xml at 1920x1080, a 1-spp render of the scene's camera, the guides given; every figure the median of --reps calls after
3 warm-ups, each call between two HIP events on the call's stream.  Beside it one level of the denoiser's k_dn_step in the same run:
bhrt_denoise_dev with a variance at K = 2 (prepare + a level + the last level) minus K = 1 (prepare + the last level).  Prints one JSON line
with the algorithmic bytes per pixel:
    estimate            radiance 12 + z 4 + normal 12 + albedo 12 read, out 12 written: 52 (40 without demodulation)
    with v and l        + variance 12 + length 4 read: 68
    one k_dn_step       two float4 planes read, one written: 48
The halo re-reads of a 16 x 16 workgroup ((16 + 2R)^2 / 256 of the read bytes, 1.89 at R = 3) come from the cache and are not counted.
Run it twice (two processes) and keep both lines."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import bhraytracer_amd as B
    from conftest import ensure_mesh
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda", 0)
    ensure_mesh(224)
    sc = B.Scene(os.path.join(ROOT, "tests/scenes/c3_mesh.xml"))
    sc.upload(0)
    W, H = sc.width, sc.height
    px = W * H
    f3 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device=dev)  # noqa: E731
    z, n, al, rad, var, out, den = torch.zeros((H, W), dtype=torch.float32, device=dev), f3(), f3(), f3(), f3(), f3(), f3()
    sc.first_hit_dev(z.data_ptr(), n.data_ptr(), al.data_ptr())
    sc.render_var_dev(B.default_opts(spp=1, seed=1), 0, rad.data_ptr(), var.data_ptr())
    torch.manual_seed(1)
    ln = torch.randint(0, 9, (H, W), device=dev).float()       # half of the pixels below min_length = 4
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def timed(call):
        for _ in range(3):
            call()
        s.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            s.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    P = lambda t: t.data_ptr()  # noqa: E731
    res = {"frame": f"{W}x{H}", "reps": a.reps, "lib": os.path.basename(B.LIB_PATH)}
    for R in (1, 2, 3, 4):
        o = B.default_spatial_variance_opts(radius=R)
        res[f"estimate_r{R}"] = dict(timed(lambda: sc.variance_spatial_dev(o, P(rad), 0, 0, P(z), P(n), P(al), P(out), s.cuda_stream)), bytes_per_pixel=52)
    o3, o3n = B.default_spatial_variance_opts(), B.default_spatial_variance_opts(demodulate=0)
    res["estimate_r3_no_demodulation"] = dict(timed(lambda: sc.variance_spatial_dev(o3n, P(rad), 0, 0, P(z), P(n), 0, P(out), s.cuda_stream)), bytes_per_pixel=40)
    res["estimate_r3_with_length"] = dict(timed(lambda: sc.variance_spatial_dev(o3, P(rad), P(var), P(ln), P(z), P(n), P(al), P(out), s.cuda_stream)), bytes_per_pixel=68)
    res["estimate_r3_guides_computed"] = dict(timed(lambda: sc.variance_spatial_dev(o3, P(rad), 0, 0, 0, 0, 0, P(out), s.cuda_stream)), bytes_per_pixel=52)
    sc.variance_spatial_dev(o3, P(rad), 0, 0, P(z), P(n), P(al), P(var))
    for K in (1, 2):
        dn = B.default_denoise_opts(iterations=K)
        res[f"denoise_k{K}"] = timed(lambda: sc.denoise_dev(dn, P(rad), P(var), P(z), P(n), P(al), P(den), 0, stream=s.cuda_stream))
    res["one_dn_step"] = {"ms_median": res["denoise_k2"]["ms_median"] - res["denoise_k1"]["ms_median"], "bytes_per_pixel": 48}
    for k, r in res.items():
        if isinstance(r, dict) and "bytes_per_pixel" in r:
            r["GBps"] = r["bytes_per_pixel"] * px / r["ms_median"] / 1e6
    res["checksum"] = float(var.double().sum()) + float(den.double().sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
