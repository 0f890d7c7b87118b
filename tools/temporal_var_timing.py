"""Times the two variance-carrying stages of temporal reprojection (csrc/temporal.hip stages 1V and 2V) beside the stages they
extend, with the method of tools/temporal_timing.py: tests/scenes/c3_mesh.xml at 1920x1080, the previous view the scene's camera, the current
one moved by (+1.5, 0, +0.5) with the same target; every figure the median of --reps calls after 3 warm-ups, each call between two HIP events
on the call's stream.  Prints one JSON line with the algorithmic bytes per pixel (the guides are given, the albedo images take part):
    reproject        z 4 + normal 12 + albedo 12 read; taps of z' 4 + normal' 12 + radiance' 12 + length' 4 + albedo' 12, counted once per
                     pixel; history 12 + length 4 + motion 8 written: 96
    reproject_var    + variance' 12 read, + history variance 12 written: 120
    accumulate       radiance 12 + history 12 + length 4 read, out 12 + length 4 + rgb8 3 written: 47
    accumulate_var   + variance 12 + history variance 12 read, + out variance 12 written: 83
Run it twice (two processes) and keep both lines."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import bhraytracer_amd as B
    from conftest import ensure_mesh
    from temporal_timing import xml_pose
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda", 0)
    ensure_mesh(224)
    path = os.path.join(ROOT, "tests/scenes/c3_mesh.xml")
    sc = B.Scene(path)
    sc.upload(0)
    W, H = sc.width, sc.height
    px = W * H
    pos, target, up = xml_pose(path)
    f3 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device=dev)  # noqa: E731
    f1 = lambda: torch.zeros((H, W), dtype=torch.float32, device=dev)  # noqa: E731
    pz, pn, pa, prad, pvar = f1(), f3(), f3(), f3(), f3()
    fr0 = sc.camera_frame()
    sc.first_hit_dev(pz.data_ptr(), pn.data_ptr(), pa.data_ptr())
    sc.render_var_dev(B.default_opts(spp=4, seed=1), 0, prad.data_ptr(), pvar.data_ptr())
    plen = torch.full((H, W), 4.0, dtype=torch.float32, device=dev)
    sc.set_camera((pos[0] + 1.5, pos[1], pos[2] + 0.5), target, up)
    z, n, al, rad, var = f1(), f3(), f3(), f3(), f3()
    sc.first_hit_dev(z.data_ptr(), n.data_ptr(), al.data_ptr())
    sc.render_var_dev(B.default_opts(spp=4, seed=2), 0, rad.data_ptr(), var.data_ptr())
    hist, hvar, ln, out, ovar, oln = f3(), f3(), f1(), f3(), f3(), f1()
    mo = torch.zeros((H, W, 2), dtype=torch.float32, device=dev)
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
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

    ro, to = B.default_reproject_opts(), B.default_temporal_opts()
    res = {"frame": f"{W}x{H}", "reps": a.reps, "lib": os.path.basename(B.LIB_PATH)}
    P = lambda t: t.data_ptr()  # noqa: E731
    cases = {
        "reproject": (lambda: sc.reproject_dev(ro, fr0, P(pz), P(pn), P(prad), P(plen), P(pa), P(z), P(n), P(al), P(hist), P(ln), P(mo), s.cuda_stream), 96),
        "reproject_var": (lambda: sc.reproject_var_dev(ro, fr0, P(pz), P(pn), P(prad), P(pvar), P(plen), P(pa), P(z), P(n), P(al), P(hist), P(hvar), P(ln), P(mo),
                                                       stream=s.cuda_stream), 120),
        "accumulate": (lambda: sc.temporal_accumulate_dev(to, P(rad), 4.0, P(hist), P(ln), P(out), P(oln), P(rgb), s.cuda_stream), 47),
        "accumulate_var": (lambda: sc.temporal_accumulate_var_dev(to, P(rad), P(var), 4.0, P(hist), P(hvar), P(ln), P(out), P(ovar), P(oln), P(rgb), s.cuda_stream), 83),
    }
    for k, (call, bpp) in cases.items():
        res[k] = dict(timed(call), bytes_per_pixel=bpp)
        res[k]["GBps"] = bpp * px / res[k]["ms_median"] / 1e6
    res["valid_share"] = float((ln > 0).float().mean())
    res["checksum"] = float(out.double().sum()) + float(ovar.double().sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
