"""Times the two stages of temporal reprojection (csrc/temporal.hip) on the GPU: tests/scenes/c3_mesh.xml at 1920x1080, the
previous view the scene's camera, the current one moved by (+1.5, 0, +0.5) with the same target.  Every figure is the median of --reps calls
after a warm-up, each call between two HIP events on the call's stream.  Prints one JSON line with the algorithmic bytes per pixel:
    reproject   current view z 4 + normal 12 (+ albedo 12) read; per valid pixel up to four taps of z' 4 + normal' 12 + radiance' 12 + length' 4
                (+ albedo' 12), neighbours share them: counted once per pixel; history 12 + length 4 + motion 8 written
    accumulate  radiance 12 + history 12 + length 4 read (the 3 x 3 block's re-reads hit the cache), out 12 + length 4 + rgb8 3 written
BHRT_LIB selects another build of the library (python -m bhraytracer_amd.build --variant NAME -D...), for A/B runs of a kernel change."""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def xml_pose(path):
    cam = open(path).read().split("<camera>")[1]
    out = []
    for tag in ("position", "target", "up"):
        m = re.search(r"<%s ([^>]*)/>" % tag, cam).group(1)
        out.append(tuple(float((re.search(r'%s="([^"]*)"' % k, m) or [0, 0])[1]) for k in "xyz"))
    return out


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
    path = os.path.join(ROOT, "tests/scenes/c3_mesh.xml")
    sc = B.Scene(path)
    sc.upload(0)
    W, H = sc.width, sc.height
    px = W * H
    pos, target, up = xml_pose(path)
    f3 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device=dev)  # noqa: E731
    f1 = lambda: torch.zeros((H, W), dtype=torch.float32, device=dev)  # noqa: E731
    pz, pn, pa, prad = f1(), f3(), f3(), f3()
    fr0 = sc.camera_frame()
    sc.first_hit_dev(pz.data_ptr(), pn.data_ptr(), pa.data_ptr())
    sc.render_dev(B.default_opts(spp=4, seed=1), 0, prad.data_ptr())
    plen = torch.full((H, W), 4.0, dtype=torch.float32, device=dev)
    sc.set_camera((pos[0] + 1.5, pos[1], pos[2] + 0.5), target, up)
    z, n, al, rad = f1(), f3(), f3(), f3()
    sc.first_hit_dev(z.data_ptr(), n.data_ptr(), al.data_ptr())
    sc.render_dev(B.default_opts(spp=4, seed=2), 0, rad.data_ptr())
    hist, ln, out, oln = f3(), f1(), f3(), f1()
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
        "first_hit": (lambda: sc.first_hit_dev(P(z), P(n), P(al), s.cuda_stream), 28),
        "reproject_guides_given": (lambda: sc.reproject_dev(ro, fr0, P(pz), P(pn), P(prad), P(plen), 0, P(z), P(n), 0, P(hist), P(ln), P(mo), s.cuda_stream), 16 + 32 + 24),
        "reproject_guides_given_albedo": (lambda: sc.reproject_dev(ro, fr0, P(pz), P(pn), P(prad), P(plen), P(pa), P(z), P(n), P(al), P(hist), P(ln), P(mo), s.cuda_stream),
                                          28 + 44 + 24),
        "reproject_guides_computed_albedo": (lambda: sc.reproject_dev(ro, fr0, P(pz), P(pn), P(prad), P(plen), P(pa), 0, 0, 0, P(hist), P(ln), P(mo), s.cuda_stream),
                                             28 + 28 + 44 + 24),
    }
    for k, (call, bpp) in cases.items():
        res[k] = dict(timed(call), bytes_per_pixel=bpp)
    res["valid_share"] = float((ln > 0).float().mean())
    for name, ck in (("accumulate_clamp_off", -1.0), ("accumulate_clamp_3", 3.0)):
        o = B.default_temporal_opts(clamp_k=ck, max_length=to.max_length)
        res[name] = dict(timed(lambda: sc.temporal_accumulate_dev(o, P(rad), 4.0, P(hist), P(ln), P(out), P(oln), P(rgb), s.cuda_stream)), bytes_per_pixel=28 + 19)
    for k, v in res.items():
        if isinstance(v, dict):
            v["GBps"] = v["bytes_per_pixel"] * px / v["ms_median"] / 1e6
    res["checksum"] = float(out.double().sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
