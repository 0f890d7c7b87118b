"""Times the temporal session (bhrt_temporal_*) against the chain of host wrappers it replaces, in one process: tests/scenes/c3_mesh.xml
at 1920x1080, --spp 4, --frames 8 along the move of tools/temporal_timing.py (+1.5, 0, +0.5, the same target), in the mode carry_variance +
spatial_variance + denoise, the displayed frame delivered as rgb8 in host memory on both sides.  Prints one JSON line:
    session, chain   per-frame wall time (a host clock around calls that end in a device synchronise), median / min / max over the frames of
                     --rounds alternating runs (session, chain, session, chain, ...); frame 0 of the first session run allocates and is reported
                     apart; `same_bytes`: the rgb8 of every frame of both sides is identical
    split            one more run of the session's own sequence through the _dev calls on tensors, the first-hit trace and the image stages
                     between HIP events on the call's stream, the render (which synchronises its own stream) by the host clock: medians per frame
    first_hit        bhrt_first_hit_ex_dev with all four images against bhrt_first_hit_dev + bhrt_first_hit_node_dev: medians of --reps calls
                     after 3 warm-ups, each between two HIP events."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

f32 = np.float32


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests/scenes/c3_mesh.xml"))
    a = ap.parse_args()
    import torch
    import bhraytracer_amd as B
    from conftest import ensure_mesh
    from temporal_timing import xml_pose
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda", 0)
    if "gen/mesh_224.obj" in open(a.scene).read():
        ensure_mesh(224)
    sc = B.Scene(a.scene)
    sc.upload(0)
    W, H = sc.width, sc.height
    pos, target, up = xml_pose(a.scene)
    p0 = f32(list(pos))
    p1 = p0 + f32([1.5, 0.0, 0.5])

    def set_frame(k):
        p = (p0 + (p1 - p0) * (f32(k) / f32(max(a.frames - 1, 1)))).astype(f32)
        sc.set_camera(p, target, up)

    opts = lambda k: B.default_opts(spp=a.spp, seed=1 + k)  # noqa: E731
    ro, to, dn = B.default_reproject_opts(), B.default_temporal_opts(), B.default_denoise_opts()
    sv = B.default_spatial_variance_opts(min_length=4.0 * a.spp)
    topts = B.default_temporal_session_opts(carry_variance=1, spatial_variance=1, denoise=1)
    topts.spatial.min_length = 4.0 * a.spp

    def run_session():
        ms, frames = [], []
        sc.temporal_begin(opts(0), topts)
        for k in range(a.frames):
            set_frame(k)
            t0 = time.perf_counter()
            rgb = sc.temporal_frame(want_radiance=False)[0]
            ms.append((time.perf_counter() - t0) * 1e3)
            frames.append(rgb)
        sc.temporal_end()
        return ms, frames

    def run_chain():  # the host wrappers as bhrt render --temporal N --denoise --spatial-variance chained them
        ms, frames, prev = [], [], None
        for k in range(a.frames):
            set_frame(k)
            t0 = time.perf_counter()
            z, n, al = sc.first_hit()
            _, cur, cv = sc.render_var(opts(k))
            if a.spp < 2:
                cv = sc.variance_spatial(sv, cur, None, None, z, n, al)
            h = hv = hl = None
            if prev is not None:
                h, hv, hl = sc.reproject_var(ro, *prev, z, n, al, want=("history", "history_variance", "length"))[:3]
            acc, accv, ln, _ = sc.temporal_accumulate_var(to, cur, cv, float(a.spp), h, hv, hl)
            est = sc.variance_spatial(sv, acc, accv, ln, z, n, al)
            rgb = sc.denoise(dn, acc, est, z, n, al)[1]
            prev = (sc.camera_frame(), z, n, acc, accv, ln, al)
            ms.append((time.perf_counter() - t0) * 1e3)
            frames.append(rgb)
        return ms, frames

    res = {"scene": os.path.basename(a.scene), "frame": f"{W}x{H}", "spp": a.spp, "frames": a.frames, "rounds": a.rounds, "lib": os.path.basename(B.LIB_PATH)}
    run_chain()  # warm-up of both sides: code objects, the render's workspace, the scene's scratch
    first_ms, _ = run_session()
    res["session_first_run_frame0_ms"] = first_ms[0]
    s_ms, c_ms, same = [], [], True
    for _ in range(a.rounds):
        ms, fs = run_session()
        s_ms += ms
        ms, fc = run_chain()
        c_ms += ms
        same = same and all(np.array_equal(x, y) for x, y in zip(fs, fc))
    res["session"], res["chain"], res["same_bytes"] = stats(s_ms), stats(c_ms), bool(same)
    res["chain_over_session"] = res["chain"]["ms_median"] / res["session"]["ms_median"]

    # the session's sequence through the _dev calls, timed by parts
    f3 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device=dev)  # noqa: E731
    f1 = lambda: torch.zeros((H, W), dtype=torch.float32, device=dev)  # noqa: E731
    P = lambda t: t.data_ptr()  # noqa: E731
    views = [dict(z=f1(), n=f3(), a=f3()) for _ in range(2)]
    acc, accv, aln = [f3(), f3()], [f3(), f3()], [f1(), f1()]
    cur, cv, hist, hvar, hln, est = f3(), f3(), f3(), f3(), f1(), f3()
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    part = {"guides": [], "render": [], "image_stages": []}
    frame = None
    for k in range(a.frames):
        set_frame(k)
        c, p = views[k & 1], views[(k & 1) ^ 1]
        o, q = k & 1, (k & 1) ^ 1  # this frame's accumulated images and the previous frame's
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(s)
        sc.first_hit_ex_dev(P(c["z"]), P(c["n"]), P(c["a"]), 0, s.cuda_stream)
        e[1].record(s)
        s.synchronize()
        t0 = time.perf_counter()
        sc.render_var_dev(opts(k), 0, P(cur), P(cv))
        part["render"].append((time.perf_counter() - t0) * 1e3)
        e[2].record(s)
        if k > 0:
            sc.reproject_var_dev(ro, frame, P(p["z"]), P(p["n"]), P(acc[q]), P(accv[q]), P(aln[q]), P(p["a"]), P(c["z"]), P(c["n"]), P(c["a"]), P(hist), P(hvar), P(hln),
                                 stream=s.cuda_stream)
        h = (P(hist), P(hvar), P(hln)) if k > 0 else (0, 0, 0)
        sc.temporal_accumulate_var_dev(to, P(cur), P(cv), float(a.spp), h[0], h[1], h[2], P(acc[o]), P(accv[o]), P(aln[o]), 0, s.cuda_stream)
        sc.variance_spatial_dev(sv, P(acc[o]), P(accv[o]), P(aln[o]), P(c["z"]), P(c["n"]), P(c["a"]), P(est), s.cuda_stream)
        sc.denoise_dev(dn, P(acc[o]), P(est), P(c["z"]), P(c["n"]), P(c["a"]), 0, P(rgb), s.cuda_stream)
        e[3].record(s)
        s.synchronize()
        part["guides"].append(e[0].elapsed_time(e[1]))
        part["image_stages"].append(e[2].elapsed_time(e[3]))
        frame = sc.camera_frame()
    res["split"] = {k: stats(v[1:]) for k, v in part.items()}  # frame 0 has no reprojection
    res["split_last_frame_same_bytes"] = bool(np.array_equal(rgb.cpu().numpy(), fs[-1])) if a.rounds > 0 else None

    # one trace against two
    node = torch.zeros((H, W), dtype=torch.int32, device=dev)
    v = views[0]

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
        return stats(ms)

    def pair():
        sc.first_hit_dev(P(v["z"]), P(v["n"]), P(v["a"]), s.cuda_stream)
        sc.first_hit_node_dev(P(node), s.cuda_stream)

    res["first_hit"] = {"pair": timed(pair), "ex": timed(lambda: sc.first_hit_ex_dev(P(v["z"]), P(v["n"]), P(v["a"]), P(node), s.cuda_stream)),
                        "first_hit_alone": timed(lambda: sc.first_hit_dev(P(v["z"]), P(v["n"]), P(v["a"]), s.cuda_stream))}
    res["first_hit"]["pair_over_ex"] = res["first_hit"]["pair"]["ms_median"] / res["first_hit"]["ex"]["ms_median"]
    print(json.dumps(res))
    sc.close()


if __name__ == "__main__":
    main()
