"""Times what moving objects add on the GPU, with the method of tools/temporal_timing.py: tests/scenes/c3_mesh.xml at 1920x1080,
a static camera, every figure the median of --reps calls after 3 warm-up calls, each call between two HIP events on the call's stream.
    reproject                k_reproject, guides given, no albedo: the existing kernel, for comparison from the same run
    reproject_moving_static  the bhrt_reproject_moving_dev call, guides and ids given, nothing moved: the copy of the node records (88 B per node,
                             pinned memory, on the stream) and k_reproject_moving, both between the two events; not the kernel alone
    reproject_moving_mesh    the same with the mesh node translated: every pixel of the mesh walks its chain
    first_hit, first_hit_node   k_first_hit (z, normal, albedo) and k_first_hit_node (the id image)
    set_node_transform_ms    one bhrt_scene_set_node_transform on the uploaded scene, host wall clock (median), beside reload_upload_ms: loading
                             the XML again and uploading it
Prints one JSON line.  BHRT_LIB selects another build of the library."""
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
    f3 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device=dev)  # noqa: E731
    f1 = lambda: torch.zeros((H, W), dtype=torch.float32, device=dev)  # noqa: E731
    i1 = lambda: torch.zeros((H, W), dtype=torch.int32, device=dev)  # noqa: E731
    P = lambda t: t.data_ptr()  # noqa: E731
    pz, pn, pa, prad, pid = f1(), f3(), f3(), f3(), i1()
    fr0, xf0 = sc.camera_frame(), sc.node_transforms()
    sc.first_hit_dev(P(pz), P(pn), P(pa))
    sc.first_hit_node_dev(P(pid))
    sc.render_dev(B.default_opts(spp=4, seed=1), 0, P(prad))
    plen = torch.full((H, W), 4.0, dtype=torch.float32, device=dev)
    z, n, al, ids = f1(), f3(), f3(), i1()
    hist, ln = f3(), f1()
    mo = torch.zeros((H, W, 2), dtype=torch.float32, device=dev)
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

    ro = B.default_reproject_opts()
    res = {"frame": f"{W}x{H}", "reps": a.reps, "lib": os.path.basename(B.LIB_PATH), "n_nodes": int(sc.info.n_nodes)}
    mesh = next(k for k, nd in enumerate(sc.flat_view().nodes) if nd.obj_type == 3)

    def current_view():
        sc.first_hit_dev(P(z), P(n), P(al))
        sc.first_hit_node_dev(P(ids))
        torch.cuda.synchronize()

    plain = lambda: sc.reproject_dev(ro, fr0, P(pz), P(pn), P(prad), P(plen), 0, P(z), P(n), 0, P(hist), P(ln), P(mo), s.cuda_stream)  # noqa: E731
    moving = lambda: sc.reproject_moving_dev(ro, fr0, xf0, P(pz), P(pn), P(prad), P(plen), 0, P(pid), P(z), P(n), 0, P(ids), P(hist), P(ln), P(mo),  # noqa: E731
                                             s.cuda_stream)
    current_view()
    res["first_hit"] = timed(lambda: sc.first_hit_dev(P(z), P(n), P(al), s.cuda_stream))
    res["first_hit_node"] = timed(lambda: sc.first_hit_node_dev(P(ids), s.cuda_stream))
    res["reproject"] = timed(plain)
    res["reproject_moving_static"] = timed(moving)
    res["valid_share_static"] = float((ln > 0).float().mean())
    saved = sc.node_transform(mesh)
    host = []
    for k in range(a.reps):                                   # the setter on the uploaded scene: alternately moved and restored
        ops = [B.translate(0.5, 0.25, 0.25)] if k % 2 == 0 else []
        t0 = time.perf_counter()
        sc.set_node_transform(mesh, saved["tm"], saved["pos"], ops)
        host.append((time.perf_counter() - t0) * 1e3)
    res["set_node_transform_ms"] = {"ms_median": statistics.median(host), "ms_min": min(host), "ms_max": max(host)}
    sc.set_node_transform(mesh, saved["tm"], saved["pos"], [B.translate(0.5, 0.25, 0.25)])
    current_view()
    res["reproject_moving_mesh"] = timed(moving)
    res["valid_share_mesh"] = float((ln > 0).float().mean())
    res["mesh_pixel_share"] = float((ids == mesh).float().mean())
    res["reproject_camera_only_valid_share_mesh"] = None
    plain()
    s.synchronize()
    res["reproject_camera_only_valid_share_mesh"] = float((ln > 0).float().mean())
    t0 = time.perf_counter()
    fresh = B.Scene(path)
    fresh.upload(0)
    res["reload_upload_ms"] = (time.perf_counter() - t0) * 1e3
    fresh.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
