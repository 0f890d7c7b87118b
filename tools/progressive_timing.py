"""Times a progressive session (bhrt_progressive_*) against the blocking render on the GPU: the C3 headline frame
(tests/scenes/c3_mesh.xml, 1920x1080, 64 spp) and the closed room (tests/scenes/c3_room.xml), each three ways —
    blocking   bhrt_render_var_dev, one call (BHRT_BLOCKING_LIB=path: of another build of the same ABI, e.g. the parent commit's)
    8x8        a session in eight steps of 8, then one frame
    64x1       a session in 64 steps of 1, then one frame
— and bhrt_progressive_frame_dev alone on 1920x1080 and 3840x2160 frames.  Wall time per frame from the host clock around calls that end
in a stream synchronise; frame_dev from HIP events.  For kernel times run it under `rocprofv3 --kernel-trace --stats`.

Without --case the tool is a driver: every measurement is a child process of its own, under its own `timeout -k 10`, in a chain that
stops at the first one that fails (a fault, an abort or a time limit ends the run: nothing more is started on the device).  Prints one
JSON line with the algorithmic bytes of the two session kernels:
    fold    per pixel and step: 12 B per sample of the step read, 36 B of state read (none in the first step), 40 B written, 4 B per survivor listed
    frame   per pixel: 40 B read, 12 + 3 + 12 + 4 B written"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES = {"c3": "c3_mesh.xml", "c3room": "c3_room.xml"}
SPP = 64
# name -> seconds its child may take
CASES = {"c3:blocking": 240, "c3:8x8": 240, "c3:64x1": 300, "c3room:blocking": 240, "c3room:8x8": 240, "c3room:64x1": 300, "frame:1920x1080": 120, "frame:3840x2160": 120}


def fold_bytes(px, steps, n):
    return sum(px * (12 * n + (36 if k else 0) + 40) for k in range(steps))


def render_case(B, scene, how, reps):
    import torch
    from conftest import ensure_mesh
    ensure_mesh(224)
    sc = B.Scene(os.path.join(ROOT, "tests", "scenes", SCENES[scene]))
    sc.upload(0)
    W, H = sc.width, sc.height
    dev = torch.device("cuda", 0)
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    rad, var = (torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
    o = B.default_opts(spp=SPP, gi_bounces=3)
    res = {"frame": f"{W}x{H} x {SPP} spp", "reps": reps}
    if how == "blocking":
        def once():
            st = sc.render_var_dev(o, rgb.data_ptr(), rad.data_ptr(), var.data_ptr())
            return st.passes
    else:
        steps, n = (int(x) for x in how.split("x"))
        res["fold_bytes"] = fold_bytes(W * H, steps, n)

        def once():
            passes = 0
            sc.progressive_begin(o)
            for _ in range(steps):
                st = sc.progressive_step(n)
                passes += st.passes
            sc.progressive_frame_dev(rgb.data_ptr(), rad.data_ptr(), var.data_ptr(), 0)
            assert sc.progressive_status().finished == 1
            sc.progressive_end()
            return passes
    once()  # warm-up: code objects, the workspace, learned pass sizes
    secs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        passes = once()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    res.update(seconds=secs, seconds_min=min(secs), seconds_median=sorted(secs)[len(secs) // 2], passes=passes)
    return res


def frame_case(B, size, reps):
    import torch
    W, H = (int(x) for x in size.split("x"))
    with tempfile.TemporaryDirectory() as tmp:  # the scene refers to no file beside it: nothing is written into the tree
        xml = os.path.join(tmp, f"progressive_{W}x{H}.xml")
        with open(xml, "w") as f:
            f.write(f"""<xml><scene><object type="sphere" name="s" material="m"/><material type="blinn" name="m"><diffuse value="0.5"/></material>
              <light type="point" name="l"><intensity value="10"/><position z="10"/></light></scene>
              <camera><position z="10"/><target z="0"/><up y="1"/><width value="{W}"/><height value="{H}"/></camera></xml>""")
        sc = B.Scene(xml)
    sc.upload(0)
    dev = torch.device("cuda", 0)
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    rad, var = (torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
    cnt = torch.zeros((H, W), dtype=torch.int32, device=dev)
    sc.progressive_begin(B.default_opts(spp=4, gi_bounces=0))
    sc.progressive_step(2)
    s = torch.cuda.current_stream(dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    args = (rgb.data_ptr(), rad.data_ptr(), var.data_ptr(), cnt.data_ptr(), s.cuda_stream)
    sc.progressive_frame_dev(*args)
    torch.cuda.synchronize()
    ev0.record(s)
    for _ in range(reps):
        sc.progressive_frame_dev(*args)
    ev1.record(s)
    torch.cuda.synchronize()
    sc.progressive_end()
    ms = ev0.elapsed_time(ev1) / reps
    nbytes = W * H * (40 + 31)
    return {"ms_per_call": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frame-reps", type=int, default=50)
    ap.add_argument("--case", default=None, help="one measurement, in this process: " + ", ".join(CASES))
    ap.add_argument("--only", default=None, help="driver: comma-separated cases instead of all")
    a = ap.parse_args()
    if a.case is None:  # the driver: touches no device itself
        res = {}
        for case in (a.only.split(",") if a.only else CASES):
            env = dict(os.environ)
            if case.endswith(":blocking") and env.get("BHRT_BLOCKING_LIB"):
                env["BHRT_LIB"] = env["BHRT_BLOCKING_LIB"]
            cmd = ["timeout", "-k", "10", str(CASES[case]), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps), "--frame-reps", str(a.frame_reps)]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(json.dumps(res))
                raise SystemExit(f"{case}: exit status {r.returncode}; nothing more is started")
            res[case] = json.loads(r.stdout.strip().splitlines()[-1])
            if env.get("BHRT_LIB"):
                res[case]["lib"] = env["BHRT_LIB"]
        print(json.dumps(res))
        return
    import bhraytracer_amd as B
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    kind, what = a.case.split(":")
    print(json.dumps(frame_case(B, what, a.frame_reps) if kind == "frame" else render_case(B, kind, what, a.reps)))


if __name__ == "__main__":
    main()
