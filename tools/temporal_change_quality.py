#!/usr/bin/env python3
"""The measurements behind the temporal change test's defaults and its cost.

    python tools/temporal_change_quality.py [--out profiles/temporal_change_quality.json] [--skip-time]

Quality, on tests/scenes/c3_mesh_small.xml (320 x 240), a temporal session with carry_variance + spatial_variance + denoise + follow_nodes, a
static camera, 8 frames, at 1 spp and at 4 spp:
  (a) nothing moves;
  (b) the node "ball" is translated by BALL_MOVE at frame 4 and stays there.
Truth: a 256-spp bhrt_render of the scene state of each frame (two states), seed A; a second render of each state with seed B gives the truth's
own spread.  The changed region: the pixels where |L(T1_A) - L(T0_A)| is above the largest, over the pixel's 3 x 3 block, of
|L(T0_A) - L(T0_B)| + |L(T1_A) - L(T1_B)| (the truth differs before and after the move by more than its own two-seed spread; the block keeps a
pixel whose two seeds agree by chance from counting).  For the stage off and for (sigma_lo, sigma_hi) in PAIRS the tool reports the MSE of the
displayed frame against the frame's truth over the changed region and over the rest for frames 4..7 of (b), the whole-frame MSE of frame 7 of
(a), and the share of pixels with lambda > 0 over frames 1..7 of (a).  The stage-off still figure is measured with two session seeds: their
difference is how far a pair's still figure may lie above the stage-off one.  The chosen pair: among the pairs within that bound at both sample
counts, the lowest changed-region MSE relative to the stage-off one, averaged over the two sample counts.

Time, at 1920 x 1080 on random images over a flat first hit: HIP events around bhrt_temporal_change_dev and around bhrt_variance_spatial_dev at
the same radius, in one process, each the median of 30 calls after 3 warm-ups."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bhraytracer_amd as B  # noqa: E402

XML = os.path.join(ROOT, "tests", "scenes", "c3_mesh_small.xml")
BALL_MOVE = (-1.5, 0.5, 0.75)          # tests/test_temporal_session.py's
PAIRS = [(1.0, 2.0), (1.5, 3.0), (2.0, 4.0), (3.0, 6.0)]
FRAMES, MOVE_AT = 8, 4
TRUTH_SPP, SEED_A, SEED_B = 256, 9001, 9002
f32 = np.float32


def lum(x):
    return (f32(0.2126) * x[..., 0] + f32(0.7152) * x[..., 1]) + f32(0.0722) * x[..., 2]


def block_max(a):
    """The largest value of each pixel's 3 x 3 block (clamped at the border)."""
    p = np.pad(a, 1, mode="edge")
    H, W = a.shape
    return np.max([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)


def set_ball(sc, saved, moved):
    sc.set_node_transform(sc.node_index("ball"), saved["tm"], saved["pos"], [B.translate(*(BALL_MOVE if moved else (0.0, 0.0, 0.0)))])


def truths():
    sc = B.Scene(XML)
    try:
        saved = sc.node_transform(sc.node_index("ball"))
        out = {}
        for moved in (0, 1):
            set_ball(sc, saved, moved)
            for seed in (SEED_A, SEED_B):
                out[moved, seed] = sc.render(B.default_opts(spp=TRUTH_SPP, seed=seed))[1]
        return out
    finally:
        sc.close()


def sequence(spp, seed, moving, pair):
    """The displayed frames of one session, and lambda of each frame (None with the stage off)."""
    sc = B.Scene(XML)
    try:
        saved = sc.node_transform(sc.node_index("ball"))
        sc.temporal_begin(B.default_opts(spp=spp, seed=seed), B.default_temporal_session_opts(carry_variance=1, spatial_variance=1, denoise=1, follow_nodes=1))
        if pair is not None:
            sc.temporal_set_change(B.default_change_opts(sigma_lo=pair[0], sigma_hi=pair[1]))
        shown, lam = [], []
        for k in range(FRAMES):
            set_ball(sc, saved, moving and k >= MOVE_AT)
            shown.append(sc.temporal_frame()[1])
            lam.append(sc.temporal_image(B.TEMPORAL_IMG_CHANGE) if pair is not None else None)
        return shown, lam
    finally:
        sc.close()


def quality():
    T = truths()
    T0, T1 = T[0, SEED_A], T[1, SEED_A]
    spread = np.abs(lum(T0) - lum(T[0, SEED_B])) + np.abs(lum(T1) - lum(T[1, SEED_B]))
    changed = np.abs(lum(T1) - lum(T0)) > block_max(spread)
    mse = lambda x, t, m=None: float(np.mean(((x - t) ** 2)[m] if m is not None else (x - t) ** 2))  # noqa: E731
    res = {"changed_pixels": int(changed.sum()), "pixels": int(changed.size), "by_spp": {}}
    for spp in (1, 4):
        rows = []
        still_off = [mse(sequence(spp, seed, False, None)[0][FRAMES - 1], T0) for seed in (100, 200)]
        tol = abs(still_off[0] - still_off[1])
        for pair in [None] + PAIRS:
            moved, _ = sequence(spp, 100, True, pair)
            still, lam = (None, None) if pair is None else sequence(spp, 100, False, pair)
            rows.append({"pair": pair,
                         "changed_mse": [mse(moved[k], T1, changed) for k in range(MOVE_AT, FRAMES)],
                         "rest_mse": [mse(moved[k], T1, ~changed) for k in range(MOVE_AT, FRAMES)],
                         "still_mse": still_off[0] if pair is None else mse(still[FRAMES - 1], T0),
                         "still_share": 0.0 if pair is None else float(np.mean([(lam[k] > 0).mean() for k in range(1, FRAMES)]))})
            print(spp, rows[-1], flush=True)
        res["by_spp"][str(spp)] = {"still_off_two_seeds": still_off, "still_tolerance": tol, "rows": rows}
    # the choice
    score = {}
    for i, pair in enumerate(PAIRS):
        ok, rel = True, []
        for spp in ("1", "4"):
            S = res["by_spp"][spp]
            off, row = S["rows"][0], S["rows"][i + 1]
            ok = ok and row["still_mse"] <= off["still_mse"] + S["still_tolerance"]
            rel.append(float(np.mean(row["changed_mse"])) / float(np.mean(off["changed_mse"])))
        score[str(pair)] = {"within_still_bound": bool(ok), "changed_mse_relative_to_off": rel, "mean": float(np.mean(rel))}
    res["score"] = score
    elig = [p for p in PAIRS if score[str(p)]["within_still_bound"]]
    best = min(elig, key=lambda p: score[str(p)]["mean"]) if elig else None
    res["chosen"] = best if best is not None and score[str(best)]["mean"] < 1.0 else None
    return res


def timing(radius=3, W=1920, H=1080, calls=30, warm=3):
    import torch
    d = tempfile.mkdtemp()
    xml = os.path.join(d, "frame.xml")
    with open(xml, "w") as f:
        f.write(f"""<xml><scene><object type="sphere" name="s" material="m"/><material type="blinn" name="m"><diffuse value="0.5"/></material>
          <light type="point" name="l"><intensity value="10"/><position z="10"/></light></scene>
          <camera><position z="10"/><target z="0"/><up y="1"/><width value="{W}"/><height value="{H}"/></camera></xml>""")
    sc = B.Scene(xml)
    try:
        sc.upload(0)
        dev = torch.device("cuda", 0)
        g = torch.Generator(device=dev).manual_seed(1)
        c = torch.rand((H, W, 3), device=dev, generator=g)
        h = c + 0.05 * torch.randn((H, W, 3), device=dev, generator=g)
        v = 0.002 * torch.rand((H, W, 3), device=dev, generator=g)
        hv = 0.001 * torch.rand((H, W, 3), device=dev, generator=g)
        l = torch.randint(0, 17, (H, W), device=dev, generator=g).float()
        z = torch.full((H, W), 3.0, device=dev)
        n = torch.zeros((H, W, 3), device=dev)
        n[..., 2] = 1
        a = torch.full((H, W, 3), 0.5, device=dev)
        out_l, out_c, out_v = torch.empty((H, W), device=dev), torch.empty((H, W), device=dev), torch.empty((H, W, 3), device=dev)
        s = torch.cuda.Stream(dev)
        co, so = B.default_change_opts(radius=radius), B.default_spatial_variance_opts(radius=radius)
        P = lambda t: t.data_ptr()  # noqa: E731
        calls_by_name = {
            "temporal_change": lambda: sc.temporal_change_dev(co, P(c), P(v), P(h), P(hv), P(l), P(z), P(n), P(out_l), P(out_c), stream=s.cuda_stream),
            "variance_spatial": lambda: sc.variance_spatial_dev(so, P(c), P(v), P(l), P(z), P(n), P(a), P(out_v), stream=s.cuda_stream),
        }
        res = {"width": W, "height": H, "radius": radius, "calls": calls, "warm_ups": warm}
        torch.cuda.synchronize()
        for name, call in calls_by_name.items():
            ms = []
            for k in range(warm + calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                call()
                e1.record(s)
                s.synchronize()
                if k >= warm:
                    ms.append(e0.elapsed_time(e1))
            res[name + "_ms"] = {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}
        return res
    finally:
        sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_change_quality.json"))
    ap.add_argument("--skip-time", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    res = {}
    if not args.skip_time:
        res["time"] = {str(R): timing(R) for R in (1, 2, 3, 4)}
        print(json.dumps(res["time"]), flush=True)
    if not args.skip_quality:
        res["quality"] = quality()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
