#!/usr/bin/env python3
"""The measurements behind guided upsampling: what it buys at equal sample count, and what the stage costs.

    python tools/upsample_quality.py [--out profiles/upsample_quality.json] [--skip-time] [--skip-quality]

Quality at equal sample count, on tests/scenes/c3_mesh_small.xml, c3_room_small.xml and c2_glass_small.xml: the full-size frame at 4 spp, the
half-size frame at 16 spp upsampled with s = 2, and the quarter-size frame at 64 spp upsampled with s = 4 (bhrt_scene_clone +
bhrt_scene_set_resolution, bhrt_render_var, both bhrt_first_hit images, bhrt_upsample with the defaults), each also through bhrt_denoise with
its variance (bhrt_render_var's, bhrt_upsample's out_variance) and the full-size first hit.  For the upsampled frames the plain bilinear frame
(every surface test passing, demodulate = 0) is reported beside the guided one, and the guided one with bhrt_upsample_opts.fallback =
BHRT_UPSAMPLE_FALLBACK_LIGHT ("light") beside the default rule's, also over the pixels with confidence 0 alone ("lost").  MSE of the linear radiance against the 256-spp full-size frame
(another seed), over the whole frame and over the edge pixels: those whose 3 x 3 block holds more than one first-hit node.  A second 256-spp
frame gives the truth's own MSE.  The guided and the plain frame are also compared over the pixels with confidence > 0 alone: what is left is
the error of the pixels that fell back to taps off their surface.

Time, at 1920 x 1080 from 960 x 540 (s = 2) and from 480 x 270 (s = 4), on random images over a flat first hit: HIP events around
bhrt_upsample_dev (all four outputs, demodulate on, guides passed in) and around bhrt_variance_spatial_dev at R = 1 in the same process, each
the median of 30 calls after 3 warm-ups.  Every bhrt_upsample_dev row is taken with fallback = albedo and with fallback = light, one after the other,
and the whole list is gone through three times: the rounds' medians are kept beside the median of all 90 calls, so that the two rules are
compared inside their own spread.  A flat first hit has no pixel without a passing tap; the `lost1` rows repeat s = 2 with 1 % of the full
pixels moved to a depth none of their taps has, which is the share the scenes above show."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bhraytracer_amd as B  # noqa: E402

SCENES = ("c3_mesh_small", "c3_room_small", "c2_glass_small")
BUDGET = ((1, 4), (2, 16), (4, 64))     # (factor, spp): 4 samples per full pixel each
TRUTH_SPP, SEED, SEED_A, SEED_B = 256, 11, 9001, 9002
f32 = np.float32


def edge_pixels(node):
    """Pixels whose 3 x 3 block holds more than one first-hit node."""
    H, W = node.shape
    pad = np.pad(node, 1, mode="edge")
    return np.any([pad[dy:dy + H, dx:dx + W] != node for dy in range(3) for dx in range(3)], axis=0)


def quality_of(name):
    full = B.Scene(os.path.join(ROOT, "tests", "scenes", name + ".xml"))
    try:
        W, H = full.width, full.height
        truth = full.render(B.default_opts(spp=TRUTH_SPP, seed=SEED_A))[1]
        truth_b = full.render(B.default_opts(spp=TRUTH_SPP, seed=SEED_B))[1]
        edges = edge_pixels(full.first_hit_node())
        z, n, a = full.first_hit()
        dn = B.default_denoise_opts()

        def mse(x, mask=None):
            d = (x.astype(np.float64) - truth) ** 2
            if mask is not None:
                return {"frame": float(d[mask].mean()), "edges": float(d[mask & edges].mean())}
            return {"frame": float(d.mean()), "edges": float(d[edges].mean())}
        res = {"width": W, "height": H, "edge_pixels": int(edges.sum()), "truth_second_seed": mse(truth_b), "rows": []}
        for s, spp in BUDGET:
            o = B.default_opts(spp=spp, seed=SEED)
            row = {"factor": s, "spp": spp}
            if s == 1:
                _, rad, var = full.render_var(o)
                row["frame"] = mse(rad)
                row["denoised"] = mse(full.denoise(dn, rad, var, z, n, a)[0])
            else:
                low = full.clone()
                try:
                    low.set_resolution(W // s, H // s)
                    _, c, v = low.render_var(o)
                    zl, nl, al = low.first_hit()
                finally:
                    low.close()
                up = full.upsample(B.default_upsample_opts(), c, zl, nl, al, v, z, n, a, want=("out", "variance", "confidence"))
                plain = full.upsample(B.default_upsample_opts(depth_tolerance=3e38, normal_threshold=-float("inf"), demodulate=0), c, np.ones_like(zl), nl, None, v,
                                      np.ones((H, W), f32), n, None, want=("out", "variance"))
                row["frame"] = mse(up["out"])
                row["denoised"] = mse(full.denoise(dn, up["out"], up["variance"], z, n, a)[0])
                lit = full.upsample(B.default_upsample_opts(fallback=B.UPSAMPLE_FALLBACK_LIGHT), c, zl, nl, al, v, z, n, a, want=("out", "variance", "confidence"))
                assert lit["confidence"].tobytes() == up["confidence"].tobytes()
                row["light"] = mse(lit["out"])
                row["light_denoised"] = mse(full.denoise(dn, lit["out"], lit["variance"], z, n, a)[0])
                row["plain_bilinear"] = mse(plain["out"])
                row["plain_bilinear_denoised"] = mse(full.denoise(dn, plain["out"], plain["variance"], z, n, a)[0])
                sure = up["confidence"] > 0                                    # the pixels with a tap on their own surface
                row["confidence_zero_share"] = float((~sure).mean())
                if (~sure).any():
                    row["frame_where_lost"], row["light_where_lost"], row["plain_bilinear_where_lost"] = mse(up["out"], ~sure), mse(lit["out"], ~sure), mse(plain["out"], ~sure)
                row["frame_where_confident"], row["plain_bilinear_where_confident"] = mse(up["out"], sure), mse(plain["out"], sure)
            print(name, row, flush=True)
            res["rows"].append(row)
        return res
    finally:
        full.close()


def timing(W=1920, H=1080, calls=30, warm=3, rounds=3):
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
        P = lambda t: t.data_ptr()  # noqa: E731

        def guides(h, w):
            n = torch.zeros((h, w, 3), device=dev)
            n[..., 2] = 1
            return torch.full((h, w), 3.0, device=dev), n, 0.1 + 0.8 * torch.rand((h, w, 3), device=dev, generator=g)
        z, n, a = guides(H, W)
        c_full, v_full = torch.rand((H, W, 3), device=dev, generator=g), 0.002 * torch.rand((H, W, 3), device=dev, generator=g)
        out, out_v, conf = torch.empty((H, W, 3), device=dev), torch.empty((H, W, 3), device=dev), torch.empty((H, W), device=dev)
        rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(dev)
        so = B.default_spatial_variance_opts(radius=1)
        rules = (("", B.default_upsample_opts()), ("_light", B.default_upsample_opts(fallback=B.UPSAMPLE_FALLBACK_LIGHT)))
        z_lost = torch.where(torch.rand((H, W), device=dev, generator=g) < 0.01, torch.full_like(z, 50.0), z)      # 1 % of the pixels: no tap passes
        calls_by_name = {"variance_spatial_r1": lambda: sc.variance_spatial_dev(so, P(c_full), P(v_full), 0, P(z), P(n), P(a), P(out_v), stream=s.cuda_stream)}
        keep = []
        for f in (2, 4):
            w, h = W // f, H // f
            zl, nl, al = guides(h, w)
            c, v = torch.rand((h, w, 3), device=dev, generator=g), 0.002 * torch.rand((h, w, 3), device=dev, generator=g)
            keep.append((zl, nl, al, c, v))
            for tag, uo in rules:
                calls_by_name["upsample_s%d%s" % (f, tag)] = (lambda uo=uo, w=w, h=h, c=c, v=v, zl=zl, nl=nl, al=al: sc.upsample_dev(
                    uo, w, h, P(c), P(v), P(zl), P(nl), P(al), P(z), P(n), P(a), P(out), P(out_v), P(conf), P(rgb), stream=s.cuda_stream))
            for tag, uo in rules:
                calls_by_name["upsample_s%d_out_only%s" % (f, tag)] = (lambda uo=uo, w=w, h=h, c=c, zl=zl, nl=nl, al=al: sc.upsample_dev(
                    uo, w, h, P(c), 0, P(zl), P(nl), P(al), P(z), P(n), P(a), P(out), stream=s.cuda_stream))
            if f == 2:
                for tag, uo in rules:
                    calls_by_name["upsample_s2_lost1%s" % tag] = (lambda uo=uo, w=w, h=h, c=c, v=v, zl=zl, nl=nl, al=al: sc.upsample_dev(
                        uo, w, h, P(c), P(v), P(zl), P(nl), P(al), P(z_lost), P(n), P(a), P(out), P(out_v), P(conf), P(rgb), stream=s.cuda_stream))
        res = {"width": W, "height": H, "calls": calls, "warm_ups": warm, "rounds": rounds}
        torch.cuda.synchronize()
        ms = {name: [] for name in calls_by_name}
        for _ in range(rounds):
            for name, call in calls_by_name.items():
                ms[name].append([])
                for k in range(warm + calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    call()
                    e1.record(s)
                    s.synchronize()
                    if k >= warm:
                        ms[name][-1].append(e0.elapsed_time(e1))
        for name, per_round in ms.items():
            every = np.concatenate(per_round)
            res[name + "_ms"] = {"median": float(np.median(every)), "min": float(np.min(every)), "max": float(np.max(every)),
                                 "round_medians": [float(np.median(r)) for r in per_round]}
        return res
    finally:
        sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_quality.json"))
    ap.add_argument("--skip-time", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    res = {}
    if not args.skip_time:
        res["time"] = timing()
        print(json.dumps(res["time"]), flush=True)
    if not args.skip_quality:
        res["quality"] = {name: quality_of(name) for name in SCENES}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
