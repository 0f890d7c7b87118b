"""Times the denoiser's kernels on the GPU: k_variance on the C3 headline frame (tests/scenes/c3_mesh.xml, 1920x1080, 64 spp) and the
whole filter (k_dn_prepare + K x k_dn_step) on 1920x1080 and 3840x2160 frames, with the guides given, with and without a variance
image.  Wall time per call from HIP events; for kernel times run it under `rocprofv3 --kernel-trace --stats`.  Prints one JSON line
with the algorithmic bytes of each kernel group:
    variance  2 x 12 B per sample (the samples are read twice: mean, then squared deviations) + 12 B per pixel written
    filter    prepare: 12 B radiance + 12 B variance + 4 + 12 + 12 B guides read, 32 B of planes written per pixel;
              step: 32 B read (centre (e, v_L) and (n, z)), 16 B written per pixel; last step: + 12 B albedo, 12 B out + 3 B rgb8 instead
--sampled times the filter for sampled guides as well (bhrt_denoise_sampled_dev: k_dns_prepare + K x k_dns_step) on the same frames
with a band of partial coverage; it reads 4 B of coverage more per pixel in prepare and in every step (the last step 4 B more again)."""
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--no-variance-kernel", action="store_true")
    ap.add_argument("--sampled", action="store_true", help="also time bhrt_denoise_sampled_dev (the filter for sampled guides)")
    a = ap.parse_args()
    import torch
    import bhraytracer_amd as B
    from conftest import ensure_mesh
    if B.device_count() < 1:
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"iterations": a.iterations, "reps": a.reps}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if not a.no_variance_kernel:
        ensure_mesh(224)
        sc = B.Scene(os.path.join(ROOT, "tests/scenes/c3_mesh.xml"))
        sc.upload(0)
        W, H = sc.width, sc.height
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        var = torch.zeros_like(rad)
        o = B.default_opts(spp=64, gi_bounces=3, timers=1)
        st0 = sc.render_var_dev(o, 0, rad.data_ptr(), 0)
        st1 = sc.render_var_dev(o, 0, rad.data_ptr(), var.data_ptr())
        res["variance"] = {"frame": f"{W}x{H} x 64 spp", "render_s": st0.seconds_total, "render_with_variance_s": st1.seconds_total,
                           "passes": st1.passes, "bytes": W * H * 64 * 24 + W * H * 12}
    for W, H in ((1920, 1080), (3840, 2160)):
        xml = os.path.join(ROOT, "tests", "scenes", f"_tmp_denoise_{W}x{H}.xml")
        with open(xml, "w") as f:
            f.write(f"""<xml><scene><object type="sphere" name="s" material="m"/><material type="blinn" name="m"><diffuse value="0.5"/></material>
              <light type="point" name="l"><intensity value="10"/><position z="10"/></light></scene>
              <camera><position z="10"/><target z="0"/><up y="1"/><width value="{W}"/><height value="{H}"/></camera></xml>""")
        try:
            sc = B.Scene(xml)
        finally:
            os.remove(xml)
        sc.upload(0)
        import test_denoise as T
        c, v, z, n, al = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in T.synthetic(W, H))
        out = torch.zeros_like(c)
        rgb = torch.zeros(c.shape, dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev)
        for name, vp in (("with_variance", v.data_ptr()), ("without_variance", 0)):
            o = B.default_denoise_opts(iterations=a.iterations)
            args = (c.data_ptr(), vp, z.data_ptr(), n.data_ptr(), al.data_ptr(), out.data_ptr(), rgb.data_ptr(), s.cuda_stream)
            sc.denoise_dev(o, *args)
            torch.cuda.synchronize()
            ev0.record(s)
            for _ in range(a.reps):
                sc.denoise_dev(o, *args)
            ev1.record(s)
            torch.cuda.synchronize()
            px = W * H
            nbytes = px * (40 + (12 if vp else 0) + 32) + (a.iterations - 1) * px * 48 + px * (32 + 12 + 12 + 3)
            ms = ev0.elapsed_time(ev1) / a.reps
            res[f"denoise_{W}x{H}_{name}"] = {"ms_per_call": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6}
            if not a.sampled:
                continue
            # the filter for sampled guides: a ramp of partial coverage over the middle tenth of the columns, n and albedo scaled by it
            cov = torch.clamp((torch.arange(W, device=dev, dtype=torch.float32) - 0.45 * W) / (0.1 * W), 0, 1).repeat(H, 1).contiguous()
            cov = torch.where(z >= 1e30, torch.zeros_like(cov), cov)
            n_s, al_s = (n * cov[..., None]).contiguous(), (al * cov[..., None]).contiguous()
            z_s = torch.where(cov > 0, z, torch.full_like(z, 1e30))
            args = (c.data_ptr(), vp, z_s.data_ptr(), n_s.data_ptr(), al_s.data_ptr(), cov.data_ptr(), out.data_ptr(), rgb.data_ptr(), s.cuda_stream)
            sc.denoise_sampled_dev(o, B.DENOISE_SIGMA_COVERAGE, *args)
            torch.cuda.synchronize()
            ev0.record(s)
            for _ in range(a.reps):
                sc.denoise_sampled_dev(o, B.DENOISE_SIGMA_COVERAGE, *args)
            ev1.record(s)
            torch.cuda.synchronize()
            nbytes += px * 4 * (a.iterations + 2)
            ms = ev0.elapsed_time(ev1) / a.reps
            res[f"denoise_sampled_{W}x{H}_{name}"] = {"ms_per_call": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
