#!/usr/bin/env python3
"""Records tests/golden/intersect_edges.npz: what the UNMODIFIED reference (oracle/_ref/ref_harness, built by `make -C oracle ref`)
answers for the ray families of tests/test_intersect_edges.py on tests/scenes/intersect_edges.xml.  The rays themselves are not
stored: this script imports the test module's `families()`, which rebuilds them from the scene.

Per closest-hit family and hit side (1 front, 2 back, 3 both), through the harness command `rays`:
  <family>_node_<side>   int16   node index of the hit, -1 = none
  <family>_front_<side>  int8    HitInfo::front
  <family>_zbits_<side>  uint32  the bits of HitInfo::z
  <family>_pN_sha_<side>         SHA-256 of HitInfo::p and N over the hit rays (the form of <scene>_primary_pN_sha in make_golden.py)
Per shadow family, through `shadow`:
  <family>_vis           int8    GenLight::Shadow

Runs where a checkout of the reference exists:  python tests/golden/make_intersect_edges.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SCENES = os.path.join(ROOT, "tests", "scenes")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(pre, *args):
    subprocess.run([HARNESS, "intersect_edges.xml", pre, *map(str, args)], cwd=SCENES, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    import bhraytracer_amd as B
    import oracle_lib as O
    import test_intersect_edges as T
    sc = B.Scene(os.path.join(SCENES, "intersect_edges.xml"))
    F = T.families(sc, O)
    out = {}
    with tempfile.TemporaryDirectory(prefix="bhrt_edges_") as tmp:
        pre = os.path.join(tmp, "e")
        for k in T.closest_names(F):
            n = len(F[k]["o"])
            for side in T.SIDES:
                np.concatenate([F[k]["o"], F[k]["d"], np.full((n, 1), side, np.float32)], 1).astype(np.float32).tofile(pre + ".in")
                run(pre, "--rays", pre + ".in", "rays")
                ri = np.fromfile(pre + ".rays_i32", np.int32).reshape(n, 2)
                rf = np.fromfile(pre + ".rays_f32", np.float32).reshape(n, 16)
                out[f"{k}_node_{side}"] = ri[:, 0].astype(np.int16)
                out[f"{k}_front_{side}"] = ri[:, 1].astype(np.int8)
                out[f"{k}_zbits_{side}"] = rf[:, 0].copy().view(np.uint32)
                out[f"{k}_pN_sha_{side}"] = T.sha(rf[ri[:, 0] >= 0][:, 1:7])
            print(f"{k}: {n} rays, hits per side {[int((out[f'{k}_node_{s}'] >= 0).sum()) for s in T.SIDES]}")
        for k in T.shadow_names(F):
            n = len(F[k]["o"])
            np.concatenate([F[k]["o"], F[k]["d"], F[k]["tmax"][:, None]], 1).astype(np.float32).tofile(pre + ".in")
            run(pre, "--shadow", pre + ".in", "shadow")
            out[f"{k}_vis"] = np.fromfile(pre + ".shadow_f32", np.float32).astype(np.int8)
            assert len(out[f"{k}_vis"]) == n
            print(f"{k}: {n} rays, {int((out[f'{k}_vis'] == 0).sum())} blocked")
    path = os.path.join(HERE, "intersect_edges.npz")
    np.savez_compressed(path, **out)
    print(f"intersect_edges.npz: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
