#!/usr/bin/env python3
"""Where the samples per pixel of tests/test_gpu_emissive_tex.py's equivalence tests come from (EQ_SPP, EQ_SE_MEASURED): the oracle's render, on the CPU, of the
plain-emitter side of the comparison — the white half of the quad as an emissive quad over the Lambert and the roughness-0.05 metal floor — with the test's own
sizes and seeds (16 seeds, 48 x 32, max_bounces 3).  Per floor and spp: the standard error of the whole-image mean and of the four quadrant means over the seeds,
relative to the mean.  The comparison needs every one under 1 %; the test's spp is the smallest listed that leaves a factor of four.  Needs no GPU; a few seconds.
usage: python3 tools/emissive_tex_spp.py [--spp 32 64 128]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pbr_amd as pbr
from oracle import ora
import test_gpu_emissive_tex as T

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, nargs="+", default=[32, 64, 128])
a = ap.parse_args()
ora.build()
out = {}
for kind in ("lambert", "metal"):
    for spp in a.spp:
        o = ora.Oracle().load_scene(T.plain_scene(pbr, kind))
        mean, se = T.seed_means(o.render, spp)
        o.close()
        out[f"{kind}_{spp}"] = {"relative_se": [float(x) for x in se / mean], "max": float((se / mean).max())}
print(json.dumps(out))
