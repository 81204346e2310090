#!/usr/bin/env python3
"""What the thin lens costs on the benchmark scene: the atrium at 1920x1080 with the pinhole (R = 0) and with an aperture (R > 0), alternating in one process.
Per frame: seconds_render, seconds_trace_closest and node visits per closest-hit ray from ptc_stats — once at max_bounces 0, where every ray is a camera ray
and the loss of primary-ray coherence shows undiluted, and once at the benchmark's 8 bounces, the whole-frame cost (DESIGN.md §6 estimated at most 7.6 %).
The images are checked to differ and to be finite; nothing is gated.
`--one`: one warmed frame of each kind at equal path counts (1080p x SPP in ONE batch, >= 2^21 paths), the run to put behind
`rocprofv3 --kernel-trace --stats --` for the k_raygen and k_raygen_lens rows.
usage: python3 tools/lens_bench.py [--one] [--spp N] [--radius R] [--focus F] [--blades N] [--reps K]   (-> profiles/lens_1080p.txt)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

ap = argparse.ArgumentParser()
ap.add_argument("--one", action="store_true")
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--radius", type=float, default=0.1)
ap.add_argument("--focus", type=float, default=12.0)
ap.add_argument("--blades", type=int, default=0)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
W, H = 1920, 1080
assert W * H * a.spp >= 1 << 21, "at least 2^21 paths per frame"

pt = pbr.PathTracer(0).load_scene(pbr.scenes.atrium())
lenses = {"pinhole": (0.0, a.focus, 0, 0.0), "lens": (a.radius, a.focus, a.blades, 0.0)}


def frame(kind, bounces):
    pt.set_camera_lens(*lenses[kind])
    img = pt.render(W, H, a.spp, seed=1, max_bounces=bounces)
    st = pt.stats()
    rays = st["segments"]      # closest-hit rays traced
    return img, {"seconds_render": st["seconds_render"], "seconds_trace_closest": st["seconds_trace_closest"], "seconds_shade": st["seconds_shade"], "paths": st["paths"],
                 "closest_rays": rays, "node_visits_per_ray": st["node_visits_closest"] / max(rays, 1), "tri_tests_per_ray": st["tri_tests_closest"] / max(rays, 1)}


out = {"scene": "atrium", "size": [W, H], "spp": a.spp, "lens": dict(zip(("aperture_radius", "focus_distance", "blades", "rotation"), lenses["lens"]))}
for kind in lenses:      # warm-up: queues, overflow slabs, clocks
    frame(kind, 8)
if a.one:
    for kind in lenses:
        _, out[kind] = frame(kind, 8)
    print(json.dumps(out))
    sys.exit(0)
for bounces in (0, 8):
    runs = {k: [] for k in lenses}
    imgs = {}
    for _ in range(a.reps):
        for kind in lenses:
            imgs[kind], s = frame(kind, bounces)
            runs[kind].append(s)
    assert np.isfinite(imgs["lens"]).all() and not np.array_equal(imgs["lens"], imgs["pinhole"])
    res = {}
    for kind, rs in runs.items():
        res[kind] = {k: (float(np.median([r[k] for r in rs])) if k.startswith(("seconds", "node", "tri")) else rs[0][k]) for k in rs[0]}
        res[kind]["seconds_render_all"] = [r["seconds_render"] for r in rs]
    res["lens_over_pinhole"] = {k: res["lens"][k] / res["pinhole"][k] for k in ("seconds_render", "seconds_trace_closest", "node_visits_per_ray") if res["pinhole"][k] > 0}
    out[f"max_bounces_{bounces}"] = res
print(json.dumps(out))
