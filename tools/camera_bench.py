#!/usr/bin/env python3
"""What the camera models cost on the benchmark scene: the atrium at 1920x1080 x SPP under each projection of ptc_set_camera_ex, and under the
look-at camera of ptc_set_camera, alternating in one process.  Per frame: seconds_render, seconds_trace_closest, seconds_shade and node visits per closest-hit
ray from ptc_stats; the median of --reps frames and every frame's seconds_render (the run-to-run spread is the margin a comparison has to clear).  The
extended perspective camera stands where the look-at camera stands, so those two frames trace the same scene content (mirrored left to right); the orthographic
and the panoramic frame see other parts of the atrium and are not comparable ray for ray: their rows say what such a frame costs, not what the projection adds.
The images are checked to be finite and to differ; nothing is gated.
`--one`: one warmed frame of each kind at equal path counts in ONE batch, the run to put behind `rocprofv3 --kernel-trace --stats --` for the k_raygen and
k_raygen_proj rows (both write 64 B per path).
usage: python3 tools/camera_bench.py [--one] [--spp N] [--reps K]   (-> profiles/camera_1080p.txt)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

ap = argparse.ArgumentParser()
ap.add_argument("--one", action="store_true")
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
W, H = 1920, 1080

desc = pbr.scenes.atrium()
cam = desc.camera
pt = pbr.PathTracer(0).load_scene(desc)
look = pbr.ptc.look_at_matrix(cam.position, cam.target)
KINDS = {
    "look_at": lambda: pt.set_camera(cam.position, cam.target, cam.fov_y, W / H),
    "perspective_ex": lambda: pt.set_camera_ex(look, "perspective", yfov=cam.fov_y, aspect=W / H),
    "orthographic": lambda: pt.set_camera_ex(look, "orthographic", xmag=8.0 * W / H, ymag=8.0),
    "equirect": lambda: pt.set_camera_ex(look, "equirect"),
}


def frame(kind):
    KINDS[kind]()
    img = pt.render(W, H, a.spp, seed=1, max_bounces=8)
    st = pt.stats()
    rays = st["segments"]
    return img, {"seconds_render": st["seconds_render"], "seconds_trace_closest": st["seconds_trace_closest"], "seconds_shade": st["seconds_shade"], "paths": st["paths"],
                 "closest_rays": rays, "node_visits_per_ray": st["node_visits_closest"] / max(rays, 1)}


out = {"scene": "atrium", "size": [W, H], "spp": a.spp, "max_bounces": 8}
for kind in KINDS:      # warm-up: queues, overflow slabs, clocks
    frame(kind)
if a.one:
    for kind in KINDS:
        _, out[kind] = frame(kind)
    print(json.dumps(out))
    sys.exit(0)
runs, imgs = {k: [] for k in KINDS}, {}
for _ in range(a.reps):
    for kind in KINDS:
        imgs[kind], s = frame(kind)
        runs[kind].append(s)
assert all(np.isfinite(i).all() for i in imgs.values()) and not np.array_equal(imgs["orthographic"], imgs["look_at"]) and not np.array_equal(imgs["equirect"], imgs["look_at"])
for kind, rs in runs.items():
    out[kind] = {k: (float(np.median([r[k] for r in rs])) if k.startswith(("seconds", "node")) else rs[0][k]) for k in rs[0]}
    out[kind]["seconds_render_all"] = [r["seconds_render"] for r in rs]
out["perspective_ex_over_look_at"] = out["perspective_ex"]["seconds_render"] / out["look_at"]["seconds_render"]
print(json.dumps(out, indent=1))
