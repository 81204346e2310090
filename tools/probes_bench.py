#!/usr/bin/env python3
"""What baking light probes costs on the benchmark scene: a GRID^3 grid of probes in the atrium's bounding box at SPP samples each (default
32^3 x 1024 = 33.5 M paths) beside a camera frame of the same path count on the same context, in Mpaths/s from ptc_stats.seconds_render; and the
case that decides the accumulator's layout, few probes with many samples (64 x 65,536).  Nothing is gated; the coefficients are checked to be finite.
This tool itself reports whole frames only.  It does NOT time k_raygen_probe and k_accumulate_sh: ptc_stats has no span for them.  Their times come from a
separate run under the profiler, `rocprofv3 --kernel-trace --stats -- python3 tools/probes_bench.py --one`, whose two frames (--one-spp samples of the grid in
ONE batch, default 16, and one 64 x 65,536 frame) are read from the kernel trace by hand and set against the byte floors (64 B written per path, 16 B read per
path) in profiles/probes_atrium.txt — for those two path counts, not for the 1,024-sample bake.
usage: python3 tools/probes_bench.py [--one] [--grid G] [--spp N] [--bounces B]   (-> profiles/probes_atrium.txt)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

ap = argparse.ArgumentParser()
ap.add_argument("--one", action="store_true")
ap.add_argument("--one-spp", type=int, default=16)
ap.add_argument("--grid", type=int, default=32)
ap.add_argument("--spp", type=int, default=1024)
ap.add_argument("--bounces", type=int, default=8)
ap.add_argument("--few", type=int, nargs=2, default=(64, 65536), metavar=("PROBES", "SPP"))
a = ap.parse_args()

desc = pbr.scenes.atrium()
pt = pbr.PathTracer(0).load_scene(desc)
verts, _, _ = pt.flat_scene()
lo, hi = verts[:, 0:3].min(0).astype(np.float64), verts[:, 0:3].max(0).astype(np.float64)
cell = (hi - lo) / a.grid
g = (np.arange(a.grid) + 0.5)
zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
grid = (lo + np.stack([xx.ravel(), yy.ravel(), zz.ravel()], -1) * cell).astype(np.float32)
few = grid[np.linspace(0, len(grid) - 1, a.few[0]).astype(np.int64)]


def bake(P, spp):
    sh = pt.render_probes(P, spp, seed=3, max_bounces=a.bounces)
    st = pt.stats()
    assert np.isfinite(sh).all()
    return {"probes": len(P), "spp": spp, "paths": st["paths"], "seconds_render": st["seconds_render"], "mpaths_per_s": st["paths"] / st["seconds_render"] / 1e6,
            "segments_per_path": st["segments"] / st["paths"], "node_visits_per_closest_ray": st["node_visits_closest"] / max(st["segments"], 1),
            "mean_coef0": float(sh[:, 0].mean())}


def camera(n_paths_per_sample, spp):
    w = 1920
    h = max(1, round(n_paths_per_sample / w))
    pt.render(w, h, spp, seed=3, max_bounces=a.bounces)
    st = pt.stats()
    return {"size": [w, h], "spp": spp, "paths": st["paths"], "seconds_render": st["seconds_render"], "mpaths_per_s": st["paths"] / st["seconds_render"] / 1e6,
            "segments_per_path": st["segments"] / st["paths"], "node_visits_per_closest_ray": st["node_visits_closest"] / max(st["segments"], 1)}


out = {"scene": "atrium", "triangles": desc.n_triangles, "grid": [a.grid] * 3, "origin": lo.tolist(), "cell": cell.tolist(), "max_bounces": a.bounces}
bake(grid, 2)      # warm-up: queues, overflow slabs, clocks
if a.one:
    out["grid_one_batch"] = bake(grid, a.one_spp)
    out["few_probes"] = bake(few, a.few[1])
    print(json.dumps(out))
    sys.exit(0)
out["probe_frame"] = bake(grid, a.spp)
out["camera_frame"] = camera(len(grid), a.spp)
out["probe_over_camera_mpaths"] = out["probe_frame"]["mpaths_per_s"] / out["camera_frame"]["mpaths_per_s"]
out["few_probes"] = bake(few, a.few[1])
print(json.dumps(out))
