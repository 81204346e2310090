#!/usr/bin/env python3
"""What baking a lightmap costs on the benchmark scene: the atrium's floor (instance 0, a displaced 264 x 132 grid patch whose texture coordinates
fill the unit square) into an atlas of SIZE x SIZE texels at SPP samples each (default 1024^2 x 64 = 67.1 M paths) beside a camera frame of the same path count
on the same context, in Mpaths/s from ptc_stats.seconds_render; the wall time of ptc_lightmap_begin (coverage, compaction, texel records, the owned list) and of
ptc_lightmap_read (resolve, dilation, read-back).  Nothing is gated; the atlas is checked to be finite and fully covered.
This tool itself reports whole calls only: ptc_stats has no span for the new kernels.  Their times come from a separate run under the profiler,
`rocprofv3 --kernel-trace --stats -- python3 tools/lightmap_bench.py --one`, which bakes --one-spp samples (default 16) in ONE batch; the rows of k_lm_cover,
k_lm_texels, k_raygen_texel, k_lm_first_hit, k_lm_scatter and k_lm_dilate are read from the kernel trace by hand and set against their byte floors in
profiles/lightmap_atrium.txt.
usage: python3 tools/lightmap_bench.py [--one] [--size N] [--spp N] [--bounces B] [--instance I]   (-> profiles/lightmap_atrium.txt)"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

ap = argparse.ArgumentParser()
ap.add_argument("--one", action="store_true")
ap.add_argument("--one-spp", type=int, default=16)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--bounces", type=int, default=8)
ap.add_argument("--instance", type=int, default=0)
ap.add_argument("--dilate", type=int, default=2)
a = ap.parse_args()

desc = pbr.scenes.atrium()
pt = pbr.PathTracer(0).load_scene(desc)


def bake(size, spp):
    t0 = time.perf_counter()
    pt.lightmap_begin(a.instance, size, size, spp, seed=3, max_bounces=a.bounces)
    t1 = time.perf_counter()
    pt.frame_add_samples(spp)
    pt.sync()
    t2 = time.perf_counter()
    atlas, back = pt.read_lightmap(dilate=a.dilate, with_backface=True)
    t3 = time.perf_counter()
    st = pt.stats()
    n, dropped = pt.lightmap_texel_count()
    assert np.isfinite(atlas).all()
    return {"atlas": [size, size], "texels": n, "dropped": dropped, "spp": spp, "paths": st["paths"], "seconds_render": st["seconds_render"],
            "mpaths_per_s": st["paths"] / st["seconds_render"] / 1e6, "segments_per_path": st["segments"] / st["paths"],
            "node_visits_per_closest_ray": st["node_visits_closest"] / max(st["segments"], 1), "seconds_begin_wall": t1 - t0, "seconds_samples_wall": t2 - t1,
            "seconds_read_wall": t3 - t2, "baked_fraction": float((atlas[..., 3] == 1).mean()), "invalid_entries": int((back > 0.1).sum()),
            "mean_irradiance": atlas[..., :3][atlas[..., 3] == 1].mean(0).tolist()}


def camera(n_paths_per_sample, spp):
    w = 1920
    h = max(1, round(n_paths_per_sample / w))
    pt.render(w, h, spp, seed=3, max_bounces=a.bounces)
    st = pt.stats()
    return {"size": [w, h], "spp": spp, "paths": st["paths"], "seconds_render": st["seconds_render"], "mpaths_per_s": st["paths"] / st["seconds_render"] / 1e6,
            "segments_per_path": st["segments"] / st["paths"], "node_visits_per_closest_ray": st["node_visits_closest"] / max(st["segments"], 1)}


m = desc.meshes[desc.instances[a.instance].mesh]
out = {"scene": "atrium", "triangles": desc.n_triangles, "instance": a.instance, "instance_triangles": int(m.indices.size // 3), "max_bounces": a.bounces, "dilate": a.dilate}
bake(a.size, 2)      # warm-up: queues, overflow slabs, the lightmap's buffers, clocks
if a.one:
    out["one_batch"] = bake(a.size, a.one_spp)
    print(json.dumps(out))
    sys.exit(0)
out["lightmap_frame"] = bake(a.size, a.spp)
out["camera_frame"] = camera(out["lightmap_frame"]["texels"], a.spp)
out["lightmap_over_camera_mpaths"] = out["lightmap_frame"]["mpaths_per_s"] / out["camera_frame"]["mpaths_per_s"]
print(json.dumps(out))
