#!/usr/bin/env python3
"""What punctual lights cost on the benchmark scene: the atrium at 1920x1080 with 0, 1 and 16 lights (a mix of point, spot and directional), alternating in one
process.  Per frame: ms (seconds_render of ptc_stats), seconds_shade and seconds_trace_any, shadow rays and any-hit launches.  With lights a bounce has two more
launches — k_shade_punctual and a second k_trace_any — whose time shows as the growth of seconds_shade and seconds_trace_any over the frame without lights; their
share of the frame is that growth over seconds_render.  The default 64 spp is one batch above 2^26 paths, where the kernels of a batch run one after the other
and ptc_stats has per-kernel times for the frame without lights too (below that, its any-hit launches overlap the closest-hit ones and only the frame time is
comparable).  The images are checked to be finite and the lit ones to be no darker anywhere than the unlit one; nothing is gated.
`--one N`: one warmed frame with N lights, the run to put behind `rocprofv3 --kernel-trace --stats --` for the k_shade_punctual row.
`--scene textured_atrium`: the textured benchmark scene, whose hits make the pass gather texels (the lamps stand where they stand in the atrium).
usage: python3 tools/lights_bench.py [--one N] [--spp N] [--bounces B] [--reps K] [--scene NAME]   (-> profiles/lights_1080p.txt)"""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

ap = argparse.ArgumentParser()
ap.add_argument("--one", type=int, default=None)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--bounces", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--scene", choices=["atrium", "textured_atrium"], default="atrium")
a = ap.parse_args()
W, H = 1920, 1080


def lights(n):
    """n lights inside the 40 x 12 x 20 m hall: lamps between the columns at 5 m, every third a spot pointing down and outwards, the last of 16 a sun through the roof."""
    out = []
    for i in range(n):
        x, z = -16.0 + 32.0 * ((i * 5) % 16) / 15.0, (-5.0, 0.0, 5.0)[i % 3]
        if n >= 16 and i == n - 1:
            out.append(dict(type="directional", direction=(0.3, -1.0, 0.2), intensity=(1.5, 1.4, 1.2)))
        elif i % 3 == 1:
            out.append(dict(type="spot", position=(x, 7.0, z), direction=(0.3, -1.0, 0.2), intensity=(300.0, 280.0, 240.0), cos_inner=math.cos(math.radians(25)), cos_outer=math.cos(math.radians(40)),
                            range=25.0))
        else:
            out.append(dict(type="point", position=(x, 5.0, z), intensity=(60.0, 55.0, 45.0), range=20.0))
    return out


pt = pbr.PathTracer(0).load_scene(pbr.scenes.by_name(a.scene))


def frame(n):
    pt.clear_lights()
    for l in lights(n):
        pt.add_light(l)
    img = pt.render(W, H, a.spp, seed=1, max_bounces=a.bounces)
    st = pt.stats()
    return img, {k: st[k] for k in ("seconds_render", "seconds_shade", "seconds_trace_any", "seconds_trace_closest", "shadow_rays", "launches_trace_any", "paths")}


counts = (0, 1, 16) if a.one is None else (a.one,)
out = {"scene": a.scene, "size": [W, H], "spp": a.spp, "max_bounces": a.bounces}
for n in counts:      # warm-up: queues, overflow slabs, clocks
    frame(n)
if a.one is not None:
    _, out[f"lights_{a.one}"] = frame(a.one)
    print(json.dumps(out))
    sys.exit(0)
runs, imgs = {n: [] for n in counts}, {}
for _ in range(a.reps):
    for n in counts:
        imgs[n], s = frame(n)
        runs[n].append(s)
for n in counts:
    assert np.isfinite(imgs[n]).all() and (imgs[n][..., :3] >= imgs[0][..., :3]).all()
base = None
for n in counts:
    rs = runs[n]
    res = {k: (float(np.median([r[k] for r in rs])) if k.startswith("seconds") else rs[0][k]) for k in rs[0]}
    res["ms"] = 1e3 * res["seconds_render"]
    res["ms_all"] = [1e3 * r["seconds_render"] for r in rs]
    if n == 0:
        base = res
    elif base["seconds_shade"] > 0 and base["seconds_trace_any"] > 0:      # per-kernel times exist for the frame without lights: the two new launches' time and share
        d_shade, d_any = res["seconds_shade"] - base["seconds_shade"], res["seconds_trace_any"] - base["seconds_trace_any"]
        res["punctual_shade_ms"], res["punctual_any_ms"] = 1e3 * d_shade, 1e3 * d_any
        res["new_launches_share_of_frame"] = (d_shade + d_any) / res["seconds_render"]
    res["ms_over_no_lights"] = res["seconds_render"] / base["seconds_render"]
    out[f"lights_{n}"] = res
print(json.dumps(out))
