#!/usr/bin/env python3
"""What alpha coverage costs: a scene with MASK and BLEND materials against the SAME scene forced opaque, alternating in one process, at 1920x1080 x 1 spp (the
viewer's frame: launch-bound, where the rounds of a resolution weigh most) and at a large batch (--spp, default 64: one batch above 2^26 paths, where the kernels of a
batch run one after the other).  The scene is the textured atrium with the alpha channel of its albedo texture cut into a foliage-like pattern and its textured
materials set to MASK (cutoff 0.5) or BLEND; `--layers N` sets ptc_set_alpha_max_layers (default 8).
Per frame: ms (seconds_render of ptc_stats), seconds_alpha, the pass counters of ptc_get_alpha_stats, and the launches a bounce gains.
The rounds that pass nothing on their own: `all_covering` is the same scene with every texel alpha 255 under MASK — no ray passes a surface and the image is the opaque
scene's bit for bit (checked), so its time over the opaque frame's is what the pass costs before it lets a single ray through: the queued rounds that find their queue empty,
the lost overlap of any(b) with closest(b + 1), and the walk of every OCCLUDED shadow record to its (opaque) occluder by the closest-hit kernel (`shadow_walked`).
Nothing is gated: no threshold exists for this pass yet.
`--one NAME`: one warmed frame of `opaque`, `all_covering`, `mask` or `blend`, the run to put behind `rocprofv3 --kernel-trace --stats --` for the k_alpha_filter rows.
usage: python3 tools/alpha_bench.py [--one NAME] [--spp N] [--bounces B] [--reps K] [--layers N] [--scale S]   (-> profiles/alpha_1080p.txt)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

NAMES = ("opaque", "all_covering", "mask", "blend")
ap = argparse.ArgumentParser()
ap.add_argument("--one", choices=NAMES, default=None)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--bounces", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--scale", type=float, default=1.0)
a = ap.parse_args()
W, H = 1920, 1080


def scene(name):
    d = pbr.scenes.textured_atrium(a.scale)
    if name in ("mask", "blend"):      # holes: discs of alpha 0 (mask) or a soft ramp (blend) over a third of the albedo texture
        t = d.textures[0]
        yy, xx = np.mgrid[0:t.shape[0], 0:t.shape[1]]
        r = np.hypot((xx % 64) - 32, (yy % 64) - 32)
        t[..., 3] = np.where(r < 18, 0, 255) if name == "mask" else np.clip((r - 8) * 12, 0, 255)
    if name != "opaque":
        for m in d.materials:
            if m.tex_color >= 0 and not any(m.emissive):
                m.alpha_mode, m.alpha_cutoff = ("blend" if name == "blend" else "mask"), 0.5
    return d


tracers = {}


def frame(name, spp):
    if name not in tracers:
        tracers[name] = pbr.PathTracer(0).load_scene(scene(name))
        tracers[name].set_alpha_max_layers(a.layers)
    pt = tracers[name]
    img = pt.render(W, H, spp, seed=1, max_bounces=a.bounces)
    st, al = pt.stats(), pt.alpha_stats()
    res = {k: st[k] for k in ("seconds_render", "seconds_trace_closest", "seconds_trace_any", "seconds_shade", "launches_trace_closest", "launches_trace_any", "paths", "segments", "shadow_rays")}
    res.update(al)
    return img, res


names = NAMES if a.one is None else (a.one,)
out = {"scene": "textured_atrium", "size": [W, H], "max_bounces": a.bounces, "max_layers": a.layers}
for spp in (1, a.spp):
    for n in names:      # warm-up: queues, overflow slabs, clocks
        frame(n, spp)
    if a.one is not None:
        out[f"{a.one}_{spp}spp"] = frame(a.one, spp)[1]
        continue
    runs, imgs = {n: [] for n in names}, {}
    for _ in range(a.reps):
        for n in names:
            imgs[n], s = frame(n, spp)
            runs[n].append(s)
    assert all(np.isfinite(imgs[n]).all() for n in names)
    assert np.array_equal(imgs["opaque"].view(np.uint32), imgs["all_covering"].view(np.uint32)), "all-covering alpha is not the opaque image"
    base = None
    for n in names:
        rs = runs[n]
        res = {k: (float(np.median([r[k] for r in rs])) if k.startswith("seconds") else rs[0][k]) for k in rs[0]}
        res["ms"] = 1e3 * res["seconds_render"]
        res["ms_all"] = [1e3 * r["seconds_render"] for r in rs]
        if n == "opaque":
            base = res
        res["ms_over_opaque"] = res["seconds_render"] / base["seconds_render"]
        if n == "all_covering":
            res["nothing_passes_ms"] = res["ms"] - base["ms"]
        out[f"{n}_{spp}spp"] = res
print(json.dumps(out))
