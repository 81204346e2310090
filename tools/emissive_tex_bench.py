#!/usr/bin/env python3
"""What textured emission costs on the benchmark scene: the atrium at 1920x1080 with its ceiling panels as plain emitters (material 5, the scene as it is) and with
the same panels as textured emitters — base emission 0, an emission texture and the panels' radiance as its factor — alternating in one process on two contexts.
The texture is a 64 x 64 checkerboard of white and `--dark` (default 255: all white, so both scenes hold the same light and the images must agree).  Per frame: ms
(seconds_render of ptc_stats), seconds_shade and seconds_trace_any, shadow rays and any-hit launches; for the textured frame the pass's own seconds
(ptc_get_emissive_tex_stats), its share of the frame and the extra any-hit launches.  With the panels textured k_shade no longer samples them (the emitter table is
empty) and k_shade_emissive_tex does: a bounce has one more kernel and the same number of any-hit launches.  `--both`: the panels stay plain emitters AND a second,
textured set of panels hangs 0.5 m below them, so a bounce has the pass on top of everything it had: one more kernel, one more scan and one more any-hit launch.
The default 64 spp is one batch above 2^26 paths, where the kernels of a batch run one after the other and ptc_stats has per-kernel times.  The images are checked
to be finite and, all white, to agree in the mean within 1 %; nothing is gated.
usage: python3 tools/emissive_tex_bench.py [--spp N] [--bounces B] [--reps K] [--dark V] [--both]   (-> profiles/emissive_tex_1080p.txt)"""
import argparse, copy, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--bounces", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--dark", type=int, default=255)
ap.add_argument("--both", action="store_true")
a = ap.parse_args()
W, H = 1920, 1080
plain = pbr.scenes.atrium()
PANELS = [k for k, m in enumerate(plain.materials) if any(float(x) > 0.0 for x in m.emissive)]      # the atrium's emitter material: the one with a non-zero emissive
assert len(PANELS) == 1, PANELS
PANELS = PANELS[0]
tex = np.full((64, 64, 4), 255, np.uint8)
tex[::2, 1::2, :3] = a.dark
tex[1::2, ::2, :3] = a.dark
textured = copy.deepcopy(plain)
textured.textures = list(textured.textures) + [tex]
radiance = tuple(float(x) for x in plain.materials[PANELS].emissive)
em = pbr.scene.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (0.0, 0.0, 0.0), emissive_texture=len(textured.textures) - 1, emissive_texture_factor=radiance)
if a.both:      # a second set of panels, textured, half a metre below the plain ones
    textured.materials.append(em)
    for it in [it for it in plain.instances if plain.meshes[it.mesh].material == PANELS]:
        m = copy.deepcopy(plain.meshes[it.mesh])
        m.material = len(textured.materials) - 1
        m.vertices = m.vertices.copy()
        m.vertices["position"][:, 1] -= 0.5
        textured.meshes.append(m)
        textured.instances.append(pbr.scene.InstanceDesc(len(textured.meshes) - 1, it.t, it.q_wxyz, it.s, it.matrix))
else:
    textured.materials[PANELS] = em

ctx = {"plain": pbr.PathTracer(0).load_scene(plain), "textured": pbr.PathTracer(0).load_scene(textured)}


def frame(which):
    pt = ctx[which]
    img = pt.render(W, H, a.spp, seed=1, max_bounces=a.bounces)
    st = pt.stats()
    s = {k: st[k] for k in ("seconds_render", "seconds_shade", "seconds_trace_any", "seconds_trace_closest", "shadow_rays", "launches_trace_any", "n_emitters", "paths")}
    e = pt.emissive_tex_stats()
    s.update(entries=e["entries"], hit_additions=e["hit_additions"], shadow_records=e["shadow_records"], seconds_emissive_tex=e["seconds_emissive_tex"])
    return img, s


out = {"scene": "atrium", "size": [W, H], "spp": a.spp, "max_bounces": a.bounces, "dark": a.dark, "both": a.both}
for which in ctx:      # warm-up: queues, overflow slabs, clocks
    frame(which)
runs, imgs = {k: [] for k in ctx}, {}
for _ in range(a.reps):
    for which in ctx:
        imgs[which], s = frame(which)
        runs[which].append(s)
for which in ctx:
    assert np.isfinite(imgs[which]).all()
    rs = runs[which]
    res = {k: (float(np.median([r[k] for r in rs])) if k.startswith("seconds") else rs[0][k]) for k in rs[0]}
    res["ms"] = 1e3 * res["seconds_render"]
    res["ms_all"] = [1e3 * r["seconds_render"] for r in rs]
    res["mean_radiance"] = float(imgs[which][..., :3].mean())
    out[which] = res
t, p = out["textured"], out["plain"]
t["ms_over_plain"] = t["seconds_render"] / p["seconds_render"]
t["pass_share_of_frame"] = t["seconds_emissive_tex"] / t["seconds_render"]
t["extra_any_hit_launches"] = t["launches_trace_any"] - p["launches_trace_any"]
if a.dark == 255 and not a.both:
    assert abs(t["mean_radiance"] / p["mean_radiance"] - 1.0) < 0.01, (t["mean_radiance"], p["mean_radiance"])
print(json.dumps(out))
