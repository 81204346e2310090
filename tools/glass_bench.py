#!/usr/bin/env python3
"""What dielectric transmission costs: the atrium with glass against the SAME scene with transmission 0, alternating in one process, at 1920x1080 x 1 spp (the
viewer's frame: launch-bound, where the rounds of a resolution weigh most) and at a large batch (--spp, default 64).
  plain   the atrium as it is: no transmissive material, no pass
  empty   the atrium plus one tiny thin pane behind the back wall, where no ray arrives: the pass runs and every round finds its queue empty — the cost of the
          queued rounds and of the lost overlap of any(b) with closest(b + 1) on their own
  glass   the dielectric columns as thin-walled glass tubes and the arches as solid glass with Beer attenuation (transmission 1, ior 1.5)
Per frame: ms (seconds_render of ptc_stats), seconds_glass and the counters of ptc_get_glass_stats.  `--interactions N` sets ptc_set_glass_max_interactions (default 8).
Nothing is gated: no threshold exists for this pass yet.
`--shadows`: transparent shadows (ptc_set_glass_shadows) instead: the same frames of `empty` and `glass`, each with a `sun` (a directional light, so that
the punctual pass has shadow records too), with the feature off and on — `empty` shows the queued rounds of the shadow walk alone (its hidden pane is thin, so the
walk runs and walks nothing), `glass` the walk at work; per frame also the counters of ptc_get_glass_shadow_stats.  (-> profiles/glass_shadows_1080p.txt)
`--one NAME`: one warmed frame, the run to put behind `rocprofv3 --kernel-trace --stats --` for the k_glass_filter rows.
usage: python3 tools/glass_bench.py [--shadows] [--one NAME] [--spp N] [--bounces B] [--reps K] [--interactions N] [--scale S]   (-> profiles/glass_1080p.txt)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

NAMES = ("plain", "empty", "glass")
ap = argparse.ArgumentParser()
ap.add_argument("--one", choices=NAMES, default=None)
ap.add_argument("--shadows", action="store_true")
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--bounces", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--interactions", type=int, default=8)
ap.add_argument("--scale", type=float, default=1.0)
a = ap.parse_args()
W, H = 1920, 1080


def scene(name):
    d = pbr.scenes.atrium(a.scale)
    S = pbr.scene
    if name == "empty":
        d.materials.append(S.Material((1.0, 1.0, 1.0, 1.0), 0.0, 0.2, transmission=1.0))
        d.meshes.append(S.MeshDesc(*pbr.scenes._quad((0.0, 1.0, -10.02), (0.01, 1.0, -10.02), (0.01, 1.01, -10.02), (0.0, 1.01, -10.02)), len(d.materials) - 1))
        d.instances.append(S.InstanceDesc(len(d.meshes) - 1))
    if name == "glass":
        d.materials[2].transmission, d.materials[2].thin_walled = 1.0, True
        m = d.materials[3]
        m.transmission, m.thin_walled, m.attenuation_color, m.attenuation_distance = 1.0, False, (0.6, 0.85, 0.9), 0.3
    if a.shadows:
        d.lights = [dict(type="sun", direction=(0.3, -1.0, 0.2), intensity=(3.0, 2.8, 2.5))]
    return d


tracers = {}


def frame(name, spp, shadows=False):
    if (name, shadows) not in tracers:
        tracers[name, shadows] = pbr.PathTracer(0).set_glass_shadows(shadows).load_scene(scene(name))
        tracers[name, shadows].set_glass_max_interactions(a.interactions)
    pt = tracers[name, shadows]
    img = pt.render(W, H, spp, seed=1, max_bounces=a.bounces)
    st, gl = pt.stats(), pt.glass_stats()
    res = {k: st[k] for k in ("seconds_render", "seconds_trace_closest", "seconds_trace_any", "seconds_shade", "launches_trace_closest", "launches_trace_any", "paths", "segments", "shadow_rays")}
    res.update(gl)
    if a.shadows:
        res.update({"shadow_" + k: v for k, v in pt.glass_shadow_stats().items()})
    return img, res


def shadows_rows():
    """--shadows: empty and glass, each off and on, alternating; ms on / off per scene."""
    out = {"scene": "atrium + sun", "size": [W, H], "max_bounces": a.bounces, "max_interactions": a.interactions}
    cases = [(n, on) for n in ("empty", "glass") for on in (False, True)]
    for spp in (1, a.spp):
        for n, on in cases:
            frame(n, spp, on)
        runs = {c: [] for c in cases}
        for _ in range(a.reps):
            for c in cases:
                img, s = frame(c[0], spp, c[1])
                assert np.isfinite(img).all()
                runs[c].append(s)
        for n, on in cases:
            rs = runs[n, on]
            res = {k: (float(np.median([r[k] for r in rs])) if k.startswith("seconds") else rs[0][k]) for k in rs[0]}
            res["ms"] = 1e3 * res["seconds_render"]
            res["ms_all"] = [1e3 * r["seconds_render"] for r in rs]
            off = out.get(f"{n}_off_{spp}spp", res)
            res["ms_over_off"] = res["ms"] / off["ms"]
            out[f"{n}_{'on' if on else 'off'}_{spp}spp"] = res
            print(f"{n:6s} shadows {'on ' if on else 'off'} {spp:4d} spp  ms {res['ms']:9.3f}  (all: {' '.join('%.3f' % x for x in res['ms_all'])})  x off {res['ms_over_off']:5.2f}  seconds_glass {res['seconds_glass']:8.5f}  "
                  f"walked {res['shadow_walked']:10d}  passes {res['shadow_passes']:10d}  visible {res['shadow_visible']:10d}  exhausted {res['shadow_exhausted']:8d}")
        assert out[f"empty_on_{spp}spp"]["shadow_passes"] == 0, "a shadow record reached the hidden pane"
    print(json.dumps(out))


if a.shadows:
    shadows_rows()
    sys.exit(0)


names = NAMES if a.one is None else (a.one,)
out = {"scene": "atrium", "size": [W, H], "max_bounces": a.bounces, "max_interactions": a.interactions}
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
    assert runs["empty"][0]["reflections"] + runs["empty"][0]["refractions"] == 0, "a ray reached the hidden pane"
    base = None
    for n in names:
        rs = runs[n]
        res = {k: (float(np.median([r[k] for r in rs])) if k.startswith("seconds") else rs[0][k]) for k in rs[0]}
        res["ms"] = 1e3 * res["seconds_render"]
        res["ms_all"] = [1e3 * r["seconds_render"] for r in rs]
        if n == "plain":
            base = res
        res["ms_over_plain"] = res["seconds_render"] / base["seconds_render"]
        if n == "empty":
            res["empty_rounds_ms"] = res["ms"] - base["ms"]
        out[f"{n}_{spp}spp"] = res
    for n in names:
        r = out[f"{n}_{spp}spp"]
        print(f"{n:8s} {spp:4d} spp  ms {r['ms']:9.3f}  (all: {' '.join('%.3f' % x for x in r['ms_all'])})  x plain {r['ms_over_plain']:5.2f}  seconds_glass {r['seconds_glass']:8.5f}  "
              f"reflections {r['reflections']:10d}  refractions {r['refractions']:10d}  standing {r['standing']:10d}  exhausted {r['exhausted']:8d}"
              + (f"  empty_rounds_ms {r['empty_rounds_ms']:.3f}" if n == "empty" else ""))
print(json.dumps(out))
