#!/usr/bin/env python3
"""How far a refit carries: the viewer turns its nodes without bound (src/gltf_viewer/App.cpp:306-313).  A third of the atrium's instances is turned about +Y by
theta = 0 .. pi; per angle, node visits per closest-hit / shadow ray, the tree's surface-area cost (ptc_stats.bvh_sa_cost) and the frame rate of
  refit    the tree of the commit (SAH builder), refitted on the device (ptc_scene_refit)
  rebuild  a new LBVH built on the device from the moved vertices (ptc_scene_rebuild, csrc/pt_build.hip)
  rebuild (SAH)  the same with the SAH device builder (ptc_set_device_builder): the binned-SAH tree built on the device — the fresh commit's tree, byte for byte
  commit   a fresh ptc_scene_commit of the moved description with the SAH builder (the host build: what a rebuild policy could fall back to)
The counters are the oracle's (tests hold them bit for bit), so this is the curve tools/tree_quality.py would give, in seconds instead of hours.
usage: python3 tools/refit_curve.py [w h spp]"""
import copy, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

w, h, spp = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (960, 540, 8)
angles = [0.0] + [math.pi / k for k in (64, 32, 16, 8, 6, 4, 3, 2)] + [math.pi * 3 / 4, math.pi]
base = pbr.scenes.by_name("atrium")
movers = [i for i, it in enumerate(base.instances) if i % 3 == 0 and getattr(it, "matrix", None) is None]


def turned(theta):
    d = copy.deepcopy(base)
    for i in movers:
        d.instances[i].q_wxyz = (math.cos(theta / 2), 0.0, math.sin(theta / 2), 0.0)
    return d


def measure(pt):
    t0 = time.time()
    pt.render(w, h, spp, seed=3, max_bounces=8)
    s = pt.stats()
    return {"visits_closest": s["node_visits_closest"] / s["segments"], "visits_any": s["node_visits_any"] / max(1, s["shadow_rays"]),
            "tris_closest": s["tri_tests_closest"] / s["segments"], "sa_cost": s["bvh_sa_cost"], "sa_cost_built": s["bvh_sa_cost_built"],
            "mpaths_s": s["paths"] / s["seconds_render"] / 1e6, "nodes": s["n_bvh_nodes"]}


refit_pt = pbr.PathTracer(0).load_scene(base)          # SAH commit, then only refits
rebuild_pt = pbr.PathTracer(0).load_scene(base)        # SAH commit, then a device rebuild per angle
sah_pt = pbr.PathTracer(0).set_device_builder("sah").load_scene(base)      # SAH commit on the device, then a device SAH rebuild per angle
print(f"atrium {refit_pt.stats()['n_triangles']} triangles, {len(movers)} of {len(base.instances)} instances turned about +Y; {w}x{h}x{spp} spp per point")
print(f"{'theta':>6} | {'refit: visits c/a':>18} {'cost':>7} {'ratio':>6} {'Mp/s':>6} | {'rebuild (LBVH, device)':>22} {'cost':>7} {'Mp/s':>6} {'ms':>5} | {'fresh SAH commit':>17} {'cost':>7} {'Mp/s':>6} {'ms':>6} | {'rebuild (SAH, device)':>21} {'Mp/s':>6} {'ms':>5}")
rows = []
for theta in angles:
    d = turned(theta)
    for i in movers:
        refit_pt.update_instance(i, d.instances[i].t, d.instances[i].q_wxyz, d.instances[i].s)
        rebuild_pt.update_instance(i, d.instances[i].t, d.instances[i].q_wxyz, d.instances[i].s)
        sah_pt.update_instance(i, d.instances[i].t, d.instances[i].q_wxyz, d.instances[i].s)
    refit_pt.scene_refit()
    a = measure(refit_pt)
    rebuild_pt.scene_rebuild()
    b = measure(rebuild_pt); b["ms"] = rebuild_pt.stats()["seconds_rebuild"] * 1e3
    fresh = pbr.PathTracer(0).load_scene(d)
    c = measure(fresh); c["ms"] = fresh.stats()["seconds_commit"] * 1e3
    fresh.close()
    sah_pt.scene_rebuild()
    e = measure(sah_pt); e["ms"] = sah_pt.stats()["seconds_rebuild"] * 1e3
    rows.append({"theta": theta, "refit": a, "rebuild": b, "commit": c, "rebuild_sah": e})
    print(f"{theta:6.3f} | {a['visits_closest']:8.2f} /{a['visits_any']:8.2f} {a['sa_cost']:7.2f} {a['sa_cost'] / a['sa_cost_built']:6.2f} {a['mpaths_s']:6.0f} | "
          f"{b['visits_closest']:10.2f} /{b['visits_any']:9.2f} {b['sa_cost']:7.2f} {b['mpaths_s']:6.0f} {b['ms']:5.2f} | {c['visits_closest']:7.2f} /{c['visits_any']:8.2f} {c['sa_cost']:7.2f} {c['mpaths_s']:6.0f} {c['ms']:6.1f} | "
          f"{e['visits_closest']:10.2f} /{e['visits_any']:8.2f} {e['mpaths_s']:6.0f} {e['ms']:5.2f}")
print(json.dumps(rows))
