#!/usr/bin/env python3
"""Differential fuzzing of GPU vs oracle on random scenes (the generator of tests/test_gpu_parity.py): image bits and all traversal counters; every third
scene through the LBVH builder (committed ON THE DEVICE — flatten, shading records, tree — and held byte for byte against the host's commit of the same description), every other scene moved and refitted afterwards (ptc_update_instance + ptc_scene_refit against the oracle's; the refit runs on
the device, csrc/pt_refit.hip, and its BVH units and shading tables are also held byte for byte against a host refit of the same moves on a description-only context);
every scene with two triangles or more is finally REBUILT on the device (ptc_scene_rebuild, csrc/pt_build.hip) and held, byte for byte, against a fresh host commit of the scene
as it then stands with the LBVH builder, and its image and counters against the oracle's LBVH of it.  With PTC_DEVICE_BVH=sah in the environment the device builds the
binned-SAH tree (ptc_set_device_builder): the SAH scenes commit on the device too, and every rebuild is held against a host commit with the SAH builder.
usage: python tools/fuzz_parity.py [n] [seed]"""
import importlib.util, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pbr_amd as pbr
from oracle import ora
spec = importlib.util.spec_from_file_location("tg", os.path.join(ROOT, "tests", "test_gpu_parity.py")); tg = importlib.util.module_from_spec(spec); spec.loader.exec_module(tg)
n, seed = (int(sys.argv[1]) if len(sys.argv) > 1 else 200), (int(sys.argv[2]) if len(sys.argv) > 2 else 7)
rng = np.random.default_rng(seed)
bad = 0
n_dev_refits = 0
n_rebuilds = 0
n_dev_commits = 0
n_sah_commits = n_sah_rebuilds = 0
rebuild_builder = "sah" if os.environ.get("PTC_DEVICE_BVH") == "sah" else "lbvh"      # the tree ptc_scene_rebuild makes
for k in range(n):
    if k % 50 == 0: print("scene", k, flush=True)
    d = tg._random_scene(pbr.scene, rng, k)
    d.bvh_builder = "lbvh" if k % 3 == 2 else "sah"          # every third scene through the Morton-LBVH builder
    w, h = int(rng.integers(8, 70)), int(rng.integers(8, 70))
    spp, mb, s = int(rng.integers(1, 6)), int(rng.integers(0, 9)), int(rng.integers(0, 1 << 40))
    pt, o = pbr.PathTracer(0).load_scene(d), ora.Oracle().load_scene(d)
    g, c = pt.render(w, h, spp, seed=s, max_bounces=mb), o.render(w, h, spp, seed=s, max_bounces=mb)
    ok = np.array_equal(g.view(np.uint32), c.view(np.uint32)) and all(pt.stats()[x] == o.stats()[x] for x in tg.COUNTERS)
    if not ok:
        bad += 1
        print("MISMATCH scene", k, d.bvh_builder, "pixels", int((g != c).any(-1).sum()), flush=True)
    if pt.internals()["commit_on_device"]:       # an LBVH scene on a device context flattens and builds ON THE DEVICE: the bytes of the host's commit of the same description
        n_dev_commits += 1
        n_sah_commits += pt.internals()["device_build_sah"]
        a, b = tg._scene_bytes(pt), tg._scene_bytes(pbr.PathTracer(pbr.DEVICE_NONE).load_scene(d))
        if not all(a[key].shape == b[key].shape and np.array_equal(a[key], b[key]) for key in a):
            bad += 1
            print("COMMIT MISMATCH scene", k, [key for key in a if a[key].shape != b[key].shape or not np.array_equal(a[key], b[key])], flush=True)
    moves = []
    if k % 2 == 0:          # every other scene is then moved (random new transforms for a third of its instances) and refitted on both sides
        moved = False
        host = pbr.PathTracer(pbr.DEVICE_NONE).load_scene(d)
        for i, it in enumerate(d.instances):
            if rng.random() > 0.34:
                continue
            if getattr(it, "matrix", None) is not None:
                m = np.asarray(it.matrix, np.float32).reshape(16).copy()
                m[12:15] += rng.normal(0, 0.3, 3).astype(np.float32)
                pt.update_instance(i, matrix=m); o.update_instance(i, matrix=m); host.update_instance(i, matrix=m); moves.append((i, ("m", m)))
            else:
                q = rng.normal(0, 1, 4); q /= np.linalg.norm(q)
                t = tuple(float(x) for x in np.asarray(it.t) + rng.normal(0, 0.3, 3))
                sc = tuple(float(x) for x in np.asarray(it.s) * rng.uniform(0.7, 1.4, 3))
                pt.update_instance(i, t, tuple(float(x) for x in q), sc); o.update_instance(i, t, tuple(float(x) for x in q), sc); host.update_instance(i, t, tuple(float(x) for x in q), sc)
                moves.append((i, ("t", t, tuple(float(x) for x in q), sc)))
            moved = True
        if moved:
            pt.scene_refit(); o.scene_refit()
            host.scene_refit()
            a, b = tg._scene_bytes(pt), tg._scene_bytes(host)
            n_dev_refits += pt.internals()["refit_on_device"]
            if not all(np.array_equal(a[x], b[x]) for x in a):
                bad += 1
                print("MISMATCH device refit vs host refit, scene", k, [x for x in a if not np.array_equal(a[x], b[x])], flush=True)
            g, c = pt.render(w, h, spp, seed=s, max_bounces=mb), o.render(w, h, spp, seed=s, max_bounces=mb)
            ok = np.array_equal(g.view(np.uint32), c.view(np.uint32)) and all(pt.stats()[x] == o.stats()[x] for x in tg.COUNTERS)
            if not ok:
                bad += 1
                print("MISMATCH after refit, scene", k, d.bvh_builder, "pixels", int((g != c).any(-1).sum()), flush=True)
    # the tree rebuilt on the device = the host's LBVH build of the scene as it now stands (moved or not), to the byte; image and counters = the oracle's LBVH
    if pt.stats()["n_triangles"] >= 2:
        import copy
        d2 = copy.deepcopy(d)
        d2.bvh_builder = rebuild_builder
        try:
            pt.scene_rebuild()
        except pbr.PtcError as e:
            bad += 1
            print("REBUILD FAILED scene", k, e, flush=True)
            continue
        n_rebuilds += 1
        n_sah_rebuilds += pt.internals()["device_build_sah"]
        for i, m in moves:                      # the moves, written into the description: a commit of THAT is what the rebuilt tree must equal
            if m[0] == "m":
                d2.instances[i].matrix = m[1]
            else:
                d2.instances[i].t, d2.instances[i].q_wxyz, d2.instances[i].s = m[1], m[2], m[3]
        fresh = pbr.PathTracer(pbr.DEVICE_NONE).load_scene(d2)
        o2 = ora.Oracle().load_scene(d2)
        a, b = tg._scene_bytes(pt), tg._scene_bytes(fresh)
        if not all(a[x].shape == b[x].shape and np.array_equal(a[x], b[x]) for x in a):
            bad += 1
            print(f"MISMATCH device rebuild vs host {rebuild_builder} commit, scene", k, [x for x in a if not (a[x].shape == b[x].shape and np.array_equal(a[x], b[x]))], flush=True)
        g, c = pt.render(w, h, spp, seed=s, max_bounces=mb), o2.render(w, h, spp, seed=s, max_bounces=mb)
        ok = np.array_equal(g.view(np.uint32), c.view(np.uint32)) and all(pt.stats()[x] == o2.stats()[x] for x in tg.COUNTERS)
        if not ok:
            bad += 1
            print("MISMATCH after rebuild, scene", k, "pixels", int((g != c).any(-1).sum()), flush=True)
print(f"{n} scenes, {n_dev_commits} commits on the device ({n_sah_commits} SAH), {n_dev_refits} refits on the device, {n_rebuilds} rebuilds on the device ({n_sah_rebuilds} SAH), {bad} mismatches")
sys.exit(1 if bad else 0)
