"""k_trace_closest and k_trace_any (through ptc_debug_trace_closest / ptc_debug_trace_any) on a real MI355X against the float64 search of all triangles
of tests/trace_reference.py — for every path that puts a tree into HBM: the host's commit (SAH, LBVH), the commit on the device with either device
builder, the refit and the rebuild on the device after instance updates (rotation, non-uniform scale, a sheared matrix), and a pose followed by a
refit or a rebuild on the deforming scene.  Per path: 0 lost, 0 ghost, any-hit never wrong, the caps held, every solid hit within 16 x E32 of float64;
and on the same rays — aimed at interiors, edges and vertices, starting inside boxes and on box planes, with zero, negative-zero and tiny direction
components, which tests/test_gpu_parity.py::test_hit_records never sends — the oracle's bits.  Launches are ragged: 1, 63, 65 and 2048 + 37 rays; the Cornell box
adds the edges of a wave's ray ring and of a chunk, and one launch long enough for chunks of 512 handed out through the work counter.
Small scenes (at most 5,904 triangles): a test is a few launches and a numpy reference of a second or less."""
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_reference as dref  # noqa: E402
import denoise_reference as dnref  # noqa: E402
import trace_reference as tr  # noqa: E402
from test_trace_truth_host import move_instances, moved_desc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = 2048 + 37
RAGGED = (1, 63, 65)
RAGGED_RING = (64, 128, 129, 511, 512, 513)      # one scene more: the ring of prepared rays (64), twice it, and the edges of a TRACE_CHUNK
SCENES = ("cornell", "sphere", "atrium")


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _desc(pbr, scene, builder):
    d = {"cornell": pbr.scenes.cornell_box, "sphere": lambda: pbr.scenes.sphere_scene(24, 13), "atrium": lambda: pbr.scenes.atrium(0.02)}[scene]()
    d.bvh_builder = builder
    return d


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _truth_of(oracles, seed):
    """Rays (box planes of every given oracle's tree) for the scene those oracles hold, the truth of its flat_scene(), and each oracle's answers."""
    verts, idx, _ = oracles[0].flat_scene()
    pl = [tr.box_planes(o.bvh()[0]) for o in oracles]
    rays = tr.make_rays(verts, idx, (np.concatenate([p[0] for p in pl]), np.concatenate([p[1] for p in pl])), N_RAYS + 8, seed)
    rays = tuple(x[:N_RAYS] for x in rays)
    assert len(rays[0]) == N_RAYS
    truth = tr.any_all(verts, idx, rays[0], rays[1], rays[2])
    return dict(verts=verts, idx=idx, rays=rays, truth=truth, e32=tr.e32_of(verts, idx, rays[0], rays[1], truth)[:2])


@functools.lru_cache(maxsize=None)
def _case(scene, state):
    """Per scene and state ("commit", "moved"): the oracles {builder: committed (and, moved: refitted)}, {builder: a fresh commit of the moved description},
    one set of rays and its truth — computed once, shared by every path of that state."""
    import pbr_amd as pbr
    from oracle import ora

    own, fresh = {}, {}
    for b in ("sah", "lbvh"):
        d = _desc(pbr, scene, b)
        own[b] = ora.Oracle().load_scene(d)
        if state == "moved":
            move_instances(own[b], d)
            fresh[b] = ora.Oracle().load_scene(moved_desc(d))
    c = _truth_of(list(own.values()) + list(fresh.values()), seed=7 + 2 * SCENES.index(scene) + (state == "moved"))
    c.update(own=own, fresh=fresh)
    return c


def _answers(ctx, rays, n=None):
    o, d, tm = (x[:n] for x in rays[:3])
    t, prim, uv = ctx.trace_closest(o, d)
    return t, prim, uv, ctx.trace_any(o, d, tm)


def _hold(tag, pt, c, oracle, ragged=RAGGED):
    """The device's answers for the case's rays: the truth, the oracle's bits (when there is an oracle with that tree), and ragged launches."""
    ans = _answers(pt, c["rays"])
    tr.assert_true(tag, c["verts"], c["idx"], c["rays"], c["truth"], c["e32"], *ans)
    v, i, _ = pt.flat_scene()
    assert _bits(v, c["verts"]) and np.array_equal(i, c["idx"]), tag + ": the reference is not that of this state's own flat_scene()"
    if oracle is not None:
        for name, got, want in zip(("t", "prim", "uv", "occluded"), ans, _answers(oracle, c["rays"])):
            assert _bits(got, want) if got.dtype == np.float32 else np.array_equal(got, want), "%s: %s differs from the oracle's" % (tag, name)
    for n in ragged:
        for name, got, want in zip(("t", "prim", "uv", "occluded"), _answers(pt, c["rays"], n), ans):
            assert _bits(got, want[:n]) if got.dtype == np.float32 else np.array_equal(got, want[:n]), "%s: %s of a launch of %d rays" % (tag, name, n)


def _commit(gpu, d, path):
    """host-sah / host-lbvh: the host's build, uploaded; device-lbvh / device-sah: the commit on the device with that device builder."""
    where, builder = path.split("-")
    pt = gpu.PathTracer(0).set_device_builder(builder if where == "device" else "lbvh")
    if where == "host":
        os.environ["PTC_COMMIT"] = "host"
    try:
        pt.load_scene(d)
    finally:
        os.environ.pop("PTC_COMMIT", None)
    assert pt.internals()["commit_on_device"] == (where == "device"), path
    return pt


PATHS = ("host-sah", "host-lbvh", "device-lbvh", "device-sah")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("scene", SCENES)
def test_commit_paths(gpu, ora, scene, path):
    builder = path.split("-")[1]
    c = _case(scene, "commit")
    pt = _commit(gpu, _desc(gpu, scene, builder), path)
    _hold("%s %s" % (scene, path), pt, c, c["own"][builder], RAGGED + RAGGED_RING if scene == "cornell" else RAGGED)
    pt.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("scene", SCENES)
def test_refit_on_the_device_after_instance_updates(gpu, ora, scene, path):
    """The refit keeps the committed topology, so the oracle with the same tree is the oracle's own refit."""
    builder = path.split("-")[1]
    c = _case(scene, "moved")
    d = _desc(gpu, scene, builder)
    pt = move_instances(_commit(gpu, d, path), d)
    assert pt.internals()["refit_on_device"] == 1
    _hold("%s %s refit" % (scene, path), pt, c, c["own"][builder])
    pt.close()


@pytest.mark.parametrize("dev_builder", ["lbvh", "sah"])
@pytest.mark.parametrize("scene", SCENES)
def test_rebuild_on_the_device_after_instance_updates(gpu, ora, scene, dev_builder):
    """ptc_scene_rebuild makes the device builder's tree of the moved triangles: that of a fresh commit of the moved description (tests/test_gpu_parity.py and
    tests/test_gpu_device_sah.py hold the bytes), whose oracle gives the bits."""
    c = _case(scene, "moved")
    d = _desc(gpu, scene, "sah")
    pt = gpu.PathTracer(0).set_device_builder(dev_builder).load_scene(d)
    move_instances(pt, d, how="scene_rebuild")
    _hold("%s rebuild %s" % (scene, dev_builder), pt, c, c["fresh"][dev_builder])
    pt.close()


# ---- the deforming scene ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deform_case():
    import pbr_amd as pbr
    from oracle import ora

    sc = dref.scene(pbr)
    posed = dref.plain_desc(sc.desc, dref.posed_vertices(sc.desc, sc.poses["a"]))
    fresh = {b: ora.Oracle().load_scene(dataclasses.replace(posed, bvh_builder=b)) for b in ("sah", "lbvh")}
    c = _truth_of(list(fresh.values()), seed=31)
    c.update(sc=sc, fresh=fresh)
    return c


@pytest.mark.parametrize("how", ["refit", "rebuild-lbvh", "rebuild-sah"])
def test_pose_then_refit_or_rebuild(gpu, ora, how):
    """ptc_update_mesh_pose (pose "a" of tests/deform_reference.scene, evaluated by k_deform) followed by a refit — the committed tree of the rest pose around the posed
    triangles, which no oracle holds: the truth alone — or by a rebuild: the tree of a fresh commit of the posed vertices, and its oracle's bits."""
    c = _deform_case()
    sc = c["sc"]
    if how == "refit":
        pt = gpu.PathTracer(0).load_scene(sc.desc)
        dref.apply_pose(pt, sc.poses["a"]).scene_refit()
        assert pt.internals()["refit_on_device"] == 1
        oracle = None
    else:
        b = how.split("-")[1]
        pt = gpu.PathTracer(0).set_device_builder(b).load_scene(dataclasses.replace(sc.desc, bvh_builder=b))
        dref.apply_pose(pt, sc.poses["a"]).scene_rebuild()
        oracle = c["fresh"][b]
    _hold("deform pose a %s" % how, pt, c, oracle)
    pt.close()


# ---- the overflow slab of the traversal stack ----------------------------------------------------------------------------------------------
def test_two_stack_entries_in_lds(gpu, ora, tmp_path):
    """PTC_STACK_LDS=2 (read at the commit; a process of its own): the groups of pending children beyond two go through the global overflow slab.  The
    atrium's LBVH (depth 5), refitted: held against the truth and the oracle's bits, like the default stack in test_refit_on_the_device_after_instance_updates."""
    c = _case("atrium", "moved")
    rays_file, out = str(tmp_path / "rays.npz"), str(tmp_path / "child.npz")
    np.savez(rays_file, org=c["rays"][0], dirs=c["rays"][1], tmax=c["rays"][2])
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r, %r]\n"
            "import pbr_amd\nfrom test_gpu_trace_truth import _desc\nfrom test_trace_truth_host import move_instances\n"
            "d = _desc(pbr_amd, 'atrium', 'lbvh')\npt = move_instances(pbr_amd.PathTracer(0).load_scene(d), d)\n"
            "r = np.load(%r)\nt, prim, uv = pt.trace_closest(r['org'], r['dirs'])\nocc = pt.trace_any(r['org'], r['dirs'], r['tmax'])\n"
            "np.savez(%r, t=t, prim=prim, uv=uv, occ=occ, stack_lds=pt.internals()['stack_lds'], depth=pt.stats()['bvh_max_depth'])\n"
            % (ROOT, os.path.join(ROOT, "physically-based-renderer_amd"), os.path.join(ROOT, "tests"), rays_file, out))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PTC_STACK_LDS="2"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert int(got["stack_lds"]) == 2 and int(got["depth"]) >= 4
    ans = (got["t"], got["prim"], got["uv"], got["occ"])
    tr.assert_true("atrium lbvh refit, 2 stack entries in LDS", c["verts"], c["idx"], c["rays"], c["truth"], c["e32"], *ans)
    for name, a, b in zip(("t", "prim", "uv", "occluded"), ans, _answers(c["own"]["lbvh"], c["rays"])):
        assert _bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b), name


# ---- a long queue: chunks of TRACE_CHUNK rays, the later ones handed out through the work counter -------------------------------------------
def test_long_queue_hands_chunks_out_through_the_work_counter(gpu, tmp_path):
    """Every launch above is a short queue (fewer than 512 rays per wave of the grid): chunks of 64 dealt round-robin, no atomic.  Here the Cornell box is committed
    with PTC_TRACE_BLOCKS_PER_CU=1 (read at the commit; a process of its own), a grid of W = 4 waves per CU, and the case's rays are tiled to 2 * 512 * W + 37:
    at least 2 W + 1 chunks of 512 for W waves, so every wave's first chunk is its static one and the rest go through the work counter.  Every answer of both kernels
    is, bit for bit, the one this process's default-policy context gives for the same ray (test_commit_paths holds those to the truth)."""
    c = _case("cornell", "commit")
    pt = gpu.PathTracer(0).load_scene(_desc(gpu, "cornell", "sah"))
    base = _answers(pt, c["rays"])
    pt.close()
    rays_file, out = str(tmp_path / "rays.npz"), str(tmp_path / "child.npz")
    np.savez(rays_file, org=c["rays"][0], dirs=c["rays"][1], tmax=c["rays"][2])
    code = ("import sys, numpy as np, torch; sys.path[:0] = [%r, %r, %r]\n"
            "import pbr_amd\nfrom test_gpu_trace_truth import _desc\n"
            "pt = pbr_amd.PathTracer(0).load_scene(_desc(pbr_amd, 'cornell', 'sah'))\n"
            "waves = 4 * torch.cuda.get_device_properties(0).multi_processor_count\n"
            "r = np.load(%r)\nsel = np.arange(2 * 512 * waves + 37) %% len(r['org'])\n"
            "o, d, tm = (np.ascontiguousarray(r[k][sel]) for k in ('org', 'dirs', 'tmax'))\n"
            "t, prim, uv = pt.trace_closest(o, d)\nocc = pt.trace_any(o, d, tm)\n"
            "np.savez(%r, t=t, prim=prim, uv=uv, occ=occ, sel=sel, waves=waves, policy=pt.launch_policy())\n"
            % (ROOT, os.path.join(ROOT, "physically-based-renderer_amd"), os.path.join(ROOT, "tests"), rays_file, out))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PTC_TRACE_BLOCKS_PER_CU="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert " trace_blocks_per_cu=1 " in str(got["policy"]) and " chunk=512u " in str(got["policy"]), str(got["policy"])
    sel, waves = got["sel"], int(got["waves"])
    assert len(sel) == 2 * 512 * waves + 37 and -(-len(sel) // 512) > waves >= 4         # more chunks of 512 than waves: the hand-out through the counter runs
    for name, a, b in zip(("t", "prim", "uv", "occluded"), (got["t"], got["prim"], got["uv"], got["occ"]), base):
        assert len(a) == len(sel)
        assert _bits(a, b[sel]) if a.dtype == np.float32 else np.array_equal(a, b[sel]), name


# ---- the guide buffers: a full frame's camera rays -------------------------------------------------------------------------------------------
def test_guide_hits_of_a_frame(gpu):
    """Primitive, Z and barycentrics of the first-hit guides (k_raygen_guides + k_trace_closest + k_guides) of a 96 x 64 frame against the truth of the
    pixel-centre rays (denoise_reference.guide_dirs: their float32 mirror), by the same rules."""
    w, h = 96, 64
    d = dataclasses.replace(_desc(gpu, "sphere", "sah"))
    d.camera = dataclasses.replace(d.camera, aspect=w / h)
    pt = gpu.PathTracer(0).load_scene(d)
    pt.frame_begin(w, h, 1, seed=1, max_bounces=2)
    pt.frame_guides()
    prim, uv = pt.read_guide_hit()
    z = pt.read_guide(gpu.ptc.GUIDE_NORMAL_DEPTH)[..., 3]
    dirs, pos = dnref.guide_dirs(d.camera, w, h)
    org, dirs = np.ascontiguousarray(np.broadcast_to(pos, dirs.shape).reshape(-1, 3)), dirs.reshape(-1, 3)
    verts, idx, _ = pt.flat_scene()
    truth = tr.closest_all(verts, idx, org, dirs)
    e32 = tr.e32_of(verts, idx, org, dirs, truth)
    assert e32[2] > 0.3 * w * h
    rays = (org, dirs, np.ones(len(org), np.float32), np.full(len(org), tr.MISS))
    tr.assert_true("guides sphere 96x64", verts, idx, rays, truth, e32[:2], z.reshape(-1), prim.reshape(-1), uv.reshape(-1, 2), None)
    pt.close()
