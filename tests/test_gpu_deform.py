"""Deforming meshes on the device (csrc/pt_deform.hip): a pose set with ptc_update_mesh_pose and applied by a refit, a rebuild or a group
refit gives — bit for bit — the object-space vertices of the numpy restatement (tests/deform_reference.py) and the scene of a fresh commit of plain meshes
that hold them; a refused pose leaves HBM alone; the temporal history survives a deformation.  The scene is deform_reference.scene: four meshes of 3, 257,
64 and 130 vertices, so every slice starts at an odd offset and the kernel runs blocks of 1, 2 and 1 partly filled waves."""
import os
import subprocess
import sys

import numpy as np
import pytest

import deform_reference as dref
from test_deform_host import ALL_KEYS, REFIT_KEYS, _bits, _same, _tables

pytestmark = pytest.mark.gpu
W, H, SPP = 64, 48, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


@pytest.fixture(scope="module")
def sc(gpu):
    return dref.scene(gpu, w=W, h=H)


@pytest.fixture(scope="module")
def ref_a(gpu, sc):
    """pose "a": the reference vertices, and a fresh commit of plain meshes that hold them — tables, image and rays, computed once"""
    verts = dref.posed_vertices(sc.desc, sc.poses["a"])
    fresh = gpu.PathTracer(0).load_scene(dref.plain_desc(sc.desc, verts))
    out = dict(verts=verts, tables=_tables(fresh), image=fresh.render(W, H, SPP, seed=3, max_bounces=4), stats=fresh.stats(), rays=_rays(), )
    out["hits"] = fresh.trace_closest(*out["rays"])
    fresh.close()
    return out


def _rays():
    rng = np.random.default_rng(11)
    o = np.tile(np.array([0.0, 0.0, 5.5], np.float32), (4096, 1)) + 0.2 * rng.standard_normal((4096, 3)).astype(np.float32)
    t = np.stack([rng.uniform(-2.2, 2.2, 4096), rng.uniform(-2.0, 2.6, 4096), rng.uniform(0.0, 1.5, 4096)], 1).astype(np.float32)
    d = t - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _posed(gpu, sc, pose="a", how="scene_refit", desc=None):
    pt = gpu.PathTracer(0).load_scene(desc or sc.desc)
    dref.apply_pose(pt, sc.poses[pose])
    getattr(pt, how)()
    return pt


def _mesh_vertices_equal(pt, verts):
    return [m for m, n in enumerate(dref.N_VERTS) if not _bits(pt.mesh_vertices(m, n), verts[m])]


def test_device_pose_and_refit_against_the_reference(gpu, sc, ref_a, tmp_path):
    pt = _posed(gpu, sc)
    assert pt.internals()["refit_on_device"] == 1
    assert _mesh_vertices_equal(pt, ref_a["verts"]) == []
    assert pt.internals()["mesh_vertices_from_device"] == 1      # read from HBM, where the kernel wrote them: not the host's evaluation
    got = _tables(pt)
    assert _same(got, ref_a["tables"], REFIT_KEYS) == []
    # the tree: a context that committed the same vertices as plain meshes, took the reference vertices through update_mesh_vertices and refitted
    base = dref.plain_desc(sc.desc, dref.posed_vertices(sc.desc, {}))
    other = gpu.PathTracer(0).load_scene(base)
    for m in range(4):
        other.update_mesh_vertices(m, np.ascontiguousarray(ref_a["verts"][m]).view(gpu.scene.MESH_VERTEX).reshape(-1))
    other.scene_refit()
    assert other.internals()["refit_on_device"] == 1
    assert _mesh_vertices_equal(other, ref_a["verts"]) == []
    assert _same(got, _tables(other), ALL_KEYS) == []
    # ... and the refit on the host, in a process of its own (PTC_REFIT is read per call)
    host = _refit_in_a_child(tmp_path, PTC_REFIT="host")
    assert int(host["on_device"]) == 0 and int(host["from_device"]) == 0
    assert _same(got, host, ALL_KEYS) == []
    assert all(_bits(host["mesh%d" % m], ref_a["verts"][m]) for m in range(4))


def _refit_in_a_child(tmp_path, **env):
    """pose "a" + ptc_scene_refit on a device context in a fresh process with `env` set: its tables, its mesh vertices, and the two internals flags"""
    out = str(tmp_path / "child.npz")
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r, %r]\n"
            "import pbr_amd, deform_reference as dref\nfrom test_deform_host import _tables\n"
            "sc = dref.scene(pbr_amd, w=%d, h=%d)\npt = pbr_amd.PathTracer(0).load_scene(sc.desc)\n"
            "dref.apply_pose(pt, sc.poses['a']).scene_refit()\n"
            "t = _tables(pt); t['on_device'] = np.array(pt.internals()['refit_on_device'])\n"
            "t.update({'mesh%%d' %% m: pt.mesh_vertices(m, n) for m, n in enumerate(dref.N_VERTS)})\n"
            "t['from_device'] = np.array(pt.internals()['mesh_vertices_from_device'])\nnp.savez(%r, **t)\n"
            % (ROOT, os.path.join(ROOT, "physically-based-renderer_amd"), os.path.join(ROOT, "tests"), W, H, out))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


def test_lds_variant_of_the_kernel_writes_the_same_bytes(gpu, sc, ref_a, tmp_path):
    """PTC_DEFORM_LDS=1 selects k_deform<true>, which stages the joint matrices in LDS (read per launch, so in a process of its own): meshes 2 (1 joint) and
    3 (70 joints, the highest index in use) take it, mesh 1 (no skin) does not.  Mesh vertices read back from HBM, flat scene and tables: the reference's bits."""
    lds = _refit_in_a_child(tmp_path, PTC_DEFORM_LDS="1")
    assert int(lds["on_device"]) == 1 and int(lds["from_device"]) == 1
    assert all(_bits(lds["mesh%d" % m], ref_a["verts"][m]) for m in range(4))
    assert _same(lds, ref_a["tables"], REFIT_KEYS) == []


@pytest.mark.parametrize("builder", ["lbvh", "sah"])
def test_pose_and_rebuild_against_a_fresh_commit(gpu, sc, ref_a, builder):
    import dataclasses

    pt = gpu.PathTracer(0).set_device_builder(builder).load_scene(dataclasses.replace(sc.desc, bvh_builder=builder))
    dref.apply_pose(pt, sc.poses["a"]).scene_rebuild()
    assert _mesh_vertices_equal(pt, ref_a["verts"]) == []
    fresh = gpu.PathTracer(0).set_device_builder(builder).load_scene(dataclasses.replace(dref.plain_desc(sc.desc, ref_a["verts"]), bvh_builder=builder))
    assert fresh.internals()["commit_on_device"] == 1 == pt.internals()["commit_on_device"]
    assert _same(_tables(pt), _tables(fresh), ALL_KEYS) == []
    assert _same(_tables(pt), ref_a["tables"], REFIT_KEYS) == []


def test_image_and_trace_parity(gpu, sc, ref_a):
    pt = _posed(gpu, sc)
    img = pt.render(W, H, SPP, seed=3, max_bounces=4)
    assert _bits(img, ref_a["image"])
    st = pt.stats()
    for k in ("paths", "segments", "shadow_rays", "hits"):
        assert st[k] == ref_a["stats"][k], k
    t, prim, uv = pt.trace_closest(*ref_a["rays"])
    t0, prim0, uv0 = ref_a["hits"]
    assert (prim0 >= 0).sum() > 500 and len(set(prim0.tolist())) > 100
    assert _bits(t, t0) and np.array_equal(prim, prim0) and _bits(uv, uv0)


def test_non_finite_pose_leaves_the_scene_alone(gpu, sc, ref_a):
    pt = _posed(gpu, sc)
    before = pt.render(W, H, SPP, seed=3, max_bounces=4)
    assert _bits(before, ref_a["image"])
    dref.apply_pose(pt, sc.poses["nonfinite"])
    rc = pt._L.ptc_scene_refit(pt._h)
    assert rc == -2 and b"non-finite" in pt._L.ptc_last_error(pt._h)
    assert _bits(pt.render(W, H, SPP, seed=3, max_bounces=4), before)
    assert _mesh_vertices_equal(pt, ref_a["verts"]) == []
    # non-finite BASE vertices are caught on the device, after the kernel has run: the slice goes back to the live pose
    dref.apply_pose(pt, {3: sc.poses["a"][3]})
    bad = np.ascontiguousarray(sc.desc.meshes[1].vertices).copy()
    bad["position"][200, 1] = np.inf
    pt.update_mesh_vertices(1, bad)
    rc = pt._L.ptc_scene_refit(pt._h)
    assert rc == -2 and b"non-finite" in pt._L.ptc_last_error(pt._h)
    assert _bits(pt.render(W, H, SPP, seed=3, max_bounces=4), before)
    assert _mesh_vertices_equal(pt, ref_a["verts"]) == []
    pt.update_mesh_vertices(1, sc.desc.meshes[1].vertices).scene_refit()      # a good base again: the scene of pose "a"
    assert _same(_tables(pt), ref_a["tables"], REFIT_KEYS) == []


def test_temporal_history_survives_a_deformation(gpu, sc):
    """Accumulate under pose "t", shift mesh 3 parallel to the image plane ("t_shifted"), refit, accumulate: both steps under the comparison rules of
    tests/test_gpu_temporal.py (16 x E32, at most 1 % of the class-1 pixels left out as fragile), and the motion buffer finds the shifted mesh's history
    where the surface was before.  The poses are smooth ones: see deform_reference.scene."""
    import temporal_reference as tref
    from test_gpu_temporal import _frame, _hold_step, _positions

    pt = _posed(gpu, sc, pose="t")
    params = dict(max_history=32, sigma_z=1.0, demodulate=1)
    cam = sc.desc.camera
    prev = None
    first_tri = np.cumsum([0] + [sc.desc.meshes[i.mesh].indices.size // 3 for i in sc.desc.instances])
    for step, seed in (("first", 1), ("deformed", 2)):
        if step == "deformed":
            dref.apply_pose(pt, sc.poses["t_shifted"]).scene_refit()
            assert pt.internals()["refit_on_device"] == 1
        tri = _positions(pt)
        rad, guides = _frame(pt, W, H, seed)
        got, _, e64 = _hold_step("deform " + step, pt, rad, guides, prev, params)
        if step == "deformed":
            prim = guides[2]
            on_moved = (prim >= first_tri[4]) & (prim < first_tri[5]) & (guides[0][..., 3] == 1)
            assert on_moved.sum() > 20
            xs = np.tile(np.arange(W, dtype=np.float32), (H, 1))
            keep = on_moved & e64["valid"]
            assert keep.sum() > 10
            assert (got["motion"][..., 2][keep] > 0).all()                              # history was found ...
            assert (np.abs(got["motion"][..., 0][keep] - xs[keep]) > 0.5).all()         # ... where the surface was BEFORE the shift
            elsewhere = (guides[0][..., 3] == 1) & ~on_moved & e64["valid"] & (prim < first_tri[3])
            assert (np.abs(got["motion"][..., 0][elsewhere] - xs[elsewhere]) < 1e-2).all()
        prev = tref.previous_state(got["history"], got["moments"], guides[1], guides[0], cam, tri)


def test_group_refit_takes_context_zeros_poses(gpu, sc, ref_a):
    g = gpu.Group([0]).load_scene(sc.desc)
    dref.apply_pose(g.ctx(0), sc.poses["a"])
    g.scene_refit()
    pt = g.ctx(0)
    assert pt.internals()["refit_on_device"] == 1
    assert _mesh_vertices_equal(pt, ref_a["verts"]) == []
    assert _same(_tables(pt), ref_a["tables"], REFIT_KEYS) == []
    assert _bits(g.render(W, H, SPP, seed=3, max_bounces=4), ref_a["image"])
    g.close()


def test_cli_poses_a_gltf_scene_before_the_commit(gpu, tmp_path):
    """ptc_render --gltf a.glb --animation N --time T poses the asset before the commit: another image than the bind pose's; an animation the asset does not
    have is an error."""
    from test_deform_host import _cylinder

    desc, nodes, skin, anim, _ = _cylinder(gpu)
    path, out = str(tmp_path / "bend.glb"), str(tmp_path / "o.pfm")
    gpu.gltf.write_glb(desc, path, nodes=(nodes, [0, 1]), skins=[skin], animations=[anim])
    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    cam = ["--cam-pos", "0", "1", "6", "--cam-target", "0", "1", "0", "--fov", "45"]
    common = [exe, "--gltf", path, "--sky", "--width", "48", "--height", "48", "--spp", "2", "--seed", "4", "--bounces", "3", "--out", out] + cam
    imgs = {}
    for name, extra in (("bind", []), ("posed", ["--animation", "0", "--time", "1.1"])):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1000:]
        with open(out, "rb") as f:
            assert f.readline().strip() == b"PF" and f.readline().split() == [b"48", b"48"]
            f.readline()
            imgs[name] = np.frombuffer(f.read(), "<f4").reshape(48, 48, 3).copy()
    assert np.isfinite(imgs["posed"]).all() and not np.array_equal(imgs["bind"], imgs["posed"])
    bad = subprocess.run(common + ["--animation", "2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "animation" in bad.stderr
    # the same pose through the Python binding, committed on a device context: the scene in HBM is the one a description-only context evaluates on the
    # host at t = 1.1 (which tests/test_deform_host.py holds against the float64 evaluation of the glTF rules), and not the bind pose
    a = gpu.gltf.Asset(path)
    got = {}
    for name, device, kw in (("device", 0, dict(animation=0, time=1.1)), ("host", gpu.DEVICE_NONE, dict(animation=0, time=1.1)), ("bind", gpu.DEVICE_NONE, {})):
        pt = gpu.PathTracer(device)
        a.load_into(pt, camera=desc.camera, **kw)
        got[name] = pt.flat_scene()[:2] + (pt.shading_tables()[0],)      # on the device context the shading records are read back from HBM
        pt.close()
    assert _bits(got["device"][0], got["host"][0]) and np.array_equal(got["device"][1], got["host"][1]) and _bits(got["device"][2], got["host"][2])
    assert got["bind"][0].shape == got["host"][0].shape and not _bits(got["bind"][0], got["host"][0])
